"""Shared-step Hermite across ranks on the GPU: P ranks give the one-rank run bit for bit.

The one-process tests use the virtual group (runtime/hermite.py HermiteVirtualGroup: the slice
kernels, the control kernel and the schedule of the RCCL path, the gathers as device copies) with
chunk 1024, the smallest shapes that still have uneven slices, a part-ghost last unit and
j-chunks of another rank: 2049 bodies are 3 units of 1024 rows (P = 2, 3), 4097 are 5 (P = 2, 3,
5), 3000 have a last unit of 952 real rows. The reference of every test is the one-rank engine,
run once per configuration and shared; "equal" is always bitwise. The RCCL tests run one process
per rank, on one GPU over loopback sockets (and on distinct GPUs where there are that many).
"""
import ctypes
import functools
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from gravsim.config import G_SI, SimConfig
from gravsim.models import initial_conditions as ic
from gravsim.models.initial_conditions import BodySet
from gravsim.parallel.partition import hermite_partition
from gravsim.runtime.hermite import HermiteHipEngine, HermiteVirtualGroup
from gravsim.utils import checkpoint as ckpt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ["fp32", "fp64", "mixed"]
SHAPES = [(2049, 2), (2049, 3), (4097, 2), (4097, 3), (4097, 5), (3000, 2), (3000, 3)]
ARRAYS = ("pos", "vel", "acc", "jerk")
DT = 4e5


def _cfg(n, dtype, **kw):
    kw.setdefault("dt", DT)
    return SimConfig(n=n, dtype=dtype, device="gpu", integrator="hermite", chunk=1024,
                     **kw).validate()


def _snap(eng):
    """State, carried derivatives and the control block of an engine or a group."""
    st = eng.status()
    s = eng.state()
    a, j = eng.carried()
    return dict(pos=s.pos, vel=s.vel, acc=a, jerk=j, mass=s.mass, t=st.time, steps=st.steps,
                dt_last=st.dt_last, dt_next=st.dt_next, dt_min=st.dt_min, finished=st.finished)


def _same(got, ref, keys=("t", "steps", "dt_last", "dt_next", "dt_min", "finished")):
    for k in ARRAYS:
        assert np.array_equal(got[k], ref[k]), k
    for k in keys:
        assert got[k] == ref[k], (k, got[k], ref[k])


@functools.lru_cache(maxsize=None)
def _bodies(n, seed=7):
    return ic.solar_random(n, seed)


def _run(make, b, steps, **load):
    eng = make()
    try:
        eng.load(b, **load)
        eng.step(steps)
        return _snap(eng)
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _one_rank(n, dtype, steps, eta=0.0, t_end=None):
    cfg = _cfg(n, dtype, eta=eta, t_end=t_end)
    return _run(lambda: HermiteHipEngine(cfg), _bodies(n), steps)


# ---- 1. fixed step ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,P", SHAPES)
def test_fixed_step_equals_one_rank(hip, n, P, dtype):
    ref = _one_rank(n, dtype, 6)
    got = _run(lambda: HermiteVirtualGroup(_cfg(n, dtype), P), _bodies(n), 6)
    assert ref["steps"] == 6 and ref["t"] == 6 * DT
    _same(got, ref)


# ---- 2. adaptive step, an end time that cuts the last step -------------------------------------
@functools.lru_cache(maxsize=None)
def _cut_end(n, dtype, k=5):
    """An end time inside step k of the adaptive run: half of the step it would take."""
    cfg = _cfg(n, dtype, eta=0.02)
    s = _run(lambda: HermiteHipEngine(cfg), _bodies(n), k - 1)
    assert 0 < s["dt_next"] < DT
    return s["t"] + 0.5 * s["dt_next"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,P", [(4097, 3), (4097, 5), (3000, 2)])
def test_adaptive_step_and_end_time(hip, n, P, dtype):
    t_end = _cut_end(n, dtype)
    enq = 5 + 20  # (20 chains past the end: no-ops that still gather)
    ref = _one_rank(n, dtype, enq, eta=0.02, t_end=t_end)
    assert ref["finished"] and ref["steps"] == 5 and ref["t"] == t_end
    assert ref["dt_min"] < DT  # (adaptive steps; the fifth was cut to end inside it)
    grp = HermiteVirtualGroup(_cfg(n, dtype, eta=0.02, t_end=t_end), P)
    try:
        grp.load(_bodies(n))
        grp.step(enq)
        got = _snap(grp)
        sts = grp.statuses()
    finally:
        grp.close()
    _same(got, ref)
    assert all(s == sts[0] for s in sts)  # every shard's control block is the same


# ---- 3. a planted pair fixes the step, wherever it lives ----------------------------------------
def _bind(b, i, j, sep):
    """Make bodies i, j a circular binary of separation sep at i's place."""
    u, t = np.array([0.6, 0.0, 0.8]), np.array([0.0, 1.0, 0.0])
    b.pos[j] = b.pos[i] + sep * u
    b.vel[j] = b.vel[i] + math.sqrt(G_SI * (b.mass[i] + b.mass[j]) / sep) * t


@pytest.mark.parametrize("where", ["last rank's last rows", "rank 0's first unit"])
@pytest.mark.parametrize("dtype", ["fp64", "mixed"])
def test_planted_pair_fixes_the_step_on_every_shard(hip, dtype, where):
    n, P = 3000, 3
    b = _bodies(n).copy()
    _bind(b, 1023, 1024, 1e8)  # a pair that straddles the first slice cut
    loose = b.copy()
    i = n - 2 if where.startswith("last") else 10
    _bind(b, i, i + 1, 1e6)
    assert hermite_partition(n, 1024, P, P - 1) == (2048, 1024) and n - 2 >= 2048

    def steps_of(make, bodies):
        eng = make()
        try:
            eng.load(bodies)
            out = []
            for _ in range(3):
                eng.step(1)
                sts = eng.statuses() if hasattr(eng, "statuses") else [eng.status()]
                out.append([(s.dt_last, s.time, s.steps) for s in sts])
            return out
        finally:
            eng.close()

    cfg = _cfg(n, dtype, eta=0.02)
    ref = steps_of(lambda: HermiteHipEngine(cfg), b)
    base = steps_of(lambda: HermiteHipEngine(cfg), loose)
    got = steps_of(lambda: HermiteVirtualGroup(cfg, P), b)
    for k in range(3):
        assert ref[k][0][0] < 0.25 * base[k][0][0]  # the planted pair sets the minimum
        assert got[k] == ref[k] * P  # h, t and steps of every shard are the one-rank values


# ---- 4. derivatives -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,P", [(3000, 3), (2049, 2)])
def test_derivs_through_the_group(hip, n, P, dtype):
    b = _bodies(n).copy()
    b.pos -= b.pos[0]  # the Sun at the origin, where the ghost rows are: with softening (and no
    cfg = _cfg(n, dtype, softening=1e9, cutoff=0.0)  # cutoff) those pairs are not zeroed by law

    def derivs(make):
        eng = make()
        try:
            eng.load(b)
            first = eng.derivs()
            eng.step(2)  # (then every rank's x, v are current in its own rows only)
            return first + eng.derivs()
        finally:
            eng.close()

    ref = derivs(lambda: HermiteHipEngine(cfg))
    got = derivs(lambda: HermiteVirtualGroup(cfg, P))
    assert np.all(ref[0][:, 3] < 0) and not np.array_equal(ref[0], ref[2])
    for g, r in zip(got, ref):  # a, j and phi at the start and after two steps
        assert g.shape == (n, 4) and np.array_equal(g, r)


# ---- 5. launch shapes ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_launch_shapes_give_the_same_bits(hip, dtype):
    n, P = 4097, 3
    ref = _one_rank(n, dtype, 3, eta=0.02)
    for ipl in ((1, 2) if dtype == "fp64" else (1, 2, 4)):
        for groups in (1, 2, 5):
            grp = HermiteVirtualGroup(_cfg(n, dtype, eta=0.02, ipl=ipl, split_groups=groups), P)
            try:
                lay = [e.native_layout for e in grp.shards]
                assert all(x["ipl"] == ipl and x["split_groups"] == groups for x in lay)
                grp.load(_bodies(n))
                grp.step(3)
                _same(_snap(grp), ref)
            finally:
                grp.close()


# ---- 6. refusals and layout ---------------------------------------------------------------------
def test_refusals_and_layout(hip):
    from gravsim.runtime.engines import _gs_config

    with pytest.raises(ValueError, match="unit"):
        HermiteVirtualGroup(_cfg(1024, "fp32"), 2)
    c = _gs_config(_cfg(1024, "fp32"), 0, 2, 0)  # ... and the native object itself
    h = ctypes.c_void_p()
    assert hip.gs_hermite_create(ctypes.byref(c), ctypes.byref(h)) != 0 and not h.value
    assert b"more ranks than units" in hip.gs_last_error()
    for kw in (dict(eta=0.02, block_steps=True), dict(collisions="detect")):
        with pytest.raises(ValueError, match="one rank"):
            HermiteHipEngine(_cfg(4097, "fp32", **kw), 0, 2)
    n, P = 4097, 3
    grp = HermiteVirtualGroup(_cfg(n, "fp32"), P, order=[1, 0, 2])
    try:
        for e in grp.shards:
            e.load(_bodies(n))
        with pytest.raises(RuntimeError, match="out of order"):
            grp.step(1)
        # a shard's layout reports its slice
        for r, e in enumerate(grp.shards):
            begin, rows = hermite_partition(n, 1024, P, r)
            lay = e.native_layout
            assert (lay["local_begin"], lay["n_local"], lay["n_pad"]) == (begin, rows, 5120)
            assert (e.layout.local_begin, e.layout.n_local) == (begin, rows)
        assert [e.layout.n_local for e in grp.shards] == [2048, 2048, 1024]
        assert grp.shards[2].layout.real_local == range(4096, 4097)
        # a lone rank of three has nobody to gather from
        with pytest.raises(RuntimeError, match="communicator"):
            grp.shards[0].step(1)
    finally:
        grp.close()


# ---- 7. state through the group, checkpoints across rank counts ---------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_carried_state_and_checkpoints_continue_bit_for_bit(hip, tmp_path, dtype):
    n = 4097
    cfg = _cfg(n, dtype, eta=0.02)
    ref = _one_rank(n, dtype, 6, eta=0.02)
    mid = _one_rank(n, dtype, 3, eta=0.02)
    carry = dict(acc=mid["acc"], jerk=mid["jerk"], t=mid["t"], dt_next=mid["dt_next"],
                 dt_min=mid["dt_min"])
    keys = ("t", "dt_last", "dt_next", "dt_min")  # (the step count restarts with the state)
    b = BodySet(mid["pos"], mid["vel"], mid["mass"])
    _same(_run(lambda: HermiteVirtualGroup(cfg, 3), b, 3, **carry), ref, keys)
    # a checkpoint written at P = 3 after 3 steps, resumed on one rank and on two
    grp = HermiteVirtualGroup(cfg, 3)
    try:
        grp.load(_bodies(n))
        grp.step(3)
        s = _snap(grp)
    finally:
        grp.close()
    _same(s, mid)
    path = ckpt.save(str(tmp_path / "p3.gsck"), BodySet(s["pos"], s["vel"], s["mass"]), 3,
                     dict(time=s["t"], dt_next=s["dt_next"], dt_min=s["dt_min"]),
                     {"acc": s["acc"], "jerk": s["jerk"]})
    c = ckpt.load(path)
    carry = dict(acc=c.extra["acc"], jerk=c.extra["jerk"], t=c.meta["time"],
                 dt_next=c.meta["dt_next"], dt_min=c.meta["dt_min"])
    _same(_run(lambda: HermiteHipEngine(cfg), c.bodies, 3, **carry), ref, keys)
    _same(_run(lambda: HermiteVirtualGroup(cfg, 2), c.bodies, 3, **carry), ref, keys)


# ---- 8, 9. real RCCL ----------------------------------------------------------------------------
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


RCCL_N, RCCL_STEPS = 4097, 5


def _rccl_worker(rank, world, port, out_dir, devices):
    env = dict(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
               WORLD_SIZE=str(world), LOCAL_RANK=str(rank) if devices else "0")
    os.environ.update(env)
    if devices:
        os.environ.pop("GRAVSIM_RCCL_RANK_HOSTS", None)
    else:  # one "host" per rank: RCCL's socket transport over loopback (tests/test_rccl_gpu.py)
        os.environ["GRAVSIM_RCCL_RANK_HOSTS"] = "1"
    status = "started"
    try:
        import gravsim  # noqa: F401
        from gravsim.parallel import comm
        from gravsim.runtime.engines import HipEngine

        dist = comm.init(timeout_s=120)
        try:
            cfg = _cfg(RCCL_N, "mixed", eta=0.02)
            eng = HermiteHipEngine(cfg, rank, world, device=rank if devices else 0, dist=dist)
            uid = comm.broadcast_bytes(dist, HipEngine.unique_id() if rank == 0 else None)
            eng.comm_init(uid)
            eng.set_step_timeout(60.0)
            info = eng.comm_info()
            assert (info["rccl_nranks"], info["rccl_rank"]) == (world, rank), info
            eng.load(_bodies(RCCL_N))
            eng.step(RCCL_STEPS)
            eng.sync()
            eng.comm_check()
            s = _snap(eng)
            a4, j4 = eng.derivs()
            np.savez(os.path.join(out_dir, f"rank{rank}.npz"), a4=a4, j4=j4,
                     **{k: np.asarray(v) for k, v in s.items()})
            eng.close()
            status = "ok"
        finally:
            comm.shutdown(dist)
    except BaseException as e:  # noqa: BLE001 - the parent reads the reason from the file
        status = f"{type(e).__name__}: {e}"
        raise
    finally:
        with open(os.path.join(out_dir, f"status{rank}.txt"), "w") as f:
            f.write(status)


def _rccl_run_and_check(tmp_path, world, devices):
    import torch.multiprocessing as mp

    ctx = mp.start_processes(_rccl_worker, args=(world, _port(), str(tmp_path), devices),
                             nprocs=world, start_method="spawn", join=False)
    import time

    deadline, done = time.monotonic() + 170, False
    try:
        # (join returns when any rank exits, True once all have; it raises if one failed)
        while not done and time.monotonic() < deadline:
            done = ctx.join(timeout=max(0.1, deadline - time.monotonic()))
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
    status = [(tmp_path / f"status{r}.txt").read_text() if (tmp_path / f"status{r}.txt").exists()
              else "no status" for r in range(world)]
    assert done and status == ["ok"] * world, status
    cfg = _cfg(RCCL_N, "mixed", eta=0.02)
    eng = HermiteHipEngine(cfg)
    try:
        eng.load(_bodies(RCCL_N))
        eng.step(RCCL_STEPS)
        ref = _snap(eng)
        a4, j4 = eng.derivs()
    finally:
        eng.close()
    assert ref["steps"] == RCCL_STEPS and ref["dt_min"] < DT
    for r in range(world):  # every rank returns all rows and holds the same control block
        got = np.load(tmp_path / f"rank{r}.npz")
        for k in ARRAYS:
            assert np.array_equal(got[k], ref[k]), (r, k)
        for k in ("t", "steps", "dt_last", "dt_next", "dt_min"):
            assert got[k] == ref[k], (r, k)
        assert np.array_equal(got["a4"], a4) and np.array_equal(got["j4"], j4)


@pytest.mark.parametrize("world", [2, 3])
def test_rccl_ranks_on_one_gpu_equal_one_rank(hip, tmp_path, world):
    """P processes over RCCL (P = 2: an uneven split 3 + 2 units, grouped broadcasts; P = 3:
    2 + 2 + 1) against the one-rank engine. Most of the time is process and RCCL start-up."""
    _rccl_run_and_check(tmp_path, world, devices=False)


def test_rccl_ranks_on_distinct_gpus_equal_one_rank(hip, tmp_path):
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 visible GPUs")
    _rccl_run_and_check(tmp_path, 2, devices=True)


# ---- 10. the CLI end to end ---------------------------------------------------------------------
def test_cli_two_ranks_write_the_one_rank_dump(hip, tmp_path):
    import json

    env = dict(os.environ, PYTHONPATH=ROOT, GRAVSIM_RCCL_RANK_HOSTS="1")
    args = ["-m", "gravsim", "--num-bodies", "4097", "--chunk", "1024", "--steps", "6",
            "--integrator", "hermite", "--eta", "0.02", "--dt", str(DT), "--dtype", "mixed",
            "--device", "gpu", "--quiet", "--diagnostics", "--checkpoint-every", "6"]
    out = {}
    for name, extra in (("one", []), ("two", ["--gpus", "2"])):
        txt, ckd, mj = (tmp_path / f"{name}.{e}" for e in ("txt", "ck", "json"))
        # (one run: the text dump, and the state with its carried a, j as a checkpoint)
        subprocess.run([sys.executable, *args, *extra, "--dump", str(txt), "--checkpoint-dir",
                        str(ckd), "--metrics-json", str(mj)], cwd=ROOT, env=env, check=True,
                       timeout=170)
        out[name] = (txt.read_text(), ckpt.load(ckpt.latest(str(ckd))),
                     json.loads(mj.read_text().splitlines()[-1]))
    (t1, c1, m1), (t2, c2, m2) = out["one"], out["two"]
    assert t1 == t2 and t1.count("Particle ") == 4097
    assert np.array_equal(c1.bodies.pos, c2.bodies.pos)
    assert np.array_equal(c1.bodies.vel, c2.bodies.vel)
    assert all(np.array_equal(c1.extra[k], c2.extra[k]) for k in ("acc", "jerk"))
    assert all(c1.meta[k] == c2.meta[k] for k in ("time", "dt_next", "dt_min"))
    assert (m1["nranks"], m2["nranks"]) == (1, 2) and m1["steps_taken"] == m2["steps_taken"] == 6
    assert m1["time_reached"] == m2["time_reached"]
    # the conserved quantities come from the gathered rows in the one-rank order
    k1, k2 = m1["extra"]["conservation"], m2["extra"]["conservation"]
    assert k1["energy_start"] == k2["energy_start"] and k1["energy_end"] == k2["energy_end"]
