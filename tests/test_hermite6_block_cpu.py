"""6th-order Hermite with individual block time steps, without a GPU: the NumPy oracle
(oracle.simulate_hermite6_block) against the shared-step oracle and on a tight binary among 254
other bodies, the native CPU engine against it, checkpoints, the refusals and the CLI.

The engine inputs are Plummer spheres (64 bodies seed 9, 200 bodies seed 4), softening 1e9 m,
dt = 8 d, eta = 0.25, 32 d: the oracle takes 143 and 254 block steps on them (1493 and 5959
body-steps, deepest levels 8 and 7). The seeds are those of 1..12 whose level decisions lean
furthest from a threshold (oracle.level_lean 1.4e-3 and 1.6e-4 of a level), so no decision is
marginal under the rounding differences between the engines.
"""
import functools
import json
import math
import subprocess
import sys

import numpy as np
import pytest

from gravsim.config import G_SI, SimConfig
from gravsim.models import initial_conditions as ic
from gravsim.models.initial_conditions import BodySet
from gravsim.ops import oracle
from gravsim.parallel import comm
from gravsim.runtime.hermite import HermiteCpuEngine
from gravsim.runtime.simulation import Simulation
from gravsim.utils import checkpoint as ckpt

DAY = 86400.0
DT, ETA, SOFT = 8 * DAY, 0.25, 1e9
INPUTS = {64: 9, 200: 4}
STEPS = {64: (143, 1493), 200: (254, 5959)}  # block steps, body-steps over 32 d


def bodies(n):
    return ic.plummer(n, seed=INPUTS[n])


def cfg_for(n, **kw):
    kw.setdefault("t_end", 32 * DAY)
    return SimConfig(n=n, dt=DT, steps=1000, dtype="fp64", device="cpu", integrator="hermite",
                     hermite_order=6, eta=ETA, softening=SOFT, block_steps6=True, **kw)


@functools.lru_cache(maxsize=None)
def oracle_run(n):
    b = bodies(n)
    stats = {}
    out = oracle.simulate_hermite6_block(b.pos, b.vel, b.mass, DT, 32 * DAY, ETA, softening=SOFT,
                                         stats=stats)
    for y in out[:3]:
        y.setflags(write=False)
    return out + (stats,)


# ---- 1. oracle ----------------------------------------------------------------------------
def test_level_0_is_the_shared_fixed_step_bit_for_bit():
    """max_level = 0: every body steps by dt, and the block scheme is simulate_hermite6."""
    b = ic.solar_random(100, 3)
    dt, K = 3600.0, 6
    x, v, lev, log, clamped = oracle.simulate_hermite6_block(b.pos, b.vel, b.mass, dt, K * dt,
                                                             ETA, max_level=0)
    rx, rv, _, t, taken = oracle.simulate_hermite6(b.pos, b.vel, b.mass, dt, K)
    assert np.array_equal(x, rx) and np.array_equal(v, rv)
    assert taken == [dt] * K and log == [(k, 100) for k in range(1, K + 1)]
    assert not lev.any() and t == K * dt


def test_rows_entry_is_the_full_entry():
    b = ic.solar_random(300, 5)
    a0 = oracle.acc_jerk_snap(b.pos, b.vel, np.zeros_like(b.pos), b.mass)[0]
    full = oracle.acc_jerk_snap(b.pos, b.vel, a0, b.mass)
    idx = np.random.default_rng(2).permutation(300)[:77]
    rows = oracle.acc_jerk_snap_rows(b.pos, b.vel, a0, b.mass, idx)
    for r, f in zip(rows, full):
        assert np.array_equal(r, f[idx])
    a1, j1, s1 = (y + 1e-3 * np.abs(y).max() for y in full)
    h = np.full(300, 50.0)
    want, valid = oracle.hermite6_dt_bodies(*full, a1, j1, s1, h, ETA)
    assert valid.all() and want.min() == oracle.hermite6_dt(*full, a1, j1, s1, 50.0, ETA)


def test_oracle_refusals():
    b = bodies(64)
    for kw in (dict(eta=0.0), dict(t_end=DT * 1.5), dict(max_level=41), dict(max_level=-1),
               dict(levels=np.full(64, 25)), dict(levels=np.ones(64, int), body_times=np.ones(64))):
        args = dict(dt=DT, t_end=2 * DT, eta=ETA)
        args.update(kw)
        with pytest.raises(ValueError):
            oracle.simulate_hermite6_block(b.pos, b.vel, b.mass, softening=SOFT, **args)


def test_oracle_schedule_from_a_given_block_state():
    """Massless bodies moving at 1 m/s, levels and body times given: a = j = s = c = 0, no level
    changes, and the run is the integer schedule, exact (what tests/test_hermite6_block_gpu.py
    holds the device chain to at 20,000 bodies)."""
    n, L = 40, 3
    i = np.arange(n)
    lev = (i % 4).astype(np.int32)
    tb = ((i // 4) % (1 << lev)) * (1 << (L - lev))
    pos, vel = np.zeros((n, 3)), np.zeros((n, 3))
    pos[:, 0], vel[:, 0] = i, 1.0
    x, v, out_lev, log, clamped = oracle.simulate_hermite6_block(
        pos, vel, np.zeros(n), 8.0, 8.0, ETA, max_level=L, levels=lev, body_times=tb)
    assert np.array_equal(x[:, 0], i + (8 - tb)) and np.array_equal(v, vel)
    assert np.array_equal(out_lev, lev) and clamped == 0
    t, stp, want = tb.astype(np.int64).copy(), np.int64(1) << (L - lev).astype(np.int64), []
    while t.min() < 8:
        nxt = int((t + stp).min())
        due = t + stp == nxt
        t[due] = nxt
        want.append((nxt, int(due.sum())))
    assert log == want and [t for t, _ in log] == list(range(1, 9))


COM = np.array([1.5e11, 0.7e11, -0.3e11])
COM_V = np.array([0.0, 3e4, 0.0])


def binary_case():
    """256 solar+random bodies (seed 1) with bodies 3 and 4 replaced by two bodies of 6e24 kg on
    a circular orbit 1e7 m apart about a centre of mass at COM moving at 30 km/s:
    (bodies, period)."""
    b = ic.solar_random(256, 1)
    m, sep = 6e24, 1e7
    v = math.sqrt(G_SI * 2 * m / sep)
    b.pos[3], b.pos[4] = COM + [sep / 2, 0, 0], COM - [sep / 2, 0, 0]
    b.vel[3], b.vel[4] = COM_V + [0, v / 2, 0], COM_V - [0, v / 2, 0]
    b.mass[3] = b.mass[4] = m
    return b, 2 * math.pi * math.sqrt(sep ** 3 / (G_SI * 2 * m))


def relative_orbit_energy(b, pos, vel):
    r, v = pos[4] - pos[3], vel[4] - vel[3]
    return 0.5 * (v * v).sum() - G_SI * (b.mass[3] + b.mass[4]) / math.sqrt((r * r).sum())


def total_energy(b, pos, vel):
    _, phi = oracle.accelerations(pos, b.mass, with_potential=True)
    return 0.5 * (b.mass * (vel ** 2).sum(1)).sum() + 0.5 * (b.mass * phi).sum()


def test_binary_among_256_bodies():
    """Two periods in 16 macro steps of period / 8. Order 6 at eta 0.25 holds the relative orbit
    better than order 4 at its customary eta 0.02 with no more body-steps. On this input:
    order 6: 66 block steps, 4196 body-steps, binary at level 2, dE/E 2.0e-10, relative orbit
    2.2e-7; order 4: 132 block steps, 4328 body-steps, level 3, 1.5e-9, 1.6e-6."""
    b, period = binary_case()
    dt = period / 8
    e0, r0 = total_energy(b, b.pos, b.vel), relative_orbit_energy(b, b.pos, b.vel)
    seen, out = [], {}

    def check(tb, lev):
        seen.append(bool((tb % (np.int64(1) << (24 - lev).astype(np.int64)) == 0).all()))

    for order, eta, run in ((6, 0.25, oracle.simulate_hermite6_block),
                            (4, 0.02, oracle.simulate_hermite_block)):
        stats = {}
        x, v, lev, log, clamped = run(b.pos, b.vel, b.mass, dt, 16 * dt, eta, stats=stats,
                                      check=check if order == 6 else None)
        out[order] = dict(block_steps=len(log), body_steps=sum(m for _, m in log),
                          level=int(lev[3]), clamped=clamped, level_max=stats["level_max"],
                          dE=abs(total_energy(b, x, v) - e0) / abs(e0),
                          dE_rel=abs(relative_orbit_energy(b, x, v) - r0) / abs(r0))
        print(f"order {order} block, eta {eta}: {out[order]}")
        assert log[-1][0] == 16 << 24 and lev[3] == lev[4]
    assert all(seen) and len(seen) == out[6]["block_steps"]
    assert out[6]["clamped"] == 0 and out[6]["level_max"] < 24
    assert out[6]["dE_rel"] < out[4]["dE_rel"]
    assert out[6]["body_steps"] <= out[4]["body_steps"]


# ---- 2. CPU engine ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 200])
def test_cpu_engine_matches_oracle(n):
    """The (t_ticks, n_active) log and the levels exactly, positions to 1e-10 of max |x| (the
    gate of the fp64 order-6 chain, docs/DESIGN.md section 21)."""
    x, v, lev, log, clamped, stats = oracle_run(n)
    assert (len(log), sum(m for _, m in log)) == STEPS[n] and clamped == 0
    assert stats["lean"] >= 1e-4
    eng = HermiteCpuEngine(cfg_for(n).validate())
    eng.load(bodies(n))
    eng.step(4)
    st, got = eng.status(), eng.state()
    err = np.abs(got.pos - x).max() / np.abs(x).max()
    print(f"n={n}: {st.block_steps} block steps, position error {err:.2e} of max |x|")
    assert eng.block_log == log
    assert err <= 1e-10
    assert np.array_equal(eng.levels(), lev) and (eng.body_times() == 4 << 24).all()
    assert (st.block_steps, st.body_steps) == STEPS[n] and st.steps == 4
    assert st.time == 32 * DAY and st.finished and st.level_max == stats["level_max"]
    assert st.level_clamped == 0
    eng.step(3)  # past t_end: nothing happens
    assert eng.status() == st


def test_checkpoint_mid_run_resumes_bit_exact(tmp_path):
    cfg = cfg_for(64, t_end=None).replace(steps=2)
    sim = Simulation(cfg)
    sim.engine.load(bodies(64))
    sim.run()
    path = str(tmp_path / "c.gsck")
    sim.save_checkpoint(path)
    c = ckpt.load(path)
    assert c.meta["block_steps"] and c.meta["hermite_order"] == 6 and c.meta["time"] == 2 * DT
    assert all(k in c.extra for k in ("acc", "jerk", "snap", "crackle", "level"))
    assert np.array_equal(c.extra["level"][:, 0], sim.engine.levels())
    sim.run(2)
    ref, ref_lev, ref_c = sim.global_state(), sim.engine.levels(), sim.engine.carried()
    sim2 = Simulation(cfg.replace(resume=path))
    assert np.array_equal(sim2.engine.levels(), c.extra["level"][:, 0])
    m = sim2.run(2)
    got = sim2.global_state()
    assert np.array_equal(got.pos, ref.pos) and np.array_equal(got.vel, ref.vel)
    assert np.array_equal(sim2.engine.levels(), ref_lev)
    assert all(np.array_equal(p, q) for p, q in zip(sim2.engine.carried(), ref_c))
    assert sim2.step == 4 and m.time_reached == 4 * DT and m.steps == 2
    assert m.block_steps > 2 and m.pair_evals == m.body_steps * 64 and m.hermite_order == 6


# ---- 3. refusals and the CLI ----------------------------------------------------------------
def test_refusals():
    ok = dict(integrator="hermite", hermite_order=6, eta=ETA, block_steps6=True, dt=100.0,
              dtype="fp64")
    SimConfig(**ok, t_end=300.0).validate()
    # order 4's option keeps refusing order 6 and names the one that runs; order 4 has no use
    # for the new one
    with pytest.raises(ValueError, match="--block-steps6"):
        SimConfig(**dict(ok, block_steps6=False, block_steps=True)).validate()
    with pytest.raises(ValueError, match="order 6"):
        SimConfig(**dict(ok, hermite_order=4, eta=0.02)).validate()
    with pytest.raises(ValueError, match="fp64 only"):
        SimConfig(**dict(ok, dtype="fp32")).validate()
    with pytest.raises(ValueError, match="collisions"):
        SimConfig(**ok, collisions="detect").validate()
    with pytest.raises(ValueError, match="mixed"):
        SimConfig(**dict(ok, dtype="mixed")).validate()
    with pytest.raises(ValueError, match="one rank"):
        SimConfig(**ok, gpus=2, device="gpu").validate()
    for kw in (dict(ok, eta=0.0), dict(ok, t_end=250.0), dict(ok, max_level=41)):
        with pytest.raises(ValueError):
            SimConfig(**kw).validate()
    with pytest.raises(ValueError, match="fp64 only"):
        HermiteCpuEngine(SimConfig(n=8, device="cpu", **dict(ok, dtype="fp32")))
    with pytest.raises(ValueError, match="one rank"):
        Simulation(SimConfig(n=64, device="cpu", **ok), comm.DistInfo(rank=1, world=2))


def test_cli_block_steps_metrics(tmp_path):
    out = tmp_path / "m.jsonl"
    root = str(__import__("pathlib").Path(__file__).resolve().parent.parent)
    base = [sys.executable, "-m", "gravsim", "--n", "64", "--init", "plummer", "--integrator",
            "hermite", "--hermite-order", "6", "--eta", "0.25", "--block-steps6", "--max-level",
            "20", "--dt", str(DT), "--softening", "1e9", "--steps", "2", "--device", "cpu",
            "--quiet", "--log-format", "none"]
    r = subprocess.run(base + ["--dtype", "fp64", "--metrics-json", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    m = json.loads(out.read_text().splitlines()[-1])
    assert m["hermite_order"] == 6 and m["steps"] == 2 and m["time_reached"] == 2 * DT
    assert m["block_steps"] > 2 and m["body_steps"] >= 2 * 64
    assert m["pair_evals"] == m["body_steps"] * 64 and 0 < m["level_max"] <= 20
    assert m["level_clamped"] == 0
    r = subprocess.run(base + ["--dtype", "fp32"], capture_output=True, text=True, timeout=300,
                       cwd=root)
    assert r.returncode != 0 and "fp64 only" in r.stderr
