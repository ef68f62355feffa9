"""Hermite with individual block time steps, without a GPU: the NumPy oracle's invariants, the
native CPU engine against it, the indexed acceleration+jerk entry, checkpoints, refusals, the
level cap, and the energy and work the scheme is for.

The two inputs are Plummer spheres (64 bodies seed 5, 200 bodies seed 9), softening 1e9 m,
dt = 8 d, eta = 0.02. The oracle takes 232 and 403 block steps over 32 d on them (1459 and 6268
body-steps), and the (t, n_active) sequence is the same under relative position perturbations of
1e-15, 1e-13 and 1e-7.
"""
import ctypes
import functools
import json
import subprocess
import sys

import numpy as np
import pytest

from gravsim.config import G_SI, SimConfig
from gravsim.models import initial_conditions as ic
from gravsim.ops import _native, oracle
from gravsim.parallel import comm
from gravsim.parallel.partition import layout
from gravsim.runtime.hermite import HermiteCpuEngine
from gravsim.runtime.simulation import Simulation
from gravsim.utils import checkpoint as ckpt

import test_hermite_block_sched_gpu as sched  # (its 700-body input and oracle run; no GPU needed)

DAY = 86400.0
DT, ETA, SOFT = 8 * DAY, 0.02, 1e9
INPUTS = {64: 5, 200: 9}
STEPS = {64: (232, 1459), 200: (403, 6268)}  # block steps, body-steps over 32 d


def bodies(n):
    return ic.plummer(n, seed=INPUTS[n])


def cfg_for(n, **kw):
    kw.setdefault("t_end", 32 * DAY)
    return SimConfig(n=n, dt=DT, steps=1000, dtype="fp64", device="cpu", integrator="hermite",
                     eta=ETA, softening=SOFT, block_steps=True, **kw)


@functools.lru_cache(maxsize=None)
def oracle_run(n, days=32, rel=0.0):
    b = bodies(n)
    pos = b.pos
    if rel:
        pos = pos * (1.0 + rel * np.random.default_rng(1).uniform(-1, 1, pos.shape))
    seen = []

    def check(tb, lev):
        step = np.int64(1) << (24 - lev).astype(np.int64)
        seen.append(bool((tb % step == 0).all()))

    out = oracle.simulate_hermite_block(pos, b.vel, b.mass, DT, days * DAY, ETA,
                                        softening=SOFT, check=check)
    return out + (seen,)


def energy(b, pos, vel):
    """Total energy with the softened potential, the bodies' own -mu / eps terms left out."""
    _, phi = oracle.accelerations(pos, b.mass, softening=SOFT, with_potential=True)
    phi = phi + G_SI * b.mass / SOFT
    return 0.5 * (b.mass * (vel ** 2).sum(1)).sum() + 0.5 * (b.mass * phi).sum()


def drift(b, pos, vel):
    e0 = energy(b, b.pos, b.vel)
    return abs(energy(b, pos, vel) - e0) / abs(e0)


# ---- 1. oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 200])
def test_oracle_invariants(n):
    x, v, lev, log, clamped, seen = oracle_run(n)
    assert all(seen) and len(seen) == len(log)   # tb_i is a multiple of body i's step, always
    assert log[-1][0] == 4 << 24                 # all bodies end on t_end ...
    assert [m for t, m in log if t % (1 << 24) == 0] == [n] * 4  # ... and meet at every dt
    assert any(m == n for _, m in log)
    assert (len(log), sum(m for _, m in log)) == STEPS[n]
    assert clamped == 0 and 0 <= lev.min() and lev.max() <= 24
    assert [t for t, _ in log] == sorted({t for t, _ in log})
    for rel in (1e-15, 1e-13, 1e-7):
        assert oracle_run(n, rel=rel)[3] == log, rel


def test_oracle_refusals():
    b = bodies(64)
    for kw in (dict(eta=0.0), dict(t_end=DT * 1.5), dict(max_level=41), dict(max_level=-1)):
        args = dict(dt=DT, t_end=2 * DT, eta=ETA)
        args.update(kw)
        with pytest.raises(ValueError):
            oracle.simulate_hermite_block(b.pos, b.vel, b.mass, softening=SOFT, **args)


# ---- 1b. oracle: sparse sources, vectorised level rule, a given block state ----------------
def sparse_input(n=300):
    """Test particles (ic.tracer_particles) with the massive bodies at 0, 255, 256, 257, n - 1
    and two moons of the last one that go deep."""
    tau = lambda e: 2 * DT * 2.0 ** -e / np.sqrt(ETA)  # noqa: E731
    return ic.tracer_particles(n, 5, moons=((-1, 1, tau(8.5), 1.0), (-1, n - 10, tau(6.5), 1.0)))


def test_sparse_sources_match_the_dense_sums():
    """A column with mu = 0 adds +-0 to every row, and NumPy adds the columns of a row in order,
    so the sums over the sources alone may even be the same bits; the gate is what a changed
    order could do, 4 n 2^-53 sum |terms| per component."""
    n = 300
    b, src = sparse_input(n)
    assert (b.mass[src] > 0).all() and not np.delete(b.mass, src).any() and len(src) == 5
    da, dj, dphi, sa, sj = oracle.acc_jerk(b.pos, b.vel, b.mass, with_potential=True,
                                           with_abs=True)
    tol = 4 * n * 2.0 ** -53
    a, j, phi = oracle.acc_jerk(b.pos, b.vel, b.mass, with_potential=True, sources=src)
    assert (np.abs(a - da) <= tol * sa).all() and (np.abs(j - dj) <= tol * sj).all()
    assert (np.abs(phi - dphi) <= tol * np.abs(dphi)).all()
    idx = np.random.default_rng(3).permutation(n)[:77]
    ra, rj = oracle.acc_jerk_rows(b.pos, b.vel, b.mass, idx, sources=src)
    assert (np.abs(ra - da[idx]) <= tol * sa[idx]).all()
    assert (np.abs(rj - dj[idx]) <= tol * sj[idx]).all()
    assert np.array_equal(ra, a[idx]) and np.array_equal(rj, j[idx])  # (same columns, same order)


def test_sparse_block_run_matches_the_dense_run():
    """Two macro steps of dt = 16 d with max_level 8. Positions: every evaluation may differ by
    tol sum |terms| of the acceleration, and x answers an acceleration error e held over the
    time T by at most e T^2 / 2, times the growth of a perturbation over the run, 58 on the moons
    of this family (measured in tests/test_hermite_block_sched_gpu.py)."""
    n, dt = 300, 2 * DT
    b, src = sparse_input(n)
    sd, ss = {}, {}
    dense = oracle.simulate_hermite_block(b.pos, b.vel, b.mass, dt, 2 * dt, ETA, max_level=8,
                                          stats=sd)
    sparse = oracle.simulate_hermite_block(b.pos, b.vel, b.mass, dt, 2 * dt, ETA, max_level=8,
                                           sources=src, stats=ss)
    assert sparse[3] == dense[3] and sparse[4] == dense[4] > 0
    assert np.array_equal(sparse[2], dense[2]) and len(np.unique(dense[2])) >= 4
    assert len(dense[3]) == 512 and ss["level_max"] == sd["level_max"] == 8
    assert all(np.array_equal(p, q) for p, q in zip(ss["active"], sd["active"]))
    assert min(ss["lean"], sd["lean"]) >= 1e-9
    sa = oracle.acc_jerk(b.pos, b.vel, b.mass, with_abs=True)[2]
    tol = 4 * n * 2.0 ** -53 * sa.max() * (2 * dt) ** 2 / 2 * 58
    err = np.abs(sparse[0] - dense[0]).max()
    print(f"sparse against dense: {err:.3e} m, bound {tol:.3e} m")
    assert err <= tol


def test_sources_refuse_a_massive_body_outside_them():
    b, src = sparse_input()
    for bad in (src[1:], src[:-1], []):
        with pytest.raises(ValueError, match="mass"):
            oracle.acc_jerk_rows(b.pos, b.vel, b.mass, [0, 1], sources=bad)
        with pytest.raises(ValueError, match="mass"):
            oracle.acc_jerk(b.pos, b.vel, b.mass, sources=bad)
        with pytest.raises(ValueError, match="mass"):
            oracle.simulate_hermite_block(b.pos, b.vel, b.mass, DT, DT, ETA, sources=bad)
    with pytest.raises(ValueError, match="range"):
        oracle.acc_jerk(b.pos, b.vel, b.mass, sources=list(src) + [b.n])
    # massless bodies among the sources are fine
    a, _ = oracle.acc_jerk(b.pos, b.vel, b.mass, sources=list(src) + [7])
    assert np.array_equal(a, oracle.acc_jerk(b.pos, b.vel, b.mass, sources=src)[0])


def test_vectorised_level_rule_is_the_scalar_rule():
    """Random inputs that take every branch: invalid, halvings (one, several, into the cap),
    the doubling (allowed and not by t_next, and refused at level 0), and staying."""
    rng = np.random.default_rng(11)
    dt, seen = 100.0, set()
    for L in (0, 1, 5, 24):
        m = 4000
        k = rng.integers(0, L + 1, m).astype(np.int32)
        want = np.ldexp(dt, -k) * 2.0 ** rng.uniform(-4, 3, m)
        on = rng.random(m) < 0.1  # (exactly on a threshold)
        want[on] = np.ldexp(dt, -k[on]) * rng.choice([0.5, 1.0, 2.0], int(on.sum()))
        want[::50], want[1::50] = np.nan, np.inf
        valid = np.isfinite(want) & (rng.random(m) < 0.9)
        for t_next in (1 << L, 3 << max(L - 2, 0), 5, 1 << max(L - 1, 0)):
            new, hit = oracle.block_new_levels(k, want, valid, t_next, dt, L)
            assert new.dtype == np.int32 and hit.dtype == bool
            for i in range(m):
                r = oracle.block_new_level(int(k[i]), want[i], bool(valid[i]), t_next, dt, L)
                assert (int(new[i]), bool(hit[i])) == r, (L, i, k[i], want[i], t_next)
                seen.add("invalid" if not valid[i] else "clamped" if r[1] else
                         "down%d" % min(r[0] - k[i], 2) if r[0] > k[i] else
                         "up" if r[0] < k[i] else
                         "held" if k[i] > 0 and want[i] >= 2 * np.ldexp(dt, -int(k[i])) else "stay")
    assert seen == {"invalid", "clamped", "down1", "down2", "up", "held", "stay"}
    a = rng.normal(size=(500, 3))
    j = rng.normal(size=(500, 3)) * 10.0 ** rng.uniform(-3, 3, (500, 1))
    j[::25] = 0
    for L in (0, 3, 24):
        lev = oracle.block_first_levels(a, j, dt, ETA, L)
        for i in range(500):
            an, jn = np.sqrt((a[i] ** 2).sum()), np.sqrt((j[i] ** 2).sum())
            k = 0
            while jn > 0 and k < L and np.ldexp(dt, -k) > 0.5 * ETA * an / jn:
                k += 1
            assert lev[i] == k


def test_oracle_starts_from_a_given_block_state():
    """Massless bodies moving at 1 m/s, levels and body times given: the run is the integer
    schedule, exact."""
    n, L = 40, 3
    i = np.arange(n)
    lev = (i % 4).astype(np.int32)
    tb = ((i // 4) % (1 << lev)) * (1 << (L - lev))
    pos, vel = np.zeros((n, 3)), np.zeros((n, 3))
    pos[:, 0], vel[:, 0] = i, 1.0
    x, v, out_lev, log, clamped = oracle.simulate_hermite_block(
        pos, vel, np.zeros(n), 8.0, 8.0, ETA, max_level=L, sources=[], levels=lev, body_times=tb)
    assert np.array_equal(x[:, 0], i + (8 - tb)) and np.array_equal(v, vel)
    assert np.array_equal(out_lev, lev) and clamped == 0
    assert [t for t, _ in log] == list(range(1, 9))
    assert sum(m for _, m in log) == int(((8 - tb) >> (L - lev)).sum())
    for kw in (dict(levels=lev + 1), dict(levels=lev, body_times=tb + 1),
               dict(levels=lev[:-1]), dict(levels=lev, body_times=-tb - 8)):
        with pytest.raises(ValueError, match="block state"):
            oracle.simulate_hermite_block(pos, vel, np.zeros(n), 8.0, 8.0, ETA, max_level=L, **kw)


# ---- 2. CPU engine ------------------------------------------------------------------------
def test_cpu_engine_matches_the_sparse_oracle():
    """The 700-body input of tests/test_hermite_block_sched_gpu.py (active sets of 3 to 5 bodies
    spread over the whole index range, 768 clamped steps, one macro step of 256 block steps); the
    assertions and the gate of test_cpu_engine_matches_oracle (the oracle's response to a
    perturbation of 1e-13 is 5.8e-12 here: within the gate's condition, see there)."""
    n = 700
    b, src = sched.family(n)
    x, v, lev, log, clamped, stats = sched._oracle_run(n)
    eng = HermiteCpuEngine(SimConfig(n=n, dt=sched.DT, steps=10, dtype="fp64", device="cpu",
                                     integrator="hermite", eta=ETA, block_steps=True,
                                     max_level=sched.LMAX, t_end=sched.DT).validate())
    eng.load(b)
    eng.step(1)
    st, got = eng.status(), eng.state()
    assert eng.block_log == log
    assert np.abs(got.pos - x).max() / np.abs(x).max() <= 1e-10
    assert np.array_equal(eng.levels(), lev) and (eng.body_times() == 1 << sched.LMAX).all()
    assert (st.block_steps, st.body_steps) == (len(log), sum(m for _, m in log)) == (256, 3282)
    assert st.steps == 1 and st.level_clamped == clamped == 768
    assert st.time == sched.DT and st.finished and st.level_max == stats["level_max"] == 8
    eng.step(3)  # past t_end: nothing happens
    assert eng.status() == st


@pytest.mark.parametrize("n", [64, 200])
def test_cpu_engine_matches_oracle(n):
    """Gate 1e-10 relative: 403 block steps x the 128 eps per-evaluation gate = 6e-12, and the
    oracle's own response to a perturbation grows by about 1 over the run."""
    x, v, lev, log, clamped, _ = oracle_run(n)
    eng = HermiteCpuEngine(cfg_for(n).validate())
    eng.load(bodies(n))
    eng.step(4)
    st, got = eng.status(), eng.state()
    assert eng.block_log == log
    assert np.abs(got.pos - x).max() / np.abs(x).max() <= 1e-10
    assert np.array_equal(eng.levels(), lev) and (eng.body_times() == 4 << 24).all()
    assert (st.block_steps, st.body_steps) == STEPS[n] and st.steps == 4
    assert st.time == 32 * DAY and st.finished and st.level_max == max(lev.max(), st.level_max)
    eng.step(3)  # past t_end: nothing happens
    assert eng.status() == st


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_accjerk_idx_is_bit_equal_to_the_range_entry(dtype):
    n = 700
    T, P = (np.float32, _native.fptr) if dtype == "fp32" else (np.float64, _native.dptr)
    lib = _native.cpu_lib()
    b = ic.solar_random(n, 3)
    X, V = np.zeros((n, 4), T), np.zeros((n, 4), T)
    X[:, :3], X[:, 3], V[:, :3] = b.pos, G_SI * b.mass, b.vel
    suf = "f32" if dtype == "fp32" else "f64"
    chunk = layout(n, 0, 1, 0).chunk
    fa, fj = np.zeros((n, 4), T), np.zeros((n, 4), T)
    assert getattr(lib, f"gs_cpu_accjerk_{suf}")(P(X), P(V), n, 0, n, chunk, T(1e-20), T(0),
                                                 P(fa), P(fj)) == 0
    idx_fn = getattr(lib, f"gs_cpu_accjerk_idx_{suf}")
    rng = np.random.default_rng(2)
    for m in (1, 2, 255, 256, 257, n):
        idx = rng.permutation(n)[:m].astype(np.int32)  # scrambled
        ga, gj = np.full((m, 4), 7, T), np.full((m, 4), 7, T)
        assert idx_fn(P(X), P(V), n, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), m, chunk,
                      T(1e-20), T(0), P(ga), P(gj)) == 0
        assert np.array_equal(ga, fa[idx]) and np.array_equal(gj, fj[idx]), m
    bad = np.array([n], dtype=np.int32)
    assert idx_fn(P(X), P(V), n, bad.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 1, chunk,
                  T(1e-20), T(0), P(fa), P(fj)) != 0


# ---- 3. driver: checkpoints, refusals, the level cap ---------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_checkpoint_mid_run_resumes_bit_exact(tmp_path, dtype):
    cfg = cfg_for(64, t_end=None).replace(dtype=dtype, steps=2)
    sim = Simulation(cfg)
    sim.engine.load(bodies(64))
    sim.run()
    path = str(tmp_path / "c.gsck")
    sim.save_checkpoint(path)
    c = ckpt.load(path)
    assert c.meta["block_steps"] and c.meta["max_level"] == 24 and c.meta["level_column"] == 0
    assert np.array_equal(c.extra["level"][:, 0], sim.engine.levels())
    assert not c.extra["level"][:, 1:].any() and c.meta["time"] == 2 * DT
    sim.run(2)
    ref, ref_lev = sim.global_state(), sim.engine.levels()
    sim2 = Simulation(cfg.replace(resume=path))
    m = sim2.run(2)
    got = sim2.global_state()
    assert np.array_equal(got.pos, ref.pos) and np.array_equal(got.vel, ref.vel)
    assert np.array_equal(sim2.engine.levels(), ref_lev)
    assert sim2.step == 4 and m.time_reached == 4 * DT and m.steps == 2
    assert m.block_steps > 2 and m.pair_evals == m.body_steps * 64
    # a shared-step checkpoint resumed with block steps: the levels start afresh
    shared = Simulation(cfg.replace(block_steps=False, eta=0.0, steps=1))
    shared.engine.load(bodies(64))
    shared.run()
    p2 = str(tmp_path / "s.gsck")
    shared.save_checkpoint(p2)
    assert "level" not in ckpt.load(p2).extra
    sim3 = Simulation(cfg.replace(resume=p2))
    a, j = sim3.engine.carried()
    assert np.array_equal(sim3.engine.levels(),
                          oracle.block_first_levels(a, j, DT, ETA, 24))
    assert sim3.run(1).time_reached == 2 * DT


def test_refusals():
    ok = dict(integrator="hermite", eta=0.02, block_steps=True, dt=100.0)
    SimConfig(**ok, t_end=300.0).validate()
    assert SimConfig().block_steps is False and SimConfig().max_level == 24
    for kw in (dict(ok, eta=0.0), dict(ok, t_end=250.0), dict(ok, max_level=41),
               dict(ok, max_level=-1), dict(ok, integrator="kd", eta=0.0)):
        with pytest.raises(ValueError):
            SimConfig(**kw).validate()
    with pytest.raises(ValueError, match="hermite runs on one rank"):
        Simulation(SimConfig(n=64, device="cpu", **ok), comm.DistInfo(rank=1, world=2))
    with pytest.raises(ValueError, match="hermite runs on one rank"):
        HermiteCpuEngine(SimConfig(n=64, device="cpu", **ok), 0, 2)


def test_level_cap_is_reported():
    """The eccentric pair wants steps near pericentre far below dt / 4."""
    b = ic.kepler()
    b.vel = b.vel * 0.6
    dt = 16 * DAY
    out = {}
    for L in (2, 24):
        eng = HermiteCpuEngine(SimConfig(n=2, dt=dt, dtype="fp64", device="cpu",
                                         integrator="hermite", eta=0.02, block_steps=True,
                                         max_level=L).validate())
        eng.load(b)
        eng.step(8)
        out[L] = eng.status()
        assert eng.levels().max() <= L and out[L].time == 8 * dt
    assert out[2].level_clamped > 0 and out[2].level_max == 2
    assert out[24].level_clamped == 0 and 2 < out[24].level_max < 24
    assert out[2].dt_min == dt / 4
    o = oracle.simulate_hermite_block(b.pos, b.vel, b.mass, dt, 8 * dt, 0.02, max_level=2)
    assert o[4] == out[2].level_clamped


# ---- 4. what the scheme is for -------------------------------------------------------------
def test_energy_and_work_against_the_shared_step():
    """64 bodies to 64 d: the oracle's shared adaptive step takes 320 steps (20480 body-steps,
    energy drift 1.8e-7); block steps 2761 body-steps with a smaller drift."""
    b = bodies(64)
    x, v, _, t, taken = oracle.simulate(b.pos, b.vel, b.mass, DT, 10 ** 6, softening=SOFT,
                                        integrator="hermite", eta=ETA, t_end=64 * DAY)
    shared_drift, shared_body_steps = drift(b, x, v), 64 * len(taken)
    eng = HermiteCpuEngine(cfg_for(64, t_end=64 * DAY).validate())
    eng.load(b)
    eng.step(8)
    st, got = eng.status(), eng.state()
    block_drift = drift(b, got.pos, got.vel)
    print(f"shared: {len(taken)} steps, {shared_body_steps} body-steps, drift {shared_drift:.2e}; "
          f"block: {st.block_steps} block steps, {st.body_steps} body-steps, "
          f"drift {block_drift:.2e}")
    assert t == 64 * DAY == st.time
    assert block_drift <= shared_drift
    assert st.body_steps <= shared_body_steps / 4


def test_cli_block_steps_metrics(tmp_path):
    out = tmp_path / "m.jsonl"
    root = str(__import__("pathlib").Path(__file__).resolve().parent.parent)
    r = subprocess.run([sys.executable, "-m", "gravsim", "--n", "64", "--init", "plummer",
                        "--integrator", "hermite", "--eta", "0.02", "--block-steps", "--max-level",
                        "20", "--dt", str(DT), "--softening", "1e9", "--steps", "2", "--device",
                        "cpu", "--dtype", "fp64", "--metrics-json", str(out), "--quiet",
                        "--log-format", "none"], capture_output=True, text=True, timeout=300,
                       cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    m = json.loads(out.read_text().splitlines()[-1])
    assert m["steps"] == 2 and m["time_reached"] == 2 * DT
    assert m["block_steps"] > 2 and m["body_steps"] >= 2 * 64
    assert m["pair_evals"] == m["body_steps"] * 64 and 0 < m["level_max"] <= 20
    assert m["level_clamped"] == 0
    r = subprocess.run([sys.executable, "-m", "gravsim", "--n", "64", "--integrator", "hermite",
                        "--block-steps", "--device", "cpu", "--steps", "1"], capture_output=True,
                       text=True, timeout=300, cwd=root)
    assert r.returncode != 0 and "eta" in r.stderr
