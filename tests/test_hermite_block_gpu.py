"""Hermite block time steps on the GPU: the two evaluate paths of a block step (narrow: parallel
over j; wide: the gathered i-owned kernel) against the NumPy oracle and against each other's
promises about bits, then whole runs against the oracle, determinism, checkpoints and the CLI.

Accuracy gates: |err| <= 128 eps sum_j |term_ij| (tests/test_hermite_gpu.py), scales from
oracle.acc_jerk(with_abs=True).
"""
import functools
import json
import subprocess
import sys

import numpy as np
import pytest

from gravsim.config import G_SI, SimConfig
from gravsim.models import initial_conditions as ic
from gravsim.models.initial_conditions import BodySet
from gravsim.ops import oracle
from gravsim.ops.force import acc_jerk
from gravsim.runtime.hermite import HermiteHipEngine
from gravsim.runtime.simulation import Simulation

pytestmark = pytest.mark.gpu

EPS = {"fp32": 2.0 ** -24, "fp64": 2.0 ** -53}
SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 2047, 2048, 2049, 4097]
GROUP = 4  # active bodies a narrow workgroup carries per pass (gs_hermite.h kNarrowGroup)
LENGTHS = [1, 2, GROUP - 1, GROUP, GROUP + 1, 63, 64, 65, 257]
DAY = 86400.0
DT, ETA, SOFT = 8 * DAY, 0.02, 1e9
PLUMMER = {64: 5, 200: 9}


def _engine(n, dtype="fp64", **kw):
    kw.setdefault("integrator", "hermite")
    kw.setdefault("eta", ETA)
    kw.setdefault("block_steps", True)
    return HermiteHipEngine(SimConfig(n=n, dtype=dtype, device="gpu", **kw).validate())


def quantized_acc_jerk(b, dtype, **kw):
    """Oracle on the inputs as the kernel sees them (positions, velocities, mu rounded to dtype)."""
    T = np.float32 if dtype == "fp32" else np.float64
    p = b.pos.astype(T).astype(np.float64)
    v = b.vel.astype(T).astype(np.float64)
    mu = (G_SI * b.mass).astype(T).astype(np.float64)
    return oracle.acc_jerk(p, v, mu, G=1.0, with_potential=True, with_abs=True, **kw)


def worst_ratio(got, ref, scale, dtype):
    return float((np.abs(got - ref) / (EPS[dtype] * scale + 1e-300)).max())


def active_lists(n):
    """Sorted entries of a seeded permutation, of every length in LENGTHS and n, clipped to n."""
    perm = np.random.default_rng(100 + n).permutation(n)
    return {m: np.sort(perm[:m]).astype(np.int32) for m in sorted({min(m, n) for m in
                                                                  LENGTHS + [n]})}


@functools.lru_cache(maxsize=None)
def _ref(n, dtype):
    return quantized_acc_jerk(ic.solar_random(n, seed=7 + n), dtype)


@functools.lru_cache(maxsize=None)
def _paths(n, dtype):
    """One engine per (n, dtype): the shared-step derivs() and, for every active list, the rows
    of both block paths."""
    eng = _engine(n, dtype, dt=3600.0)
    try:
        eng.load(ic.solar_random(n, seed=7 + n))
        eng.set_block_tuning(narrow_max=n)
        full = eng.derivs()
        out = {m: {p: eng.derivs(active=idx, path=p) for p in ("narrow", "wide")}
               for m, idx in active_lists(n).items()}
        return full, out
    finally:
        eng.close()


# ---- 1. the two evaluate paths against the oracle -----------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_both_paths_match_oracle(hip, n, dtype):
    ra, rj, rphi, sa, sj = _ref(n, dtype)
    _, out = _paths(n, dtype)
    for m, idx in active_lists(n).items():
        for path in ("narrow", "wide"):
            a4, j4 = out[m][path]
            r = (worst_ratio(a4[:, :3], ra[idx], sa[idx], dtype),
                 worst_ratio(j4[:, :3], rj[idx], sj[idx], dtype),
                 worst_ratio(a4[:, 3], rphi[idx], np.abs(rphi[idx]), dtype))
            print(f"n={n} {dtype} {path} n_act={m}: acc {r[0]:.1f} jerk {r[1]:.1f} phi {r[2]:.1f}")
            assert a4.shape == (m, 4) and max(r) <= 128.0, (m, path, r)
            assert not j4[:, 3].any()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_wide_path_bits_are_the_shared_step_kernels(hip, n, dtype):
    (fa, fj), out = _paths(n, dtype)
    for m, idx in active_lists(n).items():
        a4, j4 = out[m]["wide"]
        assert np.array_equal(a4, fa[idx]) and np.array_equal(j4, fj[idx]), m


@pytest.mark.parametrize("n", [3, 257, 2049])
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_narrow_bits_depend_on_the_body_alone(hip, n, dtype):
    """Alone, among others, at another slot, in another order: the same bits."""
    eng = _engine(n, dtype, dt=3600.0)
    try:
        eng.load(ic.solar_random(n, seed=7 + n))
        eng.set_block_tuning(narrow_max=n)
        every = np.arange(n, dtype=np.int32)
        ea, ej = eng.derivs(active=every, path="narrow")
        for i in sorted({0, 1, n // 2, n - 1}):
            a1, j1 = eng.derivs(active=[i], path="narrow")
            assert np.array_equal(a1[0], ea[i]) and np.array_equal(j1[0], ej[i]), i
        rev = every[::-1].copy()
        ra, rj = eng.derivs(active=rev, path="narrow")
        assert np.array_equal(ra, ea[rev]) and np.array_equal(rj, ej[rev])
        some = np.sort(np.random.default_rng(n).permutation(n)[: min(n, 7)]).astype(np.int32)
        sa, sj = eng.derivs(active=some, path="narrow")
        assert np.array_equal(sa, ea[some]) and np.array_equal(sj, ej[some])
        # narrow_max does not change them either, and bounds the narrow path
        eng.set_block_tuning(narrow_max=min(n, 5))
        ta, tj = eng.derivs(active=some[: min(n, 5)])
        assert np.array_equal(ta, ea[some[: min(n, 5)]])
        if n > 5:
            with pytest.raises(RuntimeError, match="narrow_max"):
                eng.derivs(active=every, path="narrow")
            wa, _ = eng.derivs(active=some)  # 7 > narrow_max: wide
            assert np.array_equal(wa, eng.derivs()[0][some])
    finally:
        eng.close()


# ---- 2. the pair law ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("path", ["narrow", "wide"])
def test_coincident_self_and_ghost_pairs_contribute_exactly_zero(hip, dtype, path):
    """Body 0 sits on body 1 and on the origin, where the ghost rows are. Its derivatives are
    those with body 1 massless and elsewhere, bit for bit: the pair with body 1, its own and
    those with the ghost rows add exactly nothing."""
    pos = np.array([[0, 0, 0], [0, 0, 0], [-1e11, 2e10, 0], [3e10, -1e11, 5e9]], dtype=float)
    vel = np.array([[0, 1e4, 0], [0, -2e4, 3e3], [1e3, 0, 0], [0, 2e3, -1e3]], dtype=float)
    mass = np.array([1e25, 2e25, 3e25, 4e25])
    apart = pos.copy()
    apart[1] = [5e10, 5e10, 5e10]
    got = []
    for p, m in ((pos, mass), (apart, mass * np.array([1, 0, 1, 1]))):
        eng = _engine(4, dtype, dt=3600.0)
        try:
            eng.load(BodySet(p, vel, m))
            got.append(eng.derivs(active=[0, 2], path=path))
        finally:
            eng.close()
    (a, j), (a_ref, j_ref) = got
    assert np.isfinite(a).all() and np.isfinite(j).all()
    assert np.array_equal(a[0], a_ref[0]) and np.array_equal(j[0], j_ref[0])
    ra, rj, rphi, sa, sj = quantized_acc_jerk(BodySet(pos, vel, mass), dtype)
    idx = [0, 2]
    assert worst_ratio(a[:, :3], ra[idx], sa[idx], dtype) <= 128.0
    assert worst_ratio(j[:, :3], rj[idx], sj[idx], dtype) <= 128.0
    assert worst_ratio(a[:, 3], rphi[idx], np.abs(rphi[idx]), dtype) <= 128.0


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_softening_matches_oracle_on_both_paths(hip, dtype):
    """softening 1e9 m. On the wide path, which sums in j order, the fp32 potential of the Sun is
    the one row beyond the gate, as in tests/test_hermite_gpu.py test_softening_matches_oracle
    (its own term -mu / eps swamps the others in fp32): asserted against the bound of an fp32 sum
    of n terms, (n - 1) eps, and at the gate against the fp32 CPU engine, which sums in the same
    order. The narrow path folds lanes, waves and slices by a tree, so the Sun's own term meets
    3 rows of its lane, 6 + 3 partial sums of the fold and the other slices' sums, a dozen
    roundings of its size: that row holds the gate too."""
    n = 1000
    b = ic.solar_random(n, 11)
    idx = np.sort(np.random.default_rng(5).permutation(n)[:300]).astype(np.int32)
    idx[0] = 0  # the Sun
    kw = dict(softening=SOFT)
    ra, rj, rphi, sa, sj = quantized_acc_jerk(b, dtype, **kw)
    eng = _engine(n, dtype, dt=3600.0, **kw)
    try:
        eng.load(b)
        eng.set_block_tuning(narrow_max=n)
        for path in ("narrow", "wide"):
            a4, j4 = eng.derivs(active=idx, path=path)
            assert worst_ratio(a4[:, :3], ra[idx], sa[idx], dtype) <= 128.0
            assert worst_ratio(j4[:, :3], rj[idx], sj[idx], dtype) <= 128.0
            lo = 0
            if dtype == "fp32" and path == "wide":
                lo = 1
                sun = worst_ratio(a4[:1, 3], rphi[:1], np.abs(rphi[:1]), dtype)
                _, _, cphi = acc_jerk(b.pos, b.vel, b.mass, device="cpu", dtype="fp32", **kw)
                vs_cpu = worst_ratio(a4[:1, 3], cphi[:1], np.abs(rphi[:1]), dtype)
                print(f"{path}: fp32 phi of the Sun {sun:.1f} x eps x scale against the oracle, "
                      f"{vs_cpu:.2f} against the fp32 CPU engine")
                assert sun <= n - 1 and vs_cpu <= 128.0
            assert worst_ratio(a4[lo:, 3], rphi[idx][lo:], np.abs(rphi[idx][lo:]), dtype) <= 128.0
    finally:
        eng.close()


# ---- 3. runs --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_all_at_level_0_is_the_shared_step_bit_for_bit(hip, dtype):
    """Slow, widely spaced bodies and dt = 1 s: every dt_want >> dt, so every body stays at level
    0, a block step is a shared step, and with the wide path the bits are the same."""
    n, K = 700, 3
    b = ic.solar_random(n, 12)
    out = []
    for block in (True, False):
        eng = _engine(n, dtype, dt=1.0, block_steps=block)
        try:
            eng.load(b)
            if block:
                eng.set_block_tuning(narrow_max=0)
            eng.step(K)
            st, s = eng.status(), eng.state()
            out.append((s.pos, s.vel) + eng.carried())
            assert st.time == K and st.steps == K
            if block:
                assert (st.level_max, st.block_steps, st.body_steps) == (0, K, K * n)
                assert not eng.levels().any() and (eng.body_times() == K << 24).all()
            else:
                assert st.dt_last == 1.0 and st.dt_next == 1.0
        finally:
            eng.close()
    for x, y in zip(*out):
        assert np.array_equal(x, y)


def test_mode_toggles_reach_the_bits_of_a_fresh_engine(hip):
    """The device buffers of a mode are built and dropped with the mode (gs_hermite's groups): an
    engine brought to block steps with collisions through every toggle, off and on again, runs to
    the bits of one created that way. n = 2049: two chunks, n_pad 4096. The narrow path's
    neighbour and snap partials are re-derived at the switches of collisions, block mode, the
    narrow slots and the order.
    (Order 6 refuses collisions, so the switch to it with collisions on is refused and leaves the
    engine as it was; it is then taken with collisions off, holds block steps of its own once, and
    collisions go back on after order 4.)"""
    n, K = 2049, 3
    kw = dict(dt=DAY, max_level=6)  # (levels up to 6 in use, about 40 block steps a macro step)
    rng = np.random.default_rng(11)
    b = ic.solar_random(n, 7 + n)
    b = BodySet(b.pos, b.vel, b.mass, np.abs(rng.normal(size=n)) * 1e8 * (rng.random(n) > 0.25))
    A = _engine(n, "fp64", collisions="detect", **kw)
    B = _engine(n, "fp64", block_steps=False, **kw)
    try:
        lib, h, L = B.lib, B._h, int(B.cfg.max_level)

        def ok(rc):
            assert rc == 0, lib.gs_last_error().decode()

        ok(lib.gs_hermite_set_collisions(h, 1))
        ok(lib.gs_hermite_set_block(h, 1, L))
        ok(lib.gs_hermite_set_block_tuning(h, 0))
        ok(lib.gs_hermite_set_block_tuning(h, n))
        ok(lib.gs_hermite_set_collisions(h, 0))
        ok(lib.gs_hermite_set_collisions(h, 1))
        ok(lib.gs_hermite_set_block(h, 0, L))
        assert lib.gs_hermite_set_order(h, 6) != 0 and lib.gs_hermite_get_order(h) == 4
        assert b"order 6 has no collisions" in lib.gs_last_error()
        ok(lib.gs_hermite_set_collisions(h, 0))
        ok(lib.gs_hermite_set_order(h, 6))
        assert lib.gs_hermite_get_order(h) == 6
        ok(lib.gs_hermite_set_block6(h, 1, L))  # (the narrow slots with the snap partials)
        ok(lib.gs_hermite_set_block_tuning(h, n))
        ok(lib.gs_hermite_set_block6(h, 0, L))
        ok(lib.gs_hermite_set_order(h, 4))
        ok(lib.gs_hermite_set_collisions(h, 1))
        ok(lib.gs_hermite_set_block(h, 1, L))
        ok(lib.gs_hermite_set_block_tuning(h, n))
        B.block = B.collisions = True  # (what load() and the reads of the Python engine ask)
        A.set_block_tuning(n)
        out = []
        for eng in (A, B):
            assert eng.status_narrow_max() == n  # (every active set takes the narrow path)
            eng.load(b)
            eng.step(K)
            st, s = eng.status(), eng.state()
            assert st.steps == K and st.time == K * DAY and st.block_steps > K
            out.append((s.pos, s.vel, *eng.carried(), eng.levels(), eng.body_times(),
                        *eng.neighbours(), *eng.closest(),
                        np.array([st.block_steps, st.body_steps, st.level_max, st.overlaps])))
        assert out[0][4].any() and (out[0][7] >= 0).all()  # (levels in use, neighbours found)
        for x, y in zip(*out):
            assert x.tobytes() == y.tobytes()
    finally:
        A.close()
        B.close()


@functools.lru_cache(maxsize=None)
def _oracle_run(n, days=32):
    b = ic.plummer(n, seed=PLUMMER[n])
    return oracle.simulate_hermite_block(b.pos, b.vel, b.mass, DT, days * DAY, ETA, softening=SOFT)


def _block_run(n, dtype, narrow_max=None, days=32):
    eng = _engine(n, dtype, dt=DT, softening=SOFT, t_end=days * DAY)
    try:
        eng.load(ic.plummer(n, seed=PLUMMER[n]))
        if narrow_max is not None:
            eng.set_block_tuning(narrow_max=narrow_max)
        eng.step(days // 8 + 2)  # (the steps past t_end are no-ops)
        return eng.state(), eng.status(), eng.levels(), eng.body_times()
    finally:
        eng.close()


@pytest.mark.parametrize("n", [64, 200])
@pytest.mark.parametrize("narrow_max", [None, "n", 0, 16])
def test_fp64_run_matches_oracle(hip, n, narrow_max):
    """Default narrow_max, always narrow, always wide, and a mix of both. Gate 1e-10 relative:
    403 block steps x the 128 eps per-evaluation gate = 6e-12, perturbation growth about 1."""
    x, v, lev, log, clamped = _oracle_run(n)
    s, st, glev, tb = _block_run(n, "fp64", n if narrow_max == "n" else narrow_max)
    assert st.block_steps == len(log) and st.body_steps == sum(m for _, m in log)
    err = np.abs(s.pos - x).max() / np.abs(x).max()
    print(f"n={n} narrow_max={narrow_max}: {st.block_steps} block steps, position error {err:.2e}")
    assert err <= 1e-10
    assert np.array_equal(glev, lev) and (tb == 4 << 24).all()
    assert st.time == 32 * DAY and st.finished and st.steps == 4
    assert st.level_clamped == clamped == 0 and st.level_max >= lev.max()


def _energy(b, pos, vel):
    _, phi = oracle.accelerations(pos, b.mass, softening=SOFT, with_potential=True)
    phi = phi + G_SI * b.mass / SOFT  # (without the bodies' own -mu / eps)
    return 0.5 * (b.mass * (vel ** 2).sum(1)).sum() + 0.5 * (b.mass * phi).sum()


def _drift(b, s):
    e0 = _energy(b, b.pos, b.vel)
    return abs(_energy(b, s[0], s[1]) - e0) / abs(e0)


def test_fp32_run(hip):
    """The level sequence of an fp32 run may differ from the fp64 oracle's (the criterion is
    built from differences), so the invariants, the work and the energy are asserted. The energy
    gate is 4 x the larger of the fp32 shared-step drift and the oracle's block drift, both
    measured here; the margin is for rounding in the level choice. On one MI355X: fp32 block
    drift 6.8e-8 in 402 block steps and 6268 body-steps, fp32 shared-step drift 3.8e-9 in 285
    steps (57,000 body-steps), fp64 oracle block drift 4.4e-8."""
    n = 200
    b = ic.plummer(n, seed=PLUMMER[n])
    s, st, lev, tb = _block_run(n, "fp32")
    assert (tb == 4 << 24).all() and st.time == 32 * DAY and st.finished
    assert np.isfinite(s.pos).all() and np.isfinite(s.vel).all()
    assert 0 <= lev.min() and lev.max() <= st.level_max <= 24 and st.level_clamped == 0
    eng = _engine(n, "fp32", dt=DT, softening=SOFT, t_end=32 * DAY, block_steps=False)
    try:
        eng.load(b)
        while not eng.status().finished:
            eng.step(64)
        sh, sh_st = eng.state(), eng.status()
    finally:
        eng.close()
    ox, ov = _oracle_run(n)[:2]
    d_block, d_shared, d_oracle = _drift(b, (s.pos, s.vel)), _drift(b, (sh.pos, sh.vel)), \
        _drift(b, (ox, ov))
    print(f"fp32 block: {st.block_steps} block steps, {st.body_steps} body-steps, drift "
          f"{d_block:.2e}; fp32 shared: {sh_st.steps} steps, drift {d_shared:.2e}; fp64 oracle "
          f"block drift {d_oracle:.2e}")
    assert st.body_steps < 0.5 * sh_st.steps * n
    assert d_block <= 4.0 * max(d_shared, d_oracle)


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_same_run_twice_gives_the_same_bits(hip, dtype):
    a, b = _block_run(200, dtype, 16), _block_run(200, dtype, 16)
    assert np.array_equal(a[0].pos, b[0].pos) and np.array_equal(a[0].vel, b[0].vel)
    assert a[1] == b[1] and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_gpu_resume_is_bit_exact(hip, tmp_path, dtype):
    cfg = SimConfig(n=200, steps=2, dt=DT, dtype=dtype, device="gpu", integrator="hermite",
                    eta=ETA, softening=SOFT, block_steps=True, init="plummer", seed=9)
    sim = Simulation(cfg)
    m = sim.run()
    assert m.steps == 2 and m.block_steps > 2 and m.pair_evals == m.body_steps * 200
    path = str(tmp_path / "c.gsck")
    sim.save_checkpoint(path)
    sim.run(2)
    ref, ref_lev, ref_st = sim.global_state(), sim.engine.levels(), sim.engine.status()
    sim.close()
    sim2 = Simulation(cfg.replace(resume=path))
    sim2.run(2)
    got, lev, st, step2 = sim2.global_state(), sim2.engine.levels(), sim2.engine.status(), \
        sim2.step
    sim2.close()
    assert np.array_equal(got.pos, ref.pos) and np.array_equal(got.vel, ref.vel)
    assert np.array_equal(lev, ref_lev) and st.time == ref_st.time == 4 * DT and step2 == 4


def test_cli_block_steps_metrics(hip, tmp_path):
    out = tmp_path / "m.jsonl"
    root = str(__import__("pathlib").Path(__file__).resolve().parent.parent)
    r = subprocess.run([sys.executable, "-m", "gravsim", "--n", "3000", "--init", "plummer",
                        "--integrator", "hermite", "--eta", "0.02", "--block-steps", "--dt",
                        str(DT), "--softening", "1e9", "--steps", "1", "--device", "gpu",
                        "--dtype", "fp32", "--metrics-json", str(out), "--quiet",
                        "--log-format", "none"], capture_output=True, text=True, timeout=300,
                       cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    m = json.loads(out.read_text().splitlines()[-1])
    assert m["device"] == "gpu" and m["steps"] == 1 and m["time_reached"] == DT
    assert m["block_steps"] > 1 and 3000 <= m["body_steps"] < m["block_steps"] * 3000
    assert m["pair_evals"] == m["body_steps"] * 3000 and 0 < m["level_max"] <= 24
