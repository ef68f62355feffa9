"""The gfx950 Hermite acceleration+jerk kernel and its device-side step chain against the NumPy
oracle and the native CPU engine: tile and chunk edges, the pair law, bitwise launch-shape
independence, order of accuracy, the device-chosen time step, the driver and checkpoints.

Accuracy gates: |err| <= 128 eps sum_j |term_ij| (tests/test_gpu_kernels.py assert_close_sum),
with the jerk's scale from oracle.acc_jerk(with_abs=True).
"""
import ctypes
import functools
import math

import numpy as np
import pytest

from gravsim.config import G_SI, SimConfig
from gravsim.models import initial_conditions as ic
from gravsim.models.initial_conditions import BodySet
from gravsim.ops import _native, oracle
from gravsim.ops.force import acc_jerk
from gravsim.runtime.hermite import HermiteCpuEngine, HermiteHipEngine
from gravsim.runtime.simulation import Simulation

pytestmark = pytest.mark.gpu

EPS = {"fp32": 2.0 ** -24, "fp64": 2.0 ** -53}
SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 2047, 2048, 2049, 4097]


def _engine(n, dtype="fp64", **kw):
    kw.setdefault("integrator", "hermite")
    return HermiteHipEngine(SimConfig(n=n, dtype=dtype, device="gpu", **kw).validate())


def _derivs(b, dtype, **kw):
    eng = _engine(b.n, dtype, **kw)
    try:
        eng.load(b)
        return eng.derivs()
    finally:
        eng.close()


def quantized_acc_jerk(b, dtype, **kw):
    """Oracle on the inputs as the kernel sees them (positions, velocities, mu rounded to dtype)."""
    T = np.float32 if dtype == "fp32" else np.float64
    p = b.pos.astype(T).astype(np.float64)
    v = b.vel.astype(T).astype(np.float64)
    mu = (G_SI * b.mass).astype(T).astype(np.float64)
    return oracle.acc_jerk(p, v, mu, G=1.0, with_potential=True, with_abs=True, **kw)


@functools.lru_cache(maxsize=None)
def _ref(n, dtype):
    return quantized_acc_jerk(ic.solar_random(n, seed=7 + n), dtype)


def worst_ratio(got, ref, scale, dtype):
    return float((np.abs(got - ref) / (EPS[dtype] * scale + 1e-300)).max())


def eccentric_pair():
    """ic.kepler() with both velocities scaled by 0.6: eccentricity 0.64, period 173.9 days."""
    b = ic.kepler()
    b.vel = b.vel * 0.6
    mt = b.mass.sum()
    r = np.linalg.norm(b.pos[1] - b.pos[0])
    v = np.linalg.norm(b.vel[1] - b.vel[0])
    sma = -G_SI * mt / (2.0 * (0.5 * v * v - G_SI * mt / r))
    return b, 2.0 * math.pi * math.sqrt(sma ** 3 / (G_SI * mt)), r


# ---- 1. kernel against the oracle --------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_derivs_match_oracle(hip, n, dtype):
    b = ic.solar_random(n, seed=7 + n)
    ra, rj, rphi, sa, sj = _ref(n, dtype)
    a4, j4 = _derivs(b, dtype)
    r = (worst_ratio(a4[:, :3], ra, sa, dtype), worst_ratio(j4[:, :3], rj, sj, dtype),
         worst_ratio(a4[:, 3], rphi, np.abs(rphi), dtype))
    print(f"n={n} {dtype}: acc {r[0]:.1f} jerk {r[1]:.1f} phi {r[2]:.1f} (x eps x scale)")
    assert r[0] <= 128.0 and r[1] <= 128.0 and r[2] <= 128.0
    assert not j4[:, 3].any()


def test_one_shot_entry_and_native_refusals(hip):
    b = ic.solar_random(300, 4)
    ga, gj, gphi = acc_jerk(b.pos, b.vel, b.mass, device="gpu", dtype="fp64")
    ca, cj, cphi = acc_jerk(b.pos, b.vel, b.mass, device="cpu", dtype="fp64")
    assert np.allclose(ga, ca, rtol=1e-11, atol=0) and np.allclose(gj, cj, rtol=1e-9, atol=0)
    assert np.allclose(gphi, cphi, rtol=1e-13, atol=0)
    # the native object itself refuses a second rank and a missing self-term guard
    from gravsim.runtime.engines import _gs_config

    for cfg, nranks in ((SimConfig(n=64, device="gpu"), 2),
                        (SimConfig(n=64, device="gpu", cutoff=0.0), 1)):
        c = _gs_config(cfg, 0, nranks, 0)
        h = ctypes.c_void_p()
        assert hip.gs_hermite_create(ctypes.byref(c), ctypes.byref(h)) != 0 and not h.value
        assert b"hermite" in hip.gs_last_error()


# ---- 2. cutoff and softening -------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_coincident_pair_contributes_zero(hip, dtype):
    pos = np.array([[1e11, 0, 0], [1e11, 0, 0], [-1e11, 2e10, 0]], dtype=float)
    vel = np.array([[0, 1e4, 0], [0, -2e4, 3e3], [1e3, 0, 0]], dtype=float)
    b = BodySet(pos, vel, np.array([1e25, 2e25, 3e25]))
    a4, j4 = _derivs(b, dtype)
    assert np.isfinite(a4).all() and np.isfinite(j4).all()
    ra, rj, rphi, sa, sj = quantized_acc_jerk(b, dtype)
    # each coincident body feels the third body only
    only3 = oracle.acc_jerk(pos[[0, 2]], vel[[0, 2]], b.mass[[0, 2]])
    assert np.allclose(ra[0], only3[0][0], rtol=1e-12)
    assert np.allclose(rj[0], only3[1][0], rtol=1e-12)
    assert worst_ratio(a4[:, :3], ra, sa, dtype) <= 128.0
    assert worst_ratio(j4[:, :3], rj, sj, dtype) <= 128.0


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("family", ["solar_random", "random_cube"])
def test_softening_matches_oracle(hip, dtype, family):
    """softening = 1e9 m, with and without the hard cutoff: acc, jerk and phi of every body at
    the 128 eps scale gate, but for one figure, the fp32 phi of the Sun (solar_random row 0).

    With softening a body's own pair has r^2 = eps^2 >= cutoff^2, so by the project's pair law
    phi_i includes -mu_i / eps (as in oracle.accelerations and the one-sided kernels). For the
    Sun that one term (1.3e11) is 1e5 times the sum of the 999 others, each of which
    (20 .. 2000) is below half an fp32 ulp (4096) of the running sum: an fp32 sum in j order
    drops them all, an error of sum(others) / (mu / eps) = 8.8e-6 = 147.7 eps whoever does the
    sum. The gate and the prescribed order cannot both hold for that row, so it is asserted
    (a) against the bound of a sequential fp32 sum of n terms, (n - 1) eps sum |terms|
    (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4, first order), and
    (b) at the 128 eps scale gate against the native fp32 CPU engine, which sums in the same
    order with a correctly rounded 1 / sqrt."""
    n = 1000
    b = getattr(ic, family)(n, 11)
    for kw in (dict(softening=1e9), dict(softening=1e9, cutoff=0.0)):
        ra, rj, rphi, sa, sj = quantized_acc_jerk(b, dtype, **kw)
        a4, j4 = _derivs(b, dtype, **kw)
        assert worst_ratio(a4[:, :3], ra, sa, dtype) <= 128.0
        assert worst_ratio(j4[:, :3], rj, sj, dtype) <= 128.0
        lo = 0
        if family == "solar_random" and dtype == "fp32":
            lo = 1
            sun = worst_ratio(a4[:1, 3], rphi[:1], np.abs(rphi[:1]), dtype)
            _, _, cphi = acc_jerk(b.pos, b.vel, b.mass, device="cpu", dtype="fp32", **kw)
            vs_cpu = worst_ratio(a4[:1, 3], cphi[:1], np.abs(rphi[:1]), dtype)
            print(f"fp32 phi of the Sun, softened: {sun:.1f} x eps x scale against the oracle, "
                  f"{vs_cpu:.2f} against the fp32 CPU engine")
            assert sun <= n - 1
            assert vs_cpu <= 128.0
        assert worst_ratio(a4[lo:, 3], rphi[lo:], np.abs(rphi[lo:]), dtype) <= 128.0


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_body_at_origin_beside_ghost_rows(hip, dtype):
    """Ghost rows sit at the origin, massless: a real body there meets them at r = 0."""
    pos = np.array([[0, 0, 0], [1.5e11, 0, 0], [0, -2e11, 1e10]], dtype=float)
    vel = np.array([[0, 0, 0], [0, 3e4, 0], [2e4, 0, 0]], dtype=float)
    b = BodySet(pos, vel, np.array([2e30, 6e24, 6e23]))
    eng = _engine(3, dtype, dt=3600.0)
    try:
        eng.load(b)
        a4, j4 = eng.derivs()
        ra, rj, rphi, sa, sj = quantized_acc_jerk(b, dtype)
        assert np.isfinite(a4).all() and np.isfinite(j4).all()
        assert worst_ratio(a4[:, :3], ra, sa, dtype) <= 128.0
        assert worst_ratio(j4[:, :3], rj, sj, dtype) <= 128.0
        eng.step(3)
        assert eng.nonfinite() == 0 and np.isfinite(eng.state().pos).all()
    finally:
        eng.close()


# ---- 3. bits -----------------------------------------------------------------------------
def _run_shape(dtype, ipl, groups, eta):
    eng = _engine(5000, dtype, dt=4e5, eta=eta, ipl=ipl, split_groups=groups)
    try:
        assert ipl == 0 or eng.native_layout["ipl"] == ipl
        eng.init_ics("solar+random", 3)
        eng.step(3)
        st = eng.status()
        s = eng.state()
        a, j = eng.carried()
        return s.pos, s.vel, a, j, (st.time, st.dt_last, st.dt_next, st.steps)
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("eta", [0.0, 0.05])
def test_every_launch_shape_gives_the_same_bits(hip, dtype, eta):
    """n = 5000: 3 chunks of 2048 (the last partly ghosts); IPL 1, 2 (fp32: 4) x 1, 2, 3 chunk
    groups, the auto shape, and the same shape twice."""
    ref = _run_shape(dtype, 0, 0, eta)
    again = _run_shape(dtype, 0, 0, eta)
    shapes = [(ipl, g) for ipl in ((1, 2, 4) if dtype == "fp32" else (1, 2)) for g in (1, 2, 3)]
    for got in [again] + [_run_shape(dtype, ipl, g, eta) for ipl, g in shapes]:
        for x, y in zip(got[:4], ref[:4]):
            assert np.array_equal(x, y)
        assert got[4] == ref[4]
    assert ref[4][3] == 3 and np.isfinite(ref[0]).all()
    if eta:
        assert ref[4][1] < 4e5  # the criterion chose the steps


# ---- 4. steps against the oracle and the CPU engine --------------------------------------
def test_steps_match_oracle_fp64(hip):
    b = ic.solar_random(800, 20250307)
    eng = _engine(800, "fp64", dt=3600.0)
    eng.load(b)
    eng.step(10)
    got = eng.state()
    st = eng.status()
    eng.close()
    x, v, _, t, _ = oracle.simulate(b.pos, b.vel, b.mass, 3600.0, 10, integrator="hermite")
    assert np.abs(got.pos - x).max() / np.abs(x).max() < 1e-12
    assert np.abs(got.vel - v).max() / np.abs(v).max() < 1e-10
    assert st.time == t and st.steps == 10


def test_steps_match_cpu_engine_fp32(hip):
    b = ic.solar_random(800, 5)
    cfg = SimConfig(n=800, dtype="fp32", dt=3600.0, integrator="hermite")
    out = []
    for eng in (HermiteHipEngine(cfg.replace(device="gpu")),
                HermiteCpuEngine(cfg.replace(device="cpu"))):
        eng.load(b)
        eng.step(10)
        out.append(eng.state())
        eng.close()
    tol = 1e-5  # (tests/test_gpu_kernels.py test_steps_match_oracle, fp32)
    assert np.abs(out[0].pos - out[1].pos).max() / np.abs(out[1].pos).max() < tol
    assert np.abs(out[0].vel - out[1].vel).max() / np.abs(out[1].vel).max() < tol * 10


# ---- 5. order on the device --------------------------------------------------------------
def test_fourth_order_on_the_device(hip):
    b, T, r = eccentric_pair()
    errs = []
    for m in (500, 1000, 2000):
        eng = _engine(2, "fp64", dt=T / m)
        eng.load(b)
        eng.step(m)
        errs.append(np.linalg.norm(eng.state().pos - b.pos) / r)
        eng.close()
    print("closure errors", errs, "ratios", errs[0] / errs[1], errs[1] / errs[2])
    assert 12.0 <= errs[0] / errs[1] <= 22.0
    assert 12.0 <= errs[1] / errs[2] <= 22.0
    assert errs[1] < 1e-6


# ---- 6. device-side time step ------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 257, 4097])
def test_dt_next_after_one_adaptive_step(hip, n):
    """A tight pair at the last two indices sets the minimum from the partly filled last tile
    (and, at 4097, from the last workgroup of the last chunk)."""
    b = ic.solar_random(n, seed=31 + n)
    b.pos[n - 1] = b.pos[n - 2] + np.array([1e7, 0.0, 0.0])
    b.vel[n - 1] = b.vel[n - 2] + np.array([0.0, 5e3, 0.0])
    b.mass[n - 2:] = 1e25
    dt_max, eta = 3600.0, 0.02
    _, _, _, _, taken = oracle.simulate(b.pos, b.vel, b.mass, dt_max, 2, integrator="hermite",
                                        eta=eta)
    assert taken[1] < 0.5 * dt_max
    if n <= 257:  # (the same bodies with the pair pulled apart choose a much longer step)
        loose = b.copy()
        loose.pos[n - 1] = loose.pos[n - 2] + np.array([3e10, 0.0, 0.0])
        others = oracle.simulate(loose.pos, loose.vel, loose.mass, dt_max * 100, 2,
                                 integrator="hermite", eta=eta)[4]
        assert taken[1] < 0.5 * others[1]  # the pair sets the minimum
    eng = _engine(n, "fp64", dt=dt_max, eta=eta)
    try:
        eng.load(b)
        assert abs(eng.status().dt_next / taken[0] - 1.0) < 1e-9  # (eta / 2) min |a| / |j|
        eng.step(1)
        st = eng.status()
        assert abs(st.dt_last / taken[0] - 1.0) < 1e-9 and st.steps == 1
        assert abs(st.dt_next / taken[1] - 1.0) < 1e-9
    finally:
        eng.close()


def test_adaptive_orbit_on_the_device(hip):
    b, T, _ = eccentric_pair()
    x, v, _, t, taken = oracle.simulate(b.pos, b.vel, b.mass, T / 50, 100000,
                                        integrator="hermite", eta=0.02, t_end=T)
    eng = _engine(2, "fp64", dt=T / 50, eta=0.02, t_end=T)
    try:
        eng.load(b)
        eng.step(len(taken) - 1)
        assert not eng.status().finished
        eng.step(1)
        st = eng.status()
        assert st.finished and st.time == T and st.steps == len(taken)
        assert abs(st.dt_min / min(taken[:-1]) - 1.0) < 1e-9
        got = eng.state()
        assert np.abs(got.pos - x).max() / np.abs(x).max() < 1e-12
        assert np.abs(got.vel - v).max() / np.abs(v).max() < 1e-10
        a0, j0 = eng.carried()
        eng.step(64)  # past t_end: no-ops, not counted
        after, st2 = eng.state(), eng.status()
        assert np.array_equal(after.pos, got.pos) and np.array_equal(after.vel, got.vel)
        assert all(np.array_equal(p, q) for p, q in zip(eng.carried(), (a0, j0)))
        assert (st2.time, st2.steps, st2.dt_last, st2.dt_min) == (st.time, st.steps, st.dt_last,
                                                                  st.dt_min)
    finally:
        eng.close()


# ---- 7. driver ---------------------------------------------------------------------------
def test_driver_diagnostics_and_t_end(hip):
    t_end = 1e5
    cfg = SimConfig(n=3000, steps=400, dt=4e5, dtype="fp64", device="gpu", integrator="hermite",
                    eta=0.0005, t_end=t_end, diagnostics=True)
    sim = Simulation(cfg)
    try:
        m = sim.run()
        c = m.extra["conservation"]
        for k in ("energy_rel_drift", "momentum_rel_drift", "angular_momentum_rel_drift"):
            assert np.isfinite(c[k]), k
        assert m.time_reached == t_end and 33 <= m.steps_taken == m.steps < 400
        assert m.device == "gpu" and 0 < m.dt_min <= cfg.dt
        assert sim.engine.status().steps == m.steps  # at most 32 no-ops ran, none counted
        # the run guard's hooks exist: one rank has no communicator to abort
        assert sim.engine.abort() is False and "one rank" in sim.engine.comm_stage()
    finally:
        sim.close()


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("eta", [0.0, 0.02])
def test_gpu_resume_is_bit_exact(hip, tmp_path, dtype, eta):
    cfg = SimConfig(n=3000, steps=5, dt=4e5, dtype=dtype, device="gpu", integrator="hermite",
                    eta=eta)
    sim = Simulation(cfg)
    sim.run()
    path = str(tmp_path / "c.gsck")
    sim.save_checkpoint(path)
    sim.run(3)
    ref, ref_st = sim.global_state(), sim.engine.status()
    sim.close()
    sim2 = Simulation(cfg.replace(resume=path))
    sim2.run(3)
    got, got_st, step2 = sim2.global_state(), sim2.engine.status(), sim2.step
    sim2.close()
    assert np.array_equal(got.pos, ref.pos) and np.array_equal(got.vel, ref.vel)
    assert (got_st.time, got_st.dt_next, got_st.dt_min) == (ref_st.time, ref_st.dt_next,
                                                             ref_st.dt_min)
    assert step2 == 8
    if eta:
        assert ref_st.dt_last < cfg.dt
