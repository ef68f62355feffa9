"""Hermite in mixed precision on the GPU (dtype "mixed": fp64 state, fp32 pair kernels on
double-single predicted positions): the evaluate kernels against the NumPy oracle at the tile and
chunk edges, launch-shape and block-path promises about bits, the pair law, the fp64 round trip,
the dynamics the mode is for (with the same thresholds as tests/test_hermite_mixed_cpu.py),
the device chain against the CPU engine, checkpoints and refusals.

Reference: oracle.acc_jerk on the inputs as the pair kernel sees them, positions as hi + lo
(ds_seen), velocities and mu rounded to fp32. Gate: |err| <= 128 * 2^-24 * scale, the scales from
with_abs=True and |phi| (tests/test_hermite_gpu.py).
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
from gravsim.parallel import comm
from gravsim.runtime.hermite import HermiteCpuEngine, HermiteHipEngine
from gravsim.runtime.simulation import Simulation

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
GATE = 128.0
F32, F64 = np.float32, np.float64
SIZES = [1, 2, 3, 255, 256, 257, 2047, 2048, 2049, 4097]


# ---- shared helpers (the same in tests/test_hermite_mixed_cpu.py) --------------------------
def ds_seen(pos):
    """The position a double-single (hi, lo) fp32 pair carries."""
    pos = np.asarray(pos, F64)
    hi = pos.astype(F32)
    lo = (pos - hi).astype(F32)
    return hi.astype(F64) + lo.astype(F64)


def reference(b, **kw):
    """(acc, jerk, phi, acc scale, jerk scale) of the inputs as the mixed pair kernel sees them."""
    v = b.vel.astype(F32).astype(F64)
    mu = (G_SI * b.mass).astype(F32).astype(F64)
    return oracle.acc_jerk(ds_seen(b.pos), v, mu, G=1.0, with_potential=True, with_abs=True, **kw)


def worst_ratio(got, ref, scale):
    return float((np.abs(got - ref) / (EPS * scale + 1e-300)).max())


def ratios(a4, j4, ref, idx=slice(None)):
    ra, rj, rphi, sa, sj = ref
    return (worst_ratio(a4[:, :3], ra[idx], sa[idx]), worst_ratio(j4[:, :3], rj[idx], sj[idx]),
            worst_ratio(a4[:, 3], rphi[idx], np.abs(rphi[idx])))


def tight_pairs(n, seed, npairs=16, sep=1e6):
    """solar+random with up to npairs circular binaries of separation sep wherever the random
    bodies happen to be: body 3 + 2k + 1 is moved next to body 3 + 2k."""
    b = ic.solar_random(n, seed)
    rng = np.random.default_rng(seed)
    for k in range(npairs):
        i = 3 + 2 * k
        if i + 1 >= n:
            break
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        t = np.cross(u, (0.3, 0.5, 0.8))
        t /= np.linalg.norm(t)
        b.pos[i + 1] = b.pos[i] + sep * u
        b.vel[i + 1] = b.vel[i] + math.sqrt(G_SI * (b.mass[i] + b.mass[i + 1]) / sep) * t
    return b


COM = np.array([1.5e11, 0.7e11, -0.3e11])
COM_V = np.array([0.0, 3e4, 0.0])


def offset_binary(sep):
    """Two bodies of 6e24 kg on a circular orbit of separation sep about a centre of mass at COM
    that moves at 30 km/s. Returns (bodies, period)."""
    m = 6e24
    v = math.sqrt(G_SI * 2 * m / sep)
    pos = np.array([COM + [sep / 2, 0, 0], COM - [sep / 2, 0, 0]])
    vel = np.array([COM_V + [0, v / 2, 0], COM_V - [0, v / 2, 0]])
    return BodySet(pos, vel, np.array([m, m])), 2 * math.pi * math.sqrt(sep ** 3 / (G_SI * 2 * m))


def binary_energy(pos, vel, mass):
    """Energy of the relative orbit of bodies 0 and 1 per unit reduced mass."""
    r, v = pos[1] - pos[0], vel[1] - vel[0]
    return 0.5 * (v * v).sum() - G_SI * (mass[0] + mass[1]) / math.sqrt((r * r).sum())


def binary_drift(b, state):
    e0 = binary_energy(b.pos, b.vel, b.mass)
    return abs(binary_energy(state.pos, state.vel, b.mass) - e0) / abs(e0)


def run_sim(b, dtype, device="gpu", **kw):
    sim = Simulation(SimConfig(n=b.n, dtype=dtype, device=device, integrator="hermite", **kw))
    try:
        sim.engine.load(b)
        m = sim.run()
        return sim.global_state(), sim.engine.status(), m
    finally:
        sim.close()


def _engine(n, dtype="mixed", **kw):
    kw.setdefault("integrator", "hermite")
    return HermiteHipEngine(SimConfig(n=n, dtype=dtype, device="gpu", **kw).validate())


def _derivs(b, dtype="mixed", **kw):
    eng = _engine(b.n, dtype, **kw)
    try:
        eng.load(b)
        return eng.derivs()
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _pairs_ref(n):
    return reference(tight_pairs(n, 7 + n))


# ---- 1. kernel against the reference ---------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_derivs_match_reference(hip, n):
    """Tile (256) and chunk (2048) edges; 4097 has 3 chunks."""
    b = tight_pairs(n, 7 + n)
    a4, j4 = _derivs(b)
    r = ratios(a4, j4, _pairs_ref(n))
    print(f"n={n} mixed: acc {r[0]:.1f} jerk {r[1]:.1f} phi {r[2]:.1f} (x 2^-24 x scale)")
    assert max(r) <= GATE
    assert not j4[:, 3].any()


def test_fp32_kernel_fails_the_same_inputs(hip):
    """Control: the workload exercises what the mode is for."""
    n = 2049
    a4, _ = _derivs(tight_pairs(n, 7 + n), "fp32")
    ra, _, _, sa, _ = _pairs_ref(n)
    c = worst_ratio(a4[:, :3], ra, sa)
    print(f"n={n} fp32 kernel on the same bodies: acc {c:.3g} (x 2^-24 x scale)")
    assert c > 1000.0 * GATE


# ---- 2. launch shapes --------------------------------------------------------------------------
def test_every_launch_shape_gives_the_same_bits(hip):
    n = 4097
    b = tight_pairs(n, 7 + n)
    fa, fj = _derivs(b)
    for ipl in (1, 2, 4):
        for groups in (1, 2, 3):
            eng = _engine(n, ipl=ipl, split_groups=groups)
            try:
                assert eng.native_layout["ipl"] == ipl
                eng.load(b)
                a4, j4 = eng.derivs()
            finally:
                eng.close()
            assert np.array_equal(a4, fa) and np.array_equal(j4, fj), (ipl, groups)
    assert max(ratios(fa, fj, _pairs_ref(n))) <= GATE


# ---- 3. the pair law ---------------------------------------------------------------------------
def test_coincident_pair_contributes_zero(hip):
    pos = np.array([[1e11, 0, 0], [1e11, 0, 0], [-1e11, 2e10, 0]], dtype=float)
    vel = np.array([[0, 1e4, 0], [0, -2e4, 3e3], [1e3, 0, 0]], dtype=float)
    b = BodySet(pos, vel, np.array([1e25, 2e25, 3e25]))
    a4, j4 = _derivs(b)
    assert np.isfinite(a4).all() and np.isfinite(j4).all()
    ref = reference(b)
    # each coincident body feels the third body only
    only3 = oracle.acc_jerk(ds_seen(pos[[0, 2]]), vel[[0, 2]], b.mass[[0, 2]])
    assert np.allclose(ref[0][0], only3[0][0], rtol=1e-6, atol=0)
    assert max(ratios(a4, j4, ref)) <= GATE
    assert np.allclose(a4[0, :3], only3[0][0], rtol=1e-5, atol=0)


@pytest.mark.parametrize("family", ["solar_random", "random_cube"])
def test_softening_matches_reference(hip, family):
    """softening = 1e9 m, with and without the hard cutoff, as tests/test_hermite_gpu.py
    test_softening_matches_oracle: every figure at the gate but the potential of the Sun
    (solar_random row 0), whose own term -mu / eps swamps the others in an fp32 chunk sum
    whoever does the sum. The chunk sums of this mode are fp32, so that row is asserted as
    there: against the bound of a sequential fp32 sum of n terms, (n - 1) eps sum |terms|, and
    at the gate against the CPU engine of the same mode, which sums in the same order."""
    n = 1000
    b = getattr(ic, family)(n, 11)
    for kw in (dict(softening=1e9), dict(softening=1e9, cutoff=0.0)):
        ra, rj, rphi, sa, sj = reference(b, **kw)
        a4, j4 = _derivs(b, **kw)
        assert np.isfinite(a4).all() and np.isfinite(j4).all()
        assert worst_ratio(a4[:, :3], ra, sa) <= GATE
        assert worst_ratio(j4[:, :3], rj, sj) <= GATE
        lo = 0
        if family == "solar_random":
            lo = 1
            sun = worst_ratio(a4[:1, 3], rphi[:1], np.abs(rphi[:1]))
            _, _, cphi = acc_jerk(b.pos, b.vel, b.mass, device="cpu", dtype="mixed", **kw)
            vs_cpu = worst_ratio(a4[:1, 3], cphi[:1], np.abs(rphi[:1]))
            print(f"mixed phi of the Sun, softened: {sun:.1f} x eps x scale against the "
                  f"reference, {vs_cpu:.2f} against the mixed CPU engine")
            assert sun <= n - 1
            assert vs_cpu <= GATE
        assert worst_ratio(a4[lo:, 3], rphi[lo:], np.abs(rphi[lo:])) <= GATE


def test_pair_that_differs_in_the_lo_parts_only_interacts(hip):
    """x = 1.5e11 and 1.5e11 + 100: one fp32 ulp there is 16384 m, so the hi parts are equal and
    the separation lives in the lo parts alone."""
    pos = np.array([[1.5e11, 2e10, 0], [1.5e11 + 100.0, 2e10, 0], [-1e11, 2e10, 1e10]])
    vel = np.array([[0, 1e4, 0], [0, 1e4 + 50.0, 0], [1e3, 0, 0]], dtype=float)
    b = BodySet(pos, vel, np.array([1e20, 2e20, 3e25]))
    assert np.array_equal(pos[0].astype(F32), pos[1].astype(F32))
    a4, j4 = _derivs(b)
    ref = reference(b)
    assert max(ratios(a4, j4, ref)) <= GATE
    want = G_SI * 2e20 / 100.0 ** 2  # body 0 is pulled towards +x by body 1
    assert a4[0, 0] > 0 and abs(a4[0, 0] / want - 1.0) < 1e-5
    a32, _ = _derivs(b, "fp32")  # control: to fp32 the two coincide
    assert abs(a32[0, 0]) < 1e-3 * want


# ---- 4. round trip -----------------------------------------------------------------------------
def test_state_round_trip_is_bit_exact(hip):
    n = 300
    b = tight_pairs(n, 5)
    b.pos += np.random.default_rng(1).uniform(-1, 1, b.pos.shape)  # metres beside 1e11
    assert (b.pos != b.pos.astype(F32)).all() and (b.vel != b.vel.astype(F32)).any()
    eng = _engine(n)
    try:
        eng.load(b)
        s = eng.state()
        assert np.array_equal(s.pos, b.pos) and np.array_equal(s.vel, b.vel)
        assert np.array_equal(s.mass, b.mass)
        eng.derivs()  # (the split pass leaves the state alone)
        s = eng.state()
        assert np.array_equal(s.pos, b.pos) and np.array_equal(s.vel, b.vel)
    finally:
        eng.close()


# ---- 5. block paths ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _block_paths(n):
    b = tight_pairs(n, 7 + n)
    eng = _engine(n, dt=3600.0, eta=0.02, block_steps=True)
    try:
        eng.load(b)
        eng.set_block_tuning(narrow_max=n)
        full = eng.derivs()
        every = np.arange(n, dtype=np.int32)
        narrow = eng.derivs(active=every, path="narrow")
        wide = eng.derivs(active=every, path="wide")
        perm = np.random.default_rng(100 + n).permutation(n)
        some = {m: np.sort(perm[:m]).astype(np.int32) for m in (1, 4, 5, 64) if m <= n}
        parts = {m: {p: eng.derivs(active=idx, path=p) for p in ("narrow", "wide")}
                 for m, idx in some.items()}
        # body i alone, among 7 others, and in another slot
        i = int(perm[0])
        others = np.array([k for k in perm[1:8]], dtype=np.int32)
        alone = eng.derivs(active=[i], path="narrow")
        first = eng.derivs(active=np.concatenate([[i], others]).astype(np.int32), path="narrow")
        last = eng.derivs(active=np.concatenate([others, [i]]).astype(np.int32), path="narrow")
        return dict(full=full, narrow=narrow, wide=wide, some=some, parts=parts, i=i,
                    alone=alone, first=first, last=last, n_others=len(others))
    finally:
        eng.close()


@pytest.mark.parametrize("n", [257, 2049])
def test_narrow_bits_depend_on_the_body_alone(hip, n):
    r = _block_paths(n)
    i, k = r["i"], r["n_others"]
    for c in (0, 1):
        assert np.array_equal(r["alone"][c][0], r["narrow"][c][i])
        assert np.array_equal(r["first"][c][0], r["narrow"][c][i])
        assert np.array_equal(r["last"][c][k], r["narrow"][c][i])
    for m, idx in r["some"].items():
        assert np.array_equal(r["parts"][m]["narrow"][0], r["narrow"][0][idx]), m
        assert np.array_equal(r["parts"][m]["narrow"][1], r["narrow"][1][idx]), m


@pytest.mark.parametrize("n", [3, 257, 2049])
def test_wide_bits_are_the_shared_step_kernels(hip, n):
    r = _block_paths(n)
    assert np.array_equal(r["wide"][0], r["full"][0]) and np.array_equal(r["wide"][1], r["full"][1])
    for m, idx in r["some"].items():
        assert np.array_equal(r["parts"][m]["wide"][0], r["full"][0][idx]), m
        assert np.array_equal(r["parts"][m]["wide"][1], r["full"][1][idx]), m


def test_narrow_path_matches_reference(hip):
    n = 2049
    r, ref = _block_paths(n), _pairs_ref(n)
    for m, idx in r["some"].items():
        a4, j4 = r["parts"][m]["narrow"]
        q = ratios(a4, j4, ref, idx)
        print(f"n={n} mixed narrow n_act={m}: acc {q[0]:.1f} jerk {q[1]:.1f} phi {q[2]:.1f}")
        assert a4.shape == (m, 4) and max(q) <= GATE and not j4[:, 3].any()
    q = ratios(*r["narrow"], ref)
    print(f"n={n} mixed narrow, every body: acc {q[0]:.1f} jerk {q[1]:.1f} phi {q[2]:.1f}")
    assert max(q) <= GATE


def test_all_at_level_0_is_the_shared_step_bit_for_bit(hip):
    """Slow, widely spaced bodies and dt = 1 s: every body stays at level 0, a block step is a
    shared step, and with the wide path the bits are the same."""
    n, K = 700, 3
    b = ic.solar_random(n, 12)
    out = []
    for block in (True, False):
        eng = _engine(n, dt=1.0, eta=0.02, block_steps=block)
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
        finally:
            eng.close()
    for x, y in zip(*out):
        assert np.array_equal(x, y)
    assert (out[0][0] != b.pos).any()


# ---- 6. dynamics on the device chain -----------------------------------------------------------
def test_offset_binary_energy(hip):
    b, T = offset_binary(1e7)
    out = {}
    for dtype in ("mixed", "fp32"):
        st, status, _ = run_sim(b, dtype, dt=T / 400, steps=800)
        assert status.steps == 800
        out[dtype] = binary_drift(b, st)
    print(f"relative energy error of the binary after 2 periods: {out}")
    assert out["mixed"] <= 1e-6
    assert out["fp32"] >= 1e-3  # control


def test_sub_ulp_motion(hip):
    pos = np.array([[1.5e11, 0, 0], [7.5e11, 0, 0]], dtype=float)
    vel = np.array([[1.0, 0, 0], [0, 0, 0]], dtype=float)
    b = BodySet(pos, vel, np.array([1.0, 1.0]))
    st, _, _ = run_sim(b, "mixed", dt=1.0, steps=100)
    assert abs((st.pos[0, 0] - 1.5e11) - 100.0) <= 1e-6
    st32, _, _ = run_sim(b, "fp32", dt=1.0, steps=100)
    assert st32.pos[0, 0] == float(F32(1.5e11))  # control: 1 m is far below the ulp of 16 km


def test_adaptive_step_lands_on_t_end(hip):
    b, T = offset_binary(1e7)
    st, status, m = run_sim(b, "mixed", dt=T / 8, steps=2000, eta=0.02, t_end=T)
    assert status.finished and status.time == T == m.time_reached
    assert 8 < status.steps < 2000 and 0 < status.dt_min < T / 8 and m.dt_min == status.dt_min
    print(f"adaptive, one period in {status.steps} steps, dt_min {status.dt_min:.3g} s: "
          f"energy error of the binary {binary_drift(b, st):.3e}")
    assert np.isfinite(st.pos).all()


def test_block_steps_track_the_fp64_engine(hip):
    b, T = offset_binary(1e7)
    b = BodySet(np.vstack([b.pos, np.zeros((1, 3))]), np.vstack([b.vel, np.zeros((1, 3))]),
                np.append(b.mass, 1.989e30))
    out = {}
    for dtype in ("mixed", "fp64"):
        st, status, _ = run_sim(b, dtype, dt=T / 8, steps=16, eta=0.02, block_steps=True)
        assert status.time == 16 * (T / 8)
        out[dtype] = (binary_drift(b, st), status)
    (dm, sm), (d64, s64) = out["mixed"], out["fp64"]
    print(f"binary energy drift over 2 periods, block steps: mixed {dm:.3e} fp64 {d64:.3e}; "
          f"body_steps {sm.body_steps} / {s64.body_steps}, level_max {sm.level_max} / "
          f"{s64.level_max}")
    assert dm <= d64 + 1e-6
    assert abs(sm.level_max - s64.level_max) <= 1 and sm.level_max > 0
    assert sm.level_clamped == 0 and sm.body_steps > 16 * 3


# ---- 7. the GPU against the CPU engine of the same mode ----------------------------------------
def test_gpu_and_cpu_engines_agree(hip):
    """Both evaluate within the gate of the one reference (they differ in the rounding of the
    reciprocal square root, so not bit for bit). Then 5 fixed steps of 0.5 s: a binary of
    tight_pairs (separation 1e6 m, masses up to 1e25 kg) accelerates at up to 670 m/s^2; one
    fp32 ulp in r^-1 is 1.8e-7 of s = mu r^-3, 1.2e-4 m/s^2, which over 2.5 s moves a body by
    4e-4 m: below 1e-9 of the separation of the closest bodies."""
    n, sep = 1000, 1e6
    b = tight_pairs(n, 7 + n, sep=sep)
    ref = reference(b)
    cfg = SimConfig(n=n, dtype="mixed", dt=0.5, integrator="hermite")
    out = []
    for eng in (HermiteHipEngine(cfg.replace(device="gpu")),
                HermiteCpuEngine(cfg.replace(device="cpu"))):
        try:
            eng.load(b)
            r = ratios(*eng.derivs(), ref)
            print(f"{eng.kind} mixed n={n}: acc {r[0]:.1f} jerk {r[1]:.1f} phi {r[2]:.1f}")
            assert max(r) <= GATE
            eng.step(5)
            assert eng.status().time == 2.5
            out.append(eng.state())
        finally:
            eng.close()
    d = np.abs(out[0].pos - out[1].pos).max()
    print(f"after 5 steps the engines differ by {d:.3g} m")
    assert d <= 1e-9 * sep
    assert (out[0].pos != b.pos).any()


# ---- 8. checkpoints ----------------------------------------------------------------------------
@pytest.mark.parametrize("block", [False, True])
def test_gpu_resume_is_bit_exact(hip, tmp_path, block):
    kw = dict(n=200, eta=0.02, block_steps=True, softening=1e9, dt=8 * 86400.0, init="plummer",
              seed=9) if block else dict(n=3000, eta=0.02, dt=4e5)
    cfg = SimConfig(steps=3, dtype="mixed", device="gpu", integrator="hermite", **kw)
    whole = Simulation(cfg.replace(steps=6))
    whole.run()
    ref, ref_st, ref_carried = whole.global_state(), whole.engine.status(), whole.engine.carried()
    ref_lev = whole.engine.levels() if block else None
    whole.close()
    sim = Simulation(cfg)
    sim.run()
    path = str(tmp_path / "c.gsck")
    sim.save_checkpoint(path)
    sim.close()
    from gravsim.utils import checkpoint as ckpt

    assert ckpt.load(path).meta["dtype"] == "mixed"
    sim2 = Simulation(cfg.replace(resume=path))
    sim2.run(3)
    got, got_st = sim2.global_state(), sim2.engine.status()
    try:
        assert np.array_equal(got.pos, ref.pos) and np.array_equal(got.vel, ref.vel)
        assert all(np.array_equal(x, y) for x, y in zip(sim2.engine.carried(), ref_carried))
        assert (got_st.time, got_st.dt_next) == (ref_st.time, ref_st.dt_next)
        assert sim2.step == 6
        if block:  # (dt_min is dt 2^-level_max of the levels seen since the state was set)
            assert np.array_equal(sim2.engine.levels(), ref_lev)
        else:
            assert got_st.dt_min == ref_st.dt_min and ref_st.dt_last < cfg.dt
    finally:
        sim2.close()


# ---- 9. refusals -------------------------------------------------------------------------------
def test_refusals(hip):
    from gravsim.runtime.engines import _gs_config

    cfg = SimConfig(n=64, dtype="mixed", device="gpu", integrator="hermite")
    c = _gs_config(cfg, 0, 1, 0)
    assert c.dtype == _native.GS_MIXED
    s = ctypes.c_void_p()
    assert hip.gs_stepper_create(ctypes.byref(c), ctypes.byref(s)) != 0 and not s.value
    assert b"mixed" in hip.gs_last_error()
    L = _native.GsLayout()
    assert hip.gs_layout_compute(ctypes.byref(c), ctypes.byref(L)) != 0
    assert b"mixed" in hip.gs_last_error()
    c.dtype = 7
    h = ctypes.c_void_p()
    assert hip.gs_hermite_create(ctypes.byref(c), ctypes.byref(h)) != 0 and not h.value
    assert b"dtype" in hip.gs_last_error()
    with pytest.raises(ValueError, match="hermite runs on one rank"):
        Simulation(cfg, comm.DistInfo(rank=1, world=2))
    with pytest.raises(ValueError):
        HermiteHipEngine(cfg, 0, 2)
