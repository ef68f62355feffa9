"""Hermite in mixed precision (dtype "mixed": fp64 state, fp32 pair arithmetic on double-single
predicted positions), without a GPU: the config and the CLI, the native CPU engine's
gs_cpu_accjerk_mixed / _idx_mixed / gs_cpu_hermite_step_mixed against the NumPy oracle, and the
two things the mode is for, each with the fp32 engine as the control that fails them: a tight
binary far from the origin, and motion below an fp32 ulp of the coordinate.

Reference: oracle.acc_jerk on the inputs as the pair arithmetic sees them, positions as
hi + lo (ds_seen), velocities and mu rounded to fp32. Gate: |err| <= 128 * 2^-24 * scale, the
scales from with_abs=True and |phi| (tests/test_hermite_gpu.py).
"""
import ctypes
import functools
import math

import numpy as np
import pytest

from gravsim import cli
from gravsim.config import G_SI, SimConfig
from gravsim.models import initial_conditions as ic
from gravsim.models.initial_conditions import BodySet
from gravsim.ops import _native, oracle
from gravsim.ops.force import acc_jerk
from gravsim.parallel.partition import layout
from gravsim.runtime.hermite import HermiteCpuEngine
from gravsim.runtime.simulation import Simulation
from gravsim.utils import checkpoint as ckpt

EPS = 2.0 ** -24
GATE = 128.0
F32, F64 = np.float32, np.float64


# ---- shared helpers (the same in tests/test_hermite_mixed_gpu.py) --------------------------
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


def ratios(a, j, phi, ref, idx=slice(None)):
    ra, rj, rphi, sa, sj = ref
    return (worst_ratio(a, ra[idx], sa[idx]), worst_ratio(j, rj[idx], sj[idx]),
            worst_ratio(phi, rphi[idx], np.abs(rphi[idx])))


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


@functools.lru_cache(maxsize=None)
def _pairs_ref(n):
    return reference(tight_pairs(n, 7 + n))


def run_sim(b, dtype, device="cpu", **kw):
    sim = Simulation(SimConfig(n=b.n, dtype=dtype, device=device, integrator="hermite", **kw))
    try:
        sim.engine.load(b)
        m = sim.run()
        return sim.global_state(), sim.engine.status(), m
    finally:
        sim.close()


# ---- 1. config and CLI -----------------------------------------------------------------------
def test_config_and_cli():
    SimConfig(dtype="mixed", integrator="hermite").validate()
    SimConfig(dtype="mixed", integrator="hermite", ipl=4).validate()  # (the rules of fp32)
    for kw in (dict(integrator="kd"), dict(integrator="leapfrog"), dict(),
               dict(integrator="hermite", ipl=8)):
        with pytest.raises(ValueError):
            SimConfig(dtype="mixed", **kw).validate()
    with pytest.raises(ValueError):
        SimConfig(dtype="fp16", integrator="hermite").validate()
    p = cli.build_parser()
    a = p.parse_args(["--dtype", "mixed", "--integrator", "hermite", "--n", "8"])
    cfg = cli.config_from_args(a)
    assert cfg.dtype == "mixed" and cfg.validate().integrator == "hermite"
    with pytest.raises(SystemExit):
        p.parse_args(["--dtype", "fp16"])
    # the KD engines never see it as fp32
    from gravsim.runtime.engines import _gs_config

    assert _gs_config(cfg, 0, 1, 0).dtype == _native.GS_MIXED == 2


# ---- 2. the native evaluation against the reference ------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 65, 257, 2049])
def test_accjerk_mixed_matches_reference(n):
    b = tight_pairs(n, 7 + n)
    ref = _pairs_ref(n)
    a, j, phi = acc_jerk(b.pos, b.vel, b.mass, device="cpu", dtype="mixed")
    r = ratios(a, j, phi, ref)
    print(f"n={n} mixed: acc {r[0]:.1f} jerk {r[1]:.1f} phi {r[2]:.1f} (x 2^-24 x scale)")
    assert max(r) <= GATE
    if n > 4:  # control: the inputs exercise what the mode is for
        a32, _, _ = acc_jerk(b.pos, b.vel, b.mass, device="cpu", dtype="fp32")
        c = worst_ratio(a32, ref[0], ref[3])
        print(f"n={n} fp32 engine on the same bodies: acc {c:.3g}")
        assert c > 1000.0 * GATE


# ---- 3. the indexed entry ---------------------------------------------------------------------
def test_accjerk_idx_mixed_is_bit_equal_to_the_range_entry():
    n = 700
    lib, P = _native.cpu_lib(), _native.dptr
    b = tight_pairs(n, 3)
    X, V = np.zeros((n, 4)), np.zeros((n, 4))
    X[:, :3], X[:, 3], V[:, :3] = b.pos, G_SI * b.mass, b.vel
    chunk = layout(n, 0, 1, 0).chunk
    fa, fj = np.zeros((n, 4)), np.zeros((n, 4))
    assert lib.gs_cpu_accjerk_mixed(P(X), P(V), n, 0, n, chunk, 1e-20, 0.0, P(fa), P(fj)) == 0
    assert fa[:, :3].any() and not fj[:, 3].any()
    # a sub-range is the same rows
    sa, sj = np.zeros((100, 4)), np.zeros((100, 4))
    assert lib.gs_cpu_accjerk_mixed(P(X), P(V), n, 300, 400, chunk, 1e-20, 0.0, P(sa), P(sj)) == 0
    assert np.array_equal(sa, fa[300:400]) and np.array_equal(sj, fj[300:400])
    rng = np.random.default_rng(2)
    for m in (1, 2, 255, 256, 257, n):
        for idx in (np.sort(rng.permutation(n)[:m]), rng.permutation(n)[:m]):
            idx = idx.astype(np.int32)
            ga, gj = np.full((m, 4), 7.0), np.full((m, 4), 7.0)
            assert lib.gs_cpu_accjerk_idx_mixed(
                P(X), P(V), n, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), m, chunk,
                1e-20, 0.0, P(ga), P(gj)) == 0
            assert np.array_equal(ga, fa[idx]) and np.array_equal(gj, fj[idx]), m
    bad = np.array([n], dtype=np.int32)
    assert lib.gs_cpu_accjerk_idx_mixed(
        P(X), P(V), n, bad.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 1, chunk, 1e-20, 0.0,
        P(fa), P(fj)) != 0


# ---- 4. what the double-single pair loses -----------------------------------------------------
def test_double_single_positions_are_as_good_as_fp64():
    b = tight_pairs(2049, 11, sep=1e6)
    mu = G_SI * b.mass
    raw, _, _, scale, _ = oracle.acc_jerk(b.pos, b.vel, mu, G=1.0, with_potential=True,
                                          with_abs=True)
    seen = oracle.acc_jerk(ds_seen(b.pos), b.vel, mu, G=1.0)[0]
    r = worst_ratio(seen, raw, scale)
    print(f"oracle acc on ds_seen(pos) against raw fp64 positions: {r:.3f} x 2^-24 x scale")
    assert r < 2.0


# ---- 5. a tight binary far from the origin ----------------------------------------------------
def test_offset_binary_energy():
    b, T = offset_binary(1e7)
    out = {}
    for dtype in ("mixed", "fp32"):
        st, status, _ = run_sim(b, dtype, dt=T / 400, steps=800)
        assert status.steps == 800
        out[dtype] = binary_drift(b, st)
    print(f"relative energy error of the binary after 2 periods: {out}")
    assert out["mixed"] <= 1e-6
    assert out["fp32"] >= 1e-3  # control


# ---- 6. motion below an fp32 ulp of the coordinate --------------------------------------------
def test_sub_ulp_motion():
    pos = np.array([[1.5e11, 0, 0], [7.5e11, 0, 0]], dtype=float)
    vel = np.array([[1.0, 0, 0], [0, 0, 0]], dtype=float)
    b = BodySet(pos, vel, np.array([1.0, 1.0]))
    st, _, _ = run_sim(b, "mixed", dt=1.0, steps=100)
    assert abs((st.pos[0, 0] - 1.5e11) - 100.0) <= 1e-6
    st32, _, _ = run_sim(b, "fp32", dt=1.0, steps=100)
    assert st32.pos[0, 0] == float(F32(1.5e11))  # control: 1 m is far below the ulp of 16 km


# ---- 7. block steps ---------------------------------------------------------------------------
def binary_and_sun():
    b, T = offset_binary(1e7)
    return BodySet(np.vstack([b.pos, np.zeros((1, 3))]), np.vstack([b.vel, np.zeros((1, 3))]),
                   np.append(b.mass, 1.989e30)), T


def test_block_steps_track_the_fp64_engine():
    b, T = binary_and_sun()
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


# ---- 8. checkpoints ---------------------------------------------------------------------------
@pytest.mark.parametrize("block", [False, True])
def test_resume_is_bit_exact(tmp_path, block):
    kw = dict(eta=0.02, block_steps=True, softening=1e9, dt=8 * 86400.0) if block else \
        dict(eta=0.02, dt=4e5)
    cfg = SimConfig(n=200, steps=3, dtype="mixed", device="cpu", integrator="hermite", seed=4,
                    **kw)
    whole = Simulation(cfg.replace(steps=6))
    whole.run()
    ref, ref_st = whole.global_state(), whole.engine.status()
    ref_carried = whole.engine.carried()
    sim = Simulation(cfg)
    sim.run()
    path = str(tmp_path / "c.gsck")
    sim.save_checkpoint(path)
    c = ckpt.load(path)
    assert c.meta["dtype"] == "mixed" and c.step == 3
    # the state is fp64: what the file holds is what the engine holds
    assert np.array_equal(c.bodies.pos, sim.global_state().pos)
    assert (c.bodies.pos != c.bodies.pos.astype(F32)).any()
    sim2 = Simulation(cfg.replace(resume=path))
    sim2.run(3)
    got, got_st = sim2.global_state(), sim2.engine.status()
    assert np.array_equal(got.pos, ref.pos) and np.array_equal(got.vel, ref.vel)
    assert all(np.array_equal(x, y) for x, y in zip(sim2.engine.carried(), ref_carried))
    assert (got_st.time, got_st.dt_next) == (ref_st.time, ref_st.dt_next) and sim2.step == 6
    if block:
        assert np.array_equal(sim2.engine.levels(), whole.engine.levels())
    # a file written by another dtype loads as before
    other = Simulation(cfg.replace(dtype="fp64"))
    other.run()
    p2 = str(tmp_path / "d.gsck")
    other.save_checkpoint(p2)
    sim3 = Simulation(cfg.replace(resume=p2))
    assert np.array_equal(sim3.global_state().pos, other.global_state().pos)
    assert sim3.run(1).dtype == "mixed" and sim3.engine.nonfinite() == 0


def test_engine_holds_fp64_state():
    b = tight_pairs(65, 1)
    eng = HermiteCpuEngine(SimConfig(n=65, dtype="mixed", device="cpu",
                                     integrator="hermite").validate())
    eng.load(b)
    s = eng.state()
    assert np.array_equal(s.pos, b.pos) and np.array_equal(s.vel, b.vel)
    a4, j4 = eng.derivs()
    i4, _ = eng.derivs(active=[4, 3])
    assert a4.dtype == np.float64 and np.array_equal(i4, a4[[4, 3]])
