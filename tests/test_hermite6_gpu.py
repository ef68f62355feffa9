"""The gfx950 acceleration+jerk+snap kernel of the 6th-order Hermite scheme and its device-side
step chain against the NumPy oracle and the native CPU engine: tile and chunk edges, the pair
law, bitwise launch-shape independence, the step chain, the order of accuracy, the driver,
checkpoints, the native refusals, and one step from a state the test chose (section 7).

Accuracy gates: |err| <= 128 eps sum_j |term_ij| (the project's gate), with the snap's scale from
oracle.acc_jerk_snap(with_abs=True). The reference is the oracle on the inputs as the kernel sees
them: positions, velocities and mu rounded to the dtype, and for the snap the acceleration rows
the kernel's second pass read, which are its own first-pass output."""
import ctypes

import numpy as np
import pytest

from gravsim.config import G_SI, SimConfig
from gravsim.models import initial_conditions as ic
from gravsim.models.initial_conditions import BodySet
from gravsim.ops import _native, oracle
from gravsim.ops.force import acc_jerk_snap
from gravsim.runtime.hermite import HermiteCpuEngine, HermiteHipEngine
from gravsim.runtime.simulation import Simulation

import hermite6_helpers as h6
import hermite6_probe_helpers as h6p

pytestmark = pytest.mark.gpu

EPS = {"fp32": 2.0 ** -24, "fp64": 2.0 ** -53}
SIZES = [1, 2, 3, 255, 256, 257, 1000, 2047, 2048, 2049, 4097]


def _engine(n, dtype="fp64", **kw):
    kw.setdefault("integrator", "hermite")
    kw.setdefault("hermite_order", 6)
    return HermiteHipEngine(SimConfig(n=n, dtype=dtype, device="gpu", **kw).validate())


def _derivs(b, dtype, **kw):
    eng = _engine(b.n, dtype, **kw)
    try:
        eng.load(b)
        return eng.derivs()
    finally:
        eng.close()


def quantized_ref(b, dtype, acc_in, **kw):
    """Oracle on the inputs as the kernel sees them; acc_in: the acceleration rows it read."""
    T = np.float32 if dtype == "fp32" else np.float64
    p = b.pos.astype(T).astype(np.float64)
    v = b.vel.astype(T).astype(np.float64)
    mu = (G_SI * b.mass).astype(T).astype(np.float64)
    return oracle.acc_jerk_snap(p, v, np.asarray(acc_in, dtype=T).astype(np.float64), mu, G=1.0,
                                with_potential=True, with_abs=True, **kw)


def worst_ratio(got, ref, scale, dtype):
    return float((np.abs(got - ref) / (EPS[dtype] * scale + 1e-300)).max())


def ratios(b, dtype, a4, j4, s4, **kw):
    ra, rj, rs, rphi, sa, sj, ss = quantized_ref(b, dtype, a4[:, :3], **kw)
    return (worst_ratio(a4[:, :3], ra, sa, dtype), worst_ratio(j4[:, :3], rj, sj, dtype),
            worst_ratio(s4[:, :3], rs, ss, dtype), worst_ratio(a4[:, 3], rphi, np.abs(rphi), dtype))


# ---- 1. kernel against the oracle --------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_derivs_match_oracle(hip, n, dtype):
    b = ic.solar_random(n, seed=7 + n)
    a4, j4, s4 = _derivs(b, dtype)
    r = ratios(b, dtype, a4, j4, s4)
    print(f"n={n} {dtype}: acc {r[0]:.1f} jerk {r[1]:.1f} snap {r[2]:.1f} phi {r[3]:.1f} "
          "(x eps x scale)")
    assert max(r) <= 128.0
    assert not j4[:, 3].any() and not s4[:, 3].any()


def test_one_shot_entry_matches_the_cpu_engine(hip):
    b = ic.solar_random(300, 4)
    g = acc_jerk_snap(b.pos, b.vel, b.mass, device="gpu", dtype="fp64")
    c = acc_jerk_snap(b.pos, b.vel, b.mass, device="cpu", dtype="fp64")
    for got, ref, tol in zip(g, c, (1e-11, 1e-9, 1e-8, 1e-13)):
        assert np.allclose(got, ref, rtol=tol, atol=0)


# ---- 2. the pair law ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_coincident_pair_contributes_zero(hip, dtype):
    pos = np.array([[1e11, 0, 0], [1e11, 0, 0], [-1e11, 2e10, 0]], dtype=float)
    vel = np.array([[0, 1e4, 0], [0, -2e4, 3e3], [1e3, 0, 0]], dtype=float)
    b = BodySet(pos, vel, np.array([1e25, 2e25, 3e25]))
    a4, j4, s4 = _derivs(b, dtype)
    assert np.isfinite(a4).all() and np.isfinite(j4).all() and np.isfinite(s4).all()
    # each coincident body feels the third body only: the oracle of the pair (0, 2) alone
    ra, rj, rs, rphi, sa, sj, ss = quantized_ref(b, dtype, a4[:, :3])
    sub = BodySet(pos[[0, 2]], vel[[0, 2]], b.mass[[0, 2]])
    only3 = quantized_ref(sub, dtype, a4[[0, 2], :3])
    for k in range(3):
        assert np.allclose(only3[k][0], (ra, rj, rs)[k][0], rtol=1e-12)
    assert max(ratios(b, dtype, a4, j4, s4)) <= 128.0


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_body_at_origin_beside_ghost_rows(hip, dtype):
    """Ghost rows sit at the origin, massless, at rest and unaccelerated: a real body there
    meets them at r = 0, and they add exactly zero to a, j and s."""
    pos = np.array([[0, 0, 0], [1.5e11, 0, 0], [0, -2e11, 1e10]], dtype=float)
    vel = np.array([[0, 0, 0], [0, 3e4, 0], [2e4, 0, 0]], dtype=float)
    b = BodySet(pos, vel, np.array([2e30, 6e24, 6e23]))
    eng = _engine(3, dtype, dt=3600.0)
    try:
        eng.load(b)
        a4, j4, s4 = eng.derivs()
        assert np.isfinite(a4).all() and np.isfinite(j4).all() and np.isfinite(s4).all()
        assert max(ratios(b, dtype, a4, j4, s4)[:3]) <= 128.0
        eng.step(3)
        assert eng.nonfinite() == 0 and np.isfinite(eng.state().pos).all()
        assert all(np.isfinite(r).all() for r in eng.carried())
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_softening_matches_oracle(hip, dtype):
    """softening = 1e9 m, with and without the hard cutoff: a, j, s at the 128 eps scale gate
    (phi is the 4th-order test's, with its one excused figure, and is not repeated here)."""
    b = ic.random_cube(1000, 11)
    for kw in (dict(softening=1e9), dict(softening=1e9, cutoff=0.0)):
        a4, j4, s4 = _derivs(b, dtype, **kw)
        r = ratios(b, dtype, a4, j4, s4, **kw)
        print(f"{dtype} {kw}: acc {r[0]:.1f} jerk {r[1]:.1f} snap {r[2]:.1f}")
        assert max(r[:3]) <= 128.0


# ---- 3. bits -----------------------------------------------------------------------------
def _built_ipls(hip, dtype):
    return [i for i in (1, 2, 4) if hip.gs_hermite6_ipl_ok(int(dtype == "fp64"), i)]


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("n", [4097, 10000])
def test_every_launch_shape_gives_the_same_bits(hip, dtype, n):
    """n = 4097: 3 chunks of 2048 (the last almost all ghosts); n = 10,000: 5 chunks. Every built
    IPL x 1, 2, 3, 5 chunk groups, the auto shape, and (n = 4097) a 20-step adaptive run."""
    b = ic.solar_random(n, seed=3)

    def run(ipl, groups):
        eng = _engine(n, dtype, dt=4e5, eta=0.25, ipl=ipl, split_groups=groups)
        try:
            assert ipl == 0 or eng.native_layout["ipl"] == ipl
            assert eng.native_layout["n_chunks"] == (3 if n == 4097 else 5)
            eng.load(b)
            out = list(eng.derivs())
            if n == 4097:
                eng.step(20)
                st, s = eng.status(), eng.state()
                assert st.steps == 20
                out += [s.pos, s.vel, *eng.carried(), np.array([st.time, st.dt_last, st.dt_next])]
            return out
        finally:
            eng.close()

    ipls = _built_ipls(hip, dtype)
    assert ipls == ([1, 2] if dtype == "fp32" else [1])
    ref = run(0, 0)
    for ipl in ipls:
        for g in (1, 2, 3, 5):
            for x, y in zip(run(ipl, g), ref):
                assert np.array_equal(x, y), (ipl, g)


# ---- 4. the step chain -------------------------------------------------------------------
def test_step_chain_matches_the_oracle(hip):
    eng = _engine(h6.CASE_N, "fp64", dt=h6.CASE_DT, eta=h6.CASE_ETA, t_end=h6.adaptive_case()[1])
    try:
        h6.check_against_oracle(eng)
    finally:
        eng.close()


def test_gpu_and_cpu_engines_agree(hip):
    b = ic.solar_random(300, 5)
    kw = dict(n=300, dt=4e5, eta=0.25, dtype="fp64", integrator="hermite", hermite_order=6)
    g, c = HermiteHipEngine(SimConfig(device="gpu", **kw)), HermiteCpuEngine(SimConfig(device="cpu",
                                                                                       **kw))
    try:
        for e in (g, c):
            e.load(b)
            e.step(40)
        x, y = g.state().pos, c.state().pos
        d = float(np.abs(x - y).max() / np.abs(y).max())
        print(f"GPU fp64 against CPU fp64 after 40 steps: {d:.2e} of max |x|")
        assert d <= 1e-10
        assert abs(g.status().time - c.status().time) <= 1e-9 * c.status().time
        assert g.status().steps == c.status().steps == 40
    finally:
        g.close()


@pytest.mark.parametrize("n", [1, 2])
def test_smallest_systems_and_end_times(hip, n):
    """n = 1 moves on a straight line whatever the step rule; n = 2 follows the oracle with a
    fixed step, with t_end on a step boundary and with t_end inside a step."""
    b = h6.two_body(0.5)[0] if n == 2 else BodySet(np.array([[1e11, 2e10, 0.0]]),
                                                   np.array([[1e3, -2e3, 5e2]]), np.array([1e25]))
    dt = 36000.0
    for eta, t_end, steps in ((0.0, None, 7), (0.0, 5 * dt, 5), (0.0, 4.3 * dt, 5),
                              (0.25, 4.3 * dt, None)):
        eng = _engine(n, "fp64", dt=dt, eta=eta, t_end=t_end)
        try:
            eng.load(b)
            eng.step(12 if t_end is not None else steps)
            st, s = eng.status(), eng.state()
            x, v, _, t, taken = oracle.simulate_hermite6(b.pos, b.vel, b.mass, dt,
                                                         12 if t_end is not None else steps,
                                                         eta=eta, t_end=t_end)
            assert st.steps == len(taken) and (steps is None or st.steps == steps)
            assert st.time == t and st.finished == (t_end is not None)
            assert np.abs(s.pos - x).max() <= 1e-12 * np.abs(x).max()
            if n == 1:
                assert np.allclose(s.pos, b.pos + b.vel * t, rtol=1e-14, atol=0)
                assert not any(r.any() for r in eng.carried())
        finally:
            eng.close()


def test_order_of_the_gpu_engine(hip):
    o = h6.orders(h6.engine_positions(HermiteHipEngine, "gpu"))
    print(f"orders on the GPU, fp64: {o[0]:.2f} {o[1]:.2f}")
    assert 5.7 <= o[0] <= 6.3 and 5.7 <= o[1] <= 6.3


# ---- 5. the driver -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_simulation_resume_is_bit_exact(hip, tmp_path, dtype):
    cfg = SimConfig(n=1500, dt=4e5, eta=0.25, steps=8, dtype=dtype, device="gpu", seed=9,
                    integrator="hermite", hermite_order=6, diagnostics=True, structure=True)
    whole = Simulation(cfg)
    m = whole.run()
    ref, ref_st, ref_rows = whole.global_state(), whole.engine.status(), whole.engine.carried()
    whole.close()
    assert m.hermite_order == 6 and m.steps_taken == 8
    assert np.isfinite(m.extra["conservation"]["energy_rel_drift"])
    assert len(m.structure["samples"]) == 2
    first = Simulation(cfg.replace(diagnostics=False, structure=False))
    first.run(5)
    path = first.save_checkpoint(str(tmp_path / "c.gsck"))
    first.close()
    second = Simulation(cfg.replace(diagnostics=False, structure=False, resume=path))
    assert second.step == 5 and not second.order_restart
    second.run(3)
    got, got_st, rows = second.global_state(), second.engine.status(), second.engine.carried()
    second.close()
    assert np.array_equal(got.pos, ref.pos) and np.array_equal(got.vel, ref.vel)
    assert all(np.array_equal(x, y) for x, y in zip(rows, ref_rows)) and len(rows) == 4
    assert (got_st.time, got_st.dt_next) == (ref_st.time, ref_st.dt_next)
    assert ref_st.dt_last < cfg.dt  # the criterion, not the ceiling, chose the steps


# ---- 6. what order 6 leaves out ----------------------------------------------------------
def test_native_refusals_name_the_option(hip):
    from gravsim.runtime.engines import _gs_config

    def create(cfg, nranks=1):
        c = _gs_config(cfg, 0, nranks, 0)
        h = ctypes.c_void_p()
        assert hip.gs_hermite_create(ctypes.byref(c), ctypes.byref(h)) == 0, hip.gs_last_error()
        assert hip.gs_hermite_set_adaptive(h, 0.25, 3600.0, -1.0) == 0
        return h

    base = SimConfig(n=2048, device="gpu", softening=1e6)
    h = create(base)
    try:
        assert hip.gs_hermite_get_order(h) == 4
        assert hip.gs_hermite_set_order(h, 5) != 0 and b"4 or 6" in hip.gs_last_error()
        assert hip.gs_hermite_set_order(h, 6) == 0 and hip.gs_hermite_get_order(h) == 6
        assert hip.gs_hermite_set_block(h, 1, 10) != 0
        assert b"gs_hermite_set_block" in hip.gs_last_error()
        assert hip.gs_hermite_set_collisions(h, 1) != 0
        assert b"gs_hermite_set_collisions" in hip.gs_last_error()
        arr = (ctypes.c_void_p * 1)(h)
        assert hip.gs_hermite_group_step(arr, 1, 1) != 0 and b"group" in hip.gs_last_error()
        # back to order 4, block steps on: order 6 is then refused
        assert hip.gs_hermite_set_order(h, 4) == 0 and hip.gs_hermite_get_order(h) == 4
        assert hip.gs_hermite_set_block(h, 1, 10) == 0
        assert hip.gs_hermite_set_order(h, 6) != 0 and b"gs_hermite_set_block" in hip.gs_last_error()
        assert hip.gs_hermite_set_block(h, 0, 0) == 0
        assert hip.gs_hermite_set_collisions(h, 1) == 0
        assert hip.gs_hermite_set_order(h, 6) != 0
        assert b"gs_hermite_set_collisions" in hip.gs_last_error()
    finally:
        hip.gs_hermite_destroy(h)
    h = create(base.replace(dtype="mixed", integrator="hermite"))
    try:
        assert hip.gs_hermite_set_order(h, 6) != 0 and b"GS_MIXED" in hip.gs_last_error()
    finally:
        hip.gs_hermite_destroy(h)
    h = create(base, nranks=2)
    try:
        assert hip.gs_hermite_set_order(h, 6) != 0 and b"nranks > 1" in hip.gs_last_error()
    finally:
        hip.gs_hermite_destroy(h)
    with pytest.raises(ValueError, match="--gpus"):
        HermiteHipEngine(SimConfig(n=2048, device="gpu", integrator="hermite", hermite_order=6),
                         0, 2)


# ---- order 6 switched on and off again: the order-4 run is untouched ----------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_order_6_then_4_is_the_fresh_order_4_run(hip, dtype):
    """gs_hermite_set_order(6) then (4) on an order-4 engine leaves the launch shape and, after
    load() and 3 adaptive steps, every bit of state(), carried() and status() as a fresh order-4
    engine has them: the path through the launch shape and the frees of the order's arrays."""
    n = 2049
    b = ic.solar_random(n, seed=7 + n)

    def run(switch):
        eng = _engine(n, dtype, hermite_order=4, dt=3600.0, eta=0.05)
        try:
            if switch:
                for order in (6, 4):
                    assert hip.gs_hermite_set_order(eng._h, order) == 0, hip.gs_last_error()
                    assert hip.gs_hermite_get_order(eng._h) == order
            L = _native.GsLayout()
            assert hip.gs_hermite_layout(eng._h, ctypes.byref(L)) == 0
            eng.load(b)
            eng.step(3)
            eng.sync()
            s = eng.state()
            return (s.pos, s.vel, s.mass) + tuple(eng.carried()), eng.status(), \
                (L.as_dict()["ipl"], L.as_dict()["split_groups"])
        finally:
            eng.close()

    rows_a, st_a, shape_a = run(False)
    rows_b, st_b, shape_b = run(True)
    assert shape_a == shape_b
    assert st_a == st_b and st_a.steps == 3
    for x, y in zip(rows_a, rows_b):
        assert x.tobytes() == y.tobytes()


# ---- 7. one step from a supplied state ----------------------------------------------------
@pytest.mark.parametrize("n", h6p.STEP_SIZES)
@pytest.mark.parametrize("dtype,ipl", [("fp32", 1), ("fp32", 2), ("fp64", 1)])
def test_one_step_from_a_supplied_state(hip, n, dtype, ipl):
    """The evaluate kernel reads acceleration rows the test chose, inside the step chain: the
    state is (x0, 0, A0, 0, 0, 0) with A0 unrelated to any kernel output and h = 1024 s, so the
    predicted rows are known to the bit (h6p.supplied_state). After step(1): a1, j1, s1 against
    oracle.acc_jerk_snap at those rows at 128 eps scale (the gated launch, the HM_STEP reduce and
    the predict kernel's AP; n_pad holds 1048, 2047 and 2047 ghost rows), v1 and x1 against
    h6_correct at 10 roundings, the crackle against oracle.hermite6_high at one rounding, and
    dt_next against oracle.hermite6_dt at 1e-9 (h6p.check_supplied_step). The CPU engine passes
    the same gates (tests/test_hermite6_probe_cpu.py) and stands at the same time and step."""
    kw = dict(n=n, dtype=dtype, integrator="hermite", hermite_order=6, dt=h6p.STEP_H,
              eta=h6p.STEP_ETA)
    eng = HermiteHipEngine(SimConfig(device="gpu", ipl=ipl, **kw).validate())
    try:
        assert eng.native_layout["ipl"] == ipl
        out = h6p.check_supplied_step(eng, n, dtype, label=f"step n {n} {dtype} ipl {ipl}")
    finally:
        eng.close()
    print(f"step n={n} {dtype} ipl {ipl}: {h6p.fmt(out['worst'])}; v1 {out['v']:.2f} x1 "
          f"{out['x']:.2f} of {h6p.CORRECT_ROUNDINGS} u sum |terms|; crackle {out['crackle']:.2f} "
          f"of its bound; dt_next {out['dt_next']:.6g} ({out['dt_rel']:.1e} relative), body "
          f"{out['row']}")
    cpu = HermiteCpuEngine(SimConfig(device="cpu", **kw).validate())
    ref = h6p.check_supplied_step(cpu, n, dtype, label=f"cpu step n {n} {dtype}")
    g, c = out["status"], ref["status"]
    assert (g.time, g.steps) == (c.time, c.steps) == (h6p.STEP_H, 1)
    # (dt_next is gated on each engine's own rows above: in fp32 the two engines' a1, j1, s1
    # differ by their rounding, and the steps they ask for with them, by about 1e-7)
    if n == 1000 and ipl == 1:  # a fixed step of the same size: the same rows, the ceiling next
        fixed = HermiteHipEngine(SimConfig(device="gpu", **dict(kw, eta=0.0)).validate())
        try:
            st = h6p.supplied_case(n, dtype)[0]
            fixed.load(st["bodies"], **st["load"])
            fixed.step(1)
            s = fixed.state()
            for x, y in zip((s.pos, s.vel) + tuple(fixed.carried()), out["rows"]):
                assert np.array_equal(x, y)
            assert fixed.status().dt_next == h6p.STEP_H
        finally:
            fixed.close()
