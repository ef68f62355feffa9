"""6th-order Hermite block time steps on the GPU (fp64): the two evaluate paths of a block step
(narrow: parallel over j; wide: the gathered i-owned kernel) against the NumPy oracle and against
their promises about bits, then whole runs against the oracle and the CPU engine, determinism,
checkpoints, and the step chain with the active list spread over many workgroups.

Accuracy gates: |err| <= 128 eps sum_j |term_ij| (tests/test_hermite6_gpu.py), scales from
oracle.acc_jerk_snap(with_abs=True); the snap's reference is taken at the acceleration rows the
kernel read, the carried a of the engine. Runs: the (t, n_active) log and the levels exactly,
positions to 1e-10 of max |x| (docs/DESIGN.md section 21's gate of the fp64 chain). The run
inputs and their seeds are those of tests/test_hermite6_block_cpu.py.
"""
import functools

import numpy as np
import pytest

from gravsim.config import G_SI, SimConfig
from gravsim.models import initial_conditions as ic
from gravsim.models.initial_conditions import BodySet
from gravsim.ops import oracle
from gravsim.runtime.hermite import HermiteCpuEngine, HermiteHipEngine
from gravsim.runtime.simulation import Simulation

import test_hermite6_block_cpu as cpu6  # (its inputs and oracle runs; no GPU needed)

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
SIZES = [3, 257, 2049, 4097]  # 2049: three chunks of 1024; 4097: five narrow slices, the last
#                               of 1024 rows holding one real body
DAY = 86400.0
DT, ETA, SOFT = cpu6.DT, cpu6.ETA, cpu6.SOFT


def _engine(n, block=True, **kw):
    kw.setdefault("eta", ETA)
    kw.setdefault("hermite_order", 6)
    kw["block_steps6" if kw["hermite_order"] == 6 else "block_steps"] = block
    return HermiteHipEngine(SimConfig(n=n, dtype="fp64", device="gpu", integrator="hermite",
                                      **kw).validate())


def active_lists(n):
    """One body, five (two groups of kNarrowGroup6 = 2 and a partial one), every body, and a list
    of up to 7 that ends in the last real row."""
    perm = np.random.default_rng(100 + n).permutation(n)
    head = perm[:6]
    tail = np.sort(np.append(head[head != n - 1], n - 1))
    out = {"one": perm[:1], "five": np.sort(perm[: min(n, 5)]), "all": np.arange(n), "tail": tail}
    return {k: v.astype(np.int32) for k, v in out.items()}


def worst(got, ref, scale):
    return float((np.abs(got - ref) / (EPS * scale + 1e-300)).max())


@functools.lru_cache(maxsize=None)
def _paths(n):
    """One engine per n: the carried acceleration, derivs() (gs_hermite_derivs6) and, for every
    active list, the rows of both block paths."""
    b = ic.solar_random(n, seed=7 + n)
    eng = _engine(n, dt=3600.0)
    try:
        eng.load(b)
        eng.set_block_tuning(narrow_max=n)
        carried = eng.carried()[0]
        full = eng.derivs()
        out = {k: {p: eng.derivs(active=idx, path=p) for p in ("narrow", "wide")}
               for k, idx in active_lists(n).items()}
    finally:
        eng.close()
    mu = G_SI * b.mass
    ref = oracle.acc_jerk_snap(b.pos, b.vel, carried, mu, G=1.0, with_potential=True,
                               with_abs=True)
    return b, full, out, ref


# ---- 1. the two evaluate paths --------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_both_paths_match_oracle(hip, n):
    _, _, out, (ra, rj, rs, rphi, sa, sj, ss) = _paths(n)
    for name, idx in active_lists(n).items():
        for path in ("narrow", "wide"):
            a4, j4, s4 = out[name][path]
            r = (worst(a4[:, :3], ra[idx], sa[idx]), worst(j4[:, :3], rj[idx], sj[idx]),
                 worst(s4[:, :3], rs[idx], ss[idx]),
                 worst(a4[:, 3], rphi[idx], np.abs(rphi[idx])))
            print(f"n={n} {path} {name} ({len(idx)}): acc {r[0]:.1f} jerk {r[1]:.1f} snap "
                  f"{r[2]:.1f} phi {r[3]:.1f} (x eps x scale)")
            assert a4.shape == (len(idx), 4) and max(r) <= 128.0, (name, path, r)
            assert not j4[:, 3].any() and not s4[:, 3].any()


@pytest.mark.parametrize("n", SIZES)
def test_wide_path_bits_are_the_shared_step_kernels(hip, n):
    """gs_hermite_derivs6's second pass reads (x, v, a of its first pass), and a fresh engine
    carries that a: the same rows, so the same bits."""
    _, (fa, fj, fs), out, _ = _paths(n)
    for name, idx in active_lists(n).items():
        a4, j4, s4 = out[name]["wide"]
        assert np.array_equal(a4, fa[idx]) and np.array_equal(j4, fj[idx]), name
        assert np.array_equal(s4, fs[idx]), name


@pytest.mark.parametrize("n", SIZES)
def test_narrow_bits_depend_on_the_body_alone(hip, n):
    """Alone, in a full group, at the other slot of a group, among all, and for every narrow_max
    that admits the list: the same bits."""
    eng = _engine(n, dt=3600.0)
    try:
        eng.load(ic.solar_random(n, seed=7 + n))
        eng.set_block_tuning(narrow_max=n)
        every = np.arange(n, dtype=np.int32)
        ref = eng.derivs(active=every, path="narrow")
        for i in sorted({0, 1, n // 2, n - 1}):
            alone = eng.derivs(active=[i], path="narrow")
            assert all(np.array_equal(g[0], r[i]) for g, r in zip(alone, ref)), i
            other = (i + 1) % n
            for pair in ([i, other], [other, i]):  # slot 0 and slot 1 of a full group
                got = eng.derivs(active=pair, path="narrow")
                assert all(np.array_equal(g, r[pair]) for g, r in zip(got, ref)), pair
        rev = every[::-1].copy()
        assert all(np.array_equal(g, r[rev]) for g, r in
                   zip(eng.derivs(active=rev, path="narrow"), ref))
        some = active_lists(n)["five"]
        for cap in sorted({len(some), len(some) + 1, min(n, 64)}):
            eng.set_block_tuning(narrow_max=cap)
            got = eng.derivs(active=some)  # (by narrow_max: narrow)
            assert all(np.array_equal(g, r[some]) for g, r in zip(got, ref)), cap
        if n > 5:
            eng.set_block_tuning(narrow_max=4)
            with pytest.raises(RuntimeError, match="narrow_max"):
                eng.derivs(active=some, path="narrow")
            wide = eng.derivs(active=some)  # 5 > narrow_max: wide
            assert np.array_equal(wide[2], eng.derivs()[2][some])
    finally:
        eng.close()


@pytest.mark.parametrize("path", ["narrow", "wide"])
def test_coincident_self_and_ghost_pairs_contribute_exactly_zero(hip, path):
    """Body 0 sits on body 1 and on the origin, where the ghost rows are. Its derivatives are
    those with body 1 massless and elsewhere, bit for bit: the pair with body 1, its own and
    those with the ghost rows add exactly nothing to a, j, s and phi. The acceleration rows are
    supplied (zero for bodies 0 and 1 in both runs), so both runs read the same rows."""
    pos = np.array([[0, 0, 0], [0, 0, 0], [-1e11, 2e10, 0], [3e10, -1e11, 5e9]], dtype=float)
    vel = np.array([[0, 1e4, 0], [0, -2e4, 3e3], [1e3, 0, 0], [0, 2e3, -1e3]], dtype=float)
    mass = np.array([1e25, 2e25, 3e25, 4e25])
    acc = np.array([[0, 0, 0], [0, 0, 0], [1e-3, -2e-3, 5e-4], [-4e-4, 1e-3, 2e-3]])
    zero = np.zeros((4, 3))
    apart = pos.copy()
    apart[1] = [5e10, 5e10, 5e10]
    got = []
    for p, m in ((pos, mass), (apart, mass * np.array([1, 0, 1, 1]))):
        eng = _engine(4, dt=3600.0)
        try:
            eng.load(BodySet(p, vel, m), acc=acc, jerk=zero, snap=zero, crackle=zero)
            got.append(eng.derivs(active=[0, 2], path=path))
        finally:
            eng.close()
    (a, j, s), (a_ref, j_ref, s_ref) = got
    assert all(np.isfinite(y).all() for y in (a, j, s))
    assert np.array_equal(a[0], a_ref[0]) and np.array_equal(j[0], j_ref[0])
    assert np.array_equal(s[0], s_ref[0])
    ra, rj, rs, rphi, sa, sj, ss = oracle.acc_jerk_snap(pos, vel, acc, G_SI * mass, G=1.0,
                                                         with_potential=True, with_abs=True)
    idx = [0, 2]
    assert worst(a[:, :3], ra[idx], sa[idx]) <= 128.0 and worst(j[:, :3], rj[idx], sj[idx]) <= 128.0
    assert worst(s[:, :3], rs[idx], ss[idx]) <= 128.0
    assert worst(a[:, 3], rphi[idx], np.abs(rphi[idx])) <= 128.0


# ---- 2. runs --------------------------------------------------------------------------------
def test_level_0_is_the_shared_fixed_step_bit_for_bit(hip):
    """max_level = 0 and the wide path: a block step is a shared step of dt, and x, v, a, j, s, c
    are those of the shared fixed-step run."""
    n, K = 300, 5
    b = ic.solar_random(n, 12)
    out = []
    for block in (True, False):
        eng = _engine(n, dt=3600.0, block=block, max_level=0, eta=ETA if block else 0.0)
        try:
            eng.load(b)
            if block:
                eng.set_block_tuning(narrow_max=0)
            eng.step(K)
            st, s = eng.status(), eng.state()
            out.append((s.pos, s.vel) + eng.carried())
            assert st.time == K * 3600.0 and st.steps == K
            if block:
                assert (st.level_max, st.block_steps, st.body_steps) == (0, K, K * n)
                assert not eng.levels().any() and (eng.body_times() == K).all()
        finally:
            eng.close()
    assert len(out[0]) == 6
    for x, y in zip(*out):
        assert np.array_equal(x, y)


def _block_run(n, narrow_max=None, order=6, toggle=False):
    eng = _engine(n, dt=DT, softening=SOFT, t_end=32 * DAY, hermite_order=order,
                  eta=ETA if order == 6 else 0.02)
    try:
        if toggle:  # an order-4 block engine: order 6 with its block steps on, and off again
            lib, h = eng.lib, eng._h
            assert lib.gs_hermite_set_order(h, 6) != 0  # (not while order 4's block mode is on)
            assert lib.gs_hermite_set_block(h, 0, 0) == 0 and lib.gs_hermite_set_order(h, 6) == 0
            assert lib.gs_hermite_set_block6(h, 1, 24) == 0
            assert lib.gs_hermite_set_order(h, 4) != 0 and b"off first" in lib.gs_last_error()
            assert lib.gs_hermite_set_block6(h, 0, 0) == 0 and lib.gs_hermite_set_order(h, 4) == 0
            assert lib.gs_hermite_set_block(h, 1, 24) == 0
        eng.load(cpu6.bodies(n))
        if narrow_max is not None:
            eng.set_block_tuning(narrow_max=narrow_max)
        eng.step(6)  # (the steps past t_end are no-ops)
        return eng.state(), eng.status(), eng.levels(), eng.body_times(), eng.carried()
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _cpu_run(n):
    eng = HermiteCpuEngine(cpu6.cfg_for(n).validate())
    eng.load(cpu6.bodies(n))
    eng.step(4)
    return eng.state().pos, eng.levels(), list(eng.block_log)


@pytest.mark.parametrize("n", [64, 200])
@pytest.mark.parametrize("narrow_max", [None, "n", 0, 16])
def test_fp64_run_matches_oracle_and_cpu_engine(hip, n, narrow_max):
    """Default narrow_max, always narrow, always wide, and a mix of both."""
    x, v, lev, log, clamped, stats = cpu6.oracle_run(n)
    cx, clev, clog = _cpu_run(n)
    s, st, glev, tb, _ = _block_run(n, n if narrow_max == "n" else narrow_max)
    err = np.abs(s.pos - x).max() / np.abs(x).max()
    err_cpu = np.abs(s.pos - cx).max() / np.abs(x).max()
    print(f"n={n} narrow_max={narrow_max}: {st.block_steps} block steps, position error "
          f"{err:.2e} (oracle) {err_cpu:.2e} (CPU engine) of max |x|")
    assert (st.block_steps, st.body_steps) == cpu6.STEPS[n] == (len(log), sum(m for _, m in log))
    assert clog == log
    assert np.array_equal(glev, lev) and np.array_equal(glev, clev) and (tb == 4 << 24).all()
    assert err <= 1e-10 and err_cpu <= 1e-10
    assert st.time == 32 * DAY and st.finished and st.steps == 4
    assert st.level_clamped == clamped == 0 and st.level_max == stats["level_max"]


def test_same_run_twice_gives_the_same_bits(hip):
    a, b = _block_run(200, 16), _block_run(200, 16)
    assert np.array_equal(a[0].pos, b[0].pos) and np.array_equal(a[0].vel, b[0].vel)
    assert a[1] == b[1] and np.array_equal(a[2], b[2])
    assert all(np.array_equal(p, q) for p, q in zip(a[4], b[4])) and len(a[4]) == 4


def test_order_6_on_and_off_leaves_an_order_4_block_run(hip):
    a, b = _block_run(200, order=4), _block_run(200, order=4, toggle=True)
    assert np.array_equal(a[0].pos, b[0].pos) and np.array_equal(a[0].vel, b[0].vel)
    assert a[1] == b[1] and np.array_equal(a[2], b[2]) and a[1].block_steps > 4
    assert all(np.array_equal(p, q) for p, q in zip(a[4], b[4])) and len(a[4]) == 2


def test_gpu_resume_is_bit_exact(hip, tmp_path):
    cfg = SimConfig(n=200, steps=2, dt=DT, dtype="fp64", device="gpu", integrator="hermite",
                    hermite_order=6, eta=ETA, softening=SOFT, block_steps6=True, init="plummer",
                    seed=4)
    sim = Simulation(cfg)
    m = sim.run()
    assert m.steps == 2 and m.block_steps > 2 and m.pair_evals == m.body_steps * 200
    assert m.hermite_order == 6
    path = str(tmp_path / "c.gsck")
    sim.save_checkpoint(path)
    sim.run(2)
    ref, ref_lev, ref_st, ref_c = sim.global_state(), sim.engine.levels(), sim.engine.status(), \
        sim.engine.carried()
    sim.close()
    sim2 = Simulation(cfg.replace(resume=path))
    sim2.run(2)
    got, lev, st, step2, c2 = sim2.global_state(), sim2.engine.levels(), sim2.engine.status(), \
        sim2.step, sim2.engine.carried()
    sim2.close()
    assert np.array_equal(got.pos, ref.pos) and np.array_equal(got.vel, ref.vel)
    assert all(np.array_equal(p, q) for p, q in zip(c2, ref_c))
    assert np.array_equal(lev, ref_lev) and st.time == ref_st.time == 4 * DT and step2 == 4


def test_native_refusals(hip):
    """gs_hermite_set_block6 is order 6's and refuses fp32 by name; gs_hermite_set_block stays
    order 4's."""
    def raw(dtype):
        return HermiteHipEngine(SimConfig(n=64, dtype=dtype, device="gpu", integrator="hermite",
                                          eta=ETA, dt=DT).validate())
    eng = raw("fp32")
    try:
        assert eng.lib.gs_hermite_set_block6(eng._h, 1, 24) != 0
        assert b"order is not 6" in eng.lib.gs_last_error()
        assert eng.lib.gs_hermite_set_order(eng._h, 6) == 0
        assert eng.lib.gs_hermite_set_block6(eng._h, 1, 24) != 0
        assert b"fp64 only" in eng.lib.gs_last_error()
    finally:
        eng.close()
    eng = raw("fp64")
    try:
        assert eng.lib.gs_hermite_set_order(eng._h, 6) == 0
        assert eng.lib.gs_hermite_set_block(eng._h, 1, 24) != 0
        assert b"gs_hermite_set_block6" in eng.lib.gs_last_error()
        assert eng.lib.gs_hermite_set_block6(eng._h, 1, 24) == 0
        assert eng.lib.gs_hermite_set_collisions(eng._h, 1) != 0
        assert b"collisions" in eng.lib.gs_last_error()
    finally:
        eng.close()


# ---- 3. the chain over many workgroups -------------------------------------------------------
N3, L3, DT3 = 20000, 3, 8.0


def _schedule_state():
    """Levels 0..3 and body times inside the first macro step, each a multiple of the body's own
    step, no body at tick 0: the level-3 bodies sit at the edges of workgroups 0, 1, 77 and 78
    (the last), the others are spread over all 79."""
    i = np.arange(N3)
    lev = np.ones(N3, dtype=np.int32)
    lev[i % 7 == 3] = 2
    lev[i % 1000 == 1] = 0
    lev[[0, 63, 64, 255, 256, 19711, 19712, 19967, 19968, N3 - 1]] = 3
    stp = np.int64(1) << (L3 - lev).astype(np.int64)
    m = np.zeros(N3, dtype=np.int64)
    for k in range(L3 + 1):
        at = np.nonzero(lev == k)[0]
        m[at] = np.arange(len(at)) % (1 << k)
    tb = np.where(lev == 0, 0, np.maximum(m, 1)) * stp
    return lev, tb


def _integer_schedule(lev, tb, end):
    """The (t_next, n_active) log of the block scheme while no level changes: what
    oracle.simulate_hermite6_block does on massless bodies (tests/test_hermite6_block_cpu.py
    test_oracle_schedule_from_a_given_block_state asserts that on the oracle itself)."""
    t, stp = tb.astype(np.int64).copy(), np.int64(1) << (L3 - lev).astype(np.int64)
    log = []
    while t.min() < end:
        nxt = int((t + stp).min())
        due = t + stp == nxt
        t[due] = nxt
        log.append((nxt, int(due.sum())))
    return log


@pytest.mark.parametrize("narrow_max", [None, 0, 16])
def test_schedule_over_many_workgroups(hip, narrow_max):
    """20,000 massless bodies at 1 m/s with a supplied block state: a = j = s = c = 0, the
    criterion is invalid, levels never change, and the run is the integer schedule: 7 block steps
    with active lists from 4 bodies to all 20,000 in 79 workgroups, exact counters and exact
    positions."""
    lev, tb = _schedule_state()
    log = _integer_schedule(lev, tb, 8)
    assert min(m for _, m in log) <= 16 and max(m for _, m in log) == N3 and len(log) == 7
    pos, vel = np.zeros((N3, 3)), np.zeros((N3, 3))
    pos[:, 0], vel[:, 0] = np.arange(N3), 1.0
    eng = _engine(N3, dt=DT3, max_level=L3)
    try:
        eng.load(BodySet(pos, vel, np.zeros(N3)), levels=lev, body_times=tb)
        if narrow_max is not None:
            eng.set_block_tuning(narrow_max=narrow_max)
        cut = eng.status_narrow_max()
        if narrow_max is None:  # both evaluate paths are taken
            assert any(m <= cut for _, m in log) and any(m > cut for _, m in log)
        assert np.array_equal(eng.body_times(), tb) and eng.status().time == DT3 * tb.min() / 8
        eng.step(1)
        s, st, glev, gtb = eng.state(), eng.status(), eng.levels(), eng.body_times()
    finally:
        eng.close()
    want = pos.copy()
    want[:, 0] += 8 - tb
    assert np.array_equal(s.pos, want) and np.array_equal(s.vel, vel)
    assert np.array_equal(glev, lev) and (gtb == 8).all()
    assert (st.block_steps, st.body_steps) == (len(log), sum(m for _, m in log))
    assert st.level_clamped == 0 and st.level_max == 3 and st.time == 8.0 and st.steps == 1
