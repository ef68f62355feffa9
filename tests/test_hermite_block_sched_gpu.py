"""The scheduling chain of the Hermite block steps on the GPU (block_next / ctrl / predict /
compact / correct / init of csrc/hip/nbody_hermite.hip, and the shared step's hermite_ctrl /
hermite_reduce minima) with real bodies in many workgroups, up to 514 of them, against the NumPy
oracle.

The reference is affordable because the bodies are test particles (ic.tracer_particles): a Sun,
7 bodies of 1e24..1e27 kg at the edges of workgroups 0, 1, 255, 256 and at the last index, and
massless particles everywhere else. A pair with mu_j = 0 adds exactly zero to a, j and phi, in
the kernels and in the oracle, so the oracle sums over the massive columns only
(oracle.simulate_hermite_block(sources=...)): O(n_active x 8) per block step.

Seven particles are moons of the last body, at the indices that put sparse active sets where the
chain's index arithmetic can go wrong (moons()): three that want a step below dt 2^-8 and are
clamped at level 8 on every one of their steps, in workgroups >= 256 only (at n = 700: in the
first and the last of the three), and four at level 7 on both sides of index 65,536 (at
n = 700: two, in the first two workgroups). dt = 16 d, eta = 0.02, max_level = 8, one macro
step. What the oracle does on the three inputs (seed 5), asserted below:

    n        block steps  body-steps  level_clamped  levels populated   lean     response to a relative
                                                                                 position perturbation of
                                                                                 1e-15        1e-13
    700      256          3,282       768            0,1,2,3,7,8        5.8e-05  6.7e-14      5.8e-12
    66,000   256          224,101     768            0..5,7,8           4.0e-08  9.6e-15      4.7e-13
    131,400  256          445,481     768            0..3,7,8           3.8e-07  1.4e-14      5.7e-13

"lean" is the closest any level decision came to a threshold, min |log2(dt / dt_want) - nearest
integer|: fp64 kernel noise is about 1e-14, so no decision can legitimately go the other way and
levels, counters and the (t, n_active) log must be the oracle's exactly. The (t, n_active) log,
the levels and the clamp count are the same under both perturbations. "response" is
max |x' - x| / max |x| between the perturbed and the unperturbed oracle run: the growth of a
perturbation over the run is 58 at most (the clamped moons, 100 radians of their orbit). The gate
is the block-run gate of tests/test_hermite_block_gpu.py, 1e-10 relative, whose basis is (block
steps) x (128 eps per evaluation) x (perturbation growth); with a growth above 1 it is kept only
while the response to 1e-13 is at most 1e-10 / 4, which _family() asserts on every input.

Active sets at 66,000 and 131,400 bodies: 127 block steps touch only the three deep moons
(workgroups 256, 257 and the last: all >= 256, three workgroups, every other one empty), 129 mix
bodies below and above index 65,536; 248 block steps have at most 2,048 active bodies and 8 have
6,506 to all, so both evaluate paths run under the default narrow_max (2,048 and 4,096).

Measured on one MI355X: position error against the oracle 8e-18 (700), 3.1e-15 to 4.4e-15
(66,000) and 3.7e-15 (131,400) for every narrow_max; level_clamped 768 everywhere; the shared
step's first dt within 2.2e-16 and the next within 8.5e-12 of the oracle's; max_level = 2 on the
Plummer sphere: 1,129 clamped steps on both sides. Wall time of a test, load and read-back
included: the first of each size, which also runs the oracle three times (cached afterwards),
0.25 s, 1.1 s and 2.0 s; then at 131,400 bodies 1.2 s (always wide) and 0.24 s (narrow_max 16),
at 66,000 0.41 s, 0.13 s and 0.15 s (always narrow); a shared-step case 0.12 s and 0.26 s; every
other test below 0.1 s; the 34 together 10 s.
"""
import functools

import numpy as np
import pytest

from gravsim.config import SimConfig
from gravsim.models import initial_conditions as ic
from gravsim.models.initial_conditions import MASSIVE_AT, BodySet
from gravsim.ops import oracle
from gravsim.runtime.hermite import HermiteHipEngine

pytestmark = pytest.mark.gpu

DAY = 86400.0
DT, ETA, LMAX, SEED = 16 * DAY, 0.02, 8, 5
WG = 256  # bodies per workgroup of the chain's kernels (gs_kernels.h kForceBlock)
SIZES = [700, 66000, 131400]


def _tau(e):
    """The dynamical time of a moon whose Aarseth step on a circular orbit, sqrt(eta) tau, is
    dt 2^-e."""
    return DT * 2.0 ** -e / np.sqrt(ETA)


def moons(n):
    """(host, particle, tau, speed) of the seven moons: `deep` want level 9 (e = 8.5: halfway
    between two thresholds) and are clamped at 8, `mid` sit at level 7 (e = 6.5)."""
    deep = [1, n - 3, n - 2] if n < 65536 + WG else [65538, 65800, n - 2]
    mid = [2, 301] if n < 65536 + WG else [1, 300, 65534, 65540]
    return tuple((-1, p, _tau(8.5), 1.0) for p in deep) + \
        tuple((-1, p, _tau(6.5), 1.0) for p in mid)


def family(n):
    return ic.tracer_particles(n, SEED, moons=moons(n))


def _engine(n, dtype="fp64", **kw):
    kw.setdefault("eta", ETA)
    kw.setdefault("block_steps", True)
    return HermiteHipEngine(SimConfig(n=n, dtype=dtype, device="gpu", integrator="hermite",
                                      **kw).validate())


@functools.lru_cache(maxsize=None)
def _oracle_run(n, rel=0.0):
    b, src = family(n)
    pos = b.pos
    if rel:
        pos = pos * (1.0 + rel * np.random.default_rng(1).uniform(-1, 1, pos.shape))
    stats = {}
    out = oracle.simulate_hermite_block(pos, b.vel, b.mass, DT, DT, ETA, max_level=LMAX,
                                        sources=src, stats=stats)
    return out + (stats,)


def _workgroups(act):
    return np.unique(act // WG)


@functools.lru_cache(maxsize=None)
def _family(n):
    """The oracle's run on input n, after asserting on it everything the test relies on (module
    docstring), so that no comparison below can pass vacuously."""
    x, v, lev, log, clamped, stats = _oracle_run(n)
    for rel in (1e-15, 1e-13):
        px, _, plev, plog, pclamped, _ = _oracle_run(n, rel)
        resp = np.abs(px - x).max() / np.abs(x).max()
        print(f"n={n}: response to a relative perturbation of {rel:g}: {resp:.2e}")
        assert plog == log and np.array_equal(plev, lev) and pclamped == clamped, rel
        if rel == 1e-13:
            assert resp <= 1e-10 / 4  # (the condition for the 1e-10 gate)
    act = stats["active"]
    nwg = -(-n // WG)
    print(f"n={n}: {len(log)} block steps, {sum(m for _, m in log)} body-steps, clamped "
          f"{clamped}, lean {stats['lean']:.2e}, levels {np.bincount(lev, minlength=LMAX + 1)}")
    assert stats["lean"] >= 1e-9
    assert len(np.unique(lev)) >= 4
    assert [len(a) for a in act] == [m for _, m in log]
    if n >= 66000:
        assert any(a.min() >= WG * WG for a in act)           # workgroups >= 256 alone
        assert any(a.min() < WG * WG <= a.max() for a in act)  # both sides of index 65,536
        assert any(3 <= len(_workgroups(a)) < nwg for a in act)
        assert clamped > 0
    else:
        # 3 workgroups in all: a sparse set in every one of them, and one that leaves the middle
        # one empty
        assert any(len(_workgroups(a)) == 3 and len(a) <= 16 for a in act)
        assert any(list(_workgroups(a)) == [0, 2] for a in act)
    return x, v, lev, log, clamped, stats


NARROW = {"default": None, "never": 0, "16": 16, "always": "n"}


@pytest.mark.parametrize("n,narrow", [(n, k) for n in SIZES for k in NARROW
                                      if not (k == "always" and n > 66000)])
def test_fp64_run_matches_sparse_oracle(hip, n, narrow):
    """One macro step of 256 block steps whose active sets lie in up to 514 workgroups. Gate and
    inputs: module docstring."""
    x, v, lev, log, clamped, stats = _family(n)
    b, src = family(n)
    narrow_max = n if NARROW[narrow] == "n" else NARROW[narrow]
    eng = _engine(n, dt=DT, max_level=LMAX, t_end=DT)
    try:
        eng.load(b)
        a0, j0 = oracle.acc_jerk(b.pos, b.vel, b.mass, sources=src)
        first = oracle.block_first_levels(a0, j0, DT, ETA, LMAX)
        assert np.array_equal(eng.levels(), first)           # block_init_kernel, every workgroup
        assert not eng.body_times().any() and eng.status().level_max == first.max()
        if narrow_max is not None:
            eng.set_block_tuning(narrow_max=narrow_max)
        cut = eng.status_narrow_max()
        if narrow_max is None:  # both evaluate paths are taken
            assert any(m <= cut for _, m in log) and any(m > cut for _, m in log)
        eng.step(2)  # (the step past t_end is a no-op)
        s, st, glev, tb = eng.state(), eng.status(), eng.levels(), eng.body_times()
    finally:
        eng.close()
    err = np.abs(s.pos - x).max() / np.abs(x).max()
    print(f"n={n} narrow_max={cut}: {st.block_steps} block steps, {st.body_steps} body-steps, "
          f"clamped {st.level_clamped}, position error {err:.2e}")
    assert st.block_steps == len(log) and st.body_steps == sum(m for _, m in log)
    assert np.array_equal(glev, lev)
    assert st.level_clamped == clamped
    assert st.level_max >= stats["level_max"] and st.level_max <= LMAX
    assert (tb == 1 << LMAX).all()
    assert st.time == DT and st.steps == 1 and st.finished
    assert err <= 1e-10


# ---- 2. the schedule alone: no forces, every number exact ------------------------------------
N2, L2, DT2 = 66000, 3, 8.0


def _schedule_levels():
    i = np.arange(N2)
    lev = np.zeros(N2, dtype=np.int32)
    lev[i % 7 == 3] = 1
    lev[i % 1000 == 1] = 2
    lev[[0, 63, 64, 255, 256, 65535, 65536, 65537, N2 - 1]] = 3
    return lev


def _massless():
    pos, vel = np.zeros((N2, 3)), np.zeros((N2, 3))
    pos[:, 0] = np.arange(N2)  # (below 2^24: exact in fp32 too, as is every sum below)
    vel[:, 0] = 1.0
    return BodySet(pos, vel, np.zeros(N2))


def _count_schedule(lev, tb, end):
    """(block steps, body-steps) of the integer schedule from body times tb to `end` ticks."""
    t, stp = tb.astype(np.int64).copy(), np.int64(1) << (L2 - lev).astype(np.int64)
    steps = body = 0
    while t.min() < end:
        due = t + stp == (t + stp).min()
        t[due] += stp[due]
        steps, body = steps + 1, body + int(due.sum())
    assert (t == end).all()
    return steps, body


SCHEDULE_CASES = [("fp64", None), ("fp64", 0), ("fp32", None), ("mixed", None)]


@pytest.mark.parametrize("dtype,narrow_max", SCHEDULE_CASES)
def test_schedule_of_loaded_levels_is_exact(hip, dtype, narrow_max):
    """All masses 0: a = j = 0, the criterion is invalid, levels never change, and the run is the
    integer schedule of the loaded levels: 16 block steps of 1 s ticks over two macro steps."""
    lev, b = _schedule_levels(), _massless()
    eng = _engine(N2, dtype, dt=DT2, max_level=L2)
    try:
        eng.load(b, levels=lev)
        if narrow_max is not None:
            eng.set_block_tuning(narrow_max=narrow_max)
        assert eng.status().time == 0.0 and np.array_equal(eng.levels(), lev)
        eng.step(2)
        s, st, glev, tb = eng.state(), eng.status(), eng.levels(), eng.body_times()
    finally:
        eng.close()
    assert np.array_equal(s.pos, b.pos + np.array([16.0, 0.0, 0.0]))
    assert np.array_equal(s.vel, b.vel)
    assert np.array_equal(glev, lev) and (tb == 2 << L2).all()
    assert st.block_steps == 16 == _count_schedule(lev, np.zeros(N2, np.int64), 16)[0]
    assert st.body_steps == 2 * int((1 << lev.astype(np.int64)).sum())
    assert st.body_steps == _count_schedule(lev, np.zeros(N2, np.int64), 16)[1]
    assert st.level_clamped == 0 and st.level_max == 3
    assert st.time == 16.0 and st.steps == 2


@pytest.mark.parametrize("floor", [0, 1])
@pytest.mark.parametrize("dtype,narrow_max", SCHEDULE_CASES)
def test_schedule_from_a_mid_macro_state_is_exact(hip, dtype, narrow_max, floor):
    """Body times that differ between the bodies, each a multiple of the body's own step inside
    the first macro step. floor = 1: no body at level 0, and none at tick 0, so the run's time,
    the earliest body time, is not 0 either."""
    lev, b = np.maximum(_schedule_levels(), floor), _massless()
    stp = np.int64(1) << (L2 - lev).astype(np.int64)
    m = np.zeros(N2, dtype=np.int64)  # which multiple of its step: all of them, level by level
    for k in range(L2 + 1):
        at = np.nonzero(lev == k)[0]
        m[at] = np.arange(len(at)) % (1 << k)
    if floor:
        m = np.maximum(m, 1)
    tb = m * stp
    assert (tb < 8).all() and len(np.unique(tb)) >= 7 and (tb.min() > 0) == bool(floor)
    steps, body = _count_schedule(lev, tb, 8)
    assert body == int(((8 - tb) // stp).sum())
    eng = _engine(N2, dtype, dt=DT2, max_level=L2)
    try:
        eng.load(b, levels=lev, body_times=tb)
        if narrow_max is not None:
            eng.set_block_tuning(narrow_max=narrow_max)
        assert eng.status().time == DT2 * tb.min() / 8
        assert np.array_equal(eng.body_times(), tb)
        eng.step(1)
        s, st, glev, gtb = eng.state(), eng.status(), eng.levels(), eng.body_times()
    finally:
        eng.close()
    want = b.pos.copy()
    want[:, 0] += 8 - tb
    assert np.array_equal(s.pos, want) and np.array_equal(s.vel, b.vel)
    assert np.array_equal(glev, lev) and (gtb == 8).all()
    assert (st.block_steps, st.body_steps) == (steps, body)
    assert st.level_clamped == 0 and st.level_max == 3 and st.time == 8.0


# ---- 3. the shared adaptive step beyond 256 workgroups ---------------------------------------
def _tight(n, where):
    """(host, particle) of the tightest pair: the minimum of dt_i comes from workgroup 0, 255,
    256, 257 or the last."""
    return {"wg0": (3, 1), "wg255": (65533, 65534), "wg256": (65539, 65538),
            "wg257": (65801, 65800), "last": (n - 3, n - 2)}[where]


def _shared_reference(n, where):
    """(bodies, first step, next step) of the oracle's shared adaptive step, after asserting that
    the tight particle sets both minima with a factor 2 to spare."""
    host, part = _tight(n, where)
    b, src = ic.tracer_particles(n, SEED, massive=MASSIVE_AT + (host,),
                                 moons=((host, part, 1e5, 0.5),))
    a0, j0 = oracle.acc_jerk(b.pos, b.vel, b.mass, sources=src)
    with np.errstate(divide="ignore", invalid="ignore"):
        each = 0.5 * ETA * np.sqrt((a0 * a0).sum(1)) / np.sqrt((j0 * j0).sum(1))
    first = oracle.hermite_first_dt(a0, j0, ETA)
    others = np.delete(each, part)
    assert first == each[part] < 0.5 * np.nanmin(others) and first < DT
    h = first
    xp = b.pos + (b.vel * h + (a0 * (h * h / 2) + j0 * (h * h * h / 6)))
    vp = b.vel + (a0 * h + j0 * (h * h / 2))
    a1, j1 = oracle.acc_jerk(xp, vp, b.mass, sources=src)
    nxt = oracle.hermite_dt(a0, j0, a1, j1, h, ETA)
    want, valid = oracle.hermite_dt_bodies(a0, j0, a1, j1, np.full(n, h), ETA)
    assert valid[part] and abs(nxt / want[part] - 1.0) < 1e-12 and nxt < DT
    assert nxt < 0.5 * np.delete(np.where(valid, want, np.inf), part).min()
    return b, first, nxt


@pytest.mark.parametrize("n", [66000, 131400])
@pytest.mark.parametrize("where", ["wg0", "wg255", "wg256", "wg257", "last"])
def test_shared_step_minimum_from_any_workgroup(hip, n, where):
    """One particle at half the circular speed 1e5 s (dynamical time) from one more massive
    body: its dt_i is below half of every other body's, before and after the first step, so
    hermite_ctrl_kernel's h and the next step are its, whichever workgroup holds it. The 1e-9
    gate is that of tests/test_hermite_gpu.py test_dt_next_after_one_adaptive_step."""
    b, first, nxt = _shared_reference(n, where)
    eng = _engine(n, dt=DT, block_steps=False)
    try:
        eng.load(b)
        st0 = eng.status()
        eng.step(1)
        st = eng.status()
    finally:
        eng.close()
    print(f"n={n} {where}: first dt {first:.6g} s (device {st0.dt_next / first - 1:+.1e}), next "
          f"{nxt:.6g} s (device {st.dt_next / nxt - 1:+.1e})")
    assert abs(st0.dt_next / first - 1.0) < 1e-9
    assert abs(st.dt_last / first - 1.0) < 1e-9 and st.steps == 1 and st.time == st.dt_last
    assert abs(st.dt_next / nxt - 1.0) < 1e-9


# ---- 4. the level cap on the device ----------------------------------------------------------
def test_level_cap_is_counted_on_the_device(hip):
    """tests/test_hermite_block_cpu.py test_level_cap_is_reported on the GPU: the Plummer sphere
    of tests/test_hermite_block_gpu.py (200 bodies, seed 9, 32 d of dt = 8 d, softening 1e9 m)
    with max_level = 2, against the dense oracle; gate 1e-10 as there."""
    n, dt, soft = 200, 8 * DAY, 1e9
    b = ic.plummer(n, seed=9)
    stats = {}
    x, v, lev, log, clamped = oracle.simulate_hermite_block(
        b.pos, b.vel, b.mass, dt, 4 * dt, ETA, max_level=2, softening=soft, stats=stats)
    assert clamped > 0 and stats["lean"] >= 1e-9
    eng = _engine(n, dt=dt, max_level=2, softening=soft, t_end=4 * dt)
    try:
        eng.load(b)
        eng.step(4)
        s, st, glev = eng.state(), eng.status(), eng.levels()
    finally:
        eng.close()
    print(f"max_level 2: {st.block_steps} block steps, clamped {st.level_clamped} (oracle "
          f"{clamped})")
    assert st.level_clamped == clamped and st.level_max == 2
    assert st.block_steps == len(log) and st.body_steps == sum(m for _, m in log)
    assert np.array_equal(glev, lev)
    assert np.abs(s.pos - x).max() / np.abs(x).max() <= 1e-10
