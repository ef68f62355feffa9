"""Nearest neighbours, closest approaches and overlaps from the Hermite acceleration+jerk kernels
on the GPU (the NN flag of csrc/hip/nbody_hermite.hip, gs_hermite_set_collisions and friends).

Pair measure q_ij = r^2 - (R_i + R_j)^2 on the kernel's own r^2; nearest neighbour = smallest q,
lowest j on an exact tie, (+inf, -1) when there is none (docs/DESIGN.md §17).

Reference: oracle.nearest_neighbours (fp64 NumPy) on the inputs as the pair kernel sees them:
positions and radii rounded to fp32 (fp32), positions as hi + lo and radii rounded to fp32
(mixed), as they are (fp64). Bound of a pair: B = 8 u (r^2 + s^2), u = 2^-24 (fp32, mixed) or
2^-53 (fp64), s = R_i + R_j: three rounded differences, three fmas, one add and one fma form q.
  * the returned q is within B of the oracle's q of the returned pair;
  * that oracle value is within 2 B of the oracle's minimum;
  * where the oracle's best and second-best q differ by more than 2 B the index is the oracle's;
    at most 1 % of the bodies may be excused by a smaller gap.
Excused share of the oracle alone on these inputs (measured on the CPU, tests/
test_hermite_nn_cpu.py test_excused_share_of_the_inputs): 0 of every size and dtype, solar+random
and Plummer.
"""
import functools
import json
import os

import numpy as np
import pytest

from gravsim.cli import main
from gravsim.config import G_SI, SimConfig
from gravsim.models import initial_conditions as ic
from gravsim.models.initial_conditions import BodySet
from gravsim.ops import oracle
from gravsim.runtime.hermite import HermiteCpuEngine, HermiteHipEngine
from gravsim.runtime.simulation import Simulation
from gravsim.utils import checkpoint as ck
from hermite_nn_helpers import (DTYPES, SIZES, SOFT, U, chain_and_bystander, check_against_oracle,
                                head_on, lattice, merger_with_bystander, run_driver, with_radii)

pytestmark = pytest.mark.gpu

def _cfg(n, dtype, **kw):
    kw.setdefault("integrator", "hermite")
    kw.setdefault("collisions", "detect")
    return SimConfig(n=n, dtype=dtype, device="gpu", **kw).validate()


def _engine(n, dtype, **kw):
    return HermiteHipEngine(_cfg(n, dtype, **kw))


def _block_engine(n, dtype, **kw):
    kw.setdefault("dt", 3600.0)
    kw.setdefault("max_level", 6)
    eng = _engine(n, dtype, block_steps=True, eta=0.02, **kw)
    eng.set_block_tuning(n)  # (any active set may take the narrow path)
    return eng


def _nn(b, dtype, **kw):
    eng = _engine(b.n, dtype, **kw)
    try:
        eng.load(b)
        return eng.derivs_nn()
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _bodies(family, n):
    b = ic.solar_random(n, 7 + n) if family == "solar" else ic.make("plummer", n, 7 + n, G_SI)
    return with_radii(b, 100 + n)


# ---- 1. against the oracle -----------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_nn_matches_oracle(hip, n, dtype):
    """Workgroup (256), tile and chunk (2048) edges; 4097 has three chunks plus pad rows."""
    b = _bodies("solar", n)
    _, _, q, nn = _nn(b, dtype)
    ex = check_against_oracle(q, nn, b, dtype)
    print(f"n={n} {dtype}: excused {ex:.4f}")
    if n == 1:
        assert np.isinf(q[0]) and q[0] > 0 and nn[0] == -1


@pytest.mark.parametrize("dtype", DTYPES)
def test_nn_matches_oracle_plummer_softened(hip, dtype):
    b = _bodies("plummer", 2049)
    for kw in (dict(), dict(softening=SOFT), dict(softening=SOFT, cutoff=0.0)):
        _, _, q, nn = _nn(b, dtype, **kw)
        check_against_oracle(q, nn, b, dtype, kw.get("softening", 0.0), kw.get("cutoff", 1e-10))


@pytest.mark.parametrize("dtype", DTYPES)
def test_block_paths_match_oracle(hip, dtype):
    """The narrow and the wide evaluate of a block step, on an active set that is no prefix."""
    n = 4097
    b = _bodies("solar", n)
    idx = np.random.default_rng(5).permutation(n)[:301].astype(np.int32)
    eng = _block_engine(n, dtype)
    try:
        eng.load(b)
        for path in ("narrow", "wide"):
            _, _, q, nn = eng.derivs_nn(idx, path)
            check_against_oracle(q, nn, b, dtype, rows=idx)
    finally:
        eng.close()


# ---- 2. planted cases ------------------------------------------------------------------------
def _far_pair(b, i, j, sep=1e5):
    """Move bodies i and j to a corner of their own, sep apart."""
    b.pos[i] = (9e11, 9e11, 9e11)
    b.pos[j] = b.pos[i] + (sep, 0.0, 0.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nearest_in_another_chunk_and_in_the_last_row(hip, dtype):
    n = 4097
    b = _bodies("solar", n).copy()
    b.radius[[5, 4000, 9, n - 1]] = 0.0
    _far_pair(b, 5, 4000)
    b.pos[9] = (-9e11, 9e11, -9e11)
    b.pos[n - 1] = b.pos[9] + (0.0, 2e5, 0.0)
    _, _, q, nn = _nn(b, dtype)
    assert nn[5] == 4000 and nn[4000] == 5 and nn[9] == n - 1 and nn[n - 1] == 9
    check_against_oracle(q, nn, b, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_large_body_is_nearest_by_q_not_by_distance(hip, dtype):
    """A Sun-sized body 8e8 m away (q = 1.5e17) against a point 5e8 m away (q = 2.5e17)."""
    pos = np.array([[0, 0, 0], [5e8, 0, 0], [0, 8e8, 0], [3e11, 1e11, 0]], dtype=float)
    b = BodySet(pos, np.zeros((4, 3)), np.array([1e24, 1e23, 2e30, 1e24]),
                np.array([0.0, 0.0, 7e8, 0.0]))
    _, _, q, nn = _nn(b, dtype)
    assert nn[0] == 2 and q[0] > 0
    assert oracle.nearest_neighbours(pos, None)[1][0] == 1  # (by distance it is body 1)
    check_against_oracle(q, nn, b, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_sun_at_the_origin_never_sees_a_pad_row(hip, dtype):
    """With softening the ghost rows (at the origin) are not below the cutoff: r^2 = eps^2, the
    smallest q there is for a body at the origin. Shared kernel and both block paths."""
    for n in (3, 257):
        b = ic.solar_random(n, 11)
        b = BodySet(b.pos, b.vel, b.mass, np.zeros(n))
        assert not b.pos[0].any()
        eng = _block_engine(n, dtype, softening=SOFT, cutoff=0.0)
        try:
            eng.load(b)
            assert eng.layout.n_pad > n
            got = [eng.derivs_nn()[2:], eng.derivs_nn(np.arange(n), "narrow")[2:],
                   eng.derivs_nn(np.arange(n), "wide")[2:]]
        finally:
            eng.close()
        for q, nn in got:
            assert (nn >= 0).all() and (nn < n).all()
            check_against_oracle(q, nn, b, dtype, SOFT, 0.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_single_body_and_pair_below_the_cutoff(hip, dtype):
    one = BodySet(np.array([[1e11, 2e10, 0.0]]), np.zeros((1, 3)), np.array([1e24]),
                  np.array([1e7]))
    _, _, q, nn = _nn(one, dtype)
    assert q[0] == np.inf and nn[0] == -1
    pos = np.array([[1e11, 0, 0], [1e11, 0, 0], [-1e11, 2e10, 0]], dtype=float)
    b = BodySet(pos, np.zeros((3, 3)), np.array([1e25, 2e25, 3e25]), np.array([1e6, 1e6, 3e6]))
    _, _, q, nn = _nn(b, dtype)
    assert list(nn) == [2, 2, 0]  # (the coincident pair is skipped; 0 before 1 on the tie)
    check_against_oracle(q, nn, b, dtype, cap=1.0)  # (body 2's two candidates tie exactly)
    two = BodySet(pos[:2], np.zeros((2, 3)), b.mass[:2], b.radius[:2])
    _, _, q, nn = _nn(two, dtype)
    assert np.all(np.isinf(q)) and list(nn) == [-1, -1]


# ---- 3. exact ties and bit identity across shapes, paths, active sets and slots ------------------
def _every_shape(b, dtype):
    """(label, q, nn) of all bodies through every launch shape and both block paths, the block
    paths with active sets in different orders (so every body sits in different slots)."""
    n = b.n
    out = []
    probe = _engine(n, dtype)
    n_chunks = probe.native_layout["n_chunks"]
    probe.close()
    for ipl in (1, 2, 4) if dtype != "fp64" else (1, 2):
        for groups in range(1, n_chunks + 1):
            eng = _engine(n, dtype, ipl=ipl, split_groups=groups)
            try:
                # (mixed with collisions on has no 4-body tile: the layout reports the 2 it runs)
                assert eng.native_layout["ipl"] == (2 if dtype == "mixed" and ipl == 4 else ipl)
                eng.load(b)
                out.append(((ipl, groups), *eng.derivs_nn()[2:]))
            finally:
                eng.close()
    eng = _block_engine(n, dtype)
    try:
        eng.load(b)
        rng = np.random.default_rng(9)
        for path in ("narrow", "wide"):
            for order in (np.arange(n), np.arange(n)[::-1], rng.permutation(n)):
                idx = np.ascontiguousarray(order, dtype=np.int32)
                _, _, q, nn = eng.derivs_nn(idx, path)
                back = np.empty(n, dtype=np.int64)
                back[idx] = np.arange(n)
                out.append(((path, int(idx[0])), q[back], nn[back]))
            part = np.ascontiguousarray(rng.permutation(n)[:77], dtype=np.int32)
            _, _, q, nn = eng.derivs_nn(part, path)
            full = out[0]
            assert np.array_equal(q.view(np.int64), full[1][part].view(np.int64)), path
            assert np.array_equal(nn, full[2][part]), path
    finally:
        eng.close()
    return n_chunks, out


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_ties_go_to_the_lowest_index(hip, dtype):
    n = 2049
    b = lattice(n)
    oq, onn = oracle.nearest_neighbours(b.pos, b.radius)  # (exact in fp64 too; argmin: lowest j)
    d2 = ((b.pos[None, :, :] - b.pos[:64, None, :]) ** 2).sum(-1)
    d2[d2 == 0] = np.inf
    assert ((d2 == d2.min(1)[:, None]).sum(1) > 1).sum() > 32  # (most bodies have exact ties)
    n_chunks, shapes = _every_shape(b, dtype)
    assert n_chunks >= 2 and len(shapes) >= 2 * n_chunks + 6
    for label, q, nn in shapes:
        assert np.array_equal(nn, onn), label
        assert np.array_equal(q, oq), label


@pytest.mark.parametrize("dtype", DTYPES)
def test_bits_do_not_depend_on_shape_path_or_slot(hip, dtype):
    n = 2049
    b = _bodies("solar", n)
    _, shapes = _every_shape(b, dtype)
    _, q0, nn0 = shapes[0]
    for label, q, nn in shapes[1:]:
        assert np.array_equal(q.view(np.int64), q0.view(np.int64)), label
        assert np.array_equal(nn, nn0), label
    check_against_oracle(q0, nn0, b, dtype)


# ---- 4. the mode switch changes no other bit -----------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_mode_on_changes_no_bit_of_a_j_phi(hip, dtype):
    n = 2049
    b = _bodies("solar", n)
    idx = np.random.default_rng(2).permutation(n)[:500].astype(np.int32)
    got = {}
    for mode in ("off", "detect"):
        eng = _block_engine(n, dtype, collisions=mode)
        try:
            eng.load(b)
            got[mode] = [eng.derivs(), eng.derivs(idx, "narrow"), eng.derivs(idx, "wide")]
            eng.step(1)
            s = eng.state()
            got[mode].append((s.pos, s.vel))
            got[mode].append(eng.carried())
        finally:
            eng.close()
    for off, on in zip(got["off"], got["detect"]):
        assert np.array_equal(off[0], on[0]) and np.array_equal(off[1], on[1])
    for mode in ("off", "detect"):  # (and the shared step)
        eng = _engine(n, dtype, collisions=mode, dt=3600.0)
        try:
            eng.load(b)
            eng.step(3)
            s = eng.state()
            got[mode] = (s.pos, s.vel, *eng.carried())
        finally:
            eng.close()
    assert all(np.array_equal(x, y) for x, y in zip(got["off"], got["detect"]))


def test_collisions_off_refuses_the_queries(hip):
    eng = _engine(8, "fp64", collisions="off")
    try:
        eng.load(ic.solar_random(8, 1))
        with pytest.raises(ValueError):
            eng.neighbours()
        assert eng.status().overlaps == 0
    finally:
        eng.close()


def test_mixed_collisions_asked_for_four_per_lane_runs_two(hip):
    """Mixed precision with collisions on has no 4-bodies-per-lane evaluate kernel: the launch
    shape caps ipl at 2, and the gathered (wide) evaluate of a block step runs with it, to the
    bits of an engine that was asked for 2."""
    n = 2049
    b = _bodies("solar", n)
    idx = np.arange(0, n, 3, dtype=np.int32)
    got = {}
    for ipl in (4, 2):
        eng = _block_engine(n, "mixed", ipl=ipl)
        try:
            assert eng.native_layout["ipl"] == 2
            eng.load(b)
            got[ipl] = eng.derivs(active=idx, path="wide")
        finally:
            eng.close()
    a4, j4 = got[4]
    assert a4.shape == (len(idx), 4) and np.isfinite(a4).all() and np.isfinite(j4).all()
    assert np.any(a4[:, :3] != 0.0)
    assert np.array_equal(a4, got[2][0]) and np.array_equal(j4, got[2][1])


# ---- 5. closest-approach record and overlap stop -------------------------------------------------
@pytest.mark.parametrize("dtype,centre", [("fp64", (1.5e11, 0.7e11, -0.3e11)),
                                          ("mixed", (1.5e11, 0.7e11, -0.3e11)),
                                          ("fp32", (0.0, 0.0, 0.0))])
def test_shared_step_stops_at_the_oracles_step(hip, dtype, centre):
    b = head_on(centre)
    kw = dict(dt=1000.0, steps=200)
    rec = {}
    taken = oracle.simulate_hermite(b.pos, b.vel, b.mass, 1000.0, 200, radius=b.radius,
                                    collisions="merge", record=rec)[4]
    assert 50 < len(taken) < 120 and rec["overlaps"] == 2
    assert rec["ca_q"].max() < -1e13  # (the deciding q is far from 0: `drift` below is 8e10)
    cpu = HermiteCpuEngine(SimConfig(n=2, dtype=dtype, device="cpu", integrator="hermite",
                                     collisions="merge", **kw).validate())
    cpu.load(b)
    cpu.step(200)
    gpu = _engine(2, dtype, collisions="merge", **kw)
    try:
        gpu.load(b)
        for _ in range(4):
            gpu.step(50)  # (whatever the host's polling period)
        st = gpu.status()
        assert st.steps == cpu.status().steps == len(taken)
        assert st.overlaps == cpu.status().overlaps == 2
        assert st.time == cpu.status().time == sum(taken)
        cq, cn = gpu.closest()
        assert list(cn) == [1, 0] and list(cpu.closest()[1]) == [1, 0]
        # q of the engine against the oracle's: the bound of the pair, plus what the rounding of
        # the state on the way there moves it: per step a few roundings of |x| in the state's
        # precision (4 allowed, on both bodies), times dq / d sep = 2 sep
        B = 8.0 * U[dtype] * 2.0 * 4.1e7 ** 2
        ustate = 2.0 ** -24 if dtype == "fp32" else 2.0 ** -53
        drift = 2.0 * 4.1e7 * (2 * 4 * len(taken) * ustate * np.abs(b.pos).max())
        print(f"{dtype}: |dq| {np.abs(cq - rec['ca_q']).max():.3g} bound {B + drift:.3g}")
        assert np.abs(cq - rec["ca_q"]).max() <= B + drift
        lq, ln = gpu.neighbours()
        assert np.array_equal(lq, cq) and list(ln) == [1, 0]  # (closing: the latest is the closest)
        # detect records the same and never stops; clear_overlap lets the stopped run go on
        gpu.clear_overlap()
        assert gpu.status().overlaps == 0
        gpu.step(1)
        assert gpu.status().steps == len(taken) + 1 and gpu.status().overlaps == 2
    finally:
        gpu.close()
    det = _engine(2, dtype, collisions="detect", **kw)
    try:
        det.load(b)
        det.step(len(taken) + 5)
        assert det.status().steps == len(taken) + 5 and det.status().overlaps >= 2
    finally:
        det.close()


@pytest.mark.parametrize("dtype", ["fp64", "mixed"])
def test_block_run_records_the_overlap_inside_the_macro_step(hip, dtype):
    """Block steps never stop inside a macro step: the record carries what happened."""
    # (1e23 kg: the pull between the bodies is felt, Aarseth steps of a few 1000 s, yet they are
    # still 2e7 m apart at the end of the macro step, far from the point-mass singularity)
    b = head_on((1.5e11, 0.7e11, -0.3e11), mass=1e23)
    kw = dict(dt=88000.0, eta=0.02, max_level=10)  # (one macro step: touch at 7.95e4 s)
    rec = {}
    oracle.simulate_hermite_block(b.pos, b.vel, b.mass, kw["dt"], kw["dt"], kw["eta"],
                                  kw["max_level"], radius=b.radius, collisions="detect",
                                  record=rec)
    assert rec["overlaps"] >= 2 and (rec["ca_q"] < 0).all()
    eng = _engine(2, dtype, collisions="merge", block_steps=True, **kw)
    try:
        eng.load(b)
        assert eng.status().overlaps == 0
        eng.step(1)
        st = eng.status()
        assert st.steps == 1 and st.time == kw["dt"] and st.block_steps > 4
        cq, cn = eng.closest()
        assert list(cn) == [1, 0] and (cq < 0).all()
        assert st.overlaps >= 2
        if dtype == "fp64":
            assert st.overlaps == rec["overlaps"]
        lq, _ = eng.neighbours()
        assert (lq < 0).all()  # (still overlapping at the boundary)
        if dtype == "fp64":
            assert np.allclose(cq, rec["ca_q"], rtol=1e-6, atol=0)
    finally:
        eng.close()


# ---- 6. many workgroups ----------------------------------------------------------------------
def test_overlap_counter_and_record_beyond_workgroup_0(hip):
    """66,000 tracer particles in block steps, one overlapping pair across index 65,536 (two
    massless bodies 1 km apart with radii of 10 km, moving together): the evaluation the run
    starts with and every later correction of either body counts one overlap each, from
    workgroups 255 and 256, and their records name each other."""
    n, dt, eta, L = 66000, 16 * 86400.0, 0.02, 8
    b, massive = ic.tracer_particles(n, 5)
    i, j = 65530, 65541  # (workgroups 255 and 256, neither a massive body)
    assert b.mass[i] == 0 and b.mass[j] == 0
    b.pos[j] = b.pos[i] + (1e3, 0.0, 0.0)
    b.vel[j] = b.vel[i]
    rad = np.zeros(n)
    rad[[i, j]] = 1e4
    b = BodySet(b.pos, b.vel, b.mass, rad)
    stats = {}
    oracle.simulate_hermite_block(b.pos, b.vel, b.mass, dt, dt, eta, L, sources=massive,
                                  stats=stats)
    corrections = sum(int(np.isin([i, j], act).sum()) for act in stats["active"])
    rows = np.array([0, 255, 256, 300, i, 65536, j, n - 1])
    oq, onn = oracle.nearest_neighbours(b.pos, rad, rows=rows)
    eng = _engine(n, "fp64", collisions="detect", block_steps=True, dt=dt, eta=eta, max_level=L)
    try:
        eng.load(b)
        assert eng.status().overlaps == 2
        q, nn = eng.neighbours()
        assert np.array_equal(nn[rows], onn)
        assert np.allclose(q[rows], oq, rtol=1e-12, atol=0)
        assert nn[i] == j and nn[j] == i and q[i] < 0
        eng.step(1)
        st = eng.status()
        assert st.steps == 1 and st.overlaps == 2 + corrections
        cq, cn = eng.closest()
        assert cn[i] == j and cn[j] == i and cq[i] < 0 and cq[j] < 0
        assert ((cq < 0).sum()) == 2
    finally:
        eng.close()


# ---- 7. the driver on the GPU: merge runs, metrics, CLI, checkpoints -----------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("block", [False, True])
def test_three_body_chain_becomes_one_body(hip, block, dtype):
    b = chain_and_bystander()
    kw = dict(block_steps=True, eta=0.02, max_level=6) if block else {}
    s, ids, m, _ = run_driver(b, device="gpu", dtype=dtype, steps=3, collisions="merge", **kw)
    assert list(ids) == [0, 3] and m.mergers == 2 and m.bodies_left == 2 and m.steps_taken == 3
    assert m.overlaps_seen == 3 and m.closest_q_min < 0 and m.device == "gpu"
    rt = 1e-6 if dtype == "fp32" else 1e-15
    assert s.n == 2 and np.isclose(s.mass[0], 6e24, rtol=rt) and np.isclose(s.mass[1], 1e23, rtol=rt)
    assert np.isclose(s.radius[0], np.cbrt(3 * 2e7 ** 3), rtol=1e-15) and s.radius[1] == 1e6
    p0, p1 = (b.mass[:, None] * b.vel).sum(0), (s.mass[:, None] * s.vel).sum(0)
    assert np.abs(p1 - p0).max() <= 8 * rt * np.abs(b.mass[:, None] * b.vel).sum() + \
        1e-12 * np.abs(b.mass[:, None] * b.vel).sum()


@pytest.mark.parametrize("block", [False, True])
def test_detect_reports_and_changes_no_bit_of_a_run(hip, block):
    b = head_on((1.5e11, 0.7e11, -0.3e11), mass=1e23)
    kw = dict(dt=8000.0, block_steps=True, eta=0.02, max_level=6) if block else {}
    steps = 11 if block else 85
    off, _, m0, _ = run_driver(b, device="gpu", steps=steps, collisions="off", **kw)
    det, ids, m1, _ = run_driver(b, device="gpu", steps=steps, collisions="detect", **kw)
    assert np.array_equal(off.pos, det.pos) and np.array_equal(off.vel, det.vel)
    assert m1.mergers == 0 and m1.bodies_left == 2 and list(ids) == [0, 1]
    assert m1.overlaps_seen >= 2 and m1.closest_q_min < 0 and m1.steps_taken == steps
    assert m0.overlaps_seen is None


@pytest.mark.parametrize("dtype", ["fp64", "mixed"])
def test_resume_is_bit_exact_across_a_merger(hip, tmp_path, dtype):
    """Two bodies merge at step 71; checkpoints at 50 (before) and 100 (after)."""
    h = head_on((1.5e11, 0.7e11, -0.3e11))
    b = BodySet(np.vstack([h.pos, [[2e11, 0, 0]]]), np.vstack([h.vel, [[0, 2e4, 0]]]),
                np.append(h.mass, 1e22), np.append(h.radius, 1e6))
    kw = dict(collisions="merge", checkpoint_dir=str(tmp_path), dtype=dtype)
    full, ids, m, step = run_driver(b, device="gpu", steps=120, checkpoint_every=50, **kw)
    assert m.mergers == 1 and list(ids) == [0, 2] and step == 120 and m.steps_taken == 120
    for at, left in ((50, 3), (100, 2)):
        c = ck.load(ck.path_for(str(tmp_path), at))
        assert c.bodies.n == left
        got, gids, gm, gstep = run_driver(b, device="gpu", steps=120, resume=ck.path_for(str(tmp_path), at),
                                          run_steps=120 - at, **kw)
        assert gstep == 120 and list(gids) == [0, 2] and gm.mergers == 1
        assert np.array_equal(got.pos, full.pos) and np.array_equal(got.vel, full.vel)


def test_cli_merge_end_to_end(hip, tmp_path):
    out = tmp_path / "m.json"
    rc = main(["--n", "64", "--steps", "20", "--dt", "3600", "--device", "gpu", "--init", "cold",
               "--integrator", "hermite", "--collisions", "merge", "--body-density", "1e-3",
               "--quiet", "--log-format", "none", "--metrics-json", str(out)])
    d = json.loads(out.read_text().strip().splitlines()[-1])
    assert rc == 0 and d["device"] == "gpu"
    assert d["mergers"] >= 1 and d["bodies_left"] == 64 - d["mergers"]
    assert d["steps_taken"] == 20 and d["overlaps_seen"] >= d["mergers"] and d["closest_q_min"] < 0


@pytest.mark.parametrize("dtype", ["fp64", "mixed"])
def test_block_run_merges_at_the_macro_boundary(hip, tmp_path, dtype):
    """Block steps, macro step 44,000 s: the two bodies of 1e23 kg touch at about 7.9e4 s, inside
    the second macro step, and are merged at its boundary (88,000 s), not before and not later.
    The driver's figures carry across the engine restart, and a resume is bit-exact from the
    checkpoint before the merger (step 1) and from the one after it (step 2)."""
    b = merger_with_bystander(mass=1e23)
    kw = dict(device="gpu", dtype=dtype, dt=44000.0, block_steps=True, eta=0.02, max_level=10)
    first, ids1, m1, _ = run_driver(b, steps=1, collisions="merge", **kw)
    assert m1.mergers == 0 and list(ids1) == [0, 1, 2] and first.n == 3 and m1.overlaps_seen == 0
    two, ids2, m2, _ = run_driver(b, steps=2, collisions="merge", **kw)
    assert m2.mergers == 1 and list(ids2) == [0, 2] and m2.bodies_left == 2 and two.n == 2
    assert m2.steps_taken == 2 and m2.time_reached == 88000.0 and m2.overlaps_seen >= 2
    # the same two macro steps without the merger: what the merged body is made of
    det, _, md, _ = run_driver(b, steps=2, collisions="detect", **kw)
    assert det.n == 3 and np.array_equal(det.pos[2], two.pos[1]) and two.mass[1] == 1e22
    mt = det.mass[0] + det.mass[1]
    assert two.mass[0] == mt and two.radius[0] == np.cbrt(2 * 2.05e7 ** 3)
    com = (det.mass[:2, None] * det.pos[:2]).sum(0) / mt
    assert np.abs(two.pos[0] - com).max() <= 4 * np.finfo(float).eps * np.abs(com).max()
    p0, p1 = (det.mass[:, None] * det.vel).sum(0), (two.mass[:, None] * two.vel).sum(0)
    assert np.abs(p1 - p0).max() <= 8 * np.finfo(float).eps * np.abs(det.mass[:, None] * det.vel).sum()
    # up to the merger the engine did what the detect run did; pairs are counted against 3 bodies
    assert (m2.block_steps, m2.body_steps, m2.level_max, m2.level_clamped) == \
        (md.block_steps, md.body_steps, md.level_max, md.level_clamped)
    assert m2.block_steps > 2 and m2.pair_evals == 3 * m2.body_steps
    # four macro steps: the counters of the engine before and of the engine after add up
    ckdir = str(tmp_path)
    full, ids, m, step = run_driver(b, steps=4, collisions="merge", checkpoint_dir=ckdir,
                                    checkpoint_every=1, **kw)
    tail, _, mtail, _ = run_driver(two, steps=2, collisions="merge", **kw)
    assert m.mergers == 1 and list(ids) == [0, 2] and step == 4 and m.steps_taken == 4
    assert m.time_reached == 176000.0
    assert m.block_steps == m2.block_steps + mtail.block_steps
    assert m.body_steps == m2.body_steps + mtail.body_steps
    assert m.pair_evals == 3 * m2.body_steps + 2 * mtail.body_steps
    assert m.level_max == max(m2.level_max, mtail.level_max)
    assert m.level_clamped == m2.level_clamped + mtail.level_clamped
    assert np.array_equal(full.pos, tail.pos) and np.array_equal(full.vel, tail.vel)
    for at, left in ((1, 3), (2, 2)):
        c = ck.load(ck.path_for(ckdir, at))
        assert c.bodies.n == left and c.meta["block_steps"] and "level" in c.extra
        got, gids, gm, gstep = run_driver(b, steps=4, collisions="merge",
                                          resume=ck.path_for(ckdir, at), run_steps=4 - at, **kw)
        assert gstep == 4 and list(gids) == [0, 2] and gm.mergers == 1
        assert np.array_equal(got.pos, full.pos) and np.array_equal(got.vel, full.vel)


def test_periodic_work_never_runs_ahead_of_a_stopped_engine(hip, tmp_path):
    """Shared step, merger at step 71 of 120, a frame every 10 steps: 12 frames, each taken at its
    own step (3 bodies up to step 70, 2 from step 80), and one checkpoint per period."""
    b = merger_with_bystander()
    sim = Simulation(SimConfig(n=3, device="gpu", integrator="hermite", dt=1000.0, steps=120,
                               collisions="merge", record_every=10, checkpoint_every=40,
                               checkpoint_dir=str(tmp_path)))
    try:
        sim.engine.load(b)
        m = sim.run()
        frames = sim.trajectory
    finally:
        sim.close()
    assert m.mergers == 1 and m.steps_taken == 120
    assert [len(f) for f in frames] == [3] * 7 + [2] * 5
    for a, c in zip(frames[7:], frames[8:]):
        assert not np.array_equal(a, c)
    assert sorted(p.name for p in tmp_path.iterdir()) == \
        sorted(os.path.basename(ck.path_for(str(tmp_path), k)) for k in (40, 80, 120))
