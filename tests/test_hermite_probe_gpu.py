"""Marker probe of the Hermite evaluate kernels on the GPU: every body against a reference at the
geometries that only exist at size (tests/hermite_probe_helpers.py).

hermite_eval_kernel sweeps the j rows chunk by chunk in LDS tiles and flushes one partial per
chunk; the grid's y extent splits the chunks into groups; hermite_narrow_kernel splits the j rows
into up to 64 slices; the SLICE forms evaluate one rank's rows with their own partial stride; the
reduce kernels fold the partials (and, with collisions on, the nearest neighbour of each). The
tests of these kernels against the oracle stop at 4,097 bodies (3 chunks), and the larger inputs
of the suite have massive bodies in 5 workgroups only. Here all bodies but K <= 256 markers are
massless and the markers sit in every chunk, tile end, narrow slice and rank unit, so a lost,
doubled or misrouted partial of any chunk is far above the gate for every body, all n bodies
are gated on a, j and phi at |err| <= 128 eps x scale (eps of the pair type), and a failure
names the markers, chunk, tile, chunk group, i-block, slice or rank (hermite_probe_helpers.locate).

Cases, with the geometry the engine's layout reported (n_pad, chunk, chunks, ipl, groups: asserted
against gs_hermite_layout; tiles per chunk and narrow slices: the helper's mirror of
nbody_hermite.hip, which the layout does not report):

    n        chunk        n_pad / chunks  what it reaches
    20,000   forced 1024  20,480 / 20     every tile's first and last row is a marker (fp64: one
                                          end of every 128-row tile); 20 narrow slices; 20 units
                                          for the rank splits; every ipl x 1, 3, 7, 20 groups
    40,000   forced 8192  40,960 / 5      32 (fp32) and 64 (fp64) tiles per chunk: the flush test
                                          and the prefetch over long chunks; also 2 groups (3 + 2)
    66,000   auto 2048    67,584 / 33     the auto shape with a short last group and empty groups
                                          (fp32: ipl 4, 32 groups of 2, 15 empty; fp64: ipl 2, 16
                                          of 3, 5 empty); 53 slices of 1280, the last ghosts only
    67,584   auto 2048    67,584 / 33     no ghost row; the short last slice (rows 66,560 ..)
                                          holds bodies and markers
    135,000  auto 4096    135,168 / 33    4096-row chunks (16 / 32 tiles), groups of 3 (fp32) and
                                          5 (fp64); 59 slices of 2304, the short last one (from
                                          row 133,632) with bodies
    262,144  auto 4096    262,144 / 64    the benchmark size; fp32 and mixed only

Worst ratios |got - ref| / (eps x scale) over all bodies on one MI355X, acc / jerk / phi (the gate
is 128 and stays there); shared step = every launch shape = wide path = every rank count, which
are bitwise equal; with collisions on the same figures again:

    n        K    fp32                fp64                mixed
    20,000   158  4.80 / 3.39 / 4.82  5.10 / 3.75 / 5.31  1.91 / 1.50 / 0.88
    40,000   256  4.48 / 2.64 / 4.58  4.70 / 3.03 / 4.59  3.77 / 2.29 / 3.76
    66,000   256  6.91 / 3.91 / 6.69  6.74 / 4.23 / 6.35  1.28 / 1.87 / 0.77
    67,584   256  6.63 / 4.49 / 6.73  6.82 / 4.46 / 6.33  1.47 / 1.60 / 0.71
    135,000  256  7.20 / 4.25 / 6.40  6.66 / 4.22 / 6.89  1.38 / 1.60 / 0.73
    262,144  256  9.01 / 6.70 / 9.56  -                   1.30 / 2.33 / 0.56

Narrow path, a list of 8,088 to 8,157 bodies (one of every workgroup, the markers, both sides of
every slice boundary, filled up evenly): at most 8.90 / 5.20 / 7.76 (fp32), 8.33 / 5.55 / 8.58
(fp64), 1.27 / 1.92 / 0.80 (mixed). Nearest neighbours: every index the reference's wherever its
best and second-best q are more than 2 B apart; share of bodies excused by a smaller gap, a
property of the inputs that tests/test_hermite_probe_cpu.py asserts from the reference alone: at
most 0.0015 over all bodies and 0.0042 on the list (fp32, mixed), 0 in fp64.

Wall time of a test, load and read-back included: the first of a case also builds the reference on
the host (cached afterwards): 0.2 to 0.6 s in fp32 and mixed up to 135,000 bodies, 1.0 s at
262,144, and 0.5 to 2.6 s in fp64 (two-sum compensation); every other test 0.01 to 0.2 s, the
twelve launch shapes 0.06 s; the 61 together 17 s. No kernel change was needed.

Control on the device (a scratch build, not part of the suite): with the evaluate kernel changed
not to zero its sums after the flush of chunk 12, the 66,000-body cases fail at 2.5e6 (fp32,
mixed) and 1.4e15 (fp64) x eps x scale and the message names chunk 12, doubled, chunk group 6
(fp32) and 4 (fp64) for every i-block; at 20,000 bodies the auto shape (one chunk a group) passes
and the one-group shape fails the same way.
"""
import functools
import time

import numpy as np
import pytest

from gravsim.config import SimConfig
from gravsim.runtime.hermite import HermiteHipEngine, HermiteVirtualGroup

import hermite_probe_helpers as hp

pytestmark = pytest.mark.gpu

DT = 8.0  # [s] fixed step of the rank runs, and the block engines' largest step
IPLS = {"fp32": (1, 2, 4), "mixed": (1, 2, 4), "fp64": (1, 2)}
RANKS = [(n, P) for n in hp.CASES for P in hp.CASES[n]["ranks"]]


def _cfg(n, dtype, **kw):
    return SimConfig(n=n, dtype=dtype, device="gpu", integrator="hermite", dt=DT,
                     chunk=hp.CASES[n]["chunk"], **kw).validate()


def _block_cfg(n, dtype, **kw):
    return _cfg(n, dtype, block_steps=True, eta=0.02, **kw)


def _assert_layout(eng, n, dtype, ipl=0, groups=0, nn=False):
    """The case runs the geometry it was chosen for; returns it as text."""
    want, g, lay = hp.CASES[n], hp.geometry(n, dtype, ipl, groups, nn), eng.native_layout
    assert (lay["n_pad"], lay["chunk"], lay["n_chunks"]) == \
        (want["n_pad"], g["chunk"], want["n_chunks"])
    assert (lay["ipl"], lay["split_groups"]) == (g["ipl"], g["groups"]), lay
    if not (ipl or groups or nn):
        assert (lay["ipl"], lay["split_groups"]) == want["auto"][dtype]
    return (f"n_pad {lay['n_pad']} chunk {lay['chunk']} x {lay['n_chunks']} ({g['tpc']} tiles) "
            f"ipl {lay['ipl']} groups {lay['split_groups']} of {g['per']} "
            f"({g['groups'] - g['used_groups']} empty) slices {g['n_slices']} x {g['slice']}")


def _fmt(w):
    return f"acc {w[0]:.2f} jerk {w[1]:.2f} phi {w[2]:.2f}"


def _derivs(n, dtype, **kw):
    b = hp.probe_case(n, dtype)[0]
    eng = HermiteHipEngine(_cfg(n, dtype, **kw))
    try:
        geo = _assert_layout(eng, n, dtype, kw.get("ipl", 0), kw.get("split_groups", 0))
        eng.load(b)
        return eng.derivs() + (geo,)
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _auto(n, dtype):
    return _derivs(n, dtype)


# ---- a. the shared step's evaluate -------------------------------------------------------------
@pytest.mark.parametrize("n,dtype", hp.PROBE)
def test_shared_step_evaluate_every_body(hip, n, dtype):
    hp.probe_case(n, dtype)
    t0 = time.perf_counter()
    a4, j4, geo = _auto(n, dtype)
    w = hp.assert_gate(a4, j4, n, dtype, label=f"derivs n {n} {dtype}")
    print(f"probe n {n} {dtype} [{geo}]: {_fmt(w)} ({time.perf_counter() - t0:.2f} s)")
    if n == 40000:  # two groups of 3 and 2 long chunks: a flush inside a group's sweep
        a2, j2, _ = _derivs(n, dtype, split_groups=2)
        assert np.array_equal(a2, a4) and np.array_equal(j2, j4)


@pytest.mark.parametrize("dtype", hp.DTYPES)
def test_every_launch_shape_at_20000(hip, dtype):
    """Every ipl x 1, 3, 7, 20 chunk groups (20, 7, 3, 1 chunks a group; 7 groups leave the last
    one short): each at the gate and bitwise the auto shape."""
    n = 20000
    ref = _auto(n, dtype)
    t0 = time.perf_counter()
    for ipl in IPLS[dtype]:
        for groups in (1, 3, 7, 20):
            a4, j4, _ = _derivs(n, dtype, ipl=ipl, split_groups=groups)
            w = hp.assert_gate(a4, j4, n, dtype, label=f"n {n} {dtype} ipl {ipl} groups {groups}",
                               ipl=ipl, groups=groups)
            assert np.array_equal(a4, ref[0]) and np.array_equal(j4, ref[1]), (ipl, groups)
    print(f"shapes n {n} {dtype}: {len(IPLS[dtype]) * 4} shapes, {_fmt(w)} "
          f"({time.perf_counter() - t0:.2f} s)")


# ---- b. the block paths ------------------------------------------------------------------------
@pytest.mark.parametrize("n,dtype", hp.PROBE)
def test_block_paths_every_slice(hip, n, dtype):
    b, m, _ = hp.probe_case(n, dtype)
    act = hp.active_list(n, dtype, m)
    t0 = time.perf_counter()
    eng = HermiteHipEngine(_block_cfg(n, dtype))
    try:
        geo = _assert_layout(eng, n, dtype)
        eng.load(b)
        eng.set_block_tuning(narrow_max=8192)
        assert eng.status_narrow_max() == 8192 >= len(act)
        full = eng.derivs()
        wide = eng.derivs(active=np.arange(n, dtype=np.int32), path="wide")
        narrow = eng.derivs(active=act, path="narrow")
        back = eng.derivs(active=act[::-1].copy(), path="narrow")
    finally:
        eng.close()
    auto = _auto(n, dtype)
    assert np.array_equal(full[0], auto[0]) and np.array_equal(full[1], auto[1])
    assert np.array_equal(wide[0], full[0]) and np.array_equal(wide[1], full[1])
    w = hp.assert_gate(*narrow, n, dtype, rows=act, label=f"narrow n {n} {dtype}", narrow=True)
    assert np.array_equal(back[0][::-1], narrow[0]) and np.array_equal(back[1][::-1], narrow[1])
    print(f"block paths n {n} {dtype} [{geo}]: narrow list of {len(act)}: {_fmt(w)} "
          f"({time.perf_counter() - t0:.2f} s)")


# ---- c. ranks ----------------------------------------------------------------------------------
def _snap(eng):
    s, (a, j), st = eng.state(), eng.carried(), eng.status()
    return s.pos, s.vel, a, j, (st.time, st.steps)


@functools.lru_cache(maxsize=None)
def _one_rank(n, dtype):
    eng = HermiteHipEngine(_cfg(n, dtype))
    try:
        eng.load(hp.probe_case(n, dtype)[0])
        d = eng.derivs()
        eng.step(2)
        return d, _snap(eng)
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", hp.DTYPES)
@pytest.mark.parametrize("n,P", RANKS)
def test_rank_slices_equal_one_rank(hip, n, P, dtype):
    """P = 2, 3, 8 over 20 units and 5, 7 over 66: row0 up to row 57,344, uneven slices, P not
    dividing the units. derivs() and two fixed steps: bitwise the one-rank run."""
    b = hp.probe_case(n, dtype)[0]
    ref_d, ref_s = _one_rank(n, dtype)
    t0 = time.perf_counter()
    grp = HermiteVirtualGroup(_cfg(n, dtype), P)
    try:
        rows = [(e.native_layout["local_begin"], e.native_layout["n_local"]) for e in grp.shards]
        assert rows == hp.rank_rows(n, P)
        grp.load(b)
        a4, j4 = grp.derivs()
        grp.step(2)
        got = _snap(grp)
    finally:
        grp.close()
    w = hp.assert_gate(a4, j4, n, dtype, label=f"ranks n {n} P {P} {dtype}", P=P)
    assert np.array_equal(a4, ref_d[0]) and np.array_equal(j4, ref_d[1])
    for x, y in zip(got[:4], ref_s[:4]):
        assert np.array_equal(x, y)
    assert got[4] == ref_s[4] == (2 * DT, 2)
    assert (ref_s[0] != b.pos).any()
    print(f"ranks n {n} P {P} {dtype} rows {[c for _, c in rows]}: {_fmt(w)} "
          f"({time.perf_counter() - t0:.2f} s)")


# ---- d. nearest neighbours ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", hp.DTYPES)
@pytest.mark.parametrize("n", hp.NN_SIZES)
def test_nearest_neighbours_every_body(hip, n, dtype):
    """Collisions "detect": the nearest neighbour of every body is its nearest marker (module
    docstring of the helpers), and every chunk and narrow slice holds the winner for at least 64
    bodies, so the fold over PN / NNI picks it out of every partial."""
    b, m, _ = hp.probe_case(n, dtype)
    hp.nn_reference(n, dtype)
    assert min(hp.winners_home(n, dtype)) >= 64
    act = hp.active_list(n, dtype, m)
    t0 = time.perf_counter()
    eng = HermiteHipEngine(_block_cfg(n, dtype, collisions="detect"))
    try:
        geo = _assert_layout(eng, n, dtype, nn=True)
        if dtype == "mixed":
            assert eng.native_layout["ipl"] == 2  # (no 4-body tile with collisions on)
        eng.load(b)
        eng.set_block_tuning(narrow_max=8192)
        every = eng.derivs_nn()
        paths = {p: eng.derivs_nn(act, p) for p in ("narrow", "wide")}
    finally:
        eng.close()
    w = hp.assert_gate(every[0], every[1], n, dtype, label=f"nn n {n} {dtype}", nn=True)
    ex = [hp.check_nn(every[2], every[3], n, dtype)]
    for p, (a4, j4, q, nn) in paths.items():
        hp.assert_gate(a4, j4, n, dtype, rows=act, label=f"nn {p} n {n} {dtype}", nn=True,
                       narrow=p == "narrow")
        ex.append(hp.check_nn(q, nn, n, dtype, rows=act))
    print(f"nn n {n} {dtype} [{geo}]: {_fmt(w)}, excused all / narrow / wide "
          f"{ex[0]:.5f} / {ex[1]:.5f} / {ex[2]:.5f} ({time.perf_counter() - t0:.2f} s)")
