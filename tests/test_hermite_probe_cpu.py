"""The Hermite marker probe without a GPU (tests/hermite_probe_helpers.py): its reference against
the dense oracle, the coverage and visibility conditions of every case of
tests/test_hermite_probe_gpu.py, mutation controls on a NumPy emulation of the chunked sum, and
the native CPU engine through the same probe at the smallest case.

Mutation controls: each takes the emulated partials of a case, breaks them the way an index
error in the kernels would, and asserts that the gate fails for at least 99.9 % of the affected
bodies and that locate() names the unit. One mutation of the issue's list cannot change a sum:
exchanging the partials of two chunks for one i-block leaves the same terms in the fold (only
their order changes, which the bitwise launch-shape comparisons of the GPU file pin); the control
asserts that, and then the form of that error that does lose a term: the i-block reads chunk
c1's partial in both slots, so c1 is doubled and c2 missing.
"""
import math

import numpy as np
import pytest

from gravsim.config import SimConfig
from gravsim.ops import oracle
from gravsim.runtime.hermite import HermiteCpuEngine

import hermite_nn_helpers as nnh
import hermite_probe_helpers as hp
from test_hermite_mixed_cpu import ds_seen

SMALL = 20000


# ---- 1. the reference itself -----------------------------------------------------------------
def _small_set(n=5000, K=64):
    m = np.unique(np.concatenate([[0, n - 1], np.arange(K - 2) * (n // K) + 17]))
    return hp.probe_bodies(n, seed=3, markers=m)


@pytest.mark.parametrize("dtype", hp.DTYPES)
def test_reference_matches_dense_oracle(dtype):
    """5,000 bodies, 64 markers: the O(K n) reference against oracle.acc_jerk over all columns
    (the massless columns add exact zeros there). The dense sum is a plain fp64 sum of K
    non-zero terms: K eps64 scale bounds its error (Higham eq. 4.4, first order)."""
    b, m = _small_set()
    p, v, mu = hp.seen(b, dtype)
    if dtype == "mixed":
        assert np.array_equal(p, ds_seen(b.pos))
    dense = oracle.acc_jerk(p, v, mu, G=1.0, with_potential=True, with_abs=True)
    ref = hp.reference(b, m, dtype)
    for got, want in zip(ref[3:], dense[3:]):  # the scales
        assert np.allclose(got, want, rtol=1e-13, atol=0)
    r = hp.ratios(*hp.as_rows4(dense), ref, "fp64")
    print(f"{dtype}: probe reference against the dense oracle {r.max():.2f} eps64 x scale")
    assert r.max() <= len(m)
    assert (ref[2] < 0).all() and np.abs(ref[1]).min() > 0


def test_fp64_reference_is_summed_to_two_eps():
    """The reference's own summation must not eat the gate: 64 bodies of the smallest case
    against (a) math.fsum, the exact sum of the same fp64 terms, and (b) the terms recomputed
    and summed in long double (where that is wider than double)."""
    b, m, ref = hp.probe_case(SMALL, "fp64")
    rows = np.linspace(0, SMALL - 1, 64).astype(int)
    p, v, mu = hp.seen(b, "fp64")
    ta, tj, tp = hp.pair_terms(p[rows], v[rows], p[m], v[m], mu[m])

    def exact(t):
        flat = t.reshape(len(rows), len(m), -1)
        return np.array([[math.fsum(flat[i, :, c]) for c in range(flat.shape[2])]
                         for i in range(len(rows))]).reshape(t.shape[:1] + t.shape[2:])

    scales = (ref[3][rows], ref[4][rows])
    r = hp.ratios(*hp.as_rows4(tuple(x[rows] for x in ref)),
                  (exact(ta), exact(tj), exact(tp)) + scales, "fp64")
    print(f"two-sum against the exact sum: {r.max():.3f} eps64 x scale")
    assert r.max() <= 2.0
    if np.finfo(np.longdouble).eps < 2.0 ** -60:
        L = np.longdouble
        la, lj, lp = hp.pair_terms(p[rows].astype(L), v[rows].astype(L), p[m].astype(L),
                                   v[m].astype(L), mu[m].astype(L))
        wide = tuple(hp.two_sum_reduce(t).astype(np.float64) for t in (la, lj, lp))
        r = hp.ratios(*hp.as_rows4(tuple(x[rows] for x in ref)), wide + scales, "fp64")
        print(f"fp64 terms against long double terms: {r.max():.3f} eps64 x scale")
        assert r.max() <= 2.0


@pytest.mark.parametrize("dtype", hp.DTYPES)
def test_nn_reference_matches_dense_oracle(dtype):
    b, m = _small_set()
    q, nn, q2 = hp.nn_over_markers(b, m, dtype)
    pos, rad = nnh.seen(b.pos, b.radius, dtype)
    oq, onn, oq2 = oracle.nearest_neighbours(pos, rad, hp.CUTOFF, second=True)
    assert np.array_equal(nn, onn) and np.array_equal(q, oq) and np.array_equal(q2, oq2)
    assert np.isin(nn, m).all() and (q < 0).all()


# ---- 2. every case: geometry, coverage, visibility ---------------------------------------------
@pytest.mark.parametrize("n,dtype", hp.PROBE)
def test_case_geometry_coverage_and_visibility(n, dtype):
    want, g = hp.CASES[n], hp.geometry(n, dtype)
    assert (g["n_pad"], g["n_chunks"], g["slice"], g["n_slices"]) == \
        (want["n_pad"], want["n_chunks"], want["slice"], want["n_slices"])
    assert (g["ipl"], g["groups"]) == want["auto"][dtype]
    b, m, ref = hp.probe_case(n, dtype)  # (asserts the coverage)
    assert len(m) <= hp.MAX_MARKERS and not b.mass[np.setdiff1d(np.arange(n), m)].any()
    assert (np.abs(b.vel).max(1) > 0).all()
    rest = np.setdiff1d(np.arange(n), m)
    d = np.sqrt(((b.pos[rest[::7], None, :] - b.pos[m][None, :, :]) ** 2).sum(-1))
    assert d.max() / d.min() <= 5.01  # all (body, marker) distances within a factor 5
    vis = hp.visibility(b, m, ref, dtype)
    print(f"n={n} {dtype}: K {len(m)}, hidden shares {vis} (1 / n = {1 / n:.2e}: the self terms)")
    assert max(vis.values()) <= 1e-4
    if dtype == "mixed":
        shift = hp.hi_only_shift(b, m, ref)[rest]
        print(f"n={n} mixed: the hi parts alone move the reference by {shift.min():.0f} .. "
              f"{shift.max():.0f} x 2^-24 x scale")
        assert shift.min() > 10.0 * hp.GATE
    if n in hp.NN_SIZES:
        q, nn, _ = hp.nn_reference(n, dtype)
        home = hp.winners_home(n, dtype)
        act = hp.active_list(n, dtype, m)
        ex = (hp.check_nn(np.array(q), np.array(nn), n, dtype),
              hp.check_nn(q[act], nn[act], n, dtype, rows=act))
        print(f"n={n} {dtype}: winners per chunk >= {home[0]}, per slice >= {home[1]}; excused "
              f"by the reference alone {ex[0]:.5f}, on the active list {ex[1]:.5f}")
        assert min(home) >= 64


def test_geometries_reach_what_they_are_for():
    """The structures the cases were chosen for (the table of tests/test_hermite_probe_gpu.py)."""
    assert hp.every_tile_end(20000) and not hp.every_tile_end(40000)
    assert [hp.geometry(20000, "fp32", groups=k)["per"] for k in (1, 3, 7, 20)] == [20, 7, 3, 1]
    assert hp.geometry(20000, "fp32", groups=7)["short_last"] == 2  # 3 + 3 + ... + 2
    assert [c // hp.HERMITE_UNIT for _, c in hp.rank_rows(20000, 3)] == [7, 7, 6]
    assert [c // hp.HERMITE_UNIT for _, c in hp.rank_rows(66000, 7)] == [10, 10, 10, 9, 9, 9, 9]
    assert (hp.geometry(40000, "fp32")["tpc"], hp.geometry(40000, "fp64")["tpc"]) == (32, 64)
    g = hp.geometry(66000, "fp32")
    assert (g["per"], g["used_groups"], g["groups"] - g["used_groups"], g["short_last"]) == \
        (2, 17, 15, 1)
    g = hp.geometry(66000, "fp64")
    assert (g["per"], g["used_groups"], g["groups"] - g["used_groups"]) == (3, 11, 5)
    assert g["last_slice_real"] == 0                                   # ghost rows only
    assert hp.geometry(67584, "fp32")["last_slice_real"] == 1024      # rows 66,560 ..
    g = hp.geometry(135000, "fp32")
    assert (g["chunk"], g["tpc"], g["per"], 58 * g["slice"], g["last_slice_real"]) == \
        (4096, 16, 3, 133632, 1368)
    assert hp.geometry(262144, "mixed")["chunk"] == 4096
    assert hp.geometry(135000, "mixed", nn=True)["ipl"] == 2


# ---- 3. mutation controls ----------------------------------------------------------------------
def _caught(a4, j4, n, dtype, affected, rows=None):
    r = hp.ratios(a4, j4, hp.probe_case(n, dtype)[2], dtype, rows).max(1)
    return float((r[affected] > hp.GATE).mean()), float(np.delete(r, affected).max(initial=0.0))


@pytest.fixture(scope="module")
def tiles():
    """Tile partials of the smallest case in fp32 (80 tiles of 256 rows, 20 chunks of 4)."""
    g = hp.geometry(SMALL, "fp32")
    P = hp.unit_partials(SMALL, "fp32", np.arange(g["n_pad"] // g["tile"]) * g["tile"])
    P.setflags(write=False)
    return g, P


def _chunks(g, P):
    """The chunk partials: the tiles of a chunk added in order, from zero."""
    out = np.zeros((g["n_chunks"],) + P.shape[1:])
    for t in range(P.shape[0]):
        out[t // g["tpc"]] += P[t]
    return out


def test_emulation_passes_unbroken(tiles):
    g, P = tiles
    w = hp.assert_gate(*hp.fold(_chunks(g, P)), SMALL, "fp32", label="emulation")
    assert max(w) < 1.0  # (fp64 sums against an fp32 gate)


@pytest.mark.parametrize("chunk,tile", [(0, 0), (7, 2), (19, 2)])
def test_dropped_tile_is_caught_and_located(tiles, chunk, tile):
    g, P = tiles
    Q = np.array(P)
    Q[chunk * g["tpc"] + tile] = 0.0
    a4, j4 = hp.fold(_chunks(g, Q))
    share, _ = _caught(a4, j4, SMALL, "fp32", np.arange(SMALL))
    assert share >= 0.999
    top = hp.locate(a4, j4, SMALL, "fp32")[0]
    assert top["fitted"] == top["rows"] and len(top["units"]) == 1
    u = top["units"][0]
    assert (u["kind"], u["what"], u["chunk"], u["tile"]) == ("tile", "missing", chunk, tile)
    assert u["group"] == chunk and len(u["markers"]) == 2
    with pytest.raises(AssertionError, match="missing"):
        hp.assert_gate(a4, j4, SMALL, "fp32", label="dropped tile")


@pytest.mark.parametrize("what,factor", [("missing", 0.0), ("doubled", 2.0)])
def test_dropped_or_doubled_chunk_is_caught_and_located(tiles, what, factor):
    g, P = tiles
    C = _chunks(g, P)
    C[13] *= factor
    a4, j4 = hp.fold(C)
    share, _ = _caught(a4, j4, SMALL, "fp32", np.arange(SMALL))
    assert share >= 0.999
    top = hp.locate(a4, j4, SMALL, "fp32", ipl=2, groups=7)[0]
    assert top["fitted"] == top["rows"] and len(top["units"]) == 1
    u = top["units"][0]
    assert (u["kind"], u["what"], u["chunk"], u["group"]) == ("chunk", what, 13, 13 // 3)
    assert len(u["markers"]) == 8


def test_exchanged_partials_of_one_iblock(tiles):
    """Module docstring: the pure exchange changes no sum; the half-done one is caught."""
    g, P = tiles
    C = _chunks(g, P)
    blk = slice(3 * g["iblock"], 4 * g["iblock"])
    X = np.array(C)
    X[4, blk], X[11, blk] = C[11, blk], C[4, blk]
    assert max(hp.assert_gate(*hp.fold(X), SMALL, "fp32", label="exchange")) < 1.0
    X = np.array(C)
    X[11, blk] = C[4, blk]
    a4, j4 = hp.fold(X)
    affected = np.arange(blk.start, blk.stop)
    share, others = _caught(a4, j4, SMALL, "fp32", affected)
    assert share >= 0.999 and others < 1.0
    top = hp.locate(a4, j4, SMALL, "fp32")[0]
    assert top["fitted"] == top["rows"] and top["iblocks"] == [3]
    assert sorted((u["kind"], u["what"], u["chunk"]) for u in top["units"]) == \
        [("chunk", "doubled", 4), ("chunk", "missing", 11)]


def test_dropped_short_last_slice_is_caught_and_located():
    """67,584 bodies: the 53rd narrow slice has 1,024 rows, all real, with markers."""
    n, dtype = 67584, "fp32"
    g = hp.geometry(n, dtype)
    b, m, _ = hp.probe_case(n, dtype)
    act = hp.active_list(n, dtype, m)
    assert g["last_slice_real"] == 1024 and (m >= 52 * g["slice"]).sum() >= 2
    S = hp.unit_partials(n, dtype, np.arange(g["n_slices"]) * g["slice"], rows=act)
    assert max(hp.assert_gate(*hp.fold(S), n, dtype, rows=act, label="slices")) < 1.0
    S[52] = 0.0
    a4, j4 = hp.fold(S)
    share, _ = _caught(a4, j4, n, dtype, np.arange(len(act)), rows=act)
    assert share >= 0.999
    top = hp.locate(a4, j4, n, dtype, rows=act, narrow=True)[0]
    assert top["fitted"] == top["rows"] and len(top["units"]) == 1
    u = top["units"][0]
    assert (u["kind"], u["what"], u["slice"]) == ("slice", "missing", 52)
    assert len(top["where"]) > 40  # (the failing rows come from all over the list)


def test_rows_of_another_rank_are_caught_and_located(tiles):
    """P = 3 at 20,000 bodies (7 + 7 + 6 units): rank 0 reads its rows out of rank 1's
    partials, the local row kept, as a wrong row0 or a wrong stride would do."""
    g, P = tiles
    a4, j4 = (np.array(x) for x in hp.fold(_chunks(g, P)))
    (r0, c0), (r1, c1), _ = hp.rank_rows(SMALL, 3)
    assert (r0, c0, r1, c1) == (0, 7168, 7168, 7168)
    a4[r0:r0 + c0], j4[r0:r0 + c0] = a4[r1:r1 + c1].copy(), j4[r1:r1 + c1].copy()
    share, others = _caught(a4, j4, SMALL, "fp32", np.arange(r0, r0 + c0))
    assert share >= 0.999 and others < 1.0
    top = hp.locate(a4, j4, SMALL, "fp32", P=3)[0]
    assert (top["kind"], top["rank"], top["holds_rank"]) == ("rows of another rank", 0, 1)
    assert top["fitted"] == top["rows"] and top["where"] == [("rank", 0)]


# ---- 4. the native CPU engine through the probe ------------------------------------------------
@pytest.mark.parametrize("dtype", hp.DTYPES)
def test_cpu_engine_passes_the_probe(dtype):
    """gs_cpu_accjerk_* and gs_cpu_nn_* at 20,000 bodies in 20 chunks of 1024."""
    b, m, _ = hp.probe_case(SMALL, dtype)
    eng = HermiteCpuEngine(SimConfig(n=SMALL, dtype=dtype, device="cpu", integrator="hermite",
                                     chunk=1024, collisions="detect", dt=1.0).validate())
    try:
        eng.load(b, acc=np.zeros((SMALL, 3)), jerk=np.zeros((SMALL, 3)))
        a4, j4, q, nn = eng.derivs_nn()
    finally:
        eng.close()
    w = hp.assert_gate(a4, j4, SMALL, dtype, label=f"cpu engine {dtype}")
    ex = hp.check_nn(q, nn, SMALL, dtype)
    print(f"cpu engine n={SMALL} {dtype}: acc {w[0]:.1f} jerk {w[1]:.1f} phi {w[2]:.1f} "
          f"(x eps x scale), nn excused {ex:.5f}")
