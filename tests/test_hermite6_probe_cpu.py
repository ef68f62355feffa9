"""The order-6 marker probe without a GPU (tests/hermite6_probe_helpers.py): its reference against
the dense oracle, the launch shapes by hand, what the gate can see of the snap in every fp32 case
of tests/test_hermite6_probe_gpu.py, mutation controls on a NumPy emulation of the chunked sum,
the native CPU engine through the probe at the smallest case, and one step of the CPU engine from
a supplied state.

Mutation controls: each takes the emulated partials of the 20,000-body case, breaks them the way
an index error in hermite6_eval_kernel would, and asserts that the snap gate fails for at least
99.9 % of the bodies and that locate() names the chunk: a dropped tile, a dropped chunk, a
doubled chunk (the missed reset after a flush), and a chunk whose `ta` tile alone came from the
previous chunk, which leaves a and j exact and is named by the fit of the acceleration rows.
"""
import numpy as np
import pytest

from gravsim.config import SimConfig
from gravsim.ops import oracle
from gravsim.ops.force import acc_jerk_snap
from gravsim.runtime.hermite import HermiteCpuEngine

import hermite6_probe_helpers as h6p
import hermite_probe_helpers as hp

SMALL = 20000


# ---- 1. the reference itself -----------------------------------------------------------------
@pytest.mark.parametrize("dtype", h6p.DTYPES)
def test_reference_matches_dense_oracle(dtype):
    """5,000 bodies, 64 markers, acceleration rows of the test's own: the O(K n) reference against
    oracle.acc_jerk_snap over all columns (the massless columns add exact zeros there). The dense
    sum is a plain fp64 sum of K non-zero terms: K eps64 scale bounds its error (Higham eq. 4.4,
    first order)."""
    n = 5000
    m = np.unique(np.concatenate([[0, n - 1], np.arange(62) * (n // 64) + 17]))
    b, m = hp.probe_bodies(n, seed=3, markers=m)
    acc_in = np.random.default_rng(5).normal(size=(n, 3)) * 0.05
    vw = h6p.view(b, m, dtype, acc_in)
    assert np.array_equal(vw.acc, h6p.quantize(acc_in, dtype))
    dense = oracle.acc_jerk_snap(vw.p, vw.v, vw.acc, vw.mu, G=1.0, with_potential=True,
                                 with_abs=True)
    ref = h6p.reference(vw)
    for got, want in zip(ref[4:], dense[4:]):  # the scales
        assert np.allclose(got, want, rtol=1e-13, atol=0)
    z = np.zeros((n, 1))
    a4, j4, s4 = np.concatenate([dense[0], dense[3][:, None]], 1), \
        np.concatenate([dense[1], z], 1), np.concatenate([dense[2], z], 1)
    r = h6p.ratios(a4, j4, s4, ref, "fp64")
    print(f"{dtype}: probe reference against the dense oracle {h6p.fmt(h6p.worst4(r))} "
          "eps64 x scale")
    assert r.max() <= len(m)
    assert (ref[3] < 0).all() and np.abs(ref[2]).min() > 0


# ---- 2. every case: launch shape and what the gate sees of the snap ---------------------------
@pytest.mark.parametrize("n,dtype", h6p.PROBE)
def test_auto_launch_shapes_by_hand(n, dtype):
    g = h6p.geometry(n, dtype)
    assert (g["n_pad"], g["n_chunks"]) == (hp.CASES[n]["n_pad"], hp.CASES[n]["n_chunks"])
    assert (g["ipl"], g["groups"], g["per"], g["groups"] - g["used_groups"]) == h6p.AUTO[n][dtype]


def test_geometries_reach_what_they_are_for():
    assert h6p.geometry(20000, "fp32")["n_chunks"] == 20
    # two bodies a lane would leave 40 x 20 = 800 < 1024 workgroup-chunks
    assert 20480 // 512 * 20 < 1024 and h6p.launch_shape(20480, 20, "fp32") == (1, 20)
    assert [h6p.geometry(20000, "fp32", 2, k)["per"] for k in (1, 3, 7, 20)] == [20, 7, 3, 1]
    assert h6p.geometry(20000, "fp32", 2, 7)["short_last"] == 2
    assert h6p.launch_shape(20480, 20, "fp64", ipl=2)[0] == 1  # (no fp64 form with 2)
    assert (h6p.geometry(40000, "fp32")["tpc"], h6p.geometry(40000, "fp64")["tpc"]) == (32, 64)
    assert h6p.geometry(40000, "fp32", groups=2)["per"] == 3   # 3 + 2 long chunks
    g = h6p.geometry(66000, "fp32")
    assert (g["tpc"], g["per"], g["used_groups"], g["short_last"]) == (8, 3, 11, 0)
    g = h6p.geometry(66000, "fp64")
    assert (g["tpc"], g["per"], g["used_groups"], g["short_last"]) == (16, 5, 7, 3)
    g = h6p.geometry(135000, "fp32")
    assert (g["chunk"], g["tpc"], g["per"], g["short_last"]) == (4096, 16, 5, 3)
    g = h6p.geometry(135000, "fp64")
    assert (g["tpc"], g["per"], g["used_groups"], g["short_last"]) == (32, 9, 4, 6)
    g = h6p.geometry(262144, "fp32")
    assert (g["n_chunks"], g["tpc"], g["per"]) == (64, 16, 16)
    # the last partial row of the largest case, in rows of 16 or 32 bytes: the index needs 64 bits
    # in bytes only (64 x 262,144 x 16 = 2^28)
    assert 64 * 262144 < 2 ** 31


@pytest.mark.parametrize("n", sorted(h6p.AUTO))
def test_snap_is_visible_to_the_gate(n):
    """fp32 (fp64 is ten orders of magnitude clearer), acc_in the rounded reference acceleration:
    the conditions under which the GPU test cannot pass vacuously. The single-term cap is 1e-3,
    not the 1e-4 of a and j: the q part is a few per cent of the snap's scale here."""
    vw, ref = h6p.cpu_case(n, "fp32")
    vis = h6p.snap_visibility(vw, ref, h6p.geometry(n, "fp32"))
    print(f"n={n} fp32: K {len(vw.m)}: {vis}")
    assert vis["term"] <= 1e-3
    assert vis["chunk"] == 0
    assert vis["acc_rows"] <= 1e-5
    assert vis["q_move"] > 10.0


# ---- 3. mutation controls ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiles():
    """Tile partials of the smallest case in fp32 (80 tiles of 256 rows, 20 chunks of 4)."""
    vw, ref = h6p.cpu_case(SMALL, "fp32")
    g = h6p.geometry(SMALL, "fp32", ipl=2, groups=7)
    P = h6p.unit_partials(vw, np.arange(g["n_pad"] // g["tile"]) * g["tile"])
    P.setflags(write=False)
    return vw, ref, g, P


def _chunks(g, P):
    out = np.zeros((g["n_chunks"],) + P.shape[1:])
    for t in range(P.shape[0]):
        out[t // g["tpc"]] += P[t]
    return out


def _snap_caught(rows, vw, ref):
    r = h6p.ratios(*rows, ref, vw.dtype)[:, 6:9].max(1)
    return float((r > h6p.GATE).mean())


def test_emulation_passes_unbroken(tiles):
    vw, ref, g, P = tiles
    w = h6p.assert_gate(*h6p.fold(_chunks(g, P)), vw, ref, g, label="emulation")
    assert max(w) < 1.0  # (fp64 sums against an fp32 gate)


@pytest.mark.parametrize("chunk,tile", [(0, 0), (7, 2), (19, 2)])
def test_dropped_tile_is_caught_and_located(tiles, chunk, tile):
    vw, ref, g, P = tiles
    Q = np.array(P)
    Q[chunk * g["tpc"] + tile] = 0.0
    rows = h6p.fold(_chunks(g, Q))
    assert _snap_caught(rows, vw, ref) >= 0.999
    top = h6p.locate(*rows, vw, ref, g)[0]
    assert top["fitted"] == top["rows"] and len(top["units"]) == 1
    u = top["units"][0]
    assert (u["kind"], u["what"], u["chunk"], u["tile"]) == ("tile", "missing", chunk, tile)
    assert u["group"] == chunk // 3
    with pytest.raises(AssertionError, match="missing"):
        h6p.assert_gate(*rows, vw, ref, g, label="dropped tile")


@pytest.mark.parametrize("what,factor", [("missing", 0.0), ("doubled", 2.0)])
def test_dropped_or_doubled_chunk_is_caught_and_located(tiles, what, factor):
    vw, ref, g, P = tiles
    C = _chunks(g, P)
    C[13] *= factor
    rows = h6p.fold(C)
    assert _snap_caught(rows, vw, ref) >= 0.999
    top = h6p.locate(*rows, vw, ref, g)[0]
    assert top["fitted"] == top["rows"] and len(top["units"]) == 1
    u = top["units"][0]
    assert (u["kind"], u["what"], u["chunk"], u["group"]) == ("chunk", what, 13, 13 // 3)
    assert len(u["markers"]) == 8


def test_stale_acceleration_tile_is_caught_and_located(tiles):
    """Chunk 13 sweeps the (x, mu) and (v, 0) rows of its own j bodies and the (ap, 0) rows of
    chunk 12's: a and j stay exact, the snap fails, and the fit names chunk 13."""
    vw, ref, g, P = tiles
    mine = (vw.m // g["chunk"]) == 13
    acc_m = vw.acc[vw.m].copy()
    acc_m[mine] = vw.acc[vw.m[mine] - g["chunk"]]
    Q = h6p.unit_partials(vw, np.arange(g["n_chunks"]) * g["chunk"], acc_m=acc_m)
    rows = h6p.fold(Q)
    r = h6p.ratios(*rows, ref, "fp32")
    assert np.delete(r, (6, 7, 8), 1).max() < 1.0
    assert _snap_caught(rows, vw, ref) >= 0.999
    top = h6p.locate(*rows, vw, ref, g)[0]
    assert top["kind"] == "acc rows" and top["fitted"] == top["rows"]
    u = top["units"][0]
    assert (u["kind"], u["chunk"], u["group"]) == ("chunk", 13, 13 // 3)
    assert u["markers"] == vw.m[mine].tolist()
    with pytest.raises(AssertionError, match="other acceleration rows"):
        h6p.assert_gate(*rows, vw, ref, g, label="stale ta tile")


# ---- 4. the native CPU engine ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", h6p.DTYPES)
def test_cpu_engine_passes_the_probe(dtype):
    """gs_cpu_accjerksnap_* at 20,000 bodies in 20 chunks of 1024, the snap against the reference
    at the acceleration rows the second pass read (the first pass's output)."""
    b, m = h6p.probe_bodies(SMALL)
    a, j, s, phi = acc_jerk_snap(b.pos, b.vel, b.mass, device="cpu", dtype=dtype, chunk=1024)
    z = np.zeros((SMALL, 1))
    a4, j4, s4 = np.concatenate([a, phi[:, None]], 1), np.concatenate([j, z], 1), \
        np.concatenate([s, z], 1)
    vw, ref = h6p.case_reference(SMALL, dtype, a)
    w = h6p.assert_gate(a4, j4, s4, vw, ref, h6p.geometry(SMALL, dtype),
                        label=f"cpu engine {dtype}")
    print(f"cpu engine n={SMALL} {dtype}: {h6p.fmt(w)} (x eps x scale)")


@pytest.mark.parametrize("dtype", h6p.DTYPES)
@pytest.mark.parametrize("n", h6p.STEP_SIZES)
def test_cpu_engine_one_step_from_a_supplied_state(n, dtype):
    """h6p.check_supplied_step on the CPU engine: the same gates as the GPU engine's."""
    eng = HermiteCpuEngine(SimConfig(n=n, dtype=dtype, device="cpu", integrator="hermite",
                                     hermite_order=6, dt=h6p.STEP_H, eta=h6p.STEP_ETA).validate())
    out = h6p.check_supplied_step(eng, n, dtype, label=f"cpu step n {n} {dtype}")
    print(f"cpu step n={n} {dtype}: {h6p.fmt(out['worst'])}; v1 {out['v']:.2f} x1 {out['x']:.2f} "
          f"of {h6p.CORRECT_ROUNDINGS} u sum |terms|; crackle {out['crackle']:.2f} of its bound; "
          f"dt_next {out['dt_next']:.6g} ({out['dt_rel']:.1e} relative), body {out['row']}")
