"""The marker probe of the sym schedule (tests/sym_probe_helpers.py) checked on the CPU: its
reference against the NumPy oracle, the coverage of every geometry the GPU probe runs, its
sensitivity (which terms could vanish unseen), its mutation controls (a dropped or doubled
block of terms fails the gate and is located) and a correct engine passing it.

Reference: cuda.cu:53-60 visits each pair once and scatters both sides; the sym schedule does
so by chunk pairs, and the probe makes every chunk pair visible in every body's sum.
"""
import ctypes

import numpy as np
import pytest

from gravsim.ops import _native, oracle
from gravsim.ops.force import cpu_accelerations

import sym_probe_helpers as sp


@pytest.mark.parametrize("n", [3000, 20000])
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_reference_equals_oracle(n, dtype):
    """The helper's K-term sums against oracle.accelerations on the same quantised bodies
    (the massless bodies' terms are exact zeros there; the sources of the 20000-body case are
    the markers alone, oracle.acc_jerk's `sources`, the same pair law). The two differ by the
    oracle's plain summation (K - 1 roundings) and a few roundings per term."""
    b, m = sp.probe_bodies(n, dtype, seed=3)
    acc, absacc = sp.reference(b, m, dtype)
    pos, _, mu = sp.seen(b, dtype)
    if n <= 3000:
        ref, _, absref = oracle.accelerations(pos, mu, G=1.0, with_potential=True, with_abs=True)
    else:
        ref, _, absref, _ = oracle.acc_jerk(pos, np.zeros_like(pos), mu, G=1.0, with_abs=True,
                                            sources=m)
    u = 2.0 ** -53
    assert (np.abs(absacc - absref) <= (len(m) + 8) * u * absref).all()
    assert (np.abs(acc - ref) <= (len(m) + 8) * u * absref).all()
    assert (absref[np.setdiff1d(np.arange(n), m)] > 0).all()


def test_reference_cutoff_is_the_hard_select():
    """cutoff= drops exactly the pairs with r^2 < cutoff^2 (oracle.accelerations' select)."""
    b, m = sp.probe_bodies(3000, "fp64", seed=4)
    pos = b.pos.copy()
    pos[7] = pos[m[1]] + np.array([3e7, 0.0, 0.0])
    b = sp.BodySet(pos, b.vel, b.mass)
    acc, absacc = sp.reference(b, m, "fp64", cutoff=1e8)
    ref, _, absref = oracle.accelerations(pos, sp.G_SI * b.mass, G=1.0, cutoff=1e8,
                                          with_potential=True, with_abs=True)
    assert (np.abs(acc - ref) <= 16 * 2.0 ** -53 * absref).all()
    full, _ = sp.reference(b, m, "fp64")
    assert np.abs(full[7] - acc[7]).max() > 0.5 * np.abs(full[7]).max()  # the twin's main term


@pytest.mark.parametrize("n", sorted(sp.SYM_CASES))
def test_geometry_table_matches_native(n):
    """The geometry each probe case expects (L, D, split segments, rows per block) is what
    the native library computes, and the Python mirror agrees."""
    lib = _native.cpu_lib()
    want = sp.SYM_CASES[n]
    v = [ctypes.c_int32() for _ in range(5)]
    assert lib.gs_sym_geometry(want["n_pad"], *[ctypes.byref(x) for x in v]) == 0
    NC, H, L, S, D = (x.value for x in v)
    assert (NC, L, S, D) == (want["NC"], want["L"], want["S"], want["D"]) and H == NC // 2
    assert lib.gs_sym_split_segments(want["n_pad"]) == want["Kr"]
    if want["Kr"]:
        assert lib.gs_sym_split_parts(want["n_pad"]) == want["Np"]
    g = sp.geometry(n)
    assert {k: g[k] for k in want} == want


@pytest.mark.parametrize("n,dtype", sp.SYM_PROBE)
def test_coverage_holds(n, dtype):
    m = sp.place_markers(n, dtype)
    sp.assert_coverage(n, m)
    real = -(-n // sp.C)
    per_chunk = np.bincount(m // sp.C, minlength=real)
    assert (per_chunk >= (2 if n <= 131072 else 1)).all() and len(m) <= 256
    assert m[0] == 0 and m[-1] == n - 1
    assert {0, 63, 64, 127} <= set((m % sp.Q).tolist())


def test_coverage_notices_a_gap():
    """Taking the only markers of one quantum out of the antipodal servers is reported."""
    n = 65536
    m = sp.place_markers(n)
    assert not any(sp.coverage(n, m).values())
    q3 = m[(m % sp.C) // sp.Q == 3]
    gone = sp.coverage(n, np.setdiff1d(m, q3))
    assert (16, 3) in gone["shell"] and (1, 3) in gone["shell"]
    lo = m[(m % sp.C) < sp.C // 8]
    assert sp.coverage(n, np.setdiff1d(m, lo))["diag"] == [0]


@pytest.mark.parametrize("n,dtype", sp.SYM_PROBE + [(12000, "fp32"), (12000, "fp64")])
def test_sensitivity_share(n, dtype):
    """A condition on the data, not a measurement: the (body, marker) pairs whose term lies
    within the gate in all three components could vanish unseen. Their share must be <= 1e-4.
    With these data they are the K self-pairs (term zero) and nothing else in fp64 and up to
    90000 bodies in fp32; the fp32 gate at K >= 74 also hides a few far markers from a body
    next to a near one (524288: 1253 of 1.3e8 pairs, share 9.3e-6; 12000: share 8.3e-5)."""
    b, m, acc, absacc = sp.probe_case(n, dtype)
    blind = sp.blind_pairs(b, m, absacc, dtype)
    assert blind >= len(m)  # the self-pairs are always among them
    share = blind / (n * len(m))
    print(f"n {n} {dtype} K {len(m)}: blind pairs {blind} (self-pairs {len(m)}), "
          f"share {share:.2e}")
    assert share <= 1e-4


def _block(n, dtype, kind):
    """(bodies of i chunk A, marker, expected unit fields) of one mutation block."""
    g = sp.geometry(n)
    NC, L, D = g["NC"], g["L"], g["D"]
    m = sp.place_markers(n, dtype)
    h = sp.shell_lens(NC)
    d = {"diag": 0, "d1": 1, "antipodal": NC // 2}[kind]
    # the first marker from a third of the way in whose i chunk A = B - d is a real row
    mk = next(int(x) for x in np.roll(m, -(len(m) // 3))
              if (int(x) // sp.C - d) % NC < g["real_chunks"])
    B = mk // sp.C
    if kind == "diag":
        want = dict(A=B, B=B, d=0, row=B, side="i", kind="diagonal",
                    part=(mk % sp.C) // (sp.C // D))
    else:
        A = (B - d) % NC
        owns = d <= h[A]
        assert owns or NC - d <= h[B]  # one of the two rows holds the pair
        want = dict(A=A, B=B, d=d, row=A if owns else B, side="i" if owns else "j",
                    kind="segment")
        if owns:  # (on the j side the segment follows the body's own quantum)
            want["segment"] = ((d - 1) * 16 + (mk % sp.C) // sp.Q) // L
    rows = np.arange(want["A"] * sp.C, min(n, (want["A"] + 1) * sp.C))
    return rows, mk, want


@pytest.mark.parametrize("n,dtype", [(65536, "fp32"), (150000, "fp64"), (40000, "fp32")])
@pytest.mark.parametrize("kind", ["d1", "antipodal", "diag"])
@pytest.mark.parametrize("what", ["missing", "doubled"])
def test_mutation_is_caught_and_located(n, dtype, kind, what):
    """Control on the reference alone: drop (or double) the terms of one (i chunk, marker)
    block. The gate fails, and locate names that block: chunks, distance, owning row, side,
    segment."""
    b, m, acc, absacc = sp.probe_case(n, dtype)
    rows, mk, want = _block(n, dtype, kind)
    pos, _, mu = sp.seen(b, dtype)
    t = sp.pair_terms(pos[rows], pos[[mk]], mu[[mk]])[:, 0, :]
    got = acc.copy()
    got[rows] += t if what == "doubled" else -t
    hit = rows[rows != mk]  # (the marker's own term is zero)
    ratio = sp.gate_ratio(got, acc, absacc, dtype).max(1)
    assert (ratio[hit] > sp.GATE).all() and (np.delete(ratio, hit) == 0).all()
    with pytest.raises(AssertionError, match="units"):
        sp.assert_probe_gate(got, acc, absacc, m, b, dtype)
    found = sp.locate(got, acc, absacc, m, b, dtype, worst=64)
    assert found and all(e["marker"] == mk and e["what"] == what for e in found)
    assert sum(e["bodies"] for e in found) == len(hit) == sum(e["fitted"] for e in found)
    for e in found:
        for k, v in want.items():
            assert e[k] == v, (k, e, want)
    if want["side"] == "j":  # the j-side segments follow the bodies' quanta: all 16 / L hit
        g = sp.geometry(n)
        segs = {e["segment"] for e in found}
        d_own = (want["A"] - want["B"]) % g["NC"]
        full = len(rows) == sp.C
        assert not full or segs == set(range((d_own - 1) * 16 // g["L"], d_own * 16 // g["L"]))


def test_gate_passes_the_unmutated_reference():
    b, m, acc, absacc = sp.probe_case(65536, "fp32")
    assert sp.assert_probe_gate(acc, acc, absacc, m, b, "fp32") == 0.0
    assert sp.locate(acc, acc, absacc, m, b, "fp32") == []


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_cpu_engine_passes_the_probe(dtype):
    """The probe accepts a correct engine: the native CPU engine on a 16384-body probe set."""
    n = 16384
    b, m, acc, absacc = sp.probe_case(n, dtype)
    got, _ = cpu_accelerations(b.pos, b.mass, dtype=dtype)
    worst = sp.assert_probe_gate(got, acc, absacc, m, b, dtype, label=f"cpu {dtype}")
    print(f"cpu engine n {n} {dtype} K {len(m)}: worst ratio {worst:.2f}")
