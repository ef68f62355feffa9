"""Marker probe of the Newton-3 sym schedule on the GPU: every body against a reference at every
geometry of the schedule (tests/sym_probe_helpers.py).

Reference: cuda.cu:53-60 evaluates each pair once and scatters +F / -F. The sym schedule does
that by chunk pairs whose index arithmetic changes with the padded size (gs_sym_geometry:
segment length L, diagonal parts D, split segments Kr x Np, row blocks of RB rows, all-ghost
rows and chunks, the fused or the three-kernel tail). All bodies but K <= 256 markers are
massless, so each body's acceleration is a sum of K terms: a dropped, doubled or misrouted
(row, segment part) partial is far above the gate 128 eps sum|term| for every body it
touches, and all n bodies are gated, from L = 1 with ghost rows to L = 16. A failure names
the unit (chunks, distance, owning row, i or j side, segment).

Also here: the one-sided path mode=auto picks at 12000 bodies, the hard cutoff across chunk
pairs (diagonal, d = 1, NC/2 - 1, NC/2) for every body, and the kick-drift of one step against
the step-path acceleration to two roundings at the sizes of both tails.

Worst ratios |got - ref| / (eps sum|term|) over all bodies on an MI355X (the gate is 128 and
stays there), fp32 / fp64; exact and fast cutoff modes give the same figures:

    n        K    geometry                          fp32    fp64
    40000    40   NC 24  L 1  D 16 RB 3             6.49    8.09
    65536    64   NC 32  L 2  D 8  Kr 8  Np 2       7.25    9.53
    90000    88   NC 48  L 2  D 8  Kr 12 Np 2 RB 3  9.14    9.93
    131072   128  NC 64  L 4  D 4  Kr 8  Np 4       9.65    11.66
    150000   74   NC 80  L 4  D 4  Kr 10 Np 4 RB 5  9.89    11.42
    262144   128  NC 128 L 8  D 2  Kr 8  Np 4       10.07   12.92
    524288   256  NC 256 L 16 D 1  Kr 8  Np 4       14.80   -
    12000    12   one-sided (mode auto -> split)    6.59    7.87

Cutoff case (65536, cutoff 1e8 m, exact): 7.25 / 9.53 over all bodies, the four twins at most
1.23 / 2.80. One step against the step-path acceleration: kick 0.50 and drift at most 0.69 of
the two-rounding bound in fp32, both exactly 0 in fp64: the step uses the bits of the query.
"""
import ctypes

import numpy as np
import pytest

from gravsim.config import SimConfig
from gravsim.models.initial_conditions import BodySet

import sym_probe_helpers as sp

pytestmark = pytest.mark.gpu

# n, dtypes, cutoff modes (None: the default)
_PROBE = [(n, dt, cm)
          for n, dt in sp.SYM_PROBE
          for cm in (("exact", "fast") if n in (65536, 131072) else (None,))]


def _engine(n, dtype, **kw):
    from gravsim.runtime.engines import HipEngine

    return HipEngine(SimConfig(n=n, dtype=dtype, device="gpu", **kw))


def _assert_geometry(e, n):
    """The case runs in the regime it was chosen for (a retune of gs_sym_geometry must not
    silently move it to another)."""
    want = sp.SYM_CASES[n]
    assert e.native_layout["mode"] == 3
    assert e.native_layout["n_pad"] == want["n_pad"]
    v = [ctypes.c_int32() for _ in range(5)]
    assert e.lib.gs_sym_geometry(want["n_pad"], *[ctypes.byref(x) for x in v]) == 0
    assert (v[0].value, v[2].value) == (want["NC"], want["L"])
    S, D, Kr, Np = e.sym_geometry()
    assert (S, D, Kr) == (want["S"], want["D"], want["Kr"])
    assert Np == want["Np"] or Kr == 0
    return f"NC {want['NC']} L {want['L']} S {S} D {D} Kr {Kr} Np {Np} RB {want['RB']}"


@pytest.mark.parametrize("n,dtype,cutoff_mode", _PROBE)
def test_sym_probe_every_body(hip, n, dtype, cutoff_mode):
    b, m, ref, absref = sp.probe_case(n, dtype)
    kw = {} if cutoff_mode is None else {"cutoff_mode": cutoff_mode}
    e = _engine(n, dtype, mode="sym", **kw)
    try:
        geo = _assert_geometry(e, n)
        e.load(b)
        if cutoff_mode is not None:
            assert e.force_mode()["exact"] == (cutoff_mode == "exact")
        got = e.accel(step_path=True)[:n, :3]
    finally:
        e.close()
    worst = sp.assert_probe_gate(got, ref, absref, m, b, dtype,
                                 label=f"sym n {n} {dtype} {cutoff_mode}")
    print(f"sym probe n {n} {dtype} cutoff_mode {cutoff_mode} K {len(m)} [{geo}]: "
          f"worst ratio {worst:.2f}")


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_one_sided_auto_probe_every_body(hip, dtype):
    """mode=auto below the sym threshold: the one-sided path at 12000 bodies (six 2048-body
    chunks, the last one partial), every body."""
    n = 12000
    b, m, ref, absref = sp.probe_case(n, dtype)
    e = _engine(n, dtype)
    try:
        assert e.native_layout["mode"] != 3
        mode = e.native_layout["mode"]
        e.load(b)
        got = e.accel(step_path=True)[:n, :3]
    finally:
        e.close()
    worst = sp.assert_probe_gate(got, ref, absref, m, b, dtype, label=f"auto n {n} {dtype}")
    print(f"one-sided probe n {n} {dtype} K {len(m)} [mode {mode}]: worst ratio {worst:.2f}")


def _twins(n, dtype, cutoff):
    """Probe bodies with four massless twins 3e7 m from a marker each, so that the (twin,
    marker) chunk pair is diagonal, d = 1, d = NC/2 - 1 and d = NC/2; no other (body, marker)
    pair within 1e-5 (relative, in r^2) of the cutoff (another seed if one is)."""
    g = sp.geometry(n)
    NC = g["NC"]
    for seed in range(8):
        b, m = sp.probe_bodies(n, dtype, seed=seed)
        pos = b.pos.copy()
        twins = []
        for k, d in enumerate((0, 1, NC // 2 - 1, NC // 2)):
            mk = int(m[(k * len(m)) // 4 + 1])
            A = (mk // sp.C - d) % NC
            i = A * sp.C + 1000 + 37 * k
            assert i < n and i not in m and i not in [t for t, _, _ in twins]
            step = np.zeros(3)
            step[k % 3] = 3e7
            pos[i] = pos[mk] + step
            twins.append((i, mk, d))
        b = BodySet(pos, b.vel, b.mass)
        p, _, _ = sp.seen(b, dtype)
        near = 0
        for i0 in range(0, n, 8192):
            dd = p[m][None, :, :] - p[i0:i0 + 8192, None, :]
            r2 = (dd * dd).sum(-1)
            near += int((np.abs(r2 - cutoff ** 2) <= 1e-5 * cutoff ** 2).sum())
        if not near:
            for i, mk, _ in twins:  # well inside the cutoff as the kernel sees them
                assert ((p[i] - p[mk]) ** 2).sum() < 0.25 * cutoff ** 2
            return b, m, twins
    raise AssertionError("no seed keeps every pair clear of the cutoff boundary")


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_sym_cutoff_excludes_pairs_across_chunk_pairs(hip, dtype):
    """The hard cutoff for every body (test_sym_exact_cutoff judges against the global max|a|
    only): a twin inside a marker's cutoff gets nothing from it, whether the row of the twin
    or the row of the marker evaluates the pair, and every other body keeps every term."""
    n, cutoff = 65536, 1e8
    b, m, twins = _twins(n, dtype, cutoff)
    ref, absref = sp.reference(b, m, dtype, cutoff=cutoff)
    full, _ = sp.reference(b, m, dtype)
    for i, mk, d in twins:  # the excluded term dominated the twin's sum
        assert np.abs(full[i] - ref[i]).max() > 100 * np.abs(ref[i]).max(), (i, mk, d)
    e = _engine(n, dtype, mode="sym", cutoff=cutoff, cutoff_mode="exact")
    try:
        _assert_geometry(e, n)
        e.load(b)
        assert e.force_mode()["exact"]
        got = e.accel(step_path=True)[:n, :3]
    finally:
        e.close()
    worst = sp.assert_probe_gate(got, ref, absref, m, b, dtype, cutoff=cutoff,
                                 label=f"cutoff n {n} {dtype}")
    tw = [round(float(sp.gate_ratio(got[i], ref[i], absref[i], dtype).max()), 2)
          for i, _, _ in twins]
    print(f"cutoff probe n {n} {dtype} K {len(m)}: worst ratio {worst:.2f}, twins "
          f"(d = 0, 1, NC/2 - 1, NC/2) {tw}")


@pytest.mark.parametrize("n,dtype", [(65536, "fp32"), (131072, "fp32"), (262144, "fp32"),
                                     (524288, "fp32"), (65536, "fp64"), (262144, "fp64")])
def test_sym_step_is_kick_drift_of_the_step_path_accel(hip, n, dtype):
    """One step against the step-path acceleration a of the same state, for every body and
    component: v1 = fl(v0 + fl(a dt)) and x1 = fl(x0 + fl(v1 dt)) to two roundings each (the
    bound holds with or without a contracted multiply-add), in fp64 from the values as the
    dtype holds them; mass comes back unchanged. 65536 to 262144 run the fused tail
    (sym_tail_kernel), 524288 the three-kernel tail (sym_finalize_kernel)."""
    b, m, ref, absref = sp.probe_case(n, dtype)
    dt = 3600.0
    e = _engine(n, dtype, mode="sym", dt=dt)
    try:
        _assert_geometry(e, n)
        e.load(b)
        a = e.accel(step_path=True)[:n, :3]
        e.step(1)
        e.sync()
        st = e.state()
        assert e.nonfinite() == 0
    finally:
        e.close()
    sp.assert_probe_gate(a, ref, absref, m, b, dtype, label=f"step n {n} {dtype}")
    x0, v0, _ = sp.seen(b, dtype)
    eps = sp.EPS[dtype]
    kick = a * dt
    rv = np.abs(st.vel - (v0 + kick)) / (2.0 * eps * (np.abs(v0) + np.abs(kick)) + 1e-300)
    drift = st.vel * dt
    rx = np.abs(st.pos - (x0 + drift)) / (2.0 * eps * (np.abs(x0) + np.abs(drift)) + 1e-300)
    print(f"step probe n {n} {dtype}: kick {rv.max():.3f}, drift {rx.max():.3f} of the "
          f"two-rounding bound")
    assert rv.max() <= 1.0, f"kick: body {rv.max(1).argmax()} at {rv.max():.3g} x the bound"
    assert rx.max() <= 1.0, f"drift: body {rx.max(1).argmax()} at {rx.max():.3g} x the bound"
    assert np.array_equal(st.mass, b.mass)
