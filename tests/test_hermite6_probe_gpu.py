"""Marker probe of the 6th-order evaluate kernel on the GPU: every body against a reference at the
geometries that only exist at size, and one step of the device chain from a state the test chose
(tests/hermite6_probe_helpers.py).

hermite6_eval_kernel sweeps the j rows chunk by chunk in three LDS tiles at once, (x, mu), (v, 0)
and (ap, 0), and flushes one partial per chunk into PA, PJ and PS; the grid's y extent splits the
chunks into groups; hermite6_reduce_kernel folds up to 64 partials. Its tests against the oracle
(tests/test_hermite6_gpu.py) stop at 4,097 bodies in 3 chunks. Here all bodies but K <= 256
markers are massless and the markers sit in every chunk and tile end, so a lost, doubled or
misrouted partial of any chunk, or a chunk swept with another chunk's acceleration rows, is far
above the gate for every body (tests/test_hermite6_probe_cpu.py asserts that from the reference
alone): all n bodies are gated on a, j, s and phi at |err| <= 128 eps x scale, the snap against
the reference at the acceleration rows its pass read (the first pass's output), and a failure
names chunk, tile, chunk group and i-block (hermite6_probe_helpers.locate).

Cases, with the geometry the engine's layout reported (n_pad, chunk, chunks, ipl, groups: asserted
against gs_hermite_layout and against the shapes derived by hand, hermite6_probe_helpers.AUTO):

    n        chunk        n_pad / chunks  fp32 ipl x groups      fp64 ipl x groups
    20,000   forced 1024  20,480 / 20     1 x 20 (2 would leave  1 x 20
                                          800 < 1024 units)
    40,000   forced 8192  40,960 / 5      1 x 5; 32 tiles        1 x 5; 64 tiles a chunk
                                          a chunk                (both also in 2 groups, 3 + 2)
    66,000   auto 2048    67,584 / 33     2 x 16 of 3, 5 empty   1 x 8 of 5, the last 3, 1 empty
    135,000  auto 4096    135,168 / 33    2 x 8 of 5, last 3,    1 x 4 of 9, the last 6
                                          1 empty
    262,144  auto 4096    262,144 / 64    2 x 4 of 16            -

Worst ratios |got - ref| / (eps x scale) over all bodies on one MI355X, acc / jerk / snap / phi
(the gate is 128 and stays there); every launch shape at 20,000 bodies (fp32: ipl 1, 2 x 1, 3, 7,
20 groups; fp64: ipl 1) and the two-group shape at 40,000 are bitwise the automatic shape, the
former also after two fixed steps in state(), carried() and status():

    n        K    fp32                       fp64
    20,000   158  4.80 / 2.80 / 1.19 / 4.82  5.10 / 2.80 / 3.10 / 5.31
    40,000   256  4.48 / 2.99 / 1.70 / 4.58  4.70 / 3.17 / 3.15 / 4.59
    66,000   256  6.91 / 4.14 / 1.99 / 6.69  6.74 / 4.34 / 3.21 / 6.35
    135,000  256  7.20 / 3.89 / 1.73 / 6.40  6.66 / 4.56 / 2.30 / 6.89
    262,144  256  9.01 / 5.82 / 1.65 / 9.56  -

One step from a supplied state (a1, j1, s1 of carried(): acc / jerk / snap; v1 and x1 in units of
u_T sum |terms|, gate 10; the crackle in units of its bound, one rounding to T; dt_next against
oracle.hermite6_dt, gate 1e-9 relative), fp32 with 1 and 2 bodies a lane bitwise equal:

    n        fp32                                        fp64
    1,000    58.6 / 43.3 / 44.7; 1.67, 0.98; 0.95; 0     8.41 / 11.0 / 12.7; 0, 0; 0; 0
    2,049    89.3 / 75.7 / 75.5; 1.77, 0.99; 1.00; 0     8.78 / 11.2 / 10.5; 0, 0; 0; 1.8e-16
    4,097    84.9 / 71.3 / 71.3; 1.72, 0.98; 1.00; 1e-16 89.1 / 57.7 / 62.0; 0, 0; 0; 0
    20,000   4.49 / 2.71 / 2.53; 1.93, 0.98; 0.99; 0     5.35 / 3.19 / 2.72; 0, 0; 0; 0

(the small sizes are tests/test_hermite6_gpu.py::test_one_step_from_a_supplied_state; in fp64 the
corrector and the crackle are the reference's expression tree in the same type and agree to the
bit). At 20,000 bodies the step asked for is 11.5361 s (fp64: 11.5363 s) under the ceiling of
1024 s, from body 703 in workgroup 2, and from body 19,997 in workgroup 78 of 80 once that body
and body 703 have exchanged rows; at the small sizes it comes from body 0 (0.058 to 0.109 s).

Wall time of a test, load and read-back included, the reference built on the host in it (cached
afterwards): evaluate_every_body 0.18 to 0.92 s up to 66,000 bodies, 1.7 / 1.9 s at 135,000
(fp32 / fp64), 3.1 s at 262,144; the launch shapes 0.09 s (8 shapes) and 0.07 s (4); a supplied
step at 20,000 bodies 0.02 to 0.5 s; these 17 and the 9 supplied-state cases of
tests/test_hermite6_gpu.py together 17 s, the session's start included. No kernel change was
needed.

Control on the device (a scratch build, not part of the suite, run once): with
hermite6_eval_kernel changed not to zero its sums after the flush of chunk 12, the 66,000-body
cases fail at 3.1e6 (fp32) and 1.7e15 (fp64) x eps x scale in a, j, s and phi, and the message
names chunk 12, doubled, chunk group 4 (fp32) and 2 (fp64), for every i-block, all 1024 located
rows fitted; the 22 cases of tests/test_hermite6_gpu.py::test_derivs_match_oracle (up to 4,097
bodies in 3 chunks, one chunk a group) pass on that build.
"""
import functools
import time

import numpy as np
import pytest

from gravsim.config import SimConfig
from gravsim.runtime.hermite import HermiteHipEngine

import hermite6_probe_helpers as h6p
import hermite_probe_helpers as hp

pytestmark = pytest.mark.gpu

DT = 8.0  # [s] fixed step of the two steps every launch shape takes


def _cfg(n, dtype, **kw):
    kw.setdefault("dt", DT)
    return SimConfig(n=n, dtype=dtype, device="gpu", integrator="hermite", hermite_order=6,
                     chunk=hp.CASES[n]["chunk"], **kw).validate()


def _assert_layout(eng, n, dtype, ipl=0, groups=0):
    """The case runs the geometry it was chosen for; returns it as text."""
    want, g, lay = hp.CASES[n], h6p.geometry(n, dtype, ipl, groups), eng.native_layout
    assert (lay["n_pad"], lay["chunk"], lay["n_chunks"]) == \
        (want["n_pad"], g["chunk"], want["n_chunks"])
    assert (lay["ipl"], lay["split_groups"]) == (g["ipl"], g["groups"]), lay
    if not (ipl or groups):
        assert (lay["ipl"], lay["split_groups"]) == h6p.AUTO[n][dtype][:2]
    return (f"n_pad {lay['n_pad']} chunk {lay['chunk']} x {lay['n_chunks']} ({g['tpc']} tiles) "
            f"ipl {lay['ipl']} groups {lay['split_groups']} of {g['per']} "
            f"({g['groups'] - g['used_groups']} empty)")


def _run(n, dtype, steps=0, **kw):
    """derivs() of the probe case under a launch shape, then `steps` fixed steps: (a4, j4, s4,
    geometry text, state after the steps or None)."""
    b = h6p.probe_bodies(n)[0]
    eng = HermiteHipEngine(_cfg(n, dtype, **kw))
    try:
        geo = _assert_layout(eng, n, dtype, kw.get("ipl", 0), kw.get("split_groups", 0))
        eng.load(b)
        out = eng.derivs() + (geo,)
        after = None
        if steps:
            eng.step(steps)
            s, st = eng.state(), eng.status()
            after = (s.pos, s.vel) + tuple(eng.carried()) + (
                np.array([st.time, st.dt_last, st.dt_next, st.dt_min, st.steps]),)
        return out + (after,)
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _auto(n, dtype, steps=0):
    return _run(n, dtype, steps)


def _gate(rows, n, dtype, label, ipl=0, groups=0):
    a4, j4, s4 = rows
    vw, ref = h6p.case_reference(n, dtype, a4[:, :3])
    return h6p.assert_gate(a4, j4, s4, vw, ref, h6p.geometry(n, dtype, ipl, groups), label=label)


# ---- a. every body at every case ---------------------------------------------------------------
@pytest.mark.parametrize("n,dtype", h6p.PROBE)
def test_evaluate_every_body(hip, n, dtype):
    t0 = time.perf_counter()
    a4, j4, s4, geo, _ = _auto(n, dtype)
    w = _gate((a4, j4, s4), n, dtype, f"derivs n {n} {dtype}")
    print(f"probe6 n {n} {dtype} [{geo}]: {h6p.fmt(w)} ({time.perf_counter() - t0:.2f} s)")
    if n == 40000:  # two groups of 3 and 2 long chunks: a flush inside a group's sweep
        a2, j2, s2, _, _ = _run(n, dtype, split_groups=2)
        assert np.array_equal(a2, a4) and np.array_equal(j2, j4) and np.array_equal(s2, s4)


@pytest.mark.parametrize("dtype", h6p.DTYPES)
def test_every_launch_shape_at_20000(hip, dtype):
    """Every built ipl x 1, 3, 7, 20 chunk groups (20, 7, 3, 1 chunks a group; 7 groups leave the
    last one short): each at the gate, bitwise the auto shape, and bitwise the auto shape after
    two fixed steps in state(), the four rows of carried() and status()."""
    n = 20000
    ref = _auto(n, dtype, 2)
    assert len(ref[4]) == 7 and ref[4][6][4] == 2
    assert (ref[4][0] != h6p.probe_bodies(n)[0].pos).any()
    t0 = time.perf_counter()
    for ipl in h6p.IPLS[dtype]:
        for groups in (1, 3, 7, 20):
            got = _run(n, dtype, 2, ipl=ipl, split_groups=groups)
            w = _gate(got[:3], n, dtype, f"n {n} {dtype} ipl {ipl} groups {groups}", ipl, groups)
            for x, y in zip(got[:3] + got[4], ref[:3] + ref[4]):
                assert np.array_equal(x, y), (ipl, groups)
    print(f"shapes6 n {n} {dtype}: {len(h6p.IPLS[dtype]) * 4} shapes, {h6p.fmt(w)} "
          f"({time.perf_counter() - t0:.2f} s)")


# ---- b. one step from a supplied state at 20,000 bodies ----------------------------------------
@pytest.mark.parametrize("top", [False, True])
@pytest.mark.parametrize("dtype,ipl", [("fp32", 1), ("fp32", 2), ("fp64", 1)])
def test_one_step_from_a_supplied_state_at_20000(hip, dtype, ipl, top):
    """h6p.check_supplied_step (the gated launch, the HM_STEP reduce, the predict kernel's AP, the
    corrector, the crackle and the step criterion) in 20 chunks and 80 workgroups; top: the body
    that asks for the smallest step stands in row 19,997 (h6p.supplied_state), so the minimum
    comes from workgroup 78, the last with real rows: the fold over wgmin."""
    n = 20000
    top_row = n - 3 if top else -1
    t0 = time.perf_counter()
    h6p.supplied_case(n, dtype, top_row)
    t1 = time.perf_counter()
    eng = HermiteHipEngine(_cfg(n, dtype, dt=h6p.STEP_H, eta=h6p.STEP_ETA, ipl=ipl))
    try:
        assert eng.native_layout["ipl"] == ipl and eng.native_layout["n_chunks"] == 20
        out = h6p.check_supplied_step(eng, n, dtype, top_row, h6p.geometry(n, dtype, ipl),
                                      label=f"step n {n} {dtype} ipl {ipl}")
    finally:
        eng.close()
    if top:
        assert out["wg"] == (n - 1) // h6p.WG == 78
    print(f"step6 n {n} {dtype} ipl {ipl}: {h6p.fmt(out['worst'])}; v1 {out['v']:.2f} x1 "
          f"{out['x']:.2f} of {h6p.CORRECT_ROUNDINGS} u sum |terms|; crackle {out['crackle']:.2f} "
          f"of its bound; dt_next {out['dt_next']:.6g} ({out['dt_rel']:.1e} relative) from body "
          f"{out['row']} in workgroup {out['wg']} (reference {t1 - t0:.2f} s, step and checks "
          f"{time.perf_counter() - t1:.2f} s)")
