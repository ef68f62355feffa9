"""Marker probe of the 6th-order evaluate kernel and one step from a supplied state
(tests/test_hermite6_probe_cpu.py, tests/test_hermite6_probe_gpu.py and section 7 of
tests/test_hermite6_gpu.py). NumPy only; the bodies, the markers, the compensated sum and the
unit fit are those of tests/hermite_probe_helpers.py.

hermite6_eval_kernel (csrc/hip/nbody_hermite6.hip) sweeps three LDS tiles a j-tile, (x, mu),
(v, 0) and (ap, 0), flushes one partial per chunk into PA, PJ and PS, and hermite6_reduce_kernel
folds them. All bodies but K <= 256 markers are massless, so a, j, s and phi of every body are
sums of K terms and the reference costs O(K n) at any size. The snap term also reads an
acceleration row of the j body and one of the i body, q = acc_in_j - acc_in_i: the reference takes
those rows as an argument, so a test can hand it the rows the kernel read, or rows of its own.

Launch shape of order 6 (launch_shape of csrc/hip/hermite.hip): at most 2 bodies per lane in fp32
and 1 in fp64, the automatic choice going down to 1 where 2 leave fewer than 1024
workgroup-chunks; groups = ceil(2048 / i-blocks), at most one per chunk. By hand, for AUTO below:

    n        n_pad    chunks  fp32: blocks at ipl 2 x chunks -> ipl, groups      fp64 (ipl 1)
    20,000   20,480   20      40 x 20 = 800 < 1024 -> 1; 2127 // 80 = 26 -> 20   the same
    40,000   40,960   5       80 x 5 = 400 < 1024 -> 1; 2207 // 160 = 13 -> 5    the same
    66,000   67,584   33      132 x 33 -> 2; 2179 // 132 = 16 groups of 3,       2311 // 264 = 8
                              11 used, 5 empty                                   of 5, 7 used
    135,000  135,168  33      264 x 33 -> 2; 2311 // 264 = 8 of 5, 7 used,       2575 // 528 = 4
                              the last with 3                                    of 9, the last 6
    262,144  262,144  64      512 x 64 -> 2; 2559 // 512 = 4 of 16               -

One step from a supplied state: see supplied_state().
"""
from __future__ import annotations

import hashlib
from functools import lru_cache

import numpy as np

from gravsim.config import G_SI
from gravsim.models import initial_conditions as ic
from gravsim.models.initial_conditions import BodySet
from gravsim.ops import oracle

import hermite_probe_helpers as hp

WG, GATE, EPS, CUTOFF = hp.WG, hp.GATE, hp.EPS, hp.CUTOFF
DTYPES = ("fp32", "fp64")
NP_T = {"fp32": np.float32, "fp64": np.float64}
# n -> dtype -> (ipl, groups, chunks a group, empty groups) of the automatic launch shape, by hand
# from launch_shape of csrc/hip/hermite.hip (module docstring); chunk, n_pad and n_chunks are
# hp.CASES[n]'s.
AUTO = {
    20000: {"fp32": (1, 20, 1, 0), "fp64": (1, 20, 1, 0)},
    40000: {"fp32": (1, 5, 1, 0), "fp64": (1, 5, 1, 0)},
    66000: {"fp32": (2, 16, 3, 5), "fp64": (1, 8, 5, 1)},
    135000: {"fp32": (2, 8, 5, 1), "fp64": (1, 4, 9, 0)},
    262144: {"fp32": (2, 4, 16, 0)},
}
PROBE = [(n, dt) for n in AUTO for dt in DTYPES if dt in AUTO[n]]
IPLS = {"fp32": (1, 2), "fp64": (1,)}   # the forms that are built (hermite6_ipl_ok)
COLS = ("ax", "ay", "az", "jx", "jy", "jz", "sx", "sy", "sz", "phi")
# The velocities about the common drift are an eighth of hp.probe_bodies' (1.25 km/s a
# component). The snap term is s (q - 6 alpha u - 3 beta d) with beta d ~ |w|^2 / r. Measured at
# 20,000 bodies in fp32 with hp.probe_bodies' 10 km/s: the q part, the only one that reads the
# acceleration rows, is 0.16 % of the snap's scale (median over the bodies), 5.5e-3 of the single
# terms are under twice the gate, a (body, chunk) pair hides a chunk of wrong acceleration rows in
# 7e-4 of the cases, and the smallest move when q is dropped is 15 x the gate. At a fifth of the
# speed the single-term share is still 1.1e-3 to 1.7e-3; at an eighth it is 4e-5 to 2.7e-4 over
# the five cases, no pair hides a chunk, and dropping q moves every body by more than 499 x the
# gate (tests/test_hermite6_probe_cpu.py asserts the caps). The other parts of the term stay the
# larger share of the scale (at a tenth of the speed the q part is 7 to 9 % of it). Jerk terms and
# their scale are linear in w, so what the gate sees of the jerk does not change.
VEL_SPREAD = 0.125


# ---- geometry ---------------------------------------------------------------------------------
def launch_shape(n_loc: int, n_chunks: int, dtype: str, ipl: int = 0, groups: int = 0) -> tuple:
    """(ipl, chunk groups) of the order-6 evaluate launch (launch_shape, order == 6)."""
    top, low, want = (1 if dtype == "fp64" else 2), 1, 1024
    if ipl == 0:
        ipl = top
        while ipl > low and n_loc // (WG * ipl) * n_chunks < want:
            ipl >>= 1
    ipl = min(ipl, top)
    blocks = n_loc // (WG * ipl)
    g = groups if groups > 0 else (2 * want + blocks - 1) // blocks
    return ipl, max(1, min(g, n_chunks))


def geometry(n: int, dtype: str, ipl: int = 0, groups: int = 0) -> dict:
    """hp.geometry of case n under the order-6 launch shape."""
    g = hp.geometry(n, dtype)
    ipl, groups = launch_shape(g["n_pad"], g["n_chunks"], dtype, ipl, groups)
    per = -(-g["n_chunks"] // groups)
    g.update(ipl=ipl, groups=groups, per=per, used_groups=-(-g["n_chunks"] // per),
             short_last=g["n_chunks"] % per, iblock=WG * ipl)
    return g


# ---- the reference ----------------------------------------------------------------------------
def quantize(x, dtype: str) -> np.ndarray:
    return np.asarray(x, dtype=np.float64).astype(NP_T[dtype]).astype(np.float64)


def pair_terms6(pi, vi, ai, pm, vm, am, mum, with_abs: bool = False):
    """fp64 terms of K sources on b bodies by oracle.acc_jerk_snap's own expressions: a, jerk and
    snap terms (b, K, 3) and phi terms (b, K), zero for r^2 < CUTOFF^2 (the self pair); with_abs:
    the three scale terms (b, K, 3) after them."""
    d = pm[None, :, :] - pi[:, None, :]
    w = vm[None, :, :] - vi[:, None, :]
    q = am[None, :, :] - ai[:, None, :]
    r2 = (d * d).sum(-1)
    ok = r2 >= CUTOFF * CUTOFF
    inv = np.zeros_like(r2)
    np.divide(1.0, np.sqrt(r2, where=ok, out=np.ones_like(r2)), where=ok, out=inv)
    inv2 = inv * inv
    mi = mum[None, :] * inv
    s = (mi * inv2)[:, :, None]
    al = ((d * w).sum(-1) * inv2)[:, :, None]
    be = (((w * w).sum(-1) + (d * q).sum(-1)) * inv2)[:, :, None] + al * al
    A = s * d
    Jt = s * w - 3.0 * al * A
    out = (A, Jt, s * q - 6.0 * al * Jt - 3.0 * be * A, -mi)
    if with_abs:
        ad, aw = np.abs(d), np.abs(w)
        aal = (np.abs(d * w).sum(-1) * inv2)[:, :, None]
        abe = (((w * w).sum(-1) + np.abs(d * q).sum(-1)) * inv2)[:, :, None] + aal * aal
        out += (s * ad, s * (aw + 3.0 * aal * ad),
                s * (np.abs(q) + 6.0 * aal * (aw + 3.0 * aal * ad) + 3.0 * abe * ad))
    return out


def _geom(pi, pm, mum):
    """d (b, K, 3), 1 / r^2 (b, K) and s = mu / r^3 (b, K, 1), zero under the cutoff."""
    d = pm[None, :, :] - pi[:, None, :]
    r2 = (d * d).sum(-1)
    ok = r2 >= CUTOFF * CUTOFF
    inv = np.zeros_like(r2)
    np.divide(1.0, np.sqrt(r2, where=ok, out=np.ones_like(r2)), where=ok, out=inv)
    inv2 = inv * inv
    return d, inv2, (mum[None, :] * inv * inv2)[:, :, None]


def snap_of_acc_rows(pi, pm, mum, dq, geom=None):
    """(b, K, 3): what marker k adds to the snap of a body when q changes by dq ((K, 3): the
    marker's acceleration row reads am + dq[k]; or (b, K, 3)): the snap term is linear in q,
    dS = s (dq - 3 (d.dq) d / r^2)."""
    d, inv2, s = _geom(pi, pm, mum) if geom is None else geom
    dq = dq[None, :, :] if dq.ndim == 2 else dq
    return s * (dq - 3.0 * ((d * dq).sum(-1) * inv2)[:, :, None] * d)


class View:
    """The rows as the kernel of `dtype` sees them, in fp64: positions, velocities, the
    acceleration rows the snap is taken at, mu = G m; the sorted marker rows."""

    def __init__(self, p, v, acc, mu, markers, dtype: str):
        self.p, self.v, self.mu, self.dtype = p, v, mu, dtype
        self.acc = quantize(acc, dtype)
        self.m = np.asarray(markers, dtype=np.int64)
        self.n = len(p)
        rest = np.ones(self.n, dtype=bool)
        rest[self.m] = False
        assert not mu[rest].any(), "a body outside the markers has mass"

    def terms(self, r, with_abs: bool = False, acc_m=None):
        """pair_terms6 of the markers on the bodies r; acc_m: other acceleration rows of the
        markers than their own (what a wrong `ta` tile would hold)."""
        m = self.m
        return pair_terms6(self.p[r], self.v[r], self.acc[r], self.p[m], self.v[m],
                           self.acc[m] if acc_m is None else acc_m, self.mu[m], with_abs)

    def rows10(self, r, acc_m=None):
        """(len(r), K, 10) terms in the order of COLS."""
        ta, tj, ts, tp = self.terms(r, acc_m=acc_m)
        return np.concatenate([ta, tj, ts, tp[:, :, None]], 2)


def view(b: BodySet, markers, dtype: str, acc_in) -> View:
    p, v, mu = hp.seen(b, dtype)
    return View(p, v, acc_in, mu, markers, dtype)


def reference(vw: View, block: int = 2048) -> tuple:
    """(acc, jerk, snap (n, 3), phi (n,), acc scale, jerk scale, snap scale (n, 3)) of the K marker
    columns on all n bodies: the sums and scales of oracle.acc_jerk_snap(with_abs=True), whose
    massless columns add exact zeros. fp64: the sums with two-sum compensation
    (hp.two_sum_reduce), since a plain sum of 256 terms could use up a good part of 128 eps."""
    n = vw.n
    out = [np.zeros((n, 3)) for _ in range(3)] + [np.zeros(n)]
    out += [np.zeros((n, 3)) for _ in range(3)]

    def rows(i0):
        sl = slice(i0, min(n, i0 + block))
        t = vw.terms(sl, with_abs=True)
        if vw.dtype == "fp64":
            s = hp.two_sum_reduce(np.concatenate(t[:3] + (t[3][:, :, None],), 2))
            sums = (s[:, :3], s[:, 3:6], s[:, 6:9], s[:, 9])
        else:
            sums = tuple(x.sum(1) for x in t[:4])
        for o, x in zip(out, sums + tuple(x.sum(1) for x in t[4:])):
            o[sl] = x

    hp._threads(rows, n, block)
    for o in out:
        o.setflags(write=False)
    return tuple(out)


@lru_cache(maxsize=None)
def probe_bodies(n: int):
    """(bodies, markers) of hp.probe_bodies for case n, read-only, the coverage asserted in
    integers for both tile widths (it depends on chunks, tiles and slices, not on the order)."""
    b, m = hp.probe_bodies(n)
    b = BodySet(b.pos, hp.DRIFT + VEL_SPREAD * (b.vel - hp.DRIFT), b.mass, b.radius)
    for dtype in DTYPES:
        hp.assert_coverage(n, dtype, m)
    for a in (b.pos, b.vel, b.mass, b.radius):
        a.setflags(write=False)
    return b, m


_CASE_REF: dict = {}


def case_reference(n: int, dtype: str, acc_in) -> tuple:
    """(view, reference) of case n at the acceleration rows acc_in (n, 3); the latest per
    (n, dtype) is kept, keyed by the bytes of acc_in: every launch shape returns the same bits,
    so a case computes it once."""
    acc = np.ascontiguousarray(acc_in, dtype=np.float64)
    key = hashlib.sha1(acc.tobytes()).hexdigest()
    hit = _CASE_REF.get((n, dtype))
    if hit is None or hit[0] != key:
        b, m = probe_bodies(n)
        vw = view(b, m, dtype, acc)
        hit = _CASE_REF[(n, dtype)] = (key, vw, reference(vw))
    return hit[1], hit[2]


@lru_cache(maxsize=None)
def cpu_case(n: int, dtype: str):
    """(view, reference) of case n with acc_in the reference acceleration rounded to the dtype:
    what the conditions that need no engine are stated on."""
    b, m = probe_bodies(n)
    p, _, mu = hp.seen(b, dtype)
    acc = np.zeros((n, 3))

    def rows(i0):
        d, _, s = _geom(p[i0:i0 + 4096], p[m], mu[m])
        acc[i0:i0 + 4096] = (s * d).sum(1)

    hp._threads(rows, n, 4096)
    return case_reference(n, dtype, quantize(acc, dtype))


# ---- the gate ---------------------------------------------------------------------------------
def columns(ref, r=slice(None), dtype: str = "fp64"):
    """(reference, eps x scale) (rows, 10) in the order of COLS."""
    ra, rj, rs, rphi, sa, sj, ss = (x[r] for x in ref)
    return (np.concatenate([ra, rj, rs, rphi[:, None]], 1),
            EPS[dtype] * np.concatenate([sa, sj, ss, np.abs(rphi)[:, None]], 1) + 1e-300)


def got10(a4, j4, s4):
    return np.concatenate([a4[:, :3], j4[:, :3], s4[:, :3], a4[:, 3:4]], 1)


def ratios(a4, j4, s4, ref, dtype: str, rows=None) -> np.ndarray:
    """|got - ref| / (eps scale) per row and column of COLS."""
    want, bound = columns(ref, slice(None) if rows is None else np.asarray(rows), dtype)
    return np.abs(got10(a4, j4, s4) - want) / bound


def worst4(r) -> tuple:
    return (float(r[:, :3].max()), float(r[:, 3:6].max()), float(r[:, 6:9].max()),
            float(r[:, 9].max()))


def fmt(w) -> str:
    return f"acc {w[0]:.2f} jerk {w[1]:.2f} snap {w[2]:.2f} phi {w[3]:.2f}"


def assert_gate(a4, j4, s4, vw: View, ref, g: dict, label: str = "", phi: bool = True) -> tuple:
    """All rows at the gate for a, j, s (and phi); a failure names what the error corresponds to
    (locate). Returns the worst ratios (acc, jerk, snap, phi)."""
    r = ratios(a4, j4, s4, ref, vw.dtype)
    if not phi:
        r[:, 9] = 0.0
    w = worst4(r)
    finite = all(np.isfinite(x).all() for x in (a4, j4, s4))
    if not max(w) <= GATE or not finite:
        found = [{k: v if k not in ("iblocks", "where") or len(v) <= 8 else
                  f"{len(v)} from {v[0]} to {v[-1]}" for k, v in e.items()}
                 for e in locate(a4, j4, s4, vw, ref, g, phi=phi)]
        raise AssertionError(f"{label}: {fmt(w)} x eps x scale (gate {GATE:g}); {found}")
    assert not j4[:, 3].any() and not s4[:, 3].any()
    return w


def locate(a4, j4, s4, vw: View, ref, g: dict, phi: bool = True, worst: int = 4,
           limit: int = 1024) -> list:
    """hp.locate_units on the ten columns: a missing or doubled marker, tile or chunk. Where that
    fits fewer than half of the failing rows and a, j and phi of those rows are at the gate, the
    error is in the snap alone, and the fit of acc_rows_unit() is put first."""
    got = got10(a4, j4, s4)
    if not phi:
        got[:, 9] = ref[3]
    found = hp.locate_units(got, lambda r: columns(ref, r, vw.dtype), vw.rows10, vw.m, g, vw.n,
                            worst=worst, limit=limit)
    fitted, rows = sum(e["fitted"] for e in found), sum(e["rows"] for e in found)
    if found and 2 * fitted < rows:
        e = acc_rows_unit(got, vw, ref, g, limit)
        if e is not None:
            found.insert(0, e)
    return found


def acc_rows_unit(got, vw: View, ref, g: dict, limit: int = 1024):
    """A snap-only residual as other acceleration rows in one tile or chunk of j bodies: for every
    tile and chunk with markers, the least-squares change dm of its markers' acceleration rows
    (3 unknowns a marker; the snap is linear in them, snap_of_acc_rows) over the `limit` worst
    rows; the smallest unit whose fit brings the most rows back to the gate, as a dict like
    hp.locate_units' with kind "acc rows"."""
    want, bound = columns(ref, slice(None), vw.dtype)
    r = np.abs(got - want) / bound
    r = np.where(np.isfinite(r), r, np.inf)
    bad = np.nonzero(~(r.max(1) <= GATE))[0]
    if not len(bad) or not (np.delete(r[bad], (6, 7, 8), 1) <= GATE).all():
        return None
    bad = bad[np.argsort(-r[bad].max(1), kind="stable")][:limit]
    res = ((got - want)[bad, 6:9] / bound[bad, 6:9]).reshape(-1)          # (3 b) in gate units
    m, best = vw.m, None
    eye = np.eye(3)
    for kind, width in (("tile", g["tile"]), ("chunk", g["chunk"])):
        for u in np.unique(m // width):
            ks = np.nonzero(m // width == u)[0]
            # design matrix: unit change of component e of marker k -> the snap of every row
            D = np.stack([snap_of_acc_rows(vw.p[bad], vw.p[m[ks]], vw.mu[m[ks]],
                                           np.broadcast_to(eye[e], (len(ks), 3)))
                          for e in range(3)], -1)                         # (b, k, 3 out, 3 e)
            D = (D / bound[bad, None, 6:9, None]).transpose(0, 2, 1, 3).reshape(3 * len(bad), -1)
            dm, *_ = np.linalg.lstsq(D, res, rcond=None)
            left = np.abs(res - D @ dm).reshape(len(bad), 3).max(1)
            n_fit = int((left <= GATE).sum())
            if best is None or n_fit > best[0]:
                best = (n_fit, kind, int(u), ks, dm.reshape(-1, 3))
    n_fit, kind, u, ks, dm = best
    c = u * (g["tile"] if kind == "tile" else g["chunk"]) // g["chunk"]
    e = dict(kind="acc rows", units=[dict(kind=kind, what="other acceleration rows", chunk=c,
                                          group=c // g["per"], markers=m[ks].tolist())],
             rows=len(bad), fitted=n_fit, ratio=float(r[bad].max()),
             iblocks=sorted({int(i) // g["iblock"] for i in bad}), where=[],
             rows_read_minus_own=np.abs(dm).max())
    if kind == "tile":
        e["units"][0]["tile"] = u % g["tpc"]
    return e


# ---- NumPy emulation of the chunked sum (the mutation controls) -------------------------------
def unit_partials(vw: View, starts, acc_m=None, block: int = 4096) -> np.ndarray:
    """(units, n, 10) fp64: the partial sums (COLS) of every row over the markers of every unit
    of j rows that begins at starts[u]; acc_m: the markers' acceleration rows as the sweep read
    them, where not their own."""
    M = hp._unit_matrix(np.asarray(starts), vw.m)
    out = np.zeros((len(starts), vw.n, 10))

    def part(i0):
        sl = slice(i0, min(vw.n, i0 + block))
        out[:, sl] = np.einsum("uk,bkc->ubc", M, vw.rows10(sl, acc_m), optimize=True)

    hp._threads(part, vw.n, block)
    return out


def fold(partials):
    """The reduce: the partials added in unit order, as (a4, j4, s4)."""
    s = np.zeros(partials.shape[1:])
    for u in range(partials.shape[0]):
        s = s + partials[u]
    z = np.zeros((len(s), 1))
    return (np.concatenate([s[:, :3], s[:, 9:10]], 1), np.concatenate([s[:, 3:6], z], 1),
            np.concatenate([s[:, 6:9], z], 1))


# ---- what the gate can see of the snap --------------------------------------------------------
def snap_visibility(vw: View, ref, g: dict, block: int = 2048) -> dict:
    """From the reference alone:
    term: share of the (body, marker) snap terms, the K zero self terms included, with
        |term| < 2 x 128 eps |scale vector|;
    chunk: share of the (body, chunk) pairs whose whole snap partial is within 128 eps scale in
        every component (a dropped or doubled chunk that the gate would not see);
    acc_rows: the same for what a chunk's partial changes by when its markers' acceleration rows
        read as zero (a chunk whose `ta` tile alone is wrong);
    q_move: over all bodies, the smallest move of the reference snap when the whole q part is
        dropped (acc_in = 0), largest component, in units of the gate 128 eps scale."""
    n, m, eps = vw.n, vw.m, EPS[vw.dtype]
    ss = ref[6]
    chunks = np.arange(-(-n // g["chunk"])) * g["chunk"]
    M = hp._unit_matrix(chunks, m)
    assert M.any(1).all()
    move = np.zeros(n)

    def rows(i0):
        sl = slice(i0, min(n, i0 + block))
        geom = d, inv2, s3 = _geom(vw.p[sl], vw.p[m], vw.mu[m])
        q = vw.acc[m][None, :, :] - vw.acc[sl][:, None, :]
        w = vw.v[m][None, :, :] - vw.v[sl][:, None, :]
        al = ((d * w).sum(-1) * inv2)[:, :, None]
        be = (((w * w).sum(-1) + (d * q).sum(-1)) * inv2)[:, :, None] + al * al
        ts = s3 * (q - 6.0 * al * (w - 3.0 * al * d) - 3.0 * be * d)  # (pair_terms6's snap term)
        lim = GATE * eps * ss[sl]
        term = int((np.linalg.norm(ts, axis=-1) <
                    2.0 * GATE * eps * np.linalg.norm(ss[sl], axis=-1)[:, None]).sum())
        part = np.einsum("ck,bkx->bcx", M, ts, optimize=True)
        chunk = int((np.abs(part) <= lim[:, None, :]).all(-1).sum())
        dacc = np.einsum("ck,bkx->bcx", M,
                         snap_of_acc_rows(None, None, None, -vw.acc[m], geom), optimize=True)
        acc_rows = int((np.abs(dacc) <= lim[:, None, :]).all(-1).sum())
        move[sl] = (np.abs(snap_of_acc_rows(None, None, None, q, geom).sum(1)) / lim).max(1)
        return term, chunk, acc_rows

    tot = np.array(hp._threads(rows, n, block)).sum(0)
    return {"term": tot[0] / (n * len(m)), "chunk": tot[1] / (n * len(chunks)),
            "acc_rows": tot[2] / (n * len(chunks)), "q_move": float(move.min())}


# ---- one step from a supplied state -----------------------------------------------------------
STEP_H = 1024.0          # [s] the step: a power of two, so h / 2 and h^2 / 2 are exact
STEP_ETA = 0.25
STEP_SIZES = (1000, 2049, 4097)
A0_MAX = 0.5             # [m/s^2] largest |component| of A0


def supplied_state(n: int, dtype: str, top_row: int = -1) -> dict:
    """The state one step is taken from, and its prediction to the bit.

    x0: solar_random positions (n = 20,000: the probe case's), v0 = 0, a0 = A0 with components
    uniform in +-A0_MAX, j0 = s0 =
    c0 = 0, h = STEP_H. Reading h6_taylor and h6_predict (gs_hermite_scheme.h) with these rows in
    the state type T: t.h2 = (h h) / 2 = 2^19 exactly; every product with a zero row is zero and
    every sum with it exact, under any contraction; a t.h2 is exact (a power of two); so
        xp = fl_T(x + a h^2 / 2)  (one rounding),  vp = a h  (exact),  ap = a,
    which NumPy reproduces in T. The shift |a| h^2 / 2 is at most sqrt(3) x 0.5 x 2^19 = 4.6e5 m
    < UNIT / 4, so in the probe case no distance of a massless body to a marker leaves
    0.7 U .. 5.3 U (supplied_case asserts it, and that no two markers come within U / 20).

    top_row: the massless body that asks for the smallest next step in the plain case (from the
    reference rows) and the massless body top_row exchange their rows of x0 and A0, so the
    minimum over the bodies comes from row top_row. (A larger A0 does not move the minimum there:
    with components of 0.001 to 1.3 m/s^2, the most the shift allows, that body asks for 12.1 to
    14.6 s against the 11.5 s of the smallest, since a1, j1 and s1 weigh as much as a1 - a0.)"""
    T = NP_T[dtype]
    if n == 20000:
        b, markers = probe_bodies(n)
    else:
        b, markers = ic.solar_random(n, seed=7 + n), None
    rng = np.random.default_rng(6 * n + 1)
    A0 = rng.uniform(-A0_MAX, A0_MAX, (n, 3))
    pos = b.pos.copy()
    if top_row >= 0:
        base, _, ref = supplied_case(n, dtype)
        low = int(body_dts(base, ref[0], ref[1], ref[2]).argmin())
        assert b.mass[low] == 0 and b.mass[top_row] == 0 and low != top_row
        for y in (pos, A0):
            y[[low, top_row]] = y[[top_row, low]]
    assert np.sqrt((A0 ** 2).sum(1)).max() * STEP_H ** 2 / 2 < hp.UNIT / 4
    x0, a0 = pos.astype(T), A0.astype(T)
    mu = (G_SI * b.mass).astype(T).astype(np.float64)
    xp = (x0 + a0 * T(STEP_H * STEP_H / 2)).astype(np.float64)
    vp = (a0 * T(STEP_H)).astype(np.float64)
    ap = a0.astype(np.float64)
    z = np.zeros((n, 3))
    return dict(n=n, dtype=dtype, markers=markers, x0=x0.astype(np.float64), a0=ap, xp=xp, vp=vp,
                ap=ap, mu=mu, h=STEP_H, top_row=top_row,
                bodies=BodySet(pos, z.copy(), b.mass.copy()),
                load=dict(acc=A0, jerk=z, snap=z, crackle=z, dt_next=STEP_H))


@lru_cache(maxsize=None)
def supplied_case(n: int, dtype: str, top_row: int = -1):
    """(state, view or None, reference) of supplied_state: the dense oracle.acc_jerk_snap at the
    predicted rows for the small sizes, the marker reference at 20,000 bodies."""
    st = supplied_state(n, dtype, top_row)
    if st["markers"] is None:
        ref = oracle.acc_jerk_snap(st["xp"], st["vp"], st["ap"], st["mu"], G=1.0, cutoff=CUTOFF,
                                   with_potential=True, with_abs=True)
        return st, None, ref
    vw = View(st["xp"], st["vp"], st["ap"], st["mu"], st["markers"], dtype)
    rest = np.setdiff1d(np.arange(n), vw.m)
    d = np.sqrt(((st["xp"][rest[::7], None, :] - st["xp"][vw.m][None, :, :]) ** 2).sum(-1))
    assert d.min() > 0.7 * hp.UNIT and d.max() < 5.3 * hp.UNIT
    d = np.sqrt(((st["xp"][vw.m, None, :] - st["xp"][vw.m][None, :, :]) ** 2).sum(-1))
    assert d[d > 0].min() > 0.05 * hp.UNIT  # (marker to marker)
    return st, vw, reference(vw)


def correct_reference(st: dict, v1_T, a1, j1, s1):
    """h6_correct in fp64 on the kernel's own T-valued rows, the same expression tree, with the
    kernel's own v1 in x1: (v1, x1, sum |terms| of v1, of x1)."""
    h, x0, a0 = st["h"], st["x0"], st["a0"]
    z = np.zeros_like(a0)
    hh, h10, h120 = h / 2, (h * h) / 10, (h * h * h) / 120
    v1 = z + ((a0 + a1) * hh + ((z - j1) * h10 + (z + s1) * h120))
    x1 = x0 + ((z + v1_T) * hh + ((a0 - a1) * h10 + (z + j1) * h120))
    sv = (np.abs(a0) + np.abs(a1)) * hh + np.abs(j1) * h10 + np.abs(s1) * h120
    sx = np.abs(x0) + np.abs(v1_T) * hh + (np.abs(a0) + np.abs(a1)) * h10 + np.abs(j1) * h120
    return v1, x1, sv, sx


# Roundings of h6_correct as written, per output, h a power of two (h / 2 exact):
# h10 = (h h) / 10 and h120 = (h h h) / 120: one each (the products of powers of two are exact);
# (a0 + a1) hh: 1 (the sum); (j0 - j1) h10: difference, h10, product = 3; (s0 + s1) h120: 3;
# the three sums that join them and the state: 3. Ten in all, each of a value that is at most
# sum |terms|, so to first order |err| <= 10 u_T sum |terms|; the second-order part 45 u^2 and the
# fp64 evaluation of the reference (10 u_64) are below 1e-6 of that in fp32, and in fp64 the
# reference is the same expression tree in the same type (the libraries are built with
# -ffp-contract=off), so it differs by nothing. x1 has the same form in (v + v1), (a0 - a1),
# (j0 + j1).
CORRECT_ROUNDINGS = 10
# fp64 roundings of h6_high's c1 (h a power of two: hp, hp^2, 1 / hp and its powers, 6 ih3, 24 ih4
# and 120 ih5 are exact, as are / 8, / 16, / 2 and the products with hp and hp^2):
# a3: Am, Jp, Sm (the sum or difference in each) 3, 5 Am and 5 Jp 2, two sums 2, the product 1: 8;
# a4: Jm, Sp 2, the sum 1, the product 1: 4; a5: 3 + 2 + 2 + 1 = 8; c1 = a3 + hp a4 + hp^2 a5 / 2:
# 2 sums. 22 in all.
HIGH_ROUNDINGS = 22


def crackle_reference(st: dict, a1, j1, s1):
    """(c1 of oracle.hermite6_high, sum |terms| of c1) on the rows of the step."""
    z = np.zeros_like(a1)
    c1 = oracle.hermite6_high(st["a0"], z, z, a1, j1, s1, st["h"])[0]
    hp_ = 0.5 * st["h"]
    hp2, ih = hp_ * hp_, 1.0 / hp_
    A, J, S = np.abs(a1) + np.abs(st["a0"]), hp_ * np.abs(j1), hp2 * np.abs(s1)
    tot = (6.0 * ih ** 3 / 8.0) * (5.0 * A + 5.0 * J + S) \
        + hp_ * (24.0 * ih ** 4 / 16.0) * (J + S) \
        + (hp2 / 2.0) * (120.0 * ih ** 5 / 16.0) * (3.0 * A + 3.0 * J + S)
    return c1, tot


def body_dts(st: dict, a1, j1, s1, eta: float = STEP_ETA) -> np.ndarray:
    """The step every body asks for after the step (the expression of oracle.hermite6_dt, per
    body; inf where the ratio is zero or not finite)."""
    z = np.zeros_like(a1)
    c1, p1, a5 = oracle.hermite6_high(st["a0"], z, z, a1, j1, s1, st["h"])
    nrm = lambda y: np.sqrt((y * y).sum(1))  # noqa: E731
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = (nrm(a1) * nrm(s1) + nrm(j1) ** 2) / (nrm(c1) * nrm(a5) + nrm(p1) ** 2)
        dt = eta * ratio ** (1.0 / 6.0)
    return np.where((ratio > 0) & np.isfinite(dt), dt, np.inf)


def check_supplied_step(eng, n: int, dtype: str, top_row: int = -1, g: dict | None = None,
                        label: str = "") -> dict:
    """Load supplied_state into `eng` (order 6, dt = STEP_H, eta = STEP_ETA), take one step and
    gate everything it leaves: a1, j1, s1 at 128 eps scale against the reference at the predicted
    rows; v1 and x1 at CORRECT_ROUNDINGS u_T sum |terms|; the crackle at one rounding to T plus
    HIGH_ROUNDINGS u_64 sum |terms|; dt_next at 1e-9 relative against oracle.hermite6_dt, which
    must be below the ceiling h (the criterion, not the ceiling, is what is compared).
    Returns the figures, the status among them."""
    st, vw, ref = supplied_case(n, dtype, top_row)
    u = EPS[dtype]
    eng.load(st["bodies"], **st["load"])
    eng.step(1)
    a1, j1, s1, c1 = eng.carried()
    s, status = eng.state(), eng.status()
    z1 = np.zeros((n, 1))
    a4, j4, s4 = (np.concatenate([y, z1], 1) for y in (a1, j1, s1))
    if vw is None:
        r = ratios(a4, j4, s4, ref, dtype)
        r[:, 9] = 0.0  # (carried() has no phi)
        w = worst4(r)
        assert max(w) <= GATE, f"{label}: {fmt(w)} x eps x scale (gate {GATE:g})"
    else:
        w = assert_gate(a4, j4, s4, vw, ref, g, label=label, phi=False)
    v1r, x1r, sv, sx = correct_reference(st, s.vel, a1, j1, s1)
    rv = float((np.abs(s.vel - v1r) / (u * sv + 1e-300)).max())
    rx = float((np.abs(s.pos - x1r) / (u * sx + 1e-300)).max())
    assert rv <= CORRECT_ROUNDINGS and rx <= CORRECT_ROUNDINGS, (label, rv, rx)
    cr, ctot = crackle_reference(st, a1, j1, s1)
    rc = float((np.abs(c1 - cr) / (u * np.abs(cr) + HIGH_ROUNDINGS * EPS["fp64"] * ctot
                                   + 1e-300)).max())
    assert rc <= 1.0, (label, rc)
    assert np.abs(c1).min() > 0 and (s.pos != st["x0"]).any(1).all()
    dts = body_dts(st, a1, j1, s1)
    z = np.zeros_like(a1)
    want = oracle.hermite6_dt(st["a0"], z, z, a1, j1, s1, st["h"], STEP_ETA)
    row = int(dts.argmin())
    assert want == dts[row] < st["h"], (want, dts[row], st["h"])
    rdt = abs(status.dt_next - want) / want
    assert rdt <= 1e-9, (label, status.dt_next, want)
    assert (status.time, status.steps, status.dt_last) == (st["h"], 1, st["h"])
    if top_row >= 0:
        assert row == top_row, (row, top_row)
    return dict(worst=w, v=rv, x=rx, crackle=rc, dt_next=status.dt_next, dt_rel=rdt, row=row,
                wg=row // WG, status=status, rows=(s.pos, s.vel, a1, j1, s1, c1))
