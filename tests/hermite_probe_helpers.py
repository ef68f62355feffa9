"""Marker probe of the Hermite evaluate kernels' j coverage at many-chunk geometries
(tests/test_hermite_probe_cpu.py and tests/test_hermite_probe_gpu.py). NumPy only.

All bodies but K <= 256 markers are massless, but every body has a velocity, so every body's
a, j and phi is a sum of K terms, one per marker, and the reference costs O(K n). A marker in
chunk c, tile t reaches a body through every stage of csrc/hip/nbody_hermite.hip that has an
index: the LDS tile of the sweep, the flush of chunk c's partial PA / PJ[c][i] (the chunk group
that owns c, the i-block of the body), the narrow slice, the rank's rows, and the fold of the
partials in the reduce. With K small one lost, doubled or misrouted partial is far above the
rounding gate 128 eps sum |term| for almost every body, so all n bodies are gated at every size.

Bodies: the markers sit on a sphere of radius U (quasi-uniform Fibonacci points, radii 0.97 U to
U), every other body in the shell 2 U .. 4 U around it: all (body, marker) distances lie in
U .. 5 U. The whole configuration is shifted by (1.5e11, 0.7e11, -0.3e11) m; its extent 8 U is
4e7 m, so that what fp32 drops of a position (half an ulp of 16384 m in x) moves a term by
more than ten times the gate: the lo rows of mixed precision carry information on every tile
(hi_only_shift). Each massless body's coordinates sit 0.3 to 0.5 ulp off the fp32 grid for that.

Nearest neighbours: the markers have one radius R = 1.05 x the extent and every other body
radius 0. Then q = r^2 - (R_i + R_j)^2 to a marker is negative and to any other body >= 0, and a
marker's nearest is a marker (r^2 - 4 R^2 < -R^2 since extent^2 < 3 R^2): the nearest neighbour
of every body is its nearest marker, an O(K n) reference (nn_reference asserts the inequality).

Reference times on an 8-core host, per cached case, fp32 and mixed / fp64 (which adds the
two-sum pass): 20,000: 0.2 / 0.8 s; 66,000: 0.6 / 2.3 s; 135,000: 1.2 / 4.6 s; 262,144: 2.4 s.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from functools import lru_cache

import numpy as np

from gravsim.config import G_SI
from gravsim.models.initial_conditions import BodySet
from gravsim.ops import oracle
from gravsim.parallel.partition import HERMITE_UNIT, auto_chunk, hermite_partition, round_up

import hermite_nn_helpers as nnh

WG = 256                 # rows per workgroup (gs_common.h kForceBlock)
TILE = {"fp32": 256, "mixed": 256, "fp64": 128}   # rows per LDS tile (gs_tile.h Tile<T>)
EPS = {"fp32": 2.0 ** -24, "mixed": 2.0 ** -24, "fp64": 2.0 ** -53}
GATE = 128.0             # the project's gate: |got - ref| <= 128 eps scale
MAX_MARKERS = 256
CUTOFF = 1e-10           # SimConfig's default: only the self pair is zeroed
UNIT = 5e6               # [m] radius of the marker sphere
SHIFT = np.array([1.5e11, 0.7e11, -0.3e11])
DRIFT = np.array([0.0, 3e4, 0.0])
R_MARKER = 1.05 * 8 * UNIT
# Offsets within a 256-row tile, cycled over the interior markers: the ends of the fp32 tile, the
# ends of the two fp64 tiles in it, and the wave edges.
OFFSETS = (0, 255, 128, 127, 1, 254, 64, 191, 63, 192)

# n -> forced chunk (0: auto), the geometry expected from reading gs_hermite_create,
# launch_shape and hermite_narrow_slice, and the rank counts of the group tests.
CASES = {
    20000: dict(chunk=1024, n_pad=20480, n_chunks=20, slice=1024, n_slices=20, ranks=(2, 3, 8),
                auto={"fp32": (2, 20), "mixed": (2, 20), "fp64": (1, 20)}),
    40000: dict(chunk=8192, n_pad=40960, n_chunks=5, slice=1024, n_slices=40, ranks=(),
                auto={"fp32": (2, 5), "mixed": (2, 5), "fp64": (1, 5)}),
    66000: dict(chunk=0, n_pad=67584, n_chunks=33, slice=1280, n_slices=53, ranks=(5, 7),
                auto={"fp32": (4, 32), "mixed": (4, 32), "fp64": (2, 16)}),
    67584: dict(chunk=0, n_pad=67584, n_chunks=33, slice=1280, n_slices=53, ranks=(),
                auto={"fp32": (4, 32), "mixed": (4, 32), "fp64": (2, 16)}),
    135000: dict(chunk=0, n_pad=135168, n_chunks=33, slice=2304, n_slices=59, ranks=(),
                 auto={"fp32": (4, 16), "mixed": (4, 16), "fp64": (2, 8)}),
    262144: dict(chunk=0, n_pad=262144, n_chunks=64, slice=4096, n_slices=64, ranks=(),
                 auto={"fp32": (4, 8), "mixed": (4, 8)}),
}
DTYPES = ("fp32", "fp64", "mixed")
PROBE = [(n, dt) for n in CASES for dt in DTYPES if dt in CASES[n]["auto"]]
NN_SIZES = (20000, 66000, 135000)


# ---- geometry (Python mirror of csrc/hip/hermite.hip and nbody_hermite.hip) --------------------
def narrow_slice(n_pad: int) -> int:
    """j rows per narrow slice (hermite_narrow_slice)."""
    return round_up(max(n_pad // 64, 4 * WG), WG)


def launch_shape(n_loc: int, n_chunks: int, dtype: str, ipl: int = 0, groups: int = 0,
                 nn: bool = False) -> tuple:
    """(ipl, chunk groups) of the evaluate launch (launch_shape)."""
    fp64 = dtype == "fp64"
    top = 2 if fp64 or (dtype == "mixed" and nn) else 4
    want = 1024
    if ipl == 0:
        ipl = top
        while ipl > (1 if fp64 else 2) and n_loc // (WG * ipl) * n_chunks < want:
            ipl >>= 1
    ipl = min(ipl, top)
    blocks = n_loc // (WG * ipl)
    g = groups if groups > 0 else (2 * want + blocks - 1) // blocks
    return ipl, max(1, min(g, n_chunks))


def geometry(n: int, dtype: str, ipl: int = 0, groups: int = 0, nn: bool = False) -> dict:
    """The geometry of case n: chunks, tiles, narrow slices and the launch shape."""
    chunk = CASES[n]["chunk"] or auto_chunk(n)
    n_pad = round_up(n, chunk)
    n_chunks = n_pad // chunk
    sl = narrow_slice(n_pad)
    ipl, groups = launch_shape(n_pad, n_chunks, dtype, ipl, groups, nn)
    per = -(-n_chunks // groups)
    return dict(n=n, n_pad=n_pad, chunk=chunk, n_chunks=n_chunks, tile=TILE[dtype],
                tpc=chunk // TILE[dtype], slice=sl, n_slices=-(-n_pad // sl),
                last_slice_real=max(0, n - (-(-n_pad // sl) - 1) * sl), ipl=ipl, groups=groups,
                per=per, used_groups=-(-n_chunks // per), short_last=n_chunks % per,
                iblock=WG * ipl)


def rank_rows(n: int, P: int) -> list:
    """(first row, rows) of every rank of a P-rank run of case n."""
    return [hermite_partition(n, CASES[n]["chunk"], P, r) for r in range(P)]


# ---- markers ----------------------------------------------------------------------------------
def _windows(n: int) -> list:
    """Row ranges [lo, hi) that must hold a marker: every chunk, every narrow slice with real
    rows, and every rank's first and last unit of 1024 rows for each P of the case."""
    g = geometry(n, "fp32")
    w = [(c * g["chunk"], min(n, (c + 1) * g["chunk"])) for c in range(-(-n // g["chunk"]))]
    w += [(s * g["slice"], min(n, (s + 1) * g["slice"])) for s in range(g["n_slices"])
          if s * g["slice"] < n]
    for P in CASES[n]["ranks"]:
        for row0, rows in rank_rows(n, P):
            w += [(lo, min(n, lo + HERMITE_UNIT)) for lo in _end_units(n, row0, rows)]
    return w


def _end_units(n: int, row0: int, rows: int) -> tuple:
    """First rows of a rank's first unit and of its last unit that holds a body."""
    assert row0 < n, "a rank holds ghost rows only"
    return row0, (min(row0 + rows, n) - 1) // HERMITE_UNIT * HERMITE_UNIT


def every_tile_end(n: int) -> bool:
    """Whether the K <= 256 markers can take the first and the last row of every 256-row tile."""
    return 2 * -(-n // WG) <= MAX_MARKERS


@lru_cache(maxsize=None)
def place_markers(n: int) -> np.ndarray:
    """Sorted marker rows of case n, the same for every dtype (coverage() states what holds)."""
    chunk = CASES[n]["chunk"] or auto_chunk(n)
    m = {0, n - 1}
    if every_tile_end(n):
        for t0 in range(0, n, WG):
            m.update((t0, min(n, t0 + WG) - 1))
    else:  # the first row of the first tile and the last real row of the last tile of a chunk
        for c0 in range(0, n, chunk):
            m.update((c0, min(n, c0 + chunk) - 1))
    k = 0
    for c0 in range(0, n, chunk):  # one strictly between a chunk's first and last 128-row tile
        lo, last = c0 + 128, (min(n, c0 + chunk) - 1) // 128 * 128
        if last > lo and not any(lo <= i < last for i in m):
            m.add(lo + (OFFSETS[k % len(OFFSETS)] + WG * (k % 3)) % (last - lo))
            k += 1
    rows = np.array(sorted(m))
    k = 0
    for lo, hi in _windows(n):  # windows still empty: a marker at a cycling offset
        if not ((rows >= lo) & (rows < hi)).any():
            m.add(lo + OFFSETS[k % len(OFFSETS)] % (hi - lo))
            rows = np.array(sorted(m))
            k += 1
    # the rest step through the interior tiles of the chunks, one tile per chunk per round
    real_chunks, tpc = -(-n // chunk), chunk // WG
    k = 0
    while not every_tile_end(n) and len(m) < MAX_MARKERS and \
            k < real_chunks * (tpc - 2) * len(OFFSETS):
        c, rnd = k % real_chunks, k // real_chunks
        row = c * chunk + (1 + (rnd + 3 * c) % (tpc - 2)) * WG + \
            OFFSETS[(rnd // (tpc - 2) + c + rnd) % len(OFFSETS)]
        if row < n:
            m.add(row)
        k += 1
    out = np.array(sorted(m), dtype=np.int64)
    out.setflags(write=False)
    return out


def coverage(n: int, dtype: str, markers) -> dict:
    """What the markers leave uncovered, in integers (all lists empty: everything holds):
    ends: bodies 0 and n - 1; chunks, slices (narrow slices with real rows, the short last one
    included), units ((P, rank, unit) of each rank's first and last unit of 1024 rows);
    tile_ends: every_tile_end cases: tiles of this dtype with a first or last real row that is no
    marker (fp64: 128-row tiles, one marker on either end, since both ends of all 157 of them
    would take 314 markers); chunk_tiles: elsewhere, chunks whose first or last real tile holds
    no marker; interior: elsewhere, chunks of more than two tiles with no marker strictly
    between the first and the last tile."""
    g = geometry(n, dtype)
    m = np.asarray(markers, dtype=np.int64)
    assert m.ndim == 1 and len(m) and (np.diff(m) > 0).all() and m[0] >= 0 and m[-1] < n
    has = set(m.tolist())
    chunk, T, sl = g["chunk"], g["tile"], g["slice"]

    def empty(lo, hi):
        return not ((m >= lo) & (m < min(hi, n))).any()

    out = {"ends": [i for i in (0, n - 1) if i not in has],
           "count": [] if len(m) <= MAX_MARKERS else [len(m)],
           "chunks": [c for c in range(-(-n // chunk)) if empty(c * chunk, (c + 1) * chunk)],
           "slices": [s for s in range(g["n_slices"])
                      if s * sl < n and empty(s * sl, (s + 1) * sl)],
           "units": [], "tile_ends": [], "chunk_tiles": [], "interior": []}
    for P in CASES[n]["ranks"]:
        for r, (row0, rows) in enumerate(rank_rows(n, P)):
            out["units"] += [(P, r, lo // HERMITE_UNIT) for lo in _end_units(n, row0, rows)
                             if empty(lo, lo + HERMITE_UNIT)]
    if every_tile_end(n):
        for t0 in range(0, n, T):
            ends = (t0 in has, min(n, t0 + T) - 1 in has)
            if not (all(ends) if T == WG else any(ends)):
                out["tile_ends"].append(t0 // T)
    else:
        for c in range(-(-n // chunk)):
            lo, hi = c * chunk, min(n, (c + 1) * chunk)
            last = (hi - 1) // T * T
            if empty(lo, lo + T) or empty(last, hi):
                out["chunk_tiles"].append(c)
            if last - (lo + T) > 0 and empty(lo + T, last):
                out["interior"].append(c)
    return out


def assert_coverage(n: int, dtype: str, markers) -> None:
    bad = {k: v for k, v in coverage(n, dtype, markers).items() if v}
    assert not bad, f"n = {n} {dtype}: markers leave uncovered {bad}"


# ---- bodies -----------------------------------------------------------------------------------
def _off_grid(x, rng):
    """x moved to 0.3 .. 0.5 fp32 ulp beside its nearest fp32 value, on a random side."""
    hi = x.astype(np.float32)
    ulp = np.spacing(np.abs(hi)).astype(np.float64)
    return hi.astype(np.float64) + rng.choice((-1.0, 1.0), x.shape) * rng.uniform(0.3, 0.5,
                                                                                 x.shape) * ulp


def probe_bodies(n: int, seed: int = 0, markers=None):
    """(bodies, markers) of the module docstring; marker masses uniform in [1, 2] x 1e22 kg."""
    markers = place_markers(n) if markers is None else np.asarray(markers, dtype=np.int64)
    K = len(markers)
    rng = np.random.default_rng(104729 * (seed + 1) + n)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    pos = u * (UNIT * np.cbrt(rng.uniform(8.0, 64.0, n)))[:, None]       # shell 2 U .. 4 U
    k = np.arange(K) + 0.5                                                # Fibonacci sphere
    z, az = 1.0 - 2.0 * k / K, np.pi * (1.0 + 5.0 ** 0.5) * k
    fib = np.stack([np.sqrt(1 - z * z) * np.cos(az), np.sqrt(1 - z * z) * np.sin(az), z], -1)
    pos[markers] = fib[rng.permutation(K)] * (UNIT * rng.uniform(0.97, 1.0, K))[:, None]
    pos += SHIFT
    rest = np.ones(n, dtype=bool)
    rest[markers] = False
    pos[rest] = _off_grid(pos[rest], rng)
    vel = rng.normal(size=(n, 3)) * 1e4 + DRIFT
    mass, radius = np.zeros(n), np.zeros(n)
    mass[markers] = rng.uniform(1e22, 2e22, K)
    radius[markers] = R_MARKER
    return BodySet(pos, vel, mass, radius), markers


def seen(b: BodySet, dtype: str):
    """Positions, velocities and mu = G m as the pair kernel of `dtype` sees them, in fp64:
    fp32 rounds all three; mixed: positions hi + lo (tests/test_hermite_mixed_gpu.py ds_seen),
    velocities and mu in fp32; fp64 as given."""
    pos, _ = nnh.seen(b.pos, np.zeros(b.n), dtype)
    vel, mu = np.asarray(b.vel, np.float64), G_SI * np.asarray(b.mass, np.float64)
    if dtype != "fp64":
        vel, mu = vel.astype(np.float32).astype(np.float64), mu.astype(np.float32).astype(
            np.float64)
    return pos, vel, mu


def pair_terms(pos_i, vel_i, pos_m, vel_m, mu_m):
    """fp64 terms of K sources on b bodies by oracle.acc_jerk's own expressions: a terms
    (b, K, 3), jerk terms (b, K, 3), phi terms (b, K); zero for r^2 < CUTOFF^2 (the self pair)."""
    d = pos_m[None, :, :] - pos_i[:, None, :]
    w = vel_m[None, :, :] - vel_i[:, None, :]
    r2 = (d * d).sum(-1)
    ok = r2 >= CUTOFF * CUTOFF
    inv = np.zeros_like(r2)
    np.divide(1.0, np.sqrt(r2, where=ok, out=np.ones_like(r2)), where=ok, out=inv)
    inv2 = inv * inv
    mi = mu_m[None, :] * inv
    s = mi * inv2
    al = 3.0 * (d * w).sum(-1) * inv2
    return s[:, :, None] * d, s[:, :, None] * (w - al[:, :, None] * d), -mi


def two_sum_reduce(t):
    """Compensated sum over axis 1 (Knuth's two-sum, the error terms added at the end): the
    result carries the exact sum of the terms to a few u^2 sum |term| plus one rounding."""
    s = np.zeros(t.shape[:1] + t.shape[2:], dtype=t.dtype)
    e = np.zeros_like(s)
    for k in range(t.shape[1]):
        x = t[:, k]
        y = s + x
        z = y - s
        e += (s - (y - z)) + (x - z)
        s = y
    return s + e


def _threads(fn, n: int, block: int):
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return list(ex.map(fn, range(0, n, block)))


def reference(b: BodySet, markers, dtype: str, pos=None, block: int = 2048):
    """(acc (n, 3), jerk (n, 3), phi (n,), acc scale, jerk scale) of the K marker terms on the
    inputs as the kernel of `dtype` sees them. The scales, and for fp32 and mixed the sums, are
    oracle.acc_jerk(sources=markers)'s. fp64: the same terms summed with two-sum compensation,
    since a plain sum of 256 terms could use up a good part of the gate of 128 eps.
    pos: other positions than seen()'s (hi_only_shift)."""
    markers = np.asarray(markers, dtype=np.int64)
    p, v, mu = seen(b, dtype)
    p = p if pos is None else pos
    ra, rj, rphi, sa, sj = oracle.acc_jerk(p, v, mu, G=1.0, cutoff=CUTOFF, sources=markers,
                                           with_potential=True, with_abs=True)
    if dtype == "fp64":
        def rows(i0):
            ta, tj, tp = pair_terms(p[i0:i0 + block], v[i0:i0 + block], p[markers], v[markers],
                                    mu[markers])
            ra[i0:i0 + block] = two_sum_reduce(ta)
            rj[i0:i0 + block] = two_sum_reduce(tj)
            rphi[i0:i0 + block] = two_sum_reduce(tp)

        _threads(rows, b.n, block)
    return ra, rj, rphi, sa, sj


@lru_cache(maxsize=None)
def probe_case(n: int, dtype: str):
    """(bodies, markers, reference) of one case, computed once and read-only; the coverage is
    asserted in integers first, so no comparison against it can pass vacuously."""
    b, m = probe_bodies(n)
    assert_coverage(n, dtype, m)
    ref = reference(b, m, dtype)
    for a in (b.pos, b.vel, b.mass, b.radius) + ref:
        a.setflags(write=False)
    return b, m, ref


def visibility(b: BodySet, markers, ref, dtype: str, block: int = 2048) -> dict:
    """Shares of the (body, marker) terms, the K zero self terms included, that a gate of 128 eps
    could hide, for acceleration and jerk: `norm`: |term| < 2 x 128 eps |scale vector|; `comp`:
    every component within 2 x 128 eps of its own scale (the test a comparison really applies)."""
    markers = np.asarray(markers, dtype=np.int64)
    p, v, mu = seen(b, dtype)
    _, _, _, sa, sj = ref
    lim = 2.0 * GATE * EPS[dtype]

    def rows(i0):
        ta, tj, _ = pair_terms(p[i0:i0 + block], v[i0:i0 + block], p[markers], v[markers],
                               mu[markers])
        out = []
        for t, s in ((ta, sa[i0:i0 + block]), (tj, sj[i0:i0 + block])):
            out.append(int((np.linalg.norm(t, axis=-1) <
                            lim * np.linalg.norm(s, axis=-1)[:, None]).sum()))
            out.append(int((np.abs(t) <= lim * s[:, None, :]).all(-1).sum()))
        return out

    tot = np.array(_threads(rows, b.n, block)).sum(0) / (b.n * len(markers))
    return {"acc_norm": tot[0], "acc_comp": tot[1], "jerk_norm": tot[2], "jerk_comp": tot[3]}


def hi_only_shift(b: BodySet, markers, ref) -> np.ndarray:
    """Mixed precision: for every body, how far the reference moves when it is recomputed from
    the hi parts of the positions alone, in units of 2^-24 x scale: the largest over the
    components of a, j and phi. Above 10 x 128 for a massless body: its lo row matters."""
    hi = np.asarray(b.pos, np.float64).astype(np.float32).astype(np.float64)
    return ratios(*as_rows4(reference(b, markers, "mixed", pos=hi)), ref, "mixed").max(1)


def as_rows4(r):
    """A reference tuple as the (a4, j4) an engine returns."""
    return np.concatenate([r[0], r[2][:, None]], 1), np.concatenate(
        [r[1], np.zeros((len(r[1]), 1))], 1)


# ---- the gate ---------------------------------------------------------------------------------
def ratios(a4, j4, ref, dtype: str, rows=None) -> np.ndarray:
    """|got - ref| / (eps scale) per row and component (ax, ay, az, jx, jy, jz, phi)."""
    idx = slice(None) if rows is None else np.asarray(rows)
    ra, rj, rphi, sa, sj = (x[idx] for x in ref)
    got = np.concatenate([a4[:, :3], j4[:, :3], a4[:, 3:4]], 1)
    want = np.concatenate([ra, rj, rphi[:, None]], 1)
    scale = np.concatenate([sa, sj, np.abs(rphi)[:, None]], 1)
    return np.abs(got - want) / (EPS[dtype] * scale + 1e-300)


def assert_gate(a4, j4, n: int, dtype: str, rows=None, label: str = "", **where) -> tuple:
    """All rows at the gate for a, j and phi; a failure names what the error corresponds to
    (locate). Returns the worst ratios (acc, jerk, phi)."""
    b, m, ref = probe_case(n, dtype)
    r = ratios(a4, j4, ref, dtype, rows)
    worst = (float(r[:, :3].max()), float(r[:, 3:6].max()), float(r[:, 6].max()))
    if not max(worst) <= GATE or not (np.isfinite(a4).all() and np.isfinite(j4).all()):
        found = [{k: v if k not in ("iblocks", "where") or len(v) <= 8 else
                  f"{len(v)} from {v[0]} to {v[-1]}" for k, v in e.items()}
                 for e in locate(a4, j4, n, dtype, rows, **where)]
        raise AssertionError(f"{label}: acc {worst[0]:.3g} jerk {worst[1]:.3g} phi {worst[2]:.3g}"
                             f" x eps x scale (gate {GATE:g}); {found}")
    assert not j4[:, 3].any()
    return worst


# ---- what a failure corresponds to ------------------------------------------------------------
def _holds(got_row, want_bound) -> bool:
    """Whether one returned row is at the gate against (reference, eps x scale) of another row."""
    return bool((np.abs(got_row - want_bound[0][0]) / want_bound[1][0]).max() <= GATE)


def _unit_matrix(starts, markers) -> np.ndarray:
    """(units, K) 0/1: marker k lies in the unit that begins at starts[u]."""
    u = np.searchsorted(starts, markers, side="right") - 1
    M = np.zeros((len(starts), len(markers)))
    M[u, np.arange(len(markers))] = 1.0
    return M


def locate(a4, j4, n: int, dtype: str, rows=None, ipl: int = 0, groups: int = 0, P: int = 0,
           narrow: bool = False, nn: bool = False, worst: int = 4, limit: int = 1024) -> list:
    """locate_units() on the (a, j, phi) columns of case n under the launch shape ipl x groups."""
    b, m, ref = probe_case(n, dtype)
    p, v, mu = seen(b, dtype)

    def columns(r):
        ra, rj, rphi, sa, sj = (x[r] for x in ref)
        return (np.concatenate([ra, rj, rphi[:, None]], 1),
                EPS[dtype] * np.concatenate([sa, sj, np.abs(rphi)[:, None]], 1) + 1e-300)

    def terms(r):
        ta, tj, tp = pair_terms(p[r], v[r], p[m], v[m], mu[m])
        return np.concatenate([ta, tj, tp[:, :, None]], 2)

    got = np.concatenate([a4[:, :3], j4[:, :3], a4[:, 3:4]], 1)
    return locate_units(got, columns, terms, m, geometry(n, dtype, ipl, groups, nn), n, rows, P,
                        narrow, worst, limit)


def locate_units(got, columns, terms, m, g: dict, n: int, rows=None, P: int = 0,
                 narrow: bool = False, worst: int = 4, limit: int = 1024) -> list:
    """For the rows that miss the gate (the `limit` worst), fit what the residual is: up to two
    units, each missing (-1) or doubled (+1), where a unit is one marker, the markers of one
    tile, of one chunk or (narrow) of one narrow slice, the smallest unit that fits first; where
    no unit fits and P ranks are in use, whether the row holds the reference of the same local
    row of another rank. got: (rows, C) what the kernel returned; columns(r): (reference,
    eps x scale) (len(r), C) of the bodies r; terms(r): the (len(r), K, C) marker terms; g: the
    geometry. Returns the `worst` largest groups as dicts: kind / what / markers /
    chunk / tile / group (the chunk group under the launch shape of g) or slice, the
    i-blocks and the ranks (or narrow slices) of the failing rows, rows, fitted (how many of
    them the fit brings back inside the gate), ratio."""
    idx = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    want, bound = columns(idx)
    r_all = np.abs(got - want) / bound
    rmax = np.where(np.isfinite(r_all), r_all, np.inf).max(1)
    bad = np.nonzero(~(rmax <= GATE))[0]
    bad = bad[np.argsort(-rmax[bad], kind="stable")][:limit]
    if not len(bad):
        return []
    cand = [("marker", np.eye(len(m)), m)]
    if narrow:
        st = np.arange(g["n_slices"]) * g["slice"]
        cand.append(("slice", _unit_matrix(st, m), st))
    else:
        st = np.arange(g["n_pad"] // g["tile"]) * g["tile"]
        cand.append(("tile", _unit_matrix(st, m), st))
        st = np.arange(g["n_chunks"]) * g["chunk"]
        cand.append(("chunk", _unit_matrix(st, m), st))
    kinds = [(k, int(s)) for k, M, starts in cand for s, row in zip(starts, M) if row.any()]
    M = np.concatenate([M[M.any(1)] for _, M, _ in cand])
    T = terms(idx[bad])                                                   # (b, K, C)
    C = T.shape[2]
    U = np.einsum("uk,bkc->buc", M, T, optimize=True)                     # (b, units, C)
    bound = bound[bad]
    res = got[bad] - want[bad]
    res = np.where(np.isfinite(res), res, 0.0)
    # one unit: missing (got = ref - U) or doubled (got = ref + U)
    left = np.stack([np.abs((res[:, None, :] + U) / bound[:, None, :]).max(-1),
                     np.abs((res[:, None, :] - U) / bound[:, None, :]).max(-1)], -1)
    flat = left.reshape(len(bad), -1)
    best = flat.argmin(1)  # (the first of equal fits: the smallest unit)
    fits = [[divmod(int(k2), 2)] for k2 in best]
    fitted = flat[np.arange(len(bad)), best] <= GATE
    # two units, each a whole chunk (narrow: slice), where one does not fit
    big = np.array([u for u, (k, _) in enumerate(kinds) if k == ("slice" if narrow else "chunk")])
    sg = np.array([1.0, -1.0])  # index 0: missing (res + U), 1: doubled
    for i0 in range(0, len(bad), 32):
        sl = np.nonzero(~fitted[i0:i0 + 32])[0] + i0
        if not len(sl) or len(big) < 2:
            continue
        V = U[sl][:, big, None, :] * sg[None, None, :, None]              # (b, nb, 2, C)
        V = V.reshape(len(sl), -1, C)
        two = np.abs((res[sl][:, None, None, :] + V[:, :, None, :] + V[:, None, :, :])
                     / bound[sl][:, None, None, :]).max(-1)               # (b, 2 nb, 2 nb)
        k = two.reshape(len(sl), -1).argmin(1)
        for j, (i, kk) in enumerate(zip(sl, k)):
            a, c = divmod(int(kk), two.shape[1])
            if two[j, a, c] <= GATE and a // 2 != c // 2:
                fits[i] = sorted([(int(big[a // 2]), a % 2), (int(big[c // 2]), c % 2)])
                fitted[i] = True
    ranks = rank_rows(n, P) if P else []
    groups_out: dict = {}
    for i, row in enumerate(idx[bad]):
        key, extra = tuple(fits[i]), {}
        if not fitted[i] and P:  # another rank's rows?
            me = next(r for r, (r0, c) in enumerate(ranks) if r0 <= row < r0 + c)
            for r, (r0, c) in enumerate(ranks):
                src = row - ranks[me][0] + r0
                if r != me and src < n and _holds(got[bad[i]], columns(np.array([src]))):
                    key, extra = ("rows", me, r), dict(kind="rows of another rank", rank=me,
                                                      holds_rank=r)
                    fitted[i] = True
                    break
        e = groups_out.get(key)
        if e is None:
            e = dict(extra, rows=0, fitted=0, ratio=0.0, iblocks=set(), where=set())
            if not extra:
                e["units"] = []
                for u, sign in fits[i]:
                    kind, start = kinds[u]
                    d = dict(kind=kind, what="doubled" if sign else "missing",
                             markers=m[M[u] > 0].tolist())
                    if kind == "slice":
                        d["slice"] = start // g["slice"]
                    else:
                        if narrow:
                            d["slice"] = start // g["slice"]
                        c = start // g["chunk"]
                        d.update(chunk=c, group=c // g["per"])
                        if kind != "chunk":
                            tiles = sorted({int(x % g["chunk"]) // g["tile"] for x in d["markers"]})
                            d["tile"] = tiles[0] if len(tiles) == 1 else tiles
                    e["units"].append(d)
            groups_out[key] = e
        e["rows"] += 1
        e["fitted"] += int(fitted[i])
        e["ratio"] = max(e["ratio"], float(rmax[bad[i]]))
        e["iblocks"].add(int(row) // g["iblock"])
        if narrow:
            e["where"].add(("slice", int(row) // g["slice"]))
        elif P:
            e["where"].add(("rank", next(r for r, (r0, c) in enumerate(ranks)
                                         if r0 <= row < r0 + c)))
    out = sorted(groups_out.values(), key=lambda e: (-e["rows"], -e["ratio"]))[:worst]
    for e in out:
        e["iblocks"], e["where"] = sorted(e["iblocks"]), sorted(e["where"])
    return out


# ---- NumPy emulation of the chunked sum (the mutation controls) -------------------------------
def unit_partials(n: int, dtype: str, starts, rows=None, block: int = 4096) -> np.ndarray:
    """(units, rows, 7) fp64: the partial sum (ax, ay, az, jx, jy, jz, phi) of every row over the
    markers of every unit of j rows that begins at starts[u]: chunks, tiles or narrow slices."""
    b, m, _ = probe_case(n, dtype)
    p, v, mu = seen(b, dtype)
    idx = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    M = _unit_matrix(np.asarray(starts), m)
    out = np.zeros((len(starts), len(idx), 7))

    def part(i0):
        r = idx[i0:i0 + block]
        ta, tj, tp = pair_terms(p[r], v[r], p[m], v[m], mu[m])
        T = np.concatenate([ta, tj, tp[:, :, None]], 2)
        out[:, i0:i0 + block] = np.einsum("uk,bkc->ubc", M, T, optimize=True)

    _threads(part, len(idx), block)
    return out


def fold(partials):
    """The reduce: the partials added in unit order, as (a4, j4)."""
    s = np.zeros(partials.shape[1:])
    for u in range(partials.shape[0]):
        s = s + partials[u]
    return (np.concatenate([s[:, :3], s[:, 6:7]], 1),
            np.concatenate([s[:, 3:6], np.zeros((len(s), 1))], 1))


# ---- the narrow active list -------------------------------------------------------------------
def active_list(n: int, dtype: str, markers) -> np.ndarray:
    """At most 8,192 sorted rows: one of every workgroup, the markers, and the rows on both
    sides of every narrow-slice boundary."""
    g = geometry(n, dtype)
    wg = np.arange(-(-n // WG))
    rows = set(np.minimum(wg * WG + (wg * 37) % WG, n - 1).tolist()) | set(
        np.asarray(markers).tolist())
    for s in range(1, g["n_slices"]):
        rows.update(i for i in (s * g["slice"] - 1, s * g["slice"]) if i < n)
    # ... filled up with evenly spaced rows: a marker's nearest and second nearest markers are
    # often within the bound of each other, and the markers must stay a small part of the list
    # for the share of such rows to stay below 1 % (check_nn)
    rows.update(np.linspace(0, n - 1, 8192 - len(rows)).astype(np.int64).tolist())
    out = np.array(sorted(rows), dtype=np.int32)
    assert len(out) <= 8192 and len(np.unique(out // WG)) == len(wg)
    assert np.isin(markers, out).all()
    assert all({s * g["slice"] - 1, s * g["slice"]} <= rows for s in range(1, -(-n // g["slice"])))
    return out


# ---- nearest neighbours -----------------------------------------------------------------------
def nn_over_markers(b: BodySet, markers, dtype: str, block: int = 4096):
    """(q, nn, second-best q) of every body over the marker columns alone, after asserting that
    this is the nearest neighbour over all columns: with D an upper bound of the extent (twice
    the largest distance from the centre) and R the markers' radius, D^2 < R^2 (a massless
    body: any marker has q < 0 <= q of any massless one) and D^2 < 3 R^2 (a marker: another
    marker has q <= D^2 - 4 R^2 < -R^2 <= q of any massless one)."""
    m, n = np.asarray(markers, dtype=np.int64), b.n
    pos, rad = nnh.seen(b.pos, b.radius, dtype)
    D = 2.0 * np.sqrt(((pos - SHIFT) ** 2).sum(1).max())
    R = float(rad[m].min())
    rest = np.ones(n, dtype=bool)
    rest[m] = False
    assert len(m) >= 2 and not rad[rest].any() and (rad[m] == R).all()
    assert D * D < R * R and D * D < 3.0 * R * R
    q, nn, q2 = np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n)

    def rows(i0):
        d = pos[m][None, :, :] - pos[i0:i0 + block, None, :]
        r2 = (d * d).sum(-1)
        sr = rad[m][None, :] + rad[i0:i0 + block, None]
        qq = np.where(r2 >= CUTOFF * CUTOFF, r2 - sr * sr, np.inf)
        qq[m[None, :] == np.arange(i0, min(n, i0 + block))[:, None]] = np.inf
        k = qq.argmin(1)  # (the first of equal minima: the lowest j, the markers being sorted)
        ar = np.arange(len(k))
        q[i0:i0 + block], nn[i0:i0 + block] = qq[ar, k], m[k]
        qq[ar, k] = np.inf
        q2[i0:i0 + block] = qq.min(1)

    _threads(rows, n, block)
    for a in (q, nn, q2):
        a.setflags(write=False)
    return q, nn, q2


@lru_cache(maxsize=None)
def nn_reference(n: int, dtype: str):
    b, m, _ = probe_case(n, dtype)
    return nn_over_markers(b, m, dtype)


def winners_home(n: int, dtype: str) -> tuple:
    """(fewest bodies whose nearest neighbour lives in one chunk, the same per narrow slice with
    real rows): the NN fold must pick the winner out of every partial for that many bodies."""
    g = geometry(n, dtype)
    _, nn, _ = nn_reference(n, dtype)
    per_chunk = np.bincount(nn // g["chunk"], minlength=-(-n // g["chunk"]))
    per_slice = np.bincount(nn // g["slice"], minlength=-(-n // g["slice"]))
    return int(per_chunk.min()), int(per_slice.min())


def check_nn(q, nn, n: int, dtype: str, rows=None, cap: float = 0.01) -> float:
    """The three assertions and the bound B = 8 u (r^2 + s^2) of
    hermite_nn_helpers.check_against_oracle against the marker-column reference; returns the
    excused share."""
    b, m, _ = probe_case(n, dtype)
    pos, rad = nnh.seen(b.pos, b.radius, dtype)
    idx = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    oq, onn, oq2 = (x[idx] for x in nn_reference(n, dtype))
    assert (nn >= 0).all() and (nn < n).all() and (nn != idx).all()
    qr, scale = nnh.pair_q(pos, rad, idx, nn)
    B = 8.0 * nnh.U[dtype] * scale
    assert (np.abs(q - qr) <= B).all(), float((np.abs(q - qr) / B).max())
    assert (qr - oq <= 2.0 * B).all(), "a returned neighbour is not among the nearest"
    _, sbest = nnh.pair_q(pos, rad, idx, onn)
    clear = (oq2 - oq) > 2.0 * 8.0 * nnh.U[dtype] * sbest
    assert np.array_equal(nn[clear], onn[clear])
    excused = 1.0 - clear.mean()
    assert excused <= cap, excused
    return float(excused)
