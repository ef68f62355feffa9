"""Marker probe of the Newton-3 sym schedule's pair coverage (tests/test_sym_probe_cpu.py and
tests/test_gpu_sym_probe.py). NumPy only.

All bodies but K markers are massless, so every body's acceleration is a sum of K terms, one
per marker. A marker in chunk B seen from a body in chunk A runs the chunk pair (A, B) through
every stage of the schedule (csrc/hip/nbody_sym.hip): the tile (i side or j-side carriers,
whichever row owns the pair), the partial slot, the split parts or the diagonal parts, the row
reduce, the node tree and the tail. With K small, one lost or doubled term is far above the
rounding gate 128 eps sum_j |term_ij| for every body, and the reference costs O(K n), so all n
bodies are checked at every size.

Reference times measured on an 8-core host (row blocks on 8 threads, fp64 terms; the fp64
cases add the two-sum compensation), bodies included, per cached case:

    n        K    fp32    fp64
    40000    40   0.3 s   0.3 s    (the first case pays the thread pool and imports)
    65536    64   0.2 s   0.2 s
    90000    88   0.2 s   0.4 s
    131072   128  0.3 s   0.8 s
    150000   74   0.2 s   0.4 s
    262144   128  0.6 s   1.4 s
    524288   256  2.7 s   -
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from functools import lru_cache

import numpy as np

from gravsim.config import G_SI
from gravsim.models import initial_conditions as ic
from gravsim.models.initial_conditions import BodySet
from gravsim.ops import _native
from gravsim.parallel import partition

C = partition.SYM_CHUNK  # 2048 bodies per chunk
Q = 128                  # bodies per quantum (16 quanta per chunk)
EPS = {"fp32": 2.0 ** -24, "fp64": 2.0 ** -53}
GATE = 128.0             # the project's gate: |got - ref| <= 128 eps sum_j |term_ij|
MAX_MARKERS = 256
# Offsets within a 128-body quantum, cycled over the markers: both halves of the fp32 j-pair
# tile (0-63 | 64-127) and the ends of the fp64 64-body tiles come first.
OFFSETS = (0, 63, 64, 127, 1, 62, 65, 126, 31, 32, 95, 96)

# The sym cases of the GPU probe (tests/test_gpu_sym_probe.py): n -> expected geometry.
SYM_CASES = {
    40000: dict(n_pad=49152, NC=24, L=1, S=192, D=16, Kr=0, Np=2, RB=3),
    65536: dict(n_pad=65536, NC=32, L=2, S=128, D=8, Kr=8, Np=2, RB=1),
    90000: dict(n_pad=98304, NC=48, L=2, S=192, D=8, Kr=12, Np=2, RB=3),
    131072: dict(n_pad=131072, NC=64, L=4, S=128, D=4, Kr=8, Np=4, RB=1),
    150000: dict(n_pad=163840, NC=80, L=4, S=160, D=4, Kr=10, Np=4, RB=5),
    262144: dict(n_pad=262144, NC=128, L=8, S=128, D=2, Kr=8, Np=4, RB=1),
    524288: dict(n_pad=524288, NC=256, L=16, S=128, D=1, Kr=8, Np=4, RB=1),
}
SYM_PROBE = [(n, dt) for n in SYM_CASES for dt in ("fp32", "fp64")
             if not (n == 524288 and dt == "fp64")]


def geometry(n: int) -> dict:
    """The sym schedule's geometry at n bodies (Python mirror of layout.cpp)."""
    n_pad = partition.layout(n, sym=True).n_pad
    g = partition.sym_geometry(n_pad)
    kr, npart = partition.sym_split(n_pad)
    B = partition.sym_blocks(g["NC"])
    g.update(n=n, n_pad=n_pad, Kr=kr, Np=npart, B=B, RB=g["NC"] // B,
             real_chunks=-(-n // C))
    return g


@lru_cache(maxsize=None)
def shell_lens(NC: int) -> tuple:
    """h(A) of every row: NC/2 for the rows that take their antipodal chunk, else NC/2 - 1
    (layout.cpp gs_sym_shell_len, the native library's own)."""
    lib = _native.cpu_lib()
    return tuple(int(lib.gs_sym_shell_len(A, NC)) for A in range(NC))


def _serving_chunks(g: dict, d: int) -> list:
    """Real chunks B such that a real row A = B - d holds B in its shell."""
    NC, real, h = g["NC"], g["real_chunks"], shell_lens(g["NC"])
    return [B for B in range(real) if (B - d) % NC < real and d <= h[(B - d) % NC]]


def place_markers(n: int, dtype: str = "fp32") -> np.ndarray:
    """Sorted marker indices: every real chunk holds one (two up to 131072 bodies), bodies 0
    and n - 1 are markers, the offsets within a quantum cycle through OFFSETS, and the quanta
    are chosen so that coverage() holds: the distances d with the fewest serving chunks (the
    antipodal one first) pick their 16 quanta first. The same for both dtypes."""
    if dtype not in EPS:
        raise ValueError(dtype)
    g = geometry(n)
    NC, real = g["NC"], g["real_chunks"]
    per = 2 if n <= 131072 else 1
    last = (n - 1) // C
    avail = [min(16, -(-(min(n, (c + 1) * C) - c * C) // Q)) for c in range(real)]
    quanta = [[] for _ in range(real)]       # chosen quanta per chunk
    fixed = {0: [0]}                          # body 0, body n - 1
    fixed.setdefault(last, []).append(n - 1)
    for c, idx in fixed.items():
        for i in idx:
            if (i % C) // Q not in quanta[c]:
                quanta[c].append((i % C) // Q)
    serve = {d: _serving_chunks(g, d) for d in range(1, NC // 2 + 1)}

    def free(c):
        return len(quanta[c]) < max(per, len(fixed.get(c, ())))

    for d in sorted(serve, key=lambda d: (len(serve[d]), -d)):
        have = {q for c in serve[d] for q in quanta[c]}
        for q in range(16):
            if q in have:
                continue
            cand = [c for c in serve[d] if free(c) and q < avail[c] and q not in quanta[c]]
            if not cand:
                continue  # (coverage() reports it)
            # the chunk that serves the fewest distances: the flexible ones stay free
            c = min(cand, key=lambda c: (sum(c in serve[e] for e in serve), c))
            quanta[c].append(q)
    count = [sum(q in qs for qs in quanta) for q in range(16)]
    for c in range(real):  # the chunks still free: the least used quantum
        while free(c):
            q = min((q for q in range(avail[c]) if q not in quanta[c]),
                    key=lambda q: (count[q], q))
            quanta[c].append(q)
            count[q] += 1
    out, k = set(i for idx in fixed.values() for i in idx), 0
    for c in range(real):
        for q in quanta[c]:
            if any(i // C == c and (i % C) // Q == q for i in out):
                continue  # the fixed marker of this quantum
            room = min(n, c * C + (q + 1) * Q) - (c * C + q * Q)
            out.add(c * C + q * Q + min(OFFSETS[k % len(OFFSETS)], room - 1))
            k += 1
    m = np.array(sorted(out), dtype=np.int64)
    assert len(m) <= MAX_MARKERS and m[0] == 0 and m[-1] == n - 1
    return m


def coverage(n: int, markers) -> dict:
    """What the markers leave uncovered, in integer arithmetic (all lists empty: it holds).
    shell: (d, q) for which no real row A holds a chunk (A + d) mod NC in its shell with a
    marker in quantum q; diag: diagonal parts 0 .. D-1 no marker falls into (within its own
    chunk); chunks: real chunks with fewer markers than asked; ends / offsets: bodies 0 and
    n - 1, and the offsets 0, 63, 64, 127 within a quantum."""
    g = geometry(n)
    NC, real, D = g["NC"], g["real_chunks"], g["D"]
    m = np.asarray(markers, dtype=np.int64)
    assert m.ndim == 1 and len(m) and (np.diff(m) > 0).all() and m[0] >= 0 and m[-1] < n
    chunk, quantum = m // C, (m % C) // Q
    in_chunk = [set(quantum[chunk == c].tolist()) for c in range(real)]
    shell = []
    for d in range(1, NC // 2 + 1):
        have = set().union(*[in_chunk[B] for B in _serving_chunks(g, d)], set())
        shell += [(d, q) for q in range(16) if q not in have]
    parts = set(((m % C) // (C // D)).tolist())
    per = 2 if n <= 131072 else 1
    return {
        "shell": shell,
        "diag": [p for p in range(D) if p not in parts],
        "chunks": [c for c in range(real) if (chunk == c).sum() < per],
        "ends": [i for i in (0, n - 1) if i not in set(m.tolist())],
        "offsets": [o for o in (0, 63, 64, 127) if o not in set((m % Q).tolist())],
        "count": [] if len(m) <= MAX_MARKERS else [len(m)],
    }


def assert_coverage(n: int, markers) -> None:
    bad = {k: v for k, v in coverage(n, markers).items() if v}
    assert not bad, f"n = {n}: markers leave uncovered {bad}"


def probe_bodies(n: int, dtype: str = "fp32", seed: int = 0):
    """(bodies, markers): random_cube positions and velocities (a few 1e4 m/s), marker masses
    uniform in [1e24, 1e25] kg, every other mass 0."""
    b = ic.random_cube(n, seed=1000 + seed)
    markers = place_markers(n, dtype)
    rng = np.random.default_rng(7919 * (seed + 1) + n)
    mass = np.zeros(n)
    mass[markers] = rng.uniform(1e24, 1e25, len(markers))
    return BodySet(b.pos, b.vel, mass), markers


def seen(bodies: BodySet, dtype: str):
    """Positions, velocities and mu = G m as the kernel of `dtype` sees them, in fp64."""
    T = np.float32 if dtype == "fp32" else np.float64
    rd = lambda x: np.asarray(x, dtype=np.float64).astype(T).astype(np.float64)  # noqa: E731
    return rd(bodies.pos), rd(bodies.vel), rd(G_SI * np.asarray(bodies.mass, dtype=np.float64))


def pair_terms(p_i, p_m, mu_m, cut2: float = 0.0):
    """fp64 terms (b, K, 3) of K sources on b bodies: mu d / r^3 with d = x_m - x_i, zero for
    a pair with r^2 < cut2 and for r = 0 (the self term)."""
    d = p_m[None, :, :] - p_i[:, None, :]
    r2 = (d * d).sum(-1)
    ok = (r2 >= cut2) & (r2 > 0.0)
    inv = np.zeros_like(r2)
    np.divide(1.0, np.sqrt(r2, where=ok, out=np.ones_like(r2)), where=ok, out=inv)
    s = mu_m[None, :] * inv * inv * inv
    return s[:, :, None] * d


def _two_sum_reduce(t):
    """Compensated sum over axis 1 of (b, K, 3): s + e carries the exact sum of the terms seen
    so far up to O(u^2) (Knuth's two-sum; the error terms are added at the end)."""
    s = np.zeros((t.shape[0], 3))
    e = np.zeros_like(s)
    for k in range(t.shape[1]):
        x = t[:, k, :]
        y = s + x
        z = y - s
        e += (s - (y - z)) + (x - z)
        s = y
    return s + e


def reference(bodies: BodySet, markers, dtype: str, cutoff=None, block: int = 2048):
    """(acc, absacc) (n, 3): the K marker terms of every body on the inputs as the kernel sees
    them (positions and mu rounded to dtype), computed in fp64. fp64: summed with two-sum
    compensation, so the reference's own error is a few 2^-53 sum |term| (a plain sum of 128
    terms could use up the whole gate). cutoff: pairs with r^2 < cutoff^2 give nothing (the
    reference's hard select); None: only the self term gives nothing."""
    markers = np.asarray(markers, dtype=np.int64)
    pos, _, mu = seen(bodies, dtype)
    rest = np.ones(bodies.n, dtype=bool)
    rest[markers] = False
    assert not mu[rest].any(), "a body outside the markers has mass"
    p_m, mu_m = pos[markers], mu[markers]
    cut2 = 0.0 if cutoff is None else float(cutoff) ** 2
    n = bodies.n
    acc, absacc = np.zeros((n, 3)), np.zeros((n, 3))

    def rows(i0: int) -> None:
        t = pair_terms(pos[i0:i0 + block], p_m, mu_m, cut2)
        acc[i0:i0 + block] = _two_sum_reduce(t) if dtype == "fp64" else t.sum(1)
        absacc[i0:i0 + block] = np.abs(t).sum(1)

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        list(ex.map(rows, range(0, n, block)))
    return acc, absacc


@lru_cache(maxsize=None)
def probe_case(n: int, dtype: str):
    """(bodies, markers, acc, absacc) of one probe data set, computed once and read-only."""
    b, m = probe_bodies(n, dtype)
    acc, absacc = reference(b, m, dtype)
    for a in (b.pos, b.vel, b.mass, m, acc, absacc):
        a.setflags(write=False)
    return b, m, acc, absacc


def blind_pairs(bodies: BodySet, markers, absacc, dtype: str, block: int = 2048) -> int:
    """How many (body, marker) pairs have a term within the gate in all three components:
    such a term could vanish unseen (the K self-pairs, whose term is zero, among them)."""
    pos, _, mu = seen(bodies, dtype)
    markers = np.asarray(markers, dtype=np.int64)
    bound = GATE * EPS[dtype] * absacc

    def rows(i0: int) -> int:
        t = pair_terms(pos[i0:i0 + block], pos[markers], mu[markers])
        return int((np.abs(t) <= bound[i0:i0 + block, None, :]).all(-1).sum())

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return sum(ex.map(rows, range(0, bodies.n, block)))


def gate_ratio(got, ref, absacc, dtype: str) -> np.ndarray:
    """|got - ref| / (eps sum |term|) per body and component: the gate is <= 128."""
    return np.abs(got - ref) / (EPS[dtype] * absacc + 1e-300)


def unit_of(g: dict, i: int, m: int) -> dict:
    """The unit of the schedule that evaluates the pair (body i, marker m): i chunk A, marker
    chunk B, d = (B - A) mod NC, the owning row, whether body i sits on the row's i side or is
    reached through the j-side carriers, and the shell segment (with its split part) or the
    diagonal part."""
    NC, L, S, D, Kr, Np = g["NC"], g["L"], g["S"], g["D"], g["Kr"], g["Np"]
    A, B = int(i) // C, int(m) // C
    d = (B - A) % NC
    out = {"A": A, "B": B, "d": d}
    if A == B:
        out.update(row=A, side="i", kind="diagonal", part=(int(m) % C) // (C // D))
        return out
    h = shell_lens(NC)
    if d <= h[A]:  # row A owns the pair: the marker is a j body of its shell
        row, side, dist, q = A, "i", d, (int(m) % C) // Q
    else:          # row B owns it: body i is a j body of the marker's row
        row, side, dist, q = B, "j", (A - B) % NC, (int(i) % C) // Q
    sq = (dist - 1) * 16 + q
    seg = sq // L
    out.update(row=row, side=side, kind="segment", segment=seg,
               part=(sq % L) * Np // L if seg >= S - Kr else None)
    return out


def locate(got, ref, absacc, markers, bodies: BodySet, dtype: str, cutoff=None, worst: int = 5,
           limit: int = 8192) -> list:
    """For the bodies that miss the gate (the `limit` worst), fit which marker's term is
    missing (coefficient -1) or doubled (+1): the (marker, sign) that leaves the smallest
    residual. Returns the `worst` largest groups as dicts (unit_of's fields, plus marker,
    what, bodies, fitted: how many of them the fit brings back inside the gate, ratio)."""
    g = geometry(bodies.n)
    markers = np.asarray(markers, dtype=np.int64)
    ratio = gate_ratio(got, ref, absacc, dtype).max(1)
    bad = np.nonzero(ratio > GATE)[0]
    bad = bad[np.argsort(-ratio[bad], kind="stable")][:limit]
    if not len(bad):
        return []
    pos, _, mu = seen(bodies, dtype)
    cut2 = 0.0 if cutoff is None else float(cutoff) ** 2
    groups: dict = {}
    for i0 in range(0, len(bad), 512):
        ib = bad[i0:i0 + 512]
        t = pair_terms(pos[ib], pos[markers], mu[markers], cut2)       # (b, K, 3)
        r = (np.asarray(got)[ib] - ref[ib])[:, None, :]
        bound = (EPS[dtype] * absacc[ib] + 1e-300)[:, None, :]
        left = np.stack([(np.abs(r + t) / bound).max(-1),              # missing: got = ref - t
                         (np.abs(r - t) / bound).max(-1)], axis=-1)    # doubled: got = ref + t
        flat = left.reshape(len(ib), -1)
        best = flat.argmin(1)
        for i, k2, res in zip(ib, best, flat[np.arange(len(ib)), best]):
            k, sign = divmod(int(k2), 2)
            u = unit_of(g, int(i), int(markers[k]))
            key = (u["A"], int(markers[k]), sign, u.get("segment"), u["part"])
            e = groups.setdefault(key, dict(u, marker=int(markers[k]),
                                            what="doubled" if sign else "missing",
                                            bodies=0, fitted=0, ratio=0.0))
            e["bodies"] += 1
            e["fitted"] += int(res <= GATE)
            e["ratio"] = max(e["ratio"], float(ratio[i]))
    return sorted(groups.values(), key=lambda e: (-e["bodies"], -e["ratio"]))[:worst]


def assert_probe_gate(got, ref, absacc, markers, bodies: BodySet, dtype: str, cutoff=None,
                      label: str = "") -> float:
    """The project's gate on every body; a failure names the worst units (locate). Returns
    the worst ratio (<= 128)."""
    worst = float(gate_ratio(got, ref, absacc, dtype).max())
    if not worst <= GATE or not np.isfinite(np.asarray(got)).all():
        where = locate(got, ref, absacc, markers, bodies, dtype, cutoff)
        raise AssertionError(
            f"{label}: error {worst:.3g} x eps x sum|terms| (gate {GATE:g}); units: {where}")
    return worst
