"""NumPy fp64 oracle: the intended physics of the reference, as one vectorised function.

    a_i = sum_{j : |x_j - x_i| >= r_cut} G m_j (x_j - x_i) / |x_j - x_i|^3      (mpi.c:59-73)
    v <- v + a dt ;  x <- x + v dt                                             (mpi.c:206-215)

with every acceleration of a step evaluated from the positions at the start of that step
(synchronous / Jacobi). This is NOT the reference output — cuda.cu overflows in fp32 and
never refreshes its device positions, and mpi.c updates in place — but the physics all three
programs intend. Optional Plummer softening eps: r^2 -> r^2 + eps^2.
"""
from __future__ import annotations

import os

import numpy as np

from ..config import G_SI


def accelerations(pos: np.ndarray, mass: np.ndarray, G: float = G_SI, cutoff: float = 1e-10,
                  softening: float = 0.0, block: int = 256, with_potential: bool = False,
                  with_abs: bool = False):
    """Direct-sum accelerations (n, 3) in fp64; optionally the potential phi (n,) too.

    with_abs also returns sum_j |term_ij| per component (n, 3): the scale against which a
    floating-point sum of the terms should be judged (error <= c * eps * sum |terms|)."""
    pos = np.asarray(pos, dtype=np.float64)
    mu = G * np.asarray(mass, dtype=np.float64)
    n = pos.shape[0]
    acc = np.zeros((n, 3))
    absacc = np.zeros((n, 3))
    phi = np.zeros(n)
    cut2 = cutoff * cutoff
    eps2 = softening * softening

    def rows(i0: int) -> None:
        i1 = min(n, i0 + block)
        d = pos[None, :, :] - pos[i0:i1, None, :]            # (b, n, 3)  x_j - x_i
        r2 = (d * d).sum(-1) + eps2
        ok = r2 >= cut2
        inv = np.zeros_like(r2)
        inv[ok] = 1.0 / np.sqrt(r2[ok])
        mi = mu[None, :] * inv
        s = mi * inv * inv
        acc[i0:i1] = (s[:, :, None] * d).sum(1)
        if with_abs:
            absacc[i0:i1] = (s[:, :, None] * np.abs(d)).sum(1)
        phi[i0:i1] = -mi.sum(1)

    starts = range(0, n, block)
    if n * n >= 1 << 24 and len(starts) > 1:
        # Row blocks are independent (each writes its own rows; same bits in any order) and
        # NumPy releases the GIL inside these array operations: a few threads cut the
        # oracle's wall time on the large reference sums the tests use.
        from concurrent.futures import ThreadPoolExecutor

        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
            list(ex.map(rows, starts))
    else:
        for i0 in starts:
            rows(i0)
    out = (acc,)
    if with_potential:
        out += (phi,)
    if with_abs:
        out += (absacc,)
    return out if len(out) > 1 else acc


def _source_columns(mass, sources):
    """The j bodies of a sum: all (None), or the index array `sources` when every body outside it
    has mass exactly 0 (such a pair adds exactly zero to a, j and phi, so leaving it out changes
    no term of the sum, only the cost)."""
    if sources is None:
        return slice(None)
    src = np.asarray(sources, dtype=np.int64).ravel()
    n = len(mass)
    if src.size and (src.min() < 0 or src.max() >= n):
        raise ValueError("sources: index out of range")
    rest = np.ones(n, dtype=bool)
    rest[src] = False
    if np.any(np.asarray(mass)[rest] != 0):
        raise ValueError("sources: a body outside them has mass")
    return src


def acc_jerk(pos, vel, mass, G: float = G_SI, cutoff: float = 1e-10, softening: float = 0.0,
             block: int = 256, with_potential: bool = False, with_abs: bool = False,
             sources=None):
    """Direct-sum accelerations and jerks (n, 3) in fp64; optionally phi (n,) too.

        a_i = sum_j mu_j d / r^3,  j_i = sum_j mu_j (w - 3 (d.w) d / r^2) / r^3,
        d = x_j - x_i, w = v_j - v_i, r^2 = |d|^2 + eps^2, mu = G m,

    a pair contributing zero to all three when r^2 < cutoff^2 (the pair law of
    accelerations()). with_abs also returns the rounding scales (n, 3) of both sums:
    sum_j |a term| and, per component c,
    sum_j mu_j r^-3 (|w_c| + 3 (sum_k |d_k w_k|) |d_c| / r^2).
    sources: the only bodies with mass (_source_columns); the sums run over them alone."""
    pos = np.asarray(pos, dtype=np.float64)
    vel = np.asarray(vel, dtype=np.float64)
    mu = G * np.asarray(mass, dtype=np.float64)
    n = pos.shape[0]
    cols = _source_columns(mu, sources)
    pos_j, vel_j, mu = pos[cols], vel[cols], mu[cols]
    if sources is not None:  # (rows x sources stays a few MB however many rows there are)
        block = max(block, 65536 // max(1, len(mu)))
    acc, jerk = np.zeros((n, 3)), np.zeros((n, 3))
    absacc, absjerk = np.zeros((n, 3)), np.zeros((n, 3))
    phi = np.zeros(n)
    cut2 = cutoff * cutoff
    eps2 = softening * softening
    def rows(i0: int) -> None:
        i1 = min(n, i0 + block)
        d = pos_j[None, :, :] - pos[i0:i1, None, :]          # (b, n, 3)  x_j - x_i
        w = vel_j[None, :, :] - vel[i0:i1, None, :]
        r2 = (d * d).sum(-1) + eps2
        ok = r2 >= cut2
        inv = np.zeros_like(r2)
        inv[ok] = 1.0 / np.sqrt(r2[ok])
        inv2 = inv * inv
        mi = mu[None, :] * inv
        s = mi * inv2
        al = 3.0 * (d * w).sum(-1) * inv2
        acc[i0:i1] = (s[:, :, None] * d).sum(1)
        jerk[i0:i1] = (s[:, :, None] * (w - al[:, :, None] * d)).sum(1)
        phi[i0:i1] = -mi.sum(1)
        if with_abs:
            absacc[i0:i1] = (s[:, :, None] * np.abs(d)).sum(1)
            aal = 3.0 * np.abs(d * w).sum(-1) * inv2
            absjerk[i0:i1] = (s[:, :, None] * (np.abs(w) + aal[:, :, None] * np.abs(d))).sum(1)

    starts = range(0, n, block)
    if n * len(mu) >= 1 << 22 and len(starts) > 1:
        # (independent row blocks on a few threads, as in accelerations())
        from concurrent.futures import ThreadPoolExecutor

        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
            list(ex.map(rows, starts))
    else:
        for i0 in starts:
            rows(i0)
    out = (acc, jerk)
    if with_potential:
        out += (phi,)
    if with_abs:
        out += (absacc, absjerk)
    return out


# ---- k nearest neighbours, local density and cluster structure -------------------------------
def k_nearest(pos, k: int = 6, block: int = 256):
    """The k nearest neighbours of every body in fp64: (r2 (n, k), idx (n, k) int32), the first k
    entries of the ascending lexicographic order on (r^2_ij, j) over j != i. The body itself is
    left out by index, not by distance: another body at the same position is a neighbour at
    r^2 = 0. No softening, no cutoff. Entries past the n - 1 neighbours there are: (+inf, -1)."""
    pos = np.asarray(pos, dtype=np.float64)
    n, k = pos.shape[0], int(k)
    if k < 1:
        raise ValueError("k must be >= 1")
    r2 = np.full((n, k), np.inf)
    idx = np.full((n, k), -1, dtype=np.int32)
    m = min(k, n - 1)
    jj = np.arange(n)
    for b0 in range(0, n if m > 0 else 0, block):
        rows = np.arange(b0, min(b0 + block, n))
        d = pos[None, :, :] - pos[rows, None, :]
        rr = (d * d).sum(-1)
        rr[np.arange(len(rows)), rows] = np.inf  # (after every real pair, whatever its j)
        order = np.lexsort((np.broadcast_to(jj, rr.shape), rr), axis=1)[:, :m]
        r2[rows, :m] = np.take_along_axis(rr, order, 1)
        idx[rows, :m] = order
    return r2, idx


def density_from_lists(r2, idx, mass, k: int = 6):
    """Casertano & Hut (1985) local density from k-nearest lists (at least k columns):
    rho_i = (sum of the masses of the k - 1 nearest) / (4/3 pi r_k^3), r_k the k-th distance.
    Returns (rho (n,), degenerate (n,) bool): a body with r_k = 0 or fewer than k neighbours has
    no density (rho 0, flagged)."""
    r2, idx = np.asarray(r2, dtype=np.float64), np.asarray(idx)
    mass, k = np.asarray(mass, dtype=np.float64), int(k)
    if k < 2 or r2.shape[1] < k:
        raise ValueError("the local density needs k >= 2 and lists of at least k columns")
    rk2 = r2[:, k - 1]
    bad = (idx[:, k - 1] < 0) | ~np.isfinite(rk2) | (rk2 <= 0)
    inner = np.where(idx[:, :k - 1] >= 0, mass[np.clip(idx[:, :k - 1], 0, None)], 0.0).sum(1)
    rk = np.sqrt(np.where(bad, 1.0, rk2))
    rho = np.where(bad, 0.0, inner / (4.0 / 3.0 * np.pi * rk ** 3))
    return rho, bad


def local_density(pos, mass, k: int = 6):
    """rho_i of density_from_lists on the fp64 lists of k_nearest (nan where undefined)."""
    rho, bad = density_from_lists(*k_nearest(pos, k), mass, k)
    return np.where(bad, np.nan, rho)


def cluster_structure(pos, mass, k: int = 6, fractions=(0.1, 0.5, 0.9), lists=None):
    """Structure read-outs of a cluster (Casertano & Hut 1985), all fp64:
      density_centre    x_d = sum rho_i x_i / sum rho_i
      core_radius       sqrt(sum rho_i^2 |x_i - x_d|^2 / sum rho_i^2)
      density_max       max rho_i
      lagrangian_radii  per fraction f, the radius about x_d of the first body (by radius) at
                        which the cumulative mass fraction reaches f
      degenerate        bodies without a density (r_k = 0, or fewer than k neighbours): left
                        out of the weighted sums (not of the cumulative mass)
    lists: (r2, idx) of k_nearest from another device (default: the oracle's own). When no body
    has a density the centre is the centre of mass and core_radius, density_max are 0."""
    pos = np.asarray(pos, dtype=np.float64)
    mass = np.asarray(mass, dtype=np.float64)
    r2, idx = k_nearest(pos, k) if lists is None else lists
    rho, bad = density_from_lists(r2, idx, mass, k)
    w = rho.sum()
    if w > 0:
        xd = (rho[:, None] * pos).sum(0) / w
    else:
        xd = (mass[:, None] * pos).sum(0) / mass.sum() if mass.sum() > 0 else pos.mean(0)
    rad2 = ((pos - xd) ** 2).sum(1)
    w2 = (rho * rho).sum()
    order = np.argsort(rad2, kind="stable")
    cum = np.cumsum(mass[order])
    lag = []
    for f in fractions:
        at = int(np.searchsorted(cum, f * cum[-1], side="left")) if cum[-1] > 0 else 0
        lag.append(float(np.sqrt(rad2[order[min(at, len(order) - 1)]])))
    return {"density_centre": [float(c) for c in xd],
            "core_radius": float(np.sqrt((rho * rho * rad2).sum() / w2)) if w2 > 0 else 0.0,
            "density_max": float(rho.max()) if len(rho) else 0.0,
            "lagrangian_radii": lag, "degenerate": int(bad.sum())}


# ---- nearest neighbours, overlaps and mergers ------------------------------------------------
def nearest_neighbours(pos, radius, cutoff: float = 1e-10, softening: float = 0.0, rows=None,
                       block: int = 256, second: bool = False):
    """Nearest neighbour of every body (or of the bodies `rows`) by the pair measure

        q_ij = r^2_ij - (R_i + R_j)^2,    r^2 = |x_j - x_i|^2 + softening^2,

    in fp64: (q (m,), nn (m,) int32), the j of the smallest q, the lowest j on an exact tie,
    (+inf, -1) where there is none. Every body takes part, massless ones too; a pair the pair
    law zeroes (r^2 < cutoff^2: the self term, coincident bodies) does not. Body i overlaps its
    neighbour when q_i < softening^2, that is |d|^2 < (R_i + R_j)^2. radius None: zeros (the
    nearest body by distance). second: also the second smallest q (m,) (+inf when none)."""
    pos = np.asarray(pos, dtype=np.float64)
    n = pos.shape[0]
    R = np.zeros(n) if radius is None else np.asarray(radius, dtype=np.float64)
    idx = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    q, nn = np.full(len(idx), np.inf), np.full(len(idx), -1, dtype=np.int32)
    q2 = np.full(len(idx), np.inf)
    cut2, eps2 = cutoff * cutoff, softening * softening
    for b0 in range(0, len(idx), block):
        r = idx[b0:b0 + block]
        d = pos[None, :, :] - pos[r, None, :]
        r2 = (d * d).sum(-1) + eps2
        sr = R[None, :] + R[r, None]
        qq = np.where(r2 >= cut2, r2 - sr * sr, np.inf)
        qq[np.arange(len(r)), r] = np.inf  # (j != i: with softening the law keeps the self pair)
        k = qq.argmin(1)  # (the first of equal minima: the lowest j)
        best = qq[np.arange(len(r)), k]
        q[b0:b0 + block] = best
        nn[b0:b0 + block] = np.where(np.isfinite(best), k, -1)
        if second and n > 1:
            qq[np.arange(len(r)), k] = np.inf
            q2[b0:b0 + block] = qq.min(1)
    return (q, nn, q2) if second else (q, nn)


def overlap_components(ca_q, ca_nn, softening: float = 0.0, eps2=None):
    """Connected components of the pairs (i, ca_nn_i) with ca_q_i < softening^2: a label per
    body, the lowest index of its component (its own where it overlaps nobody). eps2: the
    threshold itself (an engine's softening^2 as its pair type rounds it)."""
    ca_q, ca_nn = np.asarray(ca_q, dtype=np.float64), np.asarray(ca_nn, dtype=np.int64)
    n = len(ca_q)
    root = np.arange(n)

    def find(i):
        while root[i] != i:
            root[i] = root[root[i]]
            i = root[i]
        return i

    eps2 = softening * softening if eps2 is None else float(eps2)
    for i in np.nonzero((ca_q < eps2) & (ca_nn >= 0))[0]:
        a, b = find(int(i)), find(int(ca_nn[i]))
        if a != b:
            root[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)], dtype=np.int64)


def merge_overlaps(pos, vel, mass, radius, ids, ca_q, ca_nn, softening: float = 0.0, eps2=None):
    """Perfect mergers at a synchronised state: every component of overlap_components() becomes
    one body at the place of its lowest index, with that body's id, mass sum m, the position and
    velocity of the centre of mass (the plain mean where the component is massless) and
    R = (sum R^3)^(1/3); the absorbed bodies are removed and the order of the rest stays. Mass
    and linear momentum are conserved to rounding. Returns (pos, vel, mass, radius, ids,
    mergers), mergers the number of bodies absorbed."""
    pos, vel = np.asarray(pos, dtype=np.float64), np.asarray(vel, dtype=np.float64)
    mass, radius = np.asarray(mass, dtype=np.float64), np.asarray(radius, dtype=np.float64)
    ids = np.asarray(ids, dtype=np.int64)
    label = overlap_components(ca_q, ca_nn, softening, eps2)
    keep = label == np.arange(len(label))
    p, v, m, R = pos.copy(), vel.copy(), mass.copy(), radius.copy()
    for root in np.nonzero(keep & (np.bincount(label, minlength=len(label)) > 1))[0]:
        mem = np.nonzero(label == root)[0]
        mt = mass[mem].sum()
        w = mass[mem] / mt if mt > 0 else np.full(len(mem), 1.0 / len(mem))
        p[root] = (w[:, None] * pos[mem]).sum(0)
        v[root] = (w[:, None] * vel[mem]).sum(0)
        m[root] = mt
        R[root] = np.cbrt((radius[mem] ** 3).sum())
    return p[keep], v[keep], m[keep], R[keep], ids[keep], int((~keep).sum())


class _Closest:
    """The closest-approach record of the engines: min of q per body and the neighbour then,
    the latest (q, nn), and the number of (body, evaluation) overlaps seen."""

    def __init__(self, n, radius, cutoff, softening):
        self.R = np.zeros(n) if radius is None else np.asarray(radius, dtype=np.float64)
        self.cutoff, self.softening = cutoff, softening
        self.q, self.nn = np.full(n, np.inf), np.full(n, -1, dtype=np.int32)
        self.ca_q, self.ca_nn = np.full(n, np.inf), np.full(n, -1, dtype=np.int32)
        self.overlaps = 0

    def see(self, xp, rows=None):
        q, nn = nearest_neighbours(xp, self.R, self.cutoff, self.softening, rows)
        r = slice(None) if rows is None else rows
        self.q[r], self.nn[r] = q, nn
        less = q < self.ca_q[r]
        self.ca_q[r] = np.where(less, q, self.ca_q[r])
        self.ca_nn[r] = np.where(less, nn, self.ca_nn[r])
        hit = int((q < self.softening * self.softening).sum())
        self.overlaps += hit
        return hit

    def export(self, out):
        out.update(q=self.q.copy(), nn=self.nn.copy(), ca_q=self.ca_q.copy(),
                   ca_nn=self.ca_nn.copy(), overlaps=self.overlaps)


def hermite_dt(a0, j0, a1, j1, h, eta):
    """Aarseth's criterion after a Hermite step of size h from (a0, j0) to (a1, j1):
    min over the bodies of sqrt(eta (|a1||a2'| + |j1|^2) / (|j1||a3| + |a2'|^2)) with the 2nd
    and 3rd derivatives the two evaluations imply; bodies with |j1| = 0 or a non-finite ratio
    are skipped (inf when none is left)."""
    da = a0 - a1
    a2 = (-6.0 * da - h * (4.0 * j0 + 2.0 * j1)) / h ** 2
    a3 = (12.0 * da + 6.0 * h * (j0 + j1)) / h ** 3
    a2p = a2 + h * a3
    nrm = lambda y: np.sqrt((y * y).sum(1))  # noqa: E731
    an, jn, n2, n3 = nrm(a1), nrm(j1), nrm(a2p), nrm(a3)
    with np.errstate(divide="ignore", invalid="ignore"):
        dt = np.sqrt(eta * (an * n2 + jn * jn) / (jn * n3 + n2 * n2))
    dt = dt[(jn > 0) & np.isfinite(dt)]
    return float(dt.min()) if dt.size else float("inf")


def hermite_first_dt(a, j, eta):
    """(eta / 2) min |a| / |j| over the bodies with |j| > 0 and a finite ratio."""
    an, jn = np.sqrt((a * a).sum(1)), np.sqrt((j * j).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        dt = 0.5 * eta * an / jn
    dt = dt[(jn > 0) & np.isfinite(dt)]
    return float(dt.min()) if dt.size else float("inf")


def simulate_hermite(pos, vel, mass, dt, steps, G=G_SI, cutoff=1e-10, softening=0.0, eta=0.0,
                     t_end=None, record_every=0, radius=None, collisions="off", record=None):
    """4th-order Hermite predictor-corrector (Makino & Aarseth 1992), one evaluation per step at
    the predicted state. eta > 0: one shared step h = min(dt, min_i dt_i) chosen each step
    (hermite_dt; the first from hermite_first_dt); t_end: the step is cut to reach it exactly and
    the run stops there (`steps` caps the count). Returns (pos, vel, traj, t, list of steps).

    collisions "detect" | "merge" (radius: per body, None zeros): every evaluation (the one the
    run starts with, then each step's at the predicted state) also gives each body's nearest
    neighbour (nearest_neighbours); `record` (a dict) receives the latest q and nn, the
    closest-approach record ca_q, ca_nn and the overlap count. "merge": the run takes no further
    step once an evaluation has seen an overlap (merging itself is merge_overlaps, the
    caller's)."""
    if collisions not in ("off", "detect", "merge"):
        raise ValueError("collisions must be off, detect or merge")
    x = np.array(pos, dtype=np.float64, copy=True)
    v = np.array(vel, dtype=np.float64, copy=True)
    a, j = acc_jerk(x, v, mass, G, cutoff, softening)
    near = None if collisions == "off" else _Closest(len(x), radius, cutoff, softening)
    if near is not None:
        near.see(x)
    t, taken, traj = 0.0, [], []
    nxt = hermite_first_dt(a, j, eta) if eta > 0 else dt
    while len(taken) < steps and (t_end is None or t < t_end):
        if collisions == "merge" and near.overlaps:
            break
        h = min(dt, nxt)
        cut = t_end is not None and h >= t_end - t
        if cut:
            h = t_end - t
        xp = x + (v * h + (a * (h * h / 2) + j * (h * h * h / 6)))
        vp = v + (a * h + j * (h * h / 2))
        a1, j1 = acc_jerk(xp, vp, mass, G, cutoff, softening)
        if near is not None:
            near.see(xp)
        v1 = v + ((a + a1) * (h / 2) + (j - j1) * (h * h / 12))
        x = x + ((v + v1) * (h / 2) + (a - a1) * (h * h / 12))
        if eta > 0:
            nxt = hermite_dt(a, j, a1, j1, h, eta)
        v, a, j = v1, a1, j1
        t = t_end if cut else t + h
        taken.append(h)
        if record_every and len(taken) % record_every == 0:
            traj.append(x.copy())
    if near is not None and record is not None:
        near.export(record)
    return x, v, traj, t, taken


# ---- 6th-order Hermite (Nitadori & Makino 2008) -----------------------------------------------
def acc_jerk_snap(pos, vel, acc_in, mass, G: float = G_SI, cutoff: float = 1e-10,
                  softening: float = 0.0, block: int = 256, with_potential: bool = False,
                  with_abs: bool = False):
    """Direct-sum accelerations, jerks and snaps (n, 3) in fp64; optionally phi (n,) too.

        A_ij = mu_j d / r^3,  J_ij = mu_j w / r^3 - 3 alpha A_ij,
        S_ij = mu_j q / r^3 - 6 alpha J_ij - 3 beta A_ij,
        d = x_j - x_i, w = v_j - v_i, q = acc_in_j - acc_in_i, r^2 = |d|^2 + eps^2,
        alpha = (d.w) / r^2,  beta = (|w|^2 + d.q) / r^2 + alpha^2,

    a pair contributing zero to all when r^2 < cutoff^2. acc_in is the acceleration the snap is
    taken at (the snap of a state is acc_jerk_snap(x, v, a(x), ...)). with_abs also returns the
    rounding scales (n, 3) of the three sums: those of acc_jerk and, per component c of the snap,
    sum_j mu_j r^-3 [|q_c| + 6 al (|w_c| + 3 al |d_c|) + 3 be |d_c|] with
    al = sum_k |d_k w_k| / r^2 and be = (sum_k w_k^2 + sum_k |d_k q_k|) / r^2 + al^2."""
    pos = np.asarray(pos, dtype=np.float64)
    vel = np.asarray(vel, dtype=np.float64)
    ain = np.asarray(acc_in, dtype=np.float64)
    mu = G * np.asarray(mass, dtype=np.float64)
    n = pos.shape[0]
    acc, jerk, snap = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    absacc, absjerk, abssnap = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    phi = np.zeros(n)
    cut2 = cutoff * cutoff
    eps2 = softening * softening

    def rows(i0: int) -> None:
        i1 = min(n, i0 + block)
        d = pos[None, :, :] - pos[i0:i1, None, :]            # (b, n, 3)  x_j - x_i
        w = vel[None, :, :] - vel[i0:i1, None, :]
        q = ain[None, :, :] - ain[i0:i1, None, :]
        r2 = (d * d).sum(-1) + eps2
        ok = r2 >= cut2
        inv = np.zeros_like(r2)
        inv[ok] = 1.0 / np.sqrt(r2[ok])
        inv2 = inv * inv
        mi = mu[None, :] * inv
        s = (mi * inv2)[:, :, None]
        al = ((d * w).sum(-1) * inv2)[:, :, None]
        be = (((w * w).sum(-1) + (d * q).sum(-1)) * inv2)[:, :, None] + al * al
        A = s * d
        Jt = s * w - 3.0 * al * A
        acc[i0:i1] = A.sum(1)
        jerk[i0:i1] = Jt.sum(1)
        snap[i0:i1] = (s * q - 6.0 * al * Jt - 3.0 * be * A).sum(1)
        phi[i0:i1] = -mi.sum(1)
        if with_abs:
            ad, aw = np.abs(d), np.abs(w)
            aal = (np.abs(d * w).sum(-1) * inv2)[:, :, None]
            abe = (((w * w).sum(-1) + np.abs(d * q).sum(-1)) * inv2)[:, :, None] + aal * aal
            absacc[i0:i1] = (s * ad).sum(1)
            absjerk[i0:i1] = (s * (aw + 3.0 * aal * ad)).sum(1)
            abssnap[i0:i1] = (s * (np.abs(q) + 6.0 * aal * (aw + 3.0 * aal * ad)
                                   + 3.0 * abe * ad)).sum(1)

    starts = range(0, n, block)
    if n * n >= 1 << 22 and len(starts) > 1:
        # (independent row blocks on a few threads, as in accelerations())
        from concurrent.futures import ThreadPoolExecutor

        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
            list(ex.map(rows, starts))
    else:
        for i0 in starts:
            rows(i0)
    out = (acc, jerk, snap)
    if with_potential:
        out += (phi,)
    if with_abs:
        out += (absacc, absjerk, abssnap)
    return out


def hermite6_high(a0, j0, s0, a1, j1, s1, h):
    """The 3rd, 4th and 5th derivatives of a at t1 = t0 + h of the quintic that takes
    (a0, j0, s0) at t0 and (a1, j1, s1) at t1: (c1, p1, a5), a5 being constant over the step.
    h a scalar, or one value per row."""
    h = np.asarray(h, dtype=np.float64)
    hp = 0.5 * (h[:, None] if h.ndim else h)
    hp2 = hp * hp
    Am, Jm, Jp = a1 - a0, hp * (j1 - j0), hp * (j1 + j0)
    Sm, Sp = hp2 * (s1 - s0), hp2 * (s1 + s0)
    ih = 1.0 / hp
    ih3 = ih * ih * ih
    ih4 = ih3 * ih
    ih5 = ih4 * ih
    a3 = (6.0 * ih3) * (-5.0 * Am + 5.0 * Jp - Sm) / 8.0
    a4 = (24.0 * ih4) * (-Jm + Sp) / 16.0
    a5 = (120.0 * ih5) * (3.0 * Am - 3.0 * Jp + Sm) / 16.0
    return a3 + hp * a4 + hp2 * a5 / 2.0, a4 + hp * a5, a5


def hermite6_dt(a0, j0, s0, a1, j1, s1, h, eta):
    """Nitadori & Makino's criterion after a 6th-order step of size h: min over the bodies of
    eta ((|a1||s1| + |j1|^2) / (|c1||a5| + |p1|^2))^(1/6) with the higher derivatives of
    hermite6_high (eta enters linearly: useful values are 0.2 to 0.5); bodies with a zero or
    non-finite ratio are skipped (inf when none is left)."""
    c1, p1, a5 = hermite6_high(a0, j0, s0, a1, j1, s1, h)
    nrm = lambda y: np.sqrt((y * y).sum(1))  # noqa: E731
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = (nrm(a1) * nrm(s1) + nrm(j1) ** 2) / (nrm(c1) * nrm(a5) + nrm(p1) ** 2)
        dt = eta * ratio ** (1.0 / 6.0)
    dt = dt[(ratio > 0) & np.isfinite(dt)]
    return float(dt.min()) if dt.size else float("inf")


def hermite6_start(pos, vel, mass, G=G_SI, cutoff=1e-10, softening=0.0):
    """a, j, s of a state in the two passes a 6th-order run starts with: the first with
    acc_in = 0 gives a and j, the second with acc_in = a gives s."""
    a, _, _ = acc_jerk_snap(pos, vel, np.zeros_like(np.asarray(pos, dtype=np.float64)), mass, G,
                            cutoff, softening)
    return acc_jerk_snap(pos, vel, a, mass, G, cutoff, softening)


def simulate_hermite6(pos, vel, mass, dt, steps, G=G_SI, cutoff=1e-10, softening=0.0, eta=0.0,
                      t_end=None, record_every=0):
    """6th-order Hermite predictor-corrector (Nitadori & Makino 2008), one evaluation per step
    at the predicted (x, v, a); the state carries a, j, s and the crackle c (0 at the start).
    eta > 0: one shared step h = min(dt, min_i dt_i) chosen each step (hermite6_dt; the first from
    hermite_first_dt); t_end: the step is cut to reach it exactly and the run stops there
    (`steps` caps the count). Returns (pos, vel, traj, t, list of steps), as simulate_hermite."""
    x = np.array(pos, dtype=np.float64, copy=True)
    v = np.array(vel, dtype=np.float64, copy=True)
    a, j, s = hermite6_start(x, v, mass, G, cutoff, softening)
    c = np.zeros_like(a)
    t, taken, traj = 0.0, [], []
    nxt = hermite_first_dt(a, j, eta) if eta > 0 else dt
    while len(taken) < steps and (t_end is None or t < t_end):
        h = min(dt, nxt)
        cut = t_end is not None and h >= t_end - t
        if cut:
            h = t_end - t
        h2, h3, h4, h5 = (h * h) / 2, (h * h * h) / 6, (h * h * h * h) / 24, \
            (h * h * h * h * h) / 120
        xp = x + (v * h + (a * h2 + (j * h3 + (s * h4 + c * h5))))
        vp = v + (a * h + (j * h2 + (s * h3 + c * h4)))
        ap = a + (j * h + (s * h2 + c * h3))
        a1, j1, s1 = acc_jerk_snap(xp, vp, ap, mass, G, cutoff, softening)
        hh, h10, h120 = h / 2, (h * h) / 10, (h * h * h) / 120
        v1 = v + ((a + a1) * hh + ((j - j1) * h10 + (s + s1) * h120))
        x = x + ((v + v1) * hh + ((a - a1) * h10 + (j + j1) * h120))
        if eta > 0:
            nxt = hermite6_dt(a, j, s, a1, j1, s1, h, eta)
        c = hermite6_high(a, j, s, a1, j1, s1, h)[0]
        v, a, j, s = v1, a1, j1, s1
        t = t_end if cut else t + h
        taken.append(h)
        if record_every and len(taken) % record_every == 0:
            traj.append(x.copy())
    return x, v, traj, t, taken


def step(pos, vel, mass, dt, G=G_SI, cutoff=1e-10, softening=0.0):
    """One synchronous kick-drift step; returns new (pos, vel)."""
    a = accelerations(pos, mass, G, cutoff, softening)
    v = vel + a * dt
    x = pos + v * dt
    return x, v


def simulate(pos, vel, mass, dt, steps, G=G_SI, cutoff=1e-10, softening=0.0, record_every=0,
             integrator="kd", eta=0.0, t_end=None):
    """Run `steps` steps. Returns (pos, vel, trajectory list of positions if record_every).

    integrator "leapfrog": kick-drift-kick, v_{1/2} = v_0 + a_0 dt/2, x_1 = x_0 + v_{1/2} dt,
    v_1 = v_{1/2} + a_1 dt/2 (velocities returned synchronized).
    integrator "hermite" (simulate_hermite; eta, t_end): also returns the time reached and the
    list of steps taken: (pos, vel, traj, t, steps)."""
    if integrator == "hermite":
        return simulate_hermite(pos, vel, mass, dt, steps, G, cutoff, softening, eta, t_end,
                                record_every)
    if eta or t_end is not None:
        raise ValueError("eta and t_end belong to integrator hermite")
    x = np.array(pos, dtype=np.float64, copy=True)
    v = np.array(vel, dtype=np.float64, copy=True)
    traj = []
    if integrator == "leapfrog":
        a = accelerations(x, mass, G, cutoff, softening)
        for s in range(steps):
            v = v + 0.5 * dt * a
            x = x + v * dt
            a = accelerations(x, mass, G, cutoff, softening)
            v = v + 0.5 * dt * a
            if record_every and (s + 1) % record_every == 0:
                traj.append(x.copy())
        return x, v, traj
    for s in range(steps):
        x, v = step(x, v, mass, dt, G, cutoff, softening)
        if record_every and (s + 1) % record_every == 0:
            traj.append(x.copy())
    return x, v, traj


def gauss_seidel_step(pos, vel, mass, dt, nranks, G=G_SI, cutoff=1e-10):
    """Emulation of mpi.c's in-place update inside each rank's block (mpi.c:196-216, D6).

    Kept only to document the defect in tests: results depend on `nranks`.
    """
    x = np.array(pos, dtype=np.float64, copy=True)
    v = np.array(vel, dtype=np.float64, copy=True)
    n = x.shape[0]
    base, rem = divmod(n, nranks)
    snapshot = x.copy()  # what other ranks hold until the Allgatherv
    new_x = x.copy()
    for r in range(nranks):
        start = r * base + min(r, rem)
        cnt = base + (1 if r < rem else 0)
        local = snapshot.copy()
        for i in range(start, start + cnt):
            d = local - local[i]
            r2 = (d * d).sum(1)
            ok = r2 >= cutoff * cutoff
            ok[i] = False
            inv = np.zeros(n)
            inv[ok] = 1.0 / np.sqrt(r2[ok])
            a = ((G * mass * inv ** 3)[:, None] * d).sum(0)
            v[i] = v[i] + a * dt
            local[i] = local[i] + v[i] * dt
            new_x[i] = local[i]
    return new_x, v


# ---- Hermite with individual block time steps ------------------------------------------------
def acc_jerk_rows(pos, vel, mass, idx, G: float = G_SI, cutoff: float = 1e-10,
                  softening: float = 0.0, sources=None):
    """acc_jerk() of the bodies `idx` only, against all bodies: (len(idx), 3) each.
    sources: the only bodies with mass (_source_columns); the sums run over them alone, so a
    set of a few massive bodies and many massless test particles costs len(idx) x len(sources)."""
    pos = np.asarray(pos, dtype=np.float64)
    vel = np.asarray(vel, dtype=np.float64)
    mu = G * np.asarray(mass, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    cols = _source_columns(mu, sources)
    pos_j, vel_j, mu = pos[cols], vel[cols], mu[cols]
    blk = 256 if sources is None else max(256, 65536 // max(1, len(mu)))
    acc, jerk = np.zeros((len(idx), 3)), np.zeros((len(idx), 3))
    for b0 in range(0, len(idx), blk):
        rows = idx[b0:b0 + blk]
        d = pos_j[None, :, :] - pos[rows, None, :]
        w = vel_j[None, :, :] - vel[rows, None, :]
        r2 = (d * d).sum(-1) + softening * softening
        ok = r2 >= cutoff * cutoff
        inv = np.zeros_like(r2)
        inv[ok] = 1.0 / np.sqrt(r2[ok])
        inv2 = inv * inv
        s = mu[None, :] * inv * inv2
        al = 3.0 * (d * w).sum(-1) * inv2
        acc[b0:b0 + blk] = (s[:, :, None] * d).sum(1)
        jerk[b0:b0 + blk] = (s[:, :, None] * (w - al[:, :, None] * d)).sum(1)
    return acc, jerk


def hermite_dt_bodies(a0, j0, a1, j1, h, eta):
    """hermite_dt()'s criterion per body, h (m,) each body's own step: (dt_want, valid) with
    valid False where |j1| = 0 or the ratio is not finite."""
    h = np.asarray(h, dtype=np.float64)[:, None]
    da = a0 - a1
    with np.errstate(divide="ignore", invalid="ignore"):
        a2 = (-6.0 * da - h * (4.0 * j0 + 2.0 * j1)) / h ** 2
        a3 = (12.0 * da + 6.0 * h * (j0 + j1)) / h ** 3
        a2p = a2 + h * a3
        nrm = lambda y: np.sqrt((y * y).sum(1))  # noqa: E731
        an, jn, n2, n3 = nrm(a1), nrm(j1), nrm(a2p), nrm(a3)
        dt = np.sqrt(eta * (an * n2 + jn * jn) / (jn * n3 + n2 * n2))
    return dt, (jn > 0) & np.isfinite(dt)


def block_first_levels(a, j, dt, eta, max_level):
    """Starting level per body: the smallest k with dt 2^-k <= (eta / 2) |a| / |j|, capped at
    max_level; level 0 where |j| = 0 or the ratio is not finite."""
    an, jn = np.sqrt((a * a).sum(1)), np.sqrt((j * j).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        want = 0.5 * eta * an / jn
    ok = (jn > 0) & np.isfinite(want)
    lev = np.zeros(len(an), dtype=np.int32)
    want = np.where(ok, want, np.inf)
    for k in range(max_level):  # (every body at once: one more halving where it is still wanted)
        more = (lev == k) & (np.ldexp(dt, -k) > want)
        if not more.any():
            break
        lev[more] = k + 1
    return lev


def block_new_level(k, dt_want, valid, t_next, dt, max_level):
    """The level rule of one active body after its step to t_next (ticks): (new k, clamped)."""
    if not valid:
        return k, False
    if dt_want < np.ldexp(dt, -k):
        while k < max_level and np.ldexp(dt, -k) > dt_want:
            k += 1
        return k, bool(np.ldexp(dt, -k) > dt_want)
    if k > 0 and dt_want >= 2.0 * np.ldexp(dt, -k) and t_next % (1 << (max_level - k + 1)) == 0:
        return k - 1, False
    return k, False


def block_new_levels(k, dt_want, valid, t_next, dt, max_level):
    """block_new_level() of many active bodies at once (the same comparisons on arrays):
    (new levels int32, clamped bool)."""
    k = np.asarray(k, dtype=np.int32)
    valid = np.asarray(valid, dtype=bool)
    want = np.where(valid, np.asarray(dt_want, dtype=np.float64), np.inf)
    dtk = np.ldexp(dt, -k)
    down = valid & (want < dtk)
    new = k.copy()
    while True:
        more = down & (new < max_level) & (np.ldexp(dt, -new) > want)
        if not more.any():
            break
        new[more] += 1
    clamped = down & (np.ldexp(dt, -new) > want)
    span = np.int64(1) << (max_level - k.astype(np.int64) + 1)
    up = valid & ~down & (k > 0) & (want >= 2.0 * dtk) & (t_next % span == 0)
    new[up] -= 1
    return new, clamped


def level_lean(dt_want, valid, dt):
    """How near a level decision came to going the other way: min over the valid bodies of
    |log2(dt / dt_want) - nearest integer| (every threshold of the level rules is dt_want against
    dt 2^-k for a whole k); inf when no body is valid."""
    valid = np.asarray(valid, dtype=bool)
    if not valid.any():
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.log2(dt / np.asarray(dt_want, dtype=np.float64)[valid])
    e = e[np.isfinite(e)]  # (dt_want = 0: every level is too long, no threshold is near)
    return float(np.abs(e - np.rint(e)).min()) if e.size else float("inf")


def _simulate_block(pos, vel, start, advance, dt, t_end, eta, max_level, check, levels,
                    body_times, stats):
    """The block schedule of both orders: the checks, the block state, the due set, the level
    rule, the log and the stats. The order's own part is two callables: start(x, v) evaluates
    the state and returns the carried rows, a and j first; advance(x, v, rows, act, h) takes the
    due bodies `act` over the steps h (n,) from every body's own time (predict, evaluate their
    rows, correct, write the state) and returns (dt_want, valid) of each."""
    if not eta > 0:
        raise ValueError("block steps need eta > 0")
    L = int(max_level)
    if not 0 <= L <= 40:
        raise ValueError("max_level must be in 0..40")
    macro = int(round(t_end / dt))
    if macro * dt != t_end:
        raise ValueError("t_end must be a whole multiple of dt")
    x = np.array(pos, dtype=np.float64, copy=True)
    v = np.array(vel, dtype=np.float64, copy=True)
    n = x.shape[0]
    rows = start(x, v)
    a, j = rows[:2]
    tb = (np.zeros(n, dtype=np.int64) if body_times is None else
          np.array(body_times, dtype=np.int64))
    lev = (block_first_levels(a, j, dt, eta, L) if levels is None else
           np.array(levels, dtype=np.int32))
    if lev.shape != (n,) or tb.shape != (n,) or (lev < 0).any() or (lev > L).any() or \
            (tb < 0).any() or (tb % (np.int64(1) << (L - lev).astype(np.int64))).any():
        raise ValueError("block state: level out of 0..max_level, or a body time that is no "
                         "multiple of its step")
    lean = float("inf")
    if stats is not None and levels is None:
        an, jn = np.sqrt((a * a).sum(1)), np.sqrt((j * j).sum(1))
        with np.errstate(divide="ignore", invalid="ignore"):
            first = 0.5 * eta * an / jn
        lean = level_lean(first, (jn > 0) & np.isfinite(first), dt)
    level_max, active = int(lev.max()) if n else 0, []
    end = macro << L
    log, clamped = [], 0
    while tb.min() < end:
        stp = np.int64(1) << (L - lev).astype(np.int64)
        t_next = int((tb + stp).min())
        act = np.nonzero(tb + stp == t_next)[0]
        h = dt * np.ldexp((t_next - tb).astype(np.float64), -L)
        want, valid = advance(x, v, rows, act, h)
        tb[act] = t_next
        lev[act], hit = block_new_levels(lev[act], want, valid, t_next, dt, L)
        clamped += int(hit.sum())
        log.append((t_next, int(len(act))))
        if stats is not None:
            lean = min(lean, level_lean(want, valid, dt))
            level_max = max(level_max, int(lev[act].max()))
            active.append(act)
        if check is not None:
            check(tb, lev)
    if stats is not None:
        stats.update(active=active, lean=lean, level_max=level_max)
    return x, v, lev.copy(), log, clamped


def simulate_hermite_block(pos, vel, mass, dt, t_end, eta, max_level=24, G=G_SI, cutoff=1e-10,
                           softening=0.0, check=None, sources=None, levels=None,
                           body_times=None, stats=None, radius=None, collisions="off",
                           record=None):
    """4th-order Hermite with individual block time steps (Makino 1991): body i steps by
    dt 2^-k_i, time is an integer count of ticks of dt 2^-max_level, only the bodies that are due
    are evaluated (against every body predicted to that time) and corrected. t_end must be a
    whole multiple of dt; every multiple of dt synchronises all bodies. `check(tb, level)` is
    called after every block step. Returns (pos, vel, levels, [(t_ticks, n_active)],
    level_clamped).

    sources: the only bodies with mass (acc_jerk_rows); only the due bodies and the sources are
    then predicted, so a block step costs n_active x len(sources). levels, body_times (ticks):
    the block state to start from (default: block_first_levels, all at 0); a body's time must be
    a multiple of its step. stats: a dict that receives "active" (the index array of every block
    step), "lean" (level_lean over every level decision, the first included) and "level_max".

    collisions "detect" | "merge" (radius per body; not with sources): as simulate_hermite, the
    active bodies of each block step against all bodies predicted to its time; the run never
    stops inside a macro step, `record` carries what happened (merging at the boundary is the
    caller's, merge_overlaps)."""
    if collisions not in ("off", "detect", "merge"):
        raise ValueError("collisions must be off, detect or merge")
    if collisions != "off" and sources is not None:
        raise ValueError("collisions need every body's predicted state (no sources)")
    mass = np.asarray(mass, dtype=np.float64)
    src = None if sources is None else np.unique(_source_columns(mass, sources))
    near = None if collisions == "off" else _Closest(len(mass), radius, cutoff, softening)

    def start(x, v):
        if near is not None:
            near.see(x)
        return acc_jerk(x, v, mass, G, cutoff, softening, sources=src)

    def advance(x, v, rows, act, h):
        a, j = rows
        # the bodies whose predicted state is read: all, or the due ones and the sources
        need = np.arange(len(x)) if src is None else np.union1d(act, src)
        h = h[need]
        hc = h[:, None]
        xn, vn, an_, jn_ = x[need], v[need], a[need], j[need]
        xp = xn + (vn * hc + (an_ * (hc * hc / 2) + jn_ * (hc * hc * hc / 6)))
        vp = vn + (an_ * hc + jn_ * (hc * hc / 2))
        at = np.searchsorted(need, act)  # (the due bodies' rows of the predicted arrays)
        a1, j1 = acc_jerk_rows(xp, vp, mass[need], at, G, cutoff, softening,
                               sources=None if src is None else np.searchsorted(need, src))
        if near is not None:
            near.see(xp, act)
        ha = hc[at]
        a0, j0, v0 = a[act], j[act], v[act]
        v1 = v0 + ((a0 + a1) * (ha / 2) + (j0 - j1) * (ha * ha / 12))
        x[act] = x[act] + ((v0 + v1) * (ha / 2) + (a0 - a1) * (ha * ha / 12))
        v[act], a[act], j[act] = v1, a1, j1
        return hermite_dt_bodies(a0, j0, a1, j1, h[at], eta)

    out = _simulate_block(pos, vel, start, advance, dt, t_end, eta, max_level, check, levels,
                          body_times, stats)
    if near is not None and record is not None:
        near.export(record)
    return out


# ---- 6th-order Hermite with individual block time steps --------------------------------------
def acc_jerk_snap_rows(pos, vel, acc_in, mass, idx, G: float = G_SI, cutoff: float = 1e-10,
                       softening: float = 0.0):
    """acc_jerk_snap() of the bodies `idx` only, against all bodies: (len(idx), 3) each (the
    same terms in the same column order, so the rows are those of the full call bit for bit)."""
    pos = np.asarray(pos, dtype=np.float64)
    vel = np.asarray(vel, dtype=np.float64)
    ain = np.asarray(acc_in, dtype=np.float64)
    mu = G * np.asarray(mass, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    acc, jerk, snap = (np.zeros((len(idx), 3)) for _ in range(3))
    for b0 in range(0, len(idx), 256):
        rows = idx[b0:b0 + 256]
        d = pos[None, :, :] - pos[rows, None, :]
        w = vel[None, :, :] - vel[rows, None, :]
        q = ain[None, :, :] - ain[rows, None, :]
        r2 = (d * d).sum(-1) + softening * softening
        ok = r2 >= cutoff * cutoff
        inv = np.zeros_like(r2)
        inv[ok] = 1.0 / np.sqrt(r2[ok])
        inv2 = inv * inv
        s = (mu[None, :] * inv * inv2)[:, :, None]
        al = ((d * w).sum(-1) * inv2)[:, :, None]
        be = (((w * w).sum(-1) + (d * q).sum(-1)) * inv2)[:, :, None] + al * al
        A = s * d
        Jt = s * w - 3.0 * al * A
        acc[b0:b0 + 256] = A.sum(1)
        jerk[b0:b0 + 256] = Jt.sum(1)
        snap[b0:b0 + 256] = (s * q - 6.0 * al * Jt - 3.0 * be * A).sum(1)
    return acc, jerk, snap


def hermite6_dt_bodies(a0, j0, s0, a1, j1, s1, h, eta):
    """hermite6_dt()'s criterion per body, h (m,) each body's own step: (dt_want, valid) with
    valid False where the ratio is zero or not finite."""
    h = np.asarray(h, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        c1, p1, a5 = hermite6_high(a0, j0, s0, a1, j1, s1, h)
        nrm = lambda y: np.sqrt((y * y).sum(1))  # noqa: E731
        ratio = (nrm(a1) * nrm(s1) + nrm(j1) ** 2) / (nrm(c1) * nrm(a5) + nrm(p1) ** 2)
        dt = eta * ratio ** (1.0 / 6.0)
    return dt, (ratio > 0) & np.isfinite(dt)


def simulate_hermite6_block(pos, vel, mass, dt, t_end, eta, max_level=24, G=G_SI, cutoff=1e-10,
                            softening=0.0, check=None, levels=None, body_times=None, stats=None):
    """6th-order Hermite (simulate_hermite6) with the individual block time steps of
    simulate_hermite_block: body i carries x, v, a, j, s, c, a time in ticks of dt 2^-max_level
    and a level k (step dt 2^-k). A run starts with hermite6_start (c = 0) and the levels of
    block_first_levels, the first-step rule of the shared order-6 run. A block step predicts
    every body from its own time over its own h (x to h^5, v to h^4, a to h^3), evaluates a1, j1,
    s1 of the due bodies against all predicted rows, corrects them over their own h, forms c1 and
    the step each wants (hermite6_dt_bodies) and applies the level rule of order 4
    (block_new_levels). t_end, check, levels, body_times, stats and the return value are those of
    simulate_hermite_block; there are no sources and no collisions."""
    mass = np.asarray(mass, dtype=np.float64)

    def start(x, v):
        a, j, s = hermite6_start(x, v, mass, G, cutoff, softening)
        return a, j, s, np.zeros_like(a)

    def advance(x, v, rows, act, h):
        a, j, s, c = rows
        hc = h[:, None]
        h2, h3, h4, h5 = (hc * hc) / 2, (hc * hc * hc) / 6, (hc * hc * hc * hc) / 24, \
            (hc * hc * hc * hc * hc) / 120
        xp = x + (v * hc + (a * h2 + (j * h3 + (s * h4 + c * h5))))
        vp = v + (a * hc + (j * h2 + (s * h3 + c * h4)))
        ap = a + (j * hc + (s * h2 + c * h3))
        a1, j1, s1 = acc_jerk_snap_rows(xp, vp, ap, mass, act, G, cutoff, softening)
        ha = hc[act]
        hh, h10, h120 = ha / 2, (ha * ha) / 10, (ha * ha * ha) / 120
        a0, j0, s0, v0 = a[act], j[act], s[act], v[act]
        v1 = v0 + ((a0 + a1) * hh + ((j0 - j1) * h10 + (s0 + s1) * h120))
        x[act] = x[act] + ((v0 + v1) * hh + ((a0 - a1) * h10 + (j0 + j1) * h120))
        want, valid = hermite6_dt_bodies(a0, j0, s0, a1, j1, s1, h[act], eta)
        c[act] = hermite6_high(a0, j0, s0, a1, j1, s1, h[act])[0]
        v[act], a[act], j[act], s[act] = v1, a1, j1, s1
        return want, valid

    return _simulate_block(pos, vel, start, advance, dt, t_end, eta, max_level, check, levels,
                           body_times, stats)
