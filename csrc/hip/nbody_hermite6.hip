// gfx950 kernels of the 6th-order Hermite scheme (Nitadori & Makino 2008; gs_hermite_scheme.h).
//
// The hot kernel evaluates, for every body i at the predicted state (xp, vp, ap),
//     a_i = sum_j A_ij,   A_ij = mu_j d r^-3
//     j_i = sum_j J_ij,   J_ij = mu_j w r^-3 - 3 alpha A_ij
//     s_i = sum_j S_ij,   S_ij = mu_j q r^-3 - 6 alpha J_ij - 3 beta A_ij
//     d = xp_j - xp_i, w = vp_j - vp_i, q = ap_j - ap_i, r^2 = |d|^2 + eps^2,
//     alpha = (d.w) r^-2, beta = (|w|^2 + d.q) r^-2 + alpha^2
// (and phi_i = -sum_j mu_j / r where asked), with the project's pair law: a pair contributes
// exactly zero to all of them when r^2 < cutoff^2.
//   * It follows hermite_eval_kernel (nbody_hermite.hip): one-sided, i-owned, no atomics; a lane
//     owns IPL i-bodies and keeps their 9 sums (and phi) in registers.
//   * A j-body is three rows, (x, y, z, mu), (v, 0) and (ap, 0), staged into double-buffered LDS
//     tiles by LDS-DMA (tile_fill; 3 x 2 x 4 KiB = 24 KiB) and read back as broadcast
//     ds_read_b128.
//   * The pair term shares the acceleration and jerk arithmetic of the 4th-order kernel bit for
//     bit (s = mu r^-1 r^-2, 3 alpha = (d.w)(3 r^-2), u = w - 3 alpha d) and adds
//     S_ij = s (q - 6 alpha u - 3 beta d): never r^-5 or G m_i m_j. fp32 runs over pairs of i as
//     2-vectors (v_pk_*), fp64 through rsqrt_dev.
//   * Canonical chunked summation: every chunk is summed from zero in j order into
//     PA / PJ / PS[chunk][i], and the reduce kernel adds the chunk sums in chunk order, so IPL
//     and the number of chunk groups change the grid, never the bits.
// Step chain (one stream, no host round trip): control (hermite_ctrl_kernel, shared with the
// 4th-order chain) -> predict -> evaluate -> reduce + correct + next-step minima.
// Block time steps (fp64): the chain of nbody_hermite.hip, whose next-time minima, control,
// compaction and start kernels it runs as they are (they read the block state, n_real, A and J
// only): next + control -> predict-all + mark (block6_predict_kernel) -> compact -> evaluate of the
// active bodies, narrow (hermite6_narrow_kernel, parallel over j) or wide (the LIST form of
// hermite6_eval_kernel) by n_act -> reduce + correct + new level (block6_correct_kernel). The
// predictor, the fold of the partials, the HM_OUT store and the corrector of a body are device
// functions that the shared step's kernels and the block step's both call (h6predict_row, h6fold,
// h6out, h6correct_row); the launchers are the H6Args overloads of order 4's (gs_hermite.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "gs_common.h"
#include "gs_hermite.h"
#include "gs_hermite_scheme.h"
#include "gs_tile.h"

namespace gs {

// The sums and the predicted rows of one i-body (V = T) or of a pair of them (V = f2).
template <typename V>
struct H6Body {
  V x, y, z, u, v, w, bx, by, bz;                 // predicted position, velocity, acceleration
  V ax, ay, az, ph, jx, jy, jz, sx, sy, sz;       // current chunk
};

template <typename V>
__device__ __forceinline__ void h6reset(H6Body<V>& b) {
  b.ax = b.ay = b.az = b.ph = b.jx = b.jy = b.jz = b.sx = b.sy = b.sz = V(0.0f);
}

// One i-j interaction (per element of V). The first 26 operations are hinteract()'s; the snap
// adds 3 sub (q), 2 fma + mul (|w|^2), 2 fma + mul (d.q), add, mul, mul, fma (3 beta), add
// (6 alpha), and 3 fma per component.
template <bool PHI, typename V, typename T>
__device__ __forceinline__ void h6interact(H6Body<V>& b, const V4<T>& xj, const V4<T>& vj,
                                           const V4<T>& aj, T cut2, T eps2) {
  const V dx = V(xj.x) - b.x, dy = V(xj.y) - b.y, dz = V(xj.z) - b.z;
  const V wx = V(vj.x) - b.u, wy = V(vj.y) - b.v, wz = V(vj.z) - b.w;
  const V qx = V(aj.x) - b.bx, qy = V(aj.y) - b.by, qz = V(aj.z) - b.bz;
  const V r2 = fmav(dz, dz, fmav(dy, dy, fmav(dx, dx, V(eps2))));
  const V inv = inv_cut(r2, cut2);
  const V inv2 = inv * inv;
  const V mi = V(xj.w) * inv;
  const V s = mi * inv2;
  const V dw = fmav(dz, wz, fmav(dy, wy, dx * wx));
  const V i3 = V(T(3)) * inv2;
  const V al3 = dw * i3;  // 3 alpha
  const V ww = fmav(wz, wz, fmav(wy, wy, wx * wx));
  const V dq = fmav(dz, qz, fmav(dy, qy, dx * qx));
  const V al = dw * inv2;
  const V be3 = fmav(al3, al, (ww + dq) * i3);  // 3 beta
  const V al6 = al3 + al3;
  const V ux = fmav(-al3, dx, wx), uy = fmav(-al3, dy, wy), uz = fmav(-al3, dz, wz);
  b.ax = fmav(s, dx, b.ax);
  b.ay = fmav(s, dy, b.ay);
  b.az = fmav(s, dz, b.az);
  b.jx = fmav(s, ux, b.jx);
  b.jy = fmav(s, uy, b.jy);
  b.jz = fmav(s, uz, b.jz);
  b.sx = fmav(s, fmav(-al6, ux, fmav(-be3, dx, qx)), b.sx);
  b.sy = fmav(s, fmav(-al6, uy, fmav(-be3, dy, qy)), b.sy);
  b.sz = fmav(s, fmav(-al6, uz, fmav(-be3, dz, qz)), b.sz);
  if constexpr (PHI) b.ph += mi;
}

// The lane's bodies: IPL of them as scalars, or (fp32, even IPL) IPL / 2 pairs as 2-vectors.
template <typename T, int IPL>
struct H6Lane {
  static constexpr bool PK = sizeof(T) == 4 && IPL % 2 == 0;
  using V = std::conditional_t<PK, f2, T>;
  static constexpr int NB = PK ? IPL / 2 : IPL;
  H6Body<V> b[NB];
};

// EVALUATE: grid (n_pad / (256 IPL), groups). Workgroup (b, g) sweeps the chunks of group g and
// stores one partial per chunk and i-body: PA[c][i] = (ax, ay, az, sum mu / r),
// PJ[c][i] = (jx, jy, jz, 0), PS[c][i] = (sx, sy, sz, 0).
// LIST (a block step's wide path): lane slot s owns body blk.list[s] (spare slots: a copy of the
// last entry), the partials are stored per slot and i-blocks beyond n_act exit; the j loop, hence
// a body's bits, is the same.
template <typename T, bool PHI, int IPL, bool LIST = false>
__global__ __launch_bounds__(kBlock) void hermite6_eval_kernel(H6Args<T> a, int gated) {
  constexpr int TB = Tile<T>::kBodies;
  using Lane = H6Lane<T, IPL>;
  using V = typename Lane::V;
  constexpr int E = Lane::PK ? 2 : 1;  // i-bodies per element group
  __shared__ __attribute__((aligned(16))) V4<T> tx[2][TB];
  __shared__ __attribute__((aligned(16))) V4<T> tv[2][TB];
  __shared__ __attribute__((aligned(16))) V4<T> ta[2][TB];
  if (gated && !a.ctrl->active) return;  // the run has reached t_end: a no-op step
  const int64_t ib = (int64_t)blockIdx.x * (kBlock * IPL);
  int64_t n_act = 0;
  if constexpr (LIST) {
    const HermiteBlockCtrl* bc = a.blk.bc;
    if (!bc->active || bc->path != HP_WIDE) return;
    n_act = bc->n_act;
    if (ib >= n_act) return;
  }
  const int per = (a.n_chunks + (int)gridDim.y - 1) / (int)gridDim.y;
  const int c0 = (int)blockIdx.y * per;
  const int c1 = min(c0 + per, a.n_chunks);
  const int tpc = (int)(a.chunk / TB);  // tiles per chunk
  const int ntiles = (c1 - c0) * tpc;
  if (ntiles <= 0) return;
  const V4<T>* XP = reinterpret_cast<const V4<T>*>(a.XP);
  const V4<T>* VP = reinterpret_cast<const V4<T>*>(a.VP);
  const V4<T>* AP = reinterpret_cast<const V4<T>*>(a.AP);
  V4<T>* PA = reinterpret_cast<V4<T>*>(a.PA);
  V4<T>* PJ = reinterpret_cast<V4<T>*>(a.PJ);
  V4<T>* PS = reinterpret_cast<V4<T>*>(a.PS);
  Lane ln;
#pragma unroll
  for (int k = 0; k < IPL; ++k) {
    int64_t row = ib + threadIdx.x + k * kBlock;
    if constexpr (LIST) row = a.blk.list[row < n_act ? row : n_act - 1];
    const V4<T> x = XP[row], v = VP[row], p = AP[row];
    H6Body<V>& b = ln.b[k / E];
    vset(b.x, k % E, x.x); vset(b.y, k % E, x.y); vset(b.z, k % E, x.z);
    vset(b.u, k % E, v.x); vset(b.v, k % E, v.y); vset(b.w, k % E, v.z);
    vset(b.bx, k % E, p.x); vset(b.by, k % E, p.y); vset(b.bz, k % E, p.z);
  }
  auto fill = [&](int t) {
    const int64_t j0 = (int64_t)(c0 + t / tpc) * a.chunk + (int64_t)(t % tpc) * TB;
    tile_fill<T>(XP + j0, tx[t & 1]);
    tile_fill<T>(VP + j0, tv[t & 1]);
    tile_fill<T>(AP + j0, ta[t & 1]);
  };
  fill(0);
#pragma unroll
  for (int k = 0; k < Lane::NB; ++k) h6reset(ln.b[k]);
  for (int t = 0; t < ntiles; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // tile t is in LDS for every wave; buffer (t+1)&1 is free
    if (t + 1 < ntiles) fill(t + 1);
    const V4<T>* cx = tx[t & 1];
    const V4<T>* cv = tv[t & 1];
    const V4<T>* ca = ta[t & 1];
#pragma unroll 4
    for (int j = 0; j < TB; ++j) {
      const V4<T> xj = cx[j], vj = cv[j], aj = ca[j];  // uniform addresses: broadcast ds_reads
#pragma unroll
      for (int k = 0; k < Lane::NB; ++k) h6interact<PHI>(ln.b[k], xj, vj, aj, a.cut2, a.eps2);
    }
    if ((t + 1) % tpc == 0) {
      const int c = c0 + t / tpc;
#pragma unroll
      for (int k = 0; k < IPL; ++k) {
        const H6Body<V>& b = ln.b[k / E];
        V4<T> oa, oj, os;
        oa.x = vget(b.ax, k % E); oa.y = vget(b.ay, k % E); oa.z = vget(b.az, k % E);
        oa.w = vget(b.ph, k % E);
        oj.x = vget(b.jx, k % E); oj.y = vget(b.jy, k % E); oj.z = vget(b.jz, k % E);
        oj.w = T(0);
        os.x = vget(b.sx, k % E); os.y = vget(b.sy, k % E); os.z = vget(b.sz, k % E);
        os.w = T(0);
        const int64_t o = (int64_t)c * a.n_pad + ib + threadIdx.x + k * kBlock;
        PA[o] = oa;
        PJ[o] = oj;
        PS[o] = os;
      }
#pragma unroll
      for (int k = 0; k < Lane::NB; ++k) h6reset(ln.b[k]);
    }
  }
}

// ---------------------------------------------------------------------------------------
// What the shared step's kernels and the block step's share, per body.

template <typename T>
__device__ __forceinline__ V4<T>* rows4(T* p) { return reinterpret_cast<V4<T>*>(p); }

// The predicted rows of body i over h (x to h^5, v to h^4, a to h^3; xp.w = mu).
template <typename T>
__device__ __forceinline__ void h6predict_row(const H6Args<T>& a, int64_t i, T h, V4<T>& xp,
                                              V4<T>& vp, V4<T>& ap) {
  const H6Taylor<T> t = h6_taylor(h);
  const V4<T> x = rows4(a.X)[i], v = rows4(a.V)[i], ac = rows4(a.A)[i], jk = rows4(a.J)[i],
              sn = rows4(a.S)[i], cr = rows4(a.C)[i];
  T px, pv, pa;
  h6_predict(t, x.x, v.x, ac.x, jk.x, sn.x, cr.x, px, pv, pa);
  xp.x = px; vp.x = pv; ap.x = pa;
  h6_predict(t, x.y, v.y, ac.y, jk.y, sn.y, cr.y, px, pv, pa);
  xp.y = px; vp.y = pv; ap.y = pa;
  h6_predict(t, x.z, v.z, ac.z, jk.z, sn.z, cr.z, px, pv, pa);
  xp.z = px; vp.z = pv; ap.z = pa;
  xp.w = x.w;
}

// ... and their store (ghost rows: zero).
template <typename T>
__device__ __forceinline__ void h6predicted(const H6Args<T>& a, int64_t i, const V4<T>& xp,
                                            const V4<T>& vp, const V4<T>& ap) {
  rows4(a.XP)[i] = xp; rows4(a.VP)[i] = vp; rows4(a.AP)[i] = ap;
}

// m = (a1, j1, s1) and ph of one row: its `parts` partials, `stride` rows apart, added from zero
// in order. UNROLL4: the block step's loop (a schedule hint, the sums are the same).
template <bool UNROLL4, typename T>
__device__ __forceinline__ void h6fold(const void* pa_, const void* pj_, const void* ps_, int parts,
                                       int64_t stride, int64_t row, T (&m)[3][3], T& ph) {
  const V4<T>* PA = reinterpret_cast<const V4<T>*>(pa_);
  const V4<T>* PJ = reinterpret_cast<const V4<T>*>(pj_);
  const V4<T>* PS = reinterpret_cast<const V4<T>*>(ps_);
  auto add = [&](int c) {
    const int64_t o = (int64_t)c * stride + row;
    const V4<T> pa = PA[o], pj = PJ[o], ps = PS[o];
    m[0][0] += pa.x; m[0][1] += pa.y; m[0][2] += pa.z; ph += pa.w;
    m[1][0] += pj.x; m[1][1] += pj.y; m[1][2] += pj.z;
    m[2][0] += ps.x; m[2][1] += ps.y; m[2][2] += ps.z;
  };
  if constexpr (UNROLL4) {
#pragma unroll 4
    for (int c = 0; c < parts; ++c) add(c);
  } else {
    for (int c = 0; c < parts; ++c) add(c);
  }
}

template <typename T>
__device__ __forceinline__ V4<T> h6row(const T (&v)[3]) {
  return V4<T>{v[0], v[1], v[2], T(0)};
}

// HM_OUT: (a, -sum mu / r), j, s of the sums m to row (or slot) `row` of the outputs.
template <typename T>
__device__ __forceinline__ void h6out(const H6Args<T>& a, int64_t row, const T (&m)[3][3], T ph) {
  V4<T> oa = h6row(m[0]);
  oa.w = -ph;
  rows4(a.a_out)[row] = oa; rows4(a.j_out)[row] = h6row(m[1]); rows4(a.s_out)[row] = h6row(m[2]);
}

// What h6_dt reads: the new a, j, s and the higher derivatives at the end of the step.
struct H6Rates {
  double a1[3], j1[3], s1[3], c1[3], p1[3], a5[3];
};

// The corrector of body i over hd with the sums m = (a1, j1, s1), the crackle c1 and the higher
// derivatives; stores x, v, a, j, s, c.
template <typename T>
__device__ __forceinline__ H6Rates h6correct_row(const H6Args<T>& a, int64_t i, double hd,
                                                 const T (&m)[3][3]) {
  V4<T>*X = rows4(a.X), *V = rows4(a.V), *A = rows4(a.A), *J = rows4(a.J), *S = rows4(a.S);
  const T h = (T)hd;
  const V4<T> x = X[i], v = V[i], a0 = A[i], j0 = J[i], s0 = S[i];
  const T xs[3] = {x.x, x.y, x.z}, vs[3] = {v.x, v.y, v.z};
  const T as[3] = {a0.x, a0.y, a0.z}, js[3] = {j0.x, j0.y, j0.z}, ss[3] = {s0.x, s0.y, s0.z};
  T x1[3], v1[3];
  H6Rates r;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    h6_correct(h, xs[d], vs[d], as[d], js[d], ss[d], m[0][d], m[1][d], m[2][d], x1[d], v1[d]);
    r.a1[d] = m[0][d]; r.j1[d] = m[1][d]; r.s1[d] = m[2][d];
    h6_high(hd, as[d], js[d], ss[d], r.a1[d], r.j1[d], r.s1[d], r.c1[d], r.p1[d], r.a5[d]);
  }
  const V4<T> ox = {x1[0], x1[1], x1[2], x.w}, ov = {v1[0], v1[1], v1[2], T(0)};
  const V4<T> oc = {(T)r.c1[0], (T)r.c1[1], (T)r.c1[2], T(0)};
  X[i] = ox; V[i] = ov; A[i] = h6row(m[0]); J[i] = h6row(m[1]); S[i] = h6row(m[2]);
  rows4(a.C)[i] = oc;
  return r;
}

// PREDICT over the step's h (ghost rows stay zero).
template <typename T>
__global__ __launch_bounds__(kBlock) void hermite6_predict_kernel(H6Args<T> a) {
  if (!a.ctrl->active) return;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n_pad) return;
  V4<T> xp = {T(0), T(0), T(0), T(0)}, vp = xp, ap = xp;
  if (i < a.n_real) h6predict_row(a, i, (T)a.ctrl->h, xp, vp, ap);
  h6predicted(a, i, xp, vp, ap);
}

// REDUCE (+ CORRECT): one thread per body adds its chunk partials in chunk order, then HM_STEP
// applies the corrector, stores a1, j1, s1, c1 and the body's wish for the next step, HM_INIT
// starts a run (a, j, s <- sums, c <- 0; the first step (eta / 2) |a| / |j|), HM_OUT returns the
// derivatives. Per-workgroup dt minima go to wgmin (+inf when no body of the workgroup takes
// part: ghost rows, a zero or non-finite ratio, or a fixed-step run).
template <typename T>
__global__ __launch_bounds__(kBlock) void hermite6_reduce_kernel(H6Args<T> a) {
  __shared__ double red[kBlock / 64];
  if (a.mode == HM_STEP && !a.ctrl->active) return;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;  // (n_pad: a multiple of 256)
  T m[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, ph = 0;  // a1, j1, s1
  h6fold<false>(a.PA, a.PJ, a.PS, a.n_chunks, a.n_pad, i, m, ph);
  if (a.mode == HM_OUT) return h6out(a, i, m, ph);
  const V4<T> z = {T(0), T(0), T(0), T(0)};
  V4<T>*X = rows4(a.X), *V = rows4(a.V), *A = rows4(a.A), *J = rows4(a.J), *S = rows4(a.S),
        *C = rows4(a.C);
  const double eta = a.ctrl->eta;
  double dti = INFINITY;
  if (i >= a.n_real) {
    A[i] = z; J[i] = z; S[i] = z; C[i] = z;
    if (a.mode == HM_STEP) {
      X[i] = z;
      V[i] = z;
    }
  } else if (a.mode == HM_INIT) {
    A[i] = h6row(m[0]); J[i] = h6row(m[1]); S[i] = h6row(m[2]); C[i] = z;
    if (eta > 0.0) {
      const double ad[3] = {m[0][0], m[0][1], m[0][2]}, jd[3] = {m[1][0], m[1][1], m[1][2]};
      double d;
      if (hermite_first_dt(eta, ad, jd, d)) dti = d;
    }
  } else {
    const H6Rates r = h6correct_row(a, i, a.ctrl->h, m);
    double d;
    if (eta > 0.0 && h6_dt(eta, r.a1, r.j1, r.s1, r.c1, r.p1, r.a5, d)) dti = d;
  }
  dti = block_min(dti, red);
  if (threadIdx.x == 0) a.wgmin[blockIdx.x] = dti;
}

// ---------------------------------------------------------------------------------------
// Block time steps (fp64): body i stands at tb_i ticks and steps by 2^(L - level_i) ticks.

// PREDICT-ALL + MARK: every real body from its own tb to t_next (x to h^5, v to h^4, a to h^3);
// ghost rows zero; counts the due bodies of the workgroup for the compaction
// (block_compact_kernel, nbody_hermite.hip).
template <typename T>
__global__ __launch_bounds__(kBlock) void block6_predict_kernel(H6Args<T> a) {
  __shared__ int cnt[kBlock / 64];
  const HBlock& b = a.blk;
  if (!b.bc->active) return;
  const int L = b.bc->L;
  const int64_t t_next = b.bc->t_ticks;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;  // (n_pad: a multiple of 256)
  V4<T> xp = {T(0), T(0), T(0), T(0)}, vp = xp, ap = xp;
  bool due = false;
  if (i < a.n_real) {
    due = body_due(b, i, L, t_next);
    h6predict_row(a, i, (T)ticks_seconds(b.bc->dt_max, t_next - b.tb[i], L), xp, vp, ap);
  }
  h6predicted(a, i, xp, vp, ap);
  const int c = __popcll(__ballot(due));
  if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) b.wgcount[blockIdx.x] = cnt[0] + cnt[1] + cnt[2] + cnt[3];
}

// NARROW EVALUATE (n_act <= narrow_max): parallel over j, the geometry of hermite_narrow_kernel.
// Grid (n_slices, passes): workgroup (s, y) takes the j rows of slice s and the groups y,
// y + passes, ... of kNarrowGroup6 active bodies. The group's predicted rows are wave-uniform;
// the lanes stride over the slice with coalesced 32-byte loads of (XP, VP, AP), each summing its
// rows from zero in j order; the lanes are folded by a fixed tree (shuffle-down 32..1 in the
// wave, then the four waves in order through LDS) and one partial (a, sum mu / r), j, s per
// (slice, slot) is stored. Slice length and tree depend on n_pad only, so a body's bits depend
// on neither the group size, its slot nor the other active bodies.
template <typename T, bool PHI>
__global__ __launch_bounds__(kBlock) void hermite6_narrow_kernel(H6Args<T> a) {
  constexpr int G = kNarrowGroup6;
  __shared__ T red[kBlock / 64][G][10];
  const HBlock& b = a.blk;
  if (!b.bc->active || b.bc->path != HP_NARROW) return;
  const int n_act = min(b.bc->n_act, b.cap);
  const int ngroups = (n_act + G - 1) / G;
  const int64_t j0 = (int64_t)blockIdx.x * b.slice;
  const int64_t j1 = min(j0 + (int64_t)b.slice, a.n_pad);
  const V4<T>* XP = reinterpret_cast<const V4<T>*>(a.XP);
  const V4<T>* VP = reinterpret_cast<const V4<T>*>(a.VP);
  const V4<T>* AP = reinterpret_cast<const V4<T>*>(a.AP);
  V4<T>* NA = reinterpret_cast<V4<T>*>(b.NA);
  V4<T>* NJ = reinterpret_cast<V4<T>*>(b.NJ);
  V4<T>* NS = reinterpret_cast<V4<T>*>(a.NS);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int g = blockIdx.y; g < ngroups; g += (int)gridDim.y) {
    H6Body<T> st[G];
#pragma unroll
    for (int k = 0; k < G; ++k) {  // (spare slots of the last group: a copy)
      const int64_t row = b.list[min(g * G + k, n_act - 1)];
      const V4<T> x = XP[row], v = VP[row], p = AP[row];
      st[k].x = x.x; st[k].y = x.y; st[k].z = x.z;
      st[k].u = v.x; st[k].v = v.y; st[k].w = v.z;
      st[k].bx = p.x; st[k].by = p.y; st[k].bz = p.z;
      h6reset(st[k]);
    }
    for (int64_t j = j0 + threadIdx.x; j < j1; j += kBlock) {
      const V4<T> xj = XP[j], vj = VP[j], aj = AP[j];
#pragma unroll
      for (int k = 0; k < G; ++k) h6interact<PHI>(st[k], xj, vj, aj, a.cut2, a.eps2);
    }
#pragma unroll
    for (int k = 0; k < G; ++k) {
      T v[10] = {st[k].ax, st[k].ay, st[k].az, st[k].ph, st[k].jx,
                 st[k].jy, st[k].jz, st[k].sx, st[k].sy, st[k].sz};
#pragma unroll
      for (int c = 0; c < 10; ++c) {
        for (int off = 32; off > 0; off >>= 1) v[c] += __shfl_down(v[c], off, 64);
        if (lane == 0) red[wave][k][c] = v[c];
      }
    }
    __syncthreads();
    if (threadIdx.x < G && g * G + (int)threadIdx.x < n_act) {
      const int k = threadIdx.x;
      T v[10];
#pragma unroll
      for (int c = 0; c < 10; ++c)
        v[c] = ((red[0][k][c] + red[1][k][c]) + red[2][k][c]) + red[3][k][c];
      const V4<T> oa = {v[0], v[1], v[2], v[3]}, oj = {v[4], v[5], v[6], T(0)},
                  os = {v[7], v[8], v[9], T(0)};
      const int64_t o = (int64_t)blockIdx.x * b.cap + (g * G + k);
      NA[o] = oa;
      NJ[o] = oj;
      NS[o] = os;
    }
    __syncthreads();
  }
}

// REDUCE + CORRECT + NEW LEVEL, one thread per slot of the active list: the slice partials in
// slice order (narrow) or the chunk partials in chunk order (wide), then the corrector over the
// body's own h, c1 and the higher derivatives, the step the body wants (h6_dt) and the level rule
// of order 4 (block_new_level). HM_OUT: the sums go to a_out / j_out / s_out [slot] and nothing
// else is touched.
template <typename T>
__global__ __launch_bounds__(kBlock) void block6_correct_kernel(H6Args<T> a) {
  const HBlock& b = a.blk;
  HermiteBlockCtrl* bc = b.bc;
  if (!bc->active) return;
  const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (s >= bc->n_act) return;
  const bool narrow = bc->path == HP_NARROW;
  T m[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, ph = 0;  // a1, j1, s1
  h6fold<true>(narrow ? b.NA : (void*)a.PA, narrow ? b.NJ : (void*)a.PJ,
               narrow ? (void*)a.NS : (void*)a.PS, narrow ? b.n_slices : a.n_chunks,
               narrow ? (int64_t)b.cap : a.n_pad, s, m, ph);
  if (a.mode == HM_OUT) return h6out(a, s, m, ph);
  const int64_t i = b.list[s];
  const int L = bc->L;
  const int64_t t_next = bc->t_ticks;
  const double dt_max = bc->dt_max;
  const H6Rates r = h6correct_row(a, i, ticks_seconds(dt_max, t_next - b.tb[i], L), m);
  b.tb[i] = t_next;
  double want;
  const bool rated = h6_dt(bc->eta, r.a1, r.j1, r.s1, r.c1, r.p1, r.a5, want);
  b.level[i] = block_new_level(bc, b.level[i], rated, want, t_next, L, dt_max);
}

// ---------------------------------------------------------------------------------------
// Host launchers: validate, compute the grid, dispatch.

// The forms that are built: 1 or 2 i-bodies per lane in fp32, 1 in fp64.
bool hermite6_ipl_ok(int fp64, int ipl) { return ipl == 1 || (ipl == 2 && !fp64); }

template <typename T>
static bool args6_ok(const H6Args<T>& a, int ipl = 1) {
  return chunk_geometry_ok<T>(a.n_pad, a.chunk, a.n_chunks, ipl) && a.n_real >= 1 &&
         a.n_real <= a.n_pad;
}

// What every evaluate launch needs (the shared step's and the block step's wide path), and its
// grid.
template <typename T>
static bool eval6_ok(const H6Args<T>& a, int ipl) {
  return hermite6_ipl_ok(sizeof(T) == 8, ipl) && args6_ok(a, ipl) && a.XP && a.VP && a.AP &&
         a.PA && a.PJ && a.PS;
}

template <typename T>
static dim3 eval6_grid(const H6Args<T>& a, int ipl, int groups) {
  return dim3((unsigned)(a.n_pad / (kBlock * ipl)), (unsigned)clamp_groups(groups, a.n_chunks));
}

template <typename T, int IPL>
static hipError_t eval6_go(const H6Args<T>& a, dim3 grid, bool gated, hipStream_t s) {
  return a.phi ? hlaunch(hermite6_eval_kernel<T, true, IPL>, grid, s, a, (int)gated)
               : hlaunch(hermite6_eval_kernel<T, false, IPL>, grid, s, a, (int)gated);
}

template <typename T>
hipError_t launch_hermite6_eval(const H6Args<T>& a, int ipl, int groups, bool gated,
                                hipStream_t s) {
  if (!eval6_ok(a, ipl) || (gated && !a.ctrl)) return hipErrorInvalidValue;
  if constexpr (sizeof(T) == 4) {
    if (ipl == 2) return eval6_go<T, 2>(a, eval6_grid(a, ipl, groups), gated, s);
  }
  return eval6_go<T, 1>(a, eval6_grid(a, ipl, groups), gated, s);
}

template <typename T>
hipError_t launch_hermite6_predict(const H6Args<T>& a, hipStream_t s) {
  if (!args6_ok(a) || !a.ctrl) return hipErrorInvalidValue;
  return hlaunch(hermite6_predict_kernel<T>, row_grid(a.n_pad), s, a);
}

template <typename T>
hipError_t launch_hermite6_reduce(const H6Args<T>& a, hipStream_t s) {
  if (!args6_ok(a) || !a.ctrl || !a.wgmin) return hipErrorInvalidValue;
  return hlaunch(hermite6_reduce_kernel<T>, row_grid(a.n_pad), s, a);
}

// ---- block steps (fp64): the H6Args overloads of order 4's launchers ------------------------
template <typename T>
static bool block6_ok(const H6Args<T>& a) {
  const HBlock& b = a.blk;
  return args6_ok(a) && b.bc && b.tb && b.level && b.list && b.wgcount && b.wgnext;
}

template <typename T>
hipError_t launch_block_next(const H6Args<T>& a, hipStream_t s) {
  return launch_block_next<T, T>(base_view(a), s);
}

template <typename T>
hipError_t launch_block_predict(const H6Args<T>& a, hipStream_t s) {
  if (!block6_ok(a)) return hipErrorInvalidValue;
  const hipError_t e = hlaunch(block6_predict_kernel<T>, row_grid(a.n_pad), s, a);
  if (e != hipSuccess) return e;
  return launch_block_compact<T, T>(base_view(a), s);
}

template <typename T>
hipError_t launch_block_narrow(const H6Args<T>& a, hipStream_t s) {
  const HBlock& b = a.blk;
  if (!block6_ok(a)) return hipErrorInvalidValue;
  if (b.cap < 1) return hipSuccess;  // (narrow_max 0: every step is wide)
  if (b.slice < kBlock || b.slice % kBlock || (int64_t)b.n_slices * b.slice < a.n_pad || !b.NA ||
      !b.NJ || !a.NS || b.cap > a.n_pad)
    return hipErrorInvalidValue;
  const int groups = (b.cap + kNarrowGroup6 - 1) / kNarrowGroup6;
  const dim3 grid((unsigned)b.n_slices, (unsigned)(groups < 16 ? groups : 16));
  return a.phi ? hlaunch(hermite6_narrow_kernel<T, true>, grid, s, a)
               : hlaunch(hermite6_narrow_kernel<T, false>, grid, s, a);
}

template <typename T>
hipError_t launch_block_wide(const H6Args<T>& a, int ipl, int groups, hipStream_t s) {
  if (!eval6_ok(a, ipl) || !block6_ok(a)) return hipErrorInvalidValue;
  const dim3 grid = eval6_grid(a, ipl, groups);
  return a.phi ? hlaunch(hermite6_eval_kernel<T, true, 1, true>, grid, s, a, 0)
               : hlaunch(hermite6_eval_kernel<T, false, 1, true>, grid, s, a, 0);
}

template <typename T>
hipError_t launch_block_correct(const H6Args<T>& a, hipStream_t s) {
  if (!block6_ok(a)) return hipErrorInvalidValue;
  return hlaunch(block6_correct_kernel<T>, row_grid(a.n_pad), s, a);
}

template hipError_t launch_block_next<double>(const H6Args<double>&, hipStream_t);
template hipError_t launch_block_predict<double>(const H6Args<double>&, hipStream_t);
template hipError_t launch_block_narrow<double>(const H6Args<double>&, hipStream_t);
template hipError_t launch_block_wide<double>(const H6Args<double>&, int, int, hipStream_t);
template hipError_t launch_block_correct<double>(const H6Args<double>&, hipStream_t);

#define GS_HERMITE6_INSTANTIATE(T)                                                          \
  template hipError_t launch_hermite6_predict<T>(const H6Args<T>&, hipStream_t);             \
  template hipError_t launch_hermite6_eval<T>(const H6Args<T>&, int, int, bool, hipStream_t); \
  template hipError_t launch_hermite6_reduce<T>(const H6Args<T>&, hipStream_t);
GS_HERMITE6_INSTANTIATE(float)
GS_HERMITE6_INSTANTIATE(double)

}  // namespace gs
