// gfx950 kernels of the 4th-order Hermite integrator (Makino & Aarseth 1992).
//
// The hot kernel evaluates, for every body i at the predicted state (xp, vp),
//     a_i   = sum_j mu_j d / r^3
//     j_i   = sum_j mu_j (w - 3 (d.w) d / r^2) / r^3          d = xp_j - xp_i, w = vp_j - vp_i
//     phi_i = -sum_j mu_j / r                                  r^2 = |d|^2 + eps^2
// with the project's pair law (a pair contributes exactly zero to all three when
// r^2 < cutoff^2: the self term, coincident bodies, a ghost row on a body at the origin).
//   * One-sided and i-owned like force_split_kernel: a lane owns IPL i-bodies and keeps a, j
//     (and phi behind a template flag) in registers; no atomics.
//   * A j-body is two rows, (x, y, z, mu) and (vx, vy, vz, 0); both are staged into
//     double-buffered LDS tiles by LDS-DMA (tile_fill) and read back as broadcast ds_read_b128.
//   * fp32 runs over pairs of i as 2-vectors: everything but the v_rsq_f32 and the cutoff
//     select is a v_pk_* (26 packed operations per two pairs). Never r^-5 or G m_i m_j:
//     s = mu r^-1 r^-2, alpha = 3 (d.w) r^-2, term = s (w - alpha d).
//   * Canonical chunked summation (gs::auto_chunk): every chunk is summed from zero in j order
//     into PA / PJ[chunk][i], and the reduce kernel adds the chunk sums in chunk order, so the
//     bits do not depend on IPL or on how many chunk groups the grid has.
//   * Mixed precision (HArgs<float, double>): the state, the predictor, the reduce and the
//     corrector are fp64; the predictor hands the pair kernels the position as a double-single
//     pair of fp32 rows, hi = float(xp) and lo = float(xp - hi), a third LDS tile, and the pair
//     term starts from d = (hi_j - hi_i) + (lo_j - lo_i); all else is the fp32 kernel (hsep).
//   * Collisions (template flag NN, off by default and then compiled out): every body has a
//     radius, carried in the spare component of the VP row, and the evaluate kernels also keep,
//     per i-body, the j of the smallest q = r^2 - (R_i + R_j)^2 (the lowest j on an exact tie),
//     stored per chunk or slice beside the partial sums; the reduce kernels fold them, keep
//     the latest and the closest (q, j) per body and count the overlaps (q < eps^2).
// Step chain (one stream, no host round trip): control (next h from the last step's
// per-workgroup dt minima; advances t, steps) -> predict -> evaluate -> reduce + correct.
// Block time steps (each body on its own step dt 2^-k; second half of this file): next-time
// minima + control -> predict-all + mark -> compact (scan) -> evaluate of the active bodies,
// narrow (hermite_narrow_kernel, parallel over j) or wide (the GATHER form of
// hermite_eval_kernel) by n_act -> reduce + correct + new level of the active bodies.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gs_common.h"
#include "gs_hermite.h"
#include "gs_tile.h"

namespace gs {

// Separation of a pair: plain, or (DS, mixed precision) from double-single positions hi + lo,
// where the difference of the hi parts is exact whenever the bodies are close and the lo parts
// restore what float(x) dropped.
template <bool DS, typename V>
__device__ __forceinline__ V hsep(V qh, V xh, V ql, V xl) {
  if constexpr (DS) return (qh - xh) + (ql - xl);
  return qh - xh;
}

// The lo rows of a lane's i-bodies (DS only).
template <typename T, int IPL>
struct HLo {
  T x[IPL], y[IPL], z[IPL];
};

// One i-j interaction: 6 sub, 3 fma (r^2), rsq + select, 3 mul (r^-2, mu r^-1, s), mul + 2 fma
// (d.w), 2 mul (alpha), 3 fma (a), 3 fma (w - alpha d), 3 fma (j); DS: 3 sub and 3 add more.
// NN (collisions on): also the pair measure q = r^2 - (R_i + R_j)^2 (one add, one fma on the
// kernel's own r^2; R_j rides in p.w) and a strict-less compare-and-select against the best so
// far, so that the lowest j keeps an exact tie. A pair the law zeroes, a ghost row j (jreal
// false) or the body itself (with softening the law does not zero the self pair) takes no part.
template <typename T, bool PHI, bool DS = false, bool NN = false>
__device__ __forceinline__ void hinteract(T xi, T yi, T zi, T ui, T vi, T wi, const V4<T>& q,
                                          const V4<T>& p, T cut2, T eps2, T& ax, T& ay, T& az,
                                          T& ph, T& jx, T& jy, T& jz, const V4<T>& l = V4<T>(),
                                          T lxi = T(0), T lyi = T(0), T lzi = T(0), T ri = T(0),
                                          bool jreal = false, int32_t jg = 0, int32_t self = 0,
                                          T* bq = nullptr, int32_t* bn = nullptr) {
  const T dx = hsep<DS>(q.x, xi, l.x, lxi), dy = hsep<DS>(q.y, yi, l.y, lyi),
          dz = hsep<DS>(q.z, zi, l.z, lzi);
  const T wx = p.x - ui, wy = p.y - vi, wz = p.z - wi;
  const T r2 = fma_(dz, dz, fma_(dy, dy, fma_(dx, dx, eps2)));
  const bool ok = r2 >= cut2;
  T inv;
  if constexpr (sizeof(T) == 8) {
    // Branch-free (as the one-sided force kernel): the refinement runs on 1 below the cutoff.
    inv = rsqrt_dev(ok ? r2 : T(1));
    inv = ok ? inv : T(0);
  } else {
    inv = ok ? rsqrt_dev(r2) : T(0);
  }
  const T inv2 = inv * inv;
  const T mi = q.w * inv;
  const T s = mi * inv2;
  const T dw = fma_(dz, wz, fma_(dy, wy, dx * wx));
  const T al = dw * (T(3) * inv2);
  ax = fma_(s, dx, ax);
  ay = fma_(s, dy, ay);
  az = fma_(s, dz, az);
  jx = fma_(s, fma_(-al, dx, wx), jx);
  jy = fma_(s, fma_(-al, dy, wy), jy);
  jz = fma_(s, fma_(-al, dz, wz), jz);
  if constexpr (PHI) ph += mi;
  if constexpr (NN) {
    const T sr = p.w + ri;
    const T qv = fma_(-sr, sr, r2);
    const T qe = (ok && jreal && jg != self) ? qv : T(INFINITY);
    const bool lt = qe < *bq;
    *bq = lt ? qe : *bq;
    *bn = lt ? jg : *bn;
  }
}

// fp32, two i per lane as 2-vectors: each element sees exactly hinteract()'s arithmetic.
__device__ __forceinline__ f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }

template <bool PHI, bool DS = false, bool NN = false>
__device__ __forceinline__ void hinteract_pk(f2 xi, f2 yi, f2 zi, f2 ui, f2 vi, f2 wi,
                                             const V4<float>& q, const V4<float>& p, float cut2,
                                             float eps2, f2& ax, f2& ay, f2& az, f2& ph, f2& jx,
                                             f2& jy, f2& jz, const V4<float>& l = V4<float>(),
                                             f2 lxi = f2(0.0f), f2 lyi = f2(0.0f),
                                             f2 lzi = f2(0.0f), f2 ri = f2(0.0f),
                                             bool jreal = false, int32_t jg = 0,
                                             const int32_t* self = nullptr, float* bq = nullptr,
                                             int32_t* bn = nullptr) {
  const f2 dx = hsep<DS>(f2(q.x), xi, f2(l.x), lxi), dy = hsep<DS>(f2(q.y), yi, f2(l.y), lyi),
           dz = hsep<DS>(f2(q.z), zi, f2(l.z), lzi);
  const f2 wx = f2(p.x) - ui, wy = f2(p.y) - vi, wz = f2(p.z) - wi;
  const f2 r2 = fma2(dz, dz, fma2(dy, dy, fma2(dx, dx, f2(eps2))));
  f2 inv;
  inv.x = r2.x >= cut2 ? rsqrt_dev(r2.x) : 0.0f;
  inv.y = r2.y >= cut2 ? rsqrt_dev(r2.y) : 0.0f;
  const f2 inv2 = inv * inv;
  const f2 mi = f2(q.w) * inv;
  const f2 s = mi * inv2;
  const f2 dw = fma2(dz, wz, fma2(dy, wy, dx * wx));
  const f2 al = dw * (f2(3.0f) * inv2);
  ax = fma2(s, dx, ax);
  ay = fma2(s, dy, ay);
  az = fma2(s, dz, az);
  jx = fma2(s, fma2(-al, dx, wx), jx);
  jy = fma2(s, fma2(-al, dy, wy), jy);
  jz = fma2(s, fma2(-al, dz, wz), jz);
  if constexpr (PHI) ph += mi;
  if constexpr (NN) {
    const f2 sr = f2(p.w) + ri;
    const f2 qv = fma2(-sr, sr, r2);
    const float q0 = (r2.x >= cut2 && jreal && jg != self[0]) ? qv.x : INFINITY;
    const float q1 = (r2.y >= cut2 && jreal && jg != self[1]) ? qv.y : INFINITY;
    const bool l0 = q0 < bq[0], l1 = q1 < bq[1];
    bq[0] = l0 ? q0 : bq[0];
    bn[0] = l0 ? jg : bn[0];
    bq[1] = l1 ? q1 : bq[1];
    bn[1] = l1 ? jg : bn[1];
  }
}

template <typename T, int IPL>
struct HState {
  T x[IPL], y[IPL], z[IPL], u[IPL], v[IPL], w[IPL];  // predicted position and velocity
  T ax[IPL], ay[IPL], az[IPL], ph[IPL], jx[IPL], jy[IPL], jz[IPL];  // current chunk
};

// Nearest neighbour of a lane's i-bodies (NN kernels): own radius and row, the best q of the
// current chunk or slice and its j.
template <typename T, int IPL>
struct HNear {
  T r[IPL], q[IPL];
  int32_t n[IPL], self[IPL];
};

template <typename T, int IPL>
__device__ __forceinline__ void hnear_reset(HNear<T, IPL>& s) {
#pragma unroll
  for (int k = 0; k < IPL; ++k) {
    s.q[k] = T(INFINITY);
    s.n[k] = -1;
  }
}

template <typename T, int IPL>
__device__ __forceinline__ void hzero(HState<T, IPL>& s) {
#pragma unroll
  for (int k = 0; k < IPL; ++k)
    s.ax[k] = s.ay[k] = s.az[k] = s.ph[k] = s.jx[k] = s.jy[k] = s.jz[k] = T(0);
}

template <typename T, int IPL, bool PHI, bool DS = false, bool NN = false>
__device__ __forceinline__ void hinteract_all(HState<T, IPL>& s, const V4<T>& q, const V4<T>& p,
                                              T cut2, T eps2, const V4<T>& l = V4<T>(),
                                              const HLo<T, IPL>& lo = HLo<T, IPL>(),
                                              HNear<T, IPL>* nr = nullptr, bool jreal = false,
                                              int32_t jg = 0) {
  if constexpr (sizeof(T) == 4 && IPL % 2 == 0) {
#pragma unroll
    for (int k = 0; k < IPL; k += 2) {
      f2 ax = {s.ax[k], s.ax[k + 1]}, ay = {s.ay[k], s.ay[k + 1]}, az = {s.az[k], s.az[k + 1]};
      f2 jx = {s.jx[k], s.jx[k + 1]}, jy = {s.jy[k], s.jy[k + 1]}, jz = {s.jz[k], s.jz[k + 1]};
      f2 ph = {s.ph[k], s.ph[k + 1]};
      if constexpr (NN)
        hinteract_pk<PHI, DS, true>(
            f2{s.x[k], s.x[k + 1]}, f2{s.y[k], s.y[k + 1]}, f2{s.z[k], s.z[k + 1]},
            f2{s.u[k], s.u[k + 1]}, f2{s.v[k], s.v[k + 1]}, f2{s.w[k], s.w[k + 1]}, q, p, cut2,
            eps2, ax, ay, az, ph, jx, jy, jz, l, f2{lo.x[k], lo.x[k + 1]},
            f2{lo.y[k], lo.y[k + 1]}, f2{lo.z[k], lo.z[k + 1]}, f2{nr->r[k], nr->r[k + 1]}, jreal,
            jg, &nr->self[k], &nr->q[k], &nr->n[k]);
      else
        hinteract_pk<PHI, DS>(
            f2{s.x[k], s.x[k + 1]}, f2{s.y[k], s.y[k + 1]}, f2{s.z[k], s.z[k + 1]},
            f2{s.u[k], s.u[k + 1]}, f2{s.v[k], s.v[k + 1]}, f2{s.w[k], s.w[k + 1]}, q, p, cut2,
            eps2, ax, ay, az, ph, jx, jy, jz, l, f2{lo.x[k], lo.x[k + 1]},
            f2{lo.y[k], lo.y[k + 1]}, f2{lo.z[k], lo.z[k + 1]});
      s.ax[k] = ax.x; s.ax[k + 1] = ax.y;
      s.ay[k] = ay.x; s.ay[k + 1] = ay.y;
      s.az[k] = az.x; s.az[k + 1] = az.y;
      s.jx[k] = jx.x; s.jx[k + 1] = jx.y;
      s.jy[k] = jy.x; s.jy[k + 1] = jy.y;
      s.jz[k] = jz.x; s.jz[k + 1] = jz.y;
      s.ph[k] = ph.x; s.ph[k + 1] = ph.y;
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < IPL; ++k) {
    if constexpr (NN)
      hinteract<T, PHI, DS, true>(s.x[k], s.y[k], s.z[k], s.u[k], s.v[k], s.w[k], q, p, cut2, eps2,
                                  s.ax[k], s.ay[k], s.az[k], s.ph[k], s.jx[k], s.jy[k], s.jz[k],
                                  l, lo.x[k], lo.y[k], lo.z[k], nr->r[k], jreal, jg, nr->self[k],
                                  &nr->q[k], &nr->n[k]);
    else
      hinteract<T, PHI, DS>(s.x[k], s.y[k], s.z[k], s.u[k], s.v[k], s.w[k], q, p, cut2, eps2,
                            s.ax[k], s.ay[k], s.az[k], s.ph[k], s.jx[k], s.jy[k], s.jz[k], l,
                            lo.x[k], lo.y[k], lo.z[k]);
  }
}

// EVALUATE: grid (n_pad / (256 IPL), groups). Workgroup (b, g) sweeps the chunks of group g and
// stores one partial per chunk: PA[c][i] = (ax, ay, az, sum mu/r), PJ[c][i] = (jx, jy, jz, 0).
// GATHER (a block step's wide path): lane slot s owns body list[s], the partials are stored per
// slot and i-blocks beyond n_act exit; the j loop, hence a body's bits, is the same.
// Mixed precision (S is not T): a third tile carries the lo rows XL, the lane keeps the lo rows
// of its i-bodies, and only the separation differs (hsep).
// NN: the lane also keeps the nearest neighbour (smallest q, lowest j on a tie) of each of its
// i-bodies over the chunk; the partial is (PJ[c][i].w, PN[c][i]). j is uniform over the wave, so
// the ghost-row test is a scalar compare.
// SLICE (a rank of a multi-rank run): the i-rows are the rank's own, a.row0 + [0, a.n_loc), which
// the grid's x extent covers; the partials are indexed by local row with stride a.n_loc. The j
// sweep is the same, so a body's bits are those of the one-rank run.
template <typename T, int IPL, bool PHI, bool GATHER = false, typename S = T, bool NN = false,
          bool SLICE = false>
__global__ __launch_bounds__(kBlock) void hermite_eval_kernel(HArgs<T, S> a, int gated) {
  constexpr bool DS = sizeof(S) != sizeof(T);
  constexpr int TB = Tile<T>::kBodies;
  __shared__ __attribute__((aligned(16))) V4<T> tx[2][TB];
  __shared__ __attribute__((aligned(16))) V4<T> tv[2][TB];
  __shared__ __attribute__((aligned(16))) V4<T> tl[2][DS ? TB : 1];
  if (gated && !a.ctrl->active) return;  // the run has reached t_end: a no-op step
  const int64_t ib = (int64_t)blockIdx.x * (kBlock * IPL);  // (SLICE: counted from a.row0)
  int64_t n_act = 0;
  if constexpr (GATHER) {
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
  V4<T>* PA = reinterpret_cast<V4<T>*>(a.PA);
  V4<T>* PJ = reinterpret_cast<V4<T>*>(a.PJ);
  const V4<T>* XL = reinterpret_cast<const V4<T>*>(a.XL);
  HState<T, IPL> st;
  HLo<T, IPL> lo;
  HNear<T, IPL> nr;
#pragma unroll
  for (int k = 0; k < IPL; ++k) {
    int64_t row = ib + threadIdx.x + k * kBlock;
    if constexpr (SLICE) row += a.row0;
    if constexpr (GATHER) row = a.blk.list[row < n_act ? row : n_act - 1];  // (spare slots: a copy)
    const V4<T> x = XP[row];
    const V4<T> v = VP[row];
    st.x[k] = x.x; st.y[k] = x.y; st.z[k] = x.z;
    st.u[k] = v.x; st.v[k] = v.y; st.w[k] = v.z;
    if constexpr (NN) {
      nr.r[k] = v.w;
      nr.self[k] = (int32_t)row;
    }
    if constexpr (DS) {
      const V4<T> l = XL[row];
      lo.x[k] = l.x; lo.y[k] = l.y; lo.z[k] = l.z;
    }
  }
  auto fill = [&](int t) {
    const int64_t j0 = (int64_t)(c0 + t / tpc) * a.chunk + (int64_t)(t % tpc) * TB;
    tile_fill<T>(XP + j0, tx[t & 1]);
    tile_fill<T>(VP + j0, tv[t & 1]);
    if constexpr (DS) tile_fill<T>(XL + j0, tl[t & 1]);
  };
  fill(0);
  hzero<T, IPL>(st);
  if constexpr (NN) hnear_reset<T, IPL>(nr);
  for (int t = 0; t < ntiles; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // tile t is in LDS for every wave; buffer (t+1)&1 is free
    if (t + 1 < ntiles) fill(t + 1);
    const V4<T>* cx = tx[t & 1];
    const V4<T>* cv = tv[t & 1];
    const V4<T>* cl = tl[t & 1];
    if constexpr (NN) {
      const int32_t jb = (int32_t)((int64_t)(c0 + t / tpc) * a.chunk + (int64_t)(t % tpc) * TB);
      const int32_t nreal = (int32_t)a.n_real;
#pragma unroll 4
      for (int j = 0; j < TB; ++j) {
        const V4<T> q = cx[j], p = cv[j];
        const int32_t jg = jb + j;
        if constexpr (DS)
          hinteract_all<T, IPL, PHI, true, true>(st, q, p, a.cut2, a.eps2, cl[j], lo, &nr,
                                                 jg < nreal, jg);
        else
          hinteract_all<T, IPL, PHI, false, true>(st, q, p, a.cut2, a.eps2, V4<T>(),
                                                  HLo<T, IPL>(), &nr, jg < nreal, jg);
      }
    } else {
#pragma unroll 4
      for (int j = 0; j < TB; ++j) {
        const V4<T> q = cx[j], p = cv[j];  // uniform addresses: broadcast ds_reads
        if constexpr (DS)
          hinteract_all<T, IPL, PHI, true>(st, q, p, a.cut2, a.eps2, cl[j], lo);
        else
          hinteract_all<T, IPL, PHI>(st, q, p, a.cut2, a.eps2);
      }
    }
    if ((t + 1) % tpc == 0) {
      const int c = c0 + t / tpc;
#pragma unroll
      for (int k = 0; k < IPL; ++k) {
        V4<T> oa, oj;
        oa.x = st.ax[k]; oa.y = st.ay[k]; oa.z = st.az[k]; oa.w = st.ph[k];
        oj.x = st.jx[k]; oj.y = st.jy[k]; oj.z = st.jz[k]; oj.w = T(0);
        if constexpr (NN) {
          oj.w = nr.q[k];
          a.PN[(int64_t)c * a.n_pad + ib + threadIdx.x + k * kBlock] = nr.n[k];
        }
        if constexpr (SLICE) {
          PA[(int64_t)c * a.n_loc + ib + threadIdx.x + k * kBlock] = oa;
          PJ[(int64_t)c * a.n_loc + ib + threadIdx.x + k * kBlock] = oj;
        } else {
          PA[(int64_t)c * a.n_pad + ib + threadIdx.x + k * kBlock] = oa;
          PJ[(int64_t)c * a.n_pad + ib + threadIdx.x + k * kBlock] = oj;
        }
      }
      hzero<T, IPL>(st);
      if constexpr (NN) hnear_reset<T, IPL>(nr);
    }
  }
}

__device__ __forceinline__ double wave_min(double v) {
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_down(v, off, 64));
  return v;
}

// Minimum over the workgroup's threads (valid in thread 0).
__device__ __forceinline__ double block_min(double v, double* red) {
  v = wave_min(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kBlock / 64; ++w) v = fmin(v, red[w]);
  return v;
}

// CONTROL (one workgroup): the step the chain is about to take. h = min(dt_max, min_i dt_i)
// from the last reduce's per-workgroup minima (adaptive) or dt_max (fixed), cut to t_end - t;
// once t >= t_end, or (collisions "stop") once a step has seen an overlap, the chain's other
// kernels return at once and nothing is counted.
__global__ __launch_bounds__(kBlock) void hermite_ctrl_kernel(HermiteCtrl* ctrl,
                                                              const double* wgmin, int nwg) {
  __shared__ double red[kBlock / 64];
  double m = INFINITY;
  for (int k = threadIdx.x; k < nwg; k += kBlock) m = fmin(m, wgmin[k]);
  m = block_min(m, red);
  if (threadIdx.x != 0) return;
  HermiteCtrl c = *ctrl;
  if ((c.has_end && c.t >= c.t_end) || (c.ov_stop && c.overlaps != 0)) {
    ctrl->active = 0;  // (an overlap seen by the last reduce: the run stops at that step)
    return;
  }
  double h = c.dt_max;
  if (c.eta > 0.0 && m < h) h = m;
  bool cut = false;
  if (c.has_end && h >= c.t_end - c.t) {
    h = c.t_end - c.t;
    cut = true;
  }
  c.h = h;
  c.t = cut ? c.t_end : c.t + h;
  c.dt_last = h;
  if (!cut && h < c.dt_min) c.dt_min = h;
  c.steps += 1;
  c.active = 1;
  *ctrl = c;
}

// PREDICT: xp = x + v h + a h^2/2 + j h^3/6, vp = v + a h + j h^2/2 (ghost rows stay zero).
// Store row i of the predicted state for the evaluate kernels: as it is, or (mixed precision,
// S is not T) the position split into XP = (float(xp), mu), XL = (float(xp - double(hi)), 0).
// NN: the spare component of the VP row carries the body's radius (R, state precision).
template <typename T, typename S, bool NN = false>
__device__ __forceinline__ void store_predicted(const HArgs<T, S>& a, int64_t i, const V4<S>& xp,
                                                const V4<S>& vp) {
  V4<T> h, v;
  h.x = (T)xp.x; h.y = (T)xp.y; h.z = (T)xp.z; h.w = (T)xp.w;
  v.x = (T)vp.x; v.y = (T)vp.y; v.z = (T)vp.z; v.w = T(0);
  if constexpr (NN) v.w = (T)a.R[i];
  reinterpret_cast<V4<T>*>(a.XP)[i] = h;
  reinterpret_cast<V4<T>*>(a.VP)[i] = v;
  if constexpr (sizeof(S) != sizeof(T)) {
    V4<T> l;
    l.x = (T)(xp.x - (S)h.x); l.y = (T)(xp.y - (S)h.y); l.z = (T)(xp.z - (S)h.z); l.w = T(0);
    reinterpret_cast<V4<T>*>(a.XL)[i] = l;
  }
}

// SLICE: the grid covers the rank's rows a.row0 + [0, a.n_loc) of the full-length XP, VP (XL).
template <typename T, typename S, bool NN = false, bool SLICE = false>
__global__ __launch_bounds__(kBlock) void hermite_predict_kernel(HArgs<T, S> a) {
  if (!a.ctrl->active) return;
  const int64_t i = (SLICE ? a.row0 : 0) + (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n_pad) return;
  V4<S> xp = {S(0), S(0), S(0), S(0)}, vp = xp;
  if (i < a.n_real) {
    const S h = (S)a.ctrl->h;
    const S h2 = (h * h) / S(2), h3 = (h * h * h) / S(6);
    const V4<S> x = reinterpret_cast<const V4<S>*>(a.X)[i];
    const V4<S> v = reinterpret_cast<const V4<S>*>(a.V)[i];
    const V4<S> ac = reinterpret_cast<const V4<S>*>(a.A)[i];
    const V4<S> jk = reinterpret_cast<const V4<S>*>(a.J)[i];
    xp.x = x.x + (v.x * h + (ac.x * h2 + jk.x * h3));
    xp.y = x.y + (v.y * h + (ac.y * h2 + jk.y * h3));
    xp.z = x.z + (v.z * h + (ac.z * h2 + jk.z * h3));
    xp.w = x.w;
    vp.x = v.x + (ac.x * h + jk.x * h2);
    vp.y = v.y + (ac.y * h + jk.y * h2);
    vp.z = v.z + (ac.z * h + jk.z * h2);
  }
  store_predicted<T, S, NN>(a, i, xp, vp);
}

// SPLIT (mixed precision): the predictor's output at h = 0, for the derivatives of the current
// state (ghost rows of X, V are zero).
__global__ __launch_bounds__(kBlock) void hermite_split_kernel(HArgs<float, double> a) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n_pad) return;
  store_predicted<float, double>(a, i, reinterpret_cast<const V4<double>*>(a.X)[i],
                                 reinterpret_cast<const V4<double>*>(a.V)[i]);
}

// STAGE (collisions on): XP, VP (and XL) <- the current X, V with the radius in VP's spare
// component, for an evaluation of the current state in any precision.
template <typename T, typename S>
__global__ __launch_bounds__(kBlock) void hermite_stage_kernel(HArgs<T, S> a) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n_pad) return;
  store_predicted<T, S, true>(a, i, reinterpret_cast<const V4<S>*>(a.X)[i],
                              reinterpret_cast<const V4<S>*>(a.V)[i]);
}

// The latest (q, nn) of body i, its closest-approach record since the last clear, and the
// overlap count (q < eps2, that is |d|^2 < (R_i + R_j)^2) of the control block.
template <typename T, typename S>
__device__ __forceinline__ void nn_record(const HArgs<T, S>& a, int64_t i, T q, int32_t nn,
                                          unsigned long long* overlaps) {
  a.nn_q[i] = (double)q;
  a.nn_i[i] = nn;
  if ((double)q < a.ca_q[i]) {
    a.ca_q[i] = (double)q;
    a.ca_i[i] = nn;
  }
  if (q < a.eps2) atomicAdd(overlaps, 1ull);
}

__device__ __forceinline__ double norm3(double x, double y, double z) {
  return sqrt(x * x + y * y + z * z);
}

// REDUCE (+ CORRECT): one thread per body adds its chunk partials in chunk order, then
// HM_STEP applies the corrector and Aarseth's criterion, HM_INIT starts a run from (x, v),
// HM_OUT returns the derivatives. Per-workgroup dt minima go to wgmin (+inf when no body of the
// workgroup takes part: ghost rows, |j| = 0, a non-finite ratio, or a fixed-step run).
// NN: the chunks' (q, j) partials fold with a strict less in chunk order (the lowest j keeps a
// tie); HM_OUT writes them to q_out / nn_out, the other modes record them (nn_record).
// SLICE: the grid covers the rank's rows; it reads the rank's partials [n_chunks][n_loc] and
// writes the rows' entries of the full-length X, V, A, J, outputs and wgmin.
template <typename T, typename S, bool NN = false, bool SLICE = false>
__global__ __launch_bounds__(kBlock) void hermite_reduce_kernel(HArgs<T, S> a) {
  __shared__ double red[kBlock / 64];
  if (a.mode == HM_STEP && !a.ctrl->active) return;
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;  // (n_pad is a multiple of 256)
  const int64_t li = i;  // the row's slot in the partials
  int64_t pstride = a.n_pad;
  if constexpr (SLICE) {
    i += a.row0;
    pstride = a.n_loc;
  }
  const V4<T>* PA = reinterpret_cast<const V4<T>*>(a.PA);
  const V4<T>* PJ = reinterpret_cast<const V4<T>*>(a.PJ);
  S a1x = 0, a1y = 0, a1z = 0, sp = 0, j1x = 0, j1y = 0, j1z = 0;
  T bq = T(INFINITY);
  int32_t bn = -1;
  for (int c = 0; c < a.n_chunks; ++c) {
    const V4<T> pa = PA[(int64_t)c * pstride + li];
    const V4<T> pj = PJ[(int64_t)c * pstride + li];
    a1x += pa.x; a1y += pa.y; a1z += pa.z; sp += pa.w;
    j1x += pj.x; j1y += pj.y; j1z += pj.z;
    if constexpr (NN) {
      if (pj.w < bq) {
        bq = pj.w;
        bn = a.PN[(int64_t)c * pstride + li];
      }
    }
  }
  if (a.mode == HM_OUT) {
    V4<S> oa, oj;
    oa.x = a1x; oa.y = a1y; oa.z = a1z; oa.w = -sp;
    oj.x = j1x; oj.y = j1y; oj.z = j1z; oj.w = S(0);
    reinterpret_cast<V4<S>*>(a.a_out)[i] = oa;
    reinterpret_cast<V4<S>*>(a.j_out)[i] = oj;
    if constexpr (NN) {
      a.q_out[i] = (double)bq;
      a.nn_out[i] = bn;
    }
    return;
  }
  if constexpr (NN) {
    if (i < a.n_real) nn_record<T, S>(a, i, bq, bn, &a.ctrl->overlaps);
  }
  V4<S>* A = reinterpret_cast<V4<S>*>(a.A);
  V4<S>* J = reinterpret_cast<V4<S>*>(a.J);
  const double eta = a.ctrl->eta;
  double dti = INFINITY;
  if (i >= a.n_real) {
    const V4<S> z = {S(0), S(0), S(0), S(0)};
    A[i] = z;
    J[i] = z;
    if (a.mode == HM_STEP) {
      reinterpret_cast<V4<S>*>(a.X)[i] = z;
      reinterpret_cast<V4<S>*>(a.V)[i] = z;
    }
  } else if (a.mode == HM_INIT) {
    if (eta > 0.0) {
      const double an = norm3(a1x, a1y, a1z), jn = norm3(j1x, j1y, j1z);
      const double d = 0.5 * eta * an / jn;
      if (jn > 0.0 && isfinite(d)) dti = d;
    }
  } else {
    const double hd = a.ctrl->h;
    const S h = (S)hd;
    const S hh = h / S(2), h12 = (h * h) / S(12);
    V4<S>* X = reinterpret_cast<V4<S>*>(a.X);
    V4<S>* V = reinterpret_cast<V4<S>*>(a.V);
    const V4<S> x = X[i], v = V[i], a0 = A[i], j0 = J[i];
    V4<S> v1, x1;
    v1.x = v.x + ((a0.x + a1x) * hh + (j0.x - j1x) * h12);
    v1.y = v.y + ((a0.y + a1y) * hh + (j0.y - j1y) * h12);
    v1.z = v.z + ((a0.z + a1z) * hh + (j0.z - j1z) * h12);
    v1.w = S(0);
    x1.x = x.x + ((v.x + v1.x) * hh + (a0.x - a1x) * h12);
    x1.y = x.y + ((v.y + v1.y) * hh + (a0.y - a1y) * h12);
    x1.z = x.z + ((v.z + v1.z) * hh + (a0.z - a1z) * h12);
    x1.w = x.w;
    X[i] = x1;
    V[i] = v1;
    if (eta > 0.0) {
      // Aarseth's criterion from the 2nd and 3rd derivatives the two evaluations imply
      const double ih = 1.0 / hd, ih2 = ih * ih, ih3 = ih2 * ih;
      const double da[3] = {(double)a0.x - (double)a1x, (double)a0.y - (double)a1y,
                            (double)a0.z - (double)a1z};
      const double jo[3] = {j0.x, j0.y, j0.z}, jn[3] = {j1x, j1y, j1z};
      double s2[3], s3[3];
      for (int d = 0; d < 3; ++d) {
        const double a2 = (-6.0 * da[d] - hd * (4.0 * jo[d] + 2.0 * jn[d])) * ih2;
        s3[d] = (12.0 * da[d] + 6.0 * hd * (jo[d] + jn[d])) * ih3;
        s2[d] = a2 + hd * s3[d];
      }
      const double an = norm3(a1x, a1y, a1z), jnn = norm3(j1x, j1y, j1z);
      const double n2 = norm3(s2[0], s2[1], s2[2]), n3 = norm3(s3[0], s3[1], s3[2]);
      const double d = sqrt(eta * (an * n2 + jnn * jnn) / (jnn * n3 + n2 * n2));
      if (jnn > 0.0 && isfinite(d)) dti = d;
    }
  }
  if (i < a.n_real) {
    V4<S> oa, oj;
    oa.x = a1x; oa.y = a1y; oa.z = a1z; oa.w = S(0);
    oj.x = j1x; oj.y = j1y; oj.z = j1z; oj.w = S(0);
    A[i] = oa;
    J[i] = oj;
  }
  dti = block_min(dti, red);
  if (threadIdx.x == 0) a.wgmin[(SLICE ? a.row0 / kBlock : 0) + blockIdx.x] = dti;
}


// ---------------------------------------------------------------------------------------
// Block time steps: body i stands at tb_i ticks and steps by 2^(L - level_i) ticks.

__device__ __forceinline__ int64_t wave_min_i64(int64_t v) {
  for (int off = 32; off > 0; off >>= 1) {
    const long long o = __shfl_down((long long)v, off, 64);
    v = o < v ? (int64_t)o : v;
  }
  return v;
}

__device__ __forceinline__ int wave_sum_i32(int v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// Seconds of a span of ticks: dt_max ticks 2^-L in fp64 (the run's dtype takes a cast of it).
__device__ __forceinline__ double ticks_seconds(double dt_max, int64_t ticks, int L) {
  return dt_max * ldexp((double)ticks, -L);
}

__device__ __forceinline__ bool body_due(const HBlock& b, int64_t i, int L, int64_t t_next) {
  return b.tb[i] + ((int64_t)1 << (L - b.level[i])) == t_next;
}

// NEXT, stage 1: per-workgroup minimum of tb + step over the real bodies.
template <typename T, typename S>
__global__ __launch_bounds__(kBlock) void block_next_kernel(HArgs<T, S> a) {
  __shared__ int64_t red[kBlock / 64];
  const HBlock& b = a.blk;
  const int L = b.bc->L;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  int64_t v = INT64_MAX;
  if (i < a.n_real) v = b.tb[i] + ((int64_t)1 << (L - b.level[i]));
  v = wave_min_i64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kBlock / 64; ++w) v = red[w] < v ? red[w] : v;
    b.wgnext[blockIdx.x] = v;
  }
}

// NEXT, stage 2 and CONTROL (one workgroup): t_next = the earliest due time; past the target the
// chain's other kernels return at once.
__global__ __launch_bounds__(kBlock) void block_ctrl_kernel(HermiteBlockCtrl* bc,
                                                            const int64_t* wgnext, int nwg) {
  __shared__ int64_t red[kBlock / 64];
  int64_t m = INT64_MAX;
  for (int k = threadIdx.x; k < nwg; k += kBlock) m = wgnext[k] < m ? wgnext[k] : m;
  m = wave_min_i64(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int w = 1; w < kBlock / 64; ++w) m = red[w] < m ? red[w] : m;
  if (bc->t_ticks >= bc->target || m > bc->target) {
    bc->active = 0;
    return;
  }
  bc->t_ticks = m;
  bc->n_act = 0;
  bc->path = 0;
  bc->active = 1;
}

// PREDICT-ALL + MARK: every real body from its own tb to t_next; counts the due bodies of the
// workgroup for the compaction.
template <typename T, typename S, bool NN = false>
__global__ __launch_bounds__(kBlock) void block_predict_kernel(HArgs<T, S> a) {
  __shared__ int cnt[kBlock / 64];
  const HBlock& b = a.blk;
  if (!b.bc->active) return;
  const int L = b.bc->L;
  const int64_t t_next = b.bc->t_ticks;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;  // (n_pad: a multiple of 256)
  V4<S> xp = {S(0), S(0), S(0), S(0)}, vp = xp;
  bool due = false;
  if (i < a.n_real) {
    due = body_due(b, i, L, t_next);
    const S h = (S)ticks_seconds(b.bc->dt_max, t_next - b.tb[i], L);
    const S h2 = (h * h) / S(2), h3 = (h * h * h) / S(6);
    const V4<S> x = reinterpret_cast<const V4<S>*>(a.X)[i];
    const V4<S> v = reinterpret_cast<const V4<S>*>(a.V)[i];
    const V4<S> ac = reinterpret_cast<const V4<S>*>(a.A)[i];
    const V4<S> jk = reinterpret_cast<const V4<S>*>(a.J)[i];
    xp.x = x.x + (v.x * h + (ac.x * h2 + jk.x * h3));
    xp.y = x.y + (v.y * h + (ac.y * h2 + jk.y * h3));
    xp.z = x.z + (v.z * h + (ac.z * h2 + jk.z * h3));
    xp.w = x.w;
    vp.x = v.x + (ac.x * h + jk.x * h2);
    vp.y = v.y + (ac.y * h + jk.y * h2);
    vp.z = v.z + (ac.z * h + jk.z * h2);
  }
  store_predicted<T, S, NN>(a, i, xp, vp);
  const int c = __popcll(__ballot(due));
  if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) b.wgcount[blockIdx.x] = cnt[0] + cnt[1] + cnt[2] + cnt[3];
}

// COMPACT: the due bodies in ascending order, by a scan (workgroup offset = sum of the counts of
// the workgroups before it; ballot prefix inside): no atomic append, so the list is the
// oracle's. The last workgroup publishes n_act and picks the evaluate path.
template <typename T, typename S>
__global__ __launch_bounds__(kBlock) void block_compact_kernel(HArgs<T, S> a) {
  __shared__ int red[kBlock / 64];
  __shared__ int cnt[kBlock / 64];
  const HBlock& b = a.blk;
  HermiteBlockCtrl* bc = b.bc;
  if (!bc->active) return;
  int s = 0;
  for (int k = threadIdx.x; k < (int)blockIdx.x; k += kBlock) s += b.wgcount[k];
  s = wave_sum_i32(s);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool due = i < a.n_real && body_due(b, i, bc->L, bc->t_ticks);
  const unsigned long long mask = __ballot(due);
  if (lane == 0) {
    red[wave] = s;
    cnt[wave] = __popcll(mask);
  }
  __syncthreads();
  const int base = red[0] + red[1] + red[2] + red[3];
  int off = base;
  for (int w = 0; w < wave; ++w) off += cnt[w];
  if (due) b.list[off + __popcll(mask & ((1ull << lane) - 1ull))] = (int32_t)i;
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    const int n_act = base + cnt[0] + cnt[1] + cnt[2] + cnt[3];
    bc->n_act = n_act;
    bc->path = n_act <= bc->narrow_max ? HP_NARROW : HP_WIDE;
    bc->block_steps += 1;
    bc->body_steps += (unsigned long long)n_act;
  }
}

// NARROW EVALUATE (n_act <= narrow_max): parallel over j. Grid (n_slices, passes): workgroup
// (s, y) takes the j rows of slice s and the groups y, y + passes, ... of kNarrowGroup active
// bodies. The group's predicted rows are wave-uniform (broadcast operands); the lanes stride
// over the slice with coalesced 16-byte loads of (XP, VP), each summing its rows from zero in
// j order; the lanes are folded by a fixed tree (shuffle-down 32..1 in the wave, then the
// four waves in order through LDS) and one partial per (slice, slot) is stored. Slice length and
// tree depend on n_pad only, so a body's bits depend neither on the other active bodies nor on
// its slot. fp32 runs two i-bodies as 2-vectors (hinteract_pk).
// NN: a lane folds its rows with a strict less in j order; the lanes' and the waves' (q, j) fold
// lexicographically (the smaller q, on a tie the lower j); the partial is (NJ[s][slot].w,
// NNI[s][slot]).
template <typename T, bool PHI, typename S = T, bool NN = false>
__global__ __launch_bounds__(kBlock) void hermite_narrow_kernel(HArgs<T, S> a) {
  constexpr bool DS = sizeof(S) != sizeof(T);
  constexpr int G = kNarrowGroup;
  __shared__ T red[kBlock / 64][G][8];
  __shared__ int32_t redn[kBlock / 64][NN ? G : 1];
  const HBlock& b = a.blk;
  if (!b.bc->active || b.bc->path != HP_NARROW) return;
  const int n_act = min(b.bc->n_act, b.cap);
  const int ngroups = (n_act + G - 1) / G;
  const int64_t j0 = (int64_t)blockIdx.x * b.slice;
  const int64_t j1 = min(j0 + (int64_t)b.slice, a.n_pad);
  const V4<T>* XP = reinterpret_cast<const V4<T>*>(a.XP);
  const V4<T>* VP = reinterpret_cast<const V4<T>*>(a.VP);
  V4<T>* NA = reinterpret_cast<V4<T>*>(b.NA);
  V4<T>* NJ = reinterpret_cast<V4<T>*>(b.NJ);
  const V4<T>* XL = reinterpret_cast<const V4<T>*>(a.XL);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int g = blockIdx.y; g < ngroups; g += (int)gridDim.y) {
    HState<T, G> st;
    HLo<T, G> lo;
    HNear<T, G> nr;
#pragma unroll
    for (int k = 0; k < G; ++k) {
      const int slot = min(g * G + k, n_act - 1);  // (spare slots of the last group: a copy)
      const int64_t row = b.list[slot];
      const V4<T> x = XP[row];
      const V4<T> v = VP[row];
      st.x[k] = x.x; st.y[k] = x.y; st.z[k] = x.z;
      st.u[k] = v.x; st.v[k] = v.y; st.w[k] = v.z;
      if constexpr (NN) {
      nr.r[k] = v.w;
      nr.self[k] = (int32_t)row;
    }
      if constexpr (DS) {
        const V4<T> l = XL[row];
        lo.x[k] = l.x; lo.y[k] = l.y; lo.z[k] = l.z;
      }
    }
    hzero<T, G>(st);
    if constexpr (NN) hnear_reset<T, G>(nr);
    for (int64_t j = j0 + threadIdx.x; j < j1; j += kBlock) {
      const V4<T> q = XP[j], p = VP[j];
      if constexpr (NN) {
        if constexpr (DS)
          hinteract_all<T, G, PHI, true, true>(st, q, p, a.cut2, a.eps2, XL[j], lo, &nr,
                                               j < a.n_real, (int32_t)j);
        else
          hinteract_all<T, G, PHI, false, true>(st, q, p, a.cut2, a.eps2, V4<T>(), HLo<T, G>(),
                                                &nr, j < a.n_real, (int32_t)j);
      } else if constexpr (DS) {
        hinteract_all<T, G, PHI, true>(st, q, p, a.cut2, a.eps2, XL[j], lo);
      } else {
        hinteract_all<T, G, PHI>(st, q, p, a.cut2, a.eps2);
      }
    }
#pragma unroll
    for (int k = 0; k < G; ++k) {
      T v[7] = {st.ax[k], st.ay[k], st.az[k], st.ph[k], st.jx[k], st.jy[k], st.jz[k]};
#pragma unroll
      for (int c = 0; c < 7; ++c) {
        for (int off = 32; off > 0; off >>= 1) v[c] += __shfl_down(v[c], off, 64);
        if (lane == 0) red[wave][k][c] = v[c];
      }
      if constexpr (NN) {
        T bq = nr.q[k];
        int32_t bn = nr.n[k];
        for (int off = 32; off > 0; off >>= 1) {
          const T oq = __shfl_down(bq, off, 64);
          const int32_t on = __shfl_down(bn, off, 64);
          const bool take = oq < bq || (oq == bq && on < bn);
          bq = take ? oq : bq;
          bn = take ? on : bn;
        }
        if (lane == 0) {
          red[wave][k][7] = bq;
          redn[wave][k] = bn;
        }
      }
    }
    __syncthreads();
    if (threadIdx.x < G && g * G + (int)threadIdx.x < n_act) {
      const int k = threadIdx.x;
      T v[7];
#pragma unroll
      for (int c = 0; c < 7; ++c) v[c] = ((red[0][k][c] + red[1][k][c]) + red[2][k][c]) + red[3][k][c];
      V4<T> oa, oj;
      oa.x = v[0]; oa.y = v[1]; oa.z = v[2]; oa.w = v[3];
      oj.x = v[4]; oj.y = v[5]; oj.z = v[6]; oj.w = T(0);
      const int64_t o = (int64_t)blockIdx.x * b.cap + (g * G + k);
      if constexpr (NN) {
        T bq = red[0][k][7];
        int32_t bn = redn[0][k];
#pragma unroll
        for (int w = 1; w < kBlock / 64; ++w) {
          const T oq = red[w][k][7];
          const int32_t on = redn[w][k];
          const bool take = oq < bq || (oq == bq && on < bn);
          bq = take ? oq : bq;
          bn = take ? on : bn;
        }
        oj.w = bq;
        a.NNI[o] = bn;
      }
      NA[o] = oa;
      NJ[o] = oj;
    }
    __syncthreads();
  }
}

// REDUCE + CORRECT + NEW LEVEL, one thread per slot of the active list: the slice partials in
// slice order (narrow) or the chunk partials in chunk order (wide), then the corrector over the
// body's own h, Aarseth's dt_want and the level rule: any number of halvings (capped at L), at
// most one doubling and only where t_next allows the doubled step. HM_OUT: the sums go to
// a_out / j_out [slot] and nothing else is touched.
template <typename T, typename S, bool NN = false>
__global__ __launch_bounds__(kBlock) void block_correct_kernel(HArgs<T, S> a) {
  const HBlock& b = a.blk;
  HermiteBlockCtrl* bc = b.bc;
  if (!bc->active) return;
  const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (s >= bc->n_act) return;
  S a1x = 0, a1y = 0, a1z = 0, sp = 0, j1x = 0, j1y = 0, j1z = 0;
  T bq = T(INFINITY);
  int32_t bn = -1;
  if (bc->path == HP_NARROW) {
    const V4<T>* NA = reinterpret_cast<const V4<T>*>(b.NA);
    const V4<T>* NJ = reinterpret_cast<const V4<T>*>(b.NJ);
#pragma unroll 8
    for (int c = 0; c < b.n_slices; ++c) {  // (unrolled: the loads of 8 slices are in flight)
      const V4<T> pa = NA[(int64_t)c * b.cap + s];
      const V4<T> pj = NJ[(int64_t)c * b.cap + s];
      a1x += pa.x; a1y += pa.y; a1z += pa.z; sp += pa.w;
      j1x += pj.x; j1y += pj.y; j1z += pj.z;
      if constexpr (NN) {
        if (pj.w < bq) {
          bq = pj.w;
          bn = a.NNI[(int64_t)c * b.cap + s];
        }
      }
    }
  } else {
    const V4<T>* PA = reinterpret_cast<const V4<T>*>(a.PA);
    const V4<T>* PJ = reinterpret_cast<const V4<T>*>(a.PJ);
    for (int c = 0; c < a.n_chunks; ++c) {
      const V4<T> pa = PA[(int64_t)c * a.n_pad + s];
      const V4<T> pj = PJ[(int64_t)c * a.n_pad + s];
      a1x += pa.x; a1y += pa.y; a1z += pa.z; sp += pa.w;
      j1x += pj.x; j1y += pj.y; j1z += pj.z;
      if constexpr (NN) {
        if (pj.w < bq) {
          bq = pj.w;
          bn = a.PN[(int64_t)c * a.n_pad + s];
        }
      }
    }
  }
  if (a.mode == HM_OUT) {
    V4<S> oa, oj;
    oa.x = a1x; oa.y = a1y; oa.z = a1z; oa.w = -sp;
    oj.x = j1x; oj.y = j1y; oj.z = j1z; oj.w = S(0);
    reinterpret_cast<V4<S>*>(a.a_out)[s] = oa;
    reinterpret_cast<V4<S>*>(a.j_out)[s] = oj;
    if constexpr (NN) {
      a.q_out[s] = (double)bq;
      a.nn_out[s] = bn;
    }
    return;
  }
  const int64_t i = b.list[s];
  if constexpr (NN) nn_record<T, S>(a, i, bq, bn, &bc->overlaps);
  const int L = bc->L;
  const int64_t t_next = bc->t_ticks;
  const double dt_max = bc->dt_max, eta = bc->eta;
  const double hd = ticks_seconds(dt_max, t_next - b.tb[i], L);
  const S h = (S)hd;
  const S hh = h / S(2), h12 = (h * h) / S(12);
  V4<S>* X = reinterpret_cast<V4<S>*>(a.X);
  V4<S>* V = reinterpret_cast<V4<S>*>(a.V);
  V4<S>* A = reinterpret_cast<V4<S>*>(a.A);
  V4<S>* J = reinterpret_cast<V4<S>*>(a.J);
  const V4<S> x = X[i], v = V[i], a0 = A[i], j0 = J[i];
  V4<S> v1, x1;
  v1.x = v.x + ((a0.x + a1x) * hh + (j0.x - j1x) * h12);
  v1.y = v.y + ((a0.y + a1y) * hh + (j0.y - j1y) * h12);
  v1.z = v.z + ((a0.z + a1z) * hh + (j0.z - j1z) * h12);
  v1.w = S(0);
  x1.x = x.x + ((v.x + v1.x) * hh + (a0.x - a1x) * h12);
  x1.y = x.y + ((v.y + v1.y) * hh + (a0.y - a1y) * h12);
  x1.z = x.z + ((v.z + v1.z) * hh + (a0.z - a1z) * h12);
  x1.w = x.w;
  X[i] = x1;
  V[i] = v1;
  V4<S> oa, oj;
  oa.x = a1x; oa.y = a1y; oa.z = a1z; oa.w = S(0);
  oj.x = j1x; oj.y = j1y; oj.z = j1z; oj.w = S(0);
  A[i] = oa;
  J[i] = oj;
  b.tb[i] = t_next;
  // Aarseth's criterion (as hermite_reduce_kernel), per body
  const double ih = 1.0 / hd, ih2 = ih * ih, ih3 = ih2 * ih;
  const double da[3] = {(double)a0.x - (double)a1x, (double)a0.y - (double)a1y,
                        (double)a0.z - (double)a1z};
  const double jo[3] = {j0.x, j0.y, j0.z}, jn[3] = {j1x, j1y, j1z};
  double s2[3], s3[3];
  for (int d = 0; d < 3; ++d) {
    const double a2 = (-6.0 * da[d] - hd * (4.0 * jo[d] + 2.0 * jn[d])) * ih2;
    s3[d] = (12.0 * da[d] + 6.0 * hd * (jo[d] + jn[d])) * ih3;
    s2[d] = a2 + hd * s3[d];
  }
  const double an = norm3(a1x, a1y, a1z), jnn = norm3(j1x, j1y, j1z);
  const double n2 = norm3(s2[0], s2[1], s2[2]), n3 = norm3(s3[0], s3[1], s3[2]);
  const double want = sqrt(eta * (an * n2 + jnn * jnn) / (jnn * n3 + n2 * n2));
  int k = b.level[i];
  if (jnn > 0.0 && isfinite(want)) {
    const double dtk = ldexp(dt_max, -k);
    if (want < dtk) {
      while (k < L && ldexp(dt_max, -k) > want) ++k;
      if (ldexp(dt_max, -k) > want) atomicAdd(&bc->level_clamped, 1ull);
    } else if (k > 0 && want >= 2.0 * dtk &&
               (t_next & (((int64_t)1 << (L - k + 1)) - 1)) == 0) {
      --k;
    }
  }
  b.level[i] = k;
  if (k > bc->level_max) atomicMax(&bc->level_max, k);
}

// START: the level of every real body from the carried a, j (the smallest k with
// dt_max 2^-k <= (eta / 2) |a| / |j|, capped at L; 0 where |j| = 0 or the ratio is not finite),
// all standing at tick t0.
template <typename T, typename S>
__global__ __launch_bounds__(kBlock) void block_init_kernel(HArgs<T, S> a, int64_t t0) {
  const HBlock& b = a.blk;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n_pad) return;
  int k = 0;
  if (i < a.n_real) {
    const V4<S> ac = reinterpret_cast<const V4<S>*>(a.A)[i];
    const V4<S> jk = reinterpret_cast<const V4<S>*>(a.J)[i];
    const double an = norm3(ac.x, ac.y, ac.z), jn = norm3(jk.x, jk.y, jk.z);
    const double want = 0.5 * b.bc->eta * an / jn;
    if (jn > 0.0 && isfinite(want))
      while (k < b.bc->L && ldexp(b.bc->dt_max, -k) > want) ++k;
    if (k > b.bc->level_max) atomicMax(&b.bc->level_max, k);
  }
  b.tb[i] = t0;
  b.level[i] = k;
}

// ---------------------------------------------------------------------------------------
// Host launchers.

// A rank's slice of a multi-rank run (never with collisions or block steps).
template <typename T, typename S>
static bool is_slice(const HArgs<T, S>& a) { return a.n_loc != a.n_pad; }

template <typename T, typename S, int IPL>
static hipError_t launch_eval_t(const HArgs<T, S>& a, int groups, bool gated, hipStream_t s) {
  if (is_slice(a)) {
    const dim3 grid((unsigned)(a.n_loc / (kBlock * IPL)), (unsigned)groups);
    if (a.phi)
      hipLaunchKernelGGL((hermite_eval_kernel<T, IPL, true, false, S, false, true>), grid,
                         dim3(kBlock), 0, s, a, (int)gated);
    else
      hipLaunchKernelGGL((hermite_eval_kernel<T, IPL, false, false, S, false, true>), grid,
                         dim3(kBlock), 0, s, a, (int)gated);
    return hipGetLastError();
  }
  const dim3 grid((unsigned)(a.n_pad / (kBlock * IPL)), (unsigned)groups);
  // Mixed precision with collisions on would need all 256 VGPRs at 4 i-bodies per lane: that
  // kernel is not built, and the runtime's launch shape never asks for it (hermite.hip).
  constexpr bool kNoNN = IPL == 4 && sizeof(S) != sizeof(T);
  if constexpr (kNoNN) {
    if (a.nn) return hipErrorInvalidValue;
  }
  if constexpr (!kNoNN) {
    if (a.nn) {
      if (a.phi)
        hipLaunchKernelGGL((hermite_eval_kernel<T, IPL, true, false, S, true>), grid,
                           dim3(kBlock), 0, s, a, (int)gated);
      else
        hipLaunchKernelGGL((hermite_eval_kernel<T, IPL, false, false, S, true>), grid,
                           dim3(kBlock), 0, s, a, (int)gated);
      return hipGetLastError();
    }
  }
  if (a.phi)
    hipLaunchKernelGGL((hermite_eval_kernel<T, IPL, true, false, S>), grid, dim3(kBlock), 0, s, a,
                       (int)gated);
  else
    hipLaunchKernelGGL((hermite_eval_kernel<T, IPL, false, false, S>), grid, dim3(kBlock), 0, s, a,
                       (int)gated);
  return hipGetLastError();
}

// The arrays a collisions-on launch writes.
template <typename T, typename S>
static bool nn_args_ok(const HArgs<T, S>& a) {
  return a.R && a.PN && a.nn_q && a.nn_i && a.ca_q && a.ca_i && a.q_out && a.nn_out &&
         a.n_pad <= INT32_MAX;
}

bool hermite_ipl_ok(int fp64, int ipl) { return ipl == 1 || ipl == 2 || (ipl == 4 && !fp64); }

template <typename T, typename S>
hipError_t launch_hermite_eval(const HArgs<T, S>& a, int ipl, int groups, bool gated,
                               hipStream_t s) {
  if (a.n_chunks < 1 || a.n_pad % (kBlock * ipl) || a.chunk % Tile<T>::kBodies ||
      (int64_t)a.n_chunks * a.chunk != a.n_pad || (gated && !a.ctrl) ||
      (sizeof(S) != sizeof(T) && !a.XL) || (a.nn && !nn_args_ok(a)))
    return hipErrorInvalidValue;
  if (a.row0 < 0 || a.n_loc < 1 || a.row0 + a.n_loc > a.n_pad || a.n_loc % (kBlock * ipl) ||
      a.row0 % kBlock || (is_slice(a) && (a.nn || a.blk.bc)))
    return hipErrorInvalidValue;
  if (groups < 1) groups = 1;
  if (groups > a.n_chunks) groups = a.n_chunks;
  switch (ipl) {
    case 1: return launch_eval_t<T, S, 1>(a, groups, gated, s);
    case 2: return launch_eval_t<T, S, 2>(a, groups, gated, s);
    case 4:
      if constexpr (sizeof(T) == 4) return launch_eval_t<T, S, 4>(a, groups, gated, s);
      return hipErrorInvalidValue;
    default: return hipErrorInvalidValue;
  }
}

template <typename T, typename S>
hipError_t launch_hermite_ctrl(const HArgs<T, S>& a, hipStream_t s) {
  hipLaunchKernelGGL(hermite_ctrl_kernel, dim3(1), dim3(kBlock), 0, s, a.ctrl, a.wgmin,
                     (int)(a.n_pad / kBlock));
  return hipGetLastError();
}

template <typename T, typename S>
hipError_t launch_hermite_predict(const HArgs<T, S>& a, hipStream_t s) {
  if (is_slice(a)) {
    if (a.nn || a.row0 < 0 || a.row0 % kBlock || a.n_loc % kBlock || a.row0 + a.n_loc > a.n_pad)
      return hipErrorInvalidValue;
    hipLaunchKernelGGL((hermite_predict_kernel<T, S, false, true>),
                       dim3((unsigned)(a.n_loc / kBlock)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
  }
  if (a.nn)
    hipLaunchKernelGGL((hermite_predict_kernel<T, S, true>), dim3((unsigned)(a.n_pad / kBlock)),
                       dim3(kBlock), 0, s, a);
  else
    hipLaunchKernelGGL((hermite_predict_kernel<T, S>), dim3((unsigned)(a.n_pad / kBlock)),
                       dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_hermite_split(const HArgs<float, double>& a, hipStream_t s) {
  hipLaunchKernelGGL(hermite_split_kernel, dim3((unsigned)(a.n_pad / kBlock)), dim3(kBlock), 0, s,
                     a);
  return hipGetLastError();
}

template <typename T, typename S>
hipError_t launch_hermite_stage(const HArgs<T, S>& a, hipStream_t s) {
  if (!a.R) return hipErrorInvalidValue;
  hipLaunchKernelGGL((hermite_stage_kernel<T, S>), dim3((unsigned)(a.n_pad / kBlock)),
                     dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

template <typename T, typename S>
hipError_t launch_hermite_reduce(const HArgs<T, S>& a, hipStream_t s) {
  if (is_slice(a)) {
    if (a.nn || a.row0 < 0 || a.row0 % kBlock || a.n_loc % kBlock || a.row0 + a.n_loc > a.n_pad)
      return hipErrorInvalidValue;
    hipLaunchKernelGGL((hermite_reduce_kernel<T, S, false, true>),
                       dim3((unsigned)(a.n_loc / kBlock)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
  }
  if (a.nn)
    hipLaunchKernelGGL((hermite_reduce_kernel<T, S, true>), dim3((unsigned)(a.n_pad / kBlock)),
                       dim3(kBlock), 0, s, a);
  else
    hipLaunchKernelGGL((hermite_reduce_kernel<T, S>), dim3((unsigned)(a.n_pad / kBlock)),
                       dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

int32_t hermite_narrow_slice(int64_t n_pad) {
  // At most 64 slices of at least 1024 rows (4 per lane, which amortise the fold of the lanes;
  // 64 partials keep the reduce's chain of dependent adds short): a function of n_pad alone,
  // since it fixes the bits.
  return (int32_t)round_up(n_pad / 64 > 4 * kBlock ? n_pad / 64 : 4 * kBlock, kBlock);
}

template <typename T, typename S>
hipError_t launch_block_next(const HArgs<T, S>& a, hipStream_t s) {
  const unsigned nwg = (unsigned)(a.n_pad / kBlock);
  hipLaunchKernelGGL((block_next_kernel<T, S>), dim3(nwg), dim3(kBlock), 0, s, a);
  hipLaunchKernelGGL(block_ctrl_kernel, dim3(1), dim3(kBlock), 0, s, a.blk.bc, a.blk.wgnext,
                     (int)nwg);
  return hipGetLastError();
}

template <typename T, typename S>
hipError_t launch_block_predict(const HArgs<T, S>& a, hipStream_t s) {
  const unsigned nwg = (unsigned)(a.n_pad / kBlock);
  if (a.nn)
    hipLaunchKernelGGL((block_predict_kernel<T, S, true>), dim3(nwg), dim3(kBlock), 0, s, a);
  else
    hipLaunchKernelGGL((block_predict_kernel<T, S>), dim3(nwg), dim3(kBlock), 0, s, a);
  hipLaunchKernelGGL((block_compact_kernel<T, S>), dim3(nwg), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

template <typename T, typename S>
hipError_t launch_block_narrow(const HArgs<T, S>& a, hipStream_t s) {
  const HBlock& b = a.blk;
  if (b.cap < 1) return hipSuccess;  // (narrow_max 0: every step is wide)
  if (b.slice < kBlock || b.slice % kBlock || (int64_t)b.n_slices * b.slice < a.n_pad ||
      !b.NA || !b.NJ || (sizeof(S) != sizeof(T) && !a.XL) ||
      (a.nn && (!nn_args_ok(a) || !a.NNI)))
    return hipErrorInvalidValue;
  const int groups = (b.cap + kNarrowGroup - 1) / kNarrowGroup;
  const dim3 grid((unsigned)b.n_slices, (unsigned)(groups < 16 ? groups : 16));
  if (a.nn && a.phi)
    hipLaunchKernelGGL((hermite_narrow_kernel<T, true, S, true>), grid, dim3(kBlock), 0, s, a);
  else if (a.nn)
    hipLaunchKernelGGL((hermite_narrow_kernel<T, false, S, true>), grid, dim3(kBlock), 0, s, a);
  else if (a.phi)
    hipLaunchKernelGGL((hermite_narrow_kernel<T, true, S>), grid, dim3(kBlock), 0, s, a);
  else
    hipLaunchKernelGGL((hermite_narrow_kernel<T, false, S>), grid, dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

template <typename T, typename S, int IPL>
static hipError_t launch_wide_t(const HArgs<T, S>& a, int groups, hipStream_t s) {
  const dim3 grid((unsigned)(a.n_pad / (kBlock * IPL)), (unsigned)groups);
  if (a.nn && a.phi)
    hipLaunchKernelGGL((hermite_eval_kernel<T, IPL, true, true, S, true>), grid, dim3(kBlock), 0,
                       s, a, 0);
  else if (a.nn)
    hipLaunchKernelGGL((hermite_eval_kernel<T, IPL, false, true, S, true>), grid, dim3(kBlock), 0,
                       s, a, 0);
  else if (a.phi)
    hipLaunchKernelGGL((hermite_eval_kernel<T, IPL, true, true, S>), grid, dim3(kBlock), 0, s, a,
                       0);
  else
    hipLaunchKernelGGL((hermite_eval_kernel<T, IPL, false, true, S>), grid, dim3(kBlock), 0, s, a,
                       0);
  return hipGetLastError();
}

template <typename T, typename S>
hipError_t launch_block_wide(const HArgs<T, S>& a, int ipl, int groups, hipStream_t s) {
  if (a.n_chunks < 1 || a.n_pad % (kBlock * ipl) || a.chunk % Tile<T>::kBodies ||
      (int64_t)a.n_chunks * a.chunk != a.n_pad || !a.blk.bc || !a.blk.list ||
      (sizeof(S) != sizeof(T) && !a.XL) || (a.nn && !nn_args_ok(a)))
    return hipErrorInvalidValue;
  if (groups < 1) groups = 1;
  if (groups > a.n_chunks) groups = a.n_chunks;
  switch (ipl) {
    case 1: return launch_wide_t<T, S, 1>(a, groups, s);
    case 2: return launch_wide_t<T, S, 2>(a, groups, s);
    case 4:
      if constexpr (sizeof(T) == 4) return launch_wide_t<T, S, 4>(a, groups, s);
      return hipErrorInvalidValue;
    default: return hipErrorInvalidValue;
  }
}

template <typename T, typename S>
hipError_t launch_block_correct(const HArgs<T, S>& a, hipStream_t s) {
  if (a.nn)
    hipLaunchKernelGGL((block_correct_kernel<T, S, true>), dim3((unsigned)(a.n_pad / kBlock)),
                       dim3(kBlock), 0, s, a);
  else
    hipLaunchKernelGGL((block_correct_kernel<T, S>), dim3((unsigned)(a.n_pad / kBlock)),
                       dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

template <typename T, typename S>
hipError_t launch_block_init(const HArgs<T, S>& a, int64_t t0, hipStream_t s) {
  hipLaunchKernelGGL((block_init_kernel<T, S>), dim3((unsigned)(a.n_pad / kBlock)), dim3(kBlock), 0,
                     s, a, t0);
  return hipGetLastError();
}

#define GS_HERMITE_INSTANTIATE(T, S)                                                          \
  template hipError_t launch_hermite_ctrl<T, S>(const HArgs<T, S>&, hipStream_t);                \
  template hipError_t launch_hermite_predict<T, S>(const HArgs<T, S>&, hipStream_t);             \
  template hipError_t launch_hermite_eval<T, S>(const HArgs<T, S>&, int, int, bool, hipStream_t); \
  template hipError_t launch_hermite_reduce<T, S>(const HArgs<T, S>&, hipStream_t);              \
  template hipError_t launch_hermite_stage<T, S>(const HArgs<T, S>&, hipStream_t);               \
  template hipError_t launch_block_next<T, S>(const HArgs<T, S>&, hipStream_t);                  \
  template hipError_t launch_block_predict<T, S>(const HArgs<T, S>&, hipStream_t);               \
  template hipError_t launch_block_narrow<T, S>(const HArgs<T, S>&, hipStream_t);                \
  template hipError_t launch_block_wide<T, S>(const HArgs<T, S>&, int, int, hipStream_t);        \
  template hipError_t launch_block_correct<T, S>(const HArgs<T, S>&, hipStream_t);               \
  template hipError_t launch_block_init<T, S>(const HArgs<T, S>&, int64_t, hipStream_t);
GS_HERMITE_INSTANTIATE(float, float)
GS_HERMITE_INSTANTIATE(double, double)
GS_HERMITE_INSTANTIATE(float, double)  // mixed precision

}  // namespace gs
