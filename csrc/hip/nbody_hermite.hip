// gfx950 kernels of the 4th-order Hermite integrator (Makino & Aarseth 1992).
//
// The hot kernel evaluates, for every body i at the predicted state (xp, vp),
//     a_i   = sum_j mu_j d / r^3
//     j_i   = sum_j mu_j (w - 3 (d.w) d / r^2) / r^3          d = xp_j - xp_i, w = vp_j - vp_i
//     phi_i = -sum_j mu_j / r                                  r^2 = |d|^2 + eps^2
// with the project's pair law (a pair contributes exactly zero to all three when
// r^2 < cutoff^2: the self term, coincident bodies, a ghost row on a body at the origin).
//   * One-sided and i-owned like force_split_kernel: a lane owns IPL i-bodies and keeps a, j
//     (and phi where the variant has it) in registers; no atomics.
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
//     term starts from d = (hi_j - hi_i) + (lo_j - lo_i); all else is the fp32 kernel.
//   * Collisions (NN, off by default and then compiled out): every body has a
//     radius, carried in the spare component of the VP row, and the evaluate kernels also keep,
//     per i-body, the j of the smallest q = r^2 - (R_i + R_j)^2 (the lowest j on an exact tie),
//     stored per chunk or slice beside the partial sums; the reduce kernels fold them, keep
//     the latest and the closest (q, j) per body and count the overlaps (q < eps^2).
// Step chain (one stream, no host round trip): control (next h from the last step's
// per-workgroup dt minima; advances t, steps) -> predict -> evaluate -> reduce + correct.
// Block time steps (each body on its own step dt 2^-k; second half of this file): next-time
// minima + control -> predict-all + mark -> compact (scan) -> evaluate of the active bodies,
// narrow (hermite_narrow_kernel, parallel over j) or wide (the Rows::List form of
// hermite_eval_kernel) by n_act -> reduce + correct + new level of the active bodies.
// Every kernel that comes in forms takes one HVariant (pair type, state type, PHI, NN, row
// mode); the host maps the run's settings to it in one place (with_variant, with_ipl), where the
// rule for which forms are built is written down.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "gs_common.h"
#include "gs_hermite.h"
#include "gs_hermite_scheme.h"
#include "gs_tile.h"

namespace gs {

// The i-rows a kernel works on: all n_pad rows, the rows of a block step's active list
// (a.blk.list), or a rank's slice a.row0 + [0, a.n_loc) of a multi-rank run.
enum class Rows { All, List, Slice };

// One form of a kernel: T the type of the pair arithmetic, S of the state (mixed precision: S is
// not T, and the pair term works on double-single positions, DS); PHI: the potential sum too;
// NN: collisions on. Kernels that do not sum pairs have the one form, PHI off, for both.
template <typename T_, typename S_, bool PHI_, bool NN_, Rows ROWS_>
struct HVariant {
  using T = T_;
  using S = S_;
  using Args = HArgs<T_, S_>;
  static constexpr bool PHI = PHI_, NN = NN_, DS = sizeof(S_) != sizeof(T_);
  static constexpr Rows ROWS = ROWS_;
};

// Separation of a pair: plain, or (DS, mixed precision) from double-single positions hi + lo,
// where the difference of the hi parts is exact whenever the bodies are close and the lo parts
// restore what float(x) dropped.
template <bool DS, typename V>
__device__ __forceinline__ V hsep(V qh, V xh, V ql, V xl) {
  if constexpr (DS) return (qh - xh) + (ql - xl);
  return qh - xh;
}

// One i-j interaction: 6 sub, 3 fma (r^2), rsq + select, 3 mul (r^-2, mu r^-1, s), mul + 2 fma
// (d.w), 2 mul (alpha), 3 fma (a), 3 fma (w - alpha d), 3 fma (j); DS: 3 sub and 3 add more.
// NN (collisions on): also the pair measure q = r^2 - (R_i + R_j)^2 (one add, one fma on the
// kernel's own r^2; R_j rides in p.w) and a strict-less compare-and-select against the best so
// far, so that the lowest j keeps an exact tie. A pair the law zeroes, a ghost row j (jreal
// false) or the body itself (with softening the law does not zero the self pair) takes no part.
// The operands of a flag that is off (DS: l, lxi, lyi, lzi; NN: ri, jreal, jg, self, bq, bn) are
// never read: every caller passes what it has, and the compiler drops them.
// Written once over the element type V (gs_tile.h): T for one i-body, f2 for two (fp32: every
// operation but the v_rsq_f32 and the selects is then a v_pk_*); bq, bn and self point at the
// entries of the element's first body.
template <bool PHI, bool DS, bool NN, typename V, typename T>
__device__ __forceinline__ void hinteract(V xi, V yi, V zi, V ui, V vi, V wi, const V4<T>& q,
                                          const V4<T>& p, T cut2, T eps2, V& ax, V& ay, V& az,
                                          V& ph, V& jx, V& jy, V& jz, const V4<T>& l, V lxi,
                                          V lyi, V lzi, V ri, bool jreal, int32_t jg,
                                          const int32_t* self, T* bq, int32_t* bn) {
  const V dx = hsep<DS>(V(q.x), xi, V(l.x), lxi), dy = hsep<DS>(V(q.y), yi, V(l.y), lyi),
          dz = hsep<DS>(V(q.z), zi, V(l.z), lzi);
  const V wx = V(p.x) - ui, wy = V(p.y) - vi, wz = V(p.z) - wi;
  const V r2 = fmav(dz, dz, fmav(dy, dy, fmav(dx, dx, V(eps2))));
  const V inv = inv_cut(r2, cut2);
  const V inv2 = inv * inv;
  const V mi = V(q.w) * inv;
  const V s = mi * inv2;
  const V dw = fmav(dz, wz, fmav(dy, wy, dx * wx));
  const V al = dw * (V(T(3)) * inv2);
  ax = fmav(s, dx, ax);
  ay = fmav(s, dy, ay);
  az = fmav(s, dz, az);
  jx = fmav(s, fmav(-al, dx, wx), jx);
  jy = fmav(s, fmav(-al, dy, wy), jy);
  jz = fmav(s, fmav(-al, dz, wz), jz);
  if constexpr (PHI) ph += mi;
  if constexpr (NN) {
    const V sr = V(p.w) + ri;
    const V qv = fmav(-sr, sr, r2);
    // (Written per element type, and the scalar form through one-element loops: one form for
    // both, in five shapes, moved the VGPRs of one or two NN kernels by one; these two hold every
    // kernel at the parent's figures, profiles/tile_sweep_resources.md.)
    if constexpr (std::is_same<V, f2>::value) {
      const float q0 = (r2.x >= cut2 && jreal && jg != self[0]) ? qv.x : INFINITY;
      const float q1 = (r2.y >= cut2 && jreal && jg != self[1]) ? qv.y : INFINITY;
      const bool l0 = q0 < bq[0], l1 = q1 < bq[1];
      bq[0] = l0 ? q0 : bq[0];
      bn[0] = l0 ? jg : bn[0];
      bq[1] = l1 ? q1 : bq[1];
      bn[1] = l1 ? jg : bn[1];
    } else {
      constexpr int E = 1;
      T qe[E];
      bool lt[E];
#pragma unroll
      for (int e = 0; e < E; ++e)
        qe[e] = (vget(r2, e) >= cut2 && jreal && jg != self[e]) ? vget(qv, e) : T(INFINITY);
#pragma unroll
      for (int e = 0; e < E; ++e) lt[e] = qe[e] < bq[e];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        bq[e] = lt[e] ? qe[e] : bq[e];
        bn[e] = lt[e] ? jg : bn[e];
      }
    }
  }
}

// A lane's i-bodies: the predicted rows and the sums of the current chunk; the lo rows (read by
// DS kernels only); the nearest neighbours (NN kernels only): own radius and row, the best q of
// the current chunk or slice and its j.
template <typename T, int IPL>
struct HState {
  T x[IPL], y[IPL], z[IPL], u[IPL], v[IPL], w[IPL];  // predicted position and velocity
  T ax[IPL], ay[IPL], az[IPL], ph[IPL], jx[IPL], jy[IPL], jz[IPL];  // current chunk
};
template <typename T, int IPL>
struct HLo {
  T x[IPL], y[IPL], z[IPL];
};
template <typename T, int IPL>
struct HNear {
  T r[IPL], q[IPL];
  int32_t n[IPL], self[IPL];
};

// Body k of the lane <- row `row` of the predicted state.
template <bool DS, bool NN, typename T, int IPL>
__device__ __forceinline__ void hload_row(HState<T, IPL>& st, HLo<T, IPL>& lo, HNear<T, IPL>& nr,
                                          int k, const V4<T>* XP, const V4<T>* VP,
                                          const V4<T>* XL, int64_t row) {
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

// The sums of the lane start from zero, and (NN) its nearest neighbours from (+inf, none).
template <bool NN, typename T, int IPL>
__device__ __forceinline__ void hreset(HState<T, IPL>& s, HNear<T, IPL>& nr) {
#pragma unroll
  for (int k = 0; k < IPL; ++k)
    s.ax[k] = s.ay[k] = s.az[k] = s.ph[k] = s.jx[k] = s.jy[k] = s.jz[k] = T(0);
  if constexpr (NN) {
#pragma unroll
    for (int k = 0; k < IPL; ++k) {
      nr.q[k] = T(INFINITY);
      nr.n[k] = -1;
    }
  }
}

// Row j = (q, p, lo row l, row number jg, real or ghost) against every i-body of the lane.
template <bool PHI, bool DS, bool NN, typename T, int IPL>
__device__ __forceinline__ void hinteract_all(HState<T, IPL>& s, const HLo<T, IPL>& lo,
                                              HNear<T, IPL>& nr, const V4<T>& q, const V4<T>& p,
                                              const V4<T>& l, bool jreal, int32_t jg, T cut2,
                                              T eps2) {
  if constexpr (sizeof(T) == 4 && IPL % 2 == 0) {
#pragma unroll
    for (int k = 0; k < IPL; k += 2) {
      f2 ax = {s.ax[k], s.ax[k + 1]}, ay = {s.ay[k], s.ay[k + 1]}, az = {s.az[k], s.az[k + 1]};
      f2 jx = {s.jx[k], s.jx[k + 1]}, jy = {s.jy[k], s.jy[k + 1]}, jz = {s.jz[k], s.jz[k + 1]};
      f2 ph = {s.ph[k], s.ph[k + 1]};
      hinteract<PHI, DS, NN>(
          f2{s.x[k], s.x[k + 1]}, f2{s.y[k], s.y[k + 1]}, f2{s.z[k], s.z[k + 1]},
          f2{s.u[k], s.u[k + 1]}, f2{s.v[k], s.v[k + 1]}, f2{s.w[k], s.w[k + 1]}, q, p, cut2,
          eps2, ax, ay, az, ph, jx, jy, jz, l, f2{lo.x[k], lo.x[k + 1]},
          f2{lo.y[k], lo.y[k + 1]}, f2{lo.z[k], lo.z[k + 1]}, f2{nr.r[k], nr.r[k + 1]}, jreal,
          jg, &nr.self[k], &nr.q[k], &nr.n[k]);
      s.ax[k] = ax.x; s.ax[k + 1] = ax.y;
      s.ay[k] = ay.x; s.ay[k + 1] = ay.y;
      s.az[k] = az.x; s.az[k + 1] = az.y;
      s.jx[k] = jx.x; s.jx[k + 1] = jx.y;
      s.jy[k] = jy.x; s.jy[k + 1] = jy.y;
      s.jz[k] = jz.x; s.jz[k + 1] = jz.y;
      s.ph[k] = ph.x; s.ph[k + 1] = ph.y;
    }
  } else {
#pragma unroll
    for (int k = 0; k < IPL; ++k)
      hinteract<PHI, DS, NN>(s.x[k], s.y[k], s.z[k], s.u[k], s.v[k], s.w[k], q, p, cut2, eps2,
                             s.ax[k], s.ay[k], s.az[k], s.ph[k], s.jx[k], s.jy[k], s.jz[k], l,
                             lo.x[k], lo.y[k], lo.z[k], nr.r[k], jreal, jg, &nr.self[k], &nr.q[k],
                             &nr.n[k]);
  }
}

// EVALUATE: grid (rows / (256 IPL), groups). Workgroup (b, g) sweeps the chunks of group g and
// stores one partial per chunk: PA[c][i] = (ax, ay, az, sum mu/r), PJ[c][i] = (jx, jy, jz, 0).
// Rows::List (a block step's wide path): lane slot s owns body list[s], the partials are stored
// per slot and i-blocks beyond n_act exit; the j loop, hence a body's bits, is the same.
// Mixed precision (DS): a third tile carries the lo rows XL, the lane keeps the lo rows of its
// i-bodies, and only the separation differs.
// NN: the lane also keeps the nearest neighbour (smallest q, lowest j on a tie) of each of its
// i-bodies over the chunk; the partial is (PJ[c][i].w, PN[c][i]). j is uniform over the wave, so
// the ghost-row test is a scalar compare.
// Rows::Slice (a rank of a multi-rank run): the i-rows are the rank's own, a.row0 + [0, a.n_loc),
// which the grid's x extent covers; the partials are indexed by local row with stride a.n_loc.
// The j sweep is the same, so a body's bits are those of the one-rank run.
template <typename K, int IPL>
__global__ __launch_bounds__(kBlock) void hermite_eval_kernel(typename K::Args a, int gated) {
  using T = typename K::T;
  constexpr bool DS = K::DS, NN = K::NN;
  constexpr int TB = Tile<T>::kBodies;
  __shared__ __attribute__((aligned(16))) V4<T> tx[2][TB];
  __shared__ __attribute__((aligned(16))) V4<T> tv[2][TB];
  __shared__ __attribute__((aligned(16))) V4<T> tl[2][DS ? TB : 1];
  if (gated && !a.ctrl->active) return;  // the run has reached t_end: a no-op step
  const int64_t ib = (int64_t)blockIdx.x * (kBlock * IPL);  // (Slice: counted from a.row0)
  int64_t n_act = 0;
  if constexpr (K::ROWS == Rows::List) {
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
  HLo<T, IPL> lo = {};
  HNear<T, IPL> nr = {};
#pragma unroll
  for (int k = 0; k < IPL; ++k) {
    int64_t row = ib + threadIdx.x + k * kBlock;
    if constexpr (K::ROWS == Rows::Slice) row += a.row0;
    if constexpr (K::ROWS == Rows::List)
      row = a.blk.list[row < n_act ? row : n_act - 1];  // (spare slots: a copy)
    hload_row<DS, NN>(st, lo, nr, k, XP, VP, XL, row);
  }
  auto fill = [&](int t) {
    const int64_t j0 = (int64_t)(c0 + t / tpc) * a.chunk + (int64_t)(t % tpc) * TB;
    tile_fill<T>(XP + j0, tx[t & 1]);
    tile_fill<T>(VP + j0, tv[t & 1]);
    if constexpr (DS) tile_fill<T>(XL + j0, tl[t & 1]);
  };
  fill(0);
  hreset<NN>(st, nr);
  const int64_t pstride = K::ROWS == Rows::Slice ? a.n_loc : a.n_pad;  // of the partials
  for (int t = 0; t < ntiles; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // tile t is in LDS for every wave; buffer (t+1)&1 is free
    if (t + 1 < ntiles) fill(t + 1);
    const V4<T>* cx = tx[t & 1];
    const V4<T>* cv = tv[t & 1];
    const V4<T>* cl = tl[t & 1];
    // (NN only) the tile's first row and the count of real rows
    const int32_t jb = (int32_t)((int64_t)(c0 + t / tpc) * a.chunk + (int64_t)(t % tpc) * TB);
    const int32_t nreal = (int32_t)a.n_real;
#pragma unroll 4
    for (int j = 0; j < TB; ++j) {
      const V4<T> q = cx[j], p = cv[j];  // uniform addresses: broadcast ds_reads
      hinteract_all<K::PHI, DS, NN>(st, lo, nr, q, p, DS ? cl[j] : V4<T>(), jb + j < nreal,
                                    jb + j, a.cut2, a.eps2);
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
          a.PN[(int64_t)c * pstride + ib + threadIdx.x + k * kBlock] = nr.n[k];
        }
        PA[(int64_t)c * pstride + ib + threadIdx.x + k * kBlock] = oa;
        PJ[(int64_t)c * pstride + ib + threadIdx.x + k * kBlock] = oj;
      }
      hreset<NN>(st, nr);
    }
  }
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

// The predictor of real body i over h: xp = x + v h + a h^2/2 + j h^3/6, vp = v + a h + j h^2/2.
template <typename T, typename S>
__device__ __forceinline__ void hpredict(const HArgs<T, S>& a, int64_t i, S h, V4<S>& xp,
                                         V4<S>& vp) {
  const S h2 = (h * h) / S(2), h3 = (h * h * h) / S(6);
  const V4<S> x = reinterpret_cast<const V4<S>*>(a.X)[i];
  const V4<S> v = reinterpret_cast<const V4<S>*>(a.V)[i];
  const V4<S> ac = reinterpret_cast<const V4<S>*>(a.A)[i];
  const V4<S> jk = reinterpret_cast<const V4<S>*>(a.J)[i];
  // h4_predict (gs_hermite_scheme.h) per component, written out: through the helper, in any of
  // four shapes, the fp32 block_predict_kernel takes 32 to 34 VGPRs against the 35 of this text
  // (profiles/hermite_scheme_resources.md), and the kernels' resources are held equal.
  xp.x = x.x + (v.x * h + (ac.x * h2 + jk.x * h3));
  xp.y = x.y + (v.y * h + (ac.y * h2 + jk.y * h3));
  xp.z = x.z + (v.z * h + (ac.z * h2 + jk.z * h3));
  xp.w = x.w;
  vp.x = v.x + (ac.x * h + jk.x * h2);
  vp.y = v.y + (ac.y * h + jk.y * h2);
  vp.z = v.z + (ac.z * h + jk.z * h2);
}

// Store row i of the predicted state for the evaluate kernels: as it is, or (mixed precision,
// S is not T) the position split into XP = (float(xp), mu), XL = (float(xp - double(hi)), 0).
// Spare::Radius (collisions on): the spare component of the VP row carries the body's radius (R,
// state precision).
enum class Spare { Zero, Radius };
template <Spare SPARE, typename T, typename S>
__device__ __forceinline__ void store_predicted(const HArgs<T, S>& a, int64_t i, const V4<S>& xp,
                                                const V4<S>& vp) {
  V4<T> h, v;
  h.x = (T)xp.x; h.y = (T)xp.y; h.z = (T)xp.z; h.w = (T)xp.w;
  v.x = (T)vp.x; v.y = (T)vp.y; v.z = (T)vp.z; v.w = T(0);
  if constexpr (SPARE == Spare::Radius) v.w = (T)a.R[i];
  reinterpret_cast<V4<T>*>(a.XP)[i] = h;
  reinterpret_cast<V4<T>*>(a.VP)[i] = v;
  if constexpr (sizeof(S) != sizeof(T)) {
    V4<T> l;
    l.x = (T)(xp.x - (S)h.x); l.y = (T)(xp.y - (S)h.y); l.z = (T)(xp.z - (S)h.z); l.w = T(0);
    reinterpret_cast<V4<T>*>(a.XL)[i] = l;
  }
}

// PREDICT over the step's h (ghost rows stay zero).
// Rows::Slice: the grid covers the rank's rows a.row0 + [0, a.n_loc) of the full-length XP, VP
// (XL).
template <typename K>
__global__ __launch_bounds__(kBlock) void hermite_predict_kernel(typename K::Args a) {
  using S = typename K::S;
  if (!a.ctrl->active) return;
  const int64_t i =
      (K::ROWS == Rows::Slice ? a.row0 : 0) + (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n_pad) return;
  V4<S> xp = {S(0), S(0), S(0), S(0)}, vp = xp;
  if (i < a.n_real) hpredict(a, i, (S)a.ctrl->h, xp, vp);
  store_predicted<K::NN ? Spare::Radius : Spare::Zero>(a, i, xp, vp);
}

// SPLIT (mixed precision): the predictor's output at h = 0, for the derivatives of the current
// state (ghost rows of X, V are zero).
__global__ __launch_bounds__(kBlock) void hermite_split_kernel(HArgs<float, double> a) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n_pad) return;
  store_predicted<Spare::Zero>(a, i, reinterpret_cast<const V4<double>*>(a.X)[i],
                               reinterpret_cast<const V4<double>*>(a.V)[i]);
}

// STAGE (collisions on): XP, VP (and XL) <- the current X, V with the radius in VP's spare
// component, for an evaluation of the current state in any precision.
template <typename T, typename S>
__global__ __launch_bounds__(kBlock) void hermite_stage_kernel(HArgs<T, S> a) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n_pad) return;
  store_predicted<Spare::Radius>(a, i, reinterpret_cast<const V4<S>*>(a.X)[i],
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

// The derivatives of one body, summed from its partials (state precision), and (NN) the
// nearest neighbour folded from them.
template <typename T, typename S>
struct HSum {
  S ax = 0, ay = 0, az = 0, ph = 0, jx = 0, jy = 0, jz = 0;
  T q = T(INFINITY);
  int32_t n = -1;
};

// One step of the in-order fold of a body's partials: m += the partial at index o; NN: its (q, j)
// with a strict less, so that on a tie the earlier partial (the lower j) stays.
template <bool NN, typename T, typename S>
__device__ __forceinline__ void hfold(HSum<T, S>& m, const V4<T>* PA, const V4<T>* PJ,
                                      const int32_t* PN, int64_t o) {
  const V4<T> pa = PA[o];
  const V4<T> pj = PJ[o];
  m.ax += pa.x; m.ay += pa.y; m.az += pa.z; m.ph += pa.w;
  m.jx += pj.x; m.jy += pj.y; m.jz += pj.z;
  if constexpr (NN) {
    if (pj.w < m.q) {
      m.q = pj.w;
      m.n = PN[o];
    }
  }
}

// (The helpers below take the arrays, not the HArgs: a reference to the kernel's argument block
// costs a kernel that does not otherwise take one a private copy of it, and registers.)

// The carried a, j of body i <- the sums.
template <typename T, typename S>
__device__ __forceinline__ void hcarry(V4<S>* A, V4<S>* J, int64_t i, const HSum<T, S>& m) {
  V4<S> oa, oj;
  oa.x = m.ax; oa.y = m.ay; oa.z = m.az; oa.w = S(0);
  oj.x = m.jx; oj.y = m.jy; oj.z = m.jz; oj.w = S(0);
  A[i] = oa;
  J[i] = oj;
}

// The corrector of body i over h: x, v <- corrected from the carried (a0, j0), which are handed
// back for the criterion, and the new sums.
template <typename T, typename S>
__device__ __forceinline__ void hcorrect(V4<S>* X, V4<S>* V, const V4<S>* A, const V4<S>* J,
                                         int64_t i, S h, const HSum<T, S>& m, V4<S>& a0,
                                         V4<S>& j0) {
  const S hh = h / S(2), h12 = (h * h) / S(12);
  const V4<S> x = X[i], v = V[i];
  a0 = A[i];
  j0 = J[i];
  S cx[3], cv[3];  // (a vector's component does not bind to a reference)
  h4_correct<S>(hh, h12, x.x, v.x, a0.x, j0.x, m.ax, m.jx, cx[0], cv[0]);
  h4_correct<S>(hh, h12, x.y, v.y, a0.y, j0.y, m.ay, m.jy, cx[1], cv[1]);
  h4_correct<S>(hh, h12, x.z, v.z, a0.z, j0.z, m.az, m.jz, cx[2], cv[2]);
  const V4<S> x1 = {cx[0], cx[1], cx[2], x.w}, v1 = {cv[0], cv[1], cv[2], S(0)};
  X[i] = x1;
  V[i] = v1;
}

// Aarseth's criterion from the 2nd and 3rd derivatives that the two evaluations (a0, j0 before
// the step hd, the sums after it) imply. False where |j| = 0 or the ratio is not finite.
template <typename T, typename S>
__device__ __forceinline__ bool aarseth_dt(double hd, double eta, const V4<S>& a0,
                                           const V4<S>& j0, const HSum<T, S>& m, double& dt) {
  const double a0d[3] = {a0.x, a0.y, a0.z}, j0d[3] = {j0.x, j0.y, j0.z};
  const double a1d[3] = {m.ax, m.ay, m.az}, j1d[3] = {m.jx, m.jy, m.jz};
  return h4_dt(hd, eta, a0d, j0d, a1d, j1d, dt);
}

// REDUCE (+ CORRECT): one thread per body adds its chunk partials in chunk order, then
// HM_STEP applies the corrector and Aarseth's criterion, HM_INIT starts a run from (x, v),
// HM_OUT returns the derivatives. Per-workgroup dt minima go to wgmin (+inf when no body of the
// workgroup takes part: ghost rows, |j| = 0, a non-finite ratio, or a fixed-step run).
// NN: HM_OUT writes the folded (q, j) to q_out / nn_out, the other modes record them (nn_record).
// Rows::Slice: the grid covers the rank's rows; it reads the rank's partials [n_chunks][n_loc]
// and writes the rows' entries of the full-length X, V, A, J, outputs and wgmin.
template <typename K>
__global__ __launch_bounds__(kBlock) void hermite_reduce_kernel(typename K::Args a) {
  using T = typename K::T;
  using S = typename K::S;
  constexpr bool SLICE = K::ROWS == Rows::Slice, NN = K::NN;
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
  HSum<T, S> m;
  for (int c = 0; c < a.n_chunks; ++c) hfold<NN>(m, PA, PJ, a.PN, (int64_t)c * pstride + li);
  if (a.mode == HM_OUT) {
    V4<S> oa, oj;
    oa.x = m.ax; oa.y = m.ay; oa.z = m.az; oa.w = -m.ph;
    oj.x = m.jx; oj.y = m.jy; oj.z = m.jz; oj.w = S(0);
    reinterpret_cast<V4<S>*>(a.a_out)[i] = oa;
    reinterpret_cast<V4<S>*>(a.j_out)[i] = oj;
    if constexpr (NN) {
      a.q_out[i] = (double)m.q;
      a.nn_out[i] = m.n;
    }
    return;
  }
  if constexpr (NN) {
    if (i < a.n_real) nn_record<T, S>(a, i, m.q, m.n, &a.ctrl->overlaps);
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
      const double ad[3] = {m.ax, m.ay, m.az}, jd[3] = {m.jx, m.jy, m.jz};
      double d;
      if (hermite_first_dt(eta, ad, jd, d)) dti = d;
    }
  } else {
    const double hd = a.ctrl->h;
    V4<S> a0, j0;
    hcorrect(reinterpret_cast<V4<S>*>(a.X), reinterpret_cast<V4<S>*>(a.V), A, J, i, (S)hd, m, a0,
             j0);
    if (eta > 0.0) {
      double d;
      if (aarseth_dt(hd, eta, a0, j0, m, d)) dti = d;
    }
  }
  if (i < a.n_real) hcarry(A, J, i, m);
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

// Minimum over the workgroup's threads (valid in thread 0).
__device__ __forceinline__ int64_t block_min_i64(int64_t v, int64_t* red) {
  v = wave_min_i64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kBlock / 64; ++w) v = red[w] < v ? red[w] : v;
  return v;
}

__device__ __forceinline__ int wave_sum_i32(int v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// (ticks_seconds, body_due and the level rule block_new_level: gs_hermite.h, shared with order 6)

// NEXT, stage 1: per-workgroup minimum of tb + step over the real bodies.
template <typename T, typename S>
__global__ __launch_bounds__(kBlock) void block_next_kernel(HArgs<T, S> a) {
  __shared__ int64_t red[kBlock / 64];
  const HBlock& b = a.blk;
  const int L = b.bc->L;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  int64_t v = INT64_MAX;
  if (i < a.n_real) v = b.tb[i] + ((int64_t)1 << (L - b.level[i]));
  v = block_min_i64(v, red);
  if (threadIdx.x == 0) b.wgnext[blockIdx.x] = v;
}

// NEXT, stage 2 and CONTROL (one workgroup): t_next = the earliest due time; past the target the
// chain's other kernels return at once.
__global__ __launch_bounds__(kBlock) void block_ctrl_kernel(HermiteBlockCtrl* bc,
                                                            const int64_t* wgnext, int nwg) {
  __shared__ int64_t red[kBlock / 64];
  int64_t m = INT64_MAX;
  for (int k = threadIdx.x; k < nwg; k += kBlock) m = wgnext[k] < m ? wgnext[k] : m;
  m = block_min_i64(m, red);
  if (threadIdx.x != 0) return;
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
template <typename K>
__global__ __launch_bounds__(kBlock) void block_predict_kernel(typename K::Args a) {
  using S = typename K::S;
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
    hpredict(a, i, (S)ticks_seconds(b.bc->dt_max, t_next - b.tb[i], L), xp, vp);
  }
  store_predicted<K::NN ? Spare::Radius : Spare::Zero>(a, i, xp, vp);
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
// its slot. fp32 runs two i-bodies as 2-vectors (hinteract over f2).
// NN: a lane folds its rows with a strict less in j order; the lanes' and the waves' (q, j) fold
// lexicographically (the smaller q, on a tie the lower j); the partial is (NJ[s][slot].w,
// NNI[s][slot]).
template <typename K>
__global__ __launch_bounds__(kBlock) void hermite_narrow_kernel(typename K::Args a) {
  using T = typename K::T;
  constexpr bool DS = K::DS, NN = K::NN;
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
    HLo<T, G> lo = {};
    HNear<T, G> nr = {};
#pragma unroll
    for (int k = 0; k < G; ++k)  // (spare slots of the last group: a copy)
      hload_row<DS, NN>(st, lo, nr, k, XP, VP, XL, (int64_t)b.list[min(g * G + k, n_act - 1)]);
    hreset<NN>(st, nr);
    for (int64_t j = j0 + threadIdx.x; j < j1; j += kBlock) {
      const V4<T> q = XP[j], p = VP[j];
      if constexpr (DS)  // (the lo row straight from memory: a copy of it costs a move per row)
        hinteract_all<K::PHI, DS, NN>(st, lo, nr, q, p, XL[j], j < a.n_real, (int32_t)j, a.cut2,
                                      a.eps2);
      else
        hinteract_all<K::PHI, DS, NN>(st, lo, nr, q, p, V4<T>(), j < a.n_real, (int32_t)j, a.cut2,
                                      a.eps2);
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
template <typename K>
__global__ __launch_bounds__(kBlock) void block_correct_kernel(typename K::Args a) {
  using T = typename K::T;
  using S = typename K::S;
  constexpr bool NN = K::NN;
  const HBlock& b = a.blk;
  HermiteBlockCtrl* bc = b.bc;
  if (!bc->active) return;
  const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (s >= bc->n_act) return;
  HSum<T, S> m;
  if (bc->path == HP_NARROW) {
    const V4<T>* NA = reinterpret_cast<const V4<T>*>(b.NA);
    const V4<T>* NJ = reinterpret_cast<const V4<T>*>(b.NJ);
#pragma unroll 8
    for (int c = 0; c < b.n_slices; ++c)  // (unrolled: the loads of 8 slices are in flight)
      hfold<NN>(m, NA, NJ, a.NNI, (int64_t)c * b.cap + s);
  } else {
    const V4<T>* PA = reinterpret_cast<const V4<T>*>(a.PA);
    const V4<T>* PJ = reinterpret_cast<const V4<T>*>(a.PJ);
    for (int c = 0; c < a.n_chunks; ++c) hfold<NN>(m, PA, PJ, a.PN, (int64_t)c * a.n_pad + s);
  }
  if (a.mode == HM_OUT) {
    V4<S> oa, oj;
    oa.x = m.ax; oa.y = m.ay; oa.z = m.az; oa.w = -m.ph;
    oj.x = m.jx; oj.y = m.jy; oj.z = m.jz; oj.w = S(0);
    reinterpret_cast<V4<S>*>(a.a_out)[s] = oa;
    reinterpret_cast<V4<S>*>(a.j_out)[s] = oj;
    if constexpr (NN) {
      a.q_out[s] = (double)m.q;
      a.nn_out[s] = m.n;
    }
    return;
  }
  const int64_t i = b.list[s];
  if constexpr (NN) nn_record<T, S>(a, i, m.q, m.n, &bc->overlaps);
  const int L = bc->L;
  const int64_t t_next = bc->t_ticks;
  const double dt_max = bc->dt_max, eta = bc->eta;
  const double hd = ticks_seconds(dt_max, t_next - b.tb[i], L);
  V4<S>* A = reinterpret_cast<V4<S>*>(a.A);
  V4<S>* J = reinterpret_cast<V4<S>*>(a.J);
  V4<S> a0, j0;
  hcorrect(reinterpret_cast<V4<S>*>(a.X), reinterpret_cast<V4<S>*>(a.V), A, J, i, (S)hd, m, a0,
           j0);
  hcarry(A, J, i, m);
  b.tb[i] = t_next;
  double want;
  const bool rated = aarseth_dt(hd, eta, a0, j0, m, want);
  b.level[i] = block_new_level(bc, b.level[i], rated, want, t_next, L, dt_max);
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
    const double ad[3] = {ac.x, ac.y, ac.z}, jd[3] = {jk.x, jk.y, jk.z};
    double want;
    if (hermite_first_dt(b.bc->eta, ad, jd, want))
      while (k < b.bc->L && ldexp(b.bc->dt_max, -k) > want) ++k;
    if (k > b.bc->level_max) atomicMax(&b.bc->level_max, k);
  }
  b.tb[i] = t0;
  b.level[i] = k;
}

// ---------------------------------------------------------------------------------------
// Host launchers: validate, compute the grid, dispatch.

// (hlaunch, row_grid and clamp_groups: gs_hermite.h, shared with nbody_hermite6.hip)

// A rank's slice of a multi-rank run.
template <typename T, typename S>
static bool is_slice(const HArgs<T, S>& a) { return a.n_loc != a.n_pad; }

// The forms that are built (the one place that says so).
// Rows::All and Rows::List have PHI x NN; a slice never carries
// collisions (nor block state: slice_ok), so Rows::Slice has PHI alone. The evaluate kernels
// come with 1 or 2 i-bodies per lane, and with 4 where the pair type is fp32, except mixed
// precision with collisions on: that kernel would need all 256 VGPRs, and the runtime's launch
// shape (hermite.hip) never asks for it.
template <typename K>
constexpr bool eval_built(int ipl) {
  return ipl == 1 || ipl == 2 || (ipl == 4 && sizeof(typename K::T) == 4 && !(K::DS && K::NN));
}

bool hermite_ipl_ok(int fp64, int ipl) { return ipl == 1 || ipl == 2 || (ipl == 4 && !fp64); }

// f(HVariant) for the run's settings. Over::List: the block step's kernels, which work on the
// active list; Over::Run: all rows, or the rank's slice. Sums::Pairs: the kernels that sum pairs
// come with and without the potential (a.phi); the others have the one form, PHI off.
enum class Over { Run, List };
enum class Sums { None, Pairs };

template <Rows R, Sums P, typename T, typename S, typename F>
static hipError_t with_flags(const HArgs<T, S>& a, F&& f) {
  constexpr bool kPhi = P == Sums::Pairs, kNN = R != Rows::Slice;
  if (a.nn && !kNN) return hipErrorInvalidValue;
  const bool phi = kPhi && a.phi;
  if constexpr (kPhi && kNN)
    if (phi && a.nn) return f(HVariant<T, S, true, true, R>());
  if constexpr (kPhi)
    if (phi) return f(HVariant<T, S, true, false, R>());
  if constexpr (kNN)
    if (a.nn) return f(HVariant<T, S, false, true, R>());
  return f(HVariant<T, S, false, false, R>());
}

template <Over O, Sums P, typename T, typename S, typename F>
static hipError_t with_variant(const HArgs<T, S>& a, F&& f) {
  if constexpr (O == Over::List) {
    return with_flags<Rows::List, P>(a, f);
  } else {
    if (is_slice(a)) return with_flags<Rows::Slice, P>(a, f);
    return with_flags<Rows::All, P>(a, f);
  }
}

// f(IPL) for the i-bodies per lane of an evaluate kernel of variant K.
template <typename K, typename F>
static hipError_t with_ipl(int ipl, F&& f) {
  if (!eval_built<K>(ipl)) return hipErrorInvalidValue;
  if (ipl == 1) return f(std::integral_constant<int, 1>());
  if (ipl == 2) return f(std::integral_constant<int, 2>());
  if constexpr (eval_built<K>(4)) return f(std::integral_constant<int, 4>());
  return hipErrorInvalidValue;
}

// The arrays a collisions-on launch writes.
template <typename T, typename S>
static bool nn_args_ok(const HArgs<T, S>& a) {
  return a.R && a.PN && a.nn_q && a.nn_i && a.ca_q && a.ca_i && a.q_out && a.nn_out &&
         a.n_pad <= INT32_MAX;
}

// The geometry of an evaluate launch: whole chunks of whole tiles, whole workgroups of ipl rows.
template <typename T, typename S>
static bool eval_geometry_ok(const HArgs<T, S>& a, int ipl) {
  return hermite_ipl_ok(sizeof(T) == 8, ipl) &&
         chunk_geometry_ok<T>(a.n_pad, a.chunk, a.n_chunks, ipl) &&
         (sizeof(S) == sizeof(T) || a.XL) && (!a.nn || nn_args_ok(a));
}

// The rows row0 + [0, n_loc) of a launch: whole units of `unit` rows inside n_pad (one rank: all
// of them); a slice carries no block state.
template <typename T, typename S>
static bool slice_ok(const HArgs<T, S>& a, int64_t unit) {
  return a.row0 >= 0 && a.n_loc >= 1 && a.row0 + a.n_loc <= a.n_pad && a.n_loc % unit == 0 &&
         a.row0 % kBlock == 0 && !(is_slice(a) && a.blk.bc);
}

template <typename T, typename S>
hipError_t launch_hermite_eval(const HArgs<T, S>& a, int ipl, int groups, bool gated,
                               hipStream_t s) {
  if (!eval_geometry_ok(a, ipl) || (gated && !a.ctrl) || !slice_ok(a, (int64_t)kBlock * ipl))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)(a.n_loc / (kBlock * ipl)), (unsigned)clamp_groups(groups, a.n_chunks));
  return with_variant<Over::Run, Sums::Pairs>(a, [&](auto k) {
    using K = decltype(k);
    return with_ipl<K>(ipl, [&](auto n) {
      return hlaunch(hermite_eval_kernel<K, decltype(n)::value>, grid, s, a, (int)gated);
    });
  });
}

template <typename T, typename S>
hipError_t launch_hermite_ctrl(const HArgs<T, S>& a, hipStream_t s) {
  return hlaunch(hermite_ctrl_kernel, dim3(1), s, a.ctrl, a.wgmin, (int)(a.n_pad / kBlock));
}

template <typename T, typename S>
hipError_t launch_hermite_predict(const HArgs<T, S>& a, hipStream_t s) {
  if (is_slice(a) && !slice_ok(a, kBlock)) return hipErrorInvalidValue;
  return with_variant<Over::Run, Sums::None>(a, [&](auto k) {
    return hlaunch(hermite_predict_kernel<decltype(k)>, row_grid(a.n_loc), s, a);
  });
}

hipError_t launch_hermite_split(const HArgs<float, double>& a, hipStream_t s) {
  return hlaunch(hermite_split_kernel, row_grid(a.n_pad), s, a);
}

template <typename T, typename S>
hipError_t launch_hermite_stage(const HArgs<T, S>& a, hipStream_t s) {
  if (!a.R) return hipErrorInvalidValue;
  return hlaunch(hermite_stage_kernel<T, S>, row_grid(a.n_pad), s, a);
}

template <typename T, typename S>
hipError_t launch_hermite_reduce(const HArgs<T, S>& a, hipStream_t s) {
  if (is_slice(a) && !slice_ok(a, kBlock)) return hipErrorInvalidValue;
  return with_variant<Over::Run, Sums::None>(a, [&](auto k) {
    return hlaunch(hermite_reduce_kernel<decltype(k)>, row_grid(a.n_loc), s, a);
  });
}

int32_t hermite_narrow_slice(int64_t n_pad) {
  // At most 64 slices of at least 1024 rows (4 per lane, which amortise the fold of the lanes;
  // 64 partials keep the reduce's chain of dependent adds short): a function of n_pad alone,
  // since it fixes the bits.
  return (int32_t)round_up(n_pad / 64 > 4 * kBlock ? n_pad / 64 : 4 * kBlock, kBlock);
}

template <typename T, typename S>
hipError_t launch_block_next(const HArgs<T, S>& a, hipStream_t s) {
  const hipError_t e = hlaunch(block_next_kernel<T, S>, row_grid(a.n_pad), s, a);
  if (e != hipSuccess) return e;
  return hlaunch(block_ctrl_kernel, dim3(1), s, a.blk.bc, a.blk.wgnext, (int)(a.n_pad / kBlock));
}

template <typename T, typename S>
hipError_t launch_block_predict(const HArgs<T, S>& a, hipStream_t s) {
  const hipError_t e = with_variant<Over::List, Sums::None>(a, [&](auto k) {
    return hlaunch(block_predict_kernel<decltype(k)>, row_grid(a.n_pad), s, a);
  });
  if (e != hipSuccess) return e;
  return launch_block_compact<T, S>(a, s);
}

template <typename T, typename S>
hipError_t launch_block_compact(const HArgs<T, S>& a, hipStream_t s) {
  return hlaunch(block_compact_kernel<T, S>, row_grid(a.n_pad), s, a);
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
  return with_variant<Over::List, Sums::Pairs>(a, [&](auto k) {
    return hlaunch(hermite_narrow_kernel<decltype(k)>, grid, s, a);
  });
}

template <typename T, typename S>
hipError_t launch_block_wide(const HArgs<T, S>& a, int ipl, int groups, hipStream_t s) {
  if (!eval_geometry_ok(a, ipl) || !a.blk.bc || !a.blk.list) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(a.n_pad / (kBlock * ipl)), (unsigned)clamp_groups(groups, a.n_chunks));
  return with_variant<Over::List, Sums::Pairs>(a, [&](auto k) {
    using K = decltype(k);
    return with_ipl<K>(ipl, [&](auto n) {
      return hlaunch(hermite_eval_kernel<K, decltype(n)::value>, grid, s, a, 0);
    });
  });
}

template <typename T, typename S>
hipError_t launch_block_correct(const HArgs<T, S>& a, hipStream_t s) {
  return with_variant<Over::List, Sums::None>(a, [&](auto k) {
    return hlaunch(block_correct_kernel<decltype(k)>, row_grid(a.n_pad), s, a);
  });
}

template <typename T, typename S>
hipError_t launch_block_init(const HArgs<T, S>& a, int64_t t0, hipStream_t s) {
  return hlaunch(block_init_kernel<T, S>, row_grid(a.n_pad), s, a, t0);
}

#define GS_HERMITE_INSTANTIATE(T, S)                                                          \
  template hipError_t launch_hermite_ctrl<T, S>(const HArgs<T, S>&, hipStream_t);                \
  template hipError_t launch_hermite_predict<T, S>(const HArgs<T, S>&, hipStream_t);             \
  template hipError_t launch_hermite_eval<T, S>(const HArgs<T, S>&, int, int, bool, hipStream_t); \
  template hipError_t launch_hermite_reduce<T, S>(const HArgs<T, S>&, hipStream_t);              \
  template hipError_t launch_hermite_stage<T, S>(const HArgs<T, S>&, hipStream_t);               \
  template hipError_t launch_block_next<T, S>(const HArgs<T, S>&, hipStream_t);                  \
  template hipError_t launch_block_predict<T, S>(const HArgs<T, S>&, hipStream_t);               \
  template hipError_t launch_block_compact<T, S>(const HArgs<T, S>&, hipStream_t);               \
  template hipError_t launch_block_narrow<T, S>(const HArgs<T, S>&, hipStream_t);                \
  template hipError_t launch_block_wide<T, S>(const HArgs<T, S>&, int, int, hipStream_t);        \
  template hipError_t launch_block_correct<T, S>(const HArgs<T, S>&, hipStream_t);               \
  template hipError_t launch_block_init<T, S>(const HArgs<T, S>&, int64_t, hipStream_t);
GS_HERMITE_INSTANTIATE(float, float)
GS_HERMITE_INSTANTIATE(double, double)
GS_HERMITE_INSTANTIATE(float, double)  // mixed precision

}  // namespace gs
