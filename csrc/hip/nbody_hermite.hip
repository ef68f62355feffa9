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
// Step chain (one stream, no host round trip): control (next h from the last step's
// per-workgroup dt minima; advances t, steps) -> predict -> evaluate -> reduce + correct.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gs_common.h"
#include "gs_hermite.h"
#include "gs_tile.h"

namespace gs {

// One i-j interaction: 6 sub, 3 fma (r^2), rsq + select, 3 mul (r^-2, mu r^-1, s), mul + 2 fma
// (d.w), 2 mul (alpha), 3 fma (a), 3 fma (w - alpha d), 3 fma (j).
template <typename T, bool PHI>
__device__ __forceinline__ void hinteract(T xi, T yi, T zi, T ui, T vi, T wi, const V4<T>& q,
                                          const V4<T>& p, T cut2, T eps2, T& ax, T& ay, T& az,
                                          T& ph, T& jx, T& jy, T& jz) {
  const T dx = q.x - xi, dy = q.y - yi, dz = q.z - zi;
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
}

// fp32, two i per lane as 2-vectors: each element sees exactly hinteract()'s arithmetic.
__device__ __forceinline__ f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }

template <bool PHI>
__device__ __forceinline__ void hinteract_pk(f2 xi, f2 yi, f2 zi, f2 ui, f2 vi, f2 wi,
                                             const V4<float>& q, const V4<float>& p, float cut2,
                                             float eps2, f2& ax, f2& ay, f2& az, f2& ph, f2& jx,
                                             f2& jy, f2& jz) {
  const f2 dx = f2(q.x) - xi, dy = f2(q.y) - yi, dz = f2(q.z) - zi;
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
}

template <typename T, int IPL>
struct HState {
  T x[IPL], y[IPL], z[IPL], u[IPL], v[IPL], w[IPL];  // predicted position and velocity
  T ax[IPL], ay[IPL], az[IPL], ph[IPL], jx[IPL], jy[IPL], jz[IPL];  // current chunk
};

template <typename T, int IPL>
__device__ __forceinline__ void hzero(HState<T, IPL>& s) {
#pragma unroll
  for (int k = 0; k < IPL; ++k)
    s.ax[k] = s.ay[k] = s.az[k] = s.ph[k] = s.jx[k] = s.jy[k] = s.jz[k] = T(0);
}

template <typename T, int IPL, bool PHI>
__device__ __forceinline__ void hinteract_all(HState<T, IPL>& s, const V4<T>& q, const V4<T>& p,
                                              T cut2, T eps2) {
  if constexpr (sizeof(T) == 4 && IPL % 2 == 0) {
#pragma unroll
    for (int k = 0; k < IPL; k += 2) {
      f2 ax = {s.ax[k], s.ax[k + 1]}, ay = {s.ay[k], s.ay[k + 1]}, az = {s.az[k], s.az[k + 1]};
      f2 jx = {s.jx[k], s.jx[k + 1]}, jy = {s.jy[k], s.jy[k + 1]}, jz = {s.jz[k], s.jz[k + 1]};
      f2 ph = {s.ph[k], s.ph[k + 1]};
      hinteract_pk<PHI>(f2{s.x[k], s.x[k + 1]}, f2{s.y[k], s.y[k + 1]}, f2{s.z[k], s.z[k + 1]},
                        f2{s.u[k], s.u[k + 1]}, f2{s.v[k], s.v[k + 1]}, f2{s.w[k], s.w[k + 1]},
                        q, p, cut2, eps2, ax, ay, az, ph, jx, jy, jz);
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
  for (int k = 0; k < IPL; ++k)
    hinteract<T, PHI>(s.x[k], s.y[k], s.z[k], s.u[k], s.v[k], s.w[k], q, p, cut2, eps2, s.ax[k],
                      s.ay[k], s.az[k], s.ph[k], s.jx[k], s.jy[k], s.jz[k]);
}

// EVALUATE: grid (n_pad / (256 IPL), groups). Workgroup (b, g) sweeps the chunks of group g and
// stores one partial per chunk: PA[c][i] = (ax, ay, az, sum mu/r), PJ[c][i] = (jx, jy, jz, 0).
template <typename T, int IPL, bool PHI>
__global__ __launch_bounds__(kBlock) void hermite_eval_kernel(HArgs<T> a, int gated) {
  constexpr int TB = Tile<T>::kBodies;
  __shared__ __attribute__((aligned(16))) V4<T> tx[2][TB];
  __shared__ __attribute__((aligned(16))) V4<T> tv[2][TB];
  if (gated && !a.ctrl->active) return;  // the run has reached t_end: a no-op step
  const int64_t ib = (int64_t)blockIdx.x * (kBlock * IPL);
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
  HState<T, IPL> st;
#pragma unroll
  for (int k = 0; k < IPL; ++k) {
    const V4<T> x = XP[ib + threadIdx.x + k * kBlock];
    const V4<T> v = VP[ib + threadIdx.x + k * kBlock];
    st.x[k] = x.x; st.y[k] = x.y; st.z[k] = x.z;
    st.u[k] = v.x; st.v[k] = v.y; st.w[k] = v.z;
  }
  auto fill = [&](int t) {
    const int64_t j0 = (int64_t)(c0 + t / tpc) * a.chunk + (int64_t)(t % tpc) * TB;
    tile_fill<T>(XP + j0, tx[t & 1]);
    tile_fill<T>(VP + j0, tv[t & 1]);
  };
  fill(0);
  hzero<T, IPL>(st);
  for (int t = 0; t < ntiles; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // tile t is in LDS for every wave; buffer (t+1)&1 is free
    if (t + 1 < ntiles) fill(t + 1);
    const V4<T>* cx = tx[t & 1];
    const V4<T>* cv = tv[t & 1];
#pragma unroll 4
    for (int j = 0; j < TB; ++j) {
      const V4<T> q = cx[j], p = cv[j];  // uniform addresses: broadcast ds_reads
      hinteract_all<T, IPL, PHI>(st, q, p, a.cut2, a.eps2);
    }
    if ((t + 1) % tpc == 0) {
      const int c = c0 + t / tpc;
#pragma unroll
      for (int k = 0; k < IPL; ++k) {
        V4<T> oa, oj;
        oa.x = st.ax[k]; oa.y = st.ay[k]; oa.z = st.az[k]; oa.w = st.ph[k];
        oj.x = st.jx[k]; oj.y = st.jy[k]; oj.z = st.jz[k]; oj.w = T(0);
        PA[(int64_t)c * a.n_pad + ib + threadIdx.x + k * kBlock] = oa;
        PJ[(int64_t)c * a.n_pad + ib + threadIdx.x + k * kBlock] = oj;
      }
      hzero<T, IPL>(st);
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
// once t >= t_end the chain's other kernels return at once and nothing is counted.
__global__ __launch_bounds__(kBlock) void hermite_ctrl_kernel(HermiteCtrl* ctrl,
                                                              const double* wgmin, int nwg) {
  __shared__ double red[kBlock / 64];
  double m = INFINITY;
  for (int k = threadIdx.x; k < nwg; k += kBlock) m = fmin(m, wgmin[k]);
  m = block_min(m, red);
  if (threadIdx.x != 0) return;
  HermiteCtrl c = *ctrl;
  if (c.has_end && c.t >= c.t_end) {
    ctrl->active = 0;
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
template <typename T>
__global__ __launch_bounds__(kBlock) void hermite_predict_kernel(HArgs<T> a) {
  if (!a.ctrl->active) return;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n_pad) return;
  V4<T> xp = {T(0), T(0), T(0), T(0)}, vp = xp;
  if (i < a.n_real) {
    const T h = (T)a.ctrl->h;
    const T h2 = (h * h) / T(2), h3 = (h * h * h) / T(6);
    const V4<T> x = reinterpret_cast<const V4<T>*>(a.X)[i];
    const V4<T> v = reinterpret_cast<const V4<T>*>(a.V)[i];
    const V4<T> ac = reinterpret_cast<const V4<T>*>(a.A)[i];
    const V4<T> jk = reinterpret_cast<const V4<T>*>(a.J)[i];
    xp.x = x.x + (v.x * h + (ac.x * h2 + jk.x * h3));
    xp.y = x.y + (v.y * h + (ac.y * h2 + jk.y * h3));
    xp.z = x.z + (v.z * h + (ac.z * h2 + jk.z * h3));
    xp.w = x.w;
    vp.x = v.x + (ac.x * h + jk.x * h2);
    vp.y = v.y + (ac.y * h + jk.y * h2);
    vp.z = v.z + (ac.z * h + jk.z * h2);
  }
  reinterpret_cast<V4<T>*>(a.XP)[i] = xp;
  reinterpret_cast<V4<T>*>(a.VP)[i] = vp;
}

__device__ __forceinline__ double norm3(double x, double y, double z) {
  return sqrt(x * x + y * y + z * z);
}

// REDUCE (+ CORRECT): one thread per body adds its chunk partials in chunk order, then
// HM_STEP applies the corrector and Aarseth's criterion, HM_INIT starts a run from (x, v),
// HM_OUT returns the derivatives. Per-workgroup dt minima go to wgmin (+inf when no body of the
// workgroup takes part: ghost rows, |j| = 0, a non-finite ratio, or a fixed-step run).
template <typename T>
__global__ __launch_bounds__(kBlock) void hermite_reduce_kernel(HArgs<T> a) {
  __shared__ double red[kBlock / 64];
  if (a.mode == HM_STEP && !a.ctrl->active) return;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;  // (n_pad is a multiple of 256)
  const V4<T>* PA = reinterpret_cast<const V4<T>*>(a.PA);
  const V4<T>* PJ = reinterpret_cast<const V4<T>*>(a.PJ);
  T a1x = 0, a1y = 0, a1z = 0, sp = 0, j1x = 0, j1y = 0, j1z = 0;
  for (int c = 0; c < a.n_chunks; ++c) {
    const V4<T> pa = PA[(int64_t)c * a.n_pad + i];
    const V4<T> pj = PJ[(int64_t)c * a.n_pad + i];
    a1x += pa.x; a1y += pa.y; a1z += pa.z; sp += pa.w;
    j1x += pj.x; j1y += pj.y; j1z += pj.z;
  }
  if (a.mode == HM_OUT) {
    V4<T> oa, oj;
    oa.x = a1x; oa.y = a1y; oa.z = a1z; oa.w = -sp;
    oj.x = j1x; oj.y = j1y; oj.z = j1z; oj.w = T(0);
    reinterpret_cast<V4<T>*>(a.a_out)[i] = oa;
    reinterpret_cast<V4<T>*>(a.j_out)[i] = oj;
    return;
  }
  V4<T>* A = reinterpret_cast<V4<T>*>(a.A);
  V4<T>* J = reinterpret_cast<V4<T>*>(a.J);
  const double eta = a.ctrl->eta;
  double dti = INFINITY;
  if (i >= a.n_real) {
    const V4<T> z = {T(0), T(0), T(0), T(0)};
    A[i] = z;
    J[i] = z;
    if (a.mode == HM_STEP) {
      reinterpret_cast<V4<T>*>(a.X)[i] = z;
      reinterpret_cast<V4<T>*>(a.V)[i] = z;
    }
  } else if (a.mode == HM_INIT) {
    if (eta > 0.0) {
      const double an = norm3(a1x, a1y, a1z), jn = norm3(j1x, j1y, j1z);
      const double d = 0.5 * eta * an / jn;
      if (jn > 0.0 && isfinite(d)) dti = d;
    }
  } else {
    const double hd = a.ctrl->h;
    const T h = (T)hd;
    const T hh = h / T(2), h12 = (h * h) / T(12);
    V4<T>* X = reinterpret_cast<V4<T>*>(a.X);
    V4<T>* V = reinterpret_cast<V4<T>*>(a.V);
    const V4<T> x = X[i], v = V[i], a0 = A[i], j0 = J[i];
    V4<T> v1, x1;
    v1.x = v.x + ((a0.x + a1x) * hh + (j0.x - j1x) * h12);
    v1.y = v.y + ((a0.y + a1y) * hh + (j0.y - j1y) * h12);
    v1.z = v.z + ((a0.z + a1z) * hh + (j0.z - j1z) * h12);
    v1.w = T(0);
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
    V4<T> oa, oj;
    oa.x = a1x; oa.y = a1y; oa.z = a1z; oa.w = T(0);
    oj.x = j1x; oj.y = j1y; oj.z = j1z; oj.w = T(0);
    A[i] = oa;
    J[i] = oj;
  }
  dti = block_min(dti, red);
  if (threadIdx.x == 0) a.wgmin[blockIdx.x] = dti;
}

// ---------------------------------------------------------------------------------------
// Host launchers.

template <typename T, int IPL>
static hipError_t launch_eval_t(const HArgs<T>& a, int groups, bool gated, hipStream_t s) {
  const dim3 grid((unsigned)(a.n_pad / (kBlock * IPL)), (unsigned)groups);
  if (a.phi)
    hipLaunchKernelGGL((hermite_eval_kernel<T, IPL, true>), grid, dim3(kBlock), 0, s, a,
                       (int)gated);
  else
    hipLaunchKernelGGL((hermite_eval_kernel<T, IPL, false>), grid, dim3(kBlock), 0, s, a,
                       (int)gated);
  return hipGetLastError();
}

bool hermite_ipl_ok(int fp64, int ipl) { return ipl == 1 || ipl == 2 || (ipl == 4 && !fp64); }

template <typename T>
hipError_t launch_hermite_eval(const HArgs<T>& a, int ipl, int groups, bool gated,
                               hipStream_t s) {
  if (a.n_chunks < 1 || a.n_pad % (kBlock * ipl) || a.chunk % Tile<T>::kBodies ||
      (int64_t)a.n_chunks * a.chunk != a.n_pad || (gated && !a.ctrl))
    return hipErrorInvalidValue;
  if (groups < 1) groups = 1;
  if (groups > a.n_chunks) groups = a.n_chunks;
  switch (ipl) {
    case 1: return launch_eval_t<T, 1>(a, groups, gated, s);
    case 2: return launch_eval_t<T, 2>(a, groups, gated, s);
    case 4:
      if constexpr (sizeof(T) == 4) return launch_eval_t<T, 4>(a, groups, gated, s);
      return hipErrorInvalidValue;
    default: return hipErrorInvalidValue;
  }
}

template <typename T>
hipError_t launch_hermite_ctrl(const HArgs<T>& a, hipStream_t s) {
  hipLaunchKernelGGL(hermite_ctrl_kernel, dim3(1), dim3(kBlock), 0, s, a.ctrl, a.wgmin,
                     (int)(a.n_pad / kBlock));
  return hipGetLastError();
}

template <typename T>
hipError_t launch_hermite_predict(const HArgs<T>& a, hipStream_t s) {
  hipLaunchKernelGGL((hermite_predict_kernel<T>), dim3((unsigned)(a.n_pad / kBlock)),
                     dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

template <typename T>
hipError_t launch_hermite_reduce(const HArgs<T>& a, hipStream_t s) {
  hipLaunchKernelGGL((hermite_reduce_kernel<T>), dim3((unsigned)(a.n_pad / kBlock)),
                     dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

#define GS_HERMITE_INSTANTIATE(T)                                                          \
  template hipError_t launch_hermite_ctrl<T>(const HArgs<T>&, hipStream_t);                \
  template hipError_t launch_hermite_predict<T>(const HArgs<T>&, hipStream_t);             \
  template hipError_t launch_hermite_eval<T>(const HArgs<T>&, int, int, bool, hipStream_t); \
  template hipError_t launch_hermite_reduce<T>(const HArgs<T>&, hipStream_t);
GS_HERMITE_INSTANTIATE(float)
GS_HERMITE_INSTANTIATE(double)

}  // namespace gs
