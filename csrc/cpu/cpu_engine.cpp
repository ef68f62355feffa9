// Native CPU direct-sum engine (fp64 and fp32), OpenMP over i.
//
// Replaces the per-rank CPU loop of mpi.c:196-216 (and the pair map of pyspark.py:59-86)
// with the intended physics: accelerations for step k use only step-k positions (Jacobi),
// never the in-place Gauss-Seidel update of mpi.c. The j sum follows the
// canonical chunk order shared with the GPU kernels so that results do not depend on the
// number of ranks. Serves BASELINE config #1 ("1,024 bodies on CPU") and as a fast oracle.
#include <math.h>

#include <cmath>
#include <limits>
#include <string>
#include <type_traits>
#include <vector>
#include <stdint.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#if defined(__AVX2__) && defined(__FMA__)
#include <immintrin.h>
#define GS_CPU_SIMD 1
#endif

#include "gravsim.h"
#include "gs_hermite_scheme.h"

void gs_set_error(const char* msg);

namespace {

template <typename T>
inline T rsqrt_ref(T r2) { return T(1) / std::sqrt(r2); }

template <typename T>
inline void accel_one(const T* X4, int64_t n_real, int64_t i, int32_t chunk, T cut2, T eps2,
                      T out[4]) {
  const T xi = X4[4 * i], yi = X4[4 * i + 1], zi = X4[4 * i + 2];
  const int64_t n_chunks = (n_real + chunk - 1) / chunk;
  T tx = 0, ty = 0, tz = 0, tp = 0;
  for (int64_t c = 0; c < n_chunks; ++c) {
    T ax = 0, ay = 0, az = 0, ph = 0;
    // Rows in [n_real, n_pad) are massless ghosts: their terms are exact zeros (the GPU
    // kernels sweep them anyway), so the CPU stops at n_real.
    const int64_t j0 = c * chunk, j1 = j0 + chunk < n_real ? j0 + chunk : n_real;
    for (int64_t j = j0; j < j1; ++j) {
      const T dx = X4[4 * j] - xi, dy = X4[4 * j + 1] - yi, dz = X4[4 * j + 2] - zi;
      const T mu = X4[4 * j + 3];
      const T r2 = std::fma(dz, dz, std::fma(dy, dy, std::fma(dx, dx, eps2)));
      const T inv = (r2 >= cut2) ? rsqrt_ref(r2) : T(0);
      const T mi = mu * inv;
      const T s = mi * (inv * inv);
      ax = std::fma(s, dx, ax);
      ay = std::fma(s, dy, ay);
      az = std::fma(s, dz, az);
      ph += mi;
    }
    tx += ax; ty += ay; tz += az; tp += ph;
  }
  out[0] = tx; out[1] = ty; out[2] = tz; out[3] = -tp;
}

#ifdef GS_CPU_SIMD
// AVX2 lanes over i (4 fp64 / 8 fp32 bodies per vector). Every lane runs exactly the scalar
// accel_one() sequence (same fma nesting, correctly rounded sqrt and divide, same chunk
// order), so the vector and scalar paths agree bit for bit; only independent i are batched.
template <typename T> struct Simd;
template <> struct Simd<double> {
  using V = __m256d;
  static constexpr int L = 4;
  static V set1(double a) { return _mm256_set1_pd(a); }
  static V zero() { return _mm256_setzero_pd(); }
  static V sub(V a, V b) { return _mm256_sub_pd(a, b); }
  static V add(V a, V b) { return _mm256_add_pd(a, b); }
  static V mul(V a, V b) { return _mm256_mul_pd(a, b); }
  static V fma(V a, V b, V c) { return _mm256_fmadd_pd(a, b, c); }
  static V inv_sqrt_masked(V r2, V cut2) {
    const V inv = _mm256_div_pd(_mm256_set1_pd(1.0), _mm256_sqrt_pd(r2));
    return _mm256_and_pd(inv, _mm256_cmp_pd(r2, cut2, _CMP_GE_OQ));
  }
  static void store(double* p, V a) { _mm256_storeu_pd(p, a); }
};
template <> struct Simd<float> {
  using V = __m256;
  static constexpr int L = 8;
  static V set1(float a) { return _mm256_set1_ps(a); }
  static V zero() { return _mm256_setzero_ps(); }
  static V sub(V a, V b) { return _mm256_sub_ps(a, b); }
  static V add(V a, V b) { return _mm256_add_ps(a, b); }
  static V mul(V a, V b) { return _mm256_mul_ps(a, b); }
  static V fma(V a, V b, V c) { return _mm256_fmadd_ps(a, b, c); }
  static V inv_sqrt_masked(V r2, V cut2) {
    const V inv = _mm256_div_ps(_mm256_set1_ps(1.0f), _mm256_sqrt_ps(r2));
    return _mm256_and_ps(inv, _mm256_cmp_ps(r2, cut2, _CMP_GE_OQ));
  }
  static void store(float* p, V a) { _mm256_storeu_ps(p, a); }
};

// Accelerations of bodies [i, i + L); out[d * L + l] = component d of body i + l.
template <typename T, bool PHI>
inline void accel_block(const T* X4, int64_t n_real, int64_t i, int32_t chunk, T cut2, T eps2,
                        T* out) {
  using S = Simd<T>;
  using V = typename S::V;
  constexpr int L = S::L;
  alignas(32) T bx[L], by[L], bz[L];
  for (int l = 0; l < L; ++l) {
    bx[l] = X4[4 * (i + l)];
    by[l] = X4[4 * (i + l) + 1];
    bz[l] = X4[4 * (i + l) + 2];
  }
  V xi, yi, zi;
  memcpy(&xi, bx, sizeof(V));
  memcpy(&yi, by, sizeof(V));
  memcpy(&zi, bz, sizeof(V));
  const V e2 = S::set1(eps2), c2 = S::set1(cut2);
  const int64_t n_chunks = (n_real + chunk - 1) / chunk;
  V tx = S::zero(), ty = S::zero(), tz = S::zero(), tp = S::zero();
  for (int64_t c = 0; c < n_chunks; ++c) {
    V ax = S::zero(), ay = S::zero(), az = S::zero(), ph = S::zero();
    const T* q = X4 + 4 * c * (int64_t)chunk;
    const int64_t len = n_real - c * (int64_t)chunk < chunk ? n_real - c * (int64_t)chunk : chunk;
    for (int64_t j = 0; j < len; ++j, q += 4) {
      const V dx = S::sub(S::set1(q[0]), xi), dy = S::sub(S::set1(q[1]), yi),
              dz = S::sub(S::set1(q[2]), zi);
      const V r2 = S::fma(dz, dz, S::fma(dy, dy, S::fma(dx, dx, e2)));
      const V inv = S::inv_sqrt_masked(r2, c2);
      const V mi = S::mul(S::set1(q[3]), inv);
      const V s = S::mul(mi, S::mul(inv, inv));
      ax = S::fma(s, dx, ax);
      ay = S::fma(s, dy, ay);
      az = S::fma(s, dz, az);
      if (PHI) ph = S::add(ph, mi);
    }
    tx = S::add(tx, ax); ty = S::add(ty, ay); tz = S::add(tz, az);
    if (PHI) tp = S::add(tp, ph);
  }
  S::store(out, tx);
  S::store(out + L, ty);
  S::store(out + 2 * L, tz);
  S::store(out + 3 * L, tp);
  if (PHI)
    for (int l = 0; l < L; ++l) out[3 * L + l] = -out[3 * L + l];
}
#endif

template <typename T>
int accel_range(const T* X4, int64_t n_real, int64_t i0, int64_t i1, int32_t chunk, T cut2,
                T eps2, T* acc4) {
  if (chunk <= 0 || i1 < i0) { gs_set_error("cpu_accel: bad arguments"); return -1; }
  int64_t i_vec = i0;
#ifdef GS_CPU_SIMD
  constexpr int L = Simd<T>::L;
  const int64_t nblk = (i1 - i0) / L;
  i_vec = i0 + nblk * L;
#pragma omp parallel for schedule(static)
  for (int64_t b = 0; b < nblk; ++b) {
    T out[4 * L];
    const int64_t i = i0 + b * L;
    accel_block<T, true>(X4, n_real, i, chunk, cut2, eps2, out);
    for (int l = 0; l < L; ++l)
      for (int d = 0; d < 4; ++d) acc4[4 * (i + l - i0) + d] = out[d * L + l];
  }
#endif
#pragma omp parallel for schedule(static)
  for (int64_t i = i_vec; i < i1; ++i) {
    T out[4];
    accel_one<T>(X4, n_real, i, chunk, cut2, eps2, out);
    for (int d = 0; d < 4; ++d) acc4[4 * (i - i0) + d] = out[d];
  }
  return 0;
}

template <typename T>
inline void kick_drift(const T* X4, T* Xn4, T* vel4, int64_t i0, int64_t i, const T a[3], T dt) {
  T* v = vel4 + 4 * (i - i0);
  T* xo = Xn4 + 4 * i;
  // Kick then drift (cuda.cu:73-76, mpi.c:207-215, pyspark.py:97-99).
  for (int d = 0; d < 3; ++d) {
    v[d] = v[d] + a[d] * dt;
    xo[d] = X4[4 * i + d] + v[d] * dt;
  }
  xo[3] = X4[4 * i + 3];
}

template <typename T>
int step_range(const T* X4, T* Xn4, T* vel4, int64_t n_real, int64_t i0, int64_t i1,
               int32_t chunk, T dt, T cut2, T eps2) {
  if (chunk <= 0 || i1 < i0) { gs_set_error("cpu_step: bad arguments"); return -1; }
  const int64_t i_real = i1 < n_real ? i1 : (i0 > n_real ? i0 : n_real);  // [i0, i_real) real
  int64_t i_vec = i0;
#ifdef GS_CPU_SIMD
  constexpr int L = Simd<T>::L;
  const int64_t nblk = (i_real - i0) / L;
  i_vec = i0 + nblk * L;
#pragma omp parallel for schedule(static)
  for (int64_t b = 0; b < nblk; ++b) {
    T out[4 * L];
    const int64_t i = i0 + b * L;
    accel_block<T, false>(X4, n_real, i, chunk, cut2, eps2, out);
    for (int l = 0; l < L; ++l) {
      const T a[3] = {out[l], out[L + l], out[2 * L + l]};
      kick_drift<T>(X4, Xn4, vel4, i0, i + l, a, dt);
    }
  }
#endif
#pragma omp parallel for schedule(static)
  for (int64_t i = i_vec; i < i1; ++i) {
    if (i >= n_real) {
      T* v = vel4 + 4 * (i - i0);
      T* xo = Xn4 + 4 * i;
      xo[0] = xo[1] = xo[2] = xo[3] = 0;
      v[0] = v[1] = v[2] = v[3] = 0;
      continue;
    }
    T a[4];
    accel_one<T>(X4, n_real, i, chunk, cut2, eps2, a);
    kick_drift<T>(X4, Xn4, vel4, i0, i, a, dt);
  }
  return 0;
}

// fp64 accelerations of bodies [i0, i1) with, per component, the sum of the terms' absolute
// values: out8[8 * (i - i0) + d] = a_d, out8[8 * (i - i0) + 4 + d] = sum_j |term_ij,d|
// (d < 3; entries 3 and 7 are 0). A floating-point sum of the terms is judged against that
// scale: |a_gpu - a| <= c * eps * sum |terms| (the accuracy gates of bench.py and the 1M test).
// A = double (the fp32 gates) or long double (x87 extended, 64-bit significand: the fp64 gates,
// where an fp64 reference's own rounding is of the fp64 kernel's order).
template <typename A>
int accel_abs_range(const double* X4, int64_t n_real, int64_t i0, int64_t i1, double cut2,
                    double eps2, double* out8) {
  if (i1 < i0) { gs_set_error("cpu_accel_abs: bad arguments"); return -1; }
#pragma omp parallel for schedule(dynamic, 1)
  for (int64_t i = i0; i < i1; ++i) {
    const A xi = X4[4 * i], yi = X4[4 * i + 1], zi = X4[4 * i + 2];
    A a[3] = {0, 0, 0}, s_abs[3] = {0, 0, 0};
    for (int64_t j = 0; j < n_real; ++j) {
      const A dx = (A)X4[4 * j] - xi, dy = (A)X4[4 * j + 1] - yi, dz = (A)X4[4 * j + 2] - zi;
      A r2;
      if constexpr (std::is_same<A, double>::value)
        r2 = std::fma(dz, dz, std::fma(dy, dy, std::fma(dx, dx, eps2)));
      else
        r2 = dx * dx + dy * dy + dz * dz + (A)eps2;  // (fmal is a libm software call)
      if (!(r2 >= (A)cut2)) continue;
      const A inv = (A)1 / std::sqrt(r2);
      const A s = (A)X4[4 * j + 3] * inv * inv * inv;
      const A t[3] = {s * dx, s * dy, s * dz};
      for (int d = 0; d < 3; ++d) {
        a[d] += t[d];
        s_abs[d] += std::fabs(t[d]);
      }
    }
    double* o = out8 + 8 * (i - i0);
    for (int d = 0; d < 3; ++d) {
      o[d] = (double)a[d];
      o[4 + d] = (double)s_abs[d];
    }
    o[3] = o[7] = 0.0;
  }
  return 0;
}

// ---- the rows of a pair loop ------------------------------------------------------------------
// Position rows X (x, y, z, mu) and, where the operation needs them, lo rows L and velocity rows
// V, all of the pair type T. fp32 and fp64 point at the caller's arrays. Mixed precision (fp64
// state, fp32 pair arithmetic on double-single positions) fills the rows the GPU predictor hands
// its pair kernels: X = (float(x), mu), L = (float(x - double(hi)), 0), V = (float(v), 0).
template <typename T>
struct Rows {
  const T *X = nullptr, *L = nullptr, *V = nullptr;
  std::vector<T> own;  // mixed: the storage of X, L (and V)
};

// S: the type of the caller's arrays; the pair type is float for MIXED and S otherwise.
template <typename S, bool MIXED>
using pair_t = std::conditional_t<MIXED, float, S>;

// V4 null: no velocity rows (nn, knn).
template <typename S, bool MIXED>
Rows<pair_t<S, MIXED>> make_rows(const S* X4, const S* V4, int64_t n) {
  Rows<pair_t<S, MIXED>> r;
  if constexpr (!MIXED) {
    r.X = X4;
    r.V = V4;
  } else {
    r.own.resize((size_t)(V4 ? 12 : 8) * n);
    float *H = r.own.data(), *L = H + 4 * n, *W = V4 ? L + 4 * n : nullptr;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; ++i) {
      for (int d = 0; d < 3; ++d) {
        const float hi = (float)X4[4 * i + d];
        H[4 * i + d] = hi;
        L[4 * i + d] = (float)(X4[4 * i + d] - (double)hi);
        if (W) W[4 * i + d] = (float)V4[4 * i + d];
      }
      H[4 * i + 3] = (float)X4[4 * i + 3];
      L[4 * i + 3] = 0.0f;
      if (W) W[4 * i + 3] = 0.0f;
    }
    r.X = H;
    r.L = L;
    r.V = W;
  }
  return r;
}

// The rows a driver serves: idx[0..n_idx), or (idx null) i0 + k. False, with the error set, for
// a range or an index outside [0, n_real), or when the driver's own checks (args_ok) failed.
bool rows_ok(const char* what, bool args_ok, const int32_t* idx, int64_t i0, int64_t n_idx,
             int64_t n_real) {
  const char* why = nullptr;
  if (!args_ok || n_idx < 0 || (!idx && (i0 < 0 || i0 + n_idx > n_real))) why = "bad arguments";
  for (int64_t k = 0; !why && idx && k < n_idx; ++k)
    if (idx[k] < 0 || idx[k] >= n_real) why = "index out of range";
  if (why) gs_set_error((std::string(what) + ": " + why).c_str());
  return !why;
}

// ---- the Hermite pair term (both orders) ----------------------------------------------------
// Acceleration, jerk and potential of body i at the rows r, and (SNAP, the 6th-order scheme) the
// snap at the predicted acceleration rows A4: the arithmetic of the GPU kernels
// (nbody_hermite.hip hinteract, nbody_hermite6.hip h6interact, whose first 26 operations are the
// same), chunk sums in T from zero in j order, added in chunk order into totals of type O (T, or
// double for mixed: the GPU's reduce). MIXED (order 4 only): the separation is
// (h_j - h_i) + (l_j - l_i).
template <typename T, bool MIXED, bool SNAP, typename O>
inline void accjerk_one(const Rows<T>& r, const T* A4, int64_t n_real, int64_t i, int32_t chunk,
                        T cut2, T eps2, O a4[4], O j4[4], O* s4) {
  static_assert(!(MIXED && SNAP), "the 6th-order scheme has no mixed precision");
  const T *X4 = r.X, *L4 = r.L, *V4 = r.V;
  const T xi = X4[4 * i], yi = X4[4 * i + 1], zi = X4[4 * i + 2];
  const T ui = V4[4 * i], vi = V4[4 * i + 1], wi = V4[4 * i + 2];
  T bxi = 0, byi = 0, bzi = 0;
  if constexpr (SNAP) {
    bxi = A4[4 * i]; byi = A4[4 * i + 1]; bzi = A4[4 * i + 2];
  }
  const int64_t n_chunks = (n_real + chunk - 1) / chunk;
  O ta[4] = {0, 0, 0, 0}, tj[3] = {0, 0, 0}, ts[3] = {0, 0, 0};
  for (int64_t c = 0; c < n_chunks; ++c) {
    T ax = 0, ay = 0, az = 0, ph = 0, jx = 0, jy = 0, jz = 0, sx = 0, sy = 0, sz = 0;
    const int64_t j0 = c * chunk, j1 = j0 + chunk < n_real ? j0 + chunk : n_real;
    for (int64_t j = j0; j < j1; ++j) {
      T dx = X4[4 * j] - xi, dy = X4[4 * j + 1] - yi, dz = X4[4 * j + 2] - zi;
      if (MIXED) {
        dx = dx + (L4[4 * j] - L4[4 * i]);
        dy = dy + (L4[4 * j + 1] - L4[4 * i + 1]);
        dz = dz + (L4[4 * j + 2] - L4[4 * i + 2]);
      }
      const T wx = V4[4 * j] - ui, wy = V4[4 * j + 1] - vi, wz = V4[4 * j + 2] - wi;
      const T r2 = std::fma(dz, dz, std::fma(dy, dy, std::fma(dx, dx, eps2)));
      const T inv = (r2 >= cut2) ? rsqrt_ref(r2) : T(0);
      const T inv2 = inv * inv;
      const T mi = X4[4 * j + 3] * inv;
      const T s = mi * inv2;
      const T dw = std::fma(dz, wz, std::fma(dy, wy, dx * wx));
      const T i3 = T(3) * inv2;
      const T al3 = dw * i3;  // 3 alpha
      const T ux = std::fma(-al3, dx, wx), uy = std::fma(-al3, dy, wy),
              uz = std::fma(-al3, dz, wz);
      ax = std::fma(s, dx, ax);
      ay = std::fma(s, dy, ay);
      az = std::fma(s, dz, az);
      jx = std::fma(s, ux, jx);
      jy = std::fma(s, uy, jy);
      jz = std::fma(s, uz, jz);
      ph += mi;
      if constexpr (SNAP) {
        const T qx = A4[4 * j] - bxi, qy = A4[4 * j + 1] - byi, qz = A4[4 * j + 2] - bzi;
        const T ww = std::fma(wz, wz, std::fma(wy, wy, wx * wx));
        const T dq = std::fma(dz, qz, std::fma(dy, qy, dx * qx));
        const T al = dw * inv2;
        const T be3 = std::fma(al3, al, (ww + dq) * i3);  // 3 beta
        const T al6 = al3 + al3;
        sx = std::fma(s, std::fma(-al6, ux, std::fma(-be3, dx, qx)), sx);
        sy = std::fma(s, std::fma(-al6, uy, std::fma(-be3, dy, qy)), sy);
        sz = std::fma(s, std::fma(-al6, uz, std::fma(-be3, dz, qz)), sz);
      }
    }
    ta[0] += ax; ta[1] += ay; ta[2] += az; ta[3] += ph;
    tj[0] += jx; tj[1] += jy; tj[2] += jz;
    if constexpr (SNAP) {
      ts[0] += sx; ts[1] += sy; ts[2] += sz;
    }
  }
  a4[0] = ta[0]; a4[1] = ta[1]; a4[2] = ta[2]; a4[3] = -ta[3];
  j4[0] = tj[0]; j4[1] = tj[1]; j4[2] = tj[2]; j4[3] = 0;
  if constexpr (SNAP) {
    s4[0] = ts[0]; s4[1] = ts[1]; s4[2] = ts[2]; s4[3] = 0;
  }
}

// Row k of the output is body idx[k] (a block step's active set), or (idx null) body i0 + k.
// SNAP: A4 the predicted acceleration rows, snap4 the third output (both null otherwise).
template <typename S, bool MIXED, bool SNAP = false>
int accjerk_rows(const S* X4, const S* V4, int64_t n_real, const int32_t* idx, int64_t i0,
                 int64_t n_idx, int32_t chunk, S cut2, S eps2, S* acc4, S* jerk4,
                 const S* A4 = nullptr, S* snap4 = nullptr) {
  using T = pair_t<S, MIXED>;
  const bool args_ok = chunk > 0 && (!SNAP || (X4 && V4 && A4 && acc4 && jerk4 && snap4));
  if (!rows_ok(SNAP ? "cpu_accjerksnap" : "cpu_accjerk", args_ok, idx, i0, n_idx, n_real))
    return -1;
  const Rows<T> r = make_rows<S, MIXED>(X4, V4, n_real);
  const T* AP = nullptr;
  if constexpr (SNAP) AP = A4;
#pragma omp parallel for schedule(static)
  for (int64_t k = 0; k < n_idx; ++k)
    accjerk_one<T, MIXED, SNAP, S>(r, AP, n_real, idx ? idx[k] : i0 + k, chunk, (T)cut2, (T)eps2,
                                   acc4 + 4 * k, jerk4 + 4 * k, SNAP ? snap4 + 4 * k : nullptr);
  return 0;
}

// A list entry's idx may be null only for an empty list (a null idx means a range to the drivers).
inline bool list_ok(const char* what, const int32_t* idx, int64_t n_idx) {
  if (idx || n_idx == 0) return true;
  gs_set_error((std::string(what) + ": bad arguments").c_str());
  return false;
}

// ---- nearest neighbours (the NN flag of the GPU kernels) ------------------------------------
// q_ij = r^2 - (R_i + R_j)^2 with the pair's own r^2 (one add, one fma), the smallest over the
// real j != i whose pair the law does not zero, the lowest j on a tie (a strict less in j order);
// (+inf, -1) when there is none. MIXED: the separation from double-single rows (X, L).
template <typename T, bool MIXED>
inline void nn_one(const Rows<T>& r, const T* R, int64_t n_real, int64_t i, T cut2, T eps2,
                   T* q_out, int32_t* nn_out) {
  const T *X4 = r.X, *L4 = r.L;
  const T xi = X4[4 * i], yi = X4[4 * i + 1], zi = X4[4 * i + 2], ri = R[i];
  T bq = std::numeric_limits<T>::infinity();
  int32_t bn = -1;
  for (int64_t j = 0; j < n_real; ++j) {
    T dx = X4[4 * j] - xi, dy = X4[4 * j + 1] - yi, dz = X4[4 * j + 2] - zi;
    if (MIXED) {
      dx = dx + (L4[4 * j] - L4[4 * i]);
      dy = dy + (L4[4 * j + 1] - L4[4 * i + 1]);
      dz = dz + (L4[4 * j + 2] - L4[4 * i + 2]);
    }
    const T r2 = std::fma(dz, dz, std::fma(dy, dy, std::fma(dx, dx, eps2)));
    const T sr = R[j] + ri;
    const T qv = std::fma(-sr, sr, r2);
    if (r2 >= cut2 && j != i && qv < bq) {
      bq = qv;
      bn = (int32_t)j;
    }
  }
  *q_out = bq;
  *nn_out = bn;
}

// Bodies idx[0..n_idx) (idx null: i0 + k). X4 rows of 4, R n_real radii, q: all of type S.
template <typename S, bool MIXED>
int nn_rows(const S* X4, const S* R, int64_t n_real, const int32_t* idx, int64_t i0, int64_t n_idx,
            S cut2, S eps2, S* q, int32_t* nn) {
  using T = pair_t<S, MIXED>;
  if (!rows_ok("cpu_nn", X4 && R && q && nn && n_real <= INT32_MAX, idx, i0, n_idx, n_real))
    return -1;
  const Rows<T> r = make_rows<S, MIXED>(X4, nullptr, n_real);
  const std::vector<T> Rt(R, R + (MIXED ? n_real : 0));  // (mixed: the radii in fp32, once)
  const T* Rp;
  if constexpr (MIXED) Rp = Rt.data(); else Rp = R;
#pragma omp parallel for schedule(static)
  for (int64_t k = 0; k < n_idx; ++k) {
    T qt;
    nn_one<T, MIXED>(r, Rp, n_real, idx ? idx[k] : i0 + k, (T)cut2, (T)eps2, &qt, nn + k);
    q[k] = (S)qt;
  }
  return 0;
}

// ---- k nearest neighbours (nbody_knn.hip) -----------------------------------------------------
// The first k of the ascending order on (r^2, j) over the real j != i: r^2 = fma(dz, dz,
// fma(dy, dy, dx dx)) of d = x_j - x_i (MIXED: (h_j - h_i) + (l_j - l_i)), no softening, no
// cutoff. A sweep in ascending j with a strict less keeps the lower j on a tie, which is the
// lexicographic order. (+inf, -1) past the neighbours there are.
constexpr int kKnnMax = 8;

template <typename T, bool MIXED, typename O>
inline void knn_one(const Rows<T>& rows, int64_t n_real, int64_t i, int32_t k, O* r2,
                    int32_t* idx) {
  const T *X4 = rows.X, *L4 = rows.L;
  const T xi = X4[4 * i], yi = X4[4 * i + 1], zi = X4[4 * i + 2];
  T r[kKnnMax];
  int32_t n[kKnnMax];
  for (int s = 0; s < kKnnMax; ++s) {
    r[s] = std::numeric_limits<T>::infinity();
    n[s] = -1;
  }
  for (int64_t j = 0; j < n_real; ++j) {
    T dx = X4[4 * j] - xi, dy = X4[4 * j + 1] - yi, dz = X4[4 * j + 2] - zi;
    if (MIXED) {
      dx = dx + (L4[4 * j] - L4[4 * i]);
      dy = dy + (L4[4 * j + 1] - L4[4 * i + 1]);
      dz = dz + (L4[4 * j + 2] - L4[4 * i + 2]);
    }
    const T c = std::fma(dz, dz, std::fma(dy, dy, dx * dx));
    if (j == i || !(c < r[k - 1])) continue;  // (slots from k on never reach the output)
    int s = k - 1;
    for (; s > 0 && c < r[s - 1]; --s) {
      r[s] = r[s - 1];
      n[s] = n[s - 1];
    }
    r[s] = c;
    n[s] = (int32_t)j;
  }
  for (int s = 0; s < k; ++s) {
    r2[s] = (O)r[s];
    idx[s] = n[s];
  }
}

template <typename S, bool MIXED>
int knn_rows(const S* X4, int64_t n_real, int64_t i0, int64_t i1, int32_t k, S* r2,
             int32_t* idx) {
  using T = pair_t<S, MIXED>;
  if (!(X4 && r2 && idx && n_real >= 1 && n_real <= INT32_MAX && i0 >= 0 && i1 >= i0 &&
        i1 <= n_real && k >= 1 && k <= kKnnMax)) {
    gs_set_error("cpu_knn: bad arguments (n >= 1, rows within [0, n], k in 1..8)");
    return -1;
  }
  const Rows<T> r = make_rows<S, MIXED>(X4, nullptr, n_real);
#pragma omp parallel for schedule(static)
  for (int64_t i = i0; i < i1; ++i)
    knn_one<T, MIXED, S>(r, n_real, i, k, r2 + (i - i0) * k, idx + (i - i0) * k);
  return 0;
}

template <typename T>
double hermite_first_dt(const T* A4, const T* J4, int64_t n, double eta) {
  double dtm = INFINITY;
#pragma omp parallel for schedule(static) reduction(min : dtm)
  for (int64_t i = 0; i < n; ++i) {
    const double a[3] = {A4[4 * i], A4[4 * i + 1], A4[4 * i + 2]};
    const double j[3] = {J4[4 * i], J4[4 * i + 1], J4[4 * i + 2]};
    double d;
    if (gs::hermite_first_dt(eta, a, j, d) && d < dtm) dtm = d;
  }
  return dtm;
}

// One step of size h in place (the GPU chain's predict / evaluate / correct arithmetic).
// scratch: xp, vp, a1, j1 (n_real * 4 each).
// MIXED (T = double): the evaluation goes through the double-single fp32 pair arithmetic.
template <typename T, bool MIXED = false>
int hermite_step(T* X4, T* V4, T* A4, T* J4, T* scratch, int64_t n, int32_t chunk, double hd,
                 T cut2, T eps2, double eta, double* dt_min_out) {
  if (chunk <= 0 || n < 1 || !(hd > 0.0) || !scratch) {
    gs_set_error("cpu_hermite_step: bad arguments");
    return -1;
  }
  T *XP = scratch, *VP = scratch + 4 * n, *A1 = scratch + 8 * n, *J1 = scratch + 12 * n;
  const T h = (T)hd;
  const T h2 = (h * h) / T(2), h3 = (h * h * h) / T(6);
#pragma omp parallel for schedule(static)
  for (int64_t i = 0; i < n; ++i) {
    for (int d = 0; d < 3; ++d) {
      const int64_t k = 4 * i + d;
      gs::h4_predict(h, h2, h3, X4[k], V4[k], A4[k], J4[k], XP[k], VP[k]);
    }
    XP[4 * i + 3] = X4[4 * i + 3];
    VP[4 * i + 3] = 0;
  }
  if (accjerk_rows<T, MIXED>(XP, VP, n, nullptr, 0, n, chunk, cut2, eps2, A1, J1)) return -1;
  const T hh = h / T(2), h12 = (h * h) / T(12);
  double dtm = INFINITY;
#pragma omp parallel for schedule(static) reduction(min : dtm)
  for (int64_t i = 0; i < n; ++i) {
    double a0[3], j0[3], a1[3], j1[3];
    for (int d = 0; d < 3; ++d) {
      const int64_t k = 4 * i + d;
      a0[d] = A4[k]; j0[d] = J4[k]; a1[d] = A1[k]; j1[d] = J1[k];
      T x1, v1;
      gs::h4_correct(hh, h12, X4[k], V4[k], A4[k], J4[k], A1[k], J1[k], x1, v1);
      X4[k] = x1;
      V4[k] = v1;
      A4[k] = A1[k];
      J4[k] = J1[k];
    }
    A4[4 * i + 3] = 0;
    J4[4 * i + 3] = 0;
    double d;
    if (eta > 0.0 && gs::h4_dt(hd, eta, a0, j0, a1, j1, d) && d < dtm) dtm = d;
  }
  if (dt_min_out) *dt_min_out = dtm;
  return 0;
}

// ---- 6th-order Hermite (Nitadori & Makino 2008; gs_hermite_scheme.h) ----------------------
// One 6th-order step of size h in place (the GPU chain's predict / evaluate / correct
// arithmetic, gs_hermite_scheme.h). scratch: xp, vp, ap, a1, j1, s1 (n * 4 each).
template <typename T>
int hermite6_step(T* X4, T* V4, T* A4, T* J4, T* S4, T* C4, T* scratch, int64_t n, int32_t chunk,
                  double hd, T cut2, T eps2, double eta, double* dt_min_out) {
  if (chunk <= 0 || n < 1 || !(hd > 0.0) || !scratch || !X4 || !V4 || !A4 || !J4 || !S4 || !C4) {
    gs_set_error("cpu_hermite6_step: bad arguments");
    return -1;
  }
  T *XP = scratch, *VP = scratch + 4 * n, *AP = scratch + 8 * n, *A1 = scratch + 12 * n,
    *J1 = scratch + 16 * n, *S1 = scratch + 20 * n;
  const T h = (T)hd;
  const gs::H6Taylor<T> tl = gs::h6_taylor(h);
#pragma omp parallel for schedule(static)
  for (int64_t i = 0; i < n; ++i) {
    for (int d = 0; d < 3; ++d) {
      const int64_t k = 4 * i + d;
      gs::h6_predict(tl, X4[k], V4[k], A4[k], J4[k], S4[k], C4[k], XP[k], VP[k], AP[k]);
    }
    XP[4 * i + 3] = X4[4 * i + 3];
    VP[4 * i + 3] = 0;
    AP[4 * i + 3] = 0;
  }
  if (accjerk_rows<T, false, true>(XP, VP, n, nullptr, 0, n, chunk, cut2, eps2, A1, J1, AP, S1))
    return -1;
  double dtm = INFINITY;
#pragma omp parallel for schedule(static) reduction(min : dtm)
  for (int64_t i = 0; i < n; ++i) {
    double a1[3], j1[3], s1[3], c1[3], p1[3], a5[3];
    for (int d = 0; d < 3; ++d) {
      const int64_t k = 4 * i + d;
      T x1, v1;
      gs::h6_correct(h, X4[k], V4[k], A4[k], J4[k], S4[k], A1[k], J1[k], S1[k], x1, v1);
      a1[d] = A1[k]; j1[d] = J1[k]; s1[d] = S1[k];
      gs::h6_high(hd, A4[k], J4[k], S4[k], a1[d], j1[d], s1[d], c1[d], p1[d], a5[d]);
      X4[k] = x1; V4[k] = v1;
      A4[k] = A1[k]; J4[k] = J1[k]; S4[k] = S1[k]; C4[k] = (T)c1[d];
    }
    A4[4 * i + 3] = 0; J4[4 * i + 3] = 0; S4[4 * i + 3] = 0; C4[4 * i + 3] = 0;
    double d;
    if (eta > 0.0 && gs::h6_dt(eta, a1, j1, s1, c1, p1, a5, d) && d < dtm) dtm = d;
  }
  if (dt_min_out) *dt_min_out = dtm;
  return 0;
}

}  // namespace

extern "C" {

int gs_cpu_accjerksnap_f64(const double* X4, const double* V4, const double* A4, int64_t n_real,
                           int64_t i0, int64_t i1, int32_t chunk, double cut2, double eps2,
                           double* acc4, double* jerk4, double* snap4) {
  return accjerk_rows<double, false, true>(X4, V4, n_real, nullptr, i0, i1 - i0, chunk, cut2, eps2,
                                           acc4, jerk4, A4, snap4);
}
int gs_cpu_accjerksnap_f32(const float* X4, const float* V4, const float* A4, int64_t n_real,
                           int64_t i0, int64_t i1, int32_t chunk, float cut2, float eps2,
                           float* acc4, float* jerk4, float* snap4) {
  return accjerk_rows<float, false, true>(X4, V4, n_real, nullptr, i0, i1 - i0, chunk, cut2, eps2,
                                          acc4, jerk4, A4, snap4);
}
int gs_cpu_accjerksnap_idx_f64(const double* X4, const double* V4, const double* A4,
                               int64_t n_real, const int32_t* idx, int64_t n_idx, int32_t chunk,
                               double cut2, double eps2, double* acc4, double* jerk4,
                               double* snap4) {
  if (!list_ok("cpu_accjerksnap_idx", idx, n_idx)) return -1;
  return accjerk_rows<double, false, true>(X4, V4, n_real, idx, 0, n_idx, chunk, cut2, eps2, acc4,
                                           jerk4, A4, snap4);
}
int gs_cpu_hermite6_step_f64(double* X4, double* V4, double* A4, double* J4, double* S4,
                             double* C4, double* scratch, int64_t n_real, int32_t chunk, double h,
                             double cut2, double eps2, double eta, double* dt_min_out) {
  return hermite6_step<double>(X4, V4, A4, J4, S4, C4, scratch, n_real, chunk, h, cut2, eps2, eta,
                               dt_min_out);
}
int gs_cpu_hermite6_step_f32(float* X4, float* V4, float* A4, float* J4, float* S4, float* C4,
                             float* scratch, int64_t n_real, int32_t chunk, double h, float cut2,
                             float eps2, double eta, double* dt_min_out) {
  return hermite6_step<float>(X4, V4, A4, J4, S4, C4, scratch, n_real, chunk, h, cut2, eps2, eta,
                              dt_min_out);
}

int gs_cpu_accel_abs_f64(const double* X4, int64_t n_real, int64_t i0, int64_t i1, double cut2,
                         double eps2, double* out8) {
  return accel_abs_range<double>(X4, n_real, i0, i1, cut2, eps2, out8);
}
int gs_cpu_accel_abs_ld(const double* X4, int64_t n_real, int64_t i0, int64_t i1, double cut2,
                        double eps2, double* out8) {
  return accel_abs_range<long double>(X4, n_real, i0, i1, cut2, eps2, out8);
}

int gs_cpu_accel_f64(const double* X4, int64_t n_real, int64_t i0, int64_t i1, int32_t chunk,
                     double cut2, double eps2, double* acc4) {
  return accel_range<double>(X4, n_real, i0, i1, chunk, cut2, eps2, acc4);
}
int gs_cpu_accel_f32(const float* X4, int64_t n_real, int64_t i0, int64_t i1, int32_t chunk,
                     float cut2, float eps2, float* acc4) {
  return accel_range<float>(X4, n_real, i0, i1, chunk, cut2, eps2, acc4);
}
int gs_cpu_step_f64(const double* X4, double* Xn4, double* vel4, int64_t n_real, int64_t i0,
                    int64_t i1, int32_t chunk, double dt, double cut2, double eps2) {
  return step_range<double>(X4, Xn4, vel4, n_real, i0, i1, chunk, dt, cut2, eps2);
}
int gs_cpu_step_f32(const float* X4, float* Xn4, float* vel4, int64_t n_real, int64_t i0,
                    int64_t i1, int32_t chunk, float dt, float cut2, float eps2) {
  return step_range<float>(X4, Xn4, vel4, n_real, i0, i1, chunk, dt, cut2, eps2);
}
int gs_cpu_accjerk_f64(const double* X4, const double* V4, int64_t n_real, int64_t i0, int64_t i1,
                       int32_t chunk, double cut2, double eps2, double* acc4, double* jerk4) {
  return accjerk_rows<double, false>(X4, V4, n_real, nullptr, i0, i1 - i0, chunk, cut2, eps2, acc4,
                                     jerk4);
}
int gs_cpu_accjerk_f32(const float* X4, const float* V4, int64_t n_real, int64_t i0, int64_t i1,
                       int32_t chunk, float cut2, float eps2, float* acc4, float* jerk4) {
  return accjerk_rows<float, false>(X4, V4, n_real, nullptr, i0, i1 - i0, chunk, cut2, eps2, acc4,
                                    jerk4);
}
int gs_cpu_accjerk_mixed(const double* X4, const double* V4, int64_t n_real, int64_t i0,
                         int64_t i1, int32_t chunk, double cut2, double eps2, double* acc4,
                         double* jerk4) {
  return accjerk_rows<double, true>(X4, V4, n_real, nullptr, i0, i1 - i0, chunk, cut2, eps2, acc4,
                                    jerk4);
}
int gs_cpu_accjerk_idx_f64(const double* X4, const double* V4, int64_t n_real, const int32_t* idx,
                           int64_t n_idx, int32_t chunk, double cut2, double eps2, double* acc4,
                           double* jerk4) {
  if (!list_ok("cpu_accjerk_idx", idx, n_idx)) return -1;
  return accjerk_rows<double, false>(X4, V4, n_real, idx, 0, n_idx, chunk, cut2, eps2, acc4,
                                     jerk4);
}
int gs_cpu_accjerk_idx_f32(const float* X4, const float* V4, int64_t n_real, const int32_t* idx,
                           int64_t n_idx, int32_t chunk, float cut2, float eps2, float* acc4,
                           float* jerk4) {
  if (!list_ok("cpu_accjerk_idx", idx, n_idx)) return -1;
  return accjerk_rows<float, false>(X4, V4, n_real, idx, 0, n_idx, chunk, cut2, eps2, acc4,
                                    jerk4);
}
int gs_cpu_accjerk_idx_mixed(const double* X4, const double* V4, int64_t n_real,
                             const int32_t* idx, int64_t n_idx, int32_t chunk, double cut2,
                             double eps2, double* acc4, double* jerk4) {
  if (!list_ok("cpu_accjerk_idx", idx, n_idx)) return -1;
  return accjerk_rows<double, true>(X4, V4, n_real, idx, 0, n_idx, chunk, cut2, eps2, acc4,
                                    jerk4);
}
int gs_cpu_nn_f64(const double* X4, const double* R, int64_t n_real, int64_t i0, int64_t i1,
                  double cut2, double eps2, double* q, int32_t* nn) {
  return nn_rows<double, false>(X4, R, n_real, nullptr, i0, i1 - i0, cut2, eps2, q, nn);
}
int gs_cpu_nn_f32(const float* X4, const float* R, int64_t n_real, int64_t i0, int64_t i1,
                  float cut2, float eps2, float* q, int32_t* nn) {
  return nn_rows<float, false>(X4, R, n_real, nullptr, i0, i1 - i0, cut2, eps2, q, nn);
}
int gs_cpu_nn_mixed(const double* X4, const double* R, int64_t n_real, int64_t i0, int64_t i1,
                    double cut2, double eps2, double* q, int32_t* nn) {
  return nn_rows<double, true>(X4, R, n_real, nullptr, i0, i1 - i0, cut2, eps2, q, nn);
}
int gs_cpu_nn_idx_f64(const double* X4, const double* R, int64_t n_real, const int32_t* idx,
                      int64_t n_idx, double cut2, double eps2, double* q, int32_t* nn) {
  if (!idx) { gs_set_error("cpu_nn_idx: null argument"); return -1; }
  return nn_rows<double, false>(X4, R, n_real, idx, 0, n_idx, cut2, eps2, q, nn);
}
int gs_cpu_nn_idx_f32(const float* X4, const float* R, int64_t n_real, const int32_t* idx,
                      int64_t n_idx, float cut2, float eps2, float* q, int32_t* nn) {
  if (!idx) { gs_set_error("cpu_nn_idx: null argument"); return -1; }
  return nn_rows<float, false>(X4, R, n_real, idx, 0, n_idx, cut2, eps2, q, nn);
}
int gs_cpu_nn_idx_mixed(const double* X4, const double* R, int64_t n_real, const int32_t* idx,
                        int64_t n_idx, double cut2, double eps2, double* q, int32_t* nn) {
  if (!idx) { gs_set_error("cpu_nn_idx: null argument"); return -1; }
  return nn_rows<double, true>(X4, R, n_real, idx, 0, n_idx, cut2, eps2, q, nn);
}
int gs_cpu_knn_f64(const double* X4, int64_t n_real, int64_t i0, int64_t i1, int32_t k,
                   double* r2, int32_t* idx) {
  return knn_rows<double, false>(X4, n_real, i0, i1, k, r2, idx);
}
int gs_cpu_knn_f32(const float* X4, int64_t n_real, int64_t i0, int64_t i1, int32_t k, float* r2,
                   int32_t* idx) {
  return knn_rows<float, false>(X4, n_real, i0, i1, k, r2, idx);
}
int gs_cpu_knn_mixed(const double* X4, int64_t n_real, int64_t i0, int64_t i1, int32_t k,
                     double* r2, int32_t* idx) {
  return knn_rows<double, true>(X4, n_real, i0, i1, k, r2, idx);
}
double gs_cpu_hermite_first_dt_f64(const double* A4, const double* J4, int64_t n_real,
                                   double eta) {
  return hermite_first_dt<double>(A4, J4, n_real, eta);
}
double gs_cpu_hermite_first_dt_f32(const float* A4, const float* J4, int64_t n_real, double eta) {
  return hermite_first_dt<float>(A4, J4, n_real, eta);
}
int gs_cpu_hermite_step_f64(double* X4, double* V4, double* A4, double* J4, double* scratch,
                            int64_t n_real, int32_t chunk, double h, double cut2, double eps2,
                            double eta, double* dt_min_out) {
  return hermite_step<double>(X4, V4, A4, J4, scratch, n_real, chunk, h, cut2, eps2, eta,
                              dt_min_out);
}
int gs_cpu_hermite_step_f32(float* X4, float* V4, float* A4, float* J4, float* scratch,
                            int64_t n_real, int32_t chunk, double h, float cut2, float eps2,
                            double eta, double* dt_min_out) {
  return hermite_step<float>(X4, V4, A4, J4, scratch, n_real, chunk, h, cut2, eps2, eta,
                             dt_min_out);
}
int gs_cpu_hermite_step_mixed(double* X4, double* V4, double* A4, double* J4, double* scratch,
                              int64_t n_real, int32_t chunk, double h, double cut2, double eps2,
                              double eta, double* dt_min_out) {
  return hermite_step<double, true>(X4, V4, A4, J4, scratch, n_real, chunk, h, cut2, eps2, eta,
                                    dt_min_out);
}
int gs_cpu_set_threads(int32_t n) {
#ifdef _OPENMP
  if (n > 0) omp_set_num_threads(n);
  return omp_get_max_threads();
#else
  (void)n;
  return 1;
#endif
}

int gs_cpu_num_threads(void) {
#ifdef _OPENMP
  return omp_get_max_threads();
#else
  return 1;
#endif
}

}  // extern "C"
