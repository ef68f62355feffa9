// Device helpers shared by the one-sided force kernels (nbody_kernels.hip), the Hermite kernels
// of both orders (nbody_hermite.hip, nbody_hermite6.hip) and the k-nearest-neighbour kernel
// (nbody_knn.hip): 4-vectors, the reciprocal square root, the fused multiply-adds, the helpers of
// a pair term written once over its element type (a scalar or a 2-vector: fmav, inv_cut, vget /
// vset), the workgroup minimum, the LDS-DMA tile fill and the geometry an evaluate launch must
// have.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "gs_common.h"

namespace gs {

template <typename T> struct VecT;
template <> struct VecT<float> { using type = float __attribute__((ext_vector_type(4))); };
template <> struct VecT<double> { using type = double __attribute__((ext_vector_type(4))); };
template <typename T> using V4 = typename VecT<T>::type;

constexpr int kBlock = kForceBlock;  // 256 = 4 waves of 64

__device__ __forceinline__ float rsqrt_dev(float x) { return __builtin_amdgcn_rsqf(x); }

// fp64: v_rsq_f64 seed (max relative error 5.2e-8, measured: profiles/r1_microbench_v3.jsonl)
// + one Halley step, cubically convergent: e = 1 - x y^2, y <- y + y e (1/2 + 3/8 e).
// (5.2e-8)^3 is far below 2^-53, so one step reaches double precision in 5 f64 ops where two
// Newton steps need 7 (512K fp64: profiles/r1_sweep_512k_fp64_halley.log vs _newton.log).
__device__ __forceinline__ double rsqrt_dev(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  const double e = __builtin_fma(-x * y, y, 1.0);
  const double p = __builtin_fma(e, 0.375, 0.5);
  return __builtin_fma(y * e, p, y);
}

__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }

// Two fp32 values per lane as one 2-vector (v_pk_* operands).
using f2 = float __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }

// The pair terms are written once over their element type V: a scalar T (one i-body) or, fp32
// with an even number of bodies per lane, f2 (two i-bodies, v_pk_* operations). Each element of
// a 2-vector sees exactly the scalar arithmetic, so the bits do not depend on the packing.

// The fused multiply-add of V: fma_ (a scalar) or fma2 (a pair).
template <typename V>
__device__ __forceinline__ V fmav(V a, V b, V c) {
  if constexpr (std::is_same<V, f2>::value) return fma2(a, b, c);
  else return fma_(a, b, c);
}

// Element e of a V (a scalar is its own element 0).
template <typename V, typename T>
__device__ __forceinline__ void vset(V& dst, int e, T v) {
  if constexpr (std::is_same<V, f2>::value) {
    if (e == 0) dst.x = v; else dst.y = v;
  } else {
    dst = v;
  }
}
template <typename V>
__device__ __forceinline__ auto vget(const V& src, int e) {
  if constexpr (std::is_same<V, f2>::value) return e == 0 ? src.x : src.y;
  else return src;
}

__device__ __forceinline__ f2 rsqrt_dev(f2 x) {
  f2 y;
  y.x = rsqrt_dev(x.x);
  y.y = rsqrt_dev(x.y);
  return y;
}

// 1 / sqrt(r2) where the pair law keeps the pair (r2 >= cut2), else 0.
__device__ __forceinline__ float inv_cut(float r2, float cut2) {
  return r2 >= cut2 ? rsqrt_dev(r2) : 0.0f;
}
__device__ __forceinline__ f2 inv_cut(f2 r2, float cut2) {
  f2 inv;
  inv.x = r2.x >= cut2 ? rsqrt_dev(r2.x) : 0.0f;
  inv.y = r2.y >= cut2 ? rsqrt_dev(r2.y) : 0.0f;
  return inv;
}
__device__ __forceinline__ double inv_cut(double r2, double cut2) {
  // Branch-free: the refinement would otherwise be predicated behind exec-mask jumps; it runs
  // on 1 below the cutoff.
  const bool ok = r2 >= cut2;
  const double inv = rsqrt_dev(ok ? r2 : 1.0);
  return ok ? inv : 0.0;
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

// LDS tile geometry: kTileBytes per tile buffer (4 KiB = 256 fp32 / 128 fp64 bodies),
// double-buffered. Each wave-instruction of the fill moves one 1-KiB piece.
constexpr int kTileBytes = 4096;
static_assert(kTileBytes % 1024 == 0, "tile must be whole 1 KiB wave pieces");
template <typename T> struct Tile { static constexpr int kBodies = kTileBytes / sizeof(V4<T>); };

// The geometry of a chunked evaluate launch over n_pad rows with ipl i-bodies per lane: whole
// chunks of whole tiles, whole workgroups of ipl rows per lane.
template <typename T>
inline bool chunk_geometry_ok(int64_t n_pad, int64_t chunk, int32_t n_chunks, int ipl) {
  return n_chunks >= 1 && n_pad % (kBlock * ipl) == 0 && chunk % Tile<T>::kBodies == 0 &&
         (int64_t)n_chunks * chunk == n_pad;
}

// Issue the LDS-DMA fill of one tile: per round each of the 4 waves moves one 1-KiB piece
// (64 lanes x 16 B); the LDS destination is the wave-uniform base + lane*16.
template <typename T>
__device__ __forceinline__ void tile_fill(const V4<T>* __restrict__ src, V4<T>* dst) {
  constexpr int kRound = kBlock * 16;  // bytes one pass of the workgroup moves
  static_assert(kTileBytes % kRound == 0, "tile must be whole workgroup x 1 KiB-per-wave passes");
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < kTileBytes / kRound; ++r) {
    const char* g = reinterpret_cast<const char*>(src) + r * kRound + wave * 1024 + lane * 16;
    char* l = reinterpret_cast<char*>(dst) + r * kRound + wave * 1024;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)l, 16, 0, 0);
  }
}

}  // namespace gs
