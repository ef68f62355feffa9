// gfx950 k-nearest-neighbour kernel (the Casertano & Hut local density rests on it) and its
// stateless entry point gs_hip_knn.
//
// Definition (every layer implements exactly it): the k nearest neighbours of body i are the
// first k entries of the ascending lexicographic order on (r^2_ij, j) over the real bodies
// j != i. The body itself is left out by index, never by distance; r^2 is formed in the pair
// type as d = x_j - x_i (mixed: hsep's (hi_j - hi_i) + (lo_j - lo_i)), r^2 = fma(dz, dz,
// fma(dy, dy, dx dx)), with no softening and no cutoff. Entries past the n - 1 neighbours there
// are read (+inf, -1). The order is total, so the lists are a property of the body set: any
// launch shape gives the same bits.
//   * One-sided and i-owned like hermite_eval_kernel: a lane owns IPL i-bodies, the j position
//     rows (and the lo rows of a mixed run) arrive in double-buffered LDS tiles by LDS-DMA
//     (tile_fill) and are read back as broadcast ds_read_b128; no atomics.
//   * Every i-body carries an ascending list of kKnnMax (r^2, j) in registers. A candidate
//     enters by a branch-free compare-and-select chain with a strict less, so within a sweep in
//     ascending j the lower j keeps an exact tie.
//   * The chain costs several times the r^2 itself and a body accepts only O(k log N)
//     candidates per sweep, so the chain sits behind a wave-uniform test: does any lane of the
//     wave hold a body whose candidate beats the worst of its list (GS_KNN_EARLY, a
//     compile-time knob for the A/B of bench/knn_rate.py; the bits are the same either way).
//   * Grid (n_pad / (256 IPL), groups): workgroup (b, g) sweeps the canonical chunks
//     (gs::auto_chunk) of group g and stores its list per body; knn_merge_kernel folds the
//     groups' lists of a body under the lexicographic order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "gravsim.h"
#include "gs_common.h"
#include "gs_stepper.h"
#include "gs_tile.h"

#ifndef GS_KNN_EARLY
#define GS_KNN_EARLY 1
#endif

namespace gs {

constexpr int kKnnMax = 8;

struct KnnArgs {
  const void* X;   // [n_pad] rows (x, y, z, 0) of the pair type (mixed: the hi parts)
  const void* XL;  // mixed: [n_pad] rows of the lo parts
  void* LR;        // [groups][kKnnMax][n_pad] r^2 of the groups' lists (pair type)
  int32_t* LI;     // [groups][kKnnMax][n_pad] their j
  double* R;       // [n_real][k] merged r^2
  int32_t* I;      // [n_real][k] merged j
  int64_t n_real, n_pad;
  int32_t chunk, n_chunks, k, groups;
};

template <typename T, int IPL>
struct KList {
  T r[IPL][kKnnMax];
  int32_t n[IPL][kKnnMax];
};

// (c, j) into the ascending list: slot s takes its upper neighbour when the candidate goes
// above it, the candidate when it goes exactly there, and keeps its entry otherwise.
template <typename T>
__device__ __forceinline__ void knn_insert(T* r, int32_t* n, T c, int32_t j) {
#pragma unroll
  for (int s = kKnnMax - 1; s > 0; --s) {
    const bool up = c < r[s - 1], here = c < r[s];
    r[s] = up ? r[s - 1] : (here ? c : r[s]);
    n[s] = up ? n[s - 1] : (here ? j : n[s]);
  }
  const bool here = c < r[0];
  r[0] = here ? c : r[0];
  n[0] = here ? j : n[0];
}

// The same under the full order on (r^2, j): the merge of lists from different j ranges.
template <typename T>
__device__ __forceinline__ bool knn_less(T c, int32_t j, T r, int32_t n) {
  return c < r || (c == r && j < n);
}

template <typename T>
__device__ __forceinline__ void knn_insert_lex(T* r, int32_t* n, T c, int32_t j) {
#pragma unroll
  for (int s = kKnnMax - 1; s > 0; --s) {
    const bool up = knn_less(c, j, r[s - 1], n[s - 1]), here = knn_less(c, j, r[s], n[s]);
    r[s] = up ? r[s - 1] : (here ? c : r[s]);
    n[s] = up ? n[s - 1] : (here ? j : n[s]);
  }
  const bool here = knn_less(c, j, r[0], n[0]);
  r[0] = here ? c : r[0];
  n[0] = here ? j : n[0];
}

template <bool DS, typename V>
__device__ __forceinline__ V knn_sep(V qh, V xh, V ql, V xl) {
  if constexpr (DS) return (qh - xh) + (ql - xl);
  return qh - xh;
}

// r^2 of the lane's IPL bodies against row q (l: its lo row). fp32 with two bodies per lane
// runs as 2-vectors (v_pk_*); each element sees the scalar arithmetic.
template <typename T, int IPL, bool DS>
__device__ __forceinline__ void knn_r2(const T* x, const T* y, const T* z, const T* lx,
                                       const T* ly, const T* lz, const V4<T>& q, const V4<T>& l,
                                       T* r2) {
  if constexpr (sizeof(T) == 4 && IPL == 2) {
    const f2 dx = knn_sep<DS>(f2(q.x), f2{x[0], x[1]}, f2(l.x), f2{lx[0], lx[1]});
    const f2 dy = knn_sep<DS>(f2(q.y), f2{y[0], y[1]}, f2(l.y), f2{ly[0], ly[1]});
    const f2 dz = knn_sep<DS>(f2(q.z), f2{z[0], z[1]}, f2(l.z), f2{lz[0], lz[1]});
    const f2 v = __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
    r2[0] = v.x;
    r2[1] = v.y;
  } else {
#pragma unroll
    for (int k = 0; k < IPL; ++k) {
      const T dx = knn_sep<DS>(q.x, x[k], l.x, lx[k]), dy = knn_sep<DS>(q.y, y[k], l.y, ly[k]),
              dz = knn_sep<DS>(q.z, z[k], l.z, lz[k]);
      r2[k] = fma_(dz, dz, fma_(dy, dy, dx * dx));
    }
  }
}

template <typename T, int IPL, bool DS>
__global__ __launch_bounds__(kBlock) void knn_kernel(KnnArgs a) {
  constexpr int TB = Tile<T>::kBodies;
  __shared__ __attribute__((aligned(16))) V4<T> tx[2][TB];
  __shared__ __attribute__((aligned(16))) V4<T> tl[2][DS ? TB : 1];
  const int64_t ib = (int64_t)blockIdx.x * (kBlock * IPL);
  if (ib >= a.n_real) return;  // a block of ghost rows
  const int per = (a.n_chunks + (int)gridDim.y - 1) / (int)gridDim.y;
  const int c0 = (int)blockIdx.y * per;
  const int c1 = min(c0 + per, a.n_chunks);
  const int tpc = (int)(a.chunk / TB);  // tiles per chunk
  const int ntiles = max(c1 - c0, 0) * tpc;
  const V4<T>* X = reinterpret_cast<const V4<T>*>(a.X);
  const V4<T>* XL = reinterpret_cast<const V4<T>*>(a.XL);
  T x[IPL], y[IPL], z[IPL], lx[IPL], ly[IPL], lz[IPL];
  int32_t self[IPL];
  KList<T, IPL> ls;
#pragma unroll
  for (int k = 0; k < IPL; ++k) {
    const int64_t row = ib + threadIdx.x + k * kBlock;
    const V4<T> p = X[row];
    x[k] = p.x; y[k] = p.y; z[k] = p.z;
    lx[k] = ly[k] = lz[k] = T(0);
    if constexpr (DS) {
      const V4<T> l = XL[row];
      lx[k] = l.x; ly[k] = l.y; lz[k] = l.z;
    }
    self[k] = (int32_t)row;
#pragma unroll
    for (int s = 0; s < kKnnMax; ++s) {
      ls.r[k][s] = T(INFINITY);
      ls.n[k][s] = -1;
    }
  }
  auto fill = [&](int t) {
    const int64_t j0 = (int64_t)(c0 + t / tpc) * a.chunk + (int64_t)(t % tpc) * TB;
    tile_fill<T>(X + j0, tx[t & 1]);
    if constexpr (DS) tile_fill<T>(XL + j0, tl[t & 1]);
  };
  if (ntiles > 0) fill(0);
  const int32_t nreal = (int32_t)a.n_real;
  for (int t = 0; t < ntiles; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // tile t is in LDS for every wave; buffer (t+1)&1 is free
    if (t + 1 < ntiles) fill(t + 1);
    const V4<T>* cx = tx[t & 1];
    const V4<T>* cl = tl[t & 1];
    const int32_t jb = (int32_t)((int64_t)(c0 + t / tpc) * a.chunk + (int64_t)(t % tpc) * TB);
#pragma unroll 4
    for (int j = 0; j < TB; ++j) {
      const V4<T> q = cx[j];  // uniform address: a broadcast ds_read
      V4<T> l = V4<T>();
      if constexpr (DS) l = cl[j];
      const int32_t jg = jb + j;
      const bool jreal = jg < nreal;  // (scalar: j is uniform over the wave)
      T c[IPL];
      knn_r2<T, IPL, DS>(x, y, z, lx, ly, lz, q, l, c);
      bool any = false;
#pragma unroll
      for (int k = 0; k < IPL; ++k) {
        c[k] = (jreal && jg != self[k]) ? c[k] : T(INFINITY);
        any = any || c[k] < ls.r[k][kKnnMax - 1];
      }
#if GS_KNN_EARLY
      if (__any(any)) {
#else
      {
#endif
#pragma unroll
        for (int k = 0; k < IPL; ++k) knn_insert<T>(ls.r[k], ls.n[k], c[k], jg);
      }
    }
  }
  T* LR = reinterpret_cast<T*>(a.LR);
#pragma unroll
  for (int k = 0; k < IPL; ++k) {
    const int64_t row = ib + threadIdx.x + k * kBlock;
#pragma unroll
    for (int s = 0; s < kKnnMax; ++s) {
      const int64_t o = ((int64_t)blockIdx.y * kKnnMax + s) * a.n_pad + row;
      LR[o] = ls.r[k][s];
      a.LI[o] = ls.n[k][s];
    }
  }
}

// MERGE: one lane per real body folds the groups' lists and writes the first k entries.
template <typename T>
__global__ __launch_bounds__(kBlock) void knn_merge_kernel(KnnArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n_real) return;
  const T* LR = reinterpret_cast<const T*>(a.LR);
  T r[kKnnMax];
  int32_t n[kKnnMax];
#pragma unroll
  for (int s = 0; s < kKnnMax; ++s) {
    r[s] = T(INFINITY);
    n[s] = -1;
  }
  for (int g = 0; g < a.groups; ++g) {
#pragma unroll
    for (int s = 0; s < kKnnMax; ++s) {
      const int64_t o = ((int64_t)g * kKnnMax + s) * a.n_pad + i;
      const int32_t j = a.LI[o];
      if (j >= 0) knn_insert_lex<T>(r, n, LR[o], j);
    }
  }
#pragma unroll
  for (int s = 0; s < kKnnMax; ++s) {
    if (s < a.k) {
      a.R[i * a.k + s] = (double)r[s];
      a.I[i * a.k + s] = n[s];
    }
  }
}

template <typename T, int IPL, bool DS>
static void knn_launch_t(const KnnArgs& a, hipStream_t s) {
  const dim3 grid((unsigned)(a.n_pad / (kBlock * IPL)), (unsigned)a.groups);
  hipLaunchKernelGGL((knn_kernel<T, IPL, DS>), grid, dim3(kBlock), 0, s, a);
  hipLaunchKernelGGL((knn_merge_kernel<T>), dim3((unsigned)((a.n_real + kBlock - 1) / kBlock)),
                     dim3(kBlock), 0, s, a);
}

static void knn_launch(const KnnArgs& a, int32_t dtype, int32_t ipl, hipStream_t s) {
  if (dtype == GS_FP64) {
    if (ipl == 2) knn_launch_t<double, 2, false>(a, s);
    else knn_launch_t<double, 1, false>(a, s);
  } else if (dtype == GS_MIXED) {
    if (ipl == 2) knn_launch_t<float, 2, true>(a, s);
    else knn_launch_t<float, 1, true>(a, s);
  } else {
    if (ipl == 2) knn_launch_t<float, 2, false>(a, s);
    else knn_launch_t<float, 1, false>(a, s);
  }
}

// What one call owns on the device; freed on every way out.
struct KnnScratch {
  void *X = nullptr, *XL = nullptr, *LR = nullptr, *LI = nullptr, *R = nullptr, *I = nullptr;
  rt::DevMem mem;  // (the six above)
  hipStream_t s = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int prev = -1;
  ~KnnScratch() {
    if (s) (void)hipStreamSynchronize(s);
    mem.release();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (s) (void)hipStreamDestroy(s);
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

#define GS_KNN_HIP(call)                                                            \
  do {                                                                              \
    hipError_t e_ = (call);                                                         \
    if (e_ != hipSuccess) {                                                         \
      char b_[384];                                                                 \
      snprintf(b_, sizeof(b_), "%s:%d %s: %s", __FILE__, __LINE__, #call,           \
               hipGetErrorString(e_));                                              \
      gs_set_error(b_);                                                             \
      return -1;                                                                    \
    }                                                                               \
  } while (0)

template <typename T>
static void knn_rows(const double* pos, int64_t n, int64_t n_pad, bool mixed, std::vector<T>& H,
                     std::vector<T>& L) {
  H.assign((size_t)n_pad * 4, T(0));
  if (mixed) L.assign((size_t)n_pad * 4, T(0));
  for (int64_t i = 0; i < n; ++i)
    for (int d = 0; d < 3; ++d) {
      const T hi = (T)pos[3 * i + d];
      H[4 * i + d] = hi;
      if (mixed) L[4 * i + d] = (T)(pos[3 * i + d] - (double)hi);
    }
}

// reps launches of kernel + merge, each between two events (ms, if given, gets their
// milliseconds); the last one's lists are downloaded when r2 / idx are given.
static int knn_run(const double* pos, int64_t n, int32_t dtype, int32_t k, int32_t ipl,
                   int32_t groups, int32_t device, int32_t reps, double* ms, double* r2,
                   int32_t* idx, int64_t* info) {
  if (!pos || n < 1 || n > (int64_t)1 << 30 || k < 1 || k > kKnnMax || reps < 1 ||
      (dtype != GS_FP32 && dtype != GS_FP64 && dtype != GS_MIXED) || groups < 0 ||
      !gs_knn_ipl_ok(dtype, ipl)) {
    gs_set_error("gs_hip_knn: bad arguments (n >= 1, k in 1..8, ipl 0 / 1 / 2, groups >= 0)");
    return -1;
  }
  KnnArgs a{};
  a.n_real = n;
  a.chunk = auto_chunk(n);
  a.n_pad = round_up(n, a.chunk);
  a.n_chunks = (int32_t)(a.n_pad / a.chunk);
  a.k = k;
  // Auto shape, from the sweep of profiles/knn_shapes.json (16K, 64K and 256K bodies): one body
  // per lane everywhere (the wave-uniform test then speaks for 64 bodies, not 128, and twice the
  // waves fit), and chunk groups up to about 2048 (fp64: 1024) workgroups but 4 at the least;
  // more groups cost insertions, since every group fills a list of its own from empty.
  if (ipl == 0) ipl = 1;
  const int64_t iblocks = a.n_pad / (kBlock * ipl);
  if (groups == 0) {
    const int64_t want = dtype == GS_FP64 ? 1024 : 2048;
    groups = (int32_t)((want + iblocks - 1) / iblocks);
    if (groups < 4) groups = 4;
  }
  if (groups > a.n_chunks) groups = a.n_chunks;
  const int per = (a.n_chunks + groups - 1) / groups;
  a.groups = (a.n_chunks + per - 1) / per;  // (no group without a chunk)
  const size_t esz = dtype == GS_FP64 ? 8 : 4;
  std::vector<double> Hd, Ld;
  std::vector<float> Hf, Lf;
  KnnScratch d;  // (after the host rows: a copy in flight ends before they go)
  GS_KNN_HIP(hipGetDevice(&d.prev));
  GS_KNN_HIP(hipSetDevice(device));
  GS_KNN_HIP(hipStreamCreateWithFlags(&d.s, hipStreamNonBlocking));
  GS_KNN_HIP(hipEventCreate(&d.e0));
  GS_KNN_HIP(hipEventCreate(&d.e1));
  const size_t rows = (size_t)a.n_pad * 4 * esz, lists = (size_t)a.groups * kKnnMax * a.n_pad;
  if (d.mem.alloc(&d.X, rows, "knn X") ||
      (dtype == GS_MIXED && d.mem.alloc(&d.XL, rows, "knn XL")) ||
      d.mem.alloc(&d.LR, lists * esz, "knn LR") ||
      d.mem.alloc(&d.LI, lists * sizeof(int32_t), "knn LI") ||
      d.mem.alloc(&d.R, (size_t)n * k * sizeof(double), "knn R") ||
      d.mem.alloc(&d.I, (size_t)n * k * sizeof(int32_t), "knn I"))
    return -1;
  if (dtype == GS_FP64) {
    knn_rows<double>(pos, n, a.n_pad, false, Hd, Ld);
    GS_KNN_HIP(hipMemcpyAsync(d.X, Hd.data(), rows, hipMemcpyHostToDevice, d.s));
  } else {
    knn_rows<float>(pos, n, a.n_pad, dtype == GS_MIXED, Hf, Lf);
    GS_KNN_HIP(hipMemcpyAsync(d.X, Hf.data(), rows, hipMemcpyHostToDevice, d.s));
    if (dtype == GS_MIXED)
      GS_KNN_HIP(hipMemcpyAsync(d.XL, Lf.data(), rows, hipMemcpyHostToDevice, d.s));
  }
  a.X = d.X; a.XL = d.XL; a.LR = d.LR; a.LI = (int32_t*)d.LI;
  a.R = (double*)d.R; a.I = (int32_t*)d.I;
  for (int32_t r = 0; r < reps; ++r) {
    GS_KNN_HIP(hipEventRecord(d.e0, d.s));
    knn_launch(a, dtype, ipl, d.s);
    GS_KNN_HIP(hipGetLastError());
    GS_KNN_HIP(hipEventRecord(d.e1, d.s));
    GS_KNN_HIP(hipEventSynchronize(d.e1));
    if (ms) {
      float t = 0;
      GS_KNN_HIP(hipEventElapsedTime(&t, d.e0, d.e1));
      ms[r] = (double)t;
    }
  }
  if (r2)
    GS_KNN_HIP(hipMemcpyAsync(r2, d.R, (size_t)n * k * sizeof(double), hipMemcpyDeviceToHost,
                              d.s));
  if (idx)
    GS_KNN_HIP(hipMemcpyAsync(idx, d.I, (size_t)n * k * sizeof(int32_t), hipMemcpyDeviceToHost,
                              d.s));
  GS_KNN_HIP(hipStreamSynchronize(d.s));
  if (info) {
    info[0] = a.n_pad; info[1] = ipl; info[2] = a.groups; info[3] = a.chunk;
  }
  return 0;
}

}  // namespace gs

extern "C" {

int32_t gs_knn_ipl_ok(int32_t dtype, int32_t ipl) {
  return (dtype == GS_FP32 || dtype == GS_FP64 || dtype == GS_MIXED) && ipl >= 0 && ipl <= 2;
}

int gs_hip_knn(const double* pos, int64_t n, int32_t dtype, int32_t k, int32_t ipl,
               int32_t groups, int32_t device, double* r2, int32_t* idx) {
  if (!r2 || !idx) {
    gs_set_error("gs_hip_knn: null argument");
    return -1;
  }
  return gs::knn_run(pos, n, dtype, k, ipl, groups, device, 1, nullptr, r2, idx, nullptr);
}

int gs_hip_knn_time(const double* pos, int64_t n, int32_t dtype, int32_t k, int32_t ipl,
                    int32_t groups, int32_t device, int32_t reps, double* ms, int64_t* info4) {
  if (!ms) {
    gs_set_error("gs_hip_knn_time: null argument");
    return -1;
  }
  return gs::knn_run(pos, n, dtype, k, ipl, groups, device, reps, ms, nullptr, nullptr, info4);
}

int32_t gs_knn_early_out(void) { return GS_KNN_EARLY; }

}  // extern "C"
