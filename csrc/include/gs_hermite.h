// Internal interface between the Hermite kernels (nbody_hermite.hip, nbody_hermite6.hip) and
// their runtime (hermite.hip). The schemes' arithmetic is in gs_hermite_scheme.h. Not part of
// the C API (gravsim.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gs_common.h"

namespace gs {

// Device control block of a Hermite run: the step chain reads and advances it on the device,
// so the host never waits for a step to learn the next step size.
struct HermiteCtrl {
  double t;        // time reached
  double h;        // size of the step the chain is taking (set by the control kernel)
  double dt_last;  // size of the last step taken
  double dt_min;   // smallest criterion-chosen step so far (steps cut short by t_end excluded)
  double dt_max;   // configured dt: fixed step, or the adaptive ceiling
  double eta;      // Aarseth accuracy parameter (0: fixed step)
  double t_end;    // end time (has_end)
  unsigned long long steps;  // steps taken (no-op launches past t_end are not counted)
  int32_t has_end;
  int32_t active;  // 1 while the chain of the current launch takes a step, 0 once t >= t_end
  // collisions (gs_hermite_set_collisions; both 0 otherwise)
  unsigned long long overlaps;  // bodies seen with q < eps2 by the reduces so far
  int32_t ov_stop;              // 1: the chain takes no further step once overlaps != 0
  int32_t pad_;
};

// Control block of a block-step run (individual steps dt_max 2^-k): time is a count of ticks of
// dt_max 2^-L. The chain's kernels read it on the device and return at once when there is
// nothing for them to do (the target time is reached, or the step takes the other evaluate path).
struct HermiteBlockCtrl {
  int64_t t_ticks;   // time reached
  int64_t target;    // the chain stops here (a multiple of 2^L: a macro step boundary)
  double dt_max, eta;
  unsigned long long block_steps, body_steps, level_clamped;
  int32_t L;           // max_level
  int32_t level_max;   // deepest level any body has had
  int32_t n_act;       // size of the active list of the current block step
  int32_t narrow_max;  // n_act <= narrow_max: narrow path
  int32_t path;        // HP_* of the current block step
  int32_t active;      // 1 while the current chain takes a block step
  unsigned long long overlaps;  // collisions: active bodies corrected with q < eps2 so far
};
enum { HP_NARROW = 1, HP_WIDE = 2 };

// Per-body block-step state and the work arrays of one block step.
struct HBlock {
  HermiteBlockCtrl* bc;
  int64_t* tb;       // [n_pad] body time (ticks), a multiple of the body's step 2^(L - level)
  int32_t* level;    // [n_pad]
  int32_t* list;     // [n_pad] active bodies, ascending
  int32_t* wgcount;  // [n_pad / 256] active bodies per workgroup of the predict kernel
  int64_t* wgnext;   // [n_pad / 256] per-workgroup min of tb + step
  void *NA, *NJ;     // narrow partials [n_slices][cap] rows of 4 (of the pair type)
  int32_t slice;     // j rows per slice (a multiple of 256; depends on n_pad only)
  int32_t n_slices;
  int32_t cap;       // slots of the narrow partial buffer (= narrow_max)
};

constexpr int kNarrowGroup = 4;  // active bodies a narrow workgroup carries per pass
// ... and of order 6 (nbody_hermite6.hip), whose bodies hold 10 fp64 sums and 9 fp64 row values
// each: the most that leaves the kernel without scratch (docs/DESIGN.md section 23).
constexpr int kNarrowGroup6 = 2;

#ifdef __HIPCC__
// The arithmetic every block-step kernel of both orders shares.
// Seconds of a span of ticks: dt_max ticks 2^-L in fp64 (the run's dtype takes a cast of it).
__device__ __forceinline__ double ticks_seconds(double dt_max, int64_t ticks, int L) {
  return dt_max * ldexp((double)ticks, -L);
}

__device__ __forceinline__ bool body_due(const HBlock& b, int64_t i, int L, int64_t t_next) {
  return b.tb[i] + ((int64_t)1 << (L - b.level[i])) == t_next;
}

// The level of an active body after its step to t_next from level k, where its criterion gave
// `want` (rated): any number of halvings (capped at L, a clamp is counted), at most one doubling
// and only where t_next allows the doubled step. Records the deepest level.
__device__ __forceinline__ int block_new_level(HermiteBlockCtrl* bc, int k, bool rated,
                                               double want, int64_t t_next, int L,
                                               double dt_max) {
  if (rated) {
    const double dtk = ldexp(dt_max, -k);
    if (want < dtk) {
      while (k < L && ldexp(dt_max, -k) > want) ++k;
      if (ldexp(dt_max, -k) > want) atomicAdd(&bc->level_clamped, 1ull);
    } else if (k > 0 && want >= 2.0 * dtk &&
               (t_next & (((int64_t)1 << (L - k + 1)) - 1)) == 0) {
      --k;
    }
  }
  if (k > bc->level_max) atomicMax(&bc->level_max, k);
  return k;
}
#endif

// What the reduce kernel does with the summed derivatives.
enum { HM_STEP = 0,   // corrector: x, v, a, j <- corrected; per-workgroup min of dt_i
       HM_INIT = 1,   // a, j <- sums; per-workgroup min of (eta / 2) |a| / |j|
       HM_OUT = 2 };  // write (ax, ay, az, phi) and (jx, jy, jz, 0) to a_out / j_out

// Arrays hold 4 components per body over n_pad rows: X = (x, y, z, mu), V = (vx, vy, vz, 0),
// A = (ax, ay, az, phi), J = (jx, jy, jz, 0); XP / VP the predicted state (what the evaluate
// kernel reads); PA / PJ the per-chunk partial sums [n_chunks][n_pad].
// T is the type of the pair arithmetic, S the type of the state. Mixed precision is
// HArgs<float, double>: x, v, a, j and the reduce, corrector and criterion in fp64, the predicted
// position handed to the evaluate kernels as double-single rows XP = (float(xp), mu) and
// XL = (float(xp - double(float(xp))), 0), so that d = (XP_j - XP_i) + (XL_j - XL_i) in fp32 is
// free of the common part; VP and the partials are fp32 rows. XL is null where S is T.
template <typename T, typename S = T>
struct HArgs {
  S *X, *V, *A, *J;
  T *XP, *VP;
  T *PA, *PJ;
  S *a_out, *j_out;
  HermiteCtrl* ctrl;
  double* wgmin;     // [n_pad / 256] per-workgroup dt minima of the last reduce
  int64_t n_real, n_pad, chunk;
  int32_t n_chunks;
  int32_t mode;      // HM_*
  int32_t phi;       // evaluate: accumulate the potential sum too
  T cut2, eps2;
  HBlock blk;        // block-step mode (all null otherwise)
  T* XL;             // mixed precision: lo rows of the predicted position (last: the fields
                     // above keep the offsets the fp32 and fp64 kernels were tuned with)
  // Collisions (nn != 0; all null otherwise; after XL for the same reason, and the narrow
  // path's NNI here and not in HBlock, which sits before XL). Pair measure of bodies i, j:
  // q = r^2 - (R_i + R_j)^2 with the kernel's own r^2; the nearest neighbour of i is the real
  // j != i of the smallest q, the lowest j on an exact tie, (+inf, -1) when there is none.
  S* R;              // [n_pad] radius (ghost rows 0); rides in the VP row's spare component
  int32_t* PN;       // [n_chunks][n_pad] j of the chunk partial whose q is PJ[c][i].w
  int32_t* NNI;      // [n_slices][cap] the same beside NJ (narrow path)
  double* nn_q;      // [n_pad] latest q of each body, and
  int32_t* nn_i;     //         its neighbour
  double* ca_q;      // [n_pad] closest approach since the last clear: min of q over the body's
  int32_t* ca_i;     //         evaluations, and the neighbour then
  double* q_out;     // HM_OUT: q and neighbour per row of a_out / j_out
  int32_t* nn_out;
  int32_t nn;
  // A rank's slice of a multi-rank run (last, as above): the rank predicts, evaluates and
  // corrects rows row0 + [0, n_loc) (whole units of 1024 rows) against all j; PA / PJ are then
  // [n_chunks][n_loc], indexed by local row; every other array keeps its full length and the
  // runtime gathers the slices. One rank: row0 = 0, n_loc = n_pad, and the kernels are the
  // Rows::All forms.
  int64_t row0, n_loc;
};

template <typename T, typename S>
hipError_t launch_hermite_ctrl(const HArgs<T, S>& a, hipStream_t s);
template <typename T, typename S>
hipError_t launch_hermite_predict(const HArgs<T, S>& a, hipStream_t s);
// Evaluate acc, jerk (and phi) of every body at (XP, VP) into PA / PJ: grid (n_pad / (256 ipl),
// groups); always (ctrl == nullptr) or only while ctrl->active.
template <typename T, typename S>
hipError_t launch_hermite_eval(const HArgs<T, S>& a, int ipl, int groups, bool gated,
                               hipStream_t s);
template <typename T, typename S>
hipError_t launch_hermite_reduce(const HArgs<T, S>& a, hipStream_t s);
// Collisions on: XP, VP (XL) <- the current X, V with the radii, in any precision (what
// launch_hermite_split does for mixed runs without them).
template <typename T, typename S>
hipError_t launch_hermite_stage(const HArgs<T, S>& a, hipStream_t s);
// Block-step chain (hermite.hip enqueues them in this order, all on one stream):
// next-time minima, control, predict-all + mark, compact, narrow evaluate, wide (gathered)
// evaluate, reduce + correct + new level. mode of the last: HM_STEP or HM_OUT.
template <typename T, typename S>
hipError_t launch_block_next(const HArgs<T, S>& a, hipStream_t s);
template <typename T, typename S>
hipError_t launch_block_predict(const HArgs<T, S>& a, hipStream_t s);
// The compaction alone (launch_block_predict ends with it): it reads blk and n_real only, so the
// order-6 chain runs it after its own predict-all + mark.
template <typename T, typename S>
hipError_t launch_block_compact(const HArgs<T, S>& a, hipStream_t s);
template <typename T, typename S>
hipError_t launch_block_narrow(const HArgs<T, S>& a, hipStream_t s);
template <typename T, typename S>
hipError_t launch_block_wide(const HArgs<T, S>& a, int ipl, int groups, hipStream_t s);
template <typename T, typename S>
hipError_t launch_block_correct(const HArgs<T, S>& a, hipStream_t s);
// Levels and times of a run that starts from the carried a, j at tick t0.
template <typename T, typename S>
hipError_t launch_block_init(const HArgs<T, S>& a, int64_t t0, hipStream_t s);
// j rows per narrow slice for n_pad bodies.
int32_t hermite_narrow_slice(int64_t n_pad);
// Mixed precision: XP, XL, VP <- the split of the current X, V (the predictor's output at h = 0),
// for an evaluation of the derivatives of the current state.
hipError_t launch_hermite_split(const HArgs<float, double>& a, hipStream_t s);
// ipl values the evaluate kernel is compiled for (fp32 pairs: 1, 2, 4; fp64: 1, 2).
bool hermite_ipl_ok(int fp64, int ipl);

// ---- 6th order (nbody_hermite6.hip) ---------------------------------------------------------
// Arrays hold 4 components per body over n_pad rows (ghost rows zero), all of the run's one
// type T (order 6 has no mixed precision): X = (x, y, z, mu), V, A, J, S, C the state; XP, VP,
// AP = (ap, 0) the predicted rows the evaluate kernel reads; PA = (a, sum mu / r), PJ, PS the
// per-chunk partial sums [n_chunks][n_pad]. mode is HM_*: HM_STEP corrects and forms c1 and the
// per-workgroup dt minima, HM_INIT stores a, j, s (c <- 0) and the minima of the first step,
// HM_OUT writes (a, phi), j, s to the outputs. The control kernel is the 4th-order chain's.
template <typename T>
struct H6Args {
  T *X, *V, *A, *J, *S, *C;
  T *XP, *VP, *AP;
  T *PA, *PJ, *PS;
  T *a_out, *j_out, *s_out;
  HermiteCtrl* ctrl;
  double* wgmin;  // [n_pad / 256]
  int64_t n_real, n_pad, chunk;
  int32_t n_chunks;
  int32_t mode;
  int32_t phi;
  T cut2, eps2;
  // Block steps (fp64; all null otherwise; last: the fields above keep their offsets). The
  // narrow partials are blk.NA, blk.NJ and NS, [n_slices][cap] rows of 4 each.
  HBlock blk;
  T* NS;
};

// ipl values the order-6 evaluate kernel is compiled for (fp32: 1, 2; fp64: 1).
bool hermite6_ipl_ok(int fp64, int ipl);
template <typename T>
hipError_t launch_hermite6_predict(const H6Args<T>& a, hipStream_t s);
// a, j, s (and phi) of every body at (XP, VP, AP) into PA / PJ / PS: grid (n_pad / (256 ipl),
// groups); always, or (gated) only while ctrl->active.
template <typename T>
hipError_t launch_hermite6_eval(const H6Args<T>& a, int ipl, int groups, bool gated,
                                hipStream_t s);
template <typename T>
hipError_t launch_hermite6_reduce(const H6Args<T>& a, hipStream_t s);
// Order-6 block-step chain (fp64 only): the overloads of launch_block_next, _predict (predict-all
// + mark, then the compaction), _narrow, _wide and _correct (mode HM_STEP or HM_OUT) for H6Args,
// enqueued as order 4's are. The next-time minima, the control, the compaction and the start are
// order 4's kernels on base_view(a); the predict-all, the narrow and the wide evaluate and the
// correct kernel are the order's own.
template <typename T>
hipError_t launch_block_next(const H6Args<T>& a, hipStream_t s);
template <typename T>
hipError_t launch_block_predict(const H6Args<T>& a, hipStream_t s);
template <typename T>
hipError_t launch_block_narrow(const H6Args<T>& a, hipStream_t s);
template <typename T>
hipError_t launch_block_wide(const H6Args<T>& a, int ipl, int groups, hipStream_t s);
template <typename T>
hipError_t launch_block_correct(const H6Args<T>& a, hipStream_t s);

// What order 4's kernels read of an order-6 run: the control (ctrl, wgmin, n_pad) and the block
// state (blk, n_real, n_pad).
template <typename T>
HArgs<T, T> base_view(const H6Args<T>& a) {
  HArgs<T, T> c{};
  c.ctrl = a.ctrl;
  c.wgmin = a.wgmin;
  c.blk = a.blk;
  c.n_real = a.n_real;
  c.n_pad = a.n_pad;
  return c;
}

#ifdef __HIPCC__
// Launch helpers of both kernel files: workgroups of kForceBlock threads.
template <typename... P, typename... A>
hipError_t hlaunch(void (*kernel)(P...), dim3 grid, hipStream_t s, const A&... args) {
  hipLaunchKernelGGL(kernel, grid, dim3(kForceBlock), 0, s, args...);
  return hipGetLastError();
}

// Workgroups of one thread per row.
inline dim3 row_grid(int64_t rows) { return dim3((unsigned)(rows / kForceBlock)); }

inline int clamp_groups(int groups, int n_chunks) {
  return groups < 1 ? 1 : groups > n_chunks ? n_chunks : groups;
}
#endif

}  // namespace gs
