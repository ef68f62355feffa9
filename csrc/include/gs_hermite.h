// Internal interface between the Hermite kernels (nbody_hermite.hip) and their runtime
// (hermite.hip). Not part of the C API (gravsim.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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
};

// What the reduce kernel does with the summed derivatives.
enum { HM_STEP = 0,   // corrector: x, v, a, j <- corrected; per-workgroup min of dt_i
       HM_INIT = 1,   // a, j <- sums; per-workgroup min of (eta / 2) |a| / |j|
       HM_OUT = 2 };  // write (ax, ay, az, phi) and (jx, jy, jz, 0) to a_out / j_out

// Arrays hold 4 components per body over n_pad rows: X = (x, y, z, mu), V = (vx, vy, vz, 0),
// A = (ax, ay, az, phi), J = (jx, jy, jz, 0); XP / VP the predicted state (what the evaluate
// kernel reads); PA / PJ the per-chunk partial sums [n_chunks][n_pad].
template <typename T>
struct HArgs {
  T *X, *V, *A, *J;
  T *XP, *VP;
  T *PA, *PJ;
  T *a_out, *j_out;
  HermiteCtrl* ctrl;
  double* wgmin;     // [n_pad / 256] per-workgroup dt minima of the last reduce
  int64_t n_real, n_pad, chunk;
  int32_t n_chunks;
  int32_t mode;      // HM_*
  int32_t phi;       // evaluate: accumulate the potential sum too
  T cut2, eps2;
};

template <typename T>
hipError_t launch_hermite_ctrl(const HArgs<T>& a, hipStream_t s);
template <typename T>
hipError_t launch_hermite_predict(const HArgs<T>& a, hipStream_t s);
// Evaluate acc, jerk (and phi) of every body at (XP, VP) into PA / PJ: grid (n_pad / (256 ipl),
// groups); always (ctrl == nullptr) or only while ctrl->active.
template <typename T>
hipError_t launch_hermite_eval(const HArgs<T>& a, int ipl, int groups, bool gated, hipStream_t s);
template <typename T>
hipError_t launch_hermite_reduce(const HArgs<T>& a, hipStream_t s);
// ipl values the evaluate kernel is compiled for (fp32: 1, 2, 4; fp64: 1, 2).
bool hermite_ipl_ok(int fp64, int ipl);

}  // namespace gs
