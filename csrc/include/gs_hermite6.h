// 6th-order Hermite scheme (Nitadori & Makino 2008): the arithmetic the CPU engine
// (cpu_engine.cpp) and the GPU kernels (nbody_hermite6.hip) share, and (HIP only) the interface
// between those kernels and their runtime (hermite.hip). Not part of the C API (gravsim.h).
//
// State per body: x, v, a, j, s (snap, a'') and c (crackle, a'''). One step of size h:
//   predict   xp = x + v h + a h^2/2 + j h^3/6 + s h^4/24 + c h^5/120
//             vp = v + a h + j h^2/2 + s h^3/6 + c h^4/24
//             ap = a + j h + s h^2/2 + c h^3/6
//   evaluate  a1, j1, s1 at (xp, vp, ap): one pass over the pairs
//   correct   v1 = v + (h/2)(a + a1) - (h^2/10)(j1 - j) + (h^3/120)(s + s1)
//             x1 = x + (h/2)(v + v1) - (h^2/10)(a1 - a) + (h^3/120)(j + j1)
//   derive    c1 and, for the step criterion, a'''' and a''''' at t1 from the quintic through
//             (a, j, s) at t0 and (a1, j1, s1) at t1.
#pragma once
#include <math.h>
#include <stdint.h>

#include "gs_common.h"

namespace gs {

// Taylor coefficients of the predictor over h, in the state type.
template <typename S>
struct H6Taylor {
  S h, h2, h3, h4, h5;  // h, h^2/2, h^3/6, h^4/24, h^5/120
};
template <typename S>
GS_HD H6Taylor<S> h6_taylor(S h) {
  H6Taylor<S> t;
  t.h = h;
  t.h2 = (h * h) / S(2);
  t.h3 = (h * h * h) / S(6);
  t.h4 = (h * h * h * h) / S(24);
  t.h5 = (h * h * h * h * h) / S(120);
  return t;
}

// One component of the predictor.
template <typename S>
GS_HD void h6_predict(const H6Taylor<S>& t, S x, S v, S a, S j, S s, S c, S& xp, S& vp, S& ap) {
  xp = x + (v * t.h + (a * t.h2 + (j * t.h3 + (s * t.h4 + c * t.h5))));
  vp = v + (a * t.h + (j * t.h2 + (s * t.h3 + c * t.h4)));
  ap = a + (j * t.h + (s * t.h2 + c * t.h3));
}

// One component of the corrector.
template <typename S>
GS_HD void h6_correct(S h, S x, S v, S a0, S j0, S s0, S a1, S j1, S s1, S& x1, S& v1) {
  const S hh = h / S(2), h10 = (h * h) / S(10), h120 = (h * h * h) / S(120);
  v1 = v + ((a0 + a1) * hh + ((j0 - j1) * h10 + (s0 + s1) * h120));
  x1 = x + ((v + v1) * hh + ((a0 - a1) * h10 + (j0 + j1) * h120));
}

// One component of the 3rd, 4th and 5th derivatives of a at t1 (c1, p1, a5; the 5th is constant
// over the step), in fp64 whatever the state type.
GS_HD void h6_high(double h, double a0, double j0, double s0, double a1, double j1, double s1,
                   double& c1, double& p1, double& a5) {
  const double hp = 0.5 * h, hp2 = hp * hp;
  const double Am = a1 - a0, Jm = hp * (j1 - j0), Jp = hp * (j1 + j0);
  const double Sm = hp2 * (s1 - s0), Sp = hp2 * (s1 + s0);
  const double ih = 1.0 / hp, ih3 = ih * ih * ih, ih4 = ih3 * ih, ih5 = ih4 * ih;
  const double a3 = (6.0 * ih3) * (-5.0 * Am + 5.0 * Jp - Sm) / 8.0;
  const double a4 = (24.0 * ih4) * (-Jm + Sp) / 16.0;
  a5 = (120.0 * ih5) * (3.0 * Am - 3.0 * Jp + Sm) / 16.0;
  c1 = a3 + hp * a4 + hp2 * a5 / 2.0;
  p1 = a4 + hp * a5;
}

GS_HD double h6_norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

// The step a body asks for after a step (Nitadori & Makino's criterion, eta linear):
// eta ((|a1||s1| + |j1|^2) / (|c1||a5| + |p1|^2))^(1/6). False where the ratio is zero or not
// finite: the body takes no part in the minimum.
GS_HD bool h6_dt(double eta, const double a1[3], const double j1[3], const double s1[3],
                 const double c1[3], const double p1[3], const double a5[3], double& dt) {
  const double an = h6_norm3(a1[0], a1[1], a1[2]), jn = h6_norm3(j1[0], j1[1], j1[2]);
  const double sn = h6_norm3(s1[0], s1[1], s1[2]), cn = h6_norm3(c1[0], c1[1], c1[2]);
  const double pn = h6_norm3(p1[0], p1[1], p1[2]), qn = h6_norm3(a5[0], a5[1], a5[2]);
  const double ratio = (an * sn + jn * jn) / (cn * qn + pn * pn);
  dt = eta * pow(ratio, 1.0 / 6.0);
  return ratio > 0.0 && isfinite(dt);
}

}  // namespace gs

#if defined(__HIPCC__)
#include "gs_hermite.h"

namespace gs {

// Arrays hold 4 components per body over n_pad rows (ghost rows zero), all of the run's one
// type T (order 6 has no mixed precision): X = (x, y, z, mu), V, A, J, S, C the state; XP, VP,
// AP = (ap, 0) the predicted rows the evaluate kernel reads; PA = (a, sum mu / r), PJ, PS the
// per-chunk partial sums [n_chunks][n_pad]. mode is HM_* of gs_hermite.h: HM_STEP corrects and
// forms c1 and the per-workgroup dt minima, HM_INIT stores a, j, s (c <- 0) and the minima of
// the first step, HM_OUT writes (a, phi), j, s to the outputs.
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

}  // namespace gs
#endif
