// The arithmetic of the Hermite schemes, once for host and device: the CPU engine
// (cpu_engine.cpp) and the GPU kernels (nbody_hermite.hip, nbody_hermite6.hip) call these, and
// both libraries are built with -ffp-contract=off, so the same expression tree gives the same
// bits. Nothing of HIP is included. Not part of the C API (gravsim.h).
//
// 4th order (Makino & Aarseth 1992). State per body: x, v, a, j. One step of size h:
//   predict   xp = x + v h + a h^2/2 + j h^3/6,  vp = v + a h + j h^2/2
//   evaluate  a1, j1 at (xp, vp): one pass over the pairs
//   correct   v1 = v + (h/2)(a + a1) + (h^2/12)(j - j1)
//             x1 = x + (h/2)(v + v1) + (h^2/12)(a - a1)
//   criterion Aarseth's, from the a'' and a''' that the two evaluations imply.
// 6th order (Nitadori & Makino 2008). State per body: x, v, a, j, s (snap, a'') and c (crackle,
// a'''). One step of size h:
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

GS_HD double norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

// The first step of a run, from the derivatives of the starting state (both orders):
// (eta / 2) |a| / |j|. False where |j| = 0 or the ratio is not finite: the body takes no part in
// the minimum.
GS_HD bool hermite_first_dt(double eta, const double a[3], const double j[3], double& dt) {
  const double an = norm3(a[0], a[1], a[2]), jn = norm3(j[0], j[1], j[2]);
  dt = 0.5 * eta * an / jn;
  return jn > 0.0 && isfinite(dt);
}

// ---- 4th order ------------------------------------------------------------------------------

// One component of the predictor; h2 = h^2/2 and h3 = h^3/6 in the state type.
template <typename S>
GS_HD void h4_predict(S h, S h2, S h3, S x, S v, S a, S j, S& xp, S& vp) {
  xp = x + (v * h + (a * h2 + j * h3));
  vp = v + (a * h + j * h2);
}

// One component of the corrector; hh = h/2 and h12 = h^2/12 in the state type.
template <typename S>
GS_HD void h4_correct(S hh, S h12, S x, S v, S a0, S j0, S a1, S j1, S& x1, S& v1) {
  v1 = v + ((a0 + a1) * hh + (j0 - j1) * h12);
  x1 = x + ((v + v1) * hh + (a0 - a1) * h12);
}

// The step a body asks for after a step of size hd: Aarseth's criterion from the 2nd and 3rd
// derivatives that the two evaluations (a0, j0 before the step, a1, j1 after it) imply, in fp64
// whatever the state type. False where |j1| = 0 or the ratio is not finite.
GS_HD bool h4_dt(double hd, double eta, const double a0[3], const double j0[3], const double a1[3],
                 const double j1[3], double& dt) {
  const double ih = 1.0 / hd, ih2 = ih * ih, ih3 = ih2 * ih;
  double s2[3], s3[3];
  for (int d = 0; d < 3; ++d) {
    const double da = a0[d] - a1[d];
    const double a2 = (-6.0 * da - hd * (4.0 * j0[d] + 2.0 * j1[d])) * ih2;
    s3[d] = (12.0 * da + 6.0 * hd * (j0[d] + j1[d])) * ih3;
    s2[d] = a2 + hd * s3[d];
  }
  const double an = norm3(a1[0], a1[1], a1[2]), jn = norm3(j1[0], j1[1], j1[2]);
  const double n2 = norm3(s2[0], s2[1], s2[2]), n3 = norm3(s3[0], s3[1], s3[2]);
  dt = sqrt(eta * (an * n2 + jn * jn) / (jn * n3 + n2 * n2));
  return jn > 0.0 && isfinite(dt);
}

// ---- 6th order ------------------------------------------------------------------------------

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

// The step a body asks for after a step (Nitadori & Makino's criterion, eta linear):
// eta ((|a1||s1| + |j1|^2) / (|c1||a5| + |p1|^2))^(1/6). False where the ratio is zero or not
// finite: the body takes no part in the minimum.
GS_HD bool h6_dt(double eta, const double a1[3], const double j1[3], const double s1[3],
                 const double c1[3], const double p1[3], const double a5[3], double& dt) {
  const double an = norm3(a1[0], a1[1], a1[2]), jn = norm3(j1[0], j1[1], j1[2]);
  const double sn = norm3(s1[0], s1[1], s1[2]), cn = norm3(c1[0], c1[1], c1[2]);
  const double pn = norm3(p1[0], p1[1], p1[2]), qn = norm3(a5[0], a5[1], a5[2]);
  const double ratio = (an * sn + jn * jn) / (cn * qn + pn * pn);
  dt = eta * pow(ratio, 1.0 / 6.0);
  return ratio > 0.0 && isfinite(dt);
}

}  // namespace gs
