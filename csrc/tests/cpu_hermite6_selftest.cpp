// Host-side self-test of the 6th-order Hermite functions of the native CPU engine
// (gs_cpu_accjerksnap_*, gs_cpu_hermite6_step_* in csrc/cpu/cpu_engine.cpp), a program of its own
// in the style of cpu_hermite_selftest.cpp, meant to be built with -fsanitize=address,undefined:
//   g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -Icsrc/include \
//       csrc/tests/cpu_hermite6_selftest.cpp csrc/cpu/cpu_engine.cpp csrc/common/layout.cpp
// Exit code 0 = pass.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "gravsim.h"

static int fails = 0;
#define EXPECT(c, ...)                        \
  do {                                        \
    if (!(c)) {                               \
      fprintf(stderr, "FAIL %s:%d ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);           \
      fprintf(stderr, "\n");                  \
      ++fails;                                \
    }                                         \
  } while (0)

static const int32_t kChunk = 1024;
static const double kEps2 = 1e14, kCut2 = 1e-20;

// The definition, pair by pair in plain j order: A_ij = mu d / r^3, J_ij = mu w / r^3 - 3 alpha
// A_ij, S_ij = mu q / r^3 - 6 alpha J_ij - 3 beta A_ij, with the sum of |term| per component of
// the snap as the scale its rounding is judged against.
static void naive_snap(const std::vector<double>& X, const std::vector<double>& V,
                       const std::vector<double>& B, int64_t n, std::vector<double>& S,
                       std::vector<double>& scale) {
  for (int64_t i = 0; i < n; ++i) {
    double s[3] = {0, 0, 0}, sc[3] = {0, 0, 0};
    for (int64_t j = 0; j < n; ++j) {
      double d[3], w[3], q[3], r2 = kEps2, dw = 0, ww = 0, dq = 0;
      for (int c = 0; c < 3; ++c) {
        d[c] = X[4 * j + c] - X[4 * i + c];
        w[c] = V[4 * j + c] - V[4 * i + c];
        q[c] = B[4 * j + c] - B[4 * i + c];
        r2 += d[c] * d[c];
        dw += d[c] * w[c];
        ww += w[c] * w[c];
        dq += d[c] * q[c];
      }
      if (r2 < kCut2) continue;
      const double r3 = r2 * sqrt(r2), mu = X[4 * j + 3];
      const double al = dw / r2, be = (ww + dq) / r2 + al * al;
      for (int c = 0; c < 3; ++c) {
        const double Ac = mu * d[c] / r3, Jc = mu * w[c] / r3 - 3.0 * al * Ac;
        const double t[3] = {mu * q[c] / r3, -6.0 * al * Jc, -3.0 * be * Ac};
        s[c] += t[0] + t[1] + t[2];
        sc[c] += fabs(t[0]) + fabs(t[1]) + fabs(t[2]);
      }
    }
    for (int c = 0; c < 3; ++c) {
      S[4 * i + c] = s[c];
      scale[4 * i + c] = sc[c];
    }
  }
}

template <typename T>
static bool same(const std::vector<T>& a, size_t ao, const std::vector<T>& b, size_t bo, size_t n) {
  return memcmp(a.data() + ao, b.data() + bo, n * sizeof(T)) == 0;
}

template <typename T>
static bool finite(const std::vector<T>& a) {
  for (T v : a)
    if (!isfinite(v)) return false;
  return true;
}

// One precision: all rows against the 4th-order entry (a, j bit-equal) and the naive snap, a
// sub-range, the refusals, and two steps with each step rule.
template <typename T, typename Snap, typename AccJerk, typename Step>
static void check(const char* name, const std::vector<double>& Xd, const std::vector<double>& Vd,
                  int64_t n, Snap snap, AccJerk accjerk, Step step, double eps) {
  const T cut2 = (T)kCut2, eps2 = (T)kEps2;
  const std::vector<T> X(Xd.begin(), Xd.end()), V(Vd.begin(), Vd.end());
  std::vector<T> A(4 * n), J(4 * n), S(4 * n), A4(4 * n), J4(4 * n), Z(4 * n, T(0));
  EXPECT(accjerk(X.data(), V.data(), n, 0, n, kChunk, cut2, eps2, A4.data(), J4.data()) == 0,
         "%s accjerk", name);
  std::vector<T> B = A4;  // the acceleration the snap is taken at (its phi column is not read)
  EXPECT(snap(X.data(), V.data(), B.data(), n, 0, n, kChunk, cut2, eps2, A.data(), J.data(),
              S.data()) == 0, "%s", name);
  EXPECT(finite(A) && finite(J) && finite(S), "%s: not finite at n = %lld", name, (long long)n);
  EXPECT(same(A, 0, A4, 0, 4 * n) && same(J, 0, J4, 0, 4 * n),
         "%s: a, j differ from the 4th-order entry at n = %lld", name, (long long)n);
  // the snap against the definition on the same (rounded) inputs
  std::vector<double> Xr(X.begin(), X.end()), Vr(V.begin(), V.end()), Br(B.begin(), B.end());
  std::vector<double> Sref(4 * n, 0.0), scale(4 * n, 0.0);
  naive_snap(Xr, Vr, Br, n, Sref, scale);
  double worst = 0.0;
  for (int64_t i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c)
      if (scale[4 * i + c] > 0.0) {
        const double r = fabs((double)S[4 * i + c] - Sref[4 * i + c]) / (eps * scale[4 * i + c]);
        if (r > worst) worst = r;
      } else {
        EXPECT(S[4 * i + c] == T(0), "%s: snap without a term is not zero", name);
      }
  EXPECT(worst < 64.0, "%s: snap off the definition by %g eps x scale at n = %lld", name, worst,
         (long long)n);
  // a sub-range returns the same rows
  const int64_t i0 = n > 1 ? n / 3 + 1 : 0, i1 = n > 1 ? n - n / 5 : 1, m = i1 - i0;
  std::vector<T> a(4 * m), j(4 * m), s(4 * m);
  EXPECT(snap(X.data(), V.data(), B.data(), n, i0, i1, kChunk, cut2, eps2, a.data(), j.data(),
              s.data()) == 0, "%s range", name);
  EXPECT(same(a, 0, A, 4 * i0, 4 * m) && same(j, 0, J, 4 * i0, 4 * m) &&
             same(s, 0, S, 4 * i0, 4 * m), "%s: rows [%lld, %lld)", name, (long long)i0,
         (long long)i1);
  // refusals
  EXPECT(snap(X.data(), V.data(), B.data(), n, 0, n + 1, kChunk, cut2, eps2, a.data(), j.data(),
              s.data()) != 0, "%s: i1 > n accepted", name);
  EXPECT(snap(X.data(), V.data(), B.data(), n, -1, 0, kChunk, cut2, eps2, a.data(), j.data(),
              s.data()) != 0, "%s: i0 < 0 accepted", name);
  EXPECT(snap(X.data(), V.data(), B.data(), n, 1, 0, kChunk, cut2, eps2, a.data(), j.data(),
              s.data()) != 0, "%s: i1 < i0 accepted", name);
  EXPECT(snap(X.data(), V.data(), B.data(), n, 0, n, 0, cut2, eps2, a.data(), j.data(),
              s.data()) != 0, "%s: chunk 0 accepted", name);
  EXPECT(snap(X.data(), V.data(), nullptr, n, 0, n, kChunk, cut2, eps2, a.data(), j.data(),
              s.data()) != 0, "%s: null acceleration rows accepted", name);
  EXPECT(snap(X.data(), V.data(), B.data(), n, 0, n, kChunk, cut2, eps2, a.data(), j.data(),
              nullptr) != 0, "%s: null snap output accepted", name);
  // two steps of one hour, fixed and with the step criterion on
  for (double eta : {0.0, 0.25}) {
    std::vector<T> x = X, v = V, ac = A, jk = J, sn = S, cr = Z, scratch(24 * n);
    for (int64_t i = 0; i < n; ++i) ac[4 * i + 3] = 0;
    for (int k = 0; k < 2; ++k) {
      double dt = -1.0;
      EXPECT(step(x.data(), v.data(), ac.data(), jk.data(), sn.data(), cr.data(), scratch.data(),
                  n, kChunk, 3600.0, cut2, eps2, eta, &dt) == 0, "%s step", name);
      EXPECT(eta > 0.0 && n > 1 ? (dt > 0.0 && isfinite(dt)) : isinf(dt), "%s: dt_min %g", name,
             dt);
    }
    EXPECT(finite(x) && finite(v) && finite(ac) && finite(jk) && finite(sn) && finite(cr),
           "%s: step not finite", name);
    EXPECT(n == 1 || !same(x, 0, X, 0, 4 * n), "%s: the step moved nothing", name);
    EXPECT(step(x.data(), v.data(), ac.data(), jk.data(), sn.data(), cr.data(), nullptr, n, kChunk,
                3600.0, cut2, eps2, eta, nullptr) != 0, "%s: null scratch accepted", name);
    EXPECT(step(x.data(), v.data(), ac.data(), jk.data(), nullptr, cr.data(), scratch.data(), n,
                kChunk, 3600.0, cut2, eps2, eta, nullptr) != 0, "%s: null snap accepted", name);
    EXPECT(step(x.data(), v.data(), ac.data(), jk.data(), sn.data(), cr.data(), scratch.data(), n,
                kChunk, 0.0, cut2, eps2, eta, nullptr) != 0, "%s: h = 0 accepted", name);
  }
}

int main() {
  for (int64_t n : {1, 2, 3, 1024, 1031, 2055}) {
    std::vector<double> pos(3 * n), vel(3 * n), mass(n), X(4 * n), V(4 * n, 0.0);
    gs_ic_fill_host(GS_IC_SOLAR_RANDOM, 7, n, 0, n, pos.data(), vel.data(), mass.data());
    for (int64_t i = 0; i < n; ++i) {
      for (int d = 0; d < 3; ++d) {
        X[4 * i + d] = pos[3 * i + d];
        V[4 * i + d] = vel[3 * i + d];
      }
      X[4 * i + 3] = 6.674e-11 * mass[i];
    }
    check<double>("f64", X, V, n, gs_cpu_accjerksnap_f64, gs_cpu_accjerk_f64,
                  gs_cpu_hermite6_step_f64, 2.220446049250313e-16);
    check<float>("f32", X, V, n, gs_cpu_accjerksnap_f32, gs_cpu_accjerk_f32,
                 gs_cpu_hermite6_step_f32, 1.1920928955078125e-07);
  }
  if (fails) {
    fprintf(stderr, "%d failures\n", fails);
    return 1;
  }
  printf("cpu_hermite6_selftest ok\n");
  return 0;
}
