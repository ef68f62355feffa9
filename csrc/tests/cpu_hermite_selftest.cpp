// Host-side self-test of the Hermite functions of the native CPU engine (gs_cpu_accjerk_*,
// gs_cpu_accjerk_idx_*, gs_cpu_hermite_step_* in csrc/cpu/cpu_engine.cpp), a program of its own
// in the style of cpu_nn_selftest.cpp, meant to be built with -fsanitize=address,undefined:
//   g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -Icsrc/include \
//       csrc/tests/cpu_hermite_selftest.cpp csrc/cpu/cpu_engine.cpp csrc/common/layout.cpp
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

// The engine's fp64 expression, body by body: chunk sums from zero, added in chunk order.
static void naive_accjerk(const std::vector<double>& X, const std::vector<double>& V, int64_t n,
                          std::vector<double>& A, std::vector<double>& J) {
  for (int64_t i = 0; i < n; ++i) {
    double t[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int64_t j0 = 0; j0 < n; j0 += kChunk) {
      double ax = 0, ay = 0, az = 0, ph = 0, jx = 0, jy = 0, jz = 0;
      for (int64_t j = j0; j < j0 + kChunk && j < n; ++j) {
        const double dx = X[4 * j] - X[4 * i], dy = X[4 * j + 1] - X[4 * i + 1],
                     dz = X[4 * j + 2] - X[4 * i + 2];
        const double wx = V[4 * j] - V[4 * i], wy = V[4 * j + 1] - V[4 * i + 1],
                     wz = V[4 * j + 2] - V[4 * i + 2];
        const double r2 = fma(dz, dz, fma(dy, dy, fma(dx, dx, kEps2)));
        const double inv = (r2 >= kCut2) ? 1.0 / sqrt(r2) : 0.0;
        const double inv2 = inv * inv;
        const double mi = X[4 * j + 3] * inv;
        const double s = mi * inv2;
        const double dw = fma(dz, wz, fma(dy, wy, dx * wx));
        const double al = dw * (3.0 * inv2);
        ax = fma(s, dx, ax);
        ay = fma(s, dy, ay);
        az = fma(s, dz, az);
        jx = fma(s, fma(-al, dx, wx), jx);
        jy = fma(s, fma(-al, dy, wy), jy);
        jz = fma(s, fma(-al, dz, wz), jz);
        ph += mi;
      }
      const double c[7] = {ax, ay, az, ph, jx, jy, jz};
      for (int d = 0; d < 7; ++d) t[d] += c[d];
    }
    const double a[4] = {t[0], t[1], t[2], -t[3]}, jk[4] = {t[4], t[5], t[6], 0.0};
    memcpy(&A[4 * i], a, sizeof(a));
    memcpy(&J[4 * i], jk, sizeof(jk));
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

// One precision: the range form over all rows and over [i0, i1), the list form on a permuted
// list with repeats and on an empty list, the refusals, and two steps with each step rule.
template <typename T, typename Range, typename List, typename Step>
static void check(const char* name, const std::vector<T>& X, const std::vector<T>& V, int64_t n,
                  Range range, List list, Step step, std::vector<T>& A, std::vector<T>& J) {
  const T cut2 = (T)kCut2, eps2 = (T)kEps2;
  EXPECT(range(X.data(), V.data(), n, 0, n, kChunk, cut2, eps2, A.data(), J.data()) == 0, "%s",
         name);
  EXPECT(finite(A) && finite(J), "%s: not finite at n = %lld", name, (long long)n);
  const int64_t i0 = n > 1 ? n / 3 + 1 : 0, i1 = n > 1 ? n - n / 5 : 1, m = i1 - i0;
  std::vector<T> a(4 * m), j(4 * m);
  EXPECT(range(X.data(), V.data(), n, i0, i1, kChunk, cut2, eps2, a.data(), j.data()) == 0,
         "%s range", name);
  EXPECT(same(a, 0, A, 4 * i0, 4 * m) && same(j, 0, J, 4 * i0, 4 * m), "%s: rows [%lld, %lld)",
         name, (long long)i0, (long long)i1);
  std::vector<int32_t> idx;
  for (int64_t k = 0; k < n; ++k) idx.push_back((int32_t)((k * 7 + 3) % n));  // (7 !| n)
  for (int64_t k = 0; k < n && k < 5; ++k) idx.push_back(idx[(size_t)k]);
  std::vector<T> al(4 * idx.size()), jl(4 * idx.size());
  EXPECT(list(X.data(), V.data(), n, idx.data(), (int64_t)idx.size(), kChunk, cut2, eps2,
              al.data(), jl.data()) == 0, "%s idx", name);
  for (size_t k = 0; k < idx.size(); ++k)
    EXPECT(same(al, 4 * k, A, 4 * (size_t)idx[k], 4) && same(jl, 4 * k, J, 4 * (size_t)idx[k], 4),
           "%s: list row %zu of n = %lld", name, k, (long long)n);
  EXPECT(list(X.data(), V.data(), n, idx.data(), 0, kChunk, cut2, eps2, nullptr, nullptr) == 0,
         "%s: empty list", name);
  EXPECT(list(X.data(), V.data(), n, nullptr, 0, kChunk, cut2, eps2, nullptr, nullptr) == 0,
         "%s: empty null list", name);
  // refusals
  int32_t bad = (int32_t)n;
  EXPECT(range(X.data(), V.data(), n, 0, n + 1, kChunk, cut2, eps2, a.data(), j.data()) != 0,
         "%s: i1 > n accepted", name);
  EXPECT(range(X.data(), V.data(), n, -1, 0, kChunk, cut2, eps2, a.data(), j.data()) != 0,
         "%s: i0 < 0 accepted", name);
  EXPECT(range(X.data(), V.data(), n, 1, 0, kChunk, cut2, eps2, a.data(), j.data()) != 0,
         "%s: i1 < i0 accepted", name);
  EXPECT(range(X.data(), V.data(), n, 0, n, 0, cut2, eps2, a.data(), j.data()) != 0,
         "%s: chunk 0 accepted", name);
  EXPECT(list(X.data(), V.data(), n, &bad, 1, kChunk, cut2, eps2, a.data(), j.data()) != 0,
         "%s: index n accepted", name);
  bad = -1;
  EXPECT(list(X.data(), V.data(), n, &bad, 1, kChunk, cut2, eps2, a.data(), j.data()) != 0,
         "%s: index -1 accepted", name);
  EXPECT(list(X.data(), V.data(), n, nullptr, 1, kChunk, cut2, eps2, a.data(), j.data()) != 0,
         "%s: null list accepted", name);
  // two steps of one hour, fixed and with the step criterion on
  for (double eta : {0.0, 0.02}) {
    std::vector<T> x = X, v = V, ac = A, jk = J, scratch(16 * n);
    for (int64_t i = 0; i < n; ++i) ac[4 * i + 3] = 0;
    for (int k = 0; k < 2; ++k) {
      double dt = -1.0;
      EXPECT(step(x.data(), v.data(), ac.data(), jk.data(), scratch.data(), n, kChunk, 3600.0, cut2,
                  eps2, eta, &dt) == 0, "%s step", name);
      EXPECT(eta > 0.0 && n > 1 ? (dt > 0.0 && isfinite(dt)) : isinf(dt), "%s: dt_min %g", name,
             dt);
    }
    EXPECT(finite(x) && finite(v) && finite(ac) && finite(jk), "%s: step not finite", name);
    EXPECT(n == 1 || !same(x, 0, X, 0, 4 * n), "%s: the step moved nothing", name);
    EXPECT(step(x.data(), v.data(), ac.data(), jk.data(), nullptr, n, kChunk, 3600.0, cut2, eps2,
                eta, nullptr) != 0, "%s: null scratch accepted", name);
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
    std::vector<double> A(4 * n), J(4 * n), Aref(4 * n), Jref(4 * n), Am(4 * n), Jm(4 * n);
    check<double>("f64", X, V, n, gs_cpu_accjerk_f64, gs_cpu_accjerk_idx_f64,
                  gs_cpu_hermite_step_f64, A, J);
    naive_accjerk(X, V, n, Aref, Jref);
    EXPECT(same(A, 0, Aref, 0, 4 * n) && same(J, 0, Jref, 0, 4 * n),
           "f64 differs from the naive loop at n = %lld", (long long)n);
    check<double>("mixed", X, V, n, gs_cpu_accjerk_mixed, gs_cpu_accjerk_idx_mixed,
                  gs_cpu_hermite_step_mixed, Am, Jm);
    std::vector<float> Xf(X.begin(), X.end()), Vf(V.begin(), V.end()), Af(4 * n), Jf(4 * n);
    check<float>("f32", Xf, Vf, n, gs_cpu_accjerk_f32, gs_cpu_accjerk_idx_f32,
                 gs_cpu_hermite_step_f32, Af, Jf);
  }
  if (fails) {
    fprintf(stderr, "%d failures\n", fails);
    return 1;
  }
  printf("cpu_hermite_selftest ok\n");
  return 0;
}
