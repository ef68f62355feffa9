// Host-side self-test of the nearest-neighbour functions of the native CPU engine
// (gs_cpu_nn_* in csrc/cpu/cpu_engine.cpp), a program of its own in the style of cpu_selftest.cpp,
// meant to be built with -fsanitize=address,undefined:
//   g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -Icsrc/include \
//       csrc/tests/cpu_nn_selftest.cpp csrc/cpu/cpu_engine.cpp csrc/common/layout.cpp
// Exit code 0 = pass.
#include <math.h>
#include <stdio.h>

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

int main() {
  const double eps2 = 1e6, cut2 = 1e-20;
  for (int64_t n : {1, 2, 3, 257, 1031}) {
    std::vector<double> pos(3 * n), vel(3 * n), mass(n), X(4 * n), R(n);
    gs_ic_fill_host(GS_IC_SOLAR_RANDOM, 7, n, 0, n, pos.data(), vel.data(), mass.data());
    for (int64_t i = 0; i < n; ++i) {
      for (int d = 0; d < 3; ++d) X[4 * i + d] = pos[3 * i + d];
      X[4 * i + 3] = 0.0;
      R[i] = (i % 4) ? 1e7 * (double)(i % 13) : 0.0;
    }
    // naive fp64 reference: smallest q over j != i, lowest j on a tie
    std::vector<double> q(n), qref(n);
    std::vector<int32_t> nn(n), nref(n);
    for (int64_t i = 0; i < n; ++i) {
      qref[i] = INFINITY;
      nref[i] = -1;
      for (int64_t j = 0; j < n; ++j) {
        const double dx = X[4 * j] - X[4 * i], dy = X[4 * j + 1] - X[4 * i + 1],
                     dz = X[4 * j + 2] - X[4 * i + 2];
        const double r2 = fma(dz, dz, fma(dy, dy, fma(dx, dx, eps2)));
        const double s = R[j] + R[i];
        const double v = fma(-s, s, r2);
        if (j != i && r2 >= cut2 && v < qref[i]) {
          qref[i] = v;
          nref[i] = (int32_t)j;
        }
      }
    }
    EXPECT(gs_cpu_nn_f64(X.data(), R.data(), n, 0, n, cut2, eps2, q.data(), nn.data()) == 0, "f64");
    for (int64_t i = 0; i < n; ++i)
      EXPECT(q[i] == qref[i] && nn[i] == nref[i], "f64 body %lld of %lld", (long long)i,
             (long long)n);
    if (n == 1) EXPECT(isinf(q[0]) && nn[0] == -1, "a single body has no neighbour");
    // the _idx form on a list in reverse order, and a sub-range
    std::vector<int32_t> idx;
    for (int64_t i = n - 1; i >= 0; i -= 3) idx.push_back((int32_t)i);
    std::vector<double> qi(idx.size());
    std::vector<int32_t> ni(idx.size());
    EXPECT(gs_cpu_nn_idx_f64(X.data(), R.data(), n, idx.data(), (int64_t)idx.size(), cut2, eps2,
                             qi.data(), ni.data()) == 0, "idx f64");
    for (size_t k = 0; k < idx.size(); ++k)
      EXPECT(qi[k] == qref[idx[k]] && ni[k] == nref[idx[k]], "idx row %zu", k);
    if (n > 2) {
      EXPECT(gs_cpu_nn_f64(X.data(), R.data(), n, 1, n - 1, cut2, eps2, q.data(), nn.data()) == 0,
             "range");
      EXPECT(q[0] == qref[1] && nn[n - 3] == nref[n - 2], "range rows");
    }
    // mixed and fp32: the same neighbour wherever the fp64 gap is wide; always in range
    std::vector<double> qm(n);
    std::vector<int32_t> nm(n);
    EXPECT(gs_cpu_nn_mixed(X.data(), R.data(), n, 0, n, cut2, eps2, qm.data(), nm.data()) == 0,
           "mixed");
    EXPECT(gs_cpu_nn_idx_mixed(X.data(), R.data(), n, idx.data(), (int64_t)idx.size(), cut2, eps2,
                               qi.data(), ni.data()) == 0, "idx mixed");
    std::vector<float> Xf(X.begin(), X.end()), Rf(R.begin(), R.end()), qf(n);
    std::vector<int32_t> nf(n);
    EXPECT(gs_cpu_nn_f32(Xf.data(), Rf.data(), n, 0, n, (float)cut2, (float)eps2, qf.data(),
                         nf.data()) == 0, "f32");
    EXPECT(gs_cpu_nn_idx_f32(Xf.data(), Rf.data(), n, idx.data(), (int64_t)idx.size(), (float)cut2,
                             (float)eps2, qf.data(), ni.data()) == 0, "idx f32");
    for (int64_t i = 0; i < n; ++i) {
      EXPECT(nm[i] >= -1 && nm[i] < n && nm[i] != i, "mixed index");
      EXPECT(nf[i] >= -1 && nf[i] < n && nf[i] != i, "f32 index");
      if (n > 1) EXPECT(fabs(qm[i] - qref[i]) <= 1e-5 * (fabs(qref[i]) + 4e16), "mixed q");
    }
    // refusals
    int32_t badi = (int32_t)n;
    EXPECT(gs_cpu_nn_idx_f64(X.data(), R.data(), n, &badi, 1, cut2, eps2, q.data(), nn.data()) != 0,
           "index out of range accepted");
    EXPECT(gs_cpu_nn_f64(X.data(), R.data(), n, 0, n + 1, cut2, eps2, q.data(), nn.data()) != 0,
           "range past n accepted");
    EXPECT(gs_cpu_nn_f64(X.data(), nullptr, n, 0, n, cut2, eps2, q.data(), nn.data()) != 0,
           "null radii accepted");
  }
  if (fails) {
    fprintf(stderr, "%d failures\n", fails);
    return 1;
  }
  printf("cpu_nn_selftest ok\n");
  return 0;
}
