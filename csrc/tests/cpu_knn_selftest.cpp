// Host-side self-test of the k-nearest-neighbour functions of the native CPU engine
// (gs_cpu_knn_* in csrc/cpu/cpu_engine.cpp), a program of its own in the style of
// cpu_nn_selftest.cpp, meant to be built with -fsanitize=address,undefined:
//   g++ -O1 -g -std=c++17 -fopenmp -ffp-contract=off -fsanitize=address,undefined \
//       -Icsrc/include csrc/tests/cpu_knn_selftest.cpp csrc/cpu/cpu_engine.cpp \
//       csrc/common/layout.cpp
// Every entry point against a brute-force sort of (r^2, j) in its own arithmetic. Exit code 0 =
// pass.
#include <math.h>
#include <stdio.h>

#include <algorithm>
#include <utility>
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

// Brute force in type T: all (r^2, j), j != i, sorted lexicographically. lo (mixed): the lo rows.
template <typename T>
static void brute(const std::vector<T>& X, const std::vector<T>* L, int64_t n, int32_t k,
                  std::vector<double>& r2, std::vector<int32_t>& idx) {
  r2.assign((size_t)n * k, INFINITY);
  idx.assign((size_t)n * k, -1);
  for (int64_t i = 0; i < n; ++i) {
    std::vector<std::pair<T, int32_t>> all;
    for (int64_t j = 0; j < n; ++j) {
      if (j == i) continue;
      T d[3];
      for (int c = 0; c < 3; ++c) {
        d[c] = X[4 * j + c] - X[4 * i + c];
        if (L) d[c] = d[c] + ((*L)[4 * j + c] - (*L)[4 * i + c]);
      }
      all.emplace_back(std::fma(d[2], d[2], std::fma(d[1], d[1], d[0] * d[0])), (int32_t)j);
    }
    std::sort(all.begin(), all.end());
    for (int32_t s = 0; s < k && s < (int32_t)all.size(); ++s) {
      r2[i * k + s] = (double)all[s].first;
      idx[i * k + s] = all[s].second;
    }
  }
}

template <typename A, typename B>
static bool same(const std::vector<A>& a, const std::vector<B>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (!((double)a[i] == (double)b[i])) return false;
  return true;
}

int main() {
  for (int64_t n : {1, 2, 7, 9, 257, 1031}) {
    std::vector<double> pos(3 * n), vel(3 * n), mass(n), X(4 * n);
    gs_ic_fill_host(GS_IC_RANDOM, 11, n, 0, n, pos.data(), vel.data(), mass.data());
    if (n > 8)  // coincident bodies far apart in index: neighbours at r^2 = 0, ties by j
      for (int d = 0; d < 3; ++d) pos[3 * (n - 1) + d] = pos[3 * 2 + d];
    for (int64_t i = 0; i < n; ++i) {
      for (int d = 0; d < 3; ++d) X[4 * i + d] = pos[3 * i + d];
      X[4 * i + 3] = mass[i];
    }
    std::vector<float> Xf(X.begin(), X.end()), H(4 * n), L(4 * n);
    for (int64_t i = 0; i < 4 * n; ++i) {
      H[i] = (float)X[i];
      L[i] = (float)(X[i] - (double)H[i]);
    }
    for (int32_t k : {1, 6, 8}) {
      std::vector<double> rref, r((size_t)n * k), rm((size_t)n * k);
      std::vector<int32_t> iref, ix((size_t)n * k);
      std::vector<float> rf((size_t)n * k);
      brute<double>(X, nullptr, n, k, rref, iref);
      EXPECT(gs_cpu_knn_f64(X.data(), n, 0, n, k, r.data(), ix.data()) == 0, "f64");
      EXPECT(same(r, rref) && same(ix, iref), "f64 lists n=%lld k=%d", (long long)n, k);
      if (n > 2) {  // a sub-range lands at row 0
        std::vector<double> rs((size_t)(n - 2) * k);
        std::vector<int32_t> is((size_t)(n - 2) * k);
        EXPECT(gs_cpu_knn_f64(X.data(), n, 1, n - 1, k, rs.data(), is.data()) == 0, "f64 range");
        bool ok = true;
        for (size_t t = 0; t < rs.size(); ++t)
          ok = ok && rs[t] == rref[k + t] && is[t] == iref[k + t];
        EXPECT(ok, "f64 sub-range n=%lld k=%d", (long long)n, k);
      }
      brute<float>(Xf, nullptr, n, k, rref, iref);
      EXPECT(gs_cpu_knn_f32(Xf.data(), n, 0, n, k, rf.data(), ix.data()) == 0, "f32");
      EXPECT(same(rf, rref) && same(ix, iref), "f32 lists n=%lld k=%d", (long long)n, k);
      brute<float>(H, &L, n, k, rref, iref);
      EXPECT(gs_cpu_knn_mixed(X.data(), n, 0, n, k, rm.data(), ix.data()) == 0, "mixed");
      EXPECT(same(rm, rref) && same(ix, iref), "mixed lists n=%lld k=%d", (long long)n, k);
    }
    // refusals
    std::vector<double> r(8 * n);
    std::vector<int32_t> ix(8 * n);
    EXPECT(gs_cpu_knn_f64(X.data(), n, 0, n, 0, r.data(), ix.data()) != 0, "k = 0 accepted");
    EXPECT(gs_cpu_knn_f64(X.data(), n, 0, n, 9, r.data(), ix.data()) != 0, "k = 9 accepted");
    EXPECT(gs_cpu_knn_f64(X.data(), n, 0, n + 1, 6, r.data(), ix.data()) != 0, "range accepted");
    EXPECT(gs_cpu_knn_mixed(nullptr, n, 0, n, 6, r.data(), ix.data()) != 0, "null accepted");
    EXPECT(gs_cpu_knn_f32(Xf.data(), 0, 0, 0, 6, nullptr, ix.data()) != 0, "n = 0 accepted");
  }
  if (fails) {
    fprintf(stderr, "%d failure(s)\n", fails);
    return 1;
  }
  printf("cpu_knn_selftest ok\n");
  return 0;
}
