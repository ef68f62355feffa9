// Host-side self-test of the device buffer groups (gs::DevGroup, csrc/include/gs_devmem.h) on a
// backend of host memory, a program of its own in the style of cpu_selftest.cpp, meant to be
// built with -fsanitize=address,undefined (a double free or a use after free is then an error):
//   g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -Icsrc/include \
//       csrc/tests/cpu_devmem_selftest.cpp csrc/cpu/cpu_engine.cpp csrc/common/layout.cpp
// Exit code 0 = pass.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gravsim.h"
#include "gs_devmem.h"

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

// Host memory for device memory. It counts the live blocks (the sanitizer's leak check is off
// where this runs) and fails the fail_at-th allocation since the last arm().
struct FakeMem {
  static int live, calls, fail_at;
  static size_t last_bytes;
  static void arm(int k) { calls = 0; fail_at = k; }
  static const char* alloc(void** p, size_t bytes) {
    last_bytes = bytes;
    if (++calls == fail_at) return "out of fake memory";
    *p = malloc(bytes);
    ++live;
    return nullptr;
  }
  static void free(void* p) {
    ::free(p);
    --live;
  }
  static void mem_info(size_t* free_b, size_t* total_b) {
    *free_b = (size_t)2e9;
    *total_b = (size_t)8e9;
  }
};
int FakeMem::live = 0, FakeMem::calls = 0, FakeMem::fail_at = 0;
size_t FakeMem::last_bytes = 0;

using Group = gs::DevGroup<FakeMem>;

// An owner with five slots of several pointer types, as the runtime's structs have.
struct Owner {
  void* a = nullptr;
  float* b = nullptr;
  double* c = nullptr;
  int32_t* d = nullptr;
  unsigned long long* e = nullptr;
  bool all_null() const { return !a && !b && !c && !d && !e; }
  bool none_null() const { return a && b && c && d && e; }
};
static const char* const kTags[5] = {"alpha", "beta", "gamma", "delta", "epsilon"};
static const size_t kBytes[5] = {7000000, 64, 24, 4096, 8};
static const char* const kGB[5] = {"(0.007 GB)", "(0.000 GB)", "(0.000 GB)", "(0.000 GB)",
                                   "(0.000 GB)"};

static int fill5(Group& g, Owner& o) {
  return g.alloc(&o.a, kBytes[0], kTags[0]) || g.alloc(&o.b, kBytes[1], kTags[1]) ||
                 g.alloc(&o.c, kBytes[2], kTags[2]) || g.alloc(&o.d, kBytes[3], kTags[3]) ||
                 g.alloc(&o.e, kBytes[4], kTags[4])
             ? -1
             : 0;
}

int main() {
  // the k-th of five allocations fails: the group is empty, every slot null, nothing live, and
  // the error names the buffer, its size, the backend's reason and the free memory
  for (int k = 1; k <= 5; ++k) {
    Owner o;
    Group g;
    FakeMem::arm(k);
    EXPECT(g.rebuild([&](Group& gg) { return fill5(gg, o); }) == -1, "k %d: rebuild succeeded", k);
    EXPECT(o.all_null(), "k %d: a slot is left non-null", k);
    EXPECT(FakeMem::live == 0, "k %d: %d blocks live", k, FakeMem::live);
    EXPECT(g.entries().empty(), "k %d: entries left", k);
    const char* err = gs_last_error();
    char head[64];
    snprintf(head, sizeof(head), "device allocation of %s %s failed", kTags[k - 1], kGB[k - 1]);
    EXPECT(strstr(err, head) != nullptr, "k %d: error text '%s' lacks '%s'", k, err, head);
    EXPECT(strstr(err, "out of fake memory (free 2.000 of 8.000 GB)") != nullptr,
           "k %d: error text '%s'", k, err);
  }

  // a failed alloc outside rebuild leaves the slot and the group as they were
  {
    Owner o;
    Group g;
    FakeMem::arm(0);
    EXPECT(g.alloc(&o.b, 64, "beta") == 0, "alloc");
    float* const was = o.b;
    FakeMem::arm(1);
    EXPECT(g.alloc(&o.b, 128, "beta2") == -1, "alloc did not fail");
    EXPECT(o.b == was && g.entries().size() == 1 && FakeMem::live == 1, "a failed alloc changed");
    o.b[15] = 1.0f;  // (still owned: the sanitizer would object to a freed block)
  }
  EXPECT(FakeMem::live == 0, "the destructor left %d blocks live", FakeMem::live);

  // success: the ledger in allocation order; release() nulls every slot; twice is harmless
  {
    Owner o;
    Group g;
    FakeMem::arm(0);
    EXPECT(g.rebuild([&](Group& gg) { return fill5(gg, o); }) == 0, "rebuild failed");
    EXPECT(o.none_null() && FakeMem::live == 5, "5 buffers expected, %d live", FakeMem::live);
    EXPECT(g.entries().size() == 5, "5 entries expected");
    for (size_t i = 0; i < g.entries().size() && i < 5; ++i)
      EXPECT(strcmp(g.entries()[i].tag, kTags[i]) == 0 && g.entries()[i].bytes == kBytes[i],
             "entry %zu: %s, %zu bytes", i, g.entries()[i].tag, g.entries()[i].bytes);
    memset(o.d, 0xff, kBytes[3]);
    g.release();
    EXPECT(o.all_null() && FakeMem::live == 0 && g.entries().empty(), "release left something");
    g.release();
    EXPECT(FakeMem::live == 0, "a second release freed again");

    // rebuild over a complete group with a failing fill: empty, nothing live
    EXPECT(g.rebuild([&](Group& gg) { return fill5(gg, o); }) == 0, "rebuild failed");
    void* const first = o.a;
    FakeMem::arm(3);
    EXPECT(g.rebuild([&](Group& gg) { return fill5(gg, o); }) == -1, "rebuild succeeded");
    EXPECT(o.all_null() && FakeMem::live == 0 && g.entries().empty(),
           "a failed rebuild left the old group (%p) or part of the new", first);

    // rebuild over a complete group: the old buffers go, the new ones stand
    FakeMem::arm(0);
    EXPECT(g.rebuild([&](Group& gg) { return fill5(gg, o); }) == 0, "rebuild failed");
    EXPECT(g.rebuild([&](Group& gg) { return gg.alloc(&o.c, 24, "gamma"); }) == 0, "rebuild failed");
    EXPECT(!o.a && !o.b && o.c && !o.d && !o.e && FakeMem::live == 1 && g.entries().size() == 1,
           "rebuild to one buffer: %d live", FakeMem::live);
  }
  EXPECT(FakeMem::live == 0, "the destructor left %d blocks live", FakeMem::live);

  // a request of zero bytes is recorded as such and allocates 16
  {
    Owner o;
    Group g;
    FakeMem::arm(0);
    EXPECT(g.alloc(&o.e, 0, "empty") == 0, "alloc of 0 bytes");
    EXPECT(g.entries()[0].bytes == 0 && FakeMem::last_bytes == 16, "0 bytes: recorded %zu, got %zu",
           g.entries()[0].bytes, FakeMem::last_bytes);
    o.e[1] = 1;  // (the last of the 16 bytes)
  }
  EXPECT(FakeMem::live == 0, "the destructor left %d blocks live", FakeMem::live);

  if (fails) {
    fprintf(stderr, "%d failure(s)\n", fails);
    return 1;
  }
  printf("cpu_devmem_selftest ok\n");
  return 0;
}
