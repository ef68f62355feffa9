// Device buffers owned in groups (no HIP include: the backend is a template parameter).
//
// A DevGroup holds the buffers that share one lifetime rule ("exist while the order is 6"). Each
// buffer is allocated into a pointer of the owner (its slot); the group remembers the slot and
// nulls it when it frees the buffer, so a freed buffer never leaves a pointer behind and nothing
// is freed twice. rebuild() states a rule once: a group is either complete or empty.
//
// The backend B supplies three static operations:
//   const char* alloc(void** p, size_t bytes)   null, or why it failed (*p untouched)
//   void free(void* p)                          (a failure is ignored)
//   void mem_info(size_t* free_b, size_t* total_b)
// The runtime's is gs::rt::HipMem (gs_stepper.h); csrc/tests/cpu_devmem_selftest.cpp has a fake
// one on host memory, which is what the parameter is for.
#pragma once
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <vector>

void gs_set_error(const char* msg);

namespace gs {

template <typename B>
class DevGroup {
 public:
  struct Entry {
    void* slot;  // address of the owner's pointer
    void* p;
    size_t bytes;  // as asked for (0 allocates 16)
    const char* tag;
  };

  DevGroup() = default;
  DevGroup(const DevGroup&) = delete;
  DevGroup& operator=(const DevGroup&) = delete;
  ~DevGroup() { release(); }

  // `bytes` of device memory into *slot. On failure *slot and the group stay as they were, the
  // error names the buffer, its size and the free memory, and -1 comes back.
  template <typename T>
  int alloc(T** slot, size_t bytes, const char* tag) {
    void* v = nullptr;
    if (const char* why = B::alloc(&v, bytes ? bytes : 16)) {
      size_t free_b = 0, total_b = 0;
      B::mem_info(&free_b, &total_b);
      char b[320];
      snprintf(b, sizeof(b), "device allocation of %s (%.3f GB) failed: %s (free %.3f of %.3f GB)",
               tag, bytes / 1e9, why, free_b / 1e9, total_b / 1e9);
      gs_set_error(b);
      return -1;
    }
    *slot = static_cast<T*>(v);
    entries_.push_back({slot, v, bytes, tag});
    return 0;
  }

  // Free every buffer, null every slot, empty the group.
  void release() {
    for (const Entry& e : entries_) {
      B::free(e.p);
      memset(e.slot, 0, sizeof(void*));  // (the slot's own type is gone: a null object pointer)
    }
    entries_.clear();
  }

  // release(), then fill(*this); a fill that fails (nonzero) leaves the group empty.
  template <typename F>
  int rebuild(F fill) {
    release();
    if (fill(*this) == 0) return 0;
    release();
    return -1;
  }

  // The ledger: what the group holds, in allocation order.
  const std::vector<Entry>& entries() const { return entries_; }

 private:
  std::vector<Entry> entries_;
};

}  // namespace gs
