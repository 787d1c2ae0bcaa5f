// workspace_carve.h -- one pass over a workspace gives its pointers and its size. A workspace has one function that takes its
// arrays from a Carve in order; run over the allocation it sets the pointers, run over NULL it only counts, and the count
// of that run is what the allocation is sized from: no formula next to the carve can disagree with it. Host only.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace cldn {

struct Carve {
  uint8_t* base;   // NULL: a sizing pass
  size_t off = 0;
  explicit Carve(void* base_) : base((uint8_t*)base_) {}
  // [count] of T at the next multiple of `align` (a power of two; offsets count from `base`, which hipMalloc aligns to 256)
  template <class T>
  T* take(size_t count, size_t align = alignof(T)) {
    off = (off + align - 1u) & ~(align - 1u);
    T* const at = base ? (T*)(base + off) : nullptr;
    off += count * sizeof(T);
    return at;
  }
  void pad(size_t bytes) { off += bytes; }
  size_t bytes() const { return off; }
};

}  // namespace cldn
