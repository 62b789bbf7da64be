// Each caller-allocated `ws` of mp_*_workspace() bytes is described once, by a struct over a
// Carver whose members take their arrays in declaration order.  The size function builds it over
// a null base (it only measures), the entry point over the caller's pointer, so the two cannot
// disagree.  Only the units that carve a workspace include this header: it pulls in rocPRIM.
#pragma once

#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "mp_common.h"

namespace mp {

// Bump allocator in 256-byte steps; `off` is the extent of the arrays taken so far.
struct Carver {
  char* base;
  size_t off = 0;
  Carver(void* ws) : base((char*)ws) {}
  // an array of no elements still takes one step, as one of one element does
  template <class T>
  T* take(int64_t count) {
    T* p = base ? (T*)(base + off) : nullptr;
    off += align_up((size_t)(count > 0 ? count : 1) * sizeof(T), 256);
    return p;
  }
  // rocPRIM's temp storage follows the arrays, 256 spare bytes follow it.  An entry point checks ws_bytes
  // against this before it reports a failed size query: its size function ran the same query and ignored it
  void* rest() const { return base ? base + off : nullptr; }
  size_t total(size_t temp_bytes) const { return off + align_up(temp_bytes, 256) + 256; }
};

// temp bytes (into *bytes, which the caller zeroes, as for every size query of these units) of the
// stable select of the flagged positions of [0, n): uint8 flags in, int64 positions and their count out
static inline hipError_t select_positions_bytes(int64_t n, size_t* bytes) {
  rocprim::counting_iterator<int64_t> it(0);
  return rocprim::select((void*)nullptr, *bytes, it, (const uint8_t*)nullptr, (int64_t*)nullptr,
                         (unsigned long long*)nullptr, (size_t)(n > 0 ? n : 1), (hipStream_t)0, false);
}

}  // namespace mp
