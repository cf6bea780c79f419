// Device and page-locked memory of one owner (a handle, or one of its lanes): a buffer is freed because it was allocated here, not because a
// list names it.  No pool and no reuse -- a registry.  A destroy function sets the device, drains its stream and calls release_all().
#pragma once
#include <algorithm>
#include <vector>

#include "carve.hpp"
#include "common.hpp"

namespace uvo {

struct DevMem {
  struct Block {
    void* p;
    size_t bytes;
    bool pinned;
  };
  std::vector<Block> blocks;
  int alloc_bytes(void** p, size_t bytes, bool pinned);  // *p = NULL when it fails
  template <class T>
  int alloc(T** p, size_t n, bool pinned = false) {  // n elements (at least one)
    return alloc_bytes((void**)p, std::max<size_t>(n, 1) * sizeof(T), pinned);
  }
  size_t bytes_of(const void* p) const;  // 0: not a buffer of this owner
  void release(void* p);
  void release_all();
};

// One block of owner m that holds the arrays `layout` (a callable on a Carve&) describes: measured, allocated, then placed
template <class F>
int alloc_carved(DevMem& m, F&& layout, bool pinned = false) {
  Carve measure{nullptr}, place{nullptr};
  layout(measure);
  RC(m.alloc(&place.base, measure.off, pinned));
  layout(place);
  return UVO_OK;
}

}  // namespace uvo
