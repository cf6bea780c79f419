// One description of a block that holds several arrays, walked twice: with base == NULL it measures (off ends at the byte count), with
// the allocated block it places the pointers.  Host only, no HIP: tests/emu/carve_emu.cpp builds it with a plain compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace uvo {

struct Carve {
  uint8_t* base;
  size_t off = 0;
  // `count` elements of T at the next multiple of `align` (alignof(T): directly behind the array in front, as one copy of both needs)
  template <class T>
  Carve& take(T*& p, size_t count, size_t align = 256) {
    off = (off + align - 1) / align * align;
    if (base) p = reinterpret_cast<T*>(base + off);
    off += count * sizeof(T);
    return *this;
  }
};

}  // namespace uvo
