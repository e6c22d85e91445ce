// Carving one scratch block into 256-byte-aligned regions (host arithmetic
// only: no HIP, so tests/cpp/carve_test.cpp checks it on any machine).
//
// First pass: take() the regions in their fixed order; need() is then the size
// to reserve.  Second pass, once the block exists: Region::in(base) gives each
// region's typed pointer.  A region starts where the one before it ended,
// rounded up to 256 bytes; an empty region takes no room.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace sks {

template <class T>
struct Region {
  size_t off = 0;  // bytes from the block's start, a multiple of 256
  T* in(void* base) const { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }
};

class Carver {
 public:
  static constexpr size_t kAlign = 256;
  template <class T>
  Region<T> take(size_t count) {
    const Region<T> r{next_};
    end_ = next_ + count * sizeof(T);
    next_ = (end_ + kAlign - 1) & ~(kAlign - 1);
    return r;
  }
  size_t need() const { return end_; }  // the end of the last region taken

 private:
  size_t next_ = 0, end_ = 0;
};

// The four arrays of a join layout (join.hpp JoinLayout, format in
// join_common.hpp), writable as the layout build needs them.
struct LayoutArrays {
  uint64_t* vals;
  uint64_t* masks;
  uint32_t* boff;
  uint64_t* bstart;
};

struct LayoutRegions {
  Region<uint64_t> vals, masks;
  Region<uint32_t> boff;
  Region<uint64_t> bstart;
  LayoutArrays in(void* base) const { return {vals.in(base), masks.in(base), boff.in(base), bstart.in(base)}; }
};

// A layout of `total` elements (an empty one still gets one slot) of `ew` words
// in `blocks` 64-sketch blocks, each with a row of `boff_words`
// (join_layout_boff_words(log_b)) bucket starts: vals, masks, boff, bstart.
inline LayoutRegions carve_layout(Carver& cv, uint64_t total, uint32_t blocks, size_t boff_words, int ew) {
  const size_t slots = (size_t)std::max<uint64_t>(total, 1);
  LayoutRegions r;
  r.vals = cv.take<uint64_t>(slots * ew);
  r.masks = cv.take<uint64_t>(slots);
  r.boff = cv.take<uint32_t>((size_t)blocks * boff_words);
  r.bstart = cv.take<uint64_t>((size_t)blocks + 1);
  return r;
}

}  // namespace sks
