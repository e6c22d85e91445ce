// csrc/scratch_carve.hpp on the CPU (no HIP, no libsks): the scratch of the
// all-pairs ANI call — a join layout, 16 bytes of status, the packed count
// tiles (16 KB each; none when the caller brings its own) and the layout
// build's temporary storage plus 256 bytes — must sit where the offset chain
//   al(x) = (x + 255) & ~255
//   o_vals = 0, o_masks = al(o_vals + tot * 8 * ew), o_boff = al(o_masks + tot * 8),
//   o_bst = al(o_boff + nb * BW * 4), o_stat = al(o_bst + (nb + 1) * 8),
//   o_cnt = al(o_stat + 16), o_tmp = al(o_cnt + tiles * 16384), need = o_tmp + temp + 256
// with tot = max(total, 1) puts it; the expected offsets below are that chain
// evaluated by hand.  BW = 2^log_b + 2^max(log_b - 3, 0) + 1 (join_common.hpp).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "scratch_carve.hpp"

namespace {

int failures = 0;

void check(bool ok, const char* shape, const char* what) {
  if (ok) return;
  std::printf("FAIL %s: %s\n", shape, what);
  ++failures;
}

struct Shape {
  const char* name;
  uint64_t total;
  uint32_t blocks;
  size_t boff_words;
  int ew;
  uint64_t tiles;  // packed count tiles in scratch (0: the caller's)
  size_t temp;
  size_t want[7];  // vals, masks, boff, bstart, stat, counts, temp
  size_t want_need;
};

void run(const Shape& s) {
  sks::Carver cv;
  const sks::LayoutRegions lay = sks::carve_layout(cv, s.total, s.blocks, s.boff_words, s.ew);
  const sks::Region<uint32_t> stat = cv.take<uint32_t>(4);
  const sks::Region<int32_t> cnt = cv.take<int32_t>(s.tiles * 4096);
  const sks::Region<char> tmp = cv.take<char>(s.temp + 256);
  const uint64_t tot = s.total ? s.total : 1;
  const size_t off[7] = {lay.vals.off, lay.masks.off, lay.boff.off, lay.bstart.off, stat.off, cnt.off, tmp.off};
  const size_t bytes[7] = {tot * 8 * s.ew, tot * 8,          s.blocks * s.boff_words * 4, (s.blocks + 1) * 8ul,
                           16,             s.tiles * 16384, s.temp + 256};
  for (int i = 0; i < 7; ++i) {
    check(off[i] % 256 == 0, s.name, "a region is not 256-byte aligned");
    check(off[i] == s.want[i], s.name, "a region is not at the hand-evaluated offset");
    // in the stated order, without overlap, each at least its requested size
    const size_t next = i < 6 ? off[i + 1] : cv.need();
    check(off[i] + bytes[i] <= next, s.name, "a region is smaller than requested or overlaps the next");
  }
  check(cv.need() == off[6] + bytes[6], s.name, "need is not the end of the last region");
  check(cv.need() == s.want_need, s.name, "need is not the hand-evaluated size");

  // the second pass: typed pointers into a block of `need` bytes
  std::vector<char> block(cv.need());
  const sks::LayoutArrays a = lay.in(block.data());
  check(reinterpret_cast<char*>(a.vals) == block.data() + off[0] &&
            reinterpret_cast<char*>(a.masks) == block.data() + off[1] &&
            reinterpret_cast<char*>(a.boff) == block.data() + off[2] &&
            reinterpret_cast<char*>(a.bstart) == block.data() + off[3] && tmp.in(block.data()) == block.data() + off[6],
        s.name, "a pointer is not base + offset");
  a.vals[tot * s.ew - 1] = 1;  // the last word of the first and of the last region are inside the block
  tmp.in(block.data())[s.temp + 255] = 1;
}

}  // namespace

int main() {
  const Shape shapes[] = {
      // n = 1, no elements: one slot all the same (tot = 1); log_b = 0, BW = 3; one tile
      //   masks al(8) = 256; boff al(256 + 8) = 512; bstart al(512 + 12) = 768; stat al(768 + 16) = 1024;
      //   counts al(1024 + 16) = 1280; temp al(1280 + 16384 = 17664) = 17664; need 17664 + 1000 + 256
      {"n=1 total=0", 0, 1, 3, 1, 1, 1000, {0, 256, 512, 768, 1024, 1280, 17664}, 18920},
      {"n=1 total=1", 1, 1, 3, 1, 1, 1000, {0, 256, 512, 768, 1024, 1280, 17664}, 18920},
      // n = 64 sketches of 100: one block; log_b = 4, BW = 16 + 2 + 1 = 19; one tile
      //   masks al(51200) = 51200; boff al(102400) = 102400; bstart al(102400 + 76 = 102476) = 102656;
      //   stat al(102656 + 16) = 102912; counts al(102928) = 103168; temp al(103168 + 16384 = 119552) = 119552
      {"n=64", 6400, 1, 19, 1, 1, 1000, {0, 51200, 102400, 102656, 102912, 103168, 119552}, 120808},
      // n = 65 sketches of 100: two blocks (a second bstart row), three tiles
      //   masks al(52000) = 52224; boff al(52224 + 52000 = 104224) = 104448; bstart al(104448 + 152 = 104600) =
      //   104704; stat al(104704 + 24) = 104960; counts al(104976) = 105216; temp al(105216 + 49152 = 154368) = 154368
      {"n=65", 6500, 2, 19, 1, 3, 1000, {0, 52224, 104448, 104704, 104960, 105216, 154368}, 155624},
      // 128-bit elements, 1001 of them (every region but the last ends off a 256-byte boundary); log_b = 7,
      // BW = 128 + 16 + 1 = 145; the caller's count tiles (an empty region: temp starts where it would)
      //   masks al(16016) = 16128; boff al(16128 + 8008 = 24136) = 24320; bstart al(24320 + 580 = 24900) = 25088;
      //   stat al(25088 + 16) = 25344; counts al(25360) = 25600; temp al(25600 + 0) = 25600
      {"ew=2 total=1001", 1001, 1, 145, 2, 0, 1000, {0, 16128, 24320, 25088, 25344, 25600, 25600}, 26856},
  };
  for (const Shape& s : shapes) run(s);
  if (failures) return 1;
  std::printf("carve ok: %zu shapes\n", sizeof shapes / sizeof shapes[0]);
  return 0;
}
