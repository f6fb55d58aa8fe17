// Workgroup-id maps shared by host and device code (included by common.hpp).  No HIP headers:
// a plain C++ compiler can build the host side (tests/test_wgrad_block_map_cpu.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MIPIPE_HD __host__ __device__ __forceinline__
#else
#define MIPIPE_HD inline
#endif

namespace mipipe {

// XCD-aware bijective remap of a linear workgroup id (guide §5 "XCD swizzle must be
// bijective"): the hardware deals linear ids round-robin over the 8 XCDs, so class wg % 8 gets
// the contiguous run of logical ids starting at its offset, in slot order wg / 8 — consecutive
// logical tiles land on the same XCD (shared L2).
MIPIPE_HD uint32_t xcd_remap(uint32_t wg, uint32_t nwg) {
  constexpr uint32_t NX = 8;
  if (nwg < NX) return wg;
  uint32_t q = nwg / NX, r = nwg % NX;
  uint32_t x = wg % NX, l = wg / NX;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + l;
}

// Placement of a split-K launch's blocks on a 1-D grid of tiles * splits workgroups: the logical
// order is split-major (tile fastest, so within a split tn runs fastest and same-tm tiles stay
// adjacent), and xcd_remap hands each XCD a contiguous run of it.  The tiles of one k-slice —
// the blocks that read the same operand rows — then sit on one XCD (two where a run boundary
// cuts the slice) in adjacent dispatch slots, instead of one tile's splits, which share nothing
// but their output, sitting there.  Bijective for every (tiles, splits) because xcd_remap is.
struct TileSplit {
  uint32_t tile, split;
};
MIPIPE_HD TileSplit splitk_block_map(uint32_t wg, uint32_t tiles, uint32_t splits) {
  const uint32_t v = xcd_remap(wg, tiles * splits);
  const uint32_t s = v / tiles;
  return TileSplit{v - s * tiles, s};
}

}  // namespace mipipe
