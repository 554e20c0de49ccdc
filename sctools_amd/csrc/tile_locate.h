// The inverse of tile_prefix.h's prefix: which tile holds item number `target`, from the three
// levels of tile sums (c0 per tile, c1 per block of 32 tiles, c2 per block of 1,024).  A pure
// function shared by fastq.hip's line_end_kernel and the stand-alone host check program
// tests/host/tile_locate_check.cpp.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define SCT_TILE_HD __host__ __device__ __forceinline__
#else
#define SCT_TILE_HD inline
#endif

namespace sct {

struct TileAt {
  int64_t tile;               // -1: none (target >= the total count)
  unsigned long long before;  // the count of the tiles before `tile` (its exclusive prefix)
};

// The first tile whose inclusive prefix exceeds `target` -- the tile holding item `target`
// (0-based) -- in at most ceil(ntiles / 1024) + 32 + 32 steps.  Tiles of count 0 may sit anywhere
// (whole blocks of them too): a step passes every tile or block that ends at or before the target.
// Each level is walked inside the block the level above chose, and never past the arrays' ends.
SCT_TILE_HD TileAt tile_locate(const unsigned long long* c0, const unsigned long long* c1,
                               const unsigned long long* c2, int64_t ntiles, unsigned long long target) {
  const int64_t n1 = (ntiles + 31) >> 5, n2 = (ntiles + 1023) >> 10;
  unsigned long long pre = 0;
  int64_t a = 0;
  while (a < n2 && c2[a] <= target - pre) pre += c2[a++];
  if (a == n2) return TileAt{-1, pre};
  int64_t b = a << 5;
  const int64_t bend = b + 32 < n1 ? b + 32 : n1;
  while (b < bend && c1[b] <= target - pre) pre += c1[b++];
  if (b == bend) return TileAt{-1, pre};  // (levels that do not add up: c2[a] promised an item here)
  int64_t t = b << 5;
  const int64_t tend = t + 32 < ntiles ? t + 32 : ntiles;
  while (t < tend && c0[t] <= target - pre) pre += c0[t++];
  if (t == tend) return TileAt{-1, pre};
  return TileAt{t, pre};
}

}  // namespace sct
