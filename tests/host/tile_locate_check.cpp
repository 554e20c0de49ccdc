// Stand-alone host check of sctools_amd/csrc/tile_locate.h (no HIP, no Python).  Reads from stdin
// any number of cases "ntiles  c0[0] .. c0[ntiles - 1]  ntargets  target ..." (decimal), forms c1 and
// c2 as plain sums of c0 over blocks of 32 and 1,024 tiles (tile_prefix.h's definition, in arrays of
// exactly ceil(ntiles / 32) and ceil(ntiles / 1024) words, so a step past an end is an
// AddressSanitizer report), and prints "tile before" per target (tile -1 = none), then
// "ok <cases> <targets>".  tests/test_tile_locate_host.py holds the lines against a plain prefix sum;
// the program is built with AddressSanitizer and UBSan.
#include <cstdio>
#include <vector>

#include "../../sctools_amd/csrc/tile_locate.h"

int main() {
  long long ntiles = 0;
  long cases = 0, targets = 0;
  while (std::scanf("%lld", &ntiles) == 1) {
    if (ntiles < 1) return 2;
    std::vector<unsigned long long> c0((size_t)ntiles), c1((size_t)((ntiles + 31) / 32), 0ull),
        c2((size_t)((ntiles + 1023) / 1024), 0ull);
    for (long long t = 0; t < ntiles; ++t) {
      if (std::scanf("%llu", &c0[(size_t)t]) != 1) return 2;
      c1[(size_t)(t / 32)] += c0[(size_t)t];
      c2[(size_t)(t / 1024)] += c0[(size_t)t];
    }
    long long nt = 0;
    if (std::scanf("%lld", &nt) != 1) return 2;
    for (long long k = 0; k < nt; ++k) {
      unsigned long long target = 0;
      if (std::scanf("%llu", &target) != 1) return 2;
      const sct::TileAt at = sct::tile_locate(c0.data(), c1.data(), c2.data(), ntiles, target);
      std::printf("%lld %llu\n", (long long)at.tile, at.before);
      ++targets;
    }
    ++cases;
  }
  std::printf("ok %ld %ld\n", cases, targets);
  return 0;
}
