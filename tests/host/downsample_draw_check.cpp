// Stand-alone host check of sctools_amd/csrc/downsample_draw.h (no HIP, no Python): reads cases from
// stdin, one per line, and prints one line per case:
//   d seed key j            the stream and the draw of read j
//   t seed key r T          thin(seed, key, r, T), and the same as 64 strided shares summed
//   y seed k n T            the tally key of k and thin_tally(seed, k, n, T)
//   b draw k th[0..k)       the bucket of `draw` among the k thresholds, and whether they are a legal set
// (all numbers decimal, unsigned 64-bit).  tests/test_downsample_draw_host.py compares the lines with
// tests/downsample_reference.py; the program is built with AddressSanitizer and UBSan.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../sctools_amd/csrc/downsample_draw.h"

static bool number(uint64_t* v) {
  unsigned long long x = 0;
  if (std::scanf("%llu", &x) != 1) return false;
  *v = x;
  return true;
}

int main() {
  char what = 0;
  long cases = 0;
  while (std::scanf(" %c", &what) == 1) {
    uint64_t a = 0, b = 0, c = 0, d = 0;
    if (what == 'd') {
      if (!number(&a) || !number(&b) || !number(&c)) return 1;
      std::printf("%" PRIu64 " %" PRIu64 "\n", sct::downsample_stream(a, b), sct::downsample_draw(a, b, c));
    } else if (what == 't') {
      if (!number(&a) || !number(&b) || !number(&c) || !number(&d)) return 1;
      uint64_t shared = 0;
      for (uint64_t lane = 0; lane < 64; ++lane)
        shared += sct::downsample_thin_stride(sct::downsample_stream(a, b), lane, 64, c, d);
      std::printf("%" PRIu64 " %" PRIu64 "\n", sct::downsample_thin(a, b, c, d), shared);
    } else if (what == 'y') {
      if (!number(&a) || !number(&b) || !number(&c) || !number(&d) || b > 3) return 1;
      const uint64_t key = sct::downsample_tally_key((int)b);
      std::printf("%" PRIu64 " %" PRIu64 "\n", key, sct::downsample_thin(a, key, c, d));
    } else if (what == 'b') {
      if (!number(&a) || !number(&b) || b > 100) return 1;
      std::vector<uint64_t> th((size_t)b);  // exactly k words: a search that reads th[k] is caught
      for (uint64_t& t : th)
        if (!number(&t)) return 1;
      const bool ok = sct::downsample_thresholds_ok(th.data(), (int64_t)b);
      const int at = ok ? sct::downsample_bucket(a, th.data(), (int)b) : -1;
      std::printf("%d %d\n", at, ok ? 1 : 0);
    } else {
      std::printf("bad case\n");
      return 1;
    }
    ++cases;
  }
  std::printf("ok %ld\n", cases);
  return 0;
}
