// Stand-alone host check of sctools_amd/csrc/close_pairs_mask.h (no HIP, no Python), exhaustive and
// without input: for every plane count B = 1..6 and threshold t = 0..3, every distance 0..2^B - 1
// in every one of the 32 bit positions (the other 31 positions holding each background distance in
// turn) is compared against the plain integer compare and read back with dist_at; then the sort
// word: round trip at the corners, integer order = (i, j) order, and the radix sort's end bit.
// Prints "ok <comparisons>" or the first failure.  tests/test_close_pairs_mask_host.py builds it
// with AddressSanitizer and UBSan and runs it.
#include <cinttypes>
#include <cstdio>

#include "../../sctools_amd/csrc/close_pairs_mask.h"

namespace cp = sct::close_pairs;

static long g_checks = 0;

template <int B>
static bool check_planes() {
  for (uint32_t bg = 0; bg < (1u << B); ++bg)      // distance of the other 31 positions
    for (uint32_t v = 0; v < (1u << B); ++v)       // distance of position k
      for (int k = 0; k < 32; ++k) {
        uint32_t d[B];
        for (int b = 0; b < B; ++b) {
          d[b] = ((bg >> b) & 1u) ? ~0u : 0u;
          d[b] = (d[b] & ~(1u << k)) | (((v >> b) & 1u) << k);
        }
        for (int t = 0; t <= cp::kMaxD; ++t) {
          const uint32_t got = cp::le_mask<B>(d, t);
          uint32_t want = bg <= (uint32_t)t ? ~0u : 0u;
          want = (want & ~(1u << k)) | ((v <= (uint32_t)t ? 1u : 0u) << k);
          ++g_checks;
          if (got != want) {
            std::printf("le_mask B=%d t=%d v=%u k=%d bg=%u: got %08x want %08x\n", B, t, v, k, bg, got, want);
            return false;
          }
        }
        for (int p = 0; p < 32; ++p) {
          ++g_checks;
          if (cp::dist_at<B>(d, p) != (p == k ? v : bg)) {
            std::printf("dist_at B=%d v=%u k=%d bg=%u p=%d: got %u\n", B, v, k, bg, p, cp::dist_at<B>(d, p));
            return false;
          }
        }
      }
  return true;
}

static bool check_words() {
  const uint32_t top = 0x7FFFFFFFu;
  const uint32_t idx[] = {0u, 1u, 2u, 31u, 32u, 255u, 256u, 65535u, 65536u, 737279u, top - 1, top};
  uint64_t prev = 0;
  bool first = true;
  for (uint32_t i : idx)
    for (uint32_t j : idx) {
      if (j <= i) continue;
      for (uint32_t dist = 0; dist <= (uint32_t)cp::kMaxD; ++dist) {
        const uint64_t w = cp::pack_pair(i, j, dist);
        ++g_checks;
        if (cp::pair_i(w) != i || cp::pair_j(w) != j || cp::pair_dist(w) != dist) {
          std::printf("pack_pair(%u, %u, %u) reads back (%u, %u, %u)\n", i, j, dist, cp::pair_i(w), cp::pair_j(w),
                      cp::pair_dist(w));
          return false;
        }
        // (i, j) ascending in the loops: the words ascend, whatever the distance of the pair before
        if (!first && dist == 0 && w <= (prev | 3u)) {
          std::printf("pack_pair(%u, %u, 0) does not sort after the pair before it\n", i, j);
          return false;
        }
        prev = w;
        first = false;
      }
    }
  // the end bit covers every word of indices below n and is minimal
  const int64_t ns[] = {1, 2, 3, 4, 5, 256, 257, 65536, 65537, 737280, (int64_t)1 << 30, ((int64_t)1 << 31) - 1};
  for (int64_t n : ns) {
    const int bits = cp::pair_word_bits(n);
    const uint64_t w = cp::pack_pair((uint32_t)(n - 1), (uint32_t)(n - 1), 3);
    ++g_checks;
    if (bits < 33 || bits > 64 || (bits < 64 && (w >> bits) != 0) || (n > 1 && (w >> (bits - 1)) == 0)) {
      std::printf("pair_word_bits(%" PRId64 ") = %d for top word %016" PRIx64 "\n", n, bits, w);
      return false;
    }
  }
  return true;
}

int main() {
  const bool ok = check_planes<1>() && check_planes<2>() && check_planes<3>() && check_planes<4>() &&
                  check_planes<5>() && check_planes<6>() && check_words();
  if (!ok) return 1;
  std::printf("ok %ld\n", g_checks);
  return 0;
}
