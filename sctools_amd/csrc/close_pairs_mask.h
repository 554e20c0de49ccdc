// Pure pieces of the close-pairs pass (allpairs.hip: allpairs_close_kernel), host and device:
//   - the bit-sliced comparison "distance <= t" over the B distance planes of 32 pairs;
//   - the distance of one of the 32 positions, read back out of the planes;
//   - the 64-bit sort word of a pair (i, j, dist), whose integer order is the (i, j) order.
// The planes are those of the pair kernel's adder tree: bit k of d[b] = bit b of the distance of
// pair k.  Checked exhaustively on the host by tests/host/close_pairs_mask_check.cpp.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SCT_CP_HD __host__ __device__ inline
#else
#define SCT_CP_HD inline
#endif

namespace sct {
namespace close_pairs {

constexpr int kMaxD = 3;  // thresholds 0..3: the comparison reads planes 0 and 1, the rest must be 0

// The threshold as three all-or-nothing words (wave-uniform in the kernel), so that the comparison
// itself has no branch: low two bits {d1 d0} > t  <=>  (d1 & a) | (d0 & b) | (d1 & d0 & c).
//   t = 0: d1 | d0     t = 1: d1     t = 2: d1 & d0     t = 3: never
struct LeSelect {
  uint32_t a, b, c;
};
SCT_CP_HD LeSelect le_select(int t) {
  return LeSelect{t <= 1 ? ~0u : 0u, t == 0 ? ~0u : 0u, t == 2 ? ~0u : 0u};
}

// bit k set <=> the distance of pair k is <= t (t = 0..kMaxD, as le_select(t))
template <int B>
SCT_CP_HD uint32_t le_mask(const uint32_t (&d)[B], const LeSelect& sel) {
  const uint32_t d0 = d[0];
  const uint32_t d1 = B > 1 ? d[B > 1 ? 1 : 0] : 0u;
  uint32_t gt = (d1 & sel.a) | (d0 & sel.b) | (d1 & d0 & sel.c);
  for (int b = 2; b < B; ++b) gt |= d[b];
  return ~gt;
}
template <int B>
SCT_CP_HD uint32_t le_mask(const uint32_t (&d)[B], int t) {
  return le_mask<B>(d, le_select(t));
}

// the distance of pair k (0..31)
template <int B>
SCT_CP_HD uint32_t dist_at(const uint32_t (&d)[B], int k) {
  uint32_t v = 0;
  for (int b = 0; b < B; ++b) v |= ((d[b] >> k) & 1u) << b;
  return v;
}

// Sort word of a close pair: i (31 bits), j (31 bits), dist (2 bits), most significant first.  A
// pair occurs once, so ascending words are ascending (i, j).  i, j < 2^31, dist <= kMaxD.
SCT_CP_HD uint64_t pack_pair(uint32_t i, uint32_t j, uint32_t dist) {
  return (uint64_t)i << 33 | (uint64_t)j << 2 | (uint64_t)dist;
}
SCT_CP_HD uint32_t pair_i(uint64_t w) { return (uint32_t)(w >> 33); }
SCT_CP_HD uint32_t pair_j(uint64_t w) { return (uint32_t)(w >> 2) & 0x7FFFFFFFu; }
SCT_CP_HD uint32_t pair_dist(uint64_t w) { return (uint32_t)w & 3u; }
// bits of the word that can be set for indices below n (the radix sort's end bit), n >= 1
SCT_CP_HD int pair_word_bits(int64_t n) {
  int b = 0;
  while (b < 31 && ((int64_t)1 << b) < n) ++b;
  return 33 + b;
}

}  // namespace close_pairs
}  // namespace sct
