// The judgement of the swapped-molecule removal (include/sctools_hip.h, "removing swapped molecules"):
// pure functions shared by the kernels of molecules.hip, its host checks and the stand-alone host check
// program tests/host/swapped_keep_check.cpp.  Nothing here is computed modulo 2^64: the sum of the
// other samples' reads saturates, and the two sides of the comparison are 96-bit products held as a
// high and a low word.
#pragma once

#include <stdint.h>

#include "mix64.h"

namespace sct {

constexpr int kSwappedMaxSamples = 16;           // counters of one call
constexpr uint64_t kSwappedMaxDen = 1ull << 32;  // num <= den <= 2^32

// a + b, or 2^64 - 1 when that is smaller
SCT_HD uint64_t swapped_add_sat(uint64_t a, uint64_t b) {
  const uint64_t s = a + b;
  return s < a ? ~0ull : s;
}

// a * b for b <= 2^32 (b == 2^32 included: its low half is 0 and its high half 1), as hi * 2^64 + lo
SCT_HD void swapped_mul(uint64_t a, uint64_t b, uint64_t* hi, uint64_t* lo) {
  const uint64_t a_lo = a & 0xffffffffull, a_hi = a >> 32;
  const uint64_t b_lo = b & 0xffffffffull, b_hi = b >> 32;  // b_hi is 0 or 1
  // a * b_lo = a_hi * b_lo * 2^32 + a_lo * b_lo, each product below 2^64
  const uint64_t low = a_lo * b_lo, mid = a_hi * b_lo;
  uint64_t l = low + (mid << 32);
  uint64_t h = (mid >> 32) + (l < low ? 1 : 0);
  // + a * b_hi * 2^32
  if (b_hi) {
    const uint64_t add = a << 32;
    l += add;
    h += (a >> 32) + (l < add ? 1 : 0);
  }
  *hi = h;
  *lo = l;
}

// Whether the sample that holds r reads of a molecule keeps it when the other samples hold `others`
// together: r * (den - num) >= num * others in the integers, which is r / (r + others) >= num / den.
// 1 <= num <= den <= 2^32.
SCT_HD bool swapped_keeps(uint64_t r, uint64_t others, uint64_t num, uint64_t den) {
  if (others == 0) return true;
  uint64_t lh, ll, rh, rl;
  swapped_mul(r, den - num, &lh, &ll);
  swapped_mul(others, num, &rh, &rl);
  return lh != rh ? lh > rh : ll >= rl;
}

// what a call takes: 1 <= s <= 16 samples, and 1 <= num <= den <= 2^32 with 2 * num > den, so that two
// samples can never both keep one molecule
SCT_HD bool swapped_params_ok(int64_t s, uint64_t num, uint64_t den) {
  if (s < 1 || s > kSwappedMaxSamples) return false;
  if (num < 1 || num > den || den > kSwappedMaxDen) return false;
  return 2 * num > den;
}

}  // namespace sct
