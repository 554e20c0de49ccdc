// The draw of the read downsampling (include/sctools_hip.h, "downsampling reads"): pure functions
// shared by the kernels of molecules.hip, its host checks and the stand-alone host check program
// tests/host/downsample_draw_check.cpp.  All arithmetic is unsigned 64-bit and wraps modulo 2^64.
#pragma once

#include <stdint.h>

#include "mix64.h"

namespace sct {

constexpr uint64_t kDownsampleG = 0x9e3779b97f4a7c15ull;
constexpr uint64_t kDownsampleKeepAll = 1ull << 32;  // the threshold that keeps every read
constexpr int kDownsampleMaxPoints = 64;             // thresholds of one curve

// the stream of a key under a seed: everything a molecule's draws depend on beside the read number
SCT_HD uint64_t downsample_stream(uint64_t seed, uint64_t key) { return mix64(key ^ mix64(seed ^ kDownsampleG)); }

// the draw of read j = 0, 1, ... of a stream, below 2^32; (j + 1) * G wraps
SCT_HD uint64_t downsample_draw_at(uint64_t stream, uint64_t j) {
  return mix64(stream + (j + 1) * kDownsampleG) >> 32;
}
SCT_HD uint64_t downsample_draw(uint64_t seed, uint64_t key, uint64_t j) {
  return downsample_draw_at(downsample_stream(seed, key), j);
}

// The reads j = j0, j0 + step, ... below r that are kept at `threshold` (draw < threshold).  (0, 1) is
// thin() itself; (lane, 64) is a wave's share of it, to be summed.
SCT_HD uint64_t downsample_thin_stride(uint64_t stream, uint64_t j0, uint64_t step, uint64_t r, uint64_t threshold) {
  uint64_t kept = 0;
  for (uint64_t j = j0; j < r; j += step) kept += downsample_draw_at(stream, j) < threshold;
  return kept;
}
SCT_HD uint64_t downsample_thin(uint64_t seed, uint64_t key, uint64_t r, uint64_t threshold) {
  return downsample_thin_stride(downsample_stream(seed, key), 0, 1, r, threshold);
}

// the key of tally k (0 no match, 1 ambiguous, 2 bad UMI, 3 no feature): the top bit is set, which
// no molecule's key has
SCT_HD uint64_t downsample_tally_key(int k) { return (1ull << 63) | (uint64_t)k; }

// the bucket of a draw among k ascending thresholds: the first t with draw < thresholds[t], else k.
// A read in bucket b is kept at every thresholds[t] with t >= b.
SCT_HD int downsample_bucket(uint64_t draw, const uint64_t* thresholds, int k) {
  int lo = 0, hi = k;  // thresholds[t] <= draw for t < lo, draw < thresholds[t] for t >= hi
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (draw < thresholds[mid]) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// what a curve takes: 1 <= k <= 64 thresholds, none above 2^32, none below the one before it
SCT_HD bool downsample_thresholds_ok(const uint64_t* thresholds, int64_t k) {
  if (k < 1 || k > kDownsampleMaxPoints) return false;
  for (int64_t t = 0; t < k; ++t) {
    if (thresholds[t] > kDownsampleKeepAll) return false;
    if (t > 0 && thresholds[t] < thresholds[t - 1]) return false;
  }
  return true;
}

}  // namespace sct
