// The arithmetic of the chunked host pipeline (encode_host.cpp: host_items): how many items a
// chunk holds and where each array's chunk lies in a stage's device block and in its share of the
// page-locked stage.  Pure functions: no HIP call, nothing of the library.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>

namespace sct {

constexpr int kPipeStages = 3;  // HostStage::pipe: one chunk's H2D, another's kernel, a third's D2H

// Element-wise calls: ~16 MB of traffic per chunk (item_bytes = inputs + outputs of one item), at
// least four chunks when there are enough items.
inline int64_t items_chunk(int64_t n, size_t item_bytes) {
  int64_t chunk = std::max<int64_t>(1 << 16, (int64_t)(((size_t)16 << 20) / std::max<size_t>(item_bytes, 1)));
  chunk = std::min<int64_t>(chunk, std::max<int64_t>(1 << 16, (n + 3) / 4));
  return std::min<int64_t>(chunk, n);
}

// The encode stream: the caller's chunk (<= 0: 16M records), 2M at most when an array goes through
// the stage (<= 2M * (L + 10) B of it per stage), and at least four chunks when there are enough
// records, so the three stages overlap even for one piece of a stream (a few million records).
inline int64_t stream_chunk(int64_t n, int64_t chunk, bool staged) {
  if (chunk <= 0) chunk = 1 << 24;
  if (staged) chunk = std::min<int64_t>(chunk, 1 << 21);
  chunk = std::min<int64_t>(chunk, std::max<int64_t>(1 << 18, (n + 3) / 4));
  return std::min<int64_t>(chunk, n);
}

// One stage of a call with N arrays: array k's chunk at doff[k] of the stage's device block (dtot
// bytes) and, when it is staged (a pageable caller array), at hoff[k] of the stage's htot bytes of
// the page-locked buffer.  Every segment is 256-byte aligned; a page-locked array takes no stage
// bytes, and an absent one (item_bytes 0) none of either.
template <int N>
struct StageLayout {
  size_t doff[N], hoff[N], dtot = 0, htot = 0;
  StageLayout(int64_t chunk, const size_t (&item_bytes)[N], const bool (&staged)[N]) {
    const auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    for (int k = 0; k < N; ++k) {
      doff[k] = dtot;
      dtot += al((size_t)chunk * item_bytes[k]);
      hoff[k] = htot;
      if (staged[k]) htot += al((size_t)chunk * item_bytes[k]);
    }
  }
};

}  // namespace sct
