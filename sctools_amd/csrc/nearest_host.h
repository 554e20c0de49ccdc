// The staged batch call behind the nearest *_host entry points (nearest_host.cpp) and their
// multi-device forms (devices.cpp).
#pragma once

#include "sct_common.h"

namespace sct {

// Host arrays of one batch.  qual == nullptr: sct_nearest_query; else sct_nearest_correct over
// quality rows qual_stride bytes apart.
struct NearestIn {
  const uint64_t* queries;
  const uint8_t* qual;
  int64_t qual_stride;
  int64_t nq;
};

// What comes back.  tally == nullptr: index[nq] and dist[nq] are written; else the indices are
// tallied on the device and only the words come back, ADDED to counts[nw] and tally[2].
// stats (nullable, correct only) is added to as well.
struct NearestWant {
  int32_t* index;
  uint8_t* dist;
  uint64_t* counts;
  uint64_t* tally;
  uint64_t* stats;
};

// One pool block for every form, in 256-byte-aligned segments:
//   queries | quality rows packed to L bytes (L > 0) | index | dist | tail words
// The tail is what is read back in one copy: counts[nw], tally[2] and the error word of the tally
// when one is wanted, then the two statistics of correct (L > 0).
struct NearestLayout {
  size_t qual, index, dist, tail, total;             // byte offsets in the block (queries at 0)
  size_t counts = 0, tally, err, stats, tail_words;  // word offsets in the tail, and its length
  NearestLayout(int64_t nq, int L, bool tallied, int64_t nw) {
    const auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    qual = al((size_t)nq * 8);
    index = qual + al((size_t)nq * (size_t)L);
    dist = index + al((size_t)nq * 4);
    tail = dist + al((size_t)nq);
    tally = tallied ? (size_t)nw : 0;
    err = tally + (tallied ? 2 : 0);
    stats = err + (tallied ? 1 : 0);
    tail_words = stats + (L > 0 ? 2 : 0);
    total = tail + tail_words * 8;
  }
};

// One batch through the plan on the calling thread's stage and stream: one pool block, the copies
// in, the query or correct pass, the tally if wanted, the copies out, one synchronisation; the
// caller's arrays are touched only once every status is known.  nq == 0 is SCT_OK at once.  The
// caller has checked its pointers (tally and counts before anything, the others when nq > 0).
int nearest_host_batch(sct_nearest_plan* p, const NearestIn& in, const NearestWant& want);

}  // namespace sct
