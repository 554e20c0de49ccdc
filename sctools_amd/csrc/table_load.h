// The load rule of the open-addressing tables (open_table.h): their limits and the policy by which a
// batch is fed, as pure host functions shared by count.hip, molecules.hip, molecules_merge_plan.h and
// the stand-alone host check program tests/host/table_load_check.cpp.
//
// A batch goes in as sub-batches of at most capacity / 4 items.  The host tracks an upper bound of
// the claimed slots (the last size it read plus the items fed since) and reads the device's size
// word whenever the bound passes capacity / 2; a true size above capacity / 2 grows the table, x4
// while more than capacity / 2 items of the batch remain, else x2.  A launch therefore starts at a
// true size of at most capacity / 2 and adds at most capacity / 4: the load never passes 3/4, and a
// probe, which is bounded by the capacity anyway, always finds an empty slot.
#pragma once

#include <stdint.h>

namespace sct {

constexpr int64_t kTableMinCapacity = 64;
constexpr int64_t kTableMaxCapacity = 1LL << 31;  // slot numbers are uint32 in the fetches

// the smallest power of two at or above the hint, at least kTableMinCapacity; 0 <= hint <= 2^31
inline int64_t table_capacity_for(int64_t hint) {
  int64_t cap = kTableMinCapacity;
  while (cap < hint) cap *= 2;
  return cap;
}

inline int64_t table_sub_batch(int64_t remaining, int64_t capacity) {
  return remaining < capacity / 4 ? remaining : capacity / 4;
}

// the bound of claimed slots no longer shows that the next sub-batch fits: read the size word
inline bool table_size_due(int64_t size_bound, int64_t capacity) { return size_bound > capacity / 2; }

inline int64_t table_growth_factor(int64_t remaining, int64_t capacity) { return remaining > capacity / 2 ? 4 : 2; }

// capacity * factor, or 0 when that would pass kTableMaxCapacity (the growth is refused)
inline int64_t table_grown(int64_t capacity, int64_t factor) {
  return capacity * factor <= kTableMaxCapacity ? capacity * factor : 0;
}

// The feed loop over n items.  read_size() makes size_bound the true size; grow(factor) changes the
// capacity or fails; launch(done, m) enqueues the items [done, done + m).  Each returns 0 or the
// status the loop stops with.
template <class ReadSize, class Grow, class Launch>
int table_feed(int64_t n, const int64_t& capacity, int64_t& size_bound, ReadSize read_size, Grow grow, Launch launch) {
  int64_t done = 0;
  while (done < n) {
    if (table_size_due(size_bound, capacity)) {
      if (int rc = read_size(); rc != 0) return rc;
      if (table_size_due(size_bound, capacity)) {
        if (int rc = grow(table_growth_factor(n - done, capacity)); rc != 0) return rc;
        continue;
      }
    }
    const int64_t m = table_sub_batch(n - done, capacity);
    if (int rc = launch(done, m); rc != 0) return rc;
    size_bound += m;
    done += m;
  }
  return 0;
}

}  // namespace sct
