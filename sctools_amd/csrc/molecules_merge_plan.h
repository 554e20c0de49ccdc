// The growth target of sct_molecules_merge (include/sctools_hip.h, "merging molecule counters"): a
// pure function shared by molecules.hip and the stand-alone host check program
// tests/host/molecules_merge_plan_check.cpp.
#pragma once

#include <stdint.h>

#include "molecules_key.h"
#include "table_load.h"

namespace sct {

constexpr int64_t kMolMinCapacity = kTableMinCapacity;
constexpr int64_t kMolMaxCapacity = kTableMaxCapacity;

// The capacity `dst` must have before the keys of `src` move into it: the smallest power of two that
// is no smaller than dst_capacity and holds dst_size + src_size keys at a load of at most 1/2 (every
// key of src may be new to dst).  0 = does not fit: that would take more than 2^31 slots.
// dst_capacity is a power of two in [64, 2^31]; the sizes are >= 0 and at most 2^31 each.
SCT_MOL_HD int64_t mol_merge_capacity(int64_t dst_capacity, int64_t dst_size, int64_t src_size) {
  const int64_t keys = dst_size + src_size;
  if (keys > kMolMaxCapacity / 2) return 0;
  int64_t cap = dst_capacity;
  while (cap / 2 < keys) cap *= 2;
  return cap;
}

}  // namespace sct
