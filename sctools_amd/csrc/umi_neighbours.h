// The UMI collapse's neighbour arithmetic (include/sctools_hip.h, "collapsing UMIs one base apart"):
// pure functions shared by the collapse and fetch kernels of molecules.hip and the stand-alone
// host check program tests/host/umi_neighbours_check.cpp.
#pragma once

#include <stdint.h>

#include "molecules_key.h"

namespace sct {

// The j-th of the 3 * L codes one base away from `code`, 0 <= j < 3 * L: base position j / 3
// (position 0 = the low digit, the last base) carries the (j % 3 + 1)-th next of the four bases,
// cyclically.  kind 2: digit d of 0..3 -> (d + 1 + j % 3) & 3.  kind 3: triplet t of 1..4 (a good
// UMI has no other) -> ((t - 1) + 1 + j % 3) & 3, plus 1: never N, never an invalid triplet.
// The change is an XOR inside the position's own bits, so nothing carries: `code` may be a whole
// key, whose index bits stay as they are.
SCT_MOL_HD uint64_t umi_neighbour(uint64_t code, int kind, int j) {
  const int shift = kind * (j / 3);
  const uint64_t one = kind == 3 ? 1u : 0u;
  const uint64_t field = kind == 3 ? 7u : 3u;
  const uint64_t d = (code >> shift) & field;
  const uint64_t nb = (((d - one) + 1u + (uint64_t)(j % 3)) & 3u) + one;
  return code ^ ((d ^ nb) << shift);
}

// (a_reads, a_code) < (b_reads, b_code): by reads, and by code on equal reads
SCT_MOL_HD bool umi_support_less(uint64_t a_reads, uint64_t a_code, uint64_t b_reads, uint64_t b_code) {
  return a_reads < b_reads || (a_reads == b_reads && a_code < b_code);
}

}  // namespace sct
