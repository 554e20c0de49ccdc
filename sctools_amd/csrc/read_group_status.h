// Read groups (include/sctools_hip.h, "read groups"): the pure functions shared by the tag kernels of
// molecules.hip and the stand-alone host check program tests/host/read_group_status_check.cpp.
//
// The status of a read is decided in two steps, because the second needs a probe of the snapshot's
// keys and the first says whether the probe is made at all: read_group_read_status() from the read
// alone, then read_group_slot_status() from what the probe found.  read_group_status() is the two in
// one, the contract's order of precedence.
//
// The per-slot word of a snapshot: the final UMI of the slot's key (its image's UMI) in the low
// umi_bits <= 62 bits and, in bit 63, whether the final molecule is kept.  A UMI never reaches bit 63,
// so the flag is spare at every legal width.
#pragma once

#include "molecules_key.h"

namespace sct {

// the numbers of include/sctools_hip.h's SCT_READ_* (kept equal by a static_assert in molecules.hip)
enum {
  READ_GROUPED = 0,
  READ_NO_BARCODE = 1,
  READ_AMBIGUOUS = 2,
  READ_BAD_UMI = 3,
  READ_NO_FEATURE = 4,
  READ_ABSENT = 5,
  READ_LOST = 6,
  READ_BAD_INDEX = 7,
  READ_NSTATUS = 8,
  READ_LOOKUP = -1  // read_group_read_status: the read has a key, the snapshot decides
};

// Rules 1..5: the read by itself.  nf == 0: a snapshot without features, `feature` is not looked at.
SCT_MOL_HD int read_group_read_status(int32_t index, int32_t feature, int64_t nw, int64_t nf, bool umi_bad) {
  if (index == -1) return READ_NO_BARCODE;
  if (index == -2) return READ_AMBIGUOUS;
  if (index < 0 || (int64_t)index >= nw) return READ_BAD_INDEX;
  if (nf != 0 && (feature < -2 || (int64_t)feature >= nf)) return READ_BAD_INDEX;
  if (umi_bad) return READ_BAD_UMI;
  if (nf != 0 && feature < 0) return READ_NO_FEATURE;
  return READ_LOOKUP;
}

// Rules 6..8: what the probe of the snapshot says (`kept` is the slot word's flag, and always set in a
// snapshot that is not resolved).
SCT_MOL_HD int read_group_slot_status(bool found, bool kept) {
  return !found ? READ_ABSENT : kept ? READ_GROUPED : READ_LOST;
}

SCT_MOL_HD int read_group_status(int32_t index, int32_t feature, int64_t nw, int64_t nf, bool umi_bad, bool found,
                                 bool kept) {
  const int s = read_group_read_status(index, feature, nw, nf, umi_bad);
  return s == READ_LOOKUP ? read_group_slot_status(found, kept) : s;
}

constexpr uint64_t kReadGroupKept = 1ull << 63;

SCT_MOL_HD uint64_t read_group_word(uint64_t final_umi, bool kept) { return final_umi | (kept ? kReadGroupKept : 0); }
SCT_MOL_HD uint64_t read_group_word_umi(uint64_t word) { return word & ~kReadGroupKept; }
SCT_MOL_HD bool read_group_word_kept(uint64_t word) { return (word & kReadGroupKept) != 0; }

}  // namespace sct
