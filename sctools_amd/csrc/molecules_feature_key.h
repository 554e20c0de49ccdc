// The feature counter's key arithmetic (include/sctools_hip.h, "counting molecules per feature"):
// pure functions shared by the kernels of molecules.hip, its host checks and the stand-alone host
// check program tests/host/molecules_feature_key_check.cpp.  A key is
// (((index << feat_bits) | feature) << umi_bits) | umi; molecules_key.h has the two-part key, the
// width rule of an index and the bad-UMI test, all of which hold here unchanged.
#pragma once

#include "molecules_key.h"

namespace sct {

// bits of a feature below nf: max(1, bit_length(nf - 1)), the rule of mol_idx_bits; nf >= 1
SCT_MOL_HD int mol_feat_bits(int64_t nf) { return mol_idx_bits(nf); }

// kind * L when (nw, nf, kind, L) is a legal feature counter, else 0: what mol_umi_bits asks of
// (nw, kind, L), 1 <= nf < 2^31, and idx_bits + feat_bits + kind * L <= 63 (the top bit stays 0)
SCT_MOL_HD int mol_feature_umi_bits(int64_t nw, int64_t nf, int kind, int L) {
  if (nf < 1 || nf >= (1LL << 31)) return 0;
  const int umi_bits = mol_umi_bits(nw, kind, L);
  if (umi_bits == 0) return 0;
  return mol_idx_bits(nw) + mol_feat_bits(nf) + umi_bits <= 63 ? umi_bits : 0;
}

// the key of 0 <= index < nw, 0 <= feature < nf and a good UMI
SCT_MOL_HD uint64_t mol_fkey(uint32_t index, uint32_t feature, uint64_t umi, int feat_bits, int umi_bits) {
  return ((((uint64_t)index << feat_bits) | (uint64_t)feature) << umi_bits) | umi;
}
SCT_MOL_HD uint32_t mol_fkey_index(uint64_t key, int feat_bits, int umi_bits) {
  return (uint32_t)(key >> (feat_bits + umi_bits));
}
SCT_MOL_HD uint32_t mol_fkey_feature(uint64_t key, int feat_bits, int umi_bits) {
  return (uint32_t)((key >> umi_bits) & ((1ull << feat_bits) - 1ull));
}
SCT_MOL_HD uint64_t mol_fkey_umi(uint64_t key, int umi_bits) { return mol_key_umi(key, umi_bits); }

// In the rows sorted by key, a row opens a matrix entry when its (index, feature) differs from the
// previous row's (row 0 always does; the caller says so).
SCT_MOL_HD bool mol_fkey_head(uint64_t key, uint64_t prev, int umi_bits) {
  return (key >> umi_bits) != (prev >> umi_bits);
}

}  // namespace sct
