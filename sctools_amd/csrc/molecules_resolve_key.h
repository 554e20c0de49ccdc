// Resolving features (include/sctools_hip.h, "resolving features"): the pure functions shared by the
// kernels of molecules.hip and the stand-alone host check program
// tests/host/molecules_resolve_key_check.cpp.
//
// The sort word of a stored key (index, feature, umi) whose image is `image_umi` is
// (((index << umi_bits) | image_umi) << feat_bits) | feature: the key's own three parts in another
// order, so it is as wide as the key (idx_bits + feat_bits + umi_bits <= 63) and ascending word order
// is (index, image, feature) order.  A group's rows -- one (index, image umi) over all features -- are
// therefore adjacent, ordered by feature, and the rows of one collapsed molecule carry one word.
#pragma once

#include "molecules_feature_key.h"

namespace sct {

SCT_MOL_HD uint64_t mol_resolve_word(uint32_t index, uint32_t feature, uint64_t image_umi, int feat_bits,
                                     int umi_bits) {
  return ((((uint64_t)index << umi_bits) | image_umi) << feat_bits) | (uint64_t)feature;
}
// the same from a stored key and the key of its image (which shares index and feature with it)
SCT_MOL_HD uint64_t mol_resolve_word_of(uint64_t key, uint64_t image_key, int feat_bits, int umi_bits) {
  return mol_resolve_word(mol_fkey_index(key, feat_bits, umi_bits), mol_fkey_feature(key, feat_bits, umi_bits),
                          mol_fkey_umi(image_key, umi_bits), feat_bits, umi_bits);
}
SCT_MOL_HD uint32_t mol_resolve_index(uint64_t word, int feat_bits, int umi_bits) {
  return (uint32_t)(word >> (feat_bits + umi_bits));
}
SCT_MOL_HD uint32_t mol_resolve_feature(uint64_t word, int feat_bits) {
  return (uint32_t)(word & ((1ull << feat_bits) - 1ull));
}
SCT_MOL_HD uint64_t mol_resolve_image(uint64_t word, int feat_bits, int umi_bits) {
  return (word >> feat_bits) & ((1ull << umi_bits) - 1ull);
}

// In the rows sorted by word (row 0 opens both; the caller says so): a group opens when
// (index, image) differs from the previous row's, a collapsed molecule when the word does.
SCT_MOL_HD bool mol_resolve_group_head(uint64_t word, uint64_t prev, int feat_bits) {
  return (word >> feat_bits) != (prev >> feat_bits);
}
SCT_MOL_HD bool mol_resolve_molecule_head(uint64_t word, uint64_t prev) { return word != prev; }

// What a run of a group's collapsed molecules folds to: the largest reads among them, how many have
// it (capped at 2: one or more than one is all the rule asks), the members and the sum of their
// reads.  The combine is associative and commutative with the empty run {0, 0, 0, 0} as its unit, so
// a walk along the rows and a reduction across lanes share one rule.
struct ResolveGroup {
  uint64_t top;
  uint32_t at_top;
  uint64_t members, reads;
};
SCT_MOL_HD ResolveGroup mol_resolve_member(uint64_t reads) { return ResolveGroup{reads, 1u, 1ull, reads}; }
SCT_MOL_HD ResolveGroup mol_resolve_combine(const ResolveGroup& a, const ResolveGroup& b) {
  const uint32_t both = a.at_top + b.at_top;
  return ResolveGroup{a.top > b.top ? a.top : b.top,
                      a.top == b.top ? (both > 2u ? 2u : both) : (a.top > b.top ? a.at_top : b.at_top),
                      a.members + b.members, a.reads + b.reads};
}
// the group's verdict: a unique winner keeps its molecule, anything else ties every member
SCT_MOL_HD bool mol_resolve_unique(const ResolveGroup& g) { return g.at_top == 1u; }

}  // namespace sct
