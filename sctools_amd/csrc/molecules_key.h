// The molecule counter's key arithmetic (include/sctools_hip.h, "counting molecules"): pure
// functions shared by the kernels of molecules.hip, its host checks and the stand-alone host
// check program tests/host/molecules_key_check.cpp.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define SCT_MOL_HD __host__ __device__ __forceinline__
#else
#define SCT_MOL_HD inline
#endif

namespace sct {

// bits of a whitelist index below nw: max(1, bit_length(nw - 1)); nw >= 1
SCT_MOL_HD int mol_idx_bits(int64_t nw) {
  int b = 1;
  while (b < 63 && ((nw - 1) >> b) != 0) ++b;
  return b;
}

// kind * L when (nw, kind, L) is a legal counter, else 0: 1 <= nw < 2^31, kind 2 or 3,
// 1 <= kind * L and idx_bits + kind * L <= 63 (a key's top bit is then always 0)
SCT_MOL_HD int mol_umi_bits(int64_t nw, int kind, int L) {
  if (nw < 1 || nw >= (1LL << 31) || (kind != 2 && kind != 3) || L < 1 || L > 31) return 0;
  const int umi_bits = kind * L;
  return mol_idx_bits(nw) + umi_bits <= 63 ? umi_bits : 0;
}

// (index << umi_bits) | umi for 0 <= index < nw and a good UMI
SCT_MOL_HD uint64_t mol_key(uint32_t index, uint64_t umi, int umi_bits) {
  return ((uint64_t)index << umi_bits) | umi;
}
SCT_MOL_HD uint32_t mol_key_index(uint64_t key, int umi_bits) { return (uint32_t)(key >> umi_bits); }
SCT_MOL_HD uint64_t mol_key_umi(uint64_t key, int umi_bits) { return key & ((1ull << umi_bits) - 1ull); }

// A UMI is bad when it has a bit at or above umi_bits (1 <= umi_bits <= 62) or, for kind 3, when
// one of its umi_bits / 3 triplets is not C 1, A 2, G 3 or T 4.  With b2 b1 b0 the bits of a
// triplet, it is one of 1..4 exactly when b2 != (b1 | b0): 0 and 5, 6 (N), 7 fail.  The test
// runs on every triplet of the word at once, bit 0 of each triplet carrying its answer.
SCT_MOL_HD bool mol_umi_bad(uint64_t umi, int kind, int umi_bits) {
  if ((umi >> umi_bits) != 0) return true;
  if (kind != 3) return false;
  const uint64_t ones = 0x1249249249249249ull & ((1ull << umi_bits) - 1ull);  // bit 0 of every triplet
  const uint64_t good = ((umi >> 2) ^ ((umi >> 1) | umi)) & ones;
  return good != ones;
}

}  // namespace sct
