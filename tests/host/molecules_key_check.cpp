// Stand-alone host check of sctools_amd/csrc/molecules_key.h (no HIP, no Python): reads cases
// "nw kind L index umi" (decimal, one per line) from stdin and prints, per case,
// "umi_bits idx_bits bad key index_back umi_back": umi_bits is 0 for an illegal (nw, kind, L), and
// the key with its two halves taken apart again is printed for legal counters and good UMIs only
// (0 0 0 otherwise).  tests/test_molecules_key_host.py compares the lines with
// tests/molecules_reference.py; the program is built with AddressSanitizer and UBSan.
#include <cinttypes>
#include <cstdio>

#include "../../sctools_amd/csrc/molecules_key.h"

int main() {
  long long nw = 0;
  int kind = 0, L = 0;
  unsigned index = 0;
  unsigned long long umi = 0;
  long cases = 0;
  while (std::scanf("%lld %d %d %u %llu", &nw, &kind, &L, &index, &umi) == 5) {
    const int umi_bits = sct::mol_umi_bits(nw, kind, L);
    if (umi_bits == 0) {
      std::printf("0 0 0 0 0 0\n");
      ++cases;
      continue;
    }
    const bool bad = sct::mol_umi_bad(umi, kind, umi_bits);
    uint64_t key = 0, back_umi = 0;
    uint32_t back_index = 0;
    if (!bad) {
      key = sct::mol_key(index, umi, umi_bits);
      back_index = sct::mol_key_index(key, umi_bits);
      back_umi = sct::mol_key_umi(key, umi_bits);
    }
    std::printf("%d %d %d %" PRIu64 " %" PRIu32 " %" PRIu64 "\n", umi_bits, sct::mol_idx_bits(nw), bad ? 1 : 0, key,
                back_index, back_umi);
    ++cases;
  }
  std::printf("ok %ld\n", cases);
  return 0;
}
