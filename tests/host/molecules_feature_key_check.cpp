// Stand-alone host check of sctools_amd/csrc/molecules_feature_key.h (no HIP, no Python): reads one
// command per line from stdin and prints one answer line for each.
//   bits  nf                               -> feat_bits
//   legal nw nf kind L                     -> umi_bits of a legal feature counter, else 0
//   pack  nw nf kind L index feature umi   -> key index' feature' umi' (the key packed and taken apart)
//   head  umi_bits key prev                -> 1 when key opens an entry after prev, else 0
// Numbers are decimal (keys and UMIs unsigned).  tests/test_molecules_feature_key_host.py holds the
// answers against tests/count_matrix_reference.py; the program is built with AddressSanitizer and UBSan.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../sctools_amd/csrc/molecules_feature_key.h"

int main() {
  char cmd[16];
  long cases = 0;
  while (std::scanf("%15s", cmd) == 1) {
    if (!std::strcmp(cmd, "bits")) {
      long long nf = 0;
      if (std::scanf("%lld", &nf) != 1) return 2;
      std::printf("%d\n", sct::mol_feat_bits(nf));
    } else if (!std::strcmp(cmd, "legal")) {
      long long nw = 0, nf = 0;
      int kind = 0, L = 0;
      if (std::scanf("%lld %lld %d %d", &nw, &nf, &kind, &L) != 4) return 2;
      std::printf("%d\n", sct::mol_feature_umi_bits(nw, nf, kind, L));
    } else if (!std::strcmp(cmd, "pack")) {
      long long nw = 0, nf = 0;
      int kind = 0, L = 0;
      uint32_t index = 0, feature = 0;
      uint64_t umi = 0;
      if (std::scanf("%lld %lld %d %d %" SCNu32 " %" SCNu32 " %" SCNu64, &nw, &nf, &kind, &L, &index, &feature, &umi) != 7)
        return 2;
      const int umi_bits = sct::mol_feature_umi_bits(nw, nf, kind, L), fb = sct::mol_feat_bits(nf);
      if (umi_bits == 0) return 3;
      const uint64_t key = sct::mol_fkey(index, feature, umi, fb, umi_bits);
      std::printf("%" PRIu64 " %" PRIu32 " %" PRIu32 " %" PRIu64 "\n", key, sct::mol_fkey_index(key, fb, umi_bits),
                  sct::mol_fkey_feature(key, fb, umi_bits), sct::mol_fkey_umi(key, umi_bits));
    } else if (!std::strcmp(cmd, "head")) {
      int umi_bits = 0;
      uint64_t key = 0, prev = 0;
      if (std::scanf("%d %" SCNu64 " %" SCNu64, &umi_bits, &key, &prev) != 3) return 2;
      std::printf("%d\n", sct::mol_fkey_head(key, prev, umi_bits) ? 1 : 0);
    } else {
      return 2;
    }
    ++cases;
  }
  std::printf("ok %ld\n", cases);
  return 0;
}
