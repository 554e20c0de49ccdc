// Stand-alone host check of sctools_amd/csrc/molecules_resolve_key.h (no HIP, no Python): reads one
// command per line from stdin and prints one answer line for each.
//   word  nw nf kind L index feature image -> word index' feature' image' (the word packed and taken apart)
//   of    nw nf kind L index feature umi image -> the word made from the key and the image's key
//   heads feat_bits word prev              -> group-head molecule-head (1 or 0 each)
//   fold  n r1 .. rn                       -> top at_top members reads unique, folded left to right from the unit
//   split n k r1 .. rn                     -> the same from combine(fold(r1..rk), fold(rk+1..rn))
// Numbers are decimal (words unsigned).  tests/test_molecules_resolve_key_host.py holds the answers
// against tests/feature_resolve_reference.py; the program is built with AddressSanitizer and UBSan.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sctools_amd/csrc/molecules_resolve_key.h"

namespace {

sct::ResolveGroup fold(const std::vector<uint64_t>& r, size_t from, size_t to) {
  sct::ResolveGroup g{0, 0, 0, 0};
  for (size_t i = from; i < to; ++i) g = sct::mol_resolve_combine(g, sct::mol_resolve_member(r[i]));
  return g;
}

void print(const sct::ResolveGroup& g) {
  std::printf("%" PRIu64 " %" PRIu32 " %" PRIu64 " %" PRIu64 " %d\n", g.top, g.at_top, g.members, g.reads,
              sct::mol_resolve_unique(g) ? 1 : 0);
}

bool read_reads(long n, std::vector<uint64_t>* r) {
  for (long i = 0; i < n; ++i) {
    uint64_t v = 0;
    if (std::scanf("%" SCNu64, &v) != 1) return false;
    r->push_back(v);
  }
  return true;
}

}  // namespace

int main() {
  char cmd[16];
  long cases = 0;
  while (std::scanf("%15s", cmd) == 1) {
    if (!std::strcmp(cmd, "word") || !std::strcmp(cmd, "of")) {
      const bool of = cmd[0] == 'o';
      long long nw = 0, nf = 0;
      int kind = 0, L = 0;
      uint32_t index = 0, feature = 0;
      uint64_t umi = 0, image = 0;
      if (std::scanf("%lld %lld %d %d %" SCNu32 " %" SCNu32, &nw, &nf, &kind, &L, &index, &feature) != 6) return 2;
      if (of && std::scanf("%" SCNu64, &umi) != 1) return 2;
      if (std::scanf("%" SCNu64, &image) != 1) return 2;
      const int umi_bits = sct::mol_feature_umi_bits(nw, nf, kind, L), fb = sct::mol_feat_bits(nf);
      if (umi_bits == 0) return 3;
      const uint64_t word = of ? sct::mol_resolve_word_of(sct::mol_fkey(index, feature, umi, fb, umi_bits),
                                                          sct::mol_fkey(index, feature, image, fb, umi_bits), fb, umi_bits)
                               : sct::mol_resolve_word(index, feature, image, fb, umi_bits);
      std::printf("%" PRIu64 " %" PRIu32 " %" PRIu32 " %" PRIu64 "\n", word, sct::mol_resolve_index(word, fb, umi_bits),
                  sct::mol_resolve_feature(word, fb), sct::mol_resolve_image(word, fb, umi_bits));
    } else if (!std::strcmp(cmd, "heads")) {
      int fb = 0;
      uint64_t word = 0, prev = 0;
      if (std::scanf("%d %" SCNu64 " %" SCNu64, &fb, &word, &prev) != 3) return 2;
      std::printf("%d %d\n", sct::mol_resolve_group_head(word, prev, fb) ? 1 : 0,
                  sct::mol_resolve_molecule_head(word, prev) ? 1 : 0);
    } else if (!std::strcmp(cmd, "fold")) {
      long n = 0;
      std::vector<uint64_t> r;
      if (std::scanf("%ld", &n) != 1 || n < 0 || !read_reads(n, &r)) return 2;
      print(fold(r, 0, r.size()));
    } else if (!std::strcmp(cmd, "split")) {
      long n = 0, k = 0;
      std::vector<uint64_t> r;
      if (std::scanf("%ld %ld", &n, &k) != 2 || n < 0 || k < 0 || k > n || !read_reads(n, &r)) return 2;
      print(sct::mol_resolve_combine(fold(r, 0, (size_t)k), fold(r, (size_t)k, r.size())));
    } else {
      return 2;
    }
    ++cases;
  }
  std::printf("ok %ld\n", cases);
  return 0;
}
