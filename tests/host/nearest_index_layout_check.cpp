// Stand-alone host check of sctools_amd/csrc/nearest_index_layout.h (no HIP, no Python): the
// arithmetic of the nearest index layouts as nearest.hip's builders call it.  Reads lines from stdin
// and prints one line per case (masks in hex, everything else decimal):
//   "scheme KIND BITS MAX_D NW FORCED"  the layouts a plan tries, in order: "3 1", "2", ...
//   "auto MIN_BASES NW"                 1 if keys of MIN_BASES bases are wide enough for NW codes
//   "halves KIND BITS NW"               GA GB pbits ndw index_bytes | offA offB entA entB packed rankB
//   "oa KIND BITS MAX_D NW"             "none", or P nkeys slots groups index_bytes a:b:keymask ... |
//                                       one offset per key table
//   "csr KIND BITS MAX_D NW LOAD OCC.." (max_d + 1 occupied counts) lg0 index_bytes
//                                       mask:lo_bit:nbits:mul:shift:buckets ... | off code index per part
// After the "|" come the segment offsets of the layout's device block, then "total BYTES touched T":
// a block of up to kTouchLimit bytes is allocated with malloc and the first and last byte of every
// segment written (T = 1), so an offset or a total that does not fit shows under AddressSanitizer.
// tests/test_nearest_index_layout_host.py compares these lines with tests/nearest_reference.py; the
// program is built with AddressSanitizer and UBSan.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../sctools_amd/csrc/nearest_index_layout.h"

namespace nix = sct::nearest_index;

namespace {

constexpr int64_t kTouchLimit = 4 << 20;

// prints the offsets and the total; touches [off[i], off[i + 1]) and [off[n - 1], total)
void carve(const int64_t* off, int n, int64_t total) {
  std::printf(" |");
  for (int i = 0; i < n; ++i) std::printf(" %" PRId64, off[i]);
  int touched = 0;
  if (total <= kTouchLimit) {
    char* block = static_cast<char*>(std::malloc((size_t)total));
    if (!block) std::abort();
    for (int i = 0; i < n; ++i) {
      const int64_t end = i + 1 < n ? off[i + 1] : total;
      block[off[i]] = (char)i;
      block[end - 1] = (char)i;
    }
    std::free(block);
    touched = 1;
  }
  std::printf(" total %" PRId64 " touched %d\n", total, touched);
}

}  // namespace

int main() {
  char what[16];
  long cases = 0;
  while (std::scanf("%15s", what) == 1) {
    int kind = 0, bits = 0, max_d = 0;
    long long nw = 0, x = 0;
    if (std::strcmp(what, "scheme") == 0 && std::scanf("%d %d %d %lld %lld", &kind, &bits, &max_d, &nw, &x) == 5) {
      const nix::Builders b = nix::builders(kind, bits, max_d, nw, x);
      for (int i = 0; i < b.n; ++i) std::printf(i ? " %d" : "%d", b.scheme[i]);
      std::printf("\n");
    } else if (std::strcmp(what, "auto") == 0 && std::scanf("%d %lld", &bits, &nw) == 2) {
      std::printf("%d\n", nix::oa_keys_wide_enough(bits, nw) ? 1 : 0);
    } else if (std::strcmp(what, "halves") == 0 && std::scanf("%d %d %lld", &kind, &bits, &nw) == 3) {
      const int G = nix::positions(kind, bits);
      const nix::HalvesDims d = nix::halves_dims(G, nw);
      const nix::HalvesBlock b = nix::halves_block(d, nw);
      std::printf("%d %d %d %" PRId64 " %" PRId64, d.GA, d.GB, d.pbits, d.ndw, nix::halves_index_bytes(G, nw));
      const int64_t off[6] = {b.offA, b.offB, b.entA, b.entB, b.packed, b.rankB};
      carve(off, 6, b.total);
    } else if (std::strcmp(what, "oa") == 0 && std::scanf("%d %d %d %lld", &kind, &bits, &max_d, &nw) == 4) {
      nix::OaLayout l;
      if (!nix::oa_layout(kind, bits, max_d, nw, &l)) {
        std::printf("none\n");
      } else {
        std::printf("%d %d %" PRId64 " %" PRId64 " %" PRId64, l.P, l.nkeys, l.slots, l.groups,
                    nix::oa_index_bytes(l.nkeys, l.slots));
        for (int t = 0; t < l.nkeys; ++t) std::printf(" %d:%d:%" PRIx64, l.a[t], l.b[t], l.keymask[t]);
        const nix::OaBlock b = nix::oa_block(l.nkeys, l.slots);
        carve(b.slots, l.nkeys, b.total);
      }
    } else if (std::strcmp(what, "csr") == 0 && std::scanf("%d %d %d %lld %lld", &kind, &bits, &max_d, &nw, &x) == 5) {
      const int G = nix::positions(kind, bits), P = max_d + 1, lg0 = nix::csr_lg0(nw);
      if (P > nix::kMaxParts) return 2;
      int64_t nbuckets[nix::kMaxParts], off[3 * nix::kMaxParts];
      nix::CsrPart part[nix::kMaxParts];
      for (int k = 0; k < P; ++k) {
        long long occ = 0;
        if (std::scanf("%lld", &occ) != 1) return 2;
        // (lg0 == 0, where the build counts nothing: csr_lg gives 0)
        part[k] = nix::csr_part(kind, G, P, k, nix::csr_lg(lg0, x, (uint64_t)occ));
        nbuckets[k] = part[k].buckets;
      }
      std::printf("%d %" PRId64, lg0, nix::csr_index_bytes(P, nbuckets, nw));
      for (int k = 0; k < P; ++k)
        std::printf(" %" PRIx64 ":%d:%d:%" PRIx64 ":%d:%" PRId64, part[k].mask, part[k].lo_bit, part[k].nbits,
                    part[k].mul, part[k].shift, nbuckets[k]);
      const nix::CsrBlock b = nix::csr_block(P, nbuckets, nw);
      for (int k = 0; k < P; ++k) off[3 * k] = b.off[k], off[3 * k + 1] = b.code[k], off[3 * k + 2] = b.index[k];
      carve(off, 3 * P, b.total);
    } else {
      std::printf("bad line\n");
      return 2;
    }
    ++cases;
  }
  std::printf("ok %ld limits %d %d %d\n", cases, nix::kMaxParts, nix::kMaxKeys, nix::kGroup);
  return 0;
}
