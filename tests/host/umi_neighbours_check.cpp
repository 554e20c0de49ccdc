// Stand-alone host check of sctools_amd/csrc/umi_neighbours.h (no HIP, no Python): reads cases
// "kind L code a_reads b_reads b_code" (decimal, one per line) from stdin and prints, per case, the
// 3 * L neighbours of `code` in the header's order j = 0 .. 3 * L - 1 and then the order predicate
// (a_reads, code) < (b_reads, b_code) as 0 / 1.  `code` may be a whole key: the neighbours then keep
// its index bits.  tests/test_umi_neighbours_host.py compares the lines with
// tests/umi_collapse_reference.py; the program is built with AddressSanitizer and UBSan.
#include <cinttypes>
#include <cstdio>

#include "../../sctools_amd/csrc/umi_neighbours.h"

int main() {
  int kind = 0, L = 0;
  unsigned long long code = 0, a_reads = 0, b_reads = 0, b_code = 0;
  long cases = 0;
  while (std::scanf("%d %d %llu %llu %llu %llu", &kind, &L, &code, &a_reads, &b_reads, &b_code) == 6) {
    if ((kind != 2 && kind != 3) || L < 1 || kind * L > 62) {
      std::printf("bad case\n");
      return 1;
    }
    for (int j = 0; j < 3 * L; ++j) std::printf("%" PRIu64 " ", sct::umi_neighbour(code, kind, j));
    std::printf("%d\n", sct::umi_support_less(a_reads, code, b_reads, b_code) ? 1 : 0);
    ++cases;
  }
  std::printf("ok %ld\n", cases);
  return 0;
}
