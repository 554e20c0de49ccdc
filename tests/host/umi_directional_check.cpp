// Stand-alone host check of sctools_amd/csrc/umi_directional.h (no HIP, no Python): reads cases
// "u_reads v_reads a_reads a_code b_reads b_code" (decimal, one per line) from stdin and prints, per
// case, the edge test u -> v, the label order (a_reads, a_code) < (b_reads, b_code) and
// umi_support_less of the same four numbers, each as 0 / 1.
// tests/test_umi_directional_host.py compares the lines with the big-integer statements of
// tests/umi_directional_reference.py; the program is built with AddressSanitizer and UBSan.
#include <cstdio>

#include "../../sctools_amd/csrc/umi_directional.h"

int main() {
  unsigned long long u = 0, v = 0, a_reads = 0, a_code = 0, b_reads = 0, b_code = 0;
  long cases = 0;
  while (std::scanf("%llu %llu %llu %llu %llu %llu", &u, &v, &a_reads, &a_code, &b_reads, &b_code) == 6) {
    if (u == 0 || v == 0) {  // a stored molecule has at least one read
      std::printf("bad case\n");
      return 1;
    }
    std::printf("%d %d %d\n", sct::umi_directional_edge(u, v) ? 1 : 0,
                sct::umi_label_less(a_reads, a_code, b_reads, b_code) ? 1 : 0,
                sct::umi_support_less(a_reads, a_code, b_reads, b_code) ? 1 : 0);
    ++cases;
  }
  std::printf("ok %ld\n", cases);
  return 0;
}
