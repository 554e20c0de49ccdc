// Stand-alone host check of sctools_amd/csrc/molecules_merge_plan.h (no HIP, no Python): reads cases
// "dst_capacity dst_size src_size" (decimal, one per line) from stdin and prints, per case, the
// capacity sct_molecules_merge grows the target to before any key moves, 0 when the merged table
// does not fit 2^31 slots.  tests/test_molecules_merge_plan_host.py asserts the contract's bounds
// on the lines; the program is built with AddressSanitizer and UBSan.
#include <cinttypes>
#include <cstdio>

#include "../../sctools_amd/csrc/molecules_merge_plan.h"

int main() {
  long long cap = 0, dst_size = 0, src_size = 0;
  long cases = 0;
  while (std::scanf("%lld %lld %lld", &cap, &dst_size, &src_size) == 3) {
    std::printf("%" PRId64 "\n", sct::mol_merge_capacity(cap, dst_size, src_size));
    ++cases;
  }
  std::printf("ok %ld limits %" PRId64 " %" PRId64 "\n", cases, sct::kMolMinCapacity, sct::kMolMaxCapacity);
  return 0;
}
