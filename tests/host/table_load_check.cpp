// Stand-alone host check of sctools_amd/csrc/table_load.h (no HIP, no Python): the feed loop both
// counters run, over a simulated table.  Reads lines from stdin:
//   "cap HINT"              prints the capacity a counter is created with for that hint
//   "grown CAPACITY FACTOR" prints the capacity a growth reaches, 0 when it is refused
//   "feed HINT N PPM"       feeds N items to a table created for HINT; of every sub-batch,
//                           ceil(m * PPM / 10^6) items are new keys (PPM 10^6: pairwise distinct), and at
//                           least one while the table is empty (PPM 0: N copies of one item)
// A feed prints one line: "feed" and then, in order, an event per step of the loop -- "r" the size
// word was read, "g<capacity>" the table grew to that capacity, "l<capacity>:<size>" a sub-batch was
// launched into that capacity and <size> slots were claimed when it ended -- and last " max
// <size>/<capacity>", the largest share of its capacity a table held at the end of any launch, and
// " end <capacity> <status>".  tests/test_table_load_host.py asserts the load rule on these lines; the
// program is built with AddressSanitizer and UBSan.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../sctools_amd/csrc/table_load.h"

namespace {

int feed(int64_t hint, int64_t n, int64_t ppm) {
  int64_t capacity = sct::table_capacity_for(hint);
  int64_t size_bound = 0;  // the host's bound
  int64_t size = 0;        // the device's size word
  int64_t max_size = 0, max_capacity = capacity;
  std::printf("feed");
  const int rc = sct::table_feed(
      n, capacity, size_bound,
      [&] {
        std::printf(" r");
        size_bound = size;
        return 0;
      },
      [&](int64_t factor) {
        const int64_t cap = sct::table_grown(capacity, factor);
        if (cap == 0) return 1;
        capacity = cap;
        std::printf(" g%" PRId64, capacity);
        return 0;
      },
      [&](int64_t, int64_t m) {
        int64_t fresh = (m * ppm + 999999) / 1000000;
        if (size == 0 && fresh == 0) fresh = 1;
        size += fresh;
        std::printf(" l%" PRId64 ":%" PRId64, capacity, size);
        if (size * max_capacity > max_size * capacity) max_size = size, max_capacity = capacity;  // both below 2^32
        return 0;
      });
  std::printf(" max %" PRId64 "/%" PRId64 " end %" PRId64 " %d\n", max_size, max_capacity, capacity, rc);
  return rc;
}

}  // namespace

int main() {
  char what[16];
  long cases = 0;
  while (std::scanf("%15s", what) == 1) {
    long long a = 0, b = 0, c = 0;
    if (std::strcmp(what, "cap") == 0 && std::scanf("%lld", &a) == 1) {
      std::printf("%" PRId64 "\n", sct::table_capacity_for(a));
    } else if (std::strcmp(what, "grown") == 0 && std::scanf("%lld %lld", &a, &b) == 2) {
      std::printf("%" PRId64 "\n", sct::table_grown(a, b));
    } else if (std::strcmp(what, "feed") == 0 && std::scanf("%lld %lld %lld", &a, &b, &c) == 3) {
      (void)feed(a, b, c);
    } else {
      std::printf("bad line\n");
      return 2;
    }
    ++cases;
  }
  std::printf("ok %ld limits %" PRId64 " %" PRId64 "\n", cases, sct::kTableMinCapacity, sct::kTableMaxCapacity);
  return 0;
}
