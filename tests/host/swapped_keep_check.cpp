// Stand-alone host check of sctools_amd/csrc/swapped_keep.h (no HIP, no Python): reads cases from
// stdin, one per line, and prints one line per case:
//   k r others num den          whether swapped_keeps(r, others, num, den)
//   a x y                       the saturating sum of x and y
//   p s num den                 whether swapped_params_ok(s, num, den); s is signed
//   m s num den r[0..s)         how many of the s samples keep a molecule they hold r[t] reads of
// (all other numbers decimal, unsigned 64-bit).  tests/test_swapped_keep_host.py compares the lines with
// tests/swapped_reference.py; the program is built with AddressSanitizer and UBSan.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../sctools_amd/csrc/swapped_keep.h"

static bool number(uint64_t* v) {
  unsigned long long x = 0;
  if (std::scanf("%llu", &x) != 1) return false;
  *v = x;
  return true;
}

int main() {
  char what = 0;
  long cases = 0;
  while (std::scanf(" %c", &what) == 1) {
    uint64_t a = 0, b = 0, c = 0, d = 0;
    long long s = 0;
    if (what == 'k') {
      if (!number(&a) || !number(&b) || !number(&c) || !number(&d)) return 1;
      std::printf("%d\n", sct::swapped_keeps(a, b, c, d) ? 1 : 0);
    } else if (what == 'a') {
      if (!number(&a) || !number(&b)) return 1;
      std::printf("%" PRIu64 "\n", sct::swapped_add_sat(a, b));
    } else if (what == 'p') {
      if (std::scanf("%lld", &s) != 1 || !number(&a) || !number(&b)) return 1;
      std::printf("%d\n", sct::swapped_params_ok((int64_t)s, a, b) ? 1 : 0);
    } else if (what == 'm') {
      if (std::scanf("%lld", &s) != 1 || !number(&a) || !number(&b)) return 1;
      if (!sct::swapped_params_ok((int64_t)s, a, b)) return 1;
      std::vector<uint64_t> r((size_t)s);
      for (uint64_t& x : r)
        if (!number(&x)) return 1;
      int keepers = 0;
      for (size_t k = 0; k < r.size(); ++k) {
        uint64_t others = 0;
        for (size_t t = 0; t < r.size(); ++t)
          if (t != k) others = sct::swapped_add_sat(others, r[t]);
        keepers += sct::swapped_keeps(r[k], others, a, b) ? 1 : 0;
      }
      std::printf("%d\n", keepers);
    } else {
      std::printf("bad case\n");
      return 1;
    }
    ++cases;
  }
  std::printf("ok %ld\n", cases);
  return 0;
}
