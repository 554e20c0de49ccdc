// Stand-alone host check of sctools_amd/csrc/read_group_status.h (no HIP, no Python), built with
// AddressSanitizer and UBSan by tests/test_read_group_status_host.py.  It takes no input.
//   the precedence: every combination of index in {-3, -2, -1, 0, nw - 1, nw}, feature in {-3, -2, -1, 0,
//     nf - 1, nf}, with and without features, umi-bad, found and kept against the contract's list
//     written out as a chain of ifs, and the two-step form against the one-step form;
//   the slot word: pack and unpack of the extreme UMIs (0, all ones, one bit at either end) at the
//     extreme widths of both kinds -- one base, and the widest a 63-bit key leaves beside a one-bit
//     index -- with both values of the kept flag.
// Prints "ok <checks>".
#include <cstdint>
#include <cstdio>

#include "../../sctools_amd/csrc/read_group_status.h"

namespace {

long checks = 0;
int failed = 0;

void expect(bool ok, const char* what, long long a, long long b) {
  ++checks;
  if (ok) return;
  if (failed++ < 10) std::fprintf(stderr, "%s: %lld %lld\n", what, a, b);
}

// the contract's list, in its order
int by_the_list(int32_t index, int32_t feature, int64_t nw, int64_t nf, bool bad, bool found, bool kept) {
  if (index == -1) return 1;
  if (index == -2) return 2;
  if (index < -2 || index >= nw) return 7;
  if (nf != 0 && (feature < -2 || feature >= nf)) return 7;
  if (bad) return 3;
  if (nf != 0 && feature < 0) return 4;
  if (!found) return 5;
  if (!kept) return 6;
  return 0;
}

}  // namespace

int main() {
  const int64_t nws[] = {1, 5, (1LL << 31) - 1}, nfs[] = {0, 1, 6, (1LL << 31) - 1};
  for (int64_t nw : nws)
    for (int64_t nf : nfs) {
      const int64_t idx[] = {-3, -2, -1, 0, nw - 1, nw}, feat[] = {-3, -2, -1, 0, nf - 1, nf};
      for (int64_t i : idx)
        for (int64_t f : feat) {
          if (i > INT32_MAX || f > INT32_MAX || f < INT32_MIN) continue;
          for (int bits = 0; bits < 8; ++bits) {
            const bool bad = bits & 1, found = bits & 2, kept = bits & 4;
            const int want = by_the_list((int32_t)i, (int32_t)f, nw, nf, bad, found, kept);
            const int got = sct::read_group_status((int32_t)i, (int32_t)f, nw, nf, bad, found, kept);
            expect(got == want, "status", got, want);
            const int alone = sct::read_group_read_status((int32_t)i, (int32_t)f, nw, nf, bad);
            const int two = alone == sct::READ_LOOKUP ? sct::read_group_slot_status(found, kept) : alone;
            expect(two == want, "two steps", two, want);
          }
        }
    }
  // widths: kind * L for L = 1 and the largest L with 1 + kind * L <= 63
  const int widths[] = {2, 62, 3, 60};
  for (int w : widths) {
    const uint64_t all = (1ull << w) - 1ull;
    const uint64_t umis[] = {0, all, 1, 1ull << (w - 1), all >> 1, all & 0x5555555555555555ull};
    for (uint64_t u : umis)
      for (int kept = 0; kept < 2; ++kept) {
        const uint64_t word = sct::read_group_word(u, kept != 0);
        expect(sct::read_group_word_umi(word) == u, "umi", (long long)word, (long long)u);
        expect(sct::read_group_word_kept(word) == (kept != 0), "kept", (long long)word, kept);
        expect((word & ~sct::kReadGroupKept) == u, "the flag is the only other bit", (long long)word, (long long)u);
      }
  }
  if (failed) return 1;
  std::printf("ok %ld\n", checks);
  return 0;
}
