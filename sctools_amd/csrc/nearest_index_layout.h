// The arithmetic of the nearest-whitelist index layouts (nearest.hip), once: which layouts a plan
// tries, how the base positions split into blocks, the sizes of the half-key, open-addressing and CSR
// tables, the one device block each layout lives in, and the bytes sct_nearest_plan_info reports.
// Pure host functions shared by nearest.hip's builders and the stand-alone host check program
// tests/host/nearest_index_layout_check.cpp.  (sct::NearestLayout in nearest_host.h is something
// else: the staging block of the *_host calls.)
#pragma once

#include <stdint.h>

namespace sct {
namespace nearest_index {

constexpr int kMaxParts = 8;  // CSR blocks: max_d + 1
constexpr int kMaxKeys = 6;   // open-addressing keys: C(4, 2) pairs at max_d = 2
constexpr int kGroup = 4;     // open-addressing slots per 64-byte group
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;  // the CSR buckets' multiplicative hash
enum Scheme { kAuto = 0, kOa = 1, kCsr = 2, kHalves = 3 };  // SCT_NEAREST_* / SCT_TUNE_NEAREST_SCHEME

inline int64_t at_least(int64_t x, int64_t lo) { return x < lo ? lo : x; }

// ---------------------------------------------------------------- positions and blocks
inline int positions(int kind, int code_bits) { return (code_bits + kind - 1) / kind; }

struct Block {
  int lo_bit, nbits;  // the block's first bit and its width (<= 64)
  uint64_t mask;      // its bits, in place
};
// Block b of P over G positions: positions [G b / P, G (b + 1) / P).  22 ThreeBit positions end at
// bit 66: the last block is clamped at bit 64.
inline Block block(int kind, int G, int P, int b) {
  const int lo = G * b / P * kind, top = G * (b + 1) / P * kind, hi = top < 64 ? top : 64;
  return Block{lo, hi - lo, (hi - lo >= 64 ? ~0ull : (1ull << (hi - lo)) - 1ull) << lo};
}

// ---------------------------------------------------------------- one device block per layout
// 256-byte-aligned segments end to end: add() gives the next segment's offset
struct Carve {
  int64_t total = 0;
  int64_t add(int64_t bytes) {
    const int64_t at = total;
    total += (bytes + 255) & ~(int64_t)255;
    return at;
  }
};

// ---------------------------------------------------------------- half keys
// what the host knows before the build; the whitelist's digits (all A/C/G/T) are checked on the device
inline bool halves_possible(int G, int max_d, int64_t nw) { return max_d <= 1 && G >= 2 && G <= 16 && nw > 0; }

struct HalvesDims {
  int GA, GB;      // digits of the high half A = [GB, G) and of the low half B = [0, GB)
  int64_t nA, nB;  // keys of each half: 4^GA, 4^GB
  int pbits;       // bits of a packed whitelist index: ceil(log2 nw), at least 1
  int64_t ndw;     // dwords of the packed permutation of 2 nw entries
};
inline HalvesDims halves_dims(int G, int64_t nw) {
  HalvesDims d{};
  d.GB = G / 2;
  d.GA = G - d.GB;
  d.nA = 1LL << (2 * d.GA);
  d.nB = 1LL << (2 * d.GB);
  d.pbits = 1;
  while (d.pbits < 32 && (1LL << d.pbits) < nw) ++d.pbits;
  d.ndw = (2 * at_least(nw, 1) * d.pbits + 31) / 32 + 2;  // + 2: the last 8-byte load's second dword
  return d;
}

struct HalvesBlock {
  int64_t offA, offB, entA, entB, packed, rankB, total;
};
inline HalvesBlock halves_block(const HalvesDims& d, int64_t nw) {
  const int64_t n = at_least(nw, 1);
  Carve c;
  HalvesBlock b{};
  b.offA = c.add((d.nA + 1) * 4);
  b.offB = c.add((d.nB + 1) * 4);
  b.entA = c.add(n * 2 + 16);  // + 16 B: the last chunk's 16-byte load may run past nw
  b.entB = c.add(n * 2 + 16);
  b.packed = c.add(d.ndw * 4);
  b.rankB = c.add(n);
  b.total = c.total;
  return b;
}
// both offset tables, both entry tables and the packed permutation, without padding or rankB
inline int64_t halves_index_bytes(int G, int64_t nw) {
  const HalvesDims d = halves_dims(G, nw);
  return (d.nA + d.nB + 2) * 4 + nw * 4 + (2 * nw * d.pbits + 31) / 32 * 4;
}

// ---------------------------------------------------------------- open addressing
// Keys are the whole code at max_d = 0 (P = 1 block), else the pairs of P = max_d + 2 blocks: a code
// within max_d agrees exactly on at least two of them.
struct OaLayout {
  int P, nkeys;
  int a[kMaxKeys], b[kMaxKeys];  // the blocks of key t (a == b: one block)
  uint64_t keymask[kMaxKeys];
  int64_t slots;   // per key table: the power of two >= max(kGroup, 2 nw), load <= 1/2
  int64_t groups;  // slots / kGroup
};
// false where the plan cannot take open addressing: more blocks than positions, or more than kMaxKeys keys
inline bool oa_layout(int kind, int code_bits, int max_d, int64_t nw, OaLayout* out) {
  const int G = positions(kind, code_bits), P = max_d == 0 ? 1 : max_d + 2;
  const int nkeys = max_d == 0 ? 1 : P * (P - 1) / 2;
  if (P > G || nkeys > kMaxKeys) return false;
  OaLayout l{};
  l.P = P;
  for (int a = 0; a < P; ++a)
    for (int b = max_d == 0 ? a : a + 1; b < P; ++b) {
      l.a[l.nkeys] = a;
      l.b[l.nkeys] = b;
      l.keymask[l.nkeys++] = block(kind, G, P, a).mask | block(kind, G, P, b).mask;
    }
  l.slots = kGroup;
  while (l.slots < 2 * nw) l.slots *= 2;
  l.groups = l.slots / kGroup;
  *out = l;
  return true;
}
// the bases of the smallest key: every position at max_d = 0, else the two smallest blocks of a floor split
inline int oa_min_bases(int kind, int code_bits, int max_d) {
  const int G = positions(kind, code_bits);
  return max_d == 0 ? G : 2 * (G / (max_d + 2));
}
// The automatic rule: keys are nearly unique for random codes when 4^min_bases >= nw / 2, i.e. at most
// ~2 codes share a key.  (nw < 2^31, so 16 bases always do.)
inline bool oa_keys_wide_enough(int min_bases, int64_t nw) {
  return min_bases >= 16 || (2ull << (2 * min_bases)) >= (uint64_t)at_least(nw, 2);
}
inline int64_t oa_index_bytes(int nkeys, int64_t slots) { return nkeys * slots * 16; }

struct OaBlock {
  int64_t slots[kMaxKeys], total;
};
inline OaBlock oa_block(int nkeys, int64_t slots) {
  Carve c;
  OaBlock b{};
  for (int t = 0; t < nkeys; ++t) b.slots[t] = c.add(slots * 16);
  b.total = c.total;
  return b;
}

// ---------------------------------------------------------------- CSR buckets per block
// log2 of the provisional bucket count, ~nw / 2 buckets: its occupied buckets count the part's
// distinct block values
inline int csr_lg0(int64_t nw) {
  int lg0 = 0;
  while (lg0 < 28 && (1LL << lg0) * 2 < nw) ++lg0;
  return lg0;
}
// log2 of a part's bucket count: `load` buckets per occupied provisional one, never more than those
inline int csr_lg(int lg0, int64_t load, uint64_t occupied) {
  int lg = 0;
  while (lg < lg0 && (1ull << lg) < (uint64_t)load * (occupied < 1 ? 1 : occupied)) ++lg;
  return lg;
}
struct CsrPart {
  uint64_t mask, mul;  // mul: 0 when there is a single bucket
  int lo_bit, nbits;
  int shift;        // 64 - lg, in [1, 63]
  int64_t buckets;  // 2^lg
};
// part k of P = max_d + 1 with 2^lg buckets
inline CsrPart csr_part(int kind, int G, int P, int k, int lg) {
  const Block b = block(kind, G, P, k);
  return CsrPart{b.mask, lg == 0 ? 0ull : kGolden, b.lo_bit, b.nbits, lg == 0 ? 63 : 64 - lg, 1LL << lg};
}
inline int64_t csr_index_bytes(int nparts, const int64_t* nbuckets, int64_t nw) {
  int64_t bytes = 0;
  for (int k = 0; k < nparts; ++k) bytes += (nbuckets[k] + 1) * 4 + nw * 12;
  return bytes;
}

struct CsrBlock {
  int64_t off[kMaxParts], code[kMaxParts], index[kMaxParts], total;
};
inline CsrBlock csr_block(int nparts, const int64_t* nbuckets, int64_t nw) {
  const int64_t n = at_least(nw, 1);
  Carve c;
  CsrBlock b{};
  for (int k = 0; k < nparts; ++k) {
    b.off[k] = c.add((nbuckets[k] + 1) * 4);
    b.code[k] = c.add(n * 8);
    b.index[k] = c.add(n * 4);
  }
  b.total = c.total;
  return b;
}

// ---------------------------------------------------------------- the choice
// The layouts a plan tries, in order; a later one is built only when the earlier one turns out not to
// apply (the half keys, on a whitelist with other digits).  `forced` is SCT_TUNE_NEAREST_SCHEME: the
// half keys are tried when it is kAuto or kHalves, kOa takes open addressing wherever the plan can,
// kCsr never does.
struct Builders {
  int n;
  int scheme[2];
};
inline Builders builders(int kind, int code_bits, int max_d, int64_t nw, int64_t forced) {
  Builders r{};
  if ((forced == kAuto || forced == kHalves) && halves_possible(positions(kind, code_bits), max_d, nw))
    r.scheme[r.n++] = kHalves;
  OaLayout l;
  bool oa = oa_layout(kind, code_bits, max_d, nw, &l);
  if (forced == kCsr) oa = false;
  else if (forced != kOa) oa = oa && oa_keys_wide_enough(oa_min_bases(kind, code_bits, max_d), nw);
  r.scheme[r.n++] = oa ? kOa : kCsr;
  return r;
}

}  // namespace nearest_index
}  // namespace sct
