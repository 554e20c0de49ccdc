// Per-record decode / GC / Hamming device functions shared by the batch kernels (encode.hip) and
// the resident scalar server (scalar_server.hip), and the limb count of a record.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

inline int words_for(int bits, int L) {
  const int64_t w = ((int64_t)bits * L + 63) / 64;
  return (int)(w > 0 ? w : 1);
}

__device__ __forceinline__ uint64_t limb(const uint64_t* w, int words, int i) {
  return i < words ? w[i] : 0ull;
}

// value of the `width`-bit group starting at bit `pos` of a multi-limb integer
__device__ __forceinline__ uint32_t group_at(const uint64_t* w, int words, int64_t pos, int width) {
  const int i = (int)(pos >> 6), off = (int)(pos & 63);
  uint64_t v = limb(w, words, i) >> off;
  if (off + width > 64) v |= limb(w, words, i + 1) << (64 - off);
  return (uint32_t)(v & ((1u << width) - 1u));
}

__device__ __forceinline__ void decode2_limbs(const uint64_t* w, int words, int L, uint8_t* o) {
  for (int p = 0; p < L; ++p) {
    const int64_t pos = 2LL * (L - 1 - p);
    const uint32_t v = pos < 64LL * words ? group_at(w, words, pos, 2) : 0u;
    // "ACTG"[v] from a register (the string literal was a global load per base: ~2 us of a
    // 16-base scalar decode)
    o[p] = (uint8_t)(0x47544341u >> (8 * v));
  }
}

// A one-limb code is read once into a register and its bases leave four to a store: through the
// generic path the byte stores to o (which may alias w) made the compiler reload the code for
// every base, one dependent LDS read each in the scalar server (85 ns per base per call)
__device__ __forceinline__ void decode2_record(const uint64_t* w, int words, int L, uint8_t* o) {
  if (words != 1) {
    decode2_limbs(w, words, L, o);
    return;
  }
  const uint64_t c = w[0];
  auto base = [&](int p) {  // "ACTG"[group L-1-p], 'A' above the limb
    const int pos = 2 * (L - 1 - p);
    const uint32_t v = pos < 64 ? (uint32_t)(c >> pos) & 3u : 0u;
    return (0x47544341u >> (8 * v)) & 0xFFu;
  };
  int p = 0;
  if (((uintptr_t)o & 3u) == 0u)
    for (; p + 4 <= L; p += 4)
      *reinterpret_cast<uint32_t*>(o + p) = base(p) | base(p + 1) << 8 | base(p + 2) << 16 | base(p + 3) << 24;
  for (; p < L; ++p) o[p] = (uint8_t)base(p);
}

// o[maxlen - 1 - t] = base of triplet t for t <= the top non-zero triplet; returns that
// count, and in err the first invalid triplet value (0 / 5 / 7) or -1
__device__ __forceinline__ int32_t decode3_limbs(const uint64_t* w, int words, int maxlen, uint8_t* o,
                                                 int32_t& err) {
  const int ntrip = (64 * words + 2) / 3;
  int top = -1;
  for (int t = ntrip - 1; t >= 0; --t)
    if (group_at(w, words, 3LL * t, 3) != 0u) {
      top = t;
      break;
    }
  err = -1;
  for (int t = 0; t <= top; ++t) {
    const uint32_t v = group_at(w, words, 3LL * t, 3);
    uint8_t ch = 0;
    switch (v) {
      case 1: ch = 'C'; break;
      case 2: ch = 'A'; break;
      case 3: ch = 'G'; break;
      case 4: ch = 'T'; break;
      case 6: ch = 'N'; break;
      default:
        if (err < 0) err = (int32_t)v;
        break;
    }
    o[maxlen - 1 - t] = ch;
  }
  return top + 1;
}

// (a one-limb code in a register, as decode2_record)
__device__ __forceinline__ int32_t decode3_record(const uint64_t* w, int words, int maxlen, uint8_t* o,
                                                  int32_t& err) {
  if (words != 1) return decode3_limbs(w, words, maxlen, o, err);
  const uint64_t c = w[0];
  const int top = c ? (63 - __clzll((long long)c)) / 3 : -1;  // the top non-zero triplet
  err = -1;
  for (int t = 0; t <= top; ++t) {
    const uint32_t v = (uint32_t)(c >> (3 * t)) & 7u;
    // C A G T at 1..4, N at 6 (bytes of 0x544741434E: v = 1..4 -> byte v - 1, 6 -> byte 4)
    const bool ok = (v >= 1u && v <= 4u) || v == 6u;
    if (!ok && err < 0) err = (int32_t)v;
    o[maxlen - 1 - t] = ok ? (uint8_t)(0x4E54474143ull >> (8 * (v == 6u ? 4u : v - 1u))) : (uint8_t)0;
  }
  return top + 1;
}

// bit-0-of-each-triplet mask for limb i (64*i mod 3 shifts the pattern)
__device__ __forceinline__ uint64_t m3(int i) {
  switch (i % 3) {
    case 0: return 0x9249249249249249ull;
    case 1: return 0x4924924924924924ull;
    default: return 0x2492492492492492ull;
  }
}

__device__ __forceinline__ int32_t gc_record(int kind, const uint64_t* w, int words, int L) {
  int32_t g = 0;
  for (int i = 0; i < words; ++i) {
    uint64_t m;
    if (kind == 2) {
      const int64_t lo = 64LL * i, rem = 2LL * L - lo;  // bits of the L groups inside this limb
      if (rem <= 0) break;
      m = 0x5555555555555555ull;
      if (rem < 64) m &= (1ull << rem) - 1ull;
    } else {
      m = m3(i);
    }
    g += __popcll(w[i] & m);
  }
  return g;
}

__device__ __forceinline__ int32_t hamming_record(int kind, const uint64_t* x, const uint64_t* y, int words) {
  int32_t d = 0;
  if (kind == 2) {
    for (int i = 0; i < words; ++i) {
      const uint64_t v = x[i] ^ y[i];
      d += __popcll((v | (v >> 1)) & 0x5555555555555555ull);
    }
  } else {
    uint64_t v = x[0] ^ y[0];
    for (int i = 0; i < words; ++i) {
      const uint64_t nx = i + 1 < words ? (x[i + 1] ^ y[i + 1]) : 0ull;
      const uint64_t s = v | ((v >> 1) | (nx << 63)) | ((v >> 2) | (nx << 62));
      d += __popcll(s & m3(i));
      v = nx;
    }
  }
  return d;
}

}  // namespace
