// Element-wise encoding kernels for gfx950: encode (TwoBit/ThreeBit + GC + flags),
// decode, gc_content and pairwise Hamming distance.  All are one-record-per-lane,
// HBM-bound streaming kernels; the byte->code map is a 256-entry LDS table.
//
// Reference semantics (src/sctools/encodings.py):
//   TwoBit map      :53-69   A/a 0, C/c 1, T/t 2, G/g 3; IUPAC ambiguity -> random
//                            (flagged here, drawn by the Python caller in order);
//                            anything else -> KeyError (flagged here)
//   TwoBit.encode   :75-88   MSB-first, 2 bits per byte
//   TwoBit.decode   :90-100  exactly L bases from the LSB upward
//   TwoBit.gc       :102-111 low bit of each of the L groups
//   TwoBit.hamming  :113-121 non-zero 2-bit groups of a^b
//   ThreeBit map    :139-149 C 1, A 2, G 3, T 4, N 6, any other byte -> 6
//   ThreeBit.encode :155-167 MSB-first, 3 bits per byte
//   ThreeBit.decode :169-180 triplets up to the top non-zero one; 0/5/7 -> KeyError
//   ThreeBit.gc     :182-192 bit 0 of every triplet
//   ThreeBit.hamming:194-202 non-zero 3-bit groups of a^b
//
// This file holds the batch kernels and the device-pointer entry points.  The per-record decode /
// GC / Hamming functions are in encode_records.h (the resident scalar server, scalar_server.hip,
// runs them too); the host-array entry points are in encode_host.cpp.
#include <stddef.h>

#include <algorithm>

#include "sct_common.h"
#include "encode_common.h"
#include "encode_records.h"

namespace {

constexpr int WG = 256;
__device__ __forceinline__ void fill_lut(uint8_t* lut, int kind) {
  for (int c = threadIdx.x; c < 256; c += blockDim.x) lut[c] = lut_entry(kind, c);
  __syncthreads();
}

// Records at seqs + r * stride of L bytes, or (starts != nullptr) at seqs + starts[r] of
// lens[r] bytes each (variable-length lines: the whitelist ingest, sctools_amd/csrc/lines.hip).
__global__ __launch_bounds__(WG) void encode_kernel(int kind, const uint8_t* __restrict__ seqs,
                                                    int64_t n, int64_t stride, int L_all, int words,
                                                    bool dword_path, uint64_t* __restrict__ codes,
                                                    uint8_t* __restrict__ gc,
                                                    uint8_t* __restrict__ flags,
                                                    const int64_t* __restrict__ starts = nullptr,
                                                    const int32_t* __restrict__ lens = nullptr) {
  __shared__ uint8_t lut[256];
  fill_lut(lut, kind);
  for (int64_t r = (int64_t)blockIdx.x * WG + threadIdx.x; r < n; r += (int64_t)gridDim.x * WG) {
    const int L = starts ? lens[r] : L_all;
    RecordReader rd{seqs + (starts ? starts[r] : r * stride), dword_path, 0u, -1};
    uint32_t g, fl;
    encode_record(lut, kind, rd, L, words, codes + r * words, g, fl);
    if (gc) gc[r] = (uint8_t)(g > 255 ? 255 : g);
    if (flags) flags[r] = (uint8_t)fl;
  }
}

// Variable-length records of one limb (the whitelist's lines): each lane loads the aligned
// dwords that hold its record (at most 9 for 32 bases: every load independent, and a wave's
// loads of consecutive lines cover consecutive lines of memory), realigns them by the start's
// byte offset and reads every position's LUT entry independently.  Only dwords holding a byte
// of the record are loaded, so no load leaves the pages the record lies in.  Records longer
// than 32 bytes take the byte loop.
__global__ __launch_bounds__(WG) void encode_var_kernel(int kind, const uint8_t* __restrict__ buf, int64_t n,
                                                        const int64_t* __restrict__ starts,
                                                        const int32_t* __restrict__ lens,
                                                        uint64_t* __restrict__ codes, uint8_t* __restrict__ gc,
                                                        uint8_t* __restrict__ flags) {
  __shared__ uint8_t lut[256];
  fill_lut(lut, kind);
  const uint64_t gcm = kind == 2 ? 0x5555555555555555ull : 0x9249249249249249ull;
  for (int64_t r = (int64_t)blockIdx.x * WG + threadIdx.x; r < n; r += (int64_t)gridDim.x * WG) {
    const uint8_t* rec = buf + starts[r];
    const int L = lens[r];
    uint64_t code = 0;
    uint32_t fl = 0;
    if (L == 0) {
    } else if (L <= 32) {
      const int o = (int)((uintptr_t)rec & 3), o8 = 8 * o;
      const uint32_t* dw = reinterpret_cast<const uint32_t*>(rec - o);
      uint32_t d[9], w[8];
#pragma unroll
      for (int k = 0; k < 9; ++k) {  // dword k of the record, clamped to its last one (no branch)
        const int kk = 4 * k < o + L ? k : (o + L - 1) >> 2;
        d[k] = __builtin_nontemporal_load(dw + kk);
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) w[k] = (uint32_t)((((uint64_t)d[k + 1] << 32) | d[k]) >> o8);
#pragma unroll
      for (int p = 0; p < 32; ++p)
        if (p < L) {
          const uint32_t e = lut[(w[p >> 2] >> (8 * (p & 3))) & 0xFFu];
          code = (code << kind) | (e & 7u);
          fl |= e;
        }
    } else {
      for (int p = 0; p < L; ++p) {
        const uint32_t e = lut[rec[p]];
        code = (code << kind) | (e & 7u);
        fl |= e;
      }
    }
    codes[r] = code;
    if (gc) {
      const uint32_t g = (uint32_t)__popcll(code & gcm);
      gc[r] = (uint8_t)(g > 255 ? 255 : g);
    }
    if (flags) flags[r] = (uint8_t)(((fl & F_AMBIG) ? 1u : 0u) | ((fl & F_INVALID) ? 2u : 0u));
  }
}

// Contiguous records (stride == L, one limb): a workgroup stages 256 records with
// coalesced 16-byte loads into LDS, then each lane packs its record from LDS (dword reads
// when L % 4 == 0, conflict-free for odd L/4) through the LDS byte LUT.  The staging
// turns the per-lane, L-byte-strided global loads of encode_kernel into full-line reads.
template <int BITS, int R>
__global__ __launch_bounds__(WG) void encode_tiled_kernel(const uint8_t* __restrict__ seqs,
                                                          int64_t n, int L,
                                                          uint64_t* __restrict__ codes,
                                                          uint8_t* __restrict__ gc,
                                                          uint8_t* __restrict__ flags) {
  __shared__ uint8_t lut[256];
  extern __shared__ __attribute__((aligned(16))) uint4 stage4[];  // R * WG * L bytes
  fill_lut(lut, BITS);
  const uint8_t* stage = reinterpret_cast<const uint8_t*>(stage4);
  const int tid = threadIdx.x;
  constexpr int TILE = R * WG;  // records per workgroup iteration: R in flight per lane
  const int64_t ntiles = (n + TILE - 1) / TILE;
  typedef unsigned v4u __attribute__((ext_vector_type(4)));
  // a thread's 16-B loads of a tile are all issued before any of them is stored to LDS (8
  // per batch: 7 at L = 28).  When one batch holds a whole tile (L * R <= 128) the next
  // tile's loads are issued right after this tile's LDS stores, so they fly while this
  // tile is packed.
  const bool pipe = L * R <= 128;
  v4u t[8];
  auto fetch = [&](int64_t tl, int64_t k0) {
    const int64_t rb = tl * TILE, nr = n - rb < TILE ? n - rb : TILE;
    const int64_t m16 = (nr * L) >> 4;
    const v4u* s4 = reinterpret_cast<const v4u*>(seqs + rb * L);  // 16-B aligned: TILE * L % 16 == 0
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int64_t k = k0 + u * WG + tid;
      if (k < m16) t[u] = __builtin_nontemporal_load(s4 + k);
    }
  };
  if (pipe && (int64_t)blockIdx.x < ntiles) fetch(blockIdx.x, 0);
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r0 = tile * TILE;
    const int64_t nrec = n - r0 < TILE ? n - r0 : TILE;
    const int64_t nbytes = nrec * L;
    const uint8_t* src = seqs + r0 * L;
    const int64_t n16 = nbytes >> 4;
    for (int64_t k0 = 0; k0 < n16; k0 += 8 * WG) {
      if (!pipe) fetch(tile, k0);
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t k = k0 + u * WG + tid;
        if (k < n16) stage4[k] = make_uint4(t[u].x, t[u].y, t[u].z, t[u].w);
      }
    }
    if (pipe && tile + gridDim.x < ntiles) fetch(tile + gridDim.x, 0);
    for (int64_t k = (n16 << 4) + tid; k < nbytes; k += WG)
      reinterpret_cast<uint8_t*>(stage4)[k] = src[k];
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
      const int lr = rr * WG + tid;  // consecutive lanes -> consecutive records (coalesced stores)
      if (lr < nrec) {
        const uint8_t* rec = stage + (int64_t)lr * L;
        uint64_t code = 0;
        uint32_t fl = 0;
        bool done = false;
        if (BITS == 2 && (L & 3) == 0) {
          // TwoBit, 4 bases per dword without the LUT: u = the bytes upper-cased; their low 3
          // bits (A 1, C 3, T 4, G 7) index a v_perm byte table of the expected letters, so
          // u == table[u & 7] in every byte iff all four are ACGTacgt.  The values are
          // (u >> 1) & 3 per byte (A 0, C 1, T 2, G 3), gathered MSB-first into one byte by
          // one multiply: v * (1 + 2^10 + 2^20 + 2^30) puts byte j's value at bits 30 - 2j,
          // every other partial product in a disjoint 2-bit slot below 24 (no carries).
          // A byte that is not a base (N, IUPAC, invalid: 1 % of config 5's reads) has code bits
          // 0 (lut & 7 for every such byte), so it is cleared through the byte mask of the
          // mismatch and only its flag is read from the LUT -- every lane runs the same steps
          // (the divergent 28-step LUT loop this replaces cost 1.2 ms of 7.8 on config 5's 1e9
          // reads: half the waves carried a read with an N).  One limb: L <= 32, <= 8 dwords.
          const uint32_t* rw = reinterpret_cast<const uint32_t*>(rec);
          uint32_t nzs[8], anyb = 0;
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            nzs[k] = 0;
            if (k < (L >> 2)) {
              const uint32_t u = rw[k] & 0xDFDFDFDFu;
              const uint32_t d = u ^ __builtin_amdgcn_perm(0x47010154u, 0x43014101u, u & 0x07070707u);
              const uint32_t nz = (((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | d) & 0x80808080u;  // bit 7: differs
              const uint32_t v = ((u >> 1) & 0x03030303u) & ~((nz - (nz >> 7)) | nz);
              code = (code << 8) | ((v * 0x40100401u) >> 24);
              nzs[k] = nz;
              anyb |= nz;
            }
          }
          if (anyb) {
#pragma unroll
            for (int k = 0; k < 8; ++k)
              for (uint32_t b = nzs[k]; b; b &= b - 1) fl |= lut[(rw[k] >> (__builtin_ctz(b) - 7)) & 0xFFu];
          }
          done = true;
        }
        if (done) {
        } else if ((L & 3) == 0) {
          const uint32_t* rw = reinterpret_cast<const uint32_t*>(rec);
          for (int k = 0; k < (L >> 2); ++k) {
            const uint32_t w = rw[k];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
              const uint32_t e = lut[(w >> (8 * b)) & 0xFFu];
              code = (code << BITS) | (e & 7u);
              fl |= e;
            }
          }
        } else {
          for (int p = 0; p < L; ++p) {
            const uint32_t e = lut[rec[p]];
            code = (code << BITS) | (e & 7u);
            fl |= e;
          }
        }
        const int64_t r = r0 + lr;
        codes[r] = code;
        if (gc)
          gc[r] = (uint8_t)__popcll(code & (BITS == 2 ? 0x5555555555555555ull : 0x9249249249249249ull));
        if (flags) flags[r] = (uint8_t)(((fl & F_AMBIG) ? 1u : 0u) | ((fl & F_INVALID) ? 2u : 0u));
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(WG) void decode2_kernel(const uint64_t* __restrict__ codes, int64_t n,
                                                     int words, int L, uint8_t* __restrict__ out) {
  for (int64_t r = (int64_t)blockIdx.x * WG + threadIdx.x; r < n; r += (int64_t)gridDim.x * WG)
    decode2_record(codes + r * words, words, L, out + r * L);
}

__global__ __launch_bounds__(WG) void decode3_kernel(const uint64_t* __restrict__ codes, int64_t n,
                                                     int words, int maxlen, uint8_t* __restrict__ out,
                                                     int32_t* __restrict__ lengths,
                                                     int32_t* __restrict__ bad) {
  for (int64_t r = (int64_t)blockIdx.x * WG + threadIdx.x; r < n; r += (int64_t)gridDim.x * WG) {
    int32_t err;
    lengths[r] = decode3_record(codes + r * words, words, maxlen, out + r * maxlen, err);
    bad[r] = err;
  }
}

__global__ __launch_bounds__(WG) void gc_kernel(int kind, const uint64_t* __restrict__ codes,
                                                int64_t n, int words, int L,
                                                int32_t* __restrict__ out) {
  for (int64_t r = (int64_t)blockIdx.x * WG + threadIdx.x; r < n; r += (int64_t)gridDim.x * WG)
    out[r] = gc_record(kind, codes + r * words, words, L);
}

__global__ __launch_bounds__(WG) void hamming_kernel(int kind, const uint64_t* __restrict__ a,
                                                     const uint64_t* __restrict__ b, int64_t n,
                                                     int words, int32_t* __restrict__ out) {
  for (int64_t r = (int64_t)blockIdx.x * WG + threadIdx.x; r < n; r += (int64_t)gridDim.x * WG)
    out[r] = hamming_record(kind, a + r * words, b + r * words, words);
}

// Per-position base counts.  Base p of a code is bits 2j, 2j + 1 with j = L - 1 - p, and only
// j < 32 can be non-zero, so the work is the 32 2-bit fields j of the codes, counted in
// registers with SWAR counters (no per-code atomics, no per-field loop): per code the
// indicator masks of values 1, 2, 3 (bit 2j set when field j holds that value) are added into
// nibble counters (fields 2i / 2i + 1 in nibble i of two words), folded every 15 codes into
// byte counters (field 4k + q in byte k of word q), and those, every 255 codes or at the end,
// are widened to 16-bit lanes, summed over the wave by shuffles and added to the workgroup's
// LDS tally.  Each workgroup writes its 128 partials (bin-major), which
// base_frequency_reduce_kernel sums: no same-address global atomics.  A lane's codes are
// gridDim * 256 apart, so a wave's loads stay coalesced.
__global__ __launch_bounds__(WG) void base_frequency_kernel(const uint64_t* __restrict__ codes,
                                                            int64_t n, unsigned long long* __restrict__ part) {
  constexpr uint64_t K5 = 0x5555555555555555ull, K1 = 0x1111111111111111ull, KF = 0x0F0F0F0F0F0F0F0Full;
  __shared__ unsigned long long tally[32][4];
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < 128) tally[tid >> 2][tid & 3] = 0;
  __syncthreads();
  const int64_t G = (int64_t)gridDim.x * WG;
  unsigned long long seen = 0;
  for (int64_t e0 = (int64_t)blockIdx.x * WG + tid; e0 - tid < n; e0 += 255 * G) {  // epochs of <= 255 codes per lane
    uint64_t Q[3][4] = {};  // [value - 1][q]: byte k counts field 4k + q
    for (int c = 0; c < 17; ++c) {
      const int64_t c0 = e0 + (int64_t)c * 15 * G;
      if (c0 - tid >= n) break;  // workgroup-uniform
      uint64_t N[3][2] = {};  // [value - 1][field parity]: nibble i counts field 2i + parity
      uint64_t xs[15];
#pragma unroll
      for (int u = 0; u < 15; ++u) {  // all 15 loads issued first (clamped, not branched around)
        const int64_t r = c0 + u * G;
        xs[u] = codes[r < n ? r : n - 1];
      }
#pragma unroll
      for (int u = 0; u < 15; ++u) {
        const int64_t r = c0 + u * G;
        if (r < n) {
          const uint64_t x = xs[u];
          const uint64_t lo = x & K5, hi = (x >> 1) & K5, m3 = lo & hi, m[3] = {lo ^ m3, hi ^ m3, m3};
#pragma unroll
          for (int v = 0; v < 3; ++v) {
            N[v][0] += m[v] & K1;
            N[v][1] += (m[v] >> 2) & K1;
          }
          ++seen;
        }
      }
#pragma unroll
      for (int v = 0; v < 3; ++v) {
        Q[v][0] += N[v][0] & KF;         // fields 4k
        Q[v][2] += (N[v][0] >> 4) & KF;  // fields 4k + 2
        Q[v][1] += N[v][1] & KF;         // fields 4k + 1
        Q[v][3] += (N[v][1] >> 4) & KF;  // fields 4k + 3
      }
    }
    // bytes -> 16-bit lanes (even / odd bytes), summed over the wave (<= 64 * 255 per lane)
#pragma unroll
    for (int v = 0; v < 3; ++v)
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          uint64_t w = (Q[v][q] >> (8 * h)) & 0x00FF00FF00FF00FFull;  // u16 lane i = byte 2i + h
#pragma unroll
          for (int o = 32; o; o >>= 1) w += __shfl_xor(w, o);
          if (lane < 4) {  // lane i takes u16 lane i: byte k = 2i + h, field 4k + q
            const int k = 2 * lane + h;
            atomicAdd(&tally[4 * k + q][v + 1], (unsigned long long)((w >> (16 * lane)) & 0xFFFFu));
          }
        }
  }
  for (int o = 32; o; o >>= 1) seen += __shfl_xor(seen, o);
  if (lane == 0) atomicAdd(&tally[0][0], seen);  // codes seen; value 0 = seen - the rest
  __syncthreads();
  if (tid < 128) {
    const int j = tid >> 2, v = tid & 3;
    unsigned long long t = tally[j][v];
    if (v == 0) t = tally[0][0] - tally[j][1] - tally[j][2] - tally[j][3];
    part[(size_t)tid * gridDim.x + blockIdx.x] = t;
  }
}

// L <= 16 (every output field j < 16 lies in a code's low 32 bits; the bits above are never
// read): the same partials from 32-bit words at a third of the instructions.  Per code the
// indicator masks m_v (bit 2j set when field j holds v = 1..3) come from x and x >> 1 by one
// bitop3 each; three codes' masks add in one v_add3_u32 (2-bit fields, <= 3), five such sums
// into nibble counters (fields 2i / 2i + 1 in nibble i of two words, <= 15), then into byte
// counters (field 4k + {0, 2, 1, 3}[w] in byte k of word w).  The host sizes the grid so no
// lane sees more than 255 codes.  The workgroup's 12 x 256 byte-counter words meet in LDS and
// 192 threads sum them (byte pairs widened to 16-bit lanes, <= 256 * 255), so the epilogue is
// 16 LDS reads and 8 shuffles per thread instead of 24 64-bit wave reductions per wave.
__global__ __launch_bounds__(WG) void base_frequency16_kernel(const uint64_t* __restrict__ codes, int64_t n,
                                                              unsigned long long* __restrict__ part) {
  constexpr uint32_t K5 = 0x55555555u, K3 = 0x33333333u, KF = 0x0F0F0F0Fu;
  __shared__ uint32_t xch[WG / 64][12][64];
  __shared__ uint32_t cnt[16][4];  // [field j][value v]
  __shared__ uint32_t seen_w[WG / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t G = (int64_t)gridDim.x * WG;
  const uint32_t* lo32 = reinterpret_cast<const uint32_t*>(codes);  // (little endian: word 2r = low half)
  uint32_t B[3][4] = {};
  uint32_t seen = 0;
  for (int64_t c0 = (int64_t)blockIdx.x * WG + tid; c0 - tid < n; c0 += 15 * G) {  // rounds of 15 codes
    uint32_t xs[15];
#pragma unroll
    for (int u = 0; u < 15; ++u) {  // all 15 loads issued first (clamped, then zeroed: a zero adds no mask)
      const int64_t r = c0 + u * G;
      xs[u] = lo32[2 * (r < n ? r : n - 1)];
    }
#pragma unroll
    for (int u = 0; u < 15; ++u) {
      const bool in = c0 + u * G < n;
      xs[u] = in ? xs[u] : 0u;
      seen += in ? 1u : 0u;
    }
    uint32_t Ne[3] = {0, 0, 0}, No[3] = {0, 0, 0};
#pragma unroll
    for (int g = 0; g < 5; ++g) {
      uint32_t m[3][3];
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const uint32_t x = xs[3 * g + t], y = x >> 1;
        m[0][t] = x & ~y & K5;  // 01: value 1
        m[1][t] = ~x & y & K5;  // 10: value 2
        m[2][t] = x & y & K5;   // 11: value 3
      }
#pragma unroll
      for (int v = 0; v < 3; ++v) {
        const uint32_t S = m[v][0] + m[v][1] + m[v][2];
        Ne[v] += S & K3;
        No[v] += (S >> 2) & K3;
      }
    }
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      B[v][0] += Ne[v] & KF;         // fields 4k
      B[v][1] += (Ne[v] >> 4) & KF;  // fields 4k + 2
      B[v][2] += No[v] & KF;         // fields 4k + 1
      B[v][3] += (No[v] >> 4) & KF;  // fields 4k + 3
    }
  }
#pragma unroll
  for (int v = 0; v < 3; ++v)
#pragma unroll
    for (int w = 0; w < 4; ++w) xch[wave][4 * v + w][lane] = B[v][w];
  for (int o = 32; o; o >>= 1) seen += __shfl_xor(seen, o);
  if (lane == 0) seen_w[wave] = seen;
  __syncthreads();
  if (tid < 192) {  // word w = 4 v + q of all 256 lanes: 16 threads (one 16-lane group of a wave) per word
    const int w = tid >> 4, sub = tid & 15;
    uint32_t e = 0, o = 0;  // bytes 0, 2 / 1, 3 as 16-bit lanes
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int l = sub + 16 * i;
      const uint32_t x = xch[l >> 6][w][l & 63];
      e += x & 0x00FF00FFu;
      o += (x >> 8) & 0x00FF00FFu;
    }
#pragma unroll
    for (int s = 8; s; s >>= 1) {
      e += __shfl_xor(e, s);
      o += __shfl_xor(o, s);
    }
    if (sub == 0) {
      const int v = w >> 2, q = w & 3, off = q == 0 ? 0 : (q == 1 ? 2 : (q == 2 ? 1 : 3));
      cnt[off][v + 1] = e & 0xFFFFu;         // byte 0: field off
      cnt[4 + off][v + 1] = o & 0xFFFFu;     // byte 1: field 4 + off
      cnt[8 + off][v + 1] = e >> 16;         // byte 2
      cnt[12 + off][v + 1] = o >> 16;        // byte 3
    }
  }
  __syncthreads();
  if (tid < 128) {
    const int j = tid >> 2, v = tid & 3;
    uint32_t all = 0;
#pragma unroll
    for (int k = 0; k < WG / 64; ++k) all += seen_w[k];
    uint32_t t = 0;
    if (j < 16)
      t = v ? cnt[j][v] : all - cnt[j][1] - cnt[j][2] - cnt[j][3];
    else
      t = v ? 0u : all;  // (fields 16..31 are not output for L <= 16)
    part[(size_t)tid * gridDim.x + blockIdx.x] = t;
  }
}

// out[4 (L - 1 - j) + v] = the sum of the workgroups' partials of (j, v) (one workgroup per
// bin); bases p < L - 32 are all 0: n of value 0
__global__ __launch_bounds__(WG) void base_frequency_reduce_kernel(const unsigned long long* __restrict__ part,
                                                                   int parts, int64_t n, int L,
                                                                   unsigned long long* __restrict__ out) {
  const int b = blockIdx.x, j = b >> 2, v = b & 3;
  unsigned long long s = 0;
  for (int i = threadIdx.x; i < parts; i += WG) s += part[(size_t)b * parts + i];
#pragma unroll
  for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
  __shared__ unsigned long long ws[WG / 64];
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < WG / 64; ++w) s += ws[w];
    if (j < 32 && j < L) out[4 * (L - 1 - j) + v] = s;
  }
  if (b == 0)
    for (int p = threadIdx.x; p < L - 32; p += WG)
      for (int k = 0; k < 4; ++k) out[4 * p + k] = k ? 0ull : (unsigned long long)n;
}

unsigned grid_for(int64_t n) {
  const int64_t b = sct::ceil_div(n, WG);
  return (unsigned)(b < 8192 ? (b > 0 ? b : 1) : 8192);
}

}  // namespace

extern "C" int sct_encode(int kind, const uint8_t* seqs, int64_t n, int64_t stride, int L,
                          uint64_t* codes, uint8_t* gc, uint8_t* flags, void* stream) {
  SCT_CHECK(kind == 2 || kind == 3, "kind must be 2 or 3");
  SCT_CHECK(n >= 0 && L >= 0 && stride >= L, "bad n/L/stride");
  SCT_CHECK(gc == nullptr || L <= 255, "gc output needs L <= 255");
  if (n == 0) return SCT_OK;
  SCT_CHECK(codes != nullptr && (L == 0 || seqs != nullptr), "NULL pointer");
  const int words = words_for(kind, L);
  constexpr int R = 4;  // tiled encoder: 4 x 256 records staged per iteration (28 KiB at L = 28)
  // (fewer records than one tile -- the drop-in's scalar calls -- skip the occupancy query)
  if (n >= R * WG && stride == L && words == 1 && L > 0 && L <= 64 && (uintptr_t)seqs % 16 == 0) {
    const size_t lds = (size_t)R * WG * L;
    const int64_t tiles = sct::ceil_div(n, R * WG);
    // one workgroup per tile (no loop), as a one-pass copy grid: 6.58 vs 7.68 ms for the
    // resident grid's loop on 100M 16-bp records (SCT_TUNE_ENCODE_GRID = 0 restores it)
    int64_t grid = tiles;
    if (sct::tune(SCT_TUNE_ENCODE_GRID, 1) != 1 || tiles >= (1LL << 31)) {
      sct::scalar_quiesce();
      // persistent: exactly the resident workgroups (a 4096 grid at 5 per CU left a partial
      // last round of workgroups, each looping over many tiles)
      int dev = 0, cus = 0, per_cu = 0;
      if (hipGetDevice(&dev) != hipSuccess ||
          hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        cus = 256;
      if (kind == 2)
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, encode_tiled_kernel<2, R>, WG, lds);
      else
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, encode_tiled_kernel<3, R>, WG, lds);
      grid = std::min<int64_t>(tiles, (int64_t)std::max(cus, 1) * std::max(per_cu, 1));
    }
    if (kind == 2)
      hipLaunchKernelGGL((encode_tiled_kernel<2, R>), dim3((unsigned)grid), dim3(WG), lds,
                         sct::as_stream(stream), seqs, n, L, codes, gc, flags);
    else
      hipLaunchKernelGGL((encode_tiled_kernel<3, R>), dim3((unsigned)grid), dim3(WG), lds,
                         sct::as_stream(stream), seqs, n, L, codes, gc, flags);
    SCT_LAUNCH_CHECK();
    return SCT_OK;
  }
  const bool dw = (L % 4 == 0) && (stride % 4 == 0) && ((uintptr_t)seqs % 4 == 0);
  hipLaunchKernelGGL(encode_kernel, dim3(grid_for(n)), dim3(WG), 0, sct::as_stream(stream), kind,
                     seqs, n, stride, L, words, dw, codes, gc, flags, (const int64_t*)nullptr,
                     (const int32_t*)nullptr);
  SCT_LAUNCH_CHECK();
  return SCT_OK;
}

extern "C" int sct_encode_var(int kind, const uint8_t* buf, const int64_t* starts, const int32_t* lens,
                              int64_t n, int words, uint64_t* codes, uint8_t* gc, uint8_t* flags, void* stream) {
  SCT_CHECK(kind == 2 || kind == 3, "kind must be 2 or 3");
  SCT_CHECK(n >= 0 && words >= 1, "bad n/words");
  if (n == 0) return SCT_OK;
  SCT_CHECK(buf && starts && lens && codes, "NULL pointer");
  if (words == 1) {
    hipLaunchKernelGGL(encode_var_kernel, dim3((unsigned)std::min<int64_t>(sct::ceil_div(n, WG), 1 << 30)), dim3(WG), 0, sct::as_stream(stream), kind, buf, n,
                       starts, lens, codes, gc, flags);
    SCT_LAUNCH_CHECK();
    return SCT_OK;
  }
  hipLaunchKernelGGL(encode_kernel, dim3(grid_for(n)), dim3(WG), 0, sct::as_stream(stream), kind, buf, n,
                     (int64_t)0, 0, words, false, codes, gc, flags, starts, lens);
  SCT_LAUNCH_CHECK();
  return SCT_OK;
}

extern "C" int sct_decode2(const uint64_t* codes, int64_t n, int words, int L, uint8_t* out,
                           void* stream) {
  SCT_CHECK(n >= 0 && words >= 1 && L >= 0, "bad n/words/L");
  if (n == 0 || L == 0) return SCT_OK;
  SCT_CHECK(codes && out, "NULL pointer");
  hipLaunchKernelGGL(decode2_kernel, dim3(grid_for(n)), dim3(WG), 0, sct::as_stream(stream), codes,
                     n, words, L, out);
  SCT_LAUNCH_CHECK();
  return SCT_OK;
}

extern "C" int sct_decode3(const uint64_t* codes, int64_t n, int words, int maxlen, uint8_t* out,
                           int32_t* lengths, int32_t* bad, void* stream) {
  SCT_CHECK(n >= 0 && words >= 1, "bad n/words");
  SCT_CHECK(maxlen >= (64 * words + 2) / 3, "maxlen %d < %d", maxlen, (64 * words + 2) / 3);
  if (n == 0) return SCT_OK;
  SCT_CHECK(codes && out && lengths && bad, "NULL pointer");
  hipLaunchKernelGGL(decode3_kernel, dim3(grid_for(n)), dim3(WG), 0, sct::as_stream(stream), codes,
                     n, words, maxlen, out, lengths, bad);
  SCT_LAUNCH_CHECK();
  return SCT_OK;
}

extern "C" int sct_gc_content(int kind, const uint64_t* codes, int64_t n, int words, int L,
                              int32_t* out, void* stream) {
  SCT_CHECK(kind == 2 || kind == 3, "kind must be 2 or 3");
  SCT_CHECK(n >= 0 && words >= 1 && L >= 0, "bad n/words/L");
  if (n == 0) return SCT_OK;
  SCT_CHECK(codes && out, "NULL pointer");
  hipLaunchKernelGGL(gc_kernel, dim3(grid_for(n)), dim3(WG), 0, sct::as_stream(stream), kind, codes,
                     n, words, L, out);
  SCT_LAUNCH_CHECK();
  return SCT_OK;
}

extern "C" int sct_hamming_pairs(int kind, const uint64_t* a, const uint64_t* b, int64_t n,
                                 int words, int32_t* out, void* stream) {
  SCT_CHECK(kind == 2 || kind == 3, "kind must be 2 or 3");
  SCT_CHECK(n >= 0 && words >= 1, "bad n/words");
  if (n == 0) return SCT_OK;
  SCT_CHECK(a && b && out, "NULL pointer");
  hipLaunchKernelGGL(hamming_kernel, dim3(grid_for(n)), dim3(WG), 0, sct::as_stream(stream), kind, a,
                     b, n, words, out);
  SCT_LAUNCH_CHECK();
  return SCT_OK;
}

extern "C" int sct_base_frequency(const uint64_t* codes, int64_t n, int L, uint64_t* out,
                                  void* stream) {
  SCT_CHECK(n >= 0 && L >= 0 && L <= 1024, "bad n/L");
  SCT_CHECK(out != nullptr && (n == 0 || codes != nullptr), "NULL pointer");
  if (L == 0) return SCT_OK;
  hipStream_t s = sct::as_stream(stream);
  if (n == 0) {
    SCT_HIP(hipMemsetAsync(out, 0, (size_t)L * 4 * 8, s));  // no code: every count 0
    return SCT_OK;
  }
  // 64-bit form: >= 32 codes per lane before the wave / workgroup reduction (at 8 per lane, 3.7M
  // codes on 1,024 workgroups, that epilogue -- 24 64-bit wave reductions per wave -- was most of
  // the kernel).  32-bit form (L <= 16): rounds of 15 codes per lane, never more than 255
  int blocks = (int)std::min<int64_t>(sct::ceil_div(n, 32 * WG), 512);
  if (L <= 16) {
    // one round per lane (15 codes) measured best: 3.69M codes 15.6-17.7 us, two rounds 13.2-21.4,
    // three 17.5-19.4, the 64-bit kernel 23.2-27.6 (profiles/ab_basefreq16_r05.jsonl)
    blocks = (int)std::max<int64_t>(std::min<int64_t>(sct::ceil_div(n, 15 * WG), 4096), sct::ceil_div(n, 255 * WG));
  }
  void* part = nullptr;
  SCT_HIP(sct::pool_alloc(&part, (size_t)128 * blocks * 8, s));
  if (L <= 16)
    hipLaunchKernelGGL(base_frequency16_kernel, dim3(blocks), dim3(WG), 0, s, codes, n, (unsigned long long*)part);
  else
    hipLaunchKernelGGL(base_frequency_kernel, dim3(blocks), dim3(WG), 0, s, codes, n, (unsigned long long*)part);
  hipError_t le = hipGetLastError();
  if (le == hipSuccess)
    hipLaunchKernelGGL(base_frequency_reduce_kernel, dim3(128), dim3(WG), 0, s, (const unsigned long long*)part,
                       blocks, n, L, reinterpret_cast<unsigned long long*>(out));
  if (le == hipSuccess) le = hipGetLastError();
  sct::pool_free(part, s);
  if (le != hipSuccess) return sct::fail(SCT_E_HIP, "kernel launch: %s", hipGetErrorString(le));
  return SCT_OK;
}

