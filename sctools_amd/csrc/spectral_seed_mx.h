// SCT_ALLPAIRS_SPECTRAL, timing variant only (never in the product library): the int8 seed of 14-bit
// columns as int8 MFMA products.  Built into a side library by
//   bash tools/build_variant_lib.sh seedmx "-DSCT_SEED_MX_VARIANT=1"
// (every int8 plan on 14-bit columns then seeds through seed_mx_kernel) and timed / checked byte for
// byte against the product library by tools/seed_mx_ab.py.  It lost its A/B in round 9 (DESIGN.md
// Appendix A: the seed is bound by its 4 GiB of stores, which the Gray walk already reaches); it stays
// as the starting point for a seed that shares the chip with the tile.
#pragma once

#include <type_traits>

#include "spectral_seed.h"

namespace sct_spectral {

// ---------------------------------------------------------------- seed (int8) on the matrix cores
// The same bytes as a product of two +-1 matrices (14-bit columns, <= 127 codes per column).  Split
// the slice z = (r: bits 8..17, zm: bits 4..7, zn: bits 0..3) and every code's h = code >> 14 alike:
//   value(z, c) = sum_k s_k(r) (-1)^<zm, h_k[4..7]> (-1)^<zn, h_k[0..3]> = sum_k A_r[zm][k] B[k][zn],
//   s_k(r) = (-1)^<r, h_k[8..17]>,
// so one v_mfma_i32_16x16x64_i8 gives the 256 slices (zm, zn) of one r for a column's first 64 codes
// (bytes past the column's codes are 0 in A).  r runs a Gray walk inside a segment of 2^sb values:
// one bit b flips per step and A_r ^= PM_b (0xFE in the bytes of the codes with bit b of h[8..17]
// set: +1 <-> -1).  Operands come from the bit planes at workgroup start: lane l (row / column
// l & 15, codes 16 (l >> 4) .. + 15 of the block) reads the 16 plane bits of its codes, XORs the
// planes its row selects and spreads the 16 parity bits to bytes.
//
// Workgroup = 16 waves x 8 columns = 128 columns (one 128-B line per slice) x one segment.  Per step
// a wave packs the previous step's 8 accumulator tiles to bytes and writes them to the stage, then
// issues this step's A update and products and only then meets the barrier and stores the previous
// step out: the products run on the matrix pipe under the barrier and the stores, and the stage is
// double-buffered so one barrier per step is enough.  A column's codes 64.. (rare) add one product
// per step whose A is rebuilt from the block's planes (kept in LDS).
constexpr int kMxCols = 8;                          // columns per wave
constexpr int kMxWaves = 16;                        // waves per workgroup
constexpr int kMxRow = kMxCols * kMxWaves;          // columns (= stage row bytes) per workgroup
constexpr int kMxRows = 256;                        // slices per step: (zm, zn)
constexpr int kMxRowBits = 8;
constexpr int kMxMaxSegBits = 8;                    // r values per segment <= 256

// Ablations (-DSCT_SEED_MX_ABL=k, wrong results by design): 1 = products, A update and pack only (no
// stage, barrier or store); 2 = the same with the stage and its barrier, no global stores; 3 = the
// stores alone, from a constant stage; 5-9 = the stores alone in other shapes: rows of 128 (5, 6),
// 256 (7, 8) or 1,024 bytes (9) per workgroup, odd numbers non-temporal
#ifndef SCT_SEED_MX_ABL
#define SCT_SEED_MX_ABL 0
#endif
constexpr int kMxAbl = SCT_SEED_MX_ABL;

typedef long mx_v2l __attribute__((ext_vector_type(2)));
typedef int mx_v4i __attribute__((ext_vector_type(4)));

// ---- index arithmetic
// stage row of (accumulator register q, lane): zm = 4 (lane >> 4) + q, zn = lane & 15
__host__ __device__ constexpr int mx_stage_row(int lane, int q) { return (4 * (lane >> 4) + q) * 16 + (lane & 15); }
// a row's 16-B positions are XOR-permuted so the waves' 8-B writes spread over the banks
__host__ __device__ constexpr int mx_swz(int row) { return (row >> 1) & 7; }
// 8-B position of wave wv's piece inside stage row `row` (pairs of pieces stay in column order)
__host__ __device__ constexpr int mx_stage_pos8(int row, int wv) { return wv ^ (2 * mx_swz(row)); }
// first column (inside the workgroup's 128) of 16-B position u of stage row `row`
__host__ __device__ constexpr int mx_stage_col(int row, int u) { return 16 * (u ^ mx_swz(row)); }
// the plane bits of lane l's 16 codes of a 64-code block: group (l >> 5) of the block, shift 16 ((l >> 4) & 1)
__host__ __device__ constexpr int mx_lane_group(int lane) { return lane >> 5; }
__host__ __device__ constexpr int mx_lane_shift(int lane) { return 16 * ((lane >> 4) & 1); }
// segment bits for a range of nr r values: the largest power of two <= nr / 4, <= 2^kMxMaxSegBits
__host__ __device__ constexpr int mx_seg_bits(int nr) {
  int sb = 0;
  while (sb < kMxMaxSegBits && (8 << sb) <= nr) ++sb;
  return sb;
}

// bits 4 q .. 4 q + 3 of p as the low bits of four bytes
__device__ __forceinline__ uint32_t mx_spread(uint32_t p, int q) {
  return (((p >> (4 * q)) & 15u) * 0x00204081u) & 0x01010101u;
}
__device__ __forceinline__ mx_v2l mx_pack(const uint32_t* w) {
  return mx_v2l{(long)(((uint64_t)w[1] << 32) | w[0]), (long)(((uint64_t)w[3] << 32) | w[2])};
}
// 16 parity bits -> 16 bytes: +1 / -1 under `valid` (0 elsewhere); masks: 0xFE where the bit is set
__device__ __forceinline__ mx_v2l mx_signs(uint32_t par, uint32_t valid) {
  uint32_t w[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) w[q] = (mx_spread(par, q) * 0xFEu + 0x01010101u) & (mx_spread(valid, q) * 0xFFu);
  return mx_pack(w);
}
__device__ __forceinline__ mx_v2l mx_masks(uint32_t bits) {
  uint32_t w[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) w[q] = mx_spread(bits, q) * 0xFEu;
  return mx_pack(w);
}
// lane l's A_r and B bytes from the 18 planes pl of its 32-code group: m = the block's codes from
// the lane's first one on (<= 0: none), r = the slice bits 8.. folded into A (workgroup-uniform)
template <class C>
__device__ __forceinline__ void mx_operands(const uint32_t* pl, int lane, int m, int r, mx_v2l& A, mx_v2l& B) {
  const int lo = lane & 15, sh = mx_lane_shift(lane);
  uint32_t pa = 0, pb = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const uint32_t on = 0u - ((uint32_t)(lo >> b) & 1u);
    pa ^= pl[4 + b] & on;
    pb ^= pl[b] & on;
  }
#pragma unroll
  for (int b = 0; b < C::kHiBits - kMxRowBits; ++b)
    if ((r >> b) & 1) pa ^= pl[kMxRowBits + b];
  const uint32_t valid = (1u << min(max(m, 0), 16)) - 1u;
  A = mx_signs((pa >> sh) & 0xFFFFu, valid);
  B = mx_signs((pb >> sh) & 0xFFFFu, 0xFFFFu);
}

// the body of seed_mx_kernel (grid: kLo / 128 column blocks x segments of 2^sb r values, 1,024 threads)
template <class C>
__device__ __forceinline__ void seed_mx_body(const uint32_t* __restrict__ planes, const uint32_t* __restrict__ gofs,
                                             const uint32_t* __restrict__ off, int z0, int z1,
                                             int8_t* __restrict__ buf, int sb) {
  static_assert(C::kHiBits - kMxRowBits <= 10 && C::kPlaneWords % 4 == 0, "r bits / plane words");
  constexpr int PW = C::kPlaneWords;
  __shared__ mx_v2l pm_s[kMxMaxSegBits][kMxWaves][kMxCols][4];  // the walk's sign masks (codes 0..63)
  __shared__ uint4 stage[2][kMxRows * kMxRow / 16];             // double-buffered store-out
  __shared__ uint4 p1_s[kMxRow * 2 * PW / 4];                   // planes of the columns' codes 64..127
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, lo = lane & 15;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cw = blockIdx.x * kMxRow, c0 = cw + wv * kMxCols;
  const int ra = z0 >> kMxRowBits, rb = (z1 + kMxRows - 1) >> kMxRowBits;
  const int rs = ((ra >> sb) + (int)blockIdx.y) << sb, S = 1 << sb;
  const int grp = mx_lane_group(lane), sh = mx_lane_shift(lane);
  for (int e = tid; e < kMxRow * 2 * PW / 4; e += 64 * kMxWaves) {
    const int cc = e / (2 * PW / 4), gg = 2 + (e % (2 * PW / 4)) / (PW / 4), wd = e % (PW / 4);
    const uint32_t G0 = gofs[cw + cc];
    p1_s[e] = gg < (int)(gofs[cw + cc + 1] - G0)
                  ? reinterpret_cast<const uint4*>(planes + ((int64_t)G0 + gg) * PW)[wd]
                  : make_uint4(0u, 0u, 0u, 0u);
  }
  unsigned ovf = 0;  // the wave's columns of more than 64 codes
  mx_v2l A[kMxCols], B[kMxCols];
#pragma unroll
  for (int cc = 0; cc < kMxCols; ++cc) {
    const int c = c0 + cc, m = (int)(off[c + 1] - off[c]);
    const uint32_t G0 = gofs[c];
    ovf |= (unsigned)(m > 64) << cc;
    uint32_t pl[C::kHiBits];
    if (grp < (int)(gofs[c + 1] - G0)) {
      load_planes<C>(planes, (int64_t)G0 + grp, pl);
    } else {
#pragma unroll
      for (int k = 0; k < C::kHiBits; ++k) pl[k] = 0u;
    }
    mx_operands<C>(pl, lane, m - 16 * g, rs, A[cc], B[cc]);
    uint32_t v = 0;  // lane lo < sb: the mask of walked bit lo
#pragma unroll
    for (int b = 0; b < kMxMaxSegBits; ++b)
      if (lo == b) v = pl[kMxRowBits + b];
    if (lo < sb) pm_s[lo][wv][cc][g] = mx_masks((v >> sh) & 0xFFFFu);
    __builtin_amdgcn_sched_barrier(0);  // one column's planes in registers at a time
  }
  __syncthreads();
  // the segment's walk; kOvf: the wave has columns of more than 64 codes (a code path of its own, so
  // the common one carries none of its registers; both meet the same barriers)
  auto walk = [&](auto has_ovf) {
    constexpr bool kOvf = decltype(has_ovf)::value;
    // (new values here: the allocator then keeps the operands in registers through this walk
    // whatever it did with them during the set-up or does in the other walk)
#pragma unroll
    for (int cc = 0; cc < kMxCols; ++cc) asm volatile("" : "+v"(A[cc]), "+v"(B[cc]));
    mx_v4i acc[kMxCols] = {};
    int rprev = -1;
    unsigned n = 0;
    uint32_t sink = 0;  // (ablations)
#pragma unroll 1
    for (int i = 0; i <= S; ++i) {
      uint4* stg = stage[n & 1];
      if (rprev >= 0 && kMxAbl < 3) {
        // [row 4 g + q][columns 4 k .. 4 k + 3]: the products' low bytes, to the lane's stage pieces
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          uint32_t w[kMxCols / 4];
#pragma unroll
          for (int k = 0; k < kMxCols / 4; ++k)
            w[k] = __builtin_amdgcn_perm((uint32_t)acc[4 * k + 1][q], (uint32_t)acc[4 * k][q], 0x0c0c0400u) |
                   __builtin_amdgcn_perm((uint32_t)acc[4 * k + 3][q], (uint32_t)acc[4 * k + 2][q], 0x04000c0cu);
          const int row = mx_stage_row(lane, q);
          if constexpr (kMxAbl == 1) sink ^= w[0] ^ w[1];
          else reinterpret_cast<uint2*>(stg)[row * (kMxRow / 8) + mx_stage_pos8(row, wv)] = make_uint2(w[0], w[1]);
        }
        if constexpr (kOvf) {
          for (unsigned ov = ovf; ov; ov &= ov - 1) {  // codes 64..: one more product, added to the lane's bytes
            const int cc = __builtin_ctz(ov), c = c0 + cc;
            const uint4* src = p1_s + ((wv * kMxCols + cc) * 2 + grp) * (PW / 4);
            uint32_t pw[PW];
#pragma unroll
            for (int k = 0; k < PW / 4; ++k) {
              const uint4 t = src[k];
              pw[4 * k] = t.x;
              pw[4 * k + 1] = t.y;
              pw[4 * k + 2] = t.z;
              pw[4 * k + 3] = t.w;
            }
            mx_v2l A1, B1;
            mx_operands<C>(pw, lane, (int)(off[c + 1] - off[c]) - 64 - 16 * g, rprev, A1, B1);
            const mx_v4i a1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(A1, B1, mx_v4i{0, 0, 0, 0}, 0, 0, 0);
            uint8_t* st8 = reinterpret_cast<uint8_t*>(stg);
#pragma unroll
            for (int q = 0; q < 4; ++q) {  // |sum| <= 127: the byte sum modulo 256 is exact
              const int row = mx_stage_row(lane, q);
              st8[row * kMxRow + 8 * mx_stage_pos8(row, wv) + cc] += (uint8_t)a1[q];
            }
          }
        }
      }
      // this step's A and products only now: the accumulators are free again
      __builtin_amdgcn_sched_barrier(0);
      int r = -1;
      if (i < S) {
        if (i && kMxAbl < 3) {
          const int bb = __builtin_ctz(i);
#pragma unroll
          for (int cc = 0; cc < kMxCols; ++cc) {
            A[cc] ^= pm_s[bb][wv][cc][g];
            if (cc % 4 == 3) __builtin_amdgcn_sched_barrier(0);  // four masks in flight, not eight
          }
        }
        const int rr = rs ^ (i ^ (i >> 1));
        if (rr >= ra && rr < rb) r = rr;
      }
      if (r >= 0 && kMxAbl < 3)
#pragma unroll
        for (int cc = 0; cc < kMxCols; ++cc)
          acc[cc] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[cc], B[cc], mx_v4i{0, 0, 0, 0}, 0, 0, 0);
      if (rprev >= 0 && kMxAbl != 1) {
        if constexpr (kMxAbl < 3) __syncthreads();
#pragma unroll
        for (int t = 0; t < kMxRows * kMxRow / 16 / (64 * kMxWaves); ++t) {
          const int e = t * 64 * kMxWaves + tid, row = e / (kMxRow / 16), z = rprev * kMxRows + row;
          if constexpr (kMxAbl == 2) {
            const uint4 v = stg[e];
            sink ^= v.x ^ v.y ^ v.z ^ v.w;
          } else if constexpr (kMxAbl >= 5) {  // stores alone in other shapes: rows of RB bytes, non-temporal
            constexpr int RB = kMxAbl <= 6 ? 128 : (kMxAbl <= 8 ? 256 : 1024), G = RB / 128, U = RB / 16;
            const int j = blockIdx.x % G, zz = rprev * kMxRows + j * (kMxRows / G) + e / U;
            const uint4 v = stg[e];
            v4u_t* dst = reinterpret_cast<v4u_t*>(buf + (int64_t)(zz - z0) * C::kLo + (blockIdx.x / G) * RB + 16 * (e % U));
            if (zz >= z0 && zz < z1) {
              if constexpr (kMxAbl % 2 == 1) __builtin_nontemporal_store(v4u_t{v.x, v.y, v.z, v.w}, dst);
              else *dst = v4u_t{v.x, v.y, v.z, v.w};
            }
          } else if (z >= z0 && z < z1) {
            *reinterpret_cast<uint4*>(buf + (int64_t)(z - z0) * C::kLo + cw + mx_stage_col(row, e % (kMxRow / 16))) =
                stg[e];
          }
        }
        ++n;
      }
      rprev = r;
    }
    if constexpr (kMxAbl == 1 || kMxAbl == 2)
      if (sink == 0x12345678u && z1 < 0) *reinterpret_cast<uint32_t*>(buf) = sink;
  };
  if (ovf) walk(std::true_type());
  else walk(std::false_type());
}

// the same slices by the matrix form (seed_mx_kernel): segments of 2^sb r values (256 slices each),
// aligned on the absolute r, at least four per range where it has that many
template <class C, class Kernel>
int launch_seed_mx(Kernel kernel, State& st, int8_t* buf, int z0, int z1, hipStream_t s) {
  const int ra = z0 >> kMxRowBits, rb = (z1 + kMxRows - 1) >> kMxRowBits;
  const int sb = mx_seg_bits(rb - ra);
  const int nseg = ((rb - 1) >> sb) - (ra >> sb) + 1;
  hipLaunchKernelGGL(kernel, dim3(C::kLo / kMxRow, (unsigned)nseg), dim3(64 * kMxWaves), 0, s, st.d_planes, st.d_gofs,
                     st.d_off, z0, z1, buf, sb);
  SCT_LAUNCH_CHECK();
  return SCT_OK;
}

}  // namespace sct_spectral
