// Spectral all-pairs scheme: the TwoBit distance histogram of n 16-base codes from the
// Walsh-Hadamard transform of their multiplicity f over Z_2^32.
//
//   d(x, y) = digit weight of x ^ y (non-zero 2-bit digits), so the ordered-pair counts
//   N(d) = sum_{v : wt(v) = d} R(v), R = f (*) f (XOR autocorrelation), and with
//   F = WHT(f):  N(d) = 2^-32 sum_z F(z)^2 K_d(wt(z)),  K_d the q = 4 Krawtchouk
//   polynomial.  The device computes S_w = sum_{wt(z) = w} F(z)^2 (17 uint64); the host
//   (sct_counts_to_hist_ex) applies K and halves: hist[d] = (N(d) - n [d = 0]) / 2.
//
// z = (slice z >> 14, column z & 0x3FFF); the 2^18 slices are the plan's work items.
//   seed   F's partial sums over the high 18 bits, per column, from bit planes of the
//          column's codes: a Gray-code walk over 64 slices costs one XOR and one
//          popcount per 32 codes per value.  |seed| <= codes in the column, so the
//          values go to HBM as int8 (int16 / int32 for denser columns): 16 KB per slice
//   tile   reads a slice back, transforms it over the 14 column bits (int8 seeds: two
//          64-point stages on the matrix cores + Parseval for the top digit), F^2 binned
//          by digit weight; writes nothing
// 8 GB of HBM traffic per job at int8, whatever n is.  Exact: |F| <= n <= 1e8 in int32,
// F^2 in uint64, S_w in three non-carrying limbs (spectral.h: sum_w S_w = 2^32 sum f^2 exceeds
// 2^64 for multisets with sum f^2 >= 2^32).
#include <string.h>

#include <algorithm>
#include <vector>
#include <type_traits>

#include <mutex>

#include <hipcub/hipcub.hpp>

#include "sct_common.h"
#include "spectral.h"
#include "spectral_seed.h"
#ifdef SCT_SEED_MX_VARIANT
#include "spectral_seed_mx.h"
#endif

namespace sct_spectral {
namespace {

using Cols = Columns<kLoBits>;
constexpr int kLo = Cols::kLo;            // columns (= tile values)
constexpr int kHiBits = Cols::kHiBits;    // 18 bit planes
constexpr int kRegGroups = 2;             // int16 / int32 seeds: groups whose planes stay in registers
constexpr int kMaxOrder = 1 << 16;        // largest slice range with a digit-weight order table

// in-register WHT of N values
template <int N>
__device__ __forceinline__ void wht(int32_t* x) {
#pragma unroll
  for (int h = 1; h < N; h <<= 1)
#pragma unroll
    for (int i = 0; i < N; ++i)
      if (!(i & h)) {
        const int32_t a = x[i], b = x[i | h];
        x[i] = a + b;
        x[i | h] = a - b;
      }
}

// Privatised counting sort (the build of every step; no global atomics):
//   hist_wg   workgroup g counts its contiguous share of the codes per column in LDS and
//             writes the 2^14 counts to H[g][.]
//   prefix    per column: H[g][c] <- sum of H[g' < g][c] (in place), m(c) = the total
//   scan      one workgroup: off / gofs = exclusive scans of m(c) and ceil(m(c) / 32)
//   scatter   workgroup g: LDS cursors off[c] + H[g][c], one LDS atomic per code
constexpr int kSortWGs = 128;
constexpr int kSortThreads = 1024;

__global__ __launch_bounds__(kSortThreads) void column_hist_wg_kernel(const uint64_t* __restrict__ codes, int64_t n,
                                                                      uint32_t* __restrict__ H) {
  __shared__ uint32_t h[kLo];
  for (int c = threadIdx.x; c < kLo; c += kSortThreads) h[c] = 0;
  __syncthreads();
  int64_t b, e;
  wg_range(n, b, e);
  for (int64_t i = b + threadIdx.x; i < e; i += kSortThreads) atomicAdd(&h[codes[i] & (kLo - 1)], 1u);
  __syncthreads();
  uint32_t* out = H + (int64_t)blockIdx.x * kLo;
  for (int c = threadIdx.x; c < kLo; c += kSortThreads) out[c] = h[c];
}

__global__ __launch_bounds__(256) void column_prefix_kernel(uint32_t* __restrict__ H, int wgs,
                                                            uint32_t* __restrict__ m) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  uint32_t run = 0;
#pragma unroll 8
  for (int g = 0; g < wgs; ++g) {
    const uint32_t v = H[(int64_t)g * kLo + c];
    H[(int64_t)g * kLo + c] = run;
    run += v;
  }
  m[c] = run;
}

// one workgroup of 1024: 16 columns per thread, wave scans + one LDS pass over the waves
__global__ __launch_bounds__(1024) void column_scan16_kernel(const uint32_t* __restrict__ m,
                                                             uint32_t* __restrict__ off,
                                                             uint32_t* __restrict__ gofs) {
  __shared__ uint32_t wsum[2][16];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  uint32_t v[16];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint4 q = reinterpret_cast<const uint4*>(m)[t * 4 + k];
    v[4 * k] = q.x;
    v[4 * k + 1] = q.y;
    v[4 * k + 2] = q.z;
    v[4 * k + 3] = q.w;
  }
  uint32_t s = 0, sg = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    s += v[k];
    sg += (v[k] + 31) / 32;
  }
  uint32_t is = s, isg = sg;  // inclusive scans over the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t a = __shfl_up(is, d), ag = __shfl_up(isg, d);
    if (lane >= d) {
      is += a;
      isg += ag;
    }
  }
  if (lane == 63) {
    wsum[0][wave] = is;
    wsum[1][wave] = isg;
  }
  __syncthreads();
  uint32_t base = 0, baseg = 0;
  for (int w = 0; w < wave; ++w) {
    base += wsum[0][w];
    baseg += wsum[1][w];
  }
  uint32_t run = base + is - s, rung = baseg + isg - sg;
  uint32_t o[16], og[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    o[k] = run;
    og[k] = rung;
    run += v[k];
    rung += (v[k] + 31) / 32;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    reinterpret_cast<uint4*>(off)[t * 4 + k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
    reinterpret_cast<uint4*>(gofs)[t * 4 + k] = make_uint4(og[4 * k], og[4 * k + 1], og[4 * k + 2], og[4 * k + 3]);
  }
  if (t == 1023) {
    off[kLo] = run;
    gofs[kLo] = rung;
  }
}

__global__ __launch_bounds__(kSortThreads) void column_scatter_wg_kernel(const uint64_t* __restrict__ codes,
                                                                         int64_t n,
                                                                         const uint32_t* __restrict__ H,
                                                                         const uint32_t* __restrict__ off,
                                                                         uint32_t* __restrict__ hi) {
  __shared__ uint32_t cur[kLo];
  const uint32_t* pre = H + (int64_t)blockIdx.x * kLo;
  for (int c = threadIdx.x; c < kLo; c += kSortThreads) cur[c] = off[c] + pre[c];
  __syncthreads();
  int64_t b, e;
  wg_range(n, b, e);
  for (int64_t i = b + threadIdx.x; i < e; i += kSortThreads) {
    const uint64_t x = codes[i];
    hi[atomicAdd(&cur[x & (kLo - 1)], 1u)] = (uint32_t)(x >> kLoBits);
  }
}

// group g's planes (load_planes layout)
__global__ void planes_kernel(const uint32_t* __restrict__ hi, const uint32_t* __restrict__ off,
                              const uint32_t* __restrict__ gofs, int64_t max_groups,
                              uint32_t* __restrict__ planes) {
  const int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (g >= (int64_t)gofs[kLo]) return;
  int a = 0, b = kLo;  // column c: gofs[c] <= g < gofs[c + 1]
  while (b - a > 1) {
    const int m = (a + b) >> 1;
    if (gofs[m] <= (uint32_t)g) a = m;
    else b = m;
  }
  const uint32_t first = off[a] + 32u * ((uint32_t)g - gofs[a]);
  const uint32_t last = min(first + 32u, off[a + 1]);
  uint32_t p[kHiBits];
#pragma unroll
  for (int k = 0; k < kHiBits; ++k) p[k] = 0;
  for (uint32_t i = first; i < last; ++i) {
    const uint32_t h = hi[i], bit = 1u << (i - first);
#pragma unroll
    for (int k = 0; k < kHiBits; ++k) p[k] |= (h >> k) & 1u ? bit : 0u;
  }
  store_planes<Cols>(planes, g, p);
}

typedef unsigned v4u __attribute__((ext_vector_type(4)));

// Value type of the seed -> tile intermediate: |seed| <= codes in the column, so the
// densest column decides (int8 for whitelists up to ~1.2M random barcodes).
template <typename T>
struct Chunk {
  static constexpr int kVals = 16 / sizeof(T);                  // columns per 16-B chunk
  static constexpr int kLog = sizeof(T) == 1 ? 4 : (sizeof(T) == 2 ? 3 : 2);
  static constexpr int kPerThread = 64 / kVals;                 // chunks per tile thread
};

// Position of column c inside a slice row of the intermediate.  Chosen so that the tile
// kernel's thread t, reading 16-B chunks at t*kVals + j*2^(kLog+8), receives the columns
// with bits 4..11 = t and registers q = column bits 0..3 + 16 * bits 12, 13, whatever T is.
template <typename T>
__device__ __forceinline__ int column_pos(int c) {
  constexpr int L = Chunk<T>::kLog;
  return (c & ((1 << L) - 1)) | (((c >> 4) & 255) << L) | (((c >> L) & ((16 >> L) - 1)) << (L + 8)) |
         ((c >> 12) << 12);
}


// int16 / int32 seeds (columns of more than 127 codes): a workgroup owns 256 columns and walks of
// 64 slices (blockIdx.y, strided): each lane walks its column in Gray order (one XOR per step
// from registers) group by group into a 64-value accumulator array; dwords of 4 / sizeof(T)
// consecutive slices per column are staged in LDS, transposed in registers and written as 16-B
// chunks of slice rows.  (int8 seeds: seed_sm_kernel below.)
template <typename T>
__device__ __forceinline__ void seed_body(const uint32_t* __restrict__ planes, const uint32_t* __restrict__ gofs,
                                          const uint32_t* __restrict__ off, int z0, int z1, T* __restrict__ buf) {
  constexpr int NT = 256;
  constexpr int P = 4 / sizeof(T);          // slices per staged dword
  constexpr int V = Chunk<T>::kVals;        // columns per 16-B output chunk
  __shared__ uint32_t stage[(kWalk / P) * NT];
  const int tid = threadIdx.x;
  const int c0 = blockIdx.x * NT, c = c0 + tid;
  const int m = (int)(off[c + 1] - off[c]);
  const uint32_t g0 = gofs[c];
  const int ng = (int)(gofs[c + 1] - g0);
  int wng = ng;
#pragma unroll
  for (int s = 32; s; s >>= 1) wng = max(wng, __shfl_xor(wng, s));
  // the first kRegGroups groups' planes stay in registers for all of this workgroup's walks
  uint32_t pr[kRegGroups][kHiBits];
#pragma unroll
  for (int g = 0; g < kRegGroups; ++g)
    if (g < ng) {
      load_planes<Cols>(planes, (int64_t)g0 + g, pr[g]);
    } else {
#pragma unroll
      for (int k = 0; k < kHiBits; ++k) pr[g][k] = 0u;
    }
  // Co-resident workgroups start together and run identical walks, so they stay in
  // lockstep: all 12 waves of a CU walk (VALU-bound) and then all store (HBM-bound).
  // Starting them 0 / 1,536 / 3,072 cycles apart lets one workgroup's stores drain under
  // another's walk (What was tried (14)).
  {
    const int ph = (blockIdx.x + blockIdx.y) % 3;
    if (ph >= 1) __builtin_amdgcn_s_sleep(24);
    if (ph == 2) __builtin_amdgcn_s_sleep(24);
  }
  const int za = z0 & ~(kWalk - 1);
  const int nwalks = (z1 - za + kWalk - 1) / kWalk;
  for (int wk = blockIdx.y; wk < nwalks; wk += gridDim.y) {
    const int zblk = za + wk * kWalk;
    int acc[kWalk];
    auto walk = [&](const uint32_t* p, auto first) {
      uint32_t x = 0;
#pragma unroll
      for (int k = kWalkBits; k < kHiBits; ++k)
        if ((zblk >> k) & 1) x ^= p[k];
      if constexpr (decltype(first)::value) acc[0] = __popc(x);
      else acc[0] += __popc(x);
#pragma unroll
      for (int i = 1; i < kWalk; ++i) {
        x ^= p[ctz_c(i)];
        if constexpr (decltype(first)::value) acc[gray(i)] = __popc(x);
        else acc[gray(i)] += __popc(x);
      }
    };
    walk(pr[0], std::true_type());  // columns without codes: planes 0, popc 0
#pragma unroll
    for (int g = 1; g < kRegGroups; ++g)
      if (g < wng) walk(pr[g], std::false_type());
    for (int g = kRegGroups; g < wng; ++g) {  // dense columns: the rest from L2
      uint32_t p[kHiBits];
      if (g < ng) {
        load_planes<Cols>(planes, (int64_t)g0 + g, p);
      } else {
#pragma unroll
        for (int k = 0; k < kHiBits; ++k) p[k] = 0u;
      }
      walk(p, std::false_type());
    }
    {
      __syncthreads();  // the previous walk's store-out reads of `stage` are done
      // 4-dword groups of a 16-dword column block XOR-swizzled by the block, so the
      // store-out's b128 reads of 16 consecutive columns are conflict-free
      auto sidx = [](int row, int col) { return row * 256 + (col ^ (((col >> 6) & 3) << 2)); };
#pragma unroll
      for (int r = 0; r < kWalk / P; ++r) {
        uint32_t w = 0;
#pragma unroll
        for (int j = 0; j < P; ++j)
          w |= ((uint32_t)(m - 2 * acc[r * P + j]) & (0xFFFFFFFFu >> (32 - 8 * sizeof(T)))) << (8 * sizeof(T) * j);
        stage[sidx(r, tid)] = w;
      }
      __syncthreads();
      // blocks of V columns x P slices: V dwords in, P chunks out
      constexpr int kBlocks = (kWalk / P) * (256 / V);
#pragma unroll
      for (int r = 0; r < kBlocks / 256; ++r) {
        const int b = tid + 256 * r, row = b / (256 / V), cb = (b % (256 / V)) * V;
        uint32_t d[V];
#pragma unroll
        for (int k = 0; k < V; k += 4) {
          const uint4 v = *reinterpret_cast<const uint4*>(stage + sidx(row, cb + k));
          d[k] = v.x;
          d[k + 1] = v.y;
          d[k + 2] = v.z;
          d[k + 3] = v.w;
        }
        uint32_t out[P][4];
        if constexpr (P == 2) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            out[0][k] = __builtin_amdgcn_perm(d[2 * k + 1], d[2 * k], 0x05040100u);
            out[1][k] = __builtin_amdgcn_perm(d[2 * k + 1], d[2 * k], 0x07060302u);
          }
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) out[0][k] = d[k];
        }
#pragma unroll
        for (int j = 0; j < P; ++j) {
          const int z = zblk + row * P + j;
          if (z < z0 || z >= z1) continue;
          *reinterpret_cast<uint4*>(buf + (int64_t)(z - z0) * kLo + column_pos<T>(c0 + cb)) =
              make_uint4(out[j][0], out[j][1], out[j][2], out[j][3]);
        }
      }
    }
  }
}

// int8 seeds: the step-major walk shared with the 16-bit columns (seed_sm_body, spectral_seed.h).
// 96 VGPRs: 5 waves per SIMD (the Gray-block state costs two more registers; at this bound the
// compiler spills one 8-byte value, reloaded once per walk)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void seed_sm_kernel(
    const uint32_t* __restrict__ planes, const uint32_t* __restrict__ gofs, const uint32_t* __restrict__ off, int z0,
    int z1, int8_t* __restrict__ buf, int lp) {
  seed_sm_body<Cols>(planes, gofs, off, z0, z1, buf, lp);
}

#ifdef SCT_SEED_MX_VARIANT
// timing variant: int8 seeds as int8 MFMA products (seed_mx_body, spectral_seed_mx.h): 16 waves, 4 per SIMD
__global__ __launch_bounds__(64 * kMxWaves) void seed_mx_kernel(const uint32_t* __restrict__ planes,
                                                                const uint32_t* __restrict__ gofs,
                                                                const uint32_t* __restrict__ off, int z0, int z1,
                                                                int8_t* __restrict__ buf, int sb) {
  seed_mx_body<Cols>(planes, gofs, off, z0, z1, buf, sb);
}
#endif

template <typename T>
__global__ __launch_bounds__(256) void seed_kernel(const uint32_t* __restrict__ planes,
                                                   const uint32_t* __restrict__ gofs,
                                                   const uint32_t* __restrict__ off, int z0, int z1,
                                                   T* __restrict__ buf) {
  seed_body<T>(planes, gofs, off, z0, z1, buf);
}

// LDS word of column e in the tile kernel: bits 2, 3, 4 XORed with bits 6, 5, 10, so the
// phase-1 b128 stores (8-lane groups: e bits 4..6 vary) and the phase-2 b32 loads (32-lane
// groups: e bits 0..3, 10 vary) are both conflict-free.
__device__ __forceinline__ int swz(int e) {
  return e ^ (((e >> 6) & 1) << 2) ^ (((e >> 5) & 1) << 3) ^ (((e >> 10) & 1) << 4);
}

// Butterfly over a lane bit without LDS: v_permlane{32,16}_swap brings the partner lane's
// value of register a into this lane's b (and b's into the partner), so the pair is
// combined in-lane.  Afterwards the lane bit and the register bit that told a from b have
// traded places.
__device__ __forceinline__ void lane_butterfly32(int32_t& a, int32_t& b) {
  const auto r = __builtin_amdgcn_permlane32_swap((unsigned)a, (unsigned)b, false, false);
  a = (int32_t)(r[0] + r[1]);
  b = (int32_t)(r[0] - r[1]);
}
__device__ __forceinline__ void lane_butterfly16(int32_t& a, int32_t& b) {
  const auto r = __builtin_amdgcn_permlane16_swap((unsigned)a, (unsigned)b, false, false);
  a = (int32_t)(r[0] + r[1]);
  b = (int32_t)(r[0] - r[1]);
}

// int16 / int32 seeds (columns of more than 127 codes: dense sets and multisets with heavy
// duplicates): per slice the WHT over the 14 column bits on the VALU, then S_w += F^2 by digit
// weight.  Persistent: workgroups stride over the chunk's slices.  Here sum_w S_w = 2^32 sum f^2
// can exceed 2^64, so every lane's per-slice sum (64 squares < 2^54 each: n <= 1e8) goes to the
// LDS bins as its two 32-bit halves (bins_lo / bins_hi never carry: < 2^26 adds each) and the
// bins to the counts' three limbs (add_weight_sum).
//   phase 1  registers q = e bits 0..3 + 16 * (12, 13); thread = e bits 4..11
//   phase 2  registers q = e bits 4..9;  lane = e bits 0..3, 10, 11; wave = e bits 12, 13
//   phase 3  lane bits 5, 4 (e 11, 10) by permlane swaps against q bits 1, 0 (e 5, 4):
//            then q = (e 10, 11, 6..9), lane = e bits 0..5, wave = e bits 12, 13 -- whole
//            2-bit digits, so an element's digit weight is thread constant + compile time.
template <typename T>
__global__ __launch_bounds__(256) void tile_kernel(const T* __restrict__ buf, int z0, int nslices,
                                                   unsigned long long* __restrict__ counts,
                                                   unsigned long long add_n,
                                                   const unsigned long long* __restrict__ sumsq) {
  static_assert(sizeof(T) >= 2, "int8 seeds take tile_reg_kernel");
  __shared__ int32_t lds[kLo];
  __shared__ unsigned long long bins_lo[17], bins_hi[17];
  constexpr int V = Chunk<T>::kVals, L = Chunk<T>::kLog;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < 17) bins_lo[tid] = bins_hi[tid] = 0;
  const int t2 = (lane & 15) | ((lane >> 4) << 10) | (wave << 12);  // phase-2 e base
  const int wt_thread = digit_weight((uint32_t)lane | ((uint32_t)wave << 12));
  for (int s = blockIdx.x; s < nslices; s += gridDim.x) {
    const T* row = buf + (int64_t)s * kLo;
    int32_t x[64];
#pragma unroll
    for (int j = 0; j < Chunk<T>::kPerThread; ++j) {
      const v4u v = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(row + tid * V + (j << (L + 8))));
      const T* e = reinterpret_cast<const T*>(&v);
#pragma unroll
      for (int r = 0; r < V; ++r) x[j * V + r] = e[r];
    }
    wht<64>(x);
    __syncthreads();  // the previous slice's phase-2 reads are done
#pragma unroll
    for (int q = 0; q < 64; q += 4)
      *reinterpret_cast<int4*>(lds + swz((q & 15) | (tid << 4) | ((q >> 4) << 12))) =
          make_int4(x[q], x[q + 1], x[q + 2], x[q + 3]);
    __syncthreads();
    const int a2 = swz(t2);
#pragma unroll
    for (int q = 0; q < 64; ++q) x[q] = lds[a2 ^ swz(q << 4)];
    wht<64>(x);
#pragma unroll
    for (int q = 0; q < 64; ++q)
      if (!(q & 2)) lane_butterfly32(x[q], x[q | 2]);  // e bit 11 <-> q bit 1 (e bit 5)
#pragma unroll
    for (int q = 0; q < 64; ++q)
      if (!(q & 1)) lane_butterfly16(x[q], x[q | 1]);  // e bit 10 <-> q bit 0 (e bit 4)
    unsigned long long acc[4] = {0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < 64; ++q)
      acc[digit_weight_c((uint32_t)(q & 3)) + digit_weight_c((uint32_t)(q >> 2))] +=
          (unsigned long long)((int64_t)x[q] * x[q]);
    const int w0 = digit_weight((uint32_t)(z0 + s)) + wt_thread;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (acc[k] & 0xFFFFFFFFull) atomicAdd(&bins_lo[w0 + k], acc[k] & 0xFFFFFFFFull);
      if (acc[k] >> 32) atomicAdd(&bins_hi[w0 + k], acc[k] >> 32);
    }
  }
  __syncthreads();
  if (tid < 17) add_weight_sum(counts, tid, bins_lo[tid], bins_hi[tid]);
  add_job_constants(counts, add_n, sumsq);
}

typedef int v4i_t __attribute__((ext_vector_type(4)));
typedef short v2s_t __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------- register-resident tile (int8 seeds)
// One WAVE transforms one whole slice with no LDS exchange and no barrier, on
// v_mfma_i32_32x32x32_i8 (operands: A row / B column = l & 31, k = 16 (l >> 5) + j; C rows
// 8 (i >> 2) + 4 (l >> 5) + (i & 3), column l & 31).  The 12 column bits of a plane R (bits 12,
// 13) split into a stage-1 set P = {0, 1, 2, 3, 4, 10} and a stage-2 set Q = {5, 6, 7, 8, 9, 11},
// which do not follow the 2-bit digits: what matters is that after both stages three whole
// digits are lane bits and three are register / tile indices.
//   loads: lane l's 16 B hold column bits 0..3 = j, 4 = l bit 5, 5 = l bit 3, 6, 7 = l bits 0, 1,
//     8 = l bit 4, 9 = l bit 2; load (mt, ks) of plane R adds 1024 ks + 2048 mt + 4096 R: every
//     load instruction of a wave reads one whole contiguous KiB of the slice.
//   stage 1 (per plane): the bytes are the A operand as loaded (row m = l & 31: five Q bits, the
//     sixth = mt; k = 16 (l >> 5) + j + 32 ks = P) against B = H_64 (column n = l & 31 + 32 nt):
//     C1[m][n] = sum_P D * H, two chained K-steps ks per (nt, mt) tile.  Transformed P' = n:
//     lane bits 0..4 = column bits 0..4, nt = bit 10.  A lane's 16 outputs are rows (m bits
//     0, 1, 3, 4) = i and m bit 2 = l >> 5: exactly stage 2's B operand (k = 16 (l >> 5) + i
//     + 32 mt, a relabeling of Q), packed into bytes in registers.
//   stage 2: H_64 over Q (A = the same H registers, K-steps = stage 1's M-tiles mt).  |v + 128|
//     < 2^15 needs two bytes: with y = v + 128 = 256 h + l', v = 256 h + (l' - 128), so H v =
//     (H h << 8) + H (l' - 128): the high bytes' chain of two MFMAs, one shift of its 16
//     results, then the low bytes' chain into that accumulator.  The byte split goes through
//     int16 pairs (one v_perm packs two stage-1 outputs), which are also what the plane sums
//     accumulate (v_pk_add_u16; the sum over the planes of v + 128 from -384 stays within
//     +-32,640).  Output row bit t is the column bit of B's k bit t: i bits 0, 1 = column bits
//     6, 7; l >> 5 = bit 5; i bits 2, 3 = bits 8, 9; the M-tile = bit 11.
//   R (one base digit) by Parseval instead of a butterfly: with G_R = the 12-bit transform of
//     plane R and F(R') = sum_R (-1)^<R, R'> G_R,  F(0) = transform of sum_R D_R = sum_R C1_R
//     (added after stage 1) and sum_{R' != 0} F(R')^2 = 4 sum_R G_R^2 - F(0)^2.  So every
//     (P', Q') adds F(0)^2 to weight w and 4 sum G_R^2 - F(0)^2 to weight w + 1: five stage-2
//     transforms per slice (4 planes + the sum), no exchange between planes.
//   Half step: stage 2 is H_2 x H_32 with column bit 11 outermost (M-tile t out, K-step ks in):
//     the M-tiles are U + V and U - V for U = H_32 B[0], V = H_32 B[1].  Bits (10, 11) are one
//     digit of value nt + 2 t: for nt = 1 it is 1 or 3, non-zero either way, so both M-tiles fall
//     into one bin, which needs only (U + V)^2 + (U - V)^2 = 2 (U^2 + V^2).  N-tile 1 therefore
//     stops at U and V -- two chains of two MFMAs on the +H_32 block (high and low byte of one
//     K-step) instead of two of four -- and its squares count twice (integers throughout: the
//     histogram is bit for bit what the full butterfly gives).  N-tile 0 (digit 0 or 2: two
//     bins) keeps the butterfly.
//   Per plane 8 + 16 MFMAs by the tiling (one N-tile nt at a time, its two chains interleaved),
//     per slice 4 * 8 + 5 * 16 = 112; 79 issued: the half step takes 4 from each of the five
//     N-tile-1 calls and equal H blocks 13 more (see H below: 5 in N-tile 0, 8 in stage 1).  Stage 1 of
//     both N-tiles runs before either stage 2, so N-tile 1 waits as 16 VGPRs of int16 pairs,
//     not as 32 of shared first K-step + 8 of bytes.  The next plane's loads are in
//     flight while this one is transformed -- across slices too: the next slice's first plane
//     is loaded during this slice's last plane and the plane-sum transforms.
// Weight of (P', Q', R'): digits (0, 1), (2, 3), (4, 5) = l & 3, (l >> 2) & 3, l >> 4 (thread
// constant) + digits (6, 7), (8, 9), (10, 11) = i & 3, i >> 2, nt + 2 M-tile (compile time) +
// the slice's + [R' != 0].  Each wave of the grid takes a contiguous run
// of slice positions; position u is slice order[u] (a whole aligned chunk sorted by digit
// weight, so the run's weight changes rarely and F^2 is binned in registers) or u.
//   Chain (plans whose densest column holds <= kChainMaxM codes): the per-plane stage 2 without
//     the shift.  |v| <= 64 m <= 8000, so y = v + 128 is in [-7872, 8128], h in [-31, 31] and 4 h
//     fits a byte: H v = (64 H) (4 h) + H (l' - 128), the high K-steps on A = 64 H (bytes 0x40 /
//     0xC0) against B = 4 h = (Bh << 2) & 0xFCFCFCFC (the mask drops the two bits the dword shift
//     carries into each byte from its neighbour), all K-steps one MFMA chain into one accumulator
//     with no vector instruction between them.  (m = 126: y reaches 8192, 4 h = 128.)  The
//     plane sums (|h| up to 127) keep the shift form.
typedef int v16i_t __attribute__((ext_vector_type(16)));
constexpr unsigned kChainMaxM = 125;
template <bool Chain>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void tile_reg_kernel(
    const int8_t* __restrict__ buf, const uint16_t* __restrict__ order, int z0, int nslices,
    unsigned long long* __restrict__ counts, unsigned long long add_n, const unsigned long long* __restrict__ sumsq) {
  // int8 seeds: every column holds <= 127 codes, so sum_w S_w = 2^32 sum f^2 <= 2^32 * 2^14 * 127^2
  // < 2^62 and 64-bit register / LDS sums cannot wrap
  __shared__ unsigned long long bins[17];
  // (the wave index through readfirstlane: the slice run, its loop and the order lookups
  // become scalar)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (tid < 17) bins[tid] = 0;
  __syncthreads();
  // H_64 rows 32 t + (l & 31), columns 32 ks + 16 (l >> 5) + j: stage 1's B (N-tile t) and
  // stage 2's A (M-tile t), K-step ks.  H_64 = H_2 x H_32: the four blocks are H_32 and, for
  // t = ks = 1, -H_32.  (So tiles t = 0 and 1 share the MFMA of a chain's first K-step when they
  // start from the same accumulator, and the compiler issues it once.)
  v4i_t H[2][2];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    uint32_t v = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = lane & 31, col = 16 * (lane >> 5) + 4 * d + r;
      v |= ((__popc(row & col) & 1) ? 0xFFu : 0x01u) << (8 * r);
    }
    H[0][0][d] = H[0][1][d] = H[1][0][d] = (int)v;
    H[1][1][d] = (int)(v ^ 0xFEFEFEFEu);  // bytes 0x01 <-> 0xFF
  }
  // 64 H (Chain): bytes 0x01 -> 0x40, 0xFF -> 0xC0; the block of t = ks = 1 negated likewise
  v4i_t H64[2][2];
  if constexpr (Chain) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const uint32_t v = ((uint32_t)H[0][0][d] << 6) & 0xC0C0C0C0u;
      H64[0][0][d] = H64[0][1][d] = H64[1][0][d] = (int)v;
      H64[1][1][d] = (int)(v ^ 0x80808080u);
    }
  }
  const int wt_thread = digit_weight((uint32_t)lane);
  const int lane_off = 16 * (lane >> 5) + 32 * ((lane >> 3) & 1) + 64 * (lane & 3) + 256 * ((lane >> 4) & 1) +
                       512 * ((lane >> 2) & 1);
  const int gw = blockIdx.x * 4 + wave, GW = gridDim.x * 4;
  const int ub = (int)((int64_t)nslices * gw / GW), ue = (int)((int64_t)nslices * (gw + 1) / GW);
  // accA: the plane-sum transform's squares (its N-tile 1 as (2 U) U, see stage2); accB: the
  // planes' N-tile 0, both M-tiles; Bn: the planes' N-tile 1, U^2 + V^2 at weight index wi (entry
  // wi + 1), doubled at the flush.  6 VGPRs where the parent held 8 of a second N-tile-0 sum.
  unsigned long long accA[4] = {0, 0, 0, 0}, accB[4] = {0, 0, 0, 0}, Bn[3] = {0, 0, 0};
  int cur_w = -1;
  auto flush = [&]() {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (accA[k]) atomicAdd(&bins[cur_w + wt_thread + k], accA[k]);
      const unsigned long long n1 = k ? 2 * Bn[k - 1] : 0;  // N-tile 1: entries 1..3
      const unsigned long long b = 4 * (accB[k] + n1) - accA[k];
      if (b) atomicAdd(&bins[cur_w + wt_thread + k + 1], b);
      accA[k] = 0;
      accB[k] = 0;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) Bn[k] = 0;
  };
  // d[2 mt + ks]: M-tile mt (column bit 11), K-step ks (column bit 10)
  auto load_plane = [&](int sl, int R, v4i_t* dst) {
    const int8_t* p = buf + ((int64_t)sl * kLo + 4096 * R) + lane_off;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      dst[k] = __builtin_nontemporal_load(reinterpret_cast<const v4i_t*>(p + 1024 * k));
  };
  // stage 2 of N-tile nt from its byte splits (Bl / Bh [K-step]), two chains interleaved, then
  // their squares into acc; chain_c: the high bytes as 64 H against 4 h instead of the shift (the
  // caller's |v| <= 64 kChainMaxM).
  //   nt = 0: the chains are the two M-tiles, digit (10, 11) = 0 and 2: c[t] = H_64 rows 32 t.
  //   nt = 1: the M-tiles would be digit values 1 and 3, both non-zero: one weight, one bin.  With
  //     U = H_32 B[0], V = H_32 B[1] they are U + V and U - V, and the bin needs only
  //     (U + V)^2 + (U - V)^2 = 2 (U^2 + V^2): the last butterfly (column bit 11) is left out.
  //     c[ks] = H_32 B[ks], each a chain of two MFMAs (high, low byte of its own K-step) on the
  //     +H_32 block alone; row i and the lane weigh as before.  sum_c: acc is Bn, indexed by wi,
  //     the flush doubles it; else the factor 2 goes into the square, (2 U) U at entry wi + 1.
  auto stage2 = [&](const v4i_t* Bl, const v4i_t* Bh, auto nt_c, auto chain_c, auto sum_c,
                    unsigned long long* acc) {
    constexpr int nt = decltype(nt_c)::value;
    constexpr bool chain = decltype(chain_c)::value, half = nt == 1;
    v16i_t c[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) c[t][i] = 0;
    // nt = 1: chain t takes K-step ks = t alone
    if constexpr (chain) {
      v4i_t Bh4[2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int d = 0; d < 4; ++d) Bh4[ks][d] = (int)(((uint32_t)Bh[ks][d] << 2) & 0xFCFCFCFCu);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int t = 0; t < 2; ++t)
          if (!half || t == ks)
            c[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(half ? H64[0][0] : H64[t][ks], Bh4[ks], c[t], 0, 0, 0);
    } else {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int t = 0; t < 2; ++t)
          if (!half || t == ks)
            c[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(half ? H[0][0] : H[t][ks], Bh[ks], c[t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) c[t][i] <<= 8;
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int t = 0; t < 2; ++t)
        if (!half || t == ks)
          c[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(half ? H[0][0] : H[t][ks], Bl[ks], c[t], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      // digits (6, 7) = i & 3, (8, 9) = i >> 2, (10, 11) = nt + 2 M-tile
      constexpr int w0 = digit_weight_c((uint32_t)nt), w1 = digit_weight_c((uint32_t)(nt | 2));
      static_assert(!half || (w0 == 1 && w1 == 1), "N-tile 1: both M-tiles in one bin");
      constexpr bool sum = half && decltype(sum_c)::value, dbl = half && !sum;
      const int wi = digit_weight_c((uint32_t)(i & 3)) + digit_weight_c((uint32_t)(i >> 2));
#ifdef SCT_TILE_SQ_ABL
      // timing-only ablation (wrong results): the squares replaced by one full-rate XOR, the floor
      // of any exact F^2 accumulate (ab_tile_squares_r06)
      acc[wi + (sum ? 0 : w0)] ^= (uint32_t)c[0][i];
      acc[wi + (sum ? 0 : w1)] ^= (uint32_t)c[1][i];
#else
      acc[wi + (sum ? 0 : w0)] += (unsigned long long)((int64_t)(dbl ? 2 * c[0][i] : c[0][i]) * c[0][i]);
      acc[wi + (sum ? 0 : w1)] += (unsigned long long)((int64_t)(dbl ? 2 * c[1][i] : c[1][i]) * c[1][i]);
#endif
    }
  };
  // int16 pairs (v + 128 of stage 1, |.| < 2^15) of one M-tile -> its high / low byte operand
  auto split16 = [&](const uint32_t* pr, v4i_t& Bl, v4i_t& Bh) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      Bl[d] = (int)(__builtin_amdgcn_perm(pr[2 * d + 1], pr[2 * d], 0x06040200u) ^ 0x80808080u);
      Bh[d] = (int)__builtin_amdgcn_perm(pr[2 * d + 1], pr[2 * d], 0x07050301u);
    }
  };
  auto pairs16 = [&](const v16i_t& c1, uint32_t* pr) {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      pr[k] = __builtin_amdgcn_perm((uint32_t)c1[2 * k + 1], (uint32_t)c1[2 * k], 0x05040100u);
  };
  // planes in turn (a runtime loop: one plane's 16 VGPRs of bytes live at a time, the next
  // plane's loads in flight), the per-plane sums of all four stage-1 tiles carried across
  // (a chunk of 2^k > kMaxOrder slices: each aligned 2^16 block in its own weight order)
  auto slice_at = [&](int u) { return order ? ((u & ~(kMaxOrder - 1)) | (int)order[u & (kMaxOrder - 1)]) : u; };
  // The first plane of the next slice is loaded during this slice's last plane and tail (dn is
  // free then), so no load of a wave's run but its first is waited for right after its issue.
  v4i_t dn[4];
  int s_next = ub < ue ? slice_at(ub) : 0;
  if (ub < ue) load_plane(s_next, 0, dn);
  for (int u = ub; u < ue; ++u) {
    const int s = s_next;
    const bool more = u + 1 < ue;
    if (more) s_next = slice_at(u + 1);
    const int wz = digit_weight((uint32_t)(z0 + s));  // wave-uniform
    if (wz != cur_w) {
      if (cur_w >= 0) flush();
      cur_w = wz;
    }
    uint32_t csp[2][2][8];  // [nt][mt]: sum over the planes of v + 128 as int16 pairs, from -384
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int k = 0; k < 8; ++k) csp[nt][mt][k] = 0xFE80FE80u;
#pragma unroll 1
    for (int R = 0; R < 4; ++R) {
      v4i_t d[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) d[k] = dn[k];
      if (R < 3 || more) load_plane(R < 3 ? s : s_next, R < 3 ? R + 1 : 0, dn);
      // stage 1 of both N-tiles first, down to their int16 pairs: N-tile 1's 16 VGPRs of pairs
      // wait through N-tile 0's stage 2 instead of the 32 of the shared first K-step + 8 of bytes
      uint32_t pr[2][2][8];
      auto stage1 = [&](auto nt_c) {
        constexpr int nt = decltype(nt_c)::value;
        v16i_t c1[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int i = 0; i < 16; ++i) c1[mt][i] = 128;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int mt = 0; mt < 2; ++mt)
            c1[mt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(d[2 * mt + ks], H[nt][ks], c1[mt], 0, 0, 0);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          pairs16(c1[mt], pr[nt][mt]);
#pragma unroll
          for (int k = 0; k < 8; ++k)
            csp[nt][mt][k] = __builtin_bit_cast(uint32_t, __builtin_bit_cast(v2s_t, csp[nt][mt][k]) +
                                                              __builtin_bit_cast(v2s_t, pr[nt][mt][k]));
        }
      };
      auto ntile = [&](auto nt_c) {
        constexpr int nt = decltype(nt_c)::value;
        v4i_t Bl[2], Bh[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) split16(pr[nt][mt], Bl[mt], Bh[mt]);
        stage2(Bl, Bh, nt_c, std::bool_constant<Chain>(), std::true_type(), nt ? Bn : accB);
        __builtin_amdgcn_sched_barrier(0);
      };
      stage1(std::integral_constant<int, 1>());
      stage1(std::integral_constant<int, 0>());
      __builtin_amdgcn_sched_barrier(0);
      ntile(std::integral_constant<int, 0>());
      ntile(std::integral_constant<int, 1>());
    }
    v4i_t Bl[2], Bh[2];
    split16(csp[0][0], Bl[0], Bh[0]);
    split16(csp[0][1], Bl[1], Bh[1]);
    stage2(Bl, Bh, std::integral_constant<int, 0>(), std::false_type(), std::false_type(), accA);
    split16(csp[1][0], Bl[0], Bh[0]);
    split16(csp[1][1], Bl[1], Bh[1]);
    stage2(Bl, Bh, std::integral_constant<int, 1>(), std::false_type(), std::false_type(), accA);
  }
  if (cur_w >= 0) flush();
  __syncthreads();
  if (tid < 17) add_weight_sum64(counts, tid, bins[tid]);
  add_job_constants(counts, add_n, sumsq);
}

// sum f^2 (ensure_sumsq): SPECTRAL codes are < 2^32, so the low 32 bits are the code
__global__ void low32_kernel(const uint64_t* __restrict__ codes, int64_t n, uint32_t* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (uint32_t)codes[i];
}

// sorted codes: sum over i of 2 r_i + 1, r_i = #{j < i : key j = key i} (a code of multiplicity f
// adds 1 + 3 + ... + 2f - 1 = f^2); r_i by a lower-bound search when the left neighbour is equal
__global__ __launch_bounds__(256) void sumsq_kernel(const uint32_t* __restrict__ sorted, int64_t n,
                                                    unsigned long long* __restrict__ out) {
  unsigned long long acc = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t v = sorted[i];
    int64_t r = 0;
    if (i > 0 && sorted[i - 1] == v) {
      int64_t a = 0, b = i - 1;  // first index holding v lies in [a, b]
      while (a < b) {
        const int64_t m = (a + b) >> 1;
        if (sorted[m] < v) a = m + 1;
        else b = m;
      }
      r = i - a;
    }
    acc += 2 * (unsigned long long)r + 1;
  }
#pragma unroll
  for (int s = 32; s; s >>= 1) acc += __shfl_xor(acc, s);
  if ((threadIdx.x & 63) == 0 && acc) atomicAdd(out, acc);
}

// the plan's probe (one pass over the codes): their OR, and the code counts of every 14- and
// 16-bit column (global atomics: 737K codes over 2^14 / 2^16 counters barely contend)
__global__ __launch_bounds__(256) void probe_kernel(const uint64_t* __restrict__ codes, int64_t n,
                                                    uint32_t* __restrict__ cnt14, uint32_t* __restrict__ cnt16,
                                                    unsigned long long* __restrict__ out) {
  unsigned long long o = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t x = codes[i];
    o |= x;
    atomicAdd(&cnt14[x & (kLo - 1)], 1u);
    atomicAdd(&cnt16[x & 0xFFFFu], 1u);
  }
#pragma unroll
  for (int s = 32; s; s >>= 1) o |= __shfl_xor(o, s);
  if ((threadIdx.x & 63) == 0 && o) atomicOr(out, o);
}
// The 14-bit column counts without global atomics (sets of >= kProbeHistMin codes): workgroup g
// counts its contiguous share in LDS (as column_hist_wg_kernel) and writes H[g][.], ORing the
// codes on the way; probe_max14_kernel sums each column over the workgroups and takes the max.
// The 16-bit counts (only asked for when 14-bit columns would need int16 seeds, or forced) keep
// the atomic probe_kernel below.
constexpr int64_t kProbeHistMin = 1 << 17;
__global__ __launch_bounds__(kSortThreads) void probe_hist14_kernel(const uint64_t* __restrict__ codes, int64_t n,
                                                                    uint32_t* __restrict__ H,
                                                                    unsigned long long* __restrict__ out) {
  __shared__ uint32_t h[kLo];
  for (int c = threadIdx.x; c < kLo; c += kSortThreads) h[c] = 0;
  __syncthreads();
  int64_t b, e;
  wg_range(n, b, e);
  unsigned long long o = 0;
  for (int64_t i = b + threadIdx.x; i < e; i += kSortThreads) {
    const uint64_t x = codes[i];
    o |= x;
    atomicAdd(&h[x & (kLo - 1)], 1u);
  }
#pragma unroll
  for (int s = 32; s; s >>= 1) o |= __shfl_xor(o, s);
  if ((threadIdx.x & 63) == 0 && o) atomicOr(out, o);
  __syncthreads();
  uint32_t* row = H + (int64_t)blockIdx.x * kLo;
  for (int c = threadIdx.x; c < kLo; c += kSortThreads) row[c] = h[c];
}

__global__ __launch_bounds__(256) void probe_max14_kernel(const uint32_t* __restrict__ H, int wgs,
                                                          unsigned long long* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  uint32_t m = 0;
#pragma unroll 8
  for (int g = 0; g < wgs; ++g) m += H[(int64_t)g * kLo + c];
#pragma unroll
  for (int s = 32; s; s >>= 1) m = max(m, (uint32_t)__shfl_xor(m, s));
  if ((threadIdx.x & 63) == 0 && m) atomicMax(out + 1, (unsigned long long)m);
}

// out[1] = max cnt14, out[2] = max cnt16 (grid covers the 2^16 counters)
__global__ __launch_bounds__(256) void probe_max_kernel(const uint32_t* __restrict__ cnt14,
                                                        const uint32_t* __restrict__ cnt16,
                                                        unsigned long long* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  unsigned m14 = c < kLo ? cnt14[c] : 0u, m16 = cnt16[c];
#pragma unroll
  for (int s = 32; s; s >>= 1) {
    m14 = max(m14, (unsigned)__shfl_xor(m14, s));
    m16 = max(m16, (unsigned)__shfl_xor(m16, s));
  }
  if ((threadIdx.x & 63) == 0) {
    if (m14) atomicMax(out + 1, (unsigned long long)m14);
    if (m16) atomicMax(out + 2, (unsigned long long)m16);
  }
}

template <typename T>
int launch_seed(State& st, T* buf, int z0, int z1, hipStream_t s) {
  if constexpr (sizeof(T) == 1) {
#ifdef SCT_SEED_MX_VARIANT
    return launch_seed_mx<Cols>(seed_mx_kernel, st, buf, z0, z1, s);
#else
    return launch_seed_sm<Cols>(seed_sm_kernel, st, buf, z0, z1, s);
#endif
  } else {
    // 16 walks per workgroup for a full chunk; smaller chunks keep >= 64 workgroup rows (as
    // launch_seed_sm)
    const int walks = (z1 - (z0 & ~(kWalk - 1)) + kWalk - 1) / kWalk;
    const int per_wg = std::max(1, std::min(kSeedWalks, walks / 64));
    const dim3 sgrid(kLo / 256, (unsigned)((walks + per_wg - 1) / per_wg));
    hipLaunchKernelGGL(seed_kernel<T>, sgrid, dim3(256), 0, s, st.d_planes, st.d_gofs, st.d_off, z0, z1, buf);
    SCT_LAUNCH_CHECK();
    return SCT_OK;
  }
}

template <typename T>
int launch_tile(State& st, int z0, int z1, unsigned long long* counts, hipStream_t s, unsigned long long add_n = 0) {
  T* buf = reinterpret_cast<T*>(st.d_buf);
  if constexpr (sizeof(T) == 1) {
    // an aligned power-of-two range goes in digit-weight order (table 2^b at offset 2^b)
    const int ns = z1 - z0;
    const uint16_t* order = ((ns & (ns - 1)) == 0 && z0 % ns == 0) ? st.d_order + std::min(ns, kMaxOrder) : nullptr;
    const dim3 rgrid((unsigned)std::max(1, std::min(st.grid * st.tile_wgs, (z1 - z0 + 3) / 4)));
    hipLaunchKernelGGL(st.tile_chain ? tile_reg_kernel<true> : tile_reg_kernel<false>, rgrid, dim3(256), 0, s, buf,
                       order, z0, z1 - z0, counts, add_n, st.sumsq_ptr());
  } else {
    const dim3 grid((unsigned)std::min(st.grid * 2, z1 - z0));
    hipLaunchKernelGGL(tile_kernel<T>, grid, dim3(256), 0, s, buf, z0, z1 - z0, counts, add_n,
                       st.sumsq_ptr());
  }
  SCT_LAUNCH_CHECK();
  return SCT_OK;
}

template <typename T>
int launch_chunk(State& st, int z0, int z1, unsigned long long* counts, hipStream_t s, unsigned long long add_n) {
  return launch_seed_tile(
      st, s, [&] { return launch_seed<T>(st, reinterpret_cast<T*>(st.d_buf), z0, z1, s); },
      [&] { return launch_tile<T>(st, z0, z1, counts, s, add_n); });
}

template <typename T>
int time_chunk(State& st, int z0, int z1, unsigned long long* counts, int repeats, hipStream_t s,
               double* seed_ms, double* tile_ms) {
  return time_seed_tile(
      st, repeats, s, [&] { return launch_seed<T>(st, reinterpret_cast<T*>(st.d_buf), z0, z1, s); },
      [&] { return launch_tile<T>(st, z0, z1, counts, s); }, seed_ms, tile_ms);
}

}  // namespace

// ---------------------------------------------------------------- plan cache (workspace)
struct Workspace {
  int device = -1;
  bool busy = false;
  bool release = false;  // sct_allpairs_cache_release() while lent out: free on return
  bool order_ready = false;
  void* p[W_NSLOTS] = {};
  size_t cap[W_NSLOTS] = {};
  // a plan's private arena (SCT_ALLPAIRS_NO_CACHE): one block, the slots carved from it in turn,
  // freed whole when the plan goes -- one hipMalloc / hipFree per call instead of one per slot
  // (a hipFree costs ~110 us, profiles/dropin_hip_api_r06.csv); slots that do not fit get their own
  bool arena = false;
  uint8_t* base = nullptr;
  size_t size = 0, used = 0;
  std::vector<void*> extra;
};

namespace {
std::mutex g_ws_mu;
Workspace* g_ws[64] = {};

void ws_free(Workspace* ws) {
  if (ws->arena) {
    if (ws->base) (void)hipFree(ws->base);
    for (void* q : ws->extra) (void)hipFree(q);
  } else {
    for (int k = 0; k < W_NSLOTS; ++k)
      if (ws->p[k]) (void)hipFree(ws->p[k]);
  }
  delete ws;
}
}  // namespace

Workspace* ws_arena(size_t bytes) {
  auto* ws = new Workspace();
  ws->arena = true;
  ws->busy = true;
  if (hipGetDevice(&ws->device) != hipSuccess || hipMalloc((void**)&ws->base, bytes) != hipSuccess) {
    (void)hipGetLastError();  // (no block: every slot its own allocation, as without an arena)
    ws->base = nullptr;
    bytes = 0;
  }
  ws->size = bytes;
  return ws;
}

Workspace* ws_acquire() {
  if (sct::tune(SCT_TUNE_PLAN_CACHE, 1) == 0) return nullptr;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  std::lock_guard<std::mutex> lk(g_ws_mu);
  Workspace*& ws = g_ws[dev];
  if (!ws) {
    ws = new Workspace();
    ws->device = dev;
  }
  if (ws->busy) return nullptr;
  ws->busy = true;
  ws->release = false;
  return ws;
}

void ws_release(Workspace* ws) {
  if (!ws) return;
  if (ws->arena) {
    ws_free(ws);
    return;
  }
  std::lock_guard<std::mutex> lk(g_ws_mu);
  ws->busy = false;
  if (ws->release) {
    g_ws[ws->device] = nullptr;
    ws_free(ws);
  }
}

int ws_get(Workspace* ws, int slot, size_t bytes, void** p) {
  bytes = std::max<size_t>(bytes, 256);
  if (!ws) {
    SCT_HIP(hipMalloc(p, bytes));
    return SCT_OK;
  }
  if (ws->arena) {
    if (ws->cap[slot] < bytes) {
      const size_t at = (ws->used + 255) & ~(size_t)255;
      if (ws->base && at + bytes <= ws->size) {
        ws->p[slot] = ws->base + at;
        ws->used = at + bytes;
      } else {
        void* q = nullptr;
        SCT_HIP(hipMalloc(&q, bytes));
        ws->extra.push_back(q);
        ws->p[slot] = q;
      }
      ws->cap[slot] = bytes;
      if (slot == W_ORDER) ws->order_ready = false;
    }
    *p = ws->p[slot];
    return SCT_OK;
  }
  if (ws->cap[slot] < bytes) {  // grow (rare: a larger set than any before on this device)
    if (ws->p[slot]) (void)hipFree(ws->p[slot]);
    ws->p[slot] = nullptr;
    ws->cap[slot] = 0;
    if (slot == W_ORDER) ws->order_ready = false;
    SCT_HIP(hipMalloc(&ws->p[slot], bytes));
    ws->cap[slot] = bytes;
  }
  *p = ws->p[slot];
  return SCT_OK;
}

void ws_put(Workspace* ws, void* p) {
  if (!ws && p) (void)hipFree(p);
}

bool* ws_order_ready(Workspace* ws) { return ws ? &ws->order_ready : nullptr; }

void ws_release_all() {
  std::lock_guard<std::mutex> lk(g_ws_mu);
  for (auto& ws : g_ws) {
    if (!ws) continue;
    if (ws->busy) {
      ws->release = true;
      continue;
    }
    int cur = 0;
    const bool dev_ok = hipGetDevice(&cur) == hipSuccess && hipSetDevice(ws->device) == hipSuccess;
    ws_free(ws);
    if (dev_ok) (void)hipSetDevice(cur);
    ws = nullptr;
  }
}

void note_stream(State& st, hipStream_t s) {
  for (auto& u : st.used)
    if (u.first == s) {
      (void)hipEventRecord(u.second, s);
      return;
    }
  hipEvent_t e = nullptr;
  if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return;
  (void)hipEventRecord(e, s);
  st.used.emplace_back(s, e);
}

int make_order_table(State& st) {
  // for every power of two L <= 2^16: the offsets [0, L) sorted by digit weight, stored
  // at [L, 2L) (an aligned range of L slices adds a constant weight to all of them); the
  // same for every plan, so sorted once per process and uploaded once per workspace
  static const std::vector<uint16_t> order = [] {
    std::vector<uint16_t> o(2 * kMaxOrder);
    for (int len = 1; len <= kMaxOrder; len *= 2) {  // a stable counting sort by weight (0..8)
      int start[10] = {};
      for (int u = 0; u < len; ++u) ++start[digit_weight_c((uint32_t)u) + 1];
      for (int w = 1; w < 10; ++w) start[w] += start[w - 1];
      uint16_t* b = o.data() + len;
      for (int u = 0; u < len; ++u) b[start[digit_weight_c((uint32_t)u)]++] = (uint16_t)u;
    }
    return o;
  }();
  void* p = nullptr;
  if (int rc = ws_get(st.ws, W_ORDER, order.size() * 2, &p); rc != SCT_OK) return rc;
  st.d_order = reinterpret_cast<uint16_t*>(p);
  bool* ready = ws_order_ready(st.ws);
  if (!ready || !*ready) {
    SCT_HIP(hipMemcpy(st.d_order, order.data(), order.size() * 2, hipMemcpyHostToDevice));
    if (ready) *ready = true;
  }
  return SCT_OK;
}

int probe(Workspace* ws, const uint64_t* d_codes, int64_t n, unsigned long long* out) {
  void* p = nullptr;
  constexpr size_t kWords = (size_t)kLo + (1u << 16);
  const bool hist = n >= kProbeHistMin;  // (smaller sets: the atomic counts are as quick)
  const size_t hbytes = hist ? (size_t)kSortWGs * kLo * 4 : 0;
  if (int rc = ws_get(ws, W_PROBE, hbytes + kWords * 4 + 32, &p); rc != SCT_OK) return rc;
  struct Put {
    Workspace* ws;
    void* p;
    ~Put() { ws_put(ws, p); }
  } put{ws, p};
  uint32_t* H = reinterpret_cast<uint32_t*>(p);
  uint32_t* cnt14 = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(p) + hbytes);
  uint32_t* cnt16 = cnt14 + kLo;
  unsigned long long* res = reinterpret_cast<unsigned long long*>(cnt16 + (1u << 16));
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(1024, sct::ceil_div(n, 256)));
  if (hist) {
    // OR and the 14-bit counts first; the 16-bit ones only when the 14-bit layout cannot take
    // int8 seeds (or 16-bit columns are forced: SCT_TUNE_SPECTRAL_COLUMNS)
    SCT_HIP(hipMemsetAsync(res, 0, 32, 0));
    hipLaunchKernelGGL(probe_hist14_kernel, dim3(kSortWGs), dim3(kSortThreads), 0, 0, d_codes, n, H, res);
    SCT_LAUNCH_CHECK();
    hipLaunchKernelGGL(probe_max14_kernel, dim3(kLo / 256), dim3(256), 0, 0, H, kSortWGs, res);
    SCT_LAUNCH_CHECK();
    SCT_HIP(hipMemcpy(out, res, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (out[1] <= 127 && sct::tune(SCT_TUNE_SPECTRAL_COLUMNS, 0) != kLoBits16) return SCT_OK;  // (out[2] = 0: unused)
  }
  SCT_HIP(hipMemsetAsync(cnt14, 0, kWords * 4 + 32, 0));
  if (n > 0) {
    hipLaunchKernelGGL(probe_kernel, dim3(blocks), dim3(256), 0, 0, d_codes, n, cnt14, cnt16, res);
    SCT_LAUNCH_CHECK();
    hipLaunchKernelGGL(probe_max_kernel, dim3((1u << 16) / 256), dim3(256), 0, 0, cnt14, cnt16, res);
    SCT_LAUNCH_CHECK();
  }
  SCT_HIP(hipMemcpy(out, res, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return SCT_OK;
}

int alloc_buf(State& st, int64_t* chunk, int64_t min_chunk, size_t bytes_per_slice) {
  for (;;) {
    const size_t bytes = (size_t)((*chunk + 15) & ~15ll) * bytes_per_slice;  // whole 16-slice groups
    const int rc = ws_get(st.ws, W_BUF, bytes, &st.d_buf);
    if (rc == SCT_OK) {
      st.buf_bytes = bytes;
      return SCT_OK;
    }
    (void)hipGetLastError();  // clear the out-of-memory state
    if (rc != SCT_E_NOMEM || *chunk / 2 < min_chunk) return rc;
    *chunk /= 2;
  }
}

// resident register-tile workgroups per CU (VGPR bound: 3)
template <typename K>
static int tile_wgs_per_cu(K kernel) {
  int v = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, kernel, 256, 0) != hipSuccess || v <= 0) v = 2;
  return v;
}

int create(State& st, const uint64_t* d_codes, int64_t n, int64_t chunk, int cus, unsigned max14, unsigned max16) {
  st.n = n;
  st.chunk = std::max<int64_t>(kWalk, std::min<int64_t>(chunk, kSlices));
  st.grid = std::max(1, cus);  // CUs; the tile kernels' persistent grids are sized from it
  if (n < 2) return SCT_OK;
  // the densest column bounds |seed| and so the intermediate's width (the codes are fixed
  // for the plan's life); a set too dense for int8 seeds on 14-bit columns takes 16-bit
  // columns when every one of those holds <= 127 codes (spectral16.hip)
  const unsigned maxm = max14;
  const int64_t force = sct::tune(SCT_TUNE_SPECTRAL_COLUMNS, 0);
  if (((maxm > 127 && force != kLoBits) || force == kLoBits16) && max16 <= 127)
    return create16(st, d_codes, n, max16, chunk, cus);
  if (int rc = get_slot(st, W_HI, (size_t)n * 4, &st.d_hi); rc != SCT_OK) return rc;
  if (int rc = get_slot(st, W_OFF, (size_t)(kLo + 1) * 4, &st.d_off); rc != SCT_OK) return rc;
  if (int rc = get_slot(st, W_CNT, (size_t)2 * kLo * 4, &st.d_cnt); rc != SCT_OK) return rc;  // counts, then cursors
  st.max_m = maxm;
  st.elem_bytes = maxm <= 127 ? 1 : (maxm <= 32767 ? 2 : 4);
  // the intermediate holds one chunk: at most 4 GiB (all 2^18 slices at int8: one seed and one
  // tile launch per count; int16 / int32 seeds take 2 / 4 passes)
  st.chunk = std::min<int64_t>(st.chunk, (int64_t(4) << 30) / ((int64_t)kLo * st.elem_bytes));
  // the unbroken stage-2 chain needs 4 h in a byte: |v| <= 64 * 125 (tile_reg_kernel);
  // SCT_TUNE_TILE_CHAIN = 0 keeps the shift form for every plan
  st.tile_chain = st.elem_bytes == 1 && maxm <= kChainMaxM && sct::tune(SCT_TUNE_TILE_CHAIN, 1) != 0;
  static const int per_cu[2] = {tile_wgs_per_cu(tile_reg_kernel<false>), tile_wgs_per_cu(tile_reg_kernel<true>)};
  st.tile_wgs = per_cu[st.tile_chain];
  if (int rc = make_order_table(st); rc != SCT_OK) return rc;
  st.max_groups = sct::ceil_div(n, 32) + kLo;
  if (int rc = get_slot(st, W_GOFS, (size_t)(kLo + 1) * 4, &st.d_gofs); rc != SCT_OK) return rc;
  if (int rc = get_slot(st, W_HIST, (size_t)kSortWGs * kLo * 4, &st.d_hist); rc != SCT_OK) return rc;
  if (int rc = get_slot(st, W_PLANES, (size_t)st.max_groups * Cols::kPlaneWords * 4, &st.d_planes); rc != SCT_OK)
    return rc;
  if (int rc = alloc_buf(st, &st.chunk, std::min<int64_t>(st.chunk, 4096), (size_t)kLo * st.elem_bytes); rc != SCT_OK)
    return rc;
  if (int rc = get_slot(st, W_SUMSQ, sizeof(unsigned long long), &st.d_sumsq); rc != SCT_OK) return rc;
  return SCT_OK;
}

void wait_idle(State& st) {
  for (auto& u : st.used) {
    (void)hipEventSynchronize(u.second);
    (void)hipEventDestroy(u.second);
  }
  st.used.clear();
}

void destroy(State& st) {
  // the plan's work has to be done before its buffers serve another plan (or are freed)
  wait_idle(st);
  for (void* p : {(void*)st.d_hi, (void*)st.d_off, (void*)st.d_cnt, (void*)st.d_gofs, (void*)st.d_planes,
                  (void*)st.d_hist, st.d_buf, (void*)st.d_order, (void*)st.d_sumsq, st.d_sumsq_tmp})
    ws_put(st.ws, p);
  ws_release(st.ws);
  st = State();
}

int ensure_sumsq(State& st, const uint64_t* d_codes, hipStream_t s) {
  if (st.sumsq_ready || st.distinct) return SCT_OK;
  // scratch: low 32 bits (4n), sorted (4n), radix-sort temp
  size_t tmp = 0;
  SCT_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)st.n, 0,
                                            32, s));
  const size_t keys = ((size_t)st.n * 4 + 255) & ~(size_t)255;
  const size_t need = 2 * keys + tmp;
  char* base = reinterpret_cast<char*>(st.d_buf);
  if (need > st.buf_bytes) {  // a small test chunk: scratch of its own, kept for the plan's life
    if (int rc = ws_get(st.ws, W_SUMSQ_TMP, need, &st.d_sumsq_tmp); rc != SCT_OK) return rc;
    base = reinterpret_cast<char*>(st.d_sumsq_tmp);
  }
  uint32_t* k0 = reinterpret_cast<uint32_t*>(base);
  uint32_t* k1 = reinterpret_cast<uint32_t*>(base + keys);
  const int blocks = (int)std::min<int64_t>(2048, sct::ceil_div(st.n, 256));
  hipLaunchKernelGGL(low32_kernel, dim3(blocks), dim3(256), 0, s, d_codes, st.n, k0);
  SCT_LAUNCH_CHECK();
  SCT_HIP(hipcub::DeviceRadixSort::SortKeys(base + 2 * keys, tmp, k0, k1, (int)st.n, 0, 32, s));
  SCT_HIP(hipMemsetAsync(st.d_sumsq, 0, sizeof(unsigned long long), s));
  hipLaunchKernelGGL(sumsq_kernel, dim3(blocks), dim3(256), 0, s, k1, st.n, st.d_sumsq);
  SCT_LAUNCH_CHECK();
  st.sumsq_ready = true;
  return SCT_OK;
}

int build(State& st, const uint64_t* d_codes, hipStream_t s) {
  if (st.n < 2) return SCT_OK;
  if (int rc = ensure_sumsq(st, d_codes, s); rc != SCT_OK) return rc;
  if (st.lo_bits == kLoBits16) return build16(st, d_codes, s);
  hipEvent_t t0 = st.timer ? st.timer->start(s) : nullptr;
  hipLaunchKernelGGL(column_hist_wg_kernel, dim3(kSortWGs), dim3(kSortThreads), 0, s, d_codes, st.n, st.d_hist);
  SCT_LAUNCH_CHECK();
  hipLaunchKernelGGL(column_prefix_kernel, dim3(kLo / 256), dim3(256), 0, s, st.d_hist, kSortWGs, st.d_cnt);
  SCT_LAUNCH_CHECK();
  hipLaunchKernelGGL(column_scan16_kernel, dim3(1), dim3(1024), 0, s, st.d_cnt, st.d_off, st.d_gofs);
  SCT_LAUNCH_CHECK();
  hipLaunchKernelGGL(column_scatter_wg_kernel, dim3(kSortWGs), dim3(kSortThreads), 0, s, d_codes, st.n, st.d_hist,
                     st.d_off, st.d_hi);
  SCT_LAUNCH_CHECK();
  if (st.max_m <= 32 * kPlaneSlots) {
    hipLaunchKernelGGL(planes_slot_kernel<Cols>, dim3(kLo * kPlaneSlots / 256), dim3(256), 0, s, st.d_hi, st.d_off,
                       st.d_gofs, st.d_planes);
  } else {
    hipLaunchKernelGGL(planes_kernel, dim3((unsigned)sct::ceil_div(st.max_groups, 256)), dim3(256), 0, s,
                       st.d_hi, st.d_off, st.d_gofs, st.max_groups, st.d_planes);
  }
  SCT_LAUNCH_CHECK();
  if (st.timer) st.timer->stop(s, t0, sct::LaunchTimer::BUILD);
  return SCT_OK;
}

int count(State& st, int64_t z_begin, int64_t z_end, unsigned long long* d_counts, hipStream_t s) {
  SCT_CHECK(0 <= z_begin && z_begin <= z_end && z_end <= kSlices, "slice range [%lld, %lld)",
            (long long)z_begin, (long long)z_end);
  if (st.n < 2 || z_begin == z_end) return SCT_OK;
  if (st.lo_bits == kLoBits16) return count16(st, z_begin, z_end, d_counts, s);
  for (int64_t z0 = z_begin; z0 < z_end; z0 += st.chunk) {
    const int z1 = (int)std::min<int64_t>(z_end, z0 + st.chunk);
    // d_counts[0] += n by the job's first tile launch (the range holding slice 0)
    const unsigned long long add_n = z0 == 0 ? (unsigned long long)st.n : 0ull;
    const int rc = st.elem_bytes == 1   ? launch_chunk<int8_t>(st, (int)z0, z1, d_counts, s, add_n)
                   : st.elem_bytes == 2 ? launch_chunk<int16_t>(st, (int)z0, z1, d_counts, s, add_n)
                                        : launch_chunk<int32_t>(st, (int)z0, z1, d_counts, s, add_n);
    if (rc != SCT_OK) return rc;
  }
  return SCT_OK;
}

int seed_slices(State& st, int64_t z_begin, int64_t z_end, int8_t* d_out, hipStream_t s) {
  SCT_CHECK(0 <= z_begin && z_begin < z_end && z_end <= kSlices, "seed_slices: slice range [%lld, %lld)",
            (long long)z_begin, (long long)z_end);
  SCT_CHECK(st.n >= 2 && st.lo_bits == kLoBits && st.elem_bytes == 1, "seed_slices: not an int8 plan on 14-bit columns");
  return launch_seed<int8_t>(st, d_out, (int)z_begin, (int)z_end, s);
}

int seed_rows(State& st, int64_t z_begin, int64_t z_end, void* d_out, int64_t out_bytes, hipStream_t s) {
  SCT_CHECK(st.n >= 2, "seed_rows: a plan of fewer than 2 codes has no seed");
  const int64_t slices = st.lo_bits == kLoBits16 ? kSlices16 : kSlices;
  SCT_CHECK(0 <= z_begin && z_begin < z_end && z_end <= slices, "seed_rows: slice range [%lld, %lld) outside [0, %lld)",
            (long long)z_begin, (long long)z_end, (long long)slices);
  const int64_t row = ((int64_t)1 << st.lo_bits) * st.elem_bytes;
  SCT_CHECK(out_bytes == (z_end - z_begin) * row, "seed_rows: %lld bytes for %lld rows of %lld", (long long)out_bytes,
            (long long)(z_end - z_begin), (long long)row);
  const int z0 = (int)z_begin, z1 = (int)z_end;
  if (st.lo_bits == kLoBits16) return seed_rows16(st, z0, z1, static_cast<int8_t*>(d_out), s);
  return st.elem_bytes == 1   ? launch_seed<int8_t>(st, static_cast<int8_t*>(d_out), z0, z1, s)
         : st.elem_bytes == 2 ? launch_seed<int16_t>(st, static_cast<int16_t*>(d_out), z0, z1, s)
                              : launch_seed<int32_t>(st, static_cast<int32_t*>(d_out), z0, z1, s);
}

int time_kernels(State& st, int64_t z_begin, int64_t z_end, unsigned long long* d_counts, int repeats,
                 hipStream_t s, double* seed_ms, double* tile_ms, int64_t* slices) {
  SCT_CHECK(0 <= z_begin && z_begin < z_end && z_end <= kSlices && repeats > 0 && st.n >= 2,
            "time_kernels: empty range or plan");
  if (st.lo_bits == kLoBits16) return time_kernels16(st, z_begin, z_end, d_counts, repeats, s, seed_ms, tile_ms, slices);
  const int z1 = (int)std::min<int64_t>(z_end, z_begin + st.chunk);
  *slices = z1 - z_begin;
  return st.elem_bytes == 1   ? time_chunk<int8_t>(st, (int)z_begin, z1, d_counts, repeats, s, seed_ms, tile_ms)
         : st.elem_bytes == 2 ? time_chunk<int16_t>(st, (int)z_begin, z1, d_counts, repeats, s, seed_ms, tile_ms)
                              : time_chunk<int32_t>(st, (int)z_begin, z1, d_counts, repeats, s, seed_ms, tile_ms);
}

}  // namespace sct_spectral
