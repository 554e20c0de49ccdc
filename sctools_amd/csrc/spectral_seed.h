// SCT_ALLPAIRS_SPECTRAL: what the two column widths share (spectral.hip: 14-bit columns,
// spectral16.hip: 16-bit columns) -- the bit-plane layout and its slot build, the int8 seed
// (step-major Gray walk) and the host's seed / chunk / timing launches.  The
// column split is the one parameter: Columns<14> and Columns<16>.
#pragma once

#include <algorithm>

#include "spectral.h"

namespace sct_spectral {

// z = (slice z >> kLoBits, column z & (kLo - 1)).  Bit planes of a 32-code group: planes +
// g * kPlaneWords holds its kHiBits planes (plane k bit j = bit k of (code >> kLoBits) of the
// group's j-th code) padded with zero words to whole 16-B words, so one lane's group is
// kPlaneWords / 4 aligned loads: 18 planes in 20 words, 16 planes in 16.
template <int kBits>
struct Columns {
  static constexpr int kLoBits = kBits;
  static constexpr int kLo = 1 << kBits;              // columns per slice
  static constexpr int kHiBits = kSpaceBits - kBits;  // bit planes per group
  static constexpr int kPlaneWords = (kHiBits + 3) / 4 * 4;
};

typedef unsigned v4u_t __attribute__((ext_vector_type(4)));
constexpr int kWalk = 64;             // slices per Gray walk
constexpr int kWalkBits = 6;
constexpr int kRegGroupsSM = 3;       // int8 seed: 32-code groups whose planes stay in registers
constexpr int kMaxWalkBlockBits = 4;  // walks per Gray-ordered block: <= 16
constexpr int kSeedWalks = 16;        // walks per workgroup (4-32 within noise, round 3)
constexpr int kPlaneSlots = 4;        // planes_slot_kernel: groups per column (<= 128 codes)

// workgroup blockIdx.x's contiguous share of n items
__device__ __forceinline__ void wg_range(int64_t n, int64_t& b, int64_t& e) {
  b = n * blockIdx.x / gridDim.x;
  e = n * (blockIdx.x + 1) / gridDim.x;
}

template <class C>
__device__ __forceinline__ void load_planes(const uint32_t* __restrict__ planes, int64_t g, uint32_t* p) {
  const uint4* q = reinterpret_cast<const uint4*>(planes + g * C::kPlaneWords);
  uint32_t w[C::kPlaneWords];
#pragma unroll
  for (int i = 0; i < C::kPlaneWords / 4; ++i) {
    const uint4 v = q[i];
    w[4 * i] = v.x;
    w[4 * i + 1] = v.y;
    w[4 * i + 2] = v.z;
    w[4 * i + 3] = v.w;
  }
#pragma unroll
  for (int k = 0; k < C::kHiBits; ++k) p[k] = w[k];
}
template <class C>
__device__ __forceinline__ void store_planes(uint32_t* __restrict__ planes, int64_t g, const uint32_t* p) {
  constexpr int H = C::kHiBits;
  uint4* q = reinterpret_cast<uint4*>(planes + g * C::kPlaneWords);
#pragma unroll
  for (int i = 0; i < C::kPlaneWords / 4; ++i)
    q[i] = make_uint4(4 * i < H ? p[4 * i] : 0u, 4 * i + 1 < H ? p[4 * i + 1] : 0u,
                      4 * i + 2 < H ? p[4 * i + 2] : 0u, 4 * i + 3 < H ? p[4 * i + 3] : 0u);
}

// planes of group slot k of column c (thread (c, k); every column holds <= 32 * kPlaneSlots codes)
template <class C>
__global__ __launch_bounds__(256) void planes_slot_kernel(const uint32_t* __restrict__ hi,
                                                          const uint32_t* __restrict__ off,
                                                          const uint32_t* __restrict__ gofs,
                                                          uint32_t* __restrict__ planes) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int c = t / kPlaneSlots, k = t % kPlaneSlots;
  const uint32_t g0 = gofs[c];
  if (k >= (int)(gofs[c + 1] - g0)) return;
  const uint32_t first = off[c] + 32u * k, last = min(first + 32u, off[c + 1]);
  uint32_t p[C::kHiBits];
#pragma unroll
  for (int b = 0; b < C::kHiBits; ++b) p[b] = 0;
  for (uint32_t i = first; i < last; ++i) {
    const uint32_t h = hi[i], bit = 1u << (i - first);
#pragma unroll
    for (int b = 0; b < C::kHiBits; ++b) p[b] |= (h >> b) & 1u ? bit : 0u;
  }
  store_planes<C>(planes, (int64_t)g0 + k, p);
}

// ---------------------------------------------------------------- seed (int8)
// buf[(z - z0) kLo + c] = m(c) - 2 sum over the column's groups of popc(XOR of the planes of z's
// high bits); a workgroup = 256 columns x walks of 64 slices.  Step-major walk: per step every
// group's XOR and popcount, and the step's sum goes to the byte stage at once -- no 64-value
// accumulator array, so the first three groups' planes stay in registers at 4+ waves per SIMD.
// G = the wave's group count (<= 3; a fourth group, columns of > 96 codes, is walked afterwards
// from L2 into the lane's own stage bytes).
// the walk's start state: every group's planes XORed for the slice bits 6 and up of zblk
template <class C, int G>
__device__ __forceinline__ void walk_start(const uint32_t (*pr)[C::kHiBits], int zblk, uint32_t* x) {
#pragma unroll
  for (int g = 0; g < G; ++g) {
    uint32_t v = 0;
#pragma unroll
    for (int k = kWalkBits; k < C::kHiBits; ++k)
      if ((zblk >> k) & 1) v ^= pr[g][k];
    x[g] = v;
  }
}

// 64 Gray steps from the start state x; x is left at the last slice's state, which is the
// start state with plane 5 flipped (gray(63) = 32)
template <class C, int G>
__device__ __forceinline__ void walk_from(const uint32_t (*pr)[C::kHiBits], uint32_t* x, uint8_t* st8, int tid) {
#pragma unroll
  for (int i = 0; i < kWalk; ++i) {
    uint32_t a = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
      if (i) x[g] ^= pr[g][ctz_c(i)];
      a = g ? popc_add(x[g], a) : (uint32_t)__popc(x[g]);  // one v_bcnt per group, no v_add3
    }
    st8[gray(i) * 256 + tid] = (uint8_t)a;
    if ((i & 7) == 7) __builtin_amdgcn_sched_barrier(0);  // keep the scheduler from hoisting steps
  }
}

// after the register groups' walk of slices zblk..zblk + 63: the groups beyond them (columns of
// > 96 codes) from L2 into the lane's stage bytes, then the stage to HBM as int8 m - 2 * sum
template <class C>
__device__ __forceinline__ void seed_finish(const uint32_t* __restrict__ planes, uint32_t g0, int ng, int wng,
                                            uint8_t* st8, int tid, int co, const uint32_t* mx, int mcb, int c0,
                                            int zblk, int z0, int z1, int8_t* __restrict__ buf) {
  constexpr int NT = 256;
  for (int g = kRegGroupsSM; g < wng; ++g) {
    uint32_t p[C::kHiBits];
    if (g < ng) {
      load_planes<C>(planes, (int64_t)g0 + g, p);
    } else {
#pragma unroll
      for (int k = 0; k < C::kHiBits; ++k) p[k] = 0u;
    }
    uint32_t x = 0;
#pragma unroll
    for (int k = kWalkBits; k < C::kHiBits; ++k)
      if ((zblk >> k) & 1) x ^= p[k];
#pragma unroll
    for (int i = 0; i < kWalk; ++i) {
      if (i) x ^= p[ctz_c(i)];
      st8[gray(i) * NT + co] += (uint8_t)__popc(x);
      if ((i & 7) == 7) __builtin_amdgcn_sched_barrier(0);
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kWalk / 16; ++r) {
    const int row = tid / (NT / 16) + 16 * r, z = zblk + row;
    const uint4 v = *reinterpret_cast<const uint4*>(st8 + row * NT + mcb);
    const uint4 o = make_uint4((mx[0] - (v.x + v.x)) ^ 0x80808080u, (mx[1] - (v.y + v.y)) ^ 0x80808080u,
                               (mx[2] - (v.z + v.z)) ^ 0x80808080u, (mx[3] - (v.w + v.w)) ^ 0x80808080u);
    // non-temporal: the 4 GiB of seeds are read back once, by the tile, long after they left the caches
    if (z >= z0 && z < z1)
      __builtin_nontemporal_store(v4u_t{o.x, o.y, o.z, o.w},
                                  reinterpret_cast<v4u_t*>(buf + (int64_t)(z - z0) * C::kLo + c0 + mcb));
  }
}

// the workgroup's walks for a wave group count G: walks in blocks of 2^lp aligned on the
// absolute walk index, each block in Gray order -- consecutive walks differ in one slice
// bit (6 + t), so a walk starts from the previous one's last state with planes 5 and 6 + t
// flipped: two XORs per group instead of the start state's planes
template <class C, int G>
__device__ __forceinline__ void seed_walks(const uint32_t (*pr)[C::kHiBits], const uint32_t* __restrict__ planes,
                                           uint32_t g0, int ng, int wng, uint8_t* st8, int tid, int co,
                                           const uint32_t* mx, int mcb, int c0, int z0, int z1,
                                           int8_t* __restrict__ buf, int lp) {
  const int wa = (z0 & ~(kWalk - 1)) >> kWalkBits, we = (z1 + kWalk - 1) >> kWalkBits, P = 1 << lp;
  const int b1 = (we + P - 1) >> lp;
  for (int b = (wa >> lp) + blockIdx.y; b < b1; b += gridDim.y) {
    uint32_t x[G];
    walk_start<C, G>(pr, (b << lp) << kWalkBits, x);
    for (int j = 0; j < P; ++j) {  // workgroup-uniform
      if (j) {
        const int t = __builtin_ctz(j);
#pragma unroll
        for (int g = 0; g < G; ++g) {
          uint32_t f = pr[g][kWalkBits - 1];
#pragma unroll
          for (int k = 0; k < kMaxWalkBlockBits; ++k)
            if (k == t) f ^= pr[g][kWalkBits + k];
          x[g] ^= f;
        }
      }
      const int w = (b << lp) + (j ^ (j >> 1));
      if (w < wa || w >= we) {  // outside the range: the state as if walked
#pragma unroll
        for (int g = 0; g < G; ++g) x[g] ^= pr[g][kWalkBits - 1];
        continue;
      }
      __syncthreads();  // the previous walk's store-out reads of `stage` are done
      walk_from<C, G>(pr, x, st8, co);
      seed_finish<C>(planes, g0, ng, wng, st8, tid, co, mx, mcb, c0, w << kWalkBits, z0, z1, buf);
    }
  }
}

// the body of seed_sm_kernel / seed16_sm_kernel (grid: kLo / 256 column blocks x walk blocks)
template <class C>
__device__ __forceinline__ void seed_sm_body(const uint32_t* __restrict__ planes, const uint32_t* __restrict__ gofs,
                                             const uint32_t* __restrict__ off, int z0, int z1,
                                             int8_t* __restrict__ buf, int lp) {
  constexpr int NT = 256;
  __shared__ uint32_t stage[kWalk * NT / 4];
  uint8_t* st8 = reinterpret_cast<uint8_t*>(stage);
  const int tid = threadIdx.x;
  const int c0 = blockIdx.x * NT;
  // columns to lanes by group count (seed_lane_column): in column order nearly every wave of a
  // dense set would walk 3 groups; the stage rows and the store-out stay in column order
  const int co = seed_lane_column(gofs, c0, tid);
  const int c = c0 + co;
  const uint32_t g0 = gofs[c];
  const int ng = (int)(gofs[c + 1] - g0);
  int wng = ng;
#pragma unroll
  for (int s = 32; s; s >>= 1) wng = max(wng, __shfl_xor(wng, s));
  uint32_t pr[kRegGroupsSM][C::kHiBits];
#pragma unroll
  for (int g = 0; g < kRegGroupsSM; ++g)
    if (g < ng) {
      load_planes<C>(planes, (int64_t)g0 + g, pr[g]);
    } else {
#pragma unroll
      for (int k = 0; k < C::kHiBits; ++k) pr[g][k] = 0u;
    }
  // the 16 columns this lane stores out: their code counts as biased bytes
  const int mcb = (tid % (NT / 16)) * 16;
  uint32_t mx[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    mx[k] = 0x80808080u;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int cc = c0 + mcb + 4 * k + b;
      mx[k] |= (off[cc + 1] - off[cc]) << (8 * b);
    }
  }
  // co-resident workgroups start 0 / 1,536 / 3,072 cycles apart, so one's stores drain under
  // another's walk (What was tried (14))
  {
    const int ph = (blockIdx.x + blockIdx.y) % 3;
    if (ph >= 1) __builtin_amdgcn_s_sleep(24);
    if (ph == 2) __builtin_amdgcn_s_sleep(24);
  }
  if (wng <= 1) seed_walks<C, 1>(pr, planes, g0, ng, wng, st8, tid, co, mx, mcb, c0, z0, z1, buf, lp);
  else if (wng == 2) seed_walks<C, 2>(pr, planes, g0, ng, wng, st8, tid, co, mx, mcb, c0, z0, z1, buf, lp);
  else seed_walks<C, 3>(pr, planes, g0, ng, wng, st8, tid, co, mx, mcb, c0, z0, z1, buf, lp);
}

// ---------------------------------------------------------------- host
// slices [z0, z1) of int8 seeds by `kernel` (seed_sm_kernel / seed16_sm_kernel).  16 walks per
// workgroup for a full chunk (measured best at 65,536 slices of 14-bit columns); smaller chunks
// keep the grid at >= 4,096 workgroups (kLo / 256 column blocks x rows) so it still fills the chip.
template <class C, class Kernel>
int launch_seed_sm(Kernel kernel, State& st, int8_t* buf, int z0, int z1, hipStream_t s) {
  constexpr int kMinRows = 4096 / (C::kLo / 256);
  const int walks = (z1 - (z0 & ~(kWalk - 1)) + kWalk - 1) / kWalk;
  const int per_wg = std::max(1, std::min(kSeedWalks, walks / kMinRows));
  int lp = 0;  // walks per Gray-ordered block: the largest power of two <= per_wg, <= 16
  while (lp < kMaxWalkBlockBits && (2 << lp) <= per_wg) ++lp;
  const int wa = (z0 & ~(kWalk - 1)) / kWalk, we = (z1 + kWalk - 1) / kWalk;
  const int nb = ((we + (1 << lp) - 1) >> lp) - (wa >> lp);
  hipLaunchKernelGGL(kernel, dim3(C::kLo / 256, (unsigned)nb), dim3(256), 0, s, st.d_planes, st.d_gofs, st.d_off, z0,
                     z1, buf, lp);
  SCT_LAUNCH_CHECK();
  return SCT_OK;
}

// one chunk: `seed` then `tile` (each enqueues its kernel on s and returns an SCT_* code), each
// under the plan's LaunchTimer when it has one
template <class Seed, class Tile>
int launch_seed_tile(State& st, hipStream_t s, Seed&& seed, Tile&& tile) {
  hipEvent_t t0 = st.timer ? st.timer->start(s) : nullptr;
  int rc = seed();
  if (st.timer) st.timer->stop(s, t0, sct::LaunchTimer::SEED);
  if (rc != SCT_OK) return rc;
  t0 = st.timer ? st.timer->start(s) : nullptr;
  rc = tile();
  if (st.timer) st.timer->stop(s, t0, sct::LaunchTimer::TILE);
  return rc;
}

// Bench aid: the seed and tile launches of one chunk timed apart, each as `repeats` back-to-back
// launches bracketed by HIP events (the timestamps of events between dependent kernels of one
// stream do not split the kernels reliably), after one warm launch of each; the plan's
// LaunchTimer stays silent meanwhile.  The tile's counts receive garbage.
template <class Seed, class Tile>
int time_seed_tile(State& st, int repeats, hipStream_t s, Seed&& seed, Tile&& tile, double* seed_ms,
                  double* tile_ms) {
  hipEvent_t e[3];
  for (auto& x : e) SCT_HIP(hipEventCreate(&x));
  struct Restore {
    hipEvent_t* e;
    State& st;
    sct::LaunchTimer* timer;
    ~Restore() {
      for (int i = 0; i < 3; ++i) (void)hipEventDestroy(e[i]);
      st.timer = timer;
    }
  } guard{e, st, st.timer};
  st.timer = nullptr;
  int rc = seed();  // warm
  if (rc == SCT_OK) rc = tile();
  SCT_HIP(hipEventRecord(e[0], s));
  for (int r = 0; rc == SCT_OK && r < repeats; ++r) rc = seed();
  SCT_HIP(hipEventRecord(e[1], s));
  for (int r = 0; rc == SCT_OK && r < repeats; ++r) rc = tile();
  SCT_HIP(hipEventRecord(e[2], s));
  if (rc != SCT_OK) return rc;
  SCT_HIP(hipEventSynchronize(e[2]));
  float a = 0, b = 0;
  SCT_HIP(hipEventElapsedTime(&a, e[0], e[1]));
  SCT_HIP(hipEventElapsedTime(&b, e[1], e[2]));
  *seed_ms = a / repeats;
  *tile_ms = b / repeats;
  return SCT_OK;
}

}  // namespace sct_spectral
