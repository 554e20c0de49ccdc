// Counting observed barcodes on the device (no reference kernel: the reference counts with
// collections.Counter on the host, barcode.py:100-102).
//
// sct_counter: a streaming group-by of uint64 codes with Counter's semantics -- per distinct code
// its count and the global position of its first occurrence, so the rows come back in
// first-occurrence order, which is Counter's iteration order.
//
// The table is open addressing over three parallel arrays of `capacity` (a power of two) slots:
// keys (EMPTY = 2^64 - 1), counts (0) and first (INT64_MAX).  A lane claims a slot with one 64-bit
// atomicCAS(&keys[s], EMPTY, code); whoever finds EMPTY or its own code there adds to counts[s]
// and takes the min into first[s].  Counts and first positions are only ever touched by atomics
// of their own, so nothing is published, no lane waits for another lane's store, and the probe
// loop is bounded by the capacity (a full table sets the overflow word, never spins).
// A key is written once and never changes, so a plain load that already shows the lane's own code
// skips the CAS; a stale load can only show EMPTY, and then the CAS decides.
//
// EMPTY is itself a legal code (the 32-bp all-G TwoBit barcode), so that one key is counted in a
// side slot outside the table (two words: count, first).  Key 0 needs no special case: the
// arrays are initialised by a kernel, not by zero fill.
//
// The host keeps the load factor bounded: a batch goes in as sub-batches of at most capacity / 4
// codes; the host tracks an upper bound of the claimed slots (the last size it read plus the
// codes fed since) and reads the device's size word whenever the bound passes capacity / 2; a
// true size above capacity / 2 grows the table (x4 while more than capacity / 2 codes of the
// batch remain, else x2) and a rehash kernel re-inserts every (key, count, first) row by the
// same claim rule.  The load therefore never passes 3/4.
//
// Pre-aggregation before the global atomics (SCT_TUNE_COUNT_PREAGG; DESIGN.md has the A/B):
//   0  none: one claim + add + min per code;
//   1  equal codes of a wave merged first (one lane per distinct code carries the count);
//   2  a per-workgroup LDS table of the tile's codes, flushed with one global row per distinct code.
//
// sct_index_tally: counts[idx] += 1 over the int32 indices sct_nearest_query leaves on the device
// (-1 -> tally[0], -2 -> tally[1]); each tile is pre-aggregated in an LDS table keyed by index, the
// two negative answers by wave ballots.  An index outside [-2, nw) sets an error word and is never
// stored through.
#include <hipcub/hipcub.hpp>

#include <limits.h>

#include <algorithm>
#include <vector>

#include "mix64.h"
#include "sct_common.h"

namespace {

typedef unsigned long long u64;

constexpr int WG = 256;
constexpr u64 EMPTY = ~0ull;
constexpr long long NO_FIRST = LLONG_MAX;
constexpr int64_t kMinCapacity = 64;
constexpr int64_t kMaxCapacity = 1LL << 31;  // slot numbers are uint32 in the fetch
// device words of a counter
enum { W_SIZE = 0, W_OVERFLOW = 1, W_SIDE_COUNT = 2, W_SIDE_FIRST = 3, W_CURSOR = 4, W_NWORDS = 8 };
// LDS pre-aggregation: a tile of kTile codes in a table of 2 * kTile slots (load <= 1/2)
constexpr int kItems = 4;
constexpr int kTile = WG * kItems;
constexpr int kLdsSlots = 2 * kTile;
constexpr uint32_t EMPTY32 = 0xFFFFFFFFu;

struct Table {
  u64* keys;
  u64* counts;
  long long* first;
  u64* words;
  u64 mask;  // capacity - 1
};

using sct::mix64;

// One (code, count, first) row into the table; true when this call claimed a new slot.
__device__ __forceinline__ bool table_add(const Table& t, u64 code, u64 count, long long first) {
  if (code == EMPTY) {  // the sentinel's own key: the side slot
    atomicAdd(&t.words[W_SIDE_COUNT], count);
    atomicMin(reinterpret_cast<long long*>(&t.words[W_SIDE_FIRST]), first);
    return false;
  }
  u64 s = mix64(code) & t.mask;
  for (u64 probe = 0; probe <= t.mask; ++probe) {
    u64 k = t.keys[s];
    bool claimed = false;
    if (k == EMPTY) {
      k = atomicCAS(&t.keys[s], EMPTY, code);
      claimed = k == EMPTY;
      if (claimed) k = code;
    }
    if (k == code) {
      atomicAdd(&t.counts[s], count);
      atomicMin(&t.first[s], first);
      return claimed;
    }
    s = (s + 1) & t.mask;
  }
  atomicOr(&t.words[W_OVERFLOW], 1ull);  // full table: the host fails with SCT_E_RANGE
  return false;
}

// One add of the wave's claimed slots to the size word.
__device__ __forceinline__ void bump_size(const Table& t, int claims) {
  for (int o = 32; o > 0; o >>= 1) claims += __shfl_xor(claims, o);
  if ((threadIdx.x & 63) == 0 && claims > 0) atomicAdd(&t.words[W_SIZE], (u64)claims);
}

__global__ void __launch_bounds__(WG) counter_init_kernel(Table t, int64_t capacity, int init_words) {
  for (int64_t s = (int64_t)blockIdx.x * WG + threadIdx.x; s < capacity; s += (int64_t)gridDim.x * WG) {
    t.keys[s] = EMPTY;
    t.counts[s] = 0;
    t.first[s] = NO_FIRST;
  }
  if (init_words && blockIdx.x == 0 && threadIdx.x < W_NWORDS)
    t.words[threadIdx.x] = threadIdx.x == W_SIDE_FIRST ? (u64)NO_FIRST : 0ull;
}

// MERGE = false: one row per code.  MERGE = true: equal codes of a wave are merged first -- the
// lowest lane holding a code carries the count of its copies (its position is their minimum, as
// positions rise with the lane), the others add nothing.
template <bool MERGE>
__global__ void __launch_bounds__(WG) counter_insert_kernel(Table t, const u64* __restrict__ codes, int64_t n,
                                                            long long base) {
  const int64_t stride = (int64_t)gridDim.x * WG;
  const int64_t gid = (int64_t)blockIdx.x * WG + threadIdx.x;
  const int64_t iters = (n + stride - 1) / stride;  // the same for every lane: the wave stays whole
  int claims = 0;
  for (int64_t it = 0; it < iters; ++it) {
    const int64_t i = it * stride + gid;
    const bool active = i < n;
    const u64 c = active ? __builtin_nontemporal_load(&codes[i]) : 0ull;
    u64 count = 1;
    bool rep = active;
    if (MERGE) {
      const int lane = threadIdx.x & 63;
      u64 todo = __ballot(active);
      while (todo) {  // wave-uniform: one distinct code leaves per pass
        const int leader = __ffsll((long long)todo) - 1;
        const u64 lc = __shfl(c, leader);
        const u64 m = __ballot(active && c == lc);
        if (lane == leader) count = (u64)__popcll(m);
        else if (active && c == lc) rep = false;
        todo &= ~m;
      }
    }
    if (rep) claims += table_add(t, c, count, base + i) ? 1 : 0;
  }
  bump_size(t, claims);
}

// A tile of kTile codes is grouped in an LDS table first (keys, counts, lowest offset in the tile),
// then every occupied LDS slot becomes one global row.  A code that finds no LDS slot within
// kLdsSlots probes (the table holds twice a tile's codes, so none does) goes to the global table
// directly.
__global__ void __launch_bounds__(WG) counter_insert_lds_kernel(Table t, const u64* __restrict__ codes, int64_t n,
                                                                long long base) {
  __shared__ u64 lkey[kLdsSlots];
  __shared__ uint32_t lcnt[kLdsSlots];
  __shared__ uint32_t loff[kLdsSlots];
  for (int s = threadIdx.x; s < kLdsSlots; s += WG) {
    lkey[s] = EMPTY;
    lcnt[s] = 0;
    loff[s] = EMPTY32;
  }
  __syncthreads();
  const int64_t ntiles = (n + kTile - 1) / kTile;
  int claims = 0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // block-uniform
    const int64_t t0 = tile * kTile;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      const int off = k * WG + threadIdx.x;
      const int64_t i = t0 + off;
      if (i >= n) continue;
      const u64 c = __builtin_nontemporal_load(&codes[i]);
      bool placed = false;
      if (c != EMPTY) {
        uint32_t s = (uint32_t)mix64(c) & (kLdsSlots - 1);
        for (int probe = 0; probe < kLdsSlots; ++probe) {
          u64 k0 = lkey[s];
          if (k0 == EMPTY) {
            k0 = atomicCAS(&lkey[s], EMPTY, c);
            if (k0 == EMPTY) k0 = c;
          }
          if (k0 == c) {
            atomicAdd(&lcnt[s], 1u);
            atomicMin(&loff[s], (uint32_t)off);
            placed = true;
            break;
          }
          s = (s + 1) & (kLdsSlots - 1);
        }
      }
      if (!placed) claims += table_add(t, c, 1, base + i) ? 1 : 0;
    }
    __syncthreads();
    for (int s = threadIdx.x; s < kLdsSlots; s += WG) {
      const u64 c = lkey[s];
      if (c == EMPTY) continue;
      claims += table_add(t, c, lcnt[s], base + t0 + loff[s]) ? 1 : 0;
      lkey[s] = EMPTY;
      lcnt[s] = 0;
      loff[s] = EMPTY32;
    }
    __syncthreads();
  }
  bump_size(t, claims);
}

// every row of the old table into the new one (the size word carries over unchanged)
__global__ void __launch_bounds__(WG) counter_rehash_kernel(Table from, int64_t from_capacity, Table to) {
  for (int64_t s = (int64_t)blockIdx.x * WG + threadIdx.x; s < from_capacity; s += (int64_t)gridDim.x * WG) {
    const u64 c = from.keys[s];
    if (c != EMPTY) (void)table_add(to, c, from.counts[s], from.first[s]);
  }
}

// fetch: (first, slot) of every occupied slot, in any order (the sort by first fixes the order);
// the side slot's row has slot number EMPTY32
__global__ void __launch_bounds__(WG) counter_compact_kernel(Table t, int64_t capacity, int64_t room,
                                                             long long* __restrict__ row_first,
                                                             uint32_t* __restrict__ row_slot) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * WG;
  const int64_t iters = (capacity + stride - 1) / stride;
  for (int64_t it = 0; it < iters; ++it) {
    const int64_t s = it * stride + (int64_t)blockIdx.x * WG + threadIdx.x;
    bool occ = s < capacity && t.keys[s] != EMPTY;
    if (s == 0 && t.words[W_SIDE_COUNT] != 0) {  // the thread of slot 0 also writes the side row
      const u64 at = atomicAdd(&t.words[W_CURSOR], 1ull);
      if ((int64_t)at < room) {
        row_first[at] = (long long)t.words[W_SIDE_FIRST];
        row_slot[at] = EMPTY32;
      }
    }
    const u64 m = __ballot(occ);
    if (m == 0) continue;
    u64 at = 0;
    const int leader = __ffsll((long long)m) - 1;
    if (lane == leader) at = atomicAdd(&t.words[W_CURSOR], (u64)__popcll(m));
    at = __shfl(at, leader) + (u64)__popcll(m & ((1ull << lane) - 1ull));
    if (occ && (int64_t)at < room) {
      row_first[at] = t.first[s];
      row_slot[at] = (uint32_t)s;
    }
  }
}

__global__ void __launch_bounds__(WG) counter_gather_kernel(Table t, int64_t rows,
                                                            const long long* __restrict__ row_first,
                                                            const uint32_t* __restrict__ row_slot,
                                                            u64* __restrict__ keys, u64* __restrict__ counts,
                                                            long long* __restrict__ first) {
  for (int64_t r = (int64_t)blockIdx.x * WG + threadIdx.x; r < rows; r += (int64_t)gridDim.x * WG) {
    const uint32_t s = row_slot[r];
    keys[r] = s == EMPTY32 ? EMPTY : t.keys[s];
    counts[r] = s == EMPTY32 ? t.words[W_SIDE_COUNT] : t.counts[s];
    first[r] = row_first[r];
  }
}

// counts[idx] += 1 through an LDS table of the tile's indices; words: [0] error flag
__global__ void __launch_bounds__(WG) index_tally_kernel(const int32_t* __restrict__ index, int64_t n, int64_t nw,
                                                         u64* __restrict__ counts, u64* __restrict__ tally,
                                                         u64* __restrict__ err) {
  __shared__ uint32_t lkey[kLdsSlots];
  __shared__ uint32_t lcnt[kLdsSlots];
  __shared__ uint32_t lneg[2];
  for (int s = threadIdx.x; s < kLdsSlots; s += WG) {
    lkey[s] = EMPTY32;
    lcnt[s] = 0;
  }
  if (threadIdx.x < 2) lneg[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t ntiles = (n + kTile - 1) / kTile;
  bool bad = false;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // block-uniform
    const int64_t t0 = tile * kTile;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      const int64_t i = t0 + k * WG + threadIdx.x;
      const bool active = i < n;
      const int32_t v = active ? __builtin_nontemporal_load(&index[i]) : 0;
      const bool none = active && v == -1, tie = active && v == -2;
      const bool valid = active && v >= 0 && (int64_t)v < nw;
      bad |= active && !none && !tie && !valid;
      const u64 mn = __ballot(none), mt = __ballot(tie);  // the two popular answers: one LDS add per wave
      if (lane == 0) {
        if (mn) atomicAdd(&lneg[0], (uint32_t)__popcll(mn));
        if (mt) atomicAdd(&lneg[1], (uint32_t)__popcll(mt));
      }
      if (!valid) continue;
      bool placed = false;
      uint32_t s = ((uint32_t)v * 0x9E3779B1u) >> (32 - 11);
      static_assert(kLdsSlots == 1 << 11, "the hash shift assumes 2048 LDS slots");
      for (int probe = 0; probe < kLdsSlots; ++probe) {
        uint32_t k0 = lkey[s];
        if (k0 == EMPTY32) {
          k0 = atomicCAS(&lkey[s], EMPTY32, (uint32_t)v);
          if (k0 == EMPTY32) k0 = (uint32_t)v;
        }
        if (k0 == (uint32_t)v) {
          atomicAdd(&lcnt[s], 1u);
          placed = true;
          break;
        }
        s = (s + 1) & (kLdsSlots - 1);
      }
      if (!placed) atomicAdd(&counts[v], 1ull);  // (v < nw was checked above)
    }
    __syncthreads();
    for (int s = threadIdx.x; s < kLdsSlots; s += WG) {
      const uint32_t v = lkey[s];
      if (v == EMPTY32) continue;
      atomicAdd(&counts[v], (u64)lcnt[s]);  // v came from a checked index: v < nw
      lkey[s] = EMPTY32;
      lcnt[s] = 0;
    }
    __syncthreads();
  }
  if (threadIdx.x < 2 && lneg[threadIdx.x]) atomicAdd(&tally[threadIdx.x], (u64)lneg[threadIdx.x]);
  if (__ballot(bad) && lane == 0) atomicOr(err, 1ull);
}

inline unsigned grid_for(int64_t n, int64_t per_block, int64_t cap = 256 * 8) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cap, sct::ceil_div(n, per_block)));
}

}  // namespace

struct sct_counter {
  int device = 0;
  int64_t capacity = 0;
  Table t{};
  u64* h_words = nullptr;  // page-locked read-back of the device words
  int64_t total = 0;       // codes seen
  int64_t size_bound = 0;  // claimed slots: the last size read plus the codes fed since
  int64_t grows = 0;
  hipEvent_t last = nullptr;  // the last work enqueued (another stream's call waits for it)
  hipStream_t last_stream = nullptr;
  bool used = false;
};

namespace {

void free_table(Table& t) {
  if (t.keys) (void)hipFree(t.keys);
  if (t.counts) (void)hipFree(t.counts);
  if (t.first) (void)hipFree(t.first);
  t.keys = t.counts = nullptr;
  t.first = nullptr;
}

int alloc_table(Table& t, int64_t capacity) {
  hipError_t e = hipMalloc((void**)&t.keys, (size_t)capacity * 8);
  if (e == hipSuccess) e = hipMalloc((void**)&t.counts, (size_t)capacity * 8);
  if (e == hipSuccess) e = hipMalloc((void**)&t.first, (size_t)capacity * 8);
  if (e != hipSuccess) {
    free_table(t);
    return sct::fail(e == hipErrorOutOfMemory ? SCT_E_NOMEM : SCT_E_HIP, "counter table of %lld slots: %s",
                     (long long)capacity, hipGetErrorString(e));
  }
  t.mask = (u64)capacity - 1;
  return SCT_OK;
}

// work on `s` starts after whatever the counter enqueued last on another stream
int enter(sct_counter* c, hipStream_t s) {
  if (c->used && c->last_stream != s) SCT_HIP(hipStreamWaitEvent(s, c->last, 0));
  return SCT_OK;
}

int leave(sct_counter* c, hipStream_t s) {
  SCT_HIP(hipEventRecord(c->last, s));
  c->last_stream = s;
  c->used = true;
  return SCT_OK;
}

// the device words, read back after everything enqueued on `s`
int read_words(sct_counter* c, hipStream_t s) {
  SCT_HIP(hipMemcpyAsync(c->h_words, c->t.words, W_NWORDS * 8, hipMemcpyDeviceToHost, s));
  SCT_HIP(hipStreamSynchronize(s));
  if (c->h_words[W_OVERFLOW])
    return sct::fail(SCT_E_RANGE, "counter table of %lld slots is full", (long long)c->capacity);
  c->size_bound = (int64_t)c->h_words[W_SIZE];
  return SCT_OK;
}

int grow(sct_counter* c, int64_t factor, hipStream_t s) {
  const int64_t cap = c->capacity * factor;
  if (cap > kMaxCapacity)
    return sct::fail(SCT_E_RANGE, "counter cannot grow past %lld slots", (long long)kMaxCapacity);
  Table nt = c->t;
  nt.keys = nt.counts = nullptr;
  nt.first = nullptr;
  if (int rc = alloc_table(nt, cap); rc != SCT_OK) return rc;
  hipLaunchKernelGGL(counter_init_kernel, dim3(grid_for(cap, 4096)), dim3(WG), 0, s, nt, cap, 0);
  hipLaunchKernelGGL(counter_rehash_kernel, dim3(grid_for(c->capacity, 1024)), dim3(WG), 0, s, c->t, c->capacity, nt);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(s);  // the old arrays are read until here
  if (e != hipSuccess) {
    free_table(nt);
    return sct::fail(SCT_E_HIP, "counter rehash: %s", hipGetErrorString(e));
  }
  free_table(c->t);
  c->t = nt;
  c->capacity = cap;
  c->grows += 1;
  return SCT_OK;
}

int update_device(sct_counter* c, const uint64_t* d_codes, int64_t n, hipStream_t s) {
  if (int rc = enter(c, s); rc != SCT_OK) return rc;
  const int64_t mode = sct::tune(SCT_TUNE_COUNT_PREAGG, 1);
  int64_t done = 0;
  while (done < n) {
    if (c->size_bound > c->capacity / 2) {
      if (int rc = read_words(c, s); rc != SCT_OK) return rc;
      if (c->size_bound > c->capacity / 2) {
        if (int rc = grow(c, n - done > c->capacity / 2 ? 4 : 2, s); rc != SCT_OK) return rc;
        continue;
      }
    }
    const int64_t m = std::min(n - done, c->capacity / 4);
    const u64* src = reinterpret_cast<const u64*>(d_codes) + done;
    const long long base = (long long)(c->total + done);
    if (mode == 2)
      hipLaunchKernelGGL(counter_insert_lds_kernel, dim3(grid_for(m, kTile)), dim3(WG), 0, s, c->t, src, m, base);
    else if (mode == 0)
      hipLaunchKernelGGL(counter_insert_kernel<false>, dim3(grid_for(m, 4 * WG)), dim3(WG), 0, s, c->t, src, m, base);
    else
      hipLaunchKernelGGL(counter_insert_kernel<true>, dim3(grid_for(m, 4 * WG)), dim3(WG), 0, s, c->t, src, m, base);
    SCT_LAUNCH_CHECK();
    c->size_bound += m;
    done += m;
  }
  c->total += n;
  return leave(c, s);
}

// rows in first-occurrence order into device arrays with room for `room` rows
int fetch_device(sct_counter* c, uint64_t* d_keys, uint64_t* d_counts, int64_t* d_first, int64_t room,
                 hipStream_t s) {
  if (int rc = enter(c, s); rc != SCT_OK) return rc;
  if (int rc = read_words(c, s); rc != SCT_OK) return rc;
  const int64_t rows = c->size_bound + (c->h_words[W_SIDE_COUNT] ? 1 : 0);
  SCT_CHECK(room >= rows, "room for %lld rows, the counter holds %lld", (long long)room, (long long)rows);
  if (rows == 0) return SCT_OK;
  SCT_CHECK(d_keys && d_counts && d_first, "NULL output");
  int end_bit = 1;  // first positions are below the codes seen
  while (end_bit < 64 && (c->total >> end_bit) != 0) ++end_bit;
  size_t sort_bytes = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (const u64*)nullptr, (u64*)nullptr,
                                           (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)rows, 0, end_bit, s);
  const auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t b8 = al((size_t)rows * 8), b4 = al((size_t)rows * 4);
  void* blk = nullptr;
  SCT_HIP(sct::pool_alloc(&blk, 2 * b8 + 2 * b4 + sort_bytes, s));
  uint8_t* b = static_cast<uint8_t*>(blk);
  long long* first_in = reinterpret_cast<long long*>(b);
  long long* first_out = reinterpret_cast<long long*>(b + b8);
  uint32_t* slot_in = reinterpret_cast<uint32_t*>(b + 2 * b8);
  uint32_t* slot_out = reinterpret_cast<uint32_t*>(b + 2 * b8 + b4);
  void* sort_tmp = b + 2 * b8 + 2 * b4;
  hipError_t e = hipMemsetAsync(&c->t.words[W_CURSOR], 0, 8, s);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(counter_compact_kernel, dim3(grid_for(c->capacity, 1024)), dim3(WG), 0, s, c->t, c->capacity,
                       rows, first_in, slot_in);
    // first positions are >= 0 and distinct: an unsigned sort of them is the row order
    e = hipcub::DeviceRadixSort::SortPairs(sort_tmp, sort_bytes, reinterpret_cast<const u64*>(first_in),
                                           reinterpret_cast<u64*>(first_out), slot_in, slot_out, (int)rows, 0, end_bit, s);
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(counter_gather_kernel, dim3(grid_for(rows, 1024)), dim3(WG), 0, s, c->t, rows, first_out,
                       slot_out, reinterpret_cast<u64*>(d_keys), reinterpret_cast<u64*>(d_counts),
                       reinterpret_cast<long long*>(d_first));
    e = hipGetLastError();
  }
  sct::pool_free(blk, s);
  if (e != hipSuccess) return sct::fail(SCT_E_HIP, "counter fetch: %s", hipGetErrorString(e));
  return leave(c, s);
}

}  // namespace

int sct::tally_launch(const int32_t* d_index, int64_t n, int64_t nw, uint64_t* d_counts, uint64_t* d_tally,
                      uint64_t* d_err, hipStream_t s) {
  hipLaunchKernelGGL(index_tally_kernel, dim3(grid_for(n, kTile)), dim3(WG), 0, s, d_index, n, nw,
                     reinterpret_cast<u64*>(d_counts), reinterpret_cast<u64*>(d_tally), reinterpret_cast<u64*>(d_err));
  SCT_LAUNCH_CHECK();
  return SCT_OK;
}

extern "C" int sct_counter_create(int64_t capacity_hint, sct_counter** out) {
  SCT_CHECK(out != nullptr, "counter is NULL");
  *out = nullptr;
  SCT_CHECK(capacity_hint >= 0 && capacity_hint <= kMaxCapacity, "capacity hint %lld outside [0, 2^31]",
            (long long)capacity_hint);
  int64_t cap = kMinCapacity;
  while (cap < capacity_hint) cap *= 2;
  auto* c = new sct_counter();
  const auto fail_with = [&](int rc) {
    sct_counter_destroy(c);
    return rc;
  };
  hipError_t e = hipGetDevice(&c->device);
  if (e != hipSuccess) return fail_with(sct::fail(SCT_E_HIP, "counter: %s", hipGetErrorString(e)));
  c->capacity = cap;
  if (int rc = alloc_table(c->t, cap); rc != SCT_OK) return fail_with(rc);
  e = hipMalloc((void**)&c->t.words, W_NWORDS * 8);
  if (e == hipSuccess) e = hipHostMalloc((void**)&c->h_words, W_NWORDS * 8, hipHostMallocDefault);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->last, hipEventDisableTiming);
  if (e == hipSuccess) {
    sct::HostStage* hs = sct::host_stage();
    if (!hs) return fail_with(SCT_E_HIP);
    hipLaunchKernelGGL(counter_init_kernel, dim3(grid_for(cap, 4096)), dim3(WG), 0, hs->stream, c->t, cap, 1);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(hs->stream);
  }
  if (e != hipSuccess)
    return fail_with(sct::fail(e == hipErrorOutOfMemory ? SCT_E_NOMEM : SCT_E_HIP, "counter: %s", hipGetErrorString(e)));
  *out = c;
  return SCT_OK;
}

extern "C" int sct_counter_destroy(sct_counter* c) {
  if (!c) return SCT_OK;
  if (c->last) {
    if (c->used) (void)hipEventSynchronize(c->last);  // the work it enqueued reads these arrays
    (void)hipEventDestroy(c->last);
  }
  free_table(c->t);
  if (c->t.words) (void)hipFree(c->t.words);
  if (c->h_words) (void)hipHostFree(c->h_words);
  delete c;
  return SCT_OK;
}

extern "C" int sct_counter_update(sct_counter* c, const uint64_t* d_codes, int64_t n, void* stream) {
  SCT_CHECK(n >= 0, "n must be >= 0");
  SCT_CHECK(c != nullptr, "counter is NULL");
  if (n == 0) return SCT_OK;
  SCT_CHECK(d_codes != nullptr, "NULL codes");
  return update_device(c, d_codes, n, sct::as_stream(stream));
}

extern "C" int sct_counter_update_host(sct_counter* c, const uint64_t* codes, int64_t n) {
  SCT_CHECK(n >= 0, "n must be >= 0");
  SCT_CHECK(c != nullptr, "counter is NULL");
  if (n == 0) return SCT_OK;
  SCT_CHECK(codes != nullptr, "NULL codes");
  sct::HostStage* hs = sct::host_stage();
  if (!hs) return SCT_E_HIP;
  hipStream_t s = hs->stream;
  // pieces through one pool buffer: a piece's copy is ordered after the previous piece's kernels
  const int64_t piece = std::min<int64_t>(n, 1LL << 24);
  sct::PoolBlock buf(s);
  if (int rc = buf.alloc((size_t)piece * 8); rc != SCT_OK) return rc;
  int rc = SCT_OK;
  for (int64_t b = 0; b < n && rc == SCT_OK && buf.ok(); b += piece) {
    const int64_t m = std::min(piece, n - b);
    buf.note(hipMemcpyAsync(buf.p, codes + b, (size_t)m * 8, hipMemcpyHostToDevice, s));
    if (buf.ok()) rc = update_device(c, static_cast<const uint64_t*>(buf.p), m, s);
  }
  return buf.finish(rc, "counter update");  // no caller pointer is kept past the return
}

extern "C" int sct_counter_info(sct_counter* c, int64_t* nunique, int64_t* total, int64_t* capacity) {
  SCT_CHECK(c != nullptr, "counter is NULL");
  if (nunique) {
    sct::HostStage* hs = sct::host_stage();
    if (!hs) return SCT_E_HIP;
    if (int rc = enter(c, hs->stream); rc != SCT_OK) return rc;
    if (int rc = read_words(c, hs->stream); rc != SCT_OK) return rc;
    *nunique = c->size_bound + (c->h_words[W_SIDE_COUNT] ? 1 : 0);
  }
  if (total) *total = c->total;
  if (capacity) *capacity = c->capacity;
  return SCT_OK;
}

extern "C" int sct_counter_fetch(sct_counter* c, uint64_t* d_keys, uint64_t* d_counts, int64_t* d_first, int64_t room,
                                 void* stream) {
  SCT_CHECK(room >= 0, "room must be >= 0");
  SCT_CHECK(c != nullptr, "counter is NULL");
  return fetch_device(c, d_keys, d_counts, d_first, room, sct::as_stream(stream));
}

extern "C" int sct_counter_fetch_host(sct_counter* c, uint64_t* keys, uint64_t* counts, int64_t* first, int64_t room) {
  SCT_CHECK(room >= 0, "room must be >= 0");
  SCT_CHECK(c != nullptr, "counter is NULL");
  SCT_CHECK(room == 0 || (keys && counts && first), "NULL output");
  sct::HostStage* hs = sct::host_stage();
  if (!hs) return SCT_E_HIP;
  hipStream_t s = hs->stream;
  if (int rc = enter(c, s); rc != SCT_OK) return rc;
  if (int rc = read_words(c, s); rc != SCT_OK) return rc;
  const int64_t rows = c->size_bound + (c->h_words[W_SIDE_COUNT] ? 1 : 0);
  SCT_CHECK(room >= rows, "room for %lld rows, the counter holds %lld", (long long)room, (long long)rows);
  if (rows == 0) return SCT_OK;
  const size_t b8 = ((size_t)rows * 8 + 255) & ~(size_t)255;
  sct::PoolBlock blk(s);
  if (int rc = blk.alloc(3 * b8); rc != SCT_OK) return rc;
  uint8_t* b = blk.bytes();
  const int rc = fetch_device(c, (uint64_t*)b, (uint64_t*)(b + b8), (int64_t*)(b + 2 * b8), rows, s);
  if (rc == SCT_OK) {
    blk.note(hipMemcpyAsync(keys, b, (size_t)rows * 8, hipMemcpyDeviceToHost, s));
    if (blk.ok()) blk.note(hipMemcpyAsync(counts, b + b8, (size_t)rows * 8, hipMemcpyDeviceToHost, s));
    if (blk.ok()) blk.note(hipMemcpyAsync(first, b + 2 * b8, (size_t)rows * 8, hipMemcpyDeviceToHost, s));
  }
  return blk.finish(rc, "counter fetch");
}

extern "C" int sct_index_tally(const int32_t* d_index, int64_t n, int64_t nw, uint64_t* d_counts, uint64_t* d_tally,
                               void* stream) {
  SCT_CHECK(n >= 0 && nw >= 0, "n and nw must be >= 0");
  SCT_CHECK(nw <= (int64_t)INT32_MAX, "nw beyond int32 indices");
  SCT_CHECK(d_tally != nullptr && (nw == 0 || d_counts != nullptr), "NULL counts");
  if (n == 0) return SCT_OK;
  SCT_CHECK(d_index != nullptr, "NULL index");
  hipStream_t s = sct::as_stream(stream);
  sct::PoolBlock d_err(s);
  if (int rc = d_err.alloc(8); rc != SCT_OK) return rc;
  uint64_t h_err = 0;
  d_err.note(hipMemsetAsync(d_err.p, 0, 8, s));
  int rc = SCT_OK;
  if (d_err.ok()) rc = sct::tally_launch(d_index, n, nw, d_counts, d_tally, (uint64_t*)d_err.p, s);
  if (d_err.ok() && rc == SCT_OK) d_err.note(hipMemcpyAsync(&h_err, d_err.p, 8, hipMemcpyDeviceToHost, s));
  rc = d_err.finish(rc, "index tally");  // the status below is the error word's
  if (rc == SCT_OK && h_err)
    rc = sct::fail(SCT_E_RANGE, "index outside [-2, %lld) (not counted)", (long long)nw);
  return rc;
}
