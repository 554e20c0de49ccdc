// Counting observed barcodes on the device (no reference kernel: the reference counts with
// collections.Counter on the host, barcode.py:100-102).
//
// sct_counter: a streaming group-by of uint64 codes with Counter's semantics -- per distinct code
// its count and the global position of its first occurrence, so the rows come back in
// first-occurrence order, which is Counter's iteration order.
//
// The table is open_table.h's (the claim-by-CAS probe, the bound on the load, the ordering of a
// counter's calls) over three parallel arrays of `capacity` slots: keys, counts (0) and first
// (INT64_MAX).  Whoever finds its code in a slot, claimed by itself or not, adds to counts[s] and
// takes the min into first[s].
//
// EMPTY is itself a legal code (the 32-bp all-G TwoBit barcode), so that one key is counted in a
// side slot outside the table (two words: count, first).  Key 0 needs no special case: the
// arrays are initialised by a kernel, not by zero fill.
//
// Growth re-inserts every (key, count, first) row into the new table by the same claim rule.
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
#include <limits.h>

#include <algorithm>
#include <vector>

#include "sorted_rows.h"

namespace {

using namespace sct::open_table;

constexpr long long NO_FIRST = LLONG_MAX;
// the counter's own device words
enum { W_SIDE_COUNT = W_OWN, W_SIDE_FIRST, W_CURSOR };
constexpr uint32_t EMPTY32 = 0xFFFFFFFFu;

struct Table {
  u64* keys;
  u64* counts;
  long long* first;
  u64* words;
  u64 mask;  // capacity - 1
};

// One (code, count, first) row into the table; true when this call claimed a new slot.
__device__ __forceinline__ bool table_add(const Table& t, u64 code, u64 count, long long first) {
  if (code == EMPTY) {  // the sentinel's own key: the side slot
    atomicAdd(&t.words[W_SIDE_COUNT], count);
    atomicMin(reinterpret_cast<long long*>(&t.words[W_SIDE_FIRST]), first);
    return false;
  }
  u64 slot;
  const bool claimed = claim<true>(t.keys, t.mask, &t.words[W_OVERFLOW], code, &slot);
  if (slot != NO_SLOT) {
    atomicAdd(&t.counts[slot], count);
    atomicMin(&t.first[slot], first);
  }
  return claimed;
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
  int claims = 0;
  for_each_item(n, [&](int64_t i, bool active) {
    const u64 c = active ? __builtin_nontemporal_load(&codes[i]) : 0ull;
    const Merged m = MERGE ? wave_merge(active, c) : Merged{active, 1};
    if (m.rep) claims += table_add(t, c, m.count, base + i) ? 1 : 0;
  });
  add_claims(&t.words[W_SIZE], claims);
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
      const int s = c != EMPTY ? lds_claim(lkey, (uint32_t)sct::mix64(c) & (kLdsSlots - 1), c) : -1;
      if (s >= 0) {
        atomicAdd(&lcnt[s], 1u);
        atomicMin(&loff[s], (uint32_t)off);
      } else {
        claims += table_add(t, c, 1, base + i) ? 1 : 0;
      }
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
  add_claims(&t.words[W_SIZE], claims);
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
  for_each_item(capacity, [&](int64_t s, bool in) {
    const bool occ = in && t.keys[s] != EMPTY;
    if (s == 0 && t.words[W_SIDE_COUNT] != 0) {  // the thread of slot 0 also writes the side row
      const u64 at = atomicAdd(&t.words[W_CURSOR], 1ull);
      if ((int64_t)at < room) {
        row_first[at] = (long long)t.words[W_SIDE_FIRST];
        row_slot[at] = EMPTY32;
      }
    }
    const u64 at = compact_at(occ, &t.words[W_CURSOR]);
    if (occ && (int64_t)at < room) {
      row_first[at] = t.first[s];
      row_slot[at] = (uint32_t)s;
    }
  });
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
      static_assert(kLdsSlots == 1 << 11, "the hash shift assumes 2048 LDS slots");
      const int s = lds_claim(lkey, ((uint32_t)v * 0x9E3779B1u) >> (32 - 11), (uint32_t)v);
      if (s >= 0) atomicAdd(&lcnt[s], 1u);
      else atomicAdd(&counts[v], 1ull);  // (v < nw was checked above)
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

}  // namespace

struct sct_counter : Host {
  sct_counter() : Host("counter") {}
  Table t{};  // t.words is Host::words
  int64_t grows = 0;
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

int grow(sct_counter* c, int64_t factor, hipStream_t s) {
  const int64_t cap = sct::table_grown(c->capacity, factor);
  if (cap == 0)
    return sct::fail(SCT_E_RANGE, "counter cannot grow past %lld slots", (long long)sct::kTableMaxCapacity);
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
  const auto launch = [&](int64_t done, int64_t m) -> int {
    const u64* src = reinterpret_cast<const u64*>(d_codes) + done;
    const long long base = (long long)(c->total + done);
    if (mode == 2)
      hipLaunchKernelGGL(counter_insert_lds_kernel, dim3(grid_for(m, kTile)), dim3(WG), 0, s, c->t, src, m, base);
    else if (mode == 0)
      hipLaunchKernelGGL(counter_insert_kernel<false>, dim3(grid_for(m, 4 * WG)), dim3(WG), 0, s, c->t, src, m, base);
    else
      hipLaunchKernelGGL(counter_insert_kernel<true>, dim3(grid_for(m, 4 * WG)), dim3(WG), 0, s, c->t, src, m, base);
    SCT_LAUNCH_CHECK();
    return SCT_OK;
  };
  SCT_TRY(feed(c, n, s, [&](int64_t factor) { return grow(c, factor, s); }, launch));
  c->total += n;
  return leave(c, s);
}

// rows in first-occurrence order into device arrays with room for `room` rows
int fetch_device(sct_counter* c, uint64_t* d_keys, uint64_t* d_counts, int64_t* d_first, int64_t room,
                 hipStream_t s) {
  if (int rc = enter_read(c, s); rc != SCT_OK) return rc;
  const int64_t rows = c->size_bound + (c->h_words[W_SIDE_COUNT] ? 1 : 0);
  SCT_CHECK(room >= rows, "room for %lld rows, the counter holds %lld", (long long)room, (long long)rows);
  if (rows == 0) return SCT_OK;
  SCT_CHECK(d_keys && d_counts && d_first, "NULL output");
  int end_bit = 1;  // first positions are below the codes seen
  while (end_bit < 64 && (c->total >> end_bit) != 0) ++end_bit;
  // first positions are >= 0 and distinct: an unsigned sort of them is the row order
  SortedRows<true> sr(rows, end_bit, s);
  SCT_HIP(sr.alloc());
  hipError_t e = sr.sort(&c->t.words[W_CURSOR], [&](u64* first, uint32_t* slot) {
    hipLaunchKernelGGL(counter_compact_kernel, dim3(grid_for(c->capacity, 1024)), dim3(WG), 0, s, c->t, c->capacity,
                       rows, reinterpret_cast<long long*>(first), slot);
  });
  if (e == hipSuccess) {
    hipLaunchKernelGGL(counter_gather_kernel, dim3(grid_for(rows, 1024)), dim3(WG), 0, s, c->t, rows,
                       reinterpret_cast<const long long*>(sr.word()), sr.slot(), reinterpret_cast<u64*>(d_keys),
                       reinterpret_cast<u64*>(d_counts), reinterpret_cast<long long*>(d_first));
    e = hipGetLastError();
  }
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
  SCT_CHECK(capacity_hint >= 0 && capacity_hint <= sct::kTableMaxCapacity, "capacity hint %lld outside [0, 2^31]",
            (long long)capacity_hint);
  const int64_t cap = sct::table_capacity_for(capacity_hint);
  auto* c = new sct_counter();
  const auto fail_with = [&](int rc) {
    sct_counter_destroy(c);
    return rc;
  };
  hipError_t e = hipGetDevice(&c->device);
  if (e != hipSuccess) return fail_with(sct::fail(SCT_E_HIP, "counter: %s", hipGetErrorString(e)));
  c->capacity = cap;
  if (int rc = alloc_table(c->t, cap); rc != SCT_OK) return fail_with(rc);
  e = open_words(c);
  c->t.words = c->words;
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
  close_words(c);
  free_table(c->t);
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
    if (int rc = enter_read(c, hs->stream); rc != SCT_OK) return rc;
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
  if (int rc = enter_read(c, s); rc != SCT_OK) return rc;
  const int64_t rows = c->size_bound + (c->h_words[W_SIDE_COUNT] ? 1 : 0);
  SCT_CHECK(room >= rows, "room for %lld rows, the counter holds %lld", (long long)room, (long long)rows);
  if (rows == 0) return SCT_OK;
  Staged st(s);
  st.add(keys, 8, rows), st.add(counts, 8, rows), st.add(first, 8, rows);
  if (int rc = st.alloc(); rc != SCT_OK) return rc;
  const int rc = fetch_device(c, st.dev<uint64_t>(0), st.dev<uint64_t>(1), st.dev<int64_t>(2), rows, s);
  return st.finish(rc, "counter fetch");
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
