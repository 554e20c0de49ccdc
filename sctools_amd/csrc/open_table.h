// The open-addressing table under the barcode counter (count.hip) and the molecule counter
// (molecules.hip): the one statement of the rule both rest on.
//
// Device.  A table is `capacity` (a power of two) uint64 key slots, EMPTY = 2^64 - 1, probed linearly
// from mix64(key).  A lane claims a slot with one 64-bit compare-and-swap of EMPTY for its key.  A key is
// written once and never changes, so a plain load that already shows the lane's own key skips the
// CAS; a stale load can only show EMPTY, and then the CAS decides.  Whatever else a counter keeps per
// slot is only ever touched by atomics of its own, so nothing is published and no lane waits for
// another lane's store.  The probe is bounded by the capacity: a full table sets the overflow word
// and never spins.  Claimed slots are summed per wave into the size word.
//
// Host.  The load stays at or below 3/4 by the feed policy of table_load.h.  A counter's calls are
// ordered across streams by one event: work on a stream starts after whatever the counter enqueued
// last on another one (enter), and every call records what it enqueued (leave).
//
// Device words: [W_SIZE] claimed slots, [W_OVERFLOW] a probe found the table full; a counter numbers
// its own words from W_OWN up to W_NWORDS.
#pragma once

#include <algorithm>

#include "mix64.h"
#include "sct_common.h"
#include "table_load.h"

namespace sct {
namespace open_table {

typedef unsigned long long u64;

constexpr int WG = 256;
constexpr u64 EMPTY = ~0ull;
constexpr u64 NO_SLOT = ~0ull;
enum { W_SIZE = 0, W_OVERFLOW = 1, W_OWN = 2, W_NWORDS = 8 };
// LDS pre-aggregation: a tile of kTile items in a table of 2 * kTile slots (load <= 1/2)
constexpr int kItems = 4;
constexpr int kTile = WG * kItems;
constexpr int kLdsSlots = 2 * kTile;

// ---- device

// The probe: true in the one call whose CAS took the slot.  SLOT: *slot is the slot that holds `key`
// when the call returns, or NO_SLOT when the table is full.  A full table sets the overflow word (the
// host fails with SCT_E_RANGE).
template <bool SLOT = false>
__device__ __forceinline__ bool claim(u64* __restrict__ keys, u64 mask, u64* __restrict__ overflow, u64 key,
                                      u64* slot = nullptr) {
  u64 s = mix64(key) & mask;
  for (u64 probe = 0; probe <= mask; ++probe) {
    u64 k = keys[s];
    bool claimed = false;
    if (k == EMPTY) {
      k = atomicCAS(&keys[s], EMPTY, key);
      claimed = k == EMPTY;
      if (claimed) k = key;
    }
    if (k == key) {
      if (SLOT) *slot = s;
      return claimed;
    }
    s = (s + 1) & mask;
  }
  atomicOr(overflow, 1ull);
  if (SLOT) *slot = NO_SLOT;
  return false;
}

// the slot that holds `key`, or NO_SLOT: the probe without the claim, read-only
__device__ __forceinline__ u64 find(const u64* __restrict__ keys, u64 mask, u64 key) {
  u64 s = mix64(key) & mask;
  for (u64 probe = 0; probe <= mask; ++probe) {
    const u64 k = keys[s];
    if (k == key) return s;
    if (k == EMPTY) return NO_SLOT;
    s = (s + 1) & mask;
  }
  return NO_SLOT;
}

// find() for a caller that issued the first load itself: `s` is the key's home slot, mix64(key) & mask,
// and `k` what keys[s] showed.  A lane that probes several tables loads every home slot first and
// resolves them afterwards, so that the loads are in flight together.
__device__ __forceinline__ u64 find_from(const u64* __restrict__ keys, u64 mask, u64 key, u64 s, u64 k) {
  for (u64 probe = 0; probe <= mask; ++probe) {
    if (k == key) return s;
    if (k == EMPTY) return NO_SLOT;
    s = (s + 1) & mask;
    k = keys[s];
  }
  return NO_SLOT;
}

// Equal keys of a wave merged: the lowest active lane holding a key is its `rep` and carries the
// `count` of its copies, the others add nothing.  Called by every lane of the wave.  The leader is
// one lane of 64, and saying so keeps the pass a branch: as selects it runs a percent slower on a
// wave of distinct keys (64 passes).
struct Merged {
  bool rep;
  u64 count;
};
__device__ __forceinline__ Merged wave_merge(bool active, u64 key) {
  const int lane = threadIdx.x & 63;
  Merged r{active, 1};
  u64 todo = __ballot(active);
  while (todo) {  // wave-uniform: one distinct key leaves per pass
    const int leader = __ffsll((long long)todo) - 1;
    const u64 lk = __shfl(key, leader);
    const u64 m = __ballot(active && key == lk);
    if (__builtin_expect(lane == leader, 0)) r.count = (u64)__popcll(m);
    else if (active && key == lk) r.rep = false;
    todo &= ~m;
  }
  return r;
}

// The claim of a slot in a workgroup's LDS table lkey[kLdsSlots] (empty = all ones), probed linearly
// from `start`: the slot that holds `key`, or -1 when none was found in kLdsSlots probes.
template <class K>
__device__ __forceinline__ int lds_claim(K* lkey, uint32_t start, K key) {
  constexpr K kEmpty = (K) ~(K)0;
  uint32_t s = start;
#pragma unroll 1
  for (int probe = 0; probe < kLdsSlots; ++probe) {
    K k = lkey[s];
    if (k == kEmpty) {
      k = atomicCAS(&lkey[s], kEmpty, key);
      if (k == kEmpty) k = key;
    }
    if (k == key) return (int)s;
    s = (s + 1) & (kLdsSlots - 1);
  }
  return -1;
}

// A compaction step, called by every lane of the wave: the output position of this lane's occupied
// slot -- one add on the cursor per wave, the lanes ranked by popcount.
__device__ __forceinline__ u64 compact_at(bool occ, u64* __restrict__ cursor) {
  const int lane = threadIdx.x & 63;
  const u64 m = __ballot(occ);
  u64 at = 0;
  if (m != 0) {
    const int leader = __ffsll((long long)m) - 1;
    if (lane == leader) at = atomicAdd(cursor, (u64)__popcll(m));
    at = __shfl(at, leader) + (u64)__popcll(m & ((1ull << lane) - 1ull));
  }
  return at;
}

// one add of the wave's claimed slots to the size word; called by every lane of the wave
__device__ __forceinline__ void add_claims(u64* __restrict__ size_word, int claims) {
  for (int o = 32; o > 0; o >>= 1) claims += __shfl_xor(claims, o);
  if ((threadIdx.x & 63) == 0 && claims > 0) atomicAdd(size_word, (u64)claims);
}

// The walks of a kernel over n items.  Each is called by every lane of every wave, and its callback
// runs the same number of times in every lane of a wave, so the callback may ballot and shuffle.

// A lane per item, grid stride: f(i, i < n) for i = the lane's number, + the grid's lanes, ...  The
// trip count is the same for every lane: the wave stays whole, and a lane past the end is told so.
template <class F>
__device__ __forceinline__ void for_each_item(int64_t n, F f) {
  const int64_t stride = (int64_t)gridDim.x * WG;
  const int64_t gid = (int64_t)blockIdx.x * WG + threadIdx.x;
  const int64_t iters = (n + stride - 1) / stride;
  for (int64_t it = 0; it < iters; ++it) {
    const int64_t i = it * stride + gid;
    f(i, i < n);
  }
}

// A wave per 64 adjacent items: f(base) for the wave's tiles [base, base + 64), base < n a multiple of
// 64 and wave-uniform; lane l's item is base + l, which lies past the end only in the last tile.
template <class F>
__device__ __forceinline__ void for_each_wave_tile(int64_t n, F f) {
  const int64_t nwaves = (int64_t)gridDim.x * (WG / 64);
  for (int64_t base = (((int64_t)blockIdx.x * WG + threadIdx.x) >> 6) * 64; base < n; base += nwaves * 64) f(base);
}

// The lanes of a ballot taken one after the other by the whole wave: f(src) for every set bit of the
// wave-uniform `mask`, lowest first.
template <class F>
__device__ __forceinline__ void wave_serial(u64 mask, F f) {
  while (mask) {
    const int src = __ffsll((long long)mask) - 1;
    mask &= mask - 1;
    f(src);
  }
}

// ---- host

inline unsigned grid_for(int64_t n, int64_t per_block, int64_t cap = 256 * 8) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cap, ceil_div(n, per_block)));
}

inline size_t up256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// Pieces of one pool block, each starting on a multiple of 256 bytes: take() gives a piece's offset,
// `size` is the block to allocate.
struct Carve {
  size_t size = 0;
  size_t take(size_t bytes) {
    const size_t at = up256(size);
    size = at + bytes;
    return at;
  }
};

// a device array of capacity * 8 bytes, every byte `fill`; `what` names it in the message
inline int alloc_filled(u64** p, int64_t capacity, int fill, hipStream_t s, const char* what) {
  hipError_t e = hipMalloc((void**)p, (size_t)capacity * 8);
  if (e == hipSuccess) e = hipMemsetAsync(*p, fill, (size_t)capacity * 8, s);
  if (e != hipSuccess) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    return fail(e == hipErrorOutOfMemory ? SCT_E_NOMEM : SCT_E_HIP, "%s of %lld slots: %s", what, (long long)capacity,
                hipGetErrorString(e));
  }
  return SCT_OK;
}

// what every counter on such a table keeps on the host
struct Host {
  const char* name;  // "<name> table of N slots is full"
  int device = 0;
  int64_t capacity = 0;
  u64* words = nullptr;    // the device words
  u64* h_words = nullptr;  // their page-locked read-back
  int64_t total = 0;       // items fed
  int64_t size_bound = 0;  // claimed slots: the last size read plus the items fed since
  hipEvent_t last = nullptr;  // the last work enqueued (another stream's call waits for it)
  hipStream_t last_stream = nullptr;
  bool used = false;
  explicit Host(const char* noun) : name(noun) {}
};

// the device words (not initialised), their read-back and the event
inline hipError_t open_words(Host* c) {
  hipError_t e = hipMalloc((void**)&c->words, W_NWORDS * 8);
  if (e == hipSuccess) e = hipHostMalloc((void**)&c->h_words, W_NWORDS * 8, hipHostMallocDefault);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->last, hipEventDisableTiming);
  return e;
}

// waits for the work the counter enqueued (it reads the counter's arrays), then frees what open_words made
inline void close_words(Host* c) {
  if (c->last) {
    if (c->used) (void)hipEventSynchronize(c->last);
    (void)hipEventDestroy(c->last);
  }
  if (c->words) (void)hipFree(c->words);
  if (c->h_words) (void)hipHostFree(c->h_words);
}

// work on `s` starts after whatever the counter enqueued last on another stream
inline int enter(Host* c, hipStream_t s) {
  if (c->used && c->last_stream != s) SCT_HIP(hipStreamWaitEvent(s, c->last, 0));
  return SCT_OK;
}

inline int leave(Host* c, hipStream_t s) {
  SCT_HIP(hipEventRecord(c->last, s));
  c->last_stream = s;
  c->used = true;
  return SCT_OK;
}

// the device words, read back after everything enqueued on `s`; the size becomes exact
inline int read_words(Host* c, hipStream_t s) {
  SCT_HIP(hipMemcpyAsync(c->h_words, c->words, W_NWORDS * 8, hipMemcpyDeviceToHost, s));
  SCT_HIP(hipStreamSynchronize(s));
  if (c->h_words[W_OVERFLOW])
    return fail(SCT_E_RANGE, "%s table of %lld slots is full", c->name, (long long)c->capacity);
  c->size_bound = (int64_t)c->h_words[W_SIZE];
  return SCT_OK;
}

// how a call that needs the table's size opens: ordered after the counter's earlier work, size exact
inline int enter_read(Host* c, hipStream_t s) {
  if (int rc = enter(c, s); rc != SCT_OK) return rc;
  return read_words(c, s);
}

// before a compaction (compact_at): the cursor word it counts the rows in
inline hipError_t zero_cursor(u64* cursor, hipStream_t s) { return hipMemsetAsync(cursor, 0, 8, s); }

// The outputs of a *_host call, staged: columns of `count` elements of `elem` bytes in one pool block,
// each on a multiple of 256 bytes.  A column whose host pointer is NULL was not asked for: it takes
// no room and its device pointer is NULL.  add() every column, alloc(), run the device form on
// dev<T>(i) (i: the order of the add() calls), then finish() copies the columns back -- `count` may be
// lowered first -- and ends the call as PoolBlock::finish does.
struct Staged {
  struct Column {
    void* host;
    size_t elem, count, at;
  };
  PoolBlock blk;
  Carve cv;
  Column cols[8];
  int n = 0;
  explicit Staged(hipStream_t s) : blk(s) {}
  void add(void* host, size_t elem, size_t count) {
    cols[n++] = Column{host, elem, count, host ? cv.take(elem * count) : 0};
  }
  int alloc() { return blk.alloc(std::max<size_t>(cv.size, 1)); }
  template <class T>
  T* dev(int i) const {
    return cols[i].host ? reinterpret_cast<T*>(blk.bytes() + cols[i].at) : nullptr;
  }
  int finish(int rc, const char* what) {
    for (int i = 0; i < n && rc == SCT_OK && blk.ok(); ++i) {
      const Column& c = cols[i];
      if (c.host && c.count)
        blk.note(hipMemcpyAsync(c.host, dev<uint8_t>(i), c.elem * c.count, hipMemcpyDeviceToHost, blk.s));
    }
    return blk.finish(rc, what);
  }
};

// n items on `s` by table_load.h's policy: grow(factor) re-makes the table at capacity * factor,
// launch(done, m) enqueues the items [done, done + m); both return a status
template <class Grow, class Launch>
int feed(Host* c, int64_t n, hipStream_t s, Grow grow, Launch launch) {
  return table_feed(n, c->capacity, c->size_bound, [&] { return read_words(c, s); }, grow, launch);
}

}  // namespace open_table
}  // namespace sct
