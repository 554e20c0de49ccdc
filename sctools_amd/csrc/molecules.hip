// Counting molecules on the device: distinct (whitelist index, UMI) pairs per barcode (no reference
// kernel: the reference slices the UMI out of the read, fastq.py:181-200, and never counts with it).
//
// sct_molecules: a device *set* of molecule keys, key = (index << umi_bits) | umi (molecules_key.h),
// whose claim event drives a per-barcode tally.  The table is open_table.h's (the claim-by-CAS probe,
// the bound on the load, the ordering of a counter's calls) over the keys alone.  A key's top bit is
// always 0 (idx_bits + umi_bits <= 63), so EMPTY is never a key and there is no side slot.  The lane
// whose CAS claimed the slot, and only that lane, adds 1 to molecules[index].
//
// Per read the insert loads 12 B once (int32 index, uint64 umi).  The answers -1 / -2 and the bad
// UMIs are counted by wave ballots into registers and added to the tally once per wave; an index
// outside [-2, nw) sets the error word and is never stored through.  Good reads are pre-aggregated
// before the global atomics (SCT_TUNE_COUNT_PREAGG, the counter's knob; every form gives the same
// numbers):
//   0  none: one probe and one reads[index] add per read;
//   1  (default) equal keys of a wave merged first (one lane per distinct key carries the count);
//   2  a per-workgroup LDS table of the tile's keys: every distinct key of the tile costs one global
//      probe and one reads[index] add that carries the tile's count for that key.
// DESIGN.md §3.10 has the A/B: 1 and 2 are level when a molecule's reads are adjacent (both twice as
// fast as 0 there), and 1 is ahead of 2 when they are far apart.
//
// The rehash kernel re-inserts keys: molecules, reads and the size word are not touched by it.
//
// Everything that reads the table back goes through one stage, the table's rows sorted by key
// (sorted_rows.h): the compaction kernel writes every occupied slot's key and, where a later step
// needs cnt[slot] or the slot itself, the slot number beside it; a radix sort orders them.  One emit
// kernel turns the sorted rows into the columns a fetch form asked for (fetch_rows, under the six
// fetch entry points), and the count matrix runs over the same rows.  The merge between devices uses
// the compaction alone, with cnt[slot] written beside the key.  The *_host forms stage their outputs
// in one pool block (open_table.h, Staged) around the device forms.
//
// A *counted* counter (sct_molecules_create_counted) keeps a second array cnt[capacity] of uint64
// beside the keys: the reads of every molecule.  COUNTED is a template parameter of the insert
// kernels, so a plain counter runs the instantiations without it: the claim returns the slot, and
// the lane that carries a key's pre-aggregated count adds it to cnt[slot] as it adds it to
// reads[index].  cnt is zero wherever keys is EMPTY, so the add needs no ordering against the claim.
// The counted rehash moves each count with its key by a plain store (a key is unique in the old
// table).  On such a table the UMI collapse (include/sctools_hip.h, "collapsing UMIs one base
// apart") is one read-only pass: per molecule the 3 * L neighbour keys (umi_neighbours.h) are probed
// with the insert's hash and bounded linear probe, the best (mreads, code) among the molecule and
// its stored neighbours is its parent, and the parent's *slot* is claimed in a scratch bitmap of one
// bit per slot -- the lane whose atomicOr flips the bit adds 1 to collapsed[index], which is the
// molecules[index] idiom again and counts every distinct parent once however many children it has.
// Every shared write of the pass is an atomic and nothing it reads changes, so there is no
// inter-workgroup protocol.  fetch_counted sorts (key, slot) pairs and recomputes each row's parent
// with the same device function.  The directional clusters (include/sctools_hip.h, "directional
// clusters") are the transitive form of that pass: a label per slot in scratch,
// the same probes in a discovery pass, then one launch per sweep over the molecules whose label may
// still grow until a sweep moves nothing; the host reads two words between sweeps, and no kernel
// waits for another.  Both passes probe through one neighbour_scan and compare one Candidate (reads,
// code, slot) by one wave_max, and every kernel's loop over slots, rows or reads is one of
// open_table.h's walks: for_each_item, for_each_wave_tile, wave_serial.
//
// Merging (include/sctools_hip.h, "merging molecule counters"): the rows of another counter -- its
// table in place when both live on one device, its occupied rows compacted and copied into pool
// scratch when they do not -- go through the insert's own claim, one row per molecule with the
// molecule's reads as its count.  The target is grown first (molecules_merge_plan.h) so that every
// row may be new at a load of at most 1/2; reads[] and the tally are added by a kernel of their own.
// A counter's calls make its device current for their duration (DeviceGuard).
//
// Downsampling (include/sctools_hip.h, "downsampling reads") is the merge on one
// device with a draw per read in front of it (downsample_draw.h): a walk over the source's table in
// place that keeps m of a molecule's reads and claims the molecule with m as its count when m > 0.
// The survivors are counted first, by the one-threshold form of the curve pass, so the target grows
// to what survives; the curve itself is the same walk into a per-workgroup LDS histogram.  A molecule
// with many reads is thinned by its whole wave, as the collapse shares a molecule's neighbours.
// Merge and downsample share the growth in front of the claim kernel (make_room) and what follows
// it (absorbed); the scratch of every device form is a sct::StreamBlock, given back stream-ordered
// on every path out of its scope.
//
// Removing swapped molecules (include/sctools_hip.h, "removing swapped molecules")
// is the same walk with a judgement in place of the draw (swapped_keep.h): the lane of a stored molecule
// probes the tables of the lane's other samples in place, read-only, sums the molecule's reads there and
// keeps it when its own share reaches the fraction.  The marking pass writes a bit per slot and the
// sums; the survivors are known before the target grows, and the claim pass takes the marked slots
// through the same set_take a downsample's survivors go through.
//
// A *feature counter* (include/sctools_hip.h, "counting molecules per feature") has a third key part
// between the index and the UMI (molecules_feature_key.h).  FEATURES is a template parameter of the
// insert kernels as COUNTED is: a counter without features runs the instantiations without it, and
// the feature insert loads 16 B per read (int32 index, int32 feature, uint64 umi).  Everything that
// works on whole keys (rehash, merge, compaction, the neighbours of the collapse, which change UMI
// bits only) is the same code; the barcode of a key is key >> idx_shift in both kinds of counter.
// The count matrix is built from the sorted (key, slot) rows of fetch_counted by a run pass: a wave
// takes 64 adjacent rows, a row is a head when its (index, feature) differs from the row before it
// (lane 0 looks one row back in global memory), the heads of every wave tile are counted, a scan of
// the tile counts numbers the entries, and a second pass writes feature[e], adds 1 to its barcode's
// entry count and reduces each entry's rows inside the wave -- run length, cnt[slot], the slot's bit
// in the collapse pass's bitmap -- to one 64-bit integer atomic add per (wave, entry) and value.
// A scan of the nw + 1 entry counts is indptr.
//
// Resolving features (include/sctools_hip.h, "resolving features") decides which
// collapsed molecules survive when a (barcode, UMI) was seen under several features.  The method's own
// pass names every molecule's image; a compaction writes, per occupied slot, the key re-packed as
// (index, image UMI, feature) (molecules_resolve_key.h) with the slot beside it, and the image slot
// into a word per table slot where the method has none already; the sorted-rows stage orders the
// words, so a group's rows are adjacent and a collapsed molecule's rows adjacent inside it.  In the run
// pass the lane whose row opens a group walks the group, sums cnt[slot] per collapsed molecule, folds
// (top, how many at top, members, reads) and sets the unique winner's image slot in a bitmap of one
// bit per slot.  The matrix's fill kernel counts that bitmap per entry as it counts the collapse
// pass's, in the same block, whose rows the key sort then reuses.
//
// Read groups (include/sctools_hip.h, "read groups") keep what those passes make
// instead of throwing it away: a snapshot object with its own copy of the keys and, per slot, the
// final UMI with the kept flag and the final molecule's reads, against which batches of reads are
// tagged by a probe and one or two loads each.  Its kernels and entry points are at the end of the file.
#include <algorithm>
#include <type_traits>

#include "sorted_rows.h"  // (first: the HIP runtime's qualifiers, which the key headers below use)

#include "downsample_draw.h"
#include "molecules_feature_key.h"
#include "molecules_key.h"
#include "molecules_merge_plan.h"
#include "molecules_resolve_key.h"
#include "read_group_status.h"
#include "swapped_keep.h"
#include "umi_directional.h"
#include "umi_neighbours.h"

namespace {

using namespace sct::open_table;

// the molecule counter's own device words; W_TALLY .. W_TALLY + 3 = no match, ambiguous, bad UMI and
// (feature counters) no feature
enum { W_ERROR = W_OWN, W_CURSOR, W_TALLY };
static_assert(W_TALLY + 4 <= W_NWORDS, "the tally lives in the device words");

struct Set {
  u64* keys;
  u64* cnt;        // mreads per slot, counted counters only (else NULL and never touched)
  u64* reads;      // nw
  u64* molecules;  // nw
  u64* words;
  u64 mask;  // capacity - 1
  int64_t nw;
  int kind;
  int umi_bits;
  int64_t nf;     // features, 0 in a counter without them
  int feat_bits;  // 0 in a counter without features
  int idx_shift;  // feat_bits + umi_bits: a key's barcode is key >> idx_shift
};

// The molecule `key` of barcode `index` claimed: molecules[index] += 1 from the lane that claimed the
// key's slot (1 is returned there, 0 elsewhere).  COUNTED: the carrier of the key also adds `count` to
// the slot's mreads (cnt is zero at every empty slot, so it does not matter whether the claiming lane
// or another one adds first).
template <bool COUNTED>
__device__ __forceinline__ int set_claim(const Set& t, u64 key, uint32_t index, u64 count) {
  u64 slot = NO_SLOT;
  const bool claimed = claim<COUNTED>(t.keys, t.mask, &t.words[W_OVERFLOW], key, &slot);
  if (COUNTED && slot != NO_SLOT) atomicAdd(&t.cnt[slot], count);
  if (!claimed) return 0;
  atomicAdd(&t.molecules[index], 1ull);
  return 1;
}

// `count` reads of one molecule: reads[index] += count, and the claim.  The index comes out of a key
// built from a checked index: index < nw.  FEATURES: the barcode lies above the feature bits.
template <bool COUNTED, bool FEATURES>
__device__ __forceinline__ int set_add(const Set& t, u64 key, u64 count) {
  const uint32_t index = sct::mol_key_index(key, FEATURES ? t.idx_shift : t.umi_bits);
  atomicAdd(&t.reads[index], count);
  return set_claim<COUNTED>(t, key, index, count);
}

// What one read is: rule 1..5 of the contract (FEATURES: with 3b and 4b).  `key` is set for GOOD only.
enum { R_SKIP = 0, R_NONE, R_TIE, R_BADUMI, R_ERROR, R_GOOD, R_NOFEATURE };
template <bool FEATURES>
__device__ __forceinline__ int classify(const Set& t, int32_t v, int32_t f, u64 umi, u64* key) {
  if (v == -1) return R_NONE;
  if (v == -2) return R_TIE;
  if (v < 0 || (int64_t)v >= t.nw) return R_ERROR;
  if (FEATURES && (f < -2 || (int64_t)f >= t.nf)) return R_ERROR;
  if (sct::mol_umi_bad(umi, t.kind, t.umi_bits)) return R_BADUMI;
  if (FEATURES) {
    if (f < 0) return R_NOFEATURE;
    *key = sct::mol_fkey((uint32_t)v, (uint32_t)f, umi, t.feat_bits, t.umi_bits);
  } else {
    *key = sct::mol_key((uint32_t)v, umi, t.umi_bits);
  }
  return R_GOOD;
}

// read i of a batch as the insert kernels see it: 12 B, and 4 B more with a feature
template <bool FEATURES>
__device__ __forceinline__ int classify_at(const Set& t, const int32_t* __restrict__ index,
                                           const int32_t* __restrict__ feature, const u64* __restrict__ umi, int64_t i,
                                           u64* key) {
  const int32_t f = FEATURES ? __builtin_nontemporal_load(&feature[i]) : 0;
  return classify<FEATURES>(t, __builtin_nontemporal_load(&index[i]), f, __builtin_nontemporal_load(&umi[i]), key);
}

// The popular non-answers of a wave's reads, summed in registers (the same in every lane); the
// fourth, a read with no feature, exists in a feature counter only.
template <bool FEATURES>
struct WaveTally {
  static constexpr int kN = FEATURES ? 4 : 3;
  uint32_t n[kN] = {};
  bool error = false;
  __device__ __forceinline__ void see(int what) {
    n[0] += (uint32_t)__popcll(__ballot(what == R_NONE));
    n[1] += (uint32_t)__popcll(__ballot(what == R_TIE));
    n[2] += (uint32_t)__popcll(__ballot(what == R_BADUMI));
    if (FEATURES) n[kN - 1] += (uint32_t)__popcll(__ballot(what == R_NOFEATURE));
    error |= what == R_ERROR;
  }
  // the claimed slots into the size word, one add per wave and non-zero tally, the error word
  __device__ __forceinline__ void flush(const Set& t, int claims) {
    add_claims(&t.words[W_SIZE], claims);
    const bool any_error = __ballot(error) != 0;
    if ((threadIdx.x & 63) != 0) return;
    for (int k = 0; k < kN; ++k)
      if (n[k]) atomicAdd(&t.words[W_TALLY + k], (u64)n[k]);
    if (any_error) atomicOr(&t.words[W_ERROR], 1ull);
  }
};

// MERGE = false: one probe per read.  MERGE = true: equal keys of a wave are merged first -- the
// lowest lane holding a key carries the count of its copies, the others add nothing.
template <bool MERGE, bool COUNTED, bool FEATURES>
__global__ void __launch_bounds__(WG) molecules_insert_kernel(Set t, const int32_t* __restrict__ index,
                                                              const int32_t* __restrict__ feature,
                                                              const u64* __restrict__ umi, int64_t n) {
  WaveTally<FEATURES> wt;
  int claims = 0;
  for_each_item(n, [&](int64_t i, bool in) {
    u64 key = 0;
    int what = R_SKIP;
    if (in) what = classify_at<FEATURES>(t, index, feature, umi, i, &key);
    wt.see(what);
    const bool good = what == R_GOOD;
    const Merged m = MERGE ? wave_merge(good, key) : Merged{good, 1};
    if (m.rep) claims += set_add<COUNTED, FEATURES>(t, key, m.count);
  });
  wt.flush(t, claims);
}

// A tile of kTile reads is grouped in an LDS table first (keys, counts), then every occupied LDS slot
// becomes one global probe and one reads[index] add.  A key that finds no LDS slot within kLdsSlots
// probes (the table holds twice a tile's reads, so none does) goes to the global path directly.
template <bool COUNTED, bool FEATURES>
__global__ void __launch_bounds__(WG) molecules_insert_lds_kernel(Set t, const int32_t* __restrict__ index,
                                                                  const int32_t* __restrict__ feature,
                                                                  const u64* __restrict__ umi, int64_t n) {
  __shared__ u64 lkey[kLdsSlots];
  __shared__ uint32_t lcnt[kLdsSlots];
  for (int s = threadIdx.x; s < kLdsSlots; s += WG) {
    lkey[s] = EMPTY;
    lcnt[s] = 0;
  }
  __syncthreads();
  const int64_t ntiles = (n + kTile - 1) / kTile;
  WaveTally<FEATURES> wt;
  int claims = 0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // block-uniform
    const int64_t t0 = tile * kTile;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      const int64_t i = t0 + k * WG + threadIdx.x;
      u64 key = 0;
      int what = R_SKIP;
      if (i < n) what = classify_at<FEATURES>(t, index, feature, umi, i, &key);
      wt.see(what);
      if (what != R_GOOD) continue;
      const int s = lds_claim(lkey, (uint32_t)sct::mix64(key) & (kLdsSlots - 1), key);
      if (s >= 0) atomicAdd(&lcnt[s], 1u);
      else claims += set_add<COUNTED, FEATURES>(t, key, 1);
    }
    __syncthreads();
    for (int s = threadIdx.x; s < kLdsSlots; s += WG) {
      const u64 key = lkey[s];
      if (key == EMPTY) continue;
      claims += set_add<COUNTED, FEATURES>(t, key, (u64)lcnt[s]);
      lkey[s] = EMPTY;
      lcnt[s] = 0;
    }
    __syncthreads();
  }
  wt.flush(t, claims);
}

// every key of the old table into the new one (molecules, reads and the size word stay).  COUNTED:
// the count moves with its key.  A key is unique in the old table, so exactly one lane meets it and
// that lane's plain store is the only write to the new slot's count.
template <bool COUNTED>
__global__ void __launch_bounds__(WG) molecules_rehash_kernel(const u64* __restrict__ from,
                                                              const u64* __restrict__ from_cnt, int64_t from_capacity,
                                                              u64* __restrict__ to, u64* __restrict__ to_cnt,
                                                              u64 to_mask, u64* __restrict__ words) {
  for (int64_t s = (int64_t)blockIdx.x * WG + threadIdx.x; s < from_capacity; s += (int64_t)gridDim.x * WG) {
    const u64 key = from[s];
    if (key == EMPTY) continue;
    u64 slot = NO_SLOT;
    (void)claim<COUNTED>(to, to_mask, &words[W_OVERFLOW], key, &slot);
    if (COUNTED && slot != NO_SLOT) to_cnt[slot] = from_cnt[s];
  }
}

// ---- UMI collapse (the contract's "parent" rule; one implementation for collapse and fetch_counted)

// A stored molecule as a candidate for parent or label: ordered by (mreads, code), umi_support_less.
struct Candidate {
  u64 reads, code;
  uint32_t slot;  // (capacity <= 2^31)
};
__device__ __forceinline__ Candidate candidate_max(const Candidate& a, const Candidate& b) {
  return sct::umi_support_less(a.reads, a.code, b.reads, b.code) ? b : a;
}
// the best of the 64 lanes' candidates, in every lane
__device__ __forceinline__ Candidate wave_max(Candidate b) {
  for (int o = 32; o > 0; o >>= 1)
    b = candidate_max(b, Candidate{__shfl_xor(b.reads, o), __shfl_xor(b.code, o), __shfl_xor(b.slot, o)});
  return b;
}

// visit(neighbour, slot, mreads) for every stored one among the neighbours j0, j0 + step, ... of `key`
template <class Visit>
__device__ __forceinline__ void neighbour_scan(const Set& t, u64 key, int j0, int step, Visit visit) {
  const int n1 = 3 * (t.umi_bits / t.kind);
  for (int j = j0; j < n1; j += step) {
    const u64 nb = sct::umi_neighbour(key, t.kind, j);
    const u64 s = find(t.keys, t.mask, nb);
    if (s != NO_SLOT) visit(nb, (uint32_t)s, t.cnt[s]);
  }
}

// The parent rule over the candidates j0, j0 + step, ... of the molecule `key` held in `slot`: the
// stored key that maximises (mreads, code) over the key itself and those of its 3 * L one-base
// neighbours under the same index.  (0, 1) is the whole rule in one lane; (lane, 64) is a wave's
// share of it, to be reduced by wave_max.
__device__ __forceinline__ Candidate parent_scan(const Set& t, u64 key, uint32_t slot, int j0, int step) {
  Candidate b{t.cnt[slot], key, slot};
  neighbour_scan(t, key, j0, step,
                 [&](u64 nb, uint32_t s, u64 r) { b = candidate_max(b, Candidate{r, nb, s}); });
  return b;
}

// the claim of a parent's slot: true in the one lane that flips its bit 0 -> 1
__device__ __forceinline__ bool bitmap_claim(uint32_t* __restrict__ bitmap, uint32_t at) {
  const uint32_t bit = 1u << (at & 31);
  return (atomicOr(&bitmap[at >> 5], bit) & bit) == 0;
}

// One lane per slot (SCT_TUNE_COLLAPSE_FORM 0).  The lane of an occupied slot finds the molecule's
// parent and claims the parent's slot in the bitmap; the lane that flips the bit 0 -> 1, and only
// that lane, adds 1 to collapsed[index].  Molecules that move are summed per wave, one add per wave.
__global__ void __launch_bounds__(WG) molecules_collapse_kernel(Set t, int64_t capacity, uint32_t* __restrict__ bitmap,
                                                                u64* __restrict__ collapsed,
                                                                u64* __restrict__ ncorrected) {
  uint32_t moved = 0;
  for_each_item(capacity, [&](int64_t s, bool in) {
    const u64 key = in ? t.keys[s] : EMPTY;
    bool moves = false;
    if (key != EMPTY) {
      const Candidate parent = parent_scan(t, key, (uint32_t)s, 0, 1);
      moves = parent.code != key;
      if (bitmap_claim(bitmap, parent.slot)) atomicAdd(&collapsed[sct::mol_key_index(key, t.idx_shift)], 1ull);
    }
    moved += (uint32_t)__popcll(__ballot(moves));
  });
  if ((threadIdx.x & 63) == 0 && moved) atomicAdd(ncorrected, (u64)moved);
}

// A wave per 64 slots (SCT_TUNE_COLLAPSE_FORM 1, the default: DESIGN.md §3.10.1 has the A/B).  The
// occupied slots are taken one after the other: every lane probes its share of the molecule's
// neighbours, the wave reduces the lanes' winners by the rule's own order, and lane 0 claims.  The
// same answers as one lane per slot.
__global__ void __launch_bounds__(WG) molecules_collapse_wave_kernel(Set t, int64_t capacity,
                                                                     uint32_t* __restrict__ bitmap,
                                                                     u64* __restrict__ collapsed,
                                                                     u64* __restrict__ ncorrected) {
  const int lane = threadIdx.x & 63;
  uint32_t moved = 0;  // the same in every lane
  for_each_wave_tile(capacity, [&](int64_t base) {  // (capacity is a multiple of 64: base + lane < capacity)
    const u64 mine = t.keys[base + lane];
    wave_serial(__ballot(mine != EMPTY), [&](int src) {
      const u64 key = __shfl(mine, src);
      const Candidate b = wave_max(parent_scan(t, key, (uint32_t)(base + src), lane, 64));
      if (lane == 0 && bitmap_claim(bitmap, b.slot))
        atomicAdd(&collapsed[sct::mol_key_index(key, t.idx_shift)], 1ull);
      moved += b.code != key;
    });
  });
  if (lane == 0 && moved) atomicAdd(ncorrected, (u64)moved);
}

// ---- directional clusters (include/sctools_hip.h, "directional clusters"): the low 31 bits of
// lab[slot] are the slot of the best ancestor of the slot's molecule known so far (capacity <= 2^31),
// meaningful where keys is occupied.  A label names a stored molecule, so it is compared by
// (cnt[label], keys[label]).  The top bit says that the label may still grow: the molecule has an
// in-neighbour whose own word has the bit.  A word without it is final.  Two molecules of a cluster
// share index and feature bits, so the labels' order (umi_label_less) is the candidates'.

constexpr uint32_t kLabelOpen = 1u << 31, kLabelSlot = kLabelOpen - 1;

__device__ __forceinline__ Candidate label_at(const Set& t, uint32_t slot) {
  return Candidate{t.cnt[slot], t.keys[slot], slot};
}
// a word is read and written while other waves do the same: whole words, in any order
__device__ __forceinline__ uint32_t label_load(const uint32_t* lab, u64 slot) {
  return __atomic_load_n(&lab[slot], __ATOMIC_RELAXED);
}

// A wave per 64 items, the shape of molecules_collapse_wave_kernel: an item is a table slot (n = the
// capacity, a multiple of 64) or, LISTED, an entry of list[n].  The occupied items are taken one
// after the other; lane j probes neighbour j (and j + 64) of the molecule v, applies the edge test
// neighbour -> v to what it finds, and the wave reduces the lanes' candidates by the labels' order.
//   DISCOVER: the candidates are the in-neighbours themselves, lab[v] becomes the best of them and v,
//     open when v has any in-edge.  A v without an in-edge is a root and final.
//   otherwise, a sweep: the candidates are lab[v], lab[lab[v]] and lab[a] of every in-neighbour a --
//     ancestors of v all -- and a label that moves sets *changed.  v stays open while an in-neighbour's
//     word is open; when none is, this sweep read their final labels and lab[v] is final too (label
//     and bit are one word).  Only v's own wave writes lab[v] and a label only ever grows, so
//     updating in place reaches the fixpoint of the plain iteration; a sweep that changes nothing
//     read final labels only.
// The open molecules are appended to worklist[room] (if not NULL), one add on the cursor per wave and
// 64 items: the next sweep's list.  Molecules that only feed each other (1-read sets) stay open until
// no label moves.
template <bool DISCOVER, bool LISTED>
__global__ void __launch_bounds__(WG) molecules_directional_kernel(Set t, int64_t n, const uint32_t* __restrict__ list,
                                                                   uint32_t* lab, uint32_t* __restrict__ worklist,
                                                                   int64_t room, u64* __restrict__ cursor,
                                                                   u64* __restrict__ changed) {
  const int lane = threadIdx.x & 63;
  bool moved = false;  // the same in every lane
  for_each_wave_tile(n, [&](int64_t base) {
    const int64_t i = base + lane;
    uint32_t slot = 0;
    u64 mine = EMPTY;
    if (i < n) {
      slot = LISTED ? list[i] : (uint32_t)i;
      mine = t.keys[slot];
    }
    u64 still_open = 0;
    wave_serial(__ballot(mine != EMPTY), [&](int src) {
      const u64 key = __shfl(mine, src);
      const uint32_t v = __shfl(slot, src);
      const u64 v_reads = t.cnt[v];
      const uint32_t word = DISCOVER ? v : label_load(lab, v);
      const uint32_t was = word & kLabelSlot;
      // (lab[x] is never below x)
      Candidate b = DISCOVER ? Candidate{v_reads, key, v} : label_at(t, label_load(lab, was) & kLabelSlot);
      bool open = false;
      neighbour_scan(t, key, lane, 64, [&](u64 nb, uint32_t s, u64 r) {
        if (!sct::umi_directional_edge(r, v_reads)) return;
        const uint32_t theirs = DISCOVER ? kLabelOpen : label_load(lab, s);
        open |= (theirs & kLabelOpen) != 0;
        b = candidate_max(b, DISCOVER ? Candidate{r, nb, s} : label_at(t, theirs & kLabelSlot));
      });
      b = wave_max(b);
      const bool any_open = __ballot(open) != 0;
      const uint32_t now = b.slot | (any_open ? kLabelOpen : 0);
      if (lane == 0 && (DISCOVER || now != word)) __atomic_store_n(&lab[v], now, __ATOMIC_RELAXED);
      still_open |= any_open ? 1ull << src : 0;
      moved |= b.slot != was;
    });
    if (worklist) {
      const bool listed = (still_open >> lane) & 1;
      const u64 at = compact_at(listed, cursor);
      if (listed && (int64_t)at < room) worklist[at] = slot;
    }
  });
  if (!DISCOVER && lane == 0 && moved) atomicOr(changed, 1ull);
}

// collapsed[index] += the molecules of the barcode that are their own label, one add per (wave,
// index); the others are summed per wave into *ncorrected.
__global__ void __launch_bounds__(WG) molecules_directional_count_kernel(Set t, int64_t capacity,
                                                                         const uint32_t* __restrict__ lab,
                                                                         u64* __restrict__ collapsed,
                                                                         u64* __restrict__ ncorrected) {
  uint32_t moved = 0;
  for_each_item(capacity, [&](int64_t s, bool in) {
    const u64 key = in ? t.keys[s] : EMPTY;
    const bool occ = key != EMPTY;
    const bool root = occ && (lab[s] & kLabelSlot) == (uint32_t)s;
    const u64 index = occ ? sct::mol_key_index(key, t.idx_shift) : 0;
    const Merged m = wave_merge(root, index);
    if (m.rep) atomicAdd(&collapsed[index], m.count);
    moved += (uint32_t)__popcll(__ballot(occ && !root));
  });
  if ((threadIdx.x & 63) == 0 && moved) atomicAdd(ncorrected, (u64)moved);
}

// fetch and merge: the occupied slots' keys in any order (the sort fixes the order) and, beside each,
// nothing, its slot number (uint32: capacity <= 2^31) or its mreads (u64); at most `room` are written
enum { BESIDE_NONE, BESIDE_SLOT, BESIDE_COUNT };
template <int BESIDE>
__global__ void __launch_bounds__(WG) molecules_compact_kernel(const u64* __restrict__ keys,
                                                               const u64* __restrict__ cnt, int64_t capacity,
                                                               u64* __restrict__ cursor, int64_t room,
                                                               u64* __restrict__ out_key, void* __restrict__ beside) {
  for_each_item(capacity, [&](int64_t s, bool in) {
    const u64 key = in ? keys[s] : EMPTY;
    const bool occ = key != EMPTY;
    const u64 at = compact_at(occ, cursor);
    if (occ && (int64_t)at < room) {
      out_key[at] = key;
      if (BESIDE == BESIDE_SLOT) static_cast<uint32_t*>(beside)[at] = (uint32_t)s;
      if (BESIDE == BESIDE_COUNT) static_cast<u64*>(beside)[at] = cnt[s];
    }
  });
}

// the sorted keys as rows: index, UMI and, if asked, the feature.  SLOTS: `slots` (the keys' slot
// numbers, sorted with them; else NULL, as mreads and parent are) also gives, each if asked, mreads
// and the parent's UMI: the one-step parent, or with `lab` (the directional labels) the root.
template <bool SLOTS>
__global__ void __launch_bounds__(WG) molecules_emit_kernel(Set t, const u64* __restrict__ keys,
                                                            const uint32_t* __restrict__ slots, int64_t rows,
                                                            int32_t* __restrict__ index, int32_t* __restrict__ feature,
                                                            u64* __restrict__ umi, u64* __restrict__ mreads,
                                                            u64* __restrict__ parent, const uint32_t* __restrict__ lab) {
  for (int64_t r = (int64_t)blockIdx.x * WG + threadIdx.x; r < rows; r += (int64_t)gridDim.x * WG) {
    const u64 key = keys[r];
    const uint32_t slot = SLOTS ? slots[r] : 0;  // (loaded with the key, ahead of the stores)
    index[r] = (int32_t)sct::mol_key_index(key, t.idx_shift);
    if (feature) feature[r] = (int32_t)sct::mol_fkey_feature(key, t.feat_bits, t.umi_bits);
    umi[r] = sct::mol_key_umi(key, t.umi_bits);
    if (!SLOTS) continue;
    if (mreads) mreads[r] = t.cnt[slot];
    if (parent)
      parent[r] = sct::mol_key_umi(lab ? t.keys[lab[slot] & kLabelSlot] : parent_scan(t, key, slot, 0, 1).code, t.umi_bits);
  }
}

// ---- the count matrix (include/sctools_hip.h, "counting molecules per feature"): the run pass over
// the rows sorted by key.  A wave tile is 64 adjacent rows, one per lane.

// whether this lane's row opens an entry: its (index, feature) differs from the previous row's.  The
// previous row is the lane below; lane 0 reads it from global memory.  Called by every lane.
__device__ __forceinline__ bool row_is_head(const u64* __restrict__ keys, int64_t r, bool in, u64 key, int umi_bits) {
  u64 prev = __shfl_up(key, 1);
  if ((threadIdx.x & 63) == 0 && in && r > 0) prev = keys[r - 1];
  return in && (r == 0 || sct::mol_fkey_head(key, prev, umi_bits));
}

// heads[tile] = the entries that open in the tile's 64 rows
__global__ void __launch_bounds__(WG) molecules_matrix_heads_kernel(const u64* __restrict__ keys, int64_t rows,
                                                                    int umi_bits, u64* __restrict__ heads) {
  const int lane = threadIdx.x & 63;
  for_each_wave_tile(rows, [&](int64_t base) {
    const int64_t r = base + lane;
    const bool in = r < rows;
    const u64 key = in ? keys[r] : 0;
    const u64 m = __ballot(row_is_head(keys, r, in, key, umi_bits));
    if (lane == 0) heads[base >> 6] = (u64)__popcll(m);
  });
}

// base[tile] = the entries that open before the tile (the scan of heads[]).  Row r belongs to entry
// e = base + (heads of the tile at or below its lane) - 1; a tile whose lane 0 is no head continues
// entry base - 1.  A head writes feature[e] and adds 1 to its barcode's entry count.  The rows of an
// entry are adjacent lanes: the lowest of them in this wave (a head, or lane 0) adds the wave's share
// of each value to the entry, one integer atomic add per (wave, entry) and value -- the run length,
// the sum of cnt[slot], and the slots whose bit the collapse pass set (the entry's distinct parents:
// a parent lies in its child's entry) or, with `lab` in place of the bitmap, the slots that are their
// own directional label (the entry's roots).  Each value array is nullable.
__global__ void __launch_bounds__(WG) molecules_matrix_fill_kernel(Set t, const u64* __restrict__ keys,
                                                                   const uint32_t* __restrict__ slots, int64_t rows,
                                                                   const u64* __restrict__ base,
                                                                   const uint32_t* __restrict__ bitmap,
                                                                   const uint32_t* __restrict__ lab,
                                                                   u64* __restrict__ row_entries,
                                                                   int32_t* __restrict__ feature,
                                                                   u64* __restrict__ molecules, u64* __restrict__ reads,
                                                                   u64* __restrict__ collapsed) {
  const int lane = threadIdx.x & 63;
  const u64 at_or_below = ~0ull >> (63 - lane), below = at_or_below >> 1;
  for_each_wave_tile(rows, [&](int64_t row0) {
    const int64_t r = row0 + lane;
    const bool in = r < rows;
    const u64 key = in ? keys[r] : 0;
    const bool head = row_is_head(keys, r, in, key, t.umi_bits);
    const u64 heads = __ballot(head), valid = __ballot(in);
    const u64 e = base[row0 >> 6] + (u64)__popcll(heads & at_or_below) - 1;  // lane 0 of tile 0 is a head: e >= 0
    if (head) {
      feature[e] = (int32_t)sct::mol_fkey_feature(key, t.feat_bits, t.umi_bits);
      atomicAdd(&row_entries[sct::mol_key_index(key, t.idx_shift)], 1ull);
    }
    // this lane's run: from itself up to the next head, within the tile's rows
    const bool first = in && (head || lane == 0);
    const u64 later = heads & ~at_or_below;
    const u64 run = (later ? (later & (~later + 1)) - 1 : ~0ull) & ~below & valid;
    if (molecules && first) atomicAdd(&molecules[e], (u64)__popcll(run));
    if (reads) {
      const u64 mine = in ? t.cnt[slots[r]] : 0;
      u64 sum = mine;  // the inclusive prefix sums of the tile's mreads
      for (int o = 1; o < 64; o <<= 1) {
        const u64 up = __shfl_up(sum, o);
        if (lane >= o) sum += up;
      }
      const int last = run ? 63 - __clzll((long long)run) : lane;
      const u64 through = __shfl(sum, last);
      if (first) atomicAdd(&reads[e], through - sum + mine);
    }
    if (collapsed) {
      const uint32_t s = in ? slots[r] : 0;
      const u64 images = __ballot(in && (lab ? (lab[s] & kLabelSlot) == s : (bitmap[s >> 5] >> (s & 31)) & 1u));
      const u64 n = (u64)__popcll(images & run);
      if (first && n) atomicAdd(&collapsed[e], n);
    }
  });
}

// ---- resolving features (include/sctools_hip.h, "resolving features"; the word, the head tests and
// the group fold: molecules_resolve_key.h)

// The compaction of the resolve pass: a wave per 64 slots (the capacity is a multiple of 64), and for
// every occupied slot s the re-packed word of its key under its image, with s beside it.  The image
// slot p is s itself (IMAGE_SELF), the one-step parent's by one lane's scan or by the wave's
// (IMAGE_PARENT, IMAGE_PARENT_WAVE: the two forms of the collapse pass, SCT_TUNE_COLLAPSE_FORM) or the
// directional label (IMAGE_ROOT, `lab` as directional_labels left it).  A parent is scanned for once
// per molecule: it is kept in image[s] for the run pass, and its bit is set in `parents` (if not
// NULL), which is then the collapse pass's bitmap.  At most `room` rows are written.
enum { IMAGE_SELF, IMAGE_PARENT, IMAGE_PARENT_WAVE, IMAGE_ROOT };
template <int IMAGE>
__global__ void __launch_bounds__(WG) molecules_resolve_rows_kernel(Set t, int64_t capacity,
                                                                    const uint32_t* __restrict__ lab,
                                                                    uint32_t* __restrict__ image,
                                                                    uint32_t* __restrict__ parents,
                                                                    u64* __restrict__ cursor, int64_t room,
                                                                    u64* __restrict__ out_word,
                                                                    uint32_t* __restrict__ out_slot) {
  const int lane = threadIdx.x & 63;
  for_each_wave_tile(capacity, [&](int64_t base) {
    const uint32_t s = (uint32_t)(base + lane);
    const u64 key = t.keys[s];
    const bool occ = key != EMPTY;
    uint32_t p = s;
    u64 image_key = key;
    if (IMAGE == IMAGE_PARENT && occ) {
      const Candidate b = parent_scan(t, key, s, 0, 1);
      p = b.slot, image_key = b.code;
    }
    if (IMAGE == IMAGE_PARENT_WAVE)
      wave_serial(__ballot(occ), [&](int src) {
        const Candidate b = wave_max(parent_scan(t, __shfl(key, src), (uint32_t)(base + src), lane, 64));
        if (lane == src) p = b.slot, image_key = b.code;
      });
    if (IMAGE == IMAGE_ROOT && occ) {
      p = lab[s] & kLabelSlot;
      image_key = t.keys[p];
    }
    if ((IMAGE == IMAGE_PARENT || IMAGE == IMAGE_PARENT_WAVE) && occ) {
      image[s] = p;
      if (parents) atomicOr(&parents[p >> 5], 1u << (p & 31));
    }
    const u64 at = compact_at(occ, cursor);
    if (occ && (int64_t)at < room) {
      out_word[at] = sct::mol_resolve_word_of(key, image_key, t.feat_bits, t.umi_bits);
      out_slot[at] = s;
    }
  });
}

// The run pass over the rows sorted by word, a wave per 64 adjacent rows.  The lane whose row opens a
// group (the previous row is the lane below's; lane 0 reads it from global memory, as row_is_head
// does) walks forward over the group's rows to its end, wherever that lies: no tile hands anything to
// the next.  On the way it sums cnt[slot] over the rows of each collapsed molecule, folds the
// molecules by mol_resolve_combine and remembers the image slot of the best.  A unique best keeps its
// molecule: its image slot's bit is set in `kept` (a bit per table slot, zero before) and
// resolved[index] += 1 (if not NULL), merged per wave and index.  tally[4] += the groups of two or
// more members, the lost members, the tied members and the reads of both, one add per wave and word.
// Past the last row stands a word no key packs to (a word's top bit is 0).
constexpr u64 kNoWord = ~0ull;
__global__ void __launch_bounds__(WG) molecules_resolve_kernel(Set t, const u64* __restrict__ words,
                                                               const uint32_t* __restrict__ slots, int64_t rows,
                                                               const uint32_t* __restrict__ image,
                                                               uint32_t* __restrict__ kept, u64* __restrict__ resolved,
                                                               u64* __restrict__ tally) {
  const int lane = threadIdx.x & 63;
  u64 sums[4] = {};  // n_shared, n_lost, n_tied, reads_dropped
  for_each_wave_tile(rows, [&](int64_t base) {
    const int64_t r = base + lane;
    const bool in = r < rows;
    const u64 word = in ? words[r] : 0;
    u64 prev = __shfl_up(word, 1);
    if (lane == 0 && in && r > 0) prev = words[r - 1];
    const bool head = in && (r == 0 || sct::mol_resolve_group_head(word, prev, t.feat_bits));
    bool keeps = false;
    if (head) {
      sct::ResolveGroup g{0, 0, 0, 0};
      uint32_t winner = 0;
      int64_t q = r;
      u64 w = word;
      for (;;) {  // a collapsed molecule per turn: the rows that carry the word w
        const uint32_t first = slots[q];
        const uint32_t p = image ? image[first] & kLabelSlot : first;
        u64 reads = 0, next;
        do {
          reads += t.cnt[slots[q]];
          next = ++q < rows ? words[q] : kNoWord;
        } while (!sct::mol_resolve_molecule_head(next, w));
        if (reads > g.top) winner = p;
        g = sct::mol_resolve_combine(g, sct::mol_resolve_member(reads));
        if (sct::mol_resolve_group_head(next, w, t.feat_bits)) break;
        w = next;
      }
      keeps = sct::mol_resolve_unique(g);
      sums[0] += g.members >= 2;
      if (keeps) {
        sums[1] += g.members - 1;
        sums[3] += g.reads - g.top;
        atomicOr(&kept[winner >> 5], 1u << (winner & 31));
      } else {
        sums[2] += g.members;
        sums[3] += g.reads;
      }
    }
    const u64 index = sct::mol_resolve_index(word, t.feat_bits, t.umi_bits);
    const Merged m = wave_merge(keeps, index);
    if (resolved && m.rep) atomicAdd(&resolved[index], m.count);
  });
  for (int k = 0; k < 4; ++k) {
    for (int o = 32; o > 0; o >>= 1) sums[k] += __shfl_xor(sums[k], o);
    if (lane == 0 && sums[k]) atomicAdd(&tally[k], sums[k]);
  }
}

// ---- merge (include/sctools_hip.h, "merging molecule counters")

// Slot i of another counted table read in place, once and past the caches: its key (EMPTY for an empty
// slot or a lane past the end) and the molecule's reads.
__device__ __forceinline__ void counted_row(const u64* __restrict__ keys, const u64* __restrict__ cnt, int64_t i,
                                            bool in, u64* key, u64* r) {
  *key = EMPTY, *r = 0;
  if (!in) return;
  *key = __builtin_nontemporal_load(&keys[i]);
  *r = __builtin_nontemporal_load(&cnt[i]);
}

// `count` reads of a molecule of another counted table into `t`: the claim, and reads[index] += count
// (the index comes out of a stored key: index < nw).  What a downsample and a swapped-molecule removal
// do with a survivor; the merge adds whole reads[] arrays instead.
__device__ __forceinline__ int set_take(const Set& t, u64 key, u64 count) {
  const uint32_t index = sct::mol_key_index(key, t.idx_shift);
  atomicAdd(&t.reads[index], count);
  return set_claim<true>(t, key, index, count);
}

// The rows (keys[], cnt[] or NULL, n) of another counter into the table `t`: its own table as it
// stands (n = its capacity; a row equal to EMPTY is an empty slot and is skipped) or its occupied
// rows, dense.  A row is one molecule: the key is claimed in `t` by the insert's rule -- the lane
// whose CAS took the slot, and only that lane, adds 1 to molecules[index] -- and, COUNTED, the row's
// reads are added to the slot's.  The source is read once, coalesced and past the caches; the plain
// instantiation never looks at cnt.  Claims are summed per wave into the size word.  reads, the
// tally and total are not this kernel's (molecules_add_kernel, the host).
template <bool COUNTED>
__global__ void __launch_bounds__(WG) molecules_merge_kernel(Set t, const u64* __restrict__ keys,
                                                             const u64* __restrict__ cnt, int64_t n) {
  int claims = 0;
  for_each_item(n, [&](int64_t i, bool in) {
    u64 key = EMPTY, count = 0;
    if (in) {
      key = __builtin_nontemporal_load(&keys[i]);
      if (COUNTED) count = __builtin_nontemporal_load(&cnt[i]);
    }
    if (key != EMPTY) claims += set_claim<COUNTED>(t, key, sct::mol_key_index(key, t.idx_shift), count);
  });
  add_claims(&t.words[W_SIZE], claims);
}

// reads[nw] += the other counter's, and its tallies (the fourth is 0 without features) (`words` is its device words or a copy)
__global__ void __launch_bounds__(WG) molecules_add_kernel(u64* __restrict__ reads, u64* __restrict__ words,
                                                           const u64* __restrict__ from_reads,
                                                           const u64* __restrict__ from_words, int64_t nw) {
  const int64_t gid = (int64_t)blockIdx.x * WG + threadIdx.x;
  for (int64_t i = gid; i < nw; i += (int64_t)gridDim.x * WG) reads[i] += from_reads[i];
  if (gid < 4) words[W_TALLY + gid] += from_words[W_TALLY + gid];
}

// ---- downsampling (include/sctools_hip.h, "downsampling reads"; the draw: downsample_draw.h)

// what a share of a molecule's reads gives: the reads kept (at the last threshold) and the lowest
// bucket among them (any value at or above the number of thresholds when none is kept)
struct Thinned {
  u64 kept;
  int first;
};

// The walk of the three kernels below over a counted table in place (n = its capacity): a grid stride
// with the wave kept whole, keys and mreads loaded once and past the caches.  A molecule of fewer than
// `wave_reads` reads is thinned by its own lane, share(stream, 0, 1, r).  The others are taken one
// after the other by the whole wave, the shape of molecules_collapse_wave_kernel: lane l takes the
// reads j = l, l + 64, ..., the shares are summed (and the lowest bucket taken) across the wave, and
// the molecule's own lane goes on.  molecule(key, thinned) runs once per stored molecule, in its lane.
template <class Share, class Molecule>
__device__ __forceinline__ void downsample_walk(const u64* __restrict__ keys, const u64* __restrict__ cnt, int64_t n,
                                                u64 seed, u64 wave_reads, Share share, Molecule molecule) {
  const int lane = threadIdx.x & 63;
  for_each_item(n, [&](int64_t i, bool in) {
    u64 key, r;
    counted_row(keys, cnt, i, in, &key, &r);
    const bool occ = key != EMPTY;
    const u64 stream = sct::downsample_stream(seed, key);
    const bool heavy = occ && r >= wave_reads;
    if (occ && !heavy) molecule(key, share(stream, 0, 1, r));
    wave_serial(__ballot(heavy), [&](int src) {
      Thinned m = share(__shfl(stream, src), (u64)lane, 64, __shfl(r, src));
      for (int o = 32; o > 0; o >>= 1) {
        m.kept += __shfl_xor(m.kept, o);
        m.first = min(m.first, __shfl_xor(m.first, o));
      }
      if (lane == src) molecule(key, m);
    });
  });
}

// Thin-and-claim, molecules_merge_kernel<true> with the draw in front: a molecule of `src` that keeps
// m > 0 of its reads at `threshold` is claimed in `t` by the insert's rule, with m as its count, and
// reads[index] += m.  A molecule that keeps none leaves no trace.  Claims are summed per wave into the
// size word; the tally and total are not this kernel's.
__global__ void __launch_bounds__(WG) molecules_downsample_kernel(Set t, const u64* __restrict__ keys,
                                                                  const u64* __restrict__ cnt, int64_t n,
                                                                  u64 threshold, u64 seed, u64 wave_reads) {
  int claims = 0;
  downsample_walk(
      keys, cnt, n, seed, wave_reads,
      [&](u64 stream, u64 j0, u64 step, u64 r) {
        return Thinned{sct::downsample_thin_stride(stream, j0, step, r, threshold), 0};
      },
      [&](u64 key, const Thinned& m) {
        if (m.kept != 0) claims += set_take(t, key, m.kept);
      });
  add_claims(&t.words[W_SIZE], claims);
}

// The curve at one threshold: *reads += the reads kept, *molecules += the molecules that keep any.
// The sums stay in lane registers and are reduced once per wave: one add per wave and word.
__global__ void __launch_bounds__(WG) molecules_downsample_count_kernel(const u64* __restrict__ keys,
                                                                        const u64* __restrict__ cnt, int64_t n,
                                                                        u64 threshold, u64 seed, u64 wave_reads,
                                                                        u64* __restrict__ reads,
                                                                        u64* __restrict__ molecules) {
  u64 kept = 0, alive = 0;
  downsample_walk(
      keys, cnt, n, seed, wave_reads,
      [&](u64 stream, u64 j0, u64 step, u64 r) {
        return Thinned{sct::downsample_thin_stride(stream, j0, step, r, threshold), 0};
      },
      [&](u64, const Thinned& m) {
        kept += m.kept;
        alive += m.kept != 0;
      });
  for (int o = 32; o > 0; o >>= 1) {
    kept += __shfl_xor(kept, o);
    alive += __shfl_xor(alive, o);
  }
  if ((threadIdx.x & 63) != 0) return;
  if (kept) atomicAdd(reads, kept);
  if (alive) atomicAdd(molecules, alive);
}

// The whole curve in one walk.  The k ascending thresholds lie in LDS; a read's bucket is the first
// threshold that keeps it (a binary search), a molecule's bucket the lowest of its reads'.  Both are
// counted into a per-workgroup LDS histogram -- a read or molecule that no threshold keeps counts
// nowhere -- and at the end of the workgroup the inclusive prefix over the buckets turns "first kept
// at t" into "kept at t": one 64-bit add per non-zero word.  reads[k] and molecules[k] are added to.
struct CurvePoints {
  u64 threshold[sct::kDownsampleMaxPoints];
};
__global__ void __launch_bounds__(WG) molecules_downsample_curve_kernel(const u64* __restrict__ keys,
                                                                        const u64* __restrict__ cnt, int64_t n,
                                                                        CurvePoints points, int k, u64 seed,
                                                                        u64 wave_reads, u64* __restrict__ reads,
                                                                        u64* __restrict__ molecules) {
  constexpr int K = sct::kDownsampleMaxPoints;
  __shared__ uint64_t threshold[K];
  __shared__ u64 first_kept[2][K];  // [0] reads, [1] molecules, by bucket
  for (int t = threadIdx.x; t < K; t += WG) {
    threshold[t] = points.threshold[t < k ? t : k - 1];
    first_kept[0][t] = first_kept[1][t] = 0;
  }
  __syncthreads();
  downsample_walk(
      keys, cnt, n, seed, wave_reads,
      [&](u64 stream, u64 j0, u64 step, u64 r) {
        Thinned m{0, k};
        for (u64 j = j0; j < r; j += step) {
          const int b = sct::downsample_bucket(sct::downsample_draw_at(stream, j), threshold, k);
          if (b >= k) continue;
          atomicAdd(&first_kept[0][b], 1ull);
          m.kept += 1;
          m.first = min(m.first, b);
        }
        return m;
      },
      [&](u64, const Thinned& m) {
        if (m.first < k) atomicAdd(&first_kept[1][m.first], 1ull);
      });
  __syncthreads();
  if ((int)threadIdx.x >= 2 * k) return;
  const int what = (int)threadIdx.x / k, t = (int)threadIdx.x % k;
  u64 sum = 0;
  for (int b = 0; b <= t; ++b) sum += first_kept[what][b];
  if (sum) atomicAdd(what == 0 ? &reads[t] : &molecules[t], sum);
}

// words[W_TALLY + k] += the reads of tally k kept at `threshold`: read j < from.n[k] draws under the
// key no molecule can have (downsample_tally_key).  A grid stride over j, one add per wave and tally.
struct TallyReads {
  u64 n[4];
};
__global__ void __launch_bounds__(WG) molecules_downsample_tally_kernel(TallyReads from, u64 threshold, u64 seed,
                                                                        u64* __restrict__ words) {
  const u64 gid = (u64)blockIdx.x * WG + threadIdx.x, stride = (u64)gridDim.x * WG;
  for (int k = 0; k < 4; ++k) {
    const u64 stream = sct::downsample_stream(seed, sct::downsample_tally_key(k));
    u64 kept = sct::downsample_thin_stride(stream, gid, stride, from.n[k], threshold);
    for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o);
    if ((threadIdx.x & 63) == 0 && kept) atomicAdd(&words[W_TALLY + k], kept);
  }
}

// ---- removing swapped molecules (include/sctools_hip.h, "removing swapped molecules"; the judgement:
// swapped_keep.h)

// the other samples' tables, by value: at most 15 of them are probed, 24 B each
struct ProbedTables {
  struct {
    const u64* keys;
    const u64* cnt;
    u64 mask;
  } of[sct::kSwappedMaxSamples];
};
enum { S_SHARED = 0, S_REMOVED, S_REMOVED_READS, S_KEPT_READS, S_NWORDS };

// The marking pass over one sample's table in place (n = its capacity, a multiple of 64): the walk of
// downsample_walk, a lane per slot with the wave kept whole.  The lane of an occupied slot loads the
// key's home slot in every other table before it looks at any of them -- one random line per table, in
// flight together -- then finishes each probe as find() would and, where the key is stored, loads its
// reads there; these loads too are issued before their sum is taken.  The kept flags of a wave's 64
// slots are one ballot: the walk's tiles start on multiples of 64 (the grid's stride is a multiple of
// WG), so the word kept[i >> 6] is this wave's alone and lane 0 stores it plainly.  Every word of
// kept[n / 64] is written.  sums[S_NWORDS] += the shared and the removed molecules, the reads of the
// removed and of the kept ones, summed in registers, one add per wave and non-zero word.
__global__ void __launch_bounds__(WG) molecules_swapped_mark_kernel(const u64* __restrict__ keys,
                                                                    const u64* __restrict__ cnt, int64_t n,
                                                                    ProbedTables others, int nothers, u64 num, u64 den,
                                                                    u64* __restrict__ kept, u64* __restrict__ sums) {
  constexpr int kMost = sct::kSwappedMaxSamples - 1;
  const int lane = threadIdx.x & 63;
  u64 acc[S_NWORDS] = {};
  for_each_item(n, [&](int64_t i, bool in) {
    u64 key, r;
    counted_row(keys, cnt, i, in, &key, &r);
    const bool occ = key != EMPTY;
    bool keep = false;
    if (occ) {
      const u64 h = sct::mix64(key);
      u64 first[kMost], slot[kMost], theirs[kMost];
#pragma unroll
      for (int t = 0; t < kMost; ++t)
        if (t < nothers) first[t] = others.of[t].keys[h & others.of[t].mask];
#pragma unroll
      for (int t = 0; t < kMost; ++t)
        if (t < nothers) slot[t] = find_from(others.of[t].keys, others.of[t].mask, key, h & others.of[t].mask, first[t]);
#pragma unroll
      for (int t = 0; t < kMost; ++t)
        if (t < nothers) theirs[t] = slot[t] != NO_SLOT ? others.of[t].cnt[slot[t]] : 0;
      u64 sum = 0;
#pragma unroll
      for (int t = 0; t < kMost; ++t)
        if (t < nothers) sum = sct::swapped_add_sat(sum, theirs[t]);
      keep = sct::swapped_keeps(r, sum, num, den);
      acc[S_SHARED] += sum != 0;
      acc[S_REMOVED] += !keep;
      acc[keep ? S_KEPT_READS : S_REMOVED_READS] += r;
    }
    const u64 word = __ballot(keep);
    if (lane == 0 && in) kept[i >> 6] = word;
  });
  for (int k = 0; k < S_NWORDS; ++k) {
    for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o);
    if (lane == 0 && acc[k]) atomicAdd(&sums[k], acc[k]);
  }
}

// The claim, molecules_merge_kernel<true> with the marking pass's word in front: the molecule of a
// slot whose bit is set in kept[] is claimed in `t` by the insert's rule with its reads as its count,
// and reads[index] += them (set_take, as a downsample's survivor).  The keys and reads of the other
// slots are not loaded.  Claims are summed per wave into the size word; the tally and total are not
// this kernel's.
__global__ void __launch_bounds__(WG) molecules_swapped_claim_kernel(Set t, const u64* __restrict__ keys,
                                                                     const u64* __restrict__ cnt, int64_t n,
                                                                     const u64* __restrict__ kept) {
  int claims = 0;
  for_each_item(n, [&](int64_t i, bool in) {
    const bool mine = in && ((kept[i >> 6] >> (i & 63)) & 1);
    u64 key, r;
    counted_row(keys, cnt, i, mine, &key, &r);
    if (key != EMPTY) claims += set_take(t, key, r);
  });
  add_claims(&t.words[W_SIZE], claims);
}

}  // namespace

struct sct_molecules : Host {
  sct_molecules() : Host("molecule") {}
  int idx_bits = 0;
  Set t{};               // t.words is Host::words
  bool counted = false;  // keeps t.cnt beside t.keys
  // what the last directional pass took (sct_molecules_directional_info)
  int64_t dir_sweeps = 0, dir_listed = 0, dir_swept = 0;
};

namespace {

// A device made current for a scope, and the caller's put back: a counter's calls run on the
// counter's device (its allocations, the pool, the thread's host stage and every launch follow the
// current device) whatever device the caller had current.
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  hipError_t e;
  explicit DeviceGuard(int device) {
    e = hipGetDevice(&prev);
    if (e == hipSuccess && prev != device) {
      e = hipSetDevice(device);
      switched = e == hipSuccess;
    }
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
};

// in every call on a counter, after the argument checks and before the counter is used: its device
// is current until the call returns
#define SCT_ON_DEVICE_OF(c)                                                                       \
  DeviceGuard on_device_((c)->device);                                                            \
  if (on_device_.e != hipSuccess)                                                                 \
  return sct::fail(SCT_E_HIP, "molecule counter's device %d: %s", (c)->device, hipGetErrorString(on_device_.e))

// the same for a call that works on host arrays: `s` is this thread's stage stream of that device
#define SCT_ON_STAGE_OF(c, s)                  \
  SCT_ON_DEVICE_OF(c);                         \
  sct::HostStage* stage_ = sct::host_stage();  \
  if (!stage_) return SCT_E_HIP;               \
  hipStream_t s = stage_->stream

// a table's keys are filled with 0xFF, every slot EMPTY; a counted table's mreads with 0 (an insert
// adds to it, a rehash stores into it)
constexpr const char* kKeysName = "molecule table";
constexpr const char* kCountsName = "molecule read counts";

int grow(sct_molecules* c, int64_t factor, hipStream_t s) {
  const int64_t cap = sct::table_grown(c->capacity, factor);
  if (cap == 0)
    return sct::fail(SCT_E_RANGE, "molecule table cannot grow past %lld slots", (long long)sct::kTableMaxCapacity);
  u64* nk = nullptr;
  u64* nc = nullptr;
  if (int rc = alloc_filled(&nk, cap, 0xFF, s, kKeysName); rc != SCT_OK) return rc;
  if (c->counted) {
    if (int rc = alloc_filled(&nc, cap, 0, s, kCountsName); rc != SCT_OK) {
      (void)hipFree(nk);
      return rc;
    }
  }
  const auto rehash = c->counted ? molecules_rehash_kernel<true> : molecules_rehash_kernel<false>;
  hipLaunchKernelGGL(rehash, dim3(grid_for(c->capacity, 1024)), dim3(WG), 0, s, c->t.keys, c->t.cnt, c->capacity, nk,
                     nc, (u64)cap - 1, c->t.words);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(s);  // the old arrays are read until here
  if (e != hipSuccess) {
    (void)hipFree(nk);
    if (nc) (void)hipFree(nc);
    return sct::fail(SCT_E_HIP, "molecule table rehash: %s", hipGetErrorString(e));
  }
  (void)hipFree(c->t.keys);
  c->t.keys = nk;
  if (c->counted) {
    (void)hipFree(c->t.cnt);
    c->t.cnt = nc;
  }
  c->t.mask = (u64)cap - 1;
  c->capacity = cap;
  return SCT_OK;
}

int range_error(const sct_molecules* c) {
  if (c->t.nf)
    return sct::fail(SCT_E_RANGE, "index outside [-2, %lld) or feature outside [-2, %lld) (not counted)",
                     (long long)c->t.nw, (long long)c->t.nf);
  return sct::fail(SCT_E_RANGE, "index outside [-2, %lld) (not counted)", (long long)c->t.nw);
}

// the update form must be the counter's: three arrays for a feature counter, two for any other
int need_features(const sct_molecules* c, bool features) {
  if (features) {
    SCT_CHECK(c->t.nf != 0, "the molecule counter has no features (sct_molecules_create_features makes one that has)");
  } else {
    SCT_CHECK(c->t.nf == 0, "a feature counter is updated with a feature per read (sct_molecules_update_features)");
  }
  return SCT_OK;
}

// *range is set when the batch held an index outside [-2, nw) or a feature outside [-2, nf) (rules 3
// and 3b; the status stays SCT_OK).  d_feature is the third array of a feature counter, else NULL.
int update_device(sct_molecules* c, const int32_t* d_index, const int32_t* d_feature, const uint64_t* d_umi, int64_t n,
                  hipStream_t s, bool* range) {
  if (int rc = enter(c, s); rc != SCT_OK) return rc;
  const int64_t mode = sct::tune(SCT_TUNE_COUNT_PREAGG, 1);
  const auto launch_batch = [&](int64_t done, int64_t m) -> int {
    const int32_t* idx = d_index + done;
    const u64* umi = reinterpret_cast<const u64*>(d_umi) + done;
    const dim3 grid(mode <= 1 ? grid_for(m, 4 * WG) : grid_for(m, kTile));
    const int32_t* feat = d_feature ? d_feature + done : nullptr;
    const auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(WG), 0, s, c->t, idx, feat, umi, m); };
    const auto of_mode = [&](auto counted, auto features) {
      constexpr bool C = decltype(counted)::value, F = decltype(features)::value;
      if (mode == 0) launch(molecules_insert_kernel<false, C, F>);
      else if (mode == 1) launch(molecules_insert_kernel<true, C, F>);
      else launch(molecules_insert_lds_kernel<C, F>);
    };
    const auto of_counted = [&](auto features) {
      c->counted ? of_mode(std::true_type{}, features) : of_mode(std::false_type{}, features);
    };
    d_feature ? of_counted(std::true_type{}) : of_counted(std::false_type{});
    SCT_LAUNCH_CHECK();
    return SCT_OK;
  };
  SCT_TRY(feed(c, n, s, [&](int64_t factor) { return grow(c, factor, s); }, launch_batch));
  c->total += n;
  // rule 3: the error word of this call's kernels (the read-back also makes the size exact)
  if (int rc = read_words(c, s); rc != SCT_OK) return rc;
  if (c->h_words[W_ERROR]) {
    *range = true;
    SCT_HIP(hipMemsetAsync(&c->t.words[W_ERROR], 0, 8, s));
  }
  return leave(c, s);
}

// the compaction of c's table on `s` (the cursor is zero): at most `rows` keys, and what goes beside them
void compact(const sct_molecules* c, int beside_what, int64_t rows, u64* out_key, void* beside, hipStream_t s) {
  const auto kernel = beside_what == BESIDE_NONE   ? molecules_compact_kernel<BESIDE_NONE>
                      : beside_what == BESIDE_SLOT ? molecules_compact_kernel<BESIDE_SLOT>
                                                   : molecules_compact_kernel<BESIDE_COUNT>;
  hipLaunchKernelGGL(kernel, dim3(grid_for(c->capacity, 1024)), dim3(WG), 0, s, c->t.keys, c->t.cnt, c->capacity,
                     &c->t.words[W_CURSOR], rows, out_key, beside);
}

// the table's molecules as rows sorted by key (sorted_rows.h), enqueued into sr's block
template <bool SLOTS>
hipError_t sort_rows(const sct_molecules* c, SortedRows<SLOTS>& sr) {
  return sr.sort(&c->t.words[W_CURSOR], [&](u64* keys, uint32_t* slots) {
    compact(c, SLOTS ? BESIDE_SLOT : BESIDE_NONE, sr.rows, keys, slots, sr.s);
  });
}
int key_bits(const sct_molecules* c) { return c->idx_bits + c->t.idx_shift; }

int method_check(int method) {
  SCT_CHECK(method == SCT_COLLAPSE_ONE_STEP || method == SCT_COLLAPSE_DIRECTIONAL,
            "unknown collapse method %d (SCT_COLLAPSE_ONE_STEP or SCT_COLLAPSE_DIRECTIONAL)", method);
  return SCT_OK;
}

// The directional pass's scratch at `b`, in its one layout: three words (the worklist's cursor and the
// sweep's changed word, read back together, and n_corrected), a word per slot and two worklists of an
// entry per molecule, a sweep's own and the one it writes.  The size is exact when it is planned
// (enter_read).
struct DirectionalScratch {
  u64* words;
  uint32_t* lab;
  uint32_t* worklist[2];
  enum { D_CURSOR = 0, D_CHANGED, D_NCORRECTED, D_NWORDS };
  static size_t bytes(const sct_molecules* c) { return 256 + (size_t)c->capacity * 4 + (size_t)c->size_bound * 8; }
  DirectionalScratch(const sct_molecules* c, uint8_t* b)
      : words(reinterpret_cast<u64*>(b)), lab(reinterpret_cast<uint32_t*>(b + 256)),
        worklist{lab + c->capacity, lab + c->capacity + c->size_bound} {}
};

// lab[] of the table as it stands on `s`, which is waited for between the sweeps: the discovery pass,
// then sweeps until one changes nothing -- each over the molecules the pass before it left open
// (SCT_TUNE_DIRECTIONAL_FORM 1, the default; an empty list ends them too) or over the whole table (0).
// The three words are zeroed here.  After k sweeps a label is at least the best ancestor within k + 1
// edges (a sweep reads nothing older than the sweep before it left), so `molecules` sweeps settle any
// table and the cap of molecules + 2 is never met.
int directional_labels(sct_molecules* c, const DirectionalScratch& ds, hipStream_t s) {
  const bool listed = sct::tune(SCT_TUNE_DIRECTIONAL_FORM, 1) != 0;
  const int64_t rows = c->size_bound;
  u64* h_words = &c->h_words[W_CURSOR];  // cursor and changed (free between two read_words)
  const auto read_words = [&]() -> int {
    SCT_HIP(hipMemcpyAsync(h_words, ds.words, 16, hipMemcpyDeviceToHost, s));
    SCT_HIP(hipStreamSynchronize(s));
    return SCT_OK;
  };
  const auto open_left = [&]() { return std::min<int64_t>((int64_t)h_words[DirectionalScratch::D_CURSOR], rows); };
  SCT_HIP(hipMemsetAsync(ds.words, 0, DirectionalScratch::D_NWORDS * 8, s));
  hipLaunchKernelGGL((molecules_directional_kernel<true, false>), dim3(grid_for(c->capacity, WG)), dim3(WG), 0, s, c->t,
                     c->capacity, nullptr, ds.lab, listed ? ds.worklist[0] : nullptr, rows,
                     &ds.words[DirectionalScratch::D_CURSOR], nullptr);
  SCT_LAUNCH_CHECK();
  int64_t n = c->capacity;
  if (listed) {
    SCT_TRY(read_words());
    n = open_left();
  }
  c->dir_listed = listed ? n : rows;
  c->dir_sweeps = c->dir_swept = 0;
  for (int from = 0; n > 0; from ^= 1) {
    if (c->dir_sweeps >= rows + 2)
      return sct::fail(SCT_E_INTERNAL, "directional clusters: %lld sweeps over %lld molecules did not settle",
                       (long long)c->dir_sweeps, (long long)rows);
    SCT_HIP(hipMemsetAsync(ds.words, 0, 16, s));
    if (listed)
      hipLaunchKernelGGL((molecules_directional_kernel<false, true>), dim3(grid_for(n, WG)), dim3(WG), 0, s, c->t, n,
                         ds.worklist[from], ds.lab, ds.worklist[from ^ 1], rows,
                         &ds.words[DirectionalScratch::D_CURSOR], &ds.words[DirectionalScratch::D_CHANGED]);
    else
      hipLaunchKernelGGL((molecules_directional_kernel<false, false>), dim3(grid_for(n, WG)), dim3(WG), 0, s, c->t, n,
                         nullptr, ds.lab, nullptr, 0, nullptr, &ds.words[DirectionalScratch::D_CHANGED]);
    SCT_LAUNCH_CHECK();
    c->dir_sweeps += 1;
    c->dir_swept += listed ? n : rows;
    SCT_TRY(read_words());
    if (h_words[DirectionalScratch::D_CHANGED] == 0) break;
    if (listed) n = open_left();
  }
  return SCT_OK;
}

// the number of molecules, read on `s` after the counter's earlier work; `room` must hold them
int rows_for_fetch(sct_molecules* c, int64_t room, hipStream_t s, int64_t* rows) {
  if (int rc = enter_read(c, s); rc != SCT_OK) return rc;
  *rows = c->size_bound;
  SCT_CHECK(room >= *rows, "room for %lld molecules, the counter holds %lld", (long long)room, (long long)*rows);
  return SCT_OK;
}

// The distinct molecules in ascending key order into device arrays: `rows` > 0 rows, as rows_for_fetch
// gave them on `s`.  Beside index and UMI, each if asked: the feature column of a feature counter,
// each row's mreads and its parent's UMI.  SLOTS: the slots travel through the sort, for the last two.
// The parent of SCT_COLLAPSE_DIRECTIONAL is the root: the labels are made first, in the rows' block.
template <bool SLOTS>
int fetch_rows_as(sct_molecules* c, int method, int32_t* d_index, int32_t* d_feature, uint64_t* d_umi,
                  uint64_t* d_mreads, uint64_t* d_parent, int64_t rows, hipStream_t s) {
  SortedRows<SLOTS> sr(rows, key_bits(c), s);
  const bool roots = SLOTS && d_parent && method == SCT_COLLAPSE_DIRECTIONAL;
  const size_t o_labels = roots ? sr.take(DirectionalScratch::bytes(c)) : 0;
  SCT_HIP(sr.alloc());
  const uint32_t* lab = nullptr;
  if (roots) {
    const DirectionalScratch ds(c, sr.template at<uint8_t>(o_labels));
    SCT_TRY(directional_labels(c, ds, s));
    lab = ds.lab;
  }
  hipError_t e = sort_rows(c, sr);
  if (e == hipSuccess) {
    // (the grid of each form as it was: a row with a slot may cost a parent's probes)
    hipLaunchKernelGGL(molecules_emit_kernel<SLOTS>, dim3(grid_for(rows, SLOTS ? WG : 1024)), dim3(WG), 0, s, c->t,
                       sr.word(), sr.slot(), rows, d_index, d_feature, reinterpret_cast<u64*>(d_umi),
                       reinterpret_cast<u64*>(d_mreads), reinterpret_cast<u64*>(d_parent), lab);
    e = hipGetLastError();
  }
  if (e != hipSuccess) return sct::fail(SCT_E_HIP, "molecule fetch: %s", hipGetErrorString(e));
  return leave(c, s);
}
int fetch_rows(sct_molecules* c, int method, int32_t* d_index, int32_t* d_feature, uint64_t* d_umi,
               uint64_t* d_mreads, uint64_t* d_parent, int64_t rows, hipStream_t s) {
  const auto as = d_mreads || d_parent ? fetch_rows_as<true> : fetch_rows_as<false>;
  return as(c, method, d_index, d_feature, d_umi, d_mreads, d_parent, rows, s);
}

// the device forms: `given` says whether the form's own columns are there, asked only when rows are
int fetch_device(sct_molecules* c, int method, int32_t* d_index, int32_t* d_feature, uint64_t* d_umi,
                 uint64_t* d_mreads, uint64_t* d_parent, bool given, int64_t room, hipStream_t s) {
  SCT_ON_DEVICE_OF(c);
  int64_t rows = 0;
  if (int rc = rows_for_fetch(c, room, s, &rows); rc != SCT_OK) return rc;
  if (rows == 0) return SCT_OK;
  SCT_CHECK(given, "NULL output");
  return fetch_rows(c, method, d_index, d_feature, d_umi, d_mreads, d_parent, rows, s);
}

// the host forms: the columns asked for, staged
int fetch_host(sct_molecules* c, int method, int32_t* index, int32_t* feature, uint64_t* umi, uint64_t* mreads,
               uint64_t* parent, int64_t room) {
  SCT_ON_STAGE_OF(c, s);
  int64_t rows = 0;
  if (int rc = rows_for_fetch(c, room, s, &rows); rc != SCT_OK) return rc;
  if (rows == 0) return SCT_OK;
  Staged st(s);
  st.add(umi, 8, rows), st.add(mreads, 8, rows), st.add(parent, 8, rows);
  st.add(index, 4, rows), st.add(feature, 4, rows);
  if (int rc = st.alloc(); rc != SCT_OK) return rc;
  const int rc = fetch_rows(c, method, st.dev<int32_t>(3), st.dev<int32_t>(4), st.dev<uint64_t>(0),
                            st.dev<uint64_t>(1), st.dev<uint64_t>(2), rows, s);
  return st.finish(rc, "molecule fetch");
}

int need_counted(const sct_molecules* c) {
  SCT_CHECK(c->counted, "the molecule counter keeps no read counts (sct_molecules_create_counted does)");
  return SCT_OK;
}

// The collapse pass's scratch at `b`, in its one layout: the n_corrected word, the bitmap of one bit
// per slot (capacity >= 64: whole words) and, for a caller that keeps no collapsed[nw] of its own,
// that array.  The caller zeroes all of it.
struct CollapseScratch {
  u64* ncorrected;
  uint32_t* bitmap;
  u64* collapsed;
  static size_t bytes(const sct_molecules* c, bool own_collapsed) {
    return 8 + (size_t)c->capacity / 8 + (own_collapsed ? (size_t)c->t.nw * 8 : 0);
  }
  CollapseScratch(const sct_molecules* c, uint8_t* b)
      : ncorrected(reinterpret_cast<u64*>(b)), bitmap(reinterpret_cast<uint32_t*>(b + 8)),
        collapsed(reinterpret_cast<u64*>(b + 8 + (size_t)c->capacity / 8)) {}
};

// the collapse of the table as it stands on `s`, in the form SCT_TUNE_COLLAPSE_FORM names: the parents'
// bits into `bitmap`, collapsed[nw] and the n_corrected word added to (all zero before)
hipError_t collapse_pass(const sct_molecules* c, uint32_t* bitmap, u64* collapsed, u64* ncorrected, hipStream_t s) {
  const bool wave = sct::tune(SCT_TUNE_COLLAPSE_FORM, 1) == 1;
  const auto kernel = wave ? molecules_collapse_wave_kernel : molecules_collapse_kernel;
  hipLaunchKernelGGL(kernel, dim3(grid_for(c->capacity, WG)), dim3(WG), 0, s, c->t, c->capacity, bitmap, collapsed,
                     ncorrected);
  return hipGetLastError();
}

// the directional clusters of the table as it stands on `s`: its labels, then collapsed[nw] and the
// n_corrected word of `ds` added to (collapsed zero before)
int directional_pass(sct_molecules* c, const DirectionalScratch& ds, u64* collapsed, hipStream_t s) {
  SCT_TRY(directional_labels(c, ds, s));
  hipLaunchKernelGGL(molecules_directional_count_kernel, dim3(grid_for(c->capacity, 1024)), dim3(WG), 0, s, c->t,
                     c->capacity, ds.lab, collapsed, &ds.words[DirectionalScratch::D_NCORRECTED]);
  SCT_LAUNCH_CHECK();
  return SCT_OK;
}

// ---- resolving features

// the methods of the resolve entry points: the two collapse methods and SCT_COLLAPSE_NONE
int resolve_method_check(int method) {
  SCT_CHECK(method == SCT_COLLAPSE_ONE_STEP || method == SCT_COLLAPSE_DIRECTIONAL || method == SCT_COLLAPSE_NONE,
            "unknown resolve method %d (SCT_COLLAPSE_ONE_STEP, SCT_COLLAPSE_DIRECTIONAL or SCT_COLLAPSE_NONE)", method);
  return SCT_OK;
}

// The resolve pass's scratch at `b`, in its one layout: the four tally words and the kept bitmap of
// one bit per slot (zeroed together by the pass) and, for the one-step method, the image slot of
// every slot (written for every occupied slot before it is read).  The directional method reads its
// images from the labels and SCT_COLLAPSE_NONE has none.
struct ResolveScratch {
  u64* tally;
  uint32_t* kept;
  uint32_t* image;
  static size_t zeroed(const sct_molecules* c) { return 256 + (size_t)c->capacity / 8; }
  static size_t bytes(const sct_molecules* c, int method) {
    return up256(zeroed(c)) + (method == SCT_COLLAPSE_ONE_STEP ? (size_t)c->capacity * 4 : 0);
  }
  ResolveScratch(const sct_molecules* c, uint8_t* b)
      : tally(reinterpret_cast<u64*>(b)), kept(reinterpret_cast<uint32_t*>(b + 256)),
        image(reinterpret_cast<uint32_t*>(b + up256(zeroed(c)))) {}
};

// The resolve pass of the table as it stands, enqueued on sr's stream in sr's block: the rows under
// their images sorted by the re-packed word, then the run pass -- rs.kept and rs.tally (zeroed here)
// and resolved[nw] (nullable; zero before) added to.  `lab`: the directional labels, made before.
// `parents` (one-step only, nullable, zero before) receives the parents' bits, which makes it the
// collapse pass's bitmap without a second scan.  sr's rows are free again when this returns.
hipError_t resolve_pass(const sct_molecules* c, int method, SortedRows<true>& sr, const ResolveScratch& rs,
                        const uint32_t* lab, uint32_t* parents, u64* resolved) {
  hipStream_t s = sr.s;
  hipError_t e = hipMemsetAsync(rs.tally, 0, ResolveScratch::zeroed(c), s);
  if (e != hipSuccess) return e;
  const bool wave = sct::tune(SCT_TUNE_COLLAPSE_FORM, 1) == 1;
  const auto rows_kernel = method == SCT_COLLAPSE_NONE          ? molecules_resolve_rows_kernel<IMAGE_SELF>
                           : method == SCT_COLLAPSE_DIRECTIONAL ? molecules_resolve_rows_kernel<IMAGE_ROOT>
                           : wave                               ? molecules_resolve_rows_kernel<IMAGE_PARENT_WAVE>
                                                                : molecules_resolve_rows_kernel<IMAGE_PARENT>;
  const uint32_t* image = method == SCT_COLLAPSE_NONE ? nullptr : method == SCT_COLLAPSE_DIRECTIONAL ? lab : rs.image;
  e = sr.sort(&c->t.words[W_CURSOR], [&](u64* words, uint32_t* slots) {
    hipLaunchKernelGGL(rows_kernel, dim3(grid_for(c->capacity, WG)), dim3(WG), 0, s, c->t, c->capacity, lab, rs.image,
                       parents, &c->t.words[W_CURSOR], sr.rows, words, slots);
  });
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(molecules_resolve_kernel, dim3(grid_for((sr.rows + 63) / 64, WG / 64)), dim3(WG), 0, s, c->t,
                     sr.word(), sr.slot(), sr.rows, image, rs.kept, resolved, rs.tally);
  return hipGetLastError();
}

// resolved[nw] and, if asked, tally[4], written on `s` from the table as it stands
int resolve_device(sct_molecules* c, int method, uint64_t* d_resolved, uint64_t* d_tally, hipStream_t s) {
  if (int rc = enter_read(c, s); rc != SCT_OK) return rc;
  SCT_HIP(hipMemsetAsync(d_resolved, 0, (size_t)c->t.nw * 8, s));
  if (c->size_bound == 0) {
    if (d_tally) SCT_HIP(hipMemsetAsync(d_tally, 0, 4 * 8, s));
    return leave(c, s);
  }
  SortedRows<true> sr(c->size_bound, key_bits(c), s);
  const bool directional = method == SCT_COLLAPSE_DIRECTIONAL;
  const size_t o_labels = directional ? sr.take(DirectionalScratch::bytes(c)) : 0;
  const size_t o_resolve = sr.take(ResolveScratch::bytes(c, method));
  SCT_HIP(sr.alloc());
  const uint32_t* lab = nullptr;
  if (directional) {
    const DirectionalScratch ds(c, sr.at<uint8_t>(o_labels));
    SCT_TRY(directional_labels(c, ds, s));
    lab = ds.lab;
  }
  const ResolveScratch rs(c, sr.at<uint8_t>(o_resolve));
  hipError_t e = resolve_pass(c, method, sr, rs, lab, nullptr, reinterpret_cast<u64*>(d_resolved));
  if (e == hipSuccess && d_tally) e = hipMemcpyAsync(d_tally, rs.tally, 4 * 8, hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return sct::fail(SCT_E_HIP, "molecule resolve: %s", hipGetErrorString(e));
  return leave(c, s);
}

// collapsed[nw] and, if asked, n_corrected of the directional clusters
int collapse_directional_device(sct_molecules* c, uint64_t* d_collapsed, uint64_t* d_ncorrected, hipStream_t s) {
  if (int rc = enter_read(c, s); rc != SCT_OK) return rc;
  SCT_HIP(hipMemsetAsync(d_collapsed, 0, (size_t)c->t.nw * 8, s));
  if (d_ncorrected) SCT_HIP(hipMemsetAsync(d_ncorrected, 0, 8, s));
  if (c->size_bound > 0) {
    sct::PoolBlock blk(s);
    SCT_TRY(blk.alloc(DirectionalScratch::bytes(c)));
    const DirectionalScratch ds(c, blk.bytes());
    int rc = directional_pass(c, ds, reinterpret_cast<u64*>(d_collapsed), s);
    if (rc == SCT_OK && d_ncorrected)
      blk.note(hipMemcpyAsync(d_ncorrected, &ds.words[DirectionalScratch::D_NCORRECTED], 8, hipMemcpyDeviceToDevice, s));
    SCT_TRY(blk.finish(rc, "directional clusters"));
  }
  return leave(c, s);
}

// collapsed[nw] and, if asked, n_corrected, written on `s` from the table as it stands
int collapse_device(sct_molecules* c, int method, uint64_t* d_collapsed, uint64_t* d_ncorrected, hipStream_t s) {
  if (method == SCT_COLLAPSE_DIRECTIONAL) return collapse_directional_device(c, d_collapsed, d_ncorrected, s);
  if (int rc = enter_read(c, s); rc != SCT_OK) return rc;
  const size_t bytes = CollapseScratch::bytes(c, false);
  sct::StreamBlock blk(s);
  SCT_HIP(blk.alloc(bytes));
  const CollapseScratch cs(c, blk.bytes());
  hipError_t e = hipMemsetAsync(blk.p, 0, bytes, s);
  if (e == hipSuccess) e = hipMemsetAsync(d_collapsed, 0, (size_t)c->t.nw * 8, s);
  if (e == hipSuccess && c->size_bound > 0)
    e = collapse_pass(c, cs.bitmap, reinterpret_cast<u64*>(d_collapsed), cs.ncorrected, s);
  if (e == hipSuccess && d_ncorrected) e = hipMemcpyAsync(d_ncorrected, cs.ncorrected, 8, hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return sct::fail(SCT_E_HIP, "molecule collapse: %s", hipGetErrorString(e));
  return leave(c, s);
}

// reads, molecules and the tally copied out on `s` (each destination nullable)
int counts_copy(sct_molecules* c, uint64_t* reads, uint64_t* molecules, uint64_t* tally, hipMemcpyKind kind,
                hipStream_t s) {
  if (int rc = enter(c, s); rc != SCT_OK) return rc;
  const size_t nb = (size_t)c->t.nw * 8;
  if (reads) SCT_HIP(hipMemcpyAsync(reads, c->t.reads, nb, kind, s));
  if (molecules) SCT_HIP(hipMemcpyAsync(molecules, c->t.molecules, nb, kind, s));
  if (tally) SCT_HIP(hipMemcpyAsync(tally, &c->t.words[W_TALLY], 3 * 8, kind, s));
  return leave(c, s);
}

// ---- merge

int merge_check(const sct_molecules* dst, const sct_molecules* src) {
  SCT_CHECK(dst != src, "a molecule counter cannot be merged into itself");
  SCT_CHECK(dst->t.nw == src->t.nw, "merge: the counters' nw differ (%lld and %lld)", (long long)dst->t.nw,
            (long long)src->t.nw);
  SCT_CHECK(dst->t.kind == src->t.kind, "merge: the counters' kind differ (%d and %d)", dst->t.kind, src->t.kind);
  SCT_CHECK(dst->t.umi_bits == src->t.umi_bits, "merge: the counters' L differ (%d and %d)",
            dst->t.umi_bits / dst->t.kind, src->t.umi_bits / src->t.kind);
  SCT_CHECK(dst->t.nf == src->t.nf, "merge: the counters' nf differ (%lld and %lld; 0: no features)",
            (long long)dst->t.nf, (long long)src->t.nf);
  SCT_CHECK(dst->counted == src->counted, "merge: one counter keeps read counts and the other does not");
  return SCT_OK;
}

// Room in dst, which holds `size` molecules, for `incoming` more, every one of which may be new
// (molecules_merge_plan.h): the table is grown on `s` if it must be.  `what` names the operation.
int make_room(sct_molecules* dst, int64_t size, int64_t incoming, const char* what, hipStream_t s) {
  const int64_t cap = sct::mol_merge_capacity(dst->capacity, size, incoming);
  if (cap == 0)
    return sct::fail(SCT_E_RANGE, "%s: %lld + %lld molecules need a table of more than %lld slots", what,
                     (long long)size, (long long)incoming, (long long)sct::kTableMaxCapacity);
  return cap > dst->capacity ? grow(dst, cap / dst->capacity, s) : SCT_OK;
}

// What follows the claim kernel of a merge or a downsample on `s`: from_reads[nw] and the tallies of
// from_words added to dst's, `total` reads and `incoming` molecules more in dst's books (the size a
// bound: the next read of the size word makes it exact), and the work recorded in both counters, the
// first failure kept.  src's later work on `ss`, and src_rows (its scratch, if any) going back there
// with src's device current, wait for the kernels that read them.
int absorbed(sct_molecules* dst, sct_molecules* src, const u64* from_reads, const u64* from_words, int64_t nw,
             int64_t total, int64_t incoming, const char* what, hipStream_t s, hipStream_t ss,
             sct::StreamBlock* src_rows = nullptr) {
  hipLaunchKernelGGL(molecules_add_kernel, dim3(grid_for(nw, 4 * WG)), dim3(WG), 0, s, dst->t.reads, dst->t.words,
                     from_reads, from_words, nw);
  const hipError_t launched = hipGetLastError();
  dst->total += total;
  dst->size_bound += incoming;
  int rc = launched == hipSuccess ? SCT_OK : sct::fail(SCT_E_HIP, "molecule %s: %s", what, hipGetErrorString(launched));
  if (int rl = leave(dst, s); rc == SCT_OK) rc = rl;
  SCT_ON_DEVICE_OF(src);
  if (ss != s) (void)hipStreamWaitEvent(ss, dst->last, 0);
  if (src_rows) src_rows->free();
  if (int rl = leave(src, ss); rc == SCT_OK) rc = rl;
  return rc;
}

// src's occupied rows, dense and unsorted, into `blk`, a pool block on src's device and stream (src's
// device is current): keys[rows] at its head, then *cnt = cnt[rows] for a counted counter, written by
// the compaction beside the keys.
int merge_compact(sct_molecules* src, int64_t rows, sct::StreamBlock& blk, const u64** cnt) {
  Carve cv;
  const size_t o_keys = cv.take((size_t)rows * 8), o_cnt = src->counted ? cv.take((size_t)rows * 8) : 0;
  SCT_HIP(blk.alloc(cv.size));
  u64* counts = src->counted ? reinterpret_cast<u64*>(blk.bytes() + o_cnt) : nullptr;
  *cnt = counts;
  hipError_t e = zero_cursor(&src->t.words[W_CURSOR], blk.s);
  if (e == hipSuccess) {
    compact(src, counts ? BESIDE_COUNT : BESIDE_NONE, rows, reinterpret_cast<u64*>(blk.bytes() + o_keys), counts, blk.s);
    e = hipGetLastError();
  }
  if (e != hipSuccess) return sct::fail(SCT_E_HIP, "molecule merge, compacting the source: %s", hipGetErrorString(e));
  return SCT_OK;
}

// dst <- dst + src on `s`, a stream of dst's device (the contract: include/sctools_hip.h).  `dense`:
// src's rows, reads and words travel into scratch on dst's device first, which is the only way
// between two devices; otherwise the kernels read src's own arrays.
int merge(sct_molecules* dst, sct_molecules* src, hipStream_t s) {
  const bool dense = dst->device != src->device || sct::tune(SCT_TUNE_MERGE_ROWS, 0) == 1;
  // the two sizes, read once; nothing has changed when one of these steps fails
  hipStream_t ss = s;  // src's side of a dense merge runs on the thread's stage stream of src's device
  {
    SCT_ON_DEVICE_OF(src);
    if (dense) {
      sct::HostStage* hs = sct::host_stage();
      if (!hs) return SCT_E_HIP;
      ss = hs->stream;
    }
    SCT_TRY(enter_read(src, ss));  // SCT_E_RANGE for a source that overflowed
  }
  const int64_t src_size = src->size_bound;
  SCT_ON_DEVICE_OF(dst);
  SCT_TRY(enter_read(dst, s));
  SCT_TRY(make_room(dst, dst->size_bound, src_size, "merge", s));

  const int64_t nw = dst->t.nw;
  const u64* keys = src->t.keys;
  const u64* cnt = src->t.cnt;
  const u64* from_reads = src->t.reads;
  const u64* from_words = src->t.words;
  int64_t nrows = src->capacity;
  sct::StreamBlock src_blk(ss), dst_blk(s);
  if (dense) {
    const u64* src_cnt = nullptr;  // in src_blk, whose head is the keys
    if (src_size > 0) {
      SCT_ON_DEVICE_OF(src);
      SCT_TRY(merge_compact(src, src_size, src_blk, &src_cnt));
    }
    {  // src's arrays are read by dst's stream from here on: after what src's stream has enqueued
      SCT_ON_DEVICE_OF(src);
      SCT_TRY(leave(src, ss));
    }
    Carve cv;
    const size_t o_words = cv.take(W_NWORDS * 8), o_reads = cv.take((size_t)nw * 8);
    const size_t o_keys = cv.take((size_t)src_size * 8), o_cnt = src->counted ? cv.take((size_t)src_size * 8) : 0;
    hipError_t e = dst_blk.alloc(cv.size);
    uint8_t* b = dst_blk.bytes();
    if (e == hipSuccess && ss != s) e = hipStreamWaitEvent(s, src->last, 0);
    if (e == hipSuccess) e = hipMemcpyPeerAsync(b + o_words, dst->device, src->t.words, src->device, W_NWORDS * 8, s);
    if (e == hipSuccess) e = hipMemcpyPeerAsync(b + o_reads, dst->device, src->t.reads, src->device, (size_t)nw * 8, s);
    if (e == hipSuccess && src_size > 0)
      e = hipMemcpyPeerAsync(b + o_keys, dst->device, src_blk.p, src->device, (size_t)src_size * 8, s);
    if (e == hipSuccess && src_size > 0 && src->counted)
      e = hipMemcpyPeerAsync(b + o_cnt, dst->device, src_cnt, src->device, (size_t)src_size * 8, s);
    if (e != hipSuccess) {
      // nothing of dst has changed; src's rows go back on its own stream, after the copies that read them
      (void)hipStreamSynchronize(s);
      return sct::fail(SCT_E_HIP, "molecule merge, copying the source's rows: %s", hipGetErrorString(e));
    }
    from_words = reinterpret_cast<const u64*>(b + o_words);
    from_reads = reinterpret_cast<const u64*>(b + o_reads);
    keys = reinterpret_cast<const u64*>(b + o_keys);
    cnt = src->counted ? reinterpret_cast<const u64*>(b + o_cnt) : nullptr;
    nrows = src_size;
  }
  if (src_size > 0) {
    const dim3 grid(grid_for(nrows, 4 * WG));
    if (dst->counted)
      hipLaunchKernelGGL(molecules_merge_kernel<true>, grid, dim3(WG), 0, s, dst->t, keys, cnt, nrows);
    else
      hipLaunchKernelGGL(molecules_merge_kernel<false>, grid, dim3(WG), 0, s, dst->t, keys, nullptr, nrows);
  }
  return absorbed(dst, src, from_reads, from_words, nw, src->total, src_size, "merge", s, ss, &src_blk);
}

// ---- downsample

// a molecule of at least this many reads is thinned by its whole wave (SCT_TUNE_DOWNSAMPLE_WAVE_READS;
// DESIGN.md §3.10.7 has the sweep: 64 ahead of 256, 1024 and 4096 where few molecules carry half the reads)
constexpr int64_t kDownsampleWaveReads = 64;
u64 downsample_wave_reads() { return (u64)sct::tune(SCT_TUNE_DOWNSAMPLE_WAVE_READS, kDownsampleWaveReads); }

// The curve of c's table as it stands, enqueued on `s`: reads[k] and molecules[k] (device words, zero
// before) are added to.  One threshold runs the register form, more the LDS histogram.
hipError_t curve_pass(const sct_molecules* c, const uint64_t* thresholds, int k, u64 seed, u64* reads, u64* molecules,
                      hipStream_t s) {
  const dim3 grid(grid_for(c->capacity, 4 * WG));
  if (k == 1) {
    hipLaunchKernelGGL(molecules_downsample_count_kernel, grid, dim3(WG), 0, s, c->t.keys, c->t.cnt, c->capacity,
                       (u64)thresholds[0], seed, downsample_wave_reads(), reads, molecules);
  } else {
    CurvePoints points{};
    for (int t = 0; t < k; ++t) points.threshold[t] = thresholds[t];
    hipLaunchKernelGGL(molecules_downsample_curve_kernel, grid, dim3(WG), 0, s, c->t.keys, c->t.cnt, c->capacity,
                       points, k, seed, downsample_wave_reads(), reads, molecules);
  }
  return hipGetLastError();
}

// reads[k] and molecules[k] (each nullable) written on `s` from the table as it stands
int curve_device(sct_molecules* c, const uint64_t* thresholds, int k, u64 seed, uint64_t* d_reads,
                 uint64_t* d_molecules, hipStream_t s) {
  if (int rc = enter_read(c, s); rc != SCT_OK) return rc;
  sct::StreamBlock blk(s);
  const size_t bytes = (size_t)k * 8;
  SCT_HIP(blk.alloc(2 * bytes));
  u64* sums = static_cast<u64*>(blk.p);
  hipError_t e = hipMemsetAsync(sums, 0, 2 * bytes, s);
  if (e == hipSuccess && c->size_bound > 0) e = curve_pass(c, thresholds, k, seed, sums, sums + k, s);
  if (e == hipSuccess && d_reads) e = hipMemcpyAsync(d_reads, sums, bytes, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess && d_molecules) e = hipMemcpyAsync(d_molecules, sums + k, bytes, hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return sct::fail(SCT_E_HIP, "molecule downsample curve: %s", hipGetErrorString(e));
  return leave(c, s);
}

int curve_check(const sct_molecules* c, const uint64_t* thresholds, int64_t k) {
  SCT_CHECK(c != nullptr, "molecule counter is NULL");
  SCT_CHECK(k >= 1 && k <= sct::kDownsampleMaxPoints, "downsample curve: %lld thresholds, outside [1, %d]",
            (long long)k, sct::kDownsampleMaxPoints);
  SCT_CHECK(thresholds != nullptr, "NULL thresholds");
  SCT_CHECK(sct::downsample_thresholds_ok(thresholds, k),
            "downsample curve: the thresholds must not decrease and none may be above 2^32");
  return need_counted(c);
}

int downsample_check(const sct_molecules* dst, const sct_molecules* src, uint64_t threshold) {
  SCT_CHECK(dst != nullptr && src != nullptr, "molecule counter is NULL");
  SCT_CHECK(dst != src, "a molecule counter cannot be downsampled into itself");
  if (int rc = need_counted(src); rc != SCT_OK) return rc;
  if (int rc = need_counted(dst); rc != SCT_OK) return rc;
  if (int rc = merge_check(dst, src); rc != SCT_OK) return rc;
  SCT_CHECK(threshold <= sct::kDownsampleKeepAll, "downsample: threshold %llu is above 2^32",
            (unsigned long long)threshold);
  SCT_CHECK(dst->device == src->device,
            "downsample: the counters live on devices %d and %d (downsample on the source's device, then merge)",
            dst->device, src->device);
  return SCT_OK;
}

// dst <- dst + src thinned at `threshold`, on `s` (the contract: include/sctools_hip.h).  Both counters
// are counted and live on the device that is current.  The kept reads, molecules and tallies are
// counted into scratch first and read back once; until then nothing of dst has changed.
int downsample(sct_molecules* dst, sct_molecules* src, u64 threshold, u64 seed, hipStream_t s) {
  SCT_TRY(enter_read(src, s));  // SCT_E_RANGE for a source that overflowed
  const int64_t src_size = src->size_bound;
  TallyReads tally{};
  u64 tally_most = 0;
  for (int k = 0; k < 4; ++k) {
    tally.n[k] = src->h_words[W_TALLY + k];
    tally_most = std::max(tally_most, tally.n[k]);
  }
  SCT_TRY(enter_read(dst, s));
  // the scratch has the layout of a counter's device words: the kept tallies where molecules_add_kernel
  // looks for them, the kept reads and molecules in the two words before the counter's own
  sct::StreamBlock blk(s);
  SCT_HIP(blk.alloc(W_NWORDS * 8));
  u64* kept = static_cast<u64*>(blk.p);
  enum { K_READS = 0, K_MOLECULES = 1 };
  static_assert(K_MOLECULES < W_TALLY, "the kept sums lie below the tally");
  hipError_t e = hipMemsetAsync(kept, 0, W_NWORDS * 8, s);
  const uint64_t point = threshold;
  if (e == hipSuccess && src_size > 0) e = curve_pass(src, &point, 1, seed, &kept[K_READS], &kept[K_MOLECULES], s);
  if (e == hipSuccess && tally_most > 0) {
    const int64_t most = (int64_t)std::min<u64>(tally_most, 1ull << 62);
    hipLaunchKernelGGL(molecules_downsample_tally_kernel, dim3(grid_for(most, 64 * WG)), dim3(WG), 0, s, tally,
                       threshold, seed, kept);
    e = hipGetLastError();
  }
  // (dst's read-back words are free between two read_words)
  if (e == hipSuccess) e = hipMemcpyAsync(dst->h_words, kept, W_NWORDS * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess)
    return sct::fail(SCT_E_HIP, "molecule downsample, counting the kept reads: %s", hipGetErrorString(e));
  const int64_t survivors = (int64_t)dst->h_words[K_MOLECULES];
  u64 kept_total = dst->h_words[K_READS];
  for (int k = 0; k < 4; ++k) kept_total += dst->h_words[W_TALLY + k];
  SCT_TRY(make_room(dst, dst->size_bound, survivors, "downsample", s));
  if (survivors > 0)
    hipLaunchKernelGGL(molecules_downsample_kernel, dim3(grid_for(src->capacity, 4 * WG)), dim3(WG), 0, s, dst->t,
                       src->t.keys, src->t.cnt, src->capacity, threshold, seed, downsample_wave_reads());
  // the kept tallies (reads[] was the thinning kernel's: nw = 0 here)
  return absorbed(dst, src, kept, kept, 0, (int64_t)kept_total, survivors, "downsample", s, s);
}

// ---- removing swapped molecules

int swapped_check(sct_molecules* const* src, int64_t ns, int64_t k, const sct_molecules* dst, uint64_t num,
                  uint64_t den) {
  SCT_CHECK(src != nullptr && dst != nullptr, "molecule counter is NULL");
  SCT_CHECK(ns >= 1 && ns <= sct::kSwappedMaxSamples, "remove swapped: %lld samples, outside [1, %d]", (long long)ns,
            sct::kSwappedMaxSamples);
  SCT_CHECK(k >= 0 && k < ns, "remove swapped: sample %lld outside [0, %lld)", (long long)k, (long long)ns);
  SCT_CHECK(sct::swapped_params_ok(ns, num, den),
            "remove swapped: the fraction %llu / %llu must have 1 <= num <= den <= 2^32 and 2 * num > den",
            (unsigned long long)num, (unsigned long long)den);
  for (int64_t t = 0; t < ns; ++t) SCT_CHECK(src[t] != nullptr, "molecule counter is NULL");
  for (int64_t t = 0; t < ns; ++t) {
    SCT_CHECK(src[t] != dst, "remove swapped: the target is sample %lld itself", (long long)t);
    for (int64_t u = 0; u < t; ++u)
      SCT_CHECK(src[u] != src[t], "remove swapped: samples %lld and %lld are the same counter", (long long)u,
                (long long)t);
  }
  if (int rc = need_counted(dst); rc != SCT_OK) return rc;
  for (int64_t t = 0; t < ns; ++t) {
    if (int rc = need_counted(src[t]); rc != SCT_OK) return rc;
    if (int rc = merge_check(dst, src[t]); rc != SCT_OK) return rc;
  }
  for (int64_t t = 0; t < ns; ++t)
    SCT_CHECK(dst->device == src[t]->device,
              "remove swapped: the counters live on devices %d and %d (merge each into a counter on one device first)",
              dst->device, src[t]->device);
  return SCT_OK;
}

// dst <- dst + the molecules of src[k] that the other samples do not take from it, on `s` (the
// contract: include/sctools_hip.h).  All counters are counted and live on the device that is current.
// The marking pass writes a bit per slot of src[k] and four sums into scratch; they are read back once,
// and until then nothing of dst has changed.
int swapped(sct_molecules* const* src, int64_t ns, int64_t k, sct_molecules* dst, u64 num, u64 den, uint64_t* tally,
            hipStream_t s) {
  sct_molecules* mine = src[k];
  for (int64_t t = 0; t < ns; ++t) SCT_TRY(enter_read(src[t], s));  // SCT_E_RANGE for a sample that overflowed
  const int64_t src_size = mine->size_bound;
  u64 carried = 0;  // the reads of src[k] that never became molecules
  for (int j = 0; j < 4; ++j) carried += mine->h_words[W_TALLY + j];
  SCT_TRY(enter_read(dst, s));
  Carve cv;
  const size_t o_sums = cv.take(S_NWORDS * 8), o_kept = cv.take((size_t)mine->capacity / 8);
  sct::StreamBlock blk(s);
  SCT_HIP(blk.alloc(cv.size));
  u64* sums = reinterpret_cast<u64*>(blk.bytes() + o_sums);
  u64* kept = reinterpret_cast<u64*>(blk.bytes() + o_kept);
  hipError_t e = hipMemsetAsync(sums, 0, S_NWORDS * 8, s);
  if (e == hipSuccess && src_size > 0) {
    ProbedTables others{};
    int nothers = 0;
    for (int64_t t = 0; t < ns; ++t)
      if (t != k && src[t]->size_bound > 0)  // (an empty sample holds nothing to find)
        others.of[nothers++] = {src[t]->t.keys, src[t]->t.cnt, src[t]->t.mask};
    hipLaunchKernelGGL(molecules_swapped_mark_kernel, dim3(grid_for(mine->capacity, 4 * WG)), dim3(WG), 0, s,
                       mine->t.keys, mine->t.cnt, mine->capacity, others, nothers, num, den, kept, sums);
    e = hipGetLastError();
  }
  // (dst's read-back words are free between two read_words)
  static_assert(S_NWORDS <= W_NWORDS, "the sums fit the read-back words");
  if (e == hipSuccess) e = hipMemcpyAsync(dst->h_words, sums, S_NWORDS * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return sct::fail(SCT_E_HIP, "molecule remove swapped, marking: %s", hipGetErrorString(e));
  const u64 shared = dst->h_words[S_SHARED], removed = dst->h_words[S_REMOVED];
  const u64 removed_reads = dst->h_words[S_REMOVED_READS], kept_reads = dst->h_words[S_KEPT_READS];
  const int64_t survivors = src_size - (int64_t)removed;
  SCT_TRY(make_room(dst, dst->size_bound, survivors, "remove swapped", s));
  if (tally) tally[0] = shared, tally[1] = removed, tally[2] = removed_reads;
  if (survivors > 0)
    hipLaunchKernelGGL(molecules_swapped_claim_kernel, dim3(grid_for(mine->capacity, 4 * WG)), dim3(WG), 0, s, dst->t,
                       mine->t.keys, mine->t.cnt, mine->capacity, kept);
  // src[k]'s tallies from its own device words (reads[] was the claim kernel's: nw = 0 here)
  int rc = absorbed(dst, mine, mine->t.reads, mine->t.words, 0, (int64_t)(kept_reads + carried), survivors,
                    "remove swapped", s, s);
  for (int64_t t = 0; t < ns; ++t)
    if (t != k)
      if (int rl = leave(src[t], s); rc == SCT_OK) rc = rl;
  return rc;
}

}  // namespace

namespace {

// nf == 0: a counter without features
int create(int64_t nw, int64_t nf, int kind, int L, int64_t capacity_hint, int flags, int device, sct_molecules** out) {
  SCT_CHECK(out != nullptr, "molecule counter is NULL");
  *out = nullptr;
  SCT_CHECK((flags & ~SCT_MOLECULES_COUNTED) == 0, "unknown flags 0x%x", (unsigned)flags);
  const bool counted = (flags & SCT_MOLECULES_COUNTED) != 0;
  SCT_CHECK(device >= -1, "device %d: a HIP ordinal, or -1 for the current device", device);
  SCT_CHECK(nw >= 1 && nw < (1LL << 31), "nw %lld outside [1, 2^31)", (long long)nw);
  SCT_CHECK(kind == 2 || kind == 3, "kind must be 2 (TwoBit) or 3 (ThreeBit)");
  SCT_CHECK(L >= 1, "UMI length L must be >= 1");
  const int umi_bits = sct::mol_umi_bits(nw, kind, L);
  SCT_CHECK(umi_bits > 0, "index bits %d + UMI bits %lld do not fit a 63-bit key", sct::mol_idx_bits(nw),
            (long long)kind * L);
  const int feat_bits = nf ? sct::mol_feat_bits(nf) : 0;
  SCT_CHECK(nf == 0 || sct::mol_feature_umi_bits(nw, nf, kind, L) > 0,
            "index bits %d + feature bits %d + UMI bits %d do not fit a 63-bit key", sct::mol_idx_bits(nw), feat_bits,
            umi_bits);
  SCT_CHECK(capacity_hint >= 0 && capacity_hint <= sct::kTableMaxCapacity, "capacity hint %lld outside [0, 2^31]",
            (long long)capacity_hint);
  const int64_t cap = sct::table_capacity_for(capacity_hint);
  hipError_t e = hipSuccess;
  if (device < 0) {
    e = hipGetDevice(&device);
  } else {
    int ndev = 0;
    e = hipGetDeviceCount(&ndev);
    SCT_CHECK(e != hipSuccess || device < ndev, "device %d: %d device(s) are visible", device, ndev);
  }
  if (e != hipSuccess) return sct::fail(SCT_E_HIP, "molecule counter: %s", hipGetErrorString(e));
  DeviceGuard on_device(device);
  if (on_device.e != hipSuccess)
    return sct::fail(SCT_E_HIP, "molecule counter on device %d: %s", device, hipGetErrorString(on_device.e));
  auto* c = new sct_molecules();
  c->device = device;
  const auto fail_with = [&](int rc) {
    sct_molecules_destroy(c);
    return rc;
  };
  sct::HostStage* hs = sct::host_stage();
  if (!hs) return fail_with(SCT_E_HIP);
  c->capacity = cap;
  c->counted = counted;
  c->idx_bits = sct::mol_idx_bits(nw);
  c->t.nw = nw;
  c->t.kind = kind;
  c->t.umi_bits = umi_bits;
  c->t.nf = nf;
  c->t.feat_bits = feat_bits;
  c->t.idx_shift = feat_bits + umi_bits;
  c->t.mask = (u64)cap - 1;
  if (int rc = alloc_filled(&c->t.keys, cap, 0xFF, hs->stream, kKeysName); rc != SCT_OK) return fail_with(rc);
  if (counted)
    if (int rc = alloc_filled(&c->t.cnt, cap, 0, hs->stream, kCountsName); rc != SCT_OK) return fail_with(rc);
  // reads and molecules are one allocation of 2 * nw words, the tally lives in the device words
  e = hipMalloc((void**)&c->t.reads, (size_t)nw * 16);
  if (e == hipSuccess) {
    c->t.molecules = c->t.reads + nw;
    e = hipMemsetAsync(c->t.reads, 0, (size_t)nw * 16, hs->stream);
  }
  if (e == hipSuccess) e = open_words(c);
  c->t.words = c->words;
  if (e == hipSuccess) e = hipMemsetAsync(c->words, 0, W_NWORDS * 8, hs->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(hs->stream);
  if (e != hipSuccess)
    return fail_with(sct::fail(e == hipErrorOutOfMemory ? SCT_E_NOMEM : SCT_E_HIP, "molecule counter: %s",
                               hipGetErrorString(e)));
  *out = c;
  return SCT_OK;
}

}  // namespace

extern "C" int sct_molecules_create_ex(int64_t nw, int kind, int L, int64_t capacity_hint, int flags, int device,
                                       sct_molecules** out) {
  return create(nw, 0, kind, L, capacity_hint, flags, device, out);
}

extern "C" int sct_molecules_create_features(int64_t nw, int64_t nf, int kind, int L, int64_t capacity_hint, int flags,
                                             int device, sct_molecules** out) {
  SCT_CHECK(out != nullptr, "molecule counter is NULL");
  *out = nullptr;
  SCT_CHECK(nf >= 1 && nf < (1LL << 31), "nf %lld outside [1, 2^31)", (long long)nf);
  return create(nw, nf, kind, L, capacity_hint, flags, device, out);
}

extern "C" int sct_molecules_create(int64_t nw, int kind, int L, int64_t capacity_hint, sct_molecules** out) {
  return sct_molecules_create_ex(nw, kind, L, capacity_hint, 0, -1, out);
}

extern "C" int sct_molecules_create_counted(int64_t nw, int kind, int L, int64_t capacity_hint, sct_molecules** out) {
  return sct_molecules_create_ex(nw, kind, L, capacity_hint, SCT_MOLECULES_COUNTED, -1, out);
}

extern "C" int sct_molecules_destroy(sct_molecules* c) {
  if (!c) return SCT_OK;
  DeviceGuard on_device(c->device);  // (best effort: the frees below name their memory themselves)
  close_words(c);
  if (c->t.keys) (void)hipFree(c->t.keys);
  if (c->t.cnt) (void)hipFree(c->t.cnt);
  if (c->t.reads) (void)hipFree(c->t.reads);
  delete c;
  return SCT_OK;
}

namespace {

// The argument checks of an entry-point family, stated once for its device and its host form.

// the update forms; `features` says which form the caller used, and n == 0 passes with no array looked at
int update_check(const sct_molecules* c, bool features, const int32_t* index, const int32_t* feature,
                 const uint64_t* umi, int64_t n) {
  SCT_CHECK(n >= 0, "n must be >= 0");
  SCT_CHECK(c != nullptr, "molecule counter is NULL");
  if (n == 0) return SCT_OK;
  if (features) SCT_CHECK(index != nullptr && feature != nullptr && umi != nullptr, "NULL index, feature or umi");
  else SCT_CHECK(index != nullptr && umi != nullptr, "NULL index or umi");
  return need_features(c, features);
}

// fetch and fetch_counted (`counted`); the host forms go on to ask for their columns
int fetch_check(const sct_molecules* c, int method, bool counted, int64_t room) {
  SCT_CHECK(room >= 0, "room must be >= 0");
  SCT_CHECK(c != nullptr, "molecule counter is NULL");
  if (int rc = method_check(method); rc != SCT_OK) return rc;
  return counted ? need_counted(c) : SCT_OK;
}

int collapse_check(const sct_molecules* c, int method, const uint64_t* collapsed) {
  SCT_CHECK(c != nullptr, "molecule counter is NULL");
  if (int rc = method_check(method); rc != SCT_OK) return rc;
  if (int rc = need_counted(c); rc != SCT_OK) return rc;
  SCT_CHECK(collapsed != nullptr, "NULL output");
  return SCT_OK;
}

// the two update forms' common part
int update_entry(sct_molecules* c, bool features, const int32_t* d_index, const int32_t* d_feature,
                 const uint64_t* d_umi, int64_t n, void* stream) {
  SCT_TRY(update_check(c, features, d_index, d_feature, d_umi, n));
  if (n == 0) return SCT_OK;
  SCT_ON_DEVICE_OF(c);
  bool range = false;
  const int rc = update_device(c, d_index, d_feature, d_umi, n, sct::as_stream(stream), &range);
  return rc == SCT_OK && range ? range_error(c) : rc;
}

int update_host_entry(sct_molecules* c, bool features, const int32_t* index, const int32_t* feature,
                      const uint64_t* umi, int64_t n) {
  SCT_TRY(update_check(c, features, index, feature, umi, n));
  if (n == 0) return SCT_OK;
  SCT_ON_STAGE_OF(c, s);
  // pieces through one pool buffer (umis, then indices, then features): a piece's copies are ordered
  // after the previous piece's kernels.  An out-of-range index in one piece does not stop the others.
  const int64_t piece = std::min<int64_t>(n, 1LL << 24);
  sct::PoolBlock buf(s);
  if (int rc = buf.alloc((size_t)piece * (features ? 16 : 12)); rc != SCT_OK) return rc;
  uint64_t* d_umi = static_cast<uint64_t*>(buf.p);
  int32_t* d_index = reinterpret_cast<int32_t*>(d_umi + piece);
  int32_t* d_feature = features ? d_index + piece : nullptr;
  int rc = SCT_OK;
  bool range = false;
  for (int64_t b = 0; b < n && rc == SCT_OK && buf.ok(); b += piece) {
    const int64_t m = std::min(piece, n - b);
    buf.note(hipMemcpyAsync(d_umi, umi + b, (size_t)m * 8, hipMemcpyHostToDevice, s));
    if (buf.ok()) buf.note(hipMemcpyAsync(d_index, index + b, (size_t)m * 4, hipMemcpyHostToDevice, s));
    if (buf.ok() && features) buf.note(hipMemcpyAsync(d_feature, feature + b, (size_t)m * 4, hipMemcpyHostToDevice, s));
    if (buf.ok()) rc = update_device(c, d_index, d_feature, d_umi, m, s, &range);
  }
  rc = buf.finish(rc, "molecule update");  // no caller pointer is kept past the return
  return rc == SCT_OK && range ? range_error(c) : rc;
}

}  // namespace

extern "C" int sct_molecules_update(sct_molecules* c, const int32_t* d_index, const uint64_t* d_umi, int64_t n,
                                    void* stream) {
  return update_entry(c, false, d_index, nullptr, d_umi, n, stream);
}

extern "C" int sct_molecules_update_host(sct_molecules* c, const int32_t* index, const uint64_t* umi, int64_t n) {
  return update_host_entry(c, false, index, nullptr, umi, n);
}

extern "C" int sct_molecules_update_features(sct_molecules* c, const int32_t* d_index, const int32_t* d_feature,
                                             const uint64_t* d_umi, int64_t n, void* stream) {
  return update_entry(c, true, d_index, d_feature, d_umi, n, stream);
}

extern "C" int sct_molecules_update_features_host(sct_molecules* c, const int32_t* index, const int32_t* feature,
                                                  const uint64_t* umi, int64_t n) {
  return update_host_entry(c, true, index, feature, umi, n);
}

// the size and the tally words as the counter's work so far leaves them: c->size_bound, c->h_words
static int read_info(sct_molecules* c) {
  SCT_ON_STAGE_OF(c, s);
  return enter_read(c, s);
}

extern "C" int sct_molecules_features_info(sct_molecules* c, int64_t* nf, int64_t* n_no_feature) {
  SCT_CHECK(c != nullptr, "molecule counter is NULL");
  if (n_no_feature) {
    if (int rc = read_info(c); rc != SCT_OK) return rc;
    *n_no_feature = (int64_t)c->h_words[W_TALLY + 3];
  }
  if (nf) *nf = c->t.nf;
  return SCT_OK;
}

extern "C" int sct_molecules_info(sct_molecules* c, int64_t* nmolecules, int64_t* total, int64_t* capacity) {
  SCT_CHECK(c != nullptr, "molecule counter is NULL");
  if (nmolecules) {
    if (int rc = read_info(c); rc != SCT_OK) return rc;
    *nmolecules = c->size_bound;
  }
  if (total) *total = c->total;
  if (capacity) *capacity = c->capacity;
  return SCT_OK;
}

extern "C" int sct_molecules_counts(sct_molecules* c, uint64_t* d_reads, uint64_t* d_molecules, uint64_t* d_tally,
                                    void* stream) {
  SCT_CHECK(c != nullptr, "molecule counter is NULL");
  SCT_ON_DEVICE_OF(c);
  return counts_copy(c, d_reads, d_molecules, d_tally, hipMemcpyDeviceToDevice, sct::as_stream(stream));
}

extern "C" int sct_molecules_counts_host(sct_molecules* c, uint64_t* reads, uint64_t* molecules, uint64_t* tally) {
  SCT_CHECK(c != nullptr, "molecule counter is NULL");
  SCT_ON_STAGE_OF(c, s);
  const int rc = counts_copy(c, reads, molecules, tally, hipMemcpyDeviceToHost, s);
  const hipError_t e = hipStreamSynchronize(s);  // the caller's arrays are written until here
  if (rc == SCT_OK && e != hipSuccess) return sct::fail(SCT_E_HIP, "molecule counts: %s", hipGetErrorString(e));
  return rc;
}

extern "C" int sct_molecules_fetch(sct_molecules* c, int32_t* d_index, uint64_t* d_umi, int64_t room, void* stream) {
  SCT_TRY(fetch_check(c, SCT_COLLAPSE_ONE_STEP, false, room));
  return fetch_device(c, SCT_COLLAPSE_ONE_STEP, d_index, nullptr, d_umi, nullptr, nullptr, d_index && d_umi, room,
                      sct::as_stream(stream));
}

extern "C" int sct_molecules_fetch_host(sct_molecules* c, int32_t* index, uint64_t* umi, int64_t room) {
  SCT_TRY(fetch_check(c, SCT_COLLAPSE_ONE_STEP, false, room));
  SCT_CHECK(room == 0 || (index && umi), "NULL output");
  return fetch_host(c, SCT_COLLAPSE_ONE_STEP, index, nullptr, umi, nullptr, nullptr, room);
}

// The entry points that take a collapse method (include/sctools_hip.h, "directional clusters"); the
// ones without are these with SCT_COLLAPSE_ONE_STEP.
extern "C" int sct_molecules_collapse_by(sct_molecules* c, int method, uint64_t* d_collapsed, uint64_t* d_ncorrected,
                                         void* stream) {
  SCT_TRY(collapse_check(c, method, d_collapsed));
  SCT_ON_DEVICE_OF(c);
  return collapse_device(c, method, d_collapsed, d_ncorrected, sct::as_stream(stream));
}

extern "C" int sct_molecules_collapse(sct_molecules* c, uint64_t* d_collapsed, uint64_t* d_ncorrected, void* stream) {
  return sct_molecules_collapse_by(c, SCT_COLLAPSE_ONE_STEP, d_collapsed, d_ncorrected, stream);
}

extern "C" int sct_molecules_collapse_by_host(sct_molecules* c, int method, uint64_t* collapsed,
                                              uint64_t* ncorrected) {
  SCT_TRY(collapse_check(c, method, collapsed));
  SCT_ON_STAGE_OF(c, s);
  Staged st(s);
  st.add(collapsed, 8, (size_t)c->t.nw), st.add(ncorrected, 8, 1);
  if (int rc = st.alloc(); rc != SCT_OK) return rc;
  return st.finish(collapse_device(c, method, st.dev<uint64_t>(0), st.dev<uint64_t>(1), s), "molecule collapse");
}

extern "C" int sct_molecules_collapse_host(sct_molecules* c, uint64_t* collapsed, uint64_t* ncorrected) {
  return sct_molecules_collapse_by_host(c, SCT_COLLAPSE_ONE_STEP, collapsed, ncorrected);
}

extern "C" int sct_molecules_directional_info(sct_molecules* c, int64_t* sweeps, int64_t* worklist, int64_t* swept) {
  SCT_CHECK(c != nullptr, "molecule counter is NULL");
  if (sweeps) *sweeps = c->dir_sweeps;
  if (worklist) *worklist = c->dir_listed;
  if (swept) *swept = c->dir_swept;
  return SCT_OK;
}

extern "C" int sct_molecules_fetch_counted_by(sct_molecules* c, int method, int32_t* d_index, uint64_t* d_umi,
                                              uint64_t* d_mreads, uint64_t* d_parent, int64_t room, void* stream) {
  SCT_TRY(fetch_check(c, method, true, room));
  return fetch_device(c, method, d_index, nullptr, d_umi, d_mreads, d_parent, d_index && d_umi && d_mreads, room,
                      sct::as_stream(stream));
}

extern "C" int sct_molecules_fetch_counted(sct_molecules* c, int32_t* d_index, uint64_t* d_umi, uint64_t* d_mreads,
                                           uint64_t* d_parent, int64_t room, void* stream) {
  return sct_molecules_fetch_counted_by(c, SCT_COLLAPSE_ONE_STEP, d_index, d_umi, d_mreads, d_parent, room, stream);
}

extern "C" int sct_molecules_fetch_counted_by_host(sct_molecules* c, int method, int32_t* index, uint64_t* umi,
                                                   uint64_t* mreads, uint64_t* parent, int64_t room) {
  SCT_TRY(fetch_check(c, method, true, room));
  SCT_CHECK(room == 0 || (index && umi && mreads), "NULL output");
  return fetch_host(c, method, index, nullptr, umi, mreads, parent, room);
}

extern "C" int sct_molecules_fetch_counted_host(sct_molecules* c, int32_t* index, uint64_t* umi, uint64_t* mreads,
                                                uint64_t* parent, int64_t room) {
  return sct_molecules_fetch_counted_by_host(c, SCT_COLLAPSE_ONE_STEP, index, umi, mreads, parent, room);
}

extern "C" int sct_molecules_merge(sct_molecules* dst, sct_molecules* src, void* stream) {
  SCT_CHECK(dst != nullptr && src != nullptr, "molecule counter is NULL");
  if (int rc = merge_check(dst, src); rc != SCT_OK) return rc;
  return merge(dst, src, sct::as_stream(stream));
}

extern "C" int sct_molecules_downsample(sct_molecules* dst, sct_molecules* src, uint64_t threshold, uint64_t seed,
                                        void* stream) {
  if (int rc = downsample_check(dst, src, threshold); rc != SCT_OK) return rc;
  SCT_ON_DEVICE_OF(dst);
  return downsample(dst, src, (u64)threshold, (u64)seed, sct::as_stream(stream));
}

extern "C" int sct_molecules_downsample_curve(sct_molecules* c, const uint64_t* thresholds, int64_t k, uint64_t seed,
                                              uint64_t* d_reads, uint64_t* d_molecules, void* stream) {
  if (int rc = curve_check(c, thresholds, k); rc != SCT_OK) return rc;
  SCT_ON_DEVICE_OF(c);
  return curve_device(c, thresholds, (int)k, (u64)seed, d_reads, d_molecules, sct::as_stream(stream));
}

extern "C" int sct_molecules_downsample_curve_host(sct_molecules* c, const uint64_t* thresholds, int64_t k,
                                                   uint64_t seed, uint64_t* reads, uint64_t* molecules) {
  if (int rc = curve_check(c, thresholds, k); rc != SCT_OK) return rc;
  SCT_ON_STAGE_OF(c, s);
  Staged st(s);
  st.add(reads, 8, (size_t)k), st.add(molecules, 8, (size_t)k);
  if (int rc = st.alloc(); rc != SCT_OK) return rc;
  return st.finish(curve_device(c, thresholds, (int)k, (u64)seed, st.dev<uint64_t>(0), st.dev<uint64_t>(1), s),
                   "molecule downsample curve");
}

extern "C" int sct_molecules_swapped(sct_molecules* const* src, int64_t s, int64_t k, sct_molecules* dst, uint64_t num,
                                     uint64_t den, uint64_t* tally, void* stream) {
  if (int rc = swapped_check(src, s, k, dst, num, den); rc != SCT_OK) return rc;
  SCT_ON_DEVICE_OF(dst);
  return swapped(src, s, k, dst, (u64)num, (u64)den, tally, sct::as_stream(stream));
}

// ---- counting molecules per feature: the rows with their feature, and the count matrix

namespace {

int need_feature_counter(const sct_molecules* c) {
  SCT_CHECK(c->t.nf != 0, "the molecule counter has no features (sct_molecules_create_features makes one that has)");
  return SCT_OK;
}

// The CSR matrix of the table as it stands, on `s`: d_indptr[nw + 1], d_feature[nnz] and the value
// arrays asked for, each [nnz].  *nnz is a host word, written in every case that gets as far as
// counting the entries; room < nnz is SCT_E_INVALID with nothing else written.  All scratch is the
// one block of the sorted (key, slot) rows: after them the tile head counts and their scan, the entry
// count per barcode and, for the collapsed values, the collapse pass's scratch with a collapsed[nw]
// of its own; both scans run in the sort's scratch.
// `rv` (the resolved matrix, else NULL): the resolve pass runs first, in the same block -- its rows lie
// where the rows sorted by key go afterwards, and its scratch behind the pieces above.  It shares what
// it made with the collapsed values: the labels, or the parents' bitmap (no second neighbour scan).
// resolved[e] is the entry's slots whose bit is set in the kept bitmap, the fill kernel's count of a
// bitmap: in its one launch when collapsed is not asked for, else in a second launch of its value part
// (feature[] is written again with the same values, the entry counts go to a spare array).  tally[4]
// is copied out after the room check, so a call without room writes nothing.
struct ResolvedOut {
  uint64_t* d_resolved;  // [nnz], nullable
  uint64_t* d_tally;     // [4], nullable
};
int matrix_device(sct_molecules* c, int method, int64_t* d_indptr, int32_t* d_feature, uint64_t* d_molecules,
                  uint64_t* d_reads, uint64_t* d_collapsed, const ResolvedOut* rv, int64_t room, int64_t* nnz,
                  hipStream_t s) {
  if (int rc = enter_read(c, s); rc != SCT_OK) return rc;
  const int64_t rows = c->size_bound, nw = c->t.nw;
  SCT_CHECK(nw + 1 < (1LL << 31), "matrix: nw + 1 = %lld row offsets are more than one scan takes", (long long)nw + 1);
  *nnz = 0;
  if (rows == 0) {
    SCT_HIP(hipMemsetAsync(d_indptr, 0, (size_t)(nw + 1) * 8, s));
    if (rv && rv->d_tally) SCT_HIP(hipMemsetAsync(rv->d_tally, 0, 4 * 8, s));
    return leave(c, s);
  }
  const int64_t ntiles = (rows + 63) / 64;
  size_t scan_tiles_bytes = 0, scan_rows_bytes = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scan_tiles_bytes, (const u64*)nullptr, (u64*)nullptr,
                                         (int)(ntiles + 1), s);
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scan_rows_bytes, (const u64*)nullptr, (u64*)nullptr, (int)(nw + 1), s);
  SortedRows<true> sr(rows, key_bits(c), s, std::max(scan_tiles_bytes, scan_rows_bytes));
  const size_t o_heads = sr.take((size_t)(ntiles + 1) * 8), o_base = sr.take((size_t)(ntiles + 1) * 8);
  const size_t o_row_entries = sr.take((size_t)(nw + 1) * 8);
  const bool directional = method == SCT_COLLAPSE_DIRECTIONAL;
  const size_t pass_bytes = directional ? DirectionalScratch::bytes(c) : CollapseScratch::bytes(c, true);
  const size_t o_pass = d_collapsed || (rv && directional) ? sr.take(pass_bytes) : 0;
  const bool second_fill = rv && rv->d_resolved && d_collapsed;
  const size_t o_resolve = rv ? sr.take(ResolveScratch::bytes(c, method)) : 0;
  const size_t o_spare_entries = second_fill ? sr.take((size_t)(nw + 1) * 8) : 0;
  SCT_HIP(sr.alloc());
  u64* heads = sr.at<u64>(o_heads);
  u64* base = sr.at<u64>(o_base);
  u64* row_entries = sr.at<u64>(o_row_entries);
  const u64* keys_out = sr.word();
  const uint32_t* slots_out = sr.slot();
  const dim3 tiles_grid(grid_for(ntiles, WG / 64));
  const uint32_t* bitmap = nullptr;
  const uint32_t* lab = nullptr;
  const uint32_t* kept = nullptr;
  const u64* resolve_tally = nullptr;
  hipError_t e = hipSuccess;
  if (rv) {
    // 0. the resolve pass, with the images it shares with the collapsed values
    uint32_t* parents = nullptr;
    if (directional) {
      const DirectionalScratch ds(c, sr.at<uint8_t>(o_pass));
      SCT_TRY(directional_labels(c, ds, s));
      lab = ds.lab;
    } else if (d_collapsed) {
      e = hipMemsetAsync(sr.at<void>(o_pass), 0, pass_bytes, s);
      bitmap = parents = CollapseScratch(c, sr.at<uint8_t>(o_pass)).bitmap;
    }
    const ResolveScratch rs(c, sr.at<uint8_t>(o_resolve));
    if (e == hipSuccess) e = resolve_pass(c, method, sr, rs, lab, parents, nullptr);
    kept = rs.kept;
    resolve_tally = rs.tally;
  }
  // 1. the rows sorted by key, and the entries that open in every tile; their sum is nnz
  if (e == hipSuccess) e = hipMemsetAsync(&heads[ntiles], 0, 8, s);
  if (e == hipSuccess) e = sort_rows(c, sr);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(molecules_matrix_heads_kernel, tiles_grid, dim3(WG), 0, s, keys_out, rows, c->t.umi_bits, heads);
    e = hipcub::DeviceScan::ExclusiveSum(sr.tmp(), scan_tiles_bytes, heads, base, (int)(ntiles + 1), s);
  }
  // (the host word beside the cursor's read-back is free between two read_words)
  if (e == hipSuccess) e = hipMemcpyAsync(&c->h_words[W_CURSOR], &base[ntiles], 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  const int64_t entries = e == hipSuccess ? (int64_t)c->h_words[W_CURSOR] : 0;
  if (e == hipSuccess && entries <= room) {
    // 2. the entries: feature, the values, the entries of every barcode and their scan
    e = hipMemsetAsync(row_entries, 0, (size_t)(nw + 1) * 8, s);
    if (e == hipSuccess && d_molecules) e = hipMemsetAsync(d_molecules, 0, (size_t)entries * 8, s);
    if (e == hipSuccess && d_reads) e = hipMemsetAsync(d_reads, 0, (size_t)entries * 8, s);
    if (e == hipSuccess && d_collapsed && rv) {
      // (the resolve pass made the labels, or the parents' bitmap)
      e = hipMemsetAsync(d_collapsed, 0, (size_t)entries * 8, s);
    } else if (e == hipSuccess && d_collapsed && directional) {
      // the entry's roots: the labels alone (the sweeps wait for the stream)
      e = hipMemsetAsync(d_collapsed, 0, (size_t)entries * 8, s);
      const DirectionalScratch ds(c, sr.at<uint8_t>(o_pass));
      if (e == hipSuccess) SCT_TRY(directional_labels(c, ds, s));
      lab = ds.lab;
    } else if (e == hipSuccess && d_collapsed) {
      e = hipMemsetAsync(d_collapsed, 0, (size_t)entries * 8, s);
      if (e == hipSuccess) e = hipMemsetAsync(sr.at<void>(o_pass), 0, pass_bytes, s);
      const CollapseScratch cs(c, sr.at<uint8_t>(o_pass));
      bitmap = cs.bitmap;
      if (e == hipSuccess) e = collapse_pass(c, cs.bitmap, cs.collapsed, cs.ncorrected, s);
    }
    u64* d_kept = rv ? reinterpret_cast<u64*>(rv->d_resolved) : nullptr;
    if (e == hipSuccess && d_kept) e = hipMemsetAsync(d_kept, 0, (size_t)entries * 8, s);
    if (e == hipSuccess) {
      // (without collapsed values the kept bitmap takes the bitmap's place in the one launch)
      const bool kept_here = d_kept && !second_fill;
      hipLaunchKernelGGL(molecules_matrix_fill_kernel, tiles_grid, dim3(WG), 0, s, c->t, keys_out, slots_out, rows, base,
                         kept_here ? kept : bitmap, kept_here ? nullptr : lab, row_entries, d_feature,
                         reinterpret_cast<u64*>(d_molecules),
                         reinterpret_cast<u64*>(d_reads), kept_here ? d_kept : reinterpret_cast<u64*>(d_collapsed));
      if (second_fill)
        hipLaunchKernelGGL(molecules_matrix_fill_kernel, tiles_grid, dim3(WG), 0, s, c->t, keys_out, slots_out, rows,
                           base, kept, nullptr, sr.at<u64>(o_spare_entries), d_feature, nullptr, nullptr, d_kept);
      e = hipcub::DeviceScan::ExclusiveSum(sr.tmp(), scan_rows_bytes, row_entries, reinterpret_cast<u64*>(d_indptr),
                                           (int)(nw + 1), s);
    }
    if (e == hipSuccess && rv && rv->d_tally)
      e = hipMemcpyAsync(rv->d_tally, resolve_tally, 4 * 8, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipGetLastError();
  }
  if (e != hipSuccess) return sct::fail(SCT_E_HIP, "molecule matrix: %s", hipGetErrorString(e));
  *nnz = entries;
  if (int rc = leave(c, s); rc != SCT_OK) return rc;
  SCT_CHECK(room >= entries, "room for %lld matrix entries, the matrix has %lld", (long long)room, (long long)entries);
  return SCT_OK;
}

// the checks of fetch_features, device and host: `given` its own columns, `counts` mreads or parent asked for
int fetch_features_check(const sct_molecules* c, int method, bool given, bool counts, int64_t room) {
  if (int rc = fetch_check(c, method, false, room); rc != SCT_OK) return rc;
  SCT_CHECK(room == 0 || given, "NULL output");
  if (int rc = need_feature_counter(c); rc != SCT_OK) return rc;
  return counts ? need_counted(c) : SCT_OK;
}

// the checks every matrix call makes before it touches the device
int matrix_check(const sct_molecules* c, int method, const void* indptr, const void* feature, const void* reads,
                 const void* collapsed, int64_t room, const int64_t* nnz) {
  if (int rc = method_check(method); rc != SCT_OK) return rc;
  SCT_CHECK(room >= 0, "room must be >= 0");
  SCT_CHECK(c != nullptr, "molecule counter is NULL");
  SCT_CHECK(nnz != nullptr, "NULL nnz");
  SCT_CHECK(indptr != nullptr && (room == 0 || feature != nullptr), "NULL output");
  if (int rc = need_feature_counter(c); rc != SCT_OK) return rc;
  if (reads || collapsed)
    if (int rc = need_counted(c); rc != SCT_OK) return rc;
  return SCT_OK;
}

}  // namespace

extern "C" int sct_molecules_fetch_features_by(sct_molecules* c, int method, int32_t* d_index, int32_t* d_feature,
                                               uint64_t* d_umi, uint64_t* d_mreads, uint64_t* d_parent, int64_t room,
                                               void* stream) {
  SCT_TRY(fetch_features_check(c, method, d_index && d_feature && d_umi, d_mreads || d_parent, room));
  return fetch_device(c, method, d_index, d_feature, d_umi, d_mreads, d_parent, true, room, sct::as_stream(stream));
}

extern "C" int sct_molecules_fetch_features(sct_molecules* c, int32_t* d_index, int32_t* d_feature, uint64_t* d_umi,
                                            uint64_t* d_mreads, uint64_t* d_parent, int64_t room, void* stream) {
  return sct_molecules_fetch_features_by(c, SCT_COLLAPSE_ONE_STEP, d_index, d_feature, d_umi, d_mreads, d_parent, room,
                                         stream);
}

extern "C" int sct_molecules_fetch_features_by_host(sct_molecules* c, int method, int32_t* index, int32_t* feature,
                                                    uint64_t* umi, uint64_t* mreads, uint64_t* parent, int64_t room) {
  SCT_TRY(fetch_features_check(c, method, index && feature && umi, mreads || parent, room));
  return fetch_host(c, method, index, feature, umi, mreads, parent, room);
}

extern "C" int sct_molecules_fetch_features_host(sct_molecules* c, int32_t* index, int32_t* feature, uint64_t* umi,
                                                 uint64_t* mreads, uint64_t* parent, int64_t room) {
  return sct_molecules_fetch_features_by_host(c, SCT_COLLAPSE_ONE_STEP, index, feature, umi, mreads, parent, room);
}

extern "C" int sct_molecules_matrix_by(sct_molecules* c, int method, int64_t* d_indptr, int32_t* d_feature,
                                       uint64_t* d_molecules, uint64_t* d_reads, uint64_t* d_collapsed, int64_t room,
                                       int64_t* nnz, void* stream) {
  SCT_TRY(matrix_check(c, method, d_indptr, d_feature, d_reads, d_collapsed, room, nnz));
  SCT_ON_DEVICE_OF(c);
  return matrix_device(c, method, d_indptr, d_feature, d_molecules, d_reads, d_collapsed, nullptr, room, nnz,
                       sct::as_stream(stream));
}

extern "C" int sct_molecules_matrix(sct_molecules* c, int64_t* d_indptr, int32_t* d_feature, uint64_t* d_molecules,
                                    uint64_t* d_reads, uint64_t* d_collapsed, int64_t room, int64_t* nnz, void* stream) {
  return sct_molecules_matrix_by(c, SCT_COLLAPSE_ONE_STEP, d_indptr, d_feature, d_molecules, d_reads, d_collapsed, room,
                                 nnz, stream);
}

extern "C" int sct_molecules_matrix_by_host(sct_molecules* c, int method, int64_t* indptr, int32_t* feature,
                                            uint64_t* molecules, uint64_t* reads, uint64_t* collapsed, int64_t room,
                                            int64_t* nnz) {
  SCT_TRY(matrix_check(c, method, indptr, feature, reads, collapsed, room, nnz));
  SCT_ON_STAGE_OF(c, s);
  if (int rc = enter_read(c, s); rc != SCT_OK) return rc;
  // nnz <= nmolecules: the device arrays never need more room than that
  const int64_t r = std::min(room, c->size_bound);
  Staged st(s);
  st.add(indptr, 8, (size_t)c->t.nw + 1), st.add(feature, 4, r);
  st.add(molecules, 8, r), st.add(reads, 8, r), st.add(collapsed, 8, r);
  if (int rc = st.alloc(); rc != SCT_OK) return rc;
  const int rc = matrix_device(c, method, st.dev<int64_t>(0), st.dev<int32_t>(1), st.dev<uint64_t>(2),
                               st.dev<uint64_t>(3), st.dev<uint64_t>(4), nullptr, r, nnz, s);
  for (int i = 1; i < st.n; ++i) st.cols[i].count = (size_t)*nnz;  // what the matrix wrote of its room
  return st.finish(rc, "molecule matrix");
}

extern "C" int sct_molecules_matrix_host(sct_molecules* c, int64_t* indptr, int32_t* feature, uint64_t* molecules,
                                         uint64_t* reads, uint64_t* collapsed, int64_t room, int64_t* nnz) {
  return sct_molecules_matrix_by_host(c, SCT_COLLAPSE_ONE_STEP, indptr, feature, molecules, reads, collapsed, room, nnz);
}

// ---- resolving features (include/sctools_hip.h): the entry points

namespace {

// what every resolve call needs: a known method and a counted feature counter
int resolve_check(const sct_molecules* c, int method) {
  SCT_CHECK(c != nullptr, "molecule counter is NULL");
  if (int rc = resolve_method_check(method); rc != SCT_OK) return rc;
  if (int rc = need_feature_counter(c); rc != SCT_OK) return rc;
  return need_counted(c);
}

// the checks of the resolved matrix before it touches the device: the matrix's, with the resolve methods
int matrix_resolved_check(const sct_molecules* c, int method, const void* indptr, const void* feature,
                          const void* collapsed, int64_t room, const int64_t* nnz) {
  if (int rc = resolve_check(c, method); rc != SCT_OK) return rc;
  SCT_CHECK(room >= 0, "room must be >= 0");
  SCT_CHECK(nnz != nullptr, "NULL nnz");
  SCT_CHECK(indptr != nullptr && (room == 0 || feature != nullptr), "NULL output");
  SCT_CHECK(!(collapsed && method == SCT_COLLAPSE_NONE), "SCT_COLLAPSE_NONE collapses nothing: no collapsed values");
  return SCT_OK;
}

}  // namespace

extern "C" int sct_molecules_resolve(sct_molecules* c, int method, uint64_t* d_resolved, uint64_t* d_tally,
                                     void* stream) {
  SCT_TRY(resolve_check(c, method));
  SCT_CHECK(d_resolved != nullptr, "NULL output");
  SCT_ON_DEVICE_OF(c);
  return resolve_device(c, method, d_resolved, d_tally, sct::as_stream(stream));
}

extern "C" int sct_molecules_resolve_host(sct_molecules* c, int method, uint64_t* resolved, uint64_t* tally) {
  SCT_TRY(resolve_check(c, method));
  SCT_CHECK(resolved != nullptr, "NULL output");
  SCT_ON_STAGE_OF(c, s);
  Staged st(s);
  st.add(resolved, 8, (size_t)c->t.nw), st.add(tally, 8, 4);
  if (int rc = st.alloc(); rc != SCT_OK) return rc;
  return st.finish(resolve_device(c, method, st.dev<uint64_t>(0), st.dev<uint64_t>(1), s), "molecule resolve");
}

extern "C" int sct_molecules_matrix_resolved(sct_molecules* c, int method, int64_t* d_indptr, int32_t* d_feature,
                                             uint64_t* d_molecules, uint64_t* d_reads, uint64_t* d_collapsed,
                                             uint64_t* d_resolved, uint64_t* d_tally, int64_t room, int64_t* nnz,
                                             void* stream) {
  SCT_TRY(matrix_resolved_check(c, method, d_indptr, d_feature, d_collapsed, room, nnz));
  SCT_ON_DEVICE_OF(c);
  const ResolvedOut rv{d_resolved, d_tally};
  return matrix_device(c, method, d_indptr, d_feature, d_molecules, d_reads, d_collapsed, &rv, room, nnz,
                       sct::as_stream(stream));
}

extern "C" int sct_molecules_matrix_resolved_host(sct_molecules* c, int method, int64_t* indptr, int32_t* feature,
                                                  uint64_t* molecules, uint64_t* reads, uint64_t* collapsed,
                                                  uint64_t* resolved, uint64_t* tally, int64_t room, int64_t* nnz) {
  SCT_TRY(matrix_resolved_check(c, method, indptr, feature, collapsed, room, nnz));
  SCT_ON_STAGE_OF(c, s);
  if (int rc = enter_read(c, s); rc != SCT_OK) return rc;
  const int64_t r = std::min(room, c->size_bound);
  Staged st(s);
  st.add(indptr, 8, (size_t)c->t.nw + 1), st.add(feature, 4, r);
  st.add(molecules, 8, r), st.add(reads, 8, r), st.add(collapsed, 8, r), st.add(resolved, 8, r);
  st.add(tally, 8, 4);
  if (int rc = st.alloc(); rc != SCT_OK) return rc;
  const ResolvedOut rv{st.dev<uint64_t>(5), st.dev<uint64_t>(6)};
  const int rc = matrix_device(c, method, st.dev<int64_t>(0), st.dev<int32_t>(1), st.dev<uint64_t>(2),
                               st.dev<uint64_t>(3), st.dev<uint64_t>(4), &rv, r, nnz, s);
  for (int i = 1; i < 6; ++i) st.cols[i].count = (size_t)*nnz;  // what the matrix wrote of its room
  return st.finish(rc, "molecule matrix");
}

// ---- read groups (include/sctools_hip.h, "read groups"; the status rule and the slot word:
// read_group_status.h)
//
// A snapshot keeps its own copy of the counter's keys and, per slot, what a read that finds the slot
// needs, written at the slot itself: the word (the final UMI with the kept flag) and, if asked, the
// final molecule's reads.  A read costs the probe and one line per column; nothing is chased through
// the image.  Only the lowest ordinal is shared by the reads of a final molecule, so it lives at the
// image's slot, whose number is kept per slot beside it.

namespace {

static_assert(SCT_READ_GROUPED == sct::READ_GROUPED && SCT_READ_NO_BARCODE == sct::READ_NO_BARCODE &&
                  SCT_READ_AMBIGUOUS == sct::READ_AMBIGUOUS && SCT_READ_BAD_UMI == sct::READ_BAD_UMI &&
                  SCT_READ_NO_FEATURE == sct::READ_NO_FEATURE && SCT_READ_ABSENT == sct::READ_ABSENT &&
                  SCT_READ_LOST == sct::READ_LOST && SCT_READ_BAD_INDEX == sct::READ_BAD_INDEX,
              "the header's status numbers are read_group_status.h's");
static_assert(W_NWORDS == sct::READ_NSTATUS, "a snapshot's device words are its eight status tallies");

// sum[image slot] += cnt[s] over the occupied slots s: the reads of every final molecule, at its
// image's slot (sum is zero before; `image` as the resolve pass or the directional labels left it)
__global__ void __launch_bounds__(WG) read_groups_sum_kernel(Set t, int64_t capacity,
                                                             const uint32_t* __restrict__ image,
                                                             u64* __restrict__ sum) {
  for_each_item(capacity, [&](int64_t s, bool in) {
    if (in && t.keys[s] != EMPTY) atomicAdd(&sum[image[s] & kLabelSlot], t.cnt[s]);
  });
}

// The snapshot's columns of every occupied slot s, with p its image's slot (s itself without `image`):
// word[s] = the UMI of keys[p] with the kept flag (p's bit in `kept`; set without a bitmap), and each
// if asked reads[s] = sum[p] (cnt[s] without `sum`: every key its own image) and image_out[s] = p.
__global__ void __launch_bounds__(WG) read_groups_fill_kernel(Set t, int64_t capacity,
                                                              const uint32_t* __restrict__ image,
                                                              const uint32_t* __restrict__ kept,
                                                              const u64* __restrict__ sum, u64* __restrict__ word,
                                                              u64* __restrict__ reads,
                                                              uint32_t* __restrict__ image_out) {
  for_each_item(capacity, [&](int64_t s, bool in) {
    if (!in || t.keys[s] == EMPTY) return;
    const uint32_t p = image ? image[s] & kLabelSlot : (uint32_t)s;
    const bool keeps = kept ? (kept[p >> 5] >> (p & 31)) & 1u : true;
    word[s] = sct::read_group_word(sct::mol_key_umi(t.keys[p], t.umi_bits), keeps);
    if (reads) reads[s] = sum ? sum[p] : t.cnt[s];
    if (image_out) image_out[s] = p;
  });
}

// what the tag kernels read of a snapshot: t.keys is the snapshot's copy, t.words its tallies
struct Groups {
  Set t;
  const u64* word;
  const u64* reads;       // NULL unless READS
  u64* first;             // per image slot, the lowest ordinal of a GROUPED read; NULL unless FIRST
  const uint32_t* image;  // the image's slot of every slot; NULL unless FIRST
};

// Read i of a batch has the ordinal base + i.  TAG_MIN: the GROUPED reads atomicMin their ordinal into
// their final molecule's word and nothing else is written.  TAG_EMIT: the columns asked for and the
// status tallies, summed per wave and added once per wave and status; first[i] says that the word
// holds this read's ordinal, which is final for this batch once every TAG_MIN launch of it is done --
// a later batch's ordinals are all larger.
enum { TAG_EMIT, TAG_MIN };
template <bool FEATURES, int PASS>
__global__ void __launch_bounds__(WG) read_groups_tag_kernel(Groups g, const int32_t* __restrict__ index,
                                                             const int32_t* __restrict__ feature,
                                                             const u64* __restrict__ umi, int64_t n, u64 base,
                                                             u64* __restrict__ final_umi, uint8_t* __restrict__ status,
                                                             u64* __restrict__ reads, uint8_t* __restrict__ first) {
  const Set& t = g.t;
  uint32_t tally[sct::READ_NSTATUS] = {};
  for_each_item(n, [&](int64_t i, bool in) {
    int what = -1;
    if (in) {
      const int32_t v = __builtin_nontemporal_load(&index[i]);
      const int32_t f = FEATURES ? __builtin_nontemporal_load(&feature[i]) : 0;
      const u64 u = __builtin_nontemporal_load(&umi[i]);
      what = sct::read_group_read_status(v, f, t.nw, FEATURES ? t.nf : 0, sct::mol_umi_bad(u, t.kind, t.umi_bits));
      u64 out_umi = u, out_reads = 0, slot = NO_SLOT;
      if (what == sct::READ_LOOKUP) {
        const u64 key = FEATURES ? sct::mol_fkey((uint32_t)v, (uint32_t)f, u, t.feat_bits, t.umi_bits)
                                 : sct::mol_key((uint32_t)v, u, t.umi_bits);
        slot = find(t.keys, t.mask, key);
        const u64 w = slot != NO_SLOT ? g.word[slot] : 0;
        what = sct::read_group_slot_status(slot != NO_SLOT, sct::read_group_word_kept(w));
        if (slot != NO_SLOT) {
          out_umi = sct::read_group_word_umi(w);
          if (PASS == TAG_EMIT && reads) out_reads = g.reads[slot];
        }
      }
      const bool grouped = what == sct::READ_GROUPED;
      if (PASS == TAG_MIN) {
        if (grouped) atomicMin(&g.first[g.image[slot]], base + (u64)i);
      } else {
        __builtin_nontemporal_store(out_umi, &final_umi[i]);
        __builtin_nontemporal_store((uint8_t)what, &status[i]);
        if (reads) __builtin_nontemporal_store(out_reads, &reads[i]);
        if (first)
          __builtin_nontemporal_store((uint8_t)(grouped && g.first[g.image[slot]] == base + (u64)i), &first[i]);
      }
    }
    if (PASS == TAG_EMIT)
      for (int k = 0; k < sct::READ_NSTATUS; ++k) tally[k] += (uint32_t)__popcll(__ballot(what == k));
  });
  if (PASS != TAG_EMIT || (threadIdx.x & 63) != 0) return;
  for (int k = 0; k < sct::READ_NSTATUS; ++k)
    if (tally[k]) atomicAdd(&t.words[k], (u64)tally[k]);
}

}  // namespace

// Host::words are the eight status tallies, Host::total the reads tagged so far (the next ordinal)
struct sct_read_groups : Host {
  sct_read_groups() : Host("read groups") {}
  Groups g{};
  int flags = 0;
  u64 bad_index_seen = 0;  // the BAD_INDEX tally as the last tag call read it
  u64* keys = nullptr;
  u64* word = nullptr;
  u64* reads = nullptr;
  u64* first = nullptr;
  uint32_t* image = nullptr;
};

namespace {

// The columns of the snapshot `g` from mol's table as it stands on `s` (it holds molecules, and its
// size is exact): the method's images by the pass that makes them for resolve, the kept bitmap by the
// resolve pass itself, the final molecules' reads by one sum over the occupied slots.  All scratch
// is stream-ordered pool memory.
int read_groups_build(sct_molecules* c, sct_read_groups* g, int method, hipStream_t s) {
  const bool resolved = (g->flags & SCT_GROUPS_RESOLVED) != 0;
  const bool directional = method == SCT_COLLAPSE_DIRECTIONAL, one_step = method == SCT_COLLAPSE_ONE_STEP;
  const size_t slots8 = (size_t)c->capacity * 8;
  Carve cv;
  const size_t o_labels = directional ? cv.take(DirectionalScratch::bytes(c)) : 0;
  const size_t o_resolve = resolved || one_step ? cv.take(ResolveScratch::bytes(c, method)) : 0;
  const size_t o_sum = g->reads && method != SCT_COLLAPSE_NONE ? cv.take(slots8) : 0;
  sct::StreamBlock blk(s);
  SCT_HIP(blk.alloc(std::max<size_t>(cv.size, 1)));
  const uint32_t* image = nullptr;
  const uint32_t* kept = nullptr;
  if (directional) {
    const DirectionalScratch ds(c, blk.bytes() + o_labels);
    SCT_TRY(directional_labels(c, ds, s));
    image = ds.lab;
  }
  hipError_t e = hipSuccess;
  if (resolved) {
    const ResolveScratch rs(c, blk.bytes() + o_resolve);
    SortedRows<true> sr(c->size_bound, key_bits(c), s);
    SCT_HIP(sr.alloc());
    e = resolve_pass(c, method, sr, rs, image, nullptr, nullptr);
    if (one_step) image = rs.image;
    kept = rs.kept;
  } else if (one_step) {
    // the resolve pass's rows kernel with room for no row: it leaves the parents in rs.image
    const ResolveScratch rs(c, blk.bytes() + o_resolve);
    const bool wave = sct::tune(SCT_TUNE_COLLAPSE_FORM, 1) == 1;
    const auto rows_kernel = wave ? molecules_resolve_rows_kernel<IMAGE_PARENT_WAVE> : molecules_resolve_rows_kernel<IMAGE_PARENT>;
    hipLaunchKernelGGL(rows_kernel, dim3(grid_for(c->capacity, WG)), dim3(WG), 0, s, c->t, c->capacity, nullptr,
                       rs.image, nullptr, &c->t.words[W_CURSOR], (int64_t)0, nullptr, nullptr);
    e = hipGetLastError();
    image = rs.image;
  }
  u64* sum = nullptr;
  if (e == hipSuccess && o_sum) {
    sum = reinterpret_cast<u64*>(blk.bytes() + o_sum);
    e = hipMemsetAsync(sum, 0, slots8, s);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(read_groups_sum_kernel, dim3(grid_for(c->capacity, 1024)), dim3(WG), 0, s, c->t, c->capacity,
                         image, sum);
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(read_groups_fill_kernel, dim3(grid_for(c->capacity, 1024)), dim3(WG), 0, s, c->t, c->capacity,
                       image, kept, sum, g->word, g->reads, g->image);
    e = hipGetLastError();
  }
  if (e != hipSuccess) return sct::fail(SCT_E_HIP, "read groups: %s", hipGetErrorString(e));
  return SCT_OK;
}

int read_groups_check(const sct_read_groups* g, const void* index, const void* feature, const void* umi, int64_t n,
                      const void* final_umi, const void* status, const void* reads, const void* first) {
  SCT_CHECK(n >= 0, "n must be >= 0");
  SCT_CHECK(g != nullptr, "read groups is NULL");
  SCT_CHECK((reads != nullptr) == ((g->flags & SCT_GROUPS_READS) != 0),
            "the reads column is written exactly when the read groups were made with SCT_GROUPS_READS");
  SCT_CHECK((first != nullptr) == ((g->flags & SCT_GROUPS_FIRST) != 0),
            "the first column is written exactly when the read groups were made with SCT_GROUPS_FIRST");
  SCT_CHECK((feature != nullptr) == (g->g.t.nf != 0) || (n == 0 && feature == nullptr),
            g->g.t.nf ? "read groups of a feature counter are tagged with a feature per read"
                      : "the read groups' counter has no features");
  if (n == 0) return SCT_OK;
  SCT_CHECK(index != nullptr && umi != nullptr, "NULL index or umi");
  SCT_CHECK(final_umi != nullptr && status != nullptr, "NULL output");
  return SCT_OK;
}

// n > 0 reads on `s`, on the snapshot's device; *range: the batch held a BAD_INDEX read
int read_groups_tag_device(sct_read_groups* g, const int32_t* d_index, const int32_t* d_feature, const uint64_t* d_umi,
                           int64_t n, uint64_t* d_final_umi, uint8_t* d_status, uint64_t* d_reads, uint8_t* d_first,
                           hipStream_t s, bool* range) {
  if (int rc = enter(g, s); rc != SCT_OK) return rc;
  const dim3 grid(grid_for(n, 4 * WG));
  const u64 base = (u64)g->total;
  const auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(WG), 0, s, g->g, d_index, d_feature, reinterpret_cast<const u64*>(d_umi), n,
                       base, reinterpret_cast<u64*>(d_final_umi), d_status, reinterpret_cast<u64*>(d_reads), d_first);
  };
  if (d_first) {
    d_feature ? launch(read_groups_tag_kernel<true, TAG_MIN>) : launch(read_groups_tag_kernel<false, TAG_MIN>);
    SCT_LAUNCH_CHECK();
  }
  d_feature ? launch(read_groups_tag_kernel<true, TAG_EMIT>) : launch(read_groups_tag_kernel<false, TAG_EMIT>);
  SCT_LAUNCH_CHECK();
  g->total += n;
  SCT_HIP(hipMemcpyAsync(g->h_words, g->words, W_NWORDS * 8, hipMemcpyDeviceToHost, s));
  SCT_HIP(hipStreamSynchronize(s));
  *range = g->h_words[sct::READ_BAD_INDEX] != g->bad_index_seen;
  g->bad_index_seen = g->h_words[sct::READ_BAD_INDEX];
  return leave(g, s);
}

int read_groups_range_error(const sct_read_groups* g) {
  if (g->g.t.nf)
    return sct::fail(SCT_E_RANGE, "index outside [-2, %lld) or feature outside [-2, %lld) (tagged SCT_READ_BAD_INDEX)",
                     (long long)g->g.t.nw, (long long)g->g.t.nf);
  return sct::fail(SCT_E_RANGE, "index outside [-2, %lld) (tagged SCT_READ_BAD_INDEX)", (long long)g->g.t.nw);
}

}  // namespace

extern "C" int sct_read_groups_destroy(sct_read_groups* g) {
  if (!g) return SCT_OK;
  DeviceGuard on_device(g->device);
  close_words(g);
  if (g->keys) (void)hipFree(g->keys);
  if (g->word) (void)hipFree(g->word);
  if (g->reads) (void)hipFree(g->reads);
  if (g->first) (void)hipFree(g->first);
  if (g->image) (void)hipFree(g->image);
  delete g;
  return SCT_OK;
}

extern "C" int sct_read_groups_create(sct_molecules* c, int method, int flags, sct_read_groups** out, void* stream) {
  SCT_CHECK(out != nullptr, "read groups is NULL");
  *out = nullptr;
  SCT_CHECK(c != nullptr, "molecule counter is NULL");
  SCT_TRY(resolve_method_check(method));
  SCT_CHECK((flags & ~(SCT_GROUPS_RESOLVED | SCT_GROUPS_READS | SCT_GROUPS_FIRST)) == 0, "unknown flags 0x%x",
            (unsigned)flags);
  if (flags & SCT_GROUPS_RESOLVED) SCT_TRY(need_feature_counter(c));
  if ((flags & (SCT_GROUPS_RESOLVED | SCT_GROUPS_READS)) || method != SCT_COLLAPSE_NONE) SCT_TRY(need_counted(c));
  SCT_ON_DEVICE_OF(c);
  hipStream_t s = sct::as_stream(stream);
  SCT_TRY(enter_read(c, s));
  auto* g = new sct_read_groups();
  const auto fail_with = [&](int rc) {
    sct_read_groups_destroy(g);
    return rc;
  };
  g->device = c->device;
  g->capacity = c->capacity;
  g->flags = flags;
  const size_t slots8 = (size_t)c->capacity * 8;
  hipError_t e = hipMalloc((void**)&g->keys, slots8);
  if (e == hipSuccess) e = hipMalloc((void**)&g->word, slots8);
  if (e == hipSuccess && (flags & SCT_GROUPS_READS)) e = hipMalloc((void**)&g->reads, slots8);
  if (e == hipSuccess && (flags & SCT_GROUPS_FIRST)) e = hipMalloc((void**)&g->first, slots8);
  if (e == hipSuccess && (flags & SCT_GROUPS_FIRST)) e = hipMalloc((void**)&g->image, slots8 / 2);
  if (e == hipSuccess) e = open_words(g);
  if (e == hipSuccess) e = hipMemsetAsync(g->words, 0, W_NWORDS * 8, s);
  if (e == hipSuccess && g->first) e = hipMemsetAsync(g->first, 0xFF, slots8, s);
  if (e == hipSuccess) e = hipMemcpyAsync(g->keys, c->t.keys, slots8, hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess)
    return fail_with(sct::fail(e == hipErrorOutOfMemory ? SCT_E_NOMEM : SCT_E_HIP, "read groups of %lld slots: %s",
                               (long long)c->capacity, hipGetErrorString(e)));
  g->g.t = c->t;
  g->g.t.keys = g->keys;
  g->g.t.cnt = g->g.t.reads = g->g.t.molecules = nullptr;
  g->g.t.words = g->words;
  g->g.word = g->word, g->g.reads = g->reads, g->g.first = g->first, g->g.image = g->image;
  int rc = c->size_bound > 0 ? read_groups_build(c, g, method, s) : SCT_OK;
  // the counter's arrays are read until here; the snapshot's are written until here
  if (int rl = leave(c, s); rc == SCT_OK) rc = rl;
  if (int rl = leave(g, s); rc == SCT_OK) rc = rl;
  if (rc != SCT_OK) return fail_with(rc);
  *out = g;
  return SCT_OK;
}

extern "C" int sct_read_groups_tag(sct_read_groups* g, const int32_t* d_index, const int32_t* d_feature,
                                   const uint64_t* d_umi, int64_t n, uint64_t* d_final_umi, uint8_t* d_status,
                                   uint64_t* d_reads, uint8_t* d_first, void* stream) {
  SCT_TRY(read_groups_check(g, d_index, d_feature, d_umi, n, d_final_umi, d_status, d_reads, d_first));
  if (n == 0) return SCT_OK;
  SCT_ON_DEVICE_OF(g);
  bool range = false;
  const int rc = read_groups_tag_device(g, d_index, d_feature, d_umi, n, d_final_umi, d_status, d_reads, d_first,
                                        sct::as_stream(stream), &range);
  return rc == SCT_OK && range ? read_groups_range_error(g) : rc;
}

extern "C" int sct_read_groups_tag_host(sct_read_groups* g, const int32_t* index, const int32_t* feature,
                                        const uint64_t* umi, int64_t n, uint64_t* final_umi, uint8_t* status,
                                        uint64_t* reads, uint8_t* first) {
  SCT_TRY(read_groups_check(g, index, feature, umi, n, final_umi, status, reads, first));
  if (n == 0) return SCT_OK;
  SCT_ON_STAGE_OF(g, s);
  // one staged call: the up to four outputs, then the three inputs, which travel one way only
  Staged st(s);
  st.add(final_umi, 8, (size_t)n), st.add(reads, 8, (size_t)n), st.add(status, 1, (size_t)n), st.add(first, 1, (size_t)n);
  st.add(const_cast<uint64_t*>(umi), 8, (size_t)n), st.add(const_cast<int32_t*>(index), 4, (size_t)n);
  st.add(const_cast<int32_t*>(feature), 4, (size_t)n);
  if (int rc = st.alloc(); rc != SCT_OK) return rc;
  for (int i = 4; i < st.n; ++i) {
    const Staged::Column& col = st.cols[i];
    if (col.host && st.blk.ok())
      st.blk.note(hipMemcpyAsync(st.dev<uint8_t>(i), col.host, col.elem * col.count, hipMemcpyHostToDevice, s));
    st.cols[i].count = 0;  // (not copied back)
  }
  bool range = false;
  int rc = SCT_OK;
  if (st.blk.ok())
    rc = read_groups_tag_device(g, st.dev<int32_t>(5), st.dev<int32_t>(6), st.dev<uint64_t>(4), n, st.dev<uint64_t>(0),
                                st.dev<uint8_t>(2), st.dev<uint64_t>(1), st.dev<uint8_t>(3), s, &range);
  rc = st.finish(rc, "read groups tag");
  return rc == SCT_OK && range ? read_groups_range_error(g) : rc;
}

extern "C" int sct_read_groups_info(sct_read_groups* g, int64_t* tagged, uint64_t* tally) {
  SCT_CHECK(g != nullptr, "read groups is NULL");
  if (tally) {
    SCT_ON_STAGE_OF(g, s);
    SCT_TRY(enter(g, s));
    SCT_HIP(hipMemcpyAsync(g->h_words, g->words, W_NWORDS * 8, hipMemcpyDeviceToHost, s));
    SCT_HIP(hipStreamSynchronize(s));
    for (int k = 0; k < W_NWORDS; ++k) tally[k] = g->h_words[k];
  }
  if (tagged) *tagged = g->total;
  return SCT_OK;
}
