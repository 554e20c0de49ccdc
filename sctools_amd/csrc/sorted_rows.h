// The occupied slots of an open_table.h table as rows sorted by a 64-bit word: the stage under every
// fetch and under the count matrix.  A counter's own compaction kernel writes one word per occupied
// slot (the molecule counter: the key; the barcode counter: the first position) and, if asked, the
// uint32 slot number beside it, in any order; a radix sort of the words' low `end_bit` bits fixes
// the order.  One pool block holds the two sides of the sort, the sort's scratch and whatever
// pieces the caller takes after them.
#pragma once

#include <hipcub/hipcub.hpp>

#include "open_table.h"

namespace sct {
namespace open_table {

// SLOTS: SortPairs of (word, slot); else SortKeys of the words alone
template <bool SLOTS>
struct SortedRows {
  const int64_t rows;  // > 0
  const int end_bit;
  const hipStream_t s;
  size_t sort_bytes = 0;
  Carve cv;
  size_t o_in, o_out, o_slot_in = 0, o_slot_out = 0, o_tmp;
  StreamBlock blk;  // given back on `s` when the rows leave scope

  // plans the block; tmp_at_least: the caller's other uses of the sort's scratch (after the sort)
  SortedRows(int64_t rows_, int end_bit_, hipStream_t s_, size_t tmp_at_least = 0)
      : rows(rows_), end_bit(end_bit_), s(s_), blk(s_) {
    (void)run(nullptr);
    o_in = cv.take((size_t)rows * 8), o_out = cv.take((size_t)rows * 8);
    if (SLOTS) o_slot_in = cv.take((size_t)rows * 4), o_slot_out = cv.take((size_t)rows * 4);
    o_tmp = cv.take(std::max(sort_bytes, tmp_at_least));
  }
  // a piece of the caller's in the same block (before alloc): its offset, for at()
  size_t take(size_t bytes) { return cv.take(bytes); }
  hipError_t alloc() { return blk.alloc(cv.size); }
  template <class T>
  T* at(size_t offset) const {
    return reinterpret_cast<T*>(blk.bytes() + offset);
  }
  // cursor = 0, compact(word_in, slot_in or NULL) enqueues the counter's compaction, then the sort
  template <class Compact>
  hipError_t sort(u64* cursor, Compact compact) {
    const hipError_t e = zero_cursor(cursor, s);
    if (e != hipSuccess) return e;
    compact(at<u64>(o_in), SLOTS ? at<uint32_t>(o_slot_in) : nullptr);
    return run(at<void>(o_tmp));
  }
  // the sorted rows, and the scratch, which is free again once the sort is enqueued
  const u64* word() const { return at<u64>(o_out); }
  const uint32_t* slot() const { return SLOTS ? at<uint32_t>(o_slot_out) : nullptr; }
  void* tmp() const { return at<void>(o_tmp); }

 private:
  // tmp == NULL sizes the sort (no pointer is read)
  hipError_t run(void* tmp) {
    const u64* in = tmp ? at<u64>(o_in) : nullptr;
    u64* out = tmp ? at<u64>(o_out) : nullptr;
    if constexpr (SLOTS)
      return hipcub::DeviceRadixSort::SortPairs(tmp, sort_bytes, in, out, tmp ? at<const uint32_t>(o_slot_in) : nullptr,
                                                tmp ? at<uint32_t>(o_slot_out) : nullptr, (int)rows, 0, end_bit, s);
    else
      return hipcub::DeviceRadixSort::SortKeys(tmp, sort_bytes, in, out, (int)rows, 0, end_bit, s);
  }
};

}  // namespace open_table
}  // namespace sct
