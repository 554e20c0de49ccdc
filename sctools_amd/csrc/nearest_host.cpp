// The host-array entry points of the nearest index: each checks its arguments and makes one call.
// Host code only; the plan, the kernels and their launches are in nearest.hip and count.hip.
#include <algorithm>

#include "nearest_host.h"

int sct::nearest_host_batch(sct_nearest_plan* p, const NearestIn& in, const NearestWant& want) {
  if (in.nq == 0) return SCT_OK;
  const bool correct = in.qual != nullptr, tallied = want.tally != nullptr;
  const char* what = correct ? (tallied ? "nearest correct count" : "nearest correct")
                             : (tallied ? "nearest count" : "nearest query");
  const int L = correct ? nearest_plan_positions(p) : 0;
  if (correct) {
    if (int rc = correct_plan_check(p); rc != SCT_OK) return rc;
    SCT_CHECK(in.qual_stride >= L, "qual_stride %lld below the %d positions of the plan", (long long)in.qual_stride, L);
  }
  HostStage* hs = host_stage();
  if (!hs) return SCT_E_HIP;
  hipStream_t s = hs->stream;
  const int64_t nq = in.nq, nw = nearest_plan_size(p);
  const NearestLayout lay(nq, L, tallied, nw);
  if (lay.tail_words)  // the tail comes home through the stage's page-locked buffer
    if (int rc = stage_reserve(hs, lay.tail_words * 8, 0); rc != SCT_OK) return rc;
  PoolBlock blk(s);
  if (int rc = blk.alloc(lay.total); rc != SCT_OK) return rc;
  uint8_t* b = blk.bytes();
  const uint64_t* d_q = reinterpret_cast<const uint64_t*>(b);
  int32_t* d_index = reinterpret_cast<int32_t*>(b + lay.index);
  uint64_t* d_tail = reinterpret_cast<uint64_t*>(b + lay.tail);
  const uint64_t* h_tail = reinterpret_cast<const uint64_t*>(hs->pinned);
  blk.note(hipMemcpyAsync(b, in.queries, (size_t)nq * 8, hipMemcpyHostToDevice, s));
  if (correct && blk.ok())
    blk.note(in.qual_stride == L ? hipMemcpyAsync(b + lay.qual, in.qual, (size_t)nq * L, hipMemcpyHostToDevice, s)
                                 : hipMemcpy2DAsync(b + lay.qual, (size_t)L, in.qual, (size_t)in.qual_stride,
                                                    (size_t)L, (size_t)nq, hipMemcpyHostToDevice, s));
  if (lay.tail_words && blk.ok()) blk.note(hipMemsetAsync(d_tail, 0, lay.tail_words * 8, s));
  int rc = SCT_OK;
  if (blk.ok()) {
    rc = correct ? sct_nearest_correct(p, d_q, b + lay.qual, L, nq, d_index, b + lay.dist, d_tail + lay.stats, s)
                 : sct_nearest_query(p, d_q, nq, d_index, b + lay.dist, s);
    if (rc == SCT_OK && tallied)
      rc = tally_launch(d_index, nq, nw, d_tail + lay.counts, d_tail + lay.tally, d_tail + lay.err, s);
    if (rc == SCT_OK && !tallied) {
      blk.note(hipMemcpyAsync(want.index, d_index, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
      if (blk.ok()) blk.note(hipMemcpyAsync(want.dist, b + lay.dist, (size_t)nq, hipMemcpyDeviceToHost, s));
    }
    if (rc == SCT_OK && lay.tail_words && blk.ok())
      blk.note(hipMemcpyAsync(hs->pinned, d_tail, lay.tail_words * 8, hipMemcpyDeviceToHost, s));
  }
  rc = blk.finish(rc, what);
  if (rc != SCT_OK) return rc;
  if (tallied) {
    if (h_tail[lay.err]) return fail(SCT_E_RANGE, "nearest index outside [-2, %lld)", (long long)nw);
    for (int64_t j = 0; j < nw; ++j) want.counts[j] += h_tail[lay.counts + j];
    want.tally[0] += h_tail[lay.tally];
    want.tally[1] += h_tail[lay.tally + 1];
  }
  if (correct && want.stats) {
    want.stats[0] += h_tail[lay.stats];
    want.stats[1] += h_tail[lay.stats + 1];
  }
  return SCT_OK;
}

extern "C" int sct_nearest_query_host(sct_nearest_plan* p, const uint64_t* queries, int64_t nq, int32_t* index,
                                      uint8_t* dist) {
  SCT_CHECK(p != nullptr, "plan is NULL");
  SCT_CHECK(nq >= 0 && (nq == 0 || (queries && index && dist)), "bad arguments");
  return sct::nearest_host_batch(p, {queries, nullptr, 0, nq}, {index, dist, nullptr, nullptr, nullptr});
}

extern "C" int sct_nearest_count_host(sct_nearest_plan* p, const uint64_t* queries, int64_t nq, uint64_t* counts,
                                      uint64_t* tally) {
  SCT_CHECK(nq >= 0, "nq must be >= 0");
  SCT_CHECK(p != nullptr, "plan is NULL");
  SCT_CHECK(tally != nullptr && (sct::nearest_plan_size(p) == 0 || counts != nullptr), "NULL counts");
  SCT_CHECK(nq == 0 || queries != nullptr, "NULL queries");
  return sct::nearest_host_batch(p, {queries, nullptr, 0, nq}, {nullptr, nullptr, counts, tally, nullptr});
}

extern "C" int sct_nearest_correct_host(sct_nearest_plan* p, const uint64_t* queries, const uint8_t* qual,
                                        int64_t qual_stride, int64_t nq, int32_t* index, uint8_t* dist,
                                        uint64_t* stats) {
  if (int rc = sct::correct_plan_check(p); rc != SCT_OK) return rc;
  SCT_CHECK(nq >= 0 && (nq == 0 || (queries && qual && index && dist)), "bad arguments");
  return sct::nearest_host_batch(p, {queries, qual, qual_stride, nq}, {index, dist, nullptr, nullptr, stats});
}

// sct_nearest_count_host with sct_nearest_correct in place of the query: the final indices feed the
// same tally, and only the counts, the two tallies and the two statistics come back.
extern "C" int sct_nearest_correct_count_host(sct_nearest_plan* p, const uint64_t* queries, const uint8_t* qual,
                                              int64_t qual_stride, int64_t nq, uint64_t* counts, uint64_t* tally,
                                              uint64_t* stats) {
  SCT_CHECK(nq >= 0, "nq must be >= 0");
  SCT_CHECK(p != nullptr, "plan is NULL");
  SCT_CHECK(tally != nullptr && (sct::nearest_plan_size(p) == 0 || counts != nullptr), "NULL counts");
  if (sct::nearest_plan_positions(p) == 0) return sct::correct_plan_check(p);  // not a half-key plan: says why
  SCT_CHECK(nq == 0 || (queries != nullptr && qual != nullptr), "NULL queries or qualities");
  return sct::nearest_host_batch(p, {queries, qual, qual_stride, nq}, {nullptr, nullptr, counts, tally, stats});
}

extern "C" int sct_nearest_plan_create_host(int kind, const uint64_t* whitelist, int64_t nw, int code_bits, int max_d,
                                            sct_nearest_plan** out) {
  SCT_CHECK(out != nullptr, "plan is NULL");
  SCT_CHECK(nw >= 0 && (nw == 0 || whitelist), "bad whitelist");
  // the whitelist through the library's stream-ordered pool on the thread's stream (no per-call
  // hipMalloc / hipFree: a stream of batches builds its index once, but the flows that build
  // one per file set pay it each time); it goes back ordered after the build's reads of it
  sct::HostStage* hs = sct::host_stage();
  if (!hs) return SCT_E_HIP;
  hipStream_t s = hs->stream;
  sct::PoolBlock dw(s);
  if (int rc = dw.alloc(std::max<size_t>((size_t)nw * 8, 8)); rc != SCT_OK) return rc;
  if (nw) dw.note(hipMemcpyAsync(dw.p, whitelist, (size_t)nw * 8, hipMemcpyHostToDevice, s));
  const int rc = dw.ok() ? sct_nearest_plan_create(kind, (const uint64_t*)dw.p, nw, code_bits, max_d, s, out)
                         : sct::fail(SCT_E_HIP, "whitelist copy: %s", hipGetErrorString(dw.e));
  return dw.finish(rc, "nearest plan");
}

extern "C" int sct_nearest_plan_set_posterior_host(sct_nearest_plan* p, const uint32_t* prior, const uint32_t* qweight,
                                                   int num, int den) {
  if (int rc = sct::correct_plan_check(p); rc != SCT_OK) return rc;
  sct::HostStage* hs = sct::host_stage();
  if (!hs) return SCT_E_HIP;
  hipStream_t s = hs->stream;
  if (!prior) return sct_nearest_plan_set_posterior(p, nullptr, qweight, num, den, s);
  const size_t bytes = (size_t)sct::nearest_plan_size(p) * 4;
  sct::PoolBlock dp(s);
  if (int rc = dp.alloc(bytes); rc != SCT_OK) return rc;
  dp.note(hipMemcpyAsync(dp.p, prior, bytes, hipMemcpyHostToDevice, s));
  const int rc = dp.ok() ? sct_nearest_plan_set_posterior(p, (const uint32_t*)dp.p, qweight, num, den, s)
                         : sct::fail(SCT_E_HIP, "prior copy: %s", hipGetErrorString(dp.e));
  return dp.finish(rc, "set posterior");
}

extern "C" int sct_nearest_host(int kind, const uint64_t* whitelist, int64_t nw, const uint64_t* queries,
                                int64_t nq, int code_bits, int max_d, int32_t* index, uint8_t* dist) {
  SCT_CHECK(nw >= 0 && nq >= 0, "bad sizes");
  // a host-whitelist plan and one host query pass; the results are read back before the plan goes
  sct_nearest_plan* plan = nullptr;
  int rc = sct_nearest_plan_create_host(kind, whitelist, nw, code_bits, max_d, &plan);
  if (rc != SCT_OK) return rc;
  rc = sct_nearest_query_host(plan, queries, nq, index, dist);
  sct_nearest_plan_destroy(plan);
  return rc;
}
