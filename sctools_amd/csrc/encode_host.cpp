// The host-array entry points of the encoders: each checks its arguments, tries the resident
// scalar server (scalar_server.hip) for a small call, and else runs the device-pointer entry point
// of encode.hip on the thread's host stage.  Host code only.
//
// Every *_host call runs on the thread's host stage (sct::HostStage): small calls (the
// drop-in's scalar methods are batches of one) read their inputs from and write their
// outputs to the page-locked buffer directly (zero-copy: one launch and one stream sync,
// no allocation), larger ones pack inputs / outputs into one H2D and one D2H copy through
// the stage's device buffer, and only calls above kStageBytes allocate per call.
#include <string.h>

#include <algorithm>

#include "sct_common.h"
#include "encode_records.h"
#include "host_pipeline.h"
#include "scalar_server.h"

namespace {
using sct::In;
using sct::Out;

// launch(ptrs, stream): ptrs = device-visible inputs then outputs (nullptr for a null host
// pointer).  zero_copy = false for kernels that update outputs atomically (PCIe atomics on
// host memory are not assumed).
template <int NI, int NO, class F>
int host_call(const In (&ins)[NI], const Out (&outs)[NO], bool zero_copy, F&& launch) {
  constexpr int N = NI + NO;
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  size_t off[N], total = 0;
  for (int k = 0; k < NI; ++k) {
    off[k] = total;
    total += al(ins[k].p ? ins[k].bytes : 0);
  }
  const size_t in_total = total;
  for (int k = 0; k < NO; ++k) {
    off[NI + k] = total;
    total += al(outs[k].p ? outs[k].bytes : 0);
  }
  sct::HostStage* st = sct::host_stage();
  if (!st) return SCT_E_HIP;
  void* ptr[N];
  if (zero_copy && total <= sct::kZeroCopyBytes) {
    SCT_TRY(sct::stage_reserve(st, total, 0));
    for (int k = 0; k < NI; ++k) {
      if (ins[k].p && ins[k].bytes) memcpy(st->pinned + off[k], ins[k].p, ins[k].bytes);
      ptr[k] = ins[k].p ? st->pinned_dev + off[k] : nullptr;
    }
    for (int k = 0; k < NO; ++k) ptr[NI + k] = outs[k].p ? st->pinned_dev + off[NI + k] : nullptr;
    SCT_TRY(launch(ptr, st->stream));
    // a few-microsecond kernel: poll instead of a blocking sync (saves the wake-up)
    hipError_t q;
    while ((q = hipStreamQuery(st->stream)) == hipErrorNotReady) {
    }
    SCT_HIP(q);
    for (int k = 0; k < NO; ++k)
      if (outs[k].p && outs[k].bytes) memcpy(outs[k].p, st->pinned + off[NI + k], outs[k].bytes);
    return SCT_OK;
  }
  if (total <= sct::kStageBytes) {
    SCT_TRY(sct::stage_reserve(st, total, total));
    for (int k = 0; k < NI; ++k) {
      if (ins[k].p && ins[k].bytes) memcpy(st->pinned + off[k], ins[k].p, ins[k].bytes);
      ptr[k] = ins[k].p ? st->dev + off[k] : nullptr;
    }
    for (int k = 0; k < NO; ++k) ptr[NI + k] = outs[k].p ? st->dev + off[NI + k] : nullptr;
    if (in_total) SCT_HIP(hipMemcpyAsync(st->dev, st->pinned, in_total, hipMemcpyHostToDevice, st->stream));
    SCT_TRY(launch(ptr, st->stream));
    if (total > in_total)
      SCT_HIP(hipMemcpyAsync(st->pinned + in_total, st->dev + in_total, total - in_total, hipMemcpyDeviceToHost,
                             st->stream));
    SCT_HIP(hipStreamSynchronize(st->stream));
    for (int k = 0; k < NO; ++k)
      if (outs[k].p && outs[k].bytes) memcpy(outs[k].p, st->pinned + off[NI + k], outs[k].bytes);
    return SCT_OK;
  }
  sct::DevBuf buf[N];
  for (int k = 0; k < NI; ++k) {
    ptr[k] = nullptr;
    if (!ins[k].p) continue;
    SCT_HIP(buf[k].alloc(ins[k].bytes));
    if (ins[k].bytes)
      SCT_HIP(hipMemcpyAsync(buf[k].p, ins[k].p, ins[k].bytes, hipMemcpyHostToDevice, st->stream));
    ptr[k] = buf[k].p;
  }
  for (int k = 0; k < NO; ++k) {
    ptr[NI + k] = nullptr;
    if (!outs[k].p) continue;
    SCT_HIP(buf[NI + k].alloc(outs[k].bytes));
    ptr[NI + k] = buf[NI + k].p;
  }
  SCT_TRY(launch(ptr, st->stream));
  for (int k = 0; k < NO; ++k)
    if (outs[k].p && outs[k].bytes)
      SCT_HIP(hipMemcpyAsync(outs[k].p, buf[NI + k].p, outs[k].bytes, hipMemcpyDeviceToHost, st->stream));
  SCT_HIP(hipStreamSynchronize(st->stream));
  return SCT_OK;
}

// The one chunked pipeline: the large element-wise calls (the *_array forms on host arrays) and the
// encode stream.  n items, item r of input k at ins[k].p + r * ins[k].bytes (bytes = PER ITEM
// here), likewise the outputs (a null output is skipped).  Chunks of items flow through three
// device blocks on the thread's three pipeline streams, so one chunk's H2D copy, another's kernel
// and a third's D2H copy overlap: the call runs at the PCIe rate of its larger direction.  Each
// caller array the runtime already page-locks (sct_host_pinned: the pool arrays the drop-in
// returns, hipHostMalloc, torch pin_memory, the caller's own hipHostRegister) is copied by DMA in
// place; each pageable one through the thread's pinned stage, filled and emptied by par_memcpy
// while the other stages' copies and kernels run.  The library never page-locks caller memory
// itself (registering and unregistering ranges the runtime may also lock for its own pageable
// copies is not something to do behind the caller's back).  launch(ptrs, m, stream) runs the kernel
// on m items at the device pointers.  stream_chunk < 0: the element-wise chunk size
// (sct::items_chunk); else the stream's (sct::stream_chunk) for this `chunk` argument.
constexpr size_t kStreamMinBytes = (size_t)8 << 20;  // below: one staged round trip (host_call)
constexpr int64_t kItemsChunk = -1;

template <int NI, int NO, class F>
int host_items(int64_t n, int64_t stream_chunk, const In (&ins)[NI], const Out (&outs)[NO], F&& launch) {
  constexpr int N = NI + NO, NSTAGE = sct::kPipeStages;
  size_t item[N], per = 0;
  bool staged[N], any_staged = false;
  for (int k = 0; k < N; ++k) {
    const void* p = k < NI ? ins[k].p : outs[k - NI].p;
    item[k] = !p ? 0 : (k < NI ? ins[k].bytes : outs[k - NI].bytes);
    per += item[k];
    staged[k] = p && !sct::host_range_pinned(p, (size_t)n * item[k]);
    any_staged |= staged[k];
  }
  const int64_t chunk = stream_chunk < 0 ? sct::items_chunk(n, per) : sct::stream_chunk(n, stream_chunk, any_staged);
  const sct::StageLayout<N> lay(chunk, item, staged);
  sct::HostStage* hs = sct::host_stage();
  if (!hs) return SCT_E_HIP;
  if (lay.htot) SCT_TRY(sct::stage_reserve(hs, NSTAGE * lay.htot, 0));
  static_assert(NSTAGE == 3, "HostStage::pipe holds three streams");
  for (int k = 0; k < NSTAGE; ++k)  // the thread's pipeline streams (kept across calls)
    if (!hs->pipe[k]) SCT_HIP(hipStreamCreateWithFlags(&hs->pipe[k], hipStreamNonBlocking));
  hipStream_t* st = hs->pipe;
  struct Streams {
    hipStream_t* s;
    ~Streams() {  // (any return leaves nothing in flight on the caller's arrays, the stage or the blocks)
      for (int k = 0; k < NSTAGE; ++k) (void)hipStreamSynchronize(s[k]);
    }
  } guard{st};
  // one device block per stage from the library's stream-ordered pool, freed on its stage's stream
  // before the streams are waited for (declared after the guard).  All three frees go out before
  // the first wait: sct::PoolBlock's free-and-wait per block, one after the other, cost a
  // 3.3M-record stream 0.5 ms of its 1.5 (profiles/ab_host_pipeline_r11.jsonl, "variant": "poolblock")
  struct Blocks {
    void* p[NSTAGE] = {};
    hipStream_t* s;
    ~Blocks() {
      for (int k = 0; k < NSTAGE; ++k) sct::pool_free(p[k], s[k]);
    }
  } blk{{}, st};
  for (int k = 0; k < NSTAGE; ++k) SCT_HIP(sct::pool_alloc(&blk.p[k], lay.dtot, st[k]));
  auto hstage = [&](int k, int a) { return hs->pinned + (size_t)k * lay.htot + lay.hoff[a]; };
  struct {
    int64_t r0, m;
  } pend[NSTAGE] = {};
  auto drain = [&](int k) -> int {  // wait for stage k's chunk; pageable outputs copied out
    if (pend[k].m == 0) return SCT_OK;
    SCT_HIP(hipStreamSynchronize(st[k]));
    for (int o = 0; o < NO; ++o)
      if (staged[NI + o])
        sct::par_memcpy(static_cast<uint8_t*>(outs[o].p) + (size_t)pend[k].r0 * outs[o].bytes, hstage(k, NI + o),
                        (size_t)pend[k].m * outs[o].bytes);
    pend[k].m = 0;
    return SCT_OK;
  };
  int64_t c = 0;
  for (int64_t r0 = 0; r0 < n; r0 += chunk, ++c) {
    const int k = (int)(c % NSTAGE);  // stage k's previous chunk is ordered before on st[k]
    const int64_t m = std::min<int64_t>(chunk, n - r0);
    // stage k's pinned buffers are about to be refilled (device blocks and DMA in place are
    // ordered by the stream: no host wait when nothing is staged)
    if (any_staged) SCT_TRY(drain(k));
    void* ptr[N];
    uint8_t* dev = static_cast<uint8_t*>(blk.p[k]);
    for (int a = 0; a < NI; ++a) {
      const uint8_t* src = static_cast<const uint8_t*>(ins[a].p) + (size_t)r0 * ins[a].bytes;
      const size_t b = (size_t)m * ins[a].bytes;
      if (staged[a]) {
        sct::par_memcpy(hstage(k, a), src, b);
        src = hstage(k, a);
      }
      SCT_HIP(hipMemcpyAsync(dev + lay.doff[a], src, b, hipMemcpyHostToDevice, st[k]));
      ptr[a] = dev + lay.doff[a];
    }
    for (int o = 0; o < NO; ++o) ptr[NI + o] = outs[o].p ? dev + lay.doff[NI + o] : nullptr;
    SCT_TRY(launch(ptr, m, st[k]));
    for (int o = 0; o < NO; ++o) {
      if (!outs[o].p) continue;
      uint8_t* dst = staged[NI + o] ? hstage(k, NI + o) : static_cast<uint8_t*>(outs[o].p) + (size_t)r0 * outs[o].bytes;
      SCT_HIP(hipMemcpyAsync(dst, dev + lay.doff[NI + o], (size_t)m * outs[o].bytes, hipMemcpyDeviceToHost, st[k]));
    }
    pend[k] = {r0, m};
  }
  for (int k = 0; k < NSTAGE; ++k) SCT_TRY(drain(k));
  return SCT_OK;
}

// total bytes of an element-wise call
template <int NI, int NO>
size_t items_bytes(int64_t n, const In (&ins)[NI], const Out (&outs)[NO]) {
  size_t per = 0;
  for (int k = 0; k < NI; ++k) per += ins[k].bytes;
  for (int k = 0; k < NO; ++k) per += outs[k].p ? outs[k].bytes : 0;
  return (size_t)n * per;
}
}  // namespace

extern "C" int sct_encode_host(int kind, const uint8_t* seqs, int64_t n, int64_t stride, int L,
                               uint64_t* codes, uint8_t* gc, uint8_t* flags) {
  SCT_CHECK(kind == 2 || kind == 3, "kind must be 2 or 3");
  SCT_CHECK(n >= 0 && L >= 0 && stride >= L, "bad n/L/stride");
  if (n == 0) return SCT_OK;
  const int words = words_for(kind, L);
  const In ins[1] = {{seqs, (size_t)((n - 1) * stride + L)}};
  const Out outs[3] = {{codes, (size_t)n * words * 8}, {gc, (size_t)n}, {flags, (size_t)n}};
  if (codes && (L == 0 || seqs) && (gc == nullptr || L <= 255)) {
    const int rc = sct::srv_call(sct::OP_ENCODE, kind, n, words, L, stride, 0, ins, 1, outs, 3);
    if (rc != 1) return rc;
  }
  return host_call(ins, outs, true, [&](void** p, hipStream_t s) {
    return sct_encode(kind, (const uint8_t*)p[0], n, stride, L, (uint64_t*)p[1], (uint8_t*)p[2], (uint8_t*)p[3], s);
  });
}

extern "C" int sct_base_frequency_host(const uint64_t* codes, int64_t n, int L, uint64_t* out) {
  SCT_CHECK(n >= 0 && L >= 0 && L <= 1024, "bad n/L");
  if (L == 0) return SCT_OK;
  return host_call<1, 1>({{codes, (size_t)n * 8}}, {{out, (size_t)L * 4 * 8}}, false, [&](void** p, hipStream_t s) {
    return sct_base_frequency((const uint64_t*)p[0], n, L, (uint64_t*)p[1], s);
  });
}

// Host-resident stream (config 5): records live in host memory and flow through host_items
// (PCIe-bound: L + 10 bytes per read cross the link).
extern "C" int sct_encode_stream_host(int kind, const uint8_t* seqs, int64_t n, int L,
                                      uint64_t* codes, uint8_t* gc, uint8_t* flags,
                                      int64_t chunk) {
  SCT_CHECK(kind == 2 || kind == 3, "kind must be 2 or 3");
  SCT_CHECK(n >= 0 && L >= 1 && words_for(kind, L) == 1, "stream encode needs 1 <= L and one limb");
  SCT_CHECK(gc != nullptr && flags != nullptr && codes != nullptr && seqs != nullptr, "NULL pointer");
  if (n == 0) return SCT_OK;
  const In ii[1] = {{seqs, (size_t)L}};
  const Out oo[3] = {{codes, 8}, {gc, 1}, {flags, 1}};
  return host_items(n, std::max<int64_t>(chunk, 0), ii, oo, [&](void** p, int64_t m, hipStream_t s) {
    return sct_encode(kind, (const uint8_t*)p[0], m, L, L, (uint64_t*)p[1], (uint8_t*)p[2], (uint8_t*)p[3], s);
  });
}

extern "C" int sct_decode2_host(const uint64_t* codes, int64_t n, int words, int L, uint8_t* out) {
  SCT_CHECK(n >= 0 && words >= 1 && L >= 0, "bad n/words/L");
  if (n == 0 || L == 0) return SCT_OK;
  const In ins[1] = {{codes, (size_t)n * words * 8}};
  const Out outs[1] = {{out, (size_t)n * L}};
  if (codes && out) {
    const int rc = sct::srv_call(sct::OP_DECODE2, 2, n, words, L, 0, 0, ins, 1, outs, 1);
    if (rc != 1) return rc;
  }
  const In ii[1] = {{codes, (size_t)words * 8}};
  const Out oo[1] = {{out, (size_t)L}};
  if (codes && out && items_bytes(n, ii, oo) >= kStreamMinBytes)
    return host_items(n, kItemsChunk, ii, oo, [&](void** p, int64_t m, hipStream_t s) {
      return sct_decode2((const uint64_t*)p[0], m, words, L, (uint8_t*)p[1], s);
    });
  return host_call(ins, outs, true, [&](void** p, hipStream_t s) {
    return sct_decode2((const uint64_t*)p[0], n, words, L, (uint8_t*)p[1], s);
  });
}

extern "C" int sct_decode3_host(const uint64_t* codes, int64_t n, int words, int maxlen,
                                uint8_t* out, int32_t* lengths, int32_t* bad) {
  SCT_CHECK(n >= 0 && words >= 1, "bad n/words");
  if (n == 0) return SCT_OK;
  const In ins[1] = {{codes, (size_t)n * words * 8}};
  const Out outs[3] = {{out, (size_t)n * maxlen}, {lengths, (size_t)n * 4}, {bad, (size_t)n * 4}};
  if (codes && out && lengths && bad && maxlen >= (64 * words + 2) / 3) {
    const int rc = sct::srv_call(sct::OP_DECODE3, 3, n, words, 0, 0, maxlen, ins, 1, outs, 3);
    if (rc != 1) return rc;
  }
  const In ii[1] = {{codes, (size_t)words * 8}};
  const Out oo[3] = {{out, (size_t)maxlen}, {lengths, 4}, {bad, 4}};
  if (codes && out && lengths && bad && items_bytes(n, ii, oo) >= kStreamMinBytes)
    return host_items(n, kItemsChunk, ii, oo, [&](void** p, int64_t m, hipStream_t s) {
      return sct_decode3((const uint64_t*)p[0], m, words, maxlen, (uint8_t*)p[1], (int32_t*)p[2], (int32_t*)p[3], s);
    });
  return host_call(ins, outs, true, [&](void** p, hipStream_t s) {
    return sct_decode3((const uint64_t*)p[0], n, words, maxlen, (uint8_t*)p[1], (int32_t*)p[2], (int32_t*)p[3], s);
  });
}

extern "C" int sct_gc_content_host(int kind, const uint64_t* codes, int64_t n, int words, int L,
                                   int32_t* out) {
  SCT_CHECK(n >= 0 && words >= 1, "bad n/words");
  if (n == 0) return SCT_OK;
  const In ins[1] = {{codes, (size_t)n * words * 8}};
  const Out outs[1] = {{out, (size_t)n * 4}};
  if ((kind == 2 || kind == 3) && L >= 0 && codes && out) {
    const int rc = sct::srv_call(sct::OP_GC, kind, n, words, L, 0, 0, ins, 1, outs, 1);
    if (rc != 1) return rc;
  }
  const In ii[1] = {{codes, (size_t)words * 8}};
  const Out oo[1] = {{out, 4}};
  if (codes && out && items_bytes(n, ii, oo) >= kStreamMinBytes)
    return host_items(n, kItemsChunk, ii, oo, [&](void** p, int64_t m, hipStream_t s) {
      return sct_gc_content(kind, (const uint64_t*)p[0], m, words, L, (int32_t*)p[1], s);
    });
  return host_call(ins, outs, true, [&](void** p, hipStream_t s) {
    return sct_gc_content(kind, (const uint64_t*)p[0], n, words, L, (int32_t*)p[1], s);
  });
}

extern "C" int sct_hamming_pairs_host(int kind, const uint64_t* a, const uint64_t* b, int64_t n,
                                      int words, int32_t* out) {
  SCT_CHECK(n >= 0 && words >= 1, "bad n/words");
  if (n == 0) return SCT_OK;
  const In ins[2] = {{a, (size_t)n * words * 8}, {b, (size_t)n * words * 8}};
  const Out outs[1] = {{out, (size_t)n * 4}};
  if ((kind == 2 || kind == 3) && a && b && out) {
    const int rc = sct::srv_call(sct::OP_HAMMING, kind, n, words, 0, 0, 0, ins, 2, outs, 1);
    if (rc != 1) return rc;
  }
  const In ii[2] = {{a, (size_t)words * 8}, {b, (size_t)words * 8}};
  const Out oo[1] = {{out, 4}};
  if (a && b && out && items_bytes(n, ii, oo) >= kStreamMinBytes)
    return host_items(n, kItemsChunk, ii, oo, [&](void** p, int64_t m, hipStream_t s) {
      return sct_hamming_pairs(kind, (const uint64_t*)p[0], (const uint64_t*)p[1], m, words, (int32_t*)p[2], s);
    });
  return host_call(ins, outs, true, [&](void** p, hipStream_t s) {
    return sct_hamming_pairs(kind, (const uint64_t*)p[0], (const uint64_t*)p[1], n, words, (int32_t*)p[2], s);
  });
}
