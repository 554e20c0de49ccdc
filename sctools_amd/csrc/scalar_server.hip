// Resident scalar server.
// A scalar drop-in call (TwoBit.encode, hamming_distance, decode, gc_content: a batch of
// one) costs a kernel launch and its completion signal, ~15 us, while the work is a few
// hundred instructions.  Instead, the first such call of a host thread on a device launches
// one 64-lane server kernel that polls a page-locked, host-coherent mailbox over PCIe:
// the host writes the request (opcode, sizes, the packed inputs) and then its sequence
// number, all in one 64-B line the wave polls (larger payloads continue past it); the wave
// runs the same per-record device functions as the batch kernels (one record per lane,
// n <= 64) and answers with one checksummed 64-B response line (SrvMailbox::resp) that
// carries the sequence number, the status and small outputs.  The wave exits after
// idle_ticks of its wall clock without a
// request, on the mailbox's stop word, or never while a request is pending; it always
// writes its launch id to exit_gen last, so the host tells "exited" from "slow" without a
// HIP call, and relaunches (the pending request is served first) when it finds its
// request unanswered and the server gone.
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <vector>

#include "sct_common.h"
#include "encode_common.h"
#include "encode_records.h"
#include "scalar_server.h"

namespace {
using sct::OP_ENCODE;
using sct::OP_DECODE2;
using sct::OP_DECODE3;
using sct::OP_GC;
using sct::OP_HAMMING;
constexpr int kSrvIn = 1024, kSrvOut = 1024, kSrvMaxN = 64;

constexpr int kSrvInline = 28;  // payload bytes that ride in the request line itself
#ifndef SCT_SRV_COPIES
#define SCT_SRV_COPIES 4  // copies of the request line, one poll in flight on each
#endif
constexpr int kSrvCopies = SCT_SRV_COPIES;
static_assert(kSrvCopies >= 1 && kSrvCopies <= 8, "copies of the request line");

// One request line of 64 B: req[0] = seq (written last), req[1..7] = the packed fields,
// req[8..14] = the first 28 payload bytes, req[15] = line_check(req[0..14]); payload bytes
// 28.. follow in `more`.  The host writes the line kSrvCopies times (req, req_copy[..]) and the
// wave keeps one 64-B load in flight on each copy, so a scalar call (payload <= 28 B: a pair of
// one-limb codes, a 28-base record) is seen a fraction of a PCIe round trip after it lands
// (two loads in flight on the SAME line were slower than one: tools/scalar_floor_probe.hip).
// Nothing guarantees that the 16 dwords of one poll are one
// snapshot, so the wave takes a sequence number only when it is newer than the last served
// one (a copy not yet rewritten still shows the previous request) and the check word matches:
// a line mixing this request's seq with the previous request's fields is only polled again.
struct SrvMailbox {
  alignas(64) uint32_t req[16];
  uint32_t more[(kSrvIn - kSrvInline) / 4];
  // the other copies of the request line (dwords 0..15 of each row), 256 B apart
  alignas(256) uint32_t req_copy[kSrvCopies > 1 ? kSrvCopies - 1 : 1][64];
  // control (host)
  alignas(64) uint32_t stop;
  // response line (device), written by one 16-lane store: resp[0] = the served seq,
  // resp[1] = status, resp[2..14] = the outputs when they fit 52 bytes, resp[15] =
  // line_check(resp[0..14]).  No fence orders the line's dwords, so the host takes the line
  // only when the check matches (a torn write is waited out, never read).  Larger outputs go
  // to `out` first, behind a release fence.
  alignas(64) uint32_t resp[16];
  // the launch id on exit (device)
  alignas(64) uint32_t exit_gen;
  alignas(64) uint32_t out[kSrvOut / 4];
};
constexpr int kSrvInlineOut = 52;

// The check word of a 64-B line: the XOR of a hash of each of its first 15 dwords and their
// positions -- on the device one hash per lane and a 4-step XOR across the lanes of a DPP row,
// where a chained hash cost 15 dependent readlanes and multiplies on the request path (twice:
// request and response)
__host__ __device__ inline uint32_t word_mix(uint32_t w, uint32_t k) {
  uint32_t h = w ^ (0x9E3779B9u * (k + 1u));
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  h *= 0x846CA68Bu;
  h ^= h >> 16;
  return h;
}
inline uint32_t line_check(const uint32_t* w) {
  uint32_t h = 0;
  for (uint32_t k = 0; k < 15; ++k) h ^= word_mix(w[k], k);
  return h;
}
// every lane: line_check of the 16-lane row holding it (lane r of the row holds dword r)
__device__ __forceinline__ uint32_t line_check_row(uint32_t v, int lane) {
  const int r = lane & 15;
  int h = (int)(r < 15 ? word_mix(v, (uint32_t)r) : 0u);
  h ^= __builtin_amdgcn_update_dpp(0, h, 0x128, 0xF, 0xF, false);  // row_ror:8
  h ^= __builtin_amdgcn_update_dpp(0, h, 0x124, 0xF, 0xF, false);  // row_ror:4
  h ^= __builtin_amdgcn_update_dpp(0, h, 0x122, 0xF, 0xF, false);  // row_ror:2
  h ^= __builtin_amdgcn_update_dpp(0, h, 0x121, 0xF, 0xF, false);  // row_ror:1
  return (uint32_t)h;
}
static_assert(offsetof(SrvMailbox, more) == 64, "the payload continues after the request line");

__device__ __forceinline__ uint32_t sys_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ int32_t sys_load(const int32_t* p) {
  return (int32_t)sys_load(reinterpret_cast<const uint32_t*>(p));
}

__global__ __launch_bounds__(64) void scalar_server_kernel(SrvMailbox* mb, uint32_t served, uint32_t gen,
                                                           uint64_t idle_ticks) {
  __shared__ uint8_t lut[2][256];
  __shared__ uint32_t in_l[kSrvIn / 4], out_l[kSrvOut / 4];
  const int lane = threadIdx.x;
  for (int c = lane; c < 256; c += 64) {
    lut[0][c] = lut_entry(2, c);
    lut[1][c] = lut_entry(3, c);
  }
  __syncthreads();
  // One poll in flight on each copy of the request line, and the wall clock read only every 32nd
  // round of polls (the idle exit).  Round-6 A/B of the library's C call (one TwoBit pair,
  // tools/scalar_floor_probe.hip, profiles/scalar_floor_r06/): two loads in flight on the same
  // line 4.81-4.84 us, one poll at a time 3.47-3.49 (the clock read on every poll +0.02-0.03),
  // one poll on each of two copies and the lane-parallel check word 2.09-2.22, on each of four
  // 1.98.  A polled mailbox answers in steps of its polls, so the time also depends on the host's
  // own time between calls: averaged over 0-2 us of it, 2.23-2.25 us with four copies, 2.5 with
  // two, 4.2 before round 6 (the polls bunched, see below).  Sleeping a calibrated quarter round
  // trip after every reload made it worse: 2.81-3.04.
  uint64_t t_last = wall_clock64();
  bool served_since = false;  // t_last is refreshed at the next clock read, off the request path
  // Serves the request `line` holds (lane r of each row holds dword r; a new seq, check word
  // matched).
  auto serve = [&](const uint32_t line) {
    const uint32_t seq = __builtin_amdgcn_readlane(line, 0);
    const uint32_t h1 = __builtin_amdgcn_readlane(line, 1), h2 = __builtin_amdgcn_readlane(line, 2),
                   h3 = __builtin_amdgcn_readlane(line, 3), h4 = __builtin_amdgcn_readlane(line, 4),
                   h5 = __builtin_amdgcn_readlane(line, 5), h6 = __builtin_amdgcn_readlane(line, 6),
                   h7 = __builtin_amdgcn_readlane(line, 7);
    auto off16 = [](uint32_t v) { return v == 0xFFFFu ? -1 : (int)v; };
    const uint32_t op = h1 & 0xFFu;
    const int kind = (int)((h1 >> 8) & 0xFFu), words = (int)(h1 >> 16);
    const int n = (int)(h2 & 0xFFFFu), L = (int)(h2 >> 16);
    const int stride = (int)(h3 & 0xFFFFu), maxlen = (int)(h3 >> 16);
    const int in_words = ((int)(h4 & 0xFFFFu) + 3) / 4, out_words = ((int)(h4 >> 16) + 3) / 4;
    const int io[2] = {off16(h5 & 0xFFFFu), off16(h5 >> 16)};
    const int oo[3] = {off16(h6 & 0xFFFFu), off16(h6 >> 16), off16(h7 & 0xFFFFu)};
    // payload: the first 7 dwords came with the line; the rest (if any) in one more round trip.
    // No acquire fence: the rest is read with system-scope loads (they bypass the caches) issued
    // only after this wave saw the sequence number the host stored after the payload, so they
    // return the new bytes; a system-scope acquire here was a whole-L2 invalidate
    // (buffer_inv sc0 sc1) on every request (round 6)
    if (lane >= 8 && lane < 15 && lane - 8 < in_words) in_l[lane - 8] = line;
    for (int k = kSrvInline / 4 + lane; k < in_words; k += 64) in_l[k] = sys_load(&mb->more[k - kSrvInline / 4]);
    for (int k = lane; k < out_words; k += 64) out_l[k] = 0u;
    __syncthreads();
    const uint8_t* in8 = reinterpret_cast<const uint8_t*>(in_l);
    uint8_t* out8 = reinterpret_cast<uint8_t*>(out_l);
    const int r = lane;
    if (r < n) {
      switch (op) {
        case OP_ENCODE: {
          RecordReader rd{in8 + io[0] + r * stride, false, 0u, -1};
          uint32_t g, fl;
          encode_record(lut[kind == 2 ? 0 : 1], kind, rd, L, words,
                        reinterpret_cast<uint64_t*>(out8 + oo[0]) + r * words, g, fl);
          if (oo[1] >= 0) out8[oo[1] + r] = (uint8_t)(g > 255 ? 255 : g);
          if (oo[2] >= 0) out8[oo[2] + r] = (uint8_t)fl;
          break;
        }
        case OP_DECODE2:
          decode2_record(reinterpret_cast<const uint64_t*>(in8 + io[0]) + r * words, words, L, out8 + oo[0] + r * L);
          break;
        case OP_DECODE3: {
          int32_t err;
          const int32_t len = decode3_record(reinterpret_cast<const uint64_t*>(in8 + io[0]) + r * words, words, maxlen,
                                             out8 + oo[0] + r * maxlen, err);
          reinterpret_cast<int32_t*>(out8 + oo[1])[r] = len;
          reinterpret_cast<int32_t*>(out8 + oo[2])[r] = err;
          break;
        }
        case OP_GC:
          reinterpret_cast<int32_t*>(out8 + oo[0])[r] =
              gc_record(kind, reinterpret_cast<const uint64_t*>(in8 + io[0]) + r * words, words, L);
          break;
        case OP_HAMMING:
          reinterpret_cast<int32_t*>(out8 + oo[0])[r] =
              hamming_record(kind, reinterpret_cast<const uint64_t*>(in8 + io[0]) + r * words,
                             reinterpret_cast<const uint64_t*>(in8 + io[1]) + r * words, words);
          break;
        default:
          break;
      }
    }
    __syncthreads();
    const bool inline_out = out_words * 4 <= kSrvInlineOut;
    if (!inline_out) {
      for (int k = lane; k < out_words; k += 64)
        __hip_atomic_store(&mb->out[k], out_l[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    }
    const uint32_t status = op >= OP_ENCODE && op <= OP_HAMMING ? 0u : 1u;
    uint32_t v = lane == 0 ? seq : lane == 1 ? status : (lane < 15 && inline_out && lane - 2 < out_words) ? out_l[lane - 2] : 0u;
    const uint32_t check = line_check_row(v, lane);
    if (lane == 15) v = check;
    if (lane < 16) __hip_atomic_store(&mb->resp[lane], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    served = seq;
    served_since = true;
  };
  // Every lane loads dword (lane & 15), so no lane branch surrounds the loads, and a copy's next
  // load is issued only after its line was examined (into the same register): the wait for the
  // oldest poll is then vmcnt(kSrvCopies - 1) and the other copies' loads stay in flight.  (An
  // array of copies in a loop over j was compiled with a full drain every round: the registers
  // rotated.)
  auto line_at = [&](int j) { return j == 0 ? mb->req + (lane & 15) : mb->req_copy[j - 1] + (lane & 15); };
  // The copies' polls are spread over a round trip: after the first poll and after every request
  // (when the polls in flight all came back while it was served) the next kSrvCopies - 1 polls are
  // issued a round trip / kSrvCopies apart (the round trip timed once here on the 100-MHz wall
  // clock); in between, each copy is reissued as soon as it was examined, which keeps the spacing.
  // Issued back to back instead, the polls stay bunched and a request waits for the next burst:
  // a saw-tooth of 2.0-2.9 us per C call over the host's own time between calls.
  uint64_t delta = 0, t_issue = 0;  // wall-clock ticks between spaced polls; the last one's issue
  int stagger = 0;                  // polls left to space
#ifndef SCT_SRV_NO_STAGGER
  {
    __builtin_amdgcn_s_waitcnt(0);
    const uint64_t t0 = wall_clock64();
    const uint32_t x = sys_load(line_at(0));
    __builtin_amdgcn_s_waitcnt(0);
    const uint64_t t1 = wall_clock64() + (__builtin_amdgcn_readlane(x, 0) & 0u);
    delta = min<uint64_t>((t1 - t0) / kSrvCopies, 100);
  }
#endif
  auto reload = [&](int j) {
    if (stagger > 0) {
      t_issue += delta;
      while (wall_clock64() < t_issue) {
      }
      --stagger;
    }
    return sys_load(line_at(j));
  };
  // (one load site per copy: with a second one on the request path the compiler gave the copies
  // new registers and moved them back at the end of every round, a full drain of the polls)
  auto step = [&](uint32_t& v, int j) {
    if ((int32_t)(__builtin_amdgcn_readlane(v, 0) - served) > 0 &&
        __builtin_amdgcn_readlane(line_check_row(v, lane), 0) == __builtin_amdgcn_readlane(v, 15)) {
      serve(v);
      t_issue = wall_clock64() - delta;  // this copy's poll goes out at once, the next ones spaced
      stagger = kSrvCopies;
    }
    v = reload(j);
  };
  static_assert(kSrvCopies == 2 || kSrvCopies == 4, "2 or 4 copies of the request line");
  t_issue = wall_clock64() - delta;
  stagger = kSrvCopies;
  uint32_t v0 = reload(0), v1 = reload(1);
  uint32_t v2 = kSrvCopies > 2 ? reload(2) : 0u, v3 = kSrvCopies > 2 ? reload(3) : 0u;
  for (uint32_t it = 1;; ++it) {
    step(v0, 0);
    step(v1, 1);
    if constexpr (kSrvCopies > 2) {
      step(v2, 2);
      step(v3, 3);
    }
    // the stop word costs a round trip of its own: looked at every 128th round of polls (~0.2 ms)
    if ((it & 127) == 0 && sys_load(&mb->stop) != 0u) break;
    if ((it & 31) == 0) {
      const uint64_t now = wall_clock64();
      if (served_since) t_last = now, served_since = false;
      else if (now - t_last > idle_ticks) break;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  if (lane == 0) __hip_atomic_store(&mb->exit_gen, gen, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

struct Server {
  int device = -1;
  SrvMailbox* mb = nullptr;      // host view
  SrvMailbox* mb_dev = nullptr;  // device view
  hipStream_t stream = nullptr;
  uint32_t seq = 0;
  std::atomic<uint32_t> gen{0};
  uint64_t idle_ticks = 0;
};

std::mutex g_srv_mu;
std::vector<Server*> g_servers;  // every server of the process (quiesce, exit)
std::atomic<int64_t> g_srv_launches{0};

template <class T>
T host_load(const T* p) {
  return __atomic_load_n(p, __ATOMIC_ACQUIRE);
}

bool server_running(const Server* sv) { return host_load(&sv->mb->exit_gen) != sv->gen.load(); }

// ask one server to exit and wait (bounded) for its exit mark; no HIP calls (process exit)
void server_stop(Server* sv, int64_t wait_us) {
  if (!server_running(sv)) return;
  __atomic_store_n(&sv->mb->stop, 1u, __ATOMIC_RELEASE);
  const auto t0 = std::chrono::steady_clock::now();
  while (server_running(sv) &&
         std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(wait_us)) {
  }
}

void stop_all_at_exit() {
  std::lock_guard<std::mutex> g(g_srv_mu);
  for (Server* sv : g_servers) server_stop(sv, 200000);
}

bool server_enabled() { return sct::tune(SCT_TUNE_SCALAR_SERVER, 1) != 0; }

// A host thread's servers (one per device).  When the thread ends its servers are stopped
// and their stream and mailbox freed, so thread churn does not pile up resident waves,
// streams and pinned memory; a server that does not confirm its exit is left alone (its
// mailbox must outlive it).
struct ThreadServers {
  Server* per_dev[64] = {};
  ~ThreadServers() {
    for (Server*& sv : per_dev) {
      if (!sv) continue;
      {  // out of the process list under the lock; the (bounded, up to 1 s) stop outside it
        std::lock_guard<std::mutex> g(g_srv_mu);
        g_servers.erase(std::remove(g_servers.begin(), g_servers.end(), sv), g_servers.end());
      }
      server_stop(sv, 1000000);
      if (server_running(sv)) {  // left alone, and back in the list for the exit-time stop
        std::lock_guard<std::mutex> g(g_srv_mu);
        g_servers.push_back(sv);
        continue;
      }
      int cur = -1;
      if (hipGetDevice(&cur) == hipSuccess && hipSetDevice(sv->device) == hipSuccess) {
        (void)hipStreamSynchronize(sv->stream);
        (void)hipStreamDestroy(sv->stream);
        (void)hipHostFree(sv->mb);
        (void)hipSetDevice(cur);
      }
      (void)hipGetLastError();
      delete sv;
      sv = nullptr;
    }
  }
};

// nullptr (error set) if the server cannot be created; callers then take the launch path
Server* server() {
  static thread_local ThreadServers mine;
  Server** per_dev = mine.per_dev;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  if (per_dev[dev]) return per_dev[dev];
  auto* sv = new Server();
  sv->device = dev;
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) khz = 100000;
  const int64_t ms = sct::tune(SCT_TUNE_SCALAR_IDLE_MS, 5);
  sv->idle_ticks = (uint64_t)khz * (uint64_t)(ms > 0 ? ms : 5);
  if (hipStreamCreateWithFlags(&sv->stream, hipStreamNonBlocking) != hipSuccess ||
      hipHostMalloc((void**)&sv->mb, sizeof(SrvMailbox), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess ||
      hipHostGetDevicePointer((void**)&sv->mb_dev, sv->mb, 0) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;  // leaked on this rare path; the launch path still works
  }
  memset(sv->mb, 0, sizeof(SrvMailbox));  // exit_gen == gen == 0: "not running"
  {
    std::lock_guard<std::mutex> g(g_srv_mu);
    if (g_servers.empty()) atexit(stop_all_at_exit);  // runs before HIP's own teardown
    g_servers.push_back(sv);
  }
  per_dev[dev] = sv;
  return sv;
}

int server_launch(Server* sv) {
  SCT_HIP(hipStreamSynchronize(sv->stream));  // the previous server has returned
  const uint32_t gen = sv->gen.load() + 1;
  __atomic_store_n(&sv->mb->stop, 0u, __ATOMIC_RELEASE);
  sv->gen.store(gen);
  hipLaunchKernelGGL(scalar_server_kernel, dim3(1), dim3(64), 0, sv->stream, sv->mb_dev, host_load(&sv->mb->resp[0]), gen,
                     sv->idle_ticks);
  SCT_LAUNCH_CHECK();
  g_srv_launches.fetch_add(1);
  return SCT_OK;
}
}  // namespace

int sct::srv_call(uint32_t op, int kind, int64_t n, int words, int L, int64_t stride, int maxlen, const In* ins, int ni,
                  const Out* outs, int no) {
  if (!server_enabled() || n > kSrvMaxN || stride > kSrvIn || L > kSrvOut || maxlen > kSrvOut || words > 255) return 1;
  // 8-byte aligned pieces (the widest element is a uint64 code): a pair of one-limb codes is 16 B
  // and rides in the request line; 16-byte alignment made it 32 B, past the 28 inline bytes, and
  // cost every hamming_distance call a second PCIe round trip for the rest (round 6)
  auto al = [](size_t x) { return (x + 7) & ~(size_t)7; };
  int32_t io[2] = {-1, -1}, oo[3] = {-1, -1, -1};
  size_t tin = 0, tout = 0;
  for (int k = 0; k < ni; ++k) {
    io[k] = (int32_t)tin;
    tin += al(ins[k].bytes);
  }
  for (int k = 0; k < no; ++k) {
    if (!outs[k].p) continue;
    oo[k] = (int32_t)tout;
    tout += al(outs[k].bytes);
  }
  if (tin > (size_t)kSrvIn || tout > (size_t)kSrvOut) return 1;
  Server* sv = server();
  if (!sv) return 1;
  SrvMailbox* mb = sv->mb;
  uint32_t req[16] = {};  // the request line, written to both copies; seq last in each
  {  // payload bytes [0, 28) into req[8..14], the rest into `more`
    uint8_t pay[kSrvIn];
    for (int k = 0; k < ni; ++k)
      if (ins[k].bytes) memcpy(pay + io[k], ins[k].p, ins[k].bytes);
    memcpy(&req[8], pay, std::min<size_t>(tin, kSrvInline));
    if (tin > (size_t)kSrvInline) memcpy(mb->more, pay + kSrvInline, tin - kSrvInline);
  }
  auto o16 = [](int32_t v) { return v < 0 ? 0xFFFFu : (uint32_t)v; };
  req[1] = op | (uint32_t)kind << 8 | (uint32_t)words << 16;
  req[2] = (uint32_t)n | (uint32_t)L << 16;
  req[3] = (uint32_t)stride | (uint32_t)maxlen << 16;
  req[4] = (uint32_t)tin | (uint32_t)tout << 16;
  req[5] = o16(io[0]) | o16(io[1]) << 16;
  req[6] = o16(oo[0]) | o16(oo[1]) << 16;
  req[7] = o16(oo[2]);
  const uint32_t seq = ++sv->seq;
  req[0] = seq;
  req[15] = line_check(req);
  for (int j = 0; j < kSrvCopies; ++j) {
    uint32_t* line = j == 0 ? mb->req : mb->req_copy[j - 1];
    memcpy(line + 1, req + 1, 15 * 4);
    __atomic_store_n(&line[0], seq, __ATOMIC_RELEASE);
  }
  const auto t0 = std::chrono::steady_clock::now();
  uint32_t line[16];
  auto answered = [&]() {  // the whole response line of this request, check included
    if (host_load(&mb->resp[0]) != seq) return false;
    for (int k = 0; k < 16; ++k) line[k] = host_load(&mb->resp[k]);
    return line[0] == seq && line_check(line) == line[15];
  };
  for (uint32_t spin = 1;; ++spin) {
    if (answered()) break;
    if (!server_running(sv)) {
      if (answered()) break;  // served just before it left
      SCT_TRY(server_launch(sv));
      continue;
    }
    if ((spin & 4095) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10))
      return sct::fail(SCT_E_HIP, "scalar server: no answer in 10 s");
  }
  if (line[1] != 0) return sct::fail(SCT_E_HIP, "scalar server: bad request");
  const uint8_t* res = tout <= (size_t)kSrvInlineOut ? reinterpret_cast<const uint8_t*>(line + 2)
                                                     : reinterpret_cast<const uint8_t*>(mb->out);
  for (int k = 0; k < no; ++k)
    if (outs[k].p && outs[k].bytes) memcpy(outs[k].p, res + oo[k], outs[k].bytes);
  return SCT_OK;
}

void sct::scalar_quiesce() {
  std::lock_guard<std::mutex> g(g_srv_mu);
  for (Server* sv : g_servers) server_stop(sv, 1000000);
}

extern "C" int sct_scalar_server_stop(void) {
  sct::scalar_quiesce();
  return SCT_OK;
}

extern "C" int sct_scalar_server_status(int64_t* launches, int* running) {
  if (launches) *launches = g_srv_launches.load();
  if (running) {
    std::lock_guard<std::mutex> g(g_srv_mu);
    int c = 0;
    for (Server* sv : g_servers) c += server_running(sv) ? 1 : 0;
    *running = c;
  }
  return SCT_OK;
}
