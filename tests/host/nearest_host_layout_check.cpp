// Stand-alone host check of the two pieces of host arithmetic behind the nearest *_host entry
// points: sct::NearestLayout (the one pool block of all four forms) and sct::PoolBlock (free the
// block on the stream, synchronise once, merge the HIP error -- on every path).  The pool and the
// stream are stubs here: a block is a malloc'ed buffer, so AddressSanitizer sees a segment that
// runs past the block, a block that is never freed and one freed twice.  No GPU, no Python:
//   c++ -std=c++17 -g -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ -I<rocm>/include this.cpp
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../sctools_amd/csrc/nearest_host.h"

// ---------------------------------------------------------------- stubs
static std::string g_error;
static std::vector<std::string> g_log;  // "free" / "sync" in call order
static int g_live = 0;
static hipError_t g_alloc_result = hipSuccess, g_sync_result = hipSuccess;

void sct::set_error(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_error = buf;
}
hipError_t sct::pool_alloc(void** p, size_t bytes, hipStream_t) {
  if (g_alloc_result != hipSuccess) return g_alloc_result;
  *p = malloc(bytes);
  ++g_live;
  return hipSuccess;
}
void sct::pool_free(void* p, hipStream_t) {
  free(p);
  --g_live;
  g_log.push_back("free");
}
extern "C" hipError_t hipStreamSynchronize(hipStream_t) {
  g_log.push_back("sync");
  return g_sync_result;
}
extern "C" const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "stub error"; }

#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                         \
    }                                                                  \
  } while (0)

// ---------------------------------------------------------------- the block layout
static void check_layout(int64_t nq, int L, bool tallied, int64_t nw) {
  const sct::NearestLayout lay(nq, L, tallied, nw);
  const size_t need[4] = {(size_t)nq * 8, (size_t)nq * (size_t)L, (size_t)nq * 4, (size_t)nq};
  const size_t at[5] = {0, lay.qual, lay.index, lay.dist, lay.tail};
  for (int k = 0; k < 4; ++k) {
    EXPECT(at[k] % 256 == 0 && at[k + 1] % 256 == 0);
    EXPECT(at[k] + need[k] <= at[k + 1]);       // a segment ends before the next begins
    EXPECT(at[k + 1] - at[k] < need[k] + 256);  // and wastes less than one alignment unit
  }
  // the tail: counts[nw] tally[2] err[1] if tallied, then stats[2] if correcting; nothing else
  const size_t words = (tallied ? (size_t)nw + 3 : 0) + (L > 0 ? 2 : 0);
  EXPECT(lay.tail_words == words && lay.total == lay.tail + words * 8);
  if (tallied) EXPECT(lay.counts == 0 && lay.tally == (size_t)nw && lay.err == (size_t)nw + 2);
  if (L > 0) EXPECT(lay.stats + 2 == words && (!tallied || lay.stats == lay.err + 1));
  // every byte the pipeline touches lies in the block, and no two segments share one
  sct::PoolBlock blk(nullptr);
  EXPECT(blk.alloc(lay.total) == SCT_OK);
  uint8_t* b = blk.bytes();
  memset(b, 0, lay.total);
  for (int k = 0; k < 4; ++k) memset(b + at[k], k + 1, need[k]);
  uint64_t* tail = reinterpret_cast<uint64_t*>(b + lay.tail);
  if (tallied) {
    for (int64_t j = 0; j < nw; ++j) tail[lay.counts + j] = 0x0505050505050505ull;
    tail[lay.tally] = tail[lay.tally + 1] = 0x0606060606060606ull;
    tail[lay.err] = 0x0707070707070707ull;
  }
  if (L > 0) tail[lay.stats] = tail[lay.stats + 1] = 0x0808080808080808ull;
  size_t seen[9] = {};
  for (size_t i = 0; i < lay.total; ++i) {
    EXPECT(b[i] <= 8);
    ++seen[b[i]];
  }
  for (int k = 0; k < 4; ++k) EXPECT(seen[k + 1] == need[k]);
  EXPECT(seen[5] == (tallied ? (size_t)nw * 8 : 0) && seen[6] == (tallied ? 16u : 0u) && seen[7] == (tallied ? 8u : 0u));
  EXPECT(seen[8] == (L > 0 ? 16u : 0u));
  EXPECT(blk.finish(SCT_OK, "layout") == SCT_OK);
}

// ---------------------------------------------------------------- the guard
static int early_return(bool fail_after_alloc) {
  sct::PoolBlock blk(nullptr);
  if (int rc = blk.alloc(64); rc != SCT_OK) return rc;
  memset(blk.p, 1, 64);
  if (fail_after_alloc) return sct::fail(SCT_E_INVALID, "an argument check after the allocation");
  return blk.finish(SCT_OK, "early");
}

static void check_guard() {
  const std::vector<std::string> free_then_sync = {"free", "sync"};
  // the normal end: the block goes back before the one synchronisation
  g_log.clear();
  EXPECT(early_return(false) == SCT_OK && g_live == 0 && g_log == free_then_sync);
  // a return before finish(): freed and synchronised all the same, the status and message kept
  g_log.clear();
  EXPECT(early_return(true) == SCT_E_INVALID && g_live == 0 && g_log == free_then_sync);
  EXPECT(g_error == "an argument check after the allocation");
  // the allocation fails: nothing to free, nothing enqueued to wait for
  g_log.clear();
  g_alloc_result = hipErrorOutOfMemory;
  EXPECT(early_return(false) == SCT_E_NOMEM && g_live == 0 && g_log.empty());
  g_alloc_result = hipSuccess;
  {  // the first noted error wins and becomes the status with its prefix
    sct::PoolBlock blk(nullptr);
    EXPECT(blk.alloc(8) == SCT_OK && blk.ok());
    blk.note(hipSuccess);
    blk.note(hipErrorInvalidValue);
    blk.note(hipErrorOutOfMemory);
    EXPECT(!blk.ok() && blk.e == hipErrorInvalidValue);
    g_log.clear();
    EXPECT(blk.finish(SCT_OK, "nearest count") == SCT_E_HIP && g_error == "nearest count: stub error");
    EXPECT(g_live == 0 && g_log == free_then_sync && blk.p == nullptr);
    g_log.clear();
  }  // the destructor after finish(): no second free, no second synchronisation
  EXPECT(g_log.empty() && g_live == 0);
  {  // a status the call already has is not replaced
    sct::PoolBlock blk(nullptr);
    EXPECT(blk.alloc(8) == SCT_OK);
    blk.note(hipErrorInvalidValue);
    const int rc = sct::fail(SCT_E_RANGE, "the call's own failure");
    EXPECT(blk.finish(rc, "x") == SCT_E_RANGE && g_error == "the call's own failure" && g_live == 0);
  }
  {  // the synchronisation's own error is merged too
    sct::PoolBlock blk(nullptr);
    EXPECT(blk.alloc(8) == SCT_OK);
    g_sync_result = hipErrorInvalidValue;
    EXPECT(blk.finish(SCT_OK, "sync") == SCT_E_HIP && g_error == "sync: stub error" && g_live == 0);
    g_sync_result = hipSuccess;
  }
  {  // no block (set_posterior without priors never allocates): finish only synchronises
    sct::PoolBlock blk(nullptr);
    g_log.clear();
    EXPECT(blk.finish(SCT_OK, "none") == SCT_OK && g_log == std::vector<std::string>{"sync"});
    g_log.clear();
  }
  EXPECT(g_log.empty());
}

int main() {
  for (int64_t nq : {1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000, 1257, 4099})
    for (int L : {0, 2, 5, 16})
      for (int tallied = 0; tallied < 2; ++tallied)
        for (int64_t nw : {0, 1, 300}) check_layout(nq, L, tallied != 0, nw);
  check_guard();
  EXPECT(g_live == 0);
  printf("nearest host layout and guard: ok\n");
  return 0;
}
