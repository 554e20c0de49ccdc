// Stand-alone host check of the arithmetic behind the chunked host pipeline (host_items in
// sctools_amd/csrc/encode_host.cpp): the two chunk policies of host_pipeline.h against the formulas
// the two pipelines used before they became one, written out here step by step, and
// sct::StageLayout for every combination of page-locked and pageable arrays.  A stage's device
// block and the page-locked stage are malloc'ed buffers here and every byte a chunk occupies is
// written, so AddressSanitizer sees a segment that runs past its block.  No GPU, no Python:
//   c++ -std=c++17 -g -fsanitize=address,undefined this.cpp
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <utility>

#include "../../sctools_amd/csrc/host_pipeline.h"

#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                         \
    }                                                                  \
  } while (0)

// ---------------------------------------------------------------- the chunk policies
// the element-wise pipeline as it was: ~16 MB of traffic per chunk, at least four chunks
static int64_t old_items_chunk(int64_t n, size_t per) {
  int64_t chunk = (int64_t)((16u << 20) / (per ? per : 1));
  if (chunk < 65536) chunk = 65536;
  int64_t quarter = n / 4 + (n % 4 ? 1 : 0);
  if (quarter < 65536) quarter = 65536;
  if (chunk > quarter) chunk = quarter;
  if (chunk > n) chunk = n;
  return chunk;
}

// the encode stream as it was
static int64_t old_stream_chunk(int64_t n, int64_t chunk, bool staged) {
  if (chunk <= 0) chunk = 16777216;
  if (staged && chunk > 2097152) chunk = 2097152;
  int64_t quarter = n / 4 + (n % 4 ? 1 : 0);
  if (quarter < 262144) quarter = 262144;
  if (chunk > quarter) chunk = quarter;
  if (chunk > n) chunk = n;
  return chunk;
}

static const int64_t kN[] = {1, 65535, 65536, 262144, 262145, 3 * 262144 + 1, 16777216, 1000000000};

// ---------------------------------------------------------------- the stage layout
static size_t g_touched = 0;

template <int N>
static void check_layout(int64_t chunk, const size_t (&item)[N], unsigned staged_mask) {
  bool staged[N];
  for (int k = 0; k < N; ++k) staged[k] = item[k] && ((staged_mask >> k) & 1u);
  const sct::StageLayout<N> lay(chunk, item, staged);
  size_t need[N], want_h = 0;
  for (int k = 0; k < N; ++k) {
    need[k] = (size_t)chunk * item[k];
    if (staged[k]) want_h += (need[k] + 255) / 256 * 256;
  }
  EXPECT(lay.dtot % 256 == 0 && lay.htot % 256 == 0);
  EXPECT(lay.htot == want_h);  // page-locked and absent arrays take no stage bytes
  for (int k = 0; k < N; ++k) {
    const size_t dend = k + 1 < N ? lay.doff[k + 1] : lay.dtot;
    EXPECT(lay.doff[k] % 256 == 0);
    EXPECT(lay.doff[k] + need[k] <= dend);       // a segment ends before the next begins
    EXPECT(dend - lay.doff[k] < need[k] + 256);  // and wastes less than one alignment unit
    const size_t hend = k + 1 < N ? lay.hoff[k + 1] : lay.htot;
    EXPECT(lay.hoff[k] <= hend);
    if (staged[k]) {
      EXPECT(lay.hoff[k] % 256 == 0);
      EXPECT(lay.hoff[k] + need[k] <= hend && hend - lay.hoff[k] < need[k] + 256);
    } else {
      EXPECT(hend == lay.hoff[k]);
    }
  }
  // every byte a chunk occupies, in one device block and in the three stages' shares of the
  // page-locked buffer, lies inside and belongs to one array only (the largest chunks by
  // arithmetic alone)
  const size_t stage_bytes = (size_t)sct::kPipeStages * lay.htot;
  if (lay.dtot + stage_bytes > ((size_t)8 << 20)) return;
  uint8_t* dev = static_cast<uint8_t*>(malloc(lay.dtot ? lay.dtot : 1));
  uint8_t* pin = static_cast<uint8_t*>(malloc(stage_bytes ? stage_bytes : 1));
  EXPECT(dev && pin);
  memset(dev, 0, lay.dtot);
  memset(pin, 0, stage_bytes);
  for (int k = 0; k < N; ++k) {
    memset(dev + lay.doff[k], k + 1, need[k]);
    if (staged[k])
      for (int s = 0; s < sct::kPipeStages; ++s) memset(pin + (size_t)s * lay.htot + lay.hoff[k], 16 * (s + 1) + k + 1, need[k]);
  }
  size_t seen[256] = {};
  for (size_t i = 0; i < lay.dtot; ++i) ++seen[dev[i]];
  for (int k = 0; k < N; ++k) EXPECT(seen[k + 1] == need[k]);
  memset(seen, 0, sizeof(seen));
  for (size_t i = 0; i < stage_bytes; ++i) ++seen[pin[i]];
  for (int k = 0; k < N; ++k)
    for (int s = 0; s < sct::kPipeStages; ++s) EXPECT(seen[16 * (s + 1) + k + 1] == (staged[k] ? need[k] : 0));
  g_touched += lay.dtot + stage_bytes;
  free(dev);
  free(pin);
}

template <int N>
static void check_items(const size_t (&item)[N]) {
  size_t per = 0;
  for (int k = 0; k < N; ++k) per += item[k];
  int64_t last = -1;
  for (int64_t n : kN) {
    const int64_t chunk = sct::items_chunk(n, per);
    EXPECT(chunk == old_items_chunk(n, per) && chunk >= 1 && chunk <= n);
    if (chunk == last) continue;  // (the same layout again)
    last = chunk;
    for (unsigned mask = 0; mask < (1u << N); ++mask) check_layout(chunk, item, mask);
  }
}

static void check_stream(int L) {
  const size_t item[4] = {(size_t)L, 8, 1, 1};  // records in; codes, GC and flags out
  std::set<std::pair<int64_t, unsigned>> done;    // (the same layout again)
  for (int64_t n : kN)
    for (int64_t arg : {(int64_t)0, (int64_t)1, (int64_t)524288, n})
      for (unsigned mask = 0; mask < 16; ++mask) {
        const bool staged = mask != 0;
        const int64_t chunk = sct::stream_chunk(n, arg, staged);
        EXPECT(chunk == old_stream_chunk(n, arg, staged) && chunk >= 1 && chunk <= n);
        if (arg == 524288 && n >= 4 * 524288) EXPECT(chunk == 524288);
        if (!done.insert({chunk, mask}).second) continue;
        check_layout(chunk, item, mask);
        // the tiled encoder's condition on the records of every chunk: a 16-byte aligned start
        const bool st[4] = {(mask & 1u) != 0, (mask & 2u) != 0, (mask & 4u) != 0, (mask & 8u) != 0};
        EXPECT(sct::StageLayout<4>(chunk, item, st).doff[0] % 16 == 0);
      }
}

int main() {
  check_items<2>({16, 4});     // two-limb codes -> GC
  check_items<2>({8, 16});     // one-limb codes -> 16 bases
  check_items<2>({8, 4});      // one-limb codes -> GC
  check_items<3>({8, 8, 4});   // Hamming pairs
  check_items<4>({8, 22, 4, 4});  // ThreeBit decode: bases, lengths, bad
  check_items<4>({8, 22, 0, 0});  // absent outputs take nothing
  for (int L : {1, 16, 28}) check_stream(L);
  EXPECT(g_touched > 0);
  printf("host pipeline chunking and layout: ok (%zu MiB touched)\n", g_touched >> 20);
  return 0;
}
