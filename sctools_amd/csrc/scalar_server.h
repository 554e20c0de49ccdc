// The host arrays of a *_host call (encode_host.cpp) and the resident scalar server's call
// (scalar_server.hip) that serves the small ones.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace sct {

struct In {
  const void* p;
  size_t bytes;
};
struct Out {
  void* p;
  size_t bytes;
};

enum : uint32_t { OP_ENCODE = 1, OP_DECODE2 = 2, OP_DECODE3 = 3, OP_GC = 4, OP_HAMMING = 5 };

// One request of n <= 64 records through the calling thread's server on the current device:
// ins[ni] (ni <= 2) are packed into the mailbox, outs[no] (no <= 3; a null p is skipped) come back.
// Returns SCT_OK when served, 1 when the request does not fit the server (the caller takes
// the launch path), or an error code.
__attribute__((visibility("hidden"))) int srv_call(uint32_t op, int kind, int64_t n, int words, int L, int64_t stride, int maxlen, const In* ins, int ni,
             const Out* outs, int no);

}  // namespace sct
