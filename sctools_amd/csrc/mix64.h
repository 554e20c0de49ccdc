// The slot hash of the device hash tables (count.hip, molecules.hip).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define SCT_HD __host__ __device__ __forceinline__
#else
#define SCT_HD inline
#endif

namespace sct {

SCT_HD uint64_t mix64(uint64_t x) {  // murmur3's finaliser: every input bit reaches the low bits
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

}  // namespace sct
