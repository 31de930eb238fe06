// Counter-based Philox4x32-10 (Random123's round function and constants, restated; no rocRAND) and the 53-bit uniform
// the samplers take from two of its words.  Shared by kernels_shots.hip and kernels_mps_sample.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace bornvi {

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
    const uint32_t lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
    c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

__device__ __forceinline__ double unit53(uint32_t lo, uint32_t hi) {
  return (double)((((uint64_t)hi << 32) | lo) >> 11) * 0x1p-53;
}

}  // namespace bornvi
