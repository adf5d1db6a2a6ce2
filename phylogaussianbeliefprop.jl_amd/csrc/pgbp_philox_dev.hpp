// The counter-based generator of the device's normals, written once (pgbp_simulate.hip: counter (family, trait pair, site, 0);
// pgbp_post_uni.hip: counter (entry, draw, site, 1)): Philox4x32-10 and the 53-bit uniform of two of its outputs.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pgbp {

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw 2011): ten rounds, the key bumped between them
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t* __restrict__ out) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the 53-bit uniform of two outputs, offset by half a unit (never 0; the sum is rounded to nearest like any other)
__device__ __forceinline__ double sim_uniform(uint32_t a, uint32_t b) {
#pragma clang fp contract(off)
  const unsigned long long k = ((unsigned long long)(a >> 5) << 26) | (unsigned long long)(b >> 6);
  return ((double)k + 0.5) * 0x1p-53;
}

}  // namespace pgbp
