// Counter-based normals shared by the kernels that add per-pixel noise (augment.hip, expose.hip): Philox4x32-10 keyed by
// a 64-bit key and counted by the pixel index, Box-Muller in fp32.  tests/aug_ref.py restates both in numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dfl {

__device__ __forceinline__ uint32_t mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }

// Philox4x32-10 (Salmon et al., SC'11): counter (c0, c1, 0, 0), key (k0, k1)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, uint32_t& o0, uint32_t& o1) {
  uint32_t x0 = c0, x1 = c1, x2 = 0u, x3 = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = mulhi32(0xD2511F53u, x0), lo0 = 0xD2511F53u * x0;
    const uint32_t hi1 = mulhi32(0xCD9E8D57u, x2), lo1 = 0xCD9E8D57u * x2;
    const uint32_t n0 = hi1 ^ x1 ^ k0, n2 = hi0 ^ x3 ^ k1;
    x0 = n0;
    x1 = lo1;
    x2 = n2;
    x3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  o0 = x0;
  o1 = x1;
}

// one standard normal per (key, index): u1 in (0, 1], u2 in [0, 1), z = sqrt(-2 ln u1) cos(2 pi u2), fp32
__device__ __forceinline__ float aug_normal(uint64_t key, int64_t idx) {
  uint32_t r0, r1;
  philox4x32_10((uint32_t)idx, (uint32_t)((uint64_t)idx >> 32), (uint32_t)key, (uint32_t)(key >> 32), r0, r1);
  const float u1 = (float)((r0 >> 8) + 1u) * 5.9604644775390625e-8f;   // 2^-24
  const float u2 = (float)(r1 >> 8) * 5.9604644775390625e-8f;
  return sqrtf(-2.f * logf(u1)) * cosf(6.2831853071795864769f * u2);
}

}  // namespace dfl
