// What csrc/sim.hip (global gradient-NCC) and csrc/sim_patch.hip (patch-wise gradient-NCC) share: the Sobel gradients, the
// fixed-order sums of a workgroup and the NCC of one-pass sums.  One definition, so that both files give the same bits.
#pragma once
#include "common.h"

namespace dfl {

constexpr int SIM_THREADS = 256;

// Sobel gradients of p at interior pixel (r, c): each sum left to right, so the fixed and the moving image share bits
__device__ __forceinline__ void sim_sobel(const float* __restrict__ p, int W, int r, int c, float& gx, float& gy) {
  const float* up = p + (size_t)(r - 1) * W + c;
  const float* mid = up + W;
  const float* dn = mid + W;
  const float a = up[-1], b = up[0], cc = up[1], d = mid[-1], f = mid[1], g = dn[-1], h = dn[0], i = dn[1];
  gx = ((cc + 2.f * f) + i) - ((a + 2.f * d) + g);
  gy = ((g + 2.f * h) + i) - ((a + 2.f * b) + cc);
}

__device__ __forceinline__ double sim_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// N sums of a workgroup of SIM_THREADS threads -> thread 0's v[]; lds holds N * 4 doubles
template <int N>
__device__ __forceinline__ void sim_block_sum(double (&v)[N], double* lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = sim_wave_sum(v[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) lds[wave * N + k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = ((lds[k] + lds[N + k]) + lds[2 * N + k]) + lds[3 * N + k];
  }
}

// A variance is 0 when it is at most 2^-40 of the sum of squares: below that the one-pass form cannot tell
__device__ __forceinline__ double sim_ncc(double n, double sa, double saa, double sb, double sbb, double sab) {
  const double va = saa - sa * sa / n, vb = sbb - sb * sb / n;
  const double eps = 9.094947017729282e-13;                             // 2^-40
  if (!(va > eps * saa) || !(vb > eps * sbb)) return 0.0;
  return (sab - sa * sb / n) / sqrt(va * vb);
}

}  // namespace dfl
