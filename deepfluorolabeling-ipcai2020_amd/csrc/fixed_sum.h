// The fixed-order float64 reduction of the registration kernels (csrc/sim.hip, sim_patch.hip, drr_grad.hip): wave shuffles,
// the four waves through LDS as ((w0 + w1) + w2) + w3, one record per workgroup with plain stores, then the records in
// index order.  No atomics, so a result's bits depend on its own inputs and on the launch shape alone.
#pragma once
#include "common.h"

namespace dfl {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// N sums of a workgroup of four waves -> thread 0's v[]; lds holds N * 4 doubles.  A kernel that calls this again
// puts a barrier in between: the next call's lane 0 writes the LDS that thread 0 reads here.
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], double* lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = wave_sum(v[k]);
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

// One number of R records of N doubles each, added in index order; rec points at that number in record 0
__device__ __forceinline__ double records_sum(const double* __restrict__ rec, int R, int N) {
  double acc = 0.0;
  for (int t = 0; t < R; ++t) acc += rec[(size_t)t * N];
  return acc;
}

}  // namespace dfl
