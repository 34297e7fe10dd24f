// The row epilogue of the patch-resident bf16 convolution kernels (convp_bf16.hip, convq_bf16.hip), written once.
//
// dfl_conv2d defines one epilogue for bf16 tensors: bias, ReLU, + BN(add), accumulate, ONE rounding to bf16, store, and the
// statistics of the values AS STORED (sum v, sum v * u with u = v or the partner tensor stat_other).  Both kernels drop their
// accumulators into LDS as an fp32 image [rows][BN columns] and let every thread take 8 consecutive columns of a row; what a
// thread does with those eight sums, where the per-column constants come from and how the threads' statistics meet is here:
//   ep_col_consts  a column's bias and the scale / shift of "+ BN(add)", given or derived from the live totals
//   ep_row8        one 8-column unit of one output pixel, from "v holds eight sums" to "s1 and s2 updated"
//   ep_stats_tail  the fixed-order reduction of the threads' s1 / s2 through LDS, [RPS][2][BN]
// The callers keep what differs between them: the decode of an image row into a pixel and the element offsets (convp's
// scatter2x2 addressing, the 32-bit offset arithmetic), convq's sum of its two k-groups' images, the K-slice stores.
//
// NOT here, on purpose -- each would need its own parameters and the shared body would be machinery:
//   * convn_bf16.hip: its epilogue runs on the accumulator registers in another lane layout (16 values per lane,
//     permlane32_swap, buffer stores);
//   * convs.hip and its finish kernel: 4-channel units, the pair's second product, out_scale;
//   * the per-element row loop of convp_finish_kernel (one column per thread): only its constants come from ep_col_consts;
//   * the fp32 epilogue, conv_epilogue.h.
#pragma once
#include "common.h"

namespace dfl {

// Column n of the GEMM (`ok`: it exists), whose bias is bias[co] (`bias_on`: the caller wants it -- not under K slices, where the
// finish kernel adds it).  Absent terms are 0 / 1 / 0.
__device__ __forceinline__ void ep_col_consts(const dfl_conv_args& a, int n, int co, bool ok, bool bias_on, float* bias, float* sc,
                                              float* sh) {
  *bias = 0.f;
  *sc = 1.f;
  *sh = 0.f;
  if (a.bias != nullptr && ok && bias_on) *bias = a.bias[co];
  if (a.add != nullptr && ok) {
    if (a.add_scale != nullptr) *sc = a.add_scale[n], *sh = a.add_shift[n];
    else if (a.add_tot != nullptr) bn_live_affine(a.add_tot, a.add_gamma, a.add_beta, a.add_count, a.bn_eps, a.Ntot, n, sc, sh);
  }
}

// eight floats at a 16-byte aligned address (an LDS table) or of a register array
__device__ __forceinline__ void ep_ld8(const float* p, float* f) {
  const float4 lo = *reinterpret_cast<const float4*>(p), hi = *reinterpret_cast<const float4*>(p + 4);
  f[0] = lo.x; f[1] = lo.y; f[2] = lo.z; f[3] = lo.w; f[4] = hi.x; f[5] = hi.y; f[6] = hi.z; f[7] = hi.w;
}

// v[8]: the sums of 8 consecutive columns of one output pixel.  cbias / casc / cash: those columns' constants (ep_col_consts); the
// scale and shift are fetched only when there is an `add` (a caller that passes LDS pointers keeps 16 registers free that way).
// add_off / y_off / so_off: element offsets of the unit in add / y / stat_other, the caller's arithmetic.
__device__ __forceinline__ void ep_row8(const dfl_conv_args& a, float (&v)[8], const float* cbias, const float* casc, const float* cash,
                                        const unsigned short* addp, uint32_t add_off, unsigned short* yp, uint32_t y_off,
                                        const unsigned short* sop, uint32_t so_off, bool do_stats, float (&s1)[8], float (&s2)[8]) {
  {
    float cb[8];
    ep_ld8(cbias, cb);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      v[e] += cb[e];
      if (a.relu) v[e] = fmaxf(v[e], 0.f);
    }
  }
  if (addp != nullptr) {
    float o[8], sc[8], sh[8];
    unpack8(*reinterpret_cast<const u32x4*>(addp + add_off), o);
    ep_ld8(casc, sc);
    ep_ld8(cash, sh);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] += fmaf(o[e], sc[e], sh[e]);
  }
  if (a.accumulate) {
    float o[8];
    unpack8(*reinterpret_cast<const u32x4*>(yp + y_off), o);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] += o[e];
  }
  const u32x4 w = pack8(v);
  *reinterpret_cast<u32x4*>(yp + y_off) = w;
  if (do_stats) {
    float vr[8], u[8];
    unpack8(w, vr);                                   // statistics of the values as stored
    if (sop != nullptr) {
      unpack8(*reinterpret_cast<const u32x4*>(sop + so_off), u);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) u[e] = vr[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      s1[e] += vr[e];
      s2[e] = fmaf(vr[e], u[e], s2[e]);
    }
  }
}

// Per-column sums of the workgroup's NT threads: thread (urow, ucol) leaves its s1 / s2 in red[RPS][2][BN] (`rowthread`: it has
// a row at all), then column n0 + col < Ntot is summed over w = 0 .. RPS - 1 -- a fixed order -- and handed to
// store(which, n, sum): a row of stat_partials or the layer's live totals, the caller's choice.
template <int BN, int RPS, int NT, typename Store>
__device__ __forceinline__ void ep_stats_tail(float* red, const float (&s1)[8], const float (&s2)[8], int urow, int ucol, bool rowthread, int n0,
                                              int Ntot, Store store) {
  __syncthreads();                                    // the image `red` lies in is no longer read
  if (rowthread) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      red[(urow * 2 + 0) * BN + ucol + e] = s1[e];
      red[(urow * 2 + 1) * BN + ucol + e] = s2[e];
    }
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 2 * BN; idx += NT) {
    const int which = idx / BN, col = idx - which * BN;
    const int n = n0 + col;
    if (n < Ntot) {
      float sum = 0.f;
      for (int w = 0; w < RPS; ++w) sum += red[(w * 2 + which) * BN + col];
      store(which, n, sum);
    }
  }
}

}  // namespace dfl
