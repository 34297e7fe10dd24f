// The weight-gradient tile of the output heads (bf16 features, F = 32, small capacities): what both backward kernels
// (head.hip, head_mfma.h) share.  A kernel leaves 128 pixels in LDS as a row image of bf16 values, one row per pixel:
//   bytes [0,128)    V = dlogits (8) | dmid (24)     dheat (16)     0 (16)
//   bytes [128,256)  x (32)                          U = logits (8) | mid (24)
// and its four waves multiply the first block, transposed, by the second on the matrix cores (contraction over the
// pixels through transposing LDS reads, as csrc/wgradp_bf16.hip): a 64 x 64 fp32 product per workgroup, a 32 x 32
// quarter per wave.  Every workgroup stores its sum over its tiles as one partial; head_wgrad_finish_kernel (head.hip)
// adds the partials up and files the three blocks of the product that are weight gradients.
#pragma once
#include "common.h"

namespace dfl {

constexpr int HEAD_WG_PITCH = 320;                             // bytes from one pixel's row to the next
constexpr int HEAD_WG_ROWS = 128;                              // pixels of a row image
constexpr int HEAD_WG_LDS = HEAD_WG_ROWS * HEAD_WG_PITCH;      // bytes of LDS a row image takes
constexpr int HEAD_WG_PART = 64 * 64;                          // floats of a workgroup's partial
constexpr int HEAD_WG_V = 0, HEAD_WG_DHEAT = 64, HEAD_WG_ZERO = 96, HEAD_WG_X = 128, HEAD_WG_U = 192;   // byte offsets in a row

// 8 consecutive pixels of one column of a [pixel][column] bf16 image: two transposing reads (csrc/wgradp_bf16.hip)
__device__ __forceinline__ bf16x8_t htr_read8(const unsigned char* base, uint32_t r0, uint32_t r1) {
  typedef short hs16x4_t __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(3))) hs16x4_t* lds_p;
  const hs16x4_t x = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(base + r0));
  const hs16x4_t y = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(base + r1));
  return __builtin_bit_cast(bf16x8_t, __builtin_shufflevector(x, y, 0, 1, 2, 3, 4, 5, 6, 7));
}

// This lane's place in its wave's quarter of the product (workgroups of four waves)
struct HeadWgLane {
  int lane, wave, trow;        // trow: its pixel within a 16-pixel step of the contraction (and trow + 4)
  uint32_t a_col, b_col;       // byte offsets of its A and B fragments within a row
  __device__ __forceinline__ HeadWgLane() : lane(threadIdx.x & 63), wave(threadIdx.x >> 6) {
    trow = 8 * (lane >> 5) + ((lane & 15) >> 2);
    const uint32_t tcb = (uint32_t)((16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2);
    a_col = (uint32_t)((wave >> 1) * 64) + tcb;
    b_col = (uint32_t)HEAD_WG_X + (uint32_t)((wave & 1) * 64) + tcb;
  }
  // acc += (first block)^T (second block) over the pixels of the row image at ab
  __device__ __forceinline__ void product(const unsigned char* ab, f32x16& acc) const {
#pragma unroll
    for (int ks = 0; ks < HEAD_WG_ROWS / 16; ++ks) {
      const uint32_t r0 = (uint32_t)(ks * 16 + trow) * (uint32_t)HEAD_WG_PITCH, r1 = r0 + 4u * (uint32_t)HEAD_WG_PITCH;
      const bf16x8_t af = htr_read8(ab, r0 + a_col, r1 + a_col);
      const bf16x8_t bf = htr_read8(ab, r0 + b_col, r1 + b_col);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc, 0, 0, 0);
    }
  }
  // wg_partial[block][row of the first block (64)][column of the second (64)]
  __device__ __forceinline__ void store(float* wg_partial, const f32x16& acc) const {
    float* part = wg_partial + (int64_t)blockIdx.x * HEAD_WG_PART;
    const int col = (wave & 1) * 32 + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) part[((wave >> 1) * 32 + mfma32_row(r, lane)) * 64 + col] = acc[r];
  }
};

}  // namespace dfl
