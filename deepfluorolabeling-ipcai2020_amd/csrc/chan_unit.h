// The channel unit of the streaming NHWC kernels (bn_elem.hip, upsample.hip): what one thread moves per access.
//   W = 1: one fp32 channel, W = 4: four fp32 channels (one float4), W = 8: eight bf16 channels (16 bytes).
// A kernel body is written once over ChanUnit<W, BF> -- fp32 values in registers, whatever the storage -- and is
// instantiated three times; chan_unit_width() picks the form of a launch and DFL_LAUNCH_UNIT dispatches on it.
#pragma once
#include <initializer_list>

#include "common.h"

namespace dfl {

// `base` is the tensor, `elem` the offset of the unit's first channel in elements (2 bytes for bf16, 4 for fp32).
template <int W, bool BF>
struct ChanUnit {
  static_assert(BF ? W == 8 : (W == 1 || W == 4), "units: 1 or 4 fp32 channels, 8 bf16 channels");

  static __device__ __forceinline__ void load(const void* base, int64_t elem, float* v) {
    if constexpr (BF) {
      unpack8(*reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned short*>(base) + elem), v);
    } else if constexpr (W == 4) {
      const float4 w = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + elem);
      v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
    } else {
      v[0] = reinterpret_cast<const float*>(base)[elem];
    }
  }

  // stored (optional, may be v itself): the values as they now stand in memory, i.e. after the bf16 rounding
  static __device__ __forceinline__ void store(void* base, int64_t elem, const float* v, float* stored = nullptr) {
    if constexpr (BF) {
      const u32x4 w = pack8(v);
      *reinterpret_cast<u32x4*>(reinterpret_cast<unsigned short*>(base) + elem) = w;
      if (stored != nullptr) unpack8(w, stored);
    } else {
      if constexpr (W == 4) *reinterpret_cast<float4*>(reinterpret_cast<float*>(base) + elem) = make_float4(v[0], v[1], v[2], v[3]);
      else reinterpret_cast<float*>(base)[elem] = v[0];
      if (stored != nullptr && stored != v) {
#pragma unroll
        for (int j = 0; j < W; ++j) stored[j] = v[j];
      }
    }
  }
};

// index i of a grid-stride loop over [N][H][W][cq units] -> unit, x, y, n
__device__ __forceinline__ void unit_coords(int64_t i, int cq, int W, int H, int* u, int* x, int* y, int* n) {
  *u = (int)(i % cq);
  int64_t pix = i / cq;
  *x = (int)(pix % W);
  pix /= W;
  *y = (int)(pix % H);
  *n = (int)(pix / H);
}

// ---- host side: which unit a launch takes
struct ChanOperand {
  const void* p;   // NULL: an optional tensor that is absent
  int64_t ld;      // its pixel stride in elements
};

// *W = 8 for bf16 tensors, which must qualify (C and every ld a multiple of 8, every pointer 16-byte aligned, and
// whatever else the caller folds into bf16_more_ok): the one place that refuses them.  fp32: 4 where the same holds with 4, else 1.
inline int chan_unit_width(const char* who, bool bf16, int C, std::initializer_list<ChanOperand> ops, int* W,
                           const char* strides = "ld", bool bf16_more_ok = true, const char* bf16_more = "") {
  const int w = bf16 ? 8 : 4;
  bool ok = C % w == 0;
  for (const ChanOperand& o : ops) ok = ok && (o.p == nullptr || (o.ld % w == 0 && aligned16(o.p)));
  DFL_REQUIRE(!bf16 || (ok && bf16_more_ok), "%s (bf16): C and %s must be multiples of 8, tensors 16-byte aligned%s", who, strides,
              bf16_more);
  *W = ok ? w : 1;
  return DFL_OK;
}

// one kernel body `kernel<W, BF>`, three instantiations, 256 threads
#define DFL_LAUNCH_UNIT(W, kernel, grid, stream, ...)                                                                  \
  do {                                                                                                                 \
    if ((W) == 8) hipLaunchKernelGGL((kernel<8, true>), grid, dim3(256), 0, static_cast<hipStream_t>(stream), __VA_ARGS__);      \
    else if ((W) == 4) hipLaunchKernelGGL((kernel<4, false>), grid, dim3(256), 0, static_cast<hipStream_t>(stream), __VA_ARGS__); \
    else hipLaunchKernelGGL((kernel<1, false>), grid, dim3(256), 0, static_cast<hipStream_t>(stream), __VA_ARGS__);              \
  } while (0)

}  // namespace dfl
