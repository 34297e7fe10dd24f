// Bilinear x2 up-sampling of NHWC tensors and its adjoint -- up_mode='upsample' of the reference
// (train_test_code/unet.py:242-244: nn.Sequential(nn.Upsample(mode='bilinear', scale_factor=2), nn.Conv2d(in, out, 1))).
// The 1x1 convolution is pointwise and the interpolation weights of a pixel sum to one, so conv1x1(upsample(x)) =
// upsample(conv1x1(x)) with the bias added once: the plan runs the 1x1 convolution on the SMALL grid (a quarter of the
// products) and these kernels spread its result over the 2H x 2W grid, straight into the up half of the concat buffer.
//
// torch semantics (align_corners=False): source coordinate s = (o + 0.5) / 2 - 0.5, clamped at 0; i0 = floor(s),
// i1 = min(i0 + 1, n - 1); weights (1 - frac, frac).  I.e. output 2i takes (i-1: 0.25, i: 0.75), output 2i+1 takes
// (i: 0.75, i+1: 0.25), border rows / columns replicate.
//
// Both kernels stream: one thread per (pixel, 8 bf16 or 4 fp32 channels), 16-byte accesses, fp32 arithmetic.
#include "chan_unit.h"

namespace dfl {

__device__ __forceinline__ void up_coords(int o, int n, int* i0, int* i1, float* w0, float* w1) {
  float s = 0.5f * ((float)o + 0.5f) - 0.5f;
  if (s < 0.f) s = 0.f;
  const int a = (int)s;
  *i0 = a;
  *i1 = a < n - 1 ? a + 1 : a;
  *w1 = s - (float)a;
  *w0 = 1.f - *w1;
}

// VEC: channels per thread (the channel unit of chan_unit.h: 8 for bf16 tensors, 4 or 1 for fp32)
// y[n, oy, ox, c] = sum of the (up to) four source pixels of (oy, ox)
template <int VEC, bool BF>
__global__ void __launch_bounds__(256) upsample2x_fwd_kernel(const dfl_upsample_args a, int64_t total_units, int cq) {
  const int Ho = 2 * a.H, Wo = 2 * a.W;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total_units; i += stride) {
    int u, ox, oy, n;
    unit_coords(i, cq, Wo, Ho, &u, &ox, &oy, &n);
    const int c = u * VEC;
    int y0, y1, x0, x1;
    float wy0, wy1, wx0, wx1;
    up_coords(oy, a.H, &y0, &y1, &wy0, &wy1);
    up_coords(ox, a.W, &x0, &x1, &wx0, &wx1);
    const int64_t r0 = ((int64_t)n * a.H + y0) * a.W, r1 = ((int64_t)n * a.H + y1) * a.W;
    float v00[VEC], v01[VEC], v10[VEC], v11[VEC], o[VEC];
    ChanUnit<VEC, BF>::load(a.x, (r0 + x0) * a.ldx + c, v00);
    ChanUnit<VEC, BF>::load(a.x, (r0 + x1) * a.ldx + c, v01);
    ChanUnit<VEC, BF>::load(a.x, (r1 + x0) * a.ldx + c, v10);
    ChanUnit<VEC, BF>::load(a.x, (r1 + x1) * a.ldx + c, v11);
#pragma unroll
    for (int e = 0; e < VEC; ++e) o[e] = wy0 * (wx0 * v00[e] + wx1 * v01[e]) + wy1 * (wx0 * v10[e] + wx1 * v11[e]);
    ChanUnit<VEC, BF>::store(a.y, (((int64_t)n * Ho + oy) * Wo + ox) * a.ldy + c, o);
  }
}

// adjoint: x[n, iy, ix, c] (+)= sum over the outputs (oy, ox) that read (iy, ix) of their weight * y[n, oy, ox, c]
template <int VEC, bool BF>
__global__ void __launch_bounds__(256) upsample2x_bwd_kernel(const dfl_upsample_args a, int64_t total_units, int cq) {
  const int Ho = 2 * a.H, Wo = 2 * a.W;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total_units; i += stride) {
    int u, ix, iy, n;
    unit_coords(i, cq, a.W, a.H, &u, &ix, &iy, &n);
    const int c = u * VEC;
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    for (int oy = 2 * iy - 1; oy <= 2 * iy + 2; ++oy) {
      if (oy < 0 || oy >= Ho) continue;
      int y0, y1;
      float wy0, wy1;
      up_coords(oy, a.H, &y0, &y1, &wy0, &wy1);
      const float wy = (y0 == iy ? wy0 : 0.f) + (y1 == iy ? wy1 : 0.f);
      if (wy == 0.f) continue;
      for (int ox = 2 * ix - 1; ox <= 2 * ix + 2; ++ox) {
        if (ox < 0 || ox >= Wo) continue;
        int x0, x1;
        float wx0, wx1;
        up_coords(ox, a.W, &x0, &x1, &wx0, &wx1);
        const float w = wy * ((x0 == ix ? wx0 : 0.f) + (x1 == ix ? wx1 : 0.f));
        if (w == 0.f) continue;
        float v[VEC];
        ChanUnit<VEC, BF>::load(a.y, (((int64_t)n * Ho + oy) * Wo + ox) * a.ldy + c, v);
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = fmaf(w, v[e], acc[e]);
      }
    }
    const int64_t xo = (((int64_t)n * a.H + iy) * a.W + ix) * a.ldx + c;
    if (a.accumulate) {
      float o[VEC];
      ChanUnit<VEC, BF>::load(a.x, xo, o);
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[e] += o[e];
    }
    ChanUnit<VEC, BF>::store(const_cast<void*>(a.x), xo, acc);
  }
}

static unsigned up_grid(int64_t units) {
  int64_t b = ceil_div(units, 256);
  if (b > 8192) b = 8192;
  return (unsigned)(b < 1 ? 1 : b);
}

static int up_check(const dfl_upsample_args* a, const char* who, int* vec) {
  DFL_REQUIRE(a && a->x && a->y && a->N > 0 && a->H > 0 && a->W > 0 && a->C > 0, "%s: bad arguments", who);
  DFL_REQUIRE(a->ldx >= a->C && a->ldy >= a->C, "%s: pixel strides below the channel count", who);
  return chan_unit_width(who, a->bf16, a->C, {{a->x, a->ldx}, {a->y, a->ldy}}, vec, "pixel strides");
}

}  // namespace dfl

extern "C" int dfl_upsample2x_fwd(const dfl_upsample_args* a, dfl_stream_t stream) {
  int vec;
  const int rc = dfl::up_check(a, "dfl_upsample2x_fwd", &vec);
  if (rc != DFL_OK) return rc;
  const int cq = a->C / vec;
  const int64_t total = (int64_t)a->N * (2 * a->H) * (2 * a->W) * cq;
  DFL_LAUNCH_UNIT(vec, dfl::upsample2x_fwd_kernel, dim3(dfl::up_grid(total)), stream, *a, total, cq);
  return dfl::check_launch("dfl_upsample2x_fwd");
}

extern "C" int dfl_upsample2x_bwd(const dfl_upsample_args* a, dfl_stream_t stream) {
  int vec;
  const int rc = dfl::up_check(a, "dfl_upsample2x_bwd", &vec);
  if (rc != DFL_OK) return rc;
  const int cq = a->C / vec;
  const int64_t total = (int64_t)a->N * a->H * a->W * cq;
  DFL_LAUNCH_UNIT(vec, dfl::upsample2x_bwd_kernel, dim3(dfl::up_grid(total)), stream, *a, total, cq);
  return dfl::check_launch("dfl_upsample2x_bwd");
}
