// Result overlays on the device: the pixel work of the reference's overlay_est_ann.py / overlay_est_heat.py /
// examples_dataset/make_preproc_overlays.py -- min/max normalisation, 8-bit quantisation, segmentation tint, heat blend,
// yellow landmark markers -- for a batch of images, optionally tiled into one make_grid canvas.
// Contract: include/dfl_hip.h (dfl_overlay_args).  Two launches: per-image min / max partials (OVL_NB slices per image),
// then one pass per output pixel whose blocks first combine the partials of their image.  Markers are a per-pixel gather
// over the image's boxes staged in LDS (no scatter, no races).
// Built with -ffp-contract=off: every product and sum is rounded on its own, as torch's CPU ops round them.
// The min / max record, the colour of a pixel, the ellipse test and the canvas are overlay.h's, shared with overlay_fullres.hip.
#include "overlay.h"

namespace dfl {

__device__ __forceinline__ void ovl_block_minmax(float& mn, float& mx, float* red) {
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
    red[wave * 2] = mn;
    red[wave * 2 + 1] = mx;
  }
  __syncthreads();
  mn = fminf(fminf(red[0], red[2]), fminf(red[4], red[6]));
  mx = fmaxf(fmaxf(red[1], red[3]), fmaxf(red[5], red[7]));
}

// phase 1: grid (OVL_NB, B), 256 threads
__global__ void __launch_bounds__(256) ovl_minmax_kernel(const dfl_overlay_args a) {
  __shared__ float red[2][8];
  const int b = blockIdx.y;
  const int64_t hw = (int64_t)a.H * a.W;
  const float* img = a.image + (int64_t)b * a.H * a.ld_image;
  const float* heat = a.heat != nullptr ? a.heat + (int64_t)b * a.H * a.ld_heat : nullptr;
  float mn = INFINITY, mx = -INFINITY, hmn = INFINITY, hmx = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)OVL_NB * 256) {
    const int y = (int)(i / a.W), x = (int)(i - (int64_t)y * a.W);
    const float v = img[(int64_t)y * a.ld_image + x];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
    if (heat != nullptr) {
      const float h = heat[(int64_t)y * a.ld_heat + x];
      hmn = fminf(hmn, h);
      hmx = fmaxf(hmx, h);
    }
  }
  ovl_block_minmax(mn, mx, red[0]);
  ovl_block_minmax(hmn, hmx, red[1]);
  if (threadIdx.x == 0)
    reinterpret_cast<OvlSlice*>(a.scratch + (int64_t)b * DFL_OVERLAY_SCRATCH_FLOATS)[blockIdx.x] = OvlSlice{mn, mx, hmn, hmx};
}

// Pillow's box: float coordinates truncated toward zero; clamped far outside int range (such a box is never drawn)
template <typename T>
__device__ __forceinline__ int ovl_trunc(T v) {
  const T c = v < (T)-1e9 ? (T)-1e9 : (v > (T)1e9 ? (T)1e9 : v);
  return (int)c;
}

// (the full-resolution overlays build their boxes on the host under another visibility rule: overlay.fullres_marks)
template <typename T>
__device__ __forceinline__ bool ovl_box(const T* c, T r, const dfl_overlay_args& a, OvlBox& bx) {
  const T x = c[0], y = c[1];
  if (!isfinite(x) || !isfinite(y)) return false;
  const T fx0 = x - r, fy0 = y - r, fx1 = x + r, fy1 = y + r;    // rounded in T, as torch computes the box
  const int x0 = ovl_trunc(fx0), y0 = ovl_trunc(fy0), x1 = ovl_trunc(fx1), y1 = ovl_trunc(fy1);
  if (x1 < 0 || y1 < 0 || x0 >= a.W || y0 >= a.H) return false;
  const int w = x1 - x0, h = y1 - y0;
  if (w < 0 || h < 0 || w >= DFL_OVERLAY_STAMP_DIM || h >= DFL_OVERLAY_STAMP_DIM) return false;
  const int off = a.stamp_index[w * DFL_OVERLAY_STAMP_DIM + h];
  if (off < 0) return false;
  bx.x0 = x0;
  bx.y0 = y0;
  bx.w = w;
  bx.h = h;
  bx.off = off;
  return true;
}

// the padding of the grid canvas and its empty tiles: the pixels of three bands, numbered one after the other
__device__ void ovl_zero_padding(const dfl_overlay_args& a) {
  const int xmaps = ovl_xmaps(a.B), ymaps = (a.B + xmaps - 1) / xmaps;
  const int64_t Wc = ovl_canvas_ld(a.B, a.W);
  const int64_t th = a.H + OVL_PAD, tw = a.W + OVL_PAD;
  const int64_t nA = (int64_t)(ymaps + 1) * OVL_PAD * Wc;                  // full-width pad rows
  const int64_t perB = (int64_t)(xmaps + 1) * OVL_PAD;
  const int64_t nB = (int64_t)ymaps * a.H * perB;                          // pad columns beside the tile rows
  const int64_t hw = (int64_t)a.H * a.W;
  const int64_t nC = (int64_t)(xmaps * ymaps - a.B) * hw;                  // tiles past the last image
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nA + nB + nC; i += (int64_t)gridDim.x * 256) {
    int64_t r, c;
    if (i < nA) {
      const int64_t band = i / (OVL_PAD * Wc), rem = i - band * (OVL_PAD * Wc);
      r = band * th + rem / Wc;
      c = rem % Wc;
    } else if (i < nA + nB) {
      const int64_t j = i - nA, row = j / perB, cc = j - row * perB;
      r = (row / a.H) * th + OVL_PAD + row % a.H;
      c = (cc / OVL_PAD) * tw + cc % OVL_PAD;
    } else {
      const int64_t j = i - nA - nB, cell = a.B + j / hw, p = j % hw;
      r = (cell / xmaps) * th + OVL_PAD + p / a.W;
      c = (cell % xmaps) * tw + OVL_PAD + p % a.W;
    }
    unsigned char* o = a.out + (r * Wc + c) * 3;
    o[0] = 0;
    o[1] = 0;
    o[2] = 0;
  }
}

// phase 2: grid (gx, B [+1 padding row of blocks]), 256 threads
__global__ void __launch_bounds__(256) ovl_render_kernel(const dfl_overlay_args a) {
  __shared__ float red[4];
  __shared__ OvlBox boxes[DFL_OVERLAY_MAX_MARKERS];
  __shared__ int2 crosses[DFL_OVERLAY_MAX_MARKERS];
  __shared__ int n_box, n_cross;
  const int b = blockIdx.y;
  const bool grid = a.grid != 0 && a.B > 1;
  if (b == a.B) {                                        // (block-uniform) the canvas padding
    ovl_zero_padding(a);
    return;
  }
  // combine this image's min / max slices (one wave), stage its markers
  if (threadIdx.x < 64) ovl_combine(a.scratch, b, red);
  if (threadIdx.x == 0) {
    n_box = 0;
    n_cross = 0;
  }
  __syncthreads();
  for (int l = threadIdx.x; l < a.n_gt; l += 256) {
    OvlBox bx;
    bool ok;
    if (a.gt_f64)
      ok = ovl_box(static_cast<const double*>(a.gt_lands) + ((int64_t)b * a.n_gt + l) * 2, a.radius, a, bx);
    else
      ok = ovl_box(static_cast<const float*>(a.gt_lands) + ((int64_t)b * a.n_gt + l) * 2, (float)a.radius, a, bx);
    if (ok) boxes[atomicAdd(&n_box, 1)] = bx;
  }
  for (int l = threadIdx.x; l < a.n_est; l += 256) {
    const int2 c = make_int2(a.est_lands[((int64_t)b * a.n_est + l) * 2], a.est_lands[((int64_t)b * a.n_est + l) * 2 + 1]);
    if (c.x >= 0 && c.y >= 0 && c.x - a.cross < a.W && c.y - a.cross < a.H) crosses[atomicAdd(&n_cross, 1)] = c;
  }
  __syncthreads();
  const float mn = red[0], mx = red[1], d = mx - mn;
  const float hmn = red[2], hd = red[3] - red[2];
  const bool hdiv = hd > 1e-3f;
  const int nb = n_box, nc = n_cross;
  const int64_t hw = (int64_t)a.H * a.W;
  const float* img = a.image + (int64_t)b * a.H * a.ld_image;
  const unsigned char* lab = a.labels != nullptr ? a.labels + (int64_t)b * a.H * a.ld_labels : nullptr;
  const float* heat = a.heat != nullptr ? a.heat + (int64_t)b * a.H * a.ld_heat : nullptr;
  const int64_t Wc = grid ? ovl_canvas_ld(a.B, a.W) : a.W;
  const int64_t obase = grid ? ovl_tile_origin(b, a.B, a.H, a.W) : (int64_t)b * hw;   // the image's pixel (0, 0) in the output
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)gridDim.x * 256) {
    const int y = (int)(i / a.W), x = (int)(i - (int64_t)y * a.W);
    const float v = ovl_grey(img[(int64_t)y * a.ld_image + x], mn, d);
    float v0 = v, v1 = v, v2 = v;
    if (lab != nullptr) ovl_tint(v0, v1, v2, lab[(int64_t)y * a.ld_labels + x], a.n_tint, a.tint_scale, a.tint_add);
    if (heat != nullptr) {
      float h = heat[(int64_t)y * a.ld_heat + x] - hmn;
      if (hdiv) h = h / hd;
      const float k = 1.f - h;
      v0 = k * v0 + h * a.heat_color[0];
      v1 = k * v1 + h * a.heat_color[1];
      v2 = k * v2 + h * a.heat_color[2];
    }
    uint32_t r0 = ovl_quant(v0, a.quant), r1 = ovl_quant(v1, a.quant), r2 = ovl_quant(v2, a.quant);
    bool mark = ovl_in_stamps(boxes, nb, a.stamp_spans, x, y);
    for (int k = 0; k < nc && !mark; ++k) {
      const int2 c = crosses[k];
      mark = (x == c.x && abs(y - c.y) <= a.cross) || (y == c.y && abs(x - c.x) <= a.cross);
    }
    if (mark) {
      r0 = 255u;
      r1 = 255u;
      r2 = 0u;
    }
    unsigned char* o = a.out + (obase + (grid ? (int64_t)y * Wc + x : i)) * 3;
    o[0] = (unsigned char)r0;
    o[1] = (unsigned char)r1;
    o[2] = (unsigned char)r2;
  }
}

void ovl_launch_minmax(const dfl_overlay_args& a, hipStream_t s) {
  hipLaunchKernelGGL(ovl_minmax_kernel, dim3(OVL_NB, a.B), dim3(256), 0, s, a);
}

}  // namespace dfl

extern "C" int dfl_overlay_batch(const dfl_overlay_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_overlay_batch: null args");
  DFL_REQUIRE(a->B > 0 && a->B < 65535 && a->H > 0 && a->W > 0, "dfl_overlay_batch: bad sizes");
  DFL_REQUIRE(a->image != nullptr && a->out != nullptr && a->scratch != nullptr, "dfl_overlay_batch: image, out and scratch are required");
  DFL_REQUIRE(a->ld_image >= a->W && (a->labels == nullptr || a->ld_labels >= a->W) && (a->heat == nullptr || a->ld_heat >= a->W),
              "dfl_overlay_batch: a row stride is below W");
  DFL_REQUIRE((int64_t)a->H * a->W < (1ll << 31), "dfl_overlay_batch: image too large");
  DFL_REQUIRE(a->n_tint >= 0 && a->n_tint <= DFL_OVERLAY_MAX_COLORS && (a->n_tint == 0 || a->labels != nullptr),
              "dfl_overlay_batch: n_tint must be 0..%d and needs labels", DFL_OVERLAY_MAX_COLORS);
  DFL_REQUIRE(a->n_gt >= 0 && a->n_gt <= DFL_OVERLAY_MAX_MARKERS && a->n_est >= 0 && a->n_est <= DFL_OVERLAY_MAX_MARKERS,
              "dfl_overlay_batch: at most %d markers of each kind per image", DFL_OVERLAY_MAX_MARKERS);
  DFL_REQUIRE(a->n_gt == 0 || (a->gt_lands != nullptr && a->stamp_index != nullptr && a->stamp_spans != nullptr && a->radius >= 0.0),
              "dfl_overlay_batch: ellipse markers need centres, the stamp table and a radius >= 0");
  DFL_REQUIRE(a->n_est == 0 || (a->est_lands != nullptr && a->cross >= 0), "dfl_overlay_batch: crosses need centres and cross >= 0");
  DFL_REQUIRE(a->quant == DFL_OVERLAY_ROUND || a->quant == DFL_OVERLAY_TRUNC, "dfl_overlay_batch: bad quant");
  hipStream_t s = static_cast<hipStream_t>(stream);
  dfl::ovl_launch_minmax(*a, s);
  const int64_t hw = (int64_t)a->H * a->W;
  int64_t gx = dfl::ceil_div(hw, 256);
  const int64_t cap = 8192 / a->B > 4 ? 8192 / a->B : 4;
  if (gx > cap) gx = cap;
  const bool grid = a->grid != 0 && a->B > 1;
  hipLaunchKernelGGL(dfl::ovl_render_kernel, dim3((unsigned)gx, a->B + (grid ? 1 : 0)), dim3(256), 0, s, *a);
  return dfl::check_launch("dfl_overlay_batch");
}
