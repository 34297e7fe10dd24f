// What the two overlay renderers share (overlay.hip: dfl_overlay_batch; overlay_fullres.hip: dfl_fullres_overlay): the
// min / max record of an image, the colour of a pixel, the ellipse test and the make_grid canvas.  Contract: include/dfl_hip.h.
#pragma once
#include "common.h"
// every product and sum is rounded on its own, as torch's CPU ops round them: an FMA moves values across the 8-bit
// truncation boundaries.  The pragma is lexical, so it stands here and not only in the flags of the including sources.
#pragma clang fp contract(off)

namespace dfl {

// ---- the min / max record: OVL_NB slices per image at scratch + b * DFL_OVERLAY_SCRATCH_FLOATS -----------------------
struct OvlSlice {
  float mn, mx, hmn, hmx;           // image min, max; heat min, max (+-inf without a heat map)
};
constexpr int OVL_NB = 64;          // slices per image: one per lane of the wave that combines them
static_assert(OVL_NB * sizeof(OvlSlice) <= DFL_OVERLAY_SCRATCH_FLOATS * sizeof(float), "overlay scratch");

// per-image min / max slices of a.image (and a.heat) into a.scratch: the one launch of ovl_minmax_kernel (overlay.hip)
void ovl_launch_minmax(const dfl_overlay_args& a, hipStream_t s);

// the first wave of a block: image b's slices -> red[0..3] = image min, max, heat min, max (valid after a barrier)
__device__ __forceinline__ void ovl_combine(const float* scratch, int b, float* red) {
  static_assert(OVL_NB == 64, "one slice per lane");
  const OvlSlice p = reinterpret_cast<const OvlSlice*>(scratch + (int64_t)b * DFL_OVERLAY_SCRATCH_FLOATS)[threadIdx.x];
  float mn = p.mn, mx = p.mx, hmn = p.hmn, hmx = p.hmx;
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    hmn = fminf(hmn, __shfl_xor(hmn, o, 64));
    hmx = fmaxf(hmx, __shfl_xor(hmx, o, 64));
  }
  if (threadIdx.x == 0) {
    red[0] = mn;
    red[1] = mx;
    red[2] = hmn;
    red[3] = hmx;
  }
}

// ---- the colour of a pixel ------------------------------------------------------------------------------------------
// the 8-bit grey level of v in an image of minimum mn and range d = max - min, as a float in [0, 1]; d == 0: level 0
__device__ __forceinline__ float ovl_grey(float v, float mn, float d) {
  int g = 0;
  if (d != 0.f) {
    const float t = (v - mn) / d;
    g = (int)(t * 255.f);
  }
  return (float)g / 255.f;
}

// labels 1 .. n_tint are tinted; every other label leaves the pixel as it is
__device__ __forceinline__ void ovl_tint(float& v0, float& v1, float& v2, int l, int n_tint, float ts, const float (*tint_add)[3]) {
  if (l >= 1 && l <= n_tint) {
    v0 = ts * v0 + tint_add[l - 1][0];
    v1 = ts * v1 + tint_add[l - 1][1];
    v2 = ts * v2 + tint_add[l - 1][2];
  }
}

// a channel to 8 bits: DFL_OVERLAY_ROUND adds 0.5, then clamp and truncate (a constant quant folds in the caller)
__device__ __forceinline__ uint32_t ovl_quant(float v, int quant) {
  float q = v * 255.f;
  if (quant == DFL_OVERLAY_ROUND) q = q + 0.5f;
  return (uint32_t)fminf(fmaxf(q, 0.f), 255.f);
}

// ---- ellipses -------------------------------------------------------------------------------------------------------
struct OvlBox {
  int x0, y0, w, h, off;   // box corner, size (x1 - x0, y1 - y0), first row in stamp_spans
};

// does the filled ellipse of any of the nb boxes (LDS) cover pixel (x, y)?  spans: per box row, first | last << 16 column
__device__ __forceinline__ bool ovl_in_stamps(const OvlBox* boxes, int nb, const int32_t* spans, int x, int y) {
  bool mark = false;
  for (int k = 0; k < nb && !mark; ++k) {
    const OvlBox bx = boxes[k];
    const unsigned dx = (unsigned)(x - bx.x0), dy = (unsigned)(y - bx.y0);
    if (dx <= (unsigned)bx.w && dy <= (unsigned)bx.h) {
      const int s = spans[bx.off + (int)dy];
      mark = (int)dx >= (s & 0xffff) && (int)dx <= (s >> 16);
    }
  }
  return mark;
}

// ---- the make_grid(nrow = OVL_NROW, padding = OVL_PAD) canvas of n_tiles images of h x w (overlay.grid_shape) -------
constexpr int OVL_PAD = 2, OVL_NROW = 8;
__device__ __forceinline__ int ovl_xmaps(int n_tiles) { return n_tiles < OVL_NROW ? n_tiles : OVL_NROW; }
// pixels per canvas row
__device__ __forceinline__ int64_t ovl_canvas_ld(int n_tiles, int w) { return (int64_t)(w + OVL_PAD) * ovl_xmaps(n_tiles) + OVL_PAD; }
// pixel (0, 0) of tile k, in pixels from the canvas's first
__device__ __forceinline__ int64_t ovl_tile_origin(int k, int n_tiles, int h, int w) {
  const int xmaps = ovl_xmaps(n_tiles);
  return ((int64_t)(k / xmaps) * (h + OVL_PAD) + OVL_PAD) * ovl_canvas_ld(n_tiles, w) + (int64_t)(k % xmaps) * (w + OVL_PAD) + OVL_PAD;
}

}  // namespace dfl
