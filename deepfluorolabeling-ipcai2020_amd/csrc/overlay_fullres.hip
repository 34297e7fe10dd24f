// Full-resolution dataset overlays on the device: the pixel work of the reference's
// examples_dataset/make_full_res_overlays.py -- 180-degree rotation, grey level, segmentation tint, yellow landmark
// ellipses, anti-aliased text stamps -- fused with Pillow's 8-bit BILINEAR reduction, written as tiles of one make_grid
// canvas; and that reduction alone for uint8 RGB batches.
// Contract: include/dfl_hip.h (dfl_resample_plan, dfl_resample_args, dfl_fullres_args).
// Both kernels work on output tiles of RS_TR x RS_TW pixels.  A tile walks the input rows its vertical taps need,
// RS_RPI rows at a time: the full-resolution RGB pixels of those rows (only the columns its horizontal taps need) are
// produced into LDS -- read from memory for the plain resample, computed from image, labels, boxes and text masks for
// the overlay -- then reduced horizontally into a per-tile column buffer in LDS; the vertical pass reads that buffer.
// The full-resolution RGB image never reaches HBM; the rows shared by vertically adjacent tiles are computed twice.
// Built with -ffp-contract=off: the grey level and the tint round every product and sum as torch's CPU ops do.
// The pixel before the text is overlay.h's, shared with overlay.hip: grey level, tint, the TRUNC quantisation, ellipses.
#include "overlay.h"

namespace dfl {

constexpr int RS_TR = DFL_RESAMPLE_TILE_ROWS, RS_TW = DFL_RESAMPLE_TILE_COLS;
constexpr int RS_THREADS = 256;
constexpr int RS_RPI = RS_THREADS / RS_TW;   // input rows produced per step: one horizontal output per thread
constexpr int RS_PREC = 22;                  // Pillow's PRECISION_BITS for 8-bit images
static_assert(RS_THREADS % RS_TW == 0, "tile width");

__device__ __forceinline__ uint32_t rs_clip8(int s) {
  s >>= RS_PREC;
  return (uint32_t)(s < 0 ? 0 : (s > 255 ? 255 : s));
}

struct RsSpan {
  int ox0, ox1, oy0, oy1, cx0, cx1, ry0, ry1, ok;
};

// the input rows / columns the block's tile reads; ok == 0 when the tables ask for more than the plan's spans
__device__ void rs_span(const dfl_resample_plan& P, RsSpan& sp) {
  if (threadIdx.x == 0) {
    sp.ox0 = blockIdx.x * RS_TW;
    sp.oy0 = blockIdx.y * RS_TR;
    sp.ox1 = min(sp.ox0 + RS_TW, P.w_out);
    sp.oy1 = min(sp.oy0 + RS_TR, P.h_out);
    int c0 = P.w_in, c1 = 0, r0 = P.h_in, r1 = 0, ok = 1;
    for (int ox = sp.ox0; ox < sp.ox1; ++ox) {
      const int s = P.h_bounds[2 * ox], n = P.h_bounds[2 * ox + 1];
      ok &= (s >= 0 && n >= 1 && n <= P.kh && s + n <= P.w_in);
      c0 = min(c0, s);
      c1 = max(c1, s + n);
    }
    for (int oy = sp.oy0; oy < sp.oy1; ++oy) {
      const int s = P.v_bounds[2 * oy], n = P.v_bounds[2 * oy + 1];
      ok &= (s >= 0 && n >= 1 && n <= P.kv && s + n <= P.h_in);
      r0 = min(r0, s);
      r1 = max(r1, s + n);
    }
    ok &= (c1 - c0 <= P.span_cols && r1 - r0 <= P.span_rows);
    sp.cx0 = c0;
    sp.cx1 = c1;
    sp.ry0 = r0;
    sp.ry1 = r1;
    sp.ok = ok;
  }
  __syncthreads();
}

// one tile: src(y, x) gives the full-resolution pixel (r | g << 8 | b << 16); out points at output pixel (0, 0), rows
// ld pixels apart
template <class Src>
__device__ void rs_tile(const dfl_resample_plan& P, const RsSpan& sp, const Src& src, unsigned char* out, int64_t ld,
                        uint32_t* lds) {
  uint32_t* stage = lds;                                  // [RS_RPI][span_cols]
  uint32_t* hbuf = lds + RS_RPI * P.span_cols;            // [span_rows][RS_TW]
  const int tid = threadIdx.x, ncols = sp.cx1 - sp.cx0;
  const int hr = tid / RS_TW, hx = tid % RS_TW, hox = sp.ox0 + hx;
  int h_x0 = 0, h_n = 0;
  const int32_t* hk = nullptr;
  if (hox < sp.ox1) {
    h_x0 = P.h_bounds[2 * hox] - sp.cx0;
    h_n = P.h_bounds[2 * hox + 1];
    hk = P.h_coefs + (int64_t)hox * P.kh;
  }
  for (int r0 = sp.ry0; r0 < sp.ry1; r0 += RS_RPI) {
    for (int i = tid; i < RS_RPI * ncols; i += RS_THREADS) {
      const int rr = i / ncols, c = i - rr * ncols, y = r0 + rr;
      if (y < sp.ry1) stage[rr * P.span_cols + c] = src(y, sp.cx0 + c);
    }
    __syncthreads();
    const int y = r0 + hr;
    if (y < sp.ry1 && hk != nullptr) {
      const uint32_t* row = stage + hr * P.span_cols + h_x0;
      int s0 = 1 << (RS_PREC - 1), s1 = s0, s2 = s0;
      for (int j = 0; j < h_n; ++j) {
        const uint32_t p = row[j];
        const int w = hk[j];
        s0 += (int)(p & 255u) * w;
        s1 += (int)((p >> 8) & 255u) * w;
        s2 += (int)((p >> 16) & 255u) * w;
      }
      hbuf[(y - sp.ry0) * RS_TW + hx] = rs_clip8(s0) | rs_clip8(s1) << 8 | rs_clip8(s2) << 16;
    }
    __syncthreads();
  }
  for (int i = tid; i < RS_TR * RS_TW; i += RS_THREADS) {
    const int oy = sp.oy0 + i / RS_TW, xl = i % RS_TW, ox = sp.ox0 + xl;
    if (oy >= sp.oy1 || ox >= sp.ox1) continue;
    const int y0 = P.v_bounds[2 * oy] - sp.ry0, n = P.v_bounds[2 * oy + 1];
    const int32_t* vk = P.v_coefs + (int64_t)oy * P.kv;
    int s0 = 1 << (RS_PREC - 1), s1 = s0, s2 = s0;
    for (int j = 0; j < n; ++j) {
      const uint32_t p = hbuf[(y0 + j) * RS_TW + xl];
      const int w = vk[j];
      s0 += (int)(p & 255u) * w;
      s1 += (int)((p >> 8) & 255u) * w;
      s2 += (int)((p >> 16) & 255u) * w;
    }
    unsigned char* o = out + ((int64_t)oy * ld + ox) * 3;
    o[0] = (unsigned char)rs_clip8(s0);
    o[1] = (unsigned char)rs_clip8(s1);
    o[2] = (unsigned char)rs_clip8(s2);
  }
}

struct RsSrcU8 {
  const unsigned char* p;
  int W;
  __device__ uint32_t operator()(int y, int x) const {
    const unsigned char* q = p + ((int64_t)y * W + x) * 3;
    return (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16;
  }
};

// grid (ceil(w_out / RS_TW), ceil(h_out / RS_TR), B), RS_THREADS threads
__global__ void __launch_bounds__(RS_THREADS) rs_u8_kernel(const dfl_resample_args a) {
  extern __shared__ uint32_t lds[];
  __shared__ RsSpan sp;
  rs_span(a.plan, sp);
  if (!sp.ok) return;
  const int b = blockIdx.z;
  const RsSrcU8 src{a.in + (int64_t)b * a.plan.h_in * a.plan.w_in * 3, a.plan.w_in};
  rs_tile(a.plan, sp, src, a.out + (int64_t)b * a.plan.h_out * a.plan.w_out * 3, a.plan.w_out, lds);
}

struct FrSrc {
  const float* img;
  const unsigned char* lab;
  const int32_t* spans;
  const unsigned char* masks;
  const OvlBox* boxes;     // LDS
  const OvlBox* texts;     // LDS: x, y, w, h, first byte
  const float (*tint_add)[3];
  int H, W, rot, nb, nt, n_tint;
  float mn, d, ts;

  __device__ uint32_t operator()(int y, int x) const {
    const int sy = rot ? H - 1 - y : y, sx = rot ? W - 1 - x : x;
    const int64_t i = (int64_t)sy * W + sx;
    const float v = ovl_grey(img[i], mn, d);
    float v0 = v, v1 = v, v2 = v;
    ovl_tint(v0, v1, v2, lab[i], n_tint, ts, tint_add);
    uint32_t r0 = ovl_quant(v0, DFL_OVERLAY_TRUNC), r1 = ovl_quant(v1, DFL_OVERLAY_TRUNC), r2 = ovl_quant(v2, DFL_OVERLAY_TRUNC);
    if (ovl_in_stamps(boxes, nb, spans, x, y)) {
      r0 = 255u;
      r1 = 255u;
      r2 = 0u;
    }
    for (int k = 0; k < nt; ++k) {
      const OvlBox t = texts[k];
      const unsigned dx = (unsigned)(x - t.x0), dy = (unsigned)(y - t.y0);
      if (dx < (unsigned)t.w && dy < (unsigned)t.h) {
        const uint32_t m = masks[t.off + (int)dy * t.w + (int)dx], ink = 255u * m + 128u;
        uint32_t q;
        q = r0 * (255u - m) + ink;
        r0 = ((q >> 8) + q) >> 8;
        q = r1 * (255u - m) + ink;
        r1 = ((q >> 8) + q) >> 8;
        q = r2 * (255u - m) + ink;
        r2 = ((q >> 8) + q) >> 8;
      }
    }
    return r0 | r1 << 8 | r2 << 16;
  }
};

// grid (ceil(w_out / RS_TW), ceil(h_out / RS_TR), B), RS_THREADS threads
__global__ void __launch_bounds__(RS_THREADS) fr_render_kernel(const dfl_fullres_args a) {
  extern __shared__ uint32_t lds[];
  __shared__ RsSpan sp;
  __shared__ float red[4];                               // image min, max (and the heat pair, which nobody reads here)
  __shared__ OvlBox boxes[DFL_FULLRES_MAX_BOXES];
  __shared__ OvlBox texts[DFL_FULLRES_MAX_TEXTS];
  __shared__ int n_box, n_text;
  const int b = blockIdx.z;
  rs_span(a.plan, sp);
  if (!sp.ok) return;
  if (threadIdx.x < 64) ovl_combine(a.scratch, b, red);  // this image's min / max slices (one wave)
  if (threadIdx.x == 0) {
    n_box = 0;
    n_text = 0;
    for (int k = 0; k < DFL_FULLRES_MAX_TEXTS; ++k) {    // in order: later text blends over earlier text
      const int32_t* t = a.texts + ((int64_t)b * DFL_FULLRES_MAX_TEXTS + k) * 3;
      const int id = t[2];
      if (id < 0 || id >= a.n_text_stamps) continue;
      const int32_t* st = a.text_stamps + id * 3;
      OvlBox tx{t[0], t[1], st[0], st[1], st[2]};
      if (tx.w <= 0 || tx.h <= 0 || tx.x0 >= sp.cx1 || tx.y0 >= sp.ry1 || tx.x0 + tx.w <= sp.cx0 || tx.y0 + tx.h <= sp.ry0)
        continue;
      texts[n_text++] = tx;
    }
  }
  __syncthreads();
  // the ellipses that reach this tile's input span
  const int nbx = min(max(a.n_boxes[b], 0), DFL_FULLRES_MAX_BOXES);
  for (int k = threadIdx.x; k < nbx; k += RS_THREADS) {
    const int32_t* p = a.boxes + ((int64_t)b * DFL_FULLRES_MAX_BOXES + k) * 5;
    const OvlBox bx{p[0], p[1], p[2], p[3], p[4]};
    if (bx.w < 0 || bx.h < 0 || bx.off < 0 || bx.off + bx.h >= a.n_stamp_spans) continue;
    if (bx.x0 >= sp.cx1 || bx.y0 >= sp.ry1 || bx.x0 + bx.w < sp.cx0 || bx.y0 + bx.h < sp.ry0) continue;
    boxes[atomicAdd(&n_box, 1)] = bx;
  }
  __syncthreads();
  FrSrc src;
  src.img = a.image + (int64_t)b * a.H * a.W;
  src.lab = a.labels + (int64_t)b * a.H * a.W;
  src.spans = a.stamp_spans;
  src.masks = a.text_masks;
  src.boxes = boxes;
  src.texts = texts;
  src.tint_add = a.tint_add;
  src.H = a.H;
  src.W = a.W;
  src.rot = a.rot180[b] != 0;
  src.nb = n_box;
  src.nt = n_text;
  src.n_tint = a.n_tint;
  src.mn = red[0];
  src.d = red[1] - red[0];
  src.ts = a.tint_scale;
  // tile (tile0 + b) of the make_grid canvas
  const int k = a.tile0 + b, ho = a.plan.h_out, wo = a.plan.w_out;
  const bool grid = a.n_tiles > 1;                       // a single image is the canvas
  const int64_t ld = grid ? ovl_canvas_ld(a.n_tiles, wo) : wo, base = grid ? ovl_tile_origin(k, a.n_tiles, ho, wo) : 0;
  rs_tile(a.plan, sp, src, a.out + base * 3, ld, lds);
}

static int check_plan(const dfl_resample_plan& p, const char* what, size_t& lds) {
  DFL_REQUIRE(p.h_bounds != nullptr && p.h_coefs != nullptr && p.v_bounds != nullptr && p.v_coefs != nullptr,
              "%s: the resample plan's tables are required", what);
  DFL_REQUIRE(p.h_in > 0 && p.w_in > 0 && p.h_out > 0 && p.w_out > 0 && p.kh > 0 && p.kv > 0, "%s: bad plan sizes", what);
  DFL_REQUIRE(p.h_out < 65535 * RS_TR && p.span_rows > 0 && p.span_cols > 0 && p.span_rows <= p.h_in && p.span_cols <= p.w_in,
              "%s: bad plan spans", what);
  lds = 4 * ((size_t)RS_RPI * p.span_cols + (size_t)RS_TW * p.span_rows);
  DFL_REQUIRE(lds <= DFL_RESAMPLE_MAX_LDS, "%s: a tile needs %zu bytes of LDS (> %d): reduction too strong", what, lds,
              DFL_RESAMPLE_MAX_LDS);
  return 0;
}

}  // namespace dfl

extern "C" int dfl_resample_bilinear_u8(const dfl_resample_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_resample_bilinear_u8: null args");
  DFL_REQUIRE(a->in != nullptr && a->out != nullptr, "dfl_resample_bilinear_u8: in and out are required");
  DFL_REQUIRE(a->B > 0 && a->B < 65535, "dfl_resample_bilinear_u8: bad batch");
  size_t lds = 0;
  if (dfl::check_plan(a->plan, "dfl_resample_bilinear_u8", lds) != 0) return DFL_ERR_INVALID_ARG;
  const dim3 grid((unsigned)dfl::ceil_div(a->plan.w_out, dfl::RS_TW), (unsigned)dfl::ceil_div(a->plan.h_out, dfl::RS_TR), a->B);
  hipLaunchKernelGGL(dfl::rs_u8_kernel, grid, dim3(dfl::RS_THREADS), lds, static_cast<hipStream_t>(stream), *a);
  return dfl::check_launch("dfl_resample_bilinear_u8");
}

extern "C" int dfl_fullres_overlay(const dfl_fullres_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_fullres_overlay: null args");
  DFL_REQUIRE(a->image != nullptr && a->labels != nullptr && a->rot180 != nullptr && a->boxes != nullptr &&
                  a->n_boxes != nullptr && a->texts != nullptr && a->scratch != nullptr && a->out != nullptr,
              "dfl_fullres_overlay: image, labels, rot180, boxes, n_boxes, texts, scratch and out are required");
  DFL_REQUIRE(a->B > 0 && a->B < 65535 && a->H > 0 && a->W > 0 && (int64_t)a->H * a->W < (1ll << 31),
              "dfl_fullres_overlay: bad sizes");
  DFL_REQUIRE(a->plan.h_in == a->H && a->plan.w_in == a->W, "dfl_fullres_overlay: the plan is for %d x %d, images are %d x %d",
              a->plan.h_in, a->plan.w_in, a->H, a->W);
  DFL_REQUIRE(a->n_tint >= 0 && a->n_tint <= DFL_OVERLAY_MAX_COLORS, "dfl_fullres_overlay: n_tint must be 0..%d",
              DFL_OVERLAY_MAX_COLORS);
  DFL_REQUIRE(a->n_stamp_spans >= 0 && (a->n_stamp_spans == 0 || a->stamp_spans != nullptr),
              "dfl_fullres_overlay: ellipse stamps missing");
  DFL_REQUIRE(a->n_text_stamps >= 0 && (a->n_text_stamps == 0 || (a->text_stamps != nullptr && a->text_masks != nullptr)),
              "dfl_fullres_overlay: text stamps missing");
  DFL_REQUIRE(a->n_tiles >= 1 && a->tile0 >= 0 && a->tile0 + a->B <= a->n_tiles,
              "dfl_fullres_overlay: images %d..%d are not tiles of a %d-tile canvas", a->tile0, a->tile0 + a->B - 1, a->n_tiles);
  size_t lds = 0;
  if (dfl::check_plan(a->plan, "dfl_fullres_overlay", lds) != 0) return DFL_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  dfl_overlay_args mm = {};
  mm.image = a->image;
  mm.scratch = a->scratch;
  mm.B = a->B;
  mm.H = a->H;
  mm.W = a->W;
  mm.ld_image = a->W;
  dfl::ovl_launch_minmax(mm, s);
  const dim3 grid((unsigned)dfl::ceil_div(a->plan.w_out, dfl::RS_TW), (unsigned)dfl::ceil_div(a->plan.h_out, dfl::RS_TR), a->B);
  hipLaunchKernelGGL(dfl::fr_render_kernel, grid, dim3(dfl::RS_THREADS), lds, s, *a);
  return dfl::check_launch("dfl_fullres_overlay");
}
