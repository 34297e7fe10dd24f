// Training files from the full-resolution dataset: crop, log-transform, 180-degree rotation and box reduction of the
// projections; the same reduction of the label maps by the most frequent label; and the inverse for labels.
// Contract: include/dfl_hip.h (dfl_preproc_projs_args, dfl_preproc_segs_args, dfl_restore_labels_args); the arithmetic
// is restated in numpy by tests/preproc_ref.py.
//
// Reductions: one thread owns one output pixel and reads its F x F box, F contiguous elements per row -- one load of
// up to 16 bytes per row and lane, and the 64 lanes of a wave read 64 * F contiguous elements of every row, so each
// cache line is fetched once.  F is a template parameter: the loads of a box are all issued before the first is used.
// Nothing is exchanged between lanes except the per-projection maximum, so there is no LDS and no barrier.  A rotated
// projection reverses the OUTPUT index: output (i, j) of a rotated image is the box that ends at cropped row
// Rc - i * F, read in ascending address order like any other.
// Box sums are fp64 (log2 of every pixel, added in fp64, scaled once): the mean of n equal values is that value, so
// a constant image comes out as exactly 0, and the rounding that is left is the logarithm's.
#include "common.h"

namespace dfl {

constexpr int PP_WAVES = 4;                 // waves per block: 64 output columns x 4 output rows (x PP_RPT rows each)
constexpr float PP_LN2 = 0.693147180559945309417f;

// output rows per thread: small boxes are a few bytes, so a thread takes several to keep enough loads in flight
template <int F> struct pp_rpt { static constexpr int value = F == 1 ? 8 : F == 2 ? 4 : F <= 4 ? 2 : 1; };

// rows / columns [lo, hi) of the crop window that output index i covers (rot: counted from the far end)
__device__ __forceinline__ void pp_span(int i, int f, int n, int rot, int& lo, int& hi) {
  const int a = i * f, b = min(a + f, n);
  lo = rot ? n - b : a;
  hi = rot ? n - a : b;
}

// K consecutive elements as fp32.  WIDE: the address is a multiple of 4 bytes -- one (or two) wide loads
template <typename T, int K, bool WIDE>
__device__ __forceinline__ void pp_load(const T* p, float (&v)[K]) {
  T raw[K];
  if (WIDE) {
    __builtin_memcpy(raw, __builtin_assume_aligned(p, 4), sizeof(raw));
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k) raw[k] = p[k];
  }
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = (float)raw[k];
}

// rows of a full box loaded together: at most 64 values wait in registers
template <int F> struct pp_rows { static constexpr int value = F * F <= 64 ? F : (64 / F > 0 ? 64 / F : 1); };

// Pass 1.  LOG: out = the box mean of log2(max(I, min_intensity)), and the bit pattern of the projection's largest
// max(I, min_intensity) into imax[n] (positive floats order like unsigned integers); else out = the box mean of I.
template <typename T, int F, bool WIDE, bool LOG>
__global__ __launch_bounds__(64 * PP_WAVES) void preproc_projs_kernel(const T* __restrict__ pixels, const int32_t* __restrict__ rot180,
                                                                     float* __restrict__ out, uint32_t* __restrict__ imax, int R,
                                                                     int C, int crop, int Ro, int Co, float min_i) {
  constexpr int RPT = pp_rpt<F>::value, RG = pp_rows<F>::value;
  const int n = blockIdx.z, Rc = R - 2 * crop, Cc = C - 2 * crop;
  const int rot = rot180[n] != 0;
  const int j = blockIdx.x * 64 + threadIdx.x;
  const T* img = pixels + (size_t)n * R * C;
  float* o = out + (size_t)n * Ro * Co;
  float vmax = 0.f;
  int c0 = 0, c1 = 0;
  if (j < Co) pp_span(j, F, Cc, rot, c0, c1);
#pragma unroll
  for (int t = 0; t < RPT; ++t) {
    const int i = (blockIdx.y * PP_WAVES + threadIdx.y) * RPT + t;
    if (i >= Ro || j >= Co) continue;
    int r0, r1;
    pp_span(i, F, Rc, rot, r0, r1);
    const T* p = img + (size_t)(crop + r0) * C + crop + c0;
    // the mean is the sum times the reciprocal of the count (a constant for a full box; only a clipped box divides):
    // within 2^-52 of the quotient, so the same fp32
    double sum = 0.0, inv = 1.0 / (F * F);
    if (r1 - r0 == F && c1 - c0 == F) {
#pragma unroll
      for (int g = 0; g < F; g += RG) {
        float v[RG][F];
#pragma unroll
        for (int r = 0; r < RG; ++r)
          if (g + r < F) pp_load<T, F, WIDE>(p + (size_t)(g + r) * C, v[r]);
#pragma unroll
        for (int r = 0; r < RG; ++r) {
          if (g + r >= F) continue;
#pragma unroll
          for (int c = 0; c < F; ++c) {
            float x = v[r][c];
            if (LOG) {
              x = fmaxf(x, min_i);
              vmax = fmaxf(vmax, x);
              x = log2f(x);
            }
            sum += (double)x;
          }
        }
      }
    } else {                                   // a clipped box of the bottom / right edge (top / left when rotated)
      inv = 1.0 / (double)((r1 - r0) * (c1 - c0));
      for (int r = 0; r < r1 - r0; ++r) {
        for (int c = 0; c < c1 - c0; ++c) {
          float x = (float)p[(size_t)r * C + c];
          if (LOG) {
            x = fmaxf(x, min_i);
            vmax = fmaxf(vmax, x);
            x = log2f(x);
          }
          sum += (double)x;
        }
      }
    }
    o[(size_t)i * Co + j] = (float)(sum * inv);
  }
  if (LOG) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, d, 64));
    // one atomic per wave, and none once the maximum on record is at least the wave's (a stale read only errs low)
    if (threadIdx.x == 0 && __float_as_uint(vmax) > __atomic_load_n(imax + n, __ATOMIC_RELAXED)) atomicMax(imax + n, __float_as_uint(vmax));
  }
}

// Pass 2 (log only), over the outputs in place: v = ln 2 * (log2(I0) - mean log2)
__global__ __launch_bounds__(256) void preproc_finish_kernel(float* __restrict__ out, const uint32_t* __restrict__ imax, int per_image) {
  const int n = blockIdx.y;
  const float l0 = log2f(__uint_as_float(imax[n]));
  float* o = out + (size_t)n * per_image;
  for (int k = blockIdx.x * 256 + threadIdx.x; k < per_image; k += gridDim.x * 256) o[k] = PP_LN2 * (l0 - o[k]);
}

// Sixteen 16-bit counters in four 64-bit registers.  Up to 15 labels at a time are counted as one-hot nibbles of one
// 64-bit word (add 1 << 4 * label), then spread into the 16-bit fields: no array is indexed with a run-time value.
struct PpCounts {
  uint64_t w[4] = {0, 0, 0, 0};
  uint64_t nib = 0;
  __device__ __forceinline__ void add(uint32_t label) { nib += 1ull << (4 * (label & 15u)); }
  __device__ __forceinline__ void flush() {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint64_t x = (nib >> (16 * q)) & 0xffffull;
      w[q] += (x & 0xfull) | ((x & 0xf0ull) << 12) | ((x & 0xf00ull) << 24) | ((x & 0xf000ull) << 36);
    }
    nib = 0;
  }
  // the most frequent label; of equally frequent ones the smallest
  __device__ __forceinline__ uint32_t argmax() const {
    uint32_t best = 0, arg = 0;
#pragma unroll
    for (int l = 0; l < 16; ++l) {
      const uint32_t c = (uint32_t)(w[l >> 2] >> (16 * (l & 3))) & 0xffffu;
      if (c > best) {
        best = c;
        arg = l;
      }
    }
    return arg;
  }
};

template <int F>
__global__ __launch_bounds__(64 * PP_WAVES) void preproc_segs_kernel(const unsigned char* __restrict__ segs, const int32_t* __restrict__ rot180,
                                                                    unsigned char* __restrict__ out, int32_t* __restrict__ status,
                                                                    int R, int C, int crop, int Ro, int Co) {
  constexpr int RPT = pp_rpt<F>::value;
  constexpr int HALF = F < 16 ? F : 8;         // labels counted between two flushes: at most 15
  const int n = blockIdx.z, Rc = R - 2 * crop, Cc = C - 2 * crop;
  const int rot = rot180[n] != 0;
  const int j = blockIdx.x * 64 + threadIdx.x;
  const unsigned char* img = segs + (size_t)n * R * C;
  unsigned char* o = out + (size_t)n * Ro * Co;
  uint32_t big = 0;
  int c0 = 0, c1 = 0;
  if (j < Co) pp_span(j, F, Cc, rot, c0, c1);
#pragma unroll
  for (int t = 0; t < RPT; ++t) {
    const int i = (blockIdx.y * PP_WAVES + threadIdx.y) * RPT + t;
    if (i >= Ro || j >= Co) continue;
    int r0, r1;
    pp_span(i, F, Rc, rot, r0, r1);
    const unsigned char* p = img + (size_t)(crop + r0) * C + crop + c0;
    PpCounts cnt;
    if (r1 - r0 == F && c1 - c0 == F) {
      unsigned char v[F][F];
#pragma unroll
      for (int r = 0; r < F; ++r) __builtin_memcpy(v[r], p + (size_t)r * C, F);   // any byte address: one or two wide loads
#pragma unroll
      for (int r = 0; r < F; ++r) {
#pragma unroll
        for (int c = 0; c < F; ++c) {
          big |= v[r][c];
          cnt.add(v[r][c]);
          if (c % HALF == HALF - 1) cnt.flush();
        }
      }
    } else {
      for (int r = 0; r < r1 - r0; ++r) {
        for (int c = 0; c < c1 - c0; ++c) {
          const uint32_t l = p[(size_t)r * C + c];
          big |= l;
          cnt.add(l);
          if ((c & 7) == 7) cnt.flush();
        }
        cnt.flush();
      }
    }
    o[(size_t)i * Co + j] = (unsigned char)cnt.argmax();
  }
  if (big > 15u) atomicOr(status, 1);          // a label above 15: the caller reports it
}

// Full-resolution pixel (r, c) takes the label of the box that contains it; the border of `crop` pixels is 0.
// One thread writes V consecutive columns of one row (V = 16: one 16-byte store).
template <int V>
__global__ __launch_bounds__(256) void restore_labels_kernel(const unsigned char* __restrict__ labels, const int32_t* __restrict__ rot180,
                                                             unsigned char* __restrict__ out, int R, int C, int crop, int f, int Ro,
                                                             int Co) {
  const int n = blockIdx.z, r = blockIdx.y, cb = (blockIdx.x * 256 + threadIdx.x) * V;
  if (cb >= C) return;
  const int Rc = R - 2 * crop, Cc = C - 2 * crop;
  const int rot = rot180[n] != 0;
  const int rr = r - crop;
  unsigned char v[V];
#pragma unroll
  for (int k = 0; k < V; ++k) v[k] = 0;
  if (rr >= 0 && rr < Rc) {
    const unsigned char* row = labels + ((size_t)n * Ro + (rot ? Rc - 1 - rr : rr) / f) * Co;
    // column of the rotated crop of the first pixel as box q and offset m (one division; `bias` boxes keep it
    // non-negative left of the window), then one step per pixel
    const int cc = cb - crop, bias = (crop + V) / f + 1;
    const int xb = (rot ? Cc - 1 - cc : cc) + bias * f;
    int q = xb / f - bias, m = xb % f;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      if (cc + k >= 0 && cc + k < Cc) v[k] = row[q];
      if (rot) {
        if (--m < 0) {
          m = f - 1;
          --q;
        }
      } else if (++m == f) {
        m = 0;
        ++q;
      }
    }
  }
  unsigned char* o = out + ((size_t)n * R + r) * C + cb;
  if (V == 16) {
    uint4 w;
    __builtin_memcpy(&w, v, 16);
    *reinterpret_cast<uint4*>(o) = w;
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k) o[k] = v[k];
  }
}

static int pp_check_geometry(const char* what, int N, int R, int C, int crop, int f) {
  DFL_REQUIRE(N >= 1 && R >= 1 && C >= 1 && crop >= 0, "%s: bad sizes (N %d, R %d, C %d, crop %d)", what, N, R, C, crop);
  DFL_REQUIRE(N <= 65535, "%s: at most 65535 images per call, got %d", what, N);
  DFL_REQUIRE(f >= 1 && f <= DFL_PREPROC_MAX_FACTOR, "%s: factor must be 1..%d, got %d", what, DFL_PREPROC_MAX_FACTOR, f);
  DFL_REQUIRE((int64_t)2 * crop < (R < C ? R : C), "%s: a crop of %d leaves nothing of %d x %d images", what, crop, R, C);
  DFL_REQUIRE((int64_t)R * C < ((int64_t)1 << 31), "%s: %d x %d images exceed 2^31 pixels", what, R, C);
  return DFL_OK;
}

static dim3 pp_grid(int N, int Ro, int Co, int rpt) {
  return dim3((unsigned)ceil_div(Co, 64), (unsigned)ceil_div(Ro, PP_WAVES * rpt), (unsigned)N);
}

template <int F>
static void pp_launch_projs(const dfl_preproc_projs_args* a, int Ro, int Co, hipStream_t s) {
  const dim3 grid = pp_grid(a->N, Ro, Co, pp_rpt<F>::value), block(64, PP_WAVES);
#define PP_GO(T, WIDE, LOG)                                                                                                 \
  preproc_projs_kernel<T, F, WIDE, LOG><<<grid, block, 0, s>>>(static_cast<const T*>(a->pixels), a->rot180, a->out, a->scratch, \
                                                               a->R, a->C, a->crop, Ro, Co, a->min_intensity)
  if (!a->u16) {
    if (a->log) PP_GO(float, true, true);
    else PP_GO(float, true, false);
    return;
  }
  // rows of the crop window start on 4-byte addresses when the pointer, the row pitch, the crop and the box are even
  const bool wide = (reinterpret_cast<uintptr_t>(a->pixels) & 3u) == 0 && a->C % 2 == 0 && a->crop % 2 == 0 && F % 2 == 0;
  if (wide) {
    if constexpr (F % 2 == 0) {               // (an odd box never starts every row on a 4-byte address)
      if (a->log) PP_GO(uint16_t, true, true);
      else PP_GO(uint16_t, true, false);
    }
  } else {
    if (a->log) PP_GO(uint16_t, false, true);
    else PP_GO(uint16_t, false, false);
  }
#undef PP_GO
}

template <int F>
static void pp_launch_segs(const dfl_preproc_segs_args* a, int Ro, int Co, hipStream_t s) {
  preproc_segs_kernel<F><<<pp_grid(a->N, Ro, Co, pp_rpt<F>::value), dim3(64, PP_WAVES), 0, s>>>(a->segs, a->rot180, a->out, a->status,
                                                                                               a->R, a->C, a->crop, Ro, Co);
}

#define PP_FOR_FACTOR(f, CALL)                                                                                  \
  switch (f) {                                                                                                  \
    case 1: CALL(1); break;   case 2: CALL(2); break;   case 3: CALL(3); break;   case 4: CALL(4); break;       \
    case 5: CALL(5); break;   case 6: CALL(6); break;   case 7: CALL(7); break;   case 8: CALL(8); break;       \
    case 9: CALL(9); break;   case 10: CALL(10); break; case 11: CALL(11); break; case 12: CALL(12); break;     \
    case 13: CALL(13); break; case 14: CALL(14); break; case 15: CALL(15); break; case 16: CALL(16); break;     \
  }

}  // namespace dfl

extern "C" int dfl_preproc_projs(const dfl_preproc_projs_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_preproc_projs: null args");
  DFL_REQUIRE(a->pixels != nullptr && a->rot180 != nullptr && a->out != nullptr, "dfl_preproc_projs: pixels, rot180 and out are required");
  if (dfl::pp_check_geometry("dfl_preproc_projs", a->N, a->R, a->C, a->crop, a->factor) != DFL_OK) return DFL_ERR_INVALID_ARG;
  DFL_REQUIRE(!a->log || a->scratch != nullptr, "dfl_preproc_projs: the log transform needs scratch (N words)");
  DFL_REQUIRE(!a->log || a->min_intensity > 0.f, "dfl_preproc_projs: min_intensity must be positive for the log transform, got %g",
              (double)a->min_intensity);
  DFL_REQUIRE(a->u16 || (reinterpret_cast<uintptr_t>(a->pixels) & 3u) == 0, "dfl_preproc_projs: fp32 pixels must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int f = a->factor, Rc = a->R - 2 * a->crop, Cc = a->C - 2 * a->crop;
  const int Ro = (Rc + f - 1) / f, Co = (Cc + f - 1) / f;
  if (a->log && hipMemsetAsync(a->scratch, 0, sizeof(uint32_t) * (size_t)a->N, s) != hipSuccess)
    return dfl::check_launch("dfl_preproc_projs (memset)");
#define PP_CALL(F) dfl::pp_launch_projs<F>(a, Ro, Co, s)
  PP_FOR_FACTOR(f, PP_CALL)
#undef PP_CALL
  int rc = dfl::check_launch("dfl_preproc_projs");
  if (rc != DFL_OK || !a->log) return rc;
  const int per_image = Ro * Co;
  const int bx = (int)(dfl::ceil_div(per_image, 256) < 64 ? dfl::ceil_div(per_image, 256) : 64);
  dfl::preproc_finish_kernel<<<dim3(bx, a->N), 256, 0, s>>>(a->out, a->scratch, per_image);
  return dfl::check_launch("dfl_preproc_projs (finish)");
}

extern "C" int dfl_preproc_segs(const dfl_preproc_segs_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_preproc_segs: null args");
  DFL_REQUIRE(a->segs != nullptr && a->rot180 != nullptr && a->out != nullptr && a->status != nullptr,
              "dfl_preproc_segs: segs, rot180, out and status are required");
  if (dfl::pp_check_geometry("dfl_preproc_segs", a->N, a->R, a->C, a->crop, a->factor) != DFL_OK) return DFL_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int f = a->factor, Rc = a->R - 2 * a->crop, Cc = a->C - 2 * a->crop;
  const int Ro = (Rc + f - 1) / f, Co = (Cc + f - 1) / f;
  if (hipMemsetAsync(a->status, 0, sizeof(int32_t), s) != hipSuccess) return dfl::check_launch("dfl_preproc_segs (memset)");
#define PP_CALL(F) dfl::pp_launch_segs<F>(a, Ro, Co, s)
  PP_FOR_FACTOR(f, PP_CALL)
#undef PP_CALL
  return dfl::check_launch("dfl_preproc_segs");
}

extern "C" int dfl_restore_labels(const dfl_restore_labels_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_restore_labels: null args");
  DFL_REQUIRE(a->labels != nullptr && a->rot180 != nullptr && a->out != nullptr, "dfl_restore_labels: labels, rot180 and out are required");
  if (dfl::pp_check_geometry("dfl_restore_labels", a->N, a->R, a->C, a->crop, a->factor) != DFL_OK) return DFL_ERR_INVALID_ARG;
  DFL_REQUIRE(a->R <= 65535, "dfl_restore_labels: at most 65535 rows, got %d", a->R);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int f = a->factor, Rc = a->R - 2 * a->crop, Cc = a->C - 2 * a->crop;
  const int Ro = (Rc + f - 1) / f, Co = (Cc + f - 1) / f;
  if (a->C % 16 == 0 && dfl::aligned16(a->out)) {
    dfl::restore_labels_kernel<16><<<dim3((unsigned)dfl::ceil_div(a->C, 16 * 256), a->R, a->N), 256, 0, s>>>(
        a->labels, a->rot180, a->out, a->R, a->C, a->crop, f, Ro, Co);
  } else {
    dfl::restore_labels_kernel<1><<<dim3((unsigned)dfl::ceil_div(a->C, 256), a->R, a->N), 256, 0, s>>>(
        a->labels, a->rot180, a->out, a->R, a->C, a->crop, f, Ro, Co);
  }
  return dfl::check_launch("dfl_restore_labels");
}
