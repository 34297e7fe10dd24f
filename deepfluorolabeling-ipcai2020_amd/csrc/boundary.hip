// Boundary loss (include/dfl_hip.h, "Boundary loss"; restated in numpy by tests/boundary_ref.py): the
// signed distance maps phi of a batch of one-hot targets, and the term L_B = mean(seg * phi) with its gradient
// beta * phi / N, added onto the value and the gradient that dfl_dice_ncc_loss left in the same places.
//
// dfl_boundary_maps: arg-max -> uint8 labels; the exact EDT of labels_dist.hip (dfl_label_edt, boundary 0) over the pairs
// of label sets ({c}, every label < C but c), a chunk of (images, classes) at a time so that the two int32 planes per pair
// stay below MAP_CHUNK_BYTES; combine -> phi.  Rows throughout: a wave owns a row of an (image, class), a lane a pixel, so
// no index is divided per pixel and every wave access is one contiguous segment.
//
// dfl_boundary_loss: both stages stream rows of (image, class) planes -- wave k of the grid takes rows k, k + waves, ..; in
// a row pixel x belongs to a lane by the SHAPE alone (head pixels up to the first 16-byte boundary of the dense phi row, then
// quads of four, then the tail), whatever the alignment of seg / dseg, which only decides between one 16-byte access and
// four 4-byte ones.  So the order of the float64 sum depends on the launch shape alone (csrc/fixed_sum.h: wave shuffle,
// four waves through LDS, one record per workgroup, records in index order; no atomics).
#include "common.h"
#include "fixed_sum.h"

namespace dfl {
namespace {

constexpr int NT = 256, NW = NT / 64;
constexpr int NONE = DFL_LABEL_EDT_NONE;
constexpr int MAX_PAIRS = DFL_LABEL_MAX_CLASSES / 2;      // ({c}, not c) pairs per dfl_label_edt call: 2 * 15 <= 31 sets
constexpr int64_t MAP_CHUNK_BYTES = 256ll << 20;          // rowdist + dist2 of one chunk (a single pair may exceed it)
constexpr int ROW_GRID = 2048;                            // maps: workgroups at most (8 per CU), rows grid-strided
constexpr int LOSS_GRID = 1024;                           // loss: workgroups (= records of the sum) at most

int64_t align256(int64_t v) { return (v + 255) & ~255ll; }

// ---- stage 1 of the maps: labels[b][y][x] = argmax_c tseg[b][c][y][x], the first maximum (torch.max) -------------------
__global__ __launch_bounds__(NT) void bl_argmax_kernel(const float* __restrict__ tseg, int64_t sN, int64_t sC, int64_t sH,
                                                       unsigned char* __restrict__ labels, int C, int h, int w, int64_t rows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t r = (int64_t)blockIdx.x * NW + wave; r < rows; r += (int64_t)gridDim.x * NW) {
    const int64_t b = r / h;
    const int y = (int)(r - b * h);
    const float* row = tseg + b * sN + y * sH;
    unsigned char* out = labels + r * w;
    for (int x = lane; x < w; x += 64) {
      float best = row[x];
      int arg = 0;
      for (int c = 1; c < C; ++c) {
        const float v = row[c * sC + x];
        if (v > best) {
          best = v;
          arg = c;
        }
      }
      out[x] = (unsigned char)arg;
    }
  }
}

// ---- stage 3 of the maps: one chunk of Bc images x CK classes.  d2 = [Bc][2 CK][h w]: plane 2 j to the pixels of class
// c0 + j, plane 2 j + 1 to the pixels of every other class.  NONE in the plane a pixel reads: the class is absent from the
// image (outside pixel) or fills it (inside pixel): phi = +0.
__global__ __launch_bounds__(NT) void bl_combine_kernel(const unsigned char* __restrict__ labels, const int* __restrict__ d2,
                                                        float* __restrict__ phi, int C, int c0, int CK, int h, int w, int64_t rows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t hw = (int64_t)h * w;
  for (int64_t r = (int64_t)blockIdx.x * NW + wave; r < rows; r += (int64_t)gridDim.x * NW) {
    const int64_t bj = r / h;                 // (image of the chunk, class of the chunk)
    const int y = (int)(r - bj * h);
    const int64_t b = bj / CK;
    const int j = (int)(bj - b * CK);
    const int c = c0 + j;
    const unsigned char* lab = labels + b * hw + (int64_t)y * w;
    const int* to_in = d2 + (bj * 2) * hw + (int64_t)y * w;
    const int* to_out = to_in + hw;
    float* out = phi + (b * C + c) * hw + (int64_t)y * w;
    for (int x = lane; x < w; x += 64) {
      const bool inside = lab[x] == c;
      const int d = inside ? to_out[x] : to_in[x];
      float v = 0.f;
      if (d != NONE) v = inside ? (float)(1.0 - sqrt((double)d)) : (float)sqrt((double)d);
      out[x] = v;
    }
  }
}

// ---- the term -----------------------------------------------------------------------------------------------------------
// Row r of the B * C * h rows -> its three row pointers; bg: a row of the skipped background channel
struct Row {
  const float* seg;
  const float* phi;
  float* dseg;
  int head;          // pixels in front of the first 16-byte boundary of the phi row (phi itself is 16-byte aligned)
  bool bg;
};
__device__ __forceinline__ Row row_of(const dfl_boundary_loss_args& a, int64_t r) {
  const int64_t bc = r / a.h;
  const int y = (int)(r - bc * a.h);
  const int64_t b = bc / a.C;
  const int c = (int)(bc - b * a.C);
  Row o;
  o.seg = a.seg != nullptr ? a.seg + b * a.seg_sN + c * a.seg_sC + y * a.seg_sH : nullptr;
  o.phi = a.phi + r * a.w;
  const bool dense = a.dseg_sN == 0;
  o.dseg = a.dseg == nullptr ? nullptr : (dense ? a.dseg + r * a.w : a.dseg + b * a.dseg_sN + c * a.dseg_sC + y * a.dseg_sH);
  o.head = (int)((4 - ((r * a.w) & 3)) & 3);
  if (o.head > a.w) o.head = a.w;
  o.bg = a.skip_bg && c == 0;
  return o;
}
__device__ __forceinline__ bool at16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

__device__ __forceinline__ void load4(const float* p, bool vec, float* v) {
  if (vec) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
  }
}

// stage 1: sum of seg * phi over the rows of this workgroup's waves -> rec[blockIdx.x]
__global__ __launch_bounds__(NT) void bl_sum_kernel(const dfl_boundary_loss_args a, double* __restrict__ rec, int64_t rows) {
  __shared__ double lds[NW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool phi16 = at16(a.phi);
  double v[1] = {0.0};
  for (int64_t r = (int64_t)blockIdx.x * NW + wave; r < rows; r += (int64_t)gridDim.x * NW) {
    const Row o = row_of(a, r);
    if (o.bg) continue;                                  // (the same for the whole wave)
    const int nq = (a.w - o.head) >> 2, tail0 = o.head + 4 * nq;
    if (lane < o.head) v[0] += (double)o.seg[lane] * (double)o.phi[lane];
    const bool svec = at16(o.seg + o.head);
    for (int q = lane; q < nq; q += 64) {
      const int x = o.head + 4 * q;
      float s[4], p[4];
      load4(o.phi + x, phi16, p);
      load4(o.seg + x, svec, s);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[0] += (double)s[e] * (double)p[e];
    }
    if (tail0 + lane < a.w) v[0] += (double)o.seg[tail0 + lane] * (double)o.phi[tail0 + lane];
  }
  block_sum<1>(v, lds);
  if (threadIdx.x == 0) rec[blockIdx.x] = v[0];
}

// the records in index order, beta / N, one rounding to float: one thread adds; all threads fetch the records into LDS
// first, so that the adding thread does not wait for a global load per record
__global__ __launch_bounds__(NT) void bl_value_kernel(const dfl_boundary_loss_args a, const double* __restrict__ rec, int R) {
  __shared__ double rec_s[LOSS_GRID];
  for (int i = threadIdx.x; i < R; i += NT) rec_s[i] = rec[i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double N = (double)a.B * (double)(a.C - (a.skip_bg ? 1 : 0)) * (double)a.h * (double)a.w;
  const double term = (double)a.beta * (records_sum(rec_s, R, 1) / N);
  *a.loss = a.accumulate_loss ? (float)((double)*a.loss + term) : (float)term;
}

__device__ __forceinline__ float grad_elem(float k, float p, float old, bool acc) { return acc ? old + k * p : k * p; }

// stage 2: dseg (+)= k * phi, k = grad_scale * (float)(beta / N); a skipped background row: zeros, or left alone
__global__ __launch_bounds__(NT) void bl_grad_kernel(const dfl_boundary_loss_args a, int64_t rows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool phi16 = at16(a.phi), acc = a.accumulate_grad != 0;
  const double N = (double)a.B * (double)(a.C - (a.skip_bg ? 1 : 0)) * (double)a.h * (double)a.w;
  const float gs = a.grad_scale != nullptr ? *a.grad_scale : 1.f;
  const float k = gs * (float)((double)a.beta / N);
  for (int64_t r = (int64_t)blockIdx.x * NW + wave; r < rows; r += (int64_t)gridDim.x * NW) {
    const Row o = row_of(a, r);
    if (o.bg && acc) continue;                           // (the same for the whole wave)
    const float kr = o.bg ? 0.f : k;
    const int nq = (a.w - o.head) >> 2, tail0 = o.head + 4 * nq;
    if (lane < o.head) o.dseg[lane] = o.bg ? 0.f : grad_elem(kr, o.phi[lane], acc ? o.dseg[lane] : 0.f, acc);
    const bool dvec = at16(o.dseg + o.head);
    for (int q = lane; q < nq; q += 64) {
      const int x = o.head + 4 * q;
      float p[4], d[4] = {0.f, 0.f, 0.f, 0.f};
      if (o.bg) {
        p[0] = p[1] = p[2] = p[3] = 0.f;                 // (phi of a skipped channel may hold anything, inf included)
      } else {
        load4(o.phi + x, phi16, p);
      }
      if (acc) load4(o.dseg + x, dvec, d);
#pragma unroll
      for (int e = 0; e < 4; ++e) d[e] = grad_elem(kr, p[e], d[e], acc);
      if (dvec) {
        *reinterpret_cast<float4*>(o.dseg + x) = make_float4(d[0], d[1], d[2], d[3]);
      } else {
        o.dseg[x] = d[0]; o.dseg[x + 1] = d[1]; o.dseg[x + 2] = d[2]; o.dseg[x + 3] = d[3];
      }
    }
    const int xt = tail0 + lane;
    if (xt < a.w) o.dseg[xt] = o.bg ? 0.f : grad_elem(kr, o.phi[xt], acc ? o.dseg[xt] : 0.f, acc);
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
int check_shape(const char* who, int32_t B, int32_t C, int32_t h, int32_t w) {
  DFL_REQUIRE(B > 0 && h > 0 && w > 0, "%s: bad sizes B=%d h=%d w=%d", who, B, h, w);
  DFL_REQUIRE(C >= 2 && C <= DFL_LABEL_MAX_CLASSES, "%s: C = %d classes (2..%d)", who, C, DFL_LABEL_MAX_CLASSES);
  const int64_t far2 = (int64_t)(h - 1) * (h - 1) + (int64_t)(w - 1) * (w - 1);
  DFL_REQUIRE(far2 < (int64_t)NONE, "%s: (h-1)^2 + (w-1)^2 = %lld of %d x %d does not fit an int32 squared distance", who,
              (long long)far2, h, w);
  return DFL_OK;
}

// The chunks of the maps: Bc images x CK classes per dfl_label_edt call.  Bc * 2 CK * h w <= 2^25 words unless the chunk
// is a single (image, class), where 2 h w < 2^32: either way far inside the grid limits dfl_label_edt checks.
struct MapPlan {
  int64_t Bc, CK, labels_bytes, rowdist_bytes, dist2_bytes, total;
};
MapPlan map_plan(int64_t B, int64_t C, int64_t h, int64_t w) {
  MapPlan p;
  const int64_t hw = h * w;
  const int64_t per_pair = 2 * (2 * hw + 1) * 4;          // rowdist and dist2 of one (image, class): two sets each
  const int64_t pairs = MAP_CHUNK_BYTES / per_pair > 1 ? MAP_CHUNK_BYTES / per_pair : 1;
  const int64_t cmax = C < MAX_PAIRS ? C : MAX_PAIRS;
  if (pairs >= B) {
    p.Bc = B;
    p.CK = pairs / B < cmax ? pairs / B : cmax;
  } else {
    p.Bc = pairs;
    p.CK = 1;
  }
  const int64_t S = 2 * p.CK;
  p.labels_bytes = align256(B * hw);
  p.rowdist_bytes = align256(p.Bc * S * (hw + 1) * 4);
  p.dist2_bytes = align256(p.Bc * S * hw * 4);
  p.total = p.labels_bytes + p.rowdist_bytes + p.dist2_bytes;
  return p;
}

unsigned row_grid(int64_t rows, int cap) {
  const int64_t g = ceil_div(rows, NW);
  return (unsigned)(g < cap ? g : cap);
}

}  // namespace
}  // namespace dfl

using namespace dfl;

extern "C" int dfl_boundary_maps_scratch_bytes(int32_t B, int32_t C, int32_t h, int32_t w) {
  int rc = check_shape("dfl_boundary_maps_scratch_bytes", B, C, h, w);
  if (rc != DFL_OK) return rc;
  const MapPlan p = map_plan(B, C, h, w);
  DFL_REQUIRE(p.total < (1ll << 31), "dfl_boundary_maps_scratch_bytes: %d images of %d x %d need %lld bytes: more than an int holds", B,
              h, w, (long long)p.total);
  return (int)p.total;
}

extern "C" int dfl_boundary_maps(const float* tseg, int64_t sN, int64_t sC, int64_t sH, int32_t B, int32_t C, int32_t h, int32_t w,
                                 float* phi, void* scratch, dfl_stream_t stream) {
  int rc = check_shape("dfl_boundary_maps", B, C, h, w);
  if (rc != DFL_OK) return rc;
  const MapPlan p = map_plan(B, C, h, w);
  DFL_REQUIRE(p.total < (1ll << 31), "dfl_boundary_maps: %d images of %d x %d are too large for one call", B, h, w);
  DFL_REQUIRE(tseg && phi && scratch, "dfl_boundary_maps: missing pointer");
  DFL_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 15u) == 0, "dfl_boundary_maps: scratch is not 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t hw = (int64_t)h * w;
  unsigned char* labels = static_cast<unsigned char*>(scratch);
  int32_t* rowdist = reinterpret_cast<int32_t*>(labels + p.labels_bytes);
  int32_t* dist2 = reinterpret_cast<int32_t*>(labels + p.labels_bytes + p.rowdist_bytes);
  const int64_t lrows = (int64_t)B * h;
  hipLaunchKernelGGL(bl_argmax_kernel, dim3(row_grid(lrows, ROW_GRID)), dim3(NT), 0, st, tseg, sN, sC, sH, labels, (int)C, (int)h, (int)w,
                     lrows);
  if ((rc = check_launch("dfl_boundary_maps (arg-max)")) != DFL_OK) return rc;
  const uint32_t all = (uint32_t)((1ull << C) - 1ull);
  for (int64_t b0 = 0; b0 < B; b0 += p.Bc) {
    const int64_t Bc = B - b0 < p.Bc ? B - b0 : p.Bc;
    for (int64_t c0 = 0; c0 < C; c0 += p.CK) {
      const int64_t CK = C - c0 < p.CK ? C - c0 : p.CK;
      uint32_t sets[DFL_LABEL_MAX_CLASSES];
      for (int64_t j = 0; j < CK; ++j) {
        sets[2 * j] = 1u << (c0 + j);
        sets[2 * j + 1] = all & ~(1u << (c0 + j));
      }
      if ((rc = dfl_label_edt(labels + b0 * hw, (int32_t)Bc, h, w, sets, (int32_t)(2 * CK), 0, rowdist, dist2, stream)) != DFL_OK) return rc;
      const int64_t rows = Bc * CK * h;
      hipLaunchKernelGGL(bl_combine_kernel, dim3(row_grid(rows, ROW_GRID)), dim3(NT), 0, st, labels + b0 * hw, dist2,
                         phi + b0 * C * hw, (int)C, (int)c0, (int)CK, (int)h, (int)w, rows);
      if ((rc = check_launch("dfl_boundary_maps (combine)")) != DFL_OK) return rc;
    }
  }
  return DFL_OK;
}

extern "C" int dfl_boundary_loss_scratch_doubles(int32_t B, int32_t C, int32_t h) {
  if (B <= 0 || C <= 0 || h <= 0) return 0;
  return (int)row_grid((int64_t)B * C * h, LOSS_GRID);
}

extern "C" int dfl_boundary_loss(const dfl_boundary_loss_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a, "dfl_boundary_loss: missing argument block");
  int rc = check_shape("dfl_boundary_loss", a->B, a->C, a->h, a->w);
  if (rc != DFL_OK) return rc;
  DFL_REQUIRE(a->stage == 1 || a->stage == 2, "dfl_boundary_loss: stage %d (1: value, 2: gradient)", a->stage);
  DFL_REQUIRE(a->beta == a->beta && a->beta - a->beta == 0.f, "dfl_boundary_loss: beta is not finite");
  DFL_REQUIRE(a->phi && (a->stage == 1 ? (a->seg && a->loss && a->sums) : a->dseg != nullptr), "dfl_boundary_loss: missing pointer");
  DFL_REQUIRE((reinterpret_cast<uintptr_t>(a->phi) & 3u) == 0, "dfl_boundary_loss: phi is not 4-byte aligned");
  DFL_REQUIRE((a->dseg_sN == 0) == (a->dseg_sH == 0) && (a->dseg_sN == 0) == (a->dseg_sC == 0), "dfl_boundary_loss: give all gradient strides or none");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t rows = (int64_t)a->B * a->C * a->h;
  const unsigned grid = row_grid(rows, LOSS_GRID);
  if (a->stage == 1) {
    hipLaunchKernelGGL(bl_sum_kernel, dim3(grid), dim3(NT), 0, st, *a, a->sums, rows);
    if ((rc = check_launch("dfl_boundary_loss (sums)")) != DFL_OK) return rc;
    hipLaunchKernelGGL(bl_value_kernel, dim3(1), dim3(NT), 0, st, *a, a->sums, (int)grid);
    return check_launch("dfl_boundary_loss (value)");
  }
  hipLaunchKernelGGL(bl_grad_kernel, dim3(grid), dim3(NT), 0, st, *a, rows);
  return check_launch("dfl_boundary_loss (gradient)");
}
