// Cross-entropy / focal term on the soft-max probabilities (include/dfl_hip.h, "Cross-entropy and focal term"; DESIGN.md
// section 30; restated in numpy by tests/ce_ref.py):
//   f(s, t, w) = -w t (1 - s')^gamma log s',   s' = min(max(s, EPS), 1),   EPS = 2^-100,   0^0 = 1,
//   L_CE = (1 / N) sum f over every channel,   N = B h w (pixels),
// the value added onto what dfl_dice_ncc_loss (and dfl_boundary_loss) left in *loss, the gradient onto what they left in
// dseg.  Below EPS the gradient is still the formula at s' -- NOT the zero that the clamped value's true derivative would
// give: a confidently wrong pixel must keep its gradient.  1 / EPS = 2^100 times lambda / N stays finite in fp32, and the
// head backward multiplies by s, so the products it forms are O(1).
//
// An element with w_c t == 0 adds exactly +0, evaluates no logarithm, and in stage 2 is written as 0.0f (or, with
// accumulate_grad, left as it is: a group of four such elements is neither read nor written).  With one-hot targets that is
// C - 1 of C elements, so the accurate logf / powf run on one element in C and both stages stay streaming kernels.
//
// Both stages stream rows of (image, class) planes as csrc/boundary.hip does -- wave k of the grid takes rows k, k + waves,
// ..; in a row pixel x belongs to a lane by the SHAPE alone (head pixels up to the first multiple of four of the dense
// element index, then quads of four, then the tail), whatever the alignment of seg / tseg / dseg, which only decides between
// one 16-byte access and four 4-byte ones.  So the order of the float64 sum depends on the launch shape alone
// (csrc/fixed_sum.h: wave shuffle, four waves through LDS, one record per workgroup, records in index order; no atomics).
#include <math.h>

#include "common.h"
#include "fixed_sum.h"

namespace dfl {
namespace {

constexpr int NT = 256, NW = NT / 64;
constexpr int CE_GRID = 1024;                             // workgroups (= records of the sum) at most
constexpr float EPS = 0x1p-100f;

struct Row {
  const float* seg;
  const float* tseg;
  float* dseg;
  int head;          // pixels in front of the first multiple of four of the dense element index
  float wgt;         // class weight of the row
};
__device__ __forceinline__ Row row_of(const dfl_ce_loss_args& a, int64_t r) {
  const int64_t bc = r / a.h;
  const int y = (int)(r - bc * a.h);
  const int64_t b = bc / a.C;
  const int c = (int)(bc - b * a.C);
  Row o;
  o.seg = a.seg + b * a.seg_sN + c * a.seg_sC + y * a.seg_sH;
  o.tseg = a.tseg + b * a.tseg_sN + c * a.tseg_sC + y * a.tseg_sH;
  const bool dense = a.dseg_sN == 0;
  o.dseg = a.dseg == nullptr ? nullptr : (dense ? a.dseg + r * a.w : a.dseg + b * a.dseg_sN + c * a.dseg_sC + y * a.dseg_sH);
  o.head = (int)((4 - ((r * a.w) & 3)) & 3);
  if (o.head > a.w) o.head = a.w;
  o.wgt = a.class_wgt[c];
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

__device__ __forceinline__ float clamp_prob(float s) { return fminf(fmaxf(s, EPS), 1.f); }

// f / 1 of one element with wt = w_c t != 0: wt (1 - s')^gamma (-log s'), >= +0
template <bool FOCAL>
__device__ __forceinline__ float value_elem(float wt, float s, float gamma) {
  const float sc = clamp_prob(s);
  const float nl = -logf(sc);
  if (!FOCAL) return wt * nl;
  return wt * (powf(1.f - sc, gamma) * nl);
}

// d(k f) / ds of one element with kwt = k w_c t != 0:
//   -kwt [(1 - s')^gamma / s' - gamma (1 - s')^(gamma-1) log s'] = kwt (1 - s')^(gamma-1) [gamma log s' - (1 - s') / s']
// (both terms of the bracket are <= 0: nothing cancels; at s' = 1 the bracket is +0 - 0)
template <bool FOCAL>
__device__ __forceinline__ float grad_elem(float kwt, float s, float gamma) {
  const float sc = clamp_prob(s);
  if (!FOCAL) return -kwt / sc;
  const float om = 1.f - sc;
  const float br = gamma * logf(sc) - om / sc;
  return kwt * (powf(om, gamma - 1.f) * br);
}

// stage 1: the sum of f over the rows of this workgroup's waves -> rec[blockIdx.x]
template <bool FOCAL>
__global__ __launch_bounds__(NT) void ce_sum_kernel(const dfl_ce_loss_args a, double* __restrict__ rec, int64_t rows) {
  __shared__ double lds[NW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float gamma = a.gamma;
  double v[1] = {0.0};
  for (int64_t r = (int64_t)blockIdx.x * NW + wave; r < rows; r += (int64_t)gridDim.x * NW) {
    const Row o = row_of(a, r);
    if (o.wgt == 0.f) continue;                          // (the same for the whole wave)
    const int nq = (a.w - o.head) >> 2, tail0 = o.head + 4 * nq;
    if (lane < o.head) {
      const float t = o.tseg[lane];
      if (t != 0.f) v[0] += (double)value_elem<FOCAL>(o.wgt * t, o.seg[lane], gamma);
    }
    const bool svec = at16(o.seg + o.head), tvec = at16(o.tseg + o.head);
    for (int q = lane; q < nq; q += 64) {
      const int x = o.head + 4 * q;
      float s[4], t[4];
      load4(o.tseg + x, tvec, t);
      load4(o.seg + x, svec, s);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (t[e] != 0.f) v[0] += (double)value_elem<FOCAL>(o.wgt * t[e], s[e], gamma);
      }
    }
    const int xt = tail0 + lane;
    if (xt < a.w) {
      const float t = o.tseg[xt];
      if (t != 0.f) v[0] += (double)value_elem<FOCAL>(o.wgt * t, o.seg[xt], gamma);
    }
  }
  block_sum<1>(v, lds);
  if (threadIdx.x == 0) rec[blockIdx.x] = v[0];
}

// the records in index order, lambda / N, one rounding to float: one thread adds; all threads fetch the records into LDS
// first, so that the adding thread does not wait for a global load per record
__global__ __launch_bounds__(NT) void ce_value_kernel(const dfl_ce_loss_args a, const double* __restrict__ rec, int R) {
  __shared__ double rec_s[CE_GRID];
  for (int i = threadIdx.x; i < R; i += NT) rec_s[i] = rec[i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double N = (double)a.B * (double)a.h * (double)a.w;
  const double term = (double)a.lambda * (records_sum(rec_s, R, 1) / N);
  *a.loss = a.accumulate_loss ? (float)((double)*a.loss + term) : (float)term;
}

// stage 2: dseg (+)= d(k f) / ds, k = grad_scale * (float)(lambda / N); elements with w_c t == 0: zeros, or left alone
template <bool FOCAL>
__global__ __launch_bounds__(NT) void ce_grad_kernel(const dfl_ce_loss_args a, int64_t rows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool acc = a.accumulate_grad != 0;
  const float gamma = a.gamma;
  const double N = (double)a.B * (double)a.h * (double)a.w;
  const float gs = a.grad_scale != nullptr ? *a.grad_scale : 1.f;
  const float k = gs * (float)((double)a.lambda / N);
  for (int64_t r = (int64_t)blockIdx.x * NW + wave; r < rows; r += (int64_t)gridDim.x * NW) {
    const Row o = row_of(a, r);
    if (o.wgt == 0.f && acc) continue;                   // (the same for the whole wave)
    const bool off = o.wgt == 0.f;                       // a class of weight 0: a row of zeros, no target or seg is read
    const float kw = k * o.wgt;
    const int nq = (a.w - o.head) >> 2, tail0 = o.head + 4 * nq;
    if (lane < o.head) {
      const float t = off ? 0.f : o.tseg[lane];
      if (t != 0.f) {
        const float g = grad_elem<FOCAL>(kw * t, o.seg[lane], gamma);
        o.dseg[lane] = acc ? o.dseg[lane] + g : g;
      } else if (!acc) {
        o.dseg[lane] = 0.f;
      }
    }
    const bool svec = at16(o.seg + o.head), tvec = at16(o.tseg + o.head), dvec = at16(o.dseg + o.head);
    for (int q = lane; q < nq; q += 64) {
      const int x = o.head + 4 * q;
      float t[4] = {0.f, 0.f, 0.f, 0.f}, d[4] = {0.f, 0.f, 0.f, 0.f};
      if (!off) load4(o.tseg + x, tvec, t);
      const bool any = t[0] != 0.f || t[1] != 0.f || t[2] != 0.f || t[3] != 0.f;
      if (any) {
        float s[4];
        load4(o.seg + x, svec, s);
        if (acc) load4(o.dseg + x, dvec, d);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (t[e] != 0.f) d[e] += grad_elem<FOCAL>(kw * t[e], s[e], gamma);     // (without acc: 0.f + g = g)
        }
      } else if (acc) {
        continue;                                        // four elements left as they are
      }
      if (dvec) {
        *reinterpret_cast<float4*>(o.dseg + x) = make_float4(d[0], d[1], d[2], d[3]);
      } else {
        o.dseg[x] = d[0]; o.dseg[x + 1] = d[1]; o.dseg[x + 2] = d[2]; o.dseg[x + 3] = d[3];
      }
    }
    const int xt = tail0 + lane;
    if (xt < a.w) {
      const float t = off ? 0.f : o.tseg[xt];
      if (t != 0.f) {
        const float g = grad_elem<FOCAL>(kw * t, o.seg[xt], gamma);
        o.dseg[xt] = acc ? o.dseg[xt] + g : g;
      } else if (!acc) {
        o.dseg[xt] = 0.f;
      }
    }
  }
}

unsigned row_grid(int64_t rows) {
  const int64_t g = ceil_div(rows, NW);
  return (unsigned)(g < CE_GRID ? g : CE_GRID);
}

bool is_finite(float v) { return v - v == 0.f; }

}  // namespace
}  // namespace dfl

using namespace dfl;

extern "C" int dfl_ce_loss_scratch_doubles(int32_t B, int32_t C, int32_t h) {
  if (B <= 0 || C <= 0 || h <= 0) return 0;
  return (int)row_grid((int64_t)B * C * h);
}

extern "C" int dfl_ce_loss(const dfl_ce_loss_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a, "dfl_ce_loss: missing argument block");
  DFL_REQUIRE(a->B > 0 && a->h > 0 && a->w > 0, "dfl_ce_loss: bad sizes B=%d h=%d w=%d", a->B, a->h, a->w);
  DFL_REQUIRE(a->C >= 2 && a->C <= DFL_LABEL_MAX_CLASSES, "dfl_ce_loss: C = %d classes (2..%d)", a->C, DFL_LABEL_MAX_CLASSES);
  DFL_REQUIRE(a->stage == 1 || a->stage == 2, "dfl_ce_loss: stage %d (1: value, 2: gradient)", a->stage);
  DFL_REQUIRE(is_finite(a->lambda), "dfl_ce_loss: lambda is not finite");
  DFL_REQUIRE(is_finite(a->gamma), "dfl_ce_loss: gamma is not finite");
  DFL_REQUIRE(a->gamma == 0.f || (a->gamma >= 1.f && a->gamma <= 8.f), "dfl_ce_loss: gamma = %g (0, or 1..8)", (double)a->gamma);
  for (int c = 0; c < a->C; ++c)
    DFL_REQUIRE(is_finite(a->class_wgt[c]) && a->class_wgt[c] >= 0.f, "dfl_ce_loss: class_wgt[%d] is negative or not finite", c);
  DFL_REQUIRE(a->seg && a->tseg && (a->stage == 1 ? (a->loss && a->sums) : a->dseg != nullptr), "dfl_ce_loss: missing pointer (%s)",
              !a->seg ? "seg" : !a->tseg ? "tseg" : a->stage == 2 ? "dseg" : !a->loss ? "loss" : "sums");
  DFL_REQUIRE((a->dseg_sN == 0) == (a->dseg_sH == 0) && (a->dseg_sN == 0) == (a->dseg_sC == 0), "dfl_ce_loss: give all gradient strides (dseg_s*) or none");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t rows = (int64_t)a->B * a->C * a->h;
  const unsigned grid = row_grid(rows);
  const bool focal = a->gamma != 0.f;
  int rc;
  if (a->stage == 1) {
    if (focal) {
      hipLaunchKernelGGL(ce_sum_kernel<true>, dim3(grid), dim3(NT), 0, st, *a, a->sums, rows);
    } else {
      hipLaunchKernelGGL(ce_sum_kernel<false>, dim3(grid), dim3(NT), 0, st, *a, a->sums, rows);
    }
    if ((rc = check_launch("dfl_ce_loss (sums)")) != DFL_OK) return rc;
    hipLaunchKernelGGL(ce_value_kernel, dim3(1), dim3(NT), 0, st, *a, a->sums, (int)grid);
    return check_launch("dfl_ce_loss (value)");
  }
  if (focal) {
    hipLaunchKernelGGL(ce_grad_kernel<true>, dim3(grid), dim3(NT), 0, st, *a, rows);
  } else {
    hipLaunchKernelGGL(ce_grad_kernel<false>, dim3(grid), dim3(NT), 0, st, *a, rows);
  }
  return check_launch("dfl_ce_loss (gradient)");
}
