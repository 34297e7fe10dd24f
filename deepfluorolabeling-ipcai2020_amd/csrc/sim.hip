// Batched gradient-NCC between V rendered views and one fixed image: the similarity of dfl_amd.register.
// Contract: include/dfl_hip.h (dfl_sim_prepare_args, dfl_sim_gradncc_args); the semantics are stated in DESIGN.md
// section 16 and restated in numpy float64 by tests/reg_ref.py.
//
// dfl_sim_prepare (once per fixed image): one workgroup writes the Sobel planes of the fixed image, the counted-pixel
// plane and the five fixed-only totals.  dfl_sim_gradncc (once per generation): a workgroup owns SIM_ROWS interior rows
// of one view (grid = bands x views); thread t takes the pixels t, t + 256, ... of its band in that order, reads the
// eight neighbours of the moving image straight from global memory (consecutive lanes read consecutive columns; a
// batch of 32 views of 180 x 180 is 4 MB and stays in L2, and a row is re-read by its two neighbouring rows out of
// the vector L1) and adds six sums in float64.  Wave shuffles, then LDS across the four waves, then ONE record of six
// doubles per workgroup with plain stores; sim_finish_kernel adds a view's records in index order and writes its cost
// (csrc/fixed_sum.h: block_sum, records_sum).  The sums of a pixel, Sobel and the NCC are csrc/sim.h's.
// No atomics: the bits of a view's cost depend on that view's pixels and on H and W only.
// The *_bank_* entry points launch the same kernels with fixed_of [V] and F: view v then reads the
// planes and totals of image fixed_of[v] of a bank (sim_image_of, csrc/sim.h); the single-image entry points pass
// fixed_of = nullptr and every view reads image 0.
#include "sim.h"

namespace dfl {

constexpr int SIM_ROWS = 8;          // interior rows per workgroup

__global__ __launch_bounds__(SIM_THREADS) void sim_prepare_kernel(const float* __restrict__ fixed, const unsigned char* __restrict__ mask,
                                                                  float* __restrict__ fx, float* __restrict__ fy,
                                                                  unsigned char* __restrict__ counted, double* __restrict__ totals,
                                                                  int H, int W) {
  __shared__ double lds[SIM_FIXED * 4];
  double s[SIM_FIXED] = {0.0, 0.0, 0.0, 0.0, 0.0};
  const int64_t n = (int64_t)H * W;
  for (int64_t p = threadIdx.x; p < n; p += SIM_THREADS) {
    const int r = (int)(p / W), c = (int)(p - (int64_t)r * W);
    float gx = 0.f, gy = 0.f;
    unsigned char on = 0;
    if (r >= 1 && r <= H - 2 && c >= 1 && c <= W - 2) {
      sim_sobel(fixed, W, r, c, gx, gy);
      on = 1;
      if (mask != nullptr) {
#pragma unroll
        for (int dr = -1; dr <= 1; ++dr)
#pragma unroll
          for (int dc = -1; dc <= 1; ++dc)
            if (mask[(size_t)(r + dr) * W + (c + dc)] == 0) on = 0;
      }
    }
    fx[p] = gx;
    fy[p] = gy;
    counted[p] = on;
    if (on) sim_fixed_sums(s, gx, gy);
  }
  block_sum<SIM_FIXED>(s, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < SIM_FIXED; ++k) totals[k] = s[k];
  }
}

__global__ __launch_bounds__(SIM_THREADS) void sim_gradncc_kernel(const float* __restrict__ moving, const float* __restrict__ fx,
                                                                  const float* __restrict__ fy, const unsigned char* __restrict__ counted,
                                                                  const int32_t* __restrict__ fixed_of, double* __restrict__ scratch,
                                                                  int H, int W, int F) {
  __shared__ double lds[SIM_MOVING * 4];
  const int band = blockIdx.x, view = blockIdx.y;
  const int f = sim_image_of(fixed_of, view, F);
  sim_planes_of(fx, fy, counted, f < 0 ? 0 : f, H, W);                   // f < 0: the loop below has no pixel
  const int r0 = 1 + band * SIM_ROWS;                                   // first interior row of the band
  const int rows = min(SIM_ROWS, H - 1 - r0);                           // interior rows are 1 .. H - 2
  const int wi = W - 2;
  const float* img = moving + (size_t)view * H * W;
  double s[SIM_MOVING] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const int pixels = f < 0 ? 0 : rows * wi;
  for (int p = threadIdx.x; p < pixels; p += SIM_THREADS) {
    const int r = r0 + p / wi, c = 1 + p % wi;
    if (counted[(size_t)r * W + c]) sim_moving_sums(s, img, fx, fy, W, r, c);
  }
  block_sum<SIM_MOVING>(s, lds);
  if (threadIdx.x == 0) {
    double* rec = scratch + ((size_t)view * gridDim.x + band) * SIM_MOVING;
#pragma unroll
    for (int k = 0; k < SIM_MOVING; ++k) rec[k] = s[k];
  }
}

// One wave per view: lanes 0..5 add one of the six sums each over the view's records, in index order
__global__ __launch_bounds__(64) void sim_finish_kernel(const double* __restrict__ scratch, const double* __restrict__ totals,
                                                        const int32_t* __restrict__ fixed_of, double* __restrict__ cost, int bands,
                                                        int F) {
  __shared__ double m[SIM_MOVING];
  const int view = blockIdx.x;
  const int f = sim_image_of(fixed_of, view, F);
  if (f < 0) {                                                          // the whole workgroup: no barrier is left waiting
    if (threadIdx.x == 0) cost[view] = __builtin_nan("");
    return;
  }
  totals += (size_t)f * SIM_FIXED;
  if (threadIdx.x < SIM_MOVING) m[threadIdx.x] = records_sum(scratch + (size_t)view * bands * SIM_MOVING + threadIdx.x, bands, SIM_MOVING);
  __syncthreads();
  if (threadIdx.x == 0) {
    const double n = totals[0];
    double c = 1.0;
    if (n >= 1.0)
      c = 1.0 - 0.5 * (sim_ncc(n, m[0], m[1], totals[1], totals[2], m[2]) + sim_ncc(n, m[3], m[4], totals[3], totals[4], m[5]));
    cost[view] = c;
  }
}

inline int sim_bands(int H) { return (int)ceil_div(H - 2, SIM_ROWS); }

// ---- the adjoint: d cost[v] / d moving[v][r][c] (dfl_sim_gradncc_bwd) ----------------------------------------------------------
constexpr int SIM_COEF = 8;          // per view: alpha, beta, mean a, mean b of x, then of y (float32; sim_coef4, csrc/sim.h)

// One thread per view: the view's records added in index order (as sim_finish_kernel adds them), the coefficients in float64
__global__ __launch_bounds__(64) void sim_coef_kernel(const double* __restrict__ scratch, const double* __restrict__ totals,
                                                      const int32_t* __restrict__ fixed_of, float* __restrict__ coef, int bands, int V,
                                                      int F) {
  const int view = blockIdx.x * 64 + threadIdx.x;
  if (view >= V) return;
  const int f = sim_image_of(fixed_of, view, F);
  if (f < 0) {                                                          // sim_adjoint_kernel writes zeros and reads none of these
    for (int k = 0; k < SIM_COEF; ++k) coef[(size_t)view * SIM_COEF + k] = 0.f;
    return;
  }
  totals += (size_t)f * SIM_FIXED;
  double m[SIM_MOVING];
#pragma unroll
  for (int k = 0; k < SIM_MOVING; ++k) m[k] = records_sum(scratch + (size_t)view * bands * SIM_MOVING + k, bands, SIM_MOVING);
  const double n = totals[0];
#pragma unroll
  for (int dir = 0; dir < 2; ++dir) {
    float* out = coef + (size_t)view * SIM_COEF + 4 * dir;
    if (n >= 1.0)
      sim_coef4(out, 1.0, n, m[3 * dir], m[3 * dir + 1], totals[1 + 2 * dir], totals[2 + 2 * dir], m[3 * dir + 2]);
    else
      out[0] = out[1] = out[2] = out[3] = 0.f;
  }
}

// sim_adjoint_tile (csrc/sim.h) with the g of one correlation over the whole image: the view's eight coefficients
__global__ __launch_bounds__(SIM_THREADS) void sim_adjoint_kernel(const float* __restrict__ moving, const float* __restrict__ fx,
                                                                  const float* __restrict__ fy, const unsigned char* __restrict__ counted,
                                                                  const int32_t* __restrict__ fixed_of, const float* __restrict__ coef,
                                                                  float* __restrict__ d_moving, int H, int W, int F) {
  // every product is rounded on its own: where moving matches fixed the two terms of g cancel exactly, which an FMA would undo
#pragma clang fp contract(off)
  const float* cf = coef + (size_t)blockIdx.z * SIM_COEF;              // zeros for a view outside the bank (sim_coef_kernel)
  const float ax = cf[0], bx = cf[1], max_ = cf[2], mbx = cf[3], ay = cf[4], by = cf[5], may = cf[6], mby = cf[7];
  sim_adjoint_tile(moving, fx, fy, counted, fixed_of, d_moving, H, W, F,
                   [=](float fxp, float fyp, float mx, float my, int, int, float& gx, float& gy) {
                     gx = ax * (fxp - mbx) + bx * (mx - max_);
                     gy = ay * (fyp - mby) + by * (my - may);
                   });
}

// records [V][bands][6], then the coefficients [V][8] float32
inline int64_t sim_bwd_need(int64_t V, int H) { return V * sim_bands(H) * SIM_MOVING + V * (SIM_COEF / 2); }

}  // namespace dfl

extern "C" int64_t dfl_sim_scratch_doubles(int32_t V, int32_t H, int32_t W) {
  if (dfl::sim_sizes_ok("", V, H, W) != DFL_OK) {                       // this function's one message replaces sim_sizes_ok's
    dfl::set_error("dfl_sim_scratch_doubles: bad sizes (views %d of 1..65535, image %d x %d of at least 3 x 3)", V, H, W);
    return DFL_ERR_INVALID_ARG;
  }
  return (int64_t)V * dfl::sim_bands(H) * dfl::SIM_MOVING;
}

extern "C" int dfl_sim_prepare(const dfl_sim_prepare_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_sim_prepare: null args");
  DFL_REQUIRE(a->fixed != nullptr && a->fx != nullptr && a->fy != nullptr && a->counted != nullptr && a->totals != nullptr,
              "dfl_sim_prepare: fixed, fx, fy, counted and totals are required");
  const int rc = dfl::sim_sizes_ok("dfl_sim_prepare", 1, a->H, a->W);
  if (rc != DFL_OK) return rc;
  dfl::sim_prepare_kernel<<<1, dfl::SIM_THREADS, 0, static_cast<hipStream_t>(stream)>>>(a->fixed, a->mask, a->fx, a->fy, a->counted,
                                                                                          a->totals, a->H, a->W);
  return dfl::check_launch("dfl_sim_prepare");
}

namespace dfl {

// What dfl_sim_gradncc, dfl_sim_gradncc_bwd and their bank forms are called with: fixed_of == nullptr is one fixed image
// (F = 1), d_moving == nullptr the forward alone.  `bank` and `bwd` say which entry point `who` is.
struct sim_call {
  const float *moving, *fx, *fy;
  const unsigned char* counted;
  const double* totals;
  const int32_t* fixed_of;
  double *scratch, *cost;
  float* d_moving;
  int64_t scratch_doubles;
  int V, H, W, F;
};

static int sim_launch(const char* who, const sim_call& c, bool bank, bool bwd, dfl_stream_t stream) {
  DFL_REQUIRE(c.moving != nullptr && c.fx != nullptr && c.fy != nullptr && c.counted != nullptr && c.totals != nullptr &&
                  c.scratch != nullptr && c.cost != nullptr && (!bwd || c.d_moving != nullptr),
              "%s: moving, fx, fy, counted, totals, scratch%s are required", who, bwd ? ", cost and d_moving" : " and cost");
  int rc = sim_sizes_ok(who, c.V, c.H, c.W);
  if (rc != DFL_OK) return rc;
  if (bank && (rc = sim_bank_ok(who, c.fixed_of, c.F, c.H, c.W)) != DFL_OK) return rc;
  const int bands = sim_bands(c.H);
  const int64_t need = bwd ? sim_bwd_need(c.V, c.H) : (int64_t)c.V * bands * SIM_MOVING;
  DFL_REQUIRE(c.scratch_doubles >= need, "%s: a scratch of %lld doubles, %lld are needed (%s)", who, (long long)c.scratch_doubles,
              (long long)need, bwd ? "dfl_sim_gradncc_bwd_scratch_doubles" : "dfl_sim_scratch_doubles");
  DFL_REQUIRE(!bwd || ceil_div(c.H, SIM_TILE) <= 65535, "%s: an image of %d rows is too tall", who, c.H);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the adjoint runs the forward's own two kernels first: its cost has the forward's bits
  sim_gradncc_kernel<<<dim3((unsigned)bands, (unsigned)c.V), SIM_THREADS, 0, s>>>(c.moving, c.fx, c.fy, c.counted, c.fixed_of, c.scratch,
                                                                                  c.H, c.W, c.F);
  sim_finish_kernel<<<(unsigned)c.V, 64, 0, s>>>(c.scratch, c.totals, c.fixed_of, c.cost, bands, c.F);
  if (bwd) {
    float* coef = reinterpret_cast<float*>(c.scratch + (size_t)c.V * bands * SIM_MOVING);
    sim_coef_kernel<<<(unsigned)ceil_div(c.V, 64), 64, 0, s>>>(c.scratch, c.totals, c.fixed_of, coef, bands, c.V, c.F);
    const dim3 grid((unsigned)ceil_div(c.W, SIM_TILE), (unsigned)ceil_div(c.H, SIM_TILE), (unsigned)c.V);
    sim_adjoint_kernel<<<grid, SIM_THREADS, 0, s>>>(c.moving, c.fx, c.fy, c.counted, c.fixed_of, coef, c.d_moving, c.H, c.W, c.F);
  }
  return check_launch(who);
}

}  // namespace dfl

extern "C" int dfl_sim_gradncc(const dfl_sim_gradncc_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_sim_gradncc: null args");
  const dfl::sim_call c = {a->moving, a->fx, a->fy, a->counted, a->totals, nullptr, a->scratch, a->cost, nullptr, a->scratch_doubles,
                           a->V,      a->H,  a->W,  1};
  return dfl::sim_launch("dfl_sim_gradncc", c, false, false, stream);
}

extern "C" int dfl_sim_bank_gradncc(const dfl_sim_bank_gradncc_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_sim_bank_gradncc: null args");
  const dfl::sim_call c = {a->moving, a->fx, a->fy, a->counted, a->totals, a->fixed_of, a->scratch, a->cost, nullptr, a->scratch_doubles,
                           a->V,      a->H,  a->W,  a->F};
  return dfl::sim_launch("dfl_sim_bank_gradncc", c, true, false, stream);
}

extern "C" int dfl_sim_gradncc_bwd_scratch_doubles(int32_t V, int32_t H, int32_t W) {
  if (dfl::sim_sizes_ok("", V, H, W) != DFL_OK || dfl::sim_bwd_need(V, H) >= ((int64_t)1 << 31)) {
    dfl::set_error("dfl_sim_gradncc_bwd_scratch_doubles: bad sizes (views %d of 1..65535, image %d x %d of at least 3 x 3), or more than "
                   "2^31 - 1 doubles", V, H, W);
    return DFL_ERR_INVALID_ARG;
  }
  return (int)dfl::sim_bwd_need(V, H);
}

extern "C" int dfl_sim_gradncc_bwd(const dfl_sim_gradncc_bwd_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_sim_gradncc_bwd: null args");
  const dfl::sim_call c = {a->moving, a->fx, a->fy, a->counted, a->totals, nullptr, a->scratch, a->cost, a->d_moving, a->scratch_doubles,
                           a->V,      a->H,  a->W,  1};
  return dfl::sim_launch("dfl_sim_gradncc_bwd", c, false, true, stream);
}

extern "C" int dfl_sim_bank_gradncc_bwd(const dfl_sim_bank_gradncc_bwd_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_sim_bank_gradncc_bwd: null args");
  const dfl::sim_call c = {a->moving, a->fx, a->fy, a->counted, a->totals, a->fixed_of, a->scratch, a->cost, a->d_moving,
                           a->scratch_doubles, a->V, a->H, a->W, a->F};
  return dfl::sim_launch("dfl_sim_bank_gradncc_bwd", c, true, true, stream);
}
