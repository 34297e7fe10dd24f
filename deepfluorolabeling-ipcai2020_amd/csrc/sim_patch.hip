// Patch-wise gradient-NCC between V rendered views and one fixed image: the similarity='patch' cost of dfl_amd.register.
// Contract: include/dfl_hip.h (dfl_sim_patch_prepare_args, dfl_sim_patch_gradncc_args); the semantics are stated in
// DESIGN.md section 18 and restated in numpy float64 by tests/patch_ref.py.  Sobel, the sums of a pixel and the NCC are
// csrc/sim.h's, shared with csrc/sim.hip; the block and record sums are csrc/fixed_sum.h's.
//
// Both passes have one shape: a workgroup of 256 threads owns one patch row a (the S interior rows a s .. a s + S - 1) of
// one image.  Phase 1: thread t takes the interior columns t, t + 256, ... and adds its sums down the S rows of the band,
// row by row, in float64 (consecutive lanes read consecutive columns; with s < S a row is read again by S / s patch rows,
// out of L2), and leaves them in LDS: [sums][W - 2] doubles.  Phase 2: thread t takes the patches t, t + 256, ... of the
// row and adds each one's S column sums in index order.
//   sim_patch_prepare_kernel (once per fixed image): five sums (n, fx, fx^2, fy, fy^2) -> ptotals and pflags of the row;
//   sim_patch_count_kernel: one workgroup counts the flags -> pcount (integers in float64: exact, any order).
//   sim_patch_gradncc_kernel (once per generation): six sums (mx, mx^2, mx fx, my, my^2, my fy) -> the two NCCs of every
//   patch of the row, gated by pflags; a thread adds its patches' NCCs in index order, the workgroup adds the threads in
//   block_sum's fixed order and writes ONE record of two doubles with plain stores.
//   sim_patch_finish_kernel (one wave per view): adds the PR records in index order, divides by pcount, writes the cost.
// No atomics: the bits of a view's cost depend on that view's pixels and on H, W, rho and the stride only.
// dfl_sim_patch_eval is the same forward with two optional parts: pweights / pwsum weigh every patch
// by the energy of its fixed gradient (sim_patch_weights_kernel, once per fixed image), and d_moving asks for the adjoint:
// phase 2 then also leaves eight float32 per patch (c alpha, c beta, mean a, mean b of x, then of y; c the patch's share of
// the cost) and sim_patch_adjoint_kernel gathers them per pixel.
// dfl_sim_patch_bank_gradncc launches the same two kernels with fixed_of [V] and F: view v reads the
// planes, patch totals, flags and counts of image fixed_of[v] of a bank (sim_image_of, csrc/sim.h); dfl_sim_patch_gradncc
// passes fixed_of = nullptr and every view reads image 0.
#include "sim.h"

namespace dfl {


struct patch_grid {
  int S, PR, PC;
};

// false when a patch does not fit into the interior
inline bool patch_grid_of(int H, int W, int rho, int stride, patch_grid* g) {
  const int64_t S = 2 * (int64_t)rho + 1;
  if (H - 2 < S || W - 2 < S) return false;
  g->S = (int)S;
  g->PR = (int)((H - 2 - S) / stride + 1);
  g->PC = (int)((W - 2 - S) / stride + 1);
  return true;
}

__global__ __launch_bounds__(SIM_THREADS) void sim_patch_prepare_kernel(const float* __restrict__ fx, const float* __restrict__ fy,
                                                                        const unsigned char* __restrict__ counted,
                                                                        double* __restrict__ ptotals, unsigned char* __restrict__ pflags,
                                                                        int W, int S, int stride, int PC, int min_count) {
  extern __shared__ double cols[];                                      // [SIM_FIXED][W - 2]
  const int a = blockIdx.x, wi = W - 2;
  const int r0 = 1 + a * stride;                                        // first image row of the band
  sim_column_sums<SIM_FIXED>(cols, wi, r0, S, [=](double (&s)[SIM_FIXED], int r, int c) {
    const size_t at = (size_t)r * W + c;
    if (counted[at]) sim_fixed_sums(s, fx[at], fy[at]);
  });
  __syncthreads();
  for (int b = threadIdx.x; b < PC; b += SIM_THREADS) {
    double s[SIM_FIXED];
    sim_patch_sums<SIM_FIXED>(s, cols, wi, b * stride, S);
    const size_t p = (size_t)a * PC + b;
#pragma unroll
    for (int q = 0; q < SIM_FIXED; ++q) ptotals[p * SIM_FIXED + q] = s[q];
    unsigned char flags = 0;
    if (s[0] >= (double)min_count) {                                    // min_count >= 1: n is not 0 below
      if (sim_live(sim_var(s[0], s[1], s[2]), s[2])) flags |= 1;         // the rule of sim_ncc
      if (sim_live(sim_var(s[0], s[3], s[4]), s[4])) flags |= 2;
    }
    pflags[p] = flags;
  }
}

__global__ __launch_bounds__(SIM_THREADS) void sim_patch_count_kernel(const unsigned char* __restrict__ pflags, int* __restrict__ pcount,
                                                                      int64_t P) {
  __shared__ double lds[2 * 4];
  double s[2] = {0.0, 0.0};
  for (int64_t p = threadIdx.x; p < P; p += SIM_THREADS) {
    const unsigned char f = pflags[p];
    s[0] += (double)(f & 1);
    s[1] += (double)((f >> 1) & 1);
  }
  block_sum<2>(s, lds);
  if (threadIdx.x == 0) {
    pcount[0] = (int)s[0];
    pcount[1] = (int)s[1];
  }
}

// One workgroup, once per fixed image: w_d[p] = sum (f_d - mean f_d)^2 over the counted pixels of a patch that counts in d, else
// 0.  Thread t adds the patches t, t + 256, ... in index order, then block_sum: the sums are no integers, the order is the contract
__global__ __launch_bounds__(SIM_THREADS) void sim_patch_weights_kernel(const double* __restrict__ ptotals,
                                                                        const unsigned char* __restrict__ pflags,
                                                                        double* __restrict__ pweights, double* __restrict__ pwsum, int64_t P) {
  __shared__ double lds[2 * 4];
  double s[2] = {0.0, 0.0};
  for (int64_t p = threadIdx.x; p < P; p += SIM_THREADS) {
    const unsigned char f = pflags[p];
    const double* t = ptotals + p * SIM_FIXED;
    const double wx = (f & 1) ? sim_var(t[0], t[1], t[2]) : 0.0, wy = (f & 2) ? sim_var(t[0], t[3], t[4]) : 0.0;
    pweights[p * 2] = wx;
    pweights[p * 2 + 1] = wy;
    s[0] += wx;
    s[1] += wy;
  }
  block_sum<2>(s, lds);
  if (threadIdx.x == 0) {
    pwsum[0] = s[0];
    pwsum[1] = s[1];
  }
}

constexpr int SIM_PCOEF = 8;         // per view and patch: c alpha, c beta, mean a, mean b of x, then of y (float32; sim_coef4, csrc/sim.h)

// pweights (with pwsum) and coef are optional: both nullptr is the cost of section 18 as dfl_sim_patch_gradncc always gave it.
// One body, two instantiations: EXT = false is launched when both are nullptr and holds nothing of the two parts, so the existing
// entry points keep their registers (62 VGPRs, 8 waves per SIMD) next to the 118 of the coefficients' float64 arithmetic
template <bool EXT>
__global__ __launch_bounds__(SIM_THREADS) void sim_patch_gradncc_kernel(const float* __restrict__ moving, const float* __restrict__ fx,
                                                                        const float* __restrict__ fy,
                                                                        const unsigned char* __restrict__ counted,
                                                                        const double* __restrict__ ptotals,
                                                                        const unsigned char* __restrict__ pflags,
                                                                        const int32_t* __restrict__ fixed_of,
                                                                        const int32_t* __restrict__ pcount,
                                                                        const double* __restrict__ pweights,
                                                                        const double* __restrict__ pwsum, float* __restrict__ coef,
                                                                        double* __restrict__ scratch, int H, int W, int S, int stride,
                                                                        int PC, int F) {
  extern __shared__ double cols[];                                      // [SIM_MOVING][W - 2]
  __shared__ double lds[2 * 4];
  const int a = blockIdx.x, view = blockIdx.y, wi = W - 2;
  const int r0 = 1 + a * stride;
  const int f = sim_image_of(fixed_of, view, F);
  if (f < 0) return;                                                    // the whole workgroup: sim_patch_finish_kernel reads no record
  const size_t patches = (size_t)f * gridDim.x * PC;
  sim_planes_of(fx, fy, counted, f, H, W);
  ptotals += patches * SIM_FIXED;
  pflags += patches;
  const bool weighted = EXT && pweights != nullptr, with_coef = EXT && coef != nullptr;
  if (weighted) {
    pweights += patches * 2;
    pwsum += 2 * (size_t)f;
  }
  pcount += 2 * (size_t)f;
  if (with_coef) coef += (size_t)view * gridDim.x * PC * SIM_PCOEF;
  const float* img = moving + (size_t)view * H * W;
  sim_column_sums<SIM_MOVING>(cols, wi, r0, S, [=](double (&s)[SIM_MOVING], int r, int c) {
    if (counted[(size_t)r * W + c]) sim_moving_sums(s, img, fx, fy, W, r, c);
  });
  __syncthreads();
  double acc[2] = {0.0, 0.0};
  for (int b = threadIdx.x; b < PC; b += SIM_THREADS) {
    const size_t p = (size_t)a * PC + b;
    const unsigned char flags = pflags[p];
    if (flags == 0) {
      if (with_coef) {
#pragma unroll
        for (int q = 0; q < SIM_PCOEF; ++q) coef[p * SIM_PCOEF + q] = 0.f;
      }
      continue;
    }
    double s[SIM_MOVING];
    sim_patch_sums<SIM_MOVING>(s, cols, wi, b * stride, S);
    const double* t = ptotals + p * SIM_FIXED;
    if (!weighted) {
      if (flags & 1) acc[0] += sim_ncc(t[0], s[0], s[1], t[1], t[2], s[2]);
      if (flags & 2) acc[1] += sim_ncc(t[0], s[3], s[4], t[3], t[4], s[5]);
    } else {                                                            // a patch that does not count in d has w_d = 0
      if (flags & 1) acc[0] += pweights[p * 2] * sim_ncc(t[0], s[0], s[1], t[1], t[2], s[2]);
      if (flags & 2) acc[1] += pweights[p * 2 + 1] * sim_ncc(t[0], s[3], s[4], t[3], t[4], s[5]);
    }
    if (with_coef) {
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        float* out = coef + p * SIM_PCOEF + 4 * d;
        if (flags & (1 << d)) {                                         // it counts: pcount[d] >= 1, and pwsum[d] >= w_d > 0
          const double share = weighted ? pweights[p * 2 + d] / pwsum[d] : 1.0 / (double)pcount[d];
          sim_coef4(out, share, t[0], s[3 * d], s[3 * d + 1], t[1 + 2 * d], t[2 + 2 * d], s[3 * d + 2]);
        } else {
          out[0] = out[1] = out[2] = out[3] = 0.f;
        }
      }
    }
  }
  block_sum<2>(acc, lds);
  if (threadIdx.x == 0) {
    double* rec = scratch + ((size_t)view * gridDim.x + a) * 2;
    rec[0] = acc[0];
    rec[1] = acc[1];
  }
}

// One wave per view: lanes 0 and 1 add the view's PR records of ncc_x / ncc_y in index order; pwsum = nullptr: the uniform cost
__global__ __launch_bounds__(64) void sim_patch_finish_kernel(const double* __restrict__ scratch, const int* __restrict__ pcount,
                                                              const double* __restrict__ pwsum,
                                                              const int32_t* __restrict__ fixed_of, double* __restrict__ cost, int PR,
                                                              int F) {
  __shared__ double m[2];
  const int view = blockIdx.x;
  const int f = sim_image_of(fixed_of, view, F);
  if (f < 0) {                                                          // the whole workgroup: no barrier is left waiting
    if (threadIdx.x == 0) cost[view] = __builtin_nan("");
    return;
  }
  pcount += 2 * f;
  if (threadIdx.x < 2) {
    const double acc = records_sum(scratch + (size_t)view * PR * 2 + threadIdx.x, PR, 2);
    if (pwsum == nullptr) {
      const int n = pcount[threadIdx.x];
      m[threadIdx.x] = n > 0 ? acc / (double)n : 0.0;
    } else {                                                            // the weighted mean: the records hold sum w ncc
      const double w = pwsum[2 * (size_t)f + threadIdx.x];
      m[threadIdx.x] = w > 0.0 ? acc / w : 0.0;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) cost[view] = 1.0 - 0.5 * (m[0] + m[1]);
}

// ---- the adjoint: d cost[v] / d moving[v][r][c] (dfl_sim_patch_eval with d_moving) ------------------------------------------------
// sim_adjoint_tile (csrc/sim.h), as sim_adjoint_kernel (csrc/sim.hip): a workgroup owns a 16 x 16 tile of one view's d_moving, stages
// the tile of `moving` with a halo of 2 in LDS and computes g = d cost / d (Sobel value) on the 18 x 18 pixels around the tile; here g at interior
// pixel (i, j) is the sum over the patches that hold it -- a from max(0, ceil((i - S + 1) / s)) to min(PR - 1, i / s), b likewise,
// a outer and b inner -- of c alpha (b_q - mean b) + c beta (a_q - mean a) with the patch's eight coefficients, read straight
// from global memory (32 B per patch, L1/L2-resident: a tile of 18 x 18 pixels shares at most (17 / s + S / s + 2)^2 patches).
// LDS is 4.4 KB whatever rho and s are.  No atomics: a view's bits depend on its own pixels, its fixed image and H, W, rho, s only.
__global__ __launch_bounds__(SIM_THREADS) void sim_patch_adjoint_kernel(const float* __restrict__ moving, const float* __restrict__ fx,
                                                                        const float* __restrict__ fy,
                                                                        const unsigned char* __restrict__ counted,
                                                                        const int32_t* __restrict__ fixed_of, const float* __restrict__ coef,
                                                                        float* __restrict__ d_moving, int H, int W, int S, int stride,
                                                                        int PR, int PC, int F) {
  // every product is rounded on its own, as in sim_adjoint_kernel: where moving matches fixed the two terms of a patch cancel
#pragma clang fp contract(off)
  coef += (size_t)blockIdx.z * PR * PC * SIM_PCOEF;
  sim_adjoint_tile(moving, fx, fy, counted, fixed_of, d_moving, H, W, F,
                   [=](float bx, float by, float mx, float my, int r, int c, float& gx, float& gy) {
                     const int i = r - 1, j = c - 1;
                     const int a_lo = i < S ? 0 : (i - S + stride) / stride, a_hi = min(PR - 1, i / stride);     // ceil((i - S + 1) / s)
                     const int b_lo = j < S ? 0 : (j - S + stride) / stride, b_hi = min(PC - 1, j / stride);
                     for (int a = a_lo; a <= a_hi; ++a) {
                       const float* cf = coef + ((size_t)a * PC + b_lo) * SIM_PCOEF;
                       for (int b = b_lo; b <= b_hi; ++b, cf += SIM_PCOEF) {
                         gx += cf[0] * (bx - cf[3]) + cf[1] * (mx - cf[2]);
                         gy += cf[4] * (by - cf[7]) + cf[5] * (my - cf[6]);
                       }
                     }
                   });
}

// the checks on sizes that every entry point shares; `who` names it in the message
static int patch_sizes_ok(const char* who, int H, int W, int rho, int stride, patch_grid* g) {
  const int rc = sim_sizes_ok(who, 1, H, W);                            // the views are checked after the patches
  if (rc != DFL_OK) return rc;
  DFL_REQUIRE(rho >= 1, "%s: a patch radius of %d (at least 1)", who, rho);
  DFL_REQUIRE(stride >= 1, "%s: a patch stride of %d (at least 1)", who, stride);
  DFL_REQUIRE(patch_grid_of(H, W, rho, stride, g), "%s: a patch of side %lld does not fit into the %d x %d interior pixels", who,
              2 * (long long)rho + 1, H - 2, W - 2);
  DFL_REQUIRE(W <= DFL_SIM_PATCH_MAX_W, "%s: an image %d wide, at most %d (DFL_SIM_PATCH_MAX_W: the column sums of a band live in LDS)",
              who, W, DFL_SIM_PATCH_MAX_W);
  return DFL_OK;
}

}  // namespace dfl

extern "C" int64_t dfl_sim_patch_count(int32_t H, int32_t W, int32_t rho, int32_t stride) {
  dfl::patch_grid g;
  const int rc = dfl::patch_sizes_ok("dfl_sim_patch_count", H, W, rho, stride, &g);
  if (rc != DFL_OK) return rc;
  return (int64_t)g.PR * g.PC;
}

extern "C" int64_t dfl_sim_patch_scratch_doubles(int32_t V, int32_t H, int32_t W, int32_t rho, int32_t stride) {
  dfl::patch_grid g;
  const int rc = dfl::patch_sizes_ok("dfl_sim_patch_scratch_doubles", H, W, rho, stride, &g);
  if (rc != DFL_OK) return rc;
  DFL_REQUIRE(V >= 1 && V <= 65535, "dfl_sim_patch_scratch_doubles: 1..65535 views per call, got %d", V);
  return (int64_t)V * g.PR * 2;
}

extern "C" int dfl_sim_patch_prepare(const dfl_sim_patch_prepare_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_sim_patch_prepare: null args");
  DFL_REQUIRE(a->fx != nullptr && a->fy != nullptr && a->counted != nullptr && a->ptotals != nullptr && a->pflags != nullptr &&
                  a->pcount != nullptr,
              "dfl_sim_patch_prepare: fx, fy, counted, ptotals, pflags and pcount are required");
  dfl::patch_grid g;
  const int rc = dfl::patch_sizes_ok("dfl_sim_patch_prepare", a->H, a->W, a->rho, a->stride, &g);
  if (rc != DFL_OK) return rc;
  DFL_REQUIRE(a->min_count >= 1, "dfl_sim_patch_prepare: a min_count of %d (at least 1)", a->min_count);
  const int lds = dfl::SIM_FIXED * (a->W - 2) * (int)sizeof(double);
  DFL_LDS_OPT_IN(dfl::sim_patch_prepare_kernel, DFL_SIM_PATCH_MAX_W * dfl::SIM_FIXED * sizeof(double), "dfl_sim_patch_prepare")
  hipStream_t s = static_cast<hipStream_t>(stream);
  dfl::sim_patch_prepare_kernel<<<(unsigned)g.PR, dfl::SIM_THREADS, lds, s>>>(a->fx, a->fy, a->counted, a->ptotals, a->pflags, a->W, g.S,
                                                                              a->stride, g.PC, a->min_count);
  dfl::sim_patch_count_kernel<<<1, dfl::SIM_THREADS, 0, s>>>(a->pflags, a->pcount, (int64_t)g.PR * g.PC);
  return dfl::check_launch("dfl_sim_patch_prepare");
}

extern "C" int dfl_sim_patch_weights(const dfl_sim_patch_weights_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_sim_patch_weights: null args");
  DFL_REQUIRE(a->ptotals != nullptr && a->pflags != nullptr && a->pweights != nullptr && a->pwsum != nullptr,
              "dfl_sim_patch_weights: ptotals, pflags, pweights and pwsum are required");
  DFL_REQUIRE(a->P >= 1 && a->P < ((int64_t)1 << 31), "dfl_sim_patch_weights: %lld patches (1 .. 2^31 - 1: dfl_sim_patch_count)",
              (long long)a->P);
  dfl::sim_patch_weights_kernel<<<1, dfl::SIM_THREADS, 0, static_cast<hipStream_t>(stream)>>>(a->ptotals, a->pflags, a->pweights, a->pwsum,
                                                                                                a->P);
  return dfl::check_launch("dfl_sim_patch_weights");
}

namespace dfl {

// What dfl_sim_patch_gradncc, its bank form and dfl_sim_patch_eval are called with: fixed_of == nullptr is one fixed image
// (F = 1), pweights == nullptr the uniform cost, d_moving == nullptr the forward alone
struct sim_patch_call {
  const float *moving, *fx, *fy;
  const unsigned char* counted;
  const double* ptotals;
  const unsigned char* pflags;
  const int32_t *pcount, *fixed_of;
  const double *pweights, *pwsum;
  double *scratch, *cost;
  float* d_moving;
  int64_t scratch_doubles;
  int V, H, W, rho, stride, F;
};

// records [V][PR][2], then with the adjoint the coefficients [V][P][8] float32
inline int64_t sim_patch_need(int64_t V, const patch_grid& g, bool bwd) {
  return V * g.PR * 2 + (bwd ? V * g.PR * g.PC * (SIM_PCOEF / 2) : 0);
}

// `sizes` names the function that says how long the scratch has to be
static int sim_patch_launch(const char* who, const char* sizes, const sim_patch_call& c, bool bank, dfl_stream_t stream) {
  DFL_REQUIRE(c.moving != nullptr && c.fx != nullptr && c.fy != nullptr && c.counted != nullptr && c.ptotals != nullptr &&
                  c.pflags != nullptr && c.pcount != nullptr && c.scratch != nullptr && c.cost != nullptr,
              "%s: moving, fx, fy, counted, ptotals, pflags, pcount, scratch and cost are required", who);
  DFL_REQUIRE((c.pweights == nullptr) == (c.pwsum == nullptr), "%s: pweights and pwsum come together (both NULL: the uniform cost)", who);
  patch_grid g;
  int rc = patch_sizes_ok(who, c.H, c.W, c.rho, c.stride, &g);
  if (rc != DFL_OK) return rc;
  DFL_REQUIRE(c.V >= 1 && c.V <= 65535, "%s: 1..65535 views per call, got %d", who, c.V);
  if (bank && (rc = sim_bank_ok(who, c.fixed_of, c.F, c.H, c.W)) != DFL_OK) return rc;
  const bool bwd = c.d_moving != nullptr;
  const int64_t need = sim_patch_need(c.V, g, bwd);
  DFL_REQUIRE(c.scratch_doubles >= need, "%s: a scratch of %lld doubles, %lld are needed (%s)", who, (long long)c.scratch_doubles,
              (long long)need, sizes);
  DFL_REQUIRE(!bwd || ceil_div(c.H, SIM_TILE) <= 65535, "%s: an image of %d rows is too tall for the adjoint", who, c.H);
  const int lds = SIM_MOVING * (c.W - 2) * (int)sizeof(double);
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* coef = bwd ? reinterpret_cast<float*>(c.scratch + (size_t)c.V * g.PR * 2) : nullptr;
  const dim3 rows((unsigned)g.PR, (unsigned)c.V);
  // the adjoint runs the forward's own two kernels first: its cost has the forward's bits
  if (c.pweights != nullptr || bwd) {
    DFL_LDS_OPT_IN(sim_patch_gradncc_kernel<true>, DFL_SIM_PATCH_MAX_W * SIM_MOVING * sizeof(double), who)
    sim_patch_gradncc_kernel<true><<<rows, SIM_THREADS, lds, s>>>(c.moving, c.fx, c.fy, c.counted, c.ptotals, c.pflags, c.fixed_of, c.pcount,
                                                                  c.pweights, c.pwsum, coef, c.scratch, c.H, c.W, g.S, c.stride, g.PC, c.F);
  } else {
    DFL_LDS_OPT_IN(sim_patch_gradncc_kernel<false>, DFL_SIM_PATCH_MAX_W * SIM_MOVING * sizeof(double), who)
    sim_patch_gradncc_kernel<false><<<rows, SIM_THREADS, lds, s>>>(c.moving, c.fx, c.fy, c.counted, c.ptotals, c.pflags, c.fixed_of, c.pcount,
                                                                   nullptr, nullptr, nullptr, c.scratch, c.H, c.W, g.S, c.stride, g.PC, c.F);
  }
  sim_patch_finish_kernel<<<(unsigned)c.V, 64, 0, s>>>(c.scratch, c.pcount, c.pwsum, c.fixed_of, c.cost, g.PR, c.F);
  if (bwd) {
    const dim3 grid((unsigned)ceil_div(c.W, SIM_TILE), (unsigned)ceil_div(c.H, SIM_TILE), (unsigned)c.V);
    sim_patch_adjoint_kernel<<<grid, SIM_THREADS, 0, s>>>(c.moving, c.fx, c.fy, c.counted, c.fixed_of, coef, c.d_moving, c.H, c.W, g.S,
                                                          c.stride, g.PR, g.PC, c.F);
  }
  return check_launch(who);
}

}  // namespace dfl

extern "C" int dfl_sim_patch_gradncc(const dfl_sim_patch_gradncc_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_sim_patch_gradncc: null args");
  const dfl::sim_patch_call c = {a->moving, a->fx,      a->fy,   a->counted, a->ptotals,         a->pflags, a->pcount, nullptr, nullptr,
                                 nullptr,   a->scratch, a->cost, nullptr,    a->scratch_doubles, a->V,      a->H,      a->W,    a->rho,
                                 a->stride, 1};
  return dfl::sim_patch_launch("dfl_sim_patch_gradncc", "dfl_sim_patch_scratch_doubles", c, false, stream);
}

extern "C" int dfl_sim_patch_bank_gradncc(const dfl_sim_patch_bank_gradncc_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_sim_patch_bank_gradncc: null args");
  const dfl::sim_patch_call c = {a->moving, a->fx,      a->fy,   a->counted, a->ptotals,         a->pflags, a->pcount, a->fixed_of, nullptr,
                                 nullptr,   a->scratch, a->cost, nullptr,    a->scratch_doubles, a->V,      a->H,      a->W,        a->rho,
                                 a->stride, a->F};
  return dfl::sim_patch_launch("dfl_sim_patch_bank_gradncc", "dfl_sim_patch_scratch_doubles", c, true, stream);
}

extern "C" int dfl_sim_patch_eval_scratch_doubles(int32_t V, int32_t H, int32_t W, int32_t rho, int32_t stride, int32_t bwd) {
  dfl::patch_grid g;
  const int rc = dfl::patch_sizes_ok("dfl_sim_patch_eval_scratch_doubles", H, W, rho, stride, &g);
  if (rc != DFL_OK) return rc;
  DFL_REQUIRE(V >= 1 && V <= 65535, "dfl_sim_patch_eval_scratch_doubles: 1..65535 views per call, got %d", V);
  const int64_t need = dfl::sim_patch_need(V, g, bwd != 0);
  DFL_REQUIRE(need < ((int64_t)1 << 31), "dfl_sim_patch_eval_scratch_doubles: %lld doubles, more than 2^31 - 1", (long long)need);
  return (int)need;
}

extern "C" int dfl_sim_patch_eval(const dfl_sim_patch_eval_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_sim_patch_eval: null args");
  const bool bank = a->fixed_of != nullptr;                             // without fixed_of there is one image and F is not read
  const dfl::sim_patch_call c = {a->moving,   a->fx,      a->fy,   a->counted,  a->ptotals,         a->pflags, a->pcount, a->fixed_of, a->pweights,
                                 a->pwsum,    a->scratch, a->cost, a->d_moving, a->scratch_doubles, a->V,      a->H,      a->W,        a->rho,
                                 a->stride,   bank ? a->F : 1};
  return dfl::sim_patch_launch("dfl_sim_patch_eval", "dfl_sim_patch_eval_scratch_doubles", c, bank, stream);
}

