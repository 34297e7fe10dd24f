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
  for (int j = threadIdx.x; j < wi; j += SIM_THREADS) {
    double s[SIM_FIXED] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < S; ++k) {
      const size_t at = (size_t)(r0 + k) * W + (1 + j);
      if (counted[at]) sim_fixed_sums(s, fx[at], fy[at]);
    }
#pragma unroll
    for (int q = 0; q < SIM_FIXED; ++q) cols[q * wi + j] = s[q];
  }
  __syncthreads();
  for (int b = threadIdx.x; b < PC; b += SIM_THREADS) {
    double s[SIM_FIXED] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const int j0 = b * stride;
    for (int k = 0; k < S; ++k) {
#pragma unroll
      for (int q = 0; q < SIM_FIXED; ++q) s[q] += cols[q * wi + j0 + k];
    }
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

__global__ __launch_bounds__(SIM_THREADS) void sim_patch_gradncc_kernel(const float* __restrict__ moving, const float* __restrict__ fx,
                                                                        const float* __restrict__ fy,
                                                                        const unsigned char* __restrict__ counted,
                                                                        const double* __restrict__ ptotals,
                                                                        const unsigned char* __restrict__ pflags,
                                                                        const int32_t* __restrict__ fixed_of,
                                                                        double* __restrict__ scratch, int H, int W, int S, int stride,
                                                                        int PC, int F) {
  extern __shared__ double cols[];                                      // [SIM_MOVING][W - 2]
  __shared__ double lds[2 * 4];
  const int a = blockIdx.x, view = blockIdx.y, wi = W - 2;
  const int r0 = 1 + a * stride;
  const int f = sim_image_of(fixed_of, view, F);
  if (f < 0) return;                                                    // the whole workgroup: sim_patch_finish_kernel reads no record
  const size_t plane = (size_t)f * H * W, patches = (size_t)f * gridDim.x * PC;
  fx += plane;
  fy += plane;
  counted += plane;
  ptotals += patches * SIM_FIXED;
  pflags += patches;
  const float* img = moving + (size_t)view * H * W;
  for (int j = threadIdx.x; j < wi; j += SIM_THREADS) {
    double s[SIM_MOVING] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < S; ++k) {
      const int r = r0 + k, c = 1 + j;
      if (counted[(size_t)r * W + c]) sim_moving_sums(s, img, fx, fy, W, r, c);
    }
#pragma unroll
    for (int q = 0; q < SIM_MOVING; ++q) cols[q * wi + j] = s[q];
  }
  __syncthreads();
  double acc[2] = {0.0, 0.0};
  for (int b = threadIdx.x; b < PC; b += SIM_THREADS) {
    const size_t p = (size_t)a * PC + b;
    const unsigned char flags = pflags[p];
    if (flags == 0) continue;
    double s[SIM_MOVING] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int j0 = b * stride;
    for (int k = 0; k < S; ++k) {
#pragma unroll
      for (int q = 0; q < SIM_MOVING; ++q) s[q] += cols[q * wi + j0 + k];
    }
    const double* t = ptotals + p * SIM_FIXED;
    if (flags & 1) acc[0] += sim_ncc(t[0], s[0], s[1], t[1], t[2], s[2]);
    if (flags & 2) acc[1] += sim_ncc(t[0], s[3], s[4], t[3], t[4], s[5]);
  }
  block_sum<2>(acc, lds);
  if (threadIdx.x == 0) {
    double* rec = scratch + ((size_t)view * gridDim.x + a) * 2;
    rec[0] = acc[0];
    rec[1] = acc[1];
  }
}

// One wave per view: lanes 0 and 1 add the view's PR records of ncc_x / ncc_y in index order
__global__ __launch_bounds__(64) void sim_patch_finish_kernel(const double* __restrict__ scratch, const int* __restrict__ pcount,
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
    const int n = pcount[threadIdx.x];
    m[threadIdx.x] = n > 0 ? acc / (double)n : 0.0;
  }
  __syncthreads();
  if (threadIdx.x == 0) cost[view] = 1.0 - 0.5 * (m[0] + m[1]);
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

namespace dfl {

// what dfl_sim_patch_gradncc and its bank form are called with: fixed_of == nullptr is one fixed image (F = 1)
struct sim_patch_call {
  const float *moving, *fx, *fy;
  const unsigned char* counted;
  const double* ptotals;
  const unsigned char* pflags;
  const int32_t *pcount, *fixed_of;
  double *scratch, *cost;
  int64_t scratch_doubles;
  int V, H, W, rho, stride, F;
};

static int sim_patch_launch(const char* who, const sim_patch_call& c, bool bank, dfl_stream_t stream) {
  DFL_REQUIRE(c.moving != nullptr && c.fx != nullptr && c.fy != nullptr && c.counted != nullptr && c.ptotals != nullptr &&
                  c.pflags != nullptr && c.pcount != nullptr && c.scratch != nullptr && c.cost != nullptr,
              "%s: moving, fx, fy, counted, ptotals, pflags, pcount, scratch and cost are required", who);
  patch_grid g;
  int rc = patch_sizes_ok(who, c.H, c.W, c.rho, c.stride, &g);
  if (rc != DFL_OK) return rc;
  DFL_REQUIRE(c.V >= 1 && c.V <= 65535, "%s: 1..65535 views per call, got %d", who, c.V);
  if (bank && (rc = sim_bank_ok(who, c.fixed_of, c.F, c.H, c.W)) != DFL_OK) return rc;
  const int64_t need = (int64_t)c.V * g.PR * 2;
  DFL_REQUIRE(c.scratch_doubles >= need, "%s: a scratch of %lld doubles, %lld are needed (dfl_sim_patch_scratch_doubles)", who,
              (long long)c.scratch_doubles, (long long)need);
  const int lds = SIM_MOVING * (c.W - 2) * (int)sizeof(double);
  DFL_LDS_OPT_IN(sim_patch_gradncc_kernel, DFL_SIM_PATCH_MAX_W * SIM_MOVING * sizeof(double), who)
  hipStream_t s = static_cast<hipStream_t>(stream);
  sim_patch_gradncc_kernel<<<dim3((unsigned)g.PR, (unsigned)c.V), SIM_THREADS, lds, s>>>(
      c.moving, c.fx, c.fy, c.counted, c.ptotals, c.pflags, c.fixed_of, c.scratch, c.H, c.W, g.S, c.stride, g.PC, c.F);
  sim_patch_finish_kernel<<<(unsigned)c.V, 64, 0, s>>>(c.scratch, c.pcount, c.fixed_of, c.cost, g.PR, c.F);
  return check_launch(who);
}

}  // namespace dfl

extern "C" int dfl_sim_patch_gradncc(const dfl_sim_patch_gradncc_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_sim_patch_gradncc: null args");
  const dfl::sim_patch_call c = {a->moving,  a->fx,   a->fy, a->counted, a->ptotals, a->pflags, a->pcount, nullptr,
                                 a->scratch, a->cost, a->scratch_doubles, a->V, a->H, a->W, a->rho, a->stride, 1};
  return dfl::sim_patch_launch("dfl_sim_patch_gradncc", c, false, stream);
}

extern "C" int dfl_sim_patch_bank_gradncc(const dfl_sim_patch_bank_gradncc_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_sim_patch_bank_gradncc: null args");
  const dfl::sim_patch_call c = {a->moving,  a->fx,   a->fy, a->counted, a->ptotals, a->pflags, a->pcount, a->fixed_of,
                                 a->scratch, a->cost, a->scratch_doubles, a->V, a->H, a->W, a->rho, a->stride, a->F};
  return dfl::sim_patch_launch("dfl_sim_patch_bank_gradncc", c, true, stream);
}
