// The pose gradient of the trilinear DRR with its sampling frozen: per view and object the force F and the moment Mom
// about a pivot that a detector-space adjoint d_att exerts on the object.
// Contract: include/dfl_hip.h (dfl_drr_pose_grad_args); the semantics are stated in DESIGN.md section 19 and restated
// in numpy by tests/grad_ref.py.
//
// One thread per ray and view in the renderer's 8 x 8-tile-per-wave mapping, so that the eight gathers of a sample hit
// the lines its neighbours hit.  A thread walks the samples drr_trilinear_object took (drr_ray, drr_samples and drr_gather
// of csrc/drr.h, the functions the renderer calls), and per sample takes the gradient of the trilinear interpolant in the
// cell drr_corner picked: per axis the bilinear blend of the four corner differences, 0 where the corners were clamped
// together.  Twelve float32 sums per ray and object (grad f, and grad f times the sample's offset from the pivot -- about
// 20 voxels, never the 800 mm of t), scaled by d_att s (t1 - t0) / N, promoted to float64 and added in the fixed order of
// csrc/fixed_sum.h; ONE record of twelve doubles per workgroup and object with plain stores.  drr_grad_finish_kernel adds the
// records of a view and object in index order.  No atomics: the bits depend on that view's records, pivots and d_att only.
// Bound by the eight dependent gathers per sample, as the renderer is; the arithmetic on top is about 40 flops.
#include "drr.h"
#include "fixed_sum.h"

namespace dfl {

constexpr int DRR_GRAD_N = 12;               // F[3], then Mom[3][3] row-major

struct DrrGradParams {
  DrrScene S;
  const float* d_att;
  const float* pivots;
  double* scratch;
};

// acc[0..2] = w sum_k grad f(x_k), acc[3 + 3 a + b] = w sum_k grad f_a(x_k) (x_k - pivot)_b; zeros when the ray misses
__device__ __forceinline__ void drr_grad_object(const DrrScene& S, const dfl_drr_object& ob, const float* pivot, float c, float r,
                                                float s, float (&acc)[DRR_GRAD_N]) {
#pragma unroll
  for (int k = 0; k < DRR_GRAD_N; ++k) acc[k] = 0.f;
  DrrRay R;
  if (!drr_ray(ob, S.nx, S.ny, S.nz, c, r, R)) return;
  const DrrSamples sm = drr_samples(R, s, S.step_mm);
  const float pv[3] = {pivot[0], pivot[1], pivot[2]};
  for (int j = 0; j < sm.N; ++j) {
    DrrCell C;
    drr_gather(S, ob.mask, R, R.t0 + ((float)j + 0.5f) * sm.dt, C);
    const float* v = C.v;                                  // v[x + 2 y + 4 z]
    // along x: the four corner differences, blended over y and z
    const float e00 = v[1] - v[0], e10 = v[3] - v[2], e01 = v[5] - v[4], e11 = v[7] - v[6];
    const float ex0 = e00 + C.wy * (e10 - e00), ex1 = e01 + C.wy * (e11 - e01);
    const float gx = ex0 + C.wz * (ex1 - ex0);
    // along y: the x-blends of the renderer, differenced over y, blended over z
    const float a00 = v[0] + C.wx * e00, a10 = v[2] + C.wx * e10, a01 = v[4] + C.wx * e01, a11 = v[6] + C.wx * e11;
    const float ey0 = a10 - a00, ey1 = a11 - a01;
    const float gy = ey0 + C.wz * (ey1 - ey0);
    // along z: the two xy-blends of the renderer, differenced
    const float b0 = a00 + C.wy * ey0, b1 = a01 + C.wy * ey1;
    const float g[3] = {gx, gy, b1 - b0};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      acc[a] += g[a];
#pragma unroll
      for (int b = 0; b < 3; ++b) acc[3 + 3 * a + b] += g[a] * (C.p[b] - pv[b]);
    }
  }
#pragma unroll
  for (int k = 0; k < DRR_GRAD_N; ++k) acc[k] *= sm.w;
}

// grid = (ceil(W / 16), ceil(H / 16), views); scratch [views][n_obj][tiles][12], tiles = gridDim.x gridDim.y
__global__ __launch_bounds__(256) void drr_grad_kernel(DrrGradParams P) {
  __shared__ double lds[4 * DRR_GRAD_N];
  const DrrScene& S = P.S;
  int col, row;
  drr_tile_pixel(col, row);
  const int view = blockIdx.z;
  const bool inside = col < S.W && row < S.H;                // no thread leaves early: all of them meet at the barriers
  const float c = (float)col, r = (float)row;
  const float s = drr_ray_scale(S.q, c, r);
  const float da = inside ? P.d_att[((size_t)view * S.H + row) * S.W + col] : 0.f;
  const dfl_drr_object* obs = S.objects + (size_t)view * S.n_obj;
  const size_t tiles = (size_t)gridDim.x * gridDim.y, tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  for (int n = 0; n < S.n_obj; ++n) {
    float acc[DRR_GRAD_N];
#pragma unroll
    for (int k = 0; k < DRR_GRAD_N; ++k) acc[k] = 0.f;
    if (da != 0.f) drr_grad_object(S, obs[n], P.pivots + ((size_t)view * S.n_obj + n) * 3, c, r, s, acc);
    double sum[DRR_GRAD_N];
#pragma unroll
    for (int k = 0; k < DRR_GRAD_N; ++k) sum[k] = da != 0.f ? (double)(da * acc[k]) : 0.0;
    block_sum<DRR_GRAD_N>(sum, lds);
    if (threadIdx.x == 0) {
      double* rec = P.scratch + (((size_t)view * S.n_obj + n) * tiles + tile) * DRR_GRAD_N;
#pragma unroll
      for (int k = 0; k < DRR_GRAD_N; ++k) rec[k] = sum[k];
    }
    __syncthreads();                                         // the next object writes lds again
  }
}

// One workgroup of 64 per (view, object): lanes 0..11 add one of the twelve numbers each over the tiles, in index order
__global__ __launch_bounds__(64) void drr_grad_finish_kernel(const double* __restrict__ scratch, double* __restrict__ grad, int tiles) {
  if (threadIdx.x < DRR_GRAD_N)
    grad[(size_t)blockIdx.x * DRR_GRAD_N + threadIdx.x] =
        records_sum(scratch + (size_t)blockIdx.x * tiles * DRR_GRAD_N + threadIdx.x, tiles, DRR_GRAD_N);
}

// records of one call of sizes that drr_sizes_ok admits, or -1: more than 2^31 - 1 doubles
inline int64_t drr_grad_need(int64_t views, int64_t n_obj, int64_t H, int64_t W) {
  const int64_t tiles = ceil_div(W, 16) * ceil_div(H, 16);
  if (tiles >= ((int64_t)1 << 31) / DRR_GRAD_N || views * n_obj >= ((int64_t)1 << 31) / (tiles * DRR_GRAD_N)) return -1;
  return views * n_obj * tiles * DRR_GRAD_N;
}

}  // namespace dfl

extern "C" int dfl_drr_pose_grad_scratch_doubles(int32_t views, int32_t n_obj, int32_t H, int32_t W) {
  // the volume is not this function's business; its own message replaces the one drr_sizes_ok leaves
  const int64_t need = dfl::drr_sizes_ok("", 1, 1, 1, H, W, views, n_obj) == DFL_OK ? dfl::drr_grad_need(views, n_obj, H, W) : -1;
  if (need < 0) {
    dfl::set_error("dfl_drr_pose_grad_scratch_doubles: bad sizes (views %d of 1..65535, objects %d, detector %d x %d), or more than 2^31 - 1 "
                   "doubles", views, n_obj, H, W);
    return DFL_ERR_INVALID_ARG;
  }
  return (int)need;
}

extern "C" int dfl_drr_pose_grad(const dfl_drr_pose_grad_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_drr_pose_grad: null args");
  DFL_REQUIRE(a->mu != nullptr && a->labels != nullptr && a->objects != nullptr && a->d_att != nullptr && a->pivots != nullptr &&
                  a->grad != nullptr && a->scratch != nullptr,
              "dfl_drr_pose_grad: mu, labels, objects, d_att, pivots, grad and scratch are required");
  const int rc = dfl::drr_sizes_ok("dfl_drr_pose_grad", a->nx, a->ny, a->nz, a->H, a->W, a->views, a->n_obj);
  if (rc != DFL_OK) return rc;
  DFL_REQUIRE(a->interp == DFL_DRR_TRILINEAR, "dfl_drr_pose_grad: interp %d: the gradient exists for trilinear interpolation (1) alone",
              a->interp);
  DFL_REQUIRE(a->step_mm > 0.f && a->step_mm < __builtin_inff(), "dfl_drr_pose_grad: step_mm must be positive, got %g", (double)a->step_mm);
  const int64_t need = dfl::drr_grad_need(a->views, a->n_obj, a->H, a->W);
  DFL_REQUIRE(need >= 0, "dfl_drr_pose_grad: %d views of %d objects on %d x %d need more than 2^31 - 1 doubles of scratch", a->views, a->n_obj,
              a->H, a->W);
  DFL_REQUIRE(a->scratch_doubles >= need, "dfl_drr_pose_grad: a scratch of %lld doubles, %lld are needed (dfl_drr_pose_grad_scratch_doubles)",
              (long long)a->scratch_doubles, (long long)need);
  const dfl::DrrGradParams P = {dfl::drr_scene_of(a), a->d_att, a->pivots, a->scratch};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)dfl::ceil_div(a->W, 16), (unsigned)dfl::ceil_div(a->H, 16), (unsigned)a->views);
  dfl::drr_grad_kernel<<<grid, 256, 0, s>>>(P);
  dfl::drr_grad_finish_kernel<<<(unsigned)(a->views * a->n_obj), 64, 0, s>>>(a->scratch, a->grad, (int)(grid.x * grid.y));
  return dfl::check_launch("dfl_drr_pose_grad");
}
