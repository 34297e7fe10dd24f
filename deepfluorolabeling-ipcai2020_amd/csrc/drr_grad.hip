// The pose gradient of the trilinear DRR with its sampling frozen: per view and object the force F and the moment Mom
// about a pivot that a detector-space adjoint d_att exerts on the object.
// Contract: include/dfl_hip.h (dfl_drr_pose_grad_args); the semantics are stated in DESIGN.md section 19 and restated
// in numpy by tests/grad_ref.py.
//
// One thread per ray and view in the renderer's 8 x 8-tile-per-wave mapping, so that the eight gathers of a sample hit
// the lines its neighbours hit.  A thread walks the samples drr_trilinear_object took (the same clip, N and t_k: csrc/drr.h),
// and per sample takes the gradient of the trilinear interpolant in the cell drr_corner picked: per axis the bilinear
// blend of the four corner differences, 0 where the corners were clamped together.  Twelve float32 sums per ray and
// object (grad f, and grad f times the sample's offset from the pivot -- about 20 voxels, never the 800 mm of t), scaled
// by d_att s (t1 - t0) / N, promoted to float64, added across the wave with shuffles and across the four waves through
// LDS; ONE record of twelve doubles per workgroup and object with plain stores.  drr_grad_finish_kernel adds the records
// of a view and object in index order.  No atomics: the bits depend on that view's records, pivots and d_att only.
// Bound by the eight dependent gathers per sample, as the renderer is; the arithmetic on top is about 40 flops.
#include "drr.h"

namespace dfl {

constexpr int DRR_GRAD_N = 12;               // F[3], then Mom[3][3] row-major

struct DrrGradParams {
  const float* mu;
  const unsigned char* labels;
  const dfl_drr_object* objects;
  const float* d_att;
  const float* pivots;
  double* scratch;
  float q[9];
  int nx, ny, nz, H, W, n_obj;
  float step_mm;
};

// mu of voxel (x, y, z) if its label is admitted, else 0; the indices are inside the volume
__device__ __forceinline__ float drr_grad_masked(const DrrGradParams& P, uint32_t mask, int x, int y, int z) {
  const int idx = (z * P.ny + y) * P.nx + x;
  const uint32_t lab = P.labels[idx];
  return lab < (uint32_t)DRR_NL && ((mask >> lab) & 1u) != 0u ? P.mu[idx] : 0.f;
}

// acc[0..2] = w sum_k grad f(x_k), acc[3 + 3 a + b] = w sum_k grad f_a(x_k) (x_k - pivot)_b; zeros when the ray misses
__device__ __forceinline__ void drr_grad_object(const DrrGradParams& P, const dfl_drr_object& ob, const float* pivot, float c, float r,
                                                float s, float (&acc)[DRR_GRAD_N]) {
#pragma unroll
  for (int k = 0; k < DRR_GRAD_N; ++k) acc[k] = 0.f;
  const float o[3] = {ob.o[0], ob.o[1], ob.o[2]};
  const float d[3] = {drr_dot(ob.M, c, r), drr_dot(ob.M + 3, c, r), drr_dot(ob.M + 6, c, r)};
  const int lo[3] = {max(ob.box_lo[0], 0), max(ob.box_lo[1], 0), max(ob.box_lo[2], 0)};
  const int hi[3] = {min(ob.box_hi[0], P.nx - 1), min(ob.box_hi[1], P.ny - 1), min(ob.box_hi[2], P.nz - 1)};
  if (hi[0] < lo[0] || hi[1] < lo[1] || hi[2] < lo[2]) return;
  float t0 = 0.f, t1 = __builtin_inff();
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) ok = drr_clip(o[a], d[a], lo[a], hi[a], t0, t1) && ok;
  if (!ok || !(t1 > t0) || !(t1 < __builtin_inff())) return;
  const float span = t1 - t0;
  const float nf = fmaxf(1.f, ceilf(s * span / P.step_mm));
  const int N = (int)fminf(nf, 2147483520.f);
  const float dt = span / nf;
  const uint32_t mask = ob.mask;
  const float pv[3] = {pivot[0], pivot[1], pivot[2]};
  for (int j = 0; j < N; ++j) {
    const float t = t0 + ((float)j + 0.5f) * dt;
    const float px = o[0] + t * d[0], py = o[1] + t * d[1], pz = o[2] + t * d[2];
    int x0, x1, y0, y1, z0, z1;
    float wx, wy, wz;
    drr_corner(px, P.nx, x0, x1, wx);
    drr_corner(py, P.ny, y0, y1, wy);
    drr_corner(pz, P.nz, z0, z1, wz);
    const float v000 = drr_grad_masked(P, mask, x0, y0, z0), v100 = drr_grad_masked(P, mask, x1, y0, z0);
    const float v010 = drr_grad_masked(P, mask, x0, y1, z0), v110 = drr_grad_masked(P, mask, x1, y1, z0);
    const float v001 = drr_grad_masked(P, mask, x0, y0, z1), v101 = drr_grad_masked(P, mask, x1, y0, z1);
    const float v011 = drr_grad_masked(P, mask, x0, y1, z1), v111 = drr_grad_masked(P, mask, x1, y1, z1);
    // along x: the four corner differences, blended over y and z
    const float e00 = v100 - v000, e10 = v110 - v010, e01 = v101 - v001, e11 = v111 - v011;
    const float ex0 = e00 + wy * (e10 - e00), ex1 = e01 + wy * (e11 - e01);
    const float gx = ex0 + wz * (ex1 - ex0);
    // along y: the x-blends of the renderer, differenced over y, blended over z
    const float a00 = v000 + wx * e00, a10 = v010 + wx * e10, a01 = v001 + wx * e01, a11 = v011 + wx * e11;
    const float ey0 = a10 - a00, ey1 = a11 - a01;
    const float gy = ey0 + wz * (ey1 - ey0);
    // along z: the two xy-blends of the renderer, differenced
    const float b0 = a00 + wy * ey0, b1 = a01 + wy * ey1;
    const float gz = b1 - b0;
    const float rx = px - pv[0], ry = py - pv[1], rz = pz - pv[2];
    acc[0] += gx;
    acc[1] += gy;
    acc[2] += gz;
    acc[3] += gx * rx;
    acc[4] += gx * ry;
    acc[5] += gx * rz;
    acc[6] += gy * rx;
    acc[7] += gy * ry;
    acc[8] += gy * rz;
    acc[9] += gz * rx;
    acc[10] += gz * ry;
    acc[11] += gz * rz;
  }
  const float w = s * span / nf;
#pragma unroll
  for (int k = 0; k < DRR_GRAD_N; ++k) acc[k] *= w;
}

__device__ __forceinline__ double drr_grad_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// grid = (ceil(W / 16), ceil(H / 16), views); scratch [views][n_obj][tiles][12], tiles = gridDim.x gridDim.y
__global__ __launch_bounds__(256) void drr_grad_kernel(DrrGradParams P) {
  __shared__ double lds[4 * DRR_GRAD_N];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  const int row = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
  const int view = blockIdx.z;
  const bool inside = col < P.W && row < P.H;                // no thread leaves early: all of them meet at the barriers
  const float c = (float)col, r = (float)row;
  const float qx = drr_dot(P.q, c, r), qy = drr_dot(P.q + 3, c, r), qz = drr_dot(P.q + 6, c, r);
  const float s = sqrtf(qx * qx + qy * qy + qz * qz);
  const float da = inside ? P.d_att[((size_t)view * P.H + row) * P.W + col] : 0.f;
  const dfl_drr_object* obs = P.objects + (size_t)view * P.n_obj;
  const size_t tiles = (size_t)gridDim.x * gridDim.y, tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  for (int n = 0; n < P.n_obj; ++n) {
    float acc[DRR_GRAD_N];
#pragma unroll
    for (int k = 0; k < DRR_GRAD_N; ++k) acc[k] = 0.f;
    if (da != 0.f) drr_grad_object(P, obs[n], P.pivots + ((size_t)view * P.n_obj + n) * 3, c, r, s, acc);
    double sum[DRR_GRAD_N];
#pragma unroll
    for (int k = 0; k < DRR_GRAD_N; ++k) sum[k] = drr_grad_wave_sum(da != 0.f ? (double)(da * acc[k]) : 0.0);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < DRR_GRAD_N; ++k) lds[wave * DRR_GRAD_N + k] = sum[k];
    }
    __syncthreads();
    if (threadIdx.x < DRR_GRAD_N) {
      const int k = threadIdx.x;
      double* rec = P.scratch + (((size_t)view * P.n_obj + n) * tiles + tile) * DRR_GRAD_N;
      rec[k] = ((lds[k] + lds[DRR_GRAD_N + k]) + lds[2 * DRR_GRAD_N + k]) + lds[3 * DRR_GRAD_N + k];
    }
    __syncthreads();                                         // the next object writes lds again
  }
}

// One workgroup of 64 per (view, object): lanes 0..11 add one of the twelve numbers each over the tiles, in index order
__global__ __launch_bounds__(64) void drr_grad_finish_kernel(const double* __restrict__ scratch, double* __restrict__ grad, int tiles) {
  if (threadIdx.x < DRR_GRAD_N) {
    const double* rec = scratch + (size_t)blockIdx.x * tiles * DRR_GRAD_N + threadIdx.x;
    double acc = 0.0;
    for (int t = 0; t < tiles; ++t) acc += rec[(size_t)t * DRR_GRAD_N];
    grad[(size_t)blockIdx.x * DRR_GRAD_N + threadIdx.x] = acc;
  }
}

// records of one call, or -1: sizes dfl_drr_render refuses, or more than 2^31 - 1 doubles
inline int64_t drr_grad_need(int64_t views, int64_t n_obj, int64_t H, int64_t W) {
  if (views < 1 || views > 65535 || n_obj < 1 || H < 1 || W < 1 || H * W >= ((int64_t)1 << 31) || H > 65535 * 4) return -1;
  const int64_t tiles = ceil_div(W, 16) * ceil_div(H, 16);
  if (tiles >= ((int64_t)1 << 31) / DRR_GRAD_N || views * n_obj >= ((int64_t)1 << 31) / (tiles * DRR_GRAD_N)) return -1;
  return views * n_obj * tiles * DRR_GRAD_N;
}

}  // namespace dfl

extern "C" int dfl_drr_pose_grad_scratch_doubles(int32_t views, int32_t n_obj, int32_t H, int32_t W) {
  const int64_t need = dfl::drr_grad_need(views, n_obj, H, W);
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
  DFL_REQUIRE(a->nx >= 1 && a->ny >= 1 && a->nz >= 1 && a->H >= 1 && a->W >= 1 && a->views >= 1 && a->n_obj >= 1,
              "dfl_drr_pose_grad: bad sizes (volume %d x %d x %d, detector %d x %d, views %d, objects %d)", a->nx, a->ny, a->nz, a->H, a->W,
              a->views, a->n_obj);
  DFL_REQUIRE((int64_t)a->nx * a->ny * a->nz < ((int64_t)1 << 31), "dfl_drr_pose_grad: a volume of %d x %d x %d exceeds 2^31 voxels", a->nx,
              a->ny, a->nz);
  DFL_REQUIRE(a->views <= 65535, "dfl_drr_pose_grad: at most 65535 views per call, got %d", a->views);
  DFL_REQUIRE((int64_t)a->H * a->W < ((int64_t)1 << 31) && a->H <= 65535 * 4, "dfl_drr_pose_grad: a detector of %d x %d is too large", a->H,
              a->W);
  DFL_REQUIRE(a->interp == DFL_DRR_TRILINEAR, "dfl_drr_pose_grad: interp %d: the gradient exists for trilinear interpolation (1) alone",
              a->interp);
  DFL_REQUIRE(a->step_mm > 0.f && a->step_mm < __builtin_inff(), "dfl_drr_pose_grad: step_mm must be positive, got %g", (double)a->step_mm);
  const int64_t need = dfl::drr_grad_need(a->views, a->n_obj, a->H, a->W);
  DFL_REQUIRE(need >= 0, "dfl_drr_pose_grad: %d views of %d objects on %d x %d need more than 2^31 - 1 doubles of scratch", a->views, a->n_obj,
              a->H, a->W);
  DFL_REQUIRE(a->scratch_doubles >= need, "dfl_drr_pose_grad: a scratch of %lld doubles, %lld are needed (dfl_drr_pose_grad_scratch_doubles)",
              (long long)a->scratch_doubles, (long long)need);
  dfl::DrrGradParams P;
  P.mu = a->mu;
  P.labels = a->labels;
  P.objects = a->objects;
  P.d_att = a->d_att;
  P.pivots = a->pivots;
  P.scratch = a->scratch;
  for (int k = 0; k < 9; ++k) P.q[k] = a->qscale[k];
  P.nx = a->nx;
  P.ny = a->ny;
  P.nz = a->nz;
  P.H = a->H;
  P.W = a->W;
  P.n_obj = a->n_obj;
  P.step_mm = a->step_mm;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)dfl::ceil_div(a->W, 16), (unsigned)dfl::ceil_div(a->H, 16), (unsigned)a->views);
  dfl::drr_grad_kernel<<<grid, 256, 0, s>>>(P);
  dfl::drr_grad_finish_kernel<<<(unsigned)(a->views * a->n_obj), 64, 0, s>>>(a->scratch, a->grad, (int)(grid.x * grid.y));
  return dfl::check_launch("dfl_drr_pose_grad");
}
