// What csrc/drr.hip (the renderer) and csrc/drr_grad.hip (its pose gradient) share: the scene both walk, the pixel of a
// thread, the ray of a pixel clipped to an object's box, the placement of the trilinear samples on it and the eight
// masked loads of one sample.  One definition, so that the gradient walks exactly the samples the renderer took.
#pragma once
#include "common.h"

namespace dfl {

constexpr int DRR_NL = DFL_DRR_MAX_LABELS;

// What every walker reads: the volume, the objects of every view and the detector
struct DrrScene {
  const float* mu;
  const unsigned char* labels;
  const dfl_drr_object* objects;
  float q[9];
  int nx, ny, nz, H, W, n_obj;
  float step_mm;
};

// from dfl_drr_args or dfl_drr_pose_grad_args
template <class Args>
inline DrrScene drr_scene_of(const Args* a) {
  DrrScene S = {a->mu, a->labels, a->objects, {}, a->nx, a->ny, a->nz, a->H, a->W, a->n_obj, a->step_mm};
  for (int k = 0; k < 9; ++k) S.q[k] = a->qscale[k];
  return S;
}

// the checks on sizes that dfl_drr_render and dfl_drr_pose_grad share; `who` names the entry point in the message
inline int drr_sizes_ok(const char* who, int nx, int ny, int nz, int H, int W, int views, int n_obj) {
  DFL_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1 && H >= 1 && W >= 1 && views >= 1 && n_obj >= 1,
              "%s: bad sizes (volume %d x %d x %d, detector %d x %d, views %d, objects %d)", who, nx, ny, nz, H, W, views, n_obj);
  DFL_REQUIRE((int64_t)nx * ny * nz < ((int64_t)1 << 31), "%s: a volume of %d x %d x %d exceeds 2^31 voxels", who, nx, ny, nz);
  DFL_REQUIRE(views <= 65535, "%s: at most 65535 views per call, got %d", who, views);
  DFL_REQUIRE((int64_t)H * W < ((int64_t)1 << 31) && H <= 65535 * 4, "%s: a detector of %d x %d is too large", who, H, W);
  return DFL_OK;
}

__device__ __forceinline__ float drr_dot(const float* m, float c, float r) { return m[0] * c + m[1] * r + m[2]; }

// The pixel of a thread: a wave covers an 8 x 8 tile (lane & 7, lane >> 3), a workgroup of four waves 16 x 16
__device__ __forceinline__ void drr_tile_pixel(int& col, int& row) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  col = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  row = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
}

// mm per unit of t on the ray of pixel (c, r)
__device__ __forceinline__ float drr_ray_scale(const float* q, float c, float r) {
  const float qx = drr_dot(q, c, r), qy = drr_dot(q + 3, c, r), qz = drr_dot(q + 6, c, r);
  return sqrtf(qx * qx + qy * qy + qz * qz);
}

// t of plane k of one axis: the plane between voxels k - 1 and k
__device__ __forceinline__ float drr_plane(int k, float o, float d) { return ((float)k - 0.5f - o) / d; }

// Clip [t0, t1] to the slab [lo - 1/2, hi + 1/2] of one axis; false: the ray misses it
__device__ __forceinline__ bool drr_clip(float o, float d, int lo, int hi, float& t0, float& t1) {
  if (d == 0.f) return o >= (float)lo - 0.5f && o < (float)hi + 0.5f;
  const float ta = drr_plane(lo, o, d), tb = drr_plane(hi + 1, o, d);
  t0 = fmaxf(t0, fminf(ta, tb));
  t1 = fminf(t1, fmaxf(ta, tb));
  return true;
}

// The ray o + t d of a pixel through an object, t0 < t < t1 inside the object's box [lo, hi] clamped to the volume
struct DrrRay {
  float o[3], d[3];
  int lo[3], hi[3];
  float t0, t1;
};

// false: the ray misses the box, the box is empty, or t1 is not finite (a NaN in o or d counts as a miss)
__device__ __forceinline__ bool drr_ray(const dfl_drr_object& ob, int nx, int ny, int nz, float c, float r, DrrRay& R) {
  const int n[3] = {nx, ny, nz};
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    R.o[a] = ob.o[a];
    R.d[a] = drr_dot(ob.M + 3 * a, c, r);
    R.lo[a] = max(ob.box_lo[a], 0);
    R.hi[a] = min(ob.box_hi[a], n[a] - 1);
    ok = ok && R.hi[a] >= R.lo[a];
  }
  if (!ok) return false;
  R.t0 = 0.f;
  R.t1 = __builtin_inff();
#pragma unroll
  for (int a = 0; a < 3; ++a) ok = drr_clip(R.o[a], R.d[a], R.lo[a], R.hi[a], R.t0, R.t1) && ok;
  return ok && R.t1 > R.t0 && R.t1 < __builtin_inff();
}

// The trilinear samples of a ray: N of them at t0 + (j + 1/2) dt, each standing for w mm (s: mm per unit of t)
struct DrrSamples {
  int N;
  float dt, w;
};

__device__ __forceinline__ DrrSamples drr_samples(const DrrRay& R, float s, float step_mm) {
  const float span = R.t1 - R.t0;
  const float nf = fmaxf(1.f, ceilf(s * span / step_mm));
  return {(int)fminf(nf, 2147483520.f), span / nf, s * span / nf};
}

__device__ __forceinline__ void drr_corner(float p, int n, int& i0, int& i1, float& w) {
  const float q = fminf(fmaxf(p, -2.f), (float)n + 1.f);
  const float f = floorf(q);
  w = q - f;
  i0 = min(max((int)f, 0), n - 1);
  i1 = min(max((int)f + 1, 0), n - 1);
}

// mu of voxel (x, y, z) if its label is admitted, else 0; the indices are inside the volume
__device__ __forceinline__ float drr_masked(const DrrScene& S, uint32_t mask, int x, int y, int z) {
  const int idx = (z * S.ny + y) * S.nx + x;
  const uint32_t lab = S.labels[idx];
  return lab < (uint32_t)DRR_NL && ((mask >> lab) & 1u) != 0u ? S.mu[idx] : 0.f;
}

// One trilinear sample: the point p = o + t d, the masked values v[x + 2 y + 4 z] of the eight corners of its cell and the
// weights of the upper corners.  The renderer blends the values, the gradient differences them.
struct DrrCell {
  float p[3], v[8], wx, wy, wz;
};

__device__ __forceinline__ void drr_gather(const DrrScene& S, uint32_t mask, const DrrRay& R, float t, DrrCell& C) {
  int x[2], y[2], z[2];
#pragma unroll
  for (int a = 0; a < 3; ++a) C.p[a] = R.o[a] + t * R.d[a];
  drr_corner(C.p[0], S.nx, x[0], x[1], C.wx);
  drr_corner(C.p[1], S.ny, y[0], y[1], C.wy);
  drr_corner(C.p[2], S.nz, z[0], z[1], C.wz);
#pragma unroll
  for (int k = 0; k < 8; ++k) C.v[k] = drr_masked(S, mask, x[k & 1], y[(k >> 1) & 1], z[k >> 2]);
}

}  // namespace dfl
