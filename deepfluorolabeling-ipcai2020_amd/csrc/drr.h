// What csrc/drr.hip (the renderer) and csrc/drr_grad.hip (its pose gradient) share: the ray of a pixel, the clip of a
// ray to an object's box and the corners of a trilinear sample.  One definition, so that the gradient walks exactly the
// samples the renderer took.
#pragma once
#include "common.h"

namespace dfl {

constexpr int DRR_NL = DFL_DRR_MAX_LABELS;

__device__ __forceinline__ float drr_dot(const float* m, float c, float r) { return m[0] * c + m[1] * r + m[2]; }

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

__device__ __forceinline__ void drr_corner(float p, int n, int& i0, int& i1, float& w) {
  const float q = fminf(fmaxf(p, -2.f), (float)n + 1.f);
  const float f = floorf(q);
  w = q - f;
  i0 = min(max((int)f, 0), n - 1);
  i1 = min(max((int)f + 1, 0), n - 1);
}

}  // namespace dfl
