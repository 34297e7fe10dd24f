// What csrc/sim.hip (global gradient-NCC) and csrc/sim_patch.hip (patch-wise gradient-NCC) share: the Sobel gradients, the
// five fixed and the six moving sums of a counted pixel, the NCC of one-pass sums with its variance rule, the checks
// on sizes and which image of a bank a view belongs to; the fixed-order sums of a workgroup are csrc/fixed_sum.h.  One definition, so that both files give the same bits.
#pragma once
#include "fixed_sum.h"

namespace dfl {

constexpr int SIM_THREADS = 256;
constexpr int SIM_FIXED = 5;         // n, sum fx, fx^2, fy, fy^2 (DFL_SIM_TOTALS)
constexpr int SIM_MOVING = 6;        // sum mx, mx^2, mx fx, my, my^2, my fy

// the checks on sizes that the entry points of csrc/sim.hip share; `who` names the entry point in the message
inline int sim_sizes_ok(const char* who, int V, int H, int W) {
  DFL_REQUIRE(H >= 3 && W >= 3, "%s: an image of %d x %d (at least 3 x 3)", who, H, W);
  DFL_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "%s: an image of %d x %d is too large", who, H, W);
  DFL_REQUIRE(V >= 1 && V <= 65535, "%s: 1..65535 views per call, got %d", who, V);
  return DFL_OK;
}

// ... and of a bank of F fixed images (the *_bank_* entry points)
inline int sim_bank_ok(const char* who, const void* fixed_of, int F, int H, int W) {
  DFL_REQUIRE(fixed_of != nullptr, "%s: fixed_of is required", who);
  DFL_REQUIRE(F >= 1 && F <= 65535, "%s: a bank of 1..65535 fixed images, got %d", who, F);
  DFL_REQUIRE((int64_t)F * H * W < ((int64_t)1 << 31), "%s: a bank of %d images of %d x %d is too large (2^31 pixels or more)", who, F, H, W);
  return DFL_OK;
}

// Which fixed image a view is scored against: 0 for the single-image entry points (fixed_of == nullptr), fixed_of[view] for
// a bank of F images, and -1 when that is outside [0, F): such a view reads nothing from the banks
__device__ __forceinline__ int sim_image_of(const int32_t* __restrict__ fixed_of, int view, int F) {
  if (fixed_of == nullptr) return 0;
  const int f = fixed_of[view];
  return f >= 0 && f < F ? f : -1;
}

// Sobel gradients of a 3 x 3 window (a b c / d . f / g h i): each sum left to right, so the fixed and the moving image share bits
__device__ __forceinline__ void sim_sobel9(float a, float b, float c, float d, float f, float g, float h, float i, float& gx, float& gy) {
  gx = ((c + 2.f * f) + i) - ((a + 2.f * d) + g);
  gy = ((g + 2.f * h) + i) - ((a + 2.f * b) + c);
}

// ... of p at interior pixel (r, c)
__device__ __forceinline__ void sim_sobel(const float* __restrict__ p, int W, int r, int c, float& gx, float& gy) {
  const float* up = p + (size_t)(r - 1) * W + c;
  const float* mid = up + W;
  const float* dn = mid + W;
  sim_sobel9(up[-1], up[0], up[1], mid[-1], mid[1], dn[-1], dn[0], dn[1], gx, gy);
}

// a counted pixel with fixed gradients (gx, gy) joins the five fixed sums
__device__ __forceinline__ void sim_fixed_sums(double (&s)[SIM_FIXED], float gx, float gy) {
  const double x = (double)gx, y = (double)gy;
  s[0] += 1.0;
  s[1] += x;
  s[2] += x * x;
  s[3] += y;
  s[4] += y * y;
}

// counted pixel (r, c) of the moving image joins the six moving sums
__device__ __forceinline__ void sim_moving_sums(double (&s)[SIM_MOVING], const float* __restrict__ img, const float* __restrict__ fx,
                                                const float* __restrict__ fy, int W, int r, int c) {
  const size_t at = (size_t)r * W + c;
  float gx, gy;
  sim_sobel(img, W, r, c, gx, gy);
  const double mx = (double)gx, my = (double)gy;
  s[0] += mx;
  s[1] += mx * mx;
  s[2] += mx * (double)fx[at];
  s[3] += my;
  s[4] += my * my;
  s[5] += my * (double)fy[at];
}

// The variance of one-pass sums (n values, sum s, sum of squares ss), and whether it is live: a variance is 0 when it is
// at most 2^-40 of the sum of squares, since below that the one-pass form cannot tell
__device__ __forceinline__ double sim_var(double n, double s, double ss) { return ss - s * s / n; }
__device__ __forceinline__ bool sim_live(double var, double ss) { return var > 9.094947017729282e-13 * ss; }

__device__ __forceinline__ double sim_ncc(double n, double sa, double saa, double sb, double sbb, double sab) {
  const double va = sim_var(n, sa, saa), vb = sim_var(n, sb, sbb);
  if (!sim_live(va, saa) || !sim_live(vb, sbb)) return 0.0;
  return (sab - sa * sb / n) / sqrt(va * vb);
}

}  // namespace dfl
