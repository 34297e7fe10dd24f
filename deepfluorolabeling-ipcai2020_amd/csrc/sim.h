// What csrc/sim.hip (global gradient-NCC) and csrc/sim_patch.hip (patch-wise gradient-NCC) share: the Sobel gradients, the
// five fixed and the six moving sums of a counted pixel, the NCC of one-pass sums with its variance rule, the checks
// on sizes and which image of a bank a view belongs to, the two phases of a patch row, the coefficients of the adjoint and the
// tile body of the two adjoint kernels; the fixed-order sums of a workgroup are csrc/fixed_sum.h.  One definition, so that both
// files give the same bits.
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

// the Sobel planes and the counted-pixel plane of image f of a bank
__device__ __forceinline__ void sim_planes_of(const float* __restrict__& fx, const float* __restrict__& fy,
                                              const unsigned char* __restrict__& counted, int f, int H, int W) {
  const size_t plane = (size_t)f * H * W;
  fx += plane;
  fy += plane;
  counted += plane;
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

// ---- the two phases of a patch row (sim_patch_prepare_kernel: N = 5, sim_patch_gradncc_kernel: N = 6; csrc/sim_patch.hip) ----------
// Phase 1: thread t takes the interior columns t, t + 256, ... and adds the N sums of pixel(s, r, c) down the S rows from r0,
// row by row, into cols [N][W - 2]
template <int N, typename Pixel>
__device__ __forceinline__ void sim_column_sums(double* __restrict__ cols, int wi, int r0, int S, Pixel&& pixel) {
  for (int j = threadIdx.x; j < wi; j += SIM_THREADS) {
    double s[N] = {};
    for (int k = 0; k < S; ++k) pixel(s, r0 + k, 1 + j);
#pragma unroll
    for (int q = 0; q < N; ++q) cols[q * wi + j] = s[q];
  }
}

// Phase 2: the N sums of the patch whose first interior column is j0, over its S column sums in index order
template <int N>
__device__ __forceinline__ void sim_patch_sums(double (&s)[N], const double* __restrict__ cols, int wi, int j0, int S) {
#pragma unroll
  for (int q = 0; q < N; ++q) s[q] = 0.0;
  for (int k = 0; k < S; ++k) {
#pragma unroll
    for (int q = 0; q < N; ++q) s[q] += cols[q * wi + j0 + k];
  }
}

// ---- what the two adjoints share (csrc/sim.hip: dfl_sim_gradncc_bwd; csrc/sim_patch.hip: dfl_sim_patch_eval with d_moving) ------------
// With a the moving and b the fixed Sobel values of one direction, d(-ncc / 2) / d a_p = alpha (b_p - mean b) + beta (a_p - mean a)
// at a counted pixel, alpha = -1 / (2 sqrt(va vb)), beta = cab / (2 va sqrt(va vb)); both 0 where the rule of sim_ncc makes the ncc 0.
// The four coefficients of one direction -- share alpha, share beta, mean a, mean b -- formed in float64 and rounded once; share is
// the part of the cost these sums stand for: 1 for the whole image, w / pwsum or 1 / pcount for a patch.  n is not 0.
__device__ __forceinline__ void sim_coef4(float* __restrict__ out, double share, double n, double sa, double saa, double sb, double sbb,
                                          double sab) {
  double ca = 0.0, cb = 0.0, ma = 0.0, mb = 0.0;
  const double va = sim_var(n, sa, saa), vb = sim_var(n, sb, sbb);
  if (sim_live(va, saa) && sim_live(vb, sbb)) {
    const double root = sqrt(va * vb);
    ca = share * (-0.5 / root);
    cb = share * (0.5 * (sab - sa * sb / n) / (va * root));
    ma = sa / n;
    mb = sb / n;
  }
  out[0] = (float)ca;
  out[1] = (float)cb;
  out[2] = (float)ma;
  out[3] = (float)mb;
}

constexpr int SIM_TILE = 16;        // an adjoint kernel's tile of output pixels; 16 x 16 = SIM_THREADS
constexpr int SIM_TILE_IN = SIM_TILE + 4, SIM_TILE_G = SIM_TILE + 2;   // the tile of `moving` with a halo of 2; of g with a halo of 1

// The tile of one view's `moving` at (r0, c0) with a halo of 2 -> LDS, 0 outside the image
__device__ __forceinline__ void sim_stage_tile(float (&sm)[SIM_TILE_IN][SIM_TILE_IN + 1], const float* __restrict__ img, int H, int W, int r0,
                                               int c0) {
  for (int i = threadIdx.x; i < SIM_TILE_IN * SIM_TILE_IN; i += SIM_THREADS) {
    const int lr = i / SIM_TILE_IN, lc = i % SIM_TILE_IN, r = r0 - 2 + lr, c = c0 - 2 + lc;
    sm[lr][lc] = r >= 0 && r < H && c >= 0 && c < W ? img[(size_t)r * W + c] : 0.f;
  }
}

// Sobel^T at output pixel (tr, tc) of the tile from g on the 18 x 18 pixels around it: pixel q is at offset (dr, dc) in the window
// of p = q - (dr, dc), which sits at sg[tr + 1 - dr][tc + 1 - dc]; Sobel x has weight dc (2 - |dr|) there, Sobel y dr (2 - |dc|)
__device__ __forceinline__ float sim_sobel_gather(const float (&sgx)[SIM_TILE_G][SIM_TILE_G + 1], const float (&sgy)[SIM_TILE_G][SIM_TILE_G + 1],
                                                  int tr, int tc) {
#pragma clang fp contract(off)
  const float x = ((sgx[tr + 2][tc] + 2.f * sgx[tr + 1][tc]) + sgx[tr][tc]) - ((sgx[tr + 2][tc + 2] + 2.f * sgx[tr + 1][tc + 2]) + sgx[tr][tc + 2]);
  const float y = ((sgy[tr][tc + 2] + 2.f * sgy[tr][tc + 1]) + sgy[tr][tc]) - ((sgy[tr + 2][tc + 2] + 2.f * sgy[tr + 2][tc + 1]) + sgy[tr + 2][tc]);
  return x + y;
}

// The body of an adjoint kernel: a workgroup of SIM_THREADS owns the 16 x 16 tile (blockIdx.y, blockIdx.x) of d_moving of view
// blockIdx.z.  The tile of `moving` with a halo of 2 goes to LDS (0 outside the image); from it the 18 x 18 pixels around the tile
// get g = d cost / d (Sobel value): g(bx, by, mx, my, r, c, gx, gy) is asked at a counted interior pixel (r, c) with the fixed and
// the moving Sobel values there, and g is 0 elsewhere; every output pixel then gathers the nine pixels whose window holds it with
// the Sobel weight it has there.  A view whose image is outside the bank gets zeros.  `#pragma clang fp contract(off)` is lexical:
// a kernel's g is rounded as the kernel that writes it says.
template <typename G>
__device__ __forceinline__ void sim_adjoint_tile(const float* __restrict__ moving, const float* __restrict__ fx, const float* __restrict__ fy,
                                                 const unsigned char* __restrict__ counted, const int32_t* __restrict__ fixed_of,
                                                 float* __restrict__ d_moving, int H, int W, int F, G&& g) {
  constexpr int IN = SIM_TILE_IN, TG = SIM_TILE_G;
  __shared__ float sm[IN][IN + 1];
  __shared__ float sgx[TG][TG + 1], sgy[TG][TG + 1];
  const int view = blockIdx.z;
  const int r0 = blockIdx.y * SIM_TILE, c0 = blockIdx.x * SIM_TILE;
  const int f = sim_image_of(fixed_of, view, F);
  if (f < 0) {                                                          // the whole workgroup, before its first barrier
    const int r = r0 + threadIdx.x / SIM_TILE, c = c0 + threadIdx.x % SIM_TILE;
    if (r < H && c < W) d_moving[((size_t)view * H + r) * W + c] = 0.f;
    return;
  }
  sim_planes_of(fx, fy, counted, f, H, W);
  sim_stage_tile(sm, moving + (size_t)view * H * W, H, W, r0, c0);
  __syncthreads();
  for (int i = threadIdx.x; i < TG * TG; i += SIM_THREADS) {
    const int lr = i / TG, lc = i % TG, r = r0 - 1 + lr, c = c0 - 1 + lc;
    float gx = 0.f, gy = 0.f;
    if (r >= 1 && r <= H - 2 && c >= 1 && c <= W - 2) {
      const size_t at = (size_t)r * W + c;
      if (counted[at]) {
        // Sobel on the staged tile: pixel (r, c) sits at sm[lr + 1][lc + 1].  sim_sobel9 may fuse x + 2 y whatever the kernel's
        // contraction is; that gives the same bits either way, since 2 y is exact
        float mx, my;
        sim_sobel9(sm[lr][lc], sm[lr][lc + 1], sm[lr][lc + 2], sm[lr + 1][lc], sm[lr + 1][lc + 2], sm[lr + 2][lc], sm[lr + 2][lc + 1],
                   sm[lr + 2][lc + 2], mx, my);
        g(fx[at], fy[at], mx, my, r, c, gx, gy);
      }
    }
    sgx[lr][lc] = gx;
    sgy[lr][lc] = gy;
  }
  __syncthreads();
  const int tr = threadIdx.x / SIM_TILE, tc = threadIdx.x % SIM_TILE, r = r0 + tr, c = c0 + tc;
  if (r < H && c < W) d_moving[((size_t)view * H + r) * W + c] = sim_sobel_gather(sgx, sgy, tr, tc);
}

}  // namespace dfl
