// Mutual information between V rendered views and the fixed images they are scored against, from a joint histogram of
// integers -- the similarity of dfl_amd.register(similarity='mi').
// Contract: include/dfl_hip.h ("Mutual information"); the semantics are stated in DESIGN.md section 29 and restated in
// numpy by tests/mi_ref.py.  This file is compiled with -ffp-contract=off: every float32 step is rounded on its own.
//
// mi_prepare_range_kernel (one workgroup) takes n, min and max of the counted pixels of a fixed image; min and max of
// floats do not depend on the order.  mi_prepare_bins_kernel writes the bin of every pixel.  Neither is hot.
// mi_clear zeroes hist.  mi_hist_kernel: a workgroup owns MI_RUN consecutive pixels of one view (grid = runs x views) and
// thread t takes the pixels t, t + 256, ... of the run, so a wave reads 64 consecutive floats and bytes.  Every wave adds
// into its OWN uint32 histogram in LDS (MI_WAVES x Bm x Bf words, 64 KB at 64 x 64): neighbouring pixels of a radiograph
// fall into the same bin, same-address LDS adds serialise, and private copies keep that serialisation inside one wave
// instead of across four.  A run is 8192 pixels, so a bin holds at most 2^13 * 2^12 = 2^25 before the flush (the limit is
// 2^19 pixels).  The flush adds the non-zero bins, summed over the wave copies, to hist with 64-bit integer atomic adds.
// Integer sums: the bits of hist do not depend on decomposition, batch or arrival order.  No float atomics.
// mi_finish_kernel: one workgroup per view: hist to LDS, integer marginals, thread t adds the terms of the bins t, t + 256,
// ... in that order, a fixed tree over the 256 partial sums; with ell != NULL also the table of the adjoint.
// mi_adjoint_kernel: a workgroup stages the view's table in LDS (32 KB at 64 x 64); two table reads and one store per pixel.
// A void view (range not usable, fixed_of outside [0, F)) leaves every kernel as a whole workgroup before the first barrier.
#include <float.h>

#include "common.h"

namespace dfl {
namespace {

constexpr int MI_THREADS = 256;
constexpr int MI_WAVES = MI_THREADS / 64;
constexpr int MI_RUN = DFL_SIM_MI_RUN;                     // pixels of one view per workgroup
constexpr int MI_UNIT = DFL_SIM_MI_UNIT;
constexpr int MI_MAX = DFL_SIM_MI_MAX_BINS;
constexpr int MI_PREP_THREADS = 1024;
static_assert(MI_RUN % MI_THREADS == 0 && MI_RUN < (1 << 19), "a bin of a run fits 32 bits: 2^19 pixels x 2^12 would not");
static_assert(MI_WAVES * MI_MAX * MI_MAX * 4 <= 65536, "the wave histograms fit the LDS a launch gets without asking");
static_assert(DFL_SIM_MI_SKIP >= MI_MAX, "the skip byte is no bin");

__device__ __forceinline__ bool mi_finite(float x) { return fabsf(x) <= FLT_MAX; }

// The image a view is scored against and its moving range; false: the view is void (the same for the whole workgroup)
__device__ __forceinline__ bool mi_view(const int32_t* __restrict__ fixed_of, const float* __restrict__ mrange, int view, int F, int Bm,
                                        int* f, float* lo, float* hi, float* s) {
  *f = fixed_of == nullptr ? 0 : fixed_of[view];
  if (*f < 0 || *f >= F) return false;
  *lo = mrange[2 * (size_t)*f];
  *hi = mrange[2 * (size_t)*f + 1];
  const float d = *hi - *lo;
  *s = (float)(Bm - 1) / d;
  return mi_finite(*lo) && mi_finite(*hi) && *hi > *lo && mi_finite(d) && mi_finite(*s);
}

// The lower bin a and the weight q of the upper bin a + 1, of 4096, for a moving value inside a usable range
__device__ __forceinline__ void mi_weights(float m, float lo, float hi, float s, int Bm, int* a, int* q) {
  const float c = fminf(fmaxf(m, lo), hi);                 // NaN counts as lo
  const float x = (c - lo) * s;
  *a = x >= (float)(Bm - 1) ? Bm - 2 : (int)floorf(x);
  const float fr = x - (float)*a;
  *q = (int)floorf(fr * (float)MI_UNIT + 0.5f);
}

__global__ __launch_bounds__(MI_PREP_THREADS) void mi_prepare_range_kernel(const float* __restrict__ fixed, const unsigned char* __restrict__ mask,
                                                                           double* __restrict__ info, int64_t HW) {
  __shared__ float s_lo[MI_PREP_THREADS], s_hi[MI_PREP_THREADS];
  __shared__ unsigned int s_n[MI_PREP_THREADS];
  float lo = FLT_MAX, hi = -FLT_MAX;
  unsigned int n = 0;
  for (int64_t p = threadIdx.x; p < HW; p += MI_PREP_THREADS) {
    const float f = fixed[p];
    if (mi_finite(f) && (mask == nullptr || mask[p] != 0)) {
      lo = fminf(lo, f);
      hi = fmaxf(hi, f);
      ++n;
    }
  }
  s_lo[threadIdx.x] = lo;
  s_hi[threadIdx.x] = hi;
  s_n[threadIdx.x] = n;
  __syncthreads();
  for (int w = MI_PREP_THREADS / 2; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) {
      s_lo[threadIdx.x] = fminf(s_lo[threadIdx.x], s_lo[threadIdx.x + w]);
      s_hi[threadIdx.x] = fmaxf(s_hi[threadIdx.x], s_hi[threadIdx.x + w]);
      s_n[threadIdx.x] += s_n[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const bool any = s_n[0] != 0;
    info[0] = (double)s_n[0];
    info[1] = any ? (double)s_lo[0] : 0.0;
    info[2] = any ? (double)s_hi[0] : 0.0;
    info[3] = 0.0;
  }
}

__global__ __launch_bounds__(MI_THREADS) void mi_prepare_bins_kernel(const float* __restrict__ fixed, const unsigned char* __restrict__ mask,
                                                                     const double* __restrict__ info, unsigned char* __restrict__ fbin,
                                                                     int64_t HW, int Bf) {
  const int64_t p = (int64_t)blockIdx.x * MI_THREADS + threadIdx.x;
  if (p >= HW) return;
  const float f = fixed[p];
  int k = DFL_SIM_MI_SKIP;
  if (mi_finite(f) && (mask == nullptr || mask[p] != 0)) {
    const float lo = (float)info[1], hi = (float)info[2];   // floats, stored as doubles
    const float d = hi - lo;
    const float x = (f - lo) * ((float)Bf / d);
    k = !(d > 0.0f) ? 0 : x >= (float)Bf ? Bf - 1 : x > 0.0f ? (int)floorf(x) : 0;
  }
  fbin[p] = (unsigned char)k;
}

__global__ __launch_bounds__(MI_THREADS) void mi_clear(uint64_t* __restrict__ hist, int64_t words) {
  const int64_t i = (int64_t)blockIdx.x * MI_THREADS + threadIdx.x;
  if (i < words) hist[i] = 0;
}

__global__ __launch_bounds__(MI_THREADS) void mi_hist_kernel(const float* __restrict__ moving, const unsigned char* __restrict__ fbin,
                                                             const float* __restrict__ mrange, const int32_t* __restrict__ fixed_of,
                                                             uint64_t* __restrict__ hist, int64_t HW, int F, int Bf, int Bm) {
  extern __shared__ uint32_t mi_lds[];                      // [MI_WAVES][Bm][Bf]
  const int view = blockIdx.y, bins = Bm * Bf;
  int f;
  float lo, hi, s;
  if (!mi_view(fixed_of, mrange, view, F, Bm, &f, &lo, &hi, &s)) return;      // the whole workgroup; mi_clear left zeros
  for (int i = threadIdx.x; i < MI_WAVES * bins; i += MI_THREADS) mi_lds[i] = 0;
  __syncthreads();
  uint32_t* mine = mi_lds + (threadIdx.x >> 6) * bins;
  const int64_t p0 = (int64_t)blockIdx.x * MI_RUN;
  const int64_t end = p0 + MI_RUN < HW ? p0 + MI_RUN : HW;
  const float* __restrict__ mv = moving + (int64_t)view * HW;
  const unsigned char* __restrict__ fb = fbin + (int64_t)f * HW;
  for (int64_t p = p0 + threadIdx.x; p < end; p += MI_THREADS) {
    const int b = fb[p];
    if (b >= Bf) continue;                                  // DFL_SIM_MI_SKIP (and no bin of this Bf)
    int a, q;
    mi_weights(mv[p], lo, hi, s, Bm, &a, &q);
    if (q != MI_UNIT) atomicAdd(&mine[a * Bf + b], (uint32_t)(MI_UNIT - q));
    if (q != 0) atomicAdd(&mine[(a + 1) * Bf + b], (uint32_t)q);
  }
  __syncthreads();
  unsigned long long* out = reinterpret_cast<unsigned long long*>(hist) + (int64_t)view * bins;
  for (int i = threadIdx.x; i < bins; i += MI_THREADS) {
    uint32_t t = 0;
#pragma unroll
    for (int w = 0; w < MI_WAVES; ++w) t += mi_lds[w * bins + i];
    if (t != 0) atomicAdd(&out[i], (unsigned long long)t);
  }
}

__global__ __launch_bounds__(MI_THREADS) void mi_finish_kernel(const uint64_t* __restrict__ hist, const float* __restrict__ mrange,
                                                               const int32_t* __restrict__ fixed_of, double* __restrict__ cost,
                                                               double* __restrict__ ell, int F, int Bf, int Bm) {
  __shared__ uint64_t h[MI_MAX * MI_MAX];
  __shared__ uint64_t ha[MI_MAX], hb[MI_MAX];
  __shared__ double part[MI_THREADS];
  const int view = blockIdx.x, bins = Bm * Bf;
  int f;
  float lo, hi, s;
  if (!mi_view(fixed_of, mrange, view, F, Bm, &f, &lo, &hi, &s)) {            // the whole workgroup
    if (threadIdx.x == 0) cost[view] = __builtin_nan("");
    if (ell != nullptr)
      for (int i = threadIdx.x; i < bins; i += MI_THREADS) ell[(int64_t)view * bins + i] = 0.0;
    return;
  }
  for (int i = threadIdx.x; i < bins; i += MI_THREADS) h[i] = hist[(int64_t)view * bins + i];
  __syncthreads();
  if ((int)threadIdx.x < Bm) {
    uint64_t t = 0;
    for (int b = 0; b < Bf; ++b) t += h[threadIdx.x * Bf + b];
    ha[threadIdx.x] = t;
  } else if ((int)threadIdx.x >= MI_MAX && (int)threadIdx.x < MI_MAX + Bf) {
    const int b = threadIdx.x - MI_MAX;
    uint64_t t = 0;
    for (int a = 0; a < Bm; ++a) t += h[a * Bf + b];
    hb[b] = t;
  }
  __syncthreads();
  uint64_t total = 0;
  for (int a = 0; a < Bm; ++a) total += ha[a];              // 4096 n, an integer
  const double N = (double)total;
  double acc = 0.0;
  for (int i = threadIdx.x; i < bins; i += MI_THREADS) {
    const int a = i / Bf, b = i - a * Bf;
    const uint64_t hv = h[i];
    if (hv > 0) {
      const double hd = (double)hv;
      acc += (hd / N) * log((hd * N) / ((double)ha[a] * (double)hb[b]));
    }
    if (ell != nullptr)
      ell[(int64_t)view * bins + i] = log((double)(hv > 1 ? hv : 1)) - log((double)(ha[a] > 1 ? ha[a] : 1));
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int w = MI_THREADS / 2; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) cost[view] = total > 0 ? -part[0] : 0.0;
}

__global__ __launch_bounds__(MI_THREADS) void mi_adjoint_kernel(const float* __restrict__ moving, const unsigned char* __restrict__ fbin,
                                                                const double* __restrict__ info, const float* __restrict__ mrange,
                                                                const int32_t* __restrict__ fixed_of, const double* __restrict__ ell,
                                                                float* __restrict__ d_moving, int64_t HW, int F, int Bf, int Bm) {
  extern __shared__ double mi_table[];                      // [Bm][Bf]
  const int view = blockIdx.y, bins = Bm * Bf;
  const int64_t p0 = (int64_t)blockIdx.x * MI_RUN;
  const int64_t end = p0 + MI_RUN < HW ? p0 + MI_RUN : HW;
  float* __restrict__ dm = d_moving + (int64_t)view * HW;
  int f;
  float lo, hi, s;
  if (!mi_view(fixed_of, mrange, view, F, Bm, &f, &lo, &hi, &s)) {            // the whole workgroup
    for (int64_t p = p0 + threadIdx.x; p < end; p += MI_THREADS) dm[p] = 0.0f;
    return;
  }
  for (int i = threadIdx.x; i < bins; i += MI_THREADS) mi_table[i] = ell[(int64_t)view * bins + i];
  __syncthreads();
  const double coef = -((double)s / info[(size_t)f * DFL_SIM_MI_INFO]);      // n > 0 wherever a pixel is counted
  const float* __restrict__ mv = moving + (int64_t)view * HW;
  const unsigned char* __restrict__ fb = fbin + (int64_t)f * HW;
  for (int64_t p = p0 + threadIdx.x; p < end; p += MI_THREADS) {
    const int b = fb[p];
    const float m = mv[p];
    float g = 0.0f;
    if (b < Bf && m > lo && m < hi) {
      int a, q;
      mi_weights(m, lo, hi, s, Bm, &a, &q);
      g = (float)(coef * (mi_table[(a + 1) * Bf + b] - mi_table[a * Bf + b]));
    }
    dm[p] = g;
  }
}

int mi_image_ok(const char* who, int32_t H, int32_t W) {
  DFL_REQUIRE(H >= 1 && W >= 1, "%s: bad sizes H=%d W=%d", who, H, W);
  DFL_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "%s: %d x %d pixels: fewer than 2^31 are supported", who, H, W);
  return DFL_OK;
}

int mi_bins_ok(const char* who, const char* name, int32_t B) {
  DFL_REQUIRE(B >= 2 && B <= MI_MAX, "%s: %s = %d bins (2..%d)", who, name, B, MI_MAX);
  return DFL_OK;
}

int mi_sizes_ok(const char* who, int32_t V, int32_t H, int32_t W, int32_t F, int32_t Bf, int32_t Bm) {
  int rc = mi_image_ok(who, H, W);
  if (rc != DFL_OK) return rc;
  DFL_REQUIRE(V >= 1 && V <= 65535, "%s: 1..65535 views per call, got %d", who, V);
  DFL_REQUIRE(F >= 1 && F <= 65535, "%s: a bank of 1..65535 fixed images, got %d", who, F);
  DFL_REQUIRE((int64_t)F * H * W < ((int64_t)1 << 31), "%s: a bank of %d images of %d x %d: fewer than 2^31 pixels are supported", who, F, H, W);
  rc = mi_bins_ok(who, "Bf", Bf);
  if (rc != DFL_OK) return rc;
  return mi_bins_ok(who, "Bm", Bm);
}

// clear, histogram, finish: what dfl_sim_mi and dfl_sim_mi_bwd share, so that cost and hist have the same bits in both
void mi_forward(const float* moving, const unsigned char* fbin, const float* mrange, const int32_t* fixed_of, uint64_t* hist, double* cost,
                double* ell, int V, int64_t HW, int F, int Bf, int Bm, hipStream_t s) {
  const int64_t words = (int64_t)V * Bm * Bf;               // <= 65535 * 4096
  const unsigned runs = (unsigned)ceil_div(HW, MI_RUN);     // < 2^18
  mi_clear<<<(unsigned)ceil_div(words, MI_THREADS), MI_THREADS, 0, s>>>(hist, words);
  mi_hist_kernel<<<dim3(runs, (unsigned)V), MI_THREADS, (size_t)MI_WAVES * Bm * Bf * sizeof(uint32_t), s>>>(moving, fbin, mrange, fixed_of, hist, HW,
                                                                                                           F, Bf, Bm);
  mi_finish_kernel<<<(unsigned)V, MI_THREADS, 0, s>>>(hist, mrange, fixed_of, cost, ell, F, Bf, Bm);
}

}  // namespace
}  // namespace dfl

using namespace dfl;

extern "C" int dfl_sim_mi_prepare(const dfl_sim_mi_prepare_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_sim_mi_prepare: null args");
  int rc = mi_image_ok("dfl_sim_mi_prepare", a->H, a->W);
  if (rc != DFL_OK) return rc;
  rc = mi_bins_ok("dfl_sim_mi_prepare", "Bf", a->Bf);
  if (rc != DFL_OK) return rc;
  DFL_REQUIRE(a->fixed != nullptr && a->fbin != nullptr && a->info != nullptr, "dfl_sim_mi_prepare: fixed, fbin and info are required");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t HW = (int64_t)a->H * a->W;
  mi_prepare_range_kernel<<<1, MI_PREP_THREADS, 0, s>>>(a->fixed, a->mask, a->info, HW);
  mi_prepare_bins_kernel<<<(unsigned)ceil_div(HW, MI_THREADS), MI_THREADS, 0, s>>>(a->fixed, a->mask, a->info, a->fbin, HW, a->Bf);
  return check_launch("dfl_sim_mi_prepare");
}

extern "C" int dfl_sim_mi(const dfl_sim_mi_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_sim_mi: null args");
  const int rc = mi_sizes_ok("dfl_sim_mi", a->V, a->H, a->W, a->F, a->Bf, a->Bm);
  if (rc != DFL_OK) return rc;
  DFL_REQUIRE(a->moving != nullptr && a->fbin != nullptr && a->info != nullptr && a->mrange != nullptr && a->hist != nullptr && a->cost != nullptr,
              "dfl_sim_mi: moving, fbin, info, mrange, hist and cost are required");
  mi_forward(a->moving, a->fbin, a->mrange, a->fixed_of, a->hist, a->cost, nullptr, a->V, (int64_t)a->H * a->W, a->F, a->Bf, a->Bm,
             static_cast<hipStream_t>(stream));
  return check_launch("dfl_sim_mi");
}

extern "C" int dfl_sim_mi_bwd(const dfl_sim_mi_bwd_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_sim_mi_bwd: null args");
  const int rc = mi_sizes_ok("dfl_sim_mi_bwd", a->V, a->H, a->W, a->F, a->Bf, a->Bm);
  if (rc != DFL_OK) return rc;
  DFL_REQUIRE(a->moving != nullptr && a->fbin != nullptr && a->info != nullptr && a->mrange != nullptr && a->hist != nullptr && a->cost != nullptr &&
                  a->ell != nullptr && a->d_moving != nullptr,
              "dfl_sim_mi_bwd: moving, fbin, info, mrange, hist, cost, ell and d_moving are required");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t HW = (int64_t)a->H * a->W;
  mi_forward(a->moving, a->fbin, a->mrange, a->fixed_of, a->hist, a->cost, a->ell, a->V, HW, a->F, a->Bf, a->Bm, s);
  mi_adjoint_kernel<<<dim3((unsigned)ceil_div(HW, MI_RUN), (unsigned)a->V), MI_THREADS, (size_t)a->Bm * a->Bf * sizeof(double), s>>>(
      a->moving, a->fbin, a->info, a->mrange, a->fixed_of, a->ell, a->d_moving, HW, a->F, a->Bf, a->Bm);
  return check_launch("dfl_sim_mi_bwd");
}
