// Random augmentation of training items on the device: the per-pixel half of the reference's RandomDataAugDataSet
// (train_test_code/dataset.py:107-283) -- invert, noise, gamma, 8-bit affine warp of the reflect-padded projection
// (nearest for the labels), erase boxes -- then standardisation, one-hot masks and heat maps of the augmented rows.
// The host (dfl_amd.dataset.DeviceAugment) draws every per-item scalar and the warp matrices; per-pixel normals come
// from Philox4x32-10 keyed by a 64-bit key per item / box and counted by the pixel index (Box-Muller in fp32).
// Contract: include/dfl_hip.h (dfl_augment_args).  HBM-bound: six launches per batch, each a pass over the augmented rows.
// Built with -ffp-contract=off: every product and sum is rounded the way the numpy restatement (tests/aug_ref.py) rounds it.
#include "common.h"
#include "philox.h"

namespace dfl {

constexpr int AUG_NB = 64;     // statistics slices per image
constexpr int AUG_BOXES = 5;

// numpy 'reflect' (no edge repeat) for any distance: period 2(n-1)
__device__ __forceinline__ int aug_reflect(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  i %= p;
  if (i < 0) i += p;
  return i >= n ? p - i : i;
}

struct AugScratch {
  float* mm_raw;     // [n][AUG_NB][2] min / max of the raw image
  float* mm_noise;   // [n][AUG_NB][2] min / max after invert + noise
  double* stats;     // [n][AUG_NB][2] sum / sum of squares of the augmented padded image
  float* img;        // [n][H][W] after invert + noise
  unsigned char* lab;  // [n][H][W] warped labels (255: outside the warped frame)
};

__host__ __device__ inline size_t aug_align(size_t v) { return (v + 255) & ~(size_t)255; }

__host__ __device__ inline AugScratch aug_scratch(void* base, int n, int H, int W) {
  AugScratch s;
  char* p = static_cast<char*>(base);
  const size_t mm = aug_align((size_t)n * AUG_NB * 2 * sizeof(float));
  s.mm_raw = reinterpret_cast<float*>(p);
  p += mm;
  s.mm_noise = reinterpret_cast<float*>(p);
  p += mm;
  s.stats = reinterpret_cast<double*>(p);
  p += aug_align((size_t)n * AUG_NB * 2 * sizeof(double));
  s.img = reinterpret_cast<float*>(p);
  p += aug_align((size_t)n * H * W * sizeof(float));
  s.lab = reinterpret_cast<unsigned char*>(p);
  return s;
}

__host__ __device__ inline size_t aug_scratch_size(int n, int H, int W) {
  return 2 * aug_align((size_t)n * AUG_NB * 2 * sizeof(float)) + aug_align((size_t)n * AUG_NB * 2 * sizeof(double)) +
         aug_align((size_t)n * H * W * sizeof(float)) + aug_align((size_t)n * H * W);
}

// block-wide min and max (256 threads); every thread gets the result
__device__ __forceinline__ void block_minmax(float& mn, float& mx, float* red) {
  red[threadIdx.x] = mn;
  red[256 + threadIdx.x] = mx;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) {
      red[threadIdx.x] = fminf(red[threadIdx.x], red[threadIdx.x + off]);
      red[256 + threadIdx.x] = fmaxf(red[256 + threadIdx.x], red[256 + threadIdx.x + off]);
    }
    __syncthreads();
  }
  mn = red[0];
  mx = red[256];
  __syncthreads();
}

__device__ __forceinline__ void combine_minmax(const float* part, float& mn, float& mx) {
  mn = INFINITY;
  mx = -INFINITY;
  for (int k = 0; k < AUG_NB; ++k) {
    mn = fminf(mn, part[2 * k]);
    mx = fmaxf(mx, part[2 * k + 1]);
  }
}

// 1. min / max of the raw image
__global__ void __launch_bounds__(256) aug_minmax_kernel(const dfl_augment_args a, AugScratch s) {
  __shared__ float red[512];
  const int k = blockIdx.y;
  const int64_t hw = (int64_t)a.H * a.W;
  if ((unsigned)a.items[k].row >= (unsigned)a.B) return;   // (block-uniform)
  const float* src = a.proj + (int64_t)a.items[k].row * hw;
  float mn = INFINITY, mx = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)AUG_NB * 256) {
    const float v = src[i];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  block_minmax(mn, mx, red);
  if (threadIdx.x == 0) {
    s.mm_raw[((int64_t)k * AUG_NB + blockIdx.x) * 2 + 0] = mn;
    s.mm_raw[((int64_t)k * AUG_NB + blockIdx.x) * 2 + 1] = mx;
  }
}

// 2. invert (p = max - p) and noise (normalise by min / max, + N(0, sigma^2), map back); min / max of the result
__global__ void __launch_bounds__(256) aug_noise_kernel(const dfl_augment_args a, AugScratch s) {
  __shared__ float red[512];
  const int k = blockIdx.y;
  const dfl_augment_item& it = a.items[k];
  if ((unsigned)it.row >= (unsigned)a.B) return;
  const int64_t hw = (int64_t)a.H * a.W;
  const float* src = a.proj + (int64_t)it.row * hw;
  float* dst = s.img + (int64_t)k * hw;
  float rmn, rmx;
  combine_minmax(s.mm_raw + (int64_t)k * AUG_NB * 2, rmn, rmx);
  const bool inv = (it.flags & DFL_AUG_INVERT) != 0, noise = (it.flags & DFL_AUG_NOISE) != 0;
  // min / max after the inversion: fl(max - p) is monotone in p
  const float mn = inv ? rmx - rmx : rmn, mx = inv ? rmx - rmn : rmx, d = mx - mn;
  float omn = INFINITY, omx = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)AUG_NB * 256) {
    float v = src[i];
    if (inv) v = rmx - v;
    if (noise) {
      const float z = aug_normal(it.noise_key, i);
      if (a.noise != nullptr) a.noise[(int64_t)k * hw + i] = z;
      float t = (v - mn) / d;
      t = t + z * it.noise_sigma;
      v = t * d + mn;
    }
    dst[i] = v;
    omn = fminf(omn, v);
    omx = fmaxf(omx, v);
  }
  block_minmax(omn, omx, red);
  if (threadIdx.x == 0) {
    s.mm_noise[((int64_t)k * AUG_NB + blockIdx.x) * 2 + 0] = omn;
    s.mm_noise[((int64_t)k * AUG_NB + blockIdx.x) * 2 + 1] = omx;
  }
}

// 3. gamma (on the fly) + 8-bit bilinear affine warp of the reflect-padded projection into the (H+2pad) x (W+2pad) crop
//    (blockIdx.z == 0), nearest warp of the labels into H x W (blockIdx.z == 1).  PIL's Image.transform(AFFINE) rules:
//    source = M (x + 0.5, y + 0.5, 1); outside [0, size) -> fill 0; bilinear taps at source - 0.5, clamped to the image,
//    the second row dropped past the last one; the double result truncated to 8 bits.  Nearest: floor of the source.
__global__ void __launch_bounds__(256) aug_warp_kernel(const dfl_augment_args a, AugScratch s) {
  const int k = blockIdx.y;
  const dfl_augment_item& it = a.items[k];
  if ((unsigned)it.row >= (unsigned)a.B) return;
  const int H = a.H, W = a.W;
  const int64_t hw = (int64_t)H * W;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int ch = (H + 1) / 2, cw = (W + 1) / 2;             // affine pad: ceil(H/2), ceil(W/2)
  if (blockIdx.z == 0) {
    const int ph = ch + a.pad, pw = cw + a.pad;             // the projection's pad includes the loader's extra pad
    const int Hp = H + 2 * ph, Wp = W + 2 * pw;
    const int Ho = H + 2 * a.pad, Wo = W + 2 * a.pad;
    float nmn, nmx;
    combine_minmax(s.mm_noise + (int64_t)k * AUG_NB * 2, nmn, nmx);
    const bool gam = (it.flags & DFL_AUG_GAMMA) != 0;
    const float nd = nmx - nmn;
    // min / max after gamma: 0^g = 0 at the minimum, 1^g = 1 at the maximum
    const float mn = nmn, mx = gam ? nd + nmn : nmx, d = mx - mn;
    const float* img = s.img + (int64_t)k * hw;
    float* dst = a.x + (int64_t)it.row * Ho * Wo;
    const double* M = it.img_map;
    for (int64_t i = t0; i < (int64_t)Ho * Wo; i += stride) {
      const int oy = (int)(i / Wo), ox = (int)(i - (int64_t)oy * Wo);
      const double X = (double)(ox + cw) + 0.5, Y = (double)(oy + ch) + 0.5;   // the crop starts at ceil(H/2), ceil(W/2)
      const double xs = M[0] * X + M[1] * Y + M[2], ys = M[3] * X + M[4] * Y + M[5];
      int level = 0;
      if (xs >= 0.0 && xs < (double)Wp && ys >= 0.0 && ys < (double)Hp) {
        const double xi = xs - 0.5, yi = ys - 0.5;
        const double fx = floor(xi), fy = floor(yi);
        const int x0 = (int)fx, y0 = (int)fy;
        const double dx = xi - fx, dy = yi - fy;
        const int xa = min(max(x0, 0), Wp - 1), xb = min(max(x0 + 1, 0), Wp - 1);
        const int ya = min(max(y0, 0), Hp - 1);
        const bool second = y0 + 1 >= 0 && y0 + 1 < Hp;
        const int yb = second ? y0 + 1 : ya;
        double q[4];
        const int tx[2] = {xa, xb}, ty[2] = {ya, yb};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = aug_reflect(ty[j >> 1] - ph, H), c = aug_reflect(tx[j & 1] - pw, W);
          float v = img[(int64_t)r * W + c];
          if (gam) {
            float t = (v - nmn) / nd;
            t = powf(t, it.gamma);
            v = t * nd + nmn;
          }
          const float t = (v - mn) / d;
          q[j] = (double)(unsigned char)(t * 255.f);          // to_pil_image: mul(255).byte(), truncation
        }
        double v1 = q[0] + (q[1] - q[0]) * dx;
        const double v2 = second ? q[2] + (q[3] - q[2]) * dx : v1;
        v1 = v1 + (v2 - v1) * dy;
        level = (int)v1;
      }
      if (a.levels != nullptr) a.levels[(int64_t)k * Ho * Wo + i] = (unsigned char)level;
      dst[i] = ((float)level / 255.f) * d + mn;               // to_tensor: / 255, then back to the old range
    }
  } else {
    if (a.labels == nullptr) return;
    const int Hs = H + 2 * ch, Ws = W + 2 * cw;
    const unsigned char* lab = a.labels + (int64_t)it.row * hw;
    unsigned char* dst = s.lab + (int64_t)k * hw;
    const double* M = it.seg_map;
    for (int64_t i = t0; i < hw; i += stride) {
      const int oy = (int)(i / W), ox = (int)(i - (int64_t)oy * W);
      const double X = (double)(ox + cw) + 0.5, Y = (double)(oy + ch) + 0.5;
      const double xs = M[0] * X + M[1] * Y + M[2], ys = M[3] * X + M[4] * Y + M[5];
      unsigned char l = 255;
      if (xs >= 0.0 && xs < (double)Ws && ys >= 0.0 && ys < (double)Hs)
        l = lab[(int64_t)aug_reflect((int)ys - ch, H) * W + aug_reflect((int)xs - cw, W)];
      dst[i] = l;
    }
  }
}

// 4. erase boxes: one workgroup per item, boxes in order; each box adds N(0, (0.2 (max - min of the box))^2)
__global__ void __launch_bounds__(256) aug_erase_kernel(const dfl_augment_args a) {
  __shared__ float red[512];
  const int k = blockIdx.x;
  const dfl_augment_item& it = a.items[k];
  if ((unsigned)it.row >= (unsigned)a.B) return;
  if (!(it.flags & DFL_AUG_ERASE)) return;
  const int Wo = a.W + 2 * a.pad;
  float* img = a.x + (int64_t)it.row * (a.H + 2 * a.pad) * Wo;
  for (int b = 0; b < it.n_box && b < AUG_BOXES; ++b) {
    const int r0 = it.box[b][0], c0 = it.box[b][1], nr = it.box[b][2], nc = it.box[b][3];
    if (r0 < 0 || c0 < 0 || nr <= 0 || nc <= 0 || r0 + nr > a.H + 2 * a.pad || c0 + nc > Wo) break;   // (uniform)
    const int n = nr * nc;
    float mn = INFINITY, mx = -INFINITY;
    for (int j = threadIdx.x; j < n; j += 256) {
      const int r = j / nc, c = j - r * nc;
      const float v = img[(int64_t)(r0 + r) * Wo + c0 + c];
      mn = fminf(mn, v);
      mx = fmaxf(mx, v);
    }
    block_minmax(mn, mx, red);
    const float sig = (mx - mn) * 0.2f;
    for (int j = threadIdx.x; j < n; j += 256) {
      const int r = j / nc, c = j - r * nc;
      const int64_t i = (int64_t)(r0 + r) * Wo + c0 + c;
      img[i] = img[i] + aug_normal(it.box_key[b], i) * sig;
    }
    __syncthreads();                                          // the next box sees this one's noise
  }
}

// 5. sum / sum of squares of the augmented (padded) image, fp64 slices
__global__ void __launch_bounds__(256) aug_stats_kernel(const dfl_augment_args a, AugScratch s) {
  __shared__ double red[2][256];
  const int k = blockIdx.y;
  const int64_t n = (int64_t)(a.H + 2 * a.pad) * (a.W + 2 * a.pad);
  if ((unsigned)a.items[k].row >= (unsigned)a.B) return;
  const float* src = a.x + (int64_t)a.items[k].row * n;
  double s1 = 0.0, s2 = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)AUG_NB * 256) {
    const double v = (double)src[i];
    s1 += v;
    s2 += v * v;
  }
  red[0][threadIdx.x] = s1;
  red[1][threadIdx.x] = s2;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) {
      red[0][threadIdx.x] += red[0][threadIdx.x + off];
      red[1][threadIdx.x] += red[1][threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    s.stats[((int64_t)k * AUG_NB + blockIdx.x) * 2 + 0] = red[0][0];
    s.stats[((int64_t)k * AUG_NB + blockIdx.x) * 2 + 1] = red[1][0];
  }
}

// 6. blockIdx.z: 0 = standardise x in place, 1 = one-hot masks of the warped labels, 2 = landmarks + heat maps
__global__ void __launch_bounds__(256) aug_write_kernel(const dfl_augment_args a, AugScratch s) {
  const int k = blockIdx.y;
  const dfl_augment_item& it = a.items[k];
  if ((unsigned)it.row >= (unsigned)a.B) return;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t hw = (int64_t)a.H * a.W;
  if (blockIdx.z == 0) {
    if (!a.standardize) return;
    const int64_t n = (int64_t)(a.H + 2 * a.pad) * (a.W + 2 * a.pad);
    double s1 = 0.0, s2 = 0.0;
    for (int j = 0; j < AUG_NB; ++j) {   // same order in every thread: bit-identical statistics
      s1 += s.stats[((int64_t)k * AUG_NB + j) * 2 + 0];
      s2 += s.stats[((int64_t)k * AUG_NB + j) * 2 + 1];
    }
    const double m = s1 / (double)n;
    double var = (s2 - s1 * m) / (double)(n - 1);   // unbiased, as torch.std
    if (var < 0.0) var = 0.0;
    const float mean = (float)m, inv = (float)(1.0 / sqrt(var));
    float* x = a.x + (int64_t)it.row * n;
    for (int64_t i = t0; i < n; i += stride) x[i] = (x[i] - mean) * inv;
  } else if (blockIdx.z == 1) {
    if (a.masks == nullptr) return;
    const unsigned char* lab = s.lab + (int64_t)k * hw;
    float* dst = a.masks + (int64_t)it.row * a.C * hw;
    for (int64_t i = t0; i < hw; i += stride) {
      const int l = lab[i];                                   // 255 (outside the warped frame): every channel 0
      for (int c = 0; c < a.C; ++c) dst[(int64_t)c * hw + i] = (l == c) ? 1.f : 0.f;
    }
  } else {
    if (a.lands == nullptr) return;
    const float* lin = a.lands + (int64_t)it.row * 2 * a.L;
    float* lout = a.lands_out + (int64_t)it.row * 2 * a.L;
    float* heat = a.heats != nullptr ? a.heats + (int64_t)it.row * a.L * hw : nullptr;
    const double* M = it.land_map;
    const float s2 = a.sigma * a.sigma;
    const float kexp = 1.f / (s2 * -2.f), knorm = 1.f / (2.f * 3.14159265358979323846f * s2);
    for (int l = 0; l < a.L; ++l) {
      const float lx = lin[l], ly = lin[a.L + l];
      float mx = lx, my = ly;                                   // dataset.py:242: an inf coordinate leaves the pair as it is
      if (!isinf(lx) && !isinf(ly)) {
        const double X = M[0] * (double)lx + M[1] * (double)ly + M[2], Y = M[3] * (double)lx + M[4] * (double)ly + M[5];
        bool drop = false;
        if (a.land_rule == DFL_AUG_LANDS_REFERENCE)            // dataset.py:245-247 as written: x against H-1, y < C-1
          drop = X < 0.0 || X > (double)(a.H - 1) || Y < 0.0 || Y < (double)(a.C - 1);
        else if (a.land_rule == DFL_AUG_LANDS_IN_VIEW)
          drop = X < 0.0 || X > (double)(a.W - 1) || Y < 0.0 || Y > (double)(a.H - 1);
        mx = drop ? INFINITY : (float)X;
        my = drop ? INFINITY : (float)Y;
      }
      if (t0 == 0) {
        lout[l] = mx;
        lout[a.L + l] = my;
      }
      if (heat == nullptr) continue;
      const bool ok = !isinf(mx) && !isinf(my) && !isnan(mx) && !isnan(my);   // dataset.py:313: every finite landmark
      for (int64_t i = t0; i < hw; i += stride) {
        const int y = (int)(i / a.W), x = (int)(i - (int64_t)y * a.W);
        const float dx = (float)x - mx, dy = (float)y - my;
        heat[(int64_t)l * hw + i] = ok ? expf((dx * dx + dy * dy) * kexp) * knorm : 0.f;
      }
    }
  }
}

}  // namespace dfl

extern "C" int64_t dfl_augment_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t pad) {
  (void)pad;
  if (B <= 0 || H <= 0 || W <= 0) return -1;
  return (int64_t)dfl::aug_scratch_size(B, H, W);
}

extern "C" int dfl_augment_batch(const dfl_augment_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_augment_batch: null args");
  DFL_REQUIRE(a->n_items >= 0 && a->n_items <= a->B && a->n_items < 65536, "dfl_augment_batch: bad n_items");
  if (a->n_items == 0) return DFL_OK;
  DFL_REQUIRE(a->B > 0 && a->H > 1 && a->W > 1 && a->pad >= 0, "dfl_augment_batch: bad sizes");
  DFL_REQUIRE(a->proj != nullptr && a->x != nullptr && a->items != nullptr && a->scratch != nullptr,
              "dfl_augment_batch: proj, x, items and scratch are required");
  DFL_REQUIRE((reinterpret_cast<uintptr_t>(a->scratch) & 255) == 0, "dfl_augment_batch: scratch must be 256-byte aligned");
  DFL_REQUIRE(a->masks == nullptr || (a->labels != nullptr && a->C > 0 && a->C < 255), "dfl_augment_batch: masks need labels and C < 255");
  DFL_REQUIRE(a->lands == nullptr || (a->lands_out != nullptr && a->L > 0), "dfl_augment_batch: lands need lands_out and L");
  DFL_REQUIRE(a->heats == nullptr || (a->lands != nullptr && a->sigma > 0.f), "dfl_augment_batch: heats need lands and sigma");
  DFL_REQUIRE(a->land_rule >= DFL_AUG_LANDS_NONE && a->land_rule <= DFL_AUG_LANDS_IN_VIEW, "dfl_augment_batch: bad land_rule");
  DFL_REQUIRE(a->land_rule != DFL_AUG_LANDS_REFERENCE || a->C > 0, "dfl_augment_batch: the reference landmark rule needs C");
  DFL_REQUIRE((int64_t)(a->H + 2 * a->pad) * (a->W + 2 * a->pad) < (1ll << 31), "dfl_augment_batch: image too large");
  DFL_REQUIRE(a->lands_out == nullptr || a->lands_out != a->lands, "dfl_augment_batch: lands_out must not alias lands");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dfl::AugScratch sc = dfl::aug_scratch(a->scratch, a->n_items, a->H, a->W);
  const unsigned n = (unsigned)a->n_items;
  hipLaunchKernelGGL(dfl::aug_minmax_kernel, dim3(dfl::AUG_NB, n), dim3(256), 0, s, *a, sc);
  hipLaunchKernelGGL(dfl::aug_noise_kernel, dim3(dfl::AUG_NB, n), dim3(256), 0, s, *a, sc);
  const int64_t no = (int64_t)(a->H + 2 * a->pad) * (a->W + 2 * a->pad);
  int64_t gx = dfl::ceil_div(no, 256 * 2);
  if (gx > 512) gx = 512;
  hipLaunchKernelGGL(dfl::aug_warp_kernel, dim3((unsigned)gx, n, 2), dim3(256), 0, s, *a, sc);
  hipLaunchKernelGGL(dfl::aug_erase_kernel, dim3(n), dim3(256), 0, s, *a);
  hipLaunchKernelGGL(dfl::aug_stats_kernel, dim3(dfl::AUG_NB, n), dim3(256), 0, s, *a, sc);
  gx = dfl::ceil_div(no, 256 * 4);
  if (gx > 1024) gx = 1024;
  hipLaunchKernelGGL(dfl::aug_write_kernel, dim3((unsigned)gx, n, 3), dim3(256), 0, s, *a, sc);
  return dfl::check_launch("dfl_augment_batch");
}
