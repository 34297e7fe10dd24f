// Output heads of the U-Net (reference: train_test_code/unet.py:176-191):
//   logits = seg_conv(x)                  1x1, no bias, F -> NC
//   seg    = Softmax2d(logits)            (or logits when do_soft_max=False)
//   heat   = lands_1x1(cat(x, logits))    1x1 (F+NC -> NM) [-> 1x1 (NM -> L)], no bias, no non-linearity
// One thread per pixel (the kernels of this file), 256 consecutive pixels per workgroup.  A thread-private walk over its 128-byte
// feature row would touch 64 cache lines per wave-instruction (measured: 5x the compulsory HBM reads), so the [256][F] tile is loaded
// cooperatively (consecutive lanes = consecutive 16 bytes) into LDS (pitch F + 4: conflict-free b128 row reads) and the
// same tile carries dx back out in the backward kernel; the head weights (5 KB) are read with
// wave-uniform addresses through `const __restrict__` kernel parameters, i.e. as scalar loads into SGPR operands of the
// FMAs (no LDS traffic: the LDS-broadcast version spent 224 ds_read_b128 per pixel), logits / mid / heat stay in registers, seg and heat are stored NCHW (lane = pixel
// => unit-stride stores per channel plane).  HBM-bound: 4*F bytes in, 4*(NC+L) bytes out per pixel.
// The backward kernel recomputes logits and mid from x (cheaper than saving them), applies the softmax Jacobian
//  and leaves dx plus a per-pixel scratch row from which the three small weight gradients are
// taken by dfl_conv2d_wgrad.  With bf16 features (F = 32) the weight gradients are taken inside the kernel instead (the
// scratch is 448 bytes per pixel to write and read back): head_wgrad.h.  Such features and a head inside the small
// capacities go to the matrix-core kernels (head_mfma.h), a different algorithm for the same arithmetic.
#include "common.h"
#include "head_mfma.h"
#include "head_wgrad.h"

namespace dfl {

constexpr int HT = 256;   // pixels per workgroup tile

// A capacity sizes the per-thread arrays of the kernels, so the common shapes keep the small register footprint and heads
// with more than 8 classes / 16 landmarks / 24 mid channels (train.py --num-classes is free) run the same code with larger
// arrays.  SMALL: the capacity that also has the specialised shapes, the fused weight gradients and the matrix-core kernels.
template <int NC_, int NM_, int L_, bool SMALL_>
struct HeadCaps {
  static constexpr int NC = NC_, NM = NM_, L = L_;
  static constexpr bool SMALL = SMALL_;
};
using HeadSmall = HeadCaps<DFL_HEAD_MAX_NC, DFL_HEAD_MAX_NM, DFL_HEAD_MAX_L, true>;
using HeadLarge = HeadCaps<DFL_HEAD_LARGE_NC, DFL_HEAD_LARGE_NM, DFL_HEAD_LARGE_L, false>;

// The channel counts are template parameters for the reference's two head shapes (7 classes alone, 7 + 14 landmarks
// through 21): with run-time bounds every 4-FMA group became its own basic block (scalar load, wait, branch -- ~950
// branches per pixel, the kernels ran at 1 TB/s).  HeadShape<C> (GEN) keeps the run-time bounds for any other shape.
template <class C, int NCc = 0, int NMc = 0, int Lc = 0>
struct HeadShape {
  using Caps = C;
  static constexpr bool GEN = NCc == 0;
  static constexpr int NC = NCc, NM = NMc, L = Lc;                                                // the fixed counts (!GEN)
  static constexpr int MAXNC = C::NC, MAXNM = C::NM, MAXL = C::L;                                 // array sizes
  static constexpr int BNC = GEN ? MAXNC : NCc, BNM = GEN ? MAXNM : NMc, BL = GEN ? MAXL : Lc;    // loop bounds
};

// columns of the scratch row that hold cat(x, logits): a multiple of 4
template <class C>
inline int head_fc(int F) { return ((F + C::NC) + 3) / 4 * 4; }

// tile[p][0..F) = x[m0 + p][0..F) (zeros past M); optionally the same values go to cat[(m0 + p) * cat_ld + ..] (scratch)
__device__ __forceinline__ void head_load_tile(float* tile, int pitch, const float* __restrict__ x, int ldx, int64_t m0,
                                               int64_t M, int F, float* __restrict__ cat, int cat_ld, int x_bf16) {
  if (x_bf16) {   // bf16 features (math mode 4): 8 channels per 16-byte load, widened to fp32 in the tile
    const int f8 = F / 8;
    const unsigned short* xb = reinterpret_cast<const unsigned short*>(x);
    for (int e = threadIdx.x; e < HT * f8; e += HT) {
      const int p = e / f8, q = e - p * f8;
      float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (m0 + p < M) {
        unpack8(*reinterpret_cast<const u32x4*>(xb + (m0 + p) * ldx + 8 * q), v);
        if (cat != nullptr) {
          *reinterpret_cast<float4*>(cat + (m0 + p) * cat_ld + 8 * q) = make_float4(v[0], v[1], v[2], v[3]);
          *reinterpret_cast<float4*>(cat + (m0 + p) * cat_ld + 8 * q + 4) = make_float4(v[4], v[5], v[6], v[7]);
        }
      }
      *reinterpret_cast<float4*>(tile + p * pitch + 8 * q) = make_float4(v[0], v[1], v[2], v[3]);
      *reinterpret_cast<float4*>(tile + p * pitch + 8 * q + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
    return;
  }
  const int fq = F / 4;
  for (int e = threadIdx.x; e < HT * fq; e += HT) {
    const int p = e / fq, q = e - p * fq;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (m0 + p < M) {
      v = *reinterpret_cast<const float4*>(x + (m0 + p) * ldx + 4 * q);
      if (cat != nullptr) *reinterpret_cast<float4*>(cat + (m0 + p) * cat_ld + 4 * q) = v;
    }
    *reinterpret_cast<float4*>(tile + p * pitch + 4 * q) = v;
  }
}

// logits (lg) and mid for pixel row xr (in LDS).  K1 = F + NC = row length of w_l1.
template <class S>
__device__ __forceinline__ void head_features(const float* xr, const float* __restrict__ w_seg, const float* __restrict__ w_l1,
                                              int F, int NC, int NM, bool lands, float* lg, float* mid) {
  const int K1 = F + NC;
#pragma unroll
  for (int c = 0; c < S::MAXNC; ++c) lg[c] = 0.f;
#pragma unroll
  for (int j = 0; j < S::MAXNM; ++j) mid[j] = 0.f;
  for (int k = 0; k < F; k += 4) {
    const float4 xv = *reinterpret_cast<const float4*>(xr + k);
#pragma unroll
    for (int c = 0; c < S::BNC; ++c) {
      if (!S::GEN || c < NC) {
        const float* w = w_seg + c * F + k;
        lg[c] = fmaf(w[0], xv.x, fmaf(w[1], xv.y, fmaf(w[2], xv.z, fmaf(w[3], xv.w, lg[c]))));
      }
    }
    if (lands) {
#pragma unroll
      for (int j = 0; j < S::BNM; ++j) {
        if (!S::GEN || j < NM) {
          const float* w = w_l1 + j * K1 + k;
          mid[j] = fmaf(w[0], xv.x, fmaf(w[1], xv.y, fmaf(w[2], xv.z, fmaf(w[3], xv.w, mid[j]))));
        }
      }
    }
  }
  if (lands) {
#pragma unroll
    for (int j = 0; j < S::BNM; ++j) {
      if (!S::GEN || j < NM) {
#pragma unroll
        for (int c = 0; c < S::BNC; ++c)
          if (!S::GEN || c < NC) mid[j] = fmaf(w_l1[j * K1 + F + c], lg[c], mid[j]);
      }
    }
  }
}

template <class S>
__device__ __forceinline__ void softmax_inplace(float* lg, int NC) {
  float mx = lg[0];
#pragma unroll
  for (int c = 1; c < S::BNC; ++c)
    if (!S::GEN || c < NC) mx = fmaxf(mx, lg[c]);
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < S::BNC; ++c) {
    if (!S::GEN || c < NC) {
      lg[c] = expf(lg[c] - mx);
      sum += lg[c];
    }
  }
  const float inv = 1.0f / sum;
#pragma unroll
  for (int c = 0; c < S::BNC; ++c)
    if (!S::GEN || c < NC) lg[c] *= inv;
}

template <class S>
__global__ void __launch_bounds__(256) head_fwd_kernel(const dfl_head_fwd_args a, const float* __restrict__ w_seg,
                                                      const float* __restrict__ w_l1, const float* __restrict__ w_l2) {
  extern __shared__ __attribute__((aligned(16))) float tile[];
  const int F = a.F, NC = S::GEN ? a.NC : S::NC, NM = S::GEN ? a.NM : S::NM, L = S::GEN ? a.L : S::L;
  const int pitch = F + 4;
  const int64_t HW = (int64_t)a.H * a.W;
  const int64_t M = (int64_t)a.N * HW;
  const bool lands = L > 0;
  for (int64_t m0 = (int64_t)blockIdx.x * HT; m0 < M; m0 += (int64_t)gridDim.x * HT) {
    __syncthreads();
    head_load_tile(tile, pitch, a.x, a.ldx, m0, M, F, nullptr, 0, a.x_bf16);
    __syncthreads();
    const int64_t m = m0 + threadIdx.x;
    if (m >= M) continue;
    float lg[S::MAXNC], mid[S::MAXNM];
    head_features<S>(tile + threadIdx.x * pitch, w_seg, w_l1, F, NC, NM, lands, lg, mid);
    const int64_t n = m / HW, pp = m - n * HW;
    if (lands) {
      float* hp = a.heat + n * L * HW + pp;
      if (w_l2 != nullptr) {
#pragma unroll
        for (int l = 0; l < S::BL; ++l) {
          if (!S::GEN || l < L) {
            float acc = 0.f;
#pragma unroll
            for (int j = 0; j < S::BNM; ++j)
              if (!S::GEN || j < NM) acc = fmaf(w_l2[l * NM + j], mid[j], acc);
            hp[(int64_t)l * HW] = acc;
          }
        }
      } else {
#pragma unroll
        for (int l = 0; l < S::BL; ++l)
          if (!S::GEN || l < L) hp[(int64_t)l * HW] = mid[l];
      }
    }
    if (a.softmax) softmax_inplace<S>(lg, NC);
    float* sp = a.seg + n * NC * HW + pp;
#pragma unroll
    for (int c = 0; c < S::BNC; ++c)
      if (!S::GEN || c < NC) sp[(int64_t)c * HW] = lg[c];
  }
}

// Fc = head_fc(F).  FUSED (bf16 features, F = 32, small capacity): the weight gradients are taken here (head_wgrad.h) from a
// row image behind the feature tile, 128 pixels at a time; otherwise a scratch row per pixel is left for dfl_conv2d_wgrad.
template <class S, bool FUSED>
__global__ void __launch_bounds__(256) head_bwd_kernel(const dfl_head_bwd_args a, int Fc, const float* __restrict__ w_seg,
                                                      const float* __restrict__ w_l1, const float* __restrict__ w_l2) {
  extern __shared__ __attribute__((aligned(16))) float tile[];
  constexpr int MAXNC = S::MAXNC, MAXNM = S::MAXNM, MAXL = S::MAXL;
  static_assert(!FUSED || (MAXNC == 8 && MAXNM == 24 && MAXL == 16), "the row image is laid out for the small capacities");
  const int F = a.F, NC = S::GEN ? a.NC : S::NC, NM = S::GEN ? a.NM : S::NM, L = S::GEN ? a.L : S::L;
  const int K1 = F + NC;
  const int pitch = F + 4;
  const int64_t HW = (int64_t)a.H * a.W;
  const int64_t M = (int64_t)a.N * HW;
  const bool lands = L > 0 && a.dheat != nullptr;
  const int o_dlg = Fc, o_dmid = Fc + MAXNC, o_mid = o_dmid + MAXNM, o_dh = o_mid + MAXNM;   // all multiples of 4
  unsigned char* ab = reinterpret_cast<unsigned char*>(tile) + (size_t)HT * pitch * sizeof(float);
  const HeadWgLane wg;
  f32x16 wacc;
#pragma unroll
  for (int r = 0; r < 16; ++r) wacc[r] = 0.f;
  for (int64_t m0 = (int64_t)blockIdx.x * HT; m0 < M; m0 += (int64_t)gridDim.x * HT) {
    __syncthreads();
    head_load_tile(tile, pitch, a.x, a.ldx, m0, M, F, FUSED ? nullptr : a.scratch, a.scratch_ld, a.x_bf16);   // also copies x into the cat columns
    __syncthreads();
    const int64_t m = m0 + threadIdx.x;
    u32x4 rowV[4] = {}, rowD[2] = {}, rowB[8] = {};   // this pixel's bf16 row (fused form): V, dheat and [x | U], 16 bytes each
    if (m < M) {
      float* myrow = tile + threadIdx.x * pitch;
      float* sr = FUSED ? nullptr : a.scratch + m * a.scratch_ld;
      float lg[MAXNC], mid[MAXNM];
      head_features<S>(myrow, w_seg, w_l1, F, NC, NM, L > 0, lg, mid);
      const int64_t n = m / HW, pp = m - n * HW;
      if constexpr (FUSED) {                // x (exact: it was bf16), logits, mid (zeros without landmarks)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 v0 = *reinterpret_cast<const float4*>(myrow + 8 * q), v1 = *reinterpret_cast<const float4*>(myrow + 8 * q + 4);
          const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
          rowB[q] = pack8(v);
        }
        rowB[4] = pack8(lg);
#pragma unroll
        for (int q = 0; q < 3; ++q) rowB[5 + q] = pack8(mid + 8 * q);
      } else {
        // cat tail: logits then zero pad (16-byte stores: the scratch row is 16-byte aligned, every block a multiple of 4)
#pragma unroll
        for (int c = 0; c < MAXNC; c += 4)
          *reinterpret_cast<float4*>(sr + F + c) = make_float4(c + 0 < NC ? lg[c + 0] : 0.f, c + 1 < NC ? lg[c + 1] : 0.f,
                                                               c + 2 < NC ? lg[c + 2] : 0.f, c + 3 < NC ? lg[c + 3] : 0.f);
        for (int c = F + MAXNC; c < Fc; c += 4) *reinterpret_cast<float4*>(sr + c) = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      // landmark branch
      float dmid[MAXNM], dh[MAXL];
#pragma unroll
      for (int l = 0; l < MAXL; ++l) dh[l] = (lands && l < L) ? a.dheat[(n * L + l) * HW + pp] : 0.f;
#pragma unroll
      for (int j = 0; j < MAXNM; ++j) {
        float acc = 0.f;
        if (lands && j < NM) {
          if (w_l2 != nullptr) {
#pragma unroll
            for (int l = 0; l < S::BL; ++l)
              if (!S::GEN || l < L) acc = fmaf(w_l2[l * NM + j], dh[l], acc);
          } else {
            acc = (j < MAXL) ? dh[j < MAXL ? j : 0] : 0.f;
          }
        }
        dmid[j] = acc;
      }
      // logits gradient: through cat (landmark branch) + through softmax (seg branch)
      float dlg[MAXNC];
      float dot = 0.f;
#pragma unroll
      for (int c = 0; c < MAXNC; ++c) {
        float g = 0.f, sv = 0.f;
        if (c < NC) {
          g = a.dseg[(n * NC + c) * HW + pp];
          sv = a.seg[(n * NC + c) * HW + pp];
        }
        dlg[c] = g;      // provisional: upstream gradient
        lg[c] = sv;      // reuse lg for the softmax output
        dot = fmaf(g, sv, dot);
      }
#pragma unroll
      for (int c = 0; c < MAXNC; ++c) {
        float v = 0.f;
        if (c < NC) {
          v = a.softmax ? lg[c] * (dlg[c] - dot) : dlg[c];
          if (lands) {
#pragma unroll
            for (int j = 0; j < S::BNM; ++j)
              if (!S::GEN || j < NM) v = fmaf(w_l1[j * K1 + F + c], dmid[j], v);
          }
        }
        dlg[c] = v;
      }
      if constexpr (FUSED) {
        rowV[0] = pack8(dlg);
#pragma unroll
        for (int q = 0; q < 3; ++q) rowV[1 + q] = pack8(dmid + 8 * q);
#pragma unroll
        for (int q = 0; q < 2; ++q) rowD[q] = pack8(dh + 8 * q);
      } else {
#pragma unroll
        for (int c = 0; c < MAXNC; c += 4)
          *reinterpret_cast<float4*>(sr + o_dlg + c) = make_float4(dlg[c], dlg[c + 1], dlg[c + 2], dlg[c + 3]);
#pragma unroll
        for (int j = 0; j < MAXNM; j += 4) {
          *reinterpret_cast<float4*>(sr + o_dmid + j) = make_float4(dmid[j], dmid[j + 1], dmid[j + 2], dmid[j + 3]);
          const bool has = L > 0;
          *reinterpret_cast<float4*>(sr + o_mid + j) = make_float4((has && j + 0 < NM) ? mid[j + 0] : 0.f, (has && j + 1 < NM) ? mid[j + 1] : 0.f,
                                                                  (has && j + 2 < NM) ? mid[j + 2] : 0.f, (has && j + 3 < NM) ? mid[j + 3] : 0.f);
        }
#pragma unroll
        for (int l = 0; l < MAXL; l += 4) *reinterpret_cast<float4*>(sr + o_dh + l) = make_float4(dh[l], dh[l + 1], dh[l + 2], dh[l + 3]);
      }
      // dx = Wseg^T dlogits + W1[:, :F]^T dmid, into this thread's own tile row (x is no longer needed)
      for (int k = 0; k < F; k += 4) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int c = 0; c < S::BNC; ++c) {
          if (!S::GEN || c < NC) {
            const float* w = w_seg + c * F + k;
            acc.x = fmaf(w[0], dlg[c], acc.x); acc.y = fmaf(w[1], dlg[c], acc.y);
            acc.z = fmaf(w[2], dlg[c], acc.z); acc.w = fmaf(w[3], dlg[c], acc.w);
          }
        }
        if (lands) {
#pragma unroll
          for (int j = 0; j < S::BNM; ++j) {
            if (!S::GEN || j < NM) {
              const float* w = w_l1 + j * K1 + k;
              acc.x = fmaf(w[0], dmid[j], acc.x); acc.y = fmaf(w[1], dmid[j], acc.y);
              acc.z = fmaf(w[2], dmid[j], acc.z); acc.w = fmaf(w[3], dmid[j], acc.w);
            }
          }
        }
        *reinterpret_cast<float4*>(myrow + k) = acc;
      }
    }
    if constexpr (FUSED) {  // weight gradients of this tile: two halves of 128 pixels through the row image
      for (int half = 0; half < 2; ++half) {
        if (half) __syncthreads();          // the waves are done reading the first half
        if ((threadIdx.x >> 7) == half) {
          unsigned char* dst = ab + (size_t)(threadIdx.x & (HEAD_WG_ROWS - 1)) * HEAD_WG_PITCH;
#pragma unroll
          for (int q = 0; q < 4; ++q) *reinterpret_cast<u32x4*>(dst + HEAD_WG_V + 16 * q) = rowV[q];
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            *reinterpret_cast<u32x4*>(dst + HEAD_WG_DHEAT + 16 * q) = rowD[q];
            *reinterpret_cast<u32x4*>(dst + HEAD_WG_ZERO + 16 * q) = (u32x4)(0u);
          }
#pragma unroll
          for (int q = 0; q < 8; ++q) *reinterpret_cast<u32x4*>(dst + HEAD_WG_X + 16 * q) = rowB[q];
        }
        __syncthreads();
        wg.product(ab, wacc);
      }
    }
    __syncthreads();
    if (a.x_bf16) {         // dx as bf16: 8 channels per 16-byte store
      const int f8 = F / 8;
      unsigned short* dxb = reinterpret_cast<unsigned short*>(a.dx);
      for (int e = threadIdx.x; e < HT * f8; e += HT) {
        const int p = e / f8, q = e - p * f8;
        if (m0 + p < M) *reinterpret_cast<u32x4*>(dxb + (m0 + p) * a.lddx + 8 * q) = pack8(tile + p * pitch + 8 * q);
      }
      continue;
    }
    const int fq = F / 4;   // cooperative, coalesced store of the dx tile
    for (int e = threadIdx.x; e < HT * fq; e += HT) {
      const int p = e / fq, q = e - p * fq;
      if (m0 + p < M) *reinterpret_cast<float4*>(a.dx + (m0 + p) * a.lddx + 4 * q) = *reinterpret_cast<const float4*>(tile + p * pitch + 4 * q);
    }
  }
  if constexpr (FUSED) wg.store(a.wg_partial, wacc);
}

// Sums the workgroup partials of the fused head weight gradients (fixed order, fp64) and files the three blocks of the
// 64 x 64 product: rows 0-7 x columns 0-31 -> dw_seg, rows 8-31 x columns 0-39 -> dw_l1, rows 32-47 x columns 40-63 -> dw_l2.
__global__ void __launch_bounds__(256) head_wgrad_finish_kernel(const float* __restrict__ partial, int nblocks, float* __restrict__ dw_seg,
                                                                float* __restrict__ dw_l1, float* __restrict__ dw_l2, int F, int NC, int NM, int L) {
  // 16 elements of the 64 x 64 product per workgroup x 16 lanes over the workgroup partials (eight loads in flight per
  // lane), lanes added up through LDS in a fixed order
  __shared__ double red[16][17];
  const int el = threadIdx.x & 15, ln = threadIdx.x >> 4;
  const int e = blockIdx.x * 16 + el;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int b = ln;
  for (; b + 7 * 16 < nblocks; b += 8 * 16) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = partial[(int64_t)(b + u * 16) * HEAD_WG_PART + e];
    s0 += (double)v[0] + (double)v[4];
    s1 += (double)v[1] + (double)v[5];
    s2 += (double)v[2] + (double)v[6];
    s3 += (double)v[3] + (double)v[7];
  }
  for (; b < nblocks; b += 16) s0 += (double)partial[(int64_t)b * HEAD_WG_PART + e];
  red[ln][el] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (ln != 0) return;
  double tot = 0.0;
#pragma unroll
  for (int k = 0; k < 16; ++k) tot += red[k][el];
  const int row = e >> 6, col = e & 63;
  float* dst = nullptr;
  if (row < 8) {
    if (row < NC && col < F) dst = dw_seg + row * F + col;
  } else if (row < 32) {
    if (dw_l1 != nullptr && row - 8 < NM && col < F + NC) dst = dw_l1 + (row - 8) * (F + NC) + col;
  } else if (row < 48) {
    if (dw_l2 != nullptr && row - 32 < L && col >= 40 && col - 40 < NM) dst = dw_l2 + (row - 32) * NM + (col - 40);
  }
  if (dst != nullptr) *dst = (float)tot;
}

static unsigned head_grid(int64_t M) {
  int64_t b = ceil_div(M, 256);
  if (b > 4096) b = 4096;
  return (unsigned)(b < 1 ? 1 : b);
}

static unsigned head_wgrad_grid(int64_t M) {
  int64_t b = ceil_div(M, HT);
  if (b > 512) b = 512;                     // two workgroups per CU walk the tiles; one partial each
  return (unsigned)(b < 1 ? 1 : b);
}

// The checks, the scratch layout and the launchers, once per capacity C

// bf16 features with F = 32 and a head inside the small capacities (two 1x1 landmark layers, or none): matrix-core kernels
template <class C>
static bool head_mfma_ok(int x_bf16, int F, int ldx, int L, const void* w_l2, const void* w_seg) {
  return C::SMALL && x_bf16 && F == 32 && ldx % 8 == 0 && (L == 0 || w_l2 != nullptr) && aligned16(w_seg);
}

template <class C>
static int head_check(int F, int NC, int NM, int L, const void* w_l1, const void* w_l2, int ldx, const void* x, int x_bf16 = 0) {
  DFL_REQUIRE(F >= 4 && F % 4 == 0, "dfl_head: F must be a multiple of 4 (got %d)", F);
  DFL_REQUIRE(!x_bf16 || (F % 8 == 0 && ldx % 8 == 0), "dfl_head (bf16): F and ldx must be multiples of 8");
  DFL_REQUIRE(NC >= 1 && NC <= C::NC, "dfl_head: n_classes %d exceeds the supported maximum %d", NC, C::NC);
  DFL_REQUIRE(L >= 0 && L <= C::L, "dfl_head: num_lands %d exceeds the supported maximum %d", L, C::L);
  DFL_REQUIRE(ldx % 4 == 0 && aligned16(x), "dfl_head: x must be 16-byte aligned with ld %% 4 == 0");
  if (L > 0) {
    DFL_REQUIRE(w_l1 != nullptr, "dfl_head: w_l1 required when L > 0");
    DFL_REQUIRE(NM >= 1 && NM <= C::NM, "dfl_head: mid width %d exceeds the supported maximum %d", NM, C::NM);
    DFL_REQUIRE(w_l2 != nullptr || NM == L, "dfl_head: single 1x1 needs NM == L");
  }
  return DFL_OK;
}

// scratch row of the backward kernel: [cat(x, logits), padded | dlogits | dmid | mid | dheat]
template <class C>
static inline int scratch_off(int F, int which) {
  const int fc = head_fc<C>(F), off[5] = {0, fc, fc + C::NC, fc + C::NC + C::NM, fc + C::NC + 2 * C::NM};
  return which >= 0 && which < 5 ? off[which] : -1;
}
template <class C>
static inline int scratch_ld(int F) { return scratch_off<C>(F, 4) + C::L; }

// calls f(shape): one of the reference's two shapes (small capacity only), or the generic bounds
template <class C, class Fn>
static void head_with_shape(int NC, int NM, int L, const void* w_l2, Fn f) {
  if constexpr (C::SMALL) {
    if (NC == 7 && L == 14 && NM == 21 && w_l2 != nullptr) return f(HeadShape<C, 7, 21, 14>());
    if (NC == 7 && L == 0) return f(HeadShape<C, 7, 0, 0>());
  }
  f(HeadShape<C>());
}

template <class C>
static int launch_fwd(const dfl_head_fwd_args* a, dfl_stream_t stream) {
  int rc = head_check<C>(a->F, a->NC, a->NM, a->L, a->w_l1, a->w_l2, a->ldx, a->x, a->x_bf16);
  if (rc != DFL_OK) return rc;
  const int64_t M = (int64_t)a->N * a->H * a->W;
  hipStream_t hs = static_cast<hipStream_t>(stream);
  if (head_mfma_ok<C>(a->x_bf16, a->F, a->ldx, a->L, a->w_l2, a->w_seg)) {      // bf16 features, F = 32: the products run on the matrix cores
    constexpr int cap = 512;         // (2048 / 1024 / 512 / 256 workgroups: 54 / 40 / 36 / 47 us -- every wave builds the weight fragments first)
    int64_t grid = ceil_div(M, HM_TILE);
    if (grid > cap) grid = cap;
    if (a->L > 0)
      hipLaunchKernelGGL(head_mfma_fwd_kernel<true>, dim3((unsigned)grid), dim3(256), 0, hs, *a);
    else
      hipLaunchKernelGGL(head_mfma_fwd_kernel<false>, dim3((unsigned)grid), dim3(256), 0, hs, *a);
    return check_launch("dfl_head_fwd");
  }
  head_with_shape<C>(a->NC, a->NM, a->L, a->w_l2, [&](auto shape) {
    hipLaunchKernelGGL(head_fwd_kernel<decltype(shape)>, dim3(head_grid(M)), dim3(HT), (size_t)HT * (a->F + 4) * sizeof(float), hs, *a,
                       a->w_seg, a->w_l1, a->w_l2);
  });
  return check_launch("dfl_head_fwd");
}

// the thread-per-pixel backward kernel; the fused form's feature tile and row image need more LDS than a kernel has unasked
template <class S, bool FUSED>
static int launch_bwd_pixel(const dfl_head_bwd_args* a, unsigned grid, size_t lds, hipStream_t hs) {
  const auto k = head_bwd_kernel<S, FUSED>;
  if constexpr (FUSED) DFL_LDS_OPT_IN(k, lds, "dfl_head_bwd")
  hipLaunchKernelGGL(k, dim3(grid), dim3(HT), lds, hs, *a, head_fc<typename S::Caps>(a->F), a->w_seg, a->w_l1, a->w_l2);
  return check_launch("dfl_head_bwd");
}

template <class C>
static int launch_bwd(const dfl_head_bwd_args* a, dfl_stream_t stream) {
  int rc = head_check<C>(a->F, a->NC, a->NM, a->L, a->w_l1, a->w_l2, a->ldx, a->x, a->x_bf16);
  if (rc != DFL_OK) return rc;
  const bool fused = a->dw_seg != nullptr;
  const int64_t M = (int64_t)a->N * a->H * a->W;
  size_t lds = (size_t)HT * (a->F + 4) * sizeof(float);
  unsigned grid = head_grid(M);
  if (fused) {
    DFL_REQUIRE(C::SMALL, "dfl_head_bwd: the fused weight gradients serve heads of up to 8 classes, 16 landmarks and 24 mid channels");
    DFL_REQUIRE(a->x_bf16 && a->F == 32, "dfl_head_bwd: the fused weight gradients need bf16 features with F == 32 (F = %d)", a->F);
    DFL_REQUIRE(a->wg_partial != nullptr && aligned16(a->wg_partial), "dfl_head_bwd: wg_partial (dfl_head_wgrad_blocks(M) * 4096 floats) is required");
    DFL_REQUIRE((a->L == 0 || a->dw_l1 != nullptr) && ((a->L > 0 && a->w_l2 != nullptr) == (a->dw_l2 != nullptr)),
                "dfl_head_bwd: dw_l1 / dw_l2 must be given exactly for the landmark layers the head has");
    lds += HEAD_WG_LDS;
    grid = head_wgrad_grid(M);
  } else {
    DFL_REQUIRE(a->scratch_ld >= scratch_ld<C>(a->F) && a->scratch_ld % 4 == 0 && aligned16(a->scratch),
                "dfl_head_bwd: scratch_ld too small or misaligned");
  }
  hipStream_t hs = static_cast<hipStream_t>(stream);
  if (fused && head_mfma_ok<C>(a->x_bf16, a->F, a->ldx, a->L, a->w_l2, a->w_seg)) {
    DFL_REQUIRE(a->stat_totals == nullptr || (a->stat_other != nullptr && a->ldso % 8 == 0 && aligned16(a->stat_other)),
                "dfl_head_bwd: stat_totals needs stat_other (bf16, 16-byte aligned, ldso %% 8 == 0)");
    if (a->L > 0)
      hipLaunchKernelGGL(head_mfma_bwd_kernel<true>, dim3(grid), dim3(256), HEAD_WG_LDS, hs, *a);
    else
      hipLaunchKernelGGL(head_mfma_bwd_kernel<false>, dim3(grid), dim3(256), HEAD_WG_LDS, hs, *a);
    rc = check_launch("dfl_head_bwd");
  } else {
    DFL_REQUIRE(a->stat_totals == nullptr, "dfl_head_bwd: live statistics (stat_totals) are taken by the matrix-core kernels only");
    if (!fused)
      head_with_shape<C>(a->NC, a->NM, a->L, a->w_l2, [&](auto shape) { rc = launch_bwd_pixel<decltype(shape), false>(a, grid, lds, hs); });
    else if constexpr (C::SMALL)      // a single landmark 1x1, or a w_seg that is not 16-byte aligned
      rc = launch_bwd_pixel<HeadShape<C>, true>(a, grid, lds, hs);
  }
  if (rc != DFL_OK || !fused) return rc;
  hipLaunchKernelGGL(head_wgrad_finish_kernel, dim3(256), dim3(256), 0, hs, a->wg_partial, (int)grid, a->dw_seg, a->dw_l1, a->dw_l2, a->F,
                     a->NC, a->NM, a->L);
  return check_launch("dfl_head_bwd (weight-gradient sums)");
}

static inline bool head_is_large(int NC, int NM, int L) { return NC > DFL_HEAD_MAX_NC || NM > DFL_HEAD_MAX_NM || L > DFL_HEAD_MAX_L; }

}  // namespace dfl

using namespace dfl;

extern "C" int dfl_head_scratch_ld(int32_t F) { return scratch_ld<HeadSmall>(F); }
extern "C" int dfl_head_scratch_off(int32_t F, int32_t which) { return scratch_off<HeadSmall>(F, which); }

extern "C" int dfl_head_scratch_ld_for(int32_t F, int32_t NC, int32_t NM, int32_t L) {
  return head_is_large(NC, NM, L) ? scratch_ld<HeadLarge>(F) : scratch_ld<HeadSmall>(F);
}
extern "C" int dfl_head_scratch_off_for(int32_t F, int32_t NC, int32_t NM, int32_t L, int32_t which) {
  return head_is_large(NC, NM, L) ? scratch_off<HeadLarge>(F, which) : scratch_off<HeadSmall>(F, which);
}

extern "C" int dfl_head_fwd(const dfl_head_fwd_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a && a->x && a->w_seg && a->seg, "dfl_head_fwd: missing pointer");
  DFL_REQUIRE(a->N > 0 && a->H > 0 && a->W > 0 && a->ldx >= a->F, "dfl_head_fwd: bad sizes");
  DFL_REQUIRE(a->L == 0 || a->heat != nullptr, "dfl_head_fwd: heat output required when L > 0");
  return head_is_large(a->NC, a->NM, a->L) ? launch_fwd<HeadLarge>(a, stream) : launch_fwd<HeadSmall>(a, stream);
}

extern "C" int dfl_head_wgrad_blocks(int64_t M) {
  DFL_REQUIRE(M > 0, "dfl_head_wgrad_blocks: bad size");
  return (int)head_wgrad_grid(M);
}

extern "C" int dfl_head_bwd(const dfl_head_bwd_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a && a->x && a->seg && a->dseg && a->w_seg && a->dx && (a->scratch || a->dw_seg), "dfl_head_bwd: missing pointer");
  DFL_REQUIRE(a->N > 0 && a->H > 0 && a->W > 0 && a->ldx >= a->F && a->lddx >= a->F, "dfl_head_bwd: bad sizes");
  DFL_REQUIRE(a->lddx % (a->x_bf16 ? 8 : 4) == 0 && aligned16(a->dx), "dfl_head_bwd: dx alignment");
  return head_is_large(a->NC, a->NM, a->L) ? launch_bwd<HeadLarge>(a, stream) : launch_bwd<HeadSmall>(a, stream);
}
