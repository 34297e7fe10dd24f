// Heads on the matrix cores (bf16 features, F = 32, up to 8 classes / 24 mid channels / 16 landmarks; round 3).
//
// Channel-major products: D[channel][pixel] = W[channel][k] * B[k][pixel] with v_mfma_f32_32x32x16_bf16 -- the weights are the
// A operand (32 rows), 32 consecutive pixels the columns.  A lane then owns ONE pixel (column lane & 31) in every product,
// its B fragment of the features is 16 bytes of that pixel's NHWC row straight from global memory, and the per-pixel work
// between the products (softmax, its Jacobian) stays inside the lane pair (l, l + 32) that shares the pixel.  A product's
// result becomes the next product's B operand by four v_permlane32_swap per 16 rows (acc_to_b): no LDS, no barrier in the
// chain.  fp32 weights and computed operands enter as hi + lo bf16 pairs (hi*hi + hi*lo + lo*hi, fp32 accumulation: 2^-17
// of the value, the accuracy of the fp32 kernels this replaces); the features are exact bf16.
//   rows of U  = [logits (0..7) | mid (8..31)]      mid = (W1x + W1c Wseg) x   (folded once per wave, fp32)
//   rows of V  = [dlogits (0..7) | dmid (8..31)]    dmid = W2^T dheat;  dlogits = softmax'(seg, dseg) + W1c^T dmid
//   dx         = [Wseg^T | W1x^T] V
// The three weight gradients are taken from the tile's row image (head_wgrad.h): the rows [V | dheat] and [x | U] go to LDS as
// bf16 -- a lane's B fragments ARE 16-byte pieces of those rows -- and four waves contract them over the 128 pixels of the tile.
#pragma once
#include "common.h"
#include "head_wgrad.h"

namespace dfl {

struct HFrag { bf16x8_t hi, lo; };

__device__ __forceinline__ HFrag hsplit8(const float* v) {
  HFrag f;
  float r[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const __bf16 h = (__bf16)v[e];
    f.hi[e] = h;
    r[e] = v[e] - (float)h;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) f.lo[e] = (__bf16)r[e];
  return f;
}

// acc += A * B with both operands as hi + lo pairs (three products); B exact bf16: two
__device__ __forceinline__ void hmm3(f32x16& acc, const HFrag& a, const HFrag& b) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.lo, b.hi, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi, b.lo, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi, b.hi, acc, 0, 0, 0);
}
__device__ __forceinline__ void hmm2(f32x16& acc, const HFrag& a, const bf16x8_t b) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.lo, b, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi, b, acc, 0, 0, 0);
}

// Rows 16 s .. 16 s + 15 of a product (accumulator registers 8 s .. 8 s + 7: rows 16 s + {0-3, 8-11} in the lower lane half,
// {4-7, 12-15} in the upper) -> the B-fragment order: 8 consecutive rows 16 s + 8 h .. per lane of half h.
__device__ __forceinline__ void acc_to_b(const f32x16& acc, int s, float* v) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[8 * s + j]), __float_as_uint(acc[8 * s + 4 + j]), false, false);
    v[j] = __uint_as_float(r[0]);
    v[4 + j] = __uint_as_float(r[1]);
  }
}

// The head's matrices as A fragments (row = lane & 31, k = 16 s + 8 (lane >> 5) + e), built once per wave from the fp32 weights
struct HeadW {
  const float* w_seg; const float* w_l1; const float* w_l2;
  int NC, NM, L, K1;
  __device__ __forceinline__ float wseg(int c, int f) const { return c < NC ? w_seg[c * 32 + f] : 0.f; }
  __device__ __forceinline__ float w1x(int j, int f) const { return j < NM ? w_l1[j * K1 + f] : 0.f; }
  __device__ __forceinline__ float w1c(int j, int c) const { return (j < NM && c < NC) ? w_l1[j * K1 + 32 + c] : 0.f; }
  __device__ __forceinline__ float w2(int l, int j) const { return (l < L && j < NM) ? w_l2[l * NM + j] : 0.f; }
  // U = [Wseg ; W1x + W1c Wseg] x
  __device__ __forceinline__ HFrag a_u(int m, int k0, bool lands) const {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = m < 8 ? wseg(m, k0 + e) : (lands ? w1x(m - 8, k0 + e) : 0.f);
    if (lands && m >= 8 && m - 8 < NM) {
      for (int c = 0; c < NC; ++c) {             // rows of Wseg are 128 bytes: two 16-byte loads per class (the same for every lane)
        const float wc = w_l1[(m - 8) * K1 + 32 + c];
        const float4 s0 = *reinterpret_cast<const float4*>(w_seg + c * 32 + k0), s1 = *reinterpret_cast<const float4*>(w_seg + c * 32 + k0 + 4);
        v[0] = fmaf(wc, s0.x, v[0]); v[1] = fmaf(wc, s0.y, v[1]); v[2] = fmaf(wc, s0.z, v[2]); v[3] = fmaf(wc, s0.w, v[3]);
        v[4] = fmaf(wc, s1.x, v[4]); v[5] = fmaf(wc, s1.y, v[5]); v[6] = fmaf(wc, s1.z, v[6]); v[7] = fmaf(wc, s1.w, v[7]);
      }
    }
    return hsplit8(v);
  }
  // heat = W2 mid: row l, k = row of U
  __device__ __forceinline__ HFrag a_h(int m, int k0) const {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (k0 + e >= 8) ? w2(m, k0 + e - 8) : 0.f;
    return hsplit8(v);
  }
  // dmid = W2^T dheat: row 8 + j, k = landmark
  __device__ __forceinline__ HFrag a_dm(int m, int k0) const {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = m >= 8 ? w2(k0 + e, m - 8) : 0.f;
    return hsplit8(v);
  }
  // dlogits += W1c^T dmid: row c, k = row of V
  __device__ __forceinline__ HFrag a_dl(int m, int k0) const {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (m < 8 && k0 + e >= 8) ? w1c(k0 + e - 8, m) : 0.f;
    return hsplit8(v);
  }
  // dx = Wseg^T dlogits + W1x^T dmid: row f, k = row of V
  __device__ __forceinline__ HFrag a_dx(int m, int k0, bool lands) const {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int r = k0 + e;
      v[e] = r < 8 ? wseg(r, m) : (lands ? w1x(r - 8, m) : 0.f);
    }
    return hsplit8(v);
  }
};

constexpr int HM_TILE = HEAD_WG_ROWS;   // pixels per workgroup tile (4 waves x 32): one row image

__device__ __forceinline__ bf16x8_t hload_x(const unsigned short* xb, int64_t m, int64_t M, int ldx, int s, int h) {
  uint4 w = make_uint4(0u, 0u, 0u, 0u);
  if (m < M) w = *reinterpret_cast<const uint4*>(xb + m * ldx + 16 * s + 8 * h);
  return __builtin_bit_cast(bf16x8_t, w);
}

template <bool LANDS>
__global__ void __launch_bounds__(256) head_mfma_fwd_kernel(const dfl_head_fwd_args a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l = lane & 31, h = lane >> 5;
  const HeadW W{a.w_seg, a.w_l1, a.w_l2, a.NC, a.NM, a.L, 32 + a.NC};
  HFrag au[2], ah[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    au[s] = W.a_u(l, 16 * s + 8 * h, LANDS);
    if (LANDS) ah[s] = W.a_h(l, 16 * s + 8 * h);
  }
  const unsigned short* xb = reinterpret_cast<const unsigned short*>(a.x);
  const int64_t HW = (int64_t)a.H * a.W, M = (int64_t)a.N * HW;
  const int64_t ntiles = (M + HM_TILE - 1) / HM_TILE;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t m = t * HM_TILE + wave * 32 + l;
    const bf16x8_t x0 = hload_x(xb, m, M, a.ldx, 0, h), x1 = hload_x(xb, m, M, a.ldx, 1, h);
    f32x16 u;
#pragma unroll
    for (int r = 0; r < 16; ++r) u[r] = 0.f;
    hmm2(u, au[0], x0);
    hmm2(u, au[1], x1);
    const int64_t n = m / HW, pp = m - n * HW;
    if (LANDS) {
      f32x16 ht;
#pragma unroll
      for (int r = 0; r < 16; ++r) ht[r] = 0.f;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        float v[8];
        acc_to_b(u, s, v);
        hmm3(ht, ah[s], hsplit8(v));
      }
      if (m < M) {
        float* hp = a.heat + n * a.L * HW + pp;
#pragma unroll
        for (int r = 0; r < 8; ++r) {            // rows 0 .. 15
          const int row = mfma32_row(r, lane);
          if (row < a.L) hp[(int64_t)row * HW] = ht[r];
        }
      }
    }
    // logits: rows 0-3 in the lower lane half, 4-7 in the upper
    float lg[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) lg[j] = u[j];
    if (a.softmax) {
      float mx = -INFINITY;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (4 * h + j < a.NC) mx = fmaxf(mx, lg[j]);
      mx = fmaxf(mx, xor32(mx));
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        lg[j] = 4 * h + j < a.NC ? expf(lg[j] - mx) : 0.f;
        sum += lg[j];
      }
      sum += xor32(sum);
      const float inv = 1.0f / sum;
#pragma unroll
      for (int j = 0; j < 4; ++j) lg[j] *= inv;
    }
    if (m < M) {
      float* sp = a.seg + n * a.NC * HW + pp;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (4 * h + j < a.NC) sp[(int64_t)(4 * h + j) * HW] = lg[j];
    }
  }
}

template <bool LANDS>
__global__ void __launch_bounds__(256) head_mfma_bwd_kernel(const dfl_head_bwd_args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ab[];       // the tile's row image: HEAD_WG_LDS bytes
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l = lane & 31, h = lane >> 5;
  const bool lands = LANDS && a.dheat != nullptr;                           // (no landmark gradient: dmid = 0)
  const HeadW W{a.w_seg, a.w_l1, a.w_l2, a.NC, a.NM, a.L, 32 + a.NC};
  HFrag au[2], adl[2], adx[2], adm;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    au[s] = W.a_u(l, 16 * s + 8 * h, LANDS);
    adx[s] = W.a_dx(l, 16 * s + 8 * h, LANDS);
    if (LANDS) adl[s] = W.a_dl(l, 16 * s + 8 * h);
  }
  if (LANDS) adm = W.a_dm(l, 8 * h);
  const HeadWgLane wg;
  f32x16 wacc;
#pragma unroll
  for (int r = 0; r < 16; ++r) wacc[r] = 0.f;
  unsigned char* myrow = ab + (size_t)(wave * 32 + l) * HEAD_WG_PITCH;
  *reinterpret_cast<uint4*>(myrow + HEAD_WG_ZERO + 16 * h) = make_uint4(0u, 0u, 0u, 0u);    // stays zero
  const unsigned short* xb = reinterpret_cast<const unsigned short*>(a.x);
  unsigned short* dxb = reinterpret_cast<unsigned short*>(a.dx);
  const unsigned short* sob = reinterpret_cast<const unsigned short*>(a.stat_other);
  float st1[16], st2[16];                                                  // live statistics: [s][e] sums of dx and of dx * r
#pragma unroll
  for (int q = 0; q < 16; ++q) st1[q] = st2[q] = 0.f;
  const int64_t HW = (int64_t)a.H * a.W, M = (int64_t)a.N * HW;
  const int64_t ntiles = (M + HM_TILE - 1) / HM_TILE;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t m = t * HM_TILE + wave * 32 + l;
    const bool live = m < M;
    const int64_t n = m / HW, pp = m - n * HW;
    const bf16x8_t x0 = hload_x(xb, m, M, a.ldx, 0, h), x1 = hload_x(xb, m, M, a.ldx, 1, h);
    // upstream gradients in the layouts the products want
    float dh[8], g[4], sv[4];
#pragma unroll
    for (int e = 0; e < 8; ++e) dh[e] = (lands && live && 8 * h + e < a.L) ? a.dheat[(n * a.L + 8 * h + e) * HW + pp] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool ok = live && 4 * h + j < a.NC;
      g[j] = ok ? a.dseg[(n * a.NC + 4 * h + j) * HW + pp] : 0.f;
      sv[j] = ok ? a.seg[(n * a.NC + 4 * h + j) * HW + pp] : 0.f;
    }
    // U = [logits | mid]
    f32x16 u, v;
#pragma unroll
    for (int r = 0; r < 16; ++r) u[r] = v[r] = 0.f;
    hmm2(u, au[0], x0);
    hmm2(u, au[1], x1);
    // V = [dlogits | dmid]: dmid = W2^T dheat, dlogits = W1c^T dmid + softmax Jacobian
    const HFrag dhf = hsplit8(dh);
    if (LANDS) {
      hmm3(v, adm, dhf);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        float t8[8];
        acc_to_b(v, s, t8);
        hmm3(v, adl[s], hsplit8(t8));          // adds rows 0..7 only (the other rows of adl are zero)
      }
    }
    {
      float dot = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) dot = fmaf(g[j], sv[j], dot);
      dot += xor32(dot);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] += a.softmax ? sv[j] * (g[j] - dot) : g[j];
    }
    // dx = [Wseg^T | W1x^T] V; the B fragments of V and U are also this pixel's weight-gradient rows
    f32x16 dx;
#pragma unroll
    for (int r = 0; r < 16; ++r) dx[r] = 0.f;
    HFrag vf[2];
    bf16x8_t uf[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float t8[8];
      acc_to_b(v, s, t8);
      vf[s] = hsplit8(t8);
      hmm3(dx, adx[s], vf[s]);
      acc_to_b(u, s, t8);
#pragma unroll
      for (int e = 0; e < 8; ++e) uf[s][e] = (__bf16)t8[e];
    }
    __syncthreads();                            // the previous tile's weight-gradient reads are done
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      *reinterpret_cast<bf16x8_t*>(myrow + HEAD_WG_V + 32 * s + 16 * h) = vf[s].hi;
      *reinterpret_cast<bf16x8_t*>(myrow + HEAD_WG_U + 32 * s + 16 * h) = uf[s];
    }
    *reinterpret_cast<bf16x8_t*>(myrow + HEAD_WG_DHEAT + 16 * h) = dhf.hi;
    *reinterpret_cast<bf16x8_t*>(myrow + HEAD_WG_X + 16 * h) = x0;
    *reinterpret_cast<bf16x8_t*>(myrow + HEAD_WG_X + 32 + 16 * h) = x1;
    // dx rows: 8 consecutive features per lane and 16-row group
    if (live) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        float t8[8];
        acc_to_b(dx, s, t8);
        const u32x4 w = pack8(t8);
        *reinterpret_cast<u32x4*>(dxb + m * a.lddx + 16 * s + 8 * h) = w;
        if (a.stat_totals != nullptr) {                                    // sums of the values as stored
          const u32x4 rr = *reinterpret_cast<const u32x4*>(sob + m * a.ldso + 16 * s + 8 * h);
#pragma unroll
          for (int e2 = 0; e2 < 4; ++e2) {
            st1[8 * s + 2 * e2] += bf_lo(w[e2]);
            st1[8 * s + 2 * e2 + 1] += bf_hi(w[e2]);
            st2[8 * s + 2 * e2] = fmaf(bf_lo(w[e2]), bf_lo(rr[e2]), st2[8 * s + 2 * e2]);
            st2[8 * s + 2 * e2 + 1] = fmaf(bf_hi(w[e2]), bf_hi(rr[e2]), st2[8 * s + 2 * e2 + 1]);
          }
        }
      }
    }
    __syncthreads();
    wg.product(ab, wacc);
  }
  if (a.stat_totals != nullptr) {
    // live statistics of dx (include/dfl_hip.h): this lane's sums over its pixels -> the 32 lanes of its half (same channels,
    // other pixels) by butterflies -> the four waves through LDS, a fixed order -> one fp64 atomic per (channel, sum)
    __syncthreads();
    float* sred = reinterpret_cast<float*>(ab);                            // [4 waves][2 halves][32]: (sum, e) pairs
#pragma unroll
    for (int q = 0; q < 32; ++q) {
      float v = q < 16 ? st1[q] : st2[q - 16];
#pragma unroll
      for (int off = 1; off < 32; off <<= 1) v += __shfl_xor(v, off, 64);
      if (l == 0) sred[(wave * 2 + h) * 32 + q] = v;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
      // thread = (which, s, hh, e): channel 16 s + 8 hh + e
      const int which = threadIdx.x >> 5, s_ = (threadIdx.x >> 4) & 1, hh = (threadIdx.x >> 3) & 1, e = threadIdx.x & 7;
      const int q = which * 16 + s_ * 8 + e;
      const float t = ((sred[(0 * 2 + hh) * 32 + q] + sred[(1 * 2 + hh) * 32 + q]) + sred[(2 * 2 + hh) * 32 + q]) + sred[(3 * 2 + hh) * 32 + q];
      bn_live_add(a.stat_totals, (int)blockIdx.x, which, 32, 16 * s_ + 8 * hh + e, t);
    }
  }
  wg.store(a.wg_partial, wacc);
}

}  // namespace dfl
