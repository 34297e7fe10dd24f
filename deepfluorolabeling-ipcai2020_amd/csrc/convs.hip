// Latency form of the convolution (round 5): the kernel dfl_conv2d takes for the SMALL problems of a batch-1 inference
// forward (dfl_conv_args.latency_form; reference: the per-image loops of train_test_code/util.py:116-165 and :318-356 call
// UNet.forward, unet.py:161-193, on one image at a time).  One kernel body for bf16 tensors and for fp32 tensors; what differs
// between them is an element form (ElemBF16, ElemF32<MATH> below).
//
// Why a second kernel for the same contract.  At batch 1 and 192x192 every layer of the paper network is 0.01 - 1 GFLOP: the
// forward is a chain of 44 dependent convolutions whose time is not throughput but the LENGTH OF EACH KERNEL'S DEPENDENCY
// CHAIN.  The patch-resident kernel (convp_bf16.hip) is built for throughput -- geometry tables, patch image staged through
// LDS (global -> registers -> LDS -> barrier), weight ring, accumulators -> LDS -> rows -> stores -- and takes 5 - 15 us per
// launch on these shapes where a dependent launch boundary costs 1.5 (docs/experiments/infer192_r05: 58 kernels, 0.48 ms;
// a grid barrier inside one persistent launch costs 4.2 us without and 12 us with agent-scope fences on this chip, so one
// launch for the whole forward is no way out either).  This kernel keeps the chain as short as the hardware allows:
//   * no LDS staging, no barrier in front of the matrix instructions: a wave owns ONE 32-pixel x 32-channel output tile and
//     a range of k-steps of 16 channels; both MFMA operands come straight from global memory (L2) in the fragment layout -- the
//     pixel fragment is the lane's own 8 consecutive channels of its pixel at the tap's offset (zero padding = out-of-range
//     buffer offset), the weight fragment a coalesced run of the packed weights;
//   * the loads of two register sets of k-steps are in flight before the first matrix instruction;
//   * D = W * X orientation: a lane ends up with 4 consecutive channels of ITS pixel per accumulator group, so the epilogue
//     (bias, ReLU, + BN(add), 2x2 scatter) runs on the accumulators and stores 4 channels per group -- no transpose;
//   * K is split over the 8 waves of a workgroup (partial tiles meet in LDS, summed in a fixed order) so that a layer with
//     18 ... 576 k-steps still is a few k-steps deep per wave, and over workgroups (fp32 partial slices + a finish kernel:
//     convp_finish_kernel for bf16 tensors, conv_finish_kernel of conv_gemm.hip for fp32 tensors) only for the weight-heavy
//     levels whose 5 - 19 MB of weights need every CU's memory pipe.
//
// bf16 tensors (ElemBF16).  A fragment is 16 bytes per operand, the weights are the [k/16][n][16] layout convp uses (one
// coalesced 1 KiB run per k-step), a register set holds 9 k-steps.  Same arithmetic as convp_kernel: bf16 products, fp32
// accumulation (another summation order), values rounded to bf16 once.
//
// fp32 tensors (ElemF32<MATH>), for the arithmetics that hold north_star's 1e-4 forward bar -- math mode 0 (fp32 matrix
// instructions, v_mfma_f32_32x32x2_f32) and mode 1 (bf16x3: every fp32 operand value cut into hi + lo bf16 parts, hi*hi + hi*lo +
// lo*hi on the bf16 matrix pipe).  A fragment is 32 bytes per operand -- two quads of the packed weights [K/4][N][4] (plain fp32
// or split hi4 | lo4 bf16) -- and a register set holds 4 k-steps (a step holds 16 registers here).  Nothing is rounded on the way,
// so the producer-side BatchNorm (out_scale) IS the consumer's affine on load.  The fp32 instruction contracts k in pairs
// {j, 8 + j} of a step (lane half = k half): sums are formed in another order than conv_gemm_kernel's, within the 1e-6-class
// differences every tile shape of that kernel has against every other.
//
// PAIR form (dfl_conv2d_pair): the last 3x3 convolution of a residual block and the block's 1x1 convolution -- y1 = ReLU(conv(x) +
// bias), y2 = conv1x1(x3) + bias3 + BN(y1) (unet.py:218-231) -- as ONE launch: the waves of a tile take the k-steps of the second
// product behind their share of the first (a second accumulator tile), the epilogue stores y1 and forms y2 from the STORED value
// (bf16: the rounded one) exactly as the two launches do.  11 of the 44 launches of a forward.  The two element forms schedule the
// second product differently, each as measured: bf16 requests its at most SU2 k-steps per wave up front into registers of their
// own, fp32 runs it as a second pass through the first product's registers.
#include <stdlib.h>
#include <string.h>

#include "common.h"
#include "convp.h"

namespace dfl {

// Waves per workgroup, a template parameter: 8 (512 threads, one workgroup per CU) where eight waves share a tile's k-steps, 4 (256
// threads, two workgroups per CU) otherwise -- a layer of 1152 wave tasks then is 288 workgroups over all 256 CUs instead of 144 on 144
// (the fragments of this form are not reused across waves: a CU's L1 fill is what a 36-k-step layer waits for).
constexpr int SCONST_PER_WAVE = 6 * 32;            // per wave: bias, add_scale, add_shift, bias3, out_scale, out_shift of its tile's 32 columns

// What the kernels take of a plan: the block and the latency fields of ConvP under ConvP's names.  The 180 bytes of patch geometry a
// ConvP carries for the other families stay on the host: a launch of this form is bound by its kernel arguments and first loads
// (with a whole ConvP the bf16x3 batch-1 forward measured 0.9 % slower, docs/experiments/convs_unified)
struct ConvS {
  dfl_conv_args a;
  int Mtot, Cout, Hg, Wg, splits;
  int s_mt, s_nt, s_ksplit_shift, s_cpk_shift, s_ksteps, s_kper;
  uint32_t x_bytes, w_bytes;
};
static ConvS convs_args(const ConvP& p) {
  ConvS k;
  k.a = p.a;
  k.Mtot = p.Mtot; k.Cout = p.Cout; k.Hg = p.Hg; k.Wg = p.Wg; k.splits = p.splits;
  k.s_mt = p.s_mt; k.s_nt = p.s_nt; k.s_ksplit_shift = p.s_ksplit_shift; k.s_cpk_shift = p.s_cpk_shift; k.s_ksteps = p.s_ksteps; k.s_kper = p.s_kper;
  k.x_bytes = p.x_bytes; k.w_bytes = p.w_bytes;
  return k;
}

// second convolution of a pair (1x1, stride 1, no affine on load): y2 = x3 * w3 + bias3 + add_scale * y1 + add_shift
struct ConvPair {
  const void* x3;
  const void* w3;
  const float* bias3;
  const float* add_scale;
  const float* add_shift;
  void* y2;
  int ldx3, ldy2, ksteps2, kper2;
  int x3_one;                      // the network's first block: x3 is the 1-channel fp32 image, w3 the fp32 quad-packed weights
  int w3_split;                    // fp32 tensors: dfl_conv_args.w_split of the second convolution
  uint32_t x3_bytes, w3_bytes;
};

// ---- element forms: what the kernel body below leaves to the tensors' number format
//   BYTES, Frag, SU       bytes per element, the fragment of a k-step (8 channels of a pixel / of a weight column), k-steps per register set
//   w_addr, load_x/_w     the fragment loads; the weight fragment's address in the packed layout
//   affine, mma           the BatchNorm affine on load (zero padding after it), the product of a k-step
//   Store: Out4, idx_t,   four output channels of a pixel in memory: their address (32-bit element offsets where the planner
//   at, val, round4       guarantees them), their values as fp32, four fp32 as they are stored
//   PAIR_UPFRONT, SU2     the schedule of a pair's second product; PAIR_AFF: pairs whose first convolution has an affine on load exist
struct StoreBF16 {
  typedef u32x2 Out4;
  typedef uint32_t idx_t;
  static __device__ __forceinline__ Out4* at(const void* base, idx_t pix, int ld, int col) {
    return reinterpret_cast<Out4*>(reinterpret_cast<unsigned short*>(const_cast<void*>(base)) + (pix * (uint32_t)ld + (uint32_t)col));
  }
  static __device__ __forceinline__ Out4 zero4() { return (Out4){0u, 0u}; }
  static __device__ __forceinline__ float4 val(const Out4 w) { return make_float4(bf_lo(w.x), bf_hi(w.x), bf_lo(w.y), bf_hi(w.y)); }
  static __device__ __forceinline__ Out4 round4(const float4 v) { return (Out4){pack_bf2(v.x, v.y), pack_bf2(v.z, v.w)}; }
};
struct StoreF32 {
  typedef float4 Out4;
  typedef int64_t idx_t;
  static __device__ __forceinline__ Out4* at(const void* base, idx_t pix, int ld, int col) {
    return reinterpret_cast<Out4*>(reinterpret_cast<float*>(const_cast<void*>(base)) + (pix * ld + col));
  }
  static __device__ __forceinline__ Out4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  static __device__ __forceinline__ float4 val(const Out4 w) { return w; }
  static __device__ __forceinline__ Out4 round4(const float4 v) { return v; }
};

struct ElemBF16 : StoreBF16 {
  typedef StoreBF16 Store;
  static constexpr const char* WHAT = "dfl_conv2d (bf16, latency form)";
  static constexpr const char* PAIR_WHAT = "dfl_conv2d_pair";
  static constexpr int BYTES = 2;
  static constexpr int SU = 9;
  static constexpr bool PAIR_UPFRONT = true, PAIR_AFF = false;
  static constexpr int SU2 = 4;    // k-steps per wave of a pair's second product (registers of their own)
  typedef u32x4 Frag;              // one 16-byte load
  struct WAddr { uint32_t row, col; };               // chunk-packed [k/16][n][16]: bytes per k-step, this lane's column and half
  static __device__ __forceinline__ WAddr w_addr(int Ntot, int n, int lh) { return {(uint32_t)Ntot * 32u, (uint32_t)n * 32u + (uint32_t)lh * 16u}; }
  static __device__ __forceinline__ Frag load_x(__amdgpu_buffer_rsrc_t rs, bool ok, uint32_t off) {
    return __builtin_amdgcn_raw_buffer_load_b128(rs, ok ? off : OOB, 0, 0);
  }
  static __device__ __forceinline__ Frag load_w(__amdgpu_buffer_rsrc_t rs, bool ok, int s, const WAddr& wa) {
    return __builtin_amdgcn_raw_buffer_load_b128(rs, ok ? (uint32_t)s * wa.row + wa.col : OOB, 0, 0);
  }
  static __device__ __forceinline__ void affine(Frag& x, const float4 s0, const float4 s1, const float4 h0, const float4 h1, bool ok) {
    Frag y;
    y.x = pack_bf2(fmaf(bf_lo(x.x), s0.x, h0.x), fmaf(bf_hi(x.x), s0.y, h0.y));
    y.y = pack_bf2(fmaf(bf_lo(x.y), s0.z, h0.z), fmaf(bf_hi(x.y), s0.w, h0.w));
    y.z = pack_bf2(fmaf(bf_lo(x.z), s1.x, h1.x), fmaf(bf_hi(x.z), s1.y, h1.y));
    y.w = pack_bf2(fmaf(bf_lo(x.w), s1.z, h1.z), fmaf(bf_hi(x.w), s1.w, h1.w));
    x.x = ok ? y.x : 0u; x.y = ok ? y.y : 0u; x.z = ok ? y.z : 0u; x.w = ok ? y.w : 0u;
  }
  static __device__ __forceinline__ void mma(f32x16& acc, const Frag& w, const Frag& x, bool) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, w), __builtin_bit_cast(bf16x8_t, x), acc, 0, 0, 0);
  }
};

// 8 fp32 values -> hi and lo bf16 parts (hi = bf16(v), lo = bf16(v - hi)): the split conv_gemm_kernel applies at its LDS write
__device__ __forceinline__ void fsplit8(const u32x4 v0, const u32x4 v1, u32x4* hi, u32x4* lo) {
  const float f[8] = {__uint_as_float(v0.x), __uint_as_float(v0.y), __uint_as_float(v0.z), __uint_as_float(v0.w),
                      __uint_as_float(v1.x), __uint_as_float(v1.y), __uint_as_float(v1.z), __uint_as_float(v1.w)};
  uint32_t h[4], l[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    h[e] = pack_bf2(f[2 * e], f[2 * e + 1]);
    l[e] = pack_bf2(f[2 * e] - bf_lo(h[e]), f[2 * e + 1] - bf_hi(h[e]));
  }
  *hi = (u32x4){h[0], h[1], h[2], h[3]};
  *lo = (u32x4){l[0], l[1], l[2], l[3]};
}

template <int MATH>                // 0: fp32 matrix instructions, 1: bf16x3
struct ElemF32 : StoreF32 {
  typedef StoreF32 Store;
  static constexpr const char* WHAT = "dfl_conv2d (fp32 tensors, latency form)";
  static constexpr const char* PAIR_WHAT = "dfl_conv2d_pair (fp32 tensors)";
  static constexpr int BYTES = 4;
  static constexpr int SU = 4;
  static constexpr bool PAIR_UPFRONT = false, PAIR_AFF = true;
  static constexpr int SU2 = 0;    // (the second product of a pair is a second pass through the first one's registers)
  struct Frag { u32x4 v0, v1; };   // two 16-byte loads
  struct WAddr { uint32_t row, col; int lh2; };      // quad-packed [K/4][N][4]: bytes per quad row, this lane's column, its half's first quad of a step
  static __device__ __forceinline__ WAddr w_addr(int Ntot, int n, int lh) { return {(uint32_t)Ntot * 16u, (uint32_t)n * 16u, 2 * lh}; }
  static __device__ __forceinline__ Frag load_x(__amdgpu_buffer_rsrc_t rs, bool ok, uint32_t off) {
    Frag f;
    f.v0 = __builtin_amdgcn_raw_buffer_load_b128(rs, ok ? off : OOB, 0, 0);
    f.v1 = __builtin_amdgcn_raw_buffer_load_b128(rs, ok ? off + 16u : OOB, 0, 0);
    return f;
  }
  static __device__ __forceinline__ Frag load_w(__amdgpu_buffer_rsrc_t rs, bool ok, int s, const WAddr& wa) {
    const uint32_t wo = (uint32_t)(s * 4 + wa.lh2) * wa.row + wa.col;
    Frag f;
    f.v0 = __builtin_amdgcn_raw_buffer_load_b128(rs, ok ? wo : OOB, 0, 0);
    f.v1 = __builtin_amdgcn_raw_buffer_load_b128(rs, ok ? wo + wa.row : OOB, 0, 0);
    return f;
  }
  static __device__ __forceinline__ void affine(Frag& x, const float4 s0, const float4 s1, const float4 h0, const float4 h1, bool ok) {
    x.v0.x = ok ? __float_as_uint(fmaf(__uint_as_float(x.v0.x), s0.x, h0.x)) : 0u;
    x.v0.y = ok ? __float_as_uint(fmaf(__uint_as_float(x.v0.y), s0.y, h0.y)) : 0u;
    x.v0.z = ok ? __float_as_uint(fmaf(__uint_as_float(x.v0.z), s0.z, h0.z)) : 0u;
    x.v0.w = ok ? __float_as_uint(fmaf(__uint_as_float(x.v0.w), s0.w, h0.w)) : 0u;
    x.v1.x = ok ? __float_as_uint(fmaf(__uint_as_float(x.v1.x), s1.x, h1.x)) : 0u;
    x.v1.y = ok ? __float_as_uint(fmaf(__uint_as_float(x.v1.y), s1.y, h1.y)) : 0u;
    x.v1.z = ok ? __float_as_uint(fmaf(__uint_as_float(x.v1.z), s1.z, h1.z)) : 0u;
    x.v1.w = ok ? __float_as_uint(fmaf(__uint_as_float(x.v1.w), s1.w, h1.w)) : 0u;
  }
  static __device__ __forceinline__ void mma(f32x16& acc, const Frag& w, const Frag& x, bool w_split) {
    if constexpr (MATH == 0) {
      const float wv[8] = {__uint_as_float(w.v0.x), __uint_as_float(w.v0.y), __uint_as_float(w.v0.z), __uint_as_float(w.v0.w),
                           __uint_as_float(w.v1.x), __uint_as_float(w.v1.y), __uint_as_float(w.v1.z), __uint_as_float(w.v1.w)};
      const float xv[8] = {__uint_as_float(x.v0.x), __uint_as_float(x.v0.y), __uint_as_float(x.v0.z), __uint_as_float(x.v0.w),
                           __uint_as_float(x.v1.x), __uint_as_float(x.v1.y), __uint_as_float(x.v1.z), __uint_as_float(x.v1.w)};
#pragma unroll
      for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[j], xv[j], acc, 0, 0, 0);
    } else {
      u32x4 whi, wlo, xhi, xlo;
      if (w_split) {                                        // split quads: 4 hi bf16 | 4 lo bf16 per 16-byte slot
        whi = (u32x4){w.v0.x, w.v0.y, w.v1.x, w.v1.y};
        wlo = (u32x4){w.v0.z, w.v0.w, w.v1.z, w.v1.w};
      } else {
        fsplit8(w.v0, w.v1, &whi, &wlo);
      }
      fsplit8(x.v0, x.v1, &xhi, &xlo);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, wlo), __builtin_bit_cast(bf16x8_t, xhi), acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, whi), __builtin_bit_cast(bf16x8_t, xlo), acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, whi), __builtin_bit_cast(bf16x8_t, xhi), acc, 0, 0, 0);
    }
  }
};

template <class S>
__global__ void convs_pair_finish_kernel(const ConvS p, const ConvPair q);       // (K-sliced pairs, below)

template <class P, bool AFF, bool PAIR, int SWAVES>
__global__ void __launch_bounds__(64 * SWAVES, SWAVES == 8 ? 1 : 2) convs_kernel(const ConvS p, const ConvPair q) {
  typedef typename P::Frag Frag;
  typedef typename P::Out4 Out4;
  typedef typename P::idx_t idx_t;
  constexpr int SU = P::SU;
  constexpr bool UPFRONT = PAIR && P::PAIR_UPFRONT;
  constexpr int NACC = PAIR ? 2 : 1;
  constexpr int SCONST_FLOATS = SWAVES * SCONST_PER_WAVE;
  constexpr int TABQ = 1024 / (64 * SWAVES);            // table entries per thread (Cin <= 1024)
  constexpr int SRED = SWAVES * NACC * 16 * 64;          // floats: partial tiles of the workgroup's waves
  extern __shared__ __attribute__((aligned(16))) float sm[];      // [8][NACC*16][64] partial tiles, [8][6][32] constants, [2][Cin] scale / shift
  const dfl_conv_args& a = p.a;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int ksh = p.s_ksplit_shift, ksplit = 1 << ksh;
  const int grp = wave >> ksh, kw = wave & (ksplit - 1);
  const int tile = (int)blockIdx.x * (SWAVES >> ksh) + grp;
  const bool tok = tile < p.s_mt * p.s_nt;
  const int mi = tok ? tile / p.s_nt : 0, ni = tok ? tile - mi * p.s_nt : 0;

  // this lane's pixel of the gather grid and the input pixel of its tap (0, 0)
  const int pix = mi * 32 + li;
  const bool pok = tok && pix < p.Mtot;
  const int HW = p.Hg * p.Wg;
  const int img = pix / HW, rem = pix - img * HW;
  const int gy = rem / p.Wg, gx = rem - gy * p.Wg;
  const int iy0 = gy * a.stride - a.pad, ix0 = gx * a.stride - a.pad;
  const int pbase = (img * a.Hin + iy0) * a.Win + ix0;
  const uint32_t ldxb = (uint32_t)a.ldx * (uint32_t)P::BYTES, lhb = (uint32_t)lh * (uint32_t)(8 * P::BYTES);
  // this lane's weight column
  const int n = ni * 32 + li;
  const bool nok = tok && n < a.Ntot;
  const typename P::WAddr wa = P::w_addr(a.Ntot, n, lh);

  __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, (int)p.x_bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, (int)p.w_bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rsX3 = rsX, rsW3 = rsW;
  if constexpr (UPFRONT) {
    rsX3 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(q.x3), 0, (int)q.x3_bytes, 0x00020000);
    rsW3 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(q.w3), 0, (int)q.w3_bytes, 0x00020000);
  }

  // k-steps of this wave: slice (blockIdx.y, kw) of the layer's T * Cin / 16 steps, s = tap * cpk + chunk, walked as v = 0 .. n1 - 1
  // (the second product's k-steps of a PAIR are shared out over all K slices and waves as well: t = t_begin .. t_begin + n2 - 1)
  const int cpk_sh = p.s_cpk_shift, cpk = 1 << cpk_sh;
  const int KW = a.KW, kw_magic = (256 + KW - 1) / KW;
  const int slice = (int)blockIdx.y * ksplit + kw;
  const int s_begin = slice * p.s_kper;
  const int n1 = max(0, min(p.s_ksteps, s_begin + p.s_kper) - s_begin);
  const int t_begin = PAIR ? slice * q.kper2 : 0;
  const int n2 = PAIR ? max(0, min(q.ksteps2, t_begin + q.kper2) - t_begin) : 0;
  const uint32_t x3off = PAIR ? (uint32_t)pix * (uint32_t)q.ldx3 * (uint32_t)P::BYTES + lhb : 0u;
  const bool w_split = a.w_split != 0;

  Frag xb[2][SU], wb[2][SU];
  uint32_t okm[2] = {0u, 0u};
  auto load_group = [&](int buf, int v0) {
    uint32_t m = 0;
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const int v = v0 + u;                              // (wave-uniform)
      const int s = s_begin + v;
      const bool live = v < n1;
      const int tap = s >> cpk_sh, cc = s & (cpk - 1);
      const int ty = (tap * kw_magic) >> 8, tx = tap - ty * KW;
      const bool ok = pok && live && (unsigned)(iy0 + ty) < (unsigned)a.Hin && (unsigned)(ix0 + tx) < (unsigned)a.Win;
      const uint32_t xo = (uint32_t)(pbase + ty * a.Win + tx) * ldxb + (uint32_t)(cc * (16 * P::BYTES)) + lhb;
      xb[buf][u] = P::load_x(rsX, ok, xo);
      wb[buf][u] = P::load_w(rsW, live && nok, s, wa);
      m |= ok ? (1u << u) : 0u;
    }
    okm[buf] = m;
  };
  // bf16 pairs: the second product has at most SU2 k-steps per wave (host): their fragments get registers of their own, are
  // requested with the first ones and used last -- no branch per step in the main loop
  Frag x2b[UPFRONT ? P::SU2 : 1], w2b[UPFRONT ? P::SU2 : 1];

  f32x16 acc, acc2;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f, acc2[r] = 0.f;
  float* cst = sm + SRED + wave * SCONST_PER_WAVE;       // this wave's [6][32] epilogue constants
  float* tab = sm + SRED + SCONST_FLOATS;                // [2][Cin]
  auto compute_group = [&](int buf, int v0) {
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      Frag x = xb[buf][u];
      if constexpr (AFF) {                               // BatchNorm affine of the input; zero padding applies AFTER it
        const int cc = (s_begin + v0 + u) & (cpk - 1);
        const float* sc = tab + cc * 16 + lh * 8;
        const float* sh = sc + a.Cin;
        const float4 s0v = *reinterpret_cast<const float4*>(sc), s1v = *reinterpret_cast<const float4*>(sc + 4);
        const float4 h0v = *reinterpret_cast<const float4*>(sh), h1v = *reinterpret_cast<const float4*>(sh + 4);
        P::affine(x, s0v, s1v, h0v, h1v, (okm[buf] >> u) & 1u);
      }
      P::mma(acc, wb[buf][u], x, w_split);
    }
  };

  // ---- what the epilogue needs from memory is requested FIRST (loads return in order: the LDS copies below then wait for these
  //      few loads only, the fragments behind them land meanwhile): per wave the constants of its tile's 32 columns (lane l < 32:
  //      column ni*32 + l) and, AFF, the scale / shift table of the input channels
  const bool sliced = p.splits > 1;
  const bool scat = a.scatter2x2 != 0;
  const float* asc_p = PAIR ? q.add_scale : a.add_scale;
  const float* ash_p = PAIR ? q.add_shift : a.add_shift;
  float k0 = 0.f, k1 = 1.f, k2 = 0.f, k3 = 0.f, k4 = 1.f, k5 = 0.f;
  {
    const int c = ni * 32 + li;
    const bool on = tok && c < a.Ntot && lh == 0;
    const int cco = scat ? c % p.Cout : c;
    if (on && a.bias != nullptr) k0 = a.bias[cco];
    if (on && asc_p != nullptr) k1 = asc_p[c], k2 = ash_p[c];
    if (PAIR && on && q.bias3 != nullptr) k3 = q.bias3[c];
    if (!PAIR && on && a.out_scale != nullptr) k4 = a.out_scale[cco], k5 = a.out_shift[cco];
  }
  float tsc[TABQ], tsh[TABQ];
  if constexpr (AFF) {
#pragma unroll
    for (int e = 0; e < TABQ; ++e) {
      tsc[e] = 1.f;
      tsh[e] = 0.f;
      const int c = tid + e * 64 * SWAVES;
      if (c < a.Cin) {
        tsc[e] = a.in_scale[c];
        tsh[e] = a.in_shift[c];
      }
    }
  }
  load_group(0, 0);
  if (SU < n1) load_group(1, SU);
  if constexpr (UPFRONT) {
#pragma unroll
    for (int u = 0; u < P::SU2; ++u) {
      const int t = t_begin + u;
      const bool live = u < n2;
      x2b[u] = P::load_x(rsX3, pok && live, x3off + (uint32_t)(t * (16 * P::BYTES)));
      w2b[u] = P::load_w(rsW3, live && nok, t, wa);
    }
  }
  // (which wave finishes which accumulator group -- channels ni*32 + 8 g + 4 lh + 0..3 of the lane's pixel: one wave of the tile ->
  //  all four; two -> g = kw, kw + 2; four -> g = kw; eight -> the even wave 2g finishes group g, see below)
  auto owns = [&](int g) { return ksplit == 8 ? ((kw >> 1) == g && (kw & 1) == 0) : ((g & (ksplit - 1)) == kw); };
  Out4 addv[4];
  float x3v = 0.f;
  float4 w3v[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int c = ni * 32 + 8 * g + 4 * lh;
    const bool on = !sliced && owns(g) && pok && c < a.Ntot;
    addv[g] = (!PAIR && on && a.add != nullptr) ? *P::at(a.add, (idx_t)pix, a.ldadd, c) : P::zero4();
    w3v[g] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (PAIR && q.x3_one && on) {                        // fp32 quad-packed weights of a 1-channel 1x1 window: w[n][0]
      const float* wq = reinterpret_cast<const float*>(q.w3) + (int64_t)c * 4;
      w3v[g] = make_float4(wq[0], wq[4], wq[8], wq[12]);
    }
  }
  if (PAIR && q.x3_one && pok) x3v = reinterpret_cast<const float*>(q.x3)[(int64_t)pix * q.ldx3];
  if (lh == 0) {
    cst[li] = k0;
    cst[32 + li] = k1;
    cst[64 + li] = k2;
    cst[96 + li] = k3;
    cst[128 + li] = k4;
    cst[160 + li] = k5;
  }
  if constexpr (AFF) {
#pragma unroll
    for (int e = 0; e < TABQ; ++e) {
      const int c = tid + e * 64 * SWAVES;
      if (c < a.Cin) {
        tab[c] = tsc[e];
        tab[a.Cin + c] = tsh[e];
      }
    }
    __syncthreads();
  }

  // ---- k-steps of the first product
  {
    int v0 = 0;
    while (true) {
      compute_group(0, v0);
      v0 += SU;
      if (v0 >= n1) break;
      if (v0 + SU < n1) load_group(0, v0 + SU);
      compute_group(1, v0);
      v0 += SU;
      if (v0 >= n1) break;
      if (v0 + SU < n1) load_group(1, v0 + SU);
    }
  }
  // ---- second product of a pair
  if constexpr (UPFRONT) {
#pragma unroll
    for (int u = 0; u < P::SU2; ++u) P::mma(acc2, w2b[u], x2b[u], false);
  } else if constexpr (PAIR) {
    // a second pass through the same registers (one more load round; the launch it replaces costs more)
    if (!q.x3_one) {
      rsX3 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(q.x3), 0, (int)q.x3_bytes, 0x00020000);
      rsW3 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(q.w3), 0, (int)q.w3_bytes, 0x00020000);
      const bool w3_split = q.w3_split != 0;
      for (int v0 = 0; v0 < n2; v0 += SU) {
#pragma unroll
        for (int u = 0; u < SU; ++u) {
          const int t = t_begin + v0 + u;
          const bool live = v0 + u < n2;
          xb[0][u] = P::load_x(rsX3, pok && live, x3off + (uint32_t)(t * (16 * P::BYTES)));
          wb[0][u] = P::load_w(rsW3, live && nok, t, wa);
        }
#pragma unroll
        for (int u = 0; u < SU; ++u) P::mma(acc2, wb[0][u], xb[0][u], w3_split);
      }
    }
  }

  // ---- the waves of a tile add up through LDS (fixed order), each finishing its share of the accumulator groups
  if (ksplit > 1) {
    float* mine = sm + (wave * NACC * 16) * 64 + lane;
#pragma unroll
    for (int r = 0; r < 16; ++r) mine[r * 64] = acc[r];
    if constexpr (PAIR) {
#pragma unroll
      for (int r = 0; r < 16; ++r) mine[(16 + r) * 64] = acc2[r];
    }
    __syncthreads();
  }
  auto finish_group = [&](int g, float4 v, float4 v2) {
    const int c = ni * 32 + 8 * g + 4 * lh;
    if (!pok || c >= a.Ntot) return;
    if (sliced) {                                        // raw sums of this K slice: the finish kernels do the rest
      *reinterpret_cast<float4*>(a.partial + ((int64_t)blockIdx.y * p.Mtot + pix) * a.Ntot + c) = v;
      if constexpr (PAIR) *reinterpret_cast<float4*>(a.partial + ((int64_t)(p.splits + blockIdx.y) * p.Mtot + pix) * a.Ntot + c) = v2;
      return;
    }
    const float4 cb = *reinterpret_cast<const float4*>(cst + 8 * g + 4 * lh);
    const float4 cs = *reinterpret_cast<const float4*>(cst + 32 + 8 * g + 4 * lh);
    const float4 ch = *reinterpret_cast<const float4*>(cst + 64 + 8 * g + 4 * lh);
    v.x += cb.x; v.y += cb.y; v.z += cb.z; v.w += cb.w;
    if (a.relu) {
      v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    }
    if (!PAIR && a.add != nullptr) {
      const float4 t = P::val(addv[g]);
      v.x += fmaf(t.x, cs.x, ch.x);
      v.y += fmaf(t.y, cs.y, ch.y);
      v.z += fmaf(t.z, cs.z, ch.z);
      v.w += fmaf(t.w, cs.w, ch.w);
    }
    idx_t opix = (idx_t)pix;
    int ocol = c;
    if (scat) {
      const int ab = c / p.Cout;
      ocol = c - ab * p.Cout;
      opix = ((idx_t)img * a.Hout + 2 * gy + (ab >> 1)) * a.Wout + 2 * gx + (ab & 1);
    }
    Out4* dst = P::at(a.y, opix, a.ldy, ocol);
    if (a.accumulate) {
      const float4 o = P::val(*dst);
      v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
    }
    // sv: the value as it is stored (bf16: rounded once).  The pair epilogue and the output affine work on it
    Out4 w = P::round4(v);
    const float4 sv = P::val(w);
    if (!PAIR && a.out_scale != nullptr) {               // the consumer's BatchNorm: what its affine on load computes, rounded as it would
      const float4 os = *reinterpret_cast<const float4*>(cst + 128 + 8 * g + 4 * lh);
      const float4 oh = *reinterpret_cast<const float4*>(cst + 160 + 8 * g + 4 * lh);
      w = P::round4(make_float4(fmaf(sv.x, os.x, oh.x), fmaf(sv.y, os.y, oh.y), fmaf(sv.z, os.z, oh.z), fmaf(sv.w, os.w, oh.w)));
    }
    *dst = w;
    if constexpr (PAIR) {
      // the second convolution's epilogue, as its own launch performs it: product + bias3, then + BN(y1) of the STORED y1
      const float4 c3 = *reinterpret_cast<const float4*>(cst + 96 + 8 * g + 4 * lh);
      float4 o;
      if (q.x3_one) {                                    // (direct_conv_kernel<1,1,1>: acc = bias; acc = fma(x, w, acc))
        o.x = fmaf(x3v, w3v[g].x, c3.x); o.y = fmaf(x3v, w3v[g].y, c3.y); o.z = fmaf(x3v, w3v[g].z, c3.z); o.w = fmaf(x3v, w3v[g].w, c3.w);
      } else {
        o.x = v2.x + c3.x; o.y = v2.y + c3.y; o.z = v2.z + c3.z; o.w = v2.w + c3.w;
      }
      o.x += fmaf(sv.x, cs.x, ch.x);
      o.y += fmaf(sv.y, cs.y, ch.y);
      o.z += fmaf(sv.z, cs.z, ch.z);
      o.w += fmaf(sv.w, cs.w, ch.w);
      *P::at(q.y2, (idx_t)pix, q.ldy2, c) = P::round4(o);
    }
  };
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ksplit == 1) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
      finish_group(g, make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]),
                   PAIR ? make_float4(acc2[4 * g], acc2[4 * g + 1], acc2[4 * g + 2], acc2[4 * g + 3]) : zero4);
  } else if (ksplit <= 4) {
    // wave kw of the tile's ksplit waves takes the groups g = kw, kw + ksplit, ...
    const float* base = sm + ((grp << ksh) * NACC * 16) * 64 + lane;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if ((g & (ksplit - 1)) != kw) continue;
      float v[4] = {0.f, 0.f, 0.f, 0.f}, v2[4] = {0.f, 0.f, 0.f, 0.f};
      for (int w_ = 0; w_ < ksplit; ++w_) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] += base[(w_ * NACC * 16 + 4 * g + j) * 64];
        if constexpr (PAIR) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v2[j] += base[(w_ * NACC * 16 + 16 + 4 * g + j) * 64];
        }
      }
      finish_group(g, make_float4(v[0], v[1], v[2], v[3]), make_float4(v2[0], v2[1], v2[2], v2[3]));
    }
  } else {
    // eight waves: the even ones finish one group each (g = kw / 2); the sums are formed by ALL lanes of waves 2g and 2g + 1 --
    // wave 2g adds the partial tiles 0..3, wave 2g + 1 the tiles 4..7 -- and meet in LDS once more
    const float* base = sm + lane;
    const int g = kw >> 1, half = kw & 1;
    float v[4] = {0.f, 0.f, 0.f, 0.f}, v2[4] = {0.f, 0.f, 0.f, 0.f};
    for (int w_ = 4 * half; w_ < 4 * half + 4; ++w_) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] += base[(w_ * NACC * 16 + 4 * g + j) * 64];
      if constexpr (PAIR) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v2[j] += base[(w_ * NACC * 16 + 16 + 4 * g + j) * 64];
      }
    }
    __syncthreads();                                     // every partial tile has been read
    if (half) {
#pragma unroll
      for (int j = 0; j < 4; ++j) sm[(g * 8 + j) * 64 + lane] = v[j];
      if constexpr (PAIR) {
#pragma unroll
        for (int j = 0; j < 4; ++j) sm[(g * 8 + 4 + j) * 64 + lane] = v2[j];
      }
    }
    __syncthreads();
    if (!half) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] += sm[(g * 8 + j) * 64 + lane];
      if constexpr (PAIR) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v2[j] += sm[(g * 8 + 4 + j) * 64 + lane];
      }
#pragma unroll
      for (int gg = 0; gg < 4; ++gg)                     // (static register indices: a run-time g would put per-group registers in scratch)
        if (gg == g) finish_group(gg, make_float4(v[0], v[1], v[2], v[3]), make_float4(v2[0], v2[1], v2[2], v2[3]));
    }
  }
}

// K-sliced pairs: y1 = ReLU(sum of the first product's slices + bias), y2 = sum of the second product's slices + bias3 + BN(y1) -- the pair
// epilogue of convs_kernel on the sums (a.partial: [2][splits][M][Ntot] fp32).  One thread: 4 consecutive channels of a pixel.
template <class S>
__global__ void __launch_bounds__(256) convs_pair_finish_kernel(const ConvS p, const ConvPair q) {
  typedef typename S::idx_t idx_t;
  const dfl_conv_args& a = p.a;
  const int nq = a.Ntot >> 2;
  const int idx = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (idx >= p.Mtot * nq) return;
  const int pix = idx / nq, c = (idx - pix * nq) * 4;
  const int64_t slice = (int64_t)p.Mtot * a.Ntot;
  const float* p1 = a.partial + (int64_t)pix * a.Ntot + c;
  const float* p2 = p1 + (int64_t)p.splits * slice;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f), o = v;
  for (int s = 0; s < p.splits; ++s) {
    const float4 t1 = *reinterpret_cast<const float4*>(p1 + (int64_t)s * slice), t2 = *reinterpret_cast<const float4*>(p2 + (int64_t)s * slice);
    v.x += t1.x; v.y += t1.y; v.z += t1.z; v.w += t1.w;
    o.x += t2.x; o.y += t2.y; o.z += t2.z; o.w += t2.w;
  }
  if (a.bias != nullptr) { v.x += a.bias[c]; v.y += a.bias[c + 1]; v.z += a.bias[c + 2]; v.w += a.bias[c + 3]; }
  if (a.relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
  const typename S::Out4 w = S::round4(v);
  const float4 sv = S::val(w);
  *S::at(a.y, (idx_t)pix, a.ldy, c) = w;
  if (q.bias3 != nullptr) { o.x += q.bias3[c]; o.y += q.bias3[c + 1]; o.z += q.bias3[c + 2]; o.w += q.bias3[c + 3]; }
  o.x += fmaf(sv.x, q.add_scale[c], q.add_shift[c]);
  o.y += fmaf(sv.y, q.add_scale[c + 1], q.add_shift[c + 1]);
  o.z += fmaf(sv.z, q.add_scale[c + 2], q.add_shift[c + 2]);
  o.w += fmaf(sv.w, q.add_scale[c + 3], q.add_shift[c + 3]);
  *S::at(q.y2, (idx_t)pix, q.ldy2, c) = S::round4(o);
}

// ---- host side ------------------------------------------------------------------------------------------------------

// Can these arguments take the latency form?  The caller has validated them -- convp_validate of conv_plan.hip for bf16 tensors,
// conv_prepare of conv_gemm.hip for fp32 tensors -- and filled the layer constants of p (a, gather grid, Mtot, Cout, T, extents).
bool convs_eligible(const dfl_conv_args& a, const ConvP& p) {
  if (!a.latency_form || !convs_enabled()) return false;
  if (a.x_mode != 0 || a.x_out != nullptr || a.stat_partials != nullptr || a.stat_totals != nullptr || a.stat_other != nullptr) return false;
  if (a.in_tot != nullptr || a.add_tot != nullptr) return false;
  if (a.out_scale != nullptr && a.accumulate) return false;
  const int cpk = a.Cin / 16;
  if (cpk < 1 || (cpk & (cpk - 1)) != 0 || a.Cin > 1024) return false;
  if (a.Ntot % 8 != 0 || p.Mtot > (1 << 16)) return false;
  if (p.Cout % 4 != 0) return false;
  // a latency problem, not a throughput problem: the largest layer of a 192x192 image is 1.4 GFLOP (operands are not reused
  // across tiles here: beyond this the patch-resident kernels win)
  if (2.0 * p.Mtot * a.Ntot * (double)(p.T * a.Cin) > 1.5e9) return false;
  // (round 5, measured with tools/kbench_infer.py 192 1 and docs/experiments/infer192_r05: with 8 k-steps per register set and the
  //  BatchNorm affine on load the 3x3 layers of the two widest levels were 2 - 3 us slower in this form; with 9 k-steps and the affine
  //  moved into the producer every layer of a 192x192 forward is faster here: 0.335 -> 0.320 ms without an exception)
  if (a.x_bf16) return a.KW <= 16;                     // (alignment, strides and the weight packing: convp_validate)
  // fp32 tensors: what conv_prepare does not ask of every block
  const int mm = math_mode();
  if (a.y_bf16 || (mm != 0 && mm != 1) || a.x_split || p.T > 16) return false;
  if ((a.out_scale == nullptr) != (a.out_shift == nullptr)) return false;
  if (a.w_split != 0 && !(a.w_split == 1 && mm == 1)) return false;
  if (a.Cin % 16 != 0 || a.ldx % 4 != 0 || !aligned16(a.x) || a.ldy % 4 != 0 || !aligned16(a.y)) return false;
  if (a.add != nullptr && (a.ldadd % 4 != 0 || !aligned16(a.add))) return false;
  return p.x_bytes != 0 && p.w_bytes != 0;             // (conv_prepare leaves 0 where a tensor reaches 2 GiB)
}

static int convs_waves(int ksplit_shift) { return ksplit_shift == 3 ? 8 : 4; }      // (always eight waves: 0.320 instead of 0.3125 ms per forward)
static size_t convs_lds(int waves, int nacc, int Cin) { return (size_t)(waves * nacc * 16 * 64 + waves * SCONST_PER_WAVE + 2 * Cin) * 4; }

// Work split: 32 x 32 tiles, `ksplit` waves of a workgroup per tile, `splits` K slices over workgroups.  Aim: about one wave
// per SIMD-slot pair of the chip (2048 waves) and at least `least` k-steps per wave; cross-workgroup slices only when the eight
// waves of a workgroup would be left with more than two register sets of `su` k-steps each.
static void work_split(const dfl_conv_args& a, ConvP* p, int force_splits, int su, int least) {
  p->s_mt = (int)ceil_div(p->Mtot, 32);
  p->s_nt = (int)ceil_div(a.Ntot, 32);
  const int cpk = a.Cin / 16;
  int sh = 0;
  while ((1 << sh) < cpk) ++sh;
  p->s_cpk_shift = sh;
  p->s_ksteps = p->T * cpk;
  const int tiles = p->s_mt * p->s_nt;
  int want = 2048 / tiles;
  if (want > p->s_ksteps / least) want = p->s_ksteps / least;
  if (want < 1) want = 1;
  // K slices over workgroups cost a finish launch (4.7 us)
  int zs = 1;
  if (force_splits > 0) zs = force_splits;
  else if (want > 8 && p->s_ksteps > 8 * 2 * su) zs = want / 8;
  if (zs > 16) zs = 16;
  if (zs > p->s_ksteps) zs = p->s_ksteps;
  int per = want / zs;
  int ksh = 0;
  while (ksh < 3 && (2 << ksh) <= per) ++ksh;
  p->s_ksplit_shift = ksh;
  p->s_kper = (int)ceil_div(p->s_ksteps, (int64_t)zs << ksh);
  if (force_splits <= 0) zs = (int)ceil_div(p->s_ksteps, (int64_t)p->s_kper << ksh);      // (no empty slices when the choice is free)
  p->splits = zs;
  p->tile = CONVS_TILE;
  const int W = convs_waves(ksh);
  p->grid = (int)ceil_div(tiles, W >> ksh);
  p->lds_bytes = (int)convs_lds(W, 1, a.Cin);
}

void convs_plan(const dfl_conv_args& a, ConvP* p, int force_splits) {
  if (a.x_bf16) work_split(a, p, force_splits, ElemBF16::SU, 6);
  else work_split(a, p, force_splits, ElemF32<0>::SU, 4);
}

// The convolution (and, PAIR, the K-slice finish of a pair) in element form P
template <class P, bool PAIR>
static int convs_launch_t(const ConvP& p, const ConvPair& q, hipStream_t s) {
  const char* what = PAIR ? P::PAIR_WHAT : P::WHAT;
  const ConvS k_args = convs_args(p);
  dim3 grid((unsigned)p.grid, (unsigned)p.splits);
  const int W = convs_waves(p.s_ksplit_shift);
  const size_t lds = convs_lds(W, PAIR ? 2 : 1, p.a.Cin);
  const bool aff = p.a.in_scale != nullptr;
#define DFL_CONVS_LAUNCH(AFF_, W_)                                                                                       \
  {                                                                                                               \
    auto k = convs_kernel<P, AFF_, PAIR, W_>;                                                                     \
    if (lds > 64 * 1024) DFL_LDS_OPT_IN(k, 96 * 1024, what)                                                       \
    hipLaunchKernelGGL(k, grid, dim3(64 * W_), lds, s, k_args, q);                                                    \
  }
  if constexpr (PAIR && !P::PAIR_AFF) {                   // (pair_ok refuses an affine on load)
    if (W == 8) DFL_CONVS_LAUNCH(false, 8) else DFL_CONVS_LAUNCH(false, 4)
  } else if (aff) {
    if (W == 8) DFL_CONVS_LAUNCH(true, 8) else DFL_CONVS_LAUNCH(true, 4)
  } else {
    if (W == 8) DFL_CONVS_LAUNCH(false, 8) else DFL_CONVS_LAUNCH(false, 4)
  }
#undef DFL_CONVS_LAUNCH
  if (PAIR && p.splits > 1) {
    const int rc = check_launch(what);
    if (rc != DFL_OK) return rc;
    hipLaunchKernelGGL(convs_pair_finish_kernel<typename P::Store>, dim3((unsigned)ceil_div((int64_t)p.Mtot * (p.a.Ntot / 4), 256)), dim3(256), 0, s, k_args, q);
  }
  return check_launch(what);
}

template <bool PAIR>
static int convs_launch_form(const ConvP& p, const ConvPair& q, hipStream_t s) {
  if (p.a.x_bf16) return convs_launch_t<ElemBF16, PAIR>(p, q, s);
  return math_mode() == 0 ? convs_launch_t<ElemF32<0>, PAIR>(p, q, s) : convs_launch_t<ElemF32<1>, PAIR>(p, q, s);
}

// K slices of an fp32 block are left to the caller's conv_finish (conv_gemm.hip), those of a bf16 block to convp_launch
int convs_launch(const ConvPlan& pl, hipStream_t s) {
  ConvPair none;
  memset(&none, 0, sizeof(none));
  return convs_launch_form<false>(pl.p, none, s);
}

// ---- pairs (dfl_conv2d_pair): conditions under which (a, b) run as one launch; pa = a's plan in latency form
static bool pair_ok(const dfl_conv_args* a, const dfl_conv_args* b, const ConvP& pa) {
  const bool bf = a->x_bf16 != 0;
  const int bytes = bf ? ElemBF16::BYTES : ElemF32<0>::BYTES;
  const bool one = bf ? !b->x_bf16 : b->Cin == 1;        // the network's first block: b reads the 1-channel fp32 image
  if (pa.tile != CONVS_TILE) return false;
  if (pa.splits > 1 && (one || a->partial == nullptr)) return false;
  if (a->scatter2x2 || a->accumulate || a->add != nullptr || a->out_scale != nullptr) return false;
  if (!b->latency_form || b->KH != 1 || b->KW != 1 || b->stride != 1 || b->pad != 0 || b->scatter2x2 || b->accumulate || b->relu) return false;
  if (b->in_scale != nullptr || b->in_tot != nullptr || b->add_tot != nullptr || b->x_mode != 0 || b->x_out != nullptr || b->out_scale != nullptr) return false;
  if (b->stat_partials != nullptr || b->stat_totals != nullptr || b->stat_other != nullptr || b->splits > 1) return false;
  if (b->add != a->y || b->ldadd != a->ldy || b->add_scale == nullptr || b->add_shift == nullptr) return false;
  if (b->N != a->N || b->Hout != a->Hout || b->Wout != a->Wout || b->Hin != a->Hout || b->Win != a->Wout || b->Ntot != a->Ntot) return false;
  if (b->y == a->y || b->y == nullptr || b->ldy % 4 != 0 || b->x == nullptr || b->w == nullptr) return false;
  if (bf) {
    // the second product's fragments have registers of their own; no pair instantiation with an affine on load
    if (a->in_scale != nullptr || !b->y_bf16) return false;
    if (!one && ceil_div(b->Cin / 16, (int64_t)pa.splits << pa.s_ksplit_shift) > ElemBF16::SU2) return false;
    if (one) return b->Cin == 1 && b->w_split == 0 && b->x_split == 0;
    if (b->w_split != 2) return false;
  } else {
    if (b->x_bf16 || b->y_bf16 || b->x_split || !aligned16(b->y)) return false;
    if (one) return b->w_split == 0;
    if (b->w_split != 0 && !(b->w_split == 1 && math_mode() == 1)) return false;
  }
  if (b->Cin % 16 != 0 || b->ldx % (16 / bytes) != 0 || !aligned16(b->x) || !aligned16(b->w)) return false;
  const int64_t xb = (((int64_t)b->N * b->Hin * b->Win - 1) * b->ldx + b->Cin) * bytes, wb = (int64_t)b->Cin * b->Ntot * bytes;
  return xb < (1ll << 31) - 4096 && wb < (1ll << 31) - 4096;
}

int convs_pair_ok(const dfl_conv_args* a, const dfl_conv_args* b, const ConvP& pa) {
  if (!pair_ok(a, b, pa)) return 0;
  return pa.splits > 1 ? 2 : 1;            // 2: K slices -- a->partial holds [2][splits][M][Ntot] floats
}

// a then b as ONE launch (the caller has checked convs_pair_ok; p = a's plan)
int convs_pair_launch(const ConvP& p, const dfl_conv_args* b, hipStream_t s) {
  const int bytes = p.a.x_bf16 ? ElemBF16::BYTES : ElemF32<0>::BYTES;
  ConvPair q;
  memset(&q, 0, sizeof(q));
  q.x3 = b->x;
  q.w3 = b->w;
  q.bias3 = b->bias;
  q.add_scale = b->add_scale;
  q.add_shift = b->add_shift;
  q.y2 = b->y;
  q.ldx3 = b->ldx;
  q.ldy2 = b->ldy;
  q.x3_one = b->Cin == 1 ? 1 : 0;
  q.w3_split = b->w_split;
  if (!q.x3_one) {
    q.ksteps2 = b->Cin / 16;
    q.kper2 = (int)ceil_div(q.ksteps2, (int64_t)p.splits << p.s_ksplit_shift);
    q.x3_bytes = (uint32_t)((((int64_t)b->N * b->Hin * b->Win - 1) * b->ldx + b->Cin) * bytes);
    q.w3_bytes = (uint32_t)((int64_t)b->Cin * b->Ntot * bytes);
  }
  return convs_launch_form<true>(p, q, s);
}

// ---- the network's first convolution in the same spirit (1-channel fp32 image, 3x3 window, stride 1: unet.py:211 with in_channels = 1):
// direct_conv3_rows_kernel walks bands of rows, three per workgroup -- 32 workgroups for one 192x192 image, 13 us.  Here a thread owns
// one pixel and 8 channels (a wave: 64 consecutive pixels of one channel group): 9 loads of the image, the 9 x 8 weights from LDS,
// the multiply-adds in direct_conv3_rows_kernel's order (bit-identical results), one 16-byte store.
template <bool BF>
__global__ void __launch_bounds__(256) convs_first_kernel(const dfl_conv_args a, int M) {
  __shared__ __attribute__((aligned(16))) float wl[9 * 64 + 3 * 64];          // [9][Ntot] weights, bias, out_scale, out_shift
  const int ncg = a.Ntot >> 3;                            // channel groups of 8
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wpb = 4;                                      // waves per block
  const int gw = (int)blockIdx.x * wpb + wave;            // global wave: (pixel block of 64, channel group)
  const int cg = gw % ncg, pb = gw / ncg;
  const int pix = pb * 64 + lane;
  const bool pok = pix < M;
  const int HW = a.Hout * a.Wout;
  const int img = pix / HW, rem = pix - img * HW;
  const int oy = rem / a.Wout, ox = rem - oy * a.Wout;
  float xv[9];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int iy = oy - a.pad + dy, ix = ox - a.pad + dx;
      const bool ok = pok && (unsigned)iy < (unsigned)a.Hin && (unsigned)ix < (unsigned)a.Win;
      xv[dy * 3 + dx] = ok ? a.x[((int64_t)(img * a.Hin + iy) * a.Win + ix) * a.ldx] : 0.f;
    }
  const int Nt = a.Ntot;
  for (int i = threadIdx.x; i < 9 * Nt; i += 256) {
    const int k = i / Nt, nn = i - k * Nt;
    wl[i] = a.w[((int64_t)(k >> 2) * Nt + nn) * 4 + (k & 3)];                 // quad-packed operand
  }
  for (int i = threadIdx.x; i < Nt; i += 256) {
    wl[9 * Nt + i] = a.bias != nullptr ? a.bias[i] : 0.f;
    wl[10 * Nt + i] = a.out_scale != nullptr ? a.out_scale[i] : 1.f;
    wl[11 * Nt + i] = a.out_scale != nullptr ? a.out_shift[i] : 0.f;
  }
  __syncthreads();
  const int n0 = cg * 8;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = wl[9 * Nt + n0 + j];
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = fmaf(xv[k], wl[k * Nt + n0 + j], acc[j]);
  if (a.relu) {
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = fmaxf(acc[j], 0.f);
  }
  if constexpr (!BF) {                                    // fp32 tensors: nothing is rounded, the output affine is the consumer's fma
    if (a.out_scale != nullptr) {
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = fmaf(acc[j], wl[10 * Nt + n0 + j], wl[11 * Nt + n0 + j]);
    }
    if (pok) {
      float* dst = a.y + ((int64_t)pix * a.ldy + n0);
      *reinterpret_cast<float4*>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
      *reinterpret_cast<float4*>(dst + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
    }
    return;
  }
  u32x4 w;
  w.x = pack_bf2(acc[0], acc[1]);
  w.y = pack_bf2(acc[2], acc[3]);
  w.z = pack_bf2(acc[4], acc[5]);
  w.w = pack_bf2(acc[6], acc[7]);
  if (a.out_scale != nullptr) {
    const float* os = wl + 10 * Nt + n0;
    const float* oh = wl + 11 * Nt + n0;
    const u32x4 t = w;
    w.x = pack_bf2(fmaf(bf_lo(t.x), os[0], oh[0]), fmaf(bf_hi(t.x), os[1], oh[1]));
    w.y = pack_bf2(fmaf(bf_lo(t.y), os[2], oh[2]), fmaf(bf_hi(t.y), os[3], oh[3]));
    w.z = pack_bf2(fmaf(bf_lo(t.z), os[4], oh[4]), fmaf(bf_hi(t.z), os[5], oh[5]));
    w.w = pack_bf2(fmaf(bf_lo(t.w), os[6], oh[6]), fmaf(bf_hi(t.w), os[7], oh[7]));
  }
  if (pok) *reinterpret_cast<u32x4*>(reinterpret_cast<unsigned short*>(a.y) + ((int64_t)pix * a.ldy + n0)) = w;
}

bool convs_first_ok(const dfl_conv_args* a) {
  if (!a->latency_form || !convs_enabled()) return false;
  if (a->x_bf16 || a->Cin != 1 || a->KH != 3 || a->KW != 3 || a->stride != 1 || a->w_split != 0 || a->x_split != 0) return false;
  if (a->Ntot % 8 != 0 || a->Ntot > 64 || a->ldy % 8 != 0 || !aligned16(a->y)) return false;
  if (a->add != nullptr || a->accumulate || a->scatter2x2 || a->splits > 1 || a->in_scale != nullptr || a->in_tot != nullptr) return false;
  if (a->stat_partials != nullptr || a->stat_totals != nullptr || a->stat_other != nullptr || a->x_mode != 0) return false;
  const int ho = a->Hin + 2 * a->pad - 2, wo = a->Win + 2 * a->pad - 2;
  if (ho != a->Hout || wo != a->Wout) return false;
  return (int64_t)a->N * a->Hout * a->Wout <= (1 << 16);
}

int convs_first_launch(const dfl_conv_args* a, hipStream_t s) {
  const int M = a->N * a->Hout * a->Wout;
  const int waves = (int)ceil_div(M, 64) * (a->Ntot / 8);
  if (a->y_bf16) hipLaunchKernelGGL(convs_first_kernel<true>, dim3((unsigned)ceil_div(waves, 4)), dim3(256), 0, s, *a, M);
  else hipLaunchKernelGGL(convs_first_kernel<false>, dim3((unsigned)ceil_div(waves, 4)), dim3(256), 0, s, *a, M);
  return check_launch("dfl_conv2d (first layer, latency form)");
}

}  // namespace dfl
