// Patch-resident convolution for bf16 tensors (math mode 4, "bf16 storage": BASELINE configs[1] as named -- bf16
// activations and weights in HBM, fp32 accumulation / statistics / master weights).
//
// Serves what conv_gemm.hip / conv_rows.hip serve for fp32 tensors -- nn.Conv2d 3x3 / 1x1 / 2x2-stride-2,
// nn.ConvTranspose2d(k2,s2) (scatter epilogue) and, with re-packed weights, every data gradient (reference:
// train_test_code/unet.py:93,207,211,218,240; torch autograd at train.py:422) -- with a different decomposition, built
// around what bf16 changes: the matrix pipe is 16x faster than for fp32 products, so the loop must not touch LDS or the
// vector-load return path once per tap.
//
//   * A workgroup owns a PATCH of output pixels (PH x PW pixels of IPP images, WM*TM*32 GEMM rows) and BN = WN*TN*32 output
//     columns.  The input pixels the patch needs for ALL taps -- the patch with its halo -- are staged in LDS ONCE per
//     block of CK input channels (BatchNorm affine applied there, zero padding written as zeros), [pixel][CK] bf16 with a
//     pixel pitch of 2*CK + 16 bytes.  Every tap then is an address offset: lane l of a 32-row tile reads its pixel's 16
//     bytes (8 channels) with one ds_read_b128 at base(l) + tap offset + chunk offset.  The pitch (odd multiple of 16
//     bytes) spreads the 16 pixels of a b128 lane group over all 64 banks: no conflicts for consecutive pixels.  The loop
//     has NO barrier (the image is static while it runs) and no per-tap gather, masks or bounds logic at all.
//   * Weights never touch LDS: they are packed [k/16][n][16 k] bf16 (dfl_pack_job.split = 2), so the MFMA B fragment of a
//     wave -- 32 columns x 16 k -- is one fully coalesced 1 KiB buffer load straight into registers.  Waves of a
//     workgroup that share output columns re-read those lines from L1/L2; waves split the N dimension first (WN), so this
//     happens only for the 32/64-channel layers whose whole weight tensor is 18-147 KiB.  Fragments are prefetched two
//     groups of four k-steps ahead (a ring of three register sets).
//   * v_mfma_f32_32x32x16_bf16, fp32 accumulators, TM x TN tiles per wave.
//   * Epilogue as dfl_conv2d defines it (bias, ReLU, + BN(other), accumulate, NHWC / 2x2-scatter store, per-channel
//     statistics); values are rounded to bf16 once, the statistics are taken from the ROUNDED values (what consumers
//     normalise).  K slices (blockIdx.z = ranges of channel blocks) leave fp32 partial sums for convp_finish_kernel.
//
// Geometry (patch shape, resident channels, K slices, tile configuration) is chosen on the host per layer
// (convp_plan, conv_plan.hip): candidates are scored by matrix work x rounds over the 256 CUs, including the fill of the last tiles.
#include "common.h"
#include "conv_ep_bf16.h"
#include "convp.h"

namespace dfl {

#ifndef DFL_BRB_U
#define DFL_BRB_U 4
#endif

__device__ __forceinline__ float round_bf(float v) { return (float)(__bf16)v; }
// q / d for the small row indices of a patch (q < 65536, d < 65536): one multiply-high with m = ceil(2^32 / d) from the host
// (the epilogue decodes a patch row into (image, y, x) for every row it stores: two 35-instruction divisions each before)
__device__ __forceinline__ int pdiv(int q, uint32_t m, int d) { return d == 1 ? q : (int)__umulhi((uint32_t)q, m); }
__device__ __forceinline__ float ld_bf(const __bf16* p) { return (float)*p; }

// KS = 2 ("two k-groups"): 512 threads -- the same 4-wave tile layout twice.  Both groups share the staged patch image and
// take alternate ring groups of k-steps; their accumulators meet in LDS before the epilogue.  Two waves per SIMD instead of
// one cover each other's fragment-read and weight-load latencies in the k loop (a batch-16 layer of the deep levels has one
// workgroup per CU, i.e. ONE wave per SIMD: its k loop runs at 35-41 % of the matrix rate), the patch is staged by twice
// the threads, and -- unlike more K slices -- no partial sums go through HBM.
// AFF: what happens to an input unit on its way into the LDS image -- 0: nothing; 1: BatchNorm affine (scale, shift); 2: BatchNorm +
// ReLU backward (dfl_conv_args.x_mode): x is dy, x2 the saved ReLU output r, the staged value [r > 0] * (A dy + B r + C).
#ifndef DFL_CONVP_G1
#define DFL_CONVP_G1 4
#endif
#ifndef DFL_CONVP_MINW3
#define DFL_CONVP_MINW3 2
#endif
template <int WM, int WN, int TM, int TN, int AFF, bool GA, int KS = 1>
__global__ void __launch_bounds__(256 * KS, (TM * TN >= 6 || KS == 2) ? 1 : (TM * TN <= 3 ? DFL_CONVP_MINW3 : 2)) convp_kernel(const ConvP p) {
  static_assert(WM * WN == 4, "four waves per k-group");
  static_assert(KS == 1 || (KS == 2 && !GA), "two k-groups: LDS-image form only");
  static_assert(AFF != 2 || !GA, "the fused BatchNorm + ReLU backward operand is staged through LDS");
  constexpr int NT = 256 * KS;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const dfl_conv_args& a = p.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = (tid >> 6) & 3;
  // k-group of this wave: a compile-time 0 for one group, wave-uniform (scalar register) for two -- the k loop's cursors and
  // liveness tests must stay scalar
  const int kg = KS == 1 ? 0 : __builtin_amdgcn_readfirstlane(tid >> 8);
  const int wm = wave / WN, wn = wave % WN, li = lane & 31, lh = lane >> 5;
  const int S = p.pix_stride;
  const int PP = p.PH * p.PW;

  // ---- which patch, column tile and K slice.  The grid is linear; workgroup b runs on XCD b % 8 (observed, used for
  //      speed only).  Layers whose weights outweigh their activations (deep levels: 5-19 MB of weights against a 4 MB
  //      L2 per XCD) put all patches of one (column tile, K slice) pair on ONE XCD, so that every XCD streams only its
  //      share of the weights instead of all of them; the others keep patches adjacent (activation reuse in L2).
  int bpatch, btile, bslice;
  {
    const int b = blockIdx.x;
    if (p.xcd_mode == 0) {
      bpatch = b % p.npatch;
      const int r = b / p.npatch;
      btile = r % p.ntiles;
      bslice = r / p.ntiles;
    } else {
      const int x = b & 7, r = b >> 3;
      int s;
      if (p.xcd_mode == 1) {                        // pairs round-robin over the XCDs
        s = x + 8 * (r / p.npatch);
        bpatch = r % p.npatch;
      } else {                                      // fewer pairs than XCDs: 8 / pairs XCDs share one pair's patches
        const int pairs = p.ntiles * p.splits;
        s = x % pairs;
        bpatch = x / pairs + (8 / pairs) * r;
      }
      if (s >= p.ntiles * p.splits || bpatch >= p.npatch) return;
      btile = s % p.ntiles;
      bslice = s / p.ntiles;
    }
  }
  const int per_img = p.npy * p.npx;
  const int pg = bpatch / per_img, pr = bpatch - pg * per_img;
  const int ppy = pr / p.npx, ppx = pr - ppy * p.npx;
  const int img0 = pg * p.IPP, gy0 = ppy * p.PH, gx0 = ppx * p.PW;
  const int n0 = btile * (WN * TN * 32);

  // ---- LDS base of each tile row of this lane (tap (0,0), channel chunk 0, this lane's k half)
  uint32_t a_base[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    int q = (wm * TM + i) * 32 + li;
    int img = pdiv(q, p.mPP, PP);
    int r = q - img * PP;
    int py = pdiv(r, p.mPW, p.PW), px = r - py * p.PW;
    if (img >= p.IPP) img = 0, py = 0, px = 0;   // padding rows of the last tile: any valid address, results are dropped
    a_base[i] = (uint32_t)(((img * p.IH + py * a.stride) * p.IW + px * a.stride) * S + lh * 16);
  }

  __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, (int)p.x_bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, (int)p.w_bytes, 0x00020000);
  uint32_t b_voff[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = n0 + (wn * TN + j) * 32 + li;
    b_voff[j] = n < a.Ntot ? (uint32_t)(n * 32 + lh * 16) : OOB;
  }

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // ---- "live" BatchNorm statistics (dfl_conv_args.in_tot / add_tot): scale / shift are derived here, one channel per thread,
  //      into two small LDS tables behind everything else the kernel keeps in LDS ([2][128] for the input channels of the
  //      resident block, [2][BN] for the epilogue's "+ BN(add)")
  float* in_tab = reinterpret_cast<float*>(smem + p.tab_off);
  float* add_tab = in_tab + 384;                      // (in_tab: [3][128] -- scale, shift, or the three backward coefficients)
  // The epilogue's per-column constants -- bias, scale and shift of "+ BN(add)" (given, or derived from the live totals) -- go into
  // the table [3][BN] HERE, at kernel start (round 6).  They used to be fetched from global memory in front of the row loop, where the
  // whole workgroup then waited one memory round trip for them: 1.4-2 us of every launch by the phase clocks of convq_bf16.hip,
  // whose epilogue is this one -- exposed wherever a layer has one workgroup per CU.
  {
    constexpr int BN0 = WN * TN * 32;
    const bool scat0 = a.scatter2x2 != 0;
    for (int col = tid; col < BN0; col += NT) {
      const int n = n0 + col;
      float sc_, sh_, b_;
      ep_col_consts(a, n, scat0 ? n % p.Cout : n, n < a.Ntot, true, &b_, &sc_, &sh_);
      add_tab[col] = sc_;
      add_tab[BN0 + col] = sh_;
      add_tab[2 * BN0 + col] = b_;
    }
  }

  // ---- staging geometry: 16-byte units (8 channels) of the patch image, `upp` per pixel; a thread keeps its channel
  //      group, its pixel advances by 256 / upp per pass
  const int upp = p.CK >> 3, upp_sh = p.upp_shift;
  const int cg = tid & (upp - 1);
  const int dpix = NT >> upp_sh;
  const int dpix_y = dpix / p.IW, dpix_x = dpix - dpix_y * p.IW;
  const int npix = p.IPP * p.IH * p.IW;
  const int CKC = p.CK >> 4;                       // 16-channel chunks per resident block (a power of two)
  const int ckc_sh = p.upp_shift - 1;
  const int S_steps = p.T * CKC;                   // k-steps per block
  const int cin_chunks = a.Cin >> 4;
  const int KW = a.KW;
  // tap / KW without a division: (tap * ceil(256 / KW)) >> 8 is exact for tap < 16 (at most 16 taps), KW <= 16.  The k loop asks for
  // it once per k-step; the scalar division the compiler emits for it (22 dependent scalar instructions) sat in the chain
  // cursor -> LDS address -> fragment read -> matrix instruction and made that chain longer than the three matrix instructions
  // of a k-step (rocprofv3: 15-18 scalar instructions per matrix instruction in these kernels).
  const int kw_magic = (256 + KW - 1) / KW;

#ifdef DFL_CONVP_TRACE   // diagnosis build (docs/experiments/convp_trace.py): shader-clock stamps of wave 0 at the phase boundaries
  long long tr_t[10];
  tr_t[6] = tr_t[7] = tr_t[8] = 0;
  tr_t[0] = __builtin_amdgcn_s_memtime();
  tr_t[5] = __builtin_amdgcn_s_memrealtime();
  tr_t[1] = tr_t[2] = 0;
#define TR(i) tr_t[i] = __builtin_amdgcn_s_memtime();
#define TRACC(i, t0) tr_t[i] += __builtin_amdgcn_s_memtime() - (t0);
#else
#define TR(i)
#define TRACC(i, t0)
#endif
  if constexpr (GA) {
    // ---- Windows that do not overlap (1x1 / stride 1, 2x2 / stride 2; no padding, no affine on load), "global A": every
    //      input pixel belongs to ONE GEMM row, so there is nothing to share through LDS and the A fragment of a lane -- 8
    //      channels of one pixel of its row's window -- is one 16-byte load straight from the tensor, like the B fragment.  No LDS image, no staging round trip before the first matrix instruction, no barrier before the
    //      epilogue; a wave keeps two groups of k-steps (A and B) in flight.  These layers are HBM streams (K = Cin is
    //      2 ... 64 k-steps): what they need is bytes in flight, not the patch reuse the LDS image exists for.
    uint32_t a_goff[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int q = (wm * TM + i) * 32 + li;
      const int img = pdiv(q, p.mPP, PP);
      const int r = q - img * PP;
      const int py = pdiv(r, p.mPW, p.PW), px = r - py * p.PW;
      const int n = img0 + img, gy = gy0 + py, gx = gx0 + px;
      const bool ok = img < p.IPP && n < a.N && gy < p.Hg && gx < p.Wg;
      a_goff[i] = ok ? (uint32_t)(((n * a.Hin + gy * a.stride) * a.Win + gx * a.stride) * a.ldx) * 2u + (uint32_t)lh * 16u : OOB;
    }
    constexpr int GG = 2;
    const int chunks = a.Cin >> 4;
    const int steps = p.T * chunks;                    // k = tap * Cin + c, as the weights are packed
    const int ngr = (steps + GG - 1) / GG;
    u32x4 areg[3][GG][TM], bqreg[3][GG][TN];
    int ls = 0, lcc = 0, ltx = 0;
    uint32_t lao = 0;                                  // byte offset of (tap, chunk) from the window's first pixel
    const uint32_t bstep = (uint32_t)a.Ntot * 32u;
    const uint32_t pixb = (uint32_t)a.ldx * 2u;
    const uint32_t tap_x = pixb - (uint32_t)chunks * 32u, tap_y = (uint32_t)(a.Win - a.KW) * pixb;
    auto load_gr = [&](int set) {
#pragma unroll
      for (int e = 0; e < GG; ++e) {
        const bool live = ls < steps;
        const uint32_t ao = live ? lao : 0u, bo = live ? (uint32_t)ls * bstep : 0u;
#pragma unroll
        for (int i = 0; i < TM; ++i) areg[set][e][i] = __builtin_amdgcn_raw_buffer_load_b128(rsX, live ? a_goff[i] : OOB, ao, 0);
#pragma unroll
        for (int j = 0; j < TN; ++j) bqreg[set][e][j] = __builtin_amdgcn_raw_buffer_load_b128(rsW, live ? b_voff[j] : OOB, bo, 0);
        ++ls;
        lao += 32u;
        if (++lcc == chunks) {
          lcc = 0;
          lao += tap_x;
          if (++ltx == a.KW) {
            ltx = 0;
            lao += tap_y;
          }
        }
      }
    };
    auto compute_gr = [&](int set) {
#pragma unroll
      for (int e = 0; e < GG; ++e)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const bf16x8_t bf = __builtin_bit_cast(bf16x8_t, bqreg[set][e][j]);
#pragma unroll
          for (int i = 0; i < TM; ++i)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, areg[set][e][i]), bf, acc[i][j], 0, 0, 0);
        }
    };
    load_gr(0);
    load_gr(1);
    for (int g = 0; g < ngr; g += 3) {
      load_gr(2);
      compute_gr(0);
      if (g + 1 < ngr) {
        load_gr(0);
        compute_gr(1);
      }
      if (g + 2 < ngr) {
        load_gr(1);
        compute_gr(2);
      }
    }
  } else {
  // B fragments ride a ring of three register sets, loaded two groups (2 G k-steps) ahead of their use.
  constexpr int G = TN == 1 ? DFL_CONVP_G1 : 2;    // k-steps per ring set (the ring holds 3 * G * TN fragments)
  const int ngroups_all = (S_steps + G - 1) / G;
  // k-group kg takes the ring groups kg, kg + KS, ...: local group gl is global group gl * KS + kg
  const int ngroups = (ngroups_all - kg + KS - 1) / KS;
  u32x4 breg[3][G][TN];
  auto load_group = [&](int blk, int gl, int set) {
    const int g = gl * KS + kg;
#pragma unroll
    for (int e = 0; e < G; ++e) {
      const int s = g * G + e;
      const bool live = gl < ngroups && s < S_steps;
      const int tap = s >> ckc_sh, cc = s & (CKC - 1);
      const uint32_t soff = live ? (uint32_t)((tap * cin_chunks + blk * CKC + cc)) * (uint32_t)a.Ntot * 32u : 0u;
#pragma unroll
      for (int j = 0; j < TN; ++j) breg[set][e][j] = __builtin_amdgcn_raw_buffer_load_b128(rsW, live ? b_voff[j] : OOB, soff, 0);
    }
  };
  const int blk_begin = bslice * p.blk_per_slice;
  const int blk_end = min(blk_begin + p.blk_per_slice, p.nblk);
  for (int blk = blk_begin; blk < blk_end; ++blk) {
    const int c0 = blk * p.CK;
    // ================================================================ stage the patch image of channels [c0, c0 + CK)
    if (blk != blk_begin) __syncthreads();         // every wave is done reading the previous image
#ifdef DFL_CONVP_TRACE
    const long long tb0 = __builtin_amdgcn_s_memtime();
#endif
    {
      float sc[8], sh[8], sq[8];
      if constexpr (AFF == 1) {
        if (a.in_tot != nullptr) {                   // live statistics: this block's channels, one per thread, through LDS
          if (tid < p.CK) bn_live_affine(a.in_tot, a.in_gamma, a.in_beta, a.in_count, a.bn_eps, a.Cin, c0 + tid, in_tab + tid, in_tab + 128 + tid);
          __syncthreads();
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            sc[e] = in_tab[cg * 8 + e];
            sh[e] = in_tab[128 + cg * 8 + e];
          }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            sc[e] = a.in_scale[c0 + cg * 8 + e];
            sh[e] = a.in_shift[c0 + cg * 8 + e];
          }
        }
      }
      __amdgpu_buffer_rsrc_t rsR = rsX, rsO = rsX;
      bool store_on = false;                       // x_out: this workgroup writes the interior of its patch (column tile 0 only)
      if constexpr (AFF == 2) {                    // d(pre-activation) = [r > 0] * (sc dy + sh r + sq); no BatchNorm: 1, 0, 0
        rsR = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x2), 0, (int)p.x2_bytes, 0x00020000);
        store_on = a.x_out != nullptr && btile == 0;
        if (store_on) rsO = __builtin_amdgcn_make_buffer_rsrc(a.x_out, 0, (int)p.xo_bytes, 0x00020000);
        if (a.in_tot != nullptr) {                   // live statistics: A, B, C of this block's channels, one per thread, through LDS
          if (tid < p.CK)
            bn_live_coef(a.in_tot, a.in_gamma, a.in_mean, a.in_invstd, a.in_count, a.Cin, c0 + tid, in_tab + tid, in_tab + 128 + tid, in_tab + 256 + tid);
          __syncthreads();
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            sc[e] = in_tab[cg * 8 + e];
            sh[e] = in_tab[128 + cg * 8 + e];
            sq[e] = in_tab[256 + cg * 8 + e];
          }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int c = c0 + cg * 8 + e;
            sc[e] = a.in_scale != nullptr ? a.in_scale[c] : 1.f;
            sh[e] = a.in_scale != nullptr ? a.in_scale[a.Cin + c] : 0.f;
            sq[e] = a.in_scale != nullptr ? a.in_scale[2 * a.Cin + c] : 0.f;
          }
        }
      }
      int pix = tid >> upp_sh;
      int img = pix / (p.IH * p.IW);
      int rem = pix - img * (p.IH * p.IW);
      int iy = rem / p.IW, ix = rem - iy * p.IW;
      const int ybase = gy0 * a.stride - a.pad, xbase = gx0 * a.stride - a.pad;
      const uint32_t cbyte = (uint32_t)((c0 + cg * 8) * 2);
      constexpr int U = AFF == 2 ? DFL_BRB_U : 8;  // loads in flight per thread (two tensors in mode 2)
      for (; pix < npix; pix += U * dpix) {
        u32x4 v[U], v2[AFF == 2 ? U : 1];
        uint32_t offo[AFF == 2 ? U : 1];
        bool ok[U];
        int pixs[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int gy = ybase + iy, gx = xbase + ix, n = img0 + img;
          pixs[u] = pix + u * dpix;
          ok[u] = pixs[u] < npix && n < a.N && (unsigned)gy < (unsigned)a.Hin && (unsigned)gx < (unsigned)a.Win;
          const uint32_t off = (uint32_t)(((n * a.Hin + gy) * a.Win + gx) * a.ldx) * 2u + cbyte;
          v[u] = __builtin_amdgcn_raw_buffer_load_b128(rsX, ok[u] ? off : OOB, 0, 0);
          if constexpr (AFF == 2) {
            const uint32_t off2 = (uint32_t)(((n * a.Hin + gy) * a.Win + gx) * a.ldx2) * 2u + cbyte;
            v2[u] = __builtin_amdgcn_raw_buffer_load_b128(rsR, ok[u] ? off2 : OOB, 0, 0);
            // (stride 1: gathered pixel (iy, ix) is output pixel (iy - pad, ix - pad) of the patch)
            const bool own = store_on && ok[u] && (unsigned)(iy - a.pad) < (unsigned)p.PH && (unsigned)(ix - a.pad) < (unsigned)p.PW;
            offo[u] = own ? (uint32_t)(((n * a.Hin + gy) * a.Win + gx) * a.ldxo) * 2u + cbyte : OOB;
          }
          ix += dpix_x;
          iy += dpix_y;
          if (ix >= p.IW) {
            ix -= p.IW;
            ++iy;
          }
          while (iy >= p.IH) {
            iy -= p.IH;
            ++img;
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (pixs[u] < npix) {
            u32x4 w = v[u];
            if constexpr (AFF == 1) {              // zero padding applies AFTER the BatchNorm affine: outside pixels stay 0
              if (ok[u]) {
                w.x = pack_bf2(fmaf(bf_lo(w.x), sc[0], sh[0]), fmaf(bf_hi(w.x), sc[1], sh[1]));
                w.y = pack_bf2(fmaf(bf_lo(w.y), sc[2], sh[2]), fmaf(bf_hi(w.y), sc[3], sh[3]));
                w.z = pack_bf2(fmaf(bf_lo(w.z), sc[4], sh[4]), fmaf(bf_hi(w.z), sc[5], sh[5]));
                w.w = pack_bf2(fmaf(bf_lo(w.w), sc[6], sh[6]), fmaf(bf_hi(w.w), sc[7], sh[7]));
              }
            }
            if constexpr (AFF == 2) {              // outside pixels were loaded as zeros: r = 0 there, the value stays 0
              const u32x4 r = v2[u];
              auto brb = [](float dy, float rv, float A, float B, float Cc) { return rv > 0.f ? fmaf(A, dy, fmaf(B, rv, Cc)) : 0.f; };
              w.x = pack_bf2(brb(bf_lo(w.x), bf_lo(r.x), sc[0], sh[0], sq[0]), brb(bf_hi(w.x), bf_hi(r.x), sc[1], sh[1], sq[1]));
              w.y = pack_bf2(brb(bf_lo(w.y), bf_lo(r.y), sc[2], sh[2], sq[2]), brb(bf_hi(w.y), bf_hi(r.y), sc[3], sh[3], sq[3]));
              w.z = pack_bf2(brb(bf_lo(w.z), bf_lo(r.z), sc[4], sh[4], sq[4]), brb(bf_hi(w.z), bf_hi(r.z), sc[5], sh[5], sq[5]));
              w.w = pack_bf2(brb(bf_lo(w.w), bf_lo(r.w), sc[6], sh[6], sq[6]), brb(bf_hi(w.w), bf_hi(r.w), sc[7], sh[7], sq[7]));
              if (store_on) __builtin_amdgcn_raw_buffer_store_b128(w, rsO, offo[u], 0, 0);     // (outside the interior: out of range, dropped)
            }
            *reinterpret_cast<u32x4*>(smem + (uint32_t)pixs[u] * (uint32_t)S + (uint32_t)cg * 16u) = w;
          }
        }
      }
    }
    __syncthreads();
    TRACC(1, tb0)
#ifdef DFL_CONVP_TRACE
    const long long tb1 = __builtin_amdgcn_s_memtime();
#endif

    // ================================================================ k-steps of this block: s = tap * CKC + chunk
    // A fragments run one k-step ahead of the matrix instructions that use them: the reads of step s + 1 are issued before the
    // instructions of step s (a fragment read takes 64-128 cycles plus the scalar cursor arithmetic in front of its address, an
    // instruction 32).  (Two steps ahead, a second register set: measured no faster.)
    bf16x8_t afq[TM];
    auto fetch_a = [&](int s) {
      s = s < S_steps ? s : S_steps - 1;           // dead steps of the last group: weights were loaded as zeros
      const int tap = s >> ckc_sh, cc = s & (CKC - 1);
      const int ty = (tap * kw_magic) >> 8, tx = tap - ty * KW;
      const uint32_t aoff = (uint32_t)((ty * p.IW + tx) * S + cc * 32);
#pragma unroll
      for (int i = 0; i < TM; ++i) afq[i] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u32x4*>(smem + a_base[i] + aoff));
    };
    auto compute_group = [&](int gl, int set) {
      const int g = gl * KS + kg;
#pragma unroll
      for (int e = 0; e < G; ++e) {
        bf16x8_t af[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) af[i] = afq[i];
        // the step this k-group takes next
        fetch_a(e + 1 < G ? g * G + e + 1 : (g + KS) * G);
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const bf16x8_t bf = __builtin_bit_cast(bf16x8_t, breg[set][e][j]);
#pragma unroll
          for (int i = 0; i < TM; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf, acc[i][j], 0, 0, 0);
        }
      }
    };
    fetch_a(kg * G);
    load_group(blk, 0, 0);
    load_group(blk, 1, 1);
    for (int g = 0; g < ngroups; g += 3) {
      load_group(blk, g + 2, 2);
      compute_group(g, 0);
      if (g + 1 < ngroups) {
        load_group(blk, g + 3, 0);
        compute_group(g + 1, 1);
      }
      if (g + 2 < ngroups) {
        load_group(blk, g + 4, 1);
        compute_group(g + 2, 2);
      }
    }
    TRACC(2, tb1)
  }
  }
  TR(3)

  // ==================================================================== the two k-groups add up (through LDS, tile row by tile row)
  if constexpr (KS == 2) {
    constexpr int XP = WN * TN * 32 + 4;
    float* xg = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      __syncthreads();                                // the k loop / the previous tile row is done with this LDS region
      if (kg == 1) {
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) xg[(wm * 32 + mfma32_row(r, lane)) * XP + (wn * TN + j) * 32 + li] = acc[i][j][r];
      }
      __syncthreads();
      if (kg == 0) {
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][j][r] += xg[(wm * 32 + mfma32_row(r, lane)) * XP + (wn * TN + j) * 32 + li];
      }
    }
  }

  // ==================================================================== epilogue
  const bool sliced = p.splits > 1;
  if (sliced) {
    if (KS == 2 && kg == 1) return;
    // K slices: raw fp32 partial sums, row = GEMM row, 128-byte runs per accumulator row; convp_finish_kernel does the rest
    float* part = a.partial + (int64_t)bslice * p.Mtot * a.Ntot;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int q = (wm * TM + i) * 32 + 8 * g + 4 * lh;
        int img = pdiv(q, p.mPP, PP);
        int r = q - img * PP;
        int py = pdiv(r, p.mPW, p.PW), px = r - py * p.PW;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int n = img0 + img, gy = gy0 + py, gx = gx0 + px;
          const bool rok = img < p.IPP && n < a.N && gy < p.Hg && gx < p.Wg;
          const int64_t m = ((int64_t)n * p.Hg + gy) * p.Wg + gx;
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const int col = n0 + (wn * TN + j) * 32 + li;
            if (rok && col < a.Ntot) part[m * a.Ntot + col] = acc[i][j][4 * g + rr];
          }
          if (++px == p.PW) {
            px = 0;
            if (++py == p.PH) {
              py = 0;
              ++img;
            }
          }
        }
      }
    }
    return;
  }

  // One pass per tile row i of the waves: the WM x WN waves drop their 32 x (TN*32) accumulator tiles into LDS as a
  // [WM*32 rows][BN columns] fp32 image (lane = column: 128-byte runs per row), then every thread takes 8 consecutive
  // columns of a row -- bias, ReLU, + BN(other), accumulate, statistics on 8 values at a time, ONE 16-byte bf16 store (and
  // 16-byte loads of the partner tensors) instead of eight 2-byte accesses per tensor.
  constexpr int BN = WN * TN * 32;
  // The streamed (global A) form passes no barrier between the fill of add_tab at kernel start and the reads below: a wave that did
  // not take part in the fill can be through a short k loop (K = 64: four k-steps) before the filling wave has derived the live
  // scale / shift (16 fp64 loads + a square root per column) -- round 6 found a 1x1 layer's output changing from run to run once the
  // measured table gave it this form with 16 x 8 patches (docs/experiments/table_bisect.py).  The LDS-image form has its staging barriers.
  if constexpr (GA) __syncthreads();
  constexpr int EP = BN + 4;                          // row pitch in floats (+4: rows 4 apart on different banks)
  constexpr int UPR = BN / 8;                         // 8-column units per row
  constexpr int RPS = (NT / UPR) < WM * 32 ? (NT / UPR) : WM * 32;   // rows per step of the workgroup's threads
  static_assert(NT % UPR == 0 && (WM * 32) % RPS == 0, "row phase mapping");
  const bool rowthread = (RPS * UPR == NT) ? true : (tid < RPS * UPR);   // (two k-groups on a narrow tile: more threads than (row, unit) pairs)
  float* ep = reinterpret_cast<float*>(smem);
  const bool do_stats = a.stat_partials != nullptr || a.stat_totals != nullptr;
  const bool scat = a.scatter2x2 != 0;
  const unsigned short* addp = reinterpret_cast<const unsigned short*>(a.add);
  const unsigned short* sop = reinterpret_cast<const unsigned short*>(a.stat_other);
  unsigned short* yp = reinterpret_cast<unsigned short*>(a.y);
  const int ucol = (tid % UPR) * 8;                   // this thread's 8 columns inside the workgroup's BN
  const int urow = tid / UPR;
  const int ncol = n0 + ucol;                         // first of its GEMM columns
  const bool cok = ncol < a.Ntot;                     // (Ntot % 8 == 0: a unit is inside or outside as a whole)
  const int cab = (scat && cok) ? ncol / p.Cout : 0;
  const int cco = scat ? ncol - cab * p.Cout : ncol;
  float cbias[8] __attribute__((aligned(16))), casc[8] __attribute__((aligned(16))), cash[8] __attribute__((aligned(16))), s1[8], s2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {                       // (from the table filled at kernel start; barriers passed since)
    casc[e] = add_tab[ucol + e];
    cash[e] = add_tab[BN + ucol + e];
    cbias[e] = add_tab[2 * BN + ucol + e];
    s1[e] = 0.f;
    s2[e] = 0.f;
  }
  // The per-column constants above must have ARRIVED before the row loops: with a load still outstanding at the loop header the
  // compiler covers their first use inside the loop by s_waitcnt vmcnt(0) -- which, on every iteration, also waits for the
  // previous row's STORE to be acknowledged by memory (measured: 3 us of a workgroup's 13 on a 32-column layer).
  __builtin_amdgcn_s_waitcnt(0x0F70);                 // vmcnt(0) only
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#ifdef DFL_CONVP_TRACE
    const long long te0 = __builtin_amdgcn_s_memtime();
#endif
    __syncthreads();                                  // the previous pass (or the k loop) is done with this LDS region
    TRACC(6, te0)
#ifdef DFL_CONVP_TRACE
    const long long te1 = __builtin_amdgcn_s_memtime();
#endif
    if (KS == 1 || kg == 0) {
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          ep[(wm * 32 + mfma32_row(r, lane)) * EP + (wn * TN + j) * 32 + li] = acc[i][j][r];
    }
    __syncthreads();
    TRACC(7, te1)
#ifdef DFL_CONVP_TRACE
    const long long te2 = __builtin_amdgcn_s_memtime();
#endif
    for (int rl = rowthread ? urow : WM * 32; rl < WM * 32; rl += RPS) {    // row rl of the image = row (rl / 32) * TM*32 + i*32 + rl % 32 of the patch
      const int q = ((rl >> 5) * TM + i) * 32 + (rl & 31);
      const int img = pdiv(q, p.mPP, PP);
      const int rr = q - img * PP;
      const int py = pdiv(rr, p.mPW, p.PW), px = rr - py * p.PW;
      const int n = img0 + img, gy = gy0 + py, gx = gx0 + px;
      if (!(cok && img < p.IPP && n < a.N && gy < p.Hg && gx < p.Wg)) continue;
      // (32-bit element offsets: the host checks every tensor of the epilogue against 2^32 elements; 64-bit multiplies made this
      // loop the longest stretch of a workgroup's epilogue)
      const uint32_t m = (uint32_t)((n * p.Hg + gy) * p.Wg + gx);
      float v[8];
      const float4 v0 = *reinterpret_cast<const float4*>(ep + rl * EP + ucol);
      const float4 v1 = *reinterpret_cast<const float4*>(ep + rl * EP + ucol + 4);
      v[0] = v0.x; v[1] = v0.y; v[2] = v0.z; v[3] = v0.w; v[4] = v1.x; v[5] = v1.y; v[6] = v1.z; v[7] = v1.w;
      // pixel and column of this unit in y (scatter2x2: the 2x2 position its column group stands for)
      const uint32_t opix = scat ? (uint32_t)((n * a.Hout + 2 * gy + (cab >> 1)) * a.Wout + 2 * gx + (cab & 1)) : m;
      const int ocol = scat ? cco : ncol;
      ep_row8(a, v, cbias, casc, cash, addp, m * (uint32_t)a.ldadd + (uint32_t)ncol, yp, opix * (uint32_t)a.ldy + (uint32_t)ocol, sop,
              opix * (uint32_t)a.ldso + (uint32_t)ocol, do_stats, s1, s2);
    }
    TRACC(8, te2)
  }
#ifdef DFL_CONVP_TRACE
  if (tid == 0 && a.partial != nullptr) {
    long long* sink = reinterpret_cast<long long*>(a.partial) + (int64_t)(bpatch + p.npatch * btile) * 12;
    sink[8] = tr_t[6]; sink[9] = tr_t[7]; sink[10] = tr_t[8];
    sink[0] = tr_t[0]; sink[1] = tr_t[1]; sink[2] = tr_t[2]; sink[3] = tr_t[3]; sink[4] = __builtin_amdgcn_s_memtime();
    sink[5] = tr_t[5]; sink[6] = __builtin_amdgcn_s_memrealtime(); sink[7] = 1;
  }
#endif
  if (!do_stats) return;
  // per-column sums of the workgroup -> one row of stat_partials (rows = patches): threads of one column unit add up
  // through LDS in a fixed order
  ep_stats_tail<BN, RPS, NT>(reinterpret_cast<float*>(smem), s1, s2, urow, ucol, rowthread, n0, a.Ntot, [&](int which, int n, float sum) {
    if (scat) {                                        // rows = (patch, 2x2 position): [.][2][Cout], the sums of y's Cout channels
      const int ab = n / p.Cout, co = n - ab * p.Cout;
      if (a.stat_totals != nullptr) bn_live_add(a.stat_totals, bpatch * 4 + ab, which, p.Cout, co, sum);
      else a.stat_partials[(((int64_t)bpatch * 4 + ab) * 2 + which) * p.Cout + co] = sum;
    } else if (a.stat_totals != nullptr) {             // live statistics: added to the layer's totals (hardware fp64 atomics)
      bn_live_add(a.stat_totals, bpatch, which, a.Ntot, n, sum);
    } else {
      a.stat_partials[((int64_t)bpatch * 2 + which) * a.Ntot + n] = sum;
    }
  });
}

// K-slice finish: y = epilogue(sum_s partial[s]) -- conv_finish_kernel of conv_gemm.hip for bf16 tensors.
__global__ void __launch_bounds__(256) convp_finish_kernel(const ConvP p, int TX, int rows_per_block) {
  __shared__ float red[2][256];
  const dfl_conv_args& a = p.a;
  const int Ntot = a.Ntot;
  const int TY = 256 / TX;
  const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
  const int n = blockIdx.y * TX + tx;
  const bool nok = n < Ntot;
  int co = n, ab = 0;
  if (a.scatter2x2 && nok) {
    ab = n / p.Cout;
    co = n - ab * p.Cout;
  }
  float bias, asc, ash;
  ep_col_consts(a, n, co, nok, true, &bias, &asc, &ash);
  const __bf16* addp = reinterpret_cast<const __bf16*>(a.add);
  const __bf16* sop = reinterpret_cast<const __bf16*>(a.stat_other);
  __bf16* yp = reinterpret_cast<__bf16*>(a.y);
  const float osc = (a.out_scale != nullptr && nok) ? a.out_scale[co] : 1.f, osh = (a.out_scale != nullptr && nok) ? a.out_shift[co] : 0.f;
  const int64_t slice = (int64_t)p.Mtot * Ntot;
  const int r0 = blockIdx.x * rows_per_block;
  const int r1 = min(r0 + rows_per_block, p.Mtot);
  float s1 = 0.f, s2 = 0.f;
  if (nok) {
    for (int m = r0 + ty; m < r1; m += TY) {
      const float* pp = a.partial + (int64_t)m * Ntot + n;
      float v = 0.f;
      for (int s = 0; s < p.splits; ++s) v += pp[(int64_t)s * slice];
      v += bias;
      if (a.relu) v = fmaxf(v, 0.f);
      if (addp != nullptr) v += fmaf(ld_bf(addp + (int64_t)m * a.ldadd + n), asc, ash);
      int64_t opix = m;
      if (a.scatter2x2) {
        const int jx = m % p.Wg;
        const int t = m / p.Wg;
        const int iy = t % p.Hg;
        const int ni = t / p.Hg;
        opix = ((int64_t)ni * a.Hout + 2 * iy + (ab >> 1)) * a.Wout + 2 * jx + (ab & 1);
      }
      __bf16* dst = yp + opix * a.ldy + co;
      if (a.accumulate) v += (float)*dst;
      __bf16 hv = (__bf16)v;
      if (a.out_scale != nullptr) hv = (__bf16)fmaf((float)hv, osc, osh);       // (latency form with K slices: the consumer's BatchNorm, include/dfl_hip.h)
      *dst = hv;
      const float vr = (float)hv;
      const float u = (sop != nullptr) ? ld_bf(sop + opix * a.ldso + co) : vr;
      s1 += vr;
      s2 = fmaf(vr, u, s2);
    }
  }
  if (a.stat_partials == nullptr && a.stat_totals == nullptr) return;
  red[0][threadIdx.x] = s1;
  red[1][threadIdx.x] = s2;
  __syncthreads();
  if (ty == 0 && nok) {
    float t1 = 0.f, t2 = 0.f;
    for (int y = 0; y < TY; ++y) {
      t1 += red[0][y * TX + tx];
      t2 += red[1][y * TX + tx];
    }
    if (a.scatter2x2 && a.stat_totals != nullptr) {
      bn_live_add(a.stat_totals, (int)blockIdx.x * 4 + ab, 0, p.Cout, co, t1);
      bn_live_add(a.stat_totals, (int)blockIdx.x * 4 + ab, 1, p.Cout, co, t2);
    } else if (a.scatter2x2) {                         // rows = (row block, 2x2 position), see convp_kernel
      a.stat_partials[(((int64_t)blockIdx.x * 4 + ab) * 2 + 0) * p.Cout + co] = t1;
      a.stat_partials[(((int64_t)blockIdx.x * 4 + ab) * 2 + 1) * p.Cout + co] = t2;
    } else if (a.stat_totals != nullptr) {
      bn_live_add(a.stat_totals, (int)blockIdx.x, 0, Ntot, n, t1);
      bn_live_add(a.stat_totals, (int)blockIdx.x, 1, Ntot, n, t2);
    } else {
      a.stat_partials[((int64_t)blockIdx.x * 2 + 0) * Ntot + n] = t1;
      a.stat_partials[((int64_t)blockIdx.x * 2 + 1) * Ntot + n] = t2;
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------

// Row blocks of convp_finish_kernel = rows of stat_partials the following finalize kernel has to read.  Few (<= FIN_ROWS) and
// the finalize launch reads a few hundred KB instead of up to 4.7 MB (one row per 1-2 GEMM rows on the deep levels: its
// 10-12 us there against 5-6 us elsewhere); the finish kernel keeps its parallelism through narrow column blocks (FIN_TX).
constexpr int FIN_ROWS = 128;                  // (measured 2048 / 512 / 256 / 128 rows: 4.89 / 4.88 / 4.865 / 4.85 ms per step)
constexpr int FIN_TX = 32;
static int finish_rows_p(int M, int Ntot) {
  int64_t nb = ceil_div((int64_t)M * Ntot, 1024);
  if (nb > 2048) nb = 2048;
  if (nb > FIN_ROWS) nb = FIN_ROWS;
  if (nb > M) nb = M;
  return nb < 1 ? 1 : (int)nb;
}

int convp_finish_rows(const ConvP& p) { return finish_rows_p(p.Mtot, p.a.Ntot); }

template <int WM, int WN, int TM, int TN, bool GA = false, int KS = 1>
static int convp_launch_t(const ConvPlan& pl, hipStream_t s) {
  const ConvP& p = pl.p;
  const bool aff = p.a.in_scale != nullptr || p.a.in_tot != nullptr;
  dim3 grid((unsigned)p.grid);
  constexpr int NT_ = 256 * KS;
  if constexpr (GA) {
    auto k = convp_kernel<WM, WN, TM, TN, 0, true>;
    DFL_LDS_OPT_IN(k, kLdsOptIn, "dfl_conv2d (bf16)")
    hipLaunchKernelGGL(k, grid, dim3(256), pl.lds, s, p);
  } else if (p.a.x_mode != 0) {
    auto k = convp_kernel<WM, WN, TM, TN, 2, false, KS>;
    DFL_LDS_OPT_IN(k, kLdsOptIn, "dfl_conv2d (bf16)")
    hipLaunchKernelGGL(k, grid, dim3(NT_), pl.lds, s, p);
  } else if (aff) {
    auto k = convp_kernel<WM, WN, TM, TN, 1, false, KS>;
    DFL_LDS_OPT_IN(k, kLdsOptIn, "dfl_conv2d (bf16)")
    hipLaunchKernelGGL(k, grid, dim3(NT_), pl.lds, s, p);
  } else {
    auto k = convp_kernel<WM, WN, TM, TN, 0, false, KS>;
    DFL_LDS_OPT_IN(k, kLdsOptIn, "dfl_conv2d (bf16)")
    hipLaunchKernelGGL(k, grid, dim3(NT_), pl.lds, s, p);
  }
  return check_launch("dfl_conv2d (bf16)");
}

// The configurations conv_plan.hip numbers 0 ... 38 (dfl_conv_config reports 16 + the number)
const PatchTile* convp_tiles() {
  static const PatchTile t[kNumPatchTiles] = {
    {4, 1, 2, 1, 0, 1, convp_launch_t<4, 1, 2, 1>}, {4, 1, 1, 1, 0, 1, convp_launch_t<4, 1, 1, 1>}, {2, 2, 4, 1, 0, 1, convp_launch_t<2, 2, 4, 1>},
    {2, 2, 3, 1, 0, 1, convp_launch_t<2, 2, 3, 1>}, {2, 2, 2, 1, 0, 1, convp_launch_t<2, 2, 2, 1>}, {1, 4, 2, 1, 0, 1, convp_launch_t<1, 4, 2, 1>},
    {1, 4, 3, 1, 0, 1, convp_launch_t<1, 4, 3, 1>}, {1, 4, 4, 1, 0, 1, convp_launch_t<1, 4, 4, 1>}, {1, 4, 6, 1, 0, 1, convp_launch_t<1, 4, 6, 1>},
    {1, 4, 9, 1, 0, 1, convp_launch_t<1, 4, 9, 1>}, {2, 2, 1, 1, 0, 1, convp_launch_t<2, 2, 1, 1>}, {1, 4, 1, 1, 0, 1, convp_launch_t<1, 4, 1, 1>},
    {4, 1, 3, 1, 0, 1, convp_launch_t<4, 1, 3, 1>}, {4, 1, 4, 1, 0, 1, convp_launch_t<4, 1, 4, 1>}, {2, 2, 6, 1, 0, 1, convp_launch_t<2, 2, 6, 1>},
    // two column tiles per wave (15 ...): half the LDS fragment reads per matrix instruction
    {2, 2, 2, 2, 0, 1, convp_launch_t<2, 2, 2, 2>}, {2, 2, 3, 2, 0, 1, convp_launch_t<2, 2, 3, 2>}, {2, 2, 4, 2, 0, 1, convp_launch_t<2, 2, 4, 2>},
    {4, 1, 2, 2, 0, 1, convp_launch_t<4, 1, 2, 2>}, {4, 1, 3, 2, 0, 1, convp_launch_t<4, 1, 3, 2>}, {1, 4, 2, 2, 0, 1, convp_launch_t<1, 4, 2, 2>},
    {1, 4, 3, 2, 0, 1, convp_launch_t<1, 4, 3, 2>},
    // 1x1 windows streamed from global memory (22 ...)
    {4, 1, 1, 1, 1, 1, convp_launch_t<4, 1, 1, 1, true>}, {4, 1, 2, 1, 1, 1, convp_launch_t<4, 1, 2, 1, true>},
    {2, 2, 1, 1, 1, 1, convp_launch_t<2, 2, 1, 1, true>}, {2, 2, 2, 1, 1, 1, convp_launch_t<2, 2, 2, 1, true>},
    {1, 4, 1, 1, 1, 1, convp_launch_t<1, 4, 1, 1, true>}, {1, 4, 2, 1, 1, 1, convp_launch_t<1, 4, 2, 1, true>},
    {4, 1, 1, 2, 1, 1, convp_launch_t<4, 1, 1, 2, true>}, {2, 2, 1, 2, 1, 1, convp_launch_t<2, 2, 1, 2, true>},
    // two k-groups (512 threads, 30 ...)
    {1, 4, 3, 1, 0, 2, convp_launch_t<1, 4, 3, 1, false, 2>}, {1, 4, 2, 1, 0, 2, convp_launch_t<1, 4, 2, 1, false, 2>},
    {1, 4, 4, 1, 0, 2, convp_launch_t<1, 4, 4, 1, false, 2>}, {2, 2, 3, 1, 0, 2, convp_launch_t<2, 2, 3, 1, false, 2>},
    {2, 2, 2, 1, 0, 2, convp_launch_t<2, 2, 2, 1, false, 2>}, {1, 4, 2, 2, 0, 2, convp_launch_t<1, 4, 2, 2, false, 2>},
    {2, 2, 2, 2, 0, 2, convp_launch_t<2, 2, 2, 2, false, 2>}, {4, 1, 3, 1, 0, 2, convp_launch_t<4, 1, 3, 1, false, 2>},
    {4, 1, 2, 1, 0, 2, convp_launch_t<4, 1, 2, 1, false, 2>}};
  return t;
}

// Every bf16 plan, whatever its kernel family, then the K slices' sums
int convp_launch(const ConvPlan& pl, hipStream_t s) {
  const ConvP& p = pl.p;
  const int rc = pl.launch(pl, s);
  if (rc != DFL_OK || p.splits <= 1) return rc;
  int tx = 1;
  while (tx * 2 <= p.a.Ntot && tx * 2 <= FIN_TX) tx *= 2;
  const int nb = finish_rows_p(p.Mtot, p.a.Ntot);
  const int rpb = (int)ceil_div(p.Mtot, nb);
  dim3 grid((unsigned)nb, (unsigned)ceil_div(p.a.Ntot, tx));
  hipLaunchKernelGGL(convp_finish_kernel, grid, dim3(256), 0, s, p, tx, rpb);
  return check_launch("dfl_conv2d (bf16, split-K finish)");
}

}  // namespace dfl
