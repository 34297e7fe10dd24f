// Gather-GEMM convolution on the gfx950 fp32 matrix cores (v_mfma_f32_32x32x2_f32).
//
// One kernel family serves nn.Conv2d 3x3 / 1x1 / 2x2-stride-2, nn.ConvTranspose2d(k2,s2) (scatter epilogue) and, with
// re-packed weights, the data gradient of each of them (reference: train_test_code/unet.py:93,207,211,218,240 and torch
// autograd at train.py:422).  Contract: include/dfl_hip.h (dfl_conv2d).
//
// Per workgroup (WM x WN waves, each wave TM x TN tiles of 32x32), K walked in chunks of KC = 16 (k = tap*Cin + c):
//   * gather: each thread fetches float4s (4 channels of one pixel at one tap) of the [BM pixels][16] slab straight from
//     the NHWC activation and float4s of the quad-packed weight slab, into registers, while the MFMAs of the previous
//     chunk run out of LDS; afterwards the registers go to the other LDS buffer (one barrier per chunk).
//   * LDS images are planes of 32-byte rows: plane g of the fp32 image holds k = 8g..8g+7 of every row (two 16-byte
//     units), plane q of a split-bf16 image the 16 values of part q; the two units of a row swap places when bit 3 of
//     the row is set.  A lane reads ONE b128 per operand and 8 k-values: lane (i, h) gets unit h of row i (fp32: k =
//     8g+4h..8g+4h+3, component c feeds MFMA c; the k-order inside a chunk is permuted, the set is not).  With that
//     swap both the b128 fragment reads (16-lane groups {0-3,12-15,20-27}, ...) and the staging writes (b128: 2 rows x
//     4 quads; b64: 4 rows x 4 quads per lane group) touch every bank once: no conflict cycles (the padded row-major
//     layout this replaces spent a third of its LDS cycles on write conflicts, SQ_LDS_BANK_CONFLICT).
//   * the matrix pipe issues one 32x32x2 per 64 cycles per SIMD and a SIMD has only ~12 other issue slots in that time
//     (docs/experiments/exp_mfma.cpp: the bare loop reaches 100-125 TFLOP/s), so the fast path (MODE 1) is written to spend as
//     few VALU/SALU instructions per MFMA as possible:
//       - buffer loads with hardware bounds checking: an invalid tap/row/column gets an out-of-range offset and the load
//         returns 0 -- no clamped address, no select, no branch (a load under a condition would make hipcc branch and
//         wait vmcnt(0) per element);
//       - Cin % 16 == 0 => every chunk lies inside one tap: the (tap, channel) cursor is wave-uniform (SALU), the per-row
//         work is a bit test of a precomputed tap-validity mask and one 32-bit add;
//       - weight slab offsets are loop invariant per thread, the chunk advance rides in the scalar offset;
//       - selects / BatchNorm affine / LDS writes sit behind the MFMA block (sched_barrier) so the load latency of chunk
//         c+1 hides under the matrix work of chunk c.
//     MODE 0 is the general fallback (any Cin / alignment: the network's first layer and tiny test nets).
// Epilogue: bias, ReLU, "+ BN(other)" (residual sum), accumulate, NHWC or 2x2-scatter store, per-channel partial sums
//   (v, v*u) reduced lane -> half-wave (xor-32 shuffle) -> workgroup (LDS) -> one row of stat_partials per row block;
//   dfl_bn_finalize adds the rows in fp64.  EPI 0 = the common simple form (bias/ReLU/statistics, bounds by buffer
//   store), EPI 1 = everything.  Small-M / long-K layers are cut along K (split-K) and finished by conv_finish_kernel.
#include <stdlib.h>
#include <string.h>

#include "common.h"
#include "conv_epilogue.h"
#include "conv_plan.h"
#include "conv_rows.h"
#include "direct_small.h"

namespace dfl {

// Second launch-bound = waves per SIMD the register allocation must leave room for (residency per CU, see pick_cfg).
constexpr int conv_occ(int tiles) { return tiles >= 4 ? 2 : (tiles == 2 ? 4 : 5); }

// MATH 1 ("bf16x3") / MATH 2 ("bf16x6"): every fp32 operand value x is split at the LDS write into NP = 2 / 3 bf16
// parts (hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid)) and the product is accumulated from the part
// products of order i + j < NP on the bf16 matrix pipe (v_mfma_f32_32x32x16_bf16, fp32 accumulate): 3 / 6 instructions
// of 32 cycles per 16 k-values instead of 8 of 64.  bf16x3 drops terms of relative size 2^-16 per product (1e-4-class
// results), bf16x6 drops 2^-24: the products are as exact as fp32 multiplication.  A row of the LDS images holds the
// 16 values of part 0 (32 B), then part 1, (part 2): pitch 80 B like the 16 fp32 values of MATH 0 for NP = 2, 112 B for 3.
template <int WM, int WN, int TM, int TN, int MODE, bool AFF, int EPI, int MATH>
__global__ void __launch_bounds__(WM* WN * 64, conv_occ(TM* TN)) conv_gemm_kernel(const ConvK p) {
  static_assert(MATH == 0 || MODE == 1, "the split-bf16 product exists for the fast gather only");
  // MATH 3 / 4 = bf16x3 with operand formats fixed at compile time (the loop body then is one basic block the scheduler
  // can interleave): 3 = weights arrive as split quads, the gathered operand is split here; 4 = both arrive split.
  constexpr bool WPRE = (MATH == 3 || MATH == 4), XPRE = (MATH == 4);
  static_assert(!(XPRE && AFF), "a split input cannot take an affine on load");
  constexpr int NT = WM * WN * 64;
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  // MATH 5 = plain bf16 products (mode 3): one part, one matrix instruction per 16 k-values; split operands are read
  // through their hi halves.
  constexpr int NP = MATH == 0 ? 0 : (MATH == 2 ? 3 : (MATH == 5 ? 1 : 2));       // bf16 parts per value
  constexpr int NPL = (MATH == 0) ? 2 : NP;                // planes per LDS image
  constexpr int PLA = BM * 8 + 16, PLB = BN * 8 + 16;      // plane strides (words); +16: the two planes of a b128 write sit on different banks
  constexpr int IMA = NPL * PLA, IMB = NPL * PLB;          // one image of each operand
  constexpr int RPP = NT / 4;  // pixel rows covered per pass of the A gather
  static_assert(RPP % 16 == 0, "the unit swap of a thread's rows must not depend on the pass");
  constexpr int QA = BM / RPP;
  static_assert(BM % RPP == 0, "A tile must divide evenly");
  constexpr int NQB = (KC / 4) * BN;   // B quads per chunk: (k-quad, column)
  constexpr int QB = (NQB + NT - 1) / NT;

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;             // [2][NPL][BM rows of 8 words (+16)]  row = pixel
  float* Bs = smem + 2 * IMA;   // [2][NPL][BN rows of 8 words (+16)]  row = output column
  // weight quads of a chunk: 16 consecutive lanes take 4 columns x 4 k-quads (lanes of a quad: consecutive columns)
  auto b_map = [&](int idx, int& kq, int& nn) {
    kq = (idx >> 2) & 3;
    nn = ((idx >> 4) << 2) | (idx & 3);
  };

  const dfl_conv_args& a = p.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int li = lane & 31, lh = lane >> 5;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int Hin = a.Hin, Win = a.Win, Cin = a.Cin, KW = a.KW;
  const int Ktot = p.Ktot, Ntot = a.Ntot;
  const int T = a.KH * KW;
  const int aq = tid & 3;
  const bool has_aff = a.in_scale != nullptr || a.in_tot != nullptr;

  // ---- per-thread gather rows: position of tap (0,0) and the set of taps that fall inside the image ----------------
  int a_iy0[QA], a_ix0[QA], a_base[QA];
  uint32_t a_mask[QA];
#pragma unroll
  for (int r = 0; r < QA; ++r) {
    const int m = m0 + (tid >> 2) + r * RPP;
    uint32_t mk = 0;
    if (m < p.Mtot) {
      const int ox = m % p.Wg;
      const int t = m / p.Wg;
      const int oy = t % p.Hg;
      const int n = t / p.Hg;
      a_iy0[r] = oy * a.stride - a.pad;
      a_ix0[r] = ox * a.stride - a.pad;
      a_base[r] = n * Hin * Win;
      int ty = 0, tx = 0;
      for (int t2 = 0; t2 < T; ++t2) {
        if ((unsigned)(a_iy0[r] + ty) < (unsigned)Hin && (unsigned)(a_ix0[r] + tx) < (unsigned)Win) mk |= (1u << t2);
        if (++tx == KW) {
          tx = 0;
          ++ty;
        }
      }
    } else {
      a_iy0[r] = 0;
      a_ix0[r] = 0;
      a_base[r] = 0;
    }
    a_mask[r] = mk;
  }

  // Two register sets: the loads of chunk i+2 are issued while chunk i is multiplied and chunk i+1 (issued one
  // iteration earlier) waits to be written to LDS -- two chunks of global traffic in flight per wave, which the
  // 64x64 tiles need to cover the L2/HBM latency at batch-16 sizes.
  float4 ra[2][QA];
  float4 rb[2][QB];
  float4 sc4[2], sh4[2];
  uint32_t okA[2] = {0, 0};   // MODE 1: bit r = row r valid for the chunk in flight; MODE 0: bit 4r+j
  bool all_in[2] = {false, false};                   // MODE 1 + AFF: every row of the wave is valid for that chunk's tap
  constexpr uint32_t full_rows = (1u << QA) - 1u;
  sc4[0] = sc4[1] = make_float4(1.f, 1.f, 1.f, 1.f);
  sh4[0] = sh4[1] = make_float4(0.f, 0.f, 0.f, 0.f);

  // ---- MODE 1 state --------------------------------------------------------------------------------------------------
  uint32_t a_rowb[QA];   // byte offset (mod 2^32) of (tap (0,0), channel 4*aq) of each gather row
  uint32_t b_voff[QB];   // loop-invariant byte offset of this thread's weight quads inside a chunk slab
  __amdgpu_buffer_rsrc_t rsA, rsB;
  // MODE 1 + AFF: the per-channel scale / shift live in LDS behind the operand images ([Cin] + [Cin] floats, staged once):
  // a chunk's 2 x 16 bytes per thread then are two broadcast LDS reads instead of two more vector loads through the
  // path that already carries the operands (the loop's most contended resource).
  float* Ssc = Bs + 2 * IMB;
  float* Ssh = Ssc + Cin;
  int cur_tap = 0, cur_c0 = 0, cur_dy = 0, cur_dx = 0;   // wave-uniform cursor of the chunk to load next
  if constexpr (MODE == 1) {
    rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, (int)p.x_bytes, 0x00020000);
    rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, (int)p.w_bytes, 0x00020000);
    if constexpr (AFF) {
      for (int c = tid; c < Cin; c += NT) {
        if (a.in_tot != nullptr) {      // live statistics: scale / shift of the input channels from the producer's totals (include/dfl_hip.h)
          bn_live_affine(a.in_tot, a.in_gamma, a.in_beta, a.in_count, a.bn_eps, Cin, c, Ssc + c, Ssh + c);
        } else {
          Ssc[c] = a.in_scale[c];
          Ssh[c] = a.in_shift[c];
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < QA; ++r)
      a_rowb[r] = (uint32_t)((((int64_t)a_base[r] + (int64_t)a_iy0[r] * Win + a_ix0[r]) * a.ldx + 4 * aq) * 4);
#pragma unroll
    for (int r = 0; r < QB; ++r) {
      const int idx = tid + r * NT;
      int kq, nn;
      b_map(idx, kq, nn);
      b_voff[r] = (idx < NQB && n0 + nn < Ntot) ? (uint32_t)(((int64_t)kq * Ntot + n0 + nn) * 16) : OOB;
    }
    const int k0 = (int)blockIdx.z * p.cps * KC;
    cur_tap = k0 / Cin;
    cur_c0 = k0 - cur_tap * Cin;
    cur_dy = cur_tap / KW;
    cur_dx = cur_tap - cur_dy * KW;
  }

  const int nchunks = (Ktot + KC - 1) / KC;
  const int ch_begin = blockIdx.z * p.cps;
  const int ch_end = min(ch_begin + p.cps, nchunks);

  // Loads only ISSUE into raw registers; store_AB() (after the MFMA block) applies the affine / zero fill and writes LDS.
  // Straight-line code: a chunk past the end of the slice is fetched with out-of-range offsets (reads zeros), so the
  // main loop has no conditional loads and the compiler can keep the younger set in flight across the LDS write.
  auto load_AB = [&](int ch, int set) {
    const bool live = ch < ch_end;
    if constexpr (MODE == 1) {
      // must be called once per chunk, in order: uses and advances the uniform cursor
      const bool kvalid = live && cur_tap < T;
      const uint32_t tapb = (uint32_t)(((cur_dy * Win + cur_dx) * a.ldx + cur_c0) * 4);
      const uint32_t tbit = kvalid ? (1u << cur_tap) : 0u;
      uint32_t okm = 0;
#pragma unroll
      for (int r = 0; r < QA; ++r) {
        const bool ok = (a_mask[r] & tbit) != 0;
        okm |= ok ? (1u << r) : 0u;
        ra[set][r] = buf_load4(rsA, ok ? a_rowb[r] + tapb : OOB, 0);
      }
      okA[set] = okm;
      if constexpr (AFF) all_in[set] = __builtin_amdgcn_ballot_w64(okm == full_rows) == ~0ull;
      if constexpr (AFF) {   // this thread's 4 channels of the chunk (lanes with equal aq read one address: broadcast)
        const int cofs = (kvalid ? cur_c0 : 0) + 4 * aq;
        sc4[set] = *reinterpret_cast<const float4*>(Ssc + cofs);
        sh4[set] = *reinterpret_cast<const float4*>(Ssh + cofs);
      }
      const uint32_t soff = live ? (uint32_t)ch * (uint32_t)(KC / 4 * 16) * (uint32_t)Ntot : 0u;   // chunk = 4 k-quad rows
#pragma unroll
      for (int r = 0; r < QB; ++r) rb[set][r] = buf_load4(rsB, live ? b_voff[r] : OOB, soff);
      cur_c0 += KC;
      if (cur_c0 >= Cin) {
        cur_c0 = 0;
        ++cur_tap;
        if (++cur_dx == KW) {
          cur_dx = 0;
          ++cur_dy;
        }
      }
    } else {
      // general gather: per element (tap, channel) by division, clamped unconditional loads
      const int k = ch * KC + 4 * aq;
      float vals[QA][4], scv[4], shv[4];
      const float* aff_sc = has_aff ? a.in_scale : a.w;
      const float* aff_sh = has_aff ? a.in_shift : a.w;
      uint32_t okm = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int kj = k + j;
        const bool kvalid = live && kj < Ktot;
        const int t = kvalid ? kj / Cin : 0;
        const int c = kvalid ? kj - t * Cin : 0;
        const int dy = t / KW, dx = t - dy * KW;
        scv[j] = aff_sc[has_aff ? c : 0];
        shv[j] = aff_sh[has_aff ? c : 0];
#pragma unroll
        for (int r = 0; r < QA; ++r) {
          const bool ok = kvalid && ((a_mask[r] >> t) & 1u);
          const int64_t pix = ok ? ((int64_t)a_base[r] + (int64_t)(a_iy0[r] + dy) * Win + a_ix0[r] + dx) : 0;
          okm |= ok ? (1u << (4 * r + j)) : 0u;
          vals[r][j] = a.x[pix * a.ldx + (ok ? c : 0)];
        }
      }
      okA[set] = okm;
      sc4[set] = make_float4(scv[0], scv[1], scv[2], scv[3]);
      sh4[set] = make_float4(shv[0], shv[1], shv[2], shv[3]);
#pragma unroll
      for (int r = 0; r < QA; ++r) ra[set][r] = make_float4(vals[r][0], vals[r][1], vals[r][2], vals[r][3]);
#pragma unroll
      for (int r = 0; r < QB; ++r) {
        const int idx = tid + r * NT;
        int kq, nn;
        b_map(idx, kq, nn);
        const int kquad = ch * (KC / 4) + kq, n = n0 + nn;
        const bool ok = live && (idx < NQB) && (4 * kquad < Ktot) && (n < Ntot);
        const float4 v = *reinterpret_cast<const float4*>(a.w + (ok ? ((int64_t)kquad * Ntot + n) * 4 : 0));
        rb[set][r] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  };

  auto store_AB = [&](int buf, int set) {   // buf == set everywhere: chunk parity picks both
    float* Ab = As + buf * IMA;
    const int fA = (tid >> 5) & 1;   // unit swap of this thread's rows (bit 3 of the row tid / 4)
#pragma unroll
    for (int r = 0; r < QA; ++r) {
      const int row = (tid >> 2) + r * RPP;
      float4 v = ra[set][r];
      const float4 sc = sc4[set], sh = sh4[set];
      if constexpr (MODE == 1) {
        if constexpr (AFF) {
          // zero padding applies AFTER the BatchNorm affine: out-of-image taps must stay 0.  Their data already is 0
          // (hardware bounds check), so only the shift has to be masked -- and not even that when every row of the
          // wave sees this tap inside the image (wave-uniform test: all interior tiles, and the centre tap always).
          typedef float f2 __attribute__((ext_vector_type(2)));
          f2 h0 = {sh.x, sh.y}, h1 = {sh.z, sh.w};
          if (!all_in[set]) {
            const bool ok = (okA[set] >> r) & 1u;
            h0.x = ok ? sh.x : 0.f;
            h0.y = ok ? sh.y : 0.f;
            h1.x = ok ? sh.z : 0.f;
            h1.y = ok ? sh.w : 0.f;
          }
          const f2 r0 = __builtin_elementwise_fma((f2){v.x, v.y}, (f2){sc.x, sc.y}, h0);
          const f2 r1 = __builtin_elementwise_fma((f2){v.z, v.w}, (f2){sc.z, sc.w}, h1);
          v = make_float4(r0.x, r0.y, r1.x, r1.y);
        }
      } else {
        const uint32_t o = okA[set] >> (4 * r);
        const float s0 = has_aff ? sc.x : 1.f, s1 = has_aff ? sc.y : 1.f, s2 = has_aff ? sc.z : 1.f, s3 = has_aff ? sc.w : 1.f;
        const float h0 = has_aff ? sh.x : 0.f, h1 = has_aff ? sh.y : 0.f, h2 = has_aff ? sh.z : 0.f, h3 = has_aff ? sh.w : 0.f;
        v.x = (o & 1u) ? fmaf(v.x, s0, h0) : 0.f;
        v.y = (o & 2u) ? fmaf(v.y, s1, h1) : 0.f;
        v.z = (o & 4u) ? fmaf(v.z, s2, h2) : 0.f;
        v.w = (o & 8u) ? fmaf(v.w, s3, h3) : 0.f;
      }
      if constexpr (MATH != 0) {
        uint2 parts[NP];
        if (XPRE || ((MATH == 1 || MATH == 5) && a.x_split)) {   // the producer already left hi4 | lo4 in the slot (wave uniform)
          parts[0] = make_uint2(__float_as_uint(v.x), __float_as_uint(v.y));
          if constexpr (NP > 1) parts[1] = make_uint2(__float_as_uint(v.z), __float_as_uint(v.w));
        } else {
          split_bf16<NP>(v, parts);
        }
#pragma unroll
        for (int q = 0; q < NP; ++q) *reinterpret_cast<uint2*>(Ab + q * PLA + row * 8 + 4 * ((aq >> 1) ^ fA) + 2 * (aq & 1)) = parts[q];
      } else {
        *reinterpret_cast<float4*>(Ab + (aq >> 1) * PLA + row * 8 + 4 * ((aq & 1) ^ fA)) = v;   // one ds_write_b128, no transposition
      }
    }
    float* Bb = Bs + buf * IMB;
#pragma unroll
    for (int r = 0; r < QB; ++r) {
      const int idx = tid + r * NT;
      if (NQB % NT == 0 || idx < NQB) {   // (no branch when the tile divides evenly: one scheduling region)
        int kq, nn;
        b_map(idx, kq, nn);
        const int fB = (nn >> 3) & 1;
        if constexpr (MATH != 0) {
          uint2 parts[NP];
          if (WPRE || ((MATH == 1 || MATH == 5) && a.w_split)) {
            const float4 v = rb[set][r];
            parts[0] = make_uint2(__float_as_uint(v.x), __float_as_uint(v.y));
            if constexpr (NP > 1) parts[1] = make_uint2(__float_as_uint(v.z), __float_as_uint(v.w));
          } else {
            split_bf16<NP>(rb[set][r], parts);
          }
#pragma unroll
          for (int q = 0; q < NP; ++q) *reinterpret_cast<uint2*>(Bb + q * PLB + nn * 8 + 4 * ((kq >> 1) ^ fB) + 2 * (kq & 1)) = parts[q];
        } else {
          *reinterpret_cast<float4*>(Bb + (kq >> 1) * PLB + nn * 8 + 4 * ((kq & 1) ^ fB)) = rb[set][r];
        }
      }
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  auto compute = [&](int buf) {
    const int un = 4 * (lh ^ ((li >> 3) & 1));   // this lane's unit of its row, after the swap
    const float* Ab = As + buf * IMA + (wm * (TM * 32) + li) * 8 + un;
    const float* Bb = Bs + buf * IMB + (wn * (TN * 32) + li) * 8 + un;
    if constexpr (MATH != 0) {
      // lane (row li, k-half lh): its unit (8 consecutive bf16) of part q
      bf16x8_t ap[TM][NP], bp[TN][NP];
#pragma unroll
      for (int q = 0; q < NP; ++q) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
          ap[i][q] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(Ab + i * 256 + q * PLA));
#pragma unroll
        for (int j = 0; j < TN; ++j)
          bp[j][q] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(Bb + j * 256 + q * PLB));
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int o = NP - 1; o >= 0; --o)   // order o = qa + qb, small terms first
#pragma unroll
            for (int qa = 0; qa <= o; ++qa)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[i][qa], bp[j][o - qa], acc[i][j], 0, 0, 0);
      return;
    }
#pragma unroll
    for (int g = 0; g < KC / 8; ++g) {
      float4 av[TM], bv[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) av[i] = *reinterpret_cast<const float4*>(Ab + i * 256 + g * PLA);
#pragma unroll
      for (int j = 0; j < TN; ++j) bv[j] = *reinterpret_cast<const float4*>(Bb + j * 256 + g * PLB);
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32((&av[i].x)[q], (&bv[j].x)[q], acc[i][j], 0, 0, 0);
    }
  };

  // One-tile waves with compile-time operand formats and no affine: the half-iteration is one basic block, and the
  // scheduler is told to put the LDS writes of the next chunk (which do not depend on the matrix instructions) in front
  // of / between them instead of behind them: a wave's serial chain per chunk gets shorter (the loop is chain-bound).
  constexpr bool HINTED = WPRE && !AFF && TM * TN == 1 && (NQB % NT == 0);
  auto sched_hint = [&]() {
    if constexpr (HINTED) {
      __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);        // the 4 fragment reads
      if constexpr (XPRE) {
        __builtin_amdgcn_sched_group_barrier(0x200, 4, 0);      // the LDS writes (pure copies: hi and lo of both operands)
        __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);      // the 3 matrix instructions
      } else {
        __builtin_amdgcn_sched_group_barrier(0x200, 2, 0);      // weights: pure copies
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);      // split of the gathered operand, in two halves
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x200, 2, 0);
      }
    }
  };

  load_AB(ch_begin, 0);
  load_AB(ch_begin + 1, 1);
  store_AB(0, 0);
  __syncthreads();
  // Chunks are taken two at a time so that register set and LDS image are compile-time constants; an odd slice
  // multiplies one all-zero chunk at the end.  The sched_barriers pin the order loads | MFMAs | affine + LDS writes:
  // otherwise hipcc hoists part of store_AB() (and its vmcnt waits) above the MFMA block.
#ifdef DFL_CONV_TRACE
  // Diagnosis build only (docs/experiments/conv_phase_trace.sh): shader-clock time the first wave of every workgroup spends in
  // the four phases of the first half-iteration of each loop trip, summed over the loop, plus the whole-kernel time.
  long long tr[5] = {0, 0, 0, 0, 0};
  const long long tk0 = __builtin_amdgcn_s_memtime();
#define TR_MARK(i)                                        \
  {                                                       \
    const long long t_ = __builtin_amdgcn_s_memtime();    \
    tr[i] += t_ - tlast;                                  \
    tlast = t_;                                           \
  }
#else
#define TR_MARK(i)
#endif
#define LOOP_SYNC() __syncthreads()
  for (int ch = ch_begin; ch < ch_end; ch += 2) {
#ifdef DFL_CONV_TRACE
    long long tlast = __builtin_amdgcn_s_memtime();
#endif
    load_AB(ch + 2, 0);
    __builtin_amdgcn_sched_barrier(0);
    compute(0);
    TR_MARK(0)   // loads issued + LDS fragment reads + matrix instructions issued
    if constexpr (!HINTED) __builtin_amdgcn_sched_barrier(0);
    store_AB(1, 1);
    sched_hint();
    TR_MARK(1)   // split / affine + LDS writes
    LOOP_SYNC();
    TR_MARK(2)   // barrier
    load_AB(ch + 3, 1);
    __builtin_amdgcn_sched_barrier(0);
    compute(1);
    if constexpr (!HINTED) __builtin_amdgcn_sched_barrier(0);
    store_AB(0, 0);
    sched_hint();
    LOOP_SYNC();
  }

#ifdef DFL_CONV_TRACE
  if (a.stat_other == nullptr && a.add != nullptr && a.add_scale == nullptr && lane == 0 && wave == 0) {
    // trace sink smuggled in through `add` (unused by the traced launches): [block][6] long long
    long long* sink = reinterpret_cast<long long*>(const_cast<float*>(a.add)) +
                      (int64_t)(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z)) * 6;
    sink[0] = tr[0]; sink[1] = tr[1]; sink[2] = tr[2]; sink[3] = __builtin_amdgcn_s_memtime() - tk0;
    sink[4] = (ch_end - ch_begin + 1) / 2;
  }
#endif

  // ---- split-K: leave the raw partial sums, conv_finish_kernel applies the epilogue ---------------------------------
  if (p.splits > 1) {
    float* part = a.partial + (int64_t)blockIdx.z * p.Mtot * Ntot;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = n0 + wn * (TN * 32) + j * 32 + li;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + wm * (TM * 32) + i * 32 + mfma32_row(r, lane);
          if (n < Ntot && m < p.Mtot) part[(int64_t)m * Ntot + n] = acc[i][j][r];
        }
      }
    }
    return;
  }

  // ---- epilogue ------------------------------------------------------------------------------------------------------
  const bool do_stats = a.stat_partials != nullptr || a.stat_totals != nullptr;
  float s1[TN], s2[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    s1[j] = 0.f;
    s2[j] = 0.f;
  }
  if constexpr (EPI == 0) {
    conv_epilogue_simple<WM, WN, TM, TN>(p, acc, s1, s2, m0, n0, wm, wn, li, lh);
  } else {
    // Everything: per-column constants (this lane's TN columns), then the tile in groups of 4 consecutive rows; every
    // read the epilogue needs (residual tensor, old output, statistics partner) is issued unconditionally from a clamped
    // address for the whole group before anything is consumed: one memory round trip per group, not sixteen.
    const bool has_add = a.add != nullptr, has_so = a.stat_other != nullptr, scat = a.scatter2x2 != 0;
    int cn[TN], cco[TN], cab[TN];
    bool cok[TN];
    float cbias[TN], casc[TN], cash[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = n0 + wn * (TN * 32) + j * 32 + li;
      cok[j] = n < Ntot;
      cn[j] = cok[j] ? n : 0;
      cab[j] = scat ? cn[j] / p.Cout : 0;
      cco[j] = scat ? cn[j] - cab[j] * p.Cout : cn[j];
      cbias[j] = 0.f;
      casc[j] = 1.f;
      cash[j] = 0.f;
      if (a.bias != nullptr) cbias[j] = a.bias[cco[j]];
      if (has_add && a.add_scale != nullptr) {
        casc[j] = a.add_scale[cn[j]];
        cash[j] = a.add_shift[cn[j]];
      } else if (has_add && a.add_tot != nullptr) {      // "+ BN(add)" with live statistics
        bn_live_affine(a.add_tot, a.add_gamma, a.add_beta, a.add_count, a.bn_eps, Ntot, cn[j], &casc[j], &cash[j]);
      }
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int mb = m0 + wm * (TM * 32) + i * 32 + 8 * g + 4 * lh;   // rows mb..mb+3 <-> accumulator regs 4g..4g+3
        int jx = 0, iy = 0, ni = 0;
        if (scat) {
          const int mm = min(mb, p.Mtot - 1);
          jx = mm % p.Wg;
          const int t = mm / p.Wg;
          iy = t % p.Hg;
          ni = t / p.Hg;
        }
        int64_t off[4][TN];
        bool ok[4][TN];
        float vadd[4][TN], vold[4][TN], vso[4][TN];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int m = mb + rr;
          const bool rok = m < p.Mtot;
          const int mc = rok ? m : 0;
          const int64_t rowpix = ((int64_t)ni * a.Hout + 2 * iy) * a.Wout + 2 * jx;
          if (scat) {   // next pixel of the gather grid
            if (++jx == p.Wg) {
              jx = 0;
              if (++iy == p.Hg) {
                iy = 0;
                ++ni;
              }
            }
          }
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            ok[rr][j] = rok && cok[j];
            const int64_t o = scat ? (rowpix + (int64_t)(cab[j] >> 1) * a.Wout + (cab[j] & 1)) * a.ldy + cco[j]
                                   : (int64_t)mc * a.ldy + cn[j];
            off[rr][j] = ok[rr][j] ? o : 0;
            vadd[rr][j] = has_add ? a.add[ok[rr][j] ? ((int64_t)mc * a.ldadd + cn[j]) : 0] : 0.f;
            vold[rr][j] = a.accumulate ? a.y[off[rr][j]] : 0.f;
            vso[rr][j] = has_so ? a.stat_other[ok[rr][j] ? ((int64_t)mc * a.ldso + cn[j]) : 0] : 0.f;
          }
        }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            float v = acc[i][j][4 * g + rr] + cbias[j];
            if (a.relu) v = fmaxf(v, 0.f);
            if (has_add) v += fmaf(vadd[rr][j], casc[j], cash[j]);
            if (a.accumulate) v += vold[rr][j];
            if (ok[rr][j]) a.y[off[rr][j]] = v;
            const float vm = ok[rr][j] ? v : 0.f;
            const float u = ok[rr][j] ? (has_so ? vso[rr][j] : v) : 0.f;
            s1[j] += vm;
            s2[j] = fmaf(vm, u, s2[j]);
          }
        }
      }
    }
  }

  if (do_stats) conv_stats_tail<WM, WN, TM, TN>(p, s1, s2, smem, tid, n0, wm, wn, li, lh);
}

// Split-K finish: y = epilogue(sum_s partial[s]) with the same epilogue as above (bias, ReLU, + BN(other),
// accumulate, NHWC / 2x2-scatter store, per-channel statistics per row block).  HBM-bound stream.
__global__ void __launch_bounds__(256) conv_finish_kernel(const ConvK p, int TX, int rows_per_block) {
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
  const float bias = (a.bias != nullptr && nok) ? a.bias[co] : 0.f;
  float asc = 1.f, ash = 0.f;
  if (a.add != nullptr && a.add_scale != nullptr && nok) {
    asc = a.add_scale[n];
    ash = a.add_shift[n];
  } else if (a.add != nullptr && a.add_tot != nullptr && nok) {      // "+ BN(add)" with live statistics (include/dfl_hip.h)
    bn_live_affine(a.add_tot, a.add_gamma, a.add_beta, a.add_count, a.bn_eps, Ntot, n, &asc, &ash);
  }
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
      if (a.add != nullptr) v += fmaf(a.add[(int64_t)m * a.ldadd + n], asc, ash);
      float* dst;
      if (a.scatter2x2) {
        const int jx = m % p.Wg;
        const int t = m / p.Wg;
        const int iy = t % p.Hg;
        const int ni = t / p.Hg;
        const int64_t opix = ((int64_t)ni * a.Hout + 2 * iy + (ab >> 1)) * a.Wout + 2 * jx + (ab & 1);
        dst = a.y + opix * a.ldy + co;
      } else {
        dst = a.y + (int64_t)m * a.ldy + n;
      }
      if (a.accumulate) v += *dst;
      if (a.out_scale != nullptr) v = fmaf(v, a.out_scale[co], a.out_shift[co]);     // (latency form with K slices: the consumer's BatchNorm)
      *dst = v;
      const float u = (a.stat_other != nullptr) ? a.stat_other[(int64_t)m * a.ldso + n] : v;
      s1 += v;
      s2 = fmaf(v, u, s2);
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
    if (a.stat_totals != nullptr) {
      bn_live_add(a.stat_totals, (int)blockIdx.x, 0, Ntot, n, t1);
      bn_live_add(a.stat_totals, (int)blockIdx.x, 1, Ntot, n, t2);
    } else {
      a.stat_partials[((int64_t)blockIdx.x * 2 + 0) * Ntot + n] = t1;
      a.stat_partials[((int64_t)blockIdx.x * 2 + 1) * Ntot + n] = t2;
    }
  }
}

// ---- host side -------------------------------------------------------------------------------------

enum ConvCfg { CFG_128x128 = 0, CFG_128x64, CFG_256x32, CFG_64x64, CFG_32x64 };

static void cfg_tile(ConvCfg c, int* bm, int* bn) {
  switch (c) {
    case CFG_128x128: *bm = 128; *bn = 128; break;
    case CFG_128x64: *bm = 128; *bn = 64; break;
    case CFG_256x32: *bm = 256; *bn = 32; break;
    case CFG_64x64: *bm = 64; *bn = 64; break;
    default: *bm = 32; *bn = 64; break;
  }
}

// Largest tile that still gives the 256 CUs a few workgroups each.  Problems too small for that keep the 64x64 tile
// and are cut along K instead (split-K, see pick_splits): deep U-Net levels are M = 576..2304 pixels x K = 4608..9216.
static ConvCfg pick_cfg(int64_t M, int Ntot, bool fast = true) {
  const int64_t want = 1024;   // (512 / 256 / 128 measured with split-bf16 products as well: 1024 stays best)
  if (!fast) return CFG_64x64;   // the general-gather variant exists for one tile only
  if (Ntot <= 32) {
    if (ceil_div(M, 256) >= want / 2) return CFG_256x32;
    return (M > 32) ? CFG_64x64 : CFG_32x64;
  }
  if (Ntot >= 128 && ceil_div(M, 128) * ceil_div(Ntot, 128) >= want) return CFG_128x128;
  if (ceil_div(M, 128) * ceil_div(Ntot, 64) >= want) return CFG_128x64;
  return (M > 32) ? CFG_64x64 : CFG_32x64;
}

static int pick_splits(int64_t M, int Ntot, int Ktot, ConvCfg cfg) {
  int bm, bn;
  cfg_tile(cfg, &bm, &bn);
  const int64_t blocks = ceil_div(M, bm) * ceil_div(Ntot, bn);
  const int nchunks = (int)ceil_div(Ktot, KC);
  if (blocks >= 768 || nchunks < 16) return 1;
  int64_t s = ceil_div(1024, blocks);
  if (s > nchunks / 8) s = nchunks / 8;   // >= 128 of K per slice
  if (s > 32) s = 32;
  return s < 1 ? 1 : (int)s;
}

template <int WM, int WN, int TM, int TN, int MODE, bool AFF, int EPI, int MATH = 0>
static int launch(const ConvK& k, hipStream_t s) {
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  constexpr int npl = (MATH == 0 || MATH == 1 || MATH == 3 || MATH == 4) ? 2 : (MATH == 2 ? 3 : 1);   // planes per LDS image
  size_t lds = (size_t)(2 * npl * (BM * 8 + 16 + BN * 8 + 16)) * sizeof(float);
  if (MODE == 1 && AFF) lds += (size_t)2 * k.a.Cin * sizeof(float);   // staged scale / shift
  DFL_REQUIRE(lds <= 64 * 1024, "dfl_conv2d: %d input channels with an affine on load need %zu bytes of LDS (limit 65536)",
              k.a.Cin, lds);
  dim3 grid((unsigned)ceil_div(k.Mtot, BM), (unsigned)ceil_div(k.a.Ntot, BN), (unsigned)k.splits);
  hipLaunchKernelGGL((conv_gemm_kernel<WM, WN, TM, TN, MODE, AFF, EPI, MATH>), grid, dim3(WM * WN * 64), lds, s, k);
  return check_launch("dfl_conv2d");
}

template <int WM, int WN, int TM, int TN>
static int launch_fast(const ConvK& k, bool aff, bool general, hipStream_t s) {
  if (math_mode() == 1) {
    if (k.a.w_split && k.a.x_split)   // (never with an affine: checked by the caller)
      return general ? launch<WM, WN, TM, TN, 1, false, 1, 4>(k, s) : launch<WM, WN, TM, TN, 1, false, 0, 4>(k, s);
    if (k.a.w_split && !k.a.x_split) {
      if (aff) return general ? launch<WM, WN, TM, TN, 1, true, 1, 3>(k, s) : launch<WM, WN, TM, TN, 1, true, 0, 3>(k, s);
      return general ? launch<WM, WN, TM, TN, 1, false, 1, 3>(k, s) : launch<WM, WN, TM, TN, 1, false, 0, 3>(k, s);
    }
    if (aff) return general ? launch<WM, WN, TM, TN, 1, true, 1, 1>(k, s) : launch<WM, WN, TM, TN, 1, true, 0, 1>(k, s);
    return general ? launch<WM, WN, TM, TN, 1, false, 1, 1>(k, s) : launch<WM, WN, TM, TN, 1, false, 0, 1>(k, s);
  }
  if (math_mode() == 3) {
    if (aff) return general ? launch<WM, WN, TM, TN, 1, true, 1, 5>(k, s) : launch<WM, WN, TM, TN, 1, true, 0, 5>(k, s);
    return general ? launch<WM, WN, TM, TN, 1, false, 1, 5>(k, s) : launch<WM, WN, TM, TN, 1, false, 0, 5>(k, s);
  }
  if (math_mode() == 2) {
    if (aff) return general ? launch<WM, WN, TM, TN, 1, true, 1, 2>(k, s) : launch<WM, WN, TM, TN, 1, true, 0, 2>(k, s);
    return general ? launch<WM, WN, TM, TN, 1, false, 1, 2>(k, s) : launch<WM, WN, TM, TN, 1, false, 0, 2>(k, s);
  }
  if (aff) return general ? launch<WM, WN, TM, TN, 1, true, 1>(k, s) : launch<WM, WN, TM, TN, 1, true, 0>(k, s);
  return general ? launch<WM, WN, TM, TN, 1, false, 1>(k, s) : launch<WM, WN, TM, TN, 1, false, 0>(k, s);
}

int conv_prepare(const dfl_conv_args* a, ConvK* k) {
  DFL_REQUIRE(a != nullptr, "dfl_conv2d: null args");
  DFL_REQUIRE(a->x && a->w && a->y, "dfl_conv2d: x, w and y are required");
  DFL_REQUIRE(a->N > 0 && a->Hin > 0 && a->Win > 0 && a->Cin > 0 && a->Ntot > 0, "dfl_conv2d: bad sizes");
  DFL_REQUIRE(a->KH > 0 && a->KW > 0 && a->stride > 0 && a->pad >= 0, "dfl_conv2d: bad window");
  DFL_REQUIRE(a->KH * a->KW <= 31, "dfl_conv2d: at most 31 taps");
  DFL_REQUIRE(a->ldx >= a->Cin, "dfl_conv2d: ldx < Cin");
  DFL_REQUIRE(aligned16(a->w), "dfl_conv2d: packed weights must be 16-byte aligned");
  DFL_REQUIRE((a->in_scale == nullptr) == (a->in_shift == nullptr), "dfl_conv2d: in_scale/in_shift go together");
  DFL_REQUIRE((a->add_scale == nullptr) == (a->add_shift == nullptr), "dfl_conv2d: add_scale/add_shift go together");
  k->a = *a;
  if (a->scatter2x2) {
    DFL_REQUIRE(a->KH == 1 && a->KW == 1 && a->stride == 1 && a->pad == 0, "dfl_conv2d: scatter2x2 needs a 1x1 gather");
    DFL_REQUIRE(a->Ntot % 4 == 0, "dfl_conv2d: scatter2x2 needs Ntot = 4*Cout");
    DFL_REQUIRE(a->Hout >= 2 * a->Hin && a->Wout >= 2 * a->Win, "dfl_conv2d: scatter target too small");
    DFL_REQUIRE(a->add == nullptr && a->stat_partials == nullptr, "dfl_conv2d: scatter2x2 has no add/stats epilogue");
    k->Hg = a->Hin;
    k->Wg = a->Win;
    k->Cout = a->Ntot / 4;
  } else {
    const int ho = (a->Hin + 2 * a->pad - a->KH) / a->stride + 1;
    const int wo = (a->Win + 2 * a->pad - a->KW) / a->stride + 1;
    DFL_REQUIRE(ho == a->Hout && wo == a->Wout, "dfl_conv2d: Hout/Wout (%d,%d) do not match the window (%d,%d)",
                a->Hout, a->Wout, ho, wo);
    k->Hg = a->Hout;
    k->Wg = a->Wout;
    k->Cout = a->Ntot;
  }
  DFL_REQUIRE(a->ldy >= k->Cout, "dfl_conv2d: ldy < Cout");
  const int64_t M = (int64_t)a->N * k->Hg * k->Wg;
  DFL_REQUIRE(M < (1ll << 31) && (int64_t)a->N * a->Hin * a->Win < (1ll << 31), "dfl_conv2d: too many pixels");
  k->Mtot = (int)M;
  k->Ktot = a->KH * a->KW * a->Cin;
  // byte extents as seen from the pointers (buffer descriptors of the fast path; all must stay below 2 GiB)
  const int64_t xb = (((int64_t)a->N * a->Hin * a->Win - 1) * a->ldx + a->Cin) * 4;
  const int64_t wb = ceil_div(k->Ktot, 4) * (int64_t)a->Ntot * 16;
  const int64_t yb = a->scatter2x2 ? (((int64_t)a->N * a->Hout * a->Wout - 1) * a->ldy + k->Cout) * 4
                                   : ((M - 1) * a->ldy + a->Ntot) * 4;
  const int64_t lim = (1ll << 31) - 4096;
  k->fast = (a->Cin % KC == 0) && (a->ldx % 4 == 0) && aligned16(a->x) && xb < lim && wb < lim && yb < lim &&
            (a->in_scale == nullptr || (aligned16(a->in_scale) && aligned16(a->in_shift)));
  k->x_bytes = (uint32_t)(xb < lim ? xb : 0);
  k->w_bytes = (uint32_t)(wb < lim ? wb : 0);
  k->y_bytes = (uint32_t)(yb < lim ? yb : 0);
  const int64_t sob = (a->stat_other != nullptr) ? ((M - 1) * a->ldso + a->Ntot) * 4 : 0;
  k->so_bytes = (uint32_t)(sob < lim ? sob : 0);
  k->so_simple = sob < lim;     // the simple epilogue can fetch the statistics partner through a buffer descriptor
  k->splits = 1;
  k->cps = (int)ceil_div(k->Ktot, KC);
  return DFL_OK;
}

int conv_finish_rows(int M, int Ntot) {   // row blocks of conv_finish_kernel (= rows of stat_partials in split mode)
  int64_t nb = ceil_div((int64_t)M * Ntot, 1024);   // 4 elements per thread: the per-element loop over splits is serial
  if (nb > 2048) nb = 2048;
  if (nb > M) nb = M;
  return nb < 1 ? 1 : (int)nb;
}

int conv_gemm_cfg(const ConvK& k) { return (int)pick_cfg(k.Mtot, k.a.Ntot, k.fast); }

int conv_gemm_bm(int cfg) {
  int bm, bn;
  cfg_tile((ConvCfg)cfg, &bm, &bn);
  return bm;
}

int conv_gemm_splits(const ConvK& k) { return pick_splits(k.Mtot, k.a.Ntot, k.Ktot, pick_cfg(k.Mtot, k.a.Ntot, k.fast)); }

static int conv_finish(const ConvK& k, hipStream_t s, const char* what) {
  int tx = 1;
  while (tx * 2 <= k.a.Ntot && tx * 2 <= 256) tx *= 2;
  const int nb = conv_finish_rows(k.Mtot, k.a.Ntot);
  const int rpb = (int)ceil_div(k.Mtot, nb);
  hipLaunchKernelGGL(conv_finish_kernel, dim3((unsigned)nb, (unsigned)ceil_div(k.a.Ntot, tx)), dim3(256), 0, s, k, tx, rpb);
  return check_launch(what);
}

}  // namespace dfl

extern "C" int dfl_set_conv_rows_min_tiles(int32_t n) {
  DFL_REQUIRE(n >= 1, "dfl_set_conv_rows_min_tiles: n must be positive");
  return dfl::conv_rows_set_min_tiles(n);
}

extern "C" int dfl_conv2d_pair(const dfl_conv_args* a, const dfl_conv_args* b, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr && b != nullptr, "dfl_conv2d_pair: null arguments");
  dfl::ConvRoute r;
  if (dfl::conv_pair_route(a, b, &r) > 0) return dfl::convs_pair_launch(r.plan.p, b, static_cast<hipStream_t>(stream));
  const int rc = dfl_conv2d(a, stream);
  return rc != DFL_OK ? rc : dfl_conv2d(b, stream);
}

extern "C" int dfl_conv2d(const dfl_conv_args* a, dfl_stream_t stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (a != nullptr && a->x_bf16) {
    DFL_REQUIRE(a->y_bf16, "dfl_conv2d: bf16 input with fp32 output is not a configuration of the network");
    DFL_REQUIRE(a->splits <= 1 || a->partial != nullptr, "dfl_conv2d: splits > 1 needs the partial buffer");
  }
  dfl::ConvRoute r;
  int rc = dfl::conv_route(a, a != nullptr && a->splits > 1 ? a->splits : 1, &r);
  if (rc != DFL_OK) return rc;
  dfl::ConvK& k = r.k;
  switch (r.form) {
    case dfl::FORM_BF16: return dfl::convp_launch(r.plan, s);
    case dfl::FORM_FIRST: return dfl::convs_first_launch(a, s);
    case dfl::FORM_LATENCY32: {
      DFL_REQUIRE(r.splits <= 1 || a->partial != nullptr, "dfl_conv2d: splits > 1 needs the partial buffer");
      rc = dfl::convs_launch(r.plan, s);
      if (rc != DFL_OK || r.splits <= 1) return rc;
      k.splits = r.splits;
      return dfl::conv_finish(k, s, "dfl_conv2d (latency form, split-K finish)");
    }
    default: break;
  }
  DFL_REQUIRE(a->out_scale == nullptr, "dfl_conv2d: out_scale / out_shift are implemented by the latency form only (dfl_conv_config tells)");
  DFL_REQUIRE(a->x_mode == 0 && a->x_out == nullptr, "dfl_conv2d: x_mode (fused BatchNorm + ReLU backward operand) and x_out are implemented by the bf16 patch kernels only");
  {
    // live statistics outside the bf16 patch kernels: the 1-channel direct kernels (3x3 row form: stat_totals; 1x1: add_tot) and,
    // round 5, the fp32-tensor GEMM kernels -- producer (stat_totals: plain statistics of the stored values), consumer of an input
    // (in_tot: the fast gather, whose scale / shift table lives in LDS) and of "+ BN(add)" (add_tot)
    const bool any = a->stat_totals != nullptr || a->in_tot != nullptr || a->add_tot != nullptr;
    const bool direct = any && r.form == dfl::FORM_DIRECT;
    const bool direct_ok = direct && a->in_tot == nullptr &&
                           (a->stat_totals == nullptr || (dfl::direct_conv_rows_usable(a) && a->stat_other == nullptr)) &&
                           (a->add_tot == nullptr || (a->add != nullptr && a->add_scale == nullptr && a->add_gamma && a->add_beta && a->add_count > 0 &&
                                                      !dfl::direct_conv_rows_usable(a)));
    DFL_REQUIRE(!direct || direct_ok, "dfl_conv2d: live BatchNorm statistics: this form is not implemented by the 1-channel direct kernels");
    if (any && !direct) {
      DFL_REQUIRE(a->x_mode == 0 && !a->scatter2x2 && (a->stat_totals == nullptr || (a->stat_other == nullptr && a->stat_partials == nullptr)),
                  "dfl_conv2d (fp32 tensors): stat_totals takes the plain statistics of a non-scatter layer");
      DFL_REQUIRE(a->in_tot == nullptr || (a->in_scale == nullptr && a->in_gamma && a->in_beta && a->in_count > 0 && a->Cin % 16 == 0 && !a->x_split),
                  "dfl_conv2d (fp32 tensors): in_tot replaces in_scale / in_shift, needs in_gamma, in_beta, in_count and the fast gather (Cin %% 16 == 0)");
      DFL_REQUIRE(a->add_tot == nullptr || (a->add != nullptr && a->add_scale == nullptr && a->add_gamma && a->add_beta && a->add_count > 0),
                  "dfl_conv2d (fp32 tensors): add_tot replaces add_scale / add_shift and needs add, add_gamma, add_beta, add_count");
    }
  }
  if (r.form == dfl::FORM_DIRECT) {
    DFL_REQUIRE(!a->w_split && !a->x_split, "dfl_conv2d: split operands are not defined for the direct small-K kernels");
    return dfl::direct_conv_launch(a, s);
  }
  DFL_REQUIRE(!a->y_bf16, "dfl_conv2d: bf16 output needs bf16 input (patch kernels) or a direct small-K layer");
  if (a->splits > 1) {
    DFL_REQUIRE(a->partial != nullptr, "dfl_conv2d: splits > 1 needs the partial buffer");
    const int nchunks = (int)dfl::ceil_div(k.Ktot, dfl::KC);
    DFL_REQUIRE(a->splits <= nchunks, "dfl_conv2d: more splits than K chunks");
    k.splits = a->splits;
    k.cps = (int)dfl::ceil_div(nchunks, a->splits);
  }
  if (a->w_split || a->x_split) {
    DFL_REQUIRE(k.fast && (dfl::math_mode() == 1 || dfl::math_mode() == 3),
                "dfl_conv2d: split operands need math mode 1 or 3 (bf16x3 / bf16) and the fast path (Cin %% 16 == 0, aligned, < 2 GiB)");
    DFL_REQUIRE(!a->x_split || a->in_scale == nullptr, "dfl_conv2d: a split input cannot take an affine on load");
  }
  const bool general = a->add != nullptr || a->accumulate || a->scatter2x2 || (a->stat_other != nullptr && !k.so_simple);
  const bool aff = a->in_scale != nullptr || a->in_tot != nullptr;
  DFL_REQUIRE(a->in_tot == nullptr || k.fast, "dfl_conv2d (fp32 tensors): in_tot needs the fast gather (aligned tensors below 2 GiB)");
  if (r.form == dfl::FORM_ROWS) {   // 3x3 layers in whole row segments (it checks the epilogue / slices it can take)
    rc = dfl::conv_rows_launch(k, s);
  } else if (!k.fast) {
    rc = dfl::launch<2, 2, 1, 1, 0, true, 1>(k, s);
  } else {
    switch (r.cfg) {
      case dfl::CFG_128x128: rc = dfl::launch_fast<2, 2, 2, 2>(k, aff, general, s); break;
      case dfl::CFG_128x64: rc = dfl::launch_fast<2, 2, 2, 1>(k, aff, general, s); break;
      case dfl::CFG_256x32: rc = dfl::launch_fast<4, 1, 2, 1>(k, aff, general, s); break;
      case dfl::CFG_64x64: rc = dfl::launch_fast<2, 2, 1, 1>(k, aff, general, s); break;   // (2-wave 64x64 variants measured 10 % slower)
      default: rc = dfl::launch_fast<1, 2, 1, 1>(k, aff, general, s); break;
    }
  }
  if (rc != DFL_OK || k.splits <= 1) return rc;
  return dfl::conv_finish(k, s, "dfl_conv2d (split-K finish)");
}
