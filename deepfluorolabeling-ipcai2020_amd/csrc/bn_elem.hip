// Streaming (HBM-bound) kernels around the convolutions, in the order of this file: per-channel statistics (colstats),
// BatchNorm finalize (forward, "live", eval, backward), BatchNorm + ReLU backward, partial-sum reductions (one and batched),
// affine copy, 2x2 max-pool, weight re-layout (pack), and the three optimizers (SGD, Adam, RMSprop; alone and fused with the
// re-layout).  The tensor kernels work on NHWC rows [M][C] and are written once over the channel unit of chan_unit.h:
// 8 bf16 channels, or 4 fp32 channels (float4) when C, ld and the pointers allow it, 1 fp32 channel otherwise.
// Reference behaviour: nn.BatchNorm2d (train_test_code/unet.py:215,222), nn.ReLU (:213,220), F.max_pool2d (:169),
// torch.optim.SGD (train.py:333-334), torch.optim.Adam / RMSprop (train.py:331-352).  Contracts: include/dfl_hip.h.
#include "chan_unit.h"

namespace dfl {

// ------------------------------------------------------------------------------------------------ helpers
// A workgroup of the row kernels (colstats, bn_relu_bwd): UX threads along the row x RY = 256 / UX row lanes; blockIdx.x = a
// block of rows, blockIdx.y = a block of UX units.
struct RowGeom {
  int UX;     // threads along the row (power of two <= 256)
  int gy;     // grid.y = ceil(units / UX)
};

static RowGeom row_geom(int C, int W) {
  const int units = C / W;
  RowGeom g;
  g.UX = 1;
  while (g.UX * 2 <= units && g.UX * 2 <= 256) g.UX *= 2;
  g.gy = (int)ceil_div(units, g.UX);
  return g;
}

static int rowblocks(int64_t M, int C) {
  int64_t nb = ceil_div(M * (int64_t)C, 8192);
  if (nb > 2048) nb = 2048;
  if (nb > M) nb = M;
  if (nb < 1) nb = 1;
  return (int)nb;
}

// this thread's place in such a workgroup: unit ux (first channel c, cok: inside the row), rows r0 + uy, + RY, ... < r1
struct RowLane {
  int ux, uy, RY, c;
  bool cok;
  int64_t r0, r1;
};

template <int W>
__device__ __forceinline__ RowLane row_lane(int UX, int rows_per_block, int64_t M, int C) {
  RowLane t;
  t.RY = 256 / UX;
  t.ux = threadIdx.x % UX;
  t.uy = threadIdx.x / UX;
  t.c = (blockIdx.y * UX + t.ux) * W;
  t.cok = t.c < C;
  t.r0 = (int64_t)blockIdx.x * rows_per_block;
  t.r1 = t.r0 + rows_per_block;
  if (t.r1 > M) t.r1 = M;
  return t;
}

// NS running sums per channel of every thread -> the workgroup's sums, out[n * C + j] for the unit's channel j: the threads
// of row lane 0 add the RY lanes up in lane order.  One barrier; every thread of the workgroup must call it.
template <int NS, int W>
__device__ __forceinline__ void block_colsum(const float (&s)[NS][W], const RowLane& t, int UX, float* out, int C) {
  __shared__ float red[NS][256][W];
#pragma unroll
  for (int n = 0; n < NS; ++n)
#pragma unroll
    for (int j = 0; j < W; ++j) red[n][threadIdx.x][j] = s[n][j];
  __syncthreads();
  if (t.uy == 0 && t.cok) {
#pragma unroll
    for (int n = 0; n < NS; ++n)
#pragma unroll
      for (int j = 0; j < W; ++j) {
        float sum = 0.f;
        for (int y = 0; y < t.RY; ++y) sum += red[n][y * UX + t.ux][j];
        out[(int64_t)n * C + j] = sum;
      }
  }
}

// ------------------------------------------------------------------------------------------------ colstats
// partials[blk][0][c] = sum a, partials[blk][1][c] = sum a*b over the block's rows (b == NULL: a*a).
template <int W, bool BF>
__global__ void __launch_bounds__(256) colstats_kernel(const dfl_colstats_args a, int UX, int rows_per_block) {
  using U = ChanUnit<W, BF>;
  const RowLane t = row_lane<W>(UX, rows_per_block, a.M, a.C);
  float s[2][W];
#pragma unroll
  for (int j = 0; j < W; ++j) s[0][j] = s[1][j] = 0.f;
  if (t.cok) {
    for (int64_t r = t.r0 + t.uy; r < t.r1; r += t.RY) {
      float va[W], vb[W];
      U::load(a.a, r * a.lda + t.c, va);
      if (a.b != nullptr) U::load(a.b, r * a.ldb + t.c, vb);
#pragma unroll
      for (int j = 0; j < W; ++j) {
        s[0][j] += va[j];
        s[1][j] = fmaf(va[j], a.b != nullptr ? vb[j] : va[j], s[1][j]);
      }
    }
  }
  block_colsum<2, W>(s, t, UX, a.partials + (int64_t)blockIdx.x * 2 * a.C + t.c, a.C);
}

// ------------------------------------------------------------------------------------------------ BN finalize
// One workgroup per `cpb` channels (8 for wide layers down to 1 for narrow ones, so that even a 32-channel layer with
// thousands of partial rows spreads over tens of workgroups): 256/cpb lanes walk the partial rows, fp64 tree over them.
__device__ __forceinline__ void sum_partials_f64(const float* __restrict__ partials, int nblocks, int C, int cpb,
                                                 double* out1, double* out2, double (*red)[256]) {
  const int cl = threadIdx.x % cpb, rl = threadIdx.x / cpb, lanes = 256 / cpb;
  const int c = blockIdx.x * cpb + cl;
  double s1 = 0.0, s2 = 0.0;
  if (c < C) {
    // four rows (eight loads) in flight per lane: these kernels are one memory round trip after the other, nothing else
    int r = rl;
    for (; r + 3 * lanes < nblocks; r += 4 * lanes) {
      float v1[4], v2[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        v1[u] = partials[((int64_t)(r + u * lanes) * 2 + 0) * C + c];
        v2[u] = partials[((int64_t)(r + u * lanes) * 2 + 1) * C + c];
      }
      s1 += ((double)v1[0] + (double)v1[1]) + ((double)v1[2] + (double)v1[3]);
      s2 += ((double)v2[0] + (double)v2[1]) + ((double)v2[2] + (double)v2[3]);
    }
    for (; r < nblocks; r += lanes) {
      s1 += (double)partials[((int64_t)r * 2 + 0) * C + c];
      s2 += (double)partials[((int64_t)r * 2 + 1) * C + c];
    }
  }
  // lanes of one channel inside a wave (lane = row lane * cpb + channel: xor offsets >= cpb keep the channel), then the four waves
  for (int off = 32; off >= cpb; off >>= 1) {
    s1 += __shfl_xor(s1, off, 64);
    s2 += __shfl_xor(s2, off, 64);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane < cpb) {
    red[0][wave * 8 + lane] = s1;
    red[1][wave * 8 + lane] = s2;
  }
  __syncthreads();
  *out1 = (red[0][cl] + red[0][8 + cl]) + (red[0][16 + cl] + red[0][24 + cl]);
  *out2 = (red[1][cl] + red[1][8 + cl]) + (red[1][16 + cl] + red[1][24 + cl]);
}

static inline int finalize_cpb(int C) { return C >= 512 ? 8 : (C >= 256 ? 4 : (C >= 128 ? 2 : 1)); }

__global__ void __launch_bounds__(256) bn_finalize_kernel(const dfl_bn_finalize_args a, int cpb) {
  __shared__ double red[2][256];
  const int c = blockIdx.x * cpb + (threadIdx.x % cpb);
  double s1, s2;
  sum_partials_f64(a.partials, a.nblocks, a.C, cpb, &s1, &s2, red);
  if (threadIdx.x < cpb && c < a.C) {
    const double cnt = (double)a.count;
    const double mean = s1 / cnt;
    double var = s2 / cnt - mean * mean;  // biased variance used for normalisation
    if (var < 0.0) var = 0.0;
    const double invstd = 1.0 / sqrt(var + (double)a.eps);
    const float scale = (float)((double)a.gamma[c] * invstd);
    a.scale[c] = scale;
    a.shift[c] = (float)((double)a.beta[c] - mean * (double)a.gamma[c] * invstd);
    a.save_mean[c] = (float)mean;
    a.save_invstd[c] = (float)invstd;
    if (a.running_mean != nullptr) {
      const double mom = (double)a.momentum;
      const double unbiased = (cnt > 1.0) ? var * cnt / (cnt - 1.0) : var;
      a.running_mean[c] = (float)((1.0 - mom) * (double)a.running_mean[c] + mom * mean);
      a.running_var[c] = (float)((1.0 - mom) * (double)a.running_var[c] + mom * unbiased);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && a.num_batches_tracked != nullptr) *a.num_batches_tracked += 1;
}

// All "live" BatchNorm layers of a forward pass in one launch (dfl_bn_finalize_live): blockIdx.y = layer, a thread = a channel.
__global__ void __launch_bounds__(256) bn_finalize_live_kernel(const dfl_bn_live_job* __restrict__ jobs) {
  const dfl_bn_live_job j = jobs[blockIdx.y];
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < j.C) {
    float scale, shift;
    double mean, var;
    bn_live_affine(j.totals, j.gamma, j.beta, (double)j.count, j.eps, j.C, c, &scale, &shift, &mean, &var);
    j.scale[c] = scale;
    j.shift[c] = shift;
    j.save_mean[c] = (float)mean;
    j.save_invstd[c] = (float)(1.0 / sqrt(var + (double)j.eps));
    if (j.running_mean != nullptr) {
      const double mom = (double)j.momentum, cnt = (double)j.count;
      const double unbiased = (cnt > 1.0) ? var * cnt / (cnt - 1.0) : var;
      j.running_mean[c] = (float)((1.0 - mom) * (double)j.running_mean[c] + mom * mean);
      j.running_var[c] = (float)((1.0 - mom) * (double)j.running_var[c] + mom * unbiased);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && j.num_batches_tracked != nullptr) *j.num_batches_tracked += 1;
}

__global__ void __launch_bounds__(256) bn_bwd_finalize_live_kernel(const dfl_bn_bwd_live_job* __restrict__ jobs) {
  const dfl_bn_bwd_live_job j = jobs[blockIdx.y];
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= j.C) return;
  double sdy = 0.0, sdyr = 0.0;
#pragma unroll
  for (int r = 0; r < DFL_BN_R; ++r) {
    sdy += j.totals[(int64_t)(r * 2 + 0) * j.C + c];
    sdyr += j.totals[(int64_t)(r * 2 + 1) * j.C + c];
  }
  const double mean = (double)j.save_mean[c], invstd = (double)j.save_invstd[c];
  j.dgamma[c] = (float)(invstd * (sdyr - mean * sdy));
  j.dbeta[c] = (float)sdy;
  if (j.sum_out != nullptr) j.sum_out[c] = (float)sdy;
}

__global__ void bn_eval_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                               const float* __restrict__ rm, const float* __restrict__ rv, float* __restrict__ scale,
                               float* __restrict__ shift, int C, float eps) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) {
    const float invstd = 1.0f / sqrtf(rv[c] + eps);
    const float s = gamma[c] * invstd;
    scale[c] = s;
    shift[c] = beta[c] - rm[c] * s;
  }
}

// dy-side finalize: dgamma, dbeta and the affine form of BatchNorm+ReLU backward.
__global__ void __launch_bounds__(256) bn_bwd_finalize_kernel(const dfl_bn_bwd_finalize_args a, int cpb) {
  __shared__ double red[2][256];
  const int c = blockIdx.x * cpb + (threadIdx.x % cpb);
  double sdy, sdyr;
  sum_partials_f64(a.partials, a.nblocks, a.C, cpb, &sdy, &sdyr, red);
  if (threadIdx.x < cpb && c < a.C) {
    const double cnt = (double)a.count;
    const double mean = (double)a.save_mean[c], invstd = (double)a.save_invstd[c], g = (double)a.gamma[c];
    const double sdyx = invstd * (sdyr - mean * sdy);  // sum dy * xhat
    a.dgamma[c] = (float)sdyx;
    a.dbeta[c] = (float)sdy;
    const double s = g * invstd;
    // count == 0: the statistics were constants (eval mode, running mean / variance): no batch-mean terms
    const double c1 = a.count > 0 ? sdy / cnt : 0.0, c2 = a.count > 0 ? sdyx / cnt : 0.0;
    // dr = s*(dy - c1 - xhat*c2),  xhat = (r - mean)*invstd
    a.coef[0 * a.C + c] = (float)s;
    a.coef[1 * a.C + c] = (float)(-s * c2 * invstd);
    a.coef[2 * a.C + c] = (float)(-s * c1 + s * c2 * invstd * mean);
  }
}

// dpre = [r > 0] * (A*dy + B*r + C); partials[blk][c] = column sums of dpre, of the values as stored.
template <int W, bool BF>
__global__ void __launch_bounds__(256) bn_relu_bwd_kernel(const dfl_bn_relu_bwd_args a, int UX, int rows_per_block) {
  using U = ChanUnit<W, BF>;
  const RowLane t = row_lane<W>(UX, rows_per_block, a.M, a.C);
  const int C = a.C, c = t.c, RY = t.RY;
  float cA[W], cB[W], cC[W], s[1][W];
#pragma unroll
  for (int j = 0; j < W; ++j) {
    cA[j] = 1.f; cB[j] = 0.f; cC[j] = 0.f; s[0][j] = 0.f;
    if (a.coef != nullptr && t.cok) {
      cA[j] = a.coef[c + j];
      cB[j] = a.coef[C + c + j];
      cC[j] = a.coef[2 * C + c + j];
    }
  }
  if (t.cok) {
    auto one = [&](const float* dy, const float* rv, int64_t r) {
      float o[W];
#pragma unroll
      for (int j = 0; j < W; ++j) o[j] = rv[j] > 0.f ? fmaf(cA[j], dy[j], fmaf(cB[j], rv[j], cC[j])) : 0.f;
      if (W == 4 && a.split_out) {
        // split_out exists for the float4 form only (the launcher refuses it elsewhere): hi4 | lo4 bf16 in the float4's
        // slot (consumers: split-bf16 GEMMs only); the sums are taken from the fp32 values
        if constexpr (W == 4) {
          uint2 parts[2];
          split_bf16<2>(make_float4(o[0], o[1], o[2], o[3]), parts);
          *reinterpret_cast<uint4*>(a.dpre + r * a.ldo + c) = make_uint4(parts[0].x, parts[0].y, parts[1].x, parts[1].y);
        }
      } else {
        U::store(a.dpre, r * a.ldo + c, o, o);
      }
#pragma unroll
      for (int j = 0; j < W; ++j) s[0][j] += o[j];
    };
    // rows in flight per thread: four, but two in the float4 form, where four take it past 64 registers (8 -> 5 waves per SIMD;
    // the bf16 form is at 3 waves with or without them).  The rows are taken in row order whatever R is.
    constexpr int R = (W == 4) ? 2 : 4;
    int64_t r = t.r0 + t.uy;
    for (; r + (R - 1) * RY < t.r1; r += R * RY) {
      float dy[R][W], rv[R][W];
#pragma unroll
      for (int u = 0; u < R; ++u) U::load(a.dy, (r + u * RY) * a.lddy + c, dy[u]);
#pragma unroll
      for (int u = 0; u < R; ++u) U::load(a.r, (r + u * RY) * a.ldr + c, rv[u]);
#pragma unroll
      for (int u = 0; u < R; ++u) one(dy[u], rv[u], r + u * RY);
    }
    for (; r < t.r1; r += RY) {
      float dy[W], rv[W];
      U::load(a.dy, r * a.lddy + c, dy);
      U::load(a.r, r * a.ldr + c, rv);
      one(dy, rv, r);
    }
  }
  if (a.partials == nullptr) return;
  block_colsum<1, W>(s, t, UX, a.partials + (int64_t)blockIdx.x * C + c, C);
}

// out[c] = sum_b partials[b*stride + c] in fp64
__global__ void __launch_bounds__(256) reduce_partials_kernel(const float* __restrict__ partials, float* __restrict__ out,
                                                             int nblocks, int stride, int C) {
  __shared__ double red[256];
  const int cl = threadIdx.x & 7, rl = threadIdx.x >> 3;
  const int c = blockIdx.x * 8 + cl;
  double s = 0.0;
  if (c < C)
    for (int r = rl; r < nblocks; r += 32) s += (double)partials[(int64_t)r * stride + c];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int off = 16; off >= 1; off >>= 1) {
    if (rl < off) red[threadIdx.x] += red[threadIdx.x + off * 8];
    __syncthreads();
  }
  if (threadIdx.x < 8 && c < C) out[c] = (float)red[threadIdx.x];
}

// Batched sums (dfl_reduce_batch): blockIdx.x -> (job, block of the job) by binary search over the job table.
// A thread owns 4 consecutive outputs and reads them as one float4 per slice (n % 4 == 0 and 16-byte aligned rows: every
// weight-gradient and bias job; otherwise four scalar loads), four slices in flight, fp64 accumulation in a fixed order.
// Many slices (count >= 32): a workgroup takes 32 outputs (one 128-byte line per slice) x 32 slice lanes, eight slices of a
// lane in flight, and adds the lanes up through LDS.  Few slices: 1024 outputs per workgroup, the slices walked in order.
#ifndef DFL_RB_O
#define DFL_RB_O 32
#endif
constexpr int RB_T = 256, RB_O = DFL_RB_O, RB_S = 4 * RB_T / RB_O, RB_WIDE_MIN = 32;
static inline int reduce_job_blocks(int64_t n, int count) {
  return (int)(count >= RB_WIDE_MIN ? ceil_div(n, RB_O) : ceil_div(n, 4 * RB_T));
}

__device__ __forceinline__ void rb_load4(const float* __restrict__ p, int64_t i, int64_t n, bool vec, double* a) {
  if (vec) {
    const float4 v = *reinterpret_cast<const float4*>(p + i);
    a[0] += (double)v.x; a[1] += (double)v.y; a[2] += (double)v.z; a[3] += (double)v.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (i + e < n) a[e] += (double)p[i + e];
  }
}

__device__ __forceinline__ void rb_store4(const dfl_reduce_job& j, int64_t i, const double* v) {
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (i + e < j.n) {
      const int64_t ii = i + e;
      j.dst[j.T > 1 ? (ii % (j.n / j.T)) * j.T + ii / (j.n / j.T) : ii] = (float)v[e];
    }
}

__global__ void __launch_bounds__(RB_T) reduce_batch_kernel(const dfl_reduce_job* __restrict__ jobs, int njobs) {
  __shared__ double red[RB_S][RB_O + 2];
  int lo = 0, hi = njobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].first_block <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const dfl_reduce_job j = jobs[lo];
  const int b = (int)blockIdx.x - j.first_block;
  const bool vec = (j.n & 3) == 0 && (j.stride & 3) == 0 && (reinterpret_cast<uintptr_t>(j.src) & 15) == 0;
  if (j.count >= RB_WIDE_MIN) {
    const int o4 = threadIdx.x % (RB_O / 4), sl = threadIdx.x / (RB_O / 4);
    const int64_t i = (int64_t)b * RB_O + 4 * o4;
    double a0[4] = {0, 0, 0, 0}, a1[4] = {0, 0, 0, 0}, a2[4] = {0, 0, 0, 0}, a3[4] = {0, 0, 0, 0};
    if (i < j.n) {
      int k = sl;
      if (vec) {
        for (; k + 7 * RB_S < j.count; k += 8 * RB_S) {      // eight 16-byte loads in flight
          float4 v[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(j.src + (int64_t)(k + u * RB_S) * j.stride + i);
#pragma unroll
          for (int u = 0; u < 8; u += 4) {
            a0[0] += (double)v[u].x; a0[1] += (double)v[u].y; a0[2] += (double)v[u].z; a0[3] += (double)v[u].w;
            a1[0] += (double)v[u + 1].x; a1[1] += (double)v[u + 1].y; a1[2] += (double)v[u + 1].z; a1[3] += (double)v[u + 1].w;
            a2[0] += (double)v[u + 2].x; a2[1] += (double)v[u + 2].y; a2[2] += (double)v[u + 2].z; a2[3] += (double)v[u + 2].w;
            a3[0] += (double)v[u + 3].x; a3[1] += (double)v[u + 3].y; a3[2] += (double)v[u + 3].z; a3[3] += (double)v[u + 3].w;
          }
        }
      }
      for (; k + 3 * RB_S < j.count; k += 4 * RB_S) {
        rb_load4(j.src + (int64_t)k * j.stride, i, j.n, vec, a0);
        rb_load4(j.src + (int64_t)(k + RB_S) * j.stride, i, j.n, vec, a1);
        rb_load4(j.src + (int64_t)(k + 2 * RB_S) * j.stride, i, j.n, vec, a2);
        rb_load4(j.src + (int64_t)(k + 3 * RB_S) * j.stride, i, j.n, vec, a3);
      }
      for (; k < j.count; k += RB_S) rb_load4(j.src + (int64_t)k * j.stride, i, j.n, vec, a0);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) red[sl][4 * o4 + e] = (a0[e] + a1[e]) + (a2[e] + a3[e]);
    __syncthreads();
    for (int off = RB_S / 2; off >= 1; off >>= 1) {
      if (sl < off) {
#pragma unroll
        for (int e = 0; e < 4; ++e) red[sl][4 * o4 + e] += red[sl + off][4 * o4 + e];
      }
      __syncthreads();
    }
    if (sl == 0 && i < j.n) rb_store4(j, i, &red[0][4 * o4]);
  } else {
    const int64_t i = ((int64_t)b * RB_T + threadIdx.x) * 4;
    if (i < j.n) {
      double s[4] = {0, 0, 0, 0};
      for (int k = 0; k < j.count; ++k) rb_load4(j.src + (int64_t)k * j.stride, i, j.n, vec, s);
      rb_store4(j, i, s);
    }
  }
}

// ------------------------------------------------------------------------------------------------ affine copy
// y window = x window (* scale + shift per channel) (+ y window); a thread per (pixel, unit), grid-stride
template <int W, bool BF>
__global__ void __launch_bounds__(256) affine_copy_kernel(const dfl_affine_copy_args a, int64_t total_units, int cq) {
  using U = ChanUnit<W, BF>;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total_units; i += stride) {
    int u, xw, yh, n;
    unit_coords(i, cq, a.W, a.H, &u, &xw, &yh, &n);
    const int c = u * W;
    const int64_t so = (((int64_t)n * a.xH + a.xoy + yh) * a.xW + a.xox + xw) * a.ldx + c;
    const int64_t dof = (((int64_t)n * a.yH + a.yoy + yh) * a.yW + a.yox + xw) * a.ldy + c;
    float v[W];
    U::load(a.x, so, v);
    if (a.scale != nullptr) {
      float sc[W], sh[W];
      if constexpr (W == 4) {   // fp32 scale / shift as one float4 each in the float4 form only: the launcher asks for
        ChanUnit<4, false>::load(a.scale, c, sc);   // their 16-byte alignment there and nowhere else
        ChanUnit<4, false>::load(a.shift, c, sh);
      } else {
#pragma unroll
        for (int j = 0; j < W; ++j) { sc[j] = a.scale[c + j]; sh[j] = a.shift[c + j]; }
      }
#pragma unroll
      for (int j = 0; j < W; ++j) v[j] = fmaf(v[j], sc[j], sh[j]);
    }
    if (a.accumulate) {
      float o[W];
      U::load(a.y, dof, o);
#pragma unroll
      for (int j = 0; j < W; ++j) v[j] += o[j];
    }
    U::store(a.y, dof, v);
  }
}

// ------------------------------------------------------------------------------------------------ max pool
// the four inputs of output pixel (n, oy, ox): element offsets of the first (pixel stride ld, row stride W * ld)
__device__ __forceinline__ int64_t pool_src(const dfl_pool_args& a, int n, int oy, int ox, int ld) {
  return (((int64_t)n * a.H + 2 * oy) * a.W + 2 * ox) * ld;
}

template <int W, bool BF>
__global__ void __launch_bounds__(256) maxpool_fwd_kernel(const dfl_pool_args a, int64_t total_units, int cq) {
  using U = ChanUnit<W, BF>;
  const int Ho = a.H / 2, Wo = a.W / 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total_units; i += stride) {
    int u, ox, oy, n;
    unit_coords(i, cq, Wo, Ho, &u, &ox, &oy, &n);
    const int c = u * W;
    const int64_t s00 = pool_src(a, n, oy, ox, a.ldx) + c, s10 = s00 + (int64_t)a.W * a.ldx;
    float v0[W], v1[W], v2[W], v3[W], m[W];
    U::load(a.x, s00, v0);
    U::load(a.x, s00 + a.ldx, v1);
    U::load(a.x, s10, v2);
    U::load(a.x, s10 + a.ldx, v3);
#pragma unroll
    for (int j = 0; j < W; ++j) m[j] = fmaxf(fmaxf(v0[j], v1[j]), fmaxf(v2[j], v3[j]));
    U::store(a.y, (((int64_t)n * Ho + oy) * Wo + ox) * a.ldy + c, m);
  }
}

__device__ __forceinline__ int first_max4(float v0, float v1, float v2, float v3) {
  int k = 0;
  float m = v0;
  if (v1 > m) { m = v1; k = 1; }
  if (v2 > m) { m = v2; k = 2; }
  if (v3 > m) { k = 3; }
  return k;
}

// dx += the gradient y at the first maximum of each 2x2 window of x
template <int W, bool BF>
__global__ void __launch_bounds__(256) maxpool_bwd_kernel(const dfl_pool_args a, int64_t total_units, int cq) {
  using U = ChanUnit<W, BF>;
  const int Ho = a.H / 2, Wo = a.W / 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total_units; i += stride) {
    int u, ox, oy, n;
    unit_coords(i, cq, Wo, Ho, &u, &ox, &oy, &n);
    const int c = u * W;
    const int64_t s00 = pool_src(a, n, oy, ox, a.ldx) + c, s10 = s00 + (int64_t)a.W * a.ldx;
    const int64_t d00 = pool_src(a, n, oy, ox, a.lddx) + c, d10 = d00 + (int64_t)a.W * a.lddx;
    float v0[W], v1[W], v2[W], v3[W], g[W];
    U::load(a.x, s00, v0);
    U::load(a.x, s00 + a.ldx, v1);
    U::load(a.x, s10, v2);
    U::load(a.x, s10 + a.ldx, v3);
    U::load(a.y, (((int64_t)n * Ho + oy) * Wo + ox) * a.ldy + c, g);
    if constexpr (BF) {
      // bf16: a 2-byte read-modify-write per winner would be slow, so all four 16-byte units of dx are rewritten, the
      // losers with + 0 (which is the identity on every bf16 value but -0.0: hence not the fp32 way below)
      float e0[W], e1[W], e2[W], e3[W];
      U::load(a.dx, d00, e0);
      U::load(a.dx, d00 + a.lddx, e1);
      U::load(a.dx, d10, e2);
      U::load(a.dx, d10 + a.lddx, e3);
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const int k = first_max4(v0[j], v1[j], v2[j], v3[j]);
        e0[j] += k == 0 ? g[j] : 0.f;
        e1[j] += k == 1 ? g[j] : 0.f;
        e2[j] += k == 2 ? g[j] : 0.f;
        e3[j] += k == 3 ? g[j] : 0.f;
      }
      U::store(a.dx, d00, e0);
      U::store(a.dx, d00 + a.lddx, e1);
      U::store(a.dx, d10, e2);
      U::store(a.dx, d10 + a.lddx, e3);
    } else {
      // fp32: only the winning pixel of each channel is touched (the other three keep their bits, a -0.0 included)
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const int k = first_max4(v0[j], v1[j], v2[j], v3[j]);
        a.dx[(k < 2 ? d00 : d10) + ((k & 1) ? a.lddx : 0) + j] += g[j];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ weight pack
// GEMM operand layout of dfl_conv2d: w[kq][n][r] = W(k = 4*kq + r, n), zero for k >= K ("quad-packed": one float4 is four
// consecutive k of one output column).  The source is always a contiguous [A][B][C] parameter (C = KH*KW) and the
// (k, n) <-> (a, b, c) mapping is one of three kinds (include/dfl_hip.h).  Fast path: LDS-tiled -- a 32(A) x 32(B) x C
// tile is read as 32 runs of 32*C contiguous floats and one emitter per format (pack_emit_cells, pack_emit_quads) writes it
// as 512-byte runs; element-wise fallback (pack_src) otherwise.
constexpr int PK_T = 32, PK_CMAX = 9;
using PackTile = float[PK_T][PK_T * PK_CMAX + 1];

// K x N of the matrix a job of this kind builds
struct PackDims { int K, N; };
__device__ __forceinline__ PackDims pack_dims(int kind, int A, int B, int C) {
  return {(kind == 1) ? C * B : (kind == 2 ? C * A : A), (kind == 1) ? A : (kind == 2 ? B : C * B)};
}

__device__ __forceinline__ float pack_src(const dfl_pack_job& j, int k, int n) {
  int a, b, c;
  if (j.kind == 1) {
    c = k / j.B; b = k - c * j.B; a = n;
  } else if (j.kind == 2) {
    const int cp = k / j.A;
    a = k - cp * j.A; b = n; c = j.flip ? (j.C - 1 - cp) : cp;
  } else {
    a = k; c = n / j.B; b = n - c * j.B;
  }
  return j.src[((int64_t)a * j.B + b) * j.C + c];
}

// element r of quad slot q: a float, or (split format) hi bf16 at half-word r and lo bf16 at half-word 4 + r of the slot
// (the bf16 chunk layout, split = 2, is written cell by cell: pack_emit_cells and pack_kernel's element-wise cells)
__device__ __forceinline__ void pack_put(float* dst, int64_t q, int r, float v, int split) {
  if (!split) {
    dst[q * 4 + r] = v;
  } else {
    const __bf16 h = (__bf16)v;
    const __bf16 l = (__bf16)(v - (float)h);
    unsigned short* d16 = reinterpret_cast<unsigned short*>(dst) + q * 8;
    d16[r] = __builtin_bit_cast(unsigned short, h);
    d16[4 + r] = __builtin_bit_cast(unsigned short, l);
  }
}

// ---- a tile in LDS becomes a layout: the only two places that know the index maps of the tiled path.  (a0, b0) is the tile's
// corner in the parameter, na x nb its extent: 32 x 32 in pack_tile, where the edge guards fold away after inlining (x, 16 * blk,
// ar and bb are below 32 by construction); the last tiles of pack_kernel are smaller.
// bf16 chunk layout [K/16][N][16]: a thread builds whole cells (16 consecutive k of one column = 32 bytes) and consecutive threads
// take consecutive columns: coalesced on both sides.  The k-run channel count is a multiple of 16 here, so a block of 16 k inside
// the extent is whole.
__device__ __forceinline__ void pack_emit_cells(const PackTile& tile, unsigned short* dst16, int kind, int flip, int A, int B, int Cc,
                                                int a0, int b0, int na, int nb) {
  const int N = pack_dims(kind, A, B, Cc).N;
  const int nx = (kind == 1) ? na : nb, nk = (kind == 1) ? nb : na;   // extent along the columns and along the k run
  for (int e = threadIdx.x; e < 64 * Cc; e += 256) {           // cells of this tile: 32 columns x 2 blocks of 16 k x C taps
    const int x = e & 31, blk = (e >> 5) & 1, cp = e >> 6;
    if (x >= nx || 16 * blk >= nk) continue;
    float f[16];
    int64_t cell;
    if (kind == 1) {                // k = c*B + b (16 consecutive b), n = a
#pragma unroll
      for (int r = 0; r < 16; ++r) f[r] = tile[x][(16 * blk + r) * Cc + cp];
      cell = (int64_t)((cp * B + b0) / 16 + blk) * N + a0 + x;
    } else if (kind == 2) {         // k = c'*A + a (16 consecutive a), n = b
      const int c = flip ? (Cc - 1 - cp) : cp;
#pragma unroll
      for (int r = 0; r < 16; ++r) f[r] = tile[16 * blk + r][x * Cc + c];
      cell = (int64_t)((cp * A + a0) / 16 + blk) * N + b0 + x;
    } else {                        // k = a (16 consecutive a), n = c*B + b
#pragma unroll
      for (int r = 0; r < 16; ++r) f[r] = tile[16 * blk + r][x * Cc + cp];
      cell = (int64_t)(a0 / 16 + blk) * N + cp * B + b0 + x;
    }
    u32x4* d = reinterpret_cast<u32x4*>(dst16 + cell * 16);
    d[0] = pack8(f);
    d[1] = pack8(f + 8);
  }
}

// the quad layouts (4 floats, or 4 hi | 4 lo bf16: pack_put): the k-run channel count is a multiple of 4 here
__device__ __forceinline__ void pack_emit_quads(const PackTile& tile, float* dst, int kind, int flip, int split, int A, int B, int Cc,
                                                int a0, int b0, int na, int nb) {
  const int N = pack_dims(kind, A, B, Cc).N;
  for (int e = threadIdx.x; e < PK_T * PK_T * Cc; e += 256) {
    const int r = e & 3, x = (e >> 2) & 31, rest = e >> 7;     // rest in [0, 8*C): tap, and quad of the tile's 8 along the k run
    if (kind == 1) {                // k = c*B + b, n = a: quads run along b, columns along a
      const int c = rest >> 3, bq = rest & 7, bb = 4 * bq + r, ar = x;
      if (ar < na && bb < nb) pack_put(dst, (int64_t)((c * B + b0) / 4 + bq) * N + a0 + ar, r, tile[ar][bb * Cc + c], split);
    } else if (kind == 2) {         // k = c'*A + a, n = b: quads along a, columns along b
      const int cp = rest >> 3, aq = rest & 7, ar = 4 * aq + r, bb = x;
      const int c = flip ? (Cc - 1 - cp) : cp;
      if (ar < na && bb < nb) pack_put(dst, (int64_t)((cp * A + a0) / 4 + aq) * N + b0 + bb, r, tile[ar][bb * Cc + c], split);
    } else {                        // k = a, n = c*B + b
      const int c = rest >> 3, aq = rest & 7, ar = 4 * aq + r, bb = x;
      if (ar < na && bb < nb) pack_put(dst, (int64_t)(a0 / 4 + aq) * N + c * B + b0 + bb, r, tile[ar][bb * Cc + c], split);
    }
  }
}

__device__ __forceinline__ void pack_emit(const PackTile& tile, float* dst, int kind, int flip, int split, int A, int B, int Cc, int a0,
                                          int b0, int na, int nb) {
  if (split == 2) pack_emit_cells(tile, reinterpret_cast<unsigned short*>(dst), kind, flip, A, B, Cc, a0, b0, na, nb);
  else pack_emit_quads(tile, dst, kind, flip, split, A, B, Cc, a0, b0, na, nb);
}

// dfl_pack_weights: a (tiles, jobs) grid; a job that tiles walks its 32 x 32 x C tiles (the last ones smaller), any other one
// goes element by element
__global__ void __launch_bounds__(256) pack_kernel(const dfl_pack_job* __restrict__ jobs) {
  __shared__ PackTile tile;
  const dfl_pack_job j = jobs[blockIdx.y];
  const int A = j.A, B = j.B, Cc = j.C;
  const PackDims dims = pack_dims(j.kind, A, B, Cc);
  const int K = dims.K, N = dims.N;
  // tileable: the taps fit the LDS tile and the k-run channel count (B for kind 1, A for kinds 2 and 3) fills whole cells / quads
  if (Cc <= PK_CMAX && (((j.kind == 1) ? B : A) & (j.split == 2 ? 15 : 3)) == 0) {
    const int tb = (B + PK_T - 1) / PK_T, ta = (A + PK_T - 1) / PK_T;
    const int run = PK_T * Cc;
    for (int tidx = blockIdx.x; tidx < ta * tb; tidx += gridDim.x) {
      const int a0 = (tidx / tb) * PK_T, b0 = (tidx % tb) * PK_T;
      const int nb = min(PK_T, B - b0), na = min(PK_T, A - a0);
      __syncthreads();                                         // the previous tile has been emitted
      for (int e = threadIdx.x; e < PK_T * run; e += 256) {    // 32 rows of 32*C contiguous source floats
        const int ar = e / run, q = e - ar * run;
        if (ar < na && q < nb * Cc) tile[ar][q] = j.src[((int64_t)(a0 + ar) * B + b0) * Cc + q];
      }
      __syncthreads();
      pack_emit(tile, j.dst, j.kind, j.flip, j.split, A, B, Cc, a0, b0, na, nb);
    }
    return;
  }
  if (j.split == 2) {
    // bf16 chunk layout [ceil(K/16)][N][16]: thread = one (chunk, column) cell of 32 bytes; consecutive threads take
    // consecutive columns (coalesced 32-byte stores; the sources are small enough to live in L2)
    const int Kc = (K + 15) / 16;
    const int64_t cells = (int64_t)Kc * N;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += stride) {
      const int n = (int)(i % N), kc = (int)(i / N);
      float f[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = kc * 16 + r;
        f[r] = k < K ? pack_src(j, k, n) : 0.f;
      }
      u32x4* d = reinterpret_cast<u32x4*>(reinterpret_cast<unsigned short*>(j.dst) + i * 16);
      d[0] = pack8(f);
      d[1] = pack8(f + 8);
    }
    return;
  }
  const int Kq = (K + 3) / 4;
  const int64_t total = (int64_t)Kq * N * 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int r = (int)(i & 3);
    const int64_t t = i >> 2;
    const int n = (int)(t % N), kq = (int)(t / N);
    const int k = 4 * kq + r;
    pack_put(j.dst, i >> 2, r, (k < K) ? pack_src(j, k, n) : 0.f, j.split);
  }
}

// ------------------------------------------------------------------------------------------------ optimizer update rules
// One element's update: p = r(w, g, &s1, &s2), the rule's state streams read before and written back after; has1() / has2()
// say which of them exist (the others are neither loaded nor stored).  PackOnly: the re-layout alone, nothing read but the master.
struct PackOnly {
  __device__ bool has1() const { return false; }
  __device__ bool has2() const { return false; }
  __device__ float operator()(float w, float, float*, float*) const { return w; }
};

// torch.optim.SGD: state 1 = momentum buffer (only when momentum != 0); first: buf = g, torch's first step (dfl_sgd_step only)
struct SgdRule {
  float lr, mom, wd, gscale;
  int nesterov, first;
  __device__ bool has1() const { return mom != 0.f; }
  __device__ bool has2() const { return false; }
  __device__ __forceinline__ float operator()(float w, float gr, float* b, float*) const {
    float g = fmaf(wd, w, gr * gscale);
    if (mom != 0.f) {
      const float nb = first ? g : fmaf(mom, *b, g);
      *b = nb;
      g = nesterov ? fmaf(mom, nb, g) : nb;
    }
    return fmaf(-lr, g, w);
  }
};

// torch's _multi_tensor_adam / _multi_tensor_rmsprop (the reference's --optim adam|rmsprop, train.py:331-352) one foreach op at
// a time, in torch's order, each result rounded to fp32.  No contraction into FMAs: the flat kernel and the tiled one then give
// the same bits whatever the compiler schedules around the inlined rule.  The (1 - beta) factors are formed in double on the host.
struct AdamRule {
  float eps, wd, gscale, beta2, step_size, bc2_sqrt, w1, omb2;   // w1 = 1 - beta1 (the lerp weight), omb2 = 1 - beta2
  __device__ bool has1() const { return true; }
  __device__ bool has2() const { return true; }
  __device__ __forceinline__ float operator()(float w, float gr, float* m, float* v) const {
#pragma clang fp contract(off)
    const float g = gr * gscale + wd * w;                      // _foreach_add(grads, params, alpha=wd)
    const float d = g - *m;                                    // _foreach_lerp_(exp_avgs, grads, 1 - beta1): at::lerp
    *m = (fabsf(w1) < 0.5f) ? *m + w1 * d : g - d * (1.f - w1);
    *v = *v * beta2 + (omb2 * g) * g;                          // _foreach_mul_(beta2); _foreach_addcmul_(g, g, 1 - beta2)
    const float den = sqrtf(*v) / bc2_sqrt + eps;              // sqrt; _foreach_div_(bc2_sqrt); _foreach_add_(eps)
    return w - step_size * (*m / den);                         // _foreach_addcdiv_(params, exp_avgs, den, -step_size)
  }
};

// state 1 = square_avg, state 2 = momentum buffer (only when momentum != 0)
struct RmspropRule {
  float eps, wd, gscale, alpha, oma, lr, mom;                  // oma = 1 - alpha
  __device__ bool has1() const { return true; }
  __device__ bool has2() const { return mom != 0.f; }
  __device__ __forceinline__ float operator()(float w, float gr, float* sq, float* buf) const {
#pragma clang fp contract(off)
    const bool hasb = has2();
    const float g = gr * gscale + wd * w;                      // _foreach_add(grads, params, alpha=wd)
    *sq = *sq * alpha + (oma * g) * g;                         // _foreach_mul_(alpha); _foreach_addcmul_(g, g, 1 - alpha)
    const float avg = sqrtf(*sq) + eps;
    if (hasb) {
      *buf = *buf * mom + g / avg;                             // _foreach_mul_(momentum); _foreach_addcdiv_(buf, g, avg)
      return w + -lr * *buf;                                   // _foreach_add_(params, buf, alpha=-lr)
    }
    return w + -lr * (g / avg);                                // _foreach_addcdiv_(params, g, avg, -lr)
  }
};

// dfl_sgd_step, dfl_adam_step, dfl_rmsprop_step: a flat arena, 4-byte accesses
template <class Rule>
__global__ void __launch_bounds__(256) optim_kernel(float* __restrict__ p, const float* __restrict__ grad, float* __restrict__ s1,
                                                   float* __restrict__ s2, int64_t n, Rule r) {
  const bool has1 = r.has1(), has2 = r.has2();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float a = has1 ? s1[i] : 0.f, b = has2 ? s2[i] : 0.f;
    p[i] = r(p[i], grad[i], &a, &b);
    if (has1) s1[i] = a;
    if (has2) s2[i] = b;
  }
}

// One workgroup of the tiled re-layout (a flat list of the full 32 x 32 x C tiles of ALL jobs of the launch: no idle workgroups for
// the small layers, and both layouts of a parameter -- forward and data-gradient operand -- from one read of the master): finds
// its job, updates its 32 x 32 x C tile of the fp32 master with 16-byte accesses to
// the master, the gradient and the rule's state arenas (all at the master's offsets plus a delta, in elements), and emits the
// tile's layouts from LDS -- the weights are read once per step, and the update costs no launch of its own.  A DFL_PACK_PLAIN job
// (something without a tiled layout) updates DFL_SGD_PLAIN_TILE elements as optim_kernel does, and emits nothing.
template <class Rule>
__device__ __forceinline__ void pack_tile(const dfl_pack_job* __restrict__ jobs, int njobs, int64_t grad_delta, int64_t s1_delta,
                                          int64_t s2_delta, Rule r) {
  constexpr bool updates = !std::is_same<Rule, PackOnly>::value;
  __shared__ PackTile tile;
  // which job: the last one whose first_tile <= blockIdx.x (binary search; the few records stay in the scalar cache)
  int lo = 0, hi = njobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].first_tile <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const dfl_pack_job j = jobs[lo];
  const int tidx = (int)blockIdx.x - j.first_tile;
  float* __restrict__ P = const_cast<float*>(j.src);
  const float* __restrict__ G = j.src + grad_delta;
  float* __restrict__ S1 = P + s1_delta;
  float* __restrict__ S2 = P + s2_delta;
  const bool has1 = r.has1(), has2 = r.has2();
  if (updates && j.kind == DFL_PACK_PLAIN) {
    const int64_t i0 = (int64_t)tidx * DFL_SGD_PLAIN_TILE;
    const int64_t i1 = min((int64_t)j.A, i0 + DFL_SGD_PLAIN_TILE);
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
      float s = has1 ? S1[i] : 0.f, b = has2 ? S2[i] : 0.f;
      P[i] = r(P[i], G[i], &s, &b);
      if (has1) S1[i] = s;
      if (has2) S2[i] = b;
    }
    return;
  }
  const int A = j.A, B = j.B, Cc = j.C;
  const int tb = B / PK_T;
  const int a0 = (tidx / tb) * PK_T, b0 = (tidx % tb) * PK_T;
  const int run4 = 8 * Cc;                                     // float4 per tile row (32 * C floats)
  for (int e = threadIdx.x; e < PK_T * run4; e += 256) {
    const int ar = e / run4, q4 = e - ar * run4;
    const int64_t o = ((int64_t)(a0 + ar) * B + b0) * Cc + 4 * q4;
    float4 v = *reinterpret_cast<const float4*>(P + o);
    if constexpr (updates) {
      const float4 w = v, g = *reinterpret_cast<const float4*>(G + o);
      float4 s = has1 ? *reinterpret_cast<const float4*>(S1 + o) : make_float4(0.f, 0.f, 0.f, 0.f);
      float4 b = has2 ? *reinterpret_cast<const float4*>(S2 + o) : make_float4(0.f, 0.f, 0.f, 0.f);
      v.x = r(w.x, g.x, &s.x, &b.x);
      v.y = r(w.y, g.y, &s.y, &b.y);
      v.z = r(w.z, g.z, &s.z, &b.z);
      v.w = r(w.w, g.w, &s.w, &b.w);
      *reinterpret_cast<float4*>(P + o) = v;
      if (has1) *reinterpret_cast<float4*>(S1 + o) = s;
      if (has2) *reinterpret_cast<float4*>(S2 + o) = b;
    }
    float* t = &tile[ar][4 * q4];
    t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
  }
  __syncthreads();
  pack_emit(tile, j.dst, j.kind, j.flip, j.split, A, B, Cc, a0, b0, PK_T, PK_T);
  if (j.dst2 != nullptr) pack_emit(tile, j.dst2, j.kind2, j.flip2, j.split2, A, B, Cc, a0, b0, PK_T, PK_T);
}

// dfl_pack_weights_tiled
__global__ void __launch_bounds__(256) pack_tiles_kernel(const dfl_pack_job* __restrict__ jobs, int njobs) {
  pack_tile(jobs, njobs, 0, 0, 0, PackOnly{});
}

// dfl_sgd_pack_tiled
__global__ void __launch_bounds__(256) sgd_pack_tiles_kernel(dfl_sgd_pack_args a) {
  pack_tile(a.jobs_dev, a.njobs, a.grad_delta, a.buf_delta, 0, SgdRule{a.lr, a.momentum, a.weight_decay, a.grad_scale, a.nesterov, 0});
}

// dfl_optim_pack_tiled
template <class Rule>
__global__ void __launch_bounds__(256) optim_pack_tiles_kernel(dfl_optim_pack_args a, Rule r) {
  pack_tile(a.jobs_dev, a.njobs, a.grad_delta, a.state1_delta, a.state2_delta, r);
}

static AdamRule adam_rule(double beta1, double beta2, float eps, float wd, float step_size, float bc2_sqrt, float gscale) {
  return AdamRule{eps, wd, gscale, (float)beta2, step_size, bc2_sqrt, (float)(1.0 - beta1), (float)(1.0 - beta2)};
}

static RmspropRule rmsprop_rule(float lr, double alpha, float eps, float wd, float mom, float gscale) {
  return RmspropRule{eps, wd, gscale, (float)alpha, (float)(1.0 - alpha), lr, mom};
}

static unsigned stream_grid(int64_t units) {
  int64_t b = ceil_div(units, 256);
  if (b > 8192) b = 8192;
  if (b < 1) b = 1;
  return (unsigned)b;
}

}  // namespace dfl

using namespace dfl;

extern "C" int dfl_rowblock_count(int64_t M, int32_t C) { return rowblocks(M, C); }

extern "C" int dfl_colstats(const dfl_colstats_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a && a->a && a->partials && a->M > 0 && a->C > 0, "dfl_colstats: bad args");
  DFL_REQUIRE(a->nblocks == rowblocks(a->M, a->C), "dfl_colstats: nblocks must be dfl_rowblock_count(M, C)");
  int W;
  const int rc = chan_unit_width("dfl_colstats", a->bf16, a->C, {{a->a, a->lda}, {a->b, a->ldb}}, &W);
  if (rc != DFL_OK) return rc;
  const RowGeom g = row_geom(a->C, W);
  DFL_LAUNCH_UNIT(W, colstats_kernel, dim3((unsigned)a->nblocks, (unsigned)g.gy), stream, *a, g.UX, (int)ceil_div(a->M, a->nblocks));
  return check_launch("dfl_colstats");
}

extern "C" int dfl_bn_finalize(const dfl_bn_finalize_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a && a->partials && a->gamma && a->beta && a->scale && a->shift && a->save_mean && a->save_invstd,
              "dfl_bn_finalize: missing pointer");
  DFL_REQUIRE(a->C > 0 && a->nblocks > 0 && a->count > 0, "dfl_bn_finalize: bad sizes");
  DFL_REQUIRE((a->running_mean == nullptr) == (a->running_var == nullptr), "dfl_bn_finalize: running stats go together");
  const int cpb = finalize_cpb(a->C);
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((unsigned)ceil_div(a->C, cpb)), dim3(256), 0, static_cast<hipStream_t>(stream), *a,
                     cpb);
  return check_launch("dfl_bn_finalize");
}

extern "C" int dfl_bn_finalize_live(const dfl_bn_live_job* jobs_dev, int32_t njobs, int32_t max_C, dfl_stream_t stream) {
  DFL_REQUIRE(jobs_dev && njobs > 0 && max_C > 0, "dfl_bn_finalize_live: bad args");
  hipLaunchKernelGGL(bn_finalize_live_kernel, dim3((unsigned)ceil_div(max_C, 256), (unsigned)njobs), dim3(256), 0,
                     static_cast<hipStream_t>(stream), jobs_dev);
  return check_launch("dfl_bn_finalize_live");
}

extern "C" int dfl_bn_bwd_finalize_live(const dfl_bn_bwd_live_job* jobs_dev, int32_t njobs, int32_t max_C, dfl_stream_t stream) {
  DFL_REQUIRE(jobs_dev && njobs > 0 && max_C > 0, "dfl_bn_bwd_finalize_live: bad args");
  hipLaunchKernelGGL(bn_bwd_finalize_live_kernel, dim3((unsigned)ceil_div(max_C, 256), (unsigned)njobs), dim3(256), 0,
                     static_cast<hipStream_t>(stream), jobs_dev);
  return check_launch("dfl_bn_bwd_finalize_live");
}

extern "C" int dfl_bn_eval_prepare(const float* gamma, const float* beta, const float* running_mean,
                                   const float* running_var, float* scale, float* shift, int32_t C, float eps,
                                   dfl_stream_t stream) {
  DFL_REQUIRE(gamma && beta && running_mean && running_var && scale && shift && C > 0, "dfl_bn_eval_prepare: bad args");
  hipLaunchKernelGGL(bn_eval_kernel, dim3((unsigned)ceil_div(C, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     gamma, beta, running_mean, running_var, scale, shift, (int)C, eps);
  return check_launch("dfl_bn_eval_prepare");
}

extern "C" int dfl_bn_bwd_finalize(const dfl_bn_bwd_finalize_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a && a->partials && a->gamma && a->save_mean && a->save_invstd && a->dgamma && a->dbeta && a->coef,
              "dfl_bn_bwd_finalize: missing pointer");
  DFL_REQUIRE(a->C > 0 && a->nblocks > 0 && a->count >= 0, "dfl_bn_bwd_finalize: bad sizes");
  const int cpb = finalize_cpb(a->C);
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((unsigned)ceil_div(a->C, cpb)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), *a, cpb);
  return check_launch("dfl_bn_bwd_finalize");
}

extern "C" int dfl_bn_relu_bwd_apply(const dfl_bn_relu_bwd_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a && a->dy && a->r && a->dpre && a->M > 0 && a->C > 0, "dfl_bn_relu_bwd_apply: bad args");
  DFL_REQUIRE(a->nblocks == rowblocks(a->M, a->C), "dfl_bn_relu_bwd_apply: nblocks must be dfl_rowblock_count(M, C)");
  int W;
  const int rc = chan_unit_width("dfl_bn_relu_bwd_apply", a->bf16, a->C, {{a->dy, a->lddy}, {a->r, a->ldr}, {a->dpre, a->ldo}}, &W,
                                 "ld", !a->split_out, ", no split output");
  if (rc != DFL_OK) return rc;
  DFL_REQUIRE(!a->split_out || W == 4, "dfl_bn_relu_bwd_apply: split_out needs the vector layout (C, ld % 4 == 0, 16-byte alignment)");
  const RowGeom g = row_geom(a->C, W);
  DFL_LAUNCH_UNIT(W, bn_relu_bwd_kernel, dim3((unsigned)a->nblocks, (unsigned)g.gy), stream, *a, g.UX, (int)ceil_div(a->M, a->nblocks));
  return check_launch("dfl_bn_relu_bwd_apply");
}

extern "C" int dfl_reduce_partials(const float* partials, float* out, int32_t nblocks, int32_t stride, int32_t C,
                                   dfl_stream_t stream) {
  DFL_REQUIRE(partials && out && nblocks > 0 && C > 0 && stride >= C, "dfl_reduce_partials: bad args");
  hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)ceil_div(C, 8)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     partials, out, (int)nblocks, (int)stride, (int)C);
  return check_launch("dfl_reduce_partials");
}

extern "C" int dfl_reduce_job_blocks(int64_t n, int32_t count) {
  DFL_REQUIRE(n > 0 && count > 0, "dfl_reduce_job_blocks: bad args");
  return reduce_job_blocks(n, count);
}

extern "C" int dfl_reduce_batch(const dfl_reduce_job* jobs_dev, int32_t njobs, int32_t total_blocks, dfl_stream_t stream) {
  DFL_REQUIRE(jobs_dev && njobs > 0 && total_blocks > 0, "dfl_reduce_batch: bad args");
  hipLaunchKernelGGL(reduce_batch_kernel, dim3((unsigned)total_blocks), dim3(RB_T), 0, static_cast<hipStream_t>(stream),
                     jobs_dev, (int)njobs);
  return check_launch("dfl_reduce_batch");
}

extern "C" int dfl_affine_copy(const dfl_affine_copy_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a && a->x && a->y && a->N > 0 && a->H > 0 && a->W > 0 && a->C > 0, "dfl_affine_copy: bad args");
  DFL_REQUIRE(a->xoy >= 0 && a->xox >= 0 && a->xoy + a->H <= a->xH && a->xox + a->W <= a->xW, "dfl_affine_copy: source window");
  DFL_REQUIRE(a->yoy >= 0 && a->yox >= 0 && a->yoy + a->H <= a->yH && a->yox + a->W <= a->yW, "dfl_affine_copy: dest window");
  DFL_REQUIRE((a->scale == nullptr) == (a->shift == nullptr), "dfl_affine_copy: scale/shift go together");
  int W;
  const int rc = chan_unit_width("dfl_affine_copy", a->bf16, a->C, {{a->x, a->ldx}, {a->y, a->ldy}}, &W);
  if (rc != DFL_OK) return rc;
  // the float4 form reads scale / shift as float4 too (the other two forms read them one channel at a time)
  if (W == 4 && a->scale != nullptr && !(aligned16(a->scale) && aligned16(a->shift))) W = 1;
  const int cq = a->C / W;
  const int64_t total = (int64_t)a->N * a->H * a->W * cq;
  DFL_LAUNCH_UNIT(W, affine_copy_kernel, dim3(stream_grid(total)), stream, *a, total, cq);
  return check_launch("dfl_affine_copy");
}

// validation and unit form of both pool directions: units per pixel and units in all (one thread each, grid-stride)
static int pool_form(const dfl_pool_args* a, bool bwd, int* W, int* cq, int64_t* total) {
  DFL_REQUIRE(a && a->x && a->y && a->N > 0 && a->H >= 2 && a->W >= 2 && a->C > 0, "dfl_maxpool2x2: bad args");
  DFL_REQUIRE(!bwd || a->dx != nullptr, "dfl_maxpool2x2_bwd: dx required");
  const int rc = chan_unit_width("dfl_maxpool2x2", a->bf16, a->C, {{a->x, a->ldx}, {a->y, a->ldy}, {bwd ? a->dx : nullptr, a->lddx}}, W);
  if (rc != DFL_OK) return rc;
  *cq = a->C / *W;
  *total = (int64_t)a->N * (a->H / 2) * (a->W / 2) * *cq;
  return DFL_OK;
}

extern "C" int dfl_maxpool2x2_fwd(const dfl_pool_args* a, dfl_stream_t stream) {
  int W, cq;
  int64_t total;
  const int rc = pool_form(a, false, &W, &cq, &total);
  if (rc != DFL_OK) return rc;
  DFL_LAUNCH_UNIT(W, maxpool_fwd_kernel, dim3(stream_grid(total)), stream, *a, total, cq);
  return check_launch("dfl_maxpool2x2_fwd");
}

extern "C" int dfl_maxpool2x2_bwd(const dfl_pool_args* a, dfl_stream_t stream) {
  int W, cq;
  int64_t total;
  const int rc = pool_form(a, true, &W, &cq, &total);
  if (rc != DFL_OK) return rc;
  DFL_LAUNCH_UNIT(W, maxpool_bwd_kernel, dim3(stream_grid(total)), stream, *a, total, cq);
  return check_launch("dfl_maxpool2x2_bwd");
}

extern "C" int dfl_pack_weights(const dfl_pack_job* jobs_dev, int32_t njobs, int64_t max_elems, dfl_stream_t stream) {
  DFL_REQUIRE(jobs_dev && njobs > 0 && max_elems > 0, "dfl_pack_weights: bad args");
  int64_t bx = ceil_div(max_elems, 256 * 8);
  if (bx > 1024) bx = 1024;
  if (bx < 1) bx = 1;
  hipLaunchKernelGGL(pack_kernel, dim3((unsigned)bx, (unsigned)njobs), dim3(256), 0, static_cast<hipStream_t>(stream), jobs_dev);
  return check_launch("dfl_pack_weights");
}

extern "C" int dfl_pack_weights_tiled(const dfl_pack_job* jobs_dev, int32_t njobs, int32_t total_tiles, dfl_stream_t stream) {
  DFL_REQUIRE(jobs_dev && njobs > 0 && total_tiles > 0, "dfl_pack_weights_tiled: bad args");
  hipLaunchKernelGGL(pack_tiles_kernel, dim3((unsigned)total_tiles), dim3(256), 0, static_cast<hipStream_t>(stream), jobs_dev, (int)njobs);
  return check_launch("dfl_pack_weights_tiled");
}

extern "C" int dfl_sgd_pack_tiled(const dfl_sgd_pack_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr && a->jobs_dev != nullptr && a->njobs > 0 && a->total_tiles > 0, "dfl_sgd_pack_tiled: empty job list");
  DFL_REQUIRE(a->grad_delta % 4 == 0 && a->buf_delta % 4 == 0, "dfl_sgd_pack_tiled: gradient / momentum arenas not 16-byte congruent with the parameters");
  DFL_REQUIRE(a->momentum >= 0.f && (!a->nesterov || a->momentum > 0.f), "dfl_sgd_pack_tiled: nesterov needs a momentum");
  hipLaunchKernelGGL(sgd_pack_tiles_kernel, dim3((unsigned)a->total_tiles), dim3(256), 0, static_cast<hipStream_t>(stream), *a);
  return check_launch("dfl_sgd_pack_tiled");
}

extern "C" int dfl_sgd_step(float* p, const float* grad, float* momentum_buf, int64_t n, float lr, float momentum,
                            float weight_decay, float grad_scale, int32_t nesterov, int32_t first_step,
                            dfl_stream_t stream) {
  DFL_REQUIRE(p && grad && n > 0, "dfl_sgd_step: bad args");
  DFL_REQUIRE(momentum == 0.f || momentum_buf != nullptr, "dfl_sgd_step: momentum buffer required");
  hipLaunchKernelGGL(optim_kernel<SgdRule>, dim3(stream_grid(n)), dim3(256), 0, static_cast<hipStream_t>(stream), p, grad,
                     momentum_buf, nullptr, n, SgdRule{lr, momentum, weight_decay, grad_scale, (int)nesterov, (int)first_step});
  return check_launch("dfl_sgd_step");
}

// ---- Adam / RMSprop entry points: every coefficient is checked before anything is launched
static bool adam_coefs_ok(float lr, double beta1, double beta2, float eps, float wd, float step_size, float bc2_sqrt) {
  // step_size = lr / (1 - beta1^t) >= lr and bc2_sqrt = sqrt(1 - beta2^t) in (0, 1] for every step count t >= 1
  return lr >= 0.f && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.f && wd >= 0.f &&
         step_size >= lr && step_size < INFINITY && bc2_sqrt > 0.f && bc2_sqrt <= 1.f;
}

static bool rmsprop_coefs_ok(float lr, double alpha, float eps, float wd, float mom) {
  return lr >= 0.f && lr < INFINITY && alpha >= 0.0 && alpha < INFINITY && eps >= 0.f && wd >= 0.f && wd < INFINITY &&
         mom >= 0.f && mom < INFINITY;
}

extern "C" int dfl_adam_step(float* p, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, double beta1,
                             double beta2, float eps, float weight_decay, float step_size, float bc2_sqrt, float grad_scale,
                             dfl_stream_t stream) {
  DFL_REQUIRE(p && grad && exp_avg && exp_avg_sq && n > 0, "dfl_adam_step: bad args (NULL tensor or n <= 0)");
  DFL_REQUIRE(exp_avg != exp_avg_sq && exp_avg != p && exp_avg_sq != p, "dfl_adam_step: state tensors alias each other or p");
  DFL_REQUIRE(adam_coefs_ok(lr, beta1, beta2, eps, weight_decay, step_size, bc2_sqrt),
              "dfl_adam_step: bad coefficients (need 0 <= beta < 1, lr, eps, weight_decay >= 0, step_size = lr/(1-beta1^t) "
              ">= lr, bc2_sqrt = sqrt(1-beta2^t) in (0, 1])");
  hipLaunchKernelGGL(optim_kernel<AdamRule>, dim3(stream_grid(n)), dim3(256), 0, static_cast<hipStream_t>(stream), p, grad, exp_avg,
                     exp_avg_sq, n, adam_rule(beta1, beta2, eps, weight_decay, step_size, bc2_sqrt, grad_scale));
  return check_launch("dfl_adam_step");
}

extern "C" int dfl_rmsprop_step(float* p, const float* grad, float* square_avg, float* momentum_buf, int64_t n, float lr,
                                double alpha, float eps, float weight_decay, float momentum, float grad_scale,
                                dfl_stream_t stream) {
  DFL_REQUIRE(p && grad && square_avg && n > 0, "dfl_rmsprop_step: bad args (NULL tensor or n <= 0)");
  DFL_REQUIRE(rmsprop_coefs_ok(lr, alpha, eps, weight_decay, momentum),
              "dfl_rmsprop_step: bad coefficients (lr, alpha, eps, weight_decay, momentum must be finite and >= 0)");
  DFL_REQUIRE((momentum == 0.f) == (momentum_buf == nullptr), "dfl_rmsprop_step: momentum buffer required when (and only when) momentum > 0");
  DFL_REQUIRE(square_avg != p && (momentum_buf == nullptr || (momentum_buf != p && momentum_buf != square_avg)),
              "dfl_rmsprop_step: state tensors alias each other or p");
  hipLaunchKernelGGL(optim_kernel<RmspropRule>, dim3(stream_grid(n)), dim3(256), 0, static_cast<hipStream_t>(stream), p, grad,
                     square_avg, momentum_buf, n, rmsprop_rule(lr, alpha, eps, weight_decay, momentum, grad_scale));
  return check_launch("dfl_rmsprop_step");
}

extern "C" int dfl_optim_pack_tiled(const dfl_optim_pack_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr && a->jobs_dev != nullptr && a->njobs > 0 && a->total_tiles > 0, "dfl_optim_pack_tiled: empty job list");
  DFL_REQUIRE(a->kind == DFL_OPTIM_ADAM || a->kind == DFL_OPTIM_RMSPROP, "dfl_optim_pack_tiled: kind must be DFL_OPTIM_ADAM or DFL_OPTIM_RMSPROP");
  const bool has2 = a->kind == DFL_OPTIM_ADAM || a->momentum != 0.f;
  DFL_REQUIRE(a->grad_delta % 4 == 0 && a->state1_delta % 4 == 0 && (!has2 || a->state2_delta % 4 == 0),
              "dfl_optim_pack_tiled: gradient / state arenas not 16-byte congruent with the parameters");
  DFL_REQUIRE(a->grad_delta != 0 && a->state1_delta != 0 && a->state1_delta != a->grad_delta &&
              (!has2 || (a->state2_delta != 0 && a->state2_delta != a->grad_delta && a->state2_delta != a->state1_delta)),
              "dfl_optim_pack_tiled: parameter, gradient and state arenas overlap (equal deltas)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (a->kind == DFL_OPTIM_ADAM) {
    DFL_REQUIRE(adam_coefs_ok(a->lr, a->beta1, a->beta2, a->eps, a->weight_decay, a->step_size, a->bc2_sqrt),
                "dfl_optim_pack_tiled: bad Adam coefficients (need 0 <= beta < 1, lr, eps, weight_decay >= 0, step_size >= lr, "
                "bc2_sqrt in (0, 1])");
    hipLaunchKernelGGL(optim_pack_tiles_kernel<AdamRule>, dim3((unsigned)a->total_tiles), dim3(256), 0, s, *a,
                       adam_rule(a->beta1, a->beta2, a->eps, a->weight_decay, a->step_size, a->bc2_sqrt, a->grad_scale));
  } else {
    DFL_REQUIRE(rmsprop_coefs_ok(a->lr, a->alpha, a->eps, a->weight_decay, a->momentum),
                "dfl_optim_pack_tiled: bad RMSprop coefficients (lr, alpha, eps, weight_decay, momentum must be finite and >= 0)");
    hipLaunchKernelGGL(optim_pack_tiles_kernel<RmspropRule>, dim3((unsigned)a->total_tiles), dim3(256), 0, s, *a,
                       rmsprop_rule(a->lr, a->alpha, a->eps, a->weight_decay, a->momentum, a->grad_scale));
  }
  return check_launch("dfl_optim_pack_tiled");
}
