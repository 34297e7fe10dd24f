// Bone surfaces of a label volume (include/dfl_hip.h "Bone surfaces"): discrete marching cubes
// for up to DFL_MESH_MAX_LABELS labels per pass over the volume, the CSR topology the smoother and the normals gather
// over, windowed-sinc smoothing (one gather launch per term), fp64 affine transforms and area-weighted normals.
// No float atomics anywhere: every output element is written by exactly one thread, in an order fixed by the data.
#include "common.h"

namespace dfl {

constexpr int MC_THREADS = 256;
constexpr int MC_ROUNDS = DFL_MESH_MC_CELLS / MC_THREADS;
static_assert(MC_ROUNDS * MC_THREADS == DFL_MESH_MC_CELLS, "cells per block");
// per-label counts travel packed, 16 bits per label in one u64: a block holds at most 5 triangles per cell and label
static_assert(DFL_MESH_MC_CELLS * 5 < 65536 && DFL_MESH_MAX_LABELS * 16 <= 64, "packed triangle counts");

// lower end of edge e as (dx, dy, dz) and its axis (tools/gen_mc_table.py numbering)
__constant__ unsigned char kEdgeLo[12][4] = {
    {0, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 1, 1, 0},   // along x: (y, z) offsets
    {0, 0, 0, 1}, {1, 0, 0, 1}, {0, 0, 1, 1}, {1, 0, 1, 1},   // along y: (x, z)
    {0, 0, 0, 2}, {1, 0, 0, 2}, {0, 1, 0, 2}, {1, 1, 0, 2}};  // along z: (x, y)

struct McCell {
  int64_t base;    // linear index of the cell's lower corner
  uint32_t cases;  // 8 bits per label
};

__device__ __forceinline__ McCell mc_classify(const dfl_mesh_mc_args& a, int64_t c) {
  // cells < 2^31 (checked by the launchers): 32-bit division, far cheaper than the 64-bit sequence
  const uint32_t cx = a.nx - 1, cy = a.ny - 1, c32 = (uint32_t)c;
  const uint32_t t = c32 / cx, x = c32 - t * cx, z = t / cy, y = t - z * cy;
  const int64_t sx = 1, sy = a.nx, sz = (int64_t)a.nx * a.ny;
  const int64_t b = x + sy * y + sz * z;
  unsigned char v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = a.volume[b + ((i & 1) ? sx : 0) + ((i & 2) ? sy : 0) + ((i & 4) ? sz : 0)];
  uint32_t cases = 0;
  for (int l = 0; l < a.n_labels; ++l) {
    uint32_t k = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) k |= (uint32_t)(v[i] == (unsigned char)a.labels[l]) << i;
    cases |= k << (8 * l);
  }
  return {b, cases};
}

__device__ __forceinline__ uint64_t mc_counts(const dfl_mesh_mc_args& a, uint32_t cases) {
  uint64_t n = 0;
  for (int l = 0; l < a.n_labels; ++l) {
    const uint32_t k = (cases >> (8 * l)) & 255u;
    n |= (uint64_t)(a.tri_off[k + 1] - a.tri_off[k]) << (16 * l);
  }
  return n;
}

// exclusive scan of v over the 256 threads of the block; total = the block's sum.  lds[4] is reused after return.
__device__ __forceinline__ uint64_t block_scan_u64(uint64_t v, uint64_t* lds, uint64_t& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint64_t s = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t t = __shfl_up(s, d, 64);
    if (lane >= d) s += t;
  }
  if (lane == 63) lds[w] = s;
  __syncthreads();
  uint64_t before = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < MC_THREADS / 64; ++k) {
    const uint64_t t = lds[k];
    before += k < w ? t : 0;
    total += t;
  }
  __syncthreads();
  return before + s - v;
}

__global__ __launch_bounds__(MC_THREADS) void mc_count_kernel(dfl_mesh_mc_args a, int64_t cells) {
  __shared__ uint64_t lds[MC_THREADS / 64];
  const int64_t c0 = (int64_t)blockIdx.x * DFL_MESH_MC_CELLS;
  uint64_t n = 0;
  for (int r = 0; r < MC_ROUNDS; ++r) {
    const int64_t c = c0 + r * MC_THREADS + threadIdx.x;
    if (c < cells) n += mc_counts(a, mc_classify(a, c).cases);
  }
  uint64_t total;
  block_scan_u64(n, lds, total);
  if (threadIdx.x < DFL_MESH_MAX_LABELS)
    a.block_counts[(int64_t)blockIdx.x * DFL_MESH_MAX_LABELS + threadIdx.x] = (int32_t)((total >> (16 * threadIdx.x)) & 0xffff);
}

// one workgroup: exclusive scan of block_counts over the blocks, label by label, labels one after another
__global__ __launch_bounds__(1024) void mc_scan_kernel(dfl_mesh_mc_args a, int64_t n_blocks) {
  __shared__ int64_t lds[16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int64_t base = 0;
  for (int l = 0; l < a.n_labels; ++l) {
    if (threadIdx.x == 0) a.totals[l] = base;
    for (int64_t b0 = 0; b0 < n_blocks; b0 += 1024) {
      const int64_t b = b0 + threadIdx.x;
      const int64_t v = b < n_blocks ? a.block_counts[b * DFL_MESH_MAX_LABELS + l] : 0;
      int64_t s = v;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int64_t t = __shfl_up(s, d, 64);
        if (lane >= d) s += t;
      }
      if (lane == 63) lds[w] = s;
      __syncthreads();
      int64_t before = 0, total = 0;
      for (int k = 0; k < 16; ++k) {
        before += k < w ? lds[k] : 0;
        total += lds[k];
      }
      if (b < n_blocks) a.block_offsets[b * DFL_MESH_MAX_LABELS + l] = base + before + s - v;
      base += total;
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) a.totals[a.n_labels] = base;
}

__global__ __launch_bounds__(MC_THREADS) void mc_emit_kernel(dfl_mesh_mc_args a, int64_t cells) {
  __shared__ uint64_t lds[MC_THREADS / 64];
  const int64_t c0 = (int64_t)blockIdx.x * DFL_MESH_MC_CELLS;
  int64_t off[DFL_MESH_MAX_LABELS];
#pragma unroll
  for (int l = 0; l < DFL_MESH_MAX_LABELS; ++l)
    off[l] = l < a.n_labels ? a.block_offsets[(int64_t)blockIdx.x * DFL_MESH_MAX_LABELS + l] : 0;
  int64_t koff[12];
#pragma unroll
  for (int e = 0; e < 12; ++e)
    koff[e] = 3 * (kEdgeLo[e][0] + (int64_t)a.nx * (kEdgeLo[e][1] + (int64_t)a.ny * kEdgeLo[e][2])) + kEdgeLo[e][3];
  for (int r = 0; r < MC_ROUNDS; ++r) {
    const int64_t c = c0 + r * MC_THREADS + threadIdx.x;
    McCell m = {0, 0};
    if (c < cells) m = mc_classify(a, c);
    const uint64_t n = mc_counts(a, m.cases);
    uint64_t total;
    const uint64_t before = block_scan_u64(n, lds, total);
    if (total == 0) continue;               // uniform across the block
#pragma unroll
    for (int l = 0; l < DFL_MESH_MAX_LABELS; ++l) {
      if (l >= a.n_labels) break;
      const int nt = (int)((n >> (16 * l)) & 0xffff);
      if (nt) {
        const uint32_t k = (m.cases >> (8 * l)) & 255u;
        const unsigned char* te = a.tri_edges + 3 * a.tri_off[k];
        int64_t* out = a.keys + 3 * (off[l] + (int64_t)((before >> (16 * l)) & 0xffff));
        for (int j = 0; j < 3 * nt; ++j) out[j] = 3 * m.base + koff[te[j]];
      }
      off[l] += (int64_t)((total >> (16 * l)) & 0xffff);
    }
  }
}

__global__ __launch_bounds__(256) void mesh_decode_kernel(dfl_mesh_decode_args a) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= a.V) return;
  const int64_t key = a.keys[v], q = key / 3, ax = key - 3 * q;
  const int64_t x = q % a.nx, r = q / a.nx, y = r % a.ny, z = r / a.ny;
  a.pos[3 * v + 0] = (float)x + (ax == 0 ? 0.5f : 0.0f);
  a.pos[3 * v + 1] = (float)y + (ax == 1 ? 0.5f : 0.0f);
  a.pos[3 * v + 2] = (float)z + (ax == 2 ? 0.5f : 0.0f);
}

__global__ __launch_bounds__(256) void mesh_topology_kernel(dfl_mesh_topo_args a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.T) return;
  const int64_t p = a.tris[3 * t], q = a.tris[3 * t + 1], r = a.tris[3 * t + 2];
  if (a.edge_keys) {
    int64_t* e = a.edge_keys + 6 * t;
    e[0] = p * a.V + q;
    e[1] = q * a.V + p;
    e[2] = q * a.V + r;
    e[3] = r * a.V + q;
    e[4] = r * a.V + p;
    e[5] = p * a.V + r;
  }
  if (a.vt_keys) {
    const int64_t m = 3 * a.T;
    a.vt_keys[3 * t + 0] = p * m + 3 * t;
    a.vt_keys[3 * t + 1] = q * m + 3 * t + 1;
    a.vt_keys[3 * t + 2] = r * m + 3 * t + 2;
  }
}

// fixed[] was cleared by the launcher; every thread writes only 1s into it (no read-modify-write)
__global__ __launch_bounds__(256) void mesh_csr_kernel(dfl_mesh_csr_args a) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= a.nnz) return;
  const int64_t key = a.keys[k], row = key / a.div;
  a.col[k] = (int32_t)((key - row * a.div) / a.col_div);
  if (a.counts && a.counts[k] == 1) a.fixed[row] = 1;
  const int64_t prev = k == 0 ? -1 : a.keys[k - 1] / a.div;
  for (int64_t r = prev + 1; r <= row; ++r) a.row_ptr[r] = (int32_t)k;
  if (k == a.nnz - 1)
    for (int64_t r = row + 1; r <= a.n_rows; ++r) a.row_ptr[r] = (int32_t)a.nnz;
}

// term n of the windowed-sinc sum.  prev = T_{n-1} (x itself when FIRST), own2 = T_{n-2} at this vertex's own index:
// from x (n == 2) or from `dst`, which then receives T_n in place -- a thread reads and writes only its own element.
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void mesh_smooth_kernel(dfl_mesh_smooth_args a, const float4* prev, float4* dst,
                                                          int n, bool own2_from_x) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.V) return;
  auto at = [&](int64_t j) -> float3 {
    if (FIRST) return make_float3(a.x[3 * j], a.x[3 * j + 1], a.x[3 * j + 2]);
    const float4 p = prev[j];
    return make_float3(p.x, p.y, p.z);
  };
  // a vertex without neighbours (no triangle uses it) is held like a fixed one: W is the identity there, not 0 / 0
  const int32_t k0 = a.row_ptr[i], k1 = a.row_ptr[i + 1];
  const bool fixed = a.fixed[i] != 0 || k1 == k0;
  float3 m;
  if (fixed) {
    m = at(i);
  } else {
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int32_t k = k0; k < k1; ++k) {
      const float3 p = at(a.col[k]);
      sx += p.x;
      sy += p.y;
      sz += p.z;
    }
    const float cnt = (float)(k1 - k0);
    m = make_float3(sx / cnt, sy / cnt, sz / cnt);
  }
  const float3 x = make_float3(a.x[3 * i], a.x[3 * i + 1], a.x[3 * i + 2]);
  float3 tn, s;
  const float cn = a.coef[n];
  if (FIRST) {
    tn = m;
    const float c0 = a.coef[0];
    s = make_float3(c0 * x.x + cn * tn.x, c0 * x.y + cn * tn.y, c0 * x.z + cn * tn.z);
  } else {
    float3 t2;
    if (own2_from_x) {
      t2 = x;
    } else {
      const float4 q = dst[i];
      t2 = make_float3(q.x, q.y, q.z);
    }
    tn = make_float3(2.f * m.x - t2.x, 2.f * m.y - t2.y, 2.f * m.z - t2.z);
    const float4 s0 = reinterpret_cast<const float4*>(a.acc)[i];
    s = make_float3(s0.x + cn * tn.x, s0.y + cn * tn.y, s0.z + cn * tn.z);
  }
  if (LAST) {
    const float3 o = fixed ? x : s;
    a.out[3 * i] = o.x;
    a.out[3 * i + 1] = o.y;
    a.out[3 * i + 2] = o.z;
  } else {
    dst[i] = make_float4(tn.x, tn.y, tn.z, 0.f);
    reinterpret_cast<float4*>(a.acc)[i] = make_float4(s.x, s.y, s.z, 0.f);
  }
}

__global__ __launch_bounds__(256) void mesh_transform_kernel(dfl_mesh_xform_args a) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= a.V) return;
  const double x = a.x[3 * v], y = a.x[3 * v + 1], z = a.x[3 * v + 2];
  double o[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) o[r] = a.M[4 * r] * x + a.M[4 * r + 1] * y + a.M[4 * r + 2] * z + a.M[4 * r + 3];
#pragma unroll
  for (int r = 0; r < 3; ++r) a.out[3 * v + r] = (float)o[r];
}

__global__ __launch_bounds__(256) void mesh_normals_kernel(dfl_mesh_normals_args a) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= a.V) return;
  double nx = 0, ny = 0, nz = 0;
  for (int32_t k = a.vt_ptr[v]; k < a.vt_ptr[v + 1]; ++k) {
    const int64_t t = a.vt_tri[k];
    const float* p = a.pos + 3 * (int64_t)a.tris[3 * t];
    const float* q = a.pos + 3 * (int64_t)a.tris[3 * t + 1];
    const float* r = a.pos + 3 * (int64_t)a.tris[3 * t + 2];
    const double ux = (double)q[0] - p[0], uy = (double)q[1] - p[1], uz = (double)q[2] - p[2];
    const double wx = (double)r[0] - p[0], wy = (double)r[1] - p[1], wz = (double)r[2] - p[2];
    nx += uy * wz - uz * wy;
    ny += uz * wx - ux * wz;
    nz += ux * wy - uy * wx;
  }
  const double len = sqrt(nx * nx + ny * ny + nz * nz);
  const double s = len > 0 ? 1.0 / len : 0.0;
  a.normals[3 * v] = (float)(nx * s);
  a.normals[3 * v + 1] = (float)(ny * s);
  a.normals[3 * v + 2] = (float)(nz * s);
}

inline unsigned grid_of(int64_t n) { return (unsigned)ceil_div(n, 256); }

int mc_check(const dfl_mesh_mc_args* a, const char* what) {
  DFL_REQUIRE(a != nullptr, "%s: null args", what);
  DFL_REQUIRE(a->nx >= 2 && a->ny >= 2 && a->nz >= 2, "%s: volume of %d x %d x %d has no cells", what, a->nx, a->ny, a->nz);
  const int64_t cells = (int64_t)(a->nx - 1) * (a->ny - 1) * (a->nz - 1);
  DFL_REQUIRE(cells < (1ll << 31), "%s: %lld cells, at most 2^31 - 1", what, (long long)cells);
  DFL_REQUIRE(a->n_labels >= 1 && a->n_labels <= DFL_MESH_MAX_LABELS, "%s: 1 to %d labels", what, DFL_MESH_MAX_LABELS);
  DFL_REQUIRE(a->volume && a->tri_off && a->tri_edges && a->block_counts && a->block_offsets && a->totals,
              "%s: volume, case table, block_counts, block_offsets and totals are required", what);
  for (int l = 0; l < a->n_labels; ++l)
    DFL_REQUIRE(a->labels[l] >= 0 && a->labels[l] <= 255, "%s: label %d outside 0..255", what, a->labels[l]);
  return DFL_OK;
}

}  // namespace dfl

extern "C" int dfl_mesh_mc_count(const dfl_mesh_mc_args* a, dfl_stream_t stream) {
  if (int rc = dfl::mc_check(a, "dfl_mesh_mc_count")) return rc;
  const int64_t cells = (int64_t)(a->nx - 1) * (a->ny - 1) * (a->nz - 1);
  const int64_t nb = dfl::ceil_div(cells, DFL_MESH_MC_CELLS);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(dfl::mc_count_kernel, dim3((unsigned)nb), dim3(dfl::MC_THREADS), 0, s, *a, cells);
  hipLaunchKernelGGL(dfl::mc_scan_kernel, dim3(1), dim3(1024), 0, s, *a, nb);
  return dfl::check_launch("dfl_mesh_mc_count");
}

extern "C" int dfl_mesh_mc_emit(const dfl_mesh_mc_args* a, dfl_stream_t stream) {
  if (int rc = dfl::mc_check(a, "dfl_mesh_mc_emit")) return rc;
  DFL_REQUIRE(a->keys != nullptr, "dfl_mesh_mc_emit: keys are required");
  const int64_t cells = (int64_t)(a->nx - 1) * (a->ny - 1) * (a->nz - 1);
  const int64_t nb = dfl::ceil_div(cells, DFL_MESH_MC_CELLS);
  hipLaunchKernelGGL(dfl::mc_emit_kernel, dim3((unsigned)nb), dim3(dfl::MC_THREADS), 0, static_cast<hipStream_t>(stream), *a, cells);
  return dfl::check_launch("dfl_mesh_mc_emit");
}

extern "C" int dfl_mesh_decode(const dfl_mesh_decode_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr && a->keys != nullptr && a->pos != nullptr, "dfl_mesh_decode: keys and pos are required");
  DFL_REQUIRE(a->V >= 0 && a->nx >= 2 && a->ny >= 2, "dfl_mesh_decode: bad sizes");
  if (a->V == 0) return DFL_OK;
  hipLaunchKernelGGL(dfl::mesh_decode_kernel, dim3(dfl::grid_of(a->V)), dim3(256), 0, static_cast<hipStream_t>(stream), *a);
  return dfl::check_launch("dfl_mesh_decode");
}

extern "C" int dfl_mesh_topology(const dfl_mesh_topo_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr && a->tris != nullptr, "dfl_mesh_topology: tris are required");
  DFL_REQUIRE(a->T >= 0 && a->V >= 0 && a->V < (1ll << 31), "dfl_mesh_topology: bad sizes");
  DFL_REQUIRE(3 * a->T < (1ll << 31), "dfl_mesh_topology: at most 2^31 - 1 triangle corners");
  if (a->T == 0) return DFL_OK;
  hipLaunchKernelGGL(dfl::mesh_topology_kernel, dim3(dfl::grid_of(a->T)), dim3(256), 0, static_cast<hipStream_t>(stream), *a);
  return dfl::check_launch("dfl_mesh_topology");
}

extern "C" int dfl_mesh_csr(const dfl_mesh_csr_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr && a->keys != nullptr && a->col != nullptr && a->row_ptr != nullptr, "dfl_mesh_csr: keys, col and row_ptr are required");
  DFL_REQUIRE(a->counts == nullptr || a->fixed != nullptr, "dfl_mesh_csr: counts need fixed");
  DFL_REQUIRE(a->nnz >= 1 && a->nnz < (1ll << 31) && a->div >= 1 && a->col_div >= 1 && a->n_rows >= 1 && a->n_rows < (1ll << 31),
              "dfl_mesh_csr: bad sizes");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (a->fixed && hipMemsetAsync(a->fixed, 0, (size_t)a->n_rows, s) != hipSuccess) {
    dfl::set_error("dfl_mesh_csr: clearing fixed failed");
    return DFL_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(dfl::mesh_csr_kernel, dim3(dfl::grid_of(a->nnz)), dim3(256), 0, s, *a);
  return dfl::check_launch("dfl_mesh_csr");
}

extern "C" int dfl_mesh_smooth(const dfl_mesh_smooth_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr && a->x && a->row_ptr && a->col && a->fixed && a->out, "dfl_mesh_smooth: x, row_ptr, col, fixed and out are required");
  DFL_REQUIRE(a->iterations >= 1 && a->iterations <= DFL_MESH_MAX_ITERS, "dfl_mesh_smooth: 1 to %d iterations", DFL_MESH_MAX_ITERS);
  DFL_REQUIRE(a->iterations == 1 || (a->t_a && a->t_b && a->acc && dfl::aligned16(a->t_a) && dfl::aligned16(a->t_b) && dfl::aligned16(a->acc)),
              "dfl_mesh_smooth: t_a, t_b and acc must be 16-byte aligned [V][4] buffers");
  DFL_REQUIRE(a->V >= 1 && a->V < (1ll << 31), "dfl_mesh_smooth: bad vertex count");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned g = dfl::grid_of(a->V);
  const int N = a->iterations;
  float4* A = reinterpret_cast<float4*>(a->t_a);
  float4* B = reinterpret_cast<float4*>(a->t_b);
  if (N == 1) {
    hipLaunchKernelGGL((dfl::mesh_smooth_kernel<true, true>), dim3(g), dim3(256), 0, s, *a, nullptr, nullptr, 1, false);
    return dfl::check_launch("dfl_mesh_smooth");
  }
  hipLaunchKernelGGL((dfl::mesh_smooth_kernel<true, false>), dim3(g), dim3(256), 0, s, *a, nullptr, A, 1, false);  // T1 -> A
  for (int n = 2; n <= N; ++n) {
    // T_{n-1} sits in A for even n, in B for odd n; T_n goes where T_{n-2} is (B for n == 2: T_0 is x)
    const float4* prev = (n & 1) ? B : A;
    float4* dst = (n & 1) ? A : B;
    if (n < N)
      hipLaunchKernelGGL((dfl::mesh_smooth_kernel<false, false>), dim3(g), dim3(256), 0, s, *a, prev, dst, n, n == 2);
    else
      hipLaunchKernelGGL((dfl::mesh_smooth_kernel<false, true>), dim3(g), dim3(256), 0, s, *a, prev, dst, n, n == 2);
  }
  return dfl::check_launch("dfl_mesh_smooth");
}

extern "C" int dfl_mesh_transform(const dfl_mesh_xform_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr && a->x != nullptr && a->out != nullptr && a->V >= 0, "dfl_mesh_transform: x and out are required");
  if (a->V == 0) return DFL_OK;
  hipLaunchKernelGGL(dfl::mesh_transform_kernel, dim3(dfl::grid_of(a->V)), dim3(256), 0, static_cast<hipStream_t>(stream), *a);
  return dfl::check_launch("dfl_mesh_transform");
}

extern "C" int dfl_mesh_normals(const dfl_mesh_normals_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr && a->pos && a->tris && a->vt_ptr && a->vt_tri && a->normals && a->V >= 0,
              "dfl_mesh_normals: pos, tris, vt_ptr, vt_tri and normals are required");
  if (a->V == 0) return DFL_OK;
  hipLaunchKernelGGL(dfl::mesh_normals_kernel, dim3(dfl::grid_of(a->V)), dim3(256), 0, static_cast<hipStream_t>(stream), *a);
  return dfl::check_launch("dfl_mesh_normals");
}
