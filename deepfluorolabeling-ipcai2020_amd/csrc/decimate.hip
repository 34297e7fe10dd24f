// Quadric-error mesh decimation, one round at a time (include/dfl_hip.h "Bone surfaces"): vertex
// quadrics, the collapse key and position of every undirected edge, the two-ring minimum that selects collapses which do
// not touch, and their application.  Memoryless: every round starts from the current mesh.
// Built with -ffp-contract=off: fp64 on the fp32 positions, every product and sum rounded on its own, in the order
// written here; tests/decimate_ref.py restates each expression.  No atomics: every output element has one writer.
#include "common.h"

namespace dfl {

constexpr uint64_t KEY_NONE = ~0ull;

struct Vec3d {
  double x, y, z;
};

__device__ __forceinline__ Vec3d load3(const float* pos, int64_t v) {
  return {(double)pos[3 * v], (double)pos[3 * v + 1], (double)pos[3 * v + 2]};
}

// (p1 - p0) x (p2 - p0)
__device__ __forceinline__ Vec3d tri_normal(const Vec3d& p0, const Vec3d& p1, const Vec3d& p2) {
  const double ux = p1.x - p0.x, uy = p1.y - p0.y, uz = p1.z - p0.z;
  const double wx = p2.x - p0.x, wy = p2.y - p0.y, wz = p2.z - p0.z;
  return {uy * wz - uz * wy, uz * wx - ux * wz, ux * wy - uy * wx};
}

__device__ __forceinline__ double dot3(const Vec3d& a, const Vec3d& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// (x, y, z, 1)^T q (x, y, z, 1), q = (aa ab ac ad bb bc bd cc cd dd)
__device__ __forceinline__ double quadric_cost(const double* q, const Vec3d& p) {
  const double r0 = ((q[0] * p.x + q[1] * p.y) + q[2] * p.z) + q[3];
  const double r1 = ((q[1] * p.x + q[4] * p.y) + q[5] * p.z) + q[6];
  const double r2 = ((q[2] * p.x + q[5] * p.y) + q[7] * p.z) + q[8];
  const double r3 = ((q[3] * p.x + q[6] * p.y) + q[8] * p.z) + q[9];
  return ((p.x * r0 + p.y * r1) + p.z * r2) + r3;
}

__device__ __forceinline__ Vec3d round32(const Vec3d& p) { return {(double)(float)p.x, (double)(float)p.y, (double)(float)p.z}; }

__global__ __launch_bounds__(256) void mesh_quadrics_kernel(dfl_mesh_quadrics_args a) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= a.V) return;
  double q[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) q[i] = 0.0;
  for (int32_t k = a.vt_ptr[v]; k < a.vt_ptr[v + 1]; ++k) {
    const int64_t t = a.vt_tri[k];
    const Vec3d p0 = load3(a.pos, a.tris[3 * t]);
    const Vec3d n = tri_normal(p0, load3(a.pos, a.tris[3 * t + 1]), load3(a.pos, a.tris[3 * t + 2]));
    const double l = sqrt(dot3(n, n));
    if (l == 0.0) continue;
    const double d = -dot3(n, p0);
    q[0] += (n.x * n.x) / l;
    q[1] += (n.x * n.y) / l;
    q[2] += (n.x * n.z) / l;
    q[3] += (n.x * d) / l;
    q[4] += (n.y * n.y) / l;
    q[5] += (n.y * n.z) / l;
    q[6] += (n.y * d) / l;
    q[7] += (n.z * n.z) / l;
    q[8] += (n.z * d) / l;
    q[9] += (d * d) / l;
  }
#pragma unroll
  for (int i = 0; i < 10; ++i) a.Q[10 * v + i] = q[i];
}

// does a triangle at w (one that does not hold both u and v) turn when u and v move to x?
__device__ __forceinline__ bool ring_flips(const dfl_mesh_collapse_keys_args& a, int32_t w, int32_t u, int32_t v, const Vec3d& x) {
  for (int32_t k = a.vt_ptr[w]; k < a.vt_ptr[w + 1]; ++k) {
    const int64_t t = a.vt_tri[k];
    const int32_t i0 = a.tris[3 * t], i1 = a.tris[3 * t + 1], i2 = a.tris[3 * t + 2];
    const bool m0 = i0 == u || i0 == v, m1 = i1 == u || i1 == v, m2 = i2 == u || i2 == v;
    const bool has_u = i0 == u || i1 == u || i2 == u, has_v = i0 == v || i1 == v || i2 == v;
    if (has_u && has_v) continue;
    const Vec3d p0 = load3(a.pos, i0), p1 = load3(a.pos, i1), p2 = load3(a.pos, i2);
    const Vec3d n0 = tri_normal(p0, p1, p2);
    const Vec3d n1 = tri_normal(m0 ? x : p0, m1 ? x : p1, m2 ? x : p2);
    const double d = dot3(n0, n1);
    if (!(d > 0.0) || !(d * d >= 0.04 * (dot3(n0, n0) * dot3(n1, n1)))) return true;
  }
  return false;
}

__global__ __launch_bounds__(256) void mesh_collapse_keys_kernel(dfl_mesh_collapse_keys_args a) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.E) return;
  const int32_t u = a.edge_u[e], v = a.edge_v[e];
  const int32_t u0 = a.row_ptr[u], u1 = a.row_ptr[u + 1], v0 = a.row_ptr[v], v1 = a.row_ptr[v + 1];
  // neither end held: every edge at u and at v, (u, v) among them, lies on exactly two triangles
  bool ok = true;
  for (int32_t k = u0; k < u1; ++k) ok &= a.use[k] == 2;
  for (int32_t k = v0; k < v1; ++k) ok &= a.use[k] == 2;
  // the rows ascend: a merge finds the common neighbours
  int common = 0;
  for (int32_t i = u0, j = v0; ok && i < u1 && j < v1;) {
    const int32_t ci = a.col[i], cj = a.col[j];
    if (ci == cj) {
      ++common;
      ok &= a.row_ptr[ci + 1] - a.row_ptr[ci] >= 5;
      ++i;
      ++j;
    } else if (ci < cj) {
      ++i;
    } else {
      ++j;
    }
  }
  ok &= common == 2 && (u1 - u0) + (v1 - v0) - 4 >= 3;
  Vec3d x = {0.0, 0.0, 0.0};
  double cost = 0.0;
  if (ok) {
    double q[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) q[i] = a.Q[10 * (int64_t)u + i] + a.Q[10 * (int64_t)v + i];
    const Vec3d pu = load3(a.pos, u), pv = load3(a.pos, v);
    const Vec3d mid = {(pu.x + pv.x) * 0.5, (pu.y + pv.y) * 0.5, (pu.z + pv.z) * 0.5};
    const double c00 = q[4] * q[7] - q[5] * q[5], c01 = q[2] * q[5] - q[1] * q[7], c02 = q[1] * q[5] - q[2] * q[4];
    const double c11 = q[0] * q[7] - q[2] * q[2], c12 = q[1] * q[2] - q[0] * q[5], c22 = q[0] * q[4] - q[1] * q[1];
    const double det = (q[0] * c00 + q[1] * c01) + q[2] * c02;
    const double t3 = ((q[0] + q[4]) + q[7]) / 3.0;
    bool solved = false;
    if (det > 1e-3 * ((t3 * t3) * t3)) {
      const Vec3d s = {-(((c00 * q[3] + c01 * q[6]) + c02 * q[8]) / det), -(((c01 * q[3] + c11 * q[6]) + c12 * q[8]) / det),
                       -(((c02 * q[3] + c12 * q[6]) + c22 * q[8]) / det)};
      const Vec3d dm = {s.x - mid.x, s.y - mid.y, s.z - mid.z}, de = {pu.x - pv.x, pu.y - pv.y, pu.z - pv.z};
      if (dot3(dm, dm) <= 4.0 * dot3(de, de)) {
        x = round32(s);
        cost = quadric_cost(q, x);
        solved = true;
      }
    }
    if (!solved) {                     // the rounded midpoint, p_u, p_v: the first of the cheapest
      x = round32(mid);
      cost = quadric_cost(q, x);
      const double cu = quadric_cost(q, pu), cv = quadric_cost(q, pv);
      if (cu < cost) {
        x = pu;
        cost = cu;
      }
      if (cv < cost) {
        x = pv;
        cost = cv;
      }
    }
    cost = cost > 0.0 ? cost : 0.0;
    ok = !ring_flips(a, u, u, v, x) && !ring_flips(a, v, u, v, x);
  }
  a.key[e] = ok ? ((uint64_t)__float_as_uint((float)cost) << 32) | (uint64_t)e : KEY_NONE;
  a.cand[3 * e] = ok ? (float)x.x : 0.f;
  a.cand[3 * e + 1] = ok ? (float)x.y : 0.f;
  a.cand[3 * e + 2] = ok ? (float)x.z : 0.f;
}

__global__ __launch_bounds__(256) void mesh_collapse_m1_kernel(dfl_mesh_collapse_select_args a) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= a.V) return;
  uint64_t m = KEY_NONE;
  for (int32_t k = a.row_ptr[v]; k < a.row_ptr[v + 1]; ++k) {
    const uint64_t key = a.key[a.eid[k]];
    m = key < m ? key : m;
  }
  a.m1[v] = m;
}

__global__ __launch_bounds__(256) void mesh_collapse_m2_kernel(dfl_mesh_collapse_select_args a) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= a.V) return;
  uint64_t m = a.m1[v];
  for (int32_t k = a.row_ptr[v]; k < a.row_ptr[v + 1]; ++k) {
    const uint64_t o = a.m1[a.col[k]];
    m = o < m ? o : m;
  }
  a.m2[v] = m;
}

__global__ __launch_bounds__(256) void mesh_collapse_flag_kernel(dfl_mesh_collapse_select_args a) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.E) return;
  const uint64_t key = a.key[e];
  a.sel[e] = (key != KEY_NONE && a.m2[a.edge_u[e]] == key && a.m2[a.edge_v[e]] == key) ? 1 : 0;
}

// a gather over the edges at v: at most one of them is taken (the taken edges share no vertex)
__global__ __launch_bounds__(256) void mesh_collapse_vertex_kernel(dfl_mesh_collapse_apply_args a) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= a.V) return;
  int32_t to = (int32_t)v;
  float px = a.pos[3 * v], py = a.pos[3 * v + 1], pz = a.pos[3 * v + 2];
  for (int32_t k = a.row_ptr[v]; k < a.row_ptr[v + 1]; ++k) {
    const int64_t e = a.eid[k];
    if (!a.take[e]) continue;
    const int32_t w = a.col[k];
    if (w < v) {
      to = w;
    } else {
      px = a.cand[3 * e];
      py = a.cand[3 * e + 1];
      pz = a.cand[3 * e + 2];
    }
  }
  a.remap[v] = to;
  a.pos_out[3 * v] = px;
  a.pos_out[3 * v + 1] = py;
  a.pos_out[3 * v + 2] = pz;
}

// reads remap: launched after mesh_collapse_vertex_kernel on the same stream
__global__ __launch_bounds__(256) void mesh_collapse_tris_kernel(dfl_mesh_collapse_apply_args a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.T) return;
  const int32_t p = a.remap[a.tris[3 * t]], q = a.remap[a.tris[3 * t + 1]], r = a.remap[a.tris[3 * t + 2]];
  a.tris_out[3 * t] = p;
  a.tris_out[3 * t + 1] = q;
  a.tris_out[3 * t + 2] = r;
  a.degen[t] = (p == q || q == r || r == p) ? 1 : 0;
}

inline unsigned dec_grid(int64_t n) { return (unsigned)ceil_div(n, 256); }
inline bool dec_count(int64_t n) { return n >= 1 && n < (1ll << 31); }

}  // namespace dfl

extern "C" int dfl_mesh_quadrics(const dfl_mesh_quadrics_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr && a->pos && a->tris && a->vt_ptr && a->vt_tri && a->Q,
              "dfl_mesh_quadrics: pos, tris, vt_ptr, vt_tri and Q are required");
  DFL_REQUIRE(dfl::dec_count(a->V) && dfl::dec_count(a->T) && 3 * a->T < (1ll << 31),
              "dfl_mesh_quadrics: V and T must be at least 1, V and 3 T below 2^31");
  hipLaunchKernelGGL(dfl::mesh_quadrics_kernel, dim3(dfl::dec_grid(a->V)), dim3(256), 0, static_cast<hipStream_t>(stream), *a);
  return dfl::check_launch("dfl_mesh_quadrics");
}

extern "C" int dfl_mesh_collapse_keys(const dfl_mesh_collapse_keys_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr && a->pos && a->tris && a->row_ptr && a->col && a->use && a->vt_ptr && a->vt_tri && a->Q && a->edge_u &&
                  a->edge_v && a->key && a->cand,
              "dfl_mesh_collapse_keys: pos, tris, row_ptr, col, use, vt_ptr, vt_tri, Q, edge_u, edge_v, key and cand are required");
  DFL_REQUIRE(dfl::dec_count(a->V) && dfl::dec_count(a->T) && 3 * a->T < (1ll << 31) && dfl::dec_count(a->E) && 2 * a->E < (1ll << 31),
              "dfl_mesh_collapse_keys: V, T and E must be at least 1, V, 3 T and 2 E below 2^31");
  hipLaunchKernelGGL(dfl::mesh_collapse_keys_kernel, dim3(dfl::dec_grid(a->E)), dim3(256), 0, static_cast<hipStream_t>(stream), *a);
  return dfl::check_launch("dfl_mesh_collapse_keys");
}

extern "C" int dfl_mesh_collapse_select(const dfl_mesh_collapse_select_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr && a->row_ptr && a->col && a->eid && a->edge_u && a->edge_v && a->key && a->m1 && a->m2 && a->sel,
              "dfl_mesh_collapse_select: row_ptr, col, eid, edge_u, edge_v, key, m1, m2 and sel are required");
  DFL_REQUIRE(dfl::dec_count(a->V) && dfl::dec_count(a->E) && 2 * a->E < (1ll << 31),
              "dfl_mesh_collapse_select: V and E must be at least 1, V and 2 E below 2^31");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(dfl::mesh_collapse_m1_kernel, dim3(dfl::dec_grid(a->V)), dim3(256), 0, s, *a);
  hipLaunchKernelGGL(dfl::mesh_collapse_m2_kernel, dim3(dfl::dec_grid(a->V)), dim3(256), 0, s, *a);
  hipLaunchKernelGGL(dfl::mesh_collapse_flag_kernel, dim3(dfl::dec_grid(a->E)), dim3(256), 0, s, *a);
  return dfl::check_launch("dfl_mesh_collapse_select");
}

extern "C" int dfl_mesh_collapse_apply(const dfl_mesh_collapse_apply_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr && a->pos && a->tris && a->row_ptr && a->col && a->eid && a->take && a->cand && a->remap && a->pos_out &&
                  a->tris_out && a->degen,
              "dfl_mesh_collapse_apply: pos, tris, row_ptr, col, eid, take, cand, remap, pos_out, tris_out and degen are required");
  DFL_REQUIRE(dfl::dec_count(a->V) && dfl::dec_count(a->T) && 3 * a->T < (1ll << 31) && dfl::dec_count(a->E) && 2 * a->E < (1ll << 31),
              "dfl_mesh_collapse_apply: V, T and E must be at least 1, V, 3 T and 2 E below 2^31");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(dfl::mesh_collapse_vertex_kernel, dim3(dfl::dec_grid(a->V)), dim3(256), 0, s, *a);
  hipLaunchKernelGGL(dfl::mesh_collapse_tris_kernel, dim3(dfl::dec_grid(a->T)), dim3(256), 0, s, *a);
  return dfl::check_launch("dfl_mesh_collapse_apply");
}
