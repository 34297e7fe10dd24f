// Triangle rasteriser of the 3D scene (examples/full_res_3d_viz.py --png): a visibility buffer of 64-bit keys
// (depth bits, primitive id) filled by the integer atomic minimum, then one shading pass per sample and a box resolve.
// Contract and arithmetic: include/dfl_hip.h "Rasteriser" (DESIGN.md section 22); tests/raster_ref.py restates it.
// Built with -ffp-contract=off: every product and sum is rounded on its own.
//
// Launches: rs_clear_kernel (visibility buffer, counters, the per-record tables), rs_tris_kernel (one thread per
// triangle: set-up, then either the walk over a small box or an entry of the large list), rs_large_kernel (the large
// list: workgroups over 64 x 64 tiles of each box), rs_shade_kernel (one thread per sample), rs_resolve_kernel (one
// thread per pixel).  The only atomics are integer ones: the 64-bit minimum, the four counters and the list cursor;
// none of them lets arrival order reach a result (the list's order does not matter: its entries meet in the minimum).
#include "common.h"

namespace dfl {

constexpr uint64_t RS_EMPTY = ~0ull;
constexpr int RS_LARGE_GX = 32, RS_LARGE_GY = 256;   // rs_large_kernel's grid: entries stride x, tiles of an entry stride y

// scratch: vis u64 [S] | col u32 [S] | header | large list uint4 [DFL_RASTER_MAX_LARGE] (record, triangle, tiles, 0) | tri_base i64 [n_mesh + 1] |
// prim_base u32 [n_mesh (+1 to keep 8 bytes)]
struct RsHeader {
  uint32_t n_large;
  int32_t counts[4];
  int32_t pad[3];
};
struct RsLayout {
  uint64_t* vis;
  uint32_t* col;
  RsHeader* hdr;
  uint4* large;
  int64_t* tri_base;
  uint32_t* prim_base;
};

__host__ __device__ inline int64_t rs_scratch_bytes(int64_t S, int64_t n_mesh) {
  return S * 8 + ((S + 1) / 2) * 8 + (int64_t)sizeof(RsHeader) + (int64_t)DFL_RASTER_MAX_LARGE * 16 + (n_mesh + 1) * 8 + ((n_mesh + 1) / 2) * 8;
}
__host__ __device__ inline RsLayout rs_layout(void* scratch, int64_t S, int64_t n_mesh) {
  RsLayout L;
  char* p = static_cast<char*>(scratch);
  L.vis = reinterpret_cast<uint64_t*>(p);
  p += S * 8;
  L.col = reinterpret_cast<uint32_t*>(p);
  p += ((S + 1) / 2) * 8;                              // (rounded up: what follows stays 8-aligned)
  L.hdr = reinterpret_cast<RsHeader*>(p);
  p += sizeof(RsHeader);
  L.large = reinterpret_cast<uint4*>(p);
  p += (int64_t)DFL_RASTER_MAX_LARGE * 16;
  L.tri_base = reinterpret_cast<int64_t*>(p);
  p += (n_mesh + 1) * 8;
  L.prim_base = reinterpret_cast<uint32_t*>(p);
  return L;
}
constexpr uint32_t RS_LARGE_CAP = DFL_RASTER_MAX_LARGE;

struct RsView {            // what every kernel needs of dfl_raster_args
  const dfl_raster_mesh* meshes;
  RsLayout L;
  int32_t n_mesh, Ws, Hs;
  float half_w, half_h, znear;
};

struct RsTri {
  int32_t X[3], Y[3];
  float zd[3], w[3];
  int64_t A;               // |area|
  int32_t s;               // its sign
};

enum { RS_DRAWN = 0, RS_NEAR = 1, RS_GUARD = 2, RS_DEGENERATE = 3 };

// vertex stage and triangle set-up; idx = the three vertex indices (for the attributes)
__device__ __forceinline__ int rs_setup(const dfl_raster_mesh& m, int32_t t, const RsView& v, RsTri& T, int32_t* idx) {
  bool bad_index = false, behind = false, guard = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int32_t i = m.tris[(int64_t)t * 3 + k];
    idx[k] = i;
    if (i < 0 || i >= m.n_verts) {
      bad_index = true;
      continue;
    }
    const float x = m.pos[(int64_t)i * 3], y = m.pos[(int64_t)i * 3 + 1], z = m.pos[(int64_t)i * 3 + 2];
    float c[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) c[r] = ((m.mvp[4 * r] * x + m.mvp[4 * r + 1] * y) + m.mvp[4 * r + 2] * z) + m.mvp[4 * r + 3];
    const float w = c[3];
    if (!(isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]) && isfinite(w)) || w < v.znear) {
      behind = true;
      continue;
    }
    const float px = (c[0] / w + 1.0f) * v.half_w;
    const float py = (1.0f - c[1] / w) * v.half_h;
    const float X = rintf(256.0f * px), Y = rintf(256.0f * py);
    if (!(fabsf(X) <= 4194304.0f && fabsf(Y) <= 4194304.0f)) {
      guard = true;
      continue;
    }
    T.X[k] = (int32_t)X;
    T.Y[k] = (int32_t)Y;
    T.zd[k] = c[2] / w;
    T.w[k] = w;
  }
  if (bad_index) return RS_DEGENERATE;
  if (behind) return RS_NEAR;
  if (guard) return RS_GUARD;
  const int64_t A = (int64_t)(T.X[1] - T.X[0]) * (T.Y[2] - T.Y[0]) - (int64_t)(T.Y[1] - T.Y[0]) * (T.X[2] - T.X[0]);
  if (A == 0) return RS_DEGENERATE;
  T.s = A < 0 ? -1 : 1;
  T.A = A < 0 ? -A : A;
  return RS_DRAWN;
}

// samples whose centres lie in the triangle's bounding box, clamped to the image; false when there are none
__device__ __forceinline__ bool rs_box(const RsTri& T, const RsView& v, int& i0, int& i1, int& j0, int& j1) {
  const int32_t xmin = min(T.X[0], min(T.X[1], T.X[2])), xmax = max(T.X[0], max(T.X[1], T.X[2]));
  const int32_t ymin = min(T.Y[0], min(T.Y[1], T.Y[2])), ymax = max(T.Y[0], max(T.Y[1], T.Y[2]));
  i0 = max((xmin + 127) >> 8, 0);                      // ceil((xmin - 128) / 256)
  i1 = min((xmax - 128) >> 8, v.Ws - 1);               // floor((xmax - 128) / 256)
  j0 = max((ymin + 127) >> 8, 0);
  j1 = min((ymax - 128) >> 8, v.Hs - 1);
  return i0 <= i1 && j0 <= j1;
}

// coverage of sample (i, j) by the top-left rule and its barycentric weights l_k = E_k / |A|
__device__ __forceinline__ bool rs_cover(const RsTri& T, int i, int j, float* l) {
  const int32_t Px = 256 * i + 128, Py = 256 * j + 128;
  const float fA = (float)T.A;
  bool in = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int a = (k + 1) % 3, b = (k + 2) % 3;
    const int64_t dx = (int64_t)T.s * (T.X[b] - T.X[a]), dy = (int64_t)T.s * (T.Y[b] - T.Y[a]);
    const int64_t E = dx * (Py - T.Y[a]) - dy * (Px - T.X[a]);
    in = in && (E > 0 || (E == 0 && (dy < 0 || (dy == 0 && dx > 0))));
    l[k] = (float)E / fA;
  }
  return in;
}

__device__ __forceinline__ void rs_sample(const RsTri& T, const RsView& v, uint32_t prim, int i, int j) {
  float l[3];
  if (!rs_cover(T, i, j, l)) return;
  float d = (l[0] * T.zd[0] + l[1] * T.zd[1]) + l[2] * T.zd[2];
  if (!(d >= 0.0f && d <= 1.0f)) return;
  if (d == 0.0f) d = 0.0f;                             // -0 -> +0: the bits order as the values do
  const uint64_t key = ((uint64_t)__float_as_uint(d) << 32) | prim;
  atomicMin(reinterpret_cast<unsigned long long*>(v.L.vis + (int64_t)j * v.Ws + i), (unsigned long long)key);
}

// last m with base[m] <= g (base ascending, base[0] <= g)
template <typename B, typename G>
__device__ __forceinline__ int rs_find(const B* base, int n, G g) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((G)base[mid] <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ void __launch_bounds__(256) rs_clear_kernel(const RsView v) {
  const int64_t S = (int64_t)v.Ws * v.Hs;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < S; p += (int64_t)gridDim.x * 256) v.L.vis[p] = RS_EMPTY;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    v.L.hdr->n_large = 0;
    for (int k = 0; k < 4; ++k) v.L.hdr->counts[k] = 0;
    int64_t base = 0;
    for (int m = 0; m < v.n_mesh; ++m) {
      v.L.tri_base[m] = base;
      v.L.prim_base[m] = v.meshes[m].first_prim;
      base += v.meshes[m].n_tris;
    }
    v.L.tri_base[v.n_mesh] = base;
  }
}

__global__ void __launch_bounds__(256) rs_tris_kernel(const RsView v, const int64_t total) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  // records without triangles repeat their base: the search takes the last of equal bases, which is the one that has them
  const int mi = g < total ? rs_find(v.L.tri_base, v.n_mesh, g) : 0;
  const dfl_raster_mesh& m = v.meshes[mi];
  const int32_t t = g < total ? (int32_t)(g - v.L.tri_base[mi]) : 0;
  RsTri T;
  int32_t idx[3];
  const int st = g < total ? rs_setup(m, t, v, T, idx) : -1;
#pragma unroll
  for (int k = 1; k < 4; ++k) {                        // one addition per wave and counter; the drawn ones are the rest (rs_resolve_kernel):
                                                       // counting them here would send every wave of the launch to one address
    const unsigned long long votes = __ballot(st == k);
    if (votes != 0 && (threadIdx.x & 63) == 0) atomicAdd(&v.L.hdr->counts[k], (int)__popcll(votes));
  }
  if (st != RS_DRAWN) return;
  int i0, i1, j0, j1;
  if (!rs_box(T, v, i0, i1, j0, j1)) return;
  if (i1 - i0 >= DFL_RASTER_SMALL_BOX || j1 - j0 >= DFL_RASTER_SMALL_BOX) {
    const uint32_t slot = atomicAdd(&v.L.hdr->n_large, 1u);
    if (slot < RS_LARGE_CAP) {
      const uint32_t tiles = (uint32_t)(((i1 - i0) / DFL_RASTER_TILE + 1) * ((j1 - j0) / DFL_RASTER_TILE + 1));
      v.L.large[slot] = make_uint4((uint32_t)mi, (uint32_t)t, tiles, 0u);
      return;
    }
  }
  const uint32_t prim = m.first_prim + (uint32_t)t;
  for (int j = j0; j <= j1; ++j)
    for (int i = i0; i <= i1; ++i) rs_sample(T, v, prim, i, j);
}

// grid (RS_LARGE_GX, RS_LARGE_GY): block (bx, by) takes the entries bx, bx + GX, ... and of each the tiles by, by + GY, ...;
// the tile count in the entry lets a block pass over the entries that have no tile for it before any set-up
__global__ void __launch_bounds__(256) rs_large_kernel(const RsView v) {
  const uint32_t n = min(v.L.hdr->n_large, RS_LARGE_CAP);
  for (uint32_t e = blockIdx.x; e < n; e += gridDim.x) {
    const uint4 ent = v.L.large[e];
    if (blockIdx.y >= ent.z) continue;
    const dfl_raster_mesh& m = v.meshes[ent.x];
    RsTri T;
    int32_t idx[3];
    if (rs_setup(m, (int32_t)ent.y, v, T, idx) != RS_DRAWN) continue;      // (never: it was drawn when it was listed)
    int i0, i1, j0, j1;
    if (!rs_box(T, v, i0, i1, j0, j1)) continue;
    const uint32_t prim = m.first_prim + ent.y;
    const int ntx = (i1 - i0) / DFL_RASTER_TILE + 1, nty = (j1 - j0) / DFL_RASTER_TILE + 1;
    for (int tile = blockIdx.y; tile < ntx * nty; tile += gridDim.y) {
      const int ti = i0 + (tile % ntx) * DFL_RASTER_TILE, tj = j0 + (tile / ntx) * DFL_RASTER_TILE;
      for (int p = threadIdx.x; p < DFL_RASTER_TILE * DFL_RASTER_TILE; p += 256) {
        const int i = ti + (p % DFL_RASTER_TILE), j = tj + (p / DFL_RASTER_TILE);
        if (i <= i1 && j <= j1) rs_sample(T, v, prim, i, j);
      }
    }
  }
}

__device__ __forceinline__ float rs_unit(float c) { return fminf(fmaxf(c, 0.0f), 1.0f); }
__device__ __forceinline__ uint32_t rs_byte(float c) { return (uint32_t)rintf(255.0f * rs_unit(c)); }
__device__ __forceinline__ float rs_mix(const float* b, float q0, float q1, float q2) { return (b[0] * q0 + b[1] * q1) + b[2] * q2; }

__global__ void __launch_bounds__(256) rs_shade_kernel(const RsView v, const float ambient, const float diffuse, const float bg0,
                                                       const float bg1, const float bg2, int32_t* __restrict__ ids,
                                                       float* __restrict__ depth) {
  const int64_t S = (int64_t)v.Ws * v.Hs;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= S) return;
  const uint64_t key = v.L.vis[p];
  if (key == RS_EMPTY) {
    v.L.col[p] = rs_byte(bg0) | (rs_byte(bg1) << 8) | (rs_byte(bg2) << 16);
    if (ids != nullptr) ids[p] = -1;
    if (depth != nullptr) depth[p] = INFINITY;
    return;
  }
  const uint32_t prim = (uint32_t)key;
  if (ids != nullptr) ids[p] = (int32_t)prim;
  if (depth != nullptr) depth[p] = __uint_as_float((uint32_t)(key >> 32));
  const int mi = rs_find(v.L.prim_base, v.n_mesh, prim);
  const dfl_raster_mesh& m = v.meshes[mi];
  RsTri T;
  int32_t idx[3];
  (void)rs_setup(m, (int32_t)(prim - m.first_prim), v, T, idx);            // the set-up that drew it, bit for bit
  const int j = (int)(p / v.Ws), i = (int)(p - (int64_t)j * v.Ws);
  float l[3], b[3];
  (void)rs_cover(T, i, j, l);
#pragma unroll
  for (int k = 0; k < 3; ++k) b[k] = l[k] / T.w[k];
  const float sum = (b[0] + b[1]) + b[2];
#pragma unroll
  for (int k = 0; k < 3; ++k) b[k] = b[k] / sum;
  float base[3] = {m.rgb[0], m.rgb[1], m.rgb[2]};
  if (m.flags & DFL_RASTER_TEXTURED) {
    const float u = rs_mix(b, m.uv[(int64_t)idx[0] * 2], m.uv[(int64_t)idx[1] * 2], m.uv[(int64_t)idx[2] * 2]);
    const float w = rs_mix(b, m.uv[(int64_t)idx[0] * 2 + 1], m.uv[(int64_t)idx[1] * 2 + 1], m.uv[(int64_t)idx[2] * 2 + 1]);
    // clamped as floats first: a far-off or NaN coordinate never reaches the conversion
    const float fx = fminf(fmaxf(floorf(u * (float)m.tw), 0.0f), (float)(m.tw - 1));
    const float fy = fminf(fmaxf(floorf(w * (float)m.th), 0.0f), (float)(m.th - 1));
    const float texel = (float)m.tex[(int64_t)(int)fy * m.tw + (int)fx] / 255.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) base[c] = base[c] * texel;
  }
  if (!(m.flags & DFL_RASTER_UNLIT)) {
    float n[3], r[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
      n[c] = rs_mix(b, m.nrm[(int64_t)idx[0] * 3 + c], m.nrm[(int64_t)idx[1] * 3 + c], m.nrm[(int64_t)idx[2] * 3 + c]);
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = (m.nmat[3 * c] * n[0] + m.nmat[3 * c + 1] * n[1]) + m.nmat[3 * c + 2] * n[2];
    const float len = sqrtf((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
    const float facing = len > 0.0f ? fabsf(r[2]) / len : 0.0f;
    const float intensity = ambient + diffuse * facing;
#pragma unroll
    for (int c = 0; c < 3; ++c) base[c] = base[c] * intensity;
  }
  v.L.col[p] = rs_byte(base[0]) | (rs_byte(base[1]) << 8) | (rs_byte(base[2]) << 16);
}

__global__ void __launch_bounds__(256) rs_resolve_kernel(const RsView v, const int W, const int H, const int ssaa,
                                                         unsigned char* __restrict__ rgb, int32_t* __restrict__ counts,
                                                         const int32_t total) {
  if (counts != nullptr && blockIdx.x == 0 && threadIdx.x < 4) {
    const int32_t* c = v.L.hdr->counts;
    counts[threadIdx.x] = threadIdx.x == 0 ? total - c[1] - c[2] - c[3] : c[threadIdx.x];
  }
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (int64_t)W * H) return;
  const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
  uint32_t s0 = 0, s1 = 0, s2 = 0;
  for (int dy = 0; dy < ssaa; ++dy)
    for (int dx = 0; dx < ssaa; ++dx) {
      const uint32_t c = v.L.col[(int64_t)(y * ssaa + dy) * v.Ws + x * ssaa + dx];
      s0 += c & 255u;
      s1 += (c >> 8) & 255u;
      s2 += (c >> 16) & 255u;
    }
  const uint32_t n = (uint32_t)(ssaa * ssaa);
  rgb[p * 3] = (unsigned char)((s0 + n / 2) / n);
  rgb[p * 3 + 1] = (unsigned char)((s1 + n / 2) / n);
  rgb[p * 3 + 2] = (unsigned char)((s2 + n / 2) / n);
}

static bool rs_sizes_ok(int32_t W, int32_t H, int32_t ssaa, int32_t n_mesh) {
  return W >= 1 && H >= 1 && ssaa >= 1 && ssaa <= DFL_RASTER_MAX_SSAA && (int64_t)W * ssaa <= DFL_RASTER_MAX_DIM &&
         (int64_t)H * ssaa <= DFL_RASTER_MAX_DIM && n_mesh >= 0 && n_mesh <= DFL_RASTER_MAX_MESHES;
}

}  // namespace dfl

extern "C" int dfl_raster_scratch_bytes(int32_t W, int32_t H, int32_t ssaa, int32_t n_mesh) {
  if (!dfl::rs_sizes_ok(W, H, ssaa, n_mesh)) {
    dfl::set_error("dfl_raster_scratch_bytes: bad sizes (W %d, H %d, ssaa %d, n_mesh %d)", W, H, ssaa, n_mesh);
    return DFL_ERR_INVALID_ARG;
  }
  const int64_t bytes = dfl::rs_scratch_bytes((int64_t)W * ssaa * H * ssaa, n_mesh);
  if (bytes > INT32_MAX) {
    dfl::set_error("dfl_raster_scratch_bytes: %lld bytes, at most 2^31 - 1", (long long)bytes);
    return DFL_ERR_INVALID_ARG;
  }
  return (int)bytes;
}

extern "C" int dfl_raster_draw(const dfl_raster_args* a, dfl_stream_t stream) {
  using namespace dfl;
  DFL_REQUIRE(a != nullptr, "dfl_raster_draw: null args");
  DFL_REQUIRE(rs_sizes_ok(a->W, a->H, a->ssaa, a->n_mesh), "dfl_raster_draw: bad sizes (W %d, H %d, ssaa %d, n_mesh %d)", a->W, a->H,
              a->ssaa, a->n_mesh);
  DFL_REQUIRE(a->scratch != nullptr && a->rgb != nullptr, "dfl_raster_draw: scratch and rgb are required");
  DFL_REQUIRE((reinterpret_cast<uintptr_t>(a->scratch) & 7u) == 0, "dfl_raster_draw: scratch must be 8-byte aligned");
  DFL_REQUIRE(a->n_mesh == 0 || (a->meshes != nullptr && a->meshes_dev != nullptr),
              "dfl_raster_draw: meshes and meshes_dev are required");
  DFL_REQUIRE(a->znear > 0.0f, "dfl_raster_draw: znear must be positive");        // (refuses NaN too)
  const int32_t Ws = a->W * a->ssaa, Hs = a->H * a->ssaa;
  const int64_t S = (int64_t)Ws * Hs, need = rs_scratch_bytes(S, a->n_mesh);
  DFL_REQUIRE(need <= INT32_MAX, "dfl_raster_draw: %lld bytes of scratch, at most 2^31 - 1", (long long)need);
  DFL_REQUIRE(a->scratch_bytes >= need, "dfl_raster_draw: scratch of %d bytes is short of %lld", a->scratch_bytes, (long long)need);
  int64_t total = 0, next_prim = 0;
  for (int32_t k = 0; k < a->n_mesh; ++k) {
    const dfl_raster_mesh& m = a->meshes[k];
    DFL_REQUIRE(m.n_tris >= 0 && m.n_verts >= 0, "dfl_raster_draw: record %d: bad sizes", k);
    DFL_REQUIRE(m.n_tris == 0 || (m.pos != nullptr && m.tris != nullptr), "dfl_raster_draw: record %d: pos and tris are required", k);
    DFL_REQUIRE(m.nrm != nullptr || (m.flags & DFL_RASTER_UNLIT), "dfl_raster_draw: record %d: nrm is required unless unlit", k);
    DFL_REQUIRE(!(m.flags & DFL_RASTER_TEXTURED) || (m.uv != nullptr && m.tex != nullptr && m.tw > 0 && m.th > 0),
                "dfl_raster_draw: record %d: textured needs uv, tex, tw and th", k);
    DFL_REQUIRE((m.flags & ~(uint32_t)(DFL_RASTER_UNLIT | DFL_RASTER_TEXTURED)) == 0, "dfl_raster_draw: record %d: unknown flags", k);
    DFL_REQUIRE((int64_t)m.first_prim >= next_prim && (int64_t)m.first_prim + m.n_tris <= 0xffffffffll,
                "dfl_raster_draw: record %d: first_prim ranges must ascend without overlap below 0xffffffff", k);
    next_prim = (int64_t)m.first_prim + m.n_tris;
    total += m.n_tris;
  }
  DFL_REQUIRE(total <= INT32_MAX, "dfl_raster_draw: %lld triangles, at most 2^31 - 1", (long long)total);
  hipStream_t s = static_cast<hipStream_t>(stream);
  RsView v;
  v.meshes = a->meshes_dev;
  v.L = rs_layout(a->scratch, S, a->n_mesh);
  v.n_mesh = a->n_mesh;
  v.Ws = Ws;
  v.Hs = Hs;
  v.half_w = 0.5f * (float)Ws;
  v.half_h = 0.5f * (float)Hs;
  v.znear = a->znear;
  const int sample_blocks = (int)ceil_div(S, 256);
  hipLaunchKernelGGL(rs_clear_kernel, dim3(sample_blocks < 4096 ? sample_blocks : 4096), dim3(256), 0, s, v);
  if (total > 0) {
    hipLaunchKernelGGL(rs_tris_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, v, total);
    hipLaunchKernelGGL(rs_large_kernel, dim3(RS_LARGE_GX, RS_LARGE_GY), dim3(256), 0, s, v);
  }
  hipLaunchKernelGGL(rs_shade_kernel, dim3(sample_blocks), dim3(256), 0, s, v, a->ambient, a->diffuse, a->background[0],
                     a->background[1], a->background[2], a->ids, a->depth);
  hipLaunchKernelGGL(rs_resolve_kernel, dim3((unsigned)ceil_div((int64_t)a->W * a->H, 256)), dim3(256), 0, s, v, a->W, a->H, a->ssaa,
                     a->rgb, a->counts, (int32_t)total);
  return check_launch("dfl_raster_draw");
}
