// Clean-up of predicted label maps (include/dfl_hip.h, "Clean-up of predicted label maps"): connected components per value
// by union-find, selection of components, and a dilated mask.  Integer arithmetic and integer atomics only: every result
// is independent of the order in which workgroups and waves arrive.
//
// Components, three launches on the caller's stream, no host read-back and no waiting between workgroups:
//   1. label_tile_kernel    one workgroup per TH x TW tile, its labels resident in LDS: row runs by a wave ballot, then unions
//                           with the row above; writes the tile-local root of every pixel as a flat index and zeroes area / info
//   2. label_border_kernel  one thread per pixel on a tile border: unions with the backward neighbours in other tiles, in
//                           global memory (atomicMin on the parent array, which is the `root` output itself)
//   3. label_flatten_kernel root[p] = find(p) in place, area and info summed per run of a wave before the global atomic
//
// THE INVARIANT every loop below rests on: a parent link never points upwards -- parent[x] <= x, with parent[x] == x
// exactly at a root -- in LDS and in global memory, at every moment.  It holds after the initialisation (a pixel points to
// the start of its row run), and the only later writes are atomicMin(&parent[a], b) with b < a and, in phase 3, the store
// of a found root (<= every index on the path to it).  So a find() walks strictly downwards and takes at most as many
// steps as its start index, and a union() retry continues with a strictly smaller larger-end than before.
#include "common.h"

namespace dfl {
namespace {

constexpr int TH = DFL_LABEL_TILE_H, TW = DFL_LABEL_TILE_W, TPX = TH * TW;
constexpr int NT = 256, NW = NT / 64;
static_assert(TW == 64, "one wave walks one tile row");
static_assert(TH % NW == 0, "the waves share a tile's rows evenly");

// ---- union-find in LDS ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lds_find(const int* lab, int x) {
  for (;;) {   // terminates: lab[x] <= x, equal only at a root (the invariant above): x strictly falls
    const int p = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == x) return x;
    x = p;
  }
}
__device__ __forceinline__ void lds_union(int* lab, int a, int b) {
  for (;;) {   // terminates: max(a, b) strictly falls from one round to the next (old < a and b < a)
    a = lds_find(lab, a);
    b = lds_find(lab, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(lab + a, b);   // a retry only ever lowers a parent
    if (old == a) return;                    // a was a root and now hangs under b
    a = old;                                 // a had a parent already (old < a): that one and b are still to be united
  }
}

// ---- union-find in global memory: loads that bypass this CU's L1 (other workgroups lower parents meanwhile) -------------
__device__ __forceinline__ int g_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int g_find(const int* par, int x) {
  for (;;) {   // terminates: par[x] <= x, equal only at a root (the invariant above): x strictly falls
    const int p = g_load(par + x);
    if (p == x) return x;
    x = p;
  }
}
__device__ __forceinline__ void g_union(int* par, int a, int b) {
  for (;;) {   // terminates: max(a, b) strictly falls from one round to the next (old < a and b < a)
    a = g_find(par, a);
    b = g_find(par, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(par + a, b);   // a retry only ever lowers a parent
    if (old == a) return;
    a = old;
  }
}

// ---- phase 1 ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void label_tile_kernel(const unsigned char* __restrict__ segs, int* __restrict__ root,
                                                        int* __restrict__ area, unsigned* __restrict__ info, int H, int W,
                                                        int ntc, int tiles, int conn8) {
  __shared__ int lab[TPX];
  __shared__ short val[TPX];     // the pixel's value, -1 outside the image
  const int b = blockIdx.x / tiles, t = blockIdx.x % tiles;
  const int r0 = (t / ntc) * TH, c0 = (t % ntc) * TW;
  const int64_t base = (int64_t)b * H * W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = c0 + lane;
  for (int lr = wave; lr < TH; lr += NW) {
    const int r = r0 + lr;
    const int v = (r < H && c < W) ? (int)segs[base + (int64_t)r * W + c] : -1;
    // a pixel starts under the first pixel of its run within the tile row
    const int prev = __shfl_up(v, 1, 64);
    const unsigned long long heads = __ballot(lane == 0 || prev != v);
    const unsigned long long upto = heads & ((2ull << lane) - 1ull);   // lane 63: 2 << 63 wraps to 0, the mask to all ones
    lab[lr * TW + lane] = lr * TW + (63 - __clzll((long long)upto));
    val[lr * TW + lane] = (short)v;
  }
  __syncthreads();
  // unions with the row above; a union that the pixel to the left already stands for is left out (same run below, same run above)
  for (int lr = wave; lr < TH; lr += NW) {
    if (lr == 0) continue;
    const int i = lr * TW + lane;
    const int v = val[i];
    if (v < 0) continue;
    const bool left = lane > 0 && val[i - 1] == v;
    const bool upleft = lane > 0 && val[i - TW - 1] == v;
    if (val[i - TW] == v) {
      if (!(left && upleft)) lds_union(lab, i, i - TW);
    } else if (conn8) {
      if (upleft && !left) lds_union(lab, i, i - TW - 1);
      if (lane < TW - 1 && val[i - TW + 1] == v) lds_union(lab, i, i - TW + 1);
    }
  }
  __syncthreads();
  for (int lr = wave; lr < TH; lr += NW) {
    const int r = r0 + lr;
    if (r >= H || c >= W) continue;
    const int l = lds_find(lab, lr * TW + lane);
    const int64_t p = base + (int64_t)r * W + c;
    root[p] = (r0 + l / TW) * W + c0 + l % TW;   // the smallest flat index of the tile-local component
    area[p] = 0;
    info[p] = 0u;
  }
}

// ---- phase 2 ----------------------------------------------------------------------------------------------------------
// Items of an image: (ntr - 1) * W pixels of the first rows of tile rows 1.., then (ntc - 1) * H pixels of the first columns
// of tile columns 1.., then (8-connectivity) (ntc - 1) * H pixels of the last columns of tile columns 0..ntc-2.
__global__ __launch_bounds__(NT) void label_border_kernel(const unsigned char* __restrict__ segs, int* root, int H, int W,
                                                          int nhr, int nvc, int64_t per_image, int64_t total, int conn8) {
  const int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (g >= total) return;
  const int64_t b = g / per_image;
  int64_t k = g % per_image;
  const unsigned char* s = segs + b * H * W;
  int* par = root + b * H * W;
  if (k < (int64_t)nhr * W) {                       // first row of a tile: the three neighbours above are in other tiles
    const int r = (int)(k / W + 1) * TH, c = (int)(k % W);
    const int p = r * W + c, v = s[p];
    const bool left = c > 0 && s[p - 1] == v;
    const bool upleft = c > 0 && s[p - W - 1] == v;
    if (s[p - W] == v) {
      if (!(left && upleft)) g_union(par, p, p - W);
    } else if (conn8) {
      if (upleft && !left) g_union(par, p, p - W - 1);
      if (c + 1 < W && s[p - W + 1] == v) g_union(par, p, p - W + 1);
    }
    return;
  }
  k -= (int64_t)nhr * W;
  if (k < (int64_t)nvc * H) {                       // first column of a tile: left, and above-left unless the row case has it
    const int c = (int)(k / H + 1) * TW, r = (int)(k % H);
    const int p = r * W + c, v = s[p];
    const bool left = s[p - 1] == v;
    if (left) g_union(par, p, p - 1);
    if (conn8 && r > 0 && r % TH != 0 && !left && s[p - W] != v && s[p - W - 1] == v) g_union(par, p, p - W - 1);
    return;
  }
  k -= (int64_t)nvc * H;                            // last column of a tile (8-connectivity): above-right
  const int c = (int)(k / H + 1) * TW - 1, r = (int)(k % H);     // c + 1 = a tile's first column < W
  if (r == 0 || r % TH == 0) return;
  const int p = r * W + c, v = s[p];
  if (s[p - W] != v && s[p + 1] != v && s[p - W + 1] == v) g_union(par, p, p - W + 1);
}

// ---- phase 3 ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void label_flatten_kernel(const unsigned char* __restrict__ segs, int* root, int* area,
                                                           unsigned* info, int H, int W, int ntc, int tiles) {
  const int b = blockIdx.x / tiles, t = blockIdx.x % tiles;
  const int r0 = (t / ntc) * TH, c0 = (t % ntc) * TW;
  const int64_t base = (int64_t)b * H * W;
  const unsigned char* s = segs + base;
  int* par = root + base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = c0 + lane;
  for (int lr = wave; lr < TH; lr += NW) {          // (wave-uniform: every lane takes part in the shuffles below)
    const int r = r0 + lr;
    int rt = -1;
    unsigned bits = 0u;
    if (r < H && c < W) {
      const int p = r * W + c, v = s[p];
      // in place: whoever reads a parent meanwhile sees the old one or the root, and both lead to the root (a stored root is
      // <= every index on the path to it: the invariant holds).  The first hop q is the pixel's tile-local root, shared by
      // its neighbours in the tile: hanging it under the root as well spares them the walk beyond it.
      const int q = g_load(par + p), q2 = g_load(par + q);
      rt = q;
      if (q2 != q) {
        rt = g_find(par, q2);
        if (rt != q2) __hip_atomic_store(par + q, rt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      __hip_atomic_store(par + p, rt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (r == 0 || r == H - 1 || c == 0 || c == W - 1) bits = 0x80000000u;
      // a 4-neighbour of another value lies outside the component, one of the same value inside it
      int u;
      if (r > 0 && (u = s[p - W]) != v) bits |= 1u << (u < 30 ? u : 30);
      if (r < H - 1 && (u = s[p + W]) != v) bits |= 1u << (u < 30 ? u : 30);
      if (c > 0 && (u = s[p - 1]) != v) bits |= 1u << (u < 30 ? u : 30);
      if (c < W - 1 && (u = s[p + 1]) != v) bits |= 1u << (u < 30 ? u : 30);
    }
    // one atomic per run of equal roots in the wave's 64 pixels instead of one per pixel
    const int prev = __shfl_up(rt, 1, 64);
    const bool head = lane == 0 || prev != rt;
    const unsigned long long heads = __ballot(head);
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    const int end = above ? lane + 1 + __builtin_ctzll(above) : 64;
#pragma unroll
    for (int d = 1; d < 64; d *= 2) {
      const unsigned o = __shfl_down(bits, d, 64);
      if (lane + d < end) bits |= o;
    }
    if (head && rt >= 0) {
      atomicAdd(area + base + rt, end - lane);
      if (bits) atomicOr(info + base + rt, bits);
    }
  }
}

// ---- selection --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long comp_key(int area, int root) {
  return ((unsigned long long)(unsigned)area << 32) | (unsigned long long)(~(unsigned)root);
}

constexpr int SEL_PX = 4 * NT;     // pixels of one image per workgroup

__global__ __launch_bounds__(NT) void label_best_kernel(const unsigned char* __restrict__ segs, const int* __restrict__ area,
                                                        unsigned long long* best, int64_t HW, int chunks, int C) {
  __shared__ unsigned long long best_s[DFL_LABEL_MAX_CLASSES];
  const int b = blockIdx.x / chunks, ch = blockIdx.x % chunks;
  if (threadIdx.x < DFL_LABEL_MAX_CLASSES) best_s[threadIdx.x] = 0ull;
  __syncthreads();
  for (int j = 0; j < 4; ++j) {
    const int64_t p = (int64_t)ch * SEL_PX + j * NT + threadIdx.x;
    if (p >= HW) continue;
    const int a = area[b * HW + p], v = segs[b * HW + p];
    if (a > 0 && v >= 1 && v < C) atomicMax(&best_s[v], comp_key(a, (int)p));     // p is a root: area is 0 elsewhere
  }
  __syncthreads();
  if (threadIdx.x >= 1 && threadIdx.x < C && best_s[threadIdx.x] != 0ull) atomicMax(best + (int64_t)b * C + threadIdx.x, best_s[threadIdx.x]);
}

__global__ __launch_bounds__(NT) void label_select_kernel(const unsigned char* __restrict__ segs, const int* __restrict__ root,
                                                          const int* __restrict__ area, const unsigned* __restrict__ info,
                                                          const unsigned long long* __restrict__ best, unsigned char* __restrict__ out,
                                                          int* counts, int64_t HW, int chunks, int C, int keep, int min_area,
                                                          int fill_below) {
  __shared__ int cnt_s[DFL_LABEL_MAX_CLASSES];
  const int b = blockIdx.x / chunks, ch = blockIdx.x % chunks;
  if (threadIdx.x < DFL_LABEL_MAX_CLASSES) cnt_s[threadIdx.x] = 0;
  __syncthreads();
  const int64_t base = b * HW;
  for (int j = 0; j < 4; ++j) {
    const int64_t p = (int64_t)ch * SEL_PX + j * NT + threadIdx.x;
    if (p >= HW) continue;
    const int v = segs[base + p];
    int o = v;
    if (fill_below == 0) {
      if (v >= 1 && v < C) {
        const int rt = root[base + p], a = area[base + rt];
        const bool kept = a >= min_area && (keep == 0 || best[(int64_t)b * C + v] == comp_key(a, rt));
        if (!kept) {
          o = 0;
          atomicAdd(&cnt_s[v], 1);
        }
      }
    } else if (v == 0) {
      const int rt = root[base + p];
      const unsigned inf = info[base + rt], set = inf & 0x7fffffffu;
      if (!(inf >> 31) && area[base + rt] <= fill_below && __popc(set) == 1) {
        const int l = __ffs(set) - 1;
        if (l >= 1 && l < C && l < 30) {
          o = l;
          atomicAdd(&cnt_s[l], 1);
        }
      }
    }
    out[base + p] = (unsigned char)o;
  }
  __syncthreads();
  if (counts != nullptr && threadIdx.x < C && cnt_s[threadIdx.x] != 0)
    atomicAdd(counts + ((int64_t)b * C + threadIdx.x) * 2 + (fill_below == 0 ? 0 : 1), cnt_s[threadIdx.x]);
}

// ---- dilation ---------------------------------------------------------------------------------------------------------
// A disc is a stack of row segments: q = p + (dr, dc) lies in it when |dc| <= wid[|dr|], the largest w with w^2 + dr^2 <= r^2.
// Per tile: the in-set flags with a halo of r, per flag row the horizontal distance to the nearest set flag, then per
// pixel 2r + 1 comparisons.
constexpr int DTH = 16, DTW = 64, RMAX = DFL_LABEL_MAX_RADIUS;

__global__ __launch_bounds__(NT) void label_dilate_kernel(const unsigned char* __restrict__ segs, unsigned char* __restrict__ mask,
                                                          int H, int W, int ntc, int tiles, unsigned set, int rad) {
  __shared__ unsigned char flag[(DTH + 2 * RMAX) * (DTW + 2 * RMAX)];
  __shared__ unsigned char hd[(DTH + 2 * RMAX) * DTW];
  __shared__ unsigned char wid[RMAX + 1];
  const int b = blockIdx.x / tiles, t = blockIdx.x % tiles;
  const int r0 = (t / ntc) * DTH, c0 = (t % ntc) * DTW;
  const int64_t base = (int64_t)b * H * W;
  const int rows = DTH + 2 * rad, cols = DTW + 2 * rad;
  for (int i = threadIdx.x; i < rows * cols; i += NT) {
    const int r = r0 - rad + i / cols, c = c0 - rad + i % cols;
    unsigned char f = 0;
    if (r >= 0 && r < H && c >= 0 && c < W) {
      const int v = segs[base + (int64_t)r * W + c];
      f = (v < 32 && ((set >> v) & 1u)) ? 1 : 0;
    }
    flag[i] = f;
  }
  if ((int)threadIdx.x <= rad) {
    const int d = threadIdx.x;
    int w = 0;
    while ((w + 1) * (w + 1) + d * d <= rad * rad) ++w;     // w <= rad
    wid[d] = (unsigned char)w;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < rows * DTW; i += NT) {
    const unsigned char* row = flag + (i / DTW) * cols + rad + i % DTW;
    int dist = 255;
    for (int d = 0; d <= rad; ++d)
      if (row[-d] | row[d]) {
        dist = d;
        break;
      }
    hd[i] = (unsigned char)dist;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < DTH * DTW; i += NT) {
    const int lr = i / DTW, lc = i % DTW, r = r0 + lr, c = c0 + lc;
    if (r >= H || c >= W) continue;
    unsigned char m = 0;
    for (int dr = -rad; dr <= rad; ++dr)
      if (hd[(lr + rad + dr) * DTW + lc] <= wid[dr < 0 ? -dr : dr]) {
        m = 1;
        break;
      }
    mask[base + (int64_t)r * W + c] = m;
  }
}

// H * W < 2^31 and a grid that fits: checked before any pointer is looked at
int check_dims(const char* who, int32_t B, int32_t H, int32_t W) {
  DFL_REQUIRE(B > 0 && H > 0 && W > 0, "%s: bad sizes B=%d H=%d W=%d", who, B, H, W);
  DFL_REQUIRE((int64_t)H * W < (1ll << 31), "%s: H * W = %lld does not fit a 32-bit flat index", who, (long long)H * W);
  return DFL_OK;
}

}  // namespace
}  // namespace dfl

using namespace dfl;

extern "C" int dfl_label_components(const unsigned char* segs, int32_t B, int32_t H, int32_t W, int32_t connectivity,
                                    int32_t* root, int32_t* area, uint32_t* info, dfl_stream_t stream) {
  int rc = check_dims("dfl_label_components", B, H, W);
  if (rc != DFL_OK) return rc;
  DFL_REQUIRE(connectivity == 4 || connectivity == 8, "dfl_label_components: connectivity %d (4 or 8)", connectivity);
  DFL_REQUIRE(segs && root && area && info, "dfl_label_components: missing pointer");
  const int conn8 = connectivity == 8;
  const int64_t ntr = ceil_div(H, TH), ntc = ceil_div(W, TW), tiles = ntr * ntc;
  const int64_t per_image = (ntr - 1) * W + (ntc - 1) * H * (conn8 ? 2 : 1);
  const int64_t border_blocks = ceil_div(per_image * B, NT);
  DFL_REQUIRE(tiles * B < (1ll << 31) && border_blocks < (1ll << 31), "dfl_label_components: batch of %d images of %d x %d is too large for one grid", B, H, W);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(label_tile_kernel, dim3((unsigned)(tiles * B)), dim3(NT), 0, s, segs, root, area, info, (int)H, (int)W,
                     (int)ntc, (int)tiles, conn8);
  if ((rc = check_launch("dfl_label_components (tiles)")) != DFL_OK) return rc;
  if (border_blocks > 0) {     // (a matter of the shape, not of the data: an image of one tile has no border)
    hipLaunchKernelGGL(label_border_kernel, dim3((unsigned)border_blocks), dim3(NT), 0, s, segs, root, (int)H, (int)W,
                       (int)(ntr - 1), (int)(ntc - 1), per_image, per_image * B, conn8);
    if ((rc = check_launch("dfl_label_components (borders)")) != DFL_OK) return rc;
  }
  hipLaunchKernelGGL(label_flatten_kernel, dim3((unsigned)(tiles * B)), dim3(NT), 0, s, segs, root, area, info, (int)H, (int)W,
                     (int)ntc, (int)tiles);
  return check_launch("dfl_label_components (flatten)");
}

extern "C" int dfl_label_select_scratch_bytes(int32_t B, int32_t num_classes) {
  DFL_REQUIRE(B > 0 && num_classes >= 2 && num_classes <= DFL_LABEL_MAX_CLASSES, "dfl_label_select_scratch_bytes: bad sizes B=%d num_classes=%d", B, num_classes);
  DFL_REQUIRE((int64_t)B * num_classes * 8 < (1ll << 31), "dfl_label_select_scratch_bytes: batch of %d is too large", B);
  return (int)(B * num_classes * 8);
}

extern "C" int dfl_label_select(const unsigned char* segs, const int32_t* root, const int32_t* area, const uint32_t* info,
                                int32_t B, int32_t H, int32_t W, int32_t num_classes, int32_t keep, int32_t min_area,
                                int32_t fill_below, unsigned char* out, int32_t* counts, void* scratch, dfl_stream_t stream) {
  int rc = check_dims("dfl_label_select", B, H, W);
  if (rc != DFL_OK) return rc;
  DFL_REQUIRE(num_classes >= 2 && num_classes <= DFL_LABEL_MAX_CLASSES, "dfl_label_select: num_classes %d (2..%d)", num_classes, DFL_LABEL_MAX_CLASSES);
  DFL_REQUIRE((keep == 0 || keep == 1) && min_area >= 0 && fill_below >= 0, "dfl_label_select: keep %d (0 or 1), min_area %d, fill_below %d (not negative)", keep, min_area, fill_below);
  DFL_REQUIRE(segs && root && area && info && out && scratch, "dfl_label_select: missing pointer");
  DFL_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7u) == 0, "dfl_label_select: scratch is not 8-byte aligned");
  const int64_t HW = (int64_t)H * W, chunks = ceil_div(HW, SEL_PX);
  DFL_REQUIRE(chunks * B < (1ll << 31) && (int64_t)B * num_classes * 8 < (1ll << 31), "dfl_label_select: batch of %d images of %d x %d is too large for one grid", B, H, W);
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned long long* best = static_cast<unsigned long long*>(scratch);
  const bool largest = fill_below == 0 && keep == 1;
  if (largest && hipMemsetAsync(best, 0, (size_t)B * num_classes * 8, s) != hipSuccess) {
    set_error("dfl_label_select: hipMemsetAsync failed");
    return DFL_ERR_LAUNCH;
  }
  if (counts != nullptr && hipMemsetAsync(counts, 0, (size_t)B * num_classes * 2 * sizeof(int32_t), s) != hipSuccess) {
    set_error("dfl_label_select: hipMemsetAsync failed");
    return DFL_ERR_LAUNCH;
  }
  if (largest) {
    hipLaunchKernelGGL(label_best_kernel, dim3((unsigned)(chunks * B)), dim3(NT), 0, s, segs, area, best, HW, (int)chunks, (int)num_classes);
    if ((rc = check_launch("dfl_label_select (largest)")) != DFL_OK) return rc;
  }
  hipLaunchKernelGGL(label_select_kernel, dim3((unsigned)(chunks * B)), dim3(NT), 0, s, segs, root, area, info, best, out, counts, HW,
                     (int)chunks, (int)num_classes, (int)keep, (int)min_area, (int)fill_below);
  return check_launch("dfl_label_select");
}

extern "C" int dfl_label_dilate(const unsigned char* segs, int32_t B, int32_t H, int32_t W, uint32_t label_set, int32_t radius,
                                unsigned char* mask, dfl_stream_t stream) {
  int rc = check_dims("dfl_label_dilate", B, H, W);
  if (rc != DFL_OK) return rc;
  DFL_REQUIRE(radius >= 0 && radius <= DFL_LABEL_MAX_RADIUS, "dfl_label_dilate: radius %d (0..%d)", radius, DFL_LABEL_MAX_RADIUS);
  DFL_REQUIRE(segs && mask, "dfl_label_dilate: missing pointer");
  const int64_t ntr = ceil_div(H, DTH), ntc = ceil_div(W, DTW), tiles = ntr * ntc;
  DFL_REQUIRE(tiles * B < (1ll << 31), "dfl_label_dilate: batch of %d images of %d x %d is too large for one grid", B, H, W);
  hipLaunchKernelGGL(label_dilate_kernel, dim3((unsigned)(tiles * B)), dim3(NT), 0, static_cast<hipStream_t>(stream), segs, mask,
                     (int)H, (int)W, (int)ntc, (int)tiles, (unsigned)label_set, (int)radius);
  return check_launch("dfl_label_dilate");
}
