// Boundary distances of label maps (include/dfl_hip.h, "Boundary distances"): the exact squared
// Euclidean distance transform to the sites of a label set, and on top of it the surface-distance statistics of a
// predicted label map against the ground truth -- counts, maxima, sums of distances and order statistics.
//
// dfl_label_edt, separable as every exact EDT is:  dist2[r][c] = min over r' of (r - r')^2 + g2[r'][c], where
// g2[r'][c] = the squared distance from (r', c) to the nearest site OF ROW r' (EDT_NONE when that row has none).
//   pass 1  edt_rows_kernel   one wave per row of an (image, set): it walks the row in segments of 64 pixels from the left
//                             with the column of the last site seen (a ballot and a count of leading zeros per segment, no
//                             search), then from the right, and leaves g2; a row with a site sets the has-a-site word
//   pass 2  edt_cols_kernel   one workgroup per ER x 64 tile, lane = column, so that every row access is one contiguous
//                             segment; the g2 rows of the tile and EH rows above and below it are staged in LDS, rows
//                             beyond that window are read from global memory.  Per pixel a scan outwards from its row:
//                             k = 1, 2, .. looks at rows r - k and r + k and ends once k^2 >= the best so far.
// EXACT: a row at distance k contributes at least k^2, so once k^2 >= best no row further out can lower it, and every row
// nearer has been looked at; all sums are < 2^31 - 1 by the shape check.  TERMINATES: k rises by one per round and the loop
// also ends when both r - k and r + k have left the image, so at most max(r, H - 1 - r) rounds.
//
// The statistics and the select recompute the boundary test from est / gt per pixel; integers meet in LDS first and then
// by integer atomics, the sums of sqrt go through csrc/fixed_sum.h (one record per workgroup, added in index order).
#include "common.h"
#include "fixed_sum.h"

namespace dfl {
namespace {

constexpr int NT = 256, NW = NT / 64;
constexpr int NONE = DFL_LABEL_EDT_NONE;
constexpr int ER = 32, EH = 48, EWIN = ER + 2 * EH;      // pass 2: rows per tile, halo rows, rows of the LDS window
constexpr int PX = 4 * NT;                               // statistics: pixels of one image per workgroup
constexpr int SJ = 16, SPX = SJ * NT;                    // select: pixels of one image per workgroup
static_assert(ER % NW == 0 && EWIN % NW == 0, "the waves share a tile's rows evenly");

struct EdtSets {
  uint32_t v[DFL_LABEL_MAX_CLASSES];
};

__device__ __forceinline__ bool in_set(unsigned set, int v) { return v < 32 && ((set >> v) & 1u); }

// s = the image; (r, c) inside it
__device__ __forceinline__ bool is_site(const unsigned char* __restrict__ s, int H, int W, int r, int c, unsigned set, int boundary) {
  const int64_t p = (int64_t)r * W + c;
  if (!in_set(set, s[p])) return false;
  if (!boundary || r == 0 || r == H - 1 || c == 0 || c == W - 1) return true;
  return !(in_set(set, s[p - W]) && in_set(set, s[p + W]) && in_set(set, s[p - 1]) && in_set(set, s[p + 1]));
}

// ---- pass 1 -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void edt_rows_kernel(const unsigned char* __restrict__ segs, int* rowdist, int* has, EdtSets sets,
                                                      int S, int H, int W, int boundary, int64_t rows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t gw = (int64_t)blockIdx.x * NW + wave;
  if (gw >= rows) return;                                   // (wave-uniform: every lane of a wave takes part in the ballots)
  const int r = (int)(gw % H);
  const int64_t bs = gw / H;
  const unsigned set = sets.v[bs % S];
  const unsigned char* img = segs + (bs / S) * H * W;
  int* out = rowdist + (bs * H + r) * W;
  // from the left: the distance to the last site at or before the pixel, -1 when there is none yet
  int last = -1;
  for (int c0 = 0; c0 < W; c0 += 64) {
    const int c = c0 + lane;
    const unsigned long long m = __ballot(c < W && is_site(img, H, W, r, c, set, boundary));
    const unsigned long long upto = m & ((2ull << lane) - 1ull);     // lane 63: 2 << 63 wraps to 0, the mask to all ones
    const int left = upto ? c0 + 63 - __clzll((long long)upto) : last;
    if (c < W) out[c] = left >= 0 ? c - left : -1;
    if (m) last = c0 + 63 - __clzll((long long)m);
  }
  // from the right (a lane reads back what it stored itself: 0 exactly at a site), and the square of the smaller
  int next = -1;
  for (int c0 = ((W - 1) / 64) * 64; c0 >= 0; c0 -= 64) {
    const int c = c0 + lane;
    const int d = c < W ? out[c] : -1;
    const unsigned long long m = __ballot(c < W && d == 0);
    const unsigned long long from = m >> lane;
    const int right = from ? c + __builtin_ctzll(from) : next;
    int best = d;
    if (right >= 0 && (best < 0 || right - c < best)) best = right - c;
    if (c < W) out[c] = best < 0 ? NONE : best * best;               // best <= W - 1: the square fits (the shape check)
    if (m) next = c0 + __builtin_ctzll(m);
  }
  if (lane == 0 && last >= 0) atomicOr(has + bs, 1);
}

// ---- pass 2 -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void edt_cols_kernel(const int* __restrict__ rowdist, const int* __restrict__ has,
                                                      int* __restrict__ dist2, int H, int W, int ntc, int tiles) {
  __shared__ int win[EWIN * 64];      // (lane = column: consecutive lanes on consecutive banks)
  const int64_t bs = blockIdx.x / tiles;
  const int t = blockIdx.x % tiles;
  const int r0 = (t / ntc) * ER, c0 = (t % ntc) * 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = c0 + lane;
  const int* g = rowdist + bs * H * W;
  int* out = dist2 + bs * H * W;
  if (has[bs] == 0) {                 // (the same for the whole workgroup) no site in this image: no search
    for (int lr = wave; lr < ER; lr += NW)
      if (r0 + lr < H && c < W) out[(int64_t)(r0 + lr) * W + c] = NONE;
    return;
  }
  const int w0 = r0 - EH;
  for (int i = wave; i < EWIN; i += NW) {
    const int r = w0 + i;
    win[i * 64 + lane] = (r >= 0 && r < H && c < W) ? g[(int64_t)r * W + c] : NONE;
  }
  __syncthreads();
  for (int lr = wave; lr < ER; lr += NW) {
    const int r = r0 + lr;
    if (r >= H || c >= W) continue;
    int best = win[(lr + EH) * 64 + lane];
    // k <= H <= 46341: k * k fits 32 unsigned bits; v + kk <= (W-1)^2 + (H-1)^2 < 2^31 - 1
    for (int k = 1; (unsigned)k * (unsigned)k < (unsigned)best; ++k) {
      const int up = r - k, dn = r + k;
      if (up < 0 && dn >= H) break;
      const int kk = k * k;
      if (up >= 0) {
        const int v = up >= w0 ? win[(up - w0) * 64 + lane] : g[(int64_t)up * W + c];
        if (v != NONE && v + kk < best) best = v + kk;
      }
      if (dn < H) {
        const int v = dn < w0 + EWIN ? win[(dn - w0) * 64 + lane] : g[(int64_t)dn * W + c];
        if (v != NONE && v + kk < best) best = v + kk;
      }
    }
    out[(int64_t)r * W + c] = best;
  }
}

// ---- surface statistics -------------------------------------------------------------------------------------------------
// The entry of pixel p of image b in direction 0 (est -> gt) and 1 (gt -> est): the label it counts for (0: none) and the
// squared distance.  A pixel is a boundary site of {its own value} or of nothing.
struct Entry {
  int lab[2], d2[2];
};
__device__ __forceinline__ Entry entry_of(const unsigned char* __restrict__ est, const unsigned char* __restrict__ gt,
                                          const int* __restrict__ d2gt, const int* __restrict__ d2est, int64_t b, int H, int W,
                                          int64_t HW, int C, int64_t p) {
  Entry e;
  const int r = (int)(p / W), c = (int)(p % W);
  const unsigned char* img[2] = {est + b * HW, gt + b * HW};
  const int* dist[2] = {d2gt, d2est};
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const int v = img[d][p];
    e.lab[d] = 0;
    e.d2[d] = NONE;
    if (v >= 1 && v < C && is_site(img[d], H, W, r, c, 1u << v, 1)) {
      e.lab[d] = v;
      e.d2[d] = dist[d][(b * (C - 1) + v - 1) * HW + p];
    }
  }
  return e;
}

__global__ __launch_bounds__(NT) void surface_stats_kernel(const unsigned char* __restrict__ est, const unsigned char* __restrict__ gt,
                                                           const int* __restrict__ d2gt, const int* __restrict__ d2est, int* n,
                                                           int* max2, double* __restrict__ rec, int H, int W, int64_t HW,
                                                           int chunks, int C) {
  __shared__ int n_s[DFL_LABEL_MAX_CLASSES * 2], max_s[DFL_LABEL_MAX_CLASSES * 2];
  __shared__ double lds[2 * NW];
  const int64_t b = blockIdx.x / chunks;
  const int ch = blockIdx.x % chunks;
  if (threadIdx.x < DFL_LABEL_MAX_CLASSES * 2) n_s[threadIdx.x] = max_s[threadIdx.x] = 0;
  __syncthreads();
  int lab[4][2];
  double val[4][2];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t p = (int64_t)ch * PX + j * NT + threadIdx.x;
    lab[j][0] = lab[j][1] = 0;
    val[j][0] = val[j][1] = 0.0;
    if (p >= HW) continue;
    const Entry e = entry_of(est, gt, d2gt, d2est, b, H, W, HW, C, p);
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      if (e.lab[d] == 0) continue;
      atomicAdd(&n_s[(e.lab[d] - 1) * 2 + d], 1);
      if (e.d2[d] == NONE) continue;       // the other map has no boundary of this label: max2 and sum stay 0
      lab[j][d] = e.lab[d];
      val[j][d] = sqrt((double)e.d2[d]);
      atomicMax(&max_s[(e.lab[d] - 1) * 2 + d], e.d2[d]);
    }
  }
  __syncthreads();
  double* mine = rec + (b * chunks + ch) * (C - 1) * 2;
  for (int l = 1; l < C; ++l) {
    if (n_s[(l - 1) * 2] == 0 && n_s[(l - 1) * 2 + 1] == 0) {      // (the same for the whole workgroup)
      if (threadIdx.x < 2) mine[(l - 1) * 2 + threadIdx.x] = 0.0;
      continue;
    }
    double v[2] = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (lab[j][0] == l) v[0] += val[j][0];
      if (lab[j][1] == l) v[1] += val[j][1];
    }
    block_sum<2>(v, lds);
    if (threadIdx.x == 0) {
      mine[(l - 1) * 2] = v[0];
      mine[(l - 1) * 2 + 1] = v[1];
    }
    __syncthreads();
  }
  if (threadIdx.x < (C - 1) * 2) {
    const int64_t o = b * (C - 1) * 2 + threadIdx.x;
    if (n_s[threadIdx.x]) atomicAdd(n + o, n_s[threadIdx.x]);
    if (max_s[threadIdx.x]) atomicMax(max2 + o, max_s[threadIdx.x]);
  }
}

__global__ __launch_bounds__(NT) void surface_sum_kernel(const double* __restrict__ rec, double* __restrict__ sum, int64_t total,
                                                         int chunks, int per) {
  const int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (t >= total) return;
  const int64_t b = t / per;
  sum[t] = records_sum(rec + b * chunks * per + t % per, chunks, per);
}

// ---- radix select -------------------------------------------------------------------------------------------------------
// State per (b, l, j): hist[256], prefix (the key bytes found so far) and rem (the rank within the keys that share the
// prefix; < 0: nothing is looked for).
__global__ __launch_bounds__(NT) void select_init_kernel(const int* __restrict__ ranks, unsigned* prefix, int* rem, int64_t total) {
  const int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (t >= total) return;
  prefix[t] = 0u;
  rem[t] = ranks[t] < 0 ? -1 : ranks[t];
}

__global__ __launch_bounds__(NT) void select_hist_kernel(const unsigned char* __restrict__ est, const unsigned char* __restrict__ gt,
                                                         const int* __restrict__ d2gt, const int* __restrict__ d2est, int* hist,
                                                         const unsigned* __restrict__ prefix, const int* __restrict__ rem, int H,
                                                         int W, int64_t HW, int chunks, int C, int shift) {
  extern __shared__ int h[];          // [(C - 1) * 2][256]
  __shared__ unsigned pre_s[DFL_LABEL_MAX_CLASSES * 2];
  __shared__ int rem_s[DFL_LABEL_MAX_CLASSES * 2];
  const int64_t b = blockIdx.x / chunks;
  const int ch = blockIdx.x % chunks;
  const int per = (C - 1) * 2;
  for (int i = threadIdx.x; i < per * 256; i += NT) h[i] = 0;
  if (threadIdx.x < per) {
    pre_s[threadIdx.x] = prefix[b * per + threadIdx.x];
    rem_s[threadIdx.x] = rem[b * per + threadIdx.x];
  }
  __syncthreads();
  for (int j = 0; j < SJ; ++j) {
    const int64_t p = (int64_t)ch * SPX + j * NT + threadIdx.x;
    if (p >= HW) continue;
    const Entry e = entry_of(est, gt, d2gt, d2est, b, H, W, HW, C, p);
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      if (e.lab[d] == 0) continue;
      const unsigned key = (unsigned)e.d2[d];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int t = (e.lab[d] - 1) * 2 + q;
        if (rem_s[t] >= 0 && (shift == 24 || (key >> (shift + 8)) == pre_s[t])) atomicAdd(&h[t * 256 + ((key >> shift) & 255u)], 1);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < per * 256; i += NT)
    if (h[i]) atomicAdd(hist + b * per * 256 + i, h[i]);
}

__global__ __launch_bounds__(NT) void select_prefix_kernel(int* hist, unsigned* prefix, int* rem, int* __restrict__ kth2,
                                                           int64_t total, int last) {
  const int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (t >= total) return;
  int* hh = hist + t * 256;
  int r = rem[t], cum = 0, found = -1;
  for (int bin = 0; bin < 256; ++bin) {       // every bin is read and cleared for the next pass
    const int cnt = hh[bin];
    hh[bin] = 0;
    if (found < 0) {
      if (r >= 0 && cum + cnt > r) {
        found = bin;
        r -= cum;
      } else {
        cum += cnt;
      }
    }
  }
  unsigned pre = prefix[t];
  if (found < 0) r = -1;                      // a rank beyond the union (or none asked for)
  else pre = (pre << 8) | (unsigned)found;
  prefix[t] = pre;
  rem[t] = r;
  if (last) kth2[t] = r >= 0 ? (int)pre : -1;
}

// sizes, then (H-1)^2 + (W-1)^2 < 2^31 - 1 (which also keeps H * W below 2^31): before any pointer is looked at
int check_dims(const char* who, int32_t B, int32_t H, int32_t W) {
  DFL_REQUIRE(B > 0 && H > 0 && W > 0, "%s: bad sizes B=%d H=%d W=%d", who, B, H, W);
  const int64_t far2 = (int64_t)(H - 1) * (H - 1) + (int64_t)(W - 1) * (W - 1);
  DFL_REQUIRE(far2 < (int64_t)NONE, "%s: (H-1)^2 + (W-1)^2 = %lld of %d x %d does not fit an int32 squared distance", who,
              (long long)far2, H, W);
  return DFL_OK;
}

int check_classes(const char* who, int32_t num_classes) {
  DFL_REQUIRE(num_classes >= 2 && num_classes <= DFL_LABEL_MAX_CLASSES, "%s: num_classes %d (2..%d)", who, num_classes,
              DFL_LABEL_MAX_CLASSES);
  return DFL_OK;
}

int64_t surface_scratch(int64_t B, int64_t H, int64_t W, int64_t C) {
  const int64_t per = (C - 1) * 2;
  const int64_t stats = B * ceil_div(H * W, PX) * per * 8;
  const int64_t select = B * per * (256 * 4 + 8);
  return stats > select ? stats : select;
}

}  // namespace
}  // namespace dfl

using namespace dfl;

extern "C" int dfl_label_edt(const unsigned char* segs, int32_t B, int32_t H, int32_t W, const uint32_t* label_sets, int32_t S,
                             int32_t boundary, int32_t* rowdist, int32_t* dist2, dfl_stream_t stream) {
  int rc = check_dims("dfl_label_edt", B, H, W);
  if (rc != DFL_OK) return rc;
  DFL_REQUIRE(S >= 1 && S <= DFL_LABEL_MAX_CLASSES, "dfl_label_edt: S %d label sets (1..%d)", S, DFL_LABEL_MAX_CLASSES);
  DFL_REQUIRE(boundary == 0 || boundary == 1, "dfl_label_edt: boundary %d (0 or 1)", boundary);
  DFL_REQUIRE(segs && label_sets && rowdist && dist2, "dfl_label_edt: missing pointer");
  const int64_t BS = (int64_t)B * S, rows = BS * H;
  const int64_t ntc = ceil_div(W, 64), tiles = ceil_div(H, ER) * ntc;
  DFL_REQUIRE(ceil_div(rows, NW) < (1ll << 31) && tiles * BS < (1ll << 31), "dfl_label_edt: %d images of %d x %d with %d sets are too large for one grid", B, H, W, S);
  EdtSets sets = {};
  for (int s = 0; s < S; ++s) sets.v[s] = label_sets[s];
  hipStream_t st = static_cast<hipStream_t>(stream);
  int* has = rowdist + BS * H * W;
  if (hipMemsetAsync(has, 0, (size_t)BS * sizeof(int), st) != hipSuccess) {
    set_error("dfl_label_edt: hipMemsetAsync failed");
    return DFL_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(edt_rows_kernel, dim3((unsigned)ceil_div(rows, NW)), dim3(NT), 0, st, segs, rowdist, has, sets, (int)S, (int)H,
                     (int)W, (int)boundary, rows);
  if ((rc = check_launch("dfl_label_edt (rows)")) != DFL_OK) return rc;
  hipLaunchKernelGGL(edt_cols_kernel, dim3((unsigned)(tiles * BS)), dim3(NT), 0, st, rowdist, has, dist2, (int)H, (int)W, (int)ntc,
                     (int)tiles);
  return check_launch("dfl_label_edt (columns)");
}

extern "C" int dfl_label_surface_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t num_classes) {
  int rc = check_dims("dfl_label_surface_scratch_bytes", B, H, W);
  if (rc != DFL_OK) return rc;
  if ((rc = check_classes("dfl_label_surface_scratch_bytes", num_classes)) != DFL_OK) return rc;
  const int64_t bytes = surface_scratch(B, H, W, num_classes);
  DFL_REQUIRE(bytes < (1ll << 31), "dfl_label_surface_scratch_bytes: %d images of %d x %d need %lld bytes: more than an int holds", B, H, W, (long long)bytes);
  return (int)bytes;
}

namespace {
// the checks that dfl_label_surface_stats and dfl_label_surface_select share
int check_surface(const char* who, int32_t B, int32_t H, int32_t W, int32_t num_classes, bool pointers, const void* scratch) {
  int rc = check_dims(who, B, H, W);
  if (rc != DFL_OK) return rc;
  if ((rc = check_classes(who, num_classes)) != DFL_OK) return rc;
  DFL_REQUIRE(surface_scratch(B, H, W, num_classes) < (1ll << 31), "%s: %d images of %d x %d are too large for one call", who, B, H, W);
  DFL_REQUIRE(pointers && scratch, "%s: missing pointer", who);
  DFL_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7u) == 0, "%s: scratch is not 8-byte aligned", who);
  return DFL_OK;
}
}  // namespace

extern "C" int dfl_label_surface_stats(const unsigned char* est, const unsigned char* gt, int32_t B, int32_t H, int32_t W,
                                       int32_t num_classes, const int32_t* dist2_gt, const int32_t* dist2_est, int32_t* n,
                                       int32_t* max2, double* sum, void* scratch, dfl_stream_t stream) {
  int rc = check_surface("dfl_label_surface_stats", B, H, W, num_classes, est && gt && dist2_gt && dist2_est && n && max2 && sum, scratch);
  if (rc != DFL_OK) return rc;
  const int64_t HW = (int64_t)H * W, chunks = ceil_div(HW, PX), per = (num_classes - 1) * 2, total = B * per;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(n, 0, (size_t)total * sizeof(int32_t), st) != hipSuccess || hipMemsetAsync(max2, 0, (size_t)total * sizeof(int32_t), st) != hipSuccess) {
    set_error("dfl_label_surface_stats: hipMemsetAsync failed");
    return DFL_ERR_LAUNCH;
  }
  double* rec = static_cast<double*>(scratch);
  hipLaunchKernelGGL(surface_stats_kernel, dim3((unsigned)(chunks * B)), dim3(NT), 0, st, est, gt, dist2_gt, dist2_est, n, max2, rec,
                     (int)H, (int)W, HW, (int)chunks, (int)num_classes);
  if ((rc = check_launch("dfl_label_surface_stats")) != DFL_OK) return rc;
  hipLaunchKernelGGL(surface_sum_kernel, dim3((unsigned)ceil_div(total, NT)), dim3(NT), 0, st, rec, sum, total, (int)chunks, (int)per);
  return check_launch("dfl_label_surface_stats (sums)");
}

extern "C" int dfl_label_surface_select(const unsigned char* est, const unsigned char* gt, int32_t B, int32_t H, int32_t W,
                                        int32_t num_classes, const int32_t* dist2_gt, const int32_t* dist2_est,
                                        const int32_t* ranks, int32_t* kth2, void* scratch, dfl_stream_t stream) {
  int rc = check_surface("dfl_label_surface_select", B, H, W, num_classes, est && gt && dist2_gt && dist2_est && ranks && kth2, scratch);
  if (rc != DFL_OK) return rc;
  const int64_t HW = (int64_t)H * W, chunks = ceil_div(HW, SPX), per = (num_classes - 1) * 2, total = B * per;
  hipStream_t st = static_cast<hipStream_t>(stream);
  int* hist = static_cast<int*>(scratch);
  unsigned* prefix = reinterpret_cast<unsigned*>(hist + total * 256);
  int* rem = reinterpret_cast<int*>(prefix + total);
  if (hipMemsetAsync(hist, 0, (size_t)total * 256 * sizeof(int), st) != hipSuccess) {
    set_error("dfl_label_surface_select: hipMemsetAsync failed");
    return DFL_ERR_LAUNCH;
  }
  const unsigned small = (unsigned)ceil_div(total, NT);
  hipLaunchKernelGGL(select_init_kernel, dim3(small), dim3(NT), 0, st, ranks, prefix, rem, total);
  if ((rc = check_launch("dfl_label_surface_select (init)")) != DFL_OK) return rc;
  for (int shift = 24; shift >= 0; shift -= 8) {
    hipLaunchKernelGGL(select_hist_kernel, dim3((unsigned)(chunks * B)), dim3(NT), (size_t)per * 256 * sizeof(int), st, est, gt, dist2_gt,
                       dist2_est, hist, prefix, rem, (int)H, (int)W, HW, (int)chunks, (int)num_classes, shift);
    if ((rc = check_launch("dfl_label_surface_select (histogram)")) != DFL_OK) return rc;
    hipLaunchKernelGGL(select_prefix_kernel, dim3(small), dim3(NT), 0, st, hist, prefix, rem, kth2, total, shift == 0 ? 1 : 0);
    if ((rc = check_launch("dfl_label_surface_select (prefix)")) != DFL_OK) return rc;
  }
  return DFL_OK;
}
