// Tools in a rendered view: the chords of analytic capsules (straight wires, drills, screws; a == b: beads) along every
// pixel's ray, added to the line integrals att [V][H][W] in place, one launch per batch of views.
// Contract: include/dfl_hip.h, "Tools" (dfl_tools_args, dfl_tools_capsule) -- the definition and the arithmetic, step by
// step; tests/tools_ref.py restates both in numpy.
//
// One thread per pixel and view; a wave covers 8 x 8 pixels (csrc/drr.h: drr_tile_pixel), a workgroup of four waves
// 16 x 16.  The tiles of a view are numbered along grid.x (column tiles fastest), the views along grid.z, so no image the
// entry point accepts runs out of grid.  The thread normalises its ray once and loops over the view's records, which
// every lane reads from the same address.  A record is skipped by the whole wave -- a branch on values all lanes share --
// when its pixel rectangle misses the wave's tile, and by a single lane when it misses the lane's pixel.
// No atomics, no LDS, nothing shared between threads: a pixel's bits depend on its own ray, the view's records and the
// old value alone.  Built with -ffp-contract=off: every product and sum is rounded as the numpy restatement rounds it.
#include "common.h"
#include "drr.h"

namespace dfl {

constexpr float TOOLS_PARALLEL = 1e-10f;   // |u_perp|^2 at or below this: the ray is parallel to the axis

__device__ __forceinline__ float tl_dot(float ax, float ay, float az, float bx, float by, float bz) { return ax * bx + ay * by + az * bz; }
__device__ __forceinline__ bool tl_finite(float x) { return fabsf(x) < __builtin_inff(); }

// The sphere of squared radius rr about p widens [t0, t1] along the unit ray u
__device__ __forceinline__ void tl_sphere(float ux, float uy, float uz, float px, float py, float pz, float rr, float& t0, float& t1) {
  const float tc = tl_dot(ux, uy, uz, px, py, pz);
  const float qx = px - tc * ux, qy = py - tc * uy, qz = pz - tc * uz;     // the offset as a vector, then its square
  const float h2 = rr - tl_dot(qx, qy, qz, qx, qy, qz);
  if (h2 >= 0.f) {
    const float h = sqrtf(h2);
    t0 = fminf(t0, tc - h);
    t1 = fmaxf(t1, tc + h);
  }
}

// The chord in mm of one capsule along the unit ray u from the origin
__device__ __forceinline__ float tl_chord(const dfl_tools_capsule& k, float ux, float uy, float uz) {
  const float ax = k.a[0], ay = k.a[1], az = k.a[2], bx = k.b[0], by = k.b[1], bz = k.b[2];
  const float rr = k.r * k.r;
  float t0 = __builtin_inff(), t1 = -__builtin_inff();
  tl_sphere(ux, uy, uz, ax, ay, az, rr, t0, t1);
  tl_sphere(ux, uy, uz, bx, by, bz, rr, t0, t1);
  const float wx = bx - ax, wy = by - ay, wz = bz - az;
  const float L = sqrtf(tl_dot(wx, wy, wz, wx, wy, wz));
  if (L > 0.f) {
    const float ex = wx / L, ey = wy / L, ez = wz / L;
    const float ue = tl_dot(ux, uy, uz, ex, ey, ez);
    const float px = ux - ue * ex, py = uy - ue * ey, pz = uz - ue * ez;   // u_perp
    const float A = tl_dot(px, py, pz, px, py, pz);
    if (A > TOOLS_PARALLEL) {
      const float ae = tl_dot(ax, ay, az, ex, ey, ez);
      const float sx = ax - ae * ex, sy = ay - ae * ey, sz = az - ae * ez; // a_perp
      const float tcyl = tl_dot(px, py, pz, sx, sy, sz) / A;
      const float qx = sx - tcyl * px, qy = sy - tcyl * py, qz = sz - tcyl * pz;
      const float h2 = rr - tl_dot(qx, qy, qz, qx, qy, qz);
      if (h2 >= 0.f) {
        const float h = sqrtf(h2 / A);
        float c0 = tcyl - h, c1 = tcyl + h;
        bool keep;
        if (ue != 0.f) {
          const float s0 = ae / ue, s1 = (ae + L) / ue;
          c0 = fmaxf(c0, fminf(s0, s1));
          c1 = fminf(c1, fmaxf(s0, s1));
          keep = c1 >= c0;
        } else {
          keep = -ae >= 0.f && -ae <= L;
        }
        if (keep) {
          t0 = fminf(t0, c0);
          t1 = fmaxf(t1, c1);
        }
      }
    }
  }
  return fmaxf(t1 - fmaxf(t0, 0.f), 0.f);                                  // no piece hit: -inf -> 0
}

__global__ __launch_bounds__(256) void tools_kernel(const dfl_tools_args a, const int tiles_x) {
  const int H = a.H, W = a.W, n = a.n_tools;
  const int view = blockIdx.z;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wc0 = tx * 16 + (wave & 1) * 8, wr0 = ty * 16 + (wave >> 1) * 8;     // the wave's 8 x 8 tile
  const int col = wc0 + (lane & 7), row = wr0 + (lane >> 3);
  if (col >= W || row >= H) return;
  const float c = (float)col, r = (float)row;
  const float dx = drr_dot(a.qscale, c, r), dy = drr_dot(a.qscale + 3, c, r), dz = drr_dot(a.qscale + 6, c, r);
  const float nd = sqrtf(tl_dot(dx, dy, dz, dx, dy, dz));
  float s = 0.f, tl = 0.f;
  if (nd > 0.f && tl_finite(nd)) {
    const float ux = dx / nd, uy = dy / nd, uz = dz / nd;
    const dfl_tools_capsule* recs = a.tools + (int64_t)view * n;
    for (int j = 0; j < n; ++j) {
      const dfl_tools_capsule k = recs[j];
      if (!(k.r > 0.f)) continue;                                          // padding
      if (k.rect[0] > wc0 + 7 || k.rect[2] < wc0 || k.rect[1] > wr0 + 7 || k.rect[3] < wr0) continue;   // the whole wave
      if (!(tl_finite(k.a[0]) && tl_finite(k.a[1]) && tl_finite(k.a[2]) && tl_finite(k.b[0]) && tl_finite(k.b[1]) &&
            tl_finite(k.b[2]) && tl_finite(k.r) && tl_finite(k.mu)))
        continue;
      if (col < k.rect[0] || col > k.rect[2] || row < k.rect[1] || row > k.rect[3]) continue;
      const float len = tl_chord(k, ux, uy, uz);
      s = s + k.mu * len;
      tl = tl + len;
    }
  }
  const int64_t off = (int64_t)view * ((int64_t)H * W) + (int64_t)row * W + col;
  a.att[off] = a.att[off] + s;
  if (a.tool_len != nullptr) a.tool_len[off] = tl;
}

}  // namespace dfl

extern "C" int dfl_drr_tools(const dfl_tools_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_drr_tools: null args");
  DFL_REQUIRE(a->att != nullptr, "dfl_drr_tools: att is required");
  DFL_REQUIRE(a->n_tools >= 0 && a->n_tools <= DFL_TOOLS_MAX, "dfl_drr_tools: n_tools must be 0..%d per view, got %d", DFL_TOOLS_MAX,
              a->n_tools);
  DFL_REQUIRE(a->tools != nullptr || a->n_tools == 0, "dfl_drr_tools: %d tools per view need the tools array", a->n_tools);
  DFL_REQUIRE(a->views >= 1 && a->views <= 65535, "dfl_drr_tools: 1..65535 views per call, got %d", a->views);
  DFL_REQUIRE(a->H >= 1 && a->W >= 1, "dfl_drr_tools: bad sizes (an image of %d x %d)", a->H, a->W);
  DFL_REQUIRE((int64_t)a->H * a->W < ((int64_t)1 << 31), "dfl_drr_tools: an image of %d x %d has 2^31 pixels or more", a->H, a->W);
  for (int k = 0; k < 9; ++k)
    DFL_REQUIRE(a->qscale[k] - a->qscale[k] == 0.f, "dfl_drr_tools: qscale[%d] is not finite", k);
  if (a->n_tools == 0) return DFL_OK;
  const int64_t tiles_x = dfl::ceil_div(a->W, 16), tiles = tiles_x * dfl::ceil_div(a->H, 16);   // < 2^31 for H W < 2^31
  const dim3 grid((unsigned)tiles, 1, (unsigned)a->views);
  dfl::tools_kernel<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(*a, (int)tiles_x);
  return dfl::check_launch("dfl_drr_tools");
}
