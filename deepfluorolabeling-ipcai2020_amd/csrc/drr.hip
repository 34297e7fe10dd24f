// Digitally reconstructed radiographs, per-label path lengths and a 2D label map from the CT and its 3D annotation.
// Contract: include/dfl_hip.h (dfl_drr_object, dfl_drr_args); the semantics are stated in DESIGN.md section 15 and
// restated in numpy float64 by tests/drr_ref.py.
//
// One thread per ray and view; the objects are looped over inside the thread, so the per-label lengths and the
// attenuation stay in registers and every output is written once, with no atomics.  A wave covers an 8 x 8 pixel tile
// (lane & 7, lane >> 3) and a workgroup of four waves 16 x 16: neighbouring rays walk neighbouring voxels (their label
// and mu cache lines are shared) and leave the box after about as many steps.  MAP = 1 is the 64 x 1 row mapping that
// tools/bench_drr.py compares against.
//
// Exact mode is an incremental grid traversal.  Per axis the thread keeps the INTEGER index k of the next plane it will
// cross and computes that crossing from it, t = (k - 1/2 - o) / d -- never t += dt, whose rounding would accumulate over
// several hundred steps.  The voxel index follows from the plane indices, so nothing is rounded to find it.  The box
// exit plane is one of these planes with the same formula, so the walk ends exactly at t1; the index test of the loop
// and the clamp in front of each load keep every address inside the volume whatever the arithmetic does.
// A run of voxels of one label adds s (t_end - t_start) to that label at once: the 16-way select that finds the
// accumulator (no register array is indexed with a run-time value) runs once per run, not once per voxel.
// mu is loaded only where the label passes the mask.
#include "drr.h"

namespace dfl {

struct DrrParams {
  DrrScene S;
  float* att;
  float* plen;
  unsigned char* label_map;
  int n_labels;
  float min_len_mm;
};

// Start of the walk on one axis: k = the first plane crossed after t0, i = the voxel index at t0+, step = +-1 (0: the
// axis is never crossed, tn = inf).  Planes lo .. hi + 1 bound the voxels lo .. hi; their t are monotonic in k.
__device__ __forceinline__ void drr_axis_start(float o, float d, int lo, int hi, float t0, int& k, int& i, int& step, float& tn) {
  const float p = fminf(fmaxf(o + t0 * d, (float)lo - 1.f), (float)hi + 1.f);
  const int est = min(max((int)floorf(p + 0.5f), lo), hi);
  if (d == 0.f) {
    step = 0;
    k = 0;
    i = est;
    tn = __builtin_inff();
    return;
  }
  if (d > 0.f) {
    step = 1;
    k = est + 1;                                         // smallest k in lo .. hi + 1 with t(k) > t0
    while (k > lo && drr_plane(k - 1, o, d) > t0) --k;
    while (k < hi + 1 && !(drr_plane(k, o, d) > t0)) ++k;
    i = max(k - 1, lo);
  } else {
    step = -1;
    k = est;                                             // largest k in lo .. hi + 1 with t(k) > t0
    while (k < hi + 1 && drr_plane(k + 1, o, d) > t0) ++k;
    while (k > lo && !(drr_plane(k, o, d) > t0)) --k;
    i = min(k, hi);
  }
  tn = drr_plane(k, o, d);
}

__device__ __forceinline__ void drr_flush(float (&acc)[DRR_NL], uint32_t label, float len) {
#pragma unroll
  for (int l = 0; l < DRR_NL; ++l) acc[l] += label == (uint32_t)l ? len : 0.f;
}

constexpr uint32_t DRR_NONE = 255u;         // "not in an admitted run"

template <bool PLEN>
__device__ __forceinline__ void drr_exact_object(const DrrScene& S, const dfl_drr_object& ob, float c, float r, float s, float& att,
                                                 float (&acc)[DRR_NL]) {
  DrrRay R;
  if (!drr_ray(ob, S.nx, S.ny, S.nz, c, r, R)) return;
  const float(&o)[3] = R.o, (&d)[3] = R.d, t0 = R.t0, t1 = R.t1;
  const int(&lo)[3] = R.lo, (&hi)[3] = R.hi;
  int k[3], i[3], step[3];
  float tn[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) drr_axis_start(o[a], d[a], lo[a], hi[a], t0, k[a], i[a], step[a], tn[a]);
  const uint32_t mask = ob.mask;
  const int sy = S.nx, sz = S.nx * S.ny;
  float t_cur = t0, run_start = t0;
  uint32_t run = DRR_NONE;
  // every step moves one index by one inside the box, so the trip count is bounded by the box's extent
  while (i[0] >= lo[0] && i[0] <= hi[0] && i[1] >= lo[1] && i[1] <= hi[1] && i[2] >= lo[2] && i[2] <= hi[2]) {
    const float t_next = fminf(fminf(tn[0], tn[1]), fminf(tn[2], t1));
    const int idx = i[2] * sz + i[1] * sy + i[0];
    const uint32_t lab = S.labels[idx];
    const bool in = lab < (uint32_t)DRR_NL && ((mask >> lab) & 1u) != 0u;
    if (in) att += (s * (t_next - t_cur)) * S.mu[idx];
    if (PLEN) {
      const uint32_t now = in ? lab : DRR_NONE;
      if (now != run) {
        if (run != DRR_NONE) drr_flush(acc, run, s * (t_cur - run_start));
        run = now;
        run_start = t_cur;
      }
    }
    t_cur = t_next;
    if (t_next >= t1) break;
    // the axis with the smallest crossing advances; equal crossings follow in the next trips with length 0
    const int a = tn[0] <= tn[1] ? (tn[0] <= tn[2] ? 0 : 2) : (tn[1] <= tn[2] ? 1 : 2);
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      if (b == a) {
        k[b] += step[b];
        i[b] += step[b];
        tn[b] = drr_plane(k[b], o[b], d[b]);
      }
    }
  }
  if (PLEN && run != DRR_NONE) drr_flush(acc, run, s * (t_cur - run_start));
}

__device__ __forceinline__ void drr_trilinear_object(const DrrScene& S, const dfl_drr_object& ob, float c, float r, float s, float& att) {
  DrrRay R;
  if (!drr_ray(ob, S.nx, S.ny, S.nz, c, r, R)) return;
  const DrrSamples sm = drr_samples(R, s, S.step_mm);
  float sum = 0.f;
  for (int j = 0; j < sm.N; ++j) {
    DrrCell C;
    drr_gather(S, ob.mask, R, R.t0 + ((float)j + 0.5f) * sm.dt, C);
    const float* v = C.v;                                  // v[x + 2 y + 4 z]
    const float a00 = v[0] + C.wx * (v[1] - v[0]), a10 = v[2] + C.wx * (v[3] - v[2]);
    const float a01 = v[4] + C.wx * (v[5] - v[4]), a11 = v[6] + C.wx * (v[7] - v[6]);
    const float b0 = a00 + C.wy * (a10 - a00), b1 = a01 + C.wy * (a11 - a01);
    sum += b0 + C.wz * (b1 - b0);
  }
  att += sm.w * sum;
}

// INTERP: DFL_DRR_EXACT / DFL_DRR_TRILINEAR; PLEN: plen or label_map is wanted; MAP 0: 8 x 8 tiles per wave, 1: 64 x 1
template <int INTERP, bool PLEN, int MAP>
__global__ __launch_bounds__(256) void drr_kernel(DrrParams P) {
  const DrrScene& S = P.S;
  int col, row;
  if (MAP == 0) {
    drr_tile_pixel(col, row);
  } else {
    col = blockIdx.x * 64 + (threadIdx.x & 63);
    row = blockIdx.y * 4 + (threadIdx.x >> 6);
  }
  if (col >= S.W || row >= S.H) return;
  const int view = blockIdx.z;
  const float c = (float)col, r = (float)row;
  const float s = drr_ray_scale(S.q, c, r);
  float att = 0.f;
  float acc[DRR_NL];
#pragma unroll
  for (int l = 0; l < DRR_NL; ++l) acc[l] = 0.f;
  const dfl_drr_object* obs = S.objects + (size_t)view * S.n_obj;
  for (int n = 0; n < S.n_obj; ++n) {
    if (INTERP == DFL_DRR_EXACT) drr_exact_object<PLEN>(S, obs[n], c, r, s, att, acc);
    else drr_trilinear_object(S, obs[n], c, r, s, att);
  }
  const size_t HW = (size_t)S.H * S.W, pix = (size_t)row * S.W + col;
  P.att[(size_t)view * HW + pix] = att;
  if (PLEN) {
    if (P.plen != nullptr) {
      float* pl = P.plen + (size_t)view * P.n_labels * HW + pix;
#pragma unroll
      for (int l = 0; l < DRR_NL; ++l)
        if (l < P.n_labels) pl[(size_t)l * HW] = acc[l];
    }
    if (P.label_map != nullptr) {
      float best = 0.f;
      int arg = 0;
#pragma unroll
      for (int l = 1; l < DRR_NL; ++l) {
        if (l < P.n_labels && (arg == 0 || acc[l] > best)) {
          best = acc[l];
          arg = l;
        }
      }
      P.label_map[(size_t)view * HW + pix] = (unsigned char)(arg != 0 && best >= P.min_len_mm ? arg : 0);
    }
  }
}

}  // namespace dfl

extern "C" int dfl_drr_render(const dfl_drr_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_drr_render: null args");
  DFL_REQUIRE(a->mu != nullptr && a->labels != nullptr && a->objects != nullptr && a->att != nullptr,
              "dfl_drr_render: mu, labels, objects and att are required");
  const int rc = dfl::drr_sizes_ok("dfl_drr_render", a->nx, a->ny, a->nz, a->H, a->W, a->views, a->n_obj);
  if (rc != DFL_OK) return rc;
  DFL_REQUIRE(a->n_labels >= 1 && a->n_labels <= DFL_DRR_MAX_LABELS, "dfl_drr_render: n_labels must be 1..%d, got %d",
              DFL_DRR_MAX_LABELS, a->n_labels);
  DFL_REQUIRE(a->interp == DFL_DRR_EXACT || a->interp == DFL_DRR_TRILINEAR, "dfl_drr_render: unknown interp %d (0 exact, 1 trilinear)",
              a->interp);
  DFL_REQUIRE(a->mapping == 0 || a->mapping == 1, "dfl_drr_render: unknown mapping %d (0: 8 x 8 tiles, 1: 64 x 1 rows)", a->mapping);
  DFL_REQUIRE(a->step_mm > 0.f && a->step_mm < __builtin_inff(), "dfl_drr_render: step_mm must be positive, got %g", (double)a->step_mm);
  DFL_REQUIRE(a->interp == DFL_DRR_EXACT || (a->plen == nullptr && a->label_map == nullptr),
              "dfl_drr_render: plen and label_map need the exact interpolation");
  DFL_REQUIRE(a->min_len_mm >= 0.f, "dfl_drr_render: min_len_mm must not be negative, got %g", (double)a->min_len_mm);
  const dfl::DrrParams P = {dfl::drr_scene_of(a), a->att, a->plen, a->label_map, a->n_labels, a->min_len_mm};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool plen = a->plen != nullptr || a->label_map != nullptr;
  const dim3 grid = a->mapping == 0 ? dim3((unsigned)dfl::ceil_div(a->W, 16), (unsigned)dfl::ceil_div(a->H, 16), (unsigned)a->views)
                                    : dim3((unsigned)dfl::ceil_div(a->W, 64), (unsigned)dfl::ceil_div(a->H, 4), (unsigned)a->views);
#define DRR_GO(INTERP, PLEN)                                               \
  if (a->mapping == 0) dfl::drr_kernel<INTERP, PLEN, 0><<<grid, 256, 0, s>>>(P); \
  else dfl::drr_kernel<INTERP, PLEN, 1><<<grid, 256, 0, s>>>(P)
  if (a->interp == DFL_DRR_TRILINEAR) {
    DRR_GO(DFL_DRR_TRILINEAR, false);
  } else if (plen) {
    DRR_GO(DFL_DRR_EXACT, true);
  } else {
    DRR_GO(DFL_DRR_EXACT, false);
  }
#undef DRR_GO
  return dfl::check_launch("dfl_drr_render");
}
