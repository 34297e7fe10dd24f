// Outline cost: the truncated chamfer distance between the boundaries of S label sets in V moving label maps and in the
// fixed label maps they are scored against -- the similarity of dfl_amd.register(similarity='outline').
// Contract: include/dfl_hip.h ("Outline cost", dfl_sim_outline_args); the semantics are stated in DESIGN.md section 26 and
// restated in numpy float64 by tests/outline_ref.py.
//
// The inputs are the exact squared boundary distance maps of both sides (dfl_label_edt, boundary 1), [.][S][H][W] int32:
// a pixel is a boundary site of a map exactly where that map's own distance is 0, so no label map is read here.
//
// outline_chunk_kernel: a workgroup owns OUT_CHUNK consecutive pixels of one view (grid = chunks x views); thread t takes
// the pixels t, t + 256, ... of the chunk, so consecutive lanes read consecutive int32 of a plane.  It loops over the S
// sets and leaves ONE record of 4 S doubles per workgroup with plain stores: nM, nF (exact integers), a, b per set
// (csrc/fixed_sum.h: block_sum).  outline_finish_kernel: one workgroup per view; thread j < 4 S adds number j of the
// view's records in index order (records_sum), thread 0 then finishes every c_k and the cost in ascending k.
// No atomics: the bits of a view's numbers depend on that view's planes, its fixed map's planes, cap, S, H and W only.
// A view whose fixed_of entry is outside [0, F) reads no plane: cost NaN, counts and sums 0.
#include "common.h"
#include "fixed_sum.h"

namespace dfl {
namespace {

constexpr int OUT_THREADS = 256;
constexpr int OUT_CHUNK = DFL_SIM_OUTLINE_CHUNK;          // pixels of one view per workgroup
constexpr int OUT_PER = OUT_CHUNK / OUT_THREADS;          // ... per thread
constexpr int OUT_REC = 4;                                // nM, nF, a, b
constexpr int OUT_FINISH_THREADS = 128;                   // >= OUT_REC * DFL_LABEL_MAX_CLASSES
static_assert(OUT_CHUNK % OUT_THREADS == 0, "every thread takes the same number of pixels of a full chunk");
static_assert(OUT_REC * DFL_LABEL_MAX_CLASSES <= OUT_FINISH_THREADS, "one thread per number of a view's record");

// which fixed map a view is scored against: 0 without fixed_of, -1 when its entry is outside [0, F)
__device__ __forceinline__ int outline_map_of(const int32_t* __restrict__ fixed_of, int view, int F) {
  if (fixed_of == nullptr) return 0;
  const int f = fixed_of[view];
  return f >= 0 && f < F ? f : -1;
}

__global__ __launch_bounds__(OUT_THREADS) void outline_chunk_kernel(const int32_t* __restrict__ d2m, const int32_t* __restrict__ d2f,
                                                                    const int32_t* __restrict__ fixed_of, double* __restrict__ scratch,
                                                                    double cap, int S, int64_t HW, int F) {
  __shared__ double lds[OUT_REC * 4];
  const int chunk = blockIdx.x, view = blockIdx.y;
  const int f = outline_map_of(fixed_of, view, F);
  if (f < 0) return;                                        // the whole workgroup; outline_finish_kernel reads no record of this view
  const int64_t p0 = (int64_t)chunk * OUT_CHUNK + threadIdx.x;
  double* rec = scratch + ((size_t)view * gridDim.x + chunk) * S * OUT_REC;
  for (int k = 0; k < S; ++k) {
    const int32_t* __restrict__ pm = d2m + ((size_t)view * S + k) * HW;
    const int32_t* __restrict__ pf = d2f + ((size_t)f * S + k) * HW;
    double v[OUT_REC] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < OUT_PER; ++j) {
      const int64_t p = p0 + (int64_t)j * OUT_THREADS;
      if (p >= HW) continue;
      const int32_t m = pm[p], g = pf[p];
      if (m == 0) {                                         // a boundary site of the moving map: its distance to the fixed boundary
        v[0] += 1.0;
        v[2] += fmin(sqrt((double)g), cap);
      }
      if (g == 0) {                                         // a boundary site of the fixed map
        v[1] += 1.0;
        v[3] += fmin(sqrt((double)m), cap);
      }
    }
    block_sum<OUT_REC>(v, lds);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int i = 0; i < OUT_REC; ++i) rec[k * OUT_REC + i] = v[i];
    }
    __syncthreads();                                        // the next set's block_sum writes the LDS thread 0 just read
  }
}

__global__ __launch_bounds__(OUT_FINISH_THREADS) void outline_finish_kernel(const double* __restrict__ scratch,
                                                                            const int32_t* __restrict__ fixed_of,
                                                                            int32_t* __restrict__ counts, double* __restrict__ sums,
                                                                            double* __restrict__ cost, double cap, int S, int chunks, int F) {
  __shared__ double tot[OUT_FINISH_THREADS];
  const int view = blockIdx.x, per = S * OUT_REC;
  const bool inside = outline_map_of(fixed_of, view, F) >= 0;          // (the same for the whole workgroup)
  if ((int)threadIdx.x < per)
    tot[threadIdx.x] = inside ? records_sum(scratch + (size_t)view * chunks * per + threadIdx.x, chunks, per) : 0.0;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double total = 0.0;
  int scored = 0;
  for (int k = 0; k < S; ++k) {
    const double nM = tot[k * OUT_REC], nF = tot[k * OUT_REC + 1];
    double a = 0.0, b = 0.0;
    if (nM > 0.0 && nF > 0.0) {
      a = tot[k * OUT_REC + 2];
      b = tot[k * OUT_REC + 3];
      total += (a / nM + b / nF) / (2.0 * cap);
      ++scored;
    } else if (nM > 0.0 || nF > 0.0) {
      total += 1.0;
      ++scored;
    }
    const size_t o = ((size_t)view * S + k) * 2;
    counts[o] = (int32_t)nM;                                // exact: sums of integers far below 2^53
    counts[o + 1] = (int32_t)nF;
    sums[o] = a;
    sums[o + 1] = b;
  }
  cost[view] = !inside ? __builtin_nan("") : scored ? total / (double)scored : 1.0;
}

// sizes, then the size condition of dfl_label_edt (which also keeps H * W below 2^31): before any pointer is looked at
int outline_sizes_ok(const char* who, int32_t V, int32_t S, int32_t H, int32_t W) {
  DFL_REQUIRE(V >= 1 && V <= 65535, "%s: 1..65535 views per call, got %d", who, V);
  DFL_REQUIRE(S >= 1 && S <= DFL_LABEL_MAX_CLASSES, "%s: S %d label sets (1..%d)", who, S, DFL_LABEL_MAX_CLASSES);
  DFL_REQUIRE(H >= 1 && W >= 1, "%s: bad sizes H=%d W=%d", who, H, W);
  const int64_t far2 = (int64_t)(H - 1) * (H - 1) + (int64_t)(W - 1) * (W - 1);
  DFL_REQUIRE(far2 < (int64_t)DFL_LABEL_EDT_NONE, "%s: (H-1)^2 + (W-1)^2 = %lld of %d x %d does not fit an int32 squared distance", who,
              (long long)far2, H, W);
  return DFL_OK;
}

inline int64_t outline_chunks(int64_t H, int64_t W) { return ceil_div(H * W, OUT_CHUNK); }

}  // namespace
}  // namespace dfl

using namespace dfl;

extern "C" int dfl_sim_outline_scratch_doubles(int32_t V, int32_t S, int32_t H, int32_t W) {
  const int rc = outline_sizes_ok("dfl_sim_outline_scratch_doubles", V, S, H, W);
  if (rc != DFL_OK) return rc;
  const int64_t need = (int64_t)V * outline_chunks(H, W) * S * OUT_REC;
  DFL_REQUIRE(need < ((int64_t)1 << 31), "dfl_sim_outline_scratch_doubles: %d views of %d x %d with %d sets need %lld doubles: more than an int holds",
              V, H, W, S, (long long)need);
  return (int)need;
}

extern "C" int dfl_sim_outline(const dfl_sim_outline_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_sim_outline: null args");
  const int rc = outline_sizes_ok("dfl_sim_outline", a->V, a->S, a->H, a->W);
  if (rc != DFL_OK) return rc;
  DFL_REQUIRE(a->F >= 1, "dfl_sim_outline: F %d fixed maps (at least 1)", a->F);
  DFL_REQUIRE(a->cap > 0.0 && a->cap <= 1.7976931348623157e308, "dfl_sim_outline: a cap of %g pixels (finite and positive)", a->cap);
  DFL_REQUIRE(a->d2_moving != nullptr && a->d2_fixed != nullptr && a->counts != nullptr && a->sums != nullptr && a->cost != nullptr &&
                  a->scratch != nullptr,
              "dfl_sim_outline: d2_moving, d2_fixed, counts, sums, cost and scratch are required");
  const int64_t chunks = outline_chunks(a->H, a->W);        // < 2^31 / 1024: fits gridDim.x; V <= 65535 fits gridDim.y
  const int64_t need = (int64_t)a->V * chunks * a->S * OUT_REC;
  DFL_REQUIRE(a->scratch_doubles >= need, "dfl_sim_outline: a scratch of %lld doubles, %lld are needed (dfl_sim_outline_scratch_doubles)",
              (long long)a->scratch_doubles, (long long)need);
  hipStream_t s = static_cast<hipStream_t>(stream);
  outline_chunk_kernel<<<dim3((unsigned)chunks, (unsigned)a->V), OUT_THREADS, 0, s>>>(a->d2_moving, a->d2_fixed, a->fixed_of, a->scratch, a->cap,
                                                                                      a->S, (int64_t)a->H * a->W, a->F);
  outline_finish_kernel<<<(unsigned)a->V, OUT_FINISH_THREADS, 0, s>>>(a->scratch, a->fixed_of, a->counts, a->sums, a->cost, a->cap, a->S,
                                                                      (int)chunks, a->F);
  return check_launch("dfl_sim_outline");
}
