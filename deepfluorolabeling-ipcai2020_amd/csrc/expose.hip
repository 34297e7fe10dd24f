// Detector model: rendered line integrals att [V][R][C] -> detector intensities, one launch per batch of views.
// Contract: include/dfl_hip.h (dfl_expose_args); the semantics are stated in DESIGN.md section 17 and restated in numpy
// by tests/expose_ref.py.
//
// A workgroup of 256 threads owns a tile of EX_TH x EX_TW = 16 x 64 pixels of one view (grid = column tiles x row tiles
// x views).  It stages T = expf(-att) for the tile and a halo of rho pixels on every side into LDS once -- indices
// clamped to the image, which is the edge replication of both passes, so images smaller than the tile or than the halo
// need no other case -- blurs along rows into a second LDS plane ((16 + 2 rho) x 64: the rows the column pass reads),
// and along columns into registers: thread t takes column t & 63 of rows (t >> 6) + 4 j, j = 0..3.  Consecutive lanes read
// consecutive LDS words in all three steps (no bank conflicts) and store consecutive pixels: 4 bytes per lane as
// fp32, 2 as uint16 -- every store is its own element, so odd C (rows that are only 2-byte aligned) is no special case.
// Each blur sum runs from tap 0 upwards.  Noise: csrc/philox.h, counter = the pixel index within the view.
// No atomics and nothing shared between workgroups: a view's bits depend on its own pixels, its keys, R, C and the
// parameters only.  Built with -ffp-contract=off: every product and sum is rounded as the numpy restatement rounds it.
#include "common.h"
#include "philox.h"

namespace dfl {

constexpr int EX_TH = 16, EX_TW = 64, EX_THREADS = 256;
constexpr int EX_SW = EX_TW + 2 * DFL_EXPOSE_MAX_RADIUS;   // leading dimension of the staged plane
constexpr int EX_SH = EX_TH + 2 * DFL_EXPOSE_MAX_RADIUS;
constexpr int EX_MAX_TILES = 65535;                        // per grid axis

template <bool U16>
__global__ __launch_bounds__(EX_THREADS) void expose_kernel(const dfl_expose_args a) {
  __shared__ float sT[EX_SH * EX_SW];                      // expf(-att), tile + halo
  __shared__ float sR[EX_SH * EX_TW];                      // after the row pass, tile columns, tile + halo rows
  const int rho = a.rho, R = a.R, C = a.C;
  const int v = blockIdx.z, r0 = blockIdx.y * EX_TH, c0 = blockIdx.x * EX_TW;
  const int64_t hw = (int64_t)R * C;
  const float* __restrict__ att = a.att + (int64_t)v * hw;
  const int sh = EX_TH + 2 * rho, sw = EX_TW + 2 * rho;
  const int nt = 2 * rho + 1;

  for (int idx = threadIdx.x; idx < sh * sw; idx += EX_THREADS) {
    const int lr = idx / sw, lc = idx - lr * sw;
    const int gr = min(max(r0 - rho + lr, 0), R - 1), gc = min(max(c0 - rho + lc, 0), C - 1);
    sT[lr * EX_SW + lc] = expf(-att[(int64_t)gr * C + gc]);
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < sh * EX_TW; idx += EX_THREADS) {
    const int lr = idx / EX_TW, lc = idx - lr * EX_TW;
    const float* row = sT + lr * EX_SW + lc;               // tap k reads column c - rho + k
    float acc = 0.f;
    for (int k = 0; k < nt; ++k) acc = acc + a.taps[k] * row[k];
    sR[lr * EX_TW + lc] = acc;
  }
  __syncthreads();

  const int lc = threadIdx.x & (EX_TW - 1), c = c0 + lc;
  if (c >= C) return;                                      // (no barrier follows)
  uint64_t kq = 0, ke = 0;
  if (a.quantum) kq = a.key_q[v];
  if (a.electronic) ke = a.key_e[v];
#pragma unroll
  for (int j = 0; j < EX_TH / 4; ++j) {
    const int lr = (threadIdx.x >> 6) + 4 * j, r = r0 + lr;
    if (r >= R) break;
    const float* col = sR + lr * EX_TW + lc;               // tap k reads row r - rho + k
    float B = 0.f;
    for (int k = 0; k < nt; ++k) B = B + a.taps[k] * col[k * EX_TW];
    const int64_t i = (int64_t)r * C + c;
    const float N = a.photons * B;
    float noisy = N;
    if (a.quantum) {
      const float z = aug_normal(kq, i);
      if (a.z1 != nullptr) a.z1[(int64_t)v * hw + i] = z;
      noisy = noisy + sqrtf(N) * z;
    }
    if (a.electronic) {
      const float z = aug_normal(ke, i);
      if (a.z2 != nullptr) a.z2[(int64_t)v * hw + i] = z;
      noisy = noisy + a.electronic_sigma * z;
    }
    const float I = a.gain * noisy;
    if (U16) {
      static_cast<uint16_t*>(a.out)[(int64_t)v * hw + i] = (uint16_t)rintf(fminf(fmaxf(I, 0.f), 65535.f));
    } else {
      static_cast<float*>(a.out)[(int64_t)v * hw + i] = I;
    }
  }
}

}  // namespace dfl

extern "C" int dfl_drr_expose(const dfl_expose_args* a, dfl_stream_t stream) {
  DFL_REQUIRE(a != nullptr, "dfl_drr_expose: null args");
  DFL_REQUIRE(a->att != nullptr && a->out != nullptr, "dfl_drr_expose: att and out are required");
  DFL_REQUIRE(a->V >= 1 && a->R >= 1 && a->C >= 1, "dfl_drr_expose: bad sizes (%d views of %d x %d)", a->V, a->R, a->C);
  DFL_REQUIRE(a->V <= 65535, "dfl_drr_expose: 1..65535 views per call, got %d", a->V);
  DFL_REQUIRE((int64_t)a->R * a->C < ((int64_t)1 << 31), "dfl_drr_expose: an image of %d x %d has 2^31 pixels or more", a->R, a->C);
  DFL_REQUIRE(dfl::ceil_div(a->R, dfl::EX_TH) <= dfl::EX_MAX_TILES && dfl::ceil_div(a->C, dfl::EX_TW) <= dfl::EX_MAX_TILES,
              "dfl_drr_expose: an image of %d x %d needs more than 65535 tiles along an axis", a->R, a->C);
  DFL_REQUIRE(a->rho >= 0 && a->rho <= DFL_EXPOSE_MAX_RADIUS, "dfl_drr_expose: a blur radius rho of %d (0..%d are supported)", a->rho,
              DFL_EXPOSE_MAX_RADIUS);
  DFL_REQUIRE(a->photons > 0.f && a->photons < INFINITY, "dfl_drr_expose: photons must be positive and finite, got %g", (double)a->photons);
  DFL_REQUIRE(a->gain > 0.f && a->gain < INFINITY, "dfl_drr_expose: gain must be positive and finite, got %g", (double)a->gain);
  DFL_REQUIRE(a->electronic_sigma >= 0.f && a->electronic_sigma < INFINITY,
              "dfl_drr_expose: electronic_sigma must not be negative, got %g", (double)a->electronic_sigma);
  DFL_REQUIRE(!a->quantum || a->key_q != nullptr, "dfl_drr_expose: quantum noise needs the key array key_q");
  DFL_REQUIRE(!a->electronic || a->key_e != nullptr, "dfl_drr_expose: electronic noise needs the key array key_e");
  const dim3 grid((unsigned)dfl::ceil_div(a->C, dfl::EX_TW), (unsigned)dfl::ceil_div(a->R, dfl::EX_TH), (unsigned)a->V);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (a->u16)
    dfl::expose_kernel<true><<<grid, dfl::EX_THREADS, 0, s>>>(*a);
  else
    dfl::expose_kernel<false><<<grid, dfl::EX_THREADS, 0, s>>>(*a);
  return dfl::check_launch("dfl_drr_expose");
}
