// Host-side planning of dfl_conv2d: which kernel family takes an argument block and, for bf16 tensors, its geometry (tile
// configuration, patch shape, resident channels, K slices) and the LDS of its launch.  No kernels here: the kernel files
// (convp_bf16.hip, convq_bf16.hip, convn_bf16.hip, convs.hip, conv_gemm.hip, ...) launch what this file decides.
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "conv_plan.h"
#include "conv_rows.h"
#include "direct_small.h"

namespace dfl {

bool convs_enabled() {
  static const bool on = [] {
    const char* e = getenv("DFL_CONVS");               // 0: the latency forms are never taken (A/B against the other kernels)
    return e == nullptr || atoi(e) != 0;
  }();
  return on;
}

// ---- the tile configurations of the bf16 convolution
enum class Family { Patch, Latency, Unrolled, Narrow };
struct Tile {
  Family family;
  int layout;         // index into the family's own list: convp_tiles(), convq_layouts(), convn_layouts()
  int pers;           // the persistent form of the layout
  bool measured;      // chosen only through the measured table (tools/tune_convp.py) or a forced geometry, never by the cost model
  ConvLaunch launch;
};

// Numbered as dfl_conv_config (16 + index), the tuning file and dfl_conv_force_geometry know them:
//   0 ... 38   patch-resident (convp_bf16.hip); 22 ... 29 (streamed 1x1 / 2x2 windows) and 30 ... 38 (two k-groups) measured only
//   39         the latency form (convs.hip): plans itself, never through the search
//   40 ... 48  the unrolled 3x3 form (convq_bf16.hip), its nine layouts; 49 ... 57 the same, persistent
//   58 ... 63  the narrow 3x3 form (convn_bf16.hip), its six layouts; 64, 65 the persistent form of its layouts of three rows per wave
static const std::vector<Tile>& tiles() {
  static const std::vector<Tile> t = [] {
    const PatchTile* pt = convp_tiles();
    const QLayout* q = convq_layouts();
    const NLayout* n = convn_layouts();
    std::vector<Tile> v;
    for (int i = 0; i < kNumPatchTiles; ++i) v.push_back({Family::Patch, i, 0, pt[i].GA != 0 || pt[i].KS == 2, pt[i].launch});
    v.push_back({Family::Latency, 0, 0, false, convs_launch});
    for (int pers = 0; pers < 2; ++pers)
      for (int i = 0; i < kNumQ; ++i) v.push_back({Family::Unrolled, i, pers, true, q[i].launch});
    for (int i = 0; i < kNumN; ++i) v.push_back({Family::Narrow, i, 0, true, n[i].launch});
    for (int i = 0; i < kNumN; ++i)
      if (n[i].R <= 3) v.push_back({Family::Narrow, i, 1, true, n[i].launch});
    return v;
  }();
  return t;
}

constexpr size_t kLdsSoft = 64 * 1024, kLdsHard = 150 * 1024;   // patch images: what the search prefers, what it admits

static uint32_t magic(int d) { return (uint32_t)(((1ull << 32) + (uint64_t)d - 1) / (uint64_t)d); }   // ceil(2^32 / d)

// The patch of (ipp images, ph x pw pixels) on the layer's gather grid
static void place_patch(const dfl_conv_args& a, ConvP* p, int ipp, int ph, int pw) {
  p->IPP = ipp;
  p->PH = ph;
  p->PW = pw;
  p->mPP = magic(ph * pw);
  p->mPW = magic(pw);
  p->npy = (int)ceil_div(p->Hg, ph);
  p->npx = (int)ceil_div(p->Wg, pw);
  p->npatch = (int)ceil_div(a.N, ipp) * p->npy * p->npx;
  p->IH = (ph - 1) * a.stride + a.KH;
  p->IW = (pw - 1) * a.stride + a.KW;
}

// ck resident channels of an LDS image: the layout of its pixels
static void set_channels(ConvP* p, int ck, int nblk, int splits) {
  p->CK = ck;
  p->nblk = nblk;
  p->splits = splits;
  p->blk_per_slice = nblk / splits;
  p->pix_stride = ck * 2 + 16;
  int sh = 0;
  while ((1 << sh) < (ck >> 3)) ++sh;
  p->upp_shift = sh;
}

// Resident channels of an image of npix pixels: K slices only over whole channel blocks; more blocks (smaller ck) when the
// layer wants the slices.  false: no block of at least ck_min channels divides the layer for these slices.
static bool slice_channels(const dfl_conv_args& a, int want_splits, int ck_min, int* ck, int* nblk, int* splits) {
  *nblk = a.Cin / *ck;
  *splits = 1;
  if (want_splits <= 1) return true;
  *splits = want_splits;
  while (*nblk % *splits != 0 && *ck > ck_min) {
    *ck >>= 1;
    *nblk = a.Cin / *ck;
  }
  return *nblk % *splits == 0;
}

// Workgroup -> XCD placement (see convp_kernel): weight-major when one pass over the weights is the larger stream
static void place_on_xcds(const dfl_conv_args& a, ConvP* p) {
  const int64_t wbytes = (int64_t)a.KH * a.KW * a.Cin * a.Ntot * 2;
  const int64_t abytes = (int64_t)a.N * a.Hin * a.Win * a.Cin * 2;
  const int pairs = p->ntiles * p->splits;
  p->xcd_mode = 0;
  p->grid = p->npatch * pairs;
  if (wbytes > abytes && wbytes > (1 << 20)) {
    if (pairs >= 8 && pairs % 8 == 0) {
      p->xcd_mode = 1;
    } else if (pairs < 8 && 8 % pairs == 0 && p->npatch >= 8 / pairs) {
      p->xcd_mode = 2;
      p->grid = 8 * (int)ceil_div(p->npatch, 8 / pairs);
    }
  }
}

// Cost model (cycles), fitted to per-layer timings on MI355X (tools/kbench_bf16.py).  A workgroup's k loop is bound by
// the matrix pipe (32 cycles per instruction and wave, one wave per SIMD), by its LDS fragment reads, or by the B
// fragments coming from L1/L2 (each wave 1 KiB per k-step and column tile: ~32 B/clk/CU when the four waves read
// different columns, more when they share them); around it sit latencies nobody inside the workgroup hides: staging
// the patch (one global round trip + the LDS writes) and one pass per accumulator tile row in the epilogue.  `occ`
// workgroups share a CU (LDS, registers: 512 / allocation of the tile configuration): while one waits another computes.
static double patch_cost(const dfl_conv_args& a, const ConvP& p, const PatchTile& t) {
  static const int occ_by_tm[10] = {0, 5, 4, 4, 3, 2, 2, 2, 2, 2};
  const size_t lds = (size_t)p.lds_bytes;
  int occ = (int)((160 * 1024) / (lds + 1024));
  if (occ > occ_by_tm[t.TM]) occ = occ_by_tm[t.TM];
  if (occ < 1) occ = 1;
  const int64_t total = (int64_t)p.npatch * p.ntiles * p.splits;
  int64_t eff = ceil_div(total, 256);
  if (eff > occ) eff = occ;                                                      // workgroups actually sharing a CU
  const int64_t rounds = ceil_div(total, 256 * eff);
  const int steps = (a.KH * a.KW * (p.CK / 16) + 3) / 4 * 4 * p.blk_per_slice;
  const double mfma = (double)t.TM * t.TN * steps * 32.0;
  const double ldsread = (double)t.TM * steps * 4.0 * 4.0;                       // ds_read_b128 cycles of the 4 waves
  const double bbw = t.WN == 4 ? 32.0 : (t.WN == 2 ? 48.0 : 64.0);
  const double bload = (double)steps * t.TN * 4096.0 / bbw;
  double loop = mfma > ldsread ? mfma : ldsread;
  if (bload > loop) loop = bload;
  const double lat = (double)p.blk_per_slice * (4000.0 + (double)lds / 40.0) + 2000.0 + (p.splits > 1 ? 1500.0 : 2500.0 * t.TM);
  const double busy = (double)eff * (loop + (double)p.blk_per_slice * (double)lds / 40.0);   // what the CU's pipes must do per round
  const double per_round = busy > lat + loop ? busy : lat + loop;
  double c = (double)rounds * per_round;
  if (p.splits > 1) c += (double)p.Mtot * a.Ntot * 4.0 * (p.splits + 1) / 2000.0 + 6000.0;   // partial sums: bytes / (B per cycle of the chip) + the finish launch
  return c;
}

// ---- one geometry function per family: fill pl for a patch of (ipp images, ph x pw pixels) and want_splits K slices;
// false if the configuration cannot take it

static bool patch_geometry(const dfl_conv_args& a, ConvPlan* pl, const PatchTile& t, bool measured, int ipp, int ph, int pw, int want_splits) {
  ConvP* p = &pl->p;
  if (ipp < 1 || ph < 1 || pw < 1 || (int64_t)ipp * ph * pw > t.WM * t.TM * 32) return false;
  if (ipp > 1 && (ph != p->Hg || pw != p->Wg)) return false;
  place_patch(a, p, ipp, ph, pw);
  const int bn = t.WN * t.TN * 32;
  if (t.GA) {
    // streamed non-overlapping window (1x1 / stride 1, 2x2 / stride 2): no LDS image, no K slices
    if (a.KH != a.KW || a.stride != a.KH || a.KH > 2 || a.pad != 0 || a.in_scale != nullptr || a.in_tot != nullptr || a.x_mode != 0 || want_splits > 1) return false;
    set_channels(p, 16, a.Cin / 16, 1);
    p->lds_bytes = 0;
    p->ntiles = (int)ceil_div(a.Ntot, bn);
    p->xcd_mode = 0;
    p->grid = p->npatch * p->ntiles;
  } else {
    // resident channels: the largest power-of-two multiple of 16 (<= 128, dividing Cin) whose image fits
    const int64_t npix = (int64_t)ipp * p->IH * p->IW;
    int ck = 128;
    while (ck > 16 && (a.Cin % ck != 0 || npix * (ck * 2 + 16) > (int64_t)kLdsSoft)) ck >>= 1;
    if (a.Cin % ck != 0) return false;
    if ((size_t)npix * (ck * 2 + 16) > kLdsHard) return false;
    int nblk, splits;
    if (!slice_channels(a, want_splits, 16, &ck, &nblk, &splits)) return false;
    set_channels(p, ck, nblk, splits);
    p->ntiles = (int)ceil_div(a.Ntot, bn);
    place_on_xcds(a, p);
    p->lds_bytes = (int)(npix * (ck * 2 + 16));
  }
  // the launch: the image, or the epilogue's pass image and statistics scratch where larger, then the live-BatchNorm tables
  const int nt = 256 * t.KS, rps = nt / (bn / 8) < t.WM * 32 ? nt / (bn / 8) : t.WM * 32;
  size_t lds = (size_t)p->lds_bytes;
  const size_t epi = (size_t)t.WM * 32 * (bn + 4) * sizeof(float), red = (size_t)rps * 2 * bn * sizeof(float);
  if (lds < epi) lds = epi;
  if (lds < red) lds = red;
  p->tab_off = (int)((lds + 15) / 16 * 16);
  pl->lds = (size_t)p->tab_off + (384 + 3 * bn) * sizeof(float);
  if (pl->lds > (size_t)kLdsOptIn) return false;
  pl->cost = measured ? 0.0 : patch_cost(a, *p, t);
  return true;
}

static bool unrolled_geometry(const dfl_conv_args& a, ConvPlan* pl, int layout, int pers, int ipp, int ph, int pw, int want_splits) {
  ConvP* p = &pl->p;
  const QLayout& t = convq_layouts()[layout];
  if (ipp != 1 || ph != 8 * t.WM || pw != 12 || !convq_shape_ok(a)) return false;
  place_patch(a, p, ipp, ph, pw);
  const int64_t npix = (int64_t)p->IH * p->IW;
  // the largest resident block the layout is instantiated for and whose image fits
  int ck = 128;
  while (ck >= 32 && (a.Cin % ck != 0 || !convq_ck_ok(layout, ck) || convq_lds_bytes(ck, layout, a.Cin / ck > 1 ? 2 : 1, pers, nullptr) > (size_t)kLdsOptIn)) ck >>= 1;
  if (ck < 32) return false;
  if ((size_t)npix * (ck * 2 + 16) > kLdsHard) return false;
  int nblk, splits;
  if (!slice_channels(a, want_splits, 32, &ck, &nblk, &splits) || !convq_ck_ok(layout, ck)) return false;
  set_channels(p, ck, nblk, splits);
  p->ntiles = (int)ceil_div(a.Ntot, 32 * t.WN);
  place_on_xcds(a, p);
  if (p->grid >= 65536 || p->npatch >= 65536) return false;      // (the kernel divides workgroup numbers by multiply-high)
  int tab_off;
  const size_t lds = convq_lds_bytes(ck, layout, p->blk_per_slice, pers, &tab_off);
  if (lds > (size_t)kLdsOptIn) return false;
  if (pers) {
    if (!convq_pers_ok(layout, ck, a.x_mode)) return false;
    // persistent: as many workgroups per (column tile, K slice) as the CUs hold at once, patches dealt out evenly; pointless
    // (and refused) when that leaves one patch per workgroup
    int occ = 64 * t.WM * t.WN * t.KS == 512 ? 1 : 2;
    if ((size_t)occ * lds > 160 * 1024) occ = 1;
    int g0 = 256 * occ / (p->ntiles * splits);
    if (g0 < 1) g0 = 1;
    if (g0 >= p->npatch) return false;
    const int per = (int)ceil_div(p->npatch, g0);
    p->q_ngroups = (int)ceil_div(p->npatch, per);
    p->xcd_mode = 0;
    p->grid = p->q_ngroups * p->ntiles * splits;
  }
  p->qm_npatch = magic(pers ? p->q_ngroups : p->npatch);
  p->qm_ntiles = magic(p->ntiles);
  p->qm_perimg = magic(p->npy * p->npx);
  p->qm_npx = magic(p->npx);
  p->lds_bytes = (int)(npix * (ck * 2 + 16));
  p->tab_off = tab_off;
  pl->lds = lds;
  pl->cost = 0.0;
  return true;
}

static void narrow_patch(int layout, int* ph, int* pw) {
  const NLayout& n = convn_layouts()[layout];
  *ph = n.R * (4 / n.WX);
  *pw = 32 * n.WX;
}

// The layout fixes the patch, all input channels pass through one image in blocks of 32, no K slices, one column tile;
// workgroups are dealt to the XCDs in runs of q_ngroups patches
static bool narrow_geometry(const dfl_conv_args& a, ConvPlan* pl, int layout, int pers, int ipp, int ph, int pw, int want_splits) {
  ConvP* p = &pl->p;
  int nph, npw;
  narrow_patch(layout, &nph, &npw);
  if (ipp != 1 || ph != nph || pw != npw || want_splits > 1 || !convn_shape_ok(a) || !convn_layout_ok(layout, a.Ntot, a.Cin)) return false;
  if ((int64_t)p->Mtot * a.ldy * 2 >= (1ll << 32)) return false;     // (y is addressed with 32-bit byte offsets)
  place_patch(a, p, 1, ph, pw);
  if (p->npatch >= 65536) return false;              // (the kernel divides patch numbers by multiply-high)
  set_channels(p, 32, a.Cin / 32, 1);
  p->ntiles = 1;
  p->lds_bytes = p->IH * p->IW * 80;
  p->xcd_mode = 0;
  p->q_ngroups = (int)ceil_div(p->npatch, 8);
  p->q_stride = p->q_ngroups;
  p->grid = 8 * p->q_ngroups;
  if (pers) {                                        // persistent: two workgroups per CU (64 per XCD), each walks several patches of its XCD's run
    if (!convn_pers_ok(layout, a) || p->q_ngroups <= 64) return false;
    p->q_stride = 64;
    p->grid = 8 * 64;
  }
  p->qm_npatch = magic(p->npatch);
  p->qm_ntiles = magic(1);
  p->qm_perimg = magic(p->npy * p->npx);
  p->qm_npx = magic(p->npx);
  int tab_off;
  pl->lds = convn_lds_bytes(layout, a.Cin, a.Ntot, pers, &tab_off);
  if (pl->lds > (size_t)kLdsOptIn) return false;
  p->tab_off = tab_off;
  pl->cost = 0.0;
  return true;
}

static bool try_geometry(const dfl_conv_args& a, ConvPlan* pl, const Tile& t, int ipp, int ph, int pw, int want_splits) {
  bool ok = false;
  switch (t.family) {
    case Family::Patch: ok = patch_geometry(a, pl, convp_tiles()[t.layout], t.measured, ipp, ph, pw, want_splits); break;
    case Family::Unrolled: ok = unrolled_geometry(a, pl, t.layout, t.pers, ipp, ph, pw, want_splits); break;
    case Family::Narrow: ok = narrow_geometry(a, pl, t.layout, t.pers, ipp, ph, pw, want_splits); break;
    case Family::Latency: break;
  }
  if (!ok) return false;
  pl->launch = t.launch;
  pl->pers = t.pers;
  return true;
}

// ---- geometry candidates, forced geometry, tuning table
struct ConvGeom { int tile, ipp, ph, pw, splits; };
static thread_local ConvGeom t_force = {-1, 0, 0, 0, 0};
struct TuneEntry { int key[10]; ConvGeom g; };
static std::mutex g_tune_mu;
static std::vector<TuneEntry> g_tune;

static void tune_key(const dfl_conv_args& a, int* k) {
  k[0] = a.N; k[1] = a.Hin; k[2] = a.Win; k[3] = a.Cin; k[4] = a.Ntot;
  k[5] = a.KH; k[6] = a.KW; k[7] = a.stride; k[8] = a.pad; k[9] = a.scatter2x2 ? 1 : 0;
}

static bool tune_lookup(const dfl_conv_args& a, ConvGeom* g) {
  int k[10];
  tune_key(a, k);
  std::lock_guard<std::mutex> lock(g_tune_mu);
  for (const TuneEntry& e : g_tune)
    if (memcmp(e.key, k, sizeof(k)) == 0) {
      *g = e.g;
      return true;
    }
  return false;
}

// Column tiles a configuration may take: `wide` (tuners) the narrower ones too (more workgroups); else those the cost model
// was fitted on (one column tile per wave, as wide as the layer)
static bool columns_ok(const dfl_conv_args& a, int wn, int tn, bool wide) {
  const int n32 = (int)ceil_div(a.Ntot, 32) * 32, bn = wn * tn * 32;
  if (wide) return !(bn > n32 || (bn < 64 && n32 >= 64) || (tn > 1 && bn > a.Ntot));
  if (tn != 1) return false;
  return a.Ntot <= 32 ? wn == 1 : (a.Ntot <= 64 ? wn == 2 : wn == 4);
}

// Patch shapes of a configuration, as (images, rows, pixels per row)
static int patch_shapes(const ConvP& base, const PatchTile& t, bool wide, int (*shapes)[3]) {
  const int QP = t.WM * t.TM * 32;
  const int HW = base.Hg * base.Wg;
  int ns = 0;
  if (HW <= QP) {                                  // whole images
    shapes[ns][0] = QP / HW; shapes[ns][1] = base.Hg; shapes[ns][2] = base.Wg; ++ns;
  }
  if (base.Wg <= QP) {                             // whole rows
    int ph = QP / base.Wg;
    if (ph > base.Hg) ph = base.Hg;
    shapes[ns][0] = 1; shapes[ns][1] = ph; shapes[ns][2] = base.Wg; ++ns;
  }
  static const int kPh[] = {1, 2, 4, 8, 16, 3, 6, 12};        // row pieces (the model looks at the powers of two)
  for (int k = 0; k < (wide ? 8 : 5) && ns < 22; ++k) {
    const int ph = kPh[k];
    int pw = QP / ph;
    if (pw >= base.Wg || ph > base.Hg) continue;
    shapes[ns][0] = 1; shapes[ns][1] = ph; shapes[ns][2] = pw; ++ns;
  }
  return ns;
}

// Tile configurations x patch shapes x K slices that are valid for the layer, in that order.  The cost model looks at the
// configurations it was fitted on (`wide` false); tuners get every configuration (`wide` true).
template <typename F>
static void for_each_candidate(const dfl_conv_args& a, const ConvP& base, int force_splits, bool wide, F&& f) {
  const std::vector<Tile>& T = tiles();
  for (int ti = 0; ti < (int)T.size(); ++ti) {
    const Tile& t = T[ti];
    if (t.measured && !wide) continue;
    int shapes[24][3];
    int ns = 0;
    if (t.family == Family::Patch) {
      const PatchTile& pt = convp_tiles()[t.layout];
      if (columns_ok(a, pt.WN, pt.TN, wide)) ns = patch_shapes(base, pt, wide, shapes);
    } else if (t.family == Family::Unrolled) {       // one patch shape
      const QLayout& q = convq_layouts()[t.layout];
      if (columns_ok(a, q.WN, 1, wide)) {
        shapes[0][0] = 1; shapes[0][1] = 8 * q.WM; shapes[0][2] = 12; ns = 1;
      }
    } else if (t.family == Family::Narrow) {         // the layout's patch; takes all the layer's columns itself
      if (convn_shape_ok(a)) {
        shapes[0][0] = 1; narrow_patch(t.layout, &shapes[0][1], &shapes[0][2]); ns = 1;
      }
    }
    for (int si = 0; si < ns; ++si) {
      for (int sp = 1; sp <= 32; sp *= 2) {
        if (force_splits > 0 && sp != force_splits) continue;
        if (!wide && a.scatter2x2 == 0 && a.accumulate == 0 && sp > 1 && base.T * a.Cin < 1024) break;   // short K: never sliced
        ConvPlan q;
        q.p = base;
        if (!try_geometry(a, &q, t, shapes[si][0], shapes[si][1], shapes[si][2], sp)) continue;
        if (q.p.splits != sp) continue;
        f(ti, q);
      }
    }
  }
}

// Validates the argument block and fills the layer's constants (gather grid, extents)
static int convp_validate(const dfl_conv_args* a, ConvP* p) {
  DFL_REQUIRE(a->x && a->w && a->y, "dfl_conv2d (bf16): x, w and y are required");
  DFL_REQUIRE(a->N > 0 && a->Hin > 0 && a->Win > 0 && a->Cin > 0 && a->Ntot > 0, "dfl_conv2d (bf16): bad sizes");
  DFL_REQUIRE(a->Ntot % 8 == 0 && a->ldy % 8 == 0 && aligned16(a->y) && (a->add == nullptr || (a->ldadd % 8 == 0 && aligned16(a->add))) &&
                  (a->stat_other == nullptr || (a->ldso % 8 == 0 && aligned16(a->stat_other))),
              "dfl_conv2d (bf16): output columns and the pixel strides of y / add / stat_other must be multiples of 8, tensors 16-byte aligned");
  {
    const int64_t opx = (int64_t)a->N * a->Hout * a->Wout, lim = 1ll << 32;
    DFL_REQUIRE(opx * a->ldy < lim && (a->add == nullptr || opx * a->ldadd < lim) && (a->stat_other == nullptr || opx * a->ldso < lim),
                "dfl_conv2d (bf16): y / add / stat_other must stay below 2^32 elements");
  }
  DFL_REQUIRE(a->Cin % 16 == 0 && a->ldx % 8 == 0 && aligned16(a->x) && aligned16(a->w),
              "dfl_conv2d (bf16): needs Cin %% 16 == 0, ldx %% 8 == 0 and 16-byte aligned x / w (Cin = %d, ldx = %d)", a->Cin, a->ldx);
  DFL_REQUIRE(a->w_split == 2, "dfl_conv2d (bf16): weights must be packed with dfl_pack_job.split = 2");
  DFL_REQUIRE(a->x_mode != 0 || (a->in_scale == nullptr) == (a->in_shift == nullptr), "dfl_conv2d: in_scale/in_shift go together");
  DFL_REQUIRE(a->in_tot == nullptr || (a->in_scale == nullptr && a->in_gamma != nullptr && a->in_count > 0 &&
                                       (a->x_mode == 0 ? a->in_beta != nullptr : (a->in_mean != nullptr && a->in_invstd != nullptr))),
              "dfl_conv2d (bf16): in_tot replaces in_scale / in_shift and needs in_gamma, in_count and in_beta (x_mode 0) or in_mean, in_invstd (x_mode 1)");
  DFL_REQUIRE(a->add_tot == nullptr || (a->add != nullptr && a->add_scale == nullptr && a->add_gamma != nullptr && a->add_beta != nullptr && a->add_count > 0),
              "dfl_conv2d (bf16): add_tot replaces add_scale / add_shift and needs add, add_gamma, add_beta, add_count");

  DFL_REQUIRE((a->add_scale == nullptr) == (a->add_shift == nullptr), "dfl_conv2d: add_scale/add_shift go together");
  DFL_REQUIRE(a->KH * a->KW <= 16 && a->KH > 0 && a->KW > 0 && a->stride > 0 && a->pad >= 0, "dfl_conv2d (bf16): bad window");
  memset(p, 0, sizeof(*p));
  p->a = *a;
  if (a->scatter2x2) {
    DFL_REQUIRE(a->KH == 1 && a->KW == 1 && a->stride == 1 && a->pad == 0, "dfl_conv2d: scatter2x2 needs a 1x1 gather");
    DFL_REQUIRE(a->Ntot % 4 == 0 && a->Hout >= 2 * a->Hin && a->Wout >= 2 * a->Win, "dfl_conv2d: scatter2x2 geometry");
    DFL_REQUIRE(a->add == nullptr, "dfl_conv2d: scatter2x2 has no add epilogue");
    p->Hg = a->Hin;
    p->Wg = a->Win;
    p->Cout = a->Ntot / 4;
  } else {
    const int ho = (a->Hin + 2 * a->pad - a->KH) / a->stride + 1;
    const int wo = (a->Win + 2 * a->pad - a->KW) / a->stride + 1;
    DFL_REQUIRE(ho == a->Hout && wo == a->Wout, "dfl_conv2d: Hout/Wout (%d,%d) do not match the window (%d,%d)", a->Hout,
                a->Wout, ho, wo);
    p->Hg = a->Hout;
    p->Wg = a->Wout;
    p->Cout = a->Ntot;
  }
  DFL_REQUIRE(a->ldy >= p->Cout, "dfl_conv2d: ldy < Cout");
  const int64_t M = (int64_t)a->N * p->Hg * p->Wg;
  DFL_REQUIRE(M < (1ll << 31), "dfl_conv2d: too many pixels");
  p->Mtot = (int)M;
  p->T = a->KH * a->KW;
  const int64_t xb = (((int64_t)a->N * a->Hin * a->Win - 1) * a->ldx + a->Cin) * 2;
  const int64_t wb = (int64_t)p->T * a->Cin * a->Ntot * 2;
  const int64_t lim = (1ll << 31) - 4096;
  DFL_REQUIRE(xb < lim && wb < lim, "dfl_conv2d (bf16): tensors must stay below 2 GiB");
  p->x_bytes = (uint32_t)xb;
  p->w_bytes = (uint32_t)wb;
  if (a->x_mode != 0) {
    DFL_REQUIRE(a->x_mode == 1 && a->x2 != nullptr && a->in_shift == nullptr && a->ldx2 % 8 == 0 && aligned16(a->x2) &&
                    (a->in_scale == nullptr || aligned16(a->in_scale)),
                "dfl_conv2d (bf16): x_mode 1 needs x2 (16-byte aligned, ldx2 %% 8 == 0), coefficients in in_scale and no in_shift");
    const int64_t x2b = (((int64_t)a->N * a->Hin * a->Win - 1) * a->ldx2 + a->Cin) * 2;
    DFL_REQUIRE(x2b < lim, "dfl_conv2d (bf16): tensors must stay below 2 GiB");
    p->x2_bytes = (uint32_t)x2b;
  }
  p->xo_bytes = 0;
  if (a->x_out != nullptr) {
    DFL_REQUIRE(a->x_mode == 1 && a->KH == 3 && a->KW == 3 && a->stride == 1 && a->pad == 1 && a->Hout == a->Hin && a->Wout == a->Win,
                "dfl_conv2d (bf16): x_out goes with x_mode 1 of a 3x3 stride-1 pad-1 layer");
    DFL_REQUIRE(a->ldxo % 8 == 0 && a->ldxo >= a->Cin && aligned16(a->x_out) && a->x_out != a->x && a->x_out != a->x2,
                "dfl_conv2d (bf16): x_out must be 16-byte aligned with ldxo %% 8 == 0, ldxo >= Cin, and a tensor of its own");
    const int64_t xob = (((int64_t)a->N * a->Hin * a->Win - 1) * a->ldxo + a->Cin) * 2;
    DFL_REQUIRE(xob < lim, "dfl_conv2d (bf16): tensors must stay below 2 GiB");
    p->xo_bytes = (uint32_t)xob;
  }
  return DFL_OK;
}

static int convp_plan_search(const dfl_conv_args* a, ConvPlan* pl, int force_splits) {
  memset(pl, 0, sizeof(*pl));
  const int rc = convp_validate(a, &pl->p);
  if (rc != DFL_OK) return rc;

  // the latency form (dfl_conv_args.latency_form: small problems of a batch-1 inference forward, convs.hip) plans itself
  if (t_force.tile < 0 && convs_eligible(*a, pl->p)) {
    convs_plan(*a, &pl->p, force_splits);
    pl->lds = (size_t)pl->p.lds_bytes;
    pl->launch = tiles()[CONVS_TILE].launch;
    return DFL_OK;
  }

  DFL_REQUIRE(a->out_scale == nullptr, "dfl_conv2d (bf16): out_scale / out_shift are implemented by the latency form only (dfl_conv_config tells)");
  // a forced geometry (dfl_conv_force_geometry: tuners, tests) or an entry of the tuning table (dfl_conv_tune_add) wins
  // over the cost model, as long as it is valid for this layer and agrees with the caller's K slices
  const ConvP base = pl->p;
  int best_tile = -1;
  {
    ConvGeom g;
    const bool forced = t_force.tile >= 0;
    if (forced) g = t_force;
    if (forced || tune_lookup(*a, &g)) {
      if (g.tile >= 0 && g.tile < (int)tiles().size() && (force_splits <= 0 || force_splits == g.splits)) {
        ConvPlan q = *pl;
        if (try_geometry(*a, &q, tiles()[g.tile], g.ipp, g.ph, g.pw, g.splits) && q.p.splits == g.splits) {
          *pl = q;
          best_tile = g.tile;
        }
      }
      DFL_REQUIRE(!forced || best_tile >= 0, "dfl_conv2d (bf16): the forced geometry (tile %d, patch %dx%dx%d, %d slices) does not fit this layer",
                  g.tile, g.ipp, g.ph, g.pw, g.splits);
    }
  }
  if (best_tile < 0) {
    double best = 1e300;
    for_each_candidate(*a, base, force_splits, false, [&](int ti, const ConvPlan& q) {
      if (q.cost < best) {
        best = q.cost;
        *pl = q;
        best_tile = ti;
      }
    });
  }
  DFL_REQUIRE(best_tile >= 0, "dfl_conv2d (bf16): no patch geometry fits this layer (%dx%d, Cin %d, Ntot %d)", a->Hin, a->Win,
              a->Cin, a->Ntot);
  pl->p.tile = best_tile;
  static const bool dbg = getenv("DFL_CONVP_DEBUG") != nullptr;
  if (dbg && force_splits == 0)
    fprintf(stderr, "convp %dx%d Cin%d->%d k%d s%d: tile %d patch %dx%dx%d CK %d blocks %d splits %d lds %zu cost %.0f%s\n", a->Hin, a->Win,
            a->Cin, a->Ntot, a->KH, a->stride, best_tile, pl->p.IPP, pl->p.PH, pl->p.PW, pl->p.CK, pl->p.nblk, pl->p.splits, pl->lds,
            pl->cost, tiles()[best_tile].measured ? " (measured)" : "");
  return DFL_OK;
}

// The geometry of an argument block is resolved ONCE: a recorded program replays the same blocks every step (97 convolutions
// per training step of the paper network), and the search above -- validation, the tuning-table scan under a mutex, for
// layers the table does not list up to ~1000 try_geometry calls -- is host time the GPU waits for on a slow host
// (8.4 ms per step observed where the kernels take 5.3).  Keyed by the whole argument block (addresses
// included: they select alignment-dependent paths and are copied into ConvP) and the requested K slices; a forced
// geometry (tuners, tests) bypasses it, a changed tuning table clears it.
struct PlanMemo { dfl_conv_args a; int force_splits; ConvPlan pl; };
static std::mutex g_memo_mu;
static std::vector<PlanMemo> g_memo[64];
static inline unsigned memo_bucket(const dfl_conv_args* a, int force_splits) {
  uint64_t h = 1469598103934665603ull;
  const uint64_t* w = reinterpret_cast<const uint64_t*>(a);
  for (size_t i = 0; i < sizeof(dfl_conv_args) / 8; ++i) h = (h ^ w[i]) * 1099511628211ull;
  h ^= (uint64_t)force_splits;
  return (unsigned)((h ^ (h >> 29)) & 63u);
}
static void memo_clear() {
  std::lock_guard<std::mutex> lock(g_memo_mu);
  for (auto& b : g_memo) b.clear();
}

int convp_plan(const dfl_conv_args* a, ConvPlan* pl, int force_splits) {
  static_assert(sizeof(dfl_conv_args) % 8 == 0, "hashed as 64-bit words");
  DFL_REQUIRE(a != nullptr && pl != nullptr, "dfl_conv2d (bf16): null arguments");
  if (t_force.tile >= 0) return convp_plan_search(a, pl, force_splits);
  const unsigned b = memo_bucket(a, force_splits);
  {
    std::lock_guard<std::mutex> lock(g_memo_mu);
    for (const PlanMemo& m : g_memo[b])
      if (m.force_splits == force_splits && memcmp(&m.a, a, sizeof(*a)) == 0) {
        *pl = m.pl;
        return DFL_OK;
      }
  }
  const int rc = convp_plan_search(a, pl, force_splits);
  if (rc != DFL_OK) return rc;
  std::lock_guard<std::mutex> lock(g_memo_mu);
  if (g_memo[b].size() >= 256) g_memo[b].clear();          // bounded: 16 K argument blocks, then start over
  g_memo[b].push_back(PlanMemo{*a, force_splits, *pl});
  return DFL_OK;
}

// Candidates of the geometry search for one layer (tuners: tools/tune_convp.py): up to `max` rows of 5 integers
// (tile configuration, images per patch, patch height, patch width, K slices); returns the number of candidates.
static int convp_candidates(const dfl_conv_args* a, int32_t* out, int max) {
  ConvPlan pl;
  const int saved_tile = t_force.tile;
  t_force.tile = -1;
  const int rc = convp_plan(a, &pl, 0);               // validates the arguments and fills the layer constants
  t_force.tile = saved_tile;
  if (rc != DFL_OK) return -1;
  int n = 0;
  for_each_candidate(*a, pl.p, 0, true, [&](int ti, const ConvPlan& q) {
    if (n < max) {
      int32_t* o = out + 5 * n;
      o[0] = ti; o[1] = q.p.IPP; o[2] = q.p.PH; o[3] = q.p.PW; o[4] = q.p.splits;
    }
    ++n;
  });
  return n;
}

// The latency plan of an fp32 block: the layer constants conv_prepare has validated, then the form's own conditions and work split
static bool latency32_plan(const ConvK& k, int force_splits, ConvPlan* pl) {
  if (!k.a.latency_form || !convs_enabled()) return false;      // (training blocks: nothing is copied)
  memset(pl, 0, sizeof(*pl));
  ConvP* p = &pl->p;
  p->a = k.a;
  p->Mtot = k.Mtot;
  p->Hg = k.Hg;
  p->Wg = k.Wg;
  p->Cout = k.Cout;
  p->T = k.a.KH * k.a.KW;
  p->x_bytes = k.x_bytes;
  p->w_bytes = k.w_bytes;
  if (!convs_eligible(k.a, *p)) return false;
  convs_plan(k.a, p, force_splits);
  pl->lds = (size_t)p->lds_bytes;
  pl->launch = convs_launch;
  return true;
}

// ---- the route of dfl_conv2d and its queries
int conv_route(const dfl_conv_args* a, int want_splits, ConvRoute* r) {
  if (a != nullptr && a->x_bf16) {                    // bf16 tensors: the plan's tile configuration names the family
    const int rc = convp_plan(a, &r->plan, want_splits);
    if (rc != DFL_OK) return rc;
    r->form = FORM_BF16;
    r->cfg = 16 + r->plan.p.tile;
    r->splits = r->plan.p.splits;
    return DFL_OK;
  }
  const int rc = conv_prepare(a, &r->k);
  if (rc != DFL_OK) return rc;
  const ConvK& k = r->k;
  // the throughput forms: what runs unless a latency form takes the block, and what sizes stat_partials (the latency forms
  // take no statistics: a block that asks for them is never theirs)
  int sug;                                            // the K slices the form suggests
  if (direct_conv_ok(a)) {
    r->stat_form = FORM_DIRECT;
    r->stat_cfg = CFG_DIRECT;
    sug = 1;
  } else {
    const int t = conv_rows_tile(k);
    r->stat_form = t ? FORM_ROWS : FORM_GEMM;
    r->stat_cfg = t ? t : conv_gemm_cfg(k);
    const int rs = conv_rows_splits(k);
    sug = rs ? rs : conv_gemm_splits(k);
  }
  r->form = r->stat_form;
  r->cfg = r->stat_cfg;
  r->splits = want_splits > 0 ? want_splits : sug;
  if (convs_first_ok(a)) {                            // the 1-channel 3x3 first layer (convs.hip)
    r->form = FORM_FIRST;
    r->cfg = 16 + CONVS_TILE;
    r->splits = 1;
  } else if (latency32_plan(k, want_splits, &r->plan)) {          // the latency form of fp32 tensors (convs.hip)
    r->form = FORM_LATENCY32;
    r->cfg = 16 + CONVS_TILE;
    r->splits = r->plan.p.splits;
  }
  return DFL_OK;
}

static int want_splits(const dfl_conv_args* a) { return a != nullptr && a->splits > 1 ? a->splits : 1; }

int conv_pair_route(const dfl_conv_args* a, const dfl_conv_args* b, ConvRoute* r) {
  if (a == nullptr || b == nullptr || !a->latency_form || conv_route(a, want_splits(a), r) != DFL_OK) return 0;
  return r->form == FORM_BF16 || r->form == FORM_LATENCY32 ? convs_pair_ok(a, b, r->plan.p) : 0;
}

}  // namespace dfl

// ---- C ABI (include/dfl_hip.h)
extern "C" int dfl_conv_config(const dfl_conv_args* a) {
  dfl::ConvRoute r;
  const int rc = dfl::conv_route(a, dfl::want_splits(a), &r);
  return rc != DFL_OK ? rc : r.cfg;
}

extern "C" int dfl_conv_grid_m(const dfl_conv_args* a) {
  dfl::ConvRoute r;
  const int rc = dfl::conv_route(a, dfl::want_splits(a), &r);
  if (rc != DFL_OK) return rc;
  if (r.form == dfl::FORM_BF16) return r.plan.p.splits > 1 ? dfl::convp_finish_rows(r.plan.p) : r.plan.p.npatch;
  if (a->splits > 1) return dfl::conv_finish_rows(r.k.Mtot, a->Ntot);
  if (r.stat_form == dfl::FORM_DIRECT) return dfl::direct_conv_blocks(a);
  if (r.stat_form == dfl::FORM_ROWS) return r.k.Mtot / dfl::conv_rows_bm(r.stat_cfg);
  return (int)dfl::ceil_div(r.k.Mtot, dfl::conv_gemm_bm(r.stat_cfg));
}

extern "C" int dfl_conv_suggest_splits(const dfl_conv_args* a) {
  dfl::ConvRoute r;
  const int rc = dfl::conv_route(a, 0, &r);
  return rc != DFL_OK ? rc : r.splits;
}

extern "C" int dfl_conv_pair_ok(const dfl_conv_args* a, const dfl_conv_args* b) {
  dfl::ConvRoute r;
  return dfl::conv_pair_route(a, b, &r);
}

extern "C" int dfl_conv_candidates(const dfl_conv_args* a, int32_t* out, int32_t max_rows) {
  DFL_REQUIRE(a != nullptr && (out != nullptr || max_rows <= 0) && a->x_bf16, "dfl_conv_candidates: bf16 convolution arguments and an output table are required");
  const int n = dfl::convp_candidates(a, out, max_rows);
  return n < 0 ? (int)DFL_ERR_INVALID_ARG : n;
}

extern "C" int dfl_conv_force_geometry(const int32_t* geom) {
  if (geom == nullptr) dfl::t_force.tile = -1;
  else dfl::t_force = dfl::ConvGeom{geom[0], geom[1], geom[2], geom[3], geom[4]};
  return DFL_OK;
}

extern "C" int dfl_conv_tune_add(const int32_t* key, const int32_t* geom) {
  DFL_REQUIRE(key == nullptr || geom != nullptr, "dfl_conv_tune_add: a key needs a geometry");
  dfl::memo_clear();
  std::lock_guard<std::mutex> lock(dfl::g_tune_mu);
  if (key == nullptr) {
    dfl::g_tune.clear();
    return DFL_OK;
  }
  dfl::TuneEntry e;
  for (int i = 0; i < 10; ++i) e.key[i] = key[i];
  e.g = dfl::ConvGeom{geom[0], geom[1], geom[2], geom[3], geom[4]};
  for (dfl::TuneEntry& o : dfl::g_tune)
    if (memcmp(o.key, e.key, sizeof(e.key)) == 0) {
      o = e;
      return DFL_OK;
    }
  dfl::g_tune.push_back(e);
  return DFL_OK;
}
