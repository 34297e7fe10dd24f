// Patch-resident bf16 convolution and weight-gradient kernels (convp_bf16.hip, wgradp_bf16.hip), dispatched by
// dfl_conv2d / dfl_conv2d_wgrad when the argument block says its tensors are bf16.
#pragma once
#include "common.h"

namespace dfl {

struct ConvP {
  dfl_conv_args a;
  int Mtot, Cout;               // GEMM rows (gather-grid pixels), channels per output pixel
  int Hg, Wg;                   // gather grid per image (= Hout x Wout; Hin x Win for the 2x2-scatter form)
  int PH, PW, IPP;              // patch: PH x PW grid pixels of IPP images (IPP > 1 only for whole images)
  int npy, npx, npatch;         // patches per image along y / x, patches in all
  int IH, IW;                   // input pixels a patch needs per image, halo included
  int CK, nblk, blk_per_slice;  // input channels resident in LDS per block, blocks over Cin, blocks per K slice
  int splits, T;                // K slices (grid.z), taps
  int pix_stride, upp_shift;    // bytes per staged pixel (2 CK + 16), log2(CK / 8)
  int lds_bytes, tile;          // staged image size, index into the tile configuration table
  int ntiles, grid, xcd_mode;   // column tiles; workgroups launched (linear grid); workgroup -> (patch, tile, slice) map
  uint32_t x_bytes, w_bytes;
  uint32_t x2_bytes, xo_bytes;  // extent of the second input tensor (dfl_conv_args.x_mode) and of x_out
  uint32_t mPP, mPW;            // ceil(2^32 / (PH * PW)), ceil(2^32 / PW): divisions of patch row indices by multiply-high
  int tab_off, pad1;            // LDS offset of the live-BatchNorm tables (set by the planner)
  // latency form (convs.hip; tile == CONVS_TILE): 32 x 32 tiles over (pixels, columns), waves of a workgroup per tile (log2),
  // 16-channel chunks per tap (log2), k-steps of the layer and per wave
  int s_mt, s_nt, s_ksplit_shift, s_cpk_shift, s_ksteps, s_kper;
  // unrolled 3x3 form (convq_bf16.hip; tiles 40 ... 57): ceil(2^32 / d) for d = npatch, ntiles, patches per image, npx
  // (narrow form, convn_bf16.hip, tiles 58 ... 65: qm_perimg, qm_npx; q_ngroups = patches per XCD)
  uint32_t qm_npatch, qm_ntiles, qm_perimg, qm_npx;
  int q_ngroups, q_stride;      // persistent form: workgroups per (column tile, K slice); qm_npatch is then the magic of q_ngroups
                                // (narrow form: patches per XCD; its persistent form: workgroups per XCD = the stride of a workgroup's patches)
};
constexpr int CONVS_TILE = 39;  // value of ConvP.tile for the latency form (conv_plan.hip lists every tile configuration)
constexpr int kLdsOptIn = 160 * 1024;   // dynamic LDS the bf16 convolution kernels opt in to; every plan stays within it

struct ConvPlan;
typedef int (*ConvLaunch)(const ConvPlan& pl, hipStream_t s);

// What the planner (conv_plan.hip) hands a launcher: the kernel argument and the host-only part of the plan
struct ConvPlan {
  ConvP p;                      // tab_off included
  size_t lds;                   // dynamic LDS of the launch
  ConvLaunch launch;            // the configuration's launcher (convp_launch calls it)
  int pers;                     // the configuration's persistent form
  double cost;                  // modelled cycles (0: chosen only through the measured table)
};

// Chooses the geometry for these arguments.  force_splits: 0 = free choice, else the K-slice count to plan for.
int convp_plan(const dfl_conv_args* a, ConvPlan* pl, int force_splits);
int convp_launch(const ConvPlan& pl, hipStream_t s);
int convp_finish_rows(const ConvP& p);
bool convs_enabled();                                             // DFL_CONVS: 0 = the latency forms are never taken

// Patch-resident configurations (convp_bf16.hip): WM x WN waves of TM x TN 32 x 32 tiles; GA: A fragments straight from global
// memory (1x1 windows); KS: k-groups (1 or 2)
struct PatchTile { int WM, WN, TM, TN, GA, KS; ConvLaunch launch; };
constexpr int kNumPatchTiles = CONVS_TILE;
const PatchTile* convp_tiles();                                   // the kNumPatchTiles configurations

// Unrolled 3x3 form for the deep levels (convq_bf16.hip): 8 WM x 12 patches, 32 WN columns, KS k-groups, 64 / 128 resident channels
struct QLayout { int WM, WN, KS; ConvLaunch launch; };            // launch: pers = the persistent form (a workgroup walks q_ngroups-strided patches)
constexpr int kNumQ = 9;
const QLayout* convq_layouts();                                  // the kNumQ layouts
bool convq_shape_ok(const dfl_conv_args& a);
size_t convq_lds_bytes(int ck, int layout, int blk_per_slice, int pers, int* tab_off);   // LDS a workgroup asks for
bool convq_pers_ok(int layout, int ck, int x_mode);              // is the persistent form built for this layout / operand?
bool convq_ck_ok(int layout, int ck);                             // is the layout instantiated for ck resident channels?

// Narrow 3x3 form for the shallow levels (convn_bf16.hip): 32 / 64 output columns, epilogue on the accumulator registers
struct NLayout { int WX, R; ConvLaunch launch; };                 // waves side by side (32 pixels each) x rows per wave
constexpr int kNumN = 6;
const NLayout* convn_layouts();                                  // the kNumN layouts
bool convn_shape_ok(const dfl_conv_args& a);
bool convn_layout_ok(int layout, int ntot, int cin);              // is the layout built for this column count / one or several channel blocks?
size_t convn_lds_bytes(int layout, int cin, int ntot, int pers, int* tab_off);
bool convn_pers_ok(int layout, const dfl_conv_args& a);            // is the persistent form built for this layout / layer?

// Latency form for the small problems of a batch-1 inference forward (convs.hip): bf16 tensors, and fp32 tensors in math modes 0
// (fp32 matrix instructions) and 1 (bf16x3).  p: the validated block's layer constants; the plan is its s_* fields
bool convs_eligible(const dfl_conv_args& a, const ConvP& p);
void convs_plan(const dfl_conv_args& a, ConvP* p, int force_splits);
int convs_launch(const ConvPlan& pl, hipStream_t s);                      // (the K-slice finish is the caller's)
bool convs_first_ok(const dfl_conv_args* a);                              // the 1-channel 3x3 first layer
int convs_first_launch(const dfl_conv_args* a, hipStream_t s);
int convs_pair_ok(const dfl_conv_args* a, const dfl_conv_args* b, const ConvP& pa);   // dfl_conv_pair_ok; pa = a's plan
int convs_pair_launch(const ConvP& pa, const dfl_conv_args* b, hipStream_t s);

struct WgP;
int wgradp_suggest_splits(const dfl_wgrad_args* a);
int wgradp_launch(const dfl_wgrad_args* a, hipStream_t s);
int wgradp_config(const dfl_wgrad_args* a);

}  // namespace dfl
