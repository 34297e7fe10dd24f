// The route of dfl_conv2d and of its queries (conv_plan.hip): which kernel family takes an argument block.
#pragma once
#include "conv_epilogue.h"
#include "convp.h"

namespace dfl {

// The generic GEMM kernels of fp32 tensors (conv_gemm.hip)
int conv_prepare(const dfl_conv_args* a, ConvK* k);    // validates the block and fills k (k.splits = 1)
int conv_gemm_cfg(const ConvK& k);                     // the tile they take: what dfl_conv_config reports
int conv_gemm_bm(int cfg);                             // ... its pixels
int conv_gemm_splits(const ConvK& k);                  // the K slices they suggest
int conv_finish_rows(int M, int Ntot);                 // row blocks of conv_finish_kernel (= rows of stat_partials with K slices)

enum ConvForm {
  FORM_BF16,        // bf16 tensors: plan.p.tile names the family (patch, latency, unrolled 3x3, narrow 3x3)
  FORM_FIRST,       // the 1-channel 3x3 first layer in latency form (convs.hip)
  FORM_LATENCY32,   // the latency form of fp32 tensors (convs.hip; its K slices end in conv_finish of conv_gemm.hip)
  FORM_DIRECT,      // direct small-K kernels (direct_small.hip)
  FORM_ROWS,        // row-tiled 3x3 kernels (conv_rows.hip)
  FORM_GEMM,        // generic GEMM kernels (conv_gemm.hip)
};

struct ConvRoute {
  ConvForm form;    // what dfl_conv2d launches
  int cfg;          // what dfl_conv_config reports
  int splits;       // K slices: the planned ones, or with none requested the form's suggestion
  ConvPlan plan;    // FORM_BF16, FORM_LATENCY32
  ConvK k;          // fp32 tensors: the validated block
  ConvForm stat_form;   // fp32 tensors: the form without the latency forms, which take no statistics -- what sizes stat_partials
  int stat_cfg;         // ... and its tile
};

// want_splits: 0 = the forms choose (dfl_conv_suggest_splits), else the K slices to plan for (dfl_args.splits, at least 1)
int conv_route(const dfl_conv_args* a, int want_splits, ConvRoute* r);
// 1 / 2 (dfl_conv_pair_ok) when a and b run as one launch; r = a's route
int conv_pair_route(const dfl_conv_args* a, const dfl_conv_args* b, ConvRoute* r);

}  // namespace dfl
