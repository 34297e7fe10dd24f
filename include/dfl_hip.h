/*
 * dfl_hip.h -- C ABI of libdfl_hip.so: the MI355X (gfx950) implementation of the U-Net hot path of
 * rg2/DeepFluoroLabeling-IPCAI2020 (train_test_code/unet.py, dice.py, ncc.py, util.py ensemble).
 *
 * The reference has no FFI layer: its hot path is torch.nn calls made from Python.  Each entry
 * point below replaces one group of those calls and cites it (paths relative to the reference repo root).
 *
 * Conventions
 *   - every function returns 0 on success or a negative dfl_status; it never throws and never allocates or
 *     frees device memory: the caller owns every buffer and passes raw device pointers;
 *   - work is enqueued asynchronously on the given hipStream_t (pass the host framework's current stream);
 *   - re-entrant; no global mutable state except the thread-local last-error string;
 *   - arithmetic type: fp32 (exact-f32 MFMA v_mfma_f32_32x32x2_f32 for the contractions, fp64 for the
 *     cross-block part of the statistics/loss reductions); dfl_set_math_mode selects bf16-product variants, and
 *     math mode 4 ("bf16 storage") keeps the network's internal activations, their gradients and the GEMM
 *     copies of the weights as bf16 in HBM: argument blocks then carry *_bf16 flags, the flagged pointers address
 *     bf16 elements (declared `float*` / `const float*` here for the common case) and their ld* count elements;
 *   - ACTIVATION LAYOUT inside the network is NHWC ("pixel-major"): element (n,y,x,c) of a tensor with pixel
 *     stride ld (in floats, ld >= C) lives at ((n*H + y)*W + x)*ld + c.  A channel slice of a wider buffer is
 *     expressed by offsetting the pointer and keeping ld (this is how torch.cat in unet.py:256-257 is made
 *     free).  The network input (C = 1) and the two outputs (seg / heat maps) are plain NCHW as in the
 *     reference, so the layout is invisible at the boundary.
 */
#ifndef DFL_HIP_H
#define DFL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dfl_stream_t; /* hipStream_t */

typedef enum {
  DFL_OK = 0,
  DFL_ERR_INVALID_ARG = -1,
  DFL_ERR_UNSUPPORTED = -2,
  DFL_ERR_LAUNCH = -3,
  DFL_ERR_WORKSPACE = -4
} dfl_status;

/* Library version (major*10000 + minor*100 + patch) and the last error message of the calling thread. */
int dfl_version(void);
const char* dfl_last_error(void);
/* sizeof() of the argument structs, in declaration order (conv, wgrad, pack_job, bn_finalize, colstats,
 * bn_bwd_finalize, bn_relu_bwd, affine_copy, pool, head_fwd, head_bwd, loss, ensemble, op, reduce_job, prep,
 * est_lands, upsample, augment_args, augment_item, overlay, resample_plan, resample_args, fullres, mesh_mc,
 * mesh_decode, mesh_topo, mesh_csr, mesh_smooth, mesh_xform, mesh_normals, preproc_projs, preproc_segs, restore_labels,
 * sim_prepare, sim_gradncc, expose, tools_capsule, tools_args, sim_patch_prepare, sim_patch_gradncc, raster_mesh, raster_args, sim_gradncc_bwd, sim_patch_weights,
 * sim_patch_eval, drr_pose_grad, sim_bank_gradncc, sim_bank_gradncc_bwd, sim_patch_bank_gradncc, drr_object, drr_args, optim_pack): lets a
 * binding written in another language verify the size of its struct mirrors at load time.  Returns -1 past the end.
 * Sizes say nothing about field order or type: the Python binding derives its structs, constants and signatures from this
 * file (dfl_amd/_cabi.py), and tests/test_cabi_cpu.py holds every field offset against a C compiler's offsetof. */
int dfl_sizeof(int which);

/* ------------------------------------------------------------------------------------------------------------
 * Convolution as a gather-GEMM on the fp32 matrix cores.
 *   y[m, n] = epilogue( sum_{t < KH*KW} sum_{c < Cin} X(m, t, c) * W(k = t*Cin + c, n) )
 * m runs over the N*Hout*Wout output pixels; X(m,t,c) is the input at pixel (oy*stride - pad + t/KW,
 * ox*stride - pad + t%KW), channel c, after the optional per-channel affine in_scale/in_shift (BatchNorm
 * applied on load), and 0 outside the image (zero padding is applied AFTER the affine, as the reference pads
 * the BatchNorm output).
 * Replaces nn.Conv2d 3x3 (unet.py:211,218), 1x1 residual (unet.py:207,229-231), 2x2/stride-2 down-sampling
 * (unet.py:93,171), nn.ConvTranspose2d(k=2,s=2) (unet.py:240,255; scatter2x2 = 1) and -- with the packed
 * weights of dfl_pack_weights -- every data-gradient of those layers (torch autograd, train.py:422).
 * Epilogue order: + bias[n]; ReLU (unet.py:213,220); + add[m,n]*add_scale[n] + add_shift[n] (the BatchNorm
 * of the block's last conv, summed with the residual: unet.py:229-231); + old y (accumulate); store;
 * per-channel partial sums of v and v*u for BatchNorm (u = v, or u = stat_other[m,n]).
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
  const float* x;        /* input activations, NHWC, pixel stride ldx */
  const float* w;        /* quad-packed weights [ceil(KH*KW*Cin/4)][Ntot][4] (dfl_pack_weights), 16-byte aligned */
  const float* bias;     /* [Ntot / (scatter2x2 ? 4 : 1)] or NULL */
  const float* in_scale; /* [Cin] or NULL */
  const float* in_shift; /* [Cin] or NULL (required when in_scale is given) */
  const float* add;      /* [M][ldadd] or NULL */
  const float* add_scale;/* [Ntot] or NULL (=> scale 1, shift 0) */
  const float* add_shift;
  const float* stat_other; /* [M][ldso] or NULL (=> u = v) */
  float* y;              /* output, NHWC, pixel stride ldy */
  float* stat_partials;  /* [gridM][2][Ntot] or NULL; gridM = dfl_conv_grid_m(args).  With scatter2x2 (bf16 tensors only):
                            [4*gridM][2][Cout], the sums of y's Cout channels (stat_other is then addressed like y) */
  float* partial;        /* split-K scratch [splits][M][Ntot], required when splits > 1 */
  int32_t N, Hin, Win, Cin, ldx;
  int32_t KH, KW, stride, pad;
  int32_t Hout, Wout, Ntot, ldy;
  int32_t ldadd, ldso;
  int32_t relu;
  int32_t accumulate;
  int32_t scatter2x2;    /* ConvTranspose2d(k2,s2): Ntot = 4*Cout, column ab*Cout+co of input pixel (i,j) is stored
                            at output pixel (2i + ab/2, 2j + ab%2) of an [N, Hout, Wout] image, channel co */
  int32_t splits;        /* 0/1: one pass.  > 1: K is cut into `splits` slices (small-M, long-K layers of the deep
                            U-Net levels), raw sums go to `partial` and a finish kernel applies the epilogue */
  /* "Split" operands (math mode 1, bf16x3, fast path only): the 16-byte slot of 4 consecutive fp32 values holds their
   * 4 hi bf16 followed by their 4 lo bf16 (hi = bf16(v), lo = bf16(v - hi)) -- same addressing, and the kernel copies
   * the slot to LDS instead of splitting it itself (a value is otherwise split once per tap and column block). */
  int32_t w_split;       /* w was packed with dfl_pack_job.split = 1 (2: bf16 chunk layout, required when x_bf16) */
  int32_t x_split;       /* x is a split tensor (written by dfl_bn_relu_bwd_apply with split_out); needs in_scale == NULL */
  /* bf16 tensors (math mode 4).  x_bf16: x is bf16 NHWC (Cin % 16 == 0, ldx % 8 == 0), w is the bf16 chunk layout
   * [ceil(K/16)][Ntot][16] of dfl_pack_job.split = 2; the patch-resident kernels of csrc/convp_bf16.hip run.
   * y_bf16: y, add and stat_other are bf16 (values are rounded once, statistics are taken from the rounded values).
   * The direct small-K kernels (Cin <= 4: the network's first layer) take x_bf16 = 0, y_bf16 = 1. */
  int32_t x_bf16, y_bf16;
  /* BatchNorm + ReLU backward fused into the operand (bf16 patch kernels, x_mode = 1): x is dy, x2 the saved ReLU output r
   * (same shape, pixel stride ldx2) and the convolution's operand is  [r > 0] * (A*dy + B*r + C)  with A, B, C = in_scale[0..C),
   * [C..2C), [2C..3C) -- the coefficients dfl_bn_bwd_finalize leaves (in_scale NULL: plain ReLU backward [r > 0] * dy; in_shift
   * must be NULL).  What dfl_bn_relu_bwd_apply would materialise is never written: one tensor pass and one launch per layer less. */
  const float* x2;
  int32_t ldx2, x_mode;
  /* "Live" BatchNorm statistics (bf16 patch kernels, training; round 4).  Between a convolution and the next one stands
   * nn.BatchNorm2d in training mode (unet.py:214-222): the consumer needs scale / shift made of the producer's batch statistics.
   * dfl_bn_finalize between the two is a 5 us launch in the dependency chain, 44 times per step.  Instead:
   *   stat_totals  the producer ADDS its workgroups' column sums (sum v, sum v*v of the stored values) into [DFL_BN_R][2][Ntot]
   *                doubles with hardware fp64 atomics (row = workgroup % DFL_BN_R spreads the contention; the addends are fp32
   *                values of similar magnitude, their fp64 sum is exact -- independent of the order -- unless one of them is below
   *                2^-29 of the total).  The caller zeroes the rows before the producer runs.  stat_partials may be NULL then.
   *   in_tot       (instead of in_scale / in_shift) the consumer derives scale / shift of its input channels itself, with the
   *                arithmetic of dfl_bn_finalize: mean = s1 / count, var = s2 / count - mean^2 (biased, >= 0),
   *                scale = gamma / sqrt(var + eps), shift = beta - mean * scale, from in_tot [DFL_BN_R][2][Cin], in_gamma, in_beta.
   *   add_tot      the same for the epilogue's "+ add * add_scale + add_shift" (add_gamma, add_beta, [DFL_BN_R][2][Ntot]).
   * dfl_bn_finalize_live (one batched launch per forward pass) turns the totals into the vectors the backward pass and the
   * module state need (scale, shift, mean, invstd, running statistics). */
  double* stat_totals;
  const double* in_tot;
  const float* in_gamma;
  const float* in_beta;
  const double* add_tot;
  const float* add_gamma;
  const float* add_beta;
  double in_count, add_count;
  float bn_eps;
  int32_t reserved3;
  /* ... and for the BatchNorm + ReLU backward operand (x_mode = 1): with in_tot the three coefficients are not read from
   * in_scale but derived from the totals (sum dy, sum dy*r) [DFL_BN_R][2][Cin] left by the kernel that produced dy
   * (stat_totals together with stat_other), in_gamma, the layer's saved mean / 1/std (in_mean, in_invstd) and in_count -- the
   * arithmetic of dfl_bn_bwd_finalize. */
  const float* in_mean;
  const float* in_invstd;
  /* x_mode = 1, 3x3 stride 1 (round 4): the operand the kernel forms while it stages its patches is ALSO written to x_out
   * (bf16 [N][Hin][Win] pixels of ldxo elements, Cin channels; every element exactly once: a workgroup stores the interior of
   * its patch, its K slice's channels, column tile 0 only) -- the layer's weight gradient then reads one plain tensor
   * (dfl_wgrad_args.d_mode = 0 with bias_partial) instead of forming the same values again from (dy, r) in every (cm, cg) tile.
   * NULL: nothing is written. */
  void* x_out;
  int32_t ldxo;
  /* Latency form (round 5; bf16 tensors: csrc/convs_bf16.hip, fp32 tensors in math modes 0 / 1: csrc/convs_f32.hip): 1 asks for the
   * kernel whose dependency chain is shortest instead of the one with the highest throughput -- for the small problems of a batch-1
   * inference forward (the per-image loops of util.py:116-165 and :318-356: 44 dependent convolutions of 0.01 - 1.4 GFLOP each).  A
   * hint: honoured for at most 65536 output pixels and 1.5 GFLOP, Cin / 16 a power of two (<= 1024 channels), no statistics / live
   * totals / x_mode / x_out; otherwise the throughput kernels run.  Same contract, same roundings (another fp32 summation order);
   * dfl_conv_suggest_splits and dfl_conv_config (16 + 39) answer for the form the hint selects. */
  int32_t latency_form;
  /* Output affine (latency form only, inference): the stored value becomes bf16(out_scale[n] * bf16(v) + out_shift[n]) with v what
   * the epilogue would have stored (fp32 tensors: fma(v, out_scale[n], out_shift[n]), nothing is rounded) -- the eval-mode BatchNorm
   * between this convolution and the next one (unet.py:214-218) applied by the PRODUCER with the consumer's two roundings, so that
   * the consumer reads its operand plain (no affine on load; zero padding after BatchNorm stays zero).  Rejected by every other kernel: ask dfl_conv_config (16 + 39 = latency form) before relying on it. */
  const float* out_scale;
  const float* out_shift;
} dfl_conv_args;
#define DFL_BN_R 8

int dfl_conv2d(const dfl_conv_args* a, dfl_stream_t stream);
/* The last 3x3 convolution of a residual block and the block's 1x1 convolution (unet.py:218-231) as ONE launch.  Defined as
 * dfl_conv2d(a) followed by dfl_conv2d(b) -- both outputs are written, same roundings (y1 is rounded to bf16 before b's epilogue
 * adds its BatchNorm) -- and performed as one kernel when dfl_conv_pair_ok(a, b) says 1: a in latency form without K slices, add
 * or scatter; b a 1x1 / stride-1 convolution over the same pixels and columns with add == a->y, add_scale / add_shift, no ReLU,
 * no statistics, its input bf16 (Cin % 16 == 0) or the 1-channel fp32 image of the network's first block.  Otherwise the two
 * launches run one after the other.  A batch-1 forward has 11 such pairs among its 44 dependent convolutions.
 * dfl_conv_pair_ok: 0 = two launches; 1 = one kernel; 2 = a is K-sliced (a->splits > 1): one kernel + ONE finish launch for both
 * outputs, and a->partial must then hold 2 * splits * M * Ntot floats (the second half takes the 1x1 product's slices) -- with a
 * buffer of the single-convolution size the caller must not ask for the pair. */
int dfl_conv2d_pair(const dfl_conv_args* a, const dfl_conv_args* b, dfl_stream_t stream);
int dfl_conv_pair_ok(const dfl_conv_args* a, const dfl_conv_args* b);
/* Number of row blocks whose statistics dfl_conv2d will write for these args (= first dim of stat_partials);
 * depends on a->splits, so set that first. */
int dfl_conv_grid_m(const dfl_conv_args* a);
/* Suggested split-K factor for these args (>= 1); the caller sizes `partial` as splits*M*Ntot floats. */
int dfl_conv_suggest_splits(const dfl_conv_args* a);
/* dfl_conv_config, dfl_conv_grid_m and dfl_conv_suggest_splits answer for the kernel the block selects (csrc/conv_plan.hip), and
 * the fields that select it are the shapes, latency_form, add, accumulate, x_mode, x_out, scatter2x2 and splits -- for the latency
 * form also whether statistics are asked for (stat_partials / stat_totals / stat_other).  Set these before asking. */

/* Geometry search of the bf16 convolution (csrc/conv_plan.hip).  A geometry is 5 integers: tile configuration (the
 * value dfl_conv_config reports - 16), images per patch, patch height, patch width, K slices.  By default a cost model
 * picks one per layer; a tuning table (measured on the device: tools/tune_convp.py -> dfl_amd/tune/gfx950_convp.txt,
 * loaded when the library is opened) overrides it for the layers it lists.
 *   dfl_conv_candidates     the valid geometries of a layer: writes up to max_rows rows of 5 integers, returns their number
 *   dfl_conv_force_geometry every following dfl_conv_* call of this thread uses `geom` (error if invalid for the layer);
 *                           NULL returns to the table / model.  For tuners and tests.
 *   dfl_conv_tune_add       table entry: key = {N, Hin, Win, Cin, Ntot, KH, KW, stride, pad, scatter2x2} -> geom; a key
 *                           that is already present is replaced; key = NULL empties the table.  An entry is used when it
 *                           is valid and agrees with the caller's `splits`. */
int dfl_conv_candidates(const dfl_conv_args* a, int32_t* out, int32_t max_rows);
int dfl_conv_force_geometry(const int32_t* geom);
int dfl_conv_tune_add(const int32_t* key, const int32_t* geom);

/* ------------------------------------------------------------------------------------------------------------
 * Weight gradient of the same family of layers (torch autograd of unet.py:93,207,211,218,240):
 *   dw[(cm*Cg + cg)*T + t] = sum_m d[m, cm] * G(m, t, cg)
 * G is gathered exactly like X above (taps, stride, pad, affine-on-load, zero padding); d is dense over the
 * same M pixels.  Conv2d: G = layer input, d = output gradient, (cm,cg) = (Cout,Cin) => dw has the torch
 * layout [Cout][Cin][KH][KW].  ConvTranspose2d(k2,s2): G = output gradient gathered with stride 2, d = layer
 * input => [Cin][Cout][2][2].  The pixel range is split over `splits` blocks; with splits > 1 the kernel writes
 * partial[split][T][Cm][Cg] (tap-major: the accumulator tiles store as full 128-byte rows instead of 4-byte
 * scatters) and dfl_sum_partials / dfl_reduce_batch finish the sum into dw, transposing to [Cm][Cg][T].
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
  const float* g;        /* gathered tensor, NHWC, pixel stride ldg */
  const float* d;        /* dense tensor [M][ldd] */
  const float* in_scale; /* [Cg] or NULL: affine on load of g */
  const float* in_shift;
  float* dw;             /* [Cm][Cg][T] when splits == 1 */
  float* partial;        /* [splits][T][Cm][Cg] when splits > 1 */
  int32_t N, Hin, Win, Cg, ldg;
  int32_t KH, KW, stride, pad;
  int32_t Hout, Wout, Cm, ldd;
  int32_t splits;
  int32_t d_split;       /* d is a split tensor (see dfl_conv_args.x_split); math mode 1 fast path only */
  int32_t g_bf16, d_bf16;/* g / d are bf16 tensors (math mode 4; csrc/wgradp_bf16.hip when both are; the direct small-K
                            kernels take g_bf16 = 0, d_bf16 = 1) */
  /* BatchNorm + ReLU backward fused into the dense operand (bf16 patch kernels, d_mode = 1): d is dy, d2 the saved ReLU output
   * r (pixel stride ldd2), coef the [3][Cm] coefficients of dfl_bn_bwd_finalize (NULL: plain ReLU backward) and the operand is
   * [r > 0] * (A*dy + B*r + C), as dfl_conv_args.x_mode.  bias_partial (optional; 3x3 bf16 patch kernel: with d_mode 0 as well --
   * d is then the operand itself, materialised by dfl_conv_args.x_out): [splits][Cm] fp32 -- the column sums of the
   * operand over each pixel slice, i.e. the partial sums of the layer's BIAS gradient that dfl_bn_relu_bwd_apply used to leave. */
  int32_t d_mode;
  const float* d2;
  const float* coef;
  float* bias_partial;
  int32_t ldd2, reserved2;
  /* Live statistics (dfl_conv_args.stat_totals; round 4): instead of `coef` the kernel derives A, B, C itself from coef_tot
   * [DFL_BN_R][2][Cm] = totals of (sum dy, sum dy*r), bn_gamma, the saved mean / 1/std and bn_count (dfl_bn_bwd_finalize's arithmetic). */
  const double* coef_tot;
  const float* bn_gamma;
  const float* bn_mean;
  const float* bn_invstd;
  double bn_count;
} dfl_wgrad_args;

int dfl_conv2d_wgrad(const dfl_wgrad_args* a, dfl_stream_t stream);
/* Suggested number of splits for a problem (>= 1); the caller sizes `partial` from it. */
int dfl_wgrad_suggest_splits(const dfl_wgrad_args* a);

/* dst[r*T + t] = sum_{s < splits} src[s*n + t*(n/T) + r],  r < n/T, t < T  (T = 1: plain sum of slices); fp64 accumulation
 * in a fixed order, rounded to fp32 once. */
int dfl_sum_partials(const float* src, float* dst, int64_t n, int32_t splits, int32_t T, dfl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Batched weight re-layout (one launch for the whole network).  dfl_conv2d consumes its weights "quad-packed":
 *   w[(k/4)*Ntot*4 + n*4 + k%4] = W(k, n),  k < K = taps*Cin rounded up to a multiple of 4 with zeros,
 * i.e. one float4 holds four consecutive k of one output column.  Job j builds that matrix from a contiguous
 * parameter src[A][B][C] (C = KH*KW) with one of three index maps:
 *   kind 1: k = c*B + b,  n = a        forward operand of Conv2d        (src [Cout][Cin][T])
 *                                      data gradient of ConvTranspose2d (src [Cin][Cout][T]: k = (tap,co), n = ci)
 *   kind 2: k = c'*A + a, n = b        data gradient of a stride-1 Conv2d (src [Cout][Cin][T]); flip: c = C-1-c'
 *   kind 3: k = a,  n = c*B + b        scatter forms: ConvTranspose2d forward (src [Cin][Cout][4]) and the data
 *                                      gradient of Conv2d(k2,s2) (src [Cout][Cin][4])
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
  const float* src;
  float* dst;            /* ceil(K/4) * Ntot * 4 floats */
  int32_t A, B, C;
  int32_t kind, flip;
  int32_t split;         /* 1: write split quads (4 hi bf16 | 4 lo bf16) instead of 4 floats (dfl_conv_args.w_split);
                            2: bf16 chunk layout w[(k/16)*Ntot*16 + n*16 + k%16] (K rounded up to 16 with zeros): one MFMA B
                            fragment of 32 columns is 1 KiB contiguous; dst holds ceil(K/16)*Ntot*16 bf16 */
  /* dfl_pack_weights_tiled only (round 4): a SECOND layout of the same parameter written from the same read of it (the
   * forward operand and the data-gradient operand of a layer: the fp32 master is read once instead of twice), and the job's
   * first tile in the launch's flat tile list (tiles of 32 x 32 x C; a job has (A/32)*(B/32) of them). */
  float* dst2;           /* NULL: one layout */
  int32_t kind2, flip2;
  int32_t first_tile;
  int32_t split2;        /* format of dst2 (as split; round 5: the tiled launches write every format, not only the bf16 chunks) */
} dfl_pack_job;

/* jobs: DEVICE pointer to njobs dfl_pack_job records; max_elems = max over jobs of A*B*C. */
int dfl_pack_weights(const dfl_pack_job* jobs_dev, int32_t njobs, int64_t max_elems, dfl_stream_t stream);
/* The layouts of parameters with A % 32 == 0, B % 32 == 0, C <= 9 (any format: fp32 quads, split quads, bf16 chunks): one workgroup
 * per 32 x 32 x C tile of all jobs (first_tile: ascending prefix sums, total_tiles their sum), 16-byte loads, both layouts of a job
 * from one LDS tile. */
int dfl_pack_weights_tiled(const dfl_pack_job* jobs_dev, int32_t njobs, int32_t total_tiles, dfl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * BatchNorm2d (unet.py:215,222; torch defaults eps 1e-5, momentum 0.1).
 * Training forward: the producing dfl_conv2d leaves per-block partial sums; dfl_bn_finalize reduces them in
 * fp64, emits scale = gamma*invstd, shift = beta - mean*scale (consumers apply them on load), saves mean and
 * invstd for backward, and updates running_mean / running_var (unbiased) / num_batches_tracked.
 * Eval forward (util.py:120,173,261,313): dfl_bn_eval_prepare derives scale/shift from the running statistics.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
  const float* partials; /* [nblocks][2][C]: sum x, sum x^2 */
  const float* gamma;    /* [C] */
  const float* beta;     /* [C] */
  float* running_mean;   /* [C] or NULL */
  float* running_var;    /* [C] or NULL */
  int64_t* num_batches_tracked; /* scalar or NULL */
  float* scale;          /* [C] out */
  float* shift;          /* [C] out */
  float* save_mean;      /* [C] out */
  float* save_invstd;    /* [C] out */
  int64_t count;         /* N*H*W */
  int32_t nblocks, C;
  float eps, momentum;
} dfl_bn_finalize_args;

int dfl_bn_finalize(const dfl_bn_finalize_args* a, dfl_stream_t stream);

/* The same for "live" statistics (dfl_conv_args.stat_totals): ONE launch for all BatchNorm layers of a forward pass, after the
 * last of them -- the convolutions in between derived their scale / shift from the totals themselves.  Each job turns
 * totals [DFL_BN_R][2][C] into scale / shift / save_mean / save_invstd (what the backward pass and tests read) and updates the
 * running statistics (momentum, unbiased variance, num_batches_tracked += 1: nn.BatchNorm2d in training mode, unet.py:215,222).
 * `jobs_dev` lives in device memory. */
typedef struct {
  const double* totals;
  const float* gamma; const float* beta;
  float* running_mean; float* running_var; int64_t* num_batches_tracked;   /* all three NULL: no module state to update */
  float* scale; float* shift; float* save_mean; float* save_invstd;
  int64_t count;
  int32_t C;
  float eps, momentum;
  int32_t reserved;
} dfl_bn_live_job;
int dfl_bn_finalize_live(const dfl_bn_live_job* jobs_dev, int32_t njobs, int32_t max_C, dfl_stream_t stream);
/* Backward counterpart: what dfl_bn_bwd_finalize writes besides the coefficients (which the consumers derive themselves) --
 * dgamma = invstd * (sum dy*r - mean * sum dy), dbeta = sum dy, and optionally `sum_out` = sum dy (the bias gradient of the
 * residual 1x1 convolution that shares the block's output gradient) -- for a batch of layers in one launch. */
typedef struct {
  const double* totals;
  const float* save_mean; const float* save_invstd;
  float* dgamma; float* dbeta; float* sum_out;     /* sum_out may be NULL */
  int32_t C, reserved;
} dfl_bn_bwd_live_job;
int dfl_bn_bwd_finalize_live(const dfl_bn_bwd_live_job* jobs_dev, int32_t njobs, int32_t max_C, dfl_stream_t stream);
int dfl_bn_eval_prepare(const float* gamma, const float* beta, const float* running_mean,
                        const float* running_var, float* scale, float* shift, int32_t C, float eps,
                        dfl_stream_t stream);

/* Row-block count the streaming reductions below use for an [M][C] tensor (pure function; the caller sizes the
 * partial buffers and sets `nblocks` from it). */
int dfl_rowblock_count(int64_t M, int32_t C);

/* Per-channel partial sums over pixels: partials[blk][0][c] = sum a, partials[blk][1][c] = sum a*b (b NULL => a*a);
 * `partials` holds nblocks*2*C floats, nblocks = dfl_rowblock_count(M, C). */
typedef struct {
  const float* a; const float* b;
  float* partials;
  int64_t M;
  int32_t C, lda, ldb, nblocks;
  int32_t bf16, reserved;   /* bf16 = 1: a and b are bf16 tensors */
} dfl_colstats_args;
int dfl_colstats(const dfl_colstats_args* a, dfl_stream_t stream);

/* BatchNorm + ReLU backward (torch autograd of unet.py:213-215,220-222), two steps:
 * dfl_bn_bwd_finalize: from partial sums of (dy, dy*r) (r = the saved ReLU output that was normalised) computes
 *   dgamma, dbeta and the three coefficients A,B,C such that  d(pre-activation) = [r > 0] * (A*dy + B*r + C).
 * dfl_bn_relu_bwd_apply: materialises that tensor and leaves partial sums of it (the conv bias gradient).
 * With coef == NULL the apply step is the plain ReLU backward [r > 0] * dy (batch_norm=False). */
typedef struct {
  const float* partials; /* [nblocks][2][C]: sum dy, sum dy*r */
  const float* gamma; const float* save_mean; const float* save_invstd;
  float* dgamma; float* dbeta;   /* [C] */
  float* coef;                   /* [3][C] */
  int64_t count;                 /* elements per channel; 0: save_mean / save_invstd are constants (eval mode, running
                                    statistics): A = gamma * invstd, B = C = 0 */
  int32_t nblocks, C;
} dfl_bn_bwd_finalize_args;
int dfl_bn_bwd_finalize(const dfl_bn_bwd_finalize_args* a, dfl_stream_t stream);

typedef struct {
  const float* dy; const float* r; const float* coef; /* coef [3][C] or NULL */
  float* dpre;            /* [M][ldo] */
  float* partials;        /* [nblocks][C] sums of dpre (nblocks = dfl_rowblock_count(M, C)), or NULL */
  int64_t M;
  int32_t C, lddy, ldr, ldo, nblocks;
  int32_t split_out;      /* 1: dpre is written as a split tensor (needs C % 4 == 0, ldo % 4 == 0, 16-byte alignment) */
  int32_t bf16, reserved; /* bf16 = 1: dy, r and dpre are bf16 tensors (C % 8 == 0, ld % 8 == 0); the sums are of the rounded dpre */
} dfl_bn_relu_bwd_args;
int dfl_bn_relu_bwd_apply(const dfl_bn_relu_bwd_args* a, dfl_stream_t stream);

/* out[c] = sum_{b < nblocks} partials[b*stride + c]  (fp64 accumulation). */
int dfl_reduce_partials(const float* partials, float* out, int32_t nblocks, int32_t stride, int32_t C,
                        dfl_stream_t stream);

/* Batched form of dfl_reduce_partials / dfl_sum_partials: ONE launch finishes many small sums (the per-layer bias
 * gradients and the pixel-slice partials of dfl_conv2d_wgrad of a whole backward pass; the recorded program defers
 * them to a few flush points instead of one launch per layer).  Job j:  dst[i'] = sum_{k < count} src[k*stride + i],
 * i < n, accumulated in fp64 in a fixed order (bit-reproducible); i' = i for T <= 1, else the tap-major ->
 * [..][T] transposition i' = (i % (n/T))*T + i/(n/T) of dfl_conv2d_wgrad's slices.  first_block is the prefix sum of
 * dfl_reduce_job_blocks(n, count) over the preceding jobs; total_blocks the sum over all jobs. */
typedef struct {
  const float* src;
  float* dst;
  int64_t n, stride;
  int32_t count, first_block;
  int32_t T, reserved;
} dfl_reduce_job;
int dfl_reduce_job_blocks(int64_t n, int32_t count);
/* jobs: DEVICE pointer to njobs records. */
int dfl_reduce_batch(const dfl_reduce_job* jobs_dev, int32_t njobs, int32_t total_blocks, dfl_stream_t stream);

/* y[m,c] = x[m,c]*scale[c] + shift[c] (+ y_old when accumulate).  scale NULL => copy / add.  Used for the
 * BatchNorm output when a block has no residual branch (do_res=False, unet.py:229) and for the centre-crop copy
 * of the bridge in unpadded mode (unet.py:248-257): src/dst are [N,H,W] windows given by offsets. */
typedef struct {
  const float* x; float* y; const float* scale; const float* shift;
  int32_t N, H, W, C;           /* window size */
  int32_t ldx, xH, xW, xoy, xox;/* source image dims and window origin */
  int32_t ldy, yH, yW, yoy, yox;
  int32_t accumulate;
  int32_t bf16;                 /* 1: x and y are bf16 tensors (C % 8 == 0, ld % 8 == 0) */
} dfl_affine_copy_args;
int dfl_affine_copy(const dfl_affine_copy_args* a, dfl_stream_t stream);

/* Bilinear x2 up-sampling and its adjoint (up_mode='upsample': nn.Upsample(mode='bilinear', scale_factor=2) in front of a 1x1
 * convolution, train_test_code/unet.py:242-244; align_corners=False as torch's default).  fwd: y[N,2H,2W,C] = up(x[N,H,W,C]).
 * bwd: x (+)= up^T(y): x receives the gradient of the small tensor from y, the gradient of the large one. */
typedef struct {
  const void* x; void* y;       /* NHWC with pixel strides ldx / ldy (elements); fp32 or bf16 (both the same) */
  int32_t N, H, W, C;           /* SMALL grid: x is H x W, y is 2H x 2W */
  int32_t ldx, ldy;
  int32_t bf16;                 /* 1: bf16 tensors (C % 8 == 0, ld % 8 == 0) */
  int32_t accumulate;           /* bwd only: add to x instead of overwriting it */
} dfl_upsample_args;
int dfl_upsample2x_fwd(const dfl_upsample_args* a, dfl_stream_t stream);
int dfl_upsample2x_bwd(const dfl_upsample_args* a, dfl_stream_t stream);

/* F.max_pool2d(x, 2) (unet.py:169) and its backward (first maximum in scan order wins; gradient is ADDED to dx). */
typedef struct {
  const float* x; float* y;     /* fwd: x -> y.  bwd: x = saved input, y = dy (read), dx accumulated */
  float* dx;
  int32_t N, H, W, C, ldx, ldy, lddx;   /* H, W: input size; output is floor(H/2) x floor(W/2) */
  int32_t bf16;                          /* 1: x, y and dx are bf16 tensors (C % 8 == 0, ld % 8 == 0) */
} dfl_pool_args;
int dfl_maxpool2x2_fwd(const dfl_pool_args* a, dfl_stream_t stream);
int dfl_maxpool2x2_bwd(const dfl_pool_args* a, dfl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Output heads (unet.py:176-191): logits = seg_conv(x) (1x1, no bias); seg = Softmax2d(logits) (or logits);
 * heat = lands_1x1[1](lands_1x1[0](cat(x, logits))) (two bias-free 1x1 convs; the second is optional).
 * x is NHWC; seg and heat are written NCHW (the reference's output layout).
 * Limits: n_classes <= 16, num_lands <= 32, n_mid <= 48 (the specialised small-array kernels serve up to 8 / 16 / 24).
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
  const float* x;         /* [M][ldx], F features */
  const float* w_seg;     /* [NC][F] */
  const float* w_l1;      /* [NM][F+NC] or NULL when L == 0 */
  const float* w_l2;      /* [L][NM] or NULL (single 1x1: NM == L) */
  float* seg;             /* [N][NC][H][W] */
  float* heat;            /* [N][L][H][W] or NULL */
  int32_t N, H, W, F, ldx;
  int32_t NC, NM, L;
  int32_t softmax;
  int32_t x_bf16;         /* 1: x is a bf16 tensor (F % 8 == 0, ldx % 8 == 0); seg / heat stay fp32 */
} dfl_head_fwd_args;
int dfl_head_fwd(const dfl_head_fwd_args* a, dfl_stream_t stream);

/* Head backward: reads dseg/dheat (NCHW, dheat may be NULL), the saved features and seg, writes dx (NHWC) and a
 * per-pixel scratch [M][DFL_HEAD_SCRATCH_LD] holding cat(x,logits) | dlogits | dmid | mid | dheat (padded,
 * offsets below) from which the three weight gradients are taken with dfl_conv2d_wgrad (1x1). */
#define DFL_HEAD_MAX_NC 8
#define DFL_HEAD_MAX_L 16
#define DFL_HEAD_MAX_NM 24
/* Heads beyond those counts (train.py --num-classes is free) run the same kernels compiled with larger per-thread arrays
 * (generic bounds, no fused weight gradients): up to */
#define DFL_HEAD_LARGE_NC 16
#define DFL_HEAD_LARGE_L 32
#define DFL_HEAD_LARGE_NM 48
typedef struct {
  const float* x; const float* seg; const float* dseg; const float* dheat;
  const float* w_seg; const float* w_l1; const float* w_l2;
  float* dx;              /* [M][lddx] */
  float* scratch;         /* [M][scratch_ld] */
  int32_t N, H, W, F, ldx, lddx;
  int32_t NC, NM, L;
  int32_t softmax;
  int32_t scratch_ld;     /* >= dfl_head_scratch_ld(F) */
  int32_t x_bf16;         /* 1: x and dx are bf16 tensors; the scratch rows stay fp32 */
  /* Fused weight gradients (bf16 features with F == 32 only): when dw_seg is set the kernel takes the three weight
   * gradients itself -- per pixel tile the rows [dlogits | dmid | dheat] and [x | logits | mid], rounded to bf16, are
   * multiplied on the matrix cores (fp32 accumulation), every workgroup leaves one 64 x 64 partial in wg_partial
   * (dfl_head_wgrad_blocks(M) * 4096 floats) and a finish kernel of the same call sums them, in a fixed order, into
   * dw_seg [NC][F], dw_l1 [NM][F+NC] and dw_l2 [L][NM] (NULL where the head has no such layer).  `scratch` is then
   * neither read nor written and may be NULL. */
  float* dw_seg; float* dw_l1; float* dw_l2; float* wg_partial;
  /* Live statistics (matrix-core kernels only; round 4): dx is the gradient entering the BatchNorm of the decoder's last
   * convolution.  With stat_totals the kernel adds (sum dx, sum dx * r) of the values it stores -- r = stat_other, the saved ReLU
   * output of that convolution, [M][ldso] bf16 -- to the layer's totals [DFL_BN_R][2][F] (dfl_conv_args.stat_totals): the
   * dfl_colstats pass over dx and r and its finalize launch are not needed. */
  const float* stat_other;
  double* stat_totals;
  int32_t ldso, reserved4;
} dfl_head_bwd_args;
int dfl_head_bwd(const dfl_head_bwd_args* a, dfl_stream_t stream);
int dfl_head_wgrad_blocks(int64_t M);  /* workgroups (= partial slots) of the fused form for M pixels */
/* scratch row layout for F features: [0, Fc) cat(x, logits) with Fc = roundup4(F+NC_MAX) ; then dlogits (8),
 * dmid (24), mid (24), dheat (16). */
int dfl_head_scratch_ld(int32_t F);
int dfl_head_scratch_off(int32_t F, int32_t which); /* which: 0 cat, 1 dlogits, 2 dmid, 3 mid, 4 dheat */
/* The same for a given head shape: the scratch row of a large head (above) is wider. */
int dfl_head_scratch_ld_for(int32_t F, int32_t NC, int32_t NM, int32_t L);
int dfl_head_scratch_off_for(int32_t F, int32_t NC, int32_t NM, int32_t L, int32_t which);

/* ------------------------------------------------------------------------------------------------------------
 * Losses (dice.py:14-86, ncc.py:12-38) with their closed-form gradients.
 * seg/heat are the network outputs seen through util.center_crop (util.py:92-114): 4-D strided views given by
 * element strides (sN, sC, sH; unit stride along W) over an [B, C, h, w] window; targets likewise.
 *   loss = dice_wgt * mean_n( sum_c d_nc / Ceff ) + heat_wgt * mean_{n,l}( -(ncc_nl + 1)/2 )
 * with d_nc = (-2*sum(t*s) + 1e-4) / (sum t^2 + sum s^2 + 1e-4), classes c >= skip_bg.
 * Outputs: loss (1 float), and when grads are requested dseg/dheat as dense [B,C,h,w] tensors.
 * `sums` is a caller-provided scratch of dfl_loss_scratch_doubles(B,C,L) doubles.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
  const float* seg; const float* tseg;   /* may be NULL when C == 0 (NCC only) */
  const float* heat; const float* theat; /* NULL when L == 0 */
  float* loss;
  float* dseg; float* dheat;             /* NULL => no gradient */
  float* ncc_vals;                       /* [B][L] raw NCC values (ncc.py:38) or NULL */
  double* sums;
  int64_t seg_sN, seg_sC, seg_sH, tseg_sN, tseg_sC, tseg_sH;
  int64_t heat_sN, heat_sC, heat_sH, theat_sN, theat_sC, theat_sH;
  int32_t B, C, L, h, w;
  int32_t skip_bg;
  float dice_wgt, heat_wgt;
  /* Two-stage use (value in forward, gradient in backward -- what autograd asks for): stage 0 = everything in one call;
   * stage 1 = sums + value only, the gradient coefficients stay in `sums`; stage 2 = gradient only, from the coefficients a
   * stage-1 call left in the same `sums` (seg / heat / targets and sizes as then).  In stage 2 the gradients are
   * multiplied by *grad_scale (a DEVICE scalar: the incoming gradient of the loss; NULL = 1) and may be written as
   * strided [B,C,h,w] windows (element strides; all 0 = dense) -- e.g. the interior of a zero-bordered full-size tensor,
   * which is the gradient of the uncropped network output without a padding pass. */
  const float* grad_scale;
  int64_t dseg_sN, dseg_sC, dseg_sH, dheat_sN, dheat_sC, dheat_sH;
  int32_t stage, reserved;
} dfl_loss_args;
int dfl_dice_ncc_loss(const dfl_loss_args* a, dfl_stream_t stream);
int64_t dfl_loss_scratch_doubles(int32_t B, int32_t C, int32_t L);

/* ------------------------------------------------------------------------------------------------------------
 * Ensemble reduction for one image (util.py:326-373): labels = argmax_c( mean_nets crop(seg) ) with torch.max's
 * first-maximum rule, uint8; heat = mean_nets( (crop(h) - min) / (max - min) ), min/max over the whole cropped
 * [L,h,w] tensor of each net.  seg_ptrs/heat_ptrs: DEVICE arrays of nnets pointers to [C,Hp,Wp]/[L,Hp,Wp] NCHW
 * outputs (batch 1); the crop window starts at (oy, ox).
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
  const float* const* seg_ptrs; const float* const* heat_ptrs; /* heat_ptrs NULL when L == 0 */
  uint8_t* labels;        /* [h][w] */
  float* avg_seg;         /* [C][h][w] or NULL */
  float* heat_out;        /* [L][h][w] or NULL */
  float* minmax;          /* scratch of 2*nnets*65 floats (final [nnets][2] table + partials) */
  int32_t nnets, C, L, Hp, Wp, h, w, oy, ox;
  int32_t raw_heat;       /* 1: plain mean of the heat maps, no min-max normalisation (util.py:217-229) */
} dfl_ensemble_args;
int dfl_ensemble_reduce(const dfl_ensemble_args* a, dfl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Fused multi-tensor SGD step (torch.optim.SGD as configured at train.py:333-334):
 *   g = grad*grad_scale + wd*p ; buf = first ? g : mom*buf + g ; g = nesterov ? g + mom*buf : buf ; p -= lr*g
 * over a flat parameter arena (all tensors laid out back to back; n = total element count).
 * ------------------------------------------------------------------------------------------------------------ */
int dfl_sgd_step(float* p, const float* grad, float* momentum_buf, int64_t n, float lr, float momentum,
                 float weight_decay, float grad_scale, int32_t nesterov, int32_t first_step, dfl_stream_t stream);

/* The same update AND the bf16 weight re-layout of the next step in one pass over the weights (round 4; optimizer.step() followed
 * by the re-layout the next forward needs, train.py:333-334,424): the jobs of dfl_pack_weights_tiled, whose workgroups update
 * their 32 x 32 x C tile of the fp32 master (p, momentum buffer written back) before they emit its layouts from LDS, followed by
 * "plain" jobs (kind = DFL_PACK_PLAIN: src, A = element count, no layouts; DFL_SGD_PLAIN_TILE elements per workgroup) for what
 * has no tiled layout -- biases, BatchNorm parameters, the first layer, the heads.  Gradient and momentum buffer of an element
 * live at src + grad_delta and src + buf_delta (ELEMENTS; the three arenas share one layout; multiples of 4 for the tiled
 * jobs' 16-byte accesses).  No job may share elements with another one. */
#define DFL_PACK_PLAIN 100
#define DFL_SGD_PLAIN_TILE 4096
typedef struct {
  const dfl_pack_job* jobs_dev;
  int64_t grad_delta, buf_delta;
  int32_t njobs, total_tiles;
  float lr, momentum, weight_decay, grad_scale;
  int32_t nesterov, reserved;
} dfl_sgd_pack_args;
int dfl_sgd_pack_tiled(const dfl_sgd_pack_args* a, dfl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Fused multi-tensor Adam and RMSprop steps (torch.optim.Adam / torch.optim.RMSprop as configured by the reference's
 * train.py:331-352 --optim adam|rmsprop), over a flat arena like dfl_sgd_step; the arithmetic of torch's
 * _multi_tensor_adam (amsgrad, maximize off; coupled L2 weight decay) and _multi_tensor_rmsprop (centered off):
 *   Adam:    g = grad*grad_scale + wd*p ; m = lerp(m, g, 1-beta1) ; v = beta2*v + (1-beta2)*g*g ;
 *            p -= step_size * m / (sqrt(v)/bc2_sqrt + eps)
 *            with, for step count t (after its increment), step_size = lr/(1-beta1^t) and bc2_sqrt = sqrt(1-beta2^t),
 *            both computed by the caller in double and passed as floats (lr is then not read by the update).
 *   RMSprop: g = grad*grad_scale + wd*p ; v = alpha*v + (1-alpha)*g*g ; avg = sqrt(v) + eps ;
 *            momentum > 0:  buf = momentum*buf + g/avg ; p -= lr*buf        (momentum_buf required)
 *            momentum == 0: p -= lr*g/avg                                    (momentum_buf NULL)
 * beta1, beta2 and alpha are doubles: the factors 1 - beta and 1 - alpha are formed from them in double and then rounded to
 * fp32, as torch does with its Python-float hyper-parameters (1 - 0.999f is 1.3e-5 away from 1 - 0.999 in relative terms).
 * ------------------------------------------------------------------------------------------------------------ */
int dfl_adam_step(float* p, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, double beta1,
                  double beta2, float eps, float weight_decay, float step_size, float bc2_sqrt, float grad_scale,
                  dfl_stream_t stream);
int dfl_rmsprop_step(float* p, const float* grad, float* square_avg, float* momentum_buf, int64_t n, float lr, double alpha,
                     float eps, float weight_decay, float momentum, float grad_scale, dfl_stream_t stream);

/* Either update inside the tiled weight re-layout, as dfl_sgd_pack_tiled does for SGD: the same job list (tiled jobs of
 * dfl_pack_weights_tiled, then DFL_PACK_PLAIN jobs of DFL_SGD_PLAIN_TILE elements per workgroup).  The gradient and the two
 * state tensors of an element live at src + grad_delta, src + state1_delta, src + state2_delta (ELEMENTS, multiples of 4):
 * Adam: state1 = exp_avg, state2 = exp_avg_sq; RMSprop: state1 = square_avg, state2 = momentum buffer (not touched, and
 * state2_delta not read, when momentum == 0).  All parameters of the launch share one step count. */
#define DFL_OPTIM_ADAM 1
#define DFL_OPTIM_RMSPROP 2
typedef struct {
  const dfl_pack_job* jobs_dev;
  int64_t grad_delta, state1_delta, state2_delta;
  double beta1, beta2;          /* Adam */
  double alpha;                 /* RMSprop */
  int32_t njobs, total_tiles;
  int32_t kind;                 /* DFL_OPTIM_ADAM | DFL_OPTIM_RMSPROP */
  float lr, eps, weight_decay, grad_scale;
  float step_size, bc2_sqrt;    /* Adam */
  float momentum;               /* RMSprop */
} dfl_optim_pack_args;
int dfl_optim_pack_tiled(const dfl_optim_pack_args* a, dfl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * GPU-side input pipeline: the deterministic part of the reference loader (train_test_code/dataset.py) from raw
 * device arrays, for a whole batch in two launches.
 *   x[b]     = standardise(reflect_pad(proj[b], pad))    (dataset.py:287-293; mean / unbiased std of the PADDED image)
 *   masks[b] = one-hot(labels[b]) as float [C][H][W]     (dataset.py:448-452)
 *   heats[b] = L Gaussian maps exp(-((x-mx)^2+(y-my)^2)/(2 sigma^2)) / (2 pi sigma^2), zero for landmarks that are
 *              inf or outside [0,W-1]x[0,H-1]             (dataset.py:302-325, 421-429)
 * Any of x / masks / heats may be NULL (skipped).  lands is [B][2][L]: row 0 = column (x), row 1 = row (y).
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
  const float* proj;            /* [B][H][W] raw intensities */
  const unsigned char* labels;  /* [B][H][W] */
  const float* lands;           /* [B][2][L] */
  float* x;                     /* [B][1][H+2*pad][W+2*pad] */
  float* masks;                 /* [B][C][H][W] */
  float* heats;                 /* [B][L][H][W] */
  double* scratch;              /* dfl_prep_scratch_doubles(B) doubles (needed when x != NULL and standardize) */
  int32_t B, H, W, pad, C, L;
  float sigma;
  int32_t standardize;
} dfl_prep_args;
int64_t dfl_prep_scratch_doubles(int32_t B);
int dfl_prep_batch(const dfl_prep_args* a, dfl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Random augmentation of training items (the reference's RandomDataAugDataSet, train_test_code/dataset.py:107-283):
 * run dfl_prep_batch on the batch first, then this call overwrites the rows items[k].row of x / masks / heats /
 * lands_out with the augmented item.  Per item, in order: invert (p = max - p); noise (min/max normalised, + sigma *
 * N(0,1) with the normals from Philox4x32-10 keyed by noise_key and counted by the pixel index, Box-Muller in fp32,
 * mapped back); gamma (normalised, ^gamma, mapped back); the affine warp -- normalise, reflect-pad by ceil(H/2)+pad /
 * ceil(W/2)+pad, quantise to 8 bits by truncation, PIL's 8-bit bilinear Image.transform(AFFINE) with img_map (source =
 * img_map (x+0.5, y+0.5, 1) in the padded frame), / 255, centre crop to (H+2pad) x (W+2pad), map back; the labels
 * reflect-padded by ceil(H/2), ceil(W/2) and warped with seg_map by nearest (outside the frame: no label, all masks 0);
 * the landmarks mapped by land_map (pixel coordinates), inf kept, and dropped (inf) by land_rule; erase: n_box boxes
 * (row, col, rows, cols) in order, each + 0.2 (max - min of the box) * N(0,1) (key box_key[b], counter the pixel
 * index of the padded image); then x standardised with the mean and unbiased std of the padded image, one-hot masks,
 * and heat maps for every finite landmark.  Steps whose flag is clear are skipped (the affine warp always runs).
 * levels / noise (optional, NULL = skipped) receive the warped 8-bit levels [n_items][H+2pad][W+2pad] and the noise
 * normals [n_items][H][W] (rows of items without the noise flag are left as they are).
 * ------------------------------------------------------------------------------------------------------------ */
#define DFL_AUG_INVERT 1
#define DFL_AUG_NOISE 2
#define DFL_AUG_GAMMA 4
#define DFL_AUG_ERASE 8
#define DFL_AUG_LANDS_NONE 0        /* no landmark is dropped (the reference without segmentations) */
#define DFL_AUG_LANDS_REFERENCE 1   /* dataset.py:245-247 as written: x < 0 or x > H-1 or y < 0 or y < C-1 */
#define DFL_AUG_LANDS_IN_VIEW 2     /* the intended test: outside [0, W-1] x [0, H-1] */
typedef struct {
  double img_map[6];            /* projection: padded-frame source of an output pixel centre (PIL's inverse map) */
  double seg_map[6];            /* labels: the same in the labels' padded frame */
  double land_map[6];           /* landmarks: forward map in unpadded pixel coordinates */
  uint64_t noise_key;
  uint64_t box_key[5];
  int32_t box[5][4];            /* row, col, rows, cols in the (H+2pad) x (W+2pad) image */
  float noise_sigma, gamma;
  int32_t row;                  /* batch row this item overwrites */
  int32_t flags;                /* DFL_AUG_* */
  int32_t n_box;                /* 0..5 (more: the first 5); a box that does not fit the image or has a side <= 0
                                   ends the list: the boxes before it apply, it and those after it do not.  An item
                                   whose row is outside [0, B) is skipped: it writes no output, levels or noise */
  int32_t reserved;
} dfl_augment_item;
typedef struct {
  const float* proj;            /* [B][H][W] raw intensities (what dfl_prep_batch read) */
  const unsigned char* labels;  /* [B][H][W] or NULL */
  const float* lands;           /* [B][2][L] raw landmarks or NULL */
  float* x;                     /* [B][1][H+2*pad][W+2*pad] */
  float* masks;                 /* [B][C][H][W] or NULL */
  float* heats;                 /* [B][L][H][W] or NULL */
  float* lands_out;             /* [B][2][L] (a buffer other than lands) */
  const dfl_augment_item* items;  /* [n_items], device memory */
  void* scratch;                /* dfl_augment_scratch_bytes(n_items, H, W, pad) bytes, 256-byte aligned */
  unsigned char* levels;        /* optional, see above */
  float* noise;                 /* optional, see above */
  int32_t n_items, B, H, W, pad, C, L;
  float sigma;                  /* heat-map sigma */
  int32_t standardize, land_rule;
} dfl_augment_args;
int64_t dfl_augment_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t pad);
int dfl_augment_batch(const dfl_augment_args* a, dfl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Landmark extraction from predicted heat maps (est_lands_csv.py:96-124, the step after the network in the paper's
 * pipeline).  For image b and landmark l:  (row, col) = arg-max of heats[b][l] over the pixels whose segmentation
 * label equals label_for_land[l] (all pixels when segs / label_for_land is NULL or the entry is negative; ties -> lowest
 * flat index), kept only if ncc_2d(Gaussian 25x25 template (sigma), 25x25 window of the heat map reflect-padded by 12
 * around it) >= min_ncc (0.9 in the reference); otherwise (-1, -1).
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
  const float* heats;             /* [B][L][H][W] */
  const unsigned char* segs;      /* [B][H][W] labels or NULL */
  const int32_t* label_for_land;  /* [L] or NULL */
  int32_t* rowcol;                /* [B][L][2], 8-byte aligned: a map's slot is also where the workgroups of its arg-max pass meet (64-bit atomic max) before the answer is written there */
  float* ncc;                     /* [B][L] correlation at the arg-max (0 where none), or NULL */
  int32_t B, L, H, W;
  float sigma, min_ncc;
} dfl_est_lands_args;
int dfl_est_lands(const dfl_est_lands_args* a, dfl_stream_t stream);

/* Hard Dice of predicted label maps against ground truth (compute_actual_dice_on_test.py:63-93): for image b and
 * label l = 1..C-1 (background excluded)  dice[b][l-1] = 2*|est==l & gt==l| / (|est==l| + |gt==l|), 1.0 when the label
 * occurs in neither.  counts[b][l][3] = (|est==l|, |gt==l|, |both|) for l = 0..C-1 (exact integers). */
int dfl_hard_dice(const unsigned char* est, const unsigned char* gt, int64_t pixels_per_image, int32_t B, int32_t C,
                  int64_t* counts, double* dice, dfl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Clean-up of predicted label maps: connected components per value, selection, and a dilated bone mask.
 * (The reference has no counterpart: its tools take 'nn-segs' as the arg-max left it; the usual remedy is a round trip
 * through scipy.ndimage on the host.)  Label maps are segs [B][H][W] of unsigned char, as test_ensemble.py writes them.
 * The FLAT INDEX of a pixel is row * W + col within its image (int32): H * W < 2^31 is required and checked before
 * anything else, offsets across the batch are 64-bit.  Plain library calls, not dfl_exec ops.
 *
 * dfl_label_components: root[p] = the smallest flat index among the pixels connected to p through pixels of the same byte
 * value (connectivity 4 or 8; every value is a label, 0 included; nothing connects across images) -- canonical, so the
 * result depends on no tile size, schedule or arrival order.  area[p] = pixels of the component at its root pixel, 0
 * elsewhere.  info[p] at a root: bit 31 = the component touches the image border; bits 0..30 = the union of
 * 1 << min(v, 30) over the values v of the 4-neighbours of the component's pixels that lie outside the component; 0
 * elsewhere.  Three launches whatever the data (csrc/labels.hip): union-find per DFL_LABEL_TILE_H x DFL_LABEL_TILE_W tile
 * in LDS, unions across tile borders in global memory, then flattening with area and info; integer atomics only.
 *
 * dfl_label_select: one pass over (segs, root, area, info) of dfl_label_components, one of two jobs.
 *   remove (fill_below == 0): for the labels l = 1..num_classes-1 a component is kept when area >= min_area and, with
 *     keep == 1, when it is the largest component of its label in its image (ties: the smallest root); pixels of the other
 *     components become 0; value 0 and values >= num_classes are copied through.  (keep == 0 keeps every component.)
 *   fill (fill_below > 0): a component of value 0 that does not touch the border, has area <= fill_below and whose
 *     neighbour set (info) is exactly one label l with 1 <= l < min(num_classes, 30) becomes l (bit 30 of info stands for
 *     "30 or more" and is never filled from); everything else is copied through.
 * counts (or NULL) [B][num_classes][2] = (pixels removed of label l, pixels filled with label l) per image.  scratch:
 * dfl_label_select_scratch_bytes(B, num_classes) bytes, 8-byte aligned: per (image, label) the 64-bit slot where the
 * components of a label meet (atomic max of (area << 32) | ~root, as the arg-max of dfl_est_lands meets in rowcol).
 *
 * dfl_label_dilate: mask[p] = 1 when some pixel q of the same image with (drow)^2 + (dcol)^2 <= radius^2 has a value v < 32
 * with bit v of label_set set, else 0 (pixels outside the image do not count; radius 0..DFL_LABEL_MAX_RADIUS).
 *
 * Boundary distances (csrc/labels_dist.hip; restated in numpy by tests/surface_ref.py).
 * A LABEL SET is a 32-bit word as in dfl_label_dilate: value v < 32 is in the set when bit v is set, values >= 32 never.
 * The SITES of a set in an image: with boundary == 0 all pixels whose value is in the set; with boundary == 1 the in-set
 * pixels that have a 4-neighbour not in the set or lie on the image border (a neighbour outside the image is "not in the
 * set"): mask & ~binary_erosion(mask, 4-neighbourhood, border_value=0), the usual convention.
 *
 * dfl_label_edt: dist2[b][s][p] = the minimum of drow^2 + dcol^2 over the sites q of label_sets[s] in image b: the exact
 * squared Euclidean distance transform, int32.  DFL_LABEL_EDT_NONE everywhere in an image that has no site of that set;
 * nothing reaches across images.  (H-1)^2 + (W-1)^2 < 2^31 - 1 is required and checked before anything else.  label_sets
 * is HOST memory, [S], S = 1..DFL_LABEL_MAX_CLASSES.  rowdist is scratch of B * S * (H * W + 1) int32: per row the squared
 * horizontal distance to the nearest site of that row, then one "has a site" word per (image, set).  Three launches
 * whatever the data: the has-a-site words cleared, pass 1 along the rows (a wave per row, ballots; integer atomics
 * for the has-a-site words), pass 2 down the columns (min over r' of (r - r')^2 + rowdist[r'][c], a scan outwards from r
 * that ends once k^2 >= the best so far).
 *
 * Surface distances of label l = 1..num_classes-1 in image b: E = the boundary sites of {l} in est, G = those in gt;
 * direction 0 is the multiset { sqrt(dist2_gt[b][l-1][p]) : p in E }, direction 1 { sqrt(dist2_est[b][l-1][p]) : p in G },
 * where dist2_gt = dfl_label_edt(gt, sets {1}..{num_classes-1}, boundary 1) and dist2_est the same of est.
 *
 * dfl_label_surface_stats: n, max2 (int32) and sum (double), each [B][num_classes-1][2]: per direction the number of boundary
 * pixels, the largest squared distance and the sum of sqrt(squared distance) added in a fixed order (csrc/fixed_sum.h: one
 * record per workgroup, records in index order, no float atomics: two runs give the same bits).  Where either n of a
 * (b, l) is 0, max2 and sum of that (b, l) are 0.  The boundary test is recomputed from est / gt; no boundary map is stored.
 *
 * dfl_label_surface_select: kth2[b][l-1][j] = the squared distance of 0-based rank ranks[b][l-1][j] (device memory) in the
 * ascending union of both directions of (b, l); -1 for a rank < 0 or >= the size of the union.  Radix select on the int32
 * keys, four passes of 8 bits, each one scan of the maps: 256-bin histograms per (b, l, j) in LDS, added with integer
 * atomics, one prefix step between passes.  Integers only: the result cannot depend on arrival order.
 *
 * scratch of both: dfl_label_surface_scratch_bytes(B, H, W, num_classes) bytes, 8-byte aligned (the larger of the per-workgroup
 * records of the sums and the histograms with the state of the select).
 * ------------------------------------------------------------------------------------------------------------ */
#define DFL_LABEL_TILE_H 32
#define DFL_LABEL_TILE_W 64
#define DFL_LABEL_MAX_CLASSES 31
#define DFL_LABEL_MAX_RADIUS 32
int dfl_label_components(const unsigned char* segs, int32_t B, int32_t H, int32_t W, int32_t connectivity, int32_t* root,
                         int32_t* area, uint32_t* info, dfl_stream_t stream);
int dfl_label_select_scratch_bytes(int32_t B, int32_t num_classes);
int dfl_label_select(const unsigned char* segs, const int32_t* root, const int32_t* area, const uint32_t* info, int32_t B,
                     int32_t H, int32_t W, int32_t num_classes, int32_t keep, int32_t min_area, int32_t fill_below,
                     unsigned char* out, int32_t* counts, void* scratch, dfl_stream_t stream);
int dfl_label_dilate(const unsigned char* segs, int32_t B, int32_t H, int32_t W, uint32_t label_set, int32_t radius,
                     unsigned char* mask, dfl_stream_t stream);
#define DFL_LABEL_EDT_NONE 2147483647
int dfl_label_edt(const unsigned char* segs, int32_t B, int32_t H, int32_t W, const uint32_t* label_sets, int32_t S,
                  int32_t boundary, int32_t* rowdist, int32_t* dist2, dfl_stream_t stream);
int dfl_label_surface_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t num_classes);
int dfl_label_surface_stats(const unsigned char* est, const unsigned char* gt, int32_t B, int32_t H, int32_t W,
                            int32_t num_classes, const int32_t* dist2_gt, const int32_t* dist2_est, int32_t* n, int32_t* max2,
                            double* sum, void* scratch, dfl_stream_t stream);
int dfl_label_surface_select(const unsigned char* est, const unsigned char* gt, int32_t B, int32_t H, int32_t W,
                             int32_t num_classes, const int32_t* dist2_gt, const int32_t* dist2_est, const int32_t* ranks,
                             int32_t* kth2, void* scratch, dfl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Result overlays (overlay_est_ann.py, overlay_est_heat.py, examples_dataset/make_preproc_overlays.py of the reference):
 * uint8 RGB for a batch of B fp32 images, two launches.  Phase 1: per-image min / max of the image (and of the heat map).
 * Phase 2, per pixel, every fp32 operation rounded on its own (built with -ffp-contract=off):
 *   g = (uint8) trunc(((x - min) / (max - min)) * 255)          0 when max == min (the reference divides 0 by 0)
 *   v = g / 255 in three channels
 *   1 <= label <= n_tint:  v[c] = tint_scale * v[c] + tint_add[label-1][c]
 *   heat:  h = heat - hmin, / (hmax - hmin) only if that is > 1e-3;  v[c] = (1 - h) * v[c] + h * heat_color[c]
 *   out[c] = quant ROUND: (uint8) clamp(v * 255 + 0.5, 0, 255),  TRUNC: (uint8) clamp(v * 255, 0, 255)
 *   markers overwrite with yellow (255, 255, 0): filled ellipses of Pillow's ImageDraw.ellipse on the box
 *   (trunc(x - radius), trunc(y - radius), trunc(x + radius), trunc(y + radius)) -- the subtraction / addition in the
 *   centres' type -- drawn from a stamp table (per box (w, h), per row, the filled column span); crosses of +-cross
 *   pixels, both ends included.  Both clipped to the image.
 * grid != 0 writes image k as tile k of torchvision's make_grid(nrow=8, padding=2, pad_value=0) into one canvas
 * [(H+2)*rows+2][(W+2)*min(8,B)+2][3] (rows = ceil(B/8)), padding and empty tiles zeroed; with B == 1 the canvas is the
 * image.  Without grid, out is [B][H][W][3].
 * ------------------------------------------------------------------------------------------------------------ */
#define DFL_OVERLAY_ROUND 0
#define DFL_OVERLAY_TRUNC 1
#define DFL_OVERLAY_MAX_COLORS 8
#define DFL_OVERLAY_MAX_MARKERS 256       /* per image and kind */
#define DFL_OVERLAY_STAMP_DIM 64          /* stamp_index is [DIM][DIM]: box (w, h) at w * DIM + h */
#define DFL_OVERLAY_SCRATCH_FLOATS 256    /* scratch floats per image */
typedef struct {
  const float* image;             /* [B][H][ld_image] */
  const unsigned char* labels;    /* [B][H][ld_labels] or NULL */
  const float* heat;              /* [B][H][ld_heat] or NULL */
  const void* gt_lands;           /* [B][n_gt][2] (x = column, y = row), fp32 or fp64 (gt_f64); non-finite = none */
  const int32_t* est_lands;       /* [B][n_est][2] (column, row); negative = none */
  const int32_t* stamp_index;     /* [DIM * DIM]: first row of box (w, h) in stamp_spans, -1 = not in the table */
  const int32_t* stamp_spans;     /* per stamp row: lo | hi << 16 (lo > hi: empty row) */
  float* scratch;                 /* B * DFL_OVERLAY_SCRATCH_FLOATS floats */
  unsigned char* out;             /* see above */
  int32_t B, H, W, ld_image, ld_labels, ld_heat;
  int32_t n_tint;                 /* labels 1..n_tint are tinted (<= DFL_OVERLAY_MAX_COLORS) */
  float tint_scale;
  float tint_add[DFL_OVERLAY_MAX_COLORS][3];
  float heat_color[3];
  double radius;                  /* ellipse radius (rounded to fp32 for fp32 centres) */
  int32_t n_gt, gt_f64, n_est, cross;
  int32_t quant, grid;
} dfl_overlay_args;
int dfl_overlay_batch(const dfl_overlay_args* a, dfl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Full-resolution dataset overlays (examples_dataset/make_full_res_overlays.py of the reference) and Pillow's 8-bit
 * BILINEAR resample (Image.resize(size, Image.BILINEAR) of an RGB image, libImaging/Resample.c).
 *
 * Resample plan: per output column (row) the first input column (row) and the tap count, and kh (kv) coefficients in
 * 22-bit fixed point, computed as Pillow does (support 1 scaled by max(in / out, 1), weights normalised, then
 * rounded).  Every output pixel, per channel:  t = clip8(2^21 + sum_k in[row][x0 + k] * h_coefs[k])  for each input row
 * it needs, then  out = clip8(2^21 + sum_k t[y0 + k] * v_coefs[k]),  clip8(s) = clamp(s >> 22, 0, 255).  The kernels
 * work on output tiles of DFL_RESAMPLE_TILE_ROWS x DFL_RESAMPLE_TILE_COLS; span_rows / span_cols bound the input
 * rows / columns one tile reads (a tile whose tables ask for more writes nothing).
 * ------------------------------------------------------------------------------------------------------------ */
#define DFL_RESAMPLE_TILE_ROWS 8
#define DFL_RESAMPLE_TILE_COLS 64
#define DFL_RESAMPLE_MAX_LDS 49152        /* bytes: 4 * (4 * span_cols + DFL_RESAMPLE_TILE_COLS * span_rows) */
typedef struct {
  const int32_t* h_bounds;        /* [w_out][2]: first input column, taps */
  const int32_t* h_coefs;         /* [w_out][kh] */
  const int32_t* v_bounds;        /* [h_out][2]: first input row, taps */
  const int32_t* v_coefs;         /* [h_out][kv] */
  int32_t h_in, w_in, h_out, w_out, kh, kv;
  int32_t span_rows, span_cols;
} dfl_resample_plan;

/* uint8 RGB [B][h_in][w_in][3] -> [B][h_out][w_out][3], one launch. */
typedef struct {
  const unsigned char* in;
  unsigned char* out;
  dfl_resample_plan plan;
  int32_t B, reserved;
} dfl_resample_args;
int dfl_resample_bilinear_u8(const dfl_resample_args* a, dfl_stream_t stream);

/* Full-resolution overlays, reduced and tiled.  Image b (full resolution H x W) is drawn as the reference draws it:
 * rotated by 180 degrees when rot180[b] (source pixel (H-1-y, W-1-x)), grey level, tint of labels 1..n_tint and the
 * second 8-bit truncation exactly as dfl_overlay_batch's TRUNC path; then filled yellow ellipses from the ellipse stamp
 * table of dfl_overlay_args on the boxes[b][k] = (x0, y0, w, h, first stamp row) of image coordinates, k < n_boxes[b];
 * then up to DFL_FULLRES_MAX_TEXTS text masks texts[b][t] = (x, y, mask) (top-left in image coordinates, index into
 * text_stamps, -1 = none), in order, each blended with white ink as Pillow blends an L mask m onto RGB:
 * c = (t + (t >> 8)) >> 8 with t = c * (255 - m) + 255 * m + 128.  text_stamps[i] = (w, h, first byte in text_masks).
 * The full-resolution RGB image never leaves the chip: the resample of `plan` reduces it to h_out x w_out, written as
 * tile (tile0 + b) of torchvision's make_grid(nrow=8, padding=2) over n_tiles images into `out`, a canvas of
 * grid_shape(n_tiles, h_out, w_out) (n_tiles == 1: the image itself).  Padding pixels are not written.
 * Two launches: dfl_overlay_batch's per-image min / max partials into scratch, then the fused render + resample. */
#define DFL_FULLRES_MAX_BOXES 64          /* visible landmarks per image */
#define DFL_FULLRES_MAX_TEXTS 2
typedef struct {
  const float* image;             /* [B][H][W] */
  const unsigned char* labels;    /* [B][H][W] */
  const int32_t* rot180;          /* [B] */
  const int32_t* boxes;           /* [B][DFL_FULLRES_MAX_BOXES][5] */
  const int32_t* n_boxes;         /* [B] */
  const int32_t* texts;           /* [B][DFL_FULLRES_MAX_TEXTS][3] */
  const int32_t* stamp_spans;     /* ellipse stamp rows, as dfl_overlay_args */
  const int32_t* text_stamps;     /* [n_text_stamps][3] */
  const unsigned char* text_masks;
  float* scratch;                 /* B * DFL_OVERLAY_SCRATCH_FLOATS floats */
  unsigned char* out;
  dfl_resample_plan plan;         /* h_in == H, w_in == W */
  int32_t B, H, W, n_tint;
  float tint_scale;
  float tint_add[DFL_OVERLAY_MAX_COLORS][3];
  int32_t n_text_stamps, n_stamp_spans;
  int32_t tile0, n_tiles;
} dfl_fullres_args;
int dfl_fullres_overlay(const dfl_fullres_args* a, dfl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Bone surfaces of a label volume (examples_dataset/full_res_3d_viz.py of the reference: vtkDiscreteMarchingCubes,
 * vtkWindowedSincPolyDataFilter, vtkTransformPolyDataFilter), restated in DESIGN.md section 12.
 *
 * Discrete marching cubes: volume [nz][ny][nx] uint8, x fastest.  Cell c is the cube between grid points p and
 * p + (1,1,1), numbered c = x + (nx-1) * (y + (ny-1) * z); the case of a label sets bit i when corner
 * p + (i & 1, (i >> 1) & 1, (i >> 2) & 1) equals the label.  The case table (data/mc_cases.txt, tools/gen_mc_table.py)
 * lists triangles as edge triples: tri_off[case] .. tri_off[case + 1] - 1.  Edge e lies along axis a = e >> 2 with
 * the lower end offset by (e & 1, (e >> 1) & 1) along the two other axes in ascending order; its key is
 * 3 * (x + nx * (y + ny * z)) + a of that lower end.  Every triangle of label l (labels[l], l < n_labels) becomes
 * three int64 keys in `keys`, triangles of label 0 first, each label's in ascending cell order and table order within a
 * cell.  dfl_mesh_mc_count: per block of DFL_MESH_MC_CELLS cells the triangle counts, then one scan kernel writing
 * block_offsets (first triangle of each block and label) and totals[l] (first triangle of label l; totals[n_labels] =
 * the sum).  dfl_mesh_mc_emit (after the caller has sized `keys` from totals): the keys.  Cells < 2^31.
 * ------------------------------------------------------------------------------------------------------------ */
#define DFL_MESH_MAX_LABELS 4
#define DFL_MESH_MC_CELLS 4096            /* cells per workgroup of the two passes */
#define DFL_MESH_MAX_ITERS 64
typedef struct {
  const unsigned char* volume;
  const int32_t* tri_off;         /* [257] */
  const unsigned char* tri_edges; /* [tri_off[256]][3] */
  int32_t* block_counts;          /* [n_blocks][DFL_MESH_MAX_LABELS], n_blocks = ceil(cells / DFL_MESH_MC_CELLS) */
  int64_t* block_offsets;         /* [n_blocks][DFL_MESH_MAX_LABELS] */
  int64_t* totals;                /* [DFL_MESH_MAX_LABELS + 1] */
  int64_t* keys;                  /* [totals[n_labels]][3] (emit only) */
  int32_t nx, ny, nz, n_labels;
  int32_t labels[DFL_MESH_MAX_LABELS];
} dfl_mesh_mc_args;
int dfl_mesh_mc_count(const dfl_mesh_mc_args* a, dfl_stream_t stream);
int dfl_mesh_mc_emit(const dfl_mesh_mc_args* a, dfl_stream_t stream);

/* Vertex position of each edge key: the midpoint of the grid edge, (x, y, z) + 0.5 along its axis, fp32 [V][3]. */
typedef struct {
  const int64_t* keys;
  float* pos;
  int64_t V;
  int32_t nx, ny;
} dfl_mesh_decode_args;
int dfl_mesh_decode(const dfl_mesh_decode_args* a, dfl_stream_t stream);

/* Topology keys of a triangle list tris [T][3] (vertex ids < V): edge_keys[6t + ...] = i * V + j for the directed
 * pairs (a,b) (b,a) (b,c) (c,b) (c,a) (a,c) of triangle t = (a,b,c), and vt_keys[3t + k] = tris[t][k] * 3T + 3t + k.
 * Either output may be NULL.  Sorted (and, for edge_keys, made unique with counts), they give the CSR lists below. */
typedef struct {
  const int32_t* tris;
  int64_t* edge_keys;
  int64_t* vt_keys;
  int64_t T, V;
} dfl_mesh_topo_args;
int dfl_mesh_topology(const dfl_mesh_topo_args* a, dfl_stream_t stream);

/* CSR of sorted, distinct keys: row = key / div, col[k] = (key % div) / col_div, row_ptr [n_rows + 1].  With counts
 * (the number of times each key occurred), fixed[row] = 1 when some count is 1 (an edge of exactly one triangle), else
 * 0; fixed may be NULL without counts.  nnz >= 1. */
typedef struct {
  const int64_t* keys;
  const int64_t* counts;
  int32_t* col;
  int32_t* row_ptr;
  unsigned char* fixed;
  int64_t nnz, div, col_div;
  int64_t n_rows;
} dfl_mesh_csr_args;
int dfl_mesh_csr(const dfl_mesh_csr_args* a, dfl_stream_t stream);

/* Windowed-sinc smoothing: out = sum_{n <= iterations} coef[n] T_n with T_0 = x, T_1 = W x, T_{n+1} = 2 W T_n - T_{n-1};
 * (W y)_i = the mean of y over the neighbours col[row_ptr[i] .. row_ptr[i+1]-1] in that order, or y_i when fixed[i].
 * A vertex without neighbours (row_ptr[i] == row_ptr[i+1]: no triangle uses it) is treated as fixed.  Fixed vertices
 * are copied from x bit for bit.  One gather launch per n, fp32; t_a, t_b, acc are [V][4] scratch (unused when
 * iterations == 1).  x, out [V][3]. */
typedef struct {
  const float* x;
  const int32_t* row_ptr;
  const int32_t* col;
  const unsigned char* fixed;
  float* t_a;
  float* t_b;
  float* acc;
  float* out;
  int64_t V;
  int32_t iterations, reserved;
  float coef[DFL_MESH_MAX_ITERS + 1];
} dfl_mesh_smooth_args;
int dfl_mesh_smooth(const dfl_mesh_smooth_args* a, dfl_stream_t stream);

/* out[v] = fp32(M[0:3, 0:3] x[v] + M[0:3, 3]), evaluated in fp64 (M row-major, affine).  In place is allowed. */
typedef struct {
  const float* x;
  float* out;
  int64_t V;
  double M[16];
} dfl_mesh_xform_args;
int dfl_mesh_transform(const dfl_mesh_xform_args* a, dfl_stream_t stream);

/* Area-weighted vertex normals: n[v] = unit(sum over the triangles t of v, in vt_tri order, of (b - a) x (c - a)),
 * fp64 inside, 0 when the sum is 0.  vt_ptr [V + 1], vt_tri [3T] from dfl_mesh_csr over vt_keys. */
typedef struct {
  const float* pos;
  const int32_t* tris;
  const int32_t* vt_ptr;
  const int32_t* vt_tri;
  float* normals;
  int64_t V;
} dfl_mesh_normals_args;
int dfl_mesh_normals(const dfl_mesh_normals_args* a, dfl_stream_t stream);

/* Quadric-error decimation, one round (csrc/decimate.hip, built with -ffp-contract=off: all
 * arithmetic is fp64 on the fp32 positions, every product and sum rounded on its own, tests/decimate_ref.py restates it).
 * The caller (dfl_amd.mesh.decimate) rebuilds, every round, the neighbour CSR (row_ptr, col) and the vertex-triangle CSR
 * (vt_ptr, vt_tri) with dfl_mesh_topology and dfl_mesh_csr, and beside them: use[k] = the number of triangles on the
 * edge (row, col[k]); the undirected edges e = 0 .. E - 1 in ascending (u, v) order, u = edge_u[e] < v = edge_v[e]; and
 * eid[k] = the undirected edge of entry k.  Counts below 2^31; V, T, E >= 1.  No atomics: one writer per element.
 *
 * dfl_mesh_quadrics: Q[v] = the sum over the triangles of v, in vt_tri order, of K_t = plane plane^T / l as the 10
 * entries (aa ab ac ad bb bc bd cc cd dd), plane = (n, -n . p0), n = (p1 - p0) x (p2 - p0), l = sqrt(n . n); K_t = 0
 * when l == 0. */
typedef struct {
  const float* pos;               /* [V][3] */
  const int32_t* tris;            /* [T][3] */
  const int32_t* vt_ptr;          /* [V + 1] */
  const int32_t* vt_tri;          /* [3T] */
  double* Q;                      /* [V][10] */
  int64_t V, T;
} dfl_mesh_quadrics_args;
int dfl_mesh_quadrics(const dfl_mesh_quadrics_args* a, dfl_stream_t stream);

/* One thread per undirected edge: key[e] = (bits(fp32(cost)) << 32) | e for a candidate, all ones otherwise, and
 * cand[e] = the position the collapse would give u (zeros for a non-candidate).  Candidate: use 2, no edge of use != 2
 * at u or v, exactly two common neighbours, both of degree >= 5, deg(u) + deg(v) - 4 >= 3, and no triangle at u or v
 * (without both) whose normal turns: n0 . n1 > 0 and (n0 . n1)^2 >= 0.04 (n0 . n0)(n1 . n1).  Position: -A^-1 b of
 * q = Q[u] + Q[v] by cofactors when det A > 1e-3 (trace A / 3)^3 and it lies within twice the edge length of the
 * midpoint, else the cheapest of midpoint, p_u, p_v; rounded to fp32 before the cost and the flip test. */
typedef struct {
  const float* pos;
  const int32_t* tris;
  const int32_t* row_ptr;         /* [V + 1] */
  const int32_t* col;             /* [2E] */
  const int32_t* use;             /* [2E], aligned with col */
  const int32_t* vt_ptr;
  const int32_t* vt_tri;
  const double* Q;
  const int32_t* edge_u;          /* [E] */
  const int32_t* edge_v;          /* [E] */
  uint64_t* key;                  /* [E] */
  float* cand;                    /* [E][3] */
  int64_t V, T, E;
} dfl_mesh_collapse_keys_args;
int dfl_mesh_collapse_keys(const dfl_mesh_collapse_keys_args* a, dfl_stream_t stream);

/* Three gather launches: m1[v] = min of key over the edges at v; m2[v] = min of m1 over v and its neighbours;
 * sel[e] = 1 when e is a candidate and m2[u] == m2[v] == key[e], else 0. */
typedef struct {
  const int32_t* row_ptr;
  const int32_t* col;
  const int32_t* eid;             /* [2E], aligned with col */
  const int32_t* edge_u;
  const int32_t* edge_v;
  const uint64_t* key;
  uint64_t* m1;                   /* [V] */
  uint64_t* m2;                   /* [V] */
  unsigned char* sel;             /* [E] */
  int64_t V, E;
} dfl_mesh_collapse_select_args;
int dfl_mesh_collapse_select(const dfl_mesh_collapse_select_args* a, dfl_stream_t stream);

/* The collapses take[e] != 0 (vertex-disjoint): remap[v] = the lower end of the taken edge whose upper end v is, else
 * v; pos_out = pos with the lower end of every taken edge at cand[e]; tris_out = remap of tris; degen[t] = 1 when two
 * corners of tris_out[t] are equal. */
typedef struct {
  const float* pos;
  const int32_t* tris;
  const int32_t* row_ptr;
  const int32_t* col;
  const int32_t* eid;
  const unsigned char* take;      /* [E] */
  const float* cand;
  int32_t* remap;                 /* [V] */
  float* pos_out;                 /* [V][3] */
  int32_t* tris_out;              /* [T][3] */
  unsigned char* degen;           /* [T] */
  int64_t V, T, E;
} dfl_mesh_collapse_apply_args;
int dfl_mesh_collapse_apply(const dfl_mesh_collapse_apply_args* a, dfl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Rasteriser: the scene of full_res_3d_viz.py (the surfaces above, spheres, ray ribbons, the textured detector) drawn
 * into an 8-bit RGB image through a visibility buffer, restated in DESIGN.md section 22.  Triangles only.
 *
 * A scene is n_mesh records.  The caller passes them twice: `meshes` on the host (read for the checks below and the
 * launch sizes, never by a kernel) and `meshes_dev`, a device copy of the same bytes (read by the kernels).  pos, nrm,
 * uv, tris and tex are device pointers in both.  Records that share buffers under another matrix are instances.
 * Primitive id of triangle t of a record = first_prim + t (uint32); the ranges of the records ascend without overlap
 * and end below 0xffffffff, the background.  A triangle with a vertex index outside [0, n_verts) counts as degenerate.
 *
 * Built with -ffp-contract=off: every product and sum below is rounded on its own, divisions and square roots are
 * correctly rounded (tests/raster_ref.py restates them in numpy float32).
 *
 * Vertex stage, per corner (x, y, z), m = mvp:  clip_k = ((m[4k] x + m[4k+1] y) + m[4k+2] z) + m[4k+3];  w = clip_3;
 *   px = (clip_0 / w + 1) (0.5 Ws),  py = (1 - clip_1 / w) (0.5 Hs),  Ws = ssaa W, Hs = ssaa H (y down, sample centres
 *   at integer + 1/2);  X = rintf(256 px), Y = rintf(256 py);  zd = clip_2 / w.
 * A triangle is dropped whole when a corner has a non-finite clip value or w < znear (counts[1]; there is no near-plane
 * clipping), else when a corner has |X| or |Y| > 2^22 (counts[2]), else when its area is 0 (counts[3]); else it is
 * drawn (counts[0]), also where it then covers no sample.
 * Coverage: with s the sign of the area A = (X1-X0)(Y2-Y0) - (Y1-Y0)(X2-X0) (int64), edge k runs from corner k+1 to
 *   corner k+2 (mod 3), d = s (b - a), E_k = d.x (Py - a.y) - d.y (Px - a.x) at P = (256 i + 128, 256 j + 128).  Sample
 *   (i, j) is covered when every E_k > 0, or E_k = 0 on an edge with d.y < 0 or (d.y = 0 and d.x > 0) (top-left).
 * Depth: l_k = (float)E_k / (float)|A|;  depth = (l_0 zd_0 + l_1 zd_1) + l_2 zd_2 (-0 counts as +0); the sample counts
 *   only when 0 <= depth <= 1.  vis[j][i] = min over the triangles of (bits(depth) << 32) | prim, by the 64-bit unsigned
 *   integer atomic minimum (order-independent: every run gives the same bytes; equal depths go to the lower id).
 * Triangles whose clamped bounding box is at most DFL_RASTER_SMALL_BOX samples wide and high are walked by the thread
 *   that set them up; the others go to a list of DFL_RASTER_MAX_LARGE entries and are covered by workgroups in
 *   DFL_RASTER_TILE x DFL_RASTER_TILE tiles (when the list is full, by their thread).  Both ways give the same keys.
 * Shade, per sample: b_k = l_k / w_k, then b_k / ((b_0 + b_1) + b_2).  q = (b_0 q_0 + b_1 q_1) + b_2 q_2 for the
 *   normal components and u, v.  base = rgb, for a textured record rgb * ((float)tex[ty][tx] / 255) with
 *   tx = clamp((int)floorf(u tw), 0, tw - 1), ty from v and th.  Unless unlit: r = nmat n (rows as clip_k above, three
 *   terms), len = sqrtf((r_x r_x + r_y r_y) + r_z r_z), intensity = ambient + diffuse * (len > 0 ? |r_z| / len : 0),
 *   colour = base * intensity.  byte = rintf(255 * min(max(colour, 0), 1)).  Background samples take `background`.
 * Resolve: rgb[y][x][c] = (sum of the ssaa x ssaa sample bytes + ssaa^2 / 2) / ssaa^2 in integers.
 *
 * ids (optional) int32 [Hs][Ws]: the primitive id, -1 for background.  depth (optional) float [Hs][Ws]: +infinity for
 * background.  counts (optional) int32 [4].  scratch: dfl_raster_scratch_bytes(W, H, ssaa, n_mesh) bytes, 8-aligned
 * (negative: bad sizes or more than 2^31 - 1 bytes).  ssaa 1..DFL_RASTER_MAX_SSAA, Ws, Hs <= DFL_RASTER_MAX_DIM,
 * 0 <= n_mesh <= DFL_RASTER_MAX_MESHES, fewer than 2^31 triangles in all.  An empty scene gives the background.
 * Refused with nothing launched: NULL args, meshes (n_mesh > 0), scratch, rgb, pos or tris; bad sizes; a short
 * scratch; znear <= 0; nrm NULL without DFL_RASTER_UNLIT; DFL_RASTER_TEXTURED without uv, tex, tw > 0 and th > 0.
 * Launches: clear, triangles, large triangles (skipped when the scene is empty), shade, resolve.
 * ------------------------------------------------------------------------------------------------------------ */
#define DFL_RASTER_UNLIT 1
#define DFL_RASTER_TEXTURED 2
#define DFL_RASTER_SMALL_BOX 16           /* samples: the widest / highest box a single thread walks */
#define DFL_RASTER_TILE 64
#define DFL_RASTER_MAX_LARGE 65536
#define DFL_RASTER_MAX_SSAA 4
#define DFL_RASTER_MAX_DIM 16384
#define DFL_RASTER_MAX_MESHES 4096
typedef struct {
  const float* pos;               /* [n_verts][3] */
  const float* nrm;               /* [n_verts][3] or NULL (unlit only) */
  const float* uv;                /* [n_verts][2] or NULL */
  const int32_t* tris;            /* [n_tris][3] */
  const unsigned char* tex;       /* [th][tw] grey or NULL */
  int32_t n_verts, n_tris, tw, th;
  uint32_t first_prim, flags;
  float mvp[16];                  /* row-major, object to clip */
  float nmat[9];                  /* row-major, object normal to eye */
  float rgb[3];
} dfl_raster_mesh;
typedef struct {
  const dfl_raster_mesh* meshes;      /* host [n_mesh] */
  const dfl_raster_mesh* meshes_dev;  /* device [n_mesh], the same bytes */
  void* scratch;
  unsigned char* rgb;                 /* [H][W][3] */
  int32_t* ids;
  float* depth;
  int32_t* counts;
  int32_t n_mesh, W, H, ssaa, scratch_bytes;
  float znear, ambient, diffuse;
  float background[3];
} dfl_raster_args;
int dfl_raster_scratch_bytes(int32_t W, int32_t H, int32_t ssaa, int32_t n_mesh);
int dfl_raster_draw(const dfl_raster_args* a, dfl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Training files from the full-resolution dataset (the reference's README: crop 50 pixels from each border,
 * log-transform, rotate by 180 degrees where 'rot-180-for-up' is set, downsample), restated in DESIGN.md section 14.
 *
 * The crop window is rows crop .. R-crop-1 and the columns likewise, Rc x Cc = (R - 2 crop) x (C - 2 crop); with the
 * flag of image n set, cropped pixel (r, c) moves to (Rc-1-r, Cc-1-c).  Output pixel (i, j) of Ro x Co =
 * ceil(Rc / factor) x ceil(Cc / factor) covers rows i*factor .. min((i+1)*factor, Rc)-1 of that (rotated) crop and
 * the columns likewise: boxes of the bottom and right edges are clipped.  factor is 1..DFL_PREPROC_MAX_FACTOR.
 *
 * dfl_preproc_projs: out = the box mean of log(I0) - log(max(I, min_intensity)) with I0 the largest
 * max(I, min_intensity) of that image's crop window (log != 0; min_intensity > 0), or the box mean of I (log == 0).
 * Logarithms are fp32, box sums fp64.  Two launches: the reduction, which also takes the maximum (scratch), and one
 * over the outputs that adds log(I0).
 * dfl_preproc_segs: out = the most frequent label of the box, of equally frequent ones the smallest.  Labels are
 * 0..15; *status is set to 1 when a larger one was met (the outputs are then undefined), else 0.
 * dfl_restore_labels: the inverse for labels.  Pixel (r, c) of the crop window takes the label of the box that
 * contains it (rotation undone); the border of `crop` pixels is 0.
 * ------------------------------------------------------------------------------------------------------------ */
#define DFL_PREPROC_MAX_FACTOR 16
typedef struct {
  const void* pixels;             /* [N][R][C] fp32, or uint16 when u16 */
  const int32_t* rot180;          /* [N] */
  float* out;                     /* [N][Ro][Co] */
  uint32_t* scratch;              /* [N] words (log only) */
  int32_t N, R, C, crop, factor;
  int32_t u16, log;
  float min_intensity;
} dfl_preproc_projs_args;
int dfl_preproc_projs(const dfl_preproc_projs_args* a, dfl_stream_t stream);

typedef struct {
  const unsigned char* segs;      /* [N][R][C] */
  const int32_t* rot180;          /* [N] */
  unsigned char* out;             /* [N][Ro][Co] */
  int32_t* status;                /* one word */
  int32_t N, R, C, crop, factor, reserved;
} dfl_preproc_segs_args;
int dfl_preproc_segs(const dfl_preproc_segs_args* a, dfl_stream_t stream);

typedef struct {
  const unsigned char* labels;    /* [N][Ro][Co] */
  const int32_t* rot180;          /* [N] */
  unsigned char* out;             /* [N][R][C] */
  int32_t N, R, C, crop, factor, reserved;
} dfl_restore_labels_args;
int dfl_restore_labels(const dfl_restore_labels_args* a, dfl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Digitally reconstructed radiographs and 2D labels from the CT (csrc/drr.hip; DESIGN.md section 15 states the
 * semantics, tests/drr_ref.py restates them in numpy float64).
 *
 * mu [nz][ny][nx] is the attenuation per mm and labels the 3D annotation (0..15), both in volume index order.  Voxel i
 * occupies [i - 1/2, i + 1/2] on each index axis.  An object is a rigid pose and a label mask: the ray of output pixel
 * (c, r) is o + t d, t >= 0, in that object's index coordinates, with d = M [c, r, 1]; it is clipped to the voxel box
 * box_lo .. box_hi (inclusive voxel indices: [box_lo - 1/2, box_hi + 1/2]); a voxel counts when bit `label` of mask is
 * set.  One unit of t is s = |qscale [c, r, 1]| mm.  A direction component that is exactly 0 has no crossings on its
 * axis and the ray counts only if o lies in [box_lo - 1/2, box_hi + 1/2) there.
 *
 * interp DFL_DRR_EXACT: the radiological path.  att = sum over objects and admitted voxels of (length in the voxel) mu;
 * plen[l] = the summed length in admitted voxels of label l; label_map = the lowest l >= 1 with the largest plen[l], or
 * 0 when that length is below min_len_mm.
 * interp DFL_DRR_TRILINEAR (att only): per object N = max(1, ceil(s (t1 - t0) / step_mm)) samples at
 * t0 + (k + 1/2)(t1 - t0) / N of the trilinear interpolation of the masked volume (a corner voxel gives mu when its
 * label is admitted, else 0; corner indices are clamped to the volume); att += s (t1 - t0) / N * their sum.
 *
 * One thread per ray and view, every object inside the thread; one launch.  Rays that miss every box write 0.
 * mapping 0: a wave covers 8 x 8 pixels and a workgroup 16 x 16; 1: a wave covers 64 x 1 (tools/bench_drr.py compares).
 * ------------------------------------------------------------------------------------------------------------ */
#define DFL_DRR_EXACT 0
#define DFL_DRR_TRILINEAR 1
#define DFL_DRR_MAX_LABELS 16
typedef struct {
  float o[3];                     /* ray origin in index coordinates (x, y, z) */
  float M[9];                     /* row-major: d = M [c, r, 1] */
  int32_t box_lo[3], box_hi[3];   /* inclusive voxel box (x, y, z); box_hi < box_lo: the object is empty */
  uint32_t mask;                  /* bit l: voxels labelled l belong to the object */
} dfl_drr_object;

typedef struct {
  const float* mu;                /* [nz][ny][nx] */
  const unsigned char* labels;    /* [nz][ny][nx] */
  const dfl_drr_object* objects;  /* device, [views][n_obj] */
  float* att;                     /* [views][H][W] */
  float* plen;                    /* [views][n_labels][H][W], or NULL (exact only) */
  unsigned char* label_map;       /* [views][H][W], or NULL (exact only) */
  float qscale[9];                /* row-major */
  int32_t nx, ny, nz, H, W, views, n_obj, n_labels;
  int32_t interp, mapping;
  float step_mm, min_len_mm;
  int32_t reserved;
} dfl_drr_args;
int dfl_drr_render(const dfl_drr_args* a, dfl_stream_t stream);

/* The pose gradient of the trilinear DRR with its sampling frozen (csrc/drr_grad.hip; DESIGN.md section 19 states the
 * semantics, tests/grad_ref.py restates them in numpy).
 *
 * Take the samples x_k = o + t_k d of DFL_DRR_TRILINEAR exactly as dfl_drr_render places them for the same records,
 * qscale and step_mm (the same clip, N and t_k, the same clamped corners and masked corner values) and the ray weight
 * w = s (t1 - t0) / N.  grad f(x_k) is the gradient of the trilinear interpolant in the cell of that sample: per axis the
 * bilinear blend of the four corner differences along it; corners that were clamped together give 0.  For an
 * infinitesimal motion of object n in index coordinates, x -> x + eps (L (x - pivot_n) + tau),
 *   d (sum_rays d_att att) / d eps = <Mom, L> + F . tau,
 *   F[a]      = sum_rays d_att[v][r][c] w sum_k grad f_a(x_k),
 *   Mom[a][b] = sum_rays d_att[v][r][c] w sum_k grad f_a(x_k) (x_k - pivot_n)_b,
 * and grad[v][n] = F[0..2], then Mom row-major.  The moments are taken about the pivot inside the kernel: the raw
 * derivatives with respect to (o, M) carry t of about the source distance and cancel in the chain rule.
 * What the frozen sampling leaves out is the dependence of N, t0 and t1 on the pose.
 *
 * One thread per ray and view (8 x 8 pixels per wave), twelve float32 sums per ray and object, float64 across rays: wave
 * shuffles, LDS across the four waves, one record of twelve doubles per workgroup and object, added in index order by a
 * second kernel.  No atomics: a view's numbers have the same bits whatever else is in the batch.  Empty objects and rays
 * that miss give zeros.  scratch holds at least dfl_drr_pose_grad_scratch_doubles(views, n_obj, H, W) doubles
 * (negative: bad sizes, or more than 2^31 - 1).  Refused with nothing launched: NULL pointers, sizes that dfl_drr_render
 * refuses, interp other than DFL_DRR_TRILINEAR, a step_mm that is not positive, a short scratch.
 * The fields are those of dfl_drr_args that the trilinear renderer reads. */
typedef struct {
  const float* mu;                /* [nz][ny][nx] */
  const unsigned char* labels;    /* [nz][ny][nx] */
  const dfl_drr_object* objects;  /* device, [views][n_obj] */
  const float* d_att;             /* [views][H][W] */
  const float* pivots;            /* [views][n_obj][3], index coordinates (x, y, z) */
  double* grad;                   /* [views][n_obj][12] */
  double* scratch;
  int64_t scratch_doubles;        /* what scratch holds */
  float qscale[9];                /* row-major */
  int32_t nx, ny, nz, H, W, views, n_obj;
  int32_t interp;                 /* DFL_DRR_TRILINEAR */
  float step_mm;
} dfl_drr_pose_grad_args;
int dfl_drr_pose_grad(const dfl_drr_pose_grad_args* a, dfl_stream_t stream);
int dfl_drr_pose_grad_scratch_doubles(int32_t views, int32_t n_obj, int32_t H, int32_t W);

/* ------------------------------------------------------------------------------------------------------------
 * Gradient-NCC between V rendered views and one fixed image (csrc/sim.hip; DESIGN.md section 16 states the semantics,
 * tests/reg_ref.py restates them in numpy float64): the similarity of dfl_amd.register.
 *
 * Sobel gradients on the interior pixels 1 <= r <= H - 2, 1 <= c <= W - 2:
 *   gx = (p[r-1][c+1] + 2 p[r][c+1] + p[r+1][c+1]) - (p[r-1][c-1] + 2 p[r][c-1] + p[r+1][c-1]), gy likewise along rows.
 * An interior pixel counts when mask is NULL, else when the nine mask bytes of its 3 x 3 neighbourhood are non-zero.
 * Over the counted pixels ncc(a, b) = sum (a - mean a)(b - mean b) / sqrt(sum (a - mean a)^2 sum (b - mean b)^2), 0 when
 * either variance is 0 (at most 2^-40 of the sum of squares) or nothing is counted;
 *   cost[v] = 1 - (ncc(gx_v, gx_f) + ncc(gy_v, gy_f)) / 2.
 *
 * dfl_sim_prepare, once per fixed image: fx, fy [H][W] (0 on the border), counted [H][W] (1 / 0) and
 * totals[DFL_SIM_TOTALS] = n, sum fx, sum fx^2, sum fy, sum fy^2 over the counted pixels.
 * dfl_sim_gradncc, once per batch: one pass over moving [V][H][W]; per workgroup (a band of rows of one view) one record
 * of six float64 sums in scratch, added in index order by a second kernel.  No atomics: a view's cost has the same bits
 * whatever else is in the batch.  scratch holds at least dfl_sim_scratch_doubles(V, H, W) doubles (negative: bad sizes).
 * Refused with nothing launched: NULL pointers (mask may be NULL), H < 3, W < 3, V < 1, V > 65535, a short scratch.
 * ------------------------------------------------------------------------------------------------------------ */
#define DFL_SIM_TOTALS 5
typedef struct {
  const float* fixed;             /* [H][W] */
  const unsigned char* mask;      /* [H][W], or NULL */
  float* fx;                      /* [H][W] */
  float* fy;                      /* [H][W] */
  unsigned char* counted;         /* [H][W] */
  double* totals;                 /* [DFL_SIM_TOTALS] */
  int32_t H, W;
} dfl_sim_prepare_args;
int dfl_sim_prepare(const dfl_sim_prepare_args* a, dfl_stream_t stream);

typedef struct {
  const float* moving;            /* [V][H][W] */
  const float* fx;                /* the four outputs of dfl_sim_prepare for the same H, W */
  const float* fy;
  const unsigned char* counted;
  const double* totals;
  double* scratch;                /* [V][bands][6] */
  double* cost;                   /* [V] */
  int64_t scratch_doubles;        /* what scratch holds */
  int32_t V, H, W, reserved;
} dfl_sim_gradncc_args;
int dfl_sim_gradncc(const dfl_sim_gradncc_args* a, dfl_stream_t stream);
int64_t dfl_sim_scratch_doubles(int32_t V, int32_t H, int32_t W);

/* The adjoint of that cost (csrc/sim.hip; DESIGN.md section 19, tests/grad_ref.py): cost[V] with the bits dfl_sim_gradncc
 * gives for the same inputs (it is computed by the same two kernels), and d_moving[v][r][c] = d cost[v] / d moving[v][r][c]
 * for every pixel, the border included.
 *
 * For one direction let a be the moving and b the fixed Sobel values over the counted pixels, S_aa = sum (a - mean a)^2,
 * S_bb = sum (b - mean b)^2, S_ab = sum (a - mean a)(b - mean b).  At a counted pixel p
 *   d ncc / d a_p = (b_p - mean b) / sqrt(S_aa S_bb) - S_ab (a_p - mean a) / (S_aa^(3/2) S_bb^(1/2)),
 * and 0 at every p when the forward rule makes that ncc 0 (either variance 0, or nothing counted).  g_x = -1/2 d ncc_x / d a,
 * g_y likewise; d_moving = Sobel^T (g_x, g_y): a pixel gathers, from the counted interior pixels whose 3 x 3 window holds it,
 * g_x and g_y with the Sobel weight the pixel has in that window.
 *
 * The six sums per view are those of dfl_sim_gradncc (float64 band records added in index order); the four coefficients
 * per direction (the two factors and the two means) are computed in float64 and used per pixel in float32.  A workgroup
 * stages a 16 x 16 tile of moving with a halo of 2 in LDS.  No atomics: a view's outputs have the same bits whatever else
 * is in the batch.  scratch holds at least dfl_sim_gradncc_bwd_scratch_doubles(V, H, W) doubles (the forward's records and
 * 4 V more; negative: bad sizes, or more than 2^31 - 1).  Refused with nothing launched: what dfl_sim_gradncc refuses, and
 * a NULL d_moving. */
typedef struct {
  const float* moving;            /* [V][H][W] */
  const float* fx;                /* the four outputs of dfl_sim_prepare for the same H, W */
  const float* fy;
  const unsigned char* counted;
  const double* totals;
  double* scratch;
  double* cost;                   /* [V] */
  float* d_moving;                /* [V][H][W] */
  int64_t scratch_doubles;        /* what scratch holds */
  int32_t V, H, W, reserved;
} dfl_sim_gradncc_bwd_args;
int dfl_sim_gradncc_bwd(const dfl_sim_gradncc_bwd_args* a, dfl_stream_t stream);
int dfl_sim_gradncc_bwd_scratch_doubles(int32_t V, int32_t H, int32_t W);

/* ------------------------------------------------------------------------------------------------------------
 * Patch-wise gradient-NCC (csrc/sim_patch.hip; DESIGN.md section 18 states the semantics, tests/patch_ref.py restates
 * them in numpy float64).  Gradients, counted pixels and the "variance is 0" rule are those of dfl_sim_prepare above.
 *
 * Interior coordinates i = r - 1 in [0, H - 2), j = c - 1 in [0, W - 2); radius rho >= 1, side S = 2 rho + 1, stride
 * s >= 1.  Patch (a, b) covers i in [a s, a s + S), j in [b s, b s + S); a = 0 .. PR - 1, PR = (H - 2 - S) / s + 1 (integer
 * division), b = 0 .. PC - 1 likewise: patches lie wholly inside the interior, and trailing rows and columns that no
 * patch reaches are not used.  A patch lives when it holds at least min_count counted pixels; it counts in x when it
 * lives and the variance of the fixed gx over its counted pixels is not 0, in y likewise.  Per patch and direction ncc
 * is the ncc above over the patch's counted pixels (0 when the moving variance is 0);
 *   cost[v] = 1 - (X + Y) / 2,  X = the mean of ncc_x over the patches that count in x (0 when none does), Y likewise.
 *
 * dfl_sim_patch_prepare, once per fixed image, from the planes dfl_sim_prepare wrote: ptotals[P][DFL_SIM_TOTALS] =
 * n, sum fx, sum fx^2, sum fy, sum fy^2 per patch, P = PR PC = dfl_sim_patch_count(H, W, rho, stride) in row-major (a, b)
 * order; pflags[P]: bit 0 = counts in x, bit 1 = counts in y; pcount[2] = how many patches count in x, in y.
 * dfl_sim_patch_gradncc, once per batch: a workgroup owns one patch row of one view: column sums of the band in LDS
 * (6 (W - 2) doubles, hence DFL_SIM_PATCH_MAX_W), one thread per patch, ONE record of two doubles (sum ncc_x, sum ncc_y)
 * per workgroup in scratch; a second kernel adds a view's PR records in index order and divides by pcount.  No atomics: a
 * view's cost has the same bits whatever else is in the batch.  scratch holds at least
 * dfl_sim_patch_scratch_doubles(V, H, W, rho, stride) = 2 V PR doubles.  Both size functions are negative on bad sizes.
 * Refused with nothing launched: NULL pointers, H < 3, W < 3, H W >= 2^31, V < 1, V > 65535, rho < 1, stride < 1,
 * min_count < 1, a patch larger than the interior (H - 2 < S or W - 2 < S), W > DFL_SIM_PATCH_MAX_W, a short scratch.
 * ------------------------------------------------------------------------------------------------------------ */
#define DFL_SIM_PATCH_MAX_W 1538
typedef struct {
  const float* fx;                /* the three planes of dfl_sim_prepare for the same H, W */
  const float* fy;
  const unsigned char* counted;
  double* ptotals;                /* [P][DFL_SIM_TOTALS] */
  unsigned char* pflags;          /* [P] */
  int32_t* pcount;                /* [2] */
  int32_t H, W, rho, stride, min_count, reserved;
} dfl_sim_patch_prepare_args;
int dfl_sim_patch_prepare(const dfl_sim_patch_prepare_args* a, dfl_stream_t stream);

typedef struct {
  const float* moving;            /* [V][H][W] */
  const float* fx;                /* the planes of dfl_sim_prepare and the outputs of dfl_sim_patch_prepare, same sizes */
  const float* fy;
  const unsigned char* counted;
  const double* ptotals;
  const unsigned char* pflags;
  const int32_t* pcount;
  double* scratch;                /* [V][PR][2] */
  double* cost;                   /* [V] */
  int64_t scratch_doubles;        /* what scratch holds */
  int32_t V, H, W, rho, stride, reserved;
} dfl_sim_patch_gradncc_args;
int dfl_sim_patch_gradncc(const dfl_sim_patch_gradncc_args* a, dfl_stream_t stream);
int64_t dfl_sim_patch_count(int32_t H, int32_t W, int32_t rho, int32_t stride);
int64_t dfl_sim_patch_scratch_doubles(int32_t V, int32_t H, int32_t W, int32_t rho, int32_t stride);

/* ------------------------------------------------------------------------------------------------------------
 * The three similarity entry points above against a BANK of F fixed images: view v is scored
 * against image fixed_of[v].  fx, fy, counted are [F][H][W] and totals [F][DFL_SIM_TOTALS]; for patches ptotals is
 * [F][P][DFL_SIM_TOTALS], pflags [F][P], pcount [F][2].  Image f's slice of every bank is what dfl_sim_prepare (and
 * dfl_sim_patch_prepare) writes for it, called once per image on the slices.  fixed_of is a device array [V].
 * The kernels are those of the single-image entry points, which differ only in where a view's planes and totals start:
 * cost[v] and d_moving[v] have the bits the single-image entry point gives view v against image fixed_of[v], whatever V,
 * F and the other entries of fixed_of are.  No atomics.  Scratch: dfl_sim_scratch_doubles,
 * dfl_sim_gradncc_bwd_scratch_doubles, dfl_sim_patch_scratch_doubles.
 * fixed_of cannot be checked on the host: a view whose fixed_of[v] is outside [0, F) reads nothing from the banks, gets
 * cost[v] = NaN and, in the adjoint, d_moving[v] = 0; the other views are not affected.
 * Refused with nothing launched: what the single-image entry point refuses, F < 1, F > 65535, a NULL fixed_of,
 * F H W >= 2^31.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
  const float* moving;            /* [V][H][W] */
  const float* fx;                /* [F][H][W] */
  const float* fy;                /* [F][H][W] */
  const unsigned char* counted;   /* [F][H][W] */
  const double* totals;           /* [F][DFL_SIM_TOTALS] */
  const int32_t* fixed_of;        /* [V], device */
  double* scratch;                /* [V][bands][6] */
  double* cost;                   /* [V] */
  const void* reserved;           /* not read */
  int64_t scratch_doubles;        /* what scratch holds */
  int32_t V, H, W, F;
} dfl_sim_bank_gradncc_args;
int dfl_sim_bank_gradncc(const dfl_sim_bank_gradncc_args* a, dfl_stream_t stream);

typedef struct {
  const float* moving;            /* [V][H][W] */
  const float* fx;                /* [F][H][W] */
  const float* fy;                /* [F][H][W] */
  const unsigned char* counted;   /* [F][H][W] */
  const double* totals;           /* [F][DFL_SIM_TOTALS] */
  const int32_t* fixed_of;        /* [V], device */
  double* scratch;
  double* cost;                   /* [V] */
  float* d_moving;                /* [V][H][W] */
  const void* reserved;           /* not read */
  int64_t scratch_doubles;        /* what scratch holds */
  int32_t V, H, W, F;
} dfl_sim_bank_gradncc_bwd_args;
int dfl_sim_bank_gradncc_bwd(const dfl_sim_bank_gradncc_bwd_args* a, dfl_stream_t stream);

typedef struct {
  const float* moving;            /* [V][H][W] */
  const float* fx;                /* [F][H][W] */
  const float* fy;                /* [F][H][W] */
  const unsigned char* counted;   /* [F][H][W] */
  const double* ptotals;          /* [F][P][DFL_SIM_TOTALS] */
  const unsigned char* pflags;    /* [F][P] */
  const int32_t* pcount;          /* [F][2] */
  const int32_t* fixed_of;        /* [V], device */
  double* scratch;                /* [V][PR][2] */
  double* cost;                   /* [V] */
  int64_t scratch_doubles;        /* what scratch holds */
  int32_t V, H, W, rho, stride, F;
} dfl_sim_patch_bank_gradncc_args;
int dfl_sim_patch_bank_gradncc(const dfl_sim_patch_bank_gradncc_args* a, dfl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Weighted patch gradient-NCC and the patch adjoint (csrc/sim_patch.hip; DESIGN.md section 21 states the semantics,
 * tests/patch_grad_ref.py restates them in numpy float64).  Patches, flags and the per-patch ncc are those above.
 *
 * Weights: w_x[p] = sum (fx - mean fx)^2 over the counted pixels of a patch that counts in x, else 0; w_y likewise;
 * pwsum[d] = sum_p w_d[p], positive exactly when some patch counts in d.  dfl_sim_patch_weights, once per fixed image after
 * dfl_sim_patch_prepare (for a bank: once per image on its slices), writes pweights[P][2] and pwsum[2] in one workgroup:
 * thread t adds the patches t, t + 256, ... in index order, then the threads in a fixed order.
 *   weighted cost[v] = 1 - (X + Y) / 2,  X = sum_p w_x[p] ncc_x[p] / pwsum[0] (0 when pwsum[0] = 0), Y likewise;
 * the uniform cost above is w = 1 on the patches that count, pwsum = pcount.
 *
 * dfl_sim_patch_eval is dfl_sim_patch_gradncc with three optional parts.  pweights with pwsum (both or neither): the
 * weighted cost; both NULL: the uniform one.  fixed_of [V] (device) with F: a bank, as dfl_sim_patch_bank_gradncc (pweights
 * is then [F][P][2] and pwsum [F][2]); NULL: one image, and F is not read.  d_moving [V][H][W]: the adjoint
 * d cost[v] / d moving[v][r][c] for every pixel, the border included; NULL: the forward alone.  The forward kernels always
 * run first, so cost has the same bits with and without d_moving; with pweights, fixed_of and d_moving all NULL it has the
 * bits of dfl_sim_patch_gradncc, with fixed_of alone those of dfl_sim_patch_bank_gradncc.
 *
 * The adjoint: let c_d[p] = w_d[p] / pwsum[d] (weighted) or 1 / pcount[d] on the patches that count in d (uniform), else
 * 0.  With a the moving and b the fixed Sobel values of direction d over the counted pixels of patch p, va and vb their
 * sums of squared deviations, cab the sum of the products of the deviations:
 *   alpha_p = -1 / (2 sqrt(va vb)),  beta_p = cab / (2 va sqrt(va vb)),  both 0 where the forward rule makes that ncc 0;
 *   g_d(q) = sum over the patches p that hold the counted interior pixel q, in ascending (a, b) order, of
 *            c_d[p] alpha_p (b_q - mean_p b) + c_d[p] beta_p (a_q - mean_p a);   0 at a pixel that is not counted or in no patch;
 *   d_moving = Sobel^T (g_x, g_y), as dfl_sim_gradncc_bwd gathers it.
 * Per view and patch eight float32 (c alpha, c beta, mean a, mean b of x, then of y) are formed in float64, rounded once
 * and kept in scratch; a workgroup owns a 16 x 16 tile of d_moving and adds the patches of a pixel in float32, every product
 * rounded on its own.  No atomics: a view's outputs depend on its own pixels, its fixed image and H, W, rho, stride only.
 * A view whose fixed_of entry is outside [0, F) gets cost = NaN and d_moving = 0; the other views are not affected.
 * scratch holds at least dfl_sim_patch_eval_scratch_doubles(V, H, W, rho, stride, bwd) doubles: 2 V PR, and 4 V P more
 * with bwd != 0 (negative: bad sizes, or more than 2^31 - 1).
 * Refused with nothing launched: what dfl_sim_patch_gradncc refuses (and, with fixed_of, what the bank form refuses),
 * pweights without pwsum or pwsum without pweights, a short scratch, and with d_moving an image of more than 16 x 65535
 * rows; for dfl_sim_patch_weights NULL pointers and P < 1 or P >= 2^31.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
  const double* ptotals;          /* [P][DFL_SIM_TOTALS], of dfl_sim_patch_prepare */
  const unsigned char* pflags;    /* [P] */
  double* pweights;               /* [P][2] */
  double* pwsum;                  /* [2] */
  int64_t P;                      /* dfl_sim_patch_count(H, W, rho, stride) */
} dfl_sim_patch_weights_args;
int dfl_sim_patch_weights(const dfl_sim_patch_weights_args* a, dfl_stream_t stream);

typedef struct {
  const float* moving;            /* [V][H][W] */
  const float* fx;                /* [H][W], or [F][H][W] with fixed_of */
  const float* fy;
  const unsigned char* counted;
  const double* ptotals;          /* [P][DFL_SIM_TOTALS], or [F][P][DFL_SIM_TOTALS] */
  const unsigned char* pflags;    /* [P], or [F][P] */
  const int32_t* pcount;          /* [2], or [F][2] */
  const double* pweights;         /* [P][2], or [F][P][2]; NULL: the uniform cost */
  const double* pwsum;            /* [2], or [F][2]; NULL exactly when pweights is */
  const int32_t* fixed_of;        /* [V], device; NULL: one fixed image */
  double* scratch;                /* [V][PR][2], then [V][P][8] float32 with d_moving */
  double* cost;                   /* [V] */
  float* d_moving;                /* [V][H][W]; NULL: the forward alone */
  int64_t scratch_doubles;        /* what scratch holds */
  int32_t V, H, W, rho, stride, F;
} dfl_sim_patch_eval_args;
int dfl_sim_patch_eval(const dfl_sim_patch_eval_args* a, dfl_stream_t stream);
int dfl_sim_patch_eval_scratch_doubles(int32_t V, int32_t H, int32_t W, int32_t rho, int32_t stride, int32_t bwd);

/* ------------------------------------------------------------------------------------------------------------
 * Outline cost (csrc/sim_outline.hip; DESIGN.md section 26 states the semantics, tests/outline_ref.py restates them in
 * numpy float64): the truncated chamfer distance between the boundaries of S label sets in V moving label maps and in
 * the fixed label maps they are scored against -- the similarity of register(similarity='outline').
 *
 * A label set is a 32-bit word, as for dfl_label_edt.  For set k, a view's label map m and its fixed map f:
 *   M_k, F_k = the boundary sites of the set in m and in f, as dfl_label_edt(boundary = 1) defines them: an in-set pixel
 *              with a 4-neighbour outside the set, or on the image border;
 *   d2m, d2f = the exact squared boundary distance maps of m and of f for set k.  A pixel p is a boundary site of its map
 *              exactly when that map's own distance at p is 0, so the entry point takes the distance maps alone.
 * With cap > 0 in pixels and t(d2) = min(sqrt((double) d2), cap):
 *   a_k = sum over p in M_k of t(d2f[k][p]),  b_k = sum over p in F_k of t(d2m[k][p]),  nM_k = |M_k|,  nF_k = |F_k|;
 *   both counts positive:      c_k = (a_k / nM_k + b_k / nF_k) / (2 cap);
 *   exactly one count positive: c_k = 1, and both sums are reported as 0;
 *   both counts zero:           the set is not scored (sums 0);
 *   cost[v] = the mean of c_k over the scored sets in ascending k, or 1.0 when none is scored.
 * So the cost lies in 0 .. 1 and is 0 exactly when every scored set has the same boundary in both maps.
 * DFL_LABEL_EDT_NONE in either map means "no boundary of that set" (such a map has no zero either).
 *
 * Two launches.  The first: one workgroup per (view, chunk of DFL_SIM_OUTLINE_CHUNK pixels); it loops over the S sets,
 * reads both distance planes coalesced and writes ONE record of 4 S doubles (nM, nF, a, b per set) in scratch: the counts
 * are exact integers in float64, the sums go through csrc/fixed_sum.h.  The second: one workgroup per view; one thread per
 * number of a record adds that number over the view's records in index order, then one thread finishes counts, sums and
 * cost in ascending k.  No atomics: a view's numbers have the same bits alone, in any batch
 * and in any order of views.  scratch holds at least dfl_sim_outline_scratch_doubles(V, S, H, W) =
 * 4 V S ceil(H W / DFL_SIM_OUTLINE_CHUNK) doubles (an int: negative on bad sizes, and when the count exceeds 2^31 - 1).
 * fixed_of (device, [V]) says which of the F fixed maps a view is scored against; NULL: every view against map 0.  It
 * cannot be checked on the host: a view whose entry is outside [0, F) reads nothing out of bounds and gets cost = NaN,
 * counts and sums 0; the other views are not affected.
 * Refused with nothing launched: NULL pointers (only fixed_of may be NULL), V < 1, V > 65535, F < 1, S outside
 * 1..DFL_LABEL_MAX_CLASSES, H < 1, W < 1, (H-1)^2 + (W-1)^2 >= 2^31 - 1 (the size condition of dfl_label_edt), a cap
 * that is not finite and positive, a short scratch.
 * ------------------------------------------------------------------------------------------------------------ */
#define DFL_SIM_OUTLINE_CHUNK 1024
typedef struct {
  const int32_t* d2_moving;       /* [V][S][H][W]  dfl_label_edt(the views' label maps, sets, boundary 1) */
  const int32_t* d2_fixed;        /* [F][S][H][W]  the same of the fixed maps, made once */
  const int32_t* fixed_of;        /* device [V], 0..F-1, or NULL: every view against fixed map 0 */
  int32_t* counts;                /* [V][S][2]  nM, nF */
  double* sums;                   /* [V][S][2]  a, b */
  double* cost;                   /* [V] */
  double* scratch;
  int64_t scratch_doubles;        /* what scratch holds */
  double cap;                     /* pixels */
  int32_t V, F, S, H, W, reserved;
} dfl_sim_outline_args;
int dfl_sim_outline(const dfl_sim_outline_args* a, dfl_stream_t stream);
int dfl_sim_outline_scratch_doubles(int32_t V, int32_t S, int32_t H, int32_t W);

/* ------------------------------------------------------------------------------------------------------------
 * Mutual information (csrc/sim_mi.hip; tests/mi_ref.py restates this section in numpy): the
 * negative mutual information between the intensities of V rendered views and of the fixed images they are scored
 * against, from a joint histogram of integers -- the similarity of register(similarity='mi').  It needs neither a known
 * intensity mapping of the fixed image nor edges.  Every float32 step below is rounded on its own (csrc/build.sh compiles
 * the file with -ffp-contract=off); divisions are correctly rounded.
 *
 * dfl_sim_mi_prepare, once per fixed image (a bank: once per image on its slices of fbin [F][H][W] and info [F][4]).
 *   A pixel is counted when its fixed value is finite and mask is NULL or its mask byte is non-zero: all pixels are
 *   candidates, the border included.  lo_f, hi_f = the smallest and largest counted value, n = how many are counted;
 *   s_f = (float) Bf / (hi_f - lo_f);  fbin = clip((int) floorf((f - lo_f) s_f), 0, Bf - 1) for a counted pixel (0 when
 *   hi_f == lo_f, and where the product is NaN), DFL_SIM_MI_SKIP for one that is not counted.
 *   info[DFL_SIM_MI_INFO] = n, lo_f, hi_f, 0 (0, 0, 0, 0 when nothing is counted).  Two launches.
 *
 * dfl_sim_mi, once per batch.  View v is scored against image f = fixed_of[v] (device, [V]), or image 0 when fixed_of is
 * NULL.  mrange [F][2] (device, float32) holds the moving range (lo, hi) of every image, s = (float)(Bm - 1) / (hi - lo).
 * For a counted pixel with moving value m:
 *   x = (fminf(fmaxf(m, lo), hi) - lo) s      values outside the range clamp, NaN counts as lo
 *   a = x >= Bm - 1 ? Bm - 2 : (int) floorf(x)
 *   q = (int) floorf((x - (float) a) 4096.0f + 0.5f)
 *   hist[v][a][fbin] += DFL_SIM_MI_UNIT - q,  hist[v][a + 1][fbin] += q
 * a first-order Parzen window on the moving intensity in units of 1 / DFL_SIM_MI_UNIT pixel.  hist [V][Bm][Bf] is an
 * output and is overwritten; a view's entries sum to exactly DFL_SIM_MI_UNIT n.  With N = DFL_SIM_MI_UNIT n,
 * h_a = sum_b hist[a][b] and h_b = sum_a hist[a][b] (integers):
 *   MI = sum over hist[a][b] > 0 of (h / N) log((h N) / (h_a h_b))  in float64,  cost[v] = -MI,  0 when n == 0.
 * A view is void when lo, hi, hi - lo or s is not finite, when hi > lo does not hold, or when its fixed_of entry is
 * outside [0, F): cost NaN, hist 0, and in the adjoint ell 0 and d_moving 0; the other views are not affected (device
 * values cannot be refused on the host).
 *
 * dfl_sim_mi_bwd writes cost and hist with the bits of dfl_sim_mi (the same kernels), the table
 *   ell[v][a][b] = log(max(hist[a][b], 1)) - log(max(h_a, 1))  (float64, [V][Bm][Bf]), and
 *   d_moving[v][r][c] = (float)(-((double) s / n) (ell[a + 1][fbin] - ell[a][fbin]))  at a counted pixel with lo < m < hi,
 * exactly 0 at every other pixel (not counted, at or beyond the range, NaN).  This is the derivative of the unquantised
 * cost at a fixed range: the "+ 1" terms and log N cancel because the weights of a pixel sum to a constant, and h_b does
 * not move.  At the ends of the range the clamp makes the cost one-sided, hence the exact zeros there.
 *
 * Kernels: mi_clear zeroes hist; mi_hist_kernel: a workgroup takes DFL_SIM_MI_RUN consecutive pixels of one view, every
 * wave adds into its own uint32 histogram in LDS (integer LDS adds), and the workgroup adds its non-zero bins to hist
 * with 64-bit integer global atomic adds.  Integer sums: no decomposition, batch or arrival order changes a bit; there
 * are no float atomics.  mi_finish_kernel: one workgroup per view, marginals as integers, the float64 sum in an order
 * that depends on Bf and Bm only.  mi_adjoint_kernel stages the view's table in LDS.
 * Refused with nothing launched and the outputs untouched: NULL pointers (mask and fixed_of may be NULL), H < 1, W < 1,
 * H W >= 2^31, F < 1, F > 65535, F H W >= 2^31, V < 1, V > 65535, Bf or Bm outside 2..DFL_SIM_MI_MAX_BINS.
 * ------------------------------------------------------------------------------------------------------------ */
#define DFL_SIM_MI_UNIT 4096
#define DFL_SIM_MI_MAX_BINS 64
#define DFL_SIM_MI_SKIP 255
#define DFL_SIM_MI_INFO 4
#define DFL_SIM_MI_RUN 8192
typedef struct {
  const float* fixed;             /* [H][W] */
  const unsigned char* mask;      /* [H][W], or NULL */
  unsigned char* fbin;            /* [H][W] */
  double* info;                   /* [DFL_SIM_MI_INFO] */
  int32_t H, W, Bf, reserved;
} dfl_sim_mi_prepare_args;
int dfl_sim_mi_prepare(const dfl_sim_mi_prepare_args* a, dfl_stream_t stream);

typedef struct {
  const float* moving;            /* [V][H][W] */
  const unsigned char* fbin;      /* [F][H][W], of dfl_sim_mi_prepare with the same Bf */
  const double* info;             /* [F][DFL_SIM_MI_INFO] */
  const float* mrange;            /* [F][2], device: lo, hi of the moving intensities */
  const int32_t* fixed_of;        /* [V], device, or NULL: every view against image 0 */
  uint64_t* hist;                 /* [V][Bm][Bf] */
  double* cost;                   /* [V] */
  int32_t V, H, W, F, Bf, Bm;
} dfl_sim_mi_args;
int dfl_sim_mi(const dfl_sim_mi_args* a, dfl_stream_t stream);

typedef struct {
  const float* moving;            /* [V][H][W] */
  const unsigned char* fbin;      /* [F][H][W] */
  const double* info;             /* [F][DFL_SIM_MI_INFO] */
  const float* mrange;            /* [F][2], device */
  const int32_t* fixed_of;        /* [V], device, or NULL */
  uint64_t* hist;                 /* [V][Bm][Bf] */
  double* cost;                   /* [V] */
  double* ell;                    /* [V][Bm][Bf] */
  float* d_moving;                /* [V][H][W] */
  int32_t V, H, W, F, Bf, Bm;
} dfl_sim_mi_bwd_args;
int dfl_sim_mi_bwd(const dfl_sim_mi_bwd_args* a, dfl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Detector model: rendered line integrals -> detector intensities (csrc/expose.hip; DESIGN.md section 17 states the
 * semantics, tests/expose_ref.py restates them in numpy).  Per view v and pixel i = r C + c, all in fp32:
 *   T = expf(-att);  B = the separable blur of T with taps[0 .. 2 rho] (rows first, then columns, indices clamped to
 *   the image; each sum runs from tap 0 upwards; rho = 0: B = T);  N = photons B;
 *   noisy = N (+ sqrtf(N) z1 when quantum) (+ electronic_sigma z2 when electronic);  I = gain noisy.
 * z1, z2 are the standard normals of csrc/philox.h (Philox4x32-10, counter i, Box-Muller) under the 64-bit keys
 * key_q[v], key_e[v]; a term that is off reads no key and adds nothing.  out is fp32, or uint16 when u16: I clamped to
 * [0, 65535] and rounded to nearest even.  z1 / z2 (tests only) receive the normals when not NULL.
 * One launch; a workgroup owns a 16 x 64 tile of one view; no atomics.  Refused with nothing launched: NULL att or out,
 * V < 1 or > 65535, R < 1, C < 1, R C >= 2^31, rho outside 0..DFL_EXPOSE_MAX_RADIUS, photons <= 0, gain <= 0,
 * electronic_sigma < 0 (or any of them not finite), a noise flag with a NULL key array.
 * ------------------------------------------------------------------------------------------------------------ */
#define DFL_EXPOSE_MAX_RADIUS 8
typedef struct {
  const float* att;               /* [V][R][C], finite and >= 0 */
  void* out;                      /* [V][R][C] fp32, or uint16 when u16 */
  const uint64_t* key_q;          /* [V], device; NULL allowed when quantum == 0 */
  const uint64_t* key_e;          /* [V], device; NULL allowed when electronic == 0 */
  float* z1;                      /* [V][R][C] or NULL */
  float* z2;                      /* [V][R][C] or NULL */
  float taps[2 * DFL_EXPOSE_MAX_RADIUS + 1];   /* taps[0 .. 2 rho] */
  int32_t rho;
  int32_t V, R, C;
  int32_t u16, quantum, electronic;
  float photons, gain, electronic_sigma;
} dfl_expose_args;
int dfl_drr_expose(const dfl_expose_args* a, dfl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Tools: straight metal instruments and beads in a rendered view, as analytic capsules (csrc/drr_tools.hip; DESIGN.md
 * section 27; tests/tools_ref.py restates this text in numpy float64).  dfl_drr_tools runs between dfl_drr_render and
 * dfl_drr_expose: it adds line integrals to att in place.
 *
 * Frame.  A capsule is (a[3], b[3], r, mu): every point within r of the segment [a, b].  a and b are in mm in the camera
 * projective frame (the frame the C2I matrices of dfl_drr_render map from; the source is its origin), r > 0 in mm, mu >= 0
 * per mm.  a == b is a sphere (a bead).
 * Ray.  The ray of output pixel (c, r) is x(t) = t d, t >= 0, d = Q [c, r, 1], Q = qscale (row-major 3 x 3, the qscale of
 * dfl_drr_render).
 * Chord.  len_j = |d| * measure{ t >= 0 : dist(x(t), segment[a_j, b_j]) <= r_j }.  A capsule is convex, so the set is one
 * interval: from the smallest entry to the largest exit over the pieces the ray hits, clipped to t >= 0.  The pieces are the
 * sphere about a, the sphere about b and -- when a != b -- the cylinder about the axis, clipped to the slab between the
 * planes through a and b normal to the axis.  With u = d / |d| and e = (b - a) / |b - a|, u_perp = u - (u . e) e: a ray
 * with |u_perp|^2 <= 1e-10 (within 1e-5 rad of the axis; TOOLS_PARALLEL in csrc/drr_tools.hip) is parallel to the axis
 * and takes the two spheres alone.
 * Output.  s = 0; for j = 0 .. n_tools - 1 ascending: s += mu_j * len_j, in float32; then att[v][r][c] += s (one rounding:
 * float32(old + s)).  tool_len[v][r][c] = sum_j len_j, formed in the same order; NULL: not wanted.
 * Simplifications.  Metal adds to the tissue it displaces (the CT's attenuation along the chord is not removed).
 * Overlapping capsules count twice.  Attenuation is monoenergetic: no beam hardening and no streaks.  The label map is not
 * touched: a label is the projected anatomy whatever lies in front of it.
 *
 * Arithmetic (float32, every product and sum rounded on its own: the file is built with -ffp-contract=off; dots are summed
 * x, y, z from the left).  Per pixel: d, |d| = sqrtf(d . d), u = d / |d| per component (|d| = 0 or not finite: s = 0).
 * Per capsule and sphere centre p: tc = u . p; q = p - tc u as a VECTOR, then q2 = q . q -- never |p|^2 - tc^2, which at
 * 800 mm loses the radius of a wire -- h2 = r r - q2; hit when h2 >= 0: [tc - h, tc + h], h = sqrtf(h2).
 * Cylinder: w = b - a, L = sqrtf(w . w), e = w / L, ue = u . e, u_perp = u - ue e, A = u_perp . u_perp, ae = a . e,
 * a_perp = a - ae e, tcyl = (u_perp . a_perp) / A, q = a_perp - tcyl u_perp (the offset in the plane normal to the axis, a
 * vector again), h2 = r r - q . q; hit when h2 >= 0: [tcyl - h, tcyl + h], h = sqrtf(h2 / A), cut to the slab
 * [min, max] of ae / ue and (ae + L) / ue (ue = 0: kept whole when 0 <= -ae <= L, else dropped), dropped when empty.
 * len = max(exit - max(entry, 0), 0): u is a unit vector, so t is in mm.
 *
 * tools is a device array [views][n_tools] of dfl_tools_capsule (48 bytes).  rect = c0, r0, c1, r1 (inclusive) is a pixel
 * rectangle computed conservatively on the host: a pixel outside it skips the capsule (its chord must be 0 there), and a
 * wave whose 8 x 8 pixels are all outside skips it without diverging.  n_tools is 0 .. DFL_TOOLS_MAX and is the stride of
 * every view; a view with fewer capsules pads with r = 0 records.  Values inside the device array cannot be checked on
 * the host: a record with a field that is not finite or with r <= 0 contributes nothing.
 * One launch, one thread per pixel and view (a wave covers 8 x 8 pixels, as dfl_drr_render mapping 0); no atomics, no LDS,
 * one 4-byte load and store per pixel and output, 64-bit offsets.  n_tools == 0 returns 0 and launches nothing.
 * Refused with nothing launched and the outputs untouched: NULL att, NULL tools with n_tools > 0, views outside
 * 1..65535, H < 1, W < 1, H W >= 2^31, n_tools outside 0..DFL_TOOLS_MAX, a qscale entry that is not finite.
 * ------------------------------------------------------------------------------------------------------------ */
#define DFL_TOOLS_MAX 64
typedef struct {
  float a[3];                     /* mm, camera projective frame */
  float b[3];
  float r;                        /* mm; <= 0: a padding record */
  float mu;                       /* per mm */
  int32_t rect[4];                /* c0, r0, c1, r1, inclusive */
} dfl_tools_capsule;
typedef struct {
  float* att;                     /* [views][H][W], modified in place */
  float* tool_len;                /* [views][H][W] or NULL */
  const dfl_tools_capsule* tools; /* device, [views][n_tools]; NULL allowed when n_tools == 0 */
  float qscale[9];                /* Q, row-major */
  int32_t views, H, W, n_tools;
  int32_t reserved;               /* not read */
} dfl_tools_args;
int dfl_drr_tools(const dfl_tools_args* a, dfl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Boundary loss (csrc/boundary.hip; tests/boundary_ref.py restates this text in numpy): the signed
 * distance maps of a batch of one-hot targets and the term of Kervadec et al. (MIDL 2019) on them, fused with the value
 * and the gradient of dfl_dice_ncc_loss.
 *
 * Labels.  tseg is the one-hot target [B, C, h, w] fp32 seen through element strides (sN, sC, sH; unit stride along w), as
 * dfl_dice_ncc_loss takes it.  g[b][p] = argmax_c tseg[b][c][p], the first maximum winning (torch.max's rule).
 * Regions.  S_c = the pixels of image b with g == c;  D2(p, A) = the exact squared Euclidean distance from p to the
 * nearest pixel of A: dfl_label_edt with boundary = 0.
 * Signed distance map, per (b, c), in pixels of the target grid:
 *   phi[b][c][p] = 0                                      for every p when S_c is empty or the whole image;
 *   phi[b][c][p] = +sqrt(D2(p, S_c))                      for p outside S_c (>= 1);
 *   phi[b][c][p] = -(sqrt(D2(p, complement of S_c)) - 1)  for p in S_c (<= 0; the pixels just inside the edge get 0).
 * This is one_hot2dist of the paper's code: edt(neg) * neg - (edt(pos) - 1) * pos.  Zeros are +0.0.  The root is taken
 * in double and rounded once: (float) sqrt((double) d2) outside, (float) (1.0 - sqrt((double) d2)) inside, so a perfect
 * square gives its exact root.
 *
 * dfl_boundary_maps: phi dense [B][C][h][w] fp32, 16-byte aligned for the 16-byte loads of dfl_boundary_loss.  Three
 * stages on the caller's stream, nothing read back: (1) arg-max -> uint8 labels in scratch; (2) dfl_label_edt over pairs
 * of label sets -- {c} and "every label < C but c" -- in chunks of images x classes of at most 15 pairs (30 of the 31 sets
 * a call takes) whose int32 planes stay below 256 MiB (a single pair may exceed that); (3) per chunk, combine: a pixel
 * reads its label and the plane that applies to it; DFL_LABEL_EDT_NONE there says "class absent" (outside) or "class
 * fills the image" (inside), which is the zero rule without a reduction of its own.  Nothing reaches across images: an
 * image has the same bits alone and inside any batch.  scratch: dfl_boundary_maps_scratch_bytes(B, C, h, w) bytes (an
 * int: negative on a refusal, and when the count exceeds 2^31 - 1), 16-byte aligned.
 * Refused before any pointer is followed: B, h or w < 1, C outside 2..DFL_LABEL_MAX_CLASSES, (h-1)^2 + (w-1)^2 >=
 * 2^31 - 1 (the size condition of dfl_label_edt), a scratch beyond 2^31 - 1 bytes, NULL pointers, a misaligned scratch.
 *
 * Term.  L_B = (1/N) sum over b, c >= skip_bg, p of seg[b][c][p] * phi[b][c][p],  N = B (C - skip_bg) h w;
 *        d(beta L_B) / d seg[b][c][p] = beta phi[b][c][p] / N for c >= skip_bg, 0 for a skipped background channel.
 * dfl_boundary_loss, stage 1: the sum in float64 in a fixed order (csrc/fixed_sum.h: wave shuffle, four waves through
 * LDS, one record per workgroup in sums, the records in index order; no float atomics; the pixel-to-thread assignment is
 * fixed by the shape, so two runs give the same bits).  Then one thread: *loss = (float)(beta L_B), or with
 * accumulate_loss *loss = (float)((double) *loss + beta L_B) -- onto the value dfl_dice_ncc_loss stage 1 left there, one
 * rounding.  sums holds dfl_boundary_loss_scratch_doubles(B, C, h) doubles (an int, at most 1024; 0 on sizes < 1).
 * Stage 2: dseg[b][c][p] = k phi[b][c][p] with k = *grad_scale * (float)(beta / N) (grad_scale: a DEVICE scalar, NULL =
 * 1), through element strides (all 0 = dense [B][C][h][w]).  With accumulate_grad the product is added onto what is
 * there -- what dfl_dice_ncc_loss stage 2 wrote, launched before on the same stream -- and a skipped background channel
 * is left alone; without, that channel is written as zeros.
 * Both stages stream rows: 256 threads, a wave per row of an (image, class), at most 1024 workgroups; 16-byte accesses
 * of phi, and of seg / dseg on the rows whose address allows it (a centre-crop window starts at any column), 4-byte
 * ones otherwise and for the head and tail of a row; 64-bit offsets.
 * Refused before any pointer is followed: a NULL block, sizes as above (h w < 2^31 follows), stage other than 1 or 2,
 * a beta that is not finite, NULL phi, NULL seg / loss / sums in stage 1, NULL dseg in stage 2, gradient strides of
 * which some but not all are 0.
 * ------------------------------------------------------------------------------------------------------------ */
int dfl_boundary_maps_scratch_bytes(int32_t B, int32_t C, int32_t h, int32_t w);
int dfl_boundary_maps(const float* tseg, int64_t sN, int64_t sC, int64_t sH, int32_t B, int32_t C, int32_t h, int32_t w,
                      float* phi, void* scratch, dfl_stream_t stream);
typedef struct {
  const float* seg;               /* [B, C, h, w] through seg_s*; stage 1 */
  const float* phi;               /* dense [B][C][h][w], dfl_boundary_maps */
  float* loss;                    /* 1 float; stage 1 */
  double* sums;                   /* dfl_boundary_loss_scratch_doubles(B, C, h) doubles; stage 1 */
  const float* grad_scale;        /* device scalar or NULL (= 1); stage 2 */
  float* dseg;                    /* [B, C, h, w] through dseg_s* (all 0: dense); stage 2 */
  int64_t seg_sN, seg_sC, seg_sH;
  int64_t dseg_sN, dseg_sC, dseg_sH;
  int32_t B, C, h, w;
  int32_t skip_bg;
  int32_t stage;                  /* 1: value, 2: gradient */
  int32_t accumulate_loss, accumulate_grad;
  float beta;
  int32_t reserved;               /* not read */
} dfl_boundary_loss_args;
int dfl_boundary_loss_scratch_doubles(int32_t B, int32_t C, int32_t h);
int dfl_boundary_loss(const dfl_boundary_loss_args* a, dfl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Cross-entropy and focal term (csrc/ce_loss.hip; tests/ce_ref.py restates this text in numpy): the
 * per-pixel likelihood term on the soft-max PROBABILITIES the head writes, fused with the value and the gradient of
 * dfl_dice_ncc_loss (and of dfl_boundary_loss).  There is no logits form: dfl_head_fwd fuses the soft-max and Dice needs
 * the probabilities.
 *
 * seg [B, C, h, w] fp32 probabilities and tseg, the target of the same shape (one-hot in training; any finite values >= 0),
 * each through element strides (sN, sC, sH; unit stride along w).  class_wgt[c] >= 0 (entries >= C are not read), gamma the
 * focusing exponent.  EPS = 2^-100 (0x1p-100f), s' = min(max(s, EPS), 1):
 *   f(s, t, w) = -w t (1 - s')^gamma log s'                          with 0^0 = 1
 *   L_CE       = (1 / N) sum over b, c, p of f(seg, tseg, class_wgt[c]),   N = B h w  (pixels, not elements)
 *   d(lambda L_CE) / d seg[b][c][p] = -(lambda / N) w_c t [ (1 - s')^gamma / s' - gamma (1 - s')^(gamma-1) log s' ]
 * Every channel counts, background included (the skip_bg of Dice is not read here; class_wgt[0] = 0 leaves it out).
 * gamma = 0 is plain cross-entropy and runs without powf; otherwise 1 <= gamma <= 8 (between 0 and 1 the derivative is
 * unbounded at s = 1: refused).
 * Below EPS the gradient is STILL the formula above at s' -- not the zero that the clamped value's true derivative would
 * give: a confidently wrong pixel keeps its gradient.  1 / EPS times lambda / N is finite in fp32, and dfl_head_bwd
 * multiplies by s, so the products it forms are O(1).
 * An element with w_c t == 0 contributes exactly +0 and evaluates no logarithm; stage 2 writes it as 0.0f, and with
 * accumulate_grad leaves it as it is (the augmentation's "outside the frame: all masks 0" pixels add nothing).
 * Element terms are fp32 with the accurate logf / powf (no fast intrinsics).
 *
 * dfl_ce_loss, stage 1: the sum in float64 in a fixed order (csrc/fixed_sum.h: wave shuffle, four waves through LDS, one
 * record per workgroup in sums, the records in index order; no float atomics; the pixel-to-thread assignment is fixed by
 * the shape, so two runs give the same bits).  Then one thread: *loss = (float)(lambda L_CE), or with accumulate_loss
 * *loss = (float)((double) *loss + lambda L_CE) -- onto what dfl_dice_ncc_loss and optionally dfl_boundary_loss stage 1 left
 * there, one rounding.  sums holds dfl_ce_loss_scratch_doubles(B, C, h) doubles (an int, at most 1024; 0 on sizes < 1).
 * Stage 2: dseg[b][c][p] = the derivative above with lambda / N replaced by k = *grad_scale * (float)(lambda / N)
 * (grad_scale: a DEVICE scalar, NULL = 1), through element strides (all 0 = dense [B][C][h][w]); with accumulate_grad it
 * is added onto what is there -- what dfl_dice_ncc_loss / dfl_boundary_loss stage 2 wrote, launched before on the same
 * stream.
 * Both stages stream rows: 256 threads, a wave per row of an (image, class), at most 1024 workgroups, rows grid-strided;
 * 16-byte accesses of seg / tseg / dseg on the rows whose address allows it (a centre-crop window starts at any column),
 * 4-byte ones otherwise and for the head and tail of a row; 64-bit offsets.
 * Refused before any pointer is followed: a NULL block; B, h or w < 1; C outside 2..DFL_LABEL_MAX_CLASSES; a stage other
 * than 1 or 2; a lambda or gamma that is not finite; a gamma outside {0} and [1, 8]; a class weight (of the first C) that is
 * negative or not finite; NULL seg / tseg / loss / sums in stage 1, NULL seg / tseg / dseg in stage 2; gradient strides
 * of which some but not all are 0.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct {
  const float* seg;               /* [B, C, h, w] through seg_s* */
  const float* tseg;              /* [B, C, h, w] through tseg_s* */
  float* loss;                    /* 1 float; stage 1 */
  double* sums;                   /* dfl_ce_loss_scratch_doubles(B, C, h) doubles; stage 1 */
  const float* grad_scale;        /* device scalar or NULL (= 1); stage 2 */
  float* dseg;                    /* [B, C, h, w] through dseg_s* (all 0: dense); stage 2 */
  int64_t seg_sN, seg_sC, seg_sH;
  int64_t tseg_sN, tseg_sC, tseg_sH;
  int64_t dseg_sN, dseg_sC, dseg_sH;
  int32_t B, C, h, w;
  int32_t stage;                  /* 1: value, 2: gradient */
  int32_t accumulate_loss, accumulate_grad;
  float lambda, gamma;
  float class_wgt[32];            /* entries >= C are not read */
} dfl_ce_loss_args;
int dfl_ce_loss_scratch_doubles(int32_t B, int32_t C, int32_t h);
int dfl_ce_loss(const dfl_ce_loss_args* a, dfl_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Product arithmetic of the convolution / weight-gradient GEMMs (fast paths; odd channel counts always use fp32):
 *   0 "fp32"    v_mfma_f32_32x32x2_f32: fp32 products, fp32 accumulation.
 *   1 "bf16x3"  every fp32 operand value is split into hi + lo bf16 parts when it is staged in LDS and the product is
 *               hi*hi + hi*lo + lo*hi on the bf16 matrix pipe (fp32 accumulation): relative error 2^-16 per product
 *               -- 32x tighter than the TF32 products PyTorch uses for the reference on NVIDIA GPUs by default -- and
 *               ~1.8x the throughput of mode 0.  Forward outputs stay within the 1e-4 parity bar (measured 2e-5).
 *   2 "bf16x6"  three parts, six products: as exact as fp32 multiplication (convolutions only).
 *   3 "bf16"    plain bf16 products (operands rounded to bf16, fp32 accumulation, fp32 tensors): 2^-9 per product; the
 *               arithmetic BASELINE configs[1] names.  NOT inside the 1e-4 forward bar (measured ~1e-2); validated by
 *               training quality (tests/test_gpu_unet.py).
 *   4 "bf16s"   bf16 STORAGE (BASELINE configs[1] as named): activations, activation gradients and the GEMM copies of the
 *               weights live in HBM as bf16; products bf16, accumulation / BatchNorm statistics / losses / master weights /
 *               weight gradients fp32.  The mode is a property of the recorded program (the caller sets the *_bf16 flags
 *               of the argument blocks and allocates bf16 tensors); entry points look at the flags, not at the mode.
 *               Same validation as mode 3 (training quality, label agreement).
 * Process-wide; initial value from the environment variable DFL_MATH, else DFL_MATH_DEFAULT.
 * ------------------------------------------------------------------------------------------------------------ */
#define DFL_MATH_DEFAULT 0
int dfl_get_math_mode(void);
int dfl_set_math_mode(int32_t mode);

/* ------------------------------------------------------------------------------------------------------------
 * Program execution: run a recorded list of the calls above with ONE host->library transition.  The host builds
 * the array once per (network, input shape) and replays it every step (forward, backward); this is the launch
 * path bench.py times.  `args` points to the struct the matching function takes.
 * ------------------------------------------------------------------------------------------------------------ */
typedef enum {
  DFL_OP_CONV = 1, DFL_OP_WGRAD = 2, DFL_OP_SUM_PARTIALS = 3, DFL_OP_PACK = 4, DFL_OP_BN_FINALIZE = 5,
  DFL_OP_BN_EVAL = 6, DFL_OP_COLSTATS = 7, DFL_OP_BN_BWD_FINALIZE = 8, DFL_OP_BN_RELU_BWD = 9,
  DFL_OP_REDUCE_PARTIALS = 10, DFL_OP_AFFINE_COPY = 11, DFL_OP_POOL_FWD = 12, DFL_OP_POOL_BWD = 13,
  DFL_OP_HEAD_FWD = 14, DFL_OP_HEAD_BWD = 15, DFL_OP_MEMSET = 16, DFL_OP_REDUCE_BATCH = 17,
  DFL_OP_RECORD = 18, DFL_OP_WAIT = 19, DFL_OP_UPSAMPLE_FWD = 20, DFL_OP_UPSAMPLE_BWD = 21,
  DFL_OP_BN_FINALIZE_LIVE = 22, DFL_OP_BN_BWD_FINALIZE_LIVE = 23, DFL_OP_CONV_PAIR = 24
} dfl_op_kind;

typedef struct { const float* src; float* dst; int64_t n; int32_t splits; int32_t T; } dfl_sum_partials_args;
typedef struct { const dfl_pack_job* jobs_dev; int64_t max_elems; int32_t njobs; int32_t tiled; } dfl_pack_args;   /* tiled: max_elems = total tiles, dfl_pack_weights_tiled */
typedef struct { const float* gamma; const float* beta; const float* running_mean; const float* running_var;
                 float* scale; float* shift; int32_t C; float eps; } dfl_bn_eval_args;
typedef struct { const float* partials; float* out; int32_t nblocks, stride, C, reserved; } dfl_reduce_partials_args;
typedef struct { void* ptr; int64_t bytes; } dfl_memset_args; /* zero fill */
typedef struct { const dfl_reduce_job* jobs_dev; int32_t njobs, total_blocks; } dfl_reduce_batch_args;
typedef struct { const dfl_bn_live_job* jobs_dev; int32_t njobs, max_C; } dfl_bn_live_args;
typedef struct { const dfl_bn_bwd_live_job* jobs_dev; int32_t njobs, max_C; } dfl_bn_bwd_live_args;
typedef struct { const dfl_conv_args* a; const dfl_conv_args* b; } dfl_conv_pair_args;   /* dfl_conv2d_pair */

/* Side streams.  An op with stream = 1..DFL_MAX_SIDE_STREAMS runs on a library-owned side stream, beside the ops of the
 * caller's stream (stream 0).  DFL_OP_RECORD records library event `event` on the op's stream, DFL_OP_WAIT makes the op's
 * stream wait for it; events are library-owned, identified by small integers the program chooses (0..65535).
 * What the executor guarantees for every range [ops, ops + n_ops) it is given -- dfl_exec and dfl_graph_capture alike, so a
 * program means the same replayed op by op, as one hipGraph, or cut into ranges:
 *   - the first op of a side stream in the range starts behind everything the caller's stream held when that op was reached
 *     (earlier ops of the range included);
 *   - at the end of the range, also after a failed op, the caller's stream waits for every side stream the range used: behind
 *     the call (the graph launch) everything the range enqueued is ordered in front of later work of the caller's stream;
 *   - ops of one stream run in program order;
 *   - a DFL_OP_WAIT for an event that no op of THIS range recorded is skipped: the range that recorded it was joined at
 *     its end, which orders more than the wait asks for.
 * What a side-stream op may assume: exactly that.  Everything else is the program's job -- a side-stream op that reads what
 * the caller's stream writes LATER in the range, or writes what it reads or writes later, needs a RECORD behind it and a
 * WAIT in front of the later op; memory that both sides touch without such a pair is a race.
 * Under dfl_graph_capture the side streams join the capture (fork) and leave it (join) inside the one graph; no event or
 * stream call survives as a node.  The side streams and events are process-wide: one thread replays or captures at a time.
 * dfl_exec_timed ignores streams and events: program order on one stream is a valid schedule of any program. */
typedef struct { int32_t event; int32_t reserved; } dfl_sync_args;
#define DFL_MAX_SIDE_STREAMS 2

typedef struct {
  int32_t kind;          /* dfl_op_kind */
  int32_t stream;        /* 0 = the stream passed to dfl_exec; 1..DFL_MAX_SIDE_STREAMS = library-owned side streams.
                            Independent kernels of small layers (a layer's weight gradient next to its data
                            gradient) fill the GPU better side by side; ordering is the program's job (RECORD/WAIT). */
  const void* args;
} dfl_op;

int dfl_exec(const dfl_op* ops, int32_t n_ops, dfl_stream_t stream);
/* Same, with a hipEvent pair recorded on `stream` around every op; blocks until done and returns the per-op
 * milliseconds in ms_out[n_ops].  Measurement aid for bench.py (roofline.achieved); not used on the timed path. */
int dfl_exec_timed(const dfl_op* ops, int32_t n_ops, dfl_stream_t stream, float* ms_out);

/* hipGraph form of a program (BASELINE configs[4]: "test_ensemble.py 5-model ensemble, hipGraph-captured"; the reference
 * enqueues every torch op of UNet.forward one by one, util.py:318-373).  dfl_graph_capture records the ops -- side-stream
 * ops as parallel branches, forked and joined as "Side streams" above says -- into a hipGraph by
 * stream capture on a private stream (nothing executes; `stream` is accepted for symmetry and unused: callers usually
 * sit on the null stream, which cannot capture) and instantiates it; dfl_graph_launch replays it on any stream.  The argument structs are
 * consumed at capture time: pointers and sizes are frozen into the graph, memory CONTENTS are read at replay.  The
 * graph stays valid as long as the buffers it names do. */
/* Tuning knob (process-wide, like the math mode): dfl_conv2d takes its row-tiled 3x3 kernels (conv_rows.hip: wide
 * images, tiles of whole row segments, each kernel row staged once for its three taps) only when they yield at least
 * this many workgroups -- they have no split-K form; default 512.  Returns the previous value.  Tests lower it to
 * exercise those kernels on small problems. */
int dfl_set_conv_rows_min_tiles(int32_t n);

typedef struct dfl_graph_s* dfl_graph_t;
int dfl_graph_capture(const dfl_op* ops, int32_t n_ops, dfl_stream_t stream, dfl_graph_t* graph_out);
int dfl_graph_launch(dfl_graph_t graph, dfl_stream_t stream);
int dfl_graph_nodes(dfl_graph_t graph);      /* kernel / memset nodes captured (diagnostics), negative = error */
int dfl_graph_destroy(dfl_graph_t graph);
/* Tile configuration the launcher picks for these arguments (dfl_conv_config: csrc/conv_plan.hip, 16 + the bf16 tile
 * configurations it lists; dfl_wgrad_config: csrc/wgrad_gemm.hip); lets a profile be matched to kernel template names. */
int dfl_conv_config(const dfl_conv_args* a);
int dfl_wgrad_config(const dfl_wgrad_args* a);

#ifdef __cplusplus
}
#endif
#endif /* DFL_HIP_H */
