/*
 * rave_hip.h -- C ABI of librave_hip.so: the MI355X (gfx950 / CDNA4) hot path of RAVE.
 *
 * The reference (acids-ircam/RAVE) has NO native/FFI interface: its "operator API" for this
 * path is the set of Python leaf-module signatures that gin hands to rave.model.RAVE
 * (SURVEY.md section 8b).  Each entry point below therefore cites the reference *Python* site it
 * replaces; INTEGRATION.md shows the ctypes binding a maintainer would add on the reference
 * side.  All citations are relative to the reference tree.
 *
 * Conventions
 *   - tensors are contiguous fp32, layout (B, C, L) with L innermost (PyTorch default);
 *   - every pointer is a DEVICE pointer owned by the caller (the PyTorch caching allocator in
 *     the Python binding); the library never allocates, frees or synchronises;
 *   - alignment: activations, gradients, parameters and optimizer state may sit at any 4-byte aligned address (the
 *     kernels pick 16-byte paths only where the pointers allow them).  Buffers the caller allocates FOR the library --
 *     packed weights, workspaces, range slots -- are expected 16-byte aligned: rh_residual_unit_fwd_f32 refuses misaligned
 *     packed weights (RH_ERR_INVALID), the convolution entry points take a slower kernel or run unsplit instead;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it;
 *   - return value: RH_OK (0), <0 = invalid / unsupported argument (nothing enqueued),
 *     >0 = hipError_t of the failed launch; rh_last_error() gives a thread-local message;
 *   - re-entrant: no mutable global state (forward runs on the Python thread, backward on
 *     PyTorch's autograd thread with the GIL released by ctypes).
 */
#ifndef RAVE_HIP_H
#define RAVE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RH_VERSION 100 /* 0.1.0 */

#define RH_OK 0
#define RH_ERR_INVALID (-1)     /* inconsistent descriptor / null pointer */
#define RH_ERR_UNSUPPORTED (-2) /* valid but not implemented (e.g. groups != 1) */
#define RH_ERR_WORKSPACE (-3)   /* workspace too small; see rh_conv1d_workspace_bytes */

typedef void* rh_stream_t; /* hipStream_t */

/* Activation fused on the conv INPUT (the reference applies it as a separate nn.Module right
 * before the conv: rave/blocks.py:93-105 DilatedUnit, :559, :578, :648, :673). */
enum rh_act {
    RH_ACT_NONE = 0,
    RH_ACT_LEAKY = 1, /* nn.LeakyReLU(slope)          rave/blocks.py:90,527,612; discriminator.py:101 */
    RH_ACT_SNAKE = 2  /* x + sin^2(a x)/(a+1e-9)      rave/blocks.py:852-860 (per-channel alpha)      */
};

/*
 * One 1-D convolution geometry.  Replaces cached_conv.Conv1d / cached_conv.ConvTranspose1d as
 * used by the reference (call sites: rave/pqmf.py:256-273, rave/blocks.py:96-108,536-592,
 * 637-692) and torch.nn.Conv1d / torch.nn.Conv2d with (k,1) kernels as used by the
 * discriminators (rave/discriminator.py:77-119,174-195).
 *
 * transposed == 0:  y[b,co,l] = bias[co] + sum_{ci,t} w[co,ci,t] * act(x)[b,ci, l*stride + t*dilation - pad_left]
 *                   (zero outside [0,l_in)); pad_right is implied by l_out.            w: (c_out, c_in, kernel)
 * transposed == 1:  torch conv_transpose1d(act(x), w, stride, padding=pad_left)         w: (c_in, c_out, kernel)
 *                   l_out = (l_in-1)*stride - 2*pad_left + kernel ; dilation must be 1.
 *
 * inner > 1 describes a Conv2d with kernel (k,1), stride (s,1), padding (p,0) on a (B,C,H,W)
 * tensor with W == inner (MultiPeriodDiscriminator, rave/discriminator.py:186-195): l_in/l_out
 * are H_in/H_out and every position is `inner` contiguous elements.  in_valid (0 = all) is the
 * number of leading elements of each (b,c) input row that are real data; the remainder reads as
 * zero (this is MultiPeriodDiscriminator.fold's zero pad, done in-kernel).
 */
typedef struct rh_conv1d_desc {
    int32_t batch;
    int32_t c_in;
    int32_t c_out;
    int32_t l_in;
    int32_t l_out;
    int32_t kernel;
    int32_t stride;
    int32_t dilation;
    int32_t pad_left;
    int32_t transposed;
    int32_t groups;   /* must be 1 */
    int32_t inner;    /* 1 for Conv1d */
    int32_t in_valid; /* 0 = l_in*inner */
    int32_t act;      /* enum rh_act, fused on the conv input */
    float act_slope;  /* LeakyReLU slope */
    int32_t out_act;  /* RH_ACT_NONE / RH_ACT_LEAKY applied to the OUTPUT (forward only): y = out_act(conv + bias
                       * + residual), as WNConv2d(...) + LeakyReLU(0.1) of rave/descript_discriminator.py:22-27.
                       * The backward entry points ignore it: pass dy * out_act'(y) (rh_act_bwd_f32). */
    float out_slope;
} rh_conv1d_desc;

int rh_version(void);
const char* rh_last_error(void);


/* ---- weight preparation --------------------------------------------------------------- */

/* torch.nn.utils.weight_norm(dim=0) as applied by rave/blocks.py:15-22 `normalization`:
 *   w[r,:] = g[r] * v[r,:] / ||v[r,:]||_2 , rows = size of dim 0, cols = product of the others
 *   (dim 0 = out-channels for Conv1d, IN-channels for ConvTranspose1d).  norms[r] = ||v[r,:]||. */
int rh_weight_norm_fwd_f32(const float* v, const float* g, int64_t rows, int64_t cols, float* w,
                           float* norms, rh_stream_t stream);
/* backward of the above: dv, dg from dw (torch _weight_norm_interface_backward). */
int rh_weight_norm_bwd_f32(const float* dw, const float* v, const float* g, const float* norms,
                           int64_t rows, int64_t cols, float* dv, float* dg, rh_stream_t stream);
/* The same for MANY weight tensors in ONE launch (one workgroup per row over the concatenated rows; table by value in the
 * kernel arguments, <= 64 tensors per launch): the weight-norm backward of every `normalization(conv)` of a backward pass
 * (rave/blocks.py:15-22) collected and run once -- same arithmetic and bits as rh_weight_norm_bwd_f32 per tensor. */
typedef struct rh_wn_bwd_item {
    const float* dw;
    const float* v;
    const float* g;
    const float* norms;
    float* dv;
    float* dg;
    int64_t rows;
    int64_t cols;
} rh_wn_bwd_item;
int rh_weight_norm_bwd_batched_f32(const rh_wn_bwd_item* items, int32_t n_items, rh_stream_t stream);
/* Batched reduction of the weight gradients' K-slice partials (round 6; the per-layer ordered reduction that follows every
 * split weight-gradient kernel -- 56 launches per v2 step -- collected over several layers into one launch, the same sums in the
 * same order).  rh_defer_reduce(item) arms the NEXT rh_conv1d_bwd_weight_f32 call of this thread (consumed by it, like
 * rh_x6_set_ranges): where that call would launch the reduction of its partials it leaves them in its workspace and fills *item
 * (part = the partials [Z][n] behind the bias scratch of the workspace, out = dw, n, Z > 1); item->Z = 0 when nothing is
 * pending (dw is complete).  The caller keeps workspace and dw alive until rh_reduce_partials_batched_f32 has run on the same
 * stream.  Reference site: the weight gradients autograd produces for every conv of rave/blocks.py:514-714 in
 * rave/model.py:288-344. */
typedef struct rh_reduce_item {
    const float* part;
    float* out;
    int64_t n;
    int32_t Z;
    int32_t reserved;
} rh_reduce_item;
int rh_defer_reduce(rh_reduce_item* item);
int rh_reduce_partials_batched_f32(const rh_reduce_item* items, int32_t n_items, rh_stream_t stream);

/* Number of floats of the two packed (MFMA-friendly, K-major) copies of a weight tensor:
 * which = 0 -> operand of rh_conv1d_fwd_f32, which = 1 -> operand of rh_conv1d_bwd_data_f32. */
int64_t rh_conv1d_packed_floats(const rh_conv1d_desc* d, int which);
/* Repack w (PyTorch layout, see rh_conv1d_desc) into wp_fwd and/or wp_bwd (either may be NULL). */
int rh_conv1d_pack_f32(const rh_conv1d_desc* d, const float* w, float* wp_fwd, float* wp_bwd,
                       rh_stream_t stream);

/* Weight norm folded into the repack: v (PyTorch weight layout), g (dim-0 gains) -> norms[r] = ||v[r]||,
 * scale[r] = g[r]/norms[r] (both `rows` floats, rows = dim 0 of v) and the packed copies of
 * w = g v/||v||, without materialising w.  Replaces `normalization(cc.Conv1d(...))`
 * (rave/blocks.py:15-22) on the forward path; the gradient goes through rh_weight_norm_bwd_f32. */
int rh_conv1d_pack_wn_f32(const rh_conv1d_desc* d, const float* v, const float* g, float* norms,
                          float* scale, float* wp_fwd, float* wp_bwd, rh_stream_t stream);

/* Batched form of rh_conv1d_pack_wn_f32 for a whole model: the caller fills one opaque item per
 * weight-normalised conv (host memory, rh_prep_item_bytes() each, pointers are DEVICE pointers to the
 * parameters and to persistent norms / scale / packed buffers; the array is rh_prep_array_bytes(n) long: the items and,
 * behind them, two compact lookup tables rh_prep_link writes), links them, copies the array to the
 * device once, and then refreshes every layer's packed weights with three launches (range clear, scales, pack) per training step. */
int64_t rh_prep_item_bytes(void);
int64_t rh_prep_array_bytes(int32_t n);
/* (rh_prep_fill_item: `scale` must hold 3 * rows floats -- the scales, then the per-row max |w| and sum |w| the range
 * records of the f16 kernels are reduced from.) */
int rh_prep_fill_item(const rh_conv1d_desc* d, const float* v, const float* g, float* norms, float* scale,
                      float* wp_fwd, float* wp_bwd, void* item_host);
int rh_prep_link(void* items_host, int32_t n, int64_t* total_rows, int64_t* total_blocks);
int rh_prep_run_f32(const void* items_dev, int32_t n, int64_t total_rows, int64_t total_blocks, rh_stream_t stream);

/* ---- convolution ---------------------------------------------------------------------- */

/* y = conv(act(x)) + bias + residual.   bias (c_out), residual (B,c_out,l_out*inner) and
 * snake_alpha (c_in) may be NULL.  Replaces `act -> cc.Conv1d -> (+ x)` of DilatedUnit /
 * Residual (rave/blocks.py:31-45,83-112) and every other `activation; conv` pair of
 * EncoderV2 / GeneratorV2 / discriminator.ConvNet. */
int rh_conv1d_fwd_f32(const rh_conv1d_desc* d, const float* x, const float* wp_fwd,
                      const float* bias, const float* snake_alpha, const float* residual,
                      float* y, void* workspace, int64_t workspace_bytes, rh_stream_t stream);
/* Optional scratch for rh_conv1d_fwd_f32 / rh_conv1d_bwd_data_f32 (0 = none needed).  Geometries
 * whose output is too small to fill 256 CUs (short sequences x many channels) split the
 * reduction over (tap, input-channel) chunks across workgroups; the partial sums live in this
 * scratch and are combined in a fixed order (deterministic).  Passing NULL / too few bytes is
 * legal: the launch then runs unsplit (slower, same accumulation class). */
int64_t rh_conv1d_fwd_workspace_bytes(const rh_conv1d_desc* d);
int64_t rh_conv1d_bwd_data_workspace_bytes(const rh_conv1d_desc* d);
/* Which kernel family rh_conv1d_fwd_f32 (which = 0) / rh_conv1d_bwd_data_f32 (which = 1) would launch for this
 * geometry and operand set: 1 = exact f32 on the bf16 matrix cores (3-way split, conv_x6_kernel), 2 = the HBM-bound
 * vector-ALU kernels of the 1- / 2-channel first discriminator layers (conv_smallc.hip), 0 = f32-input MFMA kernels,
 * < 0 = invalid descriptor.  Measurement only (bench.py prices every launch against the peak of the
 * instruction it issues); has_bias / has_add = the optional operands are non-NULL. */
int rh_conv1d_kernel_family(const rh_conv1d_desc* d, int which, int has_bias, int has_add);
/* Fused Residual(DilatedUnit) forward -- y = conv_1x1(act(h), w1) + x, h = conv_k_dilated(act(x), w3) -- in ONE launch
 * (rave/blocks.py:31-45 `Residual`, :83-112 `DilatedUnit`; C = 32 / 64 / 96, stride 1, "same" padding, no biases).
 * d3 / d1 describe the two convolutions (act / act_slope = the activation in front of each), wp3_fwd / wp1_fwd are
 * their packed forward operands.  h: receives the intermediate for the backward pass, or NULL (inference: never
 * written).  Results are bit-identical to rh_conv1d_fwd_f32(d3) followed by rh_conv1d_fwd_f32(d1, residual = x).
 * wp3_fwd / wp1_fwd must be 16-byte aligned (x: 4-byte, as everywhere): RH_ERR_INVALID otherwise, nothing enqueued. */
int rh_residual_unit_fused(const rh_conv1d_desc* d3, const rh_conv1d_desc* d1);   /* 1 = the pair fits the fused launch */
int rh_residual_unit_fwd_f32(const rh_conv1d_desc* d3, const rh_conv1d_desc* d1, const float* x, const float* wp3_fwd,
                             const float* wp1_fwd, float* h, float* y, rh_stream_t stream);

/* ---- range slots of the f16 matrix-core kernels (round 6) ---------------------------------------------------------------
 * The "x6" kernels (conv_x6_kernel, unit_x6_kernel, wgrad_x6_kernel) compute exact-f32-class products on the f16 matrix cores:
 * every operand is scaled by a power of two that takes its TENSOR's largest magnitude into [2^14, 2^15) and split into two
 * f16 pieces (csrc/common.hpp).  The scale needs max |x| of each activation operand; it travels in a RANGE SLOT: an array of
 * rh_x6_range_words() uint32 in device memory (32 words in use, one per 128-byte line so that the producers' atomics do not
 * serialise; the rest stays zero), each the bit pattern of a non-negative float -- max |x| over the FINITE elements (NaN
 * and +-Inf are left out) is the largest word (any
 * upper bound within a factor of ~2^10 of it keeps f32 accuracy; a too SMALL value overflows f16: the slot must cover the
 * tensor).  rh_x6_set_ranges arms the slots of the NEXT rh_conv1d_fwd_f32 / rh_conv1d_bwd_data_f32 / rh_residual_unit_fwd_f32
 * / rh_conv1d_bwd_weight[_wn]_f32 / rh_conv2d_fwd_f32 / rh_conv2d_bwd_data_f32 / rh_conv2d_bwd_weight_f32 / rh_act_bwd_bias_f32
 * (out = the slot of g) / rh_pqmf_fold_k1_f32 / rh_reparam_fwd_f32 (out = the slot of their output) call of this thread (consumed by that call -- also when it fails validation --, like rh_set_kernel_events):
 *     in_a   weight gradient only: the slot of dy          in_b   the slot of the input activation (x; dy for bwd_data)
 *     out    where the call leaves max |output| (forward: y, bwd_data: dx; atomicMax, the caller zeroes it first) or NULL
 *     out2   rh_residual_unit_fwd_f32: the slot of the intermediate h, or NULL
 * A call whose input slot is NULL takes the f32-input MFMA kernels instead (same results to f32 rounding, slower).
 * rh_amax_f32 fills a (zeroed) slot from a tensor no kernel of this library produced.  rh_x6_uses_ranges() = 1 for this
 * build (0 = the bf16 x 6 comparison build, which ignores slots).  The weights' own range is recorded by the pack kernels
 * inside the packed operand.  Reference sites: every conv of rave/blocks.py:83-112,514-714 and rave/discriminator.py:77-119. */
int rh_x6_uses_ranges(void);
int rh_x6_range_words(void);
int rh_x6_set_ranges(const uint32_t* in_a, const uint32_t* in_b, uint32_t* out, uint32_t* out2);
int rh_amax_f32(const float* x, int64_t n, uint32_t* slot, rh_stream_t stream);

/* Diagnostics: out8 = {family, row tiles per wave, column tiles per wave, waves along the rows, K slices, input stride of the
 * fragment layout, virtual rows, workgroups} of the launch rh_conv1d_fwd_f32 (which = 0) / rh_conv1d_bwd_data_f32
 * (which = 1) would issue; zeros behind `family` for the non-bf16x6 families.  Lets the parity tests assert that the
 * benchmarked batch size runs other template instances than the small-batch tests. */
int rh_conv1d_plan_info(const rh_conv1d_desc* d, int which, int has_bias, int has_add, int32_t* out8);
/* Diagnostics (host only, nothing is launched): which INSTANCE of the f32-input MFMA kernels ("family 0") rh_conv1d_fwd_f32
 * (which = 0) / rh_conv1d_bwd_data_f32 (which = 1) would launch for a call with NO input range slot armed -- answered by the
 * planning code the launch itself runs.  has_bias / has_add = the optional operands are non-NULL; data_aligned16 = every data
 * pointer of the call (operands, packed weights, output, workspace) is 16-byte aligned (1) or only 4-byte aligned (0);
 * workspace_offered = a workspace of rh_conv1d_fwd_workspace_bytes / rh_conv1d_bwd_data_workspace_bytes is passed (1) or none (0).
 *   out24[0] = family: 0 = f32-input MFMA kernels, 2 = conv_smallc.hip (zeros behind it), 1 = the build's 16-bit kernels take
 *              the call without a slot (the three-bf16-piece comparison build only; zeros behind it), -1 = empty geometry
 *   family 0: {0, kernel (1 = conv_igemm_dma_kernel, 0 = conv_igemm_kernel), TM, TN, WM, WN,
 *              flags (bit 0 LEAKY, bit 1 VEC, bit 2 CTAIL, bit 3 = the DMA launch fell back to conv_igemm_kernel because its two
 *              stages exceed 160 KiB of LDS), ck, total K chunks, K slices, chunks per slice,
 *              finalize kernel (0 none, 1 splitk_finalize_kernel, 4 splitk_finalize4_kernel), nb, bnl, tiles_per_b, nphase, inner,
 *              pitch (floats of one staged row), segs (64-float segments of a staged row, DMA only), LDS bytes,
 *              grid x, grid y, grid z, the largest number of taps of one phase}
 * The planner reads RH_CONV_SPLIT_BELOW, RH_CONV_SPLIT_TARGET, RH_CONV_NOVEC and RH_CONV_STAGE_FLOATS once per process.
 * RH_ERR_UNSUPPORTED where the launch itself would refuse (conv_igemm_kernel's tile beyond 160 KiB of LDS). */
int rh_conv1d_f32_instance_info(const rh_conv1d_desc* d, int which, int has_bias, int has_add, int data_aligned16,
                                int workspace_offered, int32_t* out24);
/* Same question for rh_conv1d_bwd_weight_f32: 1 = wgrad_x6_kernel (bf16 matrix cores; for Conv1d it also produces the
 * bias gradient), 2 = first-layer vector-ALU kernel (weight + bias gradient in one pass), 0 = f32-input MFMA kernels. */
int rh_conv1d_bwd_weight_kernel_family(const rh_conv1d_desc* d);
/* Diagnostics for family 1: out4 = {waves per workgroup (4 = wgrad_x6_kernel; 3, 4, 6 or 9 with ONE workgroup tile over the
 * whole weight tensor = wgrad_x6_wide_kernel, whose workgroups == K slices), workgroups, K slices, 1 if the input is staged once
 * per position} of the launch rh_conv1d_bwd_weight_f32 would issue under the present RH_WGRAD_X6_* switches; zeros otherwise. */
int rh_conv1d_bwd_weight_plan_info(const rh_conv1d_desc* d, int32_t* out4);
/* Diagnostics (host only, nothing is launched): which kernel INSTANCE rh_conv1d_bwd_weight_f32 would launch now for this
 * descriptor, for dy / x pointers that are (1) or are not (0) 16-byte aligned and with (1) or without (0) both range slots
 * armed, under the present RH_WGRAD_X6_* switches -- answered by the planner and instance selection the launch itself runs.
 *   out16[0] = family (as rh_conv1d_bwd_weight_kernel_family; -1 = an empty or invalid geometry), then
 *   family 1: {1, wide, NW (wide) or tm, wm (0 = wide), AV, PART, PL, Z, steps_per_z, total_steps, workgroup-tile rows,
 *              workgroup-tile columns, steps_per_b, p8, chmax (both 0 without PL), row tiles * column tiles}
 *              = wgrad_x6_wide_kernel<NW, PL> or wgrad_x6_kernel<tm, wm, 4 / wm, AV, PART, PL>; a step is 32 positions
 *   family 0: {0, bm, bn, dma (1 = wgrad_dma_kernel, 0 = wgrad_kernel), vec, LeakyReLU operand (0 none, 1 R, 2 S), rk, Z,
 *              chunks_per_z, total_chunks, chunks_per_b, nc_max, activation of R, activation of S, waves, row tiles * column tiles}
 *   family 2: {2, 0 ...} (conv_smallc.hip) */
int rh_conv1d_bwd_weight_instance_info(const rh_conv1d_desc* d, int dy_aligned16, int x_aligned16, int ranges_armed,
                                       int32_t* out16);

/* dx = act'(x) * conv_bwd_data(dy) + add.   `x` is the forward input (needed when act != NONE),
 * `add` (B,c_in,l_in*inner) may be NULL (residual-branch gradient). */
int rh_conv1d_bwd_data_f32(const rh_conv1d_desc* d, const float* dy, const float* wp_bwd,
                           const float* x, const float* snake_alpha, const float* add, float* dx,
                           void* workspace, int64_t workspace_bytes, rh_stream_t stream);

/* Bytes of scratch rh_conv1d_bwd_weight_f32 needs for this geometry. */
int64_t rh_conv1d_workspace_bytes(const rh_conv1d_desc* d);
/* dw (PyTorch weight layout) = sum_{b,l} dy (x) act(x);  dbias (c_out, may be NULL) = sum dy.
 * Deterministic: split-K partials in `workspace`, then an ordered reduction. */
int rh_conv1d_bwd_weight_f32(const rh_conv1d_desc* d, const float* dy, const float* x,
                             const float* snake_alpha, float* dw, float* dbias, void* workspace,
                             int64_t workspace_bytes, rh_stream_t stream);
/* The same weight gradient pushed through torch._weight_norm's backward (rave/blocks.py:15-22: `normalization` =
 * weight_norm around every conv of the v2 / v3 generator; dim 0 = c_out for Conv1d, c_in for ConvTranspose1d):
 *   dg[r] = <dw[r,:], v[r,:]> / ||v[r,:]||,   dv = (g/||v||) (dw - v <dw,v>/||v||^2)
 * with `norms` = ||v[r,:]|| as the repack left them.  Where the K range was split, dv / dg come straight from the slice
 * partials in ONE launch when RH_WN_FUSED=1 (the summed weight gradient is never written; bitwise the same result as
 * rh_conv1d_bwd_weight_f32 + rh_weight_norm_bwd_f32 -- measured 3 % SLOWER on the v2 step, hence opt-in); otherwise dw
 * goes through `dw_scratch` (weight-sized, contents undefined on return) and the plain weight-norm backward kernel. */
int rh_conv1d_bwd_weight_wn_f32(const rh_conv1d_desc* d, const float* dy, const float* x, const float* snake_alpha,
                                const float* v, const float* g, const float* norms, float* dw_scratch, float* dv,
                                float* dg, float* dbias, void* workspace, int64_t workspace_bytes, rh_stream_t stream);
/* Diagnostics: how many times this process took the one-launch form above (tests assert that it really runs). */
int64_t rh_conv1d_bwd_weight_wn_fused_launches(void);

/* ---- PQMF (rave/pqmf.py CachedPQMF; M = n_band in {2, 4, 8, 16, 32}) ----------------------- */

/* 1 iff the four transforms below take this band count and this analysis kernel length (the last dimension of
 * forward_conv.weight): n_band in {2, 4, 8, 16, 32} and 1 <= kernel <= 40 * n_band (the launcher stages at most 40
 * polyphase taps; the designed banks have kernel = 32 * n_band + 1, i.e. 33 taps).  Every other band count makes the
 * entry points return RH_ERR_UNSUPPORTED.  16 runs on the MFMA kernels of pqmf.hip (and, from the Python layer, on the
 * folded fast form below); the others on the vector-ALU kernels of pqmf_bands.hip. */
int rh_pqmf_supported(int32_t n_band, int32_t kernel);
/* Frames one workgroup of the direct-form kernels produces for this band count (0: no kernel); tests place their lengths
 * around it. */
int rh_pqmf_tile_frames(int32_t n_band);

/* CachedPQMF.forward (rave/pqmf.py:279-283): strided Conv1d(1,M,K,stride=M,pad=(pad_left,*))
 * followed by reverse_half (:13-17).  x (rows, T) -> y (rows, M, n_frames) with
 * n_frames = (T + pad_left + pad_right - K)/M + 1.  w: forward_conv.weight (M,1,K). */
int rh_pqmf_analysis_fwd_f32(const float* x, const float* w, int32_t rows, int32_t t_len,
                             int32_t n_band, int32_t kernel, int32_t pad_left, int32_t n_frames,
                             float* y, rh_stream_t stream);
/* gradient of the above w.r.t. x. */
int rh_pqmf_analysis_bwd_f32(const float* dy, const float* w, int32_t rows, int32_t t_len,
                             int32_t n_band, int32_t kernel, int32_t pad_left, int32_t n_frames,
                             float* dx, rh_stream_t stream);
/* CachedPQMF.inverse (rave/pqmf.py:285-294): reverse_half, Conv1d(M,M,K2,pad=(pad_left,*)) * M,
 * band flip and interleave.  y (rows, M, n_frames) -> x (rows, n_out*M); n_out = n_frames +
 * pad_left + pad_right - K2 + 1.  w: inverse_conv.weight (M,M,K2). */
int rh_pqmf_synthesis_fwd_f32(const float* y, const float* w, int32_t rows, int32_t n_frames,
                              int32_t n_band, int32_t kernel, int32_t pad_left, int32_t n_out,
                              float* x, rh_stream_t stream);
/* gradient of the above w.r.t. y. */
int rh_pqmf_synthesis_bwd_f32(const float* dx, const float* w, int32_t rows, int32_t n_frames,
                              int32_t n_band, int32_t kernel, int32_t pad_left, int32_t n_out,
                              float* dy, rh_stream_t stream);

/* The same four transforms in the FOLDED fast form of the cosine-modulated bank (55.6 MAC/sample instead of 513;
 * rave/pqmf.py:32-52 get_qmf_bank + :245-294).  `tab` = 384 floats hs[tau] = (-1)^(tau/32) h[tau] (prototype
 * `pqmf.h`, zero padded) followed by the 16 x 32 matrix Cm[k][m] = 2 cos((2k+1) pi/32 (m - N/2) + (-1)^k pi/4).
 *   k1 (fold -> matrix):        out[row][k][n] = s(k,n) * scale * sum_m Cm[k][m] sum_j hs[m+32j] in[row][16n + m + 32j + o0]
 *   k2 (matrix -> overlap-add): out[row][q]    = scale * sum_n' hs[tau] * sum_c Cm[c][tau%32] s(c,n') in[row][c][n'],
 *                                                tau = q - 16 n' + dp in [0, 384)
 * with s = reverse_half's sign (-1 iff k odd and n even) and zero extension of `in`.  With lpad = (512 - len(h)) / 2:
 *   analysis forward   = k1(x,  o0 = lpad - pad_left, scale 1)        analysis backward  = k2(dy, dp = pad_left - lpad, 1)
 *   synthesis forward  = k2(y,  dp = 496 - 16 pad_left - lpad, 16)    synthesis backward = k1(dx, o0 = lpad - (496 - 16 pad_left), 16)
 * Valid only while forward_conv / inverse_conv hold the designed bank (the caller checks; they are never trained). */
int rh_pqmf_fold_k1_f32(const float* in, const float* tab, int32_t rows, int32_t t_len, int32_t n_frames, int32_t o0,
                        float scale, float* out, rh_stream_t stream);
int rh_pqmf_fold_k2_f32(const float* in, const float* tab, int32_t rows, int32_t n_frames, int32_t n_out, int32_t dp,
                        float scale, float* out, rh_stream_t stream);

/* ---- small fused elementwise ops ------------------------------------------------------- */

/* GeneratorV2 output head (rave/blocks.py:705-711): y = tanh(a * sigmoid(m)), with
 * x = [a | m] split on the channel axis: x (B, 2C, L) -> y (B, C, L). */
int rh_amp_tanh_fwd_f32(const float* x, int32_t batch, int32_t c, int32_t l, float* y,
                        rh_stream_t stream);
int rh_amp_tanh_bwd_f32(const float* dy, const float* x, int32_t batch, int32_t c, int32_t l,
                        float* dx, rh_stream_t stream);
/* Standalone activation (used where no conv follows). n = total elements, c/l for snake. */
int rh_act_fwd_f32(const float* x, const float* snake_alpha, int32_t act, float slope,
                   int32_t batch, int32_t c, int32_t l, float* y, rh_stream_t stream);
/* Snake backward (rave/blocks.py:852-860): dx and dalpha (c floats) from dy, x (B,c,l), alpha (c).
 * workspace: rh_snake_bwd_workspace_bytes(batch, c) bytes (ordered partial sums -> deterministic). */
int64_t rh_snake_bwd_workspace_bytes(int32_t batch, int32_t c);
int rh_snake_bwd_f32(const float* dy, const float* x, const float* alpha, int32_t batch, int32_t c,
                     int32_t l, float* dx, float* dalpha, void* workspace, int64_t workspace_bytes,
                     rh_stream_t stream);
/* g = dy * act'(y) for an OUTPUT LeakyReLU (sign(y) == sign(pre-activation)): the cotangent the backward
 * entry points of a conv with out_act expect. */
int rh_act_bwd_f32(const float* dy, const float* y, int32_t act, float slope, int64_t n, float* g, rh_stream_t stream);
/* One pass for the backward prologue of a conv with a LeakyReLU on its OUTPUT (rave/discriminator.py:50,
 * rave/descript_discriminator.py:27): g = dy * act'(y) and dbias[m] = sum over (batch, plane) of g, on (B, M, plane)
 * tensors; ordered partial sums (deterministic).  workspace: rh_act_bwd_bias_workspace_bytes(M) bytes.  With an output range
 * slot armed (rh_x6_set_ranges) the pass also leaves max |g| there. */
int64_t rh_act_bwd_bias_workspace_bytes(int32_t M);
int rh_act_bwd_bias_f32(const float* dy, const float* y, int32_t act, float slope, int32_t B, int32_t M, int64_t plane, float* g,
                        float* dbias, void* workspace, int64_t workspace_bytes, rh_stream_t stream);
/* AdaptiveInstanceNormalization in EVAL mode (rave/blocks.py:863-926; identity in training mode, :901-902).
 * stats_update = `mean = x.mean(-1); std = x.std(-1); update(mean_buf, mean, n); update(std_buf, std, n)` (:876-879, :904-909,
 * :915-920) on x (rows = batch * channels, l): per-row mean and unbiased standard deviation, then
 * buf[:rows] += (stat - buf[:rows]) / (num_updates[0] + 1); num_updates is the module's device buffer (the caller
 * increments it afterwards, as the reference does).  transfer = :887-895,
 * y = (x - mean_x) / (std_x + 1e-5) * std_y + mean_y with per-row statistics. */
int rh_adain_stats_update_f32(const float* x, int64_t rows, int32_t l, const float* num_updates, float* mean_buf,
                              float* std_buf, rh_stream_t stream);
int rh_adain_transfer_f32(const float* x, int64_t rows, int32_t l, const float* mean_x, const float* std_x,
                          const float* mean_y, const float* std_y, float* y, rh_stream_t stream);
/* nn.functional.avg_pool1d(x, 2) of MultiScaleDiscriminator (rave/discriminator.py:135). */
int rh_avgpool2_fwd_f32(const float* x, int64_t rows, int32_t l_in, float* y, rh_stream_t stream);
int rh_avgpool2_bwd_f32(const float* dy, int64_t rows, int32_t l_in, float* dx, rh_stream_t stream);

/* ---- general 2-D convolution (spectral / descript discriminators) ------------------------------ */

/*
 * torch.nn.Conv2d with zero padding on (B, C, H, W) tensors, W innermost, groups == 1, followed by the
 * LeakyReLU the reference puts right after it.  Replaces the Conv2d stacks of
 *   rave/discriminator.py:23-74  (rectified_2d_conv_block / EncodecConvNet: (9,3) kernels, stride (2,1),
 *                                 dilation (1,1|2|4); (3,3))
 *   rave/descript_discriminator.py:22-27,118-184 (WNConv2d; MRD: (3,9) stride (1,2) pad (1,4); (3,3))
 *   rave/descript_discriminator.py:30-66 (MPD: (5,1) stride (3,1) pad (2,0))
 *
 *   y[b,co,ho,wo] = act( bias[co] + sum_{ci,th,tw} w[co,ci,th,tw] * x[b,ci, ho*sh + th*dh - ph, wo*sw + tw*dw - pw] )
 *
 * `act` is applied to the OUTPUT (those networks keep the activated tensor as a feature map); the
 * backward entry points take y and apply act'(y) to dy on the fly (sign(y) == sign(pre-activation)
 * for a LeakyReLU with positive slope).  Only RH_ACT_NONE / RH_ACT_LEAKY.
 */
typedef struct rh_conv2d_desc {
    int32_t batch;
    int32_t c_in;
    int32_t c_out;
    int32_t h_in, w_in;
    int32_t h_out, w_out; /* must equal floor((in + 2*pad - dil*(k-1) - 1)/stride) + 1 */
    int32_t kh, kw;
    int32_t sh, sw;
    int32_t dh, dw;
    int32_t ph, pw;
    int32_t act;     /* enum rh_act on the output (NONE or LEAKY) */
    float act_slope;
} rh_conv2d_desc;

/* Packed weight sizes (floats): which = 0 forward operand, 1 data-gradient operand. */
int64_t rh_conv2d_packed_floats(const rh_conv2d_desc* d, int which);
/* w: (c_out, c_in, kh, kw) as torch.nn.Conv2d.weight; wp_bwd may be null. */
int rh_conv2d_pack_f32(const rh_conv2d_desc* d, const float* w, float* wp_fwd, float* wp_bwd, rh_stream_t stream);
int rh_conv2d_fwd_f32(const rh_conv2d_desc* d, const float* x, const float* wp_fwd, const float* bias /* may be null */,
                      float* y, rh_stream_t stream);
/* dx = conv2d^T(dy * act'(y)); y may be null when act == RH_ACT_NONE. */
int rh_conv2d_bwd_data_f32(const rh_conv2d_desc* d, const float* dy, const float* y, const float* wp_bwd, float* dx,
                           rh_stream_t stream);
/* Diagnostics (tests): kernel family and tile plan of a forward (which = 0) / data-gradient (1) launch.
 * out[16] = {family: 0 f32-input MFMA, 1 bf16x6 (conv2d_x6.hip), 2 vector ALU (conv2d_smallm.hip: <= 4 output rows); tm; tn; conversion tasks per thread; TR; TQ; nb; LDS bytes;
 *            workgroups; PH; PW; P (patch positions); largest tap offset in the patch; phases; row tiles; column tiles} */
int rh_conv2d_plan_info(const rh_conv2d_desc* d, int32_t which, int64_t* out);
/* Diagnostics (host only, nothing is launched): which kernel INSTANCE rh_conv2d_fwd_f32 (which = 0), rh_conv2d_bwd_data_f32 (1) or
 * rh_conv2d_bwd_weight_f32 (2) would launch now for this descriptor (its `act` included: a backward call with act != NONE takes the
 * fused-derivative paths), given what a descriptor cannot carry -- range slots armed (1) or not (0); the activation pointers 16-byte
 * aligned (1) or only 4-byte aligned (0); the same for the packed operand; the bytes of workspace offered to the weight gradient
 * (ignored for which < 2) -- under the switches that are read at every call (RH_CONV2D_X6, RH_CONV2D_SMALLM, RH_CONV_X6,
 * RH_WGRAD2D_X6; RH_WGRAD_X6, the switch of the 1-D weight gradient, also turns wgrad2d_x6_kernel off and is read per call too).
 * Answered by the selection and planning code the launch itself runs.  out[24]:
 *   out[0]  kernel: 0 conv2d_x6_kernel, 1 conv2d_dma_kernel, 2 conv2d_igemm_kernel, 3 conv2d_smallm_kernel,
 *           4 conv2d_smallc_fwd_kernel, 5 wgrad2d_x6_kernel, 6 wgrad2d_dma_kernel, 7 wgrad2d_kernel; -1 = an empty batch
 *   out[1..4] template arguments: x6 {TM, TN, NQ}; dma / igemm / wgrad2d {TM, TN, WM, WN}; smallm {KH, MM, FLIP}; smallc {KH};
 *           wgrad2d_x6 {NQX, SW}; wgrad2d_dma {TN}
 *   convolutions (which < 2): out[5..] = {TR, TQ, nb, PH, PW, ck (channels per staged chunk), phases, grid x, grid y, grid z,
 *           LDS bytes, row tiles, column tiles, family as rh_conv2d_plan_info, for conv2d_igemm_kernel why conv2d_dma_kernel did not
 *           take the call: 1 fused derivative, 2 a tensor of 2 GB, 3 the patch exceeds the DMA slots even at TR = 1 and TQ = 16,
 *           4 LDS, 5 grid, 6 RH_CONV2D_NODMA}
 *   weight gradient: out[5..] = {TR (x6) or rk, TQ (x6) or wk, Z, chunks_per_z (0 for x6), channel groups (x6) or workgroup tiles,
 *           nc_max (x6: channels of the fullest group), LDS bytes, workspace bytes the launch uses behind the bias scratch (0 when
 *           Z == 1), bytes of bias scratch in front, tiles (x6) or chunks in all, PH, patch pitch, 0, family as
 *           rh_conv2d_bwd_weight_kernel_family, 1 = the workspace offered is too small for this launch: the call fails} */
int rh_conv2d_instance_info(const rh_conv2d_desc* d, int32_t which, int32_t ranges_armed, int32_t data_aligned16,
                            int32_t packed_aligned16, int64_t workspace_bytes, int64_t* out24);
/* 1 = rh_conv2d_bwd_weight_f32 runs this geometry (act == NONE) on the bf16 matrix cores (wgrad2d_x6.hip), else 0. */
int rh_conv2d_bwd_weight_kernel_family(const rh_conv2d_desc* d);
int64_t rh_conv2d_workspace_bytes(const rh_conv2d_desc* d);
/* dw (c_out, c_in, kh, kw), dbias (c_out) or null; deterministic (ordered split-K partials in `workspace`). */
int rh_conv2d_bwd_weight_f32(const rh_conv2d_desc* d, const float* dy, const float* y, const float* x, float* dw,
                             float* dbias, void* workspace, int64_t workspace_bytes, rh_stream_t stream);

/* ---- residual vector quantisation ------------------------------- */

/* One EuclideanCodebook step (rave/quantization.py:131-181) on n_vectors x dim row-major vectors:
 * indices[n] = argmin_k (|x_n|^2 - 2 x_n.e_k) + |e_k|^2 (first index on ties, as torch.max of the negated
 * distance); residual[n] = x_n - e_ind (input of the next quantiser, ResidualVectorQuantization.forward
 * :283-300; may alias x; may be null); quantized_sum[n] += e_ind (may be null);
 * loss_partials[rh_vq_loss_partials(n_vectors)] = per-block sums of |e_ind - x_n|^2 (commitment loss
 * numerator, :263-266; may be null). */
int64_t rh_vq_loss_partials(int64_t n_vectors);
int rh_vq_assign_f32(const float* x, const float* embed, int64_t n_vectors, int32_t dim, int32_t codebook_size,
                     int64_t* indices, float* residual, float* quantized_sum, float* loss_partials, rh_stream_t stream);
/* The same step with caller-provided scratch: with rh_vq_assign_workspace_bytes(...) > 0 bytes of it the distance search
 * (rave/quantization.py:131-136) runs on the f32 matrix cores -- the same fmaf chains, hence the same distances, indices
 * and loss partials as the one-launch kernel -- in two launches; 0 bytes / NULL = rh_vq_assign_f32 (residual may alias x
 * on either path). */
int64_t rh_vq_assign_workspace_bytes(int64_t n_vectors, int32_t dim, int32_t codebook_size);
int rh_vq_assign_ws_f32(const float* x, const float* embed, int64_t n_vectors, int32_t dim, int32_t codebook_size,
                        int64_t* indices, float* residual, float* quantized_sum, float* loss_partials, void* workspace,
                        int64_t workspace_bytes, rh_stream_t stream);
/* Training-time codebook update (:165-179): cluster_size / embed_avg EMAs from per-code counts and ordered
 * vector sums (deterministic), then embed = embed_avg / (laplace_smoothing(cluster_size) * sum). */
int rh_vq_ema_update_f32(const float* x, const int64_t* indices, int64_t n_vectors, int32_t dim, int32_t codebook_size,
                         float decay, float epsilon, float* cluster_size, float* embed_avg, float* embed,
                         rh_stream_t stream);

/* ---- training data feed (SURVEY.md section 8f "next" #4) --------------------------------------------- */

/* One minibatch of the reference's per-item CPU chain (rave/dataset.py:75-78,218-229,246,283-299;
 * rave/transforms.py:96-115) in one launch: for every row r (one channel of one clip)
 *   x = float32(pcm[src_offset[r] + n]) / 32767                                   n < n_signal   (crop applied by the offset)
 *   y = lfilter([b0,b1,b2], [1,a1,a2], x) in float64 (direct form II transposed)  if coef[r][0] is not NaN
 *   out[r][n] = float32(y + noise[r][n] / 2^bit_depth)
 * coef: rows x 5 doubles (b0, b1, b2, a1, a2), b0 = NaN skips the filter (RandomApply miss); noise: U[0,1) floats.
 * The random draws (item, crop point, pole angle, noise) belong to the caller. */
int rh_feed_batch_i16_f32(const int16_t* pcm, const int64_t* src_offset, const double* coef, const float* noise,
                          int32_t rows, int32_t n_signal, int32_t bit_depth, float* out, rh_stream_t stream);

/* The same chain with the two augmentations the reference applies per item around it: RandomPitch in front of the crop
 * (`rave train --rand_pitch lo,hi`: scripts/train.py:67,169, rave/dataset.py:233-236, rave/transforms.py:56-89 =
 * scipy.signal.resample_poly(item, up, down, padtype='mean') of the whole stored item) and RandomMute behind Dequantize
 * (rave/transforms.py:168-177, rave/configs/augmentations/mute.gin).  For every row r, with up / down reduced by their gcd,
 * m = max(up, down), H = 10 m, h = the 2H + 1 doubles at taps[tap_offset] (= up * firwin(2H + 1, 1 / m, ('kaiser', 5.0))),
 * x[k] = float32(pcm[base + k]) / 32767 for k < length and n_out = ceil(length * up / down):
 *   p[n] = float32(mean + sum_k h[n down - k up + H] (x[k] - mean)),  k in [ceil((n down - H) / up), floor((n down + H) / up)]
 *          and [0, length), accumulated in float64                    n in [in_point, in_point + n_signal)
 *   y    = lfilter(coef, p) in float64 if coef[0] is not NaN;  out[r][i] = float32(y[i] + noise[r][i] / 2^bit_depth)
 * A row with up == down is not resampled (p = x, bit-identical to rh_feed_batch_i16_f32 at src_offset = base + in_point);
 * a row with mute != 0 is all zeros.  `mean` is the mean of x over the whole item row (padtype='mean').
 * `rows` is the table in HOST memory, checked here: up, down in 1..19, the item inside pcm[0, pcm_samples), the window
 * inside [0, n_out), the taps inside taps[0, n_taps) -- RH_ERR_INVALID and no launch otherwise.  `rows_dev` is the caller's
 * copy of the same table in device memory, which the kernel reads; pcm, taps, noise and out are device memory. */
typedef struct rh_feed_pitch_row {
    int64_t base;       /* offset of the item row (one channel of one item) in pcm, in samples */
    int64_t in_point;   /* crop point, in resampled samples */
    double mean;
    double coef[5];     /* b0, b1, b2, a1, a2; b0 = NaN skips the all-pass */
    int32_t length;     /* samples of the stored item row */
    int32_t up, down;
    int32_t tap_offset; /* first tap of this row's ratio in `taps` (unused when up == down) */
    int32_t mute;
    int32_t reserved;
} rh_feed_pitch_row;
int rh_feed_batch_pitch_i16_f32(const int16_t* pcm, int64_t pcm_samples, const rh_feed_pitch_row* rows,
                                const rh_feed_pitch_row* rows_dev, const double* taps, int32_t n_taps, const float* noise,
                                int32_t n_rows, int32_t n_signal, int32_t bit_depth, float* out, rh_stream_t stream);

/* The chain of rh_feed_batch_pitch_i16_f32 with the two steps `rave train --normalize` / `--derivative` put between
 * Dequantize and the augmentations (scripts/train.py:61-63,160-167, rave/dataset.py:241-245).  With v[r][i] = y[i] +
 * noise[r][i] / 2^bit_depth in float64 (the value the pitched entry point rounds to float32), rows r of one item being
 * n_channels consecutive rows:
 *   normalize  != 0: peak = max |v| over ALL rows and samples of the item (normalize_signal, rave/dataset.py:196-204);
 *                    gain = 1 if peak == 0, else 10^(min(max_gain_db, -20 log10(peak)) / 20);  otherwise gain = 1
 *   derivative != 0: out[r][i] = float32(0.5 v[r][i] gain - 0.5 v[r][i - 1] gain), v[r][-1] = 0   (lfilter([.5, -.5], [1], .)
 *                    in float64, rave/dataset.py:24-29);  otherwise out[r][i] = float32(v[r][i] gain)
 * all in float64 with ONE rounding to float32 at the end; a row with mute != 0 is all zeros and adds nothing to the peak.
 * Two launches on `stream`: the chain kernel leaves v and one peak per row in `workspace` (rh_feed_post_workspace_bytes
 * bytes, 8-byte aligned device memory owned by the caller, free for reuse once the call's work on the stream is done), the
 * second applies gain, difference and rounding; the peaks are reduced by max in a fixed order, the result is the same bits
 * on every run.  normalize == 0 && derivative == 0 is rh_feed_batch_pitch_i16_f32 (same bits; workspace may be NULL).
 * Checked on the host, RH_ERR_INVALID and no launch otherwise: everything rh_feed_batch_pitch_i16_f32 checks,
 * n_rows % n_channels == 0, max_gain_db finite, the size and alignment of the workspace. */
int64_t rh_feed_post_workspace_bytes(int32_t n_rows, int32_t n_signal);
int rh_feed_batch_post_i16_f32(const int16_t* pcm, int64_t pcm_samples, const rh_feed_pitch_row* rows,
                               const rh_feed_pitch_row* rows_dev, const double* taps, int32_t n_taps, const float* noise,
                               int32_t n_rows, int32_t n_signal, int32_t bit_depth, int32_t n_channels, int32_t normalize,
                               double max_gain_db, int32_t derivative, void* workspace, int64_t workspace_bytes, float* out,
                               rh_stream_t stream);

/* The chain of rh_feed_batch_post_i16_f32 with the Resample the reference puts right behind Dequantize when the stored
 * dataset's rate differs from the run's (rave/dataset.py:238-239, rave/transforms.py:31-40:
 * torchaudio.functional.resample(x.float(), orig_freq, new_freq) with its defaults -- sinc_interp_hann, lowpass_filter_width 6,
 * rolloff .99 -- on the cropped item).  With o, n = orig_freq, new_freq over their gcd, width = ceil(6 o / (.99 min(o, n))),
 * K = 2 width + o, h = res_taps, the float32 (n, K) table of torchaudio's _get_sinc_resample_kernel (rave_amd/data.py:
 * sinc_resample_kernel), and v the float64 row behind Dequantize (rh_feed_batch_post_i16_f32):
 *   y[r][q n + i] = float32(sum_{k < K} h[i][k] xpad[q o + k]),  xpad[m] = float32(v[r][m - width]) inside [0, n_signal), else 0,
 *                   summed in float64 in ascending k                         q n + i < n_res = ceil(n n_signal / o)
 * normalize / derivative then act on the rows y of n_res samples exactly as rh_feed_batch_post_i16_f32 describes for v, and
 * `out` is (n_rows, n_res); a row with mute != 0 is all zeros and adds nothing to the peak.  The all-pass in `rows` keeps the
 * dataset's rate; noise is (n_rows, n_signal).
 * Two or three launches on `stream`: the chain kernel leaves v and its peaks in `workspace`, the resampling kernel writes `out`
 * (both steps off) or y as doubles and max |y| per row into a second region of it, the kernel of the post entry point finishes.
 * No atomics, one writer and one order of operations per sample: the same bits on every run.  `workspace`:
 * rh_feed_resample_workspace_bytes bytes (negative: bad arguments), 8-byte aligned device memory owned by the caller.
 * orig_freq == new_freq is rh_feed_batch_post_i16_f32 (same bits; res_taps, n_res_taps and width are not looked at, and the
 * workspace is the one of that entry point).
 * Checked on the host, RH_ERR_INVALID and no launch otherwise: everything rh_feed_batch_post_i16_f32 checks; orig_freq,
 * new_freq >= 1; `width` and n_res_taps == n K against the expression above recomputed in double; K <= 8192 (kResSpan) and
 * n <= 6144 (kResOut), what one pass of the kernel stages in LDS -- every pair of the rates 16000 .. 96000 in common use fits
 * (largest K 694 at 96000 -> 22050, largest n 640 and largest table, 1.16 MB, at 22050 -> 32000); n_res and K inside int32; the size and alignment of the workspace. */
int64_t rh_feed_resample_workspace_bytes(int32_t n_rows, int32_t n_signal, int32_t orig_freq, int32_t new_freq);
int rh_feed_batch_resample_i16_f32(const int16_t* pcm, int64_t pcm_samples, const rh_feed_pitch_row* rows,
                                   const rh_feed_pitch_row* rows_dev, const double* taps, int32_t n_taps, const float* noise,
                                   int32_t n_rows, int32_t n_signal, int32_t bit_depth, int32_t n_channels, int32_t normalize,
                                   double max_gain_db, int32_t derivative, int32_t orig_freq, int32_t new_freq,
                                   const float* res_taps, int64_t n_res_taps, int32_t width, void* workspace,
                                   int64_t workspace_bytes, float* out, rh_stream_t stream);

/* FrequencyMasking (rave/transforms.py:180-195) on finished float32 rows, one launch: row r of x (n_rows, n_signal) with
 * bands[2r] = first_bin, bands[2r + 1] = n_bins loses the bins [first_bin, first_bin + n_bins) of
 * scipy.signal.stft(x, nperseg = 4096) -- periodic Hann w, hop 2048, boundary = 'zeros', 2049 bins -- and is rebuilt by
 * scipy.signal.istft.  Computed as x minus the band component: with xpad_t the frame t of the zero-padded row (the samples
 * [2048 (t - 1), 2048 (t + 1)) of x), B the indicator of the band and h_t = irfft(B . rfft(w . xpad_t)),
 *   y[2048 b + j] = x[2048 b + j] - (w[j] h_{b+1}[j] + w[j + 2048] h_b[j + 2048]) / (w[j]^2 + w[j + 2048]^2),   0 <= j < 2048
 * in float32 (the 4096-point real transforms run as 2048-point complex ones in LDS); every sample has one writer and one order
 * of operations: the same bits on every run.  A row with n_bins <= 0 is copied bit for bit (the reference returns such an item
 * itself); a band is clamped to the bins 0..2047 (the reference never masks the Nyquist bin).  `bands` is device memory and is
 * not checked here: the caller validates its draws.  twiddle: e^{-2 pi i k / 4096}, k < 4096, interleaved re, im, 8-byte
 * aligned (the table of rh_stft_loss_fwd_f32 for n_fft = 4096).  x and y must not overlap.
 * Checked on the host, RH_ERR_INVALID and no launch otherwise: null pointers, n_rows <= 0, n_signal < 4096 or not a multiple
 * of 2048 (lengths scipy would pad or shorten nperseg for), a misaligned table, overlapping x and y. */
int rh_feed_freq_mask_f32(const float* x, float* y, const int32_t* bands, int32_t n_rows, int32_t n_signal,
                          const float* twiddle, rh_stream_t stream);

/* ---- spectral distance ("next" item #1 of SURVEY.md section 8f, beside the hot path) ------------- */

/* STFT framing of torchaudio.transforms.Spectrogram(center=True, pad_mode="reflect") as used by
 * MultiScaleSTFT (rave/core.py:269-319): frames (rows, n_frames, n_fft) = window * reflect-padded x,
 * n_frames = t_len / hop + 1; and its adjoint (gradient w.r.t. x).  The FFT stays on rocFFT. */
int rh_stft_frame_fwd_f32(const float* x, const float* window, int64_t rows, int32_t t_len, int32_t n_fft,
                          int32_t hop, int32_t n_frames, float* frames, rh_stream_t stream);
int rh_stft_frame_bwd_f32(const float* dframes, const float* window, int64_t rows, int32_t t_len, int32_t n_fft,
                          int32_t hop, int32_t n_frames, float* dx, rh_stream_t stream);
/* the same with accumulate != 0: dx += ... (the scales of MultiScaleSTFT, rave/core.py:269-319, add up in place) */
int rh_stft_frame_bwd_acc_f32(const float* dframes, const float* window, int64_t rows, int32_t t_len, int32_t n_fft,
                              int32_t hop, int32_t n_frames, float* dx, int32_t accumulate, rh_stream_t stream);

/* AudioDistanceV1 on one STFT scale (rave/core.py:330-344) from two complex spectrograms (interleaved
 * re,im; n_complex elements each):  sums[0] = sum (|Sx|-|Sy|)^2, sums[1] = sum |Sx|^2,
 * sums[2] = sum |log(|Sx|+eps) - log(|Sy|+eps)|   =>   distance = sums[0]/sums[1] + sums[2]/n_complex.
 * The STFT itself stays on rocFFT.  workspace: rh_spectral_distance_workspace_bytes(). */
int64_t rh_spectral_distance_workspace_bytes(void);
int rh_spectral_distance_fwd_f32(const float* sx, const float* sy, int64_t n_complex, float eps, float* sums,
                                 void* workspace, int64_t workspace_bytes, rh_stream_t stream);
/* d distance / d Sx and / d Sy (either output may be NULL), scaled by the device scalar grad_out[0].
 * half_bins = 0: the plain gradients.  half_bins = n_fft/2+1 (spectra laid out (..., half_bins)): the interior
 * bins are halved, which makes the outputs the operand of the UNNORMALISED C2R transform that is the adjoint of
 * rfft -- d distance / d frames = irfft(dsx, n_fft, norm="forward") -- instead of autograd's zero-fill + copy +
 * C2C + real-part chain. */
int rh_spectral_distance_bwd_f32(const float* sx, const float* sy, const float* sums, const float* grad_out,
                                 int64_t n_complex, float eps, float* dsx, float* dsy, int32_t half_bins,
                                 rh_stream_t stream);

/* AudioDistanceV1.forward's sum over the scales (rave/core.py:336-344): out[0] = sum_s sums[3s]/sums[3s+1] + sums[3s+2]*inv_n[s]
 * (sums: n_scales x 3 as written by rh_spectral_distance_fwd_f32, inv_n[s] = 1 / n_complex of scale s). */
int rh_spectral_total_f32(const float* sums, const float* inv_n, int32_t n_scales, float* out, rh_stream_t stream);

/* AudioDistanceV1 on one STFT scale (rave/core.py:269-344: Spectrogram(n_fft, hop = n_fft / 4, center, reflect) -> |.| ->
 * relative L2 + L1 of logs) with the transform INSIDE the kernel: x, y (rows, t_len) f32 waveforms, window (n_fft, the
 * normalised window the reference multiplies the frames by), twiddle (n_fft complex: e^{-2 pi i k / n_fft}, interleaved).
 * n_fft in {128, 256, 512, 1024, 2048}, hop = n_fft / 4, t_len > n_fft / 2 (rh_stft_loss_supported).  Same `sums` as
 * rh_spectral_distance_fwd_f32 (n_complex = rows * (t_len / hop + 1) * (n_fft / 2 + 1)); the backward recomputes the
 * spectra, and writes (accumulate = 0) or adds (!= 0) d distance / d x and / d y (either may be NULL) times grad_out[0]. */
int rh_stft_loss_supported(int32_t n_fft, int32_t hop, int32_t t_len, int64_t rows);
/* diagnostics: out6 = {frames per forward workgroup, forward workgroups per row, hop blocks per backward workgroup, backward
 * workgroups per row, hop blocks of the last backward workgroup, dynamic LDS bytes of the backward launch} */
int rh_stft_loss_plan_info(int32_t n_fft, int32_t t_len, int64_t rows, int64_t* out6);
int64_t rh_stft_loss_workspace_bytes(int32_t n_fft, int32_t t_len, int64_t rows);
int rh_stft_loss_fwd_f32(const float* x, const float* y, const float* window, const float* twiddle, int64_t rows,
                         int32_t t_len, int32_t n_fft, float eps, float* sums, void* workspace, int64_t workspace_bytes,
                         rh_stream_t stream);
/* sums == NULL above: the per-workgroup partials stay in `workspace` (rh_stft_loss_workspace_bytes of them) and ONE call
 * finalizes all scales of a distance: sums (n_scales x 3, as above) and total = sum_s sums[s][0] / sums[s][1] + sums[s][2] *
 * inv_n[s] (AudioDistanceV1 over MultiScaleSTFT, rave/core.py:269-344) -- one launch instead of n_scales + 1 between the
 * forward and the backward pass; same reduction order, same bits.  partials[s] / partial_bytes[s]: HOST arrays. */
int rh_stft_loss_finalize_all_f32(const float* const* partials, const int64_t* partial_bytes, int32_t n_scales,
                                  const float* inv_n, float* sums, float* total, rh_stream_t stream);
int rh_stft_loss_bwd_f32(const float* x, const float* y, const float* window, const float* twiddle, int64_t rows,
                         int32_t t_len, int32_t n_fft, float eps, const float* sums, const float* grad_out, float* dx,
                         float* dy, int32_t accumulate, rh_stream_t stream);

/* WeightedInstantaneousSpectralDistance on one STFT scale (rave/core.py:347-412 over MultiScaleSTFT(magnitude=False),
 * rave/core.py:269-319: Spectrogram(n_fft, hop = n_fft / 4, center, reflect, power=None) -> abs / log1p / angle -> unwrap ->
 * derivative -> optional mask -> the two means) with the transform INSIDE the kernel.  x = target, y = prediction, (rows, t_len)
 * f32, not overlapping any output; window (n_fft: the window the frames are multiplied by, `normalized` folded in); twiddle:
 * n_fft complex FLOAT64 values e^{-2 pi i k / n_fft}, interleaved, 16-byte aligned (the transform runs in f64: a phase is as
 * wrong as the transform's error over |bin|).  Supported: n_fft in {128 ... 2048}, hop = n_fft / 4, t_len > n_fft / 2
 * (rh_inst_freq_loss_supported: the set of rh_stft_loss_supported).  frames = t_len / hop + 1, bins = n_fft / 2 + 1.
 *   sums[4] = sum (a-b)^2, sum a^2, sum |log1p a - log1p b| over rows x bins x frames (a = |X|, b = |Y|), and
 *             sum (m IFx - m IFy)^2 over rows x bins x (frames - 2), IF[j] = wrap(phi[j+2] - phi[j+1]) along the FRAMES,
 *             wrap(d) = ((d + pi) mod 2 pi) - pi in f32 with torch.remainder's sign; m = clip(log1p a[j+2], 0, 1) (weighted != 0:
 *             the mask comes from the target) or 1.  The reference's cumsum-then-diff cancels and is not computed.
 *   Sum order: per workgroup (a span of frames of one row, walked in order; one more frame to its left is transformed for its
 *   phases) a fixed tree; the partials lie in (row, workgroup) order in `workspace` (rh_inst_freq_loss_workspace_bytes) and
 *   rh_inst_freq_loss_finalize_all_f32 adds them in a fixed order for ALL scales in one launch: sums (n_scales x 4),
 *   out2[0] = sum_s sums[s][0] / sums[s][1] + sums[s][2] * inv_n[2s] (spectral_distance), out2[1] = sum_s sums[s][3] *
 *   inv_n[2s+1] (phase_distance); inv_n: DEVICE array, 1 / (rows bins frames) and 1 / (rows bins (frames - 2)) per scale;
 *   partials[s] / partial_bytes[s]: HOST arrays.  No atomics: the bits are reproducible; every launch can be captured.
 *   Exact by construction: (1) bins 0 and n_fft / 2 have an imaginary part of exactly +0, phases 0 or pi, and IF exactly 0
 *   or -pi (wrap maps +pi and -pi to -pi, as the reference's f32 arithmetic); (2) a bin that is exactly zero has phase 0
 *   (torch.angle), so a silent row has IF = 0 and a zero gradient.
 *   if_out (diagnostics, may be NULL): (rows, 2, bins, frames - 2) -- the unweighted IF of x and of y.
 * Backward: recomputes the spectra; grad_out2 = 2 DEVICE scalars (d / d spectral_distance, d / d phase_distance), sums = the
 * 4 sums of THIS scale; writes (accumulate = 0) or adds (!= 0) dx and dy (either may be NULL).  d angle / d (re, im) =
 * (-im, re) / |z|^2, 0 at z = 0; wrap has derivative 1; the mask sends a gradient to x where log1p a <= 1. */
int rh_inst_freq_loss_supported(int32_t n_fft, int32_t hop, int32_t t_len, int64_t rows);
int64_t rh_inst_freq_loss_workspace_bytes(int32_t n_fft, int32_t t_len, int64_t rows);
int rh_inst_freq_loss_fwd_f32(const float* x, const float* y, const float* window, const double* twiddle, int64_t rows,
                              int32_t t_len, int32_t n_fft, int32_t weighted, float* if_out, void* workspace,
                              int64_t workspace_bytes, rh_stream_t stream);
int rh_inst_freq_loss_finalize_all_f32(const float* const* partials, const int64_t* partial_bytes, int32_t n_scales,
                                       const float* inv_n, float* sums, float* out2, rh_stream_t stream);
int rh_inst_freq_loss_bwd_f32(const float* x, const float* y, const float* window, const double* twiddle, int64_t rows,
                              int32_t t_len, int32_t n_fft, int32_t weighted, const float* sums, const float* grad_out2,
                              float* dx, float* dy, int32_t accumulate, rh_stream_t stream);

/* The mel-spectrogram encoder input of RAVE.input_mode = "mel" (rave/model.py:238-242: `spectrogram(x)[..., :-1]`, log1p,
 * reshape; spectrogram = torchaudio.transforms.MelSpectrogram as configs/hybrid.gin binds it) in one launch, forward only
 * (nothing trainable is upstream of the audio).  x (rows, t_len) f32; window (n_fft: the module's `spectrogram.window`);
 * twiddle as for rh_stft_loss_fwd_f32 (8-byte aligned); fb (n_fft / 2 + 1, n_mels: the module's `mel_scale.fb`); bins
 * (n_mels, 2) int32: filter m is zero outside the bins [bins[2m], bins[2m+1]) (clamped to [0, n_fft / 2 + 1] by the kernel).
 *   y[row][m][f] = g(sum_k fb[k][m] * |rfft(window * frame_f)_k|^2 * scale),   g = log1p (log1p != 0) or the identity,
 * frame_f = the n_fft samples centred on f * hop of the reflect-padded row; scale = 1 / sum(window^2) for `normalized=True`,
 * else 1.  n_frames = t_len / hop (the reference drops the last frame) or t_len / hop + 1 (all of torchaudio's frames).
 * y is (rows, n_mels, n_frames): with rows = B * n_channels a reshape gives the encoder's (B, n_channels * n_mels, frames).
 * Sizes (rh_mel_supported answers 1 / 0): n_fft in {128, 256, 512, 1024, 2048}, 1 <= hop <= n_fft, 1 <= n_mels <= 128,
 * t_len > n_fft / 2, t_len >= hop, 0 < rows < 65536 -- anything else is RH_ERR_UNSUPPORTED; null pointers, a misaligned
 * twiddle table, another n_frames and a scale that is not positive and finite are RH_ERR_INVALID; nothing is enqueued in
 * any of these cases.  Every sum has one fixed order (no atomics): results are bit-identical from run to run. */
int rh_mel_supported(int32_t n_fft, int32_t hop, int32_t n_mels, int32_t t_len, int64_t rows);
int rh_mel_fwd_f32(const float* x, const float* window, const float* twiddle, const float* fb, const int32_t* bins,
                   int64_t rows, int32_t t_len, int32_t n_fft, int32_t hop, int32_t n_mels, int32_t n_frames, float scale,
                   int32_t log1p, float* y, rh_stream_t stream);

/* The mel spectrogram WITH its gradient with respect to the audio: the spectrum of the Encodec-style loss,
 * core.SpectralDistance(mel = n) (rave/core.py:458-468: torchaudio.transforms.MelSpectrogram(sr, n_fft, hop_length = n_fft / 4,
 * n_mels, power, normalized, center=False), applied to both signals at rave/core.py:484-485), one launch per direction.
 * x, window, twiddle, fb and bins as for rh_mel_fwd_f32; center = 1: frames centred on f * hop of the reflect-padded row,
 * frames = t_len / hop + 1; center = 0: frame f is x[f hop, f hop + n_fft), frames = (t_len - n_fft) / hop + 1.
 *   mel[row][m][f] = sum_k fb[k][m] * |scale * rfft(window * frame_f)_k|^power,   power 1 or 2,
 * scale = 1 / sqrt(sum(window^2)) for `normalized=True`, else 1 (NOT its square: rh_mel_fwd_f32 takes 1 / sum(window^2)).
 * rh_mel_diff_fwd_f32 (replaces torchaudio's MelSpectrogram.forward at rave/core.py:484-485) is rh_mel_fwd_f32's kernel with
 * these two switches; rh_mel_diff_bwd_f32 (replaces autograd through torch.stft, abs / pow and the filterbank product at the
 * same site) gives dx (rows, t_len) from dmel (laid out as mel) and x: a workgroup owns a span of dx, recomputes the spectrum S
 * of every frame that covers it, forms dP[k] = sum_m fb[k][m] dmel[m] over the filters whose bin range holds k, the
 * spectrum's cotangent 2 scale^2 S dP (power 2) or scale S / |S| dP (power 1; exactly 0 where |S| = 0, torch's abs at 0: a
 * silent row gives zeros, never NaN), the transposed real DFT, the window and the overlap-add with the reflected edges folded
 * back.  No workspace, no atomics, one writer and one fixed order of additions per sample: bit-identical from run to run;
 * samples that no frame covers (the uncentred tail) get 0.  Frames ride the transforms two by two, always two of the SAME row.
 * Sizes (rh_mel_diff_supported answers 1 / 0; a host function): n_fft a power of two in 128 .. 2048, 1 <= hop <= n_fft,
 * 1 <= n_mels <= 128, power in {1, 2}, center in {0, 1}, t_len >= n_fft (center = 0) or t_len > n_fft / 2 (center = 1),
 * t_len <= 2^30, 0 < rows < 65536 -- anything else is RH_ERR_UNSUPPORTED; null pointers, a misaligned twiddle table and a
 * scale that is not positive and finite are RH_ERR_INVALID; nothing is enqueued in any of these cases.  x, mel, dmel and dx
 * need only be 4-byte aligned. */
int rh_mel_diff_supported(int32_t n_fft, int32_t hop, int32_t n_mels, int32_t t_len, int64_t rows, int32_t center,
                          int32_t power);
int rh_mel_diff_fwd_f32(const float* x, const float* window, const float* twiddle, const float* fb, const int32_t* bins,
                        int64_t rows, int32_t t_len, int32_t n_fft, int32_t hop, int32_t n_mels, int32_t center, int32_t power,
                        float scale, float* mel, rh_stream_t stream);
int rh_mel_diff_bwd_f32(const float* dmel, const float* x, const float* window, const float* twiddle, const float* fb,
                        const int32_t* bins, int64_t rows, int32_t t_len, int32_t n_fft, int32_t hop, int32_t n_mels,
                        int32_t center, int32_t power, float scale, float* dx, rh_stream_t stream);

/* The plain SpectralDistance of the Encodec-style loss on one STFT scale (rave/core.py:446-490 without `mel`: torchaudio
 * Spectrogram(n_fft, hop = n_fft / 4, power, normalized, center=False) of both signals, then mean_difference(y, x, norm),
 * rave/core.py:236-252, summed over the norms; EncodecAudioDistance, rave/core.py:415-433, sums it over its scales) with the
 * transform INSIDE the kernel.  x, y (rows, t_len) f32, two buffers that do not overlap; window (n_fft: the plain window);
 * twiddle as for rh_stft_loss_fwd_f32 (8-byte aligned).  frames = (t_len - n_fft) / hop + 1, bins = n_fft / 2 + 1,
 *   A = |scale * rfft(window * frame(y))|^power,  B = the same of x,  power 1 or 2,
 * scale = 1 / sqrt(sum(window^2)) for `normalized=True`, else 1: the caller computes it, as for rh_mel_diff_*.  A frame of x
 * and the same frame of y ride one complex transform, equalised by a power of two; a pair of frames that are equal sample by
 * sample has A - B = 0 by definition (two transforms of the same samples agree to the bit, the two halves of one do not), so
 * identical signals have distance exactly 0 and a zero gradient.
 * rh_spec_dist_fwd_f32 (replaces the unfold, window product, rocFFT, abs / pow and the reductions of rave/core.py:470-490):
 *   per workgroup (a span of frames of one row, walked in order) a fixed-tree partial of sum |A - B| and sum (A - B)^2, in
 *   (row, workgroup) order in `workspace` (rh_spec_dist_workspace_bytes).  No spectrum is written anywhere.
 * rh_spec_dist_finalize_all_f32 (replaces mean_difference's launches and the sum over the scales, rave/core.py:415-433): ONE
 *   launch for all scales of a distance adds the partials in a fixed order: sums (n_scales x 2) and
 *   total = sum_s (use_l1 * sums[s][0] + use_l2 * sums[s][1]) * inv_n[s]; inv_n: DEVICE array, 1 / (rows bins frames) per scale;
 *   partials[s] / partial_bytes[s]: HOST arrays (the workspaces of the forward calls); 1 .. 8 scales.
 * rh_spec_dist_bwd_f32 (replaces autograd through all of the above): a workgroup owns a span of dx / dy, recomputes the spectra
 *   of every frame that covers it and applies the cotangent grad_out[0] * inv_n * (use_l1 sign(A - B) + use_l2 2 (A - B)) with
 *   respect to A, negated for B (grad_out: one DEVICE scalar; sign(0) = 0), the power (scale S / |S| for power 1, exactly 0
 *   where |S| = 0 as torch's abs; 2 scale^2 S for power 2), the transposed real DFT, the window and the overlap-add.  Writes
 *   (accumulate = 0) or adds (!= 0: the scales of one distance sum in place) dx and dy; either may be NULL -- both gradients ride
 *   one inverse transform, a NULL side adds none and the other side's bits do not depend on it.  Samples that no frame covers
 *   (the uncentred tail) get exactly 0.  No atomics: one writer and one fixed order of additions per sample and per sum, the
 *   bits are reproducible; every launch can be captured.
 * Sizes (rh_spec_dist_supported answers 1 / 0; a host function): n_fft a power of two in 128 .. 2048, hop = n_fft / 4,
 * n_fft <= t_len <= 2^30, 0 < rows < 65536, power in {1, 2}, at least one norm -- anything else is RH_ERR_UNSUPPORTED; null
 * pointers, a misaligned twiddle table, overlapping x / y and a scale that is not positive and finite are RH_ERR_INVALID;
 * nothing is enqueued in any of these cases.  x, y, dx and dy need only be 4-byte aligned.  The backward kernel's dynamic LDS
 * never exceeds the 150 KiB cap of rh_stft_loss_bwd_f32's plan (rh_spec_dist_plan_info: out6 as rh_stft_loss_plan_info). */
int rh_spec_dist_supported(int32_t n_fft, int32_t hop, int32_t t_len, int64_t rows, int32_t power);
int64_t rh_spec_dist_workspace_bytes(int32_t n_fft, int32_t t_len, int64_t rows);
int rh_spec_dist_plan_info(int32_t n_fft, int32_t t_len, int64_t rows, int64_t* out6);
int rh_spec_dist_fwd_f32(const float* x, const float* y, const float* window, const float* twiddle, int64_t rows,
                         int32_t t_len, int32_t n_fft, int32_t power, float scale, void* workspace, int64_t workspace_bytes,
                         rh_stream_t stream);
int rh_spec_dist_finalize_all_f32(const float* const* partials, const int64_t* partial_bytes, int32_t n_scales,
                                  const float* inv_n, int32_t use_l1, int32_t use_l2, float* sums, float* total,
                                  rh_stream_t stream);
int rh_spec_dist_bwd_f32(const float* x, const float* y, const float* window, const float* twiddle, int64_t rows,
                         int32_t t_len, int32_t n_fft, int32_t power, float scale, int32_t use_l1, int32_t use_l2,
                         const float* grad_out, float* dx, float* dy, int32_t accumulate, rh_stream_t stream);

/* The complex spectrogram in front of the spectral discriminators, with its gradient:
 * torchaudio.transforms.Spectrogram(n_fft, hop_length, power=None, normalized, center) followed by
 * cat([s.real, s.imag], 1) (rave/discriminator.py:12-20,147-152, center = 0; rave/descript_discriminator.py:153-160,
 * center = 1 with reflect padding), one launch per direction.  x (rows, t_len) f32, rows = batch * channels; window (n_fft,
 * read from the buffer passed in); twiddle as for rh_stft_loss_fwd_f32 (e^{-2 pi i k / n_fft}, k < n_fft, 8-byte aligned).
 *   out (batch, 2 * channels, n_fft / 2 + 1, frames):  out[b][p * channels + c][k][f] = scale * (p ? Im : Re)
 *       sum_n window[n] xpad[b * channels + c][f * hop + n] e^{-2 pi i k n / n_fft}
 * -- the reference's cat([real, imag], 1) itself; with channels = 1 it reads (rows, 2, bins, frames), plane 0 real, plane 1
 * imaginary.  xpad = x (center = 0, frames = (t_len - n_fft) / hop + 1) or x reflect-padded by n_fft / 2 on either side,
 * indexed in the kernel (center = 1, frames = t_len / hop + 1).  scale = 1 / sqrt(sum(window^2)) for `normalized=True`, else 1:
 * the caller computes it.  n_fft = 4096 runs as a 2048-point complex transform.
 * rh_spectrogram_bwd_f32 (replaces autograd through torch.stft at the same sites): dx (rows, t_len) = the exact adjoint
 * applied to dout (laid out as out): the transpose of the real DFT (no Hermitian doubling), the window, overlap-add, the
 * reflected edges folded back.  A workgroup owns a span of dx and transforms every frame that covers it: no workspace, no
 * atomics, one writer and one fixed order of additions per sample -- bit-identical from run to run.
 * Sizes (rh_spectrogram_supported answers 1 / 0; a host function): n_fft a power of two in 128 .. 4096, 1 <= hop <= n_fft
 * (win_length == n_fft), t_len >= n_fft (center = 0) or t_len > n_fft / 2 (center = 1), t_len <= 2^30, 0 < rows < 65536 -- anything else is
 * RH_ERR_UNSUPPORTED; null pointers, rows no multiple of channels, a misaligned twiddle table and a scale that is not
 * positive and finite are RH_ERR_INVALID; nothing is enqueued in any of these cases.  x, out, dout and dx need only be
 * 4-byte aligned (16-byte accesses are used where the pointer and the frame count allow them). */
int rh_spectrogram_supported(int32_t n_fft, int32_t hop, int32_t t_len, int64_t rows, int32_t center);
int rh_spectrogram_fwd_f32(const float* x, const float* window, const float* twiddle, int64_t rows, int32_t channels,
                           int32_t t_len, int32_t n_fft, int32_t hop, int32_t center, float scale, float* out,
                           rh_stream_t stream);
int rh_spectrogram_bwd_f32(const float* dout, const float* window, const float* twiddle, int64_t rows, int32_t channels,
                           int32_t t_len, int32_t n_fft, int32_t hop, int32_t center, float scale, float* dx,
                           rh_stream_t stream);

/* Measurement hook (bench.py's roofline leg; not part of the reference interface): arm a pair of HIP events (hipEvent_t,
 * created by the caller with timing enabled) for the calling thread's NEXT main kernel launch -- the convolution /
 * weight-gradient kernel of rh_conv1d_fwd_f32 / _bwd_data_f32 / _bwd_weight_f32 / rh_residual_unit_fwd_f32, not its split-K
 * finalize or reduction launches.  The kernel is dispatched with the events as its own start / stop events, so
 * hipEventElapsedTime(start, stop) is the duration rocprofv3 reports for that dispatch.  rh_kernel_events_used() tells whether
 * a launch consumed the pair (and disarms it).  The pair is dropped when the conv / weight-gradient call returns, whether its
 * main kernel took it or not (a failed call, a kernel without the hook): it never reaches a later call. */
int rh_set_kernel_events(void* start_event, void* stop_event);
int rh_kernel_events_used(void);
int rh_event_create(void** event);                                   /* hipEventCreate (timing enabled) */
int rh_event_destroy(void* event);
int rh_event_elapsed_ms(void* start_event, void* stop_event, float* ms);   /* after the stream has been synchronised */

/* ---- the generator loss of a training step (rave/model.py:336-344, 392-412) ---------------------------------------
 * scaled[i] = w1_i * value_i  (the weighted distance the step logs: `self.weights[...] * v`, `reg * beta_factor`)
 * total     = sum_i scaled[i] * w2_i, in term order from 0  (`loss_gen_value += v * self.weights.get(k, 1.)`)
 * as one launch, and its gradient grads[i] = (grad_total * w2_i) * w1_i as another -- instead of ~2 scalar ATen launches per
 * term in each direction between the forward and the backward pass.  Each product is rounded separately and the sum runs
 * in order: the same bits as the ATen chain.  value / w1_dev: device scalars (w1_dev NULL -> the host value w1);
 * <= 16 terms; the table travels by value (hipGraph-capturable). */
typedef struct rh_loss_item {
    const float* value;
    const float* w1_dev;
    float w1;
    float w2;
} rh_loss_item;
int rh_loss_combine_fwd_f32(const rh_loss_item* items, int32_t n_items, float* scaled, float* total, rh_stream_t stream);
int rh_loss_combine_bwd_f32(const rh_loss_item* items, int32_t n_items, const float* grad_total, float* grads,
                            rh_stream_t stream);

/* Adam step over many tensors (torch.optim.Adam, weight_decay = 0, amsgrad = False; rave/model.py:226-233): for every
 * item  m = lerp(m, g, 1 - beta1);  v = beta2 v + (1 - beta2) g^2;  p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * with t = the item's OWN step count (torch keeps one per parameter: a parameter whose first gradient comes later -- the
 * v1 generator's noise branch after the warm-up, rave/blocks.py:418 -- starts at t = 1).
 * `items` is a HOST array (the pointers inside are device pointers; it is consumed during the call: the tables travel in
 * the kernel arguments, so the call can be recorded into a hipGraph); `lr` and every `step` are device scalars -- the call
 * first advances each DISTINCT step counter among the items by one (items may share a counter) -- and `aux` is
 * 2 * n_items floats of device scratch (the bias corrections per counter). */
typedef struct rh_adam_item {
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t n;
    float* step;
} rh_adam_item;
int rh_adam_step_f32(const rh_adam_item* items, int32_t n_items, const float* lr, float beta1, float beta2, float eps,
                     float* aux, rh_stream_t stream);

/* Exponential average of the weights over many tensors (`rave train --ema`: the EMA callback of scripts/train.py:88-102).
 * rh_ema_update_f32 = on_train_batch_end (:88-96): for every item  a = a * f + b * g  with a = the average, b = the parameter,
 * f = (float)factor, g = (float)(1.0 - factor) (subtraction in double) -- three separately rounded f32 operations, bit for bit
 * what torch's `w * factor + p * (1 - factor)` gives; b is only read.
 * rh_swap_f32 = swap_weights (:98-102): exchanges the contents of a and b in one pass, in place on both sides.
 * `items` is a HOST array (device pointers inside) consumed during the call: the tables travel in the kernel arguments,
 * <= 64 tensors per launch; items with n == 0 take no slot.  The whole table is checked before anything is launched:
 * n_items < 0, a null table with n_items > 0, a null pointer in an item with n > 0, n < 0 or n >= 2^31 - 1, a == b, and a
 * factor that is not a finite number in [0, 1] are refused with RH_ERR_INVALID; n_items == 0 launches nothing. */
typedef struct rh_pair_item {
    float* a;
    float* b;
    int64_t n;
} rh_pair_item;
int rh_ema_update_f32(const rh_pair_item* items, int32_t n_items, double factor, rh_stream_t stream);
int rh_swap_f32(const rh_pair_item* items, int32_t n_items, rh_stream_t stream);

/* The recurrent latent layer (rave/blocks.py:295-319 `GRU`: torch.nn.GRU(input_size = H, hidden_size = H, num_layers = L,
 * batch_first = True) between two permute(0, 2, 1), h0 = 0; placed in front of the v2 decoder by configs/hybrid.gin, :632-633).
 * x, y, dy, dx are the model's (batch, hidden, t_len) tensors, time innermost: the permutes are addressing, no transposed
 * copy is made.  Gates in torch's order (r, z, n); w_ih / w_hh are (3H, H), b_ih / b_hh (3H): the layouts of
 * gru.weight_ih_l{k} etc.  f32 throughout; the sigmoid is 1 / (1 + expf(-a)): finite, and exactly 0 / 1 at a = -+100.
 * Every reduction has one fixed order (no atomics): results are bit-identical from run to run.
 * Sizes: hidden a multiple of 16 in [16, 128], 1 <= layers <= 4 (rh_gru_supported answers 1 / 0), batch >= 1, t_len >= 1,
 * batch * (t_len + 1) < 2^22 -- anything else is RH_ERR_UNSUPPORTED; null pointers are RH_ERR_INVALID, a short workspace
 * RH_ERR_WORKSPACE; nothing is enqueued in any of these cases.
 * `layers` is a HOST array of n_layers items (device pointers inside) consumed during the call; fwd reads the four
 * parameters of each, bwd also writes the four gradients (overwritten, not accumulated).
 * Workspace: rh_gru_workspace_bytes(..., training, &bytes), any 4-byte aligned device buffer.  With training != 0 fwd leaves in
 * it what bwd needs (per layer and step: r, z, n, W_hn h + b_hn, h) and bwd must be given the SAME buffer, unmodified,
 * with the same x and sizes; its tail is scratch of both.  With training == 0 nothing is kept (4 * batch * t_len * hidden
 * floats of scratch, roughly). */
typedef struct rh_gru_item {
    const float* w_ih;
    const float* w_hh;
    const float* b_ih;
    const float* b_hh;
    float* dw_ih; /* the four gradients: bwd only, fwd ignores them */
    float* dw_hh;
    float* db_ih;
    float* db_hh;
} rh_gru_item;
int rh_gru_supported(int32_t hidden, int32_t layers);
int rh_gru_workspace_bytes(int32_t batch, int32_t hidden, int32_t t_len, int32_t layers, int32_t training, int64_t* bytes);
int rh_gru_fwd_f32(const float* x, const rh_gru_item* layers, int32_t n_layers, int32_t batch, int32_t hidden, int32_t t_len,
                   int32_t training, float* y, void* workspace, int64_t workspace_bytes, rh_stream_t stream);
int rh_gru_bwd_f32(const float* dy, const float* x, const rh_gru_item* layers, int32_t n_layers, int32_t batch, int32_t hidden,
                   int32_t t_len, float* dx, void* workspace, int64_t workspace_bytes, rh_stream_t stream);

/* Feature-matching distance of the GAN phase (rave/model.py:359-372 over rave/core.py:236-252, norm "L1") on UNSPLIT
 * discriminator feature maps: item i is a dense f32 tensor of 2 * half elements, the real half of the batch first;
 * distance = sum_i w_i * (relative ? sum|r-f| / sum|r| : sum|r-f|)  (the host folds the 1 / count factors -- and for the
 * non-relative form 1 / half -- into w_i).  `items` is a HOST array consumed during the call (<= 80 items).  fwd writes
 * sums[2i] = sum|r-f|, sums[2i+1] = sum|r| and out[0]; bwd writes d distance / d feature * grad_out[0] into items[i].df
 * (same layout as f).  workspace: rh_feature_matching_workspace_bytes(). */
typedef struct rh_fm_item {
    const float* f;
    float* df;
    int64_t half;
    float w;
} rh_fm_item;
int64_t rh_feature_matching_workspace_bytes(const rh_fm_item* items, int32_t n_items);
int rh_feature_matching_fwd_f32(const rh_fm_item* items, int32_t n_items, int32_t relative, void* workspace,
                                int64_t workspace_bytes, float* sums, float* out, rh_stream_t stream);
int rh_feature_matching_bwd_f32(const rh_fm_item* items, int32_t n_items, int32_t relative, const float* sums,
                                const float* grad_out, rh_stream_t stream);

/* The GAN objectives (rave/core.py:151-170: hinge_gan, ls_gan, nonsaturating_gan) summed over the discriminator heads as the
 * training step accumulates them (rave/model.py:354-376), with the logged pred_real / pred_fake of the same loop.
 * Item i is one head: `real` and `fake` are two dense blocks of n f32 scores each, in any element order (a mean does not care,
 * and bwd writes d_real / d_fake in the same memory order); for an unsplit (2B, ...) score map fake = real + n.  Every pointer
 * may be any 4-byte aligned address (16-byte accesses are used where the pointers and n allow them; the bits are the same).
 * mode: RH_GAN_HINGE      dis = mean(relu(1 - r) + relu(1 + f)),       adv = mean(-f)
 *       RH_GAN_LS         dis = mean((r - 1)^2 + f^2),                  adv = mean((f - 1)^2)
 *       RH_GAN_NONSAT     p = clamp(sigmoid(s), 1e-7, 1 - 1e-7), both bounds rounded to f32 (sigmoid = 1 / (1 + expf(-s)));
 *                         dis = mean(-(logf(p_r) + logf(1 - p_f))),     adv = mean(-logf(p_f))
 * fwd: sums[4 i + {0, 1, 2, 3}] = head i's dis, adv, mean(r), mean(f);  out[0 .. 3] = loss_dis, loss_adv, pred_real, pred_fake
 * = the SUMS of those over the heads (not averages).  Two launches: per-workgroup partials into `workspace`
 * (rh_gan_loss_workspace_bytes; contents irrelevant before and after), then one ordered finalize.
 * bwd: grad_out[0 .. 1] (device memory) = d / d loss_dis, d / d loss_adv; writes d_real and d_fake of every head (overwritten,
 * not accumulated) in one launch; pred_* are logged values and carry no gradient.  Gates as ATen's: relu passes where its
 * argument is > 0 (0 at equality); the clamp passes where lo <= sigmoid(s) <= hi, so the gradient is exactly 0 wherever it
 * changed the value.  No atomics, one fixed order of additions: bit-identical from run to run.
 * `items` is a HOST array (device pointers inside) consumed during the call.  Refused before anything is launched: a null
 * table, a null real / fake (bwd: d_real / d_fake as well), null workspace / sums / out / grad_out, n <= 0 (RH_ERR_INVALID);
 * n_items outside 1 ... 80, an unknown mode (RH_ERR_UNSUPPORTED; rh_gan_loss_supported answers 1 / 0 for the pair); a
 * workspace smaller than rh_gan_loss_workspace_bytes (RH_ERR_WORKSPACE; that query returns -1 for a null table, n_items outside 1 ... 80 or an n <= 0). */
#define RH_GAN_HINGE 0
#define RH_GAN_LS 1
#define RH_GAN_NONSAT 2
typedef struct rh_gan_item {
    const float* real;
    const float* fake;
    float* d_real;
    float* d_fake;
    int64_t n;
} rh_gan_item;
int rh_gan_loss_supported(int32_t mode, int32_t n_items);
int64_t rh_gan_loss_workspace_bytes(const rh_gan_item* items, int32_t n_items);
int rh_gan_loss_fwd_f32(const rh_gan_item* items, int32_t n_items, int32_t mode, void* workspace, int64_t workspace_bytes,
                        float* sums, float* out, rh_stream_t stream);
int rh_gan_loss_bwd_f32(const rh_gan_item* items, int32_t n_items, int32_t mode, const float* grad_out, rh_stream_t stream);

/* VariationalEncoder.reparametrize (rave/blocks.py:727-745): z (batch, 2c, l) = [mean | scale] along dim 1, eps (batch, c, l)
 * the noise draw;  std = softplus(scale) + 1e-4,  zs = eps * std + mean,
 * kl[0] = (mean^2 + std^2 - log(std^2) - 1).sum(1).mean().  bwd: dz from dzs (may be NULL) and the scalar dkl (may be NULL). */
int64_t rh_reparam_workspace_bytes(void);
int rh_reparam_fwd_f32(const float* z, const float* eps, int32_t batch, int32_t c, int32_t l, float* zs, float* kl,
                       void* workspace, int64_t workspace_bytes, rh_stream_t stream);
int rh_reparam_bwd_f32(const float* z, const float* eps, const float* dzs, const float* dkl, int32_t batch, int32_t c,
                       int32_t l, float* dz, rh_stream_t stream);

/* Latent-space analysis at the end of validation (rave/model.py:463-481: `z = cat(z, 0)`, `rearrange(z, "b c t -> (b t) c")`,
 * `z.mean(0)`, `PCA(...).fit(z)`): the first and second moments of the posterior mean, accumulated one validation batch per
 * call.  `mean` is f32 (batch, channels, t_len) as validation_step returns it, time innermost, any 4-byte aligned address:
 * the rows of the statistics are the (b, t) pairs, the rearrange is addressing.  `acc` is the caller's accumulator of
 * 1 + channels + channels^2 doubles (8-byte aligned; zero it before the first call):
 *   acc[0] += batch * t_len,   acc[1 + i] += sum z[b,i,t],   acc[1 + channels + i * channels + j] += sum z[b,i,t] * z[b,j,t].
 * f64 arithmetic: the products of f32 values are exact, only the additions round.  No atomics; the split of the rows over
 * workgroups depends on (batch, t_len) only, the per-workgroup partials go through `workspace`
 * (rh_latent_moments_workspace_bytes, 8-byte aligned, contents irrelevant before and after) and are added in a fixed order:
 * the same sequence of calls gives bit-identical accumulators.  Calls on one accumulator must be stream-ordered.
 * 1 <= channels <= 128 (rh_latent_moments_supported answers 1 / 0); more channels, non-positive sizes, null or misaligned
 * pointers are RH_ERR_INVALID and enqueue nothing. */
int rh_latent_moments_supported(int32_t channels);
int rh_latent_moments_workspace_bytes(int32_t batch, int32_t channels, int32_t t_len, int64_t* bytes);
int rh_latent_moments_acc_f64(const float* mean, int32_t batch, int32_t channels, int32_t t_len, double* acc, void* workspace,
                              rh_stream_t stream);

/* Filtered-noise synthesis of the noise generators (rave/core.py:48-81 `amp_to_impulse_response` and `fft_convolve` after
 * `mod_sigmoid`, :23-24, as rave/blocks.py:230-240 `NoiseGenerator.forward` and :282-292 `NoiseGeneratorV2.forward` chain
 * them), without a transform: both are linear maps of fixed small length.
 *   amp_j = 2 sigmoid(h - 5)^2.3 + 1e-7,   ir = M amp,   out[b, d, t N + n] = sum_{k <= n} noise[b, t, d, k] ir[n - k]
 * h (batch, channels * noise_bands, t_len): the last convolution's output, channel d * noise_bands + j (the reference's permute
 * + reshape); noise (batch, t_len, channels, target_size): the U(-1, 1) draw in the layout of the reference's rand_like(ir);
 * out (batch, channels, t_len * target_size), written in place of the reference's two permutes.
 * `table` = M, (target_size, noise_bands) row-major on the device: amp_to_impulse_response applied to the identity (irfft,
 * roll, Hann window, pad -- or crop, where 2 (noise_bands - 1) > target_size -- roll).  rh_noise_synth_table_f32 fills a HOST
 * buffer of target_size * noise_bands floats with it, computed in f64 and rounded once.
 * bwd: gh = d out / d h applied to gout (same layouts; overwritten): d_ir[j] = sum_{n >= j} gout[n] noise[n - j],
 * d_amp = M^T d_ir, gh = d_amp 4.6 s^2.3 (1 - s) with s = sigmoid(h - 5).  The noise gets no gradient.
 * One launch each, no workspace, no atomics: every (b, d, t) is computed by one workgroup in a fixed order, so results are
 * bit-identical from run to run.  Every pointer may be any 4-byte aligned address.
 * Sizes: 2 <= noise_bands <= 33, 1 <= target_size <= 64 (rh_noise_synth_supported answers 1 / 0), batch, channels,
 * t_len >= 1 -- other bands / sizes are RH_ERR_UNSUPPORTED; null pointers and non-positive extents RH_ERR_INVALID; nothing is
 * enqueued in either case. */
int rh_noise_synth_supported(int32_t noise_bands, int32_t target_size);
int rh_noise_synth_table_f32(int32_t noise_bands, int32_t target_size, float* table_host);
int rh_noise_synth_fwd_f32(const float* h, const float* noise, const float* table, int32_t batch, int32_t channels,
                           int32_t t_len, int32_t noise_bands, int32_t target_size, float* out, rh_stream_t stream);
int rh_noise_synth_bwd_f32(const float* h, const float* noise, const float* table, const float* gout, int32_t batch,
                           int32_t channels, int32_t t_len, int32_t noise_bands, int32_t target_size, float* gh,
                           rh_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RAVE_HIP_H */
