/*
 * libp3d_hip.so -- C ABI of the MI355X (gfx950) hot path of
 * 3D-Pose-Estimation-with-Previleged-Information.
 *
 * The reference has no FFI of its own: its hot path is eager PyTorch modules.  Each entry
 * point below replaces the torch operator call(s) named in its comment (reference file:line);
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every tensor is fp32, NCHW, contiguous, in device (HBM) memory, owned by the caller
 *   - no hidden allocation, no hidden synchronisation: scratch comes in through `workspace`,
 *     sized by the matching *_workspace_bytes() query; work is enqueued on `stream`
 *     (a hipStream_t passed as void*, NULL = default stream)
 *   - return 0 on success, a negative P3D_E* code on error; p3d_last_error() gives the text
 *     (thread local).  Nothing throws across the boundary.
 *   - thread safe for distinct streams.
 */
#ifndef P3D_HIP_H
#define P3D_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P3D_OK 0
#define P3D_EINVAL (-1)      /* bad shape / null pointer / unsupported argument */
#define P3D_EWORKSPACE (-2)  /* workspace missing or too small */
#define P3D_ELAUNCH (-3)     /* HIP reported a launch error */

#define P3D_VERSION 100

int32_t p3d_version(void);
const char* p3d_last_error(void);
/* A second stream that is PROVEN to run beside `main_stream` (two 200-us spin kernels, one per stream, must take ~200 us, not ~400): see csrc/p3d_api.hip.
 * *overlaps = 1 if a candidate passed the probe, 0 if the returned stream shares the main stream's hardware queue after all. */
int32_t p3d_stream_create_beside(void* main_stream, void** stream, int32_t* overlaps);
/* a stream restricted to the compute units whose bit is set in mask[0 .. words) (hipExtStreamCreateWithCUMask); p3d_probe_hw_ids launches nblocks spinning blocks
   on a stream and reports where each ran: out[b] = (XCC_ID << 16) | HW_ID[15:0] */
int32_t p3d_stream_create_cumask(const uint32_t* mask, int32_t words, void** stream);
int32_t p3d_probe_hw_ids(void* stream, int32_t* out_device, int32_t nblocks, int32_t spin_us);
int32_t p3d_stream_destroy(void* stream);

/* ------------------------------------------------------------------------------------------
 * Convolution: nn.Conv2d forward / input gradient / weight gradient
 *   depthnet.py:16-33,65-89,138,156,167-173  resnet.py:142,160-172  fusionnet.py:135,164-165
 * and, through the optional mask pointers, partial_conv.PartialConv (partial_conv.py:32-57).
 *
 * x [N,C,H,W], w [K,c_total,R,S] of which this call uses input channels [c_offset, c_offset+C)
 * (c_total == C, c_offset == 0 for an ordinary conv; the fusion 1x1 conv over cat([x,y]) is two
 * calls, one per stream, the second with accumulate = 1: fusionnet.py:138-139), y [N,K,Ho,Wo].
 * Ho = (H + 2*pad - dil*(R-1) - 1)/stride + 1, same for Wo; the library re-derives and checks.
 * ------------------------------------------------------------------------------------------ */
typedef struct p3d_conv_desc {
    int32_t N, C, H, W;
    int32_t K, R, S;
    int32_t stride, pad, dil;
    int32_t Ho, Wo;
    int32_t c_total, c_offset;
    int32_t accumulate;   /* fwd: y += result (fp16 forward: must be 0); dgrad: dx += result; wgrad: dw += result */
    int32_t reserved;
} p3d_conv_desc;

/* y = conv(x * mask_in) * mult + bias.  bias [K] or NULL.  mask_in [N,1,H,W] or NULL (prologue,
 * partial_conv.py:45).  mult [N,1,Ho,Wo] or NULL (epilogue, partial_conv.py:53).  With both bias and
 * mult the result is ((raw-b)*mult + b)*mask_out with mask_out = (mult > 0)  (partial_conv.py:48-51). */
int32_t p3d_conv2d_fwd(const p3d_conv_desc* d, const float* x, const float* w, const float* bias,
                       const float* mask_in, const float* mult, float* y, void* workspace, size_t workspace_bytes, void* stream);
/* Scratch for the split-K forward the library uses when a launch would leave most CUs one long block (0 otherwise; the
 * workspace is optional: with NULL / too small the conv runs unsplit). */
size_t p3d_conv2d_fwd_workspace_bytes(const p3d_conv_desc* d);

/* dx = dgrad(dy * mult) * mask_in  (autograd of the expression above w.r.t. x).  Stride-2 convolutions are
 * computed as four dense parity-class GEMMs staged in `workspace`; a stride-1 launch of few long blocks is split over K into
 * slabs there (optional: without workspace it runs unsplit).  Query the size; 0 when none is used. */
/* Inference: nn.Conv2d (no bias) + nn.BatchNorm2d in eval mode (+ residual add, + ReLU) of a residual block (depthnet.py:42-56,
 * 98-116 under model.eval(), depth_train.py:611) as ONE kernel: y = act((conv(x, w) - mean) * gamma / sqrt(var + eps) + beta + res).
 * res may be NULL; the BatchNorm constants are folded into per-channel scale / shift at the head of the workspace. */
size_t p3d_conv2d_bn_eval_fwd_workspace_bytes(const p3d_conv_desc* d);
int32_t p3d_conv2d_bn_eval_fwd(const p3d_conv_desc* d, const float* x, const float* w, const float* gamma, const float* beta,
                               const float* running_mean, const float* running_var, float eps, const float* res, int32_t relu,
                               float* y, void* workspace, size_t workspace_bytes, void* stream);
size_t p3d_conv2d_dgrad_workspace_bytes(const p3d_conv_desc* d);
int32_t p3d_conv2d_dgrad(const p3d_conv_desc* d, const float* dy, const float* w, const float* mult,
                         const float* mask_in, float* dx, void* workspace, size_t workspace_bytes, void* stream);

/* dw[:, c_offset:c_offset+C] = wgrad(dy * mult, x * mask_in); deterministic two-stage split-K
 * reduction through `workspace`. */
size_t p3d_conv2d_wgrad_workspace_bytes(const p3d_conv_desc* d);
int32_t p3d_conv2d_wgrad(const p3d_conv_desc* d, const float* dy, const float* x, const float* mult,
                         const float* mask_in, float* dw, void* workspace, size_t workspace_bytes, void* stream);

/* The dense convolutions (whole weight tensor, odd square filters, stride 1 or 2, channel counts in steps of 16 and four-pixel-aligned rows: every layer of
 * the reference networks but the 3- / 1-channel stems and odd-sized inputs) run by DEFAULT as exact-fp32 implicit GEMMs on the bf16 matrix pipe
 * (three-piece operand split, six piece products, fp32 accumulation; csrc/p3d_fx.hip): fp32-grade results, measured error <= the
 * fp32-MFMA kernel's.  p3d_x3_enable(0) (or P3D_X3=0 in the environment) keeps every layer on the v_mfma_f32_32x32x2_f32 kernels.  Returns the previous setting. */
int32_t p3d_x3_enable(int32_t on);
/* Opt-in (default OFF; P3D_X3_ANY=1 in the environment turns it on): p3d_conv2d_fwd, p3d_conv2d_dgrad (stride 1) and p3d_conv2d_wgrad run a dense convolution with a
 * whole weight tensor that the aligned predicates refuse only for its map width (W, Wo no multiples of 4; Ho * Wo no multiple of 16: the 65 / 33 / 17 maps of the
 * reference's default 257 crop) on the ragged x3 instances instead of the fp32-MFMA kernels ("Training at any map width").  While it is on the
 * three workspace queries report the larger of the two plans.  Aligned shapes, partial convolutions and strided data gradients are launched exactly as with the switch
 * off.  Returns the previous setting.
 * p3d_conv2d_*_any_supported: 1 where the ragged instances of that pass admit the convolution (whatever the switch says; they admit aligned shapes too, which the
 * entries keep on the aligned instances), 0 otherwise -- a channel window, a strided data gradient, channel counts outside the x3 rules. */
int32_t p3d_x3_any_enable(int32_t on);
int32_t p3d_conv2d_fwd_any_supported(const p3d_conv_desc* d);
int32_t p3d_conv2d_dgrad_any_supported(const p3d_conv_desc* d);
int32_t p3d_conv2d_wgrad_any_supported(const p3d_conv_desc* d);
/* Opt-in, a switch of its own (default OFF; P3D_X3_ANY_PARTIAL=1 in the environment turns it on; independent of p3d_x3_any_enable): the same for PARTIAL convolutions.
 * p3d_conv2d_fwd, p3d_conv2d_dgrad (stride 1) and p3d_conv2d_wgrad, called with BOTH factors (mask_in and mult), no bias and a whole weight tensor, run a convolution that
 * the aligned masked instances refuse only for its map width on the masked ragged x3 instances instead of the fp32-MFMA kernels: y = conv(x * mask_in) * mult,
 * dx (+)= dgrad(dy * mult) * mask_in (the factor before the accumulate read: where mask_in is 0 an accumulating call leaves dx bit for bit), dw = wgrad(dy * mult,
 * x * mask_in).  While it is on the three workspace queries report the larger of the plans.  As for the dense switch, a forward or data gradient whose workspace is too
 * small, or an operand off a 16-B line, quietly runs on fp32-MFMA; a weight gradient whose workspace is too small fails with P3D_EWORKSPACE.  A call with one factor, a
 * bias, a channel window or a strided data gradient, every dense call and every aligned shape are launched exactly as with the switch off.  Returns the previous setting.
 * p3d_conv2d_*_masked_any_supported: 1 where the masked ragged instances of that pass admit the convolution (whatever the switch says; aligned shapes too, which the
 * entries keep on the aligned masked instances), 0 otherwise.  The rules are the dense ones at the masked thresholds: 64 result channels for the forward and the
 * data gradient, 96 on both sides for the weight gradient. */
int32_t p3d_x3_any_partial_enable(int32_t on);
int32_t p3d_conv2d_fwd_masked_any_supported(const p3d_conv_desc* d);
int32_t p3d_conv2d_dgrad_masked_any_supported(const p3d_conv_desc* d);
int32_t p3d_conv2d_wgrad_masked_any_supported(const p3d_conv_desc* d);
/* Opt-in, a switch of its own (default OFF; P3D_X3_ANY_STRIDED=1 in the environment turns it on; independent of the other three): p3d_conv2d_dgrad runs a dense
 * STRIDE-2 data gradient that the aligned predicate refuses (an odd side, W no multiple of 8: the 129 -> 65 -> 33 -> 17 maps of the default 257 crop) on the x3 kernels
 * instead of the fp32-MFMA kernels: one launch of the ragged fp32-fed instance per parity class of the input -- class (ph, pw) has (H - ph + 1) / 2 rows of
 * (W - pw + 1) / 2 pixels -- into tight class planes in the workspace, then one streaming pass (dgrad_interleave_rows_kernel) that interleaves the planes into dx, writes
 * +0 to the pixels no tap reaches (a 1x1: three of four) and adds what dx held under `accumulate` ("Stride-2 data gradients at any map width").
 * While it is on, p3d_conv2d_dgrad_workspace_bytes reports for the shapes the predicate admits at least the data-gradient weight image plus four class planes of
 * N C ceil(H / 2) ceil(W / 2) floats (rounded up to 4), each part on a 256-B line.  A workspace that is too small, or an operand off a 16-B line, quietly runs on
 * fp32-MFMA as with the switch off.  Partial convolutions, aligned shapes, stride-1 calls and every other entry are launched exactly as with the switch off.  Returns
 * the previous setting.
 * p3d_conv2d_dgrad_strided_any_supported: 1 where the class launches admit the convolution (whatever the switch says; aligned shapes too, which the entry keeps on the
 * aligned instances): the stride-2 data-gradient rule of the x3 kernels without its clauses on H and W -- whole weights, odd square filter, K in steps of 16 and >= 32,
 * C in steps of 4 and >= 96, pad == dil (R - 1) / 2, R == 1 or dil == 1.  0 otherwise, for stride 1 and for a NULL or malformed descriptor. */
int32_t p3d_x3_any_strided_enable(int32_t on);
int32_t p3d_conv2d_dgrad_strided_any_supported(const p3d_conv_desc* d);
/* TEST HOOK (tests/test_strided_any_gpu.py, tools/train_anysize_bench.py; nothing in the package calls it): the finishing pass of a stride-2 data gradient alone.
 * dx[n][c][hi][wi] (=|+=, by accumulate) stage[cls * cls_stride + ((n C + c) hc + hi / 2) wc + wi / 2] (* mask_in[n][hi][wi] when given), cls = (hi & 1) * 2 + (wi & 1),
 * hc = (H - (hi & 1) + 1) / 2, wc = (W - (wi & 1) + 1) / 2; a class whose bit in live_mask is clear contributes 0 and its plane is not read.  kernel 0:
 * dgrad_interleave_kernel (the fp32-MFMA path's, one element per thread); kernel 1: dgrad_interleave_rows_kernel (p3d_x3_any_strided_enable's).  The two are bit-equal.
 * cls_stride in floats, at least N C ceil(H / 2) ceil(W / 2); N C H W < 2^31 for kernel 1. */
int32_t p3d_dgrad_interleave(int32_t kernel, const float* stage, float* dx, const float* mask_in, int32_t N, int32_t C, int32_t H, int32_t W, size_t cls_stride,
                             int32_t live_mask, int32_t accumulate, void* stream);
/* Test and tuning hooks of the x3 path; value 0 restores the built-in behaviour unless noted.  Codes:
 *   0  forced split count of the weight-gradient launches                  (tools/split_sweep.py, tests/test_kernels_gpu.py)
 *   1  forced split count of the forward / data-gradient launches          (the same)
 *   2  forced block target of the weight-gradient split plan               (tools/split_sweep.py)
 *   3  0: the two opening image passes of a downsample block as two launches instead of the pair pass (default 1; tests/test_block_gpu.py)
 *   5  1: one launch per parity class of a strided data gradient instead of one launch for all (tests/test_geometry_gpu.py)
 *   6  1: p3d_block_* keep the activation / gradient images of dense blocks as three bf16 planes (6 B per element) instead of fp32 row images (4 B); changes what
 *         p3d_block_image_bytes reports, so set it before the buffers of a block are sized (tests/test_row_images_gpu.py, the A/B of profiles/row_images.md)
 * Any other code is ignored. */
void p3d_fx_tune(int32_t what, int32_t value);
/* How many conv launches took which path since the last reset: counts / flops [0..2] = forward, data gradient, weight gradient on the bf16-pipe kernels,
 * [3..5] = the same three on the fp32-MFMA kernels (algorithmic flops 2*N*K*Ho*Wo*C*R*S).  Host-side bookkeeping only. */
void p3d_conv_path_stats(uint64_t* counts, double* flops, int32_t reset);
/* What the last p3d_conv2d_fwd / _bn_eval_fwd / _dgrad / _wgrad call of the process launched on the fp32-MFMA family, written where the launches are made.
 * Host-side bookkeeping only.  out[P3D_FP32_LAUNCH_FIELDS]:
 *   [0] pass: 0 forward, 1 data gradient, 2 weight gradient, -1: the call launched no igemm_kernel (it ran on the x3 kernels, or was refused); every entry
 *       clears the record before anything else, and calls of other entries (the block executor) never write to it, so with pass -1 all but [10] is 0 / -1
 *   [1] tile 0..5 = 128x128, 64x256, 96x128, 64x128, 128x64, 64x64 (-1 with pass -1)     [2] TAPM     [3] MASKED     [4] WV  -- the kernel's template arguments
 *   [5] grid.x   [6] grid.y   [7] what grid.y counts: 0 nothing (1), 1 K slabs, 2 parity classes of a strided data gradient
 *   [8] 1: the operand A was the tap-major weight image at the head of the workspace
 *   [9] the finishing kernels that followed, as bits: 1 fwd_reduce, 2 dgrad_interleave, 4 dgrad_interleave2, 8 wgrad_reduce, 16 wgrad_reduce_tapm,
 *       32 wgrad_reduce16, 64 wgrad_reduce16_tapm, 128 slab_fold (then with 8 or 16)
 *   [10] 1: the call came through p3d_conv2d_bn_eval_fwd
 *   [11] what the plan wanted and the workspace had no room for, as bits: 1 the split-K slabs (the launch is unsplit), 2 the weight image
 *   [12..15] 0 */
#define P3D_FP32_LAUNCH_FIELDS 16
void p3d_conv_last_fp32_launch(int32_t* out);
/* TEST HOOK (tests/test_fp32_mfma_plan_host.py; nothing in the package calls it), host-only: how the fp32-MFMA family would run one call of an entry -- the plan the
 * entry itself follows and the workspace queries read -- as the record p3d_conv_last_fp32_launch would give after that call.  Nothing is launched, no operand exists
 * and the route is not consulted (the call is taken to have landed on this family).  entry: 0 p3d_conv2d_fwd, 1 p3d_conv2d_bn_eval_fwd, 2 p3d_conv2d_dgrad,
 * 3 p3d_conv2d_wgrad.  `options` says what the operands would be:
 *   bit 0  mask_in is given      bit 1  mult is given      (neither with entry 1)
 *   bit 2  dy (weight gradient) is 4 B off a 16-B line      bit 3  x (weight gradient) is      bit 4  the result is: dx of a strided data gradient, dw
 * workspace_bytes: what the call would be given; 0: no workspace.
 * Returns P3D_EWORKSPACE where the entry would (the eval head, the staged classes of a strided data gradient or the weight-gradient slabs do not fit) and P3D_EINVAL
 * for a malformed descriptor, an unknown entry or option and a weight gradient whose per-block window exceeds 2 GiB; out then holds the empty record (pass -1), or
 * is untouched when the arguments themselves were refused. */
int32_t p3d_conv2d_fp32_plan(int32_t entry, const p3d_conv_desc* d, int32_t options, size_t workspace_bytes, int32_t* out);
/* db[k] (=|+=) sum_{n,h,w} dy[n,k,h,w]  (bias gradient of the regressor conv, depthnet.py:156). */
int32_t p3d_conv2d_bgrad(const float* dy, int32_t N, int32_t K, int32_t HW, float* db, int32_t accumulate, void* stream);
/* bias gradient of a PartialConv with bias (partial_conv.py:48-51: out = ((raw - b) * mult + b) * mask_out, so d out / d b = mask_out):
 * db[k] = sum over n, p of dy[n][k][p] * (mult[n][p] > 0);  mult [N,1,Ho,Wo] as written by p3d_mask_count_fwd. */
int32_t p3d_conv2d_bgrad_masked(const float* dy, const float* mult, int32_t N, int32_t K, int32_t HW, float* db, int32_t accumulate, void* stream);

/* partial_conv.py:35-43: cnt = boxsum(mask); mult = R*S/(cnt+1e-6)*clamp(cnt,0,1); mask_out = clamp(cnt,0,1).
 * mask [N,1,H,W] -> mult, mask_out [N,1,Ho,Wo]. */
int32_t p3d_mask_count_fwd(const p3d_conv_desc* d, const float* mask, float* mult, float* mask_out, void* stream);

/* veil = (x != 0).float()  (partial_depthnet.py:215) */
int32_t p3d_nonzero_mask(const float* x, float* mask, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------
 * One residual block per call, training mode: BasicBlock / Bottleneck forward and backward
 *   depthnet.py:10-56 (BasicBlock), :59-116 (Bottleneck); twins resnet.py:21-119, fusionnet.py:21-127
 * conv -> BN -> ReLU -> conv -> BN -> ReLU [-> conv -> BN] -> (+ identity | downsample conv -> BN) -> [ReLU], with the BatchNorm layers between two
 * convolutions folded into the convolutions' operand fetch and epilogue (batch statistics from the producer's epilogue, normalise + ReLU in the consumer's
 * fetch, the BatchNorm backward as a per-channel affine map in the producer's dgrad / wgrad fetch).  Replaces ~12 p3d_conv2d_* / p3d_bn_* calls per direction.
 * Layouts: NCHW fp32.  conv[0..nconv-1] is the main chain, conv[3] the 1x1 downsample conv (has_downsample); every conv is bias-free.
 * Per conv i the caller owns: c[i] (raw conv output, kept for backward), a[i] (the ReLU output that feeds conv i+1, kept for backward; i < nconv-1), table[i] ([K_i][8] floats: the BN's forward constants {sc, sh, mean, invstd}
 * written by forward, its backward map {A, B, K, 0} written by backward), and for backward da[i] (gradient w.r.t. the ReLU output that feeds conv i+1; i < nconv-1),
 * gbuf (like out: dout * [out > 0]; with an identity shortcut it becomes dx in place) and dx (input gradient; only with a downsample branch).
 * Parameter gradients dw / dgamma / dbeta are written, or added onto what is there when accumulate_grads != 0 (the flat gradient buffer).  Running statistics
 * are updated in forward (momentum, unbiased variance), as p3d_bn_train_fwd does. */
typedef struct p3d_block_desc {
    int32_t nconv;              /* 2: BasicBlock (3x3, 3x3); 3: Bottleneck (1x1, 3x3 carrying stride / dilation, 1x1) */
    int32_t has_downsample;
    int32_t relu_out;           /* 0: -skip_relu on the last block of a stage (depthnet.py:176-186) */
    int32_t need_dx;
    int32_t accumulate_grads;
    int32_t masked;             /* 1: the convolutions of the main chain are partial convolutions (partial_conv.py:32-57; partial_depthnet.py:62-75,140-157): p3d_block_io.pix_in /
                                   pix_out carry their per-pixel factors; the downsample branch stays dense */
    int32_t reserved[2];
    float eps[4];
    float momentum[4];
    p3d_conv_desc conv[4];
} p3d_block_desc;

typedef struct p3d_block_io {
    const float* x;             /* block input  [N, C_in, H, W] */
    float* out;                 /* block output [N, K_last, Ho, Wo] */
    const float* w[4];
    const void* wimg[4];        /* pre-split weight images (p3d_fx_weight_images) of w[i] for the forward pass / the data gradient, or NULL: the kernels split */
    const void* wimgT[4];       /*   the fp32 weights on the fly.  The caller rebuilds an image whenever its weight changes. */
    float* c[4];
    void* aimg[4];              /* activation image (p3d_block_image_bytes(b, N, K_i, Ho_i * Wo_i) bytes: an fp32 row image in a dense block, three bf16 planes in a masked one) of a[i] = relu(bn_i(c[i])), i < nconv-1: written by
                                   forward; read by conv i+1 in forward and by its weight gradient in backward.  a[i] itself never exists as fp32.
                                   aimg[3]: read by nothing in an aligned block.  In a RAGGED block (p3d_block_any_enable) it carries the plane image of the block input x
                                   (p3d_block_image_bytes(b, N, C_in, H * W) bytes): written once by p3d_block_fwd, which feeds conv 0 and the downsample conv from it, and read by
                                   their weight gradients in p3d_block_bwd -- the caller keeps it between the two calls. */
    float* table[4];
    const float* gamma[4];
    const float* beta[4];
    float* running_mean[4];     /* may be NULL (no running statistics) */
    float* running_var[4];
    /* backward only */
    const float* dout;
    float* gbuf;                /* may be NULL when the block has a downsample branch and out_mask is given (g is then never needed as a tensor) */
    void* dcimg[4];             /* scratch, one per convolution (slot 3: the downsample branch): image of d c_i, the gradient w.r.t. conv i's raw output
                                   (p3d_block_image_bytes(b, N, K_i, Ho_i * Wo_i) bytes: an fp32 row image in a dense block, three bf16 planes in a masked one); read by conv i's weight gradient and data gradient */
    float* da[4];
    float* dx;
    float* dw[4];
    float* dgamma[4];
    float* dbeta[4];
    /* forward + backward, optional (NULL: backward reads `out`): one byte per four consecutive output elements, bit e = [out[4 i + e] > 0]; written by
       p3d_block_fwd of a block that ends in a ReLU, read by p3d_block_bwd instead of `out` (N * K_last * Ho * Wo / 4 bytes) */
    unsigned char* out_mask;
    /* masked blocks (p3d_block_desc.masked), conv i of the main chain: pix_in[i] = mask_in [N][1][H_i][W_i] of its input pixels, pix_out[i] = the renormalisation
       factor `mult` [N][1][Ho_i][Wo_i] of its output pixels (p3d_mask_count).  y_i = conv_i(a_{i-1} * pix_in[i]) * pix_out[i]. */
    const float* pix_in[4];
    const float* pix_out[4];
} p3d_block_io;

/* 1 when every convolution of the block can run on the fused kernels (dense, channel counts in steps of 16 and >= 64, four-pixel-aligned rows, maps of a
 * multiple of 16 pixels, stride <= 2 and never on a 1x1 of the main chain) */
int32_t p3d_block_supported(const p3d_block_desc* b);
/* The executor at any map width (default OFF; P3D_BLOCK_ANY=1 in the environment turns it on; independent of every p3d_x3_any_* switch).  Returns the previous setting.
 * While it is on, p3d_block_supported / p3d_block_* also take a RAGGED block: a dense block (masked == 0) that is refused only for its map size (H * W or Ho * Wo no multiple
 * of 4, rows of no multiple of 4 pixels: the 129 / 65 / 33 / 17 maps of the default 257 crop), every convolution of which, downsample included, has stride 1, whole weights,
 * channel counts in steps of 16 and >= 64 and a map of >= 16 pixels.  Aligned blocks run exactly what they run with the switch off; masked blocks at such maps stay refused, and
 * so do strided blocks under this switch (they have one of their own: p3d_block_any_strided_enable, below).  For a ragged block: every image is three bf16 planes (p3d_block_image_bytes: 6 B per element), io->aimg[3] holds the image of x (see there),
 * io->out_mask is not used (backward reads `out`), io->gbuf is required whenever relu_out, and the convolutions run on the ragged image-fed instances of the x3 kernels,
 * the BatchNorm sums in their epilogues (p3d_fx_conv_any_sums_instances), never split along K.  DESIGN.md section 3, "Residual blocks at any map width". */
int32_t p3d_block_any_enable(int32_t on);
int32_t p3d_block_any_supported(const p3d_block_desc* b);       /* 1: p3d_block_supported admits b, as a ragged block of either kind (host-only; 0 while its switch is off and for every aligned block) */
/* Ragged blocks that carry a STRIDE-2 convolution -- layer2.0 / layer3.0 of the ResNets at the default 257 crop (default OFF; P3D_BLOCK_ANY_STRIDED=1 in the environment
 * turns it on; a switch of its own: independent of p3d_block_any_enable, of p3d_x3_any_strided_enable, which the executor never reads, and of every other switch).
 * Returns the previous setting.  Alone it admits exactly the ragged blocks with a stride-2 slot; p3d_block_any_enable alone admits exactly the ones without.  The rule
 * of a stride-1 slot is p3d_block_any_enable's; a stride-2 slot needs the image-fed ragged forward and weight gradient to take it, the stride-2 class launches
 * (p3d_conv2d_dgrad_strided_any_supported's rule at 64 channels), whole weights, channel counts in steps of 16 and an OUTPUT map of >= 16 pixels; a 1x1 stride 2 only as
 * the downsample conv.  Masked strided blocks at such maps stay refused.  The block is a ragged block in every other respect (plane images, io->aimg[3], no mask bytes,
 * gbuf).  Forward: every convolution image-fed with the statistics epilogue, as in a stride-1 ragged block.  Backward: a stride-2 data gradient is one image-fed
 * ragged launch per parity class into tight class planes in the workspace (p3d_block_workspace_bytes covers them), finished for a main-chain slot by
 * block_strided_join_any_kernel -- one pass that writes da[i - 1] and takes the BatchNorm-backward sums of the layer in front -- and for conv 0 / the downsample conv by
 * dgrad_interleave_rows_kernel.  DESIGN.md section 3, "Strided residual blocks at any map width". */
int32_t p3d_block_any_strided_enable(int32_t on);
/* TEST HOOK (tests/test_block_anysize_strided_gpu.py, tools/train_anysize_bench.py; nothing in the package calls it): block_strided_join_any_kernel alone.
 * g[n][ch][hi][wi] = stage[cls * cls_stride + ((n C + ch) hc + hi / 2) wc + wi / 2] as p3d_dgrad_interleave lays the planes out (a class whose bit in live_mask is clear
 * gives +0 and is not read), and partial[ch][s][0 .. 2] = (sum gg, sum gg (c - mean), 0) over images n = s, s + split, ... with gg = g * [c * sc + sh > 0],
 * {sc, sh, mean} = table[ch][0 .. 2] (table [C][8] floats, c laid out like g, partial [C][split][3] doubles).  1 <= split <= min(N, 64); N C H W < 2^31. */
int32_t p3d_block_strided_join(const float* stage, const float* c, const float* table, float* g, double* partial, int32_t N, int32_t C, int32_t H, int32_t W,
                               size_t cls_stride, int32_t live_mask, int32_t split, void* stream);
int32_t p3d_block_workspace_bytes(const p3d_block_desc* b, size_t* main_bytes, size_t* side_bytes);
int32_t p3d_block_fwd(const p3d_block_desc* b, const p3d_block_io* io, void* workspace, size_t workspace_bytes, void* stream);
/* side_stream: NULL, or a second stream for the weight-gradient kernels (ordered by events inside the call; the caller joins the streams before it reads dw) */
int32_t p3d_block_bwd(const p3d_block_desc* b, const p3d_block_io* io, void* workspace, size_t workspace_bytes, void* side_workspace, size_t side_bytes,
                      void* stream, void* side_stream);

/* The same block on the fp16 NHWC kernels of -half_acc (depth_train.py:73-83,413-449): one call per block and direction over p3d_hconv2d_* / p3d_hbn_train_*,
 * instead of one Python-level call per layer (the fp16 step is bound by the host's enqueue work).  Tensors are fp16 NHWC unless typed otherwise; the descriptor is the
 * fp32 block's (channel counts of a convolution = the padded counts of its fp16 tensors). */
typedef struct p3d_hblock_io {
    const void* x;              /* block input */
    void* out;                  /* block output */
    const void* w_krsc[4];      /* fp16 forward weight images (p3d_weight_images_f16*) */
    const void* w_crsk[4];      /* fp16 data-gradient weight images */
    void* c[4];                 /* raw conv outputs */
    void* a[4];                 /* a[i] = relu(bn_i(c[i])), i < nconv-1; a[3] = bn_ds(c[3]), the shortcut of a downsample branch */
    float* coef[4];             /* [K_i][4] fp32 per BatchNorm: written by forward, read by backward */
    const float* gamma[4];
    const float* beta[4];
    float* running_mean[4];
    float* running_var[4];
    /* backward only */
    const void* dout;
    void* dc[4];                /* scratch: gradient w.r.t. c[i] */
    void* da[4];                /* scratch: gradient w.r.t. a[i], i < nconv-1; da[3]: the gradient that enters the shortcut (with an identity shortcut it becomes dx) */
    void* dx;                   /* gradient w.r.t. x with a downsample branch (identity: da[3]) */
    float* dw[4];               /* fp32 master gradients */
    float* dgamma[4];
    float* dbeta[4];
    int32_t c_real[4];          /* real (unpadded) input channels of conv i */
    void* out_mask;             /* or NULL: P * K_last / 8 bytes written by forward (bit = [out > 0]), read by backward in place of `out` (with p3d_hblock_fuse_sums(1)) */
} p3d_hblock_io;
int32_t p3d_hblock_workspace_bytes(const p3d_block_desc* b, size_t* main_bytes, size_t* side_bytes);
/* BatchNorm sums of the block's layers from the conv epilogues (1, the default) or from stand-alone passes (0: bit-identical to
 * the per-layer entry points); on < 0 queries.  Returns the previous setting. */
int32_t p3d_hblock_fuse_sums(int32_t on);
int32_t p3d_hblock_fwd(const p3d_block_desc* b, const p3d_hblock_io* io, void* workspace, size_t workspace_bytes, void* stream);
int32_t p3d_hblock_bwd(const p3d_block_desc* b, const p3d_hblock_io* io, void* workspace, size_t workspace_bytes, void* side_workspace, size_t side_bytes,
                       void* stream, void* side_stream);

/* Pre-split weight images for p3d_block_io.wimg / wimgT: every fp32 weight as three bf16 pieces (hi + mid + lo = w exactly), laid out as the 12 KB LDS tile
 * each (filter tap, 128-channel tile, 16-deep K step) of the conv kernels consumes, so the weight operand costs the kernels no arithmetic.  w [K][C][R*S]. */
int32_t p3d_fx_weight_image_bytes(int32_t K, int32_t C, int32_t RS, size_t* fwd_bytes, size_t* bwd_bytes);
int32_t p3d_fx_weight_images(const float* w, int32_t K, int32_t C, int32_t RS, void* img_fwd, void* img_bwd, void* stream);
/* the same for many weights in ONE launch: jobs = device array of njobs records {const float* w; void* img_fwd; void* img_bwd; int32_t K, C, RS, pad;} (40 bytes each,
 * NULL image = skip that direction), blocks = grid width per job and direction */
int32_t p3d_fx_weight_images_batched(const void* jobs, int32_t njobs, int32_t blocks, void* stream);

/* Pre-split activation images: a fp32 NCHW tensor [N][C][HW] (C % 16 == 0, HW % 4 == 0) as three bf16 planes [N][C/16][HW][16] with hi + mid + lo == the fp32
 * value exactly -- the form in which the x3 convolution kernels take an operand without splitting it (16-B copies into LDS whatever the filter tap).
 * mode 0: the tensor x itself; 1: relu(x * sc + sh) (depthnet.py:98-105: relu(bn(conv))); 2: A * (masked ? x * [x2 * sc + sh > 0] : x) + B * x2 + K, the
 * BatchNorm-backward map of the gradient x at the raw conv output x2.  table: the layer's [C][8] floats {sc, sh, mean, invstd, A, B, K, 0} as p3d_block_io.table. */
size_t p3d_fx_act_image_bytes(int32_t N, int32_t C, int32_t HW);
int32_t p3d_fx_act_image(int32_t mode, const float* x, const float* x2, const float* table, int32_t masked, void* img, int32_t N, int32_t C, int32_t HW, void* stream);
/* Row images: the same tensor in the same channel-blocked rows, holding the fp32 value itself: [N][C/16][HW][16] floats, 4 * N * C * HW bytes.  Every filter tap and
 * stride still lands on an aligned row of 16 channels (64 B); the row-fed kernel instances cut a value into its three bf16 pieces between their fetch registers and
 * LDS, with the function the plane passes use, so every result is bit-identical to the plane-fed one.  Modes and arguments as p3d_fx_act_image.
 * p3d_fx_conv_*_rows: p3d_fx_conv_*_img on row images (x_rows / dy_rows from p3d_fx_row_image); dense convolutions that p3d_fx_conv_img_supported admits, same
 * workspace (p3d_fx_conv_img_workspace_bytes).
 * p3d_block_image_bytes: bytes of one p3d_block_io.aimg / dcimg buffer of N x C x HW elements for this block: 4 per element for a dense block, 6 for a masked one
 * (and for every block under p3d_fx_tune(6, 1), and for a ragged block: p3d_block_any_enable). */
size_t p3d_fx_row_image_bytes(int32_t N, int32_t C, int32_t HW);
int32_t p3d_fx_row_image(int32_t mode, const float* x, const float* x2, const float* table, int32_t masked, void* img, int32_t N, int32_t C, int32_t HW, void* stream);
int32_t p3d_fx_conv_fwd_rows(const p3d_conv_desc* d, const void* x_rows, const float* w, const void* wimg, const float* bias, float* y, void* workspace,
                             size_t workspace_bytes, void* stream);
int32_t p3d_fx_conv_dgrad_rows(const p3d_conv_desc* d, const void* dy_rows, const float* w, const void* wimgT, float* dx, void* workspace, size_t workspace_bytes,
                               void* stream);
int32_t p3d_fx_conv_wgrad_rows(const p3d_conv_desc* d, const void* dy_rows, const float* x, const void* x_rows, float* dw, void* workspace, size_t workspace_bytes,
                               void* stream);
size_t p3d_block_image_bytes(const p3d_block_desc* b, int32_t N, int32_t C, int32_t HW);
/* The image passes that open a block's backward pass, alone (tests/test_row_images_gpu.py): d c = A g + B c + K, g = x with the mask bytes applied (gmask: bit e of byte i
 * lets element 4 i + e pass; NULL: none), the constants finalized in the prologue from fp64 partial sums [C][nrows][3] = (sum g, sum g (c_a - mean_a), sum g (c_b - mean_b))
 * and the tables' mean / invstd; d gamma and d beta are written.  c_b NULL: one image (side a); otherwise both images in one pass.  rows: 0 three planes, 1 row images. */
int32_t p3d_fx_open_images(int32_t rows, const float* x, const unsigned char* gmask, const double* partial, int32_t nrows, double count, const float* c_a, const float* table_a,
                           const float* gamma_a, float* dgamma_a, float* dbeta_a, void* img_a, const float* c_b, const float* table_b, const float* gamma_b, float* dgamma_b,
                           float* dbeta_b, void* img_b, int32_t N, int32_t C, int32_t HW, void* stream);
/* The three passes of a convolution on image operands (what p3d_block_* launches inside a block).  pass: 0 forward, 1 data gradient, 2 weight gradient.
 * wimg / wimgT: the p3d_fx_weight_images image of w for that pass, or NULL (built into the workspace).  wgrad: x (fp32) is read when x_img is NULL. */
size_t p3d_fx_conv_img_workspace_bytes(const p3d_conv_desc* d, int32_t pass);
int32_t p3d_fx_conv_img_supported(const p3d_conv_desc* d);      /* bit 0 / 1 / 2: forward / data gradient / weight gradient can take image operands */
int32_t p3d_fx_conv_fwd_img(const p3d_conv_desc* d, const void* x_img, const float* w, const void* wimg, const float* bias, float* y, void* workspace,
                            size_t workspace_bytes, void* stream);
int32_t p3d_fx_conv_dgrad_img(const p3d_conv_desc* d, const void* dy_img, const float* w, const void* wimgT, float* dx, void* workspace, size_t workspace_bytes,
                              void* stream);
int32_t p3d_fx_conv_wgrad_img(const p3d_conv_desc* d, const void* dy_img, const float* x, const void* x_img, float* dw, void* workspace, size_t workspace_bytes,
                              void* stream);
/* The same at any map width (the 129 / 65 / 33 / 17 maps of the reference's default 257 crop): mode-0 activation images of tensors whose H * W is no multiple of 4, and
 * the three passes of a DENSE convolution with a whole weight tensor on them -- the ragged image-fed instances of the x3 kernels ("Image operands
 * at any map width").
 * p3d_fx_act_image_any: mode 0 only; the bytes, layout and size (p3d_fx_act_image_bytes) of p3d_fx_act_image at any HW; C % 16 == 0, img 16-B aligned.
 * p3d_fx_conv_img_any_supported: bit 0 / 1 / 2 as p3d_fx_conv_img_supported -- what the ragged image-fed instances admit, whatever any switch says: each pass's rule at the
 * per-layer thresholds (96 result channels; the weight gradient 96 on both sides), C % 16 == 0, K % 16 == 0, Ho * Wo >= 16, no channel window, the data gradient at stride 1
 * only.  They admit aligned shapes too (and are correct there); those belong on the entries above.
 * p3d_fx_conv_{fwd,dgrad,wgrad}_img_any: the signatures of their _img siblings.  No fp32 operand: the weight gradient needs BOTH images (x is ignored).  Each checks its
 * bit, its workspace (p3d_fx_conv_img_any_workspace_bytes; P3D_EWORKSPACE when short) and the 16-B alignment of its base pointers, and counts as an x3 launch.
 * p3d_x3_any_images_enable (default OFF; P3D_X3_ANY_IMAGES=1 in the environment turns it on; independent of p3d_x3_any_enable and p3d_x3_any_partial_enable): the
 * setting callers that feed images consult (ops_block.ConvImagesFn routes a convolution the aligned query refuses to these entries while it is on).  No entry point of the
 * library looks at it: p3d_conv2d_*, the block executor and the entries above launch what they launch without it.  Returns the previous setting. */
int32_t p3d_x3_any_images_enable(int32_t on);
int32_t p3d_fx_conv_img_any_supported(const p3d_conv_desc* d);
size_t p3d_fx_conv_img_any_workspace_bytes(const p3d_conv_desc* d, int32_t pass);
int32_t p3d_fx_act_image_any(const float* x, void* img, int32_t N, int32_t C, int32_t HW, void* stream);
int32_t p3d_fx_conv_fwd_img_any(const p3d_conv_desc* d, const void* x_img, const float* w, const void* wimg, const float* bias, float* y, void* workspace,
                                size_t workspace_bytes, void* stream);
int32_t p3d_fx_conv_dgrad_img_any(const p3d_conv_desc* d, const void* dy_img, const float* w, const void* wimgT, float* dx, void* workspace, size_t workspace_bytes,
                                  void* stream);
int32_t p3d_fx_conv_wgrad_img_any(const p3d_conv_desc* d, const void* dy_img, const float* x, const void* x_img, float* dw, void* workspace, size_t workspace_bytes,
                                  void* stream);
/* The STRIDE-2 data gradient of a dense convolution on an image operand at any map side (entries of their own: the two above keep refusing stride 2).  One launch of the
 * image-fed ragged store instance per live, non-empty parity class of the input into tight class planes in the workspace -- the geometry and the planes of
 * p3d_x3_any_strided_enable's fp32-fed class launches --, then dgrad_interleave_rows_kernel: dx = (or +=, by d->accumulate) the gradient, +0 at the pixels no tap
 * reaches (which keep what they held under accumulate).
 * _supported: 1 for a well-formed stride-2 descriptor that p3d_conv2d_dgrad_strided_any_supported's rule admits at 32 input channels, with C % 16 == 0 and K % 16 == 0.
 * _workspace_bytes: the room for the data-gradient weight image plus four class planes of N C ceil(H / 2) ceil(W / 2) floats (rounded up to 4), each part on a 256-B
 * line; 0 where _supported answers 0.  dy_img: p3d_fx_act_image_any of dy; wimgT: the p3d_fx_weight_images data-gradient image of w, or NULL (built into the workspace).
 * The image, the weight image and the workspace on 16-B lines; P3D_EWORKSPACE when the workspace is short.  Counts as an x3 launch. */
int32_t p3d_fx_conv_dgrad_strided_img_any_supported(const p3d_conv_desc* d);
size_t p3d_fx_conv_dgrad_strided_img_any_workspace_bytes(const p3d_conv_desc* d);
int32_t p3d_fx_conv_dgrad_strided_img_any(const p3d_conv_desc* d, const void* dy_img, const float* w, const void* wimgT, float* dx, void* workspace, size_t workspace_bytes,
                                          void* stream);
/* What the x3 path launched: one record per launch of a forward / data-gradient convolution kernel, written where the launch is made (every caller: p3d_conv2d_*, the
 * image entries, the inference entries, p3d_block_*, p3d_fx_conv_fused).  Host-side bookkeeping only.  A record is P3D_FX_LAUNCH_FIELDS int32:
 *   [0] kernel: 0 fx_conv_kernel (128-row tile), 96 / 64: fx16_conv_kernel with that tile
 *   [1] AMODE (1: image-fed)   [2] PRO (4: the operand times its per-pixel factor)   [3] EPI: the epilogue code the instance was compiled with -- on the fx16 kernel a
 *       factor code is the instance without the factor (0 store, 1 statistics, 2 backward sums, 4 factor, 5 / 6 factor with 1 / 2, 7 factor image-fed, 8 inference,
 *       9 inference with factor)   [4] TAPI (1: taps innermost), as launched   [5] RAG (any map width)   [6] ROWS (fp32 row image)  -- the kernel's template arguments
 *   [7] grid.x   [8] grid.y (split-K slabs)   [9] grid.z (parity classes of a strided data gradient in one launch)   [10] kchunk: K steps per slab, 0 unsplit
 *   [11] the pass that followed: 0 none, 1 fx_reduce_kernel<0>, 2 fx_reduce_kernel<1>, 3 fx_reduce_kernel<2>, 4 fx_reduce_any_kernel, 5 dgrad_interleave_rows_kernel (the
 *        class launches of a stride-2 data gradient under p3d_x3_any_strided_enable, of p3d_fx_conv_dgrad_strided_img_any and of a strided ragged block's conv 0 /
 *        downsample conv: on the record of the LAST class launch), 6 block_strided_join_any_kernel (a strided ragged block's main-chain data gradient, likewise)
 *        [12] its grid.y (the image groups of fx_reduce_kernel = the rows of its partial sums; 1 for fx_reduce_any_kernel; 0 with [11] 0, 5 or 6)
 *   [13..15] 0
 * p3d_fx_launch_log: copies the records since the last reset into out, oldest first, at most max_records of them (the library keeps the first 256), and returns how
 * many launches there were since then -- more than max_records, or than 256, shows as a count above what was copied.  reset != 0: the log starts anew afterwards.
 * out may be NULL with max_records 0.
 * p3d_fx_conv_instances: every compiled instance of the two kernels as P3D_FX_INSTANCE_FIELDS int32 each -- fields [0..6] of a record --, generated from the lists
 * the instances are compiled from; returns their number (copies at most max_records).  Two instances are NOT in it: the ragged image-fed ones with the BatchNorm
 * epilogues, which have a list and a hook of their own (p3d_fx_conv_any_sums_instances, below). */
#define P3D_FX_LAUNCH_FIELDS 16
#define P3D_FX_INSTANCE_FIELDS 7
int32_t p3d_fx_launch_log(int32_t* out, int32_t max_records, int32_t reset);
int32_t p3d_fx_conv_instances(int32_t* out, int32_t max_records);
/* The instances p3d_fx_conv_instances leaves out, in the same record shape: the ragged image-fed fx_conv_kernel<1, 0, 1 | 2, false, true, false> with the BatchNorm
 * epilogues, which the ragged residual blocks launch (p3d_block_any_enable).  A list of their own in csrc/p3d_fx.hip; p3d_fx_launch_log records their launches like any
 * other ([3] 1 / 2, [5] 1).  tests/test_block_anysize_gpu.py runs each alone. */
int32_t p3d_fx_conv_any_sums_instances(int32_t* out, int32_t max_records);
/* TEST HOOK (tests/test_fx_instances_gpu.py; nothing in the package calls it): one forward (pass 0) or data-gradient (pass 1) call of the x3 kernels with any of the
 * fusions the block executor and the inference entries use, so that each can be checked alone.  src: x (forward) / dy (data gradient), fp32, ignored when f->act_img is
 * set; out: y / dx.  The fields of p3d_fx_fuse, NULL / 0 = not used:
 *   act_img  the operand as a p3d_fx_act_image image (rows = 1: a p3d_fx_row_image one; ragged = 1: p3d_fx_act_image_any -- with `partial` the ragged BatchNorm
 *            instances of p3d_fx_conv_any_sums_instances: dense, one unsplit launch, rows from p3d_fx_conv_fused_partial_rows_any; the forward at stride 2 too,
 *            with ceil(N Ho Wo / 128) rows -- that query keeps answering 0 for stride 2; the data gradient stride 1 only)
 *   wimg     the p3d_fx_weight_images image of w for this pass, or NULL: built into the workspace
 *   partial  [p3d_fx_conv_fused_partial_rows][M][2] partial sums per result channel: forward (sum y, sum y^2); data gradient (sum g, sum g (ep_c - mean)) with
 *            g = dx * [ep_c * sc + sh > 0], ep_c laid out like dx and ep_tab [M][8] = {sc, sh, mean, ...}.  The summed value is the convolution (+ bias) (* emask);
 *            what an unsplit accumulating call adds to it is not in the sums
 *   pmask, emask  partial convolution: per-pixel factor of the operand ([N][1][.][.] of src; fp32 operand only -- an image carries it) and of the result
 *   acc_src, acc_mask  data gradient with d->accumulate, stride 1, unsplit: out = dgrad + acc_src * [bit (i & 3) of acc_mask[i >> 2]] instead of out += dgrad
 *   infer, res, relu   forward with a folded weight image: out = relu?(conv * emask + bias (+ out when accumulating) (+ res))
 * Checks the null arguments, the descriptor and the shape rule of the pass (32 result channels; with a factor the partial-convolution rule) and passes everything else to
 * the launcher, which refuses the combinations it has no instance for (P3D_EINVAL with a message).  Does not zero the pixels of a strided 1x1 data gradient that no tap
 * reaches, and does not count in p3d_conv_path_stats.  Workspace: p3d_fx_conv_fused_workspace_bytes (under the p3d_fx_tune settings in force).  Both queries are
 * host-only and return 0 for a pass, a descriptor or a shape the hook refuses (the rule without a factor). */
typedef struct p3d_fx_fuse {
    const void* act_img;
    const void* wimg;
    float* partial;
    const float* ep_c;
    const float* ep_tab;
    const float* pmask;
    const float* emask;
    const float* acc_src;
    const unsigned char* acc_mask;
    const float* res;
    int32_t rows, infer, relu, ragged;
} p3d_fx_fuse;
size_t p3d_fx_conv_fused_workspace_bytes(int32_t pass, const p3d_conv_desc* d, int32_t ragged);
int32_t p3d_fx_conv_fused_partial_rows(int32_t pass, const p3d_conv_desc* d);
/* ... of a call with ragged = 1, an act_img and `partial` (dense, stride 1): such a call is ONE unsplit launch whatever the plan of the plain call, so its rows are the
 * 128-pixel tiles of the result.  0 as above. */
int32_t p3d_fx_conv_fused_partial_rows_any(int32_t pass, const p3d_conv_desc* d);
int32_t p3d_fx_conv_fused(int32_t pass, const p3d_conv_desc* d, const p3d_fx_fuse* f, const float* src, const float* w, const float* bias, float* out, void* workspace,
                          size_t workspace_bytes, void* stream);
/* TEST HOOK (tests/test_block_anysize_gpu.py; nothing in the package calls it): one image pass of mode 1 or 2 with the finalize step of its BatchNorm layer in the prologue, as
 * the block executor runs it.  any = 0: the aligned pass (p3d_fx_act_image's kernel; HW % 4 == 0); any = 1: the pass at any HW the ragged blocks use (plane images, C % 16 == 0,
 * img 16-B aligned).  Modes, x, x2, table, masked as p3d_fx_act_image.  kind 0: the constants come from `table` and the arguments behind `kind` are ignored.  Otherwise they are computed from partial sums,
 * every block in the same fixed order, and block x == 0 writes them out:
 *   kind 1 (mode 1)  partial = float [rows][C][2] (sum y, sum y^2): table {sc, sh, mean, invstd} and, if given, the running statistics (momentum, eps, unbiased variance)
 *   kind 2 (mode 2)  partial = float [rows][C][2] (sum g, sum g (c - mean)); table holds {sc, sh, mean, invstd}: d gamma, d beta written (added with `accumulate`)
 *   kind 3 (mode 2)  the same from double [C][rows][3], the second sum at index 1 + which
 * count = N * H * W of the layer. */
int32_t p3d_fx_act_image_fused(int32_t any, int32_t mode, const float* x, const float* x2, float* table, int32_t masked, void* img, int32_t N, int32_t C, int32_t HW,
                               int32_t kind, const void* partial, int32_t rows, int32_t which, double count, const float* gamma, const float* beta, float* running_mean,
                               float* running_var, float momentum, float eps, float* dgamma, float* dbeta, int32_t accumulate, void* stream);
/* TEST HOOK (tests/test_wgrad_plan_host.py; nothing in the package calls it), host-only: how the x3 kernels would run the weight gradient of d -- the plan every
 * weight-gradient entry, the block executor and the workspace queries read -- under the p3d_fx_tune settings in force.  Nothing is launched and no operand exists;
 * `operands` says what they would be:
 *   bit 0  dy is an activation image      bit 1  x is one      bit 2  the images are row images (p3d_fx_row_image)
 *   bit 3  dy has a per-pixel factor (a partial convolution's mult)      bit 4  x has one (mask_in)      bit 5  the kernels for any map width
 *   bit 6  d describes the stem instead (p3d_stem_wgrad: its N, C = Cin, H, W, K are read); bit 3 beside it: p3d_stem_wgrad_masked; no other bit
 * out receives P3D_FX_WGRAD_PLAN_FIELDS int32:
 *   [0] kernel family: 0 fx_wgrad_kernel (aligned maps), 1 fx_wgrad_any_kernel, 2 fx_wgrad_any_masked_kernel, 3 fx_wgrad_any_img_kernel
 *   [1] AIMG   [2] BIMG   [3] MASKED   [4] TAPS   [5] ROWS  -- the template arguments of fx_wgrad_kernel (0 for the other families)
 *   [6] filter taps per column tile: 0 one tap per block, 2 / 3 image-fed multi-tap layers with 64 input channels, 8 the stem
 *   [7] slabs the pixel reduction is cut into   [8] K steps (16 pixels) per slab   [9] grid.x   [10] grid.y   [11] grid.z   [12] block order (1: taps fastest)
 *   [13] 1: the slabs' columns are tap-major   [14] slab bytes, low 32 bits   [15] high 32 bits
 * Returns P3D_EINVAL, out untouched, for a malformed descriptor, a shape outside the weight-gradient rule of the x3 kernels (at 32 channels on either side, the least any
 * caller asks for; with bit 5 the rule without its width clauses; the stem: p3d_stem_supported's rule) and for operands no instance takes. */
#define P3D_FX_WGRAD_PLAN_FIELDS 16
int32_t p3d_fx_wgrad_plan(const p3d_conv_desc* d, int32_t operands, int32_t* out);
/* What the x3 weight gradient launched: one record per launch of a weight-gradient kernel, written where the launch is made (every caller: p3d_conv2d_wgrad on the x3
 * family, the image entries, p3d_block_bwd, p3d_stem_wgrad(_masked), p3d_fx_conv_wgrad_fused).  Host-side bookkeeping only, apart from p3d_fx_launch_log (which keeps the
 * forward / data-gradient launches).  A record is P3D_FX_WGRAD_LAUNCH_FIELDS int32:
 *   [0..15] the plan that was launched, in the layout of p3d_fx_wgrad_plan -- taken from the launch itself, not planned a second time
 *   [16] the finishing kernels that followed, as bits: 8 wgrad_reduce_kernel, 16 wgrad_reduce_tapm_kernel, 32 wgrad_reduce16_kernel, 64 wgrad_reduce16_tapm_kernel,
 *        128 slab_fold_kernel (then 8 or 16 over the 16 folded slabs) -- the finishing bits of p3d_conv_last_fp32_launch --, 256 fx_stem_dw_kernel (the stem)
 *   [17] accumulate: dw += instead of dw =
 *   [18..23] 0
 * p3d_fx_wgrad_launch_log behaves like p3d_fx_launch_log: copies the records since the last reset into out, oldest first, at most max_records of them (the library keeps
 * the first 256), returns how many launches there were since then, and with reset != 0 starts the log anew.  out may be NULL with max_records 0. */
#define P3D_FX_WGRAD_LAUNCH_FIELDS 24
int32_t p3d_fx_wgrad_launch_log(int32_t* out, int32_t max_records, int32_t reset);
/* TEST HOOK (tests/test_x3_wgrad_instances_gpu.py; nothing in the package calls it): one weight-gradient call of the x3 kernels with any operands, so that every
 * instance of fx_wgrad_kernel and the kernels for any map width can be checked alone.  dw (= or +=, by d->accumulate) = wgrad(dy * pmask, x * emask), into the input
 * channels [d->c_offset, d->c_offset + C) of a weight with d->c_total of them.  dy / x: the fp32 operands, ignored where the image is set.  The fields of
 * p3d_fx_wgrad_fuse, NULL / 0 = not used:
 *   dy_img, x_img  the operand as a p3d_fx_act_image image (rows = 1: p3d_fx_row_image ones; ragged = 1: p3d_fx_act_image_any)
 *   pmask, emask   partial convolution: per-pixel factor of dy ([N][1][Ho][Wo]) and of x ([N][1][H][W]); fp32 operands only -- an image carries its factor
 *   rows           the images are row images      ragged  the kernels for any map width
 * Checks the null arguments, the descriptor, the weight-gradient shape rule (32 channels on either side; ragged: without its width clauses) and the alignment: operands
 * and workspace on 16-B lines, dw on a 4-B line.  Everything else is the launcher's: operands no instance takes give P3D_EINVAL, a short workspace P3D_EWORKSPACE, both
 * before anything is launched.  Does not count in p3d_conv_path_stats.  Workspace: p3d_fx_conv_wgrad_fused_workspace_bytes (host-only; under the p3d_fx_tune settings in
 * force; 0 for a descriptor or a shape the hook refuses). */
typedef struct p3d_fx_wgrad_fuse {
    const void* dy_img;
    const void* x_img;
    const float* pmask;
    const float* emask;
    int32_t rows, ragged;
} p3d_fx_wgrad_fuse;
size_t p3d_fx_conv_wgrad_fused_workspace_bytes(const p3d_conv_desc* d, const p3d_fx_wgrad_fuse* f);
int32_t p3d_fx_conv_wgrad_fused(const p3d_conv_desc* d, const p3d_fx_wgrad_fuse* f, const float* dy, const float* x, float* dw, void* workspace, size_t workspace_bytes,
                                void* stream);

/* Inference with eval-mode BatchNorm folded into the convolutions (infer.py): s = gamma / sqrt(var + eps), w' = w * s, b' = beta - mean * s (+ s * conv bias).
 * p3d_fx_fold_bn_images: ONE launch for a table of jobs (device array of p3d_fold_job); per job kind 0 writes the forward weight image of w' over the input
 * channels [c_offset, c_offset + C) of a weight with c_total of them -- the image p3d_fx_weight_images builds from the folded fp32 weight, bit for bit --, kind 1 the
 * folded fp32 weight [K][C][RS] itself (the 7x7 stem: input of p3d_stem_weight_image), kind 2 the fp16 forward image [K][RS][Cpad] of w' (-half_acc: the image
 * p3d_weight_images_f16 builds from the folded fp32 weight, bit for bit; channels C .. Cpad - 1 are 0); bias_out (or NULL) receives b'.  gamma == NULL: no BatchNorm
 * (s = 1, b' = the conv bias or 0).  Kind 3 writes the MXFP8 image of w' (infer.fold_fp8, p3d_f8conv2d_fwd_infer): per (row k, tap, 32 input channels) one block
 * by OCP MX v1.0 with e4m3fn elements -- e = floor(log2(amax)) from the exponent bits, scale byte E8M0 = clamp(e - 8 + 127, 0, 254), X = 2^(byte - 127),
 * q = e4m3fn(RNE(clamp(w' / X, -448, 448))) (amax 0: byte 0, elements 0) -- out holds the elements [K][RS][Cpad] (bytes), then the scale bytes [K][RS][Cpad / 32]
 * (p3d_f8conv2d_weight_bytes in all); channels C .. Cpad - 1 are 0.  Kind 4 writes the fp16 DATA-GRADIENT image [Cpad][RS][K] of w' (training through a frozen BatchNorm under
 * -half_acc, ops_frozen.py): the `crsk` image p3d_weight_images_f16 builds from the folded fp32 weight (kind 1), bit for bit; Cpad in `reserved` as for kind 2,
 * channels C .. Cpad - 1 are 0.  Any other kind value is taken as kind 1.  Kinds may be mixed in one table.  blocks: grid width per job.  K <= 2048. */
typedef struct p3d_fold_job {
    const float* w;             /* conv weight [K][c_total][RS] */
    const float* conv_bias;     /* [K] or NULL */
    const float* gamma;         /* BatchNorm weight, bias, running mean, running variance [K]; all NULL: no BatchNorm */
    const float* beta;
    const float* mean;
    const float* var;
    void* out;                  /* kind 0: p3d_fx_weight_image_bytes(K, C, RS) forward bytes; kind 1: K * C * RS floats; kinds 2 and 4: K * RS * Cpad halves */
    float* bias_out;            /* [K] or NULL */
    int32_t K, C, RS, c_offset, c_total, kind;
    float eps;
    int32_t reserved;           /* kinds 2 and 4: Cpad, the padded channel count of the fp16 image (>= C, multiple of 8); kind 3: Cpad (>= C, multiple of 32); kinds 0 / 1: unused */
} p3d_fold_job;
int32_t p3d_fx_fold_bn_images(const void* jobs, int32_t njobs, int32_t blocks, void* stream);
/* y = conv(x, w') + b' (+ y when d->accumulate) (+ res) (then ReLU when relu != 0) from a folded forward weight image of exactly this descriptor's C input channels
 * (wimg_bytes must be its p3d_fx_weight_image_bytes; c_offset 0, c_total C: a channel window of a wider weight has an image of its own).  The activation comes as the
 * fp32 x or, when x_img != NULL, as its p3d_fx_act_image; bias / res may be NULL.  Split-K launches apply the same epilogue after summing their slabs.
 * supported: the forward of d runs on these kernels (image_fed: with an activation image); channel counts down to 32. */
int32_t p3d_fx_conv_fwd_infer_supported(const p3d_conv_desc* d, int32_t image_fed);
size_t p3d_fx_conv_fwd_infer_workspace_bytes(const p3d_conv_desc* d);
int32_t p3d_fx_conv_fwd_infer(const p3d_conv_desc* d, const float* x, const void* x_img, const void* wimg, size_t wimg_bytes, const float* bias, const float* res,
                              int32_t relu, float* y, void* workspace, size_t workspace_bytes, void* stream);
/* The same at ANY map width (the reference's default -side_in 257: maps of 65, 33 and 17): y = conv(x, w') + b' (+ y when d->accumulate) (+ res) (then ReLU) on the
 * "ragged" instances of the x3 forward, which take their four pixels element by element and store with 16-B or dword accesses as the address allows.  fp32 x only (no
 * activation image); wimg is the same folded image (p3d_fx_fold_bn_images kind 0, the same byte-size check); only the BASE pointers x, y, res, wimg and workspace need
 * 16-B alignment.  Split-K launches sum their slabs in a scalar pass with the same epilogue.  Workspace: p3d_fx_conv_fwd_infer_any_workspace_bytes.
 * supported: p3d_fx_conv_fwd_infer_supported(d, 0) without its W % 4 == 0 and Wo % 4 == 0 (C % 16 == 0, C >= 32, K >= 32, odd square filter, stride <= 2, no channel
 * window, accumulate 0 / 1, fewer than 2^31 elements per tensor); host only. */
int32_t p3d_fx_conv_fwd_infer_any_supported(const p3d_conv_desc* d);
size_t p3d_fx_conv_fwd_infer_any_workspace_bytes(const p3d_conv_desc* d);
int32_t p3d_fx_conv_fwd_infer_any(const p3d_conv_desc* d, const float* x, const void* wimg, size_t wimg_bytes, const float* bias, const float* res, int32_t relu,
                                  float* y, void* workspace, size_t workspace_bytes, void* stream);
/* The same for a PARTIAL convolution (partial_conv.py:32-57) with its BatchNorm folded: y = relu?(conv(x * mask_in, w') * mult + b' + res), the factor applied before
 * b' (an empty window, mult = 0, gives relu(b' + res), what the reference's BatchNorm makes of the 0 its partial conv writes there).  mask_in [N][1][H][W], mult
 * [N][1][Ho][Wo] (ops.mask_count); fp32 x only, 16-B aligned operands, wimg as above; bias / res may be NULL.  Workspace: p3d_fx_conv_fwd_infer_workspace_bytes.
 * supported: the forward of d runs on the masked x3 kernels (channel counts down to 64, no channel window, no accumulate; 0 under P3D_FX_MASKED=0); host only. */
int32_t p3d_fx_conv_fwd_infer_masked_supported(const p3d_conv_desc* d);
int32_t p3d_fx_conv_fwd_infer_masked(const p3d_conv_desc* d, const float* x, const void* wimg, size_t wimg_bytes, const float* bias, const float* mask_in,
                                     const float* mult, const float* res, int32_t relu, float* y, void* workspace, size_t workspace_bytes, void* stream);
/* The partial convolution at ANY map width: p3d_fx_conv_fwd_infer_masked on the ragged instances (PRO 4: mask_in fetched element by element at the positions of x, from
 * its one plane per image; mult applied per element in the store, each element with its own image; split-K: the scalar slab pass applies mult before b').  Same
 * arguments and the same order factor, b', res, ReLU, so an empty window gives exactly relu(b' + res).  Only the BASE pointers need 16-B alignment.
 * supported: p3d_fx_conv_fwd_infer_masked_supported without its W % 4 == 0 and Wo % 4 == 0 (C % 16 == 0, C >= 32, K >= 64, odd square filter, stride <= 2, no channel
 * window, accumulate 0; 0 under P3D_FX_MASKED=0 and for a NULL d); host only.  Workspace: p3d_fx_conv_fwd_infer_masked_any_workspace_bytes (the weight image's room,
 * then the split-K slabs, each on a 16-B line). */
int32_t p3d_fx_conv_fwd_infer_masked_any_supported(const p3d_conv_desc* d);
size_t p3d_fx_conv_fwd_infer_masked_any_workspace_bytes(const p3d_conv_desc* d);
int32_t p3d_fx_conv_fwd_infer_masked_any(const p3d_conv_desc* d, const float* x, const void* wimg, size_t wimg_bytes, const float* bias, const float* mask_in,
                                         const float* mult, const float* res, int32_t relu, float* y, void* workspace, size_t workspace_bytes, void* stream);
/* Stem tail at inference behind p3d_stem_fwd on a folded stem image: y = maxpool3x3s2(relu(c + bias[channel])) = relu(maxpool(c) + bias) (both monotone per
 * channel), no argmax output.  c [N][C][H][W] (H, W even), y [N][C][H/2][W/2]. */
int32_t p3d_stem_tail_infer(const float* c, const float* bias, float* y, int32_t N, int32_t C, int32_t H, int32_t W, void* stream);

/* The stem conv1 = Conv2d(Cin <= 4, K, 7, stride 2, padding 3) (depthnet.py:138) on the x3 kernels: restated as a 4x4 stride-1 convolution over a space-to-depth
 * image of the input (x'[c * 4 + pi * 2 + pj][i][j] = x[c][2 i + pi][2 j + pj], one 16-channel group).  p3d_stem_image: once per batch (forward and weight
 * gradient read it); p3d_stem_weight_image: once per weight update (workspace >= K * 256 floats).  H even, W % 8 == 0, K % 16 == 0, K <= 128. */
int32_t p3d_stem_supported(int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t K);
size_t p3d_stem_image_bytes(int32_t N, int32_t H, int32_t W);
size_t p3d_stem_weight_image_bytes(int32_t K);
size_t p3d_stem_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t K);
int32_t p3d_stem_image(const float* x, void* img, int32_t N, int32_t Cin, int32_t H, int32_t W, void* stream);
int32_t p3d_stem_weight_image(const float* w, int32_t K, int32_t Cin, void* wimg, void* workspace, size_t workspace_bytes, void* stream);
int32_t p3d_stem_fwd(const void* x_img, const void* wimg, float* y, int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t K, void* stream);
int32_t p3d_stem_wgrad(const float* dy, const void* x_img, float* dw, int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t K, int32_t accumulate, void* workspace,
                       size_t workspace_bytes, void* stream);
/* The same stem as a PARTIAL convolution (partial_conv.py:32-57; partial_depthnet.py:177, partial_fusionnet.py: conv(x * mask_in) * mult): mask_in [N][1][H][W] is multiplied
 * into the space-to-depth image, mult [N][1][H/2][W/2] scales the result in the forward epilogue and dy on its way into the weight gradient.  NULL factors = the dense stem. */
int32_t p3d_stem_masked_supported(int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t K);
int32_t p3d_stem_image_masked(const float* x, const float* mask_in, void* img, int32_t N, int32_t Cin, int32_t H, int32_t W, void* stream);
int32_t p3d_stem_fwd_masked(const void* x_img, const void* wimg, float* y, const float* mult, int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t K, void* stream);
/* The folded stem at ANY sides H, W >= 8 (inference; the reference's default -side_in 257).  A 7x7 / stride 2 / pad 3 conv of the input zero-extended to (Hp, Wp) >=
 * (H, W) equals, in its first (H - 1) / 2 + 1 rows and (W - 1) / 2 + 1 columns, the conv of the input itself: the added zeros are the conv's own padding.  So:
 *   p3d_stem_any_padded(H, W, &Hp, &Wp)   the smallest Wp >= W with Wp % 8 == 0, then the smallest even Hp >= H with (Hp / 2) (Wp / 2) % 16 == 0 (a supported pair maps
 *                                         to itself: 257 -> 264, 129 -> 136, 33 -> 40); returns 0 for a side below 8.  p3d_stem_any_supported: the padded pair passes
 *                                         p3d_stem_supported.  Both host only.  Every size query (p3d_stem_image_bytes, ...) takes the PADDED sides.
 *   p3d_stem_image_any(x, mask_in | NULL, img, N, Cin, H, W)   the space-to-depth image of the padded input (layout of p3d_stem_image at (Hp, Wp)); x and mask_in
 *                                         [N][1][H][W] are fetched as dwords checked against the true H and W, every pixel at or beyond them is an exact zero.
 *   p3d_stem_fwd(img, wimg, c, N, Cin, Hp, Wp, K)              the conv itself, called with the PADDED sides and never with the output factor: c [N][K][Hp/2][Wp/2]
 *                                         (p3d_conv_path_stats counts one x3 forward with the flops of the padded conv: +4.7 % at 257).
 *   p3d_stem_tail_infer_any(c, bias, mult | NULL, y, N, C, H, W)   y [N][C][Ho2][Wo2] = relu(maxpool3x3s2p1(c * mult) + bias), Ho = (H - 1) / 2 + 1, Ho2 = (Ho - 1) / 2 + 1
 *                                         (H, W: the TRUE input sides; c is read at the pitch Hp/2 x Wp/2, only rows < Ho and columns < Wo enter a window -- the pad
 *                                         columns hold real, non-zero conv outputs).  mult [N][1][Ho][Wo] dense (ops.mask_count) is multiplied in BEFORE the max: it
 *                                         stands for the epilogue factor of p3d_stem_fwd_masked.  c 16-B aligned; y is stored as dwords. */
int32_t p3d_stem_any_padded(int32_t H, int32_t W, int32_t* Hp, int32_t* Wp);
int32_t p3d_stem_any_supported(int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t K);
int32_t p3d_stem_image_any(const float* x, const float* mask_in, void* img, int32_t N, int32_t Cin, int32_t H, int32_t W, void* stream);
int32_t p3d_stem_tail_infer_any(const float* c, const float* bias, const float* mult, float* y, int32_t N, int32_t C, int32_t H, int32_t W, void* stream);
int32_t p3d_stem_wgrad_masked(const float* dy, const float* mult, const void* x_img, float* dw, int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t K, int32_t accumulate,
                              void* workspace, size_t workspace_bytes, void* stream);

/* Brackets every convolution launch (p3d_conv2d_* and the block executor) with HIP events on the stream it runs on, for bench.py's roofline line.
 * p3d_profile_collect synchronises and returns, per kind (0 forward, 1 data gradient, 2 weight gradient), the summed milliseconds, algorithmic flops and launches. */
int32_t p3d_profile_enable(int32_t on);      /* 0 off, 1 brackets, 2 brackets + the position where the conv kernel itself ended (p3d_profile_collect2's kernel_ms); returns the previous mode */
int32_t p3d_profile_collect(double* ms_by_kind, double* flops_by_kind, int64_t* launches_by_kind);
/* the same plus, per kind, the milliseconds of the conv kernels alone (without the split-K / slab sums queued behind them inside the bracket) */
int32_t p3d_profile_collect2(double* ms_by_kind, double* kernel_ms_by_kind, double* flops_by_kind, int64_t* launches_by_kind);

/* ------------------------------------------------------------------------------------------
 * BatchNorm2d (+ fused residual add and ReLU): nn.BatchNorm2d, F.relu, out + res
 *   depthnet.py:42-56,98-116,139,189-190  fusionnet.py:140
 * train:  y = act( (x-mean)*invstd*gamma + beta + res ), batch statistics (biased var for the
 *         normalisation, unbiased for running_var, momentum 0.1 by default, eps 1e-5)
 * res may be NULL; relu in {0,1}.  save_mean / save_invstd [C] are outputs kept for backward.
 * running_mean / running_var may be NULL (no update).
 * ------------------------------------------------------------------------------------------ */
size_t p3d_bn_workspace_bytes(int32_t N, int32_t C, int32_t HW);
int32_t p3d_bn_train_fwd(const float* x, const float* res, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, float* y, float* save_mean, float* save_invstd,
                         int32_t N, int32_t C, int32_t HW, float momentum, float eps, int32_t relu,
                         void* workspace, size_t workspace_bytes, void* stream);
/* Backward of the above.  y is the forward output (its sign is the ReLU mask; ignored when relu == 0).
 * y may be NULL with relu != 0 when the forward had NO residual input: the mask is then recomputed from x, gamma, beta and the
 * saved statistics (one tensor read less per pass); beta is only read in that case and may be NULL otherwise.
 * dres (may be NULL) receives the gradient of the residual input = masked dy.
 * accumulate != 0: dgamma / dbeta are added to (the caller's .grad buffers) instead of overwritten. */
int32_t p3d_bn_train_bwd(const float* dy, const float* x, const float* y, const float* gamma, const float* beta,
                         const float* save_mean, const float* save_invstd, float* dx, float* dres,
                         float* dgamma, float* dbeta, int32_t N, int32_t C, int32_t HW, int32_t relu, int32_t accumulate,
                         void* workspace, size_t workspace_bytes, void* stream);
/* eval / frozen statistics (model.eval() depth_train.py:611; freeze_batchnorm depthnet.py:158-161) */
int32_t p3d_bn_eval_fwd(const float* x, const float* res, const float* gamma, const float* beta,
                        const float* running_mean, const float* running_var, float* y,
                        int32_t N, int32_t C, int32_t HW, float eps, int32_t relu, void* stream);
int32_t p3d_bn_eval_bwd(const float* dy, const float* x, const float* y, const float* gamma,
                        const float* running_mean, const float* running_var, float* dx, float* dres,
                        float* dgamma, float* dbeta, int32_t N, int32_t C, int32_t HW, float eps, int32_t relu, int32_t accumulate,
                        void* workspace, size_t workspace_bytes, void* stream);
/* Opt-in, a switch of its own (default OFF; P3D_BN_ANY=1 in the environment turns it on; independent of every other switch): the four entries above run a call
 * that their 16-B instances refuse (HW % 4 != 0, or a tensor off a 16-B line) on PEELED instances: a row -- the HW floats of one (n, c) -- is read as up to three
 * single elements up to its first 16-B line, 16-B accesses, and up to three single elements behind its last full line (by one wavefront for rows of at most 1024
 * elements, by the block for longer ones), so the 129 / 65 / 33 / 17 maps of the default 257 crop stream 16 B per lane instead of one dword.  Taken when every non-NULL tensor of the call is on a 4-B line and all are congruent mod 16 B (one peel
 * serves them all); otherwise, and with the switch off, the entries launch exactly what they launched before.  Same per-element expressions, fp64 sums in an
 * order fixed by the shape and the grid (two runs are bit-equal); the element-wise results (eval forward, dres, eval backward dx) are bit-equal to the
 * element-by-element instance's, the sums of a training layer are added in another order.  p3d_bn_workspace_bytes is unchanged.  With the switch on
 * p3d_stem_tail_fwd / _bwd also take the shapes of p3d_stem_tail_any_supported (below).  Returns the previous setting. */
int32_t p3d_bn_any_enable(int32_t on);
/* What the last call of p3d_bn_train_fwd / _train_bwd / _eval_fwd / _eval_bwd / p3d_stem_tail_fwd / _bwd of the process launched.  Host-side bookkeeping only.
 * out[4]:  [0] the entry: 1 train_fwd, 2 train_bwd, 3 eval_fwd, 4 eval_bwd, 5 stem_tail_fwd, 6 stem_tail_bwd (0: none yet)
 *          [1] the instance: 0 vector (16-B accesses), 1 scalar (element by element), 2 peeled (for the stem tail: the any-sides kernels)
 *          [2] grid.x   [3] grid.y */
void p3d_bn_last_launch(int32_t* out);

/* Training through a frozen BatchNorm folded into its convolution (ops_frozen.py; csrc/p3d_frozen.hip): with s = gamma / sqrtf(var + eps), w' = w * s,
 * b' = beta - mean * s the layer is y = relu?(conv(x, w') + b' (+ res)), and its backward is g = dy * [y > 0] (g = dy without a ReLU), dres = g,
 * dx = dgrad(g, w'), raw = wgrad(x, g), dw = s * raw, dbeta[k] = sum g[k], dgamma[k] = (<w[k], raw[k]> - mean[k] * dbeta[k]) / sqrtf(var[k] + eps).
 * p3d_frozen_grad_mask: dy, y, g are [N][K][HW] fp32.  With y: g = dy where y > 0, else +0.  y == NULL (then g == NULL too): nothing is written, dy is g.
 * Either way sums[k] = sum over n and p of g[n][k][p] (overwritten).  16-B accesses where a channel row's address allows them (all three base pointers on 16-B
 * lines), dwords elsewhere; no element beyond N * K * HW is touched.  The sums are accumulated in fp64 in a fixed order -- per-block partials in the workspace,
 * then one ordered sum per channel -- without atomics: bitwise reproducible.  Workspace: p3d_frozen_grad_mask_workspace_bytes, on an 8-B line.
 * p3d_frozen_wgrad_finish: raw, w, dw are [K][CRS]; dw = s * raw with s the very expression of the fold (p3d_fx_fold_bn_images), dgamma and dbeta as above from
 * sums = p3d_frozen_grad_mask's; the inner product is accumulated in fp64 in a fixed order, one block per output channel.  accumulate != 0: all three are added
 * onto what is there.  dw must not be raw. */
size_t p3d_frozen_grad_mask_workspace_bytes(int32_t N, int32_t K, int32_t HW);
int32_t p3d_frozen_grad_mask(const float* dy, const float* y, float* g, float* sums, int32_t N, int32_t K, int32_t HW, void* workspace, size_t workspace_bytes,
                             void* stream);
int32_t p3d_frozen_wgrad_finish(const float* raw, const float* w, const float* gamma, const float* mean, const float* var, float eps, const float* sums,
                                float* dw, float* dgamma, float* dbeta, int32_t K, int32_t CRS, int32_t accumulate, void* stream);

/* standalone F.relu (skip_relu variants, depthnet.py:197-198) */
int32_t p3d_relu_fwd(const float* x, float* y, int64_t n, void* stream);
int32_t p3d_relu_bwd(const float* dy, const float* y, float* dx, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------
 * nn.MaxPool2d(kernel_size=3, stride=2, padding=1)  depthnet.py:140,192; partial_depthnet.py:219-220
 * x [NC,H,W] -> y [NC,Ho,Wo]; idx (uint8 tap 0..8 of the first maximum, may be NULL) feeds backward.
 * ------------------------------------------------------------------------------------------ */
int32_t p3d_maxpool3x3s2_fwd(const float* x, float* y, uint8_t* idx, int32_t NC, int32_t H, int32_t W, void* stream);
int32_t p3d_maxpool3x3s2_bwd(const float* dy, const uint8_t* idx, float* dx, int32_t NC, int32_t H, int32_t W, void* stream);

/* ------------------------------------------------------------------------------------------
 * The stem's tail in training mode: maxpool(relu(bn1(x)))  (depthnet.py:139-140, resnet.py / fusionnet.py twins) as one node.
 * The BatchNorm output is never written: forward = statistics pass + one pass that applies relu(bn(.)) inside the pooling windows; backward = two passes that
 * route the pooled gradient through the argmax bytes on the fly.  Bit-identical to p3d_bn_train_fwd + p3d_maxpool3x3s2_fwd and their backward calls.
 * x [N,C,H,W] (H, W even, W % 4 == 0) -> y [N,C,H/2,W/2], idx [N,C,H/2,W/2] bytes; save_mean / save_invstd [C] feed backward.
 * workspace: p3d_bn_workspace_bytes(N, C, H * W).
 * p3d_stem_tail_any_supported: N, C > 0, H >= 2, W >= 2, any parity (whatever the switch says).  While p3d_bn_any_enable is on, the two entries take a shape that
 * p3d_stem_tail_supported refuses and this query admits: y and idx are [N,C,Ho,Wo] with Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, idx in the encoding of
 * p3d_maxpool3x3s2_fwd; x, y, dy on 4-B lines, x and dx congruent mod 16 B.  Bit-identical to the three calls under the same switch (tensors congruent mod 16 B).
 * p3d_stem_tail_supported answers the same with the switch on or off.
 * ------------------------------------------------------------------------------------------ */
int32_t p3d_stem_tail_supported(int32_t N, int32_t C, int32_t H, int32_t W);
int32_t p3d_stem_tail_any_supported(int32_t N, int32_t C, int32_t H, int32_t W);
int32_t p3d_stem_tail_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var, float* y, uint8_t* idx,
                          float* save_mean, float* save_invstd, int32_t N, int32_t C, int32_t H, int32_t W, float momentum, float eps, void* workspace,
                          size_t workspace_bytes, void* stream);
int32_t p3d_stem_tail_bwd(const float* dy, const uint8_t* idx, const float* x, const float* gamma, const float* beta, const float* save_mean,
                          const float* save_invstd, float* dx, float* dgamma, float* dbeta, int32_t N, int32_t C, int32_t H, int32_t W, int32_t accumulate,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Volumetric soft-argmax head: utils.to_heatmap + utils.decode  (utils.py:154-194)
 * z [B, D*J, H, W] (channel = d*J + j) -> coords [B, J, 3] = (x, y, z) * depth_range.
 * ------------------------------------------------------------------------------------------ */
int32_t p3d_softargmax3d_fwd(const float* z, float* coords, int32_t B, int32_t D, int32_t J, int32_t H, int32_t W,
                             float depth_range, void* stream);
int32_t p3d_softargmax3d_bwd(const float* dcoords, const float* z, float* dz, int32_t B, int32_t D, int32_t J,
                             int32_t H, int32_t W, float depth_range, void* stream);

/* Loss block of Trainer.vanilla_train (depth_train.py:397-405):
 *   spec = relat - relat[:,key] + true_cam[:,key]
 *   loss = criterion(spec[valid]/loss_div, true_cam[valid]/loss_div), reduction 'mean'
 * criterion: 0 SmoothL1 (beta 1), 1 L1, 2 MSE.  true_val is uint8 [B,J].
 * Outputs: loss[1], spec_cam [B,J,3], drelat [B,J,3] = loss_scale * dloss/drelat.
 * count_override (device pointer to one float, may be NULL): when > 0 it replaces 3*n_valid as the divisor of the mean
 * (global count / world_size under data parallelism, read on the device so no host sync is needed). */
int32_t p3d_pose_loss_fwd_bwd(const float* relat, const float* true_cam, const uint8_t* true_val, float* loss,
                              float* spec_cam, float* drelat, int32_t B, int32_t J, int32_t key_index,
                              float loss_div, int32_t criterion, float loss_scale, const float* count_override, void* stream);

/* criterion(pred[valid], target[valid]), mean over the selected rows x C (the image-space and reconstruction losses of train.py:94,112):
 * pred/target [rows][C], valid [rows] bytes -> loss[1], dpred = d loss / d pred.  count_override as in p3d_pose_loss_fwd_bwd. */
int32_t p3d_masked_loss_fwd_bwd(const float* pred, const float* target, const uint8_t* valid, float* loss, float* dpred, int32_t rows, int32_t C,
                                int32_t criterion, const float* count_override, void* stream);

/* Evaluation statistics of one test batch (Trainer.test with P3D_DEVICE_EVAL=1: the back-rotation + utils.analyze), one launch:
 *   spec = rotate[b] @ spec_cam[b,j], truth = rotate[b] @ true_cam[b,j]            rotate [B,3,3] (np.einsum('Bij,BCj->BCi'))
 *   dist = |spec - truth|, flip = |spec - truth[b,mirror[j]]|, tangent = |(spec - truth).xy|      mirror int32 [J]
 * in numpy's float32 operations and order (no FMA contraction), then over the valid joints (true_val uint8 [B,J]) one fp64 row of
 * P3D_EVAL_ROW values at `row`: the columns below.  PCK counts dist / rough <= 1, AUC sums max(0, 1 - dist / rough) (float32 division);
 * the six classes are utils.statistics' cascade solid -> close -> depth (tangent <= close) -> jitter (<= rough) -> switch (flip <= rough)
 * -> fail.  `loss` is the device scalar p3d_pose_loss_fwd_bwd wrote.  spec_rot_out [B,J,3] (may be NULL) receives the rotated spec.
 * One block, fixed-order reduction, no atomics: the same inputs give the same row bits. */
#define P3D_EVAL_VALID 0
#define P3D_EVAL_SUM_DIST 1
#define P3D_EVAL_PCK 2
#define P3D_EVAL_SUM_AUC 3
#define P3D_EVAL_SOLID 4                 /* 4..9: solid, close, depth, jitter, switch, fail counts */
#define P3D_EVAL_LOSS 10
#define P3D_EVAL_BATCH 11
#define P3D_EVAL_PRESENT 12              /* 1.0 in every written row (0 in the padding of a sharded table) */
#define P3D_EVAL_ROW 13
int32_t p3d_pose_eval_stats(const float* spec_cam, const float* true_cam, const float* rotate, const uint8_t* true_val, const int32_t* mirror,
                            int32_t B, int32_t J, float solid, float close, float rough, const float* loss, double* row, float* spec_rot_out,
                            void* stream);

/* utils.get_recon_cam (utils.py:335-366): differentiable least-squares placement of the root-relative pose relat_cam [B,J,3] such that it projects
 * onto spec_mat [B,J,2] under intrinsics [B,3,3]: recon = relat_cam + (A^T A)^-1 A^T b.  bwd: gradients w.r.t. spec_mat and relat_cam. */
int32_t p3d_recon_cam_fwd(const float* spec_mat, const float* relat_cam, const float* intrinsics, float* recon, int32_t B, int32_t J, void* stream);
int32_t p3d_recon_cam_bwd(const float* drecon, const float* spec_mat, const float* relat_cam, const float* intrinsics, float* dspec_mat, float* drelat_cam,
                          int32_t B, int32_t J, void* stream);

/* ------------------------------------------------------------------------------------------
 * nn.utils.clip_grad_norm_ + optim.Adam(weight_decay) on flat buffers (depth_train.py:455-456, :83)
 * ------------------------------------------------------------------------------------------ */
/* accum[0] (double) += sum(g[i]^2).  Caller zeroes accum before the first call of a step. */
int32_t p3d_l2norm_sq_accum(const float* g, int64_t n, double* accum, void* stream);
/* coef = min(max_norm / (sqrt(*norm_sq) * norm_scale + 1e-6), 1) * norm_scale is applied to g on the fly
 * (norm_sq NULL or max_norm <= 0: coef = grad_scale only); then torch.optim.Adam's update with coupled L2
 * weight decay.  step is the 1-based step count.  grad_scale multiplies g before anything else (1/world_size). */
int32_t p3d_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                      float eps, float weight_decay, int32_t step, float max_norm, const double* norm_sq,
                      float grad_scale, void* stream);

/* The same update with the step counter and the -half_acc overflow rule (depth_train.py:431-446) resident on the device:
 * state[0] = optimizer steps taken (incremented by this call unless it skips), state[1] = steps skipped; with skip_nonfinite != 0
 * a non-finite *norm_sq leaves weights, moments and state[0] untouched and increments state[1].  No host read-back anywhere.
 * scratch16: 16 bytes of device memory for the constants handed from the one-thread prepare kernel to the update kernel. */
int32_t p3d_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                          float eps, float weight_decay, int32_t* state, float max_norm, const double* norm_sq,
                          float grad_scale, int32_t skip_nonfinite, void* scratch16, void* stream);

/* ------------------------------------------------------------------------------------------
 * Feature distillation loss, teacher -> student: Trainer.distill (depth_train.py:115-129).
 * teach, student [B,C,H,W]; atten [B,1,H,W].  mode 0: mean_b ||(t-s)*a||_2;  1: the same on sigmoid(t)-sigmoid(s) (-sigmoid);
 * 2 (-bin_dist): mean(BCEWithLogits(s, sigmoid(t))) * mean_b(sum a_b), as the reference computes it.
 * Outputs loss[1] and, if dstudent != NULL, loss_scale * dloss/dstudent.
 * ------------------------------------------------------------------------------------------ */
size_t p3d_distill_workspace_bytes(int32_t B);
int32_t p3d_distill_fwd_bwd(const float* teach, const float* student, const float* atten, float* loss, float* dstudent,
                            int32_t B, int32_t C, int32_t HW, int32_t mode, float loss_scale,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * On-GPU augmentation (config 5): augment_colour.random_color (augment_colour.py:48-67) and
 * augment_occluder.random_erase (augment_occluder.py:84-105) on float images [B,3,H,W] in [0,1].
 * params [B,4]: brightness delta, contrast factor, hue shift (deg), saturation factor.
 * rects  [B,4] int32: x0, y0, x1, y1 (exclusive); colour [B,3].
 * ------------------------------------------------------------------------------------------ */
int32_t p3d_augment_colour(float* img, const float* params, int32_t B, int32_t H, int32_t W, void* stream);
int32_t p3d_augment_erase(float* img, const int32_t* rects, const float* colour, int32_t B, int32_t C,
                          int32_t H, int32_t W, void* stream);
/* augment_occluder.paste_over (augment_occluder.py:7-55): alpha-blend one pre-resized occluder per image into img [B,C,H,W] (0..255 values), in place.
 * bank: the occluders' pixels, interleaved [pixel][C] fp32; alpha: one fp32 per bank pixel, or NULL (opaque); plan [B][8] int32 (device) =
 * {dst_y0, dst_x0, src_y0, src_x0, h, w, occluder row length, bank offset in pixels} (the clipped rectangles of :31-50, computed on the host);
 * max_pixels = the largest h*w of the batch; truncate != 0 reproduces the assignment into a uint8 image. */
int32_t p3d_augment_occlude(float* img, const float* bank, const float* alpha, const int32_t* plan, int32_t B, int32_t C, int32_t H, int32_t W,
                            int32_t max_pixels, int32_t truncate, void* stream);
/* Crop re-projection of the loader (depth_datasets.py:153-193 -> cameralib.reproject_image_fast, cameralib.py:667-711) for a batch:
 * dst[b][c][y][x] = bilinear sample of src[b] ([Hs][Ws][C] interleaved, uint8 if src_is_u8 else fp32) at homography[b] * (x, y, 1),
 * constant border 0; uint8 sources are rounded like cv2's uint8 output.  homography: [B][3][3] fp32 (device), new image -> old image. */
int32_t p3d_warp_crops(const void* src, int32_t src_is_u8, const float* homography, float* dst, int32_t B, int32_t Hs, int32_t Ws, int32_t C,
                       int32_t Ho, int32_t Wo, void* stream);
/* cameralib.reproject_image general case (cameralib.py:378-443): like p3d_warp_crops but through the OLD camera's lens model.  params20 = B x
 * { ray[9] (crop pixel -> old-camera direction; the full homography when undistorted), k[6] (rows 0,1 of the old intrinsics; identity rows
 * with a homography), dist[5] (k1 k2 p1 p2 k3, cameralib.project_points :636-659; zeros = none) } on the device.  round_u8: round uint8 sources like cv2. */
int32_t p3d_reproject_crops(const void* src, int32_t src_is_u8, const float* params20, float* dst, int32_t B, int32_t Hs, int32_t Ws, int32_t C,
                            int32_t Ho, int32_t Wo, int32_t round_u8, void* stream);
/* depth_datasets.enhance_ntu / enhance_pku (depth_datasets.py:39-56) in place on PNG-unit depth crops (0..1): v = x / (10/255);
 * nexponent ? exp(-v) * (v >= threshold) : v / 3.  factor (nullable, same shape): utils.to_depth's divisor map (utils.py:68-75), applied first. */
int32_t p3d_enhance_depth(float* x, const float* factor, int64_t n, float threshold, int32_t nexponent, void* stream);
/* transforms.ToTensor() + Normalize(mean, std) of the loader (depth_datasets.py:78-79,91-93), in place on [B,3,H,W] holding 0..255:
 * x = (x / 255 - mean[c]) / std[c]; mean3 / std3 are HOST pointers to 3 floats */
int32_t p3d_normalize_rgb(float* img, int32_t B, int32_t HW, const float* mean3, const float* std3, void* stream);

/* ------------------------------------------------------------------------------------------
 * fp16 path of -half_acc (depth_train.py:73-83,413-449: model.half(), fp32 master copies, static loss scale).
 * Activations are NHWC fp16 (`void*` = device pointer to IEEE half), channel counts multiples of 8; accumulation is fp32.
 * Weights come as fp16 images of the fp32 master [K][C][R][S]: [K][R][S][Cpad] (forward, wgrad columns) and
 * [Cpad][R][S][K] (dgrad), produced by p3d_weight_images_f16 after every optimizer step.
 * The descriptor is the fp32 one; d->C is the (padded) channel count of x.  Replaces the cuDNN half kernels behind
 * nn.Conv2d after model.half() (depthnet.py:16-33,65-89).
 * ------------------------------------------------------------------------------------------ */
/* Partial conv (partial_conv.py:32-57): mask_in [N][H][W] fp32 {0,1} drops masked input pixels in the operand fetch, mult [N][Ho][Wo]
 * scales the result; both may be NULL.  Backward: the caller scales dy by mult once (p3d_hscale_pixels) and passes that tensor to
 * dgrad (mask_in then multiplies dx) and wgrad (mask_in masks x).
 * d->accumulate, fp16 forward: must be 0 (p3d_hconv2d_fwd, p3d_hconv2d_fwd_stats and p3d_hconv2d_fwd_infer refuse anything else). */
int32_t p3d_hconv2d_fwd(const p3d_conv_desc* d, const void* x_nhwc, const void* w_krsc, const float* bias, const float* mask_in,
                        const float* mult, void* y_nhwc, void* stream);
int32_t p3d_hscale_pixels(const void* src_nhwc, const float* scale, void* dst_nhwc, int64_t P, int32_t C, void* stream);
/* Inference with an eval-mode BatchNorm folded into the weight image (infer.fold_half; w_krsc from p3d_fx_fold_bn_images kind 2, bias = b'):
 * y = fp16(relu?(conv(x * mask_in) * mult + bias + res)), rounded once.  res is NHWC fp16 shaped like y, or NULL; bias, mask_in and mult may be NULL.
 * The result leaves through LDS as 16-B stores, the residual is read in 16-B runs.  d->accumulate must be 0.
 * supported: 1 when the descriptor runs on this entry point (else 0, the reason in p3d_last_error()). */
int32_t p3d_hconv2d_fwd_infer_supported(const p3d_conv_desc* d);
int32_t p3d_hconv2d_fwd_infer(const p3d_conv_desc* d, const void* x_nhwc, const void* w_krsc, const float* bias, const float* mask_in, const float* mult,
                              const void* res_nhwc, int32_t relu, void* y_nhwc, void* stream);
/* Block-scaled FP8 (MXFP8) inference convolution (infer.fold_fp8): y = fp16(relu?(conv(q(x * mask_in), w_mx) * mult + bias + res)), rounded once, on
 * v_mfma_scale_f32_32x32x64_f8f6f4.  w_mx is a kind-3 fold image (p3d_fx_fold_bn_images) of d->C input channels; x is NHWC fp16 with d->C channels, quantized
 * on the fly by the same MX rule per (pixel, tap, 32 channels), so the result equals quantizing x once and convolving the dequantized operands with fp32
 * accumulation.  res, bias, mask_in, mult as for p3d_hconv2d_fwd_infer.
 * supported: 1 when the descriptor runs on this entry point, else 0 and the reason in p3d_last_error() (C not a multiple of 32, K not a multiple of 8,
 * accumulate, a channel window, a tensor beyond the 2 GiB buffer window).  weight_bytes: the size of a kind-3 image (0 when C % 32 != 0). */
int32_t p3d_f8conv2d_fwd_infer_supported(const p3d_conv_desc* d);
size_t p3d_f8conv2d_weight_bytes(int32_t K, int32_t C, int32_t RS);
int32_t p3d_f8conv2d_fwd_infer(const p3d_conv_desc* d, const void* x_nhwc, const void* w_mx, const float* bias, const float* mask_in, const float* mult,
                               const void* res_nhwc, int32_t relu, void* y_nhwc, void* stream);
/* The MXFP8 activation tensor (infer.fold_fp8(model, resident=True)): what one fp8 convolution writes and the next reads, so that an activation is quantized
 * once, by its producer, and not by every tap and row tile of its consumer.  For an NHWC activation [N][H][W][C] with C % 32 == 0, ONE allocation of
 * p3d_f8act_bytes(N * H * W, C) bytes holds
 *   e4m3fn elements  [N * H * W][C]        at byte 0, then
 *   E8M0 scale bytes [N * H * W][C / 32]   at byte N * H * W * C (the scales follow the elements, as in the kind-3 weight image).
 * A block is 32 consecutive channels of one pixel.  The rule is the one p3d_f8conv2d_fwd_infer applies to its fp16 input: e = floor(log2(amax)), scale byte
 * e - 8 + 127, element = e4m3fn(RNE(clamp(v / 2^(e - 8), -448, 448))); an all-zero block has scale byte 0 (and elements +-0).  So the block a producer writes
 * is bit for bit the block the consumer would have made from the stored fp16 value.
 * p3d_f8act_bytes: pixels * C + pixels * C / 32; 0 for C % 32 != 0 or a non-positive argument.
 * p3d_f8conv2d_fwd_infer_mx is p3d_f8conv2d_fwd_infer with either form on either side.  Exactly one of x_nhwc (fp16) / x_mx must be given, and at least one
 * of y_nhwc (fp16) / y_mx; both results hold the same values, y_mx the quantized fp16 result.  mask_in with x_mx zeroes the masked pixels' blocks (elements
 * and scale byte), which equals quantizing x * mask_in.  With fp16 on both sides it runs the kernel instance of p3d_f8conv2d_fwd_infer.
 * supported (host only): p3d_f8conv2d_fwd_infer_supported, and K % 32 == 0 when y_mx is set, and the MX tensors inside the 2 GiB buffer window. */
size_t p3d_f8act_bytes(int64_t pixels, int32_t C);
int32_t p3d_f8conv2d_fwd_infer_mx_supported(const p3d_conv_desc* d, int32_t x_is_mx, int32_t y_mx);
int32_t p3d_f8conv2d_fwd_infer_mx(const p3d_conv_desc* d, const void* x_nhwc, const void* x_mx, const void* w_mx, const float* bias, const float* mask_in,
                                  const float* mult, const void* res_nhwc, int32_t relu, void* y_nhwc, void* y_mx, void* stream);
/* d->accumulate != 0: dx += result (joins the gradient another consumer of the same input already wrote) */
int32_t p3d_hconv2d_dgrad(const p3d_conv_desc* d, const void* dy_nhwc, const void* w_crsk, const float* mask_in, void* dx_nhwc, void* stream);
/* A convolution whose epilogue also leaves the channel sums of the BatchNorm next to it (round 4; what the fp32 path's EPI 1 / 2 do), so that the BatchNorm costs no
 * pass over the tensor for its sums (reference: the nn.BatchNorm2d behind / in front of every conv of a residual block, depthnet.py:42-56,98-116).
 *   p3d_hconv2d_sum_rows(d, pass)  rows of the table: pixel tiles of the forward output (pass 0) / of the data gradient's result (pass 1, stride 1)
 *   p3d_hconv2d_fwd_stats          y = conv(x) + partial [rows][K/8][16] fp32: per (pixel tile, 8-channel group) sum y (0..7) and sum y^2 (8..15) of the ROUNDED fp16 results
 *   p3d_hconv2d_dgrad_sums         dx = dgrad(dy) (stride 1, no accumulate) + partial [rows][C/8][16]: sum g, sum g * xhat of the BatchNorm + ReLU layer whose output x is,
 *                                  g = dx masked by that layer's ReLU (recomputed from its raw output c_prev and forward constants coef_prev, as p3d_hbn_train_bwd does)
 * p3d_hbn_train_fwd_partial / p3d_hbn_train_bwd_partial finalize such a table and run the apply pass. */
int32_t p3d_hconv2d_sum_rows(const p3d_conv_desc* d, int32_t pass);
int32_t p3d_hconv2d_fwd_stats(const p3d_conv_desc* d, const void* x_nhwc, const void* w_krsc, void* y_nhwc, float* partial, void* stream);
int32_t p3d_hconv2d_dgrad_sums(const p3d_conv_desc* d, const void* dy_nhwc, const void* w_crsk, void* dx_nhwc, const void* c_prev, const float* coef_prev, float* partial,
                               void* stream);
size_t p3d_hconv2d_wgrad_workspace_bytes(const p3d_conv_desc* d);
/* dw (fp32 master gradient [K][c_real][R][S]) = (d->accumulate ? dw : 0) + scale * wgrad; c_real <= d->C (stem: 3 of 8) */
int32_t p3d_hconv2d_wgrad(const p3d_conv_desc* d, const void* dy_nhwc, const void* x_nhwc, const float* mask_in, float* dw, int32_t c_real, float scale,
                          void* workspace, size_t workspace_bytes, void* stream);
/* db[K] (fp32) = (accumulate ? db : 0) + scale * sum over the P pixels of dy[P][K] */
int32_t p3d_hconv2d_bgrad(const void* dy_nhwc, int32_t P, int32_t K, float* db, float scale, int32_t accumulate, void* stream);
/* Training through a frozen BatchNorm folded into its fp16 convolution (ops_frozen.HFrozenConvBnFn; csrc/p3d_hfrozen.hip): the mask-and-sum pass of
 * p3d_frozen_grad_mask on NHWC fp16.  dy, y, g are [P][K] halves.  With y: g = dy where y > 0, else +0.  y == NULL (then g == NULL too): nothing is written, dy is
 * g.  Either way sums[k] (fp32, overwritten) = sum over the P pixels of g[p][k].  One pass of 16-B accesses (8 channels of one pixel per lane); no element beyond
 * P * K is touched.  The sums never pass through fp16 (gradients carry the loss scale): every half is widened to fp64 and accumulated there in a fixed order --
 * per-thread accumulators, the block's pixel rows through LDS, per-block partials in the workspace, one ordered sum per channel -- without atomics: bitwise
 * reproducible.  Shape rule: K % 8 == 0, 8 <= K <= 2048, 0 < P < 2^31, dy / y / g on 16-B lines; P3D_EINVAL with a message outside it, nothing launched.
 * Workspace: p3d_hfrozen_grad_mask_workspace_bytes (0 outside the rule), on an 8-B line. */
size_t p3d_hfrozen_grad_mask_workspace_bytes(int64_t P, int32_t K);
int32_t p3d_hfrozen_grad_mask(const void* dy_nhwc, const void* y_nhwc, void* g_nhwc, float* sums, int64_t P, int32_t K, void* workspace, size_t workspace_bytes,
                              void* stream);
/* layout / precision converters: dst = scale * src; Cpad >= C, multiple of 8, the padding channels are written as 0 */
int32_t p3d_nchw_f32_to_nhwc_f16(const float* src, void* dst, int32_t N, int32_t C, int32_t HW, int32_t Cpad, float scale, void* stream);
int32_t p3d_nhwc_f16_to_nchw_f32(const void* src, float* dst, int32_t N, int32_t C, int32_t HW, float scale, void* stream);
int32_t p3d_weight_images_f16(const float* w, void* krsc, void* crsk /* may be NULL */, int32_t K, int32_t C, int32_t RS, int32_t Cpad,
                              void* stream);
/* every convolution of a network in one launch: the masters live in one flat fp32 buffer (FlatAdam), the images in one fp16 buffer;
 * table (device memory) has njobs rows {int64 w_off, krsc_off, crsk_off (-1: none); int32 K, C, RS, Cpad}, offsets in elements */
int32_t p3d_weight_images_f16_batched(const float* flat, void* images, const void* table, int32_t njobs, void* stream);

/* BatchNorm2d (+ residual + ReLU) on NHWC fp16: x, res, y, dy, dx, dres are [P = N*H*W][C] fp16; gamma, beta, running statistics
 * and dgamma / dbeta stay fp32 (they are the master parameters).  C/8 must divide 256 or be a multiple of it.
 * Training forward writes coef [C][4] fp32 = {gamma*invstd, beta - mean*gamma*invstd, mean, invstd}: the caller keeps it for backward
 * (it replaces save_mean / save_invstd of the fp32 entry points).  Backward: y may be NULL when relu != 0 and the layer had no
 * residual (the mask is recomputed from x and coef). */
size_t p3d_hbn_workspace_bytes(int32_t C);
int32_t p3d_hbn_train_fwd(const void* x, const void* res, const float* gamma, const float* beta, float* running_mean,
                          float* running_var, void* y, float* coef, int32_t P, int32_t C,
                          float momentum, float eps, int32_t relu, void* workspace, size_t workspace_bytes, void* stream);
int32_t p3d_hbn_eval_fwd(const void* x, const void* res, const float* gamma, const float* beta, const float* running_mean,
                         const float* running_var, void* y, int32_t P, int32_t C, float eps, int32_t relu,
                         void* workspace, size_t workspace_bytes, void* stream);
int32_t p3d_hbn_train_bwd(const void* dy, const void* x, const void* y, const float* coef, void* dx, void* dres, float* dgamma, float* dbeta,
                          int32_t P, int32_t C, int32_t relu, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* the same with the sums already taken by a convolution's epilogue (partial [rows][C/8][16]); bwd: a BatchNorm + ReLU layer without residual, coef2 = C float4 of scratch */
int32_t p3d_hbn_train_fwd_partial(const void* x, const void* res, const float* gamma, const float* beta, float* running_mean, float* running_var,
                                  void* y, float* coef, int32_t P, int32_t C, float momentum, float eps, int32_t relu, const float* partial, int32_t rows,
                                  uint8_t* relu_mask /* or NULL: P * C / 8 bytes, bit e of byte [pixel][8-channel group] = [y > 0] */, void* stream);
/* p3d_hbn_train_bwd of a BatchNorm + residual + ReLU layer (the closing one of a block, depthnet.py:52-56) reading those mask bytes in place of y */
int32_t p3d_hbn_train_bwd_mask(const void* dy, const void* x, const uint8_t* relu_mask, const float* coef, void* dx, void* dres, float* dgamma, float* dbeta,
                               int32_t P, int32_t C, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream);
int32_t p3d_hbn_train_bwd_partial(const void* dy, const void* x, const float* coef, void* dx, float* dgamma, float* dbeta, int32_t P, int32_t C, int32_t accumulate,
                                  const float* partial, int32_t rows, float* coef2, void* stream);
/* BatchNorm with FROZEN statistics inside a training step (freeze_batchnorm, depthnet.py:158-161, under -do_freeze): the forward is
 * p3d_hbn_eval_fwd; p3d_hbn_eval_coef writes the {scale, shift, mean, invstd} table of the running statistics for the backward, which is
 * dx = scale * g (no batch-statistics terms), dgamma = sum g * xhat, dbeta = sum g with g the ReLU-masked incoming gradient. */
int32_t p3d_hbn_eval_coef(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float* coef, int32_t C, float eps,
                          void* stream);
int32_t p3d_hbn_frozen_bwd(const void* dy, const void* x, const void* y, const float* coef, void* dx, void* dres, float* dgamma, float* dbeta,
                           int32_t P, int32_t C, int32_t relu, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* torch.cat((x, y), dim=1) of the Fusion block (fusionnet.py:138) on NHWC fp16: split == 0 writes cat[P][Ca+Cb] from a[P][Ca], b[P][Cb];
 * split != 0 writes a and b from cat (the backward of the concat) */
int32_t p3d_hconcat(void* a, void* b, void* cat, int64_t P, int32_t Ca, int32_t Cb, int32_t split, void* stream);
/* standalone F.relu on fp16 (-skip_relu, depthnet.py:197-198): dy == NULL -> out = relu(x); else out = dy masked by x > 0 */
int32_t p3d_hrelu(const void* x, const void* dy, void* out, int64_t n, void* stream);
/* nn.MaxPool2d(3, 2, 1) on NHWC fp16; idx [N][Ho][Wo][C] uint8 window codes as in p3d_maxpool3x3s2_fwd, or NULL (inference: no window codes written) */
int32_t p3d_hmaxpool3x3s2_fwd(const void* x, void* y, uint8_t* idx, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);
int32_t p3d_hmaxpool3x3s2_bwd(const void* dy, const uint8_t* idx, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);

#ifdef __cplusplus
}
#endif
#endif
