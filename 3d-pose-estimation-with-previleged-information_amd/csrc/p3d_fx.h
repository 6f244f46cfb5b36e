// Internal interface of p3d_fx.hip (exact-fp32 convolutions on the bf16 matrix pipe, with BatchNorm prologues / epilogues) to the C-ABI
// entry points in p3d_conv.hip and the residual-block executor in p3d_block.hip.  Not part of the public ABI (include/p3d_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/p3d_hip.h"

namespace p3d {

// one stride^2 parity class of a strided data gradient: the fields of FxConvParams that differ between the classes of one launch (blockIdx.z selects)
struct FxConvClass { int nR, nS, ntap, r0, rstep, s0, sstep, hoff, hstep, woff, wstep, oy0, ox0; };

struct FxConvParams {
    const float* X;         // AMODE 0: activation operand, x (FWD) or dy (DGRAD), fp32 [N][Cred][Hi][Wi]
    const unsigned char* Ximg;      // AMODE 1: the same tensor as a pre-split activation image (fx_act_image): three bf16 planes [N][Cred/16][Hi][Wi][16]
    size_t plane_bytes;     // AMODE 1: bytes between two planes of Ximg
    const unsigned char* Wimg;      // pre-split weight image (fx_build_weight_images)
    float* Y;               // result [N][M][YH][YW], or the split-K slabs
    const float* bias;      // [M] or null
    const float* ep_c;      // EPI 2: raw conv output laid out like the result
    const float* ep_tab;    // EPI 2: {sc, sh, mean} per result channel
    float* partial;         // EPI 1 / 2: [rows][M][2] partial sums
    const float* pmask;     // PRO 4 (partial convolution): per-pixel factor of the activation operand, [N][1][Hi][Wi]
    const float* emask;     // EPI 4: per-pixel factor of the result, [N][1][YH][YW]
    const float* acc_src;   // dense unsplit launches with `accumulate`: what is added to the result instead of Y's own content (laid out like Y), after
    const unsigned char* acc_mask;   //   masking by these bytes when given (bit e of byte i: element 4 i + e passes): Y = result + src * mask, Y itself is only written
    const float* ep_res;    // EPIX 8 (inference: conv + folded BatchNorm): residual added after bias and accumulation, laid out like Y, or null
    int ep_relu;            // EPIX 8: ReLU last
    size_t slab_stride;     // elements between two split-K slabs
    int N, Cred, Hi, Wi;
    int M, OH, OW, NP;      // the GEMM's pixel grid (for strided dgrad: one parity class of the input) and its size N * OH * OW
    int YH, YW, oy0, ox0, oys, oxs;     // pixel (oh, ow) of the grid is result pixel (oy0 + oh * oys, ox0 + ow * oxs)
    int R, S;               // filter size (tap index of the weight image = r * S + s)
    int nR, nS, ntap;       // taps this launch visits: r = r0 + rstep * ir (ir < nR), s likewise
    int r0, rstep, s0, sstep;
    int hmul, hoff, hstep;  // activation row of (oh, tap ir) = oh * hmul + hoff + ir * hstep
    int wmul, woff, wstep;
    int kchunk;             // K steps per split (0: no split-K; otherwise blockIdx.y selects the slab)
    int accumulate;
    int tiles_m;
    int tap_inner;          // K-step order of a multi-tap launch: 0 tap outer (all channel steps of a tap, then the next tap), 1 tap inner (the taps of a 16-channel
                            // step back to back: the shifted windows of one channel group are the same cache lines, which a wide layer otherwise re-fetches per tap)
    int ncls;               // > 0: a strided data gradient whose parity classes run as ONE launch, class blockIdx.z overriding the fields above from cls[]
    FxConvClass cls[4];
};

struct FxWgradParams {
    const float* amask;     // MASKED: per-output-pixel factor of dy, [N][1][OH][OW]
    const float* bmask;     // MASKED: per-input-pixel factor of x, [N][1][Hi][Wi]
    const float* DY;        // fp32 [N][K][OH][OW], or
    const unsigned char* DYimg;     //   its pre-split image [3][N][K/16][OH][OW][16] (AIMG)
    const float* X;         // fp32 [N][C][Hi][Wi], or
    const unsigned char* Ximg;      //   its pre-split image [3][N][C/16][Hi][Wi][16] (BIMG)
    size_t dy_plane, x_plane;       // bytes between two planes of the images
    float* slabs;           // [split][K][taps][C]
    int N, K, C, Hi, Wi, OH, OW, R, S, stride, pad, dil;
    int nsplit, spb;        // K steps (16 pixels each) per split
    int order;              // logical block order: 0 (input-channel tile, output-channel tile, tap, slab), 1 (tap, output-channel tile, input-channel tile, slab)
};

// what a launch adds to the plain convolution; null pointers = not used
// a "table" is one BatchNorm layer's [C][8] floats {sc, sh, mean, invstd, A, B, K, 0} (p3d_block.hip)
struct FxFuse {
    const void* act_img;    // FWD: pre-split image of x;  DGRAD: pre-split image of dy (fx_act_image).  The fp32 pointer of that operand is ignored then.
    const void* dy_img;     // WGRAD: pre-split image of dy
    const void* x_img;      // WGRAD: pre-split image of x
    float* partial;         // FWD: partial sums of y, y^2;  DGRAD: partial sums of g, g * (ep_c - mean)
    const float* ep_c;      // DGRAD epilogue: raw conv output laid out like dx
    const float* ep_tab;    // DGRAD epilogue: table of the BN ep_c went through
    const float* pmask;     // partial convolution (partial_conv.py:32-57): factor of the activation operand per pixel (FWD: mask_in, DGRAD: mult; WGRAD: mult for dy)
    const float* emask;     //   and of the result per pixel (FWD: mult, DGRAD: mask_in; WGRAD: mask_in for x).  Both or neither.
    const void* wimg;       // FWD / DGRAD: pre-split weight image of this conv for this direction (fx_build_weight_images), or null: built into the workspace by the call
    const float* acc_src;   // DGRAD with d->accumulate, stride 1, unsplit (fx_dgrad_accumulates_from_source): dx = dgrad + acc_src * [acc_mask bit] instead of dx += dgrad
    const unsigned char* acc_mask;
    // FWD, inference (a conv with its eval-mode BatchNorm folded into the weight image and the bias): y = conv + bias (+ y when accumulating) (+ res) (then ReLU), on
    // the split-K path applied by the reduce pass after the slabs are summed
    int infer;              // 0 / 1
    const float* res;
    int relu;
    int rows;               // 1: act_img / dy_img / x_img are fp32 ROW images (fx_row_image: [N][C/16][HW][16] floats, 4 B per element) that the kernel cuts into the three
                            // pieces itself -- dense aligned training launches only (no factor, not ragged, not inference): what the block executor keeps a_i and d c_i as
    int ragged;             // 1: the ragged instances (any map width), for inference and training alike; fp32 operands, or (dense training launches only, nothing else set
                            // but `partial` with its ep_c / ep_tab -- the ragged residual blocks: one unsplit launch; p3d_fx_conv_*_img_any) act_img for FWD (either stride, with `partial` too) / DGRAD (stride 1; a stride-2 one is the class launches of fx_conv_dgrad_strided_any with dy_img) and dy_img AND x_img for WGRAD (fx_wgrad_any_img_kernel, either stride).  With `infer`: dense, or a partial convolution
                            // with pmask and emask.  Without: FWD / DGRAD (stride 1) with the plain epilogue, WGRAD on fx_wgrad_any_kernel -- dense fp32-fed training
                            // launches (p3d_x3_any_enable), no other field set; or the same three as a partial convolution (p3d_x3_any_partial_enable): pmask AND
                            // emask set, nothing else -- the factor epilogue, fx_wgrad_any_masked_kernel
};
constexpr int FX_TAB = 8;   // floats per channel of a table

// The epilogue of a forward / data-gradient launch: EPIX of fx_conv_kernel<AMODE, PRO, EPIX, TAPI, RAG> and EPI of fx16_conv_kernel<BM, EPI, TAPI> (plain ints: the values
// are part of the kernels' mangled names, which the profiles and tools/ quote).  Every code stores the result (+ bias); the three functions below take a code apart.
// Under split-K the slabs come from the FX_EPI_STORE instance and the rest of the epilogue is done by the pass that sums them (fx_reduce_kernel).
enum : int {
    FX_EPI_STORE = 0,
    FX_EPI_STATS = 1,               // sums 1: per-(pixel tile, channel) partial sums of y, y^2 (the BatchNorm behind the conv)
    FX_EPI_BWD_SUMS = 2,            // sums 2: of g, g * (c2 - mean), g = y * [c2 * sc + sh > 0] (the BatchNorm + ReLU in front of the conv whose input gradient this is; ep_c = c2, ep_tab its table)
                                    // (3 is unused: it was the tail-sums epilogue, measured slower and removed; profiles/r04_summary.md §3.  The other codes keep their values)
    FX_EPI_FACTOR = 4,              // factor: the result times emask[pixel], in the register view; the per-layer partial convolution (fp32-fed, PRO 4)
    FX_EPI_FACTOR_STATS = 5, FX_EPI_FACTOR_BWD_SUMS = 6, FX_EPI_FACTOR_IMG = 7,     // factor with sums 1 / sums 2 / image-fed: partial convolutions inside the residual-block
                                    // executor, the sums taken of the renormalised result.  (fx16_conv_kernel reads the factor pointer at run time: fx16_epi)
    FX_EPI_INFER = 8,               // inference tail: (+ ep_res) (ReLU), the bias being the shift b' of a folded BatchNorm
    FX_EPI_INFER_FACTOR = 9,        // the same of a partial convolution: acc * emask[pixel] + b' (+ ep_res) (ReLU), the factor BEFORE the folded shift and in the staged store (an
                                    // empty window, emask = 0, gives relu(b' + res): the reference's partial conv writes 0 there and the BatchNorm behind it maps 0 to b')
};
constexpr int fx_epi_sums(int epi) { return epi == FX_EPI_STATS || epi == FX_EPI_FACTOR_STATS ? 1 : epi == FX_EPI_BWD_SUMS || epi == FX_EPI_FACTOR_BWD_SUMS ? 2 : 0; }
constexpr bool fx_epi_factor(int epi) { return epi >= FX_EPI_FACTOR && epi <= FX_EPI_FACTOR_IMG; }
constexpr bool fx_epi_infer(int epi) { return epi == FX_EPI_INFER || epi == FX_EPI_INFER_FACTOR; }

// HIP-event bracket around one conv launch (p3d_block.hip keeps the records; no-op unless p3d_profile_enable(1))
struct ProfScope {
    hipEvent_t a = nullptr, b = nullptr, m = nullptr;        // m: where the conv kernel itself ended, when slab / split-K sums follow inside the bracket
    hipStream_t st;
    int kind;
    double flops;
    ProfScope(int kind, const p3d_conv_desc* d, hipStream_t st);
    ~ProfScope();
};
// called by the launchers between a conv kernel and the pass that sums its slabs: the open bracket of this host thread notes the position (once)
void prof_kernel_done(hipStream_t st);

bool fx_enabled();
void fx_tune(int what, int value);
int fx_set_enabled(int on);
bool fx_any_enabled();                  // p3d_x3_any_enable / P3D_X3_ANY=1 (default off): the per-layer training entries use the ragged instances where the aligned predicates refuse
int fx_set_any_enabled(int on);
bool fx_any_partial_enabled();          // p3d_x3_any_partial_enable / P3D_X3_ANY_PARTIAL=1 (default off): the same for partial convolutions (both factors), independent of the dense switch
int fx_set_any_partial_enabled(int on);
bool fx_any_images_enabled();           // p3d_x3_any_images_enable / P3D_X3_ANY_IMAGES=1 (default off): image-feeding callers (ops_block.ConvImagesFn) use the ragged image-fed entries where the aligned query refuses; kept for them, read by no entry point
int fx_set_any_images_enabled(int on);
bool fx_any_strided_enabled();          // p3d_x3_any_strided_enable / P3D_X3_ANY_STRIDED=1 (default off): p3d_conv2d_dgrad runs dense stride-2 data gradients the aligned predicate refuses as ragged class launches
int fx_set_any_strided_enabled(int on);
void fx_count(int kind, const p3d_conv_desc* d);
void fx_stats(unsigned long long* counts, double* flops, int reset);
// the log of forward / data-gradient conv-kernel launches and the list of compiled instances (p3d_fx_launch_log, p3d_fx_conv_instances: include/p3d_hip.h)
int32_t fx_launch_log(int32_t* out, int32_t max_records, int32_t reset);
int32_t fx_conv_instances(int32_t* out, int32_t max_records);
int32_t fx_conv_any_sums_instances(int32_t* out, int32_t max_records);      // the ragged image-fed BatchNorm instances, a list of their own (p3d_fx_conv_any_sums_instances)
// Which convolutions the x3 kernels take, per pass: one rule each (p3d_fx.hip).  min_m: the least channel count of the result's tile rows the caller finds worth it (96:
// the per-layer entries; 64: the block executor; 32: image-fed and inference callers).  ragged: the instances that take any map width -- the same rule without its
// width / alignment clauses (forward: W % 4, Wo % 4; data gradient: those, and stride 1 only; weight gradient: (Ho Wo) % 16, Wo % 4, W % 4), so it cannot drift
// from the aligned one.
enum FxPass { FX_FWD, FX_DGRAD, FX_WGRAD };
bool fx_applies(FxPass pass, const p3d_conv_desc* d, int min_m = 96, bool ragged = false);
bool fx_masked_applies(FxPass pass, const p3d_conv_desc* d, bool ragged = false);      // partial convolutions: the masked instances take no bias (ragged: all three passes -- inference and, under p3d_x3_any_partial_enable, training; the data gradient stride 1 only)
// the stride-2 data gradient at any map side: fx_applies(FX_DGRAD) for stride 2 without its H % 2, W % 8 and width clauses, whole weights only
bool fx_dgrad_strided_any_applies(const p3d_conv_desc* d, int min_m = 96);
// ... its workspace (the weight image, then four tight class planes [N C][OHc][OWc] cls_stride floats apart, plane ph * 2 + pw; each part on a 256-B line) and its class
// launches: one ragged fp32-fed launch per live, non-empty parity class into its plane.  live_mask: bit cls set where a tap reaches the class.  The caller interleaves
// the planes into dx (dgrad_interleave_rows_kernel, p3d_conv.hip)
struct FxStridedPlan { size_t stage_offset, cls_stride, workspace; };      // bytes, floats, bytes
FxStridedPlan fx_dgrad_strided_any_plan(const p3d_conv_desc* d);
// dy_img (optional): the plane image of dy (fx_act_image_any) instead of dy -- the class launches on the image-fed ragged FX_EPI_STORE instance, same geometry, same
// planes; wimgT (with dy_img, optional): the cached data-gradient weight image, nothing is built; join: the caller finishes with block_strided_join_any_kernel
// (p3d_block.hip) instead of the interleave, which the record of the last class launch says
int32_t fx_conv_dgrad_strided_any(const p3d_conv_desc* d, const float* dy, const float* w, void* workspace, size_t workspace_bytes, int* live_mask, hipStream_t st,
                                  const void* dy_img = nullptr, const void* wimgT = nullptr, bool join = false);
// the interleave behind the class launches (p3d_conv.hip: dgrad_interleave_rows_kernel on a bounded grid), for p3d_conv2d_dgrad and the block executor alike
int32_t fx_dgrad_interleave_rows(const float* stage, float* dx, const float* mask_in, int N, int C, int H, int W, size_t cls_stride, int live, int accumulate, hipStream_t st);
size_t fx_workspace(FxPass pass, const p3d_conv_desc* d, bool ragged = false);         // FX_FWD / FX_DGRAD: weight image + split-K slabs of the call's plan; FX_WGRAD: slabs for the larger of the two
                                                                                       // split counts (fp32- or image-fed x), what a caller reserves before it knows which
int fx_partial_rows(FxPass pass, const p3d_conv_desc* d, bool ragged = false);         // FX_FWD / FX_DGRAD: rows of the per-channel partial sums of a launch with a sums epilogue (ragged: never split, one row per 128-pixel tile)
bool fx_dgrad_has_dead_classes(const p3d_conv_desc* d);
int32_t fx_dgrad_zero_dead_classes(const p3d_conv_desc* d, float* dx, hipStream_t st);      // zero-fills dx when the call does not accumulate and leaves such pixels untouched
bool fx_dgrad_accumulates_from_source(const p3d_conv_desc* d);      // stride 1 and no split-K: FxFuse::acc_src is honoured
int32_t fx_conv_fwd(const p3d_conv_desc* d, const float* x, const float* w, const float* bias, float* y, void* workspace, size_t workspace_bytes,
                    const FxFuse* fuse, hipStream_t st);
int32_t fx_conv_dgrad(const p3d_conv_desc* d, const float* dy, const float* w, float* dx, void* workspace, size_t workspace_bytes, const FxFuse* fuse,
                      hipStream_t st);
// p3d_conv.hip: fold the split slabs and write (or add) the weight gradient in the weight's own [K][C][R][S] layout; `launched`, when given, receives which kernels
// ran, as the finishing bits of p3d_conv_last_fp32_launch
int32_t wgrad_finish(const p3d_conv_desc* d, float* slabs, int nslab, bool tapm, float* dw, hipStream_t st, int32_t* launched = nullptr);
size_t fx_weight_image_bytes(int K, int C, int RS, bool bwd);
int32_t fx_build_weight_images(const float* w, int K, int C, int RS, void* img_fwd, void* img_bwd, hipStream_t st, int ctot = 0, int coff = 0);      // ctot > 0: a window of C input channels at coff
int32_t fx_build_weight_images_batched(const void* jobs, int njobs, int blocks, hipStream_t st);      // jobs: device array of {w, fwd, bwd, K, C, RS, pad} (40 B each)
// eval-mode BatchNorm folded into forward weight images (p3d_fx_fold_bn_images): jobs = device array of p3d_fold_job
int32_t fx_fold_bn_images(const void* jobs, int njobs, int blocks, hipStream_t st);
// The weight gradient.  fx_wgrad_plan is the single description of a call, derived from the descriptor and from the kinds of its operands -- what the FxFuse HOLDS (null:
// two fp32 operands on aligned maps): the workspace queries, fx_conv_wgrad and the test hook p3d_fx_wgrad_plan all read it, so the slab count, the grid and the kernel
// cannot disagree.  Everything but `ok` is filled for any operands -- a query asks before an operand exists.
enum : int { FX_WG_ALIGNED = 0, FX_WG_ANY = 1, FX_WG_ANY_MASKED = 2, FX_WG_ANY_IMG = 3 };
struct FxWgradOperands { bool aimg, bimg, pm, em, rows, ragged; };      // dy / x is an image; dy / x has a per-pixel factor; the images are row images; any map width
struct FxWgradPlan {
    bool ok;                // an instance takes this combination of operands (fx_wgrad_operands_ok); fx_conv_wgrad refuses the others with P3D_EINVAL
    int family;             // the kernel: FX_WG_ALIGNED fx_wgrad_kernel; FX_WG_ANY, _ANY_MASKED, _ANY_IMG fx_wgrad_any_kernel, _any_masked_kernel, _any_img_kernel
    bool aimg, bimg, masked;        // FX_WG_ALIGNED: the template arguments of fx_wgrad_kernel<aimg, bimg, masked, taps, rows>; 0 for the other families
    int taps;
    bool rows;
    int tile_taps;          // filter taps per column tile: 0 (one tap per block), 2 or 3 (image-fed multi-tap layers with 64 input channels), 8 (the stem)
    int splits, spb;        // slabs the pixel reduction is cut into, and K steps (16 pixels each) per slab
    dim3 grid;
    int order;              // FxWgradParams::order
    size_t slab_bytes;      // `splits` slabs of [K][taps][C] floats: the workspace of the call
    bool tapm;              // a slab's columns are tap-major (wgrad_finish transposes them into the weight's order)
};
FxWgradPlan fx_wgrad_plan(const p3d_conv_desc* d, const FxWgradOperands& o);
inline FxWgradPlan fx_wgrad_plan(const p3d_conv_desc* d, const FxFuse* f) {
    return fx_wgrad_plan(d, f ? FxWgradOperands{f->dy_img != nullptr, f->x_img != nullptr, f->pmask != nullptr, f->emask != nullptr, f->rows != 0, f->ragged != 0} : FxWgradOperands{});
}
int32_t fx_wgrad_plan_record(const p3d_conv_desc* d, int operands, int32_t* out);      // the test hook p3d_fx_wgrad_plan (include/p3d_hip.h)
// the log of weight-gradient launches (p3d_fx_wgrad_launch_log: include/p3d_hip.h): the plan that was launched, the finishing kernels behind it, `accumulate`
int32_t fx_wgrad_launch_log(int32_t* out, int32_t max_records, int32_t reset);
// plan -> workspace check ("<entry>: workspace %zu B < required %zu B", P3D_EWORKSPACE) -> slabs -> wgrad_finish: dw = (or +=, by `accumulate`) the weight gradient.
// dy / x: the fp32 operands, ignored where the FxFuse holds the image.
int32_t fx_conv_wgrad(const p3d_conv_desc* d, const float* dy, const float* x, float* dw, int accumulate, void* workspace, size_t workspace_bytes, const FxFuse* fuse,
                      const char* entry, hipStream_t st);
// Pre-split activation images: a fp32 NCHW tensor [N][C][HW] (C % 16 == 0, HW % 4 == 0) as three bf16 planes [N][C/16][HW][16] (hi + mid + lo == value exactly):
// what the x3 kernels stage into LDS with plain 16-B copies.  mode 0: the tensor itself; 1: relu(x * sc + sh) with the table's constants per channel;
// 2: A * (masked ? g * [c * sc + sh > 0] : g) + B * c + K (x = g, x2 = c): the BatchNorm-backward map.
// `fin` (optional): the finalize step of the BatchNorm layer the pass belongs to, done in the pass's prologue instead of a launch of its own -- every block sums the
// per-channel partial sums of its 16 channels (fp64, fixed order: all blocks get the same constants), block x == 0 also writes what a finalize kernel would
// (table / running statistics, or d gamma / d beta).  For few partial rows only (each block re-reads rows * 16 channels); the caller decides.
struct FxFinalize {
    int kind;               // 1: MODE 1, batch statistics from fp32 partials [rows][C][2] = (sum y, sum y^2);  2: MODE 2, backward sums from fp32 partials [rows][C][2] =
                            // (sum g, sum g (c - mean));  3: MODE 2, the same from fp64 partials [C][rows][3] (second sum at index 1 + which)
    const void* partial;
    int rows, which;
    double count;           // N * H * W
    const float* gamma;
    const float* beta;      // kind 1
    float* running_mean;    // kind 1, may be null
    float* running_var;
    float momentum, eps;    // kind 1
    float* dgamma;          // kind 2 / 3
    float* dbeta;
    int accumulate;         // kind 2 / 3: add to d gamma / d beta instead of overwriting
    float* table;           // the layer's [C][8] table: kind 1 writes {sc, sh, mean, invstd}; kind 2 / 3 read them
    const unsigned char* gmask;   // kind 3, optional: x is the gradient in FRONT of a ReLU whose mask bytes these are (bit e of byte i: element 4 i + e passes); the pass
                                  // applies the mask itself, so the masked gradient never has to exist in memory (p3d_block_io.out_mask)
};
constexpr int FX_FIN_MAX_ROWS = 512;
size_t fx_act_image_bytes(int64_t N, int64_t C, int64_t HW);
// Row images: the same channel-blocked rows holding the fp32 value itself, [N][C/16][HW][16] floats; `rows` below writes one instead of the three planes (same modes,
// finalize prologue, mask bytes and pixmul).  fx_block_row_images: the format the block executor keeps a_i / d c_i of DENSE blocks in (p3d_fx_tune(6, 1): planes)
size_t fx_row_image_bytes(int64_t N, int64_t C, int64_t HW);
bool fx_block_row_images();
bool fx_pair_map_enabled();
// pixmul (optional, [N][HW]): the image holds the tensor times this per-pixel factor (partial convolutions inside the block executor)
int32_t fx_act_image_pair(const float* x, const unsigned char* gmask, const float* c_a, const float* c_b, void* img_a, void* img_b, const FxFinalize* fa, const FxFinalize* fb,
                          int N, int C, int HW, hipStream_t st, const float* pixmul_a = nullptr, bool rows = false);
int32_t fx_act_image(int mode, const float* x, const float* x2, const float* table, int masked, void* img, int N, int C, int HW, hipStream_t st,
                     const FxFinalize* fin = nullptr, const float* pixmul = nullptr, bool rows = false);
// mode 0 at any HW (the same bytes; x read with dword loads where a row is not 16-B aligned, the last pixel group of an image partial)
int32_t fx_act_image_any(const float* x, void* img, int N, int C, int HW, hipStream_t st);
// modes 1 and 2 at any HW, plane images only: the maps and the optional finalize prologue of fx_act_image (kinds 1, 2, 3; null: the table), no mask bytes, no pixmul
int32_t fx_act_image_any_map(int mode, const float* x, const float* x2, const float* table, int masked, void* img, int N, int C, int HW, hipStream_t st,
                             const FxFinalize* fin = nullptr);

// The 7x7 stride-2 stem (Cin = 1..4) as a 4x4 stride-1 convolution over a space-to-depth image of the input (p3d_fx.hip)
bool fx_stem_applies(int N, int Cin, int H, int W, int K);
size_t fx_stem_image_bytes(int N, int H, int W);
size_t fx_stem_weight_image_bytes(int K);
size_t fx_stem_workspace(int N, int H, int W, int K);
int32_t fx_stem_image(const float* x, const float* mask, void* img, int N, int Cin, int H, int W, hipStream_t st);      // mask: per-pixel factor of x [N][1][H][W], or null
// the space-to-depth image of x zero-extended to (Hp, Wp) >= (H, W): dword fetches checked against the true sides, every pixel beyond them an exact zero
int32_t fx_stem_image_any(const float* x, const float* mask, void* img, int N, int Cin, int H, int W, int Hp, int Wp, hipStream_t st);
bool fx_stem_masked_applies(int K);
int32_t fx_stem_weight_image(const float* w, int K, int Cin, void* wimg, void* workspace, hipStream_t st);
// mult: per-pixel factor of the result (forward) / of dy (weight gradient), [N][1][H/2][W/2], or null -- the partial-convolution stem of the partial families
int32_t fx_stem_fwd(const void* x_img, const void* wimg, float* y, const float* mult, int N, int H, int W, int K, hipStream_t st);
int32_t fx_stem_wgrad(const float* dy, const float* mult, const void* x_img, float* dw, int N, int Cin, int H, int W, int K, int accumulate, void* workspace,
                      size_t workspace_bytes, hipStream_t st);

}  // namespace p3d
