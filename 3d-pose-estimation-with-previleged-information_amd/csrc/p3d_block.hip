// One residual block (BasicBlock / Bottleneck: depthnet.py:10-56,59-116 and the twins in resnet.py / fusionnet.py) per C-ABI call, training mode:
// forward and backward of   conv -> BN -> ReLU -> conv -> BN -> ReLU [-> conv -> BN] -> (+ identity | downsample conv -> BN) -> [ReLU]
// with the statistics / backward sums of the BatchNorm layers produced in the convolutions' epilogues (p3d_fx.hip) and everything that used to be host
// work of the Python autograd wrappers (workspace carving, the second stream of the weight gradients and its events, the gradient join at the block
// input) done here: one call instead of ~12 per direction.
//
// Tensors produced inside the block and consumed only by convolutions -- a_i = relu(bn_i(c_i)) and d c_i = the BatchNorm-backward map of the incoming
// gradient -- exist only as activation images (fx_act_image), channel-blocked rows [N][C/16][HW][16] in which every filter tap and stride of the two or three
// kernels that read them lands on an aligned row.  Dense blocks: fp32 row images, 4 B per element, written once by the pass that applies the BatchNorm map and
// cut into the three bf16 pieces by the row-fed kernel instances on the way into LDS.  Masked blocks (and every block under p3d_fx_tune(6, 1)): three
// pre-split bf16 planes, hi + mid + lo == the fp32 value, 6 B per element, staged with plain 16-B copies.  block_row_images() decides.  The block input x and
// the gradients that leave a data gradient stay fp32.
//
// HBM passes that are BatchNorm's own, per block: forward, per inner layer the image pass (reads c_i, writes the image of a_i) and one pass that closes
// the block (out = act(bn(c_last) + shortcut)); backward, one pass that opens it (g = dout * [out > 0] plus the channel sums of the closing BN and of
// the downsample BN) and per layer the image pass of d c_i (reads g and c_i).
//
// Blocks at map sizes the aligned kernels refuse ("ragged" blocks, block_ragged: plane images, the ragged image-fed conv instances, passes for any HW) are opt-in:
// p3d_block_any_enable takes the ones whose convolutions all have stride 1, p3d_block_any_strided_enable the ones that carry a stride-2 convolution -- there a data
// gradient is a set of class launches into tight class planes, and a main-chain one costs one more pass of BatchNorm's own, block_strided_join_any_kernel (the
// planes -> the gradient w.r.t. a_{i-1} and its channel sums at once).
#include "p3d_common.h"
#include "p3d_fx.h"
#include <vector>
#include <mutex>

namespace p3d {

using f32x4 = float __attribute__((ext_vector_type(4)));

constexpr int CLOSE_MAX_SPLIT = 64;
constexpr int FIN_CH = 16, FIN_MAX_LANES = 64;  // finalize kernels: a block sums 16 channels with blockDim / 16 row lanes each (16 lanes, or 64 when there are many rows)
static inline unsigned fin_threads(int rows) { return rows > 64 ? 1024u : 256u; }
// forward / data gradient / weight gradient from 64 channels up: half-filled 128-row tiles issue no MFMAs for their dead half (fx_live_subtiles), and
// image-fed kernels spend nothing on staging them
constexpr int BLOCK_MIN_M = 64;
// which convolutions the executor takes.  Every operand that is produced inside the block travels as a pre-split activation image, so all three passes of
// every convolution must be on the x3 kernels (there is no fp32 copy of a_i / d c_i for another kernel to read).  A main-chain convolution whose strided
// data gradient leaves input pixels untouched (1x1, stride 2: fx_dgrad_has_dead_classes) is refused: its gradient buffer is not zero-filled here (the
// reference's blocks put the stride on the 3x3; the strided 1x1 of a downsample branch ADDS onto a gradient that is already complete).
static bool block_slot(const p3d_block_desc* b, int i) { return i < b->nconv || (i == 3 && b->has_downsample); }      // slots 0 .. nconv - 1: the main chain; 3: the downsample conv
static bool block_conv_ok(const p3d_conv_desc* d, bool main_chain) {
    return fx_applies(FX_FWD, d, BLOCK_MIN_M) && fx_applies(FX_DGRAD, d, BLOCK_MIN_M) && fx_applies(FX_WGRAD, d, BLOCK_MIN_M) && (d->Ho * d->Wo) % 4 == 0 &&
           (d->H * d->W) % 4 == 0 && d->C % 16 == 0 && d->K % 16 == 0 && !(main_chain && fx_dgrad_has_dead_classes(d));
}
// The same at any map width (p3d_block_any_enable / P3D_BLOCK_ANY=1, default off): the rule above without its map-size clauses, on the ragged instances -- all three passes
// of every convolution at stride 1 (the ragged data gradient has no parity classes), whole weights, and a map of at least one K step of the image-fed weight gradient
static int g_block_any = -1;       // -1: not decided yet (environment), 0 / 1: set
static bool block_any_enabled() {
    if (g_block_any < 0) { const char* e = getenv("P3D_BLOCK_ANY"); g_block_any = (e && atoi(e) == 1) ? 1 : 0; }
    return g_block_any == 1;
}
static bool block_conv_any_ok(const p3d_conv_desc* d) {
    // (the last clause is the operand rule of the weight gradient every slot of a ragged block runs -- both operands images, any map width: fx_wgrad_operands_ok,
    // which is where "a map of at least one K step" is stated; asked of the plan so that the two cannot drift apart)
    FxWgradOperands both_images{};
    both_images.aimg = both_images.bimg = both_images.ragged = true;
    return d->stride == 1 && fx_applies(FX_FWD, d, BLOCK_MIN_M, true) && fx_applies(FX_DGRAD, d, BLOCK_MIN_M, true) && fx_applies(FX_WGRAD, d, BLOCK_MIN_M, true) &&
           d->C % 16 == 0 && d->K % 16 == 0 && d->c_offset == 0 && d->c_total == d->C && fx_wgrad_plan(d, both_images).ok;
}
// Ragged blocks that carry a stride-2 convolution (p3d_block_any_strided_enable / P3D_BLOCK_ANY_STRIDED=1, default off; a switch of its own: it looks at no other and no
// other at it -- the executor never reads p3d_x3_any_strided_enable).  The any-width rule of a stride-2 slot: the image-fed ragged forward and weight gradient take the
// stride as they are; the data gradient is the class launches of fx_conv_dgrad_strided_any, image-fed, into tight class planes in the conv scratch, finished by
// block_strided_join_any_kernel (a main-chain slot: da and the BatchNorm-backward sums in one pass) or by the interleave (conv 0 and the downsample conv: no sums to take).
// A main-chain 1x1 stride 2 is refused as in the aligned rule.
static int g_block_any_strided = -1;
static bool block_any_strided_enabled() {
    if (g_block_any_strided < 0) { const char* e = getenv("P3D_BLOCK_ANY_STRIDED"); g_block_any_strided = (e && atoi(e) == 1) ? 1 : 0; }
    return g_block_any_strided == 1;
}
static bool block_conv_any_strided_ok(const p3d_conv_desc* d, bool main_chain) {
    FxWgradOperands both_images{};
    both_images.aimg = both_images.bimg = both_images.ragged = true;
    return d->stride == 2 && fx_applies(FX_FWD, d, BLOCK_MIN_M, true) && fx_dgrad_strided_any_applies(d, BLOCK_MIN_M) && fx_applies(FX_WGRAD, d, BLOCK_MIN_M, true) &&
           d->C % 16 == 0 && d->K % 16 == 0 && d->c_offset == 0 && d->c_total == d->C && fx_wgrad_plan(d, both_images).ok && !(main_chain && fx_dgrad_has_dead_classes(d));
}

__device__ __forceinline__ void blk_sum3(double& a, double& b, double& c, double* red /*[12]*/) {
    a = wave_sum(a); b = wave_sum(b); c = wave_sum(c);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[w] = a; red[4 + w] = b; red[8 + w] = c; }
    __syncthreads();
    a = red[0] + red[1] + red[2] + red[3];
    b = red[4] + red[5] + red[6] + red[7];
    c = red[8] + red[9] + red[10] + red[11];
    __syncthreads();
}

// Forward finalize of one BatchNorm layer from the conv epilogue's partial sums: partial [rows][C][2] = (sum y, sum y^2) per pixel tile.
// One block per 64 channels, 4 row lanes per channel; fp64 combine.  Writes the table entries {sc, sh, mean, invstd} and updates the running statistics
// (momentum, unbiased variance) exactly as p3d_bn_train_fwd does.
__global__ __launch_bounds__(1024) void bn_finalize_fwd_kernel(const float* __restrict__ partial, int rows, int C, double count, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float* running_mean, float* running_var, float momentum, float eps,
                                                              float* __restrict__ table) {
    const int cl = threadIdx.x & (FIN_CH - 1), rl = threadIdx.x / FIN_CH, c = blockIdx.x * FIN_CH + cl, FIN_LANES = blockDim.x / FIN_CH;
    double s1 = 0.0, s2 = 0.0;
    if (c < C) {
        // two rows per trip with independent loads (a launch that does nothing else should not chain its round trips)
        double u1 = 0.0, u2 = 0.0;
        int r = rl;
        for (; r + FIN_LANES < rows; r += 2 * FIN_LANES) {
            const float2 v = *reinterpret_cast<const float2*>(partial + ((size_t)r * C + c) * 2);
            const float2 w = *reinterpret_cast<const float2*>(partial + ((size_t)(r + FIN_LANES) * C + c) * 2);
            s1 += v.x; s2 += v.y; u1 += w.x; u2 += w.y;
        }
        if (r < rows) {
            const float2 v = *reinterpret_cast<const float2*>(partial + ((size_t)r * C + c) * 2);
            s1 += v.x; s2 += v.y;
        }
        s1 += u1; s2 += u2;
    }
    __shared__ double red[2][FIN_MAX_LANES][FIN_CH];
    red[0][rl][cl] = s1; red[1][rl][cl] = s2;
    __syncthreads();
    if (rl != 0 || c >= C) return;
    s1 = s2 = 0.0;
    for (int i = 0; i < FIN_LANES; ++i) { s1 += red[0][i][cl]; s2 += red[1][i][cl]; }       // fixed order (the lane count follows from `rows` alone): bitwise reproducible
    const double mean = s1 / count;
    double var = s2 / count - mean * mean;
    if (var < 0.0) var = 0.0;
    const float invstd = (float)(1.0 / sqrt(var + (double)eps));
    const float fmean = (float)mean;
    const float sc = invstd * gamma[c];
    float* t = table + (size_t)c * FX_TAB;
    t[0] = sc; t[1] = __fmaf_rn(-fmean, sc, beta[c]); t[2] = fmean; t[3] = invstd;
    if (running_mean) {
        const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
        running_mean[c] = (float)((1.0 - momentum) * running_mean[c] + momentum * mean);
        running_var[c] = (float)((1.0 - momentum) * running_var[c] + momentum * unbiased);
    }
}

// Backward finalize: partial [rows][C][2] (fp32, from a dgrad epilogue / its split-K reduce) or [C][rows][3] fp64 (from the block-opening pass; `which` picks
// the second sum) = (sum g, sum g * (c - mean)).  dbeta = sum g, dgamma = invstd * sum g (c - mean); table {A, B, K}:  d c = A g + B c + K  with
// A = gamma invstd, B = -A invstd m2, K = A (mean invstd m2 - m1), m1 = dbeta / count, m2 = dgamma / count.
template <bool F64>
__global__ __launch_bounds__(1024) void bn_finalize_bwd_kernel(const void* __restrict__ partial_, int rows, int C, double count, int which, const float* __restrict__ gamma,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta, int accumulate, float* __restrict__ table) {
    const int cl = threadIdx.x & (FIN_CH - 1), rl = threadIdx.x / FIN_CH, c = blockIdx.x * FIN_CH + cl, FIN_LANES = blockDim.x / FIN_CH;
    double s1 = 0.0, s2 = 0.0;
    if (c < C) {
        double u1 = 0.0, u2 = 0.0;            // (two rows per trip with independent loads, as in bn_finalize_fwd_kernel)
        int r = rl;
        if constexpr (F64) {
            const double* partial = (const double*)partial_ + (size_t)c * rows * 3;
            const int o = 1 + which;
            for (; r + FIN_LANES < rows; r += 2 * FIN_LANES) {
                const double a0 = partial[r * 3], b0 = partial[r * 3 + o], a1 = partial[(r + FIN_LANES) * 3], b1 = partial[(r + FIN_LANES) * 3 + o];
                s1 += a0; s2 += b0; u1 += a1; u2 += b1;
            }
            if (r < rows) { s1 += partial[r * 3]; s2 += partial[r * 3 + o]; }
        } else {
            const float* partial = (const float*)partial_;
            for (; r + FIN_LANES < rows; r += 2 * FIN_LANES) {
                const float2 v = *reinterpret_cast<const float2*>(partial + ((size_t)r * C + c) * 2);
                const float2 w = *reinterpret_cast<const float2*>(partial + ((size_t)(r + FIN_LANES) * C + c) * 2);
                s1 += v.x; s2 += v.y; u1 += w.x; u2 += w.y;
            }
            if (r < rows) {
                const float2 v = *reinterpret_cast<const float2*>(partial + ((size_t)r * C + c) * 2);
                s1 += v.x; s2 += v.y;
            }
        }
        s1 += u1; s2 += u2;
    }
    __shared__ double red[2][FIN_MAX_LANES][FIN_CH];
    red[0][rl][cl] = s1; red[1][rl][cl] = s2;
    __syncthreads();
    if (rl != 0 || c >= C) return;
    s1 = s2 = 0.0;
#pragma unroll
    for (int i = 0; i < FIN_LANES; ++i) { s1 += red[0][i][cl]; s2 += red[1][i][cl]; }
    float* t = table + (size_t)c * FX_TAB;
    const float mean = t[2], is = t[3];
    const double dg = (double)is * s2;
    dbeta[c] = accumulate ? dbeta[c] + (float)s1 : (float)s1;
    dgamma[c] = accumulate ? dgamma[c] + (float)dg : (float)dg;
    const float m1 = (float)(s1 / count), m2 = (float)(dg / count);
    const float A = gamma[c] * is;
    t[4] = A; t[5] = -A * is * m2; t[6] = A * (mean * is * m2 - m1); t[7] = 0.f;
}

// What bn_finalize_fwd_kernel does for ONE channel, by a whole 256-thread block (the closing pass: one channel per block): thread t sums partial rows t, t + 256, ...
// in fp64, then the block combines them in a fixed order, so that every block of a channel arrives at the same constants.
struct CloseFin {
    const float* partial;   // [rows][C][2] = (sum y, sum y^2), or null: no BatchNorm on this operand (identity shortcut)
    int rows;
    const float* gamma;
    const float* beta;
    float* running_mean;
    float* running_var;
    float momentum, eps;
    float* table;
};
__device__ __forceinline__ void close_finalize(const CloseFin& f, int ch, int C, double count, bool owner, double* red /*[12]*/, float& sc, float& sh) {
    if (f.rows <= 0) {            // finalized by a launch of its own (many partial rows: every (channel, image group) block would re-read them all): the table holds the constants
        sc = f.table[(size_t)ch * FX_TAB]; sh = f.table[(size_t)ch * FX_TAB + 1];
        return;
    }
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int r = threadIdx.x; r < f.rows; r += 256) {
        const float2 v = *reinterpret_cast<const float2*>(f.partial + ((size_t)r * C + ch) * 2);
        s1 += v.x; s2 += v.y;
    }
    blk_sum3(s1, s2, s3, red);
    const double mean = s1 / count;
    double var = s2 / count - mean * mean;
    if (var < 0.0) var = 0.0;
    const float invstd = (float)(1.0 / sqrt(var + (double)f.eps));
    const float fmean = (float)mean;
    sc = invstd * f.gamma[ch];
    sh = __fmaf_rn(-fmean, sc, f.beta[ch]);
    if (owner && threadIdx.x == 0) {
        float* t = f.table + (size_t)ch * FX_TAB;
        t[0] = sc; t[1] = sh; t[2] = fmean; t[3] = invstd;
        if (f.running_mean) {
            const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
            f.running_mean[ch] = (float)((1.0 - f.momentum) * f.running_mean[ch] + f.momentum * mean);
            f.running_var[ch] = (float)((1.0 - f.momentum) * f.running_var[ch] + f.momentum * unbiased);
        }
    }
}

// Closes the block in forward: out = act(c * sc + sh + shortcut), shortcut = res (identity) or rc * rsc + rsh (the downsample conv's raw output and its BN).
// The batch statistics of the closing BatchNorm (and of the downsample BatchNorm) are finalized here, from the partial sums their convolutions' epilogues left.
// grid (C, split): block (c, s) owns images n = s, s + split, ...; block (c, 0) writes the channel's table entry and running statistics.
__global__ __launch_bounds__(256) void block_close_fwd_kernel(const float* __restrict__ c, const CloseFin fin, const float* __restrict__ res, const CloseFin rfin,
                                                              float* __restrict__ out, unsigned char* __restrict__ omask, int N, int C, int HW, int relu, double count) {
    const int ch = blockIdx.x, s = blockIdx.y, split = gridDim.y;
    __shared__ double red[12];
    float sc, sh, rsc = 1.f, rsh = 0.f;
    close_finalize(fin, ch, C, count, s == 0, red, sc, sh);
    const bool ds = rfin.partial != nullptr;
    if (ds) close_finalize(rfin, ch, C, count, s == 0, red, rsc, rsh);
    // One flat index over (this block's images, 16-B groups of the channel's plane): on the 16 x 16 maps a plane is 64 groups, and a loop per image would leave three
    // quarters of the block idle in every trip; two groups per trip keep four 16-B loads in flight per thread.
    const int q4 = HW >> 2, nimg = (N - s + split - 1) / split, total = nimg * q4;
    auto at = [&](int j) { const int k = j / q4; return ((size_t)(s + k * split) * C + ch) * (size_t)q4 + (j - k * q4); };      // index in 16-B groups
    const f32x4* cv = reinterpret_cast<const f32x4*>(c);
    const f32x4* rv = reinterpret_cast<const f32x4*>(res);
    f32x4* ov = reinterpret_cast<f32x4*>(out);
    auto one = [&](f32x4 q, const f32x4 r, size_t g) {
        unsigned m = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v = fmaf(q[e], sc, sh) + (ds ? fmaf(r[e], rsc, rsh) : r[e]);
            m |= (v > 0.f ? 1u : 0u) << e;
            q[e] = relu ? fmaxf(v, 0.f) : v;
        }
        ov[g] = q;
        if (omask) omask[g] = (unsigned char)m;           // which of the four outputs are positive: what the backward pass needs of `out` (1 byte instead of 16)
    };
    int j = threadIdx.x;
    for (; j + 256 < total; j += 512) {
        const size_t g0 = at(j), g1 = at(j + 256);
        const f32x4 q0 = cv[g0], r0 = rv[g0], q1 = cv[g1], r1 = rv[g1];
        one(q0, r0, g0);
        one(q1, r1, g1);
    }
    if (j < total) { const size_t g0 = at(j); one(cv[g0], rv[g0], g0); }
}

// Opens the block in backward: g = relu ? dout * [out > 0] : dout (written to gbuf when relu), and per channel the sums of g, g * (c - mean) and, with a
// downsample branch, g * (rc - rmean).  partial [C][split][3] fp64.  [out > 0] comes from the forward pass's mask bytes when the caller keeps them (omask),
// else from `out` itself.
__global__ __launch_bounds__(256) void block_open_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ out, const float* __restrict__ c,
                                                             const float* __restrict__ tab, const float* __restrict__ rc, const float* __restrict__ rtab,
                                                             float* __restrict__ gbuf, double* __restrict__ partial, const unsigned char* __restrict__ omask, int N, int C,
                                                             int HW, int relu) {
    const int ch = blockIdx.x, s = blockIdx.y, split = gridDim.y;
    const float mean = tab[ch * FX_TAB + 2], rmean = rtab ? rtab[ch * FX_TAB + 2] : 0.f;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    // (one flat index over this block's images and 16-B groups, as in block_close_fwd_kernel: the 16 x 16 maps have 64 groups per plane)
    const int q4 = HW >> 2, nimg = (N - s + split - 1) / split, total = nimg * q4;
    const f32x4* dv = reinterpret_cast<const f32x4*>(dout);
    const f32x4* ov = reinterpret_cast<const f32x4*>(out);
    const f32x4* cv = reinterpret_cast<const f32x4*>(c);
    const f32x4* rv = reinterpret_cast<const f32x4*>(rc);
    f32x4* gv = reinterpret_cast<f32x4*>(gbuf);
    for (int j = threadIdx.x; j < total; j += 256) {
        const int k = j / q4;
        const size_t i = ((size_t)(s + k * split) * C + ch) * (size_t)q4 + (j - k * q4);
        f32x4 g = dv[i];
        const f32x4 q = cv[i];
        if (relu) {
            if (omask) {
                const unsigned m = omask[i];
#pragma unroll
                for (int e = 0; e < 4; ++e) g[e] = (m >> e) & 1u ? g[e] : 0.f;
            } else {
                const f32x4 o = ov[i];
#pragma unroll
                for (int e = 0; e < 4; ++e) g[e] = o[e] > 0.f ? g[e] : 0.f;
            }
            if (gbuf) gv[i] = g;           // (null: a block with a downsample branch and mask bytes -- nobody reads g as a tensor, the image passes mask dout themselves)
        }
        float a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) { a1 += g[e]; a2 = fmaf(g[e], q[e] - mean, a2); }
        if (rc) {
            const f32x4 r = rv[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) a3 = fmaf(g[e], r[e] - rmean, a3);
        }
        s1 += a1; s2 += a2; s3 += a3;
    }
    __shared__ double red[12];
    blk_sum3(s1, s2, s3, red);
    if (threadIdx.x == 0) {
        double* dst = partial + ((size_t)ch * split + s) * 3;
        dst[0] = s1; dst[1] = s2; dst[2] = s3;
    }
}

// The two passes at any HW (a ragged block: a channel plane of odd length is only 4-B aligned): one element per lane over the same flat index, the same grid,
// expressions and fp64 sums.  No mask bytes (a plane's last byte would be shared with the next plane's first): backward takes [out > 0] from `out`, and g is
// always written when the block ends in a ReLU.
__global__ __launch_bounds__(256) void block_close_fwd_any_kernel(const float* __restrict__ c, const CloseFin fin, const float* __restrict__ res, const CloseFin rfin,
                                                                  float* __restrict__ out, int N, int C, int HW, int relu, double count) {
    const int ch = blockIdx.x, s = blockIdx.y, split = gridDim.y;
    __shared__ double red[12];
    float sc, sh, rsc = 1.f, rsh = 0.f;
    close_finalize(fin, ch, C, count, s == 0, red, sc, sh);
    const bool ds = rfin.partial != nullptr;
    if (ds) close_finalize(rfin, ch, C, count, s == 0, red, rsc, rsh);
    const int nimg = (N - s + split - 1) / split, total = nimg * HW;
    for (int j = threadIdx.x; j < total; j += 256) {
        const int k = j / HW;
        const size_t i = ((size_t)(s + k * split) * C + ch) * (size_t)HW + (j - k * HW);
        const float r = res[i], v = fmaf(c[i], sc, sh) + (ds ? fmaf(r, rsc, rsh) : r);
        out[i] = relu ? fmaxf(v, 0.f) : v;
    }
}

__global__ __launch_bounds__(256) void block_open_bwd_any_kernel(const float* __restrict__ dout, const float* __restrict__ out, const float* __restrict__ c,
                                                                 const float* __restrict__ tab, const float* __restrict__ rc, const float* __restrict__ rtab,
                                                                 float* __restrict__ gbuf, double* __restrict__ partial, int N, int C, int HW, int relu) {
    const int ch = blockIdx.x, s = blockIdx.y, split = gridDim.y;
    const float mean = tab[ch * FX_TAB + 2], rmean = rtab ? rtab[ch * FX_TAB + 2] : 0.f;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    const int nimg = (N - s + split - 1) / split, total = nimg * HW;
    for (int j = threadIdx.x; j < total; j += 256) {
        const int k = j / HW;
        const size_t i = ((size_t)(s + k * split) * C + ch) * (size_t)HW + (j - k * HW);
        float g = dout[i];
        if (relu) {
            g = out[i] > 0.f ? g : 0.f;
            gbuf[i] = g;
        }
        s1 += g; s2 += g * (c[i] - mean);
        if (rc) s3 += g * (rc[i] - rmean);
    }
    __shared__ double red[12];
    blk_sum3(s1, s2, s3, red);
    if (threadIdx.x == 0) {
        double* dst = partial + ((size_t)ch * split + s) * 3;
        dst[0] = s1; dst[1] = s2; dst[2] = s3;
    }
}

// BatchNorm-backward sums for a data gradient whose kernel could not take them in its epilogue (strided dgrad): (sum gg, sum gg (c - mean)) with
// gg = g * [c * sc + sh > 0]; partial [C][split][3] fp64 like the opening pass
__global__ __launch_bounds__(256) void bn_bwd_sums_kernel(const float* __restrict__ g, const float* __restrict__ c, const float* __restrict__ tab,
                                                          double* __restrict__ partial, int N, int C, int HW) {
    const int ch = blockIdx.x, s = blockIdx.y, split = gridDim.y;
    const float sc = tab[ch * FX_TAB], sh = tab[ch * FX_TAB + 1], mean = tab[ch * FX_TAB + 2];
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int n = s; n < N; n += split) {
        const size_t off = ((size_t)n * C + ch) * HW;
        const f32x4* gv = reinterpret_cast<const f32x4*>(g + off);
        const f32x4* cv = reinterpret_cast<const f32x4*>(c + off);
        for (int i = threadIdx.x; i < HW / 4; i += 256) {
            const f32x4 gg = gv[i], q = cv[i];
            float a1 = 0.f, a2 = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float v = fmaf(q[e], sc, sh) > 0.f ? gg[e] : 0.f; a1 += v; a2 = fmaf(v, q[e] - mean, a2); }
            s1 += a1; s2 += a2;
        }
    }
    __shared__ double red[12];
    blk_sum3(s1, s2, s3, red);
    if (threadIdx.x == 0) {
        double* dst = partial + ((size_t)ch * split + s) * 3;
        dst[0] = s1; dst[1] = s2; dst[2] = 0.0;
    }
}

// The finishing pass behind the class launches of a main-chain stride-2 data gradient of a ragged block (fx_conv_dgrad_strided_any, image-fed): one streaming pass that
//   * writes g = the gradient w.r.t. a_{i-1}, [N][C][H][W] fp32, from the four tight class planes [N C][hc][wc] (hc = (H - ph + 1) / 2, wc = (W - pw + 1) / 2, plane
//     ph * 2 + pw at stage + cls * cls_stride) -- every value the one dgrad_interleave_rows_kernel writes, bit for bit (a move; the pixels of a class no tap reaches
//     get +0 and that plane is never read), and
//   * takes the BatchNorm-backward sums of the layer in front, (sum gg, sum gg (c - mean)) with gg = g * [c * sc + sh > 0], into the fp64 partials [C][split][3]
//     that bn_bwd_sums_kernel writes (bwd_map, kind 3, consumes them unchanged)
// instead of an interleave and a sums pass that reads g again.  grid (C, split) like the passes beside it: block (ch, s) owns the planes of channel ch in images
// s, s + split, ...  A plane of an odd map starts only on a 4-B line, so it is cut into slots: slot 0 the head up to g's next 16-B line (0 .. 3 elements), then the
// body in groups of four -- one 16-B store each, c in one 16-B-wide load --, then the tail (0 .. 3 elements); head and tail go element by element.  One flat index over
// (this block's images, slots) keeps the block busy on small planes.  A body group inside one row takes two consecutive floats from each of the row's two class rows
// (pair loads, as in dgrad_interleave_rows_kernel); one that runs over a row end gathers element by element and still stores 16 B.  The sums: per slot an fp32 partial
// of at most four terms (fmaf, as bn_bwd_sums_kernel keeps them), added in fp64 per thread, then blk_sum3 -- a fixed order, no atomics.
typedef float f32x2_dw __attribute__((ext_vector_type(2), aligned(4)));      // on a dword line: the compiler picks the widest load the target allows there
typedef float f32x4_dw __attribute__((ext_vector_type(4), aligned(4)));
__global__ __launch_bounds__(256) void block_strided_join_any_kernel(const float* __restrict__ stage, const float* __restrict__ c, const float* __restrict__ tab,
                                                                     float* __restrict__ g, double* __restrict__ partial, int N, int C, int H, int W, size_t cls_stride,
                                                                     int live_mask) {
    const int ch = blockIdx.x, s = blockIdx.y, split = gridDim.y;
    const float sc = tab[ch * FX_TAB], sh = tab[ch * FX_TAB + 1], mean = tab[ch * FX_TAB + 2];
    const int HW = H * W, hc1 = H >> 1, hc0 = H - hc1, wc1 = W >> 1, wc0 = W - wc1;
    const int SL = (HW >> 2) + 2;                   // slots per plane: head, at most HW / 4 body groups, tail
    const int nimg = (N - s + split - 1) / split, total = nimg * SL;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int j = threadIdx.x; j < total; j += 256) {
        const int k = j / SL, slot = j - k * SL;
        const unsigned nc = (unsigned)(s + k * split) * (unsigned)C + (unsigned)ch;
        const size_t off = (size_t)nc * HW;
        int head = (int)((0u - (unsigned)(reinterpret_cast<uintptr_t>(g + off) >> 2)) & 3u);      // elements in front of g's next 16-B line
        if (head > HW) head = HW;
        const int nbody = (HW - head) >> 2;
        int e0, cnt;
        if (slot == 0) { e0 = 0; cnt = head; }
        else if (slot <= nbody) { e0 = head + 4 * (slot - 1); cnt = 4; }
        else if (slot == nbody + 1) { e0 = head + 4 * nbody; cnt = HW - e0; }
        else continue;
        if (cnt == 0) continue;
        int hi = e0 / W, wi = e0 - hi * W;
        const float* cp = c + off + e0;
        float* gp = g + off + e0;
        float v[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
        if (cnt == 4 && wi + 3 < W) {
            // one row: even columns from class (ph, 0) at iw = wi / 2 (+ 1 from an odd start), odd columns from class (ph, 1)
            const int ph = hi & 1, o = wi & 1, iw = wi >> 1;
            const unsigned row = nc * (unsigned)(ph ? hc1 : hc0) + (unsigned)(hi >> 1);
            f32x2_dw a = {0.f, 0.f}, b = {0.f, 0.f};
            if ((live_mask >> (ph * 2)) & 1) a = *reinterpret_cast<const f32x2_dw*>(stage + (size_t)(ph * 2) * cls_stride + row * (unsigned)wc0 + (unsigned)(iw + o));
            if ((live_mask >> (ph * 2 + 1)) & 1) b = *reinterpret_cast<const f32x2_dw*>(stage + (size_t)(ph * 2 + 1) * cls_stride + row * (unsigned)wc1 + (unsigned)iw);
            v[0] = o ? b.x : a.x; v[1] = o ? a.x : b.x; v[2] = o ? b.y : a.y; v[3] = o ? a.y : b.y;
            const f32x4_dw qq = *reinterpret_cast<const f32x4_dw*>(cp);
            q[0] = qq.x; q[1] = qq.y; q[2] = qq.z; q[3] = qq.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (e < cnt) {
                    const int ph = hi & 1, pw = wi & 1, cls = ph * 2 + pw;
                    if ((live_mask >> cls) & 1)
                        v[e] = stage[(size_t)cls * cls_stride + (nc * (unsigned)(ph ? hc1 : hc0) + (unsigned)(hi >> 1)) * (unsigned)(pw ? wc1 : wc0) + (unsigned)(wi >> 1)];
                    q[e] = cp[e];
                }
                if (++wi == W) { wi = 0; ++hi; }      // (a slot never leaves its plane)
            }
        }
        if (cnt == 4) *reinterpret_cast<f32x4*>(gp) = f32x4{v[0], v[1], v[2], v[3]};
        else {
#pragma unroll
            for (int e = 0; e < 3; ++e)
                if (e < cnt) gp[e] = v[e];
        }
        float a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < cnt) { const float gg = fmaf(q[e], sc, sh) > 0.f ? v[e] : 0.f; a1 += gg; a2 = fmaf(gg, q[e] - mean, a2); }
        s1 += a1; s2 += a2;
    }
    __shared__ double red[12];
    blk_sum3(s1, s2, s3, red);
    if (threadIdx.x == 0) {
        double* dst = partial + ((size_t)ch * split + s) * 3;
        dst[0] = s1; dst[1] = s2; dst[2] = 0.0;
    }
}

static int close_split(int N, int C) {
    int split = (int)ceil_div(2048, C);
    if (split > N) split = N;
    if (split > CLOSE_MAX_SPLIT) split = CLOSE_MAX_SPLIT;
    return split < 1 ? 1 : split;
}
// (the executor and the test hook p3d_block_strided_join; partial: [C][split][3] doubles)
static int32_t launch_strided_join(const float* stage, const float* c, const float* tab, float* g, double* partial, int N, int C, int H, int W, size_t cls_stride, int live,
                                   int split, hipStream_t st) {
    P3D_REQUIRE((int64_t)N * C * H * W < (1ll << 31), "block_strided_join: the tensor exceeds 2^31 elements");
    hipLaunchKernelGGL(block_strided_join_any_kernel, dim3((unsigned)C, (unsigned)split), dim3(256), 0, st, stage, c, tab, g, partial, N, C, H, W, cls_stride, live);
    return check_launch("block_strided_join");
}

// ---- events for the second stream -------------------------------------------------------------------------------------------------------
// (library-global pools are guarded: two host threads may drive two streams through the executor at once -- "thread-safe for distinct streams")
static std::mutex g_events_mu;
static std::vector<hipEvent_t> g_events;
static size_t g_event_next = 0;
static hipEvent_t next_event() {
    std::lock_guard<std::mutex> lock(g_events_mu);
    if (g_events.size() < 128) {
        hipEvent_t e;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
        g_events.push_back(e);
        return e;
    }
    return g_events[g_event_next++ % g_events.size()];          // a recorded event may be re-recorded once the wait on it has been enqueued
}
static bool order_after(hipStream_t waiter, hipStream_t signaller) {
    hipEvent_t e = next_event();
    return e && hipEventRecord(e, signaller) == hipSuccess && hipStreamWaitEvent(waiter, e, 0) == hipSuccess;
}
// the same in two halves: mark the signaller's position now, make the waiter wait for it later (after more work has been queued on the signaller)
static hipEvent_t mark_position(hipStream_t signaller) {
    hipEvent_t e = next_event();
    return (e && hipEventRecord(e, signaller) == hipSuccess) ? e : nullptr;
}

// ---- conv launch profile (bench.py's roofline brackets): HIP events around every conv call of the executor, on the stream it runs on ----------
struct ProfRec { int kind; double flops; hipEvent_t a, b, m; };
static thread_local ProfScope* g_prof_cur = nullptr;
static std::mutex g_prof_mu;
static std::vector<ProfRec> g_prof;
static bool g_prof_on = false;
static bool g_prof_marks = false;       // p3d_profile_enable(2): also note where the conv kernel itself ended (a third event per bracket: ~1 % on the bracketed time)
ProfScope::ProfScope(int kind_, const p3d_conv_desc* d, hipStream_t st_) : st(st_), kind(kind_) {
    flops = 2.0 * d->N * d->K * d->Ho * d->Wo * (double)d->C * d->R * d->S;
    if (g_prof_on && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess) { (void)hipEventRecord(a, st); g_prof_cur = this; }
}
void prof_kernel_done(hipStream_t st) {
    ProfScope* ps = g_prof_cur;
    if (g_prof_marks && ps && ps->a && !ps->m && ps->st == st && hipEventCreate(&ps->m) == hipSuccess) (void)hipEventRecord(ps->m, st);
}
ProfScope::~ProfScope() {
    if (a && b) {
        (void)hipEventRecord(b, st);
        std::lock_guard<std::mutex> lock(g_prof_mu);
        g_prof.push_back({kind, flops, a, b, m});
    }
    if (g_prof_cur == this) g_prof_cur = nullptr;
}

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// a partial convolution inside the executor: the per-pixel factors live in the conv kernels' epilogues (for a split-K launch: in the pass that sums the slabs)
static bool masked_conv_ok(const p3d_conv_desc* d) { return fx_masked_applies(FX_FWD, d) && fx_masked_applies(FX_DGRAD, d); }

// The admission predicate of the executor (b non-null, nconv 2 or 3): 0 = every slot is taken; otherwise *slot is the first one refused, 1 = its shape is outside
// the fused path, 2 = it is a partial convolution outside the masked instances
static int block_refusal_aligned(const p3d_block_desc* b, int* slot) {
    for (int i = 0; i < 4; ++i) {
        if (!block_slot(b, i)) continue;
        *slot = i;
        if (!block_conv_ok(&b->conv[i], i < 3)) return 1;
        if (b->masked && i != 3 && !masked_conv_ok(&b->conv[i])) return 2;
    }
    return 0;
}
// A RAGGED block: a dense block the rule above refuses, under p3d_block_any_enable, whose every convolution (downsample included) block_conv_any_ok takes -- refused for
// its map size only.  Derived from the descriptor wherever it matters (the admission, the image format, the workspace layout, both directions): an aligned block never
// is one, whatever the switch says; masked blocks at odd maps stay refused.  Every slot passes the any-width rule of its stride; a block whose slots all have stride 1
// is taken under p3d_block_any_enable, one that carries a stride-2 slot under p3d_block_any_strided_enable -- each switch admits exactly its own kind.
static bool block_ragged(const p3d_block_desc* b) {
    int slot = 0;
    if (b->masked || block_refusal_aligned(b, &slot) != 1) return false;
    bool strided = false;
    for (int i = 0; i < 4; ++i) {
        if (!block_slot(b, i)) continue;
        const p3d_conv_desc* d = &b->conv[i];
        if (d->stride == 2) strided = true;
        if (!(d->stride == 2 ? block_conv_any_strided_ok(d, i < 3) : block_conv_any_ok(d))) return false;
    }
    return strided ? block_any_strided_enabled() : block_any_enabled();
}
static int block_refusal(const p3d_block_desc* b, int* slot) {
    const int why = block_refusal_aligned(b, slot);
    return why == 1 && block_ragged(b) ? 0 : why;
}
static int32_t check_block(const p3d_block_desc* b) {
    P3D_REQUIRE(b != nullptr, "block: null descriptor");
    P3D_REQUIRE(b->nconv == 2 || b->nconv == 3, "block: nconv must be 2 (BasicBlock) or 3 (Bottleneck), got %d", b->nconv);
    int i = 0;
    const int why = block_refusal(b, &i);
    const p3d_conv_desc* d = &b->conv[i];
    P3D_REQUIRE(why != 1, "block: convolution %d (C=%d K=%d %dx%d stride %d, %dx%d input) is outside the fused path", i, d->C, d->K, d->R, d->S, d->stride, d->H, d->W);
    P3D_REQUIRE(why != 2, "block: partial convolution %d is outside the masked instances of the x3 kernels", i);
    return P3D_OK;
}

// The form of a block's activation images a_i and gradient images d c_i: fp32 row images (4 B per element; the row-fed kernel instances cut the pieces themselves) for
// dense blocks, three bf16 planes (6 B) for masked blocks -- the partial-convolution instances are plane-fed -- and for every block under p3d_fx_tune(6, 1)
// (a ragged block: planes too -- the ragged image-fed instances are plane-fed)
static bool block_row_images(const p3d_block_desc* b) { return !b->masked && fx_block_row_images() && !block_ragged(b); }

// The executor's two workspaces.  main (the launch stream's) = [conv scratch: weight images, split-K slabs | partial sums | the downsample conv's partial sums]: the
// closing conv's and the downsample conv's sums live side by side until the closing pass has read both; side (the weight-gradient stream's) = slabs.
struct BlockLayout { size_t conv_ws, part_bytes, main_bytes, side_bytes; };
static BlockLayout block_layout(const p3d_block_desc* b) {
    size_t mw = 0, sw = 0, part = 0;
    auto atleast = [](size_t& m, size_t v) { if (v > m) m = v; };
    const bool rag = block_ragged(b);          // the ragged plans: slabs on 16-B lines, partial rows = 128-pixel tiles (a launch with sums is never split)
    for (int i = 0; i < 4; ++i) {
        if (!block_slot(b, i)) continue;
        const p3d_conv_desc* d = &b->conv[i];
        atleast(mw, fx_workspace(FX_FWD, d, rag));
        atleast(mw, fx_workspace(FX_DGRAD, d, rag));
        // a stride-2 slot of a ragged block: the class planes of its data gradient live in the conv scratch between the class launches and the pass that finishes
        // them (stream-ordered, like the split-K slabs)
        if (rag && d->stride == 2) atleast(mw, fx_dgrad_strided_any_plan(d).workspace);
        atleast(part, (size_t)fx_partial_rows(FX_FWD, d, rag) * d->K * 2 * sizeof(float));
        atleast(part, (size_t)fx_partial_rows(FX_DGRAD, d, rag) * d->C * 2 * sizeof(float));
        atleast(part, (size_t)(d->K > d->C ? d->K : d->C) * CLOSE_MAX_SPLIT * 3 * sizeof(double));      // the opening pass's and bn_bwd_sums_kernel's fp64 sums
        atleast(sw, fx_workspace(FX_WGRAD, d, rag));
    }
    return BlockLayout{align256(mw), align256(part), align256(mw) + 2 * align256(part), align256(sw)};
}

// the constants of the BatchNorm behind conv `i`, as the finalize steps take them
struct BlockBn { const float *gamma, *beta; float *running_mean, *running_var; float momentum, eps; float *dgamma, *dbeta, *table; };
static BlockBn block_bn(const p3d_block_desc* b, const p3d_block_io* io, int i) {
    return BlockBn{io->gamma[i], io->beta[i], io->running_mean[i], io->running_var[i], b->momentum[i], b->eps[i], io->dgamma[i], io->dbeta[i], io->table[i]};
}

// How a BatchNorm gets from partial sums to its constants, decided here for both directions: with few partial rows (the 32 x 32 and 16 x 16 stages, split-K launches) in
// the prologue of the pass that consumes the constants; with many (layer1: 2048 pixel tiles) every block of that pass would sum all of them again, strided, in front
// of its streaming loop (measured: the closing pass ran at 4.2 TB/s), and a finalize launch of its own costs less (round 4).
// Forward: the CloseFin for the consumer's prologue, or, after a launch of bn_finalize_fwd_kernel, the same with rows = 0: read the table.
static CloseFin finalize_fwd(const BlockBn& bn, const float* partial, int rows, int C, double count, hipStream_t st) {
    if (rows > FX_FIN_MAX_ROWS) {
        hipLaunchKernelGGL(bn_finalize_fwd_kernel, dim3((unsigned)ceil_div(C, FIN_CH)), dim3(fin_threads(rows)), 0, st, partial, rows, C, count, bn.gamma, bn.beta, bn.running_mean,
                           bn.running_var, bn.momentum, bn.eps, bn.table);
        rows = 0;
    }
    return CloseFin{partial, rows, bn.gamma, bn.beta, bn.running_mean, bn.running_var, bn.momentum, bn.eps, bn.table};
}
// the same step as fx_act_image takes it (an inner layer: the consumer is the image pass of a_i)
static FxFinalize act_finalize(const CloseFin& f, double count) {
    FxFinalize fin{};
    fin.kind = 1; fin.partial = f.partial; fin.rows = f.rows; fin.count = count; fin.gamma = f.gamma; fin.beta = f.beta;
    fin.running_mean = f.running_mean; fin.running_var = f.running_var; fin.momentum = f.momentum; fin.eps = f.eps; fin.table = f.table;
    return fin;
}
// Backward: the FxFinalize for the prologue of the image pass of d c (fp64 sums of the opening pass, kind 3, always; fp32 sums of a data gradient's epilogue, kind 2,
// when the rows are few), or, after a launch of bn_finalize_bwd_kernel, one of kind 0: read the table.
static FxFinalize finalize_bwd(const BlockBn& bn, int kind, const void* partial, int rows, int which, int C, double count, int accumulate, hipStream_t st) {
    FxFinalize fin{};
    if (kind == 3 || rows <= FX_FIN_MAX_ROWS) {
        fin.kind = kind; fin.partial = partial; fin.rows = rows; fin.which = which; fin.count = count; fin.gamma = bn.gamma;
        fin.dgamma = bn.dgamma; fin.dbeta = bn.dbeta; fin.accumulate = accumulate; fin.table = bn.table;
    } else {
        hipLaunchKernelGGL(bn_finalize_bwd_kernel<false>, dim3((unsigned)ceil_div(C, FIN_CH)), dim3(fin_threads(rows)), 0, st, partial, rows, C, count, 0, bn.gamma, bn.dgamma,
                           bn.dbeta, accumulate, bn.table);
    }
    return fin;
}

}  // namespace p3d

using namespace p3d;

extern "C" {

int32_t p3d_block_supported(const p3d_block_desc* b) {
    int slot = 0;
    return fx_enabled() && b && (b->nconv == 2 || b->nconv == 3) && block_refusal(b, &slot) == 0 ? 1 : 0;
}

// on = 1 / 0: the executor also takes ragged blocks (block_ragged) / refuses them as ever.  Returns the previous setting.
int32_t p3d_block_any_enable(int32_t on) {
    const int32_t before = block_any_enabled() ? 1 : 0;
    g_block_any = on ? 1 : 0;
    return before;
}

// on = 1 / 0: the executor also takes ragged blocks that carry a stride-2 convolution / refuses them as ever.  Returns the previous setting.
int32_t p3d_block_any_strided_enable(int32_t on) {
    const int32_t before = block_any_strided_enabled() ? 1 : 0;
    g_block_any_strided = on ? 1 : 0;
    return before;
}

// Test hook: block_strided_join_any_kernel alone on given class planes (include/p3d_hip.h)
int32_t p3d_block_strided_join(const float* stage, const float* c, const float* table, float* g, double* partial, int32_t N, int32_t C, int32_t H, int32_t W,
                               size_t cls_stride, int32_t live_mask, int32_t split, void* stream) {
    P3D_REQUIRE(stage && c && table && g && partial && N > 0 && C > 0 && H > 0 && W > 0, "block_strided_join: null tensor or empty shape");
    P3D_REQUIRE(cls_stride >= (size_t)N * C * ((H + 1) / 2) * ((W + 1) / 2) && live_mask >= 0 && live_mask < 16, "block_strided_join: the class planes overlap, or a bad class mask");
    P3D_REQUIRE(split >= 1 && split <= N && split <= CLOSE_MAX_SPLIT, "block_strided_join: split must be in 1 .. min(N, %d)", CLOSE_MAX_SPLIT);
    P3D_REQUIRE((reinterpret_cast<uintptr_t>(partial) & 7) == 0 && ((reinterpret_cast<uintptr_t>(stage) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(g)) & 3) == 0,
                "block_strided_join: misaligned tensor");
    return launch_strided_join(stage, c, table, g, partial, N, C, H, W, cls_stride, live_mask, split, (hipStream_t)stream);
}

// 1: p3d_block_supported admits the block as a ragged one (host-only)
int32_t p3d_block_any_supported(const p3d_block_desc* b) {
    return fx_enabled() && b && (b->nconv == 2 || b->nconv == 3) && block_ragged(b) ? 1 : 0;
}

size_t p3d_block_image_bytes(const p3d_block_desc* b, int32_t N, int32_t C, int32_t HW) {
    if (!b || N <= 0 || C <= 0 || HW <= 0) return 0;
    return block_row_images(b) ? fx_row_image_bytes(N, C, HW) : fx_act_image_bytes(N, C, HW);
}

int32_t p3d_block_workspace_bytes(const p3d_block_desc* b, size_t* main_bytes, size_t* side_bytes) {
    if (int32_t e = check_block(b)) return e;
    const BlockLayout lay = block_layout(b);
    if (main_bytes) *main_bytes = lay.main_bytes;
    if (side_bytes) *side_bytes = lay.side_bytes;
    return P3D_OK;
}

int32_t p3d_block_fwd(const p3d_block_desc* b, const p3d_block_io* io, void* workspace, size_t workspace_bytes, void* stream) {
    if (int32_t e = check_block(b)) return e;
    P3D_REQUIRE(io && io->x && io->out, "block_fwd: null tensor");
    const BlockLayout lay = block_layout(b);
    if (!workspace || workspace_bytes < lay.main_bytes) { set_error("block_fwd: workspace %zu B < required %zu B", workspace_bytes, lay.main_bytes); return P3D_EWORKSPACE; }
    hipStream_t st = (hipStream_t)stream;
    float* partial = (float*)((char*)workspace + lay.conv_ws);
    float* partial2 = (float*)((char*)partial + lay.part_bytes);      // the downsample conv's partial sums
    const int last = b->nconv - 1;
    const bool rows = block_row_images(b);
    // a ragged block: every convolution image-fed on the ragged instances (STATS epilogue); the block input as a plane image of its own, written once here and kept
    // in aimg[3] for the weight gradients of conv 0 and of the downsample conv
    const bool rag = block_ragged(b);
    if (rag) {
        P3D_REQUIRE(io->aimg[3], "block_fwd: null image of the block input (aimg[3]: a block at a map width outside the aligned kernels)");
        if (int32_t e = fx_act_image_any(io->x, io->aimg[3], b->conv[0].N, b->conv[0].C, b->conv[0].H * b->conv[0].W, st)) return e;
    }
    for (int i = 0; i < 4; ++i) {
        const bool ds = i == 3;
        if (!block_slot(b, i)) continue;
        const p3d_conv_desc* d = &b->conv[i];
        P3D_REQUIRE(io->w[i] && io->c[i] && io->table[i] && io->gamma[i] && io->beta[i], "block_fwd: null tensor of conv %d", i);
        const bool from_x = ds || i == 0;          // the block input arrives as fp32 (split in the kernel); everything produced inside the block as an image
        if (!from_x) P3D_REQUIRE(io->aimg[i - 1], "block_fwd: null activation image %d", i - 1);
        FxFuse f{};
        f.act_img = from_x ? (rag ? io->aimg[3] : nullptr) : io->aimg[i - 1];
        f.rows = !from_x && rows;
        f.ragged = rag;
        f.partial = ds ? partial2 : partial;
        f.wimg = io->wimg[i];
        const bool mk = b->masked && !ds;
        if (mk) {
            P3D_REQUIRE(io->pix_in[i] && io->pix_out[i], "block_fwd: null per-pixel factor of partial convolution %d", i);
            f.emask = io->pix_out[i];
            if (from_x) f.pmask = io->pix_in[i];           // (an image operand carries mask_in already: the pass that wrote a_{i-1} multiplied it in)
        }
        {
            ProfScope ps(0, d, st);
            fx_count(0, d);
            if (int32_t e = fx_conv_fwd(d, from_x ? io->x : nullptr, io->w[i], nullptr, io->c[i], workspace, lay.conv_ws, &f, st)) return e;
        }
        if (ds || i == last) continue;               // the closing pass finalizes these two BatchNorm layers itself
        // a_i = relu(bn_i(c_i)), written once, as the image the next convolution (and, in backward, its weight gradient) copies into LDS
        P3D_REQUIRE(io->aimg[i], "block_fwd: null activation image %d", i);
        const double cnt = (double)d->N * d->Ho * d->Wo;
        const CloseFin cf = finalize_fwd(block_bn(b, io, i), partial, fx_partial_rows(FX_FWD, d, rag), d->K, cnt, st);
        const FxFinalize fin = act_finalize(cf, cnt);
        if (rag) {
            if (int32_t e = fx_act_image_any_map(1, io->c[i], nullptr, io->table[i], 0, io->aimg[i], d->N, d->K, d->Ho * d->Wo, st, cf.rows ? &fin : nullptr)) return e;
            continue;
        }
        if (int32_t e = fx_act_image(1, io->c[i], nullptr, io->table[i], 0, io->aimg[i], d->N, d->K, d->Ho * d->Wo, st, cf.rows ? &fin : nullptr, mk ? io->pix_in[i + 1] : nullptr, rows)) return e;
    }
    const p3d_conv_desc* dl = &b->conv[last];
    const int HW = dl->Ho * dl->Wo;
    const double cnt_close = (double)dl->N * HW;
    const CloseFin cf = finalize_fwd(block_bn(b, io, last), partial, fx_partial_rows(FX_FWD, dl, rag), dl->K, cnt_close, st);
    const CloseFin rf = b->has_downsample ? finalize_fwd(block_bn(b, io, 3), partial2, fx_partial_rows(FX_FWD, &b->conv[3], rag), dl->K, cnt_close, st) : CloseFin{};
    if (rag) {
        hipLaunchKernelGGL(block_close_fwd_any_kernel, dim3(dl->K, close_split(dl->N, dl->K)), dim3(256), 0, st, (const float*)io->c[last], cf,
                           b->has_downsample ? (const float*)io->c[3] : io->x, rf, io->out, dl->N, dl->K, HW, b->relu_out, cnt_close);
        return check_launch("block_fwd");
    }
    hipLaunchKernelGGL(block_close_fwd_kernel, dim3(dl->K, close_split(dl->N, dl->K)), dim3(256), 0, st, (const float*)io->c[last], cf,
                       b->has_downsample ? (const float*)io->c[3] : io->x, rf, io->out, b->relu_out ? io->out_mask : (unsigned char*)nullptr, dl->N, dl->K, HW, b->relu_out, cnt_close);
    return check_launch("block_fwd");
}

// ---- backward: four stages over one context ------------------------------------------------------------------------------------------------------
// Streams: a weight gradient runs on the second stream behind an event of the launch stream; it reads dcimg[i] and aimg[i - 1] / x, none of which the launch
// stream writes again inside this call, so the launch stream never waits for the second one here.
struct BwdCtx {
    const p3d_block_desc* b;
    const p3d_block_io* io;
    void* ws; size_t conv_ws;       // the launch stream's workspace: conv scratch
    void* partial;                  //   and the partial sums behind it
    float* side_ws;                 // the weight-gradient stream's slabs
    size_t side_bytes;
    hipStream_t st, ss;
    bool two;                       // ss is a stream of its own
    bool rows;                      // aimg / dcimg are fp32 row images (block_row_images)
    bool rag;                       // a ragged block (block_ragged): plane images, the ragged instances, the passes for any HW; no mask bytes, g always in memory
    int acc, last;
    // g = dout * [out > 0] never exists as a tensor when forward left mask bytes: the two opening image passes mask dout themselves, and with an identity
    // shortcut the first convolution's data gradient adds the masked dout in its epilogue (dx = dgrad + dout * mask) instead of accumulating into a copy of g
    bool g_in_memory;
    const float* g;                 // the gradient behind the closing ReLU: gbuf, or dout to be masked by
    const unsigned char* gmask;     //   these bytes (null: g is masked already)
};

// partial convolutions: the gradient image of conv `slot` carries its renormalisation factor (d raw = d c * mult: partial_conv.py:53 and its autograd)
static const float* bwd_pixmul(const BwdCtx& x, int slot) { return (x.b->masked && slot != 3) ? x.io->pix_out[slot] : nullptr; }

// The gradient that enters conv `slot` is the upstream gradient taken through its BatchNorm's backward map (masked by its ReLU, except the closing BN whose ReLU
// went into g already): d c = A g + B c + K, written ONCE, as the image both the weight gradient and the data gradient of the conv copy into LDS.  The constants
// come from channel sums (the opening pass's for the closing and the downsample BatchNorm, the downstream data gradient's epilogue for the others): finalize_bwd.
static int32_t bwd_map(const BwdCtx& x, const float* gin, int slot, int masked, int kind, int rows, int which, double cnt, const unsigned char* front_mask = nullptr) {
    const p3d_block_io* io = x.io;
    const p3d_conv_desc* dc = &x.b->conv[slot];
    P3D_REQUIRE(io->dcimg[slot], "block_bwd: null gradient image %d", slot);
    FxFinalize fin = finalize_bwd(block_bn(x.b, io, slot), kind, x.partial, rows, which, dc->K, cnt, x.acc, x.st);
    fin.gmask = front_mask;
    if (x.rag) return fx_act_image_any_map(2, gin, io->c[slot], io->table[slot], masked, io->dcimg[slot], dc->N, dc->K, dc->Ho * dc->Wo, x.st, fin.kind ? &fin : nullptr);
    return fx_act_image(2, gin, io->c[slot], io->table[slot], masked, io->dcimg[slot], dc->N, dc->K, dc->Ho * dc->Wo, x.st, fin.kind ? &fin : nullptr, bwd_pixmul(x, slot), x.rows);
}

// `ready`: the launch stream's position when the gradient image of this convolution was complete (the data gradient of the same layer has been queued on
// the launch stream since: it is the critical path and gets to the GPU first; the weight gradient only feeds the optimizer)
static int32_t launch_wgrad(const BwdCtx& x, int slot, const float* xin, const void* ximg, hipEvent_t ready) {
    const p3d_conv_desc* d = &x.b->conv[slot];
    if (x.two && (!ready || hipStreamWaitEvent(x.ss, ready, 0) != hipSuccess)) { set_error("block_bwd: event failure"); return P3D_ELAUNCH; }
    ProfScope ps(2, d, x.ss);
    fx_count(2, d);
    FxFuse fw{};
    fw.dy_img = x.io->dcimg[slot]; fw.x_img = ximg; fw.rows = x.rows; fw.ragged = x.rag;
    if (x.b->masked && slot != 3 && !ximg) fw.emask = x.io->pix_in[slot];      // the block input is fp32: x * mask_in in the kernel's split (an image carries it)
    return fx_conv_wgrad(d, nullptr, xin, x.io->dw[slot], x.acc, x.side_ws, x.side_bytes, &fw, "block_bwd", x.ss);
}

static int32_t bwd_dgrad(const BwdCtx& x, int slot, const p3d_conv_desc* dd, float* dx, const FxFuse* f) {
    ProfScope ps(1, &x.b->conv[slot], x.st);
    fx_count(1, &x.b->conv[slot]);
    return fx_conv_dgrad(dd, nullptr, x.io->w[slot], dx, x.ws, x.conv_ws, f, x.st);
}

// The data gradient of a stride-2 slot of a ragged block (p3d_block_any_strided_enable): the class launches, image-fed from dcimg[slot] with the cached wimgT[slot], into
// tight class planes in the conv scratch, then the pass that finishes them on the same stream -- join_c set (a main-chain slot i >= 1): block_strided_join_any_kernel
// writes dx = da[i - 1] and the BatchNorm-backward sums of the layer in front (its raw output join_c, its table join_tab) into x.partial as [C][join_split][3]
// doubles; otherwise (conv 0 of a BasicBlock, the downsample conv: no sums to take) the interleave, which writes the zeros of the classes no tap reaches and adds
// onto dx under `accumulate`.
static int32_t bwd_dgrad_strided(const BwdCtx& x, int slot, float* dx, int accumulate, const float* join_c, const float* join_tab, int join_split) {
    const p3d_conv_desc* d = &x.b->conv[slot];
    ProfScope ps(1, d, x.st);
    fx_count(1, d);
    const FxStridedPlan pl = fx_dgrad_strided_any_plan(d);
    int live = 0;
    if (int32_t e = fx_conv_dgrad_strided_any(d, nullptr, x.io->w[slot], x.ws, x.conv_ws, &live, x.st, x.io->dcimg[slot], x.io->wimgT[slot], join_c != nullptr)) return e;
    const float* stage = (const float*)((const char*)x.ws + pl.stage_offset);
    if (join_c) return launch_strided_join(stage, join_c, join_tab, dx, (double*)x.partial, d->N, d->C, d->H, d->W, pl.cls_stride, live, join_split, x.st);
    return fx_dgrad_interleave_rows(stage, dx, nullptr, d->N, d->C, d->H, d->W, pl.cls_stride, live, accumulate, x.st);
}

// 1. open: g = dout * [out > 0]; channel sums of the closing BN (and of the downsample BN)
static int32_t bwd_open(const BwdCtx& x) {
    const p3d_block_desc* b = x.b;
    const p3d_block_io* io = x.io;
    const p3d_conv_desc* dl = &b->conv[x.last];
    if (x.rag) {
        hipLaunchKernelGGL(block_open_bwd_any_kernel, dim3(dl->K, close_split(dl->N, dl->K)), dim3(256), 0, x.st, io->dout, (const float*)io->out, (const float*)io->c[x.last],
                           (const float*)io->table[x.last], b->has_downsample ? (const float*)io->c[3] : (const float*)nullptr,
                           b->has_downsample ? (const float*)io->table[3] : (const float*)nullptr, io->gbuf, (double*)x.partial, dl->N, dl->K, dl->Ho * dl->Wo, b->relu_out);
        return check_launch("block_bwd open");
    }
    hipLaunchKernelGGL(block_open_bwd_kernel, dim3(dl->K, close_split(dl->N, dl->K)), dim3(256), 0, x.st, io->dout, (const float*)io->out, (const float*)io->c[x.last],
                       (const float*)io->table[x.last], b->has_downsample ? (const float*)io->c[3] : (const float*)nullptr,
                       b->has_downsample ? (const float*)io->table[3] : (const float*)nullptr, x.g_in_memory ? io->gbuf : (float*)nullptr, (double*)x.partial,
                       (const unsigned char*)io->out_mask, dl->N, dl->K, dl->Ho * dl->Wo, b->relu_out);
    return check_launch("block_bwd open");
}

// 2. the two maps fed by the opening pass's sums (its partial buffer is overwritten by the first data gradient of the chain): closing BatchNorm, downsample BatchNorm
static int32_t bwd_open_images(const BwdCtx& x) {
    const p3d_block_desc* b = x.b;
    const p3d_block_io* io = x.io;
    const int last = x.last;
    const p3d_conv_desc* dl = &b->conv[last];
    const int split = close_split(dl->N, dl->K);
    const double cnt = (double)dl->N * dl->Ho * dl->Wo;
    for (int i = 0; b->masked && i < b->nconv; ++i) P3D_REQUIRE(io->pix_in[i] && io->pix_out[i], "block_bwd: null per-pixel factor of partial convolution %d", i);
    if (b->has_downsample && fx_pair_map_enabled() && !x.rag) {             // (the pair pass is aligned-only: a ragged block takes the two passes below)
        // both images in one pass: g (dout and the mask bytes) is read once
        P3D_REQUIRE(io->dcimg[last] && io->dcimg[3], "block_bwd: null gradient image");
        const FxFinalize fa = finalize_bwd(block_bn(b, io, last), 3, x.partial, split, 0, dl->K, cnt, x.acc, x.st);
        const FxFinalize fb = finalize_bwd(block_bn(b, io, 3), 3, x.partial, split, 1, dl->K, cnt, x.acc, x.st);
        return fx_act_image_pair(x.g, x.gmask, io->c[last], io->c[3], io->dcimg[last], io->dcimg[3], &fa, &fb, dl->N, dl->K, dl->Ho * dl->Wo, x.st, bwd_pixmul(x, last), x.rows);
    }
    if (int32_t e = bwd_map(x, x.g, last, 0, 3, split, 0, cnt, x.gmask)) return e;
    return b->has_downsample ? bwd_map(x, x.g, 3, 0, 3, split, 1, cnt, x.gmask) : P3D_OK;
}

// 3. the main chain, last convolution first.  Per layer the data gradient first (the chain the next layer waits for), then the weight gradient of the same layer on
//    the second stream, then the image of d c_{i-1}.  `ready`: the launch stream's position when d c_last was complete.
static int32_t bwd_chain(const BwdCtx& x, hipEvent_t ready) {
    const p3d_block_desc* b = x.b;
    const p3d_block_io* io = x.io;
    for (int i = x.last; i >= 0; --i) {
        const p3d_conv_desc* d = &b->conv[i];
        if (i > 0) P3D_REQUIRE(io->aimg[i - 1], "block_bwd: null activation image %d", i - 1);
        FxFuse f{};
        f.wimg = io->wimgT[i];
        f.act_img = io->dcimg[i]; f.rows = x.rows; f.ragged = x.rag;
        p3d_conv_desc dd = *d;
        if (i > 0) {
            const p3d_conv_desc* dp = &b->conv[i - 1];                       // producer of this conv's input
            const bool epi = d->stride == 1;
            if (epi) { f.partial = (float*)x.partial; f.ep_c = io->c[i - 1]; f.ep_tab = io->table[i - 1]; }
            if (b->masked) f.emask = io->pix_in[i];            // dx = dgrad(d raw) * mask_in: the gradient w.r.t. a_{i-1}, of which the BatchNorm-backward sums are taken
            dd.accumulate = 0;
            P3D_REQUIRE(io->da[i - 1], "block_bwd: null gradient buffer %d", i - 1);
            const double cnt = (double)dp->N * dp->Ho * dp->Wo;
            if (x.rag && !epi) {
                // a ragged block's strided data gradient: class launches, then one pass that writes da[i - 1] and takes the sums (bwd_dgrad_strided)
                const int sp = close_split(dp->N, dp->K);
                if (int32_t e = bwd_dgrad_strided(x, i, io->da[i - 1], 0, (const float*)io->c[i - 1], (const float*)io->table[i - 1], sp)) return e;
                if (int32_t e = launch_wgrad(x, i, nullptr, io->aimg[i - 1], ready)) return e;
                if (int32_t e = bwd_map(x, io->da[i - 1], i - 1, 1, 3, sp, 0, cnt)) return e;
                ready = x.two ? mark_position(x.st) : nullptr;
                continue;
            }
            if (int32_t e = bwd_dgrad(x, i, &dd, io->da[i - 1], &f)) return e;
            if (int32_t e = launch_wgrad(x, i, nullptr, io->aimg[i - 1], ready)) return e;
            if (epi) {
                if (int32_t e = bwd_map(x, io->da[i - 1], i - 1, 1, 2, fx_partial_rows(FX_DGRAD, d, x.rag), 0, cnt)) return e;
            } else {
                // a strided data gradient takes no sums in its epilogue: a pass of their own
                const int sp = close_split(dp->N, dp->K);
                hipLaunchKernelGGL(bn_bwd_sums_kernel, dim3(dp->K, sp), dim3(256), 0, x.st, (const float*)io->da[i - 1], (const float*)io->c[i - 1],
                                   (const float*)io->table[i - 1], (double*)x.partial, dp->N, dp->K, dp->Ho * dp->Wo);
                if (int32_t e = bwd_map(x, io->da[i - 1], i - 1, 1, 3, sp, 0, cnt)) return e;
            }
            ready = x.two ? mark_position(x.st) : nullptr;                  // d c_{i-1} is complete
            continue;
        }
        if (b->need_dx) {
            // block input: identity shortcut -> the gradient joins g's own buffer in place (dx = g + dgrad); downsample shortcut -> dx is written here and
            // the downsample conv's dgrad adds to it in the last stage.  No weight-gradient kernel reads g (they read the images), so the launch stream does not wait.
            float* dx;
            if (b->masked) f.emask = io->pix_in[0];
            if (b->has_downsample) { dx = io->dx; dd.accumulate = 0; }
            else {
                P3D_REQUIRE(b->relu_out, "block_bwd: an identity shortcut without the closing ReLU would overwrite the caller's gradient (not a reference block)");
                P3D_REQUIRE(io->gbuf, "block_bwd: null gradient buffer (dx of an identity shortcut)");
                dx = io->gbuf; dd.accumulate = 1;
                if (!x.g_in_memory) { f.acc_src = io->dout; f.acc_mask = io->out_mask; }      // gbuf is written here for the first time
            }
            if (x.rag && d->stride == 2) {              // (a BasicBlock's strided conv 0: no BatchNorm in front of it, the interleave finishes the classes)
                if (int32_t e = bwd_dgrad_strided(x, 0, dx, dd.accumulate, nullptr, nullptr, 0)) return e;
            } else if (int32_t e = bwd_dgrad(x, 0, &dd, dx, &f)) return e;
        }
        if (int32_t e = launch_wgrad(x, 0, io->x, x.rag ? io->aimg[3] : nullptr, ready)) return e;      // (ragged: against the image of x kept from forward)
    }
    return P3D_OK;
}

// 4. downsample branch: data gradient added onto dx, weight gradient (its gradient image was written with the closing BatchNorm's: `ready` is the chain's first event)
static int32_t bwd_downsample(const BwdCtx& x, hipEvent_t ready) {
    if (x.b->need_dx && x.rag && x.b->conv[3].stride == 2) {
        // the strided 1x1 of a ragged block: class (0, 0) alone is live; the interleave adds its plane onto dx and leaves the other pixels as they are
        if (int32_t e = bwd_dgrad_strided(x, 3, x.io->dx, 1, nullptr, nullptr, 0)) return e;
    } else if (x.b->need_dx) {
        FxFuse f{};
        f.wimg = x.io->wimgT[3];
        f.act_img = x.io->dcimg[3]; f.rows = x.rows; f.ragged = x.rag;
        p3d_conv_desc dd = x.b->conv[3];
        dd.accumulate = 1;
        if (int32_t e = bwd_dgrad(x, 3, &dd, x.io->dx, &f)) return e;
    }
    return launch_wgrad(x, 3, x.io->x, x.rag ? x.io->aimg[3] : nullptr, ready);
}

// dout -> dx (+ every parameter gradient, accumulated into io->dw / dgamma / dbeta when b->accumulate_grads, else written).
// side_stream may be null (everything on `stream`); otherwise the weight-gradient kernels run there, ordered by events behind the kernels that produce
// their operands; the caller joins the two streams before it reads the gradients.
int32_t p3d_block_bwd(const p3d_block_desc* b, const p3d_block_io* io, void* workspace, size_t workspace_bytes, void* side_workspace, size_t side_bytes,
                      void* stream, void* side_stream) {
    static_assert(sizeof(p3d_block_io) == 592, "74 pointers (ops_block.BlockIO mirrors the struct)");
    if (int32_t e = check_block(b)) return e;
    P3D_REQUIRE(io && io->x && io->out && io->dout, "block_bwd: null tensor");
    BwdCtx x{};
    x.b = b; x.io = io;
    x.rag = block_ragged(b);
    P3D_REQUIRE(!x.rag || io->aimg[3], "block_bwd: null image of the block input (aimg[3])");
    x.g_in_memory = x.rag || !(b->relu_out && io->out_mask && (b->has_downsample || !b->need_dx || fx_dgrad_accumulates_from_source(&b->conv[0])));
    P3D_REQUIRE(!x.g_in_memory || !b->relu_out || io->gbuf, "block_bwd: null gradient buffer");
    const BlockLayout lay = block_layout(b);
    if (!workspace || workspace_bytes < lay.main_bytes || !side_workspace || side_bytes < lay.side_bytes) {
        set_error("block_bwd: workspaces %zu / %zu B < required %zu / %zu B", workspace_bytes, side_bytes, lay.main_bytes, lay.side_bytes);
        return P3D_EWORKSPACE;
    }
    x.ws = workspace; x.conv_ws = lay.conv_ws; x.partial = (char*)workspace + lay.conv_ws; x.side_ws = (float*)side_workspace; x.side_bytes = side_bytes;
    x.st = (hipStream_t)stream; x.ss = side_stream ? (hipStream_t)side_stream : x.st;
    x.two = x.ss != x.st;
    x.acc = b->accumulate_grads; x.last = b->nconv - 1; x.rows = block_row_images(b);
    x.g = (b->relu_out && x.g_in_memory) ? io->gbuf : io->dout;
    x.gmask = x.g_in_memory ? nullptr : io->out_mask;          // (a ragged block has no mask bytes: io->out_mask is not looked at)

    if (int32_t e = bwd_open(x)) return e;
    if (int32_t e = bwd_open_images(x)) return e;
    const hipEvent_t ready = x.two ? mark_position(x.st) : nullptr;       // d c_last (and the downsample branch's gradient image) are complete
    if (int32_t e = bwd_chain(x, ready)) return e;
    if (b->has_downsample)
        if (int32_t e = bwd_downsample(x, ready)) return e;
    return check_launch("block_bwd");
}

// ---- the same block on the fp16 NHWC kernels (-half_acc): host-side fusion of the per-layer entry points into one call per block and direction -------------------
// BatchNorm sums in the conv epilogues (p3d_hconv2d_fwd_stats / p3d_hconv2d_dgrad_sums); p3d_hblock_fuse_sums(0): the stand-alone statistics / reduce passes (the
// configuration in which the executor is bit-identical to the per-layer path)
static int g_hblock_fused = 1;
static bool hblock_fused() { return g_hblock_fused != 0; }
// main workspace of a layer: [the partial table: max(512 stand-alone blocks, pixel tiles of either pass) rows][K float4 of constants]
static size_t hblock_rows(const p3d_conv_desc* d) {
    const int r0 = p3d_hconv2d_sum_rows(d, 0), r1 = p3d_hconv2d_sum_rows(d, 1);
    const int r = r0 > r1 ? r0 : r1;
    return (size_t)(r > 512 ? r : 512);
}

/* on = 1 / 0: BatchNorm sums from the conv epilogues / from stand-alone passes (the latter is bit-identical to the per-layer path); on < 0: query.  Returns the previous setting. */
int32_t p3d_hblock_fuse_sums(int32_t on) {
    const int32_t before = g_hblock_fused;
    if (on >= 0) g_hblock_fused = on ? 1 : 0;
    return before;
}

int32_t p3d_hblock_workspace_bytes(const p3d_block_desc* b, size_t* main_bytes, size_t* side_bytes) {
    P3D_REQUIRE(b && (b->nconv == 2 || b->nconv == 3), "hblock: nconv must be 2 or 3");
    size_t mw = 0, sw = 0;
    for (int i = 0; i < 4; ++i) {
        if (!block_slot(b, i)) continue;
        const int kc = b->conv[i].K > b->conv[i].C ? b->conv[i].K : b->conv[i].C;
        const size_t a = hblock_rows(&b->conv[i]) * kc * 2 * sizeof(float) + (size_t)kc * 4 * sizeof(float), w = p3d_hconv2d_wgrad_workspace_bytes(&b->conv[i]);
        if (a > mw) mw = a;
        if (w > sw) sw = w;
    }
    if (main_bytes) *main_bytes = align256(mw);
    if (side_bytes) *side_bytes = align256(sw);
    return P3D_OK;
}

int32_t p3d_hblock_fwd(const p3d_block_desc* b, const p3d_hblock_io* io, void* workspace, size_t workspace_bytes, void* stream) {
    P3D_REQUIRE(b && io && io->x && io->out && (b->nconv == 2 || b->nconv == 3), "hblock_fwd: bad argument");
    const int last = b->nconv - 1;
    for (int i = 0; i < 4; ++i)
        if (block_slot(b, i)) P3D_REQUIRE(io->w_krsc[i] && io->c[i] && io->coef[i] && io->gamma[i] && io->beta[i] && (i == last || io->a[i]), "hblock_fwd: null tensor of conv %d", i);
    hipStream_t st = (hipStream_t)stream;
    const bool fused = hblock_fused();
    {
        size_t need = 0;
        if (int32_t e = p3d_hblock_workspace_bytes(b, &need, nullptr)) return e;
        if (!workspace || workspace_bytes < need) { set_error("hblock_fwd: workspace %zu B < required %zu B", workspace_bytes, need); return P3D_EWORKSPACE; }
    }
    auto conv = [&](int i, const void* in) -> int32_t {
        const p3d_conv_desc* d = &b->conv[i];
        ProfScope ps(0, d, st);
        if (fused) return p3d_hconv2d_fwd_stats(d, in, io->w_krsc[i], io->c[i], (float*)workspace, stream);       // (the table is consumed by bn(i) before the next conv runs)
        return p3d_hconv2d_fwd(d, in, io->w_krsc[i], nullptr, nullptr, nullptr, io->c[i], stream);
    };
    auto bn = [&](int i, const void* res, void* y, int relu) -> int32_t {
        const p3d_conv_desc* d = &b->conv[i];
        if (fused)
            return p3d_hbn_train_fwd_partial(io->c[i], res, io->gamma[i], io->beta[i], io->running_mean[i], io->running_var[i], y, io->coef[i], d->N * d->Ho * d->Wo, d->K,
                                             b->momentum[i], b->eps[i], relu, (const float*)workspace, p3d_hconv2d_sum_rows(d, 0),
                                             (i == last && res) ? (uint8_t*)io->out_mask : nullptr, stream);
        return p3d_hbn_train_fwd(io->c[i], res, io->gamma[i], io->beta[i], io->running_mean[i], io->running_var[i], y, io->coef[i], d->N * d->Ho * d->Wo, d->K,
                                 b->momentum[i], b->eps[i], relu, workspace, workspace_bytes, stream);
    };
    if (b->has_downsample) {
        if (int32_t e = conv(3, io->x)) return e;
        if (int32_t e = bn(3, nullptr, io->a[3], 0)) return e;
    }
    const void* in = io->x;
    for (int i = 0; i <= last; ++i) {
        if (int32_t e = conv(i, in)) return e;
        if (i < last) { if (int32_t e = bn(i, nullptr, io->a[i], 1)) return e; in = io->a[i]; }
        else if (int32_t e = bn(i, b->has_downsample ? (const void*)io->a[3] : io->x, io->out, b->relu_out)) return e;
    }
    return P3D_OK;
}

int32_t p3d_hblock_bwd(const p3d_block_desc* b, const p3d_hblock_io* io, void* workspace, size_t workspace_bytes, void* side_workspace, size_t side_bytes,
                       void* stream, void* side_stream) {
    P3D_REQUIRE(b && io && io->x && io->out && io->dout && (b->nconv == 2 || b->nconv == 3), "hblock_bwd: bad argument");
    P3D_REQUIRE(b->relu_out, "hblock_bwd: blocks without the closing ReLU stay on the per-layer path");
    const int last = b->nconv - 1;
    for (int i = 0; i < 4; ++i)
        if (block_slot(b, i)) P3D_REQUIRE(io->c[i] && io->coef[i] && io->dc[i] && io->dw[i] && io->dgamma[i] && io->dbeta[i] && (i == 0 || i == 3 || io->w_crsk[i]) && (i == last || i == 3 || io->da[i]),
                                           "hblock_bwd: null tensor of conv %d", i);
    P3D_REQUIRE(io->da[3] && (!b->need_dx || !b->has_downsample || (io->dx && io->w_crsk[0] && io->w_crsk[3])) && (!b->need_dx || b->has_downsample || io->w_crsk[0]), "hblock_bwd: null gradient buffer");
    hipStream_t st = (hipStream_t)stream, ss = side_stream ? (hipStream_t)side_stream : st;
    const bool two = ss != st;
    const int acc = b->accumulate_grads;
    auto bn_bwd = [&](int i, const void* dy, const void* y, void* dres, int relu) -> int32_t {
        const p3d_conv_desc* d = &b->conv[i];
        return p3d_hbn_train_bwd(dy, io->c[i], y, io->coef[i], io->dc[i], dres, io->dgamma[i], io->dbeta[i], d->N * d->Ho * d->Wo, d->K, relu, acc, workspace, workspace_bytes, stream);
    };
    auto wgrad = [&](int i, const void* xin, hipEvent_t ready) -> int32_t {        // `ready`: the launch stream's position when dc[i] was complete
        p3d_conv_desc d = b->conv[i];
        d.accumulate = acc;
        if (two && (!ready || hipStreamWaitEvent(ss, ready, 0) != hipSuccess)) { set_error("hblock_bwd: event failure"); return P3D_ELAUNCH; }
        ProfScope ps(2, &d, ss);
        return p3d_hconv2d_wgrad(&d, io->dc[i], xin, nullptr, io->dw[i], io->c_real[i], 1.0f, two ? side_workspace : side_workspace, side_bytes, (void*)ss);
    };
    {
        size_t need = 0;
        if (int32_t e = p3d_hblock_workspace_bytes(b, &need, nullptr)) return e;
        if (!workspace || workspace_bytes < need) { set_error("hblock_bwd: workspace %zu B < required %zu B", workspace_bytes, need); return P3D_EWORKSPACE; }
    }
    auto dgrad = [&](int i, void* dx, int accumulate) -> int32_t {
        p3d_conv_desc d = b->conv[i];
        d.accumulate = accumulate;
        ProfScope ps(1, &d, st);
        return p3d_hconv2d_dgrad(&d, io->dc[i], io->w_crsk[i], nullptr, dx, stream);
    };
    // the data gradient of conv i (i > 0, stride 1) also takes the sums of the BatchNorm + ReLU in front of it; bn_bwd_fused(i - 1) then only finalizes and applies
    auto fusable = [&](int i) { return hblock_fused() && i > 0 && b->conv[i].stride == 1; };
    auto dgrad_sums = [&](int i) -> int32_t {
        p3d_conv_desc d = b->conv[i];
        d.accumulate = 0;
        ProfScope ps(1, &d, st);
        return p3d_hconv2d_dgrad_sums(&d, io->dc[i], io->w_crsk[i], io->da[i - 1], io->c[i - 1], io->coef[i - 1], (float*)workspace, stream);
    };
    auto bn_bwd_fused = [&](int j, int rows) -> int32_t {
        const p3d_conv_desc* d = &b->conv[j];
        float* coef2 = (float*)((char*)workspace + hblock_rows(&b->conv[j + 1]) * d->K * 2 * sizeof(float));
        return p3d_hbn_train_bwd_partial(io->da[j], io->c[j], io->coef[j], io->dc[j], io->dgamma[j], io->dbeta[j], d->N * d->Ho * d->Wo, d->K, acc, (const float*)workspace, rows,
                                         coef2, stream);
    };
    // closing BatchNorm: d c_last, and the gradient that enters the shortcut (dout masked by the block's output, or by the mask bytes forward left of it)
    if (hblock_fused() && io->out_mask) {
        const p3d_conv_desc* d = &b->conv[last];
        if (int32_t e = p3d_hbn_train_bwd_mask(io->dout, io->c[last], (const uint8_t*)io->out_mask, io->coef[last], io->dc[last], io->da[3], io->dgamma[last], io->dbeta[last],
                                               d->N * d->Ho * d->Wo, d->K, acc, workspace, workspace_bytes, stream)) return e;
    } else if (int32_t e = bn_bwd(last, io->dout, io->out, io->da[3], 1)) return e;
    hipEvent_t ready = two ? mark_position(st) : nullptr;
    // the downsample branch first (the order autograd runs the per-layer nodes in: dx = branch's data gradient, then the first conv's added onto it);
    // per layer the data gradient is queued before the weight gradient: it is the chain the next layer waits for
    if (b->has_downsample) {
        if (int32_t e = bn_bwd(3, io->da[3], nullptr, nullptr, 0)) return e;
        const hipEvent_t ready_ds = two ? mark_position(st) : nullptr;
        if (b->need_dx)
            if (int32_t e = dgrad(3, io->dx, 0)) return e;
        if (int32_t e = wgrad(3, io->x, ready_ds)) return e;
    }
    for (int i = last; i >= 0; --i) {
        if (i > 0) {
            if (fusable(i)) {
                if (int32_t e = dgrad_sums(i)) return e;
                if (int32_t e = wgrad(i, io->a[i - 1], ready)) return e;
                if (int32_t e = bn_bwd_fused(i - 1, p3d_hconv2d_sum_rows(&b->conv[i], 1))) return e;
            } else {
                if (int32_t e = dgrad(i, io->da[i - 1], 0)) return e;
                if (int32_t e = wgrad(i, io->a[i - 1], ready)) return e;
                if (int32_t e = bn_bwd(i - 1, io->da[i - 1], nullptr, nullptr, 1)) return e;
            }
            ready = two ? mark_position(st) : nullptr;
        } else {
            // the first conv's data gradient joins what the shortcut already delivered: the branch's data gradient (dx), or with an identity shortcut da[3] itself
            if (b->need_dx)
                if (int32_t e = dgrad(0, b->has_downsample ? io->dx : io->da[3], 1)) return e;
            if (int32_t e = wgrad(0, io->x, ready)) return e;
        }
    }
    return P3D_OK;
}

// Pre-split weight images (csrc/p3d_fx.hip): three bf16 pieces of every weight, laid out as the conv kernels' LDS tiles, one image for the forward pass
// (rows = output channels) and one for the data gradient (rows = input channels).  Rebuilt by the caller whenever the weight changes.
int32_t p3d_fx_weight_image_bytes(int32_t K, int32_t C, int32_t RS, size_t* fwd_bytes, size_t* bwd_bytes) {
    P3D_REQUIRE(K > 0 && C > 0 && RS > 0 && C % 16 == 0 && K % 16 == 0, "weight_image_bytes: channel counts must be positive multiples of 16 (K=%d C=%d)", K, C);
    if (fwd_bytes) *fwd_bytes = fx_weight_image_bytes(K, C, RS, false);
    if (bwd_bytes) *bwd_bytes = fx_weight_image_bytes(K, C, RS, true);
    return P3D_OK;
}

int32_t p3d_fx_weight_images(const float* w, int32_t K, int32_t C, int32_t RS, void* img_fwd, void* img_bwd, void* stream) {
    P3D_REQUIRE(w && img_fwd && img_bwd && K > 0 && C > 0 && RS > 0 && C % 16 == 0 && K % 16 == 0, "weight_images: bad argument");
    return fx_build_weight_images(w, K, C, RS, img_fwd, img_bwd, (hipStream_t)stream);
}

// Pre-split activation images (csrc/p3d_fx.hip): a fp32 NCHW tensor as three bf16 planes [N][C/16][HW][16], the form in which the x3 kernels take operands
// without splitting them.  mode 0: the tensor; 1: relu(x * sc + sh); 2: A * (masked ? g * [c * sc + sh > 0] : g) + B * c + K with x = g, x2 = c
// (table = one BatchNorm layer's [C][8] floats {sc, sh, mean, invstd, A, B, K, 0}).
size_t p3d_fx_act_image_bytes(int32_t N, int32_t C, int32_t HW) { return (N > 0 && C > 0 && HW > 0) ? fx_act_image_bytes(N, C, HW) : 0; }

int32_t p3d_fx_act_image(int32_t mode, const float* x, const float* x2, const float* table, int32_t masked, void* img, int32_t N, int32_t C, int32_t HW, void* stream) {
    return fx_act_image(mode, x, x2, table, masked, img, N, C, HW, (hipStream_t)stream);
}

// Row images: the same tensor, same channel-blocked rows, holding the fp32 value itself ([N][C/16][HW][16] floats); modes as p3d_fx_act_image
size_t p3d_fx_row_image_bytes(int32_t N, int32_t C, int32_t HW) { return (N > 0 && C > 0 && HW > 0) ? fx_row_image_bytes(N, C, HW) : 0; }

int32_t p3d_fx_row_image(int32_t mode, const float* x, const float* x2, const float* table, int32_t masked, void* img, int32_t N, int32_t C, int32_t HW, void* stream) {
    return fx_act_image(mode, x, x2, table, masked, img, N, C, HW, (hipStream_t)stream, nullptr, nullptr, true);
}

// The image passes that open a block's backward pass, alone (tests): d c = A g + B c + K with g = x masked by `gmask` (bit e of byte i: element 4 i + e passes; may be
// null) and the constants finalized in the pass's prologue from fp64 partial sums [C][nrows][3] = (sum g, sum g (c_a - mean_a), sum g (c_b - mean_b)) -- FxFinalize kind 3.
// c_b null: the mode-2 pass for side a.  c_b given: both images in ONE pass (fx_act_image_pair).  table_*: the layers' [C][8] tables (mean, invstd read); d gamma / d beta
// are written.  rows: 0 three-plane images, 1 fp32 row images.
int32_t p3d_fx_open_images(int32_t rows, const float* x, const unsigned char* gmask, const double* partial, int32_t nrows, double count, const float* c_a, const float* table_a,
                           const float* gamma_a, float* dgamma_a, float* dbeta_a, void* img_a, const float* c_b, const float* table_b, const float* gamma_b, float* dgamma_b,
                           float* dbeta_b, void* img_b, int32_t N, int32_t C, int32_t HW, void* stream) {
    P3D_REQUIRE(x && partial && nrows > 0 && count > 0 && c_a && table_a && gamma_a && dgamma_a && dbeta_a && img_a, "fx_open_images: null argument");
    P3D_REQUIRE(!c_b || (table_b && gamma_b && dgamma_b && dbeta_b && img_b), "fx_open_images: null argument of the second image");
    auto fin = [&](int which, const float* gamma, float* dgamma, float* dbeta, const float* table) {
        FxFinalize f{};
        f.kind = 3; f.partial = partial; f.rows = nrows; f.which = which; f.count = count; f.gamma = gamma; f.dgamma = dgamma; f.dbeta = dbeta; f.table = const_cast<float*>(table);
        f.gmask = gmask;
        return f;
    };
    const FxFinalize fa = fin(0, gamma_a, dgamma_a, dbeta_a, table_a);
    if (!c_b) return fx_act_image(2, x, c_a, table_a, 0, img_a, N, C, HW, (hipStream_t)stream, &fa, nullptr, rows != 0);
    const FxFinalize fb = fin(1, gamma_b, dgamma_b, dbeta_b, table_b);
    return fx_act_image_pair(x, gmask, c_a, c_b, img_a, img_b, &fa, &fb, N, C, HW, (hipStream_t)stream, nullptr, rows != 0);
}

// The three passes of a convolution with image operands (what p3d_block_* launches inside a block), for callers that hold images of their own.
// x_img / dy_img: p3d_fx_act_image of the fp32 tensor p3d_conv2d_* would take; wimg: the matching p3d_fx_weight_images image, or NULL (built into the workspace).
size_t p3d_fx_conv_img_workspace_bytes(const p3d_conv_desc* d, int32_t pass) {
    if (!d) return 0;
    return fx_workspace(pass == 0 ? FX_FWD : pass == 1 ? FX_DGRAD : FX_WGRAD, d);
}

// bit 0 / 1 / 2: the forward / data-gradient / weight-gradient pass of this convolution can run on image operands
int32_t p3d_fx_conv_img_supported(const p3d_conv_desc* d) {
    if (!d || !fx_enabled() || d->C % 16 != 0 || d->K % 16 != 0 || (d->H * d->W) % 4 != 0 || (d->Ho * d->Wo) % 4 != 0) return 0;
    return (fx_applies(FX_FWD, d, 32) ? 1 : 0) | (fx_applies(FX_DGRAD, d, 32) ? 2 : 0) | (fx_applies(FX_WGRAD, d, 32) ? 4 : 0);
}

static int32_t conv_fwd_img(const char* name, bool rows, const p3d_conv_desc* d, const void* x_img, const float* w, const void* wimg, const float* bias, float* y, void* workspace,
                            size_t workspace_bytes, void* stream) {
    P3D_REQUIRE(d && x_img && w && y, "%s: null argument", name);
    P3D_REQUIRE(fx_applies(FX_FWD, d, 32) && d->C % 16 == 0 && (d->H * d->W) % 4 == 0, "%s: shape outside the x3 kernels", name);
    FxFuse f{};
    f.act_img = x_img; f.wimg = wimg; f.rows = rows;
    ProfScope ps(0, d, (hipStream_t)stream);
    fx_count(0, d);
    return name_entry(name, fx_conv_fwd(d, nullptr, w, bias, y, workspace, workspace_bytes, &f, (hipStream_t)stream));
}
int32_t p3d_fx_conv_fwd_img(const p3d_conv_desc* d, const void* x_img, const float* w, const void* wimg, const float* bias, float* y, void* workspace,
                            size_t workspace_bytes, void* stream) {
    return conv_fwd_img("fx_conv_fwd_img", false, d, x_img, w, wimg, bias, y, workspace, workspace_bytes, stream);
}
int32_t p3d_fx_conv_fwd_rows(const p3d_conv_desc* d, const void* x_rows, const float* w, const void* wimg, const float* bias, float* y, void* workspace,
                             size_t workspace_bytes, void* stream) {
    return conv_fwd_img("fx_conv_fwd_rows", true, d, x_rows, w, wimg, bias, y, workspace, workspace_bytes, stream);
}

static int32_t conv_dgrad_img(const char* name, bool rows, const p3d_conv_desc* d, const void* dy_img, const float* w, const void* wimgT, float* dx, void* workspace,
                              size_t workspace_bytes, void* stream) {
    P3D_REQUIRE(d && dy_img && w && dx, "%s: null argument", name);
    P3D_REQUIRE(fx_applies(FX_DGRAD, d, 32) && d->K % 16 == 0 && (d->Ho * d->Wo) % 4 == 0, "%s: shape outside the x3 kernels", name);
    FxFuse f{};
    f.act_img = dy_img; f.wimg = wimgT; f.rows = rows;
    ProfScope ps(1, d, (hipStream_t)stream);
    fx_count(1, d);
    if (int32_t e = fx_dgrad_zero_dead_classes(d, dx, (hipStream_t)stream)) return e;
    return name_entry(name, fx_conv_dgrad(d, nullptr, w, dx, workspace, workspace_bytes, &f, (hipStream_t)stream));
}
int32_t p3d_fx_conv_dgrad_img(const p3d_conv_desc* d, const void* dy_img, const float* w, const void* wimgT, float* dx, void* workspace, size_t workspace_bytes,
                              void* stream) {
    return conv_dgrad_img("fx_conv_dgrad_img", false, d, dy_img, w, wimgT, dx, workspace, workspace_bytes, stream);
}
int32_t p3d_fx_conv_dgrad_rows(const p3d_conv_desc* d, const void* dy_rows, const float* w, const void* wimgT, float* dx, void* workspace, size_t workspace_bytes,
                               void* stream) {
    return conv_dgrad_img("fx_conv_dgrad_rows", true, d, dy_rows, w, wimgT, dx, workspace, workspace_bytes, stream);
}

// x: the fp32 input, used when x_img is NULL (the block input of a residual block); otherwise ignored
static int32_t conv_wgrad_img(const char* name, bool rows, const p3d_conv_desc* d, const void* dy_img, const float* x, const void* x_img, float* dw, void* workspace,
                              size_t workspace_bytes, void* stream) {
    P3D_REQUIRE(d && dy_img && (x || x_img) && dw, "%s: null argument", name);
    P3D_REQUIRE(fx_applies(FX_WGRAD, d, 32) && d->K % 16 == 0 && (!x_img || d->C % 16 == 0), "%s: shape outside the x3 kernels", name);
    FxFuse f{};
    f.dy_img = dy_img; f.x_img = x_img; f.rows = rows;
    ProfScope ps(2, d, (hipStream_t)stream);
    fx_count(2, d);
    return fx_conv_wgrad(d, nullptr, x, dw, d->accumulate, workspace, workspace_bytes, &f, name, (hipStream_t)stream);
}
int32_t p3d_fx_conv_wgrad_img(const p3d_conv_desc* d, const void* dy_img, const float* x, const void* x_img, float* dw, void* workspace, size_t workspace_bytes,
                              void* stream) {
    return conv_wgrad_img("fx_conv_wgrad_img", false, d, dy_img, x, x_img, dw, workspace, workspace_bytes, stream);
}
int32_t p3d_fx_conv_wgrad_rows(const p3d_conv_desc* d, const void* dy_rows, const float* x, const void* x_rows, float* dw, void* workspace, size_t workspace_bytes,
                               void* stream) {
    return conv_wgrad_img("fx_conv_wgrad_rows", true, d, dy_rows, x, x_rows, dw, workspace, workspace_bytes, stream);
}

// The same three passes at any map width (include/p3d_hip.h): the ragged image-fed instances of fx_conv_kernel and fx_wgrad_any_img_kernel.  Dense convolutions with
// whole weights only, no fp32 fallback for an operand; for the shapes p3d_fx_conv_img_supported refuses, correct at the ones it admits too.
int32_t p3d_x3_any_images_enable(int32_t on) { return fx_set_any_images_enabled(on); }

static int32_t img_any_bits(const p3d_conv_desc* d) {
    if (!d || d->N <= 0 || d->C <= 0 || d->K <= 0 || d->H <= 0 || d->W <= 0 || d->R <= 0 || d->S <= 0 || d->stride < 1 || d->dil < 1 || d->pad < 0) return 0;
    // (the kernels take the geometry from the descriptor: the output sides must be the derived ones)
    if (d->Ho <= 0 || d->Wo <= 0 || d->Ho != (d->H + 2 * d->pad - d->dil * (d->R - 1) - 1) / d->stride + 1 || d->Wo != (d->W + 2 * d->pad - d->dil * (d->S - 1) - 1) / d->stride + 1) return 0;
    if (d->C % 16 != 0 || d->K % 16 != 0 || d->Ho * d->Wo < 16 || d->c_offset != 0 || d->c_total != d->C) return 0;
    return (fx_applies(FX_FWD, d, 96, true) ? 1 : 0) | (d->stride == 1 && fx_applies(FX_DGRAD, d, 96, true) ? 2 : 0) | (fx_applies(FX_WGRAD, d, 96, true) ? 4 : 0);
}
int32_t p3d_fx_conv_img_any_supported(const p3d_conv_desc* d) { return img_any_bits(d); }

size_t p3d_fx_conv_img_any_workspace_bytes(const p3d_conv_desc* d, int32_t pass) {
    if (!d) return 0;
    return fx_workspace(pass == 0 ? FX_FWD : pass == 1 ? FX_DGRAD : FX_WGRAD, d, true);
}

int32_t p3d_fx_act_image_any(const float* x, void* img, int32_t N, int32_t C, int32_t HW, void* stream) {
    return fx_act_image_any(x, img, N, C, HW, (hipStream_t)stream);
}

int32_t p3d_fx_conv_fwd_img_any(const p3d_conv_desc* d, const void* x_img, const float* w, const void* wimg, const float* bias, float* y, void* workspace,
                                size_t workspace_bytes, void* stream) {
    P3D_REQUIRE(d && x_img && w && y, "fx_conv_fwd_img_any: null argument");
    P3D_REQUIRE(img_any_bits(d) & 1, "fx_conv_fwd_img_any: shape outside the ragged image-fed kernels");
    P3D_REQUIRE(d->accumulate == 0 || d->accumulate == 1, "fx_conv_fwd_img_any: accumulate must be 0 or 1");
    P3D_REQUIRE(aligned16(x_img, wimg, y, workspace), "fx_conv_fwd_img_any: the image, the weight image, y and the workspace must be 16-B aligned");
    const size_t need = fx_workspace(FX_FWD, d, true);
    if (need && (!workspace || workspace_bytes < need)) { set_error("fx_conv_fwd_img_any: workspace %zu B < required %zu B", workspace_bytes, need); return P3D_EWORKSPACE; }
    FxFuse f{};
    f.act_img = x_img; f.wimg = wimg; f.ragged = 1;
    ProfScope ps(0, d, (hipStream_t)stream);
    fx_count(0, d);
    return name_entry("fx_conv_fwd_img_any", fx_conv_fwd(d, nullptr, w, bias, y, workspace, workspace_bytes, &f, (hipStream_t)stream));
}

int32_t p3d_fx_conv_dgrad_img_any(const p3d_conv_desc* d, const void* dy_img, const float* w, const void* wimgT, float* dx, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    P3D_REQUIRE(d && dy_img && w && dx, "fx_conv_dgrad_img_any: null argument");
    P3D_REQUIRE(img_any_bits(d) & 2, "fx_conv_dgrad_img_any: shape outside the ragged image-fed kernels (stride 1 only)");
    P3D_REQUIRE(d->accumulate == 0 || d->accumulate == 1, "fx_conv_dgrad_img_any: accumulate must be 0 or 1");
    P3D_REQUIRE(aligned16(dy_img, wimgT, dx, workspace), "fx_conv_dgrad_img_any: the image, the weight image, dx and the workspace must be 16-B aligned");
    const size_t need = fx_workspace(FX_DGRAD, d, true);
    if (need && (!workspace || workspace_bytes < need)) { set_error("fx_conv_dgrad_img_any: workspace %zu B < required %zu B", workspace_bytes, need); return P3D_EWORKSPACE; }
    FxFuse f{};
    f.act_img = dy_img; f.wimg = wimgT; f.ragged = 1;
    ProfScope ps(1, d, (hipStream_t)stream);
    fx_count(1, d);
    return name_entry("fx_conv_dgrad_img_any", fx_conv_dgrad(d, nullptr, w, dx, workspace, workspace_bytes, &f, (hipStream_t)stream));
}

// The stride-2 data gradient on an image operand at any map side (include/p3d_hip.h): the class launches of fx_conv_dgrad_strided_any on the image-fed ragged
// instance, then the interleave.  Entries of their own: p3d_fx_conv_dgrad_img_any and p3d_fx_conv_img_any_supported keep refusing stride 2.
static bool strided_img_any_ok(const p3d_conv_desc* d) {
    if (!d || d->N <= 0 || d->C <= 0 || d->K <= 0 || d->H <= 0 || d->W <= 0 || d->R <= 0 || d->S <= 0 || d->stride != 2 || d->dil < 1 || d->pad < 0) return false;
    if (d->Ho <= 0 || d->Wo <= 0 || d->Ho != (d->H + 2 * d->pad - d->dil * (d->R - 1) - 1) / d->stride + 1 || d->Wo != (d->W + 2 * d->pad - d->dil * (d->S - 1) - 1) / d->stride + 1) return false;
    return d->C % 16 == 0 && d->K % 16 == 0 && fx_dgrad_strided_any_applies(d, 32);      // (whole weights: the rule itself)
}
int32_t p3d_fx_conv_dgrad_strided_img_any_supported(const p3d_conv_desc* d) { return strided_img_any_ok(d) ? 1 : 0; }
size_t p3d_fx_conv_dgrad_strided_img_any_workspace_bytes(const p3d_conv_desc* d) { return strided_img_any_ok(d) ? fx_dgrad_strided_any_plan(d).workspace : 0; }
int32_t p3d_fx_conv_dgrad_strided_img_any(const p3d_conv_desc* d, const void* dy_img, const float* w, const void* wimgT, float* dx, void* workspace, size_t workspace_bytes,
                                          void* stream) {
    P3D_REQUIRE(d && dy_img && w && dx, "fx_conv_dgrad_strided_img_any: null argument");
    P3D_REQUIRE(strided_img_any_ok(d), "fx_conv_dgrad_strided_img_any: shape outside the stride-2 class launches of the ragged image-fed kernels");
    P3D_REQUIRE(d->accumulate == 0 || d->accumulate == 1, "fx_conv_dgrad_strided_img_any: accumulate must be 0 or 1");
    P3D_REQUIRE(aligned16(dy_img, wimgT, workspace) && (reinterpret_cast<uintptr_t>(dx) & 3) == 0,
                "fx_conv_dgrad_strided_img_any: the image, the weight image and the workspace must be 16-B aligned");
    const FxStridedPlan pl = fx_dgrad_strided_any_plan(d);
    if (!workspace || workspace_bytes < pl.workspace) { set_error("fx_conv_dgrad_strided_img_any: workspace %zu B < required %zu B", workspace_bytes, pl.workspace); return P3D_EWORKSPACE; }
    ProfScope ps(1, d, (hipStream_t)stream);
    fx_count(1, d);
    int live = 0;
    if (int32_t e = name_entry("fx_conv_dgrad_strided_img_any", fx_conv_dgrad_strided_any(d, nullptr, w, workspace, workspace_bytes, &live, (hipStream_t)stream, dy_img, wimgT))) return e;
    return fx_dgrad_interleave_rows((const float*)((const char*)workspace + pl.stage_offset), dx, nullptr, d->N, d->C, d->H, d->W, pl.cls_stride, live, d->accumulate,
                                    (hipStream_t)stream);
}

// x: ignored (the signature of p3d_fx_conv_wgrad_img; there is no fp32 fallback here)
int32_t p3d_fx_conv_wgrad_img_any(const p3d_conv_desc* d, const void* dy_img, const float* x, const void* x_img, float* dw, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    (void)x;
    P3D_REQUIRE(d && dy_img && x_img && dw, "fx_conv_wgrad_img_any: null argument (both images are required)");
    P3D_REQUIRE(img_any_bits(d) & 4, "fx_conv_wgrad_img_any: shape outside the ragged image-fed kernels");
    P3D_REQUIRE(d->accumulate == 0 || d->accumulate == 1, "fx_conv_wgrad_img_any: accumulate must be 0 or 1");
    // (dw may sit anywhere on a 4-B line -- a view into a flat gradient buffer: wgrad_finish picks its accesses by the address)
    P3D_REQUIRE(aligned16(dy_img, x_img, workspace) && (reinterpret_cast<uintptr_t>(dw) & 3) == 0, "fx_conv_wgrad_img_any: the images and the workspace must be 16-B aligned");
    FxFuse f{};
    f.dy_img = dy_img; f.x_img = x_img; f.ragged = 1;
    ProfScope ps(2, d, (hipStream_t)stream);
    fx_count(2, d);
    return fx_conv_wgrad(d, nullptr, nullptr, dw, d->accumulate, workspace, workspace_bytes, &f, "fx_conv_wgrad_img_any", (hipStream_t)stream);
}

// What the forward / data-gradient launchers launched, and what they can launch (include/p3d_hip.h)
int32_t p3d_fx_launch_log(int32_t* out, int32_t max_records, int32_t reset) { return fx_launch_log(out, out && max_records > 0 ? max_records : 0, reset); }
int32_t p3d_fx_conv_instances(int32_t* out, int32_t max_records) { return fx_conv_instances(out, out && max_records > 0 ? max_records : 0); }
int32_t p3d_fx_conv_any_sums_instances(int32_t* out, int32_t max_records) { return fx_conv_any_sums_instances(out, out && max_records > 0 ? max_records : 0); }

// Test hook: fx_conv_fwd / fx_conv_dgrad with any FxFuse (include/p3d_hip.h).  Checks what the launchers take for granted from their callers -- the pointers, a
// well-formed descriptor, the shape rule of the pass -- and leaves every other refusal to them.  No zero fill of dead parity classes, no path count.
static bool fused_desc_ok(const p3d_conv_desc* d) {
    if (!d || d->N <= 0 || d->C <= 0 || d->K <= 0 || d->H <= 0 || d->W <= 0 || d->R <= 0 || d->S <= 0 || d->stride < 1 || d->dil < 1 || d->pad < 0) return false;
    if (d->accumulate < 0 || d->accumulate > 1 || d->c_total < d->C) return false;
    return d->Ho > 0 && d->Wo > 0 && d->Ho == (d->H + 2 * d->pad - d->dil * (d->R - 1) - 1) / d->stride + 1 && d->Wo == (d->W + 2 * d->pad - d->dil * (d->S - 1) - 1) / d->stride + 1;
}
// (0 from both queries: a descriptor, or a shape, the hook refuses -- the dense rule; a call with a factor needs 64 result channels on top)
size_t p3d_fx_conv_fused_workspace_bytes(int32_t pass, const p3d_conv_desc* d, int32_t ragged) {
    if (!fused_desc_ok(d) || pass < 0 || pass > 1 || !fx_applies(pass == 0 ? FX_FWD : FX_DGRAD, d, 32, ragged != 0)) return 0;
    return fx_workspace(pass == 0 ? FX_FWD : FX_DGRAD, d, ragged != 0);
}
int32_t p3d_fx_conv_fused_partial_rows(int32_t pass, const p3d_conv_desc* d) {
    if (!fused_desc_ok(d) || pass < 0 || pass > 1) return 0;
    if (!fx_applies(pass == 0 ? FX_FWD : FX_DGRAD, d, 32, false) && !fx_applies(pass == 0 ? FX_FWD : FX_DGRAD, d, 32, true)) return 0;
    return fx_partial_rows(pass == 0 ? FX_FWD : FX_DGRAD, d);
}
int32_t p3d_fx_conv_fused_partial_rows_any(int32_t pass, const p3d_conv_desc* d) {
    if (!fused_desc_ok(d) || pass < 0 || pass > 1 || d->stride != 1 || !fx_applies(pass == 0 ? FX_FWD : FX_DGRAD, d, 32, true)) return 0;
    return fx_partial_rows(pass == 0 ? FX_FWD : FX_DGRAD, d, true);
}
int32_t p3d_fx_conv_fused(int32_t pass, const p3d_conv_desc* d, const p3d_fx_fuse* f, const float* src, const float* w, const float* bias, float* out, void* workspace,
                          size_t workspace_bytes, void* stream) {
    P3D_REQUIRE(d && f && w && out && (src || f->act_img) && (pass == 0 || pass == 1), "fx_conv_fused: null argument, or a pass other than 0 / 1");
    P3D_REQUIRE(fused_desc_ok(d), "fx_conv_fused: malformed descriptor");
    P3D_REQUIRE(pass == 0 || !bias, "fx_conv_fused: the data gradient takes no bias");
    P3D_REQUIRE(!f->partial || pass == 0 || (f->ep_c && f->ep_tab), "fx_conv_fused: the backward sums need ep_c and ep_tab");
    P3D_REQUIRE(!f->acc_mask || f->acc_src, "fx_conv_fused: mask bytes without an accumulation source");
    const FxPass ps = pass == 0 ? FX_FWD : FX_DGRAD;
    const bool masked = f->pmask || f->emask, rag = f->ragged != 0;
    P3D_REQUIRE(masked ? fx_masked_applies(ps, d, rag) : fx_applies(ps, d, 32, rag), "fx_conv_fused: shape outside the x3 kernels");
    P3D_REQUIRE(aligned16(src, f->act_img, f->wimg, out, workspace, f->ep_c, f->acc_src, f->res) && (rag || aligned16(f->pmask, f->emask)),
                "fx_conv_fused: operands, result and workspace must be 16-B aligned");
    FxFuse x{};
    x.act_img = f->act_img; x.wimg = f->wimg; x.partial = f->partial; x.ep_c = f->ep_c; x.ep_tab = f->ep_tab; x.pmask = f->pmask; x.emask = f->emask;
    x.acc_src = f->acc_src; x.acc_mask = f->acc_mask; x.infer = f->infer != 0; x.res = f->res; x.relu = f->relu != 0; x.rows = f->rows != 0; x.ragged = rag;
    return name_entry("fx_conv_fused", pass == 0 ? fx_conv_fwd(d, src, w, bias, out, workspace, workspace_bytes, &x, (hipStream_t)stream)
                                                 : fx_conv_dgrad(d, src, w, out, workspace, workspace_bytes, &x, (hipStream_t)stream));
}

// Test hook: one image pass of mode 1 / 2 with its finalize prologue, aligned or at any HW (include/p3d_hip.h)
int32_t p3d_fx_act_image_fused(int32_t any, int32_t mode, const float* x, const float* x2, float* table, int32_t masked, void* img, int32_t N, int32_t C, int32_t HW,
                               int32_t kind, const void* partial, int32_t rows, int32_t which, double count, const float* gamma, const float* beta, float* running_mean,
                               float* running_var, float momentum, float eps, float* dgamma, float* dbeta, int32_t accumulate, void* stream) {
    P3D_REQUIRE(mode == 1 || mode == 2, "fx_act_image_fused: modes 1 and 2");
    P3D_REQUIRE(kind == 0 || (kind >= 1 && kind <= 3 && count > 0 && (which == 0 || which == 1)), "fx_act_image_fused: bad finalize request (kind %d)", kind);
    FxFinalize f{};
    if (kind != 0) {
        f.kind = kind; f.partial = partial; f.rows = rows; f.which = which; f.count = count; f.gamma = gamma; f.beta = beta; f.running_mean = running_mean;
        f.running_var = running_var; f.momentum = momentum; f.eps = eps; f.dgamma = dgamma; f.dbeta = dbeta; f.accumulate = accumulate; f.table = table;
    }
    const FxFinalize* fp = kind ? &f : nullptr;
    return any ? fx_act_image_any_map(mode, x, x2, table, masked, img, N, C, HW, (hipStream_t)stream, fp)
               : fx_act_image(mode, x, x2, table, masked, img, N, C, HW, (hipStream_t)stream, fp);
}

// Test hook: how a weight gradient would be planned, as a record (include/p3d_hip.h).  Host-only.
int32_t p3d_fx_wgrad_plan(const p3d_conv_desc* d, int32_t operands, int32_t* out) {
    P3D_REQUIRE(d && out && operands >= 0 && operands < 128, "fx_wgrad_plan: null argument, or operand bits beyond bit 6");
    P3D_REQUIRE(fused_desc_ok(d), "fx_wgrad_plan: malformed descriptor");
    return fx_wgrad_plan_record(d, operands, out);
}

// What the weight-gradient launcher launched (include/p3d_hip.h)
int32_t p3d_fx_wgrad_launch_log(int32_t* out, int32_t max_records, int32_t reset) { return fx_wgrad_launch_log(out, out && max_records > 0 ? max_records : 0, reset); }

// Test hook: fx_conv_wgrad with any operands (include/p3d_hip.h).  Like p3d_fx_conv_fused it checks the pointers, the descriptor, the shape rule and the alignment, and
// leaves every other refusal (the operand rule, the workspace) to the launcher.  No path count.
static FxFuse wgrad_fuse(const p3d_fx_wgrad_fuse* f) {
    FxFuse x{};
    x.dy_img = f->dy_img; x.x_img = f->x_img; x.pmask = f->pmask; x.emask = f->emask; x.rows = f->rows != 0; x.ragged = f->ragged != 0;
    return x;
}
// (0: a descriptor or a shape the hook refuses)
size_t p3d_fx_conv_wgrad_fused_workspace_bytes(const p3d_conv_desc* d, const p3d_fx_wgrad_fuse* f) {
    if (!f || !fused_desc_ok(d) || !fx_applies(FX_WGRAD, d, 32, f->ragged != 0)) return 0;
    const FxFuse x = wgrad_fuse(f);
    return fx_wgrad_plan(d, &x).slab_bytes;
}
int32_t p3d_fx_conv_wgrad_fused(const p3d_conv_desc* d, const p3d_fx_wgrad_fuse* f, const float* dy, const float* x, float* dw, void* workspace, size_t workspace_bytes,
                                void* stream) {
    P3D_REQUIRE(d && f && dw && (dy || f->dy_img) && (x || f->x_img), "fx_conv_wgrad_fused: null argument");
    P3D_REQUIRE(fused_desc_ok(d), "fx_conv_wgrad_fused: malformed descriptor");
    P3D_REQUIRE(fx_applies(FX_WGRAD, d, 32, f->ragged != 0), "fx_conv_wgrad_fused: shape outside the x3 kernels");
    // (dw may sit anywhere on a 4-B line, and be a channel window of a wider weight: wgrad_finish picks its accesses by the address)
    P3D_REQUIRE(aligned16(dy, x, f->dy_img, f->x_img, workspace) && (f->ragged || aligned16(f->pmask, f->emask)) && (reinterpret_cast<uintptr_t>(dw) & 3) == 0,
                "fx_conv_wgrad_fused: operands and workspace must be 16-B aligned, dw 4-B aligned");
    const FxFuse fuse = wgrad_fuse(f);
    return fx_conv_wgrad(d, dy, x, dw, d->accumulate, workspace, workspace_bytes, &fuse, "fx_conv_wgrad_fused", (hipStream_t)stream);
}

// Inference with folded BatchNorm (include/p3d_hip.h): the fold of a whole network in one launch, and the forward on the folded images with the inference epilogue.
int32_t p3d_fx_fold_bn_images(const void* jobs, int32_t njobs, int32_t blocks, void* stream) {
    P3D_REQUIRE(jobs && njobs > 0 && blocks > 0, "fold_bn_images: bad argument");
    return fx_fold_bn_images(jobs, njobs, blocks, (hipStream_t)stream);
}

int32_t p3d_fx_conv_fwd_infer_supported(const p3d_conv_desc* d, int32_t image_fed) {
    if (!d || d->c_offset != 0 || d->c_total != d->C || d->accumulate < 0 || d->accumulate > 1 || !fx_applies(FX_FWD, d, 32)) return 0;
    return !image_fed || (d->C % 16 == 0 && (d->H * d->W) % 4 == 0) ? 1 : 0;
}
size_t p3d_fx_conv_fwd_infer_workspace_bytes(const p3d_conv_desc* d) { return d ? fx_workspace(FX_FWD, d) : 0; }
// The same at any map width (fx_conv_kernel's ragged instances; split-K: their slabs, then fx_reduce_any_kernel): fp32-fed only
int32_t p3d_fx_conv_fwd_infer_any_supported(const p3d_conv_desc* d) {
    return d && d->c_offset == 0 && d->c_total == d->C && d->accumulate >= 0 && d->accumulate <= 1 && fx_applies(FX_FWD, d, 32, true) ? 1 : 0;
}
size_t p3d_fx_conv_fwd_infer_any_workspace_bytes(const p3d_conv_desc* d) { return d ? fx_workspace(FX_FWD, d, true) : 0; }
// The same for a partial convolution (FX_EPI_INFER_FACTOR; split-K: fx_reduce_kernel applies the factor before b')
int32_t p3d_fx_conv_fwd_infer_masked_supported(const p3d_conv_desc* d) {
    return d && d->c_offset == 0 && d->c_total == d->C && d->accumulate == 0 && fx_masked_applies(FX_FWD, d) ? 1 : 0;
}
// The partial convolution at any map width (the ragged PRO-4 instances, FX_EPI_INFER_FACTOR; split-K: their slabs, then fx_reduce_any_kernel with the factor before b')
int32_t p3d_fx_conv_fwd_infer_masked_any_supported(const p3d_conv_desc* d) {
    return d && d->c_offset == 0 && d->c_total == d->C && d->accumulate == 0 && fx_masked_applies(FX_FWD, d, true) ? 1 : 0;
}
size_t p3d_fx_conv_fwd_infer_masked_any_workspace_bytes(const p3d_conv_desc* d) { return d ? fx_workspace(FX_FWD, d, true) : 0; }

// What the four inference entries share: the checks (every text opens with the entry's own name), the profile bracket, the path counter and the launch.
// f says which entry this is: `ragged` a ragged one, a pmask a masked one.  (Alignment, ragged: of the base pointers only; inside the tensors the kernel picks
// 16-B or dword accesses by the address.)
static FxFuse infer_fuse(bool ragged, const void* x_img, const void* wimg, const float* mask_in, const float* mult, const float* res, int32_t relu) {
    FxFuse f{};
    f.infer = 1; f.ragged = ragged ? 1 : 0; f.act_img = x_img; f.wimg = wimg; f.pmask = mask_in; f.emask = mult; f.res = res; f.relu = relu ? 1 : 0; return f;
}
static int32_t fx_infer_entry(const char* name, bool args, const p3d_conv_desc* d, const float* x, size_t wimg_bytes, const float* bias, float* y, const FxFuse& f,
                              void* workspace, size_t workspace_bytes, void* stream) {
    P3D_REQUIRE(args, "%s: null argument", name);
    const char* kind = f.ragged ? (f.pmask ? "ragged masked " : "ragged ") : f.pmask ? "masked " : "";
    char acc[32] = "";
    if (kind[0]) snprintf(acc, sizeof(acc), " accumulate=%d", d->accumulate);
    P3D_REQUIRE(f.ragged ? (f.pmask ? p3d_fx_conv_fwd_infer_masked_any_supported(d) : p3d_fx_conv_fwd_infer_any_supported(d)) : f.pmask ? p3d_fx_conv_fwd_infer_masked_supported(d) : p3d_fx_conv_fwd_infer_supported(d, f.act_img != nullptr),
                "%s: shape outside the %sx3 kernels (N=%d C=%d %dx%d K=%d R=%d stride=%d c_offset=%d c_total=%d%s)", name, kind, d->N, d->C, d->H, d->W, d->K, d->R, d->stride,
                d->c_offset, d->c_total, acc);
    const size_t want = fx_weight_image_bytes(d->K, d->C, d->R * d->S, false);
    P3D_REQUIRE(wimg_bytes == want, "%s: weight image of %zu B does not belong to K=%d C=%d RS=%d (%zu B)", name, wimg_bytes, d->K, d->C, d->R * d->S, want);
    P3D_REQUIRE(aligned16(x, y, f.res, f.act_img, f.pmask, f.emask, f.wimg, workspace), "%s: operands must be 16-B aligned", name);
    ProfScope ps(0, d, (hipStream_t)stream);
    fx_count(0, d);
    return name_entry(name, fx_conv_fwd(d, f.act_img ? nullptr : x, nullptr, bias, y, workspace, workspace_bytes, &f, (hipStream_t)stream));
}
int32_t p3d_fx_conv_fwd_infer(const p3d_conv_desc* d, const float* x, const void* x_img, const void* wimg, size_t wimg_bytes, const float* bias, const float* res,
                              int32_t relu, float* y, void* workspace, size_t workspace_bytes, void* stream) {
    return fx_infer_entry("fx_conv_fwd_infer", d && (x || x_img) && wimg && y, d, x, wimg_bytes, bias, y, infer_fuse(false, x_img, wimg, nullptr, nullptr, res, relu), workspace,
                          workspace_bytes, stream);
}
int32_t p3d_fx_conv_fwd_infer_any(const p3d_conv_desc* d, const float* x, const void* wimg, size_t wimg_bytes, const float* bias, const float* res, int32_t relu,
                                  float* y, void* workspace, size_t workspace_bytes, void* stream) {
    return fx_infer_entry("fx_conv_fwd_infer_any", d && x && wimg && y, d, x, wimg_bytes, bias, y, infer_fuse(true, nullptr, wimg, nullptr, nullptr, res, relu), workspace,
                          workspace_bytes, stream);
}
int32_t p3d_fx_conv_fwd_infer_masked(const p3d_conv_desc* d, const float* x, const void* wimg, size_t wimg_bytes, const float* bias, const float* mask_in,
                                     const float* mult, const float* res, int32_t relu, float* y, void* workspace, size_t workspace_bytes, void* stream) {
    return fx_infer_entry("fx_conv_fwd_infer_masked", d && x && wimg && mask_in && mult && y, d, x, wimg_bytes, bias, y, infer_fuse(false, nullptr, wimg, mask_in, mult, res, relu),
                          workspace, workspace_bytes, stream);
}
int32_t p3d_fx_conv_fwd_infer_masked_any(const p3d_conv_desc* d, const float* x, const void* wimg, size_t wimg_bytes, const float* bias, const float* mask_in,
                                         const float* mult, const float* res, int32_t relu, float* y, void* workspace, size_t workspace_bytes, void* stream) {
    return fx_infer_entry("fx_conv_fwd_infer_masked_any", d && x && wimg && mask_in && mult && y, d, x, wimg_bytes, bias, y, infer_fuse(true, nullptr, wimg, mask_in, mult, res, relu),
                          workspace, workspace_bytes, stream);
}

// The stem conv1 = Conv2d(Cin <= 4, K, 7, stride 2, padding 3) (depthnet.py:138) on the x3 kernels: a 4x4 stride-1 convolution over a space-to-depth image of the
// input (csrc/p3d_fx.hip).  The caller builds the input image once per batch (p3d_stem_image: forward and weight gradient both read it) and the weight image
// once per optimizer step (p3d_stem_weight_image).
static p3d_conv_desc stem_desc(int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t K) {
    p3d_conv_desc d{};
    d.N = N; d.C = Cin; d.H = H; d.W = W; d.K = K; d.R = 7; d.S = 7; d.stride = 2; d.pad = 3; d.dil = 1; d.Ho = H / 2; d.Wo = W / 2; d.c_total = Cin;
    return d;
}
int32_t p3d_stem_supported(int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t K) { return fx_stem_applies(N, Cin, H, W, K) ? 1 : 0; }
size_t p3d_stem_image_bytes(int32_t N, int32_t H, int32_t W) { return fx_stem_image_bytes(N, H, W); }
size_t p3d_stem_weight_image_bytes(int32_t K) { return fx_stem_weight_image_bytes(K); }
size_t p3d_stem_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t K) { return fx_stem_workspace(N, H, W, K); }

int32_t p3d_stem_image(const float* x, void* img, int32_t N, int32_t Cin, int32_t H, int32_t W, void* stream) {
    return p3d_stem_image_masked(x, nullptr, img, N, Cin, H, W, stream);
}
int32_t p3d_stem_image_masked(const float* x, const float* mask_in, void* img, int32_t N, int32_t Cin, int32_t H, int32_t W, void* stream) {
    P3D_REQUIRE(x && img && N > 0 && Cin >= 1 && Cin <= 4 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0, "stem_image: bad argument");
    return fx_stem_image(x, mask_in, img, N, Cin, H, W, (hipStream_t)stream);
}
int32_t p3d_stem_masked_supported(int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t K) { return fx_stem_applies(N, Cin, H, W, K) && fx_stem_masked_applies(K) ? 1 : 0; }

int32_t p3d_stem_weight_image(const float* w, int32_t K, int32_t Cin, void* wimg, void* workspace, size_t workspace_bytes, void* stream) {
    P3D_REQUIRE(w && wimg && workspace && K > 0 && K % 16 == 0 && Cin >= 1 && Cin <= 4 && workspace_bytes >= (size_t)K * 256 * sizeof(float), "stem_weight_image: bad argument");
    return fx_stem_weight_image(w, K, Cin, wimg, workspace, (hipStream_t)stream);
}

int32_t p3d_stem_fwd(const void* x_img, const void* wimg, float* y, int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t K, void* stream) {
    return p3d_stem_fwd_masked(x_img, wimg, y, nullptr, N, Cin, H, W, K, stream);
}
int32_t p3d_stem_fwd_masked(const void* x_img, const void* wimg, float* y, const float* mult, int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t K, void* stream) {
    P3D_REQUIRE(x_img && wimg && y, "stem_fwd: null argument");
    P3D_REQUIRE(fx_stem_applies(N, Cin, H, W, K), "stem_fwd: shape outside the restated stem (N=%d Cin=%d %dx%d K=%d)", N, Cin, H, W, K);
    const p3d_conv_desc d = stem_desc(N, Cin, H, W, K);
    ProfScope ps(0, &d, (hipStream_t)stream);
    fx_count(0, &d);
    return fx_stem_fwd(x_img, wimg, y, mult, N, H, W, K, (hipStream_t)stream);
}

// The stem at ANY side >= 8 (odd crops: the reference's default -side_in 257): the input is zero-extended to (Hp, Wp) >= (H, W) that fx_stem_applies takes (the smallest Wp, then the smallest Hp for it) --
// the added zeros are the conv's own padding, so rows < (H - 1) / 2 + 1 and columns < (W - 1) / 2 + 1 of the padded conv are exactly the conv of x -- and the tail reads
// that prefix of the pitched result.  The conv itself is p3d_stem_fwd on the padded sides.
int32_t p3d_stem_any_padded(int32_t H, int32_t W, int32_t* Hp, int32_t* Wp) {
    if (H < 8 || W < 8 || H > (1 << 20) || W > (1 << 20)) return 0;
    int32_t wp = (W + 7) & ~7, hp = (H + 1) & ~1;
    while (((hp / 2) * (wp / 2)) % 16 != 0) hp += 2;       // (Wp / 2 is a multiple of 4: at most three steps)
    if (Hp) *Hp = hp;
    if (Wp) *Wp = wp;
    return 1;
}
int32_t p3d_stem_any_supported(int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t K) {
    int32_t hp = 0, wp = 0;
    return p3d_stem_any_padded(H, W, &hp, &wp) && fx_stem_applies(N, Cin, hp, wp, K) ? 1 : 0;
}
int32_t p3d_stem_image_any(const float* x, const float* mask_in, void* img, int32_t N, int32_t Cin, int32_t H, int32_t W, void* stream) {
    int32_t hp = 0, wp = 0;
    P3D_REQUIRE(x && img && N > 0 && Cin >= 1 && Cin <= 4 && p3d_stem_any_padded(H, W, &hp, &wp) && (int64_t)N * Cin * H * W < (1ll << 31), "stem_image_any: bad argument");
    P3D_REQUIRE((reinterpret_cast<uintptr_t>(img) & 15) == 0, "stem_image_any: the image must be 16-B aligned");
    return fx_stem_image_any(x, mask_in, img, N, Cin, H, W, hp, wp, (hipStream_t)stream);
}

int32_t p3d_stem_wgrad(const float* dy, const void* x_img, float* dw, int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t K, int32_t accumulate, void* workspace,
                       size_t workspace_bytes, void* stream) {
    return p3d_stem_wgrad_masked(dy, nullptr, x_img, dw, N, Cin, H, W, K, accumulate, workspace, workspace_bytes, stream);
}
int32_t p3d_stem_wgrad_masked(const float* dy, const float* mult, const void* x_img, float* dw, int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t K, int32_t accumulate,
                              void* workspace, size_t workspace_bytes, void* stream) {
    P3D_REQUIRE(dy && x_img && dw, "stem_wgrad: null argument");
    P3D_REQUIRE(fx_stem_applies(N, Cin, H, W, K), "stem_wgrad: shape outside the restated stem (N=%d Cin=%d %dx%d K=%d)", N, Cin, H, W, K);
    const p3d_conv_desc d = stem_desc(N, Cin, H, W, K);
    ProfScope ps(2, &d, (hipStream_t)stream);
    fx_count(2, &d);
    return name_entry(mult ? "stem_wgrad_masked" : "stem_wgrad", fx_stem_wgrad(dy, mult, x_img, dw, N, Cin, H, W, K, accumulate, workspace, workspace_bytes, (hipStream_t)stream));
}

// All weight images of a network in one launch.  jobs: device array of njobs records {const float* w; void* img_fwd; void* img_bwd; int32 K, C, RS, pad} (40 bytes each;
// a NULL image pointer skips that direction); blocks: grid width per job and direction (each block strides over the job's 16-B chunk positions).
int32_t p3d_fx_weight_images_batched(const void* jobs, int32_t njobs, int32_t blocks, void* stream) {
    P3D_REQUIRE(jobs && njobs > 0 && blocks > 0, "weight_images_batched: bad argument");
    return fx_build_weight_images_batched(jobs, njobs, blocks, (hipStream_t)stream);
}

// ---- profile of the conv launches made by the executor (and by p3d_conv2d_* when enabled) ---------------------------------------------------------
int32_t p3d_profile_enable(int32_t on) {
    const int32_t before = g_prof_on ? (g_prof_marks ? 2 : 1) : 0;
    g_prof_on = on != 0;
    g_prof_marks = on == 2;
    return before;
}

// Synchronises, sums the bracketed time per kind (0 forward, 1 data gradient, 2 weight gradient) and clears the records.
int32_t p3d_profile_collect(double* ms_by_kind, double* flops_by_kind, int64_t* launches_by_kind) {
    return p3d_profile_collect2(ms_by_kind, nullptr, flops_by_kind, launches_by_kind);
}

// The same with, per kind, the time of the conv kernels alone (the bracket up to the point where a split-K / slab sum was queued behind the kernel).
int32_t p3d_profile_collect2(double* ms_by_kind, double* kernel_ms_by_kind, double* flops_by_kind, int64_t* launches_by_kind) {
    for (int k = 0; k < 3; ++k) {
        if (ms_by_kind) ms_by_kind[k] = 0;
        if (kernel_ms_by_kind) kernel_ms_by_kind[k] = 0;
        if (flops_by_kind) flops_by_kind[k] = 0;
        if (launches_by_kind) launches_by_kind[k] = 0;
    }
    std::vector<ProfRec> recs;
    { std::lock_guard<std::mutex> lock(g_prof_mu); recs.swap(g_prof); }
    for (ProfRec& r : recs) {
        float ms = 0.f;
        if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            if (ms_by_kind) ms_by_kind[r.kind] += ms;
            if (flops_by_kind) flops_by_kind[r.kind] += r.flops;
            if (launches_by_kind) launches_by_kind[r.kind] += 1;
            float kms = ms;
            if (r.m && hipEventElapsedTime(&kms, r.a, r.m) != hipSuccess) kms = ms;
            if (kernel_ms_by_kind) kernel_ms_by_kind[r.kind] += kms;
        }
        (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b);
        if (r.m) (void)hipEventDestroy(r.m);
    }
    return P3D_OK;
}

}  // extern "C"
