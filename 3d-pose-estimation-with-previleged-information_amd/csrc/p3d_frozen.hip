// Training through a FROZEN (eval-mode) BatchNorm that is folded into its convolution (ops_frozen.py), fp32 NCHW, gfx950.
//
// With s = gamma / sqrtf(var + eps), w' = w * s, b' = beta - mean * s the layer is u = conv(x, w') + b' (+ res), y = relu?(u); the conv output z = conv(x, w)
// is never written.  Its backward needs two small kernels besides the two convolution gradients:
//
//   p3d_frozen_grad_mask     g = dy * [y > 0] (or g = dy without a ReLU: nothing written) and sums[k] = sum_{n,p} g[n,k,p] = dbeta.  One streaming pass: reads
//                            dy (and y), writes g.
//   p3d_frozen_wgrad_finish  from raw = wgrad(x, g): dw = s * raw, dbeta = sums, dgamma = (<w[k], raw[k]> - mean[k] * sums[k]) / sqrtf(var[k] + eps), because
//                            sum_p g[k,p] * z[k,p] = sum_{c,tap} w[k,c,tap] * raw[k,c,tap].  Weight-sized.
//
// Both reduce in fp64 in a fixed order (per-thread fp64 accumulators over a fixed assignment of elements -> wavefront shuffles -> LDS -> for the mask pass
// per-block partials in the workspace and one ordered sum); there is no floating-point atomic, so two runs give the same bits.
#include "p3d_common.h"

namespace p3d {

constexpr int FZ_MAX_SPLIT = 64;        // blocks per channel (grid.y) at the most
constexpr int FZ_MAX_CHANNELS = 2048;   // grid.x at the most: a block walks the channels k = blockIdx.x, blockIdx.x + gridDim.x, ...
constexpr int FZ_WAVE_ROW_HW = 1024;    // channel rows up to this long are taken by one wavefront each (four rows per block at a time)

__device__ __forceinline__ double block_sum1(double a, double* red /*[4]*/) {
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    a = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return a;
}

__device__ __forceinline__ float masked(float dy, float y) { return y > 0.f ? dy : 0.f; }

// Grid (min(K, FZ_MAX_CHANNELS), split).  Block (b, s) owns the images n = s, s + split, ... of the channels k = b, b + gridDim.x, ...; a channel row
// (n, k) is HW contiguous floats at element offset (n * K + k) * HW.  aligned (the three base pointers on 16-B lines): a row is read as up to three scalar
// elements up to its first 16-B line, float4 accesses, and up to three scalar elements behind the last full line -- with HW odd the rows start at every
// phase.  Otherwise everything goes element by element.  No access leaves the row.  WAVE_ROWS: one wavefront per row instead of the whole block.
// partial[k * split + s] = the block's sum of g over its rows of channel k.
template <bool RELU, bool WAVE_ROWS>
__global__ __launch_bounds__(256) void frozen_mask_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ g,
                                                          double* __restrict__ partial, int N, int K, int HW, int aligned) {
    const int s = blockIdx.y, split = gridDim.y;
    constexpr int G = WAVE_ROWS ? 64 : 256, NSUB = 256 / G;
    const int sub = WAVE_ROWS ? (int)(threadIdx.x >> 6) : 0, lane = WAVE_ROWS ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    __shared__ double red[4];
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        double acc = 0.0;
        for (int n = s + sub * split; n < N; n += NSUB * split) {
            const size_t off = ((size_t)n * K + k) * HW;
            int head = aligned ? (int)((4 - (off & 3)) & 3) : HW;
            if (head > HW) head = HW;
            const int nvec = (HW - head) >> 2, tail = head + 4 * nvec;
            for (int i = lane; i < head + (HW - tail); i += G) {             // the scalar elements in front of and behind the float4 body
                const size_t e = off + (i < head ? i : tail + (i - head));
                float v = dy[e];
                if constexpr (RELU) { v = masked(v, y[e]); g[e] = v; }
                acc += (double)v;
            }
            const float4* dv = reinterpret_cast<const float4*>(dy + off + head);
            for (int i = lane; i < nvec; i += G) {
                float4 q = dv[i];
                if constexpr (RELU) {
                    const float4 t = reinterpret_cast<const float4*>(y + off + head)[i];
                    q.x = masked(q.x, t.x); q.y = masked(q.y, t.y); q.z = masked(q.z, t.z); q.w = masked(q.w, t.w);
                    reinterpret_cast<float4*>(g + off + head)[i] = q;
                }
                acc += ((double)q.x + (double)q.y) + ((double)q.z + (double)q.w);
            }
        }
        acc = block_sum1(acc, red);
        if (threadIdx.x == 0) partial[(size_t)k * split + s] = acc;
    }
}

// sums[k] = the partials of channel k, added in the order of their blocks
__global__ __launch_bounds__(256) void frozen_mask_sum_kernel(const double* __restrict__ partial, int split, float* __restrict__ sums, int K) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    double a = 0.0;
    for (int i = 0; i < split; ++i) a += partial[(size_t)k * split + i];
    sums[k] = (float)a;
}

// One block per output channel k: dw[k] = s * raw[k] (+ dw[k]), <w[k], raw[k]> in fp64, then dgamma and dbeta by thread 0.  s is the expression of
// fx_fold_bn_kernel (p3d_fx.hip): a correctly rounded division by a correctly rounded sqrtf, so forward and backward scale by the same bits.
template <bool VEC>
__global__ __launch_bounds__(256) void frozen_finish_kernel(const float* __restrict__ raw, const float* __restrict__ w, const float* __restrict__ gamma,
                                                            const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                                            const float* __restrict__ sums, float* __restrict__ dw, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, int K, int CRS, int accumulate) {
    const int k = blockIdx.x;
    const float sd = sqrtf(var[k] + eps);
    const float s = gamma[k] / sd;
    const size_t row = (size_t)k * CRS;
    double acc = 0.0;
    if constexpr (VEC) {
        const float4* rv = reinterpret_cast<const float4*>(raw + row);
        const float4* wv = reinterpret_cast<const float4*>(w + row);
        float4* dv = reinterpret_cast<float4*>(dw + row);
        for (int i = threadIdx.x; i < CRS / 4; i += 256) {
            const float4 r = rv[i], q = wv[i];
            float4 o = {s * r.x, s * r.y, s * r.z, s * r.w};
            if (accumulate) { const float4 p = dv[i]; o.x += p.x; o.y += p.y; o.z += p.z; o.w += p.w; }
            dv[i] = o;
            acc += ((double)q.x * (double)r.x + (double)q.y * (double)r.y) + ((double)q.z * (double)r.z + (double)q.w * (double)r.w);
        }
    } else {
        for (int i = threadIdx.x; i < CRS; i += 256) {
            const float r = raw[row + i];
            float o = s * r;
            if (accumulate) o += dw[row + i];
            dw[row + i] = o;
            acc += (double)w[row + i] * (double)r;
        }
    }
    __shared__ double red[4];
    acc = block_sum1(acc, red);
    if (threadIdx.x == 0) {
        const float db = sums[k];
        const float dg = (float)((acc - (double)mean[k] * (double)db) / (double)sd);
        dgamma[k] = accumulate ? dgamma[k] + dg : dg;
        dbeta[k] = accumulate ? dbeta[k] + db : db;
    }
}

static int frozen_split(int N, int K) {
    int split = (int)ceil_div(2048, K < FZ_MAX_CHANNELS ? K : FZ_MAX_CHANNELS);      // >= ~8 blocks per CU over the chip
    if (split > N) split = N;
    if (split > FZ_MAX_SPLIT) split = FZ_MAX_SPLIT;
    return split < 1 ? 1 : split;
}

}  // namespace p3d

using namespace p3d;

extern "C" {

size_t p3d_frozen_grad_mask_workspace_bytes(int32_t N, int32_t K, int32_t HW) {
    (void)N; (void)HW;
    return K > 0 ? (size_t)K * FZ_MAX_SPLIT * sizeof(double) : 0;
}

int32_t p3d_frozen_grad_mask(const float* dy, const float* y, float* g, float* sums, int32_t N, int32_t K, int32_t HW, void* workspace, size_t workspace_bytes,
                             void* stream) {
    P3D_REQUIRE(dy && sums, "frozen_grad_mask: null tensor");
    P3D_REQUIRE((y == nullptr) == (g == nullptr), "frozen_grad_mask: y and g come together (a ReLU layer) or not at all");
    P3D_REQUIRE(N > 0 && K > 0 && HW > 0, "frozen_grad_mask: bad shape %d %d %d", N, K, HW);
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7) || workspace_bytes < p3d_frozen_grad_mask_workspace_bytes(N, K, HW)) {
        set_error("frozen_grad_mask: workspace missing, not on an 8-B line or too small");
        return P3D_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int split = frozen_split(N, K);
    const dim3 grid((unsigned)(K < FZ_MAX_CHANNELS ? K : FZ_MAX_CHANNELS), (unsigned)split);
    const int aligned = aligned16(dy, y, g) ? 1 : 0;
    double* partial = (double*)workspace;
    const bool wave_rows = HW <= FZ_WAVE_ROW_HW;
    if (y) {
        if (wave_rows) hipLaunchKernelGGL((frozen_mask_kernel<true, true>), grid, dim3(256), 0, st, dy, y, g, partial, N, K, HW, aligned);
        else hipLaunchKernelGGL((frozen_mask_kernel<true, false>), grid, dim3(256), 0, st, dy, y, g, partial, N, K, HW, aligned);
    } else {
        if (wave_rows) hipLaunchKernelGGL((frozen_mask_kernel<false, true>), grid, dim3(256), 0, st, dy, y, g, partial, N, K, HW, aligned);
        else hipLaunchKernelGGL((frozen_mask_kernel<false, false>), grid, dim3(256), 0, st, dy, y, g, partial, N, K, HW, aligned);
    }
    hipLaunchKernelGGL(frozen_mask_sum_kernel, dim3((unsigned)ceil_div(K, 256)), dim3(256), 0, st, (const double*)partial, split, sums, K);
    return check_launch("frozen_grad_mask");
}

int32_t p3d_frozen_wgrad_finish(const float* raw, const float* w, const float* gamma, const float* mean, const float* var, float eps, const float* sums,
                                float* dw, float* dgamma, float* dbeta, int32_t K, int32_t CRS, int32_t accumulate, void* stream) {
    P3D_REQUIRE(raw && w && gamma && mean && var && sums && dw && dgamma && dbeta, "frozen_wgrad_finish: null tensor");
    P3D_REQUIRE(K > 0 && CRS > 0, "frozen_wgrad_finish: bad shape %d %d", K, CRS);
    P3D_REQUIRE(raw != dw, "frozen_wgrad_finish: dw must not be the raw gradient");
    hipStream_t st = (hipStream_t)stream;
    if (CRS % 4 == 0 && aligned16(raw, w, dw))
        hipLaunchKernelGGL(frozen_finish_kernel<true>, dim3((unsigned)K), dim3(256), 0, st, raw, w, gamma, mean, var, eps, sums, dw, dgamma, dbeta, K, CRS, accumulate);
    else
        hipLaunchKernelGGL(frozen_finish_kernel<false>, dim3((unsigned)K), dim3(256), 0, st, raw, w, gamma, mean, var, eps, sums, dw, dgamma, dbeta, K, CRS, accumulate);
    return check_launch("frozen_wgrad_finish");
}

}  // extern "C"
