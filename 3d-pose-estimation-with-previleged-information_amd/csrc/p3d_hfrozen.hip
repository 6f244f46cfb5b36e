// Training through a FROZEN (eval-mode) BatchNorm folded into its fp16 convolution (-half_acc; ops_frozen.HFrozenConvBnFn), NHWC fp16, gfx950: the fp16 twin of
// p3d_frozen_grad_mask (p3d_frozen.hip), whose notes on the layer's algebra hold here unchanged.
//
//   p3d_hfrozen_grad_mask    dy, y, g are [P][K] halves.  g = dy where y > 0, else +0 (y == NULL: nothing written, dy itself is g), sums[k] = sum_p g[p][k].
//                            One streaming pass of 16-B accesses: a lane owns 8 channels of one pixel.
//
// Gradients carry the loss scale here and dy may sit near 65504, so no sum ever passes through fp16: every half is widened (exactly) to fp64 and accumulated there,
// in a fixed order -- per-thread accumulators over a fixed assignment of pixels -> LDS, the block's pixel rows added in row order -> per-block partials in the
// workspace -> one ordered sum per channel.  No atomic anywhere: two runs give the same bits.
#include "p3d_common.h"

namespace p3d {

using h8 = _Float16 __attribute__((ext_vector_type(8)));

constexpr int HFZ_MAX_K = 2048;         // K / 8 lanes take one pixel; a pixel must fit one block
constexpr int HFZ_MAX_BLOCKS = 512;     // grid.x at the most (2 blocks per CU over the chip): the rows of partials the ordered sum walks
constexpr int HFZ_UNROLL = 4;           // pixel chunks a block has in flight: a grid pass covers gridDim.x * HFZ_UNROLL chunks
constexpr int HFZ_MIN_PIXELS = 16;      // pixels per block at the least, where P allows: the partials (16 B per channel and block, written and read) stay a
                                        // sixth of the tensor traffic (6 B per channel and pixel) at the most

// With K8 = K / 8 lanes per pixel a block takes `rows` = 256 / K8 pixels at a time (a chunk: rows * K halves, contiguous in memory, lane t at halves 8 t .. 8 t + 7);
// lanes rows * K8 .. 255 idle when K8 does not divide 256.  Block b owns the chunks b, b + gridDim.x, ...; a lane therefore always meets the same 8 channels.
// partial[b * K + k] = the block's sum of g over its pixels of channel k.
template <bool RELU>
__global__ __launch_bounds__(256) void hfrozen_mask_kernel(const _Float16* __restrict__ dy, const _Float16* __restrict__ y, _Float16* __restrict__ g,
                                                           double* __restrict__ partial, int P, int K) {
    const int K8 = K >> 3, rows = 256 / K8, active = rows * K8;
    const int t = threadIdx.x;
    const long long chunks = ((long long)P + rows - 1) / rows;
    double acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.0;
    if (t < active) {
        const int r = t / K8;
        for (long long c0 = blockIdx.x; c0 < chunks; c0 += (long long)gridDim.x * HFZ_UNROLL) {
            h8 d[HFZ_UNROLL], m[HFZ_UNROLL];
            bool in[HFZ_UNROLL];
#pragma unroll
            for (int u = 0; u < HFZ_UNROLL; ++u) {
                const long long c = c0 + (long long)u * gridDim.x;
                in[u] = c < chunks && c * rows + r < P;                                   // (the last chunk may hold fewer than `rows` pixels)
                const size_t off = (size_t)c * active * 8 + (size_t)t * 8;                 // = ((c * rows + r) * K8 + lane's group) * 8
                if (in[u]) {
                    d[u] = *reinterpret_cast<const h8*>(dy + off);
                    if constexpr (RELU) m[u] = *reinterpret_cast<const h8*>(y + off);
                }
            }
#pragma unroll
            for (int u = 0; u < HFZ_UNROLL; ++u) {
                if (!in[u]) continue;
                h8 v = d[u];
                if constexpr (RELU) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = (float)m[u][e] > 0.f ? v[e] : (_Float16)0.f;
                    const long long c = c0 + (long long)u * gridDim.x;
                    *reinterpret_cast<h8*>(g + (size_t)c * active * 8 + (size_t)t * 8) = v;
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += (double)(float)v[e];
            }
        }
    }
    __shared__ double sh[256 * 8];          // [row][K]
    if (t < active) {
#pragma unroll
        for (int e = 0; e < 8; ++e) sh[t * 8 + e] = acc[e];
    }
    __syncthreads();
    for (int k = t; k < K; k += 256) {
        double a = 0.0;
        for (int r = 0; r < rows; ++r) a += sh[r * K + k];
        partial[(size_t)blockIdx.x * K + k] = a;
    }
}

// sums[k] = the partials of channel k, added in a fixed order: a block takes 16 channels (128-B runs of a partial row) in 16 slices; slice s adds the partials of
// the blocks [s * per, (s + 1) * per) in order -- eight loads in flight at a time: one thread walking all the rows one load after the other cost 0.25 ms at 1024
// rows, more than the pass itself -- and thread (slice 0, channel) adds the 16 slice sums in order.
__global__ __launch_bounds__(256) void hfrozen_mask_sum_kernel(const double* __restrict__ partial, int blocks, float* __restrict__ sums, int K) {
    const int kl = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int k = blockIdx.x * 16 + kl;
    __shared__ double sh[16][17];
    double a = 0.0;
    if (k < K) {
        const int per = (blocks + 15) >> 4;
        const int b0 = sl * per, b1 = b0 + per < blocks ? b0 + per : blocks;
        for (int b = b0; b < b1; b += 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = b + u < b1 ? partial[(size_t)(b + u) * K + k] : 0.0;
#pragma unroll
            for (int u = 0; u < 8; ++u) a += v[u];
        }
    }
    sh[sl][kl] = a;
    __syncthreads();
    if (sl == 0 && k < K) {
        double t = 0.0;
#pragma unroll
        for (int s = 0; s < 16; ++s) t += sh[s][kl];
        sums[k] = (float)t;
    }
}

static bool hfrozen_shape_ok(int64_t P, int K) { return P > 0 && P < (1ll << 31) && K >= 8 && K <= HFZ_MAX_K && K % 8 == 0; }

static int hfrozen_blocks(int64_t P, int K) {
    const int rows = 256 / (K / 8);
    int64_t blocks = ceil_div(P, rows);
    const int64_t most = P / HFZ_MIN_PIXELS > 1 ? P / HFZ_MIN_PIXELS : 1;
    if (blocks > most) blocks = most;
    if (blocks > HFZ_MAX_BLOCKS) blocks = HFZ_MAX_BLOCKS;
    return (int)blocks;
}

}  // namespace p3d

using namespace p3d;

extern "C" {

size_t p3d_hfrozen_grad_mask_workspace_bytes(int64_t P, int32_t K) {
    return hfrozen_shape_ok(P, K) ? (size_t)hfrozen_blocks(P, K) * K * sizeof(double) : 0;
}

int32_t p3d_hfrozen_grad_mask(const void* dy, const void* y, void* g, float* sums, int64_t P, int32_t K, void* workspace, size_t workspace_bytes, void* stream) {
    P3D_REQUIRE(dy && sums, "hfrozen_grad_mask: null tensor");
    P3D_REQUIRE((y == nullptr) == (g == nullptr), "hfrozen_grad_mask: y and g come together (a ReLU layer) or not at all");
    P3D_REQUIRE(hfrozen_shape_ok(P, K), "hfrozen_grad_mask: P = %lld pixels of K = %d channels: K must be a multiple of 8 in 8 .. %d, P in 1 .. 2^31 - 1",
                (long long)P, K, HFZ_MAX_K);
    P3D_REQUIRE(aligned16(dy, y, g), "hfrozen_grad_mask: dy, y and g must lie on 16-B lines");
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7) || workspace_bytes < p3d_hfrozen_grad_mask_workspace_bytes(P, K)) {
        set_error("hfrozen_grad_mask: workspace missing, not on an 8-B line or too small");
        return P3D_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int blocks = hfrozen_blocks(P, K);
    double* partial = (double*)workspace;
    if (y) hipLaunchKernelGGL(hfrozen_mask_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, (const _Float16*)dy, (const _Float16*)y, (_Float16*)g, partial, (int)P, K);
    else hipLaunchKernelGGL(hfrozen_mask_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, (const _Float16*)dy, (const _Float16*)y, (_Float16*)g, partial, (int)P, K);
    hipLaunchKernelGGL(hfrozen_mask_sum_kernel, dim3((unsigned)ceil_div(K, 16)), dim3(256), 0, st, (const double*)partial, blocks, sums, K);
    return check_launch("hfrozen_grad_mask");
}

}  // extern "C"
