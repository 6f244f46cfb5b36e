// Block-scaled FP8 (MXFP8) inference convolution, gfx950: infer.fold_fp8's forward for every conv between the stems and the heads.
//
// The same implicit GEMM as hconv_gather_kernel<32, 4, true> (p3d_hconv.hip): D[m][n] = sum_k A[m][k] * B[n][k], m = output channel, n = pixel, k = (tap,
// channel), fp16 NHWC activations in and out, the same tap walk and stride / padding / dilation handling, and its EPI 4 epilogue.  What changes is the operand
// format: both operands are MXFP8 (OCP MX v1.0: e4m3fn elements, one E8M0 scale byte per 32 consecutive channels of one tap, p3d_common.h) and the product
// is v_mfma_scale_f32_32x32x64_f8f6f4, which does twice the fp16 work per clock on half the operand bytes.
//   A: the kind-3 fold image of p3d_fx_fold_bn_images (elements [K][RS][Cpad], then scales [K][RS][Cpad / 32]), staged as it is.
//   B: the fp16 activation (times mask_in), quantized in registers on its way into LDS: one thread owns one (pixel, tap, 32-channel block) and quantizes it
//      whole (packed u16 max of the magnitudes, an integer clamp of the magnitudes to 448 X, then v_cvt_scalef32_pk_fp8_f16, which divides by X and rounds
//      to nearest even: bit-equal to the rule over every finite fp16 value and every block exponent of fp16 data, checked on the device; without the clamp it
//      returns NaN from 464 X up).  So the result is that of quantizing the input tensor once, then convolving; a padding pixel is a zero block.
// Tile 128 x 128 pixels x 64 channels (two blocks) per K-step, 4 waves of 64 x 64 (2 x 2 MFMAs of 32 x 32 x 64), double-buffered LDS rows of 64 + 16 bytes.
// Lane maps (pinned with exact integer data): lane l holds row (column) l & 31; of its 32 operand bytes, bytes 16b .. 16b + 15 belong to block b of the K-step,
// and block b's scale is the one lane r + 32 b supplies for row r -- a 32-element block lies in two lanes (its elements 0-15 in lane r, 16-31 in lane r + 32).
//
// The kernel is a template on the form of its input (XMX) and of its result (YMX); <false, false> is the instance described above.  The MX forms are the MXFP8
// activation tensor of include/p3d_hip.h (e4m3 elements [pixel][C], then E8M0 scales [pixel][C / 32]), which one conv writes and the next reads:
//   XMX: B is such a tensor.  A thread copies its block's 32 element bytes and its scale byte into the LDS places the quantizer would have filled: no VALU work on
//        the operand in the K loop.  A padding tap, a pixel past the end and a masked pixel are a zero block with scale byte 0, as the quantizer makes them.
//   YMX: the epilogue quantizes the fp16 results it has formed, by the same statement of the rule (f8_block_consts, f8_convert4).  A thread holds 8 consecutive
//        channels of a pixel, so a 32-channel block lies in the 4 lanes of a quad (lane & ~3): the magnitude maximum is reduced over the quad with two
//        quad_perm DPP moves, every lane converts its 8 values and lane 0 of the quad writes the scale byte.  The fp16 store stays when a pointer is given.
// A block quantized here is the block the consumer's quantizer would have made from the stored fp16 value, so a chain of MX-linked convs is bit-equal to the
// fp16-linked one.
#include <type_traits>

#include "p3d_gather.h"

namespace p3d {

using f8h8 = _Float16 __attribute__((ext_vector_type(8)));
using f8f16x2 = _Float16 __attribute__((ext_vector_type(2)));
using f8s2 = short __attribute__((ext_vector_type(2)));
using f8u2 = unsigned short __attribute__((ext_vector_type(2)));
using f8i8 = int __attribute__((ext_vector_type(8)));
using f8f32x16 = float __attribute__((ext_vector_type(16)));
using f8f32x4 = float __attribute__((ext_vector_type(4)));
using f8i32x4 = int __attribute__((ext_vector_type(4)));

struct F8Params {
    const unsigned char* A;   // weight elements [M][RS][Kc] e4m3
    const unsigned char* As;  // weight scales [M][RS][Kc / 32] E8M0
    const _Float16* B;        // activations NHWC [N][Hb][Wb][Kc]
    _Float16* D;              // result NHWC [N][Hd][Wd][M]
    const float* bias;        // [M] or null
    const float* bmask;       // {0,1} per pixel of B ([N][Hb][Wb]) or null
    const float* dscale;      // per-pixel factor of the result ([N][Hd][Wd]) or null
    const _Float16* res;      // residual NHWC like D, or null
    size_t a_bytes, s_bytes, b_bytes;
    int M, Kc, R, S, stride, pad, dil;
    int N, Hb, Wb, Hd, Wd;
    int tiles_m, relu;
};

// The MX instances' arguments: with XMX, B points to the input's e4m3 elements ([pixel][Kc], b_bytes of them) and Bs to its scale bytes; with YMX, Dq / Ds
// receive the result's elements [pixel][M] and scale bytes [pixel][M / 32], and D may be null.  (A type of its own, so the <false, false> instance keeps its own.)
struct F8MxParams : F8Params {
    const unsigned char* Bs;
    unsigned char* Dq;
    unsigned char* Ds;
    size_t bs_bytes;
};

// The MX rule, stated once for both quantizers.  From a block's magnitude maximum a (fp16 bits; magnitudes order like unsigned integers): the scale byte,
// the clamp bound 448 X as fp16 bits, and X = 2^(e - 8) for the conversion.
__device__ __forceinline__ void f8_block_consts(unsigned a, unsigned& sbyte, f8u2& bound, float& X) {
    const int ex = (int)(a >> 10);
    const int e = ex ? ex - 15 : (31 - __builtin_clz(a | 1u)) - 24;      // floor(log2(amax)); (a == 0: every element is 0 whatever the scale)
    sbyte = a ? (unsigned)(e + 119) : 0u;                       // e - 8 + 127: within [95, 135] for fp16 data
    // |v| clamped to 448 X = 1.75 * 2^e (as fp16 bits; below 2^-22 no element can reach it)
    const unsigned bb = e >= -14 ? (unsigned)(((e + 15) << 10) | 0x300) : (e >= -22 ? 7u << (e + 22) : 0x7bffu);
    bound = f8u2{(unsigned short)bb, (unsigned short)bb};
    X = __builtin_bit_cast(float, (unsigned)(e + 119) << 23);   // 2^(e - 8)
}

// four fp16 values (two words) of a block -> their four e4m3 bytes
__device__ __forceinline__ unsigned f8_convert4(unsigned w0, unsigned w1, f8u2 bound, float X) {
    const unsigned c0 = (w0 & 0x80008000u) | __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(f8u2, w0 & 0x7fff7fffu), bound));
    const unsigned c1 = (w1 & 0x80008000u) | __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(f8u2, w1 & 0x7fff7fffu), bound));
    f8s2 o = {0, 0};
    o = __builtin_amdgcn_cvt_scalef32_pk_fp8_f16(o, __builtin_bit_cast(f8f16x2, c0), X, false);      // bytes 0, 1
    o = __builtin_amdgcn_cvt_scalef32_pk_fp8_f16(o, __builtin_bit_cast(f8f16x2, c1), X, true);       // bytes 2, 3
    return __builtin_bit_cast(unsigned, o);
}

// the packed magnitude maximum of N words of fp16 pairs, as fp16 bits
template <int N>
__device__ __forceinline__ unsigned f8_amax(const unsigned (&w)[N]) {
    f8u2 mx = {0, 0};
#pragma unroll
    for (int i = 0; i < N; ++i) mx = __builtin_elementwise_max(mx, __builtin_bit_cast(f8u2, w[i] & 0x7fff7fffu));
    return mx[0] > mx[1] ? mx[0] : mx[1];
}

// 32 fp16 values (16 words) -> 32 e4m3 bytes (8 words) + the scale byte, by the MX rule
__device__ __forceinline__ void f8_quantize32(const unsigned (&w)[16], unsigned (&q)[8], unsigned& sbyte) {
    f8u2 bound;
    float X;
    f8_block_consts(f8_amax(w), sbyte, bound, X);
#pragma unroll
    for (int d = 0; d < 8; ++d) q[d] = f8_convert4(w[2 * d], w[2 * d + 1], bound, X);
}

// Occupancy: the MX-fed fetch holds 8 VGPRs of B where the fp16-fed one holds 16 and the quantizer's temporaries, so the XMX instances fit 3 waves per SIMD
// (144 VGPRs, no scratch; 3 blocks of 41 984 B LDS per CU) when asked to; left alone the compiler takes 180 and the K loop, 4 MFMAs per wave behind a barrier,
// has nothing to overlap its loads with (profiles/eval_folded_fp8_resident.md).  The fp16-fed instances keep the default, and <false, false> its ISA.
template <bool XMX, bool YMX>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(XMX ? 3 : 1))) void f8conv_gather_kernel(std::conditional_t<XMX || YMX, F8MxParams, F8Params> p) {
    constexpr int BM = 128, BN = 128;
    constexpr int ROWB = 80;                    // 64 e4m3 bytes (two blocks) + 16: the 16 lanes of a b128 read phase cover all 64 banks
    constexpr int OPB = BM * ROWB;              // one operand's rows per buffer
    constexpr int SCB = 2 * 128;                // one operand's scale bytes per buffer: [block][row]
    constexpr int BUF = 2 * OPB + 2 * SCB;
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * BUF];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int ncols = p.N * p.Hd * p.Wd;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int tile_m = bid % p.tiles_m, tile_n = bid / p.tiles_m;
    const int n0 = tile_n * BN, m0 = tile_m * BM;
    if (n0 >= ncols) return;
    const int RS = p.R * p.S, CB = p.Kc >> 5;
    const int nblk = RS * CB;                   // 32-channel blocks along the reduction
    const int nk = (nblk + 1) >> 1;

    const f8i32x4 rA = hmake_rsrc(p.A, p.a_bytes), rB = hmake_rsrc(p.B, p.b_bytes);
    const __amdgpu_buffer_rsrc_t rSb = __builtin_amdgcn_make_buffer_rsrc((void*)p.As, 0, (int)p.s_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rBs = [&] {       // the input's scale bytes (XMX)
        if constexpr (XMX) return __builtin_amdgcn_make_buffer_rsrc((void*)p.Bs, 0, (int)p.bs_bytes, 0x00020000);
        else return __builtin_amdgcn_make_buffer_rsrc(nullptr, 0, 0, 0x00020000);
    }();
    const __amdgpu_buffer_rsrc_t rMask = __builtin_amdgcn_make_buffer_rsrc((void*)p.bmask, 0, p.bmask ? p.N * p.Hb * p.Wb * 4 : 0, 0x00020000);

    // ---- this thread: weight row / pixel `row` of the tile, block `hb` (0 / 1) of every K-step ----
    const int row = t >> 1, hb = t & 1;
    const bool narrow = p.M <= 64;              // at most 64 result channels: every wave takes 32 of the 64 live rows (as hconv_gather_kernel)
    const int m = m0 + row;
    const int a_row = (m < p.M && (!narrow || row < 64)) ? m * RS : -1;
    const int n = n0 + row;
    int b_img = -1, b_h = 0, b_w = 0;
    if (n < ncols) {
        const int img = n / (p.Hd * p.Wd), rem = n - img * (p.Hd * p.Wd);
        const int ii = rem / p.Wd, jj = rem - ii * p.Wd;
        b_img = img * p.Hb * p.Wb; b_h = p.stride * ii - p.pad; b_w = p.stride * jj - p.pad;
    }
    int q = hb;                                 // this thread's block of the current fetch, its tap and channel block
    int tap = q / CB, cb = q - tap * CB;
    int ir = tap / p.S, is = tap - ir * p.S;

    f8f32x4 ra[2], rb[XMX ? 2 : 4];
    unsigned sa = 0, sb = 0;
    float rm = 1.f;
    auto fetch = [&]() {
        const bool live = q < nblk;
        const bool aok = live && a_row >= 0;
        const int aoff = ((a_row + tap) * CB + cb) * 32;
        ra[0] = hbuf_load16(rA, aok ? aoff : HOOB, 0, 0);
        ra[1] = hbuf_load16(rA, aok ? aoff + 16 : HOOB, 0, 0);
        sa = __builtin_amdgcn_raw_buffer_load_b8(rSb, aok ? (a_row + tap) * CB + cb : HOOB, 0, 0);
        const int hh = b_h + p.dil * ir, ww = b_w + p.dil * is;
        const bool ok = live && b_img >= 0 && (unsigned)hh < (unsigned)p.Hb && (unsigned)ww < (unsigned)p.Wb;
        const int pix = b_img + hh * p.Wb + ww;
        if constexpr (XMX) {                    // the block as it is: 32 element bytes and the scale byte (zeros outside the map, past the end, in a dead half)
            const int boff = pix * p.Kc + cb * 32;
            rb[0] = hbuf_load16(rB, ok ? boff : HOOB, 0, 0);
            rb[1] = hbuf_load16(rB, ok ? boff + 16 : HOOB, 0, 0);
            sb = __builtin_amdgcn_raw_buffer_load_b8(rBs, ok ? pix * CB + cb : HOOB, 0, 0);
        } else {
            const int boff = (pix * p.Kc + cb * 32) * 2;
#pragma unroll
            for (int i = 0; i < 4; ++i) rb[i] = hbuf_load16(rB, ok ? boff + 16 * i : HOOB, 0, 0);
        }
        if (p.bmask) rm = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rMask, ok ? pix * 4 : HOOB, 0, 0));
        q += 2; cb += 2;                        // the next K-step's block
        while (cb >= CB) {
            cb -= CB; ++tap;
            if (++is == p.S) { is = 0; ++ir; }
        }
    };
    auto stage = [&](int buf) {
        unsigned char* base = smem + buf * BUF;
        // A: row `row`, block hb at byte 32 hb of the row; scale at [hb][row]
        *reinterpret_cast<f8f32x4*>(base + row * ROWB + hb * 32) = ra[0];
        *reinterpret_cast<f8f32x4*>(base + row * ROWB + hb * 32 + 16) = ra[1];
        base[2 * OPB + hb * 128 + row] = (unsigned char)sa;
        if constexpr (XMX) {
            if (p.bmask && rm == 0.f) {                                // q(x * mask) with a {0,1} mask: a dropped pixel is a zero block
                rb[0] = rb[1] = f8f32x4{0.f, 0.f, 0.f, 0.f};
                sb = 0u;
            }
            *reinterpret_cast<f8f32x4*>(base + OPB + row * ROWB + hb * 32) = rb[0];
            *reinterpret_cast<f8f32x4*>(base + OPB + row * ROWB + hb * 32 + 16) = rb[1];
            base[2 * OPB + SCB + hb * 128 + row] = (unsigned char)sb;
        } else {
            unsigned w[16], qq[8], sbyte;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                // The 16 B hold eight fp16 values, not four floats: reinterpret the whole vector as integers, then take its words.  (Taking float elements
                // one by one and bit-casting each compiled, with hipcc 7.2, to word 0 repeated four times; the integer view keeps every word.)
                const f8i32x4 v = __builtin_bit_cast(f8i32x4, rb[i]);
#pragma unroll
                for (int e = 0; e < 4; ++e) w[4 * i + e] = (unsigned)v[e];
            }
            if (p.bmask && rm == 0.f) {                                // x * mask with a {0,1} mask: keep or drop the pixel
#pragma unroll
                for (int i = 0; i < 16; ++i) w[i] = 0u;
            }
            f8_quantize32(w, qq, sbyte);
            *reinterpret_cast<f8i32x4*>(base + OPB + row * ROWB + hb * 32) = f8i32x4{(int)qq[0], (int)qq[1], (int)qq[2], (int)qq[3]};
            *reinterpret_cast<f8i32x4*>(base + OPB + row * ROWB + hb * 32 + 16) = f8i32x4{(int)qq[4], (int)qq[5], (int)qq[6], (int)qq[7]};
            base[2 * OPB + SCB + hb * 128 + row] = (unsigned char)sbyte;
        }
    };

    f8f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const int fr = lane & 31, fh = lane >> 5;
    const int rbase = narrow ? wm * 32 : wm * 64, na = narrow ? 1 : 2;
    if (nk > 0) { fetch(); stage(0); if (nk > 1) fetch(); }
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const unsigned char* base = smem + (kt & 1) * BUF;
        f8i8 af[2], bf[2];
        int as[2], bs[2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
            if (a < na) {
                const unsigned char* rd = base + (rbase + a * 32 + fr) * ROWB + fh * 16;
                const f8i32x4 lo = *reinterpret_cast<const f8i32x4*>(rd), hi = *reinterpret_cast<const f8i32x4*>(rd + 32);
                af[a] = f8i8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                as[a] = base[2 * OPB + fh * 128 + rbase + a * 32 + fr];
            }
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const unsigned char* rd = base + OPB + (wn * 64 + b * 32 + fr) * ROWB + fh * 16;
            const f8i32x4 lo = *reinterpret_cast<const f8i32x4*>(rd), hi = *reinterpret_cast<const f8i32x4*>(rd + 32);
            bf[b] = f8i8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            bs[b] = base[2 * OPB + SCB + fh * 128 + wn * 64 + b * 32 + fr];
        }
        acc[0][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af[0], bf[0], acc[0][0], 0, 0, 0, as[0], 0, bs[0]);
        // the next step's operands go to LDS (the B quantization on the VALU) and the loads of the step after it are issued behind the first MFMA
        __builtin_amdgcn_sched_barrier(0);
        if (kt + 1 < nk) stage((kt & 1) ^ 1);
        if (kt + 2 < nk) fetch();
        __builtin_amdgcn_sched_barrier(0);
        acc[0][1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af[0], bf[1], acc[0][1], 0, 0, 0, as[0], 0, bs[1]);
        if (na > 1) {
            acc[1][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af[1], bf[0], acc[1][0], 0, 0, 0, as[1], 0, bs[0]);
            acc[1][1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af[1], bf[1], acc[1][1], 0, 0, 0, as[1], 0, bs[1]);
        }
        __syncthreads();
    }

    // ---- epilogue: hconv_gather_kernel's EPI 4, y = fp16(relu?(acc * dscale + bias + res)) rounded once; the fp32 accumulators go through LDS in two
    //      passes of 64 channels (128 pixels x 64 channels x 4 B + 16 B per row = 34 KB of the operand buffers), the residual is read and the result
    //      written in 16-B runs.  C/D layout: col = lane & 31 (pixel), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (channel) ----
    constexpr int EPITCH = 272;
    static_assert(128 * EPITCH <= 2 * BUF, "the staging tile lives in the operand buffers");
    float* T = reinterpret_cast<float*>(smem);  // (the K loop ended on a barrier)
    float dsc[2] = {1.f, 1.f};
    if (p.dscale) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int nn = n0 + wn * 64 + b * 32 + fr;
            if (nn < ncols) dsc[b] = p.dscale[nn];                 // (NHWC pixel order: the result's pixel index is n)
        }
    }
    const int cc = t & 7, pr = t >> 3;
    const int npass = (narrow || m0 + 64 >= p.M) ? 1 : 2;
    for (int h = 0; h < npass; ++h) {
        if (h > 0) __syncthreads();
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int rb0 = rbase + a * 32;
            if (a >= na || (rb0 >> 6) != h) continue;
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f8f32x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = acc[a][b][4 * g + e] * dsc[b];
                    *reinterpret_cast<f8f32x4*>(reinterpret_cast<unsigned char*>(T) + (wn * 64 + b * 32 + fr) * EPITCH + (rb0 - 64 * h + 8 * g + 4 * fh) * 4) = o;
                }
        }
        __syncthreads();
        const int ch = m0 + 64 * h + cc * 8;
        if (ch >= p.M) continue;                                    // (M % 8 == 0)
        float bias[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) bias[e] = p.bias ? p.bias[ch + e] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int pl = pr + 32 * i, nn = n0 + pl;
            if (nn >= ncols) continue;
            const unsigned char* src = reinterpret_cast<const unsigned char*>(T) + pl * EPITCH + cc * 32;
            const f8f32x4 v0 = *reinterpret_cast<const f8f32x4*>(src), v1 = *reinterpret_cast<const f8f32x4*>(src + 16);
            const size_t off = (size_t)nn * p.M + ch;
            f8h8 r = {};
            if (p.res) r = *reinterpret_cast<const f8h8*>(p.res + off);
            f8h8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float y = (e < 4 ? v0[e] : v1[e - 4]) + bias[e];
                if (p.res) y += (float)r[e];
                if (p.relu) y = fmaxf(y, 0.f);
                o[e] = (_Float16)y;
            }
            if constexpr (YMX) {
                // The block of these 8 channels lies in this lane's quad, and the quad shares both tests above (M % 32 == 0, one pixel), so its four lanes
                // are here together: the quad_perm moves read no lane that has left the loop.
                const f8i32x4 ov = __builtin_bit_cast(f8i32x4, o);
                const unsigned ow[4] = {(unsigned)ov[0], (unsigned)ov[1], (unsigned)ov[2], (unsigned)ov[3]};
                int a = (int)f8_amax(ow);
                a = max(a, __builtin_amdgcn_update_dpp(0, a, 0xb1, 0xf, 0xf, true));       // quad_perm [1, 0, 3, 2]
                a = max(a, __builtin_amdgcn_update_dpp(0, a, 0x4e, 0xf, 0xf, true));       // quad_perm [2, 3, 0, 1]
                unsigned sbyte;
                f8u2 bound;
                float X;
                f8_block_consts((unsigned)a, sbyte, bound, X);
                *reinterpret_cast<uint2*>(p.Dq + off) = uint2{f8_convert4(ow[0], ow[1], bound, X), f8_convert4(ow[2], ow[3], bound, X)};
                if ((cc & 3) == 0) p.Ds[(size_t)nn * (p.M >> 5) + (ch >> 5)] = (unsigned char)sbyte;
                if (p.D) *reinterpret_cast<f8h8*>(p.D + off) = o;
            } else {
                *reinterpret_cast<f8h8*>(p.D + off) = o;
            }
        }
    }
}

static int32_t f8validate(const p3d_conv_desc* d, const char* what) {
    P3D_REQUIRE(d, "%s: null descriptor", what);
    P3D_REQUIRE(d->N > 0 && d->C > 0 && d->H > 0 && d->W > 0 && d->K > 0 && d->R > 0 && d->S > 0, "%s: bad shape", what);
    P3D_REQUIRE(d->stride >= 1 && d->pad >= 0 && d->dil >= 1, "%s: stride %d / pad %d / dilation %d unsupported", what, d->stride, d->pad, d->dil);
    P3D_REQUIRE(d->C % 32 == 0, "%s: the input channel count must be a multiple of 32, one MX block per 32 channels (C=%d)", what, d->C);
    P3D_REQUIRE(d->K % 8 == 0, "%s: the output channel count must be a multiple of 8 (K=%d)", what, d->K);
    P3D_REQUIRE(!d->accumulate, "%s: accumulate is not supported", what);
    P3D_REQUIRE(d->c_total == d->C && d->c_offset == 0, "%s: channel windows are not supported", what);
    const int Ho = (d->H + 2 * d->pad - d->dil * (d->R - 1) - 1) / d->stride + 1, Wo = (d->W + 2 * d->pad - d->dil * (d->S - 1) - 1) / d->stride + 1;
    P3D_REQUIRE(Ho >= 1 && Wo >= 1 && Ho == d->Ho && Wo == d->Wo, "%s: Ho/Wo %dx%d do not match the geometry (%dx%d)", what, d->Ho, d->Wo, Ho, Wo);
    P3D_REQUIRE((int64_t)d->N * d->H * d->W * d->C * 2 < (1ll << 31) && (int64_t)d->N * d->Ho * d->Wo * d->K * 2 < (1ll << 31) &&
                (int64_t)d->K * d->R * d->S * d->C < (1ll << 30), "%s: a tensor exceeds the 2 GiB buffer window", what);
    return P3D_OK;
}

static size_t f8act_bytes(int64_t pixels, int32_t C) {
    if (pixels <= 0 || C <= 0 || C % 32 != 0) return 0;
    return (size_t)pixels * C + (size_t)pixels * (C / 32);
}

static int32_t f8validate_mx(const p3d_conv_desc* d, int32_t x_is_mx, int32_t y_mx, const char* what) {
    if (int32_t e = f8validate(d, what)) return e;
    P3D_REQUIRE(!y_mx || d->K % 32 == 0, "%s: an MX result needs an output channel count that is a multiple of 32, one MX block per 32 channels (K=%d)", what, d->K);
    P3D_REQUIRE((!x_is_mx || f8act_bytes((int64_t)d->N * d->H * d->W, d->C) < (1ull << 31)) &&
                (!y_mx || f8act_bytes((int64_t)d->N * d->Ho * d->Wo, d->K) < (1ull << 31)), "%s: an MX tensor exceeds the 2 GiB buffer window", what);
    return P3D_OK;
}

static void f8fill(F8Params& p, const p3d_conv_desc* d, const void* w_mx, const float* bias, const float* mask_in, const float* mult, const void* res_nhwc,
                   int32_t relu) {
    const size_t elems = (size_t)d->K * d->R * d->S * d->C;
    p.A = (const unsigned char*)w_mx; p.As = p.A + elems;
    p.bias = bias; p.bmask = mask_in; p.dscale = mult; p.res = (const _Float16*)res_nhwc;
    p.a_bytes = elems; p.s_bytes = elems / 32;
    p.M = d->K; p.Kc = d->C; p.R = d->R; p.S = d->S; p.stride = d->stride; p.pad = d->pad; p.dil = d->dil;
    p.N = d->N; p.Hb = d->H; p.Wb = d->W; p.Hd = d->Ho; p.Wd = d->Wo;
    p.tiles_m = (int)ceil_div(d->K, 128); p.relu = relu != 0;
}

template <bool XMX, bool YMX, class P>
static void f8launch(const P& p, const p3d_conv_desc* d, void* stream) {
    const int64_t tiles_n = ceil_div((int64_t)d->N * d->Ho * d->Wo, 128);
    hipLaunchKernelGGL((f8conv_gather_kernel<XMX, YMX>), dim3((unsigned)(p.tiles_m * tiles_n)), dim3(256), 0, (hipStream_t)stream, p);
}

}  // namespace p3d

using namespace p3d;

extern "C" {

int32_t p3d_f8conv2d_fwd_infer_supported(const p3d_conv_desc* d) {
    return f8validate(d, "f8conv2d_fwd_infer") == P3D_OK ? 1 : 0;
}

size_t p3d_f8conv2d_weight_bytes(int32_t K, int32_t C, int32_t RS) {
    if (K <= 0 || C <= 0 || RS <= 0 || C % 32 != 0) return 0;
    return (size_t)K * RS * C + (size_t)K * RS * (C / 32);
}

int32_t p3d_f8conv2d_fwd_infer(const p3d_conv_desc* d, const void* x_nhwc, const void* w_mx, const float* bias, const float* mask_in, const float* mult,
                               const void* res_nhwc, int32_t relu, void* y_nhwc, void* stream) {
    if (int32_t e = f8validate(d, "f8conv2d_fwd_infer")) return e;
    P3D_REQUIRE(x_nhwc && w_mx && y_nhwc, "f8conv2d_fwd_infer: null tensor");
    F8Params p = {};
    f8fill(p, d, w_mx, bias, mask_in, mult, res_nhwc, relu);
    p.B = (const _Float16*)x_nhwc; p.D = (_Float16*)y_nhwc; p.b_bytes = (size_t)d->N * d->H * d->W * d->C * 2;
    f8launch<false, false>(p, d, stream);
    return check_launch("f8conv2d_fwd_infer");
}

size_t p3d_f8act_bytes(int64_t pixels, int32_t C) {
    return f8act_bytes(pixels, C);
}

int32_t p3d_f8conv2d_fwd_infer_mx_supported(const p3d_conv_desc* d, int32_t x_is_mx, int32_t y_mx) {
    return f8validate_mx(d, x_is_mx, y_mx, "f8conv2d_fwd_infer_mx") == P3D_OK ? 1 : 0;
}

int32_t p3d_f8conv2d_fwd_infer_mx(const p3d_conv_desc* d, const void* x_nhwc, const void* x_mx, const void* w_mx, const float* bias, const float* mask_in,
                                  const float* mult, const void* res_nhwc, int32_t relu, void* y_nhwc, void* y_mx, void* stream) {
    if (int32_t e = f8validate_mx(d, x_mx != nullptr, y_mx != nullptr, "f8conv2d_fwd_infer_mx")) return e;
    P3D_REQUIRE((x_nhwc != nullptr) != (x_mx != nullptr), "f8conv2d_fwd_infer_mx: give the input as fp16 or as MX, one of the two");
    P3D_REQUIRE(y_nhwc || y_mx, "f8conv2d_fwd_infer_mx: no result tensor");
    P3D_REQUIRE(w_mx, "f8conv2d_fwd_infer_mx: null tensor");
    const size_t pix_in = (size_t)d->N * d->H * d->W, pix_out = (size_t)d->N * d->Ho * d->Wo;
    if (!x_mx && !y_mx) {                       // fp16 in, fp16 out: the instance of p3d_f8conv2d_fwd_infer
        F8Params p = {};
        f8fill(p, d, w_mx, bias, mask_in, mult, res_nhwc, relu);
        p.B = (const _Float16*)x_nhwc; p.D = (_Float16*)y_nhwc; p.b_bytes = pix_in * d->C * 2;
        f8launch<false, false>(p, d, stream);
        return check_launch("f8conv2d_fwd_infer_mx");
    }
    F8MxParams p = {};
    f8fill(p, d, w_mx, bias, mask_in, mult, res_nhwc, relu);
    p.D = (_Float16*)y_nhwc;
    if (x_mx) {
        p.B = (const _Float16*)x_mx; p.b_bytes = pix_in * d->C;
        p.Bs = (const unsigned char*)x_mx + p.b_bytes; p.bs_bytes = pix_in * (d->C / 32);
    } else {
        p.B = (const _Float16*)x_nhwc; p.b_bytes = pix_in * d->C * 2;
    }
    if (y_mx) { p.Dq = (unsigned char*)y_mx; p.Ds = p.Dq + pix_out * d->K; }
    if (x_mx && y_mx) f8launch<true, true>(p, d, stream);
    else if (x_mx) f8launch<true, false>(p, d, stream);
    else f8launch<false, true>(p, d, stream);
    return check_launch("f8conv2d_fwd_infer_mx");
}

}  // extern "C"
