// Shared helpers for libp3d_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/p3d_hip.h"

namespace p3d {

void set_error(const char* fmt, ...);
// for an entry point that shares its launch path with others: a P3D_EWORKSPACE text written there gets the entry's own name in front ("entry: path: ...")
int32_t name_entry(const char* entry, int32_t rc);

inline int32_t check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return P3D_ELAUNCH;
    }
    return P3D_OK;
}

#define P3D_REQUIRE(cond, ...)              \
    do {                                    \
        if (!(cond)) {                      \
            ::p3d::set_error(__VA_ARGS__);  \
            return P3D_EINVAL;              \
        }                                   \
    } while (0)

constexpr int WAVE = 64;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
// every pointer on a 16-B line (NULL counts as aligned)
template <typename... P> inline bool aligned16(const P*... p) { return ((reinterpret_cast<uintptr_t>(p) | ...) & 15) == 0; }

// Taps r in [0,R) with (par + pad - r*dil) % stride == 0 form an arithmetic progression r0 + step*ir; the output
// coordinate they read is ho = i + off0 - ir*offstep for the class-grid row i (hi = par + stride*i).  The parity classes of a strided data gradient, one axis at a
// time: the fp32-MFMA kernel (p3d_conv.hip) and the x3 kernels (fx_conv_dgrad, p3d_fx.hip: hoff = off0, hstep = -offstep) take theirs from here.
inline void fill_class(int par, int R, int stride, int pad, int dil, int* r0, int* step, int* n, int* off0, int* offstep) {
    *r0 = 0; *step = 1; *n = 0; *off0 = 0; *offstep = 0;
    int first = -1, second = -1;
    for (int r = 0; r < R; ++r) {
        const int t = par + pad - r * dil;
        if (((t % stride) + stride) % stride != 0) continue;
        if (first < 0) first = r;
        else if (second < 0) second = r;
        ++*n;
    }
    if (first < 0) return;
    *r0 = first;
    *step = second < 0 ? 1 : second - first;
    const int t0 = par + pad - first * dil;                 // divisible by stride
    *off0 = t0 >= 0 ? t0 / stride : -((-t0) / stride);
    *offstep = (*step * dil) / stride;                        // (step*dil) is a multiple of stride by construction
}

// MXFP8 (OCP MX v1.0, e4m3fn elements, 32-element blocks) -- the one rule of the fold (p3d_fx.hip kind 3) and the fp8 convolution (p3d_f8conv.hip):
// e = floor(log2(amax)) from the exponent bits, scale byte E8M0 = clamp(e - 8 + 127, 0, 254) (8: the exponent of 448), X = 2^(byte - 127),
// q = e4m3fn(RNE(clamp(v / X, -448, 448))), subnormals kept; amax == 0: byte 0 and every element 0.
__device__ __forceinline__ int mx_scale_byte_f32(float amax) {
    const unsigned u = __builtin_bit_cast(unsigned, amax) & 0x7fffffffu;
    if (u == 0) return 0;
    const int ex = (int)(u >> 23);
    const int e = ex ? ex - 127 : (31 - __builtin_clz(u)) - 149;
    const int b = e + 119;
    return b < 0 ? 0 : (b > 254 ? 254 : b);
}
// fp32 -> e4m3fn, round to nearest even, |x| clamped to 448 first (x finite; a NaN gives +-448)
__device__ __forceinline__ unsigned f32_to_e4m3(float x) {
    const unsigned sign = (__builtin_bit_cast(unsigned, x) >> 24) & 0x80u;
    const float a = fabsf(x);
    if (!(a < 448.f)) return sign | 0x7eu;
    if (a < 0.015625f) return sign | (unsigned)(int)rintf(a * 512.f);          // subnormal range: multiples of 2^-9 (8 * 2^-9 is the encoding of 2^-6)
    const unsigned ua = __builtin_bit_cast(unsigned, a);
    return sign | ((((ua + 0x7ffffu + ((ua >> 20) & 1u)) >> 20) - (120u << 3)) & 0x7fu);      // 3 mantissa bits, RNE; exponent bias 127 -> 7
}

}  // namespace p3d
