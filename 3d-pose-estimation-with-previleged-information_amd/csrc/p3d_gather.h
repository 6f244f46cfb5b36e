// Helpers shared by the implicit-GEMM gather kernels over NHWC fp16 activations: hconv_gather_kernel (p3d_hconv.hip) and f8conv_gather_kernel (p3d_f8conv.hip).
#pragma once
#include "p3d_common.h"

namespace p3d {

using gather_f32x4 = float __attribute__((ext_vector_type(4)));
using gather_i32x4 = int __attribute__((ext_vector_type(4)));

// 16-B buffer load, bound by intrinsic name (see p3d_conv.hip: the b128 builtin of this compiler lowers to a dword load)
__device__ gather_f32x4 hbuf_load16(gather_i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.v4f32");

__device__ __forceinline__ gather_i32x4 hmake_rsrc(const void* base, size_t bytes) {
    const unsigned n = bytes < 0x7ffffff0ull ? (unsigned)bytes : 0x7ffffff0u;
    const uint64_t a = reinterpret_cast<uint64_t>(base);
    gather_i32x4 r;
    r[0] = (int)(unsigned)a; r[1] = (int)((a >> 32) & 0xffff); r[2] = (int)n; r[3] = 0x00020000;
    return r;
}

constexpr int HOOB = (int)0x80000000;      // a voffset with this bit set is past any buffer: the load returns 0

// blocks of one XCD take consecutive tiles (the dispatcher deals blocks round-robin over the 8 XCDs)
__device__ __forceinline__ int xcd_remap(int b, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = b & 7, idx = b >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

}  // namespace p3d
