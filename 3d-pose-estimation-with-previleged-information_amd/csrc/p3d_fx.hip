// Convolution forward / data gradient / weight gradient as exact-fp32 implicit GEMMs on the bf16 matrix pipe of gfx950
// (depthnet.py:40-56,96-116 and the twins in resnet.py / fusionnet.py; partial_conv.py:32-57 for the masked instances).
//
// Arithmetic ("x3"): every fp32 operand value is cut into three bf16 pieces, each the bf16 of what the previous ones leave (x = hi + mid + lo exactly).
// Per K = 16 step the six piece products that can exceed 2^-24 |a b| (hi*hi, hi*mid, mid*hi, mid*mid, hi*lo, lo*hi) are issued on
// v_mfma_f32_32x32x16_bf16 with fp32 accumulation, smallest first: fp32-grade results (measured error <= the fp32-MFMA kernel's) at 192 matrix-pipe
// cycles per 32x32x16 block instead of the 512 of v_mfma_f32_32x32x2_f32.
//
// Where the split happens.  Weights: once per optimizer step, into "weight images" (fx_weight_images_kernel) that hold, per (filter tap, 128-row tile,
// K step), the 12 KB the kernel's LDS buffer takes.  Activations and gradients: either in the kernel, on the way from fp32 NCHW into LDS (AMODE 0: block
// inputs, per-layer entry points), or by the pass that PRODUCES the tensor (AMODE 1 / AIMG / BIMG: fx_act_image_kernel, run by the residual-block
// executor where it applies BatchNorm + ReLU or the BatchNorm-backward map anyway), into an "activation image": three bf16 planes laid out
// [n][channel / 16][h][w][16 channels], so that any (pixel, 16-channel K step) is one 32-B row per plane whatever the filter tap, stride or dilation.
// A kernel fed by images does no arithmetic on its operands: 16-B copies into LDS, fragment reads, MFMAs.
// Row images (ROWS instances, the dense residual blocks): the same rows holding the fp32 value itself, [n][channel / 16][h][w][16] floats -- 4 B per element written and
// read instead of 6.  The layout is what makes the fetch cheap; the split is done by the consumer between its fetch registers and LDS (fx_split_row8), under MFMAs.
//
// GEMM view (the pixel index is the contiguous one of the fp32 tensors):
//   FWD    y [n][m][oh][ow]  = sum_tap sum_c  W[m][c][tap] * x [n][c][oh*s - pad + r*dil][ow*s - pad + q*dil]
//   DGRAD  dx[n][m][ih][iw]  = sum_tap sum_k  W[k][m][tap] * dy[n][k][(ih + pad - r*dil)/s][(iw + pad - q*dil)/s]      (per stride^2 parity class)
//   WGRAD  dw[k][c][tap]     = sum_n sum_p    dy[n][k][p]  * x [n][c][p at tap]                                       (split over (n, p) into slabs)
// One block = 256 threads = 4 waves computes a 128 (channels) x 128 (pixels) tile; a wave owns 64 x 64 as 2 x 2 MFMA tiles.  The MFMA is
// issued with the PIXEL operand in the A slot and the CHANNEL operand in the B slot, so in the accumulator a lane is an output channel and
// its registers are pixels: four consecutive registers are four consecutive pixels (one 16-B store), and everything that is per output
// channel -- bias, the BatchNorm batch statistics of the result (EPI 1), the sums of the BatchNorm backward (EPI 2) -- is per lane, i.e. plain register
// adds followed by one cross-lane step, not a 32-lane reduction per row.
#include <type_traits>
#include <mutex>
#include "p3d_common.h"
#include "p3d_fx.h"

namespace p3d {

using bf8 = __bf16 __attribute__((ext_vector_type(8)));
using f32x16 = float __attribute__((ext_vector_type(16)));
using f32x4 = float __attribute__((ext_vector_type(4)));
using f32x2 = float __attribute__((ext_vector_type(2)));
using u32x2 = unsigned __attribute__((ext_vector_type(2)));
using s4t = short __attribute__((ext_vector_type(4)));
using s8v = short __attribute__((ext_vector_type(8)));
using i32x4 = int __attribute__((ext_vector_type(4)));

constexpr int FX_BM = 128, FX_BN = 128, FX_BK = 16;
constexpr int FX_PIECE = 128 * FX_BK * 2;          // bytes of one bf16 piece of one operand tile (128 rows or columns x 16 k)

// fp32 -> bf16 pieces.  Each piece is the round-to-nearest-even bf16 of what is left (v_cvt_pk_bf16_f32 converts and packs two values per instruction):
// hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid).  Both subtractions are exact in fp32 and the last remainder has at most 8 significant bits,
// so hi + mid + lo == x exactly.
using bf16x2 = __bf16 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned fx_pack2(float a, float b) {
    const bf16x2 h = __builtin_convertvector(f32x2{a, b}, bf16x2);
    return __builtin_bit_cast(unsigned, h);
}
__device__ __forceinline__ void fx_split2(float x0, float x1, unsigned& hp, unsigned& mp, unsigned& lp) {
    hp = fx_pack2(x0, x1);
    const float r0 = x0 - __builtin_bit_cast(float, hp << 16), r1 = x1 - __builtin_bit_cast(float, hp & 0xFFFF0000u);
    mp = fx_pack2(r0, r1);
    const float s0 = r0 - __builtin_bit_cast(float, mp << 16), s1 = r1 - __builtin_bit_cast(float, mp & 0xFFFF0000u);
    lp = fx_pack2(s0, s1);
}
// fp32 x4 -> three bf16 x4 pieces, written as 8-B chunks FX_PIECE apart
__device__ __forceinline__ void fx_split_store(unsigned char* base, const f32x4 v) {
    unsigned hp[2], mp[2], lp[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) fx_split2(v[2 * q], v[2 * q + 1], hp[q], mp[q], lp[q]);
    *reinterpret_cast<u32x2*>(base) = u32x2{hp[0], hp[1]};
    *reinterpret_cast<u32x2*>(base + FX_PIECE) = u32x2{mp[0], mp[1]};
    *reinterpret_cast<u32x2*>(base + 2 * FX_PIECE) = u32x2{lp[0], lp[1]};
}
// Row images (ROWS instances): half a 64-B row of an fp32 row image -- eight consecutive channels of one pixel, fetched as two 16-B groups -- cut into the three
// 16-B chunks the same position of a three-plane activation image holds: the channel pairs and the function are those of fx_act_image_kernel, so the chunks are
// bit for bit what that pass would have stored
__device__ __forceinline__ void fx_split_row8(const f32x4 a, const f32x4 b, i32x4 (&out)[3]) {
    unsigned hp[4], mp[4], lp[4];
    fx_split2(a[0], a[1], hp[0], mp[0], lp[0]);
    fx_split2(a[2], a[3], hp[1], mp[1], lp[1]);
    fx_split2(b[0], b[1], hp[2], mp[2], lp[2]);
    fx_split2(b[2], b[3], hp[3], mp[3], lp[3]);
    out[0] = i32x4{(int)hp[0], (int)hp[1], (int)hp[2], (int)hp[3]};
    out[1] = i32x4{(int)mp[0], (int)mp[1], (int)mp[2], (int)mp[3]};
    out[2] = i32x4{(int)lp[0], (int)lp[1], (int)lp[2], (int)lp[3]};
}

// LDS images of one piece of one operand tile:
//  "tr": rows are the reduction index, 16 rows x 128 bf16 columns, 256-B rows, the 16-B chunks of a row XOR-swizzled; MFMA fragments (8 consecutive k of one
//  column per lane) come out of ds_read_b64_tr_b16 (two per fragment).  Used for fp32 NCHW activations (FWD / DGRAD) and for image-fed WGRAD operands.
__device__ __forceinline__ int fx_tr_off(int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }
//  "rc": reduction-contiguous, 128 rows x 16 k, 32-B rows; the two 16-B halves of a row are swapped on rows with bit 3 set, which makes the 16-lane groups
//  of a ds_read_b128 hit 16 different bank quads (unswizzled they collide two by two).  Used for weights, image-fed activations (FWD / DGRAD) and for fp32
//  WGRAD operands.
__device__ __forceinline__ int fx_rc_off(int row, int half) { return 32 * row + 16 * (half ^ ((row >> 3) & 1)); }

// NA x NB of the wave's 2 x 2 sub-tiles (32 x 32 each) are computed: a wave whose rows reach beyond the tensor (272 = 2 x 128 + 16 regressor channels,
// 64-channel layers in a 128-row tile) issues no MFMAs for the sub-tiles that hold nothing
#define P3D_FX_PRODUCTS_AB(ACC, PIX, CH, NA, NB) P3D_FX_PRODUCTS_RANGE(ACC, PIX, CH, NA, NB, 0, 6)
#define P3D_FX_PRODUCTS_RANGE(ACC, PIX, CH, NA, NB, P0, P1)                                                            \
    _Pragma("unroll") for (int pa = P0; pa < P1; ++pa) {                                                               \
        constexpr int PP[6] = {2, 0, 1, 1, 0, 0}, PC[6] = {0, 2, 1, 0, 1, 0};                                           \
        _Pragma("unroll") for (int a = 0; a < NA; ++a) _Pragma("unroll") for (int b = 0; b < NB; ++b)                   \
            ACC[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(PIX[PP[pa]][a], CH[PC[pa]][b], ACC[a][b], 0, 0, 0);    \
    }
// wave-uniform count (0, 1, 2) of 32-row sub-tiles of the wave's 64 rows starting at `first` that begin below `limit`
__device__ __forceinline__ int fx_live_subtiles(int first, int limit) {
    const int n = (limit - first + 31) >> 5;
    return __builtin_amdgcn_readfirstlane(n < 0 ? 0 : (n > 2 ? 2 : n));
}

// Operand fetches are buffer loads against block-uniform resources: per-thread byte offsets change only when the filter tap changes (they carry the
// out-of-range bit 0x80000000 for padding pixels / rows beyond the tensor, which the resource's range check turns into zeros), the per-K-step part of an
// address is a wave-uniform scalar offset.  So a K step's fetch is loads only: no branches, no per-step address arithmetic.
constexpr int FX_OOB = (int)0x80000000;
__device__ f32x4 fx_buffer_load_f32x4(i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.v4f32");
__device__ i32x4 fx_buffer_load_i32x4(i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.v4i32");
__device__ float fx_buffer_load_f32(i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.f32");
__device__ __forceinline__ i32x4 fx_rsrc(const void* base, size_t bytes) {
    const unsigned n = bytes < (size_t)0x80000000u ? (unsigned)bytes : 0x80000000u;
    const uint64_t a = reinterpret_cast<uint64_t>(base);
    i32x4 r;
    r[0] = (int)(unsigned)a; r[1] = (int)((a >> 32) & 0xffff); r[2] = (int)n; r[3] = 0x00020000;
    return r;
}
__device__ __forceinline__ bf8 fx_tr_read(const unsigned char* base, const int (&off)[2]) {
    s8v v;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const s4t r4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4t*)(base + off[half]));
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * half + e] = r4[e];
    }
    return __builtin_bit_cast(bf8, v);
}
// byte offsets of the two transposing 8-B reads that give this lane its fragment (8 consecutive reduction rows of column cb + (lane & 31)) of a "tr" image:
// 16-lane group g reads the 4-row x 16-column block of rows 8 (g >> 1) + 4 half .. +3, columns cb + 16 (g & 1) .. +15
__device__ __forceinline__ void fx_tr_frag_off(int lane, int cb, int (&off)[2]) {
    const int g = lane >> 4, idx = lane & 15, q = idx >> 2, pq = idx & 3;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int row = 8 * (g >> 1) + 4 * half + q;
        off[half] = fx_tr_off(row, ((cb + 16 * (g & 1)) >> 3) + (pq >> 1)) + 8 * (pq & 1);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------------
// FWD / DGRAD
// ------------------------------------------------------------------------------------------------------------------------------------------
// The weight operand always comes from a pre-split weight image: three 16-B copies per thread and K step, no VALU work.
// AMODE 0: the activation operand is fp32 NCHW; a thread fetches four consecutive pixels of two reduction rows per K step and splits them ("tr" image).
//          PRO 4 multiplies by pmask[pixel] first (partial convolution: one factor per pixel, all channels).
// AMODE 1: the activation operand is a pre-split activation image; a thread copies one 16-B chunk (pixel, half of the 16 channels) per plane ("rc" image).
// EPIX: the epilogue, one of the FX_EPI_* codes (p3d_fx.h); below SUMS is the kind of partial sums it takes and EM whether it multiplies by emask[pixel] in registers.
// the launch's parameters as block z sees them: a strided data gradient runs its parity classes as the z slices of one grid (the longest K loops first), each a dense
// GEMM over the filter taps that reach the class
__device__ __forceinline__ FxConvParams fx_class_params(const FxConvParams& in) {
    FxConvParams p = in;
    if (in.ncls > 0) {
        const FxConvClass& c = in.cls[blockIdx.z];
        p.nR = c.nR; p.nS = c.nS; p.ntap = c.ntap; p.r0 = c.r0; p.rstep = c.rstep; p.s0 = c.s0; p.sstep = c.sstep;
        p.hoff = c.hoff; p.hstep = c.hstep; p.woff = c.woff; p.wstep = c.wstep; p.oy0 = c.oy0; p.ox0 = c.ox0;
    }
    return p;
}

// TAPI (image-fed multi-tap launches of wide layers, FxConvParams::tap_inner): the K steps walk the taps innermost
// RAG ("ragged", fx_conv_fwd with FxFuse::ragged): map widths that are not multiples of 4.  The GEMM column stays the flat pixel index, so a thread's four
// consecutive pixels may straddle an output row or an image: their positions are derived per element when the tap changes, from the first pixel's (row, column,
// image) kept across the K loop; every fetch is a dword load, and the dense store falls back to dword accesses wherever four pixels do not share an image or a
// 16-B line.  fp32-fed forward only, epilogues 8 (inference) and 0 (split-K slabs, the dense training launches); as a partial convolution (PRO 4) epilogues 9
// (inference), 4 (training, p3d_x3_any_partial_enable) and 0: the operand factor is fetched per element at the same positions from the one-plane mask (its own image
// offset, stepped beside x's), the result factor per element in the staged store -- for epilogue 4 BEFORE the accumulate read, so an empty window leaves exactly what
// the result held.
// Image-fed (AMODE 1, p3d_x3_any_images_enable), epilogue 0 only, either K order: the operand side is the AMODE 1 fetch as it is -- one pixel's 32-B row per thread, its
// position from the flat column, so nothing there knows of four-pixel groups -- and the result side the staged store above.
// Image-fed with epilogue 1 / 2 (tap-outer only; the ragged residual blocks of p3d_block_any_enable): the sums run in the register view, where a lane's four flat
// pixels may lie in two images or end beyond NP -- an element enters a sum only below NP, and for sums 2 its ep_c is read at its own (image, pixel), by the walk of
// the staged store.  red[][][] and partial[tile_n][M][2] as in the aligned instances: a fixed order, no atomics.  Never split along K (fx_conv_fwd / fx_conv_dgrad).
// ROWS (image-fed, the dense block executor's launches): the activation operand is an fp32 row image [N][Cred/16][Hi][Wi][16] (fx_row_image); a thread fetches its half of a
// pixel's 64-B row (two 16-B loads instead of three plane loads) and cuts it into the three pieces on the way from registers to LDS: same stores, same LDS image.
template <int AMODE, int PRO, int EPIX, bool TAPI = false, bool RAG = false, bool ROWS = false>
__global__ __launch_bounds__(256, 3) void fx_conv_kernel(const FxConvParams p_in) {
    static_assert(!TAPI || AMODE == 1, "the tap-inner K order is an image-fed instance");
    static_assert(!ROWS || (AMODE == 1 && !RAG), "row images feed the aligned image-fed instances");
    static_assert(!RAG || (AMODE == 1 && PRO == 0 && (EPIX == FX_EPI_STORE || EPIX == FX_EPI_STATS || EPIX == FX_EPI_BWD_SUMS)) ||
                      (AMODE == 0 && ((PRO == 0 && (EPIX == FX_EPI_STORE || EPIX == FX_EPI_INFER)) || (PRO == 4 && (EPIX == FX_EPI_STORE || EPIX == FX_EPI_INFER_FACTOR || EPIX == FX_EPI_FACTOR)))),
                  "the ragged instances are the fp32-fed forward with the plain / inference epilogue, dense or as a partial convolution, and the image-fed forward with the plain or a BatchNorm one");
    constexpr int SUMS = fx_epi_sums(EPIX);
    constexpr bool EM = fx_epi_factor(EPIX) && !RAG;          // (ragged: four pixels of the register view may lie in two images or end beyond the factor -- the staged store applies it)
    constexpr bool EM_RAG = RAG && EPIX == FX_EPI_FACTOR;
    const FxConvParams p = fx_class_params(p_in);
    static_assert(AMODE == 0 || PRO == 0, "the partial-convolution factor is applied by the in-kernel split");
    // one shared array: two buffers of [3 pixel pieces][3 channel pieces]; after the K loop the result tile on its way out (33.8 KB) and, behind it, the
    // per-channel sums of SUMS 1 / 2
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * 6 * FX_PIECE];
    constexpr int BUFB = 6 * FX_PIECE, CH0 = 3 * FX_PIECE;                             // bytes per buffer; offset of the channel (weight) pieces in a buffer
    float (*const red)[2][128] = reinterpret_cast<float (*)[2][128]>(lds + 40960);     // SUMS 1 / 2: [wave along pixels][sum kind][channel]
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), wm = wave >> 1, wn = wave & 1;
    // XCD-aware remap (bijective): blocks b, b+8, ... share an XCD; give each XCD a contiguous run of logical ids (pixel tile outer, channel tile inner)
    int bid;
    {
        const int nwg = gridDim.x, q = nwg >> 3, r = nwg & 7, xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int tile_m = bid % p.tiles_m, tile_n = bid / p.tiles_m;
    const int m0 = tile_m * FX_BM, n0 = tile_n * FX_BN;
    const int OHW = p.OH * p.OW;
    const int HWi = p.Hi * p.Wi;
    const int nfirst = n0 / OHW;                   // first image this block touches: base of the activation resources
    const int csteps = p.Cred / FX_BK;
    int nk = p.ntap * csteps, kt0 = 0;
    if (p.kchunk > 0) {                            // split-K: this block reduces K steps [kt0, kt0 + nk) into slab blockIdx.y
        kt0 = blockIdx.y * p.kchunk;
        nk = min(nk - kt0, p.kchunk);
    }
    int f_tap = kt0 / csteps, f_k = (kt0 - f_tap * csteps) * FX_BK;
    if constexpr (TAPI) { f_k = (kt0 / p.ntap) * FX_BK; f_tap = kt0 - (kt0 / p.ntap) * p.ntap; }       // K step kt = (channel step kt / ntap, tap kt % ntap)

    // weight operand: three 16-B chunks of the K step's 12 KB image tile
    const i32x4 rW = fx_rsrc(p.Wimg, (size_t)p.R * p.S * p.tiles_m * csteps * (3 * FX_PIECE));
    int w_voff[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) w_voff[j] = 16 * (t + 256 * j);

    // ---- activation operand: staging maps ----
    // AMODE 0: reduction rows trow, trow + 8; columns (pixels) 4 tp4 .. 4 tp4 + 3.  AMODE 1: pixel pp of the tile, 16-B half ph of its 32-B row.
    const int trow = t >> 5, tp4 = t & 31;
    const int pp = t >> 1, ph = (t & 1) ^ ((t >> 4) & 1);       // (the half whose place in the "rc" image is byte 16 t: a wave's chunks are 1 KB contiguous, lane-linear)
    const int col = n0 + (AMODE == 0 ? 4 * tp4 : pp);
    const bool col_ok = col < p.NP;
    int hbase = 0, wbase = 0, img_off = 0, mimg_off = 0;
    {
        const int cc = col_ok ? col : 0;
        const int pn = cc / OHW;
        const int rem = cc - pn * OHW, oh = rem / p.OW, ow = rem - oh * p.OW;
        hbase = oh * p.hmul + p.hoff;
        wbase = ow * p.wmul + p.woff;
        img_off = AMODE == 0 ? ((pn - nfirst) * p.Cred + trow) * HWi : (pn - nfirst) * csteps * HWi;       // AMODE 1: in pixels (32-B rows)
        mimg_off = (pn - nfirst) * HWi;                 // PRO 4: the per-pixel factor has one plane per image
    }
    i32x4 rX, rXi[3];
    if constexpr (AMODE == 0) {
        rX = fx_rsrc(p.X + (size_t)nfirst * p.Cred * HWi, (size_t)(p.N - nfirst) * p.Cred * HWi * sizeof(float));
    } else if constexpr (ROWS) {
        rXi[0] = fx_rsrc(p.Ximg + (size_t)nfirst * p.Cred * HWi * 4, (size_t)(p.N - nfirst) * p.Cred * HWi * 4);
    } else {
        const size_t left = (size_t)(p.N - nfirst) * p.Cred * HWi * 2;
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) rXi[pc] = fx_rsrc(p.Ximg + pc * p.plane_bytes + (size_t)nfirst * p.Cred * HWi * 2, left);
    }
    // RAG: the thread's FIRST pixel as (output row, output column, element offset of its image's reduction row trow); set_tap steps from it pixel by pixel through
    // row ends and image ends, so the K loop carries three values instead of a position per element
    // (derived here again rather than kept from the block above, which computes the same row and column: sharing them was tried and the register allocator then
    // spills 92 B per lane instead of 64, profiles/eval_folded_anysize.md)
    // PRO 4: a fourth, the offset of the image's mask plane (rPM is based at image nfirst like rX).  (Deriving all four from `col` again at every tap change, and
    // making the second sub-tile's fragment offsets from the first's in every step, were tried to free registers: neither removes the loop's spill reloads,
    // profiles/eval_folded_oddsides.md)
    int rg_oh = 0, rg_ow = 0, rg_img = 0, rg_mimg = 0;
    if constexpr (RAG) {
        const int cc = col_ok ? col : 0;
        const int pn = cc / OHW;
        const int rem = cc - pn * OHW;
        rg_oh = rem / p.OW; rg_ow = rem - rg_oh * p.OW;
        rg_img = ((pn - nfirst) * p.Cred + trow) * HWi;
        rg_mimg = (pn - nfirst) * HWi;
    }
    const i32x4 rPM = fx_rsrc(PRO == 4 ? p.pmask + (size_t)nfirst * HWi : nullptr, PRO == 4 ? (size_t)(p.N - nfirst) * HWi * sizeof(float) : 0);

    // per-tap state of the activation gather (recomputed only when the tap changes)
    int x_voff[4] = {FX_OOB, FX_OOB, FX_OOB, FX_OOB};     // AMODE 0: byte offsets of this thread's four pixels in reduction row `trow` of chunk 0; AMODE 1: [0] only
    bool x_vec = false;
    int w_tapoff = 0;                                      // scalar byte offset of the tap inside the weight image
    int cur_tap = -1;
    f32x4 tmask = {1.f, 1.f, 1.f, 1.f};                    // PRO 4: the factor of this thread's four pixels at the current tap (the same for every K step of the tap)
    auto set_tap = [&](int tap) {
        cur_tap = tap;
        const int ir = tap / p.nS, is = tap - ir * p.nS;
        const int wtap = (p.r0 + p.rstep * ir) * p.S + p.s0 + p.sstep * is;
        w_tapoff = (wtap * p.tiles_m + tile_m) * csteps * (3 * FX_PIECE);
        const int hi = hbase + ir * p.hstep, wshift = is * p.wstep, wi0 = wbase + wshift;
        const bool row_ok = col_ok && (unsigned)hi < (unsigned)p.Hi;
        if constexpr (AMODE != 0) {
            x_voff[0] = (row_ok && (unsigned)wi0 < (unsigned)p.Wi) ? (img_off + hi * p.Wi + wi0) * (ROWS ? 64 : 32) + (ROWS ? 32 : 16) * ph : FX_OOB;
        } else if constexpr (RAG) {
            const int dh = p.hoff + ir * p.hstep, dw = p.woff + wshift;         // wave-uniform: the tap's displacement
            int oh = rg_oh, ow = rg_ow, im = rg_img;
            int mim = rg_mimg;                                                  // PRO 4: the same walk over the one-plane mask (stride HWi per image)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int he = oh * p.hmul + dh, we = ow * p.wmul + dw;
                const bool ok = col + e < p.NP && (unsigned)he < (unsigned)p.Hi && (unsigned)we < (unsigned)p.Wi;
                x_voff[e] = ok ? (im + he * p.Wi + we) * 4 : FX_OOB;
                if constexpr (PRO == 4) tmask[e] = fx_buffer_load_f32(rPM, ok ? (mim + he * p.Wi + we) * 4 : FX_OOB, 0, 0);
                if (++ow == p.OW) { ow = 0; if (++oh == p.OH) { oh = 0; im += p.Cred * HWi; mim += HWi; } }      // the next flat pixel: next row, next image
            }
        } else {
            x_vec = p.wmul == 1 && ((p.woff + wshift) & 3) == 0;        // wave-uniform: the four pixels are one aligned 16-B group, in or out together
            const int base = (img_off + hi * p.Wi + wi0) * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool ok = row_ok && (unsigned)(wi0 + e * p.wmul) < (unsigned)p.Wi;
                x_voff[e] = ok ? base + e * p.wmul * 4 : FX_OOB;
            }
            if constexpr (PRO == 4) {
                const int mbase = (mimg_off + hi * p.Wi + wi0) * 4;
                if (x_vec) tmask = fx_buffer_load_f32x4(rPM, x_voff[0] >= 0 ? mbase : FX_OOB, 0, 0);
                else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) tmask[e] = fx_buffer_load_f32(rPM, x_voff[e] >= 0 ? mbase + e * p.wmul * 4 : FX_OOB, 0, 0);
                }
            }
        }
    };

    f32x4 rx[2];                                   // (ROWS: the thread's 32 B of the pixel's row)
    i32x4 rwi[3], rxi[3];                          // this thread's three 16-B chunks of the K step's weight image / activation image
    f32x4 smask = {1.f, 1.f, 1.f, 1.f};            // PRO 4: per-pixel factor of the fetched K step
    auto fetch = [&]() {
        if (f_tap != cur_tap) { asm volatile("" ::: "memory"); set_tap(f_tap); }       // (a real, wave-uniform branch: taken once per tap, not if-converted into every K step)
        {
            const int so = w_tapoff + (f_k >> 4) * (3 * FX_PIECE);
#pragma unroll
            for (int j = 0; j < 3; ++j) rwi[j] = fx_buffer_load_i32x4(rW, w_voff[j], so, 0);
        }
        if constexpr (ROWS) {
            const int so = (f_k >> 4) * HWi * 64;
#pragma unroll
            for (int i = 0; i < 2; ++i) rx[i] = fx_buffer_load_f32x4(rXi[0], x_voff[0], so + 16 * i, 0);
        } else if constexpr (AMODE != 0) {
            const int so = (f_k >> 4) * HWi * 32;                  // wave-uniform: the K step's channel group
#pragma unroll
            for (int pc = 0; pc < 3; ++pc) rxi[pc] = fx_buffer_load_i32x4(rXi[pc], x_voff[0], so, 0);
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int so = (f_k + 8 * i) * HWi * 4;             // wave-uniform: reduction chunk + this pass's 8-row step
                if (!RAG && x_vec) rx[i] = fx_buffer_load_f32x4(rX, x_voff[0], so, 0);
                else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) rx[i][e] = fx_buffer_load_f32(rX, x_voff[e], so, 0);
                }
            }
            if constexpr (PRO == 4) smask = tmask;            // (the factor of the tap these loads belong to: the next fetch may already be at another tap)
        }
        if constexpr (TAPI) { if (++f_tap == p.ntap) { f_tap = 0; f_k += FX_BK; } }
        else {
            f_k += FX_BK;
            if (f_k == p.Cred) { f_k = 0; ++f_tap; }
        }
    };
    // LDS addresses of this thread's staging stores, relative to a buffer's first piece
    const int st_p[2] = {fx_tr_off(trow, tp4 >> 1) + 8 * (tp4 & 1), fx_tr_off(trow + 8, tp4 >> 1) + 8 * (tp4 & 1)};
    const int st_p1 = fx_rc_off(pp, ph);
    auto stage = [&](int buf) {
        unsigned char* pb = lds + buf * BUFB;
        unsigned char* cb = pb + CH0;
#pragma unroll
        for (int j = 0; j < 3; ++j) *reinterpret_cast<i32x4*>(cb + 16 * (t + 256 * j)) = rwi[j];
        if constexpr (AMODE != 0) {
            if constexpr (ROWS) fx_split_row8(rx[0], rx[1], rxi);
#pragma unroll
            for (int pc = 0; pc < 3; ++pc) *reinterpret_cast<i32x4*>(pb + pc * FX_PIECE + st_p1) = rxi[pc];
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                f32x4 v = rx[i];
                if constexpr (PRO == 4) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] *= smask[e];
                }
                fx_split_store(pb + st_p[i], v);
            }
        }
    };

    f32x16 acc[2][2];               // [pixel sub-tile a][channel sub-tile b]
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    const int fr = lane & 31, fh = lane >> 5;
    // fragment read offsets: "tr" image: two transposing 8-B reads per fragment; "rc" image: one 16-B read
    int rd_p[2][2], rd_c[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        if constexpr (AMODE == 0) fx_tr_frag_off(lane, wn * 64 + a * 32, rd_p[a]);
        else rd_p[a][0] = rd_p[a][1] = fx_rc_off(wn * 64 + a * 32 + fr, fh);
        rd_c[a] = CH0 + fx_rc_off(wm * 64 + a * 32 + fr, fh);
    }
    const int live_b = fx_live_subtiles(m0 + wm * 64, p.M);       // channel sub-tiles of this wave that hold output channels
    // Software pipeline: the registers fetched during K step kt - 1 hold step kt + 1; they go to LDS at the HEAD of step kt (right behind the reads of the
    // first product's fragments), then the fetch of step kt + 2 is issued, then the step's MFMAs run.  So a fetch has a whole step to arrive, and the LDS
    // stores complete under the MFMAs instead of in front of the barrier.
    if (nk > 0) { fetch(); stage(0); if (nk > 1) fetch(); }
    __syncthreads();
    // the K loop, once per count of live channel sub-tiles (a wave-uniform choice made outside the loop, so that each copy is the straight-line loop)
    auto kloop = [&](auto nbt) {
        constexpr int NB = decltype(nbt)::value;
        bf8 pf[3][2], cf[3][2];
        auto step = [&](int kt, auto st, auto fe) {
            const int buf = kt & 1;
            const unsigned char* bb = lds + buf * BUFB;
            auto read_p = [&](int pc) {
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    if constexpr (AMODE == 0) pf[pc][a] = fx_tr_read(bb + pc * FX_PIECE, rd_p[a]);
                    else pf[pc][a] = *reinterpret_cast<const bf8*>(bb + pc * FX_PIECE + rd_p[a][0]);
                }
            };
            auto read_c = [&](int pc) {
#pragma unroll
                for (int a = 0; a < 2; ++a)
                    if (a < NB) cf[pc][a] = *reinterpret_cast<const bf8*>(bb + pc * FX_PIECE + rd_c[a]);
            };
            // Order of a step, pinned with scheduling barriers (left alone the scheduler sinks the loads to the end of the step to save registers, and a wave
            // that issues its six LDS stores before its first MFMA leaves the matrix pipe idle for their issue time): fragments of the first two products,
            // the first product's MFMAs, under them the LDS stores of step kt + 1 and the loads of step kt + 2, then the rest.
            if constexpr (NB > 0) {
                read_p(2); read_c(0); read_p(0); read_c(2);
                __builtin_amdgcn_sched_barrier(0);
                P3D_FX_PRODUCTS_RANGE(acc, pf, cf, 2, NB, 0, 1)
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (decltype(st)::value) stage(buf ^ 1);
            if constexpr (decltype(fe)::value) fetch();
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (NB > 0) {
                read_p(1); read_c(1);
                P3D_FX_PRODUCTS_RANGE(acc, pf, cf, 2, NB, 1, 6)
            }
            __syncthreads();
        };
        // (the two last steps are peeled so that the body of the main loop has no branch around its LDS stores: the wait in front of the first MFMA can then
        // count exactly the reads it needs instead of draining the stores too)
        int kt = 0;
        for (; kt + 2 < nk; ++kt) step(kt, std::true_type{}, std::true_type{});
        if (kt + 1 < nk) { step(kt, std::true_type{}, std::false_type{}); ++kt; }
        if (kt < nk) step(kt, std::false_type{}, std::false_type{});
    };
    if (live_b == 2) kloop(std::integral_constant<int, 2>{});
    else if (live_b == 1) kloop(std::integral_constant<int, 1>{});
    else kloop(std::integral_constant<int, 0>{});

    // ---- epilogue: lane = output channel (m), registers = pixels; acc[a][b][4 g + e] is pixel 32 a + 8 g + 4 fh + e of the wave's 64 ----
    // Dense results (every stride-1 launch, every split-K slab) leave through LDS: in the accumulator a store instruction would put 64 separate 16-B pieces
    // into 32 channel planes; transposed through a [64 channels][128 pixels] staging tile (two rounds, one per channel sub-tile) a wave stores two whole
    // 512-B channel rows per instruction.  Everything per element that needs the registers' view (bias, the partial-convolution factor, the BatchNorm sums
    // and their c2 operand) is done first, in place in the accumulator.
    const bool split = p.kchunk > 0;
    float* yout = p.Y + (split ? (size_t)blockIdx.y * p.slab_stride : 0);
    // (the forward-only epilogues -- statistics of y, the inference tails -- are never a parity class: their instances carry no strided path; nor do the ragged
    // ones, which fx_conv_fwd / fx_conv_dgrad launch dense only)
    constexpr bool FWD_ONLY = SUMS == 1 || fx_epi_infer(EPIX);
    const bool dense = FWD_ONLY || split || (p.oxs == 1 && p.oys == 1 && p.oy0 == 0 && p.ox0 == 0 && p.YW == p.OW && p.YH == p.OH);
    if constexpr (!FWD_ONLY && !RAG) {
        if (!dense) {
            // A parity class of a strided data gradient stores straight from the accumulator view and is done: four dwords oxs apart per lane and channel, read first
            // under `accumulate`.  It has this loop to itself, so that the dense epilogue below carries none of it (with the two in one loop every dense launch
            // paid for it: profiles/strided_paths.md).  No sums here: fx_conv_dgrad refuses the BatchNorm-backward epilogue at a stride.
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int c4 = n0 + wn * 64 + a * 32 + 8 * g + 4 * fh;
                    if (c4 >= p.NP) continue;
                    const int n = c4 / OHW, rem = c4 - n * OHW, oh = rem / p.OW, ow = rem - oh * p.OW;
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const int m = m0 + wm * 64 + b * 32 + fr;
                        if (m >= p.M) continue;
                        f32x4 v = {acc[a][b][4 * g], acc[a][b][4 * g + 1], acc[a][b][4 * g + 2], acc[a][b][4 * g + 3]};
                        if (p.bias) { const float bb = p.bias[m]; v[0] += bb; v[1] += bb; v[2] += bb; v[3] += bb; }
                        float* dst = yout + (((size_t)n * p.M + m) * p.YH + p.oy0 + oh * p.oys) * p.YW + p.ox0 + ow * p.oxs;
                        if (p.oxs == 1) {
                            if constexpr (EM) {
                                const f32x4 em = *reinterpret_cast<const f32x4*>(p.emask + ((size_t)n * p.YH + p.oy0 + oh * p.oys) * p.YW + p.ox0 + ow);
                                v[0] *= em[0]; v[1] *= em[1]; v[2] *= em[2]; v[3] *= em[3];
                            }
                            f32x4* d4 = reinterpret_cast<f32x4*>(dst);
                            if (p.accumulate) { const f32x4 o4 = *d4; v[0] += o4[0]; v[1] += o4[1]; v[2] += o4[2]; v[3] += o4[3]; }
                            *d4 = v;
                        } else {
                            if constexpr (EM) {
                                const float* em = p.emask + ((size_t)n * p.YH + p.oy0 + oh * p.oys) * p.YW + p.ox0 + ow * p.oxs;
#pragma unroll
                                for (int e = 0; e < 4; ++e) v[e] *= em[e * p.oxs];
                            }
#pragma unroll
                            for (int e = 0; e < 4; ++e) dst[e * p.oxs] = p.accumulate ? dst[e * p.oxs] + v[e] : v[e];
                        }
                    }
                }
            return;
        }
    }
    float ssum[2] = {0.f, 0.f}, ssq[2] = {0.f, 0.f};
    float esc[2] = {0.f, 0.f}, esh[2] = {0.f, 0.f}, emean[2] = {0.f, 0.f};
    if constexpr (SUMS == 2) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int m = m0 + wm * 64 + b * 32 + fr;
            if (m < p.M) { esc[b] = p.ep_tab[8 * m]; esh[b] = p.ep_tab[8 * m + 1]; emean[b] = p.ep_tab[8 * m + 2]; }
        }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c4 = n0 + wn * 64 + a * 32 + 8 * g + 4 * fh;         // first of this lane's 4 consecutive pixels
            if (c4 >= p.NP) continue;
            const int n = c4 / OHW, rem = c4 - n * OHW, oh = rem / p.OW, ow = rem - oh * p.OW;
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int m = m0 + wm * 64 + b * 32 + fr;
                if (m >= p.M) continue;
                f32x4 v = {acc[a][b][4 * g], acc[a][b][4 * g + 1], acc[a][b][4 * g + 2], acc[a][b][4 * g + 3]};
                if (!split && EPIX != FX_EPI_INFER_FACTOR) {        // (there: factor and bias in the staged store below, where no accumulator is live)
                    if (p.bias) { const float bb = p.bias[m]; v[0] += bb; v[1] += bb; v[2] += bb; v[3] += bb; }
                }
                if constexpr (EM) {               // partial convolution: the result times the per-pixel factor (before it joins an existing gradient)
                    const f32x4 em = *reinterpret_cast<const f32x4*>(p.emask + ((size_t)n * p.YH + oh) * p.YW + ow);
                    v[0] *= em[0]; v[1] *= em[1]; v[2] *= em[2]; v[3] *= em[3];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[a][b][4 * g + e] = v[e];
                if constexpr (RAG && SUMS != 0) {
                    // the four flat pixels one by one: none beyond NP, each at its own (image, pixel) (launched unsplit only)
                    int ne = n, re = rem;
#pragma unroll
                    for (int e = 0; e < 4; ++e, ++re) {
                        if (c4 + e >= p.NP) break;
                        while (re >= OHW) { re -= OHW; ++ne; }
                        if constexpr (SUMS == 1) { ssum[b] += v[e]; ssq[b] = fmaf(v[e], v[e], ssq[b]); }
                        else {
                            const float c2 = p.ep_c[((size_t)ne * p.M + m) * OHW + re];
                            const float gg = fmaf(c2, esc[b], esh[b]) > 0.f ? v[e] : 0.f;
                            ssum[b] += gg; ssq[b] = fmaf(gg, c2 - emean[b], ssq[b]);
                        }
                    }
                } else if constexpr (SUMS == 1) {
                    if (!split) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) { ssum[b] += v[e]; ssq[b] = fmaf(v[e], v[e], ssq[b]); }
                    }
                }
                if constexpr (SUMS == 2 && !RAG) {
                    if (!split) {
                        const f32x4 c2 = *reinterpret_cast<const f32x4*>(p.ep_c + ((size_t)n * p.M + m) * OHW + rem);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float gg = fmaf(c2[e], esc[b], esh[b]) > 0.f ? v[e] : 0.f;
                            ssum[b] += gg; ssq[b] = fmaf(gg, c2[e] - emean[b], ssq[b]);
                        }
                    }
                }
            }
        }
    if constexpr (SUMS == 1 || SUMS == 2) {
        if (!split) {
            // the two half-waves hold different pixels of the same channels; the two waves along the pixel axis meet in LDS behind the staging tile (the sums
            // leave the registers here, in front of the staged store: its barriers also order these writes before the reads at the end)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                ssum[b] += __shfl_xor(ssum[b], 32, 64);
                ssq[b] += __shfl_xor(ssq[b], 32, 64);
                if (fh == 0) { red[wn][0][wm * 64 + b * 32 + fr] = ssum[b]; red[wn][1][wm * 64 + b * 32 + fr] = ssq[b]; }
            }
        }
    }
    {
        // (every wave left the K loop through its last barrier: the operand buffers are free)
        constexpr int EROW = 512 + 16;               // bytes per staged channel row: 128 pixels + one 16-B pad (staging stores of 8 consecutive rows hit 32 different banks)
        const bool accum = !split && p.accumulate;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            if (b == 1) __syncthreads();             // round 0's rows have been read
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *reinterpret_cast<f32x4*>(lds + (wm * 32 + fr) * EROW + (wn * 64 + a * 32 + 8 * g + 4 * fh) * 4) =
                        f32x4{acc[a][b][4 * g], acc[a][b][4 * g + 1], acc[a][b][4 * g + 2], acc[a][b][4 * g + 3]};
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int id = t + 256 * i, row = id >> 5, q = id & 31;
                const int m = m0 + (row >> 5) * 64 + b * 32 + (row & 31);
                const int c4 = n0 + 4 * q;
                if (m >= p.M || c4 >= p.NP) continue;
                const int n = c4 / OHW, rem = c4 - n * OHW;
                f32x4 v = *reinterpret_cast<const f32x4*>(lds + row * EROW + q * 16);
                const size_t at = ((size_t)n * p.M + m) * OHW + rem;
                f32x4* dst = reinterpret_cast<f32x4*>(yout + at);
                if constexpr (RAG) {
                    // four pixels of one image on one 16-B line go out as below; anything else element by element, each with its own image and never beyond NP
                    if (!(rem + 3 < OHW && (reinterpret_cast<uintptr_t>(dst) & 15) == 0)) {
                        int ne = n, re = rem;
#pragma unroll
                        for (int e = 0; e < 4; ++e, ++re) {
                            if (c4 + e >= p.NP) break;
                            while (re >= OHW) { re -= OHW; ++ne; }
                            const size_t ae = ((size_t)ne * p.M + m) * OHW + re;
                            float ve = v[e];
                            if constexpr (EM_RAG) ve *= p.emask[(size_t)ne * OHW + re];        // the factor first, then what the result held
                            if (accum) ve += yout[ae];
                            if constexpr (EPIX == FX_EPI_INFER_FACTOR) ve = ve * p.emask[(size_t)ne * OHW + re] + (p.bias ? p.bias[m] : 0.f);      // this element's own image
                            if constexpr (fx_epi_infer(EPIX)) {
                                if (p.ep_res) ve += p.ep_res[ae];
                                if (p.ep_relu) ve = fmaxf(ve, 0.f);
                            }
                            yout[ae] = ve;
                        }
                        continue;
                    }
                }
                if constexpr (EM_RAG) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] *= p.emask[(size_t)n * OHW + rem + e];
                }
                if (accum) {
                    f32x4 o4;
                    if (p.acc_src) {              // the summand comes from another tensor (through a ReLU's mask bytes): Y is written, never read
                        o4 = *reinterpret_cast<const f32x4*>(p.acc_src + at);
                        if (p.acc_mask) {
                            const unsigned mk = p.acc_mask[at >> 2];
#pragma unroll
                            for (int e = 0; e < 4; ++e) o4[e] = (mk >> e) & 1u ? o4[e] : 0.f;
                        }
                    } else o4 = *dst;
                    v[0] += o4[0]; v[1] += o4[1]; v[2] += o4[2]; v[3] += o4[3];
                }
                if constexpr (EPIX == FX_EPI_INFER_FACTOR) {        // (fx_conv_fwd launches it dense, unsplit and without accumulate: one factor per pixel, the plane of image n)
                    // (ragged: with OHW odd the factor's line n OHW + rem and y's ((n M + m) OHW + rem) are 16-B aligned at different times -- element by element)
                    f32x4 em;
                    if constexpr (RAG) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) em[e] = p.emask[(size_t)n * OHW + rem + e];
                    } else em = *reinterpret_cast<const f32x4*>(p.emask + (size_t)n * OHW + rem);
                    const float bb = p.bias ? p.bias[m] : 0.f;
                    v[0] = v[0] * em[0] + bb; v[1] = v[1] * em[1] + bb; v[2] = v[2] * em[2] + bb; v[3] = v[3] * em[3] + bb;
                }
                if constexpr (fx_epi_infer(EPIX)) {
                    if (p.ep_res) { const f32x4 r4 = *reinterpret_cast<const f32x4*>(p.ep_res + at); v[0] += r4[0]; v[1] += r4[1]; v[2] += r4[2]; v[3] += r4[3]; }
                    if (p.ep_relu) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
                }
                *dst = v;
            }
        }
    }
    if constexpr (SUMS == 1 || SUMS == 2) {
        if (!split) {
            if (t < 128 && m0 + t < p.M) {
                float* dst = p.partial + ((size_t)tile_n * p.M + m0 + t) * 2;
                dst[0] = red[0][0][t] + red[1][0][t];
                dst[1] = red[0][1][t] + red[1][1][t];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------------
// FWD / DGRAD on v_mfma_f32_16x16x32_bf16 ("fx16"): image-fed launches only (AMODE 1, PRO 0).
// The instruction reduces over 32 k; a K step here is still 16 channels, and the two halves of the instruction's k range carry two DIFFERENT piece products of the
// same 16 channels: lanes 0-31 hold piece X of the pixel operand against piece X' of the channel operand, lanes 32-63 piece Y against Y', so that one instruction
// adds P_X C_X' + P_Y C_Y' into the accumulator.  The six products of a step are three such pairs, smallest first:
//     (P_hi | P_lo) x (C_lo | C_hi)      (P_hi | P_mid) x (C_mid | C_mid)      (P_hi | P_mid) x (C_hi | C_hi)
// = 3 x 16 instructions of 16 passes per wave and step instead of 6 x 4 of 32 passes: the same matrix-pipe cycles, 20 fragment reads per wave instead of 12, and a
// shape on which the chip holds a higher clock (MI355X_MICROARCH.md, DVFS item 7).  16 x 16 sub-tiles also make the channel tile a template parameter: BM = 96
// (wave 48 channels x 64 pixels: the 272-channel regressor is 96 + 96 + 80 instead of 128 + 128 + 16) or 64 (wave 32 x 64); 128-row tiles stay on fx_conv_kernel (fx16_bm).
// LDS images: "rc" rows of 32 B (row = pixel or channel, 16 k), NOT swizzled: a 16-lane group of the fragment read takes rows r .. r+3 / r+12 .. r+15 of one half
// and rows r+4 .. r+11 of the other, which are 16 different bank quads as they lie.  The weight image keeps the swizzle of fx_rc_off; the staging copy undoes it
// by fetching, for LDS position 16 t, the chunk that belongs there.
// In the accumulator a lane is output channel (lane & 15) of a 16-channel group and holds four consecutive pixels 4 (lane >> 4) .. + 3 of a 16-pixel group.
// ------------------------------------------------------------------------------------------------------------------------------------------
// ROWS: the activation operand is an fp32 row image, cut into pieces between the fetch registers and LDS (see fx_conv_kernel)
template <int BM, int EPI, bool TAPI = false, bool ROWS = false>
__global__ __launch_bounds__(256, 3) void fx16_conv_kernel(const FxConvParams p_in) {
    const FxConvParams p = fx_class_params(p_in);
    constexpr int SUMS = fx_epi_sums(EPI);
    static_assert(BM == 96 || BM == 64, "channel tile");
    constexpr int GA = 4, GB = BM / 32;                 // 16-pixel / 16-channel groups of a wave (2 x 2 waves; a wave: 64 pixels x BM / 2 channels)
    constexpr int WCH = BM / 2;
    constexpr int PIECE_P = 128 * 32, PIECE_C = BM * 32;
    constexpr int BUFB = 3 * PIECE_P + 3 * PIECE_C, CH0 = 3 * PIECE_P;
    constexpr int LDSB = 2 * BUFB > 43008 ? 2 * BUFB : 43008;        // after the K loop: the result tile on its way out (33.8 KB) and the per-channel sums behind it
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDSB];
    float (*const red)[2][128] = reinterpret_cast<float (*)[2][128]>(lds + 40960);
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), wm = wave >> 1, wn = wave & 1;
    int bid;
    {
        const int nwg = gridDim.x, q = nwg >> 3, r = nwg & 7, xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int tile_m = bid % p.tiles_m, tile_n = bid / p.tiles_m;
    const int m0 = tile_m * BM, n0 = tile_n * FX_BN;
    const int OHW = p.OH * p.OW;
    const int HWi = p.Hi * p.Wi;
    const int nfirst = n0 / OHW;
    const int csteps = p.Cred / FX_BK;
    const int tiles128 = (p.M + 127) >> 7;             // row tiles of the weight image
    int nk = p.ntap * csteps, kt0 = 0;
    if (p.kchunk > 0) {
        kt0 = blockIdx.y * p.kchunk;
        nk = min(nk - kt0, p.kchunk);
    }
    int f_tap = kt0 / csteps, f_k = (kt0 - f_tap * csteps) * FX_BK;
    if constexpr (TAPI) { f_k = (kt0 / p.ntap) * FX_BK; f_tap = kt0 - (kt0 / p.ntap) * p.ntap; }       // K step kt = (channel step kt / ntap, tap kt % ntap)

    // weight operand: chunk id (piece, row of the tile, half) -> where it lies in the weight image (per 128-row tile and K step: 12 KB, fx_rc_off inside a piece)
    const i32x4 rW = fx_rsrc(p.Wimg, (size_t)p.R * p.S * tiles128 * csteps * (3 * FX_PIECE));
    int w_voff[3], w_lds[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int id = t + 256 * j, pc = id / (2 * BM), i = id - pc * (2 * BM), row = i >> 1, half = i & 1;
        const int grow = m0 + row, tl = grow >> 7;
        const bool ok = pc < 3 && tl < tiles128;
        w_voff[j] = ok ? tl * csteps * (3 * FX_PIECE) + pc * FX_PIECE + fx_rc_off(grow & 127, half) : FX_OOB;
        w_lds[j] = CH0 + (pc < 3 ? pc : 0) * PIECE_C + 16 * i;
    }
    constexpr int WCHUNKS = (3 * 2 * BM + 255) / 256;       // 16-B weight chunks per thread and K step (3, or 2 with BM = 64)
    const bool w_last = (3 * 2 * BM) % 256 == 0 || t + 256 * (WCHUNKS - 1) < 3 * 2 * BM;       // (BM = 128: every thread has all three chunks)

    // activation operand: pixel pp of the tile, 16-B half ph of its 32-B row, at LDS byte 16 t of each piece
    const int pp = t >> 1, ph = t & 1;
    const int col = n0 + pp;
    const bool col_ok = col < p.NP;
    int hbase = 0, wbase = 0, img_off = 0;
    {
        const int cc = col_ok ? col : 0;
        const int pn = cc / OHW;
        const int rem = cc - pn * OHW, oh = rem / p.OW, ow = rem - oh * p.OW;
        hbase = oh * p.hmul + p.hoff;
        wbase = ow * p.wmul + p.woff;
        img_off = (pn - nfirst) * csteps * HWi;
    }
    i32x4 rXi[3];
    if constexpr (ROWS) {
        rXi[0] = fx_rsrc(p.Ximg + (size_t)nfirst * p.Cred * HWi * 4, (size_t)(p.N - nfirst) * p.Cred * HWi * 4);
    } else {
        const size_t left = (size_t)(p.N - nfirst) * p.Cred * HWi * 2;
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) rXi[pc] = fx_rsrc(p.Ximg + pc * p.plane_bytes + (size_t)nfirst * p.Cred * HWi * 2, left);
    }
    int x_voff = FX_OOB, w_tapoff = 0, cur_tap = -1;
    auto set_tap = [&](int tap) {
        cur_tap = tap;
        const int ir = tap / p.nS, is = tap - ir * p.nS;
        const int wtap = (p.r0 + p.rstep * ir) * p.S + p.s0 + p.sstep * is;
        w_tapoff = wtap * tiles128 * csteps * (3 * FX_PIECE);
        const int hi = hbase + ir * p.hstep, wi0 = wbase + is * p.wstep;
        const bool ok = col_ok && (unsigned)hi < (unsigned)p.Hi && (unsigned)wi0 < (unsigned)p.Wi;
        x_voff = ok ? (img_off + hi * p.Wi + wi0) * (ROWS ? 64 : 32) + (ROWS ? 32 : 16) * ph : FX_OOB;
    };
    i32x4 rwi[3], rxi[3];
    f32x4 rxr[2];                   // ROWS: the thread's 32 B of the pixel's row
    auto fetch = [&]() {
        if (f_tap != cur_tap) { asm volatile("" ::: "memory"); set_tap(f_tap); }
        {
            const int so = w_tapoff + (f_k >> 4) * (3 * FX_PIECE);
#pragma unroll
            for (int j = 0; j < WCHUNKS; ++j) rwi[j] = fx_buffer_load_i32x4(rW, w_voff[j], so, 0);
        }
        if constexpr (ROWS) {
            const int so = (f_k >> 4) * HWi * 64;
#pragma unroll
            for (int i = 0; i < 2; ++i) rxr[i] = fx_buffer_load_f32x4(rXi[0], x_voff, so + 16 * i, 0);
        } else {
            const int so = (f_k >> 4) * HWi * 32;
#pragma unroll
            for (int pc = 0; pc < 3; ++pc) rxi[pc] = fx_buffer_load_i32x4(rXi[pc], x_voff, so, 0);
        }
        if constexpr (TAPI) { if (++f_tap == p.ntap) { f_tap = 0; f_k += FX_BK; } }
        else {
            f_k += FX_BK;
            if (f_k == p.Cred) { f_k = 0; ++f_tap; }
        }
    };
    auto stage = [&](int buf) {
        unsigned char* pb = lds + buf * BUFB;
#pragma unroll
        for (int j = 0; j < WCHUNKS; ++j)
            if (j + 1 < WCHUNKS || w_last) *reinterpret_cast<i32x4*>(pb + w_lds[j]) = rwi[j];
        if constexpr (ROWS) fx_split_row8(rxr[0], rxr[1], rxi);
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) *reinterpret_cast<i32x4*>(pb + pc * PIECE_P + 16 * t) = rxi[pc];
    };

    f32x4 acc[GA][GB];
#pragma unroll
    for (int a = 0; a < GA; ++a)
#pragma unroll
        for (int b = 0; b < GB; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int lc = lane & 15, lq = lane >> 4, up = lane >> 5;
    // fragment read offsets of the three pairings: lanes 0-31 read the first piece of a pair, lanes 32-63 the second
    const int frow_p = 32 * (wn * 64 + lc) + 16 * (lq & 1), frow_c = CH0 + 32 * (wm * WCH + lc) + 16 * (lq & 1);
    const int rdP_hl = frow_p + (up ? 2 : 0) * PIECE_P, rdP_hm = frow_p + (up ? 1 : 0) * PIECE_P;
    const int rdC_lh = frow_c + (up ? 0 : 2) * PIECE_C, rdC_mm = frow_c + PIECE_C, rdC_hh = frow_c;
    // 16-channel groups of this wave that hold output channels (wave-uniform)
    int live_b;
    {
        const int n = (p.M - (m0 + wm * WCH) + 15) >> 4;
        live_b = __builtin_amdgcn_readfirstlane(n < 0 ? 0 : (n > GB ? GB : n));
    }
    if (nk > 0) { fetch(); stage(0); if (nk > 1) fetch(); }
    __syncthreads();
    auto kloop = [&](auto nbt) {
        constexpr int NB = decltype(nbt)::value;
        auto step = [&](int kt, auto st, auto fe) {
            const unsigned char* bb = lds + (kt & 1) * BUFB;
            bf8 pf[GA], cf[GB > 0 ? GB : 1], pg[GA], cg[GB > 0 ? GB : 1], ch[GB > 0 ? GB : 1];
            if constexpr (NB > 0) {
#pragma unroll
                for (int a = 0; a < GA; ++a) pf[a] = *reinterpret_cast<const bf8*>(bb + rdP_hl + 512 * a);
#pragma unroll
                for (int b = 0; b < NB; ++b) cf[b] = *reinterpret_cast<const bf8*>(bb + rdC_lh + 512 * b);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int a = 0; a < GA; ++a)
#pragma unroll
                    for (int b = 0; b < NB; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf[a], cf[b], acc[a][b], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (decltype(st)::value) stage((kt & 1) ^ 1);
            if constexpr (decltype(fe)::value) fetch();
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (NB > 0) {
#pragma unroll
                for (int a = 0; a < GA; ++a) pg[a] = *reinterpret_cast<const bf8*>(bb + rdP_hm + 512 * a);
#pragma unroll
                for (int b = 0; b < NB; ++b) cg[b] = *reinterpret_cast<const bf8*>(bb + rdC_mm + 512 * b);
#pragma unroll
                for (int a = 0; a < GA; ++a)
#pragma unroll
                    for (int b = 0; b < NB; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pg[a], cg[b], acc[a][b], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int b = 0; b < NB; ++b) ch[b] = *reinterpret_cast<const bf8*>(bb + rdC_hh + 512 * b);
#pragma unroll
                for (int a = 0; a < GA; ++a)
#pragma unroll
                    for (int b = 0; b < NB; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pg[a], ch[b], acc[a][b], 0, 0, 0);
            }
            __syncthreads();
        };
        int kt = 0;
        for (; kt + 2 < nk; ++kt) step(kt, std::true_type{}, std::true_type{});
        if (kt + 1 < nk) { step(kt, std::true_type{}, std::false_type{}); ++kt; }
        if (kt < nk) step(kt, std::false_type{}, std::false_type{});
    };
    if (live_b == GB) kloop(std::integral_constant<int, GB>{});
    else if (live_b == 0) kloop(std::integral_constant<int, 0>{});
    else if (GB > 1 && live_b == 1) kloop(std::integral_constant<int, 1>{});
    else if (GB > 2 && live_b == 2) kloop(std::integral_constant<int, (GB > 2 ? 2 : 0)>{});
    else if (GB > 3 && live_b == 3) kloop(std::integral_constant<int, (GB > 3 ? 3 : 0)>{});

    // ---- epilogue: lane = output channel (16 b + lc of the wave's), acc[a][b][e] = pixel 16 a + 4 lq + e of the wave's 64 ----
    // (the lane's indices derived afresh from an opaque copy of the thread index: shared with the prologue's they stay live across the K loop; two VGPRs fewer on
    // every instance of this kernel, profiles/strided_paths.md section 1)
    int et = t;
    asm volatile("" : "+v"(et));
    const int elc = et & 15, elq = (et & 63) >> 4;
    const bool split = p.kchunk > 0;
    float* yout = p.Y + (split ? (size_t)blockIdx.y * p.slab_stride : 0);
    constexpr bool FWD_ONLY = SUMS == 1 || fx_epi_infer(EPI);        // (see fx_conv_kernel)
    const bool dense = FWD_ONLY || split || (p.oxs == 1 && p.oys == 1 && p.oy0 == 0 && p.ox0 == 0 && p.YW == p.OW && p.YH == p.OH);
    if constexpr (!FWD_ONLY) {
        if (!dense) {
            // a parity class of a strided data gradient: straight from the accumulator view, in a loop of its own (see fx_conv_kernel)
#pragma unroll
            for (int a = 0; a < GA; ++a) {
                const int c4 = n0 + wn * 64 + a * 16 + 4 * elq;
                if (c4 >= p.NP) continue;
                const int n = c4 / OHW, rem = c4 - n * OHW, oh = rem / p.OW, ow = rem - oh * p.OW;
#pragma unroll
                for (int b = 0; b < GB; ++b) {
                    const int m = m0 + wm * WCH + b * 16 + elc;
                    if (m >= p.M) continue;
                    f32x4 v = acc[a][b];
                    if (p.bias) { const float bb = p.bias[m]; v[0] += bb; v[1] += bb; v[2] += bb; v[3] += bb; }
                    float* dst = yout + (((size_t)n * p.M + m) * p.YH + p.oy0 + oh * p.oys) * p.YW + p.ox0 + ow * p.oxs;
                    if (p.emask) {              // (of a partial convolution: the factor of the input pixels this class writes)
                        const float* em = p.emask + ((size_t)n * p.YH + p.oy0 + oh * p.oys) * p.YW + p.ox0 + ow * p.oxs;
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] *= em[e * p.oxs];
                    }
                    if (p.oxs == 1) {
                        f32x4* d4 = reinterpret_cast<f32x4*>(dst);
                        if (p.accumulate) { const f32x4 o4 = *d4; v[0] += o4[0]; v[1] += o4[1]; v[2] += o4[2]; v[3] += o4[3]; }
                        *d4 = v;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) dst[e * p.oxs] = p.accumulate ? dst[e * p.oxs] + v[e] : v[e];
                    }
                }
            }
            return;
        }
    }
    float ssum[GB], ssq[GB], esc[GB], esh[GB], emean[GB];
#pragma unroll
    for (int b = 0; b < GB; ++b) {
        ssum[b] = ssq[b] = esc[b] = esh[b] = emean[b] = 0.f;
        if constexpr (SUMS == 2) {
            const int m = m0 + wm * WCH + b * 16 + elc;
            if (m < p.M) { esc[b] = p.ep_tab[8 * m]; esh[b] = p.ep_tab[8 * m + 1]; emean[b] = p.ep_tab[8 * m + 2]; }
        }
    }
#pragma unroll
    for (int a = 0; a < GA; ++a) {
        const int c4 = n0 + wn * 64 + a * 16 + 4 * elq;
        if (c4 >= p.NP) continue;
        const int n = c4 / OHW, rem = c4 - n * OHW, oh = rem / p.OW, ow = rem - oh * p.OW;
#pragma unroll
        for (int b = 0; b < GB; ++b) {
            const int m = m0 + wm * WCH + b * 16 + elc;
            if (m >= p.M) continue;
            f32x4 v = acc[a][b];
            if (!split) {
                if (p.bias) { const float bb = p.bias[m]; v[0] += bb; v[1] += bb; v[2] += bb; v[3] += bb; }
            }
            if (p.emask && !split) {            // partial convolution: the result times the per-pixel renormalisation factor (before any statistics are taken of it)
                const f32x4 em = *reinterpret_cast<const f32x4*>(p.emask + ((size_t)n * p.YH + oh) * p.YW + ow);
                v[0] *= em[0]; v[1] *= em[1]; v[2] *= em[2]; v[3] *= em[3];
            }
            acc[a][b] = v;
            if constexpr (SUMS == 1) {
                if (!split) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { ssum[b] += v[e]; ssq[b] = fmaf(v[e], v[e], ssq[b]); }
                }
            }
            if constexpr (SUMS == 2) {
                if (!split) {
                    const f32x4 c2 = *reinterpret_cast<const f32x4*>(p.ep_c + ((size_t)n * p.M + m) * OHW + rem);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float gg = fmaf(c2[e], esc[b], esh[b]) > 0.f ? v[e] : 0.f;
                        ssum[b] += gg; ssq[b] = fmaf(gg, c2[e] - emean[b], ssq[b]);
                    }
                }
            }
        }
    }
    if constexpr (SUMS == 1 || SUMS == 2) {
        if (!split) {
            // the four 16-lane groups hold different pixels of the same channels; the two waves along the pixel axis meet in LDS behind the staging tile (in
            // front of the staged store, whose barriers order these writes before the reads at the end: see fx_conv_kernel)
#pragma unroll
            for (int b = 0; b < GB; ++b) {
                ssum[b] += __shfl_xor(ssum[b], 16, 64); ssq[b] += __shfl_xor(ssq[b], 16, 64);
                ssum[b] += __shfl_xor(ssum[b], 32, 64); ssq[b] += __shfl_xor(ssq[b], 32, 64);
                if (elq == 0) { red[wn][0][wm * WCH + b * 16 + elc] = ssum[b]; red[wn][1][wm * WCH + b * 16 + elc] = ssq[b]; }
            }
        }
    }
    {
        // through a [64 channels][128 pixels] staging tile, 32 channels of each wave row per round (see fx_conv_kernel)
        constexpr int EROW = 512 + 16;
        constexpr int ROUNDS = (GB + 1) / 2;
        const bool accum = !split && p.accumulate;
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            if (r > 0) __syncthreads();
#pragma unroll
            for (int b2 = 0; b2 < 2; ++b2) {
                const int b = 2 * r + b2;
                if (b < GB) {
#pragma unroll
                    for (int a = 0; a < GA; ++a)
                        *reinterpret_cast<f32x4*>(lds + (wm * 32 + b2 * 16 + elc) * EROW + (wn * 64 + a * 16 + 4 * elq) * 4) = acc[a][b < GB ? b : 0];
                }
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int id = et + 256 * i, row = id >> 5, q = id & 31;
                const int within = r * 32 + (row & 31);
                const int m = m0 + (row >> 5) * WCH + within;
                const int c4 = n0 + 4 * q;
                if (within >= WCH || m >= p.M || c4 >= p.NP) continue;
                const int n = c4 / OHW, rem = c4 - n * OHW;
                f32x4 v = *reinterpret_cast<const f32x4*>(lds + row * EROW + q * 16);
                const size_t at = ((size_t)n * p.M + m) * OHW + rem;
                f32x4* dst = reinterpret_cast<f32x4*>(yout + at);
                if (accum) {
                    f32x4 o4;
                    if (p.acc_src) {
                        o4 = *reinterpret_cast<const f32x4*>(p.acc_src + at);
                        if (p.acc_mask) {
                            const unsigned mk = p.acc_mask[at >> 2];
#pragma unroll
                            for (int e = 0; e < 4; ++e) o4[e] = (mk >> e) & 1u ? o4[e] : 0.f;
                        }
                    } else o4 = *dst;
                    v[0] += o4[0]; v[1] += o4[1]; v[2] += o4[2]; v[3] += o4[3];
                }
                if constexpr (fx_epi_infer(EPI)) {
                    if (p.ep_res) { const f32x4 r4 = *reinterpret_cast<const f32x4*>(p.ep_res + at); v[0] += r4[0]; v[1] += r4[1]; v[2] += r4[2]; v[3] += r4[3]; }
                    if (p.ep_relu) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
                }
                *dst = v;
            }
        }
    }
    if constexpr (SUMS == 1 || SUMS == 2) {
        if (!split) {
            if (et < BM && m0 + et < p.M) {
                float* dst = p.partial + ((size_t)tile_n * p.M + m0 + et) * 2;
                dst[0] = red[0][0][et] + red[1][0][et];
                dst[1] = red[0][1][et] + red[1][1][et];
            }
        }
    }
}

// y (=|+=) sum over the split-K slabs (+ bias); SUMS as in fx_conv_kernel (0 / 1 / 2): per-(chunk, channel) partial sums.  One block per (channel m, image group):
// grid (M, ngroups), block z handles images n = z, z + ngroups, ...; the partial index is the group.
template <int SUMS>
__global__ __launch_bounds__(256) void fx_reduce_kernel(const float* __restrict__ slabs, float* __restrict__ y, const float* __restrict__ bias, int nsplit,
                                                        size_t slab_stride, int N, int M, int OHW, int accumulate, const float* __restrict__ ep_c,
                                                        const float* __restrict__ ep_tab, float* __restrict__ partial, const float* __restrict__ emask,
                                                        const float* __restrict__ res, int relu) {
    const int m = blockIdx.x, grp = blockIdx.y, ngrp = gridDim.y;
    const float bb = bias ? bias[m] : 0.f;
    float esc = 0.f, esh = 0.f, emean = 0.f;
    if constexpr (SUMS == 2) { esc = ep_tab[8 * m]; esh = ep_tab[8 * m + 1]; emean = ep_tab[8 * m + 2]; }
    float s1 = 0.f, s2 = 0.f;
    const int q4 = OHW >> 2;
    for (int n = grp; n < N; n += ngrp) {
        const size_t base = ((size_t)n * M + m) * OHW;
        for (int i = threadIdx.x; i < q4; i += 256) {
            f32x4 v = *reinterpret_cast<const f32x4*>(slabs + base + 4 * i);
            for (int z = 1; z < nsplit; ++z) {
                const f32x4 u = *reinterpret_cast<const f32x4*>(slabs + (size_t)z * slab_stride + base + 4 * i);
                v[0] += u[0]; v[1] += u[1]; v[2] += u[2]; v[3] += u[3];
            }
            if (emask && bias) {
                // folded partial convolution at inference (FX_EPI_INFER_FACTOR): the factor first, then b', so that an empty window (factor 0) gives b'.  Only this pairing takes
                // the order: the training instances pass no bias with a factor, and their (v + 0) * em keeps the sign of a zero that v * em + 0 would not.
                const f32x4 em = *reinterpret_cast<const f32x4*>(emask + (size_t)n * OHW + 4 * i);
                v[0] = v[0] * em[0] + bb; v[1] = v[1] * em[1] + bb; v[2] = v[2] * em[2] + bb; v[3] = v[3] * em[3] + bb;
            } else {
                v[0] += bb; v[1] += bb; v[2] += bb; v[3] += bb;
                if (emask) {         // partial convolution: the per-pixel factor of the result (the split launches carry no epilogue)
                    const f32x4 em = *reinterpret_cast<const f32x4*>(emask + (size_t)n * OHW + 4 * i);
                    v[0] *= em[0]; v[1] *= em[1]; v[2] *= em[2]; v[3] *= em[3];
                }
            }
            f32x4* dst = reinterpret_cast<f32x4*>(y + base + 4 * i);
            if (accumulate) { const f32x4 o = *dst; v[0] += o[0]; v[1] += o[1]; v[2] += o[2]; v[3] += o[3]; }
            if (res) { const f32x4 r4 = *reinterpret_cast<const f32x4*>(res + base + 4 * i); v[0] += r4[0]; v[1] += r4[1]; v[2] += r4[2]; v[3] += r4[3]; }      // inference
            if (relu) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
            *dst = v;
            if constexpr (SUMS == 1) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { s1 += v[e]; s2 = fmaf(v[e], v[e], s2); }
            }
            if constexpr (SUMS == 2) {
                const f32x4 c2 = *reinterpret_cast<const f32x4*>(ep_c + base + 4 * i);
#pragma unroll
                for (int e = 0; e < 4; ++e) { const float gg = fmaf(c2[e], esc, esh) > 0.f ? v[e] : 0.f; s1 += gg; s2 = fmaf(gg, c2[e] - emean, s2); }
            }
        }
    }
    if constexpr (SUMS != 0) {
        __shared__ float r1[4], r2[4];
        s1 = wave_sum(s1); s2 = wave_sum(s2);
        if ((threadIdx.x & 63) == 0) { r1[threadIdx.x >> 6] = s1; r2[threadIdx.x >> 6] = s2; }
        __syncthreads();
        if (threadIdx.x == 0) {
            float* dst = partial + ((size_t)grp * M + m) * 2;
            dst[0] = r1[0] + r1[1] + r1[2] + r1[3];
            dst[1] = r2[0] + r2[1] + r2[2] + r2[3];
        }
    }
}

// The same sum for the ragged forward (fx_conv_kernel's RAG instances: OHW is no multiple of 4, so no channel row is 16-B aligned): one element per thread,
// y (=|+=) sum over the slabs (* emask) + bias (+ res) (then ReLU), in the order of the vector kernel.  total = N * M * OHW.
__global__ __launch_bounds__(256) void fx_reduce_any_kernel(const float* __restrict__ slabs, float* __restrict__ y, const float* __restrict__ bias, int nsplit,
                                                            size_t slab_stride, unsigned total, int M, int OHW, int accumulate, const float* __restrict__ emask,
                                                            const float* __restrict__ res, int relu) {
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        float v = slabs[i];
        for (int z = 1; z < nsplit; ++z) v += slabs[(size_t)z * slab_stride + i];
        if (emask) {         // folded partial convolution: the factor [N][1][OH][OW] first, then b' (an empty window gives b'), as fx_reduce_kernel
            const float em = emask[(size_t)(i / ((unsigned)M * (unsigned)OHW)) * OHW + i % (unsigned)OHW];
            v = v * em + (bias ? bias[(i / (unsigned)OHW) % (unsigned)M] : 0.f);
        } else if (bias) v += bias[(i / (unsigned)OHW) % (unsigned)M];
        if (accumulate) v += y[i];
        if (res) v += res[i];
        if (relu) v = fmaxf(v, 0.f);
        y[i] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------------
// WGRAD: dw[k][c][tap] = sum over images n and output pixels p of dyeff[n][k][p] * xeff[n][c][p at tap]
// A K step is 16 consecutive output pixels of one image (OHW % 16 == 0).  grid (C tiles, K tiles, taps * splits); slabs [split][k][tap][c] ("tap-major
// columns", what wgrad_reduce_tapm_kernel of p3d_conv.hip sums and transposes) or, for 1x1, [split][k][c].
// An fp32 operand (AIMG / BIMG false) is contiguous along the reduction (pixel) index: a thread fetches 4 pixels for two rows and splits them ("rc" image,
// rows = channels).  An image operand is contiguous along the channels: a thread copies one 16-B chunk (pixel of the step, 8 channels) per plane ("tr" image,
// rows = the step's 16 pixels, read through ds_read_b64_tr_b16).
// MASKED (partial convolution, fp32 operands only): dy * amask[output pixel], x * bmask[input pixel].
// ------------------------------------------------------------------------------------------------------------------------------------------
// TAPS (the 7x7 stride-2 stem restated as a 4x4 stride-1 convolution over a space-to-depth image with ONE 16-channel group: fx_stem_*): the columns of the
// GEMM are (filter tap, channel) pairs, a 128-column tile = eight taps, and what is a channel group for an ordinary image operand is a tap here: the thread's
// chunk is the pixel's one 32-B row, fetched at the tap's offset.  grid (taps / 8, K tiles, splits); slabs [split][k][taps * 16].
// TAPS 2 (image-fed 64-input-channel layers with a multi-tap filter: ResNet-50's layer1 3x3, ResNet-18's): a 128-column tile = TWO filter taps x 64 channels, so a 64 x 64
// weight block per tap no longer leaves three of the four waves without work (both column waves live).  grid (ceil(taps / 2), K tiles, splits); slabs as ever.
// TAPS 3 (the same with at most 64 OUTPUT channels too -- every 3x3 of ResNet-50's layer1 and ResNet-18's): dy fills half of the A image, the other half carries a third tap of
// x, and three of the four waves multiply dy by one tap each (one block = one filter row of a 3x3).  grid (ceil(taps / 3), 1, splits).
// ROWS: every image operand is an fp32 row image [N][C/16][HW][16]; the thread's chunk (one pixel, eight channels) is 32 B of the pixel's 64-B row, fetched as two 16-B
// groups and cut into the three pieces between the fetch registers and the "tr" image (fx_split_row8): the same stores to the same addresses.
template <bool AIMG, bool BIMG, bool MASKED, int TAPS = 0, bool ROWS = false>
__global__ __launch_bounds__(256, 3) void fx_wgrad_kernel(const FxWgradParams p) {
    static_assert(!ROWS || (AIMG && !MASKED && TAPS != 1), "row images feed the dense image-fed instances (not the stem's)");
    static_assert(TAPS < 2 || (AIMG && BIMG && !MASKED), "the multi-tap column tiles are image-fed instances");
    static_assert(!MASKED || !AIMG || !BIMG, "the partial-convolution factors are applied by the in-kernel split of an fp32 operand (an image carries its factor already)");
    static_assert(!TAPS || BIMG, "tap-major columns come from an image operand");
    __shared__ __attribute__((aligned(16))) unsigned char As[2 * 3 * FX_PIECE];
    __shared__ __attribute__((aligned(16))) unsigned char Bs[2 * 3 * FX_PIECE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1;
    // XCD-aware block order (the bijective remap of fx_conv_kernel): consecutive linear block ids go to different XCDs, so in grid order the blocks that share
    // a dy tile or an x tile would each fetch it into a different L2.  Logical order: channel tile fastest, then output-channel tile, then filter tap, the
    // pixel slab slowest -- every XCD works through a contiguous run of it, i.e. the tiles of one or two slabs, whose operands its L2 then holds once.
    int bx, by, bz;
    {
        const int gx = gridDim.x, gy = gridDim.y, nwg = gx * gy * gridDim.z;
        const int lin = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
        const int q = nwg >> 3, r = nwg & 7, xcd = lin & 7, idx = lin >> 3;
        const int bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
        if (p.order == 0 || TAPS) {
            bx = bid % gx;
            const int rest = bid / gx;
            by = rest % gy;
            bz = rest / gy;
        } else {
            // filter tap fastest, then the output-channel tile, then the input-channel tile, the pixel slab slowest: the blocks an XCD holds at one time read few x
            // tiles (the taps of one tile are shifted views of the same lines) -- for a wide input and few output channels (the 2048 -> 272 regressor: 27 blocks per
            // x tile) that is what keeps x from being fetched once per (output-channel tile, tap)
            const int nt = p.R * p.S;
            const int tp = bid % nt;
            int rest = bid / nt;
            by = rest % gy; rest /= gy;
            bx = rest % gx;
            bz = (rest / gx) * nt + tp;
        }
    }
    const int m0 = by * FX_BM, n0 = bx * FX_BN;
    const int ntaps = TAPS ? 1 : p.R * p.S;
    const int split = bz / ntaps, tap = bz - split * ntaps;
    const int tr = tap / p.S, ts = tap - tr * p.S;
    const int dh = tr * p.dil - p.pad, dw = ts * p.dil - p.pad;             // input coordinate = output coordinate * stride + (dh, dw)
    const int OHW = p.OH * p.OW, HWi = p.Hi * p.Wi;
    const int steps_per_img = OHW / FX_BK;
    const int total = p.N * steps_per_img;
    const int s0 = split * p.spb, s1 = (s0 + p.spb < total) ? s0 + p.spb : total;
    const int nk = s1 - s0;
    // fp32 operands: rows row, row + 64 of the tile, pixels 4 kq .. 4 kq + 3 of the step.  Image operands: pixel ipix of the step, channel group icg of the
    // tile's eight, 16-B half ih of the group's 32-B row.
    const int row = t >> 2, kq = t & 3;
    // (the pixel's bits are permuted so that the eight lanes of a ds_write_b128 group hold pixels {p, p + 1, p + 8, p + 9}: with consecutive pixels two of
    // the group's 16-B chunks share a bank quad of the "tr" image)
    const int ih = t & 1, ipix = ((t >> 1) & 1) | (((t >> 3) & 3) << 1) | (((t >> 2) & 1) << 3), icg = t >> 5;
    const bool a_ok[2] = {m0 + row < p.K, m0 + row + 64 < p.K}, b_ok[2] = {n0 + row < p.C, n0 + row + 64 < p.C};
    const int KG = p.K >> 4, CG = TAPS == 1 ? 1 : p.C >> 4;
    // TAPS 1 / 2: this thread's filter tap (one per 16-column / 64-column group of the tile) and its input offset
    const int t_tap = TAPS >= 2 ? TAPS * bx + (icg >> 2) : (n0 >> 4) + icg;
    const int t_dh = (t_tap / p.S) * p.dil - p.pad, t_dw = (t_tap - (t_tap / p.S) * p.S) * p.dil - p.pad;
    const int a_cg = (m0 >> 4) + icg, b_cg = TAPS == 1 ? 0 : TAPS >= 2 ? (icg & 3) : (n0 >> 4) + icg;
    const bool ai_ok = a_cg < KG, bi_ok = TAPS == 1 ? true : TAPS >= 2 ? t_tap < p.R * p.S : b_cg < CG;
    // TAPS 3 (64 output AND 64 input channels): dy fills only columns 0-63 of the A image, so its columns 64-127 carry a THIRD tap of x (fetched by waves 2 and 3, whose
    // threads own those columns' chunks); waves 0, 1, 2 each multiply dy by one tap's 64 channels, wave 3 only stages
    const int a3_tap = 3 * bx + 2;
    const int a3_dh = (a3_tap / p.S) * p.dil - p.pad, a3_dw = (a3_tap - (a3_tap / p.S) * p.S) * p.dil - p.pad;
    const bool a3_ok = a3_tap < p.R * p.S;
    // Buffer-load fetch (see fx_conv_kernel): per-thread byte offsets with the out-of-range bit for rows beyond the tensor / padding pixels, the image and
    // pixel position of the K step in a wave-uniform scalar offset.  (fx_applies(FX_WGRAD) bounds every tensor below 2^29 elements.)
    i32x4 rA, rB, rAi[3], rBi[3];
    constexpr int RB = ROWS ? 64 : 32, RH = ROWS ? 32 : 16;          // bytes of a pixel's row of 16 channels in an image (plane), and of a thread's half of it
    if constexpr (AIMG && ROWS) rAi[0] = fx_rsrc(p.DYimg, (size_t)p.N * p.K * OHW * 4);
    else if constexpr (AIMG) {
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) rAi[pc] = fx_rsrc(p.DYimg + pc * p.dy_plane, (size_t)p.N * p.K * OHW * 2);
    } else rA = fx_rsrc(p.DY, (size_t)p.N * p.K * OHW * sizeof(float));
    if constexpr (BIMG && ROWS) rBi[0] = fx_rsrc(p.Ximg, (size_t)p.N * p.C * HWi * 4);
    else if constexpr (BIMG) {
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) rBi[pc] = fx_rsrc(p.Ximg + pc * p.x_plane, (size_t)p.N * (TAPS == 1 ? 16 : p.C) * HWi * 2);
    } else rB = fx_rsrc(p.X, (size_t)p.N * p.C * HWi * sizeof(float));
    const i32x4 rAM = fx_rsrc(MASKED && !AIMG ? p.amask : nullptr, MASKED && !AIMG ? (size_t)p.N * OHW * sizeof(float) : 0);
    const i32x4 rBM = fx_rsrc(MASKED && !BIMG ? p.bmask : nullptr, MASKED && !BIMG ? (size_t)p.N * HWi * sizeof(float) : 0);
    int a_voff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) a_voff[i] = a_ok[i] ? ((m0 + row + 64 * i) * OHW + 4 * kq) * 4 : FX_OOB;
    const int ai_voff = ai_ok ? (a_cg * OHW + ipix) * RB + RH * ih : FX_OOB;
    const bool simple = p.R == 1 && p.S == 1 && p.stride == 1 && p.pad == 0;      // 1x1: the input pixel IS the output pixel
    const bool vec = p.stride == 1 && (dw & 3) == 0;        // uniform: the four input pixels are one aligned 16-B group, in or out together
    const int b_row = (n0 + row) * HWi;
    f32x4 ra[2], rb[2];          // (ROWS: an image operand's 32 B of the pixel's row)
    i32x4 rai[3], rbi[3];
    f32x4 ram, rbm;              // MASKED: the per-pixel factors of the fetched K step (one value per pixel, whatever the row)
    int b_voff[4] = {FX_OOB, FX_OOB, FX_OOB, FX_OOB};
    int f_img = s0 / steps_per_img, f_p = (s0 - f_img * steps_per_img) * FX_BK;
    const bool rowwise = (p.OW & (FX_BK - 1)) == 0;        // uniform: a K step never straddles two output rows
    int f_oh = f_p / p.OW, f_ow = f_p - f_oh * p.OW;       // rowwise: the step's output row and first column (scalars)
    const int tw = 4 * kq * p.stride + dw;
    auto fetch = [&]() {
        // operand A (dy)
        if constexpr (AIMG) {
            if (TAPS == 3 && wave >= 2) {                 // (wave-uniform) columns 64-127 of the A image: x at the third tap of the block
                int hi, wi;
                if (rowwise) { hi = f_oh * p.stride + a3_dh; wi = (f_ow + ipix) * p.stride + a3_dw; }
                else { const int q = f_p + ipix, oh = q / p.OW, ow = q - oh * p.OW; hi = oh * p.stride + a3_dh; wi = ow * p.stride + a3_dw; }
                const int voff = (a3_ok && (unsigned)hi < (unsigned)p.Hi && (unsigned)wi < (unsigned)p.Wi) ? ((icg & 3) * HWi + hi * p.Wi + wi) * RB + RH * ih : FX_OOB;
                const int x_so = f_img * CG * HWi * RB;
                if constexpr (ROWS) {
#pragma unroll
                    for (int i = 0; i < 2; ++i) ra[i] = fx_buffer_load_f32x4(rBi[0], voff, x_so + 16 * i, 0);
                } else {
#pragma unroll
                    for (int pc = 0; pc < 3; ++pc) rai[pc] = fx_buffer_load_i32x4(rBi[pc], voff, x_so, 0);
                }
            } else {
                const int a_so = (f_img * KG * OHW + f_p) * RB;
                if constexpr (ROWS) {
#pragma unroll
                    for (int i = 0; i < 2; ++i) ra[i] = fx_buffer_load_f32x4(rAi[0], ai_voff, a_so + 16 * i, 0);
                } else {
#pragma unroll
                    for (int pc = 0; pc < 3; ++pc) rai[pc] = fx_buffer_load_i32x4(rAi[pc], ai_voff, a_so, 0);
                }
            }
        } else {
            const int a_so = (f_img * p.K * OHW + f_p) * 4;
#pragma unroll
            for (int i = 0; i < 2; ++i) ra[i] = fx_buffer_load_f32x4(rA, a_voff[i], a_so, 0);
            if constexpr (MASKED) ram = fx_buffer_load_f32x4(rAM, 16 * kq, (f_img * OHW + f_p) * 4, 0);
        }
        // operand B (x at this block's filter tap)
        if constexpr (BIMG) {
            int b_so = f_img * CG * HWi * RB, voff;
            if (!TAPS && simple) { b_so += f_p * RB; voff = bi_ok ? (b_cg * HWi + ipix) * RB + RH * ih : FX_OOB; }
            else {
                int hi, wi;
                const int tdh = TAPS ? t_dh : dh, tdw = TAPS ? t_dw : dw;
                if (rowwise) { hi = f_oh * p.stride + tdh; wi = (f_ow + ipix) * p.stride + tdw; }        // the step's 16 pixels lie in output row f_oh (a scalar)
                else { const int q = f_p + ipix, oh = q / p.OW, ow = q - oh * p.OW; hi = oh * p.stride + tdh; wi = ow * p.stride + tdw; }
                voff = (bi_ok && (unsigned)hi < (unsigned)p.Hi && (unsigned)wi < (unsigned)p.Wi) ? (b_cg * HWi + hi * p.Wi + wi) * RB + RH * ih : FX_OOB;
            }
            if constexpr (ROWS) {
#pragma unroll
                for (int i = 0; i < 2; ++i) rb[i] = fx_buffer_load_f32x4(rBi[0], voff, b_so + 16 * i, 0);
            } else {
#pragma unroll
                for (int pc = 0; pc < 3; ++pc) rbi[pc] = fx_buffer_load_i32x4(rBi[pc], voff, b_so, 0);
            }
        } else {
            int b_so = f_img * p.C * HWi * 4;
            if (simple) {
                b_so += f_p * 4;
#pragma unroll
                for (int e = 0; e < 4; ++e) b_voff[e] = (b_row + 4 * kq + e) * 4;
            } else {
                int hi, wi0;
                if (rowwise) { hi = f_oh * p.stride + dh; wi0 = f_ow * p.stride + tw; }       // per thread, one add and one range check per pixel
                else { const int q = f_p + 4 * kq, oh = q / p.OW, ow = q - oh * p.OW; hi = oh * p.stride + dh; wi0 = ow * p.stride + dw; }
                const bool row_ok = (unsigned)hi < (unsigned)p.Hi;
                const int base = (b_row + hi * p.Wi + wi0) * 4;
#pragma unroll
                for (int e = 0; e < 4; ++e) b_voff[e] = (row_ok && (unsigned)(wi0 + e * p.stride) < (unsigned)p.Wi) ? base + e * p.stride * 4 : FX_OOB;
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int so = b_so + i * 64 * HWi * 4;
                const int rowbad = b_ok[i] ? 0 : FX_OOB;
                if (vec) rb[i] = fx_buffer_load_f32x4(rB, b_voff[0] | rowbad, so, 0);
                else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) rb[i][e] = fx_buffer_load_f32(rB, b_voff[e] | rowbad, so, 0);
                }
            }
            if constexpr (MASKED) {        // the factor at the four input pixels: the x offsets without the channel row
                const int mso = b_so - f_img * (p.C - 1) * HWi * 4;
                if (vec) rbm = fx_buffer_load_f32x4(rBM, b_voff[0] >= 0 ? b_voff[0] - b_row * 4 : FX_OOB, mso, 0);
                else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) rbm[e] = fx_buffer_load_f32(rBM, b_voff[e] >= 0 ? b_voff[e] - b_row * 4 : FX_OOB, mso, 0);
                }
            }
        }
        if ((TAPS || !simple) && rowwise) {
            f_ow += FX_BK;
            if (f_ow == p.OW) { f_ow = 0; ++f_oh; if (f_oh == p.OH) f_oh = 0; }
        }
        f_p += FX_BK;
        if (f_p == OHW) { f_p = 0; ++f_img; }
    };
    const int st_off[2] = {fx_rc_off(row, kq >> 1) + 8 * (kq & 1), fx_rc_off(row + 64, kq >> 1) + 8 * (kq & 1)};
    const int st_img = fx_tr_off(ipix, 2 * icg + ih);
    auto stage = [&](int buf) {
        unsigned char* ab = As + buf * 3 * FX_PIECE;
        unsigned char* bb = Bs + buf * 3 * FX_PIECE;
        if constexpr (AIMG) {
            if constexpr (ROWS) fx_split_row8(ra[0], ra[1], rai);
#pragma unroll
            for (int pc = 0; pc < 3; ++pc) *reinterpret_cast<i32x4*>(ab + pc * FX_PIECE + st_img) = rai[pc];
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                f32x4 va = ra[i];
                if constexpr (MASKED) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) va[e] *= ram[e];
                }
                fx_split_store(ab + st_off[i], va);
            }
        }
        if constexpr (BIMG) {
            if constexpr (ROWS) fx_split_row8(rb[0], rb[1], rbi);
#pragma unroll
            for (int pc = 0; pc < 3; ++pc) *reinterpret_cast<i32x4*>(bb + pc * FX_PIECE + st_img) = rbi[pc];
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                f32x4 vb = rb[i];
                if constexpr (MASKED) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) vb[e] *= rbm[e];
                }
                fx_split_store(bb + st_off[i], vb);
            }
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    const int fr = lane & 31, fh = lane >> 5;
    int rd_a[2][2], rd_b[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        if constexpr (AIMG) fx_tr_frag_off(lane, (TAPS == 3 ? 0 : wm * 64) + a * 32, rd_a[a]);      // (TAPS 3: every wave's rows are dy's 64 channels)
        else rd_a[a][0] = rd_a[a][1] = fx_rc_off(wm * 64 + a * 32 + fr, fh);
        if constexpr (BIMG) fx_tr_frag_off(lane, (TAPS == 3 ? (wave ? 64 : 0) : wn * 64) + a * 32, rd_b[a]);      // (TAPS 3: wave 1 the second tap of Bs, wave 2 the tap in As)
        else rd_b[a][0] = rd_b[a][1] = fx_rc_off(wn * 64 + a * 32 + fr, fh);
    }
    const int live_a = TAPS == 3 ? (wave < 3 ? fx_live_subtiles(m0, p.K) : 0) : fx_live_subtiles(m0 + wm * 64, p.K);
    const int live_b = TAPS == 3 ? (wave < 3 && 3 * bx + wave < p.R * p.S ? 2 : 0)
                     : TAPS == 2 ? (2 * bx + wn < p.R * p.S ? 2 : 0) : fx_live_subtiles(n0 + wn * 64, p.C);      // (TAPS 2 / 3: a column wave = one tap's 64 channels)
    const unsigned char* const Bsrc = (TAPS == 3 && wave == 2) ? As : Bs;
    if (nk > 0) { fetch(); stage(0); if (nk > 1) fetch(); }       // software pipeline as in fx_conv_kernel: stage step kt + 1 at the head of step kt, fetch step kt + 2
    __syncthreads();
    auto kloop = [&](auto nat, auto nbt) {             // see fx_conv_kernel: one straight-line copy of the loop per count of live sub-tiles
        constexpr int NA = decltype(nat)::value, NB = decltype(nbt)::value;
        constexpr bool LIVE = NA > 0 && NB > 0;
        auto step = [&](int kt, auto st, auto fe) {
            const int buf = kt & 1;
            bf8 af[3][2], bf[3][2];
            auto read_a = [&](int pc) {
#pragma unroll
                for (int a = 0; a < 2; ++a)
                    if (a < NA) {
                        if constexpr (AIMG) af[pc][a] = fx_tr_read(As + (buf * 3 + pc) * FX_PIECE, rd_a[a]);
                        else af[pc][a] = *reinterpret_cast<const bf8*>(As + (buf * 3 + pc) * FX_PIECE + rd_a[a][0]);
                    }
            };
            auto read_b = [&](int pc) {
#pragma unroll
                for (int a = 0; a < 2; ++a)
                    if (a < NB) {
                        if constexpr (BIMG) bf[pc][a] = fx_tr_read(Bsrc + (buf * 3 + pc) * FX_PIECE, rd_b[a]);
                        else bf[pc][a] = *reinterpret_cast<const bf8*>(Bs + (buf * 3 + pc) * FX_PIECE + rd_b[a][0]);
                    }
            };
            if constexpr (LIVE) {                                   // order of a step: see fx_conv_kernel
                read_a(2); read_b(0); read_a(0); read_b(2);
                __builtin_amdgcn_sched_barrier(0);
                P3D_FX_PRODUCTS_RANGE(acc, af, bf, NA, NB, 0, 1)
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (decltype(st)::value) stage(buf ^ 1);
            if constexpr (decltype(fe)::value) fetch();
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (LIVE) {
                read_a(1); read_b(1);
                P3D_FX_PRODUCTS_RANGE(acc, af, bf, NA, NB, 1, 6)
            }
            __syncthreads();
        };
        int kt = 0;
        for (; kt + 2 < nk; ++kt) step(kt, std::true_type{}, std::true_type{});
        if (kt + 1 < nk) { step(kt, std::true_type{}, std::false_type{}); ++kt; }
        if (kt < nk) step(kt, std::false_type{}, std::false_type{});
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    if (live_a == 0 || live_b == 0) kloop(I0{}, I0{});
    else if (live_a == 2 && live_b == 2) kloop(I2{}, I2{});
    else if (live_a == 1 && live_b == 2) kloop(I1{}, I2{});
    else if (live_a == 2 && live_b == 1) kloop(I2{}, I1{});
    else kloop(I1{}, I1{});
    // C/D layout: col = lane & 31 (input channel c, contiguous in the slab), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (output channel k)
    const int RS = TAPS == 1 ? 1 : p.R * p.S;
    float* out = p.slabs + (size_t)split * p.K * p.C * RS;
    // (TAPS 2 / 3: the wave's tap; its 64 columns are the layer's 64 input channels.  Wave 3 of a three-tap block holds nothing)
    const int otap = TAPS == 3 ? (wave < 3 ? 3 * bx + wave : RS) : TAPS == 2 ? 2 * bx + wn : tap;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int c = TAPS >= 2 ? b * 32 + fr : n0 + wn * 64 + b * 32 + fr;
            if (c >= p.C || otap >= RS) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = m0 + (TAPS == 3 ? 0 : wm * 64) + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
                if (k < p.K) out[((size_t)k * RS + otap) * p.C + c] = acc[a][b][r];
            }
        }
}

// The ragged weight gradient (p3d_x3_any_enable): fx_wgrad_kernel<false, false, false> -- both operands fp32 NCHW, unmasked, one tap per block -- without
// OHW % 16 == 0, OW % 4 == 0 and Wi % 4 == 0.  The reduction index stays the flat pixel n OHW + oh OW + ow in K steps of 16 (the columns of the ragged forward), slabs cut it
// at multiples of 16, so a step may straddle two images, a thread's four pixels an output row or an image, and the last step of the last slab may run beyond N OHW.
// A thread keeps its FIRST pixel as (output row, output column, flat index, element offsets of its rows in dy's and x's image); every fetch steps four pixels from it
// through row ends and image ends (the walk of fx_conv_kernel's RAG set_tap) into eight independent byte offsets, each with the out-of-range bit for padding and for
// pixels at or beyond N OHW -- those contribute exact zero through BOTH operands, and the resources keep the tensors' exact sizes -- then moves 16 pixels on
// (16 = di images + dr rows + dc columns, one conditional carry each: no division and no loop in the K loop).  Every fetch is a dword load: with OHW odd a channel's run of
// dy is only 4-B aligned.  LDS images, the pixel permutation of the stores, block order, partial tiles and the slab layout are fx_wgrad_kernel's.
// (A kernel of its own rather than a fifth template axis of fx_wgrad_kernel: none of that kernel's image-fed / masked / multi-tap branches applies, and its
// instances keep their symbols and their code.)
// MASKED (p3d_x3_any_partial_enable: the weight gradient of a partial convolution, dw = wgrad(dy * amask, x * bmask)): the factors are fetched in the same walk, one
// dword per pixel and operand whatever the row.  amask has one plane per image, so the factor of flat pixel q is element q; bmask's sits at the x offset without
// the channel row, its image offset carried beside x's.  A factor's offset has the out-of-range bit exactly where its operand's has, and the factor resources keep
// their exact sizes, so a pixel beyond N OHW or a padding tap is 0 * 0.  The products are taken before the three-piece split, as in fx_wgrad_kernel<.., MASKED>.
// (One text, p3d_fx_wgrad_any.h, read once per kernel rather than a kernel template or a shared body: the unmasked kernel keeps its symbol and its code.)
#define P3D_FX_WGRAD_ANY_KERNEL fx_wgrad_any_kernel
#define P3D_FX_WGRAD_ANY_MASKED false
#include "p3d_fx_wgrad_any.h"
#undef P3D_FX_WGRAD_ANY_KERNEL
#undef P3D_FX_WGRAD_ANY_MASKED
#define P3D_FX_WGRAD_ANY_KERNEL fx_wgrad_any_masked_kernel
#define P3D_FX_WGRAD_ANY_MASKED true
#include "p3d_fx_wgrad_any.h"
#undef P3D_FX_WGRAD_ANY_KERNEL
#undef P3D_FX_WGRAD_ANY_MASKED

// The image-fed ragged weight gradient (p3d_x3_any_images_enable): fx_wgrad_kernel<true, true, false> -- both operands activation images, one tap per block -- over
// the K steps of fx_wgrad_any_kernel: 16 consecutive values of the flat pixel index n OHW + oh OW + ow, the last step partial, a step free to span a row end or an image
// end.  An image operand is per pixel already: a thread copies ONE pixel's 16-B chunk (8 channels of one of the tile's eight channel groups) per plane, operand and
// step, no split and no four-pixel walk.  It keeps its pixel as (image, output row, output column) and moves
// 16 pixels on per step with one conditional carry per level (16 = di images + dr rows + dc columns; OHW >= 16, so di <= 1: p3d_fx_conv_img_any_supported refuses
// smaller maps) -- no division in the loop.  A pixel at or beyond N OHW, or one whose tap falls into the padding, carries the out-of-range bit on BOTH operands: 0 * 0,
// whatever the other operand holds, and the resources keep the images' exact sizes.  The LDS "tr" images, the pixel permutation of the chunk stores, the XCD block
// order, the partial tiles and the slab layout are fx_wgrad_kernel's.  (A kernel of its own, like fx_wgrad_any_kernel: that kernel's instances keep their code.)
__global__ __launch_bounds__(256, 3) void fx_wgrad_any_img_kernel(const FxWgradParams p) {
    __shared__ __attribute__((aligned(16))) unsigned char As[2 * 3 * FX_PIECE];
    __shared__ __attribute__((aligned(16))) unsigned char Bs[2 * 3 * FX_PIECE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1;
    int bx, by, bz;              // the XCD block order of fx_wgrad_kernel
    {
        const int gx = gridDim.x, gy = gridDim.y, nwg = gx * gy * gridDim.z;
        const int lin = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
        const int q = nwg >> 3, r = nwg & 7, xcd = lin & 7, idx = lin >> 3;
        const int bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
        if (p.order == 0) {
            bx = bid % gx;
            const int rest = bid / gx;
            by = rest % gy;
            bz = rest / gy;
        } else {
            const int nt = p.R * p.S;
            const int tp = bid % nt;
            int rest = bid / nt;
            by = rest % gy; rest /= gy;
            bx = rest % gx;
            bz = (rest / gx) * nt + tp;
        }
    }
    const int m0 = by * FX_BM, n0 = bx * FX_BN;
    const int ntaps = p.R * p.S;
    const int split = bz / ntaps, tap = bz - split * ntaps;
    const int tr = tap / p.S, ts = tap - tr * p.S;
    const int dh = tr * p.dil - p.pad, dw = ts * p.dil - p.pad;             // input coordinate = output coordinate * stride + (dh, dw)
    const int OHW = p.OH * p.OW, HWi = p.Hi * p.Wi, NP = p.N * OHW;
    const int total = (NP + FX_BK - 1) / FX_BK;                              // the last K step may hold fewer than 16 pixels
    const int s0 = split * p.spb, s1 = (s0 + p.spb < total) ? s0 + p.spb : total;
    const int nk = s1 > s0 ? s1 - s0 : 0;                                    // (a slab beyond the range writes zeros)
    // pixel ipix of the step (bits permuted as in fx_wgrad_kernel), channel group icg of the tile's eight, 16-B half ih of the group's 32-B row
    const int ih = t & 1, ipix = ((t >> 1) & 1) | (((t >> 3) & 3) << 1) | (((t >> 2) & 1) << 3), icg = t >> 5;
    const int KG = p.K >> 4, CG = p.C >> 4;
    const int a_cg = (m0 >> 4) + icg, b_cg = (n0 >> 4) + icg;
    // the thread's chunk inside an image (fx_applies(FX_WGRAD): tensors below 2^29 elements, so every byte offset stays below 2^30); a channel group beyond the tensor
    // carries the out-of-range bit here, and an offset added to it keeps the bit
    const int a_base = a_cg < KG ? a_cg * OHW * 32 + 16 * ih : FX_OOB, b_base = b_cg < CG ? b_cg * HWi * 32 + 16 * ih : FX_OOB;
    i32x4 rAi[3], rBi[3];
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) {
        rAi[pc] = fx_rsrc(p.DYimg + pc * p.dy_plane, (size_t)p.N * p.K * OHW * 2);
        rBi[pc] = fx_rsrc(p.Ximg + pc * p.x_plane, (size_t)p.N * p.C * HWi * 2);
    }
    const int a_nimg = KG * OHW, b_nimg = CG * HWi;                          // 32-B rows per image
    const int di = FX_BK / OHW, dr = (FX_BK - di * OHW) / p.OW, dc = FX_BK - di * OHW - dr * p.OW;
    // the thread's pixel as (image, output row, output column): a pixel at or beyond N OHW is one of image N or later, and a thread that starts there stays there
    int f_n, f_oh, f_ow;
    {
        const int q0 = s0 * FX_BK + ipix;
        f_n = q0 < NP ? q0 / OHW : p.N;
        const int rem = q0 < NP ? q0 - f_n * OHW : 0;
        f_oh = rem / p.OW; f_ow = rem - f_oh * p.OW;
    }
    i32x4 rai[3], rbi[3];
    auto fetch = [&]() {
        const int hi = f_oh * p.stride + dh, wi = f_ow * p.stride + dw;
        const bool ok = f_n < p.N && (unsigned)hi < (unsigned)p.Hi && (unsigned)wi < (unsigned)p.Wi;
        const int a_voff = ok ? (f_n * a_nimg + f_oh * p.OW + f_ow) * 32 + a_base : FX_OOB;
        const int b_voff = ok ? (f_n * b_nimg + hi * p.Wi + wi) * 32 + b_base : FX_OOB;
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) rai[pc] = fx_buffer_load_i32x4(rAi[pc], a_voff, 0, 0);
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) rbi[pc] = fx_buffer_load_i32x4(rBi[pc], b_voff, 0, 0);
        // the thread's pixel of the next K step
        f_ow += dc;
        if (f_ow >= p.OW) { f_ow -= p.OW; ++f_oh; }
        f_oh += dr;
        f_n += di;
        if (f_oh >= p.OH) { f_oh -= p.OH; ++f_n; }
    };
    const int st_img = fx_tr_off(ipix, 2 * icg + ih);
    auto stage = [&](int buf) {
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) *reinterpret_cast<i32x4*>(As + (buf * 3 + pc) * FX_PIECE + st_img) = rai[pc];
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) *reinterpret_cast<i32x4*>(Bs + (buf * 3 + pc) * FX_PIECE + st_img) = rbi[pc];
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    const int fr = lane & 31, fh = lane >> 5;
    int rd_a[2][2], rd_b[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        fx_tr_frag_off(lane, wm * 64 + a * 32, rd_a[a]);
        fx_tr_frag_off(lane, wn * 64 + a * 32, rd_b[a]);
    }
    const int live_a = fx_live_subtiles(m0 + wm * 64, p.K), live_b = fx_live_subtiles(n0 + wn * 64, p.C);
    if (nk > 0) { fetch(); stage(0); if (nk > 1) fetch(); }       // the software pipeline of fx_wgrad_kernel
    __syncthreads();
    auto kloop = [&](auto nat, auto nbt) {
        constexpr int NA = decltype(nat)::value, NB = decltype(nbt)::value;
        constexpr bool LIVE = NA > 0 && NB > 0;
        auto step = [&](int kt, auto st, auto fe) {
            const int buf = kt & 1;
            bf8 af[3][2], bf[3][2];
            auto read_a = [&](int pc) {
#pragma unroll
                for (int a = 0; a < 2; ++a)
                    if (a < NA) af[pc][a] = fx_tr_read(As + (buf * 3 + pc) * FX_PIECE, rd_a[a]);
            };
            auto read_b = [&](int pc) {
#pragma unroll
                for (int a = 0; a < 2; ++a)
                    if (a < NB) bf[pc][a] = fx_tr_read(Bs + (buf * 3 + pc) * FX_PIECE, rd_b[a]);
            };
            if constexpr (LIVE) {
                read_a(2); read_b(0); read_a(0); read_b(2);
                __builtin_amdgcn_sched_barrier(0);
                P3D_FX_PRODUCTS_RANGE(acc, af, bf, NA, NB, 0, 1)
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (decltype(st)::value) stage(buf ^ 1);
            if constexpr (decltype(fe)::value) fetch();
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (LIVE) {
                read_a(1); read_b(1);
                P3D_FX_PRODUCTS_RANGE(acc, af, bf, NA, NB, 1, 6)
            }
            __syncthreads();
        };
        int kt = 0;
        for (; kt + 2 < nk; ++kt) step(kt, std::true_type{}, std::true_type{});
        if (kt + 1 < nk) { step(kt, std::true_type{}, std::false_type{}); ++kt; }
        if (kt < nk) step(kt, std::false_type{}, std::false_type{});
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    if (live_a == 0 || live_b == 0) kloop(I0{}, I0{});
    else if (live_a == 2 && live_b == 2) kloop(I2{}, I2{});
    else if (live_a == 1 && live_b == 2) kloop(I1{}, I2{});
    else if (live_a == 2 && live_b == 1) kloop(I2{}, I1{});
    else kloop(I1{}, I1{});
    // C/D layout: col = lane & 31 (input channel c, contiguous in the slab), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (output channel k)
    float* out = p.slabs + (size_t)split * p.K * p.C * ntaps;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int c = n0 + wn * 64 + b * 32 + fr;
            if (c >= p.C) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = m0 + wm * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
                if (k < p.K) out[((size_t)k * ntaps + tap) * p.C + c] = acc[a][b][r];
            }
        }
}

// The prologue of fx_act_image_any_map_kernel<MODE 1 / 2>: the constants of the block's 16 channels (blockIdx.y) into cst -- the table's (fin.kind == 0) or those of the
// fused finalize step (FxFinalize, p3d_fx.h), which block x == 0 also writes out.  Ends with a barrier.  Statement for statement the prologue of fx_act_image_kernel
// below (same expressions, same summation order: the same constants from the same partials; tests/test_block_anysize_gpu.py compares the two passes byte for byte), which
// keeps its copy inline: calling this function there changes the code of its four instances with a prologue, which every aligned step runs (tools/isa_diff.py).
template <int MODE>
__device__ __forceinline__ void fx_image_constants(const FxFinalize& fin, const float* __restrict__ tab, int C, float (&cst)[16][FX_TAB], double (&fred)[2][16][16]) {
    const int cg = blockIdx.y, t = threadIdx.x;
    if (fin.kind == 0) {
        if (t < 16 * FX_TAB) cst[t >> 3][t & 7] = tab[(size_t)(cg * 16) * FX_TAB + t];
    } else {
        // fused finalize: thread (cl, rl) sums rows rl, rl + 16, ... of channel cl in fp64, lane 0 of each channel adds the 16 lanes in order
        const int cl = t & 15, rl = t >> 4, c = cg * 16 + cl;
        // (four rows per trip with independent loads: up to 32 dependent round trips otherwise, in the prologue of EVERY block of the pass)
        double s1 = 0.0, s2 = 0.0, u1 = 0.0, u2 = 0.0, v1 = 0.0, v2 = 0.0, w1 = 0.0, w2 = 0.0;
        int r = rl;
        if (fin.kind == 3) {
            const double* pd = (const double*)fin.partial + (size_t)c * fin.rows * 3;
            const int o = 1 + fin.which;
            for (; r + 48 < fin.rows; r += 64) {
                const double a0 = pd[r * 3], b0 = pd[r * 3 + o], a1 = pd[(r + 16) * 3], b1 = pd[(r + 16) * 3 + o];
                const double a2 = pd[(r + 32) * 3], b2 = pd[(r + 32) * 3 + o], a3 = pd[(r + 48) * 3], b3 = pd[(r + 48) * 3 + o];
                s1 += a0; s2 += b0; u1 += a1; u2 += b1; v1 += a2; v2 += b2; w1 += a3; w2 += b3;
            }
            for (; r < fin.rows; r += 16) { s1 += pd[r * 3]; s2 += pd[r * 3 + o]; }
        } else {
            const float* pf = (const float*)fin.partial + (size_t)c * 2;
            const size_t row = (size_t)C * 2;
            for (; r + 48 < fin.rows; r += 64) {
                const f32x2 a0 = *reinterpret_cast<const f32x2*>(pf + r * row), a1 = *reinterpret_cast<const f32x2*>(pf + (r + 16) * row);
                const f32x2 a2 = *reinterpret_cast<const f32x2*>(pf + (r + 32) * row), a3 = *reinterpret_cast<const f32x2*>(pf + (r + 48) * row);
                s1 += a0[0]; s2 += a0[1]; u1 += a1[0]; u2 += a1[1]; v1 += a2[0]; v2 += a2[1]; w1 += a3[0]; w2 += a3[1];
            }
            for (; r < fin.rows; r += 16) { const f32x2 v = *reinterpret_cast<const f32x2*>(pf + r * row); s1 += v[0]; s2 += v[1]; }
        }
        s1 = (s1 + u1) + (v1 + w1);
        s2 = (s2 + u2) + (v2 + w2);
        fred[0][rl][cl] = s1; fred[1][rl][cl] = s2;
        __syncthreads();
        if (rl == 0) {
            s1 = s2 = 0.0;
#pragma unroll
            for (int i = 0; i < 16; ++i) { s1 += fred[0][i][cl]; s2 += fred[1][i][cl]; }
            const bool owner = blockIdx.x == 0;
            if constexpr (MODE == 1) {          // as bn_finalize_fwd_kernel (p3d_block.hip)
                const double mean = s1 / fin.count;
                double var = s2 / fin.count - mean * mean;
                if (var < 0.0) var = 0.0;
                const float invstd = (float)(1.0 / sqrt(var + (double)fin.eps));
                const float fmean = (float)mean;
                const float sc = invstd * fin.gamma[c], sh = __fmaf_rn(-fmean, sc, fin.beta[c]);
                cst[cl][0] = sc; cst[cl][1] = sh;
                if (owner) {
                    float* tt = fin.table + (size_t)c * FX_TAB;
                    tt[0] = sc; tt[1] = sh; tt[2] = fmean; tt[3] = invstd;
                    if (fin.running_mean) {
                        const double unbiased = fin.count > 1.0 ? var * fin.count / (fin.count - 1.0) : var;
                        fin.running_mean[c] = (float)((1.0 - fin.momentum) * fin.running_mean[c] + fin.momentum * mean);
                        fin.running_var[c] = (float)((1.0 - fin.momentum) * fin.running_var[c] + fin.momentum * unbiased);
                    }
                }
            } else {                             // as bn_finalize_bwd_kernel
                const float* tt = fin.table + (size_t)c * FX_TAB;
                const float sc = tt[0], sh = tt[1], mean = tt[2], is = tt[3];
                const double dg = (double)is * s2;
                if (owner) {
                    fin.dbeta[c] = fin.accumulate ? fin.dbeta[c] + (float)s1 : (float)s1;
                    fin.dgamma[c] = fin.accumulate ? fin.dgamma[c] + (float)dg : (float)dg;
                }
                const float m1 = (float)(s1 / fin.count), m2 = (float)(dg / fin.count);
                const float A = fin.gamma[c] * is;
                cst[cl][0] = sc; cst[cl][1] = sh; cst[cl][4] = A; cst[cl][5] = -A * is * m2; cst[cl][6] = A * (mean * is * m2 - m1);
            }
        }
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------------------------------------------------
// Activation images: fp32 NCHW [N][C][HW] -> three bf16 planes [N][C/16][HW][16], optionally through the BatchNorm + ReLU of the forward pass (MODE 1) or
// the BatchNorm-backward map (MODE 2) of the layer the tensor belongs to (depthnet.py:98-116: out = relu(bn(conv(x))) and its autograd).
// A thread owns four consecutive pixels of eight channels (one 16-B chunk per pixel and plane): it reads eight 16-B groups (one per channel, pixels
// contiguous) and writes twelve 16-B chunks; the partner lane (ih) owns the other eight channels of the same pixels, so a lane pair writes 32-B rows.
// grid (ceil(N * HW / 4 * 2 / 256), C / 16)
// ------------------------------------------------------------------------------------------------------------------------------------------
// ROWS: the same values stored unsplit, as an fp32 row image [N][C/16][HW][16] -- a thread writes its eight channels of a pixel as two 16-B
// groups, a lane pair a whole 64-B row; the row-fed instances of the convolution kernels cut them into the three pieces themselves (fx_split_row8).
// (MODEX = MODE, or FX_IMG_ROWS + MODE for a row image: one int, so the plane instances keep the names fx_act_image_kernel<0 / 1 / 2> the profiles quote; the row
// instances are <4 / 5 / 6> and ignore plane_bytes)
constexpr int FX_IMG_ROWS = 4;
template <int MODEX>
__global__ __launch_bounds__(256) void fx_act_image_kernel(const float* __restrict__ X, const float* __restrict__ X2, const float* __restrict__ tab,
                                                           unsigned char* __restrict__ img, size_t plane_bytes, int N, int C, int HW, int masked, const FxFinalize fin,
                                                           const float* __restrict__ pixmul) {
    constexpr int MODE = MODEX % FX_IMG_ROWS;
    constexpr bool ROWS = MODEX >= FX_IMG_ROWS;
    static_assert(MODE <= 2 && MODEX < 2 * FX_IMG_ROWS, "modes 0, 1, 2 in either format");
    __shared__ float cst[16][FX_TAB];
    __shared__ double fred[2][16][16];
    const int cg = blockIdx.y, t = threadIdx.x;
    if constexpr (MODE != 0) {
        if (fin.kind == 0) {
            if (t < 16 * FX_TAB) cst[t >> 3][t & 7] = tab[(size_t)(cg * 16) * FX_TAB + t];
        } else {
            // fused finalize: thread (cl, rl) sums rows rl, rl + 16, ... of channel cl in fp64, lane 0 of each channel adds the 16 lanes in order
            const int cl = t & 15, rl = t >> 4, c = cg * 16 + cl;
            // (four rows per trip with independent loads: up to 32 dependent round trips otherwise, in the prologue of EVERY block of the pass)
            double s1 = 0.0, s2 = 0.0, u1 = 0.0, u2 = 0.0, v1 = 0.0, v2 = 0.0, w1 = 0.0, w2 = 0.0;
            int r = rl;
            if (fin.kind == 3) {
                const double* pd = (const double*)fin.partial + (size_t)c * fin.rows * 3;
                const int o = 1 + fin.which;
                for (; r + 48 < fin.rows; r += 64) {
                    const double a0 = pd[r * 3], b0 = pd[r * 3 + o], a1 = pd[(r + 16) * 3], b1 = pd[(r + 16) * 3 + o];
                    const double a2 = pd[(r + 32) * 3], b2 = pd[(r + 32) * 3 + o], a3 = pd[(r + 48) * 3], b3 = pd[(r + 48) * 3 + o];
                    s1 += a0; s2 += b0; u1 += a1; u2 += b1; v1 += a2; v2 += b2; w1 += a3; w2 += b3;
                }
                for (; r < fin.rows; r += 16) { s1 += pd[r * 3]; s2 += pd[r * 3 + o]; }
            } else {
                const float* pf = (const float*)fin.partial + (size_t)c * 2;
                const size_t row = (size_t)C * 2;
                for (; r + 48 < fin.rows; r += 64) {
                    const f32x2 a0 = *reinterpret_cast<const f32x2*>(pf + r * row), a1 = *reinterpret_cast<const f32x2*>(pf + (r + 16) * row);
                    const f32x2 a2 = *reinterpret_cast<const f32x2*>(pf + (r + 32) * row), a3 = *reinterpret_cast<const f32x2*>(pf + (r + 48) * row);
                    s1 += a0[0]; s2 += a0[1]; u1 += a1[0]; u2 += a1[1]; v1 += a2[0]; v2 += a2[1]; w1 += a3[0]; w2 += a3[1];
                }
                for (; r < fin.rows; r += 16) { const f32x2 v = *reinterpret_cast<const f32x2*>(pf + r * row); s1 += v[0]; s2 += v[1]; }
            }
            s1 = (s1 + u1) + (v1 + w1);
            s2 = (s2 + u2) + (v2 + w2);
            fred[0][rl][cl] = s1; fred[1][rl][cl] = s2;
            __syncthreads();
            if (rl == 0) {
                s1 = s2 = 0.0;
#pragma unroll
                for (int i = 0; i < 16; ++i) { s1 += fred[0][i][cl]; s2 += fred[1][i][cl]; }
                const bool owner = blockIdx.x == 0;
                if constexpr (MODE == 1) {          // as bn_finalize_fwd_kernel (p3d_block.hip)
                    const double mean = s1 / fin.count;
                    double var = s2 / fin.count - mean * mean;
                    if (var < 0.0) var = 0.0;
                    const float invstd = (float)(1.0 / sqrt(var + (double)fin.eps));
                    const float fmean = (float)mean;
                    const float sc = invstd * fin.gamma[c], sh = __fmaf_rn(-fmean, sc, fin.beta[c]);
                    cst[cl][0] = sc; cst[cl][1] = sh;
                    if (owner) {
                        float* tt = fin.table + (size_t)c * FX_TAB;
                        tt[0] = sc; tt[1] = sh; tt[2] = fmean; tt[3] = invstd;
                        if (fin.running_mean) {
                            const double unbiased = fin.count > 1.0 ? var * fin.count / (fin.count - 1.0) : var;
                            fin.running_mean[c] = (float)((1.0 - fin.momentum) * fin.running_mean[c] + fin.momentum * mean);
                            fin.running_var[c] = (float)((1.0 - fin.momentum) * fin.running_var[c] + fin.momentum * unbiased);
                        }
                    }
                } else {                             // as bn_finalize_bwd_kernel
                    const float* tt = fin.table + (size_t)c * FX_TAB;
                    const float sc = tt[0], sh = tt[1], mean = tt[2], is = tt[3];
                    const double dg = (double)is * s2;
                    if (owner) {
                        fin.dbeta[c] = fin.accumulate ? fin.dbeta[c] + (float)s1 : (float)s1;
                        fin.dgamma[c] = fin.accumulate ? fin.dgamma[c] + (float)dg : (float)dg;
                    }
                    const float m1 = (float)(s1 / fin.count), m2 = (float)(dg / fin.count);
                    const float A = fin.gamma[c] * is;
                    cst[cl][0] = sc; cst[cl][1] = sh; cst[cl][4] = A; cst[cl][5] = -A * is * m2; cst[cl][6] = A * (mean * is * m2 - m1);
                }
            }
        }
        __syncthreads();
    }
    const int ih = t & 1;
    const int q4 = HW >> 2;
    const long long quad = ((long long)blockIdx.x * 256 + t) >> 1;
    if (quad >= (long long)N * q4) return;
    const int n = (int)(quad / q4), pq = (int)(quad - (long long)n * q4);
    const size_t in0 = ((size_t)n * C + cg * 16 + 8 * ih) * HW + 4 * pq;
    f32x4 v[8], c2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        v[j] = *reinterpret_cast<const f32x4*>(X + in0 + (size_t)j * HW);
        if constexpr (MODE == 2) c2[j] = *reinterpret_cast<const f32x4*>(X2 + in0 + (size_t)j * HW);
    }
    if constexpr (MODE == 2) {
        if (fin.gmask) {                 // x = the gradient in front of the block's closing ReLU: apply that ReLU's mask bytes here
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned m = fin.gmask[(in0 + (size_t)j * HW) >> 2];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[j][e] = (m >> e) & 1u ? v[j][e] : 0.f;
            }
        }
    }
    if constexpr (MODE == 1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float sc = cst[8 * ih + j][0], sh = cst[8 * ih + j][1];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[j][e] = fmaxf(fmaf(v[j][e], sc, sh), 0.f);
        }
    }
    if constexpr (MODE == 2) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float sc = cst[8 * ih + j][0], sh = cst[8 * ih + j][1], A = cst[8 * ih + j][4], B = cst[8 * ih + j][5], K = cst[8 * ih + j][6];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float gg = (!masked || fmaf(c2[j][e], sc, sh) > 0.f) ? v[j][e] : 0.f;
                v[j][e] = fmaf(A, gg, fmaf(B, c2[j][e], K));
            }
        }
    }
    if (pixmul) {        // partial convolution: the operand the next kernel copies is this tensor times a per-pixel factor (mask_in of the conv that reads an
                         // activation image, mult of the conv whose gradient image this is); multiplied in here, the image-fed kernels stay factor-free
        const f32x4 f = *reinterpret_cast<const f32x4*>(pixmul + (size_t)n * HW + 4 * pq);
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) v[j][e] *= f[e];
    }
    if constexpr (ROWS) {
        unsigned char* dst = img + (((size_t)n * (C >> 4) + cg) * HW + 4 * pq) * 64 + 32 * ih;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            *reinterpret_cast<f32x4*>(dst + 64 * e) = f32x4{v[0][e], v[1][e], v[2][e], v[3][e]};
            *reinterpret_cast<f32x4*>(dst + 64 * e + 16) = f32x4{v[4][e], v[5][e], v[6][e], v[7][e]};
        }
    } else {
        unsigned char* dst = img + (((size_t)n * (C >> 4) + cg) * HW + 4 * pq) * 32 + 16 * ih;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            unsigned hp[4], mp[4], lp[4];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) fx_split2(v[2 * jj][e], v[2 * jj + 1][e], hp[jj], mp[jj], lp[jj]);
            *reinterpret_cast<i32x4*>(dst + 32 * e) = i32x4{(int)hp[0], (int)hp[1], (int)hp[2], (int)hp[3]};
            *reinterpret_cast<i32x4*>(dst + plane_bytes + 32 * e) = i32x4{(int)mp[0], (int)mp[1], (int)mp[2], (int)mp[3]};
            *reinterpret_cast<i32x4*>(dst + 2 * plane_bytes + 32 * e) = i32x4{(int)lp[0], (int)lp[1], (int)lp[2], (int)lp[3]};
        }
    }
}

// The two gradient images a block with a downsample branch opens its backward pass with -- d c_last and d c_ds, both = (BatchNorm-backward map)(g, c), g the block's
// upstream gradient -- in ONE pass: g (and the closing ReLU's mask bytes) are read once instead of twice.  MODE 2 with kind-3 finalize on both outputs (the fp64
// partials [C][rows][3] of block_open_bwd: sum g, sum g (c_last - mean), sum g (c_ds - mean_ds)); every value by the expressions, and the partial rows in the order, of
// fx_act_image_kernel<2>, so the images are bit-identical to two separate passes (p3d_fx_tune(3, 0) switches back: tests/test_block_gpu.py).
struct FxPairSide { const float* c; unsigned char* img; const float* gamma; float* dgamma; float* dbeta; const float* table; const float* pixmul; };
template <bool ROWS = false>          // ROWS: both images as fp32 row images (plane_bytes ignored)
__global__ __launch_bounds__(256) void fx_act_image_pair_kernel(const float* __restrict__ X, const unsigned char* __restrict__ gmask, const FxPairSide a, const FxPairSide b,
                                                                const double* __restrict__ partial, int rows, double count, int accumulate, size_t plane_bytes,
                                                                int N, int C, int HW) {
    __shared__ float cst[2][16][4];          // per side and channel: A, B, K
    __shared__ double fred[3][16][16];
    const int cg = blockIdx.y, t = threadIdx.x;
    {
        const int cl = t & 15, rl = t >> 4, c = cg * 16 + cl;
        const double* pd = partial + (size_t)c * rows * 3;
        double s[3] = {0.0, 0.0, 0.0}, u[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0};
        int r = rl;
        for (; r + 48 < rows; r += 64) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double a0 = pd[r * 3 + k], a1 = pd[(r + 16) * 3 + k], a2 = pd[(r + 32) * 3 + k], a3 = pd[(r + 48) * 3 + k];
                s[k] += a0; u[k] += a1; v[k] += a2; w[k] += a3;
            }
        }
        for (; r < rows; r += 16) {
#pragma unroll
            for (int k = 0; k < 3; ++k) s[k] += pd[r * 3 + k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) fred[k][rl][cl] = (s[k] + u[k]) + (v[k] + w[k]);
        __syncthreads();
        if (rl == 0) {
            double tot[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int i = 0; i < 16; ++i) { tot[0] += fred[0][i][cl]; tot[1] += fred[1][i][cl]; tot[2] += fred[2][i][cl]; }
            const bool owner = blockIdx.x == 0;
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                const FxPairSide& q = side == 0 ? a : b;
                const float* tt = q.table + (size_t)c * FX_TAB;
                const float mean = tt[2], is = tt[3];
                const double s1 = tot[0], dg = (double)is * tot[1 + side];
                if (owner) {
                    q.dbeta[c] = accumulate ? q.dbeta[c] + (float)s1 : (float)s1;
                    q.dgamma[c] = accumulate ? q.dgamma[c] + (float)dg : (float)dg;
                }
                const float m1 = (float)(s1 / count), m2 = (float)(dg / count);
                const float A = q.gamma[c] * is;
                cst[side][cl][0] = A; cst[side][cl][1] = -A * is * m2; cst[side][cl][2] = A * (mean * is * m2 - m1);
            }
        }
        __syncthreads();
    }
    const int ih = t & 1;
    const int q4 = HW >> 2;
    const long long quad = ((long long)blockIdx.x * 256 + t) >> 1;
    if (quad >= (long long)N * q4) return;
    const int n = (int)(quad / q4), pq = (int)(quad - (long long)n * q4);
    const size_t in0 = ((size_t)n * C + cg * 16 + 8 * ih) * HW + 4 * pq;
    f32x4 g[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] = *reinterpret_cast<const f32x4*>(X + in0 + (size_t)j * HW);
    if (gmask) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const unsigned m = gmask[(in0 + (size_t)j * HW) >> 2];
#pragma unroll
            for (int e = 0; e < 4; ++e) g[j][e] = (m >> e) & 1u ? g[j][e] : 0.f;
        }
    }
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const FxPairSide& q = side == 0 ? a : b;
        f32x4 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const f32x4 c2 = *reinterpret_cast<const f32x4*>(q.c + in0 + (size_t)j * HW);
            const float A = cst[side][8 * ih + j][0], B = cst[side][8 * ih + j][1], K = cst[side][8 * ih + j][2];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[j][e] = fmaf(A, g[j][e], fmaf(B, c2[e], K));
        }
        if (q.pixmul) {          // (a partial convolution's gradient image carries its renormalisation factor: fx_act_image_kernel)
            const f32x4 f = *reinterpret_cast<const f32x4*>(q.pixmul + (size_t)n * HW + 4 * pq);
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) v[j][e] *= f[e];
        }
        if constexpr (ROWS) {         // the fp32 row image (fx_act_image_kernel)
            unsigned char* dst = q.img + (((size_t)n * (C >> 4) + cg) * HW + 4 * pq) * 64 + 32 * ih;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                *reinterpret_cast<f32x4*>(dst + 64 * e) = f32x4{v[0][e], v[1][e], v[2][e], v[3][e]};
                *reinterpret_cast<f32x4*>(dst + 64 * e + 16) = f32x4{v[4][e], v[5][e], v[6][e], v[7][e]};
            }
        } else {
            unsigned char* dst = q.img + (((size_t)n * (C >> 4) + cg) * HW + 4 * pq) * 32 + 16 * ih;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                unsigned hp[4], mp[4], lp[4];
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) fx_split2(v[2 * jj][e], v[2 * jj + 1][e], hp[jj], mp[jj], lp[jj]);
                *reinterpret_cast<i32x4*>(dst + 32 * e) = i32x4{(int)hp[0], (int)hp[1], (int)hp[2], (int)hp[3]};
                *reinterpret_cast<i32x4*>(dst + plane_bytes + 32 * e) = i32x4{(int)mp[0], (int)mp[1], (int)mp[2], (int)mp[3]};
                *reinterpret_cast<i32x4*>(dst + 2 * plane_bytes + 32 * e) = i32x4{(int)lp[0], (int)lp[1], (int)lp[2], (int)lp[3]};
            }
        }
    }
}

static int g_pair_map = 1;
bool fx_pair_map_enabled() { return g_pair_map != 0; }
int32_t fx_act_image_pair(const float* x, const unsigned char* gmask, const float* c_a, const float* c_b, void* img_a, void* img_b, const FxFinalize* fa, const FxFinalize* fb,
                          int N, int C, int HW, hipStream_t st, const float* pixmul_a, bool rows) {
    if (!x || !c_a || !c_b || !img_a || !img_b || !fa || !fb || fa->kind != 3 || fb->kind != 3 || fa->partial != fb->partial || fa->rows != fb->rows || fa->which != 0 ||
        fb->which != 1 || N <= 0 || C <= 0 || (C & 15) || HW <= 0 || (HW & 3)) {
        set_error("fx_act_image_pair: bad argument"); return P3D_EINVAL;
    }
    const FxPairSide a{c_a, (unsigned char*)img_a, fa->gamma, fa->dgamma, fa->dbeta, fa->table, pixmul_a}, b{c_b, (unsigned char*)img_b, fb->gamma, fb->dgamma, fb->dbeta, fb->table, nullptr};
    const dim3 grid((unsigned)ceil_div((int64_t)N * (HW >> 2) * 2, 256), (unsigned)(C >> 4));
    auto* kernel = rows ? fx_act_image_pair_kernel<true> : fx_act_image_pair_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, x, gmask, a, b, (const double*)fa->partial, fa->rows, fa->count, fa->accumulate, (size_t)N * C * HW * 2, N, C, HW);
    return check_launch("fx_act_image_pair");
}

size_t fx_act_image_bytes(int64_t N, int64_t C, int64_t HW) { return (size_t)(3 * N * C * HW * 2); }
size_t fx_row_image_bytes(int64_t N, int64_t C, int64_t HW) { return (size_t)(N * C * HW * 4); }
// 1: the block executor keeps a_i and d c_i of dense blocks as three-plane images, as before the row images (p3d_fx_tune(6, 1): the A/B, tests/test_row_images_gpu.py)
static int g_plane_images = 0;
bool fx_block_row_images() { return g_plane_images == 0; }

int32_t fx_act_image(int mode, const float* x, const float* x2, const float* table, int masked, void* img, int N, int C, int HW, hipStream_t st,
                     const FxFinalize* fin, const float* pixmul, bool rows) {
    if (!x || !img || N <= 0 || C <= 0 || (C & 15) || HW <= 0 || (HW & 3) || (mode != 0 && !table && !fin) || (mode == 2 && !x2) || mode < 0 || mode > 2) {
        set_error("fx_act_image: bad argument (N=%d C=%d HW=%d mode=%d; C %% 16 == 0 and HW %% 4 == 0 are required)", N, C, HW, mode); return P3D_EINVAL;
    }
    FxFinalize f{};
    if (fin) {
        f = *fin;
        if (!((f.kind == 1 && mode == 1 && f.beta) || ((f.kind == 2 || f.kind == 3) && mode == 2 && f.dgamma && f.dbeta)) || !f.partial || f.rows <= 0 || !f.gamma || !f.table) {
            set_error("fx_act_image: inconsistent fused-finalize request (kind %d, mode %d)", f.kind, mode); return P3D_EINVAL;
        }
    }
    const size_t plane = (size_t)N * C * HW * 2;
    const dim3 grid((unsigned)ceil_div((int64_t)N * (HW >> 2) * 2, 256), (unsigned)(C >> 4));
    if (rows) {
        if (mode == 0) hipLaunchKernelGGL(fx_act_image_kernel<FX_IMG_ROWS + 0>, grid, dim3(256), 0, st, x, x2, table, (unsigned char*)img, plane, N, C, HW, masked, f, pixmul);
        else if (mode == 1) hipLaunchKernelGGL(fx_act_image_kernel<FX_IMG_ROWS + 1>, grid, dim3(256), 0, st, x, x2, table, (unsigned char*)img, plane, N, C, HW, masked, f, pixmul);
        else hipLaunchKernelGGL(fx_act_image_kernel<FX_IMG_ROWS + 2>, grid, dim3(256), 0, st, x, x2, table, (unsigned char*)img, plane, N, C, HW, masked, f, pixmul);
        return check_launch("fx_row_image");
    }
    if (mode == 0) hipLaunchKernelGGL(fx_act_image_kernel<0>, grid, dim3(256), 0, st, x, x2, table, (unsigned char*)img, plane, N, C, HW, masked, f, pixmul);
    else if (mode == 1) hipLaunchKernelGGL(fx_act_image_kernel<1>, grid, dim3(256), 0, st, x, x2, table, (unsigned char*)img, plane, N, C, HW, masked, f, pixmul);
    else hipLaunchKernelGGL(fx_act_image_kernel<2>, grid, dim3(256), 0, st, x, x2, table, (unsigned char*)img, plane, N, C, HW, masked, f, pixmul);
    return check_launch("fx_act_image");
}

// The mode-0 image at any HW (p3d_fx_act_image_any): the bytes and the layout of fx_act_image_kernel<0>, without HW % 4 == 0.  A thread owns the four-pixel group
// 4 g .. 4 g + 3 of ONE image (the last group of an image holds HW - 4 g < 4 pixels when HW is no multiple of 4) and eight channels.  With HW odd a channel row of x is
// only 4-B aligned: a row's group is one 16-B load where it is whole and its address allows, dword loads otherwise, none at or beyond the image's HW pixels -- so
// nothing is read beyond N C HW floats.  The 32-B pixel rows of the image are aligned whatever HW is: the stores keep their 16-B form, one row per pixel the group holds.
// grid (ceil(N * ceil(HW / 4) * 2 / 256), C / 16)
__global__ __launch_bounds__(256) void fx_act_image_any_kernel(const float* __restrict__ X, unsigned char* __restrict__ img, size_t plane_bytes, int N, int C, int HW) {
    const int cg = blockIdx.y, t = threadIdx.x, ih = t & 1;
    const int q4 = (HW + 3) >> 2;
    const long long quad = ((long long)blockIdx.x * 256 + t) >> 1;
    if (quad >= (long long)N * q4) return;
    const int n = (int)(quad / q4), pq = (int)(quad - (long long)n * q4);
    const int left = HW - 4 * pq;                  // pixels of this group: 4, or 1 .. 3 in the last group of an image
    const size_t in0 = ((size_t)n * C + cg * 16 + 8 * ih) * HW + 4 * pq;
    f32x4 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float* src = X + in0 + (size_t)j * HW;
        if (left >= 4 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) v[j] = *reinterpret_cast<const f32x4*>(src);
        else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[j][e] = e < left ? src[e] : 0.f;
        }
    }
    unsigned char* dst = img + (((size_t)n * (C >> 4) + cg) * HW + 4 * pq) * 32 + 16 * ih;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (e >= left) continue;
        unsigned hp[4], mp[4], lp[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) fx_split2(v[2 * jj][e], v[2 * jj + 1][e], hp[jj], mp[jj], lp[jj]);
        *reinterpret_cast<i32x4*>(dst + 32 * e) = i32x4{(int)hp[0], (int)hp[1], (int)hp[2], (int)hp[3]};
        *reinterpret_cast<i32x4*>(dst + plane_bytes + 32 * e) = i32x4{(int)mp[0], (int)mp[1], (int)mp[2], (int)mp[3]};
        *reinterpret_cast<i32x4*>(dst + 2 * plane_bytes + 32 * e) = i32x4{(int)lp[0], (int)lp[1], (int)lp[2], (int)lp[3]};
    }
}

int32_t fx_act_image_any(const float* x, void* img, int N, int C, int HW, hipStream_t st) {
    if (!x || !img || N <= 0 || C <= 0 || (C & 15) || HW <= 0 || (reinterpret_cast<uintptr_t>(img) & 15) || (reinterpret_cast<uintptr_t>(x) & 3) ||
        (int64_t)N * C * HW >= (1ll << 31)) {
        set_error("fx_act_image_any: bad argument (N=%d C=%d HW=%d; C %% 16 == 0 and a 16-B aligned image are required)", N, C, HW); return P3D_EINVAL;
    }
    const size_t plane = (size_t)N * C * HW * 2;
    const dim3 grid((unsigned)ceil_div((int64_t)N * ((HW + 3) >> 2) * 2, 256), (unsigned)(C >> 4));
    hipLaunchKernelGGL(fx_act_image_any_kernel, grid, dim3(256), 0, st, x, (unsigned char*)img, plane, N, C, HW);
    return check_launch("fx_act_image_any");
}

// Modes 1 and 2 at any HW (the residual blocks at any map width): the thread / group / row-access scheme of fx_act_image_any_kernel, the constants from
// fx_image_constants (table or fused finalize, the expressions and summation order of fx_act_image_kernel: the same constants from the same partials) and the maps of
// fx_act_image_kernel<1 / 2> element by element.  Plane images only; no mask bytes (a channel row of odd length shares its last mask byte with the next row's first) and no
// per-pixel factor.  A pixel beyond its image's HW is neither read nor written.
template <int MODE>
__global__ __launch_bounds__(256) void fx_act_image_any_map_kernel(const float* __restrict__ X, const float* __restrict__ X2, const float* __restrict__ tab,
                                                                   unsigned char* __restrict__ img, size_t plane_bytes, int N, int C, int HW, int masked, const FxFinalize fin) {
    static_assert(MODE == 1 || MODE == 2, "mode 0 is fx_act_image_any_kernel");
    __shared__ float cst[16][FX_TAB];
    __shared__ double fred[2][16][16];
    const int cg = blockIdx.y, t = threadIdx.x, ih = t & 1;
    fx_image_constants<MODE>(fin, tab, C, cst, fred);
    const int q4 = (HW + 3) >> 2;
    const long long quad = ((long long)blockIdx.x * 256 + t) >> 1;
    if (quad >= (long long)N * q4) return;
    const int n = (int)(quad / q4), pq = (int)(quad - (long long)n * q4);
    const int left = HW - 4 * pq;                  // pixels of this group: 4, or 1 .. 3 in the last group of an image
    const size_t in0 = ((size_t)n * C + cg * 16 + 8 * ih) * HW + 4 * pq;
    f32x4 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float* src = X + in0 + (size_t)j * HW;
        const float* src2 = MODE == 2 ? X2 + in0 + (size_t)j * HW : nullptr;
        f32x4 c2 = {0.f, 0.f, 0.f, 0.f};
        if (left >= 4 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(src2)) & 15) == 0) {
            v[j] = *reinterpret_cast<const f32x4*>(src);
            if constexpr (MODE == 2) c2 = *reinterpret_cast<const f32x4*>(src2);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[j][e] = e < left ? src[e] : 0.f;
                if constexpr (MODE == 2) c2[e] = e < left ? src2[e] : 0.f;
            }
        }
        const float sc = cst[8 * ih + j][0], sh = cst[8 * ih + j][1];
        if constexpr (MODE == 1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[j][e] = fmaxf(fmaf(v[j][e], sc, sh), 0.f);
        } else {
            const float A = cst[8 * ih + j][4], B = cst[8 * ih + j][5], K = cst[8 * ih + j][6];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float gg = (!masked || fmaf(c2[e], sc, sh) > 0.f) ? v[j][e] : 0.f;
                v[j][e] = fmaf(A, gg, fmaf(B, c2[e], K));
            }
        }
    }
    unsigned char* dst = img + (((size_t)n * (C >> 4) + cg) * HW + 4 * pq) * 32 + 16 * ih;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (e >= left) continue;
        unsigned hp[4], mp[4], lp[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) fx_split2(v[2 * jj][e], v[2 * jj + 1][e], hp[jj], mp[jj], lp[jj]);
        *reinterpret_cast<i32x4*>(dst + 32 * e) = i32x4{(int)hp[0], (int)hp[1], (int)hp[2], (int)hp[3]};
        *reinterpret_cast<i32x4*>(dst + plane_bytes + 32 * e) = i32x4{(int)mp[0], (int)mp[1], (int)mp[2], (int)mp[3]};
        *reinterpret_cast<i32x4*>(dst + 2 * plane_bytes + 32 * e) = i32x4{(int)lp[0], (int)lp[1], (int)lp[2], (int)lp[3]};
    }
}

int32_t fx_act_image_any_map(int mode, const float* x, const float* x2, const float* table, int masked, void* img, int N, int C, int HW, hipStream_t st, const FxFinalize* fin) {
    if (!x || !img || N <= 0 || C <= 0 || (C & 15) || HW <= 0 || (mode != 1 && mode != 2) || (!table && !fin) || (mode == 2 && !x2) ||
        (reinterpret_cast<uintptr_t>(img) & 15) || (reinterpret_cast<uintptr_t>(x) & 3) || (reinterpret_cast<uintptr_t>(x2) & 3) || (int64_t)N * C * HW >= (1ll << 31)) {
        set_error("fx_act_image_any_map: bad argument (N=%d C=%d HW=%d mode=%d; modes 1 and 2, C %% 16 == 0 and a 16-B aligned image are required)", N, C, HW, mode); return P3D_EINVAL;
    }
    FxFinalize f{};
    if (fin) {
        f = *fin;
        if (!((f.kind == 1 && mode == 1 && f.beta) || ((f.kind == 2 || f.kind == 3) && mode == 2 && f.dgamma && f.dbeta)) || !f.partial || f.rows <= 0 || !f.gamma || !f.table || f.gmask) {
            set_error("fx_act_image_any_map: inconsistent fused-finalize request (kind %d, mode %d; no mask bytes at any HW)", f.kind, mode); return P3D_EINVAL;
        }
    }
    const size_t plane = (size_t)N * C * HW * 2;
    const dim3 grid((unsigned)ceil_div((int64_t)N * ((HW + 3) >> 2) * 2, 256), (unsigned)(C >> 4));
    if (mode == 1) hipLaunchKernelGGL(fx_act_image_any_map_kernel<1>, grid, dim3(256), 0, st, x, x2, table, (unsigned char*)img, plane, N, C, HW, masked, f);
    else hipLaunchKernelGGL(fx_act_image_any_map_kernel<2>, grid, dim3(256), 0, st, x, x2, table, (unsigned char*)img, plane, N, C, HW, masked, f);
    return check_launch("fx_act_image_any_map");
}

// ------------------------------------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------------------------------------
static int g_fx = -1;       // -1: not decided yet (environment), 0 / 1: set
bool fx_enabled() {
    if (g_fx < 0) { const char* e = getenv("P3D_X3"); g_fx = (e && atoi(e) == 0) ? 0 : 1; }      // default ON; P3D_X3=0 keeps everything on the fp32-MFMA kernels
    return g_fx == 1;
}
int fx_set_enabled(int on) { const int before = fx_enabled() ? 1 : 0; g_fx = on ? 1 : 0; return before; }
// p3d_x3_any_enable: the per-layer training entries (p3d_conv2d_fwd / _dgrad / _wgrad) offer dense convolutions the aligned predicates refuse to the ragged instances
static int g_fx_any = -1;
bool fx_any_enabled() {
    if (g_fx_any < 0) { const char* e = getenv("P3D_X3_ANY"); g_fx_any = (e && atoi(e) == 1) ? 1 : 0; }      // default OFF
    return g_fx_any == 1;
}
int fx_set_any_enabled(int on) { const int before = fx_any_enabled() ? 1 : 0; g_fx_any = on ? 1 : 0; return before; }
// p3d_x3_any_partial_enable: the same offer for partial convolutions (both factors given) the aligned masked predicate refuses.  A switch of its own: neither looks at the other
static int g_fx_any_partial = -1;
bool fx_any_partial_enabled() {
    if (g_fx_any_partial < 0) { const char* e = getenv("P3D_X3_ANY_PARTIAL"); g_fx_any_partial = (e && atoi(e) == 1) ? 1 : 0; }      // default OFF
    return g_fx_any_partial == 1;
}
int fx_set_any_partial_enabled(int on) { const int before = fx_any_partial_enabled() ? 1 : 0; g_fx_any_partial = on ? 1 : 0; return before; }
// p3d_x3_any_images_enable: callers that feed convolutions pre-split images (ops_block.ConvImagesFn) offer the ones the aligned image-fed predicate refuses to the ragged
// image-fed instances (p3d_fx_conv_*_img_any).  The library only keeps the setting: no entry point looks at it, and neither of the other two switches does
static int g_fx_any_images = -1;
bool fx_any_images_enabled() {
    if (g_fx_any_images < 0) { const char* e = getenv("P3D_X3_ANY_IMAGES"); g_fx_any_images = (e && atoi(e) == 1) ? 1 : 0; }      // default OFF
    return g_fx_any_images == 1;
}
int fx_set_any_images_enabled(int on) { const int before = fx_any_images_enabled() ? 1 : 0; g_fx_any_images = on ? 1 : 0; return before; }
// p3d_x3_any_strided_enable: p3d_conv2d_dgrad offers dense stride-2 data gradients the aligned predicate refuses to the ragged instances, one launch per parity class
// into tight class planes (fx_conv_dgrad_strided_any).  A switch of its own: it looks at none of the other three and none of them at it
static int g_fx_any_strided = -1;
bool fx_any_strided_enabled() {
    if (g_fx_any_strided < 0) { const char* e = getenv("P3D_X3_ANY_STRIDED"); g_fx_any_strided = (e && atoi(e) == 1) ? 1 : 0; }      // default OFF
    return g_fx_any_strided == 1;
}
int fx_set_any_strided_enabled(int on) { const int before = fx_any_strided_enabled() ? 1 : 0; g_fx_any_strided = on ? 1 : 0; return before; }

// coverage counters (launches routed here vs to the fp32-MFMA kernel), read by bench.py so that no fallback goes uncounted
static std::mutex g_fx_count_mu;
static unsigned long long g_fx_count[6];      // fwd / dgrad / wgrad on this path, then fwd / dgrad / wgrad on the fp32-MFMA path
static double g_fx_flops[6];
void fx_count(int kind, const p3d_conv_desc* d) {
    std::lock_guard<std::mutex> lock(g_fx_count_mu);
    g_fx_count[kind] += 1;
    g_fx_flops[kind] += 2.0 * d->N * d->K * d->Ho * d->Wo * (double)d->C * d->R * d->S;
}
void fx_stats(unsigned long long* counts, double* flops, int reset) {
    std::lock_guard<std::mutex> lock(g_fx_count_mu);
    for (int i = 0; i < 6; ++i) { if (counts) counts[i] = g_fx_count[i]; if (flops) flops[i] = g_fx_flops[i]; }
    if (reset) for (int i = 0; i < 6; ++i) { g_fx_count[i] = 0; g_fx_flops[i] = 0.0; }
}

static bool fx_common(const p3d_conv_desc* d) {
    // (an input-channel window of a wider weight, c_offset / c_total: the per-call weight image is built from the window; callers with cached images pass whole weights)
    return fx_enabled() && d->c_offset >= 0 && d->c_offset + d->C <= d->c_total && d->R == d->S && (d->R & 1) && d->stride <= 2 &&
           (int64_t)d->N * d->C * d->H * d->W < (1ll << 31) && (int64_t)d->N * d->K * d->Ho * d->Wo < (1ll << 31) &&
           (int64_t)(d->K + 127) * (d->C + 127) * d->R * d->S * 6 < (1ll << 31);          // (32-bit byte offsets into the weight images)
}
// The shape rule of each pass, written once.  `ragged`: the instances that take any map width (fx_conv_kernel's RAG instances, fx_wgrad_any_kernel) -- the same rule
// with its width / alignment clauses switched off, and for the data gradient "stride 1 only" switched on (the parity classes of an odd map differ in size: the
// fp32-MFMA kernel keeps those).
// the data gradient's clauses that do not look at the map: reduction channels K in steps of 16, a reasonably filled channel tile; and, of a stride-2 one, that
// every parity class is a dense GEMM over an arithmetic progression of taps
static bool fx_dgrad_channels(const p3d_conv_desc* d, int min_m) { return d->K % FX_BK == 0 && d->K >= 32 && d->C % 4 == 0 && d->C >= min_m; }
static bool fx_dgrad_class_taps(const p3d_conv_desc* d) { return d->pad == d->dil * (d->R - 1) / 2 && (d->R == 1 || d->dil == 1); }
bool fx_applies(FxPass pass, const p3d_conv_desc* d, int min_m, bool ragged) {
    if (!fx_common(d)) return false;
    const bool widths = ragged || (d->W % 4 == 0 && d->Wo % 4 == 0);      // four consecutive pixels of one row per 16-B access
    switch (pass) {
        case FX_FWD:          // reduction channels C in steps of 16, a reasonably filled channel tile
            return widths && d->C % FX_BK == 0 && d->C >= 32 && d->K >= min_m;
        case FX_DGRAD:        // reduction channels K in steps of 16; the GEMM columns are the pixels of one stride^2 parity class of the input
            if (!(widths && fx_dgrad_channels(d, min_m))) return false;
            if (d->stride == 1) return true;
            return !ragged && d->H % 2 == 0 && d->W % 8 == 0 && fx_dgrad_class_taps(d);      // stride 2: classes of equal size
        case FX_WGRAD:        // the reduction runs over pixels in steps of 16; 32-bit byte offsets into whole tensors
            if ((int64_t)d->N * d->C * d->H * d->W >= (1ll << 29) || (int64_t)d->N * d->K * d->Ho * d->Wo >= (1ll << 29)) return false;
            return (ragged || (widths && (d->Ho * d->Wo) % FX_BK == 0)) && d->K >= min_m && d->C >= min_m && (d->R == 1 || d->C % 64 == 0);
    }
    return false;
}
// The stride-2 data gradient at ANY map side (p3d_x3_any_strided_enable): fx_applies(FX_DGRAD) for stride 2 without its H % 2, W % 8 and width clauses, whole weights
// only (the call builds its weight image; nothing that feeds a channel window lands here).  It admits aligned shapes too; those stay on the aligned instances.
bool fx_dgrad_strided_any_applies(const p3d_conv_desc* d, int min_m) {
    return fx_common(d) && d->c_offset == 0 && d->c_total == d->C && d->stride == 2 && fx_dgrad_channels(d, min_m) && fx_dgrad_class_taps(d);
}

// p3d_fx_tune(0 / 1 / 2, n): forced split counts (weight gradient, forward / data gradient) and a forced weight-gradient block target; 0 = the built-in plan
static int g_force_conv_splits = 0, g_force_wgrad_splits = 0, g_wgrad_target = 0;
// image-fed multi-tap launches with at least this many reduction channels walk the taps innermost.  Measured (profiles/r04_summary.md section 4): the
// regressor's forward (2048 channels x 9 taps) fetches 5.5x fewer bytes beyond L2 and runs 2 % faster; the 512-channel 3x3 layers fetch 3.1x fewer but run 2 % slower
// (a tap change per K step costs more than their re-reads out of the Infinity Cache): 1024 takes the first and leaves the second.  The data gradient uses the same
// threshold (its own at 512 / 256: 28.418 ms against 28.430, nothing; section 8b)
constexpr int FX_TAP_INNER_MIN = 1024;
// Block order of fx_conv_kernel / fx16_conv_kernel inside an XCD's run of logical ids: channel tile fastest, so that consecutive blocks share an activation tile and
// every pixel tile streams the whole weight image past the L2.  The other order (pixel tile fastest: the ~96 resident blocks stream one channel tile's weights
// together) was MEASURED (profiles/r04_summary.md section 4) 1 - 46 % SLOWER on every shape, layer4 and the regressor included (forward 0.896 vs 0.845 ms): the
// bytes FETCH_SIZE counts beyond L2 (3.7 - 28 x the algorithmic bytes there) come out of the 256 MB Infinity Cache at a rate these matrix-pipe-bound kernels do not
// feel, while losing the shared activation tile costs L2 hits they do.
// The weight gradient of a WIDE multi-tap layer (>= 512 input channels) takes the tap-fastest order: the nine tap blocks of one (x tile, dy tile) pair then run side by side on
// one XCD and the shifted views of the x tile are fetched once instead of once per tap -- FETCH_SIZE per launch 2.20 -> 0.80 GB for the 2048 -> 272 regressor, 254 -> 147 MB for
// the 512 -> 512 3x3, at unchanged time (0.980 / 0.978 ms, 0.398 / 0.396; profiles/r04_summary.md section 4).  Narrower layers keep order 0 (no traffic to win, +-2 % either way).
static int fx_wgrad_order(const p3d_conv_desc* d) { return (d->R * d->S > 1 && d->C >= 512) ? 1 : 0; }
static int g_class_launches = 0;      // 1: one launch per parity class of a strided data gradient (the round-3 form; p3d_fx_tune(5, 1), tests)
// channel tile of the fx16 kernel (v_mfma_f32_16x16x32_bf16) for a launch (0: the launch stays on fx_conv_kernel): 16 x 16 sub-tiles allow 96- and 64-row tiles where
// 128 rows would be mostly padding (the 272-channel regressor: 3 x 96 = 288 rows instead of 384; 64-channel layers: all four waves live).  At 128 rows the 16x16x32
// form is 1-3 % SLOWER on the large layers (20 fragment reads per step against 12, and the chip holds no higher clock on it in these kernels: profiles/r04_summary.md
// section 1), so those stay on the 32x32x16 kernel.
// The instance a code runs on there: the kernel applies p.emask at run time, so a factor code is the instance without the factor, with the pointer set; -1: none (the
// two fp32-fed partial-convolution codes).  Image-fed launches only.
constexpr int fx16_epi(int epi) {
    if (epi == FX_EPI_FACTOR || epi == FX_EPI_INFER_FACTOR) return -1;
    return fx_epi_infer(epi) ? FX_EPI_INFER : fx_epi_sums(epi) == 1 ? FX_EPI_STATS : fx_epi_sums(epi) == 2 ? FX_EPI_BWD_SUMS : FX_EPI_STORE;
}
static int fx16_bm(int M, bool img, int pro, int epi) {
    if (!img || pro != 0 || fx16_epi(epi) < 0) return 0;
    if (M <= 64) return 64;
    return ceil_div(M, 96) * 96 < ceil_div(M, 128) * 128 ? 96 : 0;
}

// What a call asks for -> the prologue and epilogue of its (unsplit) launch.  PRO 4: an fp32 operand of a partial convolution is multiplied by pmask in the kernel; an
// image carries its factor already.
struct FxSelect { int pro, epi; };
constexpr FxSelect fx_select(bool dgrad, bool img, bool masked, bool sums, bool infer) {
    const int pro = masked && !img ? 4 : 0;
    if (infer) return {pro, masked ? FX_EPI_INFER_FACTOR : FX_EPI_INFER};
    if (masked) return {pro, sums ? (dgrad ? FX_EPI_FACTOR_BWD_SUMS : FX_EPI_FACTOR_STATS) : (img ? FX_EPI_FACTOR_IMG : FX_EPI_FACTOR)};
    return {pro, sums ? (dgrad ? FX_EPI_BWD_SUMS : FX_EPI_STATS) : FX_EPI_STORE};
}

// Every compiled instance of the two convolution kernels, once: X(AMODE, PRO, EPIX, TAPI, RAG, ROWS) of fx_conv_kernel, X(BM, EPI, TAPI, ROWS) of fx16_conv_kernel.  The
// row-fed (ROWS) instances are those the dense block executor launches: the plain epilogue (its split-K slabs too) and the two BatchNorm ones, either K order, every tile.
// (A block's image-fed 3x3 is planes -> planes, so the tap-inner 96-row BatchNorm twins <96, STATS | BWD_SUMS, true, true> are reached by no block today: they are there so
// that a launch gets the same K order -- the same bits -- in both formats, like their plane-fed twins; tests/test_fx_instances_gpu.py runs them, and every other
// instance of the two lists, through p3d_fx_conv_fused against float64, and tests/test_fx_instances_host.py fails when a new entry here has no row.)  The tap-inner
// twins exist where the layers that want them land: 128-row tiles with the plain / BatchNorm epilogues, and the 96-row fx16 tile (the regressor).
#define P3D_FX_CONV_INSTANCES(X)                                                                                                                              \
    X(0, 0, FX_EPI_STORE, false, false, false) X(0, 0, FX_EPI_STATS, false, false, false) X(0, 0, FX_EPI_BWD_SUMS, false, false, false) X(0, 0, FX_EPI_INFER, false, false, false)        \
    X(0, 4, FX_EPI_STORE, false, false, false) X(0, 4, FX_EPI_FACTOR, false, false, false) X(0, 4, FX_EPI_FACTOR_STATS, false, false, false) X(0, 4, FX_EPI_INFER_FACTOR, false, false, false) \
    X(1, 0, FX_EPI_STORE, false, false, false) X(1, 0, FX_EPI_STATS, false, false, false) X(1, 0, FX_EPI_BWD_SUMS, false, false, false)                                           \
    X(1, 0, FX_EPI_FACTOR_STATS, false, false, false) X(1, 0, FX_EPI_FACTOR_BWD_SUMS, false, false, false) X(1, 0, FX_EPI_FACTOR_IMG, false, false, false) X(1, 0, FX_EPI_INFER, false, false, false) \
    X(1, 0, FX_EPI_STORE, true, false, false) X(1, 0, FX_EPI_STATS, true, false, false) X(1, 0, FX_EPI_BWD_SUMS, true, false, false) X(0, 0, FX_EPI_STORE, false, true, false) X(0, 0, FX_EPI_INFER, false, true, false) \
    X(0, 4, FX_EPI_INFER_FACTOR, false, true, false) X(0, 4, FX_EPI_STORE, false, true, false) X(0, 4, FX_EPI_FACTOR, false, true, false)                                             \
    X(1, 0, FX_EPI_STORE, false, true, false) X(1, 0, FX_EPI_STORE, true, true, false)                                                                      \
    X(1, 0, FX_EPI_STORE, false, false, true) X(1, 0, FX_EPI_STATS, false, false, true) X(1, 0, FX_EPI_BWD_SUMS, false, false, true)                        \
    X(1, 0, FX_EPI_STORE, true, false, true) X(1, 0, FX_EPI_STATS, true, false, true) X(1, 0, FX_EPI_BWD_SUMS, true, false, true)
// The ragged image-fed instances with the BatchNorm epilogues (the residual blocks at any map width, p3d_block_any_enable), X as above.  A list of their own: reported by
// p3d_fx_conv_any_sums_instances, NOT by p3d_fx_conv_instances, and each run alone by tests/test_block_anysize_gpu.py (tests/test_block_anysize_host.py fails
// when a new entry here has no case there).  Tap-outer only: no 3x3 inside a block of the reference's networks has 1024 channels.
#define P3D_FX_CONV_ANY_SUMS_INSTANCES(X) X(1, 0, FX_EPI_STATS, false, true, false) X(1, 0, FX_EPI_BWD_SUMS, false, true, false)
#define P3D_FX16_CONV_INSTANCES(X)                                                                                             \
    X(96, FX_EPI_STORE, false, false) X(96, FX_EPI_STATS, false, false) X(96, FX_EPI_BWD_SUMS, false, false) X(96, FX_EPI_INFER, false, false)             \
    X(64, FX_EPI_STORE, false, false) X(64, FX_EPI_STATS, false, false) X(64, FX_EPI_BWD_SUMS, false, false) X(64, FX_EPI_INFER, false, false)             \
    X(96, FX_EPI_STORE, true, false) X(96, FX_EPI_STATS, true, false) X(96, FX_EPI_BWD_SUMS, true, false)                       \
    X(96, FX_EPI_STORE, false, true) X(96, FX_EPI_STATS, false, true) X(96, FX_EPI_BWD_SUMS, false, true)                       \
    X(64, FX_EPI_STORE, false, true) X(64, FX_EPI_STATS, false, true) X(64, FX_EPI_BWD_SUMS, false, true)                       \
    X(96, FX_EPI_STORE, true, true) X(96, FX_EPI_STATS, true, true) X(96, FX_EPI_BWD_SUMS, true, true)
// The instance of a launch (bm 0: fx_conv_kernel; 96 / 64: fx16_conv_kernel), or null.  A tap-inner twin is looked up by the code itself: a launch with the per-pixel
// factor keeps the tap-outer order on either kernel.
using FxKernel = void (*)(const FxConvParams);
constexpr FxKernel fx_instance(int bm, bool img, int pro, int epi, bool tapi, bool rag, bool rows = false) {
    const int am = img ? 1 : 0, e = bm && !tapi ? fx16_epi(epi) : epi;
#define P3D_X(AM, PRO, EPI, TAPI, RAG, ROWS) if (bm == 0 && am == AM && pro == PRO && e == EPI && tapi == TAPI && rag == RAG && rows == ROWS) return fx_conv_kernel<AM, PRO, EPI, TAPI, RAG, ROWS>;
    P3D_FX_CONV_INSTANCES(P3D_X)
    P3D_FX_CONV_ANY_SUMS_INSTANCES(P3D_X)
#undef P3D_X
#define P3D_X(BM, EPI, TAPI, ROWS) if (bm == BM && am == 1 && pro == 0 && e == EPI && tapi == TAPI && !rag && rows == ROWS) return fx16_conv_kernel<BM, EPI, TAPI, ROWS>;
    P3D_FX16_CONV_INSTANCES(P3D_X)
#undef P3D_X
    return nullptr;
}
// everything fx_select can return for arguments that fx_conv_fwd / fx_conv_dgrad admit has its instances: on each tile the code can get, and for its split-K slabs
constexpr bool fx_select_covered() {
    for (int c = 0; c < 32; ++c) {
        const bool dgrad = c & 1, img = c & 2, masked = c & 4, sums = c & 8, infer = c & 16;
        if (dgrad ? (infer || (masked && !img && sums)) : (infer && (sums || (masked && img)))) continue;
        const FxSelect s = fx_select(dgrad, img, masked, sums, infer);
        if (!fx_instance(0, img, s.pro, s.epi, false, false) || !fx_instance(0, img, s.pro, FX_EPI_STORE, false, false)) return false;
        if (img && s.pro == 0 && fx16_epi(s.epi) >= 0 && !(fx_instance(96, img, 0, s.epi, false, false) && fx_instance(64, img, 0, s.epi, false, false))) return false;
    }
    // row images: the dense image-fed codes of training, on every tile and in either K order where the plane-fed code has a tap-inner twin
    for (int c = 0; c < 4; ++c) {
        const FxSelect s = fx_select(c & 1, true, false, c & 2, false);
        const int bms[3] = {0, 96, 64};
        for (int bm : bms)
            if (!fx_instance(bm, true, s.pro, s.epi, false, false, true) || (bm != 64 && !fx_instance(bm, true, s.pro, s.epi, true, false, true))) return false;
    }
    return fx_instance(0, false, 0, FX_EPI_INFER, false, true) && fx_instance(0, false, 0, FX_EPI_STORE, false, true) &&     // (the ragged forward: fp32-fed inference,
           fx_instance(0, false, 4, FX_EPI_INFER_FACTOR, false, true) && fx_instance(0, false, 4, FX_EPI_STORE, false, true) &&  //  dense and as a partial convolution;
           fx_instance(0, false, fx_select(false, false, true, false, false).pro, fx_select(false, false, true, false, false).epi, false, true) &&      //  training: the partial
           fx_instance(0, false, fx_select(true, false, true, false, false).pro, fx_select(true, false, true, false, false).epi, false, true) &&        //  convolution's two passes;
           fx_instance(0, true, fx_select(false, true, false, false, false).pro, fx_select(false, true, false, false, false).epi, false, true) &&       //  the image-fed dense one,
           fx_instance(0, true, fx_select(true, true, false, false, false).pro, fx_select(true, true, false, false, false).epi, true, true) &&          //  either K order;
           fx_instance(0, true, fx_select(false, true, false, true, false).pro, fx_select(false, true, false, true, false).epi, false, true) &&         //  and with the BatchNorm
           fx_instance(0, true, fx_select(true, true, false, true, false).pro, fx_select(true, true, false, true, false).epi, false, true);             //  epilogues, tap-outer)
}
static_assert(fx_select_covered(), "fx_select returns a code without a compiled instance");
void fx_tune(int what, int value) {
    switch (what) {
        case 0: g_force_wgrad_splits = value; break;
        case 1: g_force_conv_splits = value; break;
        case 2: g_wgrad_target = value; break;
        case 3: g_pair_map = value; break;                   // 0: the two opening image passes of a downsample block as two launches (tests)
        case 5: g_class_launches = value ? 1 : 0; break;
        case 6: g_plane_images = value ? 1 : 0; break;
        default: break;                                      // (unknown code: ignored)
    }
}

// How one forward / data-gradient call is launched: what the workspace and partial-row queries report and what the launchers use
struct FxPlan {
    int splits, kchunk;         // split-K: slabs, and K steps per slab (1, 0: one launch writes the result)
    int tiles_n;                // 128-pixel tiles of the GEMM's pixel grid (a strided data gradient: of one parity class)
    size_t slab_stride;         // elements between two slabs
    size_t slab_offset;         // bytes: the slabs lie behind the room for the weight image (built by the call unless the caller hands one in)
    size_t workspace;           // bytes in all
    int partial_rows;           // rows of the per-channel partial sums [rows][M][2]: pixel tiles, or under split-K the image groups of fx_reduce_kernel
};
size_t fx_weight_image_bytes(int K, int C, int RS, bool bwd) {
    const int rows = bwd ? C : K, red = bwd ? K : C;
    return (size_t)RS * ((rows + 127) / 128) * (red / FX_BK) * (3 * FX_PIECE);
}
static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// dgrad: rows = input channels, reduction = output channels, pixels = the input map; only stride 1 splits (a strided one writes its parity classes in place).
// ragged (the forward at any map width): each slab starts on a 16-B line.  ragged_sums: a ragged launch that takes BatchNorm sums is never split (the pass that sums
// ragged slabs takes none), so its partial rows are always the pixel tiles.
static FxPlan fx_plan(const p3d_conv_desc* d, bool dgrad, bool ragged = false, bool ragged_sums = false) {
    const int rows = dgrad ? d->C : d->K, red = dgrad ? d->K : d->C, RS = d->R * d->S, nk = RS * (red / FX_BK);
    const int64_t pixels = dgrad ? (int64_t)d->N * d->H * d->W : (int64_t)d->N * d->Ho * d->Wo;
    FxPlan s{1};
    s.tiles_n = (int)ceil_div(dgrad && d->stride > 1 ? (int64_t)d->N * (d->H / d->stride) * (d->W / d->stride) : pixels, FX_BN);
    const int64_t tiles = ceil_div(rows, FX_BM) * s.tiles_n;
    const bool may_split = (!dgrad || d->stride == 1) && !ragged_sums;
    int64_t want = 1;
    if (may_split && g_force_conv_splits > 0) want = g_force_conv_splits < nk ? g_force_conv_splits : nk;
    else if (may_split && tiles <= 400 && nk >= 64) {
        want = ceil_div(768, tiles);      // 768 blocks aimed at; 0 - 1024 swept in the step without a gain (profiles/r04_summary.md section 8b)
        if (want > nk / 32) want = nk / 32;
        if (want > 8) want = 8;
    }
    if (want >= 2) { s.kchunk = (int)ceil_div(nk, want); s.splits = (int)ceil_div(nk, s.kchunk); }
    if (s.splits < 2) { s.splits = 1; s.kchunk = 0; }
    s.slab_stride = ragged ? ((size_t)rows * pixels + 3) & ~(size_t)3 : (size_t)rows * pixels;
    s.slab_offset = align256(fx_weight_image_bytes(d->K, d->C, RS, dgrad));
    s.workspace = s.slab_offset + (s.splits > 1 ? (size_t)s.splits * s.slab_stride * sizeof(float) : 0);
    s.partial_rows = s.splits > 1 ? (d->N < 16 ? d->N : 16) : (int)ceil_div(pixels, FX_BN);
    return s;
}
// partial convolutions (PRO 4 / EPI 4 instances): 64-channel layers included (half-dead tiles).  P3D_FX_MASKED=0: A/B switch.  ragged: the pass's one rule at the same
// thresholds without its width clauses (the data gradient: stride 1 only) -- the masked ragged instances, fx_wgrad_any_masked_kernel
bool fx_masked_applies(FxPass pass, const p3d_conv_desc* d, bool ragged) {
    static const bool on = [] { const char* e = getenv("P3D_FX_MASKED"); return !(e && atoi(e) == 0); }();
    static const int min_m[3] = {64, 64, 96};          // FX_FWD, FX_DGRAD, FX_WGRAD
    return on && fx_applies(pass, d, min_m[pass], ragged);
}
// FX_WGRAD: the slabs of the larger of the two plans (fp32- or image-fed): what a caller reserves before it knows which
size_t fx_workspace(FxPass pass, const p3d_conv_desc* d, bool ragged) {
    if (pass != FX_WGRAD) return fx_plan(d, pass == FX_DGRAD, ragged).workspace;
    FxWgradOperands o{};
    o.ragged = ragged;
    const size_t a = fx_wgrad_plan(d, o).slab_bytes;
    o.aimg = o.bimg = true;
    const size_t b = fx_wgrad_plan(d, o).slab_bytes;
    return a > b ? a : b;
}
int fx_partial_rows(FxPass pass, const p3d_conv_desc* d, bool ragged) { return fx_plan(d, pass == FX_DGRAD, ragged, ragged).partial_rows; }

// Pre-split weight images of one conv weight w [K][C][R*S] (fp32): blockIdx.y = 0 the forward image (rows = output channels, reduction = input channels),
// 1 the data-gradient image (rows = input channels, reduction = output channels); a null image pointer skips that direction.  One thread per 16-B chunk
// position (tap, row tile, K step, row, half): eight fp32 weights -> three bf16 pieces (here the truncating split: piece = the top 16 bits of what is left;
// exact like the rounding one), written where fx_conv_kernel's linear 12 KB copy wants them.
// (ctot / coff: the image covers input channels coff .. coff + C of a weight with ctot of them -- the two halves of fusionnet's concat conv, fusionnet.py:138-139)
// (scale, fold_bn_images: the forward image of w[m][c][tap] * scale[m], one rounded product per weight)
__device__ __forceinline__ void fx_weight_image_chunks(const float* __restrict__ w, unsigned char* __restrict__ img, int K, int C, int RS, bool bwd, size_t first, size_t step,
                                                       int ctot, int coff, const float* __restrict__ scale = nullptr) {
    const int rows = bwd ? C : K, red = bwd ? K : C;
    const int tiles = (rows + 127) / 128, ksteps = red / FX_BK;
    const size_t total = (size_t)RS * tiles * ksteps * 256;
    for (size_t i = first; i < total; i += step) {
        const int half = (int)(i & 1), row = (int)((i >> 1) & 127);
        size_t j = i >> 8;
        const int ks = (int)(j % ksteps); j /= ksteps;
        const int tm = (int)(j % tiles);
        const int tap = (int)(j / tiles);
        const int m = tm * 128 + row, k0 = ks * FX_BK + half * 8;
        unsigned hi[8], mid[8], lo[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float x = 0.f;
            if (m < rows) x = bwd ? w[((size_t)(k0 + e) * ctot + coff + m) * RS + tap] : w[((size_t)m * ctot + coff + k0 + e) * RS + tap];
            if (scale && m < rows) x = x * scale[m];
            const unsigned hb = __builtin_bit_cast(unsigned, x) & 0xFFFF0000u;
            const float r1 = x - __builtin_bit_cast(float, hb);
            const unsigned mb = __builtin_bit_cast(unsigned, r1) & 0xFFFF0000u;
            const float r2 = r1 - __builtin_bit_cast(float, mb);
            hi[e] = hb; mid[e] = mb; lo[e] = __builtin_bit_cast(unsigned, r2) & 0xFFFF0000u;
        }
        unsigned char* dst = img + (((size_t)tap * tiles + tm) * ksteps + ks) * (3 * FX_PIECE) + fx_rc_off(row, half);
        *reinterpret_cast<i32x4*>(dst) = i32x4{(int)((hi[0] >> 16) | hi[1]), (int)((hi[2] >> 16) | hi[3]), (int)((hi[4] >> 16) | hi[5]), (int)((hi[6] >> 16) | hi[7])};
        *reinterpret_cast<i32x4*>(dst + FX_PIECE) = i32x4{(int)((mid[0] >> 16) | mid[1]), (int)((mid[2] >> 16) | mid[3]), (int)((mid[4] >> 16) | mid[5]), (int)((mid[6] >> 16) | mid[7])};
        *reinterpret_cast<i32x4*>(dst + 2 * FX_PIECE) = i32x4{(int)((lo[0] >> 16) | lo[1]), (int)((lo[2] >> 16) | lo[3]), (int)((lo[4] >> 16) | lo[5]), (int)((lo[6] >> 16) | lo[7])};
    }
}
__global__ __launch_bounds__(256) void fx_weight_images_kernel(const float* __restrict__ w, unsigned char* __restrict__ img_fwd, unsigned char* __restrict__ img_bwd, int K,
                                                               int C, int RS, int ctot, int coff) {
    const bool bwd = blockIdx.y == 1;
    unsigned char* img = bwd ? img_bwd : img_fwd;
    if (img) fx_weight_image_chunks(w, img, K, C, RS, bwd, (size_t)blockIdx.x * 256 + threadIdx.x, (size_t)gridDim.x * 256, ctot, coff);
}
// every convolution of a network in ONE launch (54 launches of a few microseconds each sat on the forward critical path of ResNet-50): grid (blocks, 2 * jobs)
struct FxImageJob { const float* w; unsigned char* fwd; unsigned char* bwd; int K, C, RS, pad; };
__global__ __launch_bounds__(256) void fx_weight_images_batched_kernel(const FxImageJob* __restrict__ jobs) {
    const FxImageJob j = jobs[blockIdx.y >> 1];
    const bool bwd = blockIdx.y & 1;
    unsigned char* img = bwd ? j.bwd : j.fwd;
    if (img) fx_weight_image_chunks(j.w, img, j.K, j.C, j.RS, bwd, (size_t)blockIdx.x * 256 + threadIdx.x, (size_t)gridDim.x * 256, j.C, 0);
}
int32_t fx_build_weight_images_batched(const void* jobs, int njobs, int blocks, hipStream_t st) {
    static_assert(sizeof(FxImageJob) == 40, "job table layout (ops_block.py builds it)");
    if (njobs <= 0) return P3D_OK;
    hipLaunchKernelGGL(fx_weight_images_batched_kernel, dim3((unsigned)(blocks < 1 ? 1 : blocks), (unsigned)(2 * njobs)), dim3(256), 0, st, (const FxImageJob*)jobs);
    return check_launch("fx_build_weight_images_batched");
}

// Eval-mode BatchNorm folded into the weights, for the whole network in ONE launch: grid (blocks, jobs).  Per job every block first computes the fold's
// per-channel scale s = gamma / sqrtf(var + eps) into LDS (no BatchNorm: s = 1), then strides over the job's output: kind 0 the forward weight image of
// w * s over input channels [c_offset, c_offset + C) (fx_weight_image_chunks, the layout p3d_fx_weight_images produces), kind 1 the folded fp32 weights
// [K][C][RS] (the stem, whose image p3d_stem_weight_image restates), kind 2 the fp16 forward image [K][RS][Cpad] of the fp16 path (the layout of
// p3d_weight_images_f16; Cpad in `reserved`, channels C .. Cpad - 1 written as 0), kind 3 the MXFP8 image of the fp8 path (elements [K][RS][Cpad], then the
// scale bytes [K][RS][Cpad / 32], by the MX rule of p3d_common.h from the same products as kind 2; Cpad in `reserved`, a multiple of 32), kind 4 kind 2's values as the fp16 data-gradient image [Cpad][RS][K] (the crsk layout of
// p3d_weight_images_f16: training through a frozen BatchNorm under -half_acc, ops_frozen.py).  Block 0 also writes
// b' = beta - mean * s (+ s * conv bias) when bias_out is given.
// The operation order is fixed (a division, a correctly rounded sqrtf, one product per weight), so the image equals the one built from the fold done in torch.
constexpr int FX_FOLD_MAX_K = 2048;
__global__ __launch_bounds__(256) void fx_fold_bn_kernel(const p3d_fold_job* __restrict__ jobs) {
    const p3d_fold_job j = jobs[blockIdx.y];
    __shared__ float sc[FX_FOLD_MAX_K];
    if (j.K <= 0 || j.K > FX_FOLD_MAX_K || j.C <= 0 || j.RS <= 0 || j.c_offset < 0 || j.c_offset + j.C > j.c_total || (j.kind == 0 && j.C % FX_BK != 0) ||
        ((j.kind == 2 || j.kind == 4) && (j.reserved < j.C || j.reserved % 8 != 0)) || (j.kind == 3 && (j.reserved < j.C || j.reserved % 32 != 0))) return;      // (checked by the caller)
    const bool bn = j.gamma != nullptr;
    for (int m = threadIdx.x; m < j.K; m += 256) {
        const float s = bn ? j.gamma[m] / sqrtf(j.var[m] + j.eps) : 1.f;
        sc[m] = s;
        if (blockIdx.x == 0 && j.bias_out) {
            float b = bn ? j.beta[m] - j.mean[m] * s : 0.f;
            if (j.conv_bias) b = bn ? b + s * j.conv_bias[m] : j.conv_bias[m];
            j.bias_out[m] = b;
        }
    }
    __syncthreads();
    const size_t first = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
    if (j.kind == 0) {
        fx_weight_image_chunks(j.w, (unsigned char*)j.out, j.K, j.C, j.RS, false, first, step, j.c_total, j.c_offset, bn ? sc : nullptr);
    } else if (j.kind == 2) {
        _Float16* out = (_Float16*)j.out;
        const int Cpad = j.reserved;
        const size_t total = (size_t)j.K * j.RS * Cpad;
        for (size_t i = first; i < total; i += step) {
            const int c = (int)(i % Cpad);
            const int tap = (int)((i / Cpad) % j.RS);
            const int m = (int)(i / ((size_t)Cpad * j.RS));
            float x = 0.f;
            if (c < j.C) {
                x = j.w[((size_t)m * j.c_total + j.c_offset + c) * j.RS + tap];
                if (bn) x = x * sc[m];
            }
            out[i] = (_Float16)x;
        }
    } else if (j.kind == 3) {
        // one thread per 32-channel block of one (row, tap): the same w * s as kind 2, then the MX rule (p3d_common.h); elements [K][RS][Cpad], scales [K][RS][Cpad / 32]
        unsigned char* out = (unsigned char*)j.out;
        const int Cpad = j.reserved, CB = Cpad >> 5;
        const size_t nblk = (size_t)j.K * j.RS * CB;
        unsigned char* scales = out + nblk * 32;
        for (size_t i = first; i < nblk; i += step) {
            const int cb = (int)(i % CB);
            const int tap = (int)((i / CB) % j.RS);
            const int m = (int)(i / ((size_t)CB * j.RS));
            float x[32];
            float amax = 0.f;
#pragma unroll
            for (int e = 0; e < 32; ++e) {
                const int c = cb * 32 + e;
                float v = 0.f;
                if (c < j.C) {
                    v = j.w[((size_t)m * j.c_total + j.c_offset + c) * j.RS + tap];
                    if (bn) v = v * sc[m];
                }
                x[e] = v;
                amax = fmaxf(amax, fabsf(v));
            }
            const int sb = mx_scale_byte_f32(amax);
            unsigned q[8];
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                q[d] = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) q[d] |= f32_to_e4m3(ldexpf(x[4 * d + e], 127 - sb)) << (8 * e);      // v / X, exact (X a power of two)
            }
            *reinterpret_cast<i32x4*>(out + i * 32) = i32x4{(int)q[0], (int)q[1], (int)q[2], (int)q[3]};
            *reinterpret_cast<i32x4*>(out + i * 32 + 16) = i32x4{(int)q[4], (int)q[5], (int)q[6], (int)q[7]};
            scales[i] = (unsigned char)sb;
        }
    } else if (j.kind == 4) {
        // the fp16 data-gradient image [Cpad][RS][K] of w * s: kind 2's values (one product, one rounding to half) in the crsk layout of p3d_weight_images_f16;
        // the output index runs fastest over K, so the stores are contiguous
        _Float16* out = (_Float16*)j.out;
        const size_t total = (size_t)j.reserved * j.RS * j.K;
        for (size_t i = first; i < total; i += step) {
            const int m = (int)(i % j.K);
            const int tap = (int)((i / j.K) % j.RS);
            const int c = (int)(i / ((size_t)j.K * j.RS));
            float x = 0.f;
            if (c < j.C) {
                x = j.w[((size_t)m * j.c_total + j.c_offset + c) * j.RS + tap];
                if (bn) x = x * sc[m];
            }
            out[i] = (_Float16)x;
        }
    } else {
        float* out = (float*)j.out;
        const size_t per = (size_t)j.C * j.RS, total = (size_t)j.K * per;
        for (size_t i = first; i < total; i += step) {
            const int m = (int)(i / per);
            const size_t rest = i - (size_t)m * per;
            const int c = (int)(rest / j.RS), tap = (int)(rest - (size_t)c * j.RS);
            const float x = j.w[((size_t)m * j.c_total + j.c_offset + c) * j.RS + tap];
            out[i] = bn ? x * sc[m] : x;
        }
    }
}
int32_t fx_fold_bn_images(const void* jobs, int njobs, int blocks, hipStream_t st) {
    static_assert(sizeof(p3d_fold_job) == 96, "job table layout (infer.py builds it)");
    if (njobs <= 0) return P3D_OK;
    hipLaunchKernelGGL(fx_fold_bn_kernel, dim3((unsigned)(blocks < 1 ? 1 : blocks), (unsigned)njobs), dim3(256), 0, st, (const p3d_fold_job*)jobs);
    return check_launch("fx_fold_bn_images");
}

int32_t fx_build_weight_images(const float* w, int K, int C, int RS, void* img_fwd, void* img_bwd, hipStream_t st, int ctot, int coff) {
    if (ctot <= 0) { ctot = C; coff = 0; }
    const size_t a = img_fwd ? fx_weight_image_bytes(K, C, RS, false) / 48 : 0, b = img_bwd ? fx_weight_image_bytes(K, C, RS, true) / 48 : 0;        // chunk positions (3 chunks each)
    const size_t total = a > b ? a : b;
    if (total == 0) return P3D_OK;
    const unsigned blocks = (unsigned)(ceil_div((int64_t)total, 256) < 4096 ? ceil_div((int64_t)total, 256) : 4096);
    hipLaunchKernelGGL(fx_weight_images_kernel, dim3(blocks, 2), dim3(256), 0, st, w, (unsigned char*)img_fwd, (unsigned char*)img_bwd, K, C, RS, ctot, coff);
    return check_launch("fx_build_weight_images");
}

// ---- what was launched (p3d_fx_launch_log): one record per conv-kernel launch, layout documented in include/p3d_hip.h -------------------------------
enum { FXL_KERNEL = 0, FXL_AMODE, FXL_PRO, FXL_EPI, FXL_TAPI, FXL_RAG, FXL_ROWS, FXL_GRID_X, FXL_GRID_Y, FXL_GRID_Z, FXL_KCHUNK, FXL_FINISH, FXL_FINISH_GROUPS,
       FXL_FIELDS = P3D_FX_LAUNCH_FIELDS };
static_assert(FXL_FINISH_GROUPS < FXL_FIELDS && FXL_ROWS + 1 == P3D_FX_INSTANCE_FIELDS, "the record of p3d_fx_launch_log outgrew its documented length");
enum { FX_FINISH_NONE = 0, FX_FINISH_REDUCE0, FX_FINISH_REDUCE1, FX_FINISH_REDUCE2, FX_FINISH_REDUCE_ANY, FX_FINISH_INTERLEAVE_ROWS, FX_FINISH_STRIDED_JOIN };       // FXL_FINISH
constexpr int FX_LOG_MAX = 256;
static std::mutex g_fx_log_mu;
static int32_t g_fx_log[FX_LOG_MAX][FXL_FIELDS];
static int64_t g_fx_log_n = 0;          // launches since the last reset (the first FX_LOG_MAX are kept)
int32_t fx_launch_log(int32_t* out, int32_t max_records, int32_t reset) {
    std::lock_guard<std::mutex> lock(g_fx_log_mu);
    const int64_t kept = g_fx_log_n < FX_LOG_MAX ? g_fx_log_n : FX_LOG_MAX;
    for (int64_t i = 0; out && i < kept && i < max_records; ++i)
        for (int f = 0; f < FXL_FIELDS; ++f) out[i * FXL_FIELDS + f] = g_fx_log[i][f];
    const int32_t n = (int32_t)(g_fx_log_n < INT32_MAX ? g_fx_log_n : INT32_MAX);
    if (reset) g_fx_log_n = 0;
    return n;
}
// (the ragged image-fed BatchNorm instances are not in this list: fx_conv_any_sums_instances)
static void fx_put_instance(int32_t* out, int32_t max_records, int32_t& n, int kernel, int am, int pro, int epi, bool tapi, bool rag, bool rows) {
    if (out && n < max_records) {
        const int32_t rec[P3D_FX_INSTANCE_FIELDS] = {kernel, am, pro, epi, tapi ? 1 : 0, rag ? 1 : 0, rows ? 1 : 0};
        for (int f = 0; f < P3D_FX_INSTANCE_FIELDS; ++f) out[n * P3D_FX_INSTANCE_FIELDS + f] = rec[f];
    }
    ++n;
}
int32_t fx_conv_any_sums_instances(int32_t* out, int32_t max_records) {
    int32_t n = 0;
#define P3D_X(AM, PRO, EPI, TAPI, RAG, ROWS) fx_put_instance(out, max_records, n, 0, AM, PRO, EPI, TAPI, RAG, ROWS);
    P3D_FX_CONV_ANY_SUMS_INSTANCES(P3D_X)
#undef P3D_X
    return n;
}
int32_t fx_conv_instances(int32_t* out, int32_t max_records) {
    int32_t n = 0;
    auto put = [&](int kernel, int am, int pro, int epi, bool tapi, bool rag, bool rows) { fx_put_instance(out, max_records, n, kernel, am, pro, epi, tapi, rag, rows); };
#define P3D_X(AM, PRO, EPI, TAPI, RAG, ROWS) put(0, AM, PRO, EPI, TAPI, RAG, ROWS);
    P3D_FX_CONV_INSTANCES(P3D_X)
#undef P3D_X
#define P3D_X(BM, EPI, TAPI, ROWS) put(BM, 1, 0, EPI, TAPI, false, ROWS);
    P3D_FX16_CONV_INSTANCES(P3D_X)
#undef P3D_X
    return n;
}

// the one place that launches a convolution kernel: the instance of (tile, operand, prologue, epilogue, K order, ragged), P3D_EINVAL if none was compiled.
// finish / finish_groups: the pass fx_launch_split queues behind the slabs, for the record only
static int32_t fx_launch_conv(const FxConvParams& p_in, bool img, int pro, int epi, int bm, dim3 grid, hipStream_t st, bool rag = false, bool rows = false,
                              int finish = FX_FINISH_NONE, int finish_groups = 0) {
    FxConvParams p = p_in;
    // only the STORE and backward instances of the aligned kernels hold the strided store: a parity class on any other would be written at dense addresses
    P3D_REQUIRE(!(rag || fx_epi_sums(epi) == 1 || fx_epi_infer(epi)) || (p.oxs == 1 && p.oys == 1 && p.oy0 == 0 && p.ox0 == 0 && p.YW == p.OW && p.YH == p.OH && p.ncls == 0),
                "fx_launch_conv: a strided result on a dense-only instance (rag=%d epi=%d)", rag ? 1 : 0, epi);
    if (p.tap_inner && !fx_instance(bm, img, pro, epi, true, rag, rows)) p.tap_inner = 0;
    const FxKernel kernel = fx_instance(bm, img, pro, epi, p.tap_inner != 0, rag, rows);
    if (!kernel) { set_error("fx_launch_conv: no kernel instance for img=%d pro=%d epi=%d bm=%d rows=%d", img ? 1 : 0, pro, epi, bm, rows ? 1 : 0); return P3D_EINVAL; }
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, p);
    {
        std::lock_guard<std::mutex> lock(g_fx_log_mu);
        if (g_fx_log_n < FX_LOG_MAX) {
            int32_t* r = g_fx_log[g_fx_log_n];
            for (int f = 0; f < FXL_FIELDS; ++f) r[f] = 0;
            r[FXL_KERNEL] = bm; r[FXL_AMODE] = img ? 1 : 0; r[FXL_PRO] = pro; r[FXL_EPI] = bm && !p.tap_inner ? fx16_epi(epi) : epi;       // (as fx_instance looked it up)
            r[FXL_TAPI] = p.tap_inner ? 1 : 0; r[FXL_RAG] = rag ? 1 : 0; r[FXL_ROWS] = rows ? 1 : 0;
            r[FXL_GRID_X] = (int32_t)grid.x; r[FXL_GRID_Y] = (int32_t)grid.y; r[FXL_GRID_Z] = (int32_t)grid.z; r[FXL_KCHUNK] = p.kchunk;
            r[FXL_FINISH] = finish; r[FXL_FINISH_GROUPS] = finish_groups;
        }
        ++g_fx_log_n;
    }
    return P3D_OK;
}

// A split-K call: the slabs (raw partial products, from the FX_EPI_STORE instance: bias, factor, sums and the inference tail belong to the pass that sums them), then
// that pass, which writes p.Y.  p: the parameters of the unsplit launch.
static int32_t fx_launch_split(FxConvParams p, const FxPlan& pl, bool img, int pro, int epi, int bm, float* slabs, hipStream_t st, bool rag = false, bool rows = false) {
    float* const y = p.Y;
    const float* const bias = p.bias, * const em = p.emask;
    const int OHW = p.OH * p.OW;
    p.kchunk = pl.kchunk; p.slab_stride = pl.slab_stride; p.Y = slabs; p.bias = nullptr; p.emask = nullptr;
    const int finish = rag ? FX_FINISH_REDUCE_ANY : FX_FINISH_REDUCE0 + fx_epi_sums(epi);
    if (int32_t e = fx_launch_conv(p, img, pro == 4 ? 4 : 0, FX_EPI_STORE, bm, dim3((unsigned)(p.tiles_m * pl.tiles_n), (unsigned)pl.splits), st, rag, rows, finish,
                                   rag ? 1 : pl.partial_rows)) return e;
    prof_kernel_done(st);
    if (rag) {
        const unsigned total = (unsigned)((size_t)p.N * p.M * OHW);          // (fx_common: below 2^31)
        hipLaunchKernelGGL(fx_reduce_any_kernel, dim3((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096), dim3(256), 0, st, (const float*)slabs, y, bias, pl.splits,
                           pl.slab_stride, total, p.M, OHW, p.accumulate, em, p.ep_res, p.ep_relu);
    } else {
        const int sums = fx_epi_sums(epi);       // (of the result times the factor, where there is one)
        auto* reduce = sums == 1 ? fx_reduce_kernel<1> : sums == 2 ? fx_reduce_kernel<2> : fx_reduce_kernel<0>;
        hipLaunchKernelGGL(reduce, dim3((unsigned)p.M, (unsigned)pl.partial_rows), dim3(256), 0, st, (const float*)slabs, y, bias, pl.splits, pl.slab_stride, p.N, p.M, OHW,
                           p.accumulate, p.ep_c, p.ep_tab, p.partial, em, p.ep_res, p.ep_relu);
    }
    return P3D_OK;
}

// y = conv(x, w) (+ bias); fuse may be null (plain convolution from fp32 x, the weight image built here)
int32_t fx_conv_fwd(const p3d_conv_desc* d, const float* x, const float* w, const float* bias, float* y, void* workspace, size_t workspace_bytes,
                    const FxFuse* fuse, hipStream_t st) {
    // partial convolution (partial_conv.py:45-53): y = conv(x * pmask) * emask.  An fp32 operand is multiplied by pmask before the in-kernel split (PRO 4); an image
    // operand carries its factor already (the pass that wrote it multiplied it in), so only emask is given.  With `partial` the BatchNorm statistics are taken of
    // the renormalised result (the residual-block executor: FX_EPI_FACTOR_STATS).
    const bool img = fuse && fuse->act_img;
    const bool masked = fuse && (fuse->pmask || fuse->emask);
    const bool infer = fuse && fuse->infer;
    const bool rag = fuse && fuse->ragged;          // the ragged instances (p3d_fx_conv_fwd_infer_any, p3d_fx_conv_fwd_infer_masked_any; training under p3d_x3_any_enable, partial
                                                    // convolutions under p3d_x3_any_partial_enable): any map width
    const void* wimg = fuse ? fuse->wimg : nullptr;
    const bool rows = fuse && fuse->rows;           // act_img is an fp32 row image (fx_row_image_bytes)
    P3D_REQUIRE(!rows || (img && !masked && !infer && !rag), "fx_conv_fwd: a row image feeds the dense aligned training launches only");
    if (masked && (!fuse->emask || (bias && !infer) || (img ? fuse->pmask != nullptr : fuse->pmask == nullptr))) {
        set_error("fx_conv_fwd: the partial-convolution instances take the output factor, the input factor exactly for an fp32 operand, and no bias"); return P3D_EINVAL;
    }
    // a cached weight image covers exactly the C input channels it was built for: never pair one with an input-channel window of a wider weight
    P3D_REQUIRE(!wimg || (d->c_offset == 0 && d->c_total == d->C), "fx_conv_fwd: a cached weight image with a channel window (c_offset %d, c_total %d, C %d)",
                d->c_offset, d->c_total, d->C);
    P3D_REQUIRE(!infer || (!fuse->partial && wimg && (!masked || (!img && !d->accumulate))),
                "fx_conv_fwd: the inference epilogue takes a cached folded weight image, no other fusion, and a partial convolution only from an fp32 operand");
    P3D_REQUIRE(!(fuse && (fuse->res || fuse->relu)) || infer, "fx_conv_fwd: a residual / ReLU needs the inference epilogue");
    P3D_REQUIRE(!(rag && img) || (!infer && !masked), "fx_conv_fwd: the ragged forward takes an image operand only as the dense training launch");
    const bool rag_sums = rag && fuse->partial;     // FX_EPI_STATS on the ragged image-fed instance (the residual blocks at any map width): one unsplit launch
    // (at either stride: the AMODE 1 fetch takes a pixel's position from the flat output column through hmul / wmul, the sums run over the result's flat pixels)
    P3D_REQUIRE(!rag_sums || (img && !infer && !masked),
                "fx_conv_fwd: the ragged training forward takes statistics only as the dense image-fed launch");
    const FxPlan pl = fx_plan(d, false, rag, rag_sums);
    if (pl.workspace && (!workspace || workspace_bytes < pl.workspace)) { set_error("fx_conv_fwd: workspace %zu B < required %zu B", workspace_bytes, pl.workspace); return P3D_EWORKSPACE; }
    FxConvParams p{};
    p.X = x; p.Y = y; p.bias = bias;
    if (img) { p.Ximg = (const unsigned char*)fuse->act_img; p.plane_bytes = (size_t)d->N * d->C * d->H * d->W * 2; }
    p.N = d->N; p.Cred = d->C; p.Hi = d->H; p.Wi = d->W; p.M = d->K; p.OH = d->Ho; p.OW = d->Wo; p.NP = d->N * d->Ho * d->Wo;
    p.YH = d->Ho; p.YW = d->Wo; p.oy0 = 0; p.ox0 = 0; p.oys = 1; p.oxs = 1;
    p.R = d->R; p.S = d->S; p.nR = d->R; p.nS = d->S; p.ntap = d->R * d->S; p.r0 = 0; p.rstep = 1; p.s0 = 0; p.sstep = 1;
    p.hmul = d->stride; p.hoff = -d->pad; p.hstep = d->dil; p.wmul = d->stride; p.woff = -d->pad; p.wstep = d->dil;
    p.accumulate = d->accumulate;
    const int RS = d->R * d->S;
    char* ws = (char*)workspace;
    if (!wimg) {
        if (int32_t e = fx_build_weight_images(w, d->K, d->C, RS, ws, nullptr, st, d->c_total, d->c_offset)) return e;
        wimg = ws;
    }
    p.Wimg = (const unsigned char*)wimg;
    const FxSelect sel = fx_select(false, img, masked, fuse && fuse->partial, infer);
    if (fuse) { p.partial = fuse->partial; p.pmask = fuse->pmask; p.emask = fuse->emask; p.ep_res = fuse->res; p.ep_relu = fuse->relu; }      // (res / relu: inference only, above)
    const bool split = pl.splits > 1;
    const int bm = rag ? 0 : fx16_bm(d->K, img, split ? 0 : sel.pro, split ? FX_EPI_STORE : sel.epi);
    p.tiles_m = (int)ceil_div(d->K, bm ? bm : FX_BM);
    p.tap_inner = img && RS > 1 && d->C >= FX_TAP_INNER_MIN;
    if (int32_t e = split ? fx_launch_split(p, pl, img, sel.pro, sel.epi, bm, (float*)(ws + pl.slab_offset), st, rag, rows)
                          : fx_launch_conv(p, img, sel.pro, sel.epi, bm, dim3((unsigned)(p.tiles_m * pl.tiles_n), 1), st, rag, rows)) return e;
    return check_launch("fx_conv_fwd");
}

// dx (=|+=) dgrad(dy, w); strided: one launch per parity class of the input, written straight into dx
int32_t fx_conv_dgrad(const p3d_conv_desc* d, const float* dy, const float* w, float* dx, void* workspace, size_t workspace_bytes, const FxFuse* fuse,
                      hipStream_t st) {
    // partial convolution: dx = dgrad(dy * pmask) * emask (pmask = mult of the output pixel, emask = mask_in of the input pixel).  As in fx_conv_fwd an image operand
    // carries its factor; with `partial` the BatchNorm-backward sums are taken of the masked result (FX_EPI_FACTOR_BWD_SUMS).
    const bool img = fuse && fuse->act_img;
    const bool masked = fuse && (fuse->pmask || fuse->emask);
    const void* wimg = fuse ? fuse->wimg : nullptr;
    P3D_REQUIRE(!wimg || (d->c_offset == 0 && d->c_total == d->C), "fx_conv_dgrad: a cached weight image with a channel window (c_offset %d, c_total %d, C %d)",
                d->c_offset, d->c_total, d->C);
    if (masked && (!fuse->emask || (img ? fuse->pmask != nullptr : fuse->pmask == nullptr) || (!img && fuse->partial))) {
        set_error("fx_conv_dgrad: the partial-convolution instances take the result factor and the operand factor exactly for an fp32 operand"); return P3D_EINVAL;
    }
    const bool rows = fuse && fuse->rows;           // act_img is an fp32 row image
    P3D_REQUIRE(!rows || (img && !masked && !(fuse && fuse->ragged)), "fx_conv_dgrad: a row image feeds the dense aligned launches only");
    const bool rag = fuse && fuse->ragged;          // the ragged forward instances over dy (p3d_x3_any_enable; masked: p3d_x3_any_partial_enable): any map width, stride 1, fp32-fed
    const bool rag_sums = rag && fuse->partial;     // FX_EPI_BWD_SUMS on the ragged image-fed instance (the residual blocks at any map width): one unsplit launch
    P3D_REQUIRE(!rag || (d->stride == 1 && !(img && masked) && (!rag_sums || (img && !masked)) && !fuse->acc_src),
                "fx_conv_dgrad: the ragged data gradient is the stride-1 one, dense (fp32- or image-fed) or masked (fp32-fed), with sums only as the dense image-fed launch");
    const FxPlan pl = fx_plan(d, true, rag, rag_sums);
    if (pl.workspace && (!workspace || workspace_bytes < pl.workspace)) { set_error("fx_conv_dgrad: workspace %zu B < required %zu B", workspace_bytes, pl.workspace); return P3D_EWORKSPACE; }
    if (fuse && fuse->acc_src && !(d->accumulate && fx_dgrad_accumulates_from_source(d))) {
        set_error("fx_conv_dgrad: an accumulation source needs accumulate = 1, stride 1 and an unsplit launch"); return P3D_EINVAL;
    }
    FxConvParams p{};
    p.X = dy; p.Y = dx;
    if (img) { p.Ximg = (const unsigned char*)fuse->act_img; p.plane_bytes = (size_t)d->N * d->K * d->Ho * d->Wo * 2; }
    p.N = d->N; p.Cred = d->K; p.Hi = d->Ho; p.Wi = d->Wo; p.M = d->C;
    p.YH = d->H; p.YW = d->W;
    p.R = d->R; p.S = d->S;
    p.accumulate = d->accumulate;
    const int RS = d->R * d->S;
    char* ws = (char*)workspace;
    if (!wimg) {
        if (int32_t e = fx_build_weight_images(w, d->K, d->C, RS, nullptr, ws, st, d->c_total, d->c_offset)) return e;
        wimg = ws;
    }
    p.Wimg = (const unsigned char*)wimg;
    const bool sums = fuse && fuse->partial;
    if (sums) { p.partial = fuse->partial; p.ep_c = fuse->ep_c; p.ep_tab = fuse->ep_tab; }
    if (masked) { p.pmask = fuse->pmask; p.emask = fuse->emask; }
    const bool split = pl.splits > 1;
    p.tap_inner = img && RS > 1 && d->K >= FX_TAP_INNER_MIN;
    const auto [pro, epi] = fx_select(true, img, masked, sums, false);
    const int bm = rag ? 0 : fx16_bm(d->C, img, split ? 0 : pro, split ? FX_EPI_STORE : epi);
    p.tiles_m = (int)ceil_div(d->C, bm ? bm : FX_BM);
    if (d->stride == 1) {
        p.OH = d->H; p.OW = d->W; p.NP = d->N * d->H * d->W; p.oy0 = 0; p.ox0 = 0; p.oys = 1; p.oxs = 1;
        p.nR = d->R; p.nS = d->S; p.ntap = RS; p.r0 = 0; p.rstep = 1; p.s0 = 0; p.sstep = 1;
        p.hmul = 1; p.hoff = d->pad; p.hstep = -d->dil; p.wmul = 1; p.woff = d->pad; p.wstep = -d->dil;
        if (!split && fuse && fuse->acc_src && d->accumulate) { p.acc_src = fuse->acc_src; p.acc_mask = fuse->acc_mask; }
        if (int32_t e = split ? fx_launch_split(p, pl, img, pro, epi, bm, (float*)(ws + pl.slab_offset), st, rag, rows)
                              : fx_launch_conv(p, img, pro, epi, bm, dim3((unsigned)(p.tiles_m * pl.tiles_n), 1), st, rag, rows)) return e;
        return check_launch("fx_conv_dgrad");
    }
    // stride 2: input pixel (ph + 2 i, pw + 2 j) of class (ph, pw) gathers dy at (i + off0 - ir * offstep, ...) over the taps r = r0 + rstep * ir that reach it
    if (fx_epi_sums(epi) != 0) { set_error("fx_conv_dgrad: the BatchNorm-backward epilogue is not available for strided data gradients"); return P3D_EINVAL; }
    const int st2 = d->stride;
    p.OH = d->H / st2; p.OW = d->W / st2; p.NP = d->N * p.OH * p.OW; p.oys = st2; p.oxs = st2;
    p.hmul = 1; p.wmul = 1;
    const int tiles_n = pl.tiles_n;
    FxConvClass cls[4];
    int ncls = 0;
    struct { int r0, step, n, off0, offstep; } ax[2][2];      // fill_class per axis (rows, columns) and parity: the taps r0 + step * i, i < n
    for (int par = 0; par < st2; ++par) {
        fill_class(par, d->R, st2, d->pad, d->dil, &ax[0][par].r0, &ax[0][par].step, &ax[0][par].n, &ax[0][par].off0, &ax[0][par].offstep);
        fill_class(par, d->S, st2, d->pad, d->dil, &ax[1][par].r0, &ax[1][par].step, &ax[1][par].n, &ax[1][par].off0, &ax[1][par].offstep);
    }
    for (int ph = 0; ph < st2; ++ph)
        for (int pw = 0; pw < st2; ++pw) {
            const auto &ty = ax[0][ph], &tx = ax[1][pw];
            if (ty.n == 0 || tx.n == 0) continue;      // a class no tap reaches keeps what dx held: see fx_dgrad_has_dead_classes
            FxConvParams c = p;
            c.nR = ty.n; c.nS = tx.n; c.ntap = ty.n * tx.n; c.r0 = ty.r0; c.rstep = ty.step; c.s0 = tx.r0; c.sstep = tx.step;
            c.hoff = ty.off0; c.hstep = -ty.offstep;
            c.woff = tx.off0; c.wstep = -tx.offstep;
            c.oy0 = ph; c.ox0 = pw;
            if (g_class_launches) { if (int32_t e = fx_launch_conv(c, img, pro, epi, bm, dim3((unsigned)(c.tiles_m * tiles_n), 1), st, false, rows)) return e; continue; }
            cls[ncls++] = FxConvClass{c.nR, c.nS, c.ntap, c.r0, c.rstep, c.s0, c.sstep, c.hoff, c.hstep, c.woff, c.wstep, c.oy0, c.ox0};
        }
    if (ncls > 0) {
        // one launch, the classes with the most taps in the lowest z (dispatched first: the short ones fill the tail)
        for (int i = 1; i < ncls; ++i)
            for (int j = i; j > 0 && cls[j].ntap > cls[j - 1].ntap; --j) { const FxConvClass t = cls[j]; cls[j] = cls[j - 1]; cls[j - 1] = t; }
        p.ncls = ncls;
        for (int i = 0; i < ncls; ++i) p.cls[i] = cls[i];
        if (int32_t e = fx_launch_conv(p, img, pro, epi, bm, dim3((unsigned)(p.tiles_m * tiles_n), 1, (unsigned)ncls), st, false, rows)) return e;
    }
    return check_launch("fx_conv_dgrad");
}

// The stride-2 data gradient at any map side (fx_dgrad_strided_any_applies): parity class (ph, pw) of the input is a dense [N][C][OHc][OWc] result of its own,
// OHc = (H - ph + 1) / 2 rows of OWc = (W - pw + 1) / 2 pixels, so each live, non-empty class is ONE launch of the ragged fp32-fed instance over dy -- the taps that reach
// the class from fill_class, as in fx_conv_dgrad -- into its tight plane stage + cls * cls_stride (cls = ph * 2 + pw), the layout the fp32-MFMA path stages its classes
// in.  The caller interleaves the planes into dx (p3d_conv.hip: dgrad_interleave_rows_kernel, which also writes the zeros of the classes no tap reaches and adds under
// `accumulate`).  The workspace: the data-gradient weight image, built here, then the four planes, each part on a 256-B line; cls_stride is rounded up to four floats,
// so every plane starts on a 16-B line.  No class launch is split along K.
// Image-fed (dy_img, the block executor and p3d_fx_conv_dgrad_strided_img_any): the operand is the plane image of dy (fx_act_image_any) and the class launches go to the
// image-fed ragged FX_EPI_STORE instance, tap-outer, with the same class geometry and the same planes; wimgT, when given, is the cached data-gradient weight image and
// nothing is built (the room for it in front of the planes stays unused).  join: the finishing pass the caller queues behind the planes is block_strided_join_any_kernel
// (p3d_block.hip) instead of the interleave -- for the record of the last class launch only.
FxStridedPlan fx_dgrad_strided_any_plan(const p3d_conv_desc* d) {
    FxStridedPlan s{};
    s.cls_stride = ((size_t)d->N * d->C * ((d->H + 1) / 2) * ((d->W + 1) / 2) + 3) & ~(size_t)3;
    s.stage_offset = align256(fx_weight_image_bytes(d->K, d->C, d->R * d->S, true));
    s.workspace = s.stage_offset + align256(4 * s.cls_stride * sizeof(float));
    return s;
}
int32_t fx_conv_dgrad_strided_any(const p3d_conv_desc* d, const float* dy, const float* w, void* workspace, size_t workspace_bytes, int* live_mask, hipStream_t st,
                                  const void* dy_img, const void* wimgT, bool join) {
    P3D_REQUIRE(fx_dgrad_strided_any_applies(d, 32), "fx_conv_dgrad_strided_any: shape outside the stride-2 rule of the x3 kernels");
    const bool img = dy_img != nullptr;
    P3D_REQUIRE(img || (!wimgT && !join), "fx_conv_dgrad_strided_any: a cached weight image and the joining pass belong to the image-fed form");
    const FxStridedPlan pl = fx_dgrad_strided_any_plan(d);
    if (!workspace || workspace_bytes < pl.workspace) { set_error("fx_conv_dgrad_strided_any: workspace %zu B < required %zu B", workspace_bytes, pl.workspace); return P3D_EWORKSPACE; }
    char* ws = (char*)workspace;
    const int RS = d->R * d->S;
    if (!wimgT) {
        if (int32_t e = fx_build_weight_images(w, d->K, d->C, RS, nullptr, ws, st, d->c_total, d->c_offset)) return e;
        wimgT = ws;
    }
    float* stage = (float*)(ws + pl.stage_offset);
    FxConvParams p{};
    p.X = dy; p.Wimg = (const unsigned char*)wimgT;
    if (img) { p.Ximg = (const unsigned char*)dy_img; p.plane_bytes = (size_t)d->N * d->K * d->Ho * d->Wo * 2; }
    p.N = d->N; p.Cred = d->K; p.Hi = d->Ho; p.Wi = d->Wo; p.M = d->C;
    p.R = d->R; p.S = d->S;
    p.oy0 = 0; p.ox0 = 0; p.oys = 1; p.oxs = 1; p.hmul = 1; p.wmul = 1;
    p.tiles_m = (int)ceil_div(d->C, FX_BM);
    struct { int r0, step, n, off0, offstep; } ax[2][2];      // fill_class per axis (rows, columns) and parity
    for (int par = 0; par < 2; ++par) {
        fill_class(par, d->R, 2, d->pad, d->dil, &ax[0][par].r0, &ax[0][par].step, &ax[0][par].n, &ax[0][par].off0, &ax[0][par].offstep);
        fill_class(par, d->S, 2, d->pad, d->dil, &ax[1][par].r0, &ax[1][par].step, &ax[1][par].n, &ax[1][par].off0, &ax[1][par].offstep);
    }
    FxConvParams cls[4];
    int ncls = 0, live = 0;
    for (int ph = 0; ph < 2; ++ph)
        for (int pw = 0; pw < 2; ++pw) {
            const auto &ty = ax[0][ph], &tx = ax[1][pw];
            if (ty.n == 0 || tx.n == 0) continue;      // no tap reaches the class: the interleave writes its zeros, the plane is never read
            live |= 1 << (ph * 2 + pw);
            FxConvParams c = p;
            c.OH = c.YH = (d->H - ph + 1) / 2; c.OW = c.YW = (d->W - pw + 1) / 2; c.NP = d->N * c.OH * c.OW;
            if (c.NP == 0) continue;                   // (a map one pixel high or wide has no odd row or column)
            c.nR = ty.n; c.nS = tx.n; c.ntap = ty.n * tx.n; c.r0 = ty.r0; c.rstep = ty.step; c.s0 = tx.r0; c.sstep = tx.step;
            c.hoff = ty.off0; c.hstep = -ty.offstep;
            c.woff = tx.off0; c.wstep = -tx.offstep;
            c.Y = stage + (size_t)(ph * 2 + pw) * pl.cls_stride;
            cls[ncls++] = c;
        }
    // the classes with the most taps first: the short ones fill the tail
    for (int i = 1; i < ncls; ++i)
        for (int j = i; j > 0 && cls[j].ntap > cls[j - 1].ntap; --j) { const FxConvParams t = cls[j]; cls[j] = cls[j - 1]; cls[j - 1] = t; }
    for (int i = 0; i < ncls; ++i) {
        const dim3 grid((unsigned)(cls[i].tiles_m * ceil_div(cls[i].NP, FX_BN)), 1);
        if (int32_t e = fx_launch_conv(cls[i], img, 0, FX_EPI_STORE, 0, grid, st, true, false,
                                       i == ncls - 1 ? (join ? FX_FINISH_STRIDED_JOIN : FX_FINISH_INTERLEAVE_ROWS) : FX_FINISH_NONE, 0)) return e;
    }
    prof_kernel_done(st);
    if (live_mask) *live_mask = live;
    return check_launch("fx_conv_dgrad_strided_any");
}

// input pixels of a strided 1x1 that no tap reaches: fx_conv_dgrad leaves them untouched, so a caller that does not accumulate zero-fills dx first
bool fx_dgrad_has_dead_classes(const p3d_conv_desc* d) { return d->stride > 1 && d->R == 1; }
// ... which is this: every caller of fx_conv_dgrad that hands out dx as a whole result runs it first
int32_t fx_dgrad_zero_dead_classes(const p3d_conv_desc* d, float* dx, hipStream_t st) {
    if (!fx_dgrad_has_dead_classes(d) || d->accumulate) return P3D_OK;
    if (hipMemsetAsync(dx, 0, (size_t)d->N * d->C * d->H * d->W * sizeof(float), st) != hipSuccess) { set_error("fx_conv_dgrad: zero fill of dx failed"); return P3D_ELAUNCH; }
    return P3D_OK;
}
// the dense unsplit launch can take its summand from another tensor (FxFuse::acc_src / acc_mask)
bool fx_dgrad_accumulates_from_source(const p3d_conv_desc* d) { return d->stride == 1 && fx_plan(d, true).splits == 1 && (d->H * d->W) % 4 == 0; }

// How many slabs (splits of the pixel reduction) a weight gradient is cut into.  Measured on MI355X over the ResNet layer classes at batch 64 with
// image operands (tools/split_sweep.py, profiles/r03_split_sweep.txt): the best block count depends on the tile count more than on anything else -- all
// blocks are resident at once (two or three per CU), so what matters is how evenly tiles x slabs covers the 256 CUs and whether the taps of one slab land on
// one XCD.  The round-2 plan (576 blocks for the 3x3 grids, 512 / 768 for powers of two, 3072 for the regressor) left 15-22 % on the 9-, 16-, 36- and
// 144-tile classes and 3 % on the regressor; other tile counts aim at one full round of three blocks per CU.
// image-fed weight gradients of 64-input-channel multi-tap layers pack two taps into a column tile (fx_wgrad_kernel<.., TAPS 2>)
// (returns the taps per column tile: 0 = the ordinary one-tap tiles, 2, or 3 when the output channels fit half an A image too)
static int fx_wgrad_two_taps(const p3d_conv_desc* d, bool images) {
    if (!images || d->C != 64 || d->R * d->S <= 1 || (d->Wo & 15)) return 0;
    return d->K <= 64 ? 3 : 2;
}
// ragged (fx_wgrad_any_kernel): the K steps are those of the flat pixel index, ceil(N Ho Wo / 16), and a block keeps at least 8 of them instead of 32 -- the floor of the
// fp32-MFMA plan (plan_wgrad, p3d_conv.hip).  A slab is one chain of 6 dependent fp32 accumulations per K step; at the small batches where the floor binds, 32 steps leave a
// whole reduction in one or two slabs on a handful of blocks, and its rounding error at several times that of the fp32-MFMA kernel, which sums many short slabs
// (profiles/train_anysize.md).  At batch 64 the floor binds for one class only (four tiles at 33 x 33).
// tt: the taps per column tile (the ragged kernels, image-fed or not, run one tap per block: 0)
static int fx_wgrad_splits(const p3d_conv_desc* d, int tt, bool ragged) {
    const int64_t tiles = tt ? ceil_div(d->K, FX_BM) * ceil_div(d->R * d->S, tt) : ceil_div(d->K, FX_BM) * ceil_div(d->C, FX_BN) * d->R * d->S;
    const int64_t total = ragged ? ceil_div((int64_t)d->N * d->Ho * d->Wo, FX_BK) : (int64_t)d->N * (d->Ho * d->Wo / FX_BK);
    int64_t target;
    if (g_wgrad_target > 0) target = g_wgrad_target;          // (tuning aid: p3d_fx_tune(2, n), tools/split_sweep.py)
    else if (tiles >= 256) target = 1536;
    else switch ((int)tiles) {
        case 2: target = 384; break;
        case 4: target = 640; break;
        case 5: target = 512; break;          // (two-tap column tiles of a 64 -> 64 3x3: profiles/r04_summary.md section 6)
        case 8: case 32: case 36: target = 512; break;
        case 16: target = 256; break;
        case 128: target = 1024; break;
        case 144: target = 720; break;
        default: target = 768;              // (1, 9, 64 tiles; anything the sweep has not seen)
    }
    int64_t splits = (2 * target + tiles) / (2 * tiles);                 // nearest
    const int min_steps = ragged ? 8 : 32;
    if (splits > total / min_steps) splits = total / min_steps;          // at least 32 K steps per block (ragged: 8)
    if (g_force_wgrad_splits > 0) splits = g_force_wgrad_splits < total ? g_force_wgrad_splits : total;
    if (splits < 1) splits = 1;
    const int64_t spb = ceil_div(total, splits);
    return (int)ceil_div(total, spb);
}

// Which operands an instance takes: the one validity rule of a weight-gradient call.  Aligned maps: a factor (dw = wgrad(dy * pmask, x * emask)) goes with an fp32
// operand -- an image carries its own --, never with two images; row images feed the dense image-fed instances; an image needs its channel count in steps of 16, and an
// x image a dy image beside it.  Any map width: two fp32 operands, with both factors of a partial convolution or neither, or two images without factors, their channel
// counts in steps of 16 and the map at least one K step (16 pixels); `rows` is not looked at there.
constexpr bool fx_wgrad_operands_ok(bool ragged, bool aimg, bool bimg, bool pm, bool em, bool rows, int K, int C, int ohw) {
    if (ragged) return aimg == bimg && pm == em && !(aimg && pm) && !(aimg && ((K & 15) || (C & 15) || ohw < FX_BK));
    if ((pm || em) && (pm == aimg || em == bimg || (aimg && bimg))) return false;
    if (rows && (!aimg || pm || em)) return false;
    return !((aimg && (K & 15)) || (bimg && (C & 15)) || (bimg && !aimg));
}

// Every compiled weight-gradient kernel, once: X(AIMG, BIMG, MASKED, TAPS, ROWS) of fx_wgrad_kernel (the last two are the stem's, fx_stem_wgrad) and X(family, kernel)
// of the three for any map width.  fx_wgrad_instance is the only place that names one.
#define P3D_FX_WGRAD_INSTANCES(X)                                                                                                    \
    X(1, 1, 0, 3, 1) X(1, 1, 0, 3, 0) X(1, 1, 0, 2, 1) X(1, 1, 0, 2, 0) X(1, 0, 1, 0, 0) X(0, 0, 1, 0, 0) X(1, 1, 0, 0, 1) X(1, 1, 0, 0, 0) \
    X(1, 0, 0, 0, 1) X(1, 0, 0, 0, 0) X(0, 0, 0, 0, 0) X(0, 1, 1, 1, 0) X(0, 1, 0, 1, 0)
#define P3D_FX_WGRAD_ANY_INSTANCES(X) X(FX_WG_ANY_IMG, fx_wgrad_any_img_kernel) X(FX_WG_ANY_MASKED, fx_wgrad_any_masked_kernel) X(FX_WG_ANY, fx_wgrad_any_kernel)
using FxWgradKernel = void (*)(const FxWgradParams);
constexpr FxWgradKernel fx_wgrad_instance(int family, bool aimg, bool bimg, bool masked, int taps, bool rows) {
#define P3D_X(FAMILY, KERNEL) if (family == FAMILY) return KERNEL;
    P3D_FX_WGRAD_ANY_INSTANCES(P3D_X)
#undef P3D_X
#define P3D_X(AIMG, BIMG, MASKED, TAPS, ROWS) if (aimg == AIMG && bimg == BIMG && masked == MASKED && taps == TAPS && rows == ROWS) return fx_wgrad_kernel<AIMG, BIMG, MASKED, TAPS, ROWS>;
    if (family == FX_WG_ALIGNED) { P3D_FX_WGRAD_INSTANCES(P3D_X) }
#undef P3D_X
    return nullptr;
}
// The instance of an operand combination the rule above admits: on aligned maps the operands ARE the template values, with the taps per column tile; at any map width
// one kernel per kind of operand.  Every such combination has its instance, on each column tile fx_wgrad_two_taps can ask for; and so have the stem's two.
constexpr int fx_wgrad_family(bool ragged, bool aimg, bool masked) { return !ragged ? FX_WG_ALIGNED : aimg ? FX_WG_ANY_IMG : masked ? FX_WG_ANY_MASKED : FX_WG_ANY; }
constexpr bool fx_wgrad_covered() {
    for (int c = 0; c < 64; ++c) {
        const bool ragged = c & 1, aimg = c & 2, bimg = c & 4, pm = c & 8, em = c & 16, rows = c & 32;
        if (!fx_wgrad_operands_ok(ragged, aimg, bimg, pm, em, rows, 64, 64, 256)) continue;
        for (int tt = 0; tt <= 3; tt += tt ? 1 : 2) {
            if (tt && !(aimg && bimg && !pm && !em && !ragged)) continue;          // (fx_wgrad_two_taps: image-fed dense launches only)
            if (!fx_wgrad_instance(fx_wgrad_family(ragged, aimg, pm || em), aimg, bimg, pm || em, tt, rows)) return false;
        }
    }
    return fx_wgrad_instance(FX_WG_ALIGNED, false, true, true, 1, false) && fx_wgrad_instance(FX_WG_ALIGNED, false, true, false, 1, false);
}
static_assert(fx_wgrad_covered(), "the weight-gradient plan can name an instance that is not compiled");

// The single description of a weight-gradient call (p3d_fx.h), from the descriptor and the kinds of its operands
FxWgradPlan fx_wgrad_plan(const p3d_conv_desc* d, const FxWgradOperands& o) {
    const bool ragged = o.ragged, aimg = o.aimg, bimg = o.bimg, masked = o.pm || o.em;
    const int RS = d->R * d->S, tt = ragged ? 0 : fx_wgrad_two_taps(d, aimg && bimg && !masked);
    FxWgradPlan pl{};
    pl.ok = fx_wgrad_operands_ok(ragged, aimg, bimg, o.pm, o.em, o.rows, d->K, d->C, d->Ho * d->Wo);
    pl.family = fx_wgrad_family(ragged, aimg, masked);
    if (!ragged) { pl.aimg = aimg; pl.bimg = bimg; pl.masked = masked; pl.taps = tt; pl.rows = o.rows; }
    pl.tile_taps = tt;
    pl.splits = fx_wgrad_splits(d, tt, ragged);
    // K steps: 16 consecutive output pixels of one image, or (any map width) of the flat pixel index, the last one partial
    pl.spb = (int)ceil_div(ragged ? ceil_div((int64_t)d->N * d->Ho * d->Wo, FX_BK) : (int64_t)d->N * (d->Ho * d->Wo / FX_BK), pl.splits);
    pl.grid = tt ? dim3((unsigned)ceil_div(RS, tt), (unsigned)ceil_div(d->K, FX_BM), (unsigned)pl.splits)
                 : dim3((unsigned)ceil_div(d->C, FX_BN), (unsigned)ceil_div(d->K, FX_BM), (unsigned)(pl.splits * RS));
    pl.order = fx_wgrad_order(d);
    pl.slab_bytes = (size_t)pl.splits * d->K * d->C * RS * sizeof(float);
    pl.tapm = RS > 1;
    return pl;
}

// a plan as the 16 values of p3d_fx_wgrad_plan (include/p3d_hip.h): the hook's answer and the head of a launch record
static void fx_wgrad_plan_fields(const FxWgradPlan& pl, int32_t* out) {
    const int32_t rec[P3D_FX_WGRAD_PLAN_FIELDS] = {pl.family, pl.aimg, pl.bimg, pl.masked, pl.taps, pl.rows, pl.tile_taps, pl.splits, pl.spb, (int32_t)pl.grid.x, (int32_t)pl.grid.y,
                                                  (int32_t)pl.grid.z, pl.order, pl.tapm, (int32_t)(pl.slab_bytes & 0xFFFFFFFFu), (int32_t)(pl.slab_bytes >> 32)};
    for (int i = 0; i < P3D_FX_WGRAD_PLAN_FIELDS; ++i) out[i] = rec[i];
}

// ---- what the weight gradient launched (p3d_fx_wgrad_launch_log): one record per fx_launch_wgrad, layout documented in include/p3d_hip.h ----------------
enum { FXWL_FINISH = P3D_FX_WGRAD_PLAN_FIELDS, FXWL_ACCUMULATE, FXWL_FIELDS = P3D_FX_WGRAD_LAUNCH_FIELDS };
static_assert(FXWL_ACCUMULATE < FXWL_FIELDS, "the record of p3d_fx_wgrad_launch_log outgrew its documented length");
constexpr int32_t FX_WGRAD_FIN_STEM = 256;       // fx_stem_dw_kernel, beside the FIN_ bits of wgrad_finish (p3d_conv.hip: 8 .. 128)
static std::mutex g_fx_wlog_mu;
static int32_t g_fx_wlog[FX_LOG_MAX][FXWL_FIELDS];
static int64_t g_fx_wlog_n = 0;         // launches since the last reset (the first FX_LOG_MAX are kept)
static int64_t g_fx_wlog_resets = 0;    // a reset between a launch and its finishing pass must not put the finishing bits onto another call's record
struct FxWgradLogSlot { int64_t slot, resets; };
int32_t fx_wgrad_launch_log(int32_t* out, int32_t max_records, int32_t reset) {
    std::lock_guard<std::mutex> lock(g_fx_wlog_mu);
    const int64_t kept = g_fx_wlog_n < FX_LOG_MAX ? g_fx_wlog_n : FX_LOG_MAX;
    for (int64_t i = 0; out && i < kept && i < max_records; ++i)
        for (int f = 0; f < FXWL_FIELDS; ++f) out[i * FXWL_FIELDS + f] = g_fx_wlog[i][f];
    const int32_t n = (int32_t)(g_fx_wlog_n < INT32_MAX ? g_fx_wlog_n : INT32_MAX);
    if (reset) { g_fx_wlog_n = 0; ++g_fx_wlog_resets; }
    return n;
}
// the finishing kernels that followed a launch, onto its record: `at` is what fx_launch_wgrad returned (nothing to do for a launch the log did not keep)
static void fx_wgrad_log_finish(FxWgradLogSlot at, int32_t finish) {
    std::lock_guard<std::mutex> lock(g_fx_wlog_mu);
    if (at.slot >= 0 && at.resets == g_fx_wlog_resets) g_fx_wlog[at.slot][FXWL_FINISH] = finish;
}

// the only launch of a weight-gradient kernel in the library (a plan that is `ok`, or the stem's: fx_wgrad_covered has its instance).  Writes the launch record from
// the plan it launches; returns the record's place for fx_wgrad_log_finish (slot -1 where the log is full)
static FxWgradLogSlot fx_launch_wgrad(const FxWgradParams& p, const FxWgradPlan& pl, int accumulate, hipStream_t st) {
    hipLaunchKernelGGL(fx_wgrad_instance(pl.family, pl.aimg, pl.bimg, pl.masked, pl.taps, pl.rows), pl.grid, dim3(256), 0, st, p);
    prof_kernel_done(st);
    std::lock_guard<std::mutex> lock(g_fx_wlog_mu);
    const FxWgradLogSlot at{g_fx_wlog_n < FX_LOG_MAX ? g_fx_wlog_n : -1, g_fx_wlog_resets};
    if (at.slot >= 0) {
        int32_t* r = g_fx_wlog[at.slot];
        for (int f = 0; f < FXWL_FIELDS; ++f) r[f] = 0;
        fx_wgrad_plan_fields(pl, r);
        r[FXWL_ACCUMULATE] = accumulate;
    }
    ++g_fx_wlog_n;
    return at;
}

// dw (=|+= by `accumulate`) of one convolution: plan -> workspace check (in the name of `entry`) -> slabs [split][k][tap][c] -> wgrad_finish
int32_t fx_conv_wgrad(const p3d_conv_desc* d, const float* dy, const float* x, float* dw, int accumulate, void* workspace, size_t workspace_bytes, const FxFuse* fuse,
                      const char* entry, hipStream_t st) {
    const FxWgradPlan pl = fx_wgrad_plan(d, fuse);
    if (!workspace || workspace_bytes < pl.slab_bytes) { set_error("%s: workspace %zu B < required %zu B", entry, workspace_bytes, pl.slab_bytes); return P3D_EWORKSPACE; }
    if (!pl.ok) {
        set_error("fx_conv_wgrad: no instance takes these operands (a factor goes with an fp32 operand, row images feed dense image-fed launches, an image needs channel counts in "
                  "steps of 16 and an x image a dy image; any map width: fp32 operands with both factors or neither, or two such images of 16 pixels or more without factors)");
        return P3D_EINVAL;
    }
    FxWgradParams p{};
    p.DY = dy; p.X = x; p.slabs = (float*)workspace;
    p.N = d->N; p.K = d->K; p.C = d->C; p.Hi = d->H; p.Wi = d->W; p.OH = d->Ho; p.OW = d->Wo; p.R = d->R; p.S = d->S;
    p.stride = d->stride; p.pad = d->pad; p.dil = d->dil;
    p.nsplit = pl.splits; p.spb = pl.spb; p.order = pl.order;
    if (fuse) {
        if (fuse->dy_img) { p.DYimg = (const unsigned char*)fuse->dy_img; p.dy_plane = (size_t)d->N * d->K * d->Ho * d->Wo * 2; }
        if (fuse->x_img) { p.Ximg = (const unsigned char*)fuse->x_img; p.x_plane = (size_t)d->N * d->C * d->H * d->W * 2; }
        p.amask = fuse->pmask; p.bmask = fuse->emask;
    }
    const FxWgradLogSlot at = fx_launch_wgrad(p, pl, accumulate, st);
    if (int32_t e = check_launch("fx_conv_wgrad")) return e;
    p3d_conv_desc dw_desc = *d;
    dw_desc.accumulate = accumulate;
    int32_t finish = 0;
    const int32_t e = wgrad_finish(&dw_desc, p.slabs, pl.splits, pl.tapm, dw, st, &finish);
    fx_wgrad_log_finish(at, finish);
    return e;
}


// ------------------------------------------------------------------------------------------------------------------------------------------
// The stem: conv1 = Conv2d(Cin, K, 7, stride 2, padding 3) with Cin = 3 (RGB) or 1 (depth) (depthnet.py:138).  Three input channels cannot feed a 16-deep
// K step, so the convolution is restated over a space-to-depth image of the input: x'[n][c * 4 + pi * 2 + pj][i][j] = x[n][c][2 i + pi][2 j + pj]
// (4 Cin <= 16 channels = ONE channel group, the rest zero).  Then   y[n][k][oh][ow] = sum_{r', s' in 0..3} sum_c' w'[k][c'][r'][s'] x'[n][c'][oh + r' - 2][ow + s' - 2]
// with w'[k][c * 4 + pi * 2 + pj][r'][s'] = w[k][c][2 r' - 1 + pi][2 s' - 1 + pj] (zero where that index leaves 0..6): a 4x4 stride-1 convolution over 16
// channels, 256 multiply-adds per output instead of 147 but on the bf16 pipe (fx_conv_kernel<AMODE 1>, 16 taps x 1 K step), and a weight gradient whose GEMM
// columns are the 16 x 16 (tap, channel) pairs (fx_wgrad_kernel<.., TAPS>).
// ------------------------------------------------------------------------------------------------------------------------------------------
// one thread per pixel of the half-resolution grid: 4 Cin input values -> three 32-B rows
__global__ __launch_bounds__(256) void fx_s2d_image_kernel(const float* __restrict__ x, const float* __restrict__ mask, unsigned char* __restrict__ img, size_t plane_bytes, int N,
                                                           int Cin, int H, int W) {
    const int H2 = H >> 1, W2 = W >> 1;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)N * H2 * W2) return;
    const int j2 = (int)(i % W2), i2 = (int)((i / W2) % H2), n = (int)(i / ((long long)W2 * H2));
    float v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c)                       // (static indices into v: a runtime-indexed register array would live in scratch)
#pragma unroll
        for (int pi = 0; pi < 2; ++pi)
            if (c < Cin) {
                const f32x2 q = *reinterpret_cast<const f32x2*>(x + (((size_t)n * Cin + c) * H + 2 * i2 + pi) * W + 2 * j2);
                float q0 = q[0], q1 = q[1];
                if (mask) {          // partial convolution (partial_conv.py:45): the operand is x * mask_in, one factor per pixel
                    const f32x2 mq = *reinterpret_cast<const f32x2*>(mask + ((size_t)n * H + 2 * i2 + pi) * W + 2 * j2);
                    // (two explicit scalar multiplies: written in C++ the pair is merged into v_pk_mul_f32 on its way into the packed conversion below, and the library
                    // must not contain packed-fp32 instructions -- csrc/Makefile, tests/test_build_flags.py)
                    asm("v_mul_f32 %0, %1, %2" : "=v"(q0) : "v"(q0), "v"(mq[0]));
                    asm("v_mul_f32 %0, %1, %2" : "=v"(q1) : "v"(q1), "v"(mq[1]));
                }
                v[c * 4 + pi * 2] = q0; v[c * 4 + pi * 2 + 1] = q1;
            }
    unsigned hp[8], mp[8], lp[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) fx_split2(v[2 * e], v[2 * e + 1], hp[e], mp[e], lp[e]);
    unsigned char* dst = img + (size_t)i * 32;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        *reinterpret_cast<i32x4*>(dst + 16 * h) = i32x4{(int)hp[4 * h], (int)hp[4 * h + 1], (int)hp[4 * h + 2], (int)hp[4 * h + 3]};
        *reinterpret_cast<i32x4*>(dst + plane_bytes + 16 * h) = i32x4{(int)mp[4 * h], (int)mp[4 * h + 1], (int)mp[4 * h + 2], (int)mp[4 * h + 3]};
        *reinterpret_cast<i32x4*>(dst + 2 * plane_bytes + 16 * h) = i32x4{(int)lp[4 * h], (int)lp[4 * h + 1], (int)lp[4 * h + 2], (int)lp[4 * h + 3]};
    }
}

// The same image of x zero-extended to (Hp, Wp) (p3d_stem_image_any: odd sides).  One thread per pixel of the padded half-resolution grid; every source element is a
// dword load checked against the true H and W (at odd W a row is only 4-B aligned), and what lies at or beyond them stays the exact zero v starts with, in all three planes.
__global__ __launch_bounds__(256) void fx_s2d_image_any_kernel(const float* __restrict__ x, const float* __restrict__ mask, unsigned char* __restrict__ img, size_t plane_bytes, int N,
                                                               int Cin, int H, int W, int H2, int W2) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)N * H2 * W2) return;
    const int j2 = (int)(i % W2), i2 = (int)((i / W2) % H2), n = (int)(i / ((long long)W2 * H2));
    float v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int pi = 0; pi < 2; ++pi)
#pragma unroll
            for (int pj = 0; pj < 2; ++pj) {
                const int h = 2 * i2 + pi, w = 2 * j2 + pj;
                if (c < Cin && h < H && w < W) {
                    float q = x[(((size_t)n * Cin + c) * H + h) * W + w];
                    if (mask) {          // (one explicit scalar multiply per value, as in fx_s2d_image_kernel: no packed-fp32 instruction may be formed)
                        const float mq = mask[((size_t)n * H + h) * W + w];
                        asm("v_mul_f32 %0, %1, %2" : "=v"(q) : "v"(q), "v"(mq));
                    }
                    v[c * 4 + pi * 2 + pj] = q;
                }
            }
    unsigned hp[8], mp[8], lp[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) fx_split2(v[2 * e], v[2 * e + 1], hp[e], mp[e], lp[e]);
    unsigned char* dst = img + (size_t)i * 32;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        *reinterpret_cast<i32x4*>(dst + 16 * h) = i32x4{(int)hp[4 * h], (int)hp[4 * h + 1], (int)hp[4 * h + 2], (int)hp[4 * h + 3]};
        *reinterpret_cast<i32x4*>(dst + plane_bytes + 16 * h) = i32x4{(int)mp[4 * h], (int)mp[4 * h + 1], (int)mp[4 * h + 2], (int)mp[4 * h + 3]};
        *reinterpret_cast<i32x4*>(dst + 2 * plane_bytes + 16 * h) = i32x4{(int)lp[4 * h], (int)lp[4 * h + 1], (int)lp[4 * h + 2], (int)lp[4 * h + 3]};
    }
}

// w [K][Cin][7][7] -> w' [K][16][4][4]
__global__ __launch_bounds__(256) void fx_stem_weights_kernel(const float* __restrict__ w, float* __restrict__ w2, int K, int Cin) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= K * 256) return;
    const int s2 = i & 3, r2 = (i >> 2) & 3, c2 = (i >> 4) & 15, k = i >> 8;
    const int c = c2 >> 2, pi = (c2 >> 1) & 1, pj = c2 & 1;
    const int r = 2 * r2 - 1 + pi, q = 2 * s2 - 1 + pj;
    w2[i] = (c < Cin && r >= 0 && r < 7 && q >= 0 && q < 7) ? w[((size_t)(k * Cin + c) * 7 + r) * 7 + q] : 0.f;
}

// slabs [split][K][256 = tap * 16 + c'] -> dw [K][Cin][7][7] (=|+=).  One thread per (k, column): consecutive threads sum consecutive columns over the splits
// (coalesced), then the columns that are a weight (c < Cin, the tap inside the 7x7 window) are scattered to it.
__global__ __launch_bounds__(1024) void fx_stem_dw_kernel(const float* __restrict__ slabs, int nsplit, float* __restrict__ dw, int K, int Cin, int accumulate) {
    // grid (K, 4): block = output channel k, 64 of its 256 restated columns; 16 groups of 64 threads sum every 16th slab, group 0 adds the 16 partial sums in order
    __shared__ float part[16][64];
    const int k = blockIdx.x, t = threadIdx.x, g = t >> 6, cl = t & 63, col = blockIdx.y * 64 + cl;
    float acc = 0.f;
    for (int z = g; z < nsplit; z += 16) acc += slabs[((size_t)z * K + k) * 256 + col];
    part[g][cl] = acc;
    __syncthreads();
    if (g != 0) return;
    acc = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) acc += part[j][cl];
    const int tp = col >> 4, c2 = col & 15;
    const int c = c2 >> 2, pi = (c2 >> 1) & 1, pj = c2 & 1;
    const int r = 2 * (tp >> 2) - 1 + pi, q = 2 * (tp & 3) - 1 + pj;
    if (c < Cin && r >= 0 && r < 7 && q >= 0 && q < 7) {
        float* d = dw + ((size_t)(k * Cin + c) * 7 + r) * 7 + q;
        *d = accumulate ? *d + acc : acc;
    }
}

bool fx_stem_applies(int N, int Cin, int H, int W, int K) {
    return fx_enabled() && N > 0 && (Cin == 1 || Cin == 3 || Cin == 2 || Cin == 4) && K >= 32 && K % 16 == 0 && K <= 128 && H % 2 == 0 && W % 8 == 0 && ((H / 2) * (W / 2)) % 16 == 0 &&
           (int64_t)N * K * (H / 2) * (W / 2) < (1ll << 29);
}
size_t fx_stem_image_bytes(int N, int H, int W) { return (size_t)3 * N * (H / 2) * (W / 2) * 32; }
size_t fx_stem_weight_image_bytes(int K) { return fx_weight_image_bytes(K, 16, 16, false); }
static int fx_stem_splits(int N, int H, int W) {
    const int64_t total = (int64_t)N * ((H / 2) * (W / 2) / FX_BK);
    int64_t splits = 384;                      // 2 column tiles x 384 = 768 blocks: one resident round
    if (splits > total / 32) splits = total / 32;
    if (splits < 1) splits = 1;
    const int64_t spb = ceil_div(total, splits);
    return (int)ceil_div(total, spb);
}
// The stem's weight gradient as a plan: fx_wgrad_kernel<false, true, MASKED, TAPS 1> over the 16 x 16 (tap, channel) columns, two tiles of eight taps; its own split
// rule above and its own finish (fx_stem_dw_kernel)
static FxWgradPlan fx_stem_wgrad_plan(int N, int H, int W, int K, bool masked) {
    FxWgradPlan pl{};
    pl.ok = true; pl.family = FX_WG_ALIGNED; pl.bimg = true; pl.masked = masked; pl.taps = 1; pl.tile_taps = 8;
    pl.splits = fx_stem_splits(N, H, W);
    pl.spb = (int)ceil_div((int64_t)N * ((H / 2) * (W / 2) / FX_BK), pl.splits);
    pl.grid = dim3(2, (unsigned)ceil_div(K, FX_BM), (unsigned)pl.splits);
    pl.slab_bytes = (size_t)pl.splits * K * 256 * sizeof(float);
    pl.tapm = true;
    return pl;
}
size_t fx_stem_workspace(int N, int H, int W, int K) {
    const size_t w2 = align256((size_t)K * 256 * sizeof(float));
    const size_t slabs = fx_stem_wgrad_plan(N, H, W, K, false).slab_bytes;
    return w2 > slabs ? w2 : slabs;
}

int32_t fx_stem_image(const float* x, const float* mask, void* img, int N, int Cin, int H, int W, hipStream_t st) {
    const long long total = (long long)N * (H / 2) * (W / 2);
    hipLaunchKernelGGL(fx_s2d_image_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, st, x, mask, (unsigned char*)img, (size_t)total * 32, N, Cin, H, W);
    return check_launch("fx_stem_image");
}

int32_t fx_stem_image_any(const float* x, const float* mask, void* img, int N, int Cin, int H, int W, int Hp, int Wp, hipStream_t st) {
    const long long total = (long long)N * (Hp / 2) * (Wp / 2);
    hipLaunchKernelGGL(fx_s2d_image_any_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, st, x, mask, (unsigned char*)img, (size_t)total * 32, N, Cin, H, W, Hp / 2, Wp / 2);
    return check_launch("fx_stem_image_any");
}

// w [K][Cin][7][7] -> the forward weight image of the restated convolution (workspace: K * 256 floats)
int32_t fx_stem_weight_image(const float* w, int K, int Cin, void* wimg, void* workspace, hipStream_t st) {
    hipLaunchKernelGGL(fx_stem_weights_kernel, dim3((unsigned)ceil_div((int64_t)K * 256, 256)), dim3(256), 0, st, w, (float*)workspace, K, Cin);
    return fx_build_weight_images((const float*)workspace, K, 16, 16, wimg, nullptr, st);
}

static FxConvParams fx_stem_params(int N, int H, int W, int K) {
    FxConvParams p{};
    const int H2 = H / 2, W2 = W / 2;
    p.N = N; p.Cred = 16; p.Hi = H2; p.Wi = W2; p.M = K; p.OH = H2; p.OW = W2; p.NP = N * H2 * W2;
    p.YH = H2; p.YW = W2; p.oy0 = 0; p.ox0 = 0; p.oys = 1; p.oxs = 1;
    p.R = 4; p.S = 4; p.nR = 4; p.nS = 4; p.ntap = 16; p.r0 = 0; p.rstep = 1; p.s0 = 0; p.sstep = 1;
    p.hmul = 1; p.hoff = -2; p.hstep = 1; p.wmul = 1; p.woff = -2; p.wstep = 1;
    p.tiles_m = (int)ceil_div(K, FX_BM);
    return p;
}

// y [N][K][H/2][W/2] = conv1(x) from the space-to-depth image of x and the restated weight image
bool fx_stem_masked_applies(int K) { return fx16_bm(K, true, 0, FX_EPI_STORE) != 0; }       // the per-pixel output factor lives in the fx16 kernel's epilogue
int32_t fx_stem_fwd(const void* x_img, const void* wimg, float* y, const float* mult, int N, int H, int W, int K, hipStream_t st) {
    FxConvParams p = fx_stem_params(N, H, W, K);
    if (mult) {
        if (!fx_stem_masked_applies(K)) { set_error("fx_stem_fwd: the output factor needs the fx16 kernel (K <= 64 or a 96-row fit)"); return P3D_EINVAL; }
        p.emask = mult;
    }
    p.Ximg = (const unsigned char*)x_img; p.plane_bytes = (size_t)N * (H / 2) * (W / 2) * 32;
    p.Wimg = (const unsigned char*)wimg; p.Y = y;
    const int tiles_n = (int)ceil_div(p.NP, FX_BN);
    const int bm = fx16_bm(K, true, 0, FX_EPI_STORE);
    if (bm) p.tiles_m = (int)ceil_div(K, bm);
    if (int32_t e = fx_launch_conv(p, true, 0, FX_EPI_STORE, bm, dim3((unsigned)(p.tiles_m * tiles_n), 1), st)) return e;
    return check_launch("fx_stem_fwd");
}

// The plan as the record of the test hook p3d_fx_wgrad_plan (include/p3d_hip.h): fx_wgrad_plan for the operands the bits describe, or with bit 6 the
// stem's, the descriptor's N, C, H, W, K being its arguments
int32_t fx_wgrad_plan_record(const p3d_conv_desc* d, int operands, int32_t* out) {
    FxWgradPlan pl{};
    if (operands & 64) {
        if ((operands & ~(64 | 8)) || !fx_stem_applies(d->N, d->C, d->H, d->W, d->K)) { set_error("fx_wgrad_plan: not a stem the x3 kernels take, or operand bits the stem has not"); return P3D_EINVAL; }
        pl = fx_stem_wgrad_plan(d->N, d->H, d->W, d->K, (operands & 8) != 0);
    } else {
        const FxWgradOperands o{(operands & 1) != 0, (operands & 2) != 0, (operands & 8) != 0, (operands & 16) != 0, (operands & 4) != 0, (operands & 32) != 0};
        if (!fx_applies(FX_WGRAD, d, 32, o.ragged)) { set_error("fx_wgrad_plan: shape outside the x3 kernels"); return P3D_EINVAL; }
        pl = fx_wgrad_plan(d, o);
        if (!pl.ok) { set_error("fx_wgrad_plan: no instance takes these operands"); return P3D_EINVAL; }
    }
    fx_wgrad_plan_fields(pl, out);
    return P3D_OK;
}

// dw [K][Cin][7][7] (=|+=) from dy [N][K][H/2][W/2] (fp32) and the space-to-depth image of x
int32_t fx_stem_wgrad(const float* dy, const float* mult, const void* x_img, float* dw, int N, int Cin, int H, int W, int K, int accumulate, void* workspace,
                      size_t workspace_bytes, hipStream_t st) {
    if (!workspace || workspace_bytes < fx_stem_workspace(N, H, W, K)) { set_error("fx_stem_wgrad: workspace %zu B < required %zu B", workspace_bytes, fx_stem_workspace(N, H, W, K)); return P3D_EWORKSPACE; }
    FxWgradParams p{};
    const int H2 = H / 2, W2 = W / 2;
    p.DY = dy; p.Ximg = (const unsigned char*)x_img; p.x_plane = (size_t)N * H2 * W2 * 32; p.slabs = (float*)workspace;
    p.N = N; p.K = K; p.C = 256; p.Hi = H2; p.Wi = W2; p.OH = H2; p.OW = W2; p.R = 4; p.S = 4; p.stride = 1; p.pad = 2; p.dil = 1;
    const FxWgradPlan pl = fx_stem_wgrad_plan(N, H, W, K, mult != nullptr);
    p.nsplit = pl.splits; p.spb = pl.spb;
    p.amask = mult;      // partial convolution: dw = wgrad(dy * mult, x * mask_in); the image holds x * mask_in, dy is scaled on its way into LDS
    const FxWgradLogSlot at = fx_launch_wgrad(p, pl, accumulate, st);
    hipLaunchKernelGGL(fx_stem_dw_kernel, dim3((unsigned)K, 4), dim3(1024), 0, st, (const float*)workspace, p.nsplit, dw, K, Cin, accumulate);
    fx_wgrad_log_finish(at, FX_WGRAD_FIN_STEM);
    return check_launch("fx_stem_wgrad");
}

}  // namespace p3d
