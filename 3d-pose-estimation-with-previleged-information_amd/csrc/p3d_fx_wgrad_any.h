// The one text of the ragged weight-gradient kernels, included by p3d_fx.hip once per kernel (the comment there describes it) with
//   P3D_FX_WGRAD_ANY_KERNEL   the kernel's name
//   P3D_FX_WGRAD_ANY_MASKED   false / true: the per-pixel factors of a partial convolution
// A textual include rather than a template or a shared device function: fx_wgrad_any_kernel keeps its symbol AND its code (through an inlined body the
// compiler schedules the unmasked kernel's prologue differently; tools/isa_diff.py).  No include guard: it is meant to be read twice.
__global__ __launch_bounds__(256, 3) void P3D_FX_WGRAD_ANY_KERNEL(const FxWgradParams p) {
    constexpr bool MASKED = P3D_FX_WGRAD_ANY_MASKED;
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
    const int row = t >> 2, kq = t & 3;                                      // rows row, row + 64 of the tile, pixels 4 kq .. 4 kq + 3 of the step
    const int a_bad[2] = {m0 + row < p.K ? 0 : FX_OOB, m0 + row + 64 < p.K ? 0 : FX_OOB}, b_bad[2] = {n0 + row < p.C ? 0 : FX_OOB, n0 + row + 64 < p.C ? 0 : FX_OOB};
    const i32x4 rA = fx_rsrc(p.DY, (size_t)p.N * p.K * OHW * sizeof(float));
    const i32x4 rB = fx_rsrc(p.X, (size_t)p.N * p.C * HWi * sizeof(float));
    i32x4 rAM = {}, rBM = {};
    if constexpr (MASKED) { rAM = fx_rsrc(p.amask, (size_t)p.N * OHW * sizeof(float)); rBM = fx_rsrc(p.bmask, (size_t)p.N * HWi * sizeof(float)); }
    const int a_so = 64 * OHW * 4, b_so = 64 * HWi * 4;                      // the second row (wave-uniform; the per-pixel image offsets live in the thread's offsets)
    const int a_nimg = p.K * OHW, b_nimg = p.C * HWi;                        // elements per image
    const int di = FX_BK / OHW, dr = (FX_BK - di * OHW) / p.OW, dc = FX_BK - di * OHW - dr * p.OW;
    int f_q = s0 * FX_BK + 4 * kq, f_oh, f_ow, f_a, f_b;
    int f_m = 0;                                         // MASKED: element offset of the image's plane of bmask
    {
        const int qc = f_q < NP ? f_q : 0;               // (a thread that starts beyond the end stays beyond it: its position is never used)
        const int n = qc / OHW, rem = qc - n * OHW;
        f_oh = rem / p.OW; f_ow = rem - f_oh * p.OW;
        f_a = (n * p.K + m0 + row) * OHW; f_b = (n * p.C + n0 + row) * HWi;
        if constexpr (MASKED) f_m = n * HWi;
    }
    f32x4 ra[2], rb[2];
    f32x4 ram, rbm;              // MASKED: the per-pixel factors of the fetched K step
    auto fetch = [&]() {
        int a_voff[4], b_voff[4];
        int am_voff[4], bm_voff[4];
        int oh = f_oh, ow = f_ow, ia = f_a, ib = f_b;
        int im = f_m;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool ok = f_q + e < NP;
            const int hi = oh * p.stride + dh, wi = ow * p.stride + dw;
            a_voff[e] = ok ? (ia + oh * p.OW + ow) * 4 : FX_OOB;
            b_voff[e] = (ok && (unsigned)hi < (unsigned)p.Hi && (unsigned)wi < (unsigned)p.Wi) ? (ib + hi * p.Wi + wi) * 4 : FX_OOB;
            if constexpr (MASKED) {
                am_voff[e] = ok ? (f_q + e) * 4 : FX_OOB;
                bm_voff[e] = b_voff[e] >= 0 ? (im + hi * p.Wi + wi) * 4 : FX_OOB;
            }
            if (++ow == p.OW) {      // the next flat pixel: next row, next image
                ow = 0;
                if (++oh == p.OH) { oh = 0; ia += a_nimg; ib += b_nimg; if constexpr (MASKED) im += HWi; }
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ra[i][e] = fx_buffer_load_f32(rA, a_voff[e] | a_bad[i], i * a_so, 0);
                rb[i][e] = fx_buffer_load_f32(rB, b_voff[e] | b_bad[i], i * b_so, 0);
            }
        if constexpr (MASKED) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ram[e] = fx_buffer_load_f32(rAM, am_voff[e], 0, 0);
                rbm[e] = fx_buffer_load_f32(rBM, bm_voff[e], 0, 0);
            }
        }
        // the thread's first pixel of the next K step
        f_q += FX_BK;
        f_ow += dc;
        if (f_ow >= p.OW) { f_ow -= p.OW; ++f_oh; }
        f_oh += dr;
        int carry = di;
        if (f_oh >= p.OH) { f_oh -= p.OH; ++carry; }
        f_a += carry * a_nimg; f_b += carry * b_nimg;
        if constexpr (MASKED) f_m += carry * HWi;
    };
    const int st_off[2] = {fx_rc_off(row, kq >> 1) + 8 * (kq & 1), fx_rc_off(row + 64, kq >> 1) + 8 * (kq & 1)};
    auto stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            f32x4 va = ra[i], vb = rb[i];
            if constexpr (MASKED) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { va[e] *= ram[e]; vb[e] *= rbm[e]; }
            }
            fx_split_store(As + buf * 3 * FX_PIECE + st_off[i], va);
            fx_split_store(Bs + buf * 3 * FX_PIECE + st_off[i], vb);
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
    int rd_a[2], rd_b[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        rd_a[a] = fx_rc_off(wm * 64 + a * 32 + fr, fh);
        rd_b[a] = fx_rc_off(wn * 64 + a * 32 + fr, fh);
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
                    if (a < NA) af[pc][a] = *reinterpret_cast<const bf8*>(As + (buf * 3 + pc) * FX_PIECE + rd_a[a]);
            };
            auto read_b = [&](int pc) {
#pragma unroll
                for (int a = 0; a < 2; ++a)
                    if (a < NB) bf[pc][a] = *reinterpret_cast<const bf8*>(Bs + (buf * 3 + pc) * FX_PIECE + rd_b[a]);
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
