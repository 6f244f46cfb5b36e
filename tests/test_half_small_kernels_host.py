"""What tests/test_half_small_kernels_gpu.py takes for granted, checked without a GPU: that each case meant to reach a block cap, to leave one pass of a grid or
to run both loops of hbn_sum_partials does so (and that each cap is also met from below), the block and row counts its BatchNorm sizes yield, the number of
additions behind one fp32 block partial, the variance floor of the synthetic tables, and the float64 restatements of that file against oracle/np_ops.py.  The
case builders are imported from the GPU file, so both files see the same inputs."""
import numpy as np
import torch

import test_half_small_kernels_gpu as cases
from oracle import np_ops as ref

# What one pass of each launch covers.  This table is a COPY of constants in the C sources (grid caps x block size x elements per thread), by launch line; whoever
# raises a cap there raises it here, and the tests below then say which case has to grow with it.
ONE_PASS = dict(
    hbn_sums_blocks=512,                  # p3d_hbn.hip hbn_geom: min(ceil(ceil(P / PL) / 8), HBN_MAX_BLOCKS) blocks of PL pixels; hbn_stats_kernel, hbn_bwd_reduce_kernel
    hbn_stream_blocks=2048,               # p3d_hbn.hip hbn_stream_grid: the same count capped at 2048; hbn_apply_kernel, hbn_bwd_apply_kernel
    hbn_u=4,                              #   HBN_U pixels per thread and trip of the apply kernels and of hbn_bwd_reduce_kernel
    hbn_pixels_per_thread=8,              #   the 8 of both block counts
    hbn_group_cap=256,                    #   Gb = min(C / 8, 256) groups per block, PL = 256 / Gb pixel lanes; gridDim.y = (C / 8) / Gb
    sum_partials_slices=16,               # p3d_hbn.hip hbn_sum_partials: 16 slices of the row list per channel,
    sum_partials_rows_per_trip=4,         #   four rows (16 apart) per trip while blk + 48 < nblk, then one row per trip
    hconcat=8192 * 256,                   # p3d_hbn.hip p3d_hconcat: min(ceil_div(P * (Ca + Cb) / 8, 256), 8192) x 256 16-byte chunks
    hrelu=8192 * 256,                     # p3d_hbn.hip p3d_hrelu: min(ceil_div(n / 8, 256), 8192) x 256 chunks
    hmaxpool=16384 * 256,                 # p3d_hbn.hip p3d_hmaxpool3x3s2_fwd / _bwd: (output pixel, group) forward, (input pixel, group) backward
    hscale=8192 * 256,                    # p3d_hconv.hip p3d_hscale_pixels: (pixel, group)
    to_nhwc=8192 * 256,                   # p3d_hconv.hip p3d_nchw_f32_to_nhwc_f16: (pixel, 8 channels of Cpad)
    to_nchw_c8=8192 * 256,                # p3d_hconv.hip p3d_nhwc_f16_to_nchw_f32, C % 8 == 0 and a 16-byte aligned source: (image, 8 channels, pixel)
    to_nchw=8192 * 256,                   #   otherwise nhwc_f16_to_nchw_f32_kernel: elements
    weight_images=4096 * 256,             # p3d_hconv.hip p3d_weight_images_f16: elements of the [K][RS][Cpad] image
    weight_images_batched=128,            # p3d_hconv.hip p3d_weight_images_f16_batched: dim3(128, njobs), a 32 x 32 (k, c) tile per block and trip
    hbgrad=256,                           # p3d_hconv.hip p3d_hconv2d_bgrad: one block of 256 per 8 channels, a pixel per thread and trip
)


def crossed_and_met(sizes, one):
    return any(s > one for s in sizes) and any(s <= one for s in sizes)


def test_grid_stride_caps_are_crossed_and_met_from_below():
    one = ONE_PASS
    assert crossed_and_met([p * (ca + cb) // 8 for ca, cb, p in cases.CONCAT_CASES], one['hconcat'])
    assert (8, 24, 524291) in cases.CONCAT_CASES and {(24, 8, 1), (64, 64, 100)} <= set(cases.CONCAT_CASES)
    assert crossed_and_met([n // 8 for n in cases.RELU_SIZES], one['hrelu']) and all(n % 8 == 0 for n in cases.RELU_SIZES)
    assert crossed_and_met([p * c // 8 for p, c in cases.SCALE_CASES], one['hscale'])
    assert crossed_and_met([n * hw * cpad // 8 for n, c, hw, cpad in cases.TO_NHWC_CASES], one['to_nhwc']) and {(c, cpad) for _, c, _, cpad in cases.TO_NHWC_CASES} == {(3, 8), (5, 16)}
    c8 = [n * c // 8 * hw for route, n, c, hw, off in cases.TO_NCHW_CASES if route == 'c8']
    ew = [n * c * hw for route, n, c, hw, off in cases.TO_NCHW_CASES if route == 'elementwise']
    assert crossed_and_met(c8, one['to_nchw_c8']) and crossed_and_met(ew, one['to_nchw'])
    for route, n, c, hw, off in cases.TO_NCHW_CASES:                                  # the route each case names is the one the entry takes
        assert (route == 'c8') == (c % 8 == 0 and off % 8 == 0)
    assert any(c % 8 == 0 and off == 4 for _, _, c, _, off in cases.TO_NCHW_CASES) and ('elementwise', 2, 17, 61700, 0) in cases.TO_NCHW_CASES
    fwd = [n * ((h - 1) // 2 + 1) * ((w - 1) // 2 + 1) * c // 8 for n, c, h, w in cases.POOL_SHAPES]
    bwd = [n * h * w * c // 8 for n, c, h, w in cases.POOL_SHAPES]
    assert crossed_and_met(fwd, one['hmaxpool']) and crossed_and_met(bwd, one['hmaxpool'])
    n, c, h, w = cases.POOL_SHAPES[2]
    assert c // 8 == 8 and n * h * w * 8 > one['hmaxpool'] >= n * ((h - 1) // 2 + 1) * ((w - 1) // 2 + 1) * 8      # 9 x 64 x 243 x 241: the backward cap alone, G = 8
    assert crossed_and_met([k * rs * ((c + 7) // 8 * 8) for k, c, rs in cases.WEIGHT_CASES], one['weight_images'])
    tiles = [((k + 31) // 32) * (((c + 7) // 8 * 8 + 31) // 32) for k, c, rs, _ in cases.BATCHED_JOBS]
    assert tiles == [256, 3, 2] and crossed_and_met(tiles, one['weight_images_batched'])
    assert [j[3] for j in cases.BATCHED_JOBS] == [True, False, True]
    assert crossed_and_met(cases.BGRAD_P, one['hbgrad']) and {255, 257} <= set(cases.BGRAD_P) and max(cases.BGRAD_P) > 64 * one['hbgrad']


def test_batched_plan_leaves_gaps_and_stays_apart():
    rows, nflat, nimg = cases.batched_plan()
    spans = []
    for w_off, a, b, k, c, rs, cpad in rows:
        n = k * rs * cpad
        spans += [(a, a + n)] + ([(b, b + n)] if b >= 0 else [])
        assert w_off >= cases.BATCHED_GAP and w_off + k * c * rs <= nflat
    spans.sort()
    assert spans[0][0] == cases.BATCHED_GAP and spans[-1][1] + cases.BATCHED_GAP == nimg
    assert all(nxt[0] - cur[1] == cases.BATCHED_GAP for cur, nxt in zip(spans, spans[1:]))


def test_hbn_geometry_constants():
    one = ONE_PASS
    assert (cases.HBN_MAX_BLOCKS, cases.HBN_STREAM_BLOCKS, cases.HBN_U) == (one['hbn_sums_blocks'], one['hbn_stream_blocks'], one['hbn_u'])
    for c, p in cases.HBN_SIZES:
        g, gb, pl, nblk, nstream, gy = cases.hbn_geom(p, c)
        assert gb == min(c // 8, one['hbn_group_cap']) and pl * gb == 256 and gy * gb == g
        want = max(-(-(-(-p // pl)) // one['hbn_pixels_per_thread']), 1)
        assert nblk == min(want, one['hbn_sums_blocks']) and nstream == min(want, one['hbn_stream_blocks'])


def test_hbn_sizes_yield_the_block_counts_they_are_there_for():
    geom = {(c, p): cases.hbn_geom(p, c) for c, p in cases.HBN_SIZES}
    at_2048 = [p for c, p in cases.HBN_SIZES if c == 2048]
    assert at_2048 == [1, 7, 136, 523, 4096, 4101, 16389]
    assert [geom[(2048, p)][3] for p in at_2048] == [1, 1, 17, 66, 512, 512, 512]             # rows of the table hbn_sum_partials adds
    assert [geom[(2048, p)][4] for p in at_2048] == [1, 1, 17, 66, 512, 513, 2048]             # blocks of the apply launches
    assert geom[(2048, 1)][2] == 1                                                            # PL 1
    # 4096: exactly the cap, nothing ragged; 4101: one block more wanted than the cap gives, so the statistics loop runs a 9th, ragged time (5 pixels for 512 blocks)
    assert 4096 == 8 * 512 and -(-4101 // 8) == 513 and 4101 - 8 * 512 == 5
    # ... and the apply kernels (513 blocks, 4 pixels per trip) take a second trip that ends inside its 4th pixel row
    step = geom[(2048, 4101)][4]
    assert cases.HBN_U * step < 4101 < 2 * cases.HBN_U * step and (4101 - cases.HBN_U * step) % step != 0
    # 16389: the apply grid capped; a trip is 2048 blocks x 4 pixels, and the third trip holds 5 pixels
    assert -(-16389 // 8) > 2048 and 16389 - 2 * 2048 * cases.HBN_U == 5
    # two pixel lanes per group, capped on the statistics side
    g, gb, pl, nblk, nstream, gy = geom[(1024, 8195)]
    assert pl == 2 and nblk == 512 and nstream == 513 and 8195 % 2 == 1
    assert geom[(4096, 37)][5] == 2 and geom[(4096, 37)][1] == 256                           # gridDim.y = 2: a nonzero gbase in hbn_block_reduce
    assert all(geom[k][5] == 1 for k in geom if k[0] <= 2048)
    assert geom[(64, 769)][2] == 32 and geom[(64, 769)][3] == 4 and 769 % 32 == 1
    assert [geom[(8, p)][2:5] for p in (255, 257, 2049)] == [(256, 1, 1), (256, 1, 1), (256, 2, 2)]   # one pixel short of a block's lanes, one past, several blocks
    # the modes
    assert len(cases.HBN_CASES) == 4 * (len(cases.HBN_SIZES) - 1) + 2
    assert {(r, s) for c, p, r, s in cases.HBN_CASES if p == 16389} == {(1, 1), (1, 0)}
    assert all({(r, s) for c, p, r, s in cases.HBN_CASES if (c, p) == size} == set(cases.HBN_MODES) for size in cases.HBN_SIZES if size[1] != 16389)
    assert set(cases.HBN_FROZEN_SIZES) == {(2048, 523), (2048, 4101), (64, 769)} <= set(cases.HBN_SIZES)


def sum_partials_trips(rows, sl):
    """hbn_sum_partials for slice `sl` of 16: (four-row trips, one-row trips, the rows it reads), the loop written out"""
    read, four, tail = [], 0, 0
    blk = sl
    while blk + 48 < rows:
        read += [blk, blk + 16, blk + 32, blk + 48]
        four += 1
        blk += 64
    while blk < rows:
        read.append(blk)
        tail += 1
        blk += 16
    return four, tail, read


def test_table_rows_run_both_loops_of_sum_partials():
    assert ONE_PASS['sum_partials_slices'] == 16 and ONE_PASS['sum_partials_rows_per_trip'] == 4
    kinds = {}
    for rows in sorted(set(cases.TABLE_ROWS) | {cases.hbn_geom(p, c)[3] for c, p in cases.HBN_SIZES}):
        trips = [sum_partials_trips(rows, sl) for sl in range(16)]
        assert sorted(r for _, _, read in trips for r in read) == list(range(rows))           # every row once
        kinds[rows] = (max(t[0] for t in trips), max(t[1] for t in trips), any(t[0] and t[1] for t in trips))
    assert cases.TABLE_ROWS == [1, 15, 16, 17, 48, 49, 63, 64, 65, 113, 512, 2048, 2051] and cases.TABLE_CHANNELS == [8, 2048]
    assert all(kinds[r][0] == 0 for r in (1, 15, 16, 17, 48)) and kinds[48][1] == 3            # the tail alone, up to three rows of it
    assert kinds[49] == (1, 3, False) and kinds[63] == (1, 3, False)                          # some slices take a four-row trip, the others the tail
    assert kinds[64] == (1, 0, False)                                                         # the four-row loop alone
    assert kinds[65] == (1, 1, True) and kinds[113] == (2, 3, True)                 # a slice runs a four-row trip and then the tail
    assert kinds[512] == (8, 0, False) and kinds[2048] == (32, 0, False) and kinds[2051] == (32, 1, True)
    assert kinds[17] == (0, 2, False) and kinds[66] == (1, 1, True) and kinds[4] == (0, 1, False)   # the BatchNorm sizes: 17, 66 and 4 blocks


def test_additions_behind_one_block_partial():
    """dgamma / dbeta are checked at 1e-5 * sum |terms|.  A block partial is an fp32 sum whose longest path takes hbn_additions(P, C) additions (a thread's pixels,
    then the PL lanes of hbn_block_reduce); what follows is an fp64 sum and one cast.  While that count stays at or below 160 the worst case of fp32,
    160 * 2^-24 = 9.5e-6, supports the figure: that holds for every size with PL <= 32.  At C = 8 the 256 lanes of a block are summed one after the other, so
    the count is 257 to 261 and the worst case 1.6e-5; the figure stands there on the roundings not all pointing one way (their root-sum-square is
    sqrt(261) * 2^-25 = 4.8e-7), and on an MI355X the three sizes came to at most 6e-8 of sum |terms| in all four modes (dbeta 1e-8): inside the
    figure and inside the worst case alike (profiles/half_small_kernel_parity.md)."""
    for c, p in cases.HBN_SIZES:
        adds = cases.hbn_additions(p, c)
        pl = cases.hbn_geom(p, c)[2]
        if pl <= 32:
            assert adds <= 160 and (adds + 1) * 2.0 ** -24 < 1e-5, (c, p, adds)
        else:
            assert c == 8 and pl == 256 and adds <= 8 + 256, (c, p, adds)
    assert cases.hbn_additions(16389, 2048) == 34 and cases.hbn_additions(8195, 1024) == 11 and cases.hbn_additions(769, 64) == 39
    assert [cases.hbn_additions(p, 8) for p in (255, 257, 2049)] == [257, 258, 261]
    assert max(-(-p // 256) for p in cases.BGRAD_P) + 6 + 3 <= 160                            # hbgrad_kernel: a thread's pixels, six wave_sum steps, four waves


def test_synthetic_tables_keep_the_variance_floor():
    for rows in cases.TABLE_ROWS:
        for c in cases.TABLE_CHANNELS:
            d = cases.table_inputs(rows, c)
            assert d['table'].shape == (rows, c // 8, 16) and d['table'].dtype == np.float32 and d['x'].shape == (cases.TABLE_P, c)
            st = cases.table_stats(d)
            assert st['var'].min() >= cases.TABLE_VAR_FLOOR, (rows, c, st['var'].min())
            assert (d['coef'][:, 0] > 0).all() and (d['coef'][:, 3] > 0).all()
            s1, s2 = cases.table_sums(d['table'])                                              # the backward half: dx stays well inside fp16
            sc, mu, inv = (d['coef'][:, i].astype(np.float64) for i in (0, 2, 3))
            xhat = np.abs((d['x'].astype(np.float64) - mu) * inv).max(0)
            assert (sc * (np.abs(d['dy'].astype(np.float64)).max(0) + np.abs(s1) / cases.TABLE_P + xhat * np.abs(s2) / cases.TABLE_P)).max() < 1000, (rows, c)


def test_float64_restatements_match_the_oracle():
    """apply_want, bn_sums, dx_want and table_stats of the GPU file, on CPU tensors, against oracle/np_ops.py: the same statistics handed over as a coefficient table
    or as a two-row table of partial sums give the oracle's y, dx, dgamma, dbeta and running statistics"""
    rng = np.random.default_rng(0)
    p, c = 45, 16
    x, res, dy = (cases.r16(rng.standard_normal((p, c)) * s + m) for s, m in ((2, 1), (1, 0), (1, 0)))
    gamma, beta = (1 + 0.2 * rng.standard_normal(c)).astype(np.float32), (0.3 * rng.standard_normal(c)).astype(np.float32)
    x4 = x.reshape(p, c, 1, 1).astype(np.float64)
    y_ref, mean, invstd, _, _ = ref.bn_train_fwd(x4, gamma, beta, acc=np.float64)
    xa = x.astype(np.float64)
    mean64, var64 = xa.mean(0), xa.var(0)
    inv64 = 1 / np.sqrt(var64 + cases.EPS)
    coef = torch.from_numpy(np.stack([inv64 * gamma, beta - mean64 * inv64 * gamma, mean64, inv64], 1))              # float64 table: nothing but the formulas differs
    xt, rt, gt = torch.from_numpy(x), torch.from_numpy(res), torch.from_numpy(dy).double()
    for relu in (0, 1):
        want, terms, pre = cases.apply_want(xt, rt, coef, relu)
        full = y_ref.reshape(p, c).astype(np.float64) + res
        assert np.abs(want.numpy() - (np.maximum(full, 0) if relu else full)).max() < 1e-6          # the oracle returns fp32
        assert (terms.numpy() >= np.abs(want.numpy()) - 1e-12).all()
    assert np.abs(cases.apply_want(xt, None, coef, 0)[0].numpy() - y_ref.reshape(p, c)).max() < 1e-6
    dx_ref, dg_ref, db_ref = ref.bn_train_bwd(dy.reshape(p, c, 1, 1), x.reshape(p, c, 1, 1), mean64, inv64, gamma)
    s1, s2, a1, a2, xhat = cases.bn_sums(gt, xt, coef)
    assert np.abs(s1.numpy() - db_ref).max() < 1e-5 and np.abs(s2.numpy() - dg_ref).max() < 1e-5 and (a1 >= s1.abs() - 1e-12).all() and (a2 >= s2.abs() - 1e-12).all()
    want, terms = cases.dx_want(gt, xhat, coef, s2, s1, p, False)
    assert np.abs(want.numpy() - dx_ref.reshape(p, c)).max() < 1e-6 and (terms >= want.abs() - 1e-12).all()
    frozen = ref.bn_eval_bwd(dy.reshape(p, c, 1, 1), x.reshape(p, c, 1, 1), gamma, beta, mean64, var64, cases.EPS)[0]
    assert np.abs(cases.dx_want(gt, xhat, coef, s2, s1, p, True)[0].numpy() - frozen.reshape(p, c)).max() < 1e-6
    # the ReLU mask and its bytes
    live = cases.live_of(1, None, xt, coef, None)
    assert torch.equal(live, pre > 0) and cases.live_of(0, None, xt, coef, None) is None
    y16 = torch.from_numpy(cases.r16(rng.standard_normal((p, c))))
    assert torch.equal(cases.live_of(1, rt, xt, coef, y16), y16 > 0)
    packed = np.packbits((y16.numpy() > 0).reshape(p, c // 8, 8), axis=-1, bitorder='little').reshape(p, c // 8)
    assert np.array_equal(cases.mask_bytes(y16, c).numpy(), packed)
    # table_stats on a table that IS the sums of an x (P = TABLE_P pixels in two rows)
    p5 = cases.TABLE_P
    x5 = x[:p5].astype(np.float64)
    table = np.zeros((2, c // 8, 16), dtype=np.float32)
    for r, part in enumerate((x5[:2], x5[2:])):
        table[r, :, :8] = part.sum(0).reshape(c // 8, 8)
        table[r, :, 8:] = (part * part).sum(0).reshape(c // 8, 8)
    rm, rv = rng.standard_normal(c).astype(np.float32), (1 + rng.random(c)).astype(np.float32)
    st = cases.table_stats(dict(table=table, gamma=gamma, rm=rm, rv=rv))
    _, m5, i5, nrm, nrv = ref.bn_train_fwd(x5.reshape(p5, c, 1, 1), gamma, beta, rm, rv, cases.MOMENTUM, cases.EPS)
    assert np.abs(st['mean'] - m5).max() < 1e-5 and np.abs(st['invstd'] - i5).max() < 1e-4 * i5.max()
    assert np.abs(st['rm'] - nrm).max() < 1e-5 and np.abs(st['rv'] - nrv).max() < 1e-4 * nrv.max()


def test_pool_inputs_tie_and_weight_reference_matches_the_layouts():
    x, dy = cases.pool_inputs(cases.POOL_SHAPES[1])
    assert (x == 0).mean() > 0.4 and np.array_equal(x, x.astype(np.float16).astype(np.float32)) and np.array_equal(dy, dy.astype(np.float16).astype(np.float32))
    w = cases.weight_inputs(5, 3, 4)
    a, b = cases.weight_images_want(w, 8)
    assert a.shape == (5, 4, 8) and b.shape == (8, 4, 5) and not a[:, :, 3:].any() and not b[3:].any()
    assert np.array_equal(a[:, :, :3], w.transpose(0, 2, 1)) and np.array_equal(b[:3], w.transpose(1, 2, 0))            # [K][RS][C] and [C][RS][K], as test_hconv_fwd_dgrad_wgrad states them
    xr, dyr = cases.relu_inputs(cases.RELU_SIZES[1])
    assert np.isfinite(xr).all() and (np.signbit(xr) & (xr == 0)).any() and ((xr != 0) & (np.abs(xr) < 6.2e-5)).sum() >= 16 and np.signbit(dyr[1])
