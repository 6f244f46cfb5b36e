"""Every fast convolution family on rectangular maps and at paddings other than dil * (R - 1) / 2 (tests/geometry_table.py), each against a plain
high-precision reference of the same operation, each with proof that the fast kernel ran (launch counters, autograd node types, *_supported == 1,
or bits that differ from the fallback's).  The square tests next door cannot see an H / W exchange, a row stride taken from Ho, a parity class sized
with the wrong side or a padding assumed "same"; the bodies and bounds are theirs (imported, generalised in place to (H, W)), only the geometry is new.
tests/test_geometry_host.py pins each row's admitted / refused verdict on the CPU and shows that every reference here tells a transposition apart.

Ordered so that small batches and the fp32-fed entry points (whose fallback is bit-comparable) run first.  Needs an MI355X: run with `-m gpu`."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import geometry_table as T
import test_block_gpu as tb
import test_half_gpu as th
import test_infer_fp8_gpu as t8
import test_infer_gpu as ti
import test_infer_half_gpu as t16
import test_infer_partial_gpu as tp
import test_kernels_gpu as tk
from oracle import np_ops as ref

pytestmark = pytest.mark.gpu
X3_ON = os.environ.get('P3D_X3', '1') != '0'
needs_x3 = pytest.mark.skipif(not X3_ON, reason='P3D_X3=0 keeps every layer off the x3 kernels these cases are about')
needs_blocks = pytest.mark.skipif(not X3_ON or os.environ.get('P3D_BLOCKS', '1') == '0', reason='the block executor is switched off in this run')

BY_BATCH = sorted(T.ROWS, key=lambda g: g.n * g.c * g.h * g.w)                    # smallest first
ids = lambda g: g.name
hw_id = lambda hw: '%dx%d' % hw


def _seed(g):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(g.name)) % 100003


# ---- 1. x3 kernels fed fp32 tensors (the default path of ops.conv2d) ---------------------------------------------------------------------
@pytest.mark.parametrize('g', BY_BATCH, ids=ids)
def test_x3_fp32_fed(pkg, g):
    """forward, data gradient and weight gradient with the x3 kernels off and on, against float64, at the bounds of test_x3_kernels_match_fp32_kernels;
    the passes the launch counters report on the x3 kernels are the passes the table says (the default path asks for 96 channels on the tile side)"""
    covered = tk.x3_case(pkg, g.n, g.c, g.k, g.h, g.w, g.r, g.stride, g.pad, g.dil, with_bias=g.r == 5 or g.k == 272, seed=_seed(g))
    want = (bool(g.x3 & 1) and g.k >= 96, bool(g.x3 & 2) and g.c >= 96, bool(g.x3 & 4) and g.k >= 96 and g.c >= 96)
    assert covered == want, (covered, want)


@pytest.mark.parametrize('g', [g for g in BY_BATCH if g.r > 1 and 96 <= g.c <= 256 and g.k >= 96], ids=ids)
def test_x3_accumulate(pkg, g):
    """accumulate = 1: data and weight gradient added onto existing tensors (GradJoin, a shared .grad), bound of test_x3_accumulates_into_existing_gradients"""
    stats = tk.accumulate_case(pkg, g.n, g.c, g.k, g.h, g.w, g.r, g.stride, g.pad, g.dil)
    assert stats['x3']['dgrad'][0] + stats['fp32']['dgrad'][0] == 1 and stats['x3']['wgrad'][0] + stats['fp32']['wgrad'][0] == 1, stats
    if X3_ON:
        assert stats['x3']['dgrad'][0] == int(bool(g.x3 & 2)) and stats['x3']['wgrad'][0] == int(bool(g.x3 & 4)), stats


@pytest.mark.parametrize('n,h,w', [(1, 24, 40), (3, 40, 24), (3, 8, 48), (1, 48, 8), (1, 12, 20), (3, 20, 12)])
def test_x3_conv_cat_channel_windows(pkg, n, h, w):
    """conv_cat1x1: two input-channel windows of one weight (c_offset / c_total), against float64 at the bound of the x3 family"""
    ops = pkg.ops
    gen = torch.Generator(device='cuda').manual_seed(h + 3 * w)
    xa = torch.randn(n, 128, h, w, device='cuda', generator=gen).requires_grad_(True)
    xb = torch.randn(n, 128, h, w, device='cuda', generator=gen).requires_grad_(True)
    wt = (torch.randn(128, 256, 1, 1, device='cuda', generator=gen) / 16).requires_grad_(True)
    ops.conv_path_stats(reset=True)
    y = ops.conv_cat1x1(xa, xb, wt)
    dy = torch.randn(y.shape, device='cuda', generator=gen)
    y.backward(dy)
    ops.join_side_stream()
    torch.cuda.synchronize()
    stats = ops.conv_path_stats(reset=True)
    cat = torch.cat([xa, xb], 1).detach().double().requires_grad_(True)
    w64 = wt.detach().double().requires_grad_(True)
    want = F.conv2d(cat, w64)
    want.backward(dy.double())
    rel = lambda a, b: ((a.double() - b).abs().max() / b.abs().max()).item()
    assert rel(y.detach(), want.detach()) < 4e-6
    assert rel(torch.cat([xa.grad, xb.grad], 1), cat.grad) < 4e-6 and rel(wt.grad, w64.grad) < 4e-6
    if X3_ON:
        assert stats['x3']['fwd'][0] > 0 and not any(v[0] for v in stats['fp32'].values()), stats


MASKED_ROWS = [g for g in BY_BATCH if g.name.split('_')[0] in ('3x3', '3x3s2', '5x5p0', '3x3d2p4', '1x1p2', '3x3s2p5') and g.c <= 256 and g.n <= 3]


@pytest.mark.parametrize('g', MASKED_ROWS, ids=ids)
def test_x3_partial_conv_operands(pkg, g):
    """mask_in / mult (partial_conv.py:45-53: conv(x * mask) * mult, the mask with holes and a window without a valid pixel) against float64, at the
    bounds test_conv_sampled_oracle_at_full_size holds the masked layers to (2e-5, 2e-5, 5e-5), here over every element"""
    ops = pkg.ops
    gen = torch.Generator(device='cuda').manual_seed(_seed(g))
    x = torch.randn(g.n, g.c, g.h, g.w, device='cuda', generator=gen).requires_grad_(True)
    wt = (torch.randn(g.k, g.c, g.r, g.r, device='cuda', generator=gen) / (g.c * g.r * g.r) ** 0.5).requires_grad_(True)
    mask = (torch.rand(g.n, 1, g.h, g.w, device='cuda', generator=gen) >= 0.3).float()
    mask[0, 0, :7, :9] = 0.0
    mult, _ = ops.mask_count(mask, g.r, g.stride, g.pad, g.dil)
    ops.conv_path_stats(reset=True)
    y = ops.conv2d(x, wt, None, g.stride, g.pad, g.dil, mask_in=mask, mult=mult)
    dy = torch.randn(y.shape, device='cuda', generator=gen)
    y.backward(dy)
    ops.join_side_stream()
    torch.cuda.synchronize()
    stats = ops.conv_path_stats(reset=True)
    x64, w64 = x.detach().double().requires_grad_(True), wt.detach().double().requires_grad_(True)
    cnt = F.conv2d(mask.double(), torch.ones(1, 1, g.r, g.r, dtype=torch.float64, device='cuda'), None, g.stride, g.pad, g.dil)
    mult64 = g.r * g.r / (cnt + 1e-6) * cnt.clamp(0, 1)
    assert ((mult.double() - mult64).abs().max() / mult64.abs().max()).item() < 1e-6
    want = F.conv2d(x64 * mask.double(), w64, None, g.stride, g.pad, g.dil) * mult.double()
    want.backward(dy.double())
    for name, got, w_, tol in (('fwd', y.detach(), want.detach(), 2e-5), ('dgrad', x.grad, x64.grad, 2e-5), ('wgrad', wt.grad, w64.grad, 5e-5)):
        err = ((got.double() - w_).abs().max() / w_.abs().max()).item()
        assert err < tol, (name, err)
    if X3_ON and os.environ.get('P3D_FX_MASKED', '1') != '0':
        # (the masked instances ask for 64 channels on the tile side in forward and data gradient, 96 on both sides in the weight gradient)
        want = [bool(g.x3 & 1) and g.k >= 64, bool(g.x3 & 2) and g.c >= 64, bool(g.x3 & 4) and g.k >= 96 and g.c >= 96]
        assert [stats['x3'][nm][0] for nm in ('fwd', 'dgrad', 'wgrad')] == [int(v) for v in want], stats


# ---- 2. x3 kernels fed pre-split images (what the block executor launches) ---------------------------------------------------------------
@needs_x3
@pytest.mark.parametrize('hw', T.ASPECTS + T.SMALL, ids=hw_id)
def test_activation_image_of_a_rectangular_map(pkg, hw):
    tk.act_image_split_case(pkg, 3, 48, *hw)


@needs_x3
@pytest.mark.parametrize('g', [g for g in BY_BATCH if g.x3 & 1], ids=ids)
def test_image_fed(pkg, g):
    """p3d_fx_conv_fwd_img / _dgrad_img / _wgrad_img (+ accumulate_into) at the bounds of test_image_fed_kernels_match_the_oracle, every launch counted on the
    x3 kernels; the strided data gradient also as one launch per parity class (p3d_fx_tune(5, 1)).  A row whose data gradient the predicate refuses
    (x3 == 5) runs forward and weight gradient here; its data gradient is test_x3_fp32_fed's, on the fallback."""
    L = pkg._lib.lib()
    assert L.p3d_fx_conv_img_supported(ctypes.byref(pkg.ops._desc((g.n, g.c, g.h, g.w), (g.k, g.c, g.r, g.r), g.stride, g.pad, g.dil))) == g.x3
    res = tk.image_fed_case(pkg, g.n, g.c, g.h, g.w, g.k, g.r, g.stride, g.pad, g.dil, seed=_seed(g), dgrad=bool(g.x3 & 2))
    if g.stride == 2 and g.x3 & 2:
        L.p3d_fx_tune(5, 1)
        try:
            dx = pkg.ops.conv2d_img('dgrad', res['x'].shape, res['w'], g.stride, g.pad, g.dil, dy_img=pkg.ops.act_image(res['dy']))
            torch.cuda.synchronize()
        finally:
            L.p3d_fx_tune(5, 0)
        err = np.abs(tk.host(dx) - res['want_dx']).max() / np.abs(res['want_dx']).max()
        assert err < 2e-5, err
        assert (dx - res['dx']).abs().max() <= 4e-6 * res['dx'].abs().max()


@needs_x3
@pytest.mark.parametrize('hw', T.ASPECTS, ids=hw_id)
def test_conv_module_outside_a_block_takes_images(pkg, hw):
    """nn.Conv2d routing on a rectangular map: a multi-tap conv with bias (the regressor's class) runs as ConvImagesFn; all four results against float64"""
    gen = torch.Generator(device='cuda').manual_seed(hw[0])
    conv = pkg.nn.Conv2d(128, 272, 3, padding=1).cuda()
    x = torch.randn(3, 128, *hw, device='cuda', generator=gen).requires_grad_(True)
    assert pkg.ops_block.conv_takes_images(conv, x)
    y = conv(x)
    assert type(y.grad_fn).__name__.startswith('ConvImagesFn')
    dy = torch.randn(y.shape, device='cuda', generator=gen)
    y.backward(dy)
    pkg.ops.join_side_stream()
    torch.cuda.synchronize()
    xh, wh, bh, dyh = tk.host(x), tk.host(conv.weight), tk.host(conv.bias), tk.host(dy)
    for got, want, tol in ((y, ref.conv2d_fwd(xh, wh, bh, 1, 1, 1), 2e-5), (x.grad, ref.conv2d_dgrad(dyh, wh, x.shape, 1, 1, 1), 2e-5),
                           (conv.weight.grad, ref.conv2d_wgrad(dyh, xh, conv.weight.shape, 1, 1, 1), 5e-5), (conv.bias.grad, dyh.astype(np.float64).sum((0, 2, 3)), 2e-5)):
        assert np.abs(tk.host(got) - want).max() < tol * np.abs(want).max()


# ---- 3. the fp32 block executor ------------------------------------------------------------------------------------------------------------
# (the clean-seed rule needs a seed without any pre-ReLU activation within 2e-6 of zero: about one activation in 6 * 10^5 lies that close, so the batch of
# the 960-pixel maps is 1 and that of the 384- and 240-pixel maps 3)
BLOCK_CASES = [(blk, hw, 1 if hw[0] * hw[1] > 400 else 3) for blk in T.BLOCKS for hw in T.BLOCK_MAPS]


@needs_blocks
@pytest.mark.parametrize('blk,hw,n', BLOCK_CASES, ids=['%s_c%d_p%d_s%d_d%d_%dx%d_n%d' % (b[:5] + hw + (n,)) for b, hw, n in BLOCK_CASES])
def test_fused_block(pkg, blk, hw, n):
    """p3d_block_fwd / _bwd against the per-layer path and float64 PyTorch (output, input gradient, parameter gradients, running statistics) with the clean-seed
    rule and the bounds of test_fused_block_matches_per_layer_path_and_float64; a refused map (stride 2 at 12 x 20) runs per layer, at the same bounds"""
    kind, inplanes, planes, stride, dil, with_ds = blk
    tb.fused_block_case(pkg, kind, inplanes, planes, stride, dil, n, hw, with_ds, admitted=T.block_admitted(stride, *hw))


@needs_blocks
@pytest.mark.parametrize('hw', T.ASPECTS, ids=hw_id)
def test_block_out_mask_and_masked_block(pkg, hw):
    """out_mask bytes on / off (bit-identical) and one block of partial convolutions (stride 2, downsample)"""
    h, w = hw
    tb.test_out_mask_bytes_equal_reading_the_output(pkg, ('bottleneck', 256, 128, 2, True, (3, 256, h, w), (3, 512, h // 2, w // 2)))
    tb.test_out_mask_bytes_equal_reading_the_output(pkg, ('basic', 128, 128, 1, False, (3, 128, h, w), (3, 128, h, w)))
    tb.masked_block_case(pkg, 'bottleneck', 256, 128, 2, 1, 3, h, w, True)


# ---- 4. fp16: per-layer kernels against float64, the epilogue sum tables, the block executor bit for bit ----------------------------------
@pytest.mark.parametrize('g', [g for g in BY_BATCH if g.c <= 256], ids=ids)
def test_half_per_layer(pkg, g):
    """p3d_hconv2d_fwd / _dgrad / _wgrad on fp16-rounded operands against float64 (bounds of test_hconv_fwd_dgrad_wgrad), and the partial-sum tables of
    p3d_hconv2d_fwd_stats / _dgrad_sums (p3d_hconv2d_sum_rows rows) against fp64 sums of the rounded results (bounds of test_hconv_epilogue_sums)"""
    case = (g.name, g.n, g.c, g.h, g.w, g.k, g.r, g.stride, g.pad, g.dil)
    th.test_hconv_fwd_dgrad_wgrad(case, pkg)
    th.test_hconv_epilogue_sums(case, pkg)


@pytest.mark.parametrize('blk', [('bottleneck', 256, 64, 1, 1, False), ('bottleneck', 256, 128, 2, 1, True), ('bottleneck', 512, 256, 1, 2, True),
                                 ('basic', 64, 64, 1, 1, False), ('basic', 64, 128, 2, 1, True)], ids=lambda b: '%s_c%d_p%d_s%d_d%d' % b[:5])
@pytest.mark.parametrize('hw', T.ASPECTS, ids=hw_id)
def test_half_block(pkg, blk, hw):
    """p3d_hblock_fwd / _bwd: bit-equal to the per-layer fp16 path, exactly as test_half_block_executor_equals_the_per_layer_path asserts it"""
    kind, inplanes, planes, stride, dil, with_ds = blk
    th.half_block_case(pkg, kind, inplanes, planes, stride, dil, 3, hw[0], hw[1], with_ds)


# ---- 5. folded fp32 inference (p3d_fx_conv_fwd_infer, fp32- and image-fed, split-K, masked) --------------------------------------------------
def _folded_layer(pkg, g):
    return ti._layer(pkg, g.c, g.k, g.r, g.stride, g.dil, seed=_seed(g), pad=g.pad)


@needs_x3
@pytest.mark.parametrize('g', BY_BATCH, ids=ids)
def test_folded_fp32(pkg, g):
    """infer.FoldedConv: conv + folded BatchNorm (+ residual) (+ ReLU) against float64, _rel < 2e-5, every call counted on the x3 forward; a refused row goes
    through the same public entry and lands on the fallback, at the same bound"""
    conv, bn = _folded_layer(pkg, g)
    fc = pkg.infer.FoldedConv(conv, bn)
    gen = torch.Generator(device='cuda').manual_seed(_seed(g))
    x = torch.randn(g.n, g.c, g.h, g.w, device='cuda', generator=gen)
    res = torch.randn(g.n, g.k, *T.out_hw(g), device='cuda', generator=gen)
    pkg.ops.conv_path_stats(reset=True)
    for r, relu in ((None, False), (None, True), (res, True), (res, False)):
        assert ti._rel(fc(x, r, relu), ti._conv64(x, conv, bn, r, relu)) < 2e-5, (r is not None, relu)
    stats = pkg.ops.conv_path_stats(reset=True)
    if g.x3 & 1:
        assert stats['x3']['fwd'][0] == 4 and stats['fp32']['fwd'][0] == 0, stats
    else:
        assert stats['x3']['fwd'][0] == 0 and stats['fp32']['fwd'][0] == 4, stats


@needs_x3
@pytest.mark.parametrize('g', [g for g in BY_BATCH if g.x3 & 1], ids=ids)
def test_folded_fp32_image_fed_and_masked(pkg, g):
    """the same entry fed a pre-split activation image, and p3d_fx_conv_fwd_infer_masked with holes and a window without a valid pixel (exactly b' + res there)"""
    L, ops = pkg._lib.lib(), pkg.ops
    conv, bn = _folded_layer(pkg, g)
    fc = pkg.infer.FoldedConv(conv, bn)
    c = fc.convs[0]
    gen = torch.Generator(device='cuda').manual_seed(_seed(g) + 1)
    x = torch.randn(g.n, g.c, g.h, g.w, device='cuda', generator=gen)
    res = torch.randn(g.n, g.k, *T.out_hw(g), device='cuda', generator=gen)
    d = c.desc(x)
    assert L.p3d_fx_conv_fwd_infer_supported(ctypes.byref(d), 1) == 1 and L.p3d_fx_conv_fwd_infer_masked_supported(ctypes.byref(d)) == 1
    y = torch.full((g.n, g.k) + T.out_hw(g), float('nan'), device='cuda')
    ws = torch.empty(max(L.p3d_fx_conv_fwd_infer_workspace_bytes(ctypes.byref(d)), 16), dtype=torch.uint8, device='cuda')
    ops.conv_path_stats(reset=True)
    pkg._lib.check(L.p3d_fx_conv_fwd_infer(ctypes.byref(d), None, ops._p(ops.act_image(x)), fc._at(c.img_off), c.img_bytes, fc._at(c.bias_off), ops._p(res), 1, ops._p(y),
                                           ops._p(ws), ws.numel(), ops._stream()), 'p3d_fx_conv_fwd_infer')
    assert ti._rel(y, ti._conv64(x, conv, bn, res, True)) < 2e-5
    veil = (torch.rand(g.n, 1, g.h, g.w, device='cuda', generator=gen) > 0.3).float()
    veil[0, 0, :7, :9] = 0.0
    mult, _ = ops.mask_count(veil, g.r, g.stride, g.pad, g.dil)
    y = torch.full_like(y, float('nan'))
    pkg._lib.check(L.p3d_fx_conv_fwd_infer_masked(ctypes.byref(d), ops._p(x), fc._at(c.img_off), c.img_bytes, fc._at(c.bias_off), ops._p(veil), ops._p(mult), ops._p(res), 0,
                                                  ops._p(y), ops._p(ws), ws.numel(), ops._stream()), 'p3d_fx_conv_fwd_infer_masked')
    w64, b64 = ti._fold64(conv, bn)
    want = F.conv2d(x.double() * veil.double(), w64, None, g.stride, g.pad, g.dil) * mult.double() + b64[None, :, None, None] + res.double()
    assert ti._rel(y, want) < 2e-5
    stats = ops.conv_path_stats(reset=True)
    assert stats['x3']['fwd'][0] == 2 and stats['fp32']['fwd'][0] == 0, stats


# ---- 6. the folded fp16 gather kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('g', BY_BATCH, ids=ids)
def test_folded_fp16(pkg, g):
    """p3d_hconv2d_fwd_infer (+ residual, ReLU, mask_in, mult) against float64 on the fp16 operands, _err < 2e-3; t16._infer asserts *_supported == 1"""
    conv, bn = _folded_layer(pkg, g)
    img = t16._image16(pkg, ti._torch_fold(conv, bn), g.c)
    bias = ti._fold64(conv, bn)[1].float()
    gen = torch.Generator(device='cuda').manual_seed(_seed(g))
    x16 = pkg.ops_half.to_half_nhwc(torch.randn(g.n, g.c, g.h, g.w, device='cuda', generator=gen), g.c)
    res16 = pkg.ops_half.to_half_nhwc(torch.randn(g.n, g.k, *T.out_hw(g), device='cuda', generator=gen), g.k)
    w64 = img.double().permute(0, 3, 1, 2)
    base = F.conv2d(x16.double(), w64, bias.double(), g.stride, g.pad, g.dil)
    for res, relu in ((None, False), (res16, True)):
        got = t16._infer(pkg, x16, img, bias, g.stride, g.pad, g.dil, res, relu)
        want = base if res is None else base + res.double()
        assert t16._err(got, torch.relu(want) if relu else want) < 2e-3, (res is not None, relu)
    mask = (torch.rand(g.n, 1, g.h, g.w, device='cuda', generator=gen) > 0.4).float()
    mask[0, 0, :7, :9] = 0
    mult, _ = pkg.ops.mask_count(mask, g.r, g.stride, g.pad, g.dil)
    got = t16._infer(pkg, x16, img, bias, g.stride, g.pad, g.dil, res16, True, mask_in=mask, mult=mult)
    want = torch.relu(F.conv2d(x16.double() * mask.double(), w64, None, g.stride, g.pad, g.dil) * mult.double() + bias.double()[None, :, None, None] + res16.double())
    assert t16._err(got, want) < 2e-3


# ---- 7. the MXFP8 gather kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('g', BY_BATCH, ids=ids)
def test_folded_fp8(pkg, g):
    """p3d_f8conv2d_fwd_infer against the float64 conv of the dequantized operands, t8._expect / t8._check unchanged (the bound is per element and carries
    the reduction length); t8._run asserts *_supported == 1"""
    conv, q, sc, img, bias, x16 = t8._conv_case(pkg, g.c, (g.h, g.w), g.k, g.r, g.stride, g.dil, g.n, seed=_seed(g), pad=g.pad)
    res16 = pkg.ops_half.to_half_nhwc(torch.randn(g.n, g.k, *T.out_hw(g), device='cuda'), g.k)
    for res, relu in ((None, False), (res16, True)):
        got = t8._run(pkg, x16, img, bias, g.k, g.r, g.stride, g.pad, g.dil, res, relu)
        t8._check(got, *t8._expect(x16, q, sc, bias, g.stride, g.pad, g.dil, res, relu))
    mask = (torch.rand(g.n, 1, g.h, g.w, device='cuda') > 0.4).float()
    mask[0, 0, :7, :9] = 0
    mult, _ = pkg.ops.mask_count(mask, g.r, g.stride, g.pad, g.dil)
    got = t8._run(pkg, x16, img, bias, g.k, g.r, g.stride, g.pad, g.dil, res16, True, mask_in=mask, mult=mult)
    t8._check(got, *t8._expect(x16, q, sc, bias, g.stride, g.pad, g.dil, res16, True, mask_in=mask, mult=mult))


@pytest.mark.parametrize('k', [1, 3])
@pytest.mark.parametrize('hw', T.ASPECTS[:2], ids=hw_id)
def test_fp8_identity_conv_bit_exact(pkg, hw, k):
    """test_activation_quantizer_bit_exact's identity conv on a rectangular map: every output is one product, so a transposed load or store shows bit for bit"""
    t8.quantizer_identity_case(pkg, 128, k, *hw)


# ---- 8. whole networks on a rectangular batch ------------------------------------------------------------------------------------------------
NETS = [('depthnet', 'resnet18', ()), ('resnet', 'resnet18', ('-joint_space',)), ('fusionnet', 'resnet18', ()), ('partial_depthnet', 'resnet18', ('-depth_only',))]
HALF_NETS = NETS[:1] + [('resnet', 'resnet18', ('-extra_channel',))] + NETS[2:] + [('partial_fusionnet', 'resnet18', ())]
net_id = lambda v: v if isinstance(v, str) else ''.join(v)
_SQUARE_ROUTES = {}                                       # (family, model, extra) -> conv path counters of the folded forward at 128 x 128


@needs_x3
@pytest.mark.parametrize('hw', T.NET_MAPS, ids=hw_id)
@pytest.mark.parametrize('family,model,extra', NETS + [('depthnet', 'resnet50', ())], ids=net_id)
def test_whole_network_fp32(pkg, family, model, extra, hw):
    """infer.fold(net)(x) and the unfolded eval forward against the float64 forward, bounds of test_infer_gpu.test_whole_network; the folded forward launches
    exactly the kernels it launches on a square batch (no layer falls back for the rectangle), none of them on the fp32-MFMA path for the plain families"""
    key = (family, model, extra)
    if key not in _SQUARE_ROUTES:
        _SQUARE_ROUTES[key] = ti.whole_network_case(pkg, family, model, extra, 128, 128)
    stats = ti.whole_network_case(pkg, family, model, extra, hw[0], hw[1])
    launches = lambda s: {path: {k: v[0] for k, v in s[path].items()} for path in s}
    assert launches(stats) == launches(_SQUARE_ROUTES[key]) and stats['x3']['fwd'][0] > 0, (stats, _SQUARE_ROUTES[key])
    if family in ('depthnet', 'fusionnet'):
        assert stats['fp32']['fwd'][0] == 0, stats


@needs_x3
@pytest.mark.parametrize('hw', T.NET_MAPS, ids=hw_id)
@pytest.mark.parametrize('family', ['partial_depthnet', 'partial_fusionnet'])
def test_whole_partial_network_fp32(pkg, family, hw):
    """the partial families through infer.fold (masked stem, masked convs) and unfolded, against float64: test_whole_partial_network_folded on a rectangular batch;
    no forward of the folded network on the fp32-MFMA path"""
    pkg.ops.conv_path_stats(reset=True)
    tp.whole_partial_network_case(pkg, family, 'resnet18', 128, 2, hw=hw)
    net = tp._net(pkg, family, 'resnet18', side=128, seed=2)
    fn = pkg.infer.fold(net)
    pkg.ops.conv_path_stats(reset=True)
    fn(*tp._inputs(family, 2, hw, seed=1))
    stats = pkg.ops.conv_path_stats(reset=True)
    assert stats['x3']['fwd'][0] > 0 and stats['fp32']['fwd'][0] == 0, stats


@pytest.mark.parametrize('hw', T.NET_MAPS, ids=hw_id)
@pytest.mark.parametrize('family,model,extra', HALF_NETS, ids=net_id)
def test_whole_network_fp16(pkg, family, model, extra, hw):
    """infer.fold_half and the unfolded fp16 model against the float64 forward, 2e-2 as in test_infer_half_gpu.test_whole_network"""
    t16.whole_network_case(pkg, family, model, extra, 128, 2, hw=hw)


@pytest.mark.parametrize('hw', T.NET_MAPS, ids=hw_id)
@pytest.mark.parametrize('family,model,extra', HALF_NETS, ids=net_id)
def test_whole_network_fp8(pkg, monkeypatch, family, model, extra, hw):
    """infer.fold_fp8 layer by layer: each fp8 layer against the emulated conv of the input it received, each fp16 layer bit-equal to fold_half's"""
    seen = t8.layer_by_layer_case(pkg, monkeypatch, family, model, extra, 128, 2, hw=hw)
    assert seen['fp8'] >= 10


def _train64(net, x, dz):
    """float64 PyTorch of depthnet's trunk in training mode (stem -> layer1..4 -> regressor; depthnet.py:138-156) on copies of the parameters; returns
    (z, {parameter name: gradient})"""
    p = {k: v.detach().double().requires_grad_(True) for k, v in net.named_parameters()}
    bn = lambda name, v: F.batch_norm(v, None, None, p[name + '.weight'], p[name + '.bias'], True, 0.1, 1e-5)
    conv = lambda name, m, v: F.conv2d(v, p[name + '.weight'], p.get(name + '.bias'), m.stride, m.padding, m.dilation)
    h = F.max_pool2d(torch.relu(bn('bn1', conv('conv1', net.conv1, x.double()))), 3, 2, 1)
    for lname in ('layer1', 'layer2', 'layer3', 'layer4'):
        for i, blk in enumerate(getattr(net, lname)):
            pre = '%s.%d.' % (lname, i)
            res = h if blk.downsample is None else bn(pre + 'downsample.1', conv(pre + 'downsample.0', blk.downsample[0], h))
            out, last = h, len(blk._chain) - 1
            for j, (cn, bnn) in enumerate(blk._chain):
                out = bn(pre + bnn, conv(pre + cn, getattr(blk, cn), out))
                out = torch.relu(out) if j < last else torch.relu(out + res)
            h = out
    z = conv('regressor', net.regressor, h)
    z.backward(dz.double())
    return z.detach(), {k: v.grad for k, v in p.items()}


@needs_blocks
@pytest.mark.parametrize('hw', T.NET_MAPS, ids=hw_id)
def test_training_trunk_on_a_rectangular_batch(pkg, monkeypatch, hw):
    """One training-mode forward + backward of the depthnet trunk, fused blocks on, against float64 PyTorch of the same layers.  Norm-wise, since ReLUs
    switch element by element: the output at 1e-4 (the whole-network forward bound of test_infer_gpu), every parameter gradient at 8e-3 (part (b) of
    test_resnet50_block_geometries_at_batch_64).  Every residual block runs on the executor, the stem on the restated kernels, the regressor on images."""
    torch.manual_seed(3)
    net = pkg.depthnet.resnet18(ti._args(pkg, 'resnet18'), False).cuda().train()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.3)
    assert not net.skip_relu and not net.early_dist
    gen = torch.Generator(device='cuda').manual_seed(hw[0])
    x = torch.randn(3, 3, *hw, device='cuda', generator=gen)
    calls = []
    real = pkg.ops_block.residual_block
    monkeypatch.setattr(pkg.ops_block, 'residual_block', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    assert pkg.ops_block.stem_takes_x3(net.conv1, x)
    net.zero_grad(set_to_none=True)
    z, feat = net(x)
    assert len(calls) == sum(len(getattr(net, name)) for name in ('layer1', 'layer2', 'layer3', 'layer4'))
    assert type(z.grad_fn).__name__.startswith('ConvImagesFn')
    dz = torch.randn(z.shape, device='cuda', generator=gen)
    z.backward(dz)
    pkg.ops.join_side_stream()
    torch.cuda.synchronize()
    z64, grads = _train64(net, x, dz)
    assert z.shape == z64.shape and tuple(z.shape[2:]) == (hw[0] // 16, hw[1] // 16)
    assert tb.rel2(z, z64) < 1e-4, tb.rel2(z, z64)
    for name, prm in net.named_parameters():
        assert tb.rel2(prm.grad, grads[name]) < 8e-3, (name, tb.rel2(prm.grad, grads[name]))


# ---- the head ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', [(12, 20), (20, 12), (16, 24), (24, 16)], ids=hw_id)
def test_softargmax3d_on_a_rectangular_heat_map(pkg, hw):
    """to_heatmap + decode at production depth and joint counts (16 x 17) against the oracle, forward and backward, bounds of test_head_matches_reference_golden"""
    h, w = hw
    rng = np.random.default_rng(h)
    z = (rng.standard_normal((3, 16 * 17, h, w)) * 3).astype(np.float32)
    dc = rng.standard_normal((3, 17, 3)).astype(np.float32)
    zt = tk.dev(z).requires_grad_(True)
    coords = pkg.utils.decode(pkg.utils.to_heatmap(zt, 16, 17, h, w), 1000.0)
    coords.backward(tk.dev(dc))
    assert tk.relerr(tk.host(coords), ref.softargmax3d_fwd(z, 16, 17, h, w, 1000.0)) < 2e-6
    assert tk.relerr(tk.host(zt.grad), ref.softargmax3d_bwd(dc, z, 16, 17, h, w, 1000.0)) < 5e-5
