"""Folding the stems and the partial layers at odd crop sides (infer.fold(..., any_size=True, odd_sides=True)): p3d_fx_conv_fwd_infer_masked_any and the
stem on the zero-extended space-to-depth image with its pitched tail (p3d_stem_image_any, p3d_stem_fwd on the padded sides, p3d_stem_tail_infer_any).

Every partial-conv class on the odd maps against a float64 partial conv + BatchNorm with empty windows exactly relu(b' + res), split-K, no write outside
y / the workspace / the stem's buffers, the stems dense and masked, aligned shapes through the new entries, whole networks with the launch counters and
without a BatchNorm pass, refresh(), and the Trainer at -side_in 257.  Needs an MI355X: run with `-m gpu`."""
import ctypes
import json

import numpy as np
import pytest
import torch

import test_infer_gpu as tg
import test_infer_partial_gpu as tp
from conftest import golden_path
from fenced import Fence, fenced_like
from test_infer_partial_gpu import _bn64, _count_bn, _inputs, _mask, _partial64, _pconv_layer, _pstem64, _rel

pytestmark = pytest.mark.gpu

ODD = {32: 33, 16: 17}
CLASSES = [(c, ODD[hw], k, r, s) for c, hw, k, r, s, _ in tp.CLASSES] + [(64, 65, 64, 1, 1), (64, 65, 64, 3, 1)]      # cin, side, cout, filter, stride
EPILOGUES = ((False, False), (False, True), (True, True), (True, False))       # (residual, ReLU)


def _out(h, r, stride):
    return (h + 2 * ((r - 1) // 2) - r) // stride + 1


def _veil(n, h, w, seed, block=6):
    """tp._mask on an h x w map: ~30 % holes plus a block of zeros in image 0 that empties whole windows"""
    if h == w:
        return _mask(n, h, seed, block)
    g = torch.Generator(device='cuda').manual_seed(seed)
    m = (torch.rand(n, 1, h, w, device='cuda', generator=g) >= 0.3).float()
    m[0, :, 2:2 + block, 3:3 + block] = 0
    return m


def _four_epilogues(pkg, conv, bn, x, veil, seed=0):
    """FoldedConv(any_size, odd_sides) with the four (residual, ReLU) combinations against _partial64 + _bn64 at tp's bound; mask_out bit-equal; empty windows
    exactly relu(b' + res); four x3 forwards and none on the fp32-MFMA path"""
    fc = pkg.infer.FoldedConv(conv, bn, any_size=True, odd_sides=True)
    assert fc.conv.foldable and fc.conv.partial
    n, cout = x.shape[0], conv.out_channels
    r, s = conv.kernel_size[0], conv.stride[0]
    ho, wo = _out(x.shape[2], r, s), _out(x.shape[3], r, s)
    res = torch.randn(n, cout, ho, wo, device='cuda', generator=torch.Generator(device='cuda').manual_seed(seed))
    c64, mask_out64 = _partial64(conv, x, veil)
    empty = mask_out64.expand(n, cout, ho, wo) == 0
    assert int(empty[0, 0].sum()) > 0                           # the zero block leaves windows with no valid input
    b = fc.bias(fc.conv)[None, :, None, None]
    pkg.ops.conv_path_stats(reset=True)
    for with_res, relu in EPILOGUES:
        rr = res if with_res else None
        got, mask_out = fc(x, rr, relu, veil=veil)
        want = _bn64(bn, c64, None if rr is None else rr.double(), relu)
        err = _rel(got, want)
        print('oddsides pconv', tuple(x.shape), tuple(conv.weight.shape), 's%d' % s, 'res' if with_res else '-', 'relu' if relu else '-', 'rel %.3e' % err)
        assert got.shape == want.shape
        assert err < 1e-4, (with_res, relu, err)
        assert torch.equal(mask_out.double(), mask_out64)
        exact = b.expand_as(got) if rr is None else b + rr
        exact = torch.relu(exact) if relu else exact
        assert torch.equal(got[empty], exact[empty]), (with_res, relu)
    stats = pkg.ops.conv_path_stats(reset=True)
    assert stats['x3']['fwd'][0] == 4 and stats['fp32']['fwd'][0] == 0, stats


# ---- 1. the partial classes on odd maps -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 3])
@pytest.mark.parametrize('cls', CLASSES, ids=lambda c: 'c%d_%d_k%d_%dx%d_s%d' % (c[0], c[1], c[2], c[3], c[3], c[4]))
def test_partial_class_against_float64(pkg, cls, n):
    """n = 1, 2, 3 at 65^2 / 33^2 / 17^2: 128-pixel tiles end mid-row and, from n = 2 on, span two images"""
    cin, hw, cout, k, stride = cls
    conv, bn = _pconv_layer(pkg, cin, cout, k, stride, seed=cin + cout + k + stride)
    L = pkg._lib.lib()
    d = pkg.ops._desc((n, cin, hw, hw), tuple(conv.weight.shape), stride, (k - 1) // 2, 1)
    assert L.p3d_fx_conv_fwd_infer_masked_supported(ctypes.byref(d)) == 0 and L.p3d_fx_conv_fwd_infer_masked_any_supported(ctypes.byref(d)) == 1
    x = torch.randn(n, cin, hw, hw, device='cuda')
    _four_epilogues(pkg, conv, bn, x, _veil(n, hw, hw, seed=cin + k), seed=n)


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('hw', [(17, 17), (18, 18), (19, 19), (17, 33), (33, 17)], ids=lambda hw: '%dx%d' % hw)
def test_widths_and_rectangles(pkg, hw, stride):
    """widths = 1, 2, 3 mod 4 and the two rectangles, 3x3 128 -> 128, n = 3"""
    conv, bn = _pconv_layer(pkg, 128, 128, 3, stride, seed=hw[0] * hw[1] + stride)
    x = torch.randn(3, 128, hw[0], hw[1], device='cuda')
    _four_epilogues(pkg, conv, bn, x, _veil(3, hw[0], hw[1], seed=hw[1]), seed=hw[0])


def test_keyword_off_keeps_the_module_path(pkg, monkeypatch):
    """without odd_sides a partial conv on an odd map runs as the module + the eval-mode BatchNorm pass, as before"""
    conv, bn = _pconv_layer(pkg, 128, 128, 3, 1, seed=1)
    x = torch.randn(2, 128, 17, 17, device='cuda')
    veil = _veil(2, 17, 17, seed=2)
    fc = pkg.infer.FoldedConv(conv, bn, any_size=True)
    calls = _count_bn(pkg, monkeypatch)
    got, _ = fc(x, None, True, veil=veil)
    assert calls.count('p3d_bn_eval_fwd') + calls.count('batch_norm_act') > 0
    assert _rel(got, _bn64(bn, _partial64(conv, x, veil)[0], None, True)) < 1e-4


# ---- 2. split-K ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('slabs', [2, 3])
def test_split_k(pkg, slabs):
    """forced slab counts: the ragged <0, 4, 0> slabs, then the scalar sum with the factor before b', the residual and the ReLU"""
    conv, bn = _pconv_layer(pkg, 128, 128, 3, 1, seed=slabs)
    x = torch.randn(2, 128, 17, 19, device='cuda')
    L = pkg._lib.lib()
    d = pkg.ops._desc(tuple(x.shape), tuple(conv.weight.shape), 1, 1, 1)
    unsplit = L.p3d_fx_conv_fwd_infer_masked_any_workspace_bytes(ctypes.byref(d))      # (the built-in plan: 72 K steps on 6 tiles split in two by themselves)
    fb = ctypes.c_size_t()
    L.p3d_fx_weight_image_bytes(128, 128, 9, ctypes.byref(fb), None)
    L.p3d_fx_tune(1, slabs)
    try:
        need = L.p3d_fx_conv_fwd_infer_masked_any_workspace_bytes(ctypes.byref(d))
        assert need >= fb.value + slabs * 2 * 128 * 17 * 19 * 4         # the weight image's room, then the slabs
        assert need - unsplit == (slabs - 2) * 2 * 128 * 17 * 19 * 4    # and it grows by whole slabs (2 x 128 x 17 x 19 elements: already a multiple of 4)
        _four_epilogues(pkg, conv, bn, x, _veil(2, 17, 19, seed=slabs), seed=slabs)
    finally:
        L.p3d_fx_tune(1, 0)
    assert L.p3d_fx_conv_fwd_infer_masked_any_workspace_bytes(ctypes.byref(d)) == unsplit


# ---- 3. no stray writes ----------------------------------------------------------------------------------------------------------------------
def _call_masked_any(pkg, fc, d, x, veil, mult, res, relu, y, ws, ws_bytes):
    L, ops, c = pkg._lib.lib(), pkg.ops, fc.convs[0]
    pkg._lib.check(L.p3d_fx_conv_fwd_infer_masked_any(ctypes.byref(d), ops._p(x), fc._at(c.img_off), c.img_bytes, fc._at(c.bias_off), ops._p(veil), ops._p(mult),
                                                      ops._p(res), int(relu), ops._p(y), ops._p(ws), ws_bytes, ops._stream()), 'p3d_fx_conv_fwd_infer_masked_any')


@pytest.mark.parametrize('shape,slabs', [((64, 64, 65, 65, 1, 3), 0), ((128, 128, 17, 19, 3, 2), 3)], ids=['1x1_65x65_n3', '3x3_17x19_n2_3slabs'])
def test_no_write_outside_y_or_the_workspace(pkg, shape, slabs):
    """y and the workspace at exactly their size inside fences (tests/fenced.py), the bands two images of y wide; y comes poisoned and must be written whole"""
    cin, cout, h, w, r, n = shape
    conv, bn = _pconv_layer(pkg, cin, cout, r, 1, seed=h + w)
    fc = pkg.infer.FoldedConv(conv, bn, any_size=True, odd_sides=True)
    x = torch.randn(n, cin, h, w, device='cuda')
    res = torch.randn(n, cout, h, w, device='cuda')
    veil = _veil(n, h, w, seed=r)
    mult, _ = pkg.ops.mask_count(veil, r, 1, (r - 1) // 2, 1)
    L = pkg._lib.lib()
    d = pkg.ops._desc(tuple(x.shape), tuple(conv.weight.shape), 1, (r - 1) // 2, 1)
    L.p3d_fx_tune(1, slabs)
    try:
        need = L.p3d_fx_conv_fwd_infer_masked_any_workspace_bytes(ctypes.byref(d))
        y, yfence = fenced_like((n, cout, h, w), torch.float32, 2 * cout * h * w)
        wfence = Fence(need, 8 * cout * h * w, 'cuda')
        _call_masked_any(pkg, fc, d, x, veil, mult, res, True, y, wfence.view, need)
        torch.cuda.synchronize()
    finally:
        L.p3d_fx_tune(1, 0)
    yfence.check('y')
    wfence.check('workspace')
    assert not bool(torch.isnan(y).any())                       # no poison left: every element of y was written
    assert _rel(y, _bn64(bn, _partial64(conv, x, veil)[0], res.double(), True)) < 1e-4


@pytest.mark.parametrize('masked', [False, True], ids=['dense', 'masked'])
def test_no_write_outside_the_stem_buffers(pkg, masked):
    """p3d_stem_image_any + p3d_stem_fwd + p3d_stem_tail_infer_any at 33^2, n = 3: the image, c and y each fenced and poisoned.  Every image byte is written, the
    pad pixels (rows >= 17 or columns >= 17 of the 20 x 20 half-resolution grid hold input rows / columns >= 34; pixel 16 holds row 32 and the zero row 33) are
    exact zeros in all three planes, and y holds no poison."""
    n, h, w, k = 3, 33, 33, 64
    net, _ = tg._net(pkg, 'depthnet', 'resnet18', '-depth_only', seed=3)
    fn = pkg.infer.fold(net, any_size=True, odd_sides=True)
    st = fn.stems['conv1']
    (depth,) = _inputs('partial_depthnet', n, 33, seed=3)
    x = torch.randn(n, 1, h, w, device='cuda') if not masked else depth
    veil = pkg.ops.nonzero_mask(depth) if masked else None
    mult = pkg.ops.mask_count(veil, 7, 2, 3, 1)[0] if masked else None
    L, ops = pkg._lib.lib(), pkg.ops
    hp, wp = ctypes.c_int32(), ctypes.c_int32()
    assert L.p3d_stem_any_padded(h, w, ctypes.byref(hp), ctypes.byref(wp)) == 1 and (hp.value, wp.value) == (40, 40)
    nimg = L.p3d_stem_image_bytes(n, 40, 40)
    assert nimg == 3 * n * 20 * 20 * 32
    ifence = Fence(nimg, 2 * 20 * 20 * 32, 'cuda')
    c, cfence = fenced_like((n, k, 20, 20), torch.float32, 2 * k * 400)
    y, yfence = fenced_like((n, k, 9, 9), torch.float32, 2 * k * 81)
    s = ops._stream()
    pkg._lib.check(L.p3d_stem_image_any(ops._p(x), ops._p(veil), ops._p(ifence.view), n, 1, h, w, s), 'p3d_stem_image_any')
    pkg._lib.check(L.p3d_stem_fwd(ops._p(ifence.view), fn._at(st.img_off), ops._p(c), n, 1, 40, 40, k, s), 'p3d_stem_fwd')
    pkg._lib.check(L.p3d_stem_tail_infer_any(ops._p(c), fn._at(st.bias_off), ops._p(mult), ops._p(y), n, k, h, w, s), 'p3d_stem_tail_infer_any')
    torch.cuda.synchronize()
    for f, what in ((ifence, 'image'), (cfence, 'c'), (yfence, 'y')):
        f.check(what)
    planes = ifence.view.view(torch.int16).view(3, n, 20, 20, 16)                # [plane][n][i][j][16 bf16]
    # with Cin = 1 channels 4 .. 15 of every pixel are zero; poison (0xFFFF) anywhere means an unwritten byte
    assert not bool((planes == -1).any())
    assert bool((planes[:, :, 17:] == 0).all()) and bool((planes[:, :, :, 17:] == 0).all())
    assert bool((planes[:, :, 16, :, 2:4] == 0).all()) and bool((planes[:, :, :, 16, 1] == 0).all()) and bool((planes[:, :, :, 16, 3] == 0).all())      # row 33 / column 33
    assert bool((planes[:, :, :, :, 4:] == 0).all())
    assert not bool(torch.isnan(c).any()) and not bool(torch.isnan(y).any())
    if masked:                                                  # (conv1 of a depthnet is a dense Conv2d: the float64 partial stem is built from its weight)
        want, _ = _pstem64(st.conv, st.bn, x, (depth != 0).double())
    else:
        want = tg._stem64(st.conv, st.bn, x)
    assert _rel(y, want) < 1e-4


# ---- 4. the stems ------------------------------------------------------------------------------------------------------------------------------
SIDES = [(33, 33), (129, 129), (130, 130), (33, 49)]


@pytest.mark.parametrize('cin', [1, 3])
@pytest.mark.parametrize('hw', SIDES, ids=lambda hw: '%dx%d' % hw)
def test_dense_stem_against_float64(pkg, hw, cin):
    net, _ = tg._net(pkg, 'depthnet', 'resnet18', *(('-depth_only',) if cin == 1 else ()), seed=4)
    st_on = pkg.infer.fold(net, any_size=True, odd_sides=True)
    st = st_on.stems['conv1']
    assert st.foldable and not st.masked and st.cin == cin
    x = torch.randn(3, cin, hw[0], hw[1], device='cuda')
    assert pkg._lib.lib().p3d_stem_supported(3, cin, hw[0], hw[1], st.k) == 0
    pkg.ops.conv_path_stats(reset=True)
    got = st_on._stem(st, x)
    stats = pkg.ops.conv_path_stats(reset=True)
    want = tg._stem64(st.conv, st.bn, x)
    err = _rel(got, want)
    print('oddsides dense stem', hw, cin, 'rel %.3e' % err, stats)
    assert got.shape == want.shape and err < 1e-4
    assert stats['x3']['fwd'][0] == 1 and stats['fp32']['fwd'][0] == 0, stats
    pkg.infer.fold(net, any_size=True)._stem(st, x)            # keyword off: _trunk.stem, one fp32-MFMA launch, as before
    off = pkg.ops.conv_path_stats(reset=True)
    assert off['x3']['fwd'][0] == 0 and off['fp32']['fwd'][0] == 1, off


@pytest.mark.parametrize('cin', [1, 3])
@pytest.mark.parametrize('hw', SIDES, ids=lambda hw: '%dx%d' % hw)
def test_masked_stem_against_float64(pkg, hw, cin):
    """the PartialConv stem: holes of ~30 % and one wider than the 7x7 window (tp._inputs; its corner hole is a side / 8 wide, so at 33 a 16 x 16 one is cut
    as well); the pooled mask bit-equal"""
    net = tp._net(pkg, 'partial_depthnet', 'resnet18', seed=4)
    if cin == 3:                                                # (no reference network has a three-channel partial stem: the same module with a wider conv)
        torch.manual_seed(5)
        net.conv1 = pkg.partial_conv.PartialConv(3, 64, 7, stride=2, padding=3, bias=False).cuda().eval()
    fn = pkg.infer.fold(net, any_size=True, odd_sides=True)
    st = fn.stems['conv1']
    assert st.masked and st.foldable and st.cin == cin
    (depth,) = _inputs('partial_depthnet', 3, hw, seed=4)
    depth[0, :, :16, :16] = 0
    x = depth if cin == 1 else torch.randn(3, 3, hw[0], hw[1], device='cuda') * (depth != 0)
    veil = pkg.ops.nonzero_mask(depth)
    assert pkg._lib.lib().p3d_stem_masked_supported(3, cin, hw[0], hw[1], st.k) == 0
    pkg.ops.conv_path_stats(reset=True)
    h, v = fn._stem_masked(st, x, veil)
    stats = pkg.ops.conv_path_stats(reset=True)
    want, v64 = _pstem64(st.conv, st.bn, x, (depth != 0).double())
    assert int((v64[0] == 0).sum()) > 0                         # whole pooled pixels without a valid input
    err = _rel(h, want)
    print('oddsides masked stem', hw, cin, 'rel %.3e' % err, stats)
    assert h.shape == want.shape and err < 1e-4
    assert torch.equal(v.double(), v64)
    assert stats['x3']['fwd'][0] == 1 and stats['fp32']['fwd'][0] == 0, stats


# ---- 5. aligned shapes through the new entries ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cls', [(64, 32, 64, 3, 1), (128, 32, 128, 3, 2), (256, 32, 64, 1, 1)], ids=lambda c: 'c%d_%d_k%d_%dx%d_s%d' % (c[0], c[1], c[2], c[3], c[3], c[4]))
def test_aligned_shapes_through_the_masked_any_entry(pkg, cls):
    """32^2 shapes, which p3d_fx_conv_fwd_infer_masked takes too, straight into p3d_fx_conv_fwd_infer_masked_any: every group of four pixels is one aligned line"""
    cin, hw, cout, k, stride = cls
    conv, bn = _pconv_layer(pkg, cin, cout, k, stride, seed=cin + k)
    fc = pkg.infer.FoldedConv(conv, bn, any_size=True, odd_sides=True)
    x = torch.randn(2, cin, hw, hw, device='cuda')
    veil = _mask(2, hw, seed=k, block=6)
    ho = _out(hw, k, stride)
    res = torch.randn(2, cout, ho, ho, device='cuda')
    mult, _ = pkg.ops.mask_count(veil, k, stride, (k - 1) // 2, 1)
    L = pkg._lib.lib()
    d = pkg.ops._desc(tuple(x.shape), tuple(conv.weight.shape), stride, (k - 1) // 2, 1)
    assert L.p3d_fx_conv_fwd_infer_masked_supported(ctypes.byref(d)) == 1 and L.p3d_fx_conv_fwd_infer_masked_any_supported(ctypes.byref(d)) == 1
    need = max(L.p3d_fx_conv_fwd_infer_masked_any_workspace_bytes(ctypes.byref(d)), 16)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    c64, mask_out64 = _partial64(conv, x, veil)
    empty = mask_out64.expand(2, cout, ho, ho) == 0
    b = fc.bias(fc.conv)[None, :, None, None]
    pkg.ops.conv_path_stats(reset=True)
    for with_res, relu in EPILOGUES:
        y = torch.full((2, cout, ho, ho), float('nan'), device='cuda')
        rr = res if with_res else None
        _call_masked_any(pkg, fc, d, x, veil, mult, rr, relu, y, ws, need)
        assert _rel(y, _bn64(bn, c64, None if rr is None else rr.double(), relu)) < 1e-4, (with_res, relu)
        exact = b.expand_as(y) if rr is None else b + rr
        exact = torch.relu(exact) if relu else exact
        assert torch.equal(y[empty], exact[empty]), (with_res, relu)
    stats = pkg.ops.conv_path_stats(reset=True)
    assert stats['x3']['fwd'][0] == 4 and stats['fp32']['fwd'][0] == 0, stats


@pytest.mark.parametrize('masked', [False, True], ids=['dense', 'masked'])
def test_aligned_stem_through_the_any_entries(pkg, masked):
    """a stem at 128^2, which p3d_stem_supported takes: padded to itself, every fetch and store on an aligned line"""
    net = tp._net(pkg, 'partial_depthnet', 'resnet18', seed=6)
    fn = pkg.infer.fold(net, any_size=True, odd_sides=True)
    st = fn.stems['conv1']
    assert pkg._lib.lib().p3d_stem_supported(3, 1, 128, 128, st.k) == 1
    (depth,) = _inputs('partial_depthnet', 3, 128, seed=6)
    if masked:
        y, mask_out = fn._stem_any(st, depth, pkg.ops.nonzero_mask(depth))
        want, v64 = _pstem64(st.conv, st.bn, depth, (depth != 0).double())
        assert torch.equal(fn.model.maxpool(mask_out).double(), v64)
    else:
        y, _ = fn._stem_any(st, depth)
        want = tg._stem64(st.conv, st.bn, depth)
    assert y.shape == want.shape and _rel(y, want) < 1e-4


# ---- 6. whole networks -------------------------------------------------------------------------------------------------------------------------
NETS = [('partial_depthnet', 'resnet18', (129, 129)), ('partial_depthnet', 'resnet18', (257, 257)), ('partial_depthnet', 'resnet50', (129, 129)),
        ('partial_depthnet', 'resnet50', (257, 257)), ('partial_fusionnet', 'resnet18', (129, 129)), ('depthnet', 'resnet18', (129, 193)),
        ('fusionnet', 'resnet18', (129, 129)), ('resnet', 'resnet18', (129, 129))]


def _network(pkg, family, model, hw, seed, n=2):
    """(net, inputs at hw, inputs at 128^2, float64 forward)"""
    if family.startswith('partial_'):
        net = tp._net(pkg, family, model, seed=seed)
        return net, _inputs(family, n, hw, seed=1), _inputs(family, n, 128, seed=1), lambda *t: tp._forward64(net, family, *t)
    net, _ = tg._net(pkg, family, model, *(('-joint_space',) if family == 'resnet' else ()), side=128, seed=seed)
    g = torch.Generator(device='cuda').manual_seed(0)
    make = lambda h, w: (torch.randn(n, 3, h, w, device='cuda', generator=g),) + ((torch.rand(n, 1, h, w, device='cuda', generator=g),) if family == 'fusionnet' else ())
    return net, make(*hw), make(128, 128), lambda *t: tg._forward64(net, family, *t)


@pytest.mark.parametrize('family,model,hw', NETS, ids=lambda v: v if isinstance(v, str) else '%dx%d' % v)
def test_whole_network(pkg, monkeypatch, family, model, hw):
    """fold(net, any_size=True, odd_sides=True) against the float64 forward and the unfolded eval forward at 1e-4.  Counters: no fp32-MFMA forward (one for the
    legacy network's 17-channel mat_regressor), as many x3 forwards as the same network's fold launches at 128^2 (21 for the ResNet-18 partial_depthnet: the
    stem, 8 partial convs, 11 dense convs and the head), no BatchNorm pass; with the keyword off the counts of fold(net, any_size=True) as they were (12 there)."""
    net, xin, x128, forward64 = _network(pkg, family, model, hw, seed=2)
    fn = pkg.infer.fold(net, any_size=True, odd_sides=True)
    calls = _count_bn(pkg, monkeypatch)
    pkg.ops.conv_path_stats(reset=True)
    got = fn(*xin)
    torch.cuda.synchronize()
    stats = pkg.ops.conv_path_stats(reset=True)
    assert calls == [], calls
    pkg.infer.fold(net)(*x128)
    aligned = pkg.ops.conv_path_stats(reset=True)
    plain = pkg.infer.fold(net, any_size=True)(*xin)
    off = pkg.ops.conv_path_stats(reset=True)
    with torch.no_grad():
        old = net(*xin)
        want = forward64(*xin)
    got, plain, old, want = [t if isinstance(t, tuple) else (t,) for t in (got, plain, old, want)]
    assert len(got) == len(old) == len(want) == len(plain)
    for gt, pt, ot, wt in zip(got, plain, old, want):
        assert gt.shape == ot.shape == wt.shape == pt.shape
        print('oddsides net', family, model, hw, 'folded %.3e unfolded %.3e folded-vs-unfolded %.3e' % (_rel(gt, wt), _rel(ot, wt), _rel(gt, ot)))
        assert _rel(gt, wt) < 1e-4 and _rel(ot, wt) < 1e-4
        assert _rel(gt, ot) < 1e-4
        assert _rel(pt, wt) < 1e-4
    print('oddsides net counters', family, model, hw, stats, aligned, off)
    left = 1 if family == 'resnet' else 0
    assert aligned['fp32']['fwd'][0] == left, aligned
    assert stats['fp32']['fwd'][0] == left, stats
    assert stats['x3']['fwd'][0] == aligned['x3']['fwd'][0], (stats, aligned)
    if (family, model) == ('partial_depthnet', 'resnet18'):
        assert stats['x3']['fwd'][0] == 21 and off['x3']['fwd'][0] == 12, (stats, off)
    stems = 2 if family.endswith('fusionnet') else 1
    assert off['x3']['fwd'][0] < stats['x3']['fwd'][0] and off['fp32']['fwd'][0] >= left + (stems if not family.startswith('partial_') else 0), off
    if not family.startswith('partial_'):                       # dense families: the keyword moves exactly the stems
        assert off['x3']['fwd'][0] == stats['x3']['fwd'][0] - stems and off['fp32']['fwd'][0] == left + stems, off


# ---- 7. refresh ------------------------------------------------------------------------------------------------------------------------------
def test_refresh_after_optimizer_step(pkg):
    net = tp._net(pkg, 'partial_depthnet', 'resnet18', seed=8)
    (x,) = _inputs('partial_depthnet', 2, 129, seed=8)
    fn = pkg.infer.fold(net, any_size=True, odd_sides=True)
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    net.train()
    z, feat = net(x)
    (z.square().mean() + feat.square().mean()).backward()
    opt.step()
    net.eval()
    with torch.no_grad():
        want = net(x)[0]
    assert float(net.layer1[0].bn1.running_mean.abs().max()) > 0
    assert _rel(fn(x)[0], want) > 1e-3                          # stale: the stem's and the partial layers' weights and running statistics moved
    fn.refresh()
    assert _rel(fn(x)[0], want) < 1e-4


# ---- 8. Trainer --------------------------------------------------------------------------------------------------------------------------------
def test_trainer_test_partial_at_257_matches_the_unfolded_run(pkg, tmp_path, monkeypatch):
    """Trainer.test of a partial_depthnet at the default -side_in 257 with and without P3D_FOLDED_EVAL=1: the same record at the tolerances of
    test_trainer_test_at_257_matches_the_unfolded_run; the folded run has no fp32-MFMA forward launch (the Trainer folds with odd_sides)"""
    g = np.load(golden_path('eval.npz'))
    meta = tmp_path / 'metadata.json'
    meta.write_text(json.dumps(dict(loader=dict(h36m='depth_datasets'), no_depth=dict(h36m=False),
                                    thresholds=dict(h36m=json.loads(str(g['thresh']))), root=dict(h36m=str(tmp_path)))))
    batches = []
    for it in range(2):
        c, d, tc, tv = pkg.synth.make_batch(2, side=257, rank=7, step=it, invalid_frac=0.2)
        rot = np.linalg.qr(np.random.Generator(np.random.PCG64(it)).standard_normal((2, 3, 3)))[0].astype(np.float32)
        batches.append(tuple(torch.from_numpy(a) for a in (c, d, tc, tv, rot)))
    records, counters = [], []
    for on in ('0', '1'):
        monkeypatch.setenv('P3D_FOLDED_EVAL', on)
        args = pkg.opts.parse(['-model', 'resnet18', '-suffix', 't', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1',
                               '-num_joints', '17', '-side_in', '257', '-metadata', str(meta), '-depth_only', '-partial_conv'])
        model, _ = pkg.depth_main.create_model(args)
        assert type(model).__module__.endswith('partial_depthnet')
        det = pkg.synth.det_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 0)
        model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in det.items()})
        trainer = pkg.depth_train.Trainer(args, model.cuda(), pkg.utils.get_info())
        trainer.verbose = False
        pkg.ops.conv_path_stats(reset=True)
        records.append(trainer.test(1, batches))
        counters.append(pkg.ops.conv_path_stats(reset=True))
        assert (trainer.__dict__.get('_folded_model') is not None) == (on == '1')
    want, record = records
    print('oddsides trainer', want, record, counters)
    assert counters[1]['x3']['fwd'][0] > 0 and counters[1]['fp32']['fwd'][0] == 0, counters
    assert set(record) == set(want)
    assert record['test_loss'] == pytest.approx(want['test_loss'], rel=1e-3)
    assert record['cam_mean'] == pytest.approx(want['cam_mean'], rel=1e-3)
    for k in ('score_pck', 'score_auc', 'solid', 'close', 'depth', 'jitter', 'switch', 'fail'):
        assert record[k] == pytest.approx(want[k], abs=2e-3), k
