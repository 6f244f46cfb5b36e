"""Block-scaled FP8 (MXFP8) folded inference (infer.fold_fp8, fold kind 3 of p3d_fx_fold_bn_images, p3d_f8conv2d_fwd_infer).

Fold images and scales bit-equal to the emulation (mxfp8_emul.py) of the torch fold; the kernel's activation quantizer bit-equal to the emulation
(identity convs, whose every output is one product, over subnormal, saturating, tie and zero blocks); the conv classes of ResNet-18 / -50 at 256^2 and
257^2 against a float64 conv of the dequantized operands (bound: the fp32 accumulation bound, plus MFMA_ERR, plus one fp16 ulp); whole networks layer by layer (each fp8 layer against
the emulated conv of the exact input it received, each fp16 layer bit-equal to fold_half's); coverage (every conv but the stems and heads on the fp8
entry, no BatchNorm pass); refresh(); the Trainer switch P3D_FOLDED_EVAL_FP8."""
import ctypes
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden_path
from mxfp8_emul import dequantize, quantize, scale_of
from test_infer_gpu import CLASSES, _layer, _net, _stats_, _torch_fold
from test_infer_half_gpu import _find, _inputs

pytestmark = pytest.mark.gpu


def _emul_image(w):
    """the MXFP8 image of an fp32 weight [K][C][R][S] by the rule, C padded with zeros to Cpad: (elements uint8 [K][R][S][Cpad], scales [K][R][S][Cpad/32])"""
    k, c, r, s = w.shape
    cpad = (c + 31) // 32 * 32
    wp = torch.zeros((k, r, s, cpad), dtype=torch.float32, device=w.device)
    wp[..., :c] = w.permute(0, 2, 3, 1)
    q, byte, _ = quantize(wp)
    return q.view(torch.uint8), byte


def _same_fp8(a, b):
    """bit-equal e4m3 bytes, the sign of a zero free"""
    return torch.equal(torch.where((a & 0x7f) == 0, torch.zeros_like(a), a), torch.where((b & 0x7f) == 0, torch.zeros_like(b), b))


def _fold_direct(pkg, w, gamma=None, beta=None, mean=None, var=None, eps=1e-5, cpad=None):
    """one kind-3 job through p3d_fx_fold_bn_images: (elements [K][R][S][Cpad], scales, b')"""
    k, c, r, s = w.shape
    cpad = cpad or (c + 31) // 32 * 32
    n = k * r * s * cpad
    out = torch.zeros(n + n // 32, dtype=torch.uint8, device='cuda')
    bias = torch.empty(k, dtype=torch.float32, device='cuda')
    j = pkg._lib.FoldJob()
    j.w = w.data_ptr()
    if gamma is not None:
        j.gamma, j.beta, j.mean, j.var, j.eps = gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), var.data_ptr(), eps
    j.out, j.bias_out = out.data_ptr(), bias.data_ptr()
    j.K, j.C, j.RS, j.c_offset, j.c_total, j.kind, j.reserved = k, c, r * s, 0, c, 3, cpad
    table = torch.frombuffer(bytearray((pkg._lib.FoldJob * 1)(j)), dtype=torch.uint8).cuda()
    pkg._lib.check(pkg._lib.lib().p3d_fx_fold_bn_images(pkg.ops._p(table), 1, 64, pkg.ops._stream()), 'p3d_fx_fold_bn_images')
    torch.cuda.synchronize()
    return out[:n].view(k, r, s, cpad), out[n:].view(k, r, s, cpad // 32), bias


# ---- 1. fold ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(64, 64, 1), (128, 64, 3), (2048, 512, 1), (512, 2048, 1), (256, 40, 3), (272, 512, 3)],
                         ids=lambda s: 'k%d_c%d_%dx%d' % (s[0], s[1], s[2], s[2]))
def test_fold_kind3_bit_exact(pkg, shape):
    k, c, r = shape
    torch.manual_seed(k + c + r)
    conv, bn = _layer(pkg, c, k, r, 1, 1, seed=k + c)
    w = conv.weight.detach().contiguous()
    q, sc, b = _fold_direct(pkg, w, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
    want_q, want_s = _emul_image(_torch_fold(conv, bn))
    assert torch.equal(sc, want_s)
    assert _same_fp8(q, want_q)
    assert torch.allclose(b, (bn.bias - bn.running_mean * (bn.weight / torch.sqrt(bn.running_var + bn.eps))).detach(), rtol=1e-6, atol=1e-6)


def test_fold_kind3_saturation_zero_and_subnormal_blocks(pkg):
    """no BatchNorm (w' = w): blocks whose amax lies in the top octave, all-zero blocks, e4m3 subnormals, tiny weights (scale byte clamped at 0)"""
    torch.manual_seed(3)
    k, c = 64, 96
    w = torch.randn(k, c, 3, 3, device='cuda')
    w[0, :32, 1, 1] = 0                                              # a zero block
    w[1, :, 0, 0] = 0
    w[1, 5, 0, 0] = 1.96875                                          # / X = 504 -> 448
    w[1, 6, 0, 0] = -1.8125
    w[2, 32:64, 2, 2] = torch.linspace(-2.0 ** -20, 2.0 ** -20, 32, device='cuda')       # e4m3 subnormals after scaling
    w[2, 40, 2, 2] = 2.0 ** -10
    w[3, 64:, 0, 1] = 2.0 ** -130 * torch.arange(32, device='cuda')  # amax < 2^-119: the scale byte clamps at 0
    w[4, :32, 1, 0] = 1.75 * 2.0 ** torch.arange(-20, 12, device='cuda').float()
    w = w.contiguous()
    q, sc, _ = _fold_direct(pkg, w)
    want_q, want_s = _emul_image(w)
    assert torch.equal(sc, want_s)
    assert _same_fp8(q, want_q)
    assert int(sc[0, 1, 1, 0]) == 0 and int(sc[3, 0, 1, 2]) == 0
    assert int(want_q[1, 0, 0, 5]) == 0x7e and int(want_q[1, 0, 0, 6]) == 0xfe


def test_fold_fp8_images_in_the_net(pkg):
    net, _ = _net(pkg, 'depthnet', 'resnet50', side=256)
    f8 = pkg.infer.fold_fp8(net)
    for conv, bn in ((net.layer1[0].conv2, net.layer1[0].bn2), (net.layer4[2].conv3, net.layer4[2].bn3), (net.layer3[0].downsample[0], net.layer3[0].downsample[1])):
        c = _find(f8, conv)
        assert isinstance(c, pkg.infer._F8Conv)
        q, sc = f8.image(c)
        want_q, want_s = _emul_image(_torch_fold(conv, bn))
        assert torch.equal(sc, want_s) and _same_fp8(q, want_q)


# ---- 2. conv against float64 on the dequantized operands -------------------------------------------------------------------------------
def _run(pkg, x16, img, bias, k, r, stride, pad, dil, res=None, relu=False, mask_in=None, mult=None):
    L = pkg._lib.lib()
    n, c, h, w = x16.shape
    d = pkg.ops._desc((n, c, h, w), (k, c, r, r), stride, pad, dil)
    assert L.p3d_f8conv2d_fwd_infer_supported(ctypes.byref(d)) == 1, L.p3d_last_error()
    y = torch.empty((n, k, d.Ho, d.Wo), dtype=torch.float16, device='cuda', memory_format=torch.channels_last)
    p = pkg.ops._p
    pkg._lib.check(L.p3d_f8conv2d_fwd_infer(ctypes.byref(d), p(x16), p(img), p(bias), p(mask_in), p(mult), p(res), int(relu), p(y), pkg.ops._stream()),
                   'p3d_f8conv2d_fwd_infer')
    return y


# v_mfma_scale_f32_32x32x64_f8f6f4 does not sum its 64 products at fp32 precision.  Observed, not documented: over 200 x 1024 results of the bare
# instruction on random e4m3 operands (every finite code, unit scales) the largest error was 2^-11.8 of the result's sum |a b| (profiles/eval_folded_fp8.md).
# The bound carries 2^-11 of sum |a b| for it, 1.7x that observed maximum.  The 1x1 classes with 64 input channels are reductions of one instruction each,
# so they hold the kernel to it directly.
MFMA_ERR = 2.0 ** -11


def _ulp16(v):
    a = v.abs().clamp_min(2.0 ** -14)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - 10)


def _expect(x16, q, sc, bias, stride, pad, dil, res=None, relu=False, mask_in=None, mult=None):
    """float64 conv of the dequantized operands (+ b', res, ReLU) and the error bound: n u sum|a b| (fp32 accumulation, the epilogue's three operations
    included) + MFMA_ERR sum|a b| + one fp16 ulp"""
    xin = x16.float() if mask_in is None else x16.float() * mask_in
    xq, _, xX = quantize(xin.permute(0, 2, 3, 1))
    xd = dequantize(xq, xX).permute(0, 3, 1, 2)
    wd = dequantize(q, scale_of(sc)).permute(0, 3, 1, 2)
    raw = F.conv2d(xd, wd, None, stride, pad, dil)
    mag = F.conv2d(xd.abs(), wd.abs(), None, stride, pad, dil)
    if mult is not None:
        raw, mag = raw * mult.double(), mag * mult.double()
    want = raw + bias.double()[None, :, None, None]
    mag = mag + bias.double().abs()[None, :, None, None]
    if res is not None:
        want, mag = want + res.double(), mag + res.double().abs()
    if relu:
        want = torch.relu(want)
    nterms = wd.shape[1] * wd.shape[2] * wd.shape[3] + 3
    return want, (nterms * 2.0 ** -24 + MFMA_ERR) * mag + _ulp16(want)


def _check(got, want, tol):
    assert torch.isfinite(got).all(), 'non-finite output'
    err = (got.double() - want).abs()
    bad = ~(err <= tol)                                              # (a NaN anywhere counts as a failure)
    assert not bad.any(), 'max excess %.3e at %s (got %s want %s)' % (float((err - tol).max()), tuple(bad.nonzero()[0].tolist()),
                                                                      float(got.double()[bad][0]), float(want[bad][0]))


def _conv_case(pkg, cin, hw, cout, k, stride, dil, n, seed, x=None, w=None, pad=None):
    """hw: the side of a square map, or (H, W); pad: None for dil * (k - 1) / 2"""
    torch.manual_seed(seed)
    conv, bn = _layer(pkg, cin, cout, k, stride, dil, seed=seed, pad=pad)
    wf = _torch_fold(conv, bn) if w is None else w
    q, sc = _emul_image(wf)
    img = torch.cat([q.reshape(-1), sc.reshape(-1)])
    bias = (bn.bias - bn.running_mean * (bn.weight / torch.sqrt(bn.running_var + bn.eps))).detach().float()
    if x is None:
        x = torch.randn(n, cin, *((hw, hw) if isinstance(hw, int) else hw), device='cuda')
    x16 = pkg.ops_half.to_half_nhwc(x, cin)
    return conv, q, sc, img, bias, x16


SIDES = {64: 65, 32: 33, 16: 17}


@pytest.mark.parametrize('odd', [False, True], ids=['256', '257'])
@pytest.mark.parametrize('cls', CLASSES, ids=lambda c: 'c%d_%d_k%d_%dx%d_s%d_d%d' % (c[0], c[1], c[2], c[3], c[3], c[4], c[5]))
def test_conv_class_against_float64(pkg, cls, odd):
    cin, hw, cout, k, stride, dil = cls
    hw = SIDES[hw] if odd else hw
    n = 64 if cout >= 1024 or cin >= 1024 else 8
    conv, q, sc, img, bias, x16 = _conv_case(pkg, cin, hw, cout, k, stride, dil, n, seed=cin + cout + k)
    pad = conv.padding[0]
    ho = (hw + 2 * pad - dil * (k - 1) - 1) // stride + 1
    res16 = pkg.ops_half.to_half_nhwc(torch.randn(n, cout, ho, ho, device='cuda'), cout)
    for res, relu in ((None, False), (res16, True)):
        got = _run(pkg, x16, img, bias, cout, k, stride, pad, dil, res, relu)
        _check(got, *_expect(x16, q, sc, bias, stride, pad, dil, res, relu))


@pytest.mark.parametrize('case', [(512, 16, 272, 3, 1, 1), (256, 17, 272, 1, 1, 1), (64, 33, 64, 3, 2, 1), (128, 16, 256, 3, 1, 2), (96, 20, 136, 3, 2, 2)],
                         ids=['k272_3x3', 'k272_1x1', '3x3_s2', '3x3_d2', 'c96_k136_s2_d2'])
def test_conv_shapes_residual_relu(pkg, case):
    cin, hw, cout, k, stride, dil = case
    conv, q, sc, img, bias, x16 = _conv_case(pkg, cin, hw, cout, k, stride, dil, 4, seed=cout + k)
    pad = conv.padding[0]
    ho = (hw + 2 * pad - dil * (k - 1) - 1) // stride + 1
    res16 = pkg.ops_half.to_half_nhwc(torch.randn(4, cout, ho, ho, device='cuda'), cout)
    for res, relu in ((None, False), (None, True), (res16, False), (res16, True)):
        got = _run(pkg, x16, img, bias, cout, k, stride, pad, dil, res, relu)
        _check(got, *_expect(x16, q, sc, bias, stride, pad, dil, res, relu))


@pytest.mark.parametrize('k,stride', [(3, 1), (1, 2), (3, 2)])
def test_conv_mask_in_and_mult(pkg, k, stride):
    cin, hw, cout, n = 64, 33, 128, 4
    conv, q, sc, img, bias, x16 = _conv_case(pkg, cin, hw, cout, k, stride, 1, n, seed=7 + k)
    pad = conv.padding[0]
    mask = (torch.rand(n, 1, hw, hw, device='cuda') > 0.4).float()
    mask[0, 0, :9, :9] = 0
    mult, _ = pkg.ops.mask_count(mask, k, stride, pad, 1)
    ho = mult.shape[2]
    res16 = pkg.ops_half.to_half_nhwc(torch.randn(n, cout, ho, ho, device='cuda'), cout)
    for res, relu in ((None, True), (res16, True), (res16, False)):
        got = _run(pkg, x16, img, bias, cout, k, stride, pad, 1, res, relu, mask_in=mask, mult=mult)
        _check(got, *_expect(x16, q, sc, bias, stride, pad, 1, res, relu, mask_in=mask, mult=mult))


def test_conv_fp16_subnormals_and_saturating_blocks(pkg):
    cin, hw, cout, n = 128, 16, 128, 4
    torch.manual_seed(11)
    x = torch.randn(n, cin, hw, hw, device='cuda')
    x[:, :32] *= 2.0 ** -20                                          # fp16 subnormal blocks (every block exponent from -24 up is in the data)
    x[0, 32:64, 3, 3] = 2.0 ** -24 * torch.arange(32, device='cuda')
    x[1, 64:96] = 1.75 * torch.sign(torch.randn(32, hw, hw, device='cuda'))      # blocks that reach 448 X ...
    x[1, 64, :, :] = 1.96875                                                     # ... and beyond it (clamped)
    x[2, 96:128] = 0                                                 # zero blocks
    x[3, 96:128, 5, 5] = 60000.0                                     # near the fp16 maximum
    conv, q, sc, img, bias, x16 = _conv_case(pkg, cin, hw, cout, 3, 1, 1, n, seed=5, x=x)
    got = _run(pkg, x16, img, bias, cout, 3, 1, 1, 1, None, False)
    _check(got, *_expect(x16, q, sc, bias, 1, 1, 1))


# ---- 2b. the activation quantizer, bit for bit ---------------------------------------------------------------------------------------------
def _fp16_blocks(n, c, h, w, seed):
    """fp32 tensor [n, c, h, w] of fp16 values whose 32-channel blocks (per pixel) cycle through six kinds: normal values of a random block exponent,
    fp16 subnormals, saturating blocks (amax in [1.75, 2) 2^e, so v / X in [448, 512)), exact ties between neighbouring e4m3 values after scaling,
    zero blocks (signed zeros included) and blocks spanning 20 octaves (e4m3 subnormals and underflow to zero)"""
    g = torch.Generator().manual_seed(seed)
    nb = c // 32
    v = torch.empty(n, h, w, nb, 32, dtype=torch.float64)
    e4 = torch.arange(0, 0x7f, dtype=torch.uint8).view(torch.float8_e4m3fn).double()      # the non-negative finite e4m3 values, ascending
    kinds = torch.arange(n * h * w * nb).view(n, h, w, nb) % 6
    for idx in torch.cartesian_prod(*[torch.arange(d) for d in (n, h, w, nb)]).tolist():
        kind = int(kinds[tuple(idx)])
        e = int(torch.randint(-14, 14, (1,), generator=g))
        if kind == 0:
            b = torch.randn(32, generator=g, dtype=torch.float64) * 2.0 ** e
        elif kind == 1:
            s = int(torch.randint(0, 11, (1,), generator=g))
            b = torch.randint(-(2 ** s), 2 ** s + 1, (32,), generator=g).double() * 2.0 ** -24
        elif kind == 2:
            b = (torch.rand(32, generator=g, dtype=torch.float64) * 4 - 2) * 2.0 ** e
            b[:8] = torch.sign(torch.randn(8, generator=g, dtype=torch.float64)) * (1.75 + torch.rand(8, generator=g, dtype=torch.float64) * 0.25) * 2.0 ** e
        elif kind == 3:
            e = int(torch.randint(-5, 12, (1,), generator=g))
            i = torch.randint(0, len(e4) - 1, (32,), generator=g)
            b = (e4[i] + e4[i + 1]) / 2 * 2.0 ** (e - 8) * torch.sign(torch.randn(32, generator=g, dtype=torch.float64))
            b[0] = 2.0 ** e                                          # pins the block exponent
        elif kind == 4:
            b = torch.zeros(32, dtype=torch.float64)
            b[::3] = -0.0
        else:
            b = torch.randn(32, generator=g, dtype=torch.float64) * 2.0 ** (e - torch.randint(0, 21, (32,), generator=g).double())
        v[tuple(idx)] = b
    v = v.clamp(-65504, 65504).half().float()                        # fp16 values (a tie that fp16 cannot hold is rounded, and stays a valid case)
    return v.view(n, h, w, c).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize('c,k,side', [(128, 1, 16), (96, 1, 17), (128, 3, 17)], ids=['c128_1x1', 'c96_1x1_odd', 'c128_3x3_odd'])
def test_activation_quantizer_bit_exact(pkg, c, k, side):
    quantizer_identity_case(pkg, c, k, side, side)


def quantizer_identity_case(pkg, c, k, h, w_):
    """An identity conv (w[o][i] = [o == i], the centre tap of a 3x3) with b' = 0 and no residual: every output is ONE product, q(x) X * 1, exact in the
    MFMA however it sums, then rounded to fp16 once.  So the result must equal fp16(dequantize(quantize(x))) bit for bit -- the kernel's quantizer
    against the rule, with the weight side exact (a block holding a single 1)."""
    x = _fp16_blocks(2, c, h, w_, seed=c + k).cuda()
    w = torch.zeros(c, c, k, k, device='cuda')
    w[:, :, k // 2, k // 2] = torch.eye(c, device='cuda')
    q, sc = _emul_image(w)
    img = torch.cat([q.reshape(-1), sc.reshape(-1)])
    x16 = pkg.ops_half.to_half_nhwc(x, c)
    got = _run(pkg, x16, img, torch.zeros(c, device='cuda'), c, k, 1, k // 2, 1)
    xq, _, xX = quantize(x16.float().permute(0, 2, 3, 1))
    want = dequantize(xq, xX).float().half().permute(0, 3, 1, 2)
    assert torch.isfinite(got).all()
    same = got.float() == want.float()                               # (the sign of a zero is free; a NaN is never equal)
    assert same.all(), '%d of %d differ, first at %s: got %r want %r (input %r)' % (
        int((~same).sum()), same.numel(), tuple((~same).nonzero()[0].tolist()), float(got[~same][0]), float(want[~same][0]), float(x16[~same][0]))
    xb = xq.view(torch.uint8) & 0x7f
    _, xbytes, _ = quantize(x16.float().permute(0, 2, 3, 1))
    assert (xb == 0x7e).sum() > 1000 and ((xb > 0) & (xb < 8)).sum() > 1000 and (xbytes == 0).sum() > 100      # 448s, e4m3 subnormals, zero blocks


# ---- 3. whole networks, layer by layer -------------------------------------------------------------------------------------------------
NETS = [('depthnet', 'resnet18', (), 128, 2), ('resnet', 'resnet18', ('-extra_channel',), 128, 2), ('fusionnet', 'resnet18', (), 128, 2),
        ('partial_depthnet', 'resnet18', ('-depth_only',), 128, 2), ('partial_fusionnet', 'resnet18', (), 128, 2),
        ('depthnet', 'resnet50', (), 256, 64), ('fusionnet', 'resnet50', (), 256, 64)]


@pytest.mark.parametrize('family,model,extra,side,n', NETS, ids=lambda v: v if isinstance(v, str) else ''.join(v) if isinstance(v, tuple) else str(v))
def test_whole_network_layer_by_layer(pkg, monkeypatch, family, model, extra, side, n):
    layer_by_layer_case(pkg, monkeypatch, family, model, extra, side, n)


def layer_by_layer_case(pkg, monkeypatch, family, model, extra, side, n, hw=None):
    """hw: (H, W) of the batch where it is not side x side"""
    net, args = _net(pkg, family, model, *extra, side=side, seed=len(extra))
    x, y = _inputs(family, args, n, hw or side)
    f8 = pkg.infer.fold_fp8(net)
    hf = pkg.infer.fold_half(net)
    cls = pkg.infer.Fp8FoldedNet
    orig = cls._conv_bn
    seen = {'fp8': 0, 'fp16': 0}

    def spy(self, c, xin, res=None, relu=False, mask_in=None, mult=None):
        out = orig(self, c, xin, res, relu, mask_in, mult)
        if isinstance(c, pkg.infer._F8Conv):
            q, sc = self.image(c)
            want, tol = _expect(xin, q, sc, self.bias(c), c.stride, c.pad, c.dil, res, relu, mask_in, mult)
            _check(out, want, tol)
            seen['fp8'] += 1
        else:
            ref = pkg.infer.HalfFoldedNet._conv_bn(hf, _find(hf, c.conv), xin, res, relu, mask_in, mult)
            assert torch.equal(out, ref), c.conv
            seen['fp16'] += 1
        return out

    monkeypatch.setattr(cls, '_conv_bn', spy)
    got = f8(x) if y is None else f8(x, y)
    got = got if isinstance(got, tuple) else (got,)
    assert all(t.dtype == torch.float32 and torch.isfinite(t).all() for t in got)
    assert seen['fp8'] > 0 and seen['fp16'] >= 2
    return seen


# ---- 4. coverage: every conv but the stems and heads on the fp8 entry, no BatchNorm pass ----------------------------------------------------
@pytest.mark.parametrize('family,extra', [('depthnet', ()), ('resnet', ('-extra_channel',)), ('fusionnet', ()), ('partial_depthnet', ('-depth_only',)),
                                          ('partial_fusionnet', ())], ids=lambda v: v if isinstance(v, str) else ''.join(v))
def test_fp8_coverage_and_no_batchnorm_pass(pkg, monkeypatch, family, extra):
    net, args = _net(pkg, family, 'resnet18', *extra, side=128)
    x, y = _inputs(family, args, 2, 128)
    f8 = pkg.infer.fold_fp8(net)
    stems = [net.conv1] + ([net.conv2] if family in ('fusionnet', 'partial_fusionnet') else [])
    heads = [m for m in (getattr(net, h, None) for h in ('regressor', 'cam_regressor', 'mat_regressor')) if m is not None]
    n_convs = sum(1 for m in net.modules() if isinstance(m, torch.nn.Conv2d))
    calls = []
    L = pkg._lib.lib()
    for name in ('p3d_f8conv2d_fwd_infer', 'p3d_hconv2d_fwd_infer', 'p3d_hbn_eval_fwd'):
        fn = getattr(L, name)
        monkeypatch.setattr(L, name, (lambda fn, name: lambda *a: (calls.append(name), fn(*a))[1])(fn, name))
    bn_act = pkg.ops_half.batch_norm_act
    monkeypatch.setattr(pkg.ops_half, 'batch_norm_act', lambda *a, **k: (calls.append('batch_norm_act'), bn_act(*a, **k))[1])
    f8(x) if y is None else f8(x, y)
    assert calls.count('p3d_f8conv2d_fwd_infer') == n_convs - len(stems) - len(heads)
    assert calls.count('p3d_hconv2d_fwd_infer') == len(stems) + len(heads)
    assert 'batch_norm_act' not in calls and 'p3d_hbn_eval_fwd' not in calls
    assert all(not isinstance(_find(f8, m), pkg.infer._F8Conv) for m in stems + heads)


# ---- 5. refresh --------------------------------------------------------------------------------------------------------------------------
def test_refresh_after_optimizer_step(pkg):
    net, _ = _net(pkg, 'depthnet', 'resnet18', side=128)
    x = torch.randn(2, 3, 128, 128, device='cuda')
    f8 = pkg.infer.fold_fp8(net)
    stale = f8(x)[0]
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    net.train()
    z, feat = net(x)
    (z.square().mean() + feat.square().mean()).backward()
    opt.step()
    net.eval()
    fresh = pkg.infer.fold_fp8(net)
    want = fresh(x)[0]
    assert not torch.equal(stale, want)
    f8.refresh()
    assert torch.equal(f8.buffer, fresh.buffer)
    a, b = f8(x), f8(x)
    assert torch.equal(a[0], want) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 6. Trainer -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'half_acc'])
def test_trainer_fp8_folded_test(pkg, tmp_path, monkeypatch, half):
    g = np.load(golden_path('eval.npz'))
    meta = tmp_path / 'metadata.json'
    meta.write_text(json.dumps(dict(loader=dict(h36m='depth_datasets'), no_depth=dict(h36m=False),
                                    thresholds=dict(h36m=json.loads(str(g['thresh']))), root=dict(h36m=str(tmp_path)))))
    args = pkg.opts.parse(['-model', 'resnet18', '-suffix', 't', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1',
                           '-num_joints', '17', '-side_in', '256', '-metadata', str(meta)] + (['-half_acc'] if half else []))
    model, _ = pkg.depth_main.create_model(args)
    det = pkg.synth.det_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 0)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in det.items()})
    trainer = pkg.depth_train.Trainer(args, model.cuda(), pkg.utils.get_info())
    trainer.verbose = False
    batches = []
    for it in range(2):
        c, d, tc, tv = pkg.synth.make_batch(2, side=256, rank=7, step=it, invalid_frac=0.2)
        rot = np.linalg.qr(np.random.Generator(np.random.PCG64(it)).standard_normal((2, 3, 3)))[0].astype(np.float32)
        batches.append(tuple(torch.from_numpy(a) for a in (c, d, tc, tv, rot)))
    monkeypatch.setenv('P3D_FOLDED_EVAL_FP8', '0')
    plain = trainer.test(1, batches)
    monkeypatch.setenv('P3D_FOLDED_EVAL_FP8', '1')
    runs = []
    real = pkg.infer.Fp8FoldedNet.__call__
    monkeypatch.setattr(pkg.infer.Fp8FoldedNet, '__call__', lambda self, *a: (runs.append(1), real(self, *a))[1])
    rec = trainer.test(1, batches)
    assert len(runs) == len(batches) and isinstance(trainer.__dict__.get('_folded_fp8_model'), pkg.infer.Fp8FoldedNet) and trainer._eval_net is None
    assert set(rec) == set(plain)
    for k, v in rec.items():
        if isinstance(v, float):
            assert np.isfinite(v), k


@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'half_acc'])
def test_distill_step_with_fp8_teacher(pkg, monkeypatch, half):
    monkeypatch.setenv('P3D_FOLDED_EVAL_FP8', '1')
    args = pkg.opts.parse(['-model', 'resnet18', '-suffix', 't', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1',
                           '-num_joints', '17', '-side_in', '128', '-do_teach', '-do_fusion'] + (['-half_acc'] if half else []))
    student = pkg.depthnet.resnet18(args, False)
    teacher = pkg.fusionnet.resnet18(args, False)
    for m, seed in ((student, 0), (teacher, 1)):
        det = pkg.synth.det_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in det.items()})
    trainer = pkg.depth_train.Trainer(args, student.cuda(), pkg.utils.get_info())
    trainer.set_teacher(teacher.cuda().eval())
    assert isinstance(trainer.folded_teacher, pkg.infer.Fp8FoldedNet)
    trainer.verbose = False
    c, d, tc, tv = pkg.synth.make_batch(2, side=128, rank=11, step=0)
    att = torch.ones(2, 1, 8, 8)
    record = trainer.train(1, [tuple(torch.from_numpy(a) if isinstance(a, np.ndarray) else a for a in (c, d, tc, tv, att))])
    assert trainer.skipped_steps == 0
    assert np.isfinite(record['dist_train_loss']) and record['dist_train_loss'] > 0
