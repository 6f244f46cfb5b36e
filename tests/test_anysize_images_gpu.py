"""Image operands at any map width (ops.x3_any_images / p3d_x3_any_images_enable), on the GPU: the mode-0 activation image at H * W that is no multiple of 4, and the
forward, stride-1 data gradient and weight gradient of dense convolutions fed by such images (p3d_fx_conv_*_img_any; ops_block.ConvImagesFn with the switch on)
against float64 on the same data and beside the fp32-MFMA kernels, which the same module launches with every any-width switch off.

Bounds (tests/test_kernels_gpu.py::test_x3_kernels_match_fp32_kernels, the ones the fp32-fed ragged kernels are held to): the error against float64, relative to the
largest reference value, is at most 4e-6 and at most 4 x the fp32-MFMA kernel's own on the same data.  Which kernel ran is read from the library's launch counters
(ops.conv_path_stats).  Every case prints both errors.

Measured on an MI355X (profiles/train_anysize_images.md): through the module forward 4.0e-7 - 7.2e-7, data gradient 4.9e-7 - 8.7e-7, weight gradient 2.4e-7 - 5.4e-7 (the
fp32-MFMA kernel: 4.7e-7 - 8.3e-7, 5.2e-7 - 1.0e-6, 2.2e-7 - 4.8e-7); at 2 / 3 forced slabs the regressor's forward 2.9e-6 / 1.9e-6 (fp32-MFMA 1.0e-6 / 1.1e-6, the
figure nearest a bound), the weight gradient 7.2e-7 / 4.3e-7."""
import ctypes
import json

import numpy as np
import pytest
import torch

import fenced
from conftest import golden_path

pytestmark = pytest.mark.gpu

TOL = 4e-6
PASSES = ('fwd', 'dgrad', 'wgrad')
F = torch.nn.functional
X3_ONLY, FP32_ONLY = ((1, 1, 1), (0, 0, 0)), ((0, 0, 0), (1, 1, 1))


@pytest.fixture
def switches(pkg):
    """all three any-width switches off for the test body (it turns on what it tests); what it found restored afterwards, with the forced split counts"""
    ops = pkg.ops
    before = (ops.x3_any(False), ops.x3_any_partial(False), ops.x3_any_images(False))
    try:
        yield ops
    finally:
        ops.x3_any(before[0])
        ops.x3_any_partial(before[1])
        ops.x3_any_images(before[2])
        pkg._lib.lib().p3d_fx_tune(0, 0)
        pkg._lib.lib().p3d_fx_tune(1, 0)


def _helpers():
    import test_train_anysize_gpu as A          # _data, _reference, _err, _counts, _autograd: the conventions of the fp32-fed ragged tests
    return A


def _desc(pkg, shape, accumulate=0):
    c, k, h, w, r, stride, pad, dil, n = shape
    return pkg.ops._desc((n, c, h, w), (k, c, r, r), stride, pad, dil, accumulate=accumulate)


def _module(pkg, shape, w0, b0):
    c, k, h, w, r, stride, pad, dil, n = shape
    conv = pkg.nn.Conv2d(c, k, r, stride=stride, padding=pad, dilation=dil, bias=b0 is not None).cuda()
    with torch.no_grad():
        conv.weight.copy_(w0)
        if b0 is not None:
            conv.bias.copy_(b0)
    return conv


def _module_run(pkg, shape, x, w0, b0, dy):
    """forward and backward through a pkg.nn.Conv2d module called without a join: (y, dx, dw), launch counters, the name of y's autograd node"""
    A, ops = _helpers(), pkg.ops
    conv = _module(pkg, shape, w0, b0)
    xr = x.clone().requires_grad_(True)
    ops.conv_path_stats(reset=True)
    y = conv(xr)
    node = type(y.grad_fn).__name__
    y.backward(dy)
    ops.join_side_stream()
    torch.cuda.synchronize()
    return (y.detach(), xr.grad, conv.weight.grad.clone()), A._counts(ops.conv_path_stats(reset=True)), node


def _check(name, got, off, ref, A):
    e32, e3 = A._err(off, ref), A._err(got, ref)
    print('%s: fp32-MFMA %.3e  x3 images %.3e' % (name, e32, e3))
    assert torch.isfinite(got).all(), name
    assert e3 <= TOL and e3 <= 4 * e32, (name, e32, e3)


def _ws(pkg, d, which, any_=True):
    L = pkg._lib.lib()
    query = L.p3d_fx_conv_img_any_workspace_bytes if any_ else L.p3d_fx_conv_img_workspace_bytes
    return pkg.ops.workspace(torch.device('cuda'), max(query(ctypes.byref(d), which), 16))


def _entry(pkg, which, d, w, x_img=None, dy_img=None, bias=None, out=None, ws=None, any_=True):
    """one direct call of p3d_fx_conv_{fwd,dgrad,wgrad}_img(_any), the weight image built into the workspace; returns the result"""
    ops, L = pkg.ops, pkg._lib.lib()
    c_, k_ = d.C, d.K
    name = 'p3d_fx_conv_%s_img%s' % (PASSES[which], '_any' if any_ else '')
    fn = getattr(L, name)
    ws = _ws(pkg, d, which, any_) if ws is None else ws
    b = ctypes.byref(d)
    if which == 0:
        out = torch.empty((d.N, k_, d.Ho, d.Wo), dtype=torch.float32, device='cuda') if out is None else out
        pkg._lib.check(fn(b, ops._p(x_img), ops._p(w), None, None if bias is None else ops._p(bias), ops._p(out), ops._p(ws), ws.numel(), ops._stream()), name)
    elif which == 1:
        out = torch.empty((d.N, c_, d.H, d.W), dtype=torch.float32, device='cuda') if out is None else out
        pkg._lib.check(fn(b, ops._p(dy_img), ops._p(w), None, ops._p(out), ops._p(ws), ws.numel(), ops._stream()), name)
    else:
        out = torch.empty_like(w) if out is None else out
        pkg._lib.check(fn(b, ops._p(dy_img), None, ops._p(x_img), ops._p(out), ops._p(ws), ws.numel(), ops._stream()), name)
    torch.cuda.synchronize()
    return out


# ---- 1. the image ---------------------------------------------------------------------------------------------------------------------------------------------
def _image_planes(img, n, c, hw):
    """the three bf16 planes of an activation image as float32 [3][N][C][HW] (layout [plane][n][c / 16][hw][16]), as tests/test_kernels_gpu.py decodes them"""
    raw = img.view(torch.bfloat16).reshape(3, n, c // 16, hw, 16).float()
    return raw.permute(0, 1, 2, 4, 3).reshape(3, n, c, hw)


@pytest.mark.parametrize('n,c,h,w', [(3, 32, 17, 19), (2, 16, 5, 5), (1, 48, 9, 18), (2, 16, 4, 4), (2, 32, 8, 12)], ids=lambda v: str(v))
def test_activation_image_at_any_size(pkg, n, c, h, w):
    """hi + mid + lo == x bit for bit at H * W = 3, 1, 2 and 0 mod 4; x at its exact size with NaNs behind it, the image at its exact size between fences, NaN bytes
    before the launch; at aligned sizes the bytes of p3d_fx_act_image"""
    ops, L = pkg.ops, pkg._lib.lib()
    gen = torch.Generator(device='cuda').manual_seed(3 + h * w)
    x0 = torch.randn(n, c, h, w, device='cuda', generator=gen) * torch.logspace(-6, 6, c, device='cuda').view(1, c, 1, 1)
    x, xf = fenced.fenced_like(x0.shape, torch.float32, 4096, sentinel=0xFF)          # a NaN band behind (and in front of) x
    x.copy_(x0)
    nbytes = L.p3d_fx_act_image_bytes(n, c, h * w)
    assert nbytes == 6 * x0.numel()
    out = fenced.Fence(nbytes, 65536, 'cuda')                                          # starts as NaN bytes
    pkg._lib.check(L.p3d_fx_act_image_any(ops._p(x), ops._p(out.view), n, c, h * w, ops._stream()), 'p3d_fx_act_image_any')
    torch.cuda.synchronize()
    out.check('activation image')
    xf.check('x')
    assert torch.equal(x, x0)
    planes = _image_planes(out.view, n, c, h * w)
    assert torch.isfinite(planes).all()
    back = (planes[0].double() + planes[1].double() + planes[2].double()).float().reshape(x0.shape)
    assert torch.equal(back, x0)
    assert (planes[1].abs() <= planes[0].abs() * 2.0 ** -7 + 1e-45).all() and (planes[2].abs() <= planes[0].abs() * 2.0 ** -15 + 1e-45).all()
    if (h * w) % 4 == 0:
        old = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device='cuda')
        pkg._lib.check(L.p3d_fx_act_image(0, ops._p(x), None, None, 0, ops._p(old), n, c, h * w, ops._stream()), 'p3d_fx_act_image')
        torch.cuda.synchronize()
        assert torch.equal(out.view, old)                                              # bit for bit the aligned kernel's image
    else:
        assert torch.equal(ops.act_image(x0), out.view)                                # ops.act_image routes mode 0 here
        with pytest.raises(pkg._lib.P3DError):
            ops.act_image(x0, 1, table=torch.zeros(c, 8, device='cuda'))               # modes 1 / 2 exist at aligned sizes only
        with pytest.raises(pkg._lib.P3DError):
            ops.act_image(x0, 2, x2=x0, table=torch.zeros(c, 8, device='cuda'))


# ---- 2. each pass against float64, through the module -----------------------------------------------------------------------------------------------------------
# c, k, h, w, r, stride, pad, dil, n
SHAPES = [(128, 128, 17, 17, 3, 1, 1, 1, 1), (128, 128, 17, 17, 3, 1, 1, 1, 2), (128, 128, 17, 17, 3, 1, 1, 1, 3),       # 289 pixels = 18 K steps + 1: from n = 2 a K step spans two images
          (128, 128, 17, 18, 3, 1, 1, 1, 3), (128, 128, 17, 19, 3, 1, 1, 1, 3), (128, 128, 17, 33, 3, 1, 1, 1, 2), (128, 128, 33, 17, 3, 1, 1, 1, 2),
          (128, 128, 17, 19, 3, 1, 2, 2, 3), (128, 128, 17, 19, 3, 1, 0, 1, 3),
          (128, 272, 19, 17, 3, 1, 1, 1, 1),                                                                        # a 16-channel last tile, with a bias
          (512, 128, 9, 11, 3, 1, 1, 1, 2), (128, 512, 9, 11, 3, 1, 1, 1, 2)]                                       # wide on one side: four channel tiles / 32 channel steps per tap
# the tap-inner K order starts at FX_TAP_INNER_MIN = 1024 reduction channels (csrc/p3d_fx.hip), so the two 512-channel cases above still walk the taps outermost: these
# two reach the tap-inner instance, the first in its forward, the second in its data gradient
SHAPES_TAP_INNER = [(1024, 128, 9, 11, 3, 1, 1, 1, 2), (128, 1024, 9, 11, 3, 1, 1, 1, 2)]
IDS = lambda s: 'c%d_k%d_%dx%d_%dx%d_s%d_p%d_d%d_n%d' % (s[0], s[1], s[2], s[3], s[4], s[4], s[5], s[6], s[7], s[8])


@pytest.mark.parametrize('shape', SHAPES + SHAPES_TAP_INNER, ids=IDS)
def test_each_pass_matches_float64(pkg, switches, shape):
    A = _helpers()
    with_bias = shape[1] == 272
    x, w0, b0, dy = A._data(shape, shape[2] * 100 + shape[3] + shape[8], with_bias)
    refs = A._reference(shape, x, w0, b0, dy)
    off, off_counts, off_node = _module_run(pkg, shape, x, w0, b0, dy)
    switches.x3_any_images(True)
    on, on_counts, on_node = _module_run(pkg, shape, x, w0, b0, dy)
    again = _module_run(pkg, shape, x, w0, b0, dy)[0]
    assert on_node == 'ConvImagesFnBackward' and off_node == 'Conv2dFnBackward', (on_node, off_node)
    assert on_counts == X3_ONLY and off_counts == FP32_ONLY, (on_counts, off_counts)
    for i, name in enumerate(PASSES):
        _check('%s %s' % (shape, name), on[i], off[i], refs[i], A)
        assert not torch.equal(on[i], off[i]), name                         # the other kernel really ran
        assert torch.equal(on[i], again[i]), name                           # bitwise reproducible


# ---- 3. direct entries, forced slabs ----------------------------------------------------------------------------------------------------------------------------
def _fp32_leg(pkg, shape, x, w0, b0, dy):
    A = _helpers()
    res, counts = A._autograd(pkg, shape, x, w0, b0, dy)
    assert counts == FP32_ONLY, counts
    return res


@pytest.mark.parametrize('slabs', [2, 3])
@pytest.mark.parametrize('cin,cout,h,w', [(2048, 272, 17, 17), (512, 512, 17, 19)])
def test_forward_and_data_gradient_slabs(pkg, switches, cin, cout, h, w, slabs):
    A, ops, L = _helpers(), pkg.ops, pkg._lib.lib()
    shape = (cin, cout, h, w, 3, 1, 1, 1, 2)
    x, w0, b0, dy = A._data(shape, cin + slabs, cout == 272)
    refs = A._reference(shape, x, w0, b0, dy)
    off = _fp32_leg(pkg, shape, x, w0, b0, dy)
    d = _desc(pkg, shape)
    b = ctypes.byref(d)
    own = [L.p3d_fx_conv_img_any_workspace_bytes(b, p) for p in (0, 1)]
    L.p3d_fx_tune(1, 1)
    one = [L.p3d_fx_conv_img_any_workspace_bytes(b, p) for p in (0, 1)]      # the unsplit launch: the weight image alone
    L.p3d_fx_tune(1, slabs)
    forced = [L.p3d_fx_conv_img_any_workspace_bytes(b, p) for p in (0, 1)]
    assert forced[0] >= one[0] + slabs * 2 * cout * h * w * 4 and forced[1] >= one[1] + slabs * 2 * cin * h * w * 4, (own, one, forced)
    x_img, dy_img = ops.act_image(x), ops.act_image(dy)
    ops.conv_path_stats(reset=True)
    runs = [(_entry(pkg, 0, d, w0, x_img=x_img, bias=b0), _entry(pkg, 1, d, w0, dy_img=dy_img)) for _ in range(2)]
    assert A._counts(ops.conv_path_stats(reset=True)) == ((2, 2, 0), (0, 0, 0))
    for i in (0, 1):
        _check('%s %d slabs %s' % (shape, slabs, PASSES[i]), runs[0][i], off[i], refs[i], A)
        assert torch.equal(runs[0][i], runs[1][i]), PASSES[i]


@pytest.mark.parametrize('slabs', [2, 3])
def test_weight_gradient_slabs_cut_inside_images(pkg, switches, slabs):
    A, ops, L = _helpers(), pkg.ops, pkg._lib.lib()
    shape = (128, 128, 17, 19, 3, 1, 1, 1, 3)                 # 969 pixels = 61 K steps: 31 + 30, or 21 + 21 + 19 -- every cut inside an image
    x, w0, _, dy = A._data(shape, slabs)
    refs = A._reference(shape, x, w0, None, dy)
    off = _fp32_leg(pkg, shape, x, w0, None, dy)
    d = _desc(pkg, shape)
    L.p3d_fx_tune(0, slabs)
    assert L.p3d_fx_conv_img_any_workspace_bytes(ctypes.byref(d), 2) >= slabs * 128 * 128 * 9 * 4
    x_img, dy_img = ops.act_image(x), ops.act_image(dy)
    ops.conv_path_stats(reset=True)
    runs = [_entry(pkg, 2, d, w0, x_img=x_img, dy_img=dy_img) for _ in range(2)]
    assert A._counts(ops.conv_path_stats(reset=True)) == ((0, 0, 2), (0, 0, 0))
    _check('%s %d slabs wgrad' % (shape, slabs), runs[0], off[2], refs[2], A)
    assert torch.equal(runs[0], runs[1])


# ---- 4. exact weight gradient -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stride', [1, 2])
def test_integer_weight_gradient_is_exact(pkg, switches, stride):
    """x and dy integers in [-4, 4]: every product and every partial sum is an integer below 2^24, so a pixel lost or counted twice at a row end, an image end, a
    slab edge or in the last K step changes dw"""
    ops, L = pkg.ops, pkg._lib.lib()
    gen = torch.Generator(device='cuda').manual_seed(17 + stride)
    n, c, k, h, w = 3, 128, 128, 17, 19
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    x = torch.randint(-4, 5, (n, c, h, w), device='cuda', generator=gen).float()
    dy = torch.randint(-4, 5, (n, k, ho, wo), device='cuda', generator=gen).float()
    w0 = torch.randn(k, c, 3, 3, device='cuda', generator=gen)
    want = torch.nn.grad.conv2d_weight(x.double(), w0.shape, dy.double(), stride, 1, 1).round().long()
    assert want.abs().max().item() < 2 ** 24 and n * ho * wo * 16 < 2 ** 24
    d = _desc(pkg, (c, k, h, w, 3, stride, 1, 1, n))
    assert (d.Ho, d.Wo) == (ho, wo) and L.p3d_fx_conv_img_any_supported(ctypes.byref(d)) & 4
    x_img, dy_img = ops.act_image(x), ops.act_image(dy)
    for slabs in (0, 2, 3):
        L.p3d_fx_tune(0, slabs)
        dw = _entry(pkg, 2, d, w0, x_img=x_img, dy_img=dy_img)
        assert torch.equal(dw.long(), want) and torch.equal(dw, dw.round()), (stride, slabs, (dw.double() - want.double()).abs().max().item())


@pytest.mark.parametrize('h,w,stride,n', [(4, 4, 1, 5), (5, 5, 1, 5), (4, 5, 1, 3), (9, 9, 2, 3)], ids=lambda v: str(v))
def test_small_maps(pkg, switches, h, w, stride, n):
    """the smallest maps the predicate admits: 16 output pixels (a K step is a whole image: the carry moves one image per step), 25 and 20 (a step spans two images),
    25 behind a stride of 2 -- the integer weight gradient exact, forward and data gradient within the bound of float64"""
    A, ops, L = _helpers(), pkg.ops, pkg._lib.lib()
    gen = torch.Generator(device='cuda').manual_seed(100 * h + w + stride)
    c = k = 128
    shape = (c, k, h, w, 3, stride, 1, 1, n)
    d = _desc(pkg, shape)
    bits = L.p3d_fx_conv_img_any_supported(ctypes.byref(d))
    assert d.Ho * d.Wo >= 16 and bits == (7 if stride == 1 else 5)
    x = torch.randint(-4, 5, (n, c, h, w), device='cuda', generator=gen).float()
    dy = torch.randint(-4, 5, (n, k, d.Ho, d.Wo), device='cuda', generator=gen).float()
    w0 = torch.randn(k, c, 3, 3, device='cuda', generator=gen) / (9 * c) ** 0.5
    y_ref, dx_ref, dw_ref = A._reference(shape, x, w0, None, dy)
    x_img, dy_img = ops.act_image(x), ops.act_image(dy)          # (either image pass, by H * W: the same bytes)
    for slabs in (0, 2):
        L.p3d_fx_tune(0, slabs)
        dw = _entry(pkg, 2, d, w0, x_img=x_img, dy_img=dy_img)
        assert torch.equal(dw.double(), dw_ref.round()), (slabs, (dw.double() - dw_ref).abs().max().item())
    y = _entry(pkg, 0, d, w0, x_img=x_img)
    e = A._err(y, y_ref)
    print('%s fwd: x3 images %.3e' % (shape, e))
    assert e <= TOL
    if bits & 2:
        dx = _entry(pkg, 1, d, w0, dy_img=dy_img)
        e = A._err(dx, dx_ref)
        print('%s dgrad: x3 images %.3e' % (shape, e))
        assert e <= TOL


# ---- 5. accumulate ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('slabs', [0, 2])
def test_data_gradient_accumulates(pkg, switches, slabs):
    """accumulate = 1: dx = what it held + the gradient, from the ragged store and from the sum over the slabs"""
    A, ops, L = _helpers(), pkg.ops, pkg._lib.lib()
    shape = (128, 128, 17, 17, 3, 1, 1, 1, 2)
    x, w0, _, dy = A._data(shape, 23 + slabs)
    gen = torch.Generator(device='cuda').manual_seed(5)
    fill = torch.randn(x.shape, device='cuda', generator=gen)
    want = torch.nn.grad.conv2d_input(x.shape, w0.double(), dy.double(), 1, 1, 1) + fill.double()
    d = _desc(pkg, shape, accumulate=1)
    L.p3d_fx_tune(1, slabs)
    # the fp32-MFMA kernel on the same data
    dx32 = fill.clone()
    ws = ops.workspace(x.device, L.p3d_conv2d_dgrad_workspace_bytes(ctypes.byref(d)))
    ops.conv_path_stats(reset=True)
    pkg._lib.check(L.p3d_conv2d_dgrad(ctypes.byref(d), ops._p(dy), ops._p(w0), None, None, ops._p(dx32), ops._p(ws), ws.numel(), ops._stream()), 'p3d_conv2d_dgrad')
    torch.cuda.synchronize()
    assert A._counts(ops.conv_path_stats(reset=True)) == ((0, 0, 0), (0, 1, 0))
    if slabs:
        assert L.p3d_fx_conv_img_any_workspace_bytes(ctypes.byref(d), 1) >= slabs * x.numel() * 4
    dx = _entry(pkg, 1, d, w0, dy_img=ops.act_image(dy), out=fill.clone())
    _check('accumulate, %d slabs' % slabs, dx, dx32, want, A)


# ---- 6. fenced buffers ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(128, 128, 17, 17, 3, 1, 1, 1, 3), (128, 272, 19, 17, 3, 1, 1, 1, 1)], ids=['17x17_n3', '19x17_k272_n1'])
def test_exact_size_fenced_buffers(pkg, switches, shape):
    """images, weights, results and workspaces at exactly their sizes between fences: the bands behind operands and images hold NaNs (a fetch beyond one would bring
    a NaN in), results and workspaces start as NaNs (scratch read before it is written shows), the bands around everything must stay as they were"""
    A, ops, L = _helpers(), pkg.ops, pkg._lib.lib()
    x0, w0, _, dy0 = A._data(shape, 41)
    refs = A._reference(shape, x0, w0, None, dy0)
    d = _desc(pkg, shape)
    b = ctypes.byref(d)
    fences = []

    def operand(src):
        t, f = fenced.fenced_like(src.shape, torch.float32, 4096, sentinel=0xFF)       # NaN bands
        t.copy_(src)
        fences.append(f)
        return t

    def image(src):
        f = fenced.Fence(L.p3d_fx_act_image_bytes(src.shape[0], src.shape[1], src.shape[2] * src.shape[3]), 65536, 'cuda', sentinel=0xFF)      # NaN bands, NaN bytes inside
        fences.append(f)
        return ops.act_image(src, out=f.view)

    def result(shape_):
        t, f = fenced.fenced_like(shape_, torch.float32, 4096)
        fences.append(f)
        return t

    def scratch(which):
        f = fenced.Fence(max(L.p3d_fx_conv_img_any_workspace_bytes(b, which), 16), 65536, 'cuda')
        fences.append(f)
        return f.view

    x, wt, dy = operand(x0), operand(w0), operand(dy0)
    x_img, dy_img = image(x), image(dy)
    x_img0, dy_img0 = x_img.clone(), dy_img.clone()
    y, dx, dw = result(dy0.shape), result(x0.shape), result(w0.shape)
    ops.conv_path_stats(reset=True)
    _entry(pkg, 0, d, wt, x_img=x_img, out=y, ws=scratch(0))
    _entry(pkg, 1, d, wt, dy_img=dy_img, out=dx, ws=scratch(1))
    _entry(pkg, 2, d, wt, x_img=x_img, dy_img=dy_img, out=dw, ws=scratch(2))
    assert A._counts(ops.conv_path_stats(reset=True)) == X3_ONLY
    for f in fences:
        f.check()
    for got, ref, name in zip((y, dx, dw), refs, PASSES):
        assert torch.isfinite(got).all(), name
        e = A._err(got, ref)
        print('%s fenced %s: %.3e' % (shape, name, e))
        assert e <= TOL, name
    assert torch.equal(x, x0) and torch.equal(wt, w0) and torch.equal(dy, dy0) and torch.equal(x_img, x_img0) and torch.equal(dy_img, dy_img0)
    # a workspace one byte short is refused, by name
    need = L.p3d_fx_conv_img_any_workspace_bytes(b, 2)
    short = ops.workspace(x.device, need)
    code = L.p3d_fx_conv_wgrad_img_any(b, ops._p(dy_img), None, ops._p(x_img), ops._p(dw), ops._p(short), need - 1, ops._stream())
    assert code != 0 and b'fx_conv_wgrad_img_any' in L.p3d_last_error()


# ---- 7. at aligned shapes the new entries agree with the old ----------------------------------------------------------------------------------------------------
def test_aligned_shapes_agree_with_the_aligned_entries(pkg, switches):
    """the aligned entry picks the same 128-row tile for 128 result channels (the 96-row fx16 tile does not fit better) and the same split-K plan, so forward and data
    gradient must agree bit for bit; the weight gradient runs another plan (a floor of 8 K steps per block instead of 32) and is held to float64"""
    A, ops, L = _helpers(), pkg.ops, pkg._lib.lib()
    shape = (128, 128, 16, 16, 3, 1, 1, 1, 2)
    x, w0, _, dy = A._data(shape, 7)
    refs = A._reference(shape, x, w0, None, dy)
    d = _desc(pkg, shape)
    assert L.p3d_fx_conv_img_supported(ctypes.byref(d)) == 7 and L.p3d_fx_conv_img_any_supported(ctypes.byref(d)) == 7
    x_img, dy_img = ops.act_image(x), ops.act_image(dy)
    new = [_entry(pkg, 0, d, w0, x_img=x_img), _entry(pkg, 1, d, w0, dy_img=dy_img), _entry(pkg, 2, d, w0, x_img=x_img, dy_img=dy_img)]
    old = [_entry(pkg, 0, d, w0, x_img=x_img, any_=False), _entry(pkg, 1, d, w0, dy_img=dy_img, any_=False), _entry(pkg, 2, d, w0, x_img=x_img, dy_img=dy_img, any_=False)]
    for i, name in enumerate(PASSES):
        e_new, e_old = A._err(new[i], refs[i]), A._err(old[i], refs[i])
        print('%s aligned %s: _img %.3e  _img_any %.3e' % (shape, name, e_old, e_new))
        assert torch.isfinite(new[i]).all() and e_new <= TOL, name
    assert torch.equal(new[0], old[0]) and torch.equal(new[1], old[1])


# ---- 8. nothing moves when off, or at aligned shapes when on ----------------------------------------------------------------------------------------------------
def test_switch_off_keeps_the_per_layer_path(pkg, switches):
    A, ops = _helpers(), pkg.ops
    shape = (128, 128, 17, 17, 3, 1, 1, 1, 2)
    x, w0, _, dy = A._data(shape, 9)
    conv = _module(pkg, shape, w0, None)
    assert not pkg.ops_block.conv_takes_images(conv, x)
    got, counts, node = _module_run(pkg, shape, x, w0, None, dy)
    want, want_counts = A._autograd(pkg, shape, x, w0, None, dy)
    assert node == 'Conv2dFnBackward' and counts == want_counts == FP32_ONLY
    for a, b, name in zip(got, want, PASSES):
        assert torch.equal(a, b), name
    switches.x3_any_images(True)
    assert pkg.ops_block.conv_takes_images(conv, x)                           # (the cached answer does not outlive the switch)
    switches.x3_any_images(False)
    assert not pkg.ops_block.conv_takes_images(conv, x)


def test_aligned_shapes_keep_their_launches(pkg, switches):
    A = _helpers()
    shape = (128, 272, 16, 16, 3, 1, 1, 1, 2)                                 # regressor-like: 272 output channels, a bias
    x, w0, b0, dy = A._data(shape, 11, True)
    off, off_counts, off_node = _module_run(pkg, shape, x, w0, b0, dy)
    switches.x3_any_images(True)
    on, on_counts, on_node = _module_run(pkg, shape, x, w0, b0, dy)
    assert on_node == off_node == 'ConvImagesFnBackward' and on_counts == off_counts == X3_ONLY
    for a, b, name in zip(off, on, PASSES):
        assert torch.equal(a, b), name


# ---- 9. the whole step ------------------------------------------------------------------------------------------------------------------------------------------
def _record_convs(pkg, model, seen):
    """forward hooks on every convolution: (module, called with a join, name of the autograd node of its output) per call"""
    def hook(mod, args, kwargs, out):
        joined = kwargs.get('join_put') is not None or kwargs.get('join_take') is not None or len(args) > 1
        seen.append((mod, joined, type(out.grad_fn).__name__))
    return [m.register_forward_hook(hook, with_kwargs=True) for m in model.modules() if isinstance(m, pkg.nn.Conv2d)]


def test_whole_step_at_an_odd_side(pkg, switches):
    """the reference's own step at side 257 (tests/golden/step_depth_r18_odd_b1.npz) with x3_any and x3_any_images on: the assertions of
    tests/test_train_anysize_gpu.py::test_whole_step_at_an_odd_side on the results (its tolerances are the reference golden's), and exactly the multi-tap stride-1
    convolutions with 96 channels or more on both sides that are called without a join travel as images -- the regressor among them; then a step with
    x3_any_images off, in which none does"""
    import test_step_gpu as S
    g = np.load(golden_path('step_depth_r18_odd_b1.npz'))
    meta = json.loads(str(g['meta']))
    assert meta['iters'] == 1 and meta['side'] % 2 == 1
    args, model, trainer = S.build(pkg, meta)
    names = meta['names']
    model.train()
    trainer.adapt_learn_rate(1)
    c, d, tc, tv = pkg.synth.make_batch(meta['batch'], side=meta['side'], rank=0, step=0, invalid_frac=meta['invalid_frac'])
    batch = (torch.from_numpy(c).cuda(), torch.from_numpy(d).cuda(), torch.from_numpy(tc).cuda(), torch.from_numpy(tv).cuda())
    zs = []
    hook = model.regressor.register_forward_hook(lambda m, i, o: zs.append(o.detach().cpu().numpy()))
    seen = []
    hooks = _record_convs(pkg, model, seen)
    switches.x3_any(True)
    switches.x3_any_images(True)
    loss = float(trainer.train_step(*batch))
    pkg.ops.join_side_stream()
    torch.cuda.synchronize()
    hook.remove()
    # -- tests/test_step_gpu.py::test_train_step_matches_reference on this case --
    assert abs(loss - g['losses'][0]) < 1e-3 * abs(g['losses'][0]), (loss, g['losses'][0])
    spec_sel = trainer.last_spec_cam.cpu().numpy().reshape(-1, 3)[tv.reshape(-1)]
    ref = g['spec_sel_0']
    assert np.abs(spec_sel - ref).max() < 1e-3 * np.abs(ref).max()
    total = trainer.optimizer.total_norm()
    assert abs(total - g['clip_total'][0]) < 5e-3 * g['clip_total'][0], (total, g['clip_total'][0])
    z0 = zs[0][0, :, 3, 5]
    assert np.abs(z0 - g['z_first_slice']).max() < 1e-3 * np.abs(g['z_first_slice']).max()
    assert np.abs(z0 - g['z_last_slice']).max() < 2e-3 * np.abs(g['z_last_slice']).max()
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    grads = {n: p.grad.detach().cpu().numpy() for n, p in zip(trainer.list_names, trainer.list_params)}
    gn = np.array([np.linalg.norm(grads[n].astype(np.float64)) for n in names])
    assert np.abs(gn - g['grad_norms']).max() < 5e-3 * g['grad_norms'].max()
    assert np.all(np.abs(gn - g['grad_norms']) < 3e-2 * g['grad_norms'] + 2e-4 * g['grad_norms'].max())
    pn = np.array([np.linalg.norm(sd[n].astype(np.float64)) for n in names])
    assert np.abs(pn - g['param_norms']).max() < 1e-5 * g['param_norms'].max()
    ps = np.array([sd[n].reshape(-1)[g['sample_idx'][i]] for i, n in enumerate(names)])
    assert np.abs(ps - g['param_samples']).max() < 3e-5
    bn = np.array([np.linalg.norm(sd[k].astype(np.float64)) for k in meta['buffer_names']])
    assert np.abs(bn - g['buffer_norms']).max() < 1e-4 * max(g['buffer_norms'].max(), 1.0)
    # -- the routing --
    took = {id(m) for m, _, node in seen if node == 'ConvImagesFnBackward'}
    expect = {id(m) for m, joined, _ in seen
              if m.kernel_size[0] > 1 and m.stride[0] == 1 and m.in_channels >= 96 and m.out_channels >= 96 and not joined}
    print('convolutions of the step: %d, as images: %d' % (len(seen), len(took)))
    assert took == expect, ([(m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0], j, n) for m, j, n in seen])
    assert took and id(model.regressor) in took
    # -- a second step with x3_any_images off: no convolution travels as images --
    switches.x3_any_images(False)
    del seen[:]
    trainer.train_step(*batch)
    pkg.ops.join_side_stream()
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    assert seen and not [n for _, _, n in seen if n == 'ConvImagesFnBackward']
