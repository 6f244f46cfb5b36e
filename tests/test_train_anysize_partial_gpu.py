"""Training partial convolutions on the x3 kernels at any map width (ops.x3_any_partial / p3d_x3_any_partial_enable), on the GPU: the per-layer forward, stride-1
data gradient and weight gradient of a PartialConv (both factors, no bias) at maps whose width is no multiple of 4, against float64 on the same data and beside the
fp32-MFMA masked kernels, which the same call launches with the switch off.

Reference: y = conv2d(x m) mult, dx = conv2d_input(dy mult) m (+ what dx held), dw = conv2d_weight(x m, dy mult), in float64.
Bounds (tests/test_kernels_gpu.py::test_x3_kernels_match_fp32_kernels): the error relative to the largest reference value is at most 4e-6 and at most 4 x the
fp32-MFMA kernel's own.  Which kernel ran is read from the library's launch counters (ops.conv_path_stats).

Masks: m = (rand >= 0.3) with a zero rectangle of (r + 2) x (r + 3) at the corner of image 0 and one of the same size across a row end of the last image (its last
two columns and the first r + 1 of the next row); mult from ops.mask_count.  Every case checks that some window is empty (mult == 0), some full and -- where the
filter has more than one tap -- some partial, so that all three factor paths carry data.

Measured on an MI355X (profiles/train_anysize_partial.md): forward at most 8.6e-7 (the fp32-MFMA masked kernel: 1.0e-6), data gradient 8.9e-7 (2.4e-6), weight
gradient 5.8e-7 (5.8e-7; at most 1.8 x that kernel's own error, at 3 forced slabs)."""
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


def routes(c, k, r, stride):
    """the passes the masked ragged instances take: the x3 rule of each pass at the masked thresholds 64 / 64 / 96, without the width clauses"""
    fwd = c % 16 == 0 and c >= 32 and k >= 64
    dgrad = k % 16 == 0 and k >= 32 and c % 4 == 0 and c >= 64 and stride == 1
    wgrad = k >= 96 and c >= 96 and (r == 1 or c % 64 == 0)
    return int(fwd), int(dgrad), int(wgrad)


@pytest.fixture
def partial_on(pkg):
    """the switch on for the test body; what it found restored afterwards, with the forced split counts"""
    before = pkg.ops.x3_any_partial(True)
    try:
        yield pkg.ops.x3_any_partial
    finally:
        pkg.ops.x3_any_partial(before)
        pkg._lib.lib().p3d_fx_tune(0, 0)
        pkg._lib.lib().p3d_fx_tune(1, 0)


def _counts(stats):
    return tuple(stats['x3'][nm][0] for nm in PASSES), tuple(stats['fp32'][nm][0] for nm in PASSES)


def _err(got, ref):
    return ((got.double() - ref).abs().max() / ref.abs().max()).item()


def _masks(pkg, shape, seed):
    """(mask_in [n, 1, h, w], mult [n, 1, ho, wo]) with empty, full and partial windows"""
    c, k, h, w, r, stride, pad, dil, n = shape
    gen = torch.Generator().manual_seed(1000 + seed)
    m = (torch.rand(n, 1, h, w, generator=gen) >= 0.3).float()
    m[0, 0, :r + 2, :r + 3] = 0                                     # an image corner
    flat = m[n - 1, 0].reshape(-1)
    for row in range(h // 2, h // 2 + r + 2):                       # across a row end: the last two columns of a row and the first r + 1 of the next
        flat[row * w + w - 2: row * w + w + r + 1] = 0
    m = m.cuda()
    mult, _ = pkg.ops.mask_count(m, r, stride, pad, dil)
    count = F.conv2d(m.double(), torch.ones(1, 1, r, r, dtype=torch.float64, device='cuda'), None, stride, pad, dil)
    assert (mult[count == 0] == 0).all() and (count == 0).any(), 'no empty window'
    assert (count == r * r).any(), 'no full window'
    assert r == 1 or ((count > 0) & (count < r * r)).any(), 'no partial window'
    assert (mult[0] == 0).any() and (mult[n - 1] == 0).any()
    return m, mult


def _data(shape, seed):
    c, k, h, w, r, stride, pad, dil, n = shape
    gen = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(n, c, h, w, device='cuda', generator=gen) * (torch.rand(n, c, h, w, device='cuda', generator=gen) * 4 - 2).exp2()
    w0 = torch.randn(k, c, r, r, device='cuda', generator=gen) / (c * r * r) ** 0.5
    ho, wo = ((v + 2 * pad - dil * (r - 1) - 1) // stride + 1 for v in (h, w))
    dy = torch.randn(n, k, ho, wo, device='cuda', generator=gen)
    return x, w0, dy


def _reference(shape, x, w0, dy, m, mult):
    stride, pad, dil = shape[5:8]
    xm, dym = x.double() * m.double(), dy.double() * mult.double()
    y = F.conv2d(xm, w0.double(), None, stride, pad, dil) * mult.double()
    dx = torch.nn.grad.conv2d_input(x.shape, w0.double(), dym, stride, pad, dil) * m.double()
    dw = torch.nn.grad.conv2d_weight(xm, w0.shape, dym, stride, pad, dil)
    return y, dx, dw


def _autograd(pkg, shape, x, w0, dy, m, mult, bias=None):
    """forward and backward through ops.conv2d with the two factors: (y, dx, dw), launch counters"""
    ops = pkg.ops
    stride, pad, dil = shape[5:8]
    xr, wt = x.clone().requires_grad_(True), w0.clone().requires_grad_(True)
    ops.conv_path_stats(reset=True)
    y = ops.conv2d(xr, wt, bias, stride, pad, dil, mask_in=m, mult=mult)
    y.backward(dy)
    ops.join_side_stream()
    torch.cuda.synchronize()
    return (y.detach(), xr.grad, wt.grad), _counts(ops.conv_path_stats(reset=True))


def both_legs(pkg, shape, seed=3, bit_equal_runs=False):
    """one partial convolution with the switch off and on against float64: the bounds, and the counters of both legs.  Returns the on-leg results."""
    x, w0, dy = _data(shape, seed)
    m, mult = _masks(pkg, shape, seed)
    refs = _reference(shape, x, w0, dy, m, mult)
    before = pkg.ops.x3_any_partial(False)
    try:
        off, off_counts = _autograd(pkg, shape, x, w0, dy, m, mult)
        pkg.ops.x3_any_partial(True)
        on, on_counts = _autograd(pkg, shape, x, w0, dy, m, mult)
        again = _autograd(pkg, shape, x, w0, dy, m, mult)[0] if bit_equal_runs else None
    finally:
        pkg.ops.x3_any_partial(before)
    assert off_counts == ((0, 0, 0), (1, 1, 1)), off_counts                  # the fp32-MFMA masked kernels: the parent's launches
    moved = routes(shape[0], shape[1], shape[4], shape[5])
    assert on_counts == (moved, tuple(1 - v for v in moved)), (on_counts, moved)
    for i, name in enumerate(PASSES):
        e32, e3 = _err(off[i], refs[i]), _err(on[i], refs[i])
        print('%s %s: fp32-MFMA %.3e  x3 %.3e' % (shape, name, e32, e3))
        assert torch.isfinite(on[i]).all(), name
        assert e3 <= TOL and e3 <= 4 * e32, (name, e32, e3)
        if moved[i]:
            assert not torch.equal(on[i], off[i]), name                     # the other kernel really ran
        else:
            assert torch.equal(on[i], off[i]), name                         # bit for bit where the pass stayed
        if again is not None:
            assert torch.equal(on[i], again[i]), name
    return on


# ---- 1. each pass against float64 ---------------------------------------------------------------------------------------------------------------
# c, k, h, w, r, stride, pad, dil, n
SHAPES = [(128, 128, 17, 17, 3, 1, 1, 1, 1), (128, 128, 17, 17, 3, 1, 1, 1, 2), (128, 128, 17, 17, 3, 1, 1, 1, 3),       # 289 pixels = 18 K steps + 1: from n = 2 a K step spans two images
          (128, 128, 17, 19, 3, 1, 1, 1, 3), (128, 128, 17, 18, 3, 1, 1, 1, 3), (128, 128, 33, 17, 3, 1, 1, 1, 2),
          (128, 128, 17, 19, 3, 1, 2, 2, 3), (256, 128, 19, 19, 1, 1, 0, 1, 3),
          (128, 128, 17, 17, 3, 2, 1, 1, 3), (128, 128, 19, 19, 3, 2, 1, 1, 3),       # stride 2: forward and weight gradient on x3, the data gradient stays
          (64, 64, 17, 17, 3, 1, 1, 1, 3),                                            # half-dead tiles: forward and data gradient on x3, the weight gradient stays
          (128, 272, 19, 17, 3, 1, 1, 1, 1)]                                          # a partial channel tile (272 = 2 x 128 + 16)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'c%d_k%d_%dx%d_%dx%d_s%d_p%d_d%d_n%d' % (s[0], s[1], s[2], s[3], s[4], s[4], s[5], s[6], s[7], s[8]))
def test_each_pass_matches_float64(pkg, shape):
    both_legs(pkg, shape, seed=shape[2] * 100 + shape[3] + shape[8])


# ---- 2. exact weight gradient ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stride', [1, 2])
def test_integer_weight_gradient_is_exact(pkg, partial_on, stride):
    """x and dy integers in [-4, 4], mask_in in {0, 1}, the factor of dy an integer in {0, 1, 2} handed to p3d_conv2d_wgrad itself (the ABI takes any per-pixel
    factor): every product and every partial sum is an integer below 2^24, so a pixel lost or counted twice at a row end, an image end, a slab edge or in the last
    K step, or a factor taken from the neighbouring pixel or image, changes dw"""
    ops, L = pkg.ops, pkg._lib.lib()
    gen = torch.Generator(device='cuda').manual_seed(17 + stride)
    n, c, k, h, w = 3, 128, 128, 17, 19
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    x = torch.randint(-4, 5, (n, c, h, w), device='cuda', generator=gen).float()
    dy = torch.randint(-4, 5, (n, k, ho, wo), device='cuda', generator=gen).float()
    m = torch.randint(0, 2, (n, 1, h, w), device='cuda', generator=gen).float()
    f = torch.randint(0, 3, (n, 1, ho, wo), device='cuda', generator=gen).float()
    want = torch.nn.grad.conv2d_weight(x.double() * m.double(), (k, c, 3, 3), dy.double() * f.double(), stride, 1, 1).round().long()
    assert want.abs().max().item() < 2 ** 24 and n * ho * wo * 32 < 2 ** 24
    d = ops._desc(x.shape, (k, c, 3, 3), stride, 1, 1)
    for slabs in (0, 2, 3):
        L.p3d_fx_tune(0, slabs)
        nb = L.p3d_conv2d_wgrad_workspace_bytes(ctypes.byref(d))
        ws = ops.workspace(x.device, nb)
        dw = torch.full((k, c, 3, 3), float('nan'), device='cuda')
        ops.conv_path_stats(reset=True)
        pkg._lib.check(L.p3d_conv2d_wgrad(ctypes.byref(d), ops._p(dy), ops._p(x), ops._p(f), ops._p(m), ops._p(dw), ops._p(ws), ws.numel(), ops._stream()), 'p3d_conv2d_wgrad')
        torch.cuda.synchronize()
        counts = _counts(ops.conv_path_stats(reset=True))
        assert counts[0][2] == 1 and counts[1][2] == 0, counts
        assert torch.equal(dw.long(), want) and torch.equal(dw, dw.round()), (stride, slabs, (dw.double() - want.double()).abs().max().item())


# ---- 3. forced slab counts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('slabs', [2, 3])
def test_weight_gradient_slabs_cut_inside_images(pkg, partial_on, slabs):
    L = pkg._lib.lib()
    shape = (128, 128, 17, 19, 3, 1, 1, 1, 3)                 # 969 pixels = 61 K steps: 31 + 30, or 21 + 21 + 19 -- every cut inside an image
    d = pkg.ops._desc((3, 128, 17, 19), (128, 128, 3, 3), 1, 1, 1)
    L.p3d_fx_tune(0, slabs)
    assert L.p3d_conv2d_wgrad_workspace_bytes(ctypes.byref(d)) >= slabs * 128 * 128 * 9 * 4
    both_legs(pkg, shape, seed=slabs, bit_equal_runs=True)


@pytest.mark.parametrize('slabs', [2, 3])
def test_forward_and_data_gradient_slabs(pkg, partial_on, slabs):
    L = pkg._lib.lib()
    cin, cout, h, w = 512, 512, 17, 19
    d = pkg.ops._desc((2, cin, h, w), (cout, cin, 3, 3), 1, 1, 1)
    L.p3d_fx_tune(1, slabs)
    assert L.p3d_conv2d_fwd_workspace_bytes(ctypes.byref(d)) >= slabs * 2 * cout * h * w * 4      # the query covers the slabs of the masked ragged plan
    assert L.p3d_conv2d_dgrad_workspace_bytes(ctypes.byref(d)) >= slabs * 2 * cin * h * w * 4
    both_legs(pkg, (cin, cout, h, w, 3, 1, 1, 1, 2), seed=cin + slabs, bit_equal_runs=True)


# ---- 4. accumulate --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('slabs', [0, 2])
def test_data_gradient_accumulates(pkg, partial_on, slabs):
    """accumulate = 1 (ops.GradJoin): dx = what it held + the masked gradient, from the ragged store and from the sum over the slabs; the factor comes before the
    accumulate read, so where mask_in is 0 dx keeps its bits"""
    ops, L = pkg.ops, pkg._lib.lib()
    shape = (128, 128, 17, 17, 3, 1, 1, 1, 2)
    x, w0, dy = _data(shape, 23 + slabs)
    m, mult = _masks(pkg, shape, 23 + slabs)
    gen = torch.Generator(device='cuda').manual_seed(5)
    fill = torch.randn(x.shape, device='cuda', generator=gen)
    want = _reference(shape, x, w0, dy, m, mult)[1] + fill.double()
    d = ops._desc(x.shape, w0.shape, 1, 1, 1, accumulate=1)
    L.p3d_fx_tune(1, slabs)
    res = {}
    for on in (False, True):
        partial_on(on)
        dx = fill.clone()
        ws = ops.workspace(x.device, L.p3d_conv2d_dgrad_workspace_bytes(ctypes.byref(d)))
        if on and slabs:
            assert ws.numel() >= slabs * x.numel() * 4
        ops.conv_path_stats(reset=True)
        pkg._lib.check(L.p3d_conv2d_dgrad(ctypes.byref(d), ops._p(dy), ops._p(w0), ops._p(mult), ops._p(m), ops._p(dx), ops._p(ws), ws.numel(), ops._stream()), 'p3d_conv2d_dgrad')
        torch.cuda.synchronize()
        x3, fp32 = _counts(ops.conv_path_stats(reset=True))
        assert (x3[1], fp32[1]) == ((1, 0) if on else (0, 1))
        res[on] = _err(dx, want)
        if on:
            dead = (m == 0).expand_as(dx)
            assert dead.any() and torch.equal(dx[dead], fill[dead])
    print('accumulate, %d slabs: fp32-MFMA %.3e  x3 %.3e' % (slabs, res[False], res[True]))
    assert res[True] <= TOL and res[True] <= 4 * res[False], res


# ---- 5. empty windows -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('slabs', [0, 2])
def test_empty_windows_and_masked_inputs(pkg, partial_on, slabs):
    """y is exactly 0 where mult == 0; and what x holds under mask_in == 0 never reaches y: +-1e30 there (finite, so that x * 0 is 0 as in the reference) gives the
    bits of the run with zeros there"""
    ops, L = pkg.ops, pkg._lib.lib()
    shape = (128, 128, 17, 19, 3, 1, 1, 1, 3)
    x, w0, _ = _data(shape, 31 + slabs)
    m, mult = _masks(pkg, shape, 31 + slabs)
    dead = (m == 0).expand_as(x)
    x_zero = torch.where(dead, torch.zeros_like(x), x)
    sign = torch.where(torch.rand(x.shape, device='cuda', generator=torch.Generator(device='cuda').manual_seed(2)) < 0.5, -1.0, 1.0)
    x_big = torch.where(dead, 1e30 * sign, x)
    L.p3d_fx_tune(1, slabs)
    ys = []
    for xi in (x_zero, x_big):
        ops.conv_path_stats(reset=True)
        with torch.no_grad():
            ys.append(ops.conv2d(xi, w0, None, 1, 1, 1, mask_in=m, mult=mult))
        torch.cuda.synchronize()
        assert _counts(ops.conv_path_stats(reset=True)) == ((1, 0, 0), (0, 0, 0))
    empty = (mult == 0).expand_as(ys[0])
    assert empty.any() and (ys[0][empty] == 0).all() and (ys[1][empty] == 0).all()
    assert torch.isfinite(ys[1]).all() and torch.equal(ys[0], ys[1])
    assert _err(ys[0], _reference(shape, x, w0, torch.zeros_like(ys[0]), m, mult)[0]) <= TOL


# ---- 6. fenced buffers ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(128, 128, 17, 17, 3, 1, 1, 1, 3), (128, 128, 17, 33, 3, 2, 1, 1, 2)], ids=['17x17_n3', '17x33_s2_n2'])
def test_exact_size_fenced_buffers(pkg, partial_on, shape):
    """operands, both factors, results and workspace at exactly their sizes between fences: the bands behind the operands and the factors hold NaNs (a fetch beyond
    the tensor would bring one in), results and workspace start as NaNs, the bands around everything must stay as they were"""
    ops, L = pkg.ops, pkg._lib.lib()
    c, k, h, w, r, stride, pad, dil, n = shape
    x0, w0, dy0 = _data(shape, 41)
    m0, mult0 = _masks(pkg, shape, 41)
    refs = _reference(shape, x0, w0, dy0, m0, mult0)
    d = ops._desc(x0.shape, w0.shape, stride, pad, dil)
    fences = []

    def operand(src):
        t, f = fenced.fenced_like(src.shape, torch.float32, 4096, sentinel=0xFF)       # NaN bands
        t.copy_(src)
        fences.append(f)
        return t

    def result(shape_):
        t, f = fenced.fenced_like(shape_, torch.float32, 4096)
        fences.append(f)
        return t

    def scratch(nbytes):
        f = fenced.Fence(max(nbytes, 16), 65536, 'cuda')
        fences.append(f)
        return f.view

    x, wt, dy, m, mult = operand(x0), operand(w0), operand(dy0), operand(m0), operand(mult0)
    y, dx, dw = result(dy0.shape), result(x0.shape), result(w0.shape)
    b = ctypes.byref(d)
    ops.conv_path_stats(reset=True)
    nb = L.p3d_conv2d_fwd_workspace_bytes(b)
    pkg._lib.check(L.p3d_conv2d_fwd(b, ops._p(x), ops._p(wt), None, ops._p(m), ops._p(mult), ops._p(y), ops._p(scratch(nb)), nb, ops._stream()), 'p3d_conv2d_fwd')
    nb = L.p3d_conv2d_dgrad_workspace_bytes(b)
    pkg._lib.check(L.p3d_conv2d_dgrad(b, ops._p(dy), ops._p(wt), ops._p(mult), ops._p(m), ops._p(dx), ops._p(scratch(nb)), nb, ops._stream()), 'p3d_conv2d_dgrad')
    nb = L.p3d_conv2d_wgrad_workspace_bytes(b)
    pkg._lib.check(L.p3d_conv2d_wgrad(b, ops._p(dy), ops._p(x), ops._p(mult), ops._p(m), ops._p(dw), ops._p(scratch(nb)), nb, ops._stream()), 'p3d_conv2d_wgrad')
    torch.cuda.synchronize()
    s1 = int(stride == 1)
    assert _counts(ops.conv_path_stats(reset=True)) == ((1, s1, 1), (0, 1 - s1, 0))
    for f in fences:
        f.check()
    for got, ref, name in zip((y, dx, dw), refs, PASSES):
        assert torch.isfinite(got).all(), name
        assert _err(got, ref) <= TOL, name
    assert torch.equal(x, x0) and torch.equal(wt, w0) and torch.equal(dy, dy0) and torch.equal(m, m0) and torch.equal(mult, mult0)


# ---- 7. nothing else moves ------------------------------------------------------------------------------------------------------------------------
def _off_and_on(pkg, run):
    before = pkg.ops.x3_any_partial(False)
    try:
        off = run()
        pkg.ops.x3_any_partial(True)
        on = run()
    finally:
        pkg.ops.x3_any_partial(before)
    return off, on


def _same(off, on, counts):
    assert off[1] == on[1] == counts, (off[1], on[1])
    for a, b, name in zip(off[0], on[0], PASSES):
        assert torch.equal(a, b), name


def test_aligned_masked_shapes_keep_their_launches(pkg):
    shape = (128, 128, 16, 16, 3, 1, 1, 1, 2)
    x, w0, dy = _data(shape, 7)
    m, mult = _masks(pkg, shape, 7)
    _same(*_off_and_on(pkg, lambda: _autograd(pkg, shape, x, w0, dy, m, mult)), ((1, 1, 1), (0, 0, 0)))


def test_dense_odd_shapes_do_not_see_the_switch(pkg):
    import test_train_anysize_gpu as D
    shape = (128, 128, 17, 17, 3, 1, 1, 1, 2)
    x, w0, _, dy = D._data(shape, 9)
    dense = pkg.ops.x3_any(False)
    try:
        _same(*_off_and_on(pkg, lambda: D._autograd(pkg, shape, x, w0, None, dy)), ((0, 0, 0), (1, 1, 1)))
        pkg.ops.x3_any(True)
        _same(*_off_and_on(pkg, lambda: D._autograd(pkg, shape, x, w0, None, dy)), ((1, 1, 1), (0, 0, 0)))
    finally:
        pkg.ops.x3_any(dense)


def test_a_bias_or_one_factor_stays_on_fp32(pkg):
    """the call that carries a bias is the forward: it stays on fp32-MFMA, bit for bit (the masked instances take none, aligned or ragged).  p3d_conv2d_dgrad and
    p3d_conv2d_wgrad have no bias argument -- the bias gradient is a kernel of its own -- and route as they do without one, as on the aligned masked route"""
    shape = (128, 128, 17, 17, 3, 1, 1, 1, 2)
    x, w0, dy = _data(shape, 11)
    m, mult = _masks(pkg, shape, 11)
    bias = torch.randn(128, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    fp32 = ((0, 0, 0), (1, 1, 1))
    off, on = _off_and_on(pkg, lambda: _autograd(pkg, shape, x, w0, dy, m, mult, bias=bias.clone().requires_grad_(True)))
    assert off[1] == fp32 and on[1] == ((0, 1, 1), (1, 0, 0)), (off[1], on[1])
    assert torch.equal(off[0][0], on[0][0])
    _same(*_off_and_on(pkg, lambda: _autograd(pkg, shape, x, w0, dy, m, None)), fp32)
    _same(*_off_and_on(pkg, lambda: _autograd(pkg, shape, x, w0, dy, None, mult)), fp32)


def test_default_is_off(pkg):
    """also while the dense switch is on: neither switch looks at the other"""
    import os
    shape = (128, 128, 17, 17, 3, 1, 1, 1, 2)
    x, w0, dy = _data(shape, 9)
    m, mult = _masks(pkg, shape, 9)
    assert hasattr(pkg.ops, 'x3_any_partial')
    if os.environ.get('P3D_X3_ANY_PARTIAL') == '1':
        pkg.ops.x3_any_partial(False)
    dense = pkg.ops.x3_any(True)
    try:
        _, counts = _autograd(pkg, shape, x, w0, dy, m, mult)
    finally:
        pkg.ops.x3_any(dense)
    assert counts == ((0, 0, 0), (1, 1, 1)), counts


# ---- 8. the whole step ----------------------------------------------------------------------------------------------------------------------------
def _record_convs(pkg, model):
    """forward hooks on every convolution: (partial, in channels, out channels, stride, input needs a gradient) per call"""
    seen, hooks = [], []
    for mod in model.modules():
        if isinstance(mod, pkg.nn.Conv2d):
            hooks.append(mod.register_forward_hook(lambda md, inp, out: seen.append(
                (isinstance(md, pkg.partial_conv.PartialConv), md.in_channels, md.out_channels, md.stride[0], bool(inp[0].requires_grad)))))
    return seen, hooks


def _one_step(pkg, meta, switches):
    """a fresh model from the deterministic weights, one training step with (x3_any, x3_any_partial) = switches"""
    import test_step_gpu as S
    args, model, trainer = S.build(pkg, meta)
    model.train()
    trainer.adapt_learn_rate(1)
    c, d, tc, tv = pkg.synth.make_batch(meta['batch'], side=meta['side'], rank=0, step=0, invalid_frac=meta['invalid_frac'])
    batch = (torch.from_numpy(c).cuda(), torch.from_numpy(d).cuda(), torch.from_numpy(tc).cuda(), torch.from_numpy(tv).cuda())
    seen, hooks = _record_convs(pkg, model)
    before = pkg.ops.x3_any(switches[0]), pkg.ops.x3_any_partial(switches[1])
    try:
        pkg.ops.conv_path_stats(reset=True)
        loss = float(trainer.train_step(*batch))
        pkg.ops.join_side_stream()
        torch.cuda.synchronize()
        counts = _counts(pkg.ops.conv_path_stats(reset=True))
    finally:
        pkg.ops.x3_any(before[0])
        pkg.ops.x3_any_partial(before[1])
    for h in hooks:
        h.remove()
    grads = np.array([np.linalg.norm(p.grad.detach().cpu().numpy().astype(np.float64)) for p in trainer.list_params])
    return dict(loss=loss, spec=trainer.last_spec_cam.cpu().numpy(), total=trainer.optimizer.total_norm(), grads=grads, seen=seen, counts=counts)


def test_whole_step_of_a_partial_network(pkg):
    """partial_depthnet ResNet-18 at side 129 (maps of 33 and 17), batch 2: one step with both switches off, then a fresh identical model with both on, compared at
    the tolerances of the odd-side golden step (tests/test_step_gpu.py); the launch counters against the routing worked out here from channel counts and strides"""
    meta = json.loads(str(np.load(golden_path('step_partial_r18_b2.npz'))['meta']))
    assert meta['family'] == 'partial_depthnet' and meta['model'] == 'resnet18' and meta['batch'] == 2 and '-depth_only' in meta['extra']
    meta['side'] = 129
    off = _one_step(pkg, meta, (False, False))
    on = _one_step(pkg, meta, (True, True))
    assert abs(on['loss'] - off['loss']) < 1e-3 * abs(off['loss']), (on['loss'], off['loss'])
    assert np.abs(on['spec'] - off['spec']).max() < 1e-3 * np.abs(off['spec']).max()
    assert abs(on['total'] - off['total']) < 5e-3 * off['total'], (on['total'], off['total'])
    assert np.all(np.abs(on['grads'] - off['grads']) < 3e-2 * off['grads'] + 2e-4 * off['grads'].max())
    seen = on['seen']
    assert seen == off['seen'] and len(seen) == sum(1 for nm in meta['names'] if nm.endswith('conv1.weight') or nm.endswith('conv2.weight') or nm.endswith('downsample.0.weight') or nm == 'regressor.weight')
    dgrads = sum(1 for s in seen if s[4])
    assert off['counts'] == ((0, 0, 0), (len(seen), dgrads, len(seen))), off['counts']

    def on_fp32(partial, ci, co, st):
        """per pass: does this convolution stay on fp32-MFMA?  The stem; a masked conv below 64 / 64 / 96 channels on the side the pass looks at; a dense one below
        96; a stride-2 data gradient"""
        if ci < 16:
            return True, True, True
        least = (64, 64, 96) if partial else (96, 96, 96)
        return co < least[0], ci < least[1] or st == 2, min(ci, co) < least[2]

    stem = [s for s in seen if s[1] < 16]
    assert len(stem) == 1 and stem[0][0] and not stem[0][4]
    verdicts = [on_fp32(*s[:4]) for s in seen]
    fp32 = (sum(v[0] for v in verdicts), sum(v[1] for s, v in zip(seen, verdicts) if s[4]), sum(v[2] for v in verdicts))
    x3 = (len(seen) - fp32[0], dgrads - fp32[1], len(seen) - fp32[2])
    print('both switches on: x3 %s  fp32-MFMA %s' % on['counts'])
    assert on['counts'] == (x3, fp32), (on['counts'], x3, fp32, seen)
    wide = [v for s, v in zip(seen, verdicts) if s[0] and s[1:4] == (128, 128, 1)]
    assert len(wide) >= 3 and not any(any(v) for v in wide)          # the 128 -> 128 3x3 PartialConvs of layer2: x3 in all three passes
