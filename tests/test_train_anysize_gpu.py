"""Training on the x3 kernels at any map width (ops.x3_any / p3d_x3_any_enable), on the GPU: the per-layer forward, stride-1 data gradient and weight gradient of
dense convolutions at maps whose width is no multiple of 4, against float64 on the same data and beside the fp32-MFMA kernels, which the same call launches with
the switch off.

Bounds (tests/test_kernels_gpu.py::test_x3_kernels_match_fp32_kernels): the error against float64, relative to the largest reference value, is at most 4e-6 and
at most 4 x the fp32-MFMA kernel's own.  Which kernel ran is read from the library's launch counters (ops.conv_path_stats).

Measured on an MI355X (profiles/train_anysize.md): forward and data gradient at most 2.2e-6 and 1.4e-6, the weight gradient 2.1e-7 - 4.1e-7 under its own plan (the
fp32-MFMA kernel: 2.2e-7 - 4.8e-7) and 7.2e-7 / 4.3e-7 at 2 / 3 forced slabs."""
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


@pytest.fixture
def any_on(pkg):
    """the switch on for the test body; what it found restored afterwards, with the forced split counts"""
    before = pkg.ops.x3_any(True)
    try:
        yield pkg.ops.x3_any
    finally:
        pkg.ops.x3_any(before)
        pkg._lib.lib().p3d_fx_tune(0, 0)
        pkg._lib.lib().p3d_fx_tune(1, 0)


def _counts(stats):
    return tuple(stats['x3'][nm][0] for nm in PASSES), tuple(stats['fp32'][nm][0] for nm in PASSES)


def _err(got, ref):
    return ((got.double() - ref).abs().max() / ref.abs().max()).item()


def _data(shape, seed, with_bias=False):
    c, k, h, w, r, stride, pad, dil, n = shape
    gen = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(n, c, h, w, device='cuda', generator=gen) * (torch.rand(n, c, h, w, device='cuda', generator=gen) * 4 - 2).exp2()
    w0 = torch.randn(k, c, r, r, device='cuda', generator=gen) / (c * r * r) ** 0.5
    b0 = torch.randn(k, device='cuda', generator=gen) if with_bias else None
    ho, wo = ((v + 2 * pad - dil * (r - 1) - 1) // stride + 1 for v in (h, w))
    dy = torch.randn(n, k, ho, wo, device='cuda', generator=gen)
    return x, w0, b0, dy


def _reference(shape, x, w0, b0, dy):
    c, k, h, w, r, stride, pad, dil, n = shape
    y = F.conv2d(x.double(), w0.double(), None if b0 is None else b0.double(), stride, pad, dil)
    dx = torch.nn.grad.conv2d_input(x.shape, w0.double(), dy.double(), stride, pad, dil)
    dw = torch.nn.grad.conv2d_weight(x.double(), w0.shape, dy.double(), stride, pad, dil)
    return y, dx, dw


def _autograd(pkg, shape, x, w0, b0, dy):
    """forward and backward through ops.conv2d: (y, dx, dw), launch counters"""
    ops = pkg.ops
    stride, pad, dil = shape[5:8]
    xr, wt = x.clone().requires_grad_(True), w0.clone().requires_grad_(True)
    b = None if b0 is None else b0.clone().requires_grad_(True)
    ops.conv_path_stats(reset=True)
    y = ops.conv2d(xr, wt, b, stride, pad, dil)
    y.backward(dy)
    ops.join_side_stream()
    torch.cuda.synchronize()
    return (y.detach(), xr.grad, wt.grad), _counts(ops.conv_path_stats(reset=True))


def both_legs(pkg, shape, seed=3, with_bias=False, bit_equal_runs=False):
    """one convolution with the switch off and on against float64: the bounds, and the counters of both legs.  Returns the on-leg results."""
    x, w0, b0, dy = _data(shape, seed, with_bias)
    refs = _reference(shape, x, w0, b0, dy)
    before = pkg.ops.x3_any(False)
    try:
        off, off_counts = _autograd(pkg, shape, x, w0, b0, dy)
        pkg.ops.x3_any(True)
        on, on_counts = _autograd(pkg, shape, x, w0, b0, dy)
        again = _autograd(pkg, shape, x, w0, b0, dy)[0] if bit_equal_runs else None
    finally:
        pkg.ops.x3_any(before)
    assert off_counts == ((0, 0, 0), (1, 1, 1)), off_counts                  # the fp32-MFMA kernels: the parent's launches
    s1 = int(shape[5] == 1)
    assert on_counts == ((1, s1, 1), (0, 1 - s1, 0)), on_counts              # a strided data gradient stays on the fp32-MFMA kernel
    for i, name in enumerate(PASSES):
        e32, e3 = _err(off[i], refs[i]), _err(on[i], refs[i])
        print('%s %s: fp32-MFMA %.3e  x3 %.3e' % (shape, name, e32, e3))
        assert torch.isfinite(on[i]).all(), name
        assert e3 <= TOL and e3 <= 4 * e32, (name, e32, e3)
        if on_counts[0][i]:
            assert not torch.equal(on[i], off[i]), name                     # the other kernel really ran
        else:
            assert torch.equal(on[i], off[i]), name
        if again is not None:
            assert torch.equal(on[i], again[i]), name
    return on


# ---- 1. each pass against float64 ---------------------------------------------------------------------------------------------------------------
# c, k, h, w, r, stride, pad, dil, n
SHAPES = [(128, 128, 17, 17, 3, 1, 1, 1, 1), (128, 128, 17, 17, 3, 1, 1, 1, 2), (128, 128, 17, 17, 3, 1, 1, 1, 3),       # 289 pixels = 18 K steps + 1: from n = 2 a K step spans two images
          (128, 128, 17, 18, 3, 1, 1, 1, 3), (128, 128, 17, 19, 3, 1, 1, 1, 3), (128, 128, 17, 33, 3, 1, 1, 1, 2), (128, 128, 33, 17, 3, 1, 1, 1, 2),
          (128, 128, 17, 19, 3, 1, 2, 2, 3), (128, 128, 17, 19, 3, 1, 0, 1, 3), (256, 128, 19, 19, 1, 1, 0, 1, 3),
          (128, 128, 17, 17, 3, 2, 1, 1, 3), (128, 128, 18, 18, 3, 2, 1, 1, 3), (128, 128, 19, 19, 3, 2, 1, 1, 3), (256, 128, 19, 19, 1, 2, 0, 1, 3),
          (128, 272, 19, 17, 3, 1, 1, 1, 1)]                                                                        # a partial channel tile (272 = 2 x 128 + 16), with bias


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'c%d_k%d_%dx%d_%dx%d_s%d_p%d_d%d_n%d' % (s[0], s[1], s[2], s[3], s[4], s[4], s[5], s[6], s[7], s[8]))
def test_each_pass_matches_float64(pkg, shape):
    both_legs(pkg, shape, seed=shape[2] * 100 + shape[3] + shape[8], with_bias=shape[1] == 272)


# ---- 2. exact weight gradient ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stride', [1, 2])
def test_integer_weight_gradient_is_exact(pkg, any_on, stride):
    """x and dy integers in [-4, 4]: every product and every partial sum is an integer below 2^24, so a pixel lost or counted twice at a row end, an image end, a
    slab edge or in the last K step changes dw"""
    gen = torch.Generator(device='cuda').manual_seed(17 + stride)
    n, c, k, h, w = 3, 128, 128, 17, 19
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    x = torch.randint(-4, 5, (n, c, h, w), device='cuda', generator=gen).float()
    dy = torch.randint(-4, 5, (n, k, ho, wo), device='cuda', generator=gen).float()
    w0 = torch.randn(k, c, 3, 3, device='cuda', generator=gen)
    want = torch.nn.grad.conv2d_weight(x.double(), w0.shape, dy.double(), stride, 1, 1).round().long()
    assert want.abs().max().item() < 2 ** 24 and n * ho * wo * 16 < 2 ** 24
    for slabs in (0, 2, 3):
        pkg._lib.lib().p3d_fx_tune(0, slabs)
        (_, _, dw), counts = _autograd(pkg, (c, k, h, w, 3, stride, 1, 1, n), x, w0, None, dy)
        assert counts[0][2] == 1 and counts[1][2] == 0, counts
        assert torch.equal(dw.long(), want) and torch.equal(dw, dw.round()), (stride, slabs, (dw.double() - want.double()).abs().max().item())


# ---- 3. forced slab counts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('slabs', [2, 3])
def test_weight_gradient_slabs_cut_inside_images(pkg, any_on, slabs):
    L = pkg._lib.lib()
    shape = (128, 128, 17, 19, 3, 1, 1, 1, 3)                 # 969 pixels = 61 K steps: 31 + 30, or 21 + 21 + 19 -- every cut inside an image
    d = pkg.ops._desc((3, 128, 17, 19), (128, 128, 3, 3), 1, 1, 1)
    L.p3d_fx_tune(0, slabs)
    assert L.p3d_conv2d_wgrad_workspace_bytes(ctypes.byref(d)) >= slabs * 128 * 128 * 9 * 4
    both_legs(pkg, shape, seed=slabs, bit_equal_runs=True)


@pytest.mark.parametrize('slabs', [2, 3])
@pytest.mark.parametrize('cin,cout,h,w', [(2048, 272, 17, 17), (512, 512, 17, 19)])
def test_forward_and_data_gradient_slabs(pkg, any_on, cin, cout, h, w, slabs):
    L = pkg._lib.lib()
    d = pkg.ops._desc((2, cin, h, w), (cout, cin, 3, 3), 1, 1, 1)
    L.p3d_fx_tune(1, slabs)
    assert L.p3d_conv2d_fwd_workspace_bytes(ctypes.byref(d)) >= slabs * 2 * cout * h * w * 4      # the plans really have that many slabs
    assert L.p3d_conv2d_dgrad_workspace_bytes(ctypes.byref(d)) >= slabs * 2 * cin * h * w * 4
    both_legs(pkg, (cin, cout, h, w, 3, 1, 1, 1, 2), seed=cin + slabs, with_bias=cout == 272, bit_equal_runs=True)


# ---- 4. accumulate --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('slabs', [0, 2])
def test_data_gradient_accumulates(pkg, any_on, slabs):
    """accumulate = 1 (ops.GradJoin): dx = what it held + the gradient, from the ragged store and from the sum over the slabs"""
    ops, L = pkg.ops, pkg._lib.lib()
    shape = (128, 128, 17, 17, 3, 1, 1, 1, 2)
    x, w0, _, dy = _data(shape, 23 + slabs)
    gen = torch.Generator(device='cuda').manual_seed(5)
    fill = torch.randn(x.shape, device='cuda', generator=gen)
    want = torch.nn.grad.conv2d_input(x.shape, w0.double(), dy.double(), 1, 1, 1) + fill.double()
    d = ops._desc(x.shape, w0.shape, 1, 1, 1, accumulate=1)
    L.p3d_fx_tune(1, slabs)
    res = {}
    for on in (False, True):
        any_on(on)
        dx = fill.clone()
        ws = ops.workspace(x.device, L.p3d_conv2d_dgrad_workspace_bytes(ctypes.byref(d)))
        if on and slabs:
            assert ws.numel() >= slabs * x.numel() * 4
        ops.conv_path_stats(reset=True)
        pkg._lib.check(L.p3d_conv2d_dgrad(ctypes.byref(d), ops._p(dy), ops._p(w0), None, None, ops._p(dx), ops._p(ws), ws.numel(), ops._stream()), 'p3d_conv2d_dgrad')
        torch.cuda.synchronize()
        x3, fp32 = _counts(ops.conv_path_stats(reset=True))
        assert (x3[1], fp32[1]) == ((1, 0) if on else (0, 1))
        res[on] = _err(dx, want)
    print('accumulate, %d slabs: fp32-MFMA %.3e  x3 %.3e' % (slabs, res[False], res[True]))
    assert res[True] <= TOL and res[True] <= 4 * res[False], res


# ---- 5. fenced buffers ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(128, 128, 17, 17, 3, 1, 1, 1, 3), (128, 128, 17, 33, 3, 2, 1, 1, 2)], ids=['17x17_n3', '17x33_s2_n2'])
def test_exact_size_fenced_buffers(pkg, any_on, shape):
    """operands, results and workspace at exactly their sizes between fences: the bands behind the operands hold NaNs (a fetch beyond the tensor would bring one
    in), results and workspace start as NaNs (scratch read before it is written shows), the bands around everything must stay as they were"""
    ops, L = pkg.ops, pkg._lib.lib()
    c, k, h, w, r, stride, pad, dil, n = shape
    x0, w0, _, dy0 = _data(shape, 41)
    refs = _reference(shape, x0, w0, None, dy0)
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

    x, wt, dy = operand(x0), operand(w0), operand(dy0)
    y, dx, dw = result(dy0.shape), result(x0.shape), result(w0.shape)
    b = ctypes.byref(d)
    ops.conv_path_stats(reset=True)
    nb = L.p3d_conv2d_fwd_workspace_bytes(b)
    pkg._lib.check(L.p3d_conv2d_fwd(b, ops._p(x), ops._p(wt), None, None, None, ops._p(y), ops._p(scratch(nb)), nb, ops._stream()), 'p3d_conv2d_fwd')
    nb = L.p3d_conv2d_dgrad_workspace_bytes(b)
    pkg._lib.check(L.p3d_conv2d_dgrad(b, ops._p(dy), ops._p(wt), None, None, ops._p(dx), ops._p(scratch(nb)), nb, ops._stream()), 'p3d_conv2d_dgrad')
    nb = L.p3d_conv2d_wgrad_workspace_bytes(b)
    pkg._lib.check(L.p3d_conv2d_wgrad(b, ops._p(dy), ops._p(x), None, None, ops._p(dw), ops._p(scratch(nb)), nb, ops._stream()), 'p3d_conv2d_wgrad')
    torch.cuda.synchronize()
    s1 = int(stride == 1)
    assert _counts(ops.conv_path_stats(reset=True)) == ((1, s1, 1), (0, 1 - s1, 0))
    for f in fences:
        f.check()
    for got, ref, name in zip((y, dx, dw), refs, PASSES):
        assert torch.isfinite(got).all(), name
        assert _err(got, ref) <= TOL, name
    assert torch.equal(x, x0) and torch.equal(wt, w0) and torch.equal(dy, dy0)


# ---- 6. aligned shapes: nothing moves -------------------------------------------------------------------------------------------------------------
def test_aligned_shapes_keep_their_launches(pkg):
    shape = (128, 128, 16, 16, 3, 1, 1, 1, 2)
    x, w0, _, dy = _data(shape, 7)
    before = pkg.ops.x3_any(False)
    try:
        off, off_counts = _autograd(pkg, shape, x, w0, None, dy)
        pkg.ops.x3_any(True)
        on, on_counts = _autograd(pkg, shape, x, w0, None, dy)
    finally:
        pkg.ops.x3_any(before)
    assert off_counts == on_counts == ((1, 1, 1), (0, 0, 0))
    for a, b, name in zip(off, on, PASSES):
        assert torch.equal(a, b), name


# ---- 7. the default keeps the fallback ------------------------------------------------------------------------------------------------------------
def test_default_is_off(pkg):
    import os
    shape = (128, 128, 17, 17, 3, 1, 1, 1, 2)
    x, w0, _, dy = _data(shape, 9)
    assert hasattr(pkg.ops, 'x3_any')
    if os.environ.get('P3D_X3_ANY') == '1':
        pkg.ops.x3_any(False)
    _, counts = _autograd(pkg, shape, x, w0, None, dy)
    assert counts == ((0, 0, 0), (1, 1, 1)), counts


# ---- 8. the whole step ----------------------------------------------------------------------------------------------------------------------------
def _record_convs(pkg, model):
    """forward hooks on every convolution: (in channels, out channels, stride, input needs a gradient) per call"""
    seen, hooks = [], []
    for m in model.modules():
        if isinstance(m, pkg.nn.Conv2d):
            hooks.append(m.register_forward_hook(lambda mod, inp, out: seen.append((mod.in_channels, mod.out_channels, mod.stride[0], bool(inp[0].requires_grad)))))
    return seen, hooks


def test_whole_step_at_an_odd_side(pkg):
    """the reference's own step at side 257 (tests/golden/step_depth_r18_odd_b1.npz) with the switch on: the assertions of tests/test_step_gpu.py on that case, x3
    launches in all three passes, and on the fp32-MFMA kernels exactly the stem, the 64-channel layers and the strided data gradients; then a step with the switch
    off, which launches what it always did"""
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
    seen, hooks = _record_convs(pkg, model)
    before = pkg.ops.x3_any(True)
    try:
        pkg.ops.conv_path_stats(reset=True)
        loss = float(trainer.train_step(*batch))
        pkg.ops.join_side_stream()
        torch.cuda.synchronize()
        on = _counts(pkg.ops.conv_path_stats(reset=True))
    finally:
        pkg.ops.x3_any(before)
    hook.remove()
    for h in hooks:
        h.remove()
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
    # -- the routing: every convolution of the step went through the per-layer path once per pass --
    assert len(seen) == sum(1 for n in names if n.endswith('conv1.weight') or n.endswith('conv2.weight') or n.endswith('downsample.0.weight') or n == 'regressor.weight')
    stem = [s for s in seen if s[0] < 16]
    assert len(stem) == 1 and not stem[0][3]
    fp32_fwd = sum(1 for ci, co, st, rg in seen if ci < 16 or co == 64)
    fp32_dgrad = sum(1 for ci, co, st, rg in seen if rg and (ci == 64 or st == 2))
    fp32_wgrad = sum(1 for ci, co, st, rg in seen if ci < 16 or ci == 64 or co == 64)
    dgrads = sum(1 for s in seen if s[3])
    x3, fp32 = on
    print('switch on: x3 %s  fp32-MFMA %s' % (x3, fp32))
    assert fp32 == (fp32_fwd, fp32_dgrad, fp32_wgrad), (on, seen)
    assert x3 == (len(seen) - fp32_fwd, dgrads - fp32_dgrad, len(seen) - fp32_wgrad) and min(x3) > 0, (on, seen)
    # -- a second step with the switch off: the counters of today --
    pkg.ops.x3_any(False)
    try:
        pkg.ops.conv_path_stats(reset=True)
        trainer.train_step(*batch)
        pkg.ops.join_side_stream()
        torch.cuda.synchronize()
        off = _counts(pkg.ops.conv_path_stats(reset=True))
    finally:
        pkg.ops.x3_any(before)
    assert off == ((0, 0, 0), (len(seen), dgrads, len(seen))), off
