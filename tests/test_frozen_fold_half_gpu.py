"""Training frozen-BatchNorm layers on folded fp16 convolutions under -half_acc (ops.frozen_fold_half, ops_frozen.HFrozenConvBnFn, csrc/p3d_hfrozen.hip), on the
GPU: the mask pass and fold kind 4 on fenced buffers, one layer forward and backward against float64 and beside today's path (fp16 conv, then the eval-mode
BatchNorm pass), a whole network against the fp32 step, and distillation.

Bounds.  The mask pass's sums end in one rounding to fp32 of an fp64 sum: 2^-24 ~ 6e-8 of |sum| <= sum |g|, held at 1e-7 like the fp32 kernel's.  g, the kind-4
image, y against the inference forward on the plan's own image, and dres are bit-equal to what they restate.  One layer: the error of y, dx, dw, dgamma, dbeta
against float64, relative to the largest reference value of the tensor, is at most 4 x the error of today's path on the same data in the same test (the margin
of tests/test_frozen_fold_gpu.py); the folded path rounds once where today's rounds z and y, so it should sit below 1 x.  Whole network: each fp16 leg is
measured against the fp32 step on the same weights and batch; the folded leg's median over the tensors and its worst tensor are each at most 2 x the unfolded
leg's (both are fp16 paths and the folded one has no more roundings; 2 x covers different rounding points)."""
import ctypes

import numpy as np
import pytest
import torch

import fenced

pytestmark = pytest.mark.gpu

F = torch.nn.functional
CL = torch.channels_last
P3D_EINVAL = -1


@pytest.fixture
def fold_on(pkg):
    """the -half_acc switch on for the test body; what it found restored afterwards"""
    before = pkg.ops.frozen_fold_half(True)
    try:
        yield pkg.ops.frozen_fold_half
    finally:
        pkg.ops.frozen_fold_half(before)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == torch.float16 else t.view(torch.int32)


def _half_cl(t):
    return t.half().contiguous(memory_format=CL)


# ---- 1. the mask pass -----------------------------------------------------------------------------------------------------------------------------
# The kernel's grid constants (csrc/p3d_hfrozen.hip): a block takes 256 / (K / 8) pixels at a time, the grid has HFZ_MAX_BLOCKS = 512 blocks at the most and
# a pass of it covers HFZ_UNROLL = 4 chunks per block.  At K = 8 (256 pixels a chunk) P > 512 * 4 * 256 therefore needs a second pass; at K = 64 a chunk is
# 32 pixels and 173 = 5 * 32 + 13 ends in a partial one.
GRID_PASS_PIXELS_K8 = 512 * 4 * 256
MASK_SHAPES = [(1, 8), (5, 64), (323, 2048), (GRID_PASS_PIXELS_K8 + 300, 8), (173, 64)]


def _mask_data(p, k, seed):
    gen = torch.Generator(device='cuda').manual_seed(seed)
    dy = (torch.randn(p, k, device='cuda', generator=gen) * 8).half()
    dy[:, 0] = 60000.0                                                                 # every pixel of a channel near the top of fp16: with a few pixels the
    dy[:, 1] = ((torch.rand(p, device='cuda', generator=gen) * 2 - 1) * 60000).half()  # sum leaves fp16's range
    y = torch.randn(p, k, device='cuda', generator=gen).clamp_min(0).half()            # half of it exact zeros, as a ReLU leaves them
    y.view(-1)[::7] = -0.0
    y.view(-1)[3::11] = 0.0
    y.view(-1)[5::13] = -1.5                                                           # (never behind a ReLU; the kernel tests y > 0 all the same)
    y[:, 0] = 1.0                                                                      # the large channel passes the mask whole
    return dy, y


@pytest.mark.parametrize('shape', MASK_SHAPES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'plain'])
def test_mask_pass(pkg, shape, relu):
    ops, L = pkg.ops, pkg._lib.lib()
    p, k = shape
    dy0, y0 = _mask_data(p, k, 11 + p % 1000 + k)
    fences = []

    def operand(src):
        t, f = fenced.fenced_like(src.shape, torch.float16, 4096, sentinel=0xFF)       # NaN bands: a fetch beyond the tensor would bring one into the sums
        t.copy_(src)
        fences.append(f)
        return t

    def result(shape_, dtype):
        t, f = fenced.fenced_like(shape_, dtype, 4096)
        fences.append(f)
        return t

    dy, y = operand(dy0), operand(y0)
    nb = L.p3d_hfrozen_grad_mask_workspace_bytes(p, k)
    assert nb >= 8 * k
    want_g = torch.where(y0 > 0, dy0, torch.zeros_like(dy0)) if relu else dy0
    want = want_g.double().sum(dim=0)
    scale = want_g.double().abs().sum(dim=0)
    if p >= 2:
        assert want[0].item() > 65504                                                  # the sum has left fp16's range
    runs = []
    for _ in range(2):
        g, sums = result(shape, torch.float16), result((k,), torch.float32)
        ws = fenced.Fence(nb, 65536, 'cuda')
        fences.append(ws)
        pkg._lib.check(L.p3d_hfrozen_grad_mask(ops._p(dy), ops._p(y) if relu else None, ops._p(g) if relu else None, ops._p(sums), p, k, ops._p(ws.view), nb,
                                               ops._stream()), 'p3d_hfrozen_grad_mask')
        runs.append((g, sums))
    torch.cuda.synchronize()
    for f in fences:
        f.check()
    (g, sums), (g2, sums2) = runs
    if relu:
        assert torch.equal(_bits(g), _bits(want_g))                                    # bit-equal, a masked element +0
    else:
        assert fences[2].untouched()                                                   # without y nothing is written: dy itself is g
    err = ((sums.double() - want).abs() / scale.clamp_min(1e-30)).max().item()
    print('hmask %s relu %d: sums err / sum|g| %.3e' % (shape, relu, err))
    assert torch.isfinite(sums).all() and err <= 1e-7, err
    assert torch.equal(_bits(sums), _bits(sums2)) and (not relu or torch.equal(_bits(g), _bits(g2)))
    assert torch.equal(_bits(dy), _bits(dy0)) and torch.equal(_bits(y), _bits(y0))


@pytest.mark.parametrize('p,k', [(5, 12), (5, 2056)], ids=['k12', 'k2056'])
def test_mask_pass_refuses_a_shape_outside_its_rule(pkg, p, k):
    ops, L = pkg.ops, pkg._lib.lib()
    made = [fenced.fenced_like((p, k), torch.float16, 4096) for _ in range(3)] + [fenced.fenced_like((k,), torch.float32, 4096)]
    ws = fenced.Fence(65536, 4096, 'cuda')
    (dy, y, g, sums) = (t for t, _ in made)
    rc = L.p3d_hfrozen_grad_mask(ops._p(dy), ops._p(y), ops._p(g), ops._p(sums), p, k, ops._p(ws.view), 65536, ops._stream())
    torch.cuda.synchronize()
    assert rc == P3D_EINVAL and L.p3d_last_error()
    assert L.p3d_hfrozen_grad_mask_workspace_bytes(p, k) == 0
    for _, f in made:
        f.check()
        assert f.untouched()
    ws.check()
    assert ws.untouched()


# ---- 2. fold kind 4 -------------------------------------------------------------------------------------------------------------------------------
# K, C, RS, BatchNorm
FOLDS = [(8, 8, 1, True), (96, 20, 9, True), (2048, 64, 1, True), (64, 24, 9, False)]


def test_fold_kind_4_is_the_crsk_image_of_the_folded_weight(pkg):
    """one table with a kind 1, a kind 2 and a kind 4 job per case: the kind-4 (and kind-2) image is bit for bit what p3d_weight_images_f16 builds from the
    kind-1 output of the same job; channels C .. Cpad - 1 are zero; nothing outside the images is written"""
    ops, L = pkg.ops, pkg._lib.lib()
    gen = torch.Generator(device='cuda').manual_seed(4)
    jobs, cases, fences = [], [], []
    for k, c, rs, with_bn in FOLDS:
        cpad = (c + 7) // 8 * 8
        w = torch.randn(k, c, rs, device='cuda', generator=gen) / (c * rs) ** 0.5
        gamma, beta, mean = (torch.rand(k, device='cuda', generator=gen) + 0.5, torch.randn(k, device='cuda', generator=gen) * 0.3,
                             torch.randn(k, device='cuda', generator=gen) * 0.5)
        var = torch.rand(k, device='cuda', generator=gen) * 1.5 + 0.5
        outs = {}
        for kind, shape, dtype in ((1, (k, c, rs), torch.float32), (2, (k, rs, cpad), torch.float16), (4, (cpad, rs, k), torch.float16)):
            t, f = fenced.fenced_like(shape, dtype, 4096)
            fences.append(f)
            outs[kind] = t
            j = pkg._lib.FoldJob()
            j.w, j.conv_bias = w.data_ptr(), None
            if with_bn:
                j.gamma, j.beta, j.mean, j.var = gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), var.data_ptr()
            else:
                j.gamma = j.beta = j.mean = j.var = None
            j.out, j.bias_out = t.data_ptr(), None
            j.K, j.C, j.RS, j.c_offset, j.c_total, j.kind, j.eps, j.reserved = k, c, rs, 0, c, kind, 1e-5, cpad if kind != 1 else 0
            jobs.append(j)
        cases.append((k, c, rs, cpad, with_bn, w, outs, (gamma, beta, mean, var)))
    table = torch.frombuffer(bytearray((pkg._lib.FoldJob * len(jobs))(*jobs)), dtype=torch.uint8).cuda()
    pkg._lib.check(L.p3d_fx_fold_bn_images(ops._p(table), len(jobs), 64, ops._stream()), 'p3d_fx_fold_bn_images')
    torch.cuda.synchronize()
    for f in fences:
        f.check()
    for k, c, rs, cpad, with_bn, w, outs, _ in cases:
        if not with_bn:
            assert torch.equal(outs[1], w)                                              # gamma == NULL: s = 1
        krsc = torch.empty(k, rs, cpad, dtype=torch.float16, device='cuda')
        crsk = torch.empty(cpad, rs, k, dtype=torch.float16, device='cuda')
        pkg._lib.check(L.p3d_weight_images_f16(ops._p(outs[1]), ops._p(krsc), ops._p(crsk), k, c, rs, cpad, ops._stream()), 'p3d_weight_images_f16')
        torch.cuda.synchronize()
        assert torch.equal(_bits(outs[4]), _bits(crsk)), (k, c, rs)
        assert torch.equal(_bits(outs[2]), _bits(krsc)), (k, c, rs)
        assert torch.equal(_bits(outs[4]), _bits(outs[2].permute(2, 1, 0)))             # the same values in the other layout
        if cpad > c:
            assert torch.equal(_bits(outs[4][c:]), torch.zeros_like(_bits(outs[4][c:])))        # +0 in the padding channels
        assert outs[4][:c].abs().max().item() > 0


# ---- 3. one layer ---------------------------------------------------------------------------------------------------------------------------------
# n, c, k, r, stride, h, w, res, relu, join
LAYERS = [(2, 64, 64, 3, 1, 16, 16, True, True, False), (2, 64, 64, 3, 1, 16, 16, False, True, False), (2, 64, 64, 3, 1, 16, 16, True, False, False),
          (2, 64, 64, 3, 1, 16, 16, False, False, False),
          (3, 128, 128, 3, 1, 17, 19, True, True, False), (3, 128, 256, 1, 2, 17, 19, False, False, False), (2, 64, 96, 3, 2, 33, 33, False, True, False),
          (2, 256, 64, 1, 1, 16, 16, False, True, True)]
NEAR_SWITCH = 2.0 ** -8               # gradients are compared only where |u_ref| > NEAR_SWITCH * max |u_ref| (u: the value in front of the ReLU)
LEFT_OUT_MOST = 0.08                  # the reference alone leaves out <= 3.2 % without a residual and <= 2.0 % with one (20 seeds, on the CPU)


def _layer_id(v):
    n, c, k, r, stride, h, w, res, relu, join = v
    return 'n%d_%dto%d_%dx%d_s%d_%dx%d%s%s%s' % (n, c, k, r, r, stride, h, w, '_res' if res else '', '_relu' if relu else '', '_join' if join else '')


def _layer(pkg, case, seed):
    n, c, k, r, stride, h, w, res, relu, join = case
    gen = torch.Generator(device='cuda').manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device='cuda', generator=gen)
    conv = pkg.nn.Conv2d(c, k, kernel_size=r, stride=stride, padding=r // 2, bias=False).cuda()
    bn = pkg.nn.BatchNorm2d(k).cuda().eval()
    with torch.no_grad():                                                              # drawn as in test_hbn_frozen_statistics_backward
        conv.weight.copy_(rnd(*conv.weight.shape) / (c * r * r) ** 0.5)
        bn.weight.copy_(torch.rand(k, device='cuda', generator=gen) + 0.5)
        bn.bias.copy_(rnd(k) * 0.3)
        bn.running_mean.copy_(rnd(k) * 0.5)
        bn.running_var.copy_(torch.rand(k, device='cuda', generator=gen) * 1.5 + 0.5)
    pkg.ops_half.refresh_weights(conv)
    ho, wo = ((v + 2 * (r // 2) - r) // stride + 1 for v in (h, w))
    x = _half_cl(rnd(n, c, h, w))
    rs = _half_cl(rnd(n, k, ho, wo)) if res else None
    dy = _half_cl(rnd(n, k, ho, wo))
    stash = _half_cl(rnd(n, c, h, w)) if join else None
    return conv, bn, x, rs, dy, stash


def _reference(case, conv, bn, x, rs, dy, stash):
    """float64 on the CPU: conv -> eval BatchNorm -> + res -> ReLU and its autograd on the fp16-rounded x, res, dy and the fp32 masters; returns the results and
    the value u in front of the ReLU"""
    n, c, k, r, stride, h, w, res, relu, join = case
    d = lambda t: t.detach().double().cpu().contiguous()
    xr, wr = d(x).requires_grad_(True), d(conv.weight).requires_grad_(True)
    gm, bt = d(bn.weight).requires_grad_(True), d(bn.bias).requires_grad_(True)
    rr = d(rs).requires_grad_(True) if res else None
    z = F.conv2d(xr, wr, None, stride, r // 2)
    sigma = (d(bn.running_var) + bn.eps).sqrt()
    u = (z - d(bn.running_mean)[None, :, None, None]) / sigma[None, :, None, None] * gm[None, :, None, None] + bt[None, :, None, None]
    if res:
        u = u + rr
    y = u.relu() if relu else u
    y.backward(d(dy))
    out = dict(y=y.detach(), dx=xr.grad + (d(stash) if join else 0), dw=wr.grad, dgamma=gm.grad, dbeta=bt.grad)
    if res:
        out['dres'] = rr.grad
    return out, u.detach()


def _today_model(case, conv, bn, x, rs, dy, stash):
    """Today's path as float64 arithmetic with its rounding points -- fp16 tensors, fp32 parameter gradients -- and nothing else (exact accumulation): the weight image fp16(w), z = fp16(conv(x, w16)),
    y = fp16(relu?(bn(z) + res)), dz = fp16(g * s) with g = dy * [y > 0], dx = fp16(dgrad(dz, w16)), dw = wgrad(x, dz), dgamma = sum g * xhat(z), dbeta = sum g.
    Stands in for today's path where its kernels refuse the channel count (so there is no run to compare with): its error is the rounding the formats impose
    on that path, and no figure of it comes from the code under test."""
    n, c, k, r, stride, h, w, res, relu, join = case
    d = lambda t: t.detach().double().cpu().contiguous()
    r16 = lambda t: t.half().double()
    xr, w16 = d(x), r16(d(conv.weight))
    sigma = (d(bn.running_var) + bn.eps).sqrt()
    s, mean = d(bn.weight) / sigma, d(bn.running_mean)
    z = r16(F.conv2d(xr, w16, None, stride, r // 2))
    u = (z - mean[None, :, None, None]) * s[None, :, None, None] + d(bn.bias)[None, :, None, None]
    if res:
        u = u + d(rs)
    y = r16(u.relu() if relu else u)
    g = torch.where(y > 0, d(dy), torch.zeros_like(y)) if relu else d(dy)
    dz = r16(g * s[None, :, None, None])
    dx = torch.nn.grad.conv2d_input(xr.shape, w16, dz, stride, r // 2)
    r32 = lambda t: t.float().double()                                                 # (the parameter gradients leave as fp32)
    out = dict(y=y, dx=r16(dx + (d(stash) if join else 0)), dw=r32(torch.nn.grad.conv2d_weight(xr, w16.shape, dz, stride, r // 2)),
               dgamma=r32((g * (z - mean[None, :, None, None]) / sigma[None, :, None, None]).sum(dim=(0, 2, 3))), dbeta=r32(g.sum(dim=(0, 2, 3))))
    if res:
        out['dres'] = g
    return out


def _run_layer(pkg, case, conv, bn, x, rs, dy, stash, fold):
    """forward and backward of the layer on the GPU: today's path (fp16 conv, then the BatchNorm pass) or the folded node"""
    n, c, k, r, stride, h, w, res, relu, join = case
    ops = pkg.ops
    for p in (conv.weight, bn.weight, bn.bias):
        p.grad = None
    xr = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
    rr = rs.clone(memory_format=torch.preserve_format).requires_grad_(True) if res else None
    jn = None
    if join:
        jn = ops.GradJoin()
        jn.buf = stash.clone(memory_format=torch.preserve_format)
    if fold:
        assert pkg.ops_frozen.admits_half(xr, conv, bn)
        y = pkg.ops_frozen.conv_bn_half(xr, conv, bn, res=rr, relu=relu, join_take=jn)
        assert type(y.grad_fn).__name__.startswith('HFrozenConvBnFn')
    else:
        assert not pkg.ops_frozen.admits_half(xr, conv, bn)
        y = bn(conv(xr, join_take=jn), res=rr, relu=relu)
    y.backward(dy)
    ops.join_side_stream()
    torch.cuda.synchronize()
    assert jn is None or (jn.buf is None and jn.taken)
    out = dict(y=y.detach(), dx=xr.grad, dw=conv.weight.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad)
    if res:
        out['dres'] = rr.grad
    return {name: t.clone(memory_format=torch.preserve_format) for name, t in out.items()}


@pytest.mark.parametrize('case', LAYERS, ids=_layer_id)
def test_one_layer(pkg, fold_on, case):
    """Because fp16 rounding can flip a ReLU at the switch, the gradients are compared only where |u_ref| > 2^-8 max |u_ref|: the incoming gradient dy of every
    other element is set to zero for the reference and both legs alike (an element's dy reaches every gradient, so leaving elements out of a comparison of sums
    means leaving them out of the sums); at most 8 % of the elements may be left out.  y is compared everywhere."""
    n, c, k, r, stride, h, w, res, relu, join = case
    ops, L = pkg.ops, pkg._lib.lib()
    conv, bn, x, rs, dy, stash = _layer(pkg, case, 100 + c + k + h)
    if relu:
        _, u = _reference(case, conv, bn, x, rs, dy, stash)
        keep = u.abs() > NEAR_SWITCH * u.abs().max()
        left_out = 1.0 - keep.double().mean().item()
        print('%s: %.2f %% of the elements within 2^-8 of the ReLU switch, left out' % (_layer_id(case), 100 * left_out))
        assert left_out <= LEFT_OUT_MOST, left_out
        dy = _half_cl(dy * keep.cuda().to(dy.dtype))
    operands = (conv, bn, x, rs, dy, stash)
    ref, u = _reference(case, *operands)
    stats_before = [t.clone() for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]
    fold_on(False)
    if 256 % (k // 8) == 0:
        off = _run_layer(pkg, case, *operands, fold=False)
    else:
        # 96 channels: today's BatchNorm pass does not take the layer at all (its rule: C / 8 divides 256), so there is no run to measure; the yardstick is
        # the float64 model of today's rounding points on the same data
        with pytest.raises(pkg._lib.P3DError, match='hbn'):
            _run_layer(pkg, case, *operands, fold=False)
        torch.cuda.synchronize()
        off = _today_model(case, *operands)
    fold_on(True)
    on = _run_layer(pkg, case, *operands, fold=True)
    again = _run_layer(pkg, case, *operands, fold=True)
    for a, b in zip(stats_before, (bn.running_mean, bn.running_var, bn.num_batches_tracked)):
        assert torch.equal(a, b)
    # the forward is the inference forward on the plan's own kind-2 image and b', bit for bit; dres is g
    unit = pkg.ops_frozen._unit(conv, bn, pkg.ops_frozen._HUnit)
    plan = unit.plan
    assert plan.generation == 1                                                        # three forwards, nothing written: one fold
    d = unit.desc(tuple(x.shape))
    want_y = torch.empty_like(on['y'])
    pkg._lib.check(L.p3d_hconv2d_fwd_infer(ctypes.byref(d), ops._p(x), ops._p(plan.image(unit)), ops._p(plan.bias(unit)), None, None, ops._p(rs), int(relu),
                                           ops._p(want_y), ops._stream()), 'p3d_hconv2d_fwd_infer')
    torch.cuda.synchronize()
    assert on['y'].is_contiguous(memory_format=CL) and torch.equal(_bits(on['y']), _bits(want_y))
    if res:
        g = torch.where(on['y'] > 0, dy, torch.zeros_like(dy)) if relu else dy
        assert torch.equal(_bits(on['dres']), _bits(g))
    for name in on:
        assert torch.equal(_bits(on[name]), _bits(again[name])), name
        assert torch.isfinite(on[name]).all(), name
    for name in ('y', 'dx', 'dw', 'dgamma', 'dbeta'):
        top = ref[name].abs().max()
        e_off = ((off[name].double().cpu() - ref[name]).abs().max() / top).item()
        e_on = ((on[name].double().cpu() - ref[name]).abs().max() / top).item()
        print('%s %s: today %.3e  folded %.3e  (x %.2f)' % (_layer_id(case), name, e_off, e_on, e_on / max(e_off, 1e-30)))
        assert e_on <= 4 * e_off, (name, e_off, e_on)


def test_backward_after_a_new_fold_raises(pkg, fold_on):
    case = (2, 64, 64, 3, 1, 16, 16, False, True, False)
    conv, bn, x, rs, dy, stash = _layer(pkg, case, 9)
    xr = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
    y = pkg.ops_frozen.conv_bn_half(xr, conv, bn, relu=True)
    unit = pkg.ops_frozen._unit(conv, bn, pkg.ops_frozen._HUnit)
    gen0 = unit.plan.generation
    y2 = pkg.ops_frozen.conv_bn_half(xr, conv, bn, relu=True)                          # a second forward with nothing changed: the same fold
    assert unit.plan.generation == gen0 and torch.equal(y, y2)
    with torch.no_grad():
        bn.weight.mul_(2.0)                                                            # an in-place write: the next forward folds again
    y3 = pkg.ops_frozen.conv_bn_half(xr, conv, bn, relu=True)
    assert unit.plan.generation == gen0 + 1 and not torch.equal(y, y3)
    with pytest.raises(pkg._lib.P3DError, match='fold'):
        y.backward(dy)
    y3.backward(dy)                                                                    # the forward on the current fold is fine
    pkg.ops.join_side_stream()
    torch.cuda.synchronize()
    assert torch.isfinite(xr.grad).all() and torch.isfinite(conv.weight.grad).all()
    pkg.ops.weights_changed()                                                          # parameters written behind torch's back: stale too
    pkg.ops_frozen.conv_bn_half(xr, conv, bn, relu=True)
    assert unit.plan.generation == gen0 + 2


def _frozen_block(pkg, seed, refuse_first=False):
    gen = torch.Generator(device='cuda').manual_seed(seed)
    blk = pkg._trunk.BasicBlock(64, 64).cuda().train()
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.eval()
                m.running_mean.copy_(torch.randn(64, device='cuda', generator=gen) * 0.5)
                m.running_var.copy_(torch.rand(64, device='cuda', generator=gen) * 1.5 + 0.5)
                m.weight.copy_(torch.rand(64, device='cuda', generator=gen) + 0.5)
                m.bias.copy_(torch.randn(64, device='cuda', generator=gen) * 0.3)
    if refuse_first:
        blk.bn1.train()                                                                # batch statistics: admits_half refuses the first pair, the second folds
    return blk, gen


def test_refused_first_layer_joins_a_folded_closing_layer(pkg, fold_on):
    """A block whose first pair is refused (its BatchNorm computes batch statistics) and whose closing pair folds, under FlatAdam sinks: the folded layer stashes
    g -- which its weight gradient still reads on the second stream -- in the block's join, and the unfolded fp16 convolution accumulates its data gradient
    into it behind the event left there.  Five runs are bit-equal to each other and to a run with every launch on one stream (where nothing can overtake
    anything), and the output is within fp16 rounding of the unfolded block's: y_on is rounded once, y_off after a rounded z, and the two weight images round
    w' and w apart -- a handful of 2^-11 relative roundings of values no larger than a few times the largest output, held at 1e-2 of it.  (The gradients of the
    two legs are not compared: a ReLU element that the roundings flip carries its whole dy into the block input's gradient.)"""
    ops = pkg.ops
    blk, gen = _frozen_block(pkg, 21, refuse_first=True)
    opt = pkg.optim.FlatAdam(list(blk.named_parameters()), 1e-3)
    pkg.ops_half.refresh_weights(blk, opt.flat_p)
    x = _half_cl(torch.randn(8, 64, 32, 32, device='cuda', generator=gen))
    dy = _half_cl(torch.randn(8, 64, 32, 32, device='cuda', generator=gen))
    state = {k: v.clone() for k, v in blk.state_dict().items()}

    def run():
        blk.load_state_dict(state)                                                     # (bn1 moves its running statistics)
        opt.zero_grad()
        xg = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
        y = blk(xg)
        y.backward(dy)
        ops.check_joins()
        ops.join_side_stream()
        torch.cuda.synchronize()
        return dict({n: p.grad.detach().clone() for n, p in blk.named_parameters()}, x=xg.grad.clone(memory_format=torch.preserve_format), y=y.detach().clone())

    fold_on(False)
    off = run()
    fold_on(True)
    assert ops.WGRAD_STREAM
    ops.WGRAD_STREAM = False
    try:
        one_stream = run()
    finally:
        ops.WGRAD_STREAM = True
    runs = [run() for _ in range(5)]
    assert '_hfrozen_unit' in blk.conv2.__dict__ and '_hfrozen_unit' not in blk.conv1.__dict__ and x.device in ops._side_streams
    for name in one_stream:
        assert torch.isfinite(one_stream[name]).all(), name
        for other in runs:
            assert torch.equal(_bits(one_stream[name]), _bits(other[name])), name
    err = (runs[0]['y'].float() - off['y'].float()).abs().max().item() / off['y'].float().abs().max().item()
    print('refused first layer: y folded against unfolded %.3e of the largest value' % err)
    assert err <= 1e-2, err


def test_refused_block_runs_as_ever(pkg, fold_on):
    """a block whose BatchNorms all compute batch statistics: bit-equal with the switch on and off, nothing planned for it"""
    blk, gen = _frozen_block(pkg, 3)
    for m in blk.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.train()
    pkg.ops_half.refresh_weights(blk)
    x = _half_cl(torch.randn(2, 64, 17, 19, device='cuda', generator=gen))
    dy = _half_cl(torch.randn(2, 64, 17, 19, device='cuda', generator=gen))
    state = {k: v.clone() for k, v in blk.state_dict().items()}
    res = {}
    for on in (False, True):
        fold_on(on)
        blk.load_state_dict(state)
        blk.zero_grad(set_to_none=True)
        xr = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
        y = blk(xr)
        y.backward(dy)
        pkg.ops.join_side_stream()
        torch.cuda.synchronize()
        res[on] = [y.detach().clone(), xr.grad.clone()] + [p.grad.clone() for p in blk.parameters()]
    assert not any('_hfrozen_unit' in m.__dict__ for m in blk.modules())
    for a, b in zip(res[False], res[True]):
        assert torch.equal(a, b)


# ---- 4. a whole network ---------------------------------------------------------------------------------------------------------------------------
def _network(pkg, side, half):
    flags = ['-model', 'resnet18', '-suffix', 't', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1', '-num_joints', '17',
             '-side_in', str(side)] + (['-half_acc'] if half else [])
    args = pkg.opts.parse(flags)
    torch.manual_seed(0)
    model, _ = pkg.depth_main.create_model(args)
    det = pkg.synth.det_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 0)
    rng = np.random.default_rng(7)
    for key in det:                                                                    # running statistics that make the fold matter
        if key.endswith('running_mean'):
            det[key] = (0.1 * rng.standard_normal(det[key].shape)).astype(np.float32)
        elif key.endswith('running_var'):
            det[key] = rng.uniform(0.5, 2.0, det[key].shape).astype(np.float32)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in det.items()})
    model = model.cuda().train()
    model.freeze_batchnorm()
    tr = pkg.depth_train.Trainer(args, model, pkg.utils.get_info())
    tr.verbose = False
    tr.adapt_learn_rate(1)
    return model, tr


def _refused_pairs(pkg, model, batch):
    """the BatchNorms of the dense-block pairs whose descriptor p3d_hconv2d_fwd_infer refuses at the shapes of this batch, or whose K is outside the rule: asked
    of the library directly, on a forward with the switch off"""
    L = pkg._lib.lib()
    shapes, hooks = {}, []
    for m in model.modules():
        if isinstance(m, pkg.nn.Conv2d):
            hooks.append(m.register_forward_hook(lambda mod, inp, out: shapes.__setitem__(id(mod), tuple(inp[0].shape))))
    before = pkg.ops.frozen_fold_half(False)
    try:
        model(batch[0])
    finally:
        pkg.ops.frozen_fold_half(before)
    for h in hooks:
        h.remove()
    refused, pairs_seen = [], 0
    for blk in model.modules():
        if isinstance(blk, pkg._trunk._ResidualBlock) and not blk.partial:
            pairs = [(getattr(blk, c), getattr(blk, b)) for c, b in blk._chain] + ([(blk.downsample[0], blk.downsample[1])] if blk.downsample is not None else [])
            for conv, bn in pairs:
                pairs_seen += 1
                k, c, r, _ = conv.weight.shape
                xs = shapes[id(conv)]
                d = pkg.ops._desc(xs, (k, xs[1], r, r), conv.stride[0], conv.padding[0], conv.dilation[0])
                if not (k % 8 == 0 and 8 <= k <= 2048 and c >= 8 and L.p3d_hconv2d_fwd_infer_supported(ctypes.byref(d))):
                    refused.append(bn)
    assert pairs_seen == 8 * 2 + 3
    return refused


@pytest.mark.parametrize('side', [64, 65])
def test_whole_network(pkg, fold_on, side):
    ops = pkg.ops
    c, d_, tc, tv = pkg.synth.make_batch(2, side=side, rank=0, step=0)
    batch = tuple(torch.from_numpy(v).cuda() for v in (c, d_, tc, tv))

    def leg(half, on):
        """one training step from the same parameters: (loss, gradients with the loss scale divided out, model)"""
        fold_on(on)
        model, tr = _network(pkg, side, half)
        refused = _refused_pairs(pkg, model, batch) if half else []
        before = {n: b.detach().clone() for n, b in model.named_buffers()}
        calls, keep = [], pkg.ops_half.batch_norm_act

        def counted(x, gamma, *a, **kw):
            calls.append(gamma.data_ptr())
            return keep(x, gamma, *a, **kw)

        pkg.ops_half.batch_norm_act = counted
        try:
            loss = tr.train_step(*batch)
        finally:
            pkg.ops_half.batch_norm_act = keep
        ops.join_side_stream()
        torch.cuda.synchronize()
        scale = tr.grad_scaling if half else 1.0
        grads = {n: (p.grad.detach() / scale).clone() for n, p in zip(tr.list_names, tr.list_params)}
        for n, b in model.named_buffers():                                             # running statistics and num_batches_tracked: bit-unchanged
            assert torch.equal(before[n], b), n
        if half:
            assert tr.optimizer.steps_taken() == 1 and tr.skipped_steps == 0
            # exactly the stem, any Fusion BatchNorm and the refused pairs still call ops_half.batch_norm_act, once each
            bns = {m.weight.data_ptr(): m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)}
            dense = set()
            for blk in model.modules():
                if isinstance(blk, pkg._trunk._ResidualBlock) and not blk.partial:
                    dense |= {getattr(blk, b).weight.data_ptr() for _, b in blk._chain} | ({blk.downsample[1].weight.data_ptr()} if blk.downsample is not None else set())
            folded = (dense - {bn.weight.data_ptr() for bn in refused}) if on else set()
            assert sorted(calls) == sorted(set(bns) - folded), (len(calls), len(bns), len(folded))
            if on:
                assert len(folded) > 0 and model.__dict__['_hfrozen_fold']['plan'].generation == 1      # one fold for the step
            else:
                assert '_hfrozen_fold' not in model.__dict__
        return float(loss), grads, model

    l32, g32, _ = leg(False, False)
    l_off, g_off, _ = leg(True, False)
    l_on, g_on, _ = leg(True, True)
    l_on2, g_on2, _ = leg(True, True)
    l_off2, g_off2, _ = leg(True, False)
    assert l_on == l_on2 and all(torch.equal(g_on[n], g_on2[n]) for n in g_on)         # two steps with the switch on: bit-equal
    assert l_off == l_off2 and all(torch.equal(g_off[n], g_off2[n]) for n in g_off)    # the switch off: the same step before and after it was toggled

    def figures(loss, grads):
        rel = {n: ((grads[n].double() - g32[n].double()).abs().max() / g32[n].double().abs().max().clamp_min(1e-30)).item() for n in g32}
        rel['loss'] = abs(loss - l32) / abs(l32)
        v = sorted(rel.values())
        worst = max(rel, key=rel.get)
        return v[len(v) // 2], rel[worst], worst, rel['loss']

    m_off, w_off, n_off, e_off = figures(l_off, g_off)
    m_on, w_on, n_on, e_on = figures(l_on, g_on)
    print('R18 side %d, difference from the fp32 step / largest element: off median %.3e worst %.3e (%s) loss %.3e | on median %.3e worst %.3e (%s) loss %.3e'
          % (side, m_off, w_off, n_off, e_off, m_on, w_on, n_on, e_on))
    assert all(torch.isfinite(g).all() for g in g_on.values())
    assert m_on <= 2 * m_off, (m_on, m_off)
    assert w_on <= 2 * w_off, (w_on, w_off)


# ---- 5. distillation ------------------------------------------------------------------------------------------------------------------------------
def test_distillation_step(pkg, fold_on):
    """one -do_teach -do_freeze -do_fusion -half_acc iteration with the switch on against the fp32 leg: the set-up and tolerances of
    tests/test_half_gpu.py::test_half_frozen_distillation_step"""
    flags = ['-model', 'resnet18', '-suffix', 't', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1', '-num_joints', '17',
             '-side_in', '128', '-do_teach', '-do_fusion', '-do_freeze']
    records = []
    for extra in ([], ['-half_acc']):
        args = pkg.opts.parse(flags + extra)
        student, teacher = pkg.depthnet.resnet18(args, False), pkg.fusionnet.resnet18(args, False)
        for net, seed in ((student, 0), (teacher, 1)):
            det = pkg.synth.det_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed)
            net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in det.items()})
        trainer = pkg.depth_train.Trainer(args, student.cuda(), pkg.utils.get_info())
        trainer.set_teacher(teacher.cuda())
        trainer.verbose = False
        mean0 = student.bn1.running_mean.clone()
        c, d, tc, tv = pkg.synth.make_batch(2, side=128, rank=11, step=0)
        att = np.ones((2, 1, 8, 8), np.float32)
        seen, keep = [], pkg.ops_frozen.conv_bn_half

        def counted(*a, **kw):
            seen.append(1)
            return keep(*a, **kw)

        pkg.ops_frozen.conv_bn_half = counted
        try:
            records.append(trainer.train(1, [tuple(torch.from_numpy(v) for v in (c, d, tc, tv, att))]))
        finally:
            pkg.ops_frozen.conv_bn_half = keep
        torch.cuda.synchronize()
        assert torch.equal(student.bn1.running_mean, mean0)
        if extra:
            assert trainer.optimizer.steps_taken() == 1 and trainer.skipped_steps == 0          # one optimizer step taken, no overflow skip
            assert len(seen) == 8 * 2 + 3                                              # every dense-block pair of the student ran folded, once
            assert student.__dict__['_hfrozen_fold']['plan'].generation == 1
            with pytest.raises(pkg._lib.P3DError, match='frozen_fold_half'):
                pkg.graphed.GraphedStep(trainer)
        else:
            assert not seen
    print('distillation: cam fp32 %.8e half+fold %.8e  dist fp32 %.8e half+fold %.8e'
          % (records[0]['cam_train_loss'], records[1]['cam_train_loss'], records[0]['dist_train_loss'], records[1]['dist_train_loss']))
    assert records[1]['cam_train_loss'] == pytest.approx(records[0]['cam_train_loss'], rel=5e-3)
    assert records[1]['dist_train_loss'] == pytest.approx(records[0]['dist_train_loss'], rel=2e-2)
