"""Training frozen-BatchNorm layers on folded convolutions (ops.frozen_fold, ops_frozen.py, csrc/p3d_frozen.hip), on the GPU: the two new kernels on fenced
buffers, one layer forward and backward against float64 and beside today's path (conv, then the eval-mode BatchNorm pass), whole networks, and distillation.

Bounds.  y, dx and dw: the project's x3 bound, 4e-6 of the largest reference value, and 4 x the error of today's path on the same data.
dgamma and dbeta: relative to the sum of their absolute terms (sum |w * raw| / sigma + |mean| * sum |g| / sigma, and sum |g|), GRAD_TOL = 4 x the worst error of
today's p3d_bn_eval_bwd over the cases of section 3 as measured on an MI355X (profiles/train_frozen_fold.md); it was never taken from the new kernels' output.
The sums of the mask pass end in one rounding to fp32 of an fp64 sum, 2^-24 of |sum| <= sum |g|; the finish kernel's dgamma in three (the fp32 square root, its
own result, and the fp32 `sums` it is handed counts among the inputs): 4 * 2^-24 of the absolute terms with the fp64 accumulation's own error beside it."""
import ctypes

import numpy as np
import pytest
import torch

import fenced

pytestmark = pytest.mark.gpu

TOL = 4e-6
GRAD_TOL = dict(dgamma=4 * 1.227e-7, dbeta=4 * 5.062e-8)      # 4 x the worst p3d_bn_eval_bwd figures of profiles/train_frozen_fold.md, relative to the absolute-term sums
F = torch.nn.functional


@pytest.fixture
def fold_on(pkg):
    """the switch on for the test body; what it found restored afterwards, with x3_any"""
    before = pkg.ops.frozen_fold(True)
    any_before = pkg.ops.x3_any(False)
    try:
        yield pkg.ops.frozen_fold
    finally:
        pkg.ops.frozen_fold(before)
        pkg.ops.x3_any(any_before)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. the mask pass -----------------------------------------------------------------------------------------------------------------------------
MASK_SHAPES = [(1, 16, 4), (3, 32, 17 * 19), (2, 96, 33 * 33), (5, 2051, 7)]          # the last: more channels than one grid pass, rows at every 16-B phase


def _mask_data(n, k, hw, seed):
    gen = torch.Generator(device='cuda').manual_seed(seed)
    dy = torch.randn(n, k, hw, device='cuda', generator=gen)
    y = torch.randn(n, k, hw, device='cuda', generator=gen).clamp_min(0)               # half of it exact zeros, as a ReLU leaves them
    y.view(-1)[::7] = -0.0
    y.view(-1)[3::11] = 0.0
    y.view(-1)[5::13] = -1.5                                                           # (never behind a ReLU; the kernel tests y > 0 all the same)
    return dy, y


@pytest.mark.parametrize('shape', MASK_SHAPES, ids=lambda s: '%dx%dx%d' % s)
@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'plain'])
def test_mask_pass(pkg, shape, relu):
    ops, L = pkg.ops, pkg._lib.lib()
    n, k, hw = shape
    dy0, y0 = _mask_data(n, k, hw, 11 + hw)
    fences = []

    def operand(src):
        t, f = fenced.fenced_like(src.shape, torch.float32, 4096, sentinel=0xFF)       # NaN bands: a fetch beyond the tensor would bring one into the sums
        t.copy_(src)
        fences.append(f)
        return t

    def result(shape_):
        t, f = fenced.fenced_like(shape_, torch.float32, 4096)
        fences.append(f)
        return t

    dy, y = operand(dy0), operand(y0)
    nb = L.p3d_frozen_grad_mask_workspace_bytes(n, k, hw)
    want_g = torch.where(y0 > 0, dy0, torch.zeros_like(dy0)) if relu else dy0
    want = want_g.double().sum(dim=(0, 2))
    scale = want_g.double().abs().sum(dim=(0, 2))
    runs = []
    for _ in range(2):
        g, sums = result(shape), result((k,))
        ws = fenced.Fence(nb, 65536, 'cuda')
        fences.append(ws)
        pkg._lib.check(L.p3d_frozen_grad_mask(ops._p(dy), ops._p(y) if relu else None, ops._p(g) if relu else None, ops._p(sums), n, k, hw, ops._p(ws.view), nb,
                                              ops._stream()), 'p3d_frozen_grad_mask')
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
    print('mask %s relu %d: sums err / sum|g| %.3e' % (shape, relu, err))
    assert torch.isfinite(sums).all() and err <= 1e-7, err
    assert torch.equal(_bits(sums), _bits(sums2)) and (not relu or torch.equal(_bits(g), _bits(g2)))
    assert torch.equal(dy, dy0) and torch.equal(_bits(y), _bits(y0))


def test_mask_pass_off_the_16_byte_line(pkg):
    """base pointers one float behind a 16-B line: everything goes element by element"""
    ops, L = pkg.ops, pkg._lib.lib()
    n, k, hw = 3, 32, 17 * 19
    dy0, y0 = _mask_data(n, k, hw, 5)
    hold = [torch.full((n * k * hw + 2,), float('nan'), device='cuda') for _ in range(3)]
    dy, y, g = (h[1:-1].view(n, k, hw) for h in hold)
    dy.copy_(dy0)
    y.copy_(y0)
    assert dy.data_ptr() % 16 == 4
    sums = torch.empty(k, device='cuda')
    nb = L.p3d_frozen_grad_mask_workspace_bytes(n, k, hw)
    ws = ops.workspace(dy.device, nb)
    pkg._lib.check(L.p3d_frozen_grad_mask(ops._p(dy), ops._p(y), ops._p(g), ops._p(sums), n, k, hw, ops._p(ws), nb, ops._stream()), 'p3d_frozen_grad_mask')
    want_g = torch.where(y0 > 0, dy0, torch.zeros_like(dy0))
    assert torch.equal(_bits(g), _bits(want_g))
    assert all(bool(torch.isnan(h[0])) and bool(torch.isnan(h[-1])) for h in hold)
    scale = want_g.double().abs().sum(dim=(0, 2))
    assert ((sums.double() - want_g.double().sum(dim=(0, 2))).abs() / scale).max().item() <= 1e-7


# ---- 2. the finish kernel -------------------------------------------------------------------------------------------------------------------------
FINISH_SHAPES = [(32, 32), (96, 128 * 9), (48, 2048 * 9), (33, 17)]                    # (48: the 272 rows of that layer cut for time)


def _fold_scale(pkg, gamma, var, eps):
    """s as the fold computes it, read back through bias_out: b' = beta - mean * s = s for beta = 0, mean = -1"""
    ops = pkg.ops
    k = gamma.numel()
    w = torch.ones(k, 1, 1, 1, device='cuda')
    out, s = torch.empty(k, device='cuda'), torch.empty(k, device='cuda')
    beta, mean = torch.zeros(k, device='cuda'), -torch.ones(k, device='cuda')
    j = pkg._lib.FoldJob()
    j.w, j.conv_bias, j.gamma, j.beta, j.mean, j.var = w.data_ptr(), None, gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), var.data_ptr()
    j.out, j.bias_out, j.K, j.C, j.RS, j.c_offset, j.c_total, j.kind, j.eps = out.data_ptr(), s.data_ptr(), k, 1, 1, 0, 1, 1, eps
    table = torch.frombuffer(bytearray(j), dtype=torch.uint8).cuda()
    pkg._lib.check(pkg._lib.lib().p3d_fx_fold_bn_images(ops._p(table), 1, 1, ops._stream()), 'p3d_fx_fold_bn_images')
    torch.cuda.synchronize()
    return s


@pytest.mark.parametrize('shape', FINISH_SHAPES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('accumulate', [0, 1])
def test_finish_kernel(pkg, shape, accumulate):
    ops, L = pkg.ops, pkg._lib.lib()
    k, crs = shape
    eps = 1e-5
    gen = torch.Generator(device='cuda').manual_seed(k + crs + accumulate)
    rnd = lambda *s: torch.randn(*s, device='cuda', generator=gen)
    raw0, w0 = rnd(k, crs), rnd(k, crs) / crs ** 0.5
    gamma, mean, sums = torch.rand(k, device='cuda', generator=gen) + 0.5, rnd(k), rnd(k) * 30
    var = torch.rand(k, device='cuda', generator=gen) * 1.5 + 0.5
    prior = (rnd(k, crs), rnd(k), rnd(k))
    with fenced.FencedAllocations() as fa:
        raw, w = torch.empty_like(raw0), torch.empty_like(w0)
        raw.copy_(raw0)
        w.copy_(w0)
        dw, dgamma, dbeta = torch.empty(k, crs, device='cuda'), torch.empty(k, device='cuda'), torch.empty(k, device='cuda')
    if accumulate:
        for t, p in zip((dw, dgamma, dbeta), prior):
            t.copy_(p)
    pkg._lib.check(L.p3d_frozen_wgrad_finish(ops._p(raw), ops._p(w), ops._p(gamma), ops._p(mean), ops._p(var), eps, ops._p(sums), ops._p(dw), ops._p(dgamma),
                                             ops._p(dbeta), k, crs, accumulate, ops._stream()), 'p3d_frozen_wgrad_finish')
    torch.cuda.synchronize()
    fa.check()
    s = _fold_scale(pkg, gamma, var, eps)
    assert torch.equal(raw, raw0) and torch.equal(w, w0)
    prod = s[:, None] * raw0                                                           # one fp32 product per element, as the kernel's
    if not accumulate:
        ulps = (_bits(dw).long() - _bits(prod).long()).abs().max().item()
        assert ulps <= 1, ulps
        assert torch.equal(_bits(dbeta), _bits(sums))
    else:
        want = prior[0].double() + s.double()[:, None] * raw0.double()
        room = 2.0 ** -23 * (prior[0].double().abs() + prod.double().abs())
        assert bool(((dw.double() - want).abs() <= room).all())
        assert bool(((dbeta.double() - (prior[2].double() + sums.double())).abs() <= 2.0 ** -24 * (prior[2].abs() + sums.abs()).double()).all())
    sigma = (var.double() + eps).sqrt()
    inner, inner_abs = (w0.double() * raw0.double()).sum(1), (w0.double() * raw0.double()).abs().sum(1)
    want = (inner - mean.double() * sums.double()) / sigma
    terms = (inner_abs + mean.double().abs() * sums.double().abs()) / sigma
    got = dgamma.double() - (prior[1].double() if accumulate else 0)
    err = ((got - want).abs() / terms).max().item()
    print('finish %s accumulate %d: dgamma err / terms %.3e' % (shape, accumulate, err))
    bound = 4 * 2.0 ** -24
    if accumulate:                                                                     # (the sum with what was there is rounded once more)
        assert bool(((got - want).abs() <= bound * terms + 2.0 ** -24 * (prior[1].double().abs() + want.abs())).all())
    else:
        assert err <= bound, err


# ---- 3. one layer ---------------------------------------------------------------------------------------------------------------------------------
# n, c, k, r, stride, dil, h, w, res, relu, join
LAYERS = [(2, 64, 64, 3, 1, 1, 16, 16, True, True, False), (2, 64, 64, 3, 1, 1, 16, 16, False, True, False), (2, 64, 64, 3, 1, 1, 16, 16, True, False, False),
          (2, 64, 64, 3, 1, 1, 16, 16, False, False, False),
          (3, 128, 128, 3, 1, 1, 17, 19, True, True, False), (3, 128, 256, 1, 2, 1, 17, 19, False, False, False), (2, 64, 96, 3, 2, 1, 33, 33, False, True, False),
          (2, 256, 64, 1, 1, 1, 16, 16, False, True, True)]


def _layer_id(v):
    n, c, k, r, stride, dil, h, w, res, relu, join = v
    return 'n%d_%dto%d_%dx%d_s%d_%dx%d%s%s%s' % (n, c, k, r, r, stride, h, w, '_res' if res else '', '_relu' if relu else '', '_join' if join else '')


def _layer(pkg, case, seed):
    n, c, k, r, stride, dil, h, w, res, relu, join = case
    gen = torch.Generator(device='cuda').manual_seed(seed)
    conv = pkg.nn.Conv2d(c, k, kernel_size=r, stride=stride, padding=dil * (r // 2), dilation=dil, bias=False).cuda()
    bn = pkg.nn.BatchNorm2d(k).cuda().eval()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, device='cuda', generator=gen) / (c * r * r) ** 0.5)
        bn.running_mean.copy_(torch.randn(k, device='cuda', generator=gen))
        bn.running_var.copy_(torch.rand(k, device='cuda', generator=gen) * 1.5 + 0.5)
        bn.weight.copy_(torch.rand(k, device='cuda', generator=gen) + 0.5)
        bn.bias.copy_(torch.randn(k, device='cuda', generator=gen))
    x = torch.randn(n, c, h, w, device='cuda', generator=gen)
    ho, wo = ((v + 2 * dil * (r // 2) - dil * (r - 1) - 1) // stride + 1 for v in (h, w))
    rs = torch.randn(n, k, ho, wo, device='cuda', generator=gen) if res else None
    dy = torch.randn(n, k, ho, wo, device='cuda', generator=gen)
    stash = torch.randn(n, c, h, w, device='cuda', generator=gen) if join else None
    return conv, bn, x, rs, dy, stash


def _reference(case, conv, bn, x, rs, dy, stash):
    """float64 on the CPU: conv -> eval BatchNorm -> + res -> ReLU and its autograd; also the absolute-term sums dgamma and dbeta are measured against"""
    n, c, k, r, stride, dil, h, w, res, relu, join = case
    d = lambda t: t.detach().double().cpu()
    xr, wr = d(x).requires_grad_(True), d(conv.weight).requires_grad_(True)
    gm, bt = d(bn.weight).requires_grad_(True), d(bn.bias).requires_grad_(True)
    rr = d(rs).requires_grad_(True) if res else None
    z = F.conv2d(xr, wr, None, stride, dil * (r // 2), dil)
    sigma = (d(bn.running_var) + bn.eps).sqrt()
    mean = d(bn.running_mean)
    u = (z - mean[None, :, None, None]) / sigma[None, :, None, None] * gm[None, :, None, None] + bt[None, :, None, None]
    if res:
        u = u + rr
    y = u.relu() if relu else u
    y.backward(d(dy))
    g = torch.where(y.detach() > 0, d(dy), torch.zeros_like(y.detach())) if relu else d(dy)
    raw = wr.grad * (sigma / gm.detach())[:, None, None, None]                       # dw = s * raw
    gsum = g.abs().sum(dim=(0, 2, 3))
    terms = dict(dgamma=((wr.detach() * raw).abs().sum(dim=(1, 2, 3)) + mean.abs() * gsum) / sigma, dbeta=gsum)
    out = dict(y=y.detach(), dx=xr.grad + (d(stash) if join else 0), dw=wr.grad, dgamma=gm.grad, dbeta=bt.grad)
    if res:
        out['dres'] = rr.grad
    return out, terms


def _run_layer(pkg, case, conv, bn, x, rs, dy, stash, fold):
    """forward and backward of the layer on the GPU: today's path (conv, then the BatchNorm pass) or the folded node"""
    n, c, k, r, stride, dil, h, w, res, relu, join = case
    ops = pkg.ops
    for p in (conv.weight, bn.weight, bn.bias):
        p.grad = None
    xr = x.clone().requires_grad_(True)
    rr = rs.clone().requires_grad_(True) if res else None
    jn = None
    if join:
        jn = ops.GradJoin()
        jn.buf = stash.clone()
    if fold:
        assert pkg.ops_frozen.admits(xr, conv, bn)
        y = pkg.ops_frozen.conv_bn(xr, conv, bn, res=rr, relu=relu, join_take=jn)
    else:
        y = bn(conv(xr, join_take=jn), res=rr, relu=relu)
    y.backward(dy)
    ops.join_side_stream()
    torch.cuda.synchronize()
    assert jn is None or (jn.buf is None and jn.taken)
    out = dict(y=y.detach(), dx=xr.grad, dw=conv.weight.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad)
    if res:
        out['dres'] = rr.grad
    return {name: t.clone() for name, t in out.items()}


# every ragged case with ops.x3_any off and on (it routes their gradients); at aligned maps the switch changes nothing
LAYER_RUNS = [(case, False) for case in LAYERS] + [(case, True) for case in LAYERS if case[7] % 4]


@pytest.mark.parametrize('case,x3_any', LAYER_RUNS, ids=lambda v: _layer_id(v) if isinstance(v, tuple) else ('x3any' if v else 'plain'))
def test_one_layer(pkg, fold_on, case, x3_any):
    n, c, k, r, stride, dil, h, w, res, relu, join = case
    ops = pkg.ops
    ops.x3_any(x3_any)
    operands = _layer(pkg, case, 100 + c + k + h)
    conv, bn, x, rs, dy, stash = operands
    ref, terms = _reference(case, *operands)
    stats_before = [t.clone() for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]
    fold_on(False)
    off = _run_layer(pkg, case, *operands, fold=False)
    fold_on(True)
    on = _run_layer(pkg, case, *operands, fold=True)
    again = _run_layer(pkg, case, *operands, fold=True)
    for a, b in zip(stats_before, (bn.running_mean, bn.running_var, bn.num_batches_tracked)):
        assert torch.equal(a, b)
    # the forward is the inference fold's, bit for bit; dres is g
    folded = pkg.infer.FoldedConv(conv, bn, any_size=True)(x, rs, relu)
    assert torch.equal(_bits(on['y']), _bits(folded))
    if res:
        g = torch.where(on['y'] > 0, dy, torch.zeros_like(dy)) if relu else dy
        assert torch.equal(_bits(on['dres']), _bits(g))
    for name in on:
        assert torch.equal(_bits(on[name]), _bits(again[name])), name
        assert torch.isfinite(on[name]).all(), name
    for name in ('y', 'dx', 'dw'):
        top = ref[name].abs().max()
        e_off = ((off[name].double().cpu() - ref[name]).abs().max() / top).item()
        e_on = ((on[name].double().cpu() - ref[name]).abs().max() / top).item()
        print('%s %s %s: today %.3e  folded %.3e' % (_layer_id(case), 'x3any' if x3_any else '-', name, e_off, e_on))
        assert e_on <= TOL and e_on <= 4 * e_off, (name, e_off, e_on)
    for name in ('dgamma', 'dbeta'):
        e_off = ((off[name].double().cpu() - ref[name]).abs() / terms[name].clamp_min(1e-30)).max().item()      # (a channel the ReLU closes: 0 / tiny)
        e_on = ((on[name].double().cpu() - ref[name]).abs() / terms[name].clamp_min(1e-30)).max().item()
        print('%s %s %s: today %.3e  folded %.3e' % (_layer_id(case), 'x3any' if x3_any else '-', name, e_off, e_on))
        assert e_on <= GRAD_TOL[name], (name, e_off, e_on)


def test_refused_layer_runs_as_ever(pkg, fold_on):
    """a block of 24-channel layers (the queries refuse C = 24): bit-equal with the switch on and off, in the output and every gradient"""
    gen = torch.Generator(device='cuda').manual_seed(3)
    blk = pkg._trunk.BasicBlock(24, 24).cuda()
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(24, device='cuda', generator=gen))
                m.running_var.copy_(torch.rand(24, device='cuda', generator=gen) + 0.5)
    blk.train()
    for m in blk.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eval()
    x = torch.randn(2, 24, 17, 19, device='cuda', generator=gen)
    dy = torch.randn(2, 24, 17, 19, device='cuda', generator=gen)
    res = {}
    for on in (False, True):
        fold_on(on)
        blk.zero_grad(set_to_none=True)
        xr = x.clone().requires_grad_(True)
        y = blk(xr)
        y.backward(dy)
        pkg.ops.join_side_stream()
        torch.cuda.synchronize()
        res[on] = [y.detach().clone(), xr.grad.clone()] + [p.grad.clone() for p in blk.parameters()]
    assert not any('_frozen_unit' in m.__dict__ for m in blk.modules())             # nothing was planned for it
    for a, b in zip(res[False], res[True]):
        assert torch.equal(_bits(a), _bits(b))


def test_backward_after_a_new_fold_raises(pkg, fold_on):
    case = (2, 64, 64, 3, 1, 1, 16, 16, False, True, False)
    conv, bn, x, rs, dy, stash = _layer(pkg, case, 9)
    xr = x.clone().requires_grad_(True)
    y = pkg.ops_frozen.conv_bn(xr, conv, bn, relu=True)
    unit = pkg.ops_frozen._unit(conv, bn)
    gen0 = unit.plan.generation
    y2 = pkg.ops_frozen.conv_bn(xr, conv, bn, relu=True)                               # a second forward with nothing changed: the same fold
    assert unit.plan.generation == gen0 and torch.equal(y, y2)
    with torch.no_grad():
        bn.weight.mul_(2.0)                                                            # an in-place write: the next forward folds again
    y3 = pkg.ops_frozen.conv_bn(xr, conv, bn, relu=True)
    assert unit.plan.generation == gen0 + 1 and not torch.equal(y, y3)
    with pytest.raises(pkg._lib.P3DError, match='fold'):
        y.backward(dy)
    y3.backward(dy)                                                                    # the forward on the current fold is fine
    pkg.ops.join_side_stream()
    torch.cuda.synchronize()
    assert torch.isfinite(xr.grad).all() and torch.isfinite(conv.weight.grad).all()


# ---- 4. whole networks ----------------------------------------------------------------------------------------------------------------------------
def _network(pkg, model_name, fusion, side, trainer=True):
    flags = ['-model', model_name, '-suffix', 't', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1', '-num_joints', '17',
             '-side_in', str(side)] + (['-do_fusion'] if fusion else [])
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
    tr = None
    if trainer:
        tr = pkg.depth_train.Trainer(args, model, pkg.utils.get_info())
        tr.verbose = False
        tr.adapt_learn_rate(1)
    return model, tr


def _batch(pkg, side, fusion, rank=0):
    c, d, tc, tv = pkg.synth.make_batch(2, side=side, rank=rank, step=0)
    return tuple(torch.from_numpy(v).cuda() for v in (c, d, tc, tv))


def _step(pkg, model, tr, batch, fusion, calls=None, relus=None):
    """one training step (FlatAdam sinks) or, without a trainer, forward + backward of a fixed functional of the outputs (autograd's own gradients);
    returns (loss, the sum of the loss's absolute terms, parameter gradients, buffers afterwards).  calls: receives the gamma of every ops.batch_norm_act call;
    relus: receives the output of every BatchNorm layer that ends in a ReLU, folded or not, by the BatchNorm's name."""
    ops = pkg.ops
    keep, keep_fold = ops.batch_norm_act, pkg.ops_frozen.conv_bn
    names = {id(m): n for n, m in model.named_modules()}
    hooks = []
    if calls is not None:
        def counted(x, gamma, *a, **kw):
            calls.append(gamma.data_ptr())
            return keep(x, gamma, *a, **kw)
        ops.batch_norm_act = counted
    if relus is not None:
        def folded(x, conv, bn, *a, **kw):
            y = keep_fold(x, conv, bn, *a, **kw)
            if kw.get('relu'):
                relus[names[id(bn)]] = y.detach()
            return y
        pkg.ops_frozen.conv_bn = folded
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                hooks.append(m.register_forward_hook(lambda mod, args, kw, out: relus.__setitem__(names[id(mod)], out.detach()) if kw.get('relu') else None,
                                                     with_kwargs=True))
    try:
        if tr is not None:
            loss = tr.train_step(*batch)
            scale = abs(float(loss))
            grads = {n: p.grad.detach().clone() for n, p in zip(tr.list_names, tr.list_params)}
        else:
            model.zero_grad(set_to_none=True)
            z, feat = model(batch[0], batch[1]) if fusion else model(batch[0])
            gen = torch.Generator(device='cuda').manual_seed(1)
            terms = [z * torch.randn(z.shape, device='cuda', generator=gen), feat * torch.randn(feat.shape, device='cuda', generator=gen)]
            loss = terms[0].sum() + terms[1].sum()
            scale = float(terms[0].detach().abs().sum() + terms[1].detach().abs().sum())
            loss.backward()
            ops.check_joins()
            grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    finally:
        ops.batch_norm_act, pkg.ops_frozen.conv_bn = keep, keep_fold
        for h in hooks:
            h.remove()
    ops.join_side_stream()
    torch.cuda.synchronize()
    return float(loss.detach()), scale, grads, {n: b.detach().clone() for n, b in model.named_buffers()}


def _admitted_pairs(pkg, model, batch, fusion):
    """the BatchNorms of the dense-block pairs one of the two folded forward queries admits at the shapes of this batch: asked of the library directly"""
    L = pkg._lib.lib()
    shapes, hooks = {}, []
    for m in model.modules():
        if isinstance(m, pkg.nn.Conv2d):
            hooks.append(m.register_forward_hook(lambda mod, inp, out: shapes.__setitem__(id(mod), tuple(inp[0].shape))))
    before = pkg.ops.frozen_fold(False)                                                # (today's per-layer path: every conv module is called)
    try:
        model(batch[0], batch[1]) if fusion else model(batch[0])
    finally:
        pkg.ops.frozen_fold(before)
    for h in hooks:
        h.remove()
    admitted = []
    for blk in model.modules():
        if isinstance(blk, pkg._trunk._ResidualBlock) and not blk.partial:
            pairs = [(getattr(blk, c), getattr(blk, b)) for c, b in blk._chain] + ([(blk.downsample[0], blk.downsample[1])] if blk.downsample is not None else [])
            for conv, bn in pairs:
                k, c, r, _ = conv.weight.shape
                d = pkg.ops._desc(shapes[id(conv)], conv.weight.shape, conv.stride[0], conv.padding[0], conv.dilation[0])
                if c % 16 == 0 and k % 16 == 0 and (L.p3d_fx_conv_fwd_infer_supported(ctypes.byref(d), 0) or L.p3d_fx_conv_fwd_infer_any_supported(ctypes.byref(d))):
                    admitted.append(bn)
    return admitted


# What two fp32 paths through a whole network may differ by, for which there is no float64 reference.  Every convolution pass of either leg is within TOL of the
# exact result relative to the largest value (the per-layer bound), so the two legs differ by at most 2 * TOL per pass; a gradient has passed through at most all
# `depth` convolutions forward and all of them backward; the rounding errors of distinct launches are independent and add in quadrature:
# 2 * TOL * sqrt(2 * depth), relative to the largest element of the tensor -- 5.2e-5 for R18 depthnet (21 convolutions), 1.0e-4 for R50 fusionnet (79).  It is
# held for the loss, for the output of every ReLU layer, and for EVERY parameter's gradient.
# That bound supposes the two legs differentiate the same function, and a ReLU is not continuous: an input within the forward error of zero may be masked by one leg
# and passed by the other, and that element's dy then reaches every gradient upstream (measured: R50 fusionnet at side 65 on the first batch, one element of
# layer1.0's closing ReLU, 1.9e-2 of the largest element of one gradient -- profiles/train_frozen_fold.md).  Whether that happened is read from the forward alone:
# the outputs of every ReLU layer of both legs are compared, and the gradients are compared on the first of four seeded batches on which no element has its mask
# flipped.  A batch that is passed over must show that it is this and nothing else: the flipped elements are within the forward bound of zero in both legs, and
# there are at most FLIPS_MOST of them in the network.
def _network_bound(model):
    depth = sum(1 for m in model.modules() if isinstance(m, torch.nn.Conv2d))
    return 2 * TOL * (2 * depth) ** 0.5


FLIPS_MOST = 4


def _flips(bound, y_off, y_on):
    """the ReLU outputs of the two legs: every layer within the bound of the other relative to its largest value; returns the number of elements that one leg
    masks and the other passes, each of which must be within the bound of zero in both"""
    assert sorted(y_off) == sorted(y_on) and len(y_off) > 0
    flips = 0
    for name in y_off:
        a, b = y_off[name], y_on[name]
        top = a.abs().max().item()
        assert (b.double() - a.double()).abs().max().item() <= bound * top, name
        differ = (a > 0) != (b > 0)
        n = int(differ.sum())
        if n:
            assert max(a[differ].abs().max().item(), b[differ].abs().max().item()) <= bound * top, name
            flips += n
    return flips


# model, fusion, side, FlatAdam sinks (False: autograd's own gradients, on the smaller network)
NETWORKS = [('resnet18', False, 64, True), ('resnet18', False, 65, True), ('resnet50', True, 64, True), ('resnet50', True, 65, True),
            ('resnet18', False, 64, False), ('resnet18', False, 65, False)]


@pytest.mark.parametrize('model_name,fusion,side,sinks', NETWORKS, ids=lambda v: {True: 'on', False: 'off'}[v] if isinstance(v, bool) else str(v))
def test_whole_network(pkg, fold_on, model_name, fusion, side, sinks):
    ops = pkg.ops
    ops.x3_any(side % 2 == 1)

    def leg(on, batch):
        """one step from the same parameters: (loss, its scale, gradients, ReLU outputs, model, admitted BatchNorms)"""
        fold_on(on)
        model, tr = _network(pkg, model_name, fusion, side, trainer=sinks)
        admitted = _admitted_pairs(pkg, model, batch, fusion)
        before = {n: b.detach().clone() for n, b in model.named_buffers()}
        calls, relus = [], {}
        loss, scale, grads, after = _step(pkg, model, tr, batch, fusion, calls, relus)
        for n in before:                                                           # running statistics and num_batches_tracked: bit-unchanged
            assert torch.equal(before[n], after[n]), n
        bns = {m.weight.data_ptr(): m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)}
        folded = {bn.weight.data_ptr() for bn in admitted} if on else set()
        assert len(admitted) > 0
        # exactly the other BatchNorms went through ops.batch_norm_act, once each: the stem(s), the Fusion BatchNorm and the refused layers
        assert sorted(calls) == sorted(set(bns) - folded), (len(calls), len(bns), len(folded))
        if on:
            assert model.__dict__['_frozen_fold']['plan'].generation == 1          # one fold for the step
        return loss, scale, grads, relus, model, folded

    for rank in range(4):
        batch = _batch(pkg, side, fusion, rank)
        l0, scale, g0, y0, model, _ = leg(False, batch)
        l1, _, g1, y1, model, folded = leg(True, batch)
        bound = _network_bound(model)
        flips = _flips(bound, y0, y1)
        print('%s side %d %s batch %d: %d ReLU element(s) masked by one leg only' % (model_name, side, 'sinks' if sinks else 'autograd', rank, flips))
        if flips == 0:
            break
        assert flips <= FLIPS_MOST, flips
    assert flips == 0, 'no batch without a flipped ReLU element among four'
    l2, _, g2, _, model, folded = leg(True, batch)
    assert l1 == l2 and all(torch.equal(_bits(g1[n]), _bits(g2[n])) for n in g1)       # bitwise reproducible
    if sinks:
        # the optimizer step wrote the weights: the next forward folds again, and a layer's output differs from one on the stale fold
        plan = model.__dict__['_frozen_fold']['plan']
        unit = next(u for u in plan.units if u.bn.weight.data_ptr() in folded)
        stale_w = plan.weight(unit).clone()
        x = torch.randn(2, unit.c, 16, 16, device='cuda')
        unit.seen, plan.epoch = unit._key(), ops.WEIGHT_EPOCH                         # pretend it is fresh: the forward runs on the stale fold
        y_stale = pkg.ops_frozen.conv_bn(x, unit.conv, unit.bn, relu=True)
        assert plan.generation == 1
        unit.seen = None
        with torch.enable_grad():
            model(batch[0], batch[1]) if fusion else model(batch[0])
        assert plan.generation == 2
        y_fresh = pkg.ops_frozen.conv_bn(x, unit.conv, unit.bn, relu=True)
        assert plan.generation == 2 and not torch.equal(y_stale, y_fresh)
        assert not torch.equal(stale_w, plan.weight(unit))
        assert torch.equal(y_fresh, pkg.infer.FoldedConv(unit.conv, unit.bn, any_size=True)(x, None, True))
    rel = {n: ((g1[n].double() - g0[n].double()).abs().max() / g0[n].double().abs().max().clamp_min(1e-30)).item() for n in g0}
    worst = max(rel, key=rel.get)
    print('%s side %d %s: loss off %.8e on %.8e (scale %.3e)  gradient difference / largest: median %.3e worst %.3e (%s)  bound %.3e'
          % (model_name, side, 'sinks' if sinks else 'autograd', l0, l1, scale, sorted(rel.values())[len(rel) // 2], rel[worst], worst, bound))
    assert abs(l1 - l0) <= bound * scale
    for n in rel:
        assert rel[n] <= bound, (n, rel[n])


def test_skip_relu_block_under_sinks(pkg, fold_on):
    """the closing layer of a -skip_relu block with an identity shortcut: no ReLU, so the residual's gradient is dy itself, which the weight gradient reads on the
    second stream (FlatAdam sinks) while autograd adds the first convolution's data gradient onto it for the block input.  Every gradient against float64 (two
    convolutions deep: 2 x TOL of the largest value), and five runs bit-equal."""
    ops = pkg.ops
    gen = torch.Generator(device='cuda').manual_seed(21)
    blk = pkg._trunk.BasicBlock(64, 64, skip_relu=True).cuda().train()
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.eval()
                m.running_mean.copy_(torch.randn(64, device='cuda', generator=gen))
                m.running_var.copy_(torch.rand(64, device='cuda', generator=gen) * 1.5 + 0.5)
                m.weight.copy_(torch.rand(64, device='cuda', generator=gen) + 0.5)
                m.bias.copy_(torch.randn(64, device='cuda', generator=gen))
    x = torch.randn(8, 64, 32, 32, device='cuda', generator=gen)
    dy = torch.randn(8, 64, 32, 32, device='cuda', generator=gen)
    # float64 on the CPU
    d = lambda t: t.detach().double().cpu()
    ref_p = {n: d(p).requires_grad_(True) for n, p in blk.named_parameters()}
    xr = d(x).requires_grad_(True)

    def bn64(z, b):
        m = getattr(blk, b)
        s = ref_p[b + '.weight'] / (d(m.running_var) + m.eps).sqrt()
        return (z - d(m.running_mean)[None, :, None, None]) * s[None, :, None, None] + ref_p[b + '.bias'][None, :, None, None]

    u = bn64(F.conv2d(xr, ref_p['conv1.weight'], None, 1, 1), 'bn1').relu()
    out = bn64(F.conv2d(u, ref_p['conv2.weight'], None, 1, 1), 'bn2') + xr
    out.backward(d(dy))
    want = dict({n: p.grad for n, p in ref_p.items()}, x=xr.grad, y=out.detach())
    opt = pkg.optim.FlatAdam(list(blk.named_parameters()), 1e-3)
    assert ops.WGRAD_STREAM and all(getattr(p, '_p3d_direct_grad', False) for p in blk.parameters())
    runs = []
    for _ in range(5):
        opt.zero_grad()
        xg = x.clone().requires_grad_(True)
        y = blk(xg)
        y.backward(dy)
        ops.check_joins()
        ops.join_side_stream()
        torch.cuda.synchronize()
        runs.append(dict({n: p.grad.detach().clone() for n, p in blk.named_parameters()}, x=xg.grad.clone(), y=y.detach().clone()))
    assert '_frozen_unit' in blk.conv2.__dict__ and x.device in ops._side_streams      # folded, and the weight gradients went to the second stream
    for name, ref in want.items():
        err = ((runs[0][name].double().cpu() - ref).abs().max() / ref.abs().max()).item()
        print('skip_relu block %s: %.3e' % (name, err))
        assert err <= 2 * TOL, (name, err)
        for other in runs[1:]:
            assert torch.equal(_bits(runs[0][name]), _bits(other[name])), name


# ---- 5. distillation ------------------------------------------------------------------------------------------------------------------------------
def _distill(pkg, semi):
    flags = ['-model', 'resnet18', '-suffix', 't', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1', '-num_joints', '17', '-side_in', '64',
             '-do_teach', '-do_fusion', '-do_freeze'] + (['-semi_teach', '-semi_batch', '2', '-synthetic', '1', '-workers', '0'] if semi else [])
    args = pkg.opts.parse(flags)
    student, teacher = pkg.depthnet.resnet18(args, False), pkg.fusionnet.resnet18(args, False)
    rng = np.random.default_rng(3)
    for net, seed in ((student, 0), (teacher, 1)):
        det = pkg.synth.det_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed)
        for key in det:
            if key.endswith('running_mean'):
                det[key] = (0.1 * rng.standard_normal(det[key].shape)).astype(np.float32)
            elif key.endswith('running_var'):
                det[key] = rng.uniform(0.5, 2.0, det[key].shape).astype(np.float32)
        net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in det.items()})
    trainer = pkg.depth_train.Trainer(args, student.cuda(), pkg.utils.get_info())
    att = lambda seed: torch.from_numpy(np.random.default_rng(seed).uniform(0.5, 1.5, (2, 1, 4, 4)).astype(np.float32))
    if semi:
        c, d, tc, tv = pkg.synth.make_batch(2, side=64, rank=12, step=0)
        trainer.semi_loader = [tuple(torch.from_numpy(v) for v in (c, d, tc, tv)) + (att(2),)]
        trainer.semi_worker = iter(trainer.semi_loader)
    trainer.set_teacher(teacher.cuda())
    trainer.verbose = False
    c, d, tc, tv = pkg.synth.make_batch(2, side=64, rank=11, step=0)
    record = trainer.train(1, [tuple(torch.from_numpy(v) for v in (c, d, tc, tv)) + (att(1),)])
    torch.cuda.synchronize()
    return record, {k: v.detach().cpu().numpy() for k, v in student.state_dict().items()}, student, trainer


@pytest.mark.parametrize('semi', [False, True], ids=['do_teach', 'semi_teach'])
def test_distillation_step(pkg, fold_on, semi):
    """one -do_teach -do_freeze -do_fusion iteration with the switch on against off: the tolerances tests/test_distill.py holds its legs to"""
    fold_on(False)
    rec0, sd0, _, _ = _distill(pkg, semi)
    fold_on(True)
    rec1, sd1, student, trainer = _distill(pkg, semi)
    plan = student.__dict__['_frozen_fold']['plan']
    assert plan.generation == 1                                                    # -semi_teach: two student forwards, one fold
    assert not any(m.training for m in student.modules() if isinstance(m, torch.nn.BatchNorm2d))
    for key in ('cam_train_loss', 'dist_train_loss'):
        print('%s %s: off %.8e on %.8e' % ('semi' if semi else 'teach', key, rec0[key], rec1[key]))
        assert rec1[key] == pytest.approx(rec0[key], rel=1e-3)
    names = [n for n, _ in student.named_parameters()]
    pn0 = np.array([np.linalg.norm(sd0[n].astype(np.float64)) for n in names])
    pn1 = np.array([np.linalg.norm(sd1[n].astype(np.float64)) for n in names])
    assert np.abs(pn1 - pn0).max() < 1e-5 * pn0.max()
    assert max(np.abs(sd1[n] - sd0[n]).max() for n in names) < 3e-5
    for k in sd0:
        if k not in names:
            assert np.array_equal(sd0[k], sd1[k]), k                               # frozen: the running statistics of both legs are the loaded ones
    with pytest.raises(pkg._lib.P3DError, match='frozen_fold'):
        pkg.graphed.GraphedStep(trainer)
