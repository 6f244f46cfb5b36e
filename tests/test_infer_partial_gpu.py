"""Folded inference of the partial-convolution families (infer.py: FoldedNet's partial stems and layers, p3d_fx_conv_fwd_infer_masked).

Every partial-conv class against a float64 partial conv + BatchNorm, empty windows exactly relu(b' + res); the masked stem; whole partial_depthnet and
partial_fusionnet networks against today's eval forward and a float64 forward; no BatchNorm pass and no fp32-MFMA forward launch in a folded forward; the
per-layer fallback; refresh(); the Trainer."""
import ctypes
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden_path

pytestmark = pytest.mark.gpu


def _args(pkg, model='resnet18', *extra, side=128):
    return pkg.opts.parse(['-model', model, '-suffix', 't', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1', '-num_joints', '17',
                           '-side_in', str(side)] + list(extra))


def _stats_(model, seed):
    """Non-trivial running statistics and affine parameters for every BatchNorm (a fresh model has mean 0, var 1, gamma 1, beta 0)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                c = m.num_features
                m.running_mean.copy_(0.2 * torch.randn(c, generator=g))
                m.running_var.copy_(0.5 + torch.rand(c, generator=g))
                m.weight.copy_(0.5 + torch.rand(c, generator=g))
                m.bias.copy_(0.2 * torch.randn(c, generator=g))
    return model


def _net(pkg, family, model='resnet18', side=128, seed=0):
    extra = ('-depth_only',) if family == 'partial_depthnet' else ('-do_fusion',)
    args = _args(pkg, model, *extra, side=side)
    net = getattr(getattr(pkg, family), model)(args, False)
    return _stats_(net, seed).cuda().eval()


def _fold64(conv, bn):
    w = conv.weight.detach().double()
    if bn is None:
        return w, (conv.bias.detach().double() if conv.bias is not None else torch.zeros(w.shape[0], dtype=torch.float64, device=w.device))
    s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return w * s[:, None, None, None], bn.bias.double() - bn.running_mean.double() * s


def _conv64(x, conv, bn, res=None, relu=False):
    w, b = _fold64(conv, bn)
    y = F.conv2d(x.double(), w, b, conv.stride, conv.padding, conv.dilation)
    if res is not None:
        y = y + res.double()
    return torch.relu(y) if relu else y


def _partial64(conv, x, mask):
    k = conv.kernel_size[0]
    cnt = F.conv2d(mask.double(), torch.ones(1, 1, k, k, dtype=torch.float64, device=x.device), None, conv.stride, conv.padding, conv.dilation)
    mask_out = cnt.clamp(0, 1)
    mult = k * k / (cnt + 1e-6) * mask_out
    return F.conv2d(x.double() * mask.double(), conv.weight.double(), None, conv.stride, conv.padding, conv.dilation) * mult, mask_out


def _bn64(bn, y, res=None, relu=False):
    s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    y = y * s[None, :, None, None] + (bn.bias.double() - bn.running_mean.double() * s)[None, :, None, None]
    if res is not None:
        y = y + res
    return torch.relu(y) if relu else y


def _rel(got, want):
    got, want = got.detach().double(), want.detach().double()
    return float((got - want).abs().max() / max(1.0, float(want.abs().max())))


def _blocks64(layer, x):
    for blk in layer:
        res = x if blk.downsample is None else _conv64(x, blk.downsample[0], blk.downsample[1])
        out, last = x, len(blk._chain) - 1
        for i, (cn, bnn) in enumerate(blk._chain):
            out = _conv64(out, getattr(blk, cn), getattr(blk, bnn), res if i == last else None, relu=(i < last) or not blk.skip_relu)
        x = out
    return x


def _pblocks64(layer, h, veil):
    for blk in layer:
        res = h if blk.downsample is None else _conv64(h, blk.downsample[0], blk.downsample[1])
        out, last = h, len(blk._chain) - 1
        for i, (cn, bnn) in enumerate(blk._chain):
            out, veil = _partial64(getattr(blk, cn), out, veil)
            out = _bn64(getattr(blk, bnn), out, res if i == last else None, relu=True)
        h = out
    return h, veil


def _pstem64(conv, bn, x, veil):
    c, veil = _partial64(conv, x, veil)
    return F.max_pool2d(_bn64(bn, c, relu=True), 3, 2, 1), F.max_pool2d(veil, 3, 2, 1)


def _forward64(net, family, x, y=None):
    if family == 'partial_depthnet':
        h, veil = _pstem64(net.conv1, net.bn1, x, (x != 0).double())
        h, veil = _pblocks64(net.layer1, h, veil)
        h, _ = _pblocks64(net.layer2, h, veil)
    else:
        a = _blocks64(net.layer2, _blocks64(net.layer1, F.max_pool2d(_conv64(x, net.conv1, net.bn1, relu=True), 3, 2, 1)))
        b, veil = _pstem64(net.conv2, net.bn2, y, (y != 0).double())
        b, veil = _pblocks64(net.layer5, b, veil)
        b, _ = _pblocks64(net.layer6, b, veil)
        h = _conv64(torch.cat([a, b], 1), net.fusion.conv, net.fusion.bn, relu=True)
    h = _blocks64(net.layer4, _blocks64(net.layer3, h))
    return _conv64(h, net.regressor, None), h


def _inputs(family, n, side, seed=0):
    """The synthetic recipe: color ~ N(0, 1), depth ~ U[0, 1) with values < 0.3 zeroed (partial_depthnet: the depth map is the input)."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    h, w = (side, side) if isinstance(side, int) else side      # (a square crop, or (H, W))
    depth = torch.rand(n, 1, h, w, device='cuda', generator=g)
    depth = depth * (depth >= 0.3)
    depth[0, :, :h // 8, :w // 8] = 0                            # a hole wider than the stem's 7x7 window
    if family == 'partial_depthnet':
        return (depth,)
    return torch.randn(n, 3, h, w, device='cuda', generator=g), depth


def _mask(n, hw, seed, block):
    """~30 % holes plus a block of zeros in image 0 wide enough that some windows see no valid input."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    m = (torch.rand(n, 1, hw, hw, device='cuda', generator=g) >= 0.3).float()
    m[0, :, 2:2 + block, 3:3 + block] = 0
    return m


# ---- 1. every partial-conv class: folded partial conv + BatchNorm (+ residual) (+ ReLU) against float64 ------------------------------------------------
CLASSES = [  # cin, hw, cout, k, stride, batch    (layer1 / layer2 of both families; ResNet-18 and ResNet-50)
    (64, 32, 64, 1, 1, 2), (64, 32, 256, 1, 1, 2), (256, 32, 64, 1, 1, 2), (256, 32, 128, 1, 1, 2), (128, 16, 512, 1, 1, 2),
    (64, 32, 64, 3, 1, 2), (128, 16, 128, 3, 1, 4), (64, 32, 128, 3, 2, 2), (128, 32, 128, 3, 2, 2),
    (128, 16, 128, 3, 1, 2),                            # tiles 4, 72 K steps: split-K in two (fx_plan_split)
]


def _pconv_layer(pkg, cin, cout, k, stride, seed):
    torch.manual_seed(seed)
    conv = pkg.partial_conv.PartialConv(cin, cout, k, stride=stride, padding=(k - 1) // 2, bias=False)
    bn = pkg.nn.BatchNorm2d(cout)
    mod = _stats_(torch.nn.Sequential(conv, bn), seed).cuda().eval()
    return mod[0], mod[1]


@pytest.mark.parametrize('cls', CLASSES, ids=lambda c: 'c%d_%d_k%d_%dx%d_s%d_n%d' % (c[0], c[1], c[2], c[3], c[3], c[4], c[5]))
def test_partial_class_against_float64(pkg, cls):
    cin, hw, cout, k, stride, n = cls
    conv, bn = _pconv_layer(pkg, cin, cout, k, stride, seed=cin + cout + k + stride)
    fc = pkg.infer.FoldedConv(conv, bn)
    assert fc.conv.foldable and fc.conv.partial
    x = torch.randn(n, cin, hw, hw, device='cuda')
    veil = _mask(n, hw, seed=cin + k, block=6)
    ho = (hw - 1) // stride + 1
    res = torch.randn(n, cout, ho, ho, device='cuda')
    c64, mask_out64 = _partial64(conv, x, veil)
    empty = mask_out64.expand(n, cout, ho, ho) == 0
    assert int(empty[0, 0].sum()) > 0                           # the zero block leaves windows with no valid input
    b = fc.bias(fc.conv)[None, :, None, None]
    pkg.ops.conv_path_stats(reset=True)
    for r, relu in ((None, False), (None, True), (res, True), (res, False)):
        got, mask_out = fc(x, r, relu, veil=veil)
        want = _bn64(bn, c64, None if r is None else r.double(), relu)
        assert _rel(got, want) < 1e-4, (r is not None, relu)
        assert torch.equal(mask_out.double(), mask_out64)
        exact = b.expand_as(got) if r is None else b + r      # an empty window: relu(b' + res), as the reference's BatchNorm makes of the 0 there
        exact = torch.relu(exact) if relu else exact
        assert torch.equal(got[empty], exact[empty]), (r is not None, relu)
    stats = pkg.ops.conv_path_stats(reset=True)
    assert stats['x3']['fwd'][0] == 4 and stats['fp32']['fwd'][0] == 0, stats


def test_split_k_class_takes_slabs(pkg):
    """The split-K case above really splits: its workspace holds slabs beyond the weight image."""
    L = pkg._lib.lib()
    d = pkg.ops._desc((2, 128, 16, 16), (128, 128, 3, 3), 1, 1, 1)
    fb = ctypes.c_size_t()
    L.p3d_fx_weight_image_bytes(128, 128, 9, ctypes.byref(fb), None)
    assert L.p3d_fx_conv_fwd_infer_masked_supported(ctypes.byref(d)) == 1
    assert L.p3d_fx_conv_fwd_infer_workspace_bytes(ctypes.byref(d)) >= fb.value + 2 * 2 * 128 * 16 * 16 * 4


def test_masked_entry_refusals(pkg):
    conv, bn = _pconv_layer(pkg, 64, 64, 3, 1, seed=1)
    fc = pkg.infer.FoldedConv(conv, bn)
    c = fc.conv
    L = pkg._lib.lib()
    x = torch.randn(2, 64, 16, 16, device='cuda')
    veil = _mask(2, 16, 0, 4)
    mult, _ = pkg.ops.mask_count(veil, 3, 1, 1, 1)
    y = torch.empty(2, 64, 16, 16, device='cuda')
    ws = torch.empty(1 << 22, dtype=torch.uint8, device='cuda')
    d = pkg.ops._desc(x.shape, (64, 64, 3, 3), 1, 1, 1)
    call = lambda d, nbytes, mask: L.p3d_fx_conv_fwd_infer_masked(ctypes.byref(d), pkg.ops._p(x), fc._at(c.img_off), nbytes, fc._at(c.bias_off), pkg.ops._p(mask),
                                                                  pkg.ops._p(mult), None, 0, pkg.ops._p(y), pkg.ops._p(ws), ws.numel(), pkg.ops._stream())
    assert call(d, c.img_bytes - 16, veil) != 0                 # not this descriptor's image
    assert call(d, c.img_bytes, None) != 0                      # no mask
    window = pkg.ops._desc(x.shape, (64, 128, 3, 3), 1, 1, 1, c_offset=0, c_total=128)
    assert call(window, c.img_bytes, veil) != 0
    assert call(d, c.img_bytes, veil) == 0
    with pytest.raises(pkg._lib.P3DError, match='validity mask'):
        fc(x)


# ---- 2. the masked stem ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', ['partial_depthnet', 'partial_fusionnet'])
def test_masked_stem_against_float64(pkg, family):
    net = _net(pkg, family, 'resnet18', seed=4)
    fn = pkg.infer.fold(net)
    name = 'conv1' if family == 'partial_depthnet' else 'conv2'
    st = fn.stems[name]
    assert st.masked and st.foldable
    depth = _inputs('partial_depthnet', 2, 128, seed=4)[0]
    veil = pkg.ops.nonzero_mask(depth)
    h, v = fn._stem_masked(st, depth, veil)
    want, v64 = _pstem64(st.conv, st.bn, depth, (depth != 0).double())
    assert int((v64[0] == 0).sum()) > 0                         # 7x7 windows with no valid pixel, whole pooled pixels without one
    assert _rel(h, want) < 1e-4
    assert torch.equal(v.double(), v64)


# ---- 3. whole networks -------------------------------------------------------------------------------------------------------------------
def _folds_partial_layers(fn):
    """The masked stem and every partial conv of a FoldedNet are in its fold, none left on the model's own modules."""
    partial = [c for c in fn.convs if c.partial]
    return any(st.masked and st.foldable for st in fn.stems.values()) and len(partial) > 0 and all(c.foldable for c in partial)


@pytest.mark.parametrize('family', ['partial_depthnet', 'partial_fusionnet'])
@pytest.mark.parametrize('model,side,batch', [('resnet18', 128, 2), ('resnet50', 256, 64)], ids=['r18_128_b2', 'r50_256_b64'])
def test_whole_partial_network_folded(pkg, family, model, side, batch):
    whole_partial_network_case(pkg, family, model, side, batch)


def whole_partial_network_case(pkg, family, model, side, batch, hw=None):
    """hw: (H, W) of the batch where it is not side x side"""
    net = _net(pkg, family, model, side=side, seed=2)
    inputs = _inputs(family, batch, hw or side, seed=1)
    fn = pkg.infer.fold(net)
    assert _folds_partial_layers(fn)
    got = fn(*inputs)
    with torch.no_grad():
        old = net(*inputs)
        k = min(batch, 4)                                       # (eval mode: images are independent; float64 on the first few)
        want = _forward64(net, family, *(t[:k] for t in inputs))
    for gt, ot, wt in zip(got, old, want):
        assert gt.shape == ot.shape and gt.shape[1:] == wt.shape[1:]
        assert _rel(gt[:k], wt) < 1e-4 and _rel(ot[:k], wt) < 1e-4
        assert _rel(gt, ot) < 1e-4


# ---- 4. no BatchNorm pass, no fp32-MFMA forward -----------------------------------------------------------------------------------------------
def _count_bn(pkg, monkeypatch):
    calls = []
    bn_act = pkg.ops.batch_norm_act
    monkeypatch.setattr(pkg.ops, 'batch_norm_act', lambda *a, **k: (calls.append('batch_norm_act'), bn_act(*a, **k))[1])
    L = pkg._lib.lib()
    eval_fwd = L.p3d_bn_eval_fwd
    monkeypatch.setattr(L, 'p3d_bn_eval_fwd', lambda *a: (calls.append('p3d_bn_eval_fwd'), eval_fwd(*a))[1])
    return calls


@pytest.mark.parametrize('family', ['partial_depthnet', 'partial_fusionnet'])
def test_folded_partial_forward_has_no_batchnorm_pass(pkg, monkeypatch, family):
    net = _net(pkg, family, 'resnet18', seed=5)
    inputs = _inputs(family, 2, 128, seed=5)
    fn = pkg.infer.fold(net)
    calls = _count_bn(pkg, monkeypatch)
    pkg.ops.conv_path_stats(reset=True)
    fn(*inputs)
    torch.cuda.synchronize()
    stats = pkg.ops.conv_path_stats(reset=True)
    assert calls == []
    assert stats['fp32']['fwd'][0] == 0 and stats['x3']['fwd'][0] > 0, stats
    with torch.no_grad():
        net(*inputs)
    assert calls.count('batch_norm_act') > 0 and calls.count('p3d_bn_eval_fwd') > 0


# ---- 5. the per-layer fallback ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', ['partial_depthnet', 'partial_fusionnet'])
def test_odd_side_falls_back_per_layer(pkg, monkeypatch, family):
    net = _net(pkg, family, 'resnet18', side=129, seed=7)
    inputs = _inputs(family, 2, 129, seed=7)
    fn = pkg.infer.fold(net)
    L = pkg._lib.lib()
    st = fn.stems['conv1' if family == 'partial_depthnet' else 'conv2']
    assert not L.p3d_stem_masked_supported(2, 1, 129, 129, st.k)                 # odd sides: the stem runs as the module
    calls = _count_bn(pkg, monkeypatch)
    got = fn(*inputs)
    assert calls.count('p3d_bn_eval_fwd') > 0
    with torch.no_grad():
        old = net(*inputs)
        want = _forward64(net, family, *inputs)
    for gt, ot, wt in zip(got, old, want):
        assert _rel(gt, wt) < 1e-4 and _rel(gt, ot) < 1e-4


def test_partial_conv_with_bias_falls_back(pkg):
    conv = pkg.partial_conv.PartialConv(64, 64, 3, padding=1, bias=True)
    bn = pkg.nn.BatchNorm2d(64)
    mod = _stats_(torch.nn.Sequential(conv, bn), 9).cuda().eval()
    conv, bn = mod[0], mod[1]
    fc = pkg.infer.FoldedConv(conv, bn)
    assert not fc.conv.foldable
    x = torch.randn(2, 64, 32, 32, device='cuda')
    veil = _mask(2, 32, 3, 6)
    got, _ = fc(x, None, True, veil=veil)
    k = 3
    cnt = F.conv2d(veil.double(), torch.ones(1, 1, k, k, dtype=torch.float64, device='cuda'), None, 1, 1)
    mult = k * k / (cnt + 1e-6) * cnt.clamp(0, 1)
    raw = F.conv2d(x.double() * veil.double(), conv.weight.double(), None, 1, 1)
    want = _bn64(bn, (raw * mult + conv.bias.double()[None, :, None, None]) * cnt.clamp(0, 1), relu=True)     # partial_conv.py:45-53 with a bias
    assert _rel(got, want) < 1e-4


# ---- 6. refresh ---------------------------------------------------------------------------------------------------------------------
def test_refresh_after_optimizer_step(pkg):
    net = _net(pkg, 'partial_depthnet', 'resnet18', seed=8)
    (x,) = _inputs('partial_depthnet', 2, 128, seed=8)
    fn = pkg.infer.fold(net)
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    net.train()
    z, feat = net(x)
    (z.square().mean() + feat.square().mean()).backward()
    opt.step()
    net.eval()
    with torch.no_grad():
        want = net(x)[0]
    assert float(net.layer1[0].bn1.running_mean.abs().max()) > 0
    assert _rel(fn(x)[0], want) > 1e-3                          # stale: partial-layer weights and running statistics moved
    fn.refresh()
    assert _rel(fn(x)[0], want) < 1e-4


# ---- 7. Trainer -------------------------------------------------------------------------------------------------------------------
def test_trainer_folded_test_partial(pkg, tmp_path, monkeypatch):
    g = np.load(golden_path('eval.npz'))
    meta = tmp_path / 'metadata.json'
    meta.write_text(json.dumps(dict(loader=dict(h36m='depth_datasets'), no_depth=dict(h36m=False),
                                    thresholds=dict(h36m=json.loads(str(g['thresh']))), root=dict(h36m=str(tmp_path)))))
    args = pkg.opts.parse(['-model', 'resnet18', '-suffix', 't', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1',
                           '-num_joints', '17', '-side_in', '256', '-metadata', str(meta), '-depth_only', '-partial_conv'])
    model, _ = pkg.depth_main.create_model(args)
    assert type(model).__module__.endswith('partial_depthnet')
    det = pkg.synth.det_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 0)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in det.items()})
    _stats_(model, 3)
    batches = []
    for it in range(2):
        c, d, tc, tv = pkg.synth.make_batch(2, side=256, rank=7, step=it, invalid_frac=0.2)
        rot = np.linalg.qr(np.random.Generator(np.random.PCG64(it)).standard_normal((2, 3, 3)))[0].astype(np.float32)
        batches.append(tuple(torch.from_numpy(a) for a in (c, d, tc, tv, rot)))
    records = []
    for on in ('0', '1'):
        monkeypatch.setenv('P3D_FOLDED_EVAL', on)
        trainer = pkg.depth_train.Trainer(args, model.cuda(), pkg.utils.get_info())
        trainer.verbose = False
        pkg.ops.conv_path_stats(reset=True)
        records.append(trainer.test(1, batches))
        stats = pkg.ops.conv_path_stats(reset=True)
        assert (trainer.__dict__.get('_folded_model') is not None) == (on == '1')
        if on == '1':
            assert stats['fp32']['fwd'][0] == 0, stats
    off, folded = records
    assert set(off) == set(folded)
    for k, v in off.items():
        if isinstance(v, float):
            assert folded[k] == pytest.approx(v, rel=1e-4, abs=1e-6), k


def _distill_trainer(pkg):
    g = np.load(golden_path('distill.npz'))
    args = pkg.opts.parse(['-model', 'resnet18', '-suffix', 't', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1',
                           '-num_joints', '17', '-side_in', '128', '-do_teach', '-do_fusion', '-partial_conv'])
    student = pkg.depthnet.resnet18(args, False)
    teacher = pkg.partial_fusionnet.resnet18(args, False)
    for net, seed in ((student, 0), (teacher, 1)):
        det = pkg.synth.det_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed)
        net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in det.items()})
    teacher = _stats_(teacher.cuda(), 2).eval()
    trainer = pkg.depth_train.Trainer(args, student.cuda(), pkg.utils.get_info())
    trainer.set_teacher(teacher)
    trainer.verbose = False
    c, d, tc, tv = pkg.synth.make_batch(2, side=128, rank=11, step=0)
    batch = tuple(torch.from_numpy(x) for x in (c, d, tc, tv, g['step.att']))
    return trainer, batch, student


def test_distill_step_with_fully_folded_partial_teacher(pkg, monkeypatch):
    results = []
    for on in ('0', '1'):
        monkeypatch.setenv('P3D_FOLDED_EVAL', on)
        trainer, batch, student = _distill_trainer(pkg)
        c, d, tc, tv, att = (t.cuda() for t in batch)
        assert float((d == 0).float().mean()) > 0              # the depth map has holes: the partial layers see them
        cam, dist = trainer.distill_step(1, c, d, tc, tv, att)
        assert (trainer.folded_teacher is not None) == (on == '1')
        if on == '1':
            assert trainer.folded_teacher.family == 'partial_fusionnet' and _folds_partial_layers(trainer.folded_teacher)
        results.append((float(cam), float(dist), student.state_dict()['regressor.weight'].detach().clone()))
    (c0, d0, w0), (c1, d1, w1) = results
    assert c1 == pytest.approx(c0, rel=1e-4) and d1 == pytest.approx(d0, rel=1e-4)
    assert float((w1 - w0).abs().max()) < 3e-5
