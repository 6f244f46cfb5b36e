"""Inference with BatchNorm folded into the x3 convolutions (infer.py, p3d_fx_fold_bn_images, p3d_fx_conv_fwd_infer, p3d_stem_tail_infer).

Fold images bit-exact against p3d_fx_weight_images of the fold done in torch; every conv shape class against a float64 forward; whole networks
against both today's eval path and a float64 forward of the same state_dict; no round-1 kernel in a folded forward; refresh(); the Trainer switch."""
import ctypes
import json
import os

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


def _net(pkg, module, model='resnet18', *extra, side=128, seed=0):
    args = _args(pkg, model, *extra, side=side)
    net = getattr(getattr(pkg, module), model)(*((args,) if module == 'resnet' else (args, False)))
    return _stats_(net, seed).cuda().eval(), args


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


def _torch_fold(conv, bn):
    w = conv.weight.detach()
    return w * (bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps))[:, None, None, None]


def _image_of(pkg, w):
    L = pkg._lib.lib()
    k, c, r, s = w.shape
    fb, bb = ctypes.c_size_t(), ctypes.c_size_t()
    L.p3d_fx_weight_image_bytes(k, c, r * s, ctypes.byref(fb), ctypes.byref(bb))
    img = torch.empty(fb.value, dtype=torch.uint8, device=w.device)
    imgT = torch.empty(bb.value, dtype=torch.uint8, device=w.device)
    pkg._lib.check(L.p3d_fx_weight_images(pkg.ops._p(w.contiguous()), k, c, r * s, pkg.ops._p(img), pkg.ops._p(imgT), pkg.ops._stream()), 'p3d_fx_weight_images')
    return img


def _rel(got, want):
    got, want = got.detach().double(), want.detach().double()
    return float((got - want).abs().max() / max(1.0, float(want.abs().max())))


# ---- 1. fold images ------------------------------------------------------------------------------------------------------
def test_fold_images_bit_exact(pkg):
    net, _ = _net(pkg, 'depthnet', 'resnet18', '-depth_only')
    fn = pkg.infer.fold(net)
    find = {id(c.conv): c for c in fn.convs}
    for conv, bn in ((net.layer1[0].conv1, net.layer1[0].bn1),                                  # 3x3
                     (net.layer2[0].downsample[0], net.layer2[0].downsample[1]),                # 1x1 stride 2
                     (net.layer4[0].conv1, net.layer4[0].bn1)):                                 # 3x3 dilation 2
        c = find[id(conv)]
        assert torch.equal(fn.image(c), _image_of(pkg, _torch_fold(conv, bn))), conv
        _, b = _fold64(conv, bn)
        assert torch.allclose(fn.bias(c).double(), b, rtol=1e-6, atol=1e-6)
    # the stem: folded fp32 weights, bit-exact, and the image the stem kernels read
    st = fn.stems['conv1']
    w_fold = fn.buffer[st.w_off:st.w_off + 4 * st.k * st.cin * 49].view(torch.float32).view(st.k, st.cin, 7, 7)
    assert torch.equal(w_fold, _torch_fold(net.conv1, net.bn1))
    # the two channel windows of fusionnet's Fusion 1x1
    fnet, _ = _net(pkg, 'fusionnet', 'resnet18', seed=3)
    ff = pkg.infer.fold(fnet)
    wf = _torch_fold(fnet.fusion.conv, fnet.fusion.bn)
    half = wf.shape[1] // 2
    a, b = ff.fusion
    assert torch.equal(ff.image(a), _image_of(pkg, wf[:, :half].contiguous()))
    assert torch.equal(ff.image(b), _image_of(pkg, wf[:, half:].contiguous()))


def test_cached_image_rejects_a_mismatched_window(pkg):
    net, _ = _net(pkg, 'depthnet', 'resnet18')
    fn = pkg.infer.fold(net)
    c = next(c for c in fn.convs if c.k == 128 and c.c == 128 and c.rs == 9)
    x = torch.randn(2, 128, 16, 16, device='cuda')
    L = pkg._lib.lib()
    d = pkg.ops._desc(x.shape, (128, 256, 3, 3), 1, 1, 1, c_offset=128, c_total=256)       # a window of a wider weight: the image is not its own
    y = torch.empty(2, 128, 16, 16, device='cuda')
    ws = torch.empty(1 << 24, dtype=torch.uint8, device='cuda')
    assert L.p3d_fx_conv_fwd_infer(ctypes.byref(d), pkg.ops._p(x), None, fn._at(c.img_off), c.img_bytes, None, None, 0, pkg.ops._p(y), pkg.ops._p(ws),
                                   ws.numel(), pkg.ops._stream()) != 0
    d = pkg.ops._desc(x.shape, (128, 128, 3, 3), 1, 1, 1)
    assert L.p3d_fx_conv_fwd_infer(ctypes.byref(d), pkg.ops._p(x), None, fn._at(c.img_off), c.img_bytes - 16, None, None, 0, pkg.ops._p(y), pkg.ops._p(ws),
                                   ws.numel(), pkg.ops._stream()) != 0


# ---- 2. every conv shape class, conv + folded BN (+ residual) (+ ReLU) against float64 -------------------------------------------
CLASSES = [  # cin, hw, cout, k, stride, dilation
    (64, 64, 64, 1, 1, 1), (64, 64, 64, 3, 1, 1), (64, 64, 256, 1, 1, 1), (256, 64, 64, 1, 1, 1), (256, 64, 128, 1, 1, 1), (128, 64, 128, 3, 2, 1),
    (128, 32, 512, 1, 1, 1), (256, 64, 512, 1, 2, 1), (512, 32, 128, 1, 1, 1), (128, 32, 128, 3, 1, 1), (512, 32, 256, 1, 1, 1), (256, 32, 256, 3, 2, 1),
    (256, 16, 1024, 1, 1, 1), (512, 32, 1024, 1, 2, 1), (1024, 16, 256, 1, 1, 1), (256, 16, 256, 3, 1, 1), (1024, 16, 512, 1, 1, 1), (512, 16, 512, 3, 1, 2),
    (512, 16, 2048, 1, 1, 1), (1024, 16, 2048, 1, 1, 1), (2048, 16, 512, 1, 1, 1), (512, 16, 512, 3, 1, 1),
    (64, 64, 128, 3, 2, 1), (64, 64, 128, 1, 2, 1), (128, 32, 256, 3, 2, 1), (128, 32, 256, 1, 2, 1), (256, 16, 512, 3, 1, 2), (256, 16, 512, 1, 1, 1),
]


def _layer(pkg, cin, cout, k, stride, dil, seed, pad=None):
    torch.manual_seed(seed)
    conv = pkg.nn.Conv2d(cin, cout, k, stride=stride, padding=dil * (k - 1) // 2 if pad is None else pad, dilation=dil, bias=False)
    bn = pkg.nn.BatchNorm2d(cout)
    mod = _stats_(torch.nn.Sequential(conv, bn), seed).cuda().eval()
    return mod[0], mod[1]


@pytest.mark.parametrize('cls', CLASSES, ids=lambda c: 'c%d_%d_k%d_%dx%d_s%d_d%d' % (c[0], c[1], c[2], c[3], c[3], c[4], c[5]))
def test_conv_class_against_float64(pkg, cls):
    cin, hw, cout, k, stride, dil = cls
    conv, bn = _layer(pkg, cin, cout, k, stride, dil, seed=cin + cout + k)
    fc = pkg.infer.FoldedConv(conv, bn)
    x = torch.randn(2, cin, hw, hw, device='cuda')
    ho = (hw - 1) // stride + 1
    res = torch.randn(2, cout, ho, ho, device='cuda')
    pkg.ops.conv_path_stats(reset=True)
    for r, relu in ((None, False), (None, True), (res, True), (res, False)):
        got = fc(x, r, relu)
        want = _conv64(x, conv, bn, r, relu)
        assert _rel(got, want) < 2e-5, (r is not None, relu)
    stats = pkg.ops.conv_path_stats(reset=True)
    assert stats['x3']['fwd'][0] == 4 and stats['fp32']['fwd'][0] == 0, stats      # on the folded x3 path, not the fallback


@pytest.mark.parametrize('cls', [(512, 16, 512, 3, 1, 2), (2048, 16, 512, 1, 1, 1), (512, 16, 2048, 1, 1, 1), (64, 64, 256, 1, 1, 1)])
def test_conv_class_batch64_against_float64(pkg, cls):
    cin, hw, cout, k, stride, dil = cls
    conv, bn = _layer(pkg, cin, cout, k, stride, dil, seed=7)
    fc = pkg.infer.FoldedConv(conv, bn)
    x = torch.randn(64, cin, hw, hw, device='cuda')
    res = torch.randn(64, cout, hw, hw, device='cuda')
    assert _rel(fc(x, res, True), _conv64(x, conv, bn, res, True)) < 2e-5


def test_regressor_split_k_batch64(pkg):
    torch.manual_seed(5)
    conv = pkg.nn.Conv2d(2048, 272, 3, padding=1).cuda()
    fnet, _ = _net(pkg, 'depthnet', 'resnet50', side=256, seed=1)
    fnet.regressor = conv
    fn = pkg.infer.fold(fnet)
    x = torch.randn(64, 2048, 16, 16, device='cuda')
    got = fn._head(fn.heads[0], x)
    want = F.conv2d(x.double(), conv.weight.double(), conv.bias.double(), 1, 1)
    assert _rel(got, want) < 2e-5


# ---- 3. whole networks -------------------------------------------------------------------------------------------------------------------
def _blocks64(layer, x, skip_relu_last=False):
    for blk in layer:
        res = x if blk.downsample is None else _conv64(x, blk.downsample[0], blk.downsample[1])
        out, last = x, len(blk._chain) - 1
        for i, (cn, bnn) in enumerate(blk._chain):
            out = _conv64(out, getattr(blk, cn), getattr(blk, bnn), res if i == last else None, relu=(i < last) or not blk.skip_relu)
        x = out
    return x


def _stem64(conv, bn, x):
    return F.max_pool2d(_conv64(x, conv, bn, relu=True), 3, 2, 1)


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


def _forward64(net, family, x, y=None):
    if family == 'partial_depthnet':
        veil = (x != 0).double()
        c, veil = _partial64(net.conv1, x, veil)
        h = F.max_pool2d(_bn64(net.bn1, c, relu=True), 3, 2, 1)
        veil = F.max_pool2d(veil, 3, 2, 1)
        for layer in (net.layer1, net.layer2):
            for blk in layer:
                res = h if blk.downsample is None else _conv64(h, blk.downsample[0], blk.downsample[1])
                out, last = h, len(blk._chain) - 1
                for i, (cn, bnn) in enumerate(blk._chain):
                    out, veil = _partial64(getattr(blk, cn), out, veil)
                    out = _bn64(getattr(blk, bnn), out, res if i == last else None, relu=True)
                h = out
        h = _blocks64(net.layer4, _blocks64(net.layer3, h))
        return _conv64(h, net.regressor, None), h
    if family == 'fusionnet':
        a = _blocks64(net.layer2, _blocks64(net.layer1, _stem64(net.conv1, net.bn1, x)))
        b = _blocks64(net.layer6, _blocks64(net.layer5, _stem64(net.conv2, net.bn2, y)))
        h = _conv64(torch.cat([a, b], 1), net.fusion.conv, net.fusion.bn, relu=True)
    else:
        h = _blocks64(net.layer2, _blocks64(net.layer1, _stem64(net.conv1, net.bn1, x)))
    if family == 'resnet':
        h = _blocks64(net.layer4, _blocks64(net.layer3, h))
        z = _conv64(h, net.cam_regressor, None)
        return (z, _conv64(h, net.mat_regressor, None)) if net.mat_regressor is not None else z
    m = _blocks64(net.layer3, h)
    n = _blocks64(net.layer4, torch.relu(m) if net.skip_relu else m)
    z = _conv64(torch.relu(n) if net.skip_relu else n, net.regressor, None)
    return z, (m if net.early_dist else n)


NETS = [('depthnet', 'resnet18', ()), ('depthnet', 'resnet50', ()), ('depthnet', 'resnet18', ('-depth_only',)), ('depthnet', 'resnet50', ('-depth_only',)),
        ('depthnet', 'resnet18', ('-early_dist',)), ('depthnet', 'resnet18', ('-skip_relu',)), ('depthnet', 'resnet50', ('-early_dist', '-skip_relu')),
        ('resnet', 'resnet18', ('-joint_space',)), ('fusionnet', 'resnet18', ()), ('partial_depthnet', 'resnet18', ('-depth_only',))]


@pytest.mark.parametrize('family,model,extra', NETS, ids=lambda v: v if isinstance(v, str) else ''.join(v))
def test_whole_network(pkg, family, model, extra):
    whole_network_case(pkg, family, model, extra, 128, 128)


def whole_network_case(pkg, family, model, extra, h, w, n=2):
    """infer.fold(net) and the unfolded eval forward on an [n, Cin, h, w] batch against the float64 forward; returns the conv path counters of the folded forward"""
    net, args = _net(pkg, family, model, *extra, side=128, seed=len(extra))
    g = torch.Generator(device='cuda').manual_seed(0)
    cin = 1 if args.depth_only else 3
    x = torch.randn(n, cin, h, w, device='cuda', generator=g)
    if family == 'partial_depthnet':
        x = x * (torch.rand(n, 1, h, w, device='cuda', generator=g) > 0.3)
    y = torch.rand(n, 1, h, w, device='cuda', generator=g) if family == 'fusionnet' else None
    fn = pkg.infer.fold(net)
    pkg.ops.conv_path_stats(reset=True)
    got = fn(x) if y is None else fn(x, y)
    stats = pkg.ops.conv_path_stats(reset=True)
    with torch.no_grad():
        old = net(x) if y is None else net(x, y)
        want = _forward64(net, family, x, y)
    got, old, want = [t if isinstance(t, tuple) else (t,) for t in (got, old, want)]
    assert len(got) == len(old) == len(want)
    for gt, ot, wt in zip(got, old, want):
        assert gt.shape == ot.shape == wt.shape
        assert _rel(gt, wt) < 1e-4 and _rel(ot, wt) < 1e-4
        assert _rel(gt, ot) < 1e-4
    return stats


# ---- 4. no round-1 kernel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', ['depthnet', 'fusionnet'])
def test_folded_forward_has_no_round1_launch(pkg, family):
    net, _ = _net(pkg, family, 'resnet50', side=256)
    x = torch.randn(64, 3, 256, 256, device='cuda')
    y = torch.rand(64, 1, 256, 256, device='cuda') if family == 'fusionnet' else None
    fn = pkg.infer.fold(net)
    args = (x,) if y is None else (x, y)
    pkg.ops.conv_path_stats(reset=True)
    fn(*args)
    torch.cuda.synchronize()
    folded = pkg.ops.conv_path_stats(reset=True)
    with torch.no_grad():
        net(*args)
    torch.cuda.synchronize()
    default = pkg.ops.conv_path_stats(reset=True)
    assert folded['fp32']['fwd'][0] == 0, folded
    assert folded['x3']['fwd'][0] > 0
    assert default['fp32']['fwd'][0] > 0, default


# ---- 5. refresh ---------------------------------------------------------------------------------------------------------------------
def test_refresh_after_optimizer_step(pkg):
    net, _ = _net(pkg, 'depthnet', 'resnet18', side=128)
    x = torch.randn(2, 3, 128, 128, device='cuda')
    fn = pkg.infer.fold(net)
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    net.train()
    z, feat = net(x)
    (z.square().mean() + feat.square().mean()).backward()
    opt.step()
    net.eval()
    with torch.no_grad():
        want = net(x)[0]
    assert _rel(fn(x)[0], want) > 1e-3                          # stale: the weights and running statistics moved
    fn.refresh()
    assert _rel(fn(x)[0], want) < 1e-4


# ---- 7. Trainer -------------------------------------------------------------------------------------------------------------------
def test_trainer_folded_test_matches_reference(pkg, tmp_path, monkeypatch):
    monkeypatch.setenv('P3D_FOLDED_EVAL', '1')
    g = np.load(golden_path('eval.npz'))
    meta = tmp_path / 'metadata.json'
    meta.write_text(json.dumps(dict(loader=dict(h36m='depth_datasets'), no_depth=dict(h36m=False),
                                    thresholds=dict(h36m=json.loads(str(g['thresh']))), root=dict(h36m=str(tmp_path)))))
    args = pkg.opts.parse(['-model', 'resnet18', '-suffix', 't', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1',
                           '-num_joints', '17', '-side_in', '256', '-metadata', str(meta)])
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
    pkg.ops.conv_path_stats(reset=True)
    record = trainer.test(1, batches)
    stats = pkg.ops.conv_path_stats(reset=True)
    assert trainer.__dict__.get('_folded_model') is not None and trainer._eval_net is None
    assert stats['fp32']['fwd'][0] == 0, stats                  # 256^2 at batch 2: every conv on the folded path
    want = json.loads(str(g['test_record']))
    assert set(record) == set(want)
    assert record['test_loss'] == pytest.approx(want['test_loss'], rel=1e-3)
    assert record['cam_mean'] == pytest.approx(want['cam_mean'], rel=1e-3)
    for k in ('score_pck', 'score_auc', 'solid', 'close', 'depth', 'jitter', 'switch', 'fail'):
        assert record[k] == pytest.approx(want[k], abs=2e-3), k


def _distill_trainer(pkg, teacher_eval):
    g = np.load(golden_path('distill.npz'))
    args = pkg.opts.parse(['-model', 'resnet18', '-suffix', 't', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1',
                           '-num_joints', '17', '-side_in', '128', '-do_teach', '-do_fusion'])
    student = pkg.depthnet.resnet18(args, False)
    teacher = pkg.fusionnet.resnet18(args, False)
    for net, seed in ((student, 0), (teacher, 1)):
        det = pkg.synth.det_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed)
        net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in det.items()})
    teacher = teacher.cuda()
    if teacher_eval:
        _stats_(teacher, 2).eval()
    trainer = pkg.depth_train.Trainer(args, student.cuda(), pkg.utils.get_info())
    trainer.set_teacher(teacher)
    trainer.verbose = False
    c, d, tc, tv = pkg.synth.make_batch(2, side=128, rank=11, step=0)
    batch = tuple(torch.from_numpy(x) for x in (c, d, tc, tv, g['step.att']))
    return trainer, batch, g, student


def test_distill_step_under_switch_matches_reference(pkg, monkeypatch):
    monkeypatch.setenv('P3D_FOLDED_EVAL', '1')
    trainer, batch, g, student = _distill_trainer(pkg, teacher_eval=False)
    record = trainer.train(1, [batch])
    assert trainer.folded_teacher is None                       # a teacher in training mode keeps its path
    want = json.loads(str(g['step.record']))
    assert record['cam_train_loss'] == pytest.approx(want['cam_train_loss'], rel=1e-3)
    assert record['dist_train_loss'] == pytest.approx(want['dist_train_loss'], rel=1e-3)
    names = json.loads(str(g['step.names']))
    sd = {k: v.detach().cpu().numpy() for k, v in student.state_dict().items()}
    pn = np.array([np.linalg.norm(sd[n].astype(np.float64)) for n in names])
    assert np.abs(pn - g['step.param_norms']).max() < 1e-5 * g['step.param_norms'].max()


def test_distill_step_with_folded_teacher(pkg, monkeypatch):
    results = []
    for on in ('0', '1'):
        monkeypatch.setenv('P3D_FOLDED_EVAL', on)
        trainer, batch, _, student = _distill_trainer(pkg, teacher_eval=True)
        c, d, tc, tv, att = (t.cuda() for t in batch)
        cam, dist = trainer.distill_step(1, c, d, tc, tv, att)
        assert (trainer.folded_teacher is not None) == (on == '1')
        results.append((float(cam), float(dist), student.state_dict()['regressor.weight'].detach().clone()))
    (c0, d0, w0), (c1, d1, w1) = results
    assert c1 == pytest.approx(c0, rel=1e-4) and d1 == pytest.approx(d0, rel=1e-4)
    assert float((w1 - w0).abs().max()) < 3e-5
