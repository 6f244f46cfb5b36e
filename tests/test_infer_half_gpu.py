"""-half_acc inference with BatchNorm folded into the fp16 convolutions (infer.fold_half, fold kind 2 of p3d_fx_fold_bn_images, p3d_hconv2d_fwd_infer).

Fold images bit-exact against p3d_weight_images_f16 of the fold done in torch; every ResNet-50 conv class at batch 64 against float64 arithmetic on the
fp16-rounded operands; whole networks of all five families against a float64 forward and the unfolded fp16 model; no BatchNorm pass in a folded
forward; refresh(); the Trainer switch P3D_FOLDED_EVAL_HALF."""
import ctypes
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden_path
from test_infer_gpu import CLASSES, _bn64, _conv64, _fold64, _forward64, _layer, _net, _partial64, _stats_, _torch_fold

pytestmark = pytest.mark.gpu


def _image16(pkg, w, cpad):
    """p3d_weight_images_f16 of an fp32 weight: the fp16 forward image [K][R][S][Cpad]."""
    k, c, r, s = w.shape
    img = torch.empty((k, r, s, cpad), dtype=torch.float16, device=w.device)
    pkg._lib.check(pkg._lib.lib().p3d_weight_images_f16(pkg.ops._p(w.contiguous()), pkg.ops._p(img), None, k, c, r * s, cpad, pkg.ops._stream()),
                   'p3d_weight_images_f16')
    return img


def _err(got, want):
    """max |got - want| / max |want|"""
    got, want = got.detach().double(), want.detach().double()
    return float((got - want).abs().max() / want.abs().max())


def _find(fn, conv):
    return next(c for c in fn.convs if c.conv is conv)


# ---- 1. fold images -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('extra', [(), ('-depth_only',)], ids=['cin3', 'cin1'])
def test_fold_images_bit_exact(pkg, extra):
    net, _ = _net(pkg, 'depthnet', 'resnet18', *extra)
    torch.manual_seed(4)
    with torch.no_grad():
        net.regressor.bias.normal_()                                  # a non-zero conv bias: b' = the bias (no BatchNorm, s = 1)
    hf = pkg.infer.fold_half(net)
    fn = pkg.infer.fold(net)
    for conv, bn in ((net.conv1, net.bn1),                                                       # the 7x7 stem, Cin 3 or 1 (Cpad 8)
                     (net.layer1[0].conv1, net.layer1[0].bn1),                                   # 3x3
                     (net.layer2[0].downsample[0], net.layer2[0].downsample[1]),                 # 1x1 stride 2
                     (net.layer4[0].conv1, net.layer4[0].bn1),                                   # 3x3 dilation 2
                     (net.regressor, None)):                                                     # conv bias, no BatchNorm
        c = _find(hf, conv)
        w = _torch_fold(conv, bn) if bn is not None else conv.weight.detach()
        assert torch.equal(hf.image(c), _image16(pkg, w, c.cpad)), conv
        if conv is net.conv1:
            st = fn.stems['conv1']
            assert torch.equal(hf.bias(c), fn.buffer[st.bias_off:st.bias_off + 4 * st.k].view(torch.float32))
        else:
            assert torch.equal(hf.bias(c), fn.bias(_find(fn, conv)))
    assert torch.equal(hf.bias(_find(hf, net.regressor)), net.regressor.bias.detach())


def test_fold_images_partial_convs(pkg):
    net, _ = _net(pkg, 'partial_depthnet', 'resnet18', '-depth_only', seed=2)
    hf = pkg.infer.fold_half(net)
    for conv, bn in ((net.conv1, net.bn1), (net.layer1[0].conv1, net.layer1[0].bn1), (net.layer2[0].conv2, net.layer2[0].bn2)):
        c = _find(hf, conv)
        assert c.partial
        assert torch.equal(hf.image(c), _image16(pkg, _torch_fold(conv, bn), c.cpad))
        _, b = _fold64(conv, bn)
        assert torch.allclose(hf.bias(c).double(), b, rtol=1e-6, atol=1e-6)


# ---- 2. conv classes against float64 on the fp16-rounded operands -----------------------------------------------------------------------
def _infer(pkg, x16, img, bias, stride, pad, dil, res=None, relu=False, mask_in=None, mult=None):
    L = pkg._lib.lib()
    n, cpad, h, w = x16.shape
    k, r, s, _ = img.shape
    d = pkg.ops._desc((n, cpad, h, w), (k, cpad, r, s), stride, pad, dil)
    assert L.p3d_hconv2d_fwd_infer_supported(ctypes.byref(d)) == 1
    y = torch.empty((n, k, d.Ho, d.Wo), dtype=torch.float16, device='cuda', memory_format=torch.channels_last)
    p = pkg.ops._p
    pkg._lib.check(L.p3d_hconv2d_fwd_infer(ctypes.byref(d), p(x16), p(img), p(bias), p(mask_in), p(mult), p(res), int(relu), p(y), pkg.ops._stream()),
                   'p3d_hconv2d_fwd_infer')
    return y


@pytest.mark.parametrize('cls', CLASSES, ids=lambda c: 'c%d_%d_k%d_%dx%d_s%d_d%d' % (c[0], c[1], c[2], c[3], c[3], c[4], c[5]))
def test_conv_class_batch64_against_float64(pkg, cls):
    cin, hw, cout, k, stride, dil = cls
    conv, bn = _layer(pkg, cin, cout, k, stride, dil, seed=cin + cout + k)
    img = _image16(pkg, _torch_fold(conv, bn), cin)
    _, b = _fold64(conv, bn)
    bias = b.float()
    ho = (hw - 1) // stride + 1
    x16 = pkg.ops_half.to_half_nhwc(torch.randn(64, cin, hw, hw, device='cuda'), cin)
    res16 = pkg.ops_half.to_half_nhwc(torch.randn(64, cout, ho, ho, device='cuda'), cout)
    w64 = img.double().permute(0, 3, 1, 2)
    base = F.conv2d(x16.double(), w64, bias.double(), stride, conv.padding, dil)
    for res, relu in ((None, False), (None, True), (res16, True), (res16, False)):
        got = _infer(pkg, x16, img, bias, stride, conv.padding[0], dil, res, relu)
        want = base if res is None else base + res.double()
        want = torch.relu(want) if relu else want
        assert _err(got, want) < 2e-3, (res is not None, relu)


@pytest.mark.parametrize('case', [(64, 32, 64, 3, 1, 1, 64), (1, 128, 64, 7, 2, 3, 2), (3, 64, 64, 7, 2, 3, 4)], ids=['3x3', 'stem_cin1', 'stem_cin3'])
def test_partial_conv_against_float64(pkg, case):
    cin, hw, cout, k, stride, pad, n = case
    torch.manual_seed(cin + k)
    conv = pkg.partial_conv.PartialConv(cin, cout, k, stride=stride, padding=pad, bias=False)
    bn = pkg.nn.BatchNorm2d(cout)
    mod = _stats_(torch.nn.Sequential(conv, bn), k).cuda().eval()
    conv, bn = mod[0], mod[1]
    cpad = pkg.ops_half.pad8(cin)
    img = _image16(pkg, _torch_fold(conv, bn), cpad)
    _, b = _fold64(conv, bn)
    x = torch.randn(n, cin, hw, hw, device='cuda')
    mask = (torch.rand(n, 1, hw, hw, device='cuda') > 0.4).float()
    mask[0, 0, :9, :9] = 0                                            # an all-masked window
    x16 = pkg.ops_half.to_half_nhwc(x, cpad)
    mult, mask_out = pkg.ops.mask_count(mask, k, stride, pad, 1)
    ho = mult.shape[2]
    res16 = pkg.ops_half.to_half_nhwc(torch.randn(n, cout, ho, ho, device='cuda'), cout)
    w64 = img.double().permute(0, 3, 1, 2)[:, :cin]
    raw = F.conv2d(x16.double()[:, :cin] * mask.double(), w64, None, stride, pad) * mult.double()
    for res, relu in ((None, True), (res16, True), (res16, False)):
        got = _infer(pkg, x16, img, b.float(), stride, pad, 1, res, relu, mask_in=mask, mult=mult)
        want = raw + b[None, :, None, None] + (0 if res is None else res.double())
        want = torch.relu(want) if relu else want
        assert _err(got, want) < 2e-3, (res is not None, relu)


# ---- 3. whole networks -----------------------------------------------------------------------------------------------------------------
def _forward64_partial_fusionnet(net, x, y):
    def blocks(layer, h, veil=None):
        for blk in layer:
            res = h if blk.downsample is None else _conv64(h, blk.downsample[0], blk.downsample[1])
            out, last = h, len(blk._chain) - 1
            for i, (cn, bnn) in enumerate(blk._chain):
                if veil is None:
                    out = _conv64(out, getattr(blk, cn), getattr(blk, bnn), res if i == last else None, relu=(i < last) or not blk.skip_relu)
                else:
                    out, veil = _partial64(getattr(blk, cn), out, veil)
                    out = _bn64(getattr(blk, bnn), out, res if i == last else None, relu=True)
            h = out
        return h if veil is None else (h, veil)

    a = F.max_pool2d(_conv64(x, net.conv1, net.bn1, relu=True), 3, 2, 1)
    a = blocks(net.layer2, blocks(net.layer1, a))
    veil = (y != 0).double()
    c, veil = _partial64(net.conv2, y, veil)
    h = F.max_pool2d(_bn64(net.bn2, c, relu=True), 3, 2, 1)
    veil = F.max_pool2d(veil, 3, 2, 1)
    h, veil = blocks(net.layer5, h, veil)
    h, veil = blocks(net.layer6, h, veil)
    f = _conv64(torch.cat([a, h], 1), net.fusion.conv, net.fusion.bn, relu=True)
    f = blocks(net.layer4, blocks(net.layer3, f))
    return _conv64(f, net.regressor, None), f


def _inputs(family, args, n, side, seed=0):
    """side: the side of a square crop, or (H, W)"""
    g = torch.Generator(device='cuda').manual_seed(seed)
    h, w = (side, side) if isinstance(side, int) else side
    cin = 1 if args.depth_only else (4 if getattr(args, 'extra_channel', False) else 3)
    x = torch.randn(n, cin, h, w, device='cuda', generator=g)
    if family == 'partial_depthnet':
        x = x * (torch.rand(n, 1, h, w, device='cuda', generator=g) > 0.3)
    y = None
    if family in ('fusionnet', 'partial_fusionnet'):
        y = torch.rand(n, 1, h, w, device='cuda', generator=g)
        if family == 'partial_fusionnet':
            y = y * (torch.rand(n, 1, h, w, device='cuda', generator=g) > 0.3)
    return x, y


def _half_model(pkg, net):
    net._p3d_half = True
    pkg.ops_half.refresh_weights(net)
    return net


NETS = [('depthnet', 'resnet18', (), 128, 2), ('depthnet', 'resnet18', ('-depth_only', '-skip_relu'), 128, 2), ('depthnet', 'resnet18', ('-early_dist',), 128, 2),
        ('resnet', 'resnet18', ('-joint_space',), 128, 2), ('resnet', 'resnet18', ('-extra_channel',), 128, 2), ('fusionnet', 'resnet18', (), 128, 2),
        ('partial_depthnet', 'resnet18', ('-depth_only',), 128, 2), ('partial_fusionnet', 'resnet18', (), 128, 2),
        ('depthnet', 'resnet50', (), 256, 64), ('fusionnet', 'resnet50', (), 256, 64)]


@pytest.mark.parametrize('family,model,extra,side,n', NETS, ids=lambda v: v if isinstance(v, str) else ''.join(v) if isinstance(v, tuple) else str(v))
def test_whole_network(pkg, family, model, extra, side, n):
    whole_network_case(pkg, family, model, extra, side, n)


def whole_network_case(pkg, family, model, extra, side, n, hw=None):
    """hw: (H, W) of the batch where it is not side x side"""
    net, args = _net(pkg, family, model, *extra, side=side, seed=len(extra))
    x, y = _inputs(family, args, n, hw or side)
    hf = pkg.infer.fold_half(net)
    got = hf(x) if y is None else hf(x, y)
    with torch.no_grad():
        if family == 'partial_fusionnet':
            want = _forward64_partial_fusionnet(net, x, y)
        else:
            want = _forward64(net, family, x, y)
        # (-joint_space: the unfolded fp16 model cannot run its 17-channel mat_regressor, fp16 NHWC needs K % 8 == 0; fold_half pads it to 24 rows)
        half = None if '-joint_space' in extra else _half_model(pkg, net)
        old = None if half is None else (half(x) if y is None else half(x, y))
    got, want = [t if isinstance(t, tuple) else (t,) for t in (got, want)]
    old = (None,) * len(got) if old is None else (old if isinstance(old, tuple) else (old,))
    assert len(got) == len(old) == len(want)
    for gt, ot, wt in zip(got, old, want):
        assert gt.dtype == torch.float32 and gt.shape == wt.shape
        assert _err(gt, wt) < 2e-2
        if ot is not None:
            assert ot.shape == wt.shape and _err(ot, wt) < 2e-2
            assert _err(gt, ot) < 2e-2


# ---- 4. no BatchNorm pass ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family,extra', [('depthnet', ()), ('resnet', ('-extra_channel',)), ('fusionnet', ()), ('partial_depthnet', ('-depth_only',)),
                                          ('partial_fusionnet', ())], ids=lambda v: v if isinstance(v, str) else ''.join(v))
def test_folded_forward_has_no_batchnorm_pass(pkg, monkeypatch, family, extra):
    net, args = _net(pkg, family, 'resnet18', *extra, side=128)
    x, y = _inputs(family, args, 2, 128)
    hf = pkg.infer.fold_half(net)
    half = _half_model(pkg, net)
    calls = []
    bn_act = pkg.ops_half.batch_norm_act
    monkeypatch.setattr(pkg.ops_half, 'batch_norm_act', lambda *a, **k: (calls.append('batch_norm_act'), bn_act(*a, **k))[1])
    L = pkg._lib.lib()
    eval_fwd = L.p3d_hbn_eval_fwd
    monkeypatch.setattr(L, 'p3d_hbn_eval_fwd', lambda *a: (calls.append('p3d_hbn_eval_fwd'), eval_fwd(*a))[1])
    args_in = (x,) if y is None else (x, y)
    hf(*args_in)
    assert calls == []
    with torch.no_grad():
        half(*args_in)
    assert calls.count('batch_norm_act') > 0 and calls.count('p3d_hbn_eval_fwd') > 0


# ---- 5. refresh ---------------------------------------------------------------------------------------------------------------------
def test_refresh_after_optimizer_step(pkg):
    net, _ = _net(pkg, 'depthnet', 'resnet18', side=128)
    x = torch.randn(2, 3, 128, 128, device='cuda')
    hf = pkg.infer.fold_half(net)
    stale = hf(x)[0]
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    net.train()
    z, feat = net(x)
    (z.square().mean() + feat.square().mean()).backward()
    opt.step()
    net.eval()
    fresh = pkg.infer.fold_half(net)
    want = fresh(x)[0]
    assert _err(stale, want) > 1e-2                              # the weights and running statistics moved
    hf.refresh()
    assert torch.equal(hf.buffer, fresh.buffer)
    assert torch.equal(hf(x)[0], want)


# ---- 6. Trainer -------------------------------------------------------------------------------------------------------------------
def test_trainer_half_folded_test(pkg, tmp_path, monkeypatch):
    g = np.load(golden_path('eval.npz'))
    meta = tmp_path / 'metadata.json'
    meta.write_text(json.dumps(dict(loader=dict(h36m='depth_datasets'), no_depth=dict(h36m=False),
                                    thresholds=dict(h36m=json.loads(str(g['thresh']))), root=dict(h36m=str(tmp_path)))))
    args = pkg.opts.parse(['-model', 'resnet18', '-suffix', 't', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1',
                           '-num_joints', '17', '-side_in', '256', '-metadata', str(meta), '-half_acc'])
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
    records = []
    for on in ('0', '1'):
        monkeypatch.setenv('P3D_FOLDED_EVAL_HALF', on)
        records.append(trainer.test(1, batches))
        assert (trainer.__dict__.get('_folded_half_model') is not None) == (on == '1') and trainer._eval_net is None
    plain, folded = records
    assert set(plain) == set(folded)
    assert folded['test_loss'] == pytest.approx(plain['test_loss'], rel=1e-2)
    assert folded['cam_mean'] == pytest.approx(plain['cam_mean'], rel=1e-2)
    for k in ('score_pck', 'score_auc', 'solid', 'close', 'depth', 'jitter', 'switch', 'fail'):
        assert folded[k] == pytest.approx(plain[k], abs=3e-2), k


def _distill_half_trainer(pkg, monkeypatch, folded):
    monkeypatch.setenv('P3D_FOLDED_EVAL_HALF', '1' if folded else '0')
    g = np.load(golden_path('distill_half.npz'))
    args = pkg.opts.parse(['-model', 'resnet18', '-suffix', 't', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1',
                           '-num_joints', '17', '-side_in', '128', '-do_teach', '-do_fusion', '-half_acc'])
    student = pkg.depthnet.resnet18(args, False)
    teacher = pkg.fusionnet.resnet18(args, False)
    for net, seed in ((student, 0), (teacher, 1)):
        det = pkg.synth.det_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed)
        net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in det.items()})
    trainer = pkg.depth_train.Trainer(args, student.cuda(), pkg.utils.get_info())
    trainer.set_teacher(teacher.cuda().eval())
    assert (trainer.folded_teacher is not None) == folded
    trainer.verbose = False
    c, d, tc, tv = pkg.synth.make_batch(2, side=128, rank=11, step=0)
    record = trainer.train(1, [tuple(torch.from_numpy(x) for x in (c, d, tc, tv, g['att']))])
    assert trainer.skipped_steps == 0 and trainer.optimizer.steps_taken() == 1
    names = json.loads(str(g['names']))
    sd = {k: v.detach().cpu().numpy() for k, v in student.state_dict().items()}
    return record, np.array([np.linalg.norm(sd[n].astype(np.float64)) for n in names])


def test_half_distillation_step_with_folded_teacher(pkg, monkeypatch):
    """One -half_acc distill_train iteration with the folded eval-mode teacher against the same step with the unfolded eval-mode fp16 teacher, at the
    tolerances of test_half_distillation_step_matches_reference_half.  (golden/distill_half.npz itself was made with a teacher in training mode, whose
    BatchNorm normalises with batch statistics: a folded teacher, which uses the running statistics, cannot reproduce it; profiles/eval_folded_half.md.)"""
    plain, pn_plain = _distill_half_trainer(pkg, monkeypatch, folded=False)
    folded, pn_folded = _distill_half_trainer(pkg, monkeypatch, folded=True)
    assert folded['cam_train_loss'] == pytest.approx(plain['cam_train_loss'], rel=2e-3)
    assert folded['dist_train_loss'] == pytest.approx(plain['dist_train_loss'], rel=5e-3)
    assert np.abs(pn_folded - pn_plain).max() < 1e-3 * pn_plain.max()
