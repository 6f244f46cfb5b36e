"""The folded fp32 forward at map widths that are not multiples of 4 (p3d_fx_conv_fwd_infer_any, infer.fold(..., any_size=True)): the reference's
default -side_in 257 gives maps of 65, 33 and 17, which the aligned x3 forward refuses.

Every conv shape class of the networks on those maps against a float64 forward at the aligned path's bound, batches that end a pixel tile mid-row and
mid-image, split-K, accumulate, no write outside y or the workspace, aligned shapes through the new entry, whole networks at 129^2 / 257^2 / 129 x 193
with the launch counters, and the Trainer switch at -side_in 257.  Needs an MI355X: run with `-m gpu`."""
import ctypes
import json

import numpy as np
import pytest
import torch

import geometry_table as T
import test_infer_gpu as ti
from conftest import golden_path
from test_infer_gpu import CLASSES, _conv64, _forward64, _layer, _net, _rel

pytestmark = pytest.mark.gpu

ODD = {64: 65, 32: 33, 16: 17}                      # the 256^2 chain's maps at 257^2
EPILOGUES = ((False, False), (False, True), (True, True), (True, False))       # (residual, ReLU)


def _out(h, r, stride, pad, dil):
    return (h + 2 * pad - dil * (r - 1) - 1) // stride + 1


def _four_epilogues(pkg, conv, bn, x, seed=0, counted=True):
    """FoldedConv(any_size=True) on x with the four epilogue combinations against float64, _rel < 2e-5; every call on the x3 forward, none on the fallback"""
    fc = pkg.infer.FoldedConv(conv, bn, any_size=True)
    r, s, p, d = conv.kernel_size[0], conv.stride[0], conv.padding[0], conv.dilation[0]
    gen = torch.Generator(device='cuda').manual_seed(seed)
    res = torch.randn(x.shape[0], conv.out_channels, _out(x.shape[2], r, s, p, d), _out(x.shape[3], r, s, p, d), device='cuda', generator=gen)
    pkg.ops.conv_path_stats(reset=True)
    for with_res, relu in EPILOGUES:
        rr = res if with_res else None
        err = _rel(fc(x, rr, relu), _conv64(x, conv, bn, rr, relu))
        print('anysize conv', tuple(x.shape), tuple(conv.weight.shape), 's%d p%d d%d' % (s, p, d), 'res' if with_res else '-', 'relu' if relu else '-', 'rel %.3e' % err)
        assert err < 2e-5, (with_res, relu, err)
    stats = pkg.ops.conv_path_stats(reset=True)
    if counted:
        assert stats['x3']['fwd'][0] == 4 and stats['fp32']['fwd'][0] == 0, stats
    return stats


# ---- 1. every conv shape class on the odd maps ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 3])
@pytest.mark.parametrize('cls', CLASSES, ids=lambda c: 'c%d_%d_k%d_%dx%d_s%d_d%d' % (c[0], ODD[c[1]], c[2], c[3], c[3], c[4], c[5]))
def test_conv_class_against_float64(pkg, cls, n):
    """n = 1, 2, 3 at 65^2 / 33^2 / 17^2: 4225, 1089 and 289 pixels per image, so 128-pixel tiles end mid-row and, from n = 2 on, span two images"""
    cin, hw, cout, k, stride, dil = cls
    conv, bn = _layer(pkg, cin, cout, k, stride, dil, seed=cin + cout + k)
    x = torch.randn(n, cin, ODD[hw], ODD[hw], device='cuda')
    _four_epilogues(pkg, conv, bn, x, seed=n)


@pytest.mark.parametrize('cls', [(512, 16, 512, 3, 1, 2), (2048, 16, 512, 1, 1, 1), (512, 16, 2048, 1, 1, 1), (64, 64, 256, 1, 1, 1)],
                         ids=lambda c: 'c%d_%d_k%d_%dx%d_d%d' % (c[0], ODD[c[1]], c[2], c[3], c[3], c[5]))
def test_conv_class_batch64_against_float64(pkg, cls):
    cin, hw, cout, k, stride, dil = cls
    conv, bn = _layer(pkg, cin, cout, k, stride, dil, seed=7)
    x = torch.randn(64, cin, ODD[hw], ODD[hw], device='cuda')
    _four_epilogues(pkg, conv, bn, x, seed=64)


# widths = 1, 2, 3 mod 4, the two rectangles, a 3x3 without padding and with padding 2 (c, k, h, w, r, stride, pad, dil, n)
EXTRA = [(128, 128, 17, 17, 3, 1, 1, 1, 3), (128, 128, 18, 18, 3, 1, 1, 1, 3), (128, 128, 19, 19, 3, 1, 1, 1, 3),
         (128, 128, 18, 18, 3, 2, 1, 1, 3), (128, 128, 19, 19, 1, 2, 0, 1, 3),
         (128, 128, 17, 33, 3, 1, 1, 1, 3), (128, 128, 33, 17, 3, 1, 1, 1, 3), (128, 128, 17, 33, 3, 2, 1, 1, 3), (128, 128, 33, 17, 3, 2, 1, 1, 3),
         (128, 128, 17, 33, 3, 1, 2, 2, 2), (128, 128, 33, 17, 3, 1, 2, 2, 2),
         (128, 128, 17, 33, 3, 1, 0, 1, 3), (128, 128, 33, 17, 3, 1, 0, 1, 3), (128, 128, 17, 33, 3, 1, 2, 1, 3), (128, 128, 33, 17, 3, 1, 2, 1, 3),
         (64, 272, 19, 17, 3, 1, 0, 1, 1), (64, 64, 17, 19, 3, 2, 2, 1, 2)]


@pytest.mark.parametrize('case', EXTRA, ids=lambda c: 'c%d_k%d_%dx%d_r%d_s%d_p%d_d%d_n%d' % c)
def test_widths_rectangles_paddings(pkg, case):
    c, k, h, w, r, stride, pad, dil, n = case
    conv, bn = _layer(pkg, c, k, r, stride, dil, seed=h * w + pad, pad=pad)
    x = torch.randn(n, c, h, w, device='cuda')
    _four_epilogues(pkg, conv, bn, x, seed=h + w)


@pytest.mark.parametrize('g', [g for g in T.ROWS if g.name.endswith('_refused')], ids=lambda g: g.name)
def test_refused_rows_of_the_geometry_table(pkg, g):
    """the rows p3d_fx_conv_fwd_infer refuses (Wo % 4 != 0), through FoldedConv(..., any_size=True): now on the x3 forward"""
    conv, bn = _layer(pkg, g.c, g.k, g.r, g.stride, g.dil, seed=len(g.name), pad=g.pad)
    x = torch.randn(g.n, g.c, g.h, g.w, device='cuda')
    d = pkg.ops._desc(tuple(x.shape), tuple(conv.weight.shape), g.stride, g.pad, g.dil)
    assert pkg._lib.lib().p3d_fx_conv_fwd_infer_supported(ctypes.byref(d), 0) == 0
    _four_epilogues(pkg, conv, bn, x, seed=g.h)


def test_default_keeps_the_fallback(pkg):
    """without the keyword an odd map lands on the fp32-MFMA fallback, as before"""
    conv, bn = _layer(pkg, 128, 128, 3, 1, 1, seed=1)
    x = torch.randn(2, 128, 17, 17, device='cuda')
    fc = pkg.infer.FoldedConv(conv, bn)
    pkg.ops.conv_path_stats(reset=True)
    assert _rel(fc(x, None, True), _conv64(x, conv, bn, None, True)) < 2e-5
    stats = pkg.ops.conv_path_stats(reset=True)
    assert stats['x3']['fwd'][0] == 0 and stats['fp32']['fwd'][0] == 1, stats


# ---- 2. split-K ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('slabs', [2, 3])
@pytest.mark.parametrize('shape', [(2048, 272, 17, 17), (512, 512, 17, 19)], ids=lambda s: 'c%d_k%d_%dx%d' % s)
def test_split_k(pkg, shape, slabs):
    """forced slab counts: the ragged <0, 0, 0> slabs, then the scalar sum with b', the residual and the ReLU"""
    cin, cout, h, w = shape
    conv, bn = _layer(pkg, cin, cout, 3, 1, 1, seed=cin + slabs)
    x = torch.randn(2, cin, h, w, device='cuda')
    L = pkg._lib.lib()
    d = pkg.ops._desc(tuple(x.shape), tuple(conv.weight.shape), 1, 1, 1)
    unsplit = L.p3d_fx_conv_fwd_infer_any_workspace_bytes(ctypes.byref(d))
    L.p3d_fx_tune(1, slabs)
    try:
        assert L.p3d_fx_conv_fwd_infer_any_workspace_bytes(ctypes.byref(d)) >= slabs * 2 * cout * h * w * 4      # the plan really has that many slabs
        _four_epilogues(pkg, conv, bn, x, seed=slabs)
    finally:
        L.p3d_fx_tune(1, 0)
    assert L.p3d_fx_conv_fwd_infer_any_workspace_bytes(ctypes.byref(d)) == unsplit


# ---- 3. accumulate ---------------------------------------------------------------------------------------------------------------------------
def test_fusion_second_window_accumulates(pkg):
    """the Fusion 1x1 at 33^2: x's window without b', then y's window accumulated onto it with b' and the ReLU (accumulate = 1)"""
    fnet, _ = _net(pkg, 'fusionnet', 'resnet18', seed=3)
    fn = pkg.infer.fold(fnet, any_size=True)
    half = fnet.fusion.conv.weight.shape[1] // 2
    a = torch.randn(3, half, 33, 33, device='cuda')
    b = torch.randn(3, half, 33, 33, device='cuda')
    pkg.ops.conv_path_stats(reset=True)
    got = fn._fusion(a, b)
    stats = pkg.ops.conv_path_stats(reset=True)
    want = _conv64(torch.cat([a, b], 1), fnet.fusion.conv, fnet.fusion.bn, relu=True)
    assert _rel(got, want) < 2e-5
    assert stats['x3']['fwd'][0] == 2 and stats['fp32']['fwd'][0] == 0, stats


# ---- 4. no stray writes ----------------------------------------------------------------------------------------------------------------------
def _call_any(pkg, fc, d, x, res, relu, y, ws, ws_bytes):
    L, ops, c = pkg._lib.lib(), pkg.ops, fc.convs[0]
    pkg._lib.check(L.p3d_fx_conv_fwd_infer_any(ctypes.byref(d), ops._p(x), fc._at(c.img_off), c.img_bytes, fc._at(c.bias_off), ops._p(res), int(relu), ops._p(y),
                                               ops._p(ws), ws_bytes, ops._stream()), 'p3d_fx_conv_fwd_infer_any')


@pytest.mark.parametrize('shape,slabs', [((64, 256, 65, 65, 1, 3), 0), ((128, 128, 17, 19, 3, 3), 0), ((512, 512, 17, 19, 3, 2), 3), ((128, 128, 17, 17, 3, 1), 2)],
                         ids=['1x1_65x65_n3', '3x3_17x19_n3', '3x3_17x19_n2_3slabs', '3x3_17x17_n1_2slabs'])
def test_no_write_outside_y_or_the_workspace(pkg, shape, slabs):
    """y and the workspace are views into larger buffers filled with a sentinel; what lies in front of and behind each view is unchanged afterwards
    (plain reads of ordinary memory).  The bands are two images of y wide (2 K OH OW elements), so a store with an image or channel index one too high or too
    low still lands inside a band"""
    cin, cout, h, w, r, n = shape
    conv, bn = _layer(pkg, cin, cout, r, 1, 1, seed=h + w)
    fc = pkg.infer.FoldedConv(conv, bn, any_size=True)
    x = torch.randn(n, cin, h, w, device='cuda')
    res = torch.randn(n, cout, h, w, device='cuda')
    L = pkg._lib.lib()
    d = pkg.ops._desc(tuple(x.shape), tuple(conv.weight.shape), 1, (r - 1) // 2, 1)
    L.p3d_fx_tune(1, slabs)
    try:
        need = L.p3d_fx_conv_fwd_infer_any_workspace_bytes(ctypes.byref(d))
        numel = n * cout * h * w
        guard = (2 * cout * h * w + 63) // 64 * 64                  # (a multiple of 64: the views stay 16-B aligned)
        ybig = torch.full((guard + numel + guard,), -12345.0, device='cuda')
        y = ybig[guard:guard + numel].view(n, cout, h, w)
        wguard = 4 * guard
        wbig = torch.full((wguard + need + wguard,), 0xA5, dtype=torch.uint8, device='cuda')
        ws = wbig[wguard:wguard + need]
        assert y.data_ptr() % 16 == 0 and ws.data_ptr() % 16 == 0
        _call_any(pkg, fc, d, x, res, True, y, ws, need)
        torch.cuda.synchronize()
    finally:
        L.p3d_fx_tune(1, 0)
    assert _rel(y, _conv64(x, conv, bn, res, True)) < 2e-5
    assert bool((ybig[:guard] == -12345.0).all()) and bool((ybig[guard + numel:] == -12345.0).all())
    assert bool((wbig[:wguard] == 0xA5).all()) and bool((wbig[wguard + need:] == 0xA5).all())


# ---- 5. aligned shapes through the new entry ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cls', [(64, 64, 256, 1, 1, 1), (128, 64, 128, 3, 2, 1), (512, 16, 512, 3, 1, 2), (1024, 16, 2048, 1, 1, 1)],
                         ids=lambda c: 'c%d_%d_k%d_%dx%d_s%d_d%d' % (c[0], c[1], c[2], c[3], c[3], c[4], c[5]))
def test_aligned_shapes_through_the_any_entry(pkg, cls):
    """256^2-chain shapes, which p3d_fx_conv_fwd_infer takes too, straight into p3d_fx_conv_fwd_infer_any: the ragged address arithmetic where every group of four
    pixels is one aligned 16-B line"""
    cin, hw, cout, k, stride, dil = cls
    conv, bn = _layer(pkg, cin, cout, k, stride, dil, seed=cin + k)
    fc = pkg.infer.FoldedConv(conv, bn, any_size=True)
    x = torch.randn(2, cin, hw, hw, device='cuda')
    ho = (hw - 1) // stride + 1
    res = torch.randn(2, cout, ho, ho, device='cuda')
    L = pkg._lib.lib()
    d = pkg.ops._desc(tuple(x.shape), tuple(conv.weight.shape), stride, conv.padding[0], dil)
    assert L.p3d_fx_conv_fwd_infer_supported(ctypes.byref(d), 0) == 1 and L.p3d_fx_conv_fwd_infer_any_supported(ctypes.byref(d)) == 1
    need = max(L.p3d_fx_conv_fwd_infer_any_workspace_bytes(ctypes.byref(d)), 16)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    pkg.ops.conv_path_stats(reset=True)
    for with_res, relu in EPILOGUES:
        y = torch.full((2, cout, ho, ho), float('nan'), device='cuda')
        rr = res if with_res else None
        _call_any(pkg, fc, d, x, rr, relu, y, ws, need)
        assert _rel(y, _conv64(x, conv, bn, rr, relu)) < 2e-5, (with_res, relu)
    stats = pkg.ops.conv_path_stats(reset=True)
    assert stats['x3']['fwd'][0] == 4 and stats['fp32']['fwd'][0] == 0, stats


# ---- 6. whole networks -------------------------------------------------------------------------------------------------------------------------
NETS = [('depthnet', 'resnet18', ()), ('depthnet', 'resnet50', ()), ('depthnet', 'resnet18', ('-depth_only',)), ('depthnet', 'resnet50', ('-early_dist', '-skip_relu')),
        ('resnet', 'resnet18', ('-joint_space',)), ('fusionnet', 'resnet18', ())]
# dense convs behind the stems: ResNet-18 16 + 3 downsamples, ResNet-50 48 + 4; the fusion network has two more layer1 / layer2 branches and the Fusion 1x1's
# two windows; + the heads
CONVS = {('depthnet', 'resnet18'): 19 + 1, ('depthnet', 'resnet50'): 52 + 1, ('resnet', 'resnet18'): 19 + 2, ('fusionnet', 'resnet18'): 19 + 9 + 2 + 1}


@pytest.mark.parametrize('hw', [(129, 129), (257, 257), (129, 193)], ids=lambda hw: '%dx%d' % hw)
@pytest.mark.parametrize('family,model,extra', NETS, ids=lambda v: v if isinstance(v, str) else ''.join(v))
def test_whole_network(pkg, family, model, extra, hw):
    """fold(net, any_size=True) and the unfolded eval forward against the float64 forward at the bounds of test_infer_gpu.whole_network_case.  Counters: at an odd
    side the 7x7 stems stay on _trunk.stem (the space-to-depth stem needs even sides), one fp32-MFMA forward launch each -- one stem, two for the fusion
    network -- and the legacy network's 17-channel mat_regressor (K < 32) stays on its module, one more; every other conv is an x3 launch.  fold(net) without the
    keyword keeps the parent's counters: no x3 launch, every conv on the fp32-MFMA fallback."""
    h, w = hw
    net, args = _net(pkg, family, model, *extra, side=128, seed=len(extra))
    g = torch.Generator(device='cuda').manual_seed(0)
    x = torch.randn(2, 1 if args.depth_only else 3, h, w, device='cuda', generator=g)
    y = torch.rand(2, 1, h, w, device='cuda', generator=g) if family == 'fusionnet' else None
    xin = (x,) if y is None else (x, y)
    fn = pkg.infer.fold(net, any_size=True)
    pkg.ops.conv_path_stats(reset=True)
    got = fn(*xin)
    stats = pkg.ops.conv_path_stats(reset=True)
    plain = pkg.infer.fold(net)(*xin)
    default = pkg.ops.conv_path_stats(reset=True)
    with torch.no_grad():
        old = net(*xin)
        want = _forward64(net, family, x, y)
    got, plain, old, want = [t if isinstance(t, tuple) else (t,) for t in (got, plain, old, want)]
    assert len(got) == len(old) == len(want) == len(plain)
    for gt, pt, ot, wt in zip(got, plain, old, want):
        assert gt.shape == ot.shape == wt.shape == pt.shape
        print('anysize net', family, model, extra, hw, 'folded %.3e unfolded %.3e folded-vs-unfolded %.3e' % (_rel(gt, wt), _rel(ot, wt), _rel(gt, ot)))
        assert _rel(gt, wt) < 1e-4 and _rel(ot, wt) < 1e-4
        assert _rel(gt, ot) < 1e-4
        assert _rel(pt, wt) < 1e-4
    print('anysize net counters', family, model, extra, hw, stats, default)
    stems = 2 if family == 'fusionnet' else 1
    left = stems + (1 if family == 'resnet' else 0)              # the stems, and the legacy network's mat_regressor
    convs = CONVS[(family, model)]
    assert stats['fp32']['fwd'][0] == left, stats
    assert stats['x3']['fwd'][0] == convs + stems - left, stats
    assert default['x3']['fwd'][0] == 0 and default['fp32']['fwd'][0] == convs + stems, default


@pytest.mark.parametrize('hw', [(129, 129), (257, 257)], ids=lambda hw: '%dx%d' % hw)
def test_whole_partial_network(pkg, hw):
    """partial_depthnet through fold(net, any_size=True) at an odd side, what Trainer._fold now builds for the partial families: the masked stem and the partial
    layers stay on the module path (p3d_stem_masked_supported and the masked entry refuse odd maps), the dense layer3 / layer4 and the head run on the ragged
    kernels.  Bounds of whole_network_case; the dense convs -- layer2's downsample (every shortcut is dense), layer3 (4 + 1 downsample), layer4 (4 + 1) and
    the regressor -- are the 12 x3 launches."""
    h, w = hw
    net, args = _net(pkg, 'partial_depthnet', 'resnet18', '-depth_only', side=128, seed=1)
    g = torch.Generator(device='cuda').manual_seed(0)
    x = torch.randn(2, 1, h, w, device='cuda', generator=g) * (torch.rand(2, 1, h, w, device='cuda', generator=g) > 0.3)
    fn = pkg.infer.fold(net, any_size=True)
    pkg.ops.conv_path_stats(reset=True)
    got = fn(x)
    stats = pkg.ops.conv_path_stats(reset=True)
    with torch.no_grad():
        old = net(x)
        want = _forward64(net, 'partial_depthnet', x)
    for gt, ot, wt in zip(got, old, want):
        print('anysize partial net', hw, 'folded %.3e unfolded %.3e folded-vs-unfolded %.3e' % (_rel(gt, wt), _rel(ot, wt), _rel(gt, ot)))
        assert gt.shape == ot.shape == wt.shape
        assert _rel(gt, wt) < 1e-4 and _rel(ot, wt) < 1e-4 and _rel(gt, ot) < 1e-4
    print('anysize partial net counters', hw, stats)
    assert stats['x3']['fwd'][0] == 12, stats


# ---- 7. Trainer --------------------------------------------------------------------------------------------------------------------------------
def test_trainer_test_at_257_matches_the_unfolded_run(pkg, tmp_path, monkeypatch):
    """Trainer.test at the default -side_in 257 with and without P3D_FOLDED_EVAL=1: the same record, at the tolerances of
    test_trainer_folded_test_matches_reference; the folded run is on the x3 forward"""
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
                               '-num_joints', '17', '-side_in', '257', '-metadata', str(meta)])
        model, _ = pkg.depth_main.create_model(args)
        det = pkg.synth.det_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 0)
        model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in det.items()})
        trainer = pkg.depth_train.Trainer(args, model.cuda(), pkg.utils.get_info())
        trainer.verbose = False
        pkg.ops.conv_path_stats(reset=True)
        records.append(trainer.test(1, batches))
        counters.append(pkg.ops.conv_path_stats(reset=True))
        assert (trainer.__dict__.get('_folded_model') is not None) == (on == '1')
    want, record = records
    print('anysize trainer', want, record, counters)
    assert counters[1]['x3']['fwd'][0] > 0, counters             # the folded run is on the x3 forward
    assert set(record) == set(want)
    assert record['test_loss'] == pytest.approx(want['test_loss'], rel=1e-3)
    assert record['cam_mean'] == pytest.approx(want['cam_mean'], rel=1e-3)
    for k in ('score_pck', 'score_auc', 'solid', 'close', 'depth', 'jitter', 'switch', 'fail'):
        assert record[k] == pytest.approx(want[k], abs=2e-3), k


def test_distill_step_with_folded_teacher_at_129(pkg, monkeypatch):
    """one distill_step with the eval-mode fusion teacher folded (any_size) and unfolded at 129^2, at the bound of test_distill_step_with_folded_teacher"""
    results = []
    for on in ('0', '1'):
        monkeypatch.setenv('P3D_FOLDED_EVAL', on)
        args = pkg.opts.parse(['-model', 'resnet18', '-suffix', 't', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1',
                               '-num_joints', '17', '-side_in', '129', '-do_teach', '-do_fusion'])
        student = pkg.depthnet.resnet18(args, False)
        teacher = pkg.fusionnet.resnet18(args, False)
        for net, seed in ((student, 0), (teacher, 1)):
            det = pkg.synth.det_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed)
            net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in det.items()})
        teacher = ti._stats_(teacher.cuda(), 2).eval()
        trainer = pkg.depth_train.Trainer(args, student.cuda(), pkg.utils.get_info())
        trainer.set_teacher(teacher)
        trainer.verbose = False
        c, d, tc, tv = (torch.from_numpy(a).cuda() for a in pkg.synth.make_batch(2, side=129, rank=11, step=0))
        att = torch.rand(2, 1, 9, 9, generator=torch.Generator().manual_seed(4)).cuda()          # 129 -> 65 -> 33 -> 17 -> 9
        pkg.ops.conv_path_stats(reset=True)
        cam, dist = trainer.distill_step(1, c, d, tc, tv, att)
        stats = pkg.ops.conv_path_stats(reset=True)
        assert (trainer.folded_teacher is not None) == (on == '1')
        if on == '1':
            assert stats['x3']['fwd'][0] >= 31, stats           # the folded teacher's dense convs (test_whole_network: 31 for the fusion ResNet-18)
        results.append((float(cam), float(dist), student.state_dict()['regressor.weight'].detach().clone()))
    (c0, d0, w0), (c1, d1, w1) = results
    print('anysize distill', c0, c1, d0, d1, float((w1 - w0).abs().max()))
    assert c1 == pytest.approx(c0, rel=1e-4) and d1 == pytest.approx(d0, rel=1e-4)
    assert float((w1 - w0).abs().max()) < 3e-5
