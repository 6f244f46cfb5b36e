"""MXFP8 activation tensors between the fp8 convolutions (infer.fold_fp8(model, resident=True), p3d_f8conv2d_fwd_infer_mx).

The oracle is p3d_f8conv2d_fwd_infer on the same operands, bit for bit: a block quantized in a conv's epilogue is the block the next conv's quantizer
makes from the stored fp16 value.  Producer (fp16 and MX results of one launch, and the MX result alone, against the old entry's fp16 result and its
emulated quantization), consumer (an MX input packed on the host side by the emulation), a chain of the two, the epilogue quantizer on adversarial blocks,
exact-size fenced MX buffers, whole networks against fold_fp8(net), which entry is called in which form, refresh() and the Trainer switch."""
import ctypes
import json

import numpy as np
import pytest
import torch

from conftest import golden_path
from fenced import Fence
from mxfp8_emul import quantize
from test_infer_fp8_gpu import NETS, _conv_case, _fp16_blocks, _run, _same_fp8
from test_infer_gpu import _net
from test_infer_half_gpu import _find, _inputs

pytestmark = pytest.mark.gpu

# (Cin, map side, K, filter, stride, dilation, n)
CASES = [(64, 17, 64, 1, 1, 1, 2),          # narrow M <= 64, pixel tail of 66
         (64, 33, 128, 3, 2, 1, 2),         # stride-2 padding
         (128, 16, 256, 3, 1, 2, 2),        # dilation
         (96, 20, 160, 3, 2, 2, 3),         # odd block count: a half-empty last K-step; second M tile with 32 live channels
         (256, 9, 192, 1, 1, 1, 3),         # M tile with 64 live channels, one epilogue pass
         (256, 9, 1024, 1, 1, 1, 3)]        # many M tiles
_ID = lambda c: 'c%d_%d_k%d_%dx%d_s%d_d%d_n%d' % (c[0], c[1], c[2], c[3], c[3], c[4], c[5], c[6])
_CACHE = {}


def _pack_mx(x16):
    """the MXFP8 activation tensor of an fp16 NHWC activation (an NCHW view), by the emulation: elements [pixel][C], then scale bytes [pixel][C / 32]"""
    q, byte, _ = quantize(x16.float().permute(0, 2, 3, 1))
    return torch.cat([q.contiguous().view(torch.uint8).reshape(-1), byte.reshape(-1)])


def _split_mx(y_mx, n, k, ho, wo):
    pix = n * ho * wo
    return y_mx[:pix * k].view(n, ho, wo, k), y_mx[pix * k:].view(n, ho, wo, k // 32)


def _assert_mx_of(y_mx, y16):
    """y_mx is the emulated quantization of the fp16 NHWC result y16 (an NCHW view): scale bytes equal, elements equal up to the sign of a zero"""
    n, k, ho, wo = y16.shape
    q, byte, _ = quantize(y16.float().permute(0, 2, 3, 1))
    el, sc = _split_mx(y_mx, n, k, ho, wo)
    assert torch.equal(sc, byte)
    assert _same_fp8(el, q.contiguous().view(torch.uint8))
    return el, sc


def _run_mx(pkg, shape, x16, x_mx, img, bias, k, r, stride, pad, dil, res=None, relu=False, mask_in=None, mult=None, fp16=True, mx=True, y_mx=None):
    """p3d_f8conv2d_fwd_infer_mx on an input of NCHW `shape` given as x16 or as x_mx: (y fp16 or None, y_mx or None)"""
    L = pkg._lib.lib()
    n, c, h, w = shape
    d = pkg.ops._desc((n, c, h, w), (k, c, r, r), stride, pad, dil)
    assert L.p3d_f8conv2d_fwd_infer_mx_supported(ctypes.byref(d), int(x_mx is not None), int(mx)) == 1, L.p3d_last_error()
    y = torch.empty((n, k, d.Ho, d.Wo), dtype=torch.float16, device='cuda', memory_format=torch.channels_last) if fp16 else None
    if mx and y_mx is None:
        y_mx = torch.empty(L.p3d_f8act_bytes(n * d.Ho * d.Wo, k), dtype=torch.uint8, device='cuda')
    p = pkg.ops._p
    pkg._lib.check(L.p3d_f8conv2d_fwd_infer_mx(ctypes.byref(d), p(x16), p(x_mx), p(img), p(bias), p(mask_in), p(mult), p(res), int(relu), p(y),
                                               p(y_mx) if mx else None, pkg.ops._stream()), 'p3d_f8conv2d_fwd_infer_mx')
    return y, (y_mx if mx else None)


def _case(pkg, case):
    """operands of a case and the old entry's results, computed once: ((res, relu) -> y_old)"""
    if case not in _CACHE:
        cin, hw, cout, k, stride, dil, n = case
        conv, q, sc, img, bias, x16 = _conv_case(pkg, cin, hw, cout, k, stride, dil, n, seed=cin + cout + k)
        pad = conv.padding[0]
        ho = (hw + 2 * pad - dil * (k - 1) - 1) // stride + 1
        res16 = pkg.ops_half.to_half_nhwc(torch.randn(n, cout, ho, ho, device='cuda'), cout)
        old = [(res, relu, _run(pkg, x16, img, bias, cout, k, stride, pad, dil, res, relu)) for res, relu in ((None, False), (res16, True))]
        _CACHE[case] = (img, bias, x16, pad, old)
    return _CACHE[case]


# ---- 1. producer -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=_ID)
def test_producer_fp16_and_mx_results(pkg, case):
    cin, hw, cout, k, stride, dil, n = case
    img, bias, x16, pad, old = _case(pkg, case)
    for res, relu, y_old in old:
        y, y_mx = _run_mx(pkg, x16.shape, x16, None, img, bias, cout, k, stride, pad, dil, res, relu)
        assert torch.equal(y, y_old)
        _assert_mx_of(y_mx, y_old)
        none, only = _run_mx(pkg, x16.shape, x16, None, img, bias, cout, k, stride, pad, dil, res, relu, fp16=False)
        assert none is None
        _assert_mx_of(only, y_old)


# ---- 2. consumer -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=_ID)
def test_consumer_reads_a_host_packed_mx_input(pkg, case):
    cin, hw, cout, k, stride, dil, n = case
    img, bias, x16, pad, old = _case(pkg, case)
    x_mx = _pack_mx(x16)
    assert x_mx.numel() == pkg._lib.lib().p3d_f8act_bytes(n * hw * hw, cin)
    for res, relu, y_old in old:
        y, _ = _run_mx(pkg, x16.shape, None, x_mx, img, bias, cout, k, stride, pad, dil, res, relu, mx=False)
        assert torch.equal(y, y_old)


@pytest.mark.parametrize('k,stride', [(3, 1), (1, 2)], ids=['3x3', '1x1_s2'])
def test_consumer_mask_in_and_mult(pkg, k, stride):
    cin, hw, cout, n = 64, 33, 128, 2
    conv, q, sc, img, bias, x16 = _conv_case(pkg, cin, hw, cout, k, stride, 1, n, seed=7 + k)
    pad = conv.padding[0]
    mask = (torch.rand(n, 1, hw, hw, device='cuda') > 0.4).float()
    mask[0, 0, :9, :9] = 0
    mult, _ = pkg.ops.mask_count(mask, k, stride, pad, 1)
    res16 = pkg.ops_half.to_half_nhwc(torch.randn(n, cout, mult.shape[2], mult.shape[2], device='cuda'), cout)
    x_mx = _pack_mx(x16)
    for res, relu in ((None, True), (res16, False)):
        y_old = _run(pkg, x16, img, bias, cout, k, stride, pad, 1, res, relu, mask_in=mask, mult=mult)
        y, y_mx = _run_mx(pkg, x16.shape, None, x_mx, img, bias, cout, k, stride, pad, 1, res, relu, mask_in=mask, mult=mult)
        assert torch.equal(y, y_old)
        _assert_mx_of(y_mx, y_old)


# ---- 3. chain ----------------------------------------------------------------------------------------------------------------------------
def test_chain_mx_only_link(pkg):
    """conv A (64 -> 128, 3x3 stride 2, side 33 -> 17) writes MX only, conv B (128 -> 256, 3x3 dilation 2) reads it and writes both forms"""
    img_a, bias_a, x16, pad_a, old = _case(pkg, CASES[1])
    ya_old = old[1][2]
    conv_b, _, _, img_b, bias_b, _ = _conv_case(pkg, 128, 17, 256, 3, 1, 2, 2, seed=31)
    res_b = pkg.ops_half.to_half_nhwc(torch.randn(2, 256, 17, 17, device='cuda'), 256)
    yb_old = _run(pkg, ya_old, img_b, bias_b, 256, 3, 1, 2, 2, res_b, True)
    none, ya_mx = _run_mx(pkg, x16.shape, x16, None, img_a, bias_a, 128, 3, 2, pad_a, 1, old[1][0], True, fp16=False)
    yb, yb_mx = _run_mx(pkg, ya_old.shape, None, ya_mx, img_b, bias_b, 256, 3, 1, 2, 2, res_b, True)
    assert none is None and torch.equal(yb, yb_old)
    _assert_mx_of(yb_mx, yb_old)


# ---- 4. the epilogue quantizer on adversarial blocks -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('c,k,side', [(128, 1, 16), (96, 1, 17), (128, 3, 17)], ids=['c128_1x1', 'c96_1x1_odd', 'c128_3x3_odd'])
def test_epilogue_quantizer_bit_exact(pkg, c, k, side):
    """An identity conv passes fp16(dequantize(quantize(x))) of the six block kinds of _fp16_blocks to the epilogue; its MX result against the emulation
    of the old entry's output.  The populations are asserted on the emulation first (they are properties of the generator), then on the result bytes."""
    from test_infer_fp8_gpu import _emul_image
    x = _fp16_blocks(2, c, side, side, seed=c + k).cuda()
    w = torch.zeros(c, c, k, k, device='cuda')
    w[:, :, k // 2, k // 2] = torch.eye(c, device='cuda')
    q, sc = _emul_image(w)
    img = torch.cat([q.reshape(-1), sc.reshape(-1)])
    x16 = pkg.ops_half.to_half_nhwc(x, c)
    bias = torch.zeros(c, device='cuda')
    y_old = _run(pkg, x16, img, bias, c, k, 1, k // 2, 1)
    want_q, want_s, _ = quantize(y_old.float().permute(0, 2, 3, 1))
    wb = want_q.contiguous().view(torch.uint8) & 0x7f
    assert (wb == 0x7e).sum() > 1000 and ((wb > 0) & (wb < 8)).sum() > 1000 and (want_s == 0).sum() > 100
    for fp16 in (True, False):
        y, y_mx = _run_mx(pkg, x16.shape, x16, None, img, bias, c, k, 1, k // 2, 1, fp16=fp16)
        assert y is None or torch.equal(y, y_old)
        el, s = _assert_mx_of(y_mx, y_old)
        eb = el & 0x7f
        assert (eb == 0x7e).sum() > 1000 and ((eb > 0) & (eb < 8)).sum() > 1000 and (s == 0).sum() > 100      # 448s, e4m3 subnormals, zero blocks


# ---- 5. bounds ---------------------------------------------------------------------------------------------------------------------------
def test_mx_buffers_of_exact_size(pkg):
    """x_mx and y_mx as exact-size buffers between fences, y_mx poisoned: nothing outside is written, every byte inside is (no element and no scale byte
    of a result is 0xFF: e4m3 NaN and E8M0 NaN), and reading x_mx up to its last byte gives the old entry's result"""
    case = CASES[3]
    cin, hw, cout, k, stride, dil, n = case
    img, bias, x16, pad, old = _case(pkg, case)
    res, relu, y_old = old[1]
    L = pkg._lib.lib()
    packed = _pack_mx(x16)
    fx = Fence(L.p3d_f8act_bytes(n * hw * hw, cin), 4096, 'cuda')
    assert fx.nbytes == packed.numel()
    fx.view.copy_(packed)
    fy = Fence(L.p3d_f8act_bytes(y_old.shape[0] * y_old.shape[2] * y_old.shape[3], cout), 4096, 'cuda')
    y, y_mx = _run_mx(pkg, x16.shape, None, fx.view, img, bias, cout, k, stride, pad, dil, res, relu, y_mx=fy.view)
    torch.cuda.synchronize()
    fx.check('x_mx')
    fy.check('y_mx')
    assert torch.equal(fx.view, packed)
    assert bool((fy.view != fy.poison).all())
    assert torch.equal(y, y_old)
    _assert_mx_of(fy.view, y_old)


# ---- 6. whole networks -------------------------------------------------------------------------------------------------------------------
RESIDENT_NETS = [n for n in NETS if n[1] == 'resnet18'] + [('depthnet', 'resnet50', (), 129, 2), ('fusionnet', 'resnet50', (), 128, 2)]
# depthnet: (convs that are neither stem nor head, of them fed by the pool, interior chain outputs)
COUNTS = {'resnet18': (19, 1, 8), 'resnet50': (52, 2, 32)}


@pytest.mark.parametrize('family,model,extra,side,n', RESIDENT_NETS, ids=lambda v: v if isinstance(v, str) else ''.join(v) if isinstance(v, tuple) else str(v))
def test_resident_network_bit_equal_to_fold_fp8(pkg, monkeypatch, family, model, extra, side, n):
    net, args = _net(pkg, family, model, *extra, side=side, seed=len(extra))
    x, y = _inputs(family, args, n, side)
    want = pkg.infer.fold_fp8(net)(*((x,) if y is None else (x, y)))
    rs = pkg.infer.fold_fp8(net, resident=True)
    assert isinstance(rs, pkg.infer.Fp8FoldedNet)
    calls = {'old': 0, 'new': []}
    L = pkg._lib.lib()
    old_fn, new_fn = L.p3d_f8conv2d_fwd_infer, L.p3d_f8conv2d_fwd_infer_mx
    monkeypatch.setattr(L, 'p3d_f8conv2d_fwd_infer', lambda *a: (calls.__setitem__('old', calls['old'] + 1), old_fn(*a))[1])
    monkeypatch.setattr(L, 'p3d_f8conv2d_fwd_infer_mx', lambda *a: (calls['new'].append((a[1], a[2], a[9], a[10])), new_fn(*a))[1])
    got = rs(*((x,) if y is None else (x, y)))
    want, got = (want if isinstance(want, tuple) else (want,)), (got if isinstance(got, tuple) else (got,))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and torch.isfinite(w).all() and torch.equal(g, w)
    assert calls['old'] == 0 and len(calls['new']) > 0
    assert all((x16 is None) != (xmx is None) and (y16 is not None or ymx is not None) for x16, xmx, y16, ymx in calls['new'])
    if family == 'depthnet':
        convs, pooled, interior = COUNTS[model]
        assert len(calls['new']) == convs
        assert sum(1 for _, xmx, _, _ in calls['new'] if xmx is not None) == convs - pooled
        assert sum(1 for _, _, y16, _ in calls['new'] if y16 is None) == interior


def test_resident_skip_relu_bit_equal_to_fold_fp8(pkg):
    """-skip_relu: the closing conv of layer3 and of layer4 without its ReLU (the feature map has negative values), ops.relu behind each, whose result is
    fp16 only, so layer4 opens on an fp16 input"""
    net, args = _net(pkg, 'depthnet', 'resnet18', '-skip_relu', side=64, seed=1)
    assert net.skip_relu and net.layer3[-1].skip_relu and net.layer4[-1].skip_relu and not net.layer4[0].skip_relu
    x, _ = _inputs('depthnet', args, 2, 64)
    want = pkg.infer.fold_fp8(net)(x)
    got = pkg.infer.fold_fp8(net, resident=True)(x)
    assert float(want[1].min()) < 0
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and torch.isfinite(w).all() and torch.equal(g, w)


# ---- 7. refresh, Trainer -------------------------------------------------------------------------------------------------------------------
def test_resident_refresh_after_optimizer_step(pkg):
    net, _ = _net(pkg, 'depthnet', 'resnet18', side=128)
    x = torch.randn(2, 3, 128, 128, device='cuda')
    rs = pkg.infer.fold_fp8(net, resident=True)
    stale = rs(x)[0]
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    net.train()
    z, feat = net(x)
    (z.square().mean() + feat.square().mean()).backward()
    opt.step()
    net.eval()
    fresh = pkg.infer.fold_fp8(net, resident=True)
    want = fresh(x)
    assert not torch.equal(stale, want[0])
    rs.refresh()
    assert torch.equal(rs.buffer, fresh.buffer)
    got = rs(x)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    plain = pkg.infer.fold_fp8(net)(x)
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])


def test_trainer_resident_switch(pkg, tmp_path, monkeypatch):
    g = np.load(golden_path('eval.npz'))
    meta = tmp_path / 'metadata.json'
    meta.write_text(json.dumps(dict(loader=dict(h36m='depth_datasets'), no_depth=dict(h36m=False),
                                    thresholds=dict(h36m=json.loads(str(g['thresh']))), root=dict(h36m=str(tmp_path)))))
    args = pkg.opts.parse(['-model', 'resnet18', '-suffix', 't', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1',
                           '-num_joints', '17', '-side_in', '128', '-metadata', str(meta), '-half_acc'])
    model, _ = pkg.depth_main.create_model(args)
    det = pkg.synth.det_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 0)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in det.items()})
    trainer = pkg.depth_train.Trainer(args, model.cuda(), pkg.utils.get_info())
    trainer.verbose = False
    batches = []
    for it in range(2):
        c, d, tc, tv = pkg.synth.make_batch(2, side=128, rank=7, step=it, invalid_frac=0.2)
        rot = np.linalg.qr(np.random.Generator(np.random.PCG64(it)).standard_normal((2, 3, 3)))[0].astype(np.float32)
        batches.append(tuple(torch.from_numpy(a) for a in (c, d, tc, tv, rot)))
    monkeypatch.setenv('P3D_FOLDED_EVAL_FP8', '1')
    monkeypatch.setenv('P3D_FOLDED_EVAL_FP8_RESIDENT', '0')
    want = trainer.test(1, batches)
    assert type(trainer._folded_fp8_model) is pkg.infer.Fp8FoldedNet
    monkeypatch.setenv('P3D_FOLDED_EVAL_FP8_RESIDENT', '1')
    runs = []
    real = pkg.infer.Fp8ResidentNet.__call__
    monkeypatch.setattr(pkg.infer.Fp8ResidentNet, '__call__', lambda self, *a: (runs.append(1), real(self, *a))[1])
    got = trainer.test(1, batches)
    assert len(runs) == len(batches) and isinstance(trainer._folded_fp8_resident_model, pkg.infer.Fp8ResidentNet)
    assert set(got) == set(want)
    for k in want:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
        assert np.all(np.isfinite(np.asarray(got[k], dtype=np.float64))), k
