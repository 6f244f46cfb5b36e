"""BatchNorm and the stem tail on 16-B kernels at any map width (ops.bn_any / p3d_bn_any_enable), on the GPU: the peeled instances of csrc/p3d_bn.hip -- a row's
head and tail element by element, its body in 16-B accesses -- against float64 and beside the element-by-element instances the same calls launch with the switch
off; the stem's maxpool(relu(bn(c))) as one node at odd sides, bit for bit against the three nodes under the same switch; one network step both ways.

Bounds: those of tests/test_kernels_gpu.py for the same entries (output 2e-5 absolute, running statistics 1e-6 / 1e-5, dx 5e-5, dgamma / dbeta 2e-5 relative, dres
to the bit; eval mode 1e-5 throughout); the network's is the one tests/test_frozen_fold_gpu.py derives for two fp32 legs of one function.  Which instance ran is
read from the library's own record (ops.bn_last_launch): 0 vector, 1 scalar, 2 peeled."""
import json

import numpy as np
import pytest
import torch

import fenced
from conftest import golden_path
from oracle import np_ops as ref

pytestmark = pytest.mark.gpu

VECTOR, SCALAR, PEELED = 0, 1, 2
TRAIN_FWD, TRAIN_BWD, EVAL_FWD, EVAL_BWD, STEM_FWD, STEM_BWD = 1, 2, 3, 4, 5, 6

# (4,3,1,1), (2,4,1,3): rows shorter than a vector; (3,5,1,5), (2,6,3,2), (3,4,7,1): HW = 1, 2, 3 mod 4 (with HW = 1 mod 4 four consecutive rows meet all four
# phases); (2,3,33,33), (1,2,65,65): 1089 and 4225 elements, past the 1024 up to which a wavefront walks a row, and past one trip of 256 lanes x 4; (5,1030,1,5): two
# blocks per channel, so a block has three images (one per wavefront; the fourth has none); (2,2048,1,3): one block per channel
SHAPES = [(4, 3, 1, 1), (2, 4, 1, 3), (3, 5, 1, 5), (2, 6, 3, 2), (3, 4, 7, 1), (2, 3, 17, 17), (3, 2, 17, 19), (2, 3, 33, 33), (1, 2, 65, 65), (5, 1030, 1, 5),
          (2, 2048, 1, 3)]
MODES = [('train', False, False), ('train', True, False), ('train', True, True), ('eval', True, False)]         # mode, ReLU, residual
_id = lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) and isinstance(v[0], int) else '-'.join(str(int(e) if isinstance(e, bool) else e) for e in v)


@pytest.fixture
def bn_any(pkg):
    """the switch, off when the body starts; what it found restored afterwards"""
    before = pkg.ops.bn_any(False)
    try:
        yield pkg.ops.bn_any
    finally:
        pkg.ops.bn_any(before)


def dev(a):
    return torch.from_numpy(np.array(a, dtype=a.dtype, order='C', copy=True)).cuda()           # (the shared references are read-only arrays)


def host(t):
    return t.detach().cpu().numpy()


def relerr(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _data(shape, with_res, seed=0):
    n, c, h, w = shape
    rng = np.random.default_rng(n * 1000 + c + seed)
    d = dict(x=(rng.standard_normal(shape) * 2 + 3).astype(np.float32), res=rng.standard_normal(shape).astype(np.float32) if with_res else None,
             gamma=(1 + 0.2 * rng.standard_normal(c)).astype(np.float32), beta=(0.3 * rng.standard_normal(c)).astype(np.float32),
             rm=rng.standard_normal(c).astype(np.float32), rv=(1 + rng.random(c)).astype(np.float32), dy=rng.standard_normal(shape).astype(np.float32))
    return d


# ---- 1. the float64 oracle, through ops.batch_norm_act ------------------------------------------------------------------------------------------------------
_REF = {}


def _reference(shape, mode, relu, with_res):
    """computed once per case, shared, never written to"""
    key = (shape, mode, relu, with_res)
    if key not in _REF:
        d = _data(shape, with_res)
        if mode == 'train':
            y, mean, invstd, nrm, nrv = ref.bn_train_fwd(d['x'], d['gamma'], d['beta'], d['rm'], d['rv'])
            pre = y + (d['res'] if with_res else 0)
            out = np.maximum(pre, 0) if relu else pre
            g = (d['dy'] * (out > 0) if relu else d['dy']).astype(np.float32)
            dx, dg, db = ref.bn_train_bwd(g, d['x'], mean, invstd, d['gamma'])
        else:
            out = np.maximum(ref.bn_eval_fwd(d['x'], d['gamma'], d['beta'], d['rm'], d['rv']), 0)
            g = (d['dy'] * (out > 0)).astype(np.float32)
            dx, dg, db = ref.bn_eval_bwd(g, d['x'], d['gamma'], d['beta'], d['rm'], d['rv'])
            nrm, nrv = d['rm'], d['rv']
        _REF[key] = dict(d, out=out, g=g, dx=dx, dg=dg, db=db, nrm=nrm, nrv=nrv)
        for v in _REF[key].values():
            if v is not None:
                v.setflags(write=False)
    return _REF[key]


@pytest.mark.parametrize('mode,relu,with_res', MODES, ids=['train_plain', 'train_relu', 'train_relu_res', 'eval_relu'])
@pytest.mark.parametrize('shape', SHAPES, ids=_id)
def test_against_float64(pkg, bn_any, shape, mode, relu, with_res):
    ops = pkg.ops
    r = _reference(shape, mode, relu, with_res)
    n, c, h, w = shape
    split = min(max(-(-2048 // c), 1), n, 64)
    if shape == (5, 1030, 1, 5):
        assert split == 2
    for on in (True, False):
        bn_any(on)
        xt, gt, bt = dev(r['x']).requires_grad_(True), dev(r['gamma']).requires_grad_(True), dev(r['beta']).requires_grad_(True)
        rt = dev(r['res']).requires_grad_(True) if with_res else None
        rmt, rvt = dev(r['rm']), dev(r['rv'])
        out = ops.batch_norm_act(xt, gt, bt, rmt, rvt, rt, relu, mode == 'train', 0.1, 1e-5)
        fwd = ops.bn_last_launch()
        out.backward(dev(r['dy']))
        torch.cuda.synchronize()
        bwd = ops.bn_last_launch()
        want = PEELED if on else SCALAR
        assert fwd == dict(entry=TRAIN_FWD if mode == 'train' else EVAL_FWD, instance=want, grid=(c, split)), (on, fwd)
        assert bwd == dict(entry=TRAIN_BWD if mode == 'train' else EVAL_BWD, instance=want, grid=(c, split)), (on, bwd)
        errs = dict(y=np.abs(host(out) - r['out']).max(), dx=relerr(host(xt.grad), r['dx']), dgamma=relerr(host(gt.grad), r['dg']),
                    dbeta=relerr(host(bt.grad), r['db']))
        print('%s %s switch %s: %s' % (shape, mode, 'on' if on else 'off', ' '.join('%s %.2e' % kv for kv in errs.items())))
        if mode == 'train':
            assert errs['y'] < 2e-5
            assert relerr(host(rmt), r['nrm']) < 1e-6 and relerr(host(rvt), r['nrv']) < 1e-5
            assert errs['dx'] < 5e-5
            assert errs['dgamma'] < 2e-5 and errs['dbeta'] < 2e-5
            if with_res:
                assert np.array_equal(host(rt.grad), r['g'])
        else:
            assert errs['y'] < 1e-5
            assert np.array_equal(host(rmt), r['rm']) and np.array_equal(host(rvt), r['rv'])
            assert errs['dx'] < 1e-5 and errs['dgamma'] < 1e-5 and errs['dbeta'] < 1e-5


# ---- 2. the entries themselves: tensors placed where the test wants them ---------------------------------------------------------------------------------------
def _place(t, shift):
    """a copy of t that starts `shift` floats behind a 16-B line"""
    room = torch.full((t.numel() + 8,), float('nan'), device='cuda')
    assert room.data_ptr() % 16 == 0
    view = room[shift:shift + t.numel()].view(t.shape)
    view.copy_(t)
    return view, room


def _out(shape, shift, fences):
    """an output of `shape`: inside a fence of its own (fences is a list), or NaNs `shift` floats behind a 16-B line"""
    if fences is not None:
        assert shift == 0
        numel = int(np.prod(shape))
        t, f = fenced.fenced_like(shape, torch.float32, 2 * numel // max(shape[0], 1) if len(shape) > 1 else 64)
        fences.append(f)
        return t
    return _place(torch.full(shape, float('nan'), device='cuda'), shift)[0]


def _entries(pkg, shape, mode, relu, with_res, shift=0, out_shift=None, fences=None, seed=0):
    """p3d_bn_train_fwd + _bwd (or the eval pair) as BatchNormActFn calls them; inputs `shift` floats behind a 16-B line, outputs out_shift (default: the same)"""
    ops, L = pkg.ops, pkg._lib.lib()
    check, p, st = pkg._lib.check, ops._p, ops._stream()
    out_shift = shift if out_shift is None else out_shift
    n, c, h, w = shape
    d = _data(shape, with_res, seed)
    x, dy = _place(dev(d['x']), shift)[0], _place(dev(d['dy']), out_shift)[0]
    res = _place(dev(d['res']), shift)[0] if with_res else None
    gamma, beta, rm, rv = dev(d['gamma']), dev(d['beta']), dev(d['rm']), dev(d['rv'])
    y = _out(shape, out_shift, fences)
    nb = L.p3d_bn_workspace_bytes(n, c, h * w)
    if fences is not None:
        fences.append(fenced.Fence(nb, 4096, 'cuda'))
        ws = fences[-1].view
    else:
        ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device='cuda')
    got = {}
    if mode == 'train':
        mean, invstd = _out((c,), 0, fences), _out((c,), 0, fences)
        check(L.p3d_bn_train_fwd(p(x), p(res), p(gamma), p(beta), p(rm), p(rv), p(y), p(mean), p(invstd), n, c, h * w, 0.1, 1e-5, int(relu), p(ws), nb, st),
              'p3d_bn_train_fwd')
        got.update(mean=mean, invstd=invstd)
    else:
        check(L.p3d_bn_eval_fwd(p(x), p(res), p(gamma), p(beta), p(rm), p(rv), p(y), n, c, h * w, 1e-5, int(relu), st), 'p3d_bn_eval_fwd')
    fwd = ops.bn_last_launch()
    dx = _out(shape, out_shift, fences)
    dres = _out(shape, out_shift, fences) if (with_res and relu) else None
    dgamma, dbeta = _out((c,), 0, fences), _out((c,), 0, fences)
    if mode == 'train':
        y_bwd = y if (relu and with_res) else None
        check(L.p3d_bn_train_bwd(p(dy), p(x), p(y_bwd), p(gamma), p(beta), p(mean), p(invstd), p(dx), p(dres), p(dgamma), p(dbeta), n, c, h * w, int(relu), 0,
                                 p(ws), nb, st), 'p3d_bn_train_bwd')
    else:
        check(L.p3d_bn_eval_bwd(p(dy), p(x), p(y if relu else None), p(gamma), p(rm), p(rv), p(dx), p(dres), p(dgamma), p(dbeta), n, c, h * w, 1e-5, int(relu), 0,
                                p(ws), nb, st), 'p3d_bn_eval_bwd')
    bwd = ops.bn_last_launch()
    torch.cuda.synchronize()
    got.update(y=y, rm=rm, rv=rv, dx=dx, dgamma=dgamma, dbeta=dbeta)
    if dres is not None:
        got['dres'] = dres
    return got, fwd['instance'], bwd['instance'], d


def _check_against_float64(got, d, mode, relu, with_res):
    x, dy = d['x'], d['dy']
    if mode == 'train':
        y, mean, invstd, nrm, nrv = ref.bn_train_fwd(x, d['gamma'], d['beta'], d['rm'], d['rv'])
        out = y + (d['res'] if with_res else 0)
        out = np.maximum(out, 0) if relu else out
        g = (dy * (out > 0) if relu else dy).astype(np.float32)
        dx, dg, db = ref.bn_train_bwd(g, x, mean, invstd, d['gamma'])
        tol = dict(y=2e-5, dx=5e-5, p=2e-5)
        assert relerr(host(got['rm']), nrm) < 1e-6 and relerr(host(got['rv']), nrv) < 1e-5
    else:
        out = ref.bn_eval_fwd(x, d['gamma'], d['beta'], d['rm'], d['rv']) + (d['res'] if with_res else 0)
        out = np.maximum(out, 0) if relu else out
        g = (dy * (out > 0) if relu else dy).astype(np.float32)
        dx, dg, db = ref.bn_eval_bwd(g, x, d['gamma'], d['beta'], d['rm'], d['rv'])
        tol = dict(y=1e-5, dx=1e-5, p=1e-5)
    assert np.abs(host(got['y']) - out).max() < tol['y']
    assert relerr(host(got['dx']), dx) < tol['dx']
    assert relerr(host(got['dgamma']), dg) < tol['p'] and relerr(host(got['dbeta']), db) < tol['p']
    if 'dres' in got:
        assert np.array_equal(host(got['dres']), g)


@pytest.mark.parametrize('shape', SHAPES, ids=_id)
def test_on_against_off(pkg, bn_any, shape):
    """the element-wise results -- eval forward y, dres, eval backward dx -- are the element-by-element instance's bits; two runs with the switch on are bit-equal
    in everything"""
    for mode, relu, with_res in MODES + [('eval', True, True)]:
        bn_any(False)
        off, f0, b0, _ = _entries(pkg, shape, mode, relu, with_res)
        bn_any(True)
        on, f1, b1, _ = _entries(pkg, shape, mode, relu, with_res)
        again, _, _, _ = _entries(pkg, shape, mode, relu, with_res)
        assert (f0, b0, f1, b1) == (SCALAR, SCALAR, PEELED, PEELED), (mode, f0, b0, f1, b1)
        for k in on:
            assert torch.equal(_bits(on[k]), _bits(again[k])), (mode, relu, with_res, k)
        exact = (['y', 'dx'] if mode == 'eval' else []) + (['dres'] if 'dres' in on else [])
        for k in exact:
            assert torch.equal(_bits(on[k]), _bits(off[k])), (mode, relu, with_res, k)


@pytest.mark.parametrize('shape', [(2, 8, 4, 4), (3, 16, 8, 8)], ids=_id)
def test_aligned_shapes_keep_their_instance(pkg, bn_any, shape):
    for mode, relu, with_res in MODES:
        res = {}
        for on in (False, True):
            bn_any(on)
            res[on], f, b, _ = _entries(pkg, shape, mode, relu, with_res)
            assert (f, b) == (VECTOR, VECTOR), (on, mode, f, b)
        for k in res[True]:
            assert torch.equal(_bits(res[True][k]), _bits(res[False][k])), (mode, k)


@pytest.mark.parametrize('shape', [(3, 5, 1, 5), (2, 3, 17, 17), (2, 8, 4, 4), (2, 3, 33, 33)], ids=_id)
def test_offset_views(pkg, bn_any, shape):
    """all tensors 1, 2, 3 floats behind a 16-B line: one peel serves them, instance 2 -- an aligned shape too, which vec_ok refuses for the pointers' sake --;
    x off by one float while y is not: no common peel, instance 1.  Either way the results hold the float64 bounds and the aligned placement's element-wise bits"""
    bn_any(True)
    for mode, relu, with_res in MODES:
        base, _, _, _ = _entries(pkg, shape, mode, relu, with_res)
        for shift in (1, 2, 3):
            got, f, b, d = _entries(pkg, shape, mode, relu, with_res, shift=shift)
            assert (f, b) == (PEELED, PEELED), (mode, shift, f, b)
            _check_against_float64(got, d, mode, relu, with_res)
            if mode == 'eval':
                assert torch.equal(_bits(got['y']), _bits(base['y'])) and torch.equal(_bits(got['dx']), _bits(base['dx'])), (mode, shift)
        got, f, b, d = _entries(pkg, shape, mode, relu, with_res, shift=1, out_shift=0)
        assert (f, b) == (SCALAR, SCALAR), (mode, f, b)
        _check_against_float64(got, d, mode, relu, with_res)


@pytest.mark.parametrize('shape', [(3, 5, 1, 5), (2, 3, 17, 17), (2, 3, 33, 33)], ids=_id)
def test_fences(pkg, bn_any, shape):
    """outputs and workspace exact-size, poisoned and banded: nothing outside is written, nothing unwritten is read, and the bits are those of plain buffers"""
    bn_any(True)
    for mode, relu, with_res in MODES:
        fences = []
        got, f, b, d = _entries(pkg, shape, mode, relu, with_res, fences=fences)
        assert (f, b) == (PEELED, PEELED)
        for fence in fences:
            fence.check('%s %s' % (shape, mode))
        _check_against_float64(got, d, mode, relu, with_res)
        plain, _, _, _ = _entries(pkg, shape, mode, relu, with_res)
        for k in got:
            assert torch.equal(_bits(got[k]), _bits(plain[k])), (mode, k)


# ---- 3. the stem tail ----------------------------------------------------------------------------------------------------------------------------------------
STEMS = [(2, 3, 9, 9), (1, 4, 5, 7), (2, 2, 8, 9), (2, 2, 9, 8), (1, 2, 3, 3), (1, 2, 2, 2), (1, 2, 129, 129)]


def _stem_inputs(shape):
    n, c, h, w = shape
    gen = torch.Generator(device='cuda').manual_seed(h * 7 + w)
    x0 = torch.randn(n, c, h, w, device='cuda', generator=gen)
    x0 = (x0 * 2).round() / 2                                 # values on a coarse grid: plenty of exact ties inside the pooling windows
    dy = torch.randn(n, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1, device='cuda', generator=gen)
    return x0, dy


def _stem_bn(pkg, c):
    torch.manual_seed(1)
    bn = pkg.nn.BatchNorm2d(c).cuda().train()
    with torch.no_grad():
        bn.weight.uniform_(-1.0, 1.5); bn.bias.normal_(0, 0.3); bn.running_mean.normal_(0, 0.2); bn.running_var.uniform_(0.5, 1.5)
    return bn


@pytest.mark.parametrize('shape', STEMS, ids=_id)
def test_stem_tail_is_bit_identical_to_batchnorm_relu_maxpool(pkg, bn_any, shape):
    """the body of tests/test_kernels_gpu.py's test of the same name at sides p3d_stem_tail_supported refuses, both legs under the switch"""
    ops = pkg.ops
    n, c, h, w = shape
    x0, dy = _stem_inputs(shape)
    pool = pkg.nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
    assert not ops.stem_tail_usable(x0, _stem_bn(pkg, c), pool)         # switch off
    bn_any(True)
    res = {}
    for fused in (True, False):
        bn = _stem_bn(pkg, c)
        x = x0.clone().requires_grad_(True)
        assert ops.stem_tail_usable(x, bn, pool)
        y = ops.stem_tail(x, bn) if fused else pool(bn(x, relu=True))
        if fused:
            assert ops.bn_last_launch()['entry'] == STEM_FWD and ops.bn_last_launch()['instance'] == PEELED
        y.backward(dy)
        torch.cuda.synchronize()
        if fused:
            assert ops.bn_last_launch()['entry'] == STEM_BWD and ops.bn_last_launch()['instance'] == PEELED
        res[fused] = (y.detach().clone(), x.grad.clone(), bn.weight.grad.clone(), bn.bias.grad.clone(), bn.running_mean.clone(), bn.running_var.clone(),
                      bn.num_batches_tracked.clone())
    assert res[True][0].shape == dy.shape
    for a, b, name in zip(res[True], res[False], ('y', 'dx', 'dgamma', 'dbeta', 'running_mean', 'running_var', 'num_batches_tracked')):
        assert torch.equal(a, b), name
    assert torch.isfinite(res[True][0]).all() and torch.isfinite(res[True][1]).all()


def test_stem_tail_fenced(pkg, bn_any):
    """p3d_stem_tail_fwd / _bwd at (2,3,9,9) on exact-size, poisoned, banded y, idx, statistics, dx, parameter gradients and workspace: the node's own bits"""
    ops, L = pkg.ops, pkg._lib.lib()
    check, p, st = pkg._lib.check, ops._p, ops._stream()
    shape = n, c, h, w = (2, 3, 9, 9)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    x0, dy = _stem_inputs(shape)
    bn_any(True)
    bn = _stem_bn(pkg, c)
    x = x0.clone().requires_grad_(True)
    want_y = ops.stem_tail(x, bn)
    want_y.backward(dy)
    torch.cuda.synchronize()
    bn2 = _stem_bn(pkg, c)
    fences = []

    def out(shp, dtype=torch.float32):
        t, f = fenced.fenced_like(shp, dtype, 256)
        fences.append(f)
        return t
    y, idx, mean, invstd = out((n, c, ho, wo)), out((n, c, ho, wo), torch.uint8), out((c,)), out((c,))
    dx, dgamma, dbeta = out(shape), out((c,)), out((c,))
    nb = L.p3d_bn_workspace_bytes(n, c, h * w)
    fences.append(fenced.Fence(nb, 4096, 'cuda'))
    ws = fences[-1].view
    rm, rv = bn2.running_mean, bn2.running_var
    check(L.p3d_stem_tail_fwd(p(x0), p(bn2.weight), p(bn2.bias), p(rm), p(rv), p(y), p(idx), p(mean), p(invstd), n, c, h, w, 0.1, bn2.eps, p(ws), nb, st),
          'p3d_stem_tail_fwd')
    check(L.p3d_stem_tail_bwd(p(dy), p(idx), p(x0), p(bn2.weight), p(bn2.bias), p(mean), p(invstd), p(dx), p(dgamma), p(dbeta), n, c, h, w, 0, p(ws), nb, st),
          'p3d_stem_tail_bwd')
    torch.cuda.synchronize()
    for f in fences:
        f.check('stem tail')
    assert int(idx.max()) <= 8
    for a, b, name in ((y, want_y, 'y'), (dx, x.grad, 'dx'), (dgamma, bn.weight.grad, 'dgamma'), (dbeta, bn.bias.grad, 'dbeta'), (rm, bn.running_mean, 'rm'),
                       (rv, bn.running_var, 'rv')):
        assert torch.equal(_bits(a), _bits(b.detach())), name


# ---- 4. one network ------------------------------------------------------------------------------------------------------------------------------------------
def _network(pkg, side):
    """ResNet-18 depthnet with a trainer, every BatchNorm in training mode, from deterministic parameters"""
    flags = ['-model', 'resnet18', '-suffix', 't', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1', '-num_joints', '17', '-side_in', str(side)]
    args = pkg.opts.parse(flags)
    torch.manual_seed(0)
    model, _ = pkg.depth_main.create_model(args)
    det = pkg.synth.det_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 0)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in det.items()})
    model = model.cuda().train()
    tr = pkg.depth_train.Trainer(args, model, pkg.utils.get_info())
    tr.verbose = False
    tr.adapt_learn_rate(1)
    return model, tr


def test_one_network_step(pkg, bn_any):
    """R18 depthnet, batch 2, side 65, one training step from identical parameters with the switch on against off (x3_any off in both): the loss, the output of
    every ReLU layer and every parameter gradient within 2 x 4e-6 x sqrt(2 x convolutions) of each other relative to the tensor's largest element, on the first of
    four seeded batches without a flipped ReLU element (the pattern of tests/test_frozen_fold_gpu.py::test_whole_network)"""
    import test_frozen_fold_gpu as Z
    ops = pkg.ops
    x3_before = ops.x3_any(False)
    keep_tail = ops.stem_tail

    def leg(on, batch):
        bn_any(on)
        model, tr = _network(pkg, 65)
        relus, tails = {}, []

        def tail(x, bn):
            tails.append(tuple(x.shape))
            y = keep_tail(x, bn)
            relus['stem'] = y.detach()
            return y
        ops.stem_tail = tail
        hook = model.maxpool.register_forward_hook(lambda mod, inp, out: relus.__setitem__('stem', out.detach()))
        try:
            loss, scale, grads, _ = Z._step(pkg, model, tr, batch, False, None, relus)
        finally:
            ops.stem_tail = keep_tail
            hook.remove()
        relus.pop('bn1', None)                     # (the three-node leg only: its pooled output stands for the stem in both)
        return loss, scale, grads, relus, model, tails, ops.bn_last_launch()

    try:
        for rank in range(4):
            batch = Z._batch(pkg, 65, False, rank)
            l0, scale, g0, y0, model, tails0, _ = leg(False, batch)
            l1, _, g1, y1, model, tails1, last = leg(True, batch)
            assert tails0 == [] and tails1 == [(2, 64, 33, 33)], (tails0, tails1)          # the stem ran as one StemTailFn node
            assert last['entry'] == STEM_BWD and last['instance'] == PEELED, last
            bound = Z._network_bound(model)
            flips = Z._flips(bound, y0, y1)
            print('batch %d: %d ReLU element(s) masked by one leg only' % (rank, flips))
            if flips == 0:
                break
            assert flips <= Z.FLIPS_MOST, flips
        assert flips == 0, 'no batch without a flipped ReLU element among four'
    finally:
        ops.x3_any(x3_before)
    assert bound == pytest.approx(2 * 4e-6 * (2 * 21) ** 0.5)
    print('loss %.6f / %.6f' % (l0, l1))
    assert abs(l1 - l0) <= bound * scale
    worst = 0.0
    for name in g0:
        top = g0[name].abs().max().item()
        err = (g1[name].double() - g0[name].double()).abs().max().item()
        worst = max(worst, err / max(top, 1e-30))
        assert err <= bound * top, (name, err, top)
    print('largest gradient difference %.2e of the tensor\'s largest element (bound %.2e)' % (worst, bound))


def test_whole_step_at_an_odd_side(pkg, bn_any):
    """the reference's own step at side 257 (tests/golden/step_depth_r18_odd_b1.npz) with the switch on: the assertions and tolerances of tests/test_step_gpu.py"""
    import test_step_gpu as S
    g = np.load(golden_path('step_depth_r18_odd_b1.npz'))
    meta = json.loads(str(g['meta']))
    assert meta['iters'] == 1 and meta['side'] % 2 == 1
    args, model, trainer = S.build(pkg, meta)
    names = meta['names']
    model.train()
    trainer.adapt_learn_rate(1)
    c, d, tc, tv = pkg.synth.make_batch(meta['batch'], side=meta['side'], rank=0, step=0, invalid_frac=meta['invalid_frac'])
    zs = []
    hook = model.regressor.register_forward_hook(lambda m, i, o: zs.append(o.detach().cpu().numpy()))
    bn_any(True)
    loss = float(trainer.train_step(torch.from_numpy(c).cuda(), torch.from_numpy(d).cuda(), torch.from_numpy(tc).cuda(), torch.from_numpy(tv).cuda()))
    pkg.ops.join_side_stream()
    torch.cuda.synchronize()
    hook.remove()
    last = pkg.ops.bn_last_launch()
    assert last['entry'] == STEM_BWD and last['instance'] == PEELED, last
    assert abs(loss - g['losses'][0]) < 1e-3 * abs(g['losses'][0]), (loss, g['losses'][0])
    spec_sel = trainer.last_spec_cam.cpu().numpy().reshape(-1, 3)[tv.reshape(-1)]
    want = g['spec_sel_0']
    assert np.abs(spec_sel - want).max() < 1e-3 * np.abs(want).max()
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
