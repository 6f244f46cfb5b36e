"""Stride-2 data gradients on the x3 kernels at any map side (ops.x3_any_strided / p3d_x3_any_strided_enable), on the GPU: p3d_conv2d_dgrad of dense stride-2
convolutions at odd maps -- one ragged launch per parity class into tight class planes, then dgrad_interleave_rows_kernel -- against float64 on the same data and
beside the fp32-MFMA kernel, which the same call launches with the switch off; and the interleave kernel alone against the one it stands beside.

Bounds (tests/test_train_anysize_gpu.py): the error against float64, relative to the largest reference value, is at most 4e-6 and at most 4 x the fp32-MFMA
kernel's own on the same data.  Which kernel ran is read from the library's launch counters (ops.conv_path_stats) and the x3 launch log (ops.fx_launch_log).

Measured on an MI355X (profiles/train_anysize_strided.md): 1.4e-7 - 4.3e-7 over the six shapes of the first test, where the fp32-MFMA kernel has 1.5e-7 - 4.5e-7."""
import ctypes
import json

import numpy as np
import pytest
import torch

import fenced
from conftest import golden_path

pytestmark = pytest.mark.gpu

TOL = 4e-6
FINISH_INTERLEAVE_ROWS = 5


@pytest.fixture
def strided_on(pkg):
    """the switch on for the test body; what it found restored afterwards"""
    before = pkg.ops.x3_any_strided(True)
    try:
        yield pkg.ops.x3_any_strided
    finally:
        pkg.ops.x3_any_strided(before)


def _err(got, ref):
    return ((got.double() - ref).abs().max() / ref.abs().max()).item()


def _data(n, c, k, h, w, r, seed, integers=False):
    """(dy, weight, float64 dx) of the stride-2 'same' convolution c -> k with an r x r filter on an h x w map"""
    gen = torch.Generator(device='cuda').manual_seed(seed)
    pad = r // 2
    ho, wo = (h + 2 * pad - r) // 2 + 1, (w + 2 * pad - r) // 2 + 1
    if integers:
        dy = torch.randint(-4, 5, (n, k, ho, wo), device='cuda', generator=gen).float()
        w0 = torch.randint(-4, 5, (k, c, r, r), device='cuda', generator=gen).float()
    else:
        dy = torch.randn(n, k, ho, wo, device='cuda', generator=gen) * (torch.rand(n, k, ho, wo, device='cuda', generator=gen) * 4 - 2).exp2()
        w0 = torch.randn(k, c, r, r, device='cuda', generator=gen) / (k * r * r) ** 0.5
    ref = torch.nn.grad.conv2d_input((n, c, h, w), w0.double(), dy.double(), 2, pad, 1)
    return dy, w0, ref


def _dgrad(pkg, xshape, dy, w0, accumulate=0, dx=None, ws=None, ws_bytes=None):
    """one p3d_conv2d_dgrad call at stride 2: (dx, (x3 data gradients, fp32-MFMA ones), the x3 launch records)"""
    ops, L = pkg.ops, pkg._lib.lib()
    r = w0.shape[2]
    d = ops._desc(xshape, w0.shape, 2, r // 2, 1, accumulate=accumulate)
    if ws_bytes is None:
        ws_bytes = L.p3d_conv2d_dgrad_workspace_bytes(ctypes.byref(d))
    if ws is None:
        ws = torch.full((max(ws_bytes, 16),), 0xFF, dtype=torch.uint8, device='cuda')           # poisoned: scratch read before it is written shows
    if dx is None:
        dx = torch.full(xshape, float('nan'), device='cuda')
    ops.conv_path_stats(reset=True)
    ops.fx_launch_log(reset=True)
    pkg._lib.check(L.p3d_conv2d_dgrad(ctypes.byref(d), ops._p(dy), ops._p(w0), None, None, ops._p(dx), ops._p(ws), ws_bytes, ops._stream()), 'p3d_conv2d_dgrad')
    torch.cuda.synchronize()
    stats = ops.conv_path_stats(reset=True)
    return dx, (stats['x3']['dgrad'][0], stats['fp32']['dgrad'][0]), ops.fx_launch_log(reset=True)[0]


def _live_classes(r):
    return 4 if r > 1 else 1


def _check_log(log, r):
    """one ragged fp32-fed launch per live class, unsplit, the interleave noted on the last"""
    assert len(log) == _live_classes(r), log
    for i, rec in enumerate(log):
        assert (rec['kernel'], rec['amode'], rec['pro'], rec['epi'], rec['tapi'], rec['rag'], rec['rows']) == (0, 0, 0, 0, 0, 1, 0), rec
        assert rec['grid_y'] == 1 and rec['grid_z'] == 1 and rec['kchunk'] == 0, rec
        assert rec['finish'] == (FINISH_INTERLEAVE_ROWS if i == len(log) - 1 else 0), rec


def _both(pkg, n, c, k, h, w, r, seed):
    """the switch off and on, on the same data: (float64 reference, dx off, dx on), with the routing of both legs checked"""
    dy, w0, ref = _data(n, c, k, h, w, r, seed)
    before = pkg.ops.x3_any_strided(False)
    try:
        off, off_counts, off_log = _dgrad(pkg, (n, c, h, w), dy, w0)
        pkg.ops.x3_any_strided(True)
        on, on_counts, on_log = _dgrad(pkg, (n, c, h, w), dy, w0)
    finally:
        pkg.ops.x3_any_strided(before)
    assert off_counts == (0, 1) and off_log == [], (off_counts, off_log)
    assert on_counts == (1, 0), on_counts
    _check_log(on_log, r)
    return ref, off, on


# ---- 1. against float64 -----------------------------------------------------------------------------------------------------------------------------
# n, c, k, h, w, r
SHAPES = [(2, 96, 32, 9, 11, 3),                                # classes 5 x 6 down to 4 x 5: the last class is under one 128-pixel tile
          (3, 96, 32, 17, 19, 3), (3, 96, 32, 17, 19, 1),       # 90-pixel classes: a thread's four pixels straddle rows and images
          (2, 96, 32, 16, 17, 3), (2, 96, 32, 17, 20, 3),       # one even side; W % 8 != 0
          (2, 224, 64, 9, 9, 1)]                                # two channel tiles, the second partial


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'n%d_c%d_k%d_%dx%d_%dx%d' % (s[0], s[1], s[2], s[3], s[4], s[5], s[5]))
def test_matches_float64(pkg, shape):
    n, c, k, h, w, r = shape
    ref, off, on = _both(pkg, n, c, k, h, w, r, seed=h * 100 + w + r)
    e32, e3 = _err(off, ref), _err(on, ref)
    print('%s: fp32-MFMA %.3e  x3 %.3e' % (shape, e32, e3))
    assert torch.isfinite(on).all()
    assert e3 <= TOL and e3 <= 4 * e32, (e32, e3)
    assert not torch.equal(on, off)                             # the other kernel really ran


# ---- 2. exact ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r', [3, 1])
def test_integer_data_gradient_is_exact(pkg, strided_on, r):
    """dy and w integers in [-4, 4]: every product and partial sum is an integer far below 2^24, so a pixel lost, shifted or counted twice at a row end, an image
    end, a class edge or in the interleave changes dx"""
    n, c, k, h, w = 3, 96, 32, 17, 19
    dy, w0, ref = _data(n, c, k, h, w, r, seed=29 + r, integers=True)
    assert ref.abs().max().item() < 2 ** 24
    dx, counts, log = _dgrad(pkg, (n, c, h, w), dy, w0)
    assert counts == (1, 0)
    _check_log(log, r)
    assert torch.equal(dx.double(), ref), (dx.double() - ref).abs().max().item()


# ---- 3. accumulate and dead classes ----------------------------------------------------------------------------------------------------------------------
def test_dead_classes_and_accumulate(pkg, strided_on):
    n, c, k, h, w = 2, 96, 32, 9, 11
    dy, w0, ref = _data(n, c, k, h, w, 1, seed=31)
    dead = torch.ones(h, w, dtype=torch.bool, device='cuda')
    dead[0::2, 0::2] = False
    # accumulate = 0 over NaNs: the three dead classes are exactly +0
    dx, counts, _ = _dgrad(pkg, (n, c, h, w), dy, w0)
    assert counts == (1, 0)
    assert torch.isfinite(dx).all() and _err(dx, ref) <= TOL
    assert (dx[:, :, dead].view(torch.int32) == 0).all()                    # +0: not a single sign bit
    # accumulate = 1: dead-class pixels bit-unchanged, the live class old + gradient (one rounding of the fp32 sum of two fp32 values)
    gen = torch.Generator(device='cuda').manual_seed(5)
    fill = torch.randn((n, c, h, w), device='cuda', generator=gen)
    acc, counts, _ = _dgrad(pkg, (n, c, h, w), dy, w0, accumulate=1, dx=fill.clone())
    assert counts == (1, 0)
    assert torch.equal(acc[:, :, dead].view(torch.int32), fill[:, :, dead].view(torch.int32))
    assert torch.equal(acc[:, :, 0::2, 0::2], fill[:, :, 0::2, 0::2] + dx[:, :, 0::2, 0::2])
    # a 3x3 under accumulate: every class live
    dy3, w3, ref3 = _data(n, c, k, h, w, 3, seed=37)
    plain, _, _ = _dgrad(pkg, (n, c, h, w), dy3, w3)
    acc3, counts, log = _dgrad(pkg, (n, c, h, w), dy3, w3, accumulate=1, dx=fill.clone())
    assert counts == (1, 0)
    _check_log(log, 3)
    assert torch.equal(acc3, fill + plain)
    assert _err(acc3, ref3 + fill.double()) <= TOL


# ---- 4. fenced -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(2, 96, 32, 9, 11, 3), (3, 96, 32, 17, 19, 1)], ids=['9x11_3x3', '17x19_1x1'])
def test_exact_size_fenced_buffers(pkg, strided_on, shape):
    """dy and w behind NaN bands, dx and a workspace of exactly the queried size between fences and poisoned: no byte outside is written, nothing poisoned reaches
    the result, and two runs are bit-equal"""
    ops, L = pkg.ops, pkg._lib.lib()
    n, c, k, h, w, r = shape
    dy0, w0, ref = _data(n, c, k, h, w, r, seed=41)
    d = ops._desc((n, c, h, w), w0.shape, 2, r // 2, 1)
    nb = L.p3d_conv2d_dgrad_workspace_bytes(ctypes.byref(d))
    runs = []
    for _ in range(2):
        fences = []

        def operand(src):
            t, f = fenced.fenced_like(src.shape, torch.float32, 4096, sentinel=0xFF)       # NaN bands: a fetch beyond the tensor would bring one in
            t.copy_(src)
            fences.append(f)
            return t

        dy, wt = operand(dy0), operand(w0)
        dx, f = fenced.fenced_like((n, c, h, w), torch.float32, 4096)
        fences.append(f)
        wsf = fenced.Fence(nb, 65536, 'cuda')
        fences.append(wsf)
        got, counts, log = _dgrad(pkg, (n, c, h, w), dy, wt, dx=dx, ws=wsf.view, ws_bytes=nb)
        assert counts == (1, 0)
        _check_log(log, r)
        for f in fences:
            f.check()
        assert torch.isfinite(got).all() and _err(got, ref) <= TOL
        assert torch.equal(dy, dy0) and torch.equal(wt, w0)
        runs.append(got.clone())
    assert torch.equal(runs[0], runs[1])


# ---- 5. routing ------------------------------------------------------------------------------------------------------------------------------------------
def test_routing(pkg):
    ops, L = pkg.ops, pkg._lib.lib()
    n, c, k, h, w, r = 3, 96, 32, 17, 19, 3
    ref, off, on = _both(pkg, n, c, k, h, w, r, seed=43)       # on: one x3 data gradient, one RAG record per live class, code 5 on the last; off: the counts the other way round
    dy, w0, _ = _data(n, c, k, h, w, r, seed=43)
    before = ops.x3_any_strided(False)
    try:
        # off is the parent's path: the fp32-MFMA kernel, bit for bit what the library computes with the x3 kernels disabled altogether
        x3_before = ops.set_x3(False)
        try:
            plain, counts, log = _dgrad(pkg, (n, c, h, w), dy, w0)
        finally:
            ops.set_x3(x3_before)
        assert counts == (0, 1) and log == [] and torch.equal(plain, off)
        # on, a workspace one byte short of the plan: fp32-MFMA, the bits of the switch-off run
        ops.x3_any_strided(True)
        d = ops._desc((n, c, h, w), w0.shape, 2, r // 2, 1)
        nb = L.p3d_conv2d_dgrad_workspace_bytes(ctypes.byref(d))
        short, counts, log = _dgrad(pkg, (n, c, h, w), dy, w0, ws_bytes=nb - 1)
        assert counts == (0, 1) and log == [] and torch.equal(short, off)
        # an aligned shape keeps its aligned launch (all four classes in one grid) and its bits
        dya, wa, refa = _data(2, 96, 32, 16, 16, 3, seed=47)
        res = {}
        for sw in (False, True):
            ops.x3_any_strided(sw)
            res[sw] = _dgrad(pkg, (2, 96, 16, 16), dya, wa)
        for sw in (False, True):
            dxa, counts, log = res[sw]
            assert counts == (1, 0) and len(log) == 1 and log[0]['rag'] == 0 and log[0]['grid_z'] == 4 and log[0]['finish'] == 0, (sw, counts, log)
        assert torch.equal(res[False][0], res[True][0]) and _err(res[True][0], refa) <= TOL
    finally:
        ops.x3_any_strided(before)


# ---- 6. the interleave alone -------------------------------------------------------------------------------------------------------------------------------
def _interleave(pkg, kernel, stage, dx, mask, shape, cls_stride, live, accumulate):
    n, c, h, w = shape
    ops = pkg.ops
    pkg._lib.check(pkg._lib.lib().p3d_dgrad_interleave(kernel, ops._p(stage), ops._p(dx), ops._p(mask), n, c, h, w, cls_stride, live, accumulate, ops._stream()),
                   'p3d_dgrad_interleave')
    return dx


@pytest.mark.parametrize('shape', [(2, 3, 5, 7), (1, 4, 9, 8), (3, 2, 2, 2), (2, 5, 65, 65), (4, 32, 129, 129)], ids=lambda s: '%dx%dx%dx%d' % s)
def test_interleave_kernels_are_bit_equal(pkg, shape):
    """dgrad_interleave_rows_kernel against dgrad_interleave_kernel on the same planes: every live mask, accumulate and factor combination; the planes of dead
    classes, and whatever lies between two planes, hold NaNs, which must not reach dx.  (4, 32, 129, 129) is more than one pass of either kernel's grid: 2048 x 256
    threads x 4 floats and 8192 x 256 threads; the others end in a partial chunk, start rows at every offset of a 16-B line, or are smaller than one chunk per row)"""
    n, c, h, w = shape
    total = n * c * h * w
    if shape == (4, 32, 129, 129):
        assert total > 2048 * 256 * 4 and total > 8192 * 256
    gen = torch.Generator(device='cuda').manual_seed(total)
    cls_stride = (n * c * ((h + 1) // 2) * ((w + 1) // 2) + 3) // 4 * 4
    planes = {cls: torch.randn(n * c, (h - cls // 2 + 1) // 2, (w - cls % 2 + 1) // 2, device='cuda', generator=gen) for cls in range(4)}
    mask0 = (torch.rand(n, 1, h, w, device='cuda', generator=gen) > 0.3).float() * torch.rand(n, 1, h, w, device='cuda', generator=gen)
    fill = torch.randn(n, c, h, w, device='cuda', generator=gen)
    for live in (0b1111, 0b0001):
        stage = torch.full((4 * cls_stride,), float('nan'), device='cuda')
        want = torch.zeros(n, c, h, w, device='cuda')
        for cls in range(4):
            if (live >> cls) & 1:
                stage[cls * cls_stride:cls * cls_stride + planes[cls].numel()] = planes[cls].reshape(-1)
                want[:, :, cls // 2::2, cls % 2::2] = planes[cls].view(n, c, planes[cls].shape[1], planes[cls].shape[2])
        for accumulate in (0, 1):
            for mask in (None, mask0):
                start = fill.clone() if accumulate else torch.full((n, c, h, w), float('nan'), device='cuda')
                old = _interleave(pkg, 0, stage, start.clone(), mask, shape, cls_stride, live, accumulate)
                new = _interleave(pkg, 1, stage, start.clone(), mask, shape, cls_stride, live, accumulate)
                torch.cuda.synchronize()
                what = (shape, live, accumulate, mask is not None)
                assert torch.isfinite(new).all(), what
                assert torch.equal(new.view(torch.int32), old.view(torch.int32)), what
                value = want if mask is None else want * mask
                assert torch.equal(new, fill + value if accumulate else value), what          # (and both are the plain statement of the pass)


def test_interleave_into_a_result_off_a_16_byte_line(pkg):
    """the hook alone can hand the new kernel a dx that is not 16-B aligned (the entry never does): dword accesses, the same bits, nothing written around it"""
    shape = n, c, h, w = (2, 3, 5, 7)
    total = n * c * h * w
    gen = torch.Generator(device='cuda').manual_seed(3)
    cls_stride = (n * c * 3 * 4 + 3) // 4 * 4
    stage = torch.randn(4 * cls_stride, device='cuda', generator=gen)
    for accumulate in (0, 1):
        for shift in (1, 2, 3):
            room = torch.randn(total + 8, device='cuda', generator=gen)
            held = room.clone()
            old = _interleave(pkg, 0, stage, room[shift:shift + total].clone().view(shape), None, shape, cls_stride, 0b1111, accumulate)
            _interleave(pkg, 1, stage, room[shift:shift + total].view(shape), None, shape, cls_stride, 0b1111, accumulate)
            torch.cuda.synchronize()
            assert torch.equal(room[shift:shift + total].view(torch.int32), old.reshape(-1).view(torch.int32)), (accumulate, shift)
            assert torch.equal(room[:shift], held[:shift]) and torch.equal(room[shift + total:], held[shift + total:]), (accumulate, shift)


# ---- 7. the whole step -------------------------------------------------------------------------------------------------------------------------------------
def test_whole_step_at_an_odd_side(pkg):
    """the reference's own step at side 257 (tests/golden/step_depth_r18_odd_b1.npz) with ops.x3_any and the new switch on: the assertions and tolerances of
    tests/test_train_anysize_gpu.py::test_whole_step_at_an_odd_side, with two data gradients fewer on the fp32-MFMA kernels -- layer3.0's 3x3 and its downsample
    1x1; layer2.0's have 64 input channels and stay"""
    import test_step_gpu as S
    import test_train_anysize_gpu as A
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
    seen, hooks = A._record_convs(pkg, model)
    before = pkg.ops.x3_any(True), pkg.ops.x3_any_strided(True)
    try:
        pkg.ops.conv_path_stats(reset=True)
        pkg.ops.fx_launch_log(reset=True)
        loss = float(trainer.train_step(*batch))
        pkg.ops.join_side_stream()
        torch.cuda.synchronize()
        on = A._counts(pkg.ops.conv_path_stats(reset=True))
        log = pkg.ops.fx_launch_log(reset=True)[0]
    finally:
        pkg.ops.x3_any(before[0])
        pkg.ops.x3_any_strided(before[1])
    hook.remove()
    for h in hooks:
        h.remove()
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
    # -- the routing --
    fp32_fwd = sum(1 for ci, co, st, rg in seen if ci < 16 or co == 64)
    moved = [(ci, co) for ci, co, st, rg in seen if rg and st == 2 and ci >= 96]
    assert sorted(moved) == [(128, 256), (128, 256)], moved                          # layer3.0's 3x3 and its downsample 1x1
    fp32_dgrad = sum(1 for ci, co, st, rg in seen if rg and (ci == 64 or st == 2)) - 2
    fp32_wgrad = sum(1 for ci, co, st, rg in seen if ci < 16 or ci == 64 or co == 64)
    dgrads = sum(1 for s in seen if s[3])
    x3, fp32 = on
    print('switches on: x3 %s  fp32-MFMA %s' % (x3, fp32))
    assert fp32 == (fp32_fwd, fp32_dgrad, fp32_wgrad), (on, seen)
    assert x3 == (len(seen) - fp32_fwd, dgrads - fp32_dgrad, len(seen) - fp32_wgrad) and min(x3) > 0, (on, seen)
    assert sum(1 for rec in log if rec['finish'] == FINISH_INTERLEAVE_ROWS) == 2, log


def test_frozen_fold_step_is_deterministic(pkg, strided_on):
    """one frozen-fold step (ops.frozen_fold(True), every BatchNorm frozen) at side 257 with the switch on, twice: the strided data gradients of the folded
    convolutions go through the same entry, and the results are bit-equal"""
    import test_frozen_fold_gpu as Z
    before = pkg.ops.frozen_fold(True)
    try:
        model, _ = Z._network(pkg, 'resnet18', False, 257, trainer=False)
        batch = Z._batch(pkg, 257, False)
        runs = []
        for _ in range(2):
            pkg.ops.conv_path_stats(reset=True)
            pkg.ops.fx_launch_log(reset=True)
            loss, _, grads, _ = Z._step(pkg, model, None, batch, False)
            log = pkg.ops.fx_launch_log(reset=True)[0]
            assert sum(1 for rec in log if rec['finish'] == FINISH_INTERLEAVE_ROWS) == 2, log          # layer3.0's two strided data gradients
            runs.append((loss, grads))
    finally:
        pkg.ops.frozen_fold(before)
    assert runs[0][0] == runs[1][0] and np.isfinite(runs[0][0])
    assert sorted(runs[0][1]) == sorted(runs[1][1]) and len(runs[0][1]) > 0
    for name, grad in runs[0][1].items():
        assert torch.isfinite(grad).all() and torch.equal(grad, runs[1][1][name]), name
