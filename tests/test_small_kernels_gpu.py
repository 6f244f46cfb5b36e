"""The loss, optimizer and streaming kernels past one pass of their grid: per-kernel parity with a float64 reference at the smallest sizes that make a
grid-stride loop iterate twice, leave a vector tail, start off a 16-byte boundary or give more than the first block work.  The launch lines whose caps these
sizes cross are tabled in tests/test_small_kernels_host.py, which also evaluates, on the CPU, every condition the cases below rely on (distances to the knots
of the criteria, condition numbers, the share of values left out) on the inputs the builders here return.  Outputs lie in exact-size, poisoned fences
(tests/fenced.py): a store past the last element fails the test, and so does an element that was never written.  Needs an MI355X: run with `-m gpu`."""
import functools
import json

import numpy as np
import pytest
import torch

from conftest import golden_path
from fenced import FencedAllocations, fenced_like
from oracle import np_data
from oracle import np_ops as ref

pytestmark = pytest.mark.gpu

CRITERIA = ('SmoothL1', 'L1', 'MSE')
KNOT_MARGIN = 1e-4            # no valid element lies this close to |diff| = 1 (SmoothL1) or 0 (L1): fp32 `spec` near 1000 carries about 6e-6 after / 10


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def fenced_copy(a, front=0, band=4096):
    """The values of `a` on the device, ending exactly where a poisoned Fence's interior ends and starting `front` elements into it (front = 1: a float
    tensor four bytes off a 256-byte boundary).  Returns (tensor, fence, the slack in front of it as bytes)."""
    a = np.ascontiguousarray(a)
    src = torch.from_numpy(a)
    flat, fence = fenced_like((a.size + front,), src.dtype, band)
    view = flat[front:].view(a.shape)
    view.copy_(src)
    return view, fence, flat[:front].view(torch.uint8)


def check_fences(*triples):
    torch.cuda.synchronize()
    for _, fence, slack in triples:
        fence.check()
        assert bool((slack == fence.poison).all()), 'the elements in front of an offset view were written'


# ---- pose loss (pose_loss_kernel: one block of 256 over B * J, 3 * B * J and, for the key joint, 3 * B) ------------------------------------------------
POSE_CASES = [(1, 17, 16), (6, 17, 0), (90, 17, 16), (90, 25, 7), (128, 3, 1)]              # (B, J, key joint)
POSE_PATTERNS = ('all', 'some', 'sample', 'none', 'key')
POSE_SEEDS = {(1, 17, 16): 0, (6, 17, 0): 0, (90, 17, 16): 3, (90, 25, 7): 0, (128, 3, 1): 0}    # chosen on the CPU: see pose_knot_distances


def pose_inputs(b, j, key, pattern):
    """relat mixes |diff| < 1 and > 1 after / loss_div (the data of test_pose_loss); validity: all / 30 % invalid / one whole sample invalid / nothing valid /
    the key joint invalid in every other sample.  The values do not depend on the pattern."""
    rng = np.random.default_rng(POSE_SEEDS[(b, j, key)])
    relat = (rng.standard_normal((b, j, 3)) * 8 + 1000).astype(np.float32)
    cam = (rng.standard_normal((b, j, 3)) * 8).astype(np.float32)
    some = rng.random((b, j)) >= 0.3
    val = np.ones((b, j), dtype=bool)
    if pattern == 'some':
        val = some.copy()
        val[:, key] = True
    elif pattern == 'sample':
        val[b // 2] = False
    elif pattern == 'none':
        val[:] = False
    elif pattern == 'key':
        val = some.copy()
        val[0::2, key] = False
        val[1::2, key] = True
    return relat, cam, val


def pose_knot_distances(relat, cam, key, loss_div):
    """float64 |diff| of every element outside the key joint -> (its least distance to 1, its least distance to 0, the largest |diff| of the key joint).  The key
    joint's own diff is relat[key] - relat[key] + cam[key] - cam[key]: an exact zero in float32 and float64 alike, where sign(0) = 0 on both sides."""
    r, c = relat.astype(np.float64), cam.astype(np.float64)
    diff = np.abs((r - r[:, key:key + 1] + c[:, key:key + 1] - c) / loss_div)
    rest = np.delete(diff, key, axis=1)
    return (np.abs(rest - 1).min() if rest.size else np.inf), (rest.min() if rest.size else np.inf), diff[:, key].max()


@pytest.mark.parametrize('criterion', CRITERIA)
@pytest.mark.parametrize('case', POSE_CASES, ids=lambda c: 'b%d_j%d_key%d' % c)
def test_pose_loss_sizes_and_validity(case, criterion, pkg):
    """Bounds of test_pose_loss: 1e-5 loss / 1e-6 spec / 1e-5 gradient."""
    b, j, key = case
    worst = [0.0, 0.0, 0.0]
    for pattern in POSE_PATTERNS:
        relat, cam, val = pose_inputs(b, j, key, pattern)
        count = 3 * int(val.sum())
        for loss_div in (1.0, 10.0):
            loss_ref, spec_ref, drelat_ref = ref.pose_loss_fwd_bwd(relat, cam, val, key, loss_div, criterion)
            for doubled in (False, True):                                            # count_override = twice the valid count: loss and gradient halve
                k = 0.5 if doubled and count else 1.0
                rt = dev(relat).requires_grad_(True)
                override = dev(np.array([2.0 * count], dtype=np.float32)) if doubled else None
                with FencedAllocations() as fa:
                    loss, spec = pkg.ops.pose_loss(rt, dev(cam), dev(val), key, loss_div, criterion, override)
                torch.cuda.synchronize()
                fa.check()
                assert len(fa.fences) == 3                                           # loss, spec, drelat
                loss.backward()
                what = (case, pattern, loss_div, doubled)
                errs = (abs(float(loss.detach()) - k * loss_ref) / max(abs(k * loss_ref), 1), relerr(host(spec), spec_ref), relerr(host(rt.grad), k * drelat_ref))
                worst = [max(w, e) for w, e in zip(worst, errs)]
                assert errs[0] < 1e-5 and errs[1] < 1e-6 and errs[2] < 1e-5, (what, errs)
                if count == 0:
                    assert float(loss.detach()) == 0.0 and not host(rt.grad).any(), what
    print('pose_loss', case, criterion, 'loss %.2e spec %.2e grad %.2e' % tuple(worst))


# ---- masked loss (masked_loss_kernel: one block over rows and rows * C) -------------------------------------------------------------------------------------
MASKED_SHAPES = [(4, 17, 2), (16, 17, 2), (90, 25, 3), (1, 1, 1)]
MASKED_SEEDS = {(4, 17, 2): 0, (16, 17, 2): 0, (90, 25, 3): 1, (1, 1, 1): 0}                    # chosen on the CPU: see masked_knot_distances


def masked_inputs(shape, pattern):
    rng = np.random.Generator(np.random.PCG64(MASKED_SEEDS[shape]))
    pred, target = rng.standard_normal(shape).astype(np.float32) * 2, rng.standard_normal(shape).astype(np.float32)
    valid = rng.random(shape[:2]) > 0.3
    valid[0, 0] = True
    if pattern == 'none':
        valid[:] = False
    return pred, target, valid


def masked_knot_distances(pred, target):
    diff = np.abs(pred.astype(np.float64) - target.astype(np.float64))
    return np.abs(diff - 1).min(), diff.min()


@pytest.mark.parametrize('criterion', CRITERIA)
@pytest.mark.parametrize('shape', MASKED_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_masked_loss_sizes(shape, criterion, pkg):
    """Bound of test_recon_cam_and_mat_head_kernels' masked criterion: 1e-6 on the loss and on the gradient."""
    worst = [0.0, 0.0]
    for pattern in ('some', 'none'):
        pred, target, valid = masked_inputs(shape, pattern)
        count = int(valid.sum()) * shape[-1]
        want_loss, want_grad = ref.masked_loss(pred, target, valid, criterion)
        for doubled in (False, True):
            k = 0.5 if doubled and count else 1.0
            p = dev(pred).requires_grad_(True)
            override = dev(np.array([2.0 * count], dtype=np.float32)) if doubled else None
            with FencedAllocations() as fa:
                loss = pkg.ops.masked_loss(p, dev(target), dev(valid), criterion, override)
            torch.cuda.synchronize()
            fa.check()
            assert len(fa.fences) == 2                                               # loss, dpred
            (loss * 3.0).backward()
            errs = (abs(float(loss.detach()) - k * want_loss) / max(abs(k * want_loss), 1e-30), relerr(host(p.grad), 3.0 * k * want_grad))
            worst = [max(w, e) for w, e in zip(worst, errs)]
            if count == 0:
                assert float(loss.detach()) == 0.0 and not host(p.grad).any(), (shape, pattern)
            else:
                assert errs[0] < 1e-6 and errs[1] < 1e-6, (shape, pattern, doubled, errs)
    print('masked_loss', shape, criterion, 'loss %.2e grad %.2e' % tuple(worst))


# ---- get_recon_cam (recon_cam_fwd / bwd_kernel: blocks of 64 threads, one sample each) ------------------------------------------------------------------------
RECON_BATCHES = (1, 64, 65, 130)
RECON_JOINTS = (2, 17, 25)


def recon_inputs(b, j, skew):
    """A root-relative pose a few metres in front of a camera, its projection jittered by three pixels; with `skew` K[0, 1] != 0, which alone brings the
    terms kinv[1] of recon_solve into play.  Two joints lie 0.4 - 0.6 m apart in x and in y, so the 3 x 3 normal matrix stays well conditioned."""
    rng = np.random.default_rng(1000 * b + 10 * j + int(skew))
    relat = rng.normal(0, 300, (b, j, 3))
    relat[:, 0] = 0
    if j == 2:
        relat[:, 1, :2] = rng.uniform(400, 600, (b, 2)) * rng.choice([-1.0, 1.0], (b, 2))
    t = np.stack([rng.uniform(-500, 500, b), rng.uniform(-500, 500, b), rng.uniform(3000, 5000, b)], 1)
    K = np.zeros((b, 3, 3))
    K[:, 0, 0], K[:, 1, 1], K[:, 2, 2] = rng.uniform(1000, 1300, b), rng.uniform(1000, 1300, b), 1
    K[:, 0, 2], K[:, 1, 2] = rng.uniform(600, 680, b), rng.uniform(330, 390, b)
    if skew:
        K[:, 0, 1] = rng.uniform(5, 40, b) * rng.choice([-1.0, 1.0], b)
    p = relat + t[:, None]
    uv = np.einsum('bik,bjk->bji', K, p / p[:, :, 2:])[:, :, :2] + rng.normal(0, 3, (b, j, 2))
    drecon = rng.standard_normal((b, j, 3))
    return tuple(a.astype(np.float32) for a in (uv, relat, K, drecon))


def recon_condition(spec_mat, relat, K):
    """the largest condition number of a sample's normal matrix A^T A"""
    A = ref.recon_cam(spec_mat, relat, K)[1][0]
    return max(np.linalg.cond(m) for m in A.transpose(0, 2, 1) @ A)


@pytest.mark.parametrize('j', RECON_JOINTS)
@pytest.mark.parametrize('b', RECON_BATCHES)
def test_recon_cam_batches_and_skew(b, j, pkg):
    """Bounds of test_recon_cam_and_mat_head_kernels: 1e-6 on recon and d relat, 1e-5 on d spec_mat."""
    for skew in (False, True):
        spec_mat, relat, K, drecon = recon_inputs(b, j, skew)
        want, cache = ref.recon_cam(spec_mat, relat, K)
        dspec, drelat = ref.recon_cam_bwd(drecon, cache)
        sm, rc = dev(spec_mat).requires_grad_(True), dev(relat).requires_grad_(True)
        with FencedAllocations() as fa:
            recon = pkg.utils.get_recon_cam(sm, rc, dev(K), torch.ones(b, j, dtype=torch.bool).cuda())
            recon.backward(dev(drecon))
        torch.cuda.synchronize()
        fa.check()
        assert len(fa.fences) == 3 and fa.holds(recon.detach())                      # recon, dspec_mat, drelat
        errs = (relerr(host(recon), want), relerr(host(sm.grad), dspec), relerr(host(rc.grad), drelat))
        print('recon_cam b %d j %d skew %d: recon %.2e dspec %.2e drelat %.2e' % ((b, j, skew) + errs))
        assert errs[0] < 1e-6 and errs[1] < 1e-5 and errs[2] < 1e-6, (skew, errs)


# ---- distillation (distill_reduce / grad_kernel: grid (B, 32) x 256, so one pass covers 8 192 values of a sample) ------------------------------------------
DISTILL_TOL = 1e-5                          # tests/test_distill.py
DISTILL_MODES = ('l2', 'sigmoid', 'bce')
DISTILL_SHAPES = [(3, 8, 5, 5), (1, 3, 1, 1), (2, 7, 5, 7), (2, 9, 17, 15), (5, 33, 17, 15), (1, 130, 9, 9), (2, 512, 8, 8)]


def distill_inputs(shape, same_first=False):
    b, c, h, w = shape
    rng = np.random.default_rng(b * 1000 + c * 10 + h)
    t, s = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    a = rng.random((b, 1, h, w)).astype(np.float32)
    if same_first:
        s[0] = t[0]
    return t, s, a


def distill_case(pkg, shape, mode, same_first=False):
    t, s0, a = distill_inputs(shape, same_first)
    want_loss, want_ds = ref.distill_fwd_bwd(t, s0, a, mode)
    scale = max(np.abs(want_ds).max(), 1e-12)
    raws = []
    for weight, unit_grad in ((1.0, False), (1.0, True), (0.25, False), (0.25, True)):
        s = dev(s0).requires_grad_(True)
        with FencedAllocations() as fa:
            weighted, raw = pkg.ops.distill_loss(dev(t), s, dev(a), mode, weight=weight, unit_grad=unit_grad)
        torch.cuda.synchronize()
        fa.check()
        assert len(fa.fences) in (2, 3) and fa.holds(raw) and sum(f[0] == shape for f in fa.fences) == 1       # loss, ds (+ the partial sums when the workspace grows)
        upstream = 1.0 if unit_grad else 3.0                                         # unit_grad: the caller promises an incoming gradient of 1
        (weighted * upstream).backward()
        raws.append(raw)
        err_loss, err_ds = abs(float(raw) - want_loss) / max(abs(want_loss), 1e-30), np.abs(host(s.grad) - upstream * weight * want_ds).max() / (upstream * weight * scale)
        assert err_loss < DISTILL_TOL and err_ds < DISTILL_TOL, (shape, mode, weight, unit_grad, err_loss, err_ds)
        assert float(weighted) == pytest.approx(weight * float(raw), rel=1e-6)
    with FencedAllocations() as fa:                                                  # no gradient wanted (ds == nullptr): the same loss bits
        _, raw = pkg.ops.distill_loss(dev(t), dev(s0), dev(a), mode, weight=1.0)
    torch.cuda.synchronize()
    fa.check()
    assert all(torch.equal(raw, r) for r in raws)
    print('distill', shape, mode, 'loss %.2e ds %.2e' % (err_loss, err_ds))
    return host(s.grad)


@pytest.mark.parametrize('mode', DISTILL_MODES)
@pytest.mark.parametrize('shape', DISTILL_SHAPES, ids=lambda s: '%dx%dx%dx%d' % s)
def test_distill_shapes(shape, mode, pkg):
    distill_case(pkg, shape, mode)


@pytest.mark.parametrize('mode', DISTILL_MODES)
def test_distill_sample_with_zero_norm(mode, pkg):
    """t[0] == s[0]: the first sample's norm is zero and its gradient with it (no 0 / 0)"""
    ds = distill_case(pkg, (2, 9, 17, 15), mode, same_first=True)
    assert not ds[0].any() and ds[1].any()


# ---- l2norm and Adam (<= 2 048 blocks x 256 threads: one pass covers 2 097 152 values in float4 steps, 524 288 in the scalar kernels) ------------------------
FLAT_SIZES = (1, 3, 4, 5, 1023, 1025, 2101251)
ADAM_OFFSETS = dict(aligned=(0, 0, 0, 0), all=(1, 1, 1, 1), p=(1, 0, 0, 0), g=(0, 1, 0, 0), m=(0, 0, 1, 0), v=(0, 0, 0, 1))      # floats in front of p, g, m, v
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
ADAM_TOL = 2e-6                              # test_clip_and_adam_two_steps
GRAD_NORMS = (40.0, 0.5, 0.5, 0.5)           # the clip at 5 is active on the first step alone, for grad_scale 1 and 0.5


@functools.lru_cache(maxsize=None)
def flat_inputs(n):
    """p ~ N(0, 1) and four gradients of the norms above"""
    rng = np.random.default_rng(n)
    p = rng.standard_normal(n, dtype=np.float32)
    grads = []
    for norm in GRAD_NORMS:
        g = rng.standard_normal(n)
        grads.append((g * (norm / np.sqrt((g * g).sum()))).astype(np.float32))
    return p, grads


@pytest.mark.parametrize('front', (0, 1), ids=('aligned', 'offset'))
@pytest.mark.parametrize('n', FLAT_SIZES)
def test_l2norm_tails_and_offsets(n, front, pkg):
    """The kernel squares in double (exact for float inputs) and sums in double: at most n * 2^-53 relative, 2.4e-10 at the largest n here.  1e-9."""
    g = flat_inputs(n)[0]
    gt = fenced_copy(g, front)
    accum = torch.full((1,), 3.25, dtype=torch.float64, device='cuda')             # an accumulator that already holds a value
    want = float((g.astype(np.float64) ** 2).sum())
    for calls in (1, 2):
        pkg.ops.l2norm_sq_accum(gt[0], accum)
        err = abs(float(accum) - (3.25 + calls * want)) / (3.25 + calls * want)
        assert err < 1e-9, (n, front, calls, err)
    check_fences(gt)
    assert np.array_equal(host(gt[0]), g)
    print('l2norm n %d front %d: %.2e' % (n, front, err))


def oracle_adam(p, g, m, v, step, max_norm, grad_scale, weight_decay):
    """clip_grad_norm_ on the scaled gradient + Adam -> (p, m, v, clip coefficient)"""
    coef = ref.clip_grad_norm([g.astype(np.float64) * grad_scale], max_norm)[1] if max_norm > 0 else 1.0
    return ref.adam_step(p, g, m, v, step, ADAM['lr'], weight_decay=weight_decay, grad_scale=coef * grad_scale) + (coef,)


@pytest.mark.parametrize('offsets', list(ADAM_OFFSETS), ids=list(ADAM_OFFSETS))
@pytest.mark.parametrize('n', FLAT_SIZES)
def test_adam_tails_and_offsets(n, offsets, pkg):
    """Four consecutive steps on the device's own moments, each against the oracle's step from the state the device held before it: the clip active on the
    first, inactive later, max_norm 0 with a norm given on the last; grad_scale 1 with no weight decay and 0.5 with 4e-5."""
    ops = pkg.ops
    p0, grads = flat_inputs(n)
    worst = 0.0
    for grad_scale, weight_decay in ((1.0, 0.0), (0.5, 4e-5)):
        fp, fg, fm, fv = (fenced_copy(a, front) for a, front in zip((p0, grads[0], np.zeros_like(p0), np.zeros_like(p0)), ADAM_OFFSETS[offsets]))
        norm_sq = torch.zeros(1, dtype=torch.float64, device='cuda')
        for step in (1, 2, 3, 4):
            g = grads[step - 1]
            fg[0].copy_(torch.from_numpy(g))
            before = [host(t[0]) for t in (fp, fm, fv)]
            max_norm = 5.0 if step < 4 else 0.0
            norm_sq.zero_()
            ops.l2norm_sq_accum(fg[0], norm_sq)
            ops.adam_step(fp[0], fg[0], fm[0], fv[0], ADAM['lr'], ADAM['beta1'], ADAM['beta2'], ADAM['eps'], weight_decay, step, max_norm, norm_sq, grad_scale)
            want = oracle_adam(before[0], g, before[1], before[2], step, max_norm, grad_scale, weight_decay)
            assert (want[3] < 0.5) if step == 1 else (want[3] == 1.0)
            for name, t, w in zip('pmv', (fp, fm, fv), want):
                err = np.abs(host(t[0]) - w).max()
                worst = max(worst, err)
                assert err < ADAM_TOL, (n, offsets, grad_scale, step, name, err)
        check_fences(fp, fg, fm, fv)
    print('adam n %d %s: %.2e' % (n, offsets, worst))


def test_flat_adam_pads_a_ragged_tensor_past_one_pass(pkg):
    """pkg.optim.FlatAdam's own flattening: tensors of 2 101 248 and 3 values, the second padded to 4, so the float4 kernels see 2 101 252 values in more than one
    pass and the last of them is padding that must stay zero.  Two steps, the clip active on the first; the norm at l2norm's bound, the parameters at Adam's."""
    n = max(FLAT_SIZES)
    p0, grads = flat_inputs(n)
    cuts = [(0, n - 3), (n - 3, n)]
    params = [torch.nn.Parameter(dev(p0[a:b].copy())) for a, b in cuts]
    opt = pkg.optim.FlatAdam([('p%d' % i, p) for i, p in enumerate(params)], lr=ADAM['lr'], weight_decay=4e-5)
    assert opt.total == n + 1 and opt.offsets == [0, n - 3]
    for step in (1, 2):
        g = grads[step - 1]
        before = [host(t[:n]) for t in (opt.flat_p, opt.exp_avg, opt.exp_avg_sq)]
        opt.zero_grad()
        for q, (a, b) in zip(params, cuts):
            q.grad.copy_(dev(g[a:b]))
        opt.clip_and_step(5.0)
        total = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
        assert abs(opt.total_norm() - total) < 1e-9 * total
        want = oracle_adam(before[0], g, before[1], before[2], step, 5.0, 1.0, 4e-5)
        assert (want[3] < 0.5) if step == 1 else (want[3] == 1.0)
        for name, t, w in zip('pmv', (opt.flat_p, opt.exp_avg, opt.exp_avg_sq), want):
            assert np.abs(host(t[:n]) - w).max() < ADAM_TOL, (step, name)
            assert float(t[n]) == 0.0, (step, name)                                  # the padding element: zero gradient, zero weight, stays zero
    assert all(np.array_equal(host(q), host(opt.flat_p[a:b])) for q, (a, b) in zip(params, cuts))


@pytest.mark.parametrize('front', (0, 1), ids=('aligned', 'offset'))
@pytest.mark.parametrize('n', FLAT_SIZES)
def test_adam_step_dev_counts_and_skips(n, front, pkg):
    """adam_prepare_kernel + adam_dev_kernel: state[0] counts the steps taken and feeds the bias correction, a non-finite norm_sq with skip_nonfinite leaves
    p, m, v and state[0] alone and counts in state[1]; without skip_nonfinite the step is taken (an infinite norm clips the gradient to nothing)."""
    ops = pkg.ops
    p0, grads = flat_inputs(n)
    fp, fg, fm, fv = (fenced_copy(a, front) for a in (p0, grads[0], np.zeros_like(p0), np.zeros_like(p0)))
    state = torch.zeros(2, dtype=torch.int32, device='cuda')
    scratch = torch.zeros(4, dtype=torch.float32, device='cuda')
    grad_scale, weight_decay, taken, skipped, worst = 0.5, 4e-5, 0, 0, 0.0
    #        norm_sq given     skip_nonfinite
    plan = [(None, 1), (float('inf'), 1), (float('nan'), 1), (float('inf'), 0), (None, 1)]
    for i, (given, skip) in enumerate(plan):
        g = grads[min(i, 3)]
        fg[0].copy_(torch.from_numpy(g))
        before = [host(t[0]) for t in (fp, fm, fv)]
        norm_sq = torch.zeros(1, dtype=torch.float64, device='cuda')
        if given is None:
            ops.l2norm_sq_accum(fg[0], norm_sq)
        else:
            norm_sq.fill_(given)
        ops.adam_step_dev(fp[0], fg[0], fm[0], fv[0], ADAM['lr'], ADAM['beta1'], ADAM['beta2'], ADAM['eps'], weight_decay, state, 5.0, norm_sq, grad_scale, skip,
                          scratch)
        after = [host(t[0]) for t in (fp, fm, fv)]
        if given is not None and skip:
            skipped += 1
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(after, before)), (n, i)
        else:
            taken += 1
            if given is None:
                want = oracle_adam(before[0], g, before[1], before[2], taken, 5.0, grad_scale, weight_decay)
            else:                                                                    # total = inf: the clip coefficient is 5 / inf = 0, the decay term remains
                want = ref.adam_step(before[0], g, before[1], before[2], taken, ADAM['lr'], weight_decay=weight_decay, grad_scale=0.0)
            for name, a, w in zip('pmv', after, want):
                err = np.abs(a - w).max()
                worst = max(worst, err)
                assert err < ADAM_TOL, (n, front, i, name, err)
        assert host(state).tolist() == [taken, skipped], (n, i)
    assert (taken, skipped) == (3, 2)
    check_fences(fp, fg, fm, fv)
    print('adam_step_dev n %d front %d: %.2e' % (n, front, worst))


# ---- image-side kernels ---------------------------------------------------------------------------------------------------------------------------------------
COLOUR_SHAPE = (2, 3, 129, 131)             # 16 899 px per image: augment_colour_kernel, 64 x 256 per image
ERASE_SHAPE = (4, 3, 80, 72)
ERASE_RECTS = [(5, 4, 65, 74),              # 60 wide, 70 high: 4 200 px > 16 x 256
               (-10, -5, 20, 30),           # clipped by the left and the top border
               (5, 5, 5, 9),                # empty
               (100, 100, 120, 130)]        # wholly outside
PASTE_OCC, PASTE_SIDE = (130, 127), 140     # 16 510 px > 64 x 256
NORMALIZE_SHAPE = (2, 3, 91, 91)            # 8 281 px per plane > 32 x 256
CROP_SIDE = 257                             # 66 049 px > 256 x 256, the default crop side
ENHANCE_SHAPE = (17, 1, 251, 246)           # 1 049 682 values > 4 096 x 256
ENHANCE_EDGE = 1e-5                         # test_enhance_depth_kernel leaves out values this close to the threshold


def colour_inputs():
    rng = np.random.default_rng(21)
    b = COLOUR_SHAPE[0]
    img = np.floor(rng.random(COLOUR_SHAPE) * 256).astype(np.float32)
    img[0, :, :4, :4] = 128.0                                                        # a grey patch: zero saturation, hue undefined
    img[1, :, 5, 5] = [255, 0, 0]
    params = np.stack([rng.uniform(-0.125, 0.125, b), rng.uniform(0.8, 1.25, b), rng.uniform(-18, 18, b), rng.uniform(0.8, 1.25, b)], 1).astype(np.float32)
    return img, params


def test_augment_colour_past_one_pass(pkg):
    """Criterion of test_augment_colour_and_erase; with no hue / saturation jitter drawn, bit-exact against the brightness / contrast restatement."""
    img, params = colour_inputs()
    want = np.stack([ref.augment_colour(img[i].transpose(1, 2, 0), *params[i]).transpose(2, 0, 1) for i in range(len(img))])
    t = fenced_copy(img)
    got = host(pkg.ops.augment_colour_(t[0], dev(params)))
    check_fences(t)
    diff = np.abs(got - want)
    print('augment_colour: %d values off by more than 1, %.4f %% off by 1' % ((diff > 1).sum(), 100 * (diff > 0).mean()))
    assert (diff > 1).sum() == 0 and (diff > 0).mean() < 0.01                       # at most a rounding flip of the final truncation
    params[:, 2:] = [0.0, 1.0]
    want = np.stack([ref.brightness_contrast(img[i].transpose(1, 2, 0).astype(np.uint8), params[i, 0], params[i, 1]).transpose(2, 0, 1) for i in range(len(img))])
    t = fenced_copy(img)
    got = host(pkg.ops.augment_colour_(t[0], dev(params)))
    check_fences(t)
    assert np.array_equal(got, want.astype(np.float32))


def test_augment_erase_large_and_clipped_rectangles(pkg):
    b, c, h, w = ERASE_SHAPE
    rng = np.random.default_rng(22)
    img = np.floor(rng.random(ERASE_SHAPE) * 256).astype(np.float32)
    colour = (np.floor(rng.random((b, c)) * 255) + 256).astype(np.float32)          # 256 .. 510: no pixel of the image already holds it
    rects = np.array(ERASE_RECTS, dtype=np.int32)
    want = img.copy()
    for i, (x0, y0, x1, y1) in enumerate(rects):
        want[i, :, max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = colour[i][:, None, None]
    assert [int((want[i] != img[i]).sum()) for i in range(b)] == [3 * 4200, 3 * 20 * 30, 0, 0]
    t = fenced_copy(img)
    got = host(pkg.ops.augment_erase_(t[0], dev(rects), dev(colour)))
    check_fences(t)
    assert np.array_equal(got, want)


def paste_inputs(chan):
    rng = np.random.default_rng(23 + chan)
    images = rng.integers(0, 256, (3, PASTE_SIDE, PASTE_SIDE, chan), dtype=np.uint8)
    occ = rng.integers(0, 256, PASTE_OCC + (chan,), dtype=np.uint8)
    alpha = rng.random(PASTE_OCC, dtype=np.float32)
    alpha[:20] = 1.0
    alpha[20:40] = 0.0
    centers = np.array([[70.0, 70.0], [120.3, 70.2], [0.0, 0.0]])                   # the whole occluder inside; cut by the lower border; the third image gets none
    return images, occ, alpha, centers


@pytest.mark.parametrize('truncate', (True, False), ids=('truncate', 'keep'))
@pytest.mark.parametrize('with_alpha', (True, False), ids=('alpha', 'opaque'))
@pytest.mark.parametrize('chan', (1, 3))
def test_augment_occlude_past_one_pass(chan, with_alpha, truncate, pkg):
    """Bit-exact against np_ops.paste_over: on a uint8 image (its assignment truncates) and, truncate off, on a float image"""
    images, occ, alpha, centers = paste_inputs(chan)
    a = alpha if with_alpha else None
    want = []
    for i in range(2):
        canvas = images[i].copy() if truncate else images[i].astype(np.float32)
        want.append(ref.paste_over(occ, canvas, a, centers[i]).astype(np.float32))
    want.append(images[2].astype(np.float32))
    t = fenced_copy(images.astype(np.float32).transpose(0, 3, 1, 2))
    got = host(pkg.augment.paste_over_(t[0], [occ, occ, None], [a, a, None], centers, truncate=truncate))
    check_fences(t)
    assert np.array_equal(got.transpose(0, 2, 3, 1), np.stack(want))


def test_normalize_rgb_past_one_pass(pkg):
    rng = np.random.default_rng(3)
    img = np.floor(rng.random(NORMALIZE_SHAPE) * 256).astype(np.float32)
    mean, std = np.array(pkg.ops.IMAGENET_MEAN, np.float64), np.array(pkg.ops.IMAGENET_STD, np.float64)
    want = (img.astype(np.float64) / 255 - mean[None, :, None, None]) / std[None, :, None, None]
    t = fenced_copy(img)
    got = host(pkg.ops.normalize_rgb_(t[0]))
    check_fences(t)
    err = np.abs(got - want).max()
    print('normalize_rgb: %.2e' % err)
    assert err < 2e-6


@pytest.mark.parametrize('dtype,chan', [(np.uint8, 3), (np.float32, 1)])
def test_warp_crops_at_the_default_side(dtype, chan, pkg):
    """test_warp_crops with 257 x 257 crops: the two-part criterion of that test"""
    rng = np.random.default_rng(8)
    b, hs, ws, side = 3, 60, 80, CROP_SIDE
    frames = (rng.random((b, hs, ws, chan)) * 255).astype(dtype)
    homs = []
    for i in range(b):
        f_old, f_new = 70.0 + 10 * i, (90.0 + 20 * i) * side / 48                   # a zoomed, rotated, re-centred virtual camera (no parallax)
        k_old = np.array([[f_old, 0, ws / 2], [0, f_old, hs / 2], [0, 0, 1]])
        k_new = np.array([[f_new, 0, side / 2], [0, f_new, side / 2], [0, 0, 1]])
        ang = 0.15 * (i - 1)
        r_y = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
        r_x = np.array([[1, 0, 0], [0, np.cos(0.1 * i), -np.sin(0.1 * i)], [0, np.sin(0.1 * i), np.cos(0.1 * i)]])
        homs.append(ref.crop_homography(k_old, np.eye(3), k_new, r_y @ r_x))
    homs = np.stack(homs)
    with FencedAllocations() as fa:
        out = pkg.ops.warp_crops(torch.from_numpy(frames).cuda(), dev(homs), (side, side))
    torch.cuda.synchronize()
    fa.check()
    assert fa.holds(out)
    got = host(out)
    assert np.isfinite(got).all()                                                    # (a NaN left over from the poison compares false with everything)
    want = np.stack([ref.warp_crop(frames[i], homs[i], (side, side)) for i in range(b)])
    assert got.shape == (b, chan, side, side)
    diff = np.abs(got - want)
    print('warp_crops %s: max %.3g, %.4f %% differ' % (np.dtype(dtype).name, diff.max(), 100 * (diff > 0).mean()))
    if dtype == np.uint8:
        assert (diff > 1).sum() == 0 and (diff > 0).mean() < 0.01                   # a rounding flip where the interpolant sits on .5
    else:
        assert diff.max() < 1e-3 * 255
    assert (want == 0).mean() > 0.02 and (want > 0).mean() > 0.5                    # the case crosses the frame border and the interior
    assert (want[:, :, -1] > 0).any()                                               # and the last row, which only a second pass reaches, holds picture


def golden_cameras():
    g = np.load(golden_path('camera.npz'))
    for m in json.loads(str(g['meta'])):
        v = g[m['name'] + '.in']
        yield g, m, (v[:3], v[3:12].reshape(3, 3), v[12:21].reshape(3, 3), v[21:26] if m['distorted'] else None, v[26:29])


def test_reproject_crops_at_the_default_side(pkg):
    """test_reproject_crops_kernel with 257 x 257 crops from the golden cameras, with and without distortion, rounded and not: the criterion of that test"""
    rng = np.random.Generator(np.random.PCG64(11))
    cams = list(golden_cameras())
    assert {m['distorted'] for _, m, _ in cams} == {True, False}
    side = (CROP_SIDE, CROP_SIDE)
    frames_u8 = rng.integers(0, 256, size=(len(cams), 270, 480, 3), dtype=np.uint8)
    frames_f = rng.random((len(cams), 270, 480, 1), dtype=np.float32)
    params, pairs = [], []
    for g, m, (t, R, K, dist, up) in cams:
        K = K.copy()
        K[:2] *= 0.25                                                                 # the golden cameras are 1920x1080; the test frames 480x270
        cam = pkg.cameralib.Camera(t, R, K, dist, world_up=up)
        px = cam.world_to_image(g[m['name'] + '.world'])
        lo, hi = px.min(0), px.max(0)
        new = pkg.crops.plan_crop(cam, np.concatenate([lo, hi - lo]), CROP_SIDE, 1.05, m['flipped'])
        params.append(pkg.cameralib.reproject_params(cam, new))
        pairs.append((cam, new))
    params = torch.from_numpy(np.stack(params)).cuda()
    for frames, rounded in ((frames_u8, True), (frames_u8, False), (frames_f, False)):
        with FencedAllocations() as fa:
            out = pkg.ops.reproject_crops(torch.from_numpy(frames).cuda(), params, side, round_u8=rounded)
        torch.cuda.synchronize()
        fa.check()
        assert fa.holds(out)
        got = host(out)
        assert np.isfinite(got).all()
        for i, (cam, new) in enumerate(pairs):
            want = np_data.reproject(frames[i], cam.intrinsic_matrix, cam.R, cam.distortion_coeffs, new.intrinsic_matrix, new.R, side, rounded)
            diff = np.abs(got[i] - want) / (255.0 if frames.dtype == np.uint8 else 1.0)
            print('reproject_crops %s rounded %d camera %d: max %.3g, share over 2e-3 %.2e' % (frames.dtype.name, rounded, i, diff.max(), np.mean(diff > 2e-3)))
            # random-noise frames: a 1e-4 px difference in the sample position moves a value by up to 1e-4 of full scale; rounding can flip at .5
            assert np.mean(diff > 2e-3) < (2e-3 if rounded else 1e-6), (i, rounded, diff.max())
            assert diff.max() <= (1.0 / 255 + 1e-6 if rounded else 2e-3)
            assert (want[:, -1] != 0).any()


def enhance_inputs():
    rng = np.random.Generator(np.random.PCG64(12))
    x = (rng.random(ENHANCE_SHAPE, dtype=np.float32) * 0.2).astype(np.float32)
    x[rng.random(x.shape) < 0.1] = 0
    factor = (1 + rng.random(x.shape, dtype=np.float32)).astype(np.float32)
    return x, factor


def enhance_edge(x, factor, threshold):
    """values sitting on the threshold, which test_enhance_depth_kernel leaves out"""
    return np.abs((x if factor is None else x / factor) / np.float32(10 / 255) - threshold) < ENHANCE_EDGE


def test_enhance_depth_past_one_pass(pkg):
    x, factor = enhance_inputs()
    for thr in (0.1, 0.5):
        for nexp in (False, True):
            for f in (None, factor):
                t = fenced_copy(x)
                got = host(pkg.ops.enhance_depth_(t[0], thr, nexp, None if f is None else dev(f)))
                check_fences(t)
                want = np_data.enhance(x if f is None else x / f, thr, nexp)
                edge = enhance_edge(x, f, thr)
                assert edge.mean() < 1e-3
                assert np.allclose(got[~edge], want[~edge], rtol=2e-6, atol=1e-7), (thr, nexp, f is not None)


# ---- pool, ReLU, masks ----------------------------------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(8, 65, 129, 129),            # W % 4 != 0: the generic kernels, 2 197 000 outputs > 8 192 x 256 and 8.65 M inputs
               (2, 1028, 128, 128)]          # the fwd4 / bwd4 kernels: 4 210 688 output quads > 16 384 x 256
RELU_SHAPE = (3, 349, 1003)                  # 1 050 141 values > 4 096 x 256
PCONV_SHAPE = (3, 1, 420, 420)               # 529 200 pixels > 2 048 x 256


@pytest.mark.parametrize('shape', POOL_SHAPES, ids=lambda s: '%dx%dx%dx%d' % s)
def test_maxpool_past_one_pass(shape, pkg):
    """Post-ReLU inputs, so ties are present: bit-exact forward, 1e-6 backward (test_maxpool_fwd_bwd_with_ties)"""
    rng = np.random.default_rng(sum(shape))
    x = np.maximum(rng.standard_normal(shape, dtype=np.float32), 0)
    y_ref, idx = ref.maxpool3x3s2_fwd(x)
    dy = rng.standard_normal(y_ref.shape, dtype=np.float32)
    dx_ref = ref.maxpool3x3s2_bwd(dy, idx, x.shape)
    xt = dev(x).requires_grad_(True)
    with FencedAllocations() as fa:
        y = pkg.ops.maxpool3x3s2(xt)
        y.backward(dev(dy))
    torch.cuda.synchronize()
    fa.check()
    assert len(fa.fences) == 3 and fa.holds(y.detach())                              # y, the argmax bytes, dx
    assert np.array_equal(host(y), y_ref)
    assert np.abs(host(xt.grad) - dx_ref).max() < 1e-6


def test_relu_past_one_pass(pkg):
    rng = np.random.default_rng(0)
    x = rng.standard_normal(RELU_SHAPE, dtype=np.float32)
    dy = rng.standard_normal(RELU_SHAPE, dtype=np.float32)
    xt = dev(x).requires_grad_(True)
    with FencedAllocations() as fa:
        y = pkg.ops.relu(xt)
        y.backward(dev(dy))
    torch.cuda.synchronize()
    fa.check()
    assert len(fa.fences) == 2 and fa.holds(y.detach())                              # y, dx
    assert np.array_equal(host(y), ref.relu_fwd(x))
    assert np.array_equal(host(xt.grad), ref.relu_bwd(dy, ref.relu_fwd(x)))


def test_partial_conv_masks_past_one_pass(pkg):
    """PartialConv 1 -> 1 channels, 3 x 3: nonzero_mask and mask_count on 529 200 pixels.  mask_out bit-exact, the output at the 1e-5 of the golden test."""
    rng = np.random.default_rng(4)
    x = rng.standard_normal(PCONV_SHAPE, dtype=np.float32)
    x[rng.random(PCONV_SHAPE) < 0.3] = 0
    x[0, 0, 100:120, 200:230] = 0                                                    # windows without a single valid pixel
    x[2, 0, -9:, -7:] = 0                                                            # the last of them in the last rows of the last image
    conv = pkg.partial_conv.PartialConv(1, 1, kernel_size=3, stride=1, padding=1, bias=False).cuda()
    wt = host(conv.weight)
    with FencedAllocations() as fa, torch.no_grad():
        mask = pkg.ops.nonzero_mask(dev(x))
        y, mask_out = conv(dev(x), mask)
    torch.cuda.synchronize()
    fa.check()
    assert fa.holds(mask) and fa.holds(mask_out)
    want_mask = (x != 0).astype(np.float32)
    assert np.array_equal(host(mask), want_mask)
    want_y, want_mo, _ = ref.partial_conv_fwd(x, want_mask, wt, None, 1, 1, 1)
    assert np.array_equal(host(mask_out), want_mo) and (want_mo[2, 0, -5:] == 0).any() and (want_mo[2, 0, -1] == 1).any()
    err = np.abs(host(y) - want_y).max() / max(np.abs(want_y).max(), 1.0)
    print('partial_conv: %.2e' % err)
    assert err < 1e-5
