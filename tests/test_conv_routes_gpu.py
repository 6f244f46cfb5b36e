"""The kernel family a per-layer convolution call lands on (conv_route, csrc/p3d_conv.hip): p3d_conv2d_fwd / _dgrad / _wgrad called through the C ABI on fenced,
poisoned buffers at the smallest shapes that reach each family -- the aligned x3 kernels, the ragged x3 instances (p3d_x3_any_enable), the masked x3 instances
and the fp32-MFMA kernels.  The library's own launch counters (ops.conv_path_stats) must move exactly one count, in the expected slot; the same call must fall to
the fp32-MFMA slot when an operand sits 4 bytes off a 16-B line, when the workspace is 16 B short of the query (forward, data gradient), when a bias comes with
the factors of a partial convolution, and under set_x3(False).  A weight gradient with a short workspace is refused with P3D_EWORKSPACE and launches nothing.
Every call is a valid one that one family or the other serves; results against float64, within the bounds tests/test_kernels_gpu.py holds the two families to."""
import collections
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import fenced
from test_kernels_gpu import CONV_TOL, X3_TOL

pytestmark = pytest.mark.gpu

EWORKSPACE = -2
PASSES = ('fwd', 'dgrad', 'wgrad')
Case = collections.namedtuple('Case', 'name n c k h w r stride pad masked any_width accumulate x3')       # x3: the passes the x3 kernels take, in the order of PASSES
CASES = [
    Case('aligned_1x1', 1, 128, 128, 8, 8, 1, 1, 0, False, False, 0, (1, 1, 1)),
    Case('aligned_3x3', 1, 128, 128, 8, 8, 3, 1, 1, False, False, 0, (1, 1, 1)),
    Case('ragged_1x1', 1, 128, 128, 7, 7, 1, 1, 0, False, True, 0, (1, 1, 1)),
    Case('ragged_3x3', 1, 128, 128, 7, 7, 3, 1, 1, False, True, 0, (1, 1, 1)),
    Case('masked_64', 1, 64, 64, 8, 8, 3, 1, 1, True, False, 0, (1, 1, 0)),                # the masked weight gradient starts at 96 channels
    Case('masked_128', 1, 128, 128, 8, 8, 3, 1, 1, True, False, 0, (1, 1, 1)),
    Case('strided_1x1', 1, 128, 128, 8, 8, 1, 2, 0, False, False, 0, (1, 1, 1)),           # the data gradient leaves three of four input pixels to the zero fill
    Case('strided_1x1_acc', 1, 128, 128, 8, 8, 1, 2, 0, False, False, 1, (1, 1, 1)),       #   or, accumulating, as they were
]
IDS = [c.name for c in CASES]


@functools.lru_cache(maxsize=None)
def data(case):
    """operands, factors, what the outputs hold before an accumulating call, and the float64 results of the three passes (with and without a bias)"""
    gen = torch.Generator(device='cuda').manual_seed(7 + CASES.index(case))
    n, c, k, h, w, r = case.n, case.c, case.k, case.h, case.w, case.r
    x = torch.randn(n, c, h, w, device='cuda', generator=gen)
    wt = torch.randn(k, c, r, r, device='cuda', generator=gen) / (c * r * r) ** 0.5
    bias = torch.randn(k, device='cuda', generator=gen)
    mask = mult = None
    xe = x.double()
    if case.masked:
        mask = (torch.rand(n, 1, h, w, device='cuda', generator=gen) >= 0.3).float()
        mask[0, 0, :3, :4] = 0                                                          # an empty window: mult == 0 there
        ones = torch.ones(1, 1, r, r, device='cuda', dtype=torch.float64)
        cnt = F.conv2d(mask.double(), ones, None, case.stride, case.pad)
        mult = torch.where(cnt > 0, r * r / cnt.clamp(min=1), torch.zeros_like(cnt)).float()
        xe = xe * mask.double()
    y = F.conv2d(xe, wt.double(), None, case.stride, case.pad)
    dy = torch.randn(y.shape, device='cuda', generator=gen)
    dye = dy.double()
    yb = y + bias.double().view(1, -1, 1, 1)
    if case.masked:
        y, dye = y * mult.double(), dye * mult.double()
        yb = torch.where(mult.double() > 0, y + bias.double().view(1, -1, 1, 1), torch.zeros_like(y))
    dx = torch.nn.grad.conv2d_input(x.shape, wt.double(), dye, case.stride, case.pad)
    if case.masked:
        dx = dx * mask.double()
    dw = torch.nn.grad.conv2d_weight(xe, wt.shape, dye, case.stride, case.pad)
    want = dict(fwd=y, fwd_bias=yb, dgrad=dx, wgrad=dw)
    prior = {p: torch.randn(want[p].shape, device='cuda', generator=gen) for p in PASSES}
    return dict(x=x, w=wt, bias=bias, mask=mask, mult=mult, dy=dy, want=want, prior=prior)


def off_line(t):
    """the same values 4 bytes off a 256-B line, inside a larger buffer"""
    flat = torch.empty(t.numel() + 64, device=t.device, dtype=t.dtype)
    out = flat[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4
    return out


@pytest.fixture
def switches(pkg):
    """(set_x3, x3_any) for the test body; both back where they were afterwards"""
    x3, any_width = pkg.ops.set_x3(True), pkg.ops.x3_any(False)
    yield pkg.ops.set_x3, pkg.ops.x3_any
    pkg.ops.set_x3(x3)
    pkg.ops.x3_any(any_width)


def run(pkg, case, which, misaligned=False, short=0, with_bias=False):
    """One call of the entry of pass `which`.  Returns (return code, result or None, its Fence, the workspace's Fence, the launch counters)."""
    ops, L = pkg.ops, pkg._lib.lib()
    t = data(case)
    d = ops._desc(t['x'].shape, t['w'].shape, case.stride, case.pad, 1, accumulate=case.accumulate)
    query = dict(fwd=L.p3d_conv2d_fwd_workspace_bytes, dgrad=L.p3d_conv2d_dgrad_workspace_bytes, wgrad=L.p3d_conv2d_wgrad_workspace_bytes)[which]
    nbytes = query(ctypes.byref(d)) - short
    assert nbytes >= 0
    ws = fenced.Fence(nbytes, 4096, 'cuda')
    out, fence = fenced.fenced_like(t['want'][which].shape, torch.float32, 4096)
    if case.accumulate:
        out.copy_(t['prior'][which])
    a = t['dy'] if which != 'fwd' else t['x']
    if misaligned:
        a = off_line(a)
    wsp = ops._p(ws.view) if nbytes else None
    ops.conv_path_stats(reset=True)
    if which == 'fwd':
        rc = L.p3d_conv2d_fwd(ctypes.byref(d), ops._p(a), ops._p(t['w']), ops._p(t['bias']) if with_bias else None, ops._p(t['mask']), ops._p(t['mult']), ops._p(out), wsp, nbytes,
                              ops._stream())
    elif which == 'dgrad':
        rc = L.p3d_conv2d_dgrad(ctypes.byref(d), ops._p(a), ops._p(t['w']), ops._p(t['mult']), ops._p(t['mask']), ops._p(out), wsp, nbytes, ops._stream())
    else:
        rc = L.p3d_conv2d_wgrad(ctypes.byref(d), ops._p(a), ops._p(t['x']), ops._p(t['mult']), ops._p(t['mask']), ops._p(out), wsp, nbytes, ops._stream())
    torch.cuda.synchronize()
    stats = ops.conv_path_stats(reset=True)
    fence.check('%s result' % which)
    ws.check('%s workspace' % which)
    return rc, out, fence, ws, stats


def served(pkg, case, which, family, **kw):
    """the call succeeds, exactly one launch is counted, in slot (family, which), and the result is within that family's bound of float64"""
    rc, out, _, _, stats = run(pkg, case, which, **kw)
    assert rc == 0, pkg._lib.lib().p3d_last_error()
    counts = {(f, p): stats[f][p][0] for f in ('x3', 'fp32') for p in PASSES}
    assert counts[(family, which)] == 1 and sum(counts.values()) == 1, (case.name, which, family, kw, counts)
    t = data(case)
    want = t['want']['fwd_bias' if kw.get('with_bias') else which]
    if case.accumulate:
        want = want + t['prior'][which].double()
    err = ((out.double() - want).abs().max() / want.abs().max()).item()          # (a pixel nothing wrote is still poison: NaN fails the comparison)
    tol = X3_TOL if family == 'x3' else CONV_TOL[which]
    print('%s %s %s %s: %.3g (bound %.3g)' % (case.name, which, family, kw, err, tol))
    assert err < tol, (case.name, which, family, kw, err)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_each_family_serves_its_calls(pkg, switches, case):
    set_x3, x3_any = switches
    x3_any(case.any_width)
    for which, x3 in zip(PASSES, case.x3):
        served(pkg, case, which, 'x3' if x3 else 'fp32')
        if case.name == 'masked_64' and which == 'fwd':
            served(pkg, case, which, 'fp32', with_bias=True)                       # the masked instances take no bias: the same call with one lands on fp32-MFMA


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_calls_the_x3_kernels_cannot_take_fall_to_fp32_mfma(pkg, switches, case):
    set_x3, x3_any = switches
    x3_any(case.any_width)
    for which, x3 in zip(PASSES, case.x3):
        served(pkg, case, which, 'fp32', misaligned=True)
        if x3 and which != 'wgrad' and case.stride == 1:                           # (the strided fp32-MFMA data gradient needs its whole staging buffer)
            served(pkg, case, which, 'fp32', short=16)
    if case.any_width:
        x3_any(False)
        for which in PASSES:
            served(pkg, case, which, 'fp32')
        x3_any(True)
    set_x3(False)
    for which in PASSES:
        served(pkg, case, which, 'fp32')


@pytest.mark.parametrize('case', [c for c in CASES if c.x3[2]], ids=[c.name for c in CASES if c.x3[2]])
def test_weight_gradient_with_a_short_workspace_is_refused(pkg, switches, case):
    """the route does not look at the workspace size: the call stays on the x3 kernels, whose entry refuses it before anything is launched"""
    set_x3, x3_any = switches
    x3_any(case.any_width)
    rc, out, fence, ws, stats = run(pkg, case, 'wgrad', short=16)
    assert rc == EWORKSPACE and b'workspace' in pkg._lib.lib().p3d_last_error()
    assert ws.untouched() and (case.accumulate or fence.untouched())
    if case.accumulate:
        assert torch.equal(out, data(case)['prior']['wgrad'])
    assert stats['fp32']['wgrad'][0] == 0
