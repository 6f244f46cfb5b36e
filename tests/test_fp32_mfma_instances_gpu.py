"""Every instance of the fp32-MFMA convolution kernel (igemm_kernel<MODE, tile, TAPM, MASKED, WV>, csrc/p3d_conv.hip) and each of its finishing kernels against a
float64 evaluation of the same operation: the family every p3d_conv2d_fwd / _dgrad / _wgrad call lands on when the x3 kernels refuse it, and the one every dense
layer trains on at the default 257 crop.

One row of tests/fp32_mfma_table.py = one call through the C ABI on exact-size, poisoned, fenced result and workspace buffers.  A case asserts: return code 0;
exactly one launch counted, in the fp32 slot of its pass; the library's own record of what it launched (ops.conv_last_fp32_launch) equals the row's, so a planner
change that takes a case off its instance fails by name; and the WHOLE result within CONV_TOL (tests/test_kernels_gpu.py) of float64, relative to the largest
reference value -- an element nobody wrote is still poison (NaN) and fails the comparison.  The partial-convolution factors enter the reference in float64 in the
order of partial_conv.py:45-53: (conv(x * mask_in) * mult + bias) where mult > 0, else 0.  Reductions are no longer than the longest of CONV_CASES, so its bounds
apply unchanged.  x3 is switched off for the module, so the file runs the same under P3D_X3=0."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import fenced
from fp32_mfma_table import ROWS, WINDOW_EXTRA, WINDOW_OFFSET
from test_conv_routes_gpu import off_line
from test_kernels_gpu import CONV_TOL

pytestmark = pytest.mark.gpu

BAND = 4096                    # fence elements on each side of a result, bytes on each side of a workspace
EPS = 1e-5


@pytest.fixture(scope='module', autouse=True)
def x3_off(pkg):
    was = pkg.ops.set_x3(False)
    yield
    pkg.ops.set_x3(was)


def operands(row):
    """the operands of one row, and the float64 result of its pass"""
    o = set(row.opts)
    gen = torch.Generator(device='cuda').manual_seed(1000 + ROWS.index(row))
    n, c, k, h, w, r, s = row.n, row.c, row.k, row.h, row.w, row.r, row.s
    geom = (row.stride, row.pad, row.dil)

    def randn(*shape):
        return torch.randn(*shape, device='cuda', generator=gen)
    c_total, c_offset = (c + WINDOW_EXTRA, WINDOW_OFFSET) if 'win' in o else (c, 0)
    t = dict(x=randn(n, c, h, w), w=randn(k, c_total, r, s) / (c * r * s) ** 0.5, bias=randn(k) if 'bias' in o else None, mask=None, mult=None)
    t['c_total'], t['c_offset'] = c_total, c_offset
    wd = t['w'][:, c_offset:c_offset + c].double()
    xe = t['x'].double()
    mult = None
    if o & {'mask', 'mult'}:
        mask = (torch.rand(n, 1, h, w, device='cuda', generator=gen) >= 0.3).float()
        mask[0, 0, :min(h - 2, r * row.dil + row.stride + 1), :min(w - 2, s * row.dil + row.stride + 1)] = 0          # windows with no valid pixel: mult == 0 there
        cnt = F.conv2d(mask.double(), torch.ones(1, 1, r, s, device='cuda', dtype=torch.float64), None, *geom)
        mult = torch.where(cnt > 0, r * s / cnt.clamp(min=1), torch.zeros_like(cnt)).float()
        assert (mult == 0).any() and (mult > 0).any()
        if 'mask' in o:
            t['mask'] = mask
            xe = xe * mask.double()
        if 'mult' in o:
            t['mult'] = mult
    raw = F.conv2d(xe, wd, None, *geom)
    if row.entry in ('fwd', 'bn'):
        y = raw
        if row.entry == 'bn':
            t['gamma'], t['beta'], t['mean'], t['var'] = randn(k) * 0.3 + 1, randn(k), randn(k) * 0.5, torch.rand(k, device='cuda', generator=gen) + 0.5
            sc = t['gamma'].double() / (t['var'].double() + EPS).sqrt()
            y = y * sc.view(1, -1, 1, 1) + (t['beta'].double() - t['mean'].double() * sc).view(1, -1, 1, 1)
            t['res'] = randn(*y.shape) if 'res' in o else None
            if 'res' in o:
                y = y + t['res'].double()
            if 'relu' in o:
                y = y.clamp(min=0)
        if t['mult'] is not None:
            y = y * mult.double()
        if 'bias' in o:
            y = y + t['bias'].double().view(1, -1, 1, 1)
            if t['mult'] is not None:
                y = torch.where(mult.double() > 0, y, torch.zeros_like(y))
        want = y
    else:
        t['dy'] = randn(*raw.shape)
        dye = t['dy'].double() * (mult.double() if 'mult' in o else 1)
        if row.entry == 'dgrad':
            want = torch.nn.grad.conv2d_input((n, c, h, w), wd, dye, *geom)
            if 'mask' in o:
                want = want * t['mask'].double()
        else:
            want = torch.nn.grad.conv2d_weight(xe, (k, c, r, s), dye, *geom)
    t['prior'] = randn(*want.shape) if 'acc' in o else None
    if 'acc' in o:
        want = want + t['prior'].double()
    t['want'] = want
    return t


def result_buffer(shape, off_out):
    """(tensor, fence, slack): a poisoned exact-size tensor between two fences; with off_out it starts 4 bytes behind a 16-B line, inside an interior 16 bytes
    longer, whose 4 + 12 bytes of slack must stay poison"""
    if not off_out:
        out, fence = fenced.fenced_like(shape, torch.float32, BAND)
        return out, fence, None
    numel = 1
    for v in shape:
        numel *= v
    fence = fenced.Fence(numel * 4 + 16, BAND * 4, 'cuda')
    out = fence.view.view(torch.float32)[1:1 + numel].view(shape)
    assert out.data_ptr() % 16 == 4
    return out, fence, torch.cat([fence.view[:4], fence.view[4 + numel * 4:]])


@pytest.mark.parametrize('row', ROWS, ids=[r.name for r in ROWS])
def test_instance_against_float64(pkg, row):
    ops, L = pkg.ops, pkg._lib.lib()
    o = set(row.opts)
    t = operands(row)
    d = ops._desc(t['x'].shape, (row.k, row.c, row.r, row.s), row.stride, row.pad, row.dil, c_offset=t['c_offset'], c_total=t['c_total'], accumulate=int('acc' in o))
    dref = ctypes.byref(d)
    query = dict(fwd=L.p3d_conv2d_fwd_workspace_bytes, bn=L.p3d_conv2d_bn_eval_fwd_workspace_bytes, dgrad=L.p3d_conv2d_dgrad_workspace_bytes,
                 wgrad=L.p3d_conv2d_wgrad_workspace_bytes)[row.entry]
    given = [int(v[3:]) for v in row.opts if v.startswith('ws=')]
    nbytes = given[0] if given else query(dref)
    ws = fenced.Fence(nbytes, BAND, 'cuda')
    wsp = ops._p(ws.view) if nbytes else None

    window = row.entry == 'wgrad' and 'win' in o
    shape = (row.k, t['c_total'], row.r, row.s) if row.entry == 'wgrad' else tuple(t['want'].shape)
    out, fence, slack = result_buffer(shape, 'off_out' in o)
    mine = out[:, t['c_offset']:t['c_offset'] + row.c] if window else out
    if 'acc' in o:
        mine.copy_(t['prior'])
    before = out.clone() if window else None
    x = off_line(t['x']) if 'off_x' in o else t['x']
    dy = off_line(t['dy']) if 'off_dy' in o else t.get('dy')
    torch.cuda.synchronize()
    ops.conv_path_stats(reset=True)
    if row.entry == 'fwd':
        rc = L.p3d_conv2d_fwd(dref, ops._p(x), ops._p(t['w']), ops._p(t['bias']), ops._p(t['mask']), ops._p(t['mult']), ops._p(out), wsp, nbytes, ops._stream())
    elif row.entry == 'bn':
        rc = L.p3d_conv2d_bn_eval_fwd(dref, ops._p(x), ops._p(t['w']), ops._p(t['gamma']), ops._p(t['beta']), ops._p(t['mean']), ops._p(t['var']), EPS, ops._p(t['res']),
                                      int('relu' in o), ops._p(out), wsp, nbytes, ops._stream())
    elif row.entry == 'dgrad':
        rc = L.p3d_conv2d_dgrad(dref, ops._p(dy), ops._p(t['w']), ops._p(t['mult']), ops._p(t['mask']), ops._p(out), wsp, nbytes, ops._stream())
    else:
        rc = L.p3d_conv2d_wgrad(dref, ops._p(dy), ops._p(x), ops._p(t['mult']), ops._p(t['mask']), ops._p(out), wsp, nbytes, ops._stream())
    torch.cuda.synchronize()
    stats = ops.conv_path_stats(reset=True)
    record = ops.conv_last_fp32_launch()
    fence.check('%s result' % row.name)
    ws.check('%s workspace' % row.name)
    assert rc == 0, L.p3d_last_error()

    which = 'fwd' if row.entry == 'bn' else row.entry
    counts = {(f, p): stats[f][p][0] for f in ('x3', 'fp32') for p in ('fwd', 'dgrad', 'wgrad')}
    assert counts[('fp32', which)] == 1 and sum(counts.values()) == 1, (row.name, counts)
    assert record == row.rec._asdict(), (row.name, record)

    if slack is not None:
        assert bool((slack == 0xFF).all()), '%s: bytes beside the result were written' % row.name
    if window:                                                                  # the weight's other channels are not this call's to touch
        keep = torch.ones(shape, dtype=torch.bool, device='cuda')
        keep[:, t['c_offset']:t['c_offset'] + row.c] = False
        assert torch.equal(out.view(torch.int32)[keep], before.view(torch.int32)[keep]), '%s: weight channels outside the window were written' % row.name
    err = ((mine.double() - t['want']).abs().max() / t['want'].abs().max()).item()
    print('ERR %s %s %.3g %.3g' % (row.name, which, err, CONV_TOL[which]))
    assert err < CONV_TOL[which], (row.name, err)


EMPTY = dict(pass_=-1, tile=-1, tapm=0, masked=0, wv=0, grid_x=0, grid_y=0, y_means=0, weight_image=0, finish=0, eval=0, no_room=0)


def test_a_call_that_launches_nothing_on_this_family_leaves_an_empty_record(pkg):
    """a refused call and a call the x3 kernels serve (whose slabs go through the same wgrad_finish) clear what the call before them recorded"""
    ops, L = pkg.ops, pkg._lib.lib()
    row = [r for r in ROWS if r.name == 'wgrad_reduce_tapm'][0]
    test_instance_against_float64(pkg, row)
    assert ops.conv_last_fp32_launch() == row.rec._asdict()
    assert L.p3d_conv2d_fwd(None, None, None, None, None, None, None, None, 0, None) != 0
    assert ops.conv_last_fp32_launch() == EMPTY
    test_instance_against_float64(pkg, row)
    x = torch.randn(1, 128, 8, 8, device='cuda')
    d = ops._desc(x.shape, (128, 128, 1, 1), 1, 0, 1)
    assert L.p3d_conv2d_bn_eval_fwd(ctypes.byref(d), ops._p(x), ops._p(x), None, None, None, None, EPS, None, 0, ops._p(x), None, 0, ops._stream()) != 0      # no BatchNorm tensors
    assert ops.conv_last_fp32_launch() == dict(EMPTY, eval=1)
    test_instance_against_float64(pkg, row)
    ops.set_x3(True)
    try:
        dy, (dw, fence) = torch.randn(1, 128, 8, 8, device='cuda'), fenced.fenced_like((128, 128, 1, 1), torch.float32, BAND)
        nbytes = L.p3d_conv2d_wgrad_workspace_bytes(ctypes.byref(d))
        ws = fenced.Fence(nbytes, BAND, 'cuda')
        ops.conv_path_stats(reset=True)
        rc = L.p3d_conv2d_wgrad(ctypes.byref(d), ops._p(dy), ops._p(x), None, None, ops._p(dw), ops._p(ws.view), nbytes, ops._stream())
        torch.cuda.synchronize()
        stats = ops.conv_path_stats(reset=True)
    finally:
        ops.set_x3(False)
    fence.check('dw')
    ws.check('workspace')
    assert rc == 0 and stats['x3']['wgrad'][0] == 1 and stats['fp32']['wgrad'][0] == 0
    assert ops.conv_last_fp32_launch() == EMPTY
    want = torch.nn.grad.conv2d_weight(x.double(), (128, 128, 1, 1), dy.double())
    assert ((dw.double() - want).abs().max() / want.abs().max()).item() < 4e-6
