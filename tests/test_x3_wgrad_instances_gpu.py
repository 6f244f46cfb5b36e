"""Every weight-gradient instance of the x3 convolution kernels (fx_wgrad_kernel<AIMG, BIMG, MASKED, TAPS, ROWS>, fx_wgrad_any_kernel, fx_wgrad_any_masked_kernel,
fx_wgrad_any_img_kernel, csrc/p3d_fx.hip) and each pass that sums their slabs (wgrad_finish, csrc/p3d_conv.hip; fx_stem_dw_kernel) against a float64 evaluation of the
same operation, alone: not through a residual block, an autograd Function and a chain-sized tolerance.

One row of tests/x3_wgrad_table.py = one call of the test hook p3d_fx_conv_wgrad_fused (the stem rows: p3d_stem_image(_masked) + p3d_stem_wgrad(_masked)) on an
exact-size, poisoned, fenced dw and workspace (tests/fenced.py), the workspace sized by the hook's own query.  A case asserts: return code 0; the fences intact; the
library's log of what it launched (ops.fx_wgrad_launch_log) holds exactly the row's record -- the kernel, its grid, the slabs, the block order, the finishing pass --, so a
planner change that takes a case off its instance fails by name; and the WHOLE dw against float64 (torch.nn.grad.conv2d_weight on double operands, on the GPU),
relative to the largest reference value -- an element nobody wrote is still poison (NaN) and fails the comparison.  The operation:
  dw (+= prior under 'acc') = wgrad(dy * mult, x * mask)
with the factors of a partial convolution where the row has them.  An image operand carries its factor: it is built, by the library's own image pass, from the fp32
product, and the reference uses that same product.  mask is drawn as in tests/test_fx_instances_gpu.py, mult as there from window counts, but of a second mask drawn the
same way, so that neither factor makes the other redundant; the first image of both is all zero, so its windows are empty and mult is 0 there.  Under 'win' dw is a channel
window of a wider weight: the channels outside it must be bit for bit what they held.  Under 'dwoff' dw starts one float into its buffer; that float stays poison.

Tolerance: X3_TOL (tests/test_kernels_gpu.py), the project's bound for reductions of up to 3200 terms; every row's reduction (N * Ho * Wo pixels) is at most that long
(tests/test_x3_wgrad_instances_host.py).  Measured on an MI355X: profiles/x3_wgrad_instances.md."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import fenced
import x3_wgrad_table as T
from test_kernels_gpu import X3_TOL
from x3_wgrad_table import ROWS

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(os.environ.get('P3D_X3', '1') == '0', reason='the x3 kernels are switched off')]

BAND = 4096                    # fence elements on each side of dw, bytes on each side of a workspace
EINVAL, EWORKSPACE = -1, -2


@pytest.fixture(scope='module', autouse=True)
def x3_on(pkg):
    L = pkg._lib.lib()
    assert (pkg._lib.CONSTANTS['P3D_EINVAL'], pkg._lib.CONSTANTS['P3D_EWORKSPACE']) == (EINVAL, EWORKSPACE)
    was = pkg.ops.set_x3(True)
    yield
    L.p3d_fx_tune(0, 0)
    pkg.ops.set_x3(was)


def conv_out(h, k, stride, pad, dil):
    return (h + 2 * pad - dil * (k - 1) - 1) // stride + 1


_cache = {}


def operands(row):
    """the operands of one row and the float64 weight gradient of its call; computed once per row and left unchanged"""
    if row.name in _cache:
        return _cache[row.name]
    o = set(row.opts)
    gen = torch.Generator(device='cuda').manual_seed(3000 + ROWS.index(row))
    n, c, k, h, w, r = row.n, row.c, row.k, row.h, row.w, row.r
    geom = (row.stride, row.pad, row.dil)
    ho, wo = conv_out(h, r, *geom), conv_out(w, r, *geom)

    def randn(*shape):
        return torch.randn(*shape, device='cuda', generator=gen)
    t = dict(x=randn(n, c, h, w), dy=randn(n, k, ho, wo), mult=None, mask=None, prior=None)
    c_total, c_offset = (c + T.WINDOW_EXTRA, T.WINDOW_OFFSET) if 'win' in o else (c, 0)
    t['c_total'], t['c_offset'] = c_total, c_offset
    if o & {'pm', 'em'} or row.entry == 'stem_masked':
        mask = (torch.rand(n, 1, h, w, device='cuda', generator=gen) >= 0.3).float()
        mask[0] = 0                                                                           # every window of the first image is empty: mult == 0 there
        # mult from the window counts of a SECOND mask, drawn alike: the two factors of a weight gradient are independent inputs, and with the mask's own counts a
        # 1x1 filter has mult == 0 exactly where mask == 0, so that dropping the x factor changes nothing (found with a build that ignored it)
        other = (torch.rand(n, 1, h, w, device='cuda', generator=gen) >= 0.3).float()
        other[0] = 0
        cnt = F.conv2d(other.double(), torch.ones(1, 1, r, r, device='cuda', dtype=torch.float64), None, *geom)
        mult = torch.where(cnt > 0, r * r / cnt.clamp(min=1), torch.zeros_like(cnt)).float()
        assert (mult == 0).any() and (mult > 0).any() and (mask == 0).any() and (mask > 0).any()
        if 'pm' in o or row.entry == 'stem_masked':
            t['mult'] = mult
        if 'em' in o or row.entry == 'stem_masked':
            t['mask'] = mask
    # the fp32 products an image operand is built from; the reference multiplies the same way, in float64 (a product with a 0 / 1 mask or by mult is then rounded
    # once more by the fp32 product the image pass reads: for an image operand the reference takes that rounded product)
    t['dy_eff'] = t['dy'] * t['mult'] if t['mult'] is not None else t['dy']
    t['x_eff'] = t['x'] * t['mask'] if t['mask'] is not None else t['x']
    dyd = t['dy_eff'].double() if 'dyimg' in o else (t['dy'].double() * t['mult'].double() if t['mult'] is not None else t['dy'].double())
    xd = t['x_eff'].double() if 'ximg' in o or row.entry != 'hook' else (t['x'].double() * t['mask'].double() if t['mask'] is not None else t['x'].double())
    want = torch.nn.grad.conv2d_weight(xd, (k, c, r, r), dyd, *geom)
    if 'acc' in o:
        t['prior'] = randn(k, c_total, r, r)
        want = want + t['prior'][:, c_offset:c_offset + c].double()
    t['want'] = want
    _cache[row.name] = t
    return t


def image(pkg, row, src):
    """the row's kind of image of an fp32 tensor, by the library's own pass (ops.act_image takes p3d_fx_act_image_any where H * W is no multiple of 4)"""
    ops, o = pkg.ops, set(row.opts)
    if 'rag' in o:
        n, c, h, w = src.shape
        img = torch.empty(pkg._lib.lib().p3d_fx_act_image_bytes(n, c, h * w), dtype=torch.uint8, device='cuda')
        pkg._lib.check(pkg._lib.lib().p3d_fx_act_image_any(ops._p(src.contiguous()), ops._p(img), n, c, h * w, ops._stream()), 'p3d_fx_act_image_any')
        return img
    return ops.row_image(src) if 'rows' in o else ops.act_image(src)


def result_buffer(row, t):
    """(the tensor handed to the call as dw, the whole weight it lies in, its fence, the extra leading float under 'dwoff' or None)"""
    o = set(row.opts)
    shape = (row.k, t['c_total'], row.r, row.r)
    numel = shape[0] * shape[1] * shape[2] * shape[3]
    if 'dwoff' in o:
        flat, fence = fenced.fenced_like((numel + 1,), torch.float32, BAND)
        whole, lead = flat[1:].view(shape), flat[:1]
    else:
        whole, fence = fenced.fenced_like(shape, torch.float32, BAND)
        lead = None
    if 'acc' in o:
        whole.copy_(t['prior'])
    return whole, fence, lead


def check_result(row, t, whole, before):
    o = set(row.opts)
    c0, c = t['c_offset'], row.c
    got = whole[:, c0:c0 + c]
    want = t['want']
    err = ((got.double() - want).abs().max() / want.abs().max()).item()
    print('ERR %s %s -> %s x3 %.3g tol %.3g' % (row.name, T.instance_name(T.instance(row.rec)), T.FINISH_NAMES[row.rec.finish], err, X3_TOL))
    assert err < X3_TOL, (row.name, err, X3_TOL)                                             # (a NaN -- an element nobody wrote -- fails it)
    if 'win' in o:
        outside = torch.ones(whole.shape, dtype=torch.bool, device='cuda')
        outside[:, c0:c0 + c] = False
        assert torch.equal(whole.view(torch.int32)[outside], before.view(torch.int32)[outside]), '%s: channels outside the window were written' % row.name


@pytest.mark.parametrize('row', ROWS, ids=[r.name for r in ROWS])
def test_instance_against_float64(pkg, row):
    ops, L = pkg.ops, pkg._lib.lib()
    o = set(row.opts)
    t = operands(row)
    whole, fence, lead = result_buffer(row, t)
    before = whole.clone()
    expected = [tuple(row.rec) + (0,) * (ops.FX_WGRAD_LAUNCH_LEN - len(row.rec))]
    if row.entry != 'hook':
        n, cin, h, w, k = row.n, row.c, row.h, row.w, row.k
        assert L.p3d_stem_supported(n, cin, h, w, k) == 1
        img = torch.empty(L.p3d_stem_image_bytes(n, h, w), dtype=torch.uint8, device='cuda')
        if row.entry == 'stem_masked':
            pkg._lib.check(L.p3d_stem_image_masked(ops._p(t['x']), ops._p(t['mask']), ops._p(img), n, cin, h, w, ops._stream()), 'p3d_stem_image_masked')
        else:
            pkg._lib.check(L.p3d_stem_image(ops._p(t['x']), ops._p(img), n, cin, h, w, ops._stream()), 'p3d_stem_image')
        nbytes = L.p3d_stem_workspace_bytes(n, h, w, k)
        ws = fenced.Fence(nbytes, BAND, 'cuda')
        torch.cuda.synchronize()
        ops.fx_wgrad_launch_log(reset=True)
        if row.entry == 'stem_masked':
            rc = L.p3d_stem_wgrad_masked(ops._p(t['dy']), ops._p(t['mult']), ops._p(img), ops._p(whole), n, cin, h, w, k, int('acc' in o), ops._p(ws.view), nbytes, ops._stream())
        else:
            rc = L.p3d_stem_wgrad(ops._p(t['dy']), ops._p(img), ops._p(whole), n, cin, h, w, k, int('acc' in o), ops._p(ws.view), nbytes, ops._stream())
        torch.cuda.synchronize()
        records, count = ops.fx_wgrad_launch_log(reset=True)
    else:
        d = ops._desc((row.n, row.c, row.h, row.w), (row.k, row.c, row.r, row.r), row.stride, row.pad, row.dil, c_offset=t['c_offset'], c_total=t['c_total'],
                      accumulate=int('acc' in o))
        f = pkg._lib.FxWgradFuse()
        dy_img = image(pkg, row, t['dy_eff']) if 'dyimg' in o else None
        x_img = image(pkg, row, t['x_eff']) if 'ximg' in o else None
        f.dy_img, f.x_img = ops._p(dy_img), ops._p(x_img)
        f.pmask = ops._p(t['mult']) if dy_img is None else None                               # an image carries its factor: the hook takes none for it
        f.emask = ops._p(t['mask']) if x_img is None else None
        f.rows, f.ragged = int('rows' in o), int('rag' in o)
        try:
            for what, value in row.tune:
                L.p3d_fx_tune(what, value)
            nbytes = L.p3d_fx_conv_wgrad_fused_workspace_bytes(ctypes.byref(d), ctypes.byref(f))
            assert nbytes > 0, row.name
            ws = fenced.Fence(nbytes, BAND, 'cuda')
            torch.cuda.synchronize()
            ops.fx_wgrad_launch_log(reset=True)
            stats0 = ops.conv_path_stats()
            rc = L.p3d_fx_conv_wgrad_fused(ctypes.byref(d), ctypes.byref(f), None if dy_img is not None else ops._p(t['dy']), None if x_img is not None else ops._p(t['x']),
                                           ops._p(whole), ops._p(ws.view), nbytes, ops._stream())
            torch.cuda.synchronize()
            records, count = ops.fx_wgrad_launch_log(reset=True)
        finally:
            for what, _ in row.tune:
                L.p3d_fx_tune(what, 0)
        assert ops.conv_path_stats() == stats0                                              # the hook does not count as a path launch
    fence.check('%s dw' % row.name)
    ws.check('%s workspace' % row.name)
    assert rc == 0, L.p3d_last_error()
    assert count == 1 and records == expected, (row.name, records and T.instance_name(T.instance(records[0])), records)
    if lead is not None:
        assert lead.view(torch.int32).item() == -1, '%s: the float in front of dw was written' % row.name
    check_result(row, t, whole, before)


def refused(pkg, d, f, dy, x, short=0):
    """one call of the hook that must be refused: (return code, launches logged, dw and the workspace still all poison)"""
    ops, L = pkg.ops, pkg._lib.lib()
    nbytes = L.p3d_fx_conv_wgrad_fused_workspace_bytes(ctypes.byref(d), ctypes.byref(f))
    assert nbytes > short
    dw, fence = fenced.fenced_like((d.K, d.c_total, d.R, d.S), torch.float32, BAND)
    ws = fenced.Fence(nbytes - short, BAND, 'cuda')
    torch.cuda.synchronize()
    ops.fx_wgrad_launch_log(reset=True)
    rc = L.p3d_fx_conv_wgrad_fused(ctypes.byref(d), ctypes.byref(f), ops._p(dy), ops._p(x), ops._p(dw), ops._p(ws.view), nbytes - short, ops._stream())
    torch.cuda.synchronize()
    _, count = ops.fx_wgrad_launch_log(reset=True)
    fence.check('dw of a refused call')
    ws.check('workspace of a refused call')
    return rc, count, fence.untouched() and ws.untouched()


def test_the_hook_refuses_operands_no_instance_takes(pkg):
    ops, L = pkg.ops, pkg._lib.lib()
    gen = torch.Generator(device='cuda').manual_seed(77)
    x, dy = torch.randn(2, 64, 8, 8, device='cuda', generator=gen), torch.randn(2, 64, 8, 8, device='cuda', generator=gen)
    mask, mult = torch.ones(2, 1, 8, 8, device='cuda'), torch.ones(2, 1, 8, 8, device='cuda')
    d = ops._desc((2, 64, 8, 8), (64, 64, 3, 3), 1, 1, 1)
    cases = {}
    f = pkg._lib.FxWgradFuse()                                                               # an x image without a dy image
    x_img = ops.act_image(x)
    f.x_img = ops._p(x_img)
    cases['x image alone'] = refused(pkg, d, f, dy, None)
    f = pkg._lib.FxWgradFuse()                                                               # a factor beside two images
    dy_img = ops.act_image(dy)
    f.dy_img, f.x_img, f.pmask, f.emask = ops._p(dy_img), ops._p(x_img), ops._p(mult), ops._p(mask)
    cases['factors beside two images'] = refused(pkg, d, f, None, None)
    f = pkg._lib.FxWgradFuse()                                                               # row images with a factor
    dy_rows = ops.row_image(dy)
    f.dy_img, f.emask, f.rows = ops._p(dy_rows), ops._p(mask), 1
    cases['rows with a factor'] = refused(pkg, d, f, None, x)
    # a ragged image pair whose K = 40 is no whole number of 16-channel groups (the buffers are never read: sized for 48 channels)
    d40 = ops._desc((3, 48, 5, 7), (40, 48, 1, 1), 1, 0, 1)
    dummy = torch.zeros(L.p3d_fx_act_image_bytes(3, 48, 35), dtype=torch.uint8, device='cuda')
    f = pkg._lib.FxWgradFuse()
    f.dy_img, f.x_img, f.ragged = ops._p(dummy), ops._p(dummy), 1
    cases['ragged image pair, K = 40'] = refused(pkg, d40, f, None, None)
    for what, (rc, count, untouched) in cases.items():
        assert rc == EINVAL and count == 0 and untouched, (what, rc, count, untouched, L.p3d_last_error())


def test_a_workspace_one_byte_short_is_refused(pkg):
    ops, L = pkg.ops, pkg._lib.lib()
    gen = torch.Generator(device='cuda').manual_seed(78)
    x, dy = torch.randn(2, 64, 8, 12, device='cuda', generator=gen), torch.randn(2, 32, 8, 12, device='cuda', generator=gen)
    d = ops._desc((2, 64, 8, 12), (32, 64, 3, 3), 1, 1, 1)
    rc, count, untouched = refused(pkg, d, pkg._lib.FxWgradFuse(), dy, x, short=1)
    assert rc == EWORKSPACE and count == 0 and untouched and b'fx_conv_wgrad_fused: workspace' in L.p3d_last_error(), (rc, count, untouched, L.p3d_last_error())


def test_the_log_counts_past_its_capacity_and_every_entry_writes_it(pkg):
    """more launches than the library keeps show as a count above the kept records; the per-layer entry and an image entry write the same log"""
    ops, L = pkg.ops, pkg._lib.lib()
    row = [r for r in ROWS if r.name == 'rows_1x1_k80_c48'][0]
    t = operands(row)
    d = ops._desc((row.n, row.c, row.h, row.w), (row.k, row.c, 1, 1), 1, 0, 1)
    f = pkg._lib.FxWgradFuse()
    dy_img, x_img = ops.row_image(t['dy']), ops.row_image(t['x'])
    f.dy_img, f.x_img, f.rows = ops._p(dy_img), ops._p(x_img), 1
    nbytes = L.p3d_fx_conv_wgrad_fused_workspace_bytes(ctypes.byref(d), ctypes.byref(f))
    ws, dw = torch.empty(nbytes, dtype=torch.uint8, device='cuda'), torch.empty(row.k, row.c, 1, 1, device='cuda')
    expected = tuple(row.rec) + (0,) * (ops.FX_WGRAD_LAUNCH_LEN - len(row.rec))
    torch.cuda.synchronize()
    ops.fx_wgrad_launch_log(reset=True)
    ops.fx_launch_log(reset=True)
    for _ in range(ops.FX_LOG_MAX + 3):
        assert L.p3d_fx_conv_wgrad_fused(ctypes.byref(d), ctypes.byref(f), None, None, ops._p(dw), ops._p(ws), nbytes, ops._stream()) == 0
    torch.cuda.synchronize()
    records, count = ops.fx_wgrad_launch_log(reset=False)
    assert count == ops.FX_LOG_MAX + 3 and len(records) == ops.FX_LOG_MAX and all(q == expected for q in records)
    assert ops.fx_wgrad_launch_log(reset=True)[1] == count and ops.fx_wgrad_launch_log() == ([], 0)
    # the image entry of the library writes the same record, and gives the same bits
    dw2 = ops.conv2d_img('wgrad', t['x'].shape, torch.empty(row.k, row.c, 1, 1, device='cuda'), 1, 0, 1, x_img=x_img, dy_img=dy_img, rows=True)
    torch.cuda.synchronize()
    records, count = ops.fx_wgrad_launch_log()
    assert count == 1 and records == [expected] and torch.equal(dw2, dw)
    # the forward / data-gradient log is a log of its own: no weight gradient shows there
    assert ops.fx_launch_log() == ([], 0)
