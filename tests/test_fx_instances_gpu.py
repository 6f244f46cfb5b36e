"""Every forward / data-gradient instance of the x3 convolution kernels (fx_conv_kernel<AMODE, PRO, EPI, TAPI, RAG, ROWS>, fx16_conv_kernel<BM, EPI, TAPI, ROWS>,
csrc/p3d_fx.hip) and each pass that sums split-K slabs (fx_reduce_kernel<0 / 1 / 2>, fx_reduce_any_kernel) against a float64 evaluation of the same operation, alone:
not through a residual block, its BatchNorm layers and a chain-sized tolerance.

One row of tests/fx_table.py = one call of the test hook p3d_fx_conv_fused on exact-size, poisoned, fenced result, partial-sum and workspace buffers (tests/fenced.py).
A case asserts: return code 0; the fences intact; the library's own log of what it launched (ops.fx_launch_log) equals the row's records, so a planner change that takes
a case off its instance fails by name; and the WHOLE result against float64 (torch on the GPU), relative to the largest reference value -- an element nobody wrote is
still poison (NaN) and fails the comparison.  The operation:
  forward        conv(x * pmask) * emask (+ bias) (+ prior when accumulating) (+ res) (then ReLU) -- the factor before the bias, as stated at FX_EPI_INFER_FACTOR
  data gradient  dgrad(dy * pmask) * emask, plus the prior, or plus acc_src where its mask bit is set
The one exception to "every element written": the parity classes of a strided 1x1 data gradient that no tap reaches must STILL be poison, because the hook -- unlike
every entry point that hands out dx -- does not zero them.  With `accumulate` and a factor of 0 the prior must be unchanged bit for bit (include/p3d_hip.h).

Tolerance of the result: X3_TOL (tests/test_kernels_gpu.py) for reductions up to the 3200 terms it was stated for.  The longer ones ('long': >= 1024 channels x 9
taps) follow the rule of x3_case there: the fp32-MFMA kernel runs on the same operands and e_x3 < 4 e_fp32 + 2e-7 must hold with e_fp32 < CONV_TOL.  x3_case
compares the two families under the same plan (both cut K by the same rule), and so does this file: a row the built-in plan splits is compared with p3d_conv2d_fwd /
_dgrad as they plan it (split; measured x3 4.3e-7 ... 7.3e-7, fp32 4.8e-7 ... 9.6e-7); a row that forces its x3 launch unsplit (p3d_fx_tune(1, 1): the only way to the
tap-inner BatchNorm epilogues at a test's size) is compared with the same entry given no workspace, which keeps it unsplit too -- one fp32 chain over all 9216 terms
on either side (measured x3 1.7e-6 ... 4.1e-6, fp32 1.9e-6 ... 3.7e-6).  The launch record of the comparison run is checked, and the figure of the other plan is
printed: against the fp32 kernel WITH its split (5.3e-7 ... 8.6e-7) three unsplit rows would miss the rule (rag_img_dgrad_tapi_unsplit 4.05e-6 against 3.25e-6,
img_fwd_tapi_stats 3.21e-6 against 2.99e-6, x96_fwd_tapi_stats_144 3.22e-6 against 3.05e-6): that measures the plan, not the kernel (profiles/x3_instances.md).

Sums: partial[rows][M][2] (rows from p3d_fx_conv_fused_partial_rows) is added over rows in float64 and compared per channel with float64 sums of the reference.  The
summed value is conv (+ bias) (* emask); STATS: sum y, sum y^2; BWD_SUMS: sum g, sum g (c2 - mean) with g = value * [c2 sc + sh > 0].  ep_c is drawn so that
|c2 sc + sh| >= 1e-3 everywhere (offenders are pushed away, the condition is asserted), so no element's mask depends on rounding.  Bound per channel and sum:
terms * tol * max|summand| for the convolution's error (terms = the channel's pixels, tol as for the result) plus t * 2^-24 * sum|summand| for the fp32 summation, the
standard bound of a sum of t terms: t = 128 for an unsplit launch (one partial row per 128-pixel tile), ceil(N / groups) * OH * OW for the reduce pass.
No row combines sums with an accumulation: the unsplit kernels sum in front of it, fx_reduce_kernel behind it, and no caller in the library combines them.

Measured on an MI355X: profiles/x3_instances.md."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import fenced
import fx_table as T
from fx_table import ROWS
from test_kernels_gpu import CONV_TOL, X3_TOL

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(os.environ.get('P3D_X3', '1') == '0', reason='the x3 kernels are switched off')]

BAND = 4096                    # fence elements on each side of a tensor, bytes on each side of a workspace
U = 2.0 ** -24                 # unit roundoff of fp32
MARGIN = 1e-3                  # least |c2 * sc + sh| of the BatchNorm-backward rows


@pytest.fixture(scope='module', autouse=True)
def x3_on(pkg):
    L = pkg._lib.lib()
    was = pkg.ops.set_x3(True)
    yield
    for what in (1, 5):
        L.p3d_fx_tune(what, 0)
    pkg.ops.set_x3(was)


def conv_out(h, k, stride, pad, dil):
    return (h + 2 * pad - dil * (k - 1) - 1) // stride + 1


_cache = {}


def operands(row):
    """the operands of one row, the float64 result of its call and the float64 sums; computed once per row and left unchanged"""
    if row.name in _cache:
        return _cache[row.name]
    o = set(row.opts)
    gen = torch.Generator(device='cuda').manual_seed(2000 + ROWS.index(row))
    n, c, k, h, w, r = row.n, row.c, row.k, row.h, row.w, row.r
    geom = (row.stride, row.pad, row.dil)
    ho, wo = conv_out(h, r, *geom), conv_out(w, r, *geom)
    dg = row.pass_ == 'dgrad'
    img = bool(o & {'img', 'rows'})

    def randn(*shape):
        return torch.randn(*shape, device='cuda', generator=gen)

    def rand(*shape):
        return torch.rand(*shape, device='cuda', generator=gen)
    c_total, c_offset = (c + T.WINDOW_EXTRA, T.WINDOW_OFFSET) if 'win' in o else (c, 0)
    t = dict(c_total=c_total, c_offset=c_offset, pmask=None, emask=None, bias=None, prior=None, acc_src=None, acc_mask=None, res=None, ep_c=None, ep_tab=None, sums=None)
    t['w'] = randn(k, c_total, r, r) / ((k if dg else c) * r * r) ** 0.5
    wd = t['w'][:, c_offset:c_offset + c].double()
    t['src'] = randn(n, k, ho, wo) if dg else randn(n, c, h, w)
    if 'factor' in o:
        mask = (rand(n, 1, h, w) >= 0.3).float()
        mask[0] = 0                                                                           # every window of the first image is empty: mult == 0 there
        cnt = F.conv2d(mask.double(), torch.ones(1, 1, r, r, device='cuda', dtype=torch.float64), None, *geom)
        mult = torch.where(cnt > 0, r * r / cnt.clamp(min=1), torch.zeros_like(cnt)).float()
        assert (mult == 0).any() and (mult > 0).any() and (mask == 0).any() and (mask > 0).any()
        t['pmask'], t['emask'] = (mult, mask) if dg else (mask, mult)
        if img:
            t['pmask'] = None                                                                 # an image carries its factor: the hook takes none for it
    srce = t['src'].double() * (t['pmask'].double() if t['pmask'] is not None else 1)
    core = torch.nn.grad.conv2d_input((n, c, h, w), wd, srce, *geom) if dg else F.conv2d(srce, wd, None, *geom)
    if t['emask'] is not None:
        core = core * t['emask'].double()
    if 'bias' in o:
        t['bias'] = randn(k)
        core = core + t['bias'].double().view(1, -1, 1, 1)
    t['summed'] = core                                                                        # what the sums are taken of
    want = core
    shape = tuple(core.shape)
    if 'acc' in o:
        t['prior'] = randn(*shape)
        want = want + t['prior'].double()
    if 'accsrc' in o:
        t['acc_src'] = randn(*shape)
        add = t['acc_src'].double()
        if 'accmask' in o:
            bits = rand(core.numel()) >= 0.5
            t['acc_mask'] = (bits.view(-1, 4).to(torch.int32) << torch.arange(4, device='cuda', dtype=torch.int32)).sum(1).to(torch.uint8)
            add = add * bits.view(shape).double()
        want = want + add
    if 'res' in o:
        t['res'] = randn(*shape)
        want = want + t['res'].double()
    if 'relu' in o:
        want = want.clamp(min=0)
    t['want'] = want
    if 'sums' in o:
        if dg:
            m = c
            tab = torch.full((m, 8), float('nan'), device='cuda')                             # {sc, sh, mean, ...}: the epilogue reads the first three
            tab[:, 0], tab[:, 1], tab[:, 2] = rand(m) + 0.5, randn(m) * 0.5, randn(m) * 0.3
            sc, sh, mean = (tab[:, i].double().view(1, -1, 1, 1) for i in range(3))
            c2 = randn(*shape)
            z = c2.double() * sc + sh
            away = (z >= 0).double() * (4 * MARGIN) - 2 * MARGIN
            c2 = torch.where(z.abs() < 2 * MARGIN, (away - sh) / sc, c2.double()).float()     # push the elements a rounding could flip away from the threshold
            z = c2.double() * sc + sh
            assert z.abs().min().item() >= MARGIN and (z > 0).any() and (z < 0).any()
            t['ep_c'], t['ep_tab'] = c2, tab
            g = core * (z > 0)
            s1, s2 = g, g * (c2.double() - mean)
        else:
            s1, s2 = core, core * core
        t['sums'] = [(s.sum((0, 2, 3)), s.abs().sum((0, 2, 3)), s.abs().max().item()) for s in (s1, s2)]
    _cache[row.name] = t
    return t


def fp32_error(pkg, row, t, d, unsplit):
    """the same convolution on the fp32-MFMA kernels (x3 off), its error against float64 relative to the largest reference value.  unsplit: without workspace, which
    keeps that family's launch unsplit (its plan_splitk is the rule of fx_plan: left alone it cuts K into the same slabs); the record of the launch is checked"""
    ops, L = pkg.ops, pkg._lib.lib()
    dg = row.pass_ == 'dgrad'
    out = torch.empty(tuple(t['summed'].shape), device='cuda')
    was = ops.set_x3(False)
    try:
        nbytes = 0 if unsplit else (L.p3d_conv2d_dgrad_workspace_bytes if dg else L.p3d_conv2d_fwd_workspace_bytes)(ctypes.byref(d))
        ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda') if nbytes else None
        if dg:
            rc = L.p3d_conv2d_dgrad(ctypes.byref(d), ops._p(t['src']), ops._p(t['w']), None, None, ops._p(out), ops._p(ws), nbytes, ops._stream())
        else:
            rc = L.p3d_conv2d_fwd(ctypes.byref(d), ops._p(t['src']), ops._p(t['w']), ops._p(t['bias']), None, None, ops._p(out), ops._p(ws), nbytes, ops._stream())
        torch.cuda.synchronize()
        rec = ops.conv_last_fp32_launch()
    finally:
        ops.set_x3(was)
    assert rc == 0, L.p3d_last_error()
    assert rec['pass_'] == int(dg) and (rec['grid_y'] == 1) == bool(unsplit), (row.name, rec)
    return ((out.double() - t['summed']).abs().max() / t['summed'].abs().max()).item()


def weight_image(pkg, row, t):
    """the cached weight image of the row's pass: the data-gradient one from p3d_fx_weight_images (both channel counts in steps of 16); the forward one from
    p3d_fx_fold_bn_images without a BatchNorm, where the inference entries get theirs (any number of output channels: the last 128-row tile is zero-filled)"""
    L, ops, rs = pkg._lib.lib(), pkg.ops, row.r * row.r
    if row.pass_ == 'dgrad':
        fwd, bwd = ctypes.c_size_t(), ctypes.c_size_t()
        assert L.p3d_fx_weight_image_bytes(row.k, row.c, rs, ctypes.byref(fwd), ctypes.byref(bwd)) == 0, L.p3d_last_error()
        other, image = torch.empty(fwd.value, dtype=torch.uint8, device='cuda'), torch.empty(bwd.value, dtype=torch.uint8, device='cuda')
        assert L.p3d_fx_weight_images(ops._p(t['w']), row.k, row.c, rs, ops._p(other), ops._p(image), ops._stream()) == 0, L.p3d_last_error()
        return image
    image = torch.empty(rs * -(-row.k // 128) * (row.c // 16) * 3 * 4096, dtype=torch.uint8, device='cuda')
    job = pkg._lib.FoldJob()
    job.w, job.out = t['w'].data_ptr(), image.data_ptr()
    job.K, job.C, job.RS, job.c_offset, job.c_total, job.kind = row.k, row.c, rs, 0, row.c, 0
    jobs = torch.frombuffer(bytearray((pkg._lib.FoldJob * 1)(job)), dtype=torch.uint8).cuda()
    assert L.p3d_fx_fold_bn_images(ops._p(jobs), 1, 64, ops._stream()) == 0, L.p3d_last_error()
    torch.cuda.synchronize()                                                                  # (the job table is read by the launch)
    return image


@pytest.mark.parametrize('row', ROWS, ids=[r.name for r in ROWS])
def test_instance_against_float64(pkg, row):
    ops, L = pkg.ops, pkg._lib.lib()
    o = set(row.opts)
    t = operands(row)
    dg, rag = row.pass_ == 'dgrad', 'rag' in o
    d = ops._desc((row.n, row.c, row.h, row.w), (row.k, row.c, row.r, row.r), row.stride, row.pad, row.dil, c_offset=t['c_offset'], c_total=t['c_total'],
                  accumulate=int(bool(o & {'acc', 'accsrc'})))
    dref = ctypes.byref(d)
    tol, e32 = X3_TOL, None
    if 'long' in o:
        assert not (o & {'acc', 'accsrc', 'factor', 'res', 'relu', 'win'})                  # (the comparison run is the plain convolution)
        # like with like: a row whose x3 launch is forced unsplit (p3d_fx_tune(1, 1): the only way to its epilogue at a test's size) is judged against the
        # fp32-MFMA kernel unsplit as well -- one fp32 chain over all 9216 terms each; a row the plan splits, against that family's own (equal) split
        unsplit = row.recs[0].grid_y == 1
        e32 = fp32_error(pkg, row, t, d, unsplit)
        if unsplit:
            print('ERR %s fp32-MFMA with its planned split-K: %.3g' % (row.name, fp32_error(pkg, row, t, d, False)))
        tol = 4 * e32 + 2e-7

    f = pkg._lib.FxFuse()
    image = wimg = None
    if 'img' in o:
        image = ops.act_image(t['src'])
    elif 'rows' in o:
        image = ops.row_image(t['src'])
    if 'wimg' in o:
        wimg = weight_image(pkg, row, t)
    f.act_img, f.wimg = ops._p(image), ops._p(wimg)
    f.ep_c, f.ep_tab, f.pmask, f.emask = ops._p(t['ep_c']), ops._p(t['ep_tab']), ops._p(t['pmask']), ops._p(t['emask'])
    f.acc_src, f.acc_mask, f.res = ops._p(t['acc_src']), ops._p(t['acc_mask']), ops._p(t['res'])
    f.rows, f.infer, f.relu, f.ragged = int('rows' in o), int('infer' in o), int('relu' in o), int(rag)

    shape = tuple(t['want'].shape)
    m = shape[1]
    out, fence = fenced.fenced_like(shape, torch.float32, BAND)
    if 'acc' in o:
        out.copy_(t['prior'])
    partial = pfence = None
    try:
        for what, value in row.tune:
            L.p3d_fx_tune(what, value)
        nbytes = L.p3d_fx_conv_fused_workspace_bytes(int(dg), dref, int(rag))
        assert nbytes > 0, row.name
        ws = fenced.Fence(nbytes, BAND, 'cuda')
        if 'sums' in o:
            prows = L.p3d_fx_conv_fused_partial_rows(int(dg), dref)
            partial, pfence = fenced.fenced_like((prows, m, 2), torch.float32, BAND)
            f.partial = ops._p(partial)
        torch.cuda.synchronize()
        ops.fx_launch_log(reset=True)
        stats0 = ops.conv_path_stats()
        rc = L.p3d_fx_conv_fused(int(dg), dref, ctypes.byref(f), None if image is not None else ops._p(t['src']), ops._p(t['w']), ops._p(t['bias']), ops._p(out),
                                 ops._p(ws.view), nbytes, ops._stream())
        torch.cuda.synchronize()
        records, count = ops.fx_launch_log(reset=True)
    finally:
        for what, _ in row.tune:
            L.p3d_fx_tune(what, 0)
    fence.check('%s result' % row.name)
    ws.check('%s workspace' % row.name)
    if pfence is not None:
        pfence.check('%s partial sums' % row.name)
    assert rc == 0, L.p3d_last_error()
    assert ops.conv_path_stats() == stats0                                                  # the hook does not count as a path launch
    assert count == len(records) and records == [q._asdict() for q in row.recs], (row.name, [T.instance_name(tuple(q[n] for n in T.Rec._fields[:7])) for q in records], records)

    want, got = t['want'], out
    if dg and row.stride == 2 and row.r == 1:                                               # the classes no tap reaches: untouched by the hook
        dead = torch.ones(shape, dtype=torch.bool, device='cuda')
        dead[:, :, ::2, ::2] = False
        before = t['prior'].view(torch.int32)[dead] if 'acc' in o else torch.full((int(dead.sum()),), -1, dtype=torch.int32, device='cuda')
        assert torch.equal(out.view(torch.int32)[dead], before), '%s: a parity class no tap reaches was written' % row.name
        want, got = want[:, :, ::2, ::2], out[:, :, ::2, ::2]
    err = ((got.double() - want).abs().max() / want.abs().max()).item()
    print('ERR %s %s x3 %.3g%s tol %.3g' % (row.name, row.pass_, err, '' if e32 is None else ' fp32 %.3g' % e32, tol))
    if e32 is not None:
        assert e32 < CONV_TOL[row.pass_], (row.name, e32)
    assert err < tol, (row.name, err, tol)
    if 'factor' in o and 'acc' in o:                                                        # a factor of 0 leaves what the result held, bit for bit
        zero = (t['emask'] == 0).expand(shape)
        assert zero.any() and torch.equal(out.view(torch.int32)[zero], t['prior'].view(torch.int32)[zero]), '%s: prior changed under a zero factor' % row.name

    if 'sums' in o:
        q = row.recs[0]
        pixels = want.shape[0] * want.shape[2] * want.shape[3]
        terms = 128 if q.grid_y == 1 else -(-row.n // q.finish_groups) * want.shape[2] * want.shape[3]
        assert partial.shape[0] == (q.finish_groups if q.grid_y > 1 else -(-pixels // 128))
        mine = partial.double().sum(0)
        for i, (ref, ref_abs, ref_max) in enumerate(t['sums']):
            bound = pixels * tol * ref_max + terms * U * ref_abs
            diff = (mine[:, i] - ref).abs()
            worst = (diff / bound).max().item()
            print('SUM %s [%d] worst |diff| / bound %.3g (largest |diff| %.3g, largest |sum| %.3g)' % (row.name, i, worst, diff.max().item(), ref.abs().max().item()))
            assert bool((diff <= bound).all()), (row.name, i, worst)                       # (a NaN -- a sum nobody wrote -- fails it)


def test_the_log_counts_past_its_capacity_and_starts_anew_on_reset(pkg):
    """more launches than the library keeps show as a count above the kept records; an image entry of the library writes the same log (one launch function serves all)"""
    ops, L = pkg.ops, pkg._lib.lib()
    row = [r for r in ROWS if r.name == 'x64_rows_fwd_store_64'][0]
    t = operands(row)
    d = ops._desc((row.n, row.c, row.h, row.w), (row.k, row.c, row.r, row.r), row.stride, row.pad, row.dil)
    f = pkg._lib.FxFuse()
    image = ops.row_image(t['src'])
    f.act_img, f.rows = ops._p(image), 1
    nbytes = L.p3d_fx_conv_fused_workspace_bytes(0, ctypes.byref(d), 0)
    ws, out = torch.empty(nbytes, dtype=torch.uint8, device='cuda'), torch.empty(tuple(t['want'].shape), device='cuda')
    ops.fx_launch_log(reset=True)
    for _ in range(ops.FX_LOG_MAX + 3):
        assert L.p3d_fx_conv_fused(0, ctypes.byref(d), ctypes.byref(f), None, ops._p(t['w']), ops._p(t['bias']), ops._p(out), ops._p(ws), nbytes, ops._stream()) == 0
    torch.cuda.synchronize()
    records, count = ops.fx_launch_log(reset=False)
    assert count == ops.FX_LOG_MAX + 3 and len(records) == ops.FX_LOG_MAX and all(q == row.recs[0]._asdict() for q in records)
    assert ops.fx_launch_log(reset=True)[1] == count and ops.fx_launch_log() == ([], 0)
    # a per-layer entry on the x3 path writes the same log
    y = ops.conv2d_img('fwd', t['src'].shape, t['w'], row.stride, row.pad, row.dil, x_img=image, bias=t['bias'], rows=True)
    torch.cuda.synchronize()
    records, count = ops.fx_launch_log()
    assert count == 1 and records == [row.recs[0]._asdict()] and torch.equal(y, out)
