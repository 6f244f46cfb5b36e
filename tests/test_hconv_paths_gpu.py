"""Every path of the fp16 convolution kernels (csrc/p3d_hconv.hip: hconv_gather_kernel<32, EPI 0..4>, hconv_wgrad_kernel, hwgrad_reduce_kernel) against a float64
evaluation of the same operation, element by element.  One row of tests/hconv_table.py = one call through the C ABI; tests/test_hconv_paths_host.py shows on the
CPU which path each row takes and that the rows reach all of them.

Operands are fp16-exact and normal-distributed, weights scaled by 1 / sqrt(C R S).  `want` is the float64 evaluation on the device (F.conv2d / torch.nn.grad), with
mask, factor, bias, residual and ReLU applied in float64 in the documented order; `T` is the same evaluation on the absolute values, sum |terms| per element, with
|bias|, |res| and |old| added.  Every result, table and workspace lies in an exact-size poisoned fence (tests/fenced.py): dx is NaN before the call, so a class
without taps must write its zeros, and the weight-gradient workspace is exactly p3d_hconv2d_wgrad_workspace_bytes.

fp16 results, per element:   |got - want| <= 2^-10 (|want| + |conv| where the launch accumulates) + n 2^-23 T + 2^-24,   n = R S Kc + 4
  the fp16 rounding of the result (profiles/half_small_kernel_parity.md; EPI 1's accumulate rounds the convolution and the sum), n fp32 additions at one ulp each
  whatever the order the matrix core sums in (derived, not measured), and the fp16 subnormal step.
RMS, rows with n <= 576:     rms(got - want) <= 1.1 rms(ideal - want),  ideal = want through the roundings the entry documents (one to fp16; accumulate without
  mask_in: fp16(fp16(conv) + old)): 576 truncating additions add 576 * 2^-24 = 3.4e-5 relative beside the rounding's 2.8e-4, a factor of at most 1.01.
fp32 weight gradient:        |got - (base + scale want)| <= |scale| (kchunk + ceil(splits / 8) + 12) 2^-23 T + 2^-23 (|base| + |scale want|), and HCONV_TOL['wgrad'] of
  tests/test_half_gpu.py in the max norm.
Sum tables (EPI 2 / 3):      1e-5 * sum |terms| per channel, fed from the kernel's own rounded tensor, the ReLU sign taken from the exact x * sc + sh in float64.
Bit-level: the tensors of EPI 2 / 3 equal the plain launch's; a forward with a zero bias (EPI 0) equals the plain one (EPI 1) as values; fwd_infer without residual
and ReLU equals fwd with the same bias and factors.

Each case prints `hconv_paths <name> <largest error / bound> <rms ratio>` (pytest -s), what profiles/hconv_paths.md records."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import fenced
import hconv_table as T
from hconv_table import ROWS
from test_half_gpu import HCONV_TOL

pytestmark = pytest.mark.gpu

BAND = 4096                    # fence elements on each side of a tensor, bytes on each side of a workspace
U10, U23, U24 = 2.0 ** -10, 2.0 ** -23, 2.0 ** -24
RMS_FACTOR, RMS_TERMS = 1.1, 576
SUMS_TOL = 1e-5
P3D_EINVAL, P3D_EWORKSPACE = -1, -2


def nchw(t):
    """[N][H][W][C] memory -> its [N, C, H, W] view in float64"""
    return t.permute(0, 3, 1, 2).double()


class Operands:
    """the operands of one row, `want` and `T` of its pass (float64, NCHW), the convolution's own part `conv` where the launch accumulates, and `ideal`"""

    def __init__(self, row):
        self.row, o = row, set(row.opts)
        gen = torch.Generator(device='cuda').manual_seed(2000 + ROWS.index(row) if row in ROWS else 1999)
        n, c, h, w, k, r = row.n, row.c, row.h, row.w, row.k, row.r
        geom = (row.stride, row.pad, row.dil)
        self.ho, self.wo = T.out_hw(row)

        def randn(*shape):
            return torch.randn(*shape, device='cuda', generator=gen)
        self.x = randn(n, h, w, c).half()
        self.w = (randn(k, c, r, r) / math.sqrt(c * r * r)).half()
        creal = T.c_real(row) if row.entry == 'wgrad' else 3 if 'zpad' in o else c
        self.w[:, creal:] = 0
        self.x[..., creal:] = 0
        self.krsc, self.crsk = self.w.permute(0, 2, 3, 1).contiguous(), self.w.permute(1, 2, 3, 0).contiguous()
        self.dy = randn(n, self.ho, self.wo, k).half()
        # a {0,1} pixel mask with a window that holds no valid pixel, and the partial convolution's factor for it (0 there)
        mask = (torch.rand(n, h, w, device='cuda', generator=gen) >= 0.3).float()
        mask[0, :max(1, min(h - 1, r * row.dil + row.stride + 1)), :max(1, min(w - 1, r * row.dil + row.stride + 1))] = 0
        cnt = F.conv2d(mask[:, None].double(), torch.ones(1, 1, r, r, device='cuda', dtype=torch.float64), None, *geom)
        mult = torch.where(cnt > 0, r * r / cnt.clamp(min=1), torch.zeros_like(cnt)).float()[:, 0].contiguous()
        self.mask = mask if o & {'mask', 'xmask'} else None
        self.mult = mult if 'mult' in o else None
        self.bias = randn(k) if 'bias' in o else None
        self.res = randn(n, self.ho, self.wo, k).half() if 'res' in o else None
        self.old = self.conv = None
        wd = self.w.double()
        m64 = 1 if self.mask is None else self.mask[:, None].double()
        if row.entry in ('fwd', 'stats', 'infer'):
            xe = nchw(self.x) * m64
            f64 = 1 if self.mult is None else self.mult[:, None].double()
            want, tt = F.conv2d(xe, wd, None, *geom) * f64, F.conv2d(xe.abs(), wd.abs(), None, *geom) * f64
            if self.bias is not None:
                want, tt = want + self.bias.double().view(1, -1, 1, 1), tt + self.bias.double().abs().view(1, -1, 1, 1)
            if self.res is not None:
                want, tt = want + nchw(self.res), tt + nchw(self.res).abs()
            if 'relu' in o:
                want = want.clamp(min=0)
            self.ideal = want.half().double()
        elif row.entry in ('dgrad', 'sums'):
            dye = nchw(self.dy)
            want = torch.nn.grad.conv2d_input((n, c, h, w), wd, dye, *geom) * m64
            tt = torch.nn.grad.conv2d_input((n, c, h, w), wd.abs(), dye.abs(), *geom) * m64
            self.ideal = want.half().double()
            if 'acc' in o:
                self.old = randn(n, h, w, c).half()
                self.old[..., creal:] = 0
                self.conv = want
                # two roundings without a factor (EPI 1: the rounded convolution joins the rounded gradient, as autograd adds them), one with it (EPI 0)
                self.ideal = (want + nchw(self.old)).half().double() if self.mask is not None else (self.ideal + nchw(self.old)).half().double()
                want, tt = want + nchw(self.old), tt + nchw(self.old).abs()
            if row.entry == 'sums':
                self.c_prev = randn(n, h, w, c).half()
                self.c_prev[..., 0] = 0                             # channel 0: x * sc + sh is an exact zero, which `> 0` masks out
                u = torch.rand(4, c, device='cuda', generator=gen)
                self.coef = torch.stack([0.5 + u[0], (u[1] - 0.5) * 0.6, (u[2] - 0.5) * 0.4, 0.5 + 1.5 * u[3]], 1).contiguous()
                self.coef[0, 1] = 0
                self.coef[1, 0], self.coef[1, 1] = 0, 0.25          # channel 1: sc = 0, sh > 0, every pixel live
        else:
            xe, dye = nchw(self.x) * m64, nchw(self.dy)
            scale = 1.0 / 1024 if 'small' in o else 1.0
            self.scale = scale
            want = torch.nn.grad.conv2d_weight(xe, (k, c, r, r), dye, *geom)[:, :creal] * scale
            tt = torch.nn.grad.conv2d_weight(xe.abs(), (k, c, r, r), dye.abs(), *geom)[:, :creal]
            self.ideal = None
            if 'acc' in o:
                self.old = randn(k, creal, r, r)
                self.conv = want
                want = want + self.old.double()
        self.want, self.T = want, tt


def half_out(shape_nchw):
    return fenced.fenced_like(shape_nchw, torch.float16, BAND, channels_last=True)


def launch_gather(pkg, row, t, entry, out, partial=None, bias='own', accumulate=None):
    """one call of `entry` on the operands of `row`; returns the code"""
    ops, L = pkg.ops, pkg._lib.lib()
    p, st = ops._p, ops._stream()
    acc = int('acc' in row.opts) if accumulate is None else accumulate
    d = ops._desc((row.n, row.c, row.h, row.w), (row.k, row.c, row.r, row.r), row.stride, row.pad, row.dil, accumulate=acc)
    b = t.bias if bias == 'own' else bias
    if entry == 'fwd':
        return L.p3d_hconv2d_fwd(ctypes.byref(d), p(t.x), p(t.krsc), p(b), p(t.mask), p(t.mult), p(out), st)
    if entry == 'stats':
        return L.p3d_hconv2d_fwd_stats(ctypes.byref(d), p(t.x), p(t.krsc), p(out), p(partial), st)
    if entry == 'infer':
        return L.p3d_hconv2d_fwd_infer(ctypes.byref(d), p(t.x), p(t.krsc), p(b), p(t.mask), p(t.mult), p(t.res), int('relu' in row.opts), p(out), st)
    if entry == 'dgrad':
        return L.p3d_hconv2d_dgrad(ctypes.byref(d), p(t.dy), p(t.crsk), p(t.mask), p(out), st)
    assert entry == 'sums'
    return L.p3d_hconv2d_dgrad_sums(ctypes.byref(d), p(t.dy), p(t.crsk), p(out), p(t.c_prev), p(t.coef), p(partial), st)


def report(row, ratio, rms):
    print('hconv_paths %s %.4f %s' % (row.name, ratio, 'n/a' if rms is None else '%.4f' % rms))


def check_half(row, t, got, terms):
    """the per-element bound and the RMS bound of a fp16 result"""
    got = got.double()
    assert torch.isfinite(got).all(), 'an element nobody wrote (poison) or an overflow'
    err = (got - t.want).abs()
    bound = U10 * (t.want.abs() + (t.conv.abs() if t.conv is not None else 0)) + terms * U23 * t.T + U24
    ratio = float((err / bound).max())
    ideal = float((t.ideal - t.want).pow(2).mean().sqrt())
    mine = float((got - t.want).pow(2).mean().sqrt())
    rms = mine / ideal if ideal > 0 else (1.0 if mine == 0 else float('inf'))
    report(row, ratio, rms)
    worst = int((err / bound).argmax())
    assert ratio <= 1.0, 'element %d: got %r, want %r, error %.3e, bound %.3e' % (worst, float(got.flatten()[worst]), float(t.want.flatten()[worst]),
                                                                                    float(err.flatten()[worst]), float(bound.flatten()[worst]))
    if terms <= RMS_TERMS:
        assert rms <= RMS_FACTOR, 'rms error %.4e against %.4e of the ideal rounding' % (mine, ideal)


def check_sums(row, t, got, part, m):
    """the per-(pixel tile, channel) table against the sums of the kernel's own rounded tensor"""
    plan = T.gather_plan(row)
    assert tuple(part.shape) == (plan['tiles_n'], m // 8, 16)
    tot = part.double().sum(0)
    s1, s2 = tot[:, :8].reshape(-1), tot[:, 8:].reshape(-1)
    y = got.double().permute(0, 2, 3, 1).reshape(-1, m)                    # [pixels][channels]
    if row.entry == 'stats':
        a, b = y, y * y
    else:
        cf, coef = t.c_prev.double().reshape(-1, m), t.coef.double()
        live = cf * coef[:, 0] + coef[:, 1] > 0                            # exact in float64: a fp16 times a fp32 plus a fp32
        assert not live[:, 0].any() and live[:, 1].all()
        a = torch.where(live, y, torch.zeros_like(y))
        b = a * ((cf - coef[:, 2]) * coef[:, 3])
    e1, e2 = (s1 - a.sum(0)).abs(), (s2 - b.sum(0)).abs()
    b1, b2 = SUMS_TOL * a.abs().sum(0), SUMS_TOL * b.abs().sum(0)
    assert (e1 <= b1).all() and (e2 <= b2).all(), 'channel sums off by up to %.3e / %.3e of sum |terms|' % (
        float((e1 / b1.clamp(min=1e-300)).max()) * SUMS_TOL, float((e2 / b2.clamp(min=1e-300)).max()) * SUMS_TOL)


GATHER_ROWS = [r for r in ROWS if r.entry != 'wgrad']
WGRAD_ROWS = [r for r in ROWS if r.entry == 'wgrad']


@pytest.mark.parametrize('row', GATHER_ROWS, ids=[r.name for r in GATHER_ROWS])
def test_gather_path_against_float64(pkg, row):
    o, plan = set(row.opts), T.gather_plan(row)
    t = Operands(row)
    dgrad = T.is_dgrad(row)
    shape = (row.n, row.c, row.h, row.w) if dgrad else (row.n, row.k, t.ho, t.wo)
    m = shape[1]
    out, fence = half_out(shape)
    if t.old is not None:
        out.copy_(nchw(t.old))
    part = pfence = None
    if row.entry in ('stats', 'sums'):
        part, pfence = fenced.fenced_like((plan['tiles_n'], m // 8, 16), torch.float32, BAND)
    torch.cuda.synchronize()
    rc = launch_gather(pkg, row, t, row.entry, out, part)
    torch.cuda.synchronize()
    assert rc == 0, pkg._lib.lib().p3d_last_error()
    fence.check('the result')
    check_half(row, t, out, plan['terms'])
    if 'zpad' in o:
        assert not out[:, 3:].any(), 'padding channels of dx must be zero'
    if part is not None:
        pfence.check('the sum table')
        check_sums(row, t, out, part, m)
    # ---- bit-level cross-checks, one more launch each ----
    other = None
    if row.entry in ('stats', 'sums'):
        other = 'dgrad' if dgrad else 'fwd'                                # EPI 2 / 3 against the plain launch
        bias = None
    elif row.entry == 'fwd' and not o:
        other, bias = 'fwd', torch.zeros(row.k, device='cuda')            # EPI 1 against EPI 0 with a zero bias
    elif row.entry == 'infer' and not o & {'res', 'relu'}:
        other, bias = 'fwd', t.bias                                        # EPI 4 against EPI 0 / 1
    if other:
        out2, fence2 = half_out(shape)
        rc = launch_gather(pkg, row, t, other, out2, None, bias)
        torch.cuda.synchronize()
        assert rc == 0, pkg._lib.lib().p3d_last_error()
        fence2.check('the second result')
        assert torch.equal(out, out2), '%d of %d values differ from the %s launch' % (int((out != out2).sum()), out.numel(), other)


@pytest.mark.parametrize('row', WGRAD_ROWS, ids=[r.name for r in WGRAD_ROWS])
def test_wgrad_path_against_float64(pkg, row):
    ops, L = pkg.ops, pkg._lib.lib()
    plan = T.wgrad_plan(row)
    t = Operands(row)
    creal = T.c_real(row)
    d = ops._desc((row.n, row.c, row.h, row.w), (row.k, row.c, row.r, row.r), row.stride, row.pad, row.dil, accumulate=int('acc' in row.opts))
    need = L.p3d_hconv2d_wgrad_workspace_bytes(ctypes.byref(d))
    assert need == plan['splits'] * row.k * row.r * row.r * row.c * 4
    ws = fenced.Fence(need, BAND, 'cuda')
    dw, fence = fenced.fenced_like((row.k, creal, row.r, row.r), torch.float32, BAND)
    if t.old is not None:
        dw.copy_(t.old)
    torch.cuda.synchronize()
    rc = L.p3d_hconv2d_wgrad(ctypes.byref(d), ops._p(t.dy), ops._p(t.x), ops._p(t.mask), ops._p(dw), creal, t.scale, ops._p(ws.view), need, ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, L.p3d_last_error()
    fence.check('dw')
    ws.check('the workspace')
    got = dw.double()
    assert torch.isfinite(got).all()
    base = t.old.double().abs() if t.old is not None else 0
    part = t.conv if t.conv is not None else t.want                        # scale * wgrad
    err = (got - t.want).abs()
    bound = abs(t.scale) * (plan['kchunk'] + -(-plan['splits'] // 8) + 12) * U23 * t.T + U23 * (base + part.abs())
    ratio = float((err / bound.clamp(min=1e-300)).max())
    report(row, ratio, None)
    assert (err <= bound).all(), 'largest error / bound %.3f' % ratio
    assert float(err.max()) <= HCONV_TOL['wgrad'] * float(t.want.abs().max())


# ---- refusals: the code, and poisoned outputs left as they were ----------------------------------------------------------------------------------------
REFUSAL_ROW = T.Row('refusal', 'fwd', 2, 16, 9, 11, 24, 3, 1, 1, 1, ())
ENTRY_CALLS = ('fwd', 'stats', 'infer', 'dgrad', 'sums', 'wgrad')


@pytest.fixture(scope='module')
def refusal_operands():
    t = Operands(T.Row('refusal', 'sums', 2, 16, 9, 11, 24, 3, 1, 1, 1, ()))
    t.scale = 1.0
    return t


REFUSALS = ([(e, w) for e in ENTRY_CALLS for w in ('descriptor', 'null')] + [(e, 'accumulate') for e in ('fwd', 'stats', 'infer', 'sums')] + [('wgrad', 'short')])


@pytest.mark.parametrize('entry,what', REFUSALS, ids=['%s-%s' % v for v in REFUSALS])
def test_refusals_leave_the_outputs_alone(pkg, refusal_operands, entry, what):
    """C % 8 != 0, a null tensor, d->accumulate where the entry has none, and a workspace one byte short (p3d_hconv2d_wgrad; tests/test_scratch_bounds_gpu.py part 5
    holds the same entry 256 bytes short through the autograd op, with p3d_last_error naming it, which is not repeated here)"""
    ops, L = pkg.ops, pkg._lib.lib()
    p, st, t, row = ops._p, ops._stream(), refusal_operands, REFUSAL_ROW
    d = ops._desc((row.n, row.c, row.h, row.w), (row.k, row.c, row.r, row.r), row.stride, row.pad, row.dil, accumulate=int(what == 'accumulate'))
    if what == 'descriptor':
        d.C = d.c_total = 12
    dgrad = entry in ('dgrad', 'sums')
    out, fence = half_out((row.n, row.c, row.h, row.w) if dgrad else (row.n, row.k, t.ho, t.wo))
    part, pfence = fenced.fenced_like((2, (row.c if dgrad else row.k) // 8, 16), torch.float32, BAND)
    dw, wfence = fenced.fenced_like((row.k, row.c, row.r, row.r), torch.float32, BAND)
    need = L.p3d_hconv2d_wgrad_workspace_bytes(ctypes.byref(ops._desc((row.n, row.c, row.h, row.w), (row.k, row.c, row.r, row.r), row.stride, row.pad, row.dil)))
    ws = fenced.Fence(need, BAND, 'cuda')
    null = what == 'null'
    x, dy = (None if null else t.x), (None if null else t.dy)
    torch.cuda.synchronize()
    if entry == 'fwd':
        rc = L.p3d_hconv2d_fwd(ctypes.byref(d), p(x), p(t.krsc), None, None, None, p(out), st)
    elif entry == 'stats':
        rc = L.p3d_hconv2d_fwd_stats(ctypes.byref(d), p(x), p(t.krsc), p(out), p(part), st)
    elif entry == 'infer':
        rc = L.p3d_hconv2d_fwd_infer(ctypes.byref(d), p(x), p(t.krsc), None, None, None, None, 0, p(out), st)
    elif entry == 'dgrad':
        rc = L.p3d_hconv2d_dgrad(ctypes.byref(d), p(dy), p(t.crsk), None, p(out), st)
    elif entry == 'sums':
        rc = L.p3d_hconv2d_dgrad_sums(ctypes.byref(d), p(dy), p(t.crsk), p(out), p(t.c_prev), p(t.coef), p(part), st)
    else:
        rc = L.p3d_hconv2d_wgrad(ctypes.byref(d), p(dy), p(t.x), None, p(dw), row.c, 1.0, p(ws.view), need - (what == 'short'), st)
    torch.cuda.synchronize()
    assert rc == (P3D_EWORKSPACE if what == 'short' else P3D_EINVAL) and L.p3d_last_error()
    for f, name in ((fence, 'the result'), (pfence, 'the sum table'), (wfence, 'dw'), (ws, 'the workspace')):
        f.check(name)
        assert f.untouched(), '%s was written by a refused call' % name
