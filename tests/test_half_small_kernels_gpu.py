"""The fp16 (-half_acc) BatchNorm, pool, concat, ReLU, scale, layout and weight-image kernels past one pass of their grids: per-kernel parity with float64 at
the smallest sizes that reach each block cap, make a grid-stride loop iterate again, leave a ragged last trip, run both loops of hbn_sum_partials, give
gridDim.y = 2 or take the element-wise layout route.  Operands are exact in fp16.  The BatchNorm checks are split in two so that neither half hides the
other: the statistics (coefficients, running statistics, dgamma / dbeta) against float64 sums, and the apply passes against float64 arithmetic on the
kernel's OWN coefficients, per element.  Every output and workspace lies in an exact-size poisoned fence (tests/fenced.py): an element never written is a NaN,
a store past the end fails.  The caps these sizes cross are tabled in tests/test_half_small_kernels_host.py, which also evaluates on the CPU what the cases
rely on.  The element-wise float64 expressions run in torch on the device (float64 there is IEEE arithmetic like numpy's; the host file pins them to
oracle/np_ops.py on CPU tensors); the forward statistics come from oracle/np_ops.py itself.  Needs an MI355X: run with `-m gpu`."""
import functools

import numpy as np
import pytest
import torch

from fenced import fenced_like
from oracle import np_ops as ref

pytestmark = pytest.mark.gpu

STATS_TOL = 1e-5              # HBN_TOL['stats'] of tests/test_half_gpu.py
SUMS_TOL = 1e-5               # of sum |terms| per channel: the form and figure of test_hconv_epilogue_sums
EPS, MOMENTUM = 1e-5, 0.1

# ---- the geometry of p3d_hbn.hip, restated (the constants are tabled, by launch line, in the host file) ---------------------------------------------------------
HBN_MAX_BLOCKS, HBN_STREAM_BLOCKS, HBN_U = 512, 2048, 4


def hbn_geom(p, c):
    """(G, Gb, PL, blocks of the statistics / backward-sums launch, blocks of the apply launches, gridDim.y)"""
    g = c // 8
    gb = min(g, 256)
    pl = 256 // gb
    want = max(-(-(-(-p // pl)) // 8), 1)
    return g, gb, pl, min(want, HBN_MAX_BLOCKS), min(want, HBN_STREAM_BLOCKS), g // gb


def hbn_additions(p, c):
    """additions on the longest path into one fp32 block partial: a thread's pixels one after the other, then the PL pixel lanes of its channel group"""
    _, _, pl, nblk, _, _ = hbn_geom(p, c)
    return -(-(-(-p // pl)) // nblk) + pl


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------------------------------------
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def r16(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16)


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.float16 else t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


class Fenced:
    """The outputs and workspaces of one case: each an exact-size poisoned Fence with 64 KiB of sentinel on either side."""

    def __init__(self):
        self.fences = []

    def new(self, shape, dtype):
        t, f = fenced_like(shape if isinstance(shape, tuple) else (shape,), dtype, (1 << 16) // torch.empty((), dtype=dtype).element_size())
        self.fences.append(f)
        return t

    def holding(self, a):
        """a fenced tensor that starts out with the values of numpy array `a` (in/out arguments: running statistics, accumulated gradients)"""
        src = torch.from_numpy(np.ascontiguousarray(a))
        t = self.new(tuple(src.shape), src.dtype)
        t.copy_(src)
        return t

    def check(self):
        torch.cuda.synchronize()
        for i, f in enumerate(self.fences):
            f.check('fenced tensor %d of %d' % (i, len(self.fences)))


def call(pkg, name, *args):
    pkg._lib.check(getattr(pkg._lib.lib(), name)(*args), name)


# ---- float64 restatements, plain torch: on the device in the GPU cases, on CPU tensors in the host file --------------------------------------------------------------
def apply_want(x, res, coef, relu):
    """y = act(x * sc + sh + res) in float64 from a coefficient table [C][4] = {sc, sh, mean, invstd}; -> (want, sum of |terms|, the pre-activation without res)"""
    sc, sh = coef[:, 0].double(), coef[:, 1].double()
    prod = x.double() * sc
    pre = prod + sh
    terms = prod.abs_() + sh.abs()
    want = pre
    if res is not None:
        want = pre + res.double()
        terms += res.double().abs_()
    return (want.clamp_min(0) if relu else want), terms, pre


def bn_sums(g, x, coef):
    """float64 sum g, sum g * xhat per channel and the sums of their absolute values; xhat from the table's mean and invstd"""
    xhat = (x.double() - coef[:, 2].double()) * coef[:, 3].double()
    gx = g * xhat
    return g.sum(0), gx.sum(0), g.abs().sum(0), gx.abs().sum(0), xhat


def dx_want(g, xhat, coef, dg, db, p, frozen):
    """dx = sc * (g - db / P - xhat * dg / P) (frozen statistics: sc * g) -> (want, sum of |terms|)"""
    sc = coef[:, 0].double()
    t1 = g * sc
    if frozen:
        return t1, t1.abs()
    t2 = sc * db.double() / p
    t3 = xhat * (sc * dg.double() / p)
    return t1 - t2 - t3, t1.abs() + t2.abs() + t3.abs_()


def ratio(got, want, terms):
    """largest |got - want| over its bound 2^-10 |want| + 2^-20 sum |terms| + 2^-24: one fp16 rounding, a few fp32 roundings, the fp16 subnormal floor.
    A NaN (an element never written) gives inf."""
    bound = want.abs() * 2.0 ** -10 + terms * 2.0 ** -20 + 2.0 ** -24
    r = ((got.double() - want).abs() / bound)
    return float(torch.nan_to_num(r, nan=float('inf')).max())


def mask_bytes(y, c):
    """bit e of byte [pixel][group] = [y > 0] of the group's channel e"""
    w = (2 ** torch.arange(8, dtype=torch.int32, device=y.device))
    return ((y.reshape(-1, c // 8, 8) > 0).to(torch.int32) * w).sum(-1).to(torch.uint8)


def live_of(relu, res, x, coef, y):
    """the ReLU mask the way the backward kernels take it: from y with a residual, else the sign of the exact x * sc + sh (fmaf rounds once and keeps the sign;
    float64 holds the product of an fp16 and an fp32 number exactly, and its one rounding of the sum keeps the sign too)"""
    if not relu:
        return None
    if res is not None:
        return y > 0
    return (x.double() * coef[:, 0].double() + coef[:, 1].double()) > 0


def check_sums(tag, dg, db, sums, scale=1.0):
    s1, s2, a1, a2 = sums[:4]
    e1 = float(((db.double() - s1).abs() / (a1 * SUMS_TOL + 1e-300)).max())
    e2 = float(((dg.double() - s2).abs() / (a2 * SUMS_TOL + 1e-300)).max())
    print('HSK %s dbeta %.3f dgamma %.3f of the bound 1e-5 * sum|terms|' % (tag, e1, e2))
    assert e1 <= 1 and e2 <= 1, (tag, e1, e2)           # (a NaN fails the comparison)


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


# ---- BatchNorm -----------------------------------------------------------------------------------------------------------------------------------------------------------
HBN_SIZES = [(2048, 1), (2048, 7), (2048, 136), (2048, 523), (2048, 4096), (2048, 4101), (2048, 16389), (1024, 8195), (4096, 37), (64, 769),
             (8, 255), (8, 257), (8, 2049)]                                   # (C, P)
HBN_MODES = [(0, 0), (1, 0), (1, 1), (0, 1)]                                  # (relu, residual)
HBN_CASES = [(c, p, relu, res) for c, p in HBN_SIZES for relu, res in HBN_MODES if p != 16389 or relu]
HBN_FROZEN_SIZES = [(2048, 523), (2048, 4101), (64, 769)]


# (the cache holds one size: the modes of a size are listed, and run, back to back, and the 16 389 size is 200 MB.  The arrays are handed out by reference:
# no case may write to them.)
@functools.lru_cache(maxsize=1)
def hbn_inputs(c, p):
    """x at mean 1, std 2 as in test_hbn_train_fwd_bwd (this file does not probe the cancellation in E[x^2] - mean^2); flat [P][C]"""
    rng = np.random.default_rng(c * 100003 + p)
    x = (rng.standard_normal((p, c), dtype=np.float32) * 2 + 1).astype(np.float16)
    res = rng.standard_normal((p, c), dtype=np.float32).astype(np.float16)
    dy = rng.standard_normal((p, c), dtype=np.float32).astype(np.float16)
    gamma = (1 + 0.2 * rng.standard_normal(c)).astype(np.float32)
    beta = (0.3 * rng.standard_normal(c)).astype(np.float32)
    rm = rng.standard_normal(c).astype(np.float32)
    rv = (1 + rng.random(c)).astype(np.float32)
    dg0, db0 = rng.standard_normal(c).astype(np.float32), rng.standard_normal(c).astype(np.float32)
    return dict(x=x, res=res, dy=dy, gamma=gamma, beta=beta, rm=rm, rv=rv, dg0=dg0, db0=db0)


def run_bwd(pkg, f, entry, dy, x, y_or_mask, coef, with_res, p, c, relu, init, ws):
    """one backward launch into fresh fenced outputs; init: None (accumulate = 0, outputs poisoned) or the (dgamma, dbeta) to accumulate onto"""
    ops = pkg.ops
    ptr, st = ops._p, ops._stream()
    dx = f.new((p, c), torch.float16)
    dres = f.new((p, c), torch.float16) if with_res else None
    dg = f.holding(init[0]) if init else f.new(c, torch.float32)
    db = f.holding(init[1]) if init else f.new(c, torch.float32)
    acc = int(init is not None)
    if entry == 'p3d_hbn_train_bwd_mask':
        call(pkg, entry, ptr(dy), ptr(x), ptr(y_or_mask), ptr(coef), ptr(dx), ptr(dres), ptr(dg), ptr(db), p, c, acc, ptr(ws), ws.numel(), st)
    else:
        call(pkg, entry, ptr(dy), ptr(x), ptr(y_or_mask), ptr(coef), ptr(dx), ptr(dres), ptr(dg), ptr(db), p, c, relu, acc, ptr(ws), ws.numel(), st)
    return dx, dres, dg, db


def check_bwd(pkg, f, tag, entry, d, x, res, dy, y, coef, p, c, relu, ws, frozen):
    """The backward half shared by the training and the frozen entry: sums, dx per element from the kernel's own dgamma / dbeta, dres bit for bit, accumulate = 1."""
    live = live_of(relu, res, x, coef, y)
    g16 = dy if live is None else torch.where(live, dy, torch.zeros_like(dy))
    g = g16.double()
    y_arg = y if (relu and res is not None) else None
    dx, dres, dg, db = run_bwd(pkg, f, entry, dy, x, y_arg, coef, res is not None, p, c, relu, None, ws)
    sums = bn_sums(g, x, coef)
    check_sums(tag, dg, db, sums)
    want, terms = dx_want(g, sums[4], coef, dg, db, p, frozen)
    r = ratio(dx, want, terms)
    print('HSK %s dx %.3f of its bound' % (tag, r))
    assert r <= 1, (tag, r)
    if dres is not None:
        assert same_bits(dres, g16), tag
    dx1, dres1, dg1, db1 = run_bwd(pkg, f, entry, dy, x, y_arg, coef, res is not None, p, c, relu, (d['dg0'], d['db0']), ws)
    assert same_bits(dx1, dx) and (dres is None or same_bits(dres1, dres)), tag
    assert np.array_equal(host(dg1), d['dg0'] + host(dg)) and np.array_equal(host(db1), d['db0'] + host(db)), tag        # fp32 initial + value
    return dx, dres, dg, db


@pytest.mark.parametrize('case', HBN_CASES, ids=lambda k: 'c%d_p%d_relu%d_res%d' % k)
def test_hbn_train(case, pkg):
    c, p, relu, with_res = case
    ops = pkg.ops
    L = pkg._lib.lib()
    ptr, st = ops._p, ops._stream()
    tag = 'hbn_train c%d p%d relu%d res%d' % case
    d = hbn_inputs(c, p)
    nblk = hbn_geom(p, c)[3]
    x, dy, gamma, beta = dev(d['x']), dev(d['dy']), dev(d['gamma']), dev(d['beta'])
    res = dev(d['res']) if with_res else None
    f = Fenced()
    y, coef = f.new((p, c), torch.float16), f.new((c, 4), torch.float32)
    rm, rv = f.holding(d['rm']), f.holding(d['rv'])
    ws = f.new(L.p3d_hbn_workspace_bytes(c), torch.uint8)
    call(pkg, 'p3d_hbn_train_fwd', ptr(x), ptr(res), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(y), ptr(coef), p, c, MOMENTUM, EPS, relu, ptr(ws), ws.numel(), st)
    # statistics -> coefficients, against the oracle's float64
    _, mean, invstd, nrm, nrv = ref.bn_train_fwd(d['x'].reshape(p, c, 1, 1), d['gamma'], d['beta'], d['rm'], d['rv'], MOMENTUM, EPS)
    cf = host(coef)
    errs = (relerr(cf[:, 2], mean), relerr(cf[:, 3], invstd), relerr(cf[:, 0], invstd.astype(np.float64) * d['gamma']), relerr(host(rm), nrm), relerr(host(rv), nrv))
    print('HSK %s mean %.2e invstd %.2e sc %.2e running %.2e %.2e (bound 1e-5), %d blocks' % ((tag,) + errs + (nblk,)))
    assert max(errs) < STATS_TOL, (tag, errs)
    # apply, given the kernel's own coefficients
    want, terms, _ = apply_want(x, res, coef, relu)
    r = ratio(y, want, terms)
    print('HSK %s y %.3f of its bound' % (tag, r))
    assert r <= 1, (tag, r)
    if relu and with_res:
        # the same statistics as a table (the rows the statistics pass left in the workspace): finalize + apply, and the mask bytes
        y2, coef2, mask = f.new((p, c), torch.float16), f.new((c, 4), torch.float32), f.new(p * c // 8, torch.uint8)
        call(pkg, 'p3d_hbn_train_fwd_partial', ptr(x), ptr(res), ptr(gamma), ptr(beta), None, None, ptr(y2), ptr(coef2), p, c, MOMENTUM, EPS, 1, ptr(ws), nblk,
             ptr(mask), st)
        assert same_bits(y2, y) and same_bits(coef2, coef), tag
        assert torch.equal(mask, mask_bytes(y, c).reshape(-1)), tag
    got = check_bwd(pkg, f, tag, 'p3d_hbn_train_bwd', d, x, res, dy, y, coef, p, c, relu, ws, frozen=False)
    if relu and with_res:
        for init in (None, (d['dg0'], d['db0'])):
            via = run_bwd(pkg, f, 'p3d_hbn_train_bwd_mask', dy, x, mask, coef, True, p, c, 1, init, ws)
            assert same_bits(via[0], got[0]) and same_bits(via[1], got[1]), tag
            if init is None:
                assert same_bits(via[2], got[2]) and same_bits(via[3], got[3]), tag
            else:
                assert np.array_equal(host(via[2]), d['dg0'] + host(got[2])) and np.array_equal(host(via[3]), d['db0'] + host(got[3])), tag
    if relu and not with_res:
        # the table the backward-sums pass left in the workspace through the finalize + apply entry
        dx3, dg3, db3, scratch = f.new((p, c), torch.float16), f.new(c, torch.float32), f.new(c, torch.float32), f.new((c, 4), torch.float32)
        call(pkg, 'p3d_hbn_train_bwd_partial', ptr(dy), ptr(x), ptr(coef), ptr(dx3), ptr(dg3), ptr(db3), p, c, 0, ptr(ws), nblk, ptr(scratch), st)
        assert same_bits(dx3, got[0]) and same_bits(dg3, got[2]) and same_bits(db3, got[3]), tag
    f.check()


@pytest.mark.parametrize('with_res', (0, 1))
@pytest.mark.parametrize('size', HBN_FROZEN_SIZES, ids=lambda s: 'c%d_p%d' % s)
def test_hbn_eval_and_frozen(size, with_res, pkg):
    """p3d_hbn_eval_coef, p3d_hbn_eval_fwd (with and without ReLU) and p3d_hbn_frozen_bwd: the coefficients against float64 (sc, invstd: 1e-5 of the value; the mean is a copy;
    sh = beta - mean * sc within 2^-20 of |beta| + |mean * sc|, three fp32 roundings), then both passes per element from those coefficients."""
    c, p = size
    ops = pkg.ops
    L = pkg._lib.lib()
    ptr, st = ops._p, ops._stream()
    tag = 'hbn_frozen c%d p%d res%d' % (c, p, with_res)
    d = hbn_inputs(c, p)
    x, dy = dev(d['x']), dev(d['dy'])
    res = dev(d['res']) if with_res else None
    params = [dev(d[k]) for k in ('gamma', 'beta', 'rm', 'rv')]
    f = Fenced()
    coef = f.new((c, 4), torch.float32)
    call(pkg, 'p3d_hbn_eval_coef', *[ptr(t) for t in params], ptr(coef), c, EPS, st)
    cf = host(coef).astype(np.float64)
    invstd = 1.0 / np.sqrt(d['rv'].astype(np.float64) + EPS)
    sc = d['gamma'].astype(np.float64) * invstd
    assert (np.abs(cf[:, 3] - invstd) <= STATS_TOL * invstd).all() and (np.abs(cf[:, 0] - sc) <= STATS_TOL * np.abs(sc)).all() and np.array_equal(cf[:, 2], d['rm'])
    assert (np.abs(cf[:, 1] - (d['beta'] - d['rm'].astype(np.float64) * sc)) <= 2.0 ** -20 * (np.abs(d['beta']) + np.abs(d['rm'] * sc))).all()
    ws = f.new(L.p3d_hbn_workspace_bytes(c), torch.uint8)
    for relu in (0, 1):                                                                 # (the backward pass below takes the ReLU output, the last one)
        y = f.new((p, c), torch.float16)
        call(pkg, 'p3d_hbn_eval_fwd', ptr(x), ptr(res), *[ptr(t) for t in params], ptr(y), p, c, EPS, relu, ptr(ws), ws.numel(), st)
        want, terms, _ = apply_want(x, res, coef, relu)
        r = ratio(y, want, terms)
        print('HSK %s relu%d y %.3f of its bound' % (tag, relu, r))
        assert r <= 1, (tag, relu, r)
    check_bwd(pkg, f, tag, 'p3d_hbn_frozen_bwd', d, x, res, dy, y, coef, p, c, 1, ws, frozen=True)
    f.check()


# ---- hbn_sum_partials on synthetic tables ----------------------------------------------------------------------------------------------------------------------------
TABLE_ROWS = [1, 15, 16, 17, 48, 49, 63, 64, 65, 113, 512, 2048, 2051]
TABLE_CHANNELS = [8, 2048]
TABLE_P = 5
TABLE_VAR_FLOOR = 0.1


def table_inputs(rows, c):
    """[rows][C / 8][16] floats that need not be the sums of any x: [..., :8] standard normal (sum x, or sum g), [..., 8:] in 8 .. 16 (sum x^2, or sum g * xhat),
    which keeps every channel's variance sum2 / P - (sum1 / P)^2 well above the floor (the host file asserts it)"""
    rng = np.random.default_rng(rows * 4099 + c)
    t = np.empty((rows, c // 8, 16), dtype=np.float32)
    t[:, :, :8] = rng.standard_normal((rows, c // 8, 8))
    t[:, :, 8:] = rng.uniform(8, 16, (rows, c // 8, 8))
    d = dict(table=t, x=r16(rng.standard_normal((TABLE_P, c)) * 2 + 1), res=r16(rng.standard_normal((TABLE_P, c))), dy=r16(rng.standard_normal((TABLE_P, c))))
    d.update(gamma=(1 + 0.2 * rng.standard_normal(c)).astype(np.float32), beta=(0.3 * rng.standard_normal(c)).astype(np.float32),
             rm=rng.standard_normal(c).astype(np.float32), rv=(1 + rng.random(c)).astype(np.float32),
             dg0=rng.standard_normal(c).astype(np.float32), db0=rng.standard_normal(c).astype(np.float32))
    # (sc shrinks with the row count: the column sums grow with it, and dx = sc * (g - sum1 / P - xhat * sum2 / P) has to stay inside fp16)
    d['coef'] = np.stack([rng.uniform(0.5, 1.5, c) / rows, rng.standard_normal(c) * 0.3, 1 + rng.standard_normal(c) * 0.2, rng.uniform(0.5, 2.0, c)], 1).astype(np.float32)
    return d


def table_sums(t):
    """float64 column sums -> (sum1[C], sum2[C])"""
    tot = t.astype(np.float64).sum(0)
    return tot[:, :8].reshape(-1), tot[:, 8:].reshape(-1)


def table_stats(d):
    """float64 mean, biased variance and the rest of what hbn_fwd_finalize_kernel forms from a table's column sums"""
    s1, s2 = table_sums(d['table'])
    mean = s1 / TABLE_P
    var = s2 / TABLE_P - mean * mean
    invstd = 1.0 / np.sqrt(var + EPS)
    unbiased = var * TABLE_P / (TABLE_P - 1)
    m = float(np.float32(MOMENTUM))                       # the entry takes the momentum as a C float and forms 1.0 - momentum in double
    return dict(mean=mean, var=var, invstd=invstd, sc=invstd * d['gamma'], rm=(1 - m) * d['rm'].astype(np.float64) + m * mean, rv=(1 - m) * d['rv'].astype(np.float64) + m * unbiased)


def close(got, want):
    """1e-5 relative, per element: the sums are formed in fp64 on both sides, so only the final casts remain"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool((np.abs(got - want) <= STATS_TOL * np.abs(want) + 1e-12).all())


@pytest.mark.parametrize('c', TABLE_CHANNELS)
@pytest.mark.parametrize('rows', TABLE_ROWS)
def test_hbn_partial_tables(rows, c, pkg):
    ops = pkg.ops
    ptr, st = ops._p, ops._stream()
    p = TABLE_P
    tag = 'hbn_table rows%d c%d' % (rows, c)
    d = table_inputs(rows, c)
    table, x, res, dy, gamma, beta = (dev(d[k]) for k in ('table', 'x', 'res', 'dy', 'gamma', 'beta'))
    f = Fenced()
    # forward: finalize + apply + mask bytes
    y, coef, mask = f.new((p, c), torch.float16), f.new((c, 4), torch.float32), f.new(p * c // 8, torch.uint8)
    rm, rv = f.holding(d['rm']), f.holding(d['rv'])
    call(pkg, 'p3d_hbn_train_fwd_partial', ptr(x), ptr(res), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(y), ptr(coef), p, c, MOMENTUM, EPS, 1, ptr(table), rows,
         ptr(mask), st)
    want = table_stats(d)
    cf = host(coef)
    assert close(cf[:, 2], want['mean']) and close(cf[:, 3], want['invstd']) and close(cf[:, 0], want['sc']), tag
    assert close(host(rm), want['rm']) and close(host(rv), want['rv']), tag
    yw, terms, _ = apply_want(x, res, coef, 1)
    r = ratio(y, yw, terms)
    assert r <= 1, (tag, r)
    assert torch.equal(mask, mask_bytes(y, c).reshape(-1)), tag
    # backward: finalize + apply of a BatchNorm + ReLU layer without a residual, the mask recomputed from x and the given coefficients
    coef_b = dev(d['coef'])
    s1, s2 = table_sums(d['table'])
    live = live_of(1, None, x, coef_b, None)
    g = torch.where(live, dy, torch.zeros_like(dy)).double()
    xhat = (x.double() - coef_b[:, 2].double()) * coef_b[:, 3].double()
    outs = []
    for init in (None, (d['dg0'], d['db0'])):
        dx, scratch = f.new((p, c), torch.float16), f.new((c, 4), torch.float32)
        dg = f.holding(init[0]) if init else f.new(c, torch.float32)
        db = f.holding(init[1]) if init else f.new(c, torch.float32)
        call(pkg, 'p3d_hbn_train_bwd_partial', ptr(dy), ptr(x), ptr(coef_b), ptr(dx), ptr(dg), ptr(db), p, c, int(init is not None), ptr(table), rows, ptr(scratch), st)
        outs.append((dx, dg, db))
    (dx, dg, db), (dx1, dg1, db1) = outs
    assert close(host(db), s1) and close(host(dg), s2), tag
    dw, terms = dx_want(g, xhat, coef_b, dg, db, p, False)
    r2 = ratio(dx, dw, terms)
    assert r2 <= 1, (tag, r2)
    assert same_bits(dx1, dx) and np.array_equal(host(dg1), d['dg0'] + host(dg)) and np.array_equal(host(db1), d['db0'] + host(db)), tag
    print('HSK %s y %.3f dx %.3f of their bounds' % (tag, r, r2))
    f.check()


# ---- max pool --------------------------------------------------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(1, 8, 5, 7), (2, 16, 17, 15), (9, 64, 243, 241), (4, 8, 2049, 2049)]          # (N, C, H, W)


def pool_inputs(shape):
    """max(N(0, 1), 0): half the values tie at zero"""
    rng = np.random.default_rng(sum(shape))
    x = np.maximum(rng.standard_normal(shape, dtype=np.float32), 0).astype(np.float16).astype(np.float32)
    ho, wo = (shape[2] - 1) // 2 + 1, (shape[3] - 1) // 2 + 1
    dy = rng.standard_normal(shape[:2] + (ho, wo), dtype=np.float32).astype(np.float16).astype(np.float32)
    return x, dy


def nhwc(a, dtype=torch.float16):
    """NCHW numpy -> contiguous [N][H][W][C] device tensor"""
    return torch.from_numpy(a).cuda().permute(0, 2, 3, 1).contiguous().to(dtype)


@pytest.mark.parametrize('shape', POOL_SHAPES, ids=lambda s: '%dx%dx%dx%d' % s)
def test_hmaxpool_past_one_pass(shape, pkg):
    ops = pkg.ops
    ptr, st = ops._p, ops._stream()
    n, c, h, w = shape
    x, dy = pool_inputs(shape)
    y_ref, idx_ref = ref.maxpool3x3s2_fwd(x)
    dx_ref = ref.maxpool3x3s2_bwd(dy, idx_ref, x.shape)
    ho, wo = y_ref.shape[2:]
    f = Fenced()
    xt = nhwc(x)
    del x
    yt, it = f.new((n, ho, wo, c), torch.float16), f.new((n, ho, wo, c), torch.uint8)
    call(pkg, 'p3d_hmaxpool3x3s2_fwd', ptr(xt), ptr(yt), ptr(it), n, h, w, c, st)
    assert torch.equal(yt, nhwc(y_ref)) and torch.equal(it, nhwc(idx_ref, torch.uint8))
    dxt = f.new((n, h, w, c), torch.float16)
    dyt = nhwc(dy)
    call(pkg, 'p3d_hmaxpool3x3s2_bwd', ptr(dyt), ptr(it), ptr(dxt), n, h, w, c, st)
    want = nhwc(dx_ref, torch.float32)
    err = float((dxt.float() - want).abs().max()) / max(1.0, float(want.abs().max()))
    print('HSK hmaxpool %s backward %.2e (bound 2e-3)' % (shape, err))
    assert err < 2e-3                                                                   # (a NaN fails it)
    assert torch.equal(dxt != 0, want != 0)                                             # the bound is loose: the set of inputs that received a gradient, exactly
    f.check()


# ---- bit-exact kernels -------------------------------------------------------------------------------------------------------------------------------------------------
CONCAT_CASES = [(8, 24, 524291), (24, 8, 1), (64, 64, 100)]                             # (Ca, Cb, P)


@pytest.mark.parametrize('case', CONCAT_CASES, ids=lambda k: 'ca%d_cb%d_p%d' % k)
def test_hconcat_both_directions(case, pkg):
    ops = pkg.ops
    ptr, st = ops._p, ops._stream()
    ca, cb, p = case
    rng = np.random.default_rng(ca + p)
    a, b = r16(rng.standard_normal((p, ca), dtype=np.float32)), r16(rng.standard_normal((p, cb), dtype=np.float32))
    want = dev(np.concatenate([a, b], axis=1))
    f = Fenced()
    cat = f.new((p, ca + cb), torch.float16)
    at, bt = dev(a), dev(b)                            # (held in names: a tensor that dies right after its pointer was taken hands its memory to the next one)
    call(pkg, 'p3d_hconcat', ptr(at), ptr(bt), ptr(cat), p, ca, cb, 0, st)
    assert same_bits(cat, want)
    a2, b2 = f.new((p, ca), torch.float16), f.new((p, cb), torch.float16)
    call(pkg, 'p3d_hconcat', ptr(a2), ptr(b2), ptr(want), p, ca, cb, 1, st)
    assert same_bits(a2, at) and same_bits(b2, bt)
    f.check()


RELU_SIZES = [8, 8 * (2097152 + 5)]


def relu_inputs(n):
    """finite values only, with +0, -0, both signs of the smallest and the largest subnormal and of the largest finite number among them"""
    rng = np.random.default_rng(n)
    x = r16(rng.standard_normal(n, dtype=np.float32))
    special = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03ff, 0x83ff, 0x7bff, 0xfbff], dtype=np.uint16).view(np.float16)
    x[:8] = special
    x[-8:] = special[::-1]
    if n > 128:
        x[n // 2:n // 2 + 64] = np.resize(special, 64)
    dy = r16(rng.standard_normal(n, dtype=np.float32))
    dy[1] = np.float16(-0.0)
    return x, dy


@pytest.mark.parametrize('n', RELU_SIZES)
def test_hrelu_fwd_bwd(n, pkg):
    ops = pkg.ops
    ptr, st = ops._p, ops._stream()
    x, dy = relu_inputs(n)
    assert np.isfinite(x).all()
    zero = np.float16(0)
    f = Fenced()
    out, dx = f.new(n, torch.float16), f.new(n, torch.float16)
    xt, dyt = dev(x), dev(dy)
    call(pkg, 'p3d_hrelu', ptr(xt), None, ptr(out), n, st)
    call(pkg, 'p3d_hrelu', ptr(xt), ptr(dyt), ptr(dx), n, st)
    assert same_bits(out, dev(np.where(x > 0, x, zero))) and same_bits(dx, dev(np.where(x > 0, dy, zero)))
    f.check()


SCALE_CASES = [(2097155, 8), (1000, 72)]                                                # (P, C)


@pytest.mark.parametrize('case', SCALE_CASES, ids=lambda k: 'p%d_c%d' % k)
def test_hscale_pixels(case, pkg):
    ops = pkg.ops
    ptr, st = ops._p, ops._stream()
    p, c = case
    rng = np.random.default_rng(p)
    x = r16(rng.standard_normal((p, c), dtype=np.float32))
    scale = r16(rng.uniform(0, 9, p)).astype(np.float32)                                # the mult of a partial conv: 0 .. 9
    f = Fenced()
    out = f.new((p, c), torch.float16)
    xt, scale_t = dev(x), dev(scale)
    call(pkg, 'p3d_hscale_pixels', ptr(xt), ptr(scale_t), ptr(out), p, c, st)
    assert same_bits(out, dev((x.astype(np.float32) * scale[:, None]).astype(np.float16)))         # the fp32 product rounded once
    f.check()


TO_NHWC_CASES = [(2, 3, 1025 * 1025, 8), (3, 5, 63, 16), (2, 5, 4099, 16)]              # (N, C, HW, Cpad)
TO_NCHW_CASES = [('c8', 2, 8, 1025 * 1025, 0), ('c8', 3, 16, 63, 0), ('elementwise', 2, 17, 61700, 0), ('elementwise', 3, 5, 63, 0),
                 ('elementwise', 2, 8, 4099, 4)]                                       # (route, N, C, HW, halves the source starts off a 16-byte boundary)


@pytest.mark.parametrize('case', TO_NHWC_CASES, ids=lambda k: 'n%d_c%d_hw%d_cpad%d' % k)
def test_nchw_f32_to_nhwc_f16(case, pkg):
    ops = pkg.ops
    ptr, st = ops._p, ops._stream()
    n, c, hw, cpad = case
    x = r16(np.random.default_rng(hw).standard_normal((n, c, hw), dtype=np.float32)).astype(np.float32)
    want = np.zeros((n, hw, cpad), dtype=np.float16)
    want[:, :, :c] = (x * np.float32(2)).astype(np.float16).transpose(0, 2, 1)
    f = Fenced()
    out = f.new((n, hw, cpad), torch.float16)
    xt = dev(x)
    call(pkg, 'p3d_nchw_f32_to_nhwc_f16', ptr(xt), ptr(out), n, c, hw, cpad, 2.0, st)
    assert same_bits(out, dev(want))
    f.check()


@pytest.mark.parametrize('case', TO_NCHW_CASES, ids=lambda k: '%s_n%d_c%d_hw%d_off%d' % k)
def test_nhwc_f16_to_nchw_f32(case, pkg):
    """All three routes of p3d_nhwc_f16_to_nchw_f32: the 16-byte kernel, the element-wise kernel for C % 8 != 0, and the element-wise kernel for a source that is
    not 16-byte aligned (a view 8 bytes into its allocation)."""
    ops = pkg.ops
    ptr, st = ops._p, ops._stream()
    route, n, c, hw, off = case
    x = r16(np.random.default_rng(hw + c).standard_normal((n, hw, c), dtype=np.float32))
    room = torch.empty(n * hw * c + 16, dtype=torch.float16, device='cuda')
    start = (-room.data_ptr() % 16) // 2 + off
    src = room[start:start + n * hw * c].view(n, hw, c)
    src.copy_(torch.from_numpy(x))
    assert (route == 'c8') == (c % 8 == 0 and src.data_ptr() % 16 == 0) and src.data_ptr() % 16 == 2 * off
    f = Fenced()
    out = f.new((n, c, hw), torch.float32)
    call(pkg, 'p3d_nhwc_f16_to_nchw_f32', ptr(src), ptr(out), n, c, hw, 0.5, st)
    assert same_bits(out, dev(x.astype(np.float32).transpose(0, 2, 1) * np.float32(0.5)))
    f.check()


# ---- weight images -----------------------------------------------------------------------------------------------------------------------------------------------------
WEIGHT_CASES = [(512, 250, 9), (40, 24, 9), (8, 3, 1)]                                  # (K, C, RS)
BATCHED_JOBS = [(512, 512, 1, True), (72, 3, 49, False), (40, 24, 9, True)]              # (K, C, RS, with the [Cpad][RS][K] image)
BATCHED_GAP = 8                                                                        # poisoned halves between two images, and floats between two masters


def weight_inputs(k, c, rs):
    return r16(np.random.default_rng(k + c + rs).standard_normal((k, c, rs), dtype=np.float32) / np.sqrt(c * rs)).astype(np.float32)


def weight_images_want(w, cpad):
    """[K][C][RS] fp32 -> fp16 [K][RS][Cpad] and [Cpad][RS][K], the channels C .. Cpad - 1 zero"""
    k, c, rs = w.shape
    padded = np.zeros((k, cpad, rs), dtype=np.float16)
    padded[:, :c] = w.astype(np.float16)
    return np.ascontiguousarray(padded.transpose(0, 2, 1)), np.ascontiguousarray(padded.transpose(1, 2, 0))


@pytest.mark.parametrize('with_crsk', (True, False))
@pytest.mark.parametrize('case', WEIGHT_CASES, ids=lambda k: 'k%d_c%d_rs%d' % k)
def test_weight_images(case, with_crsk, pkg):
    ops = pkg.ops
    ptr, st = ops._p, ops._stream()
    k, c, rs = case
    cpad = (c + 7) // 8 * 8
    w = weight_inputs(k, c, rs)
    want_a, want_b = weight_images_want(w, cpad)
    f = Fenced()
    krsc = f.new((k, rs, cpad), torch.float16)
    crsk = f.new((cpad, rs, k), torch.float16) if with_crsk else None
    wt = dev(w)
    call(pkg, 'p3d_weight_images_f16', ptr(wt), ptr(krsc), ptr(crsk), k, c, rs, cpad, st)
    assert same_bits(krsc, dev(want_a)) and (crsk is None or same_bits(crsk, dev(want_b)))
    f.check()


def batched_plan():
    """-> (rows of the job table, floats of the flat master buffer, halves of the image buffer); a gap in front of, between and behind the images"""
    rows, w_off, img = [], BATCHED_GAP, BATCHED_GAP
    for k, c, rs, with_crsk in BATCHED_JOBS:
        cpad = (c + 7) // 8 * 8
        n = k * rs * cpad
        a = img
        img += n + BATCHED_GAP
        b = -1
        if with_crsk:
            b = img
            img += n + BATCHED_GAP
        rows.append((w_off, a, b, k, c, rs, cpad))
        w_off += k * c * rs + BATCHED_GAP
    return rows, w_off, img


def test_weight_images_batched(pkg):
    ops = pkg.ops
    ptr, st = ops._p, ops._stream()
    rows, nflat, nimg = batched_plan()
    flat = np.full(nflat, np.nan, dtype=np.float32)
    for (w_off, a, b, k, c, rs, cpad) in rows:
        flat[w_off:w_off + k * c * rs] = weight_inputs(k, c, rs).reshape(-1)
    table = np.array(rows, dtype=[('w', '<i8'), ('a', '<i8'), ('b', '<i8'), ('K', '<i4'), ('C', '<i4'), ('RS', '<i4'), ('Cpad', '<i4')])
    assert table.dtype.itemsize == 40
    f = Fenced()
    images = f.new(nimg, torch.float16)
    flat_t = dev(flat)
    table_t = dev(table.view(np.uint8).reshape(-1))
    call(pkg, 'p3d_weight_images_f16_batched', ptr(flat_t), ptr(images), ptr(table_t), len(rows), st)
    written = torch.zeros(nimg, dtype=torch.bool, device='cuda')
    for (w_off, a, b, k, c, rs, cpad) in rows:
        n = k * rs * cpad
        want_a, want_b = weight_images_want(flat[w_off:w_off + k * c * rs].reshape(k, c, rs), cpad)
        krsc = f.new((k, rs, cpad), torch.float16)                                      # the single-job entry on the same master
        crsk = f.new((cpad, rs, k), torch.float16) if b >= 0 else None
        call(pkg, 'p3d_weight_images_f16', ptr(flat_t[w_off:]), ptr(krsc), ptr(crsk), k, c, rs, cpad, st)
        assert same_bits(images[a:a + n].view(k, rs, cpad), krsc) and same_bits(krsc, dev(want_a)), (k, c, rs)
        written[a:a + n] = True
        if b >= 0:
            assert same_bits(images[b:b + n].view(cpad, rs, k), crsk) and same_bits(crsk, dev(want_b)), (k, c, rs)
            written[b:b + n] = True
    assert int((~written).sum()) == BATCHED_GAP * (1 + sum(1 + int(j[3]) for j in BATCHED_JOBS))
    assert bool((images.view(torch.int16)[~written] == -1).all())                       # the halves between the images still hold the poison
    f.check()


# ---- the regressor's bias gradient -------------------------------------------------------------------------------------------------------------------------------------
BGRAD_P = [1, 255, 257, 16389]
BGRAD_K = [8, 272]


@pytest.mark.parametrize('k', BGRAD_K)
@pytest.mark.parametrize('p', BGRAD_P)
def test_hconv2d_bgrad(p, k, pkg):
    ops = pkg.ops
    ptr, st = ops._p, ops._stream()
    rng = np.random.default_rng(p + k)
    dy = r16(rng.standard_normal((p, k), dtype=np.float32))
    init = rng.standard_normal(k).astype(np.float32)
    s, a = dy.astype(np.float64).sum(0), np.abs(dy.astype(np.float64)).sum(0)
    dyt = dev(dy)
    f = Fenced()
    for scale in (1.0, 1.0 / 1024):
        db, db1 = f.new(k, torch.float32), f.holding(init)
        call(pkg, 'p3d_hconv2d_bgrad', ptr(dyt), p, k, ptr(db), scale, 0, st)
        call(pkg, 'p3d_hconv2d_bgrad', ptr(dyt), p, k, ptr(db1), scale, 1, st)
        err = (np.abs(host(db).astype(np.float64) - scale * s) / (SUMS_TOL * scale * a + 1e-300)).max()
        print('HSK bgrad p%d k%d scale %g: %.3f of the bound 1e-5 * scale * sum|dy|' % (p, k, scale, err))
        assert err <= 1
        assert np.array_equal(host(db1), init + host(db))                               # fp32 initial + value
    f.check()
