"""The scratch and output contract of the C ABI (include/p3d_hip.h): a launch reads no scratch byte it has not written itself, writes nothing outside
[workspace, workspace + the bytes its *_workspace_bytes query reported) and nothing outside the outputs it was handed, and a workspace shorter than the query is
refused with P3D_EWORKSPACE before anything is launched.

Everywhere else in the suite scratch is ops._scratch_buffer's grow-only buffer of at least 1 MiB, shared by every op of the process, and outputs are torch.empty
tensors the caching allocator rounds up: a query that reports too little, a kernel that reads a slab nobody wrote or a store past the end of an output all find
owned memory with plausible numbers in it.  Here every scratch request is answered with a fresh buffer of EXACTLY the requested size, filled with NaN bytes and
fenced by sentinel bands (tests/fenced.py; tests/test_fenced_host.py shows that such a fence can fail), and the existing parity bodies run on that:

  part 3   op-level cases under the `fenced_scratch` fixture: (a) the bound of the test the body is taken from, unchanged (a NaN read from scratch fails it),
           (b) the same call once more on the ordinary shared scratch gives the same bits
  part 4   outputs inside fences, straight through the C ABI
  part 5   a workspace 256 bytes short: P3D_EWORKSPACE, p3d_last_error() naming the entry, outputs untouched; NULL where the workspace is optional: the unsplit launch

Nothing here captures a graph (the fixture allocates).  Needs an MI355X: run with `-m gpu`.

Which test fences which entry point of include/p3d_hip.h (every one that takes a workspace or writes a buffer sized by a query):
  p3d_conv2d_fwd / _dgrad / _wgrad              test_fp32_conv, test_fp32_partial_conv, test_x3_conv, test_outputs_conv, test_outputs_conv_accumulate,
                                                test_short_workspace_is_refused[conv2d_*], test_optional_workspace_may_be_missing
  p3d_conv2d_bn_eval_fwd                        test_conv_bn_eval, test_short_workspace_is_refused[conv2d_bn_eval_fwd]
  p3d_block_fwd / _bwd (main and side workspace; aimg, dcimg, tables, out_mask: test_outputs_block; the weight images of
  p3d_fx_weight_images_batched)                 test_block_executor, test_masked_block_executor, test_outputs_block, ...[block_fwd / block_bwd]
  p3d_hblock_fwd / _bwd                         test_half_block_executor, test_half_training_step, ...[hblock_fwd / hblock_bwd]
  p3d_fx_weight_images, p3d_fx_fold_bn_images   test_outputs_weight_images_and_fold_kind0, test_outputs_fold_kind2, test_outputs_fold_kind3 (kind 1: test_folded_net)
  p3d_fx_act_image                              test_outputs_activation_image, test_image_fed_conv
  p3d_fx_conv_fwd_img / _dgrad_img / _wgrad_img test_image_fed_conv, ...[fx_conv_*_img]
  p3d_fx_conv_fwd_infer / _any / _masked        test_folded_conv_split_k, test_folded_conv_split_k_at_any_width, test_folded_masked_conv, test_folded_net,
                                                test_folded_net_any_size, ...[fx_conv_fwd_infer]
  p3d_stem_image(_masked), p3d_stem_weight_image, p3d_stem_fwd(_masked), p3d_stem_wgrad(_masked)
                                                test_stem, test_masked_stem, test_outputs_stem_images, ...[stem_wgrad]
  p3d_bn_train_fwd / _bwd, p3d_bn_eval_bwd      test_batchnorm_train, test_batchnorm_eval_backward, test_outputs_batchnorm, ...[bn_train_fwd / bn_train_bwd]
  p3d_stem_tail_fwd / _bwd                      test_stem_tail, ...[stem_tail_fwd / stem_tail_bwd]
  p3d_maxpool3x3s2_fwd                          test_outputs_maxpool
  p3d_distill_fwd_bwd                           test_distill, ...[distill]
  p3d_hconv2d_fwd / _dgrad / _wgrad, p3d_weight_images_f16      test_half_conv, test_outputs_half_conv, ...[hconv2d_wgrad]
  p3d_hconv2d_fwd_stats / _dgrad_sums           test_outputs_half_conv_partial_sums
  p3d_hbn_train_fwd / _bwd                      test_half_batchnorm, ...[hbn_train_fwd]; p3d_hbn_eval_fwd: test_folded_net_half (the unfolded fp16 model beside it)
  p3d_hbn_train_fwd_partial (relu_mask), p3d_hbn_train_bwd_mask  test_outputs_half_relu_mask
  whole steps (every entry a ResNet-18 step reaches, p3d_l2norm_sq_accum and the Adam kernels included)   test_training_step, test_half_training_step
  p3d_fx_conv_fwd_infer_any_workspace_bytes     test_folded_conv_split_k_at_any_width, test_folded_net_any_size (and test_infer_anysize_gpu's own fence test)
  p3d_hblock_workspace_bytes (the executor's tables and p3d_hbn_train_bwd_partial's coef2 lie inside its main workspace)   test_half_block_executor
  p3d_f8conv2d_weight_bytes                     test_outputs_fold_kind3
Left out: p3d_f8conv2d_fwd_infer / p3d_hconv2d_fwd_infer (no workspace; their y is the folded net's own allocation: parity and bits in test_folded_net_fp8 / _half, no
output fence), p3d_weight_images_f16_batched (sizes are the caller's shapes, no query; runs unfenced inside test_half_training_step), a direct call of
p3d_hbn_train_bwd_partial, p3d_hbn_frozen_bwd and the short-workspace call of p3d_bn_eval_bwd / p3d_hbn_train_bwd / p3d_hbn_eval_fwd (they share the size check of the entries
above, one function in csrc), the strided data gradient on the x3 kernels in part 5 (see SHORT), p3d_adam_step_dev's scratch16 (a fixed 16 bytes, no query)."""
import contextlib
import ctypes
import os
import zlib

import numpy as np
import pytest
import torch

import test_block_gpu as tb
import test_distill as td
import test_half_gpu as th
import test_infer_anysize_gpu as tia
import test_infer_fp8_gpu as ti8
import test_infer_gpu as ti
import test_infer_half_gpu as tih
import test_infer_partial_gpu as tip
import test_kernels_gpu as tk
import test_step_gpu as ts
from fenced import Fence, FencedAllocations
from oracle import np_ops as ref

pytestmark = pytest.mark.gpu
needs_blocks = pytest.mark.skipif(os.environ.get('P3D_X3', '1') == '0', reason='the block executor needs the x3 kernels, as in tests/test_block_gpu.py')

SCRATCH_BAND = 64 << 10        # at least this much on each side of a scratch buffer, and never less than the buffer itself: a slab, split or parity-class
#                                index one too high or too low still lands in memory the fence owns


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------------------
class FencedScratch:
    """Stands in for ops._scratch_buffer (behind ops.workspace and ops._side_launch, whoever imported them) and for the folded fp32 network's _ws: every request
    gets the interior of a fresh Fence of exactly `nbytes` bytes (16 for a request of 0: callers dereference .numel()), role 'side' allocated with the
    weight-gradient stream current as the original does.  Callers hand ws.numel() to the library, so the library sees exactly the size it reported."""

    def __init__(self, pkg):
        self.ops, self.infer = pkg.ops, pkg.infer
        self.fences = []                                     # (role, requested bytes, Fence), kept alive until the test ends
        self.originals = (self.ops._scratch_buffer, self.infer.FoldedNet._ws)
        self.short = 0                                       # part 5: hand out this many bytes less than were asked for

    def _buffer(self, device, nbytes, role):
        nbytes = int(nbytes)
        fence = Fence(nbytes or 16, max(nbytes, SCRATCH_BAND), device, stream=self.ops._side_stream(device) if role == 'side' else None)
        self.fences.append((role, nbytes, fence))
        cut = self.short if nbytes > self.short else min(nbytes, 4)      # (a query below `short` bytes -- a small table -- is answered one float short, not with nothing)
        return fence.view[:nbytes - cut] if self.short else fence.view

    @contextlib.contextmanager
    def short_by(self, nbytes):
        """every request answered with `nbytes` bytes less than it asked for (4 less where it asked for no more than that): callers pass .numel() on"""
        self.short = nbytes
        try:
            yield
        finally:
            self.short = 0

    def install(self):
        me = self
        self.ops._scratch_buffer = self._buffer
        self.infer.FoldedNet._ws = lambda net, nbytes: me._buffer(net.buffer.device, nbytes, 'infer')

    def remove(self):
        self.ops._scratch_buffer, self.infer.FoldedNet._ws = self.originals

    @contextlib.contextmanager
    def plain(self):
        """the ordinary scratch for a while: the run the fenced one is compared with"""
        self.remove()
        try:
            yield
        finally:
            self.install()

    def check(self):
        self.ops.join_side_stream()
        torch.cuda.synchronize()
        for i, (role, nbytes, fence) in enumerate(self.fences):
            fence.check("scratch request %d of %d (role '%s')" % (i, len(self.fences), role))


@pytest.fixture
def fenced_scratch(pkg):
    fs = FencedScratch(pkg)
    fs.install()
    try:
        yield fs
    finally:
        fs.remove()
    fs.check()


# ---- running a parity body twice and comparing what it compared ----------------------------------------------------------------------------------------
def _leaves(v, out):
    if isinstance(v, torch.Tensor):
        t = v.detach().contiguous().cpu().reshape(-1)
        out.append(t.view(torch.uint8).numpy().copy())
    elif isinstance(v, np.ndarray):
        out.append(np.ascontiguousarray(v).reshape(-1).view(np.uint8).copy())
    elif isinstance(v, torch.nn.Module):
        out.append(v)                                        # its state and gradients as they are when the body has ended (_settle)
    elif isinstance(v, dict):
        for k in v:
            _leaves(v[k], out)
    elif isinstance(v, (list, tuple)):
        for e in v:
            _leaves(e, out)


def _settle(tape):
    out = []
    for v in tape:
        if isinstance(v, torch.nn.Module):
            _leaves({k: t for k, t in v.state_dict().items()}, out)
            _leaves([p.grad for p in v.parameters() if p.grad is not None], out)
        else:
            out.append(v)
    return out


@contextlib.contextmanager
def _taped(watch):
    """Records, as bytes, every tensor / array that goes into or comes out of the named functions -- the comparison helpers a parity body hands its results to
    (tk.host, ti._rel, torch.equal, ...), or the factory that builds its model -- so that two runs of a body can be compared without the body returning anything."""
    tape, saved = [], []
    for obj, name in watch:
        orig = getattr(obj, name)

        def spy(*a, _orig=orig, **k):
            _leaves(a, tape)
            res = _orig(*a, **k)
            _leaves(res, tape)
            return res
        saved.append((obj, name, orig))
        setattr(obj, name, spy)
    try:
        yield tape
    finally:
        for obj, name, orig in saved:
            setattr(obj, name, orig)


def _run(body, watch):
    torch.manual_seed(0)                                     # (some bodies draw their inputs from the global generator)
    with _taped(watch) as tape:
        _leaves(body(), tape)
    torch.cuda.synchronize()
    return _settle(tape)


def fenced_then_plain(fs, body, watch=(), scratch=True):
    """(a) `body` -- an existing parity body, its own assertions inside -- on fenced, poisoned, exact-size scratch; the fences are checked; (b) once more on the
    ordinary scratch: every tensor the body compared or returned has the same bits.  scratch=False: a path that takes no workspace at all."""
    got = _run(body, watch)
    fs.check()
    assert not scratch or fs.fences, 'the case never asked for scratch: it does not test what it is here for'
    with fs.plain():
        again = _run(body, watch)
    assert len(got) == len(again) and len(got) > 0, (len(got), len(again))
    for i, (a, b) in enumerate(zip(got, again)):
        assert a.shape == b.shape and np.array_equal(a, b), 'result %d of %d is not bit-identical on fenced and on shared scratch (%d of %d bytes differ)' % (
            i, len(got), int((a != b).sum()) if a.shape == b.shape else -1, a.size)


def _params(fn, wanted=None, arg=None):
    """The rows of fn's own parametrization (the tables that are written inside a decorator; `arg`: of that argument, where it has several), all of them or those
    listed: nothing is copied that could drift"""
    rows = [m.args[1] for m in fn.pytestmark if m.name == 'parametrize' and arg in (None, m.args[0])][0]
    if wanted is None:
        return list(rows)
    missing = [w for w in wanted if w not in rows]
    assert not missing, missing
    return [r for r in rows if r in wanted]


def _named(table, names):
    rows = [r for r in table if r[0] in names]
    assert len(rows) == len(names)
    return rows


def _rows(table, wanted, width=None):
    rows = [r for r in table if (r if width is None else r[:width]) in wanted]
    assert len(rows) == len(wanted), rows
    return rows


@contextlib.contextmanager
def _tune(pkg, what, value):
    """p3d_fx_tune(what, value) around a body -- the size queries the ops make run under the same hook as their launches -- and back to the built-in plan"""
    L = pkg._lib.lib()
    L.p3d_fx_tune(what, value)
    try:
        yield
    finally:
        L.p3d_fx_tune(what, 0)


@contextlib.contextmanager
def _x3(pkg, on):
    before = pkg.ops.set_x3(on)
    try:
        yield
    finally:
        pkg.ops.set_x3(before)


# ---- part 3: op-level cases ------------------------------------------------------------------------------------------------------------------------------
# fp32-MFMA kernels: a strided 1x1, the four parity classes of a strided data gradient on an odd 33 x 31 map, the one-channel stem, K = 272 and the split-K shape
FP32_CASES = _named(tk.CONV_CASES, ('1x1s2', '3x3s2', '7x7s2c1', '3x3d2', 'big'))


@pytest.mark.parametrize('case', FP32_CASES, ids=[c[0] for c in FP32_CASES])
def test_fp32_conv(pkg, fenced_scratch, case):
    with _x3(pkg, False):
        fenced_then_plain(fenced_scratch, lambda: tk.test_conv_fwd_dgrad_wgrad(case, pkg), [(tk, 'host')])


def _partial_conv_case(pkg):
    """'3x3s2' of CONV_CASES (N 3, C 24, 33 x 31, K 70, stride 2) as a partial convolution (partial_conv.py:32-57): y = conv(x * mask_in) * mult and its two
    gradients against the oracle's partial_conv_fwd / partial_conv_bwd at the bounds of test_conv_fwd_dgrad_wgrad (tk.CONV_TOL); holes, empty windows included"""
    ops = pkg.ops
    _, n, c, h, w, k, ks, st, pad, dil, _ = _named(tk.CONV_CASES, ('3x3s2',))[0]
    rng = np.random.default_rng(17)
    x = rng.standard_normal((n, c, h, w)).astype(np.float32)
    wt = (rng.standard_normal((k, c, ks, ks)) / np.sqrt(c * ks * ks)).astype(np.float32)
    mask = (rng.random((n, 1, h, w)) > 0.3).astype(np.float32)
    mask[0, 0, :9, :11] = 0.0
    want_y, want_mo, mult = ref.partial_conv_fwd(x, mask, wt, None, st, pad, dil)
    dy = rng.standard_normal(want_y.shape).astype(np.float32)
    want_dx, want_dw = ref.partial_conv_bwd(dy, x, mask, wt, mult, st, pad, dil)
    xt, wtt, mt = tk.dev(x).requires_grad_(True), tk.dev(wt).requires_grad_(True), tk.dev(mask)
    multt, mo = ops.mask_count(mt, ks, st, pad, dil)
    y = ops.conv2d(xt, wtt, None, st, pad, dil, mask_in=mt, mult=multt)
    y.backward(tk.dev(dy))
    ops.join_side_stream()
    torch.cuda.synchronize()
    assert np.array_equal(tk.host(mo), want_mo) and (want_mo == 0).any()
    assert tk.relerr(tk.host(y), want_y) < tk.CONV_TOL['fwd']
    assert tk.relerr(tk.host(xt.grad), want_dx) < tk.CONV_TOL['dgrad']
    assert tk.relerr(tk.host(wtt.grad), want_dw) < tk.CONV_TOL['wgrad']


def test_fp32_partial_conv(pkg, fenced_scratch):
    with _x3(pkg, False):
        fenced_then_plain(fenced_scratch, lambda: _partial_conv_case(pkg), [(tk, 'host')])


X3_SHAPES = _rows(tk.X3_CASES, [(5, 192, 320, 8, 1, 1, 1), (3, 1024, 256, 16, 1, 1, 1), (3, 2048, 272, 16, 3, 1, 1), (6, 256, 256, 32, 3, 2, 1), (4, 256, 512, 64, 1, 2, 1),
                                (2, 128, 256, 32, 3, 1, 4)], width=7)
HOOKS = [None, (0, 2), (0, 3), (1, 2), (1, 3)]             # the built-in plan; forced weight-gradient splits; forced forward / data-gradient splits


@pytest.mark.parametrize('hook', HOOKS, ids=lambda h: 'builtin' if h is None else 'tune%d_%d' % h)
@pytest.mark.parametrize('case', X3_SHAPES, ids=['n%d_c%d_k%d_h%d_%dx%d_s%d_d%d' % (c[0], c[1], c[2], c[3], c[4], c[4], c[5], c[6]) for c in X3_SHAPES])
def test_x3_conv(pkg, fenced_scratch, case, hook):
    """x3_case runs the convolution on the fp32-MFMA and on the x3 kernels; torch.equal sees all six results"""
    n, c, k, h, r, stride, dil, with_bias = case
    with (_tune(pkg, *hook) if hook else contextlib.nullcontext()):
        fenced_then_plain(fenced_scratch, lambda: tk.x3_case(pkg, n, c, k, h, h, r, stride, dil * (r - 1) // 2, dil, with_bias), [(torch, 'equal')])


IMG_SHAPES = _rows(tk.IMG_CASES, [(2, 128, 16, 272, 3, 1, 1), (2, 128, 32, 128, 3, 2, 1), (2, 64, 16, 64, 5, 1, 1)])


@pytest.mark.parametrize('case', IMG_SHAPES, ids=lambda c: 'n%d_c%d_h%d_k%d_%dx%d_s%d_d%d' % (c[0], c[1], c[2], c[3], c[4], c[4], c[5], c[6]))
def test_image_fed_conv(pkg, fenced_scratch, case):
    n, c, h, k, ks, st, dil = case
    fenced_then_plain(fenced_scratch, lambda: tk.image_fed_case(pkg, n, c, h, h, k, ks, st, dil * (ks - 1) // 2, dil), [(tk, 'host')])


BN_SHAPES = _rows(tk.BN_CASES, [(3, 10, 17, 17), (2, 130, 8, 8), (5, 7, 5, 3), (3, 256, 4, 4)], width=4)


@pytest.mark.parametrize('case', BN_SHAPES, ids=lambda c: 'n%d_c%d_%dx%d' % c[:4])
def test_batchnorm_train(pkg, fenced_scratch, case):
    fenced_then_plain(fenced_scratch, lambda: tk.test_bn_train_fwd_bwd(*case, pkg), [(tk, 'host')])


def test_batchnorm_eval_backward(pkg, fenced_scratch):
    fenced_then_plain(fenced_scratch, lambda: tk.test_bn_eval_fwd_bwd(pkg), [(tk, 'host')])


@pytest.mark.parametrize('shape', _params(tk.test_stem_tail_is_bit_identical_to_batchnorm_relu_maxpool, [(3, 16, 32, 20), (2, 8, 6, 4)]), ids=lambda s: 'n%d_c%d_%dx%d' % s)
def test_stem_tail(pkg, fenced_scratch, shape):
    fenced_then_plain(fenced_scratch, lambda: tk.test_stem_tail_is_bit_identical_to_batchnorm_relu_maxpool(pkg, shape), [(torch, 'equal')])


@pytest.mark.parametrize('case', _params(tk.test_stem_on_the_x3_kernels, [(2, 3, 64, 64, 64), (3, 1, 48, 64, 64), (2, 4, 64, 64, 64)]), ids=lambda c: 'n%d_c%d_%dx%d_k%d' % c)
def test_stem(pkg, fenced_scratch, case):
    """forward, weight gradient and the weight image rebuilt after an update (its K * 256 floats of scratch are sized by hand in ops_block)"""
    fenced_then_plain(fenced_scratch, lambda: tk.test_stem_on_the_x3_kernels(case, pkg), [(tk, 'host')])


def test_masked_stem(pkg, fenced_scratch):
    case, = _params(tk.test_partial_conv_stem_on_the_restated_kernels, [(3, 1, 64, 64)])
    fenced_then_plain(fenced_scratch, lambda: tk.test_partial_conv_stem_on_the_restated_kernels(case, pkg), [(tk, 'host')])


def _smallest_per_geometry(cases):
    """the smallest case (pixels, then input channels) of each (kind, stride, dilation, downsample) combination of a block table"""
    best = {}
    for c in cases:
        kind, inplanes, planes, stride, dil, n, h, with_ds = c
        key = (kind, stride, dil, with_ds)
        if key not in best or (n * h * h, inplanes) < (best[key][5] * best[key][6] ** 2, best[key][1]):
            best[key] = c
    return list(best.values())


BLOCK_IDS = lambda c: '%s_c%d_p%d_s%d_d%d_n%d_h%d%s' % (c[0], c[1], c[2], c[3], c[4], c[5], c[6], '_ds' if c[7] else '')


# The split-K layout of the main workspace (the slabs lie inside the conv scratch, the partial rows are image groups), which the built-in plan never reaches on the
# small cases: an identity and a downsample block under forced forward / data-gradient splits.  (Masked blocks have unsplit instances only.)
SPLITK_BLOCKS = _rows(tb.CASES, [('bottleneck', 512, 128, 1, 1, 4, 16, False), ('bottleneck', 128, 128, 1, 1, 3, 32, True)])
EXECUTOR_CASES = [c + (None,) for c in _smallest_per_geometry(tb.CASES)] + [c + ((1, splits),) for c in SPLITK_BLOCKS for splits in (2, 3)]


@needs_blocks
@pytest.mark.parametrize('case', EXECUTOR_CASES, ids=lambda c: BLOCK_IDS(c) + ('_tune%d_%d' % c[8] if c[8] else ''))
def test_block_executor(pkg, fenced_scratch, case):
    """p3d_block_fwd / p3d_block_bwd on their main and side workspaces, and the per-layer path beside them"""
    hook = case[8]
    with (_tune(pkg, *hook) if hook else contextlib.nullcontext()):
        fenced_then_plain(fenced_scratch, lambda: tb.fused_block_case(pkg, *case[:8]), [(tb, 'rel'), (tb, 'rel2')])


@needs_blocks
@pytest.mark.parametrize('case', _smallest_per_geometry(tb.MASKED_CASES), ids=BLOCK_IDS)
def test_masked_block_executor(pkg, fenced_scratch, case):
    kind, inplanes, planes, stride, dil, n, h, with_ds = case
    fenced_then_plain(fenced_scratch, lambda: tb.masked_block_case(pkg, kind, inplanes, planes, stride, dil, n, h, h, with_ds), [(tb, 'rel'), (torch, 'equal')])


def _hconv_op_case(pkg, case):
    """The geometry and data of test_half_gpu.test_hconv_fwd_dgrad_wgrad through the autograd op (ops_half.conv2d), whose weight gradient takes its workspace from
    ops._side_launch; forward, data gradient and weight gradient against the float64 oracle at that test's bounds (th.HCONV_TOL)."""
    oh = pkg.ops_half
    name, n, c, h, w, k, ks, st, pad, dil = case
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x = th.r16(rng.standard_normal((n, c, h, w)))
    wt = th.r16(rng.standard_normal((k, c, ks, ks)) / np.sqrt(c * ks * ks))
    y_ref = ref.conv2d_fwd(x, wt, None, st, pad, dil)
    dy = th.r16(rng.standard_normal(y_ref.shape))
    conv = pkg.nn.Conv2d(c, k, ks, stride=st, padding=pad, dilation=dil, bias=False).cuda()
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(wt))
    oh.refresh_weights(conv)
    need_dx = c >= 8                                        # (a stem has no data-gradient weight image)
    xt = th.nhwc16(x, oh.pad8(c)).permute(0, 3, 1, 2).requires_grad_(need_dx)
    y = oh.conv2d(xt, conv, st, pad, dil)
    y.backward(th.nhwc16(dy).permute(0, 3, 1, 2))
    pkg.ops.join_side_stream()
    torch.cuda.synchronize()
    assert th.relerr(y.detach().float().cpu().numpy(), y_ref) < th.HCONV_TOL['fwd']
    if need_dx:
        got = xt.grad.float().cpu().numpy()
        assert np.isfinite(got).all() and not got[:, c:].any()
        assert th.relerr(got[:, :c], ref.conv2d_dgrad(dy, wt, x.shape, st, pad, dil)) < th.HCONV_TOL['dgrad']
    assert th.relerr(conv.weight.grad.cpu().numpy(), ref.conv2d_wgrad(dy, x, wt.shape, st, pad, dil)) < th.HCONV_TOL['wgrad']
    return y.detach(), xt.grad, conv.weight.grad


@pytest.mark.parametrize('case', th.HCONV_CASES, ids=[c[0] for c in th.HCONV_CASES])
def test_half_conv(pkg, fenced_scratch, case):
    fenced_then_plain(fenced_scratch, lambda: _hconv_op_case(pkg, case))


def _hbn_op_case(pkg, n, c, h, w, relu, with_res):
    """test_half_gpu.test_hbn_train_fwd_bwd's data through ops_half.batch_norm_act, at that test's bounds (th.HBN_TOL)"""
    oh = pkg.ops_half
    rng = np.random.default_rng(n * 1000 + c)
    x = th.r16(rng.standard_normal((n, c, h, w)) * 2 + 1)
    res = th.r16(rng.standard_normal((n, c, h, w))) if with_res else None
    gamma = (1 + 0.2 * rng.standard_normal(c)).astype(np.float32)
    beta = (0.3 * rng.standard_normal(c)).astype(np.float32)
    rm = rng.standard_normal(c).astype(np.float32)
    rv = (1 + rng.random(c)).astype(np.float32)
    y_ref, mean, invstd, nrm, nrv = ref.bn_train_fwd(x, gamma, beta, rm, rv)
    pre = y_ref + (res if with_res else 0)
    out_ref = np.maximum(pre, 0) if relu else pre
    xt = th.nhwc16(x).permute(0, 3, 1, 2).requires_grad_(True)
    rt = th.nhwc16(res).permute(0, 3, 1, 2).requires_grad_(True) if with_res else None
    gt, bt = (torch.from_numpy(a.copy()).cuda().requires_grad_(True) for a in (gamma, beta))
    rmt, rvt = (torch.from_numpy(a.copy()).cuda() for a in (rm, rv))
    y = oh.batch_norm_act(xt, gt, bt, rmt, rvt, rt, relu, True, 0.1, 1e-5)
    y_dev = y.detach().float().cpu().numpy()
    assert np.abs(y_dev - out_ref).max() < th.HBN_TOL['y'] * max(1.0, np.abs(out_ref).max())
    assert th.relerr(rmt.cpu().numpy(), nrm) < th.HBN_TOL['stats'] and th.relerr(rvt.cpu().numpy(), nrv) < th.HBN_TOL['stats']
    dy = th.r16(rng.standard_normal(x.shape))
    g = (dy * (y_dev > 0)).astype(np.float32) if relu else dy     # the mask of the kernel's own fp16 output, as in the test this is taken from
    dx_ref, dg_ref, db_ref = ref.bn_train_bwd(g, x, mean, invstd, gamma)
    y.backward(th.nhwc16(dy).permute(0, 3, 1, 2))
    torch.cuda.synchronize()
    assert np.abs(xt.grad.float().cpu().numpy() - dx_ref).max() < th.HBN_TOL['dx'] * max(1.0, np.abs(dx_ref).max())
    assert th.relerr(gt.grad.cpu().numpy(), dg_ref) < th.HBN_TOL['dparam'] and th.relerr(bt.grad.cpu().numpy(), db_ref) < th.HBN_TOL['dparam']
    if with_res:
        assert np.array_equal(rt.grad.float().cpu().numpy(), g)
    return y.detach(), xt.grad, gt.grad, bt.grad, rmt, rvt


def test_half_batchnorm(pkg, fenced_scratch):
    case, = [c for c in _params(th.test_hbn_train_fwd_bwd) if c[:4] == (3, 256, 9, 7)]
    fenced_then_plain(fenced_scratch, lambda: _hbn_op_case(pkg, *case))


def _two_smallest(cases):
    return sorted(cases, key=lambda c: (c[5] * c[6] * c[6], c[1]))[:2]


@needs_blocks
@pytest.mark.parametrize('case', _two_smallest(_params(th.test_half_block_executor_equals_the_per_layer_path)), ids=BLOCK_IDS)
def test_half_block_executor(pkg, fenced_scratch, case):
    kind, inplanes, planes, stride, dil, n, h, with_ds = case
    fenced_then_plain(fenced_scratch, lambda: th.half_block_case(pkg, kind, inplanes, planes, stride, dil, n, h, h, with_ds))


def _distill_case(pkg, mode):
    """p3d_distill_fwd_bwd at B 3, C 5, 7 x 9 = 63 pixels against Trainer.distill's expressions (depth_train.py:115-129) in float64, at td.DISTILL_TOL"""
    gen = torch.Generator(device='cuda').manual_seed(7)
    t, s0 = (torch.randn(3, 5, 7, 9, device='cuda', generator=gen) for _ in range(2))
    a = torch.rand(3, 1, 7, 9, device='cuda', generator=gen)
    s = s0.clone().requires_grad_(True)
    weighted, raw = pkg.ops.distill_loss(t, s, a, mode, weight=1.0)
    weighted.backward()
    sd, td64, ad = s0.double().requires_grad_(True), t.double(), a.double()
    if mode == 'bce':
        want = torch.nn.functional.binary_cross_entropy_with_logits(sd, torch.sigmoid(td64)) * ad.sum((1, 2, 3)).mean()
    else:
        diff = (torch.sigmoid(td64) - torch.sigmoid(sd)) if mode == 'sigmoid' else (td64 - sd)
        want = (diff * ad).reshape(3, -1).norm(dim=1).mean()
    want.backward()
    assert float(raw) == pytest.approx(float(want), rel=td.DISTILL_TOL)
    assert float((s.grad.double() - sd.grad).abs().max()) < td.DISTILL_TOL * max(float(sd.grad.abs().max()), 1e-12)
    return raw.detach(), s.grad


@pytest.mark.parametrize('mode', ['l2', 'sigmoid', 'bce'])
def test_distill(pkg, fenced_scratch, mode):
    assert mode in _params(td.test_distill_loss_matches_reference)
    fenced_then_plain(fenced_scratch, lambda: _distill_case(pkg, mode))


# ---- part 3, inference ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('slabs', [2, 3])
def test_folded_conv_split_k(pkg, fenced_scratch, slabs):
    """FoldedConv 2048 -> 272, 3x3 at 16 x 16, n = 2 with forced slab counts: the four epilogues of test_infer_gpu.test_conv_class_against_float64"""
    cls = (2048, 16, 272, 3, 1, 1)
    assert cls in tk.R50_CLASSES
    with _tune(pkg, 1, slabs):
        fenced_then_plain(fenced_scratch, lambda: ti.test_conv_class_against_float64(pkg, cls), [(ti, '_rel')])


@pytest.mark.parametrize('slabs', [2, 3])
def test_folded_conv_split_k_at_any_width(pkg, fenced_scratch, slabs):
    shape, = [s for s in _params(tia.test_split_k, arg='shape') if s[:2] == (2048, 272)]
    fenced_then_plain(fenced_scratch, lambda: tia.test_split_k(pkg, shape, slabs), [(tia, '_rel')])


def test_folded_masked_conv(pkg, fenced_scratch):
    cls = [c for c in tip.CLASSES if c[0] == 128 and c[2] == 128][-1]              # 128 -> 128 3x3 at 16 x 16, batch 2: the one that splits K in two
    fenced_then_plain(fenced_scratch, lambda: tip.test_partial_class_against_float64(pkg, cls), [(tip, '_rel'), (torch, 'equal')])


@pytest.mark.parametrize('case', _params(tk.test_conv_bn_eval_fused), ids=lambda c: 'n%d_c%d_h%d_k%d_%dx%d_s%d' % (c[0], c[1], c[2], c[4], c[5], c[5], c[6]))
def test_conv_bn_eval(pkg, fenced_scratch, case):
    fenced_then_plain(fenced_scratch, lambda: tk.test_conv_bn_eval_fused(case, pkg), [(tk, 'host')])


def test_folded_net(pkg, fenced_scratch):
    """infer.fold of the ResNet-18 depth network at 128^2, batch 2 (refresh() sizes the stem weight image's scratch by hand: covered here)"""
    fenced_then_plain(fenced_scratch, lambda: ti.whole_network_case(pkg, 'depthnet', 'resnet18', (), 128, 128), [(ti, '_rel')])


def test_folded_net_any_size(pkg, fenced_scratch):
    assert ('depthnet', 'resnet18', ()) in tia.NETS
    fenced_then_plain(fenced_scratch, lambda: tia.test_whole_network(pkg, 'depthnet', 'resnet18', (), (129, 129)), [(tia, '_rel')])


def test_folded_net_half(pkg, fenced_scratch):
    """fold_half: the fp16 forward takes no workspace; what is fenced is the unfolded fp16 model it is compared with (its BatchNorm passes)"""
    assert ('depthnet', 'resnet18', (), 128, 2) in tih.NETS
    fenced_then_plain(fenced_scratch, lambda: tih.whole_network_case(pkg, 'depthnet', 'resnet18', (), 128, 2), [(tih, '_err')])


def test_folded_net_fp8(pkg, fenced_scratch, monkeypatch):
    """fold_fp8 takes no workspace either: parity and the same bits"""
    assert ('depthnet', 'resnet18', (), 128, 2) in ti8.NETS

    def body():
        with monkeypatch.context() as m:
            ti8.layer_by_layer_case(pkg, m, 'depthnet', 'resnet18', (), 128, 2)
    fenced_then_plain(fenced_scratch, body, [(ti8, '_check'), (torch, 'equal')], scratch=False)


# ---- part 3, one eager training step each --------------------------------------------------------------------------------------------------------------
def test_training_step(pkg, fenced_scratch):
    """depth_r18_b2 against its golden at test_step_gpu's bounds; the model test_step_gpu.build made is compared afterwards: parameters, statistics, gradients"""
    assert 'depth_r18_b2' in ts.CASES
    fenced_then_plain(fenced_scratch, lambda: ts.test_train_step_matches_reference('depth_r18_b2', pkg), [(ts, 'build')])


def test_half_training_step(pkg, fenced_scratch):
    assert 'half_r18_b2' in _params(th.test_half_train_step_matches_reference_half)
    fenced_then_plain(fenced_scratch, lambda: th.test_half_train_step_matches_reference_half('half_r18_b2', pkg), [(ts, 'build')])


# ---- part 4: outputs inside fences ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def fenced_outputs():
    """Every tensor the test body or an op allocates with torch.empty & co. while the test runs lies in a fence of its own, two images wide, and comes poisoned
    (fenced.FencedAllocations): the outputs handed to the C ABI are exactly as large as the header says and not an allocator's rounding larger."""
    fa = FencedAllocations('cuda')
    fa.install()
    try:
        yield fa
    finally:
        fa.remove()
    torch.cuda.synchronize()
    fa.check()


def _fenced(pkg, fa, fs, body, expect):
    """An existing parity body, its assertions inside, on fenced outputs and fenced scratch.  expect: the outputs the case is about as (dtype, elements[, times]):
    so many tensors of exactly that type and size must have been handed out inside fences while the body ran -- a creator spelling FencedAllocations does not
    take, or a body that stops allocating the tensor that way, fails here and not silently"""
    before = len(fa.fences)
    body()
    fs.check()
    fa.check()
    made = [(dtype, int(np.prod(shape, dtype=np.int64))) for shape, dtype, _, _ in fa.fences[before:]]
    for dtype, numel, *times in expect:
        assert made.count((dtype, int(numel))) >= (times[0] if times else 1), ('no fenced %s tensor of %d elements' % (dtype, numel), sorted(set(made), key=str))


F32, F16, U8 = torch.float32, torch.float16, torch.uint8


def _acc_shapes():
    """'3x3s2' of CONV_CASES (an odd map) and the x3 case with K = 320 (no multiple of the 128-row tile) as (n, c, k, h, w, r, stride, pad, dil)"""
    _, n, c, h, w, k, ks, st, pad, dil, _ = _named(tk.CONV_CASES, ('3x3s2',))[0]
    n2, c2, k2, h2, r2, st2, dil2, _ = _rows(tk.X3_CASES, [(5, 192, 320, 8, 1, 1, 1)], width=7)[0]
    return [(n, c, k, h, w, ks, st, pad, dil), (n2, c2, k2, h2, h2, r2, st2, dil2 * (r2 - 1) // 2, dil2)]


ACC_SHAPES = _acc_shapes()


@pytest.mark.parametrize('x3', [False, True], ids=['fp32', 'x3'])
def test_outputs_conv(pkg, fenced_outputs, fenced_scratch, x3):
    """y, dx and dw of p3d_conv2d_fwd / dgrad / wgrad on both paths: overwritten (the ops' own torch.empty tensors) ..."""
    n, c, k, h, w, r, stride, pad, dil = ACC_SHAPES[0]
    ho, wo = pkg.ops.conv_out(h, r, stride, pad, dil), pkg.ops.conv_out(w, r, stride, pad, dil)
    with _x3(pkg, x3):
        _fenced(pkg, fenced_outputs, fenced_scratch, lambda: tk.test_conv_fwd_dgrad_wgrad(_named(tk.CONV_CASES, ('3x3s2',))[0], pkg),
                [(F32, n * k * ho * wo), (F32, n * c * h * w), (F32, k * c * r * r)])
    n, c, k, h, w, r, stride, pad, dil = ACC_SHAPES[1]
    if x3:                                                   # (x3_case runs both settings itself: two of each)
        _fenced(pkg, fenced_outputs, fenced_scratch, lambda: tk.x3_case(pkg, n, c, k, h, w, r, stride, pad, dil, False),
                [(F32, n * k * h * w, 2), (F32, n * c * h * w, 2), (F32, k * c * r * r, 2)])


@pytest.mark.parametrize('x3', [False, True], ids=['fp32', 'x3'])
@pytest.mark.parametrize('shape', ACC_SHAPES, ids=lambda s: 'n%d_c%d_k%d_%dx%d_%dx%d_s%d' % (s[0], s[1], s[2], s[3], s[4], s[5], s[5], s[6]))
def test_outputs_conv_accumulate(pkg, fenced_outputs, fenced_scratch, shape, x3):
    """... and accumulated onto (accumulate = 1), straight through the C ABI: the body of test_x3_accumulates_into_existing_gradients"""
    n, c, k, h, w, r = shape[:6]
    with _x3(pkg, x3):
        _fenced(pkg, fenced_outputs, fenced_scratch, lambda: tk.accumulate_case(pkg, *shape), [(F32, n * c * h * w), (F32, k * c * r * r)])


def test_outputs_activation_image(pkg, fenced_outputs, fenced_scratch):
    """p3d_fx_act_image modes 0, 1 and 2 into images of exactly p3d_fx_act_image_bytes"""
    assert pkg._lib.lib().p3d_fx_act_image_bytes(3, 48, 144) == 6 * 3 * 48 * 144
    _fenced(pkg, fenced_outputs, fenced_scratch, lambda: tk.act_image_split_case(pkg, 3, 48, 12, 12), [(U8, 6 * 3 * 48 * 144, 4)])


def test_outputs_weight_images_and_fold_kind0(pkg, fenced_outputs, fenced_scratch):
    """p3d_fx_weight_images at K 272, C 192, RS 9 (both images at p3d_fx_weight_image_bytes) and the kind-0 fold of p3d_fx_fold_bn_images, which must give the forward
    image bit for bit (test_infer_gpu.test_fold_images_bit_exact's comparison); the folded conv then runs on it at test_conv_class_against_float64's bound"""
    def body():
        conv, bn = ti._layer(pkg, 192, 272, 3, 1, 1, seed=5)
        fc = pkg.infer.FoldedConv(conv, bn)
        assert torch.equal(fc.image(fc.conv), ti._image_of(pkg, ti._torch_fold(conv, bn)))
        x = torch.randn(2, 192, 16, 16, device='cuda')
        assert ti._rel(fc(x, None, True), ti._conv64(x, conv, bn, None, True)) < 2e-5
    fb, bb = ctypes.c_size_t(), ctypes.c_size_t()
    pkg._lib.lib().p3d_fx_weight_image_bytes(272, 192, 9, ctypes.byref(fb), ctypes.byref(bb))
    _fenced(pkg, fenced_outputs, fenced_scratch, body, [(U8, fb.value), (U8, bb.value)])


def test_outputs_fold_kind2(pkg, fenced_outputs, fenced_scratch):
    """the kind-2 images of a network live side by side in ONE buffer (infer._Folded), which is what is fenced here, as a whole; the images of p3d_weight_images_f16
    they are compared with are fenced one by one ([K][R][S][Cpad] halves: the 64-channel 3x3, the padded stem)"""
    case = _params(tih.test_fold_images_bit_exact)[0]
    _fenced(pkg, fenced_outputs, fenced_scratch, lambda: tih.test_fold_images_bit_exact(pkg, case), [(F16, 64 * 9 * 64), (F16, 64 * 49 * 8)])


def test_outputs_fold_kind3(pkg, fenced_outputs, fenced_scratch):
    shape, = _params(ti8.test_fold_kind3_bit_exact, [(272, 512, 3)])
    k, c, r = shape
    assert pkg._lib.lib().p3d_f8conv2d_weight_bytes(k, c, r * r) == k * r * r * c + k * r * r * c // 32
    _fenced(pkg, fenced_outputs, fenced_scratch, lambda: ti8.test_fold_kind3_bit_exact(pkg, shape), [(U8, k * r * r * c + k * r * r * c // 32), (F32, k)])


@pytest.mark.parametrize('case', _params(tk.test_stem_on_the_x3_kernels, [(2, 3, 64, 64, 64), (3, 1, 48, 64, 64)]), ids=lambda c: 'n%d_c%d_%dx%d_k%d' % c)
def test_outputs_stem_images(pkg, fenced_outputs, fenced_scratch, case):
    """p3d_stem_image and p3d_stem_weight_image at their *_bytes sizes, y and dw of the stem"""
    n, cin, h, w, k = case
    L = pkg._lib.lib()
    _fenced(pkg, fenced_outputs, fenced_scratch, lambda: tk.test_stem_on_the_x3_kernels(case, pkg),
            [(U8, L.p3d_stem_image_bytes(n, h, w)), (U8, L.p3d_stem_weight_image_bytes(k)), (F32, n * k * (h // 2) * (w // 2)), (F32, k * cin * 49)])


@pytest.mark.parametrize('case', BN_SHAPES[:2], ids=lambda c: 'n%d_c%d_%dx%d' % c[:4])
def test_outputs_batchnorm(pkg, fenced_outputs, fenced_scratch, case):
    """y, save_mean, save_invstd (and dx, dgamma, dbeta) of p3d_bn_train_fwd / bwd"""
    n, c, h, w = case[:4]
    _fenced(pkg, fenced_outputs, fenced_scratch, lambda: tk.test_bn_train_fwd_bwd(*case, pkg), [(F32, n * c * h * w, 2), (F32, c, 4)])


@pytest.mark.parametrize('shape', _params(tk.test_maxpool_fwd_bwd_with_ties, [(1, 3, 17, 15), (2, 3, 10, 12)]), ids=lambda s: 'n%d_c%d_%dx%d' % s)
def test_outputs_maxpool(pkg, fenced_outputs, fenced_scratch, shape):
    n, c, h, w = shape
    pooled = n * c * ((h - 1) // 2 + 1) * ((w - 1) // 2 + 1)
    _fenced(pkg, fenced_outputs, fenced_scratch, lambda: tk.test_maxpool_fwd_bwd_with_ties(shape, pkg), [(F32, pooled), (U8, pooled), (F32, n * c * h * w)])


@pytest.mark.parametrize('case', _named(th.HCONV_CASES, ('3x3s2', '3x3d2', 'stem1')), ids=lambda c: c[0])
def test_outputs_half_conv(pkg, fenced_outputs, fenced_scratch, case):
    """the NHWC fp16 y and dx, the two fp16 weight images and the weight-gradient workspace of the C-level fp16 test (its own torch.empty / torch.full tensors; its
    fp32 dw is a copy of host data and not fenced here: test_half_conv has the op's own)"""
    name, n, c, h, w, k, ks, st, pad, dil = case
    cpad = (c + 7) // 8 * 8
    d = pkg.ops._desc((n, cpad, h, w), (k, cpad, ks, ks), st, pad, dil)
    need = max(pkg._lib.lib().p3d_hconv2d_wgrad_workspace_bytes(ctypes.byref(d)), 16)
    _fenced(pkg, fenced_outputs, fenced_scratch, lambda: th.test_hconv_fwd_dgrad_wgrad(case, pkg),
            [(F16, n * d.Ho * d.Wo * k), (F16, n * h * w * cpad), (F16, k * ks * ks * cpad, 2), (U8, need)])


@pytest.mark.parametrize('case', _named(th.SUM_CASES, ('ragged', '3x3d2')), ids=lambda c: c[0])
def test_outputs_half_conv_partial_sums(pkg, fenced_outputs, fenced_scratch, case):
    """`partial` of p3d_hconv2d_fwd_stats / p3d_hconv2d_dgrad_sums at p3d_hconv2d_sum_rows rows"""
    name, n, c, h, w, k, ks, st, pad, dil = case
    d = pkg.ops._desc((n, c, h, w), (k, c, ks, ks), st, pad, dil)
    L = pkg._lib.lib()
    rows = [L.p3d_hconv2d_sum_rows(ctypes.byref(d), p) for p in (0, 1)]
    _fenced(pkg, fenced_outputs, fenced_scratch, lambda: th.test_hconv_epilogue_sums(case, pkg), [(F32, rows[0] * (k // 8) * 16), (F32, rows[1] * (c // 8) * 16)])


def test_outputs_half_relu_mask(pkg, fenced_outputs, fenced_scratch):
    """relu_mask of p3d_hbn_train_fwd_partial: P * C / 8 bytes"""
    case, = _params(th.test_hbn_relu_mask_bytes, [(3, 32, 64, 9)])
    n, c, k, h = case
    _fenced(pkg, fenced_outputs, fenced_scratch, lambda: th.test_hbn_relu_mask_bytes(*case, pkg), [(U8, n * h * h * k // 8), (F16, n * h * h * k, 2)])


@needs_blocks
@pytest.mark.parametrize('case', _smallest_per_geometry(tb.CASES)[:3], ids=BLOCK_IDS)
def test_outputs_block(pkg, fenced_outputs, fenced_scratch, case):
    """what ops_block hands p3d_block_fwd / bwd, all of it torch.empty of the documented size: c, the activation and gradient images, the tables, out_mask
    (N K Ho Wo / 4 bytes), gbuf, dx and the parameter gradients"""
    kind, inplanes, planes, stride, dil, n, h, with_ds = case
    out = n * planes * (4 if kind == 'bottleneck' else 1) * (h // stride) ** 2
    _fenced(pkg, fenced_outputs, fenced_scratch, lambda: tb.fused_block_case(pkg, *case), [(U8, out // 4), (F32, out), (F32, n * inplanes * h * h)])


# ---- part 5: the size contract ---------------------------------------------------------------------------------------------------------------------------
EWORKSPACE = -2


def _bn_args(c):
    return [torch.ones(c, device='cuda', requires_grad=True), torch.zeros(c, device='cuda', requires_grad=True), torch.zeros(c, device='cuda'), torch.ones(c, device='cuda')]


def _short_bn_fwd(pkg):
    x = torch.randn(3, 10, 17, 17, device='cuda')
    return lambda: pkg.ops.batch_norm_act(x, *_bn_args(10), None, True, True, 0.1, 1e-5)


def _short_bn_bwd(pkg):
    x = torch.randn(3, 10, 17, 17, device='cuda', requires_grad=True)
    y = pkg.ops.batch_norm_act(x, *_bn_args(10), None, True, True, 0.1, 1e-5)
    return lambda: y.backward(torch.ones_like(y))


def _stem_tail(pkg, shape):
    bn = pkg.nn.BatchNorm2d(shape[1]).cuda().train()
    x = torch.randn(*shape, device='cuda', requires_grad=True)
    assert pkg.ops.stem_tail_usable(x, bn, pkg.nn.MaxPool2d(kernel_size=3, stride=2, padding=1))
    return x, bn


def _short_stem_tail_fwd(pkg):
    x, bn = _stem_tail(pkg, (3, 16, 32, 20))
    return lambda: pkg.ops.stem_tail(x, bn)


def _short_stem_tail_bwd(pkg):
    x, bn = _stem_tail(pkg, (3, 16, 32, 20))
    y = pkg.ops.stem_tail(x, bn)
    return lambda: y.backward(torch.ones_like(y))


def _conv_bwd(pkg, shape, which, x3):
    """forward of ops.conv2d on whole scratch; the returned call runs only the data gradient or only the weight gradient"""
    n, c, k, h, w, r, stride, pad, dil = shape
    pkg.ops.set_x3(x3)
    x = torch.randn(n, c, h, w, device='cuda', requires_grad=which == 'dgrad')
    wt = (torch.randn(k, c, r, r, device='cuda') / (c * r * r) ** 0.5).requires_grad_(which == 'wgrad')
    y = pkg.ops.conv2d(x, wt, None, stride, pad, dil)

    def call():
        # (the query reports the largest of the plans a shape can take, so that one query serves them all; with the split count of the x3 weight gradient forced up,
        # under the query and the launch alike, that plan is the largest)
        with (_tune(pkg, 0, 20) if (x3 and which == 'wgrad') else contextlib.nullcontext()):
            y.backward(torch.ones_like(y))
    return call


STRIDED_X3 = (6, 256, 256, 32, 32, 3, 2, 1, 1)


def _short_bn_eval(pkg):
    """(behind the scale / shift table at its head this workspace is p3d_conv2d_fwd's, which is optional: on the fp32-MFMA kernels this shape takes none, so the
    table is all the query asks for)"""
    pkg.ops.set_x3(False)
    conv = pkg.nn.Conv2d(32, 64, 3, padding=1, bias=False).cuda()
    bn = pkg.nn.BatchNorm2d(64).cuda().eval()
    x = torch.randn(2, 32, 20, 20, device='cuda')

    def call():
        with torch.no_grad():
            pkg.ops.conv_bn_eval(x, conv, bn, relu=True)
    return call


def _short_img(pkg, pass_):
    n, c, h, k, ks, st, dil = IMG_SHAPES[0]
    x = torch.randn(n, c, h, h, device='cuda')
    wt = torch.randn(k, c, ks, ks, device='cuda')
    pad = dil * (ks - 1) // 2
    x_img = pkg.ops.act_image(x)
    dy_img = pkg.ops.act_image(torch.randn(n, k, (h - 1) // st + 1, (h - 1) // st + 1, device='cuda'))
    return lambda: pkg.ops.conv2d_img(pass_, x.shape, wt, st, pad, dil, x_img=x_img, dy_img=dy_img)


def _short_infer(pkg):
    conv, bn = ti._layer(pkg, 128, 128, 3, 1, 1, seed=3)
    fc = pkg.infer.FoldedConv(conv, bn)
    x = torch.randn(2, 128, 16, 16, device='cuda')
    return lambda: fc(x, None, True)


def _short_stem_wgrad(pkg):
    conv = pkg.nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False).cuda()
    x = torch.randn(2, 3, 64, 64, device='cuda')
    assert pkg.ops_block.stem_takes_x3(conv, x)
    y = conv(x)
    return lambda: y.backward(torch.ones_like(y))


def _block(pkg, bwd):
    block = tb.build(pkg, 'bottleneck', 512, 128, 1, 1, False, seed=3)
    x = torch.randn(4, 512, 16, 16, device='cuda').relu_().requires_grad_(True)
    assert pkg.ops_block.usable(block, x) and pkg._trunk.FUSED_BLOCKS
    y = block(x)                                             # (also the forward of a first call: plan, weight images)
    assert type(y.grad_fn).__name__.startswith('ResidualBlockFn')
    return (lambda: y.backward(torch.ones_like(y))) if bwd else (lambda: block(x))


def _hblock(pkg, bwd):
    oh = pkg.ops_half
    block = tb.build(pkg, 'basic', 64, 64, 1, 1, False, seed=5)
    oh.refresh_weights(block)
    x = torch.randn(4, 64, 32, 32, device='cuda').relu_().half().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    assert oh.HALF_BLOCKS and oh.block_usable(block, x)
    y = block(x)
    assert 'HResidualBlockFn' in type(y.grad_fn).__name__
    return (lambda: y.backward(torch.ones_like(y))) if bwd else (lambda: block(x))


def _short_hconv_wgrad(pkg):
    oh = pkg.ops_half
    conv = pkg.nn.Conv2d(32, 64, 3, padding=1, bias=False).cuda()
    oh.refresh_weights(conv)
    x = torch.randn(2, 32, 20, 20, device='cuda').half().contiguous(memory_format=torch.channels_last)
    y = oh.conv2d(x, conv, 1, 1, 1)
    return lambda: y.backward(torch.ones_like(y))


def _short_hbn(pkg):
    x = torch.randn(3, 256, 9, 7, device='cuda').half().contiguous(memory_format=torch.channels_last)
    return lambda: pkg.ops_half.batch_norm_act(x, *_bn_args(256), None, True, True, 0.1, 1e-5)


def _short_distill(pkg):
    t, s = torch.randn(3, 5, 7, 9, device='cuda'), torch.randn(3, 5, 7, 9, device='cuda', requires_grad=True)
    a = torch.rand(3, 1, 7, 9, device='cuda')
    return lambda: pkg.ops.distill_loss(t, s, a, 'l2', weight=1.0)


# name: (the entry that must refuse, how to get to the call).  A query reports the largest workspace of the
# plans a shape can take; the x3 strided data gradient needs less than the parity-class staging of the fp32-MFMA kernels that the query covers, so 256 bytes
# less than the query are not short for it (it runs, exactly sized, in part 3) and the strided data gradient is refused on the fp32-MFMA path only.
SHORT = {
    'bn_train_fwd': ('p3d_bn_train_fwd', _short_bn_fwd),
    'bn_train_bwd': ('p3d_bn_train_bwd', _short_bn_bwd),
    'stem_tail_fwd': ('p3d_stem_tail_fwd', _short_stem_tail_fwd),
    'stem_tail_bwd': ('p3d_stem_tail_bwd', _short_stem_tail_bwd),
    'conv2d_dgrad_strided_fp32': ('p3d_conv2d_dgrad', lambda pkg: _conv_bwd(pkg, ACC_SHAPES[0], 'dgrad', False)),
    'conv2d_wgrad_fp32': ('p3d_conv2d_wgrad', lambda pkg: _conv_bwd(pkg, ACC_SHAPES[0], 'wgrad', False)),
    'conv2d_wgrad_x3': ('p3d_conv2d_wgrad', lambda pkg: _conv_bwd(pkg, STRIDED_X3, 'wgrad', True)),
    'conv2d_bn_eval_fwd': ('p3d_conv2d_bn_eval_fwd', _short_bn_eval),
    'fx_conv_fwd_img': ('p3d_fx_conv_fwd_img', lambda pkg: _short_img(pkg, 'fwd')),
    'fx_conv_dgrad_img': ('p3d_fx_conv_dgrad_img', lambda pkg: _short_img(pkg, 'dgrad')),
    'fx_conv_wgrad_img': ('p3d_fx_conv_wgrad_img', lambda pkg: _short_img(pkg, 'wgrad')),
    'fx_conv_fwd_infer': ('p3d_fx_conv_fwd_infer', _short_infer),
    'stem_wgrad': ('p3d_stem_wgrad', _short_stem_wgrad),
    'block_fwd': ('p3d_block_fwd', lambda pkg: _block(pkg, False)),
    'block_bwd': ('p3d_block_bwd', lambda pkg: _block(pkg, True)),
    'hblock_fwd': ('p3d_hblock_fwd', lambda pkg: _hblock(pkg, False)),
    'hblock_bwd': ('p3d_hblock_bwd', lambda pkg: _hblock(pkg, True)),
    'hconv2d_wgrad': ('p3d_hconv2d_wgrad', _short_hconv_wgrad),
    'hbn_train_fwd': ('p3d_hbn_train_fwd', _short_hbn),
    'distill': ('p3d_distill_fwd_bwd', _short_distill),
}


@pytest.mark.parametrize('name', list(SHORT))
def test_short_workspace_is_refused(pkg, fenced_outputs, fenced_scratch, name):
    """Everything up to the call runs on whole scratch; the call itself gets a workspace 256 bytes short of what the query reported (one float short where the query is no larger; its ops pass .numel() on):
    P3D_EWORKSPACE from the entry -- raised by _lib.check, which names it -- with the library's own text, nothing launched: every tensor the op had allocated for
    its results still holds its poison, and every fence is intact."""
    entry, prepare = SHORT[name]
    before = pkg.ops.set_x3(True)
    try:
        call = prepare(pkg)
        torch.cuda.synchronize()
        asked, mark = len(fenced_scratch.fences), len(fenced_outputs.fences)
        with fenced_scratch.short_by(256), pytest.raises(RuntimeError) as err:
            call()
    finally:
        pkg.ops.set_x3(before)
        pkg.ops.join_side_stream()
    assert len(fenced_scratch.fences) > asked and fenced_scratch.fences[asked][1] > 0, 'the call asked for no scratch'
    message = str(err.value)
    assert message.startswith('%s failed (%d): ' % (entry, EWORKSPACE)), message
    # p3d_last_error()'s text, as _lib.check read it on the thread that made the call (autograd's, in a backward pass), begins with the entry's own name
    assert message.split(': ', 1)[1].startswith(entry[len('p3d_'):] + ': '), message
    torch.cuda.synchronize()
    handed = [f for f in fenced_outputs.fences[mark:] if f[2]]
    assert handed, 'the op had allocated no result when it was refused: the poison check below would be empty'
    assert fenced_outputs.untouched_since(mark)
    fenced_scratch.check()
    fenced_outputs.check()


@pytest.mark.parametrize('x3', [False, True], ids=['fp32', 'x3'])
@pytest.mark.parametrize('which', ['fwd', 'dgrad'])
def test_optional_workspace_may_be_missing(pkg, fenced_outputs, x3, which):
    """p3d_conv2d_fwd and the stride-1 p3d_conv2d_dgrad on the split-K shape ('big': the query asks for slabs) with workspace NULL / 0: the documented unsplit
    launch -- success, one launch on the counters, the result at the bound of test_conv_fwd_dgrad_wgrad / test_x3_kernels_match_fp32_kernels"""
    ops, L = pkg.ops, pkg._lib.lib()
    name, n, c, h, w, k, ks, st, pad, dil, _ = _named(tk.CONV_CASES, ('big',))[0]
    gen = torch.Generator(device='cuda').manual_seed(1)
    x = torch.randn(n, c, h, w, device='cuda', generator=gen)
    wt = torch.randn(k, c, ks, ks, device='cuda', generator=gen) / (c * ks * ks) ** 0.5
    d = ops._desc(x.shape, wt.shape, st, pad, dil)
    dy = torch.randn(n, k, d.Ho, d.Wo, device='cuda', generator=gen)
    with _x3(pkg, x3):
        ops.conv_path_stats(reset=True)
        if which == 'fwd':
            assert L.p3d_conv2d_fwd_workspace_bytes(ctypes.byref(d)) > 0
            got = torch.empty(n, k, d.Ho, d.Wo, device='cuda')
            rc = L.p3d_conv2d_fwd(ctypes.byref(d), ops._p(x), ops._p(wt), None, None, None, ops._p(got), None, 0, ops._stream())
            want = torch.nn.functional.conv2d(x.double(), wt.double(), None, st, pad, dil)
        else:
            assert L.p3d_conv2d_dgrad_workspace_bytes(ctypes.byref(d)) > 0
            got = torch.empty_like(x)
            rc = L.p3d_conv2d_dgrad(ctypes.byref(d), ops._p(dy), ops._p(wt), None, None, ops._p(got), None, 0, ops._stream())
            want = torch.nn.grad.conv2d_input(x.shape, wt.double(), dy.double(), st, pad, dil)
        torch.cuda.synchronize()
        stats = ops.conv_path_stats(reset=True)
    assert rc == 0, L.p3d_last_error()
    assert sum(stats[path][which][0] for path in ('x3', 'fp32')) == 1, stats      # (the x3 kernels build their weight image in the workspace: without one the fp32-MFMA kernel runs)
    err = ((got.double() - want).abs().max() / want.abs().max()).item()
    assert err < (tk.X3_TOL if stats['x3'][which][0] else tk.CONV_TOL[which]), err
    fenced_outputs.check()
