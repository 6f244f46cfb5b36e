"""torch.autograd.Function wrappers over the C ABI (include/p3d_hip.h).

Each Function replaces the torch operator the reference calls at the cited line; arithmetic
happens only in the hand-written HIP kernels.  Tensors must be fp32 on a HIP device -- there is
no CPU or eager-PyTorch fallback: anything else raises P3DError.
"""
import ctypes
import os

import torch

from ._lib import CONSTANTS, ConvDesc, P3DError, check, lib

CRITERIA = {'SmoothL1': 0, 'L1': 1, 'MSE': 2}


def _need_gpu(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise P3DError('p3d ops run only on a HIP device (got a %s tensor); there is no CPU fallback' % t.device)
        if t.dtype != torch.float32:
            raise P3DError('p3d ops are fp32 only (got %s)' % t.dtype)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    """Raw handle of the current HIP stream of the current device (the C fast path: this runs once per kernel launch)."""
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


# When a list, every conv launch is bracketed by a pair of events on the launch stream and
# (kind, algorithmic_flops, start, end) is appended: bench.py's live per-kernel timing.
PROFILE = None


class _Timed:
    def __init__(self, kind, d, stream=None):
        """stream: where the launch goes when that is not the current stream (the weight-gradient stream of _side_launch)."""
        self.kind, self.stream = kind, stream
        self.flops = 2.0 * d.N * d.K * d.Ho * d.Wo * d.C * d.R * d.S

    def __enter__(self):
        if PROFILE is not None:
            self.start = torch.cuda.Event(enable_timing=True)
            self.end = torch.cuda.Event(enable_timing=True)
            self.start.record(self.stream)
        return self

    def __exit__(self, *exc):
        if PROFILE is not None:
            self.end.record(self.stream)
            PROFILE.append((self.kind, self.flops, self.start, self.end))
        return False


# Weight-gradient kernels leave the critical path of backward (dy -> BN backward -> dgrad -> next layer): they only feed the
# optimizer.  With P3D_WGRAD_STREAM != 0 they are launched on a second HIP stream, so the matrix-core-bound wgrad of layer i
# overlaps the HBM-bound BN backward and the grid tails of layer i-1's kernels instead of queueing behind them (_side_launch).
# join_side_stream() orders the launch stream after everything issued there (before an all-reduce / the optimizer reads .grad).
WGRAD_STREAM = os.environ.get('P3D_WGRAD_STREAM', '1') != '0'
_side_streams = {}
_scratch = {}                                                          # (device, role) -> grow-only byte buffer


def _scratch_buffer(device, nbytes, role):
    """Grow-only scratch per device and role; ops on one stream are ordered, so they share it.  Roles: 'launch' (workspace()), 'second' (also on the launch stream:
    the block executors' weight-gradient slabs when no second stream is used, beside the 'launch' scratch of the same call) and 'side', the weight-gradient
    stream's, allocated with that stream current so that the allocator knows it as the owner."""
    ws = _scratch.get((device, role))
    if ws is None or ws.numel() < nbytes:
        with torch.cuda.stream(_side_stream(device) if role == 'side' else None):
            ws = _scratch[(device, role)] = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
    return ws


def workspace(device, nbytes):
    return _scratch_buffer(device, nbytes, 'launch')


SIDE_STREAM_OVERLAPS = {}                                              # device -> what the probe found


def cu_mask_words(spec, total=256):
    """'N' -> the first N of `total` compute units, 'N:hi' -> the last N, '0x...' -> the mask itself, as little-endian 32-bit words.  (KFD deals the bits of a
    queue's mask round-robin over the eight XCDs: a contiguous run of N bits is N / 8 CUs on each.)"""
    spec = str(spec)
    if spec.lower().startswith('0x'):
        value = int(spec, 16)
    else:
        n, _, where = spec.partition(':')
        n = max(1, min(int(n), total))
        value = ((1 << n) - 1) << (total - n if where == 'hi' else 0)
    return [(value >> (32 * i)) & 0xFFFFFFFF for i in range(total // 32)]


def masked_stream(device, spec):
    """A HIP stream whose kernels run only on the compute units `spec` names (cu_mask_words), as a torch ExternalStream."""
    words = cu_mask_words(spec)
    arr = (ctypes.c_uint32 * len(words))(*words)
    handle = ctypes.c_void_p()
    with torch.cuda.device(device):
        check(lib().p3d_stream_create_cumask(arr, len(words), ctypes.byref(handle)), 'stream_create_cumask')
    return torch.cuda.ExternalStream(handle.value, device=device)


def _side_stream(device):
    """The weight-gradient stream.  HIP multiplexes the streams of one priority onto four hardware queues: a stream taken from PyTorch's pool landed on
    the launch stream's own queue whenever an RCCL communicator had been created first (rocprofv3: every kernel of the step on one queue), which costs
    the overlap plus a queue barrier per cross-stream event, +2.3 ms per step.  So the stream is chosen by measurement:
    p3d_stream_create_beside creates candidates until two spin kernels, one per stream, demonstrably run side by side."""
    st = _side_streams.get(device)
    if st is None:
        handle, found = ctypes.c_void_p(), ctypes.c_int32(0)
        with torch.cuda.device(device):
            check(lib().p3d_stream_create_beside(ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream), ctypes.byref(handle), ctypes.byref(found)), 'stream_create_beside')
        st = torch.cuda.ExternalStream(handle.value, device=device)
        SIDE_STREAM_OVERLAPS[device] = bool(found.value)
        _side_streams[device] = st
    return st


_join_queued = False
_event_ring, _event_next = [], [0]


def _mark_ready():
    """Record 'everything launched so far on the current stream' into a recycled event (creating an event per call costs ~20 us of host
    time; a recorded event may be re-recorded once the wait on it has been enqueued, which happens right after in the same call)."""
    if len(_event_ring) < 64:
        _event_ring.append(torch.cuda.Event())
    ev = _event_ring[_event_next[0] % len(_event_ring)]
    _event_next[0] += 1
    ev.record()
    return ev


def join_side_stream(device=None):
    global _join_queued
    _join_queued = False
    for dev, st in _side_streams.items():
        if device is None or dev == device:
            torch.cuda.current_stream(dev).wait_stream(st)


def _queue_join():
    """First side-stream launch of a backward pass: have the autograd engine join the streams when the pass ends, so whoever
    called .backward() sees complete gradients on the launch stream (like any other autograd result)."""
    global _join_queued
    if not _join_queued:
        _join_queued = True
        torch.autograd.Variable._execution_engine.queue_callback(join_side_stream)


def _side_launch(device, wanted, nbytes, ready=None, block=False):
    """Where a weight-gradient launch goes and what it may scribble on: (side, stream handle, scratch).  The ONE place that orders the two streams of backward.
    wanted: the caller's own conditions; the launch leaves the launch stream only if WGRAD_STREAM (read now: bench.py assigns it between passes) holds too.
    Callers pass `grads.direct and ...`: a gradient handed back to autograd is consumed on the launch stream, so only sink-bound ones may go aside.
    On the second stream: the backward pass is told to join the streams when it ends, the stream is ordered behind `ready` (an event of _mark_ready()
    recorded where the operands became final; None: the launch stream as of now) and the scratch is the second stream's own.  block=True is the call of a
    block executor, which takes the second stream beside the launch stream and orders its launches there itself: no wait here, and handle None plus the second
    launch-stream scratch (its call uses workspace() too) when everything stays on the launch stream.
    Nothing here creates an event, allocates or synchronizes in steady state (a captured step runs through it).  side is None on the launch stream; hand it to
    _Timed and, after the launch, to _side_launched."""
    if not (WGRAD_STREAM and wanted):
        return None, (None if block else _stream()), _scratch_buffer(device, nbytes, 'second' if block else 'launch')
    side = _side_stream(device)
    _queue_join()
    if not block:
        side.wait_event(_mark_ready() if ready is None else ready)
    return side, ctypes.c_void_p(side.cuda_stream), _scratch_buffer(device, nbytes, 'side')


def _side_launched(side, tensors=(), owned=None):
    """After a launch placed by _side_launch: what the second stream still reads must outlive / stay untouched until it is done.  tensors: the allocator-owned
    operands (autograd frees them while the kernel may be pending; None entries are skipped); owned: the module- or plan-owned buffer set among the operands,
    whose next user orders itself behind the event recorded here (ops_block._free_set).  Call _GradOut.done() only after this."""
    if side is not None:
        for t in tensors:
            if t is not None:
                t.record_stream(side)
        if owned is not None:
            owned.mark_side(side)


def _grad_sink(param):
    """The preallocated .grad of a parameter owned by FlatAdam (flagged _p3d_direct_grad), or None."""
    if param is not None and getattr(param, '_p3d_direct_grad', False) and param.grad is not None:
        return param.grad
    return None


def _grad_done(param):
    ready = getattr(param, '_p3d_grad_ready', None)       # set by dist.GradReducer: counts the bucket down
    if ready is not None:
        ready()


class _GradOut:
    """Where a backward writes the gradients of `params` (fp32 parameters, one for the per-parameter rule, several for all-or-nothing: the gamma / beta of a
    BatchNorm, every parameter of a block) and what it returns to autograd for them.  If EVERY parameter has a FlatAdam sink (_grad_sink), `bufs` are those
    and `direct` is set: the kernels accumulate straight into them (the buffer is zeroed once per step), so autograd's own per-parameter add kernel and its
    temporary are skipped and done() returns None for each.  Otherwise `bufs` are fresh tensors, overwritten and returned.
    done() also reports completion (under a process group dist.GradReducer may then queue an all-reduce on the second stream): call it LAST, after the launch
    and after _side_launched, so that a buffer set's next user waits for the weight gradients and not for the collective behind them."""
    __slots__ = ('params', 'direct', 'bufs')

    def __init__(self, *params):
        sinks = [_grad_sink(p) for p in params]
        self.params = params
        self.direct = all(s is not None for s in sinks)
        self.bufs = sinks if self.direct else [torch.empty(p.shape, dtype=torch.float32, device=p.device) for p in params]

    def done(self):
        if not self.direct:
            return tuple(self.bufs)
        for p in self.params:
            _grad_done(p)
        return (None,) * len(self.params)


def conv_out(h, k, stride, pad, dil):
    return (h + 2 * pad - dil * (k - 1) - 1) // stride + 1


def _desc(x_shape, w_shape, stride, pad, dil, c_offset=0, c_total=None, accumulate=0):
    n, c, h, w = x_shape
    k, cw, r, s = w_shape
    d = ConvDesc()
    d.N, d.C, d.H, d.W = n, c, h, w
    d.K, d.R, d.S = k, r, s
    d.stride, d.pad, d.dil = stride, pad, dil
    d.Ho, d.Wo = conv_out(h, r, stride, pad, dil), conv_out(w, s, stride, pad, dil)
    d.c_total = cw if c_total is None else c_total
    d.c_offset = c_offset
    d.accumulate = accumulate
    return d


# --------------------------------------------------------------------------------------------
class GradJoin:
    """Where a tensor fans out inside a residual block (block input -> first conv + shortcut), autograd would sum the two
    gradients with an extra elementwise pass (read 2, write 1 over the block input).  A GradJoin hands the gradient that is
    produced FIRST (the shortcut's: residual gradient of the closing BN, or the dgrad of the downsample conv) to the op that runs
    LAST (the first conv of the main path, created first in forward, hence last in backward), whose dgrad kernel then accumulates
    into that buffer (`accumulate = 1`).  The producer returns None to autograd, the consumer returns the joined buffer.
    Order independence: the consumer marks the join `taken` when its backward runs; a consumer that finds the slot empty behaves
    normally, and a producer that runs AFTER the consumer (or whose consumer needs no input gradient) sees `taken` and returns its
    gradient to autograd like any other Function, so the shortcut gradient is never dropped.  A gradient that was stashed but never
    picked up (the consumer's backward did not run at all) is an error: the first stash of a pass queues an engine callback that
    raises P3DError when the pass ends (`check_joins`), whoever called .backward().
    `after`: an event the producer may leave beside `buf` when a kernel on the second stream still reads the stashed buffer (ops_frozen.FrozenConvBnFn, whose
    stashed gradient is also its weight gradient's operand); the consumer orders its stream behind it before it writes (`_take`).  Only the fp32 consumers
    (Conv2dFn, FrozenConvBnFn) and HFrozenConvBnFn go through `_take`; ops_half.HConv2dFn reads `buf` itself and waits for `after` the same way (only
    HFrozenConvBnFn, under ops.frozen_fold_half, ever leaves one for it)."""
    __slots__ = ('buf', 'taken', 'after', '__weakref__')
    _live = None

    def __init__(self):
        self.buf = None
        self.taken = False
        self.after = None             # an event the consumer's stream waits for before it writes `buf` (a reader of the stashed buffer on the second stream)
        if GradJoin._live is None:
            import weakref
            GradJoin._live = weakref.WeakSet()
        GradJoin._live.add(self)


def pending_joins():
    return 0 if GradJoin._live is None else sum(1 for j in GradJoin._live if j.buf is not None)


_join_check_queued = False


def check_joins():
    """Raise if a shortcut gradient was stashed in a GradJoin and never consumed (it would silently be missing from the input gradient)."""
    global _join_check_queued
    _join_check_queued = False
    n = pending_joins()
    if n:
        for j in GradJoin._live:
            j.buf = j.after = None
        raise P3DError('%d shortcut gradient(s) were produced but never joined (ops.GradJoin): the backward pass did not reach the first '
                       'convolution of a residual block' % n)


def _stash(join, grad, after=None):
    """Producer side of a GradJoin: True if `grad` was handed to the join (return None to autograd), False if the consumer has already run.
    after: an event behind the producer's own readers of `grad` on the second stream (ops_frozen: the stashed gradient is also its weight gradient's operand);
    the consumer accumulates into the buffer only behind it (_take)."""
    global _join_check_queued
    if join is None or join.taken:
        return False
    join.buf = grad
    join.after = after
    if not _join_check_queued:
        _join_check_queued = True
        torch.autograd.Variable._execution_engine.queue_callback(check_joins)
    return True


def _take(join, x):
    """Consumer side of a GradJoin whose slot is filled: the stashed gradient, checked against the block input x it is a gradient of, with the slot emptied and
    the launch stream ordered behind the producer's `after` event when it left one."""
    joined = join.buf
    if joined.shape != x.shape or joined.dtype != x.dtype:
        raise P3DError('GradJoin: the shortcut gradient %s does not match the block input %s' % (tuple(joined.shape), tuple(x.shape)))
    if join.after is not None:
        torch.cuda.current_stream(x.device).wait_event(join.after)
    join.buf = join.after = None
    return joined


class Conv2dFn(torch.autograd.Function):
    """nn.Conv2d (depthnet.py:16-33,65-89,138,156) and, with mask_in/mult, PartialConv's masked,
    renormalised convolution (partial_conv.py:45-53).  join_put / join_take: see GradJoin."""

    @staticmethod
    def forward(ctx, x, w, bias, mask_in, mult, stride, pad, dil, join_put=None, join_take=None):
        _need_gpu(x, w, bias, mask_in, mult)
        x, w = x.contiguous(), w.contiguous()
        d = _desc(x.shape, w.shape, stride, pad, dil)
        if x.shape[1] != w.shape[1]:
            raise P3DError('conv2d: input has %d channels, weight expects %d' % (x.shape[1], w.shape[1]))
        y = torch.empty((d.N, d.K, d.Ho, d.Wo), dtype=torch.float32, device=x.device)
        L = lib()
        nbytes = L.p3d_conv2d_fwd_workspace_bytes(ctypes.byref(d))
        ws = workspace(x.device, nbytes) if nbytes else None
        with _Timed('fwd', d):
            check(L.p3d_conv2d_fwd(ctypes.byref(d), _p(x), _p(w), _p(bias), _p(mask_in), _p(mult), _p(y), _p(ws), ws.numel() if ws is not None else 0,
                                   _stream()), 'p3d_conv2d_fwd')
        ctx.save_for_backward(x, w, mask_in, mult)
        ctx.cfg = (stride, pad, dil, bias is not None)
        ctx.params = (w, bias)
        ctx.joins = (join_put, join_take)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, mask_in, mult = ctx.saved_tensors
        stride, pad, dil, has_bias = ctx.cfg
        join_put, join_take = ctx.joins
        dy = dy.contiguous()
        d = _desc(x.shape, w.shape, stride, pad, dil)
        L = lib()
        st = _stream()
        dx = dw = db = None
        # dy is complete at this point of the launch stream: the wgrad stream waits for THIS event, not for the dgrad launched below
        dy_ready = _mark_ready() if (WGRAD_STREAM and ctx.needs_input_grad[1]) else None
        if join_take is not None:
            join_take.taken = True                            # producers that run later return their gradient to autograd themselves
        if ctx.needs_input_grad[0]:
            if join_take is not None and join_take.buf is not None:
                dx = _take(join_take, x)                      # accumulate onto the shortcut's gradient: no separate add pass
                d.accumulate = 1
            else:
                dx = torch.empty_like(x)
            ws = workspace(x.device, L.p3d_conv2d_dgrad_workspace_bytes(ctypes.byref(d)))
            with _Timed('dgrad', d):
                check(L.p3d_conv2d_dgrad(ctypes.byref(d), _p(dy), _p(w), _p(mult), _p(mask_in), _p(dx), _p(ws), ws.numel(), st), 'p3d_conv2d_dgrad')
            if _stash(join_put, dx):
                dx = None                                     # the consumer returns it
        w_param, b_param = ctx.params
        if ctx.needs_input_grad[1]:
            grads = _GradOut(w_param)
            d.accumulate = int(grads.direct)
            side, wst, ws = _side_launch(x.device, grads.direct, L.p3d_conv2d_wgrad_workspace_bytes(ctypes.byref(d)), dy_ready)    # behind dy (and the zeroed gradient buffer)
            with _Timed('wgrad', d, side):
                check(L.p3d_conv2d_wgrad(ctypes.byref(d), _p(dy), _p(x), _p(mult), _p(mask_in), _p(grads.bufs[0]), _p(ws), ws.numel(), wst), 'p3d_conv2d_wgrad')
            _side_launched(side, (dy, x, mult, mask_in))
            dw, = grads.done()
        if has_bias and ctx.needs_input_grad[2]:
            grads = _GradOut(b_param)
            if mult is not None:      # PartialConv with bias: d out / d b = mask_out (partial_conv.py:48-51)
                check(L.p3d_conv2d_bgrad_masked(_p(dy), _p(mult), d.N, d.K, d.Ho * d.Wo, _p(grads.bufs[0]), int(grads.direct), st), 'p3d_conv2d_bgrad_masked')
            else:
                check(L.p3d_conv2d_bgrad(_p(dy), d.N, d.K, d.Ho * d.Wo, _p(grads.bufs[0]), int(grads.direct), st), 'p3d_conv2d_bgrad')
            db, = grads.done()
        return dx, dw, db, None, None, None, None, None, None, None


def conv2d(x, w, bias=None, stride=1, pad=0, dil=1, mask_in=None, mult=None, join_put=None, join_take=None):
    return Conv2dFn.apply(x, w, bias, mask_in, mult, stride, pad, dil, join_put, join_take)


class ConvCat1x1Fn(torch.autograd.Function):
    """conv(cat([x, y], 1), w) without materialising the concat (fusionnet.py:138-139):
    two passes over disjoint input-channel windows of w, the second accumulating."""

    @staticmethod
    def forward(ctx, x, y, w):
        _need_gpu(x, y, w)
        x, y, w = x.contiguous(), y.contiguous(), w.contiguous()
        c1, c2 = x.shape[1], y.shape[1]
        if w.shape[1] != c1 + c2 or x.shape[0] != y.shape[0] or x.shape[2:] != y.shape[2:]:
            raise P3DError('conv_cat: shapes %s %s do not match weight %s' % (tuple(x.shape), tuple(y.shape), tuple(w.shape)))
        L, st = lib(), _stream()
        d1 = _desc(x.shape, w.shape, 1, 0, 1, c_offset=0, c_total=c1 + c2)
        d2 = _desc(y.shape, w.shape, 1, 0, 1, c_offset=c1, c_total=c1 + c2, accumulate=1)
        out = torch.empty((d1.N, d1.K, d1.Ho, d1.Wo), dtype=torch.float32, device=x.device)
        # (each half runs on the x3 kernels: its weight image is built per call from the half's input-channel window of w)
        ws = workspace(x.device, max(L.p3d_conv2d_fwd_workspace_bytes(ctypes.byref(d1)), L.p3d_conv2d_fwd_workspace_bytes(ctypes.byref(d2)), 16))
        check(L.p3d_conv2d_fwd(ctypes.byref(d1), _p(x), _p(w), None, None, None, _p(out), _p(ws), ws.numel(), st), 'p3d_conv2d_fwd')
        check(L.p3d_conv2d_fwd(ctypes.byref(d2), _p(y), _p(w), None, None, None, _p(out), _p(ws), ws.numel(), st), 'p3d_conv2d_fwd')
        ctx.save_for_backward(x, y, w)
        ctx.w_param = w
        return out

    @staticmethod
    def backward(ctx, dy):
        x, y, w = ctx.saved_tensors
        dy = dy.contiguous()
        c1, c2 = x.shape[1], y.shape[1]
        L, st = lib(), _stream()
        d1 = _desc(x.shape, w.shape, 1, 0, 1, c_offset=0, c_total=c1 + c2)
        d2 = _desc(y.shape, w.shape, 1, 0, 1, c_offset=c1, c_total=c1 + c2)
        dx = dyy = dw = None
        wsd = workspace(x.device, max(L.p3d_conv2d_dgrad_workspace_bytes(ctypes.byref(d1)), L.p3d_conv2d_dgrad_workspace_bytes(ctypes.byref(d2)), 16))
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            check(L.p3d_conv2d_dgrad(ctypes.byref(d1), _p(dy), _p(w), None, None, _p(dx), _p(wsd), wsd.numel(), st), 'p3d_conv2d_dgrad')
        if ctx.needs_input_grad[1]:
            dyy = torch.empty_like(y)
            check(L.p3d_conv2d_dgrad(ctypes.byref(d2), _p(dy), _p(w), None, None, _p(dyy), _p(wsd), wsd.numel(), st), 'p3d_conv2d_dgrad')
        if ctx.needs_input_grad[2]:
            grads = _GradOut(ctx.w_param)
            for d, inp in ((d1, x), (d2, y)):
                d.accumulate = int(grads.direct)
                ws = workspace(x.device, L.p3d_conv2d_wgrad_workspace_bytes(ctypes.byref(d)))
                check(L.p3d_conv2d_wgrad(ctypes.byref(d), _p(dy), _p(inp), None, None, _p(grads.bufs[0]), _p(ws), ws.numel(), st), 'p3d_conv2d_wgrad')
            dw, = grads.done()
        return dx, dyy, dw


def conv_cat1x1(x, y, w):
    return ConvCat1x1Fn.apply(x, y, w)


def mask_count(mask, kernel, stride, pad, dil):
    """partial_conv.py:35-43 (no_grad): mask [N,1,H,W] -> (mult, mask_out) [N,1,Ho,Wo]."""
    _need_gpu(mask)
    mask = mask.contiguous()
    n, one, h, w = mask.shape
    d = _desc((n, 1, h, w), (1, 1, kernel, kernel), stride, pad, dil)
    mult = torch.empty((n, 1, d.Ho, d.Wo), dtype=torch.float32, device=mask.device)
    mask_out = torch.empty_like(mult)
    check(lib().p3d_mask_count_fwd(ctypes.byref(d), _p(mask), _p(mult), _p(mask_out), _stream()), 'p3d_mask_count_fwd')
    return mult, mask_out


def nonzero_mask(x):
    """(x != 0).float()  (partial_depthnet.py:215)"""
    _need_gpu(x)
    x = x.contiguous()
    m = torch.empty_like(x)
    check(lib().p3d_nonzero_mask(_p(x), _p(m), x.numel(), _stream()), 'p3d_nonzero_mask')
    return m


# --------------------------------------------------------------------------------------------
class BatchNormActFn(torch.autograd.Function):
    """act(bn(x) + res): nn.BatchNorm2d + optional residual add + optional F.relu
    (depthnet.py:42-56,98-116).  running_mean/running_var are updated in place in training."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, res, relu, training, momentum, eps, res_join=None):
        _need_gpu(x, gamma, beta, running_mean, running_var, res)
        x = x.contiguous()
        res = None if res is None else res.contiguous()
        n, c, h, w = x.shape
        L, st = lib(), _stream()
        y = torch.empty_like(x)
        if training:
            mean = torch.empty(c, dtype=torch.float32, device=x.device)
            invstd = torch.empty_like(mean)
            ws = workspace(x.device, L.p3d_bn_workspace_bytes(n, c, h * w))
            check(L.p3d_bn_train_fwd(_p(x), _p(res), _p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(y), _p(mean), _p(invstd),
                                     n, c, h * w, momentum, eps, int(relu), _p(ws), ws.numel(), st), 'p3d_bn_train_fwd')
            # the ReLU mask of a residual-free layer is recomputed from x in backward: y is not read (nor kept alive) for it
            ctx.save_for_backward(x, y if (relu and res is not None) else None, gamma, mean, invstd, beta)
        else:
            check(L.p3d_bn_eval_fwd(_p(x), _p(res), _p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(y),
                                    n, c, h * w, eps, int(relu), st), 'p3d_bn_eval_fwd')
            ctx.save_for_backward(x, y if relu else None, gamma, running_mean, running_var, beta)
        ctx.cfg = (bool(relu), bool(training), eps, res is not None)
        ctx.params = (gamma, beta)
        ctx.res_join = res_join
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, gamma, s1, s2, beta = ctx.saved_tensors
        relu, training, eps, has_res = ctx.cfg
        dy = dy.contiguous()
        n, c, h, w = x.shape
        L, st = lib(), _stream()
        dx = torch.empty_like(x)
        dres = None
        if has_res and ctx.needs_input_grad[5]:
            dres = torch.empty_like(x) if relu else dy      # without ReLU the residual gradient is dy itself
        grads = _GradOut(*ctx.params)
        direct = grads.direct
        dgamma, dbeta = grads.bufs
        ws = workspace(x.device, L.p3d_bn_workspace_bytes(n, c, h * w))
        dres_ptr = _p(dres) if (dres is not None and relu) else None
        if training:
            check(L.p3d_bn_train_bwd(_p(dy), _p(x), _p(y), _p(gamma), _p(beta), _p(s1), _p(s2), _p(dx), dres_ptr, _p(dgamma), _p(dbeta),
                                     n, c, h * w, int(relu), int(direct), _p(ws), ws.numel(), st), 'p3d_bn_train_bwd')
        else:
            check(L.p3d_bn_eval_bwd(_p(dy), _p(x), _p(y), _p(gamma), _p(s1), _p(s2), _p(dx), dres_ptr, _p(dgamma), _p(dbeta),
                                    n, c, h * w, eps, int(relu), int(direct), _p(ws), ws.numel(), st), 'p3d_bn_eval_bwd')
        dgamma, dbeta = grads.done()
        if dres is not None and relu and _stash(ctx.res_join, dres):    # (without ReLU dres aliases dy: never hand that out)
            dres = None
        return dx, dgamma, dbeta, None, None, dres, None, None, None, None, None


def batch_norm_act(x, gamma, beta, running_mean, running_var, res=None, relu=False, training=True, momentum=0.1, eps=1e-5, res_join=None):
    return BatchNormActFn.apply(x, gamma, beta, running_mean, running_var, res, relu, training, momentum, eps, res_join)


class ReluFn(torch.autograd.Function):
    """standalone F.relu (depthnet.py:197-198 skip_relu variants)"""

    @staticmethod
    def forward(ctx, x):
        _need_gpu(x)
        x = x.contiguous()
        y = torch.empty_like(x)
        check(lib().p3d_relu_fwd(_p(x), _p(y), x.numel(), _stream()), 'p3d_relu_fwd')
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        check(lib().p3d_relu_bwd(_p(dy), _p(y), _p(dx), y.numel(), _stream()), 'p3d_relu_bwd')
        return dx


def relu(x):
    if x.dtype == torch.float16:
        from . import ops_half
        return ops_half.relu(x)
    return ReluFn.apply(x)


# --------------------------------------------------------------------------------------------
class MaxPool3x3S2Fn(torch.autograd.Function):
    """nn.MaxPool2d(kernel_size=3, stride=2, padding=1) (depthnet.py:140,192)"""

    @staticmethod
    def forward(ctx, x):
        _need_gpu(x)
        x = x.contiguous()
        n, c, h, w = x.shape
        ho, wo = conv_out(h, 3, 2, 1, 1), conv_out(w, 3, 2, 1, 1)
        y = torch.empty((n, c, ho, wo), dtype=torch.float32, device=x.device)
        need_idx = ctx.needs_input_grad[0]
        idx = torch.empty((n, c, ho, wo), dtype=torch.uint8, device=x.device) if need_idx else None
        check(lib().p3d_maxpool3x3s2_fwd(_p(x), _p(y), _p(idx), n * c, h, w, _stream()), 'p3d_maxpool3x3s2_fwd')
        ctx.save_for_backward(idx)
        ctx.in_shape = (n, c, h, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        n, c, h, w = ctx.in_shape
        dy = dy.contiguous()
        dx = torch.empty((n, c, h, w), dtype=torch.float32, device=dy.device)
        check(lib().p3d_maxpool3x3s2_bwd(_p(dy), _p(idx), _p(dx), n * c, h, w, _stream()), 'p3d_maxpool3x3s2_bwd')
        return dx


def maxpool3x3s2(x):
    return MaxPool3x3S2Fn.apply(x)


class StemTailFn(torch.autograd.Function):
    """maxpool(relu(bn(x))) of the stem in training mode as ONE node (p3d_stem_tail_fwd / bwd): the BatchNorm output (268 MB at batch 64) is neither written nor
    read; bit-identical to BatchNormActFn + MaxPool3x3S2Fn (depthnet.py:139-140)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum, eps):
        _need_gpu(x, gamma, beta, running_mean, running_var)
        x = x.contiguous()
        n, c, h, w = x.shape
        L, st = lib(), _stream()
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1         # (h // 2, w // 2 at the even sides; the odd ones come with bn_any)
        y = torch.empty((n, c, ho, wo), dtype=torch.float32, device=x.device)
        idx = torch.empty((n, c, ho, wo), dtype=torch.uint8, device=x.device)
        mean = torch.empty(c, dtype=torch.float32, device=x.device)
        invstd = torch.empty_like(mean)
        ws = workspace(x.device, L.p3d_bn_workspace_bytes(n, c, h * w))
        check(L.p3d_stem_tail_fwd(_p(x), _p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(y), _p(idx), _p(mean), _p(invstd), n, c, h, w, momentum, eps,
                                  _p(ws), ws.numel(), st), 'p3d_stem_tail_fwd')
        ctx.save_for_backward(x, idx, gamma, beta, mean, invstd)
        ctx.params = (gamma, beta)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, idx, gamma, beta, mean, invstd = ctx.saved_tensors
        n, c, h, w = x.shape
        dy = dy.contiguous()
        L, st = lib(), _stream()
        dx = torch.empty_like(x)
        grads = _GradOut(*ctx.params)
        direct = grads.direct
        dgamma, dbeta = grads.bufs
        ws = workspace(x.device, L.p3d_bn_workspace_bytes(n, c, h * w))
        check(L.p3d_stem_tail_bwd(_p(dy), _p(idx), _p(x), _p(gamma), _p(beta), _p(mean), _p(invstd), _p(dx), _p(dgamma), _p(dbeta), n, c, h, w, int(direct),
                                  _p(ws), ws.numel(), st), 'p3d_stem_tail_bwd')
        dgamma, dbeta = grads.done()
        return dx, dgamma, dbeta, None, None, None, None


def stem_tail_usable(x, bn, pool):
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and bn.training and bn.affine and bn.track_running_stats and torch.is_grad_enabled()):
        return False
    one = lambda v: v[0] if isinstance(v, (tuple, list)) else v
    if (one(pool.kernel_size), one(pool.stride), one(pool.padding), one(pool.dilation)) != (3, 2, 1, 1) or pool.ceil_mode:
        return False
    n, c, h, w = x.shape
    L = lib()
    if L.p3d_stem_tail_supported(n, c, h, w):
        return True
    on = L.p3d_bn_any_enable(0)         # (read the switch: set, then put back)
    L.p3d_bn_any_enable(on)
    return bool(on and L.p3d_stem_tail_any_supported(n, c, h, w))


def stem_tail(x, bn):
    """maxpool(relu(bn(x))) with bn's running statistics and batch counter updated as nn.BatchNorm2d.forward does (nn.py)."""
    if getattr(bn, '_ticked', False):
        bn._ticked = False
    else:
        bn.num_batches_tracked.add_(1)
    momentum = 0.1 if bn.momentum is None else bn.momentum
    return StemTailFn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, momentum, bn.eps)


# --------------------------------------------------------------------------------------------
class SoftArgmax3dFn(torch.autograd.Function):
    """utils.to_heatmap followed by utils.decode (utils.py:154-194), fused."""

    @staticmethod
    def forward(ctx, z, depth, num_joints, height, width, depth_range):
        _need_gpu(z)
        z = z.contiguous()
        b = z.shape[0]
        if tuple(z.shape[1:]) != (depth * num_joints, height, width):
            raise P3DError('softargmax3d: z %s is not [B, %d*%d, %d, %d]' % (tuple(z.shape), depth, num_joints, height, width))
        coords = torch.empty((b, num_joints, 3), dtype=torch.float32, device=z.device)
        check(lib().p3d_softargmax3d_fwd(_p(z), _p(coords), b, depth, num_joints, height, width, depth_range, _stream()), 'p3d_softargmax3d_fwd')
        ctx.save_for_backward(z)
        ctx.cfg = (depth, num_joints, height, width, depth_range)
        return coords

    @staticmethod
    def backward(ctx, dcoords):
        (z,) = ctx.saved_tensors
        depth, num_joints, height, width, depth_range = ctx.cfg
        dcoords = dcoords.contiguous()
        dz = torch.empty_like(z)
        check(lib().p3d_softargmax3d_bwd(_p(dcoords), _p(z), _p(dz), z.shape[0], depth, num_joints, height, width, depth_range, _stream()),
              'p3d_softargmax3d_bwd')
        return dz, None, None, None, None, None


def softargmax3d(z, depth, num_joints, height, width, depth_range):
    return SoftArgmax3dFn.apply(z, depth, num_joints, height, width, float(depth_range))


class PoseLossFn(torch.autograd.Function):
    """Loss block of Trainer.vanilla_train (depth_train.py:397-405): returns (loss, spec_cam)."""

    @staticmethod
    def forward(ctx, relat, true_cam, true_val, key_index, loss_div, criterion, count_override):
        _need_gpu(relat, true_cam)
        relat, true_cam = relat.contiguous(), true_cam.contiguous()
        if not true_val.is_cuda:
            raise P3DError('pose_loss: true_val must be on the HIP device')
        val = true_val.contiguous().view(torch.uint8) if true_val.dtype == torch.bool else true_val.contiguous()
        if val.dtype != torch.uint8:
            raise P3DError('pose_loss: true_val must be bool or uint8')
        b, j, _ = relat.shape
        loss = torch.empty(1, dtype=torch.float32, device=relat.device)
        spec = torch.empty_like(relat)
        drelat = torch.empty_like(relat)
        check(lib().p3d_pose_loss_fwd_bwd(_p(relat), _p(true_cam), _p(val), _p(loss), _p(spec), _p(drelat), b, j, key_index,
                                          loss_div, CRITERIA[criterion], 1.0, _p(count_override), _stream()), 'p3d_pose_loss_fwd_bwd')
        ctx.save_for_backward(drelat)
        ctx.mark_non_differentiable(spec)
        return loss.view(()), spec

    @staticmethod
    def backward(ctx, dloss, dspec):
        (drelat,) = ctx.saved_tensors
        return drelat * dloss, None, None, None, None, None, None


def pose_loss(relat, true_cam, true_val, key_index, loss_div, criterion='SmoothL1', count_override=None):
    """count_override: optional 1-element fp32 device tensor replacing 3*n_valid as the mean's divisor."""
    return PoseLossFn.apply(relat, true_cam, true_val, int(key_index), float(loss_div), criterion, count_override)


class MaskedLossFn(torch.autograd.Function):
    """criterion(pred.view(-1, C)[valid.view(-1)], target.view(-1, C)[valid.view(-1)]) with mean reduction (train.py:94,112)."""

    @staticmethod
    def forward(ctx, pred, target, valid, criterion, count_override):
        _need_gpu(pred, target)
        if not valid.is_cuda:
            raise P3DError('masked_loss: valid must be on the HIP device')
        pred, target = pred.contiguous(), target.contiguous()
        val = valid.contiguous().view(torch.uint8) if valid.dtype == torch.bool else valid.contiguous()
        if val.dtype != torch.uint8 or pred.shape != target.shape or val.numel() * pred.shape[-1] != pred.numel():
            raise P3DError('masked_loss: pred %s / target %s / valid %s do not match' % (tuple(pred.shape), tuple(target.shape), tuple(valid.shape)))
        loss = torch.empty(1, dtype=torch.float32, device=pred.device)
        dpred = torch.empty_like(pred)
        check(lib().p3d_masked_loss_fwd_bwd(_p(pred), _p(target), _p(val), _p(loss), _p(dpred), val.numel(), pred.shape[-1], CRITERIA[criterion],
                                            _p(count_override), _stream()), 'p3d_masked_loss_fwd_bwd')
        ctx.save_for_backward(dpred)
        return loss.view(())

    @staticmethod
    def backward(ctx, dloss):
        (dpred,) = ctx.saved_tensors
        return dpred * dloss, None, None, None, None


def masked_loss(pred, target, valid, criterion='SmoothL1', count_override=None):
    return MaskedLossFn.apply(pred, target, valid, criterion, count_override)


# columns of a row of p3d_pose_eval_stats (include/p3d_hip.h P3D_EVAL_*)
EVAL_VALID, EVAL_SUM_DIST, EVAL_PCK, EVAL_SUM_AUC, EVAL_SOLID, EVAL_LOSS, EVAL_BATCH, EVAL_PRESENT, EVAL_ROW = (
    CONSTANTS['P3D_EVAL_' + n] for n in ('VALID', 'SUM_DIST', 'PCK', 'SUM_AUC', 'SOLID', 'LOSS', 'BATCH', 'PRESENT', 'ROW'))
EVAL_CLASSES = ('solid', 'close', 'depth', 'jitter', 'switch', 'fail')           # columns EVAL_SOLID + 0..5


def pose_eval_stats(spec_cam, true_cam, rotate, true_val, mirror, thresh, loss, table, row, rotated=False):
    """Evaluation statistics of one test batch into table[row] (fp64 [rows, EVAL_ROW] device table), one launch, no host sync:
    spec_cam / true_cam [B,J,3] fp32 are back-rotated by rotate [B,3,3], compared over the valid joints of true_val [B,J] (bool / uint8)
    as utils.analyze does with thresh (dict solid / close / rough) and mirror (int32 [J] device tensor, entries in [0, J)); loss is the
    device scalar ops.pose_loss returned.  rotated=True also returns the back-rotated spec_cam [B,J,3]."""
    _need_gpu(spec_cam, true_cam, rotate, loss)
    if not (true_val.is_cuda and mirror.is_cuda and table.is_cuda):
        raise P3DError('pose_eval_stats: true_val, mirror and table must be on the HIP device')
    spec_cam, true_cam, rotate = spec_cam.contiguous(), true_cam.contiguous(), rotate.contiguous()
    val = true_val.contiguous().view(torch.uint8) if true_val.dtype == torch.bool else true_val.contiguous()
    if spec_cam.dim() != 3 or spec_cam.shape[2] != 3 or true_cam.shape != spec_cam.shape:
        raise P3DError('pose_eval_stats: spec_cam %s / true_cam %s must both be [B,J,3]' % (tuple(spec_cam.shape), tuple(true_cam.shape)))
    b, j, _ = spec_cam.shape
    if tuple(rotate.shape) != (b, 3, 3) or tuple(val.shape) != (b, j) or val.dtype != torch.uint8:
        raise P3DError('pose_eval_stats: rotate %s must be [B,3,3] and true_val %s bool [B,J]' % (tuple(rotate.shape), tuple(true_val.shape)))
    if loss.numel() != 1:
        raise P3DError('pose_eval_stats: loss must be the 1-element loss of ops.pose_loss')
    if mirror.dtype != torch.int32 or mirror.numel() != j or not mirror.is_contiguous():
        raise P3DError('pose_eval_stats: mirror must be a contiguous int32 [J] tensor')
    if table.dtype != torch.float64 or table.dim() != 2 or table.shape[1] != EVAL_ROW or not table.is_contiguous():
        raise P3DError('pose_eval_stats: table must be a contiguous fp64 [rows, %d] tensor' % EVAL_ROW)
    if not 0 <= row < table.shape[0]:
        raise P3DError('pose_eval_stats: row %d outside the table of %d rows' % (row, table.shape[0]))
    out = torch.empty_like(spec_cam) if rotated else None
    check(lib().p3d_pose_eval_stats(_p(spec_cam), _p(true_cam), _p(rotate), _p(val), _p(mirror), b, j, float(thresh['solid']), float(thresh['close']),
                                    float(thresh['rough']), _p(loss), ctypes.c_void_p(table[row].data_ptr()), _p(out), _stream()),
          'p3d_pose_eval_stats')
    return out


class ReconCamFn(torch.autograd.Function):
    """utils.get_recon_cam (utils.py:335-366) with its analytic backward."""

    @staticmethod
    def forward(ctx, spec_mat, relat_cam, intrinsics):
        _need_gpu(spec_mat, relat_cam, intrinsics)
        spec_mat, relat_cam, intrinsics = spec_mat.contiguous(), relat_cam.contiguous(), intrinsics.contiguous().float()
        b, j, _ = relat_cam.shape
        if tuple(spec_mat.shape) != (b, j, 2) or tuple(intrinsics.shape) != (b, 3, 3) or relat_cam.shape[2] != 3:
            raise P3DError('get_recon_cam: spec_mat %s / relat_cam %s / intrinsics %s' % (tuple(spec_mat.shape), tuple(relat_cam.shape), tuple(intrinsics.shape)))
        recon = torch.empty_like(relat_cam)
        check(lib().p3d_recon_cam_fwd(_p(spec_mat), _p(relat_cam), _p(intrinsics), _p(recon), b, j, _stream()), 'p3d_recon_cam_fwd')
        ctx.save_for_backward(spec_mat, relat_cam, intrinsics)
        return recon

    @staticmethod
    def backward(ctx, drecon):
        spec_mat, relat_cam, intrinsics = ctx.saved_tensors
        b, j, _ = relat_cam.shape
        dspec, drelat = torch.empty_like(spec_mat), torch.empty_like(relat_cam)
        check(lib().p3d_recon_cam_bwd(_p(drecon.contiguous()), _p(spec_mat), _p(relat_cam), _p(intrinsics), _p(dspec), _p(drelat), b, j, _stream()),
              'p3d_recon_cam_bwd')
        return dspec, drelat, None


def recon_cam(spec_mat, relat_cam, intrinsics):
    return ReconCamFn.apply(spec_mat, relat_cam, intrinsics)


DISTILL_MODES = {'l2': 0, 'sigmoid': 1, 'bce': 2}


class DistillFn(torch.autograd.Function):
    """Trainer.distill (depth_train.py:115-129): feature-distillation loss of the student against the (no-grad) teacher.
    Returns (weight * loss, loss); the gradient of the first output w.r.t. the student features is produced in the forward
    launch already (scaled by `weight`), so backward is free when the incoming gradient is 1 (loss = cam_loss + weight*dist)."""

    @staticmethod
    def forward(ctx, teach, student, atten, mode, weight, unit_grad):
        _need_gpu(teach, student, atten)
        teach, student, atten = teach.contiguous(), student.contiguous(), atten.contiguous()
        b, c, h, w = student.shape
        if teach.shape != student.shape or tuple(atten.shape) != (b, 1, h, w):
            raise P3DError('distill: teacher %s / student %s / attention %s do not match' % (tuple(teach.shape), tuple(student.shape), tuple(atten.shape)))
        L = lib()
        loss = torch.empty(1, dtype=torch.float32, device=student.device)
        need = ctx.needs_input_grad[1]
        ds = torch.empty_like(student) if need else None
        ws = workspace(student.device, L.p3d_distill_workspace_bytes(b))
        check(L.p3d_distill_fwd_bwd(_p(teach), _p(student), _p(atten), _p(loss), _p(ds), b, c, h * w, DISTILL_MODES[mode], float(weight),
                                    _p(ws), ws.numel(), _stream()), 'p3d_distill_fwd_bwd')
        ctx.save_for_backward(ds)
        ctx.unit_grad = unit_grad
        raw = loss.view(())
        weighted = raw * weight if weight != 1.0 else raw.clone()
        ctx.mark_non_differentiable(raw)
        return weighted, raw

    @staticmethod
    def backward(ctx, dweighted, draw):
        (ds,) = ctx.saved_tensors
        if ds is not None and not ctx.unit_grad:
            ds = ds * dweighted
        return None, ds, None, None, None, None


def distill_loss(teach, student, atten, mode='l2', weight=1.0, unit_grad=False):
    return DistillFn.apply(teach, student, atten, mode, float(weight), unit_grad)


# --------------------------------------------------------------------------------------------
def l2norm_sq_accum(flat, accum):
    check(lib().p3d_l2norm_sq_accum(_p(flat), flat.numel(), _p(accum), _stream()), 'p3d_l2norm_sq_accum')


def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, max_norm=0.0, norm_sq=None, grad_scale=1.0):
    check(lib().p3d_adam_step(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, weight_decay, int(step), float(max_norm),
                              _p(norm_sq), float(grad_scale), _stream()), 'p3d_adam_step')


def adam_step_dev(p, g, m, v, lr, beta1, beta2, eps, weight_decay, state, max_norm, norm_sq, grad_scale, skip_nonfinite, scratch):
    """Adam with the step counter / overflow skip on the device (state: int32[2] = steps taken, steps skipped)."""
    check(lib().p3d_adam_step_dev(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, weight_decay, _p(state), float(max_norm),
                                  _p(norm_sq), float(grad_scale), int(skip_nonfinite), _p(scratch), _stream()), 'p3d_adam_step_dev')


def augment_colour_(img, params):
    """In place on img [B,3,H,W] holding 0..255 values; params [B,4] (augment_colour.py:48-67)."""
    _need_gpu(img, params)
    b, c, h, w = img.shape
    if c != 3 or not img.is_contiguous():
        raise P3DError('augment_colour: need a contiguous [B,3,H,W] image')
    check(lib().p3d_augment_colour(_p(img), _p(params.contiguous()), b, h, w, _stream()), 'p3d_augment_colour')
    return img


def augment_erase_(img, rects, colour):
    """In place: fill rects [B,4] int32 (x0,y0,x1,y1) with colour [B,C] (augment_occluder.py:84-105)."""
    _need_gpu(img, colour)
    b, c, h, w = img.shape
    if rects.dtype != torch.int32 or not img.is_contiguous():
        raise P3DError('augment_erase: rects must be int32 and img contiguous')
    check(lib().p3d_augment_erase(_p(img), _p(rects.contiguous()), _p(colour.contiguous()), b, c, h, w, _stream()), 'p3d_augment_erase')
    return img


def augment_occlude_(img, bank, alpha, plan, max_pixels, truncate=True):
    """In place: paste one occluder per image (augment_occluder.py:7-55).  bank [P,C] fp32, alpha [P] fp32 or None, plan [B,8] int32 (augment.plan_paste)."""
    _need_gpu(img, bank, alpha)
    b, c, h, w = img.shape
    if plan.dtype != torch.int32 or not plan.is_cuda or tuple(plan.shape) != (b, 8) or not img.is_contiguous() or bank.shape[-1] != c:
        raise P3DError('augment_occlude: plan must be int32 [B,8] on the device, img contiguous, bank [P,C]')
    check(lib().p3d_augment_occlude(_p(img), _p(bank.contiguous()), _p(None if alpha is None else alpha.contiguous()), _p(plan.contiguous()), b, c, h, w,
                                    int(max_pixels), int(bool(truncate)), _stream()), 'p3d_augment_occlude')
    return img


IMAGENET_MEAN = (0.485, 0.456, 0.406)       # depth_datasets.py:78-79
IMAGENET_STD = (0.229, 0.224, 0.225)


def normalize_rgb_(img, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """In place: transforms.ToTensor() + Normalize on a contiguous [B,3,H,W] fp32 device tensor holding 0..255 values."""
    _need_gpu(img)
    b, c, h, w = img.shape
    if c != 3 or not img.is_contiguous():
        raise P3DError('normalize_rgb: need a contiguous [B,3,H,W] image')
    m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    check(lib().p3d_normalize_rgb(_p(img), b, h * w, m3, s3, _stream()), 'p3d_normalize_rgb')
    return img


def warp_crops(frames, homography, out_hw):
    """Batch of crop re-projections (depth_datasets.py:153-193): frames [B,Hs,Ws,C] uint8 or fp32 (interleaved, as decoded),
    homography [B,3,3] fp32 mapping crop pixels to frame pixels -> [B,C,Ho,Wo] fp32 (0..255 values for uint8 sources)."""
    if not frames.is_cuda or frames.dtype not in (torch.uint8, torch.float32) or frames.dim() != 4:
        raise P3DError('warp_crops: frames must be a [B,Hs,Ws,C] uint8 / fp32 tensor on the HIP device')
    _need_gpu(homography)
    frames, homography = frames.contiguous(), homography.contiguous()
    b, hs, ws, c = frames.shape
    if tuple(homography.shape) != (b, 3, 3):
        raise P3DError('warp_crops: homography must be [B,3,3]')
    ho, wo = out_hw
    out = torch.empty((b, c, ho, wo), dtype=torch.float32, device=frames.device)
    check(lib().p3d_warp_crops(_p(frames), int(frames.dtype == torch.uint8), _p(homography), _p(out), b, hs, ws, c, ho, wo, _stream()), 'p3d_warp_crops')
    return out


def set_x3(on):
    """Exact-fp32 convolution kernels on the bf16 matrix pipe (csrc/p3d_fx.hip), ON by default; set_x3(False) (or P3D_X3=0) keeps every layer on the
    fp32-MFMA kernels.  Returns the previous setting."""
    global X3_EPOCH
    X3_EPOCH += 1                       # (ops_block caches per-block plans that depend on it)
    return bool(lib().p3d_x3_enable(int(bool(on))))


def x3_any(on):
    """Opt-in, OFF by default (P3D_X3_ANY=1 turns it on): the per-layer training path (Conv2dFn: forward, stride-1 data gradient, weight gradient) runs dense
    convolutions on the x3 kernels at map widths that are no multiples of 4 -- the 65 / 33 / 17 maps of the default 257 crop -- instead of the fp32-MFMA
    kernels.  Returns the previous setting."""
    return bool(lib().p3d_x3_any_enable(int(bool(on))))


def x3_any_partial(on):
    """Opt-in, OFF by default (P3D_X3_ANY_PARTIAL=1 turns it on), independent of x3_any: the per-layer training path runs PARTIAL convolutions (PartialConv without
    a bias: both factors given) on the masked x3 kernels at map widths that are no multiples of 4 -- forward, stride-1 data gradient and weight gradient of the
    partial families' layer1 / layer2 at the default 257 crop -- instead of the fp32-MFMA kernels.  Returns the previous setting."""
    return bool(lib().p3d_x3_any_partial_enable(int(bool(on))))


def x3_any_strided(on):
    """Opt-in, OFF by default (P3D_X3_ANY_STRIDED=1 turns it on), independent of x3_any, x3_any_partial and x3_any_images: the per-layer training path runs dense
    STRIDE-2 data gradients on the x3 kernels at maps the aligned kernels refuse -- the 129 -> 65 -> 33 -> 17 transitions of the default 257 crop, layers of 96 input
    channels or more -- as one ragged launch per parity class and one interleave pass, instead of the fp32-MFMA kernels.  Returns the previous setting."""
    return bool(lib().p3d_x3_any_strided_enable(int(bool(on))))


def bn_any(on):
    """Opt-in, OFF by default (P3D_BN_ANY=1 turns it on), independent of every other switch: BatchNorm calls whose rows start on no 16-B line (H * W no multiple
    of 4: the 129 / 65 / 33 / 17 maps of the default 257 crop) run on the peeled 16-B instances of csrc/p3d_bn.hip instead of the element-by-element ones, and the
    stem's maxpool(relu(bn(c))) stays one node (stem_tail) at any sides.  Returns the previous setting."""
    return bool(lib().p3d_bn_any_enable(int(bool(on))))


def bn_last_launch():
    """What the last BatchNorm / stem-tail call launched (p3d_bn_last_launch): dict of entry (1 train_fwd, 2 train_bwd, 3 eval_fwd, 4 eval_bwd, 5 stem_tail_fwd,
    6 stem_tail_bwd), instance (0 vector, 1 scalar, 2 peeled) and grid (x, y)."""
    out = (ctypes.c_int32 * 4)()
    lib().p3d_bn_last_launch(out)
    return {'entry': out[0], 'instance': out[1], 'grid': (out[2], out[3])}


def x3_any_images(on):
    """Opt-in, OFF by default (P3D_X3_ANY_IMAGES=1 turns it on), independent of x3_any and x3_any_partial: multi-tap convolutions that travel as pre-split images
    (ops_block.ConvImagesFn: nn.Conv2d called without a join, 64 input channels or more -- the regressor and the stride-1 3x3 layers of the per-layer path) do so at
    map sizes the aligned image-fed kernels refuse too -- the 129 / 65 / 33 / 17 maps of the default 257 crop -- on the ragged image-fed instances
    (p3d_fx_conv_*_img_any) instead of going to ops.conv2d.  Returns the previous setting."""
    global X3_EPOCH
    X3_EPOCH += 1                       # (ops_block.conv_takes_images caches its answer per shape and epoch)
    return bool(lib().p3d_x3_any_images_enable(int(bool(on))))


def x3_any_images_enabled():
    """The setting of x3_any_images, left as it is.  (The library keeps it -- P3D_X3_ANY_IMAGES and direct calls of p3d_x3_any_images_enable count -- and its one
    entry returns the previous setting, so it is read by setting and restoring; ops_block.conv_takes_images asks once per shape and epoch.)"""
    L = lib()
    on = L.p3d_x3_any_images_enable(0)
    L.p3d_x3_any_images_enable(on)
    return bool(on)


def block_any(on):
    """Opt-in, OFF by default (P3D_BLOCK_ANY=1 turns it on), independent of every other switch: the residual-block executor (ops_block.residual_block) also takes
    dense blocks whose convolutions all have stride 1 at map sizes the aligned kernels refuse -- the 65 / 33 / 17 maps of the default 257 crop: 14 of ResNet-50's
    16 blocks at -stride 16 -- on the ragged image-fed instances, instead of leaving them to the per-layer path.  Returns the previous setting."""
    global X3_EPOCH
    X3_EPOCH += 1                       # (ops_block caches per-block plans that depend on it)
    return bool(lib().p3d_block_any_enable(int(bool(on))))


def block_any_strided(on):
    """Opt-in, OFF by default (P3D_BLOCK_ANY_STRIDED=1 turns it on), independent of every other switch, block_any and x3_any_strided included: the residual-block
    executor also takes dense blocks that carry a STRIDE-2 convolution at map sizes the aligned kernels refuse -- layer2.0 and layer3.0 at the default 257 crop, the two
    blocks block_any leaves to the per-layer path -- with the stride-2 data gradients as image-fed class launches and one joining pass.  Returns the previous setting."""
    global X3_EPOCH
    X3_EPOCH += 1                       # (ops_block caches per-block plans that depend on it)
    return bool(lib().p3d_block_any_strided_enable(int(bool(on))))


FROZEN_FOLD = os.environ.get('P3D_FROZEN_FOLD', '0') == '1'


def frozen_fold(on):
    """Opt-in, OFF by default (P3D_FROZEN_FOLD=1 turns it on): a dense conv + BatchNorm pair of a residual block whose BatchNorm is frozen (eval mode, the
    reference's -do_freeze) trains on the folded convolution -- one x3 inference forward with b', the residual and the ReLU in its epilogue, no BatchNorm pass
    in either direction and no conv output kept (ops_frozen.py).  Returns the previous setting."""
    global FROZEN_FOLD
    previous, FROZEN_FOLD = FROZEN_FOLD, bool(on)
    return previous


FROZEN_FOLD_HALF = os.environ.get('P3D_FROZEN_FOLD_HALF', '0') == '1'


def frozen_fold_half(on):
    """frozen_fold for -half_acc, a switch of its own, OFF by default (P3D_FROZEN_FOLD_HALF=1 turns it on): a frozen conv + BatchNorm pair of a dense residual
    block that runs on fp16 NHWC activations trains on the folded fp16 convolution -- one p3d_hconv2d_fwd_infer launch with b', the residual and the ReLU in its
    epilogue, no BatchNorm pass in either direction and no conv output kept (ops_frozen.HFrozenConvBnFn).  frozen_fold and ops_frozen.admits keep their meaning:
    fp16 input is still refused there.  Returns the previous setting."""
    global FROZEN_FOLD_HALF
    previous, FROZEN_FOLD_HALF = FROZEN_FOLD_HALF, bool(on)
    return previous


X3_EPOCH = 0
WEIGHT_EPOCH = 0          # bumped whenever parameters are written behind torch's back (FlatAdam's kernels, broadcasts into / restores of flat_p): cached per-weight derivatives (ops_block.weight_images) are stale


def weights_changed():
    """Call after writing parameters through anything torch's version counters do not see on the parameter itself: the optimizer kernels, a
    broadcast or copy into FlatAdam.flat_p (the parameters are views of it, and an in-place write to the base does not bump a view's _version)."""
    global WEIGHT_EPOCH
    WEIGHT_EPOCH += 1


def act_image(x, mode=0, x2=None, table=None, masked=False, out=None):
    """Pre-split activation image of a fp32 NCHW tensor (p3d_fx_act_image): uint8 tensor of 6 bytes per element = three bf16 planes [N][C/16][H*W][16].
    mode 0: x; 1: relu(x * sc + sh); 2: A * (masked ? x * [x2 * sc + sh > 0] : x) + B * x2 + K, constants per channel from `table` [C][8].
    H * W no multiple of 4: mode 0 only (p3d_fx_act_image_any: the same bytes at any map size)."""
    _need_gpu(x)
    x = x.contiguous()
    n, c, h, w = x.shape
    if (h * w) % 4 != 0 and mode != 0:
        raise P3DError('act_image: mode %d needs H * W in steps of 4 (%d x %d); only the plain image (mode 0) exists at any map size' % (mode, h, w))
    nbytes = lib().p3d_fx_act_image_bytes(n, c, h * w)
    img = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if out is None else out
    if img.numel() != nbytes or img.dtype != torch.uint8 or not img.is_contiguous():
        raise P3DError('act_image: `out` must be a contiguous uint8 tensor of %d bytes' % nbytes)
    if (h * w) % 4 != 0:
        check(lib().p3d_fx_act_image_any(_p(x), _p(img), n, c, h * w, _stream()), 'p3d_fx_act_image_any')
        return img
    check(lib().p3d_fx_act_image(mode, _p(x), None if x2 is None else _p(x2.contiguous()), None if table is None else _p(table.contiguous()), int(bool(masked)),
                                 _p(img), n, c, h * w, _stream()), 'p3d_fx_act_image')
    return img


def row_image(x, mode=0, x2=None, table=None, masked=False, out=None):
    """Row image of a fp32 NCHW tensor (p3d_fx_row_image): uint8 tensor of 4 bytes per element = the fp32 values as [N][C/16][H*W][16]; modes as act_image.
    C in steps of 16, H * W in steps of 4."""
    _need_gpu(x)
    x = x.contiguous()
    n, c, h, w = x.shape
    nbytes = lib().p3d_fx_row_image_bytes(n, c, h * w)
    img = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if out is None else out
    if img.numel() != nbytes or img.dtype != torch.uint8 or not img.is_contiguous():
        raise P3DError('row_image: `out` must be a contiguous uint8 tensor of %d bytes' % nbytes)
    check(lib().p3d_fx_row_image(mode, _p(x), None if x2 is None else _p(x2.contiguous()), None if table is None else _p(table.contiguous()), int(bool(masked)),
                                 _p(img), n, c, h * w, _stream()), 'p3d_fx_row_image')
    return img


def open_images(x, gmask, partial, count, sides, rows=False):
    """The image passes that open a block's backward pass (p3d_fx_open_images; tests): x the upstream gradient, gmask the closing ReLU's mask bytes or None, partial the
    fp64 sums [C][nrows][3], sides one or two tuples (c, table, gamma).  Returns per side (image, dgamma, dbeta); two sides run as the one pair pass."""
    _need_gpu(x)
    x = x.contiguous()
    n, c, h, w = x.shape
    L = lib()
    nbytes = (L.p3d_fx_row_image_bytes if rows else L.p3d_fx_act_image_bytes)(n, c, h * w)
    out, args = [], []
    for (ct, tab, gamma) in sides:
        img = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        dg, db = torch.empty(c, dtype=torch.float32, device=x.device), torch.empty(c, dtype=torch.float32, device=x.device)
        out.append((img, dg, db))
        args += [_p(ct.contiguous()), _p(tab.contiguous()), _p(gamma.contiguous()), _p(dg), _p(db), _p(img)]
    if len(sides) == 1:
        args += [None] * 6
    assert partial.dtype == torch.float64 and partial.is_contiguous() and partial.shape[0] == c and partial.shape[2] == 3
    check(L.p3d_fx_open_images(int(bool(rows)), _p(x), None if gmask is None else _p(gmask), _p(partial), partial.shape[1], float(count), *args, n, c, h * w, _stream()),
          'p3d_fx_open_images')
    return out


def conv2d_img(pass_, x_shape, w, stride, pad, dil, x_img=None, dy_img=None, x=None, bias=None, accumulate_into=None, rows=False):
    """One pass of a convolution on pre-split image operands (p3d_fx_conv_*_img; what the block executor launches): 'fwd' -> y from x_img,
    'dgrad' -> dx from dy_img, 'wgrad' -> dw from dy_img and x_img (or the fp32 x).  rows: the images are row images (row_image; p3d_fx_conv_*_rows).
    For tests and tools/conv_bench.py."""
    _need_gpu(w)
    w = w.contiguous()
    d = _desc(x_shape, w.shape, stride, pad, dil)
    which = {'fwd': 0, 'dgrad': 1, 'wgrad': 2}[pass_]
    L, form = lib(), 'rows' if rows else 'img'
    ws = workspace(w.device, L.p3d_fx_conv_img_workspace_bytes(ctypes.byref(d), which))
    if which == 0:
        y = torch.empty((d.N, d.K, d.Ho, d.Wo), dtype=torch.float32, device=w.device)
        check(getattr(L, 'p3d_fx_conv_fwd_' + form)(ctypes.byref(d), _p(x_img), _p(w), None, None if bias is None else _p(bias), _p(y), _p(ws), ws.numel(), _stream()),
              'p3d_fx_conv_fwd_' + form)
        return y
    if which == 1:
        dx = torch.empty(tuple(x_shape), dtype=torch.float32, device=w.device) if accumulate_into is None else accumulate_into
        d.accumulate = int(accumulate_into is not None)
        check(getattr(L, 'p3d_fx_conv_dgrad_' + form)(ctypes.byref(d), _p(dy_img), _p(w), None, _p(dx), _p(ws), ws.numel(), _stream()), 'p3d_fx_conv_dgrad_' + form)
        return dx
    dw = torch.empty_like(w)
    check(getattr(L, 'p3d_fx_conv_wgrad_' + form)(ctypes.byref(d), _p(dy_img), None if x is None else _p(x.contiguous()), None if x_img is None else _p(x_img), _p(dw), _p(ws),
                                                  ws.numel(), _stream()), 'p3d_fx_conv_wgrad_' + form)
    return dw


def profile_convs(on):
    """HIP-event brackets around every conv launch inside the library (p3d_profile_enable); returns the previous setting."""
    return lib().p3d_profile_enable(int(on))          # 0 off, 1 brackets, 2 brackets + kernel-end marks (collect_conv_profile(kernel_only=True))


def collect_conv_profile(kernel_only=False):
    """Synchronises; dict(kind -> (ms, algorithmic flops, launches)) for 'fwd', 'dgrad', 'wgrad' since the last collect.  kernel_only: (ms, flops, launches,
    ms of the conv kernels alone -- without the split-K / slab sums queued behind them)."""
    ms, kms, fl, n = (ctypes.c_double * 3)(), (ctypes.c_double * 3)(), (ctypes.c_double * 3)(), (ctypes.c_int64 * 3)()
    check(lib().p3d_profile_collect2(ms, kms, fl, n), 'p3d_profile_collect2')
    if kernel_only:
        return {k: (float(ms[i]), float(fl[i]), int(n[i]), float(kms[i])) for i, k in enumerate(('fwd', 'dgrad', 'wgrad'))}
    return {k: (float(ms[i]), float(fl[i]), int(n[i])) for i, k in enumerate(('fwd', 'dgrad', 'wgrad'))}


def conv_path_stats(reset=False):
    """Conv launches and algorithmic flops per path since the last reset: dict(x3=dict(fwd, dgrad, wgrad), fp32=dict(...)), each (launches, flops)."""
    counts, flops = (ctypes.c_uint64 * 6)(), (ctypes.c_double * 6)()
    lib().p3d_conv_path_stats(counts, flops, int(bool(reset)))
    names = ('fwd', 'dgrad', 'wgrad')
    return dict(x3={n: (int(counts[i]), float(flops[i])) for i, n in enumerate(names)},
                fp32={n: (int(counts[3 + i]), float(flops[3 + i])) for i, n in enumerate(names)})


# the record of p3d_conv_last_fp32_launch: include/p3d_hip.h and the enum of csrc/p3d_conv.hip define the layout; tests/test_fp32_mfma_instances_host.py holds these to them
LAST_FP32_FIELDS = ('pass_', 'tile', 'tapm', 'masked', 'wv', 'grid_x', 'grid_y', 'y_means', 'weight_image', 'finish', 'eval', 'no_room')
LAST_FP32_LEN = CONSTANTS['P3D_FP32_LAUNCH_FIELDS']


def conv_last_fp32_launch():
    """What the last per-layer convolution call launched on the fp32-MFMA kernels (p3d_conv_last_fp32_launch): dict of LAST_FP32_FIELDS, pass_ -1 when it
    launched nothing there."""
    out = (ctypes.c_int32 * LAST_FP32_LEN)()
    lib().p3d_conv_last_fp32_launch(out)
    return {n: int(out[i]) for i, n in enumerate(LAST_FP32_FIELDS)}


# the record of p3d_fx_launch_log, and (its first FX_INSTANCE_LEN fields) of p3d_fx_conv_instances: include/p3d_hip.h and the enum of csrc/p3d_fx.hip define the layout;
# tests/test_fx_instances_host.py holds these to them
FX_LAUNCH_FIELDS = ('kernel', 'amode', 'pro', 'epi', 'tapi', 'rag', 'rows', 'grid_x', 'grid_y', 'grid_z', 'kchunk', 'finish', 'finish_groups')
FX_LAUNCH_LEN = CONSTANTS['P3D_FX_LAUNCH_FIELDS']
FX_INSTANCE_LEN = CONSTANTS['P3D_FX_INSTANCE_FIELDS']
FX_LOG_MAX = 256            # records the library keeps between two resets


def fx_launch_log(reset=True):
    """The forward / data-gradient conv-kernel launches of the x3 path since the last reset (p3d_fx_launch_log), oldest first: (records, count) with one dict of
    FX_LAUNCH_FIELDS per kept record; count > len(records) when more than FX_LOG_MAX were made."""
    out = (ctypes.c_int32 * (FX_LAUNCH_LEN * FX_LOG_MAX))()
    count = lib().p3d_fx_launch_log(out, FX_LOG_MAX, int(bool(reset)))
    return [{n: int(out[i * FX_LAUNCH_LEN + j]) for j, n in enumerate(FX_LAUNCH_FIELDS)} for i in range(min(count, FX_LOG_MAX))], count


# the record of p3d_fx_wgrad_launch_log: the plan of p3d_fx_wgrad_plan, the finishing kernels, `accumulate`; tests/test_x3_wgrad_instances_host.py holds these to the header
FX_WGRAD_LAUNCH_FIELDS = ('family', 'aimg', 'bimg', 'masked', 'taps', 'rows', 'tile_taps', 'splits', 'spb', 'grid_x', 'grid_y', 'grid_z', 'order', 'tapm', 'slab_bytes_lo',
                          'slab_bytes_hi', 'finish', 'accumulate')
FX_WGRAD_LAUNCH_LEN = CONSTANTS['P3D_FX_WGRAD_LAUNCH_FIELDS']


def fx_wgrad_launch_log(reset=True):
    """The weight-gradient launches of the x3 path since the last reset (p3d_fx_wgrad_launch_log), oldest first: (records, count) with one tuple of FX_WGRAD_LAUNCH_LEN
    values per kept record (the first of them named by FX_WGRAD_LAUNCH_FIELDS, the rest 0); count > len(records) when more than FX_LOG_MAX were made."""
    out = (ctypes.c_int32 * (FX_WGRAD_LAUNCH_LEN * FX_LOG_MAX))()
    count = lib().p3d_fx_wgrad_launch_log(out, FX_LOG_MAX, int(bool(reset)))
    return [tuple(int(v) for v in out[i * FX_WGRAD_LAUNCH_LEN:(i + 1) * FX_WGRAD_LAUNCH_LEN]) for i in range(min(count, FX_LOG_MAX))], count


def fx_conv_instances():
    """Every compiled instance of fx_conv_kernel / fx16_conv_kernel (p3d_fx_conv_instances) as a tuple of the first FX_INSTANCE_LEN values of FX_LAUNCH_FIELDS."""
    n = lib().p3d_fx_conv_instances(None, 0)
    out = (ctypes.c_int32 * (FX_INSTANCE_LEN * n))()
    assert lib().p3d_fx_conv_instances(out, n) == n
    return [tuple(int(out[i * FX_INSTANCE_LEN + j]) for j in range(FX_INSTANCE_LEN)) for i in range(n)]


def fx_conv_any_sums_instances():
    """The instances fx_conv_instances leaves out (p3d_fx_conv_any_sums_instances), in the same form: the ragged image-fed ones with the BatchNorm epilogues."""
    n = lib().p3d_fx_conv_any_sums_instances(None, 0)
    out = (ctypes.c_int32 * (FX_INSTANCE_LEN * n))()
    assert lib().p3d_fx_conv_any_sums_instances(out, n) == n
    return [tuple(int(out[i * FX_INSTANCE_LEN + j]) for j in range(FX_INSTANCE_LEN)) for i in range(n)]


def reproject_crops(frames, params20, out_hw, round_u8=True):
    """Batch of cameralib.reproject_image calls (cameralib.py:378-443): frames [B,Hs,Ws,C] uint8 / fp32 as decoded, params20 [B,20] fp32
    (cameralib.reproject_params) -> [B,C,Ho,Wo] fp32."""
    if not frames.is_cuda or frames.dtype not in (torch.uint8, torch.float32) or frames.dim() != 4:
        raise P3DError('reproject_crops: frames must be a [B,Hs,Ws,C] uint8 / fp32 tensor on the HIP device')
    _need_gpu(params20)
    frames, params20 = frames.contiguous(), params20.contiguous()
    b, hs, ws, c = frames.shape
    if tuple(params20.shape) != (b, 20) or params20.dtype != torch.float32:
        raise P3DError('reproject_crops: params20 must be fp32 [B,20]')
    ho, wo = out_hw
    out = torch.empty((b, c, ho, wo), dtype=torch.float32, device=frames.device)
    check(lib().p3d_reproject_crops(_p(frames), int(frames.dtype == torch.uint8), _p(params20), _p(out), b, hs, ws, c, ho, wo, int(bool(round_u8)),
                                    _stream()), 'p3d_reproject_crops')
    return out


def enhance_depth_(crops, threshold, nexponent, factor=None):
    """In place: depth_datasets.enhance_ntu / enhance_pku (depth_datasets.py:39-56) on PNG-unit depth crops, after the optional utils.to_depth
    division by `factor` (same shape)."""
    _need_gpu(crops, factor)
    if crops.dtype != torch.float32 or not crops.is_contiguous() or (factor is not None and (factor.shape != crops.shape or not factor.is_contiguous())):
        raise P3DError('enhance_depth_: contiguous fp32 crops (and factor of the same shape) expected')
    check(lib().p3d_enhance_depth(_p(crops), _p(factor), crops.numel(), float(threshold), int(bool(nexponent)), _stream()), 'p3d_enhance_depth')
    return crops


def conv_bn_eval(x, conv, bn, res=None, relu=False):
    """Inference only (no autograd): conv (no bias) + BatchNorm with frozen statistics (+ residual, + ReLU) as one kernel launch
    (model.eval() forward of a residual block, depthnet.py:42-56,98-116)."""
    from .nn import _one
    _need_gpu(x, conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, res)
    x = x.contiguous()
    res = None if res is None else res.contiguous()
    d = _desc(x.shape, conv.weight.shape, _one(conv.stride), _one(conv.padding), _one(conv.dilation))
    y = torch.empty((d.N, d.K, d.Ho, d.Wo), dtype=torch.float32, device=x.device)
    L = lib()
    ws = workspace(x.device, L.p3d_conv2d_bn_eval_fwd_workspace_bytes(ctypes.byref(d)))
    check(L.p3d_conv2d_bn_eval_fwd(ctypes.byref(d), _p(x), _p(conv.weight.detach()), _p(bn.weight.detach()), _p(bn.bias.detach()), _p(bn.running_mean),
                                   _p(bn.running_var), bn.eps, _p(res), int(relu), _p(y), _p(ws), ws.numel(), _stream()), 'p3d_conv2d_bn_eval_fwd')
    return y


def can_fuse_eval(x, conv, bn):
    """The fused inference kernel applies when nothing needs a gradient, BN uses its running statistics and the conv is plain."""
    return (not torch.is_grad_enabled() and not bn.training and x.dtype == torch.float32 and conv.bias is None
            and type(conv).__name__ == 'Conv2d' and bn.track_running_stats)
