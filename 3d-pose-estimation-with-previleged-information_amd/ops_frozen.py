"""Training through a FROZEN BatchNorm (eval mode: the reference's -do_freeze, depth_train.py:172-173, depthnet.py:158-161) on the folded convolution.

A frozen BatchNorm is a per-channel affine map, so behind a convolution it folds into the weights and a bias exactly as for inference (infer.py):
s = gamma / sqrt(var + eps), w' = w * s, b' = beta - mean * s, u = conv(x, w') + b' (+ res), y = relu?(u).  Nothing in training needs the conv output
z = conv(x, w) either:

    g = dy * [y > 0]  (g = dy without a ReLU)        dres = g        dx = dgrad(g, w')        raw = wgrad(x, g)
    dw[k] = s[k] * raw[k]        dbeta[k] = sum_p g[k, p]        dgamma[k] = (<w[k], raw[k]> - mean[k] * dbeta[k]) / sqrt(var[k] + eps)

(the last because sum_p g[k, p] * z[k, p] = sum_{c, tap} w[k, c, tap] * raw[k, c, tap]).  So a layer is one folded conv in forward, on the kernels the
inference fold uses (p3d_fx_conv_fwd_infer, at map widths that are no multiples of 4 p3d_fx_conv_fwd_infer_any), and in backward one mask pass
(p3d_frozen_grad_mask), the two conv gradients as any layer launches them, and a weight-sized finishing kernel (p3d_frozen_wgrad_finish); z is never
written and never kept, and there is no BatchNorm pass in either direction.

Opt-in: ops.frozen_fold(True) / P3D_FROZEN_FOLD=1.  _trunk.py offers every conv + BatchNorm pair of a dense residual block (downsample branch included) to
`admits`; a pair it refuses runs as before, launch for launch.

FrozenFold is the plan: ONE device buffer with the forward image of w' (fold kind 0), b' and the fp32 w' itself (kind 1: the data gradient's weight) of every
pair, filled by one p3d_fx_fold_bn_images launch, and folded again before the first forward after anything it read has changed (ops.WEIGHT_EPOCH and the
_version of w, gamma, beta and the running statistics: the staleness rule of ops_block.weight_images).  A network (TrunkBase) has one for all its pairs, checked
once per forward by a pre-hook; a pair used on its own gets a plan of one.  Two forwards with nothing written in between (-semi_teach) see one fold.  A backward
whose fold has been replaced since its forward raises P3DError: its w' is gone.

-half_acc has a twin of all this behind a switch of its own, ops.frozen_fold_half(True) / P3D_FROZEN_FOLD_HALF=1 (`admits` still refuses fp16 input; `admits_half`
is the rule there): HFrozenConvBnFn runs the folded fp16 forward of the inference fold (p3d_hconv2d_fwd_infer on a kind-2 image of w' with b', the residual and the
ReLU in its epilogue) and, in backward, p3d_hfrozen_grad_mask on NHWC fp16, p3d_hconv2d_dgrad on a kind-4 image (w' in the data gradient's layout),
p3d_hconv2d_wgrad into fp32 scratch and the same p3d_frozen_wgrad_finish on the fp32 masters.  Its plan (FrozenFold with _HUnit units) holds the kind-2 image, b'
and the kind-4 image of every pair, under the same staleness rule and generation counter; the two nodes share one backward (_backward).
"""
import ctypes

import torch

from . import ops, ops_half
from ._lib import FoldJob, P3DError, check, lib
from .nn import _one
from .ops_block import _Transient

_ALIGN = 256


def _up(v):
    return (v + _ALIGN - 1) // _ALIGN * _ALIGN


def _static_ok(conv, bn):
    """What of the admission rule depends on the modules alone: a plain bias-free Conv2d the fold takes, and a BatchNorm with running statistics."""
    if type(conv).__name__ != 'Conv2d' or conv.bias is not None or not isinstance(bn, torch.nn.BatchNorm2d):
        return False
    if not (bn.affine and bn.track_running_stats) or conv.weight.dtype != torch.float32:
        return False
    k, c, r, s = conv.weight.shape
    return c % 16 == 0 and r == s and (r & 1) == 1 and k % 16 == 0 and 32 <= k <= 2048 and bn.num_features == k


def admits(x, conv, bn):
    """The admission rule, host only: the switch is on, gradients are enabled, x is fp32, the conv is a plain bias-free Conv2d, its BatchNorm is in eval mode
    with running statistics, and one of the two folded forward entries takes the shape."""
    if not (ops.FROZEN_FOLD and torch.is_grad_enabled() and x.dtype == torch.float32 and x.dim() == 4 and not bn.training and _static_ok(conv, bn)):
        return False
    if x.shape[1] != conv.weight.shape[1]:
        return False
    return _unit(conv, bn).entry(tuple(x.shape)) is not None


class _Unit:
    """One conv + BatchNorm pair of a plan: where its image, b' and w' live in the buffer, what was folded, and which forward entry takes which input shape."""
    slot, model_slot = '_frozen_unit', '_frozen_fold'       # where a conv module keeps its unit and a network its plan

    def __init__(self, conv, bn):
        self.conv, self.bn = conv, bn
        k, c, r, s = conv.weight.shape
        self.k, self.c, self.r = k, c, r
        self.stride, self.pad, self.dil = _one(conv.stride), _one(conv.padding), _one(conv.dilation)
        self.plan = None
        self.seen = None                # the _key() of the last fold, None: not folded (BatchNorm in training mode then)
        self.entries = {}
        self.img_off = self.img_bytes = self.bias_off = self.w_off = None

    def layout(self, at):
        fb = ctypes.c_size_t()
        check(lib().p3d_fx_weight_image_bytes(self.k, self.c, self.r * self.r, ctypes.byref(fb), None), 'p3d_fx_weight_image_bytes')
        self.img_off, self.img_bytes = at, fb.value
        self.bias_off = _up(at + fb.value)
        self.w_off = _up(self.bias_off + 4 * self.k)
        return _up(self.w_off + 4 * self.k * self.c * self.r * self.r)

    def tensors(self):
        bn = self.bn
        return self.conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var

    def _key(self):
        return tuple(t._version for t in self.tensors())

    def desc(self, x_shape, accumulate=0):
        return ops._desc(x_shape, (self.k, self.c, self.r, self.r), self.stride, self.pad, self.dil, accumulate=accumulate)

    def entry(self, x_shape):
        """0: p3d_fx_conv_fwd_infer takes this input shape, 1: p3d_fx_conv_fwd_infer_any does, None: neither (host only, remembered per shape)."""
        e = self.entries.get(x_shape, -1)
        if e == -1:
            L, d = lib(), self.desc(x_shape)
            e = None
            if d.Ho > 0 and d.Wo > 0:
                if L.p3d_fx_conv_fwd_infer_supported(ctypes.byref(d), 0):
                    e = 0
                elif L.p3d_fx_conv_fwd_infer_any_supported(ctypes.byref(d)):
                    e = 1
            if len(self.entries) > 16:
                self.entries.clear()
            self.entries[x_shape] = e
        return e

    def _job(self, buf, kind, off, bias_off):
        bn = self.bn
        j = FoldJob()
        j.w, j.conv_bias = self.conv.weight.data_ptr(), None
        j.gamma, j.beta, j.mean, j.var, j.eps = bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(), float(bn.eps)
        j.out = buf.data_ptr() + off
        j.bias_out = None if bias_off is None else buf.data_ptr() + bias_off
        j.K, j.C, j.RS, j.c_offset, j.c_total, j.kind = self.k, self.c, self.r * self.r, 0, self.c, kind
        return j

    def jobs(self, buf):
        return [self._job(buf, kind, off, bias_off) for kind, off, bias_off in ((0, self.img_off, self.bias_off), (1, self.w_off, None))]


def _static_ok_half(conv, bn):
    """_static_ok for -half_acc: the fp16 kernels take 8-channel groups, and a conv with fewer than 8 input channels (a stem) has no data-gradient image."""
    if type(conv).__name__ != 'Conv2d' or conv.bias is not None or not isinstance(bn, torch.nn.BatchNorm2d):
        return False
    if not (bn.affine and bn.track_running_stats) or conv.weight.dtype != torch.float32:
        return False
    k, c, r, s = conv.weight.shape
    return c >= 8 and r == s and (r & 1) == 1 and k % 8 == 0 and 8 <= k <= 2048 and bn.num_features == k


def admits_half(x, conv, bn):
    """The admission rule under -half_acc, host only: ops.frozen_fold_half is on, gradients are enabled, x is a 4-d fp16 tensor, the conv is a plain bias-free
    Conv2d with a square odd filter and fp16 weight images including the data gradient's (so not a stem), 8 <= K <= 2048 in multiples of 8, x has the image's
    padded channel count, the BatchNorm is in eval mode with affine parameters and running statistics, and p3d_hconv2d_fwd_infer takes the descriptor."""
    if not (ops.FROZEN_FOLD_HALF and torch.is_grad_enabled() and x.dtype == torch.float16 and x.dim() == 4 and not bn.training and _static_ok_half(conv, bn)):
        return False
    images = getattr(conv, '_h_images', None)
    if images is None or images.crsk is None or x.shape[1] != images.cpad:
        return False
    return _unit(conv, bn, _HUnit).entry(tuple(x.shape)) is not None


class _HUnit(_Unit):
    """A pair of a -half_acc plan: the fp16 forward image [K][RS][Cpad] of w' (fold kind 2), b' (fp32) and the fp16 data-gradient image [Cpad][RS][K] (kind 4)."""
    slot, model_slot = '_hfrozen_unit', '_hfrozen_fold'

    def __init__(self, conv, bn):
        super().__init__(conv, bn)
        self.cpad = ops_half.pad8(self.c)
        self.dimg_off = None

    def layout(self, at):
        self.img_off, self.img_bytes = at, 2 * self.k * self.r * self.r * self.cpad
        self.bias_off = _up(at + self.img_bytes)
        self.dimg_off = _up(self.bias_off + 4 * self.k)
        return _up(self.dimg_off + self.img_bytes)

    def desc(self, x_shape, accumulate=0):
        return ops._desc(x_shape, (self.k, self.cpad, self.r, self.r), self.stride, self.pad, self.dil, accumulate=accumulate)

    def entry(self, x_shape):
        """0: p3d_hconv2d_fwd_infer takes this input shape, None: it does not (host only, remembered per shape)."""
        e = self.entries.get(x_shape, -1)
        if e == -1:
            d = self.desc(x_shape)
            e = 0 if (x_shape[1] == self.cpad and d.Ho > 0 and d.Wo > 0 and lib().p3d_hconv2d_fwd_infer_supported(ctypes.byref(d))) else None
            if len(self.entries) > 16:
                self.entries.clear()
            self.entries[x_shape] = e
        return e

    def jobs(self, buf):
        out = []
        for kind, off, bias_off in ((2, self.img_off, self.bias_off), (4, self.dimg_off, None)):
            j = self._job(buf, kind, off, bias_off)
            j.reserved = self.cpad
            out.append(j)
        return out


class FrozenFold:
    """The plan of a set of conv + BatchNorm pairs: one buffer, one fold launch, folded again lazily (module docstring).  `generation` counts the folds.
    unit: _Unit (fp32) or _HUnit (-half_acc), which decides what the buffer holds per pair."""

    def __init__(self, pairs, unit=None):
        unit = unit or _Unit
        self.units = []
        at = 0
        for conv, bn in pairs:
            u = unit(conv, bn)
            u.plan = self
            at = u.layout(at)
            conv.__dict__[unit.slot] = _Transient(unit=u, bn=bn)
            self.units.append(u)
        self.nbytes = max(at, _ALIGN)
        self.buffer = None
        self.generation = 0
        self.epoch = None
        self._table = None              # (what it was built from, device job table)

    @classmethod
    def of(cls, model, half=False):
        """The plan of a network: every pair of its dense residual blocks, downsample branches included, that the fold can take at all (half: under -half_acc)."""
        from ._trunk import _ResidualBlock
        ok = _static_ok_half if half else _static_ok
        pairs = []
        for blk in model.modules():
            if isinstance(blk, _ResidualBlock) and not blk.partial:
                named = [(getattr(blk, c), getattr(blk, b)) for c, b in blk._chain]
                if blk.downsample is not None:
                    named.append((blk.downsample[0], blk.downsample[1]))
                pairs += [p for p in named if ok(*p)]
        return cls(pairs, _HUnit if half else _Unit)

    def _stale(self, u):
        return (None if u.bn.training else u._key()) != u.seen

    def fresh(self):
        """Fold again if anything the fold read has changed (every pair looked at: the network's once-per-forward check)."""
        if self.epoch != ops.WEIGHT_EPOCH or any(self._stale(u) for u in self.units):
            self.refresh()
        return self

    def refresh(self):
        """Fold every pair whose BatchNorm is frozen from the current parameters and running statistics: one launch.  Moves `generation`."""
        active = [u for u in self.units if not u.bn.training]
        self.generation += 1
        self.epoch = ops.WEIGHT_EPOCH
        for u in self.units:
            u.seen = None
        if not active:
            return self
        device = active[0].conv.weight.device
        for u in active:
            for t in u.tensors():
                if not t.is_cuda or t.dtype != torch.float32 or t.device != device or not t.is_contiguous():
                    raise P3DError('ops_frozen: parameters and running statistics must be contiguous fp32 tensors on one HIP device')
        if self.buffer is None or self.buffer.device != device:
            self.buffer = torch.empty(self.nbytes, dtype=torch.uint8, device=device)
            self._table = None
        ident = tuple(t.data_ptr() for u in active for t in u.tensors())
        if self._table is None or self._table[0] != ident:
            jobs = [j for u in active for j in u.jobs(self.buffer)]
            table = (FoldJob * len(jobs))(*jobs)
            self._table = (ident, torch.frombuffer(bytearray(table), dtype=torch.uint8).to(device), len(jobs))
        _, table, njobs = self._table
        check(lib().p3d_fx_fold_bn_images(ops._p(table), njobs, 64, ops._stream()), 'p3d_fx_fold_bn_images')
        for u in active:
            u.seen = u._key()
        return self

    def at(self, off):
        return ctypes.c_void_p(self.buffer.data_ptr() + off)

    def bias(self, u):
        """b' of a pair as a tensor view of the buffer (tests)."""
        return self.buffer[u.bias_off:u.bias_off + 4 * u.k].view(torch.float32)

    def weight(self, u):
        """The folded fp32 weight w' of a pair as a tensor view of the buffer."""
        return self.buffer[u.w_off:u.w_off + 4 * u.k * u.c * u.r * u.r].view(torch.float32).view(u.k, u.c, u.r, u.r)

    def image(self, u):
        """The fp16 forward image [K][R][S][Cpad] of w' of a -half_acc pair as a tensor view of the buffer."""
        return self.buffer[u.img_off:u.img_off + u.img_bytes].view(torch.float16).view(u.k, u.r, u.r, u.cpad)

    def dgrad_image(self, u):
        """The fp16 data-gradient image [Cpad][R][S][K] of w' of a -half_acc pair as a tensor view of the buffer."""
        return self.buffer[u.dimg_off:u.dimg_off + u.img_bytes].view(torch.float16).view(u.cpad, u.r, u.r, u.k)


def _unit(conv, bn, kind=_Unit):
    """The pair's unit in the plan it belongs to: its network's (prepare) or, used on its own, a plan of this one pair.  kind: _Unit or, under -half_acc, _HUnit."""
    held = conv.__dict__.get(kind.slot)
    if not held or held.get('bn') is not bn:
        FrozenFold([(conv, bn)], kind)
        held = conv.__dict__[kind.slot]
    return held['unit']


def prepare(model, half=False):
    """Forward pre-hook of a network (TrunkBase): with the switch on and gradients enabled, make the network's plan on first use and fold again if it is stale.
    half: the -half_acc plan under its own switch."""
    if not ((ops.FROZEN_FOLD_HALF if half else ops.FROZEN_FOLD) and torch.is_grad_enabled()):
        return
    slot = (_HUnit if half else _Unit).model_slot
    held = model.__dict__.get(slot)
    if not held:
        held = model.__dict__[slot] = _Transient(plan=FrozenFold.of(model, half))
    held['plan'].fresh()


def has_frozen(model):
    """A BatchNorm of `model` is in eval mode (what the switch would fold)."""
    return any(isinstance(m, torch.nn.BatchNorm2d) and not m.training for m in model.modules())


class FrozenConvBnFn(torch.autograd.Function):
    """y = relu?(bn(conv(x)) + res) for a frozen bn on the folded convolution (module docstring); w, gamma, beta are the parameters the gradients belong to,
    `unit` the pair's place in its plan.  join_put / join_take / res_join: ops.GradJoin, as Conv2dFn and BatchNormActFn use them.  With a ReLU the residual's
    gradient IS g, which the weight gradient may still be reading on the second stream when backward returns: a `res` with another consumer must come with the
    join that sums the two (res_join: the block's identity shortcut); without one (the downsample branch's output) g reaches its one reader as it is."""

    @staticmethod
    def forward(ctx, x, res, w, gamma, beta, unit, relu, join_put=None, join_take=None, res_join=None):
        ops._need_gpu(x, res, w, gamma, beta)
        plan = unit.plan
        if unit.seen is None or plan.epoch != ops.WEIGHT_EPOCH or unit._key() != unit.seen:
            # Stale at the layer's own call: a pair used outside a network, or something written between the network's pre-hook and this layer.  The WHOLE plan is
            # folded again (one launch, one generation): forwards of the plan's other pairs that have not run backward yet are then refused there, which is
            # right -- what was written may have been theirs too -- and says so.
            plan.refresh()
        x = x.contiguous()
        res = None if res is None else res.contiguous()
        entry = unit.entry(tuple(x.shape))
        if entry is None:
            raise P3DError('ops_frozen: no folded forward takes a %s input of this %d -> %d convolution (ask ops_frozen.admits first)' % (tuple(x.shape), unit.c, unit.k))
        L, d = lib(), unit.desc(x.shape)
        y = torch.empty((d.N, d.K, d.Ho, d.Wo), dtype=torch.float32, device=x.device)
        if res is not None and res.shape != y.shape:
            raise P3DError('ops_frozen: the residual %s does not match the output %s' % (tuple(res.shape), tuple(y.shape)))
        with ops._Timed('fwd', d):
            if entry == 0:
                ws = ops.workspace(x.device, L.p3d_fx_conv_fwd_infer_workspace_bytes(ctypes.byref(d)))
                check(L.p3d_fx_conv_fwd_infer(ctypes.byref(d), ops._p(x), None, plan.at(unit.img_off), unit.img_bytes, plan.at(unit.bias_off), ops._p(res),
                                              int(bool(relu)), ops._p(y), ops._p(ws), ws.numel(), ops._stream()), 'p3d_fx_conv_fwd_infer')
            else:
                ws = ops.workspace(x.device, L.p3d_fx_conv_fwd_infer_any_workspace_bytes(ctypes.byref(d)))
                check(L.p3d_fx_conv_fwd_infer_any(ctypes.byref(d), ops._p(x), plan.at(unit.img_off), unit.img_bytes, plan.at(unit.bias_off), ops._p(res),
                                                  int(bool(relu)), ops._p(y), ops._p(ws), ws.numel(), ops._stream()), 'p3d_fx_conv_fwd_infer_any')
        ctx.save_for_backward(x, y if relu else None)
        ctx.cfg = (unit, plan.generation, bool(relu), res is not None)
        ctx.params = (w, gamma, beta)
        ctx.joins = (join_put, join_take, res_join)
        return y

    @staticmethod
    def backward(ctx, dy):
        return _backward(ctx, dy, _Fp32)


class _Fp32:
    """What _backward launches for the fp32 node: operands are contiguous fp32 NCHW, w' is the fp32 fold (kind 1) at unit.w_off."""

    @staticmethod
    def operand(t):
        return t.contiguous()

    @staticmethod
    def mask(L, d, dy, y, g, sums, st):
        hw = d.Ho * d.Wo
        ws = ops.workspace(dy.device, L.p3d_frozen_grad_mask_workspace_bytes(d.N, d.K, hw))
        check(L.p3d_frozen_grad_mask(ops._p(dy), ops._p(y), ops._p(g), ops._p(sums), d.N, d.K, hw, ops._p(ws), ws.numel(), st), 'p3d_frozen_grad_mask')

    @staticmethod
    def take(join, x):
        return ops._take(join, x)

    @staticmethod
    def dgrad(L, d, g, unit, dx, st):
        ws = ops.workspace(dx.device, L.p3d_conv2d_dgrad_workspace_bytes(ctypes.byref(d)))
        check(L.p3d_conv2d_dgrad(ctypes.byref(d), ops._p(g), unit.plan.at(unit.w_off), None, None, ops._p(dx), ops._p(ws), ws.numel(), st), 'p3d_conv2d_dgrad')

    @staticmethod
    def wgrad_bytes(L, d):
        return L.p3d_conv2d_wgrad_workspace_bytes(ctypes.byref(d))

    @staticmethod
    def wgrad(L, d, g, x, unit, raw, ws, wbytes, wst):
        check(L.p3d_conv2d_wgrad(ctypes.byref(d), ops._p(g), ops._p(x), None, None, raw, ops._p(ws), wbytes, wst), 'p3d_conv2d_wgrad')


class _Half:
    """What _backward launches for the -half_acc node: operands are fp16 NHWC (channels_last tensors), w' in the data gradient's layout is the kind-4 image at
    unit.dimg_off, and the weight gradient leaves fp32 rows of the conv's real input channels: what p3d_frozen_wgrad_finish takes beside the fp32 master."""

    @staticmethod
    def operand(t):
        return ops_half._cl(t)

    @staticmethod
    def mask(L, d, dy, y, g, sums, st):
        pixels = d.N * d.Ho * d.Wo
        ws = ops.workspace(dy.device, L.p3d_hfrozen_grad_mask_workspace_bytes(pixels, d.K))
        check(L.p3d_hfrozen_grad_mask(ops._p(dy), ops._p(y), ops._p(g), ops._p(sums), pixels, d.K, ops._p(ws), ws.numel(), st), 'p3d_hfrozen_grad_mask')

    @staticmethod
    def take(join, x):
        return ops_half._cl(ops._take(join, x))

    @staticmethod
    def dgrad(L, d, g, unit, dx, st):
        check(L.p3d_hconv2d_dgrad(ctypes.byref(d), ops._p(g), unit.plan.at(unit.dimg_off), None, ops._p(dx), st), 'p3d_hconv2d_dgrad')

    @staticmethod
    def wgrad_bytes(L, d):
        return L.p3d_hconv2d_wgrad_workspace_bytes(ctypes.byref(d))

    @staticmethod
    def wgrad(L, d, g, x, unit, raw, ws, wbytes, wst):
        check(L.p3d_hconv2d_wgrad(ctypes.byref(d), ops._p(g), ops._p(x), None, raw, unit.c, 1.0, ops._p(ws), wbytes, wst), 'p3d_hconv2d_wgrad')


def _backward(ctx, dy, kn):
    """The backward of both nodes (FrozenConvBnFn, HFrozenConvBnFn): the stream and join rules stand here once, `kn` (_Fp32 / _Half) names the launches."""
    x, y = ctx.saved_tensors
    unit, generation, relu, has_res = ctx.cfg
    join_put, join_take, res_join = ctx.joins
    plan, bn = unit.plan, unit.bn
    if plan.generation != generation:
        raise P3DError('ops_frozen: the fold this forward ran on has been replaced (parameters or running statistics changed between forward and backward); '
                       'run the forward again')
    dy = kn.operand(dy)
    d = unit.desc(x.shape)
    L, st = lib(), ops._stream()
    need_w = any(ctx.needs_input_grad[2:5])
    # the mask pass: g and its per-channel sums (dbeta); without a ReLU dy itself is g and only the sums are made
    sums = torch.empty(d.K, dtype=torch.float32, device=x.device)
    g = torch.empty_like(dy) if relu else dy
    kn.mask(L, d, dy, y if relu else None, g if relu else None, sums, st)
    g_ready = ops._mark_ready() if (ops.WGRAD_STREAM and need_w) else None      # g and the sums are final here: the weight-gradient stream waits for this
    dx = dres = dw = dgamma = dbeta = None
    if join_take is not None:
        join_take.taken = True
    if ctx.needs_input_grad[0]:
        if join_take is not None and join_take.buf is not None:
            dx = kn.take(join_take, x)
            d.accumulate = 1
        else:
            dx = torch.empty_like(x)
        with ops._Timed('dgrad', d):
            kn.dgrad(L, d, g, unit, dx, st)
        if ops._stash(join_put, dx):
            dx = None
    side = grads = None
    if need_w:
        w, gamma, beta = ctx.params
        grads = ops._GradOut(w, gamma, beta)
        d.accumulate = 0                                # raw is scratch, overwritten; the finish kernel does the accumulating
        wbytes = _up(kn.wgrad_bytes(L, d))
        side, wst, ws = ops._side_launch(x.device, grads.direct, wbytes + 4 * w.numel(), g_ready)
        raw = ctypes.c_void_p(ws.data_ptr() + wbytes)   # (the scratch is the stream's own: the next launch there comes behind the finish kernel)
        with ops._Timed('wgrad', d, side):              # (the finishing kernel is part of this layer's weight-gradient pass)
            kn.wgrad(L, d, g, x, unit, raw, ws, wbytes, wst)
            check(L.p3d_frozen_wgrad_finish(raw, ops._p(w), ops._p(gamma), ops._p(bn.running_mean), ops._p(bn.running_var), float(bn.eps), ops._p(sums),
                                            ops._p(grads.bufs[0]), ops._p(grads.bufs[1]), ops._p(grads.bufs[2]), d.K, unit.c * d.R * d.S, int(grads.direct), wst),
                  'p3d_frozen_wgrad_finish')
        ops._side_launched(side, (g, x, sums))
    if has_res and ctx.needs_input_grad[1]:
        # dres IS g (with a ReLU) or dy itself (without), and the weight gradient may still be reading it on the second stream when backward returns, while
        # whoever gets it next may write it: a join's consumer accumulates its data gradient into a stashed buffer, and autograd adds a second gradient of
        # the same tensor onto the first in place.  So the buffer leaves with an event behind its readers there: on the join when it is stashed (the consumer
        # waits, several nodes later), else -- a join whose consumer has run, and every gradient without a ReLU, which is never stashed -- waited for here.
        dres = g
        after = None
        if side is not None and (res_join is not None or not relu):       # (a ReLU layer without a join: the downsample branch's output, one reader)
            after = _after_event(res_join if relu else None)
            after.record(side)
        if relu and ops._stash(res_join, g, after):     # (without a ReLU dres aliases dy: never hand that out)
            dres = None
        elif after is not None:
            torch.cuda.current_stream(x.device).wait_event(after)
    if grads is not None:
        dw, dgamma, dbeta = grads.done()                # last: behind the launches, _side_launched and the event of the join
    return dx, dres, dw, dgamma, dbeta, None, None, None, None, None


_after_ring, _after_next = [], [0]          # [event, weak reference to the join it was last left on]


def _after_event(join):
    """A recycled event (ops._mark_ready's reason: creating one costs host time) to record behind the second stream's readers of a residual gradient.  Unlike
    _mark_ready's, the wait may come several nodes later (the consumer of `join`), so a slot is taken again only once the join it was left on has been consumed:
    64 slots outlast the open joins of any backward pass here (one per residual block at the most), and anything else raises."""
    import weakref
    if len(_after_ring) < 64:
        _after_ring.append([torch.cuda.Event(), None])
    slot = _after_ring[_after_next[0] % len(_after_ring)]
    _after_next[0] += 1
    holder = slot[1]() if slot[1] is not None else None
    if holder is not None and holder.after is slot[0]:
        raise P3DError('ops_frozen: more than %d residual gradients are waiting for their joins at once' % len(_after_ring))
    slot[1] = weakref.ref(join) if join is not None else None
    return slot[0]


def conv_bn(x, conv, bn, res=None, relu=False, join_put=None, join_take=None, res_join=None):
    """relu?(bn(conv(x)) + res) for a pair `admits` has taken."""
    return FrozenConvBnFn.apply(x, res, conv.weight, bn.weight, bn.bias, _unit(conv, bn), relu, join_put, join_take, res_join)


class HFrozenConvBnFn(torch.autograd.Function):
    """FrozenConvBnFn under -half_acc: y = relu?(conv(x, w') + b' (+ res)) on fp16 NHWC tensors, one p3d_hconv2d_fwd_infer launch on the plan's kind-2 image, rounded
    to fp16 once; saved for backward are x and, with a ReLU, y.  w, gamma, beta are the fp32 masters the gradients belong to, `unit` an _HUnit.  The joins, the
    streams and the residual gradient follow FrozenConvBnFn's rules (_backward)."""

    @staticmethod
    def forward(ctx, x, res, w, gamma, beta, unit, relu, join_put=None, join_take=None, res_join=None):
        ops_half._need_half(x, res)
        ops._need_gpu(w, gamma, beta)
        plan = unit.plan
        if unit.seen is None or plan.epoch != ops.WEIGHT_EPOCH or unit._key() != unit.seen:
            plan.refresh()                                  # stale at the layer's own call: the whole plan is folded again (FrozenConvBnFn.forward)
        x = ops_half._cl(x)
        res = None if res is None else ops_half._cl(res)
        if unit.entry(tuple(x.shape)) is None:
            raise P3DError('ops_frozen: p3d_hconv2d_fwd_infer does not take a %s input of this %d -> %d convolution (ask ops_frozen.admits_half first)'
                           % (tuple(x.shape), unit.c, unit.k))
        d = unit.desc(x.shape)
        y = ops_half._empty(d.N, d.K, d.Ho, d.Wo, x.device)
        if res is not None and res.shape != y.shape:
            raise P3DError('ops_frozen: the residual %s does not match the output %s' % (tuple(res.shape), tuple(y.shape)))
        with ops._Timed('fwd', d):
            check(lib().p3d_hconv2d_fwd_infer(ctypes.byref(d), ops._p(x), plan.at(unit.img_off), plan.at(unit.bias_off), None, None, ops._p(res), int(bool(relu)),
                                              ops._p(y), ops._stream()), 'p3d_hconv2d_fwd_infer')
        ctx.save_for_backward(x, y if relu else None)
        ctx.cfg = (unit, plan.generation, bool(relu), res is not None)
        ctx.params = (w, gamma, beta)
        ctx.joins = (join_put, join_take, res_join)
        return y

    @staticmethod
    def backward(ctx, dy):
        return _backward(ctx, dy, _Half)


def conv_bn_half(x, conv, bn, res=None, relu=False, join_put=None, join_take=None, res_join=None):
    """relu?(bn(conv(x)) + res) on fp16 NHWC tensors for a pair `admits_half` has taken."""
    return HFrozenConvBnFn.apply(x, res, conv.weight, bn.weight, bn.bias, _unit(conv, bn, _HUnit), relu, join_put, join_take, res_join)
