"""Fast inference forward with eval-mode BatchNorm folded into the x3 convolutions (csrc/p3d_fx.hip).

An eval-mode BatchNorm is a per-channel affine map, so behind a convolution it folds into the weights and a bias:
s = gamma / sqrt(var + eps), w' = w * s, b' = beta - mean * s (+ s * conv bias).  `fold(model)` builds the forward weight image of every w'
and every b' in ONE device buffer (p3d_fx_fold_bn_images: one launch for the whole network); `FoldedNet(x[, y])` then runs the network on
p3d_fx_conv_fwd_infer, whose epilogue adds b', the residual and the ReLU, and on p3d_stem_fwd + p3d_stem_tail_infer for the 7x7 stem.

    net = infer.fold(model.eval())      # depthnet / resnet (legacy) / fusionnet / partial_depthnet / partial_fusionnet
    z, feat = net(x)                    # what model.eval()(x) returns, under no_grad
    ...optimizer step / new running statistics...
    net.refresh()                       # re-fold from the current parameters (one launch)

A conv the x3 forward cannot take (odd sizes, fx_fwd_applies) goes through today's eval path for that layer (ops.conv_bn_eval).

The partial-convolution layers of partial_depthnet (stem, layer1, layer2) and partial_fusionnet (conv2, layer5, layer6) fold as well: each conv runs on
p3d_fx_conv_fwd_infer_masked (mask_in multiplied into the operand, y = relu?(conv * mult + b' + res), the factor before b'), each with its own
ops.mask_count, and the PartialConv stem on p3d_stem_image_masked + p3d_stem_fwd_masked (x mult) + p3d_stem_tail_infer.  A partial conv with a bias, a shape
the masked entry refuses or a stem p3d_stem_masked_supported refuses (odd sides) runs as the model's own module, that layer only.  P3D_FOLD_PARTIAL=0
(read when a network is folded) keeps every partial layer on the model's own modules, as before they folded.

`fold_half(model)` is the same for the fp16 (-half_acc) network: kind-2 fold jobs write fp16 [K][R][S][Cpad] images of every w' (the layout
p3d_weight_images_f16 produces) and `HalfFoldedNet(x[, y])` runs every conv on p3d_hconv2d_fwd_infer, whose epilogue adds b', the residual and the
ReLU before the one rounding to fp16.  The partial-convolution layers fold too (mask_in in the operand fetch, mult in the epilogue), so an fp16 folded
forward has no BatchNorm pass at all.
"""
import ctypes
import os

import torch

from . import ops, ops_block, ops_half
from ._lib import FoldJob, P3DError, check, lib
from .nn import _one

# Narrow layers (64 output channels): feed the activation as a pre-split image (p3d_fx_act_image + the 64-row fx16 tile) instead of the fp32 operand on
# the 128-row tile (half of it padding).  DESIGN.md records the measurement behind the default.
NARROW_IMAGE = os.environ.get('P3D_FOLD_NARROW_IMG', '0') != '0'
_ALIGN = 256


def fold_partial():
    """P3D_FOLD_PARTIAL=0: FoldedNet leaves the partial-convolution stems and layers on the model's own modules (A/B; read when a network is folded)."""
    return os.environ.get('P3D_FOLD_PARTIAL', '1') != '0'


def enabled():
    """P3D_FOLDED_EVAL=1: Trainer.test and the distillation teacher evaluate through a FoldedNet."""
    return os.environ.get('P3D_FOLDED_EVAL', '0') == '1'


def half_enabled():
    """P3D_FOLDED_EVAL_HALF=1: under -half_acc, Trainer.test and the distillation teacher evaluate through a HalfFoldedNet."""
    return os.environ.get('P3D_FOLDED_EVAL_HALF', '0') == '1'


def _family(model):
    name = type(model).__module__.rsplit('.', 1)[-1]
    if name not in ('depthnet', 'resnet', 'fusionnet', 'partial_depthnet', 'partial_fusionnet'):
        raise P3DError('infer.fold: unknown network family %s.%s' % (type(model).__module__, type(model).__name__))
    return name


def _check_foldable(model):
    if getattr(model, '_p3d_half', False):
        raise P3DError('infer.fold: a -half_acc (fp16) model cannot be folded onto the fp32 kernels; use infer.fold_half')
    for name, m in model.named_modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            if m.training:
                raise P3DError('infer.fold: BatchNorm %r is in training mode; call model.eval() first (folding uses the running statistics)' % name)
            if not (m.affine and m.track_running_stats):
                raise P3DError('infer.fold: BatchNorm %r has no running statistics / affine parameters' % name)
    for p in model.parameters():
        if not p.is_cuda or p.dtype != torch.float32:
            raise P3DError('infer.fold: parameters must be fp32 on the HIP device')


class _Conv:
    """One conv (+ BatchNorm) of the folded network: where its image and bias live in the buffer, and how to run it."""

    def __init__(self, conv, bn, c_offset=0, c_count=None, has_bias=True):
        from .partial_conv import PartialConv
        self.conv, self.bn = conv, bn
        k, ct, r, s = conv.weight.shape
        self.k, self.ct, self.rs, self.r = k, ct, r * s, r
        self.c_offset, self.c = c_offset, ct if c_count is None else c_count
        self.stride, self.pad, self.dil = _one(conv.stride), _one(conv.padding), _one(conv.dilation)
        self.has_bias = has_bias
        self.partial = isinstance(conv, PartialConv)
        self.foldable = self.c % 16 == 0 and r == s and (r & 1) == 1 and k % 16 == 0 and 32 <= k <= 2048      # (else: today's path)
        if self.partial and conv.bias is not None:          # (no reference network has one: the module's own path)
            self.foldable = False
        self.img_off = self.img_bytes = self.bias_off = None

    def layout(self, at):
        if not self.foldable:
            return at
        fb = ctypes.c_size_t()
        check(lib().p3d_fx_weight_image_bytes(self.k, self.c, self.rs, ctypes.byref(fb), None), 'p3d_fx_weight_image_bytes')
        self.img_off, self.img_bytes = at, fb.value
        at = _up(at + fb.value)
        if self.has_bias:
            self.bias_off = at
            at = _up(at + 4 * self.k)
        return at

    def job(self, buf):
        if not self.foldable:
            return None
        j = FoldJob()
        j.w = self.conv.weight.data_ptr()
        j.conv_bias = self.conv.bias.data_ptr() if self.conv.bias is not None else None
        if self.bn is not None:
            j.gamma, j.beta = self.bn.weight.data_ptr(), self.bn.bias.data_ptr()
            j.mean, j.var = self.bn.running_mean.data_ptr(), self.bn.running_var.data_ptr()
            j.eps = float(self.bn.eps)
        j.out = buf.data_ptr() + self.img_off
        j.bias_out = buf.data_ptr() + self.bias_off if self.bias_off is not None else None
        j.K, j.C, j.RS, j.c_offset, j.c_total, j.kind = self.k, self.c, self.rs, self.c_offset, self.ct, 0
        return j

    def desc(self, x, accumulate=0):
        return ops._desc(x.shape, (self.k, self.c, int(self.rs ** 0.5), int(self.rs ** 0.5)), self.stride, self.pad, self.dil, accumulate=accumulate)


def _up(v):
    return (v + _ALIGN - 1) // _ALIGN * _ALIGN


class _Stem:
    """The 7x7 stride-2 stem + BatchNorm + ReLU + max pool: folded fp32 weights (kind 1) -> p3d_stem_weight_image -> p3d_stem_fwd -> p3d_stem_tail_infer."""

    def __init__(self, conv, bn):
        self.conv, self.bn = conv, bn
        self.k, self.cin = conv.weight.shape[0], conv.weight.shape[1]
        self.masked = type(conv).__name__ == 'PartialConv'      # the partial families' stems: mask_in into the image, mult into the epilogue
        self.foldable = (type(conv).__name__ in ('Conv2d', 'PartialConv') and conv.bias is None and tuple(conv.kernel_size) == (7, 7) and _one(conv.stride) == 2
                         and _one(conv.padding) == 3 and _one(conv.dilation) == 1 and 1 <= self.cin <= 4 and self.k % 16 == 0 and self.k <= 128)

    def layout(self, at):
        if not self.foldable:
            return at
        self.w_off = at
        at = _up(at + 4 * self.k * self.cin * 49)
        self.img_off = at
        at = _up(at + lib().p3d_stem_weight_image_bytes(self.k))
        self.bias_off = at
        return _up(at + 4 * self.k)

    def job(self, buf):
        if not self.foldable:
            return None
        j = FoldJob()
        j.w = self.conv.weight.data_ptr()
        j.gamma, j.beta = self.bn.weight.data_ptr(), self.bn.bias.data_ptr()
        j.mean, j.var = self.bn.running_mean.data_ptr(), self.bn.running_var.data_ptr()
        j.eps = float(self.bn.eps)
        j.out = buf.data_ptr() + self.w_off
        j.bias_out = buf.data_ptr() + self.bias_off
        j.K, j.C, j.RS, j.c_offset, j.c_total, j.kind = self.k, self.cin, 49, 0, self.cin, 1
        return j


class _Folded:
    """One device buffer with the folded images and biases of `stems` and `convs`, one workspace, and the conv launcher."""

    def _allocate(self, device):
        at = 0
        for st in self.stems.values():
            at = st.layout(at)
        for c in self.convs:
            at = c.layout(at)
        self.buffer = torch.empty(max(at, _ALIGN), dtype=torch.uint8, device=device)
        self.workspace = torch.empty(1 << 20, dtype=torch.uint8, device=device)
        self.refresh()

    def _check(self):
        _check_foldable(self.model)

    # ---- folding ------------------------------------------------------------------------------------------------
    def refresh(self):
        """Re-fold every conv from the current parameters and running statistics: one fold launch (+ the stem's image restatement)."""
        self._check()
        jobs = [j for j in [st.job(self.buffer) for st in self.stems.values()] + [c.job(self.buffer) for c in self.convs] if j is not None]
        if not jobs:
            return self
        table = (FoldJob * len(jobs))(*jobs)
        host = torch.frombuffer(bytearray(table), dtype=torch.uint8)
        self._jobs = host.to(self.buffer.device)           # (kept alive until the launch has read it: the next refresh replaces it in stream order)
        L, st = lib(), ops._stream()
        check(L.p3d_fx_fold_bn_images(ops._p(self._jobs), len(jobs), 64, st), 'p3d_fx_fold_bn_images')
        for s in self.stems.values():
            if s.foldable:
                ws = self._ws(s.k * 256 * 4)
                check(L.p3d_stem_weight_image(self._at(s.w_off), s.k, s.cin, self._at(s.img_off), ops._p(ws), ws.numel(), st), 'p3d_stem_weight_image')
        return self

    def _at(self, off):
        return ctypes.c_void_p(self.buffer.data_ptr() + off)

    def _ws(self, nbytes):
        if self.workspace.numel() < nbytes:
            self.workspace = torch.empty(int(nbytes), dtype=torch.uint8, device=self.buffer.device)
        return self.workspace

    def bias(self, c):
        """b' of a folded conv as a tensor view of the buffer (tests)."""
        return self.buffer[c.bias_off:c.bias_off + 4 * c.k].view(torch.float32)

    def image(self, c):
        """The folded forward weight image of a conv (tests)."""
        return self.buffer[c.img_off:c.img_off + c.img_bytes]

    def _conv(self, c, x, res=None, relu=False, out=None, accumulate=0, bias=True):
        """y = conv(x, w') + b' (+ out) (+ res) (then ReLU) on the folded image; None when the x3 forward cannot take the conv."""
        L = lib()
        d = c.desc(x, accumulate) if c.foldable else None
        image_fed = NARROW_IMAGE and c.k <= 64
        if d is None or not L.p3d_fx_conv_fwd_infer_supported(ctypes.byref(d), int(image_fed)):
            return None
        x = x.contiguous()
        y = out if out is not None else torch.empty((d.N, d.K, d.Ho, d.Wo), dtype=torch.float32, device=x.device)
        x_img = ops.act_image(x) if image_fed else None
        ws = self._ws(L.p3d_fx_conv_fwd_infer_workspace_bytes(ctypes.byref(d)))
        check(L.p3d_fx_conv_fwd_infer(ctypes.byref(d), None if image_fed else ops._p(x), ops._p(x_img), self._at(c.img_off), c.img_bytes,
                                      self._at(c.bias_off) if (bias and c.bias_off is not None) else None, ops._p(None if res is None else res.contiguous()),
                                      int(bool(relu)), ops._p(y), ops._p(ws), ws.numel(), ops._stream()), 'p3d_fx_conv_fwd_infer')
        return y

    def _conv_bn(self, c, x, res=None, relu=False):
        y = self._conv(c, x, res, relu)
        if y is None:                                       # per-layer fallback: today's fused eval kernel
            y = ops.conv_bn_eval(x, c.conv, c.bn, res=res, relu=relu)
        return y

    def _pconv(self, c, x, veil, res=None, relu=True):
        """A partial convolution (partial_conv.py) + its folded BatchNorm: y = relu?(conv(x * veil, w') * mult + b' + res), mult and mask_out from the box count
        of veil (ops.mask_count); returns (y, mask_out).  A conv the masked entry cannot take runs as the module, then the eval-mode BatchNorm pass."""
        L = lib()
        d = c.desc(x) if c.foldable else None
        if d is None or not L.p3d_fx_conv_fwd_infer_masked_supported(ctypes.byref(d)):
            y, mask_out = c.conv(x, veil)
            return c.bn(y, res=res, relu=relu), mask_out
        if tuple(veil.shape) != (d.N, 1, d.H, d.W) or veil.dtype != torch.float32:
            raise P3DError('infer: the validity mask of a partial conv must be fp32 [N, 1, H, W] like its input, got %s %s' % (tuple(veil.shape), veil.dtype))
        mult, mask_out = ops.mask_count(veil, c.r, c.stride, c.pad, c.dil)
        x = x.contiguous()
        y = torch.empty((d.N, d.K, d.Ho, d.Wo), dtype=torch.float32, device=x.device)
        ws = self._ws(L.p3d_fx_conv_fwd_infer_workspace_bytes(ctypes.byref(d)))
        check(L.p3d_fx_conv_fwd_infer_masked(ctypes.byref(d), ops._p(x), self._at(c.img_off), c.img_bytes, self._at(c.bias_off), ops._p(veil.contiguous()),
                                             ops._p(mult), ops._p(None if res is None else res.contiguous()), int(bool(relu)), ops._p(y), ops._p(ws), ws.numel(),
                                             ops._stream()), 'p3d_fx_conv_fwd_infer_masked')
        return y, mask_out


class FoldedConv(_Folded):
    """One conv (no bias) + eval-mode BatchNorm, folded: FoldedConv(conv, bn)(x, res=None, relu=False) = relu(bn(conv(x)) + res).  For a PartialConv
    the validity mask comes along: FoldedConv(pconv, bn)(x, res, relu, veil=mask_in) = (relu(bn(pconv(x, mask_in)[0]) + res), mask_out)."""

    def __init__(self, conv, bn):
        self.model, self.stems = None, {}
        self.conv = _Conv(conv, bn)
        self.convs = [self.conv]
        self._allocate(conv.weight.device)

    def _check(self):
        if self.conv.bn.training:
            raise P3DError('infer.FoldedConv: the BatchNorm is in training mode')

    def __call__(self, x, res=None, relu=False, veil=None):
        if self.conv.partial != (veil is not None):
            raise P3DError('infer.FoldedConv: a partial convolution takes its validity mask (veil=), a dense one none')
        with torch.no_grad():
            return self._pconv(self.conv, x, veil, res, relu) if self.conv.partial else self._conv_bn(self.conv, x, res, relu)


class FoldedNet(_Folded):
    """model.eval()'s forward with every BatchNorm folded into its convolution.  Holds one device buffer with every weight image and bias, and one
    workspace.  Parameters and running statistics are read at fold / refresh() time only (the per-layer fallbacks read them live)."""

    def __init__(self, model):
        _check_foldable(model)
        self.model = model
        self.family = _family(model)
        self.device = next(model.parameters()).device
        self.skip_relu = bool(getattr(model, 'skip_relu', False))
        self.early_dist = bool(getattr(model, 'early_dist', False))
        self.stems, self.convs = {}, []
        fam = self.family
        self.fold_partial = fold_partial()
        partial = {'partial_depthnet': ('layer1', 'layer2'), 'partial_fusionnet': ('layer5', 'layer6')}.get(fam, ()) if self.fold_partial else ()
        if fam != 'partial_depthnet' or self.fold_partial:
            self.stems['conv1'] = _Stem(model.conv1, model.bn1)
        if fam == 'fusionnet' or (fam == 'partial_fusionnet' and self.fold_partial):
            self.stems['conv2'] = _Stem(model.conv2, model.bn2)
        dense = {'depthnet': ('layer1', 'layer2', 'layer3', 'layer4'), 'resnet': ('layer1', 'layer2', 'layer3', 'layer4'),
                 'fusionnet': ('layer1', 'layer2', 'layer3', 'layer4', 'layer5', 'layer6'), 'partial_depthnet': ('layer3', 'layer4'),
                 'partial_fusionnet': ('layer1', 'layer2', 'layer3', 'layer4')}[fam]
        self.blocks = {}
        for lname in dense + partial:
            plans = []
            for blk in getattr(model, lname):
                plan = dict(block=blk, chain=[self._add(_Conv(getattr(blk, c), getattr(blk, b))) for c, b in blk._chain])
                plan['ds'] = self._add(_Conv(blk.downsample[0], blk.downsample[1])) if blk.downsample is not None else None
                plans.append(plan)
            self.blocks[lname] = plans
        if fam in ('fusionnet', 'partial_fusionnet'):
            f = model.fusion
            half = f.conv.weight.shape[1] // 2
            self.fusion = (self._add(_Conv(f.conv, f.bn, 0, half, has_bias=False)), self._add(_Conv(f.conv, f.bn, half, half)))
        heads = ('cam_regressor', 'mat_regressor') if fam == 'resnet' else ('regressor',)
        self.heads = [self._add(_Conv(getattr(model, h), None)) if getattr(model, h, None) is not None else None for h in heads]
        self._allocate(self.device)

    def _add(self, c):
        self.convs.append(c)
        return c

    # ---- forward ---------------------------------------------------------------------------------------------------
    def _stem(self, s, x):
        n, cin, h, w = x.shape
        L = lib()
        if not (s.foldable and not s.masked and x.is_cuda and x.dtype == torch.float32 and cin == s.cin and L.p3d_stem_supported(n, cin, h, w, s.k)
                and (h // 2) % 2 == 0 and (w // 2) % 4 == 0):
            from ._trunk import stem
            return stem(s.conv, s.bn, self.model.maxpool, x)
        x = x.contiguous()
        st = ops._stream()
        x_img = torch.empty(L.p3d_stem_image_bytes(n, h, w), dtype=torch.uint8, device=x.device)
        check(L.p3d_stem_image(ops._p(x), ops._p(x_img), n, cin, h, w, st), 'p3d_stem_image')
        c = torch.empty((n, s.k, h // 2, w // 2), dtype=torch.float32, device=x.device)
        check(L.p3d_stem_fwd(ops._p(x_img), self._at(s.img_off), ops._p(c), n, cin, h, w, s.k, st), 'p3d_stem_fwd')
        y = torch.empty((n, s.k, h // 4, w // 4), dtype=torch.float32, device=x.device)
        check(L.p3d_stem_tail_infer(ops._p(c), self._at(s.bias_off), ops._p(y), n, s.k, h // 2, w // 2, st), 'p3d_stem_tail_infer')
        return y

    def _stem_masked(self, s, x, veil):
        """The PartialConv stem + BatchNorm + ReLU + max pool (partial_depthnet.py:177): conv(x * veil) * mult on the restated stem, then relu(maxpool(.) + b')
        (relu(maxpool(c mult) + b') = maxpool(relu(c mult + b')): both monotone per channel).  Returns (y, max-pooled mask_out)."""
        n, cin, h, w = x.shape
        L = lib()
        if not (s.foldable and ops_block.MASKED_STEM and x.is_cuda and x.dtype == torch.float32 and cin == s.cin and L.p3d_stem_masked_supported(n, cin, h, w, s.k)
                and (h // 2) % 2 == 0 and (w // 2) % 4 == 0):
            from ._trunk import stem_tail
            c, veil = s.conv(x, veil)                       # today's path (odd sides: the reference's default -side_in 257)
            return stem_tail(s.bn, self.model.maxpool, c), self.model.maxpool(veil)
        x, veil = x.contiguous(), veil.contiguous()
        mult, mask_out = ops.mask_count(veil, 7, 2, 3, 1)
        st = ops._stream()
        x_img = torch.empty(L.p3d_stem_image_bytes(n, h, w), dtype=torch.uint8, device=x.device)
        check(L.p3d_stem_image_masked(ops._p(x), ops._p(veil), ops._p(x_img), n, cin, h, w, st), 'p3d_stem_image_masked')
        c = torch.empty((n, s.k, h // 2, w // 2), dtype=torch.float32, device=x.device)
        check(L.p3d_stem_fwd_masked(ops._p(x_img), self._at(s.img_off), ops._p(c), ops._p(mult), n, cin, h, w, s.k, st), 'p3d_stem_fwd_masked')
        y = torch.empty((n, s.k, h // 4, w // 4), dtype=torch.float32, device=x.device)
        check(L.p3d_stem_tail_infer(ops._p(c), self._at(s.bias_off), ops._p(y), n, s.k, h // 2, w // 2, st), 'p3d_stem_tail_infer')
        return y, self.model.maxpool(mask_out)

    def _layer(self, name, x, veil=None):
        for plan in self.blocks[name]:
            blk = plan['block']
            res = x if plan['ds'] is None else self._conv_bn(plan['ds'], x)
            out = x
            last = len(plan['chain']) - 1
            for i, c in enumerate(plan['chain']):
                if blk.partial:                             # (the closing ReLU of a partial block is unconditional: _trunk.py forward_partial)
                    out, veil = self._pconv(c, out, veil, res if i == last else None)
                else:
                    out = self._conv_bn(c, out, relu=True) if i < last else self._conv_bn(c, out, res=res, relu=not blk.skip_relu)
            x = out
        return x if veil is None else (x, veil)

    def _fusion(self, x, y):
        a, b = self.fusion
        out = self._conv(a, x, bias=False)
        if out is not None:
            out2 = self._conv(b, y, relu=True, out=out, accumulate=1)
            if out2 is not None:
                return out2
        return self.model.fusion(x, y)                      # today's path (two windowed convs, then BatchNorm + ReLU)

    def _head(self, c, x):
        y = self._conv(c, x)
        return c.conv(x) if y is None else y

    def __call__(self, x, y=None):
        with torch.no_grad():
            return self._forward(x, y)

    def _forward(self, x, y):
        m, fam = self.model, self.family
        relu = ops.relu
        if fam == 'depthnet':
            x = self._stem(self.stems['conv1'], x)
            x = self._layer('layer2', self._layer('layer1', x))
            a = self._layer('layer3', x)
            n = self._layer('layer4', relu(a) if self.skip_relu else a)
            z = self._head(self.heads[0], relu(n) if self.skip_relu else n)
            return z, (a if self.early_dist else n)
        if fam == 'resnet':
            x = self._stem(self.stems['conv1'], x)
            for name in ('layer1', 'layer2', 'layer3', 'layer4'):
                x = self._layer(name, x)
            if self.heads[1] is not None:
                return self._head(self.heads[0], x), self._head(self.heads[1], x)
            return self._head(self.heads[0], x)
        if fam == 'fusionnet':
            x = self._stem(self.stems['conv1'], x)
            y = self._stem(self.stems['conv2'], y)
            x = self._layer('layer2', self._layer('layer1', x))
            y = self._layer('layer6', self._layer('layer5', y))
            x = self._fusion(x, y)
            a = self._layer('layer3', x)
            n = self._layer('layer4', relu(a) if self.skip_relu else a)
            z = self._head(self.heads[0], relu(n) if self.skip_relu else n)
            return z, (a if self.early_dist else n)
        from ._trunk import stem_tail
        if fam == 'partial_depthnet':
            veil = ops.nonzero_mask(x)
            if self.fold_partial:
                x, veil = self._stem_masked(self.stems['conv1'], x, veil)
                x, veil = self._layer('layer1', x, veil)
                x, _ = self._layer('layer2', x, veil)       # (layer2's mask_out feeds nothing)
            else:
                x, veil = m.conv1(x, veil)                  # P3D_FOLD_PARTIAL=0: the partial-convolution stem and layers on the model's own eval path
                x = stem_tail(m.bn1, m.maxpool, x)
                veil = m.maxpool(veil)
                x, veil = m.layer1((x, veil))
                x, veil = m.layer2((x, veil))
            x = self._layer('layer4', self._layer('layer3', x))
            return self._head(self.heads[0], x), x
        # partial_fusionnet
        x = self._stem(self.stems['conv1'], x)
        veil = ops.nonzero_mask(y)
        if self.fold_partial:
            y, veil = self._stem_masked(self.stems['conv2'], y, veil)
            x = self._layer('layer2', self._layer('layer1', x))
            y, veil = self._layer('layer5', y, veil)
            y, _ = self._layer('layer6', y, veil)
        else:
            y, veil = m.conv2(y, veil)
            y = stem_tail(m.bn2, m.maxpool, y)
            veil = m.maxpool(veil)
            x = self._layer('layer2', self._layer('layer1', x))
            y, veil = m.layer5((y, veil))
            y, veil = m.layer6((y, veil))
        x = self._fusion(x, y)
        x = self._layer('layer4', self._layer('layer3', x))
        return self._head(self.heads[0], x), x


def fold(model):
    """FoldedNet of a network in eval mode (every BatchNorm frozen); raises P3DError for a BatchNorm in training mode or a -half_acc model."""
    model = getattr(model, 'module', model)
    _check_foldable(model)
    return FoldedNet(model)


# ---- -half_acc: BatchNorm folded into the fp16 convolutions ------------------------------------------------------------------------------
def _check_half_foldable(model):
    for name, m in model.named_modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            if m.training:
                raise P3DError('infer.fold_half: BatchNorm %r is in training mode; call model.eval() first (folding uses the running statistics)' % name)
            if not (m.affine and m.track_running_stats):
                raise P3DError('infer.fold_half: BatchNorm %r has no running statistics / affine parameters' % name)
    for p in model.parameters():
        if not p.is_cuda or p.dtype != torch.float32:
            raise P3DError('infer.fold_half: parameters must be fp32 masters on the HIP device')


class _HConv:
    """One conv (+ BatchNorm) of the fp16 folded network: its fp16 image [K][R][S][Cpad] and b' in the buffer (fold kind 2).  A head whose K is not a
    multiple of 8 (the 17-channel mat_regressor of -joint_space) runs with its image and bias padded to Kpad rows of zeros; its result is the first K channels."""

    def __init__(self, conv, bn):
        from .partial_conv import PartialConv
        self.conv, self.bn = conv, bn
        k, c, r, s = conv.weight.shape
        self.k, self.kpad, self.c, self.cpad, self.r, self.s = k, ops_half.pad8(k), c, ops_half.pad8(c), r, s
        self.stride, self.pad, self.dil = _one(conv.stride), _one(conv.padding), _one(conv.dilation)
        self.partial = isinstance(conv, PartialConv)
        self.foldable = k <= 2048                           # (the fold kernel's per-job scale table; else: today's fp16 path for this layer)
        self.images = None                                  # fp16 images of the unfolded weight, for that path only
        self.img_off = self.bias_off = None

    def layout(self, at):
        if not self.foldable:
            return at
        self.img_off = at
        at = _up(at + 2 * self.kpad * self.r * self.s * self.cpad)           # (rows K .. Kpad - 1 stay zero: the buffer is zeroed once, the fold writes K rows)
        self.bias_off = at
        return _up(at + 4 * self.kpad)

    def job(self, buf):
        if not self.foldable:
            return None
        j = FoldJob()
        j.w = self.conv.weight.data_ptr()
        j.conv_bias = self.conv.bias.data_ptr() if self.conv.bias is not None else None
        if self.bn is not None:
            j.gamma, j.beta = self.bn.weight.data_ptr(), self.bn.bias.data_ptr()
            j.mean, j.var = self.bn.running_mean.data_ptr(), self.bn.running_var.data_ptr()
            j.eps = float(self.bn.eps)
        j.out = buf.data_ptr() + self.img_off
        j.bias_out = buf.data_ptr() + self.bias_off
        j.K, j.C, j.RS, j.c_offset, j.c_total, j.kind, j.reserved = self.k, self.c, self.r * self.s, 0, self.c, 2, self.cpad
        return j

    def desc(self, x):
        return ops._desc(tuple(x.shape), (self.kpad, self.cpad, self.r, self.s), self.stride, self.pad, self.dil)


class HalfFoldedNet:
    """The -half_acc model's eval forward with every BatchNorm folded into its fp16 convolution, partial-convolution layers included.  Holds one device
    buffer with every fp16 weight image and b'; reads the fp32 master parameters and running statistics at fold / refresh() time only."""

    def __init__(self, model):
        _check_half_foldable(model)
        self.model = model
        self.family = _family(model)
        self.device = next(model.parameters()).device
        self.skip_relu = bool(getattr(model, 'skip_relu', False))
        self.early_dist = bool(getattr(model, 'early_dist', False))
        self.convs = []
        fam = self.family
        self.stems = {'conv1': self._add(_HConv(model.conv1, model.bn1))}
        if fam in ('fusionnet', 'partial_fusionnet'):
            self.stems['conv2'] = self._add(_HConv(model.conv2, model.bn2))
        layers = {'depthnet': ('layer1', 'layer2', 'layer3', 'layer4'), 'resnet': ('layer1', 'layer2', 'layer3', 'layer4'),
                  'fusionnet': ('layer1', 'layer2', 'layer3', 'layer4', 'layer5', 'layer6'), 'partial_depthnet': ('layer1', 'layer2', 'layer3', 'layer4'),
                  'partial_fusionnet': ('layer1', 'layer2', 'layer3', 'layer4', 'layer5', 'layer6')}[fam]
        self.blocks = {}
        for lname in layers:
            plans = []
            for blk in getattr(model, lname):
                plan = dict(block=blk, chain=[self._add(_HConv(getattr(blk, c), getattr(blk, b))) for c, b in blk._chain])
                plan['ds'] = self._add(_HConv(blk.downsample[0], blk.downsample[1])) if blk.downsample is not None else None
                plans.append(plan)
            self.blocks[lname] = plans
        if fam in ('fusionnet', 'partial_fusionnet'):
            self.fusion = self._add(_HConv(model.fusion.conv, model.fusion.bn))
        heads = ('cam_regressor', 'mat_regressor') if fam == 'resnet' else ('regressor',)
        self.heads = [self._add(_HConv(getattr(model, h), None)) if getattr(model, h, None) is not None else None for h in heads]
        at = 0
        for c in self.convs:
            at = c.layout(at)
        self.buffer = torch.zeros(max(at, _ALIGN), dtype=torch.uint8, device=self.device)
        self.refresh()

    def _add(self, c):
        self.convs.append(c)
        return c

    # ---- folding ------------------------------------------------------------------------------------------------
    def refresh(self):
        """Re-fold every conv from the current fp32 parameters and running statistics: one fold launch for the whole network."""
        _check_half_foldable(self.model)
        jobs = [j for j in (c.job(self.buffer) for c in self.convs) if j is not None]
        if jobs:
            table = (FoldJob * len(jobs))(*jobs)
            self._jobs = torch.frombuffer(bytearray(table), dtype=torch.uint8).to(self.device)     # (kept alive until the launch has read it)
            check(lib().p3d_fx_fold_bn_images(ops._p(self._jobs), len(jobs), 64, ops._stream()), 'p3d_fx_fold_bn_images')
        for c in self.convs:
            if c.images is not None:
                c.images.refresh(c.conv.weight)
        return self

    def _at(self, off):
        return ctypes.c_void_p(self.buffer.data_ptr() + off)

    def bias(self, c):
        """b' of a folded conv as a tensor view of the buffer (tests)."""
        return self.buffer[c.bias_off:c.bias_off + 4 * c.k].view(torch.float32)

    def image(self, c):
        """The fp16 folded forward image [K][R][S][Cpad] of a conv (tests)."""
        return self.buffer[c.img_off:c.img_off + 2 * c.k * c.r * c.s * c.cpad].view(torch.float16).view(c.k, c.r, c.s, c.cpad)

    # ---- forward ---------------------------------------------------------------------------------------------------
    def _conv(self, c, x, res=None, relu=False, mask_in=None, mult=None):
        """y = fp16(relu?(conv(x * mask_in) * mult + b' + res)) on the folded image; a conv the entry point cannot take runs on today's fp16 path."""
        L = lib()
        d = c.desc(x)
        if c.foldable and L.p3d_hconv2d_fwd_infer_supported(ctypes.byref(d)):
            y = ops_half._empty(d.N, d.K, d.Ho, d.Wo, x.device)
            check(L.p3d_hconv2d_fwd_infer(ctypes.byref(d), ops._p(x), self._at(c.img_off), self._at(c.bias_off), ops._p(mask_in), ops._p(mult),
                                          ops._p(res), int(bool(relu)), ops._p(y), ops._stream()), 'p3d_hconv2d_fwd_infer')
            return y if c.kpad == c.k else y[:, :c.k]
        if c.images is None:                                # per-layer fallback: the unfolded conv, then the eval-mode BatchNorm pass
            c.images = ops_half.WeightImages(c.conv.weight, need_dgrad=False)
            c.images.refresh(c.conv.weight)
        y = ops_half.HConv2dFn.apply(x, c.conv.weight, c.conv.bias, c.images, c.stride, c.pad, c.dil, None, None, mask_in, mult)
        if c.bn is None:
            return ops_half.relu(y) if relu else y
        bn = c.bn
        return ops_half.batch_norm_act(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, res, relu, False, 0.0, bn.eps)

    def _pconv(self, c, x, veil, res=None, relu=True):
        """A partial convolution (partial_conv.py): mask_in = veil, mult and mask_out from its box count; returns (y, mask_out)."""
        mult, mask_out = ops.mask_count(veil, c.r, c.stride, c.pad, c.dil)
        return self._conv(c, x, res, relu, mask_in=veil.contiguous(), mult=mult), mask_out

    def _pool(self, x):
        """max pool 3x3 / 2 behind the folded stem (its ReLU already applied: max and ReLU commute per channel), no window codes."""
        n, c, h, w = x.shape
        y = ops_half._empty(n, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1, x.device)
        check(lib().p3d_hmaxpool3x3s2_fwd(ops._p(x), ops._p(y), None, n, h, w, c, ops._stream()), 'p3d_hmaxpool3x3s2_fwd')
        return y

    def _layer(self, name, x, veil=None):
        for plan in self.blocks[name]:
            blk = plan['block']
            res = x if plan['ds'] is None else self._conv(plan['ds'], x)
            out, last = x, len(plan['chain']) - 1
            for i, c in enumerate(plan['chain']):
                if blk.partial:                             # (the closing ReLU of a partial block is unconditional, partial_depthnet.py:70-75)
                    out, veil = self._pconv(c, out, veil, res if i == last else None)
                else:
                    out = self._conv(c, out, res if i == last else None, relu=(i < last) or not blk.skip_relu)
            x = out
        return x if veil is None else (x, veil)

    @staticmethod
    def _in(x):
        x = x.float() if x.dtype == torch.float16 else x
        return ops_half.to_half_nhwc(x, ops_half.pad8(x.shape[1]))

    @staticmethod
    def _out(*tensors):
        out = tuple(ops_half.to_float(t) for t in tensors)
        return out if len(out) > 1 else out[0]

    def __call__(self, x, y=None):
        with torch.no_grad():
            return self._forward(x, y)

    def _forward(self, x, y):
        m, fam = self.model, self.family
        relu = ops_half.relu
        if fam == 'partial_depthnet':
            veil = ops.nonzero_mask(x.float())
            h, veil = self._pconv(self.stems['conv1'], self._in(x), veil)
            h, veil = self._pool(h), m.maxpool(veil)
            h, veil = self._layer('layer1', h, veil)
            h, _ = self._layer('layer2', h, veil)
            h = self._layer('layer4', self._layer('layer3', h))
            return self._out(self._conv(self.heads[0], h), h)
        x = self._pool(self._conv(self.stems['conv1'], self._in(x), relu=True))
        if fam == 'resnet':
            for name in ('layer1', 'layer2', 'layer3', 'layer4'):
                x = self._layer(name, x)
            return self._out(*[self._conv(c, x) for c in self.heads if c is not None])
        x = self._layer('layer2', self._layer('layer1', x))
        if fam == 'fusionnet':
            y = self._pool(self._conv(self.stems['conv2'], self._in(y), relu=True))
            y = self._layer('layer6', self._layer('layer5', y))
            x = self._conv(self.fusion, ops_half.concat(x, y), relu=True)
        elif fam == 'partial_fusionnet':
            veil = ops.nonzero_mask(y.float())
            y, veil = self._pconv(self.stems['conv2'], self._in(y), veil)
            y, veil = self._pool(y), m.maxpool(veil)
            y, veil = self._layer('layer5', y, veil)
            y, _ = self._layer('layer6', y, veil)
            x = self._conv(self.fusion, ops_half.concat(x, y), relu=True)
            x = self._layer('layer4', self._layer('layer3', x))
            return self._out(self._conv(self.heads[0], x), x)
        a = self._layer('layer3', x)
        n = self._layer('layer4', relu(a) if self.skip_relu else a)
        z = self._conv(self.heads[0], relu(n) if self.skip_relu else n)
        return self._out(z, a if self.early_dist else n)


def fold_half(model):
    """HalfFoldedNet of a -half_acc network in eval mode: fp32 (or fp16) NCHW input, fp32 NCHW outputs, as model.eval()(x) returns them under
    -half_acc.  Raises P3DError for a BatchNorm in training mode or parameters that are not fp32 on the HIP device."""
    model = getattr(model, 'module', model)
    _check_half_foldable(model)
    return HalfFoldedNet(model)
