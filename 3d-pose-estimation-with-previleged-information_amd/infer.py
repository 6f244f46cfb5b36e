"""Fast inference forward with eval-mode BatchNorm folded into the x3 convolutions (csrc/p3d_fx.hip).

An eval-mode BatchNorm is a per-channel affine map, so behind a convolution it folds into the weights and a bias:
s = gamma / sqrt(var + eps), w' = w * s, b' = beta - mean * s (+ s * conv bias).  `fold(model)` builds the forward weight image of every w'
and every b' in ONE device buffer (p3d_fx_fold_bn_images: one launch for the whole network); `FoldedNet(x[, y])` then runs the network on
p3d_fx_conv_fwd_infer, whose epilogue adds b', the residual and the ReLU, and on p3d_stem_fwd + p3d_stem_tail_infer for the 7x7 stem.

    net = infer.fold(model.eval())      # depthnet / resnet (legacy) / fusionnet / partial_depthnet / partial_fusionnet
    z, feat = net(x)                    # what model.eval()(x) returns, under no_grad
    ...optimizer step / new running statistics...
    net.refresh()                       # re-fold from the current parameters (one launch)

A conv the x3 forward cannot take (odd sizes, fx_applies(FX_FWD)) goes through today's eval path for that layer (ops.conv_bn_eval).  `fold(model,
any_size=True)` sends such a dense conv to p3d_fx_conv_fwd_infer_any first, the same x3 arithmetic on the same folded image for map widths that are not
multiples of 4 (the reference's default -side_in 257: 65, 33 and 17 wide maps).  `fold(model, any_size=True, odd_sides=True)` folds what that leaves at an odd
crop as well: a partial conv the masked entry refuses goes to p3d_fx_conv_fwd_infer_masked_any (the ragged kernels with mask_in in the operand fetch and mult in
the store), and a 7x7 stem p3d_stem_supported refuses runs on p3d_stem_image_any (the space-to-depth image of the input zero-extended to sides the stem
kernel takes: 257 -> 264) + p3d_stem_fwd on the padded sides + p3d_stem_tail_infer_any (the max pool over the valid prefix of the pitched result, a masked
stem's mult multiplied in before the max).  Without odd_sides those stay where they were, launch for launch.

The partial-convolution layers of partial_depthnet (stem, layer1, layer2) and partial_fusionnet (conv2, layer5, layer6) fold as well: each conv runs on
p3d_fx_conv_fwd_infer_masked (mask_in multiplied into the operand, y = relu?(conv * mult + b' + res), the factor before b'), each with its own
ops.mask_count, and the PartialConv stem on p3d_stem_image_masked + p3d_stem_fwd_masked (x mult) + p3d_stem_tail_infer.  A partial conv with a bias, a shape
the masked entry refuses or a stem p3d_stem_masked_supported refuses (odd sides) runs as the model's own module, that layer only.

`fold_half(model)` is the same for the fp16 (-half_acc) network: kind-2 fold jobs write fp16 [K][R][S][Cpad] images of every w' (the layout
p3d_weight_images_f16 produces) and `HalfFoldedNet(x[, y])` runs every conv on p3d_hconv2d_fwd_infer, whose epilogue adds b', the residual and the
ReLU before the one rounding to fp16.  The partial-convolution layers fold too (mask_in in the operand fetch, mult in the epilogue), so an fp16 folded
forward has no BatchNorm pass at all.

`fold_fp8(model)` is the fp16 folded network with block-scaled FP8 (MXFP8) convolutions in between: every conv of the residual blocks, the partial
layers and the Fusion 1x1 that p3d_f8conv2d_fwd_infer accepts folds to a kind-3 MXFP8 image (e4m3 elements, one E8M0 scale per 32 input channels of a
tap) and runs on that entry point, which quantizes its fp16 input by the same rule while staging it; the stems and the heads stay on the fp16 folded conv
(the usual first / last layer rule), and so does a conv the entry point refuses.  One fold launch writes the kind-3 and the kind-2 images together.
`fold_fp8(model, resident=True)` gives the same outputs bit for bit, with the activations between fp8 convs kept as MXFP8 tensors: a conv quantizes its
result once, in its epilogue (p3d_f8conv2d_fwd_infer_mx), and the next conv copies the bytes in place of quantizing them per tap and row tile; the results
inside a block's chain exist as MXFP8 only (resident_forms).

All four share the plan (stems, blocks, fusion, heads), the fold launch and the walk over the network (_Folded); FoldedNet, HalfFoldedNet,
Fp8FoldedNet and Fp8ResidentNet supply the per-layer primitives.  Two A/B switches were measured and removed, because each only selected a slower path: leaving the partial stem
and layers on the model's own modules (9.80 against 8.90 ms for R50 partial_depthnet, 13.10 against 12.22 ms for partial_fusionnet,
profiles/eval_folded_partial.md), and feeding the 64-channel layers as an activation image (2.7 % slower, profiles/eval_folded.md).
"""
import ctypes
import os

import torch

from . import ops, ops_block, ops_half
from ._lib import FoldJob, P3DError, check, lib
from .nn import _one
from .partial_conv import PartialConv

_ALIGN = 256


def enabled():
    """P3D_FOLDED_EVAL=1: Trainer.test and the distillation teacher evaluate through a FoldedNet."""
    return os.environ.get('P3D_FOLDED_EVAL', '0') == '1'


def half_enabled():
    """P3D_FOLDED_EVAL_HALF=1: under -half_acc, Trainer.test and the distillation teacher evaluate through a HalfFoldedNet."""
    return os.environ.get('P3D_FOLDED_EVAL_HALF', '0') == '1'


def fp8_enabled():
    """P3D_FOLDED_EVAL_FP8=1: Trainer.test and the distillation teacher evaluate through an Fp8FoldedNet, in fp32 and under -half_acc; it takes
    precedence over P3D_FOLDED_EVAL and P3D_FOLDED_EVAL_HALF."""
    return os.environ.get('P3D_FOLDED_EVAL_FP8', '0') == '1'


def _family(model):
    name = type(model).__module__.rsplit('.', 1)[-1]
    if name not in ('depthnet', 'resnet', 'fusionnet', 'partial_depthnet', 'partial_fusionnet'):
        raise P3DError('infer.fold: unknown network family %s.%s' % (type(model).__module__, type(model).__name__))
    return name


def _check_foldable(model, who, half):
    """Refuse what folding would get wrong: a BatchNorm in training mode or without running statistics, parameters that are not fp32 on the HIP
    device, and for the fp32 fold (half False) a -half_acc model."""
    if not half and getattr(model, '_p3d_half', False):
        raise P3DError('%s: a -half_acc (fp16) model cannot be folded onto the fp32 kernels; use infer.fold_half' % who)
    for name, m in model.named_modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            if m.training:
                raise P3DError('%s: BatchNorm %r is in training mode; call model.eval() first (folding uses the running statistics)' % (who, name))
            if not (m.affine and m.track_running_stats):
                raise P3DError('%s: BatchNorm %r has no running statistics / affine parameters' % (who, name))
    for p in model.parameters():
        if not p.is_cuda or p.dtype != torch.float32:
            raise P3DError('%s: parameters must be fp32%s on the HIP device' % (who, ' masters' if half else ''))


def _fold_job(conv, bn, buf, out_off, bias_off):
    """The FoldJob of conv (+ bn: None for a head) writing to buf at out_off and bias_off; the caller sets the kind and the shape fields."""
    j = FoldJob()
    j.w = conv.weight.data_ptr()
    j.conv_bias = conv.bias.data_ptr() if conv.bias is not None else None
    if bn is not None:
        j.gamma, j.beta = bn.weight.data_ptr(), bn.bias.data_ptr()
        j.mean, j.var = bn.running_mean.data_ptr(), bn.running_var.data_ptr()
        j.eps = float(bn.eps)
    j.out = buf.data_ptr() + out_off
    j.bias_out = buf.data_ptr() + bias_off if bias_off is not None else None
    return j


def _up(v):
    return (v + _ALIGN - 1) // _ALIGN * _ALIGN


class _Conv:
    """One conv (+ BatchNorm) of the folded network: where its image and bias live in the buffer, and how to run it."""

    def __init__(self, conv, bn, c_offset=0, c_count=None, has_bias=True):
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
        fb = ctypes.c_size_t()
        check(lib().p3d_fx_weight_image_bytes(self.k, self.c, self.rs, ctypes.byref(fb), None), 'p3d_fx_weight_image_bytes')
        self.img_off, self.img_bytes = at, fb.value
        at = _up(at + fb.value)
        if self.has_bias:
            self.bias_off = at
            at = _up(at + 4 * self.k)
        return at

    def job(self, buf):
        j = _fold_job(self.conv, self.bn, buf, self.img_off, self.bias_off)
        j.K, j.C, j.RS, j.c_offset, j.c_total, j.kind = self.k, self.c, self.rs, self.c_offset, self.ct, 0
        return j

    def desc(self, x, accumulate=0):
        return ops._desc(x.shape, (self.k, self.c, int(self.rs ** 0.5), int(self.rs ** 0.5)), self.stride, self.pad, self.dil, accumulate=accumulate)


class _Stem:
    """The 7x7 stride-2 stem + BatchNorm + ReLU + max pool: folded fp32 weights (kind 1) -> p3d_stem_weight_image -> p3d_stem_fwd -> p3d_stem_tail_infer."""

    def __init__(self, conv, bn):
        self.conv, self.bn = conv, bn
        self.k, self.cin = conv.weight.shape[0], conv.weight.shape[1]
        self.masked = type(conv).__name__ == 'PartialConv'      # the partial families' stems: mask_in into the image, mult into the epilogue
        self.foldable = (type(conv).__name__ in ('Conv2d', 'PartialConv') and conv.bias is None and tuple(conv.kernel_size) == (7, 7) and _one(conv.stride) == 2
                         and _one(conv.padding) == 3 and _one(conv.dilation) == 1 and 1 <= self.cin <= 4 and self.k % 16 == 0 and self.k <= 128)

    def layout(self, at):
        self.w_off = at
        at = _up(at + 4 * self.k * self.cin * 49)
        self.img_off = at
        at = _up(at + lib().p3d_stem_weight_image_bytes(self.k))
        self.bias_off = at
        return _up(at + 4 * self.k)

    def job(self, buf):
        j = _fold_job(self.conv, self.bn, buf, self.w_off, self.bias_off)
        j.K, j.C, j.RS, j.c_offset, j.c_total, j.kind = self.k, self.cin, 49, 0, self.cin, 1
        return j


class _HConv:
    """One conv (+ BatchNorm) of the fp16 folded network: its fp16 image [K][R][S][Cpad] and b' in the buffer (fold kind 2).  A head whose K is not a
    multiple of 8 (the 17-channel mat_regressor of -joint_space) runs with its image and bias padded to Kpad rows of zeros; its result is the first K channels."""

    def __init__(self, conv, bn):
        self.conv, self.bn = conv, bn
        k, c, r, s = conv.weight.shape
        self.k, self.kpad, self.c, self.cpad, self.r, self.s = k, ops_half.pad8(k), c, ops_half.pad8(c), r, s
        self.stride, self.pad, self.dil = _one(conv.stride), _one(conv.padding), _one(conv.dilation)
        self.partial = isinstance(conv, PartialConv)
        self.foldable = k <= 2048                           # (the fold kernel's per-job scale table; else: today's fp16 path for this layer)
        self.images = None                                  # fp16 images of the unfolded weight, for that path only
        self.img_off = self.bias_off = None

    def layout(self, at):
        self.img_off = at
        at = _up(at + 2 * self.kpad * self.r * self.s * self.cpad)           # (rows K .. Kpad - 1 stay zero: the buffer is zeroed once, the fold writes K rows)
        self.bias_off = at
        return _up(at + 4 * self.kpad)

    def job(self, buf):
        j = _fold_job(self.conv, self.bn, buf, self.img_off, self.bias_off)
        j.K, j.C, j.RS, j.c_offset, j.c_total, j.kind, j.reserved = self.k, self.c, self.r * self.s, 0, self.c, 2, self.cpad
        return j

    def desc(self, x):
        return ops._desc(tuple(x.shape), (self.kpad, self.cpad, self.r, self.s), self.stride, self.pad, self.dil)


class _Folded:
    """model.eval()'s forward with every BatchNorm folded into its convolution.  Holds the plan (stems, blocks, fusion, heads) and one device buffer
    with every folded image and b', filled by one fold launch; parameters and running statistics are read at fold / refresh() time only (the
    per-layer fallbacks read them live).  The walk (_forward, _branch, _layer) is written here only and treats the activation it carries as opaque.  A
    subclass supplies the precision: its conv type (Conv), how a stem and the Fusion 1x1 fold, and the per-layer primitives the walk calls: _in, _out,
    _stem, _stem_masked, _fusion, _head, _relu (given here) and, for a conv of a residual block, _chain_conv, which as given here runs _conv_bn (dense) or
    _pconv (partial); a net whose result depends on the conv's place in its chain replaces _chain_conv itself (Fp8ResidentNet).  WHO names it in a
    refusal, HALF marks the -half_acc fold."""

    def __init__(self, model):
        self.model = model
        self.family = _family(model)
        self.skip_relu = bool(getattr(model, 'skip_relu', False))
        self.early_dist = bool(getattr(model, 'early_dist', False))
        self.stems, self.convs, self.blocks = {}, [], {}
        fusion = self.family in ('fusionnet', 'partial_fusionnet')
        self.stems['conv1'] = self._plan_stem(model.conv1, model.bn1)
        if fusion:
            self.stems['conv2'] = self._plan_stem(model.conv2, model.bn2)
        for lname in ('layer1', 'layer2', 'layer3', 'layer4') + (('layer5', 'layer6') if fusion else ()):
            plans = []
            for blk in getattr(model, lname):
                plan = dict(block=blk, chain=[self._add(self.Conv(getattr(blk, c), getattr(blk, b))) for c, b in blk._chain])
                plan['ds'] = self._add(self.Conv(blk.downsample[0], blk.downsample[1])) if blk.downsample is not None else None
                plans.append(plan)
            self.blocks[lname] = plans
        if fusion:
            self.fusion = self._plan_fusion(model.fusion)
        heads = ('cam_regressor', 'mat_regressor') if self.family == 'resnet' else ('regressor',)
        self.heads = [self._add(self._plan_head(getattr(model, h))) if getattr(model, h, None) is not None else None for h in heads]
        self._allocate(next(model.parameters()).device)

    def _add(self, c):
        self.convs.append(c)
        return c

    def _plan_head(self, conv):
        return self.Conv(conv, None)

    def _units(self):
        """Everything the fold launch writes, in buffer order."""
        return self.convs

    def _allocate(self, device):
        at = 0
        for u in self._units():
            if u.foldable:
                at = u.layout(at)
        alloc = torch.zeros if self.HALF else torch.empty       # (fp16: the padding rows K .. Kpad - 1 of a head's image and bias are read)
        self.buffer = alloc(max(at, _ALIGN), dtype=torch.uint8, device=device)
        self.refresh()

    # ---- folding ------------------------------------------------------------------------------------------------
    def refresh(self):
        """Re-fold every conv from the current parameters and running statistics: one fold launch for the whole network."""
        _check_foldable(self.model, self.WHO, self.HALF)
        jobs = [u.job(self.buffer) for u in self._units() if u.foldable]
        if jobs:
            table = (FoldJob * len(jobs))(*jobs)
            self._jobs = torch.frombuffer(bytearray(table), dtype=torch.uint8).to(self.buffer.device)     # (kept alive until the launch has read it)
            check(lib().p3d_fx_fold_bn_images(ops._p(self._jobs), len(jobs), 64, ops._stream()), 'p3d_fx_fold_bn_images')
        return self

    def _at(self, off):
        return ctypes.c_void_p(self.buffer.data_ptr() + off)

    def bias(self, c):
        """b' of a folded conv as a tensor view of the buffer (tests)."""
        return self.buffer[c.bias_off:c.bias_off + 4 * c.k].view(torch.float32)

    # ---- forward ---------------------------------------------------------------------------------------------------
    def _layer(self, name, x, veil=None):
        """The residual blocks of a layer, and the one statement of the block rule: the shortcut is the input or its downsample conv, it enters the last conv of
        the chain, every conv has a ReLU but the closing one of a skip_relu block, and a partial block threads the validity mask through its chain."""
        for plan in self.blocks[name]:
            blk, chain = plan['block'], plan['chain']
            res = x if plan['ds'] is None else self._chain_conv(plan['ds'], x)[0]
            out, last = x, len(chain) - 1
            for i, c in enumerate(chain):
                relu = blk.partial or i < last or not blk.skip_relu      # (the closing ReLU of a partial block is unconditional: _trunk.py forward_partial)
                out, mask_out = self._chain_conv(c, out, res if i == last else None, relu, veil if blk.partial else None, chain, i)
                veil = mask_out if blk.partial else veil
            x = out
        return x if veil is None else (x, veil)

    def _chain_conv(self, c, x, res=None, relu=False, veil=None, chain=None, i=0):
        """Conv c of a residual block on the activation x -> (y, mask_out): a partial conv comes with its validity mask (veil), a dense one with none
        (mask_out None).  c is chain[i] (chain None: the downsample shortcut), which only a net whose result depends on its reader looks at."""
        return (self._conv_bn(c, x, res, relu), None) if veil is None else self._pconv(c, x, veil, res, relu)

    def _branch(self, stem, layers, x):
        """A stem and its two layers.  A PartialConv stem starts the validity mask x != 0, which its layers carry (the last mask_out feeds nothing)."""
        st = self.stems[stem]
        if not isinstance(st.conv, PartialConv):
            return self._layer(layers[1], self._layer(layers[0], self._stem(st, self._in(x))))
        veil = ops.nonzero_mask(x.float())
        x, veil = self._stem_masked(st, self._in(x), veil)
        return self._layer(layers[1], *self._layer(layers[0], x, veil))[0]

    def __call__(self, x, y=None):
        with torch.no_grad():
            out = tuple(self._out(t) for t in self._forward(x, y))
        return out if len(out) > 1 else out[0]

    def _forward(self, x, y):
        """depthnet.py, resnet.py, fusionnet.py, partial_depthnet.py and partial_fusionnet.py: the x branch (stem, layer1, layer2); under fusion the
        y branch (conv2, layer5, layer6) and the Fusion 1x1; layer3, layer4 (skip_relu: ReLU between them and before the head); the heads."""
        x = self._branch('conv1', ('layer1', 'layer2'), x)
        if 'conv2' in self.stems:
            x = self._fusion(x, self._branch('conv2', ('layer5', 'layer6'), y))
        a = self._layer('layer3', x)
        n = self._layer('layer4', self._relu(a) if self.skip_relu else a)
        if self.family == 'resnet':
            return tuple(self._head(c, n) for c in self.heads if c is not None)
        return self._head(self.heads[0], self._relu(n) if self.skip_relu else n), (a if self.early_dist else n)

    def _relu(self, x):
        return ops.relu(x)


# The fp32 x3 inference entries in the order a conv is offered to them, dense (False) and masked (True): the entry (its support query is the name +
# '_supported'), what that query takes behind the descriptor and the entry between x and the weight image (p3d_fx_conv_fwd_infer alone: fed the fp32
# tensor, no activation image), the workspace query, and the FoldedNet keyword that enables the entry (None: always).
_X3 = {False: (('p3d_fx_conv_fwd_infer', (0,), (None,), 'p3d_fx_conv_fwd_infer_workspace_bytes', None),
               ('p3d_fx_conv_fwd_infer_any', (), (), 'p3d_fx_conv_fwd_infer_any_workspace_bytes', 'any_size')),
       True: (('p3d_fx_conv_fwd_infer_masked', (), (), 'p3d_fx_conv_fwd_infer_workspace_bytes', None),
              ('p3d_fx_conv_fwd_infer_masked_any', (), (), 'p3d_fx_conv_fwd_infer_masked_any_workspace_bytes', 'odd_sides'))}


class FoldedNet(_Folded):
    """The fp32 folded network, on the x3 kernels.  Besides the buffer it holds one workspace; the stems fold to fp32 weights, then each is restated
    as the image the stem kernels read."""
    WHO, HALF, Conv = 'infer.fold', False, _Conv

    def __init__(self, model, any_size=False, odd_sides=False):
        self.any_size = bool(any_size)
        self.odd_sides = bool(odd_sides) and self.any_size      # (acts only together with any_size)
        super().__init__(model)

    def _allocate(self, device):
        self.workspace = torch.empty(1 << 20, dtype=torch.uint8, device=device)
        super()._allocate(device)

    def _plan_stem(self, conv, bn):
        return _Stem(conv, bn)

    def _plan_fusion(self, f):
        """The Fusion 1x1 as its two input-channel windows: x's without b', then y's accumulated onto it with b' and the ReLU."""
        half = f.conv.weight.shape[1] // 2
        return self._add(_Conv(f.conv, f.bn, 0, half, has_bias=False)), self._add(_Conv(f.conv, f.bn, half, half))

    def _units(self):
        return list(self.stems.values()) + self.convs

    def refresh(self):
        """Re-fold every conv from the current parameters and running statistics: one fold launch (+ the stem's image restatement)."""
        super().refresh()
        for s in self.stems.values():
            if s.foldable:
                ws = self._ws(s.k * 256 * 4)
                check(lib().p3d_stem_weight_image(self._at(s.w_off), s.k, s.cin, self._at(s.img_off), ops._p(ws), ws.numel(), ops._stream()),
                      'p3d_stem_weight_image')
        return self

    def _ws(self, nbytes):
        if self.workspace.numel() < nbytes:
            self.workspace = torch.empty(int(nbytes), dtype=torch.uint8, device=self.buffer.device)
        return self.workspace

    def image(self, c):
        """The folded forward weight image of a conv (tests)."""
        return self.buffer[c.img_off:c.img_off + c.img_bytes]

    @staticmethod
    def _in(x):
        return x

    _out = _in

    def _conv(self, c, x, res=None, relu=False, out=None, accumulate=0, veil=None):
        """y = conv(x, w') + b' (+ out) (+ res) (then ReLU) on the folded image, on the first entry of _X3 that takes the conv; None when none does.  With
        a veil, the partial convolution y = relu?(conv(x * veil, w') * mult + b' + res), mult and mask_out from the box count of veil (ops.mask_count);
        returns (y, mask_out)."""
        if not c.foldable:
            return None
        L, d = lib(), c.desc(x, accumulate)
        for name, fed, image, ws_name, keyword in _X3[veil is not None]:
            if (keyword is None or getattr(self, keyword)) and getattr(L, name + '_supported')(ctypes.byref(d), *fed):
                break
        else:
            return None
        mask = ()
        if veil is not None:
            if tuple(veil.shape) != (d.N, 1, d.H, d.W) or veil.dtype != torch.float32:
                raise P3DError('infer: the validity mask of a partial conv must be fp32 [N, 1, H, W] like its input, got %s %s' % (tuple(veil.shape), veil.dtype))
            mult, mask_out = ops.mask_count(veil, c.r, c.stride, c.pad, c.dil)
            veil = veil.contiguous()
            mask = ops._p(veil), ops._p(mult)
        x = x.contiguous()
        y = out if out is not None else torch.empty((d.N, d.K, d.Ho, d.Wo), dtype=torch.float32, device=x.device)
        ws = self._ws(getattr(L, ws_name)(ctypes.byref(d)))
        check(getattr(L, name)(ctypes.byref(d), ops._p(x), *image, self._at(c.img_off), c.img_bytes, self._at(c.bias_off) if c.bias_off is not None else None,
                               *mask, ops._p(None if res is None else res.contiguous()), int(bool(relu)), ops._p(y), ops._p(ws), ws.numel(), ops._stream()), name)
        return y if veil is None else (y, mask_out)

    def _conv_bn(self, c, x, res=None, relu=False):
        y = self._conv(c, x, res, relu)
        if y is None:                                       # per-layer fallback: today's fused eval kernel
            y = ops.conv_bn_eval(x, c.conv, c.bn, res=res, relu=relu)
        return y

    def _pconv(self, c, x, veil, res=None, relu=True):
        """A partial convolution (partial_conv.py) + its folded BatchNorm -> (y, mask_out).  A conv no masked entry takes runs as the module, then the
        eval-mode BatchNorm pass."""
        out = self._conv(c, x, res, relu, veil=veil)
        if out is None:
            y, mask_out = c.conv(x, veil)
            out = c.bn(y, res=res, relu=relu), mask_out
        return out

    def _stem_x3(self, s, x, veil=None, padded=False):
        """The restated 7x7 stem + BatchNorm + ReLU + max pool -> (y, mask_out), mask_out (not pooled) None without a veil; None when the shape is outside it.
        With a veil it is the PartialConv stem (partial_depthnet.py:177), conv(x * veil) * mult with mult and mask_out from ops.mask_count.  Aligned sides: the
        space-to-depth image of x (* veil), the stem conv with mult in its epilogue, then relu(maxpool(.) + b') (= maxpool(relu(. + b')): both monotone per
        channel).  padded (odd_sides), for sides p3d_stem_supported refuses: the image zero-extended to the padded sides, the stem conv on those (never with
        the output factor), then relu(maxpool(c * mult) + b') over the valid prefix of the pitched c."""
        n, cin, h, w = x.shape
        L = lib()
        if padded:
            query, fits = L.p3d_stem_any_supported, self.odd_sides
        else:
            query, fits = (L.p3d_stem_supported if veil is None else L.p3d_stem_masked_supported), (h // 2) % 2 == 0 and (w // 2) % 4 == 0
        if not (fits and s.foldable and x.is_cuda and x.dtype == torch.float32 and cin == s.cin and query(n, cin, h, w, s.k)
                and (veil is None or (veil.dtype == torch.float32 and tuple(veil.shape) == (n, 1, h, w)))):
            return None
        hp, wp = h, w
        if padded:
            hp, wp = ctypes.c_int32(), ctypes.c_int32()
            L.p3d_stem_any_padded(h, w, ctypes.byref(hp), ctypes.byref(wp))
            hp, wp = hp.value, wp.value
        x, st = x.contiguous(), ops._stream()
        mult = mask_out = None
        if veil is not None:
            veil = veil.contiguous()
            mult, mask_out = ops.mask_count(veil, 7, 2, 3, 1)
        x_img = torch.empty(L.p3d_stem_image_bytes(n, hp, wp), dtype=torch.uint8, device=x.device)
        if padded:
            check(L.p3d_stem_image_any(ops._p(x), ops._p(veil), ops._p(x_img), n, cin, h, w, st), 'p3d_stem_image_any')
        elif veil is None:
            check(L.p3d_stem_image(ops._p(x), ops._p(x_img), n, cin, h, w, st), 'p3d_stem_image')
        else:
            check(L.p3d_stem_image_masked(ops._p(x), ops._p(veil), ops._p(x_img), n, cin, h, w, st), 'p3d_stem_image_masked')
        c = torch.empty((n, s.k, hp // 2, wp // 2), dtype=torch.float32, device=x.device)
        if padded or veil is None:
            check(L.p3d_stem_fwd(ops._p(x_img), self._at(s.img_off), ops._p(c), n, cin, hp, wp, s.k, st), 'p3d_stem_fwd')
        else:
            check(L.p3d_stem_fwd_masked(ops._p(x_img), self._at(s.img_off), ops._p(c), ops._p(mult), n, cin, h, w, s.k, st), 'p3d_stem_fwd_masked')
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        y = torch.empty((n, s.k, (ho - 1) // 2 + 1, (wo - 1) // 2 + 1), dtype=torch.float32, device=x.device)
        if padded:
            check(L.p3d_stem_tail_infer_any(ops._p(c), self._at(s.bias_off), ops._p(mult), ops._p(y), n, s.k, h, w, st), 'p3d_stem_tail_infer_any')
        else:
            check(L.p3d_stem_tail_infer(ops._p(c), self._at(s.bias_off), ops._p(y), n, s.k, ho, wo, st), 'p3d_stem_tail_infer')
        return y, mask_out

    def _stem_any(self, s, x, veil=None):
        return self._stem_x3(s, x, veil, padded=True)

    def _stem(self, s, x, veil=None):
        """The stem of a branch -> y, with a veil (a PartialConv stem) -> (y, max-pooled mask_out): the aligned restated stem, else the padded one, else the
        model's own modules (odd sides without odd_sides)."""
        out = None
        if s.masked == (veil is not None):
            out = self._stem_x3(s, x, veil) or self._stem_x3(s, x, veil, padded=True)
        if out is not None:
            return out[0] if veil is None else (out[0], self.model.maxpool(out[1]))
        from ._trunk import stem, stem_tail
        if veil is None:
            return stem(s.conv, s.bn, self.model.maxpool, x)
        c, veil = s.conv(x, veil)
        return stem_tail(s.bn, self.model.maxpool, c), self.model.maxpool(veil)

    _stem_masked = _stem

    def _fusion(self, x, y):
        a, b = self.fusion
        out = self._conv(a, x)
        if out is not None:
            out2 = self._conv(b, y, relu=True, out=out, accumulate=1)
            if out2 is not None:
                return out2
        return self.model.fusion(x, y)                      # today's path (two windowed convs, then BatchNorm + ReLU)

    def _head(self, c, x):
        y = self._conv(c, x)
        return c.conv(x) if y is None else y


class FoldedConv(FoldedNet):
    """One conv (no bias) + eval-mode BatchNorm, folded: FoldedConv(conv, bn)(x, res=None, relu=False) = relu(bn(conv(x)) + res).  For a PartialConv
    the validity mask comes along: FoldedConv(pconv, bn)(x, res, relu, veil=mask_in) = (relu(bn(pconv(x, mask_in)[0]) + res), mask_out).
    any_size (default False: a map width p3d_fx_conv_fwd_infer refuses runs on ops.conv_bn_eval, the fp32-MFMA kernel, which tests rely on): offer such a
    dense conv to p3d_fx_conv_fwd_infer_any first; with odd_sides as well, a partial conv the masked entry refuses to p3d_fx_conv_fwd_infer_masked_any."""
    WHO = 'infer.FoldedConv'

    def __init__(self, conv, bn, any_size=False, odd_sides=False):
        self.any_size = bool(any_size)
        self.odd_sides = bool(odd_sides) and self.any_size
        self.model, self.stems = torch.nn.ModuleList([conv, bn]), {}      # (model: what refresh() checks)
        self.conv = _Conv(conv, bn)
        self.convs = [self.conv]
        self._allocate(conv.weight.device)

    def __call__(self, x, res=None, relu=False, veil=None):
        if self.conv.partial != (veil is not None):
            raise P3DError('infer.FoldedConv: a partial convolution takes its validity mask (veil=), a dense one none')
        with torch.no_grad():
            return self._pconv(self.conv, x, veil, res, relu) if self.conv.partial else self._conv_bn(self.conv, x, res, relu)


def fold(model, any_size=False, odd_sides=False):
    """FoldedNet of a network in eval mode (every BatchNorm frozen); raises P3DError for a BatchNorm in training mode or a -half_acc model.
    any_size: a dense conv whose map widths are not multiples of 4 (every layer behind the stem at -side_in 257) runs on p3d_fx_conv_fwd_infer_any
    instead of the per-layer fallback.  The default stays False: without the keyword a refused layer lands on ops.conv_bn_eval (the fp32-MFMA
    kernel) exactly as before, which is what the existing tests of the fallback count.
    odd_sides (acts only with any_size): the 7x7 stems at sides the stem kernel refuses run on the padded space-to-depth image and the pitched tail, and the
    partial layers at odd map widths on p3d_fx_conv_fwd_infer_masked_any, so a partial network folds completely at 257 as it does at 256."""
    return FoldedNet(getattr(model, 'module', model), any_size=any_size, odd_sides=odd_sides)


# ---- -half_acc: BatchNorm folded into the fp16 convolutions ------------------------------------------------------------------------------
class HalfFoldedNet(_Folded):
    """The -half_acc model's eval forward with every BatchNorm folded into its fp16 convolution, partial-convolution layers included; reads the fp32
    master parameters.  The stems are convs like any other here (then the max pool), so they are in `convs`."""
    WHO, HALF, Conv = 'infer.fold_half', True, _HConv

    def _plan_stem(self, conv, bn):
        return self._add(_HConv(conv, bn))

    def _plan_fusion(self, f):
        return self._add(_HConv(f.conv, f.bn))

    def refresh(self):
        """Re-fold every conv from the current fp32 parameters and running statistics: one fold launch for the whole network."""
        super().refresh()
        for c in self.convs:
            if c.images is not None:
                c.images.refresh(c.conv.weight)
        return self

    def image(self, c):
        """The fp16 folded forward image [K][R][S][Cpad] of a conv (tests)."""
        return self.buffer[c.img_off:c.img_off + 2 * c.k * c.r * c.s * c.cpad].view(torch.float16).view(c.k, c.r, c.s, c.cpad)

    @staticmethod
    def _in(x):
        x = x.float() if x.dtype == torch.float16 else x
        return ops_half.to_half_nhwc(x, ops_half.pad8(x.shape[1]))

    @staticmethod
    def _out(x):
        return ops_half.to_float(x)

    def _conv_bn(self, c, x, res=None, relu=False, mask_in=None, mult=None):
        """y = fp16(relu?(conv(x * mask_in) * mult + b' + res)) on the folded image; a conv the entry point cannot take runs on today's fp16 path."""
        L = lib()
        d = c.desc(x)
        if c.foldable and L.p3d_hconv2d_fwd_infer_supported(ctypes.byref(d)):
            y = ops_half._empty(d.N, d.K, d.Ho, d.Wo, x.device)
            check(L.p3d_hconv2d_fwd_infer(ctypes.byref(d), ops._p(x), self._at(c.img_off), self._at(c.bias_off), ops._p(mask_in), ops._p(mult),
                                          ops._p(res), int(bool(relu)), ops._p(y), ops._stream()), 'p3d_hconv2d_fwd_infer')
            return y if c.kpad == c.k else y[:, :c.k]
        return self._unfolded(c, x, res, relu, mask_in, mult)

    def _unfolded(self, c, x, res, relu, mask_in, mult):
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
        return self._conv_bn(c, x, res, relu, mask_in=veil.contiguous(), mult=mult), mask_out

    def _pool(self, x):
        """max pool 3x3 / 2 behind the folded stem (its ReLU already applied: max and ReLU commute per channel), no window codes."""
        n, c, h, w = x.shape
        y = ops_half._empty(n, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1, x.device)
        check(lib().p3d_hmaxpool3x3s2_fwd(ops._p(x), ops._p(y), None, n, h, w, c, ops._stream()), 'p3d_hmaxpool3x3s2_fwd')
        return y

    def _stem(self, s, x):
        return self._pool(self._conv_bn(s, x, relu=True))

    def _stem_masked(self, s, x, veil):
        y, veil = self._pconv(s, x, veil)
        return self._pool(y), self.model.maxpool(veil)

    def _fusion(self, x, y):
        return self._conv_bn(self.fusion, ops_half.concat(x, y), relu=True)

    def _head(self, c, x):
        return self._conv_bn(c, x)


def fold_half(model):
    """HalfFoldedNet of a -half_acc network in eval mode: fp32 (or fp16) NCHW input, fp32 NCHW outputs, as model.eval()(x) returns them under
    -half_acc.  Raises P3DError for a BatchNorm in training mode or parameters that are not fp32 on the HIP device."""
    return HalfFoldedNet(getattr(model, 'module', model))


# ---- block-scaled FP8 (MXFP8) between fp16 stems and heads ---------------------------------------------------------------------------------
class _F8Conv(_HConv):
    """A conv (+ BatchNorm) of the fp8 folded network: its kind-3 MXFP8 image (e4m3 elements [K][R][S][C], then the E8M0 scales [K][R][S][C / 32]) and
    b' in the buffer.  Made only for convs whose C is a multiple of 32 (so Cpad = C) and whose K a multiple of 8."""

    def layout(self, at):
        self.img_off = at
        self.img_bytes = lib().p3d_f8conv2d_weight_bytes(self.k, self.cpad, self.r * self.s)
        at = _up(at + self.img_bytes)
        self.bias_off = at
        return _up(at + 4 * self.kpad)

    def job(self, buf):
        j = super().job(buf)
        j.kind = 3
        return j


class _Act:
    """An activation of an fp8 net: the fp16 NHWC tensor (h), the MXFP8 activation tensor (mx: uint8, p3d_f8act_bytes of them, include/p3d_hip.h), or
    both; shape is its NCHW shape."""
    __slots__ = ('shape', 'h', 'mx')

    def __init__(self, shape, h=None, mx=None):
        self.shape, self.h, self.mx = tuple(shape), h, mx

    @staticmethod
    def of(x):
        return x if isinstance(x, _Act) else _Act(x.shape, x)


def _mx_supported(d, x_is_mx, y_mx):
    """p3d_f8conv2d_fwd_infer_mx_supported (host only)"""
    return bool(lib().p3d_f8conv2d_fwd_infer_mx_supported(ctypes.byref(d), int(bool(x_is_mx)), int(bool(y_mx))))


class Fp8FoldedNet(HalfFoldedNet):
    """The -half_acc folded network with the convs between the stems and the heads on p3d_f8conv2d_fwd_infer (MXFP8 weights and activations, fp32
    accumulation, fp16 NHWC in and out).  Takes the same inputs and gives the same outputs as HalfFoldedNet, from fp32 master parameters."""
    WHO, MX_ENTRY = 'infer.fold_fp8', False

    def Conv(self, conv, bn):
        """_F8Conv when the fp8 entry point takes the conv's shape (queried on a nominal 1 x C x 64 x 64 input), else the fp16 folded _HConv."""
        k, c, r, s = conv.weight.shape
        d = ops._desc((1, c, 64, 64), (k, c, r, s), _one(conv.stride), _one(conv.padding), _one(conv.dilation))
        fp8 = k <= 2048 and bool(lib().p3d_f8conv2d_fwd_infer_supported(ctypes.byref(d)))
        return (_F8Conv if fp8 else _HConv)(conv, bn)

    def _plan_head(self, conv):
        return _HConv(conv, None)

    def _plan_fusion(self, f):
        return self._add(self.Conv(f.conv, f.bn))

    def image(self, c):
        """The fp16 image of an fp16 conv, as HalfFoldedNet.image; for an fp8 conv the pair (e4m3 elements [K][R][S][C] as uint8, E8M0 scale bytes
        [K][R][S][C / 32]) (tests)."""
        if not isinstance(c, _F8Conv):
            return super().image(c)
        n = c.k * c.r * c.s * c.cpad
        img = self.buffer[c.img_off:c.img_off + n + n // 32]
        return img[:n].view(c.k, c.r, c.s, c.cpad), img[n:].view(c.k, c.r, c.s, c.cpad // 32)

    def _conv_bn(self, c, x, res=None, relu=False, mask_in=None, mult=None):
        """y = fp16(relu?(conv(q(x * mask_in), w') * mult + b' + res)) on the MXFP8 image; an fp16 conv, as HalfFoldedNet; an fp8 conv the entry point
        refuses at this input runs as HalfFoldedNet's per-layer fallback (the unfolded fp16 conv, then the eval-mode BatchNorm pass)."""
        return self._conv_act(c, _Act.of(x), (True, False), res, relu, mask_in, mult).h

    def _conv_act(self, c, x, forms, res=None, relu=False, mask_in=None, mult=None):
        """_conv_bn on an _Act, the result an _Act in `forms` (fp16, mx), and the one place an fp8 conv is launched.  Here every activation is fp16 and the
        entry is p3d_f8conv2d_fwd_infer; under MX_ENTRY (Fp8ResidentNet) it is p3d_f8conv2d_fwd_infer_mx, which reads the MX input when there is one.  The
        support query is the MX entry's for both: for fp16 in and out it asks what p3d_f8conv2d_fwd_infer_supported asks."""
        if not isinstance(c, _F8Conv):
            return _Act.of(HalfFoldedNet._conv_bn(self, c, x.h, res, relu, mask_in, mult))
        L, d = lib(), c.desc(x)
        if not _mx_supported(d, x.mx is not None, forms[1]):
            return _Act.of(self._unfolded(c, x.h, res, relu, mask_in, mult))
        dev = (x.h if x.mx is None else x.mx).device
        y = ops_half._empty(d.N, d.K, d.Ho, d.Wo, dev) if forms[0] else None
        ymx = torch.empty(L.p3d_f8act_bytes(d.N * d.Ho * d.Wo, d.K), dtype=torch.uint8, device=dev) if forms[1] else None
        tail = ops._p(mask_in), ops._p(mult), ops._p(res), int(bool(relu)), ops._p(y)
        if self.MX_ENTRY:
            check(L.p3d_f8conv2d_fwd_infer_mx(ctypes.byref(d), ops._p(x.h) if x.mx is None else None, ops._p(x.mx), self._at(c.img_off), self._at(c.bias_off),
                                              *tail, ops._p(ymx), ops._stream()), 'p3d_f8conv2d_fwd_infer_mx')
        else:
            check(L.p3d_f8conv2d_fwd_infer(ctypes.byref(d), ops._p(x.h), self._at(c.img_off), self._at(c.bias_off), *tail, ops._stream()),
                  'p3d_f8conv2d_fwd_infer')
        return _Act((d.N, d.K, d.Ho, d.Wo), y, ymx)


# ---- the same, with the activations between fp8 convs kept in MXFP8 ---------------------------------------------------------------------------
def resident_forms(chain, i, d, x_is_mx=True):
    """(fp16, mx): the forms in which conv i of a block's chain writes its result under fold_fp8(resident=True); d is its descriptor at the input it gets.
    Needs no device.  The block's output (the chain's last conv; the Fusion 1x1 is a chain of one) is written in both forms: it is the next block's input
    and its residual, a feature map, or what an fp16 head reads.  An interior result has one reader, the next conv of the chain: it is written as MX only
    when that conv is an fp8 conv whose entry point accepts it as MX, and as fp16 otherwise.  An fp16 conv, and an fp8 conv the entry point refuses an MX
    result (K % 32 != 0), write fp16 as they do without resident."""
    c = chain[i]
    if not isinstance(c, _F8Conv) or not _mx_supported(d, x_is_mx, 1):
        return True, False
    if i == len(chain) - 1:
        return True, True
    nxt = chain[i + 1]
    if isinstance(nxt, _F8Conv) and _mx_supported(nxt.desc(_Act((d.N, d.K, d.Ho, d.Wo))), 1, 0):
        return False, True
    return True, False


class Fp8ResidentNet(Fp8FoldedNet):
    """Fp8FoldedNet whose fp8 convs hand each other MXFP8 activation tensors (p3d_f8conv2d_fwd_infer_mx): a conv quantizes its result once, in its
    epilogue, and its readers copy the bytes.  Bit-equal to Fp8FoldedNet, since the block a producer writes is the block the reader would have made from
    the fp16 value.  The walk carries _Act objects; what comes from an fp16 kernel (the pool behind a stem, ops.relu under skip_relu, the concat) is fp16
    only, and the stems, the heads and the per-layer fallback always find an fp16 tensor (resident_forms)."""
    MX_ENTRY = True

    def _chain_conv(self, c, x, res=None, relu=False, veil=None, chain=None, i=0):
        """The result in the forms its readers take (resident_forms); the downsample shortcut's only reader is a residual operand, which is fp16."""
        forms = (True, False) if chain is None else resident_forms(chain, i, c.desc(x), x.mx is not None)
        mask_in = mult = mask_out = None
        if veil is not None:
            mult, mask_out = ops.mask_count(veil, c.r, c.stride, c.pad, c.dil)
            mask_in = veil.contiguous()
        return self._conv_act(c, x, forms, None if res is None else res.h, relu, mask_in, mult), mask_out

    def _pool(self, x):
        return _Act.of(super()._pool(x))

    def _fusion(self, x, y):
        return self._chain_conv(self.fusion, _Act.of(ops_half.concat(x.h, y.h)), relu=True, chain=[self.fusion])[0]

    def _relu(self, x):
        return _Act.of(ops.relu(x.h))

    def _head(self, c, x):
        return super()._head(c, x.h)

    @staticmethod
    def _out(x):
        return HalfFoldedNet._out(x.h if isinstance(x, _Act) else x)


def fp8_resident_enabled():
    """P3D_FOLDED_EVAL_FP8_RESIDENT=1, which acts only together with P3D_FOLDED_EVAL_FP8=1: the fp8 fold keeps its activations in MXFP8 between the
    fp8 convs (fold_fp8(model, resident=True))."""
    return fp8_enabled() and os.environ.get('P3D_FOLDED_EVAL_FP8_RESIDENT', '0') == '1'


def fold_fp8(model, resident=False):
    """Fp8FoldedNet of a network in eval mode (fp32 or -half_acc): fp32 (or fp16) NCHW input, fp32 NCHW outputs.  Raises P3DError for a BatchNorm in
    training mode or parameters that are not fp32 on the HIP device.  resident=True: an Fp8ResidentNet, the same outputs bit for bit with the activations
    between fp8 convs kept as MXFP8 tensors (profiles/eval_folded_fp8_resident.md)."""
    return (Fp8ResidentNet if resident else Fp8FoldedNet)(getattr(model, 'module', model))
