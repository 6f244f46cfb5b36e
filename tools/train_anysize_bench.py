#!/usr/bin/env python3
"""Training at the default 257^2 crop with ops.x3_any on and off: ResNet-50 depthnet, stride 16, batch 64 (profiles/train_anysize.md).

  --classes   per conv class of the trunk at its odd map (65 / 33 / 17): p3d_conv2d_fwd, p3d_conv2d_dgrad and p3d_conv2d_wgrad timed with device events, the switch
              on and off alternating within one process, --rounds rounds of --iters launches each.  One line per class and pass: median ms [min .. max] of both legs,
              which kernel family each leg ran on (the library's launch counters), the ratio; then the sums weighted by the layers per class.
  --step      the whole training step at --side (default 257): legs `off` and `on` alternating, --rounds rounds of --iters steps after --warmup, median [min .. max]
              ms per step of each leg, the launch counts per step and pass of both legs, and the verdict: `on` wins when its median is below `off`'s by more than the
              two legs' combined spread (max - min).  On a build without ops.x3_any (the parent commit) only the `off` leg runs.
  --family    depthnet (default: the above), partial_depthnet or partial_fusionnet (profiles/train_anysize_partial.md).  For the partial families --step runs three
              legs -- `off`, `any` (ops.x3_any) and `both` (ops.x3_any and ops.x3_any_partial) -- and `both` wins when it beats `any` by more than their combined
              spread; --classes times the masked convolutions of layer1 / layer2 (both factors, no bias) on the fp32-MFMA masked kernels, on the masked ragged
              x3 instances, and the dense convolution of the same shape on the dense ragged instances.
  --images    (depthnet; profiles/train_anysize_images.md) the image-fed ragged path, ops.x3_any_images.  With --classes: every stride-1 3x3 class with 96 channels or more
              on both sides, leg `any` (p3d_conv2d_* under ops.x3_any: the fp32-fed ragged instances) against leg `img` (p3d_fx_conv_*_img_any on activation images and
              cached weight images, as ops_block.ConvImagesFn calls them), each pass alone, the image passes of x and dy on lines of their own and inside a per-layer
              total.  With --step: legs `any` (ops.x3_any alone) and `images` (ops.x3_any and ops.x3_any_images) alternating; `images` wins when it beats `any` by more
              than their combined spread.  (The `any` leg of a build without ops.x3_any_images: --step without --images, whose `on` leg it is.)
  --strided   (depthnet; profiles/train_anysize_strided.md) stride-2 data gradients on the x3 kernels at the odd maps, ops.x3_any_strided.  With --classes: the four
              stride-2 classes of ResNet-50 through p3d_conv2d_dgrad, the switch off (the fp32-MFMA kernel and its interleave) and on (the class launches and
              dgrad_interleave_rows_kernel) alternating; then the finishing pass alone, p3d_dgrad_interleave kernel 0 against kernel 1 on the same planes, in ms and in
              TB/s of the bytes it has to move (the live planes read, dx written); the class launches are the call less its interleave.  With --step: legs `any`
              (ops.x3_any and ops.x3_any_images) and `strided` (those and ops.x3_any_strided) alternating, `strided` wins when it beats `any` by more than their
              combined spread; --frozen: the same two legs of the frozen-fold step (model.freeze_batchnorm(), ops.frozen_fold).
  --bn        (depthnet; profiles/bn_anysize.md) BatchNorm and the stem tail on the peeled 16-B instances at the odd maps, ops.bn_any.  With --classes: every
              (channels, map) of ResNet-50 at 257 -- p3d_bn_train_fwd (plain, ReLU, ReLU + residual), p3d_bn_train_bwd (ReLU with the recomputed mask; ReLU + residual),
              p3d_bn_eval_fwd / _bwd (ReLU) --, the switch off (the element-by-element instance) and on (the peeled one) alternating with the aligned neighbour map
              (128 / 64 / 32 / 16: the <true> instance, the yardstick), in ms and in TB/s of the tensors the pass has to read and write; then the stem at 64 x 129^2:
              the three nodes with the switch off and on against the fused tail, and the fused tail at 128^2.  With --step: legs `any` (ops.x3_any and
              ops.x3_any_images) and `bn` (those and ops.bn_any) alternating, `bn` wins when it beats `any` by more than their combined spread; --frozen: the two legs
              of the frozen step, --no-fold: without ops.frozen_fold (every frozen BatchNorm is then a p3d_bn_eval_fwd / _bwd pair).
  --block     (depthnet; profiles/block_anysize.md) the residual-block executor at the odd maps, ops.block_any.  With --classes: forward + backward of ONE block for each
              of ResNet-50's eight block geometries at 65 / 33 / 17 (batch --batch), legs `layer` (ops.x3_any, ops.x3_any_images and ops.bn_any: the per-layer path) and
              `block` (those and ops.block_any) alternating, median [min .. max] ms, and whether the executor takes the block.  With --step: legs `rec` (the recommended configuration
              without it: ops.x3_any, ops.x3_any_images and ops.bn_any) and `block` (those and ops.block_any) alternating; `block` wins when it beats `rec` by more than
              their combined spread.  Also the peak of allocated device memory of each leg's warm-up, the plan-owned buffers of the other leg released first.
  --block-strided  (with --block; profiles/block_anysize_strided.md) strided residual blocks at the odd maps, ops.block_any_strided.  With --classes: layer2.0 and
              layer3.0 of ResNet-50 and of ResNet-18 alone, legs `layer` (ops.x3_any, ops.x3_any_images, ops.bn_any and ops.block_any, which leaves these blocks to the
              per-layer path), `layer_x3s` (those and ops.x3_any_strided) and `block` (the first four and ops.block_any_strided) alternating; then
              block_strided_join_any_kernel alone on the two ResNet-50 shapes (p3d_block_strided_join) against dgrad_interleave_rows_kernel on the same planes, in ms
              and TB/s of the bytes each has to move.  With --step: legs `block` (the four switches) and `bstrided` (those and ops.block_any_strided) alternating;
              `bstrided` wins when it beats `block` by more than their combined spread.
GPU box only."""
import argparse
import ctypes
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module('3d-pose-estimation-with-previleged-information_amd')
ops = pkg.ops
PASSES = ('fwd', 'dgrad', 'wgrad')

# Cin, odd map, Cout, k, stride, dilation, layers of the class   (the dense convs behind the stem: tools/anysize_bench.py's table at the odd maps)
R50 = [(64, 65, 64, 1, 1, 1, 1), (64, 65, 64, 3, 1, 1, 3), (64, 65, 256, 1, 1, 1, 4), (256, 65, 64, 1, 1, 1, 2),
       (256, 65, 128, 1, 1, 1, 1), (128, 65, 128, 3, 2, 1, 1), (128, 33, 512, 1, 1, 1, 4), (256, 65, 512, 1, 2, 1, 1),
       (512, 33, 128, 1, 1, 1, 3), (128, 33, 128, 3, 1, 1, 3), (512, 33, 256, 1, 1, 1, 1), (256, 33, 256, 3, 2, 1, 1),
       (256, 17, 1024, 1, 1, 1, 6), (512, 33, 1024, 1, 2, 1, 1), (1024, 17, 256, 1, 1, 1, 5), (256, 17, 256, 3, 1, 1, 5),
       (1024, 17, 512, 1, 1, 1, 1), (512, 17, 512, 3, 1, 2, 1), (512, 17, 2048, 1, 1, 1, 3), (1024, 17, 2048, 1, 1, 1, 1),
       (2048, 17, 512, 1, 1, 1, 2), (512, 17, 512, 3, 1, 1, 2), (2048, 17, 272, 3, 1, 1, 1)]


# the PartialConvs of ResNet-50's layer1 / layer2 (partial_depthnet, partial_fusionnet: the shortcuts are dense), same columns
R50_PARTIAL = [(64, 65, 64, 1, 1, 1, 1), (64, 65, 64, 3, 1, 1, 3), (64, 65, 256, 1, 1, 1, 3), (256, 65, 64, 1, 1, 1, 2),
               (256, 65, 128, 1, 1, 1, 1), (128, 65, 128, 3, 2, 1, 1), (128, 33, 512, 1, 1, 1, 4), (512, 33, 128, 1, 1, 1, 3), (128, 33, 128, 3, 1, 1, 3)]
FAMILY_FLAGS = {'depthnet': [], 'partial_depthnet': ['-depth_only', '-partial_conv'], 'partial_fusionnet': ['-do_fusion', '-partial_conv']}


def switch(on, partial=False):
    if hasattr(ops, 'x3_any'):
        ops.x3_any(on)
    elif on:
        raise SystemExit('this build has no ops.x3_any')
    if hasattr(ops, 'x3_any_partial'):
        ops.x3_any_partial(partial)
    elif partial:
        raise SystemExit('this build has no ops.x3_any_partial')


def switch_leg(leg, strided=False):
    rec = leg in ('rec', 'block', 'bstrided')   # the recommended any-width configuration: x3_any, x3_any_images, bn_any
    switch(leg in ('on', 'any', 'both', 'images', 'strided', 'bn') or rec, leg == 'both')
    if hasattr(ops, 'bn_any'):
        ops.bn_any(leg == 'bn' or rec)
    elif leg == 'bn' or rec:
        raise SystemExit('this build has no ops.bn_any')
    if hasattr(ops, 'x3_any_images'):
        ops.x3_any_images(leg == 'images' or strided or rec)
    elif leg == 'images' or rec:
        raise SystemExit('this build has no ops.x3_any_images')
    if hasattr(ops, 'block_any'):
        ops.block_any(leg in ('block', 'bstrided'))
    elif leg in ('block', 'bstrided'):
        raise SystemExit('this build has no ops.block_any')
    if hasattr(ops, 'block_any_strided'):
        ops.block_any_strided(leg == 'bstrided')
    elif leg == 'bstrided':
        raise SystemExit('this build has no ops.block_any_strided')
    if hasattr(ops, 'x3_any_strided'):
        ops.x3_any_strided(leg == 'strided')
    elif leg == 'strided':
        raise SystemExit('this build has no ops.x3_any_strided')


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def med(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def family(stats, name):
    return 'x3' if stats['x3'][name][0] else 'fp32'


def classes(a):
    L = pkg._lib.lib()
    total = {(p, leg): 0.0 for p in PASSES for leg in ('off', 'on')}
    for (c, h, k, ks, st, dil, cnt) in sorted(R50, key=lambda r: -r[0] * r[2] * r[3] ** 2 * ((r[1] // r[4] + 1) ** 2) * r[6]):
        tag = 'c%d h%d k%d %dx%d s%d d%d x%d' % (c, h, k, ks, ks, st, dil, cnt)
        if a.only and a.only not in tag:
            continue
        torch.manual_seed(c + k)
        pad = dil * (ks - 1) // 2
        x = torch.randn(a.batch, c, h, h, device='cuda')
        w = torch.randn(k, c, ks, ks, device='cuda') / (c * ks * ks) ** 0.5
        d = ops._desc(x.shape, w.shape, st, pad, dil)
        dy = torch.randn(a.batch, k, d.Ho, d.Wo, device='cuda')
        y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w)
        b = ctypes.byref(d)
        switch(True)                                             # (the larger plan: one workspace serves both legs)
        ws = torch.empty(max(L.p3d_conv2d_fwd_workspace_bytes(b), L.p3d_conv2d_dgrad_workspace_bytes(b), L.p3d_conv2d_wgrad_workspace_bytes(b), 16), dtype=torch.uint8, device='cuda')
        switch(False)
        P, stream = ops._p, ops._stream()
        calls = {'fwd': lambda: L.p3d_conv2d_fwd(b, P(x), P(w), None, None, None, P(y), P(ws), ws.numel(), stream),
                 'dgrad': lambda: L.p3d_conv2d_dgrad(b, P(dy), P(w), None, None, P(dx), P(ws), ws.numel(), stream),
                 'wgrad': lambda: L.p3d_conv2d_wgrad(b, P(dy), P(x), None, None, P(dw), P(ws), ws.numel(), stream)}
        gf = 2.0 * a.batch * k * c * ks * ks * d.Ho * d.Wo / 1e9
        for name, fn in calls.items():
            ms, ran = {'off': [], 'on': []}, {}
            for leg in ('off', 'on'):
                switch(leg == 'on')
                ops.conv_path_stats(reset=True)
                for _ in range(3):
                    assert fn() == 0, pkg._lib.lib().p3d_last_error()
                ran[leg] = family(ops.conv_path_stats(reset=True), name)
            for _ in range(a.rounds):
                for leg in ('off', 'on'):
                    switch(leg == 'on')
                    ms[leg].append(timed(fn, a.iters))
            switch(False)
            assert ran['off'] == 'fp32', (tag, name, ran)
            m0, m1 = med(ms['off']), med(ms['on'])
            print('%-28s %-5s %7.2f GF | off %-4s %.3f [%.3f..%.3f] ms %5.1f TF | on %-4s %.3f [%.3f..%.3f] ms %5.1f TF | on/off %.2f' % (
                (tag, name, gf, ran['off']) + m0 + (gf / m0[0], ran['on']) + m1 + (gf / m1[0], m1[0] / m0[0])), flush=True)
            total[(name, 'off')] += m0[0] * cnt
            total[(name, 'on')] += m1[0] * cnt
    for name in PASSES:
        print('sum over the classes x their layer counts, %-5s: off %.2f ms  on %.2f ms' % (name, total[(name, 'off')], total[(name, 'on')]))
    print('all three passes: off %.2f ms  on %.2f ms' % (sum(total[(p, 'off')] for p in PASSES), sum(total[(p, 'on')] for p in PASSES)))


def classes_partial(a):
    """the masked classes: leg `fp32` (the switch off), `x3` (ops.x3_any_partial on), `dense` (the same shape without factors under ops.x3_any)"""
    L = pkg._lib.lib()
    legs = ('fp32', 'x3', 'dense')
    total = {(p, leg): 0.0 for p in PASSES for leg in legs}
    for (c, h, k, ks, st, dil, cnt) in sorted(R50_PARTIAL, key=lambda r: -r[0] * r[2] * r[3] ** 2 * ((r[1] // r[4] + 1) ** 2) * r[6]):
        tag = 'c%d h%d k%d %dx%d s%d d%d x%d' % (c, h, k, ks, ks, st, dil, cnt)
        if a.only and a.only not in tag:
            continue
        torch.manual_seed(c + k)
        pad = dil * (ks - 1) // 2
        x = torch.randn(a.batch, c, h, h, device='cuda')
        w = torch.randn(k, c, ks, ks, device='cuda') / (c * ks * ks) ** 0.5
        m = (torch.rand(a.batch, 1, h, h, device='cuda') >= 0.3).float()
        mult, _ = ops.mask_count(m, ks, st, pad, dil)
        d = ops._desc(x.shape, w.shape, st, pad, dil)
        dy = torch.randn(a.batch, k, d.Ho, d.Wo, device='cuda')
        y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w)
        b = ctypes.byref(d)
        switch(True, True)                                       # (the largest plan: one workspace serves every leg)
        ws = torch.empty(max(L.p3d_conv2d_fwd_workspace_bytes(b), L.p3d_conv2d_dgrad_workspace_bytes(b), L.p3d_conv2d_wgrad_workspace_bytes(b), 16), dtype=torch.uint8, device='cuda')
        switch(False)
        P, stream = ops._p, ops._stream()

        def calls(masked):
            mi, mu = (P(m), P(mult)) if masked else (None, None)
            return {'fwd': lambda: L.p3d_conv2d_fwd(b, P(x), P(w), None, mi, mu, P(y), P(ws), ws.numel(), stream),
                    'dgrad': lambda: L.p3d_conv2d_dgrad(b, P(dy), P(w), mu, mi, P(dx), P(ws), ws.numel(), stream),
                    'wgrad': lambda: L.p3d_conv2d_wgrad(b, P(dy), P(x), mu, mi, P(dw), P(ws), ws.numel(), stream)}

        def set_leg(leg):
            switch(leg == 'dense', leg == 'x3')

        gf = 2.0 * a.batch * k * c * ks * ks * d.Ho * d.Wo / 1e9
        for name in PASSES:
            fns = {leg: calls(leg != 'dense')[name] for leg in legs}
            ms, ran = {leg: [] for leg in legs}, {}
            for leg in legs:
                set_leg(leg)
                ops.conv_path_stats(reset=True)
                for _ in range(3):
                    assert fns[leg]() == 0, pkg._lib.lib().p3d_last_error()
                ran[leg] = family(ops.conv_path_stats(reset=True), name)
            for _ in range(a.rounds):
                for leg in legs:
                    set_leg(leg)
                    ms[leg].append(timed(fns[leg], a.iters))
            switch(False)
            assert ran['fp32'] == 'fp32', (tag, name, ran)
            m0, m1, m2 = med(ms['fp32']), med(ms['x3']), med(ms['dense'])
            print('%-28s %-5s %7.2f GF | masked off %-4s %.3f [%.3f..%.3f] ms | masked on %-4s %.3f [%.3f..%.3f] ms | dense %-4s %.3f [%.3f..%.3f] ms | on/off %.2f  on/dense %.2f' % (
                (tag, name, gf, ran['fp32']) + m0 + (ran['x3'],) + m1 + (ran['dense'],) + m2 + (m1[0] / m0[0], m1[0] / m2[0])), flush=True)
            for leg, mm in zip(legs, (m0, m1, m2)):
                total[(name, leg)] += mm[0] * cnt
    for name in PASSES:
        print('sum over the classes x their layer counts, %-5s: masked off %.2f ms  masked on %.2f ms  dense %.2f ms' % ((name,) + tuple(total[(name, leg)] for leg in legs)))
    print('all three passes: masked off %.2f ms  masked on %.2f ms  dense %.2f ms' % tuple(sum(total[(p, leg)] for p in PASSES) for leg in legs))


def classes_images(a):
    """the classes ops_block.ConvImagesFn takes at the odd maps under ops.x3_any_images: leg `any` (fp32-fed ragged, per-layer entries) against leg `img`"""
    L = pkg._lib.lib()
    legs = ('any', 'img')
    rows = ('fwd', 'dgrad', 'wgrad', 'img x', 'img dy')
    total = {(r, leg): 0.0 for r in rows for leg in legs}
    P, stream = ops._p, ops._stream()
    for (c, h, k, ks, st, dil, cnt) in sorted(R50, key=lambda r: -r[0] * r[2] * r[3] ** 2 * ((r[1] // r[4] + 1) ** 2) * r[6]):
        tag = 'c%d h%d k%d %dx%d s%d d%d x%d' % (c, h, k, ks, ks, st, dil, cnt)
        if ks < 2 or st != 1 or min(c, k) < 96 or (a.only and a.only not in tag):
            continue
        torch.manual_seed(c + k)
        pad = dil * (ks - 1) // 2
        conv = pkg.nn.Conv2d(c, k, ks, stride=st, padding=pad, dilation=dil, bias=False).cuda()
        w = conv.weight.detach()
        x = torch.randn(a.batch, c, h, h, device='cuda')
        d = ops._desc(x.shape, w.shape, st, pad, dil)
        b = ctypes.byref(d)
        assert L.p3d_fx_conv_img_supported(b) == 0 and L.p3d_fx_conv_img_any_supported(b) == 7, tag
        dy = torch.randn(a.batch, k, d.Ho, d.Wo, device='cuda')
        y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w)
        switch(True)
        ws = torch.empty(max([L.p3d_conv2d_fwd_workspace_bytes(b), L.p3d_conv2d_dgrad_workspace_bytes(b), L.p3d_conv2d_wgrad_workspace_bytes(b), 16] +
                             [L.p3d_fx_conv_img_any_workspace_bytes(b, i) for i in range(3)]), dtype=torch.uint8, device='cuda')
        wf, wb = pkg.ops_block.weight_images(conv)
        x_img, dy_img = ops.act_image(x), ops.act_image(dy)
        calls = {('fwd', 'any'): lambda: L.p3d_conv2d_fwd(b, P(x), P(w), None, None, None, P(y), P(ws), ws.numel(), stream),
                 ('dgrad', 'any'): lambda: L.p3d_conv2d_dgrad(b, P(dy), P(w), None, None, P(dx), P(ws), ws.numel(), stream),
                 ('wgrad', 'any'): lambda: L.p3d_conv2d_wgrad(b, P(dy), P(x), None, None, P(dw), P(ws), ws.numel(), stream),
                 ('fwd', 'img'): lambda: L.p3d_fx_conv_fwd_img_any(b, P(x_img), P(w), P(wf), None, P(y), P(ws), ws.numel(), stream),
                 ('dgrad', 'img'): lambda: L.p3d_fx_conv_dgrad_img_any(b, P(dy_img), P(w), P(wb), P(dx), P(ws), ws.numel(), stream),
                 ('wgrad', 'img'): lambda: L.p3d_fx_conv_wgrad_img_any(b, P(dy_img), None, P(x_img), P(dw), P(ws), ws.numel(), stream),
                 ('img x', 'img'): lambda: L.p3d_fx_act_image_any(P(x), P(x_img), a.batch, c, h * h, stream),
                 ('img dy', 'img'): lambda: L.p3d_fx_act_image_any(P(dy), P(dy_img), a.batch, k, d.Ho * d.Wo, stream)}
        gf = 2.0 * a.batch * k * c * ks * ks * d.Ho * d.Wo / 1e9
        layer = {leg: 0.0 for leg in legs}
        for row in rows:
            ms = {leg: [] for leg in legs if (row, leg) in calls}
            for leg in ms:
                ops.conv_path_stats(reset=True)
                for _ in range(3):
                    assert calls[(row, leg)]() == 0, L.p3d_last_error()
                if row in PASSES:
                    assert family(ops.conv_path_stats(reset=True), row) == 'x3', (tag, row, leg)
            for _ in range(a.rounds):
                for leg in ms:
                    ms[leg].append(timed(calls[(row, leg)], a.iters))
            m = {leg: med(v) for leg, v in ms.items()}
            text = ' | '.join('%s %.3f [%.3f..%.3f] ms' % ((leg,) + m[leg]) for leg in m)
            ratio = ' | img/any %.2f' % (m['img'][0] / m['any'][0]) if 'any' in m else ''
            print('%-28s %-6s %7.2f GF | %s%s' % (tag, row, gf if row in PASSES else 0.0, text, ratio), flush=True)
            for leg in m:
                layer[leg] += m[leg][0]
                total[(row, leg)] += m[leg][0] * cnt
        print('%-28s layer  any %.3f ms  img %.3f ms (image passes included)  img/any %.2f' % (tag, layer['any'], layer['img'], layer['img'] / layer['any']), flush=True)
        switch(False)
    for row in rows:
        print('sum over the classes x their layer counts, %-6s: any %.2f ms  img %.2f ms' % (row, total[(row, 'any')], total[(row, 'img')]))
    print('all passes: any %.2f ms  img %.2f ms' % (sum(total[(r, 'any')] for r in rows), sum(total[(r, 'img')] for r in rows)))


def classes_strided(a):
    """the stride-2 data gradients of ResNet-50 at the odd maps: the call with ops.x3_any_strided off and on, and the two interleave kernels alone"""
    L = pkg._lib.lib()
    P, stream = ops._p, ops._stream()
    total = {'off': 0.0, 'on': 0.0}
    for (c, h, k, ks, st, dil, cnt) in R50:
        tag = 'c%d h%d k%d %dx%d s%d' % (c, h, k, ks, ks, st)
        if st != 2 or (a.only and a.only not in tag):
            continue
        torch.manual_seed(c + k)
        x_shape, w = (a.batch, c, h, h), torch.randn(k, c, ks, ks, device='cuda') / (k * ks * ks) ** 0.5
        d = ops._desc(x_shape, w.shape, st, ks // 2, 1)
        b = ctypes.byref(d)
        assert L.p3d_conv2d_dgrad_strided_any_supported(b) == 1, tag
        dy, dx = torch.randn(a.batch, k, d.Ho, d.Wo, device='cuda'), torch.empty(x_shape, device='cuda')
        ops.x3_any_strided(True)
        ws = torch.empty(L.p3d_conv2d_dgrad_workspace_bytes(b), dtype=torch.uint8, device='cuda')
        fn = lambda: L.p3d_conv2d_dgrad(b, P(dy), P(w), None, None, P(dx), P(ws), ws.numel(), stream)
        # the finishing pass alone, on planes of its own
        hc = (h + 1) // 2
        cls_stride = (a.batch * c * hc * hc + 3) // 4 * 4
        stage = torch.randn(4 * cls_stride, device='cuda')
        live = 0b1111 if ks > 1 else 0b0001
        pixels = h * h if ks > 1 else hc * hc
        nbytes = 4.0 * a.batch * c * (pixels + h * h)           # the live planes read, dx written
        fin = {kern: (lambda kern=kern: L.p3d_dgrad_interleave(kern, P(stage), P(dx), None, a.batch, c, h, h, cls_stride, live, 0, stream)) for kern in (0, 1)}
        ms, ran = {leg: [] for leg in ('off', 'on', 0, 1)}, {}
        for leg in ('off', 'on'):
            ops.x3_any_strided(leg == 'on')
            ops.conv_path_stats(reset=True)
            for _ in range(3):
                assert fn() == 0, L.p3d_last_error()
            ran[leg] = family(ops.conv_path_stats(reset=True), 'dgrad')
        for kern in (0, 1):
            for _ in range(3):
                assert fin[kern]() == 0, L.p3d_last_error()
        assert (ran['off'], ran['on']) == ('fp32', 'x3'), (tag, ran)
        for _ in range(a.rounds):
            for leg in ('off', 'on'):
                ops.x3_any_strided(leg == 'on')
                ms[leg].append(timed(fn, a.iters))
            for kern in (0, 1):
                ms[kern].append(timed(fin[kern], a.iters))
        ops.x3_any_strided(False)
        gf = 2.0 * a.batch * k * c * ks * ks * d.Ho * d.Wo / 1e9
        m = {leg: med(v) for leg, v in ms.items()}
        print('%-24s dgrad %7.2f GF | off %.3f [%.3f..%.3f] ms %5.1f TF | on %.3f [%.3f..%.3f] ms %5.1f TF | on/off %.2f' % (
            (tag, gf) + m['off'] + (gf / m['off'][0],) + m['on'] + (gf / m['on'][0], m['on'][0] / m['off'][0])), flush=True)
        print('%-24s interleave %6.1f MB | kernel 0 %.3f [%.3f..%.3f] ms %.2f TB/s | kernel 1 %.3f [%.3f..%.3f] ms %.2f TB/s | 1/0 %.2f' % (
            (tag, nbytes / 1e6) + m[0] + (nbytes / m[0][0] / 1e9,) + m[1] + (nbytes / m[1][0] / 1e9, m[1][0] / m[0][0])), flush=True)
        print('%-24s the call less its interleave | off %.3f ms %5.1f TF | on (weight image + class launches) %.3f ms %5.1f TF' % (
            tag, m['off'][0] - m[0][0], gf / (m['off'][0] - m[0][0]), m['on'][0] - m[1][0], gf / (m['on'][0] - m[1][0])), flush=True)
        total['off'] += m['off'][0] * cnt
        total['on'] += m['on'][0] * cnt
    print('sum over the classes x their layer counts, dgrad: off %.3f ms  on %.3f ms' % (total['off'], total['on']))


# channels, odd map of ResNet-50 depthnet at 257 (its aligned neighbour is the map less one)
BN_R50 = [(64, 129), (64, 65), (128, 65), (256, 65), (128, 33), (256, 33), (512, 33), (256, 17), (512, 17), (1024, 17), (2048, 17)]
INSTANCE = {0: 'vector', 1: 'scalar', 2: 'peeled'}


def classes_bn(a):
    """every BatchNorm class of ResNet-50 at the odd maps: the entries with ops.bn_any off and on and at the aligned neighbour map; then the stem"""
    L = pkg._lib.lib()
    P, stream = ops._p, ops._stream()
    legs = ('off', 'on', 'aligned')
    total = {leg: 0.0 for leg in legs}
    for (c, h) in BN_R50:
        tag = 'c%d %dx%d' % (c, h, h)
        if a.only and a.only not in tag:
            continue
        torch.manual_seed(c + h)
        gamma, beta = torch.rand(c, device='cuda') + 0.5, torch.randn(c, device='cuda')
        mean, invstd, dgamma, dbeta = (torch.empty(c, device='cuda') for _ in range(4))
        ws = torch.empty(L.p3d_bn_workspace_bytes(a.batch, c, h * h), dtype=torch.uint8, device='cuda')
        calls = {}
        for leg, side in (('odd', h), ('aligned', h - 1)):
            n, hw = a.batch, side * side
            x, res, dy = (torch.randn(n, c, side, side, device='cuda') for _ in range(3))
            y, dx, dres = (torch.empty_like(x) for _ in range(3))
            rm, rv = torch.zeros(c, device='cuda'), torch.ones(c, device='cuda')
            t = 4.0 * x.numel()

            def make(x=x, res=res, dy=dy, y=y, dx=dx, dres=dres, rm=rm, rv=rv, n=n, hw=hw, t=t):
                fwd = lambda r, relu: (lambda: L.p3d_bn_train_fwd(P(x), P(r), P(gamma), P(beta), P(rm), P(rv), P(y), P(mean), P(invstd), n, c, hw, 0.1, 1e-5, relu,
                                                                  P(ws), ws.numel(), stream))
                bwd = lambda yy, dr: (lambda: L.p3d_bn_train_bwd(P(dy), P(x), P(yy), P(gamma), P(beta), P(mean), P(invstd), P(dx), P(dr), P(dgamma), P(dbeta), n, c, hw,
                                                                 1, 0, P(ws), ws.numel(), stream))
                # the pass and the bytes it has to move: x is read by both kernels of a training pass, dy / x / y by both of a backward pass
                return [('train_fwd plain', fwd(None, 0), 3 * t), ('train_fwd relu', fwd(None, 1), 3 * t), ('train_fwd relu+res', fwd(res, 1), 4 * t),
                        ('train_bwd relu', bwd(None, None), 5 * t), ('train_bwd relu+res', bwd(y, dres), 8 * t),
                        ('eval_fwd relu', lambda: L.p3d_bn_eval_fwd(P(x), None, P(gamma), P(beta), P(rm), P(rv), P(y), n, c, hw, 1e-5, 1, stream), 2 * t),
                        ('eval_bwd relu', lambda: L.p3d_bn_eval_bwd(P(dy), P(x), P(y), P(gamma), P(rm), P(rv), P(dx), None, P(dgamma), P(dbeta), n, c, hw, 1e-5, 1, 0,
                                                                    P(ws), ws.numel(), stream), 7 * t)]
            calls[leg] = make()
        for i, (name, _, _) in enumerate(calls['odd']):
            fns = {'off': calls['odd'][i], 'on': calls['odd'][i], 'aligned': calls['aligned'][i]}
            ms, ran = {leg: [] for leg in legs}, {}
            for leg in legs:
                ops.bn_any(leg == 'on')
                for _ in range(3):
                    assert fns[leg][1]() == 0, L.p3d_last_error()
                ran[leg] = ops.bn_last_launch()['instance']
            assert (ran['off'], ran['on'], ran['aligned']) == (1, 2, 0), (tag, name, ran)
            for _ in range(a.rounds):
                for leg in legs:
                    ops.bn_any(leg == 'on')
                    ms[leg].append(timed(fns[leg][1], a.iters))
            ops.bn_any(False)
            m = {leg: med(ms[leg]) for leg in legs}
            spread = (m['off'][2] - m['off'][1]) + (m['on'][2] - m['on'][1])
            verdict = 'on wins' if m['off'][0] - m['on'][0] > spread else 'on LOSES' if m['on'][0] - m['off'][0] > spread else 'tie'
            print('%-14s %-18s | off %.3f [%.3f..%.3f] ms %.2f TB/s | on %.3f [%.3f..%.3f] ms %.2f TB/s | aligned %dx%d %.3f [%.3f..%.3f] ms %.2f TB/s | on/off %.2f  %s' % (
                (tag, name) + m['off'] + (fns['off'][2] / m['off'][0] / 1e9,) + m['on'] + (fns['on'][2] / m['on'][0] / 1e9,) + (h - 1, h - 1) + m['aligned'] +
                (fns['aligned'][2] / m['aligned'][0] / 1e9, m['on'][0] / m['off'][0], verdict)), flush=True)
            for leg in legs:
                total[leg] += m[leg][0]
        del calls
        torch.cuda.empty_cache()
    print('sum over the classes and passes (one of each): off %.2f ms  on %.2f ms  aligned neighbours %.2f ms' % (total['off'], total['on'], total['aligned']))
    if a.only and a.only != 'stem':
        return
    # the stem: maxpool(relu(bn(c))) forward + backward through autograd, as the network runs it
    pool = pkg.nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
    bn = pkg.nn.BatchNorm2d(64).cuda().train()
    legs = (('nodes off', 129, False, False), ('nodes on', 129, True, False), ('fused on', 129, True, True), ('fused 128x128', 128, False, True))
    data = {}
    for side in (129, 128):
        x = torch.randn(a.batch, 64, side, side, device='cuda').requires_grad_(True)
        data[side] = (x, torch.randn(a.batch, 64, (side - 1) // 2 + 1, (side - 1) // 2 + 1, device='cuda'))

    def run(leg, backward):
        name, side, on, fused = leg
        x, dy = data[side]
        ops.bn_any(on)
        assert ops.stem_tail_usable(x, bn, pool) == (on or side == 128), leg
        y = ops.stem_tail(x, bn) if fused else pool(bn(x, relu=True))
        if backward:
            x.grad = bn.weight.grad = bn.bias.grad = None
            y.backward(dy)
    for backward in (False, True):
        ms = {leg: [] for leg in legs}
        for leg in legs:
            for _ in range(3):
                run(leg, backward)
        for _ in range(a.rounds):
            for leg in legs:
                ms[leg].append(timed(lambda: run(leg, backward), a.iters))
        ops.bn_any(False)
        for leg in legs:
            x, dy = data[leg[1]]
            moved = 4.0 * (2 * x.numel() + dy.numel()) + dy.numel()                     # forward: x twice, the pooled map and the argmax bytes
            if backward:
                moved += 4.0 * (3 * x.numel() + 2 * dy.numel()) + 2 * dy.numel()        # backward: x twice, dx, the pooled gradient and the bytes twice
            m = med(ms[leg])
            print('stem 64 ch, %s %-14s | %.3f [%.3f..%.3f] ms  %.2f TB/s of what the fused node has to move' % (
                ('forward + backward' if backward else 'forward           ', leg[0]) + m + (moved / m[0] / 1e9,)), flush=True)


# name, inplanes, planes, stride, dilation, odd map, downsample: ResNet-50's block geometries behind the stem at 257 (-stride 16)
R50_BLOCKS = [('layer1.0', 64, 64, 1, 1, 65, True), ('layer1.1', 256, 64, 1, 1, 65, False), ('layer2.0', 256, 128, 2, 1, 65, True), ('layer2.1', 512, 128, 1, 1, 33, False),
              ('layer3.0', 512, 256, 2, 1, 33, True), ('layer3.1', 1024, 256, 1, 1, 17, False), ('layer4.0', 1024, 512, 1, 2, 17, True), ('layer4.1', 2048, 512, 1, 1, 17, False)]


# the strided blocks at 257: layer2.0 and layer3.0 of ResNet-50 (Bottleneck) and of ResNet-18 (BasicBlock), same columns with the block class in front
STRIDED_BLOCKS = [('bottleneck', 'r50.layer2.0', 256, 128, 2, 1, 65, True), ('bottleneck', 'r50.layer3.0', 512, 256, 2, 1, 33, True),
                  ('basic', 'r18.layer2.0', 64, 128, 2, 1, 65, True), ('basic', 'r18.layer3.0', 128, 256, 2, 1, 33, True)]


def classes_block(a):
    tr = pkg._trunk
    blocks = STRIDED_BLOCKS if a.block_strided else [('bottleneck',) + b for b in R50_BLOCKS]
    for kind, name, inplanes, planes, stride, dil, h, with_ds in blocks:
        if a.only and a.only not in name:
            continue
        cls = tr.Bottleneck if kind == 'bottleneck' else tr.BasicBlock
        ds = tr.Sequential(pkg.nn.Conv2d(inplanes, planes * cls.expansion, kernel_size=1, stride=stride, bias=False), pkg.nn.BatchNorm2d(planes * cls.expansion)) if with_ds else None
        torch.manual_seed(1)
        block = cls(inplanes, planes, stride, dil, ds).cuda().train()
        x = torch.randn(a.batch, inplanes, h, h, device='cuda').relu_().requires_grad_(True)
        with torch.no_grad():
            dy = torch.randn(block(x).shape, device='cuda')

        def one():
            block.zero_grad(set_to_none=True)
            x.grad = None
            block(x).backward(dy)
            ops.join_side_stream()
        ms, takes = ({'layer': [], 'layer_x3s': [], 'block': []} if a.block_strided else {'layer': [], 'block': []}), {}
        for _ in range(a.rounds):
            for leg in ms:
                if a.block_strided:
                    switch_leg('bstrided' if leg == 'block' else 'block')
                    ops.x3_any_strided(leg == 'layer_x3s')
                else:
                    switch_leg('block' if leg == 'block' else 'rec')
                takes[leg] = bool(pkg.ops_block.usable(block, x))
                for _ in range(a.warmup):
                    one()
                torch.cuda.synchronize()
                ms[leg].append(timed(one, a.iters))
        switch_leg('off')
        out = {'block': name, 'map': h, 'batch': a.batch, 'executor_takes_it': takes['block']}
        for leg in ms:
            m = med(ms[leg])
            out[leg] = {'median_ms': round(m[0], 3), 'min_ms': round(m[1], 3), 'max_ms': round(m[2], 3)}
        print(json.dumps(out), flush=True)
        del block, x, dy
        torch.cuda.empty_cache()


def join_bandwidth(a):
    """block_strided_join_any_kernel alone against dgrad_interleave_rows_kernel on the same class planes: the gradient buffers in front of the strided 3x3 of
    ResNet-50's layer2.0 and layer3.0.  Bytes each has to move: the four planes read and g written -- the join reads c too."""
    L = pkg._lib.lib()
    for name, c, h in (('r50.layer2.0 da[0]', 128, 65), ('r50.layer3.0 da[0]', 256, 33)):
        n = a.batch
        cls_stride = (n * c * ((h + 1) // 2) ** 2 + 3) // 4 * 4
        stage, cc, g = torch.randn(4 * cls_stride, device='cuda'), torch.randn(n, c, h, h, device='cuda'), torch.empty(n, c, h, h, device='cuda')
        tab = torch.rand(c, 8, device='cuda')
        split = min(n, 64, -(-2048 // c))
        partial = torch.empty(c, split, 3, dtype=torch.float64, device='cuda')
        join = lambda: L.p3d_block_strided_join(ops._p(stage), ops._p(cc), ops._p(tab), ops._p(g), ops._p(partial), n, c, h, h, cls_stride, 15, split, ops._stream())
        inter = lambda: L.p3d_dgrad_interleave(1, ops._p(stage), ops._p(g), None, n, c, h, h, cls_stride, 15, 0, ops._stream())
        out = {'tensor': name, 'shape': [n, c, h, h]}
        for leg, fn, nbytes in (('interleave', inter, 8.0 * g.numel()), ('join', join, 12.0 * g.numel())):
            assert fn() == 0, L.p3d_last_error()
            ms = []
            for _ in range(a.rounds):
                timed(fn, a.warmup)
                ms.append(timed(fn, a.iters))
            m = med(ms)
            out[leg] = {'median_ms': round(m[0], 4), 'min_ms': round(m[1], 4), 'max_ms': round(m[2], 4), 'tb_per_s': round(nbytes / m[0] / 1e9, 2)}
        print(json.dumps(out), flush=True)


def step(a):
    flags = ['-model', a.model, '-suffix', 'bench', '-data_name', 'h36m', '-save_path', '/tmp/p3d_bench', '-criterion', 'SmoothL1', '-num_joints', '17', '-side_in', str(a.side),
             '-stride', '16', '-depth', '16', '-depth_range', '1000', '-loss_div', '10', '-learn_rate', '5e-5', '-weight_decay', '4e-5', '-grad_norm', '5'] + FAMILY_FLAGS[a.family]
    args = pkg.opts.parse(flags)
    torch.manual_seed(0)
    model, _ = pkg.depth_main.create_model(args)
    model = model.cuda().train()
    if a.frozen:
        model.freeze_batchnorm()
        ops.frozen_fold(not a.no_fold)
    trainer = pkg.depth_train.Trainer(args, model, pkg.utils.get_info())
    trainer.verbose = False
    trainer.adapt_learn_rate(1)
    batches = []
    for i in range(3):
        c, d, tc, tv = pkg.synth.make_batch(a.batch, side=a.side, rank=0, step=i)
        batches.append((torch.from_numpy(c).cuda(), None if a.family == 'depthnet' else torch.from_numpy(d).cuda(), torch.from_numpy(tc).cuda(), torch.from_numpy(tv).cuda()))
    legs = ('off', 'on') if hasattr(ops, 'x3_any') and not a.off_only else ('off',)
    if a.family != 'depthnet' and len(legs) == 2:
        legs = ('off', 'any', 'both') if hasattr(ops, 'x3_any_partial') else ('off', 'any')
    if a.images:
        legs = ('any', 'images')
    if a.strided:
        legs = ('any', 'strided')
    if a.bn:
        legs = ('any', 'bn')
    if a.block:
        legs = ('block', 'bstrided') if a.block_strided else ('rec', 'block')

    def run(n):
        for i in range(n):
            trainer.train_step(*batches[i % 3])
        ops.join_side_stream()

    ms, counts, peak = {leg: [] for leg in legs}, {}, {}
    for leg in legs:
        switch_leg(leg, a.strided or a.bn)
        if a.block:
            torch.cuda.synchronize()
            pkg.ops_block.release_buffers(model)
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
        run(a.warmup)
        torch.cuda.synchronize()
        peak[leg] = round(torch.cuda.max_memory_allocated() / 2 ** 20)
        ops.conv_path_stats(reset=True)
        run(1)
        torch.cuda.synchronize()
        st = ops.conv_path_stats(reset=True)
        counts[leg] = {fam: {p: st[fam][p][0] for p in PASSES} for fam in ('x3', 'fp32')}
    for r in range(a.rounds):
        for leg in legs:
            switch_leg(leg, a.strided or a.bn)
            run(2)
            torch.cuda.synchronize()
            ms[leg].append(timed(lambda: run(a.iters), 1) / a.iters)
            print('round %d %-3s %.3f ms/step' % (r, leg, ms[leg][-1]), flush=True)
    switch_leg('off')
    out = {'side': a.side, 'batch': a.batch, 'model': a.model, 'launches_per_step': counts}
    if a.frozen:
        out['frozen_fold'] = not a.no_fold
        ops.frozen_fold(False)
    if a.family != 'depthnet':
        out['family'] = a.family
    for leg in legs:
        m = med(ms[leg])
        out[leg] = {'median_ms': round(m[0], 3), 'min_ms': round(m[1], 3), 'max_ms': round(m[2], 3)}
    if legs == ('rec', 'block'):
        spread = (out['rec']['max_ms'] - out['rec']['min_ms']) + (out['block']['max_ms'] - out['block']['min_ms'])
        out['gain_ms'] = round(out['rec']['median_ms'] - out['block']['median_ms'], 3)
        out['combined_spread_ms'] = round(spread, 3)
        out['block_wins'] = bool(out['gain_ms'] > spread)
        out['peak_allocated_mib'] = peak
    elif legs == ('block', 'bstrided'):
        spread = (out['block']['max_ms'] - out['block']['min_ms']) + (out['bstrided']['max_ms'] - out['bstrided']['min_ms'])
        out['gain_ms'] = round(out['block']['median_ms'] - out['bstrided']['median_ms'], 3)
        out['combined_spread_ms'] = round(spread, 3)
        out['bstrided_wins'] = bool(out['gain_ms'] > spread)
        out['peak_allocated_mib'] = peak
    elif legs == ('off', 'any', 'both'):
        spread = (out['any']['max_ms'] - out['any']['min_ms']) + (out['both']['max_ms'] - out['both']['min_ms'])
        out['gain_ms'] = round(out['any']['median_ms'] - out['both']['median_ms'], 3)
        out['combined_spread_ms'] = round(spread, 3)
        out['both_wins'] = bool(out['gain_ms'] > spread)
    elif legs == ('any', 'images'):
        spread = (out['any']['max_ms'] - out['any']['min_ms']) + (out['images']['max_ms'] - out['images']['min_ms'])
        out['gain_ms'] = round(out['any']['median_ms'] - out['images']['median_ms'], 3)
        out['combined_spread_ms'] = round(spread, 3)
        out['images_wins'] = bool(out['gain_ms'] > spread)
    elif legs == ('any', 'strided'):
        spread = (out['any']['max_ms'] - out['any']['min_ms']) + (out['strided']['max_ms'] - out['strided']['min_ms'])
        out['gain_ms'] = round(out['any']['median_ms'] - out['strided']['median_ms'], 3)
        out['combined_spread_ms'] = round(spread, 3)
        out['strided_wins'] = bool(out['gain_ms'] > spread)
    elif legs == ('any', 'bn'):
        spread = (out['any']['max_ms'] - out['any']['min_ms']) + (out['bn']['max_ms'] - out['bn']['min_ms'])
        out['gain_ms'] = round(out['any']['median_ms'] - out['bn']['median_ms'], 3)
        out['combined_spread_ms'] = round(spread, 3)
        out['bn_wins'] = bool(out['gain_ms'] > spread)
    elif legs == ('off', 'on'):
        spread = (out['off']['max_ms'] - out['off']['min_ms']) + (out['on']['max_ms'] - out['on']['min_ms'])
        out['gain_ms'] = round(out['off']['median_ms'] - out['on']['median_ms'], 3)
        out['combined_spread_ms'] = round(spread, 3)
        out['on_wins'] = bool(out['gain_ms'] > spread)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--classes', action='store_true')
    ap.add_argument('--step', action='store_true')
    ap.add_argument('--off-only', action='store_true', help='--step: the off leg alone')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--side', type=int, default=257)
    ap.add_argument('--model', default='resnet50')
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', default='')
    ap.add_argument('--images', action='store_true', help='the image-fed ragged path (ops.x3_any_images): see above')
    ap.add_argument('--strided', action='store_true', help='stride-2 data gradients on the x3 kernels (ops.x3_any_strided): see above')
    ap.add_argument('--bn', action='store_true', help='BatchNorm and the stem tail on the peeled instances (ops.bn_any): see above')
    ap.add_argument('--block', action='store_true', help='the residual-block executor at the odd maps (ops.block_any): see above')
    ap.add_argument('--block-strided', action='store_true', help='with --block: strided residual blocks at the odd maps (ops.block_any_strided): see above')
    ap.add_argument('--frozen', action='store_true', help='--step --strided / --bn: the frozen-fold step (every BatchNorm frozen, ops.frozen_fold)')
    ap.add_argument('--no-fold', action='store_true', help='--step --bn --frozen: every BatchNorm frozen, ops.frozen_fold off')
    ap.add_argument('--family', default='depthnet', choices=sorted(FAMILY_FLAGS))
    a = ap.parse_args()
    if (a.images or a.strided or a.bn or a.block) and a.family != 'depthnet':
        raise SystemExit('--images, --strided, --bn and --block measure the dense family')
    if a.block and not (a.step or a.classes):
        raise SystemExit('--block goes with --classes or --step')
    if a.block_strided and not a.block:
        raise SystemExit('--block-strided goes with --block')
    if a.frozen and not ((a.strided or a.bn) and a.step):
        raise SystemExit('--frozen goes with --step --strided or --step --bn')
    if a.no_fold and not (a.frozen and a.bn):
        raise SystemExit('--no-fold goes with --step --bn --frozen')
    if a.classes:
        (classes_block if a.block else classes_bn if a.bn else classes_strided if a.strided else classes_images if a.images else classes if a.family == 'depthnet' else classes_partial)(a)
        if a.block and a.block_strided and not a.only:
            join_bandwidth(a)
    if a.step:
        step(a)


if __name__ == '__main__':
    main()
