#!/usr/bin/env python3
"""Per-class timing of the folded fp32 forward at the 257^2 chain's odd maps (65 / 33 / 17), ResNet-50 depthnet, stride 16, batch 64.

Legs per conv class (conv + folded BatchNorm + ReLU), alternating within one process, --rounds rounds of --iters launches each, timed with device events:
  ragged    p3d_fx_conv_fwd_infer_any on the odd map                 (infer.FoldedConv(conv, bn, any_size=True))
  igemm     the per-layer fallback on the same odd map               (infer.FoldedConv(conv, bn): ops.conv_bn_eval, the fp32-MFMA kernel)
  aligned   p3d_fx_conv_fwd_infer on the nearest aligned map (64 / 32 / 16)
  ragged_b  with --lib2 PATH: `ragged` on a second build of libp3d_hip.so (an A/B of a tuning build, e.g. another occupancy of the ragged instances)
Prints one line per class, heaviest first (FLOPs x the number of layers of that class in the network): median ms, [min .. max], TFLOP/s, ns per GFLOP
(so that the odd and the aligned map compare per FLOP), then the sums weighted by the layer counts.  GPU box only."""
import argparse
import ctypes
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module('3d-pose-estimation-with-previleged-information_amd')

# Cin, aligned map, Cout, k, stride, dilation, layers of the class   (the dense convs behind the stem; tools/conv_bench.py's table)
R50 = [(64, 64, 64, 1, 1, 1, 1), (64, 64, 64, 3, 1, 1, 3), (64, 64, 256, 1, 1, 1, 4), (256, 64, 64, 1, 1, 1, 2),
       (256, 64, 128, 1, 1, 1, 1), (128, 64, 128, 3, 2, 1, 1), (128, 32, 512, 1, 1, 1, 4), (256, 64, 512, 1, 2, 1, 1),
       (512, 32, 128, 1, 1, 1, 3), (128, 32, 128, 3, 1, 1, 3), (512, 32, 256, 1, 1, 1, 1), (256, 32, 256, 3, 2, 1, 1),
       (256, 16, 1024, 1, 1, 1, 6), (512, 32, 1024, 1, 2, 1, 1), (1024, 16, 256, 1, 1, 1, 5), (256, 16, 256, 3, 1, 1, 5),
       (1024, 16, 512, 1, 1, 1, 1), (512, 16, 512, 3, 1, 2, 1), (512, 16, 2048, 1, 1, 1, 3), (1024, 16, 2048, 1, 1, 1, 1),
       (2048, 16, 512, 1, 1, 1, 2), (512, 16, 512, 3, 1, 1, 2), (2048, 16, 272, 3, 1, 1, 1)]


def second_lib(path):
    handle = ctypes.CDLL(path)
    for name, (res, args) in pkg._lib.SIGNATURES.items():
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = res, args
    return handle


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--lib2', default='', help='a second build of libp3d_hip.so for the ragged_b leg')
    ap.add_argument('--only', default='')
    a = ap.parse_args()
    first = pkg._lib.lib()
    other = second_lib(a.lib2) if a.lib2 else None

    def on(handle, fn):
        def call():
            pkg._lib._lib = handle
            try:
                return fn()
            finally:
                pkg._lib._lib = first
        return call

    rows, total = [], {}
    for (c, h, k, ks, st, dil, cnt) in sorted(R50, key=lambda r: -r[0] * r[2] * r[3] ** 2 * ((r[1] // r[4]) ** 2) * r[6]):
        tag = 'c%d h%d k%d %dx%d s%d d%d x%d' % (c, h + 1, k, ks, ks, st, dil, cnt)
        if a.only and a.only not in tag:
            continue
        torch.manual_seed(c + k)
        conv = pkg.nn.Conv2d(c, k, ks, stride=st, padding=dil * (ks - 1) // 2, dilation=dil, bias=False).cuda().eval()
        bn = pkg.nn.BatchNorm2d(k).cuda().eval()
        x_odd, x_al = torch.randn(a.batch, c, h + 1, h + 1, device='cuda'), torch.randn(a.batch, c, h, h, device='cuda')
        any_fc, fc = pkg.infer.FoldedConv(conv, bn, any_size=True), pkg.infer.FoldedConv(conv, bn)
        legs = {'ragged': lambda: any_fc(x_odd, relu=True), 'igemm': lambda: fc(x_odd, relu=True), 'aligned': lambda: fc(x_al, relu=True)}
        if other is not None:
            legs['ragged_b'] = on(other, legs['ragged'])
        pkg.ops.conv_path_stats(reset=True)
        for fn in legs.values():
            for _ in range(3):
                fn()
        stats = pkg.ops.conv_path_stats(reset=True)
        assert stats['x3']['fwd'][0] == 6 and stats['fp32']['fwd'][0] == 3, stats    # each leg ran on the kernel it is named after (the first library's counters)
        ms = {name: [] for name in legs}
        for _ in range(a.rounds):
            for name, fn in legs.items():
                ms[name].append(timed(fn, a.iters))
        ho_odd, ho_al = h // st + 1, h // st
        gf = {name: 2.0 * a.batch * k * c * ks * ks * (ho_al if name == 'aligned' else ho_odd) ** 2 / 1e9 for name in legs}
        line = '%-30s %7.2f GF |' % (tag, gf['ragged'])
        for name, v in ms.items():
            v.sort()
            med = v[len(v) // 2]
            line += ' %s %.3f [%.3f..%.3f] ms %5.1f TF %5.1f ns/GF |' % (name, med, v[0], v[-1], gf[name] / med, med * 1e6 / gf[name])
            total[name] = total.get(name, 0.0) + med * cnt
        print(line, flush=True)
        rows.append(tag)
    print('sum over the %d classes x their layer counts: %s' % (len(rows), '  '.join('%s %.2f ms' % kv for kv in total.items())))


if __name__ == '__main__':
    main()
