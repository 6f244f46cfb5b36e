#!/usr/bin/env python3
"""Inference throughput of the eval path (model.eval(), no_grad), ResNet-50 depthnet at batch 64, 256^2.

Legs, timed in the same process, alternating (device-synchronised, 10 warm-up + 50 timed iterations per round):
  fused     today's eval path: conv + BN (+ res + ReLU) per layer in one kernel (ops.conv_bn_eval, the fp32-MFMA kernel)
  folded    infer.fold(model): BatchNorm folded into the x3 convolutions (p3d_fx_conv_fwd_infer)
--any-size adds, for a --side whose maps are not multiples of 4 wide (the reference's default 257):
  folded_any    infer.fold(model, any_size=True): the layers `folded` leaves on the per-layer fallback run on p3d_fx_conv_fwd_infer_any
--odd-sides adds, at such a --side:
  folded_odd    infer.fold(model, any_size=True, odd_sides=True): the 7x7 stems on the padded space-to-depth image (p3d_stem_image_any, p3d_stem_tail_infer_any) and
                the partial layers on p3d_fx_conv_fwd_infer_masked_any as well (what Trainer._fold builds)
--family partial_depthnet / partial_fusionnet times those networks (depth ~ U[0, 1) with values < 0.3 zeroed; partial_depthnet: -depth_only).
--half replaces them with the -half_acc legs:
  half          today's fp16 eval forward: fp16 conv, then a stand-alone eval-mode BatchNorm (+ res + ReLU) pass per layer
  half_folded   infer.fold_half(model): BatchNorm folded into the fp16 convolutions (p3d_hconv2d_fwd_infer)
--fp8 (with --half) adds the block-scaled FP8 leg:
  fp8_folded    infer.fold_fp8(model): MXFP8 convolutions between fp16 folded stems and heads (p3d_f8conv2d_fwd_infer)
  fp8_resident  infer.fold_fp8(model, resident=True): the same bits, MXFP8 activation tensors between the fp8 convs (p3d_f8conv2d_fwd_infer_mx)
  and --distill then times the fp8 teacher (P3D_FOLDED_EVAL_FP8=1) beside the fp16 folded one; --deviation prints the relative L2 deviation of z and the
  feature map of the fp8 net against the fp32 eval forward and fold_half (depthnet and fusionnet, seeded synthetic weights and inputs).
--separate adds the round-1 leg with stand-alone BatchNorm passes; --distill also times one distill_step with and without the folded teacher
(with --half: a -half_acc student and teacher, P3D_FOLDED_EVAL_HALF; with --family partial_fusionnet: a partial_fusionnet teacher).
--test-loop times Trainer.test instead (depthnet; --test-batches batches of --batch, inputs in pinned host memory as a loader delivers them),
for the folded fp32 net (P3D_FOLDED_EVAL=1) and the folded fp16 net (-half_acc, P3D_FOLDED_EVAL_HALF=1), each with its bare forward:
  forward_<p>   the folded net alone on a device batch
  host_<p>      Trainer.test with the per-batch host metrics (P3D_DEVICE_EVAL=0)
  device_<p>    Trainer.test with the metrics on the GPU and one read-back per epoch (P3D_DEVICE_EVAL=1)
Prints one line per leg and round, then a JSON summary line."""
import argparse
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module('3d-pose-estimation-with-previleged-information_amd')

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--side', type=int, default=256)
ap.add_argument('--model', default='resnet50')
ap.add_argument('--warmup', type=int, default=10)
ap.add_argument('--iters', type=int, default=50)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--any-size', action='store_true', help='add the folded_any leg: infer.fold(model, any_size=True)')
ap.add_argument('--odd-sides', action='store_true', help='add the folded_odd leg: infer.fold(model, any_size=True, odd_sides=True)')
ap.add_argument('--separate', action='store_true')
ap.add_argument('--distill', action='store_true')
ap.add_argument('--half', action='store_true', help='-half_acc legs: half / half_folded')
ap.add_argument('--fp8', action='store_true', help='with --half (required): the fp8_folded leg (infer.fold_fp8), and an fp8 teacher under --distill')
ap.add_argument('--deviation', action='store_true', help='with --fp8: relative L2 deviation of the fp8 net (not timed)')
ap.add_argument('--only', default=None, help='time these legs only, comma-separated (one leg: profiling runs)')
ap.add_argument('--test-loop', action='store_true', help='time Trainer.test: host metrics against P3D_DEVICE_EVAL=1, fp32 and fp16 folded')
ap.add_argument('--test-batches', type=int, default=50)
ap.add_argument('--family', default='depthnet', choices=['depthnet', 'partial_depthnet', 'partial_fusionnet'])
opt = ap.parse_args()
if opt.fp8 and not opt.half:
    ap.error('--fp8 adds the fp8_folded leg beside the -half_acc legs: give it with --half')
if opt.deviation and not opt.fp8:
    ap.error('--deviation reports the fp8 net: give it with --half --fp8')
if opt.distill and opt.family == 'partial_depthnet':
    ap.error('--distill times a depthnet student with a fusionnet (--family depthnet) or partial_fusionnet (--family partial_fusionnet) teacher')



def test_loop():
    """--test-loop: Trainer.test per batch, host metrics vs P3D_DEVICE_EVAL=1, next to the bare folded forward; legs alternate per round."""
    import tempfile
    import numpy as np
    meta = os.path.join(tempfile.mkdtemp(), 'metadata.json')
    with open(meta, 'w') as f:
        json.dump(dict(loader=dict(h36m='depth_datasets'), no_depth=dict(h36m=False), thresholds=dict(h36m=dict(solid=40.0, close=80.0, rough=150.0))), f)
    distinct = min(opt.test_batches, 10)                 # distinct pinned batches, cycled: 10 x 64 x 3 x 256^2 fp32 = 0.5 GB of pinned memory
    pinned = []
    for k in range(distinct):
        c, d, tc, tv = pkg.synth.make_batch(opt.batch, side=opt.side, rank=0, step=k, invalid_frac=0.2)
        rot = np.linalg.qr(np.random.Generator(np.random.PCG64(k)).standard_normal((opt.batch, 3, 3)))[0].astype(np.float32)
        pinned.append(tuple(torch.from_numpy(a).pin_memory() for a in (c, d, tc, tv, rot)))
    batches = [pinned[i % distinct] for i in range(opt.test_batches)]
    x = pinned[0][0].cuda()
    os.environ.update(P3D_FOLDED_EVAL='1', P3D_FOLDED_EVAL_HALF='1')
    legs = {}
    for prec, extra in (('fp32', []), ('fp16', ['-half_acc'])):
        targs = pkg.opts.parse(['-model', opt.model, '-suffix', 'b', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1',
                                '-num_joints', '17', '-side_in', str(opt.side), '-metadata', meta] + extra)
        trainer = pkg.depth_train.Trainer(targs, pkg.depth_main.create_model(targs)[0].cuda(), pkg.utils.get_info())
        trainer.verbose = False
        trainer.test(1, batches[:2])                     # folds the net, plans and workspaces
        net = trainer.__dict__['_folded_half_model' if trainer.half_acc else '_folded_model']     # the folded net Trainer.test runs

        def forward(net=net):
            with torch.no_grad():
                for _ in batches:
                    net(x)

        def loop(trainer=trainer, switch='0'):
            os.environ['P3D_DEVICE_EVAL'] = switch
            try:
                return trainer.test(1, batches)
            finally:
                os.environ.pop('P3D_DEVICE_EVAL')
        legs['forward_' + prec] = forward
        legs['host_' + prec] = loop
        legs['device_' + prec] = lambda loop=loop: loop(switch='1')
    if opt.only:
        legs = {k: legs[k] for k in opt.only.split(',')}
    times, records = {k: [] for k in legs}, {}
    for r in range(opt.rounds):
        for name, fn in legs.items():
            fn()                                          # one warm pass per leg and round
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / len(batches)
            times[name].append(dt)
            if out is not None:
                records[name] = out
            print('round %d  %-16s %.3f ms / batch of %d' % (r, name, dt * 1e3, opt.batch), flush=True)
    for prec in ('fp32', 'fp16'):
        host, dev = records.get('host_' + prec), records.get('device_' + prec)
        if host and dev:
            assert host['test_loss'] == dev['test_loss'], (prec, host, dev)
    summary = {k: dict(ms_median=sorted(v)[len(v) // 2] * 1e3, ms_min=min(v) * 1e3, ms_max=max(v) * 1e3) for k, v in times.items()}
    print(json.dumps(dict(mode='test_loop', model=opt.model, batch=opt.batch, side=opt.side, batches=opt.test_batches, rounds=opt.rounds, legs=summary)))


if opt.test_loop:
    test_loop()
    sys.exit(0)

flags = {'depthnet': [], 'partial_depthnet': ['-depth_only', '-partial_conv'], 'partial_fusionnet': ['-do_fusion', '-partial_conv']}[opt.family]
args = pkg.opts.parse(['-model', opt.model, '-suffix', 'b', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1', '-num_joints', '17',
                       '-side_in', str(opt.side)] + flags)
model = pkg.depth_main.create_model(args)[0].cuda().eval()
assert type(model).__module__.endswith('.' + opt.family)
x = torch.randn(opt.batch, 3, opt.side, opt.side, device='cuda')
if opt.family != 'depthnet':
    depth = torch.rand(opt.batch, 1, opt.side, opt.side, device='cuda')
    depth = depth * (depth >= 0.3)                      # the synthetic recipe: depth ~ U[0, 1), values < 0.3 zeroed
    inputs = (depth,) if opt.family == 'partial_depthnet' else (x, depth)
else:
    inputs = (x,)
fuse = pkg.ops.can_fuse_eval
if opt.half:
    model._p3d_half = True                              # what the Trainer sets under -half_acc
    pkg.ops_half.refresh_weights(model)
    hfolded = pkg.infer.fold_half(model)
    legs = {'half': lambda: model(*inputs), 'half_folded': lambda: hfolded(*inputs)}
    if opt.fp8:
        f8folded = pkg.infer.fold_fp8(model)
        legs['fp8_folded'] = lambda: f8folded(*inputs)
        f8resident = pkg.infer.fold_fp8(model, resident=True)
        legs['fp8_resident'] = lambda: f8resident(*inputs)
else:
    folded = pkg.infer.fold(model)
    legs = {'fused': lambda: model(*inputs), 'folded': lambda: folded(*inputs)}
    if opt.any_size:
        folded_any = pkg.infer.fold(model, any_size=True)
        legs['folded_any'] = lambda: folded_any(*inputs)
    if opt.odd_sides:
        folded_odd = pkg.infer.fold(model, any_size=True, odd_sides=True)
        legs['folded_odd'] = lambda: folded_odd(*inputs)
if opt.separate:
    legs['separate'] = lambda: model(*inputs)
if opt.only:
    legs = {k: legs[k] for k in opt.only.split(',')}


def run(name, fn):
    pkg.ops.can_fuse_eval = (lambda *a: False) if name == 'separate' else fuse
    with torch.no_grad():
        for _ in range(opt.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(opt.iters):
            fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / opt.iters


gflop = 2 * 9.390 * opt.batch if (opt.family, opt.model, opt.side) == ('depthnet', 'resnet50', 256) else None
times = {k: [] for k in legs}
for r in range(opt.rounds):
    for name, fn in legs.items():
        dt = run(name, fn)
        times[name].append(dt)
        print('round %d  %-16s %.2f ms / batch of %d = %.0f crops/s%s' % (r, name, dt * 1e3, opt.batch, opt.batch / dt,
                                                                        '  (%.0f TF)' % (gflop / dt / 1e3) if gflop else ''), flush=True)
summary = {k: dict(ms_median=sorted(v)[len(v) // 2] * 1e3, ms_min=min(v) * 1e3, ms_max=max(v) * 1e3, crops_s=opt.batch / sorted(v)[len(v) // 2]) for k, v in times.items()}

if opt.distill:
    dargs = pkg.opts.parse(['-model', opt.model, '-suffix', 'b', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1', '-num_joints', '17',
                            '-side_in', str(opt.side), '-do_teach', '-do_fusion'] + (['-half_acc'] if opt.half else []) +
                           (['-partial_conv'] if opt.family == 'partial_fusionnet' else []))
    switch = 'P3D_FOLDED_EVAL_HALF' if opt.half else 'P3D_FOLDED_EVAL'
    dlegs = (('teacher', {switch: '0'}), ('folded_teacher', {switch: '1'})) + ((('fp8_teacher', {switch: '1', 'P3D_FOLDED_EVAL_FP8': '1'}),) if opt.fp8 else ())
    student = pkg.depthnet.__dict__[opt.model](dargs, False).cuda()
    teacher_family = pkg.partial_fusionnet if opt.family == 'partial_fusionnet' else pkg.fusionnet
    teacher = teacher_family.__dict__[opt.model](dargs, False).cuda().eval()
    c, d, tc, tv = (torch.from_numpy(a).cuda() for a in pkg.synth.make_batch(opt.batch, side=opt.side, rank=0, step=0))
    side_out = (opt.side - 1) // 16 + 1
    att = torch.ones(opt.batch, 1, side_out, side_out, device='cuda')
    res = {}
    for r in range(opt.rounds):
        for leg, env in dlegs:
            os.environ.update(env)
            os.environ['P3D_FOLDED_EVAL_FP8'] = env.get('P3D_FOLDED_EVAL_FP8', '0')
            tr = pkg.depth_train.Trainer(dargs, student, pkg.utils.get_info()) if r == 0 and leg == 'teacher' else tr
            tr.set_teacher(teacher)
            assert (tr.folded_teacher is not None) == (leg != 'teacher')
            assert isinstance(tr.folded_teacher, pkg.infer.Fp8FoldedNet) == (leg == 'fp8_teacher')
            for _ in range(3):
                tr.distill_step(1, c, d, tc, tv, att)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                tr.distill_step(1, c, d, tc, tv, att)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / 10
            res.setdefault(leg, []).append(dt * 1e3)
            print('round %d  distill_step %-24s %.2f ms' % (r, leg, dt * 1e3), flush=True)
    summary['distill_step_ms'] = {k: sorted(v) for k, v in res.items()}
if opt.fp8 and opt.deviation:
    def rel_l2(a, b):
        a, b = a.double(), b.double()
        return float((a - b).norm() / b.norm())

    dev = {}
    for fam in ('depthnet', 'fusionnet'):
        fargs = pkg.opts.parse(['-model', opt.model, '-suffix', 'b', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1', '-num_joints', '17',
                                '-side_in', str(opt.side)] + (['-do_fusion'] if fam == 'fusionnet' else []))
        torch.manual_seed(0)
        net = (pkg.fusionnet.__dict__[opt.model](fargs, False) if fam == 'fusionnet' else pkg.depth_main.create_model(fargs)[0]).cuda().eval()
        g = torch.Generator(device='cuda').manual_seed(1)
        xin = (torch.randn(opt.batch, 3, opt.side, opt.side, device='cuda', generator=g),)
        if fam == 'fusionnet':
            xin = xin + (torch.rand(opt.batch, 1, opt.side, opt.side, device='cuda', generator=g),)
        with torch.no_grad():
            ref32 = net(*xin)
        f8 = pkg.infer.fold_fp8(net)(*xin)
        h16 = pkg.infer.fold_half(net)(*xin)
        dev[fam] = {'z_vs_fp32': rel_l2(f8[0], ref32[0]), 'feat_vs_fp32': rel_l2(f8[1], ref32[1]),
                    'z_vs_half': rel_l2(f8[0], h16[0]), 'feat_vs_half': rel_l2(f8[1], h16[1]),
                    'half_z_vs_fp32': rel_l2(h16[0], ref32[0]), 'half_feat_vs_fp32': rel_l2(h16[1], ref32[1])}
        print('deviation %-10s %s' % (fam, ' '.join('%s %.3e' % kv for kv in dev[fam].items())), flush=True)
    summary['deviation_rel_l2'] = dev
print(json.dumps(dict(model=opt.model, family=opt.family, half=opt.half, batch=opt.batch, side=opt.side, warmup=opt.warmup, iters=opt.iters, legs=summary)))
