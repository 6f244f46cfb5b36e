"""Training frozen-BatchNorm layers on folded fp16 convolutions under -half_acc (ops.frozen_fold_half, ops_frozen.HFrozenConvBnFn, csrc/p3d_hfrozen.hip), the host
side: the new entries are declared and bound, the switch and its environment variable, every clause of the admission rule, the layout of the plan's buffer and
the refusal of whole-step capture.  The library loads, nothing launches.  No GPU needed."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from conftest import PKG_NAME, ROOT

NEW = ('p3d_hfrozen_grad_mask_workspace_bytes', 'p3d_hfrozen_grad_mask')


@pytest.fixture
def switch(pkg):
    """the -half_acc switch on for the test body; restores what it found"""
    before = pkg.ops.frozen_fold_half(True)
    try:
        yield pkg.ops.frozen_fold_half
    finally:
        pkg.ops.frozen_fold_half(before)


def test_entries_are_declared_and_bound(pkg):
    import test_abi
    declared = test_abi.declared_functions(pkg._lib.HEADER_PATH)
    handle = ctypes.CDLL(pkg._lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in pkg._lib.SIGNATURES and hasattr(handle, name), name
    L = pkg._lib.lib()
    assert L.p3d_hfrozen_grad_mask_workspace_bytes(323, 2048) >= 2048 * 8           # at least one fp64 partial per channel
    assert L.p3d_hfrozen_grad_mask_workspace_bytes(1, 8) >= 8 * 8
    for p, k in ((5, 12), (5, 0), (5, 2056), (0, 64)):                              # outside the shape rule: nothing to size
        assert L.p3d_hfrozen_grad_mask_workspace_bytes(p, k) == 0, (p, k)
    # bad arguments are refused on the host, before any launch
    assert L.p3d_hfrozen_grad_mask(None, None, None, None, 1, 8, None, 0, None) != 0


def test_switch_defaults_off_and_round_trips(pkg):
    if os.environ.get('P3D_FROZEN_FOLD_HALF') != '1':
        before = pkg.ops.frozen_fold_half(True)
        try:
            assert before is False
            assert pkg.ops.frozen_fold_half(True) is True
        finally:
            assert pkg.ops.frozen_fold_half(False) is True
        assert pkg.ops.frozen_fold_half(False) is False


@pytest.mark.parametrize('value,want', [(None, 'False False'), ('1', 'True False')])
def test_switch_follows_the_environment(value, want):
    """P3D_FROZEN_FOLD_HALF sets the -half_acc switch and leaves the fp32 one alone"""
    env = {k: v for k, v in os.environ.items() if k not in ('P3D_FROZEN_FOLD_HALF', 'P3D_FROZEN_FOLD')}
    if value is not None:
        env['P3D_FROZEN_FOLD_HALF'] = value
    code = ('import importlib, sys; sys.path.insert(0, %r); ops = importlib.import_module(%r + ".ops"); print(ops.frozen_fold_half(False), ops.frozen_fold(False))'
            % (ROOT, PKG_NAME))
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, check=True).stdout
    assert out.strip().splitlines()[-1] == want


def _pair(pkg, c=128, k=128, r=3, stride=1, dil=1, bias=False, partial=False, images=True, pad=None):
    conv_type = pkg.partial_conv.PartialConv if partial else pkg.nn.Conv2d
    conv = conv_type(c, k, kernel_size=r, stride=stride, padding=dil * (r // 2) if pad is None else pad, dilation=dil, bias=bias)
    if images:                                                            # (host tensors: the rule only asks which images there are)
        conv._h_images = pkg.ops_half.WeightImages(conv.weight, need_dgrad=c >= 8)
    return conv, pkg.nn.BatchNorm2d(k).eval()


def test_admission_rule(pkg, switch):
    admits = pkg.ops_frozen.admits_half
    x = torch.zeros(2, 128, 17, 19, dtype=torch.float16)                  # (host only: a CPU tensor is all the rule needs)
    conv, bn = _pair(pkg)
    assert admits(x, conv, bn)
    assert admits(x, *_pair(pkg, 128, 256, 1, stride=2))                  # the downsample form
    assert admits(torch.zeros(2, 64, 33, 33, dtype=torch.float16), *_pair(pkg, 64, 96, 3, stride=2))
    assert admits(torch.zeros(2, 24, 9, 9, dtype=torch.float16), *_pair(pkg, 20, 8))      # 20 real channels in a 24-channel image, K = 8
    assert admits(x, *_pair(pkg, k=2048))
    # each clause on its own
    assert not admits(x.float(), conv, bn)                                # fp32 input: the other switch's business
    assert not admits(x[0], conv, bn)                                     # not 4-d
    assert not admits(x, *_pair(pkg, bias=True))
    assert not admits(x, *_pair(pkg, partial=True))
    rect = pkg.nn.Conv2d(128, 128, kernel_size=(3, 1), padding=(1, 0), bias=False)
    rect._h_images = pkg.ops_half.WeightImages(rect.weight)
    assert not admits(x, rect, bn)                                        # not square
    assert not admits(x, *_pair(pkg, r=2, pad=1))                         # not odd
    assert not admits(x, *_pair(pkg, images=False))                       # no fp16 weight images
    stem = _pair(pkg, c=3, k=64, r=7, stride=2)
    assert stem[0]._h_images.crsk is None
    assert not admits(torch.zeros(2, 8, 17, 19, dtype=torch.float16), *stem)      # a stem: no data-gradient image
    assert not admits(x, *_pair(pkg, k=2056))                             # K beyond 2048
    assert not admits(x, *_pair(pkg, k=12))                               # K no multiple of 8
    assert not admits(torch.zeros(2, 20, 9, 9, dtype=torch.float16), *_pair(pkg, 20, 8))  # the real, not the padded channel count
    assert not admits(torch.zeros(2, 64, 17, 19, dtype=torch.float16), conv, bn)          # not this conv's input
    assert not admits(x, conv, pkg.nn.BatchNorm2d(128).train())
    assert not admits(x, conv, torch.nn.BatchNorm2d(128, affine=False).eval())
    assert not admits(x, conv, torch.nn.BatchNorm2d(128, track_running_stats=False).eval())
    assert not admits(torch.zeros(2, 128, 1, 1, dtype=torch.float16), *_pair(pkg, pad=0))  # no output: the forward query refuses the descriptor
    with torch.no_grad():
        assert not admits(x, conv, bn)                                    # nothing to train: the inference paths keep it
    switch(False)
    assert not admits(x, conv, bn)
    switch(True)
    assert admits(x, conv, bn)


def test_admission_agrees_with_the_forward_query(pkg, switch):
    L = pkg._lib.lib()
    for c, k, r, stride, dil, h, w in ((64, 64, 3, 1, 1, 16, 16), (64, 256, 1, 1, 1, 17, 17), (512, 512, 3, 1, 2, 9, 9), (128, 128, 3, 3, 1, 17, 17),
                                       (128, 128, 3, 5, 1, 17, 17)):
        conv, bn = _pair(pkg, c, k, r, stride, dil)
        d = pkg.ops._desc((2, c, h, w), (k, c, r, r), stride, dil * (r // 2), dil)
        want = bool(L.p3d_hconv2d_fwd_infer_supported(ctypes.byref(d)))
        assert pkg.ops_frozen.admits_half(torch.zeros(2, c, h, w, dtype=torch.float16), conv, bn) == want, (c, k, r, stride, dil, h, w)


def test_the_fp32_rule_still_refuses_fp16(pkg, switch):
    """the two switches are separate: with both on, `admits` refuses fp16 input and `admits_half` refuses fp32 input"""
    before = pkg.ops.frozen_fold(True)
    try:
        conv, bn = _pair(pkg)
        x = torch.zeros(2, 128, 17, 19)
        assert pkg.ops_frozen.admits(x, conv, bn) and not pkg.ops_frozen.admits(x.half(), conv, bn)
        assert pkg.ops_frozen.admits_half(x.half(), conv, bn) and not pkg.ops_frozen.admits_half(x, conv, bn)
        pkg.ops.frozen_fold(False)
        assert pkg.ops_frozen.admits_half(x.half(), conv, bn) and not pkg.ops_frozen.admits(x, conv, bn)
    finally:
        pkg.ops.frozen_fold(before)


def test_plan_layout(pkg):
    """per pair: the kind-2 image [K][RS][Cpad] halves, b' [K] floats, the kind-4 image [Cpad][RS][K] halves, each on a 256-B line, none overlapping"""
    of = pkg.ops_frozen
    pairs = [_pair(pkg, 20, 8, 1), _pair(pkg, 64, 96, 3), _pair(pkg, 128, 2048, 1)]
    plan = of.FrozenFold(pairs, of._HUnit)
    assert plan.generation == 0 and plan.buffer is None                   # nothing folded, nothing allocated
    at = 0
    for u, (conv, bn) in zip(plan.units, pairs):
        k, c, r, _ = conv.weight.shape
        cpad = (c + 7) // 8 * 8
        assert (u.k, u.c, u.cpad, u.r) == (k, c, cpad, r)
        assert u.img_bytes == 2 * k * r * r * cpad
        assert u.img_off == at
        assert u.bias_off % 256 == 0 and u.bias_off >= u.img_off + u.img_bytes
        assert u.dimg_off % 256 == 0 and u.dimg_off >= u.bias_off + 4 * k
        at = (u.dimg_off + u.img_bytes + 255) // 256 * 256
        assert of._unit(conv, bn, of._HUnit) is u and u.plan is plan
        jobs = u.jobs(torch.zeros(1, dtype=torch.uint8))
        assert [(j.kind, j.reserved, j.K, j.C, j.RS) for j in jobs] == [(2, cpad, k, c, r * r), (4, cpad, k, c, r * r)]
        assert jobs[0].bias_out is not None and not jobs[1].bias_out
    assert plan.nbytes == at
    # a pair on its own gets a plan of one, apart from its fp32 unit
    conv, bn = _pair(pkg)
    u = of._unit(conv, bn, of._HUnit)
    assert len(u.plan.units) == 1 and of._unit(conv, bn) is not u and '_hfrozen_unit' in conv.__dict__


def test_network_plan_holds_the_dense_block_pairs(pkg):
    args = pkg.opts.parse(['-model', 'resnet18', '-suffix', 'host', '-data_name', 'h36m', '-save_path', '/tmp/p3d_host', '-criterion', 'SmoothL1', '-num_joints', '17',
                           '-side_in', '64'])
    model, _ = pkg.depth_main.create_model(args)
    plan = pkg.ops_frozen.FrozenFold.of(model, half=True)
    convs = {id(u.conv) for u in plan.units}
    blocks = [m for m in model.modules() if isinstance(m, pkg._trunk._ResidualBlock)]
    assert len(plan.units) == sum(len(b._chain) + (b.downsample is not None) for b in blocks) == 8 * 2 + 3
    assert all(isinstance(u, pkg.ops_frozen._HUnit) for u in plan.units)
    assert id(model.conv1) not in convs and id(model.regressor) not in convs
    spans = sorted((u.img_off, u.dimg_off + u.img_bytes) for u in plan.units)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= plan.nbytes


def test_graphed_step_refuses_a_frozen_fold(pkg, switch):
    class _Reducer:
        active = False

    class _Trainer:
        world, reducer = 1, _Reducer()
        model = torch.nn.Sequential(pkg.nn.BatchNorm2d(32))

    tr = _Trainer()
    tr.model.train()
    pkg.graphed.GraphedStep(tr)                                           # nothing frozen: taken
    tr.model.eval()
    with pytest.raises(pkg._lib.P3DError, match='frozen_fold_half'):
        pkg.graphed.GraphedStep(tr)
    switch(False)
    pkg.graphed.GraphedStep(tr)                                           # switch off: as ever
