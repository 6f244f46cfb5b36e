"""Training frozen-BatchNorm layers on folded convolutions (ops.frozen_fold, ops_frozen.py, csrc/p3d_frozen.hip), the host side: the new entries are
declared and bound, the switch and its environment variable, the admission rule, the refusal of whole-step capture, and the identity the finishing kernel's
dgamma rests on.  The library loads, nothing launches.  No GPU needed."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from conftest import PKG_NAME, ROOT

NEW = ('p3d_frozen_grad_mask_workspace_bytes', 'p3d_frozen_grad_mask', 'p3d_frozen_wgrad_finish')


@pytest.fixture
def switch(pkg):
    """the switch on for the test body; restores what it found"""
    before = pkg.ops.frozen_fold(True)
    try:
        yield pkg.ops.frozen_fold
    finally:
        pkg.ops.frozen_fold(before)


def test_entries_are_declared_and_bound(pkg):
    import test_abi
    declared = test_abi.declared_functions(pkg._lib.HEADER_PATH)
    handle = ctypes.CDLL(pkg._lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in pkg._lib.SIGNATURES and hasattr(handle, name), name
    assert sorted(pkg._lib.SIGNATURES) == declared
    L = pkg._lib.lib()
    assert L.p3d_frozen_grad_mask_workspace_bytes(5, 2051, 7) >= 2051 * 8          # at least one fp64 partial per channel
    assert L.p3d_frozen_grad_mask_workspace_bytes(5, 0, 7) == 0
    # bad arguments are refused on the host, before any launch
    assert L.p3d_frozen_grad_mask(None, None, None, None, 1, 16, 4, None, 0, None) != 0
    assert L.p3d_frozen_wgrad_finish(None, None, None, None, None, 1e-5, None, None, None, None, 32, 32, 0, None) != 0


def test_switch_defaults_off_and_round_trips(pkg):
    assert hasattr(pkg.ops, 'frozen_fold')
    if os.environ.get('P3D_FROZEN_FOLD') != '1':
        before = pkg.ops.frozen_fold(True)
        try:
            assert before is False
            assert pkg.ops.frozen_fold(True) is True
        finally:
            assert pkg.ops.frozen_fold(False) is True
        assert pkg.ops.frozen_fold(False) is False


@pytest.mark.parametrize('value,want', [(None, 'False'), ('1', 'True')])
def test_switch_follows_the_environment(value, want):
    env = {k: v for k, v in os.environ.items() if k != 'P3D_FROZEN_FOLD'}
    if value is not None:
        env['P3D_FROZEN_FOLD'] = value
    code = 'import importlib, sys; sys.path.insert(0, %r); ops = importlib.import_module(%r + ".ops"); print(ops.frozen_fold(False))' % (ROOT, PKG_NAME)
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, check=True).stdout
    assert out.strip().splitlines()[-1] == want


def _pair(pkg, c=128, k=128, r=3, stride=1, dil=1, bias=False, partial=False):
    conv_type = pkg.partial_conv.PartialConv if partial else pkg.nn.Conv2d
    conv = conv_type(c, k, kernel_size=r, stride=stride, padding=dil * (r // 2), dilation=dil, bias=bias)
    return conv, pkg.nn.BatchNorm2d(k).eval()


def test_admission_rule(pkg, switch):
    admits = pkg.ops_frozen.admits
    x = torch.zeros(2, 128, 17, 19)                                   # (host only: a CPU tensor is all the rule needs)
    conv, bn = _pair(pkg)
    assert admits(x, conv, bn)
    assert admits(torch.zeros(2, 128, 16, 16), conv, bn)              # aligned maps: the first entry
    assert admits(x, *_pair(pkg, 128, 256, 1, stride=2))              # the downsample form
    assert admits(torch.zeros(2, 64, 33, 33), *_pair(pkg, 64, 96, 3, stride=2))
    # each clause on its own
    assert not admits(x, *_pair(pkg, bias=True))
    assert not admits(x, *_pair(pkg, partial=True))
    assert not admits(x, conv, pkg.nn.BatchNorm2d(128).train())
    assert not admits(x.half(), conv, bn)
    assert not admits(torch.zeros(2, 24, 17, 19), *_pair(pkg, c=24))
    assert not admits(x, *_pair(pkg, k=16))
    assert not admits(x, conv, torch.nn.BatchNorm2d(128, track_running_stats=False).eval())
    assert not admits(torch.zeros(2, 64, 17, 19), conv, bn)           # not this conv's input
    with torch.no_grad():
        assert not admits(x, conv, bn)                                # nothing to train: the inference paths keep it
    switch(False)
    assert not admits(x, conv, bn)
    switch(True)
    assert admits(x, conv, bn)


def test_admission_agrees_with_the_forward_queries(pkg, switch):
    """the shape clause is exactly `one of the two folded forward entries takes it`"""
    L = pkg._lib.lib()
    for c, k, r, stride, dil, h, w in ((64, 64, 3, 1, 1, 16, 16), (64, 64, 3, 1, 1, 17, 17), (64, 256, 1, 1, 1, 17, 17), (256, 64, 1, 1, 1, 16, 16),
                                       (512, 512, 3, 1, 2, 9, 9), (2048, 512, 1, 1, 1, 5, 5), (128, 128, 3, 3, 1, 17, 17)):
        conv, bn = _pair(pkg, c, k, r, stride, dil)
        d = pkg.ops._desc((2, c, h, w), (k, c, r, r), stride, dil * (r // 2), dil)
        want = bool(L.p3d_fx_conv_fwd_infer_supported(ctypes.byref(d), 0)) or bool(L.p3d_fx_conv_fwd_infer_any_supported(ctypes.byref(d)))
        assert pkg.ops_frozen.admits(torch.zeros(2, c, h, w), conv, bn) == want, (c, k, r, stride, dil, h, w)


def test_network_plan_holds_the_dense_block_pairs(pkg):
    """FrozenFold.of: every conv + BatchNorm pair of the dense residual blocks, downsample branches included; no stem, no head, no Fusion 1x1"""
    args = pkg.opts.parse(['-model', 'resnet18', '-suffix', 'host', '-data_name', 'h36m', '-save_path', '/tmp/p3d_host', '-criterion', 'SmoothL1', '-num_joints', '17', '-side_in', '64'])
    model, _ = pkg.depth_main.create_model(args)
    plan = pkg.ops_frozen.FrozenFold.of(model)
    convs = {id(u.conv) for u in plan.units}
    blocks = [m for m in model.modules() if isinstance(m, pkg._trunk._ResidualBlock)]
    want = sum(len(b._chain) + (b.downsample is not None) for b in blocks)
    assert len(plan.units) == want == 8 * 2 + 3
    assert id(model.conv1) not in convs and id(model.regressor) not in convs
    assert plan.generation == 0 and plan.buffer is None               # nothing folded, nothing allocated before the first forward
    offs = sorted((u.img_off, u.w_off + 4 * u.k * u.c * u.r * u.r) for u in plan.units)
    assert all(a[1] <= b[0] for a, b in zip(offs, offs[1:])) and offs[-1][1] <= plan.nbytes


def test_graphed_step_refuses_a_frozen_fold(pkg, switch):
    class _Reducer:
        active = False

    class _Trainer:
        world, reducer = 1, _Reducer()
        model = torch.nn.Sequential(pkg.nn.BatchNorm2d(32))

    tr = _Trainer()
    tr.model.train()
    pkg.graphed.GraphedStep(tr)                                       # nothing frozen: taken
    tr.model.eval()
    with pytest.raises(pkg._lib.P3DError, match='frozen_fold'):
        pkg.graphed.GraphedStep(tr)
    switch(False)
    pkg.graphed.GraphedStep(tr)                                       # switch off: as ever


def test_gamma_identity_in_float64():
    """sum_p g * z = <w, wgrad(x, g)> per output channel, for a strided, dilated 3x3: what p3d_frozen_wgrad_finish takes dgamma from"""
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(3, 6, 13, 11, dtype=torch.float64, generator=gen)
    w = torch.randn(5, 6, 3, 3, dtype=torch.float64, generator=gen, requires_grad=True)
    z = torch.nn.functional.conv2d(x, w, stride=2, padding=2, dilation=2)
    g = torch.randn(z.shape, dtype=torch.float64, generator=gen)
    raw, = torch.autograd.grad(z, w, g)
    lhs = (g * z.detach()).sum(dim=(0, 2, 3))
    rhs = (w.detach() * raw).sum(dim=(1, 2, 3))
    assert torch.allclose(lhs, rhs, rtol=1e-12, atol=1e-12 * float((g * z.detach()).abs().sum()))
