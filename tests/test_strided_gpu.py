"""Strided (stride 2) data gradients on the x3 kernels (fx_conv_kernel and fx16_conv_kernel): a parity class stores from the accumulator view in an epilogue
of its own, apart from the dense epilogue that goes through the LDS staging tile.  These cases hold that store to its rows, its classes and its tensor.

Reference: the float64 oracle (oracle/np_ops.conv2d_dgrad) at the bound tests/test_kernels_gpu.py and tests/test_geometry_gpu.py hold the image-fed data
gradient to (2e-5 of the largest element); the executor cases at the bounds of tests/test_block_gpu.py.  Outputs and scratch are exact-size, poisoned and
fenced (tests/fenced.py, the fixtures of tests/test_scratch_bounds_gpu.py): a store that ran past a row, into another class or beyond the tensor shows."""
import functools
import os

import numpy as np
import pytest
import torch

import test_block_gpu as tb
import test_kernels_gpu as tk
from oracle import np_ops as ref
from test_scratch_bounds_gpu import fenced_outputs, fenced_scratch          # noqa: F401  (fixtures)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(os.environ.get('P3D_X3', '1') == '0', reason='P3D_X3=0 keeps every layer off the x3 kernels these cases are about')]

#          N   C    K   H   W  R pad
DGRAD = [(2, 128, 128, 16, 16, 3, 1),         # fx_conv_kernel (128-row tile): one 128-pixel tile per class, spanning both images
         (3, 96, 64, 16, 24, 3, 1),           # fx16, 96-row tile: non-square map, three pixel tiles per class, the last one partial (32 of 128)
         (2, 64, 64, 16, 16, 3, 1),           # fx16, 64-row tile
         (2, 128, 256, 16, 16, 1, 0)]         # 1x1: one live class, three that no tap reaches
ids = ['n%d_c%d_k%d_%dx%d_r%d' % c[:6] for c in DGRAD]
TOL = 2e-5


@functools.lru_cache(maxsize=None)
def _case(i):
    """inputs (made once, never written) and the float64 data gradient of DGRAD[i]"""
    n, c, k, h, w, r, pad = DGRAD[i]
    gen = torch.Generator(device='cuda').manual_seed(100 + i)
    dy = torch.randn(n, k, h // 2, w // 2, device='cuda', generator=gen)
    wt = torch.randn(k, c, r, r, device='cuda', generator=gen) / (k * r * r) ** 0.5
    prefill = torch.randn(n, c, h, w, device='cuda', generator=gen)
    want = ref.conv2d_dgrad(tk.host(dy), tk.host(wt), (n, c, h, w), 2, pad, 1)
    return dict(shape=(n, c, h, w), dy=dy, w=wt, pad=pad, prefill=prefill, want=want)


def _dgrad(pkg, case, per_class=False, onto=None):
    L = pkg._lib.lib()
    img = pkg.ops.act_image(case['dy'])
    if per_class:
        L.p3d_fx_tune(5, 1)
    try:
        dx = pkg.ops.conv2d_img('dgrad', case['shape'], case['w'], 2, case['pad'], 1, dy_img=img, accumulate_into=onto)
        torch.cuda.synchronize()
    finally:
        if per_class:
            L.p3d_fx_tune(5, 0)
    return dx


def _rel(got, want):
    err = float(np.abs(tk.host(got).astype(np.float64) - want).max() / np.abs(want).max())
    print('max error / max |want| = %.3e' % err)
    return err


@pytest.mark.parametrize('i', range(3), ids=ids[:3])
def test_strided_3x3_dgrad_matches_the_oracle(pkg, fenced_outputs, fenced_scratch, i):
    """every element of dx is written (it starts as NaN poison inside its fence) and equals the oracle; one launch per class gives the same bits"""
    case = _case(i)
    dx = _dgrad(pkg, case)
    assert fenced_outputs.holds(dx)
    assert _rel(dx, case['want']) < TOL
    each = _dgrad(pkg, case, per_class=True)
    assert torch.equal(each, dx)
    fenced_scratch.check()
    fenced_outputs.check()


def test_strided_1x1_dgrad_accumulates_onto_the_live_class_only(pkg, fenced_outputs, fenced_scratch):
    """accumulate = 1 onto a prefilled dx: the live class is prefill + oracle, the three classes no tap reaches keep the prefill bit for bit -- and, onto a dx
    that is all poison, every dead-class byte still is"""
    case = _case(3)
    pre = case['prefill']
    dx = torch.empty(case['shape'], device='cuda')
    assert fenced_outputs.holds(dx)
    dx.copy_(pre)
    got = _dgrad(pkg, case, onto=dx)
    assert got.data_ptr() == dx.data_ptr()
    live = torch.zeros(case['shape'], dtype=torch.bool, device='cuda')
    live[:, :, ::2, ::2] = True
    assert torch.equal(dx[~live], pre[~live])
    want = tk.host(pre).astype(np.float64) + case['want']
    assert _rel(dx, want) < TOL
    assert float(np.abs(case['want'][:, :, 1::2, :]).max()) == 0.0 and float(np.abs(case['want'][:, :, :, 1::2]).max()) == 0.0
    each = torch.empty(case['shape'], device='cuda')
    each.copy_(pre)
    _dgrad(pkg, case, per_class=True, onto=each)
    assert torch.equal(each, dx)
    poison = torch.empty(case['shape'], device='cuda')                     # (FencedAllocations: all-ones bytes)
    _dgrad(pkg, case, onto=poison)
    assert bool((poison.view(torch.uint8).view(case['shape'] + (4,))[~live] == 0xFF).all())
    assert bool(torch.isnan(poison[live]).all())
    fenced_scratch.check()
    fenced_outputs.check()


def test_strided_1x1_dgrad_overwrites(pkg, fenced_outputs, fenced_scratch):
    """accumulate = 0: the live class is the oracle's, the dead classes read zero"""
    case = _case(3)
    dx = _dgrad(pkg, case)
    assert _rel(dx, case['want']) < TOL
    assert float(dx[:, :, 1::2, :].abs().max()) == 0.0 and float(dx[:, :, :, 1::2].abs().max()) == 0.0
    assert torch.equal(_dgrad(pkg, case, per_class=True), dx)


# ---- through the executor: the strided data gradient of conv 2 (Bottleneck) / conv 1 (BasicBlock) and the accumulating one of the downsample conv ----
#             kind          inplanes planes stride dil N   H  downsample
EXECUTOR = [('bottleneck', 256, 128, 2, 1, 3, 16, True),        # 256 -> 128 -> 512: fx_conv_kernel, 4 classes x 2 pixel tiles
            ('basic', 128, 256, 2, 1, 3, 16, True),             # BasicBlock: conv 1 strided, conv 2 dense
            ('bottleneck', 128, 192, 2, 1, 3, (16, 24), True),  # fx16 96-row tiles (192 = 2 x 96), non-square, last pixel tile partial
            ('bottleneck', 128, 64, 2, 1, 2, 16, True),         # fx16 64-row tile
            ('bottleneck', 128, 128, 2, 1, 32, 48, True)]       # batch 32: 144 pixel tiles per class


@pytest.mark.parametrize('case', EXECUTOR, ids=['%s_c%d_p%d_n%d_h%s' % (c[0], c[1], c[2], c[5], c[6]) for c in EXECUTOR])
def test_strided_block_on_the_executor(pkg, case):
    """p3d_block_bwd against the per-layer path and float64 at the bounds of test_block_gpu"""
    tb.fused_block_case(pkg, *case)


def test_strided_masked_block_on_the_executor(pkg):
    """the same with partial convolutions (FX_EPI_FACTOR_IMG: the input-mask factor of the pixels a class writes)"""
    tb.masked_block_case(pkg, 'bottleneck', 256, 128, 2, 1, 3, 16, 16, True)


def test_strided_block_is_reproducible(pkg):
    """two backward passes of the strided bottleneck: bit-equal gradients"""
    block, x0, dy, _ = tb.make_case(pkg, 'bottleneck', 256, 128, 2, 1, 3, 16, True, want_clean=False)
    a = tb.run(pkg, block, x0, dy, fused=True)
    b = tb.run(pkg, block, x0, dy, fused=True)
    assert torch.equal(a['dx'], b['dx'])
    for k in a['grads']:
        assert torch.equal(a['grads'][k], b['grads'][k]), k
