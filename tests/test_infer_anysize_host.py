"""The folded fp32 forward at any map width (p3d_fx_conv_fwd_infer_any[_supported | _workspace_bytes], infer.fold(..., any_size=True)): symbols, the
host-only predicate over every dense conv of the reference networks at the default 257^2 crop, what it still refuses, the keyword, and on the CPU that
the references of the rectangular GPU cases (tests/test_infer_anysize_gpu.py) tell a transposing kernel apart.  No GPU needed."""
import ctypes
import inspect
import os

import pytest
import torch
import torch.nn.functional as F

import geometry_table as T
from conftest import ROOT
from oracle import np_net

NAMES = ('p3d_fx_conv_fwd_infer_any_supported', 'p3d_fx_conv_fwd_infer_any_workspace_bytes', 'p3d_fx_conv_fwd_infer_any')
RECTANGLES = [(17, 33), (33, 17)]                     # the rectangular conv cases of the GPU file (3x3, 128 -> 128 channels)
TOL = 2e-5                                            # their bound, relative to max |reference|


def dense_convs(model, net_stride, side, n=2):
    """(name, x shape, weight shape, stride, pad, dil) of every dense conv behind the stem of a depthnet, from stage_geometry and the block lists (the
    construction of depthnet.py / _trunk.TrunkBase._make_layer: the first block of a layer carries the stride, the dilation and the downsample)."""
    kind, blocks = np_net.LAYERS[model]
    exp = 1 if kind == 'basic' else 4
    strides, dils = np_net.stage_geometry(net_stride)
    half = lambda v: (v - 1) // 2 + 1
    hw = half(half(side))                             # 7x7 stride 2 pad 3, then the 3x3 stride 2 pad 1 max pool
    out, inplanes = [], 64
    for li, (planes, nb, s, d) in enumerate(zip((64, 128, 256, 512), blocks, (1,) + strides, (1,) + dils), 1):
        for b in range(nb):
            bs, bd = (s, d) if b == 0 else (1, 1)
            ho = (hw - 1) // bs + 1
            tag = 'layer%d.%d.' % (li, b)
            if b == 0 and (s != 1 or inplanes != planes * exp):
                out.append((tag + 'downsample', (n, inplanes, hw, hw), (planes * exp, inplanes, 1, 1), bs, 0, 1))
            if kind == 'basic':
                out.append((tag + 'conv1', (n, inplanes, hw, hw), (planes, inplanes, 3, 3), bs, bd, bd))
                out.append((tag + 'conv2', (n, planes, ho, ho), (planes, planes, 3, 3), 1, 1, 1))
            else:
                out.append((tag + 'conv1', (n, inplanes, hw, hw), (planes, inplanes, 1, 1), 1, 0, 1))
                out.append((tag + 'conv2', (n, planes, hw, hw), (planes, planes, 3, 3), bs, bd, bd))
                out.append((tag + 'conv3', (n, planes, ho, ho), (planes * 4, planes, 1, 1), 1, 0, 1))
            inplanes, hw = planes * exp, ho
    out.append(('regressor', (n, inplanes, hw, hw), (16 * 17, inplanes, 3, 3), 1, 1, 1))
    return out


def test_symbols_in_header_and_bound(pkg):
    header = open(os.path.join(ROOT, 'include', 'p3d_hip.h')).read()
    for name in NAMES:
        assert name + '(' in header, name
        assert name in pkg._lib.SIGNATURES, name
        assert hasattr(pkg._lib.lib(), name), name


def test_query_is_host_only(pkg):
    L = pkg._lib.lib()
    assert L.p3d_fx_conv_fwd_infer_any_supported(None) == 0
    assert L.p3d_fx_conv_fwd_infer_any_workspace_bytes(None) == 0
    d = pkg.ops._desc((2, 512, 17, 17), (512, 512, 3, 3), 1, 1, 1)
    assert L.p3d_fx_conv_fwd_infer_any_supported(ctypes.byref(d)) == 1
    assert L.p3d_fx_conv_fwd_infer_any_workspace_bytes(ctypes.byref(d)) > 0


@pytest.mark.parametrize('model', ['resnet18', 'resnet50'])
@pytest.mark.parametrize('net_stride', [16, 8, 32])
def test_admits_every_dense_conv_at_257(pkg, model, net_stride):
    L = pkg._lib.lib()
    convs = dense_convs(model, net_stride, 257)
    assert len(convs) == {'resnet18': 16 + 3 + 1, 'resnet50': 48 + 4 + 1}[model]
    if net_stride == 16:                              # the maps the default crop gives: 65 behind the pool, 33 in layer2, 17 from layer3 on
        assert {c[1][2] for c in convs} == {65, 33, 17}
    odd = 0
    for name, xs, ws, s, pad, dil in convs:
        d = pkg.ops._desc(xs, ws, s, pad, dil)
        assert L.p3d_fx_conv_fwd_infer_any_supported(ctypes.byref(d)) == 1, (name, xs, ws, s, pad, dil)
        if d.W % 4 or d.Wo % 4:
            odd += 1
            assert L.p3d_fx_conv_fwd_infer_supported(ctypes.byref(d), 0) == 0, name      # the aligned entry keeps its verdict
    assert odd == len(convs)                          # at 257^2 no dense conv has both widths divisible by 4


def test_shapes_agree_with_the_model(pkg):
    """dense_convs against the module tree the package builds (stride 16): the same conv shapes, strides, paddings and dilations in the same order"""
    args = pkg.opts.parse(['-model', 'resnet50', '-suffix', 't', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1', '-num_joints', '17'])
    net = pkg.depthnet.resnet50(args, False)
    got = []
    for lname in ('layer1', 'layer2', 'layer3', 'layer4'):
        for blk in getattr(net, lname):
            mods = ([blk.downsample[0]] if blk.downsample is not None else []) + [getattr(blk, c) for c, _ in blk._chain]
            got += [(tuple(m.weight.shape), m.stride[0], m.padding[0], m.dilation[0]) for m in mods]
    got.append((tuple(net.regressor.weight.shape), 1, 1, 1))
    assert got == [(ws, s, pad, dil) for _, _, ws, s, pad, dil in dense_convs('resnet50', args.stride, 257)]


def test_admits_the_refused_rows_of_the_geometry_table(pkg):
    L = pkg._lib.lib()
    refused = [g for g in T.ROWS if g.name.endswith('_refused')]
    assert len(refused) == 5
    for g in refused:
        d = pkg.ops._desc((g.n, g.c, g.h, g.w), (g.k, g.c, g.r, g.r), g.stride, g.pad, g.dil)
        assert L.p3d_fx_conv_fwd_infer_supported(ctypes.byref(d), 0) == 0, g.name
        assert L.p3d_fx_conv_fwd_infer_any_supported(ctypes.byref(d)) == 1, g.name


def test_still_refuses(pkg):
    L = pkg._lib.lib()
    D = pkg.ops._desc
    no = {
        'C % 16': D((2, 72, 17, 17), (64, 72, 3, 3), 1, 1, 1),
        'K < 32': D((2, 64, 17, 17), (16, 64, 3, 3), 1, 1, 1),
        'even filter': D((2, 64, 17, 17), (64, 64, 2, 2), 1, 0, 1),
        'stride 3': D((2, 64, 17, 17), (64, 64, 3, 3), 3, 1, 1),
        'channel window': D((2, 64, 17, 17), (64, 128, 1, 1), 1, 0, 1, c_offset=64, c_total=128),
        'accumulate 2': D((2, 64, 17, 17), (64, 64, 3, 3), 1, 1, 1, accumulate=2),
    }
    for why, d in no.items():
        assert L.p3d_fx_conv_fwd_infer_any_supported(ctypes.byref(d)) == 0, why
    for d in (D((2, 64, 17, 17), (64, 64, 3, 3), 1, 1, 1), D((2, 64, 17, 17), (64, 64, 3, 3), 1, 1, 1, accumulate=1), D((2, 32, 19, 18), (32, 32, 1, 1), 2, 0, 1)):
        assert L.p3d_fx_conv_fwd_infer_any_supported(ctypes.byref(d)) == 1


def test_keyword(pkg):
    for fn in (pkg.infer.fold, pkg.infer.FoldedConv.__init__, pkg.infer.FoldedNet.__init__):
        p = inspect.signature(fn).parameters
        assert 'any_size' in p and p['any_size'].default is False, fn


@pytest.mark.parametrize('hw', RECTANGLES, ids=lambda hw: '%dx%d' % hw)
@pytest.mark.parametrize('stride,pad,dil', [(1, 1, 1), (2, 1, 1), (1, 2, 2), (1, 0, 1), (1, 2, 1)])
def test_transposed_read_is_far_from_the_reference(hw, stride, pad, dil):
    """float64 reference of a rectangular case against the same memory read as [W][H]: at least 100 x the GPU bound apart"""
    g = T.Geo('rect', 3, 128, 128, hw[0], hw[1], 3, stride, pad, dil, 0)
    assert T.transposition_gap(g) >= 100 * TOL


def test_transposed_block_chain_is_far_from_the_reference():
    """two folded 3x3 convs with a residual in float64 on a 33 x 49 map (what 129 x 193 gives in layer2) and on its [W][H] reading: 100 x the whole networks' 1e-4"""
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(2, 32, 33, 49, generator=gen, dtype=torch.float64).relu()
    w1, w2 = (torch.randn(32, 32, 3, 3, generator=gen, dtype=torch.float64) / 17 for _ in range(2))
    block = lambda v: (F.conv2d(F.conv2d(v, w1, None, 1, 1).relu(), w2, None, 1, 1) + v).relu()
    y, yt = block(x), block(T.transposed_read(x)).reshape(x.shape)
    assert float((y - yt).abs().max() / y.abs().max()) >= 100 * 1e-4
