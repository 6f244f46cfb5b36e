"""Folding the stems and the partial layers at odd crop sides (infer.fold(..., any_size=True, odd_sides=True): p3d_fx_conv_fwd_infer_masked_any, the
p3d_stem_*_any entries): symbols, the host-only predicates, the padded sides, the keyword, and in float64 on the CPU the two facts the stem route rests
on -- the conv of the zero-extended input has the conv of the input as its prefix, bit for bit, and a tail that pools over the pad columns is far from
the true stem.  No GPU needed."""
import ctypes
import inspect
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from oracle import np_net

NAMES = ('p3d_fx_conv_fwd_infer_masked_any_supported', 'p3d_fx_conv_fwd_infer_masked_any_workspace_bytes', 'p3d_fx_conv_fwd_infer_masked_any',
         'p3d_stem_any_padded', 'p3d_stem_any_supported', 'p3d_stem_image_any', 'p3d_stem_tail_infer_any')
GPU_BOUND = 1e-4                                      # the stems' bound in tests/test_infer_oddsides_gpu.py, relative to max(1, max |reference|)


def partial_convs(model, hw, n=2):
    """(name, x shape, weight shape, stride, pad) of every partial conv of layer1 and layer2 (stride-16 geometry: layer1 stride 1, layer2 stride 2) on an
    hw x hw map behind the pool; the downsamples are dense and not listed (_trunk.py)."""
    kind, blocks = np_net.LAYERS[model]
    exp = 1 if kind == 'basic' else 4
    out, inplanes = [], 64
    for li, (planes, nb, s) in enumerate(zip((64, 128), blocks[:2], (1, 2)), 1):
        for b in range(nb):
            bs = s if b == 0 else 1
            ho = (hw - 1) // bs + 1
            tag = 'layer%d.%d.' % (li, b)
            if kind == 'basic':
                out.append((tag + 'conv1', (n, inplanes, hw, hw), (planes, inplanes, 3, 3), bs, 1))
                out.append((tag + 'conv2', (n, planes, ho, ho), (planes, planes, 3, 3), 1, 1))
            else:
                out.append((tag + 'conv1', (n, inplanes, hw, hw), (planes, inplanes, 1, 1), 1, 0))
                out.append((tag + 'conv2', (n, planes, hw, hw), (planes, planes, 3, 3), bs, 1))
                out.append((tag + 'conv3', (n, planes, ho, ho), (planes * 4, planes, 1, 1), 1, 0))
            inplanes, hw = planes * exp, ho
    return out


def _padded(pkg, h, w):
    hp, wp = ctypes.c_int32(), ctypes.c_int32()
    ok = pkg._lib.lib().p3d_stem_any_padded(h, w, ctypes.byref(hp), ctypes.byref(wp))
    return ok, hp.value, wp.value


def test_symbols_in_header_and_bound(pkg):
    header = open(os.path.join(ROOT, 'include', 'p3d_hip.h')).read()
    for name in NAMES:
        assert name + '(' in header, name
        assert name in pkg._lib.SIGNATURES, name
        assert hasattr(pkg._lib.lib(), name), name


def test_queries_are_host_only(pkg):
    L = pkg._lib.lib()
    assert L.p3d_fx_conv_fwd_infer_masked_any_supported(None) == 0
    assert L.p3d_fx_conv_fwd_infer_masked_any_workspace_bytes(None) == 0
    d = pkg.ops._desc((2, 128, 33, 33), (128, 128, 3, 3), 1, 1, 1)
    assert L.p3d_fx_conv_fwd_infer_masked_any_supported(ctypes.byref(d)) == 1
    assert L.p3d_fx_conv_fwd_infer_masked_any_workspace_bytes(ctypes.byref(d)) > 0


@pytest.mark.parametrize('model', ['resnet18', 'resnet50'])
@pytest.mark.parametrize('hw', [65, 33])
def test_admits_every_partial_conv_of_layer1_and_layer2(pkg, model, hw):
    L = pkg._lib.lib()
    convs = partial_convs(model, hw)
    assert len(convs) == {'resnet18': 8, 'resnet50': 21}[model]
    for name, xs, ws, s, pad in convs:
        d = pkg.ops._desc(xs, ws, s, pad, 1)
        assert d.W % 4 or d.Wo % 4, name
        assert L.p3d_fx_conv_fwd_infer_masked_any_supported(ctypes.byref(d)) == 1, (name, xs, ws, s, pad)
        assert L.p3d_fx_conv_fwd_infer_masked_supported(ctypes.byref(d)) == 0, name       # the aligned masked entry keeps its verdict


def test_partial_shapes_agree_with_the_model(pkg):
    args = pkg.opts.parse(['-model', 'resnet50', '-suffix', 't', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1', '-num_joints', '17',
                           '-depth_only'])
    net = pkg.partial_depthnet.resnet50(args, False)
    got = []
    for lname in ('layer1', 'layer2'):
        for blk in getattr(net, lname):
            assert blk.partial
            got += [(tuple(m.weight.shape), m.stride[0], m.padding[0]) for m in (getattr(blk, c) for c, _ in blk._chain)]
    assert got == [(ws, s, pad) for _, _, ws, s, pad in partial_convs('resnet50', 65)]


def test_masked_any_refuses(pkg):
    L = pkg._lib.lib()
    D = pkg.ops._desc
    no = {
        'K < 64': D((2, 64, 33, 33), (32, 64, 3, 3), 1, 1, 1),
        'C % 16': D((2, 72, 33, 33), (64, 72, 3, 3), 1, 1, 1),
        'channel window': D((2, 64, 33, 33), (64, 128, 1, 1), 1, 0, 1, c_offset=64, c_total=128),
        'accumulate 1': D((2, 64, 33, 33), (64, 64, 3, 3), 1, 1, 1, accumulate=1),
        'even filter': D((2, 64, 33, 33), (64, 64, 2, 2), 1, 0, 1),
        'stride 3': D((2, 64, 33, 33), (64, 64, 3, 3), 3, 1, 1),
    }
    for why, d in no.items():
        assert L.p3d_fx_conv_fwd_infer_masked_any_supported(ctypes.byref(d)) == 0, why
    assert L.p3d_fx_conv_fwd_infer_masked_any_supported(ctypes.byref(D((2, 64, 33, 33), (64, 64, 3, 3), 1, 1, 1))) == 1


def test_the_aligned_masked_entry_keeps_its_verdicts(pkg):
    L = pkg._lib.lib()
    for hw, want in ((65, 0), (33, 0), (17, 0), (32, 1), (16, 1)):
        d = pkg.ops._desc((2, 128, hw, hw), (128, 128, 3, 3), 1, 1, 1)
        assert L.p3d_fx_conv_fwd_infer_masked_supported(ctypes.byref(d)) == want, hw
        assert L.p3d_fx_conv_fwd_infer_masked_any_supported(ctypes.byref(d)) == 1, hw


def test_padded_sides(pkg):
    L = pkg._lib.lib()
    assert _padded(pkg, 257, 257) == (1, 264, 264)
    assert _padded(pkg, 129, 129) == (1, 136, 136)
    assert _padded(pkg, 33, 33) == (1, 40, 40)
    ok, hp, wp = _padded(pkg, 33, 49)
    assert ok and hp >= 33 and wp >= 49 and L.p3d_stem_supported(3, 1, hp, wp, 64) == 1
    for h in range(8, 140):
        for w in (h, h + 16, 2 * h + 1):
            ok, hp, wp = _padded(pkg, h, w)
            assert ok and h <= hp < h + 8 and w <= wp < w + 8, (h, w, hp, wp)
            assert L.p3d_stem_supported(2, 3, hp, wp, 64) == 1, (h, w, hp, wp)
            assert L.p3d_stem_any_supported(2, 3, h, w, 64) == 1
            if L.p3d_stem_supported(2, 3, h, w, 64):          # an already supported pair maps to itself
                assert (hp, wp) == (h, w)
    assert _padded(pkg, 128, 128) == (1, 128, 128) and _padded(pkg, 256, 256) == (1, 256, 256)
    assert _padded(pkg, 7, 64)[0] == 0 and _padded(pkg, 64, 5)[0] == 0 and L.p3d_stem_any_supported(2, 3, 7, 64, 64) == 0
    assert L.p3d_stem_any_supported(2, 3, 129, 129, 40) == 0          # K % 16, as p3d_stem_supported
    assert L.p3d_stem_any_padded(129, 129, None, None) == 1           # (the outputs are optional)


def test_the_stem_predicates_keep_their_verdicts(pkg):
    L = pkg._lib.lib()
    assert L.p3d_stem_supported(2, 3, 129, 129, 64) == 0 and L.p3d_stem_masked_supported(2, 1, 129, 129, 64) == 0
    assert L.p3d_stem_supported(2, 3, 257, 257, 64) == 0 and L.p3d_stem_masked_supported(2, 1, 257, 257, 64) == 0
    assert L.p3d_stem_supported(2, 3, 128, 128, 64) == 1 and L.p3d_stem_masked_supported(2, 1, 128, 128, 64) == 1


def test_keyword(pkg):
    for fn in (pkg.infer.fold, pkg.infer.FoldedConv.__init__, pkg.infer.FoldedNet.__init__):
        p = inspect.signature(fn).parameters
        assert 'odd_sides' in p and p['odd_sides'].default is False, fn


# ---- the design of the stem route, in float64 ------------------------------------------------------------------------------------------------------
def _stem_case(pkg, hw, seed=0):
    h, w = (hw, hw) if isinstance(hw, int) else hw
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 3, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(16, 3, 7, 7, generator=g, dtype=torch.float64) / 12
    b = 0.2 * torch.randn(16, generator=g, dtype=torch.float64)
    ok, hp, wp = _padded(pkg, h, w)
    assert ok
    return x, wt, b, F.pad(x, (0, wp - w, 0, hp - h))


@pytest.mark.parametrize('hw', [33, 129, 130, (33, 49)], ids=str)
def test_padded_conv_prefix_is_bit_equal(pkg, hw):
    """the 7x7 / stride 2 / pad 3 conv of the zero-extended input, in its first Ho rows and Wo columns, IS the conv of the input: the zeros are the conv's own padding"""
    x, wt, _, xp = _stem_case(pkg, hw)
    c, cp = F.conv2d(x, wt, None, 2, 3), F.conv2d(xp, wt, None, 2, 3)
    ho, wo = c.shape[2:]
    assert (ho, wo) == ((x.shape[2] - 1) // 2 + 1, (x.shape[3] - 1) // 2 + 1) and cp.shape[2] >= ho and cp.shape[3] >= wo
    assert torch.equal(cp[:, :, :ho, :wo], c)


@pytest.mark.parametrize('hw', [33, 129, 130], ids=str)
def test_a_tail_over_the_pad_columns_is_far_from_the_stem(pkg, hw):
    """the pad columns of the pitched conv hold real, non-zero outputs (windows that still reach the image edge): a tail that lets them into its 3x3 windows
    differs from relu(maxpool(conv) + b) by at least 100 x the GPU bound.  (Conv widths odd: at an even width, 131 -> 66, the last window ends inside the
    map and the bug would not show.)"""
    x, wt, b, xp = _stem_case(pkg, hw, seed=1)
    c, cp = F.conv2d(x, wt, None, 2, 3), F.conv2d(xp, wt, None, 2, 3)
    ho, wo = c.shape[2:]
    assert wo % 2 == 1
    assert float(cp[:, :, :ho, wo].abs().max()) > 0             # the first pad column is not zero
    bb = b[None, :, None, None]
    want = torch.relu(F.max_pool2d(c, 3, 2, 1) + bb)
    wrong = torch.relu(F.max_pool2d(cp, 3, 2, 1) + bb)[:, :, :want.shape[2], :want.shape[3]]
    gap = float((wrong - want).abs().max() / max(1.0, float(want.abs().max())))
    print('pad-column tail gap', hw, gap)
    assert gap >= 100 * GPU_BOUND
