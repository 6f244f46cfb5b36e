"""Strided residual blocks at any map width (ops.block_any_strided / p3d_block_any_strided_enable / P3D_BLOCK_ANY_STRIDED), the host side: the switch, its
independence of the six other any-width switches, the admission table of p3d_block_supported / p3d_block_any_supported, the workspace of an admitted block and the
blocks of the two ResNets at the default 257 crop.  The library loads, nothing launches.  No GPU needed."""
import ctypes
import os
import subprocess
import sys

import pytest

from test_block_anysize_host import ALIGNED, RAGGED, block_desc

NEW = ('p3d_block_any_strided_enable', 'p3d_block_strided_join', 'p3d_fx_conv_dgrad_strided_img_any_supported', 'p3d_fx_conv_dgrad_strided_img_any_workspace_bytes',
       'p3d_fx_conv_dgrad_strided_img_any')

#           kind          inplanes planes stride dil  N  H[xW]   downsample
STRIDED = [('bottleneck', 256, 128, 2, 1, 2, 33, True),           # the block that stays out today
           ('bottleneck', 128, 64, 2, 1, 3, (9, 7), True),        # HW = 63, class planes of four sizes
           ('basic', 64, 128, 2, 1, 2, 9, True),                  # the stride on conv 0
           ('bottleneck', 128, 64, 2, 1, 2, (6, 14), True)]       # even sides the aligned rule refuses for W % 8
ALIGNED_STRIDED = ('bottleneck', 256, 128, 2, 1, 4, 32, True)


def _others(pkg):
    return (pkg.ops.x3_any, pkg.ops.x3_any_partial, pkg.ops.x3_any_images, pkg.ops.x3_any_strided, pkg.ops.bn_any, pkg.ops.block_any)


@pytest.fixture
def switches(pkg):
    """both block switches off for the test body; what it found is restored afterwards"""
    before = (pkg.ops.block_any_strided(False), pkg.ops.block_any(False))
    try:
        yield pkg.ops.block_any_strided, pkg.ops.block_any
    finally:
        pkg.ops.block_any_strided(before[0])
        pkg.ops.block_any(before[1])


def _answers(pkg, d):
    L = pkg._lib.lib()
    return L.p3d_block_supported(ctypes.byref(d)), L.p3d_block_any_supported(ctypes.byref(d))


def test_entries_are_declared_and_bound(pkg):
    handle = ctypes.CDLL(pkg._lib.LIB_PATH)
    for name in NEW:
        assert name in pkg._lib.SIGNATURES and hasattr(handle, name), name
    assert pkg._lib.SIGNATURES['p3d_fx_conv_dgrad_strided_img_any'] == pkg._lib.SIGNATURES['p3d_fx_conv_dgrad_img_any']
    assert pkg._lib.SIGNATURES['p3d_block_any_strided_enable'] == pkg._lib.SIGNATURES['p3d_block_any_enable']
    assert hasattr(pkg.ops, 'block_any_strided')
    assert ctypes.sizeof(pkg._lib.STRUCTS['p3d_block_io']) == 592


def test_switch_returns_the_previous_setting_and_bumps_the_epoch(pkg, switches):
    strided, _ = switches
    L = pkg._lib.lib()
    assert strided(True) is False and strided(True) is True and strided(False) is True and strided(False) is False
    assert L.p3d_block_any_strided_enable(1) == 0 and L.p3d_block_any_strided_enable(0) == 1
    e0 = pkg.ops.X3_EPOCH
    strided(False)
    assert pkg.ops.X3_EPOCH > e0                                                         # cached block plans are remade
    # none of the six other switches moves it, it moves none of them
    others = _others(pkg)
    before = [f(True) for f in others]
    try:
        assert strided(True) is False
        assert all(f(True) is True for f in others)
        assert strided(False) is True
        assert all(f(False) is True for f in others)
        assert strided(False) is False
    finally:
        for f, v in zip(others, before):
            f(v)


@pytest.mark.parametrize('value,want', [(None, 0), ('1', 1), ('0', 0)])
def test_switch_follows_the_environment(pkg, value, want):
    """a fresh process that only loads the library: P3D_BLOCK_ANY_STRIDED=1 turns the switch on, anything else -- P3D_BLOCK_ANY=1 too -- leaves it off"""
    env = {k: v for k, v in os.environ.items() if k != 'P3D_BLOCK_ANY_STRIDED'}
    env['P3D_BLOCK_ANY'] = '1'
    if value is not None:
        env['P3D_BLOCK_ANY_STRIDED'] = value
    code = 'import ctypes, sys; print(ctypes.CDLL(sys.argv[1]).p3d_block_any_strided_enable(0))'
    out = subprocess.run([sys.executable, '-c', code, pkg._lib.LIB_PATH], env=env, capture_output=True, text=True, check=True).stdout
    assert int(out.strip()) == want


@pytest.mark.parametrize('case', STRIDED, ids=str)
def test_strided_ragged_blocks_are_admitted_by_their_own_switch_alone(pkg, switches, case):
    strided, plain = switches
    L = pkg._lib.lib()
    d = block_desc(pkg, *case)
    b = ctypes.byref(d)
    assert _answers(pkg, d) == (0, 0)
    plain(True)                                                                          # P3D_BLOCK_ANY admits what it admits today: no strided block
    assert _answers(pkg, d) == (0, 0)
    m = ctypes.c_size_t()
    assert L.p3d_block_workspace_bytes(b, ctypes.byref(m), None) != 0
    plain(False)
    strided(True)
    assert _answers(pkg, d) == (1, 1)
    for n, c, hw in ((3, 64, 25), (2, 256, 63)):                                         # a ragged block in every respect: plane images, 6 B per element
        assert L.p3d_block_image_bytes(b, n, c, hw) == 6 * n * c * hw
    plain(True)
    assert _answers(pkg, d) == (1, 1)
    before = pkg.ops.set_x3(False)                                                       # P3D_X3=0 keeps everything off the x3 kernels
    try:
        assert _answers(pkg, d) == (0, 0)
    finally:
        pkg.ops.set_x3(before)


@pytest.mark.parametrize('case', STRIDED, ids=str)
def test_no_other_switch_changes_the_answer_for_a_strided_ragged_block(pkg, switches, case):
    strided, _ = switches
    d = block_desc(pkg, *case)
    others = _others(pkg)
    before = [f(False) for f in others]
    try:
        for on in (False, True):
            strided(on)
            want = (1, 1) if on else (0, 0)
            for f in others:
                f(True)
                assert _answers(pkg, d) == want, (on, f.__name__)
                f(False)
                assert _answers(pkg, d) == want, (on, f.__name__)
            for f in others:
                f(True)
            assert _answers(pkg, d) == want, on
            for f in others:
                f(False)
    finally:
        for f, v in zip(others, before):
            f(v)


def test_the_switch_changes_no_answer_for_the_other_kinds_of_block(pkg, switches):
    """aligned blocks (a strided one among them), stride-1 ragged blocks and masked blocks: the same answers, workspaces and image sizes with the switch off and on"""
    strided, plain = switches
    L = pkg._lib.lib()
    masked = [block_desc(pkg, 'bottleneck', 256, 64, 1, 1, 2, 17, False, masked=1), block_desc(pkg, 'bottleneck', 256, 64, 1, 1, 2, 16, False, masked=1)]
    descs = [block_desc(pkg, *c) for c in ALIGNED + [ALIGNED_STRIDED] + RAGGED] + masked
    for any_on in (False, True):
        plain(any_on)
        got = []
        for on in (False, True):
            strided(on)
            row = []
            for d in descs:
                m, s = ctypes.c_size_t(), ctypes.c_size_t()
                rc = L.p3d_block_workspace_bytes(ctypes.byref(d), ctypes.byref(m), ctypes.byref(s))
                row.append(_answers(pkg, d) + (rc, m.value if rc == 0 else 0, s.value if rc == 0 else 0, L.p3d_block_image_bytes(ctypes.byref(d), 2, 64, 25)))
            got.append(row)
        assert got[0] == got[1], any_on
    # a stride-1 ragged block: refused by the new switch alone, admitted by P3D_BLOCK_ANY
    d = block_desc(pkg, *RAGGED[0])
    plain(False)
    strided(True)
    assert _answers(pkg, d) == (0, 0)
    plain(True)
    assert _answers(pkg, d) == (1, 1)
    # an aligned strided block: admitted as an aligned block whatever the switches say
    d = block_desc(pkg, *ALIGNED_STRIDED)
    for a in (False, True):
        for s in (False, True):
            plain(a)
            strided(s)
            assert _answers(pkg, d) == (1, 0)


def test_refusals_with_the_switch_on(pkg, switches):
    strided, plain = switches
    strided(True)
    plain(True)
    # a masked strided block at an odd map
    assert _answers(pkg, block_desc(pkg, 'bottleneck', 256, 128, 2, 1, 2, 33, True, masked=1)) == (0, 0)
    # an output map of fewer than 16 pixels: ResNet-18's layer3.0 at 5 -> 3
    assert _answers(pkg, block_desc(pkg, 'basic', 128, 256, 2, 1, 2, 5, True)) == (0, 0)
    # channel counts outside the rule
    assert _answers(pkg, block_desc(pkg, 'bottleneck', 288, 72, 2, 1, 2, 17, True)) == (0, 0)
    # a 1x1 stride 2 on the main chain (the data gradient leaves three of four input pixels untouched): the stride moved from the 3x3 to the opening 1x1
    d = block_desc(pkg, 'bottleneck', 256, 128, 2, 1, 2, 33, True)
    assert _answers(pkg, d) == (1, 1)
    n, h = 2, 33
    c0 = pkg.ops._desc((n, 256, h, h), (128, 256, 1, 1), 2, 0, 1)
    c1 = pkg.ops._desc((n, 128, c0.Ho, c0.Wo), (128, 128, 3, 3), 1, 1, 1)
    d.conv[0], d.conv[1] = c0, c1
    assert (c1.Ho, c1.Wo) == (d.conv[2].H, d.conv[2].W) == (17, 17)
    assert _answers(pkg, d) == (0, 0)


@pytest.mark.parametrize('case', STRIDED, ids=str)
def test_workspace_covers_the_class_planes_of_every_strided_slot(pkg, switches, case):
    strided, _ = switches
    L = pkg._lib.lib()
    d = block_desc(pkg, *case)
    strided(True)
    m, s = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.p3d_block_workspace_bytes(ctypes.byref(d), ctypes.byref(m), ctypes.byref(s)) == 0
    up = lambda v: (v + 255) // 256 * 256
    seen = 0
    for i in range(4):
        if not (i < d.nconv or (i == 3 and d.has_downsample)):
            continue
        cd = d.conv[i]
        if cd.stride != 2:
            assert L.p3d_fx_conv_dgrad_strided_img_any_supported(ctypes.byref(cd)) == 0 and L.p3d_fx_conv_dgrad_strided_img_any_workspace_bytes(ctypes.byref(cd)) == 0
            continue
        seen += 1
        assert L.p3d_fx_conv_dgrad_strided_img_any_supported(ctypes.byref(cd)) == 1
        need = L.p3d_fx_conv_dgrad_strided_img_any_workspace_bytes(ctypes.byref(cd))
        planes = 4 * ((cd.N * cd.C * ((cd.H + 1) // 2) * ((cd.W + 1) // 2) + 3) // 4 * 4) * 4
        assert need >= up(planes) and need % 256 == 0
        part = max(cd.K, cd.C) * 64 * 3 * 8
        assert m.value >= need + 2 * up(part), (i, m.value, need)
    assert seen == 2                                                                     # the strided conv of the main chain and the downsample conv
    # the existing image-fed queries keep refusing the stride-2 data gradient
    cd = d.conv[3]
    assert L.p3d_fx_conv_img_any_supported(ctypes.byref(cd)) & 2 == 0


def _resnet_blocks(kind, n=2, side=257):
    """the block list of depthnet's ResNet-50 ('bottleneck') / ResNet-18 ('basic') at -stride 16: (kind, inplanes, planes, stride, dilation, N, H, downsample)"""
    h = ((side + 1) // 2 + 1) // 2                                                       # 7x7 stride-2 stem, 3x3 stride-2 pool: 257 -> 129 -> 65
    expansion, counts = (4, (3, 4, 6, 3)) if kind == 'bottleneck' else (1, (2, 2, 2, 2))
    inplanes, out = 64, []
    for planes, blocks, stride, dil in zip((64, 128, 256, 512), counts, (1, 2, 2, 1), (1, 1, 1, 2)):
        for i in range(blocks):
            first = i == 0
            ds = first and (stride != 1 or inplanes != planes * expansion)
            out.append((kind, inplanes, planes, stride if first else 1, dil if first else 1, n, h, ds))
            if first:
                h = (h - 1) // stride + 1
            inplanes = planes * expansion
    return out


@pytest.mark.parametrize('kind,count', [('bottleneck', 16), ('basic', 8)])
def test_every_block_of_the_resnets_at_the_default_crop_is_admitted(pkg, switches, kind, count):
    strided, plain = switches
    blocks = _resnet_blocks(kind)
    assert len(blocks) == count and [b[6] for b in blocks if b[3] == 2] == [65, 33]
    descs = [block_desc(pkg, *b) for b in blocks]
    assert sum(a[0] for a in (_answers(pkg, d) for d in descs)) == 0                     # 257: no map is aligned
    plain(True)
    assert [_answers(pkg, d)[0] for d in descs] == [0 if b[3] == 2 else 1 for b in blocks]
    strided(True)
    assert all(_answers(pkg, d) == (1, 1) for d in descs)
    plain(False)
    assert [_answers(pkg, d)[0] for d in descs] == [1 if b[3] == 2 else 0 for b in blocks]
