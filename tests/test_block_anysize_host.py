"""The residual-block executor at any map width (ops.block_any / p3d_block_any_enable / P3D_BLOCK_ANY), the host side: the switch, what p3d_block_supported admits with
it off and on, the image format and the workspace of a ragged block, and that every instance p3d_fx_conv_any_sums_instances reports is named by a case of
tests/test_block_anysize_gpu.py.  The library loads, nothing launches.  No GPU needed."""
import ctypes
import os
import subprocess
import sys

import pytest

NEW = ('p3d_block_any_enable', 'p3d_block_any_supported', 'p3d_fx_conv_any_sums_instances', 'p3d_fx_conv_fused_partial_rows_any', 'p3d_fx_act_image_fused')


def block_desc(pkg, kind, inplanes, planes, stride, dil, n, h, with_ds, masked=0):
    """the descriptor ops_block._Plan builds for _trunk.BasicBlock / Bottleneck(inplanes, planes, stride, dil) on an [n, inplanes, h, w] input"""
    h, w = (h, h) if isinstance(h, int) else h
    d = pkg._lib.STRUCTS['p3d_block_desc']()
    if kind == 'basic':
        chain = [(planes, 3, stride, dil, dil), (planes, 3, 1, 1, 1)]
    else:
        chain = [(planes, 1, 1, 0, 1), (planes, 3, stride, dil, dil), (4 * planes, 1, 1, 0, 1)]
    d.nconv, d.masked, d.has_downsample, d.relu_out = len(chain), masked, int(with_ds), 1
    shape = (n, inplanes, h, w)
    for i, (k, r, s, pad, dl) in enumerate(chain):
        cd = pkg.ops._desc(shape, (k, shape[1], r, r), s, pad, dl)
        d.conv[i] = cd
        d.eps[i], d.momentum[i] = 1e-5, 0.1
        shape = (n, k, cd.Ho, cd.Wo)
    if with_ds:
        d.conv[3] = pkg.ops._desc((n, inplanes, h, w), (shape[1], inplanes, 1, 1), stride, 0, 1)
        d.eps[3], d.momentum[3] = 1e-5, 0.1
    return d


@pytest.fixture
def switch(pkg):
    """sets the switch for the test body; restores what it found, and the forced split counts"""
    before = pkg.ops.block_any(False)
    try:
        yield pkg.ops.block_any
    finally:
        pkg.ops.block_any(before)
        pkg._lib.lib().p3d_fx_tune(0, 0)
        pkg._lib.lib().p3d_fx_tune(1, 0)


def test_entries_are_declared_and_bound(pkg):
    handle = ctypes.CDLL(pkg._lib.LIB_PATH)
    for name in NEW:
        assert name in pkg._lib.SIGNATURES and hasattr(handle, name), name
    assert pkg._lib.SIGNATURES['p3d_fx_conv_any_sums_instances'] == pkg._lib.SIGNATURES['p3d_fx_conv_instances']
    assert pkg._lib.SIGNATURES['p3d_fx_conv_fused_partial_rows_any'] == pkg._lib.SIGNATURES['p3d_fx_conv_fused_partial_rows']
    assert hasattr(pkg.ops, 'block_any')
    assert ctypes.sizeof(pkg._lib.STRUCTS['p3d_block_io']) == 592                       # no new field: the image of x travels in aimg[3]


def test_switch_returns_the_previous_setting_and_bumps_the_epoch(pkg, switch):
    L = pkg._lib.lib()
    assert switch(True) is False and switch(True) is True and switch(False) is True and switch(False) is False
    assert L.p3d_block_any_enable(1) == 0 and L.p3d_block_any_enable(0) == 1
    e0 = pkg.ops.X3_EPOCH
    switch(False)
    assert pkg.ops.X3_EPOCH > e0                                                         # cached block plans are remade
    # independent of the other any-width switches: none moves it, it moves none
    others = (pkg.ops.x3_any, pkg.ops.x3_any_partial, pkg.ops.x3_any_images, pkg.ops.x3_any_strided, pkg.ops.bn_any)
    before = [f(True) for f in others]
    try:
        assert switch(True) is False
        assert all(f(True) is True for f in others)
        assert switch(False) is True
        assert all(f(False) is True for f in others)
        assert switch(False) is False
    finally:
        for f, v in zip(others, before):
            f(v)


@pytest.mark.parametrize('value,want', [(None, 0), ('1', 1), ('0', 0)])
def test_switch_follows_the_environment(pkg, value, want):
    """a fresh process that only loads the library: P3D_BLOCK_ANY=1 turns the switch on, anything else leaves it off"""
    env = {k: v for k, v in os.environ.items() if k != 'P3D_BLOCK_ANY'}
    if value is not None:
        env['P3D_BLOCK_ANY'] = value
    code = 'import ctypes, sys; print(ctypes.CDLL(sys.argv[1]).p3d_block_any_enable(0))'
    out = subprocess.run([sys.executable, '-c', code, pkg._lib.LIB_PATH], env=env, capture_output=True, text=True, check=True).stdout
    assert int(out.strip()) == want


#          kind          inplanes planes stride dil  N  H[xW]  downsample
RAGGED = [('bottleneck', 256, 64, 1, 1, 3, 5, False),                # HW = 25 = 1 mod 4
          ('bottleneck', 64, 64, 1, 1, 2, (7, 9), True),             # 63 = 3 mod 4
          ('basic', 64, 64, 1, 1, 4, (6, 7), False),                 # 42 = 2 mod 4
          ('basic', 128, 128, 1, 1, 5, 9, False),
          ('bottleneck', 256, 128, 1, 2, 2, 17, True),               # dilation 2
          ('bottleneck', 1024, 256, 1, 1, 64, 17, False),            # ResNet-50 at the default 257 crop, batch 64: layer3.1 ...
          ('bottleneck', 2048, 512, 1, 1, 64, 17, False),            #   layer4.1
          ('bottleneck', 256, 64, 1, 1, 64, 65, False),              #   layer1.1
          ('basic', 64, 64, 1, 1, 2, 6, False)]                      # HW = 36 is a multiple of 4, the rows of 6 pixels are not: refused today for its map size all the same
ALIGNED = [('bottleneck', 512, 128, 1, 1, 4, 16, False), ('bottleneck', 256, 128, 2, 1, 4, 32, True), ('basic', 64, 64, 1, 1, 4, 32, False)]
REFUSED = [('bottleneck', 256, 128, 2, 1, 2, 33, True),              # a stride-2 block at 33 x 33
           ('basic', 128, 256, 2, 1, 4, 33, True),
           ('bottleneck', 160, 40, 1, 1, 2, 17, False),              # C = 160 (the block tests/test_block_gpu.py keeps out): 40-channel convolutions, below 64 and no whole 16-channel rows
           ('bottleneck', 288, 72, 1, 1, 2, 17, False),              # 72 channels: above the 64-channel floor, refused for `% 16` alone
           ('bottleneck', 256, 64, 1, 1, 2, 3, False)]               # a 3 x 3 map: fewer than 16 pixels


@pytest.mark.parametrize('case', RAGGED, ids=str)
def test_ragged_blocks_are_admitted_only_with_the_switch_on(pkg, switch, case):
    L = pkg._lib.lib()
    d = block_desc(pkg, *case)
    b = ctypes.byref(d)
    assert L.p3d_block_supported(b) == 0 and L.p3d_block_any_supported(b) == 0
    m = ctypes.c_size_t()
    assert L.p3d_block_workspace_bytes(b, ctypes.byref(m), None) != 0                    # refused, as ever
    switch(True)
    assert L.p3d_block_supported(b) == 1 and L.p3d_block_any_supported(b) == 1
    # plane images: 6 B per element
    for n, c, hw in ((3, 64, 25), (2, 256, 63), (64, 1024, 289)):
        assert L.p3d_block_image_bytes(b, n, c, hw) == 6 * n * c * hw
    before = pkg.ops.set_x3(False)                                                       # P3D_X3=0 keeps everything off the x3 kernels
    try:
        assert L.p3d_block_supported(b) == 0 and L.p3d_block_any_supported(b) == 0
    finally:
        pkg.ops.set_x3(before)


@pytest.mark.parametrize('case', ALIGNED, ids=str)
def test_aligned_answers_do_not_look_at_the_switch(pkg, switch, case):
    L = pkg._lib.lib()
    d = block_desc(pkg, *case)
    b = ctypes.byref(d)
    got = []
    for on in (False, True):
        switch(on)
        m, s = ctypes.c_size_t(), ctypes.c_size_t()
        assert L.p3d_block_supported(b) == 1 and L.p3d_block_any_supported(b) == 0
        assert L.p3d_block_workspace_bytes(b, ctypes.byref(m), ctypes.byref(s)) == 0
        got.append((m.value, s.value, L.p3d_block_image_bytes(b, 4, 128, 256)))
    assert got[0] == got[1] and got[0][2] == 4 * 4 * 128 * 256                           # fp32 row images, 4 B per element


@pytest.mark.parametrize('case', REFUSED, ids=str)
def test_refusals_with_the_switch_on(pkg, switch, case):
    L = pkg._lib.lib()
    d = block_desc(pkg, *case)
    for on in (False, True):
        switch(on)
        assert L.p3d_block_supported(ctypes.byref(d)) == 0 and L.p3d_block_any_supported(ctypes.byref(d)) == 0, on


def test_masked_blocks_at_odd_maps_stay_refused(pkg, switch):
    L = pkg._lib.lib()
    d = block_desc(pkg, 'bottleneck', 256, 64, 1, 1, 2, 17, False, masked=1)
    dense = block_desc(pkg, 'bottleneck', 256, 64, 1, 1, 2, 17, False)
    switch(True)
    assert L.p3d_block_supported(ctypes.byref(dense)) == 1
    assert L.p3d_block_supported(ctypes.byref(d)) == 0 and L.p3d_block_any_supported(ctypes.byref(d)) == 0
    aligned = block_desc(pkg, 'bottleneck', 256, 64, 1, 1, 2, 16, False, masked=1)       # (masked blocks at aligned maps: as ever, three-plane images)
    assert L.p3d_block_supported(ctypes.byref(aligned)) == 1 and L.p3d_block_image_bytes(ctypes.byref(aligned), 2, 64, 256) == 6 * 2 * 64 * 256


@pytest.mark.parametrize('case', RAGGED[:6], ids=str)
def test_workspace_covers_the_ragged_plans_of_every_slot(pkg, switch, case):
    """main = [conv scratch | partial sums | the downsample conv's partial sums], side = the weight-gradient slabs: each at least what the ragged plan of every slot
    needs -- its weight image, under forced split counts its slabs on 16-B lines, one partial row per 128-pixel tile in either direction, the image-fed slabs"""
    L = pkg._lib.lib()
    d = block_desc(pkg, *case)
    b = ctypes.byref(d)
    switch(True)
    slots = [i for i in range(4) if i < d.nconv or (i == 3 and d.has_downsample)]
    line = lambda elems: (elems + 3) // 4 * 4 * 4
    up = lambda v: (v + 255) // 256 * 256
    for force in (0, 2, 3):
        L.p3d_fx_tune(1, force)
        L.p3d_fx_tune(0, force)
        m, s = ctypes.c_size_t(), ctypes.c_size_t()
        assert L.p3d_block_workspace_bytes(b, ctypes.byref(m), ctypes.byref(s)) == 0
        conv_ws = part = side = 0
        for i in slots:
            cd = d.conv[i]
            cb = ctypes.byref(cd)
            conv_ws = max(conv_ws, L.p3d_fx_conv_img_any_workspace_bytes(cb, 0), L.p3d_fx_conv_img_any_workspace_bytes(cb, 1))
            side = max(side, L.p3d_fx_conv_img_any_workspace_bytes(cb, 2))
            part = max(part, -(-cd.N * cd.Ho * cd.Wo // 128) * cd.K * 8, -(-cd.N * cd.H * cd.W // 128) * cd.C * 8, max(cd.K, cd.C) * 64 * 3 * 8)
            assert L.p3d_fx_conv_fused_partial_rows_any(0, cb) == -(-cd.N * cd.Ho * cd.Wo // 128)
            assert L.p3d_fx_conv_fused_partial_rows_any(1, cb) == -(-cd.N * cd.H * cd.W // 128)
            if force:
                nk = cd.R * cd.S * cd.C // 16
                if nk >= force:
                    assert conv_ws >= min(force, nk) * line(cd.N * cd.K * cd.Ho * cd.Wo), (i, force)
        assert m.value >= up(conv_ws) + 2 * up(part), (force, m.value, conv_ws, part)
        assert s.value >= side, force
    L.p3d_fx_tune(1, 0)
    L.p3d_fx_tune(0, 0)


def test_every_new_instance_has_a_gpu_case(pkg):
    """what tests/test_fx_instances_host.py keeps for the main list: an instance added to the list of the ragged BatchNorm instances without a case that runs it alone fails here"""
    import test_block_anysize_gpu as G
    new = pkg.ops.fx_conv_any_sums_instances()
    assert len(new) == len(set(new)) >= 2
    assert not set(new) & set(pkg.ops.fx_conv_instances())                               # a list of their own
    assert (0, 1, 0, 1, 0, 1, 0) in new and (0, 1, 0, 2, 0, 1, 0) in new
    named = {c[2] for c in G.INSTANCE_CASES}
    assert set(new) <= named, sorted(set(new) - named)
    assert named <= set(new), sorted(named - set(new))                                   # and no case names an instance that does not exist
    for name, pass_, inst, *_ in G.INSTANCE_CASES:
        assert (inst[3] == 1) == (pass_ == 'fwd'), name
