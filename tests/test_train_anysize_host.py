"""Training on the x3 kernels at any map width (ops.x3_any / p3d_x3_any_enable), the host side: the three p3d_conv2d_*_any_supported queries against the
rules written out here, over the geometry table and the ResNet-50 classes of the default 257 crop (maps of 65, 33 and 17); every older *_supported query and
every workspace query with the switch on against the switch off.  No GPU needed."""
import ctypes

import pytest

import geometry_table as T

NEW = ('p3d_x3_any_enable', 'p3d_conv2d_fwd_any_supported', 'p3d_conv2d_dgrad_any_supported', 'p3d_conv2d_wgrad_any_supported')
MIN_M = 96                       # the per-layer entries' channel-tile threshold

# ResNet-50 behind the stem at side 257 (batch 2 here: the verdicts do not depend on it); c, k, h, r, stride, pad, dil
RESNET = [(64, 64, 65, 1, 1, 0, 1), (64, 64, 65, 3, 1, 1, 1), (64, 256, 65, 1, 1, 0, 1), (256, 64, 65, 1, 1, 0, 1),
          (256, 128, 65, 1, 1, 0, 1), (128, 128, 65, 3, 2, 1, 1), (128, 512, 33, 1, 1, 0, 1), (512, 128, 33, 1, 1, 0, 1), (128, 128, 33, 3, 1, 1, 1), (256, 512, 65, 1, 2, 0, 1),
          (512, 256, 33, 1, 1, 0, 1), (256, 256, 33, 3, 2, 1, 1), (256, 1024, 17, 1, 1, 0, 1), (1024, 256, 17, 1, 1, 0, 1), (256, 256, 17, 3, 1, 1, 1), (512, 1024, 33, 1, 2, 0, 1),
          (1024, 512, 17, 1, 1, 0, 1), (512, 512, 17, 3, 1, 2, 2), (512, 2048, 17, 1, 1, 0, 1), (2048, 512, 17, 1, 1, 0, 1), (1024, 2048, 17, 1, 1, 0, 1), (2048, 272, 17, 3, 1, 1, 1)]


def rules(c, k, r, stride):
    """what the ragged instances admit: (forward, data gradient, weight gradient)"""
    fwd = c % 16 == 0 and c >= 32 and k >= MIN_M
    dgrad = k % 16 == 0 and k >= 32 and c % 4 == 0 and c >= MIN_M and stride == 1
    wgrad = k >= MIN_M and c >= MIN_M and (r == 1 or c % 64 == 0)
    return int(fwd), int(dgrad), int(wgrad)


def verdicts(L, d):
    b = ctypes.byref(d)
    return L.p3d_conv2d_fwd_any_supported(b), L.p3d_conv2d_dgrad_any_supported(b), L.p3d_conv2d_wgrad_any_supported(b)


@pytest.fixture
def switch(pkg):
    """sets the switch for the test body and restores what it found"""
    before = pkg.ops.x3_any(False)
    yield pkg.ops.x3_any
    pkg.ops.x3_any(before)


def test_entries_are_declared_and_bound(pkg):
    import test_abi
    declared = test_abi.declared_functions(pkg._lib.HEADER_PATH)
    handle = ctypes.CDLL(pkg._lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in pkg._lib.SIGNATURES and hasattr(handle, name), name
    assert sorted(pkg._lib.SIGNATURES) == declared


def test_switch_defaults_off_and_returns_the_previous_state(pkg):
    import os
    if os.environ.get('P3D_X3_ANY') != '1':
        before = pkg.ops.x3_any(True)
        try:
            assert before is False
            assert pkg.ops.x3_any(True) is True
        finally:
            assert pkg.ops.x3_any(False) is True
        assert pkg.ops.x3_any(False) is False
    L = pkg._lib.lib()
    assert L.p3d_conv2d_fwd_any_supported(None) == 0 and L.p3d_conv2d_dgrad_any_supported(None) == 0 and L.p3d_conv2d_wgrad_any_supported(None) == 0


@pytest.mark.parametrize('g', T.ROWS, ids=T.IDS)
def test_table_rows(pkg, switch, g):
    L = pkg._lib.lib()
    d = pkg.ops._desc((g.n, g.c, g.h, g.w), (g.k, g.c, g.r, g.r), g.stride, g.pad, g.dil)
    want = rules(g.c, g.k, g.r, g.stride)
    for on in (False, True):                                  # the queries do not look at the switch
        switch(on)
        assert verdicts(L, d) == want, on
        assert L.p3d_fx_conv_img_supported(ctypes.byref(d)) == g.x3          # the aligned predicates keep every verdict


@pytest.mark.parametrize('side_class', RESNET, ids=lambda s: 'c%d_k%d_%d_%dx%d_s%d_d%d' % (s[0], s[1], s[2], s[3], s[3], s[4], s[6]))
def test_resnet_classes_at_the_default_crop(pkg, side_class):
    c, k, h, r, stride, pad, dil = side_class
    L = pkg._lib.lib()
    d = pkg.ops._desc((2, c, h, h), (k, c, r, r), stride, pad, dil)
    assert h % 4 != 0 and L.p3d_fx_conv_img_supported(ctypes.byref(d)) == 0          # no aligned instance takes these maps
    got = verdicts(L, d)
    assert got == rules(c, k, r, stride)
    if 64 in (c, k):
        assert got[2] == 0 and (got[0] == 0 or k != 64)       # the 64-channel layers stay on fp32-MFMA where the per-layer threshold says so
    elif stride == 2:
        assert got == (1, 0, 1)                                # a strided data gradient stays on fp32-MFMA
    else:
        assert got == (1, 1, 1)


def test_refusals(pkg):
    L = pkg._lib.lib()

    def v(c, k, h, w, r, stride, pad, dil, window=None):
        d = pkg.ops._desc((3, c, h, w), (k, c if window is None else window[1], r, r), stride, pad, dil)
        if window is not None:
            d.c_offset, d.c_total = window
        return verdicts(L, d)

    assert v(128, 128, 17, 17, 3, 1, 1, 1) == (1, 1, 1)
    assert v(128, 128, 17, 17, 3, 2, 1, 1) == (1, 0, 1)                        # stride 2: no ragged data gradient
    assert v(128, 128, 19, 19, 1, 2, 0, 1) == (1, 0, 1)
    assert v(120, 128, 17, 17, 1, 1, 0, 1) == (0, 1, 1)                        # C % 16 != 0: the forward's reduction runs in steps of 16 channels
    assert v(120, 128, 17, 17, 3, 1, 1, 1) == (0, 1, 0)                        #   and a multi-tap weight gradient wants C % 64 == 0
    assert v(128, 120, 17, 17, 1, 1, 0, 1) == (1, 0, 1)                        # K % 16 != 0: the data gradient's reduction
    assert v(160, 128, 17, 17, 3, 1, 1, 1) == (1, 1, 0)                        # R > 1 and C % 64 != 0
    assert v(160, 128, 17, 17, 1, 1, 0, 1) == (1, 1, 1)
    assert v(128, 128, 17, 17, 1, 1, 0, 1, window=(0, 256)) == (0, 0, 0)       # a channel window of a wider weight
    assert v(128, 128, 17, 17, 1, 1, 0, 1, window=(128, 256)) == (0, 0, 0)
    assert v(64, 128, 17, 17, 3, 1, 1, 1) == (1, 0, 0)                         # under the per-layer threshold
    assert v(128, 64, 17, 17, 3, 1, 1, 1) == (0, 1, 0)
    bad = pkg.ops._desc((3, 128, 17, 17), (128, 128, 3, 3), 1, 1, 1)
    bad.Ho = 7
    assert verdicts(L, bad) == (0, 0, 0)
    before = pkg.ops.set_x3(False)                                             # P3D_X3=0 / set_x3(False) keeps everything on fp32-MFMA
    try:
        assert v(128, 128, 17, 17, 3, 1, 1, 1) == (0, 0, 0)
    finally:
        pkg.ops.set_x3(before)


def _queries(pkg, d):
    L = pkg._lib.lib()
    b = ctypes.byref(d)
    supported = (L.p3d_fx_conv_img_supported(b), L.p3d_fx_conv_fwd_infer_supported(b, 0), L.p3d_fx_conv_fwd_infer_supported(b, 1), L.p3d_fx_conv_fwd_infer_masked_supported(b),
                 L.p3d_fx_conv_fwd_infer_any_supported(b), L.p3d_hconv2d_fwd_infer_supported(b), L.p3d_f8conv2d_fwd_infer_supported(b))
    workspace = (L.p3d_conv2d_fwd_workspace_bytes(b), L.p3d_conv2d_dgrad_workspace_bytes(b), L.p3d_conv2d_wgrad_workspace_bytes(b))
    other = (L.p3d_fx_conv_fwd_infer_any_workspace_bytes(b), L.p3d_conv2d_bn_eval_fwd_workspace_bytes(b))
    return supported, workspace, other


def _shapes():
    for g in T.ROWS:
        yield g.name, (g.n, g.c, g.h, g.w), (g.k, g.c, g.r, g.r), g.stride, g.pad, g.dil, g.x3 == 7
    for c, k, h, r, stride, pad, dil in RESNET:
        for n in (2, 64):
            yield 'resnet', (n, c, h, h), (k, c, r, r), stride, pad, dil, False
    yield 'partial tile', (1, 128, 19, 17), (272, 128, 3, 3), 1, 1, 1, False
    yield 'split', (2, 2048, 17, 17), (272, 2048, 3, 3), 1, 1, 1, False


def test_existing_queries_do_not_move(pkg, switch):
    """every older *_supported verdict is the same with the switch on; the three per-layer workspace queries only grow, and not at all on aligned shapes; the
    workspace queries of other entries stay"""
    grew = 0
    for name, xs, ws, stride, pad, dil, aligned in _shapes():
        d = pkg.ops._desc(xs, ws, stride, pad, dil)
        switch(False)
        sup0, wk0, oth0 = _queries(pkg, d)
        switch(True)
        sup1, wk1, oth1 = _queries(pkg, d)
        switch(False)
        assert sup1 == sup0, (name, xs, ws)
        assert oth1[0] == oth0[0], (name, xs, ws)
        assert all(b >= a for a, b in zip(wk0, wk1)), (name, xs, ws, wk0, wk1)
        if aligned:
            assert wk1 == wk0 and oth1 == oth0, (name, xs, ws)
        grew += wk1 != wk0
        assert _queries(pkg, d) == (sup0, wk0, oth0)
    assert grew > 0                   # the ragged plans do ask for room somewhere (a weight image where the fp32-MFMA plan wants none, 16-B slab starts)


def test_workspace_covers_the_ragged_plans(pkg, switch):
    """with the switch on the queries cover the pre-split weight image (and the slabs of a forced split) of the ragged launch"""
    L = pkg._lib.lib()
    d = pkg.ops._desc((2, 128, 17, 17), (128, 128, 3, 3), 1, 1, 1)
    b = ctypes.byref(d)
    image = 9 * 128 * 128 * 6                                  # three bf16 pieces per weight, rows padded to the 128-row tile
    switch(True)
    assert L.p3d_conv2d_fwd_workspace_bytes(b) >= image and L.p3d_conv2d_dgrad_workspace_bytes(b) >= image
    assert L.p3d_conv2d_wgrad_workspace_bytes(b) >= 128 * 128 * 9 * 4
    L.p3d_fx_tune(1, 3)
    L.p3d_fx_tune(0, 3)
    try:
        slab = (2 * 128 * 17 * 17 + 3) // 4 * 4 * 4            # each slab starts on a 16-B line
        assert L.p3d_conv2d_fwd_workspace_bytes(b) >= image + 3 * slab and L.p3d_conv2d_dgrad_workspace_bytes(b) >= image + 3 * slab
        assert L.p3d_conv2d_wgrad_workspace_bytes(b) >= 3 * 128 * 128 * 9 * 4
    finally:
        L.p3d_fx_tune(1, 0)
        L.p3d_fx_tune(0, 0)
