"""Image operands at any map width (ops.x3_any_images / p3d_x3_any_images_enable), the host side: the new entries are declared and bound, what
p3d_fx_conv_img_any_supported admits and refuses, that its answer does not look at the switch, what the workspace query covers under forced slab counts, the size of
an activation image at odd H * W, and the switch itself.  The library loads, nothing launches.  No GPU needed."""
import ctypes
import os

import pytest

NEW = ('p3d_x3_any_images_enable', 'p3d_fx_conv_img_any_supported', 'p3d_fx_conv_img_any_workspace_bytes', 'p3d_fx_act_image_any',
       'p3d_fx_conv_fwd_img_any', 'p3d_fx_conv_dgrad_img_any', 'p3d_fx_conv_wgrad_img_any')

# n, c, h, w, k, r, stride, pad, dil -> the bits (1 forward, 2 data gradient, 4 weight gradient)
ADMITTED = [((2, 128, 17, 17, 128, 3, 1, 1, 1), 7), ((2, 512, 17, 19, 512, 3, 1, 2, 2), 7), ((1, 2048, 17, 17, 272, 3, 1, 1, 1), 7), ((2, 256, 19, 19, 128, 1, 1, 0, 1), 7),
            ((2, 128, 17, 17, 128, 3, 2, 1, 1), 5)]                       # stride 2: no ragged data gradient


def _desc(pkg, shape):
    n, c, h, w, k, r, stride, pad, dil = shape
    return pkg.ops._desc((n, c, h, w), (k, c, r, r), stride, pad, dil)


@pytest.fixture
def switch(pkg):
    """sets the switch for the test body; restores what it found, and the forced split counts"""
    before = pkg.ops.x3_any_images(False)
    try:
        yield pkg.ops.x3_any_images
    finally:
        pkg.ops.x3_any_images(before)
        pkg._lib.lib().p3d_fx_tune(0, 0)
        pkg._lib.lib().p3d_fx_tune(1, 0)


def test_entries_are_declared_and_bound(pkg):
    import test_abi
    declared = test_abi.declared_functions(pkg._lib.HEADER_PATH)
    handle = ctypes.CDLL(pkg._lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in pkg._lib.SIGNATURES and hasattr(handle, name), name
    assert sorted(pkg._lib.SIGNATURES) == declared
    # the signatures of the _img siblings
    for p in ('fwd', 'dgrad', 'wgrad'):
        assert pkg._lib.SIGNATURES['p3d_fx_conv_%s_img_any' % p] == pkg._lib.SIGNATURES['p3d_fx_conv_%s_img' % p], p
    assert pkg._lib.SIGNATURES['p3d_fx_conv_img_any_supported'] == pkg._lib.SIGNATURES['p3d_fx_conv_img_supported']
    assert pkg._lib.SIGNATURES['p3d_fx_conv_img_any_workspace_bytes'] == pkg._lib.SIGNATURES['p3d_fx_conv_img_workspace_bytes']
    assert hasattr(pkg.ops, 'x3_any_images')


@pytest.mark.parametrize('shape,bits', ADMITTED, ids=lambda v: '_'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_admitted_shapes(pkg, switch, shape, bits):
    L = pkg._lib.lib()
    d = _desc(pkg, shape)
    for on in (False, True):                                      # the query does not look at the switch
        switch(on)
        assert L.p3d_fx_conv_img_any_supported(ctypes.byref(d)) == bits, on
    if (shape[2] * shape[3]) % 4:
        assert L.p3d_fx_conv_img_supported(ctypes.byref(d)) == 0      # the aligned query refuses these maps


def test_refusals(pkg, switch):
    L = pkg._lib.lib()

    def bits(shape, window=None):
        d = _desc(pkg, shape)
        if window is not None:
            d.c_offset, d.c_total = window
        got = []
        for on in (False, True):                                  # the query does not look at the switch
            switch(on)
            got.append(L.p3d_fx_conv_img_any_supported(ctypes.byref(d)))
        assert got[0] == got[1]
        return got[0]

    assert bits((2, 128, 17, 17, 128, 3, 1, 1, 1)) == 7
    assert bits((2, 64, 17, 17, 64, 3, 1, 1, 1)) == 0                          # a 64-channel layer: below the per-layer threshold of 96 on either side
    assert bits((2, 64, 17, 17, 128, 3, 1, 1, 1)) & 6 == 0                     #   (64 input channels: neither gradient, so never the 7 that routes)
    assert bits((2, 136, 17, 17, 128, 3, 1, 1, 1)) == 0                        # C = 136: no whole 16-channel rows of an image
    assert bits((2, 128, 17, 17, 136, 3, 1, 1, 1)) == 0                        # K likewise (the image of dy)
    assert bits((2, 128, 17, 17, 128, 3, 1, 1, 1), window=(0, 256)) == 0       # a channel window of a wider weight
    assert bits((2, 128, 17, 17, 128, 3, 1, 1, 1), window=(128, 256)) == 0
    assert bits((2, 128, 3, 3, 128, 3, 1, 1, 1)) == 0                          # a 3 x 3 map: Ho * Wo < 16, no K step of the weight gradient inside an image
    assert bits((2, 128, 4, 4, 128, 3, 1, 1, 1)) == 7                          # 16 pixels: the smallest map (aligned shapes are admitted too)
    assert L.p3d_fx_conv_img_any_supported(None) == 0
    bad = _desc(pkg, (2, 128, 17, 17, 128, 3, 1, 1, 1))
    bad.Ho = 7
    assert L.p3d_fx_conv_img_any_supported(ctypes.byref(bad)) == 0
    before = pkg.ops.set_x3(False)                                             # P3D_X3=0 / set_x3(False) keeps everything on fp32-MFMA
    try:
        assert bits((2, 128, 17, 17, 128, 3, 1, 1, 1)) == 0
    finally:
        pkg.ops.set_x3(before)


@pytest.mark.parametrize('shape,bits', ADMITTED, ids=lambda v: '_'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_workspace_covers_forced_slabs(pkg, switch, shape, bits):
    L = pkg._lib.lib()
    n, c, h, w, k, r, stride, pad, dil = shape
    d = _desc(pkg, shape)
    b = ctypes.byref(d)
    ho, wo = d.Ho, d.Wo
    line = lambda elems: (elems + 3) // 4 * 4 * 4                  # a slab of the ragged forward / data gradient starts on a 16-B line
    for s in (2, 3):
        L.p3d_fx_tune(0, s)
        steps = -(-n * ho * wo // 16)
        per = -(-steps // min(s, steps))
        splits = -(-steps // per)                                  # the ragged plan: K steps over the flat pixel index, cut evenly
        assert splits >= 2
        if bits & 4:
            assert L.p3d_fx_conv_img_any_workspace_bytes(b, 2) >= splits * k * c * r * r * 4, s
        L.p3d_fx_tune(0, 0)
        L.p3d_fx_tune(1, s)
        if bits & 1:
            assert L.p3d_fx_conv_img_any_workspace_bytes(b, 0) >= s * line(n * k * ho * wo), s
        if bits & 2:
            assert L.p3d_fx_conv_img_any_workspace_bytes(b, 1) >= s * line(n * c * h * w), s
        L.p3d_fx_tune(1, 0)
    # its own plan always has room for the weight image the call builds when it is handed none
    image = r * r * ((k + 127) // 128) * 128 * c * 6
    assert L.p3d_fx_conv_img_any_workspace_bytes(b, 0) >= image
    assert L.p3d_fx_conv_img_any_workspace_bytes(None, 0) == 0


def test_activation_image_bytes(pkg):
    L = pkg._lib.lib()
    assert L.p3d_fx_act_image_bytes(64, 256, 256) == 3 * 64 * 256 * 256 * 2          # aligned HW: as ever
    assert L.p3d_fx_act_image_bytes(2, 32, 96) == 6 * 2 * 32 * 96
    for n, c, hw in ((3, 32, 17 * 19), (2, 16, 25), (1, 48, 9 * 18), (64, 2048, 17 * 17)):
        assert L.p3d_fx_act_image_bytes(n, c, hw) == 6 * n * c * hw, (n, c, hw)


def test_switch_defaults_off_and_round_trips(pkg):
    L = pkg._lib.lib()
    if os.environ.get('P3D_X3_ANY_IMAGES') != '1':
        before = pkg.ops.x3_any_images(True)
        try:
            assert before is False
            assert pkg.ops.x3_any_images(True) is True
            assert pkg.ops.x3_any_images_enabled() is True
        finally:
            assert pkg.ops.x3_any_images(False) is True
        assert pkg.ops.x3_any_images(False) is False
        assert pkg.ops.x3_any_images_enabled() is False
    # independent of its two siblings: neither moves it, it moves neither
    before = (pkg.ops.x3_any(False), pkg.ops.x3_any_partial(False), pkg.ops.x3_any_images(False))
    try:
        pkg.ops.x3_any(True)
        pkg.ops.x3_any_partial(True)
        assert L.p3d_x3_any_images_enable(1) == 0
        assert pkg.ops.x3_any(True) is True and pkg.ops.x3_any_partial(True) is True
        assert L.p3d_x3_any_images_enable(0) == 1
        assert pkg.ops.x3_any(False) is True and pkg.ops.x3_any_partial(False) is True
    finally:
        pkg.ops.x3_any(before[0])
        pkg.ops.x3_any_partial(before[1])
        pkg.ops.x3_any_images(before[2])


def test_switch_bumps_the_epoch(pkg):
    """ops_block.conv_takes_images caches its answer per shape and epoch"""
    e0 = pkg.ops.X3_EPOCH
    before = pkg.ops.x3_any_images(False)
    try:
        assert pkg.ops.X3_EPOCH > e0
    finally:
        pkg.ops.x3_any_images(before)
