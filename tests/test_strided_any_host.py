"""Stride-2 data gradients on the x3 kernels at any map side (ops.x3_any_strided / p3d_x3_any_strided_enable), the host side: the switch's default and return
values, p3d_conv2d_dgrad_strided_any_supported against the rule written out here, and p3d_conv2d_dgrad_workspace_bytes with the switch off (the answers recorded in
tests/golden/conv_queries.json) and on (at least the weight image plus the four class planes, for admitted shapes only).  No GPU needed."""
import ctypes
import json

import pytest

from conftest import golden_path

NEW = ('p3d_x3_any_strided_enable', 'p3d_conv2d_dgrad_strided_any_supported', 'p3d_dgrad_interleave')


def rule(c, k, r, stride, pad, dil):
    """fx_applies(FX_DGRAD) for stride 2 without its H % 2, W % 8 and width clauses, at the per-layer threshold"""
    return int(stride == 2 and r % 2 == 1 and k % 16 == 0 and k >= 32 and c % 4 == 0 and c >= 96 and pad == dil * (r - 1) // 2 and (r == 1 or dil == 1))


def up(v, to):
    return (v + to - 1) // to * to


def planes_figure(n, c, h, w, k, r):
    """the data-gradient weight image (three bf16 pieces per weight, rows padded to the 128-row tile) plus four class planes, each part on a 256-B line"""
    cls_stride = up(n * c * ((h + 1) // 2) * ((w + 1) // 2), 4)
    return up(r * r * up(c, 128) * k * 6, 256) + up(4 * cls_stride * 4, 256)


@pytest.fixture
def switch(pkg):
    before = pkg.ops.x3_any_strided(False)
    yield pkg.ops.x3_any_strided
    pkg.ops.x3_any_strided(before)


def test_entries_are_declared_and_bound(pkg):
    import test_abi
    declared = test_abi.declared_functions(pkg._lib.HEADER_PATH)
    handle = ctypes.CDLL(pkg._lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in pkg._lib.SIGNATURES and hasattr(handle, name), name
    assert 'P3D_X3_ANY_STRIDED' in (pkg.ops.x3_any_strided.__doc__ or '')
    header = open(pkg._lib.HEADER_PATH).read()
    assert 'TEST HOOK (tests/test_strided_any_gpu.py' in header and '5 dgrad_interleave_rows_kernel' in header


def test_switch_defaults_off_and_returns_the_previous_state(pkg):
    import os
    ops = pkg.ops
    if os.environ.get('P3D_X3_ANY_STRIDED') != '1':
        others = (ops.x3_any(True), ops.x3_any_partial(True), ops.x3_any_images(True))         # none of the other three turns this one on
        try:
            before = ops.x3_any_strided(True)
            try:
                assert before is False
                assert ops.x3_any_strided(True) is True
                assert (ops.x3_any(True), ops.x3_any_partial(True), ops.x3_any_images(True)) == (True, True, True)      # ... nor does this one touch them
            finally:
                assert ops.x3_any_strided(False) is True
            assert ops.x3_any_strided(False) is False
        finally:
            ops.x3_any(others[0]), ops.x3_any_partial(others[1]), ops.x3_any_images(others[2])
    assert pkg._lib.lib().p3d_conv2d_dgrad_strided_any_supported(None) == 0


# n, c, h, w, k, r, stride, pad, dil
ADMITTED = [(n, c, h, h, k, r, 2, r // 2, 1) for n in (2, 64) for c, k, h, r in ((256, 512, 65, 1), (512, 1024, 33, 1), (128, 128, 65, 3), (256, 256, 33, 3))] + \
           [(2, 512, 17, 17, 512, 3, 2, 1, 1), (2, 1024, 17, 17, 2048, 1, 2, 0, 1),          # -stride 32: layer4.0 at 17 -> 9
            (2, 128, 33, 33, 256, 3, 2, 1, 1), (2, 128, 33, 33, 256, 1, 2, 0, 1),            # ResNet-18's layer3.0 at 33 -> 17
            (2, 128, 16, 16, 128, 3, 2, 1, 1), (2, 128, 16, 16, 128, 1, 2, 0, 1),            # aligned shapes are admitted too (the entry keeps them on the aligned instances)
            (2, 96, 9, 11, 32, 3, 2, 1, 1), (2, 224, 9, 9, 64, 1, 2, 0, 1), (2, 128, 17, 17, 128, 5, 2, 2, 1), (2, 128, 17, 17, 128, 1, 2, 0, 2)]
REFUSED = [(2, 64, 65, 65, 128, 3, 2, 1, 1),            # C = 64: under the per-layer threshold
           (2, 92, 17, 17, 128, 3, 2, 1, 1), (2, 98, 17, 17, 128, 1, 2, 0, 1),               # C < 96; C % 4
           (2, 128, 17, 17, 24, 3, 2, 1, 1), (2, 128, 17, 17, 16, 1, 2, 0, 1), (2, 128, 17, 17, 40, 1, 2, 0, 1),      # K = 24; K < 32; K % 16
           (2, 128, 17, 17, 128, 3, 1, 1, 1), (2, 128, 16, 16, 128, 1, 1, 0, 1),             # stride 1
           (2, 128, 24, 16, 128, 3, 2, 2, 2),           # 3x3 with dilation 2
           (2, 128, 17, 17, 128, 3, 2, 0, 1), (2, 128, 17, 17, 128, 1, 2, 1, 1),             # pad != dil (R - 1) / 2
           (2, 128, 18, 18, 128, 2, 2, 0, 1),           # an even filter
           (2, 128, 19, 19, 128, 3, 3, 1, 1)]           # stride 3


def _desc(pkg, row, accumulate=0):
    n, c, h, w, k, r, stride, pad, dil = row
    return pkg.ops._desc((n, c, h, w), (k, c, r, r), stride, pad, dil, 0, c, accumulate)


@pytest.mark.parametrize('on', [False, True])
def test_verdict_table(pkg, switch, on):
    L = pkg._lib.lib()
    switch(on)                                                  # the predicate answers whatever the switch says
    for row in ADMITTED + REFUSED:
        n, c, h, w, k, r, stride, pad, dil = row
        for accumulate in (0, 1):
            got = L.p3d_conv2d_dgrad_strided_any_supported(ctypes.byref(_desc(pkg, row, accumulate)))
            assert got == rule(c, k, r, stride, pad, dil) == int(row in ADMITTED), (row, accumulate, got)
    for off, tot in ((0, 256), (128, 256)):                     # a channel window of a wider weight
        d = pkg.ops._desc((2, 128, 17, 17), (128, tot, 3, 3), 2, 1, 1, off, tot)
        assert L.p3d_conv2d_dgrad_strided_any_supported(ctypes.byref(d)) == 0
    bad = _desc(pkg, ADMITTED[0])
    bad.Ho = 7
    assert L.p3d_conv2d_dgrad_strided_any_supported(ctypes.byref(bad)) == 0
    before = pkg.ops.set_x3(False)                              # P3D_X3=0 / set_x3(False) keeps everything on fp32-MFMA
    try:
        assert L.p3d_conv2d_dgrad_strided_any_supported(ctypes.byref(_desc(pkg, ADMITTED[0]))) == 0
    finally:
        pkg.ops.set_x3(before)


def test_workspace_query(pkg, switch):
    """off: the recorded answers of today for the rows the golden table shares with this one; on: at least the planes figure where the predicate admits, and the
    off answer everywhere else"""
    L = pkg._lib.lib()
    with open(golden_path('conv_queries.json')) as f:
        golden = json.load(f)
    col = golden['queries'].index('conv2d_dgrad_workspace_bytes')
    assert tuple(golden['configs'][0]) == (1, 0, 0)
    recorded = {tuple(r[0]): r[1][0][col] for r in golden['rows']}
    shared = grew = 0
    for row in ADMITTED + REFUSED:
        n, c, h, w, k, r, stride, pad, dil = row
        for accumulate in (0, 1):
            b = ctypes.byref(_desc(pkg, row, accumulate))
            switch(False)
            off = L.p3d_conv2d_dgrad_workspace_bytes(b)
            key = (n, c, h, w, k, r, stride, pad, dil, 0, c, accumulate)
            if key in recorded:
                assert off == recorded[key], (row, off, recorded[key])
                shared += 1
            switch(True)
            on = L.p3d_conv2d_dgrad_workspace_bytes(b)
            switch(False)
            assert L.p3d_conv2d_dgrad_workspace_bytes(b) == off
            if row in ADMITTED:
                assert on == max(off, planes_figure(n, c, h, w, k, r)), (row, off, on)
                grew += on > off
            else:
                assert on == off, (row, off, on)
    assert shared >= 8 and grew >= 8, (shared, grew)
