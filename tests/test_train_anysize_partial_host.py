"""Training partial convolutions on the x3 kernels at any map width (ops.x3_any_partial / p3d_x3_any_partial_enable), the host side: the three
p3d_conv2d_*_masked_any_supported queries against the rules written out here, the switch's return values and default, and the three per-layer workspace queries
with the switch on (they cover the masked ragged plans) and off (what they answer when it was never touched).  No GPU needed."""
import ctypes

import pytest

NEW = ('p3d_x3_any_partial_enable', 'p3d_conv2d_fwd_masked_any_supported', 'p3d_conv2d_dgrad_masked_any_supported', 'p3d_conv2d_wgrad_masked_any_supported')


def rules(c, k, r, stride):
    """what the masked ragged instances admit: (forward, data gradient, weight gradient) -- the x3 rule of each pass at the masked thresholds 64 / 64 / 96"""
    fwd = c % 16 == 0 and c >= 32 and k >= 64
    dgrad = k % 16 == 0 and k >= 32 and c % 4 == 0 and c >= 64 and stride == 1
    wgrad = k >= 96 and c >= 96 and (r == 1 or c % 64 == 0)
    return int(fwd), int(dgrad), int(wgrad)


def verdicts(L, d):
    b = ctypes.byref(d)
    return L.p3d_conv2d_fwd_masked_any_supported(b), L.p3d_conv2d_dgrad_masked_any_supported(b), L.p3d_conv2d_wgrad_masked_any_supported(b)


@pytest.fixture
def switch(pkg):
    """sets the switch for the test body and restores what it found, with the forced split counts"""
    before = pkg.ops.x3_any_partial(False)
    yield pkg.ops.x3_any_partial
    pkg.ops.x3_any_partial(before)
    pkg._lib.lib().p3d_fx_tune(0, 0)
    pkg._lib.lib().p3d_fx_tune(1, 0)


def test_entries_are_declared_and_bound(pkg):
    import test_abi
    declared = test_abi.declared_functions(pkg._lib.HEADER_PATH)
    handle = ctypes.CDLL(pkg._lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in pkg._lib.SIGNATURES and hasattr(handle, name), name
    assert sorted(pkg._lib.SIGNATURES) == declared
    assert 'P3D_X3_ANY_PARTIAL' in (pkg.ops.x3_any_partial.__doc__ or '')


def test_switch_defaults_off_and_returns_the_previous_state(pkg):
    import os
    if os.environ.get('P3D_X3_ANY_PARTIAL') != '1':
        dense = pkg.ops.x3_any(True)                          # the dense switch does not turn this one on
        try:
            before = pkg.ops.x3_any_partial(True)
            try:
                assert before is False
                assert pkg.ops.x3_any_partial(True) is True
                assert pkg.ops.x3_any(True) is True           # ... nor does this one touch the dense switch
            finally:
                assert pkg.ops.x3_any_partial(False) is True
            assert pkg.ops.x3_any_partial(False) is False
        finally:
            pkg.ops.x3_any(dense)
    L = pkg._lib.lib()
    assert L.p3d_conv2d_fwd_masked_any_supported(None) == 0 and L.p3d_conv2d_dgrad_masked_any_supported(None) == 0 and L.p3d_conv2d_wgrad_masked_any_supported(None) == 0


# c, k, h, w, r, stride, pad, dil
TABLE = [(c, k, 17, 19, r, 1, r // 2, 1) for r in (1, 3) for c in (16, 32, 48, 64, 80, 96, 112, 128) for k in (32, 48, 63, 64, 80, 95, 96, 128)] + \
        [(c, 128, 17, 17, r, 1, r // 2, 1) for r in (1, 3) for c in (60, 68, 100, 120, 160, 192)] + \
        [(128, 128, 17, 17, 3, 2, 1, 1), (128, 128, 19, 19, 1, 2, 0, 1), (64, 128, 65, 65, 3, 2, 1, 1), (128, 128, 17, 19, 3, 1, 2, 2), (128, 128, 17, 19, 5, 1, 2, 1),
         (128, 128, 16, 16, 3, 1, 1, 1), (64, 64, 32, 32, 3, 1, 1, 1), (256, 128, 16, 24, 1, 1, 0, 1), (128, 128, 16, 16, 3, 2, 1, 1)]      # aligned shapes are admitted too


@pytest.mark.parametrize('on', [False, True])
def test_verdict_table(pkg, switch, on):
    L = pkg._lib.lib()
    switch(on)                                                # the queries do not look at the switch
    seen = set()
    for c, k, h, w, r, stride, pad, dil in TABLE:
        d = pkg.ops._desc((3, c, h, w), (k, c, r, r), stride, pad, dil)
        got = verdicts(L, d)
        assert got == rules(c, k, r, stride), (c, k, h, w, r, stride)
        seen.add(got)
    assert {(1, 1, 1), (1, 1, 0), (1, 0, 1), (0, 1, 0), (0, 0, 0), (1, 0, 0)} <= seen


def test_refusals(pkg):
    L = pkg._lib.lib()

    def v(c, k, h, w, r, stride, pad, dil, window=None):
        d = pkg.ops._desc((3, c, h, w), (k, c if window is None else window[1], r, r), stride, pad, dil)
        if window is not None:
            d.c_offset, d.c_total = window
        return verdicts(L, d)

    assert v(128, 128, 17, 17, 3, 1, 1, 1) == (1, 1, 1)
    assert v(128, 128, 16, 16, 3, 1, 1, 1) == (1, 1, 1)                        # aligned shapes
    assert v(64, 64, 17, 17, 3, 1, 1, 1) == (1, 1, 0)                          # the masked thresholds: 64 / 64 / 96
    assert v(32, 64, 17, 17, 3, 1, 1, 1) == (1, 0, 0)
    assert v(64, 63, 17, 17, 1, 1, 0, 1) == (0, 0, 0)
    assert v(96, 96, 17, 17, 1, 1, 0, 1) == (1, 1, 1)
    assert v(95, 96, 17, 17, 1, 1, 0, 1) == (0, 0, 0)                          # C % 16 (forward), C % 4 (data gradient), C < 96 (weight gradient)
    assert v(128, 128, 17, 17, 3, 2, 1, 1) == (1, 0, 1)                        # stride 2: no ragged data gradient
    assert v(128, 128, 19, 19, 1, 2, 0, 1) == (1, 0, 1)
    assert v(120, 128, 17, 17, 1, 1, 0, 1) == (0, 1, 1)                        # C % 16 != 0: the forward's reduction runs in steps of 16 channels
    assert v(120, 128, 17, 17, 3, 1, 1, 1) == (0, 1, 0)                        #   and a multi-tap weight gradient wants C % 64 == 0
    assert v(160, 128, 17, 17, 3, 1, 1, 1) == (1, 1, 0)
    assert v(128, 120, 17, 17, 1, 1, 0, 1) == (1, 0, 1)                        # K % 16 != 0: the data gradient's reduction
    assert v(128, 128, 17, 17, 1, 1, 0, 1, window=(0, 256)) == (0, 0, 0)       # a channel window of a wider weight
    assert v(128, 128, 17, 17, 1, 1, 0, 1, window=(128, 256)) == (0, 0, 0)
    assert v(128, 128, 18, 18, 2, 1, 0, 1) == (0, 0, 0)                        # an even filter
    assert v(128, 128, 18, 18, 4, 1, 1, 1) == (0, 0, 0)
    bad = pkg.ops._desc((3, 128, 17, 17), (128, 128, 3, 3), 1, 1, 1)
    bad.Ho = 7
    assert verdicts(L, bad) == (0, 0, 0)
    before = pkg.ops.set_x3(False)                                             # P3D_X3=0 / set_x3(False) keeps everything on fp32-MFMA
    try:
        assert v(128, 128, 17, 17, 3, 1, 1, 1) == (0, 0, 0)
    finally:
        pkg.ops.set_x3(before)


def _workspace(pkg, d):
    L, b = pkg._lib.lib(), ctypes.byref(d)
    return L.p3d_conv2d_fwd_workspace_bytes(b), L.p3d_conv2d_dgrad_workspace_bytes(b), L.p3d_conv2d_wgrad_workspace_bytes(b)


SHAPES = [((3, 128, 17, 19), (128, 128, 3, 3), 1, 1, 1), ((2, 512, 17, 19), (512, 512, 3, 3), 1, 1, 1), ((2, 64, 33, 33), (64, 64, 3, 3), 1, 1, 1),
          ((2, 128, 65, 65), (128, 128, 3, 3), 2, 1, 1), ((2, 128, 16, 16), (128, 128, 3, 3), 1, 1, 1), ((64, 256, 65, 65), (128, 256, 1, 1), 1, 0, 1)]


def test_workspace_covers_the_masked_ragged_plans(pkg, switch):
    """with the switch on each query is at least the masked ragged plan's bytes -- the pre-split weight image and, under a forced split, the slabs, each starting on a
    16-B line; the weight gradient's slabs -- for the shapes of the GPU file's forced-slab tests"""
    L = pkg._lib.lib()
    switch(True)
    for (n, c, h, w), k, slabs_conv, slabs_wgrad in (((3, 128, 17, 19), 128, 0, 2), ((3, 128, 17, 19), 128, 0, 3), ((2, 512, 17, 19), 512, 2, 0), ((2, 512, 17, 19), 512, 3, 0)):
        d = pkg.ops._desc((n, c, h, w), (k, c, 3, 3), 1, 1, 1)
        L.p3d_fx_tune(1, slabs_conv)
        L.p3d_fx_tune(0, slabs_wgrad)
        fwd, dgrad, wgrad = _workspace(pkg, d)
        image = 9 * ((k + 127) // 128 * 128) * c * 6                           # three bf16 pieces per weight, rows padded to the 128-row tile
        slab = (n * k * h * w + 3) // 4 * 4 * 4
        assert fwd >= image + slabs_conv * slab and dgrad >= image + slabs_conv * slab, (n, c, slabs_conv)
        assert wgrad >= max(slabs_wgrad, 1) * k * c * 9 * 4, (n, c, slabs_wgrad)


def test_workspace_with_the_switch_off_is_what_it_was(pkg, switch):
    """off after having been on answers what a library whose switch was never touched answers: a fresh process gives the same numbers"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ('import ctypes, importlib, json, sys\n'
            'sys.path.insert(0, %r)\n'
            'pkg = importlib.import_module(%r)\n'
            'L = pkg._lib.lib()\n'
            'out = []\n'
            'for xs, ws, s, p, dl in %r:\n'
            '    b = ctypes.byref(pkg.ops._desc(xs, ws, s, p, dl))\n'
            '    out.append([L.p3d_conv2d_fwd_workspace_bytes(b), L.p3d_conv2d_dgrad_workspace_bytes(b), L.p3d_conv2d_wgrad_workspace_bytes(b)])\n'
            'print(json.dumps(out))\n') % (root, pkg.__name__, SHAPES)
    env = {k: v for k, v in os.environ.items() if k not in ('P3D_X3_ANY_PARTIAL',)}
    fresh = json.loads(subprocess.run([sys.executable, '-c', code], check=True, capture_output=True, text=True, env=env).stdout.strip().splitlines()[-1])
    grew = 0
    for (xs, ws, s, p, dl), untouched in zip(SHAPES, fresh):
        d = pkg.ops._desc(xs, ws, s, p, dl)
        switch(False)
        off = _workspace(pkg, d)
        switch(True)
        on = _workspace(pkg, d)
        switch(False)
        assert off == tuple(untouched) == _workspace(pkg, d), (xs, ws)
        assert all(b >= a for a, b in zip(off, on)), (xs, ws, off, on)
        if xs[2] % 4 == 0:
            assert on == off, (xs, ws)                        # aligned shapes: the masked plan was covered already
        grew += on != off
    assert grew > 0
