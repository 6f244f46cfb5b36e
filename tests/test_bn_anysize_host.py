"""BatchNorm and the stem tail on 16-B kernels at any map width (ops.bn_any / p3d_bn_any_enable), the host side: the three new entries are declared, bound and
exported; the switch defaults off, returns the previous state and is independent of the other switches; p3d_stem_tail_any_supported against the rule written
out here; p3d_stem_tail_supported answers the same whatever the switch says.  No GPU needed."""
import ctypes
import os

import pytest
import torch

NEW = ('p3d_bn_any_enable', 'p3d_stem_tail_any_supported', 'p3d_bn_last_launch')
SIDES = list(range(1, 11)) + [129]


@pytest.fixture
def switch(pkg):
    before = pkg.ops.bn_any(False)
    yield pkg.ops.bn_any
    pkg.ops.bn_any(before)


def test_entries_are_declared_and_bound(pkg):
    import test_abi
    declared = test_abi.declared_functions(pkg._lib.HEADER_PATH)
    handle = ctypes.CDLL(pkg._lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in pkg._lib.SIGNATURES and hasattr(handle, name), name
    assert 'P3D_BN_ANY' in (pkg.ops.bn_any.__doc__ or '')


def test_switch_defaults_off_and_returns_the_previous_state(pkg):
    ops = pkg.ops
    if os.environ.get('P3D_BN_ANY') == '1':          # (the default cannot be read then)
        return
    names = ('x3_any', 'x3_any_partial', 'x3_any_images', 'x3_any_strided', 'frozen_fold')
    others = [getattr(ops, n)(True) for n in names]                # none of the other switches turns this one on
    try:
        before = ops.bn_any(True)
        try:
            assert before is False
            assert ops.bn_any(True) is True
            assert [getattr(ops, n)(True) for n in names] == [True] * len(names)       # ... nor does this one touch them
            assert [getattr(ops, n)(False) for n in names] == [True] * len(names)
            assert ops.bn_any(True) is True                                            # ... nor do they touch it on the way down
        finally:
            assert ops.bn_any(False) is True
        assert ops.bn_any(False) is False
        assert [getattr(ops, n)(False) for n in names] == [False] * len(names)
    finally:
        for n, v in zip(names, others):
            getattr(ops, n)(v)


@pytest.mark.parametrize('on', [False, True])
def test_stem_tail_queries(pkg, switch, on):
    L = pkg._lib.lib()
    switch(False)
    off = {(n, c, h, w): L.p3d_stem_tail_supported(n, c, h, w) for n in (0, 2) for c in (0, 3) for h in SIDES for w in SIDES}
    switch(on)                                                      # both queries answer whatever the switch says
    for (n, c, h, w), was in off.items():
        assert L.p3d_stem_tail_any_supported(n, c, h, w) == int(n > 0 and c > 0 and h >= 2 and w >= 2), (n, c, h, w)
        assert L.p3d_stem_tail_supported(n, c, h, w) == was == int(n > 0 and c > 0 and h >= 2 and w >= 4 and h % 2 == 0 and w % 4 == 0), (n, c, h, w)
    assert L.p3d_stem_tail_any_supported(-1, 3, 9, 9) == 0 and L.p3d_stem_tail_any_supported(2, -3, 9, 9) == 0


@pytest.mark.parametrize('on', [False, True])
def test_stem_tail_is_not_usable_on_the_cpu(pkg, switch, on):
    switch(on)
    bn = pkg.nn.BatchNorm2d(3).train()
    pool = pkg.nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
    for side in (8, 9):
        assert pkg.ops.stem_tail_usable(torch.zeros(2, 3, side, side), bn, pool) is False


def test_last_launch_record_is_four_numbers(pkg):
    rec = pkg.ops.bn_last_launch()
    assert set(rec) == {'entry', 'instance', 'grid'} and 0 <= rec['entry'] <= 6 and rec['instance'] in (0, 1, 2) and len(rec['grid']) == 2
