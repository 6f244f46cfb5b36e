"""The geometry table (tests/geometry_table.py) against the host-only *_supported queries of the library: every row's admitted / refused verdict, per
family and pass.  tests/test_geometry_gpu.py relies on these verdicts to know which kernel a row must run on; if a predicate is narrowed later, this
file fails instead of the GPU tests quietly testing a fallback.  No GPU needed.

Also here, on the CPU: the references of the table can tell a kernel that exchanges H and W from a correct one -- for each family the float64
reference of a row and the reference of the same memory read as [W][H] differ by at least 100 x the tolerance the GPU comparison uses."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import geometry_table as T
from oracle import np_ops as ref


def _desc(pkg, g):
    return pkg.ops._desc((g.n, g.c, g.h, g.w), (g.k, g.c, g.r, g.r), g.stride, g.pad, g.dil)


def test_table_covers_what_it_promises():
    names = [g.name for g in T.ROWS]
    assert len(set(names)) == len(names)
    for h, w in T.ASPECTS + T.SMALL:
        assert (w, h) in T.ASPECTS + T.SMALL                                      # both orders, always
    for hw in T.ASPECTS:
        got = {(g.r, g.stride, g.dil) for g in T.ROWS if (g.h, g.w) == hw and g.pad == g.dil * (g.r - 1) // 2 and g.x3 == 7}
        assert got >= {(1, 1, 1), (1, 2, 1), (3, 1, 1), (3, 2, 1), (3, 1, 2), (5, 1, 1)}, hw
    assert {g.n for g in T.ADMITTED} >= {1, 3, 8}
    assert {g.k for g in T.ADMITTED} >= {64, 128, 272} and any(g.c >= 1024 for g in T.ADMITTED)
    assert any(g.n * int(np.prod(T.out_hw(g))) % 128 for g in T.ADMITTED)               # a last pixel tile that is cut short (1 * 12 * 20 = 240), mid-image
    assert any(128 % T.out_hw(g)[1] for g in T.ADMITTED)                                 # a tile boundary inside a row
    uneven = [g for g in T.ROWS if g.pad != g.dil * (g.r - 1) // 2 and g.x3]
    assert {(g.h, g.w) for g in uneven} == {(24, 40), (40, 24)} and len(uneven) == 14
    assert sum(g.x3 == 5 for g in T.ROWS) == 4 and sum(g.x3 == 0 for g in T.ROWS) == 5


@pytest.mark.parametrize('g', T.ROWS, ids=T.IDS)
def test_row_verdicts(pkg, g):
    L = pkg._lib.lib()
    d = _desc(pkg, g)
    b = ctypes.byref(d)
    ho, wo = T.out_hw(g)
    assert (d.Ho, d.Wo) == (ho, wo) and ho > 0 and wo > 0
    assert L.p3d_fx_conv_img_supported(b) == g.x3                                 # x3 kernels: 1 forward | 2 data gradient | 4 weight gradient
    fwd = g.x3 & 1
    assert L.p3d_fx_conv_fwd_infer_supported(b, 0) == fwd and L.p3d_fx_conv_fwd_infer_supported(b, 1) == fwd
    assert L.p3d_fx_conv_fwd_infer_masked_supported(b) == fwd
    assert L.p3d_hconv2d_fwd_infer_supported(b) == 1                              # the gather kernels take every row, the refused rectangles included
    assert L.p3d_f8conv2d_fwd_infer_supported(b) == 1
    if g.x3 == 5:                                                                 # refused for the padding alone: the same map with "same" padding passes
        same = pkg.ops._desc((g.n, g.c, g.h, g.w), (g.k, g.c, g.r, g.r), g.stride, g.dil * (g.r - 1) // 2, g.dil)
        assert L.p3d_fx_conv_img_supported(ctypes.byref(same)) == 7


def _block(pkg, kind, inplanes, planes, stride, dil, with_ds, partial=False):
    tr = pkg._trunk
    cls = tr.Bottleneck if kind == 'bottleneck' else tr.BasicBlock
    ds = None
    if with_ds:
        ds = tr.Sequential(pkg.nn.Conv2d(inplanes, planes * cls.expansion, kernel_size=1, stride=stride, bias=False), pkg.nn.BatchNorm2d(planes * cls.expansion))
    return cls(inplanes, planes, stride, dil, ds, partial=True) if partial else cls(inplanes, planes, stride, dil, ds)


@pytest.mark.parametrize('blk', T.BLOCKS, ids=lambda b: '%s_c%d_p%d_s%d_d%d' % b[:5])
def test_block_verdicts(pkg, blk):
    kind, inplanes, planes, stride, dil, with_ds = blk
    block = _block(pkg, kind, inplanes, planes, stride, dil, with_ds)
    for h, w in T.BLOCK_MAPS:
        for n in (1, 3):
            plan = pkg.ops_block._Plan(block, (n, inplanes, h, w))
            assert plan.ok == T.block_admitted(stride, h, w), (h, w, n)
    masked = _block(pkg, kind, inplanes, planes, stride, dil, with_ds, partial=True)
    for h, w in T.ASPECTS:
        assert pkg.ops_block._Plan(masked, (3, inplanes, h, w), masked=True).ok, (h, w)


def test_stem_verdicts(pkg):
    L = pkg._lib.lib()
    for h, w in T.STEM_MAPS:
        assert L.p3d_stem_supported(2, 3, h, w, 64) == 1 and L.p3d_stem_masked_supported(2, 1, h, w, 64) == 1, (h, w)
        assert (h // 2) % 2 == 0 and (w // 2) % 4 == 0                            # what infer._stem asks besides
    assert set(T.NET_MAPS) <= set(T.STEM_MAPS)


# ---- a transposition is visible to every family's comparison ----------------------------------------------------------------------------
# the loosest bound each family's GPU comparison uses, relative to max |reference| (tests/test_geometry_gpu.py)
FAMILY_TOL = {'x3 fp32-fed': 4e-6, 'image-fed': 5e-5, 'folded fp32': 2e-5, 'folded fp16': 2e-3, 'fp16 per-layer': 2e-3}


def _flat(g):
    return g.r == 1 and g.stride == 1 and g.pad == 0


def test_a_flat_pointwise_conv_has_no_geometry():
    """1x1, stride 1, no padding: a product per pixel of a flat list, the same under any reading of (H, W) -- such rows test tiles and tails, the others geometry"""
    flat = [g for g in T.ROWS if _flat(g)]
    assert flat and all(T.transposition_gap(g) == 0.0 for g in flat[:2])
    assert len(flat) <= len(T.ROWS) // 6


@pytest.mark.parametrize('g', [g for g in T.ROWS if g.c <= 256 and not _flat(g)], ids=lambda g: g.name)
def test_transposed_read_is_far_from_the_reference(g):
    gap = T.transposition_gap(g)
    for family, tol in FAMILY_TOL.items():
        assert gap >= 100 * tol, (family, gap)


def test_transposed_block_is_far_from_the_reference():
    """conv - BatchNorm (batch statistics) - ReLU - conv - BatchNorm + shortcut - ReLU in float64, on x and on its [W][H] reading: 100 x the 8e-5 of the
    block family's element-wise bound (and of the whole networks' 1e-4)"""
    gen = torch.Generator().manual_seed(1)
    for h, w in T.ASPECTS:
        x = torch.randn(3, 32, h, w, generator=gen, dtype=torch.float64).relu()
        w1, w2 = (torch.randn(32, 32, 3, 3, generator=gen, dtype=torch.float64) / 17 for _ in range(2))

        def block(v):
            a = F.batch_norm(F.conv2d(v, w1, None, 1, 1), None, None, None, None, True).relu()
            return (F.batch_norm(F.conv2d(a, w2, None, 1, 1), None, None, None, None, True) + v).relu()

        y, yt = block(x), block(T.transposed_read(x)).reshape(x.shape)
        assert float((y - yt).abs().max() / y.abs().max()) >= 100 * 1e-4, (h, w)


def test_transposed_read_is_far_beyond_the_fp8_bound():
    """the MXFP8 family's bound is per element (test_infer_fp8_gpu._expect): the transposed reading misses it by more than 100 x somewhere"""
    from test_infer_fp8_gpu import _emul_image, _expect
    gen = torch.Generator().manual_seed(2)
    for h, w in T.ASPECTS:
        x16 = torch.randn(2, 64, h, w, generator=gen).half()
        q, sc = _emul_image(torch.randn(64, 64, 3, 3, generator=gen) / 24)
        bias = torch.zeros(64)
        want, tol = _expect(x16, q, sc, bias, 1, 1, 1)
        other, _ = _expect(T.transposed_read(x16), q, sc, bias, 1, 1, 1)
        assert float(((want - other.reshape(want.shape)).abs() / tol).max()) >= 100, (h, w)


def test_transposed_heat_map_is_far_from_the_reference():
    """softargmax3d at H != W: the expectation of a heat map read as [W][H] lands 100 x 2e-6 away (the forward bound of test_head_matches_reference_golden)"""
    rng = np.random.default_rng(0)
    for h, w in ((12, 20), (20, 12)):
        z = (rng.standard_normal((2, 16 * 17, h, w)) * 3).astype(np.float32)
        c = ref.softargmax3d_fwd(z, 16, 17, h, w, 1000.0)
        ct = ref.softargmax3d_fwd(z.reshape(2, 16 * 17, w, h), 16, 17, w, h, 1000.0)
        assert np.abs(c - ct).max() / np.abs(c).max() >= 100 * 2e-6
