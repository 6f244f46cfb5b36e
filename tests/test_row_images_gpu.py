"""Row images: activation / gradient images that hold the fp32 value itself ([N][C/16][HW][16] floats) instead of three pre-split bf16 planes, and the row-fed
instances of the x3 convolution kernels that cut a value into its pieces between their fetch registers and LDS.

hi + mid + lo == x exactly and the pieces come from the same function applied to the same value, so NOTHING may differ: every comparison here is torch.equal --
the row image against the exact sum of the three planes, every row-fed launch against the plane-fed launch on the same operands, and whole residual blocks run
through the executor once per format (p3d_fx_tune(6, .)).  All outputs and images lie in exact-size, poisoned, fenced buffers (tests/fenced.py).

The pair pass and the mask bytes of a block's closing ReLU run through p3d_fx_open_images (the opening passes of the backward, alone) at the same two shapes, and
again inside the executor's downsample blocks, whose d c_last / d c_ds images are compared too."""
import ctypes
import os

import pytest
import torch

from fenced import FencedAllocations

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(os.environ.get('P3D_X3', '1') == '0', reason='row images feed the x3 kernels')]


def unblock_rows(img, shape):
    n, c, h, w = shape
    return img.view(torch.float32).view(n, c // 16, h * w, 16).permute(0, 1, 3, 2).reshape(n, c, h, w)


def plane_sum(img, shape):
    """hi + mid + lo of a three-plane image, exact (float64), as an NCHW tensor"""
    n, c, h, w = shape
    p = img.view(torch.bfloat16).view(3, n, c // 16, h * w, 16).double().sum(0)
    return p.permute(0, 1, 3, 2).reshape(n, c, h, w)


def table_for(c, gen):
    t = torch.randn(c, 8, device='cuda', generator=gen)
    t[:, 0] = t[:, 0].abs() + 0.5
    return t.contiguous()


@pytest.mark.parametrize('shape', [(3, 48, 12, 12), (2, 64, 16, 16)], ids=['n3_c48_12x12', 'n2_c64_16x16'])
@pytest.mark.parametrize('mode,masked', [(0, 0), (1, 0), (2, 0), (2, 1)], ids=['mode0', 'mode1', 'mode2', 'mode2_masked'])
def test_row_image_is_the_sum_of_the_planes(pkg, shape, mode, masked):
    ops = pkg.ops
    gen = torch.Generator(device='cuda').manual_seed(11 + mode)
    x = torch.randn(shape, device='cuda', generator=gen)
    x2 = torch.randn(shape, device='cuda', generator=gen) if mode == 2 else None
    tab = table_for(shape[1], gen) if mode else None
    with FencedAllocations() as fa:
        planes = ops.act_image(x, mode, x2, tab, masked)
        rows = ops.row_image(x, mode, x2, tab, masked)
        torch.cuda.synchronize()
    fa.check()
    assert rows.numel() == 4 * x.numel() and planes.numel() == 6 * x.numel()
    got = unblock_rows(rows, shape)
    assert torch.isfinite(got).all()
    assert torch.equal(got.double(), plane_sum(planes, shape))
    if mode == 0:
        assert torch.equal(got, x)


@pytest.mark.parametrize('shape', [(3, 48, 12, 12), (2, 64, 16, 16)], ids=['n3_c48_12x12', 'n2_c64_16x16'])
@pytest.mark.parametrize('pair', [False, True], ids=['mode2_mask_bytes', 'pair_pass_mask_bytes'])
def test_opening_passes_with_mask_bytes(pkg, shape, pair):
    """Mode 2 with the closing ReLU's mask bytes, and the pair pass (two gradient images from one read of dout and the mask bytes): constants finalized in the
    prologue from fp64 partial sums, three channel groups and a partly filled last block at 48 channels.  Row images against the exact sum of the planes;
    d gamma and d beta equal."""
    ops = pkg.ops
    n, c, h, w = shape
    gen = torch.Generator(device='cuda').manual_seed(31 + c)
    g = torch.randn(shape, device='cuda', generator=gen)
    gmask = torch.randint(0, 16, (n * c * h * w // 4,), device='cuda', generator=gen, dtype=torch.uint8)
    partial = torch.randn(c, 5, 3, device='cuda', generator=gen, dtype=torch.float64)
    sides = []
    for _ in range(2 if pair else 1):
        tab = table_for(c, gen)
        tab[:, 3] = tab[:, 3].abs() + 0.5                      # invstd
        sides.append((torch.randn(shape, device='cuda', generator=gen), tab, torch.rand(c, device='cuda', generator=gen) + 0.5))
    with FencedAllocations() as fa:
        planes = ops.open_images(g, gmask, partial, n * h * w, sides, rows=False)
        rows = ops.open_images(g, gmask, partial, n * h * w, sides, rows=True)
        torch.cuda.synchronize()
    fa.check()
    keep = torch.stack([(gmask >> e) & 1 for e in range(4)], 1).reshape(shape).bool()
    # the mask bytes are honoured: where a bit is clear the value is B c + K, whatever g holds there
    again = ops.open_images(torch.where(keep, g, torch.full_like(g, 7.0)), gmask, partial, n * h * w, sides, rows=True)
    for i, ((pi, pdg, pdb), (ri, rdg, rdb)) in enumerate(zip(planes, rows)):
        assert ri.numel() == 4 * g.numel() and pi.numel() == 6 * g.numel()
        got = unblock_rows(ri, shape)
        assert torch.isfinite(got).all()
        assert torch.equal(got.double(), plane_sum(pi, shape))
        assert torch.equal(rdg, pdg) and torch.equal(rdb, pdb)
        assert torch.equal(unblock_rows(again[i][0], shape), got)
    assert not keep.all() and keep.any()


def _supported(pkg, x_shape, w_shape, stride, pad, dil):
    d = pkg.ops._desc(x_shape, w_shape, stride, pad, dil)
    return pkg._lib.lib().p3d_fx_conv_img_supported(ctypes.byref(d)), (d.N, d.K, d.Ho, d.Wo)


#               name                 N  C     K    H   k  stride pad dil
FWD_DGRAD = [('1x1_64_256',          2, 64,   256, 16, 1, 1, 0, 1),        # 128-row tile, four K steps
             ('1x1_256_64',          3, 256,  64,  16, 1, 1, 0, 1),        # forward: 64-row fx16 tile
             ('1x1_64_256_back',     3, 256,  64,  16, 1, 1, 0, 1),        # (its data gradient: 256 rows from 64 reduction channels)
             ('3x3_64_192',          2, 64,   192, 16, 3, 1, 1, 1),        # 96-row tile
             ('3x3_dil2_128_128',    2, 128,  128, 16, 3, 1, 2, 2),
             ('1x1_s2_128_256',      3, 128,  256, 16, 1, 2, 0, 1),        # strided forward; data gradient: one live parity class, three dead ones
             ('3x3_s2_64_64',        2, 64,   64,  16, 3, 2, 1, 1),        # data gradient: all four parity classes
             ('3x3_tapi_1024_128',   2, 1024, 128, 8,  3, 1, 1, 1),        # forward: tap-inner, 128 rows, split-K
             ('3x3_tapi_1024_96',    2, 1024, 96,  8,  3, 1, 1, 1),        # forward: tap-inner, 96 rows
             ('3x3_tapi_128_1024',   2, 128,  1024, 8, 3, 1, 1, 1),        # data gradient: tap-inner to 128 rows
             ('3x3_tapi_96_1024',    2, 96,   1024, 8, 3, 1, 1, 1)]        # data gradient: tap-inner to 96 rows
FORCED_SPLIT = {'1x1_64_256', '3x3_64_192'}


def _conv_case(pkg, case, pass_, force_split):
    ops, L = pkg.ops, pkg._lib.lib()
    _, n, c, k, h, ks, stride, pad, dil = case
    x_shape, w_shape = (n, c, h, h), (k, c, ks, ks)
    bits, y_shape = _supported(pkg, x_shape, w_shape, stride, pad, dil)
    assert bits & (1 if pass_ == 'fwd' else 2), 'the image-fed kernels refuse this test shape'
    gen = torch.Generator(device='cuda').manual_seed(n + c + k)
    w = torch.randn(w_shape, device='cuda', generator=gen) * 0.1
    src = torch.randn(x_shape if pass_ == 'fwd' else y_shape, device='cuda', generator=gen)
    key = 'x_img' if pass_ == 'fwd' else 'dy_img'
    out = {}
    try:
        L.p3d_fx_tune(1, force_split)
        with FencedAllocations() as fa:
            imgs = {False: ops.act_image(src), True: ops.row_image(src)}
            for rows in (False, True):
                out[rows] = ops.conv2d_img(pass_, x_shape, w, stride, pad, dil, rows=rows, **{key: imgs[rows]})
            torch.cuda.synchronize()
        fa.check()
    finally:
        L.p3d_fx_tune(1, 0)
    assert torch.isfinite(out[False]).all()
    assert torch.equal(out[True], out[False])


@pytest.mark.parametrize('case', FWD_DGRAD, ids=[c[0] for c in FWD_DGRAD])
@pytest.mark.parametrize('pass_', ['fwd', 'dgrad'])
def test_row_fed_forward_and_data_gradient_equal_plane_fed(pkg, case, pass_):
    _conv_case(pkg, case, pass_, 0)


@pytest.mark.parametrize('case', [c for c in FWD_DGRAD if c[0] in FORCED_SPLIT], ids=[c[0] for c in FWD_DGRAD if c[0] in FORCED_SPLIT])
@pytest.mark.parametrize('pass_', ['fwd', 'dgrad'])
def test_row_fed_split_k_equals_plane_fed(pkg, case, pass_):
    _conv_case(pkg, case, pass_, 2)


def test_row_fed_data_gradient_accumulates(pkg):
    """dx += dgrad: the accumulate path of the staged store, on a row-fed launch"""
    ops = pkg.ops
    x_shape, w_shape = (2, 64, 16, 16), (256, 64, 1, 1)
    gen = torch.Generator(device='cuda').manual_seed(3)
    w = torch.randn(w_shape, device='cuda', generator=gen) * 0.1
    dy = torch.randn(2, 256, 16, 16, device='cuda', generator=gen)
    base = torch.randn(x_shape, device='cuda', generator=gen)
    out = {}
    with FencedAllocations() as fa:
        for rows in (False, True):
            img = ops.row_image(dy) if rows else ops.act_image(dy)
            acc = torch.empty_like(base).copy_(base)
            out[rows] = ops.conv2d_img('dgrad', x_shape, w, 1, 0, 1, dy_img=img, accumulate_into=acc, rows=rows)
        torch.cuda.synchronize()
    fa.check()
    assert torch.equal(out[True], out[False]) and not torch.equal(out[True], base)


#          name               N  C    K    H   k  stride pad  x as image
WGRAD = [('1x1_128_128',      2, 128, 128, 16, 1, 1, 0, True),
         ('3x3_64_64',        3, 64,  64,  16, 3, 1, 1, True),         # three taps per column tile
         ('3x3_64_128',       2, 64,  128, 16, 3, 1, 1, True),         # two taps per column tile
         ('3x3_128_128',      2, 128, 128, 16, 3, 1, 1, True),         # one tap per block, shifted windows
         ('1x1_256_64_fp32x', 2, 256, 64,  16, 1, 1, 0, False),        # image dy x fp32 x
         ('1x1_s2_fp32x',     3, 128, 256, 16, 1, 2, 0, False)]        # the same, strided


@pytest.mark.parametrize('case', WGRAD, ids=[c[0] for c in WGRAD])
@pytest.mark.parametrize('splits', [1, 3])
def test_row_fed_weight_gradient_equals_plane_fed(pkg, case, splits):
    ops, L = pkg.ops, pkg._lib.lib()
    _, n, c, k, h, ks, stride, pad, x_as_image = case
    x_shape, w_shape = (n, c, h, h), (k, c, ks, ks)
    bits, y_shape = _supported(pkg, x_shape, w_shape, stride, pad, 1)
    assert bits & 4, 'the image-fed weight gradient refuses this test shape'
    gen = torch.Generator(device='cuda').manual_seed(c + k + splits)
    w = torch.randn(w_shape, device='cuda', generator=gen)
    x = torch.randn(x_shape, device='cuda', generator=gen)
    dy = torch.randn(y_shape, device='cuda', generator=gen)
    out = {}
    try:
        L.p3d_fx_tune(0, splits)
        with FencedAllocations() as fa:
            for rows in (False, True):
                image = ops.row_image if rows else ops.act_image
                out[rows] = ops.conv2d_img('wgrad', x_shape, w, stride, pad, 1, dy_img=image(dy), x_img=image(x) if x_as_image else None,
                                           x=None if x_as_image else x, rows=rows)
            torch.cuda.synchronize()
        fa.check()
    finally:
        L.p3d_fx_tune(0, 0)
    assert torch.isfinite(out[False]).all() and float(out[False].abs().max()) > 0
    assert torch.equal(out[True], out[False])


#          kind          inplanes planes stride dil downsample  side  forced split count of forward / data gradient (0: the built-in plan)
BLOCKS = [('bottleneck', 256, 64,  1, 1, False, 16, 0),         # identity shortcut; 64-channel 16 x 16 inner layers, the opening pass reads the mask bytes
          ('bottleneck', 128, 64,  2, 1, True,  16, 0),         # stride-2 3x3, strided downsample: pair pass with mask bytes, strided data gradients
          ('bottleneck', 512, 128, 1, 2, True,  16, 0),         # dilation 2
          ('basic',      64,  64,  1, 1, False, 16, 0),
          ('bottleneck', 768, 192, 1, 1, False, 16, 1),         # 192 rows, unsplit: the 96-row tile with the BatchNorm epilogues (statistics; backward sums)
          ('bottleneck', 4096, 1024, 1, 1, False, 8, 1)]        # a 1024-deep 3x3, unsplit: the tap-inner K order with the BatchNorm epilogues


@pytest.mark.parametrize('case', BLOCKS, ids=['%s_c%d_p%d_s%d_d%d%s' % (c[0], c[1], c[2], c[3], c[4], '_ds' if c[5] else '') for c in BLOCKS])
def test_block_is_bit_identical_in_both_formats(pkg, case):
    import test_block_gpu as tb
    ob = pkg.ops_block
    kind, inplanes, planes, stride, dil, with_ds, side, force_split = case
    expansion = 4 if kind == 'bottleneck' else 1
    gen = torch.Generator(device='cuda').manual_seed(21)
    x0 = torch.randn(2, inplanes, side, side, device='cuda', generator=gen).relu_()
    dy = torch.randn(2, planes * expansion, side // stride, side // stride, device='cuda', generator=gen)
    res, images, masks = {}, {}, {}
    L = pkg._lib.lib()
    try:
        L.p3d_fx_tune(1, force_split)
        for planes_fmt in (False, True):
            ob.plane_images(planes_fmt)
            torch.manual_seed(79)
            block = tb.build(pkg, kind, inplanes, planes, stride, dil, with_ds, seed=6)          # (a fresh module: its plan owns the buffers of this format)
            with FencedAllocations() as fa:
                res[planes_fmt] = tb.run(pkg, block, x0, dy, fused=True)
            fa.check()
            plan = next(iter(block.__dict__['_blk_plans'].values()))
            bufs = plan.sets[0]
            per_el = 6 if planes_fmt else 4
            named = [('a%d' % s, t, plan.shapes[s]) for s, t in bufs.act.items()] + [('dc%d' % s, t, plan.shapes[s]) for s, t in bufs.bwd[0].items()]
            assert named and all(fa.holds(t) for _, t, _ in named), 'the images must lie in fenced buffers of their exact size'
            for name, t, shape in named:
                assert t.numel() == per_el * shape[0] * shape[1] * shape[2] * shape[3], name
                images[planes_fmt, name] = plane_sum(t, shape) if planes_fmt else unblock_rows(t, shape).double()
            masks[planes_fmt] = None if bufs.mask is None else bufs.mask.clone()
    finally:
        ob.plane_images(False)
        L.p3d_fx_tune(1, 0)
    rows, pl = res[False], res[True]
    assert torch.equal(rows['y'], pl['y']) and torch.equal(rows['dx'], pl['dx'])
    for n, g in pl['grads'].items():                       # every dw, dgamma, dbeta
        assert torch.equal(rows['grads'][n], g), n
    for n, b in pl['buffers'].items():                     # running statistics
        assert torch.equal(rows['buffers'][n], b), n
    assert (masks[False] is None) == (masks[True] is None)
    if masks[False] is not None:
        assert torch.equal(masks[False], masks[True])
    for (fmt, name), v in images.items():                  # every a_i and d c_i, the pair pass's two included: the row image is the sum of the planes
        if not fmt:
            assert torch.isfinite(v).all(), name
            assert torch.equal(v, images[True, name]), name
