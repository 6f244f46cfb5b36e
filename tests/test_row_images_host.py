"""Row images (fp32 [N][C/16][HW][16], 4 B per element) on the host side: the size query, the block executor's buffer plan (row images for dense blocks, three
bf16 planes for masked ones) and the p3d_fx_tune code that switches the executor back to planes.  No GPU call is made."""
import ctypes

import pytest
import torch


@pytest.mark.parametrize('n,c,hw', [(3, 48, 144), (64, 256, 4096), (1, 16, 4)])
def test_row_image_bytes(pkg, n, c, hw):
    L = pkg._lib.lib()
    assert L.p3d_fx_row_image_bytes(n, c, hw) == 4 * n * c * hw
    assert L.p3d_fx_act_image_bytes(n, c, hw) == 6 * n * c * hw               # the plane format keeps its size
    assert L.p3d_fx_row_image_bytes(0, c, hw) == 0 and L.p3d_fx_row_image_bytes(n, -16, hw) == 0


def _desc(pkg, masked):
    d = pkg.ops_block.BlockDesc()
    d.nconv, d.masked = 3, int(masked)
    return d


def test_block_image_bytes_by_block_kind_and_tune_code(pkg):
    L = pkg._lib.lib()
    n, c, hw = 2, 64, 256
    dense, masked = _desc(pkg, False), _desc(pkg, True)
    try:
        assert L.p3d_block_image_bytes(ctypes.byref(dense), n, c, hw) == 4 * n * c * hw
        assert L.p3d_block_image_bytes(ctypes.byref(masked), n, c, hw) == 6 * n * c * hw
        L.p3d_fx_tune(6, 1)                                                    # planes everywhere
        assert L.p3d_block_image_bytes(ctypes.byref(dense), n, c, hw) == 6 * n * c * hw
        assert L.p3d_block_image_bytes(ctypes.byref(masked), n, c, hw) == 6 * n * c * hw
        L.p3d_fx_tune(6, 0)                                                    # and back
        assert L.p3d_block_image_bytes(ctypes.byref(dense), n, c, hw) == 4 * n * c * hw
    finally:
        L.p3d_fx_tune(6, 0)
    assert L.p3d_block_image_bytes(None, n, c, hw) == 0


def test_buffer_plan_sizes_images_from_the_query(pkg):
    """ops_block._Plan: every image of a dense block is 4 B per element of the conv output it mirrors; under plane_images(True) -- and for a masked plan -- 6 B.
    A plan made under one format is not handed out under the other."""
    ob, tr = pkg.ops_block, pkg._trunk
    block = tr.Bottleneck(256, 64, 1, 1, None)
    x_shape = (2, 256, 16, 16)
    try:
        plan = ob._Plan(block, x_shape)
        assert sorted(plan.slots) == [0, 1, 2]
        for slot in plan.slots:
            nn, k, h, w = plan.shapes[slot]
            assert plan.image_bytes[slot] == 4 * nn * k * h * w
        masked = ob._Plan(block, x_shape, masked=True)
        for slot in masked.slots:
            nn, k, h, w = masked.shapes[slot]
            assert masked.image_bytes[slot] == 6 * nn * k * h * w
        assert ob.plane_images(True) is False
        planes = ob._Plan(block, x_shape)
        for slot in planes.slots:
            nn, k, h, w = planes.shapes[slot]
            assert planes.image_bytes[slot] == 6 * nn * k * h * w
        x = torch.empty(x_shape)
        a = ob.plan_for(block, x)
        assert ob.plane_images(False) is True
        b = ob.plan_for(block, x)
        assert a is not b and a.image_bytes[0] == 6 * 2 * 64 * 256 and b.image_bytes[0] == 4 * 2 * 64 * 256
    finally:
        ob.plane_images(False)
