"""What tests/test_small_kernels_gpu.py takes for granted, checked without a GPU: the float64 restatement of the distillation loss against the reference's own
outputs, the conditions its cases rely on (evaluated on the very inputs its builders return), and that each case meant to leave one pass of a kernel's grid
does leave it."""
import numpy as np
import pytest
import torch

import test_small_kernels_gpu as cases
from conftest import golden_path
from oracle import np_ops as ref


# ---- the new reference function -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', cases.DISTILL_MODES)
def test_distill_restatement_matches_the_reference(mode):
    """tests/golden/distill.npz holds what the reference's own Trainer.distill returned and its autograd gradient (fp32): the pin, before anything is judged by it"""
    g = np.load(golden_path('distill.npz'))
    loss, ds = ref.distill_fwd_bwd(g['t'], g['s'], g['a'], mode)
    assert tuple(g['s'].shape) == cases.DISTILL_SHAPES[0]
    assert abs(loss - float(g[mode + '.loss'])) < 1e-6 * abs(float(g[mode + '.loss']))
    assert np.abs(ds - g[mode + '.ds']).max() < 1e-6 * np.abs(g[mode + '.ds']).max()


@pytest.mark.parametrize('same_first', (False, True))
@pytest.mark.parametrize('mode', cases.DISTILL_MODES)
def test_distill_restatement_matches_float64_autograd(mode, same_first):
    """Trainer.distill's expressions (depth_train.py:115-129) under float64 autograd; with t[0] == s[0] torch.linalg.norm's backward gives that sample a zero
    gradient (not a NaN), the convention of the restatement and of the kernel."""
    shape = (2, 9, 17, 15)
    t, s, a = (torch.from_numpy(v).double() for v in cases.distill_inputs(shape, same_first))
    s.requires_grad_(True)
    if mode == 'bce':
        diff = torch.nn.functional.binary_cross_entropy_with_logits(s, torch.sigmoid(t)) * a
        want = diff.view(shape[0], -1).sum(-1).mean()
    else:
        diff = ((torch.sigmoid(t) - torch.sigmoid(s)) if mode == 'sigmoid' else (t - s)) * a
        want = torch.linalg.norm(diff.view(shape[0], -1), dim=-1).mean()
    want.backward()
    want = want.detach()
    loss, ds = ref.distill_fwd_bwd(t.numpy(), s.detach().numpy(), a.numpy(), mode)
    assert abs(loss - float(want)) < 1e-12 * abs(float(want))
    assert np.abs(ds - s.grad.numpy()).max() < 1e-12 * float(s.grad.abs().max())
    if same_first:
        assert torch.isfinite(s.grad).all() and not s.grad[0].any() and not ds[0].any()


# ---- the conditions of the cases ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', cases.POSE_CASES)
def test_pose_cases_keep_clear_of_the_knots(case):
    """SmoothL1 has a knot at |diff| = 1, L1 at 0.  No element outside the key joint comes within 1e-4 of either, for loss_div 1 and 10, so that no fp32 rounding
    of `spec` puts an element on the other branch; nothing is masked out to get there (the patterns only take validity away).  The key joint's own diff is an exact
    zero in both precisions: there L1's gradient is sign(0) = 0 in the kernel and in the oracle alike."""
    b, j, key = case
    relat, cam, val = cases.pose_inputs(b, j, key, 'all')
    assert val.all()
    for loss_div in (1.0, 10.0):
        to_one, to_zero, key_diff = cases.pose_knot_distances(relat, cam, key, loss_div)
        assert to_one > cases.KNOT_MARGIN and to_zero > cases.KNOT_MARGIN and key_diff == 0.0
        spec32 = relat - relat[:, key:key + 1] + cam[:, key:key + 1]
        assert np.array_equal(spec32[:, key], cam[:, key])
    some = cases.pose_inputs(b, j, key, 'some')[2]
    assert cases.pose_inputs(b, j, key, 'none')[2].sum() == 0 and not cases.pose_inputs(b, j, key, 'sample')[2][b // 2].any()
    assert some[:, key].all() and (b * j < 100 or 0.6 < np.delete(some, key, axis=1).mean() < 0.8)
    assert not cases.pose_inputs(b, j, key, 'key')[2][0, key]
    for pattern in cases.POSE_PATTERNS:                                            # the values are the same under every pattern
        assert all(np.array_equal(x, y) for x, y in zip(cases.pose_inputs(b, j, key, pattern)[:2], (relat, cam)))


@pytest.mark.parametrize('shape', cases.MASKED_SHAPES)
def test_masked_cases_keep_clear_of_the_knots(shape):
    pred, target, valid = cases.masked_inputs(shape, 'some')
    to_one, to_zero = cases.masked_knot_distances(pred, target)
    assert to_one > cases.KNOT_MARGIN and to_zero > cases.KNOT_MARGIN
    assert valid.any() and cases.masked_inputs(shape, 'none')[2].sum() == 0


def test_recon_cases_are_well_conditioned():
    for b in cases.RECON_BATCHES:
        for j in cases.RECON_JOINTS:
            for skew in (False, True):
                spec_mat, relat, K, _ = cases.recon_inputs(b, j, skew)
                assert cases.recon_condition(spec_mat, relat, K) < 1e6
                assert (K[:, 0, 1] != 0).all() == skew and not K[:, 1, 0].any()


def test_enhance_case_leaves_out_next_to_nothing():
    x, factor = cases.enhance_inputs()
    for thr in (0.1, 0.5):
        for f in (None, factor):
            assert cases.enhance_edge(x, f, thr).mean() < 1e-3


# ---- the loop bounds -----------------------------------------------------------------------------------------------------------------------------------------------
# What one pass of each launch covers.  This table is a COPY of constants in the C sources (grid caps x block size x elements per thread), by launch line; whoever
# raises a cap there raises it here, and test_cases_leave_one_pass then says which case has to grow with it.
ONE_PASS = dict(
    pose_loss=256,                        # p3d_head.hip p3d_pose_loss_fwd_bwd: pose_loss_kernel, dim3(1) x dim3(256), loops over B*J, 3*B*J and 3*B
    masked_loss=256,                      # p3d_head.hip p3d_masked_loss_fwd_bwd: masked_loss_kernel, dim3(1) x dim3(256), loops over rows and rows*C
    recon_cam=64,                         # p3d_head.hip p3d_recon_cam_fwd / _bwd: ceil_div(B, 64) blocks of 64 threads, a sample each
    distill=32 * 256,                     # p3d_distill.hip p3d_distill_fwd_bwd: grid (B, DISTILL_SPLIT = 32) x 256 per sample, blocks 256 values apart
    flat_float4=2048 * 256 * 4,           # p3d_optim.hip p3d_l2norm_sq_accum / p3d_adam_step: min(ceil_div(n, 1024), 2048) blocks x 256, float4 per thread
    flat_scalar=2048 * 256,               #   the same grids on l2norm_sq_scalar_kernel, adam_kernel<false> and (p3d_adam_step_dev) adam_dev_kernel
    augment_colour=64 * 256,              # p3d_optim.hip p3d_augment_colour: min(ceil_div(HW, 256), 64) blocks per image
    augment_erase=16 * 256,               # p3d_optim.hip p3d_augment_erase: dim3(16, C, B) over the clipped rectangle
    augment_occlude=64 * 256,             # p3d_optim.hip p3d_augment_occlude: min(ceil_div(max_pixels, 256), 64) blocks per image
    normalize=32 * 256,                   # p3d_optim.hip p3d_normalize_rgb: dim3(32, 3 * B) per plane
    crops=256 * 256,                      # p3d_optim.hip p3d_warp_crops / p3d_reproject_crops: min(ceil_div(Ho*Wo, 256), 256) blocks per image
    enhance_depth=4096 * 256,             # p3d_optim.hip p3d_enhance_depth
    maxpool=8192 * 256,                   # p3d_head.hip p3d_maxpool3x3s2_fwd / _bwd, generic kernels: outputs (forward), inputs (backward)
    maxpool4=16384 * 256,                 #   W % 4 == 0 kernels: quads of input columns per output row (forward), per input row (backward)
    relu=4096 * 256,                      # p3d_bn.hip p3d_relu_fwd / _bwd
    masks=2048 * 256,                     # p3d_conv.hip p3d_mask_count_fwd / p3d_nonzero_mask
)


def test_cases_leave_one_pass(pkg):
    one = ONE_PASS
    # pose loss: the key-joint pass (3 * B) in two iterations and in one; B * J past the block; the issue's 25-joint skeleton
    assert any(3 * b > one['pose_loss'] for b, j, k in cases.POSE_CASES) and any(3 * b <= one['pose_loss'] < 3 * b * j for b, j, k in cases.POSE_CASES)
    assert any(b * j > one['pose_loss'] for b, j, k in cases.POSE_CASES) and any(b * j * 3 <= one['pose_loss'] for b, j, k in cases.POSE_CASES)
    assert {k for _, _, k in cases.POSE_CASES} >= {0, 16} and any(j == 25 for _, j, _ in cases.POSE_CASES)
    assert any(b * j > one['masked_loss'] for b, j, c in cases.MASKED_SHAPES) and any(b * j * c <= one['masked_loss'] for b, j, c in cases.MASKED_SHAPES)
    # recon_cam: a block exactly full, one sample more, a third block
    assert one['recon_cam'] in cases.RECON_BATCHES and one['recon_cam'] + 1 in cases.RECON_BATCHES and max(cases.RECON_BATCHES) > 2 * one['recon_cam']
    # distillation: values per sample
    per = [c * h * w for _, c, h, w in cases.DISTILL_SHAPES]
    assert per == [200, 3, 245, 2295, 8415, 10530, 32768]
    assert min(per) < 256 and sum(p > one['distill'] for p in per) >= 3
    assert any(256 < p < one['distill'] and (h * w) % 256 and 256 % (h * w) for p, (_, c, h, w) in zip(per, cases.DISTILL_SHAPES))      # several blocks live, ragged, an
    assert any(p > one['distill'] and 256 % (h * w) for p, (_, c, h, w) in zip(per, cases.DISTILL_SHAPES))               # attention index that is not i % 256
    # flat buffers
    n = max(cases.FLAT_SIZES)
    assert n > one['flat_float4'] + 1024 and n % 4 == 3 and n > 4 * one['flat_scalar']
    assert {s % 4 for s in cases.FLAT_SIZES} == {0, 1, 3} and min(cases.FLAT_SIZES) == 1 and {1023, 1025} <= set(cases.FLAT_SIZES)       # ceil_div(n, 1024): 1 and 2 blocks
    assert all(len(o) == 4 for o in cases.ADAM_OFFSETS.values()) and sorted(map(sum, cases.ADAM_OFFSETS.values())) == [0, 1, 1, 1, 1, 4]
    # image side
    assert cases.COLOUR_SHAPE[2] * cases.COLOUR_SHAPE[3] > one['augment_colour']
    x0, y0, x1, y1 = cases.ERASE_RECTS[0]
    assert (x1 - x0) * (y1 - y0) > one['augment_erase'] and 0 <= x0 < x1 <= cases.ERASE_SHAPE[3] and 0 <= y0 < y1 <= cases.ERASE_SHAPE[2]
    for chan in (1, 3):
        images, occ, alpha, centers = cases.paste_inputs(chan)
        plans = [pkg.augment.plan_paste(occ.shape, images.shape[1:3], c) for c in centers[:2]]
        assert plans[0][4] * plans[0][5] == occ.shape[0] * occ.shape[1] > one['augment_occlude'] and 0 < plans[1][4] * plans[1][5] < plans[0][4] * plans[0][5]
    assert cases.NORMALIZE_SHAPE[2] * cases.NORMALIZE_SHAPE[3] > one['normalize']
    assert cases.CROP_SIDE ** 2 > one['crops']
    assert int(np.prod(cases.ENHANCE_SHAPE)) > one['enhance_depth']
    # pool, ReLU, masks
    (n0, c0, h0, w0), (n1, c1, h1, w1) = cases.POOL_SHAPES
    ho, wo = (h0 - 1) // 2 + 1, (w0 - 1) // 2 + 1
    assert w0 % 4 and n0 * c0 * ho * wo > one['maxpool'] and n0 * c0 * h0 * w0 > one['maxpool']
    assert w1 % 4 == 0 and n1 * c1 * ((h1 - 1) // 2 + 1) * (w1 // 4) > one['maxpool4'] and n1 * c1 * h1 * (w1 // 4) > one['maxpool4']
    assert int(np.prod(cases.RELU_SHAPE)) > one['relu']
    assert int(np.prod(cases.PCONV_SHAPE)) > one['masks']
