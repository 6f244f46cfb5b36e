"""Strided residual blocks at any map width (ops.block_any_strided / p3d_block_any_strided_enable): dense blocks that carry a stride-2 convolution, at maps the
aligned kernels refuse, through p3d_block_fwd / p3d_block_bwd.

1. Whole blocks: tests/test_block_gpu.py::fused_block_case unchanged -- admission, the other path really ran, the project's float64 bounds.
2. block_strided_join_any_kernel alone (p3d_block_strided_join): g bit-equal to the interleave of the same planes, the sums per channel within
   8 * 2^-24 * sum |summand| of float64 (two fp32 roundings per summand, c - mean and the product: 2 * 2^-24; fp32 partial sums of up to four terms: at most
   3 * 2^-24 more; the fp64 accumulation adds nothing at this scale), a second launch the same bits.
3. The image-fed stride-2 data gradient alone (p3d_fx_conv_dgrad_strided_img_any) against float64 conv2d_input, below X3_TOL of the largest reference value.
4. The stride-2 forward with the statistics epilogue alone: the body of tests/test_block_anysize_gpu.py::test_instance_alone at stride 2, with its bound.
5. Nothing else moves.  6. Reproducibility and the launch log.  7. Fenced exact-size buffers.  8. Two steps of a network.

The network case runs ResNet-18 and ResNet-50 at side 65.  ResNet-18's blocks carry the stride on conv 0, which has no BatchNorm in front of it inside the block and
is finished by the interleave, so no BasicBlock can launch the join kernel: the ResNet-18 leg asserts the image-fed class launches and the interleave's record, the
ResNet-50 leg at the same side and batch (Bottlenecks: the stride on the 3x3 behind a BatchNorm) the join's."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import fenced
from test_block_anysize_gpu import RAGGED_CASES
from test_block_gpu import CASES, fused_block_case, make_case, run
from test_kernels_gpu import X3_TOL

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(os.environ.get('P3D_X3', '1') == '0', reason='the block executor needs the x3 kernels')]

U = 2.0 ** -24
MARGIN = 1e-3
FINISH_INTERLEAVE_ROWS, FINISH_STRIDED_JOIN = 5, 6

#                kind          inplanes planes stride dil  N  H[xW]   downsample
STRIDED_CASES = [('bottleneck', 256, 128, 2, 1, 2, 33, True),          # the shape that stays out today
                 ('bottleneck', 128, 64, 2, 1, 3, (9, 7), True),       # HW = 63, class planes of four different sizes, 20 output pixels
                 ('basic', 64, 128, 2, 1, 2, 9, True),                 # the stride on conv 0, from the image of x: no join kernel
                 ('bottleneck', 128, 64, 2, 1, 2, (6, 14), True),      # even sides, equal classes, a plane on a 16-B line with rows that are not
                 ('bottleneck', 256, 64, 2, 1, 5, 17, True)]           # class (0, 0) has 405 pixels: four tiles, the last partial


def _id(c):
    h = c[6] if isinstance(c[6], int) else '%dx%d' % c[6]
    return '%s_c%d_p%d_s%d_d%d_n%d_h%s%s' % (c[0], c[1], c[2], c[3], c[4], c[5], h, '_ds' if c[7] else '')


@pytest.fixture
def strided(pkg):
    """the new switch on and ops.block_any off for the test body; both restored, with the forced split counts, afterwards"""
    before = (pkg.ops.block_any_strided(True), pkg.ops.block_any(False))
    try:
        yield pkg.ops.block_any_strided
    finally:
        pkg.ops.block_any_strided(before[0])
        pkg.ops.block_any(before[1])
        pkg._lib.lib().p3d_fx_tune(1, 0)


def _log(pkg):
    return pkg.ops.fx_launch_log(reset=True)[0]


def _same(a, b):
    return (torch.equal(a['y'], b['y']) and torch.equal(a['dx'], b['dx']) and all(torch.equal(a['grads'][k], b['grads'][k]) for k in a['grads'])
            and all(torch.equal(a['buffers'][k], b['buffers'][k]) for k in a['buffers']))


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


# ---- 1. whole blocks ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', STRIDED_CASES, ids=_id)
def test_strided_ragged_block_matches_per_layer_path_and_float64(case, pkg, strided):
    fused_block_case(pkg, *case)


# ---- 2. the join kernel alone ------------------------------------------------------------------------------------------------------------------------------
JOIN_SHAPES = [(3, 32, 5, 5), (2, 16, 7, 9), (3, 32, 6, 14)]


@pytest.mark.parametrize('live', [0b1111, 0b0001], ids=['live15', 'live1'])
@pytest.mark.parametrize('shape', JOIN_SHAPES, ids=['n%d_c%d_%dx%d' % s for s in JOIN_SHAPES])
def test_join_kernel_alone(shape, live, pkg):
    ops, L = pkg.ops, pkg._lib.lib()
    n, c, h, w = shape
    hw, split = h * w, 2
    gen = torch.Generator(device='cuda').manual_seed(7000 + 16 * hw + live)
    cls_stride = (n * c * ((h + 1) // 2) * ((w + 1) // 2) + 3) // 4 * 4
    want = torch.zeros(n, c, h, w, device='cuda')
    stage, sfence = fenced.fenced_like((4 * cls_stride,), torch.float32, 256)            # poison = NaN: the planes of dead classes and the gaps between planes
    assert torch.isnan(stage).all()
    for cls in range(4):
        if (live >> cls) & 1:
            plane = torch.randn(n * c, (h - cls // 2 + 1) // 2, (w - cls % 2 + 1) // 2, device='cuda', generator=gen)
            stage[cls * cls_stride:cls * cls_stride + plane.numel()] = plane.reshape(-1)
            want[:, :, cls // 2::2, cls % 2::2] = plane.view(n, c, plane.shape[1], plane.shape[2])          # the torch index interleave
    tab = torch.full((c, 8), float('nan'), device='cuda')
    tab[:, 0], tab[:, 1], tab[:, 2] = torch.rand(c, device='cuda', generator=gen) + 0.5, torch.randn(c, device='cuda', generator=gen) * 0.5, torch.randn(c, device='cuda', generator=gen) * 0.3
    sc, sh, mean = (tab[:, i].double().view(1, -1, 1, 1) for i in range(3))
    cc = torch.randn(n, c, h, w, device='cuda', generator=gen).double()
    z = cc * sc + sh
    away = (z >= 0).double() * (4 * MARGIN) - 2 * MARGIN
    cc = torch.where(z.abs() < 2 * MARGIN, (away - sh) / sc, cc).float()
    z = cc.double() * sc + sh
    assert z.abs().min().item() >= MARGIN and (z > 0).any() and (z < 0).any()
    cbuf, cfence = fenced.fenced_like(shape, torch.float32, 256)
    cbuf.copy_(cc)

    def launch():
        g, gfence = fenced.fenced_like(shape, torch.float32, 256)
        partial, pfence = fenced.fenced_like((c, split, 3), torch.float64, 64)
        rc = L.p3d_block_strided_join(ops._p(stage), ops._p(cbuf), ops._p(tab), ops._p(g), ops._p(partial), n, c, h, w, cls_stride, live, split, ops._stream())
        torch.cuda.synchronize()
        assert rc == 0, L.p3d_last_error()
        for f, what in ((gfence, 'g'), (pfence, 'partial sums'), (sfence, 'class planes'), (cfence, 'c')):
            f.check('join %s' % what)
        return g, partial

    g, partial = launch()
    dx = torch.full(shape, float('nan'), device='cuda')
    pkg._lib.check(L.p3d_dgrad_interleave(1, ops._p(stage), ops._p(dx), None, n, c, h, w, cls_stride, live, 0, ops._stream()), 'p3d_dgrad_interleave')
    torch.cuda.synchronize()
    assert torch.equal(_bits(g), _bits(dx)) and torch.equal(_bits(g), _bits(want))
    assert torch.equal(cbuf, cc) and torch.isfinite(partial).all() and bool((partial[:, :, 2] == 0).all())
    gg = want.double() * (z > 0)
    mine = partial.sum(1)
    for i, s in enumerate((gg, gg * (cc.double() - mean))):
        ref, ref_abs = s.sum((0, 2, 3)), s.abs().sum((0, 2, 3))
        diff, bound = (mine[:, i] - ref).abs(), 8 * U * ref_abs
        print('JOIN %s live %d sum %d worst |diff| / bound %.3g' % (shape, live, i, (diff / bound.clamp_min(1e-300)).max().item()))
        assert bool((diff <= bound).all()), (shape, live, i, (diff / bound.clamp_min(1e-300)).max().item())
    # each image group alone: block (ch, s) owns images s, s + split, ...
    for s_ in range(split):
        ref = gg[s_::split].sum((0, 2, 3))
        assert bool(((partial[:, s_, 0] - ref).abs() <= 8 * U * gg[s_::split].abs().sum((0, 2, 3))).all()), (shape, live, s_)
    g2, partial2 = launch()
    assert torch.equal(_bits(g), _bits(g2)) and torch.equal(_bits(partial), _bits(partial2))


# ---- 3. the image-fed strided data gradient alone ----------------------------------------------------------------------------------------------------------
DGRAD_SHAPES = [(3, 64, 64, 9, 7), (2, 128, 128, 17, 17), (2, 64, 64, 6, 14)]              # n, c, k, h, w


@pytest.mark.parametrize('r', [3, 1], ids=['3x3', '1x1'])
@pytest.mark.parametrize('shape', DGRAD_SHAPES, ids=['n%d_c%d_k%d_%dx%d' % s for s in DGRAD_SHAPES])
def test_image_fed_strided_data_gradient_alone(shape, r, pkg):
    ops, L = pkg.ops, pkg._lib.lib()
    n, c, k, h, w = shape
    pad = r // 2
    gen = torch.Generator(device='cuda').manual_seed(8000 + h * w + r)
    wt = torch.randn(k, c, r, r, device='cuda', generator=gen) / (k * r * r) ** 0.5
    d = ops._desc((n, c, h, w), (k, c, r, r), 2, pad, 1)
    dy = torch.randn(n, k, d.Ho, d.Wo, device='cuda', generator=gen)
    ref = torch.nn.grad.conv2d_input((n, c, h, w), wt.double(), dy.double(), 2, pad, 1)
    image = ops.act_image(dy)
    assert L.p3d_fx_conv_dgrad_strided_img_any_supported(ctypes.byref(d)) == 1
    assert L.p3d_fx_conv_img_any_supported(ctypes.byref(d)) & 2 == 0                    # the stride-1 entry keeps refusing it
    nbytes = L.p3d_fx_conv_dgrad_strided_img_any_workspace_bytes(ctypes.byref(d))
    assert nbytes > 0
    wimgT = None
    if r == 3:                                                                           # the cached data-gradient weight image; the 1x1 builds its own into the workspace
        fb, bb = ctypes.c_size_t(), ctypes.c_size_t()
        assert L.p3d_fx_weight_image_bytes(k, c, r * r, ctypes.byref(fb), ctypes.byref(bb)) == 0
        wf, wimgT = torch.empty(fb.value, dtype=torch.uint8, device='cuda'), torch.empty(bb.value, dtype=torch.uint8, device='cuda')
        assert L.p3d_fx_weight_images(ops._p(wt), k, c, r * r, ops._p(wf), ops._p(wimgT), ops._stream()) == 0, L.p3d_last_error()
    ws = fenced.Fence(nbytes, 4096, 'cuda')

    def call(accumulate, start):
        d.accumulate = accumulate
        dx, fence = fenced.fenced_like((n, c, h, w), torch.float32, 4096)
        if start is not None:
            dx.copy_(start)
        ops.fx_launch_log(reset=True)
        ops.conv_path_stats(reset=True)
        rc = L.p3d_fx_conv_dgrad_strided_img_any(ctypes.byref(d), ops._p(image), ops._p(wt), ops._p(wimgT), ops._p(dx), ops._p(ws.view), nbytes, ops._stream())
        torch.cuda.synchronize()
        assert rc == 0, L.p3d_last_error()
        fence.check('dx')
        ws.check('workspace')
        return dx, ops.fx_launch_log(reset=True)[0], ops.conv_path_stats(reset=True)

    dx, log, stats = call(0, None)
    err = ((dx.double() - ref).abs().max() / ref.abs().max()).item()
    print('ERR strided img dgrad %s %dx%d %.3g' % (shape, r, r, err))
    assert err < X3_TOL
    # image-fed ragged class launches, the interleave behind the last, nothing on the fp32-MFMA kernels
    assert len(log) == (4 if r == 3 else 1), log
    for i, rec in enumerate(log):
        assert (rec['kernel'], rec['amode'], rec['pro'], rec['epi'], rec['tapi'], rec['rag'], rec['rows']) == (0, 1, 0, 0, 0, 1, 0), rec
        assert rec['grid_y'] == 1 and rec['grid_z'] == 1 and rec['kchunk'] == 0 and rec['finish'] == (FINISH_INTERLEAVE_ROWS if i == len(log) - 1 else 0), rec
    assert stats['x3']['dgrad'][0] == 1 and all(v[0] == 0 for v in stats['fp32'].values()), stats
    if r == 1:                                                                           # the pixels no tap reaches: exactly +0
        dead = torch.ones(h, w, dtype=torch.bool, device='cuda')
        dead[0::2, 0::2] = False
        assert bool((_bits(dx)[:, :, dead] == 0).all())
    old = torch.randn(n, c, h, w, device='cuda', generator=gen)
    acc, log2, _ = call(1, old)
    assert torch.equal(acc, old + dx)
    if r == 1:
        assert torch.equal(acc[:, :, dead], old[:, :, dead])
    assert [rec['finish'] for rec in log2] == [rec['finish'] for rec in log]
    d.accumulate = 0


# ---- 4. the stride-2 forward with statistics alone ---------------------------------------------------------------------------------------------------------
FWD_CASES = [('s2_stats_3x3', 3, 64, 64, 9, 7, 3), ('s2_stats_1x1', 3, 64, 128, 9, 9, 1)]       # name, n, c, k, h, w, r


@pytest.mark.parametrize('case', FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_strided_forward_with_statistics_alone(case, pkg):
    name, n, c, k, h, w, r = case
    ops, L = pkg.ops, pkg._lib.lib()
    pad = r // 2
    gen = torch.Generator(device='cuda').manual_seed(9000 + r)
    wt = torch.randn(k, c, r, r, device='cuda', generator=gen) / (c * r * r) ** 0.5
    src = torch.randn(n, c, h, w, device='cuda', generator=gen)
    core = F.conv2d(src.double(), wt.double(), None, 2, pad, 1)
    shape = tuple(core.shape)
    d = ops._desc((n, c, h, w), (k, c, r, r), 2, pad, 1)
    assert shape == (n, k, d.Ho, d.Wo) and (h * w) % 4 != 0
    dref = ctypes.byref(d)
    f = pkg._lib.FxFuse()
    image = ops.act_image(src)                                      # (HW no multiple of 4: p3d_fx_act_image_any)
    f.act_img, f.ragged = ops._p(image), 1
    nbytes = L.p3d_fx_conv_fused_workspace_bytes(0, dref, 1)
    assert nbytes > 0
    pixels = n * d.Ho * d.Wo
    prows = -(-pixels // 128)                                       # one row per 128-pixel tile (the stride-1 query keeps refusing stride 2)
    assert L.p3d_fx_conv_fused_partial_rows_any(0, dref) == 0
    ws = fenced.Fence(nbytes, 4096, 'cuda')

    def call(with_sums):
        out, fence = fenced.fenced_like(shape, torch.float32, 4096)
        partial, pfence = fenced.fenced_like((prows, k, 2), torch.float32, 4096)
        f.partial = ops._p(partial) if with_sums else None
        ops.fx_launch_log(reset=True)
        rc = L.p3d_fx_conv_fused(0, dref, ctypes.byref(f), None, ops._p(wt), None, ops._p(out), ops._p(ws.view), nbytes, ops._stream())
        torch.cuda.synchronize()
        records = ops.fx_launch_log(reset=True)[0]
        assert rc == 0, L.p3d_last_error()
        fence.check('%s result' % name)
        pfence.check('%s partial sums' % name)
        ws.check('%s workspace' % name)
        return out, partial, records

    out, partial, records = call(True)
    assert len(records) == 1 and tuple(records[0][q] for q in ('kernel', 'amode', 'pro', 'epi', 'tapi', 'rag', 'rows')) == (0, 1, 0, 1, 0, 1, 0), records
    assert records[0]['grid_y'] == 1 and records[0]['kchunk'] == 0, records
    L.p3d_fx_tune(1, 1)                                             # the plain call unsplit too: the same K order
    try:
        plain, _, precords = call(False)
    finally:
        L.p3d_fx_tune(1, 0)
    assert len(precords) == 1 and precords[0]['epi'] == 0 and precords[0]['rag'] == 1 and precords[0]['kchunk'] == 0, precords
    assert torch.equal(out.view(torch.int32), plain.view(torch.int32))
    err = ((out.double() - core).abs().max() / core.abs().max()).item()
    print('ERR %s %.3g' % (name, err))
    assert err < X3_TOL
    mine = partial.double().sum(0)
    for i, s in enumerate((core, core * core)):
        ref, ref_abs, ref_max = s.sum((0, 2, 3)), s.abs().sum((0, 2, 3)), s.abs().max().item()
        bound = pixels * X3_TOL * ref_max + 128 * U * ref_abs
        diff = (mine[:, i] - ref).abs()
        print('SUM %s [%d] worst |diff| / bound %.3g' % (name, i, (diff / bound).max().item()))
        assert bool((diff <= bound).all()), (name, i, (diff / bound).max().item())


# ---- 5. nothing else moves ---------------------------------------------------------------------------------------------------------------------------------
def test_strided_blocks_stay_out_with_the_switch_off(pkg, strided):
    strided(False)
    pkg.ops.block_any(True)                                          # P3D_BLOCK_ANY alone admits what it admits today
    for case in STRIDED_CASES[:3]:
        block, x0, _, _ = make_case(pkg, *case, want_clean=False)
        assert not pkg.ops_block.usable(block, x0), case
    fused_block_case(pkg, *STRIDED_CASES[1], admitted=False)


@pytest.mark.parametrize('case,any_on', [(CASES[2], False), (CASES[5], False), (RAGGED_CASES[1], True)], ids=['aligned_strided_bottleneck', 'aligned_strided_basic', 'ragged_stride1'])
def test_other_blocks_launch_what_they_always_did(case, any_on, pkg, strided):
    """an aligned strided block and a stride-1 ragged block: the same bits and the same launch log with the new switch on and off"""
    block, x0, dy, _ = make_case(pkg, *case, want_clean=False)
    pkg.ops.block_any(any_on)
    got = {}
    for on in (False, True):
        strided(on)
        assert pkg.ops_block.usable(block, x0)
        _log(pkg)
        res = run(pkg, block, x0, dy, fused=True)
        got[on] = (res, _log(pkg))
    (a, log_a), (b, log_b) = got[False], got[True]
    assert log_a == log_b and len(log_a) > 0 and all(r['rag'] == int(any_on) for r in log_a)
    assert _same(a, b)


# ---- 6. reproducibility and the log ------------------------------------------------------------------------------------------------------------------------
def test_strided_block_is_bitwise_reproducible_and_launches_image_fed_ragged_instances(pkg, strided):
    block, x0, dy, _ = make_case(pkg, *STRIDED_CASES[1], want_clean=False)
    assert pkg.ops_block.usable(block, x0)
    run(pkg, block, x0, dy, fused=True)                              # (plans, buffers and weight images exist from here on)
    _log(pkg)
    pkg.ops.conv_path_stats(reset=True)
    first = run(pkg, block, x0, dy, fused=True)
    log, stats = _log(pkg), pkg.ops.conv_path_stats(reset=True)
    second = run(pkg, block, x0, dy, fused=True)
    assert _same(first, second)
    assert all(r['rag'] == 1 and r['amode'] == 1 and r['kernel'] == 0 and r['grid_y'] == 1 and r['kchunk'] == 0 for r in log), log
    # forward: four convolutions (downsample included), every one with the statistics; backward: conv 2 with the backward sums, four class launches of the strided
    # 3x3 finished by the join kernel, conv 0 plain, the one live class of the strided 1x1 finished by the interleave
    assert [r['epi'] for r in log[:4]] == [1, 1, 1, 1] and sorted(r['epi'] for r in log[4:]) == [0, 0, 0, 0, 0, 0, 2], log
    assert sorted(r['finish'] for r in log) == [0] * 9 + [FINISH_INTERLEAVE_ROWS, FINISH_STRIDED_JOIN], log
    assert all(v[0] == 0 for v in stats['fp32'].values()) and stats['x3']['fwd'][0] == 4 and stats['x3']['dgrad'][0] == 4 and stats['x3']['wgrad'][0] == 4, stats


# ---- 7. fenced exact-size buffers --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [STRIDED_CASES[1], STRIDED_CASES[2]], ids=_id)
def test_exact_size_fenced_buffers(case, pkg, strided):
    """every tensor the executor's Python side allocates at exactly its size, poisoned, between fences: the bands stay as they were and the results are those of an
    ordinary run, bit for bit.  (make_case builds the downsample pair before it seeds the generator, so the generator is seeded in front of both calls: the same module twice.)"""
    torch.manual_seed(77)
    block, x0, dy, _ = make_case(pkg, *case, want_clean=False)
    plain = run(pkg, block, x0, dy, fused=True)
    torch.manual_seed(77)
    block2, _, _, _ = make_case(pkg, *case, want_clean=False)                # the same module again,
    assert all(torch.equal(a, b) for a, b in zip(block.state_dict().values(), block2.state_dict().values()))
    assert pkg.ops_block.release_buffers(block2) > 0                         #   its plan and buffers to be made inside the fences
    with fenced.FencedAllocations() as fa:
        got = run(pkg, block2, x0, dy, fused=True)
        pkg.ops.join_side_stream()
        torch.cuda.synchronize()
    fa.check()
    assert len(fa.fences) > 10
    assert _same(plain, got)
    assert all(torch.isfinite(v).all() for v in [got['y'], got['dx']] + list(got['grads'].values()))


# ---- 8. a network ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model,extra', [('resnet18', []), ('resnet50', ['-stride', '16'])], ids=['resnet18', 'resnet50'])
def test_two_steps_of_a_resnet_at_side_65(model, extra, pkg, strided):
    """depthnet at side 65, batch 2, both block switches on: 17 x 17 maps behind the pool, layer2.0 goes 17 -> 9 and layer3.0 9 -> 5.  The losses are finite; the
    log shows image-fed class launches, the interleave's finishing record (every strided block: its downsample conv) and, for the Bottlenecks of ResNet-50, the join
    kernel's (a BasicBlock carries the stride on conv 0 and has none: see the module docstring)"""
    import test_step_gpu as S
    pkg.ops.block_any(True)
    args, net, trainer = S.build(pkg, {'model': model, 'side': 65, 'extra': extra})
    net.train()
    trainer.adapt_learn_rate(1)
    c, d, tc, tv = pkg.synth.make_batch(2, side=65, rank=0, step=0)
    batch = (torch.from_numpy(c).cuda(), None, torch.from_numpy(tc).cuda(), torch.from_numpy(tv).cuda())
    _log(pkg)
    losses, log = [], []
    for _ in range(2):
        losses.append(float(trainer.train_step(*batch)))
        records, count = pkg.ops.fx_launch_log(reset=True)              # (host-side bookkeeping; read per step: the library keeps the first 256 records)
        assert count == len(records)
        log += records
    pkg.ops.join_side_stream()
    torch.cuda.synchronize()
    assert all(l == l and abs(l) < float('inf') for l in losses), losses
    classes = [r for r in log if r['rag'] == 1 and r['amode'] == 1 and r['epi'] == 0 and r['finish'] in (FINISH_INTERLEAVE_ROWS, FINISH_STRIDED_JOIN)]
    finishes = [r['finish'] for r in classes]
    # two strided blocks, two steps: per block and step the downsample conv's interleave and, ResNet-18, conv 0's -- ResNet-50, the 3x3's join
    if model == 'resnet18':
        assert finishes.count(FINISH_INTERLEAVE_ROWS) == 8 and FINISH_STRIDED_JOIN not in finishes, log
    else:
        assert finishes.count(FINISH_INTERLEAVE_ROWS) == 4 and finishes.count(FINISH_STRIDED_JOIN) == 4, log
