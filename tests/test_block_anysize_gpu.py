"""The residual-block executor at any map width (ops.block_any / p3d_block_any_enable): dense blocks whose convolutions all have stride 1, at maps the aligned
kernels refuse, through p3d_block_fwd / p3d_block_bwd on the ragged image-fed instances.

Whole blocks: tests/test_block_gpu.py::fused_block_case unchanged -- usable(...) == admitted, the fused result differs in bits from the per-layer one, both within
the project's bounds of float64 (2e-5 element-wise on y, 2e-5 / 2e-3 on dx, 4x that on parameter gradients, 1e-5 on running statistics).  Then what stays on the
per-layer path with the switch on, an aligned block launch for launch, reproducibility, fenced exact-size buffers and a two-step network at side 33.

The two new conv instances alone (INSTANCE_CASES; tests/test_block_anysize_host.py fails when p3d_fx_conv_any_sums_instances reports an instance none of them names):
through p3d_fx_conv_fused with ragged = 1, an fx_act_image_any operand and `partial`.  The result must be bit-equal to the same call without `partial` -- that call
forced unsplit (p3d_fx_tune(1, 1)), as a launch with sums always is: split-K sums its slabs in another order.  The sums, added over rows in float64, are held per
channel to the bound of tests/test_fx_instances_gpu.py for an unsplit launch: pixels * X3_TOL * max|summand| + 128 * 2^-24 * sum|summand|.

The image passes of modes 1 and 2 at any HW (p3d_fx_act_image_fused, any = 1) against the aligned pass (any = 0) on the same values padded to an aligned HW, from the
table and from each finalize kind on the same partial sums: the same piece bytes for the pixels that exist, the same constants written out."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import fenced
from test_block_gpu import CASES, build, fused_block_case, make_case, run
from test_kernels_gpu import X3_TOL

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(os.environ.get('P3D_X3', '1') == '0', reason='the block executor needs the x3 kernels')]

U = 2.0 ** -24
MARGIN = 1e-3

#               kind          inplanes planes stride dil  N  H[xW]   downsample
RAGGED_CASES = [('bottleneck', 256, 64, 1, 1, 3, 5, False),           # NP = 75: one partial tile, groups straddling images, HW = 1 mod 4
                ('bottleneck', 64, 64, 1, 1, 2, (7, 9), True),        # HW = 63 = 3 mod 4, non-square, stride-1 downsample
                ('basic', 64, 64, 1, 1, 4, (6, 7), False),            # HW = 42 = 2 mod 4
                ('basic', 128, 128, 1, 1, 5, 9, False),               # NP = 405: four tiles, the last of 21 pixels
                ('bottleneck', 256, 128, 1, 2, 2, 17, True),          # the layer4.0 pattern, dilation 2
                ('bottleneck', 64, 64, 1, 1, 16, 65, True)]           # 529 partial rows > FX_FIN_MAX_ROWS: the finalize launches instead of the prologues
STAYS_OUT = [('bottleneck', 256, 128, 2, 1, 2, 33, True)]             # a stride-2 block at 33 x 33: the per-layer path, as ever


def _id(c):
    h = c[6] if isinstance(c[6], int) else '%dx%d' % c[6]
    return '%s_c%d_p%d_s%d_d%d_n%d_h%s%s' % (c[0], c[1], c[2], c[3], c[4], c[5], h, '_ds' if c[7] else '')


@pytest.fixture
def block_any(pkg):
    """the switch on for the test body; restored, with the forced split counts, afterwards"""
    before = pkg.ops.block_any(True)
    try:
        yield pkg.ops.block_any
    finally:
        pkg.ops.block_any(before)
        pkg._lib.lib().p3d_fx_tune(1, 0)


@pytest.mark.parametrize('case', RAGGED_CASES, ids=_id)
def test_ragged_block_matches_per_layer_path_and_float64(case, pkg, block_any):
    fused_block_case(pkg, *case)


@pytest.mark.parametrize('case', RAGGED_CASES[:2], ids=_id)
def test_ragged_blocks_stay_out_with_the_switch_off(case, pkg, block_any):
    block_any(False)
    block, x0, _, _ = make_case(pkg, *case, want_clean=False)
    assert not pkg.ops_block.usable(block, x0)


@pytest.mark.parametrize('case', STAYS_OUT, ids=_id)
def test_strided_blocks_at_odd_maps_stay_on_the_per_layer_path(case, pkg, block_any):
    fused_block_case(pkg, *case, admitted=False)


def test_masked_blocks_at_odd_maps_stay_on_the_per_layer_path(pkg, block_any):
    """a block of partial convolutions at 17 x 17 with the switch on: refused, so forward and backward with the executor allowed and forbidden are the same per-layer
    nodes -- no ResidualBlockFn, every result (output, veil, input gradient, parameter gradients, running statistics) bit-equal and finite.  (The yardstick of a masked
    block in tests/test_block_gpu.py is the per-layer path itself, which the reference's goldens pin; masked_block_case asserts usable(...) and cannot take this shape.)"""
    tr = pkg._trunk
    torch.manual_seed(5)
    block = tr.Bottleneck(256, 64, 1, 1, None, partial=True).cuda().train()
    gen = torch.Generator(device='cuda').manual_seed(6)
    x0 = torch.randn(2, 256, 17, 17, device='cuda', generator=gen).relu_()
    veil = (torch.rand(2, 1, 17, 17, device='cuda', generator=gen) > 0.3).float()
    veil[0, 0, :5, :7] = 0.0
    assert not pkg.ops_block.usable(block, x0, veil)
    dy = torch.randn(2, 256, 17, 17, device='cuda', generator=gen)
    got = []
    for fused in (False, True):
        before = pkg._trunk.FUSED_BLOCKS
        pkg._trunk.FUSED_BLOCKS = fused
        try:
            state = {k: v.clone() for k, v in block.state_dict().items()}
            block.zero_grad(set_to_none=True)
            x = x0.clone().requires_grad_(True)
            y, vo = block((x, veil))
            assert not type(y.grad_fn).__name__.startswith('ResidualBlockFn')
            y.backward(dy)
            pkg.ops.join_side_stream()
            torch.cuda.synchronize()
            got.append([y.detach().clone(), vo.clone(), x.grad.clone()] + [p.grad.clone() for p in block.parameters()] +
                       [v.clone() for k, v in block.state_dict().items() if 'running' in k])
            block.load_state_dict(state)
        finally:
            pkg._trunk.FUSED_BLOCKS = before
    assert len(got[0]) == len(got[1]) > 10
    for a, b in zip(*got):
        assert torch.isfinite(a).all() and torch.equal(a, b)


def _log(pkg):
    return pkg.ops.fx_launch_log(reset=True)[0]


def test_aligned_blocks_launch_what_they_always_did(pkg, block_any):
    """an aligned case: the same bits and the same launch log with the switch on and off"""
    block, x0, dy, _ = make_case(pkg, *CASES[0], want_clean=False)
    got = {}
    for on in (False, True):
        block_any(on)
        assert pkg.ops_block.usable(block, x0)
        _log(pkg)
        res = run(pkg, block, x0, dy, fused=True)
        got[on] = (res, _log(pkg))
    (a, log_a), (b, log_b) = got[False], got[True]
    assert log_a == log_b and len(log_a) > 0 and all(r['rag'] == 0 for r in log_a)
    assert torch.equal(a['y'], b['y']) and torch.equal(a['dx'], b['dx'])
    for k in a['grads']:
        assert torch.equal(a['grads'][k], b['grads'][k]), k
    for k in a['buffers']:
        assert torch.equal(a['buffers'][k], b['buffers'][k]), k


def _same(a, b):
    return (torch.equal(a['y'], b['y']) and torch.equal(a['dx'], b['dx']) and all(torch.equal(a['grads'][k], b['grads'][k]) for k in a['grads'])
            and all(torch.equal(a['buffers'][k], b['buffers'][k]) for k in a['buffers']))


def test_ragged_block_is_bitwise_reproducible_and_launches_the_new_instances(pkg, block_any):
    block, x0, dy, _ = make_case(pkg, *RAGGED_CASES[1], want_clean=False)
    assert pkg.ops_block.usable(block, x0)
    _log(pkg)
    first = run(pkg, block, x0, dy, fused=True)
    log = _log(pkg)
    second = run(pkg, block, x0, dy, fused=True)
    assert _same(first, second)
    assert all(r['rag'] == 1 and r['amode'] == 1 and r['kernel'] == 0 for r in log), log
    # forward: four convolutions (downsample included) with the statistics; backward: two data gradients with the backward sums, two plain ones (conv 0, downsample)
    assert sorted(r['epi'] for r in log) == [0, 0, 1, 1, 1, 1, 2, 2], log
    assert all(r['grid_y'] == 1 and r['kchunk'] == 0 for r in log if r['epi'] != 0), log


def test_exact_size_fenced_buffers(pkg, block_any):
    """every tensor the executor's Python side allocates (conv outputs, the plane images -- that of x among them --, tables, gradient images and gradients, the result)
    at exactly its size, poisoned, between fences: the bands must stay as they were, and the results must be those of an ordinary run, bit for bit"""
    case = RAGGED_CASES[1]
    block, x0, dy, _ = make_case(pkg, *case, want_clean=False)
    plain = run(pkg, block, x0, dy, fused=True)
    block2, _, _, _ = make_case(pkg, *case, want_clean=False)                # the same module again,
    assert pkg.ops_block.release_buffers(block2) > 0                         #   its plan and buffers to be made inside the fences
    with fenced.FencedAllocations() as fa:
        got = run(pkg, block2, x0, dy, fused=True)
        pkg.ops.join_side_stream()
        torch.cuda.synchronize()
    fa.check()
    assert len(fa.fences) > 10
    assert _same(plain, got)
    assert all(torch.isfinite(v).all() for v in [got['y'], got['dx']] + list(got['grads'].values()))


def test_two_steps_of_resnet18_at_side_33(pkg, block_any):
    """a two-step depthnet ResNet-18 at side 33: 9 x 9 maps behind the stem, then 5 x 5 and 3 x 3 -- layer1's two blocks are ragged blocks, the rest stays per-layer;
    the loss is finite and the launch log shows the new instances"""
    import test_step_gpu as S
    meta = {'model': 'resnet18', 'side': 33, 'extra': []}
    args, model, trainer = S.build(pkg, meta)
    model.train()
    trainer.adapt_learn_rate(1)
    c, d, tc, tv = pkg.synth.make_batch(2, side=33, rank=0, step=0)
    batch = (torch.from_numpy(c).cuda(), None, torch.from_numpy(tc).cuda(), torch.from_numpy(tv).cuda())
    _log(pkg)
    losses = []
    for _ in range(2):
        losses.append(float(trainer.train_step(*batch)))
    pkg.ops.join_side_stream()
    torch.cuda.synchronize()
    log = _log(pkg)
    assert all(l == l and abs(l) < float('inf') for l in losses), losses
    new = [r for r in log if r['rag'] == 1 and r['amode'] == 1 and r['epi'] in (1, 2)]
    assert {r['epi'] for r in new} == {1, 2}, log


# ---- the two instances alone ---------------------------------------------------------------------------------------------------------------------------------
#                  name                  pass    instance record (kernel, amode, pro, epi, tapi, rag, rows)   n  c    k    h  w  r
INSTANCE_CASES = [('any_stats_1x1', 'fwd', (0, 1, 0, 1, 0, 1, 0), 3, 64, 64, 5, 5, 1),
                  ('any_stats_3x3', 'fwd', (0, 1, 0, 1, 0, 1, 0), 5, 128, 192, 7, 9, 3),
                  ('any_bwd_sums_1x1', 'dgrad', (0, 1, 0, 2, 0, 1, 0), 3, 64, 64, 5, 5, 1),
                  ('any_bwd_sums_3x3', 'dgrad', (0, 1, 0, 2, 0, 1, 0), 5, 128, 192, 7, 9, 3),
                  ('any_bwd_sums_mask_switch', 'dgrad', (0, 1, 0, 2, 0, 1, 0), 3, 64, 64, 5, 5, 1)]      # the mask switches inside a four-pixel group that crosses an image
FIELDS = ('kernel', 'amode', 'pro', 'epi', 'tapi', 'rag', 'rows')


@pytest.mark.parametrize('case', INSTANCE_CASES, ids=[c[0] for c in INSTANCE_CASES])
def test_instance_alone(case, pkg, block_any):
    name, pass_, inst, n, c, k, h, w, r = case
    ops, L = pkg.ops, pkg._lib.lib()
    dg = pass_ == 'dgrad'
    pad = r // 2
    gen = torch.Generator(device='cuda').manual_seed(3000 + [q[0] for q in INSTANCE_CASES].index(name))
    wt = torch.randn(k, c, r, r, device='cuda', generator=gen) / ((k if dg else c) * r * r) ** 0.5
    src = torch.randn(n, k if dg else c, h, w, device='cuda', generator=gen)
    core = torch.nn.grad.conv2d_input((n, c, h, w), wt.double(), src.double(), 1, pad, 1) if dg else F.conv2d(src.double(), wt.double(), None, 1, pad, 1)
    shape = tuple(core.shape)
    m, hw = shape[1], h * w
    d = ops._desc((n, c, h, w), (k, c, r, r), 1, pad, 1)
    dref = ctypes.byref(d)
    f = pkg._lib.FxFuse()
    image = ops.act_image(src)                                      # (HW no multiple of 4: p3d_fx_act_image_any)
    assert hw % 4 != 0
    f.act_img, f.ragged = ops._p(image), 1
    c2 = tab = None
    if dg:
        tab = torch.full((m, 8), float('nan'), device='cuda')
        tab[:, 0], tab[:, 1], tab[:, 2] = torch.rand(m, device='cuda', generator=gen) + 0.5, torch.randn(m, device='cuda', generator=gen) * 0.5, torch.randn(m, device='cuda', generator=gen) * 0.3
        sc, sh, mean = (tab[:, i].double().view(1, -1, 1, 1) for i in range(3))
        c2 = torch.randn(*shape, device='cuda', generator=gen).double()
        if name.endswith('mask_switch'):
            # flat pixels 24 .. 27 of every channel are one lane's group: the last pixel of image 0 passes, the first two of image 1 do not, the third does
            z = c2 * sc + sh
            flat = z.permute(1, 0, 2, 3).reshape(m, n * hw)
            assert hw == 25
            flat[:, 24], flat[:, 25], flat[:, 26], flat[:, 27] = flat[:, 24].abs() + 0.1, -flat[:, 25].abs() - 0.1, -flat[:, 26].abs() - 0.1, flat[:, 27].abs() + 0.1
            c2 = (flat.reshape(m, n, h, w).permute(1, 0, 2, 3) - sh) / sc
        z = c2 * sc + sh
        away = (z >= 0).double() * (4 * MARGIN) - 2 * MARGIN
        c2 = torch.where(z.abs() < 2 * MARGIN, (away - sh) / sc, c2).float().contiguous()
        z = c2.double() * sc + sh
        assert z.abs().min().item() >= MARGIN and (z > 0).any() and (z < 0).any()
        if name.endswith('mask_switch'):
            zf = (z > 0).permute(1, 0, 2, 3).reshape(m, n * hw)
            assert zf[:, 24].all() and not zf[:, 25].any() and not zf[:, 26].any() and zf[:, 27].all()
        g = core * (z > 0)
        sums = [g, g * (c2.double() - mean)]
        f.ep_c, f.ep_tab = ops._p(c2), ops._p(tab)
    else:
        sums = [core, core * core]
    nbytes = L.p3d_fx_conv_fused_workspace_bytes(int(dg), dref, 1)
    assert nbytes > 0
    prows = L.p3d_fx_conv_fused_partial_rows_any(int(dg), dref)
    pixels = n * hw
    assert prows == -(-pixels // 128)
    ws = fenced.Fence(nbytes, 4096, 'cuda')

    def call(with_sums):
        out, fence = fenced.fenced_like(shape, torch.float32, 4096)
        partial, pfence = fenced.fenced_like((prows, m, 2), torch.float32, 4096)
        f.partial = ops._p(partial) if with_sums else None
        ops.fx_launch_log(reset=True)
        rc = L.p3d_fx_conv_fused(int(dg), dref, ctypes.byref(f), None, ops._p(wt), None, ops._p(out), ops._p(ws.view), nbytes, ops._stream())
        torch.cuda.synchronize()
        records = ops.fx_launch_log(reset=True)[0]
        assert rc == 0, L.p3d_last_error()
        fence.check('%s result' % name)
        pfence.check('%s partial sums' % name)
        ws.check('%s workspace' % name)
        return out, partial, records

    out, partial, records = call(True)
    assert len(records) == 1 and tuple(records[0][q] for q in FIELDS) == inst and records[0]['grid_y'] == 1 and records[0]['kchunk'] == 0, records
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
    for i, s in enumerate(sums):
        ref, ref_abs, ref_max = s.sum((0, 2, 3)), s.abs().sum((0, 2, 3)), s.abs().max().item()
        bound = pixels * X3_TOL * ref_max + 128 * U * ref_abs
        diff = (mine[:, i] - ref).abs()
        print('SUM %s [%d] worst |diff| / bound %.3g' % (name, i, (diff / bound).max().item()))
        assert bool((diff <= bound).all()), (name, i, (diff / bound).max().item())


# ---- the image passes ----------------------------------------------------------------------------------------------------------------------------------------
IMAGE_SHAPES = [(3, 32, 25), (2, 64, 63)]
IMAGE_VARIANTS = [(1, 0), (1, 1), (2, 0), (2, 2), (2, 3)]           # (mode, finalize kind; 0: the constants come from the table)


def _planes(img, n, c, hw):
    return img.view(torch.int16).view(3, n, c // 16, hw, 16)


@pytest.mark.parametrize('mode,kind', IMAGE_VARIANTS, ids=['mode%d_fin%d' % v for v in IMAGE_VARIANTS])
@pytest.mark.parametrize('shape', IMAGE_SHAPES, ids=['n%d_c%d_hw%d' % s for s in IMAGE_SHAPES])
def test_image_pass_matches_the_aligned_pass(shape, mode, kind, pkg):
    ops, L = pkg.ops, pkg._lib.lib()
    n, c, hw = shape
    hwp = (hw + 3) // 4 * 4
    gen = torch.Generator(device='cuda').manual_seed(100 * hw + 10 * mode + kind)
    rn = lambda *s: torch.randn(*s, device='cuda', generator=gen)
    x, x2 = rn(n, c, hw), rn(n, c, hw)
    pad = lambda t: torch.cat([t, rn(n, c, hwp - hw)], 2).contiguous()      # (what lies in the padding is the aligned pass's own business)
    xp, x2p = pad(x), pad(x2)
    count = float(n * hw)
    table = torch.zeros(c, 8, device='cuda')
    table[:, 0], table[:, 1], table[:, 2], table[:, 3] = torch.rand(c, device='cuda', generator=gen) + 0.5, rn(c) * 0.3, rn(c) * 0.2, torch.rand(c, device='cuda', generator=gen) + 0.5
    table[:, 4], table[:, 5], table[:, 6] = rn(c), rn(c) * 0.1, rn(c) * 0.1
    gamma, beta = torch.rand(c, device='cuda', generator=gen) + 0.5, rn(c) * 0.3
    rows = 5
    if kind == 1:
        partial = torch.stack([rn(rows, c) * count * 0.05, (torch.rand(rows, c, device='cuda', generator=gen) + 0.5) * count / rows], 2).contiguous()
    elif kind == 2:
        partial = (rn(rows, c, 2) * count * 0.01).contiguous()
    else:
        partial = (rn(c, rows, 3) * count * 0.01).double().contiguous()
    masked = int(mode == 2 and kind != 3)
    got = []
    for any_, xx, xx2, h in ((1, x, x2, hw), (0, xp, x2p, hwp)):
        img = torch.full((6 * n * c * h,), 0x5A, dtype=torch.uint8, device='cuda')
        tab = table.clone()
        rm, rv = torch.linspace(-1, 1, c, device='cuda'), torch.linspace(0.5, 1.5, c, device='cuda')
        dgam, dbet = torch.full((c,), float('nan'), device='cuda'), torch.full((c,), float('nan'), device='cuda')
        rc = L.p3d_fx_act_image_fused(any_, mode, ops._p(xx), ops._p(xx2) if mode == 2 else None, ops._p(tab), masked, ops._p(img), n, c, h, kind, ops._p(partial), rows,
                                      1 if kind == 3 else 0, count, ops._p(gamma), ops._p(beta), ops._p(rm), ops._p(rv), 0.1, 1e-5, ops._p(dgam), ops._p(dbet), 0, ops._stream())
        torch.cuda.synchronize()
        assert rc == 0, L.p3d_last_error()
        got.append((_planes(img, n, c, h), tab, rm, rv, dgam, dbet))
    (a, *consts_a), (b, *consts_b) = got
    assert torch.equal(a, b[:, :, :, :hw]), 'piece bytes differ'
    for u, v in zip(consts_a, consts_b):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))                          # the constants written out (NaN where nothing writes) are the same bits
    if kind == 1:
        assert not torch.equal(consts_a[0], table) and torch.isfinite(consts_a[0]).all()      # the table was written from the partials
    if kind in (2, 3):
        assert torch.isfinite(consts_a[3]).all() and torch.isfinite(consts_a[4]).all()
