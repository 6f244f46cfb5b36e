"""The table of tests/test_x3_wgrad_instances_gpu.py, checked without a GPU: it is well formed; under each row's p3d_fx_tune settings the library's own planner
(p3d_fx_wgrad_plan, host-only) answers exactly fields [0..15] of the row's record; the records name between them EVERY compiled weight-gradient kernel (the two X-macros
of csrc/p3d_fx.hip, read as tests/test_wgrad_plan_host.py reads them) and every finishing combination of wgrad_finish and the stem; the finishing bits each record
names are the ones wgrad_finish's rules give for the row's slabs and destination (spelled out here a second time, in Python); and the rows cover both block orders, slab
counts of 1, 2..16 and above 16, and an uneven last slab in every kernel family.  The library is loaded for host-only queries; nothing is launched.

The names and the length of the record exist in the header (P3D_FX_WGRAD_LAUNCH_FIELDS, P3D_FX_WGRAD_PLAN_FIELDS), in ops.FX_WGRAD_LAUNCH_FIELDS and in Rec of the table:
held to each other here, with the struct of the hook."""
import ctypes
import os
import re

import pytest

import x3_wgrad_table as T
from x3_wgrad_table import ROWS


def conv_out(h, k, stride, pad, dil):
    return (h + 2 * pad - dil * (k - 1) - 1) // stride + 1


def desc(pkg, row):
    win = 'win' in row.opts
    return pkg.ops._desc((row.n, row.c, row.h, row.w), (row.k, row.c, row.r, row.r), row.stride, row.pad, row.dil, c_offset=T.WINDOW_OFFSET if win else 0,
                         c_total=row.c + T.WINDOW_EXTRA if win else row.c, accumulate=int('acc' in row.opts))


def pixels(row):
    """N * Ho * Wo: the length of the reduction"""
    return row.n * conv_out(row.h, row.r, row.stride, row.pad, row.dil) * conv_out(row.w, row.r, row.stride, row.pad, row.dil)


def steps(row):
    """K steps of 16 pixels: whole steps of one image on aligned maps, of the flat pixel index (the last one partial) at any map width"""
    ho, wo = conv_out(row.h, row.r, row.stride, row.pad, row.dil), conv_out(row.w, row.r, row.stride, row.pad, row.dil)
    return -(-row.n * ho * wo // 16) if 'rag' in row.opts else row.n * (ho * wo // 16)


@pytest.fixture()
def lib(pkg):
    """the library with the x3 kernels on; the split rule is put back afterwards"""
    L = pkg._lib.lib()
    was = L.p3d_x3_enable(1)
    try:
        yield L
    finally:
        L.p3d_fx_tune(0, 0)
        L.p3d_x3_enable(was)


def test_the_table_is_well_formed():
    assert len({r.name for r in ROWS}) == len(ROWS) and T.UNREACHABLE == ()
    for r in ROWS:
        o = set(r.opts)
        assert r.entry in ('hook', 'stem', 'stem_masked') and o <= set(T.OPTIONS) and len(o) == len(r.opts), r.name
        assert all(what == 0 and value >= 1 for what, value in r.tune) and len(r.tune) <= 1 and isinstance(r.rec, T.Rec), r.name
        assert conv_out(r.h, r.r, r.stride, r.pad, r.dil) >= 1 and conv_out(r.w, r.r, r.stride, r.pad, r.dil) >= 1 and r.stride in (1, 2), r.name
        assert pixels(r) <= T.MAX_TERMS, r.name
        assert 0 <= T.operand_bits(r) < 128, r.name                                        # the bits p3d_fx_wgrad_plan takes
        assert r.rec.accumulate == int('acc' in o) and r.rec.finish in T.FINISH_NAMES, r.name
        assert not ({'win', 'dwoff'} <= o) and ('rows' not in o or 'dyimg' in o) and ('ximg' not in o or 'dyimg' in o), r.name
        if r.entry != 'hook':
            assert o <= {'acc'} and not r.tune and (r.r, r.stride, r.pad, r.dil) == (7, 2, 3, 1) and r.rec.finish == T.STEM_DW, r.name
        # an image carries its factor: the record's instance is the masked one only where an fp32 operand has a factor left
        if r.entry == 'hook' and 'rag' not in o:
            assert (r.rec.aimg, r.rec.bimg, r.rec.rows) == (int('dyimg' in o), int('ximg' in o), int('rows' in o)), r.name
            assert r.rec.masked == int(('pm' in o and 'dyimg' not in o) or ('em' in o and 'ximg' not in o)), r.name
        assert 4 * max(r.n * r.c * r.h * r.w, r.n * r.k * pixels(r) // r.n, r.k * (r.c + T.WINDOW_EXTRA) * r.r * r.r) <= 16 << 20, r.name      # tiny operands
        assert r.rec.slab_bytes_hi == 0 and r.rec.slab_bytes_lo <= 16 << 20, r.name


def test_the_record_layout_is_the_same_everywhere(pkg):
    header = open(pkg._lib.HEADER_PATH).read()
    plan_len = int(re.search(r'#define P3D_FX_WGRAD_PLAN_FIELDS (\d+)', header).group(1))
    launch_len = int(re.search(r'#define P3D_FX_WGRAD_LAUNCH_FIELDS (\d+)', header).group(1))
    names = pkg.ops.FX_WGRAD_LAUNCH_FIELDS
    assert names == T.Rec._fields and launch_len == pkg.ops.FX_WGRAD_LAUNCH_LEN >= len(names) == plan_len + 2
    assert names[plan_len:] == ('finish', 'accumulate')
    src_dir = os.path.join(os.path.dirname(os.path.abspath(pkg._lib.__file__)), 'csrc')
    src = open(os.path.join(src_dir, 'p3d_fx.hip')).read()
    assert re.search(r'enum \{ FXWL_FINISH = P3D_FX_WGRAD_PLAN_FIELDS, FXWL_ACCUMULATE, FXWL_FIELDS = P3D_FX_WGRAD_LAUNCH_FIELDS \}', src)
    assert int(re.search(r'constexpr int32_t FX_WGRAD_FIN_STEM = (\d+);', src).group(1)) == T.STEM_DW
    fin = re.search(r'enum \{ FIN_FWD_REDUCE = 1,(.*?)\};', open(os.path.join(src_dir, 'p3d_conv.hip')).read(), re.S).group(1)
    bits = {m.group(1): int(m.group(2)) for m in re.finditer(r'FIN_(\w+) = (\d+)', fin)}
    assert (bits['WGRAD_REDUCE'], bits['WGRAD_REDUCE_TAPM'], bits['WGRAD_REDUCE16'], bits['WGRAD_REDUCE16_TAPM'], bits['SLAB_FOLD']) == \
        (T.REDUCE, T.REDUCE_TAPM, T.REDUCE16, T.REDUCE16_TAPM, T.SLAB_FOLD)
    # the struct of the hook: the header's fields in the header's order, pointers first
    body = re.search(r'typedef struct p3d_fx_wgrad_fuse \{(.*?)\} p3d_fx_wgrad_fuse;', header, re.S).group(1)
    fields = []
    for line in body.split(';'):
        line = line.strip()
        if line.startswith('int32_t '):
            fields += [(n.strip(), ctypes.c_int32) for n in line[len('int32_t '):].split(',')]
        elif line:
            assert '*' in line, line
            fields.append((line.split('*')[-1].strip(), ctypes.c_void_p))
    assert fields == list(pkg._lib.FxWgradFuse._fields_) and [f for f, _ in fields] == ['dy_img', 'x_img', 'pmask', 'emask', 'rows', 'ragged']


def test_every_rows_plan_is_the_planners(lib, pkg):
    for r in ROWS:
        d = desc(pkg, r)
        for what, value in r.tune:
            lib.p3d_fx_tune(what, value)
        try:
            out = (ctypes.c_int32 * 16)()
            rc = lib.p3d_fx_wgrad_plan(ctypes.byref(d), T.operand_bits(r), out)
            nbytes = None
            if r.entry == 'hook':
                f = pkg._lib.FxWgradFuse()
                # (the query looks at which operands are set, never through them)
                f.dy_img, f.x_img = int('dyimg' in r.opts) * 16, int('ximg' in r.opts) * 16
                f.pmask, f.emask = int('pm' in r.opts and 'dyimg' not in r.opts) * 16, int('em' in r.opts and 'ximg' not in r.opts) * 16
                f.rows, f.ragged = int('rows' in r.opts), int('rag' in r.opts)
                nbytes = lib.p3d_fx_conv_wgrad_fused_workspace_bytes(ctypes.byref(d), ctypes.byref(f))
        finally:
            lib.p3d_fx_tune(0, 0)
        assert rc == 0, (r.name, lib.p3d_last_error())
        assert tuple(out) == tuple(r.rec[:16]), (r.name, tuple(out))
        # what the record says, from the rules: the slabs cover the K steps, the last one not empty; the slab bytes; the grid
        q, rs = r.rec, r.r * r.r
        if r.entry == 'hook':
            assert nbytes == q.slab_bytes_lo == q.splits * r.k * r.c * rs * 4, r.name
            assert q.splits * q.spb >= steps(r) > (q.splits - 1) * q.spb, r.name
            assert q.tapm == int(rs > 1) and q.order == int(rs > 1 and r.c >= 512) and q.tile_taps == q.taps, r.name
            if q.taps:
                assert (q.grid_x, q.grid_y, q.grid_z) == (-(-rs // q.taps), -(-r.k // 128), q.splits), r.name
                assert r.c == 64 and q.taps == (3 if r.k <= 64 else 2), r.name
            else:
                assert (q.grid_x, q.grid_y, q.grid_z) == (-(-r.c // 128), -(-r.k // 128), q.splits * rs), r.name
        else:
            total = r.n * ((r.h // 2) * (r.w // 2) // 16)
            assert q.splits * q.spb >= total > (q.splits - 1) * q.spb and q.slab_bytes_lo == q.splits * r.k * 256 * 4, r.name
            assert (q.grid_x, q.grid_y, q.grid_z, q.tile_taps, q.taps) == (2, -(-r.k // 128), q.splits, 8, 1), r.name
            assert lib.p3d_stem_supported(r.n, r.c, r.h, r.w, r.k) == 1, r.name


def test_every_compiled_instance_is_named(pkg):
    src = open(os.path.join(os.path.dirname(os.path.abspath(pkg._lib.__file__)), 'csrc', 'p3d_fx.hip')).read()
    body = re.search(r'#define P3D_FX_WGRAD_INSTANCES\(X\)(.*?)\n#define P3D_FX_WGRAD_ANY_INSTANCES\(X\)(.*?)\n', src, re.S)
    compiled = [(T.ALIGNED,) + tuple(int(v) for v in m) for m in re.findall(r'X\((\d), (\d), (\d), (\d), (\d)\)', body.group(1))]
    families = dict(FX_WG_ANY=T.ANY, FX_WG_ANY_MASKED=T.ANY_MASKED, FX_WG_ANY_IMG=T.ANY_IMG)
    compiled += [(families[m], 0, 0, 0, 0, 0) for m in re.findall(r'X\((FX_WG_\w+), \w+\)', body.group(2))]
    assert len(compiled) == len(set(compiled)) == 16 and len([c for c in compiled if c[0] == T.ALIGNED]) == 13
    named = {T.instance(r.rec) for r in ROWS}
    barred = {inst for inst, why in T.UNREACHABLE}
    assert not (barred & named)
    missing = set(compiled) - named - barred
    assert not missing, 'compiled weight-gradient kernels no row reaches: ' + ', '.join(sorted(T.instance_name(i) for i in missing))
    unknown = (named | barred) - set(compiled)
    assert not unknown, 'rows expect kernels that are not compiled: ' + ', '.join(sorted(T.instance_name(i) for i in unknown))


def finish_by_the_rules(r):
    """wgrad_finish (csrc/p3d_conv.hip) for the row's slabs and destination, a second time"""
    q, rs = r.rec, r.r * r.r
    if r.entry != 'hook':
        return T.STEM_DW
    tapm, bits = bool(q.tapm) and rs > 1, 0
    if q.splits > 16:
        if tapm and r.c % 16 == 0 and 17 * rs * 16 * 4 <= 64 * 1024:
            return T.REDUCE16_TAPM
        contiguous = 'win' not in r.opts and (r.k * r.c * rs) % 4 == 0 and 'dwoff' not in r.opts                # (ldw == Ncols, woff == 0, a 16-B line)
        if not tapm and contiguous:
            return T.REDUCE16
        bits = T.SLAB_FOLD
    return bits | (T.REDUCE_TAPM if tapm else T.REDUCE)


def test_finishing_passes_slabs_and_orders_are_covered():
    for r in ROWS:
        assert r.rec.finish == finish_by_the_rules(r), (r.name, T.FINISH_NAMES[r.rec.finish])
    assert {r.rec.finish for r in ROWS} == set(T.FINISH_NAMES)
    hook = [r for r in ROWS if r.entry == 'hook']
    assert {r.rec.order for r in hook} == {0, 1}
    assert [r for r in hook if r.rec.order == 1 and r.rec.splits > 1] and [r for r in hook if r.rec.order == 1 and r.rec.aimg] and \
        [r for r in hook if r.rec.order == 1 and not r.rec.aimg]
    for lo, hi in ((1, 1), (2, 16), (17, 1 << 30)):
        assert [r for r in ROWS if lo <= r.rec.splits <= hi], (lo, hi)
    for family in (T.ALIGNED, T.ANY, T.ANY_MASKED, T.ANY_IMG):                             # a last slab shorter than the others
        assert [r for r in hook if r.rec.family == family and r.rec.splits > 1 and steps(r) % r.rec.spb], family
    for taps in (2, 3):                                                                    # the multi-tap tiles: a split with an uneven slab (3), deep slabs (2)
        assert [r for r in hook if r.rec.taps == taps and r.rec.splits > 1], taps
    # more than 16 slabs into each finishing pass that takes them, fp32- and image-fed
    assert {r.rec.finish for r in hook if r.rec.splits > 16} == {T.REDUCE16, T.REDUCE16_TAPM, T.SLAB_FOLD | T.REDUCE, T.SLAB_FOLD | T.REDUCE_TAPM}
    assert [r for r in hook if r.rec.splits > 16 and r.rec.aimg] and [r for r in hook if r.rec.splits > 16 and r.rec.taps]
    # grids whose size is and is not a multiple of the eight XCDs
    sizes = {(r.rec.grid_x * r.rec.grid_y * r.rec.grid_z) % 8 == 0 for r in hook}
    assert sizes == {True, False}


def test_every_edge_of_the_family_is_named():
    def where(has=(), lacks=(), **rec):
        return [r for r in ROWS if set(has) <= set(r.opts) and not (set(lacks) & set(r.opts)) and all(getattr(r.rec, f) == v for f, v in rec.items())]
    # partial tiles: output channels past row + 64 of a tile and past a tile; a partial channel group of an image operand's tile; fp32 x off the steps of 16
    assert [r for r in where(family=T.ALIGNED, aimg=0) if r.k % 128 > 64 and r.c % 128] and [r for r in where(aimg=1, bimg=1, taps=0) if r.k % 128 and r.c % 128 and r.k > 128]
    assert [r for r in where(aimg=1, bimg=0) if r.c % 16]
    # multi-tap column tiles with a dead last tap: 25 taps in threes, 9 and 25 taps in twos
    assert [r for r in where(taps=3) if (r.r * r.r) % 3] and {(r.r * r.r) % 2 for r in where(taps=2)} == {1}
    assert [r for r in where(taps=3) if r.k < 64] and [r for r in where(taps=2) if r.k > 128]
    assert where(taps=3, rows=1) and where(taps=2, rows=1)
    # any map width: a partial last step, fewer pixels than one step, 5x7 and 9x9 maps, and an aligned map
    rag = where(has=('rag',))
    assert {(r.h, r.w) for r in rag} >= {(5, 7), (9, 9), (3, 5), (8, 8)} and [r for r in rag if pixels(r) < 16] and [r for r in rag if pixels(r) % 16]
    assert [r for r in rag if r.stride == 2]
    # factors: both on fp32 operands, x alone beside a dy image, each with a split and with accumulate
    for sel in (dict(family=T.ALIGNED, aimg=0, masked=1), dict(family=T.ALIGNED, aimg=1, masked=1), dict(family=T.ANY_MASKED)):
        mine = where(**sel)
        assert [r for r in mine if r.rec.splits > 1] and [r for r in mine if 'acc' in r.opts] and {r.r for r in mine} >= {1, 3}, sel
    # geometry: stride 2 (1x1 and 3x3), dilation, a 5x5, non-square maps
    assert {(r.r, r.stride) for r in ROWS} >= {(1, 2), (3, 2)} and [r for r in ROWS if r.dil == 2] and [r for r in ROWS if r.r == 5] and [r for r in ROWS if r.h != r.w]
    # result placement
    assert where(has=('acc',), splits=1) and [r for r in where(has=('acc',)) if r.rec.splits > 1]
    assert where(has=('win',), splits=1) and where(has=('win', 'acc')) and where(has=('dwoff',))
    # the stem: RGB and depth, a K that leaves a partial group of 64, two slabs, masked
    stems = [r for r in ROWS if r.entry != 'hook']
    assert {r.c for r in stems} >= {1, 3} and [r for r in stems if r.k % 64] and [r for r in stems if r.rec.splits == 2] and [r for r in stems if r.rec.masked]


def test_the_hooks_query_refuses_what_the_hook_refuses(pkg, lib):
    f = pkg._lib.FxWgradFuse()
    good = pkg.ops._desc((2, 32, 8, 8), (64, 32, 1, 1), 1, 0, 1)
    assert lib.p3d_fx_conv_wgrad_fused_workspace_bytes(ctypes.byref(good), ctypes.byref(f)) == 64 * 32 * 4
    assert lib.p3d_fx_conv_wgrad_fused_workspace_bytes(ctypes.byref(good), None) == 0 and lib.p3d_fx_conv_wgrad_fused_workspace_bytes(None, ctypes.byref(f)) == 0
    for bad in (pkg.ops._desc((2, 16, 8, 8), (64, 16, 1, 1), 1, 0, 1),                     # fewer than 32 channels on a side
                pkg.ops._desc((2, 32, 8, 8), (64, 32, 3, 3), 1, 1, 1),                     # a multi-tap filter over input channels that are no multiple of 64
                pkg.ops._desc((2, 32, 5, 7), (64, 32, 1, 1), 1, 0, 1)):                    # a map the aligned kernels do not take
        assert lib.p3d_fx_conv_wgrad_fused_workspace_bytes(ctypes.byref(bad), ctypes.byref(f)) == 0
    f.ragged = 1
    assert lib.p3d_fx_conv_wgrad_fused_workspace_bytes(ctypes.byref(pkg.ops._desc((2, 32, 5, 7), (64, 32, 1, 1), 1, 0, 1)), ctypes.byref(f)) > 0
    good.Ho = 7                                                                             # not the derived output side
    assert lib.p3d_fx_conv_wgrad_fused_workspace_bytes(ctypes.byref(good), ctypes.byref(f)) == 0
    assert lib.p3d_fx_conv_wgrad_fused(None, ctypes.byref(f), None, None, None, None, 0, None) != 0 and b'fx_conv_wgrad_fused' in lib.p3d_last_error()
    # the log answers without a launch ever made, and takes a null buffer
    assert lib.p3d_fx_wgrad_launch_log(None, 0, 1) >= 0 and pkg.ops.fx_wgrad_launch_log() == ([], 0)
