"""The table of tests/test_fx_instances_gpu.py, checked without a GPU: it is well-formed, every descriptor passes the shape predicates of the hook it is launched
through, the expected records name between them EVERY instance of fx_conv_kernel / fx16_conv_kernel the library was compiled with (p3d_fx_conv_instances, generated
from the lists the instances are compiled from) and each of the five finishing codes, and the split counts and partial rows the records imply are what the library's
own host queries report under the row's p3d_fx_tune settings.  The library is loaded (host-only queries) and nothing is launched.

The names and order of the record's fields exist three times (the enum of csrc/p3d_fx.hip, which defines the layout; ops.FX_LAUNCH_FIELDS; Rec of the table) and the
lengths twice (P3D_FX_LAUNCH_FIELDS / P3D_FX_INSTANCE_FIELDS of the header, ops.FX_LAUNCH_LEN / FX_INSTANCE_LEN): held to each other here."""
import ctypes
import os
import re

import pytest

import fx_table as T
from fx_table import ROWS


def conv_out(h, k, stride, pad, dil):
    return (h + 2 * pad - dil * (k - 1) - 1) // stride + 1


def desc(pkg, row):
    win = 'win' in row.opts
    return pkg.ops._desc((row.n, row.c, row.h, row.w), (row.k, row.c, row.r, row.r), row.stride, row.pad, row.dil, c_offset=T.WINDOW_OFFSET if win else 0,
                         c_total=row.c + T.WINDOW_EXTRA if win else row.c, accumulate=int(bool(set(row.opts) & {'acc', 'accsrc'})))


@pytest.fixture()
def tuned(pkg):
    """p3d_fx_tune settings of a row around a body, always back to the built-in plan"""
    L = pkg._lib.lib()
    touched = set()

    def apply(row):
        for what in touched:
            L.p3d_fx_tune(what, 0)
        touched.clear()
        for what, value in row.tune:
            L.p3d_fx_tune(what, value)
            touched.add(what)
    was = L.p3d_x3_enable(1)
    try:
        yield apply
    finally:
        for what in touched:
            L.p3d_fx_tune(what, 0)
        L.p3d_x3_enable(was)


def geometry(row):
    """(result channels M, reduction channels, result pixels per channel over the batch, pixels of the GEMM grid of one launch)"""
    ho, wo = conv_out(row.h, row.r, row.stride, row.pad, row.dil), conv_out(row.w, row.r, row.stride, row.pad, row.dil)
    if row.pass_ == 'fwd':
        return row.k, row.c, row.n * ho * wo, row.n * ho * wo
    return row.c, row.k, row.n * row.h * row.w, row.n * (row.h // row.stride) * (row.w // row.stride)


def test_the_table_is_well_formed():
    assert len({r.name for r in ROWS}) == len(ROWS)
    for r in ROWS:
        o = set(r.opts)
        assert r.pass_ in ('fwd', 'dgrad') and o <= set(T.OPTIONS) and len(o) == len(r.opts), r.name
        assert all(what in (1, 5) and value >= 1 for what, value in r.tune) and len(dict(r.tune)) == len(r.tune), r.name
        assert len(r.recs) >= 1 and all(isinstance(q, T.Rec) for q in r.recs), r.name
        ho, wo = conv_out(r.h, r.r, r.stride, r.pad, r.dil), conv_out(r.w, r.r, r.stride, r.pad, r.dil)
        assert ho >= 1 and wo >= 1 and r.stride in (1, 2), r.name
        # options that exclude each other or that a pass has no argument for
        assert not ({'img', 'rows'} <= o) and not ({'acc', 'accsrc'} <= o) and ('accmask' not in o or 'accsrc' in o), r.name
        assert not (o & {'bias', 'infer', 'res', 'relu'}) or r.pass_ == 'fwd', r.name
        assert not (o & {'accsrc'}) or r.pass_ == 'dgrad', r.name
        assert not (o & {'res', 'relu'}) or 'infer' in o, r.name
        assert 'infer' not in o or 'wimg' in o, r.name
        assert not ({'win', 'wimg'} <= o), r.name
        assert not ('wimg' in o and r.pass_ == 'dgrad') or (r.c % 16 == 0 and r.k % 16 == 0), r.name          # (what p3d_fx_weight_images takes)
        assert 'sums' not in o or not (o & {'acc', 'accsrc'}), r.name         # (the unsplit kernels sum in front of the accumulate, the reduce pass behind it: kept apart)
        m, red, pixels, grid_pixels = geometry(r)
        assert ('long' in o) == (red * r.r * r.r > T.MAX_TERMS), r.name
        img = bool(o & {'img', 'rows'})
        strided_dgrad = r.pass_ == 'dgrad' and r.stride == 2
        for q in r.recs:
            assert q.kernel in (0, 96, 64) and q.amode == int(img) and q.rag == int('rag' in o) and q.rows == int('rows' in o), r.name
            assert q.pro == (4 if 'factor' in o and not img else 0) and q.epi in T.EPI_NAMES and q.tapi in (0, 1), r.name
            assert not q.tapi or (img and r.r > 1 and red >= T.TAP_INNER_MIN), r.name
            assert q.grid_x == -(-m // (q.kernel or 128)) * -(-grid_pixels // 128) and q.grid_x >= 1, r.name
            assert (q.grid_y == 1) == (q.kchunk == 0) == (q.finish == T.NO_FINISH) == (q.finish_groups == 0), r.name
            assert q.grid_z == 1 or (strided_dgrad and q.grid_z == 4 and r.r == 3 and not dict(r.tune).get(5)), r.name
            if q.grid_y > 1:
                nk = r.r * r.r * (red // 16)
                assert q.epi == T.STORE and not strided_dgrad and q.grid_y == -(-nk // q.kchunk) and (q.grid_y - 1) * q.kchunk < nk, r.name
                sums = int('sums' in o) * (2 if r.pass_ == 'dgrad' else 1)
                assert q.finish == (T.REDUCE_ANY if 'rag' in o else T.REDUCE0 + sums) and q.finish_groups == (1 if 'rag' in o else min(r.n, 16)), r.name
            else:
                factor, sums, infer = 'factor' in o, 'sums' in o, 'infer' in o
                code = (T.INFER_FACTOR if factor else T.INFER) if infer else \
                    ((T.FACTOR_BWD_SUMS if r.pass_ == 'dgrad' else T.FACTOR_STATS) if sums else (T.FACTOR_IMG if img else T.FACTOR)) if factor else \
                    ((T.BWD_SUMS if r.pass_ == 'dgrad' else T.STATS) if sums else T.STORE)
                if q.kernel:                                  # the fx16 kernel reads the factor pointer at run time: the instance is the one without it
                    code = {T.FACTOR_STATS: T.STATS, T.FACTOR_BWD_SUMS: T.BWD_SUMS, T.FACTOR_IMG: T.STORE}.get(code, code)
                assert q.epi == code, r.name
        if strided_dgrad and dict(r.tune).get(5):
            assert len(r.recs) == (4 if r.r == 3 else 1), r.name
        else:
            assert len(r.recs) == 1, r.name


def test_the_record_layout_is_the_same_everywhere(pkg):
    src = open(os.path.join(os.path.dirname(os.path.abspath(pkg._lib.__file__)), 'csrc', 'p3d_fx.hip')).read()
    enum = re.search(r'enum \{ (FXL_KERNEL = 0,.*?)FXL_FIELDS = P3D_FX_LAUNCH_FIELDS \}', src, re.S).group(1)
    names = tuple(n.strip().split(' ')[0][len('FXL_'):].lower() for n in enum.split(',') if n.strip())
    assert names == pkg.ops.FX_LAUNCH_FIELDS == T.Rec._fields
    header = open(pkg._lib.HEADER_PATH).read()
    assert int(re.search(r'#define P3D_FX_LAUNCH_FIELDS (\d+)', header).group(1)) == pkg.ops.FX_LAUNCH_LEN >= len(names)
    assert int(re.search(r'#define P3D_FX_INSTANCE_FIELDS (\d+)', header).group(1)) == pkg.ops.FX_INSTANCE_LEN == names.index('rows') + 1
    assert int(re.search(r'constexpr int FX_LOG_MAX = (\d+);', src).group(1)) == pkg.ops.FX_LOG_MAX
    # the struct of the hook: the header's fields in the header's order, pointers first
    body = re.search(r'typedef struct p3d_fx_fuse \{(.*?)\} p3d_fx_fuse;', header, re.S).group(1)
    fields = []
    for line in body.split(';'):
        line = line.strip()
        if line.startswith('int32_t '):
            fields += [(n.strip(), ctypes.c_int32) for n in line[len('int32_t '):].split(',')]
        elif line:
            assert '*' in line, line
            fields.append((line.split('*')[-1].strip(), ctypes.c_void_p))
    assert fields == list(pkg._lib.FxFuse._fields_)


def test_every_compiled_instance_is_named_and_every_finishing_code_occurs(pkg):
    compiled = pkg.ops.fx_conv_instances()
    assert len(compiled) == len(set(compiled)) and (len([c for c in compiled if c[0] == 0]), len([c for c in compiled if c[0]])) == (31, 20), len(compiled)
    assert {c[0] for c in compiled} == {0, 96, 64}
    named = {T.instance(q) for r in ROWS for q in r.recs}
    barred = {inst for inst, why in T.UNREACHABLE}
    assert all(why for inst, why in T.UNREACHABLE) and not (barred & named)
    missing = set(compiled) - named - barred
    assert not missing, 'compiled instances no row reaches: ' + ', '.join(sorted(T.instance_name(i) for i in missing))
    unknown = (named | barred) - set(compiled)
    assert not unknown, 'rows expect instances that are not compiled: ' + ', '.join(sorted(T.instance_name(i) for i in unknown))
    assert {q.finish for r in ROWS for q in r.recs} == {T.NO_FINISH, T.REDUCE0, T.REDUCE1, T.REDUCE2, T.REDUCE_ANY}


def test_every_descriptor_passes_the_hooks_predicates_and_the_queries_agree_with_the_records(pkg, tuned):
    L = pkg._lib.lib()
    for r in ROWS:
        tuned(r)
        o = set(r.opts)
        d = ctypes.byref(desc(pkg, r))
        ps, rag = int(r.pass_ == 'dgrad'), int('rag' in o)
        m, red, pixels, _ = geometry(r)
        nbytes = L.p3d_fx_conv_fused_workspace_bytes(ps, d, rag)
        rows = L.p3d_fx_conv_fused_partial_rows(ps, d)
        # (0 from either: a descriptor or a shape the hook refuses -- its rule for a call without a factor; with one it wants 64 result channels, fx_masked_applies)
        assert nbytes > 0 and rows > 0, r.name
        assert 'factor' not in o or m >= 64, r.name
        assert rag or L.p3d_fx_conv_fused_workspace_bytes(ps, d, 1) > 0 or r.stride == 2, r.name
        if rag:                                                                         # a ragged row is one the aligned rule refuses
            assert L.p3d_fx_conv_fused_workspace_bytes(ps, d, 0) == 0, r.name
        if 'img' in o or 'rows' in o:                                                   # an image has whole groups of 16 reduction channels
            assert red % 16 == 0, r.name
        # what the first record says of the plan is what the queries report
        q = r.recs[0]
        image = (r.r * r.r * -(-m // 128) * (red // 16) * 3 * 128 * 16 * 2 + 255) // 256 * 256
        slab = m * pixels
        if rag:
            slab = (slab + 3) // 4 * 4
        assert nbytes == image + (q.grid_y * slab * 4 if q.grid_y > 1 else 0), r.name
        assert rows == (min(r.n, 16) if q.grid_y > 1 else -(-pixels // 128)), r.name
        if 'sums' in o:
            assert not rag, r.name
        assert 4 * max(r.n * r.c * r.h * r.w, m * pixels, r.k * (r.c + T.WINDOW_EXTRA) * r.r * r.r) <= 16 << 20, r.name



def test_the_hooks_queries_refuse_what_the_hook_refuses(pkg):
    L = pkg._lib.lib()
    good = pkg.ops._desc((2, 32, 8, 8), (64, 32, 1, 1), 1, 0, 1)
    assert L.p3d_fx_conv_fused_workspace_bytes(0, ctypes.byref(good), 0) > 0 and L.p3d_fx_conv_fused_partial_rows(0, ctypes.byref(good)) == 1
    for bad in (pkg.ops._desc((2, 24, 8, 8), (64, 24, 1, 1), 1, 0, 1),                     # reduction channels not in steps of 16
                pkg.ops._desc((2, 32, 8, 8), (16, 32, 1, 1), 1, 0, 1),                     # fewer than 32 result channels
                pkg.ops._desc((2, 32, 8, 6), (64, 32, 1, 1), 1, 0, 1)):                    # a width the aligned instances do not take
        assert L.p3d_fx_conv_fused_workspace_bytes(0, ctypes.byref(bad), 0) == 0
    good.Ho = 7                                                                             # not the derived output side
    assert L.p3d_fx_conv_fused_workspace_bytes(0, ctypes.byref(good), 0) == 0 and L.p3d_fx_conv_fused_partial_rows(0, ctypes.byref(good)) == 0
    assert L.p3d_fx_conv_fused_workspace_bytes(2, ctypes.byref(pkg.ops._desc((2, 32, 8, 8), (64, 32, 1, 1), 1, 0, 1)), 0) == 0      # the weight gradient is not the hook's
    f = pkg._lib.FxFuse()
    assert L.p3d_fx_conv_fused(0, None, ctypes.byref(f), None, None, None, None, None, 0, None) != 0 and b'fx_conv_fused' in L.p3d_last_error()

def rows_where(pass_=('fwd', 'dgrad'), has=(), lacks=(), **rec):
    return [r for r in ROWS if r.pass_ in pass_ and set(has) <= set(r.opts) and not (set(lacks) & set(r.opts)) and any(all(getattr(q, f) == v for f, v in rec.items()) for q in r.recs)]


def test_every_shape_and_edge_of_the_issue_is_named():
    def m_of(r):
        return r.k if r.pass_ == 'fwd' else r.c
    # result channel counts that leave dead rows on each tile
    assert {m_of(r) for r in rows_where(kernel=64)} >= {48, 64} and {m_of(r) for r in rows_where(kernel=96)} >= {80, 144, 272}
    assert {m_of(r) for r in rows_where(kernel=0, amode=1, rag=0)} >= {200, 320}
    for kernel in (0, 96, 64):                           # the BatchNorm epilogues on every tile, with a dead-row channel count, plane- and row-fed
        for epi in (T.STATS, T.BWD_SUMS):
            for rows in (0, 1):
                assert [r for r in rows_where(kernel=kernel, epi=epi, amode=1, rows=rows) if m_of(r) % (kernel or 128)], (kernel, epi, rows)
    # pixel counts: tiles that straddle images, an exact multiple of 128, W = 4, non-square maps
    assert [r for r in ROWS if (r.n, r.h, r.w) == (3, 12, 12)] and [r for r in ROWS if geometry(r)[2] % 128 == 0 and r.stride == 1]
    assert [r for r in ROWS if r.w == 4 and 'sums' in r.opts] and [r for r in ROWS if r.h != r.w and 'rag' not in r.opts]
    # ragged: odd H * W, 5x7 and 9x9; a slab stride that needs the 16-B round-up
    rag = rows_where(rag=1)
    assert {(r.h, r.w) for r in rag} == {(5, 7), (9, 9)}
    assert [r for r in rag if r.recs[0].grid_y > 1 and (geometry(r)[0] * geometry(r)[2]) % 4] and [r for r in rag if r.recs[0].grid_y > 1 and (geometry(r)[0] * geometry(r)[2]) % 4 == 0]
    # filters
    assert {(r.r, r.dil) for r in ROWS} >= {(1, 1), (3, 1), (3, 2)}
    # stride 2
    s2 = [r for r in ROWS if r.stride == 2]
    assert {r.r for r in s2 if r.pass_ == 'fwd'} >= {1, 3}
    assert [r for r in s2 if r.pass_ == 'dgrad' and r.recs[0].grid_z == 4] and [r for r in s2 if r.pass_ == 'dgrad' and r.r == 1 and not (set(r.opts) & {'acc'})]
    assert {r.r for r in s2 if r.pass_ == 'dgrad' and dict(r.tune).get(5)} >= {1, 3}
    assert {q.kernel for r in s2 if r.pass_ == 'dgrad' for q in r.recs} == {0, 96, 64} and [r for r in s2 if 'rows' in r.opts] and [r for r in s2 if 'factor' in r.opts]
    # split-K through p3d_fx_tune(1, n): n = 2 and an n that does not divide the K steps; N = 3 and N = 18; each reduce instance; bias, factor, residual + ReLU
    for finish in (T.REDUCE0, T.REDUCE1, T.REDUCE2):
        mine = rows_where(finish=finish)
        assert {r.n for r in mine} >= {3, 18}, finish
        assert [r for r in mine if r.recs[0].grid_y == 2] and [r for r in mine if (r.r * r.r * (geometry(r)[1] // 16)) % r.recs[0].kchunk], finish
        assert [r for r in mine if 'factor' in r.opts], finish
        assert [r for r in mine if r.n == 18 and r.recs[0].finish_groups == 16], finish
    assert rows_where(finish=T.REDUCE0, has=('bias',)) and rows_where(finish=T.REDUCE0, has=('infer', 'res', 'relu')) and rows_where(finish=T.REDUCE0, has=('infer', 'factor', 'bias'))
    assert rows_where(finish=T.REDUCE1, has=('bias',)) and rows_where(finish=T.REDUCE0, has=('acc',))
    any_ = rows_where(finish=T.REDUCE_ANY)
    assert [r for r in any_ if 'bias' in r.opts and 'acc' in r.opts] and [r for r in any_ if {'infer', 'res', 'relu'} <= set(r.opts) and 'factor' not in r.opts]
    assert [r for r in any_ if {'infer', 'factor'} <= set(r.opts)] and [r for r in any_ if 'factor' in r.opts and 'infer' not in r.opts]
    assert [r for r in any_ if (r.r * r.r * (geometry(r)[1] // 16)) % r.recs[0].kchunk] and [r for r in any_ if r.recs[0].grid_y == 2]
    assert [r for r in ROWS if not r.tune and r.recs[0].grid_y > 1]                       # and a split the built-in plan makes itself
    # accumulate: onto a prior, from a source with and without mask bytes, a split call; with a factor (whose zeros must leave the prior bit for bit)
    assert rows_where(has=('acc',), grid_y=1) and [r for r in rows_where(has=('acc',)) if r.recs[0].grid_y > 1]
    assert rows_where(has=('accsrc', 'accmask')) and rows_where(has=('accsrc',), lacks=('accmask',))
    assert {q.kernel for r in rows_where(has=('accsrc',)) for q in r.recs} == {0, 96}
    for ps in ('fwd', 'dgrad'):
        assert rows_where((ps,), has=('acc', 'factor')), ps
    # weight images: cached, built into the workspace, and a channel window (never cached)
    assert rows_where(has=('wimg',), lacks=('infer',)) and rows_where(lacks=('wimg',)) and rows_where(has=('win',))
    # the tap-inner order: every instance that has it is in the coverage test; here, that it is reached split and unsplit, and that the 64-row tile falls back
    assert [r for r in rows_where(tapi=1) if r.recs[0].grid_y > 1] and [r for r in rows_where(tapi=1) if r.recs[0].grid_y == 1]
    assert [r for r in rows_where(kernel=64, tapi=0) if 'long' in r.opts]
