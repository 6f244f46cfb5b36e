"""The table of tests/test_fp32_mfma_instances_gpu.py, checked without a GPU: it is well-formed, its expected records name between them every
(pass, tile, TAPM, MASKED, WV) that launch_variant (csrc/p3d_conv.hip) can emit -- 24 forward, 12 data-gradient and 72 weight-gradient instances -- and every finishing
path a call can take, every descriptor passes the library's validate, and no reduction is longer than the longest of CONV_CASES, whose bounds the GPU file uses.
The library is loaded (host-only queries) and nothing is launched.

The names and order of the record's fields exist three times (the enum of csrc/p3d_conv.hip, which defines the layout; ops.LAST_FP32_FIELDS; Rec of the table) and
the buffer length twice (P3D_FP32_LAUNCH_FIELDS of the header, ops.LAST_FP32_LEN): held to each other here."""
import ctypes
import itertools
import os
import re

import pytest

import fp32_mfma_table as T
from fp32_mfma_table import ROWS


def conv_out(h, k, stride, pad, dil):
    return (h + 2 * pad - dil * (k - 1) - 1) // stride + 1


def opts(row):
    return {v for v in row.opts if not v.startswith('ws=')}


def desc(pkg, row):
    win = 'win' in row.opts
    return pkg.ops._desc((row.n, row.c, row.h, row.w), (row.k, row.c, row.r, row.s), row.stride, row.pad, row.dil, c_offset=T.WINDOW_OFFSET if win else 0,
                         c_total=row.c + T.WINDOW_EXTRA if win else row.c, accumulate=int('acc' in row.opts))


def test_the_table_is_well_formed():
    assert len({r.name for r in ROWS}) == len(ROWS)
    for r in ROWS:
        o, rec = opts(r), r.rec
        assert r.entry in ('fwd', 'bn', 'dgrad', 'wgrad') and o <= set(T.OPTIONS), r.name
        assert len([v for v in r.opts if v.startswith('ws=')]) <= 1 and all(v in T.OPTIONS or v[3:].isdigit() for v in r.opts), r.name
        assert rec.pass_ == dict(fwd=T.FWD, bn=T.FWD, dgrad=T.DGRAD, wgrad=T.WGRAD)[r.entry] and rec.eval == int(r.entry == 'bn'), r.name
        assert 0 <= rec.tile <= 5 and rec.tapm in (0, 1) and rec.masked in (0, 1) and rec.wv in (0, 1, 2) and rec.grid_x >= 1 and rec.grid_y >= 1, r.name
        assert rec.y_means in (T.Y_ONE, T.Y_SLABS, T.Y_CLASSES) and (rec.y_means != T.Y_ONE or rec.grid_y == 1), r.name
        factors = bool(o & {'mask', 'mult'})
        # options an entry has no argument for
        assert not (o & {'res', 'relu'}) or r.entry == 'bn', r.name
        assert not (o & {'bias'}) or r.entry == 'fwd', r.name
        assert not (r.entry == 'bn' and o - {'res', 'relu'}), r.name
        assert ('off_out' not in o or r.entry == 'dgrad') and (not (o & {'off_x', 'off_dy'}) or r.entry == 'wgrad'), r.name
        ho, wo = conv_out(r.h, r.r, r.stride, r.pad, r.dil), conv_out(r.w, r.s, r.stride, r.pad, r.dil)
        assert ho >= 1 and wo >= 1, r.name
        bm, bn, _ = T.TILES[rec.tile]
        if r.entry in ('fwd', 'bn'):
            split = rec.y_means == T.Y_SLABS
            assert rec.wv == 0 and rec.tapm == int(r.c >= 16) and rec.masked == int(factors) and not (split and factors), r.name
            assert rec.finish == (T.FWD_REDUCE if split else 0) and rec.grid_x == -(-r.k // bm) * -(-(r.n * ho * wo) // bn), r.name
        elif r.entry == 'dgrad':
            assert rec.wv == 0 and rec.tapm == 1, r.name
            if r.stride == 1:
                split = rec.y_means == T.Y_SLABS
                assert rec.masked == int(factors) and rec.finish == (T.FWD_REDUCE if split else 0) and rec.grid_x == -(-r.c // bm) * -(-(r.n * r.h * r.w) // bn), r.name
            else:
                aligned = r.stride == 2 and r.w % 4 == 0 and 'off_out' not in o
                assert rec.masked == int('mult' in o) and rec.y_means == T.Y_CLASSES and rec.grid_y == r.stride ** 2, r.name
                assert rec.finish == (T.INTERLEAVE2 if aligned else T.INTERLEAVE) and rec.weight_image == 0 and rec.no_room == 0, r.name
        else:
            wv = 0
            if (ho * wo) % 4 == 0 and 'off_dy' not in o:
                wv = 2 if (r.r, r.s, r.stride, r.pad) == (1, 1, 1, 0) and 'off_x' not in o else 1
            assert rec.wv == wv and rec.masked == int(factors) and rec.y_means == T.Y_SLABS and rec.weight_image == 0 and rec.no_room == 0, r.name
            assert rec.grid_x == -(-r.k // bm) * -(-(r.c * r.r * r.s) // bn) and (not rec.tapm or r.c % bn == 0), r.name
            tapm_reduce = rec.tapm and r.r * r.s > 1
            if rec.grid_y > 16:
                lds = 17 * r.r * r.s * 16 * 4 <= 64 * 1024                         # the tile of wgrad_reduce16_tapm_kernel: up to 60 taps
                assert rec.finish in ((T.WGRAD_REDUCE16_TAPM if lds else T.SLAB_FOLD | T.WGRAD_REDUCE_TAPM,) if tapm_reduce else (T.WGRAD_REDUCE16, T.SLAB_FOLD | T.WGRAD_REDUCE)), r.name
                if not tapm_reduce:
                    assert (rec.finish == T.WGRAD_REDUCE16) == ('win' not in o and (r.k * r.c * r.r * r.s) % 4 == 0), r.name
            else:
                assert rec.finish == (T.WGRAD_REDUCE_TAPM if tapm_reduce else T.WGRAD_REDUCE), r.name


def test_reductions_and_tensors_stay_within_the_caps():
    for r in ROWS:
        ho, wo = conv_out(r.h, r.r, r.stride, r.pad, r.dil), conv_out(r.w, r.s, r.stride, r.pad, r.dil)
        terms = dict(fwd=r.c * r.r * r.s, bn=r.c * r.r * r.s, dgrad=r.k * r.r * r.s, wgrad=r.n * ho * wo)[r.entry]
        assert terms <= T.MAX_TERMS[r.entry], (r.name, terms)
        assert 4 * max(r.n * r.c * r.h * r.w, r.n * r.k * ho * wo, r.k * (r.c + T.WINDOW_EXTRA) * r.r * r.s) <= 64 << 20, r.name


def test_every_instance_launch_variant_can_emit_is_named():
    named = {(r.rec.pass_, r.rec.tile, r.rec.tapm, r.rec.masked, r.rec.wv) for r in ROWS}
    fwd = {(T.FWD, t, tapm, m, 0) for t, tapm, m in itertools.product(range(6), (0, 1), (0, 1))}
    dgrad = {(T.DGRAD, t, 1, m, 0) for t, m in itertools.product(range(6), (0, 1))}
    wgrad = {(T.WGRAD, t, tapm, m, wv) for t, tapm, m, wv in itertools.product(range(6), (0, 1), (0, 1), (0, 1, 2))}
    assert (len(fwd), len(dgrad), len(wgrad)) == (24, 12, 72)
    assert named == fwd | dgrad | wgrad, sorted((fwd | dgrad | wgrad) ^ named)


def test_the_record_layout_is_the_same_everywhere(pkg):
    src = open(os.path.join(os.path.dirname(os.path.abspath(pkg._lib.__file__)), 'csrc', 'p3d_conv.hip')).read()
    enum = re.search(r'enum \{ (LAST_PASS = 0,.*?)LAST_FIELDS = P3D_FP32_LAUNCH_FIELDS \}', src, re.S).group(1)
    names = [n.strip().split(' ')[0][len('LAST_'):].lower() for n in enum.split(',') if n.strip()]
    assert tuple('pass_' if n == 'pass' else n for n in names) == pkg.ops.LAST_FP32_FIELDS == T.Rec._fields
    length = int(re.search(r'#define P3D_FP32_LAUNCH_FIELDS (\d+)', open(pkg._lib.HEADER_PATH).read()).group(1))
    assert length == pkg.ops.LAST_FP32_LEN >= len(names)


def rows_where(entry, **rec):
    return [r for r in ROWS if r.entry in entry and all(getattr(r.rec, f) == v for f, v in rec.items())]


def test_every_finishing_path_and_edge_of_the_issue_is_named():
    # unsplit forward: per tile a ragged last row tile and a ragged last column tile whose columns span two images; each order, dense and masked
    for tile, (bm, bn, _) in enumerate(T.TILES):
        for tapm in (0, 1):
            for masked in (0, 1):
                hit = [r for r in rows_where(('fwd',), tile=tile, tapm=tapm, masked=masked, y_means=T.Y_ONE)
                       if r.k % bm and r.n >= 2 and (conv_out(r.h, r.r, r.stride, r.pad, r.dil) * conv_out(r.w, r.s, r.stride, r.pad, r.dil)) % bn]
                assert hit, (tile, tapm, masked)
    masked_forms = {frozenset(opts(r) & {'mask', 'mult', 'bias'}) for r in rows_where(('fwd',), masked=1)}
    assert {frozenset({'mask'}), frozenset({'mult'}), frozenset({'mask', 'mult'}), frozenset({'mask', 'mult', 'bias'})} <= masked_forms
    dense = rows_where(('fwd',), masked=0, y_means=T.Y_ONE)
    assert any('bias' in r.opts for r in dense) and any('acc' in r.opts for r in dense) and any(r.dil == 2 for r in dense) and any('win' in r.opts and r.r == 3 for r in dense)
    assert {(r.c, r.r, r.stride) for r in rows_where(('fwd',), tapm=0)} >= {(1, 7, 2), (3, 7, 2), (4, 5, 1), (5, 5, 1)}
    # split-K forward: every tile; 2, 4 and 8 slabs; bias; accumulate; both branches of fwd_reduce_kernel; through the eval entry with and without res / relu, and unsplit
    split = rows_where(('fwd', 'bn'), finish=T.FWD_REDUCE)
    assert {r.rec.tile for r in split} == set(range(6)) and {r.rec.grid_y for r in split} >= {2, 4, 8}
    assert any('bias' in r.opts for r in split) and any('acc' in r.opts for r in split)
    steps = [(r.r * r.s * -(-r.c // T.TILES[r.rec.tile][2]), r.rec.grid_y) for r in split]                   # K-steps (channels padded to BK per tap), slabs
    assert any(nk % -(-nk // slabs) for nk, slabs in steps) and any(nk % -(-nk // slabs) == 0 for nk, slabs in steps)       # a last slab shorter than kchunk, and a full one
    for entry in ('fwd', 'bn', 'dgrad'):
        quads = {(conv_out(r.h, r.r, 1, r.pad, r.dil) * conv_out(r.w, r.s, 1, r.pad, r.dil) if entry != 'dgrad' else r.h * r.w) % 4 == 0 for r in rows_where((entry,), finish=T.FWD_REDUCE)}
        assert quads == {True, False}, entry
    for y_means in (T.Y_ONE, T.Y_SLABS):
        assert {('res' in r.opts, 'relu' in r.opts) for r in rows_where(('bn',), y_means=y_means)} == set(itertools.product((False, True), repeat=2))
    for entry in ('fwd', 'dgrad'):
        assert rows_where((entry,), no_room=T.NO_SLAB_ROOM, y_means=T.Y_ONE) and rows_where((entry,), weight_image=1, y_means=T.Y_SLABS)
        assert rows_where((entry,), no_room=T.NO_IMAGE_ROOM) and rows_where((entry,), no_room=T.NO_IMAGE_ROOM | T.NO_SLAB_ROOM, weight_image=0)
    # data gradient
    assert {'acc' in r.opts for r in rows_where(('dgrad',), finish=T.FWD_REDUCE)} == {True, False}
    s2 = [r for r in ROWS if r.entry == 'dgrad' and r.stride == 2]
    for finish in (T.INTERLEAVE, T.INTERLEAVE2):
        mine = [r for r in s2 if r.rec.finish == finish]
        assert {r.r for r in mine} >= {1, 3, 7} and any('acc' in r.opts for r in mine) and any(r.dil == 2 for r in mine) and any(r.h % 2 for r in mine), finish
        assert {frozenset(opts(r) & {'mask', 'mult'}) for r in mine} >= {frozenset(), frozenset({'mask'}), frozenset({'mult'}), frozenset({'mask', 'mult'})}, finish
    assert any('off_out' in r.opts for r in s2) and any(r.w % 2 for r in s2)
    assert {r.r for r in ROWS if r.entry == 'dgrad' and r.stride == 3} >= {3, 5}
    # weight gradient: each finishing path with accumulate 0 and 1
    def finished(bits, **kw):
        return [r for r in rows_where(('wgrad',), finish=bits, **kw)]
    for bits in (T.WGRAD_REDUCE, T.WGRAD_REDUCE_TAPM, T.WGRAD_REDUCE16, T.WGRAD_REDUCE16_TAPM, T.SLAB_FOLD | T.WGRAD_REDUCE, T.SLAB_FOLD | T.WGRAD_REDUCE_TAPM):
        assert {'acc' in r.opts for r in finished(bits)} == {True, False}, bits
    # more than 16 tap-major slabs of a filter of 61 taps or more (7x9): the in-place fold feeds the transposing reduce; dense, windowed and masked
    fold_tapm = finished(T.SLAB_FOLD | T.WGRAD_REDUCE_TAPM)
    assert any('win' in r.opts for r in fold_tapm) and {r.rec.masked for r in fold_tapm} == {0, 1} and {(r.r, r.s) for r in fold_tapm} >= {(7, 9), (9, 7)}
    assert any(r.rec.grid_y >= 32 for r in finished(T.SLAB_FOLD | T.WGRAD_REDUCE))                           # every one of the 16 fold groups has a second slab
    plain = finished(T.WGRAD_REDUCE)
    assert any('win' not in r.opts and (r.k * r.c * r.r * r.s) % 4 == 0 for r in plain) and any((r.k * r.c * r.r * r.s) % 4 for r in plain)      # its float4 and scalar branches
    assert {r.r for r in plain if 'win' in r.opts} >= {1, 3} and any('win' in r.opts for r in finished(T.WGRAD_REDUCE_TAPM))
    assert {r.r for r in finished(T.WGRAD_REDUCE16_TAPM)} >= {3, 7} and any('win' in r.opts for r in finished(T.WGRAD_REDUCE16_TAPM))
    fold = finished(T.SLAB_FOLD | T.WGRAD_REDUCE)
    assert any('win' in r.opts and r.r == 1 for r in fold) and any((r.k * r.c * r.r * r.s) % 4 for r in fold)
    wg = [r for r in ROWS if r.entry == 'wgrad']
    assert any(r.stride == 2 for r in wg) and any(r.dil == 2 for r in wg)
    assert any('off_dy' in r.opts for r in wg if r.rec.wv == 0) and any('off_dy' not in r.opts for r in wg if r.rec.wv == 0)


def test_every_descriptor_is_valid_and_its_queries_cover_the_slabs(pkg):
    L = pkg._lib.lib()
    was = L.p3d_x3_enable(0)                   # the queries of the fp32-MFMA plans alone, as the GPU file sees them
    try:
        for r in ROWS:
            d = ctypes.byref(desc(pkg, r))
            ho, wo = conv_out(r.h, r.r, r.stride, r.pad, r.dil), conv_out(r.w, r.s, r.stride, r.pad, r.dil)
            weight = r.k * r.c * r.r * r.s * 4
            assert L.p3d_conv2d_wgrad_workspace_bytes(d) >= weight, r.name                     # (0 from a descriptor validate refuses)
            query = dict(fwd=L.p3d_conv2d_fwd_workspace_bytes, bn=L.p3d_conv2d_bn_eval_fwd_workspace_bytes, dgrad=L.p3d_conv2d_dgrad_workspace_bytes,
                         wgrad=L.p3d_conv2d_wgrad_workspace_bytes)[r.entry](d)
            given = [int(v[3:]) for v in r.opts if v.startswith('ws=')]
            rec = r.rec
            result = 4 * (r.n * r.k * ho * wo if r.entry in ('fwd', 'bn') else r.n * r.c * r.h * r.w)
            image = (weight + 255) // 256 * 256
            if r.entry == 'wgrad':
                assert query >= rec.grid_y * weight, r.name
            elif r.entry == 'dgrad' and r.stride > 1:
                assert query >= r.stride ** 2 * r.n * r.c * -(-r.h // r.stride) * -(-r.w // r.stride) * 4, r.name
            elif not given:
                head = (2 * r.k * 4 + 255) // 256 * 256 if r.entry == 'bn' else 0
                need = head + (rec.grid_y * result if rec.y_means == T.Y_SLABS else 0) + (image if rec.weight_image else 0)
                assert query >= need and (query == need or rec.masked), r.name              # (one query serves the dense call, which may split, and the partial one)
            else:                                                                               # a literal workspace: short of the query by what the record says was dropped
                assert given[0] < query and rec.no_room, r.name
                room = given[0] - (image if rec.weight_image else 0)
                assert room >= (rec.grid_y * result if rec.y_means == T.Y_SLABS else 0), r.name
                if rec.no_room & T.NO_IMAGE_ROOM:
                    assert given[0] < image, r.name
    finally:
        L.p3d_x3_enable(was)
