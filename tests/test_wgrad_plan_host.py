"""The plan of the x3 weight gradient (fx_wgrad_plan, through the test hook p3d_fx_wgrad_plan) against the plans recorded from the code it replaced
(tests/golden/wgrad_plans.json, written by tests/golden/make_wgrad_plans.py): for every weight-gradient descriptor of the conv-query sweep the x3 kernels admit, every
operand form the launcher takes and a few it refuses, under the built-in split rule, p3d_fx_tune(0, 3) and p3d_fx_tune(2, 512) -- the kernel instance, the taps per column
tile, the slabs, the K steps per slab, the grid, the block order and the slab bytes.  A handful of records are spelled out by hand from the rules, so that a stale table
cannot pass silently, and every compiled weight-gradient kernel (P3D_FX_WGRAD_INSTANCES of csrc/p3d_fx.hip) must be named by a record.  No GPU needed.

Provenance of the table: the replaced code had no such hook, so the records were NOT read off its launch path.  They come from a build of the parent commit to which the
same hook was added by hand, its body a branch-by-branch transcription of that commit's fx_wgrad_two_taps / fx_wgrad_splits / fx_wgrad_order and of the checks, grids and
kernel choices of fx_conv_wgrad_slabs / fx_stem_wgrad; that transcription is not kept in the repository.  What stands behind it besides the hand-spelled records below:
the same weight gradients, bit for bit, from the parent's library and this one through every public entry on the GPU (profiles/wgrad_plan_refactor.md section 4)."""
import importlib.util
import json
import os
import re

import pytest

from conftest import golden_path

_spec = importlib.util.spec_from_file_location('make_wgrad_plans', golden_path('make_wgrad_plans.py'))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

ALIGNED, ANY, ANY_MASKED, ANY_IMG = 0, 1, 2, 3


@pytest.fixture(scope='module')
def golden():
    with open(gen.PATH) as f:
        return json.load(f)


@pytest.fixture()
def lib(pkg):
    """the library with the x3 kernels on and the built-in split rule, put back afterwards"""
    L = pkg._lib.lib()
    was = L.p3d_x3_enable(1)
    try:
        yield L
    finally:
        L.p3d_fx_tune(0, 0)
        L.p3d_fx_tune(2, 0)
        L.p3d_x3_enable(was)


def rec(L, pkg, shape, operands, stem=False):
    """the hook's record as a dict; shape = (N, C, H, W, K, R) at stride 1 with "same" padding, or a stem's (N, Cin, H, W, K)"""
    d = gen.stem_desc(pkg, shape) if stem else gen.queries.desc(pkg, shape + (1, shape[5] // 2, 1, 0, shape[1], 0))
    p = gen.plan(L, d, operands)
    return None if p is None else dict(zip(gen.FIELDS, p), instance=p[:6], grid=p[9:12], slab_bytes=p[14] + (p[15] << 32))


def test_the_table_is_the_generators_sweep(lib, pkg, golden):
    assert golden['fields'] == gen.FIELDS and golden['forms'] == gen.FORMS and golden['stem_forms'] == gen.STEM_FORMS
    assert [tuple(c) for c in golden['configs']] == gen.CONFIGS == [(0, 0), (3, 0), (0, 512)]
    assert [tuple(r[0]) for r in golden['rows']] == [r for r in gen.sweep() if gen.admitted(lib, gen.queries.desc(pkg, r))]
    assert [tuple(r[0]) for r in golden['stem_rows']] == gen.STEMS
    assert len(golden['rows']) >= 250 and os.path.getsize(gen.PATH) < 64 * 1024
    # the sweep holds descriptors the x3 kernels refuse (they are not in the table) and ones only the kernels for any map width take
    assert len(golden['rows']) < len(gen.sweep())
    first = [gen.expand(golden, a)[0] for _, a in golden['rows']]
    assert any(r[gen.FORMS.index(0)] is None and r[gen.FORMS.index(gen.ANY)] is not None for r in first)
    # every form the launcher takes is planned for some descriptor, every form it refuses for none
    for i, form in enumerate(gen.FORMS):
        assert any(r[i] is not None for r in first) == (form in gen.TAKEN), form


def test_the_plans_do_not_move(lib, pkg, golden):
    wrong, n = [], 0
    for rows, forms, make in ((golden['rows'], gen.FORMS, gen.queries.desc), (golden['stem_rows'], gen.STEM_FORMS, gen.stem_desc)):
        descs = [make(pkg, tuple(r[0])) for r in rows]
        want = [gen.expand(golden, a) for _, a in rows]
        for ci, cfg in enumerate(gen.CONFIGS):
            with gen.config(lib, cfg):
                for (row, _), d, w in zip(rows, descs, want):
                    for form, expected in zip(forms, w[ci]):
                        got = gen.plan(lib, d, form)
                        n += 1
                        if got != expected:
                            wrong.append('%s operands %d under (splits, target) = %s: %s, recorded %s' % (row, form, cfg, got, expected))
    assert not wrong, '%d of %d plans moved:\n%s' % (len(wrong), n, '\n'.join(wrong[:40]))
    assert n > 10000


def test_every_compiled_instance_is_named_by_a_record(pkg, golden):
    src = open(os.path.join(os.path.dirname(os.path.abspath(pkg._lib.__file__)), 'csrc', 'p3d_fx.hip')).read()
    body = re.search(r'#define P3D_FX_WGRAD_INSTANCES\(X\)(.*?)\n#define P3D_FX_WGRAD_ANY_INSTANCES\(X\)(.*?)\n', src, re.S)
    compiled = [(ALIGNED,) + tuple(int(v) for v in m) for m in re.findall(r'X\((\d), (\d), (\d), (\d), (\d)\)', body.group(1))]
    families = dict(FX_WG_ANY=ANY, FX_WG_ANY_MASKED=ANY_MASKED, FX_WG_ANY_IMG=ANY_IMG)
    compiled += [(families[m], 0, 0, 0, 0, 0) for m in re.findall(r'X\((FX_WG_\w+), \w+\)', body.group(2))]
    assert len(compiled) == len(set(compiled)) == 16 and len([c for c in compiled if c[0] == ALIGNED]) == 13
    named = {tuple(i[:6]) for i in golden['insts']}
    used = {q for rows in (golden['rows'], golden['stem_rows']) for _, ans in rows for a in ans if not isinstance(a, int) for q in golden['inst_patterns'][a[0]] if q >= 0}
    assert used == set(range(len(golden['insts'])))
    assert named == set(compiled), 'compiled and never planned: %s; planned and not compiled: %s' % (sorted(set(compiled) - named), sorted(named - set(compiled)))


def test_records_spelled_out_from_the_rules(lib, pkg):
    """By hand.  K steps: N * (Ho Wo / 16) on aligned maps.  Tiles: K tiles (128) x C tiles (128) x taps, or with t taps per column tile K tiles x ceil(taps / t).  Slabs:
    the nearest of target / tiles (target 768 for 1, 3, 9 tiles; 512 for 5), at most steps / 32 (any map width: steps / 8), at least 1."""
    img, fp32 = gen.DY_IMG | gen.X_IMG, 0
    # 64 -> 64 3x3 at 16 x 16, N = 64, both operands images: three taps per column tile, one block row of taps; 1024 steps, 768 / 3 = 256 slabs cut to 1024 / 32 = 32
    r = rec(lib, pkg, (64, 64, 16, 16, 64, 3), img)
    assert r['instance'] == (ALIGNED, 1, 1, 0, 3, 0) and r['tile_taps'] == 3 and r['splits'] == 32 and r['spb'] == 32 and r['grid'] == (3, 1, 32)
    assert r['order'] == 0 and r['tapm'] == 1 and r['slab_bytes'] == 32 * 64 * 64 * 9 * 4
    assert rec(lib, pkg, (64, 64, 16, 16, 64, 3), img | gen.ROWS)['instance'] == (ALIGNED, 1, 1, 0, 3, 1)
    # N = 4: 64 steps, two slabs
    r = rec(lib, pkg, (4, 64, 16, 16, 64, 3), img)
    assert r['instance'] == (ALIGNED, 1, 1, 0, 3, 0) and (r['splits'], r['spb'], r['grid']) == (2, 32, (3, 1, 2))
    # 64 -> 128: two taps per column tile, five tiles
    r = rec(lib, pkg, (64, 64, 16, 16, 128, 3), img)
    assert r['instance'] == (ALIGNED, 1, 1, 0, 2, 0) and r['tile_taps'] == 2 and r['splits'] == 32 and r['grid'] == (5, 1, 32)
    # the same layer fp32-fed: one tap per block, the slabs times the taps in grid.z; and with a dy image alone
    r = rec(lib, pkg, (64, 64, 16, 16, 128, 3), fp32)
    assert r['instance'] == (ALIGNED, 0, 0, 0, 0, 0) and r['tile_taps'] == 0 and r['splits'] == 32 and r['grid'] == (1, 1, 9 * 32) and r['slab_bytes'] == 32 * 128 * 64 * 9 * 4
    r = rec(lib, pkg, (64, 64, 16, 16, 128, 3), gen.DY_IMG)
    assert r['instance'] == (ALIGNED, 1, 0, 0, 0, 0) and r['grid'] == (1, 1, 9 * 32)
    # a forced slab count (p3d_fx_tune(0, 3)) and a forced target (p3d_fx_tune(2, 9): nine blocks over nine tiles, one slab)
    lib.p3d_fx_tune(0, 3)
    r = rec(lib, pkg, (64, 64, 16, 16, 128, 3), fp32)
    assert (r['splits'], r['spb'], r['grid']) == (3, 342, (1, 1, 27))
    lib.p3d_fx_tune(0, 0)
    lib.p3d_fx_tune(2, 9)
    assert rec(lib, pkg, (64, 64, 16, 16, 128, 3), fp32)['splits'] == 1
    lib.p3d_fx_tune(2, 0)
    # a 17 x 17 map: refused aligned, planned at any map width -- ceil(2 * 289 / 16) = 37 steps of the flat pixel index, at least 8 per slab: 4 slabs of 10
    assert rec(lib, pkg, (2, 128, 17, 17, 128, 3), fp32) is None and rec(lib, pkg, (2, 128, 17, 17, 128, 3), img) is None
    r = rec(lib, pkg, (2, 128, 17, 17, 128, 3), gen.ANY)
    assert r['instance'] == (ANY, 0, 0, 0, 0, 0) and (r['splits'], r['spb'], r['grid']) == (4, 10, (1, 1, 9 * 4)) and r['slab_bytes'] == 4 * 128 * 128 * 9 * 4
    assert rec(lib, pkg, (2, 128, 17, 17, 128, 3), gen.ANY | gen.DY_FACTOR | gen.X_FACTOR)['instance'] == (ANY_MASKED, 0, 0, 0, 0, 0)
    r = rec(lib, pkg, (2, 128, 17, 17, 128, 3), gen.ANY | img)
    assert r['instance'] == (ANY_IMG, 0, 0, 0, 0, 0) and (r['splits'], r['spb']) == (4, 10)
    # on a 16 x 16 map the same kernels keep the 8-step floor: 32 steps, 4 slabs where the aligned plan has one
    assert rec(lib, pkg, (2, 128, 16, 16, 128, 3), gen.ANY)['splits'] == 4 and rec(lib, pkg, (2, 128, 16, 16, 128, 3), fp32)['splits'] == 1
    # a multi-tap layer with C >= 512 walks the taps fastest; a 1x1 and a narrower layer do not; 1x1 slabs are not tap-major
    assert rec(lib, pkg, (2, 512, 16, 16, 128, 3), img)['order'] == 1 and rec(lib, pkg, (2, 512, 16, 16, 128, 3), fp32)['order'] == 1
    assert rec(lib, pkg, (2, 448, 16, 16, 128, 3), img)['order'] == 0
    r = rec(lib, pkg, (2, 512, 16, 16, 128, 1), img)
    assert r['order'] == 0 and r['tapm'] == 0 and r['grid'] == (4, 1, 1)
    # a partial convolution: both factors beside fp32 operands, or a dy image (which carries its factor) beside x and its factor
    assert rec(lib, pkg, (2, 128, 16, 16, 128, 3), gen.DY_FACTOR | gen.X_FACTOR)['instance'] == (ALIGNED, 0, 0, 1, 0, 0)
    assert rec(lib, pkg, (2, 128, 16, 16, 128, 3), gen.DY_IMG | gen.X_FACTOR)['instance'] == (ALIGNED, 1, 0, 1, 0, 0)
    assert rec(lib, pkg, (2, 128, 16, 16, 128, 3), gen.DY_FACTOR) is None and rec(lib, pkg, (2, 128, 16, 16, 128, 3), gen.X_IMG) is None
    # an image needs whole groups of 16 channels
    assert rec(lib, pkg, (2, 128, 16, 16, 120, 1), fp32) is not None and rec(lib, pkg, (2, 128, 16, 16, 120, 1), gen.DY_IMG) is None
    # the stem at N = 64, 256 x 256: 64 * 1024 steps, 384 slabs (two column tiles of eight taps: 768 blocks); its own split rule ignores p3d_fx_tune
    lib.p3d_fx_tune(0, 3)
    r = rec(lib, pkg, (64, 3, 256, 256, 64), gen.STEM, stem=True)
    assert r['instance'] == (ALIGNED, 0, 1, 0, 1, 0) and r['tile_taps'] == 8 and (r['splits'], r['spb'], r['grid']) == (384, 171, (2, 1, 384)) and r['slab_bytes'] == 384 * 64 * 256 * 4
    assert rec(lib, pkg, (64, 3, 256, 256, 64), gen.STEM | gen.DY_FACTOR, stem=True)['instance'] == (ALIGNED, 0, 1, 1, 1, 0)
    assert rec(lib, pkg, (64, 3, 256, 256, 64), gen.STEM | gen.DY_IMG, stem=True) is None


def test_the_hook_refuses_cleanly(lib, pkg):
    import ctypes
    out = (ctypes.c_int32 * 16)(*([-7] * 16))
    d = gen.queries.desc(pkg, (2, 128, 16, 16, 128, 3, 1, 1, 1, 0, 128, 0))
    assert lib.p3d_fx_wgrad_plan(None, 0, out) != 0 and lib.p3d_fx_wgrad_plan(ctypes.byref(d), 0, None) != 0 and lib.p3d_fx_wgrad_plan(ctypes.byref(d), 128, out) != 0
    assert lib.p3d_fx_wgrad_plan(ctypes.byref(d), gen.X_IMG, out) != 0 and b'fx_wgrad_plan' in lib.p3d_last_error()
    d.Ho = 7
    assert lib.p3d_fx_wgrad_plan(ctypes.byref(d), 0, out) != 0
    assert list(out) == [-7] * 16
