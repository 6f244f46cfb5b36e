"""The table of tests/test_hconv_paths_gpu.py, checked without a GPU: it is well-formed; the path written out for every row is the one the restated host code of
csrc/p3d_hconv.hip derives; the restatements agree with the library itself (p3d_hconv2d_wgrad_workspace_bytes for every weight-gradient row, p3d_hconv2d_sum_rows
for every sums row) and, for fill_class_h, with a brute-force search of the taps of every pixel class; and the rows reach between them every path of REQUIRED, so a
row cannot be dropped or moved off its path unnoticed.  Then the refusals of hvalidate through the two host-only queries.  The library is loaded, nothing is launched."""
import ctypes
import itertools

import pytest

import hconv_table as T
from hconv_table import ROWS


def desc(pkg, row, **kw):
    return pkg.ops._desc((row.n, row.c, row.h, row.w), (row.k, row.c, row.r, row.r), row.stride, row.pad, row.dil, **kw)


def test_the_table_is_well_formed():
    assert len({r.name for r in ROWS}) == len(ROWS) == 173
    for r in ROWS:
        assert r.entry in T.ENTRIES and set(r.opts) <= T.OPTIONS[r.entry] and len(set(r.opts)) == len(r.opts), r.name
        ho, wo = T.out_hw(r)
        assert ho >= 1 and wo >= 1 and r.c % 8 == 0 and r.k % 8 == 0 and 1 <= r.stride <= T.HMS, r.name
        assert r.entry != 'sums' or r.stride == 1, r.name
        assert not ({'creal3', 'creal1'} & set(r.opts)) or r.c == 8, r.name
        assert 'zpad' not in r.opts or r.c == 8, r.name
        # no tensor over a few MB
        assert max(r.n * r.h * r.w * r.c * 2, r.n * ho * wo * r.k * 2, r.k * r.r * r.r * r.c * 4) <= 6 << 20, r.name    # (the largest: dy of the 64-split weight gradient, 5 MB)


def test_every_row_takes_the_path_written_for_it():
    assert set(T.PATHS) == {r.name for r in ROWS}
    wrong = ['%s: derived %r, written %r' % (r.name, T.path(r), T.PATHS[r.name]) for r in ROWS if T.path(r) != T.PATHS[r.name]]
    assert not wrong, '\n'.join(wrong)


def test_the_paths_are_complete():
    reached = set().union(*(T.features(r) for r in ROWS))
    assert not T.REQUIRED - reached, sorted(T.REQUIRED - reached)
    # ... and every row is there for something: no two rows reach the same set of paths with the same options
    seen = {}
    for r in ROWS:
        key = (frozenset(T.features(r)), r.entry, frozenset(r.opts), T.PATHS[r.name])
        assert key not in seen, '%s repeats %s' % (r.name, seen[key])
        seen[key] = r.name


def test_the_weight_gradient_plans_are_the_ones_listed():
    for key, want in T.WGRAD_PLANS.items():
        assert T.hwgrad_plan(*key) == want, key
    assert T.reduce_loops(9) == [(0, 2)] + [(0, 1)] * 7 and T.reduce_loops(32) == [(1, 0)] * 8
    assert T.reduce_loops(33) == [(1, 1)] + [(1, 0)] * 7 and T.reduce_loops(40) == [(1, 1)] * 8


def test_fill_class_h_against_brute_force():
    """every (ho, r) with ho * s - p + r * d = hi, hi in class `par`, is what the restated fill_class_h enumerates: tap r0 + step * j reads row i + off0 - offstep * j"""
    kinds = set()
    for s, R, p, d in itertools.product(range(1, 5), range(1, 8), range(0, 4), range(1, 5)):
        counts = []
        for par in range(s):
            r0, step, n, off0, offstep = T.fill_class_h(par, R, s, p, d)
            i = 50
            hi = par + s * i
            brute = {(r, (hi + p - r * d) // s - i) for r in range(R) if (hi + p - r * d) % s == 0}
            mine = {(r0 + step * j, off0 - offstep * j) for j in range(n)}
            assert mine == brute, (s, R, p, d, par, mine, brute)
            assert all(ho * s - p + r * d == par for r, ho in mine)
            counts.append(n)
            kinds |= {'dead'} if n == 0 else set()
            kinds |= {'negative'} if n and off0 < 0 else set()
            kinds |= {'step'} if n > 1 and step > 1 else set()
        kinds |= {'unequal'} if len(set(counts)) > 1 else set()
    assert kinds == {'dead', 'negative', 'step', 'unequal'}
    # the table holds each of them
    assert T.fill_class_h(1, 3, 3, 0, 2)[2:4] == (1, -1)                    # 3x3 stride 3 pad 0 dilation 2, class 1: its one tap reads the row above
    assert [T.fill_class_h(par, 3, 2, 2, 2)[2] for par in range(2)] == [3, 0]
    assert [T.fill_class_h(par, 1, 4, 0, 1)[2] for par in range(4)] == [1, 0, 0, 0]
    reached = set().union(*(T.features(r) for r in ROWS))
    assert {'class:dead', 'class:negative_off0', 'class:unequal_taps', 'class:step>1'} <= reached


def test_the_workspace_query_agrees_with_the_restated_plan(pkg):
    L = pkg._lib.lib()
    rows = [r for r in ROWS if r.entry == 'wgrad']
    assert len(rows) >= 20
    for r in rows:
        p = T.wgrad_plan(r)
        assert L.p3d_hconv2d_wgrad_workspace_bytes(ctypes.byref(desc(pkg, r))) == p['splits'] * r.k * r.r * r.r * r.c * 4, r.name


def test_sum_rows_agree_with_the_restated_tiles(pkg):
    L = pkg._lib.lib()
    rows = [r for r in ROWS if r.entry in ('stats', 'sums')]
    assert len(rows) >= 20
    for r in rows:
        assert L.p3d_hconv2d_sum_rows(ctypes.byref(desc(pkg, r)), int(r.entry == 'sums')) == T.gather_plan(r)['tiles_n'], r.name


# ---- hvalidate through the host-only queries: (what, descriptor fields, the same one pixel row / one group of 8 channels smaller or otherwise mended) ----
BASE = dict(N=2, C=16, H=9, W=11, K=24, R=3, S=3, stride=1, pad=1, dil=1)
REFUSED = [
    ('C % 8', dict(C=12), dict(C=8)),
    ('K % 8', dict(K=20), dict(K=16)),
    ('stride 0', dict(stride=0), dict(stride=1)),
    ('stride 5', dict(stride=5), dict(stride=4)),
    ('dilation 0', dict(dil=0), dict(dil=1)),
    ('pad -1', dict(pad=-1), dict(pad=0)),
    ('Ho', dict(Ho=+1), dict()),
    ('Wo', dict(Wo=-1), dict()),
    ('window offset', dict(c_offset=8, c_total=24), dict()),
    ('window total', dict(c_total=24), dict()),
    ('x of 2^31 bytes', dict(N=1, C=1024, H=1024, W=1024, K=8, R=1, S=1, pad=0), dict(N=1, C=1024, H=1023, W=1024, K=8, R=1, S=1, pad=0)),
    ('y of 2^31 bytes', dict(N=1, C=8, H=1024, W=1024, K=1024, R=1, S=1, pad=0), dict(N=1, C=8, H=1023, W=1024, K=1024, R=1, S=1, pad=0)),
    ('w of 2^31 bytes', dict(N=1, C=32768, H=1, W=1, K=32768, R=1, S=1, pad=0), dict(N=1, C=32760, H=1, W=1, K=32768, R=1, S=1, pad=0)),
]


def make_desc(pkg, fields):
    f = dict(BASE, **{k: v for k, v in fields.items() if k not in ('Ho', 'Wo', 'c_offset', 'c_total')})
    d = pkg._lib.ConvDesc()
    for k, v in f.items():
        setattr(d, k, v)
    d.Ho = T.conv_out(f['H'], f['R'], max(f['stride'], 1), f['pad'], f['dil']) + fields.get('Ho', 0)
    d.Wo = T.conv_out(f['W'], f['S'], max(f['stride'], 1), f['pad'], f['dil']) + fields.get('Wo', 0)
    d.c_total, d.c_offset = fields.get('c_total', f['C']), fields.get('c_offset', 0)
    return d


@pytest.mark.parametrize('case', REFUSED, ids=[c[0] for c in REFUSED])
def test_hvalidate_refuses(pkg, case):
    L = pkg._lib.lib()
    _, bad, good = case
    d = make_desc(pkg, bad)
    assert L.p3d_hconv2d_fwd_infer_supported(ctypes.byref(d)) == 0 and L.p3d_last_error()
    assert L.p3d_hconv2d_wgrad_workspace_bytes(ctypes.byref(d)) == 0
    d = make_desc(pkg, good)
    assert L.p3d_hconv2d_fwd_infer_supported(ctypes.byref(d)) == 1
    assert L.p3d_hconv2d_wgrad_workspace_bytes(ctypes.byref(d)) > 0


def test_the_tensors_at_the_window_are_exactly_2_31_bytes():
    for name, bad, _ in REFUSED[-3:]:
        f = dict(BASE, **bad)
        sizes = dict(x=f['N'] * f['H'] * f['W'] * f['C'] * 2, y=f['N'] * f['H'] * f['W'] * f['K'] * 2, w=f['K'] * f['C'] * 2)
        assert sizes[name[0]] == 1 << 31 and sum(v >= 1 << 31 for v in sizes.values()) == 1, name
