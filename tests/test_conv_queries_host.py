"""The host-only convolution queries against their recorded answers (tests/golden/conv_queries.json, written by tests/golden/make_conv_queries.py): the workspace
sizes of the per-layer entries, every *_supported verdict of the x3 kernels and the block executor's admission and workspaces, over a descriptor sweep and under each
setting of p3d_x3_enable, p3d_x3_any_enable and the forced split counts.  The kernel family a call lands on is decided by host code that these queries share with
the entries; a change there that moves an answer fails here with the descriptor and the query named.  No GPU needed."""
import importlib.util
import json
import os

import pytest

from conftest import golden_path

_spec = importlib.util.spec_from_file_location('make_conv_queries', golden_path('make_conv_queries.py'))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope='module')
def golden():
    with open(gen.PATH) as f:
        return json.load(f)


def _expand(ans):
    out = []
    for a in ans:
        out.append(out[a] if isinstance(a, int) else a)
    return out


def test_the_table_is_the_generators_sweep(golden):
    """same columns, settings and descriptors as the committed generator produces: the table cannot go stale against it unnoticed"""
    assert golden['queries'] == gen.QUERIES and golden['block_queries'] == gen.BLOCK_QUERIES
    assert [tuple(c) for c in golden['configs']] == gen.CONFIGS
    assert [tuple(r[0]) for r in golden['rows']] == gen.sweep()
    assert [tuple(r[0]) for r in golden['block_rows']] == gen.block_sweep()
    assert 300 <= len(golden['rows']) <= 800 and os.path.getsize(gen.PATH) < 128 * 1024
    assert {tuple(c[:2]) for c in gen.CONFIGS} == {(0, 0), (0, 1), (1, 0), (1, 1)} and any(c[2] == 3 for c in gen.CONFIGS)


def _check(pkg, rows, names, make, ask):
    L = pkg._lib.lib()
    rest = gen.answers(L, gen.desc(pkg, gen.sweep()[0]))
    descs = [make(pkg, tuple(r[0])) for r in rows]
    wrong = []
    for ci, cfg in enumerate(gen.CONFIGS):
        with gen.config(L, cfg):
            for (row, ans), d in zip(rows, descs):
                want, got = _expand(ans)[ci], ask(L, d)
                wrong += ['%s under (x3, any, splits) = %s: %s is %d, recorded %d' % (row, cfg, n, g, w) for n, g, w in zip(names, got, want) if g != w]
    assert not wrong, '%d answers moved:\n%s' % (len(wrong), '\n'.join(wrong[:40]))
    assert gen.answers(L, gen.desc(pkg, gen.sweep()[0])) == rest          # every switch is back where it was


def test_conv_queries_do_not_move(pkg, golden):
    _check(pkg, golden['rows'], gen.QUERIES, gen.desc, gen.answers)


def test_block_queries_do_not_move(pkg, golden):
    _check(pkg, golden['block_rows'], gen.BLOCK_QUERIES, gen.block_desc, gen.block_answers)
    assert any(_expand(a)[0][0] for _, a in golden['block_rows']) and not all(_expand(a)[0][0] for _, a in golden['block_rows'])
