"""The plan of a call on the fp32-MFMA convolution kernels (Fp32Plan of csrc/p3d_conv.hip, through the host-only test hook p3d_conv2d_fp32_plan) against the records
of tests/fp32_mfma_table.py.  Those records were taken from real launches on an MI355X (tests/test_fp32_mfma_instances_gpu.py asserts them of every launch), so this
holds the planner -- tile, TAPM / MASKED / WV, grid, slabs or classes, weight image, finishing kernels, what found no room -- to what the entries launch, field by
field, with no GPU: every row, with the workspace the entry's query reports or the row's literal `ws=<bytes>`.  Nothing is launched."""
import ctypes

import pytest

import fp32_mfma_table as T
from fp32_mfma_table import ROWS
from test_fp32_mfma_instances_host import desc

ENTRY = dict(fwd=0, bn=1, dgrad=2, wgrad=3)
MASK, MULT, OFF_DY, OFF_X, OFF_OUT = 1, 2, 4, 8, 16
EWORKSPACE = -2                                # P3D_EWORKSPACE


def option_bits(row):
    o = set(row.opts)
    return MASK * ('mask' in o) | MULT * ('mult' in o) | OFF_DY * ('off_dy' in o) | OFF_X * ('off_x' in o) | OFF_OUT * ('off_out' in o)


def query(L, row, d):
    return dict(fwd=L.p3d_conv2d_fwd_workspace_bytes, bn=L.p3d_conv2d_bn_eval_fwd_workspace_bytes, dgrad=L.p3d_conv2d_dgrad_workspace_bytes,
                wgrad=L.p3d_conv2d_wgrad_workspace_bytes)[row.entry](d)


def plan(pkg, L, row, nbytes):
    out = (ctypes.c_int32 * pkg.ops.LAST_FP32_LEN)(*([77] * pkg.ops.LAST_FP32_LEN))
    rc = L.p3d_conv2d_fp32_plan(ENTRY[row.entry], ctypes.byref(desc(pkg, row)), option_bits(row), nbytes, out)
    return rc, dict(zip(pkg.ops.LAST_FP32_FIELDS, out)), list(out)


@pytest.fixture(scope='module')
def lib(pkg):
    L = pkg._lib.lib()
    was = L.p3d_x3_enable(0)                   # the queries of the fp32-MFMA plans alone, as the GPU file sees them
    yield L
    L.p3d_x3_enable(was)


@pytest.mark.parametrize('row', ROWS, ids=[r.name for r in ROWS])
def test_the_plan_is_the_recorded_launch(pkg, lib, row):
    given = [int(v[3:]) for v in row.opts if v.startswith('ws=')]
    nbytes = given[0] if given else query(lib, row, ctypes.byref(desc(pkg, row)))
    rc, record, raw = plan(pkg, lib, row, nbytes)
    assert rc == 0, lib.p3d_last_error()
    want = row.rec._asdict()
    for field in pkg.ops.LAST_FP32_FIELDS:
        assert record[field] == want[field], (row.name, field, record, want)
    assert raw[len(pkg.ops.LAST_FP32_FIELDS):] == [0] * (pkg.ops.LAST_FP32_LEN - len(pkg.ops.LAST_FP32_FIELDS))
    assert record['eval'] == int(row.entry == 'bn')


def test_no_row_is_left_out_and_every_option_of_the_table_reaches_the_hook():
    assert {r.entry for r in ROWS} == set(ENTRY)
    assert {v for r in ROWS for v in r.opts if v.startswith('off_')} == {'off_dy', 'off_x', 'off_out'}
    assert any(v.startswith('ws=') for r in ROWS for v in r.opts)


def test_a_call_the_entry_refuses_has_the_empty_record(pkg, lib):
    """one byte short of the staged classes, of the weight-gradient slabs and of the eval head: P3D_EWORKSPACE and pass -1, as the entries leave it"""
    empty = dict(pass_=-1, tile=-1, tapm=0, masked=0, wv=0, grid_x=0, grid_y=0, y_means=0, weight_image=0, finish=0, eval=0, no_room=0)
    for name in ('dgrad_s2_3x3_w4', 'dgrad_s3_5x5', 'wgrad_reduce_tapm', 'wgrad_64x64_generic_masked_wv0'):
        row = T.BY_NAME[name]
        need = query(lib, row, ctypes.byref(desc(pkg, row)))
        if row.entry == 'wgrad':               # (the query serves the dense and the masked call: the larger of the two; this call's own slabs are the record's)
            need = row.rec.grid_y * row.k * row.c * row.r * row.s * 4
        assert plan(pkg, lib, row, need)[0] == 0
        rc, record, _ = plan(pkg, lib, row, need - 1)
        assert rc == EWORKSPACE and record == empty, (name, rc, record)
        assert plan(pkg, lib, row, 0)[0] == EWORKSPACE
    row = T.BY_NAME['bn_unsplit_c16']
    head = (2 * row.k * 4 + 255) // 256 * 256
    rc, record, _ = plan(pkg, lib, row, head)
    assert rc == 0 and record == row.rec._asdict()
    rc, record, _ = plan(pkg, lib, row, head - 1)
    assert rc == EWORKSPACE and record == dict(empty, eval=1)


def test_bad_arguments_are_refused_and_leave_the_record_alone(pkg, lib):
    row = T.BY_NAME['fwd_64x64_tapm_dense']
    d = desc(pkg, row)
    out = (ctypes.c_int32 * pkg.ops.LAST_FP32_LEN)(*([77] * pkg.ops.LAST_FP32_LEN))
    for entry, options in ((-1, 0), (4, 0), (0, 32), (0, -1), (1, MASK), (1, MULT)):
        assert lib.p3d_conv2d_fp32_plan(entry, ctypes.byref(d), options, 0, out) != 0 and list(out) == [77] * len(out), (entry, options)
    assert lib.p3d_conv2d_fp32_plan(0, None, 0, 0, out) != 0 and lib.p3d_conv2d_fp32_plan(0, ctypes.byref(d), 0, 0, None) != 0
    d.Ho += 1                                  # validate refuses it
    assert lib.p3d_conv2d_fp32_plan(0, ctypes.byref(d), 0, 0, out) != 0 and list(out) == [77] * len(out)


def test_the_hook_launches_nothing_and_leaves_the_last_launch_record_alone(pkg, lib):
    before = pkg.ops.conv_last_fp32_launch()
    stats = pkg.ops.conv_path_stats()
    row = T.BY_NAME['wgrad_reduce16']
    assert plan(pkg, lib, row, query(lib, row, ctypes.byref(desc(pkg, row))))[0] == 0
    assert pkg.ops.conv_last_fp32_launch() == before and pkg.ops.conv_path_stats() == stats
