"""P3D_DEVICE_EVAL on the GPU: the evaluation-statistics kernel (ops.pose_eval_stats) against numpy's float32 arithmetic -- class counts
exactly, also for joints placed exactly on the thresholds -- and Trainer.test with the switch on against the golden record and against the
switch-off record of the same process, in fp32 (folded or not) and under -half_acc with the folded fp16 net; no host read per batch."""
import json

import numpy as np
import pytest
import torch

from conftest import golden_path

pytestmark = pytest.mark.gpu

COUNT_COLUMNS = (0, 2, 4, 5, 6, 7, 8, 9, 11, 12)          # valid, pck, the six classes, batch, present
SUM_COLUMNS = (1, 3)                                       # sum dist, sum auc


def _golden_thresh():
    return json.loads(str(np.load(golden_path('eval.npz'))['thresh']))


def _launch(pkg, spec, true, rot, val, mirror, thresh, loss=1.5):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    table = torch.zeros((3, pkg.ops.EVAL_ROW), dtype=torch.float64, device='cuda')
    loss_t = torch.tensor([loss], dtype=torch.float32, device='cuda')
    out = pkg.ops.pose_eval_stats(dev(spec), dev(true), dev(rot), dev(val), dev(np.asarray(mirror, np.int32)), thresh, loss_t, table, 1, rotated=True)
    rows = table.cpu().numpy()
    assert not rows[0].any() and not rows[2].any()         # only the named row is written
    return rows[1], out.cpu().numpy()


def _numpy_row(pkg, spec, true, rot, val, mirror, thresh, loss=1.5):
    spec_r = np.einsum('Bij,BCj->BCi', rot, spec)
    true_r = np.einsum('Bij,BCj->BCi', rot, true)
    return pkg.utils.eval_row(spec_r, true_r, val, mirror, thresh, np.float32(loss), spec.shape[0]), spec_r


def _check(pkg, spec, true, rot, val, mirror, thresh):
    got, got_rot = _launch(pkg, spec, true, rot, val, mirror, thresh)
    want, want_rot = _numpy_row(pkg, spec, true, rot, val, mirror, thresh)
    assert got_rot.dtype == want_rot.dtype == np.float32
    assert np.array_equal(got_rot.view(np.int32), want_rot.view(np.int32)), 'rotated spec differs from np.einsum'
    for c in COUNT_COLUMNS:
        assert got[c] == want[c], (c, got[c], want[c])
    for c in SUM_COLUMNS:
        assert got[c] == pytest.approx(want[c], rel=1e-6), c
    assert got[pkg.ops.EVAL_LOSS] == float(np.float32(1.5))
    return got


def test_kernel_matches_analyze_on_golden_batches(pkg):
    g = np.load(golden_path('eval.npz'))
    thresh = _golden_thresh()
    mirror = pkg.utils.get_info().mirror
    for i in range(3):
        spec, true, val = g['an%d.spec' % i], g['an%d.true' % i], g['an%d.val' % i]
        eye = np.tile(np.eye(3, dtype=np.float32), (spec.shape[0], 1, 1))
        row = _check(pkg, spec, true, eye, val, mirror, thresh)
        want = json.loads(str(g['an%d.stats' % i]))
        n = row[pkg.ops.EVAL_VALID]
        assert n == want['batch_size']
        for k, key in enumerate(pkg.ops.EVAL_CLASSES):
            assert row[pkg.ops.EVAL_SOLID + k] / n == pytest.approx(want[key], abs=1e-9), key
        assert row[pkg.ops.EVAL_PCK] / n == pytest.approx(want['score_pck'], abs=1e-9)
        assert row[pkg.ops.EVAL_SUM_DIST] / n == pytest.approx(want['cam_mean'], rel=1e-6)
        assert row[pkg.ops.EVAL_SUM_AUC] / n == pytest.approx(want['score_auc'], rel=1e-6, abs=1e-9)


@pytest.mark.parametrize('seed', range(4))
def test_kernel_matches_numpy_on_random_rotated_batches(pkg, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    info = pkg.utils.get_info()
    b, j = (64, 17) if seed < 2 else (37, 17)
    thresh = _golden_thresh() if seed % 2 == 0 else dict(solid=40.3, close=80.7, rough=150.1)
    rot = np.linalg.qr(rng.standard_normal((b, 3, 3)))[0].astype(np.float32)
    true = (rng.standard_normal((b, j, 3)) * 300.0).astype(np.float32)
    scale = rng.choice([10.0, 40.0, 90.0, 200.0], size=(b, j, 1))
    spec = (true + rng.standard_normal((b, j, 3)) * scale).astype(np.float32)
    swap = rng.random((b, j)) < 0.15                                        # mirror-swapped joints: near the mirrored joint's truth
    spec[swap] = (true[:, info.mirror][swap] + rng.standard_normal((int(swap.sum()), 3)) * 20.0).astype(np.float32)
    flat = (rng.random((b, j)) < 0.1)[..., None]                            # image-plane hits: only depth is off
    spec = np.where(flat, true + np.array([5.0, -3.0, 400.0], np.float32), spec).astype(np.float32)
    val = rng.random((b, j)) >= rng.uniform(0.2, 0.3)
    row = _check(pkg, spec, true, rot, val, info.mirror, thresh)
    assert all(row[pkg.ops.EVAL_SOLID + k] > 0 for k in range(6)), 'every class should be populated'


@pytest.mark.parametrize('thresh', [None, dict(solid=40.3, close=80.7, rough=150.1)])
def test_kernel_counts_joints_exactly_on_the_thresholds(pkg, thresh):
    thresh = thresh or _golden_thresh()
    info = pkg.utils.get_info()
    rng = np.random.Generator(np.random.PCG64(11))
    b, j = 6, 17
    t = {k: np.float32(v) for k, v in thresh.items()}
    above = {k: np.nextafter(v, np.float32(np.inf)) for k, v in t.items()}
    true = (rng.standard_normal((b, j, 3)) * 300.0).astype(np.float32)
    true[:, :8, 0] = 0.0                                   # x = 0: spec - true along x is exactly the offset
    spec = true.copy()
    # joint -> x offset (and z offset): on / just above each threshold, the tangent test at `close`, PCK at `rough`
    for k, (dx, dz) in enumerate(((t['solid'], 0), (above['solid'], 0), (t['close'], 0), (above['close'], 0),
                                  (t['close'], 500.0), (above['close'], 500.0), (t['rough'], 0), (above['rough'], 0))):
        spec[:, k, 0] = dx
        spec[:, k, 2] += np.float32(dz)
    spec[:, 8:12] = true[:, info.mirror[8:12]]              # mirror-swapped joints
    eye = np.tile(np.eye(3, dtype=np.float32), (b, 1, 1))
    val = np.ones((b, j), bool)
    val[1, 3] = val[4, 0] = False
    row = _check(pkg, spec, true, eye, val, info.mirror, thresh)
    assert row[pkg.ops.EVAL_SOLID] >= b - 1 and row[pkg.ops.EVAL_PCK] >= 5 * b - 2     # joints 0-3 and 6 are within rough


def test_kernel_output_is_reproducible(pkg):
    rng = np.random.Generator(np.random.PCG64(5))
    rot = np.linalg.qr(rng.standard_normal((64, 3, 3)))[0].astype(np.float32)
    true = (rng.standard_normal((64, 17, 3)) * 300.0).astype(np.float32)
    spec = (true + rng.standard_normal((64, 17, 3)) * 80.0).astype(np.float32)
    val = rng.random((64, 17)) >= 0.25
    mirror = pkg.utils.get_info().mirror
    rows = [_launch(pkg, spec, true, rot, val, mirror, _golden_thresh())[0] for _ in range(3)]
    assert all(np.array_equal(rows[0].view(np.int64), r.view(np.int64)) for r in rows[1:])


def test_kernel_rejects_bad_arguments(pkg):
    dev = torch.zeros((2, 17, 3), device='cuda')
    val = torch.ones((2, 17), dtype=torch.bool, device='cuda')
    mirror = torch.zeros(17, dtype=torch.int32, device='cuda')
    loss = torch.zeros(1, device='cuda')
    table = torch.zeros((1, pkg.ops.EVAL_ROW), dtype=torch.float64, device='cuda')
    rot = torch.eye(3, device='cuda').expand(2, 3, 3)
    thresh = _golden_thresh()
    with pytest.raises(pkg.ops.P3DError):
        pkg.ops.pose_eval_stats(dev, dev, rot, val, mirror, thresh, loss, table, 1)          # row outside the table
    with pytest.raises(pkg.ops.P3DError):
        pkg.ops.pose_eval_stats(dev, dev, rot, val, mirror, thresh, loss, table.float(), 0)  # fp32 table
    with pytest.raises(pkg.ops.P3DError):
        pkg.ops.pose_eval_stats(dev, dev, rot, val, mirror, dict(thresh, rough=0.0), loss, table, 0)


# ---- Trainer.test -------------------------------------------------------------------------------------------------------------------

def _trainer(pkg, tmp_path, extra=()):
    g = np.load(golden_path('eval.npz'))
    meta = tmp_path / 'metadata.json'
    meta.write_text(json.dumps(dict(loader=dict(h36m='depth_datasets'), no_depth=dict(h36m=False),
                                    thresholds=dict(h36m=json.loads(str(g['thresh']))), root=dict(h36m=str(tmp_path)))))
    args = pkg.opts.parse(['-model', 'resnet18', '-suffix', 't', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1',
                           '-num_joints', '17', '-side_in', '256', '-metadata', str(meta)] + list(extra))
    model, _ = pkg.depth_main.create_model(args)
    det = pkg.synth.det_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 0)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in det.items()})
    trainer = pkg.depth_train.Trainer(args, model.cuda(), pkg.utils.get_info())
    trainer.verbose = False
    return trainer


def _batches(pkg, n):
    """The batches of tests/test_eval.py::test_trainer_test_matches_reference (n = 2), continued for n > 2."""
    out = []
    for it in range(n):
        c, d, tc, tv = pkg.synth.make_batch(2, side=256, rank=7, step=it, invalid_frac=0.2)
        rot = np.linalg.qr(np.random.Generator(np.random.PCG64(it)).standard_normal((2, 3, 3)))[0].astype(np.float32)
        out.append(tuple(torch.from_numpy(a) for a in (c, d, tc, tv, rot)))
    return out


def _agree(on, off):
    assert set(on) == set(off)
    assert on['test_loss'] == off['test_loss']
    assert on['cam_mean'] == pytest.approx(off['cam_mean'], rel=1e-6)
    assert on['score_auc'] == pytest.approx(off['score_auc'], rel=1e-6)
    for k in ('score_pck', 'solid', 'close', 'depth', 'jitter', 'switch', 'fail'):
        assert on[k] == pytest.approx(off[k], abs=1e-9), k


def _meets_golden(record):
    want = json.loads(str(np.load(golden_path('eval.npz'))['test_record']))
    assert set(record) == set(want)
    assert record['test_loss'] == pytest.approx(want['test_loss'], rel=1e-3)
    assert record['cam_mean'] == pytest.approx(want['cam_mean'], rel=1e-3)
    for k in ('score_pck', 'score_auc', 'solid', 'close', 'depth', 'jitter', 'switch', 'fail'):
        assert record[k] == pytest.approx(want[k], abs=2e-3), k


@pytest.mark.parametrize('folded', ['0', '1'])
def test_trainer_device_eval_fp32(pkg, tmp_path, monkeypatch, folded):
    monkeypatch.setenv('P3D_FOLDED_EVAL', folded)
    trainer = _trainer(pkg, tmp_path)
    batches = _batches(pkg, 2)
    monkeypatch.setenv('P3D_DEVICE_EVAL', '0')
    off = trainer.test(1, batches)
    monkeypatch.setenv('P3D_DEVICE_EVAL', '1')
    on = trainer.test(1, batches)
    assert not trainer.model.training
    _meets_golden(on)
    _agree(on, off)


def test_trainer_device_eval_half_folded(pkg, tmp_path, monkeypatch):
    monkeypatch.setenv('P3D_FOLDED_EVAL_HALF', '1')
    trainer = _trainer(pkg, tmp_path, ['-half_acc'])
    batches = _batches(pkg, 3)
    monkeypatch.setenv('P3D_DEVICE_EVAL', '0')
    off = trainer.test(1, batches)
    monkeypatch.setenv('P3D_DEVICE_EVAL', '1')
    on = trainer.test(1, batches)
    _agree(on, off)


def test_trainer_device_eval_prints_the_same_lines(pkg, tmp_path, monkeypatch, capsys):
    trainer = _trainer(pkg, tmp_path)
    trainer.verbose = True
    batches = _batches(pkg, 3)
    monkeypatch.setenv('P3D_DEVICE_EVAL', '0')
    trainer.test(2, batches)
    off = capsys.readouterr().out
    monkeypatch.setenv('P3D_DEVICE_EVAL', '1')
    trainer.test(2, batches)
    on = capsys.readouterr().out
    assert on == off and on.count('| test Epoch[2]') == 3


def test_trainer_device_eval_raises_on_a_batch_without_valid_joints(pkg, tmp_path, monkeypatch):
    trainer = _trainer(pkg, tmp_path)
    batches = _batches(pkg, 2)
    c, d, tc, tv, rot = batches[1]
    batches[1] = (c, d, tc, torch.zeros_like(tv), rot)
    monkeypatch.setenv('P3D_DEVICE_EVAL', '0')
    with pytest.raises(ZeroDivisionError):
        trainer.test(1, batches)
    monkeypatch.setenv('P3D_DEVICE_EVAL', '1')
    with pytest.raises(ZeroDivisionError):
        trainer.test(1, batches)


def test_trainer_device_eval_reads_nothing_back_per_batch(pkg, tmp_path, monkeypatch):
    monkeypatch.setenv('P3D_DEVICE_EVAL', '1')
    trainer = _trainer(pkg, tmp_path)
    batches = _batches(pkg, 6)
    trainer.test(1, batches[:2])                          # warm: plans, workspaces
    calls = []

    def counting(name, fn):
        def wrapped(*args, **kwargs):
            calls.append(name)
            return fn(*args, **kwargs)
        return wrapped

    for name in ('item', 'cpu', 'numpy', 'tolist'):
        monkeypatch.setattr(torch.Tensor, name, counting(name, getattr(torch.Tensor, name)))
    monkeypatch.setattr(torch.cuda, 'synchronize', counting('synchronize', torch.cuda.synchronize))
    counts = []
    for n in (2, 6):
        del calls[:]
        trainer.test(1, batches[:n])
        counts.append(list(calls))
    assert counts[0] == counts[1], counts
    assert len(counts[0]) >= 1                             # the one read of the table after the loop
