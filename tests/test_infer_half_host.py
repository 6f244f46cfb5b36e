"""infer.fold_half refusals and the P3D_FOLDED_EVAL_HALF switch (no GPU needed)."""
import types

import pytest


def _model(pkg, *extra):
    args = pkg.opts.parse(['-model', 'resnet18', '-suffix', 't', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1',
                           '-num_joints', '17', '-side_in', '128'] + list(extra))
    return pkg.depth_main.create_model(args)[0]


def test_fold_half_refuses_training_batchnorm(pkg):
    model = _model(pkg, '-half_acc').eval()
    model.layer3[0].downsample[1].train()
    with pytest.raises(pkg._lib.P3DError, match='training mode'):
        pkg.infer.fold_half(model)


def test_fold_half_refuses_host_parameters(pkg):
    with pytest.raises(pkg._lib.P3DError, match='fp32 masters on the HIP device'):
        pkg.infer.fold_half(_model(pkg, '-half_acc').eval())


def test_fold_half_refuses_fp16_parameters(pkg):
    model = _model(pkg).eval().half()
    with pytest.raises(pkg._lib.P3DError, match='fp32 masters'):
        pkg.infer.fold_half(model)


def test_fold_points_half_models_at_fold_half(pkg):
    model = _model(pkg).eval()
    model._p3d_half = True
    with pytest.raises(pkg._lib.P3DError, match='fold_half'):
        pkg.infer.fold(model)


@pytest.mark.parametrize('value,on', [(None, False), ('0', False), ('1', True), ('yes', False), ('', False)])
def test_folded_eval_half_switch(pkg, monkeypatch, value, on):
    if value is None:
        monkeypatch.delenv('P3D_FOLDED_EVAL_HALF', raising=False)
    else:
        monkeypatch.setenv('P3D_FOLDED_EVAL_HALF', value)
    monkeypatch.delenv('P3D_FOLDED_EVAL', raising=False)
    assert pkg.infer.half_enabled() is on
    Trainer = pkg.depth_train.Trainer
    assert Trainer._folding(types.SimpleNamespace(half_acc=True)) is on
    assert Trainer._folding(types.SimpleNamespace(half_acc=False)) is False         # fp32 training keeps P3D_FOLDED_EVAL's meaning


@pytest.mark.parametrize('fp32,half', [('1', '0'), ('1', None), ('0', '1')])
def test_the_two_switches_are_independent(pkg, monkeypatch, fp32, half):
    monkeypatch.setenv('P3D_FOLDED_EVAL', fp32)
    if half is None:
        monkeypatch.delenv('P3D_FOLDED_EVAL_HALF', raising=False)
    else:
        monkeypatch.setenv('P3D_FOLDED_EVAL_HALF', half)
    Trainer = pkg.depth_train.Trainer
    assert Trainer._folding(types.SimpleNamespace(half_acc=False)) is (fp32 == '1')
    assert Trainer._folding(types.SimpleNamespace(half_acc=True)) is (half == '1')


def test_fold_job_kind2_carries_cpad(pkg):
    import ctypes
    job = pkg._lib.FoldJob()
    job.kind, job.reserved = 2, 8
    assert ctypes.sizeof(pkg._lib.FoldJob) == 96 and job.reserved == 8
    for name in ('p3d_hconv2d_fwd_infer', 'p3d_hconv2d_fwd_infer_supported'):
        assert name in pkg._lib.SIGNATURES


def test_fwd_infer_supported_query_is_host_only(pkg):
    import ctypes
    L = pkg._lib.lib()
    d = pkg.ops._desc((64, 256, 16, 16), (512, 256, 3, 3), 1, 2, 2)
    assert L.p3d_hconv2d_fwd_infer_supported(ctypes.byref(d)) == 1
    odd = pkg.ops._desc((2, 12, 16, 16), (64, 12, 3, 3), 1, 1, 1)                  # fp16 NHWC needs channel counts that are multiples of 8
    assert L.p3d_hconv2d_fwd_infer_supported(ctypes.byref(odd)) == 0
    assert L.p3d_hconv2d_fwd_infer_supported(None) == 0
