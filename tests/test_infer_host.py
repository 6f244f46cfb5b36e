"""infer.fold refusals (no GPU needed): a BatchNorm in training mode, a -half_acc model, parameters off the HIP device."""
import pytest


def _model(pkg, *extra):
    args = pkg.opts.parse(['-model', 'resnet18', '-suffix', 't', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1',
                           '-num_joints', '17', '-side_in', '128'] + list(extra))
    return pkg.depth_main.create_model(args)[0]


def test_fold_refuses_training_batchnorm(pkg):
    model = _model(pkg).eval()
    model.layer2[1].bn2.train()
    with pytest.raises(pkg._lib.P3DError, match='training mode'):
        pkg.infer.fold(model)


def test_fold_refuses_half_model(pkg):
    model = _model(pkg).eval()
    model._p3d_half = True
    with pytest.raises(pkg._lib.P3DError, match='half_acc'):
        pkg.infer.fold(model)


def test_fold_refuses_host_parameters(pkg):
    with pytest.raises(pkg._lib.P3DError, match='HIP device'):
        pkg.infer.fold(_model(pkg).eval())


def test_fold_job_layout(pkg):
    import ctypes
    assert ctypes.sizeof(pkg._lib.FoldJob) == 96
    assert 'p3d_fx_fold_bn_images' in pkg._lib.SIGNATURES and 'p3d_stem_tail_infer' in pkg._lib.SIGNATURES
