"""The MXFP8 emulation on hand-made blocks, infer.fold_fp8 refusals, the P3D_FOLDED_EVAL_FP8 switch and its precedence, fold kind 3 and the fp8
entry point's query (no GPU needed)."""
import ctypes
import types

import pytest
import torch

from mxfp8_emul import dequantize, quantize


def _model(pkg, *extra):
    args = pkg.opts.parse(['-model', 'resnet18', '-suffix', 't', '-data_name', 'h36m', '-save_path', '/tmp/p3d', '-criterion', 'SmoothL1',
                           '-num_joints', '17', '-side_in', '128'] + list(extra))
    return pkg.depth_main.create_model(args)[0]


# ---- the emulation itself ----------------------------------------------------------------------------------------------------------------
def test_emulation_power_of_two_amax():
    v = torch.zeros(32)
    v[0], v[1], v[2] = 4.0, -1.0, 0.25                              # amax 2^2: X = 2^-6, 4 / X = 256 exact
    q, byte, X = quantize(v)
    assert int(byte[0]) == 2 - 8 + 127 and float(X[0]) == 2.0 ** -6
    assert torch.equal(dequantize(q, X).float(), v)


def test_emulation_clamps_the_top_octave():
    v = torch.zeros(32)
    v[0], v[1], v[2], v[3] = 1.0, 0.9375, -0.96875, 0.875           # / X = 2^8 * v: 256, 240, -248, 224; amax 1 -> X = 2^-8
    q, byte, X = quantize(v)
    d = dequantize(q, X).float()
    assert float(d[0]) == 1.0 and float(d[3]) == 0.875
    w = torch.zeros(32)
    w[0], w[1], w[2] = 1.96875, 1.8125, -1.75                       # amax in [1, 2): / X = 504, 464, -448: 448 is the largest e4m3 value
    q, byte, X = quantize(w)
    d = dequantize(q, X).float()
    assert int(byte[0]) == 119 and float(d[0]) == 1.75 and float(d[1]) == 1.75 and float(d[2]) == -1.75
    assert not torch.isnan(q.float()).any()


def test_emulation_keeps_e4m3_subnormals():
    v = torch.zeros(32)
    v[0] = 256.0                                                    # X = 1
    v[1], v[2], v[3] = 2.0 ** -9, 3 * 2.0 ** -9, 2.0 ** -10         # e4m3 subnormals (multiples of 2^-9); 2^-10 is a tie, to even (0)
    v[4] = 5 * 2.0 ** -10                                           # 2.5 * 2^-9 -> 2 * 2^-9 (even)
    q, byte, X = quantize(v)
    assert float(X[0]) == 1.0
    d = dequantize(q, X).float()
    assert float(d[1]) == 2.0 ** -9 and float(d[2]) == 3 * 2.0 ** -9 and float(d[3]) == 0.0 and float(d[4]) == 2 * 2.0 ** -9


def test_emulation_zero_block():
    v = torch.zeros(64)
    v[40] = 3.0
    q, byte, X = quantize(v)
    assert int(byte[0]) == 0 and torch.all(q[:32].float() == 0)
    assert int(byte[1]) == 1 - 8 + 127 and float(dequantize(q, X)[40]) == 3.0


def test_emulation_of_fp16_data_never_clamps_the_scale():
    v = torch.tensor([65504.0, 2.0 ** -24] + [0.0] * 30)
    _, byte, _ = quantize(v)
    assert int(byte[0]) == 15 + 119
    _, byte, _ = quantize(torch.tensor([2.0 ** -24] + [0.0] * 31))
    assert int(byte[0]) == -24 + 119


# ---- fold_fp8 refusals, the switch --------------------------------------------------------------------------------------------------------
def test_fold_fp8_refuses_training_batchnorm(pkg):
    model = _model(pkg).eval()
    model.layer2[0].bn1.train()
    with pytest.raises(pkg._lib.P3DError, match='training mode'):
        pkg.infer.fold_fp8(model)


def test_fold_fp8_refuses_host_parameters(pkg):
    with pytest.raises(pkg._lib.P3DError, match='infer.fold_fp8: parameters must be fp32 masters on the HIP device'):
        pkg.infer.fold_fp8(_model(pkg, '-half_acc').eval())


@pytest.mark.parametrize('value,on', [(None, False), ('0', False), ('1', True), ('yes', False), ('', False)])
def test_folded_eval_fp8_switch(pkg, monkeypatch, value, on):
    if value is None:
        monkeypatch.delenv('P3D_FOLDED_EVAL_FP8', raising=False)
    else:
        monkeypatch.setenv('P3D_FOLDED_EVAL_FP8', value)
    monkeypatch.delenv('P3D_FOLDED_EVAL', raising=False)
    monkeypatch.delenv('P3D_FOLDED_EVAL_HALF', raising=False)
    assert pkg.infer.fp8_enabled() is on
    Trainer = pkg.depth_train.Trainer
    assert Trainer._folding(types.SimpleNamespace(half_acc=True)) is on
    assert Trainer._folding(types.SimpleNamespace(half_acc=False)) is on


@pytest.mark.parametrize('half_acc', [False, True])
@pytest.mark.parametrize('fp32,half', [('1', '0'), ('0', '1'), ('1', '1'), ('0', '0')])
def test_fp8_switch_takes_precedence(pkg, monkeypatch, half_acc, fp32, half):
    monkeypatch.setenv('P3D_FOLDED_EVAL', fp32)
    monkeypatch.setenv('P3D_FOLDED_EVAL_HALF', half)
    monkeypatch.setenv('P3D_FOLDED_EVAL_FP8', '1')
    seen = []
    monkeypatch.setattr(pkg.infer, 'fold_fp8', lambda net: seen.append('fp8') or 'fp8')
    monkeypatch.setattr(pkg.infer, 'fold_half', lambda net: seen.append('half') or 'half')
    monkeypatch.setattr(pkg.infer, 'fold', lambda net: seen.append('fp32') or 'fp32')
    fake = types.SimpleNamespace(half_acc=half_acc)
    assert pkg.depth_train.Trainer._folding(fake) is True
    assert pkg.depth_train.Trainer._fold(fake, object()) == 'fp8' and seen == ['fp8']


def test_fp8_switch_off_leaves_the_other_switches(pkg, monkeypatch):
    monkeypatch.setenv('P3D_FOLDED_EVAL_FP8', '0')
    monkeypatch.setenv('P3D_FOLDED_EVAL', '0')
    monkeypatch.setenv('P3D_FOLDED_EVAL_HALF', '1')
    monkeypatch.setattr(pkg.infer, 'fold_half', lambda net: 'half')
    fake = types.SimpleNamespace(half_acc=True)
    assert pkg.depth_train.Trainer._fold(fake, object()) == 'half'
    assert pkg.depth_train.Trainer._folding(types.SimpleNamespace(half_acc=False)) is False


# ---- fold kind 3 and the entry point's query -----------------------------------------------------------------------------------------------
def test_fold_job_kind3_carries_cpad(pkg):
    for name in ('p3d_f8conv2d_fwd_infer', 'p3d_f8conv2d_fwd_infer_supported', 'p3d_f8conv2d_weight_bytes'):
        assert name in pkg._lib.SIGNATURES
    conv = torch.nn.Conv2d(64, 128, 3, padding=1, bias=False)
    c = pkg.infer._F8Conv(conv, torch.nn.BatchNorm2d(128))
    assert c.layout(0) > 0
    j = c.job(torch.zeros(16, dtype=torch.uint8))
    assert j.kind == 3 and j.reserved % 32 == 0 and j.reserved >= j.C == 64 and j.RS == 9
    L = pkg._lib.lib()
    assert L.p3d_f8conv2d_weight_bytes(128, 64, 9) == 128 * 9 * 64 + 128 * 9 * 2
    assert L.p3d_f8conv2d_weight_bytes(128, 48, 9) == 0


def test_f8_supported_query_is_host_only(pkg):
    L = pkg._lib.lib()
    ok = pkg.ops._desc((64, 256, 16, 16), (512, 256, 3, 3), 1, 2, 2)
    assert L.p3d_f8conv2d_fwd_infer_supported(ctypes.byref(ok)) == 1
    for desc, why in ((pkg.ops._desc((2, 48, 16, 16), (64, 48, 3, 3), 1, 1, 1), 'multiple of 32'),
                      (pkg.ops._desc((2, 64, 16, 16), (68, 64, 1, 1), 1, 0, 1), 'multiple of 8'),
                      (pkg.ops._desc((2, 64, 16, 16), (64, 64, 1, 1), 1, 0, 1, accumulate=1), 'accumulate')):
        assert L.p3d_f8conv2d_fwd_infer_supported(ctypes.byref(desc)) == 0
        assert why in L.p3d_last_error().decode()
    assert L.p3d_f8conv2d_fwd_infer_supported(None) == 0
