"""The MXFP8 activation tensor's size, the MX entry point's query, the format decision of the resident walk (infer.resident_forms), fold_fp8's refusals
under resident=True and the P3D_FOLDED_EVAL_FP8_RESIDENT switch (no GPU needed)."""
import ctypes
import types

import pytest
import torch

from test_infer_fp8_host import _model


def test_f8act_bytes(pkg):
    L = pkg._lib.lib()
    assert L.p3d_f8act_bytes(1, 32) == 33
    assert L.p3d_f8act_bytes(2 * 17 * 17, 64) == 578 * 64 + 578 * 2
    assert L.p3d_f8act_bytes(64 * 64 * 64, 256) == 64 * 64 * 64 * 256 + 64 * 64 * 64 * 8
    assert L.p3d_f8act_bytes(1 << 26, 64) == (1 << 32) + (1 << 27)              # 64-bit arithmetic
    assert L.p3d_f8act_bytes(100, 48) == 0
    assert L.p3d_f8act_bytes(0, 64) == 0 and L.p3d_f8act_bytes(-3, 64) == 0 and L.p3d_f8act_bytes(100, 0) == 0 and L.p3d_f8act_bytes(100, -32) == 0


def test_new_names_are_in_signatures(pkg):
    for name in ('p3d_f8act_bytes', 'p3d_f8conv2d_fwd_infer_mx_supported', 'p3d_f8conv2d_fwd_infer_mx'):
        assert name in pkg._lib.SIGNATURES
    assert len(pkg._lib.SIGNATURES['p3d_f8conv2d_fwd_infer_mx'][1]) == 12
    assert pkg._lib.lib().p3d_version() == 100


def test_mx_supported_query_is_host_only(pkg):
    L = pkg._lib.lib()
    q = lambda d, x, y: L.p3d_f8conv2d_fwd_infer_mx_supported(ctypes.byref(d), x, y)
    k136 = pkg.ops._desc((3, 96, 20, 20), (136, 96, 3, 3), 2, 2, 2)
    assert q(k136, 0, 1) == 0 and 'multiple of 32' in L.p3d_last_error().decode() and 'K=136' in L.p3d_last_error().decode()
    assert q(k136, 1, 1) == 0
    assert q(k136, 0, 0) == 1 and q(k136, 1, 0) == 1
    ok = pkg.ops._desc((3, 96, 20, 20), (160, 96, 3, 3), 2, 2, 2)
    assert all(q(ok, x, y) == 1 for x in (0, 1) for y in (0, 1))
    c48 = pkg.ops._desc((2, 48, 16, 16), (64, 48, 3, 3), 1, 1, 1)
    assert all(q(c48, x, y) == 0 for x in (0, 1) for y in (0, 1)) and 'C=48' in L.p3d_last_error().decode()
    assert L.p3d_f8conv2d_fwd_infer_mx_supported(None, 1, 1) == 0
    assert L.p3d_f8conv2d_fwd_infer_mx_supported(None, 0, 0) == 0


def test_mx_entry_refuses_bad_tensor_sets_before_any_launch(pkg):
    """both inputs, no input, no result: refused on the host (the pointers are never read)"""
    L = pkg._lib.lib()
    d = pkg.ops._desc((2, 64, 16, 16), (64, 64, 1, 1), 1, 0, 1)
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    call = lambda x16, xmx, y16, ymx: L.p3d_f8conv2d_fwd_infer_mx(ctypes.byref(d), x16, xmx, p, None, None, None, None, 0, y16, ymx, None)
    assert call(p, p, p, None) != 0 and 'one of the two' in L.p3d_last_error().decode()
    assert call(None, None, p, None) != 0 and 'one of the two' in L.p3d_last_error().decode()
    assert call(p, None, None, None) != 0 and 'no result' in L.p3d_last_error().decode()
    k136 = pkg.ops._desc((2, 64, 16, 16), (136, 64, 1, 1), 1, 0, 1)
    assert L.p3d_f8conv2d_fwd_infer_mx(ctypes.byref(k136), p, None, p, None, None, None, None, 0, None, p, None) != 0
    assert 'multiple of 32' in L.p3d_last_error().decode()


# ---- the format decision on hand-made chains ---------------------------------------------------------------------------------------------------
def _conv(pkg, cin, cout, k, stride=1, dil=1, fp8=True):
    conv = torch.nn.Conv2d(cin, cout, k, stride=stride, padding=dil * (k - 1) // 2, dilation=dil, bias=False)
    return (pkg.infer._F8Conv if fp8 else pkg.infer._HConv)(conv, torch.nn.BatchNorm2d(cout))


def _walk(pkg, chain, shape):
    """the forms of every result of a chain fed an activation of NCHW `shape`"""
    out, x = [], pkg.infer._Act(shape)
    for i, c in enumerate(chain):
        d = c.desc(x)
        out.append(pkg.infer.resident_forms(chain, i, d))
        x = pkg.infer._Act((d.N, d.K, d.Ho, d.Wo))
    return out


def test_resident_forms_bottleneck(pkg):
    chain = [_conv(pkg, 256, 64, 1), _conv(pkg, 64, 64, 3, stride=2), _conv(pkg, 64, 256, 1)]
    assert _walk(pkg, chain, (2, 256, 33, 33)) == [(False, True), (False, True), (True, True)]


def test_resident_forms_basic_block(pkg):
    chain = [_conv(pkg, 64, 128, 3, stride=2), _conv(pkg, 128, 128, 3, dil=2)]
    assert _walk(pkg, chain, (2, 64, 17, 17)) == [(False, True), (True, True)]


def test_resident_forms_next_conv_is_not_fp8(pkg):
    chain = [_conv(pkg, 64, 64, 1), _conv(pkg, 64, 64, 3, fp8=False), _conv(pkg, 64, 256, 1)]
    assert _walk(pkg, chain, (2, 64, 16, 16)) == [(True, False), (True, False), (True, True)]


def test_resident_forms_channel_counts_the_mx_forms_refuse(pkg):
    """K = 136: this conv's result cannot be MX (no 32-channel blocks), and the next conv (C = 136) is no fp8 conv's shape either; a last conv with such
    a K writes fp16 only; an fp16 conv at the end of a chain writes fp16 only"""
    chain = [_conv(pkg, 64, 136, 1), _conv(pkg, 136, 64, 3, fp8=False), _conv(pkg, 64, 136, 1)]
    assert _walk(pkg, chain, (2, 64, 16, 16)) == [(True, False), (True, False), (True, False)]
    chain = [_conv(pkg, 64, 64, 1), _conv(pkg, 64, 40, 3, fp8=False)]
    assert _walk(pkg, chain, (2, 64, 16, 16)) == [(True, False), (True, False)]
    one = [_conv(pkg, 1024, 512, 1)]                                     # the Fusion 1x1: a chain of one, both forms
    assert pkg.infer.resident_forms(one, 0, one[0].desc(pkg.infer._Act((2, 1024, 16, 16))), False) == (True, True)


# ---- refusals, the switch --------------------------------------------------------------------------------------------------------------------
def test_fold_fp8_resident_refuses_training_batchnorm(pkg):
    model = _model(pkg).eval()
    model.layer2[0].bn1.train()
    with pytest.raises(pkg._lib.P3DError, match='infer.fold_fp8: BatchNorm .* is in training mode'):
        pkg.infer.fold_fp8(model, resident=True)


def test_fold_fp8_resident_refuses_host_parameters(pkg):
    with pytest.raises(pkg._lib.P3DError, match='infer.fold_fp8: parameters must be fp32 masters on the HIP device'):
        pkg.infer.fold_fp8(_model(pkg, '-half_acc').eval(), resident=True)


@pytest.mark.parametrize('fp8,resident,on', [('1', '1', True), ('0', '1', False), (None, '1', False), ('1', '0', False), ('1', None, False), ('1', 'yes', False)])
def test_resident_switch_acts_only_with_the_fp8_switch(pkg, monkeypatch, fp8, resident, on):
    for name, value in (('P3D_FOLDED_EVAL_FP8', fp8), ('P3D_FOLDED_EVAL_FP8_RESIDENT', resident)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    monkeypatch.setenv('P3D_FOLDED_EVAL', '0')
    monkeypatch.setenv('P3D_FOLDED_EVAL_HALF', '1')
    assert pkg.infer.fp8_resident_enabled() is on
    seen = []
    monkeypatch.setattr(pkg.infer, 'fold_fp8', lambda net, **kw: seen.append(kw) or 'fp8')
    monkeypatch.setattr(pkg.infer, 'fold_half', lambda net: seen.append('half') or 'half')
    fake = types.SimpleNamespace(half_acc=True)
    Trainer = pkg.depth_train.Trainer
    assert Trainer._folding(fake) is True                              # (P3D_FOLDED_EVAL_HALF=1: the resident switch alone changes nothing)
    got = Trainer._fold(fake, object())
    if fp8 == '1':
        assert got == 'fp8' and seen == [dict(resident=True) if on else {}]      # (off: fold_fp8(net), exactly as without the switch)
    else:
        assert got == 'half' and seen == ['half']
