"""The folded partial-convolution entry points (p3d_fx_conv_fwd_infer_masked[_supported]) (no GPU needed)."""
import ctypes


def test_masked_infer_symbols_are_bound(pkg):
    for name in ('p3d_fx_conv_fwd_infer_masked', 'p3d_fx_conv_fwd_infer_masked_supported'):
        assert name in pkg._lib.SIGNATURES


def test_masked_infer_supported_query_is_host_only(pkg):
    L = pkg._lib.lib()
    layer1 = pkg.ops._desc((64, 64, 64, 64), (64, 64, 3, 3), 1, 1, 1)                # partial_depthnet layer1's 3x3 at 256^2
    assert L.p3d_fx_conv_fwd_infer_masked_supported(ctypes.byref(layer1)) == 1
    window = pkg.ops._desc((2, 64, 16, 16), (64, 128, 3, 3), 1, 1, 1, c_offset=64, c_total=128)
    assert L.p3d_fx_conv_fwd_infer_masked_supported(ctypes.byref(window)) == 0
    narrow = pkg.ops._desc((2, 64, 16, 16), (32, 64, 3, 3), 1, 1, 1)              # K = 32: the dense entry takes it, the masked one does not
    assert L.p3d_fx_conv_fwd_infer_supported(ctypes.byref(narrow), 0) == 1
    assert L.p3d_fx_conv_fwd_infer_masked_supported(ctypes.byref(narrow)) == 0
    accumulate = pkg.ops._desc((2, 64, 16, 16), (64, 64, 3, 3), 1, 1, 1, accumulate=1)
    assert L.p3d_fx_conv_fwd_infer_masked_supported(ctypes.byref(accumulate)) == 0
    assert L.p3d_fx_conv_fwd_infer_masked_supported(None) == 0

