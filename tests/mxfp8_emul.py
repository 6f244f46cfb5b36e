"""MXFP8 emulation in torch (OCP MX v1.0, e4m3fn elements, 32-element blocks along the last dimension): the rule of fold kind 3 and of
p3d_f8conv2d_fwd_infer.  e = floor(log2(amax)) (exact, from frexp), scale byte E8M0 = clamp(e - 8 + 127, 0, 254), X = 2^(byte - 127),
q = e4m3fn(RNE(clamp(v / X, -448, 448))); amax == 0: byte 0, every element 0."""
import torch


def quantize(v):
    """v: float32 tensor whose last dimension is a multiple of 32.  Returns (q as float8_e4m3fn, scale bytes uint8 [..., n / 32], X float32 [..., n / 32])."""
    v = v.float()
    shp = v.shape
    b = v.reshape(*shp[:-1], shp[-1] // 32, 32)
    amax = b.abs().amax(-1)
    e = torch.frexp(amax)[1].to(torch.int32) - 1                   # amax = m 2^p with m in [0.5, 1): floor(log2(amax)) = p - 1
    byte = torch.where(amax == 0, torch.zeros_like(e), (e + 119).clamp(0, 254))
    X = torch.pow(2.0, (byte - 127).double()).float()               # (2^-127 is an exact fp32 subnormal)
    q = (b / X[..., None]).clamp(-448, 448).to(torch.float8_e4m3fn)
    return q.reshape(shp), byte.to(torch.uint8), X


def dequantize(q, X):
    """q [..., n] float8_e4m3fn (or its uint8 bits), X [..., n / 32] -> float64 values q * X."""
    if q.dtype == torch.uint8:
        q = q.view(torch.float8_e4m3fn)
    shp = q.shape
    v = q.double().reshape(*shp[:-1], shp[-1] // 32, 32) * X.double()[..., None]
    return v.reshape(shp)


def scale_of(byte):
    return torch.pow(2.0, (byte.to(torch.int32) - 127).double())
