"""The geometry table of the fast convolution paths: rectangular maps, both (H, W) orders, batches that end a pixel tile mid-row, paddings other
than dil * (R - 1) / 2, and the rectangles the x3 predicates refuse.  One table for every family (tests/test_geometry_gpu.py drives the kernels with
it, tests/test_geometry_host.py pins each row's admitted / refused verdict to the host-only *_supported queries of the library).

A row is a Geo: batch, channels in / out, map, filter, stride, padding, dilation, and `x3`: the passes of the x3 kernels that take it, as the bits of
p3d_fx_conv_img_supported (1 forward, 2 data gradient, 4 weight gradient).  The fp16 and MXFP8 gather kernels take every row."""
import collections

import torch
import torch.nn.functional as F

Geo = collections.namedtuple('Geo', 'name n c k h w r stride pad dil x3')

ASPECTS = [(24, 40), (40, 24), (8, 48), (48, 8)]            # both orders always; the extreme pair: one 128- / 256-pixel tile spans many rows, or part of one image
SMALL = [(12, 20), (20, 12)]                               # admitted at stride 1, refused at stride 2 (Wo % 4 != 0)

# filter classes over the channel tiles: 128 rows (k 128 / 256), 96 rows (k 272), 64 rows (k 64);  name, c, k, r, stride, dil, n
FILTERS = [('1x1', 256, 128, 1, 1, 1, 1), ('1x1s2', 128, 256, 1, 2, 1, 3), ('3x3', 128, 272, 3, 1, 1, 3), ('3x3s2', 128, 128, 3, 2, 1, 1),
           ('3x3d2', 64, 64, 3, 1, 2, 3), ('5x5', 64, 128, 5, 1, 1, 1)]


def _same(r, dil):
    return dil * (r - 1) // 2


def _rows():
    rows = []
    for h, w in ASPECTS:
        for name, c, k, r, s, dil, n in FILTERS:
            rows.append(Geo('%s_%dx%d_n%d' % (name, h, w, n), n, c, k, h, w, r, s, _same(r, dil), dil, 7))
    for h, w in ASPECTS[:2]:                                 # a batch that fills whole pixel tiles (8 * 24 * 40 = 30 tiles of 256)
        rows.append(Geo('3x3_%dx%d_n8' % (h, w), 8, 128, 128, h, w, 3, 1, 1, 1, 7))
    for h, w in SMALL:
        rows.append(Geo('1x1_%dx%d_n1' % (h, w), 1, 128, 128, h, w, 1, 1, 0, 1, 7))        # 1 * 12 * 20 = 240 pixels: the only tile ends mid-row
        rows.append(Geo('3x3_%dx%d_n3' % (h, w), 3, 64, 128, h, w, 3, 1, 1, 1, 7))
    # split-K plans: >= 1024 reduction channels at few pixels
    rows.append(Geo('splitk_1x1_8x12', 1, 1024, 256, 8, 12, 1, 1, 0, 1, 7))
    rows.append(Geo('splitk_3x3_12x8', 3, 2048, 272, 12, 8, 3, 1, 1, 1, 7))
    # paddings other than "same" whose outputs keep the divisibility rules: 24x40 -> 20x36 / 28x44, and the transposes
    for h, w in ASPECTS[:2]:
        for name, c, k, r, s, pad, dil, n, x3 in [('5x5p0', 64, 128, 5, 1, 0, 1, 3, 7), ('5x5p4', 64, 128, 5, 1, 4, 1, 1, 7), ('3x3d2p0', 128, 128, 3, 1, 0, 2, 3, 7),
                                                  ('3x3d2p4', 128, 272, 3, 1, 4, 2, 1, 7), ('1x1p2', 128, 128, 1, 1, 2, 1, 3, 7),
                                                  # forward and weight gradient admitted, the strided data gradient refused (pad != dil * (R - 1) / 2): 24x40 -> 16x24
                                                  ('3x3s2p5', 128, 128, 3, 2, 5, 1, 3, 5), ('1x1s2p4', 128, 128, 1, 2, 4, 1, 1, 5)]:
            rows.append(Geo('%s_%dx%d_n%d' % (name, h, w, n), n, c, k, h, w, r, s, pad, dil, x3))
    # refused rectangles: the public entry points must fall back and still match the reference
    for h, w in SMALL:
        rows.append(Geo('1x1s2_%dx%d_refused' % (h, w), 3, 128, 128, h, w, 1, 2, 0, 1, 0))
        rows.append(Geo('3x3s2_%dx%d_refused' % (h, w), 1, 128, 128, h, w, 3, 2, 1, 1, 0))
    rows.append(Geo('3x3s2p3_24x40_refused', 3, 128, 128, 24, 40, 3, 2, 3, 1, 0))          # -> 14 x 22
    return rows


ROWS = _rows()
ADMITTED = [g for g in ROWS if g.x3 == 7]
IDS = [g.name for g in ROWS]

# residual blocks: kind, inplanes, planes, stride, dilation, downsample
BLOCKS = [('bottleneck', 512, 128, 1, 1, False), ('bottleneck', 256, 128, 2, 1, True), ('bottleneck', 256, 128, 1, 2, True),
          ('basic', 128, 128, 1, 1, False), ('basic', 128, 256, 2, 1, True)]
BLOCK_MAPS = ASPECTS + SMALL                              # (12, 20) / (20, 12): taken at stride 1, refused at stride 2

STEM_MAPS = [(96, 160), (160, 96), (128, 192), (192, 128)]
NET_MAPS = [(128, 192), (192, 128)]


def out_hw(g):
    return tuple((v + 2 * g.pad - g.dil * (g.r - 1) - 1) // g.stride + 1 for v in (g.h, g.w))


def block_admitted(stride, h, w):
    return (h, w) not in SMALL or stride == 1


def transposed_read(x):
    """The same memory read with H and W exchanged: what a kernel that swaps the two extents sees."""
    n, c, h, w = x.shape
    return x.reshape(n, c, w, h)


def transposition_gap(g, seed=0):
    """max |conv(x) - conv'(x)| / max |conv(x)| in float64, conv' being the same convolution computed on the H/W-exchanged reading of x and its
    result read back as [Ho][Wo]: how far a transposing kernel would land from the reference of row g."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(g.n, min(g.c, 64), g.h, g.w, generator=gen, dtype=torch.float64)
    wt = torch.randn(min(g.k, 32), x.shape[1], g.r, g.r, generator=gen, dtype=torch.float64) / (x.shape[1] * g.r * g.r) ** 0.5
    y = F.conv2d(x, wt, None, g.stride, g.pad, g.dil)
    yt = F.conv2d(transposed_read(x), wt, None, g.stride, g.pad, g.dil).reshape(y.shape)
    return float((y - yt).abs().max() / y.abs().max())
