"""Writes tests/golden/conv_queries.json: what every host-only convolution query of the library answers over a descriptor sweep, under each setting of
the switches the answers depend on.  tests/test_conv_queries_host.py holds the library to the recorded answers, so a change to the dispatch code that moves
a verdict or a workspace size shows up as a named (descriptor, query) pair.  Run once against the library whose answers are to be kept:

    python tests/golden/make_conv_queries.py

Needs the built library only (no GPU).  The file: QUERIES / BLOCK_QUERIES name the columns, CONFIGS the settings (x3 switch, any-width switch, forced split
count); a row is [descriptor, answers], the descriptor 12 integers (N C H W K R stride pad dil c_offset c_total accumulate; a block: index into
geometry_table.BLOCKS, N, H, W, masked), the answers one list of integers per setting -- or the index of an earlier setting with the same list."""
import ctypes
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (TESTS, os.path.dirname(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)
PATH = os.path.join(HERE, 'conv_queries.json')

QUERIES = ['conv2d_fwd_workspace_bytes', 'conv2d_dgrad_workspace_bytes', 'conv2d_wgrad_workspace_bytes', 'conv2d_bn_eval_fwd_workspace_bytes',
           'conv2d_fwd_any_supported', 'conv2d_dgrad_any_supported', 'conv2d_wgrad_any_supported', 'fx_conv_img_supported',
           'fx_conv_img_workspace_bytes(0)', 'fx_conv_img_workspace_bytes(1)', 'fx_conv_img_workspace_bytes(2)',
           'fx_conv_fwd_infer_supported(0)', 'fx_conv_fwd_infer_supported(1)', 'fx_conv_fwd_infer_any_supported', 'fx_conv_fwd_infer_masked_supported',
           'fx_conv_fwd_infer_masked_any_supported', 'fx_conv_fwd_infer_workspace_bytes', 'fx_conv_fwd_infer_any_workspace_bytes',
           'fx_conv_fwd_infer_masked_any_workspace_bytes']
BLOCK_QUERIES = ['block_supported', 'block_workspace_bytes', 'main_bytes', 'side_bytes']
# (p3d_x3_enable, p3d_x3_any_enable, forced split count of p3d_fx_tune(1, n) and p3d_fx_tune(0, n))
CONFIGS = [(1, 0, 0), (1, 1, 0), (0, 0, 0), (0, 1, 0), (1, 1, 3)]

CHANNELS = (16, 32, 48, 64, 80, 96, 112, 120, 128, 160, 272)
MAPS = (16, 24, 18, 17)                  # 8k, 4k, 4k + 2, odd


def _same(r, dil=1):
    return dil * (r - 1) // 2


def sweep():
    """the descriptors: (N, C, H, W, K, R, stride, pad, dil, c_offset, c_total, accumulate)"""
    import geometry_table as T
    from test_train_anysize_host import RESNET
    rows = []

    def add(n, c, h, w, k, r, stride=1, pad=None, dil=1, c_offset=0, c_total=None, accumulate=0):
        row = (n, c, h, w, k, r, stride, _same(r, dil) if pad is None else pad, dil, c_offset, c if c_total is None else c_total, accumulate)
        if row not in rows:
            rows.append(row)

    for g in T.ROWS:
        add(g.n, g.c, g.h, g.w, g.k, g.r, g.stride, g.pad, g.dil)
    for c, k, h, r, stride, pad, dil in RESNET:
        for n in (2, 64):
            add(n, c, h, h, k, r, stride, pad, dil)
    for c in CHANNELS:                          # channel edges: each axis alone, the diagonal, and every pair around the thresholds (64, 96), on aligned maps;
        for k in CHANNELS:                      # each axis alone on an odd one
            if 128 in (c, k) or c == k or (48 <= c <= 112 and 48 <= k <= 112):
                add(2, c, 16, 16, k, 1)
                add(3, c, 12, 20, k, 3)
            if 128 in (c, k):
                add(2, c, 17, 17, k, 3)
    for h in MAPS:                              # maps: H and W each of 8k, 4k, 4k + 2 and odd
        for w in MAPS:
            add(2, 128, h, w, 128, 3)
            add(2, 128, h, w, 128, 3, 2)
            add(2, 128, h, w, 128, 1, 2)
    for r in (1, 2, 3, 5, 7):                   # filters and strides
        for stride in (1, 2, 3):
            for h, w in ((24, 16), (16, 18), (17, 15)):
                add(2, 128, h, w, 128, r, stride)
            add(2, 64, 24, 16, 256, r, stride, pad=0)
    add(2, 128, 24, 16, 128, 3, 2, dil=2, pad=2)
    add(2, 128, 24, 16, 128, 3, 1, dil=2, pad=2)
    for h, w in ((16, 16), (17, 17)):           # channel windows of a wider weight
        for off, tot in ((0, 256), (128, 256), (64, 192), (0, 128)):
            for r in (1, 3):
                add(2, 128, h, w, 128, r, c_offset=off, c_total=tot)
    add(2, 64, 16, 16, 128, 3, c_offset=64, c_total=128)
    for shape in ((2, 128, 16, 16, 128, 3, 1), (2, 128, 17, 17, 128, 3, 1), (2, 128, 16, 16, 128, 1, 2), (2, 64, 16, 16, 64, 3, 1), (1, 2048, 8, 12, 272, 3, 1),
                  (2, 256, 16, 16, 256, 3, 2)):
        add(*shape, accumulate=1)
    for n in (1023, 1024, 4095, 4096):          # either side of 2^29 and 2^31 elements (128 channels of 64 x 64 = 2^19 per image)
        add(n, 128, 64, 64, 128, 1)
        add(n, 128, 64, 64, 128, 3)
    add(1023, 128, 64, 64, 256, 1)              # the output alone beyond 2^29
    return rows


def block_sweep():
    """(index into geometry_table.BLOCKS, N, H, W, masked)"""
    import geometry_table as T
    return [(i, n, h, w, m) for i in range(len(T.BLOCKS)) for h, w in T.BLOCK_MAPS for n in (1, 3) for m in (0, 1)]


def desc(pkg, row):
    n, c, h, w, k, r, stride, pad, dil, c_offset, c_total, accumulate = row
    return pkg.ops._desc((n, c, h, w), (k, c_total, r, r), stride, pad, dil, c_offset, c_total, accumulate)


def block_desc(pkg, row):
    import geometry_table as T
    i, n, h, w, masked = row
    kind, inplanes, planes, stride, dil, with_ds = T.BLOCKS[i]
    tr = pkg._trunk
    cls = tr.Bottleneck if kind == 'bottleneck' else tr.BasicBlock
    ds = None
    if with_ds:
        ds = tr.Sequential(pkg.nn.Conv2d(inplanes, planes * cls.expansion, kernel_size=1, stride=stride, bias=False), pkg.nn.BatchNorm2d(planes * cls.expansion))
    block = cls(inplanes, planes, stride, dil, ds, partial=True) if masked else cls(inplanes, planes, stride, dil, ds)
    return pkg.ops_block._Plan(block, (n, inplanes, h, w), masked=bool(masked)).desc


def answers(L, d):
    b = ctypes.byref(d)
    return [L.p3d_conv2d_fwd_workspace_bytes(b), L.p3d_conv2d_dgrad_workspace_bytes(b), L.p3d_conv2d_wgrad_workspace_bytes(b), L.p3d_conv2d_bn_eval_fwd_workspace_bytes(b),
            L.p3d_conv2d_fwd_any_supported(b), L.p3d_conv2d_dgrad_any_supported(b), L.p3d_conv2d_wgrad_any_supported(b), L.p3d_fx_conv_img_supported(b),
            L.p3d_fx_conv_img_workspace_bytes(b, 0), L.p3d_fx_conv_img_workspace_bytes(b, 1), L.p3d_fx_conv_img_workspace_bytes(b, 2),
            L.p3d_fx_conv_fwd_infer_supported(b, 0), L.p3d_fx_conv_fwd_infer_supported(b, 1), L.p3d_fx_conv_fwd_infer_any_supported(b),
            L.p3d_fx_conv_fwd_infer_masked_supported(b), L.p3d_fx_conv_fwd_infer_masked_any_supported(b), L.p3d_fx_conv_fwd_infer_workspace_bytes(b),
            L.p3d_fx_conv_fwd_infer_any_workspace_bytes(b), L.p3d_fx_conv_fwd_infer_masked_any_workspace_bytes(b)]


def block_answers(L, d):
    m, s = ctypes.c_size_t(), ctypes.c_size_t()
    ok = L.p3d_block_supported(ctypes.byref(d))
    rc = L.p3d_block_workspace_bytes(ctypes.byref(d), ctypes.byref(m), ctypes.byref(s))
    return [ok, rc, m.value, s.value]


class config:
    """the library under one of CONFIGS; every switch is put back on exit (the forced split counts have no getter: 0, the built-in plan, is their resting state)"""

    def __init__(self, L, cfg):
        self.L, self.cfg = L, cfg

    def __enter__(self):
        x3, any_width, splits = self.cfg
        self.before = (self.L.p3d_x3_enable(x3), self.L.p3d_x3_any_enable(any_width))
        self.L.p3d_fx_tune(1, splits)
        self.L.p3d_fx_tune(0, splits)

    def __exit__(self, *exc):
        self.L.p3d_fx_tune(1, 0)
        self.L.p3d_fx_tune(0, 0)
        self.L.p3d_x3_enable(self.before[0])
        self.L.p3d_x3_any_enable(self.before[1])


def table(pkg, rows, make, ask):
    L = pkg._lib.lib()
    descs = [make(pkg, r) for r in rows]
    per_cfg = []
    for cfg in CONFIGS:
        with config(L, cfg):
            per_cfg.append([ask(L, d) for d in descs])
    out = []
    for i, r in enumerate(rows):
        ans = []
        for c in range(len(CONFIGS)):
            a = per_cfg[c][i]
            same = [j for j in range(c) if per_cfg[j][i] == a]
            ans.append(same[0] if same else a)
        out.append([list(r), ans])
    return out


def main():
    pkg = importlib.import_module('3d-pose-estimation-with-previleged-information_amd')
    doc = dict(queries=QUERIES, block_queries=BLOCK_QUERIES, configs=[list(c) for c in CONFIGS], rows=table(pkg, sweep(), desc, answers),
               block_rows=table(pkg, block_sweep(), block_desc, block_answers))
    with open(PATH, 'w') as f:
        f.write('{\n')
        for key in ('queries', 'block_queries', 'configs'):
            f.write('"%s": %s,\n' % (key, json.dumps(doc[key])))
        for key in ('rows', 'block_rows'):
            f.write('"%s": [\n%s\n]%s\n' % (key, ',\n'.join(json.dumps(r, separators=(',', ':')) for r in doc[key]), ',' if key == 'rows' else ''))
        f.write('}\n')
    print('%s: %d descriptors, %d blocks, %d bytes' % (PATH, len(doc['rows']), len(doc['block_rows']), os.path.getsize(PATH)))


if __name__ == '__main__':
    main()
