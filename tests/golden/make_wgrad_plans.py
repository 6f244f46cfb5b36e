"""Writes tests/golden/wgrad_plans.json: the plan of the x3 weight gradient (the test hook p3d_fx_wgrad_plan: kernel instance, taps per column tile, slabs, K steps per
slab, grid, block order, slab bytes) for every weight-gradient descriptor of make_conv_queries.sweep() the x3 kernels admit, under every operand form, and for a few
stems.  tests/test_wgrad_plan_host.py holds the library to the recorded plans.  Run once against the library whose plans are to be kept:

    python tests/golden/make_wgrad_plans.py

(The committed table was written from a build of the commit before fx_wgrad_plan existed, with the hook added to it by hand as a transcription of that commit's rules:
see tests/test_wgrad_plan_host.py.)  Needs the built library only (no GPU).  The file: FIELDS names the 16 integers of a record, FORMS / STEM_FORMS the operand bits asked (bit 0 dy image, 1 x image, 2 row
images, 3 factor of dy, 4 factor of x, 5 any map width, 6 the stem), CONFIGS the p3d_fx_tune settings.  Nothing is left out, but every repeated thing is written once
(the plain table is 160 KB): a record is cut into its instance part and its size part, `insts` and `sizes` hold each distinct part once; a row is [descriptor, answers],
an answer per setting being [i, s, local] -- inst_patterns[i] gives per form the index into `insts` (-1: the hook refuses the operands), size_patterns[s] per form
the index into `local`, whose entries index `sizes` -- or the index of an earlier setting with the same answer.  expand() undoes it."""
import ctypes
import importlib
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (TESTS, os.path.dirname(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)
PATH = os.path.join(HERE, 'wgrad_plans.json')

_spec = importlib.util.spec_from_file_location('make_conv_queries', os.path.join(HERE, 'make_conv_queries.py'))
queries = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(queries)

FIELDS = ['family', 'aimg', 'bimg', 'masked', 'taps', 'rows', 'tile_taps', 'splits', 'spb', 'grid_x', 'grid_y', 'grid_z', 'order', 'tapm', 'slab_bytes_lo', 'slab_bytes_hi']
SPLIT = FIELDS.index('splits')          # a record = its instance part FIELDS[:SPLIT] + its size part FIELDS[SPLIT:]
DY_IMG, X_IMG, ROWS, DY_FACTOR, X_FACTOR, ANY, STEM = 1, 2, 4, 8, 16, 32, 64
# what the launcher takes: fp32 / fp32, dy image (planes, rows), two images (planes, rows), a partial convolution fp32-fed and with a dy image; at any map width fp32-fed
# dense and partial, two images (the row flag is not looked at there) -- and what it refuses: an x image alone, one factor, a factor beside its image, rows without an
# image, rows of a partial convolution; at any map width one image, one factor, factors beside images
TAKEN = [0, DY_IMG, DY_IMG | ROWS, DY_IMG | X_IMG, DY_IMG | X_IMG | ROWS, DY_FACTOR | X_FACTOR, DY_IMG | X_FACTOR,
         ANY, ANY | DY_FACTOR | X_FACTOR, ANY | DY_IMG | X_IMG, ANY | DY_IMG | X_IMG | ROWS]
REFUSED = [X_IMG, DY_FACTOR, DY_IMG | X_IMG | DY_FACTOR, ROWS, DY_IMG | ROWS | X_FACTOR, ANY | DY_IMG, ANY | DY_FACTOR, ANY | DY_IMG | X_IMG | DY_FACTOR | X_FACTOR]
FORMS = TAKEN + REFUSED
STEM_FORMS = [STEM, STEM | DY_FACTOR]
# (p3d_fx_tune(0, n): forced slab count; p3d_fx_tune(2, n): forced block target)
CONFIGS = [(0, 0), (3, 0), (0, 512)]
# (N, Cin, H, W, K) of a stem: the smallest map, one that splits, the training shape, the widest K
STEMS = [(2, 3, 32, 32, 64), (4, 1, 64, 64, 64), (64, 3, 256, 256, 64), (2, 3, 32, 64, 128), (8, 4, 128, 128, 32)]
# beyond make_conv_queries.sweep(): the small shapes of the GPU checks (N = 4), and batch-64 layers on whole 16-pixel rows, where the block-target table decides the slabs
EXTRA = [(4, c, h, h, k, r, 1, r // 2, 1, 0, c, 0) for h in (16, 17) for r in (1, 3) for c, k in ((64, 64), (64, 128), (128, 64), (128, 272), (272, 128))] + \
        [(64, c, h, h, k, 3, 1, 1, 1, 0, c, 0) for c, k, h in ((64, 64, 64), (64, 128, 32), (128, 128, 32), (256, 256, 16), (512, 512, 16))]


def sweep():
    rows = list(queries.sweep())
    return rows + [r for r in EXTRA if r not in rows]


def stem_desc(pkg, row):
    n, cin, h, w, k = row
    return pkg.ops._desc((n, cin, h, w), (k, cin, 7, 7), 2, 3, 1)


def plan(L, d, operands):
    """the record as a tuple, or None where the hook refuses"""
    out = (ctypes.c_int32 * len(FIELDS))()
    return tuple(out) if L.p3d_fx_wgrad_plan(ctypes.byref(d), operands, out) == 0 else None


class config:
    def __init__(self, L, cfg):
        self.L, self.cfg = L, cfg

    def __enter__(self):
        self.L.p3d_fx_tune(0, self.cfg[0])
        self.L.p3d_fx_tune(2, self.cfg[1])

    def __exit__(self, *exc):
        self.L.p3d_fx_tune(0, 0)
        self.L.p3d_fx_tune(2, 0)


def expand(doc, answers):
    """the records of one row per setting and form (None: refused), as plan() returns them"""
    out = []
    for a in answers:
        if isinstance(a, int):
            out.append(out[a])
            continue
        i, s, local = a
        out.append([None if q < 0 else tuple(doc['insts'][q] + doc['sizes'][local[z]]) for q, z in zip(doc['inst_patterns'][i], doc['size_patterns'][s])])
    return out


def admitted(L, d):
    """an x3 weight gradient takes the shape: aligned or at any map width (fp32 operands are taken wherever the shape is)"""
    return plan(L, d, 0) is not None or plan(L, d, ANY) is not None


def table(L, descs, forms):
    """per descriptor and setting, the record of each form (None: refused)"""
    per_cfg = []
    for cfg in CONFIGS:
        with config(L, cfg):
            per_cfg.append([[plan(L, d, f) for f in forms] for d in descs])
    return per_cfg


def main():
    pkg = importlib.import_module('3d-pose-estimation-with-previleged-information_amd')
    L = pkg._lib.lib()
    was = L.p3d_x3_enable(1)
    try:
        rows = [r for r in sweep() if admitted(L, queries.desc(pkg, r))]
        conv = table(L, [queries.desc(pkg, r) for r in rows], FORMS)
        stem = table(L, [stem_desc(pkg, r) for r in STEMS], STEM_FORMS)
    finally:
        L.p3d_x3_enable(was)
    doc = dict(fields=FIELDS, forms=FORMS, stem_forms=STEM_FORMS, configs=[list(c) for c in CONFIGS], insts=[], sizes=[], inst_patterns=[], size_patterns=[])

    def index(key, item):
        if item not in doc[key]:
            doc[key].append(item)
        return doc[key].index(item)

    def pack(keys, per_cfg):
        out = []
        for i, key in enumerate(keys):
            ans, full = [], []
            for c in range(len(CONFIGS)):
                recs = per_cfg[c][i]
                sizes = []                           # this answer's distinct size parts, as indices into doc['sizes'], in order of first use
                for p in recs:
                    if p is not None and index('sizes', list(p[SPLIT:])) not in sizes:
                        sizes.append(index('sizes', list(p[SPLIT:])))
                a = [index('inst_patterns', [-1 if p is None else index('insts', list(p[:SPLIT])) for p in recs]),
                     index('size_patterns', [-1 if p is None else sizes.index(index('sizes', list(p[SPLIT:]))) for p in recs]), sizes]
                same = [j for j in range(c) if full[j] == a]
                ans.append(same[0] if same else a)
                full.append(a)
            out.append([list(key), ans])
        return out

    doc['rows'], doc['stem_rows'] = pack(rows, conv), pack(STEMS, stem)
    with open(PATH, 'w') as f:
        f.write('{\n')
        for key in ('fields', 'forms', 'stem_forms', 'configs', 'insts', 'inst_patterns', 'size_patterns'):
            f.write('"%s": %s,\n' % (key, json.dumps(doc[key], separators=(',', ':'))))
        for key in ('rows', 'stem_rows', 'sizes'):
            f.write('"%s": [\n%s\n]%s\n' % (key, ',\n'.join(json.dumps(r, separators=(',', ':')) for r in doc[key]), '' if key == 'sizes' else ','))
        f.write('}\n')
    print('%s: %d descriptors, %d stems, %d instance parts, %d size parts, %d bytes' % (PATH, len(rows), len(STEMS), len(doc['insts']), len(doc['sizes']), os.path.getsize(PATH)))


if __name__ == '__main__':
    main()
