"""The tables of profiles/row_images.md sections 4 and 5, as markdown.

  row_images_tables.py kernels PARENT_DIR NEW_DIR STEPS
      two rocprofv3 --kernel-trace --stats csv directories (every kernel, no cut), folded by kernel family: a row-fed instance with its plane-fed twin
      (fx_act_image_kernel<4 | 5 | 6> with <0 | 1 | 2>, the ROWS argument of the conv kernels dropped), the shapes and K orders of one epilogue together
  row_images_tables.py shapes PLANES_R1 PLANES_R2 ROWS_R1 ROWS_R2
      outputs of tools/conv_bench.py --img (three-plane operands) and --img --rows, two rounds each: per shape, per stage, and the verdict column
      ("faster" / "SLOWER": both rounds of one format beat both of the other)"""
import collections
import csv
import glob
import os
import re
import sys


def family(name):
    name = re.sub(r'\(.*', '', name).replace('void ', '').replace('p3d::', '')
    if name.startswith('fx_act_image_kernel<'):
        return 'fx_act_image_kernel mode %d' % (int(re.search(r'<(\d)', name).group(1)) % 4)
    if name.startswith('fx_act_image_pair'):
        return 'fx_act_image_pair_kernel'
    m = re.match(r'fx_conv_kernel<(\d), (\d), (\d)', name)
    if m:
        return 'fx_conv_kernel<%s, %s, %s, ..> (%s)' % (m.group(1), m.group(2), m.group(3), 'image-fed' if m.group(1) == '1' else 'fp32-fed')
    m = re.match(r'fx16_conv_kernel<(\d+), (\d)', name)
    if m:
        return 'fx16_conv_kernel<%s, %s, ..>' % (m.group(1), m.group(2))
    m = re.match(r'fx_wgrad_kernel<(\w+), (\w+), (\w+)(?:, (\d))?', name)
    if m:
        return 'fx_wgrad_kernel<%s, %s, %s, %s>' % (m.group(1), m.group(2), m.group(3), m.group(4) or '0')
    return re.sub(r'<.*', '', name)


def load_stats(d, steps):
    path = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)[0]
    out = collections.OrderedDict()
    for r in csv.DictReader(open(path)):
        k = family(r['Name'])
        calls, ms = out.get(k, (0.0, 0.0))
        out[k] = (calls + int(r['Calls']) / steps, ms + float(r['TotalDurationNs']) / 1e6 / steps)
    return out


def kernels(parent_dir, new_dir, steps):
    p, n = load_stats(parent_dir, steps), load_stats(new_dir, steps)
    print('| kernel family | parent ms / step (calls) | new | new - parent |\n|---|---|---|---|')
    tp, tn = sum(v[1] for v in p.values()), sum(v[1] for v in n.values())
    print('| all kernels | %.3f | %.3f | %+.3f |' % (tp, tn, tn - tp))
    rest = [0.0, 0.0]
    for k in sorted(set(p) | set(n), key=lambda k: -max(p.get(k, (0, 0))[1], n.get(k, (0, 0))[1])):
        a, b = p.get(k, (0, 0)), n.get(k, (0, 0))
        if max(a[1], b[1]) < 0.05:
            rest[0] += a[1]
            rest[1] += b[1]
            continue
        print('| `%s` | %.3f (%.0f) | %.3f (%.0f) | %+.3f |' % (k, a[1], a[0], b[1], b[0], b[1] - a[1]))
    print('| everything below 0.05 ms | %.3f | %.3f | %+.3f |' % (rest[0], rest[1], rest[1] - rest[0]))


def load_bench(path, label):
    out, tag = collections.OrderedDict(), None
    for line in open(path):
        m = re.match(r'(c\d+ h\d+ k\d+ \dx\d s\d d\d x\d+)', line)
        if m:
            tag = m.group(1)
        elif line.startswith('  ' + label):
            v = re.findall(r'[\d.]+', line.split('|', 1)[1])       # fwd ms, TF, dgrad ms, TF, wgrad ms, TF, wgrad(fp32 x) ms, TF, image pass ms, GB/s
            out[tag] = dict(fwd=float(v[0]), dgrad=float(v[2]), wgrad=float(v[4]), img=float(v[9]))
    return out


def shapes(p1, p2, r1, r2):
    P, R = [load_bench(f, 'image-fed') for f in (p1, p2)], [load_bench(f, 'row-fed') for f in (r1, r2)]
    print('| shape (batch 64) | fwd planes r1 r2 | fwd rows r1 r2 | dgrad planes | dgrad rows | wgrad planes | wgrad rows | image pass of dy planes | rows | verdict |')
    print('|---|---|---|---|---|---|---|---|---|---|')
    stage = collections.OrderedDict()
    for tag in P[0]:
        cells, verdict = [], []
        for k in ('fwd', 'dgrad', 'wgrad', 'img'):
            a, b = [p[tag][k] for p in P], [r[tag][k] for r in R]
            cells += ['%.3f %.3f' % tuple(a), '%.3f %.3f' % tuple(b)]
            if max(b) < min(a):
                verdict.append(k + ' faster')
            elif min(b) > max(a):
                verdict.append(k + ' SLOWER')
        print('| %s | %s | %s |' % (tag, ' | '.join(cells), ', '.join(verdict) or 'within rounds'))
        if 'k272' in tag:
            continue                 # the regressor's operands stay on planes in the step
        cnt = int(tag.split('x')[-1])
        g = stage.setdefault(re.search(r' h(\d+) ', tag).group(1), dict(launch=0.0, side=0.0, img=0.0))
        mean = lambda runs, k: sum(x[tag][k] for x in runs) / 2
        g['launch'] += cnt * (mean(R, 'fwd') + mean(R, 'dgrad') - mean(P, 'fwd') - mean(P, 'dgrad'))
        g['side'] += cnt * (mean(R, 'wgrad') - mean(P, 'wgrad'))
        g['img'] += cnt * (mean(R, 'img') - mean(P, 'img'))
    print()
    print('| input map side | forward + data gradient, rows - planes | weight gradient (second stream) | one image pass of dy per layer |\n|---|---|---|---|')
    for h, g in stage.items():
        print('| %s | %+.3f | %+.3f | %+.3f |' % (h, g['launch'], g['side'], g['img']))


if __name__ == '__main__':
    if len(sys.argv) == 5 and sys.argv[1] == 'kernels':
        kernels(sys.argv[2], sys.argv[3], float(sys.argv[4]))
    elif len(sys.argv) == 6 and sys.argv[1] == 'shapes':
        shapes(*sys.argv[2:])
    else:
        sys.exit(__doc__)
