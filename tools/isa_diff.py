"""Compare the kernels of two device assembly files (hipcc --cuda-device-only -S of the same source in two trees).

    python tools/isa_diff.py parent.s new.s [--map OLD=NEW ...]

Kernels are matched by mangled name; --map renames a parent symbol first (an instance whose template list grew a defaulted parameter).  A body is the text
between the kernel's label and its .Lfunc_end, comments and section directives stripped, the kernel's own symbol replaced and local label numbers dropped; the .amdhsa_ descriptor block
is compared too.  Prints the counts, every kernel that differs or exists in one file only, and the resource lines of the new-only kernels."""
import re
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r'^(_Z\w+):[ \t]*(?:;[^\n]*)?\n(.*?)^\.Lfunc_end\d+:', text, re.S | re.M):
        name, body = m.group(1), m.group(2)
        desc = re.search(r'\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel' % re.escape(name), text, re.S)
        if not desc:
            continue                                    # a device function, not a kernel
        body = body + desc.group(1)
        body = re.sub(r';.*', '', body)
        body = body.replace(name, 'KERNEL')
        body = re.sub(r'\.L[A-Za-z_]*\d+(_\d+)?', '.L', body)
        # (a kernel that became a template instance moves from .text to a comdat section of its own: where the code is placed, not what it is)
        body = '\n'.join(l.strip() for l in body.splitlines() if l.strip() and not re.match(r'\s*\.(text|section)\b', l))
        out[name] = (body, desc.group(1))
    return out


def resources(desc):
    get = lambda k: (re.search(r'\.amdhsa_%s (\S+)' % k, desc) or [None, '?'])[1]
    return 'next_free_vgpr %s  scratch %s B  lds %s B' % (get('next_free_vgpr'), get('private_segment_fixed_size'), get('group_segment_fixed_size'))


def main(argv):
    renames = dict(a.split('=') for a in argv[3:] if a != '--map')
    old = {renames.get(k, k): v for k, v in kernels(argv[1]).items()}
    new = kernels(argv[2])
    same = [k for k in old if k in new and old[k][0] == new[k][0]]
    differ = [k for k in old if k in new and old[k][0] != new[k][0]]
    print('kernels: parent %d, new %d; identical %d, differ %d, parent only %d, new only %d'
          % (len(old), len(new), len(same), len(differ), len(set(old) - set(new)), len(set(new) - set(old))))
    for k in differ:
        print('DIFFERS   ', k)
    for k in sorted(set(old) - set(new)):
        print('PARENT ONLY', k)
    for k in sorted(set(new) - set(old)):
        print('NEW ONLY   ', k, '|', resources(new[k][1]))
    return 1 if differ or set(old) - set(new) else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
