"""sha256 of the gfx950 code object inside each object file of a csrc directory (default: the package's), one `name hash functions` line each: two builds whose
lines agree run the same device code, whatever their host code does.  A host-only refactor is checked by running this on a build of the parent commit and on a
build of the branch and comparing the output (profiles/conv_route_refactor.md)."""
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, '3d-pose-estimation-with-previleged-information_amd', 'csrc')
OBJDUMP = '/opt/rocm/lib/llvm/bin/llvm-objdump'


def code_objects(obj):
    """the ELF64 images embedded in the object's fat binary (as tools/scan_packed.py finds them in the library)"""
    data = open(obj, 'rb').read()
    for m in re.finditer(b'\x7fELF', data):
        i = m.start()
        if i == 0 or data[i + 4] != 2:
            continue
        e_shoff = struct.unpack_from('<Q', data, i + 0x28)[0]
        e_shentsize, e_shnum = struct.unpack_from('<HH', data, i + 0x3A)
        yield data[i:i + e_shoff + e_shentsize * e_shnum]


def main(csrc=CSRC):
    with tempfile.TemporaryDirectory() as tmp:
        for name in sorted(f for f in os.listdir(csrc) if f.endswith('.o')):
            for co in code_objects(os.path.join(csrc, name)):
                out = os.path.join(tmp, name[:-2] + '.co')
                with open(out, 'wb') as f:
                    f.write(co)
                dis = subprocess.run([OBJDUMP, '-d', out], capture_output=True, text=True).stdout
                print('%-16s %s %d' % (name, hashlib.sha256(co).hexdigest(), len(re.findall(r'^[0-9a-f]+ <.*>:$', dis, re.M))))


if __name__ == '__main__':
    main(*sys.argv[1:2])
