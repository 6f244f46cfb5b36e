"""ctypes binding of libp3d_hip.so.  include/p3d_hip.h is the only statement of the C ABI: its prototypes, structs and integer
#defines are read from it here, once, at import.

There is deliberately NO fallback: if the shared library is missing or a call fails, the
caller gets a P3DError.  PyTorch is used only to own device memory and streams.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('P3D_LIB') or os.path.join(_HERE, 'csrc', 'libp3d_hip.so')   # P3D_LIB: A/B a tuning build
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'p3d_hip.h')


class P3DError(RuntimeError):
    pass


# ---- the header reader ---------------------------------------------------------------------------------------------------------------------------------------------
# The header is plain C of a regular shape: integer #defines, `typedef struct tag { members } name;` without nesting, and prototypes `ret name(args);` whose
# parameters are all named.  Anything outside that shape raises P3DError with the declaration's text; no type ever defaults to int.
_SCALARS = {'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'size_t': ctypes.c_size_t, 'float': ctypes.c_float, 'double': ctypes.c_double}
_POINTEES = set(_SCALARS) | {'void', 'char', 'unsigned char', 'uint8_t', 'uint32_t', 'uint64_t'}          # what a c_void_p may stand for
_DECLARATOR = re.compile(r'(?P<base>\w[\w\s]*?)(?P<stars>[\s*]+)(?P<name>\w+)\s*(?:\[\s*(?P<count>\d+)\s*\])?')
_STRUCT = re.compile(r'\btypedef\s+struct\s+\w*\s*\{([^{}]*)\}\s*(\w+)\s*;')


def _declarator(text, what):
    """'const float* w[4]' -> ('float', True, 1, 'w', 4): base type without qualifiers, whether it was const, pointer depth, name, array length or None."""
    m = _DECLARATOR.fullmatch(text.strip())
    if not m:
        raise P3DError('p3d_hip.h: cannot split %s' % what)
    words = m.group('base').split()
    base = ' '.join(w for w in words if w not in ('const', 'struct'))
    return base, 'const' in words, m.group('stars').count('*'), m.group('name'), m.group('count') and int(m.group('count'))


def _ctype(base, const, stars, structs, what, member=False):
    if not stars:
        if base in _SCALARS:
            return _SCALARS[base]
        if base in structs and member:
            return structs[base]
    elif base == 'char' and const and stars == 1 and not member:
        return ctypes.c_char_p
    elif base in structs and stars == 1 and not member:
        return ctypes.POINTER(structs[base])
    elif base in _POINTEES or base in structs:
        return ctypes.c_void_p
    raise P3DError('p3d_hip.h: unknown type `%s%s` in %s' % (base, '*' * stars, what))


def _struct(name, body, structs):
    fields = []
    for decl in body.split(';'):
        if not decl.strip():
            continue
        what = 'member `%s` of struct %s' % (' '.join(decl.split()), name)
        first, *more = decl.split(',')
        base, const, stars, field, count = _declarator(first, what)
        declared = [(stars, field, count)]
        for extra in more:                                                                 # `int32_t N, C, H, W;`: the later declarators carry their own stars
            m = re.fullmatch(r'\s*(\**)\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*', extra)
            if not m:
                raise P3DError('p3d_hip.h: cannot place %s' % what)
            declared.append((len(m.group(1)), m.group(2), m.group(3) and int(m.group(3))))
        for stars, field, count in declared:
            t = _ctype(base, const, stars, structs, what, member=True)
            fields.append((field, t if count is None else t * count))
    return type(name, (ctypes.Structure,), {'_fields_': fields, '__doc__': 'struct %s of include/p3d_hip.h' % name})


def _prototype(text, structs):
    what = 'prototype `%s`' % text
    m = re.fullmatch(r'([^()]+)\(([^()]*)\)', text)
    if not m:
        raise P3DError('p3d_hip.h: cannot split %s' % what)
    base, const, stars, name, count = _declarator(m.group(1), what)
    if count is not None:
        raise P3DError('p3d_hip.h: cannot split %s' % what)
    res = None if (base, stars) == ('void', 0) else _ctype(base, const, stars, structs, what)
    args = []
    if m.group(2).strip() not in ('', 'void'):
        for arg in m.group(2).split(','):
            a_base, a_const, a_stars, _, a_count = _declarator(arg, what)
            args.append(_ctype(a_base, a_const, a_stars + (a_count is not None), structs, what))      # an array parameter is a pointer
    return name, (res, args)


def parse_header(text):
    """The ABI a header text declares: (constants, structs, signatures) = {macro: int}, {typedef name: ctypes.Structure subclass},
    {function: (restype, argtypes)}."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    constants = {m.group(1): int(m.group(2) or m.group(3))
                 for m in re.finditer(r'^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(?:(-?\d+)|\([ \t]*(-?\d+)[ \t]*\))[ \t]*$', text, re.M)}
    text = re.sub(r'^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus\b.*?^[ \t]*#[ \t]*endif[^\n]*$', ' ', text, flags=re.S | re.M)         # extern "C" { ... }
    text = re.sub(r'^[ \t]*#[^\n]*$', ' ', text, flags=re.M)
    structs = {}
    for m in _STRUCT.finditer(text):                                                       # in the header's order: a later struct may hold an earlier one
        structs[m.group(2)] = _struct(m.group(2), m.group(1), structs)
    text = _STRUCT.sub(' ', text)
    signatures = dict(_prototype(' '.join(decl.split()), structs) for decl in text.split(';') if decl.strip())
    return constants, structs, signatures


def read_header(path):
    try:
        with open(path) as f:
            text = f.read()
    except OSError as e:
        raise P3DError('the C ABI header %s cannot be read (%s)' % (path, e))
    return parse_header(text)


# CONSTANTS: the header's integer #defines (P3D_OK, P3D_EINVAL, P3D_FX_LAUNCH_FIELDS, P3D_EVAL_ROW, ...); SIGNATURES: name -> (restype, argtypes) of every function
CONSTANTS, STRUCTS, SIGNATURES = read_header(HEADER_PATH)
ConvDesc, FoldJob, FxFuse, FxWgradFuse = STRUCTS['p3d_conv_desc'], STRUCTS['p3d_fold_job'], STRUCTS['p3d_fx_fuse'], STRUCTS['p3d_fx_wgrad_fuse']

_lib = None


def lib():
    """Load (once) and return the ctypes handle.  Raises P3DError if the library is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise P3DError('libp3d_hip.so is not built (%s missing): run __graft_entry__.build() or `make -C %s`'
                           % (LIB_PATH, os.path.dirname(LIB_PATH)))
        # PyTorch-ROCm ships its own libamdhip64; it must be the HIP runtime in the process BEFORE this library is mapped, or
        # the kernels would be launched through a second runtime instance that owns no device ("no ROCm-capable device").
        import torch  # noqa: F401
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(code, what):
    if code != 0:
        msg = lib().p3d_last_error()
        raise P3DError('%s failed (%d): %s' % (what, code, msg.decode() if msg else ''))
