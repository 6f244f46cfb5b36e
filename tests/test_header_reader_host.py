"""include/p3d_hip.h is the only statement of the C ABI; _lib reads it (parse_header).  The reader on short header texts, the whole header against
tests/test_abi.py's count, and the generated structs' layout against what a C compiler makes of the same header."""
import ctypes
import os
import subprocess

import pytest

import test_abi

I32, I64, SZ, F32, F64, VP = ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float, ctypes.c_double, ctypes.c_void_p
STRUCTS = ('p3d_conv_desc', 'p3d_fold_job', 'p3d_fx_fuse', 'p3d_block_desc', 'p3d_block_io', 'p3d_hblock_io', 'p3d_fx_wgrad_fuse')


def fields(cls):
    return [(n, t) for n, t in cls._fields_]


def test_struct_members(pkg):
    consts, structs, sigs = pkg._lib.parse_header('''
        typedef struct inner {
            int32_t N, C, H, W;     /* several declarators */
            float eps[4];
        } inner;
        typedef struct outer {
            const float* w[4];      /* an array of pointers; a comment with (parentheses); and a semicolon
                                       that goes on over a line */
            /* a comment between members */
            unsigned char* mask;
            inner conv[4];
            int32_t reserved[2];
            int64_t n; size_t bytes; double sum;
            const inner* ref;
        } outer;
    ''')
    assert consts == {} and sigs == {} and list(structs) == ['inner', 'outer']
    inner, outer = structs['inner'], structs['outer']
    assert fields(inner) == [('N', I32), ('C', I32), ('H', I32), ('W', I32), ('eps', F32 * 4)]
    assert fields(outer) == [('w', VP * 4), ('mask', VP), ('conv', inner * 4), ('reserved', I32 * 2), ('n', I64), ('bytes', SZ), ('sum', F64), ('ref', VP)]
    assert issubclass(outer, ctypes.Structure) and ctypes.sizeof(outer) == 32 + 8 + 4 * 32 + 8 + 24 + 8


def test_prototypes(pkg):
    consts, structs, sigs = pkg._lib.parse_header('''
        #ifndef GUARD_H
        #define GUARD_H
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define ANSWER 42
        #define EBAD (-3)      /* a negative code */
        #define ELSE -4
        typedef struct desc { int32_t n; } desc;
        const char* last_error(void);
        /* a block comment with a call f(x); in it,
           over two lines */
        void tune(int32_t what, int32_t value);
        int32_t run(const desc* d, const float* x, float* y, void* ws, size_t ws_bytes, int64_t n, float eps, double count,
                    const unsigned char* mask, const uint8_t* idx /* may be NULL */, void** stream, size_t* bytes, const uint32_t* words);
        size_t bytes_of(const desc* d);      /* a comment behind the prototype */
        #ifdef __cplusplus
        }
        #endif
        #endif
    ''')
    assert consts == {'ANSWER': 42, 'EBAD': -3, 'ELSE': -4}
    d = ctypes.POINTER(structs['desc'])
    assert sigs == {'last_error': (ctypes.c_char_p, []), 'tune': (None, [I32, I32]),
                    'run': (I32, [d, VP, VP, VP, SZ, I64, F32, F64, VP, VP, VP, VP, VP]), 'bytes_of': (SZ, [d])}


@pytest.mark.parametrize('text, quoted', [
    ('int32_t f(unsigned x);', 'int32_t f(unsigned x)'),                       # a type outside the rule
    ('int f(void);', 'int f(void)'),
    ('int32_t f(uint8_t flag);', 'int32_t f(uint8_t flag)'),
    ('int32_t f(widget_t* w);', 'int32_t f(widget_t* w)'),                     # a pointer to a type the header never defined
    ('int32_t f(void x);', 'int32_t f(void x)'),
    ('int32_t f(int32_t);', 'int32_t f(int32_t)'),                             # an unnamed parameter
    ('int32_t f(int32_t a, void (*cb)(int32_t));', 'void (*cb)(int32_t)'),     # malformed for this reader: a function pointer
    ('int32_t f(int32_t a', 'int32_t f(int32_t a'),
    ('int32_t g;', 'int32_t g'),
    ('typedef struct s { short a; } s;', 'short a'),
    ('typedef struct s { int32_t a:3; } s;', 'int32_t a:3'),
    ('typedef struct s { int32_t a, (*b); } s;', 'int32_t a, (*b)'),
    ('typedef struct s { struct { int32_t a; } in; } s;', 'struct s'),         # a nested body
])
def test_what_it_does_not_know_raises_with_the_text(pkg, text, quoted):
    with pytest.raises(pkg._lib.P3DError) as e:
        pkg._lib.parse_header(text)
    assert quoted in str(e.value)


def test_a_missing_header_raises_with_its_path(pkg, tmp_path):
    path = str(tmp_path / 'no_such.h')
    with pytest.raises(pkg._lib.P3DError) as e:
        pkg._lib.read_header(path)
    assert path in str(e.value)


def test_every_prototype_of_the_header_is_bound(pkg):
    L = pkg._lib
    declared = test_abi.declared_functions(L.HEADER_PATH)
    assert len(L.SIGNATURES) == len(declared) and sorted(L.SIGNATURES) == declared
    scalars = (I32, I64, SZ, F32, F64, VP, ctypes.c_char_p)
    for name, (res, args) in L.SIGNATURES.items():
        assert res is None or res in (I32, SZ, ctypes.c_char_p), name
        for a in args:
            assert isinstance(a, type) and (a in scalars or issubclass(a, ctypes._Pointer) and a._type_ in L.STRUCTS.values()), (name, a)
    handle = L.lib()
    for name, (res, args) in L.SIGNATURES.items():
        fn = getattr(handle, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert L.SIGNATURES['p3d_block_bwd'] == (I32, [ctypes.POINTER(L.STRUCTS['p3d_block_desc']), ctypes.POINTER(L.STRUCTS['p3d_block_io']), VP, SZ, VP, SZ, VP, VP])
    assert L.SIGNATURES['p3d_f8act_bytes'] == (SZ, [I64, I32]) and L.SIGNATURES['p3d_fx_tune'] == (None, [I32, I32])
    assert L.SIGNATURES['p3d_fx_open_images'][1][5] is F64


def test_the_constants_and_the_class_names(pkg):
    L, ops = pkg._lib, pkg.ops
    c = L.CONSTANTS
    assert (c['P3D_OK'], c['P3D_EINVAL'], c['P3D_EWORKSPACE'], c['P3D_ELAUNCH'], c['P3D_VERSION']) == (0, -1, -2, -3, 100)
    assert (ops.LAST_FP32_LEN, ops.FX_LAUNCH_LEN, ops.FX_INSTANCE_LEN) == (c['P3D_FP32_LAUNCH_FIELDS'], c['P3D_FX_LAUNCH_FIELDS'], c['P3D_FX_INSTANCE_FIELDS']) == (16, 16, 7)
    assert c['P3D_FX_WGRAD_PLAN_FIELDS'] == 16
    assert (ops.EVAL_VALID, ops.EVAL_SUM_DIST, ops.EVAL_PCK, ops.EVAL_SUM_AUC, ops.EVAL_SOLID, ops.EVAL_LOSS, ops.EVAL_BATCH, ops.EVAL_PRESENT, ops.EVAL_ROW) == \
        (0, 1, 2, 3, 4, 10, 11, 12, 13)
    assert 'P3D_HIP_H' not in c
    assert set(L.STRUCTS) == set(STRUCTS)
    assert (L.ConvDesc, L.FoldJob, L.FxFuse, pkg.ops_block.BlockDesc, pkg.ops_block.BlockIO, pkg.ops_half.HBlockIO, L.FxWgradFuse) == tuple(L.STRUCTS[n] for n in STRUCTS)


def test_struct_layouts_are_the_c_compilers(pkg, tmp_path):
    """A program written from the parsed member lists, with no project header but p3d_hip.h, prints sizeof and every offsetof as the compiler of build() lays
    the structs out for the host; the generated ctypes classes must say the same."""
    L = pkg._lib
    lines, want = [], []
    for name in STRUCTS:
        cls = L.STRUCTS[name]
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        want.append('%s %d' % (name, ctypes.sizeof(cls)))
        for field, _ in cls._fields_:
            lines.append('    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, field, name, field))
            want.append('%s.%s %d' % (name, field, getattr(cls, field).offset))
    src = tmp_path / 'layout.cpp'
    src.write_text('#include <stdio.h>\n#include "p3d_hip.h"\nint main() {\n%s\n    return 0;\n}\n' % '\n'.join(lines))
    exe = str(tmp_path / 'layout')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')                     # csrc/Makefile's compiler; no offload arch: host code only
    subprocess.run([hipcc, '-I', os.path.dirname(L.HEADER_PATH), str(src), '-o', exe], check=True, timeout=300)
    got = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split('\n')
    assert [g for g in got if g] == want
