"""The structs of include/mvsdf_hip.h as the Python side reads them (mvsdf_amd/_lib.py::parse_structs, STRUCTS): the parser on small snippets, what it
refuses, and the real header's nine structs against sizeof / offsetof of a host C compiler that reads the same header.  No GPU needed."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from mvsdf_amd import _lib, native_step
from mvsdf_amd._lib import MvsdfError, parse_structs
from mvsdf_amd.datasets import device_batches

NAMES = ['MvsdfNetDesc', 'MvsdfTraceParams', 'MvsdfStepDesc', 'MvsdfStepParams', 'MvsdfStepInputs', 'MvsdfStepLayout', 'MvsdfLossArgs',
         'MvsdfLossLayout', 'MvsdfBatchArgs']


def fields(cls):
    return list(cls._fields_)


def test_parser_on_small_snippets():
    s = parse_structs('''
    #define MVSDF_N 3
    enum { MVSDF_M = 1 << 2 };
    typedef struct {
        int a; unsigned b; unsigned int c; long long d; size_t e; int64_t f;  double g;     /* several declarations on one line */
        const float* p;
        float * const * q;
        const void* r[MVSDF_N];                 /* an array of pointers, sized by a macro */
        float x, y[2], z [ MVSDF_M ];           /* several declarators; a literal and an enumerator as lengths */
    } MvsdfOne;
    int mvsdf_call(const MvsdfOne* one);
    ''')
    assert list(s) == ['MvsdfOne'] and issubclass(s['MvsdfOne'], C.Structure) and s['MvsdfOne'].__name__ == 'MvsdfOne'
    assert fields(s['MvsdfOne']) == [
        ('a', C.c_int), ('b', C.c_uint), ('c', C.c_uint), ('d', C.c_longlong), ('e', C.c_size_t), ('f', C.c_int64), ('g', C.c_double),
        ('p', C.c_void_p), ('q', C.c_void_p), ('r', C.c_void_p * 3), ('x', C.c_float), ('y', C.c_float * 2), ('z', C.c_float * 4)]
    assert parse_structs('typedef struct { int v[MVSDF_N]; } MvsdfA;', {'MVSDF_N': 5})['MvsdfA'].v.size == 20      # the caller's constants
    assert parse_structs('int mvsdf_no_struct(void);\nenum { MVSDF_A = 1 };') == {}


def test_a_struct_declared_earlier_is_taken_by_value():
    s = parse_structs('''
    typedef struct { float r; int n; } MvsdfInner;
    typedef struct { int a; MvsdfInner tp; const MvsdfInner* ptr; MvsdfInner two[2]; long long b; } MvsdfOuter;
    ''')
    assert list(s) == ['MvsdfInner', 'MvsdfOuter']
    assert fields(s['MvsdfOuter']) == [('a', C.c_int), ('tp', s['MvsdfInner']), ('ptr', C.c_void_p), ('two', s['MvsdfInner'] * 2), ('b', C.c_longlong)]
    assert C.sizeof(s['MvsdfOuter']) == 48 and s['MvsdfOuter'].ptr.offset == 16 and s['MvsdfOuter'].b.offset == 40    # 4 + 8, padded to 16; 8; 16; 8
    assert s['MvsdfOuter'](a=1, tp=s['MvsdfInner'](0.5, 7)).tp.n == 7


def test_comments_are_not_read():
    s = parse_structs('''
    /* typedef struct { int ghost; } MvsdfGhost; */
    // typedef struct { int ghost2; } MvsdfGhost2;
    typedef struct {
        int a;      /* a comment with a ; and a { and typedef struct { int x; } MvsdfNot; */
        int b;      // int c; }
        /* int d; */
        float e;    /* a comment over
                     * two lines; with int f; */
    } MvsdfReal;    /* struct union */
    ''')
    assert list(s) == ['MvsdfReal'] and fields(s['MvsdfReal']) == [('a', C.c_int), ('b', C.c_int), ('e', C.c_float)]


@pytest.mark.parametrize('text, struct, member', [
    ('typedef struct { int a; uint8_t flag; } MvsdfA;', 'MvsdfA', 'flag'),                               # a by-value type outside _SCALARS
    ('typedef struct { int a; short s; } MvsdfA;', 'MvsdfA', 's'),
    ('typedef struct { int a; MvsdfB later; } MvsdfA;\ntypedef struct { int x; } MvsdfB;', 'MvsdfA', 'later'),   # a struct used before its declaration
    ('typedef struct { int a; float m[3][4]; } MvsdfA;', 'MvsdfA', 'm'),                                # a two-dimensional array
    ('typedef struct { int a; unsigned bits : 3; } MvsdfA;', 'MvsdfA', 'bits'),                          # a bit-field
    ('typedef struct { int a; union { int i; float f; } u; } MvsdfA;', 'MvsdfA', 'u'),                   # a union
    ('typedef struct { int a; struct { int i; float f; } inner; int b; } MvsdfA;', 'MvsdfA', 'inner'),   # a nested anonymous struct
    ('typedef struct { int a; int (*callback)(int, float); } MvsdfA;', 'MvsdfA', 'callback'),            # a function pointer
    ('typedef struct { int a; float* p, q; } MvsdfA;', 'MvsdfA', 'p'),                                   # a pointer declaration with two declarators
    ('typedef struct { int a; float x, *y; } MvsdfA;', 'MvsdfA', 'y'),
    ('typedef struct { int a; float *p, *q; } MvsdfA;', 'MvsdfA', 'p'),
    ('typedef struct { int a; float v[MVSDF_UNKNOWN]; } MvsdfA;', 'MvsdfA', 'v'),                        # a length that is no literal and no constant
    ('typedef struct { int a; float v[2 * 3]; } MvsdfA;', 'MvsdfA', 'v'),
    ('typedef struct { int a; float v[]; } MvsdfA;', 'MvsdfA', 'v'),
    ('typedef struct { int a; float v[0]; } MvsdfA;', 'MvsdfA', 'v'),
])
def test_parser_refuses_what_it_does_not_understand(text, struct, member):
    with pytest.raises(MvsdfError, match=r'^%s, member "[^"]*\b%s\b[^"]*": ' % (struct, member)):
        parse_structs(text)


@pytest.mark.parametrize('text, name', [
    ('typedef struct { int a; } MvsdfA;\ntypedef union { int i; float f; } MvsdfU;', 'MvsdfU'),          # a union of its own
    ('typedef struct MvsdfTag { int a; } MvsdfA;', 'MvsdfTag'),                                          # a struct with a tag
    ('struct MvsdfPlain { int a; };', 'MvsdfPlain'),
    ('typedef struct {\n#ifdef MVSDF_WIDE\n    int wide;\n#endif\n    int a; } MvsdfA;', 'MvsdfA'),      # members under a condition
])
def test_parser_refuses_other_struct_forms(text, name):
    with pytest.raises(MvsdfError, match=r'\b%s\b' % name):
        parse_structs(text)


def test_the_table_is_the_real_header():
    with open(_lib.HEADER_PATH) as f:
        parsed = parse_structs(f.read())
    assert list(parsed) == NAMES and list(_lib.STRUCTS) == NAMES
    for name in NAMES:                                  # (two parses make two sets of classes: compared by field and type name)
        assert [(f, t.__name__) for f, t in fields(parsed[name])] == [(f, t.__name__) for f, t in fields(_lib.STRUCTS[name])], name
    assert (_lib.NetDesc, _lib.TraceParams) == tuple(_lib.STRUCTS[n] for n in NAMES[:2])
    assert (native_step.StepDesc, native_step.StepParams, native_step.StepInputs, native_step.StepLayout, native_step.LossArgs,
            native_step.LossLayout) == tuple(_lib.STRUCTS[n] for n in NAMES[2:8])
    assert device_batches.BatchArgs is _lib.STRUCTS[NAMES[8]] and native_step.TraceParams is _lib.TraceParams
    assert _lib.MAX_LAYERS == 12 and native_step.STEP_MAX_LAYERS == 24
    assert [len(fields(_lib.STRUCTS[n])) for n in NAMES] == [12, 8, 16, 3, 12, 19, 53, 18, 36]
    assert dict(fields(native_step.StepDesc))['tp'] is _lib.TraceParams


def _host_compiler():
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    beside = [os.path.join(os.path.dirname(hipcc), *p) for p in (('amdclang',), ('clang',), ('..', 'llvm', 'bin', 'clang'))]
    found = shutil.which('cc') or next((p for p in beside if os.access(p, os.X_OK)), None)
    assert found, 'no host C compiler: neither `cc` on the PATH nor ROCm\'s clang beside %s; the layout of the structs cannot be checked without one' % hipcc
    return found


def test_the_layout_is_the_host_compilers(tmp_path):
    """Every struct and every field the parser read, against sizeof / offsetof of a C compiler that reads the header itself: a field the parser
    dropped, reordered, mistyped or sized wrongly is a differing line."""
    lines, want = [], []
    for name, cls in _lib.STRUCTS.items():
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        want.append('%s %d' % (name, C.sizeof(cls)))
        for field, _ in fields(cls):
            lines.append('    printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (name, field, name, field, name, field))
            want.append('%s.%s %d %d' % (name, field, getattr(cls, field).offset, getattr(cls, field).size))
    src = tmp_path / 'layout.c'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mvsdf_hip.h"\nint main(void) {\n%s\n    return 0;\n}\n' % '\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run([_host_compiler(), '-I', os.path.dirname(_lib.HEADER_PATH), '-o', str(exe), str(src)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    n_fields = sum(len(fields(cls)) for cls in _lib.STRUCTS.values())
    assert n_fields == 177 and len(got) == n_fields + len(_lib.STRUCTS) == len(want)
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w]
