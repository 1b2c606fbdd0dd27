"""The ctypes prototypes are derived from include/mvsdf_hip.h (mvsdf_amd/_lib.py::parse_header): the parser on small headers, the real header, and
calls that only a typed prototype gets right.  No GPU needed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import viewsel_ref as R                                                     # noqa: E402
from mvsdf_amd import _lib                                                  # noqa: E402
from mvsdf_amd._lib import MvsdfError, lib, parse_header                    # noqa: E402

VP = C.c_void_p

SNIPPET = '''
/* a comment with (parentheses); and semicolons; int mvsdf_not_a_function(int); */
#ifndef X_H
#define X_H
#include <stdint.h>
#define MVSDF_MAX 12
#define MVSDF_CALL(a, b) \\
    mvsdf_macro_body(a, b);
#ifdef __cplusplus
extern "C" {
#endif
typedef struct {
    int n;                      /* fields; with (comments) */
    const float* w[MVSDF_MAX];
} MvsdfThing;
enum { MVSDF_A = 0, MVSDF_B = 1 };
int mvsdf_version(void);
void mvsdf_nothing();
const char* mvsdf_name(void);
const float* mvsdf_table(int i);
size_t mvsdf_bytes(int64_t n, const int64_t m);          // const in front
int mvsdf_consts(const float* a, float const* b, const float* const* c, float* const* d, int const e, const double f);
int mvsdf_arrays(const int64_t counts[7], long long out[4], int32_t** handles, void** step);
unsigned long long mvsdf_wide(unsigned long long seed, long long seq, unsigned flags, unsigned int more, uint32_t u, uint64_t key);
int mvsdf_spread(const MvsdfThing* t,   /* the thing; (really) */
                 int a,
                 float
                     b,
                 void* stream);
long long mvsdf_unnamed(int, unsigned long long, const float*, double);
#ifdef __cplusplus
}
#endif
#endif
'''


def test_parser_on_a_small_header():
    p = parse_header(SNIPPET)
    assert list(p) == ['mvsdf_version', 'mvsdf_nothing', 'mvsdf_name', 'mvsdf_table', 'mvsdf_bytes', 'mvsdf_consts', 'mvsdf_arrays', 'mvsdf_wide',
                       'mvsdf_spread', 'mvsdf_unnamed']
    assert p['mvsdf_version'] == (C.c_int, [])
    assert p['mvsdf_nothing'] == (None, [])
    assert p['mvsdf_name'] == (C.c_char_p, [])
    assert p['mvsdf_table'] == (VP, [C.c_int])
    assert p['mvsdf_bytes'] == (C.c_size_t, [C.c_int64, C.c_int64])
    assert p['mvsdf_consts'] == (C.c_int, [VP, VP, VP, VP, C.c_int, C.c_double])
    assert p['mvsdf_arrays'] == (C.c_int, [VP, VP, VP, VP])
    assert p['mvsdf_wide'] == (C.c_ulonglong, [C.c_ulonglong, C.c_longlong, C.c_uint, C.c_uint, C.c_uint32, C.c_uint64])
    assert p['mvsdf_spread'] == (C.c_int, [VP, C.c_int, C.c_float, VP])
    assert p['mvsdf_unnamed'] == (C.c_longlong, [C.c_int, C.c_ulonglong, VP, C.c_double])


@pytest.mark.parametrize('decl,fn,bad', [
    ('int mvsdf_f(int a, half b);', 'mvsdf_f', 'half'),
    ('int mvsdf_g(unsigned short n);', 'mvsdf_g', 'unsigned short'),
    ('int mvsdf_h(long double x);', 'mvsdf_h', 'long double'),
    ('bool mvsdf_r(int a);', 'mvsdf_r', 'bool'),
    ('int mvsdf_s(MvsdfThing by_value);', 'mvsdf_s', 'MvsdfThing'),
])
def test_an_unknown_scalar_spelling_raises_and_names_the_type(decl, fn, bad):
    with pytest.raises(MvsdfError) as e:
        parse_header('int mvsdf_ok(int a);\n' + decl)
    assert fn in str(e.value) and '"%s"' % bad in str(e.value)


def test_a_declaration_the_pattern_cannot_take_raises():
    with pytest.raises(MvsdfError, match='mvsdf_cb'):
        parse_header('int mvsdf_cb(void (*fn)(int), int n);')
    with pytest.raises(MvsdfError, match='mvsdf_twice'):
        parse_header('int mvsdf_twice(int a);\nint mvsdf_twice(float a);')


# the ten entry points that take float / size_t / (unsigned) long long by value and used to rely on a wrapper at every call site: {position: type}
BY_VALUE = {
    'mvsdf_sphere_intersection': {4: C.c_float},
    'mvsdf_trace': {15: C.c_size_t},
    'mvsdf_trace_stage': {16: C.c_size_t},
    'mvsdf_trace_cut_stage': {17: C.c_size_t},
    'mvsdf_tracegen_finish': {12: C.c_size_t},
    'mvsdf_depth_carve': {10: C.c_float, 11: C.c_float, 12: C.c_float, 13: C.c_float, 14: C.c_float},
    'mvsdf_loss_terms': {15: C.c_float, 16: C.c_float, 17: C.c_float, 18: C.c_float, 19: C.c_float, 20: C.c_float},
    'mvsdf_dsurf_select': {8: C.c_float, 9: C.c_float, 10: C.c_ulonglong},
    'mvsdf_dsurf_points': {8: C.c_float, 9: C.c_float, 10: C.c_ulonglong},
    'mvsdf_step_wait_counts_seq': {1: C.c_longlong},
}


def test_the_real_header_types_every_symbol():
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS)) >= 169 and _lib.EXPORTS == list(_lib.PROTOTYPES)
    L = lib()
    for name, (restype, argtypes) in _lib.PROTOTYPES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    for name, where in BY_VALUE.items():
        at = getattr(L, name).argtypes
        for k, a in enumerate(at):
            if k in where:
                assert a is where[k], (name, k, a)
            else:
                assert a in (VP, C.c_int), (name, k, a)          # everything else of these ten is a pointer or an int
    assert L.mvsdf_last_error.restype is C.c_char_p and L.mvsdf_step_destroy.restype is None
    assert L.mvsdf_step_seq.restype is C.c_longlong and L.mvsdf_step_done_seq.restype is C.c_longlong
    assert L.mvsdf_step_counts_offset.restype is C.c_size_t and L.mvsdf_chamfer_key.restype is C.c_uint64


def test_a_plain_int_seed_above_32_bits_reaches_chamfer_key_whole():
    L = lib()
    for seed in (2 ** 32 + 12345, 0x9e3779b97f4a7c15, 2 ** 64 - 1):
        for i in (0, 7, 2 ** 33 + 1):
            assert L.mvsdf_chamfer_key(seed, i) == L.mvsdf_chamfer_key(C.c_uint64(seed), C.c_int64(i))
            assert L.mvsdf_chamfer_key(seed, i) != L.mvsdf_chamfer_key(seed & 0xffffffff, i)
    assert L.mvsdf_chamfer_key(2 ** 32 + 1, 2 ** 33) != L.mvsdf_chamfer_key(2 ** 32 + 1, 0)     # (the low 32 bits of 2^33 are 0)


def test_a_workspace_query_takes_a_count_above_2_to_31_whole():
    """mvsdf_mc_workspace_bytes: 4 bytes per grid point + O(points / 1024), up to 2^60 points.  An extent of 2^32 + 4 must give twice the bytes of half
    that extent (both above 2^31) up to the header and the alignment of the regions, not those of its low 32 bits (an extent of 4)."""
    ws = lib().mvsdf_mc_workspace_bytes
    n = 2 ** 32 + 4
    whole, half, low = ws(n, 2, 2), ws(n // 2, 2, 2), ws(n & 0xffffffff, 2, 2)
    assert whole >= 4 * 4 * n and half >= 4 * 4 * (n // 2)
    assert abs(whole - 2 * half) <= 4096
    assert 0 < low < 4096 and whole != low
    assert ws(n, 2, 2) == ws(C.c_int64(n), C.c_int64(2), C.c_int64(2))


def test_plain_python_floats_reach_the_double_parameters():
    """mvsdf_viewsel_weights_host(.., double theta0, double sigma1, double sigma2, ..) with plain floats and raw addresses, against the numpy restatement
    bit for bit; an int where a double is declared converts too."""
    rng = np.random.RandomState(3)
    a, b = rng.randn(500, 3), rng.randn(500, 3)
    b[:200] = a[:200] + 0.1 * rng.randn(200, 3)
    for theta0, s1, s2 in ((7.5, 1.5, 4.0), (5, 1, 10)):
        th, wq = np.empty(len(a), np.float64), np.empty(len(a), np.int64)
        assert lib().mvsdf_viewsel_weights_host(a.ctypes.data, b.ctypes.data, len(a), theta0, s1, s2, th.ctypes.data, wq.ctypes.data) == 0
        th_r, wq_r = R.theta_wq(a, b, float(theta0), float(s1), float(s2))
        assert np.array_equal(th.view(np.uint64), th_r.view(np.uint64)) and np.array_equal(wq, wq_r)
        assert (wq > 0).sum() > 100


def test_the_stricter_prototypes_reject_what_used_to_pass_silently():
    L = lib()
    with pytest.raises(C.ArgumentError):
        L.mvsdf_packed_floats(258.0, 256)                        # a float for an int
    with pytest.raises(TypeError):
        L.mvsdf_packed_floats(258)                               # too few arguments
    with pytest.raises(C.ArgumentError):
        L.mvsdf_chamfer_key(C.c_int(1), 0)                       # a c_int instance for a uint64_t
