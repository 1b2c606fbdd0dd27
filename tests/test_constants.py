"""The result words, error bits and limits of include/mvsdf_hip.h as the Python side reads them (mvsdf_amd/_lib.py::parse_constants, K, raise_for_bits):
the parser on small snippets (enumerators and object-like macros), the real header's blocks, and every module's error table.  No GPU needed."""
import collections
import importlib
import re

import pytest

from mvsdf_amd import _lib
from mvsdf_amd._lib import K, MvsdfError, parse_constants, raise_for_bits

with open(_lib.HEADER_PATH) as _f:
    CONSTS = parse_constants(_f.read())


def test_parser_on_small_snippets():
    assert parse_constants('enum { MVSDF_A = 0, MVSDF_B = 1 };') == {'MVSDF_A': 0, 'MVSDF_B': 1}
    assert parse_constants('enum { MVSDF_HEX = 0x1F, MVSDF_SHIFT = 1 << 22, MVSDF_HEXSHIFT = 0x3 << 0x4 };') == {
        'MVSDF_HEX': 31, 'MVSDF_SHIFT': 1 << 22, 'MVSDF_HEXSHIFT': 48}
    text = '''
    typedef struct { int n; } MvsdfThing;      /* not an enum; enum { MVSDF_IN_A_COMMENT = 1 }; */
    enum {
        MVSDF_X_H_FIRST = 0,    /* a trailing comment, with = 7 and a comma */
        MVSDF_X_H_RUN = 1,      // twelve words; and a semicolon
        MVSDF_X_H_WORDS = 13
    };
    int mvsdf_call(int a);
    enum { MVSDF_X_ERR_ONE = 1, MVSDF_X_ERR_TWO = 2, };
    '''
    assert parse_constants(text) == {'MVSDF_X_H_FIRST': 0, 'MVSDF_X_H_RUN': 1, 'MVSDF_X_H_WORDS': 13, 'MVSDF_X_ERR_ONE': 1, 'MVSDF_X_ERR_TWO': 2}
    assert parse_constants('int mvsdf_no_enum(void);') == {}


def test_object_like_macros_are_constants_too():
    text = '''
    #ifndef MVSDF_GUARD_H
    #define MVSDF_GUARD_H                  /* no value: left alone */
    #define MVSDF_DEC 12
      #  define MVSDF_HEX 0x1F             /* a comment behind the value; #define MVSDF_IN_A_COMMENT 3 */
    #define MVSDF_SHIFT 1 << 4             // #define MVSDF_IN_A_LINE_COMMENT 4
    enum { MVSDF_ENUM = 7 };
    #define MVSDF_FUNCTION_LIKE(x) 3
    #define MVSDF_PAREN (3)
    #define MVSDF_SUM 1 + 2
    #define MVSDF_NAMED MVSDF_DEC
    #define MVSDF_FLOAT 1.5
    #define MVSDF_STRING "12"
    #define OTHER_PREFIX 5
    #define MVSDF_CONTINUED 1 \\
                            << 2
    #endif
    '''
    assert parse_constants(text) == {'MVSDF_ENUM': 7, 'MVSDF_DEC': 12, 'MVSDF_HEX': 31, 'MVSDF_SHIFT': 16}


@pytest.mark.parametrize('text, name', [
    ('enum { MVSDF_A = 0, MVSDF_NO_VALUE, MVSDF_C = 2 };', 'MVSDF_NO_VALUE'),
    ('enum { MVSDF_A = 0 };\nenum { MVSDF_B = 1, MVSDF_A = 2 };', 'MVSDF_A'),
    ('enum { MVSDF_A = 0, MVSDF_SUM = 1 + 2 };', 'MVSDF_SUM'),
    ('enum { MVSDF_A = 1, MVSDF_REF = MVSDF_A };', 'MVSDF_REF'),
    ('enum { MVSDF_WIDE = 1ll << 40 };', 'MVSDF_WIDE'),
    ('#define MVSDF_A 1\n#define MVSDF_A 2\n', 'MVSDF_A'),
    ('#define MVSDF_A 1\n#define MVSDF_A 1\n', 'MVSDF_A'),
    ('#define MVSDF_A 1\nenum { MVSDF_B = 0, MVSDF_A = 1 };\n', 'MVSDF_A'),
    ('enum { MVSDF_B = 0, MVSDF_A = 1 };\n#define MVSDF_A 1\n', 'MVSDF_A'),
])
def test_parser_refuses_what_it_cannot_evaluate(text, name):
    with pytest.raises(MvsdfError, match=r'\b%s\b' % name):
        parse_constants(text)


def test_the_namespace_is_the_real_header():
    assert CONSTS and vars(K) == CONSTS
    assert K.MVSDF_CNT_ROWS_SPHERE == 0 and K.MVSDF_CNT_LATE_ROUNDS == 15          # the block that was there before
    assert K.MVSDF_GREG_MAX_HYPOTHESES == 1 << 22 and K.MVSDF_PC_MAX_K == 32
    assert K.MVSDF_MAX_LAYERS == 12 and K.MVSDF_STEP_MAX_LAYERS == 24 and K.MVSDF_STEP_COUNT_RING == 64          # the object-like macros
    assert K.MVSDF_STEP_UNHIT_DEFER == 0 and K.MVSDF_STEP_UNHIT_EAGER == 1 and not hasattr(K, 'MVSDF_HIP_H')


def _blocks(kind):
    """{prefix: {name: value}} of the enumerators MVSDF_<prefix>_<kind>_<what>"""
    out = collections.defaultdict(dict)
    for name, value in CONSTS.items():
        m = re.fullmatch(r'(MVSDF_\w+?_%s_)\w+' % kind, name)
        if m:
            out[m.group(1)][name] = value
    return out


def test_error_blocks_hold_distinct_single_bits():
    blocks = _blocks('ERR')
    assert len(blocks) == 11, sorted(blocks)
    for prefix, block in blocks.items():
        values = list(block.values())
        assert all(v > 0 and v & (v - 1) == 0 for v in values), prefix
        assert len(set(values)) == len(values), prefix


def test_header_blocks_index_distinct_words_inside_the_header():
    blocks = _blocks('H')
    assert len(blocks) >= 20, sorted(blocks)
    for prefix, block in blocks.items():
        words = block.pop(prefix + 'WORDS')
        values = list(block.values())
        assert min(values) == 0 and len(set(values)) == len(values) and max(values) < words and words * 8 <= 256, prefix


# (module, the table's name, the block its bits come from, the order in which the bits are looked at: that of the `if`s the tables replaced)
TABLES = [
    ('chamfer', 'ERRORS', 'MVSDF_PC_ERR_', [4, 2, 8]),
    ('cloud', 'ERRORS', 'MVSDF_PC_ERR_', [4, 32]),
    ('registration', 'ERRORS', 'MVSDF_PC_ERR_', [4, 8]),
    ('normals', 'ERRORS', 'MVSDF_PC_ERR_', [4, 128, 256, 32]),
    ('global_reg', 'ERRORS', 'MVSDF_PC_ERR_', [4, 128, 256, 512]),
    ('fusion', 'ERRORS', 'MVSDF_FU_ERR_', [1, 2, 4, 8, 16]),
    ('tsdf', 'ERRORS', 'MVSDF_TS_ERR_', [1, 2, 4, 8]),
    ('poisson', 'ERRORS', 'MVSDF_PO_ERR_', [1, 2, 4]),
    ('stereo', 'ERRORS', 'MVSDF_PS_ERR_', [1, 2, 4, 8, 16, 32, 64]),
    ('raster', 'ERRORS', 'MVSDF_RA_ERR_', [1, 2]),
    ('viewsel', 'ERRORS', 'MVSDF_VS_ERR_', [1, 2, 4]),
    ('undistort', 'ERRORS', 'MVSDF_UD_ERR_', [1, 2]),
    ('mesh', 'CUT_ERRORS', 'MVSDF_CUT_ERR_', [1, 2, 4]),
    ('mesh', 'SIMPLIFY_ERRORS', 'MVSDF_SP_ERR_', [1, 2, 4]),
]


@pytest.mark.parametrize('module, name, prefix, order', TABLES, ids=['%s.%s' % t[:2] for t in TABLES])
def test_error_tables_keep_their_block_and_their_order(module, name, prefix, order):
    table = getattr(importlib.import_module('mvsdf_amd.' + module), name)
    bits = [row[0] for row in table]
    assert bits == order and len(set(bits)) == len(bits)
    block = {v for k, v in CONSTS.items() if k.startswith(prefix)}
    assert set(bits) <= block
    for row in table:
        assert isinstance(row[-1], str) and row[-1] and (len(row) == 2 or issubclass(row[1], Exception))


def test_borrowed_tables_are_the_lenders():
    from mvsdf_amd import raster, viewsel
    assert K.MVSDF_TX_ERR_FINITE == K.MVSDF_RA_ERR_FINITE and K.MVSDF_TX_ERR_INDEX == K.MVSDF_RA_ERR_INDEX     # texture.py reads its bits with raster's table
    assert raster.MAX_VIEWS == K.MVSDF_RA_MAX_VIEWS and viewsel.MAX_VIEWS == K.MVSDF_VS_MAX_VIEWS


def test_raise_for_bits():
    table = [(4, ValueError, 'four'), (1, KeyError, 'one'), (2, MvsdfError, 'two %d')]
    raise_for_bits(0, 'call', table)
    with pytest.raises(ValueError, match=r'^call: four$'):
        raise_for_bits(4 | 1, 'call', table)                      # the first row wins, not the lowest bit
    with pytest.raises(KeyError, match=r'call: one'):
        raise_for_bits(1 | 2 | 64, 'call', table)
    with pytest.raises(MvsdfError, match=r'^call: two %d$'):
        raise_for_bits(2, 'call', table)                          # the message is not formatted again
    with pytest.raises(MvsdfError, match=r'^call failed \(error bits 64\)$'):
        raise_for_bits(64, 'call', table)
    with pytest.raises(MvsdfError, match=r'^call failed \(error bits 8\)$'):
        raise_for_bits(8, 'call', [])
