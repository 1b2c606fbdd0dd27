"""The operand layout of the matrix-core kernels (mvsdf_amd/csrc/pack_layout.h: pack sizes, fragment maps, block order, bf16 rounding, three-term split) on the
CPU.  The header has no HIP in it: tests/native/pack_layout_table.cpp includes it alone, is compiled with the host C++ compiler and packs, for every shape of
pack_ref.SHAPES and its transpose, a matrix of recognisable bit patterns through the header's maps -- the fp32 pack, the rounded fp32 pack, the one-term bf16
pack, the three-term pack and the three-term pack of the transpose.  Each is compared byte for byte with the scattering packers of test_pack_ref_host.py
(numpy, written from the layout comments, and themselves held to pack_ref's gathering unpackers there).  basic.hip's pack kernels and the pack loops of
k_step_prologue take their (row, k) and their values from the same header; tests/test_gpu_weight_packs.py holds what they write on the device."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pack_ref as PR
from conftest import ROOT
from test_pack_ref_host import pack_bf16, pack_f32

CSRC = os.path.join(ROOT, 'mvsdf_amd', 'csrc')
SHAPES = list(PR.SHAPES) + [(k, n) for n, k in PR.SHAPES]


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    cxx = os.environ.get('CXX') or next((c for c in ('c++', 'g++', 'clang++') if shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    out = str(tmp_path_factory.mktemp('pack_layout') / 'pack_layout_table')
    subprocess.check_call([cxx, '-std=c++17', '-O0', '-Wall', '-Werror', '-I', CSRC, os.path.join(ROOT, 'tests', 'native', 'pack_layout_table.cpp'), '-o', out])
    return out


def _run(exe, mode, args):
    return subprocess.run([exe, mode] + [str(a) for a in args], check=True, stdout=subprocess.PIPE).stdout


def _matrix(N, K):
    """the program's W: element (o, k) has the bit pattern 0x3f800005 + 8 (1024 o + k) -- distinct values in [1, 2) with mantissa bits in all three bf16 terms"""
    o, k = np.meshgrid(np.arange(N, dtype=np.uint32), np.arange(K, dtype=np.uint32), indexing='ij')
    return (np.uint32(0x3f800005) + np.uint32(8) * (np.uint32(1024) * o + k)).view(np.float32)


def test_size_functions(exe):
    lines = _run(exe, 'sizes', [v for s in SHAPES for v in s]).decode().splitlines()
    assert len(lines) == len(SHAPES)
    for (N, K), line in zip(SHAPES, lines):
        assert [int(v) for v in line.split()] == [N, K, PR.packed_floats(N, K), PR.packed_bf16_elems(N, K)]


def test_packs_match_the_restatement(exe):
    blob = np.frombuffer(_run(exe, 'packs', [v for s in SHAPES for v in s]), dtype=np.uint8)
    at = 0

    def take(nbytes, dtype):
        nonlocal at
        assert at + nbytes <= blob.size, 'the program wrote less than the size functions state'
        part = blob[at:at + nbytes].view(dtype)
        at += nbytes
        return part

    for N, K in SHAPES:
        W = _matrix(N, K)
        WT = np.ascontiguousarray(W.T)
        assert len(np.unique(PR.bits(W))) == N * K
        nf, nb, nbT = 4 * PR.packed_floats(N, K), 2 * PR.packed_bf16_elems(N, K), 2 * PR.packed_bf16_elems(K, N)
        assert np.array_equal(take(nf, np.uint32), PR.bits(pack_f32(W))), ('fp32', N, K)
        assert np.array_equal(take(nf, np.uint32), PR.bits(pack_f32(PR.bf16_value(PR.bf16_bits(W))))), ('rounded fp32', N, K)
        assert np.array_equal(take(nb, np.uint16), pack_bf16(PR.bf16_bits(W)[None])), ('bf16', N, K)
        assert np.array_equal(take(3 * nb, np.uint16), pack_bf16(PR.split3(W), 3)), ('three-term', N, K)
        assert np.array_equal(take(3 * nbT, np.uint16), pack_bf16(PR.split3(WT), 3)), ('three-term of the transpose', N, K)
    assert at == blob.size, 'the program wrote more than the size functions state'


def test_three_term_split_on_the_edge_values(exe):
    """mv_x3_term on pack_ref.VALUES: the flush edge at 2^-40 and its neighbours, the binade above it, values whose second and third terms vanish, ties"""
    lines = _run(exe, 'terms', ['%08x' % b for b in PR.VALUE_BITS]).decode().splitlines()
    want = PR.split3(PR.VALUES)
    assert len(lines) == PR.VALUES.size
    for i, line in enumerate(lines):
        got = [int(v, 16) for v in line.split()]
        assert got == [int(PR.VALUE_BITS[i])] + [int(want[t, i]) for t in range(3)], line
    a = np.abs(PR.VALUES.astype(np.float64))
    assert ((a > 0) & (a < 2.0 ** -40)).any() and ((a >= 2.0 ** -40) & (a < 2.0 ** -39)).any()       # both sides of the flush edge, and the binade above it
    assert (want[1:, a >= 2.0 ** -40] == 0).all(0).any()                                              # second and third term vanish
