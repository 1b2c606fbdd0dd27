"""The rule, grid and LDS bytes of the sixteen-wave rows form (mvsdf_amd/csrc/trace_route.h: mv_rows16_on, mv_rows16_grid, mv_rows16_lds_bytes) on the CPU:
tests/native/fork_rule.cpp includes the header alone, is built with the host compiler and prints them over engines x widths x ray counts x row tiles x compute units.

The rule as stated: the three-weight-term engine (3), at most 16 column tiles (hidden width 256), ONE row tile per sphere workgroup and 4 * cus < R <= 8 * cus -- the
sphere cut's rule and the width.  The grid: the worst-case chunks of 32 rows, at most one workgroup per compute unit, at most `cap` where one is given.  The LDS: the
sphere kernel's formula for two row tiles with the second pair of activation tiles (64 activation rows)."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, 'mvsdf_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'native', 'fork_rule.cpp')


@pytest.fixture(scope='module')
def lines(tmp_path_factory):
    cxx = os.environ.get('CXX') or next((c for c in ('c++', 'g++', 'clang++') if shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('fork_rule') / 'fork_rule')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', CSRC, SRC, '-o', exe])
    return subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.decode().splitlines()


def _ints(line):
    return [int(v) for v in line.replace(':', ' ').split()[1:]]


def test_the_rows_form_is_on_where_the_rule_says(lines):
    rows = [l for l in lines if l.startswith('rule')]
    assert len(rows) == 4 * 4 * 5 * 2 * 2
    on = []
    for l in rows:
        e, nt, R, mt, cu, got, cut = _ints(l)
        want = e == 3 and nt <= 16 and mt == 1 and 4 * cu < R <= 8 * cu
        assert got == int(want), l
        assert not got or cut, l                                  # never on where the cut is off
        if got:
            on.append((nt, R, cu))
    assert sorted(on) == [(4, 1025, 256), (4, 2048, 256), (16, 1025, 256), (16, 2048, 256)]


def test_grid_is_chunks_bounded_by_compute_units_or_cap(lines):
    rows = [l for l in lines if l.startswith('grid')]
    assert len(rows) == 5 * 2 * 2 * 4
    seen_second_trip = False
    for l in rows:
        R, per, cu, cap, got, blocks = _ints(l)
        chunks = (R * per + 31) // 32
        assert blocks == chunks, l
        assert got == min(chunks, cap if cap > 0 else cu), l
        assert got >= 1
        seen_second_trip |= chunks > got
    assert seen_second_trip


def test_lds_bytes_are_the_sphere_kernels_formula(lines):
    rows = [l for l in lines if l.startswith('lds')]
    assert len(rows) == 4
    for l in rows:
        S, mr, got, sphere = _ints(l)
        floats = 64 * S + ((32 * (3 + 6 * mr) + 3) & ~3) + 32 * 4 + 32
        assert got == sphere == 4 * floats + 32, l
        assert got <= 160 * 1024, l                               # one workgroup per CU must fit the 160 KiB of LDS


def test_the_rule_names_its_uses(lines):
    uses = [int(l.split()[1]) for l in lines if l.startswith('uses')]
    assert len(uses) == 1 and 0 <= uses[0] <= 3
