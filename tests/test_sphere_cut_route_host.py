"""The sphere cut's launch rule and workspace regions (mvsdf_amd/csrc/trace_route.h: mv_sphere_cut_on, mv_trace_cut_ws) on the CPU: the header has no HIP in it, a
small program includes it alone and prints the rule over engines x row tiles x ray counts x compute units and the region offsets of a few shapes.

The rule as stated: the three-weight-term engine (3), ONE row tile per sphere workgroup, at most one workgroup per compute unit and more than one per two.  The regions: behind
mv_trace_ws(R, n).total rounded up to 256 bytes, in order and disjoint -- 16 words per ray of spilled state, one word per ray of late list, n words per ray of its
sample values -- and the late list where include/mvsdf_hip.h says it is."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, 'mvsdf_amd', 'csrc')
SRC = r'''
#include <stdio.h>
#include "trace_route.h"
int main() {
    const int Rs[] = {1, 8, 300, 512, 1024, 1032, 2040, 2048, 2049, 4096, 8192}, cus[] = {256, 64};
    for (int e = 0; e < 4; ++e) for (int mt = 1; mt <= 4; mt *= 2) for (int R : Rs) for (int cu : cus)
        printf("rule %d %d %d %d : %d\n", e, mt, R, cu, (int)mv_sphere_cut_on(e, R, mt, cu));
    const int shapes[][2] = {{1, 2}, {17, 100}, {2048, 100}, {2048, 128}, {8193, 1024}, {0, 100}};
    for (auto& s : shapes) {
        const MvTraceWs w = mv_trace_ws(s[0], s[1]);
        const MvTraceCutWs c = mv_trace_cut_ws(s[0], s[1]);
        printf("ws %d %d : %zu %zu %zu %zu %zu\n", s[0], s[1], w.total, c.spill, c.list_late, c.sv_late, c.total);
    }
    return 0;
}
'''


@pytest.fixture(scope='module')
def lines(tmp_path_factory):
    cxx = os.environ.get('CXX') or next((c for c in ('c++', 'g++', 'clang++') if shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    d = tmp_path_factory.mktemp('sphere_cut_route')
    src, exe = str(d / 'cut_route.cpp'), str(d / 'cut_route')
    with open(src, 'w') as f:
        f.write(SRC)
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', CSRC, src, '-o', exe])
    return subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.decode().splitlines()


def test_the_cut_is_on_where_the_rule_says(lines):
    rows = [l for l in lines if l.startswith('rule')]
    assert len(rows) == 4 * 3 * 11 * 2
    on = 0
    for l in rows:
        e, mt, R, cu, got = (int(v) for v in l.replace(':', ' ').split()[1:])
        want = e == 3 and mt == 1 and cu // 2 < -(-R // 8) <= cu
        assert got == int(want), l
        on += got
    assert on == 3 + 2                                            # engine 3, one tile: 1032, 2040, 2048 rays on 256 CUs; 300 and 512 rays on 64


def test_cut_regions_lie_behind_the_tracer_workspace(lines):
    rows = [l for l in lines if l.startswith('ws')]
    assert len(rows) == 6
    for l in rows:
        R, n, total, spill, late, sv, end = (int(v) for v in l.replace(':', ' ').split()[1:])
        assert total == R * (44 + 8 * n) + 256                    # (the layout tests/test_trace_route_host.py holds)
        assert spill == (total + 255) // 256 * 256 and late == spill + 64 * R and sv == late + 4 * R and end == sv + 4 * R * n + 256
