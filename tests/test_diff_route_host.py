"""The route table of the differentiable MLP passes (mvsdf_amd/csrc/diff_route.h: development switches -> kernel family and template instance of every pass of
csrc/diff_mlp.hip) on the CPU.  The header has no HIP in it: tests/native/diff_route_table.cpp includes it alone, is compiled with the host C++ compiler and
prints the route of every pass over {column tiles of the net} x {16-row tiles} x {each switch alone, none} x {x3 packs} x {gather / sub-range / counts asked for}.
The program sets each switch as the ENVIRONMENT VARIABLE the development library reads (the header's mv_switches_from_env with getenv), so a mistyped
variable name fails here too.  What stays outside this test is the launchers' map from a route's instance to the kernel template (HIP code): they refuse an
instance their family does not list, and profiles/diff_routes_ab.txt records the kernels each switch launched on the GPU.

tests/golden/diff_routes.txt was written from the dispatch code this header replaced and confirmed once against the kernels both libraries launched
(profiles/diff_routes_ab.txt).  tests/test_gpu_alt_paths.py checks that the reference fixtures pass under each switch; what it cannot see is a switch that
silently falls through to the default kernels -- test_every_switch_selects_its_route does."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, 'mvsdf_amd', 'csrc')
PASSES = ('fwd', 'bwd', 'pair', 'delta', 'rfwd', 'rbwd')


@pytest.fixture(scope='module')
def table(tmp_path_factory):
    cxx = os.environ.get('CXX') or next((c for c in ('c++', 'g++', 'clang++') if shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('diff_route') / 'diff_route_table')
    subprocess.check_call([cxx, '-std=c++17', '-O0', '-Wall', '-Werror', '-I', CSRC, os.path.join(ROOT, 'tests', 'native', 'diff_route_table.cpp'), '-o', exe])
    return subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.decode()


def _parse(text):
    """-> {(switch, ntw, tiles, x3, opt): {column: value}}; a route is ('f32', mt, ntw, nw, pd) or ('refuse', rc)"""
    rows = {}
    for line in text.splitlines():
        head, cols = line.split(' :')
        if head.startswith('edge'):
            continue
        sw, rest = head.split(' ', 1)
        key = (sw,) + tuple(int(v) for v in re.findall(r'=(-?\d+)', rest))
        d = {}
        for name, val in re.findall(r'(\w+)=(\S+)', cols):
            m = re.match(r'(\w+)[<(]([-\d,]+)[>)]$', val)
            d[name] = (m.group(1),) + tuple(int(v) for v in m.group(2).split(',')) if m else int(val)
        rows[key] = d
    return rows


def test_route_table_matches_the_committed_one(table):
    with open(os.path.join(ROOT, 'tests', 'golden', 'diff_routes.txt')) as f:
        want = f.read()
    assert len(table.splitlines()) == 11 * 3 * 5 * 2 * 2 + 8
    assert table == want


def test_every_switch_selects_its_route(table):
    rows = _parse(table)
    fam = lambda r: r[0]
    for ntw in (2, 4):
        for tiles in (1, 256, 257, 512, 513):
            base = rows[('none', ntw, tiles, 1, 0)]
            assert [fam(base[p]) for p in PASSES] == ['x3', 'x3', 'x3', 'scale', 'f32', 'f32'] and base['layer_mt'] == (1 if tiles <= 512 else 2) and base['xcd'] == 1
            # MVSDF_FUSE=0: the per-layer kernels wherever an entry point has them (the pair has none: its caller falls back), and the fp32 arithmetic
            r = rows[('fuse=0', ntw, tiles, 1, 0)]
            assert [fam(r[p]) for p in ('fwd', 'bwd', 'rfwd', 'rbwd')] == ['layers'] * 4 and fam(r['pair']) == 'f32'
            r = rows[('fuse=0', ntw, tiles, 1, 1)]
            assert r['fwd'] == ('refuse', 1) and r['rbwd'] == ('refuse', -3)
            # MVSDF_SPLIT_CHAINS=1: E.1 / E.2 launches (8 waves, the net's column tiles per wave), the fp32 arithmetic elsewhere
            r = rows[('split_chains=1', ntw, tiles, 1, 0)]
            assert r['bwd'] == ('split', 1, ntw, 8, 0) and fam(r['fwd']) == 'f32' and fam(r['pair']) == 'f32'
            # MVSDF_CHAIN_W8=1: every chain at 8 waves, one row tile, the net's column tiles per wave (the product: 16 waves)
            r = rows[('chain_w8=1', ntw, tiles, 1, 0)]
            for p in ('fwd', 'bwd', 'pair', 'rfwd', 'rbwd'):
                assert r[p] == ('f32', 1, ntw, 8, 0), p
                assert base[p][3] == 16 or (base[p][:2] == ('x3', 2) and ntw == 4), p      # (the x3 chains' two-tile form at widths above 256 has 8 waves)
            # MVSDF_CHAIN_X3=0: the fp32 chains although the packs exist
            r = rows[('chain_x3=0', ntw, tiles, 1, 0)]
            assert [fam(r[p]) for p in ('fwd', 'bwd', 'pair')] == ['f32'] * 3
            # MVSDF_DELTA_CHAIN=1: the delta pass as a chain, and no deferred step
            r = rows[('delta_chain=1', ntw, tiles, 1, 0)]
            assert fam(r['delta']) == 'f32' and rows[('delta_chain=1', ntw, tiles, 1, 1)]['delta'] == ('refuse', -3) and r['defer'] == 0 and base['defer'] == 1
            assert rows[('wg_xcd=0', ntw, tiles, 1, 0)]['xcd'] == 0
            # MVSDF_CHAIN_W8=0 is 'set': the fp32 arithmetic (historical), at the product's 16 waves
            r = rows[('chain_w8=0', ntw, tiles, 1, 0)]
            assert [fam(r[p]) for p in ('fwd', 'bwd', 'pair')] == ['f32'] * 3 and r['bwd'][3] == 16
        # MVSDF_CHAIN_MT: two row tiles where the cost model takes one, one where it takes two (x3 chains, and fp32 chains at widths <= 256)
        for x3 in (0, 1):
            if ntw == 4 and not x3:
                continue                                           # the fp32 chains have no two-tile form above width 256
            for p in ('fwd', 'pair'):
                assert rows[('none', ntw, 1, x3, 0)][p][1] == 1 and rows[('chain_mt=2', ntw, 1, x3, 0)][p][1] == 2, p
                assert rows[('none', ntw, 257, x3, 0)][p][1] == 2 and rows[('chain_mt=1', ntw, 257, x3, 0)][p][1] == 1, p
        # MVSDF_LAYER_MT=1: one row tile per k_layer workgroup above 8192 rows too
        assert rows[('none', ntw, 513, 1, 0)]['layer_mt'] == 2 and rows[('layer_mt=1', ntw, 513, 1, 0)]['layer_mt'] == 1


def test_can_defer_is_all_backward_passes_take_counts(table):
    rows = _parse(table)
    seen = set()
    for (sw, ntw, tiles, x3, opt), r in rows.items():
        with_cnt = rows[(sw, ntw, tiles, x3, 1)]
        takes = all(with_cnt[p][0] in ('f32', 'x3', 'scale') for p in ('pair', 'delta', 'rbwd'))
        assert r['defer'] == int(takes), (sw, ntw, tiles, x3, opt)
        seen.add(r['defer'])
    assert seen == {0, 1}
