"""The launch rules of the tracer (mvsdf_amd/csrc/trace_route.h: switches, engine class, template instance of every stage, tail filling, grids, LDS bytes,
workspace layout) on the CPU.  The header has no HIP in it: tests/native/trace_route_table.cpp includes it alone, is compiled with the host C++ compiler and
prints one line per {each switch alone, none} x {engine} x {widest hidden layer in 16-column tiles} x {mt = mt_samples} x {rays} x {training} x {steps given} x
{n_steps} x {compute units}, then the workspace offsets of eight shapes.  The program sets each switch as the ENVIRONMENT VARIABLE the library reads, so a
mistyped variable name fails here too.  What stays outside this test is the launchers' map from an instance to the kernel template (HIP code): they refuse an
instance their engine does not list (the sets below), and profiles/trace_routes_ab.txt records the kernels each configuration launched on the GPU.

tests/golden/trace_routes.txt.xz was written from the code this header replaced: a throw-away program that held the ladders of mv_trace_launch, dispatch_col0_bf
and mvsdf_sdf_col0, mv_tail_on, the grid and LDS arithmetic of launch_stage1 / launch_stage2 and the pointer arithmetic of the workspace verbatim, with the
launches turned into prints.  Where that code had a branch that cannot be reached (four waves x eight column tiles), the table never shows it.  The table has
414 728 lines (60 MB); the file is its xz form (`xz -dc` prints it), since no committed file may exceed 1 MiB.

The GPU tests hold the tracer's RESULTS to the oracle bit for bit; every instance gives the same bits, so a rule that silently fell through to another instance
would pass them -- test_every_switch_selects_its_route and the table do not."""
import lzma
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, 'mvsdf_amd', 'csrc')
SWITCHES = ('none', 'tail=0', 'tail=2', 'tail_stop=0', 'nfirst=1', 'nfirst=100', 'nfirst=200', 'mt_first=2', 'bf_carry=1')
ENGINES = (0, 1, 2, 3)                     # MvNet, MvNetBs<2>, MvNetBs<3>, MvNetBs<3, 3>
MAXNT, MT, N_STEPS, CUS = (4, 15, 16, 17, 32, 33), (0, 1, 2, 3, 4, 49), (2, 12, 13, 100), (256, 64)
N_R = 10                                   # 1, 17, 2048, 2049, 4096, 4097, 8192, 8193, 256 * 8 * mt1 -+ 1
COLUMNS = ('sphere', 'p1', 'p2', 'p4', 'p8', 'col0', 'tail', 'stop_left', 'nf', 'g_sphere', 'g_first', 'g_rest', 'g_part2', 'g_part4', 'g_sec', 'g_red') + \
    tuple('lds%d_%s' % (S, k) for S in (68, 260) for k in ('sphere', 'sphere2', 'p2', 'p22', 'col0'))
WS_SHAPES = ((1, 2), (17, 100), (2048, 128), (8193, 1024), (0, 100), (-5, 100), (17, 0), (17, -3))

# The instances the launchers' switches accept (trace.hip::mv_launch_inst, basic.hip::dispatch_col0), per engine: <mt.ntw.nw>, col0 with its carried-fetch flag
_EIGHT = {'1.2.8', '2.2.8', '4.2.8', '1.4.8', '2.4.8'}
_FOUR = {'1.4.4', '2.4.4', '4.4.4'}
SPHERE = {0: _EIGHT | _FOUR, 1: _EIGHT, 2: _EIGHT, 3: (_EIGHT - {'1.2.8'}) | {'1.1.16'}}
SAMPLES = {0: _EIGHT | _FOUR, 1: _EIGHT, 2: _EIGHT, 3: _EIGHT}
COL0 = {0: {i + '.0' for i in _EIGHT | _FOUR} | {'1.2.8.1'}, 1: {i + x for i in _EIGHT for x in ('.0', '.1')}}
COL0[2] = COL0[3] = COL0[1]


@pytest.fixture(scope='module')
def table(tmp_path_factory):
    cxx = os.environ.get('CXX') or next((c for c in ('c++', 'g++', 'clang++') if shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('trace_route') / 'trace_route_table')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', CSRC, os.path.join(ROOT, 'tests', 'native', 'trace_route_table.cpp'), '-o', exe])
    return subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.decode()


@pytest.fixture(scope='module')
def rows(table):
    """{(switch, engine, maxnt, mt, R, training, steps, n_steps, cus): {column: value}} and the list of ws lines"""
    out, ws = {}, []
    for line in table.splitlines():
        head, cols = line.split(' :')
        head, cols = head.split(), cols.split()
        if head[0] == 'ws':
            ws.append((int(head[1]), int(head[2]), [int(v) for v in cols]))
            continue
        key = (head[0],) + tuple(int(v) for v in head[1:])
        row = dict(zip(COLUMNS, cols[:6] + [int(v) for v in cols[6:]]))
        assert out.setdefault(key, row) == row                     # (mt1 = 1: 256 * 8 + 1 is the 2049 of the fixed sizes too)
        assert len(cols) in (6, len(COLUMNS))
    return out, ws


def test_route_table_matches_the_committed_one(table):
    with lzma.open(os.path.join(ROOT, 'tests', 'golden', 'trace_routes.txt.xz'), 'rt') as f:
        want = f.read()
    assert len(table.splitlines()) == len(SWITCHES) * len(ENGINES) * len(MAXNT) * len(MT) * N_R * 2 * 2 * len(N_STEPS) * len(CUS) + len(WS_SHAPES)
    assert table == want


def _others(a, b, moved):
    return all(a[c] == b[c] for c in a if c not in moved)


def test_every_switch_selects_its_route(rows):
    rows = rows[0]
    seen = {s: 0 for s in SWITCHES}
    for key, base in rows.items():
        if key[0] != 'none':
            continue
        eng, maxnt, mt, R, tr, st, n, cus = key[1:]
        sw = {s: rows[(s,) + key[1:]] for s in SWITCHES[1:]}
        # MVSDF_BF_CARRY moves col0's form only, and only the bf16-term engines have it
        r = sw['bf_carry=1']
        assert _others(base, r, ('col0',))
        if eng and maxnt <= 32:
            assert base['col0'].endswith('.0') and r['col0'] == base['col0'][:-1] + '1'
            seen['bf_carry=1'] += 1
        else:
            assert r['col0'] == base['col0']
        if maxnt > 32:                                                             # the tracer refuses the network: no decisions on the line
            assert all(len(r) == 6 and r['sphere'] == 'r1' for r in list(sw.values()) + [base])
            continue
        # MVSDF_TAIL=0 turns tail filling off wherever the default has it on (the queue's extra workgroup goes with it) ...
        r = sw['tail=0']
        assert r['tail'] == 0 and _others(base, r, ('tail', 'g_part2', 'g_part4'))
        assert (r['g_part2'], r['g_part4']) == (base['g_part2'] - base['tail'], base['g_part4'] - base['tail'])
        seen['tail=0'] += base['tail']
        # ... the default has it on for the fp32 engine and, above 2048 rays, the three-weight-term engine; =2 for every engine; always inside the compute-unit bound
        inside = bool(tr and st and base['g_sphere'] <= cus)
        assert base['tail'] == int(inside and (eng == 0 or (eng == 3 and R > 2048)))
        r = sw['tail=2']
        assert r['tail'] == int(inside) and _others(base, r, ('tail', 'g_part2', 'g_part4'))
        seen['tail=2'] += r['tail'] and not base['tail'] and eng in (1, 2)
        # MVSDF_TAIL_STOP moves stop_left only
        r = sw['tail_stop=0']
        assert base['stop_left'] == base['g_sphere'] // 4 and r['stop_left'] == 0 and _others(base, r, ('stop_left',))
        seen['tail_stop=0'] += base['stop_left'] > 0
        # MVSDF_NFIRST moves nf and the two sampler grids (at least 2, at most n_steps)
        assert base['nf'] == min(12, n)
        for name, want in (('nfirst=1', 2), ('nfirst=100', min(100, n)), ('nfirst=200', n)):
            r = sw[name]
            assert r['nf'] == want and _others(base, r, ('nf', 'g_first', 'g_rest'))
            rows16 = 16 * int(base['p1'].split('.')[0])
            assert r['g_first'] == -(-R * want // rows16) and r['g_rest'] == -(-R * (n - want) // rows16)
            seen[name] += want != base['nf']
        # MVSDF_MT_FIRST moves the instance of part 1 only (and the grids of its two launches with it)
        r = sw['mt_first=2']
        assert r['p1'].split('.')[0] == '2' and _others(base, r, ('p1', 'g_first', 'g_rest'))
        seen['mt_first=2'] += r['p1'] != base['p1']
    assert all(seen[s] > 100 for s in SWITCHES[1:]), seen


def test_every_instance_is_one_the_launchers_accept(rows):
    launched = {'sphere': set(), 'samples': set(), 'col0': set()}
    for key, r in rows[0].items():
        eng, maxnt = key[1], key[2]
        insts = [r[c] for c in COLUMNS[:6]]
        assert all(i.startswith('r') or not (i.split('.')[1] == '8' and i.split('.')[2] == '4') for i in insts), (key, insts)      # no 4 waves x 8 column tiles
        assert all((i == 'r1') == (maxnt > 32) for i in insts[:5])
        if maxnt <= 32:
            assert insts[0] in SPHERE[eng] and all(i in SAMPLES[eng] for i in insts[1:5]), (key, insts)
            launched['sphere'].add((eng, insts[0]))
            launched['samples'].update((eng, i) for i in insts[1:5])
        assert insts[5] == 'r-1' or insts[5] in COL0[eng], (key, insts)
        if insts[5] != 'r-1':
            launched['col0'].add((eng, insts[5]))
        # the bf16-term engines refuse only networks that are too wide (no check of mt: historical); the fp32 engine an mt outside 1, 2, 4, 49 and mt 49 above width 256
        assert (insts[5] == 'r-1') == ((maxnt > 32) if eng else (key[3] not in (1, 2, 4, 49) or (key[3] == 49 and maxnt > 16)))
    # ... and the table reaches every instance the launchers list
    assert launched['sphere'] == {(e, i) for e in ENGINES for i in SPHERE[e]}
    assert launched['samples'] == {(e, i) for e in ENGINES for i in SAMPLES[e]}
    assert launched['col0'] == {(e, i) for e in ENGINES for i in COL0[e]}


def test_workspace_regions_are_disjoint_in_order_and_fill_the_total(rows):
    ws = rows[1]
    assert [(R, n) for R, n, _ in ws] == list(WS_SHAPES)
    for R, n, off in ws:
        r, n = max(R, 0), max(n, 0)
        words = (1, 1, 4, 1, 1, 1, n, 1, 1, n)                      # 4-byte words per ray of w_zmin .. the min-sdf rows' sample values
        assert off[0] == 0 and len(off) == len(words) + 1
        for i, w in enumerate(words[:-1]):
            assert off[i + 1] == off[i] + 4 * r * w, (R, n, i)
        assert off[9] + 4 * r * words[-1] == off[10] - 256
        assert off[10] == r * (44 + 8 * n) + 256
        assert [o // (4 * r) for o in off[:6]] == [0, 1, 2, 6, 7, 8] if r else set(off[:10]) == {0}
