"""Device time of mesh simplification (Mesh.simplify, csrc/mesh_simplify.hip) on the marching-cubes mesh of a sphere of radius 0.6 over [-1, 1]^3:
the median of repeated calls after a warm-up, timed with device events, at cell = 2 h and 4 h and at target_faces = 50 000 (the whole search).
Each cell case also times the count pass alone, counts-only (what a target_faces search repeats) and full.  For scale, the host time of the numpy
restatement (tests/simplify_ref.py) on the N = 40 sphere.  Prints one JSON line.

    python tools/time_simplify.py [--resolution 256] [--repeats 9] [--only cell_2h_quadric]

The split between the sorts and the rest is the kernels' own time, from a `rocprofv3 --kernel-trace --stats` run of one case in a run of its own
(--only CASE --repeats 1), whose kernel_stats.csv this script then sums by group:

    python tools/time_simplify.py --split DIR/..._kernel_stats.csv

(sorts: k_rs_hist, k_rs_scatter and the int64 scans of their histograms; scan_top: the one-workgroup top scan both kinds of scan share; rest: the
k_sp_* passes and the flag scans.)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def sphere_mesh(n):
    from mvsdf_amd.mesh import marching_cubes
    x = torch.linspace(-1.0, 1.0, n, dtype=torch.float64, device='cuda')
    d = (x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2).sqrt() - 0.6
    h = 2.0 / (n - 1)
    return marching_cubes(d.float(), 0.0, (h,) * 3, (-1.0,) * 3), h


def median_ms(fn, repeats):
    fn()                                                              # warm-up
    rows = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        rows.append(e0.elapsed_time(e1))
    return float(np.median(rows)), rows


def split(path):
    import csv
    groups = {'sorts': 0.0, 'scan_top': 0.0, 'rest': 0.0, 'other_kernels': 0.0}
    calls = dict.fromkeys(groups, 0)
    for r in csv.DictReader(open(path)):
        name = r['Name']
        if 'k_scan_top' in name:
            g = 'scan_top'
        elif 'k_rs_' in name or ('k_scan_' in name and '<long long>' in name) or 'k_scan_block_sumIx' in name or 'k_scan_applyIx' in name:
            g = 'sorts'
        elif 'k_sp_' in name or 'k_scan_' in name:
            g = 'rest'
        else:
            g = 'other_kernels'                                        # marching cubes of the input, torch
        groups[g] += float(r['TotalDurationNs']) / 1e6
        calls[g] += int(r['Calls'])
    return {'kernel_ms': groups, 'calls': calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resolution', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--only', type=str, default=None, help='one case, e.g. cell_2h_quadric (for a profiler run)')
    ap.add_argument('--split', type=str, default=None, help='a rocprofv3 kernel_stats.csv of such a run: sum the kernels by group and exit')
    a = ap.parse_args()
    if a.split:
        print(json.dumps(split(a.split)))
        return
    assert torch.cuda.is_available(), 'time_simplify.py measures on the GPU'
    mesh, h = sphere_mesh(a.resolution)
    res = {'resolution': a.resolution, 'vertices': int(mesh.vertices.shape[0]), 'faces': len(mesh), 'cases': {}}
    for name, kw in (('cell_2h', {'cell': 2 * h}), ('cell_4h', {'cell': 4 * h}), ('target_50000', {'target_faces': 50000})):
        for placement in ('quadric', 'mean'):
            if a.only and a.only != '%s_%s' % (name, placement):
                continue
            med, rows = median_ms(lambda: mesh.simplify(placement=placement, **kw), a.repeats)
            st = dict(mesh.simplify_stats)
            row = {'median_ms': med, 'runs_ms': rows, 'stats': st}
            if 'cell' in kw:
                cnt, _ = median_ms(lambda: mesh._simplify_pass(kw['cell'], None, placement == 'quadric', True), a.repeats)
                full, _ = median_ms(lambda: mesh._simplify_pass(kw['cell'], None, placement == 'quadric', False), a.repeats)
                row.update(count_only_ms=cnt, count_full_ms=full, cluster_walk_and_corner_sort_ms=full - cnt)
            res['cases']['%s_%s' % (name, placement)] = row
    if a.only:
        print(json.dumps(res))
        return
    # the numpy restatement, for scale
    import simplify_ref as S
    v, f, n, c, hh = S.shape_mesh('sphere', 40)
    t0 = time.perf_counter()
    S.simplify(v, f, n, c, 2 * hh)
    res['numpy_restatement_n40_ms'] = (time.perf_counter() - t0) * 1e3
    m40 = type(mesh)(torch.from_numpy(v.copy()), torch.from_numpy(f.astype(np.int32)), torch.from_numpy(n.copy()), torch.from_numpy(c.copy())).to('cuda')
    res['device_n40_ms'], _ = median_ms(lambda: m40.simplify(cell=2 * hh), a.repeats)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
