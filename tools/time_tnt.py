"""Time of the pieces of the registration and F-score evaluation (mvsdf_amd/registration.py, csrc/registration.hip) on synthetic clouds: two
independent samplings of one bumpy height field over [-1, 1]^2 (default 2e6 x 2e6 points), the source moved by 1 degree and 0.004.  Reported, each
as min / median / max over --repeats runs after one warm-up run, in ms, host clock around work that ends in a device synchronise:

* tree_build: NearestTree(target) (the sort, the boxes; one wait);
* query: one tree.query of the whole source, max_dist 0.05, the error word not read (launch + synchronise);
* icp_iteration: one evaluation of the ICP (transform, query, the 17 sums, the wait that reads them) plus the host solve;
* voxel: voxel_downsample of the source at 0.004;
* fscore: both trees, both queries and both histograms at tau 0.004; query_inf and hist: a query with max_dist = +inf (fscore itself cuts its
  walks off at the last edge) and one histogram alone;
* chamfer_nearest: chamfer.nearest_distance on the same clouds (it builds its tree on every call), measured alternately with
  tree_build + query in the same loop, the comparison DESIGN.md reports.

Prints one JSON line.

    python tools/time_tnt.py [--points 2000000] [--repeats 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _surface(n, seed):
    xy = np.random.RandomState(seed).uniform(-1, 1, (n, 2))
    x, y = xy[:, 0], xy[:, 1]
    z = 0.25 * np.sin(2.3 * x + 0.4) * np.cos(1.7 * y - 0.3) + 0.1 * np.sin(5.1 * x * y + 1.0) + 0.06 * np.cos(7.0 * x - 3.0 * y)
    return np.concatenate([xy, z[:, None]], 1)


def _timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=2_000_000)
    ap.add_argument('--repeats', type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'time_tnt.py measures on the GPU'
    from mvsdf_amd import chamfer as C
    from mvsdf_amd import registration as G
    c, s = np.cos(np.radians(1.0)), np.sin(np.radians(1.0))
    move = np.array([[c, -s, 0, 0.004], [s, c, 0, -0.003], [0, 0, 1, 0.002], [0, 0, 0, 1.0]])
    tgt = torch.from_numpy(_surface(a.points, 1)).cuda()
    src = G.transform_points(torch.from_numpy(_surface(a.points, 2)).cuda(), move)
    tau, max_dist = 0.004, 0.05
    times = {k: [] for k in ('tree_build', 'query', 'build_plus_query', 'chamfer_nearest', 'icp_iteration', 'voxel', 'fscore', 'query_inf', 'hist')}
    out = {'points': a.points, 'repeats': a.repeats, 'tau': tau, 'max_dist': max_dist}
    for rep in range(a.repeats + 1):                              # the first run warms up
        tb, tree = _timed(lambda: G.NearestTree(tgt))
        tq, (dist, index) = _timed(lambda: tree.query(src, max_dist, check_finite=False))
        tc, ref = _timed(lambda: C.nearest_distance(src, tgt, max_dist))
        pr = G._Pairs(src, tree, 'time_tnt')

        def iteration():
            n, sums = pr.sums([list(r) for r in G.IDENTITY], max_dist, 'time_tnt')
            return n, G.horn_update(n, sums, tree.centre)
        ti, (n, U) = _timed(iteration)
        tv, (means, counts) = _timed(lambda: G.voxel_downsample(src, tau))
        tf, f = _timed(lambda: G.fscore(src, tgt, tau))
        tn, (dinf, _) = _timed(lambda: tree.query(src, check_finite=False))
        edges = torch.from_numpy(f['edges']).cuda()
        th, hist = _timed(lambda: G._hist(dinf, edges, tau))
        if rep == 0:
            assert torch.equal(dist, ref), 'NearestTree.query and chamfer.nearest_distance disagree'
            assert int(hist[0]) == f['below_rec'] and torch.equal(hist[1:].cpu(), torch.from_numpy(f['hist_rec']))
            out.update({'matched': n, 'voxels': int(means.shape[0]), 'precision': f['precision'], 'recall': f['recall'], 'fscore': f['fscore']})
        else:
            for k, v in zip(times, (tb, tq, tb + tq, tc, ti, tv, tf, tn, th)):
                times[k].append(v)
    out['ms'] = {k: {'min': round(min(v), 3), 'median': round(float(np.median(v)), 3), 'max': round(max(v), 3)} for k, v in times.items()}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
