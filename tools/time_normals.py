"""Time of the stages of mvsdf_amd/normals.py on a fused-like surface cloud: a random sampling of one bumpy height field over [-1, 1]^2 (time_tnt.py's
surface; default 2e6 points, k = 16), every point seen by two to four of eight views above it.  Reported, each as min / median / max over --repeats
runs after one warm-up run, in ms, host clock around work that ends in a device synchronise:

* tree_build: registration.NearestTree(points), the sort and the boxes of csrc/nn_tree.h that knn_indices builds on every call;
* knn_indices: the rows alone (tree included);
* estimate_normals: the rows and the eigenproblem (tree included);
* orient_normals: the spanning-tree orientation by `up` from those rows, with its round count;
* orient_normals_views: the same with the component signed by the view votes (packing the mask included);
* orient_to_views: every point by its own views (packing the mask included);
* cloud_knn_mean_distance: cloud.knn_mean_distance at the same N and k, the query that keeps distances only.

Prints one JSON line.

    python tools/time_normals.py [--points 2000000] [--k 16] [--repeats 5]
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
    ap.add_argument('--k', type=int, default=16)
    ap.add_argument('--repeats', type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'time_normals.py measures on the GPU'
    from mvsdf_amd import cloud, normals
    from mvsdf_amd import registration as G
    rs = np.random.RandomState(7)
    pts = torch.from_numpy(_surface(a.points, 1)).cuda()
    V = 8
    centers = torch.from_numpy(np.concatenate([rs.uniform(-1, 1, (V, 2)), np.full((V, 1), 3.0)], 1)).cuda()
    first, count = rs.randint(0, V, a.points), rs.randint(2, 5, a.points)
    vis = torch.from_numpy((((np.arange(V)[:, None] - first[None, :]) % V) < count[None, :]).astype(np.uint8)).cuda()
    names = ('tree_build', 'knn_indices', 'estimate_normals', 'orient_normals', 'orient_normals_views', 'orient_to_views', 'cloud_knn_mean_distance')
    times = {k: [] for k in names}
    out = {'points': a.points, 'k': a.k, 'views': V, 'repeats': a.repeats}
    for rep in range(a.repeats + 1):                              # the first run warms up
        tb, _ = _timed(lambda: G.NearestTree(pts))
        tk, _ = _timed(lambda: normals.knn_indices(pts, a.k))
        te, (nrm, var, nbr) = _timed(lambda: normals.estimate_normals(pts, a.k))
        to, o = _timed(lambda: normals.orient_normals(pts, nrm, nbr))
        tw, ov = _timed(lambda: normals.orient_normals(pts, nrm, nbr, centers=centers, visibility=vis))
        tv, _ = _timed(lambda: normals.orient_to_views(pts, nrm, centers, vis))
        tc, _ = _timed(lambda: cloud.knn_mean_distance(pts, a.k))
        if rep == 0:
            out.update({'rounds': o.rounds, 'n_components': o.n_components, 'upward': float((o.normals[:, 2] > 0).double().mean()),
                        'upward_views': float((ov.normals[:, 2] > 0).double().mean()), 'median_variation': float(var.median())})
        else:
            for k, v in zip(names, (tb, tk, te, to, tw, tv, tc)):
                times[k].append(v)
    out['ms'] = {k: {'min': round(min(v), 3), 'median': round(float(np.median(v)), 3), 'max': round(max(v), 3)} for k, v in times.items()}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
