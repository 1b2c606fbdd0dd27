"""Time of the cloud cleaning (mvsdf_amd/cloud.py, csrc/cloud.hip) on the fused cloud of tools/time_fusion.py's scene (49 views of 600 x 800, about
2 * 10^7 points) plus 1 % injected outliers (uniform within +-3 extents of the box centre), and on random subsets of --sizes points.

A host clock around each stage, closed by the stage's header read (plus a synchronize): stage A alone (knn_mean_distance), stage C alone
(radius_components at the eps the cleaning used) and the whole clean_points; the median of --repeats runs after a warm-up, one JSON line per
size.  Beside it, from the same process, chamfer.nearest_distance of one half of the cloud against the other (the existing 1-nearest walk, per
query).  --cpu times the numpy restatement (tests/cloud_ref.py) at --cpu_points points instead.  For the split by kernel run the script under
rocprofv3 --kernel-trace --stats in a run of its own (--repeats 1 --sizes N).

    python tools/time_clean.py [--views 49 --hw 600,800 --sizes 300000,3000000,0 --repeats 5] [--cpu [--cpu_points 30000 --jobs 1]]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _timed(fn, repeats):
    out = fn()                                                                # warm-up
    torch.cuda.synchronize()
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) * 1e3)
    return out, runs


def _ms(runs):
    return {'median_ms': round(float(np.median(runs)), 2), 'runs_ms': [round(v, 2) for v in runs]}


def scene_cloud(views, hw, view):
    """the fused cloud of time_fusion.py's scene plus 1 % outliers, shuffled -> fp64 [N,3] on the device"""
    import time_fusion
    from mvsdf_amd import fusion
    cams, depths, pairs = time_fusion.scene(views, hw, view)
    pts = fusion.fuse_depths(cams, torch.from_numpy(depths).cuda(), pairs, view=view).points
    g = torch.Generator(device='cuda').manual_seed(0)
    lo, hi = pts.amin(0), pts.amax(0)
    out = (lo + hi) / 2 + (torch.rand(len(pts) // 100, 3, dtype=torch.float64, device='cuda', generator=g) * 6 - 3) * (hi - lo).max()
    pts = torch.cat([pts, out])
    return pts[torch.randperm(len(pts), device='cuda', generator=g)].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=49)
    ap.add_argument('--hw', type=str, default='600,800')
    ap.add_argument('--view', type=int, default=10)
    ap.add_argument('--sizes', type=str, default='300000,3000000,0', help='subset sizes; 0 = the whole cloud')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--nb_neighbors', type=int, default=20)
    ap.add_argument('--cpu', action='store_true')
    ap.add_argument('--cpu_points', type=int, default=30000)
    ap.add_argument('--jobs', type=int, default=1)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'time_clean.py builds its cloud with the on-device fusion'
    from mvsdf_amd import chamfer, cloud
    whole = scene_cloud(a.views, tuple(int(v) for v in a.hw.split(',')), a.view)
    if a.cpu:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import cloud_ref
        P = whole[:a.cpu_points].cpu().numpy()
        t0 = time.perf_counter()
        c = cloud_ref.clean(P, k=a.nb_neighbors, jobs=a.jobs)
        print(json.dumps({'path': 'numpy', 'points': len(P), 'jobs': a.jobs, 'measured_s': round(time.perf_counter() - t0, 2), 'kept': int(c['keep'].sum())}))
        return
    for size in [int(s) for s in a.sizes.split(',')]:
        P = whole if size == 0 or size >= len(whole) else whole[:size].contiguous()          # the cloud is shuffled: a prefix is a random subset
        c, clean_runs = _timed(lambda: cloud.clean_points(P, nb_neighbors=a.nb_neighbors), a.repeats)
        _, knn_runs = _timed(lambda: cloud.knn_mean_distance(P, a.nb_neighbors), a.repeats)
        _, cc_runs = _timed(lambda: cloud.radius_components(P, c.eps), a.repeats)
        half = len(P) // 2
        _, nn_runs = _timed(lambda: chamfer.nearest_distance(P[:half], P[half:], max_dist=1e30), a.repeats)
        print(json.dumps({'path': 'hip', 'points': len(P), 'nb_neighbors': a.nb_neighbors, 'kept': len(c), 'passed': c.n_passed, 'clusters': c.n_clusters,
                          'rounds': c.rounds, 'median': c.median, 'eps': c.eps, 'clean_points': _ms(clean_runs), 'knn_mean_distance': _ms(knn_runs),
                          'radius_components_at_eps': _ms(cc_runs),
                          'yardstick_chamfer_nearest_half_vs_half': dict(_ms(nn_runs), queries=half, refs=len(P) - half)}), flush=True)


if __name__ == '__main__':
    main()
