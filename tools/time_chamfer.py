"""Time of each stage of the DTU Chamfer evaluation (mvsdf_amd/chamfer.py, csrc/chamfer.hip) on a synthetic DTU-sized scene in a world-mm frame:

* the evaluated mesh: marching cubes of a bumpy sphere of radius ~155 mm (about 3e5 mm^2, so about area / density^2 = 7e6 samples at 0.2);
* the stl points: 2.5e6 points on the sphere of radius + 0.5 mm, none on the cap z > 0.7 r, so that about 10 % of the mesh (z > 0.8 r) lies more
  than 20 mm from every reference point;
* an all-true observation mask at 2 mm over the whole scene, patch 60, a ground plane below the scene.

Each stage ends in a host wait (its header read), so a host clock around it is the device time plus the launch overhead.  Prints one JSON line
with the medians per stage and in total, the downsampling's round count and the counts.  --cpu runs the same scene through DTUeval-python's
formulation in numpy and scikit-learn (tests/golden/chamfer/make_chamfer_golden.py; kd-tree queries on --jobs threads) once instead.

    python tools/time_chamfer.py [--repeats 3] [--cpu [--jobs 16]]
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

R = 155.0


def _volume(xp, g):
    x, y, z = xp.meshgrid(g, g, g, indexing='ij')
    return xp.sqrt(x * x + y * y + z * z) - R - 2.0 * xp.sin(x / 9.0) * xp.cos(y / 11.0)


def _reference():
    """-> (stl fp64 [M, 3], obs_mask, bb, res, plane)"""
    rs = np.random.RandomState(0)
    d = rs.randn(3_000_000, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = R * d[d[:, 2] <= 0.7][:2_500_000]
    stl = p * (1 + (0.5 - 2.0 * np.sin(p[:, :1] / 9.0) * np.cos(p[:, 1:2] / 11.0)) / R)
    bb = np.array([[-1.1 * R] * 3, [1.1 * R] * 3], np.float32)                 # the mask covers the whole mesh, the far cap included
    res = 2.0
    obs = np.ones(tuple(int(v) for v in np.ceil((bb[1] - bb[0]) / res) + 1), bool)
    return stl, obs, bb, res, np.array([0.0, 0.0, 1.0, 1.2 * R])


N_GRID = 220


def gpu(a):
    from mvsdf_amd import chamfer as C
    assert torch.cuda.is_available(), 'time_chamfer.py measures on the GPU (--cpu for the numpy / scikit-learn path)'
    from mvsdf_amd.mesh import marching_cubes
    g = torch.linspace(-1.15 * R, 1.15 * R, N_GRID, dtype=torch.float64, device='cuda')
    h = float(g[1] - g[0])
    mesh = marching_cubes(_volume(torch, g).float(), 0.0, spacing=(h, h, h), origin=(float(g[0]),) * 3)
    stl, obs, bb, res, plane = _reference()
    s = torch.from_numpy(stl).cuda()
    out = {'faces': len(mesh), 'vertices': int(mesh.vertices.shape[0]), 'area_mm2': mesh.area(), 'stl': len(stl), 'stages_ms': {}, 'runs_ms': []}
    times = {k: [] for k in ('sample', 'downsample', 'mask', 'd2s', 's2d', 'total')}
    for rep in range(a.repeats + 1):                              # the first run warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pts = C.sample_mesh(mesh, 0.2)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        kept, n_down, rounds = C._downsample(pts, 0.2, 0, None)
        t2 = time.perf_counter()
        d_in, d_obs, s_above = C._masks(pts, kept, s, obs, bb, res, plane, 60, 'time_chamfer')
        t3 = time.perf_counter()
        dist_d2s, used_d2s, sum_d2s = C._nearest(d_obs, s, 20.0)
        t4 = time.perf_counter()
        dist_s2d, used_s2d, sum_s2d = C._nearest(s_above, d_in, 20.0)
        t5 = time.perf_counter()
        if rep:
            for k, v in zip(times, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4, t5 - t0)):
                times[k].append(v * 1e3)
    out['stages_ms'] = {k: round(float(np.median(v)), 2) for k, v in times.items()}
    out['runs_ms'] = [round(v, 2) for v in times['total']]
    out.update({'points': int(pts.shape[0]), 'down': n_down, 'rounds': rounds, 'in': len(d_in), 'obs': len(d_obs), 'stl_above': len(s_above),
                'd2s_used': used_d2s, 'far_fraction_d2s': round(1 - used_d2s / max(1, len(d_obs)), 4), 's2d_used': used_s2d,
                'mean_d2s': sum_d2s / used_d2s, 'mean_s2d': sum_s2d / used_s2d})
    out['overall'] = (out['mean_d2s'] + out['mean_s2d']) / 2
    return out


def cpu(a):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden', 'chamfer'))
    import make_chamfer_golden as script
    import mc_ref
    g = np.linspace(-1.15 * R, 1.15 * R, N_GRID)
    v, f, _ = mc_ref.marching_cubes(_volume(np, g).astype(np.float32), spacing=(g[1] - g[0],) * 3, origin=(g[0],) * 3)
    stl, obs, bb, res, plane = _reference()
    t0 = time.perf_counter()
    data = script.script_sample(v.astype(np.float64), f.astype(np.int64), 0.2)
    t1 = time.perf_counter()
    r = script.script_eval(data, stl, obs, bb, res, plane, 0.2, 60, 20.0, 0, n_jobs=a.jobs)
    t2 = time.perf_counter()
    return {'cpu_jobs': a.jobs, 'points': len(data), 'sample_s': round(t1 - t0, 1), 'downsample_mask_distances_s': round(t2 - t1, 1),
            'total_s': round(t2 - t0, 1), 'mean_d2s': float(r['mean_d2s']), 'mean_s2d': float(r['mean_s2d']), 'overall': float(r['overall'])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--cpu', action='store_true')
    ap.add_argument('--jobs', type=int, default=16)
    a = ap.parse_args()
    print(json.dumps(cpu(a) if a.cpu else gpu(a)))


if __name__ == '__main__':
    main()
