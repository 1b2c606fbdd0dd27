#!/usr/bin/env python3
"""Generate the Chamfer fixtures tests/golden/chamfer/*.npz (tests/test_chamfer_host.py, tests/test_gpu_chamfer.py).

An independent pin of mvsdf_amd/chamfer.py's metric: every step is run in DTUeval-python's own formulation, with its unseeded shuffle replaced by
the seeded order (ascending splitmix64(seed ^ i)):
  * sampling with np.linalg.norm, np.cross and np.mgrid (sample_single_tri);
  * the greedy loop over scikit-learn's NearestNeighbors(algorithm='kd_tree').radius_neighbors on the shuffled cloud;
  * the script's masking lines (BB as fp32, np.around, the ground plane on homogeneous points);
  * kneighbors(n_neighbors=1) for both directions and numpy's mean of the distances below max_dist.
Meshes come from tests/mc_ref.py over small analytic volumes plus hand-made faces (zero area, slivers with n1 = 0); point clouds sit on a lattice of
quarter steps so that grid coordinates land exactly on .5 and stl points exactly on the plane.  Each fixture stores the inputs and
  samples (the cloud P), kept (bool over P), in / obs (bool over the kept points, input order), above (bool over stl), dist_d2s / dist_s2d (the
  script's distances, +inf where not < max_dist, in input order) and mean_d2s / mean_s2d / overall.

    python tests/golden/chamfer/make_chamfer_golden.py
"""
import os
import sys

import numpy as np
from sklearn.neighbors import NearestNeighbors

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..'))
import chamfer_ref  # noqa: E402  (only for the seeded keys)
import mc_ref  # noqa: E402


def sample_single_tri(input_):
    n1, n2, v1, v2, tri_vert = input_
    c = np.mgrid[:n1 + 1, :n2 + 1]
    c += 0.5
    c[0] /= max(n1, 1e-7)
    c[1] /= max(n2, 1e-7)
    c = np.transpose(c, (1, 2, 0))
    k = c[c.sum(axis=-1) < 1]
    q = v1 * k[:, :1] + v2 * k[:, 1:] + tri_vert
    return q


def script_sample(vertices, triangles, thresh):
    tri_vert = vertices[triangles]
    v1 = tri_vert[:, 1] - tri_vert[:, 0]
    v2 = tri_vert[:, 2] - tri_vert[:, 0]
    l1 = np.linalg.norm(v1, axis=-1, keepdims=True)
    l2 = np.linalg.norm(v2, axis=-1, keepdims=True)
    area2 = np.linalg.norm(np.cross(v1, v2), axis=-1, keepdims=True)
    non_zero_area = (area2 > 0)[:, 0]
    l1, l2, area2, v1, v2, tri_vert = [arr[non_zero_area] for arr in [l1, l2, area2, v1, v2, tri_vert]]
    thr = thresh * np.sqrt(l1 * l2 / area2)
    n1 = np.floor(l1 / thr)
    n2 = np.floor(l2 / thr)
    new_pts = [sample_single_tri((n1[i, 0], n2[i, 0], v1[i:i + 1], v2[i:i + 1], tri_vert[i:i + 1, 0])) for i in range(len(n1))]
    new_pts = np.concatenate(new_pts, axis=0) if new_pts else np.zeros((0, 3))
    return np.concatenate([vertices, new_pts], axis=0)


def script_eval(data_pcd, stl, ObsMask, BB, Res, ground_plane, thresh, patch, max_dist, seed, n_jobs=1):
    order = np.argsort(chamfer_ref.keys(len(data_pcd), seed), kind='stable')     # the seeded shuffle
    shuffled = data_pcd[order]
    nn_engine = NearestNeighbors(n_neighbors=1, radius=thresh, algorithm='kd_tree', n_jobs=n_jobs)
    nn_engine.fit(shuffled)
    rnn_idxs = nn_engine.radius_neighbors(shuffled, radius=thresh, return_distance=False)
    mask = np.ones(shuffled.shape[0], dtype=np.bool_)
    for curr, idxs in enumerate(rnn_idxs):
        if mask[curr]:
            mask[idxs] = 0
            mask[curr] = 1
    kept = np.zeros(len(data_pcd), bool)
    kept[order[mask]] = True
    data_down = data_pcd[kept]                                                    # input order (the script keeps the shuffled order)

    BB = BB.astype(np.float32)
    inbound = ((data_down >= BB[:1] - patch) & (data_down < BB[1:] + patch * 2)).sum(axis=-1) == 3
    data_in = data_down[inbound]
    data_grid = np.around((data_in - BB[:1]) / Res).astype(np.int32)
    grid_inbound = ((data_grid >= 0) & (data_grid < np.expand_dims(ObsMask.shape, 0))).sum(axis=-1) == 3
    data_grid_in = data_grid[grid_inbound]
    in_obs = ObsMask[data_grid_in[:, 0], data_grid_in[:, 1], data_grid_in[:, 2]].astype(np.bool_)
    data_in_obs = data_in[grid_inbound][in_obs]
    obs = np.zeros(len(data_down), bool)
    obs[np.nonzero(inbound)[0][np.nonzero(grid_inbound)[0][in_obs]]] = True

    stl_hom = np.concatenate([stl, np.ones_like(stl[:, :1])], -1)
    above = (ground_plane.reshape((1, 4)) * stl_hom).sum(-1) > 0
    stl_above = stl[above]

    nn_engine.fit(stl)
    dist_d2s, _ = nn_engine.kneighbors(data_in_obs, n_neighbors=1, return_distance=True)
    mean_d2s = dist_d2s[dist_d2s < max_dist].mean()
    nn_engine.fit(data_in)
    dist_s2d, _ = nn_engine.kneighbors(stl_above, n_neighbors=1, return_distance=True)
    mean_s2d = dist_s2d[dist_s2d < max_dist].mean()
    d2s, s2d = dist_d2s[:, 0], dist_s2d[:, 0]
    return {'samples': data_pcd, 'kept': kept, 'in': inbound, 'obs': obs, 'above': above,
            'dist_d2s': np.where(d2s < max_dist, d2s, np.inf), 'dist_s2d': np.where(s2d < max_dist, s2d, np.inf),
            'mean_d2s': mean_d2s, 'mean_s2d': mean_s2d, 'overall': (mean_d2s + mean_s2d) / 2}


def sphere_mesh(n, r, scale, shift):
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float32)] * 3, indexing='ij'))
    vol = (np.sqrt(((g - (n - 1) / 2) ** 2).sum(0)) - r + 0.3 * np.sin(g[0] * 0.9) * np.cos(g[1] * 0.7)).astype(np.float32)
    v, f, _ = mc_ref.marching_cubes(vol, spacing=(scale,) * 3, origin=shift)
    return v.astype(np.float32), f.astype(np.int32)


def sphere_points(rs, m, center, r):
    d = rs.randn(m, 3)
    return center + r * d / np.linalg.norm(d, axis=1, keepdims=True)


def fixture_mesh(rs):
    v, f = sphere_mesh(12, 4.0, 0.7, (-4.0, -4.0, -4.0))
    # hand-made faces: zero area (a repeated corner, collinear corners), a sliver with n1 = 0, and one big face
    extra = np.array([[6, 6, 6], [6.5, 6, 6], [7, 6, 6], [6, 6.2, 6.05], [6, 8, 6], [9, 6, 6], [6, 9, 6], [6.01, 6.02, 9.5]], np.float32)
    base = len(v)
    ef = np.array([[0, 0, 1], [0, 1, 2], [0, 3, 1], [0, 5, 6], [0, 6, 7], [3, 4, 5]], np.int32) + base
    v = np.concatenate([v, extra])
    f = np.concatenate([f, ef])
    stl = sphere_points(rs, 3000, np.zeros(3), 3.1)
    stl = np.concatenate([stl, rs.uniform(-2, 2, (40, 3)) * [1, 1, 0] + [0, 0, -1.0]])   # some stl points exactly on the plane z = -1
    obs = rs.rand(14, 14, 14) < 0.8
    bb = np.array([[-3.5, -3.5, -3.5], [3.5, 3.5, 3.5]], np.float64)
    return dict(verts=v, faces=f, stl=stl, obs_mask=obs, bb=bb, res=0.5, plane=np.array([0.0, 0.0, 1.0, 1.0]), density=0.2, patch=1, max_dist=0.6, seed=0)


def fixture_pcd(rs, seed):
    # a lattice of quarter steps (exact .5 grid offsets at res 0.5), exact-radius pairs (0.25 apart at density 0.25), duplicates, far points
    g = np.stack(np.meshgrid(np.arange(-12, 13), np.arange(-12, 13), np.arange(-2, 3), indexing='ij'), -1).reshape(-1, 3) * 0.25
    pts = g[rs.rand(len(g)) < 0.7].astype(np.float64)
    pts = np.concatenate([pts, pts[:50], rs.uniform(-3, 3, (400, 3)), [[40.0, 0, 0], [-30.0, 5, 5]]])
    stl = np.concatenate([rs.uniform(-3.2, 3.2, (1500, 3)) * [1, 1, 0.3], np.stack(np.meshgrid(np.arange(-4, 5) * 0.5, np.arange(-4, 5) * 0.5,
                                                                                                  [0.5], indexing='ij'), -1).reshape(-1, 3)])
    obs = rs.rand(16, 16, 16) < 0.7
    bb = np.array([[-2.0, -2.0, -2.0], [2.0, 2.0, 2.0]], np.float64)
    return dict(points=pts, stl=stl, obs_mask=obs, bb=bb, res=0.5, plane=np.array([0.0, 0.0, 2.0, -1.0]), density=0.25, patch=1, max_dist=1.0,
                seed=seed)


def main():
    rs = np.random.RandomState(0)
    cases = {'mesh': fixture_mesh(rs), 'pcd_seed0': fixture_pcd(np.random.RandomState(1), 0), 'pcd_seed7': fixture_pcd(np.random.RandomState(1), 7)}
    for name, c in cases.items():
        if 'verts' in c:
            data = script_sample(c['verts'].astype(np.float64), c['faces'].astype(np.int64), c['density'])
        else:
            data = c['points']
        r = script_eval(data, c['stl'], c['obs_mask'], c['bb'], c['res'], c['plane'], c['density'], c['patch'], c['max_dist'], c['seed'])
        out = dict(c)
        out.update(r)
        np.savez_compressed(os.path.join(HERE, name + '.npz'), **out)
        print('%s: %d points, %d kept, %d in, %d obs, %d stl above; d2s %.6f s2d %.6f' % (name, len(data), r['kept'].sum(), r['in'].sum(), r['obs'].sum(),
                                                                                    r['above'].sum(), r['mean_d2s'], r['mean_s2d']))


if __name__ == '__main__':
    main()
