"""Bundle-adjustment problems with known truth from tests/keypoints_scene.synthetic_keypoints (no clutter): the true cameras and points, the
observations as tracks, and perturbed cameras and points to start from."""
import collections

import numpy as np

from keypoints_scene import synthetic_keypoints, project

Scene = collections.namedtuple('Scene', 'cams_true xyz_true cams xyz off view obs')


def rotation(w):
    """the exact exponential map of w (numpy's sin / cos)"""
    t = np.linalg.norm(w)
    Kx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if t == 0:
        return np.eye(3)
    return np.eye(3) + np.sin(t) / t * Kx + (1 - np.cos(t)) / (t * t) * (Kx @ Kx)


def centres(cams):
    cams = np.asarray(cams)
    return np.stack([-c[0, :3, :3].T @ c[0, :3, 3] for c in cams])


def make_scene(views=4, n_points=120, noise=0.3, seed=0, fixed=(0, 1), angle=1.0, shift=0.15, jitter=0.03, skew=0.0, shuffle=False, min_views=2):
    """-> Scene.  Cameras outside `fixed` are rotated by about `angle` degrees and their centres moved by about `shift`; points move by `jitter`.
    noise = 0 sets every observation to the exact projection of the true point.  skew: K gets s = skew and fy = 1.1 fx.  shuffle: the view
    order inside every track is shuffled and tracks are cut to random lengths from min_views to V."""
    cams0, xy, _, view_off, point, pts = synthetic_keypoints(n_points, 0, noise, seed=seed, views=views)
    cams = cams0.copy()
    cams[:, 1, 3] = [0, 0, 0, 1]
    rs = np.random.RandomState(seed + 77)
    if skew:
        cams[:, 1, 0, 1] = skew
        cams[:, 1, 1, 1] = 1.1 * cams[:, 1, 0, 0]
    tv, ob = [[] for _ in range(n_points)], [[] for _ in range(n_points)]
    for v in range(views):
        exact, _ = project(cams[v], pts)                     # with the skewed K
        drawn, _ = project(cams0[v], pts)                    # what synthetic_keypoints added its pixel noise to
        for k in range(view_off[v], view_off[v + 1]):
            j = point[k]
            tv[j].append(v)
            ob[j].append(exact[j] + (xy[k] - drawn[j]) if noise else exact[j])
    keep = [j for j in range(n_points) if len(tv[j]) >= min_views]
    off, view, obs = [0], [], []
    for j in keep:
        order = np.arange(len(tv[j]))
        if shuffle:
            order = rs.permutation(len(tv[j]))[:rs.randint(min_views, len(tv[j]) + 1)]
        view += [tv[j][q] for q in order]
        obs += [ob[j][q] for q in order]
        off.append(len(view))
    xyz_true = pts[keep]
    start = cams.copy()
    for v in range(views):
        if v in fixed:
            continue
        w = rs.normal(size=3)
        R = rotation(w / np.linalg.norm(w) * np.radians(angle)) @ cams[v, 0, :3, :3]
        d = rs.normal(size=3)
        c = centres(cams[v:v + 1])[0] + d / np.linalg.norm(d) * shift
        start[v, 0, :3, :3] = R
        start[v, 0, :3, 3] = -R @ c
    xyz = xyz_true + rs.normal(scale=jitter, size=xyz_true.shape) if jitter else xyz_true.copy()
    return Scene(cams, xyz_true, start, np.ascontiguousarray(xyz), np.asarray(off, np.int64), np.asarray(view, np.int32),
                 np.ascontiguousarray(np.asarray(obs, np.float64).reshape(-1, 2)))


def cost_of(ref, cams, xyz, s, loss_scale=None):
    return ref.residuals(cams, xyz, s.off, s.view, s.obs, loss_scale, True)[2]
