"""The stereo scene (tests/stereo_scene.py: cameras side by side in front of a sphere cap) as a source of keypoints with known truth: the true
3-D point of any pixel position in closed form (ray - sphere), and synthetic keypoints -- surface points projected into every view with pixel
noise, each with a 128-d int8 code that is the point's own code plus per-view noise, mixed with clutter keypoints that belong to no point."""
import numpy as np

from stereo_scene import CENTER, RADIUS, make_cams, render                                  # noqa: F401  (re-exported for the tests)

HW, FOCAL, VIEWS = (128, 192), 300.0, 4


def true_points(cam, xy):
    """cam [2,4,4], pixel positions xy [n,2] (centre convention: pixel (x, y) is at x + 0.5, y + 0.5) -> the sphere points they see, [n,3]"""
    E, Km = cam[0], cam[1, :3, :3]
    o = -E[:3, :3].T @ E[:3, 3] - CENTER
    d = np.stack([(xy[:, 0] - Km[0, 2]) / Km[0, 0], (xy[:, 1] - Km[1, 2]) / Km[1, 1], np.ones(len(xy))], -1) @ E[:3, :3]
    a, b, c = (d * d).sum(-1), 2 * (d @ o), (o * o).sum() - RADIUS ** 2
    t = (-b - np.sqrt(b * b - 4 * a * c)) / (2 * a)
    return o + CENTER + d * t[:, None]


def project(cam, pts):
    """-> (xy [n,2], depth [n])"""
    q = pts @ cam[0, :3, :3].T + cam[0, :3, 3]
    p = q @ cam[1, :3, :3].T
    return p[:, :2] / p[:, 2:3], q[:, 2]


def synthetic_keypoints(n_points=120, n_clutter=60, pixel_noise=0.3, code_noise=24, seed=0, views=VIEWS, hw=HW, focal=FOCAL):
    """-> (cams [V,2,4,4], xy fp64 [N,2], codes int8 [N,128], view_off int64 [V+1], point int64 [N]: the surface point behind a keypoint or -1,
    points [n_points,3]).  Keypoints of a view are shuffled."""
    rs = np.random.RandomState(seed)
    cams, _ = make_cams(views, hw, focal)
    h, w = hw
    seeds = np.stack([rs.uniform(8, w - 8, n_points), rs.uniform(8, h - 8, n_points)], 1)
    pts = true_points(cams[views // 2], seeds)
    base = rs.randint(0, 128, size=(n_points, 128))
    xy, codes, point, view_off = [], [], [], [0]
    for v in range(views):
        p, z = project(cams[v], pts)
        p = p + rs.normal(scale=pixel_noise, size=p.shape)
        inside = (z > 0) & (p[:, 0] > 1) & (p[:, 0] < w - 1) & (p[:, 1] > 1) & (p[:, 1] < h - 1)
        ids = np.nonzero(inside)[0]
        c = np.clip(base[ids] + rs.randint(-code_noise, code_noise + 1, size=(len(ids), 128)), 0, 127)
        cx = np.stack([rs.uniform(1, w - 1, n_clutter), rs.uniform(1, h - 1, n_clutter)], 1)
        cc = rs.randint(0, 128, size=(n_clutter, 128))
        rep = rs.randint(0, n_points, size=n_clutter // 2)        # half of the clutter repeats a point's code somewhere else (repeated structure)
        cc[:len(rep)] = np.clip(base[rep] + rs.randint(-code_noise, code_noise + 1, size=(len(rep), 128)), 0, 127)
        order = rs.permutation(len(ids) + n_clutter)
        xy.append(np.concatenate([p[ids], cx])[order])
        codes.append(np.concatenate([c, cc])[order])
        point.append(np.concatenate([ids, np.full(n_clutter, -1)])[order])
        view_off.append(view_off[-1] + len(order))
    return cams, np.concatenate(xy), np.concatenate(codes).astype(np.int8), np.asarray(view_off, np.int64), np.concatenate(point), pts


def track_case():
    """three views of four keypoints -> (view_off, matches (pair, off, idx, dist), the expected tracks): a chain a-b, b-c (one track of three); a
    component with two keypoints of view 0 (dropped); a pair; a keypoint nobody matches"""
    view_off = np.array([0, 4, 8, 12], np.int64)
    pair = np.array([[0, 1], [0, 2], [1, 2]], np.int32)
    off = np.array([0, 2, 3, 6], np.int64)
    idx = np.array([[0, 0], [1, 1], [2, 1], [0, 0], [1, 1], [3, 3]], np.int32)
    expected = (np.array([0, 3, 5], np.int64), np.array([0, 1, 2, 1, 2], np.int32), np.array([0, 0, 0, 3, 3], np.int32))
    return view_off, (pair, off, idx, np.zeros(len(idx), np.int32)), expected


def axis_cameras():
    """five cameras whose arithmetic is exact (focal 256, principal point (64, 64), axis-aligned rotations), all with the point (0, 0, 4) at pixel
    (64, 64) but the last two: A at the origin looking along +z; B at (4, 0, 4) looking along -x; C at (0, 4, 4) looking along -y; D at the origin
    looking along -z (the point lies behind it); E = A moved by 1/64 along x (the point at pixel (63, 64), 0.22 degrees from A's ray)"""
    Km = np.array([[256.0, 0, 64], [0, 256, 64], [0, 0, 1]])
    R = [np.eye(3), np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]]), np.array([[1.0, 0, 0], [0, 0, 1], [0, -1, 0]]), np.diag([-1.0, 1, -1]), np.eye(3)]
    c = [np.zeros(3), np.array([4.0, 0, 4]), np.array([0.0, 4, 4]), np.zeros(3), np.array([1 / 64.0, 0, 0])]
    cams = np.zeros((5, 2, 4, 4))
    for v in range(5):
        cams[v, 0] = np.eye(4)
        cams[v, 0, :3, :3] = R[v]
        cams[v, 0, :3, 3] = -R[v] @ c[v]
        cams[v, 1, :3, :3] = Km
        cams[v, 1, 3, 3] = 1.0
    return cams


def triangulation_case():
    """-> (cams, xy [N,2], view_off, tracks, max_reproj, the expected (xyz, keep, obs_keep) at min_angle 1.5).  One keypoint list per camera of
    axis_cameras; tracks: exact pair A B; exact triple A B C; B with D (behind D: one observation left, rejected); A B D (D dropped, refit,
    kept); A E B and C's pixel moved by 10 (outvoted: dropped by the one refit; E's ray is not exact, so this xyz is exact to rounding only);
    A with E (angle too small)"""
    cams = axis_cameras()
    xy = np.array([[64.0, 64.0],                     # view 0 (A)
                   [64.0, 64.0],                     # view 1 (B)
                   [64.0, 64.0], [74.0, 64.0],       # view 2 (C): exact, moved
                   [64.0, 64.0],                     # view 3 (D)
                   [63.0, 64.0]])                    # view 4 (E)
    view_off = np.array([0, 1, 2, 4, 5, 6], np.int64)
    tv = [[0, 1], [0, 1, 2], [1, 3], [0, 1, 3], [0, 4, 1, 2], [0, 4]]
    tk = [[0, 0], [0, 0, 0], [0, 0], [0, 0, 0], [0, 0, 0, 1], [0, 0]]
    track_off = np.concatenate([[0], np.cumsum([len(t) for t in tv])]).astype(np.int64)
    tracks = (track_off, np.concatenate(tv).astype(np.int32), np.concatenate(tk).astype(np.int32))
    P = [0.0, 0.0, 4.0]
    xyz = np.array([P, P, [0.0, 0, 0], P, P, [0.0, 0, 0]])
    keep = np.array([1, 1, 0, 1, 1, 0], bool)
    obs_keep = np.array([1, 1, 1, 1, 1, 0, 0, 1, 1, 0, 1, 1, 1, 0, 0, 0], bool)
    return cams, xy, view_off, tracks, 4.0, (xyz, keep, obs_keep)
