"""A synthetic multi-view stereo scene with known depth, the input of stereo.plane_sweep / estimate_scene: a band-limited random solid texture (a sum of
3-d sinusoids) on a smooth surface (the cap of a large sphere that fills every image), rendered by intersecting every pixel's ray with the sphere,
so the depth of every pixel is known in closed form.  The cameras sit side by side in front of the cap and look at its nearest point.  write_scene
writes <root>/images/<id:08>.png, cams/<id:08>_cam.txt and pair.txt (view i has id 3 i + 4, its sources are the other views, nearest first), the way
tests/mvs_scene.write_mvs_scene writes a Vis-MVSNet output directory."""
import os

import numpy as np
from PIL import Image

RADIUS, CENTER = 5.0, np.array([0.0, 0.0, 0.0])
TARGET = np.array([0.0, 0.0, -RADIUS])                  # the cap's nearest point
DISTANCE = 3.0                                           # of the camera plane from it
BASELINE = 0.6
DEPTH_MIN, DEPTH_MAX = 2.9, 4.25


def make_cams(n_views=5, hw=(64, 96), focal=150.0, n_depths=24):
    """-> cams fp64 [V,2,4,4] at hw, pairs.  Camera i sits at ((i - (V-1)/2) * BASELINE, 0.15 * that, -RADIUS - DISTANCE) and looks at TARGET; row 3 of
    cams[v,1] = DEPTH_MIN, interval, n_depths, DEPTH_MAX"""
    h, w = hw
    cams = np.zeros((n_views, 2, 4, 4))
    for i in range(n_views):
        b = (i - (n_views - 1) / 2.0) * BASELINE
        c = np.array([b, 0.15 * b, -RADIUS - DISTANCE])
        z = (TARGET - c) / np.linalg.norm(TARGET - c)
        x = np.cross(np.array([0.0, 1.0, 0.0]), z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        Rm = np.stack([x, y, z])                                                 # world -> camera
        cams[i, 0] = np.eye(4)
        cams[i, 0, :3, :3] = Rm
        cams[i, 0, :3, 3] = -Rm @ c
        cams[i, 1, :3, :3] = [[focal, 0, w / 2.0], [0, focal, h / 2.0], [0, 0, 1]]
        cams[i, 1, 3] = [DEPTH_MIN, (DEPTH_MAX - DEPTH_MIN) / max(n_depths - 1, 1), n_depths, DEPTH_MAX]
    pairs = [sorted((j for j in range(n_views) if j != i), key=lambda j: (abs(j - i), j)) for i in range(n_views)]
    return cams, pairs


def texture(points, seed=0, n_waves=48, lam=(0.12, 0.5)):
    """the solid texture at world points [...,3] -> [...,3] in [0, 1]: per colour channel a sum of n_waves sinusoids with wavelengths in lam"""
    rs = np.random.RandomState(seed + 9000)
    out = []
    for _ in range(3):
        dirs = rs.normal(size=(n_waves, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        k = dirs * (2 * np.pi / rs.uniform(lam[0], lam[1], size=(n_waves, 1)))
        ph = rs.uniform(0, 2 * np.pi, size=n_waves)
        out.append(np.sin(points @ k.T + ph).sum(-1) / np.sqrt(n_waves / 2.0))    # unit variance
    return np.clip(0.5 + 0.22 * np.stack(out, -1), 0.0, 1.0)


def render(cams, hw, seed=0):
    """-> (images uint8 [V,H,W,3], depths fp64 [V,H,W]: the camera-z depth of the sphere at every pixel centre; every ray hits the cap)"""
    h, w = hw
    xs, ys = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    images, depths = [], []
    for cam in np.asarray(cams, np.float64):
        E, K = cam[0], cam[1, :3, :3]
        o = -E[:3, :3].T @ E[:3, 3] - CENTER
        d = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs)], -1) @ E[:3, :3]     # world ray per unit camera z
        a, b, c = (d * d).sum(-1), 2 * (d @ o), (o * o).sum() - RADIUS ** 2
        disc = b * b - 4 * a * c
        assert (disc > 0).all(), 'a ray misses the sphere'
        t = (-b - np.sqrt(disc)) / (2 * a)
        pts = o + CENTER + d * t[..., None]
        images.append(np.clip(np.rint(255 * texture(pts, seed)), 0, 255).astype(np.uint8))
        depths.append(t)
    return np.stack(images), np.stack(depths)


def seen_by_a_source(cams, depths, pairs, num_src=2):
    """bool [V,H,W]: the true point of the pixel projects inside (0 <= u <= W-1, 0 <= v <= H-1, in front) at least one of its first num_src sources"""
    from fusion_ref import matrices
    P, Pinv = matrices(cams)
    V, H, W = depths.shape
    xs, ys = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    out = np.zeros((V, H, W), bool)
    for r in range(V):
        q = np.stack([xs * depths[r], ys * depths[r], depths[r], np.ones_like(xs)], -1)
        for s in pairs[r][:num_src]:
            p = q @ (P[s] @ Pinv[r]).T
            u, v = p[..., 0] / p[..., 2] - 0.5, p[..., 1] / p[..., 2] - 0.5
            out[r] |= (p[..., 2] > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
    return out


def write_cam(path, cam):
    txt = 'extrinsic\n' + '\n'.join(' '.join('%.17g' % v for v in r) for r in cam[0]) + '\n\nintrinsic\n'
    txt += '\n'.join(' '.join('%.17g' % v for v in r) for r in cam[1][:3, :3])
    txt += '\n\n%.17g %.17g %d %.17g\n' % (cam[1, 3, 0], cam[1, 3, 1], int(cam[1, 3, 2]), cam[1, 3, 3])
    with open(path, 'w') as f:
        f.write(txt)


def write_scene(root, n_views=5, img_hw=(128, 192), focal=300.0, n_depths=24, seed=0):
    """-> (root, ids, cams at image size, pairs): the input directory of estimate_scene"""
    root = str(root)
    for sub in ('images', 'cams'):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    cams, pairs = make_cams(n_views, img_hw, focal, n_depths)
    images, _ = render(cams, img_hw, seed)
    ids = [str(3 * i + 4) for i in range(n_views)]
    for i, vid in enumerate(ids):
        z = vid.zfill(8)
        write_cam(os.path.join(root, 'cams', '%s_cam.txt' % z), cams[i])
        Image.fromarray(images[i]).save(os.path.join(root, 'images', '%s.png' % z))
    with open(os.path.join(root, 'pair.txt'), 'w') as f:
        f.write('%d\n' % n_views)
        for i in range(n_views):
            f.write('%s\n%d %s\n' % (ids[i], len(pairs[i]), ' '.join('%s %.1f' % (ids[j], 100.0 - k) for k, j in enumerate(pairs[i]))))
    return root, ids, cams, pairs
