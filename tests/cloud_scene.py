"""Scenes for the cloud-cleaning tests.

two_spheres: depth maps of a main sphere and a small one well outside it, rendered analytically (ray / sphere intersection per pixel centre) for
the cameras of mvs_scene.make_views.  Every view sees the small sphere, so it is geometrically consistent and fusion keeps it: the floater the cut
exists for.  injected: the single-sphere fused cloud with uniform outliers and a dense far blob added."""
import os

import numpy as np
from PIL import Image

import mvs_scene as S
from mvsdf_amd.utils import io as sio

MAIN = (S.CENTER, 0.25)                                                    # centre, radius (world units)
# beside the main sphere, across the mean viewing direction of six views (angle 0.4 + 0.3 * 2.5), 0.14 of free space between the two surfaces
FLOATER = (S.CENTER + 0.45 * np.array([-np.sin(1.15), np.cos(1.15), 0.0]), 0.06)


def render(cams, spheres):
    """camera-z depth of the nearest sphere per pixel centre (x + 0.5, y + 0.5), 0 where the ray misses all -> fp32 [V,H,W]"""
    cams = np.asarray(cams, np.float64)
    h, w = int(round(2 * cams[0, 1, 1, 2])), int(round(2 * cams[0, 1, 0, 2]))
    xs, ys = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    out = np.zeros((len(cams), h, w), np.float32)
    for v, cam in enumerate(cams):
        E, K = cam[0], cam[1, :3, :3]
        Rm, t = E[:3, :3], E[:3, 3]
        d = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs)], -1) @ Rm      # world directions with camera z = 1
        best = np.full((h, w), np.inf)
        for centre, radius in spheres:
            o = -Rm.T @ t - np.asarray(centre, np.float64)
            a, b, c = (d * d).sum(-1), 2 * (d @ o), (o * o).sum() - radius * radius
            disc = b * b - 4 * a * c
            hit = disc > 0
            tz = np.where(hit, (-b - np.sqrt(np.where(hit, disc, 0.0))) / (2 * a), np.inf)
            best = np.where(hit & (tz > 0) & (tz < best), tz, best)
        out[v] = np.where(np.isfinite(best), best, 0.0)
    return out


def two_spheres(n_views=6, depth_hw=(60, 80), img_wh=None):
    """-> (cams fp64 [V,2,4,4], depths fp32 [V,H,W], pairs)"""
    cams, _, pairs = S.make_views(n_views, depth_hw, clean=True, img_wh=img_wh)
    return cams, render(cams, [MAIN, FLOATER]), pairs


def near_floater(points, slack=1.05):
    """bool [N]: the points on the small sphere"""
    c, r = FLOATER
    return np.linalg.norm(np.asarray(points, np.float64) - c, axis=1) <= r * slack


def write_two_spheres(root, n_views=6, depth_hw=(48, 64), img_wh=(128, 96)):
    """the directory layout of mvs_scene.write_mvs_scene with the two-sphere depth maps and probabilities that pass every threshold -> (root, ids)"""
    root = str(root)
    os.makedirs(root, exist_ok=True)
    cams, depths, pairs = two_spheres(n_views, depth_hw, img_wh)
    images = S.make_images(n_views, img_wh)
    prob = np.full(depth_hw, 0.95, np.float32)
    ids = [str(3 * i + 4) for i in range(n_views)]
    for i, vid in enumerate(ids):
        z = vid.zfill(8)
        S.write_cam(os.path.join(root, 'cam_%s_flow3.txt' % z), cams[i])
        sio.write_pfm(os.path.join(root, '%s_flow3.pfm' % z), depths[i])
        for j in range(3):
            sio.write_pfm(os.path.join(root, '%s_flow%d_prob.pfm' % (z, j + 1)), prob)
        Image.fromarray(images[i]).save(os.path.join(root, '%s.jpg' % z), quality=95)
    with open(os.path.join(root, 'pair.txt'), 'w') as f:
        f.write('%d\n' % n_views)
        for i in range(n_views):
            f.write('%s\n%d %s\n' % (ids[i], len(pairs[i]), ' '.join('%s %.1f' % (ids[j], 100.0 - k) for k, j in enumerate(pairs[i]))))
    return root, ids


def injected(hole_frac=None):
    """the issue's scene -> (points fp64 [N,3] shuffled, is_injected bool [N]): the fused points of make_views(6, (60, 80), clean=True), plus 300
    points uniform within +-3 extents of the box centre, plus a 400-point Gaussian blob (sigma = 0.01 extent) at (2.5, 0.5, -1) extents from the
    centre, shuffled with RandomState(3); extent = the largest side of the fused cloud's box"""
    import fusion_ref
    kw = {} if hole_frac is None else {'hole_frac': hole_frac}
    fused = fusion_ref.fuse(*S.make_views(6, (60, 80), clean=True, **kw))['points']
    lo, hi = fused.min(0), fused.max(0)
    centre, extent = (lo + hi) / 2, (hi - lo).max()
    rs = np.random.RandomState(3)
    uni = centre + rs.uniform(-3, 3, size=(300, 3)) * extent
    blob = centre + np.array([2.5, 0.5, -1.0]) * extent + rs.normal(size=(400, 3)) * 0.01 * extent
    pts = np.concatenate([fused, uni, blob])
    tag = np.arange(len(pts)) >= len(fused)
    order = rs.permutation(len(pts))
    return np.ascontiguousarray(pts[order]), tag[order]
