"""A Vis-MVSNet output directory from synth, the input of tools/fusion.py and tools/vismvsnet2mvsdf.py: per view cam_<id:08>_flow3.txt,
<id:08>_flow3.pfm, <id:08>_flow{1,2,3}_prob.pfm, <id:08>.jpg (larger than the depth map), and pair.txt.  View i has id 3 i + 4 (non-contiguous, as
tests/train_scene.py); its sources are the other views, nearest angle first.  make_views gives the same arrays without touching the disk."""
import os

import numpy as np
from PIL import Image

from mvsdf_amd.utils import io as sio
from mvsdf_amd.utils import synth

SIZE, CENTER = 2.0, np.array([0.1, -0.2, 0.05])


def make_views(n_views=6, depth_hw=(48, 64), seed=0, clean=False, hole_frac=None, img_wh=None):
    """-> (cams fp64 [V,2,4,4], depths fp32 [V,H,W], pairs): the issue's scene, cameras synth._camera(0.4 + 0.3 i, 2.5, 0.8, ...); clean: a
    sphere without bumps, per-view scale error or holes; hole_frac overrides the holes alone"""
    h, w = depth_hw
    img_wh = img_wh or (4 * w, 4 * h)
    cams = np.stack([synth._camera(0.4 + 0.3 * i, 2.5, 0.8, SIZE, CENTER, img_wh, 2.2 * img_wh[0], depth_hw)[2] for i in range(n_views)])
    kw = dict(bump=0.0, view_bias=0.0, hole_frac=0.0) if clean else {}
    if hole_frac is not None:
        kw['hole_frac'] = hole_frac
    depths = synth.make_depth_maps(cams[:, None], SIZE, CENTER, seed=seed, **kw)[:, 0, 0]
    pairs = [sorted((j for j in range(n_views) if j != i), key=lambda j: (abs(j - i), -j)) for i in range(n_views)]
    return cams, np.ascontiguousarray(depths), pairs


def exact_self_pair():
    """two identical cameras whose matrices and inverses are exact (powers of two) and a constant depth 2: every transform is the identity,
    so ex = ey = 0 and zr = d exactly"""
    cam = np.zeros((2, 4, 4))
    cam[0] = np.eye(4)
    cam[1, :3, :3] = [[64, 0, 16], [0, 64, 8], [0, 0, 1]]
    cam[1, 3, 3] = 1
    return np.stack([cam, cam]), np.full((2, 16, 32), 2.0, np.float32), [[1], [0]]


def make_probs(depths, seed=0, cut=1.0 / 3):
    """three probability maps per view, fp32 [V,3,H,W]: about `cut` of the pixels fail one of the thresholds (0.8, 0.7, 0.8)"""
    rs = np.random.RandomState(seed + 7000)
    V, H, W = depths.shape
    p = rs.uniform(0.85, 1.0, size=(V, 3, H, W))
    low = rs.uniform(size=(V, H, W)) < cut
    which = rs.randint(0, 3, size=(V, H, W))
    for j in range(3):
        sel = low & (which == j)
        p[:, j][sel] = rs.uniform(0.0, (0.8, 0.7, 0.8)[j], size=int(sel.sum()))
    return p.astype(np.float32)


def make_images(n_views, img_wh, seed=0):
    """smooth colour images uint8 [V,H,W,3] (they survive JPEG)"""
    rs = np.random.RandomState(seed + 8000)
    w, h = img_wh
    x, y = np.meshgrid(np.arange(w) / w, np.arange(h) / h)
    out = []
    for i in range(n_views):
        ph = rs.uniform(0, 6, size=3)
        out.append(np.stack([127.5 + 120 * np.sin(5 * x + 3 * y * (c + 1) + ph[c] + i) for c in range(3)], -1))
    return np.clip(np.rint(np.stack(out)), 0, 255).astype(np.uint8)


def write_cam(path, cam):
    txt = 'extrinsic\n' + '\n'.join(' '.join('%.17g' % v for v in r) for r in cam[0]) + '\n\nintrinsic\n'
    txt += '\n'.join(' '.join('%.17g' % v for v in r) for r in cam[1][:3, :3]) + '\n\n425.0 2.5 192 905.0\n'
    with open(path, 'w') as f:
        f.write(txt)


def write_mvs_scene(root, n_views=4, depth_hw=(20, 28), img_wh=(96, 72), seed=0, clean=True, ext='jpg'):
    """-> (root, ids): the directory described above"""
    root = str(root)
    os.makedirs(root, exist_ok=True)
    cams, depths, pairs = make_views(n_views, depth_hw, seed, clean=clean, img_wh=img_wh)
    probs = make_probs(depths, seed, cut=0.1)
    images = make_images(n_views, img_wh, seed)
    ids = [str(3 * i + 4) for i in range(n_views)]
    for i, vid in enumerate(ids):
        z = vid.zfill(8)
        write_cam(os.path.join(root, 'cam_%s_flow3.txt' % z), cams[i])
        sio.write_pfm(os.path.join(root, '%s_flow3.pfm' % z), depths[i])
        for j in range(3):
            sio.write_pfm(os.path.join(root, '%s_flow%d_prob.pfm' % (z, j + 1)), np.ascontiguousarray(probs[i, j]))
        Image.fromarray(images[i]).save(os.path.join(root, '%s.%s' % (z, ext)), **({'quality': 95} if ext == 'jpg' else {}))
    with open(os.path.join(root, 'pair.txt'), 'w') as f:
        f.write('%d\n' % n_views)
        for i in range(n_views):
            f.write('%s\n%d %s\n' % (ids[i], len(pairs[i]), ' '.join('%s %.1f' % (ids[j], 100.0 - k) for k, j in enumerate(pairs[i]))))
    return root, ids
