"""A synthetic COLMAP model for the view-selection tests: cameras on an arc around a cloud of random points, visibility decided by the frustum and a
distance cap, and writers for COLMAP's text and binary model formats (no COLMAP is installed where the tests run).  The model is the dict
mvsdf_amd.datasets.colmap.load_colmap_model returns, so a written model can be compared with what is read back.  Not a test module."""
import os
import struct

import numpy as np

from mvsdf_amd.datasets.colmap import MODEL_IDS

W, H, FOCAL = 64, 48, 60.0
RADIUS, SPACING_DEG, DIST_CAP = 4.0, 8.0, 4.7


def quaternion(R):
    """rotation matrix -> (qw, qx, qy, qz), qw > 0 (the scene's rotations are far from a half turn)"""
    qw = np.sqrt(1.0 + R[0, 0] + R[1, 1] + R[2, 2]) / 2
    return np.array([qw, (R[2, 1] - R[1, 2]) / (4 * qw), (R[0, 2] - R[2, 0]) / (4 * qw), (R[1, 0] - R[0, 1]) / (4 * qw)])


def arc_pose(phi):
    """a camera at RADIUS on the arc (angle phi about the y axis), looking at the origin -> (R, t) world -> camera"""
    C = RADIUS * np.array([np.sin(phi), 0.0, -np.cos(phi)])
    z = -C / np.linalg.norm(C)
    x = np.array([np.cos(phi), 0.0, np.sin(phi)])
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R, -R @ C


def make_scene(n_views=6, n_points=300, seed=0, model='PINHOLE', distortion=0.0, blind_image=False, double_observation=False):
    """-> the model dict.  Image ids are 3, 5, 7, ... (so the views are renumbered), names view_<id>.png.  blind_image: one more image that observes
    nothing (an empty POINTS2D line).  double_observation: the first point is observed twice by its first image."""
    rng = np.random.RandomState(seed)
    params = {'SIMPLE_PINHOLE': [FOCAL, W / 2, H / 2], 'PINHOLE': [FOCAL, FOCAL, W / 2, H / 2], 'SIMPLE_RADIAL': [FOCAL, W / 2, H / 2, distortion],
              'RADIAL': [FOCAL, W / 2, H / 2, distortion, 0.0], 'OPENCV': [FOCAL, FOCAL, W / 2, H / 2, distortion, 0.0, 0.0, 0.0]}[model]
    cameras = {1: {'model': model, 'width': W, 'height': H, 'params': np.array(params, dtype=np.float64)}}
    xyz = rng.uniform(-1, 1, (n_points, 3))
    images, seen = {}, []
    for k in range(n_views):
        R, t = arc_pose(np.radians(SPACING_DEG * (k - (n_views - 1) / 2)))
        pc = xyz @ R.T + t
        u, v = FOCAL * pc[:, 0] / pc[:, 2] + W / 2, FOCAL * pc[:, 1] / pc[:, 2] + H / 2
        vis = (pc[:, 2] > 0) & (u >= 0) & (u <= W) & (v >= 0) & (v <= H) & (np.linalg.norm(pc, axis=1) < DIST_CAP)
        idx = np.flatnonzero(vis)
        n_extra = 3                                                         # keypoints without a 3-d point, as COLMAP lists them
        xys = np.concatenate([np.stack([u[idx], v[idx]], 1), rng.uniform(0, H, (n_extra, 2))])
        pids = np.concatenate([idx + 1, -np.ones(n_extra, np.int64)]).astype(np.int64)            # point ids start at 1
        images[3 + 2 * k] = {'q': quaternion(R), 't': t, 'camera_id': 1, 'name': 'view_%d.png' % (3 + 2 * k), 'xys': xys, 'point3D_ids': pids}
        seen.append(vis)
    if blind_image:
        R, t = arc_pose(np.radians(170.0))
        images[2] = {'q': quaternion(R), 't': t, 'camera_id': 1, 'name': 'blind.png', 'xys': np.zeros((0, 2)), 'point3D_ids': np.zeros(0, np.int64)}
    seen = np.stack(seen)
    keep = np.flatnonzero(seen.sum(0) >= 1)
    off, timg, tidx = [0], [], []
    for p in keep:
        for k in np.flatnonzero(seen[:, p]):
            iid = 3 + 2 * k
            timg.append(iid)
            tidx.append(int(np.flatnonzero(images[iid]['point3D_ids'] == p + 1)[0]))
        if double_observation and len(off) == 1:
            timg.append(timg[0])
            tidx.append(len(images[timg[0]]['point3D_ids']) - 1)
        off.append(len(timg))
    points = {'ids': (keep + 1).astype(np.int64), 'xyz': xyz[keep], 'rgb': rng.randint(0, 256, (len(keep), 3)).astype(np.uint8),
              'error': rng.uniform(0, 1, len(keep)), 'track_off': np.array(off, np.int64), 'track_image': np.array(timg, np.int32),
              'track_point2D': np.array(tidx, np.int32)}
    return {'cameras': cameras, 'images': images, 'points': points}


def write_text(model, d):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, 'cameras.txt'), 'w') as f:
        f.write('# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n')
        for cid, c in model['cameras'].items():
            f.write('%d %s %d %d %s\n' % (cid, c['model'], c['width'], c['height'], ' '.join(repr(float(x)) for x in c['params'])))
    with open(os.path.join(d, 'images.txt'), 'w') as f:
        f.write('# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n#   POINTS2D[] as (X, Y, POINT3D_ID)\n')
        for iid, im in model['images'].items():
            f.write('%d %s %d %s\n' % (iid, ' '.join(repr(float(x)) for x in list(im['q']) + list(im['t'])), im['camera_id'], im['name']))
            f.write(' '.join('%r %r %d' % (float(x), float(y), p) for (x, y), p in zip(im['xys'], im['point3D_ids'])) + '\n')
    pts = model['points']
    with open(os.path.join(d, 'points3D.txt'), 'w') as f:
        f.write('# 3D point list with one line of data per point:\n#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n')
        for k, pid in enumerate(pts['ids']):
            a, b = pts['track_off'][k], pts['track_off'][k + 1]
            track = ' '.join('%d %d' % (i, j) for i, j in zip(pts['track_image'][a:b], pts['track_point2D'][a:b]))
            f.write('%d %s %d %d %d %r %s\n' % (pid, ' '.join(repr(float(x)) for x in pts['xyz'][k]), *pts['rgb'][k], float(pts['error'][k]), track))


def write_binary(model, d):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, 'cameras.bin'), 'wb') as f:
        f.write(struct.pack('<Q', len(model['cameras'])))
        for cid, c in model['cameras'].items():
            f.write(struct.pack('<iiQQ', cid, MODEL_IDS[c['model']], c['width'], c['height']))
            f.write(np.asarray(c['params'], '<f8').tobytes())
    with open(os.path.join(d, 'images.bin'), 'wb') as f:
        f.write(struct.pack('<Q', len(model['images'])))
        for iid, im in model['images'].items():
            f.write(struct.pack('<i4d3di', iid, *im['q'], *im['t'], im['camera_id']))
            f.write(im['name'].encode('utf-8') + b'\0')
            f.write(struct.pack('<Q', len(im['point3D_ids'])))
            for (x, y), p in zip(im['xys'], im['point3D_ids']):
                f.write(struct.pack('<ddq', x, y, p))
    pts = model['points']
    with open(os.path.join(d, 'points3D.bin'), 'wb') as f:
        f.write(struct.pack('<Q', len(pts['ids'])))
        for k, pid in enumerate(pts['ids']):
            a, b = pts['track_off'][k], pts['track_off'][k + 1]
            f.write(struct.pack('<Q3d3BdQ', pid, *pts['xyz'][k], *(int(c) for c in pts['rgb'][k]), pts['error'][k], b - a))
            for i, j in zip(pts['track_image'][a:b], pts['track_point2D'][a:b]):
                f.write(struct.pack('<ii', i, j))


def write_images(model, d, seed=0):
    """a small textured png per image of the model, under the names the model gives"""
    from PIL import Image
    os.makedirs(d, exist_ok=True)
    rng = np.random.RandomState(seed)
    for im in model['images'].values():
        coarse = rng.randint(0, 256, (H // 4, W // 4, 3)).astype(np.uint8)
        Image.fromarray(np.kron(coarse, np.ones((4, 4, 1), np.uint8))).save(os.path.join(d, im['name']))


def assert_models_equal(a, b):
    assert sorted(a['cameras']) == sorted(b['cameras']) and sorted(a['images']) == sorted(b['images'])
    for cid, c in a['cameras'].items():
        o = b['cameras'][cid]
        assert (c['model'], c['width'], c['height']) == (o['model'], o['width'], o['height']) and np.array_equal(c['params'], o['params'])
    for iid, im in a['images'].items():
        o = b['images'][iid]
        assert im['camera_id'] == o['camera_id'] and im['name'] == o['name']
        for k in ('q', 't', 'xys', 'point3D_ids'):
            assert np.asarray(im[k]).shape == np.asarray(o[k]).shape and np.array_equal(im[k], o[k]), (iid, k)
    for k in ('ids', 'xyz', 'rgb', 'error', 'track_off', 'track_image', 'track_point2D'):
        assert a['points'][k].shape == b['points'][k].shape and np.array_equal(a['points'][k], b['points'][k]), k


def scene_arrays(model):
    """-> (points [P,3], centres [V,3], extrinsics [V,4,4], vis bool [V,P]) of the model, the views by ascending image id, in plain numpy"""
    from mvsdf_amd.datasets.colmap import rotation
    ids = sorted(model['images'])
    E = np.stack([np.eye(4)] * len(ids))
    for i, iid in enumerate(ids):
        E[i, :3, :3] = rotation(model['images'][iid]['q'])
        E[i, :3, 3] = model['images'][iid]['t']
    centres = np.stack([-(e[:3, :3].T @ e[:3, 3]) for e in E])
    pts = model['points']
    vis = np.zeros((len(ids), len(pts['ids'])), bool)
    for p in range(len(pts['ids'])):
        for iid in pts['track_image'][pts['track_off'][p]:pts['track_off'][p + 1]]:
            vis[ids.index(int(iid)), p] = True
    return pts['xyz'], centres, E, vis
