"""COLMAP sparse models as MVS input: load_colmap_model reads a model directory (text, else binary; numpy only) and colmap_to_mvs writes what
stereo.estimate_scene, tools/fusion.py and tools/vismvsnet2mvsdf.py start from -- images/<i:08>.jpg|png, cams/<i:08>_cam.txt with depth ranges and
pair.txt -- with the view scores and depth ranges computed on the device (mvsdf_amd/viewsel.py).  A model that has poses but no (or unwanted)
points3D is served by colmap_to_mvs(..., triangulate=True): the points then come from the images themselves (mvsdf_amd/keypoints.py).

The file formats are COLMAP's documented ones.  Text: `#` lines are comments; cameras.txt `CAMERA_ID MODEL WIDTH HEIGHT PARAMS...`; images.txt two
lines per image, `IMAGE_ID QW QX QY QZ TX TY TZ CAMERA_ID NAME` and `X Y POINT3D_ID ...` (which may be empty); points3D.txt `POINT3D_ID X Y Z R G B
ERROR (IMAGE_ID POINT2D_IDX)...`.  Binary: little-endian, counts as uint64, the records in the same order (cameras carry a model id instead of the
name, image names end with a zero byte).  A pose maps world to camera: x_cam = R(qw, qx, qy, qz) x + t.

Cameras: SIMPLE_PINHOLE and PINHOLE are taken as they are; SIMPLE_RADIAL, RADIAL and OPENCV only if every distortion parameter is 0; anything else
raises ValueError (undistort the images first) unless undistortion is asked for: colmap_to_mvs(..., undistort=True), or tools/undistort.py
beforehand, resamples the images on the device to pinhole views (mvsdf_amd/undistort.py states what is computed) for SIMPLE_RADIAL, RADIAL, OPENCV,
FULL_OPENCV, OPENCV_FISHEYE, SIMPLE_RADIAL_FISHEYE and RADIAL_FISHEYE cameras.  load_colmap_model(dir, allow_distortion=True) loads such a model;
FOV, THIN_PRISM_FISHEYE and unknown models stay refused.  write_colmap_text writes a model back in the text format.  COLMAP puts the centre of pixel
(0, 0) at (0.5, 0.5), which is this project's X = x + 0.5 (fusion.py), so cx and cy are kept unchanged.
"""
import os
import shutil
import struct

import numpy as np

# model id -> (name, number of parameters), COLMAP's camera model table
MODELS = {0: ('SIMPLE_PINHOLE', 3), 1: ('PINHOLE', 4), 2: ('SIMPLE_RADIAL', 4), 3: ('RADIAL', 5), 4: ('OPENCV', 8), 5: ('OPENCV_FISHEYE', 8),
          6: ('FULL_OPENCV', 12), 7: ('FOV', 5), 8: ('SIMPLE_RADIAL_FISHEYE', 4), 9: ('RADIAL_FISHEYE', 5), 10: ('THIN_PRISM_FISHEYE', 12)}
MODEL_IDS = {name: i for i, (name, _) in MODELS.items()}
# accepted models: (indices of fx, fy, cx, cy in the parameters, first distortion parameter)
_PINHOLE_LIKE = {'SIMPLE_PINHOLE': ((0, 0, 1, 2), 3), 'PINHOLE': ((0, 1, 2, 3), 4), 'SIMPLE_RADIAL': ((0, 0, 1, 2), 3), 'RADIAL': ((0, 0, 1, 2), 3),
                 'OPENCV': ((0, 1, 2, 3), 4)}


def camera_intrinsics(camera):
    """A camera of the model -> K fp64 [3,3]; ValueError for a model with distortion"""
    name, params = camera['model'], np.asarray(camera['params'], dtype=np.float64)
    if name not in _PINHOLE_LIKE:
        raise ValueError('colmap: camera model %s is not supported (SIMPLE_PINHOLE, PINHOLE, or SIMPLE_RADIAL / RADIAL / OPENCV without distortion): '
                         'undistort the images first' % name)
    (ifx, ify, icx, icy), first = _PINHOLE_LIKE[name]
    if len(params) != MODELS[MODEL_IDS[name]][1]:
        raise ValueError('colmap: camera model %s takes %d parameters, got %d' % (name, MODELS[MODEL_IDS[name]][1], len(params)))
    if np.any(params[first:] != 0):
        raise ValueError('colmap: the %s camera has non-zero distortion parameters %s: undistort the images first' % (name, params[first:].tolist()))
    return np.array([[params[ifx], 0, params[icx]], [0, params[ify], params[icy]], [0, 0, 1]], dtype=np.float64)


def rotation(q):
    """(qw, qx, qy, qz), normalised here -> R fp64 [3,3]"""
    q = np.asarray(q, dtype=np.float64)
    w, x, y, z = q / np.sqrt((q * q).sum())
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _data_lines(path):
    with open(path) as f:
        return [ln.rstrip('\r\n') for ln in f if not ln.lstrip().startswith('#')]


def _read_text(d):
    cameras, images = {}, {}
    for ln in _data_lines(os.path.join(d, 'cameras.txt')):
        w = ln.split()
        if not w:
            continue
        if w[1] not in MODEL_IDS:
            raise ValueError('colmap: unknown camera model %s in cameras.txt: undistort the images to a pinhole model first' % w[1])
        cameras[int(w[0])] = {'model': w[1], 'width': int(w[2]), 'height': int(w[3]), 'params': np.array([float(x) for x in w[4:]], dtype=np.float64)}
    lines = _data_lines(os.path.join(d, 'images.txt'))
    k = 0
    while k < len(lines):
        w = lines[k].split()
        if not w:                                                           # blank lines between records (not the empty POINTS2D line, taken below)
            k += 1
            continue
        if len(w) < 10:
            raise ValueError('colmap: images.txt: expected IMAGE_ID QW QX QY QZ TX TY TZ CAMERA_ID NAME, got %r' % lines[k])
        p = lines[k + 1].split() if k + 1 < len(lines) else []
        if len(p) % 3:
            raise ValueError('colmap: images.txt: the POINTS2D line of image %s does not hold triples' % w[0])
        images[int(w[0])] = {'q': np.array([float(x) for x in w[1:5]]), 't': np.array([float(x) for x in w[5:8]]), 'camera_id': int(w[8]),
                             'name': ' '.join(w[9:]), 'xys': np.array([float(x) for x in p], dtype=np.float64).reshape(-1, 3)[:, :2].copy(),
                             'point3D_ids': np.array([int(x) for x in p[2::3]], dtype=np.int64)}
        k += 2
    ids, xyz, rgb, err, off, timg, tidx = [], [], [], [], [0], [], []
    for ln in _data_lines(os.path.join(d, 'points3D.txt')):
        w = ln.split()
        if not w:
            continue
        if len(w) < 8 or len(w) % 2:
            raise ValueError('colmap: points3D.txt: expected POINT3D_ID X Y Z R G B ERROR and (IMAGE_ID POINT2D_IDX) pairs, got %r' % ln)
        ids.append(int(w[0]))
        xyz.append([float(x) for x in w[1:4]])
        rgb.append([int(x) for x in w[4:7]])
        err.append(float(w[7]))
        timg += [int(x) for x in w[8::2]]
        tidx += [int(x) for x in w[9::2]]
        off.append(len(timg))
    return cameras, images, _points(ids, xyz, rgb, err, off, timg, tidx)


def _points(ids, xyz, rgb, err, off, timg, tidx):
    return {'ids': np.array(ids, dtype=np.int64), 'xyz': np.array(xyz, dtype=np.float64).reshape(-1, 3), 'rgb': np.array(rgb, dtype=np.uint8).reshape(-1, 3),
            'error': np.array(err, dtype=np.float64), 'track_off': np.array(off, dtype=np.int64), 'track_image': np.array(timg, dtype=np.int32),
            'track_point2D': np.array(tidx, dtype=np.int32)}


class _Reader:
    def __init__(self, path):
        with open(path, 'rb') as f:
            self.b, self.at, self.path = f.read(), 0, path

    def take(self, fmt):
        size = struct.calcsize('<' + fmt)
        if self.at + size > len(self.b):
            raise ValueError('colmap: %s ends in the middle of a record' % self.path)
        out = struct.unpack_from('<' + fmt, self.b, self.at)
        self.at += size
        return out

    def array(self, dtype, n):
        dt = np.dtype(dtype)
        if self.at + dt.itemsize * n > len(self.b):
            raise ValueError('colmap: %s ends in the middle of a record' % self.path)
        out = np.frombuffer(self.b, dt, n, self.at).copy()
        self.at += dt.itemsize * n
        return out

    def name(self):
        end = self.b.index(b'\0', self.at)
        s = self.b[self.at:end].decode('utf-8')
        self.at = end + 1
        return s


def _read_binary(d):
    cameras, images = {}, {}
    r = _Reader(os.path.join(d, 'cameras.bin'))
    for _ in range(r.take('Q')[0]):
        cid, mid, w, h = r.take('iiQQ')
        if mid not in MODELS:
            raise ValueError('colmap: unknown camera model id %d in cameras.bin: undistort the images to a pinhole model first' % mid)
        cameras[cid] = {'model': MODELS[mid][0], 'width': w, 'height': h, 'params': r.array('<f8', MODELS[mid][1])}
    r = _Reader(os.path.join(d, 'images.bin'))
    for _ in range(r.take('Q')[0]):
        iid = r.take('i')[0]
        q, t = r.array('<f8', 4), r.array('<f8', 3)
        cid, name = r.take('i')[0], r.name()
        obs = r.array(np.dtype([('xy', '<f8', 2), ('id', '<i8')]), r.take('Q')[0])
        images[iid] = {'q': q, 't': t, 'camera_id': cid, 'name': name, 'xys': obs['xy'].astype(np.float64).reshape(-1, 2),
                       'point3D_ids': obs['id'].astype(np.int64)}
    r = _Reader(os.path.join(d, 'points3D.bin'))
    ids, xyz, rgb, err, off, timg, tidx = [], [], [], [], [0], [], []
    for _ in range(r.take('Q')[0]):
        ids.append(r.take('Q')[0])
        xyz.append(r.array('<f8', 3))
        rgb.append(r.array('u1', 3))
        err.append(r.take('d')[0])
        tr = r.array('<i4', 2 * r.take('Q')[0]).reshape(-1, 2)
        timg += tr[:, 0].tolist()
        tidx += tr[:, 1].tolist()
        off.append(len(timg))
    return cameras, images, _points(ids, xyz, rgb, err, off, timg, tidx)


def load_colmap_model(model_dir, allow_distortion=False):
    """-> {'cameras': {id: {'model', 'width', 'height', 'params' fp64}}, 'images': {id: {'q' (qw qx qy qz), 't', 'camera_id', 'name', 'xys' fp64 [n,2],
    'point3D_ids' int64 [n]}}, 'points': {'ids' int64 [N], 'xyz' fp64 [N,3], 'rgb' uint8 [N,3], 'error' fp64 [N], 'track_off' int64 [N+1],
    'track_image' int32, 'track_point2D' int32 (the tracks in CSR form, by COLMAP image id)}}.  Reads cameras.txt / images.txt / points3D.txt where
    all three exist, else the .bin files.  Every camera must be one colmap_to_mvs can use (camera_intrinsics) or, with allow_distortion, one
    mvsdf_amd/undistort.py can turn into such a camera (undistort.camera_block)."""
    names = ('cameras', 'images', 'points3D')
    if all(os.path.exists(os.path.join(model_dir, n + '.txt')) for n in names):
        cameras, images, points = _read_text(model_dir)
    elif all(os.path.exists(os.path.join(model_dir, n + '.bin')) for n in names):
        cameras, images, points = _read_binary(model_dir)
    else:
        raise FileNotFoundError('colmap: %s holds neither cameras / images / points3D .txt nor .bin' % model_dir)
    for cam in cameras.values():
        if allow_distortion:
            from ..undistort import camera_block
            camera_block(cam)
        else:
            camera_intrinsics(cam)
    for iid, im in images.items():
        if im['camera_id'] not in cameras:
            raise ValueError('colmap: image %d refers to camera %d, which the model does not hold' % (iid, im['camera_id']))
    return {'cameras': cameras, 'images': images, 'points': points}


def write_colmap_text(model, model_dir):
    """A model (the dict load_colmap_model returns) -> model_dir/cameras.txt, images.txt and points3D.txt in COLMAP's text format; every float is
    written with repr, so load_colmap_model reads back the same bits"""
    os.makedirs(model_dir, exist_ok=True)

    def floats(xs):
        return ' '.join(repr(float(x)) for x in xs)
    with open(os.path.join(model_dir, 'cameras.txt'), 'w') as f:
        f.write('# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n# Number of cameras: %d\n' % len(model['cameras']))
        for cid, c in model['cameras'].items():
            f.write('%d %s %d %d %s\n' % (cid, c['model'], c['width'], c['height'], floats(c['params'])))
    with open(os.path.join(model_dir, 'images.txt'), 'w') as f:
        f.write('# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n#   POINTS2D[] as (X, Y, POINT3D_ID)\n'
                '# Number of images: %d\n' % len(model['images']))
        for iid, im in model['images'].items():
            f.write('%d %s %d %s\n' % (iid, floats(list(im['q']) + list(im['t'])), im['camera_id'], im['name']))
            f.write(' '.join('%r %r %d' % (float(x), float(y), p) for (x, y), p in zip(im['xys'], im['point3D_ids'])) + '\n')
    pts = model['points']
    with open(os.path.join(model_dir, 'points3D.txt'), 'w') as f:
        f.write('# 3D point list with one line of data per point:\n#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n'
                '# Number of points: %d\n' % len(pts['ids']))
        for k, pid in enumerate(pts['ids']):
            a, b = pts['track_off'][k], pts['track_off'][k + 1]
            track = ' '.join('%d %d' % (i, j) for i, j in zip(pts['track_image'][a:b], pts['track_point2D'][a:b]))
            f.write(('%d %s %d %d %d %r %s' % (pid, floats(pts['xyz'][k]), pts['rgb'][k][0], pts['rgb'][k][1], pts['rgb'][k][2], float(pts['error'][k]), track)).rstrip() + '\n')


def model_views(model):
    """The views of a model, the images sorted by COLMAP image id and renumbered from 0 -> (image ids, names, cams fp64 [V,2,4,4] with the extrinsic
    [R t; 0 0 0 1] and K (depth words still 0), track_view int32: the model's track_image as view indices)"""
    ids = sorted(model['images'])
    cams = np.zeros((len(ids), 2, 4, 4))
    for i, iid in enumerate(ids):
        im = model['images'][iid]
        cams[i, 0] = np.eye(4)
        cams[i, 0, :3, :3] = rotation(im['q'])
        cams[i, 0, :3, 3] = im['t']
        cams[i, 1, :3, :3] = camera_intrinsics(model['cameras'][im['camera_id']])
    timg = model['points']['track_image']
    lut = np.asarray(ids, dtype=np.int64)
    view = np.searchsorted(lut, timg).astype(np.int32) if len(ids) else np.zeros(len(timg), np.int32)
    if len(timg) and (not len(ids) or (view >= len(ids)).any() or (lut[np.minimum(view, len(ids) - 1)] != timg).any()):
        raise ValueError('colmap: a track of points3D refers to an image the model does not hold')
    return ids, [model['images'][i]['name'] for i in ids], cams, view


def colmap_to_mvs(model_dir, image_dir, out_root, max_d=256, interval_scale=1, num_pairs=10, theta0=5, sigma1=1, sigma2=10, undistort=False,
                  blank_pixels=0.0, min_scale=0.2, max_scale=2.0, triangulate=False):
    """A COLMAP model and its (undistorted) images -> out_root/images/<i:08>.jpg|png (jpg and png copied as they are, other formats re-encoded as png),
    out_root/cams/<i:08>_cam.txt (extrinsic, intrinsic, `depth_min interval max_d depth_max` with interval = (depth_max - depth_min) / (max_d - 1) /
    interval_scale, from viewsel.depth_ranges) and out_root/pair.txt (viewsel.view_scores + select_pairs over the model's tracks).  max_d = 0, the
    automatic hypothesis count of MVSNet's script, is not built.  undistort=True takes a model with distorted cameras (load_colmap_model's
    allow_distortion): every image is resampled on the device to its camera's pinhole view (undistort.undistorted_camera with blank_pixels, min_scale,
    max_scale) and written as png, and the camera files carry that view's intrinsics; pairs and depth ranges use points, centres and extrinsics only
    and are what they are without it.  triangulate=True replaces the model's points (which may be empty) by keypoints.sparse_model's: keypoints,
    matches and triangulated tracks from the images themselves (pinhole images only: undistort first).  -> {'ids', 'names', 'cams' [V,2,4,4], 'pairs', 'pair_scores', 'scores', 'counts'}."""
    from .. import viewsel
    from ..stereo import _write_cam
    what = 'colmap_to_mvs'
    max_d = int(max_d)
    if max_d < 2:
        raise ValueError('%s: max_d must be >= 2 (max_d = 0, the automatic hypothesis count, is not built), got %d' % (what, max_d))
    if not float(interval_scale) > 0:
        raise ValueError('%s: interval_scale must be > 0' % what)
    if triangulate and undistort:
        raise ValueError('%s: triangulate needs pinhole images: run tools/undistort.py first, then triangulate its output' % what)
    model = load_colmap_model(model_dir, allow_distortion=bool(undistort))
    if triangulate:
        from ..keypoints import sparse_model
        model = sparse_model(model, image_dir)
    if undistort:
        from .. import undistort as und
        source_cameras = model['cameras']
        model = dict(model, cameras={cid: und.undistorted_camera(c, blank_pixels, min_scale, max_scale) for cid, c in source_cameras.items()})
    ids, names, cams, view = model_views(model)
    if not ids:
        raise ValueError('%s: the model holds no image' % what)
    paths = [os.path.join(image_dir, n) for n in names]
    for p in paths:
        if not os.path.exists(p):
            raise FileNotFoundError('%s: %s (named by the model) does not exist' % (what, p))
    pts = model['points']
    tracks = (pts['track_off'], view)
    scores, counts = viewsel.view_scores(pts['xyz'], viewsel.centers_from_cams(cams), tracks, theta0, sigma1, sigma2)
    pairs, pair_scores = viewsel.select_pairs(scores, counts, num_pairs)
    ranges = viewsel.depth_ranges(pts['xyz'], tracks, cams[:, 0]).cpu().numpy()
    os.makedirs(os.path.join(out_root, 'images'), exist_ok=True)
    os.makedirs(os.path.join(out_root, 'cams'), exist_ok=True)
    if undistort:
        for cid in sorted(source_cameras):                                  # one camera's images share one source map: they go through the kernel together
            group = [i for i, iid in enumerate(ids) if model['images'][iid]['camera_id'] == cid]
            und.undistort_files(source_cameras[cid], model['cameras'][cid], [paths[i] for i in group],
                                [os.path.join(out_root, 'images', '%08d.png' % i) for i in group])
    for i, p in enumerate(paths):
        cams[i, 1, 3] = ranges[i, 0], (ranges[i, 1] - ranges[i, 0]) / (max_d - 1) / interval_scale, max_d, ranges[i, 1]
        _write_cam(os.path.join(out_root, 'cams', '%08d_cam.txt' % i), cams[i])
        if undistort:
            continue
        ext = os.path.splitext(p)[1].lower()
        if ext in ('.jpg', '.png'):
            shutil.copyfile(p, os.path.join(out_root, 'images', '%08d%s' % (i, ext)))
        else:
            from PIL import Image
            with Image.open(p) as im:
                im.convert('RGB').save(os.path.join(out_root, 'images', '%08d.png' % i))
    viewsel.write_pair(os.path.join(out_root, 'pair.txt'), ['%d' % i for i in range(len(ids))], pairs, pair_scores)
    return {'ids': ids, 'names': names, 'cams': cams, 'pairs': pairs, 'pair_scores': pair_scores, 'scores': scores, 'counts': counts}
