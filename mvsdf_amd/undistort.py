"""Image undistortion on the device: a COLMAP model with distorted cameras becomes pinhole views -- resampled images, PINHOLE cameras and undistorted
observations -- so that datasets/colmap.py, which takes pinhole cameras only, opens for the models COLMAP's mapper actually writes.  Kernels:
csrc/undistort.hip (the work split: DESIGN.md); tests/undistort_ref.py restates every step in numpy.  The idea is that of COLMAP's image
undistorter; its text is not available to this project and the reference has no counterpart, so the definition below is this project's own
statement and no agreement with COLMAP's undistorter is claimed beyond the idea.

Cameras are the dicts of datasets/colmap.py ({'model', 'width', 'height', 'params'}), the parameters in COLMAP's documented order:
SIMPLE_PINHOLE (f, cx, cy), PINHOLE (fx, fy, cx, cy), SIMPLE_RADIAL (f, cx, cy, k), RADIAL (f, cx, cy, k1, k2), OPENCV (fx, fy, cx, cy, k1, k2, p1,
p2), FULL_OPENCV (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6), OPENCV_FISHEYE (fx, fy, cx, cy, k1, k2, k3, k4), SIMPLE_RADIAL_FISHEYE (f, cx, cy,
k), RADIAL_FISHEYE (f, cx, cy, k1, k2).  One-focal models have fx = fy = f; a coefficient a model does not have is 0 (adding 0 * x changes no bit
of what follows).  FOV and THIN_PRISM_FISHEYE are refused.  The centre of pixel (x, y) is (x + 0.5, y + 0.5).

The definition (fp64 throughout, in the order written, no FMA contraction):

- Pixel <-> normalised: u = (X - cx) / fx, v = (Y - cy) / fy; X = fx * ud + cx, Y = fy * vd + cy.
- The forward map D(u, v) -> (ud, vd), with r2 = u*u + v*v, r4 = r2*r2, r6 = r4*r2:
  - SIMPLE_PINHOLE, PINHOLE: (u, v).
  - SIMPLE_RADIAL, RADIAL: s = (1 + k1*r2) + k2*r4; (u*s, v*s).
  - OPENCV, FULL_OPENCV: num = ((1 + k1*r2) + k2*r4) + k3*r6; den = ((1 + k4*r2) + k5*r4) + k6*r6; s = num / den; tx = ((2*p1)*u)*v + p2*(r2 +
    (2*u)*u); ty = ((2*p2)*u)*v + p1*(r2 + (2*v)*v); (u*s + tx, v*s + ty).
  - the three fisheye models: r = sqrt(r2); theta = atan2(r, 1) by the written-out atan2 of csrc/det_math64.h (not a library call: ocml and libm
    differ in the last bits); t2 = theta*theta; p = k4; p = p*t2 + k3; p = p*t2 + k2; p = p*t2 + k1; p = p*t2 + 1; thetad = theta*p; s = thetad / r
    if r > 1e-8 else 1; (u*s, v*s).  With every coefficient 0 this is the equidistant fisheye, which is NOT a pinhole.
- The inverse map U(xd, yd): Newton's iteration on D.  x = xd, y = yd; then up to 33 rounds, the last without an update: (fx_, fy_) = D(x, y); ex =
  fx_ - xd, ey = fy_ - yd; res = max(|ex|*fx, |ey|*fy) (the residual in pixels).  The lane stops, and no longer changes, when ex or ey is not
  finite (error), when res <= 1e-13, or after its 32nd update.  Otherwise, with h = 1e-6: a = D(x + h, y), b = D(x - h, y), p = D(x, y + h), q =
  D(x, y - h); j00 = (a.x - b.x)/(2h), j01 = (p.x - q.x)/(2h), j10 = (a.y - b.y)/(2h), j11 = (p.y - q.y)/(2h); det = j00*j11 - j01*j10 (zero or not
  finite: error); sx = (j11*ex - j01*ey)/det, sy = (j00*ey - j10*ex)/det; x = x - sx, y = y - sy.  A final res above 1e-10 px is an error.  With D
  the identity res is exactly 0 at the start, so U returns its input bit for bit.  Errors travel as bits in a device header that is read once
  per call, and raise ValueError.
- undistort_points: (X, Y) in source pixels -> U((X - cx)/fx, (Y - cy)/fy) = (xu, yu) -> (fx'*xu + cx', fy'*yu + cy') in the output camera (without
  one: fx' = fy' = 1, cx' = cy' = 0, the normalised coordinates themselves).  distort_points is the way back through D.
- The output camera (undistorted_camera): PINHOLE with the source's fx, fy.  The source's principal point must lie strictly inside its image.
  Border samples in source pixels: (0, y + 0.5) and (W, y + 0.5) for every row y, (x + 0.5, 0) and (x + 0.5, H) for every column x, and the four
  corners.  Each goes through U on the device; ratio = xu / xd for the left and right border, yu / yd for the top and bottom border, both for the
  corners (xd, yd: the sample's own normalised coordinates).  Every ratio must be finite and > 0 (else the model folds over inside the image:
  ValueError).  s_full = min(ratios) (no blank pixel in the output), s_all = max(ratios) (no source pixel lost); s = s_full + blank_pixels * (s_all
  - s_full), then max(s, min_scale), then min(s, max_scale).  W' = max(1, floor(s*W)), H' = max(1, floor(s*H)); cx' = (cx*W')/W, cy' = (cy*H')/H.
- Resampling (undistort_images): for output pixel (x, y): u = ((x + 0.5) - cx')/fx', v = ((y + 0.5) - cy')/fy'; (ud, vd) = D(u, v); Xs = fx*ud + cx,
  Ys = fy*vd + cy.  Valid iff 0 <= Xs <= W and 0 <= Ys <= H (NaN is invalid).  a = Xs - 0.5; x0 = floor(a); tx = a - x0; the neighbours x0 and x0 +
  1 are clamped to [0, W - 1]; likewise b = Ys - 0.5, y0, ty.  value = (1 - ty)*((1 - tx)*p00 + tx*p10) + ty*((1 - tx)*p01 + tx*p11), p10 the x
  neighbour, p01 the y neighbour, the texels converted to fp64 exactly.  uint8 images give uint8, floor(value + 0.5); float32 images give float32,
  value rounded to nearest.  Invalid pixels are 0; the validity mask uint8 [H', W'] belongs to the camera, not to an image.

Images are [V, H, W, C] with C in 1..4, interleaved as PIL gives them.  Images that are not on the device go through it view_chunk at a time, so
that a chunk's input and output stay within CHUNK_BYTES of device memory.
"""
import os

import numpy as np
import torch

from ._lib import check, K, lib, raise_for_bits, _header, _stream, _vp

CHUNK_BYTES = 1 << 30                                # device memory one chunk of views may take, input plus output
# model -> (family of csrc/undistort.hip, indices of fx, fy, cx, cy in the parameters, where the family's coefficients come from)
_RADIAL, _OPENCV, _FISHEYE = 1, 2, 3
_MODELS = {'SIMPLE_PINHOLE': (0, (0, 0, 1, 2), ()), 'PINHOLE': (0, (0, 1, 2, 3), ()),
           'SIMPLE_RADIAL': (_RADIAL, (0, 0, 1, 2), (3,)), 'RADIAL': (_RADIAL, (0, 0, 1, 2), (3, 4)),
           'OPENCV': (_OPENCV, (0, 1, 2, 3), (4, 5, 6, 7)), 'FULL_OPENCV': (_OPENCV, (0, 1, 2, 3), (4, 5, 6, 7, 8, 9, 10, 11)),
           'OPENCV_FISHEYE': (_FISHEYE, (0, 1, 2, 3), (4, 5, 6, 7)), 'SIMPLE_RADIAL_FISHEYE': (_FISHEYE, (0, 0, 1, 2), (3,)),
           'RADIAL_FISHEYE': (_FISHEYE, (0, 0, 1, 2), (3, 4))}
_N_PARAMS = {'SIMPLE_PINHOLE': 3, 'PINHOLE': 4, 'SIMPLE_RADIAL': 4, 'RADIAL': 5, 'OPENCV': 8, 'FULL_OPENCV': 12, 'OPENCV_FISHEYE': 8,
             'SIMPLE_RADIAL_FISHEYE': 4, 'RADIAL_FISHEYE': 5}
SUPPORTED_MODELS = tuple(_MODELS)
_UNIT = np.array([1.0, 1.0, 0.0, 0.0])


def camera_block(camera):
    """A camera dict -> (family, params fp64 [12] = fx, fy, cx, cy, the family's eight coefficients), what the C calls take; ValueError for a model
    that is not built, a wrong parameter count, a non-finite parameter or a focal length that is not > 0"""
    name = camera['model']
    if name not in _MODELS:
        raise ValueError('undistort: camera model %s is not supported (%s): undistort the images first' % (name, ', '.join(SUPPORTED_MODELS)))
    p = np.asarray(camera['params'], dtype=np.float64).reshape(-1)
    if len(p) != _N_PARAMS[name]:
        raise ValueError('undistort: camera model %s takes %d parameters, got %d' % (name, _N_PARAMS[name], len(p)))
    if not np.isfinite(p).all():
        raise ValueError('undistort: the %s camera has a parameter that is NaN or infinite: %s' % (name, p.tolist()))
    family, pin, coef = _MODELS[name]
    block = np.zeros(12)
    block[:4] = p[list(pin)]
    block[4:4 + len(coef)] = p[list(coef)]
    if not (block[0] > 0 and block[1] > 0):
        raise ValueError('undistort: the focal lengths must be > 0, got %r, %r' % (block[0], block[1]))
    return family, block


def _size(camera):
    W, H = int(camera['width']), int(camera['height'])
    if W < 1 or H < 1:
        raise ValueError('undistort: the camera is %d x %d' % (W, H))
    return W, H


def _pinhole_block(camera, what):
    """fx, fy, cx, cy of a SIMPLE_PINHOLE / PINHOLE camera, or the unit camera for None"""
    if camera is None:
        return _UNIT.copy()
    if camera['model'] not in ('SIMPLE_PINHOLE', 'PINHOLE'):
        raise ValueError('%s: the undistorted camera must be SIMPLE_PINHOLE or PINHOLE, got %s' % (what, camera['model']))
    return camera_block(camera)[1][:4].copy()


# the error bits of an undistort call (csrc/undistort.hip), in the order they are looked at
ERRORS = [(K.MVSDF_UD_ERR_FINITE, ValueError, 'a non-finite value or a singular Jacobian in the inverse map (a point far outside what the model covers, or a NaN)'),
          (K.MVSDF_UD_ERR_CONVERGE, ValueError, 'the inverse map did not converge (the point lies outside what the distortion model reaches)')]


def _map_points(points, camera, pinhole, inverse, what):
    family, block = camera_block(camera)
    pin = _pinhole_block(pinhole, what)
    p = torch.as_tensor(points)
    if p.dim() != 2 or p.shape[1] != 2:
        raise ValueError('%s: points must be [N, 2], got shape %s' % (what, tuple(p.shape)))
    dev = p.device if p.is_cuda else torch.device('cuda')
    p = p.to(dev, torch.float64).contiguous()
    n = p.shape[0]
    out = torch.empty(n, 2, dtype=torch.float64, device=dev)
    hdr = torch.empty(256, dtype=torch.uint8, device=dev)
    check(lib().mvsdf_undistort_points(_vp(p) if n else None, n, family, block.ctypes.data, pin.ctypes.data, inverse, _vp(out) if n else None, _vp(hdr),
                                       _stream(hdr)), 'mvsdf_undistort_points')
    raise_for_bits(_header(hdr, K.MVSDF_RES_H_WORDS)[K.MVSDF_RES_H_ERR], what, ERRORS)   # the one wait of the call
    return out


def undistort_points(points, camera, out_camera=None):
    """points [N, 2] in the distorted camera's pixels -> fp64 [N, 2] on the device: the pixels of out_camera (a pinhole camera dict), or the
    normalised undistorted coordinates without one.  ValueError where the inverse map fails."""
    return _map_points(points, camera, out_camera, 1, 'undistort_points')


def distort_points(points, camera, in_camera=None):
    """The way back: points [N, 2] in the pixels of the pinhole in_camera (normalised coordinates without one) -> fp64 [N, 2] on the device, the
    distorted camera's pixels"""
    return _map_points(points, camera, in_camera, 0, 'distort_points')


def border_samples(W, H):
    """The definition's border samples -> (points fp64 [2H + 2W + 4, 2] in source pixels, axis int [same]: 0 = the ratio is taken along x, 1 = along y,
    2 = both (the corners))"""
    ys, xs = np.arange(H) + 0.5, np.arange(W) + 0.5
    pts = np.concatenate([np.stack([np.zeros(H), ys], 1), np.stack([np.full(H, float(W)), ys], 1), np.stack([xs, np.zeros(W)], 1),
                          np.stack([xs, np.full(W, float(H))], 1), np.array([[0.0, 0.0], [W, 0.0], [0.0, H], [W, H]])])
    axis = np.concatenate([np.zeros(2 * H, np.int64), np.ones(2 * W, np.int64), np.full(4, 2, np.int64)])
    return pts, axis


def scale_rule(camera, undistorted, blank_pixels=0.0, min_scale=0.2, max_scale=2.0):
    """The host half of undistorted_camera: `undistorted` fp64 [n, 2] = the border samples of border_samples through U, normalised -> (the output camera,
    s, s_full, s_all)"""
    W, H = _size(camera)
    _, block = camera_block(camera)
    fx, fy, cx, cy = block[:4]
    pts, axis = border_samples(W, H)
    und = np.asarray(undistorted, dtype=np.float64)
    xd, yd = (pts[:, 0] - cx) / fx, (pts[:, 1] - cy) / fy
    with np.errstate(all='ignore'):
        ratios = np.concatenate([und[axis != 1, 0] / xd[axis != 1], und[axis != 0, 1] / yd[axis != 0]])
    if not (np.isfinite(ratios).all() and (ratios > 0).all()):
        raise ValueError('undistorted_camera: the %s model folds over inside the %d x %d image (an undistorted / distorted border ratio is not a '
                         'positive finite number)' % (camera['model'], W, H))
    s_full, s_all = ratios.min(), ratios.max()
    s = s_full + blank_pixels * (s_all - s_full)
    s = min(max(s, min_scale), max_scale)
    Wo, Ho = max(1, int(np.floor(s * W))), max(1, int(np.floor(s * H)))
    out = {'model': 'PINHOLE', 'width': Wo, 'height': Ho, 'params': np.array([fx, fy, (cx * Wo) / W, (cy * Ho) / H])}
    return out, float(s), float(s_full), float(s_all)


def check_scale_arguments(camera, blank_pixels, min_scale, max_scale, what='undistorted_camera'):
    """-> (blank_pixels, min_scale, max_scale) as floats; ValueError for values outside the rule's domain or a principal point outside the image"""
    blank_pixels, min_scale, max_scale = float(blank_pixels), float(min_scale), float(max_scale)
    if not 0 <= blank_pixels <= 1:
        raise ValueError('%s: blank_pixels must be in [0, 1], got %r' % (what, blank_pixels))
    if not (0 < min_scale <= max_scale and np.isfinite(max_scale)):
        raise ValueError('%s: 0 < min_scale <= max_scale is needed, got %r, %r' % (what, min_scale, max_scale))
    W, H = _size(camera)
    cx, cy = camera_block(camera)[1][2:4]
    if not (0 < cx < W and 0 < cy < H):
        raise ValueError('%s: the principal point (%r, %r) must lie strictly inside the %d x %d image' % (what, cx, cy, W, H))
    return blank_pixels, min_scale, max_scale


def undistorted_camera(camera, blank_pixels=0.0, min_scale=0.2, max_scale=2.0):
    """The definition's output camera: a PINHOLE camera dict whose size and principal point follow the border rule.  blank_pixels = 0: the largest
    view without a blank pixel; 1: the smallest that loses no source pixel."""
    blank_pixels, min_scale, max_scale = check_scale_arguments(camera, blank_pixels, min_scale, max_scale)
    try:
        und = undistort_points(border_samples(*_size(camera))[0], camera).cpu().numpy()
    except ValueError as e:
        raise ValueError('undistorted_camera: the %s model folds over inside the image or does not reach its border (%s)' % (camera['model'], e))
    return scale_rule(camera, und, blank_pixels, min_scale, max_scale)[0]


def _chunk(V, in_bytes, out_bytes, view_chunk):
    if view_chunk is None:
        return max(1, min(max(V, 1), CHUNK_BYTES // max(1, in_bytes + out_bytes)))
    view_chunk = int(view_chunk)
    if view_chunk < 1:
        raise ValueError('undistort_images: view_chunk must be >= 1, got %d' % view_chunk)
    return view_chunk


def undistort_images(images, camera, out_camera=None, view_chunk=None):
    """images uint8 or float32 [V, H, W, C] of one camera (torch or numpy; H, W the camera's size, C in 1..4) -> (images' [V, H', W', C] of the same
    type, mask uint8 [H', W']) by the definition.  out_camera: a pinhole camera dict with its size (default: undistorted_camera(camera)).  The views
    go through the kernel view_chunk at a time (default: all of them for images already on the device, else as many as CHUNK_BYTES holds); the
    results live where the images lived (numpy and CPU tensors give CPU tensors)."""
    what = 'undistort_images'
    family, block = camera_block(camera)
    W, H = _size(camera)
    if out_camera is None:
        out_camera = undistorted_camera(camera)
    pin = _pinhole_block(out_camera, what)
    Wo, Ho = _size(out_camera)
    img = torch.as_tensor(images)
    if img.dim() != 4 or tuple(img.shape[1:3]) != (H, W) or not 1 <= img.shape[3] <= 4:
        raise ValueError('%s: images must be [V, %d, %d, C] with C in 1..4 (the camera is %d x %d), got shape %s' % (what, H, W, W, H, tuple(img.shape)))
    if img.dtype not in (torch.uint8, torch.float32):
        raise ValueError('%s: images must be uint8 or float32, got %s' % (what, img.dtype))
    V, C = img.shape[0], img.shape[3]
    dtype = 0 if img.dtype == torch.uint8 else 1
    on_device = img.is_cuda
    dev = img.device if on_device else torch.device('cuda')
    per = img.element_size() * C
    chunk = V if (on_device and view_chunk is None) else _chunk(V, H * W * per, Ho * Wo * per, view_chunk)
    out = torch.empty(V, Ho, Wo, C, dtype=img.dtype, device=img.device)
    mask = torch.empty(Ho, Wo, dtype=torch.uint8, device=dev)
    L = lib()
    first = True
    for v0 in range(0, max(V, 1), max(chunk, 1)):
        nv = min(chunk, V - v0)
        src = img[v0:v0 + nv].to(dev).contiguous()
        dst = out[v0:v0 + nv] if on_device else torch.empty(nv, Ho, Wo, C, dtype=img.dtype, device=dev)
        check(L.mvsdf_undistort_images(_vp(src) if nv else None, nv, H, W, C, dtype, family, block.ctypes.data, pin.ctypes.data, Ho, Wo, _vp(dst) if nv else None,
                                       _vp(mask) if first else None, _stream(mask)), 'mvsdf_undistort_images')
        if not on_device and nv:
            out[v0:v0 + nv] = dst.cpu()
        first = False
    return out, (mask if on_device else mask.cpu())


def _load_group(paths, W, H, what, mode=None):
    """the image files of one camera -> (uint8 [n, H, W, C], the PIL mode they share: that of the first file where it is L, RGB or RGBA, else RGB);
    every file must have the camera's size"""
    from PIL import Image
    arrays = []
    for p in paths:
        with Image.open(p) as im:
            if im.size != (W, H):
                raise ValueError('%s: %s is %d x %d, its camera %d x %d' % (what, p, im.size[0], im.size[1], W, H))
            if mode is None:
                mode = im.mode if im.mode in ('L', 'RGB', 'RGBA') else 'RGB'
            arrays.append(np.asarray(im if im.mode == mode else im.convert(mode)).reshape(H, W, -1))
    return np.stack(arrays), mode


def undistort_files(camera, out_camera, paths, out_paths, view_chunk=None):
    """The image files `paths` of one camera through undistort_images, view_chunk files at a time, written to out_paths (png or jpg by their
    extension)"""
    from PIL import Image
    what = 'undistort_model'
    W, H = _size(camera)
    Wo, Ho = _size(out_camera)
    step = _chunk(len(paths), H * W * 4, Ho * Wo * 4, view_chunk)
    mode = None
    for k in range(0, len(paths), step):
        src, mode = _load_group(paths[k:k + step], W, H, what, mode)
        dst, _ = undistort_images(src, camera, out_camera, view_chunk=len(src))
        for a, q in zip(dst.numpy(), out_paths[k:k + step]):
            Image.fromarray(a[:, :, 0] if mode == 'L' else a).save(q)


def output_name(name):
    """the file name an undistorted image gets: png and jpg keep theirs, other formats become png"""
    return name if os.path.splitext(name)[1].lower() in ('.png', '.jpg') else os.path.splitext(name)[0] + '.png'


def undistort_model(model, image_dir, out_dir, blank_pixels=0.0, min_scale=0.2, max_scale=2.0, view_chunk=None):
    """A loaded model (datasets.colmap.load_colmap_model(dir, allow_distortion=True)) and its images -> out_dir/images/<name> (the names kept; png and
    jpg re-encoded, other formats written as png under the changed name) and out_dir/sparse/{cameras,images,points3D}.txt with PINHOLE cameras, the
    observations through undistort_points, poses and points unchanged.  Images are grouped by camera id; a file whose size differs from its camera's
    is a ValueError.  -> the undistorted model."""
    from .datasets.colmap import write_colmap_text
    what = 'undistort_model'
    for iid, im in model['images'].items():
        if im['camera_id'] not in model['cameras']:
            raise ValueError('%s: image %d refers to camera %d, which the model does not hold' % (what, iid, im['camera_id']))
        if not os.path.exists(os.path.join(image_dir, im['name'])):
            raise FileNotFoundError('%s: %s (named by the model) does not exist' % (what, os.path.join(image_dir, im['name'])))
    cameras = {cid: undistorted_camera(cam, blank_pixels, min_scale, max_scale) for cid, cam in model['cameras'].items()}
    images = {}
    for cid in sorted(model['cameras']):
        ids = [iid for iid in sorted(model['images']) if model['images'][iid]['camera_id'] == cid]
        if not ids:
            continue
        names = [model['images'][iid]['name'] for iid in ids]
        outs = [os.path.join(out_dir, 'images', output_name(n)) for n in names]
        for q in outs:
            os.makedirs(os.path.dirname(q), exist_ok=True)
        undistort_files(model['cameras'][cid], cameras[cid], [os.path.join(image_dir, n) for n in names], outs, view_chunk)
        counts = [len(model['images'][iid]['xys']) for iid in ids]
        xys = np.concatenate([np.asarray(model['images'][iid]['xys'], np.float64).reshape(-1, 2) for iid in ids])
        und = undistort_points(xys, model['cameras'][cid], cameras[cid]).cpu().numpy()              # one call per camera
        at = 0
        for iid, n, name in zip(ids, counts, names):
            images[iid] = dict(model['images'][iid], name=output_name(name), xys=und[at:at + n].copy())
            at += n
    out = {'cameras': cameras, 'images': images, 'points': model['points']}
    write_colmap_text(out, os.path.join(out_dir, 'sparse'))
    return out
