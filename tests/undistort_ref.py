"""The numpy restatement of mvsdf_amd/undistort.py's definition, operation for operation (every line is one correctly rounded fp64 operation, so the
bits equal those of csrc/undistort.hip on the host and on the device), the test cameras, and the models' formulas once more through np.arctan for the
independent checks.  Nothing here imports the module under test.  Not a test module."""
import numpy as np

from viewsel_ref import atan2_pos

STEP, STOP_PX, BOUND_PX, MAX_UPDATES, FISHEYE_EPS = 1e-6, 1e-13, 1e-10, 32, 1e-8
PINHOLE, RADIAL, OPENCV, FISHEYE = 0, 1, 2, 3
# model -> (family, indices of fx, fy, cx, cy, indices of the family's coefficients)
MODELS = {'SIMPLE_PINHOLE': (PINHOLE, (0, 0, 1, 2), ()), 'PINHOLE': (PINHOLE, (0, 1, 2, 3), ()),
          'SIMPLE_RADIAL': (RADIAL, (0, 0, 1, 2), (3,)), 'RADIAL': (RADIAL, (0, 0, 1, 2), (3, 4)),
          'OPENCV': (OPENCV, (0, 1, 2, 3), (4, 5, 6, 7)), 'FULL_OPENCV': (OPENCV, (0, 1, 2, 3), tuple(range(4, 12))),
          'OPENCV_FISHEYE': (FISHEYE, (0, 1, 2, 3), (4, 5, 6, 7)), 'SIMPLE_RADIAL_FISHEYE': (FISHEYE, (0, 0, 1, 2), (3,)),
          'RADIAL_FISHEYE': (FISHEYE, (0, 0, 1, 2), (3, 4))}

# the test cameras: 37 x 29, f = 40, principal point (18.2, 14.9): odd, and off every tile and wave multiple
W, H, F, CX, CY = 37, 29, 40.0, 18.2, 14.9
DISTORTIONS = [('SIMPLE_RADIAL', [-0.2]), ('SIMPLE_RADIAL', [0.15]), ('SIMPLE_RADIAL', [0.0]),
               ('RADIAL', [-0.2, 0.05]), ('RADIAL', [0.1, 0.02]),
               ('OPENCV', [-0.2, 0.05, 0.01, -0.005]), ('OPENCV', [0.12, -0.02, -0.004, 0.006]),
               ('FULL_OPENCV', [-0.2, 0.05, 0.01, -0.005, 0.01, 0.02, -0.01, 0.005]),
               ('OPENCV_FISHEYE', [0.05, -0.01, 0.002, -0.001]), ('OPENCV_FISHEYE', [-0.08, 0.01, 0.0, 0.0]),
               ('SIMPLE_RADIAL_FISHEYE', [-0.1]), ('SIMPLE_RADIAL_FISHEYE', [0.5]),              # barrel; pincushion (k above the 1/3 of tan's own series)
               ('RADIAL_FISHEYE', [-0.1, 0.02]), ('RADIAL_FISHEYE', [0.45, 0.1])]
ONE_FOCAL = ('SIMPLE_PINHOLE', 'SIMPLE_RADIAL', 'RADIAL', 'SIMPLE_RADIAL_FISHEYE', 'RADIAL_FISHEYE')


def camera(model, dist=(), w=W, h=H, f=F, cx=CX, cy=CY, fy=None):
    """a camera dict of the model with the test intrinsics"""
    focal = [f] if model in ONE_FOCAL else [f, f if fy is None else fy]
    return {'model': model, 'width': w, 'height': h, 'params': np.array(focal + [cx, cy] + list(dist), dtype=np.float64)}


CAMERAS = [camera(m, d) for m, d in DISTORTIONS]
CAMERA_IDS = ['%s%s' % (m, d) for m, d in DISTORTIONS]
N_COEFFICIENTS = {'SIMPLE_PINHOLE': 0, 'PINHOLE': 0, 'SIMPLE_RADIAL': 1, 'RADIAL': 2, 'OPENCV': 4, 'FULL_OPENCV': 8, 'OPENCV_FISHEYE': 4,
                  'SIMPLE_RADIAL_FISHEYE': 1, 'RADIAL_FISHEYE': 2}


def _f(x):
    return np.asarray(x, dtype=np.float64)


def block(cam):
    """-> (family, fx, fy, cx, cy, k fp64 [8])"""
    family, pin, coef = MODELS[cam['model']]
    p = _f(cam['params'])
    k = np.zeros(8)
    k[:len(coef)] = p[list(coef)]
    return (family,) + tuple(float(p[i]) for i in pin) + (k,)


def distort(family, k, u, v):
    """the forward map D on normalised coordinates"""
    u, v = _f(u), _f(v)
    with np.errstate(all='ignore'):
        r2 = u * u + v * v
        if family == RADIAL:
            r4 = r2 * r2
            s = (1.0 + k[0] * r2) + k[1] * r4
            return u * s, v * s
        if family == OPENCV:
            r4 = r2 * r2
            r6 = r4 * r2
            num = ((1.0 + k[0] * r2) + k[1] * r4) + k[4] * r6
            den = ((1.0 + k[5] * r2) + k[6] * r4) + k[7] * r6
            s = num / den
            tx = ((2.0 * k[2]) * u) * v + k[3] * (r2 + (2.0 * u) * u)
            ty = ((2.0 * k[3]) * u) * v + k[2] * (r2 + (2.0 * v) * v)
            return u * s + tx, v * s + ty
        if family == FISHEYE:
            r = np.sqrt(r2)
            theta = atan2_pos(r, 1.0)
            t2 = theta * theta
            p = np.full(r.shape, k[3])
            p = p * t2 + k[2]
            p = p * t2 + k[1]
            p = p * t2 + k[0]
            p = p * t2 + 1.0
            thetad = theta * p
            big = r > FISHEYE_EPS
            s = np.where(big, thetad / np.where(big, r, 1.0), 1.0)
            return u * s, v * s
    return u.copy(), v.copy()


def undistort(family, k, fx, fy, xd, yd):
    """the inverse map U -> (x, y, err bits per point, the final residual in pixels)"""
    xd, yd = _f(xd), _f(yd)
    x, y = xd.copy(), yd.copy()
    res = np.zeros(xd.shape)
    err = np.zeros(xd.shape, np.int64)
    live = np.ones(xd.shape, bool)
    h, h2 = STEP, 2.0 * STEP
    with np.errstate(all='ignore'):
        for it in range(MAX_UPDATES + 1):
            gx, gy = distort(family, k, x, y)
            ex, ey = gx - xd, gy - yd
            bad = live & ~(np.isfinite(ex) & np.isfinite(ey))
            err[bad] = 1
            live &= ~bad
            rx, ry = np.abs(ex) * fx, np.abs(ey) * fy
            res = np.where(live, np.where(rx > ry, rx, ry), res)
            live &= ~(res <= STOP_PX)
            if it == MAX_UPDATES or not live.any():
                break
            ax, ay = distort(family, k, x + h, y)
            bx, by = distort(family, k, x - h, y)
            px, py = distort(family, k, x, y + h)
            qx, qy = distort(family, k, x, y - h)
            j00, j01, j10, j11 = (ax - bx) / h2, (px - qx) / h2, (ay - by) / h2, (py - qy) / h2
            det = j00 * j11 - j01 * j10
            bad = live & (~np.isfinite(det) | (det == 0.0))
            err[bad] = 1
            live &= ~bad
            sx, sy = (j11 * ex - j01 * ey) / det, (j00 * ey - j10 * ex) / det
            x = np.where(live, x - sx, x)
            y = np.where(live, y - sy, y)
    err[(err == 0) & (res > BOUND_PX)] = 2
    return x, y, err, res


def _pin(cam):
    if cam is None:
        return 1.0, 1.0, 0.0, 0.0
    assert cam['model'] in ('SIMPLE_PINHOLE', 'PINHOLE')
    return block(cam)[1:5]


def undistort_points(points, cam, out_cam=None, with_err=False):
    family, fx, fy, cx, cy, k = block(cam)
    ofx, ofy, ocx, ocy = _pin(out_cam)
    p = _f(points).reshape(-1, 2)
    x, y, err, res = undistort(family, k, fx, fy, (p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy)
    out = np.stack([ofx * x + ocx, ofy * y + ocy], 1)
    return (out, err, res) if with_err else out


def distort_points(points, cam, in_cam=None):
    family, fx, fy, cx, cy, k = block(cam)
    ifx, ify, icx, icy = _pin(in_cam)
    p = _f(points).reshape(-1, 2)
    ud, vd = distort(family, k, (p[:, 0] - icx) / ifx, (p[:, 1] - icy) / ify)
    return np.stack([fx * ud + cx, fy * vd + cy], 1)


def border_samples(w, h):
    """-> (points [2h + 2w + 4, 2], axis: 0 = the ratio along x, 1 = along y, 2 = both)"""
    pts = [(0.0, y + 0.5) for y in range(h)] + [(float(w), y + 0.5) for y in range(h)] + [(x + 0.5, 0.0) for x in range(w)] + \
          [(x + 0.5, float(h)) for x in range(w)] + [(0.0, 0.0), (float(w), 0.0), (0.0, float(h)), (float(w), float(h))]
    return _f(pts), np.array([0] * (2 * h) + [1] * (2 * w) + [2] * 4)


def undistorted_camera(cam, blank_pixels=0.0, min_scale=0.2, max_scale=2.0, details=False):
    family, fx, fy, cx, cy, k = block(cam)
    w, h = cam['width'], cam['height']
    if not (0 < cx < w and 0 < cy < h):
        raise ValueError('principal point')
    pts, axis = border_samples(w, h)
    und, err, _ = undistort_points(pts, cam, None, with_err=True)
    if err.any():
        raise ValueError('the inverse map fails on the border')
    xd, yd = (pts[:, 0] - cx) / fx, (pts[:, 1] - cy) / fy
    ratios = np.concatenate([und[axis != 1, 0] / xd[axis != 1], und[axis != 0, 1] / yd[axis != 0]])
    if not (np.isfinite(ratios).all() and (ratios > 0).all()):
        raise ValueError('the model folds over')
    s_full, s_all = ratios.min(), ratios.max()
    s = s_full + blank_pixels * (s_all - s_full)
    s = min(max(s, min_scale), max_scale)
    wo, ho = max(1, int(np.floor(s * w))), max(1, int(np.floor(s * h)))
    out = {'model': 'PINHOLE', 'width': wo, 'height': ho, 'params': np.array([fx, fy, (cx * wo) / w, (cy * ho) / h])}
    return (out, s, s_full, s_all) if details else out


def source_coordinates(cam, out_cam):
    """(Xs, Ys) fp64 [H', W'] of every output pixel"""
    family, fx, fy, cx, cy, k = block(cam)
    ofx, ofy, ocx, ocy = _pin(out_cam)
    x, y = np.meshgrid(np.arange(out_cam['width'], dtype=np.float64), np.arange(out_cam['height'], dtype=np.float64))
    ud, vd = distort(family, k, ((x + 0.5) - ocx) / ofx, ((y + 0.5) - ocy) / ofy)
    return fx * ud + cx, fy * vd + cy


def taps(cam, out_cam):
    """-> (valid bool [H', W'], x0c, x1c, y0c, y1c int64, tx, ty fp64): the four clamped neighbours and the weights of every output pixel"""
    w, h = cam['width'], cam['height']
    Xs, Ys = source_coordinates(cam, out_cam)
    with np.errstate(invalid='ignore'):
        valid = (Xs >= 0.0) & (Xs <= float(w)) & (Ys >= 0.0) & (Ys <= float(h))
    a, b = np.where(valid, Xs, 0.5) - 0.5, np.where(valid, Ys, 0.5) - 0.5
    x0, y0 = np.floor(a), np.floor(b)
    tx, ty = a - x0, b - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    return (valid, np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1), np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1), tx, ty)


def undistort_images(images, cam, out_cam, window=None):
    """images uint8 or float32 [V, H, W, C] -> (images' [V, H', W', C], mask uint8 [H', W']).  window: (origin (y, x), sub-image): the images are only
    known on that window of the source (the 64-bit test), which every valid pixel's neighbours must fall into."""
    images = np.asarray(images)
    valid, x0, x1, y0, y1, tx, ty = taps(cam, out_cam)
    if window is not None:
        (oy, ox), images = window[0], np.asarray(window[1])
        x0, x1, y0, y1 = x0 - ox, x1 - ox, y0 - oy, y1 - oy
        assert (x0[valid] >= 0).all() and (y0[valid] >= 0).all() and (x1[valid] < images.shape[2]).all() and (y1[valid] < images.shape[1]).all()
        x0, x1, y0, y1 = [np.where(valid, q, 0) for q in (x0, x1, y0, y1)]
    p = images.astype(np.float64)
    tx, ty = tx[None, :, :, None], ty[None, :, :, None]
    p00, p10, p01, p11 = p[:, y0, x0], p[:, y0, x1], p[:, y1, x0], p[:, y1, x1]
    value = (1.0 - ty) * ((1.0 - tx) * p00 + tx * p10) + ty * ((1.0 - tx) * p01 + tx * p11)
    if images.dtype == np.uint8:
        out = np.floor(value + 0.5).astype(np.uint8)
    else:
        out = value.astype(np.float32)
    out[:, ~valid] = 0
    return out, valid.astype(np.uint8)


# ---- the models' formulas once more, written directly with np.arctan: independent of everything above ----

def project_direct(cam, xyz):
    """3-d points in front of the camera -> distorted pixels, by the model's documented formula"""
    u, v = xyz[:, 0] / xyz[:, 2], xyz[:, 1] / xyz[:, 2]
    return direct(cam, u, v)


def direct(cam, u, v):
    name, p = cam['model'], [float(x) for x in cam['params']]
    if name in ONE_FOCAL:
        fx, fy, cx, cy, d = p[0], p[0], p[1], p[2], p[3:]
    else:
        fx, fy, cx, cy, d = p[0], p[1], p[2], p[3], p[4:]
    r2 = u ** 2 + v ** 2
    if name in ('SIMPLE_PINHOLE', 'PINHOLE'):
        ud, vd = u, v
    elif name == 'SIMPLE_RADIAL':
        ud, vd = u * (1 + d[0] * r2), v * (1 + d[0] * r2)
    elif name == 'RADIAL':
        ud, vd = u * (1 + d[0] * r2 + d[1] * r2 ** 2), v * (1 + d[0] * r2 + d[1] * r2 ** 2)
    elif name in ('OPENCV', 'FULL_OPENCV'):
        k1, k2, p1, p2 = d[:4]
        k3, k4, k5, k6 = d[4:] if name == 'FULL_OPENCV' else (0, 0, 0, 0)
        rad = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
        ud = u * rad + 2 * p1 * u * v + p2 * (r2 + 2 * u ** 2)
        vd = v * rad + 2 * p2 * u * v + p1 * (r2 + 2 * v ** 2)
    else:
        d = d + [0.0] * (4 - len(d))
        r = np.sqrt(r2)
        th = np.arctan(r)
        thd = th * (1 + d[0] * th ** 2 + d[1] * th ** 4 + d[2] * th ** 6 + d[3] * th ** 8)
        s = np.where(r > 1e-8, thd / np.where(r > 1e-8, r, 1.0), 1.0)
        ud, vd = u * s, v * s
    return np.stack([fx * ud + cx, fy * vd + cy], -1)
