"""The numpy restatement of mvsdf_amd/raster.py's definition: rasterise, visibility, colours and the camera-centre helper.  fp64 throughout, every
operation in the order the definition writes it (numpy never contracts a product and a sum).  The yardstick of tests/test_gpu_raster.py, which
holds the device to it bit for bit; tests/test_raster_host.py checks it against closed forms."""
import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def camera_centers(P):
    P = np.asarray(P, np.float64)
    return np.stack([-np.linalg.inv(p[:3, :3]) @ p[:3, 3] for p in P])


def look_at(eye, target, hw, focal, up=(0.0, 0.0, 1.0)):
    """a pinhole camera at `eye` looking at `target` -> P fp64 [4,4] (row 2 = the depth along the axis, principal point at the image middle)"""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    K = np.array([[focal, 0, hw[1] / 2.0], [0, focal, hw[0] / 2.0], [0, 0, 1.0]])
    P = np.eye(4)
    P[:3, :3] = K @ R
    P[:3, 3] = K @ (-R @ eye)
    return P


def _row(t, X):
    return ((t[0] * X[:, 0] + t[1] * X[:, 1]) + t[2] * X[:, 2]) + t[3] * 1.0


def project(Pv, verts):
    """-> (front bool [N], sx, sy, z fp64 [N]); sx, sy are NaN where the vertex is not in front"""
    X = np.asarray(verts, np.float32).astype(np.float64)
    z = _row(Pv[2], X)
    front = z > 0
    with np.errstate(all='ignore'):
        sx = np.where(front, _row(Pv[0], X) / np.where(front, z, 1.0), np.nan)
        sy = np.where(front, _row(Pv[1], X) / np.where(front, z, 1.0), np.nan)
    return front, sx, sy, z


def _edge(px, py, qx, qy, rx, ry):
    return (qx - px) * (ry - py) - (qy - py) * (rx - px)


def raster_keys(verts, faces, P, hw, o=0.5, stats=None):
    """the key buffer uint64 [V,H,W].  stats (a dict): 'boxes' int64 [V,F] = the pixels of every face's clamped box (0: not drawn), 'ties' = the
    number of pixels where a face met an equal depth of another face."""
    H, W = hw
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    P = np.asarray(P, np.float64)
    keys = np.full((len(P), H, W), EMPTY, np.uint64)
    boxes = np.zeros((len(P), len(faces)), np.int64)
    ties = 0
    for v, Pv in enumerate(P):
        front, sx, sy, z = project(Pv, verts)
        a, b, c = faces[:, 0], faces[:, 1], faces[:, 2]
        ok = front[a] & front[b] & front[c]
        with np.errstate(all='ignore'):
            for q in (sx, sy, z):
                ok &= np.isfinite(q[a]) & np.isfinite(q[b]) & np.isfinite(q[c])
            A = _edge(sx[a], sy[a], sx[b], sy[b], sx[c], sy[c])
            ok &= ~(A == 0)
            lx = np.maximum(0.0, np.ceil(np.minimum(np.minimum(sx[a], sx[b]), sx[c]) - o))
            hx = np.minimum(float(W - 1), np.floor(np.maximum(np.maximum(sx[a], sx[b]), sx[c]) - o))
            ly = np.maximum(0.0, np.ceil(np.minimum(np.minimum(sy[a], sy[b]), sy[c]) - o))
            hy = np.minimum(float(H - 1), np.floor(np.maximum(np.maximum(sy[a], sy[b]), sy[c]) - o))
            ok &= (lx <= hx) & (ly <= hy)
        kv = keys[v]
        for f in np.nonzero(ok)[0]:
            x0, x1, y0, y1 = int(lx[f]), int(hx[f]), int(ly[f]), int(hy[f])
            boxes[v, f] = (x1 - x0 + 1) * (y1 - y0 + 1)
            ia, ib, ic = a[f], b[f], c[f]
            cx = (np.arange(x0, x1 + 1, dtype=np.float64) + o)[None, :]
            cy = (np.arange(y0, y1 + 1, dtype=np.float64) + o)[:, None]
            with np.errstate(all='ignore'):
                w0 = _edge(sx[ib], sy[ib], sx[ic], sy[ic], cx, cy)
                w1 = _edge(sx[ic], sy[ic], sx[ia], sy[ia], cx, cy)
                w2 = _edge(sx[ia], sy[ia], sx[ib], sy[ib], cx, cy)
                Af = A[f]
                if Af < 0:
                    w0, w1, w2, Af = -w0, -w1, -w2, -Af
                cov = (w0 >= 0) & (w1 >= 0) & (w2 >= 0)
                if not cov.any():
                    continue
                iz = ((w0 / Af) / z[ia] + (w1 / Af) / z[ib]) + (w2 / Af) / z[ic]
                zp = 1.0 / iz
                cov &= np.isfinite(zp) & (zp > 0)
                d32 = zp.astype(np.float32)
                cov &= ~(d32 == 0) & ~np.isinf(d32)
            key = (d32.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
            sub = kv[y0:y1 + 1, x0:x1 + 1]
            if stats is not None:
                ties += int((cov & ((sub >> np.uint64(32)) == (key >> np.uint64(32)))).sum())
            np.copyto(sub, np.minimum(sub, key), where=cov)
    if stats is not None:
        stats['boxes'] = boxes
        stats['ties'] = ties
    return keys


def resolve(keys):
    """keys -> (depth fp32, face int32)"""
    drawn = keys != EMPTY
    depth = np.where(drawn, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0))
    face = np.where(drawn, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    return depth.astype(np.float32), face


def rasterize(verts, faces, P, hw, o=0.5, stats=None):
    return resolve(raster_keys(verts, faces, P, hw, o, stats))


def _visible(Pv, verts, depth_v, o, mask_v, depth_tol):
    H, W = depth_v.shape
    front, sx, sy, z = project(Pv, verts)
    with np.errstate(all='ignore'):
        x = np.floor(sx - o + 0.5)
        y = np.floor(sy - o + 0.5)
        inside = front & (x >= 0) & (x < W) & (y >= 0) & (y < H)
    xi = np.where(inside, x, 0).astype(np.int64)
    yi = np.where(inside, y, 0).astype(np.int64)
    D = depth_v[yi, xi]
    with np.errstate(all='ignore'):
        vis = inside & (D > 0) & (z <= D.astype(np.float64) * (1.0 + depth_tol))
    if mask_v is not None:
        vis &= np.asarray(mask_v)[yi, xi] != 0
    return vis, sx, sy


def visibility(verts, P, depth, o=0.5, masks=None, depth_tol=0.01):
    """-> uint8 [V, Nv]"""
    P = np.asarray(P, np.float64)
    return np.stack([_visible(P[v], verts, depth[v], o, None if masks is None else masks[v], depth_tol)[0]
                     for v in range(len(P))]).astype(np.uint8)


def colors(verts, normals, P, depth, images, o=0.5, masks=None, depth_tol=0.01, cos_min=0.0, ignore_normals=False, fallback=(0.5, 0.5, 0.5)):
    """-> (colours fp32 [Nv,3], n_views int32 [Nv])"""
    P = np.asarray(P, np.float64)
    C = camera_centers(P)
    X = np.asarray(verts, np.float32).astype(np.float64)
    n = np.asarray(normals, np.float32).astype(np.float64)
    V, H, W = depth.shape
    nv = len(X)
    flat = (n[:, 0] == 0) & (n[:, 1] == 0) & (n[:, 2] == 0)
    S = np.zeros((nv, 3))
    Wsum = np.zeros(nv)
    used = np.zeros(nv, np.int32)
    for v in range(V):
        vis, sx, sy = _visible(P[v], verts, depth[v], o, None if masks is None else masks[v], depth_tol)
        g = C[v][None, :] - X
        with np.errstate(all='ignore'):
            cosang = ((n[:, 0] * g[:, 0] + n[:, 1] * g[:, 1]) + n[:, 2] * g[:, 2]) / np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
            take = vis & np.where(flat, bool(ignore_normals), cosang > cos_min)
            wgt = np.where(flat, 1.0, cosang)
            u, t = sx - o, sy - o
            take &= (u >= 0) & (u <= W - 1) & (t >= 0) & (t <= H - 1)
        u, t = np.where(take, u, 0.0), np.where(take, t, 0.0)
        x0, y0 = np.minimum(np.floor(u), float(W - 2)), np.minimum(np.floor(t), float(H - 2))
        fx, fy = (u - x0)[:, None], (t - y0)[:, None]
        xi, yi = x0.astype(np.int64), y0.astype(np.int64)
        im = images[v].astype(np.float64)
        c00, c01, c10, c11 = im[yi, xi], im[yi, xi + 1], im[yi + 1, xi], im[yi + 1, xi + 1]
        col = (c00 * (1.0 - fx) + c01 * fx) * (1.0 - fy) + (c10 * (1.0 - fx) + c11 * fx) * fy
        idx = np.nonzero(take)[0]
        S[idx] += wgt[idx, None] * col[idx]
        Wsum[idx] += wgt[idx]
        used[idx] += 1
    have = Wsum > 0
    with np.errstate(all='ignore'):
        out = np.where(have[:, None], (S / Wsum[:, None] / 255.0).astype(np.float32), np.asarray(fallback, np.float32)[None, :])
    return out.astype(np.float32), used
