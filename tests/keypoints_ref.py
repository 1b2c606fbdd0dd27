"""mvsdf_amd/keypoints.py's detector (1a to 1c), stages 2 to 5 and their composition restated in numpy, operation for operation: the blurs tap by tap, the matcher on integers (held in fp64, far below 2^53, so a
sum or a matrix product is exact in any order), the fp64 stages elementwise in the written order (no np.sum, no @ on a path where the device
rounds; the host-side camera arrays are inputs to both and come from the module).  Everything returns numpy arrays shaped like the module's results."""
import numpy as np

from viewsel_ref import atan2_pos, expneg, rint


def nearest_two(s, t):
    """codes int8 [ns,128], [nt,128] -> (j1 int64 [ns], D1 int64 [ns], D2 int64 [ns] (-1: none)) under the total order (D, j)"""
    s, t = s.astype(np.float64), t.astype(np.float64)             # integers below 2^53: every product and sum below is exact in any order
    ns, nt = len(s), len(t)
    j1, d1, d2 = np.zeros(ns, np.int64), np.zeros(ns, np.int64), np.full(ns, -1, np.int64)
    tt = (t * t).sum(1)
    for lo in range(0, ns, 256):
        c = s[lo:lo + 256]
        D = (((c * c).sum(1)[:, None] + tt[None, :]) - 2.0 * (c @ t.T)).astype(np.int64)
        j = np.argmin(D, axis=1)                                  # the first of equal minima: the lowest j
        rows = np.arange(len(j))
        j1[lo:lo + 256], d1[lo:lo + 256] = j, D[rows, j]
        if nt > 1:
            D[rows, j] = np.iinfo(np.int64).max
            d2[lo:lo + 256] = D.min(axis=1)
    return j1, d1, d2


def match_descriptors(codes, view_off, pairs=None, ratio=0.8, mutual=True, max_dist=None):
    codes, view_off = np.asarray(codes), np.asarray(view_off)
    V = len(view_off) - 1
    if pairs is None:
        pairs = [(a, b) for a in range(V) for b in range(a + 1, V)]
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    off, idx, dist = [0], [], []
    r2 = float(ratio) * float(ratio)
    for a, b in pairs:
        s, t = codes[view_off[a]:view_off[a + 1]], codes[view_off[b]:view_off[b + 1]]
        if len(s) and len(t):
            j1, d1, d2 = nearest_two(s, t)
            keep = (d2 < 0) | (d1.astype(np.float64) < r2 * d2.astype(np.float64))
            if max_dist is not None:
                keep &= d1 <= max_dist
            if mutual:
                keep &= nearest_two(t, s)[0][j1] == np.arange(len(s))
            i = np.nonzero(keep)[0]
            idx.append(np.stack([i, j1[i]], 1))
            dist.append(d1[i])
        off.append(off[-1] + (len(idx[-1]) if len(s) and len(t) else 0))
    idx = np.concatenate(idx).astype(np.int32) if idx else np.zeros((0, 2), np.int32)
    dist = np.concatenate(dist).astype(np.int32) if dist else np.zeros(0, np.int32)
    return pairs, np.asarray(off, np.int64), idx.reshape(-1, 2), dist


def _match_pair_ids(off):
    return np.repeat(np.arange(len(off) - 1), np.diff(off))


def _line_ok(l0, l1, l2, X, Y, limit):
    with np.errstate(divide='ignore', invalid='ignore'):
        d = np.abs((l0 * X + l1 * Y) + l2) / np.sqrt(l0 * l0 + l1 * l1)
    return ~((l0 == 0.0) & (l1 == 0.0)) & (d <= limit)


def verify_matches(xy, view_off, matches, F, max_epipolar=2.0):
    """F [M,3,3]: keypoints.fundamental_matrices"""
    pairs, off, idx, dist = matches
    m = _match_pair_ids(off)
    ga, gb = view_off[pairs[m, 0]] + idx[:, 0], view_off[pairs[m, 1]] + idx[:, 1]
    Xa, Ya, Xb, Yb = xy[ga, 0], xy[ga, 1], xy[gb, 0], xy[gb, 1]
    f = F[m]
    l = [(f[:, k, 0] * Xa + f[:, k, 1] * Ya) + f[:, k, 2] for k in range(3)]
    lt = [(f[:, 0, k] * Xb + f[:, 1, k] * Yb) + f[:, 2, k] for k in range(3)]
    keep = _line_ok(l[0], l[1], l[2], Xb, Yb, max_epipolar) & _line_ok(lt[0], lt[1], lt[2], Xa, Ya, max_epipolar)
    counts = np.bincount(m[keep], minlength=len(pairs))
    return pairs, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), idx[keep], dist[keep]


def build_tracks(view_off, matches):
    """components by union-find (the labelling's fixed point: every node carries the smallest node of its component)"""
    pairs, off, idx, _ = matches
    view_off = np.asarray(view_off)
    N = int(view_off[-1])
    m = _match_pair_ids(off)
    u, v = view_off[pairs[m, 0]] + idx[:, 0], view_off[pairs[m, 1]] + idx[:, 1]
    parent = list(range(N))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in zip(u.tolist(), v.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    label = np.array([find(x) for x in range(N)], np.int64)
    view = np.searchsorted(view_off, np.arange(N), side='right') - 1
    track_off, track_view, track_kp = [0], [], []
    order = np.lexsort((np.arange(N), label))
    bounds = np.nonzero(np.diff(label[order], prepend=-1))[0].tolist() + [N]
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        nodes = order[lo:hi]
        if len(nodes) < 2 or len(set(view[nodes].tolist())) < len(nodes):
            continue
        track_view += view[nodes].tolist()
        track_kp += (nodes - view_off[view[nodes]]).tolist()
        track_off.append(len(track_view))
    return np.asarray(track_off, np.int64), np.asarray(track_view, np.int32), np.asarray(track_kp, np.int32)


def _det3(m):
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])) + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0])


def _ray(rays, X, Y):
    d = [(rays[k, 0] * X + rays[k, 1] * Y) + rays[k, 2] for k in range(3)]
    n = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    return [d[0] / n, d[1] / n, d[2] / n]


def _fit(obs, centers, rays):
    """obs: [(v, X, Y)] -> P or None"""
    A = [[0.0, 0.0, 0.0] for _ in range(3)]
    b = [0.0, 0.0, 0.0]
    for v, X, Y in obs:
        r = _ray(rays[v], X, Y)
        c = centers[v]
        for k in range(3):
            a = [(1.0 if k == l else 0.0) - r[k] * r[l] for l in range(3)]
            for l in range(3):
                A[k][l] = A[k][l] + a[l]
            b[k] = b[k] + ((a[0] * c[0] + a[1] * c[1]) + a[2] * c[2])
    det = _det3(A)
    if not det > 0.0:
        return None
    out = []
    for k in range(3):
        m = [[b[r] if l == k else A[r][l] for l in range(3)] for r in range(3)]
        out.append(_det3(m) / det)
    return out


def _reproject(o, P, proj, limit):
    v, X, Y = o
    p = proj[v]
    row = [((p[k, 0] * P[0] + p[k, 1] * P[1]) + p[k, 2] * P[2]) + p[k, 3] * 1.0 for k in range(3)]
    if not row[2] > 0.0:
        return False, 0.0
    du, dv = row[0] / row[2] - X, row[1] / row[2] - Y
    e = np.sqrt(du * du + dv * dv)
    return bool(e <= limit), e


def triangulate_tracks(xy, view_off, tracks, cam_arrays, max_reproj=2.0, min_angle=1.5):
    """cam_arrays: keypoints.camera_arrays(cams).  One short Python loop per track (tracks are few and short)."""
    centers, rays, proj = (np.asarray(a, np.float64) for a in cam_arrays)
    track_off, track_view, track_kp = tracks
    cos_min = np.cos(np.radians(float(min_angle)))                # (host side in the module too: math.cos(math.radians(.)), the same libm call)
    T = len(track_off) - 1
    xyz, error, keep, obs_keep = np.zeros((T, 3)), np.zeros(T), np.zeros(T, bool), np.zeros(len(track_view), bool)
    xy = np.asarray(xy, np.float64)
    for t in range(T):
        q0, q1 = int(track_off[t]), int(track_off[t + 1])
        obs = [(int(track_view[q]), np.float64(xy[view_off[track_view[q]] + track_kp[q], 0]), np.float64(xy[view_off[track_view[q]] + track_kp[q], 1]))
               for q in range(q0, q1)]
        if len(obs) < 2:
            continue
        P = _fit(obs, centers, rays)
        if P is None:
            continue
        ok = [_reproject(o, P, proj, max_reproj)[0] for o in obs]
        if sum(ok) < 2:
            continue
        rest = [o for o, k in zip(obs, ok) if k]
        if len(rest) < len(obs):
            P = _fit(rest, centers, rays)
            if P is None or not all(_reproject(o, P, proj, max_reproj)[0] for o in rest):
                continue
        rr = [_ray(rays[v], X, Y) for v, X, Y in rest]
        if not any((rr[i][0] * rr[j][0] + rr[i][1] * rr[j][1]) + rr[i][2] * rr[j][2] <= cos_min for i in range(len(rr)) for j in range(i + 1, len(rr))):
            continue
        s = 0.0
        for o in rest:
            s = s + _reproject(o, P, proj, max_reproj)[1]
        xyz[t], error[t], keep[t] = P, s / float(len(rest)), True
        obs_keep[q0:q1] = ok
    return xyz, error, keep, obs_keep


def grey(images):
    img = np.asarray(images)
    if img.ndim == 3:
        return img.astype(np.float64)
    if img.dtype == np.uint8:
        q = img.astype(np.int64)
        return (299 * q[..., 0] + 587 * q[..., 1] + 114 * q[..., 2]).astype(np.float64) / 1000.0
    q = img.astype(np.float64)
    return ((299.0 * q[..., 0] + 587.0 * q[..., 1]) + 114.0 * q[..., 2]) / 1000.0


def blur(a, taps):
    """[..., h, w]: rows first (along x), then columns; every sum from 0.0 over the taps left to right, coordinates clamped"""
    r = (len(taps) - 1) // 2
    for axis in (-1, -2):
        n = a.shape[axis]
        out = np.zeros_like(a)
        for k in range(len(taps)):
            c = np.clip(np.arange(n) + k - r, 0, n - 1)
            out = out + taps[k] * np.take(a, c, axis=axis)
        a = out
    return a


def scale_space(images, taps, sizes):
    """taps: keypoints.blur_taps of keypoints.level_sigmas()[1]; sizes: keypoints.octave_sizes -> [(L [V,6,h,w], D [V,5,h,w])]"""
    base, out = grey(images), []
    for o in range(len(sizes)):
        lev = [base if o > 0 else blur(base, taps[0])]
        for s in range(1, len(taps)):
            lev.append(blur(lev[-1], taps[s]))
        L = np.stack(lev, 1)
        out.append((L, L[:, 1:] - L[:, :-1]))
        base = lev[3][:, ::2, ::2]
    return out


def detect_extrema(images, taps, sizes, sigmas, contrast=2.0, edge_ratio=10.0, border=5):
    """sigmas: keypoints.level_sigmas()[0] -> (xy [N,2], scale [N], response [N], site int32 [N,4], view_off) as keypoints.detect_extrema"""
    space = scale_space(images, taps, sizes)
    V = space[0][1].shape[0]
    r = float(edge_ratio)
    per_view = [[] for _ in range(V)]
    for o, (_, D) in enumerate(space):
        h, w = D.shape[2:]
        if h <= 2 * border or w <= 2 * border:
            continue

        def at(ds, dy, dx):
            return D[:, 1 + ds:4 + ds, border + dy:h - border + dy, border + dx:w - border + dx]
        v = at(0, 0, 0)
        gt, lt = np.ones(v.shape, bool), np.ones(v.shape, bool)
        for ds in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if ds or dy or dx:
                        gt &= v > at(ds, dy, dx)
                        lt &= v < at(ds, dy, dx)
        dxx = (at(0, 0, 1) + at(0, 0, -1)) - 2.0 * v
        dyy = (at(0, 1, 0) + at(0, -1, 0)) - 2.0 * v
        dss = (at(1, 0, 0) + at(-1, 0, 0)) - 2.0 * v
        dxy = 0.25 * ((at(0, 1, 1) - at(0, 1, -1)) - (at(0, -1, 1) - at(0, -1, -1)))
        dxs = 0.25 * ((at(1, 0, 1) - at(1, 0, -1)) - (at(-1, 0, 1) - at(-1, 0, -1)))
        dys = 0.25 * ((at(1, 1, 0) - at(1, -1, 0)) - (at(-1, 1, 0) - at(-1, -1, 0)))
        tr, de = dxx + dyy, dxx * dyy - dxy * dxy
        keep = (np.abs(v) > contrast) & (gt | lt) & (de > 0.0) & ((tr * tr) * r < ((r + 1.0) * (r + 1.0)) * de)
        gx, gy, gs = 0.5 * (at(0, 0, 1) - at(0, 0, -1)), 0.5 * (at(0, 1, 0) - at(0, -1, 0)), 0.5 * (at(1, 0, 0) - at(-1, 0, 0))
        det = _det3([[dxx, dxy, dxs], [dxy, dyy, dys], [dxs, dys, dss]])
        with np.errstate(divide='ignore', invalid='ignore'):
            ox = _det3([[-gx, dxy, dxs], [-gy, dyy, dys], [-gs, dys, dss]]) / det
            oy = _det3([[dxx, -gx, dxs], [dxy, -gy, dys], [dxs, -gs, dss]]) / det
            os_ = _det3([[dxx, dxy, -gx], [dxy, dyy, -gy], [dxs, dys, -gs]]) / det
            keep &= (det != 0.0) & np.isfinite(det) & (np.abs(ox) <= 0.5) & (np.abs(oy) <= 0.5) & (np.abs(os_) <= 0.5)
            resp = np.abs(v + 0.5 * ((gx * ox + gy * oy) + gs * os_))
        step = float(2 ** o)
        for view in range(V):
            s_, y_, x_ = np.nonzero(keep[view])                     # C order: (level, y, x)
            xs, ys = (x_ + border).astype(np.float64), (y_ + border).astype(np.float64)
            k = (view, s_, y_, x_)
            xy = np.stack([((xs + ox[k]) + 0.5) * step, ((ys + oy[k]) + 0.5) * step], 1)
            scale = np.asarray(sigmas)[s_ + 1] * step
            site = np.stack([np.full(len(s_), o), s_ + 1, y_ + border, x_ + border], 1).astype(np.int32)
            per_view[view].append((xy, scale, resp[k], site))
    cat = lambda i, shape, dt: np.concatenate([p[i] for pv in per_view for p in pv] + [np.zeros(shape, dt)])   # noqa: E731
    view_off = np.concatenate([[0], np.cumsum([sum(len(p[1]) for p in pv) for pv in per_view])]).astype(np.int64)
    return cat(0, (0, 2), np.float64), cat(1, (0,), np.float64), cat(2, (0,), np.float64), cat(3, (0, 4), np.int32), view_off


TWO_PI = 6.283185307179586


def trig_table():
    """the sine (14) and cosine (15) Taylor coefficients in ascending order, fp64 [29]: keypoints.trig_table restated"""
    out, f = [], 1.0
    fact = [1.0]
    for k in range(1, 30):
        f = f * float(k)
        fact.append(f)
    for k in range(14):
        out.append((1.0 if k % 2 == 0 else -1.0) / fact[2 * k + 1])
    for k in range(15):
        out.append((1.0 if k % 2 == 0 else -1.0) / fact[2 * k])
    return np.array(out, np.float64)


def orientation(L, site, ogauss, oradius, trig):
    """L [V,6,h,w], site [n,4] = (view, level, y, x) -> (angle, cos, sin) [n]"""
    n = len(site)
    h, w = L.shape[2:]
    v_, s_, y_, x_ = (site[:, c].astype(np.int64) for c in range(4))
    og, R = np.asarray(ogauss)[s_ - 1], np.asarray(oradius)[s_ - 1]
    hist = np.zeros((n, 36), np.int64)
    for dy in range(-int(R.max()), int(R.max()) + 1):
        for dx in range(-int(R.max()), int(R.max()) + 1):
            px, py = x_ + dx, y_ + dy
            k = np.nonzero((abs(dy) <= R) & (abs(dx) <= R) & (px >= 1) & (px <= w - 2) & (py >= 1) & (py <= h - 2))[0]
            if not len(k):
                continue
            pxk, pyk, sk, vk = px[k], py[k], s_[k], v_[k]
            gx = L[vk, sk, pyk, pxk + 1] - L[vk, sk, pyk, pxk - 1]
            gy = L[vk, sk, pyk + 1, pxk] - L[vk, sk, pyk - 1, pxk]
            mag = np.sqrt(gx * gx + gy * gy)
            t = atan2_pos(np.abs(gy), gx)
            t = np.where(gy < 0.0, -t, t)
            t = np.where(t < 0.0, t + TWO_PI, t)
            t = np.where(t >= TWO_PI, t - TWO_PI, t)
            b = np.minimum(np.floor(t * 5.729577951308232).astype(np.int64), 35)
            val = mag * expneg(-(float(dx * dx + dy * dy) * og[k]))
            np.add.at(hist, (k, b), rint(val * 4294967296.0).astype(np.int64))
    best = np.argmax(hist, 1)                                     # the first of equal maxima: the lowest bin
    rows = np.arange(n)
    l, c, r = (hist[rows, (best + d) % 36].astype(np.float64) for d in (35, 0, 1))
    den = (l - 2.0 * c) + r
    with np.errstate(divide='ignore', invalid='ignore'):
        p = np.where(den == 0.0, 0.0, (0.5 * (l - r)) / den)
    ang = ((best.astype(np.float64) + 0.5) + p) * 0.17453292519943295
    ang = np.where(ang < 0.0, ang + TWO_PI, ang)
    ang = np.where(ang >= TWO_PI, ang - TWO_PI, ang)
    u = ang - 3.141592653589793
    z = u * u
    ps, pc = np.full(n, trig[13]), np.full(n, trig[28])
    for k in range(12, -1, -1):
        ps = ps * z + trig[k]
    for k in range(13, -1, -1):
        pc = pc * z + trig[14 + k]
    some = hist[rows, best] > 0
    return np.where(some, ang, 0.0), np.where(some, -pc, 1.0), np.where(some, -(u * ps), 0.0)


def describe(L, site, cell, radius, ang=None, co=None, si=None):
    """L [V,6,h,w] of one octave, site int [n,4] = (view, level, y, x), angle with its (cos, sin) per keypoint (None: upright) -> (codes int8 [n,128],
    valid bool [n]); loops over the window offsets, vectorised over the keypoints"""
    n = len(site)
    if ang is None:
        ang, co, si = np.zeros(n), np.ones(n), np.zeros(n)
    h, w = L.shape[2:]
    v_, s_, y_, x_ = (site[:, c].astype(np.int64) for c in range(4))
    hc, R = np.asarray(cell)[s_ - 1], np.asarray(radius)[s_ - 1]
    acc = np.zeros((n, 128), np.int64)
    rows = np.arange(n)
    for dy in range(-int(R.max()), int(R.max()) + 1):
        for dx in range(-int(R.max()), int(R.max()) + 1):
            px, py = x_ + dx, y_ + dy
            ok = (abs(dy) <= R) & (abs(dx) <= R) & (px >= 1) & (px <= w - 2) & (py >= 1) & (py <= h - 2)
            rx, ry = (co * float(dx) + si * float(dy)) / hc, (co * float(dy) - si * float(dx)) / hc
            cx, cy = rx + 1.5, ry + 1.5
            ok &= (cx > -1.0) & (cx < 4.0) & (cy > -1.0) & (cy < 4.0)
            if not ok.any():
                continue
            k = np.nonzero(ok)[0]
            pxk, pyk, sk, vk = px[k], py[k], s_[k], v_[k]
            gx = L[vk, sk, pyk, pxk + 1] - L[vk, sk, pyk, pxk - 1]
            gy = L[vk, sk, pyk + 1, pxk] - L[vk, sk, pyk - 1, pxk]
            mag = np.sqrt(gx * gx + gy * gy)
            t = atan2_pos(np.abs(gy), gx)
            t = np.where(gy < 0.0, -t, t)
            rel = t - ang[k]
            rel = np.where(rel < 0.0, rel + TWO_PI, rel)
            rel = np.where(rel < 0.0, rel + TWO_PI, rel)
            rel = np.where(rel >= TWO_PI, rel - TWO_PI, rel)
            ob = rel * 1.2732395447351628
            val = mag * expneg(-((rx[k] * rx[k] + ry[k] * ry[k]) * 0.125))
            x0, y0, o0 = np.floor(cx[k]), np.floor(cy[k]), np.floor(ob)
            fx, fy, fo = cx[k] - x0, cy[k] - y0, ob - o0
            for q in range(8):
                ix, iy, io = x0.astype(np.int64) + (q & 1), y0.astype(np.int64) + ((q >> 1) & 1), (o0.astype(np.int64) + (q >> 2)) & 7
                inside = (ix >= 0) & (ix <= 3) & (iy >= 0) & (iy <= 3)
                vote = ((val * (fx if q & 1 else 1.0 - fx)) * (fy if q & 2 else 1.0 - fy)) * (fo if q & 4 else 1.0 - fo)
                rq = rint(vote * 4294967296.0).astype(np.int64)
                np.add.at(acc, (k[inside], ((iy * 4 + ix) * 8 + io)[inside]), rq[inside])
    u = acc.astype(np.float64) * 2.3283064365386963e-10
    n1 = np.zeros(n)
    for c in range(128):
        n1 = n1 + u[:, c] * u[:, c]
    n1 = np.sqrt(n1)
    valid = n1 > 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        u = u / n1[:, None]
        u = np.where(u > 0.2, 0.2, u)
        n2 = np.zeros(n)
        for c in range(128):
            n2 = n2 + u[:, c] * u[:, c]
        n2 = np.sqrt(n2)
        f = np.floor(512.0 * (u / n2[:, None]))
    codes = np.where(valid[:, None], np.where(f > 127.0, 127.0, f), 0.0).astype(np.int8)
    return codes, valid


def detect(images, taps, sizes, sigmas, cell, radius, ogauss, oradius, max_keypoints=8192, contrast=2.0, edge_ratio=10.0, upright=False):
    """-> (xy, scale, angle, response, codes, view_off) as keypoints.detect; the tables: keypoints.descriptor_tables()"""
    xy, scale, resp, site, vo = detect_extrema(images, taps, sizes, sigmas, contrast, edge_ratio)
    space = scale_space(images, taps, sizes)
    codes, valid, angle = np.zeros((len(xy), 128), np.int8), np.zeros(len(xy), bool), np.zeros(len(xy))
    view = np.repeat(np.arange(len(vo) - 1), np.diff(vo))
    for o in range(len(sizes)):
        k = np.nonzero(site[:, 0] == o)[0]
        if len(k):
            st = np.concatenate([view[k, None], site[k, 1:]], 1)
            if upright:
                codes[k], valid[k] = describe(space[o][0], st, cell, radius)
            else:
                ang, co, si = orientation(space[o][0], st, ogauss, oradius, trig_table())
                angle[k] = ang
                codes[k], valid[k] = describe(space[o][0], st, cell, radius, ang, co, si)
    k = np.nonzero(valid)[0]
    view_off = np.concatenate([[0], np.cumsum(np.bincount(view[k], minlength=len(vo) - 1))]).astype(np.int64)
    return cap_keypoints((xy[k], scale[k], angle[k], resp[k], codes[k], view_off), max_keypoints)


def cap_keypoints(kp, max_keypoints):
    """per view the first max_keypoints under (response descending, then the order), listed in the order again"""
    vo, resp, keep = kp[5], kp[3], []
    for v in range(len(vo) - 1):
        k = np.arange(vo[v], vo[v + 1])
        if len(k) > max_keypoints:
            k = np.sort(k[np.argsort(-resp[k], kind='stable')[:max_keypoints]])
        keep.append(k)
    view_off = np.concatenate([[0], np.cumsum([len(k) for k in keep])]).astype(np.int64)
    k = np.concatenate(keep).astype(np.int64)
    return tuple(f[k] for f in kp[:5]) + (view_off,)


def sparse_points(images, cams, tables, cam_arrays, F_of, keypoints=None, **kw):
    """tables = (taps, sizes, sigmas, cell, radius, ogauss, oradius); cam_arrays / F_of: keypoints.camera_arrays(cams), keypoints.fundamental_matrices(cams, pairs) ->
    (xyz, rgb, error, track_off, track_view, track_kp, keypoints tuple) as keypoints.sparse_points on equal-sized uint8 images"""
    kp = detect(images, *tables, **kw) if keypoints is None else keypoints     # (keypoints: a detect result of these images, to save the work)
    xy, vo = kp[0], kp[5]
    m = match_descriptors(kp[4], vo)
    v = verify_matches(xy, vo, m, F_of(m[0]))
    tracks = build_tracks(vo, v)
    xyz, error, keep, obs_keep = triangulate_tracks(xy, vo, tracks, cam_arrays)
    T = len(keep)
    owner = np.repeat(np.arange(T), np.diff(tracks[0]))
    counts = np.bincount(owner, weights=obs_keep, minlength=T).astype(np.int64)[keep]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    tv, tk = tracks[1][obs_keep], tracks[2][obs_keep]
    first = off[:-1]
    fxy = xy[vo[tv[first]] + tk[first]]
    img = np.asarray(images)
    rgb = img[tv[first], np.floor(fxy[:, 1]).astype(int), np.floor(fxy[:, 0]).astype(int)]
    return xyz[keep], rgb.astype(np.uint8), error[keep], off, tv, tk, kp
