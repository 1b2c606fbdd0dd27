"""numpy restatement of mvsdf_amd/registration.py's definitions (its docstring numbers them): fp64, every product and sum in the written order.
The device results are compared with these bit for bit.  nearest() narrows the candidates by a window over the sorted x coordinates before it applies
the definition; tests/test_registration_host.py holds it to the plain O(NQ) argmin."""
import math

import numpy as np

CHUNK, THREADS, ITEMS, TOP = 2048, 256, 8, 1024
SWEEPS = 16
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
IDENTITY = np.eye(4)


def d2(q, r):
    d = q - r
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _finish(m, idx, max_dist):
    dist = np.sqrt(m)
    hit = dist < max_dist
    return np.where(hit, dist, np.inf), np.where(hit, idx, -1).astype(np.int32), np.where(hit, m, np.inf)


def nearest_brute(q, r, max_dist=np.inf):
    """definition 1 by the O(NQ) table -> (dist, index, d2)"""
    q, r = np.asarray(q, np.float64).reshape(-1, 3), np.asarray(r, np.float64).reshape(-1, 3)
    D = d2(q[:, None, :], r[None, :, :])
    m = D.min(1) if len(q) else np.zeros(0)
    idx = np.array([np.flatnonzero(D[i] == m[i])[0] for i in range(len(q))], dtype=np.int64).reshape(-1)
    return _finish(m, idx, max_dist)


def nearest(q, r, max_dist=np.inf, chunk=256):
    """definition 1 -> (dist fp64 [Q], index int32 [Q], d2 fp64 [Q]).  Candidates: the references whose x lies within the distance of the best of
    eight neighbours in x order (a superset of every reference at the minimum); over them the definition's formula and tie rule."""
    q, r = np.asarray(q, np.float64).reshape(-1, 3), np.asarray(r, np.float64).reshape(-1, 3)
    if not (np.isfinite(q).all() and np.isfinite(r).all()):
        raise ValueError('a coordinate is NaN or infinite')
    R = len(r)
    order = np.argsort(r[:, 0], kind='stable')
    rs, xs = r[order], r[order, 0]
    m_all, i_all = np.empty(len(q)), np.empty(len(q), np.int64)
    big = np.iinfo(np.int64).max
    if len(q) == 0:
        return _finish(m_all, i_all, max_dist)
    # an upper bound of the minimum: the formula at some reference -- the best of eight neighbours in x order, and (if scipy is there) at the k-d
    # tree's answer, which only has to be near the minimum, not at it
    cand = np.clip(np.searchsorted(xs, q[:, 0])[:, None] + np.arange(-4, 4)[None, :], 0, R - 1)
    with np.errstate(over='ignore'):
        ub = d2(q[:, None, :], rs[cand]).min(1)
        try:
            from scipy.spatial import cKDTree
            ub = np.minimum(ub, d2(q, r[cKDTree(r).query(q)[1]]))
        except ImportError:
            pass
        rad = np.sqrt(ub) * (1 + 1e-9) + 4 * np.spacing(np.abs(q[:, 0]))
    lo_all = np.searchsorted(xs, q[:, 0] - rad, 'left')
    hi_all = np.searchsorted(xs, q[:, 0] + rad, 'right')
    by_len = np.argsort(hi_all - lo_all, kind='stable')          # chunks of similar window length
    s = 0
    while s < len(q):
        width = max(1, int((hi_all - lo_all)[by_len[min(len(q), s + chunk) - 1]]))
        sel = by_len[s:s + max(1, min(chunk, 2 ** 20 // width))]
        s += len(sel)
        qc, lo, hi = q[sel], lo_all[sel], hi_all[sel]
        idx = lo[:, None] + np.arange(max(1, int((hi - lo).max())))[None, :]
        valid = idx < hi[:, None]
        idx = np.minimum(idx, R - 1)
        with np.errstate(over='ignore'):
            D = np.where(valid, d2(qc[:, None, :], rs[idx]), np.inf)
        m = D.min(1)
        m_all[sel] = m
        i_all[sel] = np.where((D == m[:, None]) & valid, order[idx], big).min(1)
    return _finish(m_all, i_all, max_dist)


def transform_points(p, T):
    p, T = np.asarray(p, np.float64).reshape(-1, 3), np.asarray(T, np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], 1)


AXES = {'X': (1, 2, 0), 'Y': (0, 2, 1), 'Z': (0, 1, 2)}


def crop_volume(p, axis, axis_min, axis_max, polygon):
    """definition 3 -> keep bool [N]"""
    p, P = np.asarray(p, np.float64).reshape(-1, 3), np.asarray(polygon, np.float64)
    u, v, w = AXES[axis.upper()] if isinstance(axis, str) else AXES['XYZ'[axis]]
    pu, pv = p[:, u], p[:, v]
    odd = np.zeros(len(p), bool)
    n = len(P)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        for i in range(n):
            j = (i + 1) % n
            c1 = ((P[i, v] < pv) & (P[j, v] >= pv)) | ((P[j, v] < pv) & (P[i, v] >= pv))
            c2 = P[i, u] + (pv - P[i, v]) / (P[j, v] - P[i, v]) * (P[j, u] - P[i, u]) < pu
            odd ^= c1 & c2
    return (p[:, w] >= axis_min) & (p[:, w] <= axis_max) & odd


def voxel_downsample(p, voxel):
    """definition 4 -> (means fp64 [M, 3], counts int32 [M])"""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    if not np.isfinite(p).all():
        raise ValueError('a coordinate is NaN or infinite')
    o = p.min(0) - voxel / 2
    g = np.floor((p - o) / voxel)
    if (g >= 2 ** 21).any():
        raise ValueError('2^21 or more voxels on an axis')
    g = g.astype(np.uint64)
    key = g[:, 0] | g[:, 1] << np.uint64(21) | g[:, 2] << np.uint64(42)
    order = np.argsort(key, kind='stable')
    ks = key[order]
    heads = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    counts = np.diff(np.r_[heads, len(p)])
    s = np.zeros((len(heads), 3))
    for j in range(int(counts.max())):                           # the j-th point of every voxel that has one: ascending input index
        sel = np.flatnonzero(counts > j)
        s[sel] = s[sel] + p[order[heads[sel] + j]]
    return s / counts[:, None].astype(np.float64), counts.astype(np.int32)


def uniform_downsample(p, k):
    return np.asarray(p, np.float64)[::k]


# ---------------------------------------------------------------- the sums ----------------------------------------------------------------
def _halve(x):
    """the halving tree over the last axis (a power of two): lane t += lane t + w, w = half .. 1 -> lane 0"""
    x = x.copy()
    w = x.shape[-1] // 2
    while w:
        x[..., :w] = x[..., :w] + x[..., w:2 * w]
        w //= 2
    return x[..., 0]


def fixed_sum(v):
    """the sum of v [N] (zeros where an item is skipped) in the device's order (definition 5)"""
    v = np.asarray(v)
    nb = max(1, -(-len(v) // CHUNK))
    a = np.zeros(nb * CHUNK, v.dtype)
    a[:len(v)] = v
    a = a.reshape(nb, THREADS, ITEMS)
    lane = np.zeros((nb, THREADS), v.dtype)
    for k in range(ITEMS):
        lane = lane + a[:, :, k]
    part = _halve(lane)
    per = -(-nb // TOP)
    b = np.zeros(TOP * per, v.dtype)
    b[:nb] = part
    b = b.reshape(TOP, per)
    top = np.zeros(TOP, v.dtype)
    for k in range(per):
        top = top + b[:, k]
    return _halve(top)


def box_centre(r):
    r = np.asarray(r, np.float64).reshape(-1, 3)
    return (r.min(0) + r.max(0)) * 0.5


def pair_sums(src, refs, T, max_dist):
    """one evaluation of definition 5 -> (n, [sum d2, sum p [3], sum q [3], sum p_a q_b [9]], d2 [S], index [S])"""
    src, refs = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(refs, np.float64).reshape(-1, 3)
    c = box_centre(refs)
    moved = transform_points(src, T)
    _, index, dd = nearest(moved, refs, max_dist)
    ok = index >= 0
    p = moved - c
    q = refs[np.maximum(index, 0)] - c
    cols = [dd] + [p[:, a] for a in range(3)] + [q[:, a] for a in range(3)] + [p[:, a] * q[:, b] for a in range(3) for b in range(3)]
    sums = [float(fixed_sum(np.where(ok, col, 0.0))) for col in cols]
    return int(fixed_sum(ok.astype(np.int64))), sums, dd, index


# ---------------------------------------------------------------- Horn's closed form in Python floats ----------------------------------------------------------------
def compose(U, T):
    out = []
    for a in range(3):
        out.append([((U[a][0] * T[0][b] + U[a][1] * T[1][b]) + U[a][2] * T[2][b]) + U[a][3] * T[3][b] for b in range(4)])
    return out + [[0.0, 0.0, 0.0, 1.0]]


def _rotate(X, p, q, c, s, columns):
    for k in range(4):
        if columns:
            xp, xq = X[k][p], X[k][q]
            X[k][p] = c * xp - s * xq
            X[k][q] = s * xp + c * xq
        else:
            xp, xq = X[p][k], X[q][k]
            X[p][k] = c * xp - s * xq
            X[q][k] = s * xp + c * xq


def horn_rotation(M):
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = M
    A = [[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
         [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
         [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
         [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]]
    V = [[float(a == b) for b in range(4)] for a in range(4)]
    for _ in range(SWEEPS):
        for p, q in PAIRS:
            if A[p][q] == 0.0:
                continue
            theta = (A[q][q] - A[p][p]) / (2 * A[p][q])
            t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1))
            c = 1 / math.sqrt(t * t + 1)
            s = t * c
            _rotate(A, p, q, c, s, True)
            _rotate(A, p, q, c, s, False)
            _rotate(V, p, q, c, s, True)
            A[p][q] = A[q][p] = 0.0
    m = 0
    for k in (1, 2, 3):
        if A[k][k] > A[m][m]:
            m = k
    w, x, y, z = (V[k][m] for k in range(4))
    nrm = math.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / nrm, x / nrm, y / nrm, z / nrm
    if w < 0:
        w, x, y, z = -w, -x, -y, -z
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]


def horn_update(n, sums, centre):
    sp, sq, spq = sums[1:4], sums[4:7], sums[7:16]
    M = [[spq[3 * a + b] - (sp[a] * sq[b]) / n for b in range(3)] for a in range(3)]
    R = horn_rotation(M)
    pm = [sp[a] / n + centre[a] for a in range(3)]
    qm = [sq[a] / n + centre[a] for a in range(3)]
    U = []
    for a in range(3):
        U.append(R[a] + [qm[a] - ((R[a][0] * pm[0] + R[a][1] * pm[1]) + R[a][2] * pm[2])])
    return U + [[0.0, 0.0, 0.0, 1.0]]


def _rows(T):
    return [[float(x) for x in row] for row in np.asarray(T, np.float64)]


def icp(source, refs, init=IDENTITY, max_dist=np.inf, max_iter=20, rel_fitness=1e-6, rel_rmse=1e-6):
    """definition 5 -> (transformation fp64 [4, 4], fitness, inlier_rmse, iterations)"""
    source = np.asarray(source, np.float64).reshape(-1, 3)
    centre = [float(x) for x in box_centre(refs)]
    T = _rows(init)

    def evaluate(T):
        n, s, _, _ = pair_sums(source, refs, np.array(T), max_dist)
        if n == 0:
            raise ValueError('no pairs')
        return n, s, n / len(source), math.sqrt(s[0] / n)
    n, s, fitness, rmse = evaluate(T)
    iterations = 0
    for _ in range(max_iter):
        T = compose(horn_update(n, s, centre), T)
        iterations += 1
        n, s, f2, r2 = evaluate(T)
        done = abs(f2 - fitness) < rel_fitness and abs(r2 - rmse) < rel_rmse
        fitness, rmse = f2, r2
        if done:
            break
    return np.array(T, np.float64), fitness, rmse, iterations


# ---------------------------------------------------------------- the score ----------------------------------------------------------------
def edges(tau, stretch=5, bins_per_tau=100):
    return np.array([tau * k / bins_per_tau for k in range(stretch * bins_per_tau + 1)], np.float64)


def histogram(d, e):
    nb = len(e) - 1
    b = (e[1:][None, :] <= d[:, None]).sum(1)
    return np.bincount(b[b < nb], minlength=nb).astype(np.int64)


def fscore(rec, gt, tau, stretch=5, bins_per_tau=100):
    rec, gt = np.asarray(rec, np.float64), np.asarray(gt, np.float64)
    d_rec, d_gt = nearest(rec, gt)[0], nearest(gt, rec)[0]
    e = edges(tau, stretch, bins_per_tau)
    below_rec, below_gt = int((d_rec < tau).sum()), int((d_gt < tau).sum())
    P, R = below_rec / len(rec), below_gt / len(gt)
    return {'precision': P, 'recall': R, 'fscore': 2 * P * R / (P + R) if P + R > 0 else 0.0, 'below_rec': below_rec, 'below_gt': below_gt,
            'hist_rec': histogram(d_rec, e), 'hist_gt': histogram(d_gt, e), 'edges': e, 'dist_rec': d_rec, 'dist_gt': d_gt}


def tnt_stages(tau, max_points):
    return [('voxel', tau, 80 * tau), ('voxel', tau / 2, 20 * tau), ('uniform', max_points, 2 * tau)]


def _filter(p, kind, value):
    if kind == 'voxel':
        return voxel_downsample(p, value)[0]
    return p[::max(1, -(-len(p) // int(value)))]


def tnt_evaluate(rec, gt, crop, init, tau, stages=None, max_points=4000000, max_iter=20):
    """definition 7 -> dict like the module's"""
    rec, gt = np.asarray(rec, np.float64), np.asarray(gt, np.float64)
    c = (crop['orthogonal_axis'], crop['axis_min'], crop['axis_max'], np.asarray(crop['bounding_polygon'], np.float64))
    T = _rows(init)
    G = gt[crop_volume(gt, *c)]
    counts = [len(rec), len(gt), len(G)]
    for kind, value, max_dist in (tnt_stages(tau, max_points) if stages is None else stages):
        S = transform_points(rec, np.array(T))
        S = S[crop_volume(S, *c)]
        s, t = _filter(S, kind, value), _filter(G, kind, value)
        counts += [len(S), len(s), len(t)]
        U = icp(s, t, IDENTITY, max_dist, max_iter)[0]
        T = compose(_rows(U), T)
    S = transform_points(rec, np.array(T))
    S = S[crop_volume(S, *c)]
    s, t = voxel_downsample(S, tau / 2)[0], voxel_downsample(G, tau / 2)[0]
    counts += [len(S), len(s), len(t)]
    f = fscore(s, t, tau)
    return {'precision': f['precision'], 'recall': f['recall'], 'fscore': f['fscore'], 'transformation': np.array(T, np.float64),
            'histograms': (f['hist_rec'], f['hist_gt']), 'edges': f['edges'], 'points': counts, 'below_rec': f['below_rec'], 'below_gt': f['below_gt']}


# ---------------------------------------------------------------- the synthetic scene of the tests ----------------------------------------------------------------
def height_field(xy):
    x, y = xy[:, 0], xy[:, 1]
    return 0.25 * np.sin(2.3 * x + 0.4) * np.cos(1.7 * y - 0.3) + 0.1 * np.sin(5.1 * x * y + 1.0) + 0.06 * np.cos(7.0 * x - 3.0 * y)


def surface(n, seed):
    """n points of a bumpy height field over [-1, 1]^2"""
    xy = np.random.RandomState(seed).uniform(-1, 1, (n, 2))
    return np.concatenate([xy, height_field(xy)[:, None]], 1)


def rotation(axis, degrees):
    """Rodrigues' formula (for the known answers of the tests; no definition depends on it)"""
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = np.radians(degrees)
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def rigid(axis, degrees, t):
    T = np.eye(4)
    T[:3, :3] = rotation(axis, degrees)
    T[:3, 3] = t
    return T


def angle_between(Ra, Rb):
    """the rotation angle of Ra Rb^T in degrees: |Ra - Rb|_F = 2 sqrt(2) sin(angle / 2), which resolves small angles (arccos of the trace does not)"""
    f = np.linalg.norm(np.asarray(Ra)[:3, :3] - np.asarray(Rb)[:3, :3])
    return float(np.degrees(2 * np.arcsin(min(1.0, f / (2 * math.sqrt(2))))))
