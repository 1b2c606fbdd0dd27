"""The definition of mvsdf_amd/global_reg.py restated in numpy (fp64, every product and sum a separate numpy operation in the order the definition
writes it; integers exact).  Written from that module's docstring, not from the kernels.  The pair features are vectorised over [N, k], the matcher
over row chunks of the integer distance table, the sampler and the edge test over the hypotheses; each surviving hypothesis is then fitted in Python
floats by registration_ref.horn_update and scored over all correspondences."""
import collections

import numpy as np

import normals_ref as NR
import registration_ref as RR
from viewsel_ref import atan2_pos

PI = 3.141592653589793
BINS = 11
GROUPS = 3
DIM = BINS * GROUPS
GOLDEN = 0x9E3779B97F4A7C15
MIX1 = 0xBF58476D1CE4E5B9
MIX2 = 0x94D049BB133111EB

GlobalRegistration = collections.namedtuple('GlobalRegistration', 'transformation inliers hypothesis checked mask')
GlobalResult = collections.namedtuple('GlobalResult', 'transformation inliers flipped fitness inlier_rmse')


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _r2(radius):
    return np.inf if radius is None else float(radius) * float(radius)


def near_pairs(P, nb, radius=None):
    """-> (near bool [N, k], d2 fp64 [N, k], d = p_j - p_i [N, k, 3])"""
    P = np.ascontiguousarray(P, np.float64)
    j = np.asarray(nb).astype(np.int64)
    d = P[j] - P[:, None, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    near = (j != np.arange(len(P))[:, None]) & (d2 > 0) & (d2 <= _r2(radius))
    return near, d2, d


def pair_features(P, Nrm, nb, radius=None):
    """stage 1 before the binning -> (valid bool [N, k], theta, alpha, phi fp64 [N, k])"""
    Nrm = np.ascontiguousarray(Nrm, np.float64)
    j = np.asarray(nb).astype(np.int64)
    near, d2, d = near_pairs(P, nb, radius)
    with np.errstate(all='ignore'):
        dn = d / np.sqrt(d2)[..., None]
        ni = np.broadcast_to(Nrm[:, None, :], dn.shape)
        nj = Nrm[j]
        a1, a2 = dot3(ni, dn), dot3(nj, dn)
        sw = (np.abs(a1) < np.abs(a2))[..., None]
        u = np.where(sw, nj, ni)
        nt = np.where(sw, ni, nj)
        dn = np.where(sw, -dn, dn)
        phi = dot3(u, dn)
        v = cross3(dn, u)
        ln = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
        valid = near & (ln > 0)
        v = v / ln[..., None]
        w = cross3(u, v)
        alpha = dot3(v, nt)
        y, x = dot3(w, nt), dot3(u, nt)
        theta = atan2_pos(np.abs(y), np.where(valid, x, 1.0))
        theta = np.where(y < 0, -theta, theta)
    return valid, theta, alpha, phi


def bin_position(f, lo, hi):
    """11 * ((f - lo) / (hi - lo)): the bin is its floor, clamped"""
    with np.errstate(all='ignore'):
        return BINS * ((f - lo) / (hi - lo))


def bin_of(f, lo, hi):
    with np.errstate(all='ignore'):
        b = np.floor(bin_position(f, lo, hi))
    b = np.where(b >= 0, b, 0.0)                                             # (a NaN counts as bin 0)
    return np.where(b > BINS - 1, BINS - 1, b).astype(np.int64)


def spfh(P, Nrm, nb, radius=None):
    """stage 1 -> (hist int32 [N, 33], count int32 [N])"""
    valid, theta, alpha, phi = pair_features(P, Nrm, nb, radius)
    n = len(valid)
    hist = np.zeros((n, DIM), np.int32)
    rows = np.broadcast_to(np.arange(n)[:, None], valid.shape)
    for g, b in enumerate((bin_of(theta, -PI, PI), bin_of(alpha, -1.0, 1.0), bin_of(phi, -1.0, 1.0))):
        np.add.at(hist, (rows[valid], BINS * g + b[valid]), 1)
    return hist, valid.sum(1).astype(np.int32)


def fpfh(P, nb, hist, count, radius=None):
    """stage 2 -> (features fp64 [N, 33], codes int8 [N, 33])"""
    j = np.asarray(nb).astype(np.int64)
    near, d2, _ = near_pairs(P, nb, radius)
    hist, count = np.asarray(hist), np.asarray(count)
    acc = np.zeros((len(j), DIM))
    with np.errstate(all='ignore'):
        for t in range(j.shape[1]):
            jt = j[:, t]
            on = near[:, t] & (count[jt] > 0)
            term = (1.0 / d2[:, t])[:, None] * (hist[jt].astype(np.float64) / count[jt].astype(np.float64)[:, None])
            acc = acc + np.where(on[:, None], term, 0.0)
        out = np.zeros_like(acc)
        for g in range(GROUPS):
            s = np.zeros(len(j))
            for c in range(BINS * g, BINS * g + BINS):
                s = s + acc[:, c]
            for c in range(BINS * g, BINS * g + BINS):
                out[:, c] = np.where(s > 0, 100.0 * acc[:, c] / s, 0.0)
    codes = np.minimum(127.0, np.floor(out * 1.27)).astype(np.int8)
    return out, codes


def mirror_codes(codes):
    codes = np.asarray(codes)
    out = codes.copy()
    out[:, 0:BINS] = codes[:, 0:BINS][:, ::-1]
    out[:, 2 * BINS:3 * BINS] = codes[:, 2 * BINS:3 * BINS][:, ::-1]
    return out


def _match_one(s, t, chunk=2048):
    """exact integers: sum (s - t)^2 = |s|^2 + |t|^2 - 2 s . t (tests/test_global_reg_host.py holds this to the plain double loop)"""
    s, t = np.asarray(s).astype(np.int64), np.asarray(t).astype(np.int64)
    index = np.empty(len(s), np.int32)
    dist = np.empty(len(s), np.int32)
    tn = (t * t).sum(1)
    for lo in range(0, len(s), chunk):
        sc = s[lo:lo + chunk]
        D = (sc * sc).sum(1)[:, None] + tn[None, :] - 2 * (sc @ t.T)
        j = D.argmin(1)                                                      # the first minimum: the smallest j
        index[lo:lo + chunk] = j
        dist[lo:lo + chunk] = D[np.arange(len(j)), j]
    return index, dist


def match_features(src_codes, dst_codes, mutual=False):
    """stage 3 -> (index int32 [Ns], dist int32 [Ns])"""
    for c in (src_codes, dst_codes):
        c = np.asarray(c)
        if c.dtype != np.int8 or c.ndim != 2 or c.shape[1] != DIM or len(c) == 0 or c.min() < 0:
            raise ValueError('codes must be int8 [N >= 1, 33] in 0 .. 127')
    index, dist = _match_one(src_codes, dst_codes)
    if mutual:
        back, _ = _match_one(dst_codes, src_codes)
        index = np.where(back[index] == np.arange(len(index)), index, -1).astype(np.int32)
    return index, dist


# ================================================================ the hypothesis search ================================================================
def sample_indices(seed, h, M):
    """the three correspondence indices of the hypotheses h -> int64 [len(h), 3]"""
    h = np.asarray(h).astype(np.uint64)
    out = []
    with np.errstate(over='ignore'):
        for t in range(3):
            x = np.uint64(seed) ^ ((np.uint64(3) * h + np.uint64(t)) * np.uint64(GOLDEN))
            x = x ^ (x >> np.uint64(30))
            x = x * np.uint64(MIX1)
            x = x ^ (x >> np.uint64(27))
            x = x * np.uint64(MIX2)
            x = x ^ (x >> np.uint64(31))
            out.append(((x >> np.uint64(32)) * np.uint64(M)) >> np.uint64(32))
    return np.stack(out, 1).astype(np.int64)


def correspondences(corr):
    """[M, 2] as given, or an index array with its -1 entries dropped in order"""
    c = np.asarray(corr)
    if c.ndim == 1:
        keep = np.flatnonzero(c >= 0)
        c = np.stack([keep, c[keep]], 1)
    return c.astype(np.int64)


def fit3(s, t):
    """the fit of three pairs (s, t: three points each, Python floats) -> T as rows of Python floats, or None where a step is not a number"""
    c = t[0]
    p = [[s[i][a] - c[a] for a in range(3)] for i in range(3)]
    q = [[t[i][a] - c[a] for a in range(3)] for i in range(3)]
    sp, sq, spq = [0.0] * 3, [0.0] * 3, [0.0] * 9
    for i in range(3):
        for a in range(3):
            sp[a] = sp[a] + p[i][a]
            sq[a] = sq[a] + q[i][a]
            for b in range(3):
                spq[3 * a + b] = spq[3 * a + b] + p[i][a] * q[i][b]
    try:
        return RR.horn_update(3, [0.0] + sp + sq + spq, c)
    except (ZeroDivisionError, OverflowError, ValueError):
        return None


def ransac(src, dst, corr, max_dist, hypotheses=100000, seed=0, edge_ratio=0.9):
    """stage 4 -> GlobalRegistration(transformation fp64 [4, 4], inliers, hypothesis, checked, mask bool [M])"""
    src, dst = np.ascontiguousarray(src, np.float64), np.ascontiguousarray(dst, np.float64)
    corr = correspondences(corr)
    M = len(corr)
    if M < 3:
        raise ValueError('at least 3 correspondences')
    a, b = corr[:, 0], corr[:, 1]
    S, D = src[a], dst[b]
    md2 = float(max_dist) * float(max_dist)
    m = sample_indices(seed, np.arange(hypotheses), M)
    ok = np.ones(hypotheses, bool)
    for u, v in ((0, 1), (0, 2), (1, 2)):
        ok &= (m[:, u] != m[:, v]) & (a[m[:, u]] != a[m[:, v]]) & (b[m[:, u]] != b[m[:, v]])
    for u, v in ((0, 1), (0, 2), (1, 2)):
        ls = np.sqrt(RR.d2(S[m[:, u]], S[m[:, v]]))
        lt = np.sqrt(RR.d2(D[m[:, u]], D[m[:, v]]))
        ok &= (ls >= edge_ratio * lt) & (lt >= edge_ratio * ls)
    best = (0, -1, None, None)
    checked = 0
    for h in np.flatnonzero(ok).tolist():
        s = [[float(x) for x in S[i]] for i in m[h]]
        t = [[float(x) for x in D[i]] for i in m[h]]
        T = fit3(s, t)
        if T is None:
            continue
        T = np.array(T, np.float64)
        with np.errstate(all='ignore'):
            if not (RR.d2(RR.transform_points(S[m[h]], T), D[m[h]]) < md2).all():
                continue
            checked += 1
            inl = RR.d2(RR.transform_points(S, T), D) < md2
        cnt = int(inl.sum())
        if cnt > best[0]:                                                    # ascending h: the first of the largest count
            best = (cnt, h, T, inl)
    if best[1] < 0:
        return GlobalRegistration(np.eye(4), 0, -1, checked, np.zeros(M, bool))
    return GlobalRegistration(best[2], best[0], best[1], checked, best[3])


# ================================================================ the composed call ================================================================
def describe(P, given, voxel, k, radius, jobs=1):
    """downsample, normals, descriptor -> (points, normals, codes)"""
    P = np.ascontiguousarray(P, np.float64)
    ds = RR.voxel_downsample(P, voxel)[0]
    if given is None:
        nrm, _, nb = NR.estimate_normals(ds, k, jobs=jobs)
        nrm = NR.orient_normals(ds, nrm, nb)[0]
    else:
        nrm = np.ascontiguousarray(given, np.float64)[RR.nearest(ds, P)[1]]
        nb = NR.knn_indices(ds, k, jobs=jobs)[0]
    hist, count = spfh(ds, nrm, nb, radius)
    return ds, nrm, fpfh(ds, nb, hist, count, radius)[1]


def global_register(source, target, voxel, source_normals=None, target_normals=None, k=32, feature_radius=None, max_dist=None, hypotheses=100000,
                    seed=0, mutual=False, flip='auto', refine=True, jobs=1):
    radius = 5 * voxel if feature_radius is None else feature_radius
    max_dist = 1.5 * voxel if max_dist is None else max_dist
    s, _, sc = describe(source, source_normals, voxel, k, radius, jobs)
    t, _, tc = describe(target, target_normals, voxel, k, radius, jobs)
    runs = []
    for mirrored in {'auto': (False, True), False: (False,), True: (True,)}[flip]:
        index, _ = match_features(mirror_codes(sc) if mirrored else sc, tc, mutual)
        if (index >= 0).sum() >= 3:
            runs.append((ransac(s, t, index, max_dist, hypotheses, seed), mirrored))
    if not runs:
        raise ValueError('fewer than 3 correspondences')
    reg, flipped = runs[0]
    for r, f in runs[1:]:
        if r.inliers > reg.inliers:
            reg, flipped = r, f
    if not refine:
        return GlobalResult(reg.transformation, reg.inliers, flipped, None, None), reg
    T, fitness, rmse, _ = RR.icp(s, t, reg.transformation, max_dist)
    return GlobalResult(T, reg.inliers, flipped, fitness, rmse), reg


# ================================================================ the synthetic scene of the tests ================================================================
RADII = np.array([1.0, 0.8, 0.6])
# seven bumps: direction (normalised below), height, angular width
BUMPS = [((1.0, 0.2, 0.1), 0.22, 0.30), ((-0.3, 1.0, 0.4), 0.18, 0.25), ((0.2, -0.4, 1.0), 0.25, 0.35), ((-1.0, -0.5, 0.3), -0.15, 0.30),
         ((0.6, 0.7, -0.6), 0.20, 0.22), ((0.1, -1.0, -0.3), 0.16, 0.28), ((-0.5, 0.3, -1.0), -0.12, 0.33)]
MOTION_AXIS, MOTION_DEGREES, MOTION_SHIFT = (1.0, 2.0, 3.0), 170.0, (0.7, -1.3, 2.1)


def ellipsoid(dirs):
    """the surface point along each unit direction: an ellipsoid whose radius is modulated by seven Gaussian bumps of the angle"""
    r = np.ones(len(dirs))
    for c, height, width in BUMPS:
        c = np.asarray(c) / np.linalg.norm(c)
        ang = np.arccos(np.clip(dirs @ c, -1.0, 1.0))
        r = r + height * np.exp(-(ang * ang) / (2 * width * width))
    return dirs * r[:, None] * RADII[None, :]


def scene(seed, n_source=1700, n_target=1500):
    """-> (source [about 0.65 n_source, 3]: one sampling, the part of the surface with direction . (1, 1, 1) / sqrt 3 > -0.25; target [n_target, 3]:
    another sampling of the whole surface, moved; the motion fp64 [4, 4] source frame -> target frame).  No point exists twice."""
    rs = np.random.RandomState(1000 + seed)
    a = rs.normal(size=(n_source, 3))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    a = a[a @ (np.ones(3) / np.sqrt(3.0)) > -0.25]
    b = rs.normal(size=(n_target, 3))
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    motion = RR.rigid(MOTION_AXIS, MOTION_DEGREES, MOTION_SHIFT)
    return ellipsoid(a), RR.transform_points(ellipsoid(b), motion), motion


def motion_errors(T, motion):
    """(rotation error in degrees, translation error: the distance between the images of the source's origin-side centre (0, 0, 0))"""
    return RR.angle_between(T, motion), float(np.linalg.norm(np.asarray(T)[:3, 3] - motion[:3, 3]))
