"""The numpy restatement of mvsdf_amd/viewsel.py's definition, operation for operation (every line is one correctly rounded fp64 operation, so the
bits equal those of csrc/det_math64.h + csrc/viewsel.hip on the host and on the device), and a second restatement of theta and w through
np.arctan2 / np.exp for the accuracy condition.  Not a test module."""
import numpy as np

MAGIC = 6755399441055744.0                    # 1.5 * 2^52
TAN_PI_8 = 0.41421356237309503
PI, PI_2, PI_4 = 3.141592653589793, 1.5707963267948966, 0.7853981633974483
DEG = 57.29577951308232
LOG2E = 1.4426950408889634
LN2_HI = float.fromhex('0x1.62e42fee00000p-1')
LN2_LO = 1.9082149292705877e-10
EXP_MIN = -708.0
TWO32 = 4294967296.0
DBL_MAX = np.finfo(np.float64).max


def _f(x):
    return np.asarray(x, dtype=np.float64)


def rint(x):
    t = _f(x) + MAGIC
    return t - MAGIC


def atan2_pos(y, x):
    """dm64_atan2_pos: y >= 0 -> radians in [0, pi]"""
    y, x = np.broadcast_arrays(_f(y), _f(x))
    ax = np.where(x < 0.0, -x, x)
    zero = (y == 0.0) & (ax == 0.0)
    swap = y > ax
    num = np.where(swap, ax, y)
    den = np.where(zero, 1.0, np.where(swap, y, ax))
    z = num / den
    hi = z > TAN_PI_8
    z = np.where(hi, (z - 1.0) / (z + 1.0), z)
    z2 = z * z
    p = np.full(z.shape, -1.0 / 39.0)
    for k in range(37, 0, -2):                                  # 1/37, -1/35, ..., -1/3, 1
        c = (1.0 if (k // 2) % 2 == 0 else -1.0) / float(k)
        p = p * z2 + c
    r = z * p
    r = np.where(hi, PI_4 + r, r)
    r = np.where(swap, PI_2 - r, r)
    r = np.where(x < 0.0, PI - r, r)
    return np.where(zero, 0.0, r)


def expneg(x):
    """dm64_expneg: x <= 0 (clamped at -708) -> exp(x)"""
    shape = np.shape(x)
    x = np.atleast_1d(_f(x))                                      # (numpy scalars would warn about the wrap-around of the integer sum below)
    x = np.where(x > EXP_MIN, x, EXP_MIN)
    n = rint(x * LOG2E)
    r = (x - n * LN2_HI) - n * LN2_LO
    fact = 87178291200.0                                        # 14!
    p = np.full(x.shape, 1.0 / fact)
    for k in range(13, 2, -1):                                  # 1/13!, ..., 1/3!
        fact = fact / float(k + 1)
        p = p * r + 1.0 / fact
    p = p * r + 0.5
    p = p * r + 1.0
    p = p * r + 1.0
    bits = p.view(np.uint64) + (n.astype(np.int64).astype(np.uint64) << np.uint64(52))
    return bits.view(np.float64).reshape(shape)


def unit(d):
    """vs_unit: d [..., 3] -> the unit vectors, 0 where the norm is not a positive finite double"""
    d = _f(d)
    with np.errstate(over='ignore', under='ignore'):
        n = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    ok = (n > 0.0) & (n <= DBL_MAX)
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        u = d / np.where(ok, n, 1.0)[..., None]
    return np.where(ok[..., None], u, 0.0)


def theta_units(a, b):
    """vs_theta of unit vectors a, b [..., 3] -> degrees"""
    cx = a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1]
    cy = a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2]
    cz = a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
    nc = np.sqrt((cx * cx + cy * cy) + cz * cz)
    dt = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    return DEG * atan2_pos(nc, dt)


def weight(theta, theta0=5.0, s1=1.0, s2=10.0):
    d = theta - theta0
    s = np.where(theta <= theta0, s1, s2)
    q = (d * d) / (2.0 * (s * s))
    return expneg(-q)


def quantise(w):
    return rint(w * TWO32).astype(np.int64)


def theta_wq(a, b, theta0=5.0, s1=1.0, s2=10.0):
    """(theta, wq) of vectors a = c_i - p, b = c_j - p [n, 3]: what mvsdf_viewsel_weights_host returns"""
    th = theta_units(unit(a), unit(b))
    return th, quantise(weight(th, theta0, s1, s2))


def theta_w_libm(a, b, theta0=5.0, s1=1.0, s2=10.0):
    """the same through np.arctan2 / np.exp on the raw vectors (no normalisation): the yardstick of the accuracy condition"""
    a, b = _f(a), _f(b)
    c = np.cross(a, b)
    th = np.degrees(np.arctan2(np.sqrt((c * c).sum(-1)), (a * b).sum(-1)))
    return th, weight_libm(th, theta0, s1, s2)


def weight_libm(theta, theta0=5.0, s1=1.0, s2=10.0):
    s = np.where(theta <= theta0, s1, s2)
    return np.exp(-(theta - theta0) ** 2 / (2.0 * s * s))


def dense_from_tracks(track_off, track_view, V):
    P = len(track_off) - 1
    vis = np.zeros((V, P), bool)
    for p in range(P):
        vis[track_view[track_off[p]:track_off[p + 1]], p] = True
    return vis


def view_scores(points, centers, vis, theta0=5.0, s1=1.0, s2=10.0):
    """vis bool [V, P] -> (scores fp64 [V, V], counts int64 [V, V]) by the definition"""
    points, centers, vis = _f(points).reshape(-1, 3), _f(centers), np.asarray(vis).astype(bool)
    V = len(centers)
    S = np.zeros((V, V), np.int64)
    counts = vis.astype(np.int64) @ vis.astype(np.int64).T if points.shape[0] else np.zeros((V, V), np.int64)
    U = unit(centers[:, None, :] - points[None, :, :])                       # [V, P, 3]: one unit vector per view and point, as the kernel forms them
    for i in range(V - 1):
        th = theta_units(U[i][None], U[i + 1:])                               # a = the view of the lower index
        wq = quantise(weight(th, theta0, s1, s2))
        S[i, i + 1:] = np.where(vis[i][None] & vis[i + 1:], wq, 0).sum(1)
        S[i + 1:, i] = S[i, i + 1:]
    return S.astype(np.float64) * 2.0 ** -32, counts


def select_pairs(scores, counts, num_pairs=10):
    pairs, pair_scores = [], []
    V = len(scores)
    for i in range(V):
        cand = [j for j in range(V) if j != i and counts[i, j] > 0]
        cand.sort(key=lambda j: (-scores[i, j], j))
        cand = cand[:num_pairs]
        pairs.append(cand)
        pair_scores.append([float(scores[i, j]) for j in cand])
    return pairs, pair_scores


def depth_ranges(points, vis, extrinsics, lo=0.01, hi=0.99):
    points, E = _f(points), _f(extrinsics)
    out = np.empty((len(E), 2))
    for v in range(len(E)):
        p = points[np.asarray(vis[v]).astype(bool)]
        z = np.sort(((E[v, 2, 0] * p[:, 0] + E[v, 2, 1] * p[:, 1]) + E[v, 2, 2] * p[:, 2]) + E[v, 2, 3])
        n = len(z)
        out[v] = z[int(n * lo)], z[int(n * hi)]
    return out
