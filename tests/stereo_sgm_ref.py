"""The regularisation of mvsdf_amd/stereo.py ("Regularisation": semi-global aggregation of the score volume, then the pick on the regularised scores)
restated in vectorised numpy: fp64, every sum a separate numpy operation in the order the definition writes it.  Written from that module's doc, not
from the kernels.  A path is walked pixel by pixel; all the paths of one direction advance together, one image row (or column) per step."""
import numpy as np

import stereo_ref

DIRECTIONS = [(0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (-1, -1), (1, -1), (-1, 1)]              # (dy, dx)
DEFAULTS = (0.1, 0.8, 8)


def noisy_images(images, seed=5, sigma=12.0):
    """the test scene's images under seeded Gaussian noise of sigma grey levels -> uint8"""
    return np.clip(np.rint(images + np.random.RandomState(seed).normal(0, sigma, images.shape)), 0, 255).astype(np.uint8)


def _check(p1, p2, paths):
    if not (np.isfinite(p1) and np.isfinite(p2) and 0 <= p1 <= p2):
        raise ValueError('0 <= P1 <= P2, finite')
    if paths not in (4, 8):
        raise ValueError('paths is 4 or 8')


def _step(cost, prev, p1, p2):
    """cost [D,N] (NaN = invalid) at the pixels p, prev [D,N] = L_r at their q = p - r (all NaN where q is outside the image) -> L_r at p"""
    D = cost.shape[0]
    inf = np.full((1, cost.shape[1]), np.inf)
    own = np.where(np.isnan(prev), np.inf, prev)                             # an invalid entry takes no part in any minimum
    m = own.min(0)
    below = np.concatenate([inf, own[:D - 1] + p1], 0)                       # L_r(q, k-1) + P1, where k-1 exists
    above = np.concatenate([own[1:] + p1, inf], 0)                           # L_r(q, k+1) + P1
    best = np.minimum(np.minimum(own, below), np.minimum(above, (m + p2)[None]))
    with np.errstate(invalid='ignore'):
        moved = cost + (best - m[None])
    return np.where(np.isfinite(m)[None], moved, cost)                       # no valid k at q (or q outside): the path restarts


def path_costs(score, p1, p2, direction):
    """L_r of one direction, fp64 [D,R,S], NaN where the score is"""
    dy, dx = direction
    cost = 1.0 - np.asarray(score, np.float64)
    if dy == 0:                                                              # walk the columns: the same recurrence on the transposed image
        return path_costs_rows(cost.transpose(0, 2, 1), p1, p2, dx, 0).transpose(0, 2, 1)
    return path_costs_rows(cost, p1, p2, dy, dx)


def path_costs_rows(cost, p1, p2, dy, dx):
    D, R, S = cost.shape
    L = np.full((D, R, S), np.nan)
    for y in (range(R) if dy > 0 else range(R - 1, -1, -1)):
        prev = np.full((D, S), np.nan)
        yq = y - dy
        if 0 <= yq < R:
            if dx == 0:
                prev = L[:, yq]
            elif dx > 0:
                prev[:, 1:] = L[:, yq, :S - 1]                               # q = (y - dy, x - 1)
            else:
                prev[:, :S - 1] = L[:, yq, 1:]
        L[:, y] = _step(cost[:, y], prev, p1, p2)
    return L


def regularize(score, p1=DEFAULTS[0], p2=DEFAULTS[1], paths=DEFAULTS[2]):
    """score fp64 [D,R,S] (NaN = invalid) -> A fp64 [D,R,S]"""
    _check(p1, p2, paths)
    score = np.asarray(score, np.float64)
    if score.ndim != 3 or min(score.shape) < 1:
        raise ValueError('the volume is [D,R,S]')
    T = path_costs(score, p1, p2, DIRECTIONS[0])
    for r in range(1, paths):
        T = T + path_costs(score, p1, p2, DIRECTIONS[r])
    return np.where(np.isnan(score), np.nan, 1.0 - T / float(paths))


def pick(A, raw, n, dmin, interval, used):
    """the definition's winner, refinement and confidences on A; prob1 from the raw scores, prob3 / counts from n; used = the number of sources swept"""
    D, R, S = A.shape
    valid = ~np.isnan(A)
    with np.errstate(all='ignore'):
        b = np.full((R, S), -np.inf)
        ks = np.full((R, S), -1, np.int64)
        for k in range(D):
            better = valid[k] & (A[k] > b)
            b = np.where(better, A[k], b)
            ks = np.where(better, k, ks)
        has = ks >= 0
        kc = np.maximum(ks, 0)
        yy, xx = np.meshgrid(np.arange(R), np.arange(S), indexing='ij')
        km, kp = np.maximum(kc - 1, 0), np.minimum(kc + 1, D - 1)
        inner = has & (kc > 0) & (kc < D - 1) & valid[km, yy, xx] & valid[kp, yy, xx]
        a, c = A[km, yy, xx], A[kp, yy, xx]
        den = (a - 2 * b) + c
        off = np.where(inner & (den < 0), (0.5 * (a - c)) / den, 0.0)
        depth = np.where(has, (dmin + (kc + off) * interval).astype(np.float32), np.float32(0))
        prob1 = np.minimum(np.maximum(raw[kc, yy, xx], 0.0), 1.0)
        far = valid & (np.abs(np.arange(D)[:, None, None] - kc[None]) >= 2)
        b2 = np.where(far, A, -np.inf).max(0)
        prob2 = np.where(far.any(0), np.minimum(np.maximum(1 - np.maximum(b2, 0.0) / b, 0.0), 1.0), 1.0)
        prob2 = np.where(b <= 0, 0.0, prob2)
        nk = n[kc, yy, xx]
        prob3 = nk / float(max(used, 1))
        probs = np.where(has[None], np.stack([prob1, prob2, prob3]), 0.0).astype(np.float32)
    return dict(depth=depth.astype(np.float32), probs=probs, best_k=ks.astype(np.int32), counts=np.where(has, nk, 0).astype(np.int32))


def sweep_view(desc, cams, pairs, r, num_src=2, p1=DEFAULTS[0], p2=DEFAULTS[1], paths=DEFAULTS[2]):
    """stereo_ref.sweep_view with the regularisation between the scores and the pick; also reg_scores"""
    raw = stereo_ref.sweep_view(desc, cams, pairs, r, num_src)
    A = regularize(raw['scores'], p1, p2, paths)
    cams = np.asarray(cams, np.float64)
    o = pick(A, raw['scores'], raw['n'], cams[r, 1, 3, 0], cams[r, 1, 3, 1], len([int(s) for s in pairs[r]][:num_src]))
    o.update(scores=raw['scores'], reg_scores=A, n=raw['n'])
    return o


def sweep(desc, cams, pairs, num_src=2, views=None, p1=DEFAULTS[0], p2=DEFAULTS[1], paths=DEFAULTS[2]):
    """stereo_ref.sweep's dict for the regularised sweep, plus reg_scores of the last swept view"""
    desc = np.asarray(desc, np.float32)
    V, R, S, _ = desc.shape
    out = dict(depths=np.zeros((V, R, S), np.float32), probs=np.zeros((V, 3, R, S), np.float32), best_k=np.full((V, R, S), -1, np.int32),
               counts=np.zeros((V, R, S), np.int32), scores=None, reg_scores=None)
    for r in (range(V) if views is None else views):
        o = sweep_view(desc, cams, pairs, r, num_src, p1, p2, paths)
        out['depths'][r], out['probs'][r], out['best_k'][r], out['counts'][r] = o['depth'], o['probs'], o['best_k'], o['counts']
        out['scores'], out['reg_scores'] = o['scores'], o['reg_scores']
    return out
