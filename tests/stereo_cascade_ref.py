"""The cascade of mvsdf_amd/stereo.py ("Cascade": the centres, the band sweep and the coarse-to-fine result) restated in vectorised numpy: fp64, every
product and sum a separate numpy operation in the order the definition writes it.  Written from that module's doc, not from the kernels.  Stage 1 is
stereo_ref's sweep (stereo_sgm_ref's where it is regularised)."""
import numpy as np

import stereo_ref
import stereo_sgm_ref
from fusion_ref import _row, matrices
from stereo_ref import _dot

MAX_STAGES, MAX_D_BAND = 4, 64


def scale_cams(cams, sx, sy):
    """focal lengths and principal point times (sx, sy)"""
    c = np.array(cams, np.float64)
    c[..., 1, 0, 0], c[..., 1, 0, 2] = c[..., 1, 0, 0] * sx, c[..., 1, 0, 2] * sx
    c[..., 1, 1, 1], c[..., 1, 1, 2] = c[..., 1, 1, 1] * sy, c[..., 1, 1, 2] * sy
    return c


def upsample(depth, best_k, size):
    """depth fp32 [V,r,s], best_k int [V,r,s], size (R, S) -> the centres fp64 [V,R,S], NaN where there is none"""
    depth, best_k = np.asarray(depth, np.float32).astype(np.float64), np.asarray(best_k)
    V, r, s = depth.shape
    R, S = size
    u = np.clip(((np.arange(S) + 0.5) * s) / S - 0.5, 0, s - 1)
    v = np.clip(((np.arange(R) + 0.5) * r) / R - 0.5, 0, r - 1)
    x0, y0 = np.minimum(np.floor(u), s - 2), np.minimum(np.floor(v), r - 2)
    fx, fy = (u - x0)[None, None, :], (v - y0)[None, :, None]
    xi, yi = x0.astype(np.int64)[None, :], y0.astype(np.int64)[:, None]
    num, den = np.zeros((V, R, S)), np.zeros((V, R, S))
    for (dy, dx), w in (((0, 0), (1 - fx) * (1 - fy)), ((0, 1), fx * (1 - fy)), ((1, 0), (1 - fx) * fy), ((1, 1), fx * fy)):
        ok = best_k[:, yi + dy, xi + dx] >= 0
        w = w + np.zeros((V, R, S))
        num = np.where(ok, num + w * depth[:, yi + dy, xi + dx], num)
        den = np.where(ok, den + w, den)
    with np.errstate(all='ignore'):
        return np.where(den > 0, num / den, np.nan)


def band_view(desc, cams, pairs, r, centres, depth_num, step, num_src=2):
    """one reference view; centres fp64 [R,S] of that view -> dict: scores fp64 [D_b,R,S] (NaN = invalid), n, depth fp32 [R,S], probs fp32 [3,R,S],
    best_k / counts int32 [R,S]"""
    desc = np.asarray(desc, np.float32)
    V, R, S, C = desc.shape
    D, half = int(depth_num), int(depth_num) // 2
    if R < 2 or S < 2 or not 1 <= D <= MAX_D_BAND or not (np.isfinite(step) and step > 0):
        raise ValueError('R and S >= 2, 1 <= D_b <= %d, step > 0' % MAX_D_BAND)
    c = np.asarray(centres, np.float64)
    if c.shape != (R, S) or np.isinf(c).any():
        raise ValueError('centres are [R,S], NaN or finite')
    P, Pinv = matrices(np.asarray(cams, np.float64))
    used = [int(s) for s in pairs[r]][:num_src]
    ys, xs = np.meshgrid(np.arange(R), np.arange(S), indexing='ij')
    X, Y = (xs + 0.5)[None], (ys + 0.5)[None]
    with np.errstate(all='ignore'):
        d = c[None] + (np.arange(D) - half).astype(np.float64)[:, None, None] * step
        live = ~np.isnan(c)[None] & (d > 0)
        fr = desc[r].astype(np.float64)[None]
        n = np.zeros((D, R, S), np.int64)
        acc = np.zeros((D, R, S))
        for s in used:
            T = P[s] @ Pinv[r]
            q0, q1 = X * d, Y * d
            p0, p1, p2 = _row(T[0], q0, q1, d, 1.0), _row(T[1], q0, q1, d, 1.0), _row(T[2], q0, q1, d, 1.0)
            ok = live & (p2 > 0)
            u, v = p0 / p2 - 0.5, p1 / p2 - 0.5
            ok &= (u >= 0) & (u <= S - 1) & (v >= 0) & (v <= R - 1)
            x0 = np.minimum(np.floor(np.where(ok, u, 0.0)), S - 2)
            y0 = np.minimum(np.floor(np.where(ok, v, 0.0)), R - 2)
            fx, fy = u - x0, v - y0
            xi, yi = x0.astype(np.int64), y0.astype(np.int64)
            fs = desc[s].astype(np.float64)
            t00, t01 = _dot(fr, fs[yi, xi]), _dot(fr, fs[yi, xi + 1])
            t10, t11 = _dot(fr, fs[yi + 1, xi]), _dot(fr, fs[yi + 1, xi + 1])
            cs = (t00 * (1 - fx) + t01 * fx) * (1 - fy) + (t10 * (1 - fx) + t11 * fx) * fy
            n += ok
            acc = np.where(ok, acc + cs, acc)
        valid = n >= 1
        scores = np.where(valid, acc / n, np.nan)
        b = np.full((R, S), -np.inf)
        ks = np.full((R, S), -1, np.int64)
        for k in range(D):
            better = valid[k] & (scores[k] > b)
            b = np.where(better, scores[k], b)
            ks = np.where(better, k, ks)
        has = ks >= 0
        kc = np.maximum(ks, 0)
        km, kp = np.maximum(kc - 1, 0), np.minimum(kc + 1, D - 1)
        inner = has & (kc > 0) & (kc < D - 1) & valid[km, ys, xs] & valid[kp, ys, xs]
        a, cc = scores[km, ys, xs], scores[kp, ys, xs]
        den = (a - 2 * b) + cc
        off = np.where(inner & (den < 0), (0.5 * (a - cc)) / den, 0.0)
        depth = np.where(has, (c + ((kc - half) + off) * step).astype(np.float32), np.float32(0))
        prob1 = np.minimum(np.maximum(b, 0.0), 1.0)
        far = valid & (np.abs(np.arange(D)[:, None, None] - kc[None]) >= 2)
        b2 = np.where(far, scores, -np.inf).max(0)
        prob2 = np.where(far.any(0), np.minimum(np.maximum(1 - np.maximum(b2, 0.0) / b, 0.0), 1.0), 1.0)
        prob2 = np.where(b <= 0, 0.0, prob2)
        nk = n[kc, ys, xs]
        prob3 = nk / float(max(len(used), 1))
        probs = np.where(has[None], np.stack([prob1, prob2, prob3]), 0.0).astype(np.float32)
    return dict(scores=scores, n=n, depth=depth.astype(np.float32), probs=probs, best_k=ks.astype(np.int32),
                counts=np.where(has, nk, 0).astype(np.int32))


def band(desc, cams, pairs, centres, depth_num, steps, num_src=2, views=None):
    """every view of views (default: all); steps: one per view of V -> stereo_ref.sweep's dict without scores"""
    desc = np.asarray(desc, np.float32)
    V, R, S, _ = desc.shape
    out = dict(depths=np.zeros((V, R, S), np.float32), probs=np.zeros((V, 3, R, S), np.float32), best_k=np.full((V, R, S), -1, np.int32),
               counts=np.zeros((V, R, S), np.int32))
    for r in (range(V) if views is None else views):
        o = band_view(desc, cams, pairs, r, centres[r], depth_num, steps[r], num_src)
        out['depths'][r], out['probs'][r], out['best_k'][r], out['counts'][r] = o['depth'], o['probs'], o['best_k'], o['counts']
    return out


def cascade(descs, cams, pairs, num_src=2, views=None, depth_nums=(None, 32, 16), interval_scales=(4, 2, 1), regularize=None):
    """descs: one map [V,R_l,S_l,C_l] per stage; cams at the last stage's size; regularize: None or (p1, p2, paths) -> dict: depths, probs, best_k,
    counts (the final maps) and stages, a list of per-stage dicts of the same four"""
    L = len(descs)
    if not 1 <= L <= MAX_STAGES or len(depth_nums) != L or len(interval_scales) != L or any(d is None for d in depth_nums[1:]):
        raise ValueError('1 to %d stages, one depth number and one scale per stage, None for D_1 only' % MAX_STAGES)
    if not all(np.isfinite(g) and g > 0 for g in interval_scales):
        raise ValueError('scales are finite and positive')
    descs = [np.asarray(d, np.float32) for d in descs]
    cams = np.asarray(cams, np.float64)
    V = descs[0].shape[0]
    if any(d.shape[0] != V for d in descs):
        raise ValueError('V differs between the stages')
    RL, SL = descs[-1].shape[1:3]
    interval, D = cams[:, 1, 3, 1], cams[:, 1, 3, 2]
    views = list(range(V)) if views is None else list(views)
    stages = []
    for l, desc in enumerate(descs):
        R, S = desc.shape[1:3]
        c = scale_cams(cams, S / SL, R / RL)
        step = interval * interval_scales[l]
        if l == 0:
            c[:, 1, 3, 1] = step
            c[:, 1, 3, 2] = np.ceil(D / interval_scales[0]) if depth_nums[0] is None else depth_nums[0]
            if regularize is None:
                o = stereo_ref.sweep(desc, c, pairs, num_src, views)
            else:
                o = stereo_sgm_ref.sweep(desc, c, pairs, num_src, views, *regularize)
        else:
            centres = upsample(stages[-1]['depths'], stages[-1]['best_k'], (R, S))
            o = band(desc, c, pairs, centres, depth_nums[l], step, num_src, views)
        stages.append({k: o[k] for k in ('depths', 'probs', 'best_k', 'counts')})
    last, first = stages[-1], stages[0]
    R1, S1 = first['depths'].shape[1:]
    yy = ((2 * np.arange(RL) + 1) * R1) // (2 * RL)
    xx = ((2 * np.arange(SL) + 1) * S1) // (2 * SL)
    probs = last['probs'].copy()
    probs[:, 1] = np.where(last['best_k'] >= 0, first['probs'][:, 1][:, yy][:, :, xx], np.float32(0))
    return dict(depths=last['depths'], probs=probs, best_k=last['best_k'], counts=last['counts'], stages=stages)
