"""Time of the stages of mvsdf_amd/global_reg.py on a synthetic pair: two independent random samplings (default 20,000 points each, taken as already
downsampled) of one bumpy sphere, the second turned and shifted.  Reported per stage as min / median / max over --repeats runs after one warm-up run,
in ms, host clock around work that ends in a device synchronise; the matcher, whose one call is short, is timed over --inner back-to-back calls per
run and divided:

* normals: normals.estimate_normals(k) + orient_normals of one cloud (the rows of stage 1 come with it);
* spfh, fpfh: stages 1 and 2 of one cloud at the feature radius;
* match, match_mutual: stage 3 (pack, walk, unpack).  `match_rate`: the int8 operations the matrix cores execute, 2 * Ns * Nt * 64 (K = 33 padded to
  64), over the median time, and its share of the int8 MFMA peak, taken as twice the dense BF16 peak MI355X_MICROARCH.md lists (2 * 2.5e15 / s: the
  I8 forms run the cycles of the BF16 forms at twice the K); `useful_rate` counts K = 33.  These are whole-call rates (three small kernels and their
  launches), not the walk kernel's share of peak;
* cdist_argmin: the yardstick, torch.cdist of the same codes in fp32 + argmin;
* ransac: stage 4 over the matches, --hypotheses hypotheses, with the counts it found;
* global_register: the composed call without and with refine (voxel chosen below the spacing, so that nearly every point stays).

Prints one JSON line.

    python tools/time_global_reg.py [--points 20000] [--k 32] [--hypotheses 100000] [--repeats 7] [--inner 20]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

INT8_PEAK = 2 * 2.5e15


def _bumpy_sphere(n, seed):
    rs = np.random.RandomState(seed)
    d = rs.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    r = 1.0 + 0.15 * np.sin(3.1 * x + 0.4) * np.cos(2.3 * y - 0.3) + 0.1 * np.sin(4.7 * z * x + 1.0) + 0.08 * np.cos(5.0 * y - 3.0 * z)
    return d * r[:, None]


def _motion():
    a = np.radians(140.0)
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    T[:3, 3] = (0.7, -1.3, 2.1)
    return T


def _timed(f, inner=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=20000)
    ap.add_argument('--k', type=int, default=32)
    ap.add_argument('--hypotheses', type=int, default=100000)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--inner', type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'time_global_reg.py measures on the GPU'
    from mvsdf_amd import global_reg as G
    from mvsdf_amd import normals
    n = a.points
    T = _motion()
    src = torch.from_numpy(_bumpy_sphere(n, 1)).cuda()
    dst = torch.from_numpy(_bumpy_sphere(n, 2) @ T[:3, :3].T + T[:3, 3]).cuda().contiguous()
    spacing = float(np.sqrt(4 * np.pi / n))
    voxel = spacing / 2                                          # the composed call: nearly every point stays
    radius, max_dist = 5 * spacing, 1.5 * spacing

    def oriented(p):
        nrm, _, nb = normals.estimate_normals(p, a.k)
        return normals.orient_normals(p, nrm, nb).normals, nb

    def codes(p):
        nrm, nb = oriented(p)
        hist, count = G.spfh(p, nrm, nb, radius)
        return G.fpfh(p, nb, hist, count, radius)[1]
    names = ('normals', 'spfh', 'fpfh', 'match', 'match_mutual', 'cdist_argmin', 'ransac', 'global_register', 'global_register_refine')
    times = {k: [] for k in names}
    out = {'points': n, 'k': a.k, 'hypotheses': a.hypotheses, 'repeats': a.repeats, 'inner': a.inner, 'match_splits': G.match_splits(n, n)}
    dc = codes(dst)
    for rep in range(a.repeats + 1):                              # the first run warms up
        tn, (nrm, nb) = _timed(lambda: oriented(src))
        ts, (hist, count) = _timed(lambda: G.spfh(src, nrm, nb, radius))
        tf, (_, sc) = _timed(lambda: G.fpfh(src, nb, hist, count, radius))
        tm, (index, _) = _timed(lambda: G.match_features(sc, dc), a.inner)
        tu, _ = _timed(lambda: G.match_features(sc, dc, mutual=True), a.inner)
        sf, df = sc.float(), dc.float()
        tc, yard = _timed(lambda: torch.cdist(sf, df).argmin(1), a.inner)
        tr, reg = _timed(lambda: G.ransac(src, dst, index, max_dist, a.hypotheses))
        tg, res = _timed(lambda: G.global_register(src, dst, voxel, k=a.k, feature_radius=radius, max_dist=max_dist, hypotheses=a.hypotheses, refine=False))
        ti, fin = _timed(lambda: G.global_register(src, dst, voxel, k=a.k, feature_radius=radius, max_dist=max_dist, hypotheses=a.hypotheses, refine=True))
        if rep == 0:
            R = reg.transformation[:3, :3] @ T[:3, :3].T
            out.update({'inliers': reg.inliers, 'checked': reg.checked, 'correspondences': int(reg.mask.shape[0]),
                        'rotation_error_degrees': float(np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))),
                        'cdist_argmin_agrees': float((yard.int() == index).double().mean()), 'refined_fitness': fin.fitness, 'flipped': bool(res.flipped)})
        else:
            for k, v in zip(names, (tn, ts, tf, tm, tu, tc, tr, tg, ti)):
                times[k].append(v)
    out['ms'] = {k: {'min': round(min(v), 4), 'median': round(float(np.median(v)), 4), 'max': round(max(v), 4)} for k, v in times.items()}
    sec = out['ms']['match']['median'] * 1e-3
    out['match_rate'] = {'int8_ops_per_s': 2.0 * n * n * 64 / sec, 'share_of_int8_peak': 2.0 * n * n * 64 / sec / INT8_PEAK, 'useful_ops_per_s': 2.0 * n * n * 33 / sec}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
