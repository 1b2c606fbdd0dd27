"""Time of the plane sweep (mvsdf_amd/stereo.py, csrc/stereo.hip) at the shape of the reference's BYOD.md: --views cameras side by side in front of
a surface, descriptor maps of --hw with --channels channels (seeded noise, normalised: the timing depends on the geometry, not on the content),
--depths hypotheses, --num_src sources per view.

A host clock around plane_sweep, which ends in its header read (a synchronize closes the interval); the first run warms up.  The baseline is the
same definition written as plain torch calls in fp64 on the same GPU, one view and one chunk of hypotheses at a time, with explicit index gathers
(no grid_sample): sweep_torch below.  Its sums are torch's, not in channel order, so its depths are compared with a tolerance.  Prints one JSON
line: both medians, the ratio, and the gather bandwidth the HIP path achieves = 4 taps x C x 4 bytes per valid (pixel, hypothesis, source) over its
time (the bytes the lanes request; most are served by L1 / L2).

--sgm times the semi-global regularisation instead (same protocol, one JSON line): the sweep with regularize=True against the sweep without it, and
regularize_scores on the last view's score volume against the same definition as plain fp64 torch calls (regularize_torch below: one image row or
column per step, elementwise minima and sums in the definition's order, so it is compared bit for bit); the bytes the passes move = per direction
the scores read, the running sum read (not by the first) and written.

--cascade times stereo.cascade_sweep with its defaults (stages of --hw / 4, --hw / 2 and --hw, seeded noise descriptors per stage, 64 / 32 / 16
hypotheses at max_d 256; with --sgm its first stage is regularised) against the full sweep at --hw in the same run (same protocol, one JSON line),
and splits it by stage with device events around the calls cascade_sweep makes (plane_sweep, then upsample_depth + band_sweep per stage), whose
results are compared with cascade_sweep's bit for bit; samples = the (pixel, hypothesis) pairs each evaluates.

    python tools/time_stereo.py [--views 10 --hw 288,384 --channels 32 --depths 256 --num_src 2 --repeats 3 --torch_repeats 1 --chunk 8] [--sgm]
                                [--cascade]
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


def scene(views, hw, channels, depths, seed=0):
    """cameras 0.6 apart, 8 in front of the origin, looking at (0, 0, -5); hypotheses from 2.9 to 4.25"""
    h, w = hw
    cams = np.zeros((views, 2, 4, 4))
    for i in range(views):
        b = (i - (views - 1) / 2.0) * 0.6
        c = np.array([b, 0.15 * b, -8.0])
        z = (np.array([0.0, 0.0, -5.0]) - c)
        z /= np.linalg.norm(z)
        x = np.cross(np.array([0.0, 1.0, 0.0]), z)
        x /= np.linalg.norm(x)
        Rm = np.stack([x, np.cross(z, x), z])
        cams[i, 0] = np.eye(4)
        cams[i, 0, :3, :3] = Rm
        cams[i, 0, :3, 3] = -Rm @ c
        cams[i, 1, :3, :3] = [[1.5625 * w, 0, w / 2.0], [0, 1.5625 * w, h / 2.0], [0, 0, 1]]
        cams[i, 1, 3] = [2.9, 1.35 / max(depths - 1, 1), depths, 4.25]
    pairs = [sorted((j for j in range(views) if j != i), key=lambda j: (abs(j - i), j)) for i in range(views)]
    gen = torch.Generator().manual_seed(seed)
    feats = torch.randn(views, h, w, channels, generator=gen)
    return cams, pairs, feats


def sweep_torch(desc, cams, pairs, num_src, chunk):
    """the definition of mvsdf_amd/stereo.py in torch fp64; desc fp32 [V,R,S,C] on the device -> (depths fp32 [V,R,S], valid (pixel, hypothesis, source) count)"""
    from mvsdf_amd.fusion import projection_matrices
    dev = desc.device
    V, R, S, C = desc.shape
    P, Pinv = [torch.from_numpy(m).to(dev) for m in projection_matrices(cams)]
    ys, xs = torch.meshgrid(torch.arange(R, device=dev, dtype=torch.float64) + 0.5, torch.arange(S, device=dev, dtype=torch.float64) + 0.5, indexing='ij')
    out = torch.zeros(V, R, S, dtype=torch.float32, device=dev)
    nvalid = 0
    for r in range(V):
        dmin, interval, D = float(cams[r, 1, 3, 0]), float(cams[r, 1, 3, 1]), int(cams[r, 1, 3, 2])
        fr = desc[r].double()
        score = torch.full((D, R, S), float('nan'), dtype=torch.float64, device=dev)
        srcs = [(s, P[s] @ Pinv[r], desc[s].double().reshape(R * S, C)) for s in pairs[r][:num_src]]
        for k0 in range(0, D, chunk):
            d = (dmin + torch.arange(k0, min(D, k0 + chunk), device=dev, dtype=torch.float64) * interval)[:, None, None].expand(-1, R, S)
            n = torch.zeros_like(d)
            acc = torch.zeros_like(d)
            for s, T, fs in srcs:
                q0, q1 = xs * d, ys * d
                p = [((T[i, 0] * q0 + T[i, 1] * q1) + T[i, 2] * d) + T[i, 3] for i in range(3)]
                u, v = p[0] / p[2] - 0.5, p[1] / p[2] - 0.5
                ok = (p[2] > 0) & (u >= 0) & (u <= S - 1) & (v >= 0) & (v <= R - 1)
                x0 = torch.where(ok, u, torch.zeros_like(u)).floor().clamp(max=S - 2)
                y0 = torch.where(ok, v, torch.zeros_like(v)).floor().clamp(max=R - 2)
                fx, fy = u - x0, v - y0
                at = y0.long() * S + x0.long()
                t = [(fr * fs[at + o]).sum(-1) for o in (0, 1, S, S + 1)]
                cs = (t[0] * (1 - fx) + t[1] * fx) * (1 - fy) + (t[2] * (1 - fx) + t[3] * fx) * fy
                n += ok
                acc = torch.where(ok, acc + cs, acc)
                nvalid += int(ok.sum())
            score[k0:k0 + chunk] = torch.where(n > 0, acc / n, torch.full_like(acc, float('nan')))
        filled = torch.where(torch.isnan(score), torch.full_like(score, -float('inf')), score)
        b, ks = filled.max(0)                                     # (torch returns the first maximum: the lowest k)
        has = torch.isfinite(b)
        a = filled.gather(0, (ks - 1).clamp(min=0)[None])[0]
        c = filled.gather(0, (ks + 1).clamp(max=D - 1)[None])[0]
        den = (a - 2 * b) + c
        inner = has & (ks > 0) & (ks < D - 1) & torch.isfinite(a) & torch.isfinite(c) & (den < 0)
        off = torch.where(inner, 0.5 * (a - c) / den, torch.zeros_like(b))
        out[r] = torch.where(has, (dmin + (ks + off) * interval).float(), torch.zeros_like(b).float())
    return out, nvalid


SGM_DIRECTIONS = [(0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (-1, -1), (1, -1), (-1, 1)]


def regularize_torch(score, p1, p2, paths):
    """the regularisation of mvsdf_amd/stereo.py in torch fp64; score [D,R,S] on the device (NaN = invalid) -> A"""
    inf = float('inf')
    cost_all = 1.0 - score
    T = None
    for dy, dx in SGM_DIRECTIONS[:paths]:
        cost = cost_all if dy else cost_all.transpose(1, 2)                  # horizontal: the same walk over the columns
        sy, sx = (dy, dx) if dy else (dx, 0)
        D, R, S = cost.shape
        L = torch.empty_like(cost)
        edge = torch.full((D, 1), inf, dtype=cost.dtype, device=cost.device)
        top = torch.full((1, S), inf, dtype=cost.dtype, device=cost.device)
        prev = None
        for y in (range(R) if sy > 0 else range(R - 1, -1, -1)):
            c = cost[:, y]
            if prev is None:
                row = c
            else:
                own = torch.where(torch.isnan(prev), torch.full_like(prev, inf), prev)
                if sx > 0:
                    own = torch.cat([edge, own[:, :S - 1]], 1)
                elif sx < 0:
                    own = torch.cat([own[:, 1:], edge], 1)
                m = own.min(0).values
                below = torch.cat([top, own[:D - 1] + p1], 0)
                above = torch.cat([own[1:] + p1, top], 0)
                best = torch.minimum(torch.minimum(own, below), torch.minimum(above, (m + p2)[None]))
                row = torch.where(torch.isfinite(m)[None], c + (best - m[None]), c)
            L[:, y] = row
            prev = row
        L = L if dy else L.transpose(1, 2)
        T = L if T is None else T + L
    return torch.where(torch.isnan(score), score, 1.0 - T / float(paths))


def time_sgm(a, stereo, desc, cams, pairs, hw):
    p1, p2, paths = stereo.SGM_DEFAULTS
    _, plain = _timed(lambda: stereo.plane_sweep(desc, cams, pairs, num_src=a.num_src), a.repeats)
    _, runs = _timed(lambda: stereo.plane_sweep(desc, cams, pairs, num_src=a.num_src, regularize=True), a.repeats)
    vol = stereo.plane_sweep(desc, cams, pairs, num_src=a.num_src, views=[a.views - 1], scores=True).scores
    out, vruns = _timed(lambda: stereo.regularize_scores(vol, p1, p2, paths), a.repeats)
    ref, truns = _timed(lambda: regularize_torch(vol, p1, p2, paths), a.torch_repeats)
    same = torch.isnan(out) == torch.isnan(ref)
    differ = int((~same).sum()) + int((out[same & ~torch.isnan(ref)] != ref[same & ~torch.isnan(ref)]).sum())
    hip, base, one, tor = (float(np.median(v)) for v in (runs, plain, vruns, truns))
    moved = (3 * paths - 1) * vol.numel() * 8
    print(json.dumps({'sgm': [p1, p2, paths], 'views': a.views, 'hw': list(hw), 'channels': a.channels, 'depths': a.depths, 'num_src': a.num_src,
                      'sweep_sgm_median_ms': round(hip, 2), 'sweep_sgm_runs_ms': [round(v, 2) for v in runs], 'sweep_plain_median_ms': round(base, 2),
                      'sweep_plain_runs_ms': [round(v, 2) for v in plain], 'sgm_over_plain': round(hip / base, 2),
                      'regularize_hip_median_ms': round(one, 3), 'regularize_hip_runs_ms': [round(v, 3) for v in vruns],
                      'regularize_torch_median_ms': round(tor, 1), 'regularize_torch_runs_ms': [round(v, 1) for v in truns],
                      'torch_over_hip': round(tor / one, 1), 'elements_that_differ_from_torch': differ, 'elements': int(vol.numel()),
                      'invalid_share': round(float(torch.isnan(vol).double().mean()), 4), 'bytes_moved_per_volume': moved,
                      'GBps': round(moved / (one * 1e-3) / 1e9, 1)}))


def time_cascade(a, stereo, desc, cams, pairs, hw):
    from mvsdf_amd.utils.io import scale_camera
    dn, sc = stereo.CASCADE_DEFAULTS
    reg = True if a.sgm else None
    sizes = [(hw[0] // 4, hw[1] // 4), (hw[0] // 2, hw[1] // 2), hw]
    descs = [stereo.normalize_descriptors(torch.randn(a.views, r, s, a.channels, generator=torch.Generator().manual_seed(l + 1)).cuda())
             for l, (r, s) in enumerate(sizes[:-1])] + [desc]
    _, full = _timed(lambda: stereo.plane_sweep(desc, cams, pairs, num_src=a.num_src, regularize=reg), a.repeats)
    cas, runs = _timed(lambda: stereo.cascade_sweep(descs, cams, pairs, num_src=a.num_src, regularize=reg), a.repeats)
    # the same calls one by one, between device events
    stage_cams = []
    for l, (r, s) in enumerate(sizes):
        c = scale_camera(cams, (s / hw[1], r / hw[0]))
        c[:, 1, 3, 1] = cams[:, 1, 3, 1] * sc[l]
        if l == 0:
            c[:, 1, 3, 2] = np.ceil(cams[:, 1, 3, 2] / sc[0])
        stage_cams.append(c)

    def staged():
        ev = [torch.cuda.Event(enable_timing=True) for _ in sizes + [0]]
        ev[0].record()
        out = [stereo.plane_sweep(descs[0], stage_cams[0], pairs, num_src=a.num_src, regularize=reg)]
        ev[1].record()
        for l in range(1, len(sizes)):
            centres = stereo.upsample_depth(out[-1].depths, out[-1].best_k, sizes[l])
            out.append(stereo.band_sweep(descs[l], stage_cams[l], pairs, centres, dn[l], stage_cams[l][:, 1, 3, 1], num_src=a.num_src))
            ev[l + 1].record()
        torch.cuda.synchronize()
        return out, [ev[l].elapsed_time(ev[l + 1]) for l in range(len(sizes))]

    split = []
    for rep in range(a.repeats + 1):                              # the first run warms up
        out, ms = staged()
        if rep:
            split.append(ms)
    differ = sum(int((getattr(o, n) != getattr(st, n)).sum()) for o, st in zip(out, cas.stages) for n in ('depths', 'probs', 'best_k', 'counts'))
    hip, base = float(np.median(runs)), float(np.median(full))
    nums = [int(np.ceil(a.depths / sc[0])) if dn[0] is None else dn[0]] + list(dn[1:])
    print(json.dumps({'cascade': [nums, list(sc)], 'sgm': bool(a.sgm), 'views': a.views, 'stage_hw': [list(v) for v in sizes], 'channels': a.channels,
                      'depths': a.depths, 'num_src': a.num_src, 'cascade_median_ms': round(hip, 2), 'cascade_runs_ms': [round(v, 2) for v in runs],
                      'full_sweep_median_ms': round(base, 2), 'full_sweep_runs_ms': [round(v, 2) for v in full], 'full_over_cascade': round(base / hip, 2),
                      'stage_median_ms': [round(float(v), 3) for v in np.median(np.asarray(split), 0)],
                      'stage_samples_per_view': [n * r * s for n, (r, s) in zip(nums, sizes)], 'full_samples_per_view': a.depths * hw[0] * hw[1],
                      'stage_elements_that_differ_from_cascade_sweep': differ,
                      'winner_share_last_stage': round(float((cas.best_k >= 0).double().mean()), 4)}))


def _timed(fn, repeats):
    runs = []
    for rep in range(repeats + 1):                                # the first run warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if rep:
            runs.append((time.perf_counter() - t0) * 1e3)
    return out, runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=10)
    ap.add_argument('--hw', type=str, default='288,384')
    ap.add_argument('--channels', type=int, default=32)
    ap.add_argument('--depths', type=int, default=256)
    ap.add_argument('--num_src', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--torch_repeats', type=int, default=1)
    ap.add_argument('--chunk', type=int, default=8)
    ap.add_argument('--sgm', action='store_true', default=False, help='time the semi-global regularisation instead')
    ap.add_argument('--cascade', action='store_true', default=False, help='time the coarse-to-fine cascade instead (with --sgm: its first stage regularised)')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'time_stereo.py measures on the GPU'
    from mvsdf_amd import stereo
    hw = tuple(int(v) for v in a.hw.split(','))
    cams, pairs, feats = scene(a.views, hw, a.channels, a.depths)
    desc = stereo.normalize_descriptors(feats.cuda())
    if a.cascade:
        return time_cascade(a, stereo, desc, cams, pairs, hw)
    if a.sgm:
        return time_sgm(a, stereo, desc, cams, pairs, hw)
    sw, runs = _timed(lambda: stereo.plane_sweep(desc, cams, pairs, num_src=a.num_src), a.repeats)
    (ref, nvalid), truns = _timed(lambda: sweep_torch(desc, cams, pairs, a.num_src, a.chunk), a.torch_repeats)
    diff = (sw.depths - ref).abs()
    hip, tor = float(np.median(runs)), float(np.median(truns))
    print(json.dumps({'views': a.views, 'hw': list(hw), 'channels': a.channels, 'depths': a.depths, 'num_src': a.num_src,
                      'hip_median_ms': round(hip, 2), 'hip_runs_ms': [round(v, 2) for v in runs], 'torch_median_ms': round(tor, 1),
                      'torch_runs_ms': [round(v, 1) for v in truns], 'torch_over_hip': round(tor / hip, 1), 'valid_samples': nvalid,
                      'gather_GBps': round(nvalid * 4 * a.channels * 4 / (hip * 1e-3) / 1e9, 1),
                      'depth_mismatch_above_1e-4_interval': int((diff > 1e-4 * cams[0, 1, 3, 1]).sum()), 'pixels': int(diff.numel())}))


if __name__ == '__main__':
    main()
