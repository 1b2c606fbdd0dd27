"""Time of the depth-map fusion (mvsdf_amd/fusion.py, csrc/fusion.hip) on a synthetic scene of DTU size: --views cameras on a circle around a
sphere (synth._camera / synth.make_depth_maps, 2 % holes), depth maps of --hw, every view's sources its --view nearest neighbours by angle.

A host clock around fuse_depths, which ends in its header read plus the emit launch (a synchronize closes the interval).  Prints one JSON line
with the median and the runs.  --torch times the same steps written as batched torch calls on the device, one view pair at a time with
grid_sample for the gather (the way the fusion script the reference points to works); --cpu times the numpy restatement (tests/fusion_ref.py) on
--cpu_views reference views and scales to all of them.

    python tools/time_fusion.py [--views 49 --hw 600,800 --view 10 --repeats 5] [--torch] [--cpu [--cpu_views 2]]
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

from mvsdf_amd.utils import synth  # noqa: E402

SIZE, CENTER = 2.0, np.array([0.1, -0.2, 0.05])


def scene(views, hw, view):
    h, w = hw
    img_wh = (2 * w, 2 * h)
    ang = [2 * np.pi * i / views for i in range(views)]
    cams = np.stack([synth._camera(a, 2.5, 0.8, SIZE, CENTER, img_wh, 2.2 * img_wh[0], hw)[2] for a in ang])
    depths = synth.make_depth_maps(cams[:, None], SIZE, CENTER, bump=0.0, view_bias=0.0, hole_frac=0.02)[:, 0, 0]
    ring = lambda i, j: min((i - j) % views, (j - i) % views)                                    # noqa: E731
    pairs = [sorted((j for j in range(views) if j != i), key=lambda j: (ring(i, j), j))[:view] for i in range(views)]
    return cams, np.ascontiguousarray(depths), pairs


def fuse_torch(cams, depths, pairs, view=10, vthresh=2, pix_thresh=1.0, dep_thresh=0.01):
    """the definition's steps 2-4 as batched torch calls (fp64), one view pair at a time; depths: masked, fp64 [V,H,W] on the device.  The gather
    is grid_sample, so a hole is detected through a second grid_sample of the validity mask: close to the definition, not bit for bit."""
    from mvsdf_amd.fusion import projection_matrices
    dev = depths.device
    V, H, W = depths.shape
    P, Pinv = [torch.from_numpy(m).to(dev) for m in projection_matrices(cams)]
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64) + 0.5, torch.arange(W, device=dev, dtype=torch.float64) + 0.5, indexing='ij')
    X, Y = xs.reshape(-1), ys.reshape(-1)
    one = torch.ones_like(X)
    valid = (depths > 0).to(torch.float64)
    pts = []
    for r in range(V):
        d = depths[r].reshape(-1)
        n = torch.zeros_like(d)
        acc = d.clone()
        for s in pairs[r][:view]:
            p = (P[s] @ Pinv[r]) @ torch.stack([X * d, Y * d, d, one])
            u, v = p[0] / p[2], p[1] / p[2]
            grid = torch.stack([u / W * 2 - 1, v / H * 2 - 1], -1).view(1, H, W, 2)
            both = torch.nn.functional.grid_sample(torch.stack([depths[s], valid[s]])[None], grid, mode='bilinear', padding_mode='zeros', align_corners=False)[0]
            ds = both[0].reshape(-1)
            b = (P[r] @ Pinv[s]) @ torch.stack([u * ds, v * ds, ds, one])
            ex, ey = b[0] / b[2] - X, b[1] / b[2] - Y
            ok = (d > 0) & (p[2] > 0) & (both[1].reshape(-1) > 1 - 1e-9) & (b[2] > 0) & (ex * ex + ey * ey < pix_thresh * pix_thresh) \
                & ((b[2] - d).abs() < dep_thresh * d)
            n += ok
            acc = torch.where(ok, acc + b[2], acc)
        df = acc / (n + 1)
        keep = (d > 0) & (n >= vthresh)
        k = df[keep]
        pts.append((Pinv[r] @ torch.stack([X[keep] * k, Y[keep] * k, k, torch.ones_like(k)]))[:3].T)
    return torch.cat(pts)


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
    ap.add_argument('--views', type=int, default=49)
    ap.add_argument('--hw', type=str, default='600,800')
    ap.add_argument('--view', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--torch', action='store_true')
    ap.add_argument('--cpu', action='store_true')
    ap.add_argument('--cpu_views', type=int, default=2)
    a = ap.parse_args()
    hw = tuple(int(v) for v in a.hw.split(','))
    cams, depths, pairs = scene(a.views, hw, a.view)
    out = {'views': a.views, 'hw': list(hw), 'view': a.view, 'pair_pixels': int(sum(len(p) for p in pairs)) * hw[0] * hw[1]}
    if a.cpu:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import fusion_ref
        k = min(a.cpu_views, a.views)
        t0 = time.perf_counter()
        r = fusion_ref.fuse(cams, depths, [p if i < k else [] for i, p in enumerate(pairs)], view=a.view)
        t = time.perf_counter() - t0
        out.update({'path': 'numpy', 'cpu_views': k, 'measured_s': round(t, 2), 'scaled_to_all_views_s': round(t * a.views / k, 1),
                    'points_of_measured_views': int((r['view'] < k).sum())})
    else:
        assert torch.cuda.is_available(), 'time_fusion.py measures on the GPU (--cpu for the numpy restatement)'
        d = torch.from_numpy(depths).cuda()
        if a.torch:
            d64 = d.double()
            pts, runs = _timed(lambda: fuse_torch(cams, d64, pairs, a.view), a.repeats)
            out.update({'path': 'torch', 'points': int(pts.shape[0])})
        else:
            from mvsdf_amd import fusion
            f, runs = _timed(lambda: fusion.fuse_depths(cams, d, pairs, view=a.view), a.repeats)
            out.update({'path': 'hip', 'points': len(f)})
        out.update({'median_ms': round(float(np.median(runs)), 2), 'runs_ms': [round(v, 2) for v in runs]})
    print(json.dumps(out))


if __name__ == '__main__':
    main()
