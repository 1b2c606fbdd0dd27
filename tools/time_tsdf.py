"""Time of the TSDF fusion (mvsdf_amd/tsdf.py, csrc/tsdf.hip) on tools/time_fusion.py's scene at its defaults: --views cameras on a circle around a
sphere, depth maps of --hw with 2 % holes, integrated into a --grid^3 lattice centred on the sphere (half-extent 0.7 around a radius of 0.6,
trunc = 4 voxels).

Device events around integrate_depths' launch work and around Volume.mesh(), plus a host clock around the whole calls (a synchronize closes the
interval); medians after a warm-up.  --torch times the same integration written as batched fp64 torch calls on the same device, one view at a
time over the whole lattice with explicit gathers: the definition's arithmetic, not bit for bit (torch may contract and reorder).  Every mode
appends one JSON line to --out and prints it.

The scene's maps each carry a depth step of 0.12 over a patch (synth.make_depth_maps).  Where two views' patches agree, a second sheet that far
inside the sphere (22 voxels at the defaults) is a correct part of the result; max_vertex_error_voxels reports it.

    python tools/time_tsdf.py [--views 49 --hw 600,800 --grid 256 --repeats 5] [--torch] [--out profiles/tsdf_time_lines.jsonl]
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

from time_fusion import CENTER, scene  # noqa: E402


def integrate_torch(P, depths, origin, h, dims, trunc, jump, min_views):
    """the definition as batched torch calls; P fp64 [V,4,4] and depths fp32 [V,H,W] on the device -> (tsdf fp32, weight int32)"""
    dev = depths.device
    V, H, W = depths.shape
    ax = [origin[a] + torch.arange(dims[a], device=dev, dtype=torch.float64) * h for a in range(3)]
    p0, p1, p2 = torch.meshgrid(*ax, indexing='ij')
    D = torch.zeros(dims, dtype=torch.float64, device=dev)
    n = torch.zeros(dims, dtype=torch.int32, device=dev)
    for v in range(V):
        T = P[v]
        z = ((T[2, 0] * p0 + T[2, 1] * p1) + T[2, 2] * p2) + T[2, 3]
        u = (((T[0, 0] * p0 + T[0, 1] * p1) + T[0, 2] * p2) + T[0, 3]) / z - 0.5
        w = (((T[1, 0] * p0 + T[1, 1] * p1) + T[1, 2] * p2) + T[1, 3]) / z - 0.5
        ok = (z > 0) & (u >= 0) & (u <= W - 1) & (w >= 0) & (w <= H - 1)
        x0 = torch.where(ok, u, 0.0).floor_().clamp_(max=W - 2)
        y0 = torch.where(ok, w, 0.0).floor_().clamp_(max=H - 2)
        fx, fy = u - x0, w - y0
        at = y0.long() * W + x0.long()
        src = depths[v].reshape(-1)
        d00, d01, d10, d11 = src[at].double(), src[at + 1].double(), src[at + W].double(), src[at + W + 1].double()
        ok &= (d00 > 0) & (d01 > 0) & (d10 > 0) & (d11 > 0) & torch.isfinite(d00 + d01 + d10 + d11)
        mx = torch.maximum(torch.maximum(d00, d01), torch.maximum(d10, d11))
        mn = torch.minimum(torch.minimum(d00, d01), torch.minimum(d10, d11))
        ok &= ~(mx - mn > jump)
        ds = (d00 * (1 - fx) + d01 * fx) * (1 - fy) + (d10 * (1 - fx) + d11 * fx) * fy
        s = ds - z
        ok &= ~(s < -trunc)
        D += torch.where(ok, (s / trunc).clamp_(max=1.0), 0.0)
        n += ok
    valid = n >= min_views
    return torch.where(valid, (D / n).float(), 1.0), n


def _timed(fn, repeats):
    """-> (last result, host ms per run, device ms per run); the first run warms up"""
    host, devt, out = [], [], None
    for rep in range(repeats + 1):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if rep:
            host.append((time.perf_counter() - t0) * 1e3)
            devt.append(e0.elapsed_time(e1))
    return out, host, devt


def _stats(prefix, host, devt):
    r = lambda xs: [round(float(x), 3) for x in xs]                              # noqa: E731
    return {prefix + '_host_ms': round(float(np.median(host)), 3), prefix + '_device_ms': round(float(np.median(devt)), 3),
            prefix + '_host_runs_ms': r(host), prefix + '_device_runs_ms': r(devt)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=49)
    ap.add_argument('--hw', type=str, default='600,800')
    ap.add_argument('--grid', type=int, default=256)
    ap.add_argument('--min_views', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--torch', action='store_true')
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'tsdf_time_lines.jsonl'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'time_tsdf.py measures on the GPU'
    from mvsdf_amd import tsdf
    from mvsdf_amd.fusion import projection_matrices
    hw = tuple(int(v) for v in a.hw.split(','))
    cams, depths, _ = scene(a.views, hw, 10)
    d = torch.from_numpy(depths).cuda()
    dims = (a.grid,) * 3
    h = 1.4 / (a.grid - 1)
    origin = CENTER - 0.7
    out = {'views': a.views, 'hw': list(hw), 'grid': a.grid, 'voxel': h, 'trunc': 4 * h, 'min_views': a.min_views,
           'point_views': a.grid ** 3 * a.views}
    if a.torch:
        P = torch.from_numpy(projection_matrices(cams)[0]).cuda()
        (t, n), host, devt = _timed(lambda: integrate_torch(P, d, origin, h, dims, 4 * h, 4 * h, a.min_views), a.repeats)
        vol = tsdf.integrate_depths(cams, d, origin, h, dims, min_views=a.min_views)
        out.update({'path': 'torch', 'valid': int((n >= a.min_views).sum()), 'weights_differing_from_hip': int((n != vol.weight).sum()),
                    'max_abs_tsdf_difference_from_hip': float((t - vol.tsdf).abs().max())})
        out.update(_stats('integrate', host, devt))
    else:
        vol, host, devt = _timed(lambda: tsdf.integrate_depths(cams, d, origin, h, dims, min_views=a.min_views), a.repeats)
        out.update({'path': 'hip', 'valid': int(vol.valid.sum()), 'valid_share': round(vol.valid_share(), 5)})
        out.update(_stats('integrate', host, devt))
        mesh, host, devt = _timed(vol.mesh, a.repeats)
        out.update({'vertices': int(mesh.vertices.shape[0]), 'faces': len(mesh)})
        out.update(_stats('mesh', host, devt))
        r = (mesh.vertices.double() - torch.from_numpy(CENTER).cuda()).norm(dim=1)
        out['max_vertex_error_voxels'] = round(float((r - 0.6).abs().max()) / h, 3)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
