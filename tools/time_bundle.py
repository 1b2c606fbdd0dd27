#!/usr/bin/env python3
"""Times of mvsdf_amd/bundle.py on the GPU (device events, the median of 5 after a warm-up) on a synthetic problem built on the device from a seed:
by default 64 views on a circle around 200 000 points, 5 observations each (1 000 000 observations, 0.3 px noise, perturbed start).

    python tools/time_bundle.py [--views 64 --points 200000 --per_point 5 --iterations 10 --cg_iters 64 --seed 0 --json OUT]

Reports, as C-entry call times: the set-up every call shares together with one cost evaluation (copies, checks, the by-view sort, the cost and its
tree: mvsdf_ba_residuals; a trial cost is the smaller part of it and has no entry of its own), linearise + blocks (mvsdf_ba_blocks minus that call),
one S x (mvsdf_ba_schur), one whole PCG solve with its iteration count (mvsdf_ba_solve, the frozen launches after "done" included), and the whole
bundle_adjust with its single host wait and its launch count.  For S x: the bytes the product
needs (A, B and the view index once, the 6 terms of W y written and read, the place in view order) over its time, as a share of the 6.3 TB/s a copy
achieves on this device; and the same product written in plain torch fp64 (index_add_ + bmm) on the same arrays, the yardstick."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
ACHIEVABLE = 6.3e12                                   # bytes / s of a streaming copy


def problem(views, points, per_point, seed, dev):
    """-> (cams numpy [V,2,4,4] perturbed, xyz [P,3] perturbed, track_off, track_view, obs) on the device"""
    import numpy as np
    import torch
    rs = np.random.RandomState(seed)
    cams = np.zeros((views, 2, 4, 4))
    for v in range(views):
        a = 2 * math.pi * v / views
        c = np.array([8.0 * math.sin(a), 0.5 * math.sin(3 * a), -8.0 * math.cos(a)])
        z = -c / np.linalg.norm(c)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        cams[v, 0] = np.eye(4)
        cams[v, 0, :3, :3] = R
        cams[v, 0, :3, 3] = -R @ c
        cams[v, 1, :3, :3] = [[1200.0, 0.3, 640.0], [0, 1180.0, 512.0], [0, 0, 1]]
        cams[v, 1, 3, 3] = 1.0
    g = torch.Generator(device=dev).manual_seed(seed)
    xyz = torch.rand(points, 3, generator=g, device=dev, dtype=torch.float64) * 2 - 1
    view = torch.rand(points, views, generator=g, device=dev).topk(per_point, dim=1).indices.to(torch.int32).reshape(-1).contiguous()
    off = torch.arange(points + 1, device=dev, dtype=torch.int64) * per_point
    E, Km = torch.from_numpy(cams[:, 0]).to(dev), torch.from_numpy(cams[:, 1, :3, :3]).to(dev)
    X = xyz.repeat_interleave(per_point, 0)
    q = torch.einsum('nkl,nl->nk', E[view.long(), :3, :3], X) + E[view.long(), :3, 3]
    p = torch.einsum('nkl,nl->nk', Km[view.long()], q)
    obs = (p[:, :2] / p[:, 2:3] + 0.3 * torch.randn(len(view), 2, generator=g, device=dev, dtype=torch.float64)).contiguous()
    start = cams.copy()
    for v in range(1, views):
        w = rs.normal(size=3) * math.radians(0.3)
        Kx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
        R = (np.eye(3) + Kx + 0.5 * Kx @ Kx) @ cams[v, 0, :3, :3]
        u, _, vt = np.linalg.svd(R)
        start[v, 0, :3, :3] = u @ vt
        start[v, 0, :3, 3] = cams[v, 0, :3, 3] + rs.normal(size=3) * 0.02
    return start, xyz + 0.01 * torch.randn(points, 3, generator=g, device=dev, dtype=torch.float64), off, view, obs


def median_ms(fn, repeats=5):
    import torch
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def launches(views, iterations, cg_iters):
    """kernel launches of one mvsdf_ba_adjust call (memsets and copies not counted): csrc/bundle.hip's host side, restated"""
    bits = 1
    while (1 << bits) < views:
        bits += 1
    begin = 1 + 4 + 1 + 1 + ((bits + 3) // 4) * 5 + 1 + 3 + 1
    return begin + iterations * (5 + 1 + 3 * cg_iters + 2 + 3 + 1) + 2


def torch_blocks(pr, lam, floor):
    """A [nnz,2,6], B [nnz,2,3], Vinv [P,3,3], Ud [V,6,6] in plain torch fp64 at the same parameters (plain least squares)"""
    import torch
    view, owner = pr.view.long(), torch.repeat_interleave(torch.arange(pr.P, device=pr.dev), pr.off[1:] - pr.off[:-1])
    R, t, k = pr.pose[view, :9].reshape(-1, 3, 3), pr.pose[view, 9:], pr.intr[view]
    q = torch.einsum('nkl,nl->nk', R, pr.xyz[owner]) + t
    u, v, iz = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2], 1 / q[:, 2]
    D = torch.zeros(len(view), 2, 3, dtype=torch.float64, device=pr.dev)
    D[:, 0, 0], D[:, 0, 1], D[:, 0, 2] = k[:, 0] * iz, k[:, 1] * iz, -(k[:, 0] * u + k[:, 1] * v) * iz
    D[:, 1, 1], D[:, 1, 2] = k[:, 3] * iz, -(k[:, 3] * v) * iz
    qx = torch.zeros(len(view), 3, 3, dtype=torch.float64, device=pr.dev)
    qx[:, 0, 1], qx[:, 0, 2], qx[:, 1, 0], qx[:, 1, 2], qx[:, 2, 0], qx[:, 2, 1] = q[:, 2], -q[:, 1], -q[:, 2], q[:, 0], q[:, 1], -q[:, 0]
    A = torch.cat([torch.bmm(D, qx), D], 2).contiguous()
    B = torch.bmm(D, R).contiguous()
    Vb = torch.zeros(pr.P, 3, 3, dtype=torch.float64, device=pr.dev).index_add_(0, owner, torch.bmm(B.transpose(1, 2), B))
    U = torch.zeros(pr.V, 6, 6, dtype=torch.float64, device=pr.dev).index_add_(0, view, torch.bmm(A.transpose(1, 2), A))
    damp = lambda M: M + torch.diag_embed(lam * torch.clamp(torch.diagonal(M, dim1=1, dim2=2), min=floor))          # noqa: E731
    return A, B, torch.linalg.inv(damp(Vb)), damp(U), view, owner


def torch_schur(A, B, Vinv, Ud, view, owner, x):
    import torch
    u = torch.bmm(A, x[view][:, :, None])
    acc = torch.zeros(Vinv.shape[0], 3, 1, dtype=torch.float64, device=x.device).index_add_(0, owner, torch.bmm(B.transpose(1, 2), u))
    y = torch.bmm(Vinv, acc)
    wy = torch.bmm(A.transpose(1, 2), torch.bmm(B, y[owner]))
    return torch.bmm(Ud, x[:, :, None])[:, :, 0] - torch.zeros_like(x).index_add_(0, view, wy[:, :, 0])


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('--views', type=int, default=64)
    p.add_argument('--points', type=int, default=200000)
    p.add_argument('--per_point', type=int, default=5)
    p.add_argument('--iterations', type=int, default=10)
    p.add_argument('--cg_iters', type=int, default=64)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--json', type=str, default=None)
    a = p.parse_args(argv)
    import torch
    from mvsdf_amd import bundle
    from mvsdf_amd._lib import K, _stream, _vp, check, lib
    if not torch.cuda.is_available():
        raise RuntimeError('time_bundle.py: no GPU; times are measured on the device or not at all')
    dev = torch.device('cuda')
    cams, xyz, off, view, obs = problem(a.views, a.points, a.per_point, a.seed, dev)
    pr = bundle._problem(cams, xyz, off, view, obs, (0, 1), 'time_bundle')
    L, ws = lib(), bundle._workspace(pr)
    st = _stream(ws)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)                                                  # noqa: E731
    U, gc, Vb, gp, b, x, sx = z(pr.V, 6, 6), z(pr.V, 6), z(pr.P, 3, 3), z(pr.P, 3), z(pr.V, 6), z(pr.V, 6), z(pr.V, 6)
    pose, out, r, terms = z(pr.V, 12), z(pr.P, 3), z(pr.nnz, 2), z(pr.nnz)
    rod = torch.from_numpy(bundle.rodrigues_table()).to(dev)
    lam, inf = 1e-4, math.inf
    common = (_vp(pr.pose), _vp(pr.intr), _vp(pr.xyz), _vp(pr.off), _vp(pr.view), _vp(pr.obs))

    def adjust(iterations):
        check(L.mvsdf_ba_adjust(*common, _vp(pr.fixed), pr.V, pr.P, pr.nnz, _vp(rod), inf, iterations, lam, 1e-10, 1e10, bundle.FLOOR, a.cg_iters, 1e-8,
                                1e-9, _vp(ws), ws.numel(), _vp(pose), _vp(out), _vp(r), _vp(terms), st), 'mvsdf_ba_adjust')

    def blocks():
        check(L.mvsdf_ba_blocks(*common, _vp(pr.fixed), pr.V, pr.P, pr.nnz, inf, lam, bundle.FLOOR, _vp(ws), ws.numel(), _vp(U), _vp(gc), _vp(Vb), _vp(gp),
                                _vp(b), st), 'mvsdf_ba_blocks')

    def resid():
        check(L.mvsdf_ba_residuals(*common, pr.V, pr.P, pr.nnz, inf, 1, _vp(ws), ws.numel(), _vp(r), _vp(terms), st), 'mvsdf_ba_residuals')

    res = {'views': pr.V, 'points': pr.P, 'observations': pr.nnz, 'cg_iters': a.cg_iters, 'iterations': a.iterations}
    res['setup_and_cost_ms'] = median_ms(resid)
    res['blocks_call_ms'] = median_ms(blocks)
    res['linearise_blocks_ms'] = res['blocks_call_ms'] - res['setup_and_cost_ms']
    probe = torch.randn(pr.V, 6, generator=torch.Generator(device=dev).manual_seed(1), device=dev, dtype=torch.float64)
    res['schur_ms'] = median_ms(lambda: check(L.mvsdf_ba_schur(pr.V, pr.P, pr.nnz, _vp(ws), ws.numel(), _vp(probe), _vp(sx), st), 'mvsdf_ba_schur'))
    res['schur_bytes'] = pr.nnz * (18 * 8 + 6 * 8 + 6 * 8 + 4 + 4) + pr.P * (6 * 8 + 8)
    res['schur_share_of_achievable'] = res['schur_bytes'] / (res['schur_ms'] * 1e-3) / ACHIEVABLE
    res['solve_ms'] = median_ms(lambda: check(L.mvsdf_ba_solve(pr.V, pr.P, pr.nnz, None, a.cg_iters, 1e-8, _vp(ws), ws.numel(), _vp(x), st), 'mvsdf_ba_solve'))
    res['solve_cg_iterations'] = bundle._head(ws, 'time_bundle')[K.MVSDF_BA_H_CG]
    tb = torch_blocks(pr, lam, bundle.FLOOR)
    res['torch_schur_ms'] = median_ms(lambda: torch_schur(*tb, probe))
    ours, theirs = sx[2:], torch_schur(*tb, probe)[2:]                    # (views 0 and 1 are fixed: their rows are 0 in ours)
    res['schur_relative_difference_to_torch'] = float((ours - theirs).abs().max() / theirs.abs().max())
    res['adjust_ms'] = median_ms(lambda: adjust(a.iterations))
    h = bundle._head(ws, 'time_bundle')
    res.update(adjust_launches=launches(pr.V, a.iterations, a.cg_iters), adjust_iterations=h[K.MVSDF_BA_H_ITER], adjust_accepted=h[K.MVSDF_BA_H_ACCEPTED],
               adjust_cg_iterations=h[K.MVSDF_BA_H_CG], cost0=bundle.f64_from_bits(h[K.MVSDF_BA_H_COST0]), cost=bundle.f64_from_bits(h[K.MVSDF_BA_H_COST]))
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, 'w') as f:
            f.write(line + '\n')
    return res


if __name__ == '__main__':
    main()
