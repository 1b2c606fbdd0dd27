"""Device time of view_scores (mvsdf_amd/viewsel.py, csrc/viewsel.hip) in two regimes, beside a plain chunked torch formulation of the same score
on the same GPU: the median of --repeats runs after a warm-up, each between two device events, one JSON line per regime.

sparse: V = 300 views, P = 2e5 points, tracks of about 6 neighbouring views (a COLMAP model); dense: V = 49, P = 2e6, about half of the views per
point (vertex_visibility of a mesh).  The torch formulation walks the points in chunks, forms every pair (i, j) of a chunk at once (cross, dot,
torch.atan2, torch.exp, the quantised weights summed as int64 by a matrix of masks) and so uses the library functions: its scores differ from the
kernel's in the last quantum of a weight, and it is compared by TIME only (the largest difference is printed).

    python tools/time_viewsel.py [--regimes sparse,dense --repeats 3 --chunk 4096]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

REGIMES = {'sparse': (300, 200000), 'dense': (49, 2000000)}


def make(regime, seed=0):
    """-> (points [P,3], centres [V,3], vis uint8 [V,P]) on the device: cameras on a ring around a unit cube of points"""
    V, P = REGIMES[regime]
    g = torch.Generator(device='cuda').manual_seed(seed)
    pts = torch.rand(P, 3, dtype=torch.float64, device='cuda', generator=g) * 2 - 1
    phi = torch.arange(V, dtype=torch.float64, device='cuda') * (2 * np.pi / V)
    ctr = torch.stack([4 * torch.cos(phi), 0.3 * torch.sin(3 * phi), 4 * torch.sin(phi)], 1)
    if regime == 'dense':
        vis = torch.rand(V, P, device='cuda', generator=g) < 0.5
    else:                                                                   # a window of 4 to 8 neighbouring views per point
        first = torch.randint(0, V, (P,), device='cuda', generator=g)
        length = torch.randint(4, 9, (P,), device='cuda', generator=g)
        v = torch.arange(V, device='cuda').unsqueeze(1)
        vis = ((v - first.unsqueeze(0)) % V) < length.unsqueeze(0)
    return pts, ctr, vis.to(torch.uint8)


def torch_scores(pts, ctr, vis, chunk, theta0=5.0, s1=1.0, s2=10.0):
    """the same score by plain torch, `chunk` points at a time -> (scores fp64 [V,V], counts int64 [V,V])"""
    V = ctr.shape[0]
    S = torch.zeros(V, V, dtype=torch.int64, device=pts.device)
    C = torch.zeros(V, V, dtype=torch.int64, device=pts.device)
    for p0 in range(0, pts.shape[0], chunk):
        p = pts[p0:p0 + chunk]
        m = vis[:, p0:p0 + chunk].bool()
        d = ctr.unsqueeze(1) - p.unsqueeze(0)                               # [V, n, 3]
        u = d / d.norm(dim=2, keepdim=True).clamp_min(1e-300)
        dot = torch.einsum('inc,jnc->ijn', u, u)
        cr = torch.cross(u.unsqueeze(1).expand(V, V, -1, 3), u.unsqueeze(0).expand(V, V, -1, 3), dim=3).norm(dim=3)
        th = torch.atan2(cr, dot) * (180.0 / np.pi)
        s = torch.where(th <= theta0, s1, s2)
        w = torch.exp(-(th - theta0) ** 2 / (2 * s * s))
        both = m.unsqueeze(1) & m.unsqueeze(0)
        S += (torch.round(w * 2.0 ** 32).to(torch.int64) * both).sum(2)
        C += both.sum(2)
    S.fill_diagonal_(0)
    return S.double() * 2.0 ** -32, C


def timed(fn, repeats):
    fn()                                                                    # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        out = fn()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return out, ms


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--regimes', type=str, default='sparse,dense')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--chunk', type=int, default=None, help='points per step of the torch formulation (default: 2^25 / V^2)')
    ap.add_argument('--no_torch', action='store_true', help='time the kernel alone')
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), 'time_viewsel.py measures on the GPU'
    from mvsdf_amd import viewsel
    for regime in a.regimes.split(','):
        pts, ctr, vis = make(regime)
        V, P = vis.shape
        (s, c), k_ms = timed(lambda: viewsel.view_scores(pts, ctr, vis), a.repeats)
        res = {'regime': regime, 'V': V, 'P': P, 'views_per_point': round(float(vis.float().sum() / P), 2), 'repeats': a.repeats,
               'pair_terms': int((c.sum() - c.diagonal().sum()) // 2), 'kernel_ms': round(float(np.median(k_ms)), 3), 'kernel_runs': [round(v, 3) for v in k_ms]}
        if not a.no_torch:
            chunk = a.chunk or max(1, (1 << 25) // (V * V))
            (s_t, c_t), t_ms = timed(lambda: torch_scores(pts, ctr, vis, chunk), a.repeats)
            assert torch.equal(c, c_t), 'the torch formulation counts other common points'
            res.update({'torch_ms': round(float(np.median(t_ms)), 3), 'torch_runs': [round(v, 3) for v in t_ms], 'torch_chunk': chunk,
                        'max_abs_score_difference': float((s - s_t).abs().max()), 'torch_over_kernel': round(float(np.median(t_ms) / np.median(k_ms)), 2)})
        print(json.dumps(res), flush=True)
        del pts, ctr, vis


if __name__ == '__main__':
    main()
