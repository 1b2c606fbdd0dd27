"""Device time of the mesh rendering kernels (mvsdf_amd/raster.py, csrc/raster.hip): draw, resolve, visibility and colours, each between two
device events after a warm-up, the work ending in a synchronise; the median of --repeats runs, one JSON line per mesh.

The meshes are mesh.sparse_marching_cubes of the synthetic model (--width) at --resolutions (512: about 10^6 vertices whose triangles cover a few
pixels each, the small path; 64: a coarse mesh whose triangles go to the large path), drawn into --views cameras on three rings around the
origin at --hw pixels (pixel centres at +0.5), coloured from random images.  --large_face_pixels takes a list: the values are timed alternating
within every repeat (the A/B that chose raster.LARGE_FACE_PIXELS).  --count also runs the draw once with and once without the plain-load test
before the atomic, counting the atomics issued and the covered pixels.  For the split by kernel run the script under
rocprofv3 --kernel-trace --stats in a run of its own (--repeats 1).

    python tools/time_raster.py [--resolutions 512,64 --views 49 --hw 1200,1600 --repeats 3 --large_face_pixels 16 --count]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def look_at(eye, target, hw, focal):
    """a pinhole camera at `eye` looking at `target`, z up -> P fp64 [4,4] whose row 2 is the depth along the axis"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    K = np.array([[focal, 0, hw[1] / 2.0], [0, focal, hw[0] / 2.0], [0, 0, 1.0]])
    P = np.eye(4)
    P[:3, :3] = K @ R
    P[:3, 3] = K @ (-R @ eye)
    return P


def ring_cameras(views, hw, distance=2.5):
    """`views` cameras on three rings (elevations -0.5, 0.2, 0.9 rad) looking at the origin; the unit ball about fills the image height"""
    focal = 0.9 * hw[0] * distance / 2.0
    P = []
    for i in range(views):
        el, az = (-0.5, 0.2, 0.9)[i % 3], 2.0 * np.pi * i / views
        P.append(look_at(distance * np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)]), (0, 0, 0), hw, focal))
    return np.stack(P)


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--resolutions', type=str, default='512,64')
    ap.add_argument('--views', type=int, default=49)
    ap.add_argument('--hw', type=str, default='1200,1600')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--width', type=int, default=256, help='hidden width of the synthetic model')
    ap.add_argument('--large_face_pixels', type=str, default=None, help='comma-separated thresholds to alternate (default: raster.LARGE_FACE_PIXELS)')
    ap.add_argument('--view_chunk', type=int, default=None)
    ap.add_argument('--count', action='store_true', help='count atomics and covered pixels with and without the plain-load test')
    return ap


def _events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def main(argv=None):
    a = parser().parse_args(argv)
    assert torch.cuda.is_available(), 'time_raster.py measures on the GPU'
    from mvsdf_amd import mesh as M
    from mvsdf_amd import raster as R
    from mvsdf_amd._lib import check, lib
    from mvsdf_amd.model.implicit_differentiable_renderer import IDRNetwork
    from mvsdf_amd.utils import synth
    from mvsdf_amd.utils.config import ConfigDict
    hw = tuple(int(v) for v in a.hw.split(','))
    larges = [R.LARGE_FACE_PIXELS] if a.large_face_pixels is None else [int(v) for v in a.large_face_pixels.split(',')]
    m = IDRNetwork(ConfigDict(synth.model_conf(a.width)))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(a.width, 0).items()})
    m = m.cuda().eval()
    P = ring_cameras(a.views, hw)
    g = torch.Generator(device='cuda').manual_seed(0)
    images = torch.randint(0, 256, (a.views, hw[0], hw[1], 3), dtype=torch.uint8, device='cuda', generator=g)
    for n in [int(v) for v in a.resolutions.split(',')]:
        mesh = M.sparse_marching_cubes(m.implicit_network.native_sdf(), n, 0.0)
        nv, nf = mesh.vertices.shape[0], mesh.faces.shape[0]
        draw = {L: [] for L in larges}
        other = {'resolve_ms': [], 'visibility_ms': [], 'colors_ms': []}
        info = {}
        for rep in range(a.repeats + 1):                              # the first round warms up
            for L in larges:
                # rasterize = draw + resolve per view chunk; resolve is timed alone below and taken off
                ev = _events(2)
                ev[0].record()
                r = R.rasterize(mesh, P=P, hw=hw, large_face_pixels=L, view_chunk=a.view_chunk)
                ev[1].record()
                torch.cuda.synchronize()
                if rep:
                    draw[L].append(ev[0].elapsed_time(ev[1]))
                info[L] = r.stats['large_items']
            ev = _events(4)
            ws = torch.empty(256 + a.views * hw[0] * hw[1] * 8, dtype=torch.uint8, device='cuda')
            torch.cuda.synchronize()
            ev[0].record()
            st = torch.cuda.current_stream().cuda_stream
            d2, f2 = torch.empty_like(r.depth), torch.empty_like(r.face)
            done = 0
            while done < a.views:                                     # the resolve kernel over as many pixels as the draw resolved
                k = min(a.views - done, 65535)
                check(lib().mvsdf_raster_resolve(k, hw[0], hw[1], ws.data_ptr(), ws.numel(), d2[done:].data_ptr(), f2[done:].data_ptr(), st))
                done += k
            ev[1].record()
            vis = R.vertex_visibility(mesh, r)
            ev[2].record()
            col = R.color_vertices(mesh, images, raster=r)
            ev[3].record()
            torch.cuda.synchronize()
            del ws, d2, f2
            if rep:
                for k, name in enumerate(other):
                    other[name].append(ev[k].elapsed_time(ev[k + 1]))
        med = lambda v: round(float(np.median(v)), 3)                 # noqa: E731
        res = {'resolution': n, 'vertices': nv, 'faces': nf, 'views': a.views, 'hw': hw, 'repeats': a.repeats,
               'covered_fraction': round(float(r.silhouette().float().mean()), 4), 'visible_fraction': round(float(vis.float().mean()), 4),
               'colored_fraction': round(float((col.n_views > 0).float().mean()), 4),
               'rasterize_ms': {str(L): {'median': med(draw[L]), 'runs': [round(v, 3) for v in draw[L]], 'large_items': info[L]} for L in larges}}
        res.update({k: med(v) for k, v in other.items()})
        best = min(larges, key=lambda L: np.median(draw[L]))
        draw_ms = max(med(draw[best]) - res['resolve_ms'], 1e-6)
        res['draw_ms_at_%d' % best] = round(draw_ms, 3)
        res['face_views_per_s'] = round(nf * a.views / (draw_ms * 1e-3))
        if a.count:
            for name, pre in (('with_pretest', True), ('without_pretest', False)):
                c = R.rasterize(mesh, P=P, hw=hw, large_face_pixels=best, view_chunk=a.view_chunk, pretest=pre, stats=True)
                res[name] = {'atomics': c.stats['atomics'], 'covered': c.stats['covered']}
                assert torch.equal(c.depth, r.depth) and torch.equal(c.face, r.face)
        print(json.dumps(res), flush=True)
        del mesh, r, vis, col


if __name__ == '__main__':
    main()
