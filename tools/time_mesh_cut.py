"""Device time of mesh trimming (Mesh.cut_mask / Mesh.trim, csrc/mesh_cut.hip) on the largest component of the W = 256 synthetic model's mesh:
the cut (half-edge adjacency + terminal classes + push-relabel rounds + the final relabel; the call waits on the host once per relabel batch)
and the compaction (trim minus cut).  Device events around each call; the kernels alone come from a separate
`rocprofv3 --kernel-trace --stats` run of this script.  Prints one JSON line with the medians, the flow, the removed faces and the round counts.

    python tools/time_mesh_cut.py --resolution 512 [--repeats 5] [--thresh 15] [--smooth 10 2]

The model's own colours make every face bright (nothing is dark, the flow is 0); the 'field' rows give the same mesh colours from a smooth
field over the vertices, so that the flow and the rounds are those of a non-trivial cut.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resolution', type=int, default=512)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--thresh', type=int, default=15)
    ap.add_argument('--smooth', type=int, nargs='+', default=[10, 2])
    a = ap.parse_args()
    from mvsdf_amd.mesh import surface_mesh
    from mvsdf_amd.model.implicit_differentiable_renderer import IDRNetwork
    from mvsdf_amd.utils import synth
    from mvsdf_amd.utils.config import ConfigDict
    assert torch.cuda.is_available(), 'time_mesh_cut.py measures on the GPU'
    W = 256
    m = IDRNetwork(ConfigDict(synth.model_conf(W)))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(W, 0).items()})
    m = m.cuda().eval()
    mesh = surface_mesh(m, a.resolution).largest_component()
    res = {'resolution': a.resolution, 'W': W, 'faces': len(mesh), 'vertices': int(mesh.vertices.shape[0]), 'thresh': a.thresh, 'by_colors': {}}
    model_colors = mesh.vertex_colors
    for colors in ('model', 'field'):
        # 'model': the synthetic model's own (1 - s, s, 0); 'field': the same mesh with s from a smooth field over the vertices, so the cut is not trivial
        mesh.vertex_colors = model_colors if colors == 'model' else field_colors(mesh.vertices)
        res['by_colors'][colors] = time_cuts(mesh, a)
    print(json.dumps(res))


def field_colors(verts):
    s = torch.sigmoid(1.5 + 3.0 * torch.sin(verts.double() @ torch.tensor([7.0, -5.0, 4.0], dtype=torch.float64, device=verts.device))).float()
    return torch.stack([1 - s, s, torch.zeros_like(s)], 1).contiguous()


def time_cuts(mesh, a):
    out_rows = {}
    for smooth in a.smooth:
        rows = []
        for rep in range(a.repeats + 1):                          # the first round warms up
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            removed, flow = mesh.cut_mask(a.thresh, smooth)
            ev[1].record()
            stats = dict(mesh.cut_stats)
            ev[2].record()
            out = mesh.trim(a.thresh, smooth)
            ev[3].record()
            torch.cuda.synchronize()
            r = {'cut_ms': ev[0].elapsed_time(ev[1]), 'trim_ms': ev[2].elapsed_time(ev[3])}
            r['compaction_ms'] = r['trim_ms'] - r['cut_ms']
            r.update(stats)
            r['kept_faces'] = 0 if out is None else len(out)
            if rep:
                rows.append(r)
        med = {k: float(np.median([r[k] for r in rows])) for k in ('cut_ms', 'trim_ms', 'compaction_ms')}
        same = all(r[k] == rows[0][k] for r in rows for k in ('flow', 'removed', 'rounds', 'relabel_launches'))
        out_rows[smooth] = {'median': med, 'flow': rows[0]['flow'], 'removed': rows[0]['removed'], 'kept_faces': rows[0]['kept_faces'],
                                    'kept_vertices': rows[0]['kept_vertices'], 'rounds': rows[0]['rounds'],
                                    'relabel_launches': rows[0]['relabel_launches'], 'repeatable': same, 'runs': rows}
    return out_rows


if __name__ == '__main__':
    main()
