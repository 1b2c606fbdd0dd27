"""Per-stage device time of the on-device mesh extraction (mvsdf_amd/mesh.py) on the W = 256 synthetic model: the SDF volume, marching
cubes (count + scan, emit), components + selection, vertex colours, the device-to-host copy and the OBJ export.  Device events around
each stage; the kernels alone come from a separate `rocprofv3 --kernel-trace --stats` run of this script.

    python tools/time_mesh.py --resolution 512 [--repeats 3] [--out DIR] [--width 256]
    python tools/time_mesh.py --resolution 1024 --sparse [--block B --margin M]     # sparse_marching_cubes: its stages, points, peak memory
    python tools/time_mesh.py --resolution 512 --compare [--block B --margin M]     # dense and sparse alternating, arrays checked equal
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resolution', type=int, default=512)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None, help='directory for the OBJ and a JSON of the timings (default: a new temporary directory)')
    ap.add_argument('--width', type=int, default=256, help='hidden width of the synthetic model (8 layers; 512 = the shipped network)')
    ap.add_argument('--sparse', action='store_true', help='time mesh.sparse_marching_cubes per stage instead of the dense path')
    ap.add_argument('--compare', action='store_true', help='time dense and sparse extraction alternating in one process; check their arrays')
    ap.add_argument('--block', type=int, default=None, help='sparse block edge in cells (default mesh.SPARSE_BLOCK)')
    ap.add_argument('--margin', type=float, default=None, help='sparse seeding margin (default mesh.SPARSE_MARGIN)')
    a = ap.parse_args()
    from mvsdf_amd import mesh as M
    from mvsdf_amd.model.implicit_differentiable_renderer import IDRNetwork
    from mvsdf_amd.utils import plots, synth
    from mvsdf_amd.utils.config import ConfigDict
    assert torch.cuda.is_available(), 'time_mesh.py measures on the GPU'
    W, n = a.width, a.resolution
    m = IDRNetwork(ConfigDict(synth.model_conf(W)))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(W, 0).items()})
    m = m.cuda().eval()
    x = np.linspace(-1.0, 1.0, n)
    out_dir = a.out or tempfile.mkdtemp(prefix='time_mesh_')
    os.makedirs(out_dir, exist_ok=True)
    block = M.SPARSE_BLOCK if a.block is None else a.block
    margin = M.SPARSE_MARGIN if a.margin is None else a.margin
    if a.sparse or a.compare:
        return time_sparse(a, M, m, n, W, block, margin, out_dir)
    rows = []
    for rep in range(a.repeats + 1):                                  # the first round warms up
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        ev[0].record()
        vol = plots.surface_volume_device(m, n)
        ev[1].record()
        mesh = M.marching_cubes(vol, 0.0, (x[2] - x[1],) * 3, (x[0],) * 3)
        ev[2].record()
        mesh.vertex_colors = plots.surface_vertex_colors(m, mesh.vertices)
        ev[3].record()
        big = mesh.largest_component()
        ev[4].record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = big.to('cpu')
        t1 = time.perf_counter()
        path = os.path.join(out_dir, 'mesh_%d.obj' % n)
        host.export(path)
        t2 = time.perf_counter()
        r = {'sdf_volume_ms': ev[0].elapsed_time(ev[1]), 'marching_cubes_ms': ev[1].elapsed_time(ev[2]), 'colors_ms': ev[2].elapsed_time(ev[3]),
             'components_select_ms': ev[3].elapsed_time(ev[4]), 'd2h_ms': 1e3 * (t1 - t0), 'export_ms': 1e3 * (t2 - t1),
             'vertices': int(mesh.vertices.shape[0]), 'faces': int(mesh.faces.shape[0]), 'largest_vertices': int(big.vertices.shape[0]),
             'largest_faces': int(big.faces.shape[0]), 'obj_bytes': os.path.getsize(path)}
        if rep:
            rows.append(r)
        del vol
    med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
    # marching cubes includes the one host wait for the counts (mvsdf_amd/mesh.py); the kernels alone: rocprofv3 --kernel-trace --stats
    res = {'resolution': n, 'W': W, 'median': med, 'runs': rows}
    print(json.dumps(res))
    with open(os.path.join(out_dir, 'time_mesh_%d.json' % n), 'w') as f:
        json.dump(res, f, indent=1)
    v = np.array([[float(t) for t in line.split()[1:4]] for line in open(path) if line.startswith('v ')], np.float32)
    assert np.array_equal(v, host.vertices.numpy()), 'the OBJ does not read back'
    print('OBJ read back: %d vertices (%s)' % (len(v), path))


def _dense_mesh(M, plots, m, n):
    x = np.linspace(-1.0, 1.0, n)
    return M.marching_cubes(plots.surface_volume_device(m, n), 0.0, (x[2] - x[1],) * 3, (x[0],) * 3)


def time_sparse(a, M, m, n, W, block, margin, out_dir):
    """--sparse: per-stage device times of sparse_marching_cubes (events inside it), points evaluated, peak device memory.
    --compare: dense (SDF volume + marching cubes) and sparse end to end, alternating, each between two events; their arrays must be equal."""
    from mvsdf_amd.utils import plots
    rows = []
    for rep in range(a.repeats + 1):                                  # the first round warms up
        r = {}
        if a.compare:
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            torch.cuda.reset_peak_memory_stats()
            ev[0].record()
            dense = _dense_mesh(M, plots, m, n)
            ev[1].record()
            torch.cuda.synchronize()
            r['dense_peak_bytes'] = torch.cuda.max_memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            st = {}
            ev[2].record()
            sp = M.sparse_marching_cubes(m.implicit_network.native_sdf(), n, 0.0, block=block, margin=margin, stats=st)
            ev[3].record()
            torch.cuda.synchronize()
            for u, v, what in [(dense.vertices, sp.vertices, 'vertices'), (dense.normals, sp.normals, 'normals'), (dense.faces, sp.faces, 'faces')]:
                assert torch.equal(u, v), 'dense and sparse %s differ' % what
            r.update(dense_ms=ev[0].elapsed_time(ev[1]), sparse_ms=ev[2].elapsed_time(ev[3]))
            del dense
        else:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            st = {'time_stages': True}
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            sp = M.sparse_marching_cubes(m.implicit_network.native_sdf(), n, 0.0, block=block, margin=margin, stats=st)
            ev[1].record()
            torch.cuda.synchronize()
            r.update({k + '_ms': v for k, v in st.pop('stage_ms').items()})
            r['sparse_ms'] = ev[0].elapsed_time(ev[1])
        r.update(sparse_peak_bytes=torch.cuda.max_memory_allocated(), points_evaluated=st['points_evaluated'], seeds=st['seeds'],
                 active_blocks=st['active_blocks'], closure_rounds=st['closure_rounds'], workspace_bytes=st['workspace_bytes'],
                 vertices=int(sp.vertices.shape[0]), faces=int(sp.faces.shape[0]))
        if rep:
            rows.append(r)
        del sp
    med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
    res = {'resolution': n, 'W': W, 'block': block, 'margin': margin, 'mode': 'compare' if a.compare else 'sparse',
           'points_fraction': med['points_evaluated'] / n ** 3, 'median': med, 'runs': rows}
    print(json.dumps(res))
    with open(os.path.join(out_dir, 'time_mesh_%s_%d_w%d.json' % (res['mode'], n, W)), 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
