"""Per-stage device time of the on-device mesh extraction (mvsdf_amd/mesh.py) on the W = 256 synthetic model: the SDF volume, marching
cubes (count + scan, emit), components + selection, vertex colours, the device-to-host copy and the OBJ export.  Device events around
each stage; the kernels alone come from a separate `rocprofv3 --kernel-trace --stats` run of this script.

    python tools/time_mesh.py --resolution 512 [--repeats 3] [--out DIR]
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
    a = ap.parse_args()
    from mvsdf_amd import mesh as M
    from mvsdf_amd.model.implicit_differentiable_renderer import IDRNetwork
    from mvsdf_amd.utils import plots, synth
    from mvsdf_amd.utils.config import ConfigDict
    assert torch.cuda.is_available(), 'time_mesh.py measures on the GPU'
    W, n = 256, a.resolution
    m = IDRNetwork(ConfigDict(synth.model_conf(W)))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(W, 0).items()})
    m = m.cuda().eval()
    x = np.linspace(-1.0, 1.0, n)
    out_dir = a.out or tempfile.mkdtemp(prefix='time_mesh_')
    os.makedirs(out_dir, exist_ok=True)
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


if __name__ == '__main__':
    main()
