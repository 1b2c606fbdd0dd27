"""Time of the Poisson reconstruction (mvsdf_amd/poisson.py, csrc/poisson.hip) on a synthetic oriented cloud: --points seeded points on a sphere of
radius 0.6 (noise of 0.002 along the normal) in the cube of half-edge 1, at every --depth.

Device events around the stages of one reconstruction (the splat with the right-hand side, the multigrid solve, the isovalue) and around
Field.mesh(), plus a host clock around the whole call (a synchronize closes the interval); medians after a warm-up.  The solve is a chain of
memory-bound fp64 stencil passes: solve_bytes is what its passes must move, computed from the shapes (a sweep reads x and b and writes x, the
residual reads x and b and writes r, the restriction reads r and writes the coarse b, the prolongation reads the coarse x and reads and writes x, a
coarse x is cleared once per cycle, the two diagnostic residuals read x and b), and solve_share is solve_bytes / time over --hbm_rate (the
achievable HBM rate of an MI355X, 6.3e12 bytes/s).  --numpy times tests/poisson_ref.py, the numpy restatement, on this host at those depths with
--numpy_points points: a CPU restatement for tests, not a competitor.  Every depth appends one JSON line to --out and prints it.

    python tools/time_poisson.py [--depth 8,9 --points 2000000 --cycles 8 --sweeps 2 --repeats 3] [--numpy 6,7] [--out profiles/poisson_time_lines.jsonl]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def cloud(n, seed=0, radius=0.6, noise=0.002):
    rs = np.random.RandomState(seed)
    nrm = rs.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return (radius + noise * rs.normal(size=(n, 1))) * nrm, nrm


def solve_bytes(depth, cycles, sweeps):
    """the bytes the solve's passes must move (the module doc)"""
    total = 0
    for level in range(depth - 1):                                          # the levels above the 3^3 one
        m = (2 ** (depth - level) + 1) ** 3 * 8
        mc = (2 ** (depth - level - 1) + 1) ** 3 * 8
        per_cycle = 2 * sweeps * 3 * m + 3 * m + (m + mc) + (mc + 2 * m) + (m if level else 0)
        total += cycles * per_cycle
    return total + (2 ** depth + 1) ** 3 * 8 * (1 + 2 * 2)                  # chi cleared, two diagnostic residuals


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--depth', type=str, default='8,9')
    ap.add_argument('--points', type=int, default=2000000)
    ap.add_argument('--cycles', type=int, default=8)
    ap.add_argument('--sweeps', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--hbm_rate', type=float, default=6.3e12)
    ap.add_argument('--numpy', type=str, default='', help='depths at which to time the numpy restatement on this host, e.g. 6,7')
    ap.add_argument('--numpy_points', type=int, default=100000)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'poisson_time_lines.jsonl'))
    a = ap.parse_args(argv)
    import torch
    from mvsdf_amd import poisson
    origin, lines = np.array([-1.0, -1.0, -1.0]), []
    p, nrm = cloud(a.points, a.seed)
    pd, nd = torch.from_numpy(p).cuda(), torch.from_numpy(nrm).cuda()
    med = lambda v: float(np.median(v))                                    # noqa: E731
    for depth in [int(x) for x in a.depth.split(',') if x]:
        h = 2.0 / 2 ** depth
        stages = {k: [] for k in ('splat', 'solve', 'isovalue', 'mesh')}
        host, field, mesh = [], None, None
        for rep in range(a.repeats + 1):
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            t0 = time.perf_counter()
            call = poisson._Call(pd, nd, origin, h, depth, a.cycles, a.sweeps, 'time_poisson')
            ev[0].record()
            for k, stage in enumerate((poisson.STAGE_SPLAT, poisson.STAGE_SOLVE, poisson.STAGE_ISO)):
                call.run(stage)
                ev[k + 1].record()
            field = call.finish()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            m0 = torch.cuda.Event(enable_timing=True)
            m0.record()
            mesh = field.mesh()
            ev[4].record()
            torch.cuda.synchronize()
            if rep:
                host.append((t1 - t0) * 1e3)
                for k, name in enumerate(('splat', 'solve', 'isovalue')):
                    stages[name].append(ev[k].elapsed_time(ev[k + 1]))
                stages['mesh'].append(m0.elapsed_time(ev[4]))
            del call
        nbytes = solve_bytes(depth, a.cycles, a.sweeps)
        rate = nbytes / (med(stages['solve']) * 1e-3)
        line = dict(tool='time_poisson', depth=depth, lattice=2 ** depth + 1, points=a.points, cycles=a.cycles, sweeps=a.sweeps, n_used=field.n_used,
                    residual_ratio=field.residual / field.residual0, iso=field.iso, faces=0 if mesh is None else len(mesh),
                    reconstruct_host_ms=med(host), solve_bytes=nbytes, solve_bytes_per_s=rate, solve_share_of_hbm=rate / a.hbm_rate,
                    **{k + '_ms': med(v) for k, v in stages.items()})
        lines.append(line)
        print(json.dumps(line))
        del field, mesh
        torch.cuda.empty_cache()
    if a.numpy:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import poisson_ref
        q, qn = cloud(a.numpy_points, a.seed)
        for depth in [int(x) for x in a.numpy.split(',') if x]:
            t0 = time.perf_counter()
            out = poisson_ref.reconstruct(q, qn, origin, 2.0 / 2 ** depth, depth, a.cycles, a.sweeps)
            line = dict(tool='time_poisson', what='numpy restatement on the host CPU', depth=depth, points=a.numpy_points, cycles=a.cycles,
                        sweeps=a.sweeps, reconstruct_host_ms=(time.perf_counter() - t0) * 1e3, residual_ratio=out['residual'] / out['residual0'])
            lines.append(line)
            print(json.dumps(line))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'a') as fh:
        for line in lines:
            fh.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
