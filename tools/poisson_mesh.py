"""A mesh from an oriented point cloud on the device: Poisson reconstruction on a regular grid and marching cubes over the cells near the samples
(mvsdf_amd/poisson.py, which states the algorithm).  The paper's mesh baseline: the fused MVS cloud followed by Poisson reconstruction;
tools/eval_dtu.py scores the result.

    python tools/poisson_mesh.py IN.ply OUT.(ply|obj) [--depth 8] [--cycles 8] [--scale 1.1] [--no_trim] [--min_density D] [--dilate K] [--largest]
                                 [--estimate_normals [K]]
    python tools/poisson_mesh.py --data DIR OUT.(ply|obj) [--pair DIR/pair.txt] [--normal_jump 0.05] [fuse_depths' options] ...

IN.ply: a binary PLY point cloud with nx ny nz (tools/fusion.py --normals writes one; tools/clean_points.py keeps them).  --data DIR fuses DIR's
Vis-MVSNet depth maps with normals=True (tools/fusion.py's inputs and options) and reconstructs in one command.  The grid is a cube of 2^depth cells
per axis, --scale times the cloud's longest box edge, centred on the box.  --estimate_normals [K]: an IN.ply without nx ny nz gets normals from its K
(default 16) nearest neighbours and the spanning-tree orientation (mvsdf_amd/normals.py: estimate_normals + orient_normals, up = +z) instead of the
exit (give the flag after the paths, or as --estimate_normals=K); tools/estimate_normals.py has the other orientations.  Prints points used and outside, residual / residual0, the isovalue and the
face count.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('paths', type=str, nargs='+', help='IN.ply OUT, or with --data only OUT')
    ap.add_argument('--data', type=str, default=None, help='a Vis-MVSNet output directory: fuse it with normals instead of reading IN.ply')
    ap.add_argument('--depth', type=int, default=8, help='the grid has 2^depth cells per axis (2 .. 10)')
    ap.add_argument('--cycles', type=int, default=8)
    ap.add_argument('--sweeps', type=int, default=2)
    ap.add_argument('--scale', type=float, default=1.1)
    ap.add_argument('--no_trim', action='store_true', default=False, help='the watertight surface instead of the cells near the samples')
    ap.add_argument('--min_density', type=float, default=0.0)
    ap.add_argument('--dilate', type=int, default=1)
    ap.add_argument('--largest', action='store_true', default=False, help='keep the largest connected component')
    ap.add_argument('--estimate_normals', type=int, nargs='?', const=16, default=None, metavar='K',
                    help='IN.ply without nx ny nz: estimate them from K neighbours (default 16) and orient them')
    ap.add_argument('--pair', type=str, default=None, help='--data: default DATA/pair.txt')
    ap.add_argument('--normal_jump', type=float, default=0.05)
    ap.add_argument('--view', type=int, default=10, help='--data: fuse_depths\' sources per view')
    ap.add_argument('--vthresh', type=int, default=2)
    ap.add_argument('--pthresh', type=str, default='.8,.7,.8')
    ap.add_argument('--pix_thresh', type=float, default=1.0)
    ap.add_argument('--dep_thresh', type=float, default=0.01)
    a = ap.parse_args(argv)
    if len(a.paths) != (1 if a.data else 2):
        ap.error('give IN.ply OUT, or --data DIR OUT')
    a.input, a.output = (None, a.paths[0]) if a.data else a.paths
    if not a.output.lower().endswith(('.ply', '.obj')):
        ap.error('OUT must end in .ply or .obj')
    if a.input is not None and os.path.abspath(a.input) == os.path.abspath(a.output):
        ap.error('OUT must not be IN.ply')
    if not 2 <= a.depth <= 10:
        ap.error('--depth must be in 2 .. 10')
    if a.estimate_normals is not None and not 1 <= a.estimate_normals <= 32:
        ap.error('--estimate_normals K must be in 1 .. 32')
    if a.cycles < 0 or a.sweeps < 1 or a.dilate < 0:
        ap.error('--cycles must be >= 0, --sweeps >= 1, --dilate >= 0')
    if not a.scale >= 1 or a.scale == float('inf'):
        ap.error('--scale must be a finite number >= 1')
    a.pthresh = [float(v) for v in a.pthresh.split(',')]
    if len(a.pthresh) != 3:
        ap.error('--pthresh takes three comma-separated thresholds')
    return a


def main(argv=None):
    a = parse_args(argv)
    from mvsdf_amd import chamfer, fusion, poisson
    if a.data:
        from mvsdf_amd.datasets import prepare
        pair, cams, depths, probs = prepare.load_mvs_output(a.data, pair_file=a.pair)
        fused = fusion.fuse_depths(cams, depths, prepare.pair_indices(pair), probs=probs, pthresh=a.pthresh, view=a.view, vthresh=a.vthresh,
                                   pix_thresh=a.pix_thresh, dep_thresh=a.dep_thresh, normals=True, normal_jump=a.normal_jump)
        points, normals = fused.points, fused.normals
    else:
        points, normals = chamfer.load_oriented_points(a.input)
        if normals is None and a.estimate_normals is not None and len(points) > a.estimate_normals:
            from mvsdf_amd import normals as nrm
            est, _, neighbors = nrm.estimate_normals(points, a.estimate_normals)
            o = nrm.orient_normals(points, est, neighbors)
            normals = o.normals
            print('normals: estimated from %d neighbours, %d components oriented in %d rounds' % (a.estimate_normals, o.n_components, o.rounds))
        if normals is None:
            sys.exit('poisson_mesh: %s has no nx / ny / nz (tools/fusion.py --normals writes them)' % a.input)
    if len(points) == 0:
        sys.exit('poisson_mesh: the cloud is empty')
    mesh, field = poisson.poisson_mesh(points, normals, depth=a.depth, scale=a.scale, largest=a.largest, cycles=a.cycles, sweeps=a.sweeps,
                                       min_density=a.min_density, dilate=a.dilate, trim=not a.no_trim)
    n = 2 ** a.depth + 1
    print('grid: %d^3 lattice points of %.6g; points: %d used, %d outside' % (n, field.voxel, field.n_used, field.n_outside))
    ratio = field.residual / field.residual0 if field.residual0 > 0 else float('nan')
    print('residual / residual0: %.3g (%.6g / %.6g); isovalue %.9g' % (ratio, field.residual, field.residual0, field.iso))
    if mesh is None:
        sys.exit('poisson_mesh: no surface (nothing crosses the isovalue)')
    mesh.export(a.output)
    print('mesh: %d vertices, %d faces -> %s' % (mesh.vertices.shape[0], len(mesh), a.output))


if __name__ == '__main__':
    main()
