#!/usr/bin/env python3
"""Align two clouds or meshes that nothing relates yet, on the GPU (mvsdf_amd.global_reg.global_register, whose docstring is the definition): FPFH
descriptors, nearest descriptors, RANSAC over the correspondences, then point-to-point ICP.

    python tools/align_clouds.py SRC DST --voxel V [--out T.txt] [--no_refine] [--seed S] [--hypotheses H]

SRC, DST: point-cloud PLY files, or meshes (OBJ / PLY), of which the vertices are taken.  V: the edge of the voxel filter both are reduced with, in
the clouds' unit; a few times the point spacing, so that some thousand to some ten thousand points remain.  The two must have the same scale.  Prints
the 4x4 matrix that takes SRC into DST's frame, then `inliers`, `fitness` and `rmse` (the last two are ICP's; `nan` with --no_refine).  --out writes
the matrix as a one-camera trajectory in the .log format registration.load_trajectory reads (a line `0 0 1`, then the four rows), which
tools/eval_tnt.py --traj and registration.tnt_evaluate's init take."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def load_cloud(path):
    """the points of a PLY cloud, or the vertices of a mesh -> fp64 numpy [N, 3]"""
    from mvsdf_amd.chamfer import load_points
    from mvsdf_amd.mesh import load_mesh
    if path.lower().endswith('.obj'):
        return load_mesh(path).vertices.double().cpu().numpy()
    return load_points(path)


def write_matrix(path, T):
    with open(path, 'w') as f:
        f.write('0 0 1\n')
        for row in T:
            f.write(' '.join(repr(float(x)) for x in row) + '\n')


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('src', type=str)
    p.add_argument('dst', type=str)
    p.add_argument('--voxel', type=float, required=True)
    p.add_argument('--out', type=str, default=None)
    p.add_argument('--no_refine', action='store_true')
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--hypotheses', type=int, default=100000)
    args = p.parse_args(argv)
    for path in (args.src, args.dst):
        if not os.path.exists(path):
            p.exit(1, 'align_clouds.py: %s: no such file\n' % path)
    if not args.voxel > 0:
        p.exit(1, 'align_clouds.py: --voxel must be positive\n')
    from mvsdf_amd import global_reg
    r = global_reg.global_register(load_cloud(args.src), load_cloud(args.dst), args.voxel, hypotheses=args.hypotheses, seed=args.seed,
                                   refine=not args.no_refine)
    for row in r.transformation:
        print(' '.join(repr(float(x)) for x in row))
    nan = float('nan')
    print('inliers %d' % r.inliers)
    print('fitness %r' % (nan if r.fitness is None else r.fitness))
    print('rmse %r' % (nan if r.inlier_rmse is None else r.inlier_rmse))
    if args.out:
        write_matrix(args.out, r.transformation)
    return r


if __name__ == '__main__':
    main()
