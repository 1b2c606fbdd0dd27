#!/usr/bin/env python3
"""DTU Chamfer evaluation on the GPU, with the argument names of DTUeval-python's eval.py:

    python tools/eval_dtu.py DATA --scan N --dataset_dir DIR [--mode mesh|pcd] [--downsample_density 0.2] [--patch_size 60] [--max_dist 20] [--seed 0]

DATA: a mesh (OBJ / PLY, as extract_world_mesh or tools/mesh_cut.py write it) in mode mesh, a point cloud PLY (or the vertices of an OBJ) in mode pcd.
DIR holds DTU's evaluation data: ObsMask/ObsMask{N}_10.mat, ObsMask/Plane{N}.mat and Points/stl/stl{N:03}_total.ply.  Prints
'mean_d2s mean_s2d overall' as the script does (mvsdf_amd.chamfer.dtu_chamfer; the script's shuffle is replaced by the seeded order)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('data', type=str)
    p.add_argument('--scan', type=int, default=1)
    p.add_argument('--mode', type=str, default='mesh', choices=['mesh', 'pcd'])
    p.add_argument('--dataset_dir', type=str, default='.')
    p.add_argument('--downsample_density', type=float, default=0.2)
    p.add_argument('--patch_size', type=float, default=60)
    p.add_argument('--max_dist', type=float, default=20)
    p.add_argument('--seed', type=int, default=0, help='the visiting order of the radius filter: ascending splitmix64(seed ^ i)')
    args = p.parse_args(argv)
    if not os.path.exists(args.data):
        p.exit(1, 'eval_dtu.py: %s: no such file\n' % args.data)
    stl_path = os.path.join(args.dataset_dir, 'Points', 'stl', 'stl{:03}_total.ply'.format(args.scan))
    if not os.path.exists(stl_path):
        p.exit(1, 'eval_dtu.py: %s: no such file\n' % stl_path)
    from mvsdf_amd.chamfer import dtu_chamfer, load_dtu_obs, load_points
    from mvsdf_amd.mesh import load_mesh
    if args.mode == 'mesh':
        geometry = load_mesh(args.data).to('cuda')
    elif args.data.lower().endswith('.obj'):
        geometry = load_mesh(args.data).vertices.double()
    else:
        geometry = load_points(args.data)
    obs_mask, bb, res, plane = load_dtu_obs(args.dataset_dir, args.scan)
    r = dtu_chamfer(geometry, load_points(stl_path), obs_mask, bb, res, plane, density=args.downsample_density, patch=args.patch_size,
                    max_dist=args.max_dist, seed=args.seed)
    print(r['mean_d2s'], r['mean_s2d'], r['overall'])


if __name__ == '__main__':
    main()
