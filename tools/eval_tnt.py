#!/usr/bin/env python3
"""Tanks and Temples evaluation on the GPU: registration to the ground truth, crop, precision / recall / F-score at tau
(mvsdf_amd.registration.tnt_evaluate, whose docstring is the definition):

    python tools/eval_tnt.py REC --scene_dir DIR --scene NAME [--tau T] [--traj LOG] [--mode mesh|pcd] [--out DIR]

REC: a mesh (OBJ / PLY) in mode mesh, a point cloud PLY (or the vertices of an OBJ) in mode pcd.  DIR holds the benchmark's files of the scene:
NAME.ply (ground truth), NAME.json (the crop volume), NAME_trans.txt (COLMAP's frame -> the ground truth's) and, for --traj, NAME_COLMAP_SfM.log.
Without --traj the reconstruction is taken to live in the frame of the benchmark's COLMAP poses and the initial alignment is NAME_trans.txt alone;
with --traj LOG (the cameras the reconstruction was made with, in the .log format) the camera centres of LOG are first aligned to COLMAP's in closed
form (registration.align_centres; the toolbox uses RANSAC there).  tau defaults to the scene's (registration.TNT_TAU, as recalled from the toolbox).
Prints 'precision recall fscore'; with --out writes DIR/NAME.precision.txt, NAME.recall.txt (edge and count per line), NAME.transformation.txt and
NAME.fscore.txt."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('rec', type=str)
    p.add_argument('--scene_dir', type=str, default='.')
    p.add_argument('--scene', type=str, required=True)
    p.add_argument('--tau', type=float, default=None)
    p.add_argument('--traj', type=str, default=None)
    p.add_argument('--mode', type=str, default='mesh', choices=['mesh', 'pcd'])
    p.add_argument('--max_points', type=int, default=None, help='the point limit of the third registration stage')
    p.add_argument('--out', type=str, default=None)
    args = p.parse_args(argv)
    from mvsdf_amd import registration as reg
    for path in [args.rec] + ([args.traj] if args.traj else []):
        if not os.path.exists(path):
            p.exit(1, 'eval_tnt.py: %s: no such file\n' % path)
    base = os.path.join(args.scene_dir, args.scene)
    for ext in ('.ply', '.json', '_trans.txt') + (('_COLMAP_SfM.log',) if args.traj else ()):
        if not os.path.exists(base + ext):
            p.exit(1, 'eval_tnt.py: %s: no such file (scene %s)\n' % (base + ext, args.scene))
    tau = args.tau if args.tau is not None else reg.TNT_TAU.get(args.scene)
    if tau is None:
        p.exit(1, 'eval_tnt.py: no default tau for scene %s (known: %s): pass --tau\n' % (args.scene, ', '.join(sorted(reg.TNT_TAU))))
    if not tau > 0:
        p.exit(1, 'eval_tnt.py: --tau must be positive\n')
    scene = reg.load_tnt_scene(args.scene_dir, args.scene)
    init = scene['trans']
    if args.traj:
        import numpy as np
        mine, theirs = reg.load_trajectory(args.traj), scene['trajectory']
        if len(mine) != len(theirs):
            p.exit(1, 'eval_tnt.py: %s holds %d cameras, the scene\'s COLMAP trajectory %d\n' % (args.traj, len(mine), len(theirs)))
        align = reg.align_centres(np.stack([m[:3, 3] for _, m in mine]), np.stack([m[:3, 3] for _, m in theirs]))
        init = np.array(reg.compose(reg._matrix(init, 'eval_tnt'), reg._matrix(align, 'eval_tnt')))
    from mvsdf_amd.chamfer import load_points
    from mvsdf_amd.mesh import load_mesh
    if args.mode == 'mesh':
        geometry = load_mesh(args.rec).to('cuda')
    elif args.rec.lower().endswith('.obj'):
        geometry = load_mesh(args.rec).vertices.double()
    else:
        geometry = load_points(args.rec)
    kw = {} if args.max_points is None else {'max_points': args.max_points}
    r = reg.tnt_evaluate(geometry, scene['gt'], scene['crop'], init, tau, **kw)
    print(r['precision'], r['recall'], r['fscore'])
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        stem = os.path.join(args.out, args.scene)
        for name, hist in zip(('precision', 'recall'), r['histograms']):
            with open('%s.%s.txt' % (stem, name), 'w') as f:
                for e, c in zip(r['edges'][:-1], hist):
                    f.write('%r %d\n' % (float(e), int(c)))
        with open(stem + '.transformation.txt', 'w') as f:
            for row in r['transformation']:
                f.write(' '.join(repr(float(x)) for x in row) + '\n')
        with open(stem + '.fscore.txt', 'w') as f:
            f.write('tau %r\nprecision %r\nrecall %r\nfscore %r\n' % (tau, r['precision'], r['recall'], r['fscore']))
    return r


if __name__ == '__main__':
    main()
