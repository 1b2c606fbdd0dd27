"""Normals for an unoriented point cloud on the GPU (mvsdf_amd/normals.py): k-nearest PCA and a consistent sign, so that any cloud can go to
tools/poisson_mesh.py.

    python tools/estimate_normals.py IN.ply OUT.ply [--k 16] [--orient mst|views|none] [--up x,y,z]
    python tools/estimate_normals.py --colmap MODEL_DIR OUT.ply [--k 16]
    python tools/estimate_normals.py --data_root MVS_DIR OUT.ply [--k 16] [--pair FILE]

IN.ply: a binary PLY point cloud (chamfer.load_points); nx ny nz it may carry are replaced.  --orient mst (the default for IN.ply): the spanning-tree
orientation, each component signed by --up (default 0,0,1) at its highest point; none: the canonical sign of the eigenvector.  --colmap MODEL_DIR
with no IN.ply takes the model's points3D and orients every point by its own track (orient_to_views): the way from a sparse model to a Poisson proxy
mesh, from which tools/select_views.py MESH re-selects views.  --data_root MVS_DIR with no IN.ply fuses the directory's Vis-MVSNet depth maps
(tools/fusion.py's defaults) and orients the spanning tree's components by the views the points were fused from (--orient views; mst and none as
above).  Prints the point count, the median surface variation, the component and round counts.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('paths', type=str, nargs='+', help='IN.ply OUT.ply, or with --colmap / --data_root only OUT.ply')
    ap.add_argument('--k', type=int, default=16, help='neighbours per point (1 .. 32)')
    ap.add_argument('--orient', type=str, default=None, choices=('mst', 'views', 'none'))
    ap.add_argument('--up', type=str, default='0,0,1')
    ap.add_argument('--colmap', type=str, default=None, help='a COLMAP model directory: its points3D, oriented by their tracks')
    ap.add_argument('--data_root', type=str, default=None, help='a Vis-MVSNet output directory: its fused points, oriented by their views')
    ap.add_argument('--pair', type=str, default=None, help='--data_root: default DATA_ROOT/pair.txt')
    a = ap.parse_args(argv)
    if a.colmap and a.data_root:
        ap.error('give --colmap or --data_root, not both')
    source = a.colmap or a.data_root
    if len(a.paths) != (1 if source else 2):
        ap.error('give IN.ply OUT.ply, or --colmap MODEL_DIR OUT.ply, or --data_root MVS_DIR OUT.ply')
    a.input, a.output = (None, a.paths[0]) if source else a.paths
    if not a.output.lower().endswith('.ply'):
        ap.error('OUT must end in .ply')
    if a.input is not None and os.path.abspath(a.input) == os.path.abspath(a.output):
        ap.error('OUT.ply must not be IN.ply')
    if not 1 <= a.k <= 32:
        ap.error('--k must be in 1 .. 32')
    if a.orient is None:
        a.orient = 'views' if source else 'mst'
    if a.orient == 'views' and not source:
        ap.error('--orient views needs the views: --colmap MODEL_DIR or --data_root MVS_DIR')
    if a.colmap and a.orient != 'views':
        ap.error('--colmap orients by the tracks (--orient views)')
    try:
        a.up = [float(v) for v in a.up.split(',')]
    except ValueError:
        ap.error('--up takes three comma-separated numbers')
    if len(a.up) != 3 or not all(v == v and abs(v) != float('inf') for v in a.up):
        ap.error('--up takes three finite comma-separated numbers')
    return a


def main(argv=None):
    a = parse_args(argv)
    import numpy as np
    from mvsdf_amd import chamfer, fusion, normals, viewsel
    centers = visibility = colors = None
    if a.colmap:
        from mvsdf_amd.datasets import colmap
        model = colmap.load_colmap_model(a.colmap, allow_distortion=True)
        _, _, cams, track_view = colmap.model_views(model)
        points, colors = model['points']['xyz'], model['points']['rgb']
        centers, visibility = viewsel.centers_from_cams(cams), (model['points']['track_off'], track_view)
    elif a.data_root:
        from mvsdf_amd.datasets import prepare
        pair, cams, depths, probs = prepare.load_mvs_output(a.data_root, pair_file=a.pair)
        fused = fusion.fuse_depths(cams, depths, prepare.pair_indices(pair), probs=probs)
        points, colors = fused.points, fused.colors
        centers, visibility = viewsel.centers_from_cams(cams), fused.view
    else:
        points = chamfer.load_points(a.input)
    if len(points) < a.k + 1:
        sys.exit('estimate_normals: %d points are too few for %d neighbours each' % (len(points), a.k))
    nrm, variation, neighbors = normals.estimate_normals(points, a.k)
    print('%d points, k = %d, median surface variation %.6g' % (len(points), a.k, float(variation.median())))
    if a.colmap:
        nrm = normals.orient_to_views(points, nrm, np.ascontiguousarray(centers), visibility)
        print('oriented by the tracks of %d views' % len(centers))
    elif a.orient != 'none':
        views = a.orient == 'views'
        o = normals.orient_normals(points, nrm, neighbors, up=a.up, centers=np.ascontiguousarray(centers) if views else None,
                                   visibility=visibility if views else None)
        nrm = o.normals
        print('oriented: %d components, %d rounds' % (o.n_components, o.rounds))
    fusion.save_points(a.output, points, colors, normals=nrm)
    print('wrote %s' % a.output)


if __name__ == '__main__':
    main()
