"""The automatic cut of a point cloud (mvsdf_amd/cloud.py): all_torch.ply -> cut.ply with no mesh editor.

    python tools/clean_points.py IN.ply OUT.ply [--nb_neighbors 20] [--knn_ratio 3] [--eps_ratio 3] [--cluster_frac 1]

IN.ply: a binary or ASCII PLY point cloud (datasets/prepare.read_points); red / green / blue and nx / ny / nz of a binary file are kept.  Prints `N -> n_kept`, the
median neighbour distance, both radii and the cluster count.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('input', type=str)
    ap.add_argument('output', type=str)
    ap.add_argument('--nb_neighbors', type=int, default=20)
    ap.add_argument('--knn_ratio', type=float, default=3.0)
    ap.add_argument('--eps_ratio', type=float, default=3.0)
    ap.add_argument('--cluster_frac', type=float, default=1.0)
    a = ap.parse_args(argv)
    if not 1 <= a.nb_neighbors <= 32:
        ap.error('--nb_neighbors must be in 1 .. 32')
    for name in ('knn_ratio', 'eps_ratio', 'cluster_frac'):
        v = getattr(a, name)
        if not (v > 0 and v != float('inf')):
            ap.error('--%s must be a positive finite number' % name)
    if a.cluster_frac > 1:
        ap.error('--cluster_frac must be in (0, 1]')
    if os.path.abspath(a.input) == os.path.abspath(a.output):
        ap.error('OUT.ply must not be IN.ply')
    return a


def read_colors(path):
    """uint8 [N,3] of a binary PLY with red / green / blue, else None"""
    with open(path, 'rb') as fh:
        if b'format ascii' in fh.read(4096).split(b'end_header')[0]:
            return None
    import numpy as np
    from mvsdf_amd.mesh import _ply_elements
    vert = _ply_elements(path, 'clean_points')['vertex']
    if not all(k in vert.dtype.names for k in ('red', 'green', 'blue')):
        return None
    return np.ascontiguousarray(np.stack([vert[k] for k in ('red', 'green', 'blue')], 1).astype(np.uint8))


def read_normals(path):
    """fp64 [N,3] of a binary PLY with nx / ny / nz, else None"""
    with open(path, 'rb') as fh:
        if b'format ascii' in fh.read(4096).split(b'end_header')[0]:
            return None
    from mvsdf_amd.chamfer import load_oriented_points
    return load_oriented_points(path)[1]


def main(argv=None):
    a = parse_args(argv)
    from mvsdf_amd import cloud, fusion
    from mvsdf_amd.datasets import prepare
    pts = prepare.read_points(a.input)
    normals = read_normals(a.input)
    c = cloud.clean_points(pts, read_colors(a.input), nb_neighbors=a.nb_neighbors, knn_ratio=a.knn_ratio, eps_ratio=a.eps_ratio,
                           cluster_frac=a.cluster_frac)
    fusion.save_points(a.output, c.points, c.colors, normals=None if normals is None else normals[c.keep.cpu().numpy() != 0])
    print('%d -> %d points' % (len(pts), len(c)))
    print('median neighbour distance %.9g, sparse above %.9g, cluster radius %.9g' % (c.median, c.threshold, c.eps))
    print('%d points passed, %d clusters, the largest of %d points' % (c.n_passed, c.n_clusters, c.largest))
    print('wrote %s' % a.output)


if __name__ == '__main__':
    main()
