"""A mesh straight from Vis-MVSNet depth maps on the device: TSDF fusion into a voxel grid and marching cubes over the observed cells
(mvsdf_amd/tsdf.py, which states the algorithm).  The surface that tools/select_views.py, tools/render_mesh.py and tools/eval_dtu.py can use before
any training, and the paper's depth-map baseline.

    python tools/tsdf_mesh.py --data DIR [--pair DIR/pair.txt] [--resolution 256 | --voxel X] [--trunc_voxels 4] [--min_views 2]
                              [--bbox cloud|PLY] [--no_fuse] [--largest] [--simplify_faces N] [--color] [--out DIR/tsdf_mesh.ply]

Reads cam_<id:08>_flow3.txt, <id:08>_flow3.pfm and <id:08>_flow{1,2,3}_prob.pfm from DIR (prepare.load_mvs_output).  By default the depth maps go
through fuse_depths first (tools/fusion.py's options below) and its fused_depths are integrated; --no_fuse integrates the probability-masked raw
maps.  The grid covers the box of the fused cloud (--bbox cloud) or of a given point-cloud PLY such as cut.ply, padded by the truncation band.
--simplify_faces N reduces the mesh to at most N faces (Mesh.simplify) before colouring and writing.  --color takes vertex colours from DIR's <id:08>.jpg|png resized to the depth-map size (raster.color_vertices).  Prints voxels, valid share,
vertices and faces.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--data', type=str, required=True)
    ap.add_argument('--pair', type=str, default=None, help='default: DATA/pair.txt')
    ap.add_argument('--resolution', type=int, default=None, help='cells along the box\'s longest edge (default 256 unless --voxel is given)')
    ap.add_argument('--voxel', type=float, default=None, help='the voxel edge in world units')
    ap.add_argument('--trunc_voxels', type=float, default=4.0, help='the truncation distance in voxels')
    ap.add_argument('--min_views', type=int, default=2)
    ap.add_argument('--bbox', type=str, default='cloud', help='"cloud": the fused cloud\'s box; or a point-cloud PLY such as cut.ply')
    ap.add_argument('--no_fuse', action='store_true', default=False, help='integrate the masked raw depth maps instead of fuse_depths\' fused ones')
    ap.add_argument('--largest', action='store_true', default=False, help='keep the largest connected component')
    ap.add_argument('--simplify_faces', type=int, default=None, help='at most this many faces (Mesh.simplify(target_faces=N)), before --color')
    ap.add_argument('--color', action='store_true', default=False)
    ap.add_argument('--out', type=str, default=None, help='default: DATA/tsdf_mesh.ply (.ply or .obj)')
    ap.add_argument('--view', type=int, default=10, help='fuse_depths: sources per view')
    ap.add_argument('--vthresh', type=int, default=2)
    ap.add_argument('--pthresh', type=str, default='.8,.7,.8')
    ap.add_argument('--pix_thresh', type=float, default=1.0)
    ap.add_argument('--dep_thresh', type=float, default=0.01)
    a = ap.parse_args(argv)
    if a.resolution is not None and a.voxel is not None:
        ap.error('give either --resolution or --voxel')
    if a.resolution is None and a.voxel is None:
        a.resolution = 256
    if a.simplify_faces is not None and a.simplify_faces < 1:
        ap.error('--simplify_faces must be >= 1')
    if not a.trunc_voxels > 0:
        ap.error('--trunc_voxels must be > 0')
    a.pthresh = [float(v) for v in a.pthresh.split(',')]
    if len(a.pthresh) != 3:
        ap.error('--pthresh takes three comma-separated thresholds')
    return a


def find_images(data, ids):
    """the <id:08>.jpg|png of every view, or None when one view has neither (as tools/fusion.py)"""
    paths = []
    for i in ids:
        found = [p for p in (os.path.join(data, '%s.%s' % (i.zfill(8), e)) for e in ('jpg', 'png')) if os.path.exists(p)]
        if not found:
            return None
        paths.append(found[0])
    return paths


def main(argv=None):
    a = parse_args(argv)
    import math
    import numpy as np
    from mvsdf_amd import chamfer, fusion, raster, tsdf
    from mvsdf_amd.datasets import prepare
    pair, cams, depths, probs = prepare.load_mvs_output(a.data, pair_file=a.pair)
    fused = fusion.fuse_depths(cams, depths, prepare.pair_indices(pair), probs=probs, pthresh=a.pthresh, view=a.view, vthresh=a.vthresh,
                               pix_thresh=a.pix_thresh, dep_thresh=a.dep_thresh)
    maps = fused.masked_depths if a.no_fuse else fused.fused_depths
    if a.bbox == 'cloud':
        if len(fused) == 0:
            sys.exit('tsdf_mesh: the fused cloud is empty, so it has no box (lower --vthresh, or give --bbox PLY)')
        lo, hi = fused.bbox()
    else:
        pts = chamfer.load_points(a.bbox)
        if len(pts) == 0:
            sys.exit('tsdf_mesh: %s holds no points' % a.bbox)
        lo, hi = pts.min(0), pts.max(0)
    pad = int(math.ceil(a.trunc_voxels)) + 1                                    # the band in front of and behind the outermost surface
    origin, h, dims = tsdf.grid_from_bbox(lo, hi, voxel=a.voxel, resolution=a.resolution, pad_voxels=pad)
    vol = tsdf.integrate_depths(cams, maps, origin, h, dims, trunc=a.trunc_voxels * h, min_views=a.min_views)
    print('voxels: %d x %d x %d of %.6g, valid share %.4f' % (dims + (h, vol.valid_share())))
    mesh = vol.mesh()
    if mesh is None:
        sys.exit('tsdf_mesh: no surface (no valid cell crosses zero)')
    if a.largest:
        mesh = mesh.largest_component()
    if a.simplify_faces is not None:
        before = len(mesh)
        mesh = mesh.simplify(target_faces=a.simplify_faces)
        if mesh is None:
            sys.exit('tsdf_mesh: --simplify_faces %d left no face' % a.simplify_faces)
        print('simplified: %d -> %d faces' % (before, len(mesh)))
    if a.color:
        paths = find_images(a.data, pair['id_list'])
        if paths is None:
            sys.exit('tsdf_mesh: --color needs an <id:08>.jpg|png for every view in %s' % a.data)
        hh, ww = depths.shape[1:]
        images = np.stack([prepare.resize_bilinear_u8(prepare.load_image_u8(p), ww, hh) for p in paths])
        mesh = raster.color_vertices(mesh, images, cams=cams)
    out = a.out or os.path.join(a.data, 'tsdf_mesh.ply')
    mesh.export(out)
    print('mesh: %d vertices, %d faces -> %s' % (mesh.vertices.shape[0], len(mesh), out))


if __name__ == '__main__':
    main()
