#!/usr/bin/env python3
"""Colour a mesh from the input photographs of a scene, on the GPU:

    python tools/color_mesh.py IN OUT --data_dir SCENE [--no_masks] [--depth_tol 0.01] [--cos_min 0.0]

IN is any mesh in world coordinates that load_mesh reads (OBJ / PLY), for example the evaluation's surface_world_coordinates_<epoch>.obj or a
trimmed one.  It is drawn into the cameras of SCENE/cameras_hd.npz (world_mat_i, pixel centres at integer coordinates); every vertex takes the
mean of SCENE/image_hd/ over the views that see it, weighted by the cosine between its normal and the viewing ray (mvsdf_amd/raster.py states the
definition).  Visibility is also masked by SCENE/mask_hd/ unless --no_masks.  Vertices that no view sees are grey.  OUT's format follows its
extension."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('in_file', type=str)
    p.add_argument('out_file', type=str)
    p.add_argument('--data_dir', type=str, required=True, help='scene directory with image_hd/, mask_hd/ and cameras_hd.npz')
    p.add_argument('--no_masks', default=False, action='store_true', help='do not restrict visibility to mask_hd/')
    p.add_argument('--depth_tol', type=float, default=0.01, help='a vertex is visible when its depth is within (1 + depth_tol) of the drawn depth')
    p.add_argument('--cos_min', type=float, default=0.0, help='views whose ray meets the normal at a cosine not above this are left out')
    p.add_argument('--ignore_normals', default=False, action='store_true', help='vertices with a zero normal take every view at weight 1')
    return p


def main(argv=None):
    p = parser()
    args = p.parse_args(argv)
    if not os.path.exists(args.in_file):
        p.exit(1, 'color_mesh.py: %s: no such file\n' % args.in_file)
    from mvsdf_amd import raster
    from mvsdf_amd.mesh import load_mesh
    mesh = load_mesh(args.in_file).to('cuda')
    out = raster.color_mesh_from_scene(mesh, args.data_dir, masks=not args.no_masks, depth_tol=args.depth_tol, cos_min=args.cos_min,
                                       ignore_normals=args.ignore_normals)
    seen = int((out.n_views > 0).sum())
    print('[color] %d of %d vertices coloured from %d views' % (seen, out.vertices.shape[0], out.raster.depth.shape[0]))
    out.export(args.out_file)
    return out


if __name__ == '__main__':
    main()
