#!/usr/bin/env python3
"""Give a mesh a texture atlas from the input photographs of a scene, on the GPU:

    python tools/texture_mesh.py IN OUT.obj --data_dir SCENE [--density D] [--max_size S] [--faces N | --cell C] [--no_masks]
                                 [--level_seams [--seam_smoothness L]] [--charts [--chart_pad P] [--min_chart_faces N]]

IN is any mesh in world coordinates that load_mesh reads (OBJ / PLY), for example the evaluation's surface_world_coordinates_<epoch>.obj.  With
--faces N or --cell C it is simplified first (Mesh.simplify(target_faces=N) / (cell=C)).  The mesh is drawn into the cameras of
SCENE/cameras_hd.npz (world_mat_i, pixel centres at integer coordinates); every face takes the view of SCENE/image_hd/ that sees it largest and
gets a patch of the atlas at --density texels per image pixel (mvsdf_amd/texture.py states the definition).  Visibility is also masked by
SCENE/mask_hd/ unless --no_masks.  Faces that no view sees are grey.  With --level_seams the
colours are levelled across the label boundaries (mvsdf_amd/seams.py; only the PNG's colours change).  With --charts connected faces of one view share
one rectangle cut from that photograph with a margin of --chart_pad texels (1, 2, 4 or 8: the atlas is safe to mip level log2 of it), after charts
of fewer than --min_chart_faces faces have been absorbed by their neighbours (mvsdf_amd/charts.py).  Written: OUT.obj with vt / mtllib, OUT.mtl and OUT.png beside it."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('in_file', type=str)
    p.add_argument('out_file', type=str)
    p.add_argument('--data_dir', type=str, required=True, help='scene directory with image_hd/, mask_hd/ and cameras_hd.npz')
    p.add_argument('--density', type=float, default=1.0, help='texels per image pixel along a face\'s longest edge')
    p.add_argument('--max_size', type=int, default=8192, help='the atlas is at most this many texels wide; the density is halved until it fits')
    g = p.add_mutually_exclusive_group()
    g.add_argument('--faces', type=int, default=None, help='simplify to at most N faces first (Mesh.simplify(target_faces=N))')
    g.add_argument('--cell', type=float, default=None, help='simplify on a grid of this edge first (Mesh.simplify(cell=C))')
    p.add_argument('--no_masks', default=False, action='store_true', help='do not restrict visibility to mask_hd/')
    p.add_argument('--depth_tol', type=float, default=0.01, help='a vertex is visible when its depth is within (1 + depth_tol) of the drawn depth')
    p.add_argument('--cos_min', type=float, default=0.0, help='views whose ray meets the face normal at a cosine not above this are left out')
    p.add_argument('--ignore_normals', default=False, action='store_true', help='faces with a zero normal take every view that sees them')
    p.add_argument('--level_seams', default=False, action='store_true', help='level exposure differences across label boundaries (seams.level_atlas)')
    p.add_argument('--seam_smoothness', type=float, default=None, help='the weight of the smoothness entries of the levelling (default 0.1)')
    p.add_argument('--charts', default=False, action='store_true', help='one rectangle per connected region of a view instead of one patch per face (charts.py)')
    p.add_argument('--chart_pad', type=int, default=None, choices=(1, 2, 4, 8), help='margin and alignment of a chart\'s rectangle in texels (default 4)')
    p.add_argument('--min_chart_faces', type=int, default=None, help='charts of fewer faces are absorbed by their neighbours (default 4; 1: none)')
    return p


def main(argv=None):
    p = parser()
    args = p.parse_args(argv)
    if not os.path.exists(args.in_file):
        p.exit(1, 'texture_mesh.py: %s: no such file\n' % args.in_file)
    if os.path.splitext(args.out_file)[1].lower() != '.obj':
        p.exit(1, 'texture_mesh.py: %s: the output is an .obj (with its .mtl and .png beside it)\n' % args.out_file)
    if args.seam_smoothness is not None and not args.level_seams:
        p.exit(1, 'texture_mesh.py: --seam_smoothness needs --level_seams\n')
    if (args.chart_pad is not None or args.min_chart_faces is not None) and not args.charts:
        p.exit(1, 'texture_mesh.py: --chart_pad and --min_chart_faces need --charts\n')
    from mvsdf_amd import texture
    from mvsdf_amd.mesh import load_mesh
    mesh = load_mesh(args.in_file).to('cuda')
    if args.faces is not None or args.cell is not None:
        n = len(mesh)
        mesh = mesh.simplify(cell=args.cell, target_faces=args.faces)
        if mesh is None:
            p.exit(1, 'texture_mesh.py: no face survives the simplification\n')
        print('[texture] simplified: %d -> %d faces' % (n, len(mesh)))
    level, info = {}, {}
    if args.level_seams:
        level = dict(level_seams=True, level_options=dict(info=info, **({} if args.seam_smoothness is None else dict(smoothness=args.seam_smoothness))))
    cinfo = {}
    if args.charts:
        opts = dict(info=cinfo, **({} if args.chart_pad is None else dict(pad=args.chart_pad)))
        level.update(charts=True, chart_options=dict(opts, **({} if args.min_chart_faces is None else dict(min_faces=args.min_chart_faces))))
    out = texture.texture_mesh_from_scene(mesh, args.data_dir, masks=not args.no_masks, texel_density=args.density, max_size=args.max_size,
                                          depth_tol=args.depth_tol, cos_min=args.cos_min, ignore_normals=args.ignore_normals, **level)
    seen = int((out.face_view >= 0).sum())
    print('[texture] %d of %d faces textured from %d views; atlas %d x %d at %.6g texels per pixel, %.1f%% of its texels from photographs'
          % (seen, len(mesh), out.raster.depth.shape[0], out.texture.shape[1], out.texture.shape[0], out.density, 100.0 * float(out.valid.float().mean())))
    if args.charts:
        print('[texture] %d charts (%d before %d labels were absorbed)' % (cinfo['charts'], cinfo['charts_before'], sum(cinfo['changes'])))
    if args.level_seams:
        print('[texture] seams levelled: %d nodes, %d adjacency entries, %s iterations' % (info['nodes'], info['nnz'], '/'.join(str(i) for i in info['iterations'])))
    out.export(args.out_file)
    return out


if __name__ == '__main__':
    main()
