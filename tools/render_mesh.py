#!/usr/bin/env python3
"""Render a mesh into the input views of a scene, on the GPU: depth maps and, optionally, silhouettes.

    python tools/render_mesh.py IN --data_dir SCENE --out DIR [--mask_dir DIR]

IN is a mesh in world coordinates (OBJ / PLY).  It is drawn into the cameras of SCENE/cameras_hd.npz (world_mat_i, pixel centres at integer
coordinates) at the size of SCENE/image_hd/ (mvsdf_amd/raster.py states the definition).  DIR/depth/NNN.pfm is the depth along the camera axis,
0 where the mesh is not seen.  With --mask_dir the silhouettes are written there as NNN.png (255 inside)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('in_file', type=str)
    p.add_argument('--data_dir', type=str, required=True, help='scene directory with image_hd/ and cameras_hd.npz')
    p.add_argument('--out', type=str, required=True, help='output directory; depth maps go to OUT/depth/NNN.pfm')
    p.add_argument('--mask_dir', type=str, default=None,
                   help='also write the silhouettes here as NNN.png.  Pointing it at SCENE/pmask gives a scene prepared from one\'s own data the '
                        'masks tools/eval.py --eval_rendering needs; the PSNR is then taken inside the reconstruction\'s own silhouette, not inside '
                        'an independent ground-truth mask.  A directory that already holds images is refused.')
    return p


def main(argv=None):
    p = parser()
    args = p.parse_args(argv)
    if not os.path.exists(args.in_file):
        p.exit(1, 'render_mesh.py: %s: no such file\n' % args.in_file)
    import numpy as np
    from PIL import Image
    from mvsdf_amd import raster
    from mvsdf_amd.mesh import load_mesh
    from mvsdf_amd.utils import io as sio
    if args.mask_dir is not None and os.path.isdir(args.mask_dir) and sio.glob_imgs(args.mask_dir):
        p.exit(1, 'render_mesh.py: %s already holds images; silhouettes are not written over existing masks\n' % args.mask_dir)
    P, images, _ = raster.scene_views(args.data_dir, masks=False)
    mesh = load_mesh(args.in_file).to('cuda')
    r = raster.rasterize(mesh, P=P, hw=images.shape[1:3], pixel_center=0.0)
    depth = r.depth.cpu().numpy()
    sil = r.silhouette().cpu().numpy()
    os.makedirs(os.path.join(args.out, 'depth'), exist_ok=True)
    for i in range(len(depth)):
        sio.write_pfm(os.path.join(args.out, 'depth', '%03d.pfm' % i), np.ascontiguousarray(depth[i]))
    if args.mask_dir is not None:
        os.makedirs(args.mask_dir, exist_ok=True)
        for i in range(len(sil)):
            Image.fromarray(sil[i].astype(np.uint8) * 255).save(os.path.join(args.mask_dir, '%03d.png' % i))
    print('[render] %d views of %d x %d, %.1f %% of the pixels covered' % (len(depth), depth.shape[2], depth.shape[1], 100.0 * sil.mean()))
    return r


if __name__ == '__main__':
    main()
