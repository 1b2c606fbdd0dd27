#!/usr/bin/env python3
"""Re-select the source views of an MVS directory from a mesh of the scene, on the GPU:

    python tools/select_views.py MESH --data_root MVS_DIR [--num_pairs 10] [--out pair.txt] [--max_d 256]

MESH (OBJ / PLY, world coordinates) is drawn into the cameras MVS_DIR/cams/<id:08>_cam.txt at the size of MVS_DIR/images/; a vertex counts as a
point a view sees where raster.vertex_visibility says so, and the views are scored and chosen by mvsdf_amd/viewsel.py (view_scores, select_pairs):
the geometry of a first reconstruction in place of a sparse model's tracks.  The views and their ids are those of MVS_DIR/pair.txt.  The result
goes to --out (default: MVS_DIR/pair.txt, whose previous content is kept as pair.txt.bak)."""
import argparse
import os
import shutil
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('mesh', type=str)
    p.add_argument('--data_root', type=str, required=True, help='MVS directory with images/, cams/ and pair.txt')
    p.add_argument('--num_pairs', type=int, default=10)
    p.add_argument('--out', type=str, default=None)
    p.add_argument('--max_d', type=int, default=256, help='only read where a camera file does not state its own hypothesis count')
    return p


def main(argv=None):
    p = parser()
    a = p.parse_args(argv)
    pair_path = os.path.join(a.data_root, 'pair.txt')
    for f in (a.mesh, pair_path):
        if not os.path.exists(f):
            p.exit(1, 'select_views.py: %s: no such file\n' % f)
    import numpy as np
    from PIL import Image
    from mvsdf_amd import raster, viewsel
    from mvsdf_amd.mesh import load_mesh
    from mvsdf_amd.stereo import _find
    from mvsdf_amd.utils import io as sio
    ids = sio.load_pair(pair_path)['id_list']
    cams = np.stack([sio.load_cam(os.path.join(a.data_root, 'cams', '%s_cam.txt' % i.zfill(8)), a.max_d) for i in ids])
    sizes = set()
    for i in ids:
        with Image.open(_find(os.path.join(a.data_root, 'images'), i.zfill(8), ('.jpg', '.png'))) as im:
            sizes.add(im.size)
    if len(sizes) != 1:
        p.exit(1, 'select_views.py: the images under %s differ in size\n' % a.data_root)
    w, h = sizes.pop()
    mesh = load_mesh(a.mesh).to('cuda')
    r = raster.rasterize(mesh, cams=cams, hw=(h, w), pixel_center=0.5)
    vis = raster.vertex_visibility(mesh, r)
    scores, counts = viewsel.view_scores(mesh.vertices.double(), viewsel.centers_from_cams(cams), vis)
    pairs, pair_scores = viewsel.select_pairs(scores, counts, a.num_pairs)
    out = a.out or pair_path
    if os.path.abspath(out) == os.path.abspath(pair_path):
        shutil.copyfile(pair_path, pair_path + '.bak')
    viewsel.write_pair(out, ids, pairs, pair_scores)
    n = [len(q) for q in pairs]
    print('[select_views] %d views, %d vertices -> %s; %d to %d sources per view' % (len(ids), mesh.vertices.shape[0], out, min(n), max(n)))
    return pairs, pair_scores


if __name__ == '__main__':
    main()
