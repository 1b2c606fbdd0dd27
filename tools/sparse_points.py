#!/usr/bin/env python3
"""Sparse points from posed images on the GPU (mvsdf_amd/keypoints.py: keypoints, int8 MFMA matching, epipolar verification, tracks, triangulation):

    python tools/sparse_points.py MODEL_DIR IMAGE_DIR OUT_MODEL_DIR [--max_keypoints N --ratio R --max_epipolar E --max_reproj E --min_angle A --upright] [--refine]
    python tools/sparse_points.py --mvs_dir DIR --out OUT [--max_d 256 --interval_scale 1 --num_pairs 10] [the same options]

The first form takes a COLMAP model (cameras / images / points3D as .txt or .bin, pinhole cameras, points3D may be empty) and the images it names,
and writes OUT_MODEL_DIR/cameras.txt, images.txt and points3D.txt with the keypoints as observations and the triangulated points with their tracks:
what tools/colmap2mvs.py and tools/estimate_normals.py --colmap take.  The second form is BYOD.md's "suppose you have the camera files and the view
selection file" made into a command: DIR/images/<name>.jpg|png and DIR/cams/<name>_cam.txt (extrinsic and intrinsic; depth words are not needed)
-> OUT/pair.txt and OUT/cams/<name>_cam.txt with `depth_min interval max_d depth_max` from the points (mvsdf_amd/viewsel.py).  DIR's own cams/ are
never overwritten: OUT must be another directory.  --refine (first form): the cameras and points then go through bundle adjustment
(mvsdf_amd/bundle.py), the points are triangulated once more with the refined cameras and the written images carry the refined poses.  Prints views, keypoints, matches, verified matches, tracks and points."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('model_dir', nargs='?')
    p.add_argument('image_dir', nargs='?')
    p.add_argument('out_model_dir', nargs='?')
    p.add_argument('--mvs_dir', type=str, default=None, help='images/ + cams/ (the BYOD layout) instead of a COLMAP model')
    p.add_argument('--out', type=str, default=None, help='with --mvs_dir: where pair.txt and cams/ are written')
    p.add_argument('--max_keypoints', type=int, default=8192)
    p.add_argument('--ratio', type=float, default=0.8)
    p.add_argument('--max_epipolar', type=float, default=2.0)
    p.add_argument('--max_reproj', type=float, default=2.0)
    p.add_argument('--min_angle', type=float, default=1.5)
    p.add_argument('--upright', action='store_true', help='no keypoint orientation (cameras that share their up direction)')
    p.add_argument('--refine', action='store_true', help='bundle adjustment of the given poses and the points (first form only)')
    p.add_argument('--max_d', type=int, default=256, help='with --mvs_dir: depth hypotheses per view written into the camera files')
    p.add_argument('--interval_scale', type=float, default=1.0)
    p.add_argument('--num_pairs', type=int, default=10)
    return p


def _report(rep):
    print('[sparse_points] %(views)d views, %(keypoints)d keypoints, %(matches)d matches, %(verified)d verified matches, %(tracks)d tracks, %(points)d points' % rep)


def from_mvs_dir(a, options):
    import numpy as np
    from PIL import Image
    from mvsdf_amd import keypoints, viewsel
    from mvsdf_amd.stereo import _write_cam
    from mvsdf_amd.utils.io import load_cam
    if a.max_d < 2 or not a.interval_scale > 0:
        raise ValueError('sparse_points.py: max_d must be >= 2 and interval_scale > 0')
    if os.path.realpath(a.out) == os.path.realpath(a.mvs_dir):
        raise ValueError('sparse_points.py: --out must differ from --mvs_dir (the camera files there are never overwritten)')
    files = sorted(f for f in os.listdir(os.path.join(a.mvs_dir, 'images')) if os.path.splitext(f)[1].lower() in ('.jpg', '.jpeg', '.png'))
    if not files:
        raise FileNotFoundError('sparse_points.py: no jpg / png under %s' % os.path.join(a.mvs_dir, 'images'))
    stems = [os.path.splitext(f)[0] for f in files]
    images, cams = [], []
    for f, stem in zip(files, stems):
        with Image.open(os.path.join(a.mvs_dir, 'images', f)) as im:
            images.append(np.asarray(im.convert('RGB')))
        cams.append(load_cam(os.path.join(a.mvs_dir, 'cams', stem + '_cam.txt'), a.max_d))
    cams = np.stack(cams)
    rep = {}
    sp = keypoints.sparse_points(images, cams, report=rep, **options)
    _report(rep)
    tracks = (sp.track_off, sp.track_view)
    scores, counts = viewsel.view_scores(sp.xyz, viewsel.centers_from_cams(cams), tracks)
    pairs, pair_scores = viewsel.select_pairs(scores, counts, a.num_pairs)
    ranges = viewsel.depth_ranges(sp.xyz, tracks, cams[:, 0]).cpu().numpy()
    os.makedirs(os.path.join(a.out, 'cams'), exist_ok=True)
    for i, stem in enumerate(stems):
        cams[i, 1, 3] = ranges[i, 0], (ranges[i, 1] - ranges[i, 0]) / (a.max_d - 1) / a.interval_scale, a.max_d, ranges[i, 1]
        _write_cam(os.path.join(a.out, 'cams', stem + '_cam.txt'), cams[i])
    viewsel.write_pair(os.path.join(a.out, 'pair.txt'), ['%d' % int(s) if s.isdigit() else s for s in stems], pairs, pair_scores)
    return {'points': sp, 'cams': cams, 'pairs': pairs, 'report': rep}


def main(argv=None):
    p = parser()
    a = p.parse_args(argv)
    options = {'max_keypoints': a.max_keypoints, 'ratio': a.ratio, 'max_epipolar': a.max_epipolar, 'max_reproj': a.max_reproj, 'min_angle': a.min_angle,
               'upright': a.upright}
    if a.mvs_dir is not None:
        if a.out is None or a.model_dir is not None:
            p.exit(1, 'sparse_points.py: --mvs_dir DIR goes with --out OUT and without positional arguments\n')
        if a.refine:
            p.exit(1, 'sparse_points.py: --refine goes with a COLMAP model (the camera files of --mvs_dir are never rewritten)\n')
        return from_mvs_dir(a, options)
    if a.model_dir is None or a.image_dir is None or a.out_model_dir is None:
        p.exit(1, 'sparse_points.py: MODEL_DIR IMAGE_DIR OUT_MODEL_DIR, or --mvs_dir DIR --out OUT\n')
    from mvsdf_amd import keypoints
    from mvsdf_amd.datasets.colmap import load_colmap_model, write_colmap_text
    rep = {}
    model = keypoints.sparse_model(load_colmap_model(a.model_dir), a.image_dir, report=rep, **dict(options, **({'refine': True} if a.refine else {})))
    _report(rep)
    if a.refine:
        print('[sparse_points] refined: cost %(cost0).6g -> %(cost).6g in %(accepted)d accepted steps, %(points)d points' % rep['refine'])
    write_colmap_text(model, a.out_model_dir)
    return {'model': model, 'report': rep}


if __name__ == '__main__':
    main()
