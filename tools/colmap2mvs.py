#!/usr/bin/env python3
"""A COLMAP sparse model and its images as MVS input, the view selection and the depth ranges computed on the GPU:

    python tools/colmap2mvs.py MODEL_DIR IMAGE_DIR OUT [--max_d 256] [--interval_scale 1] [--num_pairs 10] [--theta0 5 --sigma1 1 --sigma2 10]
                               [--undistort [--blank_pixels 0 --min_scale 0.2 --max_scale 2]] [--triangulate]

MODEL_DIR holds cameras / images / points3D as .txt or .bin (pinhole cameras; with --undistort the images of distorted cameras are resampled to
pinhole views on the GPU first, as tools/undistort.py does, and written as png), IMAGE_DIR the images the model names.  Writes
OUT/images/<i:08>.jpg|png, OUT/cams/<i:08>_cam.txt and OUT/pair.txt, the directory tools/mvs_depth.py starts from; the views are the images by
ascending COLMAP id, renumbered from 0.  --triangulate: the model's points3D (which may be empty) are replaced by points triangulated from the images
with the model's poses (mvsdf_amd/keypoints.py) before the view selection.  mvsdf_amd/datasets/colmap.py and mvsdf_amd/viewsel.py state what is computed."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('model_dir', type=str)
    p.add_argument('image_dir', type=str)
    p.add_argument('out_root', type=str)
    p.add_argument('--max_d', type=int, default=256, help='depth hypotheses per view (0, the automatic count of MVSNet\'s script, is not built)')
    p.add_argument('--interval_scale', type=float, default=1.0)
    p.add_argument('--num_pairs', type=int, default=10, help='source views listed per view')
    p.add_argument('--theta0', type=float, default=5.0)
    p.add_argument('--sigma1', type=float, default=1.0)
    p.add_argument('--sigma2', type=float, default=10.0)
    p.add_argument('--undistort', action='store_true', help='resample the images of distorted cameras to pinhole views (mvsdf_amd/undistort.py)')
    p.add_argument('--blank_pixels', type=float, default=0.0, help='with --undistort: 0 no blank pixel in the output, 1 no source pixel lost')
    p.add_argument('--min_scale', type=float, default=0.2)
    p.add_argument('--max_scale', type=float, default=2.0)
    p.add_argument('--triangulate', action='store_true', help='points and tracks from the images and the poses (mvsdf_amd/keypoints.py) instead of points3D')
    return p


def main(argv=None):
    p = parser()
    a = p.parse_args(argv)
    if not os.path.isdir(a.model_dir):
        p.exit(1, 'colmap2mvs.py: %s: no such directory\n' % a.model_dir)
    from mvsdf_amd.datasets.colmap import colmap_to_mvs
    extra = {'undistort': True, 'blank_pixels': a.blank_pixels, 'min_scale': a.min_scale, 'max_scale': a.max_scale} if a.undistort else {}
    res = colmap_to_mvs(a.model_dir, a.image_dir, a.out_root, max_d=a.max_d, interval_scale=a.interval_scale, num_pairs=a.num_pairs, theta0=a.theta0,
                        sigma1=a.sigma1, sigma2=a.sigma2, triangulate=a.triangulate, **extra)
    n = [len(q) for q in res['pairs']]
    d = res['cams'][:, 1, 3]
    print('[colmap2mvs] %d views -> %s; %d to %d sources per view; depth %.6g to %.6g' % (len(n), a.out_root, min(n), max(n), d[:, 0].min(), d[:, 3].max()))
    return res


if __name__ == '__main__':
    main()
