#!/usr/bin/env python3
"""A COLMAP sparse model with distorted cameras and its images as pinhole views, resampled on the GPU:

    python tools/undistort.py MODEL_DIR IMAGE_DIR OUT [--blank_pixels 0] [--min_scale 0.2] [--max_scale 2] [--view_chunk N]

MODEL_DIR holds cameras / images / points3D as .txt or .bin (SIMPLE_RADIAL, RADIAL, OPENCV, FULL_OPENCV, OPENCV_FISHEYE, SIMPLE_RADIAL_FISHEYE,
RADIAL_FISHEYE or pinhole cameras), IMAGE_DIR the images the model names.  Writes OUT/images/<name> and OUT/sparse/{cameras,images,points3D}.txt
with PINHOLE cameras, which tools/colmap2mvs.py takes as they are.  blank_pixels = 0 keeps the largest view without a blank pixel, 1 the smallest
that loses no source pixel.  mvsdf_amd/undistort.py states what is computed."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('model_dir', type=str)
    p.add_argument('image_dir', type=str)
    p.add_argument('out_dir', type=str)
    p.add_argument('--blank_pixels', type=float, default=0.0, help='0: no blank pixel in the output; 1: no source pixel lost')
    p.add_argument('--min_scale', type=float, default=0.2)
    p.add_argument('--max_scale', type=float, default=2.0)
    p.add_argument('--view_chunk', type=int, default=None, help='images of one camera on the device at a time (default: what 1 GiB holds)')
    return p


def main(argv=None):
    p = parser()
    a = p.parse_args(argv)
    if not os.path.isdir(a.model_dir):
        p.exit(1, 'undistort.py: %s: no such directory\n' % a.model_dir)
    from mvsdf_amd.datasets.colmap import load_colmap_model
    from mvsdf_amd.undistort import undistort_model
    model = load_colmap_model(a.model_dir, allow_distortion=True)
    out = undistort_model(model, a.image_dir, a.out_dir, blank_pixels=a.blank_pixels, min_scale=a.min_scale, max_scale=a.max_scale, view_chunk=a.view_chunk)
    for cid in sorted(out['cameras']):
        c, s = out['cameras'][cid], model['cameras'][cid]
        print('[undistort] camera %d: %s %d x %d -> PINHOLE %d x %d' % (cid, s['model'], s['width'], s['height'], c['width'], c['height']))
    print('[undistort] %d images -> %s' % (len(out['images']), a.out_dir))
    return out


if __name__ == '__main__':
    main()
