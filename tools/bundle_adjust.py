#!/usr/bin/env python3
"""Bundle adjustment of a COLMAP model on the GPU (mvsdf_amd/bundle.py: Levenberg-Marquardt over poses and points, intrinsics fixed):

    python tools/bundle_adjust.py MODEL_DIR OUT_MODEL_DIR [--fixed I,J] [--loss_scale D] [--iterations N]

MODEL_DIR holds cameras / images / points3D as .txt or .bin (pinhole cameras; the points need their tracks, the images their observations: what
tools/sparse_points.py writes).  OUT_MODEL_DIR receives the same model as text with refined poses and points and each point's mean reprojection
error.  --fixed: the views that stay, counted over the images by ascending id (default 0; give two to pin the scale as well).  --loss_scale: the
Huber width in pixels (default: plain least squares).  Prints the cost and the RMS residual before and after."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('model_dir')
    p.add_argument('out_model_dir')
    p.add_argument('--fixed', type=str, default='0', help='comma-separated view indices that stay')
    p.add_argument('--loss_scale', type=float, default=None, help='Huber width in pixels')
    p.add_argument('--iterations', type=int, default=10)
    return p


def main(argv=None):
    a = parser().parse_args(argv)
    from mvsdf_amd import bundle
    from mvsdf_amd.datasets.colmap import load_colmap_model, write_colmap_text
    try:
        fixed = tuple(int(w) for w in a.fixed.split(',') if w.strip() != '')
    except ValueError:
        raise ValueError('bundle_adjust.py: --fixed takes comma-separated integers, got %r' % a.fixed) from None
    rep = {}
    model = bundle.refine_model(load_colmap_model(a.model_dir), report=rep, fixed_views=fixed, loss_scale=a.loss_scale, iterations=a.iterations)
    print('[bundle_adjust] %(observations)d observations: cost %(cost0).6g -> %(cost).6g, rms %(rms0).4f -> %(rms).4f px, %(iterations)d iterations, '
          '%(accepted)d accepted, %(cg_iterations)d cg iterations' % rep)
    write_colmap_text(model, a.out_model_dir)
    return {'model': model, 'report': rep}


if __name__ == '__main__':
    main()
