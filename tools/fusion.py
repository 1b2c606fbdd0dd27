"""Point-cloud fusion of Vis-MVSNet depth maps on the device (mvsdf_amd/fusion.py, which states the algorithm): the command line of the reference's
BYOD.md.

    python tools/fusion.py --data DIR --pair DIR/pair.txt --view 10 --vthresh 2 --pthresh .8,.7,.8 --no_normal --downsample -1
                           [--cam_scale 1] [--pix_thresh 1] [--dep_thresh 0.01]
    python tools/fusion.py --data DIR --normals [--normal_jump 0.05] ...

Reads cam_<id:08>_flow3.txt, <id:08>_flow3.pfm, <id:08>_flow{1,2,3}_prob.pfm and, where every view has one, <id:08>.jpg|png (resized to the
depth-map size with prepare.resize_bilinear_u8) from DIR; writes DIR/all_torch.ply; prints the points per view and the total.  One of --no_normal
(BYOD.md's) and --normals must be given: --normals adds nx ny nz from the fused depth maps (fusion.depth_normals), the input of
tools/poisson_mesh.py, and prints how many points got none.  Not built, and refused: voxel down-sampling (--downsample other than -1), --cam_scale
other than 1.
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
    ap.add_argument('--view', type=int, default=10)
    ap.add_argument('--vthresh', type=int, default=2)
    ap.add_argument('--pthresh', type=str, default='.8,.7,.8')
    ap.add_argument('--cam_scale', type=float, default=1.0)
    ap.add_argument('--no_normal', action='store_true', default=False)
    ap.add_argument('--normals', action='store_true', default=False, help='write nx ny nz (fusion.depth_normals)')
    ap.add_argument('--normal_jump', type=float, default=0.05, help='no tangent across a relative depth step above this (inf: off)')
    ap.add_argument('--downsample', type=float, default=-1)
    ap.add_argument('--pix_thresh', type=float, default=1.0)
    ap.add_argument('--dep_thresh', type=float, default=0.01)
    a = ap.parse_args(argv)
    if a.cam_scale != 1:
        ap.error('--cam_scale %g: rescaling the cameras is not built (only 1)' % a.cam_scale)
    if a.downsample != -1:
        ap.error('--downsample %g: voxel down-sampling is not built (only -1)' % a.downsample)
    if a.no_normal == a.normals:
        ap.error('pass either --no_normal, as BYOD.md does, or --normals (normals from the fused depth maps)')
    if not a.normal_jump >= 0:
        ap.error('--normal_jump must be >= 0')
    a.pthresh = [float(v) for v in a.pthresh.split(',')]
    if len(a.pthresh) != 3:
        ap.error('--pthresh takes three comma-separated thresholds')
    return a


def find_images(data, ids):
    """the <id:08>.jpg|png of every view, or None when one view has neither"""
    paths = []
    for i in ids:
        found = [p for p in (os.path.join(data, '%s.%s' % (i.zfill(8), e)) for e in ('jpg', 'png')) if os.path.exists(p)]
        if not found:
            return None
        paths.append(found[0])
    return paths


def main(argv=None):
    a = parse_args(argv)
    import numpy as np
    from mvsdf_amd import fusion
    from mvsdf_amd.datasets import prepare
    pair, cams, depths, probs = prepare.load_mvs_output(a.data, pair_file=a.pair)
    h, w = depths.shape[1:]
    paths = find_images(a.data, pair['id_list'])
    images = None if paths is None else np.stack([prepare.resize_bilinear_u8(prepare.load_image_u8(p), w, h) for p in paths])
    fused = fusion.fuse_depths(cams, depths, prepare.pair_indices(pair), probs=probs, images=images, pthresh=a.pthresh, view=a.view,
                               vthresh=a.vthresh, pix_thresh=a.pix_thresh, dep_thresh=a.dep_thresh, normals=a.normals, normal_jump=a.normal_jump)
    per_view = np.bincount(fused.view.cpu().numpy(), minlength=len(depths))
    for vid, n in zip(pair['id_list'], per_view):
        print('view %s: %d points' % (vid, n))
    out = os.path.join(a.data, 'all_torch.ply')
    fusion.save_points(out, fused.points, fused.colors, normals=fused.normals)
    if fused.normals is not None:
        print('normals: %d of %d points have none' % (int((fused.normals == 0).all(1).sum()), len(fused)))
    print('total: %d points -> %s' % (len(fused), out))


if __name__ == '__main__':
    main()
