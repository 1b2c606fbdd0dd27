"""Vis-MVSNet output -> the imfunc4/ scene directory (mvsdf_amd/datasets/prepare.py): the reference's code/datasets/vismvsnet2mvsdf.py with its
flags, without OpenCV / open3d.

    python tools/vismvsnet2mvsdf.py --data_root DIR [--range_source pcd|range|fused|clean] [--pthresh .7,.7,0] [--prob_mask] [--resize 1920,1080]
                                    [--crop 1920,1072] --ext_image_path 'IMAGES/{:08}.jpg' [--ext_image_from_one] [--fused_depth]
                                    [--nb_neighbors 20] [--knn_ratio 3] [--eps_ratio 3] [--cluster_frac 1]

Beyond the reference: --range_source fused (fuse the depth maps now, write all_torch.ply, box of the whole cloud), --range_source clean (the
same, then the automatic cut of mvsdf_amd/cloud.py: cut.ply is written and its box is taken; the four cleaning flags belong to it) and
--fused_depth (write the fused depth maps instead of the masked ones).  --show_range needs a viewer and is refused.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


CLEAN_FLAGS = ('nb_neighbors', 'knn_ratio', 'eps_ratio', 'cluster_frac')


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--data_root', type=str, default='eg/path/to/vismvsnet/output')
    ap.add_argument('--range_source', type=str, choices=['range', 'pcd', 'fused', 'clean'], default='pcd')
    ap.add_argument('--pthresh', type=str, default='.7,.7,0')
    ap.add_argument('--prob_mask', action='store_true', default=False)
    ap.add_argument('--resize', type=str, default='1920,1080')
    ap.add_argument('--crop', type=str, default='1920,1072')
    ap.add_argument('--ext_image_path', type=str, default='eg/path/to/image/{:08}.jpg')
    ap.add_argument('--ext_image_from_one', action='store_true', default=False)
    ap.add_argument('--show_range', action='store_true', default=False)
    ap.add_argument('--fused_depth', action='store_true', default=False)
    ap.add_argument('--nb_neighbors', type=int, default=None)
    ap.add_argument('--knn_ratio', type=float, default=None)
    ap.add_argument('--eps_ratio', type=float, default=None)
    ap.add_argument('--cluster_frac', type=float, default=None)
    a = ap.parse_args(argv)
    if a.show_range:
        ap.error('--show_range opens a viewer, which is not built')
    a.clean = {k: getattr(a, k) for k in CLEAN_FLAGS if getattr(a, k) is not None}
    if a.clean and a.range_source != 'clean':
        ap.error('--%s belongs to --range_source clean' % sorted(a.clean)[0])
    return a


def main(argv=None):
    a = parse_args(argv)
    from mvsdf_amd.datasets import prepare
    out = prepare.convert_scene(a.data_root, range_source=a.range_source, pthresh=a.pthresh, prob_mask=a.prob_mask, resize=a.resize, crop=a.crop,
                                ext_image_path=a.ext_image_path, ext_image_from_one=a.ext_image_from_one, fused_depth=a.fused_depth,
                                clean=a.clean if a.range_source == 'clean' else None)
    print('wrote %s' % out)


if __name__ == '__main__':
    main()
