"""Depth and confidence maps by plane sweep on the device (mvsdf_amd/stereo.py, which states the algorithm), in place of the "Run VisMVSNet" step of
the reference's BYOD.md; the flags are those of its test.py call.

    python tools/mvs_depth.py --data_root DATA/SCAN --dataset_name general --num_src 2 --max_d 256 --interval_scale 1 --resize 768,576
                              --crop 768,576 --write_result --result_dir OUT [--load_path vismvsnet.ckpt] [--descriptor patch] [--radius 2]
                              [--sgm [P1,P2]] [--sgm_paths 8] [--cascade [D1,D2,D3]] [--cascade_scales 4,2,1]

Reads DATA/SCAN/images/<id:08>.jpg|png, cams/<id:08>_cam.txt and pair.txt; writes OUT/<id:08>_flow3.pfm, <id:08>_flow{1,2,3}_prob.pfm,
cam_<id:08>_flow3.txt, <id:08>.jpg and pair.txt, which tools/fusion.py and tools/vismvsnet2mvsdf.py read.  With --load_path the descriptors are
FeatExt's feature maps from that Vis-MVSNet checkpoint, else mean-free grey patches.  The three maps are confidences of a plane sweep, not
Vis-MVSNet's probabilities: pass --pthresh .7,.02,.9 to the two tools that follow, not BYOD.md's .8,.7,.8.  --model_name is accepted and ignored (there is
one sweep); --dataset_name other than general and a run without --write_result are refused.  --sgm regularises the score volume of every view by
semi-global aggregation before the depth is picked (penalties P1,P2, default .1,.8; --sgm_paths 4 or 8 directions), which helps on noisy photographs.
--cascade sweeps coarse to fine as Vis-MVSNet's model_cas does (stereo.py, "Cascade"): D1 hypotheses over the whole range at a quarter of the depth
maps' size, then D2 and D3 around the previous depth at half and full size (default auto,32,16; auto = max_d over the first scale, 64 at 256);
--cascade_scales: the interval of every stage in units of the finest (default 4,2,1, a factor 2 per stage).  With --sgm the first stage is regularised.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--data_root', type=str, required=True)
    ap.add_argument('--result_dir', type=str, required=True)
    ap.add_argument('--dataset_name', type=str, default='general')
    ap.add_argument('--model_name', type=str, default=None)
    ap.add_argument('--load_path', type=str, default=None, help="a Vis-MVSNet checkpoint: FeatExt's feature maps as descriptors")
    ap.add_argument('--descriptor', type=str, default='patch', choices=['patch'])
    ap.add_argument('--radius', type=int, default=2)
    ap.add_argument('--num_src', type=int, default=2)
    ap.add_argument('--max_d', type=int, default=256)
    ap.add_argument('--interval_scale', type=float, default=1.0)
    ap.add_argument('--resize', type=str, default=None)
    ap.add_argument('--crop', type=str, default=None)
    ap.add_argument('--write_result', action='store_true', default=False)
    ap.add_argument('--sgm', type=str, nargs='?', const='', default=None, metavar='P1,P2',
                    help='semi-global regularisation of the score volume; penalties for a one-step change and a jump (default .1,.8)')
    ap.add_argument('--sgm_paths', type=int, default=8, choices=[4, 8])
    ap.add_argument('--cascade', type=str, nargs='?', const='', default=None, metavar='D1,D2,D3',
                    help='coarse-to-fine sweep; the hypotheses per stage, coarsest first, D1 may be auto (default auto,32,16)')
    ap.add_argument('--cascade_scales', type=str, default=None, metavar='G1,G2,G3', help='the interval scale of every stage (default 4,2,1)')
    a = ap.parse_args(argv)
    a.cascade_arg = None
    if a.cascade is not None:
        try:
            nums = [None if i == 0 and v.strip() == 'auto' else int(v) for i, v in enumerate(a.cascade.split(','))] if a.cascade else [None, 32, 16]
            scales = [float(v) for v in a.cascade_scales.split(',')] if a.cascade_scales else [float(2 ** (len(nums) - 1 - i)) for i in range(len(nums))]
        except ValueError:
            nums, scales = [], []
        if not 1 <= len(nums) <= 4 or len(scales) != len(nums) or any(n is not None and n < 1 for n in nums) or not all(0 < g < float('inf') for g in scales):
            ap.error('--cascade %s --cascade_scales %s: one to four stages, a whole number of hypotheses >= 1 (or auto for the first) and a positive '
                     'scale per stage' % (a.cascade, a.cascade_scales))
        a.cascade_arg = (tuple(nums), tuple(scales))
    elif a.cascade_scales is not None:
        ap.error('--cascade_scales needs --cascade')
    a.regularize = None
    if a.sgm is not None:
        try:
            pen = [float(v) for v in a.sgm.split(',')] if a.sgm else [0.1, 0.8]
        except ValueError:
            pen = []
        if len(pen) != 2 or not 0 <= pen[0] <= pen[1] < float('inf'):
            ap.error('--sgm %s: two penalties P1,P2 with 0 <= P1 <= P2' % a.sgm)
        a.regularize = (pen[0], pen[1], a.sgm_paths)
    if a.dataset_name != 'general':
        ap.error('--dataset_name %s: only general (images/, cams/, pair.txt) is built' % a.dataset_name)
    if not a.write_result:
        ap.error('nothing to do without --write_result, as BYOD.md passes it')
    return a


def main(argv=None):
    a = parse_args(argv)
    from mvsdf_amd import stereo
    sweep = stereo.estimate_scene(a.data_root, a.result_dir, feat_ckpt=a.load_path, descriptor=a.descriptor, num_src=a.num_src, max_d=a.max_d,
                                  interval_scale=a.interval_scale, resize=a.resize, crop=a.crop, radius=a.radius, regularize=a.regularize, cascade=a.cascade_arg)
    t = stereo.PTHRESH
    p = sweep.probs
    kept = (p[:, 0] > t[0]) & (p[:, 1] > t[1]) & (p[:, 2] > t[2]) & (sweep.depths > 0)
    print('%d views of %d x %d -> %s; %.1f %% of the pixels pass --pthresh %s' % (p.shape[0], p.shape[2], p.shape[3], a.result_dir,
                                                                                 100.0 * float(kept.float().mean()), ','.join('%g' % v for v in t)))


if __name__ == '__main__':
    main()
