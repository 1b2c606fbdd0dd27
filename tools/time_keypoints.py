"""Time of mvsdf_amd/keypoints.py at a user's sizes.  The detector: --views (default 8) images of --hw (default 1200,1600), a band-limited random
texture in uint8 RGB.  The matcher: --keypoints (default 8192) random 128-d int8 descriptors per view, one pair and all 28 pairs of 8 views in one
call.  Device events around each call after a warm-up call, medians of --repeats (default 5), in ms:

* scale_space, detect_extrema, detect: the detector's steps, each from the images on (detect contains the other two; its calls wait for the host
  once per octave), with the keypoints found and kept (max_keypoints 8192 per view);
* match_1, match_28: match_descriptors (pack, walk in both directions, merge, compaction and the call's own host wait), mutual, ratio 0.8;
* walk_rate: the int8 operations the matrix cores execute in match_28, 2 directions * 28 pairs * 2 * n * n * 128, over its median time, and the
  share of the int8 MFMA peak, taken as twice the dense BF16 peak MI355X_MICROARCH.md lists (2 * 2.5e15 / s).  A whole-call rate;
* cdist_topk: the yardstick for one direction of one pair, torch.cdist of the same codes in fp32 + topk(2, largest=False); its nearest indices
  are asserted equal to the matcher's (ratio 1, not mutual: every source whose two smallest distances differ is listed).

Prints one JSON line.

    python tools/time_keypoints.py [--keypoints 8192] [--views 8] [--hw 1200,1600] [--repeats 5] [--no_detect]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

INT8_PEAK = 2 * 2.5e15


def _timed(f, repeats):
    f()                                                           # warm-up
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = f()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--keypoints', type=int, default=8192)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--views', type=int, default=8)
    ap.add_argument('--hw', type=str, default='1200,1600')
    ap.add_argument('--no_detect', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'time_keypoints.py measures on the GPU'
    from mvsdf_amd import keypoints as KP
    n, V = a.keypoints, 8
    rs = np.random.RandomState(0)
    base = rs.randint(0, 128, size=(n, 128))
    codes = np.concatenate([np.clip(base[rs.permutation(n)] + rs.randint(-20, 21, size=(n, 128)), 0, 127) for _ in range(V)]).astype(np.int8)
    vo = np.arange(V + 1, dtype=np.int64) * n
    kp = KP.make_keypoints(torch.zeros(V * n, 2, dtype=torch.float64).cuda(), torch.from_numpy(codes).cuda(), vo)
    one = np.array([[0, 1]], np.int32)
    out = {'keypoints': n, 'repeats': a.repeats, 'splits_1': KP.match_splits(vo, one)}
    t1, m1 = _timed(lambda: KP.match_descriptors(kp, pairs=one), a.repeats)
    t28, m28 = _timed(lambda: KP.match_descriptors(kp), a.repeats)
    sf, df = kp.codes[:n].float(), kp.codes[n:2 * n].float()
    tc, top = _timed(lambda: torch.cdist(sf, df).topk(2, dim=1, largest=False), a.repeats)
    plain = KP.match_descriptors(kp, pairs=one, ratio=1.0, mutual=False)
    src, dst = plain.idx[:, 0].long(), plain.idx[:, 1].long()
    assert torch.equal(top.indices[src, 0], dst), 'torch.cdist + topk disagrees with the matcher'
    ops = 2.0 * 28 * 2.0 * n * n * 128
    out.update({'ms': {'match_1': round(t1, 4), 'match_28': round(t28, 4), 'cdist_topk': round(tc, 4)}, 'matches_1': int(m1.idx.shape[0]),
                'matches_28': int(m28.idx.shape[0]), 'compared_with_cdist': int(src.shape[0]),
                'walk_rate': {'int8_ops_per_s': ops / (t28 * 1e-3), 'share_of_int8_peak': ops / (t28 * 1e-3) / INT8_PEAK}})
    if not a.no_detect:
        h, w = (int(x) for x in a.hw.split(','))
        rs = np.random.RandomState(1)
        ys, xs = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing='ij')
        imgs = []
        for v in range(a.views):                                  # a sum of sinusoids with wavelengths of 6 to 60 pixels per channel
            ch = []
            for _ in range(3):
                acc = np.zeros((h, w), np.float32)
                for _ in range(24):
                    lam, th, ph = rs.uniform(6, 60), rs.uniform(0, np.pi), rs.uniform(0, 2 * np.pi)
                    acc += np.sin((xs * np.cos(th) + ys * np.sin(th)) * np.float32(2 * np.pi / lam) + np.float32(ph))
                ch.append(acc)
            imgs.append(np.clip(128 + 18 * np.stack(ch, -1), 0, 255).astype(np.uint8))
        images = torch.from_numpy(np.stack(imgs)).cuda()
        ts, _ = _timed(lambda: KP.scale_space(images), a.repeats)
        te, ex = _timed(lambda: KP.detect_extrema(images), a.repeats)
        td, det = _timed(lambda: KP.detect(images), a.repeats)
        out['detect'] = {'views': a.views, 'hw': [h, w], 'extrema': int(ex.view_off[-1]), 'keypoints': int(det.view_off[-1]),
                         'ms': {'scale_space': round(ts, 3), 'detect_extrema': round(te, 3), 'detect': round(td, 3)}}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
