#!/usr/bin/env python3
"""Generate the FeatExt / scene-IO golden vectors under tests/golden/featext/ by running the PyTorch reference (jzhangbs/MVSDF @ /root/reference)
on CPU.  Runs ONLY in the build container (the reference never travels to the GPU box).

* featext_*.npz: the reference's FeatExt (utils/my_utils.py) loaded from a checkpoint in Vis-MVSNet's layout ('module.feat_ext.*' among
  unrelated keys) whose weights come from tests/featext_ref.py::make_checkpoint(SEED) -- regenerated, never committed; the SHA-256 of the
  state dict is recorded -- on seeded inputs, fp32, eval mode: x and the three outputs.
* io.npz: the reference's load_pfm / load_cam / load_pair / scale_camera on small files written here (their bytes are stored too).

    python tests/golden/featext/make_featext_golden.py
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..'))
import featext_ref  # noqa: E402

sys.path.insert(0, '/root/reference/code')
from utils import my_utils  # noqa: E402

SEED = 3
CASES = {'featext_1x72x104': (1, 72, 104, 11), 'featext_3x40x56': (3, 40, 56, 12)}


def reference_featext(ckpt):
    real_load = torch.load
    torch.load = lambda *a, **k: ckpt            # FeatExt.__init__ loads 'utils/vismvsnet.pt'
    try:
        m = my_utils.FeatExt()
    finally:
        torch.load = real_load
    return m.eval()


def main():
    torch.set_num_threads(1)
    ckpt = featext_ref.make_checkpoint(SEED)
    sd = featext_ref.make_state_dict(SEED)
    net = reference_featext(ckpt)
    for name, (n, h, w, xseed) in CASES.items():
        x = np.random.RandomState(xseed).standard_normal((n, 3, h, w)).astype(np.float32)
        with torch.no_grad():
            o1, o2, o3 = net(torch.from_numpy(x))
        np.savez_compressed(os.path.join(HERE, name + '.npz'), x=x, out1=o1.numpy(), out2=o2.numpy(), out3=o3.numpy(), seed=SEED,
                            sha256=featext_ref.state_sha256(sd))
    # IO helpers
    rs = np.random.RandomState(5)
    d = tempfile.mkdtemp()
    depth = rs.uniform(400, 900, (6, 10)).astype(np.float32)
    colour = rs.standard_normal((4, 5, 3)).astype(np.float32)
    my_utils.write_pfm(os.path.join(d, 'd.pfm'), depth)
    my_utils.write_pfm(os.path.join(d, 'c.pfm'), colour, scale=2)
    cams = {}
    ext = np.eye(4)
    ext[:3, :3] = np.linalg.qr(rs.standard_normal((3, 3)))[0]
    ext[:3, 3] = rs.standard_normal(3) * 100
    K = np.array([[361.54, 0, 82.9], [0, 360.39, 66.38], [0, 0, 1]])
    for nw, tail in ((29, '425.0 2.5'), (30, '425.0 2.5 192'), (31, '425.0 2.5 192 937.0')):
        txt = 'extrinsic\n' + '\n'.join(' '.join('%.9g' % v for v in r) for r in ext) + '\n\nintrinsic\n' + \
              '\n'.join(' '.join('%.9g' % v for v in r) for r in K) + '\n\n' + tail + '\n'
        p = os.path.join(d, 'cam%d.txt' % nw)
        open(p, 'w').write(txt)
        cams['cam%d_txt' % nw] = np.frombuffer(txt.encode(), np.uint8)
        cams['cam%d' % nw] = my_utils.load_cam(p, 256, 1)
        cams['cam%d_s' % nw] = my_utils.load_cam(p, 128, 0.5)
        cams['cam%d_o' % nw] = my_utils.load_cam(p, 128, 1, override=True) if nw == 31 else my_utils.load_cam(p, 128, 1)
    cams['cam29_scaled'] = my_utils.scale_camera(cams['cam29'], 2)
    cams['cam29_scaled_xy'] = my_utils.scale_camera(cams['cam29'], (0.5, 0.25))
    cams['cam29_scaled_t'] = my_utils.scale_camera(torch.from_numpy(np.stack([cams['cam29'], cams['cam30']])), 2).numpy()
    pair = '4\n0\n3 2 310.5 1 120.25 3 50.0\n1\n2 0 200.0 2 10.5\n2\n1 0 99.0\n3\n3 0 1.0 1 2.0 2 3.0\n'
    open(os.path.join(d, 'pair.txt'), 'w').write(pair)
    pr = my_utils.load_pair(os.path.join(d, 'pair.txt'))
    pr2 = my_utils.load_pair(os.path.join(d, 'pair.txt'), min_views=2)
    np.savez_compressed(os.path.join(HERE, 'io.npz'), depth_pfm=np.frombuffer(open(os.path.join(d, 'd.pfm'), 'rb').read(), np.uint8),
                        colour_pfm=np.frombuffer(open(os.path.join(d, 'c.pfm'), 'rb').read(), np.uint8),
                        depth=np.ascontiguousarray(my_utils.load_pfm(os.path.join(d, 'd.pfm'))),
                        colour=np.ascontiguousarray(my_utils.load_pfm(os.path.join(d, 'c.pfm'))),
                        depth_src=depth, colour_src=colour,
                        pair_txt=np.frombuffer(pair.encode(), np.uint8), pair=np.array(repr(pr)), pair_min2=np.array(repr(pr2)), **cams)


if __name__ == '__main__':
    main()
