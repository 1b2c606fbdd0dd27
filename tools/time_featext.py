"""Time FeatExt (mvsdf_amd/features.py, csrc/featext.hip) per stage on the device, against the same network through PyTorch's convolutions in fp32
on the same GPU (F.conv2d / F.conv_transpose2d, i.e. MIOpen) with the same seeded weights, as the comparison line.

The comparison line does the work our kernels do and no more: eval BatchNorm folded into the weights and a bias (in fp64, as the pack does),
F.conv2d with that bias, the residual added and ReLU applied in place; the decoder concatenation is a torch.cat (PyTorch has no two-source
convolution).  torch.backends.cudnn.benchmark = True, so MIOpen searches its kernels during the warm-up.  It runs in NCHW and in channels-last;
both are reported.

Each stage is timed alone with device events (both sides keep their activations between stages), median of --steps after --warmup; 'total' is
one full forward.  FLOPs are counted from the architecture (2 per multiply-add, the transposed convolutions over their real taps); the fraction
is of the 157.3 TF fp32 matrix peak.  Prints one JSON line.

    python tools/time_featext.py [--hw 1200,1600] [--batch 7] [--steps 10] [--warmup 3] [--views 49]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch  # noqa: E402

PEAK_TF = 157.3


def flops(h, w):
    """multiply-adds x 2 per image, per stage"""
    R, S = (h + 1) // 2, (w + 1) // 2
    rs = R * S
    conv = lambda cin, cout, k, px: 2.0 * cin * cout * k * k * px
    enc = lambda cin, c, px: conv(cin, c, 3, px) + conv(c, c, 3, px) + conv(cin, c, 1, px) + 2 * conv(c, c, 3, px)
    dec = lambda cin, c, px: conv(cin, c, 3, px / 4) + conv(2 * c, c, 3, px) + 2 * conv(c, c, 3, px)   # deconv: 9 taps per input pixel
    return [conv(3, 16, 5, rs), enc(16, 32, rs), enc(32, 64, rs / 4), enc(64, 128, rs / 16), dec(128, 64, rs / 4), dec(64, 32, rs),
            conv(128, 32, 3, rs / 16) + conv(64, 32, 3, rs / 4) + conv(32, 32, 3, rs)]


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def fold(sd, device):
    """-> {conv module path: (fp32 weight, fp32 bias or None)} with eval BatchNorm folded in fp64 (features.LAYERS order)"""
    from mvsdf_amd import features
    out = {}
    for conv, bn in features.LAYERS:
        w = sd[conv + '.weight'].double()
        b = None
        if bn:
            g, beta, m, v = (sd[bn + s].double() for s in ('.weight', '.bias', '.running_mean', '.running_var'))
            sc = g / torch.sqrt(v + 1e-5)
            w = w * sc.view(-1, 1, 1, 1)
            b = (beta - m * sc).float().to(device)
        out[conv] = (w.float().to(device), b)
    return out


class TorchFeatExt:
    """FeatExt through PyTorch's fp32 convolutions with the folded weights, stage by stage (features.STAGES); acts[] keeps the activations."""
    ENC = [('2d2_0', 1), ('2d4_1', 2), ('2d8_2', 2)]
    DEC = ['2d16_3', '2d8_4']

    def __init__(self, fw, channels_last):
        import torch.nn.functional as F
        self.F, self.fw, self.acts = F, fw, {}
        if channels_last:
            self.fw = {k: (w.contiguous(memory_format=torch.channels_last), b) for k, (w, b) in fw.items()}

    def conv(self, name, x, stride=1, relu=False, res=None):
        w, b = self.fw[name]
        y = self.F.conv2d(x, w, b, stride, w.shape[-1] // 2)
        if res is not None:
            y.add_(res)
        return y.relu_() if relu else y

    def block(self, p, x, stride):
        t = self.conv(p + '.conv1', x, stride, True)
        r = self.conv(p + '.downsample.0', x, stride) if p + '.downsample.0' in self.fw else x
        return self.conv(p + '.conv2', t, 1, True, r)

    def stage(self, i):
        a = self.acts
        if i == 0:
            a['x0'] = self.conv('init_conv.0', a['x'], 2, True)
        elif i <= 3:
            name, stride = self.ENC[i - 1]
            y = self.block('unet.enc_blocks.%s.0' % name, a['x0'] if i == 1 else a['e%d' % (i - 2)], stride)
            a['e%d' % (i - 1)] = self.block('unet.enc_blocks.%s.1' % name, y, 1)
        elif i <= 5:
            p = 'unet.dec_blocks.%s' % self.DEC[i - 4]
            x, skip = (a['e2'], a['e1']) if i == 4 else (a['o2'], a['e0'])
            d = self.F.conv_transpose2d(x, self.fw[p + '.0'][0], stride=2, padding=1, output_padding=1)
            y = self.conv(p + '.1', torch.cat([d, skip], 1))
            a['o2' if i == 4 else 'o3'] = self.block(p + '.2.0', y, 1)
        else:
            a['out'] = (self.conv('final_conv_1', a['e2']), self.conv('final_conv_2', a['o2']), self.conv('final_conv_3', a['o3']))

    def __call__(self, x):
        self.acts['x'] = x
        for i in range(7):
            self.stage(i)
        return self.acts['out']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hw', default='1200,1600')
    ap.add_argument('--batch', type=int, default=7)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--views', type=int, default=49)
    a = ap.parse_args()
    h, w = (int(v) for v in a.hw.split(','))
    import featext_ref
    from mvsdf_amd import features
    sd = featext_ref.make_state_dict(0)
    net = features.FeatExt()
    net.load_state_dict(sd)
    net = net.cuda().eval()
    x = torch.randn((a.batch, 3, h, w), generator=torch.Generator().manual_seed(0)).cuda()
    xh = x.permute(0, 2, 3, 1).contiguous()
    R, S = features.output_hw(h, w)
    outs = [torch.empty((a.batch, r, s, 32), device='cuda') for r, s in ((R // 4, S // 4), (R // 2, S // 2), (R, S))]
    net.run(xh, *outs)
    torch.cuda.synchronize()
    stages = {}
    for i, name in enumerate(features.STAGES):
        stages[name] = _time(lambda: net.run(xh, *outs, stages=(i, i + 1)), a.steps, a.warmup)
    total = _time(lambda: net(x), a.steps, a.warmup)
    torch.backends.cudnn.benchmark = True
    base = {}
    with torch.no_grad():
        for layout in ('nchw', 'channels_last'):
            tf = TorchFeatExt(fold(sd, 'cuda'), layout == 'channels_last')
            xb = x.contiguous(memory_format=torch.channels_last) if layout == 'channels_last' else x
            ref = tf(xb)
            for o, r in zip(ref, outs):                                                   # same network: agree to fp32 rounding
                d = float((o - r.permute(0, 3, 1, 2)).abs().max()) / float(o.abs().max())
                assert d < 1e-4, ('the comparison line computes something else', layout, d)
            st = {}
            for i, name in enumerate(features.STAGES):
                st[name] = round(_time(lambda: tf.stage(i), a.steps, a.warmup), 4)
            base[layout] = {'total_ms': round(_time(lambda: tf(xb), a.steps, a.warmup), 4), 'stage_ms': st}
            del tf, ref
    miopen = min(b['total_ms'] for b in base.values())
    fl = flops(h, w)
    tot_fl = sum(fl) * a.batch
    res = {
        'hw': [h, w], 'batch': a.batch,
        'stage_ms': {k: round(v, 4) for k, v in stages.items()},
        'stage_tflops': {k: round(f * a.batch / (stages[k] * 1e-3) / 1e12, 2) for k, f in zip(features.STAGES, fl)},
        'total_ms': round(total, 4), 'miopen_fp32_ms': round(miopen, 4), 'miopen_fp32': base,
        'gflop_per_image': round(sum(fl) / 1e9, 2),
        'tflops': round(tot_fl / (total * 1e-3) / 1e12, 2), 'miopen_tflops': round(tot_fl / (miopen * 1e-3) / 1e12, 2),
        'frac_fp32_mfma_peak': round(tot_fl / (total * 1e-3) / 1e12 / PEAK_TF, 4),
        'ms_per_scan_%d_views' % a.views: round(total / a.batch * a.views, 2),
        'miopen_ms_per_scan_%d_views' % a.views: round(miopen / a.batch * a.views, 2),
    }
    print(json.dumps(res))


if __name__ == '__main__':
    main()
