"""A float64 restatement of the Vis-MVSNet feature CNN (FeatExt, reference code/utils/my_utils.py:499-708) over a state dict, with
torch.nn.functional, plus the seeded checkpoint the FeatExt tests and tests/golden/featext/make_featext_golden.py share.

featext64(sd, x) follows the network as mvsdf_amd/features.py's docstring states it; it never builds modules."""
import hashlib

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
ENC = [('2d2_0', 16, 32, 1), ('2d4_1', 32, 64, 2), ('2d8_2', 64, 128, 2)]
DEC = [('2d16_3', 128, 64), ('2d8_4', 64, 32)]


def _bn(sd, p, y):
    g, b, m, v = (sd[p + s].to(y) for s in ('.weight', '.bias', '.running_mean', '.running_var'))
    sh = (1, -1, 1, 1)
    return (y - m.view(sh)) / torch.sqrt(v.view(sh) + EPS) * g.view(sh) + b.view(sh)


def _conv(sd, p, y, stride=1):
    w = sd[p + '.weight'].to(y)
    return F.conv2d(y, w, stride=stride, padding=w.shape[-1] // 2)


def _block(sd, p, y, stride):
    h = torch.relu(_bn(sd, p + '.bn1', _conv(sd, p + '.conv1', y, stride)))
    h = _bn(sd, p + '.bn2', _conv(sd, p + '.conv2', h))
    r = _bn(sd, p + '.downsample.1', _conv(sd, p + '.downsample.0', y, stride)) if p + '.downsample.0.weight' in sd else y
    return torch.relu(h + r)


def featext64(sd, x, dtype=torch.float64):
    """sd: FeatExt state dict (the module's names), x [N,3,H,W] -> the three outputs in float64 on x's device; dtype=torch.float32: PyTorch's own
    fp32 CPU forward of the same network (the error yardstick of the GPU tests)."""
    y = torch.relu(_bn(sd, 'init_conv.1', _conv(sd, 'init_conv.0', x.to(dtype), 2)))
    skips = []
    for name, _, _, stride in ENC:
        y = _block(sd, 'unet.enc_blocks.%s.0' % name, y, stride)
        y = _block(sd, 'unet.enc_blocks.%s.1' % name, y, 1)
        skips.append(y)
    outs = [y]
    for i, (name, _, _) in enumerate(DEC):
        p = 'unet.dec_blocks.%s' % name
        y = F.conv_transpose2d(y, sd[p + '.0.weight'].to(y), stride=2, padding=1, output_padding=1)
        y = _conv(sd, p + '.1', torch.cat([y, skips[-2 - i]], 1))
        y = _block(sd, p + '.2.0', y, 1)
        outs.append(y)
    return tuple(_conv(sd, 'final_conv_%d' % (i + 1), o) for i, o in enumerate(outs))


def _shapes():
    """-> [(name, shape)] of every FeatExt parameter / buffer, in the module's order."""
    out = []

    def conv(p, cout, cin, k):
        out.append((p + '.weight', (cout, cin, k, k)))

    def bn(p, c):
        out.extend([(p + '.weight', (c,)), (p + '.bias', (c,)), (p + '.running_mean', (c,)), (p + '.running_var', (c,)), (p + '.num_batches_tracked', ())])
    conv('init_conv.0', 16, 3, 5)
    bn('init_conv.1', 16)
    for name, cin, cout, stride in ENC:
        for b in range(2):
            p = 'unet.enc_blocks.%s.%d' % (name, b)
            ci = cin if b == 0 else cout
            conv(p + '.conv1', cout, ci, 3)
            bn(p + '.bn1', cout)
            conv(p + '.conv2', cout, cout, 3)
            bn(p + '.bn2', cout)
            if b == 0:
                conv(p + '.downsample.0', cout, cin, 1)
                bn(p + '.downsample.1', cout)
    for name, cin, c in DEC:
        p = 'unet.dec_blocks.%s' % name
        out.append((p + '.0.weight', (cin, c, 3, 3)))
        conv(p + '.1', c, 2 * c, 3)
        conv(p + '.2.0.conv1', c, c, 3)
        bn(p + '.2.0.bn1', c)
        conv(p + '.2.0.conv2', c, c, 3)
        bn(p + '.2.0.bn2', c)
    for i, cin in enumerate((128, 64, 32)):
        conv('final_conv_%d' % (i + 1), 32, cin, 3)
    return out


def make_state_dict(seed=0):
    """Seeded FeatExt weights: He-scaled convolutions (fan-in cin k^2; the transposed ones cin k^2 / 4, the taps one output pixel sees) and
    non-trivial BatchNorm statistics -> {name: fp32 / int64 tensor}."""
    rs = np.random.RandomState(seed)
    sd = {}
    for name, shape in _shapes():
        if name.endswith('num_batches_tracked'):
            sd[name] = torch.tensor(int(rs.randint(1, 100000)), dtype=torch.int64)
            continue
        if len(shape) == 4:
            fan = shape[1] * shape[2] * shape[3] if '.dec_blocks.' not in name or not name.endswith('.0.weight') else shape[0] * 9 / 4
            v = rs.standard_normal(shape) * np.sqrt(2.0 / fan)
        elif name.endswith('running_var'):
            v = rs.uniform(0.5, 2.0, shape)
        elif name.endswith('running_mean'):
            v = rs.standard_normal(shape) * 0.2
        elif name.endswith('.weight'):
            v = rs.uniform(0.6, 1.4, shape)
        else:
            v = rs.standard_normal(shape) * 0.1
        sd[name] = torch.from_numpy(v.astype(np.float32))
    return sd


def make_checkpoint(seed=0):
    """A Vis-MVSNet checkpoint dict: the FeatExt entries under 'module.feat_ext.' among unrelated keys (my_utils.py:702-703 keeps only those)."""
    sd = make_state_dict(seed)
    rs = np.random.RandomState(seed + 1)
    full = {'module.feat_ext.' + k: v for k, v in sd.items()}
    full['module.stage1.reg.conv0.weight'] = torch.from_numpy(rs.standard_normal((8, 8, 3, 3, 3)).astype(np.float32))
    full['module.uncert_net.head.bias'] = torch.zeros(1)
    return {'state_dict': full, 'epoch': 7}


def state_sha256(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode() + b'\0' + sd[k].numpy().tobytes())
    return h.hexdigest()
