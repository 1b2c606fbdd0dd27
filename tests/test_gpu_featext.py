"""FeatExt on the fp32 matrix cores (csrc/featext.hip): every layer kind alone against float64 F.conv2d / F.conv_transpose2d, the whole network
against the reference's outputs (tests/golden/featext) and the float64 restatement (tests/featext_ref.py), determinism across calls and
batches, the channels-last outputs, and the feature-consistency loss on them.

Error rule: max |ours - fp64| <= 4 x max |PyTorch fp32 CPU - fp64| (same input, measured here) + 1e-6 max |fp64|, and never above 1e-4 max |fp64|."""
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import featext_ref as R
from conftest import GOLDEN
from mvsdf_amd.features import FeatExt, conv_layer, extract_features

pytestmark = pytest.mark.gpu
SEED = 3


def _assert_close(got, ref64, cpu32, what=''):
    got = got.detach().double().cpu()
    scale = float(ref64.abs().max())
    err = float((got - ref64).abs().max())
    e32 = float((cpu32.double() - ref64).abs().max())
    assert got.shape == ref64.shape, what
    assert err <= 4 * e32 + 1e-6 * scale and err <= 1e-4 * scale, (what, err, e32, scale)


@pytest.fixture(scope='module')
def net():
    m = FeatExt()
    m.load_state_dict(R.make_state_dict(SEED))
    return m.cuda().eval()


# (name, transposed, c1, c2, cout, k, stride)
LAYER_CASES = [
    ('init_conv5_s2', False, 3, 0, 16, 5, 2),
    ('conv3_s1', False, 16, 0, 32, 3, 1),
    ('conv3_s2', False, 32, 0, 64, 3, 2),
    ('conv3_128', False, 64, 0, 128, 3, 2),
    ('conv3_head', False, 128, 0, 32, 3, 1),
    ('conv1_s1', False, 16, 0, 32, 1, 1),
    ('conv1_s2', False, 64, 0, 128, 1, 2),
    ('deconv_128_64', True, 128, 0, 64, 3, 2),
    ('deconv_64_32', True, 64, 0, 32, 3, 2),
    ('concat_64_64', False, 64, 64, 64, 3, 1),
    ('concat_32_32', False, 32, 32, 32, 3, 1),
]


@pytest.mark.parametrize('case', LAYER_CASES, ids=[c[0] for c in LAYER_CASES])
@pytest.mark.parametrize('shape', [(1, 13, 21), (3, 9, 17)], ids=['n1_13x21', 'n3_9x17'])
@pytest.mark.parametrize('epi', [(False, False, False), (True, True, True), (True, False, True)], ids=['plain', 'bias_res_relu', 'bias_relu'])
def test_layer_alone(case, shape, epi):
    name, transposed, c1, c2, cout, k, stride = case
    n, h, w = shape
    with_bias, with_res, relu = epi
    g = torch.Generator().manual_seed(zlib.crc32(repr((name, shape, epi)).encode()))
    cin = c1 + c2
    wshape = (cin, cout, k, k) if transposed else (cout, cin, k, k)
    wt = torch.randn(wshape, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    x = torch.randn((n, cin, h, w), generator=g)
    b = torch.randn(cout, generator=g) * 0.1 if with_bias else None

    def ref(dt):
        xx, ww = x.to(dt), wt.to(dt)
        y = F.conv_transpose2d(xx, ww, stride=2, padding=1, output_padding=1) if transposed else F.conv2d(xx, ww, stride=stride, padding=k // 2)
        if b is not None:
            y = y + b.to(dt).view(1, -1, 1, 1)
        return y
    y64 = ref(torch.float64)
    res = torch.randn(y64.shape, generator=g) if with_res else None
    y32 = ref(torch.float32)
    if res is not None:
        y64, y32 = y64 + res.double(), y32 + res
    if relu:
        y64, y32 = torch.relu(y64), torch.relu(y32)
    xc = x.cuda()
    x1, x2 = (xc[:, :c1], xc[:, c1:]) if c2 else (xc, None)
    out = conv_layer(x1, wt.cuda(), b.cuda() if b is not None else None, stride, res.cuda() if res is not None else None, relu, x2=x2,
                     transposed=transposed)
    assert out.stride(1) == 1
    _assert_close(out, y64, y32, name)


@pytest.mark.parametrize('name', ['featext_1x72x104', 'featext_3x40x56'])
def test_featext_vs_reference_fixtures(net, name):
    g = np.load(os.path.join(GOLDEN, 'featext', name + '.npz'))
    x = torch.from_numpy(g['x'])
    outs = net(x.cuda())
    r64 = R.featext64(R.make_state_dict(SEED), x)
    r32 = R.featext64(R.make_state_dict(SEED), x, torch.float32)
    for o, key, a, b in zip(outs, ('out1', 'out2', 'out3'), r64, r32):
        ref = torch.from_numpy(g[key]).double()
        scale = float(ref.abs().max())
        assert float((o.double().cpu() - ref).abs().max()) <= 1e-4 * scale, key          # the reference's own fp32 outputs
        _assert_close(o, a, b, key)
    torch.cuda.synchronize()


def test_featext_larger_image_vs_fp64(net):
    x = torch.randn((3, 3, 600, 800), generator=torch.Generator().manual_seed(21)) * 1.2
    outs = net(x.cuda())
    sd = R.make_state_dict(SEED)
    with torch.no_grad():
        r64 = R.featext64(sd, x)
        r32 = R.featext64(sd, x, torch.float32)
    assert [tuple(o.shape) for o in outs] == [(3, 32, 75, 100), (3, 32, 150, 200), (3, 32, 300, 400)]
    for o, a, b, key in zip(outs, r64, r32, ('out1', 'out2', 'out3')):
        _assert_close(o, a, b, key)


def test_odd_input_size(net):
    x = torch.randn((2, 3, 39, 57), generator=torch.Generator().manual_seed(5))          # R, S = 20, 29 -> not allowed
    with pytest.raises(ValueError):
        net(x.cuda())
    x = torch.randn((2, 3, 47, 63), generator=torch.Generator().manual_seed(5))          # R, S = 24, 32
    outs = net(x.cuda())
    sd = R.make_state_dict(SEED)
    for o, a, b in zip(outs, R.featext64(sd, x), R.featext64(sd, x, torch.float32)):
        _assert_close(o, a, b)


def test_determinism_across_calls_and_batches(net):
    x = torch.randn((3, 3, 64, 88), generator=torch.Generator().manual_seed(8)).cuda()
    a = net(x)
    b = net(x)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    alone = net(x[1:2].contiguous())
    for u, v in zip(a, alone):
        assert torch.equal(u[1:2], v)
    f = extract_features(net, x, batch=2)
    assert torch.equal(f, a[2])


def test_outputs_are_channels_last_and_inputs_in_either_layout(net):
    x = torch.randn((2, 3, 40, 56), generator=torch.Generator().manual_seed(9)).cuda()
    a = net(x)
    b = net(x.contiguous(memory_format=torch.channels_last))
    for u, v in zip(a, b):
        assert u.is_contiguous(memory_format=torch.channels_last) and u.stride(1) == 1
        assert torch.equal(u, v)
    f = extract_features(net, x)
    assert f.is_contiguous(memory_format=torch.channels_last) and f.shape == (2, 32, 20, 28)


def test_weights_repacked_after_change(net):
    m = FeatExt()
    m.load_state_dict(R.make_state_dict(SEED))
    m = m.cuda()
    x = torch.randn((1, 3, 40, 56), generator=torch.Generator().manual_seed(10)).cuda()
    a = m(x)[2].clone()
    with torch.no_grad():
        dict(m.named_modules())['unet.dec_blocks.2d8_4.1'].weight.mul_(1.5)
    b = m(x)[2]
    assert not torch.equal(a, b)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    _assert_close(b, R.featext64(sd, x.cpu())[2], R.featext64(sd, x.cpu(), torch.float32)[2])


def test_grad_input_raises(net):
    x = torch.randn((1, 3, 40, 56), device='cuda', requires_grad=True)
    with pytest.raises(NotImplementedError):
        net(x)


def test_feature_loss_same_in_both_layouts(net):
    """IDRLoss's feature term on FeatExt features: channels-last (as extract_features keeps them) == the same values contiguous NCHW."""
    from mvsdf_amd.model.loss import IDRLoss
    from mvsdf_amd.utils import synth
    g = np.load(os.path.join(GOLDEN, 'feat_corr.npz'))
    B, P, V = int(g['B']), int(g['P']), int(g['V'])
    hw = tuple(int(v) for v in g['feat_hw'])
    _, gt = synth.make_batch(B, P, V, seed=int(g['seed']), size=float(g['scene_size']), center=tuple(g['scene_center']), feat_hw=hw,
                             focal_scale=float(g['focal_scale']))
    imgs = torch.randn((B * (1 + V), 3, 2 * hw[0], 2 * hw[1]), generator=torch.Generator().manual_seed(3)).cuda()
    f = extract_features(net, imgs)                                                   # [B (1 + V), 32, H, W] channels-last
    idx = torch.arange(B, device='cuda')
    src = torch.arange(B, B * (1 + V), device='cuda').view(B, V)
    feat_cl, fsrc_cl = f[idx], torch.stack([f[src[:, v]] for v in range(V)], 1)
    fsrc_cl = fsrc_cl.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    assert feat_cl.stride(1) == 1 and fsrc_cl.stride(2) == 1
    hits = torch.from_numpy(g['hits'].astype(bool)).cuda()
    pts = torch.from_numpy(g['points']).cuda()
    t = lambda k: torch.from_numpy(np.ascontiguousarray(gt[k])).cuda()
    args = (t('cam'), t('src_cams'), t('size')[:1], t('center')[:1])
    loss = IDRLoss()
    a = loss.get_feat_loss_corr(pts, None, feat_cl, args[0], fsrc_cl, args[1], args[2], args[3], hits, hits)
    b = loss.get_feat_loss_corr(pts, None, feat_cl.contiguous(), args[0], fsrc_cl.contiguous(), args[1], args[2], args[3], hits, hits)
    assert torch.isfinite(a) and float(a) != 0.0
    assert torch.equal(a, b), (float(a), float(b))
