"""FeatExt and the scene readers without a GPU: the float64 restatement (tests/featext_ref.py) against the reference's outputs, checkpoint key
mapping, the IO helpers against the reference's results on the same files, the projection-matrix decomposition and the shape rule."""
import os

import numpy as np
import pytest
import torch

import featext_ref as R
from conftest import GOLDEN
from mvsdf_amd import features
from mvsdf_amd.features import FeatExt
from mvsdf_amd.utils import io as sio

FX = os.path.join(GOLDEN, 'featext')
SEED = 3


def _fix(name):
    return np.load(os.path.join(FX, name + '.npz'))


def test_seeded_weights_are_the_ones_the_fixtures_used():
    sd = R.make_state_dict(SEED)
    for name in ('featext_1x72x104', 'featext_3x40x56'):
        g = _fix(name)
        assert int(g['seed']) == SEED and str(g['sha256']) == R.state_sha256(sd)


@pytest.mark.parametrize('name', ['featext_1x72x104', 'featext_3x40x56'])
def test_restatement_matches_reference(name):
    g = _fix(name)
    outs = R.featext64(R.make_state_dict(SEED), torch.from_numpy(g['x']))
    for o, key in zip(outs, ('out1', 'out2', 'out3')):
        ref = g[key]
        assert o.shape == ref.shape
        scale = float(np.abs(ref).max())
        assert scale > 0.1
        assert float((o - torch.from_numpy(ref).double()).abs().max()) < 1e-4 * scale, key


def test_checkpoint_key_mapping(tmp_path):
    ckpt = R.make_checkpoint(SEED)
    p = tmp_path / 'vismvsnet.pt'
    torch.save(ckpt, str(p))
    m = FeatExt.from_checkpoint(str(p))
    sd = R.make_state_dict(SEED)
    got = m.state_dict()
    assert sorted(got) == sorted(sd)
    for k in sd:
        assert torch.equal(got[k], sd[k]), k
    # the names the issue / reference use
    for k in ('init_conv.0.weight', 'unet.enc_blocks.2d4_1.0.downsample.1.running_var', 'unet.dec_blocks.2d16_3.2.0.conv1.weight',
              'unet.dec_blocks.2d8_4.0.weight', 'init_conv.1.num_batches_tracked'):
        assert k in got
    # the layer table covers every parameter and buffer except the BatchNorm counters
    mods = dict(m.named_modules())
    covered = set()
    for conv, bn in features.LAYERS:
        covered.add(conv + '.weight')
        if bn:
            covered |= {bn + s for s in ('.weight', '.bias', '.running_mean', '.running_var')}
    assert covered == {k for k in got if not k.endswith('num_batches_tracked')}
    assert all(c in mods for c, _ in features.LAYERS)
    assert m.raw_params().numel() == sum(v.numel() for k, v in sd.items() if not k.endswith('num_batches_tracked'))


def test_checkpoint_with_other_pickled_objects(tmp_path):
    import argparse
    ckpt = R.make_checkpoint(SEED)
    ckpt['args'] = argparse.Namespace(lr=1e-3)                  # not a tensor or a plain container
    p = tmp_path / 'full.pt'
    torch.save(ckpt, str(p))
    with pytest.raises(RuntimeError, match='weights_only=False'):
        FeatExt.from_checkpoint(str(p))
    m = FeatExt.from_checkpoint(str(p), weights_only=False)
    assert torch.equal(m.state_dict()['final_conv_2.weight'], R.make_state_dict(SEED)['final_conv_2.weight'])


def test_checkpoint_missing_or_extra_keys_fail_like_strict_load():
    sd = R.make_state_dict(SEED)
    missing = dict(sd)
    del missing['unet.enc_blocks.2d8_2.1.bn2.running_mean']
    with pytest.raises(RuntimeError, match='Missing key'):
        FeatExt().load_state_dict(missing)
    extra = dict(sd)
    extra['unet.enc_blocks.2d8_2.2.conv1.weight'] = torch.zeros(1)
    with pytest.raises(RuntimeError, match='Unexpected key'):
        FeatExt().load_state_dict(extra)
    bad = dict(sd)
    bad['final_conv_3.weight'] = torch.zeros(32, 64, 3, 3)
    with pytest.raises(RuntimeError, match='size mismatch'):
        FeatExt().load_state_dict(bad)


@pytest.mark.parametrize('hw', [(70, 104), (72, 100), (6, 8), (1, 8), (16, 12)])
def test_shape_rule(hw):
    with pytest.raises(ValueError):
        features.output_hw(*hw)


def test_shape_rule_accepts_what_the_decoder_can_concatenate():
    assert features.output_hw(72, 104) == (36, 52)
    assert features.output_hw(71, 103) == (36, 52)
    assert features.output_hw(1200, 1600) == (600, 800)


def test_library_rejects_the_same_shapes():
    from mvsdf_amd import _lib
    L = _lib.lib()
    assert L.mvsdf_featext_workspace_bytes(1, 72, 104) > 0
    assert L.mvsdf_featext_workspace_bytes(1, 70, 104) == 0
    assert L.mvsdf_featext_workspace_bytes(0, 72, 104) == 0
    assert L.mvsdf_featext_raw_floats() == FeatExt().raw_params().numel()
    assert L.mvsdf_featext_layer_workspace_bytes(0, 48, 24, 3, 1) == 0           # cout not a tile multiple
    assert L.mvsdf_featext_layer_workspace_bytes(1, 3, 16, 3, 2) == 0            # transposed on the generic path


def test_pfm_matches_reference_and_round_trips(tmp_path):
    g = _fix('io')
    for key in ('depth', 'colour'):
        p = tmp_path / (key + '.pfm')
        p.write_bytes(g[key + '_pfm'].tobytes())
        got = sio.load_pfm(str(p))
        assert got.dtype == np.float32 and np.array_equal(got, g[key])
        q = tmp_path / (key + '2.pfm')
        sio.write_pfm(str(q), g[key + '_src'], scale=1 if key == 'depth' else 2)
        assert q.read_bytes() == g[key + '_pfm'].tobytes()
        assert np.array_equal(sio.load_pfm(str(q)), g[key + '_src'])
    with pytest.raises(Exception):
        sio.write_pfm(str(tmp_path / 'x.pfm'), np.zeros((2, 2), np.float64))


def test_cam_pair_and_scale_match_reference(tmp_path):
    g = _fix('io')
    for nw in (29, 30, 31):
        p = tmp_path / ('cam%d.txt' % nw)
        p.write_bytes(g['cam%d_txt' % nw].tobytes())
        assert np.array_equal(sio.load_cam(str(p), 256, 1), g['cam%d' % nw])
        assert np.array_equal(sio.load_cam(str(p), 128, 0.5), g['cam%d_s' % nw])
        assert np.array_equal(sio.load_cam(str(p), 128, 1, override=(nw == 31)), g['cam%d_o' % nw])
    assert np.array_equal(sio.scale_camera(g['cam29'], 2), g['cam29_scaled'])
    assert np.array_equal(sio.scale_camera(g['cam29'], (0.5, 0.25)), g['cam29_scaled_xy'])
    t = sio.scale_camera(torch.from_numpy(np.stack([g['cam29'], g['cam30']])), 2)
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), g['cam29_scaled_t'])
    p = tmp_path / 'pair.txt'
    p.write_bytes(g['pair_txt'].tobytes())
    assert repr(sio.load_pair(str(p))) == str(g['pair'])
    assert repr(sio.load_pair(str(p), min_views=2)) == str(g['pair_min2'])


def _random_P(rs, sign=1.0):
    K = np.array([[rs.uniform(300, 3000), rs.uniform(-5, 5), rs.uniform(100, 800)], [0, rs.uniform(300, 3000), rs.uniform(100, 600)], [0, 0, 1]])
    Rm = np.linalg.qr(rs.standard_normal((3, 3)))[0]
    if np.linalg.det(Rm) < 0:
        Rm[:, 0] = -Rm[:, 0]
    c = rs.standard_normal(3) * 3
    return sign * rs.uniform(0.1, 10) * K @ np.hstack([Rm, -Rm @ c[:, None]]), K, Rm, c


@pytest.mark.parametrize('seed', range(6))
def test_load_K_Rt_from_P(seed):
    rs = np.random.RandomState(seed)
    P, K0, R0, c0 = _random_P(rs, sign=-1.0 if seed % 2 else 1.0)
    intr, pose = sio.load_K_Rt_from_P(None, P.astype(np.float32))
    K = intr[:3, :3]
    assert intr.dtype == np.float64 and pose.dtype == np.float32
    assert np.allclose(np.tril(K, -1), 0) and (np.diag(K) > 0).all() and K[2, 2] == 1.0
    Rw = pose[:3, :3].astype(np.float64).T
    assert np.allclose(Rw @ Rw.T, np.eye(3), atol=1e-5) and np.linalg.det(Rw) > 0
    assert np.allclose(K, K0, rtol=1e-4, atol=1e-3)
    assert np.allclose(pose[:3, 3], c0, rtol=1e-4, atol=1e-4)
    Pr = K @ np.hstack([Rw, -Rw @ pose[:3, 3:4].astype(np.float64)])
    s = (Pr * P).sum() / (Pr * Pr).sum()
    assert np.allclose(s * Pr, P, rtol=1e-4, atol=1e-4 * np.abs(P).max())
    assert np.array_equal(intr[3], [0, 0, 0, 1]) and np.array_equal(pose[3], [0, 0, 0, 1])


def test_load_rgb_and_mask_value_rules(tmp_path):
    from PIL import Image
    rs = np.random.RandomState(0)
    img = rs.randint(0, 256, (5, 7, 3)).astype(np.uint8)
    Image.fromarray(img).save(str(tmp_path / 'a.png'))
    rgb = sio.load_rgb(str(tmp_path / 'a.png'))
    assert rgb.shape == (3, 5, 7) and rgb.dtype == np.float32
    want = (img.astype(np.float64) * (1 / 255.0)).astype(np.float32)
    want = (want - np.float32(0.5)) * np.float32(2.0)
    assert np.array_equal(rgb, want.transpose(2, 0, 1))
    m = rs.randint(0, 256, (5, 7, 3)).astype(np.uint8)
    m[0, 0] = 255
    m[0, 1] = 0
    Image.fromarray(m).save(str(tmp_path / 'm.png'))
    grey = m[..., 0] * 0.299 + m[..., 1] * 0.587 + m[..., 2] * 0.114
    mask = sio.load_mask(str(tmp_path / 'm.png'))
    assert mask.dtype == bool and mask.shape == (5, 7) and mask[0, 0] and not mask[0, 1]
    sure = np.abs(grey - 127.5) > 1
    assert np.array_equal(mask[sure], (grey > 127.5)[sure])
    Image.fromarray(m[..., 0]).save(str(tmp_path / 'l.png'))
    assert np.array_equal(sio.load_mask(str(tmp_path / 'l.png')), m[..., 0] > 127.5)
