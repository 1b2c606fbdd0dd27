"""plane_sweep, normalize_descriptors and patch_descriptors (csrc/stereo.hip) against the numpy restatement tests/stereo_ref.py, bit for bit with no
exemption, and estimate_scene end to end into the fusion and the converter."""
import os

import numpy as np
import pytest
import torch

import mvs_scene as MS
import stereo_ref as R
import stereo_scene as SC
from mvsdf_amd import stereo

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32 if a.dtype in (np.float32, np.int32) else np.uint8)


def _same(got, want, name):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    bad = int((_bits(got) != _bits(want)).sum())
    assert bad == 0, '%s: %d of %d elements differ' % (name, bad, want.size)


def _check(desc, cams, pairs, num_src=2, views=None):
    """plane_sweep == stereo_ref.sweep in every output and in the score volume of the last view (NaN positions included), twice in a row -> the ref"""
    ref = R.sweep(desc.cpu().numpy() if isinstance(desc, torch.Tensor) else desc, cams, pairs, num_src, views)
    for _ in range(2):
        o = stereo.plane_sweep(desc, cams, pairs, num_src=num_src, views=views, scores=True)
        assert o.depths.is_cuda and o.depths.dtype == torch.float32 and o.probs.dtype == torch.float32
        assert o.best_k.dtype == torch.int32 and o.counts.dtype == torch.int32
        for name in ('depths', 'probs', 'best_k', 'counts'):
            _same(getattr(o, name), ref[name], name)
        if ref['scores'] is None:
            assert o.scores is None
        else:
            assert o.scores.dtype == torch.float64
            _same(o.scores, ref['scores'], 'scores')                           # the restatement's NaN is numpy's quiet NaN, as the kernel's
    return ref


def _descriptors(images, radius):
    """both descriptor functions against the restatement -> fp32 numpy unit descriptors"""
    raw = stereo.patch_descriptors(images, radius)
    want = R.patches(images, radius)
    _same(raw, want, 'patch_descriptors')
    desc = stereo.normalize_descriptors(raw)
    _same(desc, R.normalize(want), 'normalize_descriptors')
    return desc.cpu().numpy()


@pytest.fixture(scope='module')
def scene():
    cams, pairs = SC.make_cams(5, (64, 96))
    images, gt = SC.render(cams, (64, 96))
    return cams, pairs, gt, images, _descriptors(images, 2)


def test_synthetic_scene(scene):
    cams, pairs, gt, images, desc = scene
    assert desc.shape[-1] == 25
    ref = _check(desc, cams, pairs)
    assert (ref['best_k'] >= 0).mean() > 0.9 and ref['counts'].max() == 2


@pytest.mark.parametrize('hw', [(2, 2), (17, 16), (37, 53), (16, 33)])
def test_odd_shapes(hw):
    cams, pairs = SC.make_cams(4, hw, focal=1.5 * hw[1], n_depths=7)
    images, _ = SC.render(cams, hw)
    ref = _check(_descriptors(images, 1), cams, pairs)
    assert hw == (2, 2) or (ref['best_k'] >= 0).any()


@pytest.mark.parametrize('C', [1, 25, 32, 49])
def test_channel_counts(C):
    cams, pairs = SC.make_cams(4, (21, 30), focal=45.0, n_depths=9)
    feats = np.random.RandomState(C).normal(size=(4, 21, 30, C)).astype(np.float32)
    feats[2, 5, 6] = 0                                                        # a zero-norm texel
    desc = stereo.normalize_descriptors(feats)
    _same(desc, R.normalize(feats), 'normalize_descriptors')
    ref = _check(desc.cpu().numpy(), cams, pairs)
    assert (ref['best_k'] >= 0).any()
    _check(desc, cams, pairs, views=[2])                                      # a device tensor is used where it is


def test_pair_lists_num_src_and_views(scene):
    cams, pairs, gt, images, desc = scene
    desc, cams = desc[:, :24, :40], cams.copy()
    cams[:, 1, 0, 2], cams[:, 1, 1, 2] = 20.0, 12.0
    _check(desc, cams, pairs, num_src=10)                                     # more than the four sources there are
    _check(desc, cams, pairs, num_src=1)
    ref = _check(desc, cams, pairs, num_src=0)
    assert (ref['best_k'] == -1).all() and np.isnan(ref['scores']).all()
    some = [list(p) for p in pairs]
    some[2] = []
    ref = _check(desc, cams, some)
    assert (ref['depths'][2] == 0).all() and (ref['probs'][2] == 0).all()
    ref = _check(desc, cams, [p + p for p in pairs], num_src=8)               # a source may be listed twice: it counts twice
    assert ref['counts'].max() == 8
    ref = _check(desc, cams, pairs, views=[3, 1])
    assert (ref['best_k'][[0, 2, 4]] == -1).all() and (ref['best_k'][1] >= 0).any()
    _check(desc, cams, pairs, views=[])
    mixed = cams.copy()
    mixed[1, 1, 3, :3] = [3.0, 0.11, 5]                                       # every view sweeps its own range and number of hypotheses
    _check(desc, mixed, pairs, views=[0, 1])
    _check(desc, mixed, pairs, views=[1, 0])


def test_hypotheses_behind_and_outside_a_source():
    """source 1 looks away from the scene (p2 <= 0 at every hypothesis), source 2 is turned so that the sweep leaves its image part of the way, and
    the depth range of view 0 starts behind source 3"""
    cams, pairs = SC.make_cams(5, (37, 53), focal=80.0, n_depths=12)
    images, _ = SC.render(cams, (37, 53))
    desc = _descriptors(images, 1)
    cams[1, 0, :3] = np.diag([-1.0, 1.0, -1.0]) @ cams[1, 0, :3]              # turned about its y axis by half a turn
    a = 0.25
    cams[2, 0, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ cams[2, 0, :3]
    cams[3, 0, 2, 3] -= 3.2                                                   # pushed forward: the near hypotheses are behind it
    pairs = [[1, 2, 3], [0, 2], [0, 3, 1], [0, 4], [3]]
    ref = _check(desc, cams, pairs, num_src=3)
    o = R.sweep_view(desc, cams, pairs, 0, 3)
    assert o['n'].max() == 2 and (o['n'] == 0).any() and (o['n'] == 1).any()
    assert (o['n'][0] < o['n'][-1]).any()                                     # a source joins as the depth grows
    assert (ref['counts'][0] >= 1).any()


def test_exact_ties_and_the_last_column():
    """identical cameras with exact matrices: u = x exactly, so the last column has u = S - 1 and x0 = S - 2, fx = 1; +-0.5 descriptors score exactly
    1 at every hypothesis, so every pixel is an exact tie and the lowest k wins"""
    cams, _, pairs = MS.exact_self_pair()
    cams = cams.copy()
    cams[:, 1, 3] = [1.0, 0.5, 8, 4.5]
    f = np.random.RandomState(0).choice([-1.0, 1.0], size=(1, 16, 32, 4)).astype(np.float32)
    desc = stereo.normalize_descriptors(np.concatenate([f, f]))
    ref = _check(desc.cpu().numpy(), cams, pairs)
    assert (ref['best_k'] == 0).all() and np.array_equal(ref['scores'], np.ones((8, 16, 32))) and (ref['probs'][:, 0] == 1).all()
    ones = np.ones((2, 16, 32, 1), np.float32)                                # C = 1: every score is 1 as well
    ref = _check(ones, cams, pairs)
    assert (ref['best_k'] == 0).all()


def test_featext_features_flow_into_the_sweep():
    from mvsdf_amd.features import FeatExt, extract_features
    torch.manual_seed(0)
    net = FeatExt().cuda().eval()
    cams, pairs = SC.make_cams(3, (32, 48), focal=75.0, n_depths=8)
    images, _ = SC.render(SC.make_cams(3, (64, 96), focal=150.0)[0], (64, 96))
    rgb = torch.from_numpy(images).permute(0, 3, 1, 2).float() / 255
    feats = extract_features(net, rgb).permute(0, 2, 3, 1).contiguous()
    assert tuple(feats.shape) == (3, 32, 48, 32) and feats.is_cuda
    desc = stereo.normalize_descriptors(feats)
    _same(desc, R.normalize(feats.cpu().numpy()), 'normalize_descriptors')
    ref = _check(desc, cams, pairs)
    assert (ref['best_k'] >= 0).any()


def test_errors_raise_and_leave_the_device_usable(scene):
    cams, pairs, gt, images, desc = scene
    desc = torch.from_numpy(desc[:, :16, :16].copy()).cuda()
    good = stereo.plane_sweep(desc, cams, pairs)
    bad = desc.clone()
    bad[3, 2, 1, 0] = float('nan')
    inf = desc.clone()
    inf[0, 15, 15, 24] = float('inf')
    for d in (bad, inf):                                                      # device tensors: the kernels find the value
        with pytest.raises(ValueError):
            stereo.plane_sweep(d, cams, pairs)
        with pytest.raises(ValueError):
            stereo.normalize_descriptors(d)
        again = stereo.plane_sweep(desc, cams, pairs)
        assert torch.equal(again.depths, good.depths) and torch.equal(again.probs, good.probs)
    from mvsdf_amd._lib import lib
    assert lib().mvsdf_stereo_workspace_bytes(1, 16, 4, 2) == 0 and lib().mvsdf_stereo_workspace_bytes(16, 16, 0, 2) == 0
    assert lib().mvsdf_stereo_workspace_bytes(16, 16, 4, 2) > lib().mvsdf_stereo_volume_offset(16, 16, 4, 2) > 0


def test_estimate_scene_feeds_the_fusion_and_the_converter(tmp_path):
    """images, cams/ and pair.txt -> estimate_scene -> load_mvs_output -> fuse_depths -> convert_scene(range_source='clean').  The fused points are
    averages of depths whose winners are correct to within half an interval where the sweep is right, so the median distance of the fused cloud
    to the true surface must be within one depth interval."""
    from mvsdf_amd import fusion
    from mvsdf_amd.datasets import prepare
    root, ids, cams_hd, pairs = SC.write_scene(tmp_path / 'scan')
    out = str(tmp_path / 'out')
    sweep = stereo.estimate_scene(root, out)
    assert tuple(sweep.depths.shape) == (5, 64, 96)
    pair, cams, depths, probs = prepare.load_mvs_output(out)
    assert np.array_equal(depths, sweep.depths.cpu().numpy()) and np.array_equal(probs, sweep.probs.cpu().numpy())
    assert prepare.pair_indices(pair) == pairs and cams[0, 1, 0, 0] == 150.0 and cams[0, 1, 0, 2] == 48.0
    fused = fusion.fuse_depths(cams, depths, prepare.pair_indices(pair), probs=probs, pthresh=stereo.PTHRESH)
    assert len(fused) > 5000
    interval = (SC.DEPTH_MAX - SC.DEPTH_MIN) / 23
    dist = np.abs(np.linalg.norm(fused.points.cpu().numpy() - SC.CENTER, axis=1) - SC.RADIUS)
    print('%d fused points, median distance to the surface %.4f = %.3f intervals' % (len(fused), np.median(dist), np.median(dist) / interval))
    assert np.median(dist) <= interval
    scene_dir = prepare.convert_scene(out, range_source='clean', pthresh=stereo.PTHRESH, prob_mask=True, resize='192,128', crop='192,128',
                                      ext_image_path=os.path.join(root, 'images', '{:08}.png'))
    for name in ('cameras_hd.npz', 'image_hd/000004.png', 'mask_hd/004.png', 'depth/004.pfm'):
        assert os.path.exists(os.path.join(scene_dir, name)), name
    assert os.path.exists(os.path.join(out, 'cut.ply')) and os.path.exists(os.path.join(out, 'all_torch.ply'))


def test_a_nonfinite_feature_is_found_at_the_end_and_beyond_the_first_grid_stride():
    """the finite check (csrc/geom_prims.h: k_any_nonfinite) runs a capped grid of 2048 x 256 lanes that strides over the descriptors: a NaN in the last
    element, and one that only a lane's second round reaches, must both raise"""
    V, R, S, C = 2, 96, 96, 32
    assert V * R * S * C > 2048 * 256 + 4096
    cams, pairs = SC.make_cams(V, (R, S), focal=225.0, n_depths=2)
    g = torch.Generator().manual_seed(5)
    desc = torch.nn.functional.normalize(torch.randn(V, R, S, C, generator=g), dim=3).cuda()
    good = stereo.plane_sweep(desc, cams, pairs)
    for at in (desc.numel() - 1, 2048 * 256 + 4095):
        bad = desc.clone()
        bad.view(-1)[at] = float('nan')
        with pytest.raises(ValueError, match='NaN or infinite'):
            stereo.plane_sweep(bad, cams, pairs)
    again = stereo.plane_sweep(desc, cams, pairs)
    assert torch.equal(again.depths, good.depths) and torch.equal(again.probs, good.probs)
