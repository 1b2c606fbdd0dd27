"""upsample_depth, band_sweep and cascade_sweep (csrc/stereo.hip: k_ps_upsample, k_ps_band) against the numpy restatement
tests/stereo_cascade_ref.py, bit for bit with no exemption (equal values, equal NaN positions), estimate_scene(cascade=...) end to end into the
fusion and the converter, and features.extract_pyramid."""
import filecmp
import os

import numpy as np
import pytest
import torch

import stereo_cascade_ref as CR
import stereo_ref as R
import stereo_scene as SC
import stereo_sgm_ref as G
from mvsdf_amd import stereo

pytestmark = pytest.mark.gpu

MAPS = ('depths', 'probs', 'best_k', 'counts')


def _same(got, want, name):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(np.isnan(got), np.isnan(want)), '%s: the NaN positions differ' % name
    ok = ~np.isnan(want)
    bad = int((got[ok] != want[ok]).sum())
    assert bad == 0 and np.array_equal(got[ok], want[ok]), '%s: %d of %d elements differ' % (name, bad, want.size)


# ---------------------------------------------------------------- upsample_depth ----------------------------------------------------------------
@pytest.mark.parametrize('small,size', [((2, 2), (2, 2)), ((2, 2), (5, 7)), ((3, 5), (6, 10)), ((4, 6), (7, 13)), ((8, 8), (3, 3))],
                         ids=lambda v: '%dx%d' % v)
def test_upsample_depth_is_the_restatement(small, size):
    rs = np.random.RandomState(small[0] * 100 + size[1])
    V = 3
    depth = rs.uniform(2.9, 4.25, size=(V,) + small).astype(np.float32)
    best_k = rs.randint(0, 24, size=(V,) + small).astype(np.int32)
    best_k[rs.uniform(size=best_k.shape) < 0.2] = -1
    best_k[1, :2, :2] = -1                                                     # pixel (0, 0) of view 1 has no valid tap
    best_k[2] = -1                                                             # nor has any pixel of view 2
    want = CR.upsample(depth, best_k, size)
    assert np.isnan(want[1, 0, 0]) and np.isnan(want[2]).all() and not np.isnan(want[0]).all()
    got = stereo.upsample_depth(depth, best_k, size)
    assert got.is_cuda and got.dtype == torch.float64
    _same(got, want, 'centres %s -> %s' % (small, size))
    _same(stereo.upsample_depth(torch.from_numpy(depth).cuda(), torch.from_numpy(best_k).cuda(), size), want, 'from device tensors')


# ---------------------------------------------------------------- band_sweep ----------------------------------------------------------------
# (V, R, S, C, D_b, the descriptor base misaligned by one float): one pixel row of one hypothesis; fewer hypotheses than waves; C = 25 and 32 (the float4
# path) on sizes that are no multiple of the 8 x 8 tile, several tiles; the float4 path's alignment fallback; the largest band
BANDS = [(2, 2, 2, 1, 1, False), (3, 5, 7, 3, 2, False), (3, 9, 11, 25, 3, False), (3, 17, 33, 32, 16, False), (3, 19, 21, 32, 5, True),
         (2, 9, 11, 32, stereo.MAX_D_BAND, False)]


def _band_case(V, Rr, S, C, Db, seed):
    rs = np.random.RandomState(seed)
    cams, pairs = SC.make_cams(V, (Rr, S), 1.5625 * S, 24)
    desc = R.normalize(rs.normal(size=(V, Rr, S, C)))
    steps = cams[0, 1, 3, 1] * np.array([1.0, 1.5, 0.75])[:V]
    c = rs.uniform(SC.DEPTH_MIN, SC.DEPTH_MAX, size=(V, Rr, S))
    pick = rs.uniform(size=c.shape)
    c[pick < 0.05] = np.nan
    c[(pick >= 0.05) & (pick < 0.10)] = 0.4 * Db * steps[0] * 0.5            # part of the band has d <= 0 (all of it where D_b = 1 or 2)
    c[(pick >= 0.10) & (pick < 0.13)] = -1.0                                  # all of it has
    c[(pick >= 0.13) & (pick < 0.18)] = 1e6                                   # far beyond the scene
    c[(pick >= 0.18) & (pick < 0.23)] = 0.3 + Db * steps[0]                   # in front of it: the sources' rays leave their images
    c[0, 0, 0], c[V - 1, Rr - 1, S - 1], c[0, 0, 1] = np.nan, -1.0, 0.3 + Db * steps[0]
    return cams, pairs, desc, steps, c


@pytest.mark.parametrize('shape', BANDS, ids=lambda s: '%dx%dx%dx%d_D%d%s' % (s[:5] + ('_misaligned' if s[5] else '',)))
def test_band_sweep_is_the_restatement(shape):
    V, Rr, S, C, Db, misaligned = shape
    cams, pairs, desc, steps, c = _band_case(V, Rr, S, C, Db, sum(shape[:5]))
    views = [2, 0] if V == 3 else [1, 0]
    dev = torch.from_numpy(desc).cuda()
    if misaligned:
        flat = torch.empty(desc.size + 1, dtype=torch.float32, device='cuda')
        flat[1:] = dev.reshape(-1)
        dev = flat[1:].view(desc.shape)
        assert dev.data_ptr() % 16 == 4 and dev.is_contiguous()
    unseen = 0
    for num_src in (0, 1, 3):
        want = CR.band(desc, cams, pairs, c, Db, steps, num_src, views)
        got = stereo.band_sweep(dev if num_src else desc, cams, pairs, torch.from_numpy(c).cuda() if num_src == 1 else c, Db, steps, num_src=num_src,
                                views=views)
        assert got.depths.is_cuda and got.depths.dtype == torch.float32 and got.best_k.dtype == torch.int32 and got.scores is None
        for name in MAPS:
            _same(getattr(got, name), want[name], '%s num_src %d' % (name, num_src))
        band_front = c - (Db // 2) * steps[:, None, None]
        unseen += int(((want['best_k'] == -1) & (band_front > 0))[views].sum()) if num_src else 0
        if num_src:
            assert (want['best_k'][views] >= 0).any() or Rr == 2
        else:
            assert (want['best_k'] == -1).all()
        assert (want['best_k'][[v for v in range(V) if v not in views]] == -1).all()
    assert unseen > 0                                                          # every hypothesis in front of the camera and no source sees one
    one = stereo.band_sweep(dev, cams, pairs, c, Db, float(steps[0]), views=[0])           # one step for all
    _same(one.depths, CR.band(desc, cams, pairs, c, Db, np.full(V, steps[0]), 2, [0])['depths'], 'a single step')


def test_an_infinite_centre_raises_and_the_workspace_is_small():
    V, Rr, S, C, Db = 3, 9, 11, 32, 4
    cams, pairs, desc, steps, c = _band_case(V, Rr, S, C, Db, 3)
    want = CR.band(desc, cams, pairs, c, Db, steps, 2)
    good = torch.from_numpy(c).cuda()
    for value in (float('inf'), -float('inf')):
        bad = good.clone()
        bad[1, 8, 10] = value                                                  # a device tensor: the kernel finds it
        with pytest.raises(ValueError, match='infinite'):
            stereo.band_sweep(desc, cams, pairs, bad, Db, steps)
        got = stereo.band_sweep(desc, cams, pairs, good, Db, steps)
        for name in MAPS:
            _same(getattr(got, name), want[name], name + ' after the refusal')
    nan = torch.from_numpy(desc).cuda()
    nan[0, 1, 2, 3] = float('nan')
    with pytest.raises(ValueError, match='NaN or infinite'):
        stereo.band_sweep(nan, cams, pairs, good, Db, steps)
    from mvsdf_amd._lib import lib
    size = lib().mvsdf_stereo_band_workspace_bytes
    base = size(9, 11, 4, 3, 6)
    assert 0 < base < 4096
    assert size(9, 11, 1, 3, 6) == base and size(9, 11, stereo.MAX_D_BAND, 3, 6) == base and size(288, 384, 16, 3, 6) == base and size(2, 2, 16, 3, 6) == base
    assert size(9, 11, stereo.MAX_D_BAND + 1, 3, 6) == 0 and size(9, 11, 0, 3, 6) == 0 and size(1, 11, 4, 3, 6) == 0


# ---------------------------------------------------------------- cascade_sweep ----------------------------------------------------------------
def _rendered(sizes, V=3, n_depths=48):
    """the scene rendered through the scaled cameras of every stage -> (cams at the last size, pairs, unit patch descriptors per stage)"""
    RL, SL = sizes[-1]
    cams, pairs = SC.make_cams(V, (RL, SL), 1.5625 * SL, n_depths)
    descs = [R.normalize(R.patches(SC.render(CR.scale_cams(cams, s / SL, r / RL), (r, s))[0], 2)) for r, s in sizes]
    return cams, pairs, descs


@pytest.fixture(scope='module', params=[[(8, 12), (16, 24), (32, 48)], [(7, 11), (16, 24), (33, 47)]], ids=['ratio2', 'odd_ratios'])
def rendered(request):
    return _rendered(request.param)


@pytest.mark.parametrize('regularize', [None, True], ids=['wta', 'sgm'])
def test_cascade_sweep_is_the_restatement(rendered, regularize):
    cams, pairs, descs = rendered
    want = CR.cascade(descs, cams, pairs, 2, None, (None, 8, 4), (4, 2, 1), G.DEFAULTS if regularize else None)
    got = stereo.cascade_sweep(descs, cams, pairs, depth_nums=(None, 8, 4), regularize=regularize)
    assert isinstance(got, stereo.Cascade) and len(got.stages) == 3
    for name in MAPS:
        _same(getattr(got, name), want[name], name)
        for l in range(3):
            _same(getattr(got.stages[l], name), want['stages'][l][name], '%s of stage %d' % (name, l + 1))
    assert tuple(got.stages[0].depths.shape) == (3,) + descs[0].shape[1:3] and (want['best_k'] >= 0).mean() > 0.8
    assert (want['probs'][:, 1] != want['stages'][2]['probs'][:, 1]).any()     # probs[1] is stage 1's


def test_cascade_views_and_device_tensors(rendered):
    cams, pairs, descs = rendered
    want = CR.cascade(descs[1:], cams, pairs, 1, [2, 0], (12, 5), (3, 1.5))
    got = stereo.cascade_sweep([torch.from_numpy(d).cuda() for d in descs[1:]], cams, pairs, num_src=1, views=[2, 0], depth_nums=(12, 5),
                               interval_scales=(3, 1.5))
    for name in MAPS:
        _same(getattr(got, name), want[name], name)
    assert (want['best_k'][1] == -1).all() and (want['best_k'][0] >= 0).any()


def test_one_stage_of_scale_one_is_plane_sweep(rendered):
    cams, pairs, descs = rendered
    for reg in (None, True):
        plain = stereo.plane_sweep(descs[2], cams, pairs, regularize=reg)
        got = stereo.cascade_sweep([descs[2]], cams, pairs, depth_nums=(None,), interval_scales=(1,), regularize=reg)
        for name in MAPS:
            _same(getattr(got, name), getattr(plain, name).cpu().numpy(), name)


# ---------------------------------------------------------------- end to end ----------------------------------------------------------------
def test_estimate_scene_cascade_feeds_the_fusion_and_the_converter(tmp_path):
    """images, cams/ and pair.txt -> estimate_scene(cascade=...) -> load_mvs_output -> fuse_depths -> convert_scene(range_source='clean'), the chain
    of test_gpu_stereo.py with 96 hypotheses swept as 24 / 16 / 8: the median distance of the fused cloud to the sphere is within 4 of these
    intervals (that test's one interval at 24 hypotheses), and the fused cloud has as many points as the one from the numpy restatement's maps."""
    from mvsdf_amd import fusion
    from mvsdf_amd.datasets import prepare
    from mvsdf_amd.utils import io as sio
    root, ids, cams_hd, pairs = SC.write_scene(tmp_path / 'scan', n_depths=96)
    out = str(tmp_path / 'out')
    cas = stereo.estimate_scene(root, out, cascade=((None, 16, 8), (4, 2, 1)))
    assert isinstance(cas, stereo.Cascade) and tuple(cas.depths.shape) == (5, 64, 96) and tuple(cas.stages[0].depths.shape) == (5, 16, 24)
    pair, cams, depths, probs = prepare.load_mvs_output(out)
    assert np.array_equal(depths, cas.depths.cpu().numpy()) and np.array_equal(probs, cas.probs.cpu().numpy())
    assert prepare.pair_indices(pair) == pairs and cams[0, 1, 0, 0] == 150.0 and cams[0, 1, 0, 2] == 48.0
    fused = fusion.fuse_depths(cams, depths, prepare.pair_indices(pair), probs=probs, pthresh=stereo.PTHRESH)
    interval = (SC.DEPTH_MAX - SC.DEPTH_MIN) / 95
    dist = np.abs(np.linalg.norm(fused.points.cpu().numpy() - SC.CENTER, axis=1) - SC.RADIUS)
    print('%d fused points, median distance to the surface %.4f = %.3f intervals' % (len(fused), np.median(dist), np.median(dist) / interval))
    assert np.median(dist) <= 4 * interval
    # the same chain on the restatement
    images = [prepare.load_image_u8(os.path.join(root, 'images', '%s.png' % i.zfill(8))) for i in ids]
    sizes = [(16, 24), (32, 48), (64, 96)]
    descs = [R.normalize(R.patches(np.stack([prepare.resize_bilinear_u8(im, s, r) for im in images]), 2)) for r, s in sizes]
    cams_ref = np.stack([sio.scale_camera(sio.load_cam(os.path.join(root, 'cams', '%s_cam.txt' % i.zfill(8)), 256, 1), (0.5, 0.5)) for i in ids])
    ref = CR.cascade(descs, cams_ref, pairs, 2, None, (None, 16, 8), (4, 2, 1))
    for name in MAPS:
        _same(getattr(cas, name), ref[name], name)
    fused_ref = fusion.fuse_depths(cams, ref['depths'], pairs, probs=ref['probs'], pthresh=stereo.PTHRESH)
    assert len(fused_ref) == len(fused) > 5000
    scene_dir = prepare.convert_scene(out, range_source='clean', pthresh=stereo.PTHRESH, prob_mask=True, resize='192,128', crop='192,128',
                                      ext_image_path=os.path.join(root, 'images', '{:08}.png'))
    for name in ('cameras_hd.npz', 'image_hd/000004.png', 'mask_hd/004.png', 'depth/004.pfm'):
        assert os.path.exists(os.path.join(scene_dir, name)), name
    assert os.path.exists(os.path.join(out, 'cut.ply'))


def test_without_cascade_the_files_are_the_full_sweep(tmp_path):
    root, ids, cams_hd, pairs = SC.write_scene(tmp_path / 'scan', n_views=3, img_hw=(64, 96), focal=150.0, n_depths=12)
    outs = []
    for tag, kw in (('plain', {}), ('none', dict(cascade=None)), ('false', dict(cascade=False))):
        outs.append(str(tmp_path / tag))
        sweep = stereo.estimate_scene(root, outs[-1], **kw)
        assert isinstance(sweep, stereo.Sweep)
    names = sorted(os.listdir(outs[0]))
    assert len(names) == 3 * 6 + 1
    for other in outs[1:]:
        assert sorted(os.listdir(other)) == names
        match, mismatch, errors = filecmp.cmpfiles(outs[0], other, names, shallow=False)
        assert not mismatch and not errors, (mismatch, errors)
    cams, _ = SC.make_cams(3, (32, 48), 75.0, 12)
    images = SC.render(SC.make_cams(3, (64, 96), 150.0, 12)[0], (64, 96))[0]
    from mvsdf_amd.datasets import prepare
    desc = R.normalize(R.patches(np.stack([prepare.resize_bilinear_u8(im, 48, 32) for im in images]), 2))
    _same(sweep.depths, R.sweep(desc, cams, pairs, 2)['depths'], 'the full sweep')


def test_extract_pyramid_is_featext():
    from mvsdf_amd.features import FeatExt, extract_features, extract_pyramid, output_hw
    torch.manual_seed(3)
    net = FeatExt().cuda().eval()
    assert output_hw(7, 7) == (4, 4)
    with pytest.raises(ValueError):
        output_hw(6, 7)
    rgb = torch.randn(3, 3, 7, 7, generator=torch.Generator().manual_seed(4))
    pyr = extract_pyramid(net, rgb, batch=2)
    assert [tuple(p.shape) for p in pyr] == [(3, 1, 1, 32), (3, 2, 2, 32), (3, 4, 4, 32)] and all(p.is_cuda and p.is_contiguous() for p in pyr)
    assert torch.equal(pyr[2], extract_features(net, rgb).permute(0, 2, 3, 1))
    fwd = net(rgb.cuda())
    for p, f in zip(pyr, fwd):
        assert torch.equal(p, f.permute(0, 2, 3, 1))
