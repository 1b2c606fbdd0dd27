"""regularize_scores and plane_sweep(regularize=...) (csrc/stereo.hip: k_sg_path, k_ps_pick) against the numpy restatement tests/stereo_sgm_ref.py,
bit for bit with no exemption (equal values, equal NaN positions), and estimate_scene(regularize=True) end to end."""
import numpy as np
import pytest
import torch

import stereo_ref as R
import stereo_scene as SC
import stereo_sgm_ref as G
from mvsdf_amd import stereo

pytestmark = pytest.mark.gpu

PENALTIES = [(0.0, 0.0), (0.1, 0.8), (0.3, 0.3)]


def _same(got, want, name):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(np.isnan(got), np.isnan(want)), '%s: the NaN positions differ' % name
    ok = ~np.isnan(want)
    bad = int((got[ok] != want[ok]).sum())
    assert bad == 0 and np.array_equal(got[ok], want[ok]), '%s: %d of %d elements differ' % (name, bad, want.size)


def _volume(shape, seed):
    """uniform scores in [-1, 1]; about 15 % invalid, among them whole pixels and whole image rows (where the image has room for them)"""
    D, Rr, S = shape
    rs = np.random.RandomState(seed)
    v = rs.uniform(-1, 1, size=shape)
    v[rs.uniform(size=shape) < 0.12] = np.nan
    v[:, rs.uniform(size=(Rr, S)) < 0.03] = np.nan
    v[:, Rr // 2, S // 2] = np.nan
    if Rr >= 5:
        v[:, Rr // 3] = np.nan
    return v


# one and two hypotheses; sizes that are no multiple of a bundle of 8, 4, 2 or 1 paths; an image narrower than a bundle; 300 hypotheses > 256 lanes
# (bundles of 4 paths, five hypotheses per lane); 2100 and 4096 hypotheses: one path per workgroup, the second with the largest LDS image
SHAPES = [(1, 2, 2), (2, 3, 5), (3, 5, 7), (24, 17, 33), (65, 9, 70), (300, 6, 11), (2100, 2, 3), (4096, 3, 2)]


@pytest.fixture(scope='module')
def volumes():
    return {shape: _volume(shape, i) for i, shape in enumerate(SHAPES)}


@pytest.mark.parametrize('paths', [4, 8])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_regularize_scores_is_the_restatement(volumes, shape, paths):
    v = volumes[shape]
    dev = torch.from_numpy(v).cuda()
    for p1, p2 in PENALTIES:
        want = G.regularize(v, p1, p2, paths)
        got = stereo.regularize_scores(dev if p1 else v, p1, p2, paths)       # a device tensor is used where it is, a numpy array is copied
        assert got.is_cuda and got.dtype == torch.float64
        _same(got, want, 'A %s P1 %g P2 %g paths %d' % (shape, p1, p2, paths))
    _same(dev, v, 'the input')                                                # untouched


def test_defaults_and_an_infinite_score():
    v = _volume((5, 6, 7), 11)
    _same(stereo.regularize_scores(v), G.regularize(v), 'defaults')
    bad = torch.from_numpy(v).cuda()
    bad[2, 3, 4] = float('inf')
    with pytest.raises(ValueError, match='infinite'):
        stereo.regularize_scores(bad)
    _same(stereo.regularize_scores(v), G.regularize(v), 'after the refusal')
    from mvsdf_amd._lib import lib
    assert lib().mvsdf_stereo_sgm_workspace_bytes(6, 7, 5) > 0 and lib().mvsdf_stereo_sgm_workspace_bytes(6, 7, 4097) == 0
    assert lib().mvsdf_stereo_sgm_workspace_bytes(0, 7, 5) == 0
    assert lib().mvsdf_stereo_sweep_sgm_workspace_bytes(16, 16, 4, 2) == lib().mvsdf_stereo_workspace_bytes(16, 16, 4, 2) + 16 * 16 * 4 * 8


@pytest.fixture(scope='module')
def noisy():
    cams, pairs = SC.make_cams(5, (64, 96))
    images, _ = SC.render(cams, (64, 96))
    return cams, pairs, R.normalize(R.patches(G.noisy_images(images), 2))


@pytest.mark.parametrize('view', range(5))
def test_noisy_scene_view(noisy, view):
    cams, pairs, desc = noisy
    ref = G.sweep(desc, cams, pairs, 2, views=[view])
    o = stereo.plane_sweep(desc, cams, pairs, num_src=2, views=[view], scores=True, regularize=True)
    for name in ('depths', 'probs', 'best_k', 'counts', 'scores', 'reg_scores'):
        _same(getattr(o, name), ref[name], name)
    assert (ref['best_k'][view] >= 0).mean() > 0.9


def test_regularize_forms_and_the_unregularised_sweep(noisy):
    cams, pairs, desc = noisy
    desc, cams = desc[:, :24, :40], cams.copy()
    cams[:, 1, 0, 2], cams[:, 1, 1, 2] = 20.0, 12.0
    plain = stereo.plane_sweep(desc, cams, pairs, scores=True)
    none = stereo.plane_sweep(desc, cams, pairs, scores=True, regularize=None)
    assert none.reg_scores is None and plain.reg_scores is None
    for name in ('depths', 'probs', 'best_k', 'counts', 'scores'):
        _same(getattr(none, name), getattr(plain, name).cpu().numpy(), name)
    ref_plain = R.sweep(desc, cams, pairs, 2)
    for name in ('depths', 'probs', 'best_k', 'counts', 'scores'):
        _same(getattr(plain, name), ref_plain[name], name)
    for reg, args in (((0.05, 0.4), (0.05, 0.4, 8)), ((0.05, 0.4, 4), (0.05, 0.4, 4)), (True, G.DEFAULTS)):
        ref = G.sweep(desc, cams, pairs, 2, None, *args)
        o = stereo.plane_sweep(desc, cams, pairs, scores=True, regularize=reg)
        for name in ('depths', 'probs', 'best_k', 'counts', 'scores', 'reg_scores'):
            _same(getattr(o, name), ref[name], '%s %r' % (name, reg))
    mixed = cams.copy()
    mixed[1, 1, 3, :3] = [3.0, 0.11, 5]                                       # every view regularises its own number of hypotheses
    ref = G.sweep(desc, mixed, pairs, 2, [0, 1])
    o = stereo.plane_sweep(desc, mixed, pairs, views=[0, 1], scores=True, regularize=True)
    for name in ('depths', 'probs', 'best_k', 'counts', 'scores', 'reg_scores'):
        _same(getattr(o, name), ref[name], name)
    assert stereo.plane_sweep(desc, cams, pairs, regularize=True).reg_scores is None      # scores were not asked for


def test_estimate_scene_regularised(tmp_path):
    from mvsdf_amd.datasets import prepare
    root, ids, cams_hd, pairs = SC.write_scene(tmp_path / 'scan')
    out = str(tmp_path / 'out')
    sweep = stereo.estimate_scene(root, out, regularize=True)
    assert tuple(sweep.depths.shape) == (5, 64, 96)
    pair, cams, depths, probs = prepare.load_mvs_output(out)
    assert np.array_equal(depths, sweep.depths.cpu().numpy()) and np.array_equal(probs, sweep.probs.cpu().numpy())
    assert prepare.pair_indices(pair) == pairs
    plain = stereo.estimate_scene(root, str(tmp_path / 'plain'))
    assert not torch.equal(plain.best_k, sweep.best_k)
