"""The plane-sweep definition (mvsdf_amd/stereo.py) through its numpy restatement tests/stereo_ref.py: held to the known depth of the synthetic scene
of tests/stereo_scene.py and to closed-form cases, plus the host side of mvsdf_amd/stereo.py (argument checks, camera files, the command line).
The device result is held to the same restatement bit for bit in tests/test_gpu_stereo.py."""
import importlib.util
import os

import numpy as np
import pytest

import mvs_scene as MS
import stereo_ref as R
import stereo_scene as SC
from conftest import ROOT

HW = (64, 96)


@pytest.fixture(scope='module')
def scene():
    cams, pairs = SC.make_cams(5, HW)
    images, gt = SC.render(cams, HW)
    desc = R.normalize(R.patches(images, 2))
    return cams, pairs, gt, desc, R.sweep(desc, cams, pairs, 2)


def test_kept_pixels_of_the_scene_are_within_half_an_interval(scene):
    """A correct winner before refinement is within half a depth interval of the truth, so that is the bound on the median error of the pixels the
    recorded thresholds keep; and those thresholds must keep at least half of the pixels that a source sees (a condition on the scene)."""
    from mvsdf_amd.stereo import PTHRESH
    cams, pairs, gt, desc, o = scene
    p = o['probs']
    keep = (p[:, 0] > np.float32(PTHRESH[0])) & (p[:, 1] > np.float32(PTHRESH[1])) & (p[:, 2] > np.float32(PTHRESH[2])) & (o['depths'] > 0)
    seen = SC.seen_by_a_source(cams, gt, pairs, 2)
    interval = cams[0, 1, 3, 1]
    err = np.abs(o['depths'].astype(np.float64) - gt)
    med = np.median(err[keep]) / interval
    print('kept %d of %d seen pixels (%.3f), median |error| = %.3f intervals' % (keep.sum(), seen.sum(), keep.sum() / seen.sum(), med))
    assert 2 * keep.sum() >= seen.sum()
    assert med <= 0.5
    assert (p >= 0).all() and (p <= 1).all()


def _unit_sign_descriptors(shape, seed=0):
    """C = 4 descriptors with entries +-1: the norm is 2, the unit descriptor +-0.5 and its product with itself exactly 1"""
    return np.random.RandomState(seed).choice([-1.0, 1.0], size=shape + (4,)).astype(np.float32)


def test_identical_source_scores_exactly_one_and_the_lowest_k_wins():
    cams, depths, pairs = MS.exact_self_pair()
    cams = cams.copy()
    cams[:, 1, 3] = [1.0, 0.5, 8, 4.5]
    f = _unit_sign_descriptors((1, 16, 32))
    desc = R.normalize(np.concatenate([f, f]))
    assert np.array_equal(np.abs(desc), np.full(desc.shape, 0.5, np.float32))
    o = R.sweep_view(desc, cams, pairs, 0, 2)
    assert (o['n'] == 1).all() and np.array_equal(o['scores'], np.ones((8, 16, 32)))
    assert (o['best_k'] == 0).all() and np.array_equal(o['depth'], np.full((16, 32), 1.0, np.float32))
    assert np.array_equal(o['probs'][0], np.ones((16, 32), np.float32)) and (o['probs'][1] == 0).all() and (o['probs'][2] == 1).all()


@pytest.mark.parametrize('D', [1, 2])
def test_one_and_two_hypotheses_never_refine(D):
    cams, pairs = SC.make_cams(3, (20, 28), focal=45.0, n_depths=D)
    images, _ = SC.render(cams, (20, 28))
    desc = R.normalize(R.patches(images, 1))
    for r in range(3):
        o = R.sweep_view(desc, cams, pairs, r, 2)
        has = o['best_k'] >= 0
        assert has.any() and (o['off'] == 0).all()
        want = (cams[r, 1, 3, 0] + o['best_k'] * cams[r, 1, 3, 1]).astype(np.float32)
        assert np.array_equal(o['depth'][has], want[has]) and (o['depth'][~has] == 0).all()
        b = o['scores'][np.maximum(o['best_k'], 0), np.arange(20)[:, None], np.arange(28)[None]]
        assert (o['probs'][1][has & (b > 0)] == 1).all()                       # no k two steps away


def test_zero_norm_descriptor_scores_zero():
    cams, pairs = SC.make_cams(3, (20, 28), focal=45.0, n_depths=6)
    images, _ = SC.render(cams, (20, 28))
    raw = R.patches(images, 1)
    raw[1, 7, 9] = 0
    desc = R.normalize(raw)
    assert (desc[1, 7, 9] == 0).all()
    o = R.sweep_view(desc, cams, pairs, 1, 2)
    valid = o['n'][:, 7, 9] >= 1
    assert valid.any() and (o['scores'][valid, 7, 9] == 0).all()
    assert o['best_k'][7, 9] == np.argmax(valid) and o['probs'][0, 7, 9] == 0 and o['probs'][1, 7, 9] == 0 and o['probs'][2, 7, 9] > 0


def test_empty_pair_list_and_unswept_views_give_zeros(scene):
    cams, pairs, gt, desc, _ = scene
    o = R.sweep(desc, cams, [[] for _ in pairs], 2, views=[0])
    assert np.isnan(o['scores']).all()
    o2 = R.sweep(desc, cams, pairs, 0, views=[0])                             # num_src = 0 uses no source either
    for out in (o, o2):
        assert (out['depths'] == 0).all() and (out['probs'] == 0).all() and (out['best_k'] == -1).all() and (out['counts'] == 0).all()


def test_num_src_cuts_the_pair_list(scene):
    cams, pairs, gt, desc, full = scene
    a = R.sweep_view(desc, cams, pairs, 2, 1)
    b = R.sweep_view(desc, cams, [p[:1] for p in pairs], 2, 7)
    assert a['n'].max() == 1 and np.array_equal(a['depth'], b['depth']) and np.array_equal(a['probs'], b['probs'])
    c = R.sweep_view(desc, cams, pairs, 2, 2)
    assert np.array_equal(c['depth'], full['depths'][2]) and c['n'].max() == 2


def test_arguments_are_refused_before_anything_is_launched(scene):
    from mvsdf_amd import stereo
    cams, pairs, gt, desc, _ = scene
    desc = desc[:, :8, :8]
    nan_cam, inf_cam, no_d = cams.copy(), cams.copy(), cams.copy()
    nan_cam[1, 0, 2, 3] = np.nan
    inf_cam[3, 1, 0, 0] = np.inf
    no_d[2, 1, 3, 2] = 0
    nan_f, inf_f = desc.copy(), desc.copy()
    nan_f[4, 3, 2, 1] = np.nan
    inf_f[0, 0, 0, 0] = -np.inf
    bad_pairs = [list(p) for p in pairs]
    bad_pairs[3][0] = 5
    neg_pairs = [list(p) for p in pairs]
    neg_pairs[0][1] = -1
    for args, kw in (((desc, nan_cam, pairs), {}), ((desc, inf_cam, pairs), {}), ((desc, no_d, pairs), {}), ((nan_f, cams, pairs), {}),
                     ((inf_f, cams, pairs), {}), ((desc, cams, bad_pairs), {}), ((desc, cams, neg_pairs), {}), ((desc[:, :1], cams, pairs), {}),
                     ((desc[:, :, :1], cams, pairs), {}), ((desc[0], cams, pairs), {}), ((desc, cams[:4], pairs), {}), ((desc, cams, pairs[:4]), {}),
                     ((desc, cams, pairs), dict(views=[5])), ((desc, cams, pairs), dict(num_src=-1))):
        with pytest.raises(ValueError):
            stereo.plane_sweep(*args, **kw)
    for f in (nan_f, inf_f, desc[:, :1], desc[0]):
        with pytest.raises(ValueError):
            stereo.normalize_descriptors(f)
    for img, kw in ((np.zeros((2, 8, 8, 3), np.float32), {}), (np.zeros((2, 8, 8), np.uint8), {}), (np.zeros((2, 8, 8, 3), np.uint8), dict(radius=-1)),
                    (np.zeros((2, 8, 8, 3), np.uint8), dict(radius=16))):
        with pytest.raises(ValueError):
            stereo.patch_descriptors(img, **kw)


def test_camera_file_round_trip(tmp_path):
    from mvsdf_amd import stereo
    from mvsdf_amd.utils import io as sio
    cams, _ = SC.make_cams(2, HW)
    path = str(tmp_path / 'cam.txt')
    stereo._write_cam(path, cams[1])
    assert np.array_equal(sio.load_cam(path, 256, 1), cams[1])
    back = sio.load_cam(path, 256, 1, override=True)                         # how prepare.load_mvs_output reads it
    assert np.array_equal(back[0], cams[1, 0]) and np.array_equal(back[1, :3, :3], cams[1, 1, :3, :3]) and back[1, 3, 3] == cams[1, 1, 3, 3]


def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_' + name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_command_line(capsys):
    t = _tool('mvs_depth')
    a = t.parse_args('--data_root D --dataset_name general --model_name model_cas --num_src 2 --max_d 256 --interval_scale 1 --resize 768,576 '
                     '--crop 768,576 --write_result --result_dir O'.split())
    assert (a.data_root, a.result_dir, a.num_src, a.max_d, a.interval_scale, a.resize, a.crop, a.load_path, a.descriptor) == \
        ('D', 'O', 2, 256, 1.0, '768,576', '768,576', None, 'patch')
    for argv, word in (('--data_root D --result_dir O', 'write_result'), ('--data_root D --result_dir O --write_result --dataset_name dtu', 'general')):
        with pytest.raises(SystemExit):
            t.parse_args(argv.split())
        assert word in capsys.readouterr().err
