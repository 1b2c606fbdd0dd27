"""The cascade of mvsdf_amd/stereo.py without a GPU: every argument is refused before the device is touched, the command line, the numpy restatement
tests/stereo_cascade_ref.py against stereo_ref where they must agree, and the accuracy the cascade was built on: on the synthetic scene it loses
nothing on clean images and wins on noisy ones.

The accuracy claim, the share of the pixels a source sees whose depth is off by more than 4 intervals (128 x 192, focal 300, D = 96, stages of
32 x 48, 64 x 96 and 128 x 192 rendered through the scaled cameras, depth numbers 24, 16, 8, scales 4, 2, 1, 2 sources, 5 x 5 patches), as this
restatement measures it on the two views the test runs:

    view                         0         2
    clean, full sweep          0.98 %    1.70 %
    clean, cascade             1.38 %    1.52 %
    noise sigma 12, full      48.38 %   44.11 %
    noise sigma 12, cascade   28.05 %   22.73 %
"""
import importlib.util
import os

import numpy as np
import pytest

import stereo_cascade_ref as CR
import stereo_ref as R
import stereo_scene as SC
from conftest import ROOT

SIZES = [(32, 48), (64, 96), (128, 192)]
NUMS, SCALES = (24, 16, 8), (4, 2, 1)
VIEWS = (0, 2)


def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_' + name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def small():
    cams, pairs = SC.make_cams(3, (8, 12), 20.0, 12)
    rs = np.random.RandomState(0)
    descs = [R.normalize(rs.normal(size=(3, r, s, 3))) for r, s in ((2, 3), (4, 6), (8, 12))]
    return cams, pairs, descs


def test_arguments_are_refused_before_the_gpu_is_touched(small):
    from mvsdf_amd import stereo
    assert stereo.MAX_STAGES == CR.MAX_STAGES == 4 and 64 <= stereo.MAX_D_BAND == CR.MAX_D_BAND and stereo.MAX_D_BAND * 64 * 9 <= 64 * 1024
    assert stereo.CASCADE_DEFAULTS == ((None, 32, 16), (4, 2, 1))
    cams, pairs, descs = small
    ok = dict(depth_nums=(None, 4, 2), interval_scales=(4, 2, 1))
    bad_cams = cams.copy()
    bad_cams[1, 0, 0, 0] = np.nan
    no_depths = cams.copy()
    no_depths[:, 1, 3, 2] = 0
    backwards = cams.copy()
    backwards[:, 1, 3, 1] = -0.1
    for d, c, kw in (
            ([], cams, ok),                                                                  # L outside [1, 4]
            (descs + descs[:2], cams, dict(depth_nums=(None, 4, 2, 2, 2), interval_scales=(4, 2, 1, 1, 1))),
            (descs, cams, dict(depth_nums=(None, 4), interval_scales=(4, 2, 1))),            # tuples of the wrong length
            (descs, cams, dict(depth_nums=(None, 4, 2), interval_scales=(2, 1))),
            (descs[:2], cams, {}),                                                           # (the defaults are for three stages)
            (descs, cams, dict(depth_nums=(None, None, 2), interval_scales=(4, 2, 1))),      # None elsewhere than in D_1
            (descs, cams, dict(depth_nums=(8, 4, None), interval_scales=(4, 2, 1))),
            (descs, cams, dict(depth_nums=(None, 0, 2), interval_scales=(4, 2, 1))),         # D_b outside [1, MAX_D_BAND]
            (descs, cams, dict(depth_nums=(None, 4, stereo.MAX_D_BAND + 1), interval_scales=(4, 2, 1))),
            (descs, cams, dict(depth_nums=(None, 4, 2.5), interval_scales=(4, 2, 1))),
            (descs, cams, dict(depth_nums=(0, 4, 2), interval_scales=(4, 2, 1))),
            (descs, cams, dict(depth_nums=(None, 4, 2), interval_scales=(4, 0, 1))),         # scales
            (descs, cams, dict(depth_nums=(None, 4, 2), interval_scales=(4, -2, 1))),
            (descs, cams, dict(depth_nums=(None, 4, 2), interval_scales=(np.inf, 2, 1))),
            (descs, cams, dict(depth_nums=(None, 4, 2), interval_scales=(4, 2, np.nan))),
            (descs, backwards, ok),                                                          # a step that is not positive
            ([descs[0], descs[1][:2], descs[2]], cams, ok),                                  # V differs between the stages
            ([descs[0], descs[1][:, :1], descs[2]], cams, ok),                               # the sweep's conditions, at a middle stage
            ([descs[0], descs[1][0], descs[2]], cams, ok),
            ([descs[0], np.where(np.arange(3)[None, None, None] == 1, np.nan, descs[1]), descs[2]], cams, ok),
            (descs, bad_cams, ok), (descs, no_depths, ok), (descs, cams[:2], ok),
            (descs, cams, dict(ok, views=[0, 3])), (descs, cams, dict(ok, views=[1, 1])), (descs, cams, dict(ok, num_src=-1)),
            (descs, cams, dict(ok, regularize=(0.8, 0.1)))):
        with pytest.raises(ValueError):
            stereo.cascade_sweep(d, c, pairs, **kw)
    with pytest.raises(ValueError):
        stereo.cascade_sweep(descs, cams, [[1], [0], [5]], **ok)
    with pytest.raises(ValueError):
        CR.cascade(descs, cams, pairs, depth_nums=(None, None, 2))
    # band_sweep
    centres = np.full((3, 8, 12), 3.5)
    inf = centres.copy()
    inf[1, 2, 3] = np.inf
    for c, n, step, kw in ((centres, 0, 0.1, {}), (centres, stereo.MAX_D_BAND + 1, 0.1, {}), (centres, 2.5, 0.1, {}), (centres, 4, 0.0, {}),
                           (centres, 4, -0.1, {}), (centres, 4, np.nan, {}), (centres, 4, np.inf, {}), (centres, 4, [0.1, 0.1], {}),
                           (centres, 4, [0.1, 0.0, 0.1], {}), (centres[:2], 4, 0.1, {}), (centres[:, :7], 4, 0.1, {}), (centres[0], 4, 0.1, {}),
                           (inf, 4, 0.1, {}), (-inf, 4, 0.1, {}), (centres, 4, 0.1, dict(views=[2, 2])), (centres, 4, 0.1, dict(views=[3])),
                           (centres, 4, 0.1, dict(num_src=-1))):
        with pytest.raises(ValueError):
            stereo.band_sweep(descs[2], cams, pairs, c, n, step, **kw)
    with pytest.raises(ValueError):
        stereo.band_sweep(descs[2][:, :1], cams, pairs, centres[:, :1], 4, 0.1)
    with pytest.raises(ValueError):
        CR.band_view(descs[2], cams, pairs, 1, inf[1], 4, 0.1)
    # upsample_depth
    dep, bk = np.ones((3, 4, 6), np.float32), np.zeros((3, 4, 6), np.int32)
    for d, k, size in ((dep, bk[:2], (8, 12)), (dep[0], bk[0], (8, 12)), (dep[:, :1], bk[:, :1], (8, 12)), (dep, bk, (0, 12)), (dep, bk, (8,)), (dep, bk, 8)):
        with pytest.raises(ValueError):
            stereo.upsample_depth(d, k, size)
    # estimate_scene refuses the argument before it reads anything
    for cas in ((None, 4), ((None, 4), (2,)), ((None, None), (2, 1)), ((None, 4), (2, 0)), 3, ((None, 2, 2, 2, 2), (16, 8, 4, 2, 1))):
        with pytest.raises(ValueError):
            stereo.estimate_scene('nowhere', 'nowhere', cascade=cas)
    with pytest.raises(FileNotFoundError):
        stereo.estimate_scene('nowhere', 'nowhere', cascade=True)


def test_command_line(capsys):
    t = _tool('mvs_depth')
    base = '--data_root D --result_dir O --write_result'
    assert t.parse_args(base.split()).cascade_arg is None
    assert t.parse_args((base + ' --model_name model_cas').split()).cascade_arg is None
    assert t.parse_args((base + ' --cascade').split()).cascade_arg == ((None, 32, 16), (4.0, 2.0, 1.0))
    assert t.parse_args((base + ' --cascade auto,16,8').split()).cascade_arg == ((None, 16, 8), (4.0, 2.0, 1.0))
    assert t.parse_args((base + ' --cascade 48,16,8 --cascade_scales 3,1.5,1').split()).cascade_arg == ((48, 16, 8), (3.0, 1.5, 1.0))
    assert t.parse_args((base + ' --cascade 24,8').split()).cascade_arg == ((24, 8), (2.0, 1.0))
    a = t.parse_args((base + ' --cascade --sgm --model_name model_cas').split())
    assert a.cascade_arg == ((None, 32, 16), (4.0, 2.0, 1.0)) and a.regularize == (0.1, 0.8, 8)
    for extra in ('--cascade 16,auto,8', '--cascade a,b,c', '--cascade 16,0,8', '--cascade 16,8 --cascade_scales 4,2,1', '--cascade --cascade_scales 4,0,1',
                  '--cascade --cascade_scales 4,2,nan', '--cascade_scales 4,2,1', '--cascade 1,1,1,1,1'):
        with pytest.raises(SystemExit):
            t.parse_args((base + ' ' + extra).split())
        capsys.readouterr()


def test_one_stage_of_scale_one_is_the_sweep(small):
    cams, pairs, descs = small
    want = R.sweep(descs[2], cams, pairs, 2)
    got = CR.cascade([descs[2]], cams, pairs, 2, None, (None,), (1,))
    for name in ('depths', 'probs', 'best_k', 'counts'):
        assert np.array_equal(got[name], want[name], equal_nan=True) and got[name].dtype == want[name].dtype, name
        assert np.array_equal(got['stages'][0][name], want[name], equal_nan=True), name
    assert (want['best_k'] >= 0).mean() > 0.5


def test_upsample_and_band_by_hand():
    """centres: a constant map stays constant, a pixel whose parents have no winner has none; a band of one hypothesis at the sweep's depth has the
    sweep's score"""
    dep = np.full((1, 3, 4), 3.25, np.float32)
    bk = np.zeros((1, 3, 4), np.int32)
    bk[0, :2, :2] = -1
    c = CR.upsample(dep, bk, (6, 8))
    assert np.isnan(c[0, :3, :3]).all() and np.array_equal(c[0, 4:, :], np.full((2, 8), 3.25)) and not np.isnan(c[0, 3:, 3:]).any()
    cams, pairs = SC.make_cams(3, (8, 12), 20.0, 5)
    desc = R.normalize(np.random.RandomState(1).normal(size=(3, 8, 12, 4)))
    full = R.sweep_view(desc, cams, pairs, 1, 2)
    k = 2
    o = CR.band_view(desc, cams, pairs, 1, np.full((8, 12), cams[1, 1, 3, 0] + k * cams[1, 1, 3, 1]), 1, 0.5, 2)
    assert np.array_equal(o['scores'][0], full['scores'][k], equal_nan=True) and np.array_equal(o['n'][0], full['n'][k])
    assert set(np.unique(o['best_k'])) <= {-1, 0}
    low = CR.band_view(desc, cams, pairs, 1, np.full((8, 12), 0.05), 4, 0.05, 2)           # d = -0.05, 0, 0.05, 0.1: the first two are invalid
    assert np.isnan(low['scores'][:2]).all() and (low['n'][:2] == 0).all()
    none = CR.band_view(desc, cams, pairs, 1, np.full((8, 12), np.nan), 4, 0.05, 2)
    assert (none['best_k'] == -1).all() and not none['depth'].any() and not none['probs'].any() and not none['counts'].any()


@pytest.fixture(scope='module')
def claim():
    """-> {(noisy, view): (share of the full sweep, share of the cascade)} in percent"""
    cams, pairs = SC.make_cams(5, SIZES[-1], 300.0, 96)
    stage_cams = [CR.scale_cams(cams, s / SIZES[-1][1], r / SIZES[-1][0]) for r, s in SIZES]
    images = [SC.render(c, hw)[0] for c, hw in zip(stage_cams, SIZES)]
    gt = SC.render(cams, SIZES[-1])[1]
    seen = SC.seen_by_a_source(cams, gt, pairs, 2)
    rs = np.random.RandomState(5)
    noisy = [np.clip(np.rint(im + rs.normal(0, 12, im.shape)), 0, 255).astype(np.uint8) for im in images]         # coarse, middle, fine: in this order
    interval = cams[0, 1, 3, 1]
    out = {}
    for tag, stack in ((False, images), (True, noisy)):
        descs = [R.normalize(R.patches(im, 2)) for im in stack]
        for v in VIEWS:
            full = R.sweep_view(descs[-1], cams, pairs, v, 2)['depth']
            cas = CR.cascade(descs, cams, pairs, 2, [v], NUMS, SCALES)['depths'][v]
            out[tag, v] = tuple(100.0 * float((np.abs(d - gt[v])[seen[v]] > 4 * interval).mean()) for d in (full, cas))
    return out


@pytest.mark.parametrize('view', VIEWS)
def test_clean_scene_the_cascade_loses_at_most_a_point(claim, view):
    full, cas = claim[False, view]
    print('clean, view %d: full sweep %.2f %%, cascade %.2f %%' % (view, full, cas))
    assert cas <= full + 1.0, (full, cas)


@pytest.mark.parametrize('view', VIEWS)
def test_noisy_scene_the_cascade_wins(claim, view):
    full, cas = claim[True, view]
    print('noise sigma 12, view %d: full sweep %.2f %%, cascade %.2f %%, ratio %.2f' % (view, full, cas, cas / full))
    assert full > 40.0, full                                                                  # the condition on the input
    assert cas <= 0.7 * full, (full, cas)
