"""The regularisation of the plane sweep (mvsdf_amd/stereo.py: "Regularisation") through its numpy restatement tests/stereo_sgm_ref.py: closed forms,
a scalar walk along every path, the gain on the noisy synthetic scene that the defaults were chosen on, and the host side (argument checks, the
command line).  The device result is held to the same restatement bit for bit in tests/test_gpu_stereo_sgm.py."""
import importlib.util
import os

import numpy as np
import pytest

import stereo_ref as R
import stereo_scene as SC
import stereo_sgm_ref as G
from conftest import ROOT

HW = (64, 96)
noisy_images = G.noisy_images                                             # seed 5, sigma 12 grey levels


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def _grid_volume(shape, seed, nan_share=0.15):
    """scores on a 2^-10 grid in [-1, 1]: 1 - s, sums of eight of them and their division by 8 are all exact"""
    rs = np.random.RandomState(seed)
    v = rs.randint(-1024, 1025, size=shape).astype(np.float64) / 1024.0
    v[rs.uniform(size=shape) < nan_share] = np.nan
    return v


@pytest.mark.parametrize('paths', [4, 8])
def test_zero_penalties_return_the_input(paths):
    """P1 = P2 = 0: best = m, so L = C in every direction, T = paths * C and A = 1 - C = the score, exactly on the grid"""
    v = _grid_volume((7, 9, 11), 0)
    v[:, 3, 4] = np.nan                                                       # a pixel without a valid hypothesis
    assert _same(G.regularize(v, 0.0, 0.0, paths), v)


def _predecessors_inside(y, x, hw, paths):
    return [0 <= y - dy < hw[0] and 0 <= x - dx < hw[1] for dy, dx in G.DIRECTIONS[:paths]]


@pytest.mark.parametrize('p1,p2,paths', [(0.25, 0.5, 8), (0.25, 0.5, 4), (0.1, 0.8, 8), (0.3, 0.3, 8), (0.0, 1.0, 8)])
def test_one_hot_volume_closed_form(p1, p2, paths):
    """score 1 at k0 and 0 elsewhere, at every pixel: C is 0 at k0 and 1 elsewhere, so m = 0 on every path and L(k0) = 0.  At the first pixel of a path
    L(k) = 1; from the second on L(k) = 1 + min(L_q(k), L_q(k-1) + P1, L_q(k+1) + P1, P2) with L_q(k0) = 0 and L_q >= 1 elsewhere, so with
    P1 <= P2 <= 1 it is 1 + P1 one step from k0 (the term L_q(k0) + P1) and 1 + P2 further away (every other term is >= 1).  T sums these in
    direction order; A = 1 - T / paths."""
    D, hw, k0 = 7, (5, 6), 2
    v = np.zeros((D,) + hw)
    v[k0] = 1.0
    A = G.regularize(v, p1, p2, paths)
    for y in range(hw[0]):
        for x in range(hw[1]):
            inside = _predecessors_inside(y, x, hw, paths)
            for k in range(D):
                pen = 0.0 if k == k0 else p1 if abs(k - k0) == 1 else p2
                terms = [0.0 if k == k0 else (1.0 + (pen - 0.0) if q else 1.0) for q in inside]
                T = terms[0]
                for t in terms[1:]:
                    T = T + t
                assert A[k, y, x] == 1.0 - T / paths, (k, y, x)
    assert (A[k0] == 1.0).all()
    if (p1, p2) == (0.25, 0.5):
        assert (A[[1, 3], 1:-1, 1:-1] == -0.25).all() and (A[[0, 4, 5, 6], 1:-1, 1:-1] == -0.5).all()


def test_a_single_valid_pixel_returns_its_own_scores():
    v = np.full((6, 5, 7), np.nan)
    v[:, 2, 3] = _grid_volume((6,), 1, 0.0)
    v[4, 2, 3] = np.nan
    for paths in (4, 8):
        assert _same(G.regularize(v, 0.1, 0.8, paths), v)


def test_an_all_invalid_volume_stays_invalid():
    v = np.full((4, 3, 5), np.nan)
    A = G.regularize(v)
    assert np.isnan(A).all()
    o = G.pick(A, v, np.zeros(v.shape, np.int64), 2.0, 0.1, 2)
    assert (o['best_k'] == -1).all() and (o['depth'] == 0).all() and (o['probs'] == 0).all() and (o['counts'] == 0).all()


def test_four_paths_are_the_first_four_directions():
    """paths = 4 is ((L_1 + L_2) + L_3) + L_4 of the horizontal and vertical directions: the value at a pixel depends on its row and its column alone,
    while eight paths also see the diagonals"""
    assert G.DIRECTIONS[:4] == [(0, 1), (0, -1), (1, 0), (-1, 0)]
    v = _grid_volume((5, 7, 8), 2)
    L = [G.path_costs(v, 0.125, 0.5, d) for d in G.DIRECTIONS]
    want4 = 1.0 - (((L[0] + L[1]) + L[2]) + L[3]) / 4.0
    want8 = 1.0 - (((((((L[0] + L[1]) + L[2]) + L[3]) + L[4]) + L[5]) + L[6]) + L[7]) / 8.0
    assert _same(G.regularize(v, 0.125, 0.5, 4), want4) and _same(G.regularize(v, 0.125, 0.5, 8), want8)
    w = v.copy()
    w[:, 2, 2] = _grid_volume((5,), 3, 0.0)                                   # diagonal neighbour of (3, 3), neither in its row nor in its column
    a4, b4 = G.regularize(v, 0.125, 0.5, 4), G.regularize(w, 0.125, 0.5, 4)
    a8, b8 = G.regularize(v, 0.125, 0.5, 8), G.regularize(w, 0.125, 0.5, 8)
    assert _same(a4[:, 3, 3], b4[:, 3, 3]) and not _same(a8[:, 3, 3], b8[:, 3, 3])


def _walk(score, p1, p2, paths):
    """the definition pixel by pixel in Python scalars: every path from its first pixel on"""
    D, Rr, S = score.shape
    T = None
    for dy, dx in G.DIRECTIONS[:paths]:
        L = np.full(score.shape, np.nan)
        ys = range(Rr) if dy >= 0 else range(Rr - 1, -1, -1)
        xs = range(S) if dx >= 0 else range(S - 1, -1, -1)
        for y in ys:
            for x in xs:
                qy, qx = y - dy, x - dx
                prev = [L[j, qy, qx] for j in range(D)] if 0 <= qy < Rr and 0 <= qx < S else []
                alive = [p for p in prev if not np.isnan(p)]
                for k in range(D):
                    if np.isnan(score[k, y, x]):
                        continue
                    c = 1.0 - score[k, y, x]
                    if not alive:
                        L[k, y, x] = c
                        continue
                    m = min(alive)
                    terms = [m + p2]
                    if not np.isnan(prev[k]):
                        terms.append(prev[k])
                    if k > 0 and not np.isnan(prev[k - 1]):
                        terms.append(prev[k - 1] + p1)
                    if k < D - 1 and not np.isnan(prev[k + 1]):
                        terms.append(prev[k + 1] + p1)
                    L[k, y, x] = c + (min(terms) - m)
        T = L if T is None else T + L
    return 1.0 - T / paths


@pytest.mark.parametrize('shape,p1,p2,paths', [((1, 2, 2), 0.1, 0.8, 8), ((2, 3, 5), 0.3, 0.3, 8), ((4, 5, 4), 0.1, 0.8, 4), ((5, 4, 6), 0.1, 0.8, 8)])
def test_the_restatement_is_the_scalar_walk(shape, p1, p2, paths):
    rs = np.random.RandomState(shape[0])
    v = rs.uniform(-1, 1, size=shape)
    v[rs.uniform(size=shape) < 0.2] = np.nan
    v[:, 1, 1] = np.nan
    assert _same(G.regularize(v, p1, p2, paths), _walk(v, p1, p2, paths))


def _beyond_one_interval(depth, gt, seen, interval):
    return float((np.abs(depth.astype(np.float64) - gt)[seen] > interval).mean())


@pytest.fixture(scope='module')
def scene():
    cams, pairs = SC.make_cams(5, HW)
    images, gt = SC.render(cams, HW)
    return cams, pairs, gt, images, SC.seen_by_a_source(cams, gt, pairs, 2)


def test_the_defaults_halve_the_outliers_of_the_noisy_scene(scene):
    """Gaussian noise of sigma 12 grey levels on the images (seed 5): winner-take-all must leave more than 10 % of the seen pixels of every view beyond
    one depth interval (the condition on the input), and the regularised sweep with the defaults at most half of that share, on every view."""
    cams, pairs, gt, images, seen = scene
    desc = R.normalize(R.patches(noisy_images(images), 2))
    interval = cams[0, 1, 3, 1]
    shares = []
    for r in range(5):
        raw = R.sweep_view(desc, cams, pairs, r, 2)
        reg = G.sweep_view(desc, cams, pairs, r, 2)
        shares.append((_beyond_one_interval(raw['depth'], gt[r], seen[r], interval), _beyond_one_interval(reg['depth'], gt[r], seen[r], interval)))
        print('view %d: beyond one interval %.4f winner-take-all, %.4f regularised' % (r, shares[-1][0], shares[-1][1]))
        assert np.array_equal(reg['counts'][reg['best_k'] >= 0], raw['n'][reg['best_k'], np.arange(HW[0])[:, None], np.arange(HW[1])[None]][reg['best_k'] >= 0])
    for wta, reg in shares:
        assert wta > 0.10
    for wta, reg in shares:
        assert reg <= 0.5 * wta


def test_the_defaults_do_no_harm_on_the_clean_scene(scene):
    cams, pairs, gt, images, seen = scene
    desc = R.normalize(R.patches(images, 2))
    interval = cams[0, 1, 3, 1]
    for r in range(5):
        wta = 1 - _beyond_one_interval(R.sweep_view(desc, cams, pairs, r, 2)['depth'], gt[r], seen[r], interval)
        reg = 1 - _beyond_one_interval(G.sweep_view(desc, cams, pairs, r, 2)['depth'], gt[r], seen[r], interval)
        print('view %d: within one interval %.4f winner-take-all, %.4f regularised' % (r, wta, reg))
        assert reg >= wta


def test_prob1_is_the_raw_score_at_the_new_winner(scene):
    cams, pairs, gt, images, seen = scene
    desc = R.normalize(R.patches(noisy_images(images), 2))[:, :20, :30]
    o = G.sweep_view(desc, cams, pairs, 1, 2)
    has = o['best_k'] >= 0
    yy, xx = np.nonzero(has)
    raw = o['scores'][o['best_k'][has], yy, xx]
    assert np.array_equal(o['probs'][0][has], np.clip(raw, 0, 1).astype(np.float32))
    assert (o['best_k'] != R.sweep_view(desc, cams, pairs, 1, 2)['best_k']).any()


def test_arguments_are_refused_before_anything_is_launched(scene):
    from mvsdf_amd import stereo
    assert stereo.MAX_D_SGM == 4096 and stereo.SGM_DEFAULTS == G.DEFAULTS
    v = np.zeros((3, 4, 5))
    for kw in (dict(p1=-0.1), dict(p1=np.nan), dict(p2=np.inf), dict(p1=np.inf, p2=np.inf), dict(p1=0.9, p2=0.8), dict(paths=5), dict(paths=0)):
        with pytest.raises(ValueError):
            stereo.regularize_scores(v, **kw)
        with pytest.raises(ValueError):
            G.regularize(v, **kw)
    inf = v.copy()
    inf[1, 2, 3] = np.inf
    for bad in (np.zeros((stereo.MAX_D_SGM + 1, 1, 1)), np.zeros((4, 5)), np.zeros((2, 3, 4, 5)), np.zeros((3, 0, 5)), np.zeros((3, 4, 0)),
                np.zeros((0, 4, 5)), inf):
        with pytest.raises(ValueError):
            stereo.regularize_scores(bad)
    cams, pairs, gt, images, seen = scene
    desc = R.normalize(R.patches(images, 2))[:, :8, :8]
    deep = cams.copy()
    deep[:, 1, 3, 2] = stereo.MAX_D_SGM + 1
    for c, reg in ((cams, (0.1,)), (cams, (0.1, 0.8, 8, 1)), (cams, (0.8, 0.1)), (cams, (-1.0, 0.5)), (cams, (0.1, np.nan)), (cams, (0.1, 0.8, 5)),
                   (cams, 'yes'), (cams, 3), (deep, True)):
        with pytest.raises(ValueError):
            stereo.plane_sweep(desc, c, pairs, regularize=reg)
    with pytest.raises(ValueError):
        stereo.estimate_scene('nowhere', 'nowhere', regularize=(0.5, 0.1))


def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_' + name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_command_line(capsys):
    t = _tool('mvs_depth')
    base = '--data_root D --result_dir O --write_result'
    assert t.parse_args(base.split()).regularize is None
    assert t.parse_args((base + ' --sgm').split()).regularize == (0.1, 0.8, 8)
    assert t.parse_args((base + ' --sgm --sgm_paths 4').split()).regularize == (0.1, 0.8, 4)
    assert t.parse_args((base + ' --sgm .05,.4 --sgm_paths 8').split()).regularize == (0.05, 0.4, 8)
    assert t.parse_args((base + ' --sgm_paths 4').split()).regularize is None
    for extra in ('--sgm .5', '--sgm .5,.1', '--sgm a,b', '--sgm -1,2', '--sgm --sgm_paths 5', '--sgm .1,nan'):
        with pytest.raises(SystemExit):
            t.parse_args((base + ' ' + extra).split())
        capsys.readouterr()
