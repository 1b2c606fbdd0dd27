"""View selection without a GPU: the host entry point of csrc/det_math64.h + viewsel.hip against the numpy restatement bit for bit, the accuracy
condition against libm, the pair ordering, the depth-range index rule, the COLMAP readers and the pair.txt writer."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import colmap_scene as CS                                                   # noqa: E402
import viewsel_ref as R                                                     # noqa: E402
from mvsdf_amd import build, viewsel                                        # noqa: E402
from mvsdf_amd.datasets import colmap                                       # noqa: E402
from mvsdf_amd.utils import io as sio                                       # noqa: E402


def _vectors():
    rng = np.random.RandomState(0)
    a = rng.randn(100000, 3) * np.exp(rng.uniform(-3, 3, (100000, 1)))
    b = rng.randn(100000, 3) * np.exp(rng.uniform(-3, 3, (100000, 1)))
    b[:40000] = a[:40000] * rng.uniform(0.5, 2, (40000, 1)) + 0.1 * rng.randn(40000, 3) * np.linalg.norm(a[:40000], axis=1, keepdims=True)
    e = rng.randn(16, 3)
    edges_a = [e[0], e[1], np.zeros(3), e[2], np.zeros(3), e[3] * 1e-100, e[4] * 1e100, e[5] * 1e-200, e[6] * 1e200, e[7] * 1e-100, [1, 0, 0], [1, 0, 0],
               [0, 0, 2], [3, 0, 0]]
    edges_b = [e[0], -e[1], e[2], np.zeros(3), np.zeros(3), e[8] * 1e-100, e[9] * 1e100, e[10] * 1e-200, e[11] * 1e200, e[12] * 1e100, [0, 1, 0], [1, 1, 0],
               [0, 0, -5], [3e-9, 3, 0]]
    return np.concatenate([a, np.array(edges_a, dtype=np.float64)]), np.concatenate([b, np.array(edges_b, dtype=np.float64)])


def test_library_is_compiled_without_contraction():
    assert '-ffp-contract=off' in build.FLAGS and 'viewsel.hip' in build.SOURCES


@pytest.mark.parametrize('theta0,s1,s2', [(5.0, 1.0, 10.0), (10.0, 2.5, 4.0)])
def test_host_entry_equals_restatement(theta0, s1, s2):
    a, b = _vectors()
    th, wq = viewsel.weights_host(a, b, theta0, s1, s2)
    th_r, wq_r = R.theta_wq(a, b, theta0, s1, s2)
    assert np.array_equal(th.view(np.uint64), th_r.view(np.uint64)), 'theta differs in %d places' % (th != th_r).sum()
    assert np.array_equal(wq, wq_r)
    assert (wq > 0).sum() > 20000 and 0 <= wq.min() and wq.max() <= 2 ** 32
    n = len(a) - 14
    assert th[n] == 0 and th[n + 1] == 180                                 # a = b, a = -b
    assert (th[n + 2:n + 5] == 0).all()                                     # a zero vector: atan2(0, 0) = 0
    assert (th[n + 5:n + 7] > 0).all() and (th[n + 7:n + 9] == 0).all()     # 1e+-100 is in range, the squares of 1e+-200 are not: coincident by definition
    assert th[n + 10] == 90 and th[n + 11] == 45 and th[n + 12] == 180


def test_theta_exactly_at_theta0_takes_sigma1():
    a, b = np.array([[1.0, 0.2, -0.3]]), np.array([[0.9, 0.35, -0.2]])
    t0 = float(R.theta_wq(a, b)[0][0])                                      # the angle these vectors make, then used as theta0: d = 0 exactly
    for s1, s2 in ((1.0, 10.0), (10.0, 1.0)):
        th, wq = viewsel.weights_host(a, b, t0, s1, s2)
        assert th[0] == t0 and wq[0] == 2 ** 32
    eps = np.spacing(t0)
    above, below = viewsel.weights_host(a, b, t0 - 1e6 * eps, 1e-6, 1.0)[1][0], viewsel.weights_host(a, b, t0 + 1e6 * eps, 1e-6, 1.0)[1][0]
    assert above == R.theta_wq(a, b, t0 - 1e6 * eps, 1e-6, 1.0)[1][0] and below == R.theta_wq(a, b, t0 + 1e6 * eps, 1e-6, 1.0)[1][0]
    assert above > below                                                   # theta > theta0 falls off with sigma2 = 1, theta < theta0 with sigma1 = 1e-6


def test_accuracy_condition_against_libm():
    """|w_written - w_libm| <= 2^-33 on a dense theta grid over [0, 180] for both sigmas, theta itself included (vectors at that angle)."""
    t = np.linspace(0.0, 180.0, 1800001)
    worst = 0.0
    for s in (1.0, 10.0):
        d = np.abs(R.weight(t, 5.0, s, s) - R.weight_libm(t, 5.0, s, s)).max()
        print('max |w - w_libm| on the theta grid, sigma %g: %.3e = %.3e quanta' % (s, d, d * 2.0 ** 32))
        worst = max(worst, d)
    rad = np.radians(t[::9])
    a = np.tile([0.3, -0.4, 1.2], (len(rad), 1))
    e1, e2 = np.array([0.6, 0.8, 0.05]), np.cross([0.3, -0.4, 1.2], [0.6, 0.8, 0.05])
    e1 = e1 - a[0] * (e1 @ a[0]) / (a[0] @ a[0])
    b = 0.7 * (np.cos(rad)[:, None] * a / np.linalg.norm(a[0]) + np.sin(rad)[:, None] * e1 / np.linalg.norm(e1)) + 0 * e2
    th, wq = viewsel.weights_host(a, b)
    th_l, w_l = R.theta_w_libm(a, b)
    dt = np.abs(th - th_l).max()
    dw = np.abs(R.weight(th) - w_l).max()
    print('max |theta - theta_libm| from vectors: %.3e degrees; max |w - w_libm| from vectors: %.3e = %.3e quanta' % (dt, dw, dw * 2.0 ** 32))
    worst = max(worst, dw)
    assert worst <= 2.0 ** -33
    assert np.abs(wq - np.rint(w_l * 2.0 ** 32).astype(np.int64)).max() <= 1


def test_select_pairs_orders_by_score_then_index_and_skips_pairs_without_points():
    scores = np.array([[0.0, 2.0, 2.0, 5.0, 0.0],
                       [2.0, 0.0, 1.0, 1.0, 1.0],
                       [2.0, 1.0, 0.0, 0.0, 0.0],
                       [5.0, 1.0, 0.0, 0.0, 0.0],
                       [0.0, 1.0, 0.0, 0.0, 0.0]])
    counts = (scores > 0).astype(np.int64) + np.eye(5, dtype=np.int64) * 7
    counts[2, 3] = counts[3, 2] = 4                                         # common points whose weights all quantise to 0: still a pair
    pairs, ps = viewsel.select_pairs(scores, counts, 10)
    assert pairs == [[3, 1, 2], [0, 2, 3, 4], [0, 1, 3], [0, 1, 2], [1]]
    assert ps[0] == [5.0, 2.0, 2.0] and ps[2] == [2.0, 1.0, 0.0]
    assert viewsel.select_pairs(scores, counts, 2)[0] == [[3, 1], [0, 2], [0, 1], [0, 1], [1]]
    assert viewsel.select_pairs(torch.from_numpy(scores), torch.from_numpy(counts), 10)[0] == pairs
    assert (pairs, ps) == R.select_pairs(scores, counts, 10)
    empty = viewsel.select_pairs(np.zeros((3, 3)), np.zeros((3, 3), np.int64), 10)
    assert empty == ([[], [], []], [[], [], []])


@pytest.mark.parametrize('n', [1, 2, 100, 101])
def test_depth_range_index_rule(n):
    for q in (0.01, 0.99, 0.0, 0.5):
        assert int(viewsel._quantile_index(torch.tensor([n]), q)[0]) == int(n * q) < n
    z = np.arange(n, dtype=np.float64)[::-1]
    E = np.eye(4)[None]
    pts = np.stack([0 * z, 0 * z, z], 1)
    assert R.depth_ranges(pts, np.ones((1, n), bool), E).tolist() == [[float(int(n * 0.01)), float(int(n * 0.99))]]


@pytest.mark.parametrize('kind', ['text', 'binary'])
@pytest.mark.parametrize('model', ['PINHOLE', 'SIMPLE_PINHOLE', 'SIMPLE_RADIAL', 'OPENCV'])
def test_colmap_round_trip(tmp_path, kind, model):
    scene = CS.make_scene(model=model, blind_image=True, double_observation=True)
    assert len(scene['images'][2]['point3D_ids']) == 0                     # the image with an empty POINTS2D line
    pts = scene['points']
    assert pts['track_image'][0] == pts['track_image'][pts['track_off'][1] - 1]          # the point observed twice in one image
    (CS.write_text if kind == 'text' else CS.write_binary)(scene, str(tmp_path))
    back = colmap.load_colmap_model(str(tmp_path))
    CS.assert_models_equal(scene, back)
    ids, names, cams, view = colmap.model_views(back)
    assert ids == sorted(scene['images']) and ids[0] == 2 and names[0] == 'blind.png'
    assert view.dtype == np.int32 and view.min() >= 1 and view.max() == len(ids) - 1      # view 0 is the blind image
    assert np.allclose(cams[:, 1, :3, :3], [[CS.FOCAL, 0, CS.W / 2], [0, CS.FOCAL, CS.H / 2], [0, 0, 1]])
    E = CS.scene_arrays(scene)[2]
    assert np.array_equal(cams[:, 0], E)


def test_text_and_binary_models_are_identical(tmp_path):
    scene = CS.make_scene(blind_image=True, double_observation=True)
    CS.write_text(scene, str(tmp_path / 't'))
    CS.write_binary(scene, str(tmp_path / 'b'))
    CS.assert_models_equal(colmap.load_colmap_model(str(tmp_path / 't')), colmap.load_colmap_model(str(tmp_path / 'b')))


@pytest.mark.parametrize('kind', ['text', 'binary'])
def test_colmap_refuses_distortion_and_unknown_models(tmp_path, kind):
    write = CS.write_text if kind == 'text' else CS.write_binary
    write(CS.make_scene(model='SIMPLE_RADIAL', distortion=0.01), str(tmp_path / 'a'))
    with pytest.raises(ValueError, match='undistort'):
        colmap.load_colmap_model(str(tmp_path / 'a'))
    scene = CS.make_scene()
    scene['cameras'][1]['model'] = 'OPENCV_FISHEYE'
    scene['cameras'][1]['params'] = np.array([CS.FOCAL, CS.FOCAL, CS.W / 2, CS.H / 2, 0, 0, 0, 0], dtype=np.float64)
    write(scene, str(tmp_path / 'b'))
    with pytest.raises(ValueError, match='undistort'):
        colmap.load_colmap_model(str(tmp_path / 'b'))


def test_colmap_unknown_model_name_and_missing_files(tmp_path):
    scene = CS.make_scene()
    CS.write_text(scene, str(tmp_path))
    path = tmp_path / 'cameras.txt'
    path.write_text(path.read_text().replace('PINHOLE', 'MY_LENS'))
    with pytest.raises(ValueError, match='MY_LENS'):
        colmap.load_colmap_model(str(tmp_path))
    with pytest.raises(FileNotFoundError):
        colmap.load_colmap_model(str(tmp_path / 'nowhere'))
    with pytest.raises(ValueError, match='max_d'):
        colmap.colmap_to_mvs(str(tmp_path), str(tmp_path), str(tmp_path / 'out'), max_d=0)


def test_write_pair_round_trip(tmp_path):
    pairs = [[2, 1], [0], [], [0, 1, 2]]
    scores = [[3.25, 0.1], [1.0 / 3.0], [], [2.0 ** -32, 7e10, 0.0]]
    ids = ['0', '1', '2', '3']
    viewsel.write_pair(str(tmp_path / 'pair.txt'), ids, pairs, scores)
    back = sio.load_pair(str(tmp_path / 'pair.txt'))
    assert back['id_list'] == ids
    for i, vid in enumerate(ids):
        assert back[vid]['pair'] == [ids[j] for j in pairs[i]] and back[vid]['score'] == scores[i]
    from mvsdf_amd.datasets import prepare
    assert prepare.pair_indices(back) == pairs
    with pytest.raises(ValueError):
        viewsel.write_pair(str(tmp_path / 'bad.txt'), ids, pairs[:3], scores)
    with pytest.raises(ValueError):
        viewsel.write_pair(str(tmp_path / 'bad.txt'), ids, [[4], [], [], []], [[1.0], [], [], []])


def test_argument_errors_need_no_gpu():
    pts, ctr = np.zeros((4, 3)), np.zeros((2, 3))
    vis = np.ones((2, 4), np.uint8)
    with pytest.raises(ValueError, match='sigma'):
        viewsel.view_scores(pts, ctr, vis, sigma1=0.0)
    with pytest.raises(ValueError, match='theta0'):
        viewsel.view_scores(pts, ctr, vis, theta0=float('nan'))
    with pytest.raises(ValueError, match=r'\[P, 3\]'):
        viewsel.view_scores(np.zeros((4, 2)), ctr, vis)
    with pytest.raises(ValueError, match='centers'):
        viewsel.view_scores(pts, np.zeros((2, 4)), vis)
    with pytest.raises(ValueError, match='V must be'):
        viewsel.view_scores(pts, np.zeros((0, 3)), np.ones((0, 4), np.uint8))
    with pytest.raises(ValueError, match='lo <= hi'):
        viewsel.depth_ranges(pts, vis, np.stack([np.eye(4)] * 2), lo=0.5, hi=0.2)
    with pytest.raises(ValueError, match=r'\[V, 4, 4\]'):
        viewsel.depth_ranges(pts, vis, np.eye(4))
    with pytest.raises(ValueError):
        viewsel.weights_host(np.zeros((3, 3)), np.zeros((2, 3)))
    with pytest.raises(ValueError):
        viewsel.select_pairs(np.zeros((2, 3)), np.zeros((2, 3)))


def test_arc_scene_prefers_arc_neighbours():
    """The end-to-end GPU test relies on this property of tests/colmap_scene.py; here the restatement alone shows it on the CPU."""
    pts, ctr, E, vis = CS.scene_arrays(CS.make_scene())
    scores, counts = R.view_scores(pts, ctr, vis)
    pairs, _ = R.select_pairs(scores, counts)
    assert np.array_equal(scores, scores.T) and (np.diag(scores) == 0).all() and (vis.sum(1) > 50).all()
    for i, q in enumerate(pairs):
        assert abs(q[0] - i) == 1, (i, q)
