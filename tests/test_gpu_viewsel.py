"""View selection on the GPU: view_scores against the numpy restatement bit for bit (both visibility forms, twice in a row), depth_ranges, the
device error bits, and COLMAP model -> MVS directory -> plane sweep end to end."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import colmap_scene as CS                                                   # noqa: E402
import viewsel_ref as R                                                     # noqa: E402
from mvsdf_amd import viewsel                                               # noqa: E402

pytestmark = pytest.mark.gpu

PATTERNS = ('all', 'single', 'random', 'blind')


def _scene(V, P, seed=0):
    rng = np.random.RandomState(seed)
    phi = rng.uniform(0, 2 * np.pi, V)
    centers = np.stack([4 * np.cos(phi), rng.uniform(-1, 1, V), 4 * np.sin(phi)], 1)
    return rng.uniform(-1, 1, (P, 3)), centers


def _visibility(pattern, V, P, seed=0):
    rng = np.random.RandomState(seed + 1)
    if pattern == 'all':
        return np.ones((V, P), bool)
    if pattern == 'single':                                                 # tracks of length 1: no pairs at all
        vis = np.zeros((V, P), bool)
        vis[np.arange(P) % V, np.arange(P)] = True
        return vis
    if pattern == 'random':
        return rng.uniform(size=(V, P)) < 0.1
    vis = rng.uniform(size=(V, P)) < 0.5                                    # 'blind': one view sees nothing
    vis[V // 2] = False
    return vis


def _tracks(vis, rng=None, duplicates=False):
    """bool [V, P] -> (track_off int64 [P+1], track_view int32); with duplicates some entries are repeated and each track is shuffled"""
    off, view = [0], []
    for p in range(vis.shape[1]):
        t = np.flatnonzero(vis[:, p]).tolist()
        if duplicates and t:
            t = t + [t[i] for i in rng.randint(0, len(t), 1 + len(t) // 2)]
            rng.shuffle(t)
        view += t
        off.append(len(view))
    return np.array(off, np.int64), np.array(view, np.int32)


def _check(points, centers, vis, **kw):
    s_ref, c_ref = R.view_scores(points, centers, vis, kw.get('theta0', 5.0), kw.get('sigma1', 1.0), kw.get('sigma2', 10.0))
    results = [viewsel.view_scores(points, centers, vis.astype(np.uint8), **kw), viewsel.view_scores(points, centers, torch.from_numpy(vis).cuda(), **kw),
               viewsel.view_scores(points, centers, _tracks(vis), **kw)]
    for s, c in results:
        assert s.dtype == torch.float64 and c.dtype == torch.int64 and s.is_cuda and c.is_cuda
        assert np.array_equal(c.cpu().numpy(), c_ref)
        assert np.array_equal(s.cpu().numpy().view(np.uint64), s_ref.view(np.uint64)), 'scores differ in %d cells' % (s.cpu().numpy() != s_ref).sum()
    return s_ref, c_ref


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('P', [0, 1, 63, 1000])
@pytest.mark.parametrize('V', [1, 2, 3, 64, 65, 130])
def test_view_scores_equal_restatement(V, P, pattern):
    points, centers = _scene(V, P, seed=V * 7 + P)
    vis = _visibility(pattern, V, P, seed=V + P)
    s, c = _check(points, centers, vis)
    assert np.array_equal(s, s.T) and (np.diag(s) == 0).all() and np.array_equal(np.diag(c), vis.sum(1))
    if pattern == 'single' or P == 0 or V == 1:
        assert (s == 0).all() and (c - np.diag(np.diag(c)) == 0).all()
        assert viewsel.select_pairs(s, c) == ([[] for _ in range(V)], [[] for _ in range(V)])
    if pattern == 'all':
        assert (c == P).all()
    if pattern != 'single' and V >= 64 and P == 1000:                       # among that many cameras on the ring some pair is a few degrees apart
        assert s.max() > 1


def test_other_parameters_and_small_angles():
    points, _ = _scene(70, 500, seed=3)
    rng = np.random.RandomState(4)
    centers = np.array([0.0, 0.0, -6.0]) + 0.4 * rng.randn(70, 3)           # a tight cluster of cameras: angles around theta0, both branches of the weight
    vis = rng.uniform(size=(70, 500)) < 0.6
    s, _ = _check(points, centers, vis)
    assert s.max() > 50
    _check(points, centers, vis, theta0=2.0, sigma1=0.5, sigma2=3.0)


def test_coincident_point_shared_centre_and_duplicate_track_entries():
    points, centers = _scene(5, 40, seed=5)
    points[7] = centers[2]                                                  # a point at a camera centre: that view's unit vector is 0, theta = 0
    centers[4] = centers[1]                                                 # two views share a centre: theta = 0 for every common point
    vis = np.ones((5, 40), bool)
    s_ref, c_ref = _check(points, centers, vis)
    w0 = int(R.quantise(R.weight(np.float64(0.0))))
    assert s_ref[1, 4] == 40 * w0 * 2.0 ** -32
    rng = np.random.RandomState(6)
    vis = rng.uniform(size=(5, 40)) < 0.6
    s_ref, c_ref = R.view_scores(points, centers, vis)
    off, view = _tracks(vis, rng, duplicates=True)
    assert len(view) > vis.sum()
    s, c = viewsel.view_scores(points, centers, (torch.from_numpy(off), torch.from_numpy(view)))
    assert np.array_equal(c.cpu().numpy(), c_ref) and np.array_equal(s.cpu().numpy(), s_ref)


def test_depth_ranges_equal_restatement_and_name_the_blind_view():
    rng = np.random.RandomState(7)
    P = 300
    points = rng.uniform(-1, 1, (P, 3))
    scene = CS.make_scene(n_views=6)
    E = CS.scene_arrays(scene)[2]
    vis = np.zeros((6, P), bool)
    for v, n in enumerate((1, 2, 100, 101, 37, P)):                          # the index rule's edge counts
        vis[v, rng.permutation(P)[:n]] = True
    ref = R.depth_ranges(points, vis, E)
    for form in (vis, torch.from_numpy(vis.astype(np.uint8)).cuda(), _tracks(vis)):
        out = viewsel.depth_ranges(points, form, E)
        assert out.is_cuda and out.dtype == torch.float64 and np.array_equal(out.cpu().numpy().view(np.uint64), ref.view(np.uint64))
    assert ref[0, 0] == ref[0, 1] and (ref[2:, 0] < ref[2:, 1]).all()
    ref = R.depth_ranges(points, vis, E, 0.0, 0.5)
    assert np.array_equal(viewsel.depth_ranges(points, vis, E, lo=0.0, hi=0.5).cpu().numpy(), ref)
    vis[3] = False
    with pytest.raises(ValueError, match='view 3 sees no point'):
        viewsel.depth_ranges(points, vis, E)
    with pytest.raises(ValueError, match='view 0 sees no point'):
        viewsel.depth_ranges(np.zeros((0, 3)), np.zeros((6, 0), bool), E)


def test_device_error_bits():
    points, centers = _scene(3, 50, seed=8)
    vis = np.ones((3, 50), bool)
    bad = points.copy()
    bad[17, 1] = np.nan
    with pytest.raises(ValueError, match='NaN or infinite'):
        viewsel.view_scores(bad, centers, vis)
    badc = centers.copy()
    badc[2, 0] = np.inf
    with pytest.raises(ValueError, match='NaN or infinite'):
        viewsel.view_scores(points, badc, vis)
    off, view = _tracks(vis)
    view[11] = 3                                                            # == V
    with pytest.raises(ValueError, match='track view'):
        viewsel.view_scores(points, centers, (off, view))
    view[11] = -1
    with pytest.raises(ValueError, match='track view'):
        viewsel.view_scores(points, centers, (off, view))
    with pytest.raises(ValueError, match='NaN or infinite'):
        viewsel.depth_ranges(bad, vis, np.stack([np.eye(4)] * 3))
    s, c = viewsel.view_scores(points, centers, vis)                        # and the next call is clean again
    assert np.array_equal(s.cpu().numpy(), R.view_scores(points, centers, vis)[0])


def test_colmap_to_mvs_end_to_end(tmp_path):
    from mvsdf_amd import stereo
    from mvsdf_amd.datasets import colmap, prepare
    from mvsdf_amd.utils import io as sio
    scene = CS.make_scene(n_views=6, n_points=300)
    CS.write_binary(scene, str(tmp_path / 'sparse'))
    CS.write_images(scene, str(tmp_path / 'photos'))
    out = str(tmp_path / 'mvs')
    res = colmap.colmap_to_mvs(str(tmp_path / 'sparse'), str(tmp_path / 'photos'), out, max_d=32, num_pairs=4)
    points, centers, E, vis = CS.scene_arrays(scene)
    s_ref, c_ref = R.view_scores(points, centers, vis)
    assert np.array_equal(res['scores'].cpu().numpy(), s_ref) and np.array_equal(res['counts'].cpu().numpy(), c_ref)
    pairs_ref, ps_ref = R.select_pairs(s_ref, c_ref, 4)
    pair = sio.load_pair(os.path.join(out, 'pair.txt'))
    assert pair['id_list'] == [str(i) for i in range(6)]
    assert prepare.pair_indices(pair) == pairs_ref and [pair[str(i)]['score'] for i in range(6)] == ps_ref
    for i, q in enumerate(pairs_ref):
        assert abs(q[0] - i) == 1                                           # the first source is an arc neighbour
    ranges = R.depth_ranges(points, vis, E)
    for i in range(6):
        assert os.path.exists(os.path.join(out, 'images', '%08d.png' % i))
        cam = sio.load_cam(os.path.join(out, 'cams', '%08d_cam.txt' % i), 32, 1)
        assert np.array_equal(cam[0], E[i]) and cam[1, 3, 0] == ranges[i, 0] and cam[1, 3, 3] == ranges[i, 1] and cam[1, 3, 2] == 32
        assert cam[1, 3, 1] == (ranges[i, 1] - ranges[i, 0]) / 31 and cam[1, 0, 2] == CS.W / 2 and cam[1, 1, 2] == CS.H / 2
    sweep = stereo.estimate_scene(out, str(tmp_path / 'result'), num_src=2, max_d=32)
    assert tuple(sweep.depths.shape) == (6, CS.H // 2, CS.W // 2) and bool(torch.isfinite(sweep.depths).all()) and bool((sweep.best_k >= 0).any())
    assert os.path.exists(str(tmp_path / 'result' / '00000005_flow3.pfm'))


def test_select_views_tool_rewrites_pair_from_a_mesh(tmp_path):
    from mvsdf_amd import raster
    from mvsdf_amd.datasets import colmap, prepare
    from mvsdf_amd.mesh import Mesh
    from mvsdf_amd.utils import io as sio
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import select_views
    scene = CS.make_scene(n_views=6, n_points=300)
    CS.write_text(scene, str(tmp_path / 'sparse'))
    CS.write_images(scene, str(tmp_path / 'photos'))
    out = str(tmp_path / 'mvs')
    res = colmap.colmap_to_mvs(str(tmp_path / 'sparse'), str(tmp_path / 'photos'), out, max_d=32, num_pairs=3)
    before = open(os.path.join(out, 'pair.txt')).read()
    n = 21                                                                  # a square patch facing the arc, 21 x 21 vertices
    g = np.linspace(-1, 1, n)
    verts = np.stack([np.tile(g, n), np.repeat(g, n), 0.2 * np.sin(2 * np.tile(g, n))], 1).astype(np.float32)
    idx = (np.arange(n - 1)[:, None] * n + np.arange(n - 1)[None]).reshape(-1)
    faces = np.concatenate([np.stack([idx, idx + 1, idx + n], 1), np.stack([idx + 1, idx + n + 1, idx + n], 1)]).astype(np.int32)
    mesh = Mesh(verts, faces, np.tile(np.float32([0, 0, -1]), (n * n, 1)))
    mesh.export(str(tmp_path / 'patch.ply'))
    pairs, pair_scores = select_views.main([str(tmp_path / 'patch.ply'), '--data_root', out, '--num_pairs', '2'])
    assert open(os.path.join(out, 'pair.txt.bak')).read() == before
    pair = sio.load_pair(os.path.join(out, 'pair.txt'))
    assert prepare.pair_indices(pair) == pairs and all(len(q) == 2 for q in pairs)
    dmesh = mesh.to('cuda')
    vis = raster.vertex_visibility(dmesh, raster.rasterize(dmesh, cams=res['cams'], hw=(CS.H, CS.W))).cpu().numpy()
    assert vis.sum() > 3 * n * n
    s_ref, c_ref = R.view_scores(verts.astype(np.float64), viewsel.centers_from_cams(res['cams']), vis)
    assert (pairs, pair_scores) == R.select_pairs(s_ref, c_ref, 2)
    assert [pair[str(i)]['score'] for i in range(6)] == pair_scores


def test_nonfinite_entries_at_the_end_and_beyond_the_first_grid_stride():
    """the finite check (csrc/geom_prims.h: k_any_nonfinite) runs a capped grid of 1024 x 256 lanes that strides over its array: a NaN in the last element
    of the points, the centres and the extrinsics, and one in the points that only a lane's second round reaches, must all raise"""
    V, P = 3, 90000
    assert 3 * P > 1024 * 256 + 4096
    points, centers = _scene(V, P, seed=9)
    vis = np.ones((V, P), bool)
    E = np.stack([np.eye(4)] * V)
    E[:, 2, 3] = 6.0
    for at in (3 * P - 1, 1024 * 256 + 4095):
        bad = points.copy()
        bad.reshape(-1)[at] = np.nan
        with pytest.raises(ValueError, match='NaN or infinite'):
            viewsel.view_scores(bad, centers, vis)
        with pytest.raises(ValueError, match='NaN or infinite'):
            viewsel.depth_ranges(bad, vis, E)
    badc = centers.copy()
    badc[V - 1, 2] = np.inf
    with pytest.raises(ValueError, match='NaN or infinite'):
        viewsel.view_scores(points, badc, vis)
    badE = E.copy()
    badE[V - 1, 2, 3] = np.nan
    with pytest.raises(ValueError, match='NaN or infinite'):
        viewsel.depth_ranges(points, vis, badE)
    out = viewsel.depth_ranges(points, vis, E)                              # and the next call is clean again
    assert np.array_equal(out.cpu().numpy().view(np.uint64), R.depth_ranges(points, vis, E).view(np.uint64))
