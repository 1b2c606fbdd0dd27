"""mvsdf_amd/registration.py on the device against tests/registration_ref.py, bit for bit unless a test says otherwise.  The cases of
tests/test_registration_host.py (which holds the reference itself to brute force and known answers) run here too."""
import functools

import numpy as np
import pytest
import torch

import registration_ref as R
import test_registration_host as H
from mvsdf_amd import registration as G

pytestmark = pytest.mark.gpu
INF = float('inf')


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.astype(np.float64).view(np.uint64), b.astype(np.float64).view(np.uint64))


def _check_query(tree, refs, queries, max_dist):
    dist, index = tree.query(queries, max_dist)
    rd, ri, _ = R.nearest(queries, refs, max_dist)
    assert dist.dtype == torch.float64 and index.dtype == torch.int32 and dist.shape == (len(queries),) and index.shape == (len(queries),)
    assert _same(_np(dist), rd) and np.array_equal(_np(index), ri)
    return rd


@pytest.mark.parametrize('nr', [1, 15, 16, 17, 129, 2049])          # one leaf, a leaf's edge, a second and a third tree level
def test_query_sizes(nr):
    rs = np.random.RandomState(nr)
    refs = rs.uniform(-1, 1, (nr, 3))
    tree = G.NearestTree(refs)
    assert len(tree) == nr and _same(tree.centre, R.box_centre(refs))
    for nq in (0, 1, 255, 256, 257):
        queries = np.concatenate([refs[rs.randint(0, nr, nq // 2)] + 0.05 * rs.randn(nq // 2, 3), rs.uniform(-1.5, 1.5, (nq - nq // 2, 3))])
        rd = _check_query(tree, refs, queries, 0.2)
        _check_query(tree, refs, queries, INF)
        if nq >= 255:
            assert np.isinf(rd).any() and np.isfinite(rd).any()


def test_query_ties_and_the_strict_cut_off():
    refs, queries = H.lattice()
    tree = G.NearestTree(refs)
    for max_dist in (INF, 0.75, float(np.sqrt(0.75)), 0.5):      # sqrt(0.75): exactly the distance of the cell centres
        _check_query(tree, refs, queries, max_dist)
    dist, index = tree.query(queries[:125], float(np.sqrt(0.75)))
    assert bool(torch.isinf(dist).all()) and bool((index == -1).all())
    dist, index = tree.query(queries[125:250])
    assert np.array_equal(_np(index), np.arange(125))            # a duplicate (index >= 125) never wins over the original
    same = np.zeros((300, 3)) + [0.25, -3.0, 7.0]                # every reference at one place: index 0
    dist, index = G.NearestTree(same).query(np.array([[0.0, 0, 0], [0.25, -3.0, 7.0]]))
    assert np.array_equal(_np(index), [0, 0]) and _np(dist)[1] == 0


def test_query_rejects_non_finite_input_and_reuses_the_tree():
    rs = np.random.RandomState(0)
    refs, qa, qb = rs.randn(700, 3), rs.randn(300, 3), 2 * rs.randn(257, 3)
    tree = G.NearestTree(refs)
    for bad in (np.nan, np.inf):
        q = qa.copy()
        q[17, 1] = bad
        with pytest.raises(ValueError):
            tree.query(q)
        dist, index = tree.query(q, check_finite=False)
        assert _np(dist)[17] == INF and _np(index)[17] == -1
        r = refs.copy()
        r[5, 2] = bad
        with pytest.raises(ValueError):
            G.NearestTree(r)
    with pytest.raises(ValueError):
        tree.query(qa, 0.0)
    with pytest.raises(ValueError):
        G.NearestTree(np.zeros((0, 3)))
    a1, b1 = tree.query(qa, 0.5), tree.query(qb, 0.5)            # two queries of one tree = two fresh trees
    a2, b2 = G.NearestTree(refs).query(qa, 0.5), G.NearestTree(refs).query(qb, 0.5)
    for x, y in ((a1, a2), (b1, b2)):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    T = R.rigid((3, 1, -2), 25, (0.2, 0.1, -0.3))
    moved = tree.query(qa, 0.5, transform=T)
    plain = tree.query(G.transform_points(qa, T), 0.5)
    assert torch.equal(moved[0], plain[0]) and torch.equal(moved[1], plain[1])


def test_transform_points():
    rs = np.random.RandomState(1)
    p = rs.randn(5000, 3) * [1, 10, 100]
    for T in (R.rigid((1, 2, 3), 37, (0.3, -0.2, 0.5)), np.r_[rs.randn(3, 4), [[0, 0, 0, 1.0]]], np.eye(4)):
        assert _same(_np(G.transform_points(p, T)), R.transform_points(p, T))
    assert G.transform_points(np.zeros((0, 3)), np.eye(4)).shape == (0, 3)
    with pytest.raises(ValueError):
        G.transform_points(p, np.eye(3))


def _check_crop(p, axis, lo, hi, poly):
    keep, out = G.crop_volume(p, axis, lo, hi, poly)
    want = R.crop_volume(p, axis, lo, hi, poly)
    assert keep.dtype == torch.bool and np.array_equal(_np(keep), want) and _same(_np(out), np.asarray(p, np.float64)[want])
    return want


def test_crop_volume():
    p, want = H.crop_cases()
    assert np.array_equal(_check_crop(p, 'Z', -1.0, 1.0, H.L_SHAPE), want)
    assert np.array_equal(_check_crop(p[:, [2, 0, 1]], 'X', -1.0, 1.0, H.L_SHAPE[:, [2, 0, 1]]), want)
    assert np.array_equal(_check_crop(p[:, [0, 2, 1]], 'Y', -1.0, 1.0, H.L_SHAPE[:, [0, 2, 1]]), want)
    rs = np.random.RandomState(2)
    q = np.round(rs.uniform(-0.5, 2.5, (5000, 3)) * 8) / 8        # on a grid of eighths: many points on edges and on vertices' coordinates
    kept = _check_crop(q, 'Z', 0.0, 2.0, H.L_SHAPE)
    assert 1000 < kept.sum() < 4000
    a = np.linspace(0, 2 * np.pi, 4096, endpoint=False)
    star = np.stack([(1 + 0.3 * np.sin(7 * a)) * np.cos(a) + 1, 0 * a, (1 + 0.3 * np.sin(7 * a)) * np.sin(a) + 1], 1)      # the largest polygon
    kept = _check_crop(rs.uniform(-0.5, 2.5, (5000, 3)), 'y', 0.5, 1.5, star)
    assert 300 < kept.sum() < 3000
    with pytest.raises(ValueError):
        G.crop_volume(q, 'Z', 0.0, 2.0, H.L_SHAPE[:2])
    with pytest.raises(ValueError):
        G.crop_volume(q, 'Z', 0.0, 2.0, np.zeros((4097, 3)))
    with pytest.raises(ValueError):
        G.crop_volume(q, 'W', 0.0, 2.0, H.L_SHAPE)
    keep, out = G.crop_volume(q + 100.0, 'Z', 0.0, 2.0, H.L_SHAPE)
    assert out.shape == (0, 3) and not bool(keep.any())


def _check_voxel(p, voxel):
    means, counts = G.voxel_downsample(p, voxel)
    m, c = R.voxel_downsample(p, voxel)
    assert counts.dtype == torch.int32 and _same(_np(means), m) and np.array_equal(_np(counts), c)
    return c


def test_voxel_downsample():
    for p, voxel, means, counts in H.voxel_cases():
        assert np.array_equal(_check_voxel(p, voxel), counts) and _same(_np(G.voxel_downsample(p, voxel)[0]), means)
    p = np.random.RandomState(3).uniform(-1, 1, (5000, 3)) * [1, 2, 0.5]
    assert len(_check_voxel(p, 0.07)) > 2000
    assert np.array_equal(_check_voxel(p, 10.0), [5000])         # all points in one voxel: one lane sums 5000 points in input order
    assert np.array_equal(_check_voxel(p, 1e-5), np.ones(5000))  # every point in its own voxel
    _check_voxel(np.array([[0.0, 0, 0], [2.0 ** 21 - 1, 0, 0]]), 1.0)
    with pytest.raises(ValueError):
        G.voxel_downsample(np.array([[0.0, 0, 0], [0, 2.0 ** 21, 0]]), 1.0)         # 2^21 cells along y
    with pytest.raises(ValueError):
        G.voxel_downsample(np.array([[0.0, 0, 0], [0, np.nan, 0]]), 1.0)
    with pytest.raises(ValueError):
        G.voxel_downsample(p, 0.0)
    assert _same(_np(G.uniform_downsample(p, 7)), p[::7]) and G.uniform_downsample(p, 5000).shape == (1, 3)


def _half_matched(n, seed):
    """n source points of the height field, about half of them lifted out of reach of the target"""
    src = R.surface(n, seed)
    src[np.random.RandomState(seed).uniform(size=n) < 0.5, 2] += 5.0
    return src


@pytest.mark.parametrize('n', [2049, 257])                        # two workgroups with one item in the second; one partly filled
def test_the_17_sums_of_an_iteration(n):
    tgt = R.surface(1500, 1)
    src = _half_matched(n, n)
    T = R.rigid((1, -1, 2), 2, (0.01, 0.02, -0.01))
    tree = G.NearestTree(tgt)
    cnt, sums, d2, index = G.pair_sums(src, tree, T, 0.3)
    rc, rsums, rd2, rindex = R.pair_sums(src, tgt, T, 0.3)
    assert 0.3 * n < rc < 0.7 * n
    assert cnt == rc and np.array_equal(_np(index), rindex) and _same(_np(d2), rd2)
    assert len(sums) == 16 and _same(sums, rsums), (sums, rsums)


def test_no_matched_pair():
    tgt = R.surface(1500, 1)
    tree = G.NearestTree(tgt)
    src = R.surface(300, 2) + [0, 0, 5.0]
    cnt, sums, d2, index = G.pair_sums(src, tree, np.eye(4), 0.3)
    assert cnt == 0 and sums == [0.0] * 16 and bool((index == -1).all()) and bool(torch.isinf(d2).all())
    with pytest.raises(ValueError):
        G.icp(src, tree, max_dist=0.3)
    q = src.copy()
    q[3, 0] = np.nan
    with pytest.raises(ValueError):
        G.pair_sums(q, tree, np.eye(4), 0.3)


def test_icp_recovers_a_rigid_copy_with_the_reference_s_bits():
    src, tgt = H.rigid_copy()
    reg = G.icp(src, G.NearestTree(tgt), max_dist=0.3)
    T, fitness, rmse, iterations = R.icp(src, tgt, max_dist=0.3)
    assert reg.transformation.shape == (4, 4) and reg.transformation.dtype == np.float64
    assert _same(reg.transformation, T) and _same(reg.fitness, fitness) and _same(reg.inlier_rmse, rmse) and reg.iterations == iterations
    assert R.angle_between(reg.transformation, H.MOTION) <= H.ICP_ANGLE_BOUND
    assert np.abs(reg.transformation[:3, 3] - H.MOTION[:3, 3]).max() <= H.ICP_SHIFT_BOUND
    one = G.icp(src, G.NearestTree(tgt), max_dist=0.3, max_iter=1)
    assert one.iterations == 1 and _same(one.transformation, R.icp(src, tgt, max_dist=0.3, max_iter=1)[0])
    init = R.rigid((0, 0, 1), 1, (0.01, 0, 0))
    assert _same(G.icp(src, G.NearestTree(tgt), init, 0.3, 3).transformation, R.icp(src, tgt, init, 0.3, 3)[0])


def _check_fscore(rec, gt, tau, **kw):
    f, r = G.fscore(rec, gt, tau, **kw), R.fscore(rec, gt, tau, **kw)
    assert f['below_rec'] == r['below_rec'] and f['below_gt'] == r['below_gt'] and (f['n_rec'], f['n_gt']) == (len(rec), len(gt))
    assert f['hist_rec'].dtype == np.int64 and np.array_equal(f['hist_rec'], r['hist_rec']) and np.array_equal(f['hist_gt'], r['hist_gt'])
    cut = max(r['edges'][-1], tau)                               # the device reports +inf from there on; the definition's results do not read those
    assert _same(f['edges'], r['edges'])
    for k in ('dist_rec', 'dist_gt'):
        assert _same(_np(f[k]), np.where(r[k] < cut, r[k], np.inf)), k
    for k in ('precision', 'recall', 'fscore'):
        assert _same(f[k], r[k]), k
    return f


def test_fscore():
    rec, gt = R.surface(1200, 7) + [0.004, -0.003, 0.006], R.surface(1500, 8)
    f = _check_fscore(rec, gt, 0.02)
    assert 0.1 < f['fscore'] < 0.9 and len(f['hist_rec']) == 500 and 0 < f['hist_rec'].sum() <= 1200
    _check_fscore(rec, gt, 0.01, stretch=3, bins_per_tau=7)
    # a distance equal to tau is not below it; a distance on an edge goes to the upper bin; at or beyond the last edge it is dropped
    gt2 = np.array([[0.0, 0, 0], [10.0, 0, 0]])
    rec2 = np.array([[0.25, 0, 0], [0.5, 0, 0], [0.125, 0, 0], [10.0, 3.0, 0]])
    f = _check_fscore(rec2, gt2, 0.25, stretch=2, bins_per_tau=2)
    assert f['below_rec'] == 1 and f['precision'] == 0.25 and np.array_equal(f['hist_rec'], [0, 1, 1, 0]) and f['recall'] == 0.5
    f = _check_fscore(rec + 100.0, gt, 0.02)                      # nothing within tau: F = 0, not NaN
    assert f['precision'] == 0.0 and f['recall'] == 0.0 and f['fscore'] == 0.0 and f['hist_rec'].sum() == 0
    with pytest.raises(ValueError):
        G.fscore(rec, gt, 0.02, stretch=50, bins_per_tau=100)


TAU = 0.02


@functools.lru_cache(None)
def scene():
    """ground truth: 6000 points of the height field; reconstruction: 5000 other samples of it, moved so that H.MOTION brings them back; the crop (a
    square prism of edge 1.6) cuts off part of both -> (rec, gt, the reference's result)"""
    gt = R.surface(6000, 2)
    rec = R.transform_points(R.surface(5000, 3), np.linalg.inv(H.MOTION))
    return rec, gt, R.tnt_evaluate(rec, gt, H.CROP, np.eye(4), TAU)


def _score_at(T):
    rec, gt, _ = scene()
    c = (H.CROP['orthogonal_axis'], H.CROP['axis_min'], H.CROP['axis_max'], np.array(H.CROP['bounding_polygon']))
    S = R.transform_points(rec, T)
    return R.fscore(R.voxel_downsample(S[R.crop_volume(S, *c)], TAU / 2)[0], R.voxel_downsample(gt[R.crop_volume(gt, *c)], TAU / 2)[0], TAU)['fscore']


def test_tnt_evaluate_end_to_end(tmp_path, capsys):
    """The F-scores of this scene by registration_ref on the CPU: 0.3419 at the initial alignment (the identity), 0.7750 after the three
    registration stages, 0.7737 at the true alignment (the registered pose is 0.31 degrees from the true one: point-to-point ICP on resampled
    near-planar data slides in the plane, which the score does not see, so the rotation is not asserted).  The margin below the true alignment's
    score is twice the reference's own |registered - true| = 2 * 0.0013."""
    rec, gt, ref = scene()
    r = G.tnt_evaluate(rec, gt, H.CROP, np.eye(4), TAU)
    assert r['points'] == ref['points'] and len(r['points']) == 15 and r['points'][2] < 6000 and r['points'][3] < 5000
    assert _same(r['transformation'], ref['transformation'])
    for k in ('precision', 'recall', 'fscore'):
        assert _same(r[k], ref[k]), k
    assert np.array_equal(r['histograms'][0], ref['histograms'][0]) and np.array_equal(r['histograms'][1], ref['histograms'][1])
    assert _same(r['edges'], ref['edges']) and (r['below_rec'], r['below_gt']) == (ref['below_rec'], ref['below_gt'])
    f_init, f_true = _score_at(np.eye(4)), _score_at(H.MOTION)
    print('F-score: initial %.4f, registered %.4f, true alignment %.4f' % (f_init, r['fscore'], f_true))
    assert r['fscore'] >= f_true - 0.0026 and r['fscore'] > f_init
    # stages= replaces the table: one voxel stage only
    one = [('voxel', TAU, 80 * TAU)]
    assert _same(G.tnt_evaluate(rec, gt, H.CROP, np.eye(4), TAU, stages=one)['transformation'],
                 R.tnt_evaluate(rec, gt, H.CROP, np.eye(4), TAU, stages=one)['transformation'])
    # the command on the scene's directory prints the same three numbers
    H.write_scene(str(tmp_path), 'Shed', gt, H.CROP, np.eye(4))
    H.write_ply(str(tmp_path / 'rec.ply'), rec, '<f8')
    capsys.readouterr()
    H._tool().main([str(tmp_path / 'rec.ply'), '--scene_dir', str(tmp_path), '--scene', 'Shed', '--tau', str(TAU), '--mode', 'pcd', '--out', str(tmp_path / 'out')])
    assert capsys.readouterr().out.split() == [repr(r['precision']), repr(r['recall']), repr(r['fscore'])]
    assert _same(np.loadtxt(str(tmp_path / 'out' / 'Shed.transformation.txt')), r['transformation'])
    assert np.array_equal(np.loadtxt(str(tmp_path / 'out' / 'Shed.precision.txt'))[:, 1], r['histograms'][0])
    # --traj: the reconstruction and its cameras in a frame of their own (a similarity S away from COLMAP's).  The centres' alignment returns S to
    # 1e-13, so the registration starts 1e-13 from where it started above and the score can differ only by points that sit that close to tau or
    # to a voxel or crop boundary: none or a few of about 3000 per side, far inside 0.01
    S = R.rigid((1, -2, 0.5), 50, (3, -1, 2))
    S[:3, :3] *= 1.7
    poses = H._poses(9, 4)
    mine = [np.linalg.inv(S) @ m for m in poses]
    H.write_scene(str(tmp_path), 'Shed', gt, H.CROP, np.eye(4), poses)
    H.write_log(str(tmp_path / 'mine.log'), mine)
    H.write_ply(str(tmp_path / 'rec_mine.ply'), R.transform_points(rec, np.linalg.inv(S)), '<f8')
    t = H._tool().main([str(tmp_path / 'rec_mine.ply'), '--scene_dir', str(tmp_path), '--scene', 'Shed', '--tau', str(TAU), '--mode', 'pcd',
                        '--traj', str(tmp_path / 'mine.log')])
    assert abs(t['fscore'] - r['fscore']) < 0.01


def test_tnt_evaluate_takes_a_mesh():
    from mvsdf_amd.mesh import Mesh
    g = np.linspace(-1, 1, 41)
    xy = np.stack(np.meshgrid(g, g, indexing='ij'), -1).reshape(-1, 2)
    v = np.concatenate([xy, R.height_field(xy)[:, None]], 1).astype(np.float32)
    i = (np.arange(40)[:, None] * 41 + np.arange(40)[None, :]).reshape(-1)
    f = np.concatenate([np.stack([i, i + 41, i + 1], 1), np.stack([i + 1, i + 41, i + 42], 1)]).astype(np.int32)
    mesh = Mesh(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), torch.zeros(len(v), 3).cuda())
    from mvsdf_amd.chamfer import sample_mesh
    pts = sample_mesh(mesh, 0.02)
    stages = [('voxel', 0.04, 0.5)]
    a = G.tnt_evaluate(mesh, pts, H.CROP, np.eye(4), 0.04, stages=stages, density=0.02)
    b = G.tnt_evaluate(pts, pts, H.CROP, np.eye(4), 0.04, stages=stages)
    assert a['points'] == b['points'] and _same(a['fscore'], b['fscore']) and a['fscore'] == 1.0
