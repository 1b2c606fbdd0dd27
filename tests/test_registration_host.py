"""The numpy restatement of the registration definitions (tests/registration_ref.py) against brute force and known answers, the host half of
mvsdf_amd/registration.py (Horn's solve, the composition, the loaders, the centre alignment) and the command's argument checks.  No GPU needed."""
import importlib.util
import json
import os

import numpy as np
import pytest

import registration_ref as R
from conftest import ROOT
from mvsdf_amd import registration as G


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def lattice():
    """a 5 x 5 x 5 integer lattice with 40 of its points repeated: many exact ties, in distance and in position"""
    g = np.stack(np.meshgrid(*[np.arange(5.0)] * 3, indexing='ij'), -1).reshape(-1, 3)
    rs = np.random.RandomState(0)
    refs = np.concatenate([g, g[rs.permutation(125)[:40]]])
    queries = np.concatenate([g + 0.5, g, g + [0.5, 0, 0], rs.uniform(-1, 5, (100, 3))])
    return refs, queries


def test_nearest_equals_the_brute_force_argmin_with_the_lowest_index_on_ties():
    refs, queries = lattice()
    for max_dist in (np.inf, 0.75, np.sqrt(0.75), 0.5):          # sqrt(0.75): exactly the distance of the cell centres (strict <)
        a, b = R.nearest(queries, refs, max_dist), R.nearest_brute(queries, refs, max_dist)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    dist, index, _ = R.nearest(queries, refs)
    assert np.array_equal(index[125:250], np.arange(125)) and (dist[125:250] == 0).all()     # a duplicate (index >= 125) never wins over the original
    assert np.isinf(R.nearest(queries[:125], refs, np.sqrt(0.75))[0]).all() and np.isfinite(R.nearest(queries[:125], refs, 0.87)[0]).all()
    d, i, _ = R.nearest(np.zeros((0, 3)), refs)
    assert d.shape == (0,) and i.shape == (0,) and i.dtype == np.int32
    with pytest.raises(ValueError):
        R.nearest(np.array([[0, np.nan, 0]]), refs)


def _plain_sums(p, q):
    return [0.0] + [float(p[:, a].sum()) for a in range(3)] + [float(q[:, a].sum()) for a in range(3)] + \
        [float((p[:, a] * q[:, b]).sum()) for a in range(3) for b in range(3)]


def test_horn_returns_a_known_rotation():
    """37 degrees about (1, 2, 3) plus a translation from 50 exact pairs.  Measured with registration_ref here: largest entry error 1.7e-16,
    angle error 1.2e-14 degrees; the bounds are 100 x that (the margin is for other libm builds; only sqrt is used, which IEEE fixes)."""
    T0 = R.rigid((1, 2, 3), 37, (0.3, -0.2, 0.5))
    p = np.random.RandomState(0).uniform(-1, 1, (50, 3))
    q = R.transform_points(p, T0)
    for centre in ([0.0, 0.0, 0.0], [0.25, -0.5, 0.125]):
        sums = _plain_sums(p - centre, q - centre)
        U = np.array(R.horn_update(50, sums, centre))
        err, ang = np.abs(U - T0).max(), R.angle_between(U, T0)
        print('horn: entry error %.3g, angle error %.3g degrees' % (err, ang))
        assert err <= 1.7e-14 and ang <= 1.2e-12
        assert np.array_equal(_bits(U), _bits(G.horn_update(50, sums, centre)))          # the module spells the same arithmetic
    R3 = np.array(R.horn_rotation([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]))
    assert np.array_equal(R3, np.eye(3))                         # a diagonal N: every rotation skipped, w = 1
    A, B = np.random.RandomState(1).randn(4, 4), np.random.RandomState(2).randn(4, 4)
    A[3], B[3] = [0, 0, 0, 1], [0, 0, 0, 1]
    AB = np.array(R.compose(A.tolist(), B.tolist()))
    assert np.array_equal(_bits(AB), _bits(G.compose(A.tolist(), B.tolist()))) and np.abs(AB - A @ B).max() < 1e-15


def rigid_copy():
    """the target: 1500 points of the height field; the source: the same points shuffled and moved so that MOTION brings them back"""
    tgt = R.surface(1500, 1)
    src = R.transform_points(tgt[np.random.RandomState(0).permutation(1500)], np.linalg.inv(MOTION))
    return src, tgt


MOTION = R.rigid((1, 2, 3), 4, (0.03, -0.02, 0.025))
# what registration_ref.icp measures on rigid_copy(): 8 updates, rotation error 1.03e-14 degrees, translation error 2.8e-17, rmse 1.6e-16; the
# bounds are 100 x those
ICP_ANGLE_BOUND, ICP_SHIFT_BOUND = 1.1e-12, 2.8e-15


def test_reference_icp_recovers_a_rigid_copy():
    src, tgt = rigid_copy()
    T, fitness, rmse, iterations = R.icp(src, tgt, max_dist=0.3)
    ang, shift = R.angle_between(T, MOTION), np.abs(T[:3, 3] - MOTION[:3, 3]).max()
    print('icp: %d updates, angle error %.3g degrees, translation error %.3g, rmse %.3g' % (iterations, ang, shift, rmse))
    assert fitness == 1.0 and iterations < 20
    assert ang <= ICP_ANGLE_BOUND and shift <= ICP_SHIFT_BOUND and rmse <= 1.6e-14
    with pytest.raises(ValueError):
        R.icp(src + 100.0, tgt, max_dist=0.3)                    # nothing within max_dist


def test_fixed_order_sum():
    rs = np.random.RandomState(0)
    for n in (1, 7, 8, 9, 2047, 2048, 2049, 5000, 2048 * 1024 + 5):
        v = rs.randint(-1000, 1000, n).astype(np.float64)
        assert R.fixed_sum(v) == v.sum()                         # integers: every order gives the exact sum
        assert R.fixed_sum(np.ones(n, np.int64)) == n
    v = rs.randn(5000)
    assert abs(R.fixed_sum(v) - float(np.sum(v.astype(np.longdouble)))) < 1e-12
    lane = ((v[0] + v[1]) + v[2]) + v[3]                          # a lane's items are summed sequentially from 0.0
    assert R.fixed_sum(v[:4]) == lane


L_SHAPE = np.array([[0, 0, 9], [2, 0, 9], [2, 1, 9], [1, 1, 9], [1, 2, 9], [0, 2, 9]], np.float64)     # (the w coordinate of a vertex is not read)


def crop_cases():
    """(points, expected keep) for the L-shaped prism along Z between -1 and 1"""
    cases = [((0.5, 0.5, 0), True), ((1.5, 0.5, 0), True), ((0.5, 1.5, 0), True), ((1.5, 1.5, 0), False), ((2.5, 0.5, 0), False),
             ((-0.5, 0.5, 0), False), ((0.5, 2.5, 0), False), ((0.5, -0.5, 0), False),
             # on a vertex's v coordinate: y = 1 crosses the edges that end there once (< on one side, >= on the other)
             ((0.5, 1.0, 0), True), ((1.5, 1.0, 0), True), ((2.5, 1.0, 0), False), ((-0.5, 1.0, 0), False),
             # y = 2: a horizontal edge is never crossed, the edges that end on it are (>=): the top edge belongs to the prism, and right of x = 1
             # both are crossed -> outside; y = 0: no edge has a vertex below (<) -> the bottom edge does not belong to it
             ((0.5, 2.0, 0), True), ((1.5, 2.0, 0), False), ((0.5, 0.0, 0), False),
             # the axis bounds are inclusive
             ((0.5, 0.5, -1.0), True), ((0.5, 0.5, 1.0), True), ((0.5, 0.5, np.nextafter(1.0, 2)), False), ((0.5, 0.5, np.nextafter(-1.0, -2)), False)]
    return np.array([c[0] for c in cases], np.float64), np.array([c[1] for c in cases])


def test_crop_rule_on_a_concave_polygon():
    p, want = crop_cases()
    assert np.array_equal(R.crop_volume(p, 'Z', -1.0, 1.0, L_SHAPE), want)
    assert np.array_equal(R.crop_volume(p, 2, -1.0, 1.0, L_SHAPE[::-1]), want)            # the orientation of the polygon does not matter
    # the same prism along X (u, v, w = y, z, x) and along Y (u, v, w = x, z, y)
    assert np.array_equal(R.crop_volume(p[:, [2, 0, 1]], 'X', -1.0, 1.0, L_SHAPE[:, [2, 0, 1]]), want)
    assert np.array_equal(R.crop_volume(p[:, [0, 2, 1]], 'Y', -1.0, 1.0, L_SHAPE[:, [0, 2, 1]]), want)


def voxel_cases():
    """(points, voxel, expected means, expected counts)"""
    a = [-1.0, -1.0, -1.0]
    return [
        # negative coordinates; -0.75 lies exactly on the boundary of cells 0 and 1 along x (o = -1.25, (p - o) / 0.5 = 1.0) and belongs to cell 1
        (np.array([a, [-0.75, -1, -1], [-0.8, -1, -1]]), 0.5, np.array([[(0.0 + -1.0 + -0.8) / 2, -1, -1], [-0.75, -1, -1]]), [2, 1]),
        # ascending key: x is the lowest digit, z the highest
        (np.array([a, [-1, -1, 0.0], [-1, 0.0, -1], [0.0, -1, -1]]), 0.5, np.array([a, [0.0, -1, -1], [-1, 0.0, -1], [-1, -1, 0.0]]), [1, 1, 1, 1]),
        (np.array([[3.5, -2.25, 1e-3]]), 0.01, np.array([[3.5, -2.25, 1e-3]]), [1]),                          # a single point
    ]


def test_voxel_filter_cases():
    for p, voxel, means, counts in voxel_cases():
        m, c = R.voxel_downsample(p, voxel)
        assert np.array_equal(_bits(m), _bits(means)) and np.array_equal(c, counts) and c.dtype == np.int32
    rs = np.random.RandomState(0)
    p = rs.uniform(-1, 1, (3000, 3))
    m, c = R.voxel_downsample(p, 0.25)
    assert c.sum() == 3000 and len(m) <= 9 ** 3 and np.abs((m * c[:, None]).sum(0) - p.sum(0)).max() < 1e-9
    with pytest.raises(ValueError):
        R.voxel_downsample(np.array([[0.0, 0, 0], [2.0 ** 21, 0, 0]]), 1.0)
    assert len(R.voxel_downsample(np.array([[0.0, 0, 0], [2.0 ** 21 - 1, 0, 0]]), 1.0)[0]) == 2


def test_fscore_reference_edges_and_ties():
    gt = np.array([[0.0, 0, 0], [10.0, 0, 0]])
    rec = np.array([[0.25, 0, 0], [0.5, 0, 0], [0.125, 0, 0], [10.0, 3.0, 0]])
    f = R.fscore(rec, gt, 0.25, stretch=2, bins_per_tau=2)       # edges 0, 0.125, 0.25, 0.375, 0.5
    assert np.array_equal(f['edges'], [0, 0.125, 0.25, 0.375, 0.5])
    assert f['below_rec'] == 1 and f['precision'] == 0.25        # 0.25 is not < tau
    assert np.array_equal(f['hist_rec'], [0, 1, 1, 0])           # 0.125 on an edge -> the upper bin; 0.5 at the last edge and 3.0 are dropped
    assert f['below_gt'] == 1 and f['recall'] == 0.5 and f['fscore'] == 2 * 0.25 * 0.5 / 0.75
    far = R.fscore(rec + 100.0, gt, 0.25)
    assert far['precision'] == 0.0 and far['recall'] == 0.0 and far['fscore'] == 0.0


# ---------------------------------------------------------------- files and the command ----------------------------------------------------------------
def write_ply(path, pts, dtype='<f4'):
    name = {'<f4': 'float', '<f8': 'double'}[dtype]
    head = 'ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty %s x\nproperty %s y\nproperty %s z\nend_header\n' % (len(pts), name, name, name)
    with open(path, 'wb') as f:
        f.write(head.encode('ascii') + np.ascontiguousarray(pts, dtype).tobytes())


def write_log(path, poses):
    with open(path, 'w') as f:
        for k, m in enumerate(poses):
            f.write('%d %d 0\n' % (k, k))
            for row in m:
                f.write(' '.join(repr(float(x)) for x in row) + '\n')


def write_scene(d, scene, gt, crop, trans, poses=None):
    write_ply(os.path.join(d, scene + '.ply'), gt, '<f8')
    with open(os.path.join(d, scene + '.json'), 'w') as f:
        json.dump(dict(crop, class_name='SelectionPolygonVolume', version_major=1, version_minor=0), f)
    np.savetxt(os.path.join(d, scene + '_trans.txt'), trans, fmt='%.17g')
    if poses is not None:
        write_log(os.path.join(d, scene + '_COLMAP_SfM.log'), poses)


CROP = {'orthogonal_axis': 'Z', 'axis_min': -1.0, 'axis_max': 1.0,
        'bounding_polygon': [[-0.8, -0.8, 0.0], [0.8, -0.8, 0.0], [0.8, 0.8, 0.0], [-0.8, 0.8, 0.0]]}


def _poses(n, seed):
    rs = np.random.RandomState(seed)
    return [R.rigid(rs.randn(3), rs.uniform(0, 180), rs.uniform(-2, 2, 3)) for _ in range(n)]


def test_loaders_round_trip(tmp_path):
    gt = R.surface(100, 5)
    trans = R.rigid((0, 1, 1), 20, (1, 2, 3))
    poses = _poses(7, 0)
    write_scene(str(tmp_path), 'Shed', gt, CROP, trans, poses)
    s = G.load_tnt_scene(str(tmp_path), 'Shed')
    assert np.array_equal(s['gt'], gt) and np.array_equal(s['trans'], trans)
    assert s['crop']['orthogonal_axis'] == 'Z' and s['crop']['bounding_polygon'] == CROP['bounding_polygon'] and s['crop']['axis_max'] == 1.0
    assert len(s['trajectory']) == 7 and all(meta == (k, k, 0) and np.array_equal(m, poses[k]) for k, (meta, m) in enumerate(s['trajectory']))
    os.remove(str(tmp_path / 'Shed_COLMAP_SfM.log'))
    assert G.load_tnt_scene(str(tmp_path), 'Shed')['trajectory'] is None
    with pytest.raises(FileNotFoundError):
        G.load_tnt_scene(str(tmp_path), 'Barn')
    bad = tmp_path / 'bad.log'
    bad.write_text('0 0 0\n1 0 0 0\n0 1 0 0\n0 0 1 0\n')
    with pytest.raises(ValueError):
        G.load_trajectory(str(bad))
    bad.write_text('0 0 0\n1 0 0 0\n0 1 0 0\n0 0 1\n0 0 0 1\n')
    with pytest.raises(ValueError):
        G.load_trajectory(str(bad))


def test_align_centres_recovers_a_similarity():
    rs = np.random.RandomState(3)
    src = rs.uniform(-3, 3, (30, 3))
    S = R.rigid((2, -1, 0.5), 63, (0.5, -4, 2))
    S[:3, :3] *= 2.5
    dst = R.transform_points(src, S)
    assert np.abs(G.align_centres(src, dst) - S).max() < 1e-13
    S1 = R.rigid((2, -1, 0.5), 63, (0.5, -4, 2))
    assert np.abs(G.align_centres(src, R.transform_points(src, S1), with_scale=False) - S1).max() < 1e-13
    with pytest.raises(ValueError):
        G.align_centres(src[:2], dst[:2])


def _tool():
    spec = importlib.util.spec_from_file_location('eval_tnt', os.path.join(ROOT, 'tools', 'eval_tnt.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_the_command_rejects_a_missing_file_or_scene(tmp_path, capsys):
    tool = _tool()
    write_scene(str(tmp_path), 'Shed', R.surface(50, 1), CROP, np.eye(4))
    rec = str(tmp_path / 'rec.ply')
    write_ply(rec, R.surface(50, 2))
    for argv, word in ((['nothing.ply', '--scene_dir', str(tmp_path), '--scene', 'Shed', '--tau', '0.02'], 'nothing.ply'),
                       ([rec, '--scene_dir', str(tmp_path), '--scene', 'Barn'], 'Barn'),
                       ([rec, '--scene_dir', str(tmp_path), '--scene', 'Shed'], 'tau'),               # no default tau for an unknown scene
                       ([rec, '--scene_dir', str(tmp_path), '--scene', 'Shed', '--tau', '0.02', '--traj', rec], 'COLMAP_SfM.log')):
        with pytest.raises(SystemExit) as e:
            tool.main(argv)
        assert e.value.code == 1 and word in capsys.readouterr().err
    assert set(G.TNT_TAU) == {'Barn', 'Caterpillar', 'Church', 'Courthouse', 'Ignatius', 'Meetingroom', 'Truck'} and G.TNT_TAU['Ignatius'] == 0.003
