"""mvsdf_amd/global_reg.py on the GPU against its numpy restatement (tests/global_reg_ref.py): histograms, counts, descriptors, codes, matches,
distances, transformations, counts and masks are compared bit for bit (np.array_equal on integers and on uint64 views of fp64), every call made twice."""
import functools
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import global_reg_ref as R  # noqa: E402
import normals_ref as NR  # noqa: E402
import registration_ref as RR  # noqa: E402
from test_global_reg_host import HYPOTHESES, K, VOXEL, WORST_ROTATION, WORST_TRANSLATION  # noqa: E402
from test_gpu_normals import KINDS, make_cloud  # noqa: E402
from mvsdf_amd import fusion, global_reg, registration  # noqa: E402

pytestmark = pytest.mark.gpu
JOBS = 16


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def np_(t):
    return t.cpu().numpy()


def twice(fn):
    return fn(), fn()


# ================================================================ the descriptors ================================================================
def _check_descriptor(P, N, nb, radius, tag):
    want_h, want_c = R.spfh(P, N, nb, radius)
    want_f, want_q = R.fpfh(P, nb, want_h, want_c, radius)
    for hist, count in twice(lambda: global_reg.spfh(P, N, nb, radius)):
        assert hist.dtype == torch.int32 and count.dtype == torch.int32
        assert np.array_equal(np_(hist), want_h), (tag, int((np_(hist) != want_h).any(1).sum()))
        assert np.array_equal(np_(count), want_c), tag
    for feat, codes in twice(lambda: global_reg.fpfh(P, nb, want_h, want_c, radius)):
        assert feat.dtype == torch.float64 and codes.dtype == torch.int8
        assert same_bits(np_(feat), want_f), (tag, int((bits(np_(feat)) != bits(want_f)).any(1).sum()))
        assert np.array_equal(np_(codes), want_q), tag
    return want_c


@pytest.mark.parametrize('kind', KINDS)
def test_descriptors_are_the_restatement(kind):
    for n in (2, 9, 33, 257, 4099):                                          # k + 1 for every k, then the sizes every k runs at
        P = make_cloud(kind, n, seed=1)
        rs = np.random.RandomState(n)
        N = rs.normal(size=(n, 3))
        N /= np.linalg.norm(N, axis=1, keepdims=True)
        N[rs.uniform(size=n) < 0.05] = 0.0                                  # zero normals: their pairs have no frame
        ks = (1, 8, 32) if n > 33 else (n - 1,)
        rows, d2 = NR.knn_indices(P, max(ks), jobs=JOBS)
        radius = float(np.sqrt(np.median(d2[:, 0]))) or 0.01               # the median nearest-neighbour distance: about half the rows keep nothing
        for k in ks:
            nb = np.ascontiguousarray(rows[:, :k])                           # (a shorter row is a prefix under a total order)
            nb[::7, 0] = np.arange(n, dtype=np.int32)[::7]                   # a row entry equal to its own index is no pair
            _check_descriptor(P, N, nb, None, (kind, n, k, None))
            count = _check_descriptor(P, N, nb, radius, (kind, n, k, radius))
            if kind == 'uniform' and n > 100:
                assert (count == 0).any() and (count > 0).any()


def test_descriptors_of_estimated_normals_on_a_surface():
    """the inputs the composed call makes: a surface, its estimated and oriented normals, device tensors in"""
    P = RR.voxel_downsample(R.scene(3)[0], VOXEL)[0]
    N, _, nb = NR.estimate_normals(P, 16, jobs=JOBS)
    N = NR.orient_normals(P, N, nb)[0]
    want_h, want_c = R.spfh(P, N, nb, 5 * VOXEL)
    want_q = R.fpfh(P, nb, want_h, want_c, 5 * VOXEL)[1]
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (P, N, nb)]
    hist, count = global_reg.spfh(dev[0], dev[1], dev[2], 5 * VOXEL)
    assert np.array_equal(np_(hist), want_h) and np.array_equal(np_(count), want_c)
    codes = global_reg.fpfh(dev[0], dev[2], hist, count, 5 * VOXEL)[1]
    assert np.array_equal(np_(codes), want_q)
    assert np.array_equal(np_(global_reg.mirror_codes(codes)), R.mirror_codes(want_q))


def test_descriptor_arguments_are_checked():
    P = make_cloud('uniform', 64)
    N = np.ones((64, 3))
    nb = NR.knn_indices(P, 4)[0]
    with pytest.raises(ValueError):
        global_reg.spfh(P.astype(np.float32), N, nb)
    with pytest.raises(ValueError):
        global_reg.spfh(P, N, nb.astype(np.int64))
    with pytest.raises(ValueError):
        global_reg.spfh(P, N, np.zeros((64, 33), np.int32))
    with pytest.raises(ValueError):
        global_reg.spfh(P, N, nb, radius=0.0)
    bad = nb.copy()
    bad[5, 2] = 64
    with pytest.raises(ValueError, match='index'):
        global_reg.spfh(P, N, bad)
    Nn = N.copy()
    Nn[7, 1] = np.nan
    with pytest.raises(ValueError, match='normal'):
        global_reg.spfh(P, Nn, nb)
    hist, count = global_reg.spfh(P, N, nb)
    with pytest.raises(ValueError, match='index'):
        global_reg.fpfh(P, bad, hist, count)
    with pytest.raises(ValueError):
        global_reg.fpfh(P, nb, hist.long(), count)


# ================================================================ the matcher ================================================================
def _check_match(s, t, mutual=False):
    want_i, want_d = R.match_features(s, t, mutual)
    for index, dist in twice(lambda: global_reg.match_features(s, t, mutual)):
        assert index.dtype == torch.int32 and dist.dtype == torch.int32
        gi, gd = np_(index), np_(dist)
        assert np.array_equal(gd, want_d), (s.shape, t.shape, int((gd != want_d).sum()))
        assert np.array_equal(gi, want_i), (s.shape, t.shape, int((gi != want_i).sum()))
    return want_i, want_d


SIZES = (1, 15, 16, 17, 63, 64, 65, 257, 1031)


@functools.lru_cache(None)
def _codes(n, seed):
    return np.random.RandomState(seed).randint(0, 128, size=(n, 33)).astype(np.int8)


@pytest.mark.parametrize('ns', SIZES)
def test_match_sizes_crosswise(ns):
    for nt in SIZES:
        _check_match(_codes(ns, 1), _codes(nt, 2))


def test_match_extremes_and_ties():
    top = np.full((70, 33), 127, np.int8)
    _, d = _check_match(top, np.zeros((40, 33), np.int8))                    # the largest distance
    assert (d == 33 * 127 * 127).all()
    i, d = _check_match(top, top[:50])                                       # the largest dot product; every target ties: index 0
    assert (d == 0).all() and (i == 0).all()
    t = np.repeat(_codes(9, 3), 21, axis=0)                                  # blocks of 21 identical targets (across tile borders): the lowest index wins
    s = np.concatenate([_codes(9, 3)[::-1], _codes(30, 4)])
    i, d = _check_match(s, t)
    assert np.array_equal(i[:9], 21 * np.arange(8, -1, -1)) and (d[:9] == 0).all() and (i % 21 == 0).all()
    low = np.random.RandomState(5).randint(0, 3, size=(300, 33)).astype(np.int8)
    _check_match(low[:130], low[130:])                                       # three code values: ties between different rows everywhere


def test_match_asymmetric_pair_settles_the_operand_map():
    """sources one-hot in a different column per point, targets distinct ramps: D(i, j) = 127^2 + |t_j|^2 - 254 t_j[i] reads one entry of t_j, so a
    wrong byte order inside an operand, or rows taken for columns, gives another table"""
    s = np.zeros((33, 33), np.int8)
    s[np.arange(33), np.arange(33)] = 127
    j, c = np.meshgrid(np.arange(40), np.arange(33), indexing='ij')
    t = ((j * 29 + c * (j + 3)) % 128).astype(np.int8)
    assert len(np.unique(t, axis=0)) == 40
    want_i, want_d = _check_match(s, t)
    tn = (t.astype(np.int64) ** 2).sum(1)
    table = 127 * 127 + tn[None, :] - 254 * t.astype(np.int64).T              # [i, j]
    assert np.array_equal(want_d, table.min(1)) and np.array_equal(want_i, table.argmin(1))
    _check_match(t, s)                                                       # and with the roles exchanged


def test_match_mutual():
    for ns, nt in ((257, 63), (64, 1031), (300, 300)):
        want_i, _ = _check_match(_codes(ns, 6), _codes(nt, 7), mutual=True)
        assert (want_i >= 0).any() and (want_i < 0).any()
    c = _codes(100, 8)
    i, d = _check_match(c, c, mutual=True)                                   # a cloud against itself: everything is mutual
    assert np.array_equal(i, np.arange(100)) and (d == 0).all()


def test_match_split_targets_combine_atomically():
    """few sources and many targets: the walk over the targets is split over workgroups (GG_MIN_TILES = 64 tiles of 16 per split at the least, until
    about 2048 workgroups exist) and the splits combine by atomicMin"""
    assert global_reg.match_splits(1031, 1031) == 2 and global_reg.match_splits(17, 1024) == 1
    for ns, nt in ((17, 16 * 64 * 3 + 5), (1, 5000), (130, 2049)):
        assert global_reg.match_splits(ns, nt) >= 2
        t = _codes(nt, 9).copy()
        t[nt - 3] = t[7]                                                     # a tie between the first and the last split
        s = _codes(ns, 10).copy()
        s[0] = t[7]
        want_i, want_d = _check_match(s, t)
        assert want_i[0] == 7 and want_d[0] == 0
    _check_match(_codes(70, 11), _codes(4000, 12), mutual=True)


def test_match_arguments_are_checked():
    c = _codes(20, 1)
    with pytest.raises(ValueError):
        global_reg.match_features(c.astype(np.int32), c)
    with pytest.raises(ValueError):
        global_reg.match_features(c[:, :32], c)
    with pytest.raises(ValueError):
        global_reg.match_features(c[:0], c)
    bad = c.copy()
    bad[3, 4] = -1
    with pytest.raises(ValueError, match='code'):
        global_reg.match_features(c, bad)
    with pytest.raises(ValueError, match='code'):
        global_reg.match_features(bad, c)


# ================================================================ the hypothesis search ================================================================
def _check_ransac(src, dst, corr, max_dist, H, seed, edge_ratio=0.9):
    want = R.ransac(src, dst, corr, max_dist, H, seed, edge_ratio)
    for got in twice(lambda: global_reg.ransac(src, dst, corr, max_dist, H, seed, edge_ratio)):
        tag = (len(corr), H, seed, got[1:4], want[1:4])
        assert (got.hypothesis, got.inliers, got.checked) == (want.hypothesis, want.inliers, want.checked), tag
        assert same_bits(got.transformation, want.transformation), tag
        assert got.mask.dtype == torch.bool and np.array_equal(np_(got.mask), want.mask), tag
    return want


@functools.lru_cache(None)
def _motion_case():
    rs = np.random.RandomState(21)
    src = rs.uniform(-1, 1, size=(400, 3))
    motion = RR.rigid((0.3, -1.0, 0.5), 75.0, (0.4, 0.1, -2.0))
    dst = RR.transform_points(src, motion) + rs.normal(size=src.shape) * 0.004
    return src, dst, motion


def _corr(M, seed):
    """M correspondences of the known motion, 70 % of them replaced by random ones"""
    rs = np.random.RandomState(seed + M)
    a = rs.permutation(400)[:M] if M <= 400 else rs.randint(0, 400, size=M)
    corr = np.stack([a, a], 1).astype(np.int32)
    bad = rs.permutation(M)[:int(round(0.7 * M))]
    corr[bad, 1] = rs.randint(0, 400, size=len(bad))
    return corr


@pytest.mark.parametrize('M', (3, 4, 255, 256, 257, 1000))
def test_ransac_is_the_restatement(M):
    src, dst, motion = _motion_case()
    corr = _corr(M, 0)
    found = 0
    for H in (1, 63, 64, 65, 4096):
        want = _check_ransac(src, dst, corr, 0.03, H, seed=H)
        found += want.hypothesis >= 0
    if M >= 255:
        assert found >= 1 and want.inliers >= 0.25 * M
        assert RR.angle_between(want.transformation, motion) < 2.0


def test_ransac_edge_cases():
    src, dst, _ = _motion_case()
    one = np.stack([np.arange(300), np.zeros(300, np.int64)], 1).astype(np.int32)
    want = _check_ransac(src, dst, one, 0.5, 4096, seed=1)                   # all correspondences to one target point: every hypothesis is rejected
    assert want.hypothesis == -1 and want.checked == 0 and want.inliers == 0 and np.array_equal(want.transformation, np.eye(4))
    dup = np.repeat(np.stack([np.arange(40), np.arange(40)], 1).astype(np.int32), 5, axis=0)     # every correspondence five times
    want = _check_ransac(src, dst, dup, 0.03, 4096, seed=2)
    assert want.hypothesis >= 0 and want.inliers % 5 == 0 and want.checked < 4096
    _check_ransac(src, dst, dup, 0.03, 512, seed=2 ** 64 - 1, edge_ratio=0.0)      # no edge test: many survivors, many of them wrong
    _check_ransac(src * 1e-9, dst * 1e-9, _corr(256, 3), 1e3, 256, seed=3)   # everything within max_dist: the score ties at M, the lowest h wins
    index = np.where(np.arange(400) % 3 == 0, np.arange(400), -1).astype(np.int32)
    want = _check_ransac(src, dst, index, 0.03, 64, seed=4)                  # the index-array form
    assert len(want.mask) == int((index >= 0).sum()) and want.inliers == len(want.mask)


def test_ransac_arguments_are_checked():
    src, dst, _ = _motion_case()
    corr = _corr(100, 0)
    for kw in ({'hypotheses': 0}, {'hypotheses': 2 ** 22 + 1}, {'seed': -1}, {'seed': 2 ** 64}, {'edge_ratio': 1.5}):
        with pytest.raises(ValueError):
            global_reg.ransac(src, dst, corr, 0.1, **kw)
    with pytest.raises(ValueError):
        global_reg.ransac(src, dst, corr, 0.0)
    with pytest.raises(ValueError):
        global_reg.ransac(src, dst, corr[:2], 0.1)
    with pytest.raises(ValueError):
        global_reg.ransac(src, dst, corr.astype(np.int64), 0.1)
    bad = corr.copy()
    bad[50, 1] = 400
    with pytest.raises(ValueError, match='index'):
        global_reg.ransac(src, dst, bad, 0.1, hypotheses=4096)
    nan = src.copy()
    nan[corr[3, 0], 2] = np.inf
    with pytest.raises(ValueError, match='coordinate'):
        global_reg.ransac(nan, dst, corr, 0.1, hypotheses=64)


# ================================================================ the composed call and the command ================================================================
def test_global_register_is_the_restatement_on_the_scene():
    """the scene and the measured bounds of tests/test_global_reg_host.py"""
    s, t, motion = R.scene(0)
    want, want_reg = R.global_register(s, t, VOXEL, k=K, hypotheses=HYPOTHESES, seed=0, refine=False, jobs=JOBS)
    for got, reg in twice(lambda: global_reg.global_register(s, t, VOXEL, k=K, hypotheses=HYPOTHESES, seed=0, refine=False, return_search=True)):
        assert (got.inliers, got.flipped, reg.hypothesis, reg.checked) == (want.inliers, want.flipped, want_reg.hypothesis, want_reg.checked)
        assert same_bits(got.transformation, want.transformation) and np.array_equal(np_(reg.mask), want_reg.mask)
        assert got.fitness is None and got.inlier_rmse is None
    fin = global_reg.global_register(s, t, VOXEL, k=K, hypotheses=HYPOTHESES, seed=0)
    rot, trans = R.motion_errors(fin.transformation, motion)
    print('refined: rotation %.3f degrees, translation %.4f, fitness %.4f' % (rot, trans, fin.fitness))
    assert rot < 2 * WORST_ROTATION and trans < 2 * WORST_TRANSLATION
    ds, dt = registration.voxel_downsample(s, VOXEL)[0], registration.voxel_downsample(t, VOXEL)[0]
    truth = registration.icp(ds, registration.NearestTree(dt), motion, 1.5 * VOXEL)
    assert fin.fitness >= 0.9 * truth.fitness and fin.inliers == want.inliers


def test_global_register_takes_given_normals_and_flips():
    """analytic normals of a sphere-like scene given for both clouds, the source's negated: flip='auto' finds the mirrored codes"""
    s, t, motion = R.scene(1)
    ns = -(s / R.RADII ** 2)                                                 # about inward: the ellipsoid's gradient, negated
    tl = RR.transform_points(t, np.linalg.inv(motion))
    nt = (tl / R.RADII ** 2) @ motion[:3, :3].T
    kw = dict(source_normals=ns, target_normals=nt, k=K, hypotheses=HYPOTHESES, seed=1, refine=False)
    want, _ = R.global_register(s, t, VOXEL, jobs=JOBS, **kw)
    got = global_reg.global_register(s, t, VOXEL, **kw)
    assert (got.inliers, got.flipped) == (want.inliers, want.flipped) and same_bits(got.transformation, want.transformation)
    assert got.flipped and R.motion_errors(got.transformation, motion)[0] < 2 * WORST_ROTATION


def test_align_clouds_tool_writes_a_trajectory(tmp_path):
    spec = importlib.util.spec_from_file_location('tool_align_clouds', os.path.join(ROOT, 'tools', 'align_clouds.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    s, t, motion = R.scene(2)
    a, b, out = str(tmp_path / 'a.ply'), str(tmp_path / 'b.ply'), str(tmp_path / 'T.log')
    fusion.save_points(a, s)
    fusion.save_points(b, t)
    r = tool.main([a, b, '--voxel', str(VOXEL), '--hypotheses', str(HYPOTHESES), '--seed', '2', '--out', out])
    traj = registration.load_trajectory(out)
    assert len(traj) == 1 and traj[0][0] == (0, 0, 1) and same_bits(traj[0][1], r.transformation)
    assert R.motion_errors(r.transformation, motion)[0] < 2 * WORST_ROTATION and r.fitness > 0.8
