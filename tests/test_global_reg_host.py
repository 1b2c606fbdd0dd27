"""tests/global_reg_ref.py, the numpy restatement of mvsdf_amd/global_reg.py, on its own (no GPU): the invariances the definition promises, the matcher
against a plain double loop, the sampler against literals computed with Python integers, and the whole pipeline on a synthetic scene with a known
motion.  tests/test_gpu_global_reg.py then holds the device to this restatement bit for bit."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import global_reg_ref as G  # noqa: E402
import normals_ref as NR  # noqa: E402
import registration_ref as RR  # noqa: E402

# the scene's parameters (tests/test_gpu_global_reg.py uses the same)
VOXEL, K, HYPOTHESES = 0.07, 32, 20000
# the worst errors of the restated global_register (no refine) over the seeds 0 .. 4, as measured: 6.798 degrees (seed 0) and 0.0638 (seed 0; 0.9
# voxels); per seed (degrees, length): (6.798, 0.0638) (6.734, 0.0565) (4.358, 0.0410) (5.894, 0.0329) (3.121, 0.0279)
WORST_ROTATION, WORST_TRANSLATION = 6.798, 0.0638


def _lattice_cloud(n, seed):
    """points whose coordinates are multiples of 2^-12 in [-1, 1) (a shift by small powers of two is exact) and arbitrary normals"""
    rs = np.random.RandomState(seed)
    P = np.unique(rs.randint(-4096, 4096, size=(n, 3)), axis=0).astype(np.float64) / 4096.0
    P = P[rs.permutation(len(P))]
    N = rs.normal(size=P.shape)
    return P, N / np.linalg.norm(N, axis=1, keepdims=True)


def _descriptor(P, N, k, radius):
    nb = NR.knn_indices(P, k)[0]
    hist, count = G.spfh(P, N, nb, radius)
    feat, codes = G.fpfh(P, nb, hist, count, radius)
    return nb, hist, count, feat, codes


def test_descriptor_is_invariant_under_exact_motions():
    """a quarter turn about z ((x, y, z) -> (-y, x, z)) and a shift by powers of two are exact in fp64 and commute with every sum the definition
    writes: the histograms, counts and codes are the same integers"""
    P, N = _lattice_cloud(400, 3)
    for radius in (None, 0.3):
        nb, hist, count, _, codes = _descriptor(P, N, 12, radius)
        assert count.max() > 0 and (radius is None or count.min() < 12)
        P2 = np.stack([-P[:, 1], P[:, 0], P[:, 2]], 1) + np.array([4.0, -8.0, 16.0])
        N2 = np.stack([-N[:, 1], N[:, 0], N[:, 2]], 1)
        nb2, hist2, count2, _, codes2 = _descriptor(P2, N2, 12, radius)
        assert np.array_equal(nb, nb2)
        assert np.array_equal(hist, hist2) and np.array_equal(count, count2) and np.array_equal(codes, codes2)
        assert hist.dtype == np.int32 and count.dtype == np.int32 and codes.dtype == np.int8
        assert np.array_equal(hist.reshape(len(P), 3, 11).sum(2), np.repeat(count[:, None], 3, 1))


def _off_edges(x, eps=1e-9):
    return bool((np.abs(x - np.round(x)) > eps).all())


def test_mirror_codes_is_the_descriptor_of_negated_normals():
    rs = np.random.RandomState(5)
    P = rs.uniform(-1, 1, size=(300, 3))
    N = rs.normal(size=P.shape)
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    nb, hist, count, feat, codes = _descriptor(P, N, 10, None)
    # the cloud is built so that no feature lies on a bin edge and no positive descriptor entry on a code edge
    valid, theta, alpha, phi = G.pair_features(P, N, nb)
    assert valid.all()
    for f, lo, hi in ((theta, -G.PI, G.PI), (alpha, -1.0, 1.0), (phi, -1.0, 1.0)):
        assert _off_edges(G.bin_position(f, lo, hi))
    assert _off_edges(feat[feat > 0] * 1.27)
    _, hist_m, count_m, _, codes_m = _descriptor(P, -N, 10, None)
    assert np.array_equal(count, count_m)
    assert np.array_equal(hist_m[:, 11:22], hist[:, 11:22]) and np.array_equal(hist_m[:, :11], hist[:, 10::-1])
    assert np.array_equal(G.mirror_codes(codes), codes_m)
    assert not np.array_equal(codes, codes_m)
    assert np.array_equal(G.mirror_codes(G.mirror_codes(codes)), codes)


def _match_loops(s, t):
    index, dist = [], []
    for i in range(len(s)):
        best = None
        for j in range(len(t)):
            D = sum((int(a) - int(b)) ** 2 for a, b in zip(s[i], t[j]))
            if best is None or D < best[0]:
                best = (D, j)
        dist.append(best[0])
        index.append(best[1])
    return np.array(index, np.int32), np.array(dist, np.int32)


def test_match_features_is_the_double_loop():
    rs = np.random.RandomState(7)
    for hi in (2, 128):                                                     # codes in 0 .. 1: ties everywhere; the full range: hardly any
        s = rs.randint(0, hi, size=(37, 33)).astype(np.int8)
        t = rs.randint(0, hi, size=(29, 33)).astype(np.int8)
        t[11] = t[3]                                                         # an exact tie: the lower index wins
        s[5] = t[11]
        want_i, want_d = _match_loops(s, t)
        index, dist = G.match_features(s, t)
        assert index.dtype == np.int32 and dist.dtype == np.int32
        assert np.array_equal(index, want_i) and np.array_equal(dist, want_d)
        assert index[5] == 3 and dist[5] == 0
        back, _ = _match_loops(t, s)
        mutual, dist_m = G.match_features(s, t, mutual=True)
        assert np.array_equal(mutual, np.where(back[want_i] == np.arange(len(s)), want_i, -1)) and np.array_equal(dist_m, want_d)
        assert (mutual >= 0).any() and (mutual < 0).any()
    assert G.match_features(np.full((4, 33), 127, np.int8), np.zeros((2, 33), np.int8))[1].tolist() == [33 * 127 * 127] * 4


def test_sampler_literals():
    """the indices for a few (seed, h, M), computed with Python integers"""
    cases = [((0, 0, 3), (0, 2, 1)), ((0, 1, 1000), (26, 970, 106)), ((1, 0, 1000), (338, 893, 745)), ((7, 12345, 870), (502, 164, 316)),
             ((2 ** 64 - 1, 99999, 2 ** 31 - 1), (1434102527, 889793574, 1571202836)), ((123456789, 4194303, 257), (235, 168, 94))]
    for (seed, h, M), want in cases:
        assert tuple(G.sample_indices(seed, [h], M)[0].tolist()) == want, (seed, h, M)
    m = G.sample_indices(3, np.arange(5000), 7)
    assert m.min() == 0 and m.max() == 6


def test_ransac_finds_a_known_motion_among_outliers():
    rs = np.random.RandomState(2)
    src = rs.uniform(-1, 1, size=(200, 3))
    motion = RR.rigid((0.3, -1.0, 0.5), 75.0, (0.4, 0.1, -2.0))
    dst = RR.transform_points(src, motion)
    corr = np.stack([np.arange(200), np.arange(200)], 1).astype(np.int32)
    bad = rs.permutation(200)[:140]
    corr[bad, 1] = rs.randint(0, 200, size=140)
    truth = corr[:, 0] == corr[:, 1]
    reg = G.ransac(src, dst, corr, 1e-6, hypotheses=4096, seed=1)
    assert reg.hypothesis >= 0 and reg.inliers == int(truth.sum()) and np.array_equal(reg.mask, truth) and reg.checked >= 1
    assert np.abs(reg.transformation - motion).max() < 1e-9
    nothing = G.ransac(src, dst, np.stack([np.arange(200), np.zeros(200, np.int64)], 1), 0.1, hypotheses=512)
    assert nothing.hypothesis == -1 and nothing.inliers == 0 and nothing.checked == 0 and not nothing.mask.any()
    assert np.array_equal(nothing.transformation, np.eye(4))
    index = np.where(truth, corr[:, 1], -1).astype(np.int32)                # the index-array form: -1 entries dropped in order
    sub = G.ransac(src, dst, index, 1e-6, hypotheses=64, seed=1)
    assert len(sub.mask) == int(truth.sum()) and sub.inliers == len(sub.mask)


@functools.lru_cache(None)
def scene_run(seed, refine):
    """the restated global_register on the scene of `seed` -> (GlobalResult, the winning search, source, target, motion)"""
    s, t, motion = G.scene(seed)
    res, reg = G.global_register(s, t, VOXEL, k=K, hypotheses=HYPOTHESES, seed=seed, refine=refine)
    return res, reg, s, t, motion


def test_pipeline_recovers_the_motion_of_the_scene():
    """An ellipsoid with seven bumps; the source covers about 65 % of it, the target is an independent sampling of all of it turned by 170 degrees
    about (1, 2, 3) and shifted (global_reg_ref.scene: no point exists twice, nothing relates the frames).  About 715 source and 1020 target points
    after the voxel filter, k = 32, 20,000 hypotheses.  Measured over the seeds 0 .. 4 without refine: rotation errors 6.798, 6.734, 4.358, 5.894,
    3.121 degrees, translation errors 0.0638, 0.0565, 0.0410, 0.0329, 0.0279; inliers 64, 74, 68, 73, 66 of 702 .. 752 correspondences (9 to
    10 %).  The bounds are twice the worst value: the margin covers a re-seeding of the scene, nothing else."""
    for seed in range(5):
        res, reg, s, t, motion = scene_run(seed, False)
        rot, trans = G.motion_errors(res.transformation, motion)
        print('seed %d: rotation %.3f degrees, translation %.4f, inliers %d of %d, checked %d' % (seed, rot, trans, res.inliers, len(reg.mask), reg.checked))
        assert rot < 2 * WORST_ROTATION and trans < 2 * WORST_TRANSLATION, (seed, rot, trans)
        assert res.inliers >= 0.03 * len(reg.mask), (seed, res.inliers, len(reg.mask))
        assert res.inliers == int(reg.mask.sum()) and res.fitness is None


def test_refined_pipeline_reaches_the_fitness_of_the_true_motion():
    for seed in range(5):
        res, reg, s, t, motion = scene_run(seed, True)
        ds, dt = RR.voxel_downsample(s, VOXEL)[0], RR.voxel_downsample(t, VOXEL)[0]
        truth = RR.icp(ds, dt, motion, 1.5 * VOXEL)
        print('seed %d: fitness %.4f, from the true motion %.4f' % (seed, res.fitness, truth[1]))
        assert res.fitness >= 0.9 * truth[1], (seed, res.fitness, truth[1])
