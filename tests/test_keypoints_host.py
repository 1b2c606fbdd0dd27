"""The numpy restatement of mvsdf_amd/keypoints.py (tests/keypoints_ref.py) alone against analytic truth, the module's host-side camera arrays, its
argument checks and its constants.  No GPU needed."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keypoints_ref as R  # noqa: E402
import keypoints_scene as S  # noqa: E402
from mvsdf_amd import keypoints as KP  # noqa: E402
from mvsdf_amd._lib import K  # noqa: E402

# distance of the triangulated points of the synthetic scene to the true sphere (keypoints with 0.3 px noise, depth about 3, baseline 0.6): twice
# what the restatement measures
MEDIAN_SPHERE_DISTANCE = 2 * 0.0057         # measured 0.005695
WORST_SPHERE_DISTANCE = 2 * 0.0415          # measured 0.041495
# x_b^T F x_a of an exact correspondence, in units of |F x_a|: pixel coordinates up to 192 carried through three 3 x 3 products in fp64; a
# thousand roundings of 2^-53 at that magnitude stay below this
EPIPOLAR_ROUNDING = 192 * 1000 * 2.0 ** -53


@pytest.fixture(scope='module')
def scene():
    cams, xy, codes, vo, point, pts = S.synthetic_keypoints()
    m = R.match_descriptors(codes, vo)
    v = R.verify_matches(xy, vo, m, KP.fundamental_matrices(cams, m[0]))
    tracks = R.build_tracks(vo, v)
    tri = R.triangulate_tracks(xy, vo, tracks, KP.camera_arrays(cams))
    return dict(cams=cams, xy=xy, codes=codes, vo=vo, point=point, pts=pts, matches=m, verified=v, tracks=tracks, tri=tri)


def _globals(vo, m):
    pid = np.repeat(np.arange(len(m[0])), np.diff(m[1]))
    return vo[m[0][pid, 0]] + m[2][:, 0], vo[m[0][pid, 1]] + m[2][:, 1]


def test_constants_and_error_table():
    assert KP.DIM == 128 and K.MVSDF_KP_MAX_DIST == 128 * 127 * 127
    bits = [row[0] for row in KP.ERRORS]
    assert bits == [8, 1, 2, 128, 256, 512] and all(issubclass(row[1], Exception) and row[2] for row in KP.ERRORS)
    block = {v for k, v in vars(K).items() if k.startswith('MVSDF_PS_ERR_')}
    assert set(bits) <= block


def test_scene_matches_are_true_and_points_lie_on_the_sphere(scene):
    vo, point = scene['vo'], scene['point']
    assert (np.diff(scene['matches'][1]) >= 60).all()
    ga, gb = _globals(vo, scene['verified'])
    true = (point[ga] == point[gb]) & (point[ga] >= 0)
    assert (np.diff(scene['verified'][1]) >= 50).all() and true.mean() >= 0.9
    ga0, gb0 = _globals(vo, scene['matches'])
    false_before = int(((point[ga0] != point[gb0]) | (point[ga0] < 0)).sum())
    assert false_before > int((~true).sum())                                       # the verification removes wrong matches, not only right ones
    xyz, err, keep, obs_keep = scene['tri']
    assert keep.sum() >= 90
    d = np.abs(np.linalg.norm(xyz[keep] - S.CENTER, axis=1) - S.RADIUS)
    print('sphere distance: median %.6f max %.6f; %d points, %d verified matches, %.4f true' % (np.median(d), d.max(), keep.sum(), len(true), true.mean()))
    assert np.median(d) <= MEDIAN_SPHERE_DISTANCE and d.max() <= WORST_SPHERE_DISTANCE
    track_off = scene['tracks'][0]
    assert (err[keep] <= 2.0).all() and (np.add.reduceat(obs_keep, track_off[:-1])[keep] >= 2).all() and not obs_keep[np.repeat(~keep, np.diff(track_off))].any()


def test_matcher_rule_on_small_cases():
    s = np.zeros((1, 128), np.int8)
    t = np.zeros((3, 128), np.int8)
    t[0, 0], t[1, 0], t[2, 0] = 5, 3, 3                                              # D = 25, 9, 9: the lowest j of the tie wins, and D2 = D1 rejects
    j1, d1, d2 = R.nearest_two(s, t)
    assert (j1[0], d1[0], d2[0]) == (1, 9, 9)
    vo = np.array([0, 1, 4])
    assert len(R.match_descriptors(np.concatenate([s, t]), vo, mutual=False)[2]) == 0
    assert R.match_descriptors(np.concatenate([s, t]), vo, ratio=1.0, mutual=False)[2].tolist() == []      # 9 < 1 * 9 is false too
    m = R.match_descriptors(np.concatenate([s, t[:1]]), np.array([0, 1, 2]), mutual=False)                   # a single target: no D2, kept
    assert m[2].tolist() == [[0, 0]] and m[3].tolist() == [25]
    full = np.stack([np.full(128, 127, np.int8), np.zeros(128, np.int8)])
    assert R.match_descriptors(full, np.array([0, 1, 2]))[3].tolist() == [K.MVSDF_KP_MAX_DIST]
    assert R.match_descriptors(full, np.array([0, 1, 2]), max_dist=K.MVSDF_KP_MAX_DIST - 1)[3].tolist() == []


def test_fundamental_matrices_vanish_on_true_correspondences():
    cams, _ = S.make_cams(4, S.HW, S.FOCAL)
    rs = np.random.RandomState(3)
    pts = S.true_points(cams[1], np.stack([rs.uniform(20, 170, 50), rs.uniform(20, 100, 50)], 1))
    pairs = np.array([[0, 1], [0, 3], [2, 3]], np.int32)
    F = KP.fundamental_matrices(cams, pairs)
    for f, (a, b) in zip(F, pairs):
        xa, xb = (np.concatenate([S.project(cams[v], pts)[0], np.ones((50, 1))], 1) for v in (a, b))
        line = xa @ f.T
        assert (np.abs((xb * line).sum(1)) / np.linalg.norm(line[:, :2], axis=1) <= EPIPOLAR_ROUNDING).all()


def test_pure_x_translation_gives_the_row_difference_exactly():
    cams = S.axis_cameras()[[0, 4]]                                                  # identical intrinsics, a pure x translation
    F = KP.fundamental_matrices(cams, [(0, 1)])
    xy = np.array([[10.25, 20.5], [100.0, 64.0], [30.0, 23.75], [1.5, 64.0]])
    vo = np.array([0, 2, 4])
    m = (np.array([[0, 1]], np.int32), np.array([0, 2]), np.array([[0, 0], [1, 1]], np.int32), np.zeros(2, np.int32))
    assert R.verify_matches(xy, vo, m, F, 3.25)[2].tolist() == [[0, 0], [1, 1]]       # |dY| = 3.25 and 0
    assert R.verify_matches(xy, vo, m, F, 3.2499999)[2].tolist() == [[1, 1]]


def test_build_tracks_cases():
    vo, m, want = S.track_case()
    got = R.build_tracks(vo, m)
    assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))


def test_triangulate_tracks_cases():
    cams, xy, vo, tracks, max_reproj, (xyz, keep, obs_keep) = S.triangulation_case()
    got = R.triangulate_tracks(xy, vo, tracks, KP.camera_arrays(cams), max_reproj, 1.5)
    assert np.array_equal(got[2], keep) and np.array_equal(got[3], obs_keep)
    assert np.array_equal(got[0][[0, 1, 3]], xyz[[0, 1, 3]]) and np.array_equal(got[1][[0, 1, 3]], np.zeros(3))   # exact cameras, exact pixels: the point itself
    assert np.abs(got[0][4] - xyz[4]).max() <= 1e-12 and got[1][4] <= 1e-9
    wide = R.triangulate_tracks(xy, vo, tracks, KP.camera_arrays(cams), max_reproj, 0.1)
    assert wide[2][5] and np.abs(wide[0][5] - [0, 0, 4]).max() <= 1e-9               # 0.22 degrees passes a limit of 0.1


def test_concat_and_argument_checks():
    a = KP.make_keypoints(np.zeros((3, 2)), np.zeros((3, 128), np.int8), np.array([0, 1, 3]))
    b = KP.make_keypoints(np.ones((2, 2)), np.ones((2, 128), np.int8), np.array([0, 2]))
    c = KP.concat([a, b])
    assert c.view_off.tolist() == [0, 1, 3, 5] and c.xy.shape == (5, 2) and c.codes[3:].eq(1).all() and c.scale.shape == (5,)
    with pytest.raises(ValueError, match='codes'):
        KP.match_descriptors(a._replace(codes=torch.zeros(3, 128, dtype=torch.int16)))
    with pytest.raises(ValueError, match='view_off'):
        KP.match_descriptors(a._replace(view_off=torch.tensor([0, 2, 1])))
    with pytest.raises(ValueError, match='view_off'):
        KP.match_descriptors(a._replace(view_off=torch.tensor([0, 1, 3], dtype=torch.int32)))
    with pytest.raises(ValueError, match='codes'):
        KP.match_descriptors(a._replace(view_off=torch.tensor([0, 1, 4])))
    for pairs in ([[1, 0]], [[0, 2]], [[0, 0]]):
        with pytest.raises(ValueError, match='pair'):
            KP.match_descriptors(a, pairs=np.array(pairs, np.int32))
    with pytest.raises(ValueError, match='ratio'):
        KP.match_descriptors(a, ratio=0.0)
    with pytest.raises(ValueError, match='max_dist'):
        KP.match_descriptors(a, max_dist=-1)


# ================================================================ the scale space (restatement alone) ================================================================
# a level of a constant image: 12 blur passes of at most 21 taps, each product and sum rounded once, on values of one magnitude; DoG: twice that
CONSTANT_ROUNDING = 12 * 2 * 21 * 2.0 ** -53


def _space(img):
    return R.scale_space(img, [KP.blur_taps(s) for s in KP.level_sigmas()[1]], KP.octave_sizes(*img.shape[1:3]))


def test_octaves_and_taps():
    assert KP.octave_sizes(33, 47) == [(33, 47), (17, 24)] and KP.octave_sizes(15, 200) == [(15, 200)] and KP.octave_sizes(128, 192)[-1] == (16, 24)
    sig, inc = KP.level_sigmas()
    assert sig[0] == 1.6 and abs(sig[3] - 3.2) < 1e-15 and abs(inc[0] - np.sqrt(1.6 ** 2 - 0.25)) < 1e-15
    for s in inc:
        t = KP.blur_taps(s)
        assert len(t) == 2 * int(np.ceil(3 * s)) + 1 and abs(t.sum() - 1) < 1e-15 and np.array_equal(t, t[::-1]) and t.argmax() == len(t) // 2


def test_constant_image_and_ramp_have_no_structure():
    for L, D in _space(np.full((2, 40, 56), 200, np.uint8)):
        assert np.abs(L - 200.0).max() <= 200 * CONSTANT_ROUNDING and np.abs(D).max() <= 2 * 200 * CONSTANT_ROUNDING
    ramp = (np.arange(160, dtype=np.float32)[None, None, :] * 2 + np.arange(128, dtype=np.float32)[None, :, None])      # values up to 445
    D = _space(ramp)[0][1]
    # a symmetric normalised blur keeps a linear ramp wherever no clamped pixel is read: the six radii sum to 38
    assert np.abs(D[:, :, 40:-40, 40:-40]).max() <= 2 * 450 * CONSTANT_ROUNDING
    assert np.abs(D[:, :, :5, :]).max() > 1e-3                                        # (the clamped border is not linear: that is where structure appears)


def test_gaussian_blob_peaks_at_its_centre_and_scale():
    y, x = np.meshgrid(np.arange(64) + 0.5, np.arange(64) + 0.5, indexing='ij')
    blob = (200 * np.exp(-((x - 32.5) ** 2 + (y - 32.5) ** 2) / (2 * 3.0 ** 2))).astype(np.float32)[None]
    D = _space(blob)[0][1][0]
    s, py, px = np.unravel_index(np.argmax(np.abs(D)), D.shape)
    assert (py, px) == (32, 32) and D[s, py, px] < 0                                  # a bright blob is a minimum of the difference of Gaussians
    sig = KP.level_sigmas()[0]
    assert sig[s] <= 3.0 * 2 ** (1 / 3) and sig[s + 1] >= 3.0 / 2 ** (1 / 3)             # the level pair that brackets the blob's own sigma (within one interval)


# ================================================================ the extrema (restatement alone) ================================================================
# one blob of sigma 3 at a sub-pixel centre on 64 x 64: twice what the restatement measures
BLOB_POSITION_ERROR = 2 * 0.01432           # pixels; measured 0.01432 at the centre (30.3, 33.8)
BLOB_SCALE_RATIO_ERROR = 2 * 0.1534         # |scale / 3 - 1|; measured 0.1534: the scale is the level's sigma (2.54), not refined in s


def _extrema(img, **kw):
    sig, inc = KP.level_sigmas()
    return R.detect_extrema(img, [KP.blur_taps(s) for s in inc], KP.octave_sizes(*img.shape[1:3]), sig, **kw)


def test_one_blob_gives_one_keypoint_at_its_centre_and_scale():
    y, x = np.meshgrid(np.arange(64) + 0.5, np.arange(64) + 0.5, indexing='ij')
    for cx, cy in ((32.5, 32.5), (30.3, 33.8)):
        blob = (200 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * 3.0 ** 2))).astype(np.float32)[None]
        xy, scale, resp, site, vo = _extrema(blob)
        assert vo.tolist() == [0, 1] and site[0, 0] == 0
        err, ratio = float(np.hypot(xy[0, 0] - cx, xy[0, 1] - cy)), float(scale[0] / 3.0)
        print('blob at (%.1f, %.1f): position error %.5f, scale ratio %.4f, response %.3f' % (cx, cy, err, ratio, resp[0]))
        assert err <= BLOB_POSITION_ERROR and abs(ratio - 1) <= BLOB_SCALE_RATIO_ERROR and resp[0] > 2.0


def test_constant_image_and_ramp_give_no_keypoint():
    assert _extrema(np.full((2, 40, 56), 200, np.uint8))[4].tolist() == [0, 0, 0]
    ramp = (np.arange(160, dtype=np.float32)[None, None, :] * 2 + np.arange(128, dtype=np.float32)[None, :, None])
    assert _extrema(ramp)[4].tolist() == [0, 0]
    assert _extrema(np.ascontiguousarray(ramp[:, :11, :11]))[4].tolist() == [0, 0]     # one candidate site per level: the smallest image that has any


def test_rendered_scene_has_keypoints_in_every_view():
    cams, _ = S.make_cams(S.VIEWS, S.HW, S.FOCAL)
    images, _ = S.render(cams, S.HW, 0)
    xy, scale, resp, site, vo = _extrema(images)
    assert (np.diff(vo) >= 40).all()                                                  # the issue's cap for described keypoints; here: extrema
    assert (xy[:, 0] > 0).all() and (xy[:, 0] < S.HW[1]).all() and (xy[:, 1] > 0).all() and (xy[:, 1] < S.HW[0]).all() and (resp > 2.0).all()
    for v in range(S.VIEWS):                                                          # listed by (octave, level, y, x)
        k = site[vo[v]:vo[v + 1]].astype(np.int64)
        key = ((k[:, 0] * 8 + k[:, 1]) * 4096 + k[:, 2]) * 4096 + k[:, 3]
        assert (np.diff(key) > 0).all()


# ================================================================ the rendered scene, images to points (restatement alone) ================================================================
# distance of the points to the true sphere on the rendered scene (4 views, 128 x 192, focal 300, seed 0, defaults): twice the measured
RENDERED_MEDIAN_SPHERE_DISTANCE = 2 * 0.0037267     # measured 0.0037267
RENDERED_WORST_SPHERE_DISTANCE = 2 * 0.05918        # measured 0.0591832


@functools.lru_cache(maxsize=None)
def _rendered():
    """the rendered scene and the restatement's keypoints of it, computed once for the tests below (nothing changes them)"""
    cams, _ = S.make_cams(S.VIEWS, S.HW, S.FOCAL)
    images, _ = S.render(cams, S.HW, 0)
    sig, inc = KP.level_sigmas()
    tables = ([KP.blur_taps(s) for s in inc], KP.octave_sizes(*S.HW), sig) + KP.descriptor_tables()
    return cams, images, tables, R.detect(images, *tables)


def test_rendered_scene_from_images_to_points():
    cams, images, tables, (xy, scale, angle, resp, codes, vo) = _rendered()
    assert (np.diff(vo) >= 40).all() and codes.min() >= 0 and (angle >= 0).all() and (angle < 2 * np.pi).all()      # every view has >= 40 described keypoints
    m = R.match_descriptors(codes, vo)
    v = R.verify_matches(xy, vo, m, KP.fundamental_matrices(cams, m[0]))
    assert (np.diff(v[1]) >= 25).all()                                                # every pair has >= 25 verified matches
    ga, gb = _globals(vo, v)
    truth = np.concatenate([S.true_points(cams[a], xy[vo[a]:vo[a + 1]]) for a in range(S.VIEWS)])
    footprint = 3.0 / S.FOCAL                                                         # a pixel's footprint at the scene's depth of about 3
    true = np.linalg.norm(truth[ga] - truth[gb], axis=1) <= 3 * footprint
    assert true.mean() >= 0.9                                                         # >= 90 % of the verified matches are true (3 footprints)
    tracks = R.build_tracks(vo, v)
    xyz, err, keep, obs_keep = R.triangulate_tracks(xy, vo, tracks, KP.camera_arrays(cams))
    assert keep.sum() >= 60                                                           # >= 60 points
    d = np.abs(np.linalg.norm(xyz[keep] - S.CENTER, axis=1) - S.RADIUS)
    print('rendered scene: keypoints %s, verified %s, %.4f true, %d points, sphere distance median %.7f max %.7f'
          % (np.diff(vo).tolist(), np.diff(v[1]).tolist(), true.mean(), keep.sum(), np.median(d), d.max()))
    assert np.median(d) <= RENDERED_MEDIAN_SPHERE_DISTANCE and d.max() <= RENDERED_WORST_SPHERE_DISTANCE


def test_orientation_follows_a_quarter_turn():
    """the scene image and its np.rot90: with ratio + mutual matching, at least 30 matches, at least 0.9 of them within 1.5 px of the turned position"""
    cams, images, tables, kp = _rendered()
    image = images[:1]
    turned = np.ascontiguousarray(np.rot90(image[0]))[None]
    a = tuple(f[:kp[5][1]] for f in kp[:5])                                            # view 0 of the scene: detection is per view
    b = R.detect(turned, tables[0], KP.octave_sizes(*turned.shape[1:3]), *tables[2:])
    m = R.match_descriptors(np.concatenate([a[4], b[4]]), np.array([0, len(a[0]), len(a[0]) + len(b[0])]), ratio=0.8, mutual=True)
    pa, pb = a[0][m[2][:, 0]], b[0][m[2][:, 1]]
    d = np.linalg.norm(pb - np.stack([pa[:, 1], image.shape[2] - pa[:, 0]], 1), axis=1)       # np.rot90: (X, Y) -> (Y, W - X)
    print('rot90: %d matches, %.4f within 1.5 px' % (len(d), (d <= 1.5).mean()))
    assert len(d) >= 30 and (d <= 1.5).mean() >= 0.9


def test_trig_table_is_sine_and_cosine():
    t = KP.trig_table()
    assert np.array_equal(t, R.trig_table()) and len(t) == K.MVSDF_KP_TRIG_WORDS
    u = np.linspace(-np.pi, np.pi, 1001)
    z = u * u
    ps, pc = np.full(u.shape, t[13]), np.full(u.shape, t[28])
    for k in range(12, -1, -1):
        ps = ps * z + t[k]
    for k in range(13, -1, -1):
        pc = pc * z + t[14 + k]
    # the truncation at u = pi: pi^29 / 29! = 3e-17 and pi^30 / 30! = 3e-18; Horner's rounding on terms that reach pi^4 / 4! = 4: 30 steps of 2^-53 * 12
    assert np.abs(u * ps - np.sin(u)).max() <= 30 * 12 * 2.0 ** -53 and np.abs(pc - np.cos(u)).max() <= 30 * 12 * 2.0 ** -53


def test_sparse_model_round_trips_through_colmap_text(tmp_path):
    """the host-side assembly (keypoints.assemble_model) of the restatement's sparse points -> write_colmap_text -> load_colmap_model: the same bits"""
    from colmap_scene import assert_models_equal, quaternion
    from mvsdf_amd.datasets.colmap import _points, load_colmap_model, write_colmap_text
    cams, images, tables, kp = _rendered()
    xyz, rgb, err, off, tv, tk, _ = R.sparse_points(images, cams, tables, KP.camera_arrays(cams), lambda p: KP.fundamental_matrices(cams, p), keypoints=kp)
    ids = [3, 5, 7, 9]
    model = {'cameras': {1: {'model': 'PINHOLE', 'width': S.HW[1], 'height': S.HW[0], 'params': np.array([S.FOCAL, S.FOCAL, S.HW[1] / 2.0, S.HW[0] / 2.0])}},
             'images': {i: {'q': quaternion(cams[v, 0, :3, :3]), 't': cams[v, 0, :3, 3], 'camera_id': 1, 'name': 'view_%d.png' % v, 'xys': np.zeros((0, 2)),
                            'point3D_ids': np.zeros(0, np.int64)} for v, i in enumerate(ids)}, 'points': _points([], [], [], [], [0], [], [])}
    full = KP.assemble_model(model, ids, kp[0], kp[5], xyz, rgb, err, off, tv, tk)
    assert len(full['points']['ids']) == len(xyz) >= 60 and full['points']['ids'][0] == 1
    for v, i in enumerate(ids):
        im = full['images'][i]
        assert len(im['xys']) == kp[5][v + 1] - kp[5][v] and (im['point3D_ids'] >= 1).sum() == (tv == v).sum() and im['point3D_ids'].min() == -1
    k = 7                                                                              # a track entry points back at its point
    q = off[k]
    assert full['images'][ids[tv[q]]]['point3D_ids'][tk[q]] == k + 1 and full['points']['track_image'][q] == ids[tv[q]]
    write_colmap_text(full, str(tmp_path / 'm'))
    assert_models_equal(load_colmap_model(str(tmp_path / 'm')), full)
