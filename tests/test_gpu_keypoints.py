"""mvsdf_amd/keypoints.py on the GPU against its numpy restatement (tests/keypoints_ref.py): matches, distances, offsets, tracks and flags are
compared as integers, points and errors bit for bit (uint64 views of fp64)."""
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

pytestmark = pytest.mark.gpu
SIZES = (1, 15, 16, 17, 63, 257, 1031)


def np_(t):
    return t.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(np.asarray(a, np.float64)), np.ascontiguousarray(np.asarray(b, np.float64))
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def kp_of(codes, view_off, xy=None):
    n = len(codes)
    return KP.make_keypoints(np.zeros((n, 2)) if xy is None else xy, np.ascontiguousarray(codes, dtype=np.int8), np.asarray(view_off, np.int64))


def assert_matches(got, want, tag=''):
    assert got.pair.dtype == torch.int32 and got.off.dtype == torch.int64 and got.idx.dtype == torch.int32 and got.dist.dtype == torch.int32
    assert np.array_equal(np_(got.pair), want[0]), tag
    assert np.array_equal(np_(got.off), want[1]), (tag, np_(got.off), want[1])
    assert np.array_equal(np_(got.idx), want[2]), (tag, int((np_(got.idx) != want[2]).any(1).sum()))
    assert np.array_equal(np_(got.dist), want[3]), tag


def check_match(codes, vo, tag, **kw):
    want = R.match_descriptors(codes, vo, **kw)
    assert_matches(KP.match_descriptors(kp_of(codes, vo), **kw), want, tag)
    return want


# ================================================================ the scale space ================================================================
def _images(V, hw, dtype, channels, seed):
    rs = np.random.RandomState(seed)
    shape = (V,) + hw + ((3,) if channels == 3 else ())
    smooth = np.sin(np.arange(hw[1])[None, :] * 0.31) * np.cos(np.arange(hw[0])[:, None] * 0.23) * 60 + 128
    base = smooth[None, :, :, None] if channels == 3 else smooth[None]
    img = np.clip(base + rs.normal(scale=25, size=shape), 0, 255)
    return np.rint(img).astype(np.uint8) if dtype == np.uint8 else (img / 255.0).astype(np.float32)


@pytest.mark.parametrize('hw', [(33, 47), (64, 96), (128, 192)])
def test_scale_space_equals_the_restatement(hw):
    """33 x 47 is odd and its second octave (17 x 24) is narrower than the widest blur (21 taps); every level and every difference, bit for bit"""
    taps = [KP.blur_taps(s) for s in KP.level_sigmas()[1]]
    sizes = KP.octave_sizes(*hw)
    assert len(sizes) == {33: 2, 64: 3, 128: 4}[hw[0]]
    for V, dtype, channels in ((1, np.uint8, 3), (3, np.float32, 1), (3, np.uint8, 1), (1, np.float32, 3)):
        img = _images(V, hw, dtype, channels, V + channels)
        want = R.scale_space(img, taps, sizes)
        got = KP.scale_space(img)
        assert len(got) == len(want)
        for (L, D), (wl, wd) in zip(got, want):
            assert L.dtype == torch.float64 and tuple(L.shape) == wl.shape and tuple(D.shape) == wd.shape
            assert same_bits(np_(L), wl), (hw, V, dtype, channels, np.abs(np_(L) - wl).max())
            assert same_bits(np_(D), wd)
    flat = KP.scale_space(np.full((1,) + hw, 7, np.uint8))
    assert all(same_bits(np_(D), wd) for (_, D), (_, wd) in zip(flat, R.scale_space(np.full((1,) + hw, 7, np.uint8), taps, sizes)))


@pytest.mark.parametrize('hw', [(33, 47), (64, 96), (128, 192)])
def test_extrema_equal_the_restatement(hw):
    sig, inc = KP.level_sigmas()
    taps, sizes = [KP.blur_taps(s) for s in inc], KP.octave_sizes(*hw)
    total = 0
    for V, dtype, channels, contrast, edge in ((1, np.uint8, 3, 2.0, 10), (3, np.float32, 1, 0.002, 10), (3, np.uint8, 1, 0.5, 3), (1, np.float32, 3, 0.0, 40)):
        img = _images(V, hw, dtype, channels, 10 + V + channels)
        want = R.detect_extrema(img, taps, sizes, sig, contrast, edge)
        got = KP.detect_extrema(img, contrast, edge)
        assert got.site.dtype == torch.int32 and got.view_off.dtype == torch.int64
        assert np.array_equal(np_(got.view_off), want[4]) and np.array_equal(np_(got.site), want[3]), (hw, V, np_(got.view_off), want[4])
        assert same_bits(np_(got.xy), want[0]) and same_bits(np_(got.scale), want[1]) and same_bits(np_(got.response), want[2])
        total += len(want[1])
    assert total > 20
    flat = KP.detect_extrema(np.full((2,) + hw, 7, np.uint8))
    assert np_(flat.view_off).tolist() == [0, 0, 0] and flat.xy.shape == (0, 2) and flat.site.shape == (0, 4)


def test_extrema_on_the_rendered_scene():
    cams, _ = S.make_cams(S.VIEWS, S.HW, S.FOCAL)
    images, _ = S.render(cams, S.HW, 0)
    sig, inc = KP.level_sigmas()
    want = R.detect_extrema(images, [KP.blur_taps(s) for s in inc], KP.octave_sizes(*S.HW), sig)
    got = KP.detect_extrema(images)
    assert np.array_equal(np_(got.view_off), want[4]) and (np.diff(want[4]) >= 40).all() and np.array_equal(np_(got.site), want[3])
    assert same_bits(np_(got.xy), want[0]) and same_bits(np_(got.scale), want[1]) and same_bits(np_(got.response), want[2])


def _detect_ref(img, **kw):
    sig, inc = KP.level_sigmas()
    return R.detect(img, [KP.blur_taps(s) for s in inc], KP.octave_sizes(*img.shape[1:3]), sig, *KP.descriptor_tables(), **kw)


def assert_keypoints(got, want, tag=''):
    assert got.codes.dtype == torch.int8 and got.view_off.dtype == torch.int64 and got.xy.dtype == torch.float64
    assert np.array_equal(np_(got.view_off), want[5]), (tag, np_(got.view_off), want[5])
    assert same_bits(np_(got.angle), want[2]), (tag, int((np_(got.angle) != want[2]).sum()), len(want[2]))
    assert np.array_equal(np_(got.codes), want[4]), (tag, int((np_(got.codes) != want[4]).any(1).sum()), len(want[4]))
    for g, w in zip(got[:4], want[:4]):
        assert same_bits(np_(g), w), tag


COMBOS = [(1, np.uint8, 3, 1.0), (3, np.float32, 1, 0.002), (3, np.uint8, 1, 0.5), (1, np.float32, 3, 0.004)]


@pytest.mark.parametrize('combo', range(len(COMBOS)))
@pytest.mark.parametrize('hw', [(33, 47), (64, 96), (128, 192)])
def test_detect_equals_the_restatement(hw, combo):
    """positions, scales, angles, responses, every code and the order, bit for bit; max_keypoints below the count (1 and 17); upright"""
    V, dtype, channels, contrast = COMBOS[combo]
    img = _images(V, hw, dtype, channels, 20 + V + channels)
    want = _detect_ref(img, contrast=contrast)
    assert_keypoints(KP.detect(img, contrast=contrast), want, (hw, V, channels))
    assert (np.diff(want[5]) > (17 if hw[0] >= 64 else 1)).all() and len(np.unique(want[2])) > len(want[2]) // 2      # the caps bite; the angles differ
    for cap in (1, 17):
        capped = R.cap_keypoints(want, cap)
        assert np.diff(capped[5]).tolist() == np.minimum(cap, np.diff(want[5])).tolist()
        assert_keypoints(KP.detect(img, max_keypoints=cap, contrast=contrast), capped, (hw, V, cap))
    if combo == 0:
        up = _detect_ref(img, contrast=contrast, upright=True)
        assert (up[2] == 0).all() and not np.array_equal(up[4], want[4])
        assert_keypoints(KP.detect(img, contrast=contrast, upright=True), up, (hw, 'upright'))
        flat = KP.detect(np.full((3,) + hw, 7, np.uint8))
        assert np_(flat.view_off).tolist() == [0, 0, 0, 0] and flat.codes.shape == (0, 128)


def test_rendered_scene_from_images_to_points():
    """the whole chain on the rendered scene (4 views, 128 x 192, focal 300, seed 0): every stage equals the restatement, and the issue's caps hold"""
    cams, _ = S.make_cams(S.VIEWS, S.HW, S.FOCAL)
    images, _ = S.render(cams, S.HW, 0)
    want = _detect_ref(images)
    kp = KP.detect(images)
    assert_keypoints(kp, want, 'scene')
    xy, vo = want[0], want[5]
    assert (np.diff(vo) >= 40).all()
    wm = R.match_descriptors(want[4], vo)
    wv = R.verify_matches(xy, vo, wm, KP.fundamental_matrices(cams, wm[0]))
    wt = R.build_tracks(vo, wv)
    wp = R.triangulate_tracks(xy, vo, wt, KP.camera_arrays(cams))
    m = KP.match_descriptors(kp)
    assert_matches(m, wm, 'scene')
    v = KP.verify_matches(kp, m, cams)
    assert_matches(v, wv, 'scene')
    t = KP.build_tracks(kp, v)
    assert_tracks(t, wt, 'scene')
    assert_triangulation(KP.triangulate_tracks(kp, t, cams), wp, 'scene')
    assert (np.diff(wv[1]) >= 25).all() and wp[2].sum() >= 60


def test_sparse_points_on_the_scene_and_into_view_selection():
    """every field equals the restatement; differing sizes go through separate detections; the tracks feed view selection: adjacent cameras first"""
    from mvsdf_amd import viewsel
    cams, _ = S.make_cams(S.VIEWS, S.HW, S.FOCAL)
    images, _ = S.render(cams, S.HW, 0)
    sig, inc = KP.level_sigmas()
    tables = ([KP.blur_taps(s) for s in inc], KP.octave_sizes(*S.HW), sig) + KP.descriptor_tables()
    want = R.sparse_points(images, cams, tables, KP.camera_arrays(cams), lambda p: KP.fundamental_matrices(cams, p))
    rep = {}
    got = KP.sparse_points(images, cams, report=rep)
    assert rep['views'] == 4 and rep['points'] == len(want[0]) and rep['keypoints'] == want[6][5][-1] and rep['matches'] >= rep['verified'] >= rep['tracks']
    assert same_bits(np_(got.xyz), want[0]) and same_bits(np_(got.error), want[2]) and np.array_equal(np_(got.rgb), want[1]) and got.rgb.dtype == torch.uint8
    assert np.array_equal(np_(got.track_off), want[3]) and np.array_equal(np_(got.track_view), want[4]) and np.array_equal(np_(got.track_kp), want[5])
    assert_keypoints(got.keypoints, want[6], 'sparse_points')
    assert len(want[0]) >= 60 and (np.diff(want[3]) >= 2).all()
    as_list = KP.sparse_points([images[0], images[1], images[2], images[3]], cams)           # a list of views: the same result
    assert same_bits(np_(as_list.xyz), want[0]) and np.array_equal(np_(as_list.track_kp), want[5])
    scores, _ = viewsel.view_scores(got.xyz, viewsel.centers_from_cams(cams), (got.track_off, got.track_view))
    assert all(abs(int(b) - v) == 1 for v, b in enumerate(np.argmax(np_(scores), 1)))
    ranges = viewsel.depth_ranges(got.xyz, (got.track_off, got.track_view), cams[:, 0])
    r = np.asarray(ranges.cpu() if isinstance(ranges, torch.Tensor) else ranges)
    from stereo_scene import DEPTH_MAX, DEPTH_MIN
    assert (r[:, 0] >= DEPTH_MIN).all() and (r[:, 1] <= DEPTH_MAX).all() and (r[:, 0] < r[:, 1]).all()      # inside the scene's true depth range


def _scene_model(cams):
    from colmap_scene import quaternion
    h, w = S.HW
    cameras = {1: {'model': 'PINHOLE', 'width': w, 'height': h, 'params': np.array([cams[0, 1, 0, 0], cams[0, 1, 1, 1], cams[0, 1, 0, 2], cams[0, 1, 1, 2]])}}
    images = {3 + 2 * v: {'q': quaternion(cams[v, 0, :3, :3]), 't': cams[v, 0, :3, 3].copy(), 'camera_id': 1, 'name': 'view_%d.png' % v,
                          'xys': np.zeros((0, 2)), 'point3D_ids': np.zeros(0, np.int64)} for v in range(len(cams))}
    from mvsdf_amd.datasets.colmap import _points
    return {'cameras': cameras, 'images': images, 'points': _points([], [], [], [], [0], [], [])}


def _first_sources(pair_file):
    words = open(pair_file).read().split('\n')
    return [(int(words[1 + 2 * i]), int(words[2 + 2 * i].split()[1])) for i in range(int(words[0]))]


def test_sparse_model_through_colmap_files_into_mvs_input(tmp_path):
    """a posed model without points -> sparse_model -> write_colmap_text -> load_colmap_model (the same bits) -> colmap_to_mvs: each view's first
    source is an adjacent camera and its depth range lies inside the scene's; colmap_to_mvs(triangulate=True) and both forms of the command agree"""
    import importlib.util
    from PIL import Image
    from colmap_scene import assert_models_equal
    from mvsdf_amd.datasets.colmap import colmap_to_mvs, load_colmap_model, rotation, write_colmap_text
    from mvsdf_amd.utils.io import load_cam
    from stereo_scene import DEPTH_MAX, DEPTH_MIN, write_cam
    cams, _ = S.make_cams(S.VIEWS, S.HW, S.FOCAL)
    images, _ = S.render(cams, S.HW, 0)
    model = _scene_model(cams)
    for v in range(S.VIEWS):                                      # the poses the model really holds (a quaternion round trip of the rotation)
        cams[v, 0, :3, :3] = rotation(model['images'][3 + 2 * v]['q'])
    img_dir, posed, out_model = tmp_path / 'images', tmp_path / 'posed', tmp_path / 'sparse'
    img_dir.mkdir()
    for v in range(S.VIEWS):
        Image.fromarray(images[v]).save(img_dir / ('view_%d.png' % v))
    write_colmap_text(model, str(posed))
    rep = {}
    full = KP.sparse_model(load_colmap_model(str(posed)), str(img_dir), report=rep)
    want = KP.sparse_points(images, cams)
    assert np.array_equal(full['points']['xyz'], np_(want.xyz)) and rep['points'] == len(want.xyz) >= 60
    assert np.array_equal(full['images'][5]['xys'], np_(want.keypoints.xy)[want.keypoints.view_off[1]:want.keypoints.view_off[2]])
    assert (full['images'][5]['point3D_ids'] >= 1).sum() == int((np_(want.track_view) == 1).sum()) and set(full['points']['track_image'].tolist()) == {3, 5, 7, 9}
    write_colmap_text(full, str(out_model))
    assert_models_equal(load_colmap_model(str(out_model)), full)
    res = colmap_to_mvs(str(out_model), str(img_dir), str(tmp_path / 'mvs'), max_d=32, num_pairs=3)
    assert all(abs(src - ref) == 1 for ref, src in _first_sources(tmp_path / 'mvs' / 'pair.txt'))
    d = res['cams'][:, 1, 3]
    assert (d[:, 0] >= DEPTH_MIN).all() and (d[:, 3] <= DEPTH_MAX).all() and (d[:, 0] < d[:, 3]).all()
    tri = colmap_to_mvs(str(posed), str(img_dir), str(tmp_path / 'mvs_tri'), max_d=32, num_pairs=3, triangulate=True)
    assert np.array_equal(tri['cams'], res['cams']) and tri['pairs'] == res['pairs']
    with pytest.raises(ValueError, match='undistort'):
        colmap_to_mvs(str(posed), str(img_dir), str(tmp_path / 'no'), triangulate=True, undistort=True)
    spec = importlib.util.spec_from_file_location('sparse_points_tool', os.path.join(os.path.dirname(__file__), '..', 'tools', 'sparse_points.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = tool.main([str(posed), str(img_dir), str(tmp_path / 'sparse_tool')])
    assert_models_equal(load_colmap_model(str(tmp_path / 'sparse_tool')), full)
    assert out['report'] == rep
    byod = tmp_path / 'byod'
    (byod / 'images').mkdir(parents=True)
    (byod / 'cams').mkdir()
    for v in range(S.VIEWS):
        Image.fromarray(images[v]).save(byod / 'images' / ('%08d.png' % (3 * v + 4)))
        write_cam(str(byod / 'cams' / ('%08d_cam.txt' % (3 * v + 4))), cams[v])
    before = sorted(os.listdir(byod / 'cams'))
    tool.main(['--mvs_dir', str(byod), '--out', str(tmp_path / 'byod_out'), '--max_d', '32', '--num_pairs', '3'])
    assert sorted(os.listdir(byod / 'cams')) == before and not (byod / 'pair.txt').exists()
    assert all(abs(src - ref) == 3 for ref, src in _first_sources(tmp_path / 'byod_out' / 'pair.txt'))
    got = np.stack([load_cam(str(tmp_path / 'byod_out' / 'cams' / ('%08d_cam.txt' % (3 * v + 4))), 32) for v in range(S.VIEWS)])
    assert np.array_equal(got[:, 1, 3, [0, 3]], d[:, [0, 3]]) and np.array_equal(got[:, 0], cams[:, 0])
    with pytest.raises(ValueError, match='--out must differ'):
        tool.main(['--mvs_dir', str(byod), '--out', str(byod)])


# ================================================================ the matcher ================================================================
@pytest.mark.parametrize('ns', SIZES)
def test_matcher_equals_the_restatement_at_every_size(ns):
    """random codes, sizes crosswise; a narrow code range makes equal distances common, so the order (D, j) and the D2 = D1 rejections are exercised"""
    for nt in SIZES:
        rs = np.random.RandomState(1000 * ns + nt)
        wide = rs.randint(0, 128, size=(ns + nt, 128))
        narrow = rs.randint(0, 2, size=(ns + nt, 128)) * (rs.uniform(size=(1, 128)) < 0.06)
        for name, codes in (('wide', wide), ('narrow', narrow)):
            for mutual in (False, True):
                check_match(codes, [0, ns, ns + nt], (name, ns, nt, mutual), ratio=0.95, mutual=mutual)
    check_match(wide, [0, ns, ns + nt], ('max_dist', ns), ratio=1.0, mutual=False, max_dist=int(np.median(R.nearest_two(wide[:ns], wide[ns:])[1])))


def test_matcher_extremes_ties_and_single_targets():
    full = np.stack([np.full(128, 127), np.zeros(128, int)])
    m = KP.match_descriptors(kp_of(full, [0, 1, 2]))
    assert np_(m.dist).tolist() == [K.MVSDF_KP_MAX_DIST] and np_(m.idx).tolist() == [[0, 0]]                  # one target: no D2
    assert np_(KP.match_descriptors(kp_of(full, [0, 1, 2]), max_dist=K.MVSDF_KP_MAX_DIST - 1).off).tolist() == [0, 0]
    rs = np.random.RandomState(5)
    t = rs.randint(0, 128, size=(40, 128))
    s = np.clip(t[[7, 21, 33]] + rs.randint(-2, 3, size=(3, 128)), 0, 127)
    dup = np.concatenate([t, t[[21]]])                                                                             # target 21 again as target 40
    want = check_match(np.concatenate([s, dup]), [0, 3, 44], 'dup', ratio=0.8, mutual=False)
    assert want[2].tolist() == [[0, 7], [2, 33]]                                                                   # the duplicated nearest row: D2 = D1, rejected
    want = check_match(np.concatenate([s, dup]), [0, 3, 44], 'dup1', ratio=1.0, mutual=False, max_dist=None)
    assert want[2].tolist() == [[0, 7], [2, 33]]                                                                   # (strict: D1 < 1 * D2 fails too)
    # the lowest index of equal distances: a tie for the best is always rejected (D2 = D1), so the rule shows in the search back from b, where
    # sources 0 and 2 are the same row: target 21 answers to source 0, and only (0, 21) is mutual
    twins = np.concatenate([s[[1]], t[[5]], s[[1]]])
    for mutual, rows in ((True, [[0, 21], [1, 5]]), (False, [[0, 21], [1, 5], [2, 21]])):
        want = check_match(np.concatenate([twins, t]), [0, 3, 43], ('twins', mutual), ratio=0.8, mutual=mutual)
        assert want[2].tolist() == rows


def test_matcher_operand_map_asymmetric():
    """sources one-hot in a different column each, targets distinct rolled ramps: D(i,j) = |t_j|^2 + 127^2 - 2 * 127 * t_j[i] reads one byte of one target, over all
    128 columns (both k-steps); exchanged rows and columns or a permuted k give another table"""
    s = np.eye(128, dtype=int) * 127
    ramp = np.random.RandomState(7).permutation(128)
    t = ramp[(np.arange(128)[None, :] + 3 * np.arange(37)[:, None]) % 128]          # distinct rows of one norm: the nearest target of source i is argmax_j t_j[i]
    assert len(set(R.nearest_two(s, t)[0].tolist())) > 20
    for ratio in (1.0, 0.999):
        check_match(np.concatenate([s, t]), [0, 128, 165], 'one-hot sources', ratio=ratio, mutual=False)
        check_match(np.concatenate([t, s]), [0, 37, 165], 'one-hot targets', ratio=ratio, mutual=False)


def test_matcher_splits_and_batches():
    rs = np.random.RandomState(11)
    codes = rs.randint(0, 128, size=(5 + 3000, 128))
    vo = np.array([0, 5, 3005], np.int64)
    assert KP.match_splits(vo, [[0, 1]]) > 1                                          # few sources, many targets: the per-split merge runs
    codes[5 + 2999] = codes[5 + 17]                                                   # a nearest row repeated in another split
    codes[0] = np.clip(codes[5 + 17] + 1, 0, 127)
    for mutual in (False, True):
        check_match(codes, vo, ('split', mutual), ratio=0.9, mutual=mutual)
    # three views with 0, 40 and 300 keypoints, all pairs in one call = pair by pair
    vo3 = np.array([0, 0, 40, 340], np.int64)
    c3 = rs.randint(0, 8, size=(340, 128)) * 16
    kp = kp_of(c3, vo3)
    for mutual in (False, True):
        allp = KP.match_descriptors(kp, ratio=0.97, mutual=mutual)
        assert_matches(allp, R.match_descriptors(c3, vo3, ratio=0.97, mutual=mutual), 'batched')
        off, idx, dist = [0], [], []
        for a, b in ((0, 1), (0, 2), (1, 2)):
            one = KP.match_descriptors(kp, pairs=np.array([[a, b]], np.int32), ratio=0.97, mutual=mutual)
            off.append(off[-1] + one.idx.shape[0])
            idx.append(np_(one.idx))
            dist.append(np_(one.dist))
        assert np_(allp.off).tolist() == off and np.array_equal(np_(allp.idx), np.concatenate(idx)) and np.array_equal(np_(allp.dist), np.concatenate(dist))
        assert off[1] == 0 and off[2] == 0 and off[3] > 0
    empty = KP.match_descriptors(kp_of(c3[:0], [0, 0, 0]))
    assert np_(empty.off).tolist() == [0, 0] and empty.idx.shape == (0, 2)


def test_matcher_refuses_negative_codes():
    codes = np.zeros((20, 128), int)
    codes[13, 77] = -3
    with pytest.raises(ValueError, match='code'):
        KP.match_descriptors(kp_of(codes, [0, 10, 20]))


# ================================================================ verification, tracks, triangulation ================================================================
@pytest.fixture(scope='module')
def scene():
    cams, xy, codes, vo, point, pts = S.synthetic_keypoints()
    m = R.match_descriptors(codes, vo)
    v = R.verify_matches(xy, vo, m, KP.fundamental_matrices(cams, m[0]))
    tracks = R.build_tracks(vo, v)
    return dict(cams=cams, kp=kp_of(codes, vo, xy), xy=xy, vo=vo, matches=m, verified=v, tracks=tracks)


def as_matches(m):
    return KP.Matches(*(torch.from_numpy(np.ascontiguousarray(x)) for x in m))


def test_verify_equals_the_restatement(scene):
    assert len(scene['verified'][2]) < len(scene['matches'][2])
    for limit in (2.0, 0.5, 0.0):
        want = R.verify_matches(scene['xy'], scene['vo'], scene['matches'], KP.fundamental_matrices(scene['cams'], scene['matches'][0]), limit)
        assert_matches(KP.verify_matches(scene['kp'], as_matches(scene['matches']), scene['cams'], limit), want, limit)
    got = KP.verify_matches(scene['kp'], KP.match_descriptors(scene['kp']), scene['cams'])                  # device results handed on as they are
    assert_matches(got, scene['verified'], 'chained')


def test_verify_pure_x_translation_is_the_row_difference():
    cams = S.axis_cameras()[[0, 4]]
    xy = np.array([[10.25, 20.5], [100.0, 64.0], [30.0, 23.75], [1.5, 64.0]])
    kp = kp_of(np.zeros((4, 128), int), [0, 2, 4], xy)
    m = as_matches((np.array([[0, 1]], np.int32), np.array([0, 2]), np.array([[0, 0], [1, 1]], np.int32), np.zeros(2, np.int32)))
    assert np_(KP.verify_matches(kp, m, cams, 3.25).idx).tolist() == [[0, 0], [1, 1]]
    assert np_(KP.verify_matches(kp, m, cams, 3.2499999).idx).tolist() == [[1, 1]]
    bad = m._replace(idx=torch.tensor([[0, 0], [1, 2]], dtype=torch.int32))
    with pytest.raises(ValueError, match='index'):
        KP.verify_matches(kp, bad, cams, 1.0)


def assert_tracks(got, want, tag=''):
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.int32 and got[2].dtype == torch.int32
    for g, w in zip(got, want):
        assert np.array_equal(np_(g), w), (tag, np_(g)[:20], w[:20])


def test_build_tracks_cases_scene_and_random_lists(scene):
    vo, m, want = S.track_case()
    assert_tracks(KP.build_tracks(kp_of(np.zeros((12, 128), int), vo), as_matches(m)), want, 'case')
    assert_tracks(KP.build_tracks(scene['kp'], as_matches(scene['verified'])), scene['tracks'], 'scene')
    pairs = np.array([(a, b) for a in range(5) for b in range(a + 1, 5)], np.int32)
    vo5 = np.arange(6, dtype=np.int64) * 50
    kp5 = kp_of(np.zeros((250, 128), int), vo5)
    for seed, per_pair in ((0, 12), (1, 30), (2, 80)):                               # sparse, mixed, and mostly conflicting components
        rs = np.random.RandomState(seed)
        idx = rs.randint(0, 50, size=(len(pairs) * per_pair, 2)).astype(np.int32)
        m5 = (pairs, np.arange(len(pairs) + 1, dtype=np.int64) * per_pair, idx, np.zeros(len(idx), np.int32))
        want5 = R.build_tracks(vo5, m5)
        assert_tracks(KP.build_tracks(kp5, as_matches(m5)), want5, seed)
    assert len(want5[0]) - 1 < 5                                                      # (the dense list leaves almost no track)
    # a chain of 250 nodes across the views needs many rounds: the limit is reported, the default is enough
    chain_pairs = np.array([[0, 1]], np.int32)
    kpc = kp_of(np.zeros((600, 128), int), [0, 300, 600])
    i = np.arange(299, dtype=np.int32)
    idxc = np.concatenate([np.stack([i, i], 1), np.stack([i + 1, i], 1)])              # a_i - b_i - a_(i+1): one component of 599 nodes
    mc = (chain_pairs, np.array([0, len(idxc)]), idxc, np.zeros(len(idxc), np.int32))
    assert_tracks(KP.build_tracks(kpc, as_matches(mc)), R.build_tracks(np.array([0, 300, 600]), mc), 'chain')
    with pytest.raises(ValueError, match='round limit'):
        KP.build_tracks(kpc, as_matches(mc), max_rounds=1)


def assert_triangulation(got, want, tag=''):
    assert got[0].dtype == torch.float64 and got[2].dtype == torch.bool and got[3].dtype == torch.bool
    assert np.array_equal(np_(got[2]), want[2]) and np.array_equal(np_(got[3]), want[3]), tag
    assert same_bits(np_(got[0]), want[0]) and same_bits(np_(got[1]), want[1]), (tag, np.abs(np_(got[0]) - want[0]).max())


def test_triangulate_cases_and_scene(scene):
    cams, xy, vo, tracks, max_reproj, (xyz, keep, obs_keep) = S.triangulation_case()
    kp = kp_of(np.zeros((len(xy), 128), int), vo, xy)
    tt = tuple(torch.from_numpy(t) for t in tracks)
    for min_angle in (1.5, 0.1):
        want = R.triangulate_tracks(xy, vo, tracks, KP.camera_arrays(cams), max_reproj, min_angle)
        got = KP.triangulate_tracks(kp, tt, cams, max_reproj, min_angle)
        assert_triangulation(got, want, min_angle)
    got = KP.triangulate_tracks(kp, tt, cams, max_reproj, 1.5)
    assert np.array_equal(np_(got[2]), keep) and np.array_equal(np_(got[3]), obs_keep) and np.array_equal(np_(got[0])[[0, 1, 3]], xyz[[0, 1, 3]])
    for max_reproj, min_angle in ((2.0, 1.5), (0.4, 1.5), (2.0, 25.0)):               # the one refit and the angle test both decide on the scene
        want = R.triangulate_tracks(scene['xy'], scene['vo'], scene['tracks'], KP.camera_arrays(scene['cams']), max_reproj, min_angle)
        got = KP.triangulate_tracks(scene['kp'], tuple(torch.from_numpy(t) for t in scene['tracks']), scene['cams'], max_reproj, min_angle)
        assert_triangulation(got, want, (max_reproj, min_angle))
        assert 0 < want[2].sum() and ((max_reproj, min_angle) == (2.0, 1.5) or want[2].sum() < len(want[2]) - 5)
    bad = (tt[0], tt[1].clone(), tt[2])
    bad[1][3] = 9
    with pytest.raises(ValueError, match='view index'):
        KP.triangulate_tracks(kp, bad, cams, max_reproj, 1.5)


def test_the_stages_chain_into_view_selection(scene):
    """device results handed from stage to stage, and the tracks into viewsel's scores: each view's best partner is an adjacent camera"""
    from mvsdf_amd import viewsel
    kp, cams = scene['kp'], scene['cams']
    tracks = KP.build_tracks(kp, KP.verify_matches(kp, KP.match_descriptors(kp), cams))
    assert_tracks(tracks, scene['tracks'], 'chained')
    xyz, error, keep, obs_keep = KP.triangulate_tracks(kp, tracks, cams)
    d = np.abs(np.linalg.norm(np_(xyz)[np_(keep)] - S.CENTER, axis=1) - S.RADIUS)
    assert np_(keep).sum() >= 90 and np.median(d) <= 2 * 0.0057
    scores, counts = viewsel.view_scores(xyz, viewsel.centers_from_cams(cams), (tracks[0], tracks[1]))
    best = np.argmax(np_(scores) if isinstance(scores, torch.Tensor) else scores, 1)
    assert all(abs(int(b) - v) == 1 for v, b in enumerate(best))
