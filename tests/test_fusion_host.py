"""The depth-map fusion definition (mvsdf_amd/fusion.py) through its numpy restatement tests/fusion_ref.py: the properties that follow from the
definition itself, on the scenes of tests/mvs_scene.py, plus the host side of mvsdf_amd/fusion.py (matrices, argument checks, PLY output).  The
device result is held to the same restatement bit for bit in tests/test_gpu_fusion.py."""
import importlib.util
import os

import numpy as np
import pytest

import fusion_ref as R
import mvs_scene as S
from conftest import ROOT

DEP = 0.01


def _sphere_depth(cam, hw):
    """camera-z depth of the scene's sphere (normalised radius 0.6) at every pixel centre, fp64; 0 where the ray misses"""
    h, w = hw
    xs, ys = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    E, K = cam[0], cam[1, :3, :3]
    o = -E[:3, :3].T @ E[:3, 3] - S.CENTER
    d = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs)], -1) @ E[:3, :3]
    a, b, c = (d * d).sum(-1), 2 * (d @ o), (o * o).sum() - (0.6 * S.SIZE / 2) ** 2
    disc = b * b - 4 * a * c
    return np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), 0.0)


@pytest.fixture(scope='module')
def clean():
    cams, depths, pairs = S.make_views(6, (48, 64), clean=True)
    return cams, depths, pairs, R.fuse(cams, depths, pairs)


def test_clean_sphere_keeps_consistent_pixels_near_their_input_depth(clean):
    cams, depths, pairs, o = clean
    kept = o['fused_depths'] > 0
    valid = depths > 0
    print('kept %d of %d valid pixels' % (kept.sum(), valid.sum()))
    assert len(o['points']) == kept.sum() and 2 * kept.sum() > valid.sum()
    d = depths.astype(np.float64)
    rel = np.abs(o['df'] - d)[kept] / d[kept]
    print('largest |df - d| / d = %.6f' % rel.max())
    assert (np.abs(o['df'] - d)[kept] < DEP * d[kept]).all()          # df is a mean of d and of values within dep_thresh * d of it
    assert (o['counts'][kept] >= 2).all() and (o['counts'] <= 5).all()
    assert np.array_equal(o['fused_depths'][kept], o['df'][kept].astype(np.float32)) and (o['fused_depths'][~kept] == 0).all()


def test_points_are_the_back_projections_of_their_pixels(clean):
    cams, depths, pairs, o = clean
    _, Pinv = R.matrices(cams)
    v, p = o['view'].astype(np.int64), o['pixel'].astype(np.int64)
    assert (np.diff(v * depths[0].size + p) > 0).all()               # (view, y, x) order
    y, x = p // 64, p % 64
    df = o['df'][v, y, x]
    q = np.stack([(x + 0.5) * df, (y + 0.5) * df, df, np.ones_like(df)], 1)
    for i in range(len(q)):
        M = Pinv[v[i]]
        want = [((M[c, 0] * q[i, 0] + M[c, 1] * q[i, 1]) + M[c, 2] * q[i, 2]) + M[c, 3] * q[i, 3] for c in range(3)]
        assert np.array_equal(o['points'][i], np.array(want))
    assert np.array_equal(o['lo'], o['points'].min(0)) and np.array_equal(o['hi'], o['points'].max(0))


def test_kept_pixels_off_the_depth_step_lie_on_the_sphere(clean):
    cams, depths, pairs, o = clean
    for r in range(6):
        sph = _sphere_depth(cams[r], (48, 64))
        d = depths[r].astype(np.float64)
        on = (d > 0) & (np.abs(d - sph) <= 2.0 ** -23 * sph)         # the input depth is the sphere's, rounded to fp32; the step patch is 0.12 off
        kept = (o['fused_depths'][r] > 0) & on
        assert kept.sum() > 500
        # |df - sph| <= |df - d| + |d - sph| < dep_thresh * d + the fp32 rounding of d
        assert (np.abs(o['df'][r] - sph)[kept] < DEP * d[kept] + 2.0 ** -23 * sph[kept]).all()


def test_disagreeing_views_and_holes_cost_pixels(clean):
    n_clean = len(clean[3]['points'])
    cams, depths, pairs = S.make_views(6, (48, 64), hole_frac=0.0)   # default bumps and a per-view scale error of up to 3 % > dep_thresh
    n_bumpy = len(R.fuse(cams, depths, pairs)['points'])
    cams, depths, pairs = S.make_views(6, (48, 64))                  # and 15 % holes: the four-texel rule makes a hole cost its neighbours
    n_holes = len(R.fuse(cams, depths, pairs)['points'])
    print('kept: clean %d, bumpy %d, with holes %d' % (n_clean, n_bumpy, n_holes))
    assert 2 * n_bumpy < n_clean and n_holes < n_bumpy


def test_vthresh_zero_keeps_every_masked_pixel(clean):
    cams, depths, pairs, _ = clean
    o = R.fuse(cams, depths, pairs, vthresh=0)
    assert np.array_equal(o['fused_depths'] > 0, depths > 0) and len(o['points']) == (depths > 0).sum()
    lone = (o['counts'] == 0) & (depths > 0)
    assert lone.any() and np.array_equal(o['fused_depths'][lone], depths[lone]) and np.array_equal(o['df'][lone], depths[lone].astype(np.float64))


def test_view_cuts_the_pair_list(clean):
    cams, depths, pairs, full = clean
    a = R.fuse(cams, depths, pairs, view=1, vthresh=1)
    b = R.fuse(cams, depths, [p[:1] for p in pairs], vthresh=1)
    assert a['counts'].max() == 1 and np.array_equal(a['points'], b['points']) and np.array_equal(a['counts'], b['counts'])
    assert np.array_equal(R.fuse(cams, depths, [p + p for p in pairs], view=5)['points'], full['points'])


def test_thresholds_are_strict():
    cams, depths, pairs = S.exact_self_pair()
    o = R.fuse(cams, depths, pairs, vthresh=1)
    assert (o['counts'] == 1).all() and np.array_equal(o['df'], depths.astype(np.float64))
    assert (R.fuse(cams, depths, pairs, vthresh=1, pix_thresh=0.0)['counts'] == 0).all()        # 0 < 0 is false
    assert (R.fuse(cams, depths, pairs, vthresh=1, dep_thresh=0.0)['counts'] == 0).all()


def test_probability_mask_is_an_fp32_compare():
    depths = np.array([[[1.0, 2.0], [np.inf, -1.0]], [[np.nan, 0.0], [3.0, 4.0]]], np.float32)
    assert np.array_equal(R.mask_depths(depths), np.array([[[1, 2], [0, 0]], [[0, 0], [3, 4]]], np.float32))
    probs = np.ones((2, 3, 2, 2), np.float32)
    probs[0, 0, 0, 0] = np.float32(0.8)                               # == fp32(0.8): not above it, though above the double 0.8
    probs[1, 2, 1, 1] = np.nextafter(np.float32(0.8), np.float32(1))
    probs[1, 1, 1, 0] = 0.5
    assert np.array_equal(R.mask_depths(depths, probs), np.array([[[0, 2], [0, 0]], [[0, 0], [0, 4]]], np.float32))


def test_host_matrices_match_the_restatement():
    from mvsdf_amd import fusion
    cams, _, _ = S.make_views(4, (20, 28))
    P, Pinv = fusion.projection_matrices(cams)
    Pr, Pir = R.matrices(cams)
    assert np.array_equal(P, np.stack(Pr)) and np.array_equal(Pinv, np.stack(Pir))


def test_arguments_are_refused_before_anything_is_launched():
    from mvsdf_amd import fusion
    cams, depths, pairs = S.make_views(3, (20, 28), clean=True)
    bad = cams.copy()
    bad[1, 0, 2, 3] = np.nan
    for args, kw in (((bad, depths, pairs), {}), ((cams, depths, [[1], [3], [0]]), {}), ((cams, depths, [[1], [-1], [0]]), {}),
                     ((cams, depths, pairs), dict(view=0)), ((cams[:2], depths, pairs), {}), ((cams, depths, pairs[:2]), {}),
                     ((cams, depths[:, :1], pairs), {}), ((cams, depths[0], pairs), {}), ((cams, depths, pairs), dict(pix_thresh=float('nan'))),
                     ((cams, depths, pairs), dict(probs=np.ones((3, 2, 20, 28), np.float32))),
                     ((cams, depths, pairs), dict(images=np.zeros((3, 20, 28, 3), np.float32)))):
        with pytest.raises(ValueError):
            fusion.fuse_depths(*args, **kw)


def test_save_points_round_trip(tmp_path):
    from mvsdf_amd import chamfer, fusion
    rs = np.random.RandomState(0)
    pts = rs.normal(size=(37, 3)) * 100
    col = rs.randint(0, 256, (37, 3)).astype(np.uint8)
    for name, c in (('a.ply', None), ('b.ply', col)):
        path = str(tmp_path / name)
        fusion.save_points(path, pts, c)
        assert np.array_equal(chamfer.load_points(path), pts.astype(np.float32).astype(np.float64))
    from mvsdf_amd.mesh import _ply_elements
    assert np.array_equal(np.stack([_ply_elements(path)['vertex'][k] for k in ('red', 'green', 'blue')], 1), col)
    fusion.save_points(str(tmp_path / 'e.ply'), np.zeros((0, 3)))
    assert chamfer.load_points(str(tmp_path / 'e.ply')).shape == (0, 3)
    with pytest.raises(ValueError):
        fusion.save_points(path, pts[:, :2])


def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_' + name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fusion_command_line_and_its_refusals(capsys):
    t = _tool('fusion')
    a = t.parse_args('--data D --pair D/pair.txt --view 10 --vthresh 2 --pthresh .8,.7,.8 --cam_scale 1 --no_normal --downsample -1'.split())
    assert (a.data, a.view, a.vthresh, a.pthresh, a.pix_thresh, a.dep_thresh) == ('D', 10, 2, [0.8, 0.7, 0.8], 1.0, 0.01)
    a = t.parse_args('--data D --no_normal --pix_thresh 0.5 --dep_thresh 0.02 --view 3'.split())
    assert (a.view, a.pix_thresh, a.dep_thresh, a.pair) == (3, 0.5, 0.02, None)
    for argv, word in (('--data D', 'normal'), ('--data D --no_normal --downsample 0.5', 'down-sampling'),
                       ('--data D --no_normal --cam_scale 2', 'cam_scale'), ('--data D --no_normal --pthresh .8,.7', 'three')):
        with pytest.raises(SystemExit):
            t.parse_args(argv.split())
        assert word in capsys.readouterr().err
