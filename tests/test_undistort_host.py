"""Image undistortion without a GPU: the numpy restatement (tests/undistort_ref.py) against its own conditions -- the Newton residual, an independent
projection through np.arctan, the zero-distortion and blank-pixel rules, the written-out atan -- the library's host entry points against the
restatement bit for bit, the model writer and loader, the argument errors and the command-line parsers."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import colmap_scene as CS                                                   # noqa: E402
import undistort_ref as R                                                   # noqa: E402
import viewsel_ref as VR                                                    # noqa: E402
from mvsdf_amd import undistort                                             # noqa: E402
from mvsdf_amd._lib import lib                                              # noqa: E402
from mvsdf_amd.datasets import colmap                                       # noqa: E402

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')
cameras = pytest.mark.parametrize('cam', R.CAMERAS, ids=R.CAMERA_IDS)
IDENTITY_MODELS = ('SIMPLE_PINHOLE', 'PINHOLE', 'SIMPLE_RADIAL', 'RADIAL', 'OPENCV', 'FULL_OPENCV')
FISHEYE_MODELS = ('OPENCV_FISHEYE', 'SIMPLE_RADIAL_FISHEYE', 'RADIAL_FISHEYE')


def _grid():
    """the border samples and a grid of interior points, in source pixels"""
    g = np.stack(np.meshgrid(np.linspace(0.3, R.W - 0.3, 11), np.linspace(0.2, R.H - 0.2, 9)), -1).reshape(-1, 2)
    return np.concatenate([R.border_samples(R.W, R.H)[0], g])


def _host_points(points, cam, pin=None, inverse=1):
    """mvsdf_undistort_points_host: the kernel's functions on the CPU -> (out, error bits)"""
    family, block = undistort.camera_block(cam)
    pin = np.array([1.0, 1.0, 0.0, 0.0]) if pin is None else np.ascontiguousarray(pin['params'], dtype=np.float64)
    p = np.ascontiguousarray(points, dtype=np.float64)
    out, err = np.empty_like(p), np.zeros(1, np.int64)
    assert lib().mvsdf_undistort_points_host(p.ctypes.data, len(p), family, block.ctypes.data, pin.ctypes.data, inverse, out.ctypes.data, err.ctypes.data) == 0
    return out, int(err[0])


@cameras
def test_newton_residual(cam):
    p = _grid()
    und, err, res = R.undistort_points(p, cam, with_err=True)
    assert not err.any()
    back = R.distort_points(und, cam)
    assert np.abs(back - p).max() <= 1e-9 and res.max() <= 1e-9              # a cap: round-off here is about 1e-14 px, a failed inverse is off by > 1e-6


@cameras
def test_undistorted_points_equal_an_independent_pinhole_projection(cam):
    rng = np.random.RandomState(1)
    out_cam = R.undistorted_camera(cam, 0.5)
    fx, fy, cx, cy = out_cam['params']
    xyz = np.stack([rng.uniform(-0.4, 0.4, 400), rng.uniform(-0.3, 0.3, 400), rng.uniform(0.8, 3.0, 400)], 1)
    p_d = R.project_direct(cam, xyz)                                         # the model's formula written with np.arctan, not the restatement's functions
    inside = (p_d[:, 0] >= 0) & (p_d[:, 0] <= R.W) & (p_d[:, 1] >= 0) & (p_d[:, 1] <= R.H)
    assert inside.sum() > 100
    p_u = np.stack([fx * xyz[:, 0] / xyz[:, 2] + cx, fy * xyz[:, 1] / xyz[:, 2] + cy], 1)
    got = R.undistort_points(p_d[inside], cam, out_cam)
    assert np.abs(got - p_u[inside]).max() <= 1e-9


@pytest.mark.parametrize('model', IDENTITY_MODELS)
def test_zero_distortion_keeps_the_camera(model):
    cam = R.camera(model, [0.0] * R.N_COEFFICIENTS[model])
    p = _grid()
    normalised = np.stack([(p[:, 0] - R.CX) / R.F, (p[:, 1] - R.CY) / R.F], 1)
    assert np.array_equal(R.undistort_points(p, cam).view(np.uint64), normalised.view(np.uint64))      # U returns its input bit for bit
    for blank in (0.0, 0.5, 1.0):
        out, s, s_full, s_all = R.undistorted_camera(cam, blank, details=True)
        assert s == 1.0 and s_full == 1.0 and s_all == 1.0
        assert (out['width'], out['height']) == (R.W, R.H) and out['params'].tolist() == [R.F, R.F, R.CX, R.CY]


@pytest.mark.parametrize('model', FISHEYE_MODELS)
def test_zero_coefficients_of_a_fisheye_model_are_the_equidistant_fisheye(model):
    """A fisheye model with every coefficient 0 still maps theta, not tan(theta), to the radius: its forward map is not the identity, the ratios are
    tan(theta) / theta > 1 and the scale rule must NOT return 1 (the zero-distortion rule above covers the models whose zero is a pinhole)."""
    cam = R.camera(model, [0.0] * R.N_COEFFICIENTS[model])
    out, s, s_full, s_all = R.undistorted_camera(cam, 0.0, details=True)
    th = np.arctan((R.H - R.CY) / R.F)                                       # the nearest border sample is not nearer than the nearest border
    assert s == s_full and 1.0 < np.tan(th) / th * (1 - 1e-3) <= s_full < s_all
    assert out['width'] >= R.W and out['height'] >= R.H
    assert R.undistort_images(np.ones((1, R.H, R.W, 1), np.uint8), cam, out)[1].all()


@cameras
def test_blank_pixel_rule(cam):
    """blank_pixels = 0: no output pixel is invalid.  blank_pixels = 1: every source border sample lands inside the output rectangle BEFORE its size is
    truncated to whole pixels, [0, s W] x [0, s H] about the principal point: W' = floor(s W) drops up to one pixel, shared between the two sides
    as cx' = cx W' / W shares it, so in the output's pixels the bound is -cx (s - W'/W) <= X' <= W' + (W - cx)(s - W'/W), less than a pixel beyond
    [0, W'] (SIMPLE_RADIAL k = -0.2: s W = 40.48, W' = 40, the leftmost sample at -0.095).  Strictly inside [0, W'] cannot hold with the floor."""
    out0, s0, s_full, s_all = R.undistorted_camera(cam, 0.0, details=True)
    assert s0 == s_full <= s_all
    assert R.undistort_images(np.zeros((1, R.H, R.W, 1), np.uint8), cam, out0)[1].all()          # blank_pixels = 0: no output pixel is invalid
    out1, s1, _, _ = R.undistorted_camera(cam, 1.0, details=True)
    assert s1 == s_all
    b = R.undistort_points(R.border_samples(R.W, R.H)[0], cam, out1)
    lost_x, lost_y = s1 - out1['width'] / R.W, s1 - out1['height'] / R.H
    assert 0 <= lost_x * R.W < 1 and 0 <= lost_y * R.H < 1
    assert (b[:, 0] >= -R.CX * lost_x - 1e-9).all() and (b[:, 0] <= out1['width'] + (R.W - R.CX) * lost_x + 1e-9).all()
    assert (b[:, 1] >= -R.CY * lost_y - 1e-9).all() and (b[:, 1] <= out1['height'] + (R.H - R.CY) * lost_y + 1e-9).all()
    assert b[:, 0].min() > -1 and b[:, 1].min() > -1 and b[:, 0].max() < out1['width'] + 1 and b[:, 1].max() < out1['height'] + 1
    assert out1['width'] >= out0['width'] and out1['height'] >= out0['height']


def test_barrel_and_pincushion_examples():
    for model, dist, barrel in (('SIMPLE_RADIAL', [-0.2], True), ('SIMPLE_RADIAL', [0.15], False), ('RADIAL', [-0.2, 0.05], True), ('RADIAL', [0.1, 0.02], False),
                                ('SIMPLE_RADIAL_FISHEYE', [-0.1], True), ('SIMPLE_RADIAL_FISHEYE', [0.5], False), ('RADIAL_FISHEYE', [-0.1, 0.02], True),
                                ('RADIAL_FISHEYE', [0.45, 0.1], False)):
        _, _, s_full, s_all = R.undistorted_camera(R.camera(model, dist), details=True)
        assert (s_all > 1 and s_full > 1) if barrel else (s_full < 1 and s_all < 1), (model, dist, s_full, s_all)


def test_written_out_atan_stays_within_4_ulp_of_numpy():
    r = np.concatenate([np.linspace(0.0, 4.0, 200001), np.random.RandomState(2).uniform(0, 4, 100000), [1e-300, 1e-9, np.tan(np.pi / 8), 1.0]])
    got, ref = VR.atan2_pos(r, 1.0), np.arctan(r)
    assert (np.abs(got - ref) <= 4 * np.spacing(ref)).all()


@cameras
def test_library_host_functions_equal_the_restatement(cam):
    """the functions the kernels run, compiled for the CPU, against numpy bit for bit: points both ways, the camera rule, and images with their mask"""
    p = _grid()
    for pin in (None, R.undistorted_camera(cam, 0.5)):
        out, err = _host_points(p, cam, pin)
        assert err == 0 and np.array_equal(out.view(np.uint64), R.undistort_points(p, cam, pin).view(np.uint64))
        back, err = _host_points(out, cam, pin, inverse=0)
        assert err == 0 and np.array_equal(back.view(np.uint64), R.distort_points(out, cam, pin).view(np.uint64))
    rng = np.random.RandomState(3)
    family, block = undistort.camera_block(cam)
    for blank in (0.0, 0.5, 1.0):
        und, _ = _host_points(undistort.border_samples(R.W, R.H)[0], cam)
        out_cam = undistort.scale_rule(cam, und, blank)[0]
        ref_cam = R.undistorted_camera(cam, blank)
        assert (out_cam['model'], out_cam['width'], out_cam['height']) == ('PINHOLE', ref_cam['width'], ref_cam['height'])
        assert np.array_equal(out_cam['params'], ref_cam['params'])
        Ho, Wo = out_cam['height'], out_cam['width']
        for C, dtype in ((1, np.uint8), (3, np.uint8), (4, np.uint8), (3, np.float32)):
            img = rng.randint(0, 256, (2, R.H, R.W, C)).astype(np.uint8) if dtype == np.uint8 else rng.uniform(-256, 256, (2, R.H, R.W, C)).astype(np.float32)
            dst, mask = np.empty((2, Ho, Wo, C), dtype), np.empty((Ho, Wo), np.uint8)
            assert lib().mvsdf_undistort_images_host(img.ctypes.data, 2, R.H, R.W, C, 0 if dtype == np.uint8 else 1, family, block.ctypes.data,
                                                     out_cam['params'].ctypes.data, Ho, Wo, dst.ctypes.data, mask.ctypes.data) == 0
            ref, ref_mask = R.undistort_images(img, cam, out_cam)
            assert np.array_equal(mask, ref_mask) and np.array_equal(dst.view(np.uint8), ref.view(np.uint8))


def test_host_error_bits():
    fold = R.camera('SIMPLE_RADIAL', [-3.0])                                # D(r) = r (1 - 3 r^2) peaks at 0.22: the border at 0.45 is out of reach
    p = R.border_samples(R.W, R.H)[0]
    _, err = _host_points(p, fold)
    assert err & 3
    assert R.undistort_points(p, fold, with_err=True)[1].any()
    with pytest.raises(ValueError):
        R.undistorted_camera(fold)
    _, err = _host_points(np.array([[np.nan, 1.0], [3.0, np.inf]]), R.CAMERAS[0])
    assert err == 1
    block = undistort.camera_block(R.CAMERAS[0])[1].copy()
    block[5] = np.nan                                                        # the C call refuses non-finite parameters outright
    out, e = np.zeros((1, 2)), np.zeros(1, np.int64)
    assert lib().mvsdf_undistort_points_host(out.ctypes.data, 1, 1, block.ctypes.data, np.array([1.0, 1, 0, 0]).ctypes.data, 1, out.ctypes.data, e.ctypes.data) != 0


def _distorted_scenes():
    a = CS.make_scene(model='SIMPLE_RADIAL', distortion=-0.1)
    b = CS.make_scene()
    b['cameras'][1]['model'] = 'OPENCV_FISHEYE'
    b['cameras'][1]['params'] = np.array([CS.FOCAL, CS.FOCAL, CS.W / 2, CS.H / 2, 0.05, -0.01, 0.002, -0.001], dtype=np.float64)
    return a, b


def test_model_round_trip_and_allow_distortion(tmp_path):
    scene = CS.make_scene(blind_image=True)
    colmap.write_colmap_text(scene, str(tmp_path / 'plain'))
    CS.assert_models_equal(scene, colmap.load_colmap_model(str(tmp_path / 'plain')))
    for k, scene in enumerate(_distorted_scenes()):
        for kind, write in (('text', colmap.write_colmap_text), ('bin', CS.write_binary)):
            d = str(tmp_path / ('%s%d' % (kind, k)))
            write(scene, d)
            with pytest.raises(ValueError, match='undistort'):
                colmap.load_colmap_model(d)
            CS.assert_models_equal(scene, colmap.load_colmap_model(d, allow_distortion=True))
    for model, n in (('FOV', 5), ('THIN_PRISM_FISHEYE', 12)):
        scene = CS.make_scene()
        scene['cameras'][1]['model'] = model
        scene['cameras'][1]['params'] = np.array([CS.FOCAL, CS.FOCAL, CS.W / 2, CS.H / 2] + [0.0] * (n - 4))
        colmap.write_colmap_text(scene, str(tmp_path / model))
        for allow in (False, True):
            with pytest.raises(ValueError, match='undistort the images first'):
                colmap.load_colmap_model(str(tmp_path / model), allow_distortion=allow)
    path = tmp_path / 'plain' / 'cameras.txt'
    path.write_text(path.read_text().replace('PINHOLE', 'MY_LENS'))
    with pytest.raises(ValueError, match='MY_LENS'):
        colmap.load_colmap_model(str(tmp_path / 'plain'), allow_distortion=True)


def test_argument_errors():
    cam = R.CAMERAS[0]
    for cx, cy in ((0.0, 14.9), (37.0, 14.9), (18.2, -1.0), (18.2, 29.0)):
        with pytest.raises(ValueError, match='principal point'):
            undistort.undistorted_camera(R.camera('SIMPLE_RADIAL', [-0.2], cx=cx, cy=cy))
    with pytest.raises(ValueError, match='undistort the images first'):
        undistort.undistorted_camera({'model': 'FOV', 'width': R.W, 'height': R.H, 'params': np.array([R.F, R.F, R.CX, R.CY, 0.1])})
    with pytest.raises(ValueError, match='takes 4 parameters, got 5'):
        undistort.undistorted_camera({'model': 'SIMPLE_RADIAL', 'width': R.W, 'height': R.H, 'params': np.array([R.F, R.CX, R.CY, 0.1, 0.0])})
    for blank in (-0.1, 1.5, np.nan):
        with pytest.raises(ValueError, match='blank_pixels'):
            undistort.undistorted_camera(cam, blank_pixels=blank)
    with pytest.raises(ValueError, match='min_scale'):
        undistort.undistorted_camera(cam, min_scale=1.5, max_scale=1.0)
    with pytest.raises(ValueError, match='NaN or infinite'):
        undistort.undistorted_camera(R.camera('RADIAL', [0.1, np.nan]))
    with pytest.raises(ValueError, match='focal'):
        undistort.camera_block(R.camera('OPENCV', [0, 0, 0, 0], f=-1.0))
    with pytest.raises(ValueError, match=r'\[V, 29, 37, C\]'):
        undistort.undistort_images(np.zeros((1, R.W, R.H, 3), np.uint8), cam, R.undistorted_camera(cam))
    with pytest.raises(ValueError, match='uint8 or float32'):
        undistort.undistort_images(np.zeros((1, R.H, R.W, 3), np.float64), cam, R.undistorted_camera(cam))
    with pytest.raises(ValueError, match='SIMPLE_PINHOLE or PINHOLE'):
        undistort.undistort_images(np.zeros((1, R.H, R.W, 3), np.uint8), cam, cam)
    with pytest.raises(ValueError, match='view_chunk'):
        undistort.undistort_images(np.zeros((1, R.H, R.W, 3), np.uint8), cam, R.undistorted_camera(cam), view_chunk=0)


def test_scale_rule_clamps_and_refuses_fold_over():
    cam = R.CAMERAS[0]
    pts, _ = undistort.border_samples(R.W, R.H)
    assert np.array_equal(pts, R.border_samples(R.W, R.H)[0]) and len(pts) == 2 * R.W + 2 * R.H + 4
    und = R.undistort_points(pts, cam)
    out, s, s_full, s_all = undistort.scale_rule(cam, und, 1.0, 0.2, 1.05)
    assert s == 1.05 < s_all and (out['width'], out['height']) == (int(np.floor(1.05 * R.W)), int(np.floor(1.05 * R.H)))
    out, s, _, _ = undistort.scale_rule(cam, und, 0.0, 1.08, 2.0)
    assert s == 1.08 > s_full
    assert out['params'][2] == (R.CX * out['width']) / R.W and out['params'][3] == (R.CY * out['height']) / R.H
    flipped = und.copy()
    flipped[3, 0] = -flipped[3, 0]
    with pytest.raises(ValueError, match='folds over'):
        undistort.scale_rule(cam, flipped)


def test_command_line_parsers():
    sys.path.insert(0, TOOLS)
    import colmap2mvs
    import time_undistort
    import undistort as undistort_tool
    a = undistort_tool.parser().parse_args(['m', 'i', 'o'])
    assert (a.model_dir, a.image_dir, a.out_dir, a.blank_pixels, a.min_scale, a.max_scale, a.view_chunk) == ('m', 'i', 'o', 0.0, 0.2, 2.0, None)
    a = undistort_tool.parser().parse_args(['m', 'i', 'o', '--blank_pixels', '0.5', '--min_scale', '0.5', '--max_scale', '1.5', '--view_chunk', '3'])
    assert (a.blank_pixels, a.min_scale, a.max_scale, a.view_chunk) == (0.5, 0.5, 1.5, 3)
    a = colmap2mvs.parser().parse_args(['m', 'i', 'o'])
    assert a.undistort is False and (a.max_d, a.num_pairs) == (256, 10)
    a = colmap2mvs.parser().parse_args(['m', 'i', 'o', '--undistort', '--blank_pixels', '1'])
    assert a.undistort is True and (a.blank_pixels, a.min_scale, a.max_scale) == (1.0, 0.2, 2.0)
    a = time_undistort.parser().parse_args([])
    assert (a.models, a.views, a.width, a.height, a.channels) == ('SIMPLE_RADIAL,OPENCV_FISHEYE', 64, 4000, 3000, 3)
    with pytest.raises(SystemExit):
        undistort_tool.main([os.path.join(TOOLS, 'no_such_model'), 'i', 'o'])
    cam = time_undistort.make_camera('OPENCV_FISHEYE', 400, 300)
    assert undistort.camera_block(cam)[0] == 3 and R.undistorted_camera(cam)['width'] > 0
