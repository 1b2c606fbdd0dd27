"""TSDF fusion without a GPU: the numpy restatement (tests/tsdf_ref.py) on scenes whose answer is known exactly, the masked extractor's
restatement against tests/mc_ref.py, grid_from_bbox, the argument errors (raised before the device is touched) and the plumbing."""
import os
import re

import numpy as np
import pytest

import mc_ref
import mvs_scene as S
import tsdf_ref as R
from tsdf_ref import smooth_field
from conftest import ROOT


def _exact_grid():
    """a power-of-two lattice in front of exact_self_pair's cameras: x in [-1, 1], y in [-0.5, 0.5], z in [0.5, 3.375]"""
    return np.array([-1.0, -0.5, 0.5]), 0.125, (17, 9, 24)


def test_exact_scene():
    cams, depths, _ = S.exact_self_pair()
    origin, h, dims = _exact_grid()
    out = R.integrate(cams, depths, origin, h, dims, trunc=0.5)
    i, j, k = np.meshgrid(*[np.arange(n) for n in dims], indexing='ij')
    x, y, z = origin[0] + i * h, origin[1] + j * h, origin[2] + k * h
    u, v = (64 * x + 16 * z) / z - 0.5, (64 * y + 8 * z) / z - 0.5
    seen = (u >= 0) & (u <= 31) & (v >= 0) & (v <= 15) & (z <= 2.5)
    assert seen.any() and (~seen).any() and (seen & (z > 2)).any() and (seen & (z < 1.5)).any()
    want = np.where(seen, np.minimum((2 - z) / 0.5, 1.0), 1.0).astype(np.float32)
    assert np.array_equal(out['tsdf'], want)
    assert np.array_equal(out['weight'], np.where(seen, 2, 0))
    assert np.array_equal(out['valid'], seen)
    two = R.integrate(cams, depths, origin, h, dims, trunc=0.5, min_views=2)
    assert np.array_equal(two['tsdf'], want) and np.array_equal(two['valid'], seen)
    one = R.integrate(cams, depths, origin, h, dims, trunc=0.5, min_views=2, views=[1])
    assert np.array_equal(one['weight'], np.where(seen, 1, 0)) and not one['valid'].any() and (one['tsdf'] == 1).all()


def test_holes_are_not_interpolated():
    cams, depths, _ = S.exact_self_pair()
    origin, h, dims = _exact_grid()
    full = R.integrate(cams[:1], depths[:1], origin, h, dims, trunc=0.5)['weight']
    for hole in (0.0, -1.0, np.nan, np.inf):
        d = depths[:1].copy()
        d[0, 7, 12] = hole
        w = R.integrate(cams[:1], d, origin, h, dims, trunc=0.5)['weight']
        lost = (full == 1) & (w == 0)
        assert lost.any() and (w <= full).all()
        i, j, k = np.nonzero(lost)                                              # exactly the points whose quad holds texel (12, 7)
        x, y, z = origin[0] + i * h, origin[1] + j * h, origin[2] + k * h
        u, v = 64 * x / z + 16 - 0.5, 64 * y / z + 8 - 0.5
        assert ((u >= 11) & (u < 13) & (v >= 6) & (v < 8)).all()


def test_jump_rule_rejects_a_quad_across_a_step():
    cams, depths, _ = S.exact_self_pair()
    origin, h, dims = _exact_grid()
    d = depths[:1].copy()
    d[0, :, 16:] = 3.0                                                          # a step of 1 between columns 15 and 16
    i, j, k = np.meshgrid(*[np.arange(n) for n in dims], indexing='ij')
    x, z = origin[0] + i * h, origin[2] + k * h
    u = 64 * x / z + 16 - 0.5
    across = (u >= 15) & (u < 16)
    off = R.integrate(cams[:1], d, origin, h, dims, trunc=0.5, jump=np.inf)['weight']
    on = R.integrate(cams[:1], d, origin, h, dims, trunc=0.5)['weight']         # jump = trunc = 0.5 < 1
    assert (off[across] == 1).any()
    assert (on[across] == 0).all() and np.array_equal(on[~across], off[~across])
    assert np.array_equal(R.integrate(cams[:1], d, origin, h, dims, trunc=0.5, jump=1.0)['weight'], off)   # max - min == jump is kept
    flat = R.integrate(cams[:1], depths[:1], origin, h, dims, trunc=0.5, jump=np.inf)['weight']
    assert flat.any() and np.array_equal(R.integrate(cams[:1], depths[:1], origin, h, dims, trunc=0.5, jump=0.0)['weight'], flat)   # a constant map has no jump


@pytest.mark.parametrize('shape', [(2, 2, 2), (5, 9, 13), (12, 7, 6)])
def test_masked_restatement_with_everything_valid_is_mc_ref(shape):
    vol = smooth_field(shape, seed=sum(shape))
    sp, org = (0.5, 0.25, 0.125), (-1.0, 2.0, 0.5)
    want = mc_ref.marching_cubes(vol, 0.0, sp, org)
    got = R.marching_cubes_masked(vol, np.ones(shape, bool), 0.0, sp, org)
    assert len(want[0]) > 0 or shape == (2, 2, 2)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)


@pytest.mark.parametrize('shape', [(5, 9, 13), (12, 7, 6), (9, 9, 9)])
def test_masked_restatement_under_a_mask(shape):
    vol = smooth_field(shape, seed=sum(shape) + 1)
    ok = np.random.RandomState(3).uniform(size=shape) < 0.9
    v, f, n = R.marching_cubes_masked(vol, ok)
    dv, df, _ = mc_ref.marching_cubes(vol)
    assert 0 < len(f) < len(df) and 0 < len(v) < len(dv)
    assert np.array_equal(np.unique(f), np.arange(len(v)))                      # every vertex is referenced by a face
    # the faces are the dense faces of the valid cells, vertex for vertex
    dense = {tuple(map(tuple, dv[t])) for t in df}
    assert all(tuple(map(tuple, v[t])) in dense for t in f)
    assert np.isfinite(n).all() and np.allclose(np.linalg.norm(n, axis=1)[np.linalg.norm(n, axis=1) > 0], 1, atol=1e-6)
    junk = vol.copy()
    junk[~ok] = np.nan                                                          # invalid values are never read
    for a, b in zip(R.marching_cubes_masked(junk, ok), (v, f, n)):
        assert np.array_equal(a, b)
    junk[tuple(np.argwhere(ok)[5])] = np.inf
    with pytest.raises(ValueError):
        R.marching_cubes_masked(junk, ok)
    assert len(R.marching_cubes_masked(vol, np.zeros(shape, bool))[0]) == 0
    lone = np.zeros(shape, bool)
    lone[:2, :2, :1] = True                                                     # no cell has 8 valid corners
    assert len(R.marching_cubes_masked(vol, lone)[0]) == 0


def test_grid_from_bbox():
    from mvsdf_amd import tsdf
    origin, h, dims = tsdf.grid_from_bbox([0.0, 0.0, 0.0], [1.0, 0.5, 0.26], voxel=0.25, pad_voxels=2)
    assert h == 0.25 and dims == (9, 7, 7) and np.array_equal(origin, [-0.5, -0.5, -0.5]) and origin.dtype == np.float64
    origin, h, dims = tsdf.grid_from_bbox(np.array([-1.0, 0.0, 2.0]), np.array([1.0, 1.0, 2.0]), resolution=8, pad_voxels=0)
    assert h == 0.25 and dims == (9, 5, 2) and np.array_equal(origin, [-1.0, 0.0, 2.0])     # a flat box still gets two points
    lo, hi = np.array([0.1, -0.2, 0.05]) - 0.7, np.array([0.1, -0.2, 0.05]) + 0.6
    origin, h, dims = tsdf.grid_from_bbox(lo, hi, resolution=50)
    assert h == pytest.approx(1.3 / 50) and (origin + (np.array(dims) - 1) * h >= hi + 2 * h - 1e-12).all() and (origin <= lo - 2 * h + 1e-12).all()
    for kw in (dict(), dict(voxel=0.1, resolution=4), dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=np.nan), dict(resolution=0), dict(resolution=2.5),
               dict(voxel=0.1, pad_voxels=-1)):
        with pytest.raises(ValueError):
            tsdf.grid_from_bbox(lo, hi, **kw)
    for bad_lo, bad_hi in (([0, 0], [1, 1]), ([0, 0, 0], [1, 1, np.nan]), ([0, 0, 2], [1, 1, 1])):
        with pytest.raises(ValueError):
            tsdf.grid_from_bbox(bad_lo, bad_hi, voxel=0.1)
    with pytest.raises(ValueError):
        tsdf.grid_from_bbox([0, 0, 0], [0, 0, 0], resolution=4)


def test_argument_errors_need_no_device():
    from mvsdf_amd import mesh, tsdf
    cams, depths, _ = S.make_views(3, (20, 28), clean=True)
    org, h, dims = S.CENTER - 0.8, 0.1, (17, 17, 17)
    nan_cam, inf_cam = cams.copy(), cams.copy()
    nan_cam[1, 1, 0, 0] = np.nan
    inf_cam[2, 0, 1, 3] = np.inf
    for args, kw in (((cams[:2], depths, org, h, dims), {}), ((cams, depths[0], org, h, dims), {}), ((cams, depths[:, :1], org, h, dims), {}),
                     ((cams, depths, org[:2], h, dims), {}), ((cams, depths, org, h, (17, 17)), {}), ((cams, depths, org, h, 17), {}),
                     ((cams, depths, org, 0.0, dims), {}), ((cams, depths, org, -0.1, dims), {}), ((cams, depths, org, np.nan, dims), {}),
                     ((cams, depths, org, h, (17, 1, 17)), {}), ((cams, depths, org, h, (17, 17.0, 17)), {}),
                     ((nan_cam, depths, org, h, dims), {}), ((inf_cam, depths, org, h, dims), {}),
                     ((cams, depths, org * np.inf, h, dims), {}),
                     ((cams, depths, org, h, dims), dict(trunc=np.nan)), ((cams, depths, org, h, dims), dict(trunc=np.inf)),
                     ((cams, depths, org, h, dims), dict(trunc=0.0)), ((cams, depths, org, h, dims), dict(jump=-1.0)),
                     ((cams, depths, org, h, dims), dict(jump=np.nan)), ((cams, depths, org, h, dims), dict(min_views=0)),
                     ((cams, depths, org, h, dims), dict(min_views=1.5)),
                     ((cams, depths, org, h, dims), dict(views=[0, 3])), ((cams, depths, org, h, dims), dict(views=[-1])),
                     ((cams, depths, org, h, dims), dict(views=[]))):
        with pytest.raises(ValueError):
            tsdf.integrate_depths(*args, **kw)
    vol = np.zeros((4, 5, 6), np.float32)
    for v, ok in ((vol, np.ones((4, 5, 5), bool)), (vol, np.ones((4, 5, 6), np.float32)), (vol[0], np.ones((5, 6), bool)),
                  (vol[:1], np.ones((1, 5, 6), bool))):
        with pytest.raises(ValueError):
            mesh.marching_cubes_masked(v, ok)
    with pytest.raises(ValueError):
        mesh.marching_cubes_masked(vol, np.ones(vol.shape, bool), spacing=(1.0, np.nan, 1.0))


def test_plumbing():
    from mvsdf_amd import _lib, build
    assert 'tsdf.hip' in build.SOURCES and 'mesh_kernels.hip' in build.SOURCES
    hdr = open(os.path.join(ROOT, 'include', 'mvsdf_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    # the integration lives in tsdf.hip; the masked extractor's entry points sit beside marching_cubes' in mesh_kernels.hip, which shares mesh_common.h
    for name, where in (('mvsdf_tsdf_workspace_bytes', 'tsdf.hip'), ('mvsdf_tsdf_integrate', 'tsdf.hip'), ('mvsdf_mcm_workspace_bytes', 'mesh_kernels.hip'),
                        ('mvsdf_mcm_count', 'mesh_kernels.hip'), ('mvsdf_mcm_emit', 'mesh_kernels.hip')):
        src = open(os.path.join(ROOT, 'mvsdf_amd', 'csrc', where)).read()
        assert name in _lib.EXPORTS and re.search(r'\b%s\s*\(' % name, hdr) and re.search(r'\b%s\s*\(' % name, src), name
    assert '#include "mesh_common.h"' in open(os.path.join(ROOT, 'mvsdf_amd', 'csrc', 'mesh_kernels.hip')).read()
