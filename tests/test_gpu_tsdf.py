"""integrate_depths and marching_cubes_masked (csrc/tsdf.hip) against the numpy restatement tests/tsdf_ref.py, bit for bit, twice in a row; the
masked extractor against marching_cubes itself under an all-true mask; the geometry of the fused sphere; the command."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import mvs_scene as S
import tsdf_ref as R
from tsdf_ref import smooth_field
from conftest import ROOT
from mvsdf_amd import mesh as M
from mvsdf_amd import tsdf

pytestmark = pytest.mark.gpu
RADIUS = 0.6                                                                    # of synth.make_depth_maps' sphere, in world units (SIZE = 2)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype in (np.float32, np.int32) else a.view(np.uint8) if a.dtype == np.bool_ else a


@functools.lru_cache(maxsize=None)
def _views(n, hw, clean, hole_frac=None):
    cams, depths, _ = S.make_views(n, hw, clean=clean, hole_frac=hole_frac)               # shared: a test copies before it changes one
    return cams, depths


FLANK = S.CENTER + RADIUS * np.array([np.cos(1.0), np.sin(1.0), 0.0])            # the sphere's point that faces camera 2 (angle 0.4 + 0.3 * 2)


def _grid(dims, half=0.8, center=None):
    """the longest axis spans 2 * half; centred on S.CENTER, a grid thinner than 9 points (a column along z) on the sphere's flank, where the
    surface runs through it lengthwise"""
    if center is None:
        center = FLANK if min(dims) < 9 else S.CENTER
    h = 2.0 * half / (max(dims) - 1)
    return center - h * (np.asarray(dims) - 1) / 2.0, h, tuple(dims)


def _check_volume(cams, depths, origin, h, dims, on_device=False, **kw):
    """integrate_depths == tsdf_ref.integrate in tsdf, weight and valid, bit for bit, twice in a row -> (Volume, ref)"""
    ref = R.integrate(cams, depths, origin, h, dims, **kw)
    vol = None
    for _ in range(2):
        vol = tsdf.integrate_depths(cams, torch.from_numpy(depths).cuda() if on_device else depths, origin, h, dims, **kw)
        assert vol.tsdf.dtype == torch.float32 and vol.weight.dtype == torch.int32 and vol.valid.dtype == torch.bool and vol.tsdf.is_cuda
        for name in ('tsdf', 'weight', 'valid'):
            got = getattr(vol, name).cpu().numpy()
            assert got.shape == tuple(dims) and np.array_equal(_bits(got), _bits(ref[name].astype(got.dtype))), name
    return vol, ref


def _check_mesh(vol, ok, got, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """a Mesh (or None) == tsdf_ref.marching_cubes_masked array for array; every vertex is referenced"""
    v, f, n = R.marching_cubes_masked(vol, ok, level, spacing, origin)
    if len(v) == 0:
        assert got is None
        return 0
    assert got is not None and got.faces.dtype == torch.int32
    assert np.array_equal(_bits(got.vertices.cpu().numpy()), _bits(v)), 'vertices'
    assert np.array_equal(got.faces.cpu().numpy(), f), 'faces'
    assert np.array_equal(_bits(got.normals.cpu().numpy()), _bits(n)), 'normals'
    assert np.array_equal(np.unique(f), np.arange(len(v)))
    return len(v)


def _check_volume_mesh(vol, ref):
    for _ in range(2):
        got = vol.mesh()
        n = _check_mesh(ref['tsdf'], ref['valid'], got, 0.0, (vol.voxel,) * 3, tuple(vol.origin))
    return got, n


@pytest.mark.parametrize('dims,hw', [((17, 17, 17), (20, 28)), ((33, 20, 9), (37, 53)), ((5, 9, 66), (37, 53)), ((40, 33, 35), (48, 64))])
@pytest.mark.parametrize('clean', [True, False])
@pytest.mark.parametrize('min_views', [1, 2])
def test_integration_and_mesh_equal_the_restatement(dims, hw, clean, min_views):
    cams, depths = _views(6, hw, clean)
    origin, h, dims = _grid(dims)
    vol, ref = _check_volume(cams, depths, origin, h, dims, min_views=min_views)
    assert 0 < int(ref['valid'].sum()) < ref['valid'].size and ref['weight'].max() >= 3
    _, n = _check_volume_mesh(vol, ref)
    assert n > 0


def test_holes_of_every_kind():
    cams, depths = _views(6, (37, 53), True, 0.3)
    origin, h, dims = _grid((33, 20, 9))
    vol, ref = _check_volume(cams, depths, origin, h, dims)
    _check_volume_mesh(vol, ref)
    cams, depths = _views(6, (20, 28), False)
    depths = depths.copy()
    hit = np.argwhere(depths[0] > 0)
    (y0, x0), (y1, x1), (y2, x2) = hit[len(hit) // 2], hit[len(hit) // 3], hit[len(hit) // 4]
    zero = depths.copy()
    zero[0, y0, x0] = zero[1, y1, x1] = zero[2, y2, x2] = 0
    depths[0, y0, x0], depths[1, y1, x1], depths[2, y2, x2] = np.nan, np.inf, -1.0
    origin, h, dims = _grid((17, 17, 17))
    vol, ref = _check_volume(cams, depths, origin, h, dims, on_device=True)
    want = R.integrate(cams, zero, origin, h, dims)
    assert np.array_equal(ref['weight'], want['weight']) and np.array_equal(_bits(ref['tsdf']), _bits(want['tsdf']))
    assert np.isfinite(ref['tsdf']).all()
    _check_volume_mesh(vol, ref)


def test_cameras_inside_the_grid_and_turned_sideways():
    """camera 1 sits inside the grid beyond the sphere's centre (part of the lattice has z <= 0); camera 2 is turned sideways (most of the lattice
    falls outside its image), as in test_gpu_fusion.py::test_points_behind_and_outside_a_source"""
    cams, depths = _views(6, (37, 53), True)
    cams = cams.copy()
    c0 = -cams[0, 0, :3, :3].T @ cams[0, 0, :3, 3]
    inside = cams[0].copy()
    inside[0, :3, 3] = -inside[0, :3, :3] @ (S.CENTER + 0.3 * (S.CENTER - c0))
    cams[1] = inside
    side = cams[0].copy()
    rot = np.array([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])
    side[0, :3, :3] = rot @ side[0, :3, :3]
    side[0, :3, 3] = -side[0, :3, :3] @ c0
    cams[2] = side
    for dims in ((17, 17, 17), (5, 9, 66)):
        origin, h, dims = _grid(dims)
        i, j, k = np.meshgrid(*[np.arange(n) for n in dims], indexing='ij')
        p = np.stack([origin[0] + i * h, origin[1] + j * h, origin[2] + k * h, np.ones(dims)], -1)
        z1 = p @ R.matrices(cams)[1][2]
        assert (z1 <= 0).any() and ((z1 > 0).any() or dims != (17, 17, 17))     # camera 1 is inside the cube; the column lies behind it
        for views in (None, [1], [2], [1, 2]):
            vol, ref = _check_volume(cams, depths, origin, h, dims, views=views)
        _check_volume_mesh(vol, ref)


def test_jump_views_single_view_and_the_smallest_grid():
    cams, depths = _views(6, (20, 28), True)
    origin, h, dims = _grid((17, 17, 17))
    # jump = 0 skips every sample whose four texels are not all equal.  On a map of odd size no quad of the sphere is (the principal point is a
    # texel's centre); on one of even size the four texels around the principal point are equal by symmetry, so a few samples survive
    odd = _views(6, (37, 53), True)
    vol, ref = _check_volume(odd[0], odd[1], origin, h, dims, jump=0.0)
    assert int(vol.weight.abs().sum()) == 0 and not bool(vol.valid.any()) and bool((vol.tsdf == 1).all()) and vol.mesh() is None
    vol, ref = _check_volume(cams, depths, origin, h, dims, jump=0.0)
    assert 0 < ref['weight'].sum() < 20
    _check_volume_mesh(vol, ref)
    _check_volume(cams, depths, origin, h, dims, jump=0.01)
    _check_volume(cams, depths, origin, h, dims, jump=float('inf'), trunc=0.17)
    vol, ref = _check_volume(cams, depths, origin, h, dims, views=[4, 1], min_views=2)
    assert ref['weight'].max() == 2
    _check_volume_mesh(vol, ref)
    twice, _ = _check_volume(cams, depths, origin, h, dims, views=[3, 3])       # a view listed twice counts twice
    once, _ = _check_volume(cams, depths, origin, h, dims, views=[3])
    assert torch.equal(twice.weight, 2 * once.weight)
    vol, ref = _check_volume(cams[:1], depths[:1], origin, h, dims)             # V = 1
    assert ref['weight'].max() == 1
    _check_volume_mesh(vol, ref)
    origin, h, dims = _grid((2, 2, 2), half=0.05)                               # a single cell across the sphere's flank
    vol, ref = _check_volume(cams, depths, origin, h, dims)
    assert ref['valid'].all() and (ref['tsdf'] < 0).any() and (ref['tsdf'] > 0).any()
    _, n = _check_volume_mesh(vol, ref)
    assert n > 0


def _field_case(shape, seed, p=0.7):
    vol = smooth_field(shape, seed)
    ok = np.random.RandomState(seed + 50).uniform(size=shape) < p
    return vol, ok


@pytest.mark.parametrize('shape', [(2, 2, 2), (5, 9, 66), (33, 33, 33)])
def test_masked_extraction_on_random_fields(shape):
    sp, org = (0.5, 0.25, 0.125), (-1.0, 2.0, 0.5)
    found = 0
    for seed in range(3 if shape == (2, 2, 2) else 1):
        vol, ok = _field_case(shape, seed + sum(shape))
        if shape == (2, 2, 2):
            ok[:] = seed != 1                                                   # one cell: all valid, nothing valid, all valid
        for _ in range(2):
            found += _check_mesh(vol, ok, M.marching_cubes_masked(vol, ok, 0.0, sp, org), 0.0, sp, org)
        found += _check_mesh(vol, ok, M.marching_cubes_masked(vol, ok.astype(np.uint8) * 7, 0.1, sp, org), 0.1, sp, org)   # uint8, another level
        # a strided volume: every second plane of a larger tensor, the last axis cut short
        big = torch.full((2 * shape[0], shape[1], shape[2] + 3), float('nan'), device='cuda')
        view = big[::2, :, :shape[2]]
        view.copy_(torch.from_numpy(vol))
        assert not view.is_contiguous()
        _check_mesh(vol, ok, M.marching_cubes_masked(view, torch.from_numpy(ok).cuda(), 0.0, sp, org), 0.0, sp, org)
        _check_mesh(vol, ok, M.marching_cubes_masked(torch.from_numpy(vol).cuda().permute(2, 0, 1).contiguous().permute(1, 2, 0), ok, 0.0, sp, org),
                    0.0, sp, org)
    assert found > 0 or shape == (2, 2, 2)


@pytest.mark.parametrize('shape', [(2, 2, 2), (5, 9, 66), (33, 33, 33)])
def test_an_all_true_mask_gives_marching_cubes_itself(shape):
    """not through the restatement: the two device extractors against each other, bit for bit"""
    sp, org = (0.5, 0.25, 0.125), (-1.0, 2.0, 0.5)
    vol = torch.from_numpy(smooth_field(shape, 7 + sum(shape))).cuda()
    if shape == (2, 2, 2):
        vol = vol - vol.mean()                                                  # the one cell crosses
    for level in (0.0, 0.05):
        a = M.marching_cubes(vol, level, sp, org)
        b = M.marching_cubes_masked(vol, torch.ones(shape, dtype=torch.bool, device='cuda'), level, sp, org)
        if a is None:                                                           # the single cell at the second level
            assert b is None and level != 0.0
            continue
        assert b is not None
        assert torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32))
        assert torch.equal(a.normals.view(torch.int32), b.normals.view(torch.int32))
        assert torch.equal(a.faces, b.faces)


def test_nan_at_invalid_points_and_at_a_valid_one():
    vol, ok = _field_case((12, 9, 20), 11)
    sp, org = (0.1, 0.1, 0.1), (0.0, 0.0, 0.0)
    want = M.marching_cubes_masked(vol, ok, 0.0, sp, org)
    junk = vol.copy()
    junk[~ok] = np.nan
    junk[~ok & (np.arange(20) % 2 == 0)] = np.inf
    got = M.marching_cubes_masked(junk, ok, 0.0, sp, org)
    assert want is not None and _check_mesh(vol, ok, got, 0.0, sp, org) > 0
    for name in ('vertices', 'normals', 'faces'):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    for bad in (np.nan, np.inf, -np.inf):
        junk2 = junk.copy()
        junk2[tuple(np.argwhere(ok)[len(vol) // 2])] = bad
        with pytest.raises(ValueError):
            M.marching_cubes_masked(junk2, ok, 0.0, sp, org)
    again = M.marching_cubes_masked(junk, ok, 0.0, sp, org)                      # the device is still usable
    assert torch.equal(again.faces, want.faces)
    assert M.marching_cubes_masked(junk, np.zeros_like(ok), 0.0, sp, org) is None
    assert M.marching_cubes_masked(np.ones_like(vol), ok, 0.0, sp, org) is None  # valid cells, no crossing


@functools.lru_cache(maxsize=None)
def _sphere_mesh(dims, hw):
    cams, depths = _views(6, hw, True)
    origin, h, dims = _grid(dims)
    m, vol = tsdf.tsdf_mesh(cams, depths, origin, h, dims, trunc=4 * h)
    return m, vol, h


@pytest.mark.parametrize('dims,hw,tol', [((17, 17, 17), (20, 28), 0.5), ((33, 33, 33), (48, 64), 1.5)])
def test_the_fused_sphere_lies_on_the_sphere(dims, hw, tol):
    """every vertex within tol voxels of the sphere of radius 0.6 about S.CENTER (a numpy prototype of the definition measured 0.29 h over 173
    crossings and 0.90 h over 875 crossings between valid points; the mesh's vertices are a subset of those)"""
    m, vol, h = _sphere_mesh(dims, hw)
    assert m is not None and m.vertices.shape[0] > 50
    err = (m.vertices.double().cpu().numpy() - S.CENTER).__pow__(2).sum(1) ** 0.5 - RADIUS
    print('dims %s hw %s: %d vertices, max |r - 0.6| = %.3f h' % (dims, hw, len(err), np.abs(err).max() / h))
    assert np.abs(err).max() <= tol * h
    n = m.normals.double().cpu().numpy()
    out = (m.vertices.double().cpu().numpy() - S.CENTER) / RADIUS
    assert ((n * out).sum(1) > 0.5).all()                                       # the tsdf grows outwards: so do the normals


def test_components_export_and_the_helpers(tmp_path):
    m, vol, h = _sphere_mesh((17, 17, 17), (20, 28))
    big = m.largest_component()
    flab, ncomp = m.components()
    assert ncomp >= 1 and 0 < len(big) <= len(m) and big.vertices.shape[0] <= m.vertices.shape[0]
    for ext in ('ply', 'obj'):
        path = str(tmp_path / ('sphere.' + ext))
        big.export(path)
        back = M.load_mesh(path)
        assert torch.equal(back.faces, big.faces.cpu()) and torch.equal(back.vertices, big.vertices.cpu())
    cams, depths = _views(6, (20, 28), True)
    origin, hh, dims = _grid((17, 17, 17))
    m2, vol2 = tsdf.tsdf_mesh(cams, depths, origin, hh, dims, largest=True)
    assert torch.equal(m2.faces, big.faces) and torch.equal(m2.vertices, big.vertices) and torch.equal(vol2.tsdf, vol.tsdf)
    assert vol.valid_share() == pytest.approx(float(vol.valid.float().mean()))
    assert vol.dims == (17, 17, 17) and vol.voxel == h and vol.trunc == 4 * h and vol.jump == vol.trunc and vol.min_views == 1


def test_errors_raise_and_leave_the_device_usable():
    cams, depths = _views(6, (20, 28), True)
    origin, h, dims = _grid((17, 17, 17))
    good = tsdf.integrate_depths(cams, depths, origin, h, dims)
    bad = cams.copy()
    bad[2, 1, 0, 0] = np.nan
    for args, kw in (((bad, depths, origin, h, dims), {}), ((cams, depths, origin, h, dims), dict(views=[6])),
                     ((cams, depths, origin, 0.0, dims), {}), ((cams, depths, origin, h, (17, 1, 17)), {})):
        with pytest.raises(ValueError):
            tsdf.integrate_depths(*args, **kw)
        assert torch.equal(tsdf.integrate_depths(cams, depths, origin, h, dims).tsdf, good.tsdf)


def test_the_library_refuses_what_the_binding_would_let_through():
    """the C entry validates on the host as well: its error bits reach the header without a launch"""
    from mvsdf_amd._lib import K, lib, _header
    V, H, W = 2, 4, 4
    d = torch.ones(V, H, W, device='cuda')
    size = lib().mvsdf_tsdf_workspace_bytes(V, H, W, 2)
    assert size > 0 and lib().mvsdf_tsdf_workspace_bytes(V, 1, W, 2) == 0 and lib().mvsdf_tsdf_workspace_bytes(V, H, W, 0) == 0
    assert lib().mvsdf_mcm_workspace_bytes(2, 2, 2) > 0 and lib().mvsdf_mcm_workspace_bytes(2, 1, 2) == 0
    ws = torch.zeros(size, dtype=torch.uint8, device='cuda')
    t = torch.full((3, 3, 3), 5.0, device='cuda')
    w = torch.full((3, 3, 3), 5, dtype=torch.int32, device='cuda')
    ok = torch.zeros(3, 3, 3, dtype=torch.uint8, device='cuda')
    eye = np.tile(np.eye(4).reshape(-1), 2)
    org = np.zeros(3)

    def call(mats=eye, views=(0, 1), origin=org, voxel=0.5, dims=(3, 3, 3), trunc=1.0, jump=1.0, min_views=1):
        views, dims = np.asarray(views, np.int32), np.asarray(dims, np.int64)
        rc = lib().mvsdf_tsdf_integrate(d.data_ptr(), V, H, W, mats.ctypes.data, views.ctypes.data, len(views), origin.ctypes.data, voxel, dims.ctypes.data,
                                        trunc, jump, min_views, ws.data_ptr(), size, t.data_ptr(), w.data_ptr(), ok.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        return _header(ws, K.MVSDF_RES_H_WORDS)
    nan = eye.copy()
    nan[5] = np.nan
    fin, view, rng, shape = ([0, bit] for bit in (K.MVSDF_TS_ERR_FINITE, K.MVSDF_TS_ERR_VIEW, K.MVSDF_TS_ERR_RANGE, K.MVSDF_TS_ERR_SHAPE))
    assert call(mats=nan) == fin and call(trunc=float('inf')) == fin and call(jump=float('nan')) == fin
    assert call(origin=np.array([0.0, np.inf, 0.0])) == fin
    assert call(views=(0, 2)) == view and call(views=(-1, 0)) == view
    assert call(voxel=0.0) == rng and call(trunc=-1.0) == rng and call(jump=-0.5) == rng and call(min_views=0) == rng
    assert call(dims=(3, 1, 3)) == shape
    assert bool((t == 5).all()) and bool((w == 5).all())                        # nothing was launched
    assert call() == [0, 0] and bool((w >= 0).all()) and bool((w <= 2).all())


def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_' + name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_command_writes_a_mesh(tmp_path, capsys):
    root, ids = S.write_mvs_scene(tmp_path)
    tool = _tool('tsdf_mesh')
    tool.main(['--data', root, '--resolution', '24', '--min_views', '2', '--largest', '--color'])
    printed = capsys.readouterr().out
    out = os.path.join(root, 'tsdf_mesh.ply')
    m = M.load_mesh(out)
    assert len(m) > 0 and m.vertices.shape[0] > 0 and m.vertex_colors is not None and 'valid share' in printed
    assert 'mesh: %d vertices, %d faces' % (m.vertices.shape[0], len(m)) in printed
    other = str(tmp_path / 'raw.obj')
    tool.main(['--data', root, '--voxel', '0.06', '--no_fuse', '--min_views', '1', '--trunc_voxels', '3', '--bbox', os.path.join(root, 'tsdf_mesh.ply'),
               '--out', other])
    assert len(M.load_mesh(other)) > 0
