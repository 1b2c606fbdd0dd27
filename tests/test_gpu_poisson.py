"""poisson.reconstruct, Field.valid and Field.mesh (csrc/poisson.hip) against the numpy restatement tests/poisson_ref.py, and fusion.depth_normals
(csrc/fusion.hip) against tests/fusion_normals_ref.py: bit for bit, every call twice in a row; the accuracy of the normals; the commands."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import fusion_normals_ref as NR
import mvs_scene as S
import poisson_ref as R
from conftest import ROOT
from mvsdf_amd import chamfer, cloud, fusion, poisson
from mvsdf_amd import mesh as M

pytestmark = pytest.mark.gpu
RADIUS = 0.6                                                                    # of synth.make_depth_maps' sphere, in world units (SIZE = 2)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a.view(np.uint32) if a.dtype == np.float32 else a


def _fbits(x):
    return np.float64(x).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _cloud(depth, n):
    """a seeded sphere cloud inside the admitted part of the unit grid (radius 0.3 at depth 2, where the admitted cube has half-edge 0.5) and the
    grid -> (points, normals, origin, h); shared: a test copies before it changes one"""
    p, nrm = R.sphere_cloud(n, seed=depth, radius=0.3 if depth == 2 else RADIUS)
    return (p, nrm) + R.unit_grid(depth)


@functools.lru_cache(maxsize=None)
def _ref(depth, n, cycles, sweeps):
    p, nrm, o, h = _cloud(depth, n)
    return R.reconstruct(p, nrm, o, h, depth, cycles, sweeps)


def _check_field(f, ref):
    N = 2 ** ref['depth'] + 1
    assert f.chi.is_cuda and f.chi.dtype == torch.float64 and tuple(f.chi.shape) == (N, N, N) and tuple(f.density.shape) == (N, N, N)
    assert (f.n_used, f.n_outside) == (ref['n_used'], ref['n_outside'])
    for name in ('chi', 'density', 'values'):
        got = getattr(f, name).cpu().numpy()
        assert got.shape == ref[name].shape and np.array_equal(_bits(got), _bits(ref[name])), name
    for name in ('iso', 'residual0', 'residual'):
        assert _fbits(getattr(f, name)) == _fbits(ref[name]), (name, getattr(f, name), ref[name])


def _check_mesh(got, ref, **kw):
    v, fc, n = R.mesh(ref, **kw)
    if len(v) == 0:
        assert got is None
        return 0
    assert got is not None
    assert np.array_equal(_bits(got.vertices.cpu().numpy()), _bits(v)), 'vertices'
    assert np.array_equal(got.faces.cpu().numpy(), fc), 'faces'
    assert np.array_equal(_bits(got.normals.cpu().numpy()), _bits(n)), 'normals'
    return len(fc)


def _check(p, nrm, o, h, depth, ref=None, convert=lambda a: a, **kw):
    """reconstruct == the restatement, twice in a row -> (Field, ref)"""
    if ref is None:
        ref = R.reconstruct(np.asarray(p, np.float64), np.asarray(nrm, np.float64), o, h, depth, **kw)
    f = None
    for _ in range(2):
        f = poisson.reconstruct(convert(p), convert(nrm), o, h, depth, **kw)
        _check_field(f, ref)
    return f, ref


@pytest.mark.parametrize('sweeps', [1, 2])
@pytest.mark.parametrize('cycles', [0, 1, 8])
@pytest.mark.parametrize('depth,n', [(2, 6), (3, 200), (4, 4000), (5, 20000)])
def test_reconstruct_equals_the_restatement(depth, n, cycles, sweeps):
    p, nrm, o, h = _cloud(depth, n)
    ref = _ref(depth, n, cycles, sweeps)
    assert ref['n_used'] == n
    f, _ = _check(p, nrm, o, h, depth, ref=ref, convert=lambda a: torch.from_numpy(a).cuda(), cycles=cycles, sweeps=sweeps)
    for _ in range(2):
        faces = _check_mesh(f.mesh(), ref)
    if cycles == 0:
        assert not f.chi.any() and f.iso == 0.0 and f.residual == f.residual0 > 0 and f.mesh() is None and f.mesh(trim=False) is None
    elif cycles == 8 and depth >= 4:
        assert faces > 100 and (sweeps < 2 or f.residual / f.residual0 <= 1e-6)   # the default's bound (tests/test_poisson_host.py); one sweep gives 2e-6
        _check_mesh(f.mesh(trim=False), ref, trim=False)


def test_edge_points():
    """f = 0, the first and the last admitted cell on every axis, points just outside (counted, and nothing else changes)"""
    depth = 3
    o, h = np.array([-1.0, 0.5, 2.0]), 0.25
    N = 2 ** depth + 1
    g = np.array([[3.0, 4.0, 2.0],                                              # a lattice point
                  [1.0, 1.0, 1.0], [1.25, 1.5, 1.75], [N - 3 + 0.75, N - 3 + 0.5, N - 3 + 0.25],
                  [1.5, N - 3 + 0.5, 3.5], [N - 3 + 0.999, 1.001, 4.0], [4.5, 4.25, 4.125], [2.75, 5.5, 3.25]])
    rs = np.random.RandomState(5)
    nrm = rs.normal(size=g.shape)
    inside = o + g * h
    f, ref = _check(inside, nrm, o, h, depth)
    assert ref['n_used'] == len(g) and ref['n_outside'] == 0
    _check_mesh(f.mesh(), ref)
    out_g = np.array([[0.999, 3.0, 3.0], [3.0, 0.5, 3.0], [3.0, 3.0, -2.0], [float(N - 2), 3.0, 3.0], [3.0, N - 2 + 0.5, 3.0], [3.0, 3.0, 1e6],
                      [-1e300, 3.0, 3.0]])
    both = np.concatenate([inside[:4], o + out_g * h, inside[4:]])
    nb = np.concatenate([nrm[:4], rs.normal(size=out_g.shape), nrm[4:]])
    f2, ref2 = _check(both, nb, o, h, depth)
    assert ref2['n_outside'] == len(out_g) and f2.n_outside == len(out_g)
    for name in ('chi', 'density', 'values'):
        assert np.array_equal(_bits(ref2[name]), _bits(ref[name])), name
    assert _fbits(ref2['iso']) == _fbits(ref['iso'])
    f3, ref3 = _check(o + out_g * h, nb[4:4 + len(out_g)], o, h, depth)         # nothing admitted at all
    assert f3.n_used == 0 and np.isnan(f3.iso) and f3.mesh() is None and not f3.chi.any() and not f3.density.any()


def test_single_point_zero_normals_and_copies():
    depth = 3
    o, h = R.unit_grid(depth)
    p1, n1 = np.array([[0.13, -0.21, 0.4]]), np.array([[0.6, 0.0, -0.8]])
    f, ref = _check(p1, n1, o, h, depth)
    assert ref['n_used'] == 1 and ref['residual0'] > 0
    _check_mesh(f.mesh(), ref)
    p, nrm, _, _ = _cloud(depth, 200)
    nz = nrm.copy()
    nz[::3] = 0.0
    f, ref = _check(p, nz, o, h, depth)
    _check_mesh(f.mesh(), ref)
    f, ref = _check(p, np.zeros_like(nrm), o, h, depth)                         # density, but no field: chi = 0
    assert ref['residual0'] == 0 and not f.chi.any() and f.density.any() and f.mesh() is None
    # heavy contention on eight addresses: the integer sums are exact
    f, ref = _check(np.repeat(p1, 5000, 0), np.repeat(n1, 5000, 0), o, h, depth)
    one = R.splat(p1, n1, o, h, 2 ** depth + 1)[0]
    assert np.array_equal(f.density.cpu().numpy(), (one[3] * 5000).astype(np.float64) * 2.0 ** -32)


def test_quantisation_ties():
    """w = 0.5 exactly (f = (0.5, 0, 0)) and normals of odd multiples of 2^-32: (w * n_a) * 2^32 lands on .5 with either sign and rounds to even"""
    depth = 3
    o, h = R.unit_grid(depth)
    p = np.array([[o[0] + 3.5 * h, o[1] + 4 * h, o[2] + 2 * h]] * 4)
    nrm = np.array([[3.0, -3.0, 5.0], [-5.0, 7.0, -7.0], [1.0, -1.0, 9.0], [2.0 ** 31 + 1, -(2.0 ** 31 + 3), 11.0]]) * 2.0 ** -32
    V = R.splat(p, nrm, o, h, 2 ** depth + 1)[0]
    assert V[0, 3, 4, 2] == 2 - 2 + 0 + 2 ** 30 and V[1, 3, 4, 2] == -2 + 4 - 0 - (2 ** 30 + 2) and V[2, 4, 4, 2] == 2 - 4 + 4 + 6
    f, ref = _check(p, nrm, o, h, depth, cycles=2)
    assert ref['residual0'] > 0


@pytest.mark.parametrize('n', [1, 2047, 2048, 2049])
def test_point_counts_around_the_tree_chunk(n):
    depth = 3
    p, nrm = R.sphere_cloud(n, seed=n)
    o, h = R.unit_grid(depth)
    _check(p, nrm, o, h, depth, cycles=2)


def test_input_kinds():
    depth = 3
    p, nrm, o, h = _cloud(depth, 200)
    p32, n32 = p.astype(np.float32), nrm.astype(np.float32)
    ref32 = R.reconstruct(p32.astype(np.float64), n32.astype(np.float64), o, h, depth)
    _check(p32, n32, o, h, depth, ref=ref32)                                    # numpy fp32
    _check(p32, n32, o, h, depth, ref=ref32, convert=lambda a: torch.from_numpy(a).cuda())
    wide = torch.from_numpy(np.concatenate([p, nrm], 1)).cuda()                 # non-contiguous views of one [n, 6] tensor
    ref = _ref(depth, 200, 8, 2)
    for _ in range(2):
        _check_field(poisson.reconstruct(wide[:, :3], wide[:, 3:], torch.from_numpy(o), h, depth), ref)
    _check_field(poisson.reconstruct(torch.from_numpy(p), nrm, list(o), h, depth), ref)       # a CPU tensor beside a numpy array
    for bad in (np.nan, np.inf, -np.inf):
        q = p.copy()
        q[17, 1] = bad
        with pytest.raises(ValueError):
            poisson.reconstruct(q, nrm, o, h, depth)
        with pytest.raises(ValueError):
            poisson.reconstruct(p, q, o, h, depth)
    m, f = poisson.poisson_mesh(p, nrm, depth=depth, scale=1.25)
    o2, h2 = poisson.poisson_grid(p.min(0), p.max(0), depth, 1.25)
    ref2 = R.reconstruct(p, nrm, o2, h2, depth)
    _check_field(f, ref2)
    _check_mesh(m, ref2)


@pytest.mark.parametrize('depth,n', [(3, 200), (5, 20000)])
def test_valid_masks(depth, n):
    p, nrm, o, h = _cloud(depth, n)
    ref = _ref(depth, n, 8, 2)
    f = poisson.reconstruct(p, nrm, o, h, depth)
    some = float(np.median(ref['density'][ref['density'] > 0]))
    for min_density in (0.0, some):
        for dilate in (0, 1, 2):
            want = R.valid(ref, min_density, dilate)
            for _ in range(2):
                got = f.valid(min_density, dilate)
                assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want), (min_density, dilate)
            _check_mesh(f.mesh(min_density, dilate), ref, min_density=min_density, dilate=dilate)
    assert R.valid(ref, some, 0).sum() < R.valid(ref, 0.0, 0).sum() < R.valid(ref, 0.0, 1).sum() < R.valid(ref, 0.0, 2).sum()
    for kw in (dict(dilate=-1), dict(dilate=1.0), dict(min_density=np.nan)):
        with pytest.raises(ValueError):
            f.valid(**kw)


# ---------------------------------------------------------------- normals of the fused cloud ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _views(hw, holes):
    return S.make_views(6, hw, clean=True, hole_frac=0.1 if holes else None)


def _fused_fields(fu):
    return {k: getattr(fu, k) for k in ('points', 'colors', 'view', 'pixel', 'masked_depths', 'fused_depths', 'counts')}


def _ref_normals(fu, cams, jump):
    return NR.depth_normals(fu.fused_depths.cpu().numpy(), fu.view.cpu().numpy(), fu.pixel.cpu().numpy(), cams, jump)


@pytest.mark.parametrize('holes', [False, True])
@pytest.mark.parametrize('hw', [(20, 28), (37, 53)])
def test_fused_normals_equal_the_restatement(hw, holes):
    cams, depths, pairs = _views(hw, holes)
    plain = fusion.fuse_depths(cams, depths, pairs)
    assert plain.normals is None and len(plain) > 100
    for jump in (0.05, np.inf, 0.0):
        for _ in range(2):
            fu = fusion.fuse_depths(cams, depths, pairs, normals=True, normal_jump=jump)
            for k, v in _fused_fields(plain).items():                           # asking for normals changes nothing else
                assert v is None and getattr(fu, k) is None or torch.equal(getattr(fu, k), v), k
            want = _ref_normals(fu, cams, jump)
            assert fu.normals.dtype == torch.float64 and np.array_equal(_bits(fu.normals.cpu().numpy()), _bits(want)), jump
            assert np.array_equal(_bits(fusion.depth_normals(plain, cams, jump).cpu().numpy()), _bits(want))
    if holes:
        assert (_ref_normals(plain, cams, 0.05) == 0).all(1).any()              # a kept pixel that lost both neighbours along an axis
    # clean_fused carries the normals through its compaction and the cleaned maps give the cleaned cloud's normals
    fu = fusion.fuse_depths(cams, depths, pairs, normals=True)
    cl = cloud.clean_fused(fu, nb_neighbors=8)
    keep = cl.cleaned.keep.cpu().numpy() != 0
    assert 0 < keep.sum() and len(cl) == keep.sum() and torch.equal(cl.normals, fu.normals[torch.from_numpy(keep).cuda()])
    assert torch.equal(cl.view, fu.view[torch.from_numpy(keep).cuda()])
    assert np.array_equal(_bits(fusion.depth_normals(cl, cams).cpu().numpy()), _bits(_ref_normals(cl, cams, 0.05)))
    assert cloud.clean_fused(plain, nb_neighbors=8).normals is None


def test_normals_at_borders_lonely_pixels_and_depth_steps():
    """a hand-made fused depth map in which every pixel is a point: the image border (one-sided tangents), a pixel with no kept neighbour (no
    normal), a relative depth step of 20 % that jump = 0.05 refuses and jump = inf crosses"""
    cams, _, _ = _views((20, 28), False)
    V, H, W = 2, 20, 28
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    d = np.stack([2.4 + 0.01 * xx + 0.02 * yy + 0.003 * np.sin(xx * 0.9) * yy, 2.6 - 0.015 * xx + 0.01 * yy]).astype(np.float32)
    d[0, :, 15:] *= np.float32(1.2)                                             # the step between columns 14 and 15 of view 0
    keep = d[1, 6, 8]
    d[1, 4:9, 6:11] = 0
    d[1, 6, 8] = keep                                                           # alone in a hole
    d[1, 12, 3] = d[1, 12, 5] = 0                                               # (12, 4) keeps its neighbours above and below only
    view, pix = [a.astype(np.int32) for a in np.nonzero(d.reshape(V, -1) > 0)]
    dev = torch.device('cuda')
    fu = fusion.Fused(torch.zeros(len(view), 3, dtype=torch.float64, device=dev), None, torch.from_numpy(view).to(dev), torch.from_numpy(pix).to(dev),
                      None, torch.from_numpy(d).to(dev), None)
    got = {}
    for jump in (0.05, np.inf, 0.25, 0.0):
        want = NR.depth_normals(d, view, pix, cams[:V], jump)
        for _ in range(2):
            got[jump] = fusion.depth_normals(fu, cams[:V], jump).cpu().numpy()
            assert np.array_equal(_bits(got[jump]), _bits(want)), jump
    at = lambda v, y, x: int(np.nonzero((view == v) & (pix == y * W + x))[0][0])     # noqa: E731
    zero = lambda a: (a == 0).all(1)                                            # noqa: E731
    assert zero(got[0.05])[[at(1, 6, 8), at(1, 12, 4)]].all() and zero(got[np.inf])[[at(1, 6, 8), at(1, 12, 4)]].all()
    border = (pix // W == 0) | (pix // W == H - 1) | (pix % W == 0) | (pix % W == W - 1)
    assert border.sum() > 150 and not zero(got[0.05])[border].any()
    step = (view == 0) & ((pix % W == 14) | (pix % W == 15))
    assert (got[0.05][step] != got[np.inf][step]).any(1).all() and np.array_equal(got[0.05][~step], got[np.inf][~step])
    assert np.array_equal(got[0.25], got[np.inf]) and not zero(got[0.05])[step].any()
    lens = np.linalg.norm(got[0.05], axis=1)
    assert np.allclose(lens[~zero(got[0.05])], 1.0, atol=1e-12)
    assert zero(got[0.0]).sum() > zero(got[0.05]).sum()                         # no two neighbouring depths are equal here
    for bad in (np.nan, -0.1):
        with pytest.raises(ValueError):
            fusion.depth_normals(fu, cams[:V], bad)
    with pytest.raises(ValueError):
        fusion.depth_normals(fu, cams[:3], 0.05)
    off = fusion.Fused(fu.points, None, fu.view, fu.pixel + H * W, None, fu.fused_depths, None)
    with pytest.raises(ValueError):
        fusion.depth_normals(off, cams[:V], 0.05)


@pytest.mark.parametrize('hw,measured', [((20, 28), 9.13), ((37, 53), 16.91)])
def test_normals_are_accurate_on_the_clean_sphere(hw, measured):
    """The largest angle between a normal and the sphere's radial direction, measured with the restatement on the CPU: 9.13 degrees at 20 x 28 and
    16.91 degrees at 37 x 53 (both at the silhouette, where a texel spans the steepest depth change); 0.62 % / 0.70 % of the points have no normal.
    Twice the angle is asserted: the margin is for another seed and says nothing about precision, the device equals the restatement anyway."""
    cams, depths, pairs = _views(hw, False)
    fu = fusion.fuse_depths(cams, depths, pairs, normals=True)
    n = fu.normals.cpu().numpy()
    none = (n == 0).all(1)
    assert none.mean() <= 0.05
    rad = fu.points.cpu().numpy() - S.CENTER
    rad /= np.linalg.norm(rad, axis=1, keepdims=True)
    angle = np.degrees(np.arccos(np.clip((n * rad).sum(1)[~none], -1.0, 1.0)))
    print('largest angle %.3f degrees, %.3f %% without a normal' % (angle.max(), 100 * none.mean()))
    assert angle.max() <= 2 * measured


# ---------------------------------------------------------------- the commands ----------------------------------------------------------------
def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_' + name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_commands_end_to_end(tmp_path, capsys):
    root, _ = S.write_mvs_scene(tmp_path / 'scene', n_views=4, depth_hw=(20, 28), img_wh=(96, 72))
    _tool('fusion').main(['--data', root, '--normals'])
    ply = os.path.join(root, 'all_torch.ply')
    pts, nrm = chamfer.load_oriented_points(ply)
    assert len(pts) > 100 and nrm is not None and 'normals: ' in capsys.readouterr().out
    lens = np.linalg.norm(nrm, axis=1)
    assert (lens > 0).mean() > 0.5 and np.allclose(lens[lens > 0], 1.0, atol=1e-6)     # the probability mask punches holes: 26 % have no normal
    depth, dilate, scale = 4, 1, 1.3                                            # at depth 4 a scale of 1.1 leaves the outermost cell unadmitted
    out = str(tmp_path / 'poisson.ply')
    _tool('poisson_mesh').main([ply, out, '--depth', str(depth), '--dilate', str(dilate), '--scale', str(scale)])
    printed = capsys.readouterr().out
    assert 'points: %d used, 0 outside' % len(pts) in printed and 'residual / residual0' in printed and 'isovalue' in printed
    m = M.load_mesh(out)
    assert len(m) > 50 and ('%d faces' % len(m)) in printed
    _, h = poisson.poisson_grid(pts.min(0), pts.max(0), depth, scale)
    v = m.vertices.cpu().numpy().astype(np.float64)
    near = np.sqrt(((v[:, None, :] - pts[None]) ** 2).sum(-1).min(1))
    assert near.max() <= (dilate + 1 + np.sqrt(3.0)) * h * (1 + 1e-6)           # the derivable bound; the slack is the file's fp32 coordinates
    # the cleaned cloud keeps its normals, and --data fuses and reconstructs in one command
    cut = str(tmp_path / 'cut.ply')
    _tool('clean_points').main([ply, cut, '--nb_neighbors', '8'])
    cp, cn = chamfer.load_oriented_points(cut)
    assert cn is not None and 0 < len(cp) <= len(pts)
    rows = {tuple(r): i for i, r in enumerate(pts)}
    assert all(np.array_equal(nrm[rows[tuple(r)]], q) for r, q in zip(cp, cn))
    obj = str(tmp_path / 'direct.obj')
    _tool('poisson_mesh').main(['--data', root, obj, '--depth', str(depth), '--largest', '--no_trim'])
    assert len(M.load_mesh(obj)) > 50
