"""Poisson reconstruction without a GPU: the numpy restatement (tests/poisson_ref.py) on clouds whose surface is known, the tree sum, poisson_grid, the
PLY round trip with normals, the argument errors (raised before the device is touched) and the plumbing."""
import os
import re

import numpy as np
import pytest

import poisson_ref as R
from conftest import ROOT

_CACHE = {}


def _sphere(depth):
    """the restatement's result on the seeded sphere cloud: 4 000 points at depth 4, 20 000 at depth 5 (computed once, never changed)"""
    if depth not in _CACHE:
        p, n = R.sphere_cloud({4: 4000, 5: 20000}[depth])
        o, h = R.unit_grid(depth)
        _CACHE[depth] = (p, n, o, h, R.reconstruct(p, n, o, h, depth))
    return _CACHE[depth]


def _edge_counts(faces):
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), 1)
    return np.unique(e, axis=0, return_counts=True)[1]


def _nearest(v, p):
    return np.concatenate([np.sqrt(((v[i:i + 500, None, :].astype(np.float64) - p[None]) ** 2).sum(-1).min(1)) for i in range(0, len(v), 500)])


@pytest.mark.parametrize('depth', [4, 5])
def test_restatement_converges(depth):
    """measured: 4.1e-9 at depth 4, 2.4e-9 at depth 5 (about 0.1 per cycle); the bound leaves room for another cloud"""
    out = _sphere(depth)[4]
    assert out['n_outside'] == 0 and out['residual0'] > 0
    assert out['residual'] / out['residual0'] <= 1e-6


def test_sphere_mesh_is_closed_and_round():
    """measured: 3 512 faces, radii 0.5977 .. 0.6045 at h = 0.0625"""
    p, n, o, h, out = _sphere(5)
    v, f, _ = R.mesh(out)
    assert len(f) > 1000 and (_edge_counts(f) == 2).all()
    r = np.linalg.norm(v.astype(np.float64), axis=1)
    assert np.abs(r - 0.6).max() <= h / 4
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    assert (np.einsum('ij,ij->i', np.cross(b - a, c - a), a + b + c) > 0).all()    # the right-hand normals point outwards


def test_hemisphere_stays_open_at_the_rim():
    """a vertex sits on an edge between valid lattice points, a valid point is within `dilate` steps of one with density, and that one is a corner of
    a sample's cell: every vertex is within (dilate + 1 + sqrt 3) h of a sample (measured: 1.58 h)"""
    p, n, o, h, _ = _sphere(5)
    k = p[:, 2] > 0
    p, n = p[k], n[k]
    out = R.reconstruct(p, n, o, h, 5)
    bound = (1 + 1 + np.sqrt(3.0)) * h
    v, f, _ = R.mesh(out)
    assert len(f) > 500 and (_edge_counts(f) == 1).any()
    assert _nearest(v, p).max() <= bound
    v2, f2, _ = R.mesh(out, trim=False)
    assert len(f2) > len(f) and (_nearest(v2, p) > bound).any()


@pytest.mark.parametrize('n', [1, 2, 3, 2047, 2048, 2049, 5000])
def test_tree_sum(n):
    def literal(a):
        if len(a) == 1:
            return a[0]
        return literal(a[:len(a) // 2]) + literal(a[len(a) // 2:])

    a = np.random.RandomState(n).normal(size=n) * 10.0 ** np.random.RandomState(n + 1).randint(-8, 8, size=n)
    size = 1
    while size < n:
        size *= 2
    want = literal(list(np.concatenate([a, np.zeros(size - n)])))
    assert R.tree_sum(a) == want


def test_poisson_grid():
    from mvsdf_amd import poisson
    origin, h = poisson.poisson_grid([0.0, 0.0, 0.0], [2.0, 1.0, 0.5], 4, scale=1.0)
    assert h == 0.125 and np.array_equal(origin, [0.0, -0.5, -0.75]) and origin.dtype == np.float64
    origin, h = poisson.poisson_grid(np.array([-1.0, -1.0, -1.0]), np.array([1.0, 1.0, 1.0]), 5, scale=1.5)
    assert h == 3.0 / 32 and np.array_equal(origin, [-1.5, -1.5, -1.5])
    lo, hi = np.array([0.1, -0.2, 0.05]) - 0.7, np.array([0.1, -0.2, 0.05]) + 0.6
    origin, h = poisson.poisson_grid(lo, hi, 6)
    assert h == pytest.approx(1.1 * 1.3 / 64) and np.allclose(origin + 32 * h, (lo + hi) / 2)
    g = (np.stack([lo, hi]) - origin) / h                                       # the default scale keeps the whole box admitted
    assert (np.floor(g) >= 1).all() and (np.floor(g) <= 2 ** 6 + 1 - 3).all()
    for kw in (dict(depth=1), dict(depth=11), dict(depth=4.0), dict(depth=4, scale=0.9), dict(depth=4, scale=np.nan), dict(depth=4, scale=np.inf)):
        with pytest.raises(ValueError):
            poisson.poisson_grid(lo, hi, **kw)
    for bad_lo, bad_hi in (([0, 0], [1, 1]), ([0, 0, 0], [1, 1, np.nan]), ([0, 0, 2], [1, 1, 1]), ([0, 0, 0], [0, 0, 0])):
        with pytest.raises(ValueError):
            poisson.poisson_grid(bad_lo, bad_hi, 4)


def test_ply_round_trip_with_normals(tmp_path):
    from mvsdf_amd import chamfer, fusion
    rs = np.random.RandomState(0)
    pts, nrm = rs.normal(size=(7, 3)), rs.normal(size=(7, 3))
    col = rs.randint(0, 256, size=(7, 3)).astype(np.uint8)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)                    # noqa: E731
    for name, c, n in (('n', None, nrm), ('c', col, None), ('nc', col, nrm), ('p', None, None)):
        path = str(tmp_path / (name + '.ply'))
        fusion.save_points(path, pts, c, normals=n)
        got_p, got_n = chamfer.load_oriented_points(path)
        assert np.array_equal(got_p, f32(pts)) and np.array_equal(chamfer.load_points(path), f32(pts))
        assert got_n is None if n is None else np.array_equal(got_n, f32(nrm))
        if c is not None:
            vert = chamfer._ply_elements(path)['vertex']
            assert np.array_equal(np.stack([vert[k] for k in ('red', 'green', 'blue')], 1), col)
    # without normals the file is what it always was: this header, then x y z (r g b) records
    want = (b'ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\nproperty float y\nproperty float z\n'
            b'property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n')
    rec = np.empty(7, dtype=[('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('red', 'u1'), ('green', 'u1'), ('blue', 'u1')])
    for i, k in enumerate('xyz'):
        rec[k] = pts[:, i]
    for i, k in enumerate(('red', 'green', 'blue')):
        rec[k] = col[:, i]
    assert open(str(tmp_path / 'c.ply'), 'rb').read() == want + rec.tobytes()
    assert open(str(tmp_path / 'p.ply'), 'rb').read() == want.replace(b'property uchar red\nproperty uchar green\nproperty uchar blue\n', b'') + \
        pts.astype('<f4').tobytes()
    with pytest.raises(ValueError):
        fusion.save_points(str(tmp_path / 'bad.ply'), pts, normals=nrm[:5])


def test_argument_errors_need_no_device():
    from mvsdf_amd import poisson
    p, n = R.sphere_cloud(50)
    o, h = R.unit_grid(3)
    for args, kw in (((p, n, o, h, 1), {}), ((p, n, o, h, 11), {}), ((p, n, o, h, 3.0), {}), ((p, n, o, h, True), {}),
                     ((p[:, :2], n, o, h, 3), {}), ((p, n[:10], o, h, 3), {}), ((p.reshape(-1), n, o, h, 3), {}), ((p[:0], n[:0], o, h, 3), {}),
                     ((p.astype(np.int64), n, o, h, 3), {}), ((p, n.astype(np.float16), o, h, 3), {}),
                     ((p, n, o[:2], h, 3), {}), ((p, n, o * np.nan, h, 3), {}), ((p, n, o, 0.0, 3), {}), ((p, n, o, -1.0, 3), {}),
                     ((p, n, o, np.inf, 3), {}),
                     ((p, n, o, h, 3), dict(cycles=-1)), ((p, n, o, h, 3), dict(cycles=1.5)), ((p, n, o, h, 3), dict(sweeps=0)),
                     ((p, n, o, h, 3), dict(sweeps=2.0))):
        with pytest.raises(ValueError):
            poisson.reconstruct(*args, **kw)
    for kw in (dict(depth=0), dict(depth=12), dict(scale=0.5)):
        with pytest.raises(ValueError):
            poisson.poisson_mesh(p, n, **kw)
    with pytest.raises(ValueError):
        poisson.poisson_mesh(p * np.inf, n, depth=3)
    with pytest.raises(ValueError):
        R.reconstruct(p * np.nan, n, o, h, 3)


def test_plumbing():
    from mvsdf_amd import _lib, build
    assert 'poisson.hip' in build.SOURCES
    hdr = open(os.path.join(ROOT, 'include', 'mvsdf_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name, where in (('mvsdf_poisson_workspace_bytes', 'poisson.hip'), ('mvsdf_poisson_reconstruct', 'poisson.hip'), ('mvsdf_poisson_valid', 'poisson.hip'),
                        ('mvsdf_poisson_volume', 'poisson.hip'), ('mvsdf_fusion_normals_workspace_bytes', 'fusion.hip'),
                        ('mvsdf_fusion_normals', 'fusion.hip')):
        src = open(os.path.join(ROOT, 'mvsdf_amd', 'csrc', where)).read()
        assert name in _lib.EXPORTS and re.search(r'\b%s\s*\(' % name, hdr) and re.search(r'\b%s\s*\(' % name, src), name
    assert _lib.lib().mvsdf_poisson_workspace_bytes(100, 1) == 0 and _lib.lib().mvsdf_poisson_workspace_bytes(100, 11) == 0
    assert _lib.lib().mvsdf_poisson_workspace_bytes(0, 4) == 0
    assert _lib.lib().mvsdf_poisson_workspace_bytes(100, 4) >= 5 * 17 ** 3 * 8
