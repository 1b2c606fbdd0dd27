"""mvsdf_amd/normals.py without a GPU: every bad argument is refused before anything is launched, the build knows the kernels, the commands parse
their arguments, and the numpy restatement (tests/normals_ref.py) ALONE meets analytic surfaces, so that a wrong definition cannot pass the GPU
suite's bit-equality by being wrong twice.  The figures in the comments are this restatement's (Jacobi, index ties)."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normals_ref as R  # noqa: E402
from mvsdf_amd import build, normals  # noqa: E402

JOBS = 16


def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_' + name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ================================================================ arguments ================================================================
def test_the_build_knows_the_kernels():
    assert 'normals.hip' in build.SOURCES
    assert normals.SWEEPS == R.SWEEPS


@pytest.mark.parametrize('call', ['knn_indices', 'estimate_normals'])
def test_knn_arguments_are_refused_before_any_launch(call):
    f = getattr(normals, call)
    P = np.random.RandomState(0).uniform(size=(40, 3))
    for bad in (P.astype(np.float32), P[:, :2], P.reshape(-1), torch.from_numpy(P).float(), [[0.0, 0.0, 0.0]] * 40):
        with pytest.raises(ValueError):
            f(bad, 8)
    for k in (0, -1, 33, 2.5, True):
        with pytest.raises(ValueError):
            f(P, k)
    with pytest.raises(ValueError):
        f(P[:8], 8)                                                          # N < k + 1
    with pytest.raises(ValueError):
        f(P[:1], 1)


def test_orient_arguments_are_refused_before_any_launch():
    rs = np.random.RandomState(1)
    P, N = rs.uniform(size=(40, 3)), rs.normal(size=(40, 3))
    nb = rs.randint(0, 40, (40, 4)).astype(np.int32)
    C = rs.uniform(size=(3, 3))
    vis = np.ones((3, 40), np.uint8)
    f = normals.orient_normals
    for args in ((P.astype(np.float32), N, nb), (P, N.astype(np.float32), nb), (P, N[:39], nb), (P, N[:, :2], nb), (P, N, nb.astype(np.int64)),
                 (P, N, nb[:39]), (P, N, nb.reshape(-1)), (P, N, np.zeros((40, 33), np.int32)), (P, N, np.zeros((40, 0), np.int32))):
        with pytest.raises(ValueError):
            f(*args)
    for up in ((0, 0, np.nan), (np.inf, 0, 0), (0, 1), 'z', (0, 0, 1, 0)):
        with pytest.raises(ValueError):
            f(P, N, nb, up=up)
    for kw in (dict(centers=C), dict(visibility=vis), dict(centers=C, visibility=vis[:2]), dict(centers=C, visibility=vis[:, :39]),
               dict(centers=C, visibility=vis.astype(np.float64)), dict(centers=C.astype(np.float32), visibility=vis),
               dict(centers=C[:, :2], visibility=vis), dict(centers=C, visibility=np.zeros(39, np.int32)),
               dict(centers=C, visibility=np.zeros(40, np.float64)), dict(centers=C, visibility=(np.zeros(40, np.int64), np.zeros(0, np.int32))),
               dict(centers=C, visibility=(np.zeros(41, np.int64),))):
        with pytest.raises(ValueError):
            f(P, N, nb, **kw)
    g = normals.orient_to_views
    for args in ((P.astype(np.float32), N, C, vis), (P, N[:39], C, vis), (P, N, C[:, :2], vis), (P, N, C, vis[:2]), (P, N, C, vis[:, :39]),
                 (P, N, C, None), (P, N, C, np.zeros(39, np.int32))):
        with pytest.raises(ValueError):
            g(*args)


def test_estimate_normals_tool_parses_its_arguments():
    t = _tool('estimate_normals')
    a = t.parse_args(['in.ply', 'out.ply'])
    assert (a.input, a.output, a.k, a.orient, a.up) == ('in.ply', 'out.ply', 16, 'mst', [0.0, 0.0, 1.0])
    a = t.parse_args(['in.ply', 'out.ply', '--k', '9', '--orient', 'none', '--up', '0,-1,0.5'])
    assert (a.k, a.orient, a.up) == (9, 'none', [0.0, -1.0, 0.5])
    a = t.parse_args(['--colmap', 'sparse/0', 'out.ply'])
    assert (a.input, a.output, a.colmap, a.orient) == (None, 'out.ply', 'sparse/0', 'views')
    a = t.parse_args(['--data_root', 'mvs', 'out.ply', '--orient', 'mst'])
    assert (a.input, a.data_root, a.orient) == (None, 'mvs', 'mst')
    for bad in (['in.ply'], ['in.ply', 'out.obj'], ['in.ply', 'in.ply'], ['in.ply', 'out.ply', '--k', '0'], ['in.ply', 'out.ply', '--k', '33'],
                ['in.ply', 'out.ply', '--orient', 'views'], ['in.ply', 'out.ply', '--up', '0,0'], ['in.ply', 'out.ply', '--up', '0,0,nan'],
                ['in.ply', 'out.ply', '--up', 'a,b,c'], ['--colmap', 'm', 'in.ply', 'out.ply'], ['--colmap', 'm', '--data_root', 'd', 'out.ply'],
                ['--colmap', 'm', 'out.ply', '--orient', 'mst']):
        with pytest.raises(SystemExit):
            t.parse_args(bad)


def test_poisson_tool_takes_the_new_flag_and_is_unchanged_without_it():
    t = _tool('poisson_mesh')
    assert t.parse_args(['in.ply', 'out.ply']).estimate_normals is None
    assert t.parse_args(['in.ply', 'out.ply', '--estimate_normals']).estimate_normals == 16
    assert t.parse_args(['in.ply', 'out.ply', '--estimate_normals', '9']).estimate_normals == 9
    for bad in ('0', '33'):
        with pytest.raises(SystemExit):
            t.parse_args(['in.ply', 'out.ply', '--estimate_normals', bad])


# ================================================================ the restatement alone, on analytic surfaces ================================================================
def sphere(n, seed, noise=0.0):
    """-> (points, analytic outward normals)"""
    rs = np.random.RandomState(seed)
    x = rs.normal(size=(n, 3))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x * (1 + noise * rs.normal(size=(n, 1))), x


def torus(n, seed, R0=1.0, r0=0.35):
    rs = np.random.RandomState(seed)
    u, v = rs.uniform(0, 2 * np.pi, n), rs.uniform(0, 2 * np.pi, n)
    nrm = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], 1)
    return np.stack([R0 * np.cos(u), R0 * np.sin(u), np.zeros(n)], 1) + r0 * nrm, nrm


def angles(a, b):
    return np.degrees(np.arccos(np.clip(np.abs((a * b).sum(1)), 0, 1)))


SURFACES = {'sphere': lambda: sphere(4099, 1), 'noisy_sphere': lambda: sphere(4099, 2, 0.005), 'torus': lambda: torus(8209, 3)}
# median / maximum angle in degrees of this restatement against the analytic normal, always one component and 100 % outward:
#   k = 16: sphere 0.737 / 3.239, torus 1.435 / 7.105, noisy sphere 1.635 / 8.002;  k = 8: sphere 0.938 / 5.883, torus 1.693 / 7.628,
#   noisy sphere 3.260 / 17.038.  Asserted: median < 2 and maximum < 10 at k = 16 on the clean sphere and the torus.


@pytest.mark.parametrize('name', sorted(SURFACES))
@pytest.mark.parametrize('k', [8, 16])
def test_restatement_on_analytic_surfaces(name, k):
    P, want = SURFACES[name]()
    N, var, nb = R.estimate_normals(P, k, jobs=JOBS)
    out, labels, n_components, rounds = R.orient_normals(P, N, nb, up=(0, 0, 1))
    ang = angles(out, want)
    print(name, k, 'median %.3f max %.3f components %d rounds %d' % (np.median(ang), ang.max(), n_components, rounds))
    assert n_components == 1 and (labels == 0).all()
    assert ((out * want).sum(1) > 0).all()                                   # 100 % outward
    assert np.abs(np.sqrt((out * out).sum(1)) - 1).max() < 1e-15
    assert (var >= 0).all() and (var <= 1 / 3 + 1e-12).all()
    if k == 16 and name != 'noisy_sphere':
        assert np.median(ang) < 2 and ang.max() < 10


def test_restatement_two_components():
    a, na = sphere(2053, 4)
    b, nb_ = sphere(2053, 5)
    P = np.concatenate([a, b * 0.5 + np.array([3.0, 0, 0])])
    want = np.concatenate([na, nb_])
    N, _, nb = R.estimate_normals(P, 12, jobs=JOBS)
    out, labels, n_components, _ = R.orient_normals(P, N, nb)
    assert n_components == 2 and set(labels.tolist()) == {0, 2053}
    assert (labels[:2053] == 0).all() and (labels[2053:] == 2053).all()
    assert ((out * want).sum(1) > 0).all()


def test_restatement_view_rule():
    """a lower hemisphere seen from two centres below it: `up` = +z picks the rim, whose outward normal points slightly down, so the up rule turns the
    cap inward; the vote turns it outward.  And one exact tie, which falls back to the up rule."""
    P, want = sphere(4099, 6)
    keep = P[:, 2] < -0.2
    P, want = P[keep], want[keep]
    N, _, nb = R.estimate_normals(P, 12, jobs=JOBS)
    by_up, _, n_components, _ = R.orient_normals(P, N, nb)
    assert n_components == 1 and ((by_up * want).sum(1) < 0).all()           # the wrong way
    C = np.array([[0.5, 0.0, -4.0], [-0.5, 0.3, -5.0]])
    vis = np.ones((2, len(P)), np.uint8)
    by_views, _, _, _ = R.orient_normals(P, N, nb, centers=C, visibility=vis)
    assert ((by_views * want).sum(1) > 0).all()
    own = R.orient_to_views(P, by_up, C, vis)                                # per point: the points whose own views lie in front turn, the rest stay
    turned = (own * by_up).sum(1) < 0
    assert turned.sum() > len(P) // 2 and ((own * want).sum(1) > 0)[turned].all()
    # a tie: two points, two mirrored centres, one vote each way
    P2 = np.array([[0.0, 0, 0], [1.0, 0, 0]])
    N2 = np.array([[0.0, 0, 1], [0.0, 0, 1]])
    nb2 = np.array([[1], [0]], np.int32)
    C2 = np.array([[0.5, 0, 2.0], [0.5, 0, -2.0]])
    v2 = np.array([[1, 0], [0, 1]], np.uint8)
    for up, sign in (((0, 0, 1), 1.0), ((0, 0, -1), -1.0)):
        out, _, _, _ = R.orient_normals(P2, N2, nb2, up=up, centers=C2, visibility=v2)
        assert np.array_equal(out, sign * N2)
    assert np.array_equal(R.orient_to_views(P2, N2, C2, v2), np.array([[0.0, 0, 1], [0.0, 0, -1]]))
    assert np.array_equal(R.orient_to_views(P2, N2, C2, np.ones((2, 2), np.uint8)), N2)        # a tie per point: no flip


def test_restatement_knn_ties_go_to_the_lower_index():
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing='ij'), -1).reshape(-1, 3).astype(np.float64)
    idx, d2 = R.knn_indices(g, 6)
    i = 21                                                                   # (1, 1, 1): six neighbours at distance 1
    assert d2[i].tolist() == [1.0] * 6 and idx[i].tolist() == sorted(idx[i].tolist())
    idx3, _ = R.knn_indices(g, 3)
    assert np.array_equal(idx3, idx[:, :3])                                  # a shorter row is a prefix
    P = np.concatenate([g, g[:5]])                                           # duplicates: a neighbour at distance 0, by index
    idx, d2 = R.knn_indices(P, 2)
    assert idx[0, 0] == 64 and d2[0, 0] == 0 and idx[64, 0] == 0
