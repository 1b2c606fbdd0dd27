"""On-device DTU Chamfer evaluation (mvsdf_amd/chamfer.py, csrc/chamfer.hip) against the restatement tests/chamfer_ref.py and the fixtures
tests/golden/chamfer/*.npz (DTUeval-python's formulation under the seeded order): samples, kept sets, masks and every distance bit for bit."""
import glob
import os

import numpy as np
import pytest
import torch

import chamfer_ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, 'chamfer', '*.npz')))


def _fixture(path):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def _np(t):
    return t.cpu().numpy()


def _mesh(v, f):
    from mvsdf_amd.mesh import Mesh
    v = torch.from_numpy(np.asarray(v, np.float32))
    return Mesh(v, torch.from_numpy(np.asarray(f, np.int32)), torch.zeros_like(v)).to('cuda')


def _args(z):
    return dict(density=float(z['density']), patch=z['patch'].item(), max_dist=float(z['max_dist']), seed=int(z['seed']))


def _same_dist(a, b):
    """bit-identical, +inf in the same places"""
    return a.shape == b.shape and np.array_equal(np.isinf(a), np.isinf(b)) and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize('path', FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_fixture_every_step(path):
    from mvsdf_amd import chamfer as C
    z = _fixture(path)
    a = _args(z)
    if 'verts' in z:
        pts = C.sample_mesh(_mesh(z['verts'], z['faces']), a['density'])
        assert np.array_equal(_np(pts).view(np.int64), z['samples'].view(np.int64))
        geom = _mesh(z['verts'], z['faces'])
    else:
        pts = torch.from_numpy(z['points']).cuda()
        geom = pts
    kept = C.downsample(pts, a['density'], a['seed'])
    assert np.array_equal(_np(kept), z['kept'])
    d_in, d_obs, s_above = C.masks(pts, kept, z['stl'], z['obs_mask'], z['bb'], float(z['res']), z['plane'], a['patch'])
    d = z['samples'][z['kept']]
    assert np.array_equal(_np(d_in), d[z['in']]) and np.array_equal(_np(d_obs), d[z['obs']]) and np.array_equal(_np(s_above), z['stl'][z['above']])
    r = C.dtu_chamfer(geom, z['stl'], z['obs_mask'], z['bb'], float(z['res']), z['plane'], return_distances=True, **a)
    want = chamfer_ref.dtu_chamfer(z.get('points'), z['stl'], z['obs_mask'], z['bb'], float(z['res']), z['plane'], verts=z.get('verts'),
                                   faces=z.get('faces'), **a)
    for name in ('d2s', 's2d'):
        got = _np(r['dist_' + name])
        assert _same_dist(got, want['dist_' + name])
        fix = z['dist_' + name]
        assert np.array_equal(np.isinf(got), np.isinf(fix))
        fin = np.isfinite(fix)
        assert np.all(np.abs(got[fin] - fix[fin]) <= 1e-12 * np.abs(fix[fin]))
        assert abs(r['mean_' + name] - float(z['mean_' + name])) <= 1e-12 * abs(float(z['mean_' + name]))
    assert abs(r['overall'] - float(z['overall'])) <= 1e-12 * abs(float(z['overall']))
    for k in ('n_points', 'n_down', 'n_in', 'n_obs', 'n_stl_above', 'n_d2s_used', 'n_s2d_used'):
        assert r[k] == want[k], k
    again = C.dtu_chamfer(geom, z['stl'], z['obs_mask'], z['bb'], float(z['res']), z['plane'], return_distances=True, **a)
    for k in ('mean_d2s', 'mean_s2d', 'overall'):
        assert np.float64(again[k]).view(np.int64) == np.float64(r[k]).view(np.int64)
    assert torch.equal(again['dist_d2s'], r['dist_d2s']) and torch.equal(again['dist_s2d'], r['dist_s2d'])


def _cases():
    rs = np.random.RandomState(5)
    chain = np.zeros((3000, 3))
    chain[:, 0] = np.arange(3000) * 0.18                         # 0.9 * density
    pair = np.array([[0.0, 0, 0], [0.2, 0, 0], [0.4, 0, 0], [0.4, 0.2, 0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.2]])
    return {'cloud': rs.uniform(-3, 3, (20000, 3)) * [1, 1, 0.2], 'one_cell': rs.uniform(0, 0.1, (700, 3)), 'chain': chain, 'pairs': pair,
            'outliers': np.concatenate([rs.uniform(-1, 1, (3000, 3)), [[1e7, 0, 0], [-3e6, 2e6, 1.0]]])}


@pytest.mark.parametrize('name', list(_cases()))
@pytest.mark.parametrize('seed,density', [(0, 0.2), (1, 0.2), (12345, 0.05), (2 ** 64 - 1, 0.5)])
def test_downsample_matches_the_greedy_loop(name, seed, density):
    from mvsdf_amd import chamfer as C
    p = _cases()[name]
    got = _np(C.downsample(torch.from_numpy(p).cuda(), density, seed))
    assert np.array_equal(got, chamfer_ref.downsample(p, density, seed))


def _near_far_queries(rs, refs, n, max_dist):
    """half far from everything, the rest around the references, 40 at max_dist -+ k ulps along an axis from the isolated reference (300, 300, 300),
    where 300 -+ (max_dist + k 2^-44) is exact"""
    far = rs.uniform(-1, 1, (n // 2, 3)) * 200 + [500.0, -500.0, 0]
    near = refs[rs.randint(0, len(refs), n // 2 - 40)] + rs.randn(n // 2 - 40, 3) * 0.5
    iso = refs[-1]
    edge = []
    for k in range(-10, 10):
        edge.append(iso + [max_dist + k * 2.0 ** -44, 0, 0])
        edge.append(iso - [0, max_dist + k * 2.0 ** -44, 0])
    return np.concatenate([far, near, np.array(edge)])


@pytest.mark.parametrize('seed', [0, 1])
def test_nearest_bit_identical(seed):
    from mvsdf_amd import chamfer as C
    rs = np.random.RandomState(seed)
    refs = np.concatenate([rs.uniform(-10, 10, (30000, 3)) * [1, 1, 0.1], [[300.0, 300.0, 300.0]]])
    max_dist = 2.0
    q = _near_far_queries(rs, refs, 6000, max_dist)
    got = _np(C.nearest_distance(torch.from_numpy(q).cuda(), torch.from_numpy(refs).cuda(), max_dist))
    want = chamfer_ref.nearest(q, refs, max_dist, chunk=64)
    assert _same_dist(got, want)
    assert np.isinf(got[:3000]).all() and np.isfinite(got[3000:5960]).mean() > 0.99
    edge = got[-40:].reshape(20, 2)
    assert np.isfinite(edge[:10]).all() and np.isinf(edge[10:]).all()                   # d = max_dist + k 2^-44: finite exactly for k < 0
    got2 = _np(C.nearest_distance(torch.from_numpy(q).cuda(), torch.from_numpy(refs).cuda(), max_dist))
    assert np.array_equal(got.view(np.int64), got2.view(np.int64))


@pytest.mark.parametrize('nr', [1, 15, 16, 17, 129, 2049])
def test_nearest_at_the_tree_shape_edges(nr):
    """one leaf, a leaf's edge, a partly filled last child at two and at three levels: the descent and the walk where the tree is smallest"""
    from mvsdf_amd import chamfer as C
    rs = np.random.RandomState(100 + nr)
    refs = rs.uniform(-1, 1, (nr, 3)) * [1.0, 0.6, 0.3]
    max_dist = 0.5
    around = rs.uniform(-1.3, 1.3, (180, 3)) * [1.0, 0.6, 0.3]
    own = refs[rs.permutation(nr)[:100]]
    beyond = rs.uniform(-1, 1, (20, 3)) + [5.0, -4.0, 3.0]
    q = np.concatenate([around, own, beyond])
    got = _np(C.nearest_distance(torch.from_numpy(q).cuda(), torch.from_numpy(refs).cuda(), max_dist))
    want = chamfer_ref.nearest(q, refs, max_dist, chunk=64)
    assert _same_dist(got, want)
    assert (got[180:180 + len(own)] == 0).all() and np.isinf(got[-20:]).all()
    got2 = _np(C.nearest_distance(torch.from_numpy(q).cuda(), torch.from_numpy(refs).cuda(), max_dist))
    assert np.array_equal(got.view(np.int64), got2.view(np.int64))


def test_nearest_duplicates_and_one_reference():
    from mvsdf_amd import chamfer as C
    refs = np.array([[1.0, 2.0, 3.0]] * 40)
    q = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 4.0], [1.0, 2.0, 23.0], [1.0, 2.0, 22.999]])
    got = _np(C.nearest_distance(q, refs, 20.0))
    assert _same_dist(got, chamfer_ref.nearest(q, refs, 20.0, chunk=4))
    assert got[0] == 0 and got[1] == 1 and np.isinf(got[2]) and np.isfinite(got[3])
    got = _np(C.nearest_distance(q, refs[:1], 20.0))
    assert _same_dist(got, chamfer_ref.nearest(q, refs[:1], 20.0, chunk=4))


def test_concentric_spheres():
    """a sphere mesh of radius r against stl points on radius r + delta: both means are delta within a few percent"""
    from mvsdf_amd import chamfer as C
    from mvsdf_amd import mesh as M
    r, delta = 50.0, 1.0
    g = np.linspace(-1.2 * r, 1.2 * r, 160)
    x, y, z = np.meshgrid(g, g, g, indexing='ij')
    mesh = M.marching_cubes(torch.from_numpy(np.sqrt(x * x + y * y + z * z) - r).float().cuda(), 0.0, spacing=(g[1] - g[0],) * 3, origin=(g[0],) * 3)
    rs = np.random.RandomState(0)
    d = rs.randn(200000, 3)
    stl = (r + delta) * d / np.linalg.norm(d, axis=1, keepdims=True)
    obs = np.ones((30, 30, 30), bool)
    res = C.dtu_chamfer(mesh, stl, obs, [[-60.0] * 3, [60.0] * 3], 4.0, [0.0, 0.0, 0.0, 1.0], density=0.2, patch=60, max_dist=20.0)
    assert abs(res['mean_d2s'] - delta) < 0.05 * delta and abs(res['mean_s2d'] - delta) < 0.05 * delta
    assert res['n_d2s_used'] == res['n_obs'] > 0 and res['n_s2d_used'] == res['n_stl_above'] == len(stl)


def test_millions_of_points_invariants():
    """3 million points: the kept set's invariants on a random subset (int64 offsets, many cells, several rounds), and nearest distances on a subset"""
    from mvsdf_amd import chamfer as C
    rs = np.random.RandomState(3)
    n = 3_000_000
    p = rs.uniform(0, 1, (n, 3)) * [300.0, 300.0, 2.0]
    pt = torch.from_numpy(p).cuda()
    density, seed = 0.2, 9
    kept, n_kept, rounds = C._downsample(pt, density, seed, None)
    k = _np(kept).astype(bool)
    assert k.sum() == n_kept and rounds > 1
    keys = chamfer_ref.keys(n, seed)
    from scipy.spatial import cKDTree
    kp = p[k]
    tree = cKDTree(kp)
    kidx = np.nonzero(k)[0]
    sub = rs.randint(0, n, 20000)
    for i in sub:
        cand = tree.query_ball_point(p[i], density * 1.001)
        d = p[kidx[cand]] - p[i]
        within = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) <= density * density
        others = [j for j, w in zip(kidx[cand], within) if w and j != i]
        if k[i]:
            assert not others                                     # no other kept point within density
        else:
            assert any(keys[j] < keys[i] for j in others)        # removed by a lower-key kept neighbour
    q = p[sub[:2000]] + rs.randn(2000, 3)
    got = _np(C.nearest_distance(torch.from_numpy(q).cuda(), torch.from_numpy(kp).cuda(), 20.0))
    assert _same_dist(got, chamfer_ref.nearest(q, kp, 20.0))
    print('3e6 points: %d kept in %d rounds' % (n_kept, rounds))


def test_world_mesh_trim_chamfer_end_to_end():
    """extract_world_mesh -> Mesh.trim -> dtu_chamfer on the synthetic model, against the restatement"""
    from mvsdf_amd import chamfer as C
    from mvsdf_amd import evaluation as ev
    from mvsdf_amd.model.implicit_differentiable_renderer import IDRNetwork
    from mvsdf_amd.utils import synth
    from mvsdf_amd.utils.config import ConfigDict
    m = IDRNetwork(ConfigDict(synth.model_conf(64)))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(64, 0).items()})
    m = m.cuda().eval()
    scale = np.diag([40.0, 40.0, 40.0, 1.0])
    scale[:3, 3] = [10.0, -20.0, 600.0]
    mesh = ev.extract_world_mesh(m, scale, resolution=64)
    assert mesh is not None
    trimmed = mesh.trim(15, 10) or mesh
    v, f = _np(trimmed.vertices), _np(trimmed.faces)
    rs = np.random.RandomState(1)
    stl = v[rs.randint(0, len(v), 20000)].astype(np.float64) + rs.randn(20000, 3) * 0.5
    bb = np.stack([v.min(0) - 5, v.max(0) + 5]).astype(np.float32)
    obs = rs.rand(40, 40, 40) < 0.9
    res_ = float((bb[1] - bb[0]).max() / 39)
    plane = [0.0, 0.0, 1.0, -float(np.median(v[:, 2]))]
    got = C.dtu_chamfer(trimmed, stl, obs, bb, res_, plane, return_distances=True)
    want = chamfer_ref.dtu_chamfer(None, stl, obs, bb, res_, plane, verts=v, faces=f)
    assert _same_dist(_np(got['dist_d2s']), want['dist_d2s']) and _same_dist(_np(got['dist_s2d']), want['dist_s2d'])
    for k in ('n_points', 'n_down', 'n_in', 'n_obs', 'n_stl_above', 'n_d2s_used', 'n_s2d_used'):
        assert got[k] == want[k], k
    assert abs(got['overall'] - want['overall']) <= 1e-12 * abs(want['overall'])


def test_bad_input_and_round_limit():
    from mvsdf_amd import chamfer as C
    from mvsdf_amd._lib import MvsdfError
    good = np.random.RandomState(0).uniform(0, 1, (100, 3))
    for bad in (np.zeros((0, 3)), np.zeros((5, 2)), np.array([[0.0, np.nan, 0.0]] * 3), np.array([[0.0, 0.0, np.inf]] * 3)):
        with pytest.raises(ValueError):
            C.downsample(bad)
        with pytest.raises(ValueError):
            C.nearest_distance(good, bad)
        with pytest.raises(ValueError):
            C.nearest_distance(bad, good)
    with pytest.raises(ValueError):
        C.downsample(good, density=0.0)
    with pytest.raises(ValueError):
        C.nearest_distance(good, good, max_dist=-1.0)
    v = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0]], np.float32)
    with pytest.raises(ValueError):
        C.sample_mesh(_mesh(v, [[0, 1, 2]]), 0.2, max_points=100)                       # about 1250 points
    assert len(C.sample_mesh(_mesh(v, [[0, 1, 2]]), 0.2, max_points=10000)) > 100
    with pytest.raises(ValueError):
        C.sample_mesh(_mesh(v, [[0, 1, 3]]))                                            # a missing vertex
    vn = v.copy()
    vn[1, 0] = np.nan
    with pytest.raises(ValueError):
        C.sample_mesh(_mesh(vn, [[0, 1, 2]]))
    chain = np.zeros((500, 3))
    chain[:, 0] = np.arange(500) * 0.18
    with pytest.raises(MvsdfError):
        C.downsample(chain, 0.2, 0, max_rounds=1)
    z = _fixture(FIXTURES[0])
    with pytest.raises(ValueError):
        C.dtu_chamfer(torch.from_numpy(good).cuda(), np.array([[0.0, 0.0, np.nan]]), z['obs_mask'], z['bb'], 0.5, z['plane'])
    with pytest.raises(ValueError):
        C.dtu_chamfer(torch.from_numpy(good).cuda(), good, np.zeros((0, 2, 2), bool), z['bb'], 0.5, z['plane'])
