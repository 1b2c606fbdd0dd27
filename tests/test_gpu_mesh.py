"""On-device mesh extraction (mvsdf_amd/mesh.py, csrc/mesh_kernels.hip) against the numpy restatement tests/mc_ref.py: marching cubes bit for
bit, analytic spheres, edge cases, connected components and the model path of eval.py:109-125."""
import numpy as np
import pytest
import torch

import mc_ref

pytestmark = pytest.mark.gpu


def _np(t):
    return t.cpu().numpy()


def _check_equal(mesh, vol, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    v, f, n = mc_ref.marching_cubes(vol, level, spacing, origin)
    assert mesh is not None
    assert np.array_equal(_np(mesh.faces), f)
    assert np.array_equal(_np(mesh.vertices), v)
    assert np.abs(_np(mesh.normals) - n).max() <= 1e-6
    return v, f, n


def _random_volume(rs, shape):
    vol = rs.randn(*shape).astype(np.float32)
    vol[rs.rand(*shape) < 0.1] = 0.0                                  # values exactly at the level
    return vol


@pytest.mark.parametrize('shape', [(2, 2, 2), (5, 6, 7), (17, 31, 9), (33, 3, 40), (64, 64, 64)])
def test_random_volumes_match_the_restatement(shape):
    from mvsdf_amd.mesh import marching_cubes
    rs = np.random.RandomState(sum(shape))
    for level, sp, org in [(0.0, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)), (0.25, (0.1, 0.02, 0.3), (-1.0, 0.5, 2.0))]:
        vol = _random_volume(rs, shape)
        if not ((vol < level).any() and (vol >= level).any()):
            vol.flat[0] = level - 1.0
            vol.flat[-1] = level + 1.0
        mesh = marching_cubes(torch.from_numpy(vol).cuda(), level, sp, org)
        _check_equal(mesh, vol, level, sp, org)
        again = marching_cubes(torch.from_numpy(vol).cuda(), level, sp, org)
        for a, b in [(mesh.vertices, again.vertices), (mesh.faces, again.faces), (mesh.normals, again.normals)]:
            assert torch.equal(a, b)                                  # two runs: the same bits


def test_strided_view_equals_its_contiguous_copy():
    from mvsdf_amd.mesh import marching_cubes
    rs = np.random.RandomState(3)
    base = torch.from_numpy(_random_volume(rs, (23, 17, 29))).cuda()
    view = base.permute(1, 0, 2)                                      # the (y, x, z) layout of plots.surface_volume
    assert not view.is_contiguous()
    a = marching_cubes(view, 0.0, (0.5, 0.5, 0.5), (-1.0, -1.0, -1.0))
    b = marching_cubes(view.contiguous(), 0.0, (0.5, 0.5, 0.5), (-1.0, -1.0, -1.0))
    for x, y in [(a.vertices, b.vertices), (a.faces, b.faces), (a.normals, b.normals)]:
        assert torch.equal(x, y)
    _check_equal(a, _np(view.contiguous()), 0.0, (0.5, 0.5, 0.5), (-1.0, -1.0, -1.0))
    view2 = base[::2, 1:, ::3]
    _check_equal(marching_cubes(view2), _np(view2.contiguous()))


def _sphere_volume(n, r=0.6, center=(0.0, 0.0, 0.0)):
    x = np.linspace(-1.0, 1.0, n)
    X, Y, Z = np.meshgrid(x, x, x, indexing='ij')
    d = np.sqrt((X - center[0]) ** 2 + (Y - center[1]) ** 2 + (Z - center[2]) ** 2) - r
    return d.astype(np.float32), x


@pytest.mark.parametrize('n', [128, 257])
def test_sphere(n):
    from mvsdf_amd.mesh import marching_cubes
    r = 0.6
    vol, x = _sphere_volume(n, r)
    h = x[1] - x[0]
    mesh = marching_cubes(torch.from_numpy(vol).cuda(), 0.0, (h,) * 3, (x[0],) * 3)
    v, f, nrm = _np(mesh.vertices), _np(mesh.faces).astype(np.int64), _np(mesh.normals)
    assert mc_ref.directed_edges_ok(f, len(v))
    assert abs(mesh.area() / (4 * np.pi * r * r) - 1) < 5e-3
    assert abs(mc_ref.signed_volume(v, f) / (4 / 3 * np.pi * r ** 3) - 1) < 5e-3
    rad = np.linalg.norm(v.astype(np.float64), axis=1)
    # linear interpolation of |p| - r along an edge: the error is the chord sag, at most h^2 / (8 r) (~6e-5 h-relative at n = 257)
    assert np.abs(rad - r).max() < 0.02 * h
    assert ((nrm * v / rad[:, None]).sum(1)).min() > 0.999


def test_no_crossing_gives_none():
    from mvsdf_amd.mesh import marching_cubes
    assert marching_cubes(torch.ones(8, 9, 10, device='cuda')) is None
    assert marching_cubes(-torch.ones(8, 9, 10, device='cuda')) is None
    assert marching_cubes(torch.zeros(8, 9, 10, device='cuda')) is None     # nothing is below the level


def test_non_finite_input_raises():
    from mvsdf_amd.mesh import marching_cubes
    vol, _ = _sphere_volume(20)
    for bad in (np.nan, np.inf):
        v = vol.copy()
        v[3, 4, 5] = bad
        with pytest.raises(ValueError):
            marching_cubes(torch.from_numpy(v).cuda())


def test_box_with_faces_on_grid_planes():
    from mvsdf_amd.mesh import marching_cubes
    x = np.linspace(-1.0, 1.0, 41)                                   # grid planes at multiples of 0.05
    X, Y, Z = np.meshgrid(x, x, x, indexing='ij')
    q = np.abs(np.stack([X, Y, Z])) - np.array([0.5, 0.3, 0.7])[:, None, None, None]
    box = (np.linalg.norm(np.maximum(q, 0), axis=0) + np.minimum(q.max(0), 0)).astype(np.float32)
    box[np.abs(box) < 1e-6] = 0.0
    assert (box == 0).sum() > 1000                                    # many values exactly at the level
    h = x[1] - x[0]
    mesh = marching_cubes(torch.from_numpy(box).cuda(), 0.0, (h,) * 3, (x[0],) * 3)
    v, f, _ = _check_equal(mesh, box, 0.0, (h,) * 3, (x[0],) * 3)
    assert mc_ref.directed_edges_ok(f, len(v))
    assert mc_ref.signed_volume(v, f) > 0


def test_three_spheres_three_components():
    from mvsdf_amd.mesh import marching_cubes
    x = np.linspace(-1.0, 1.0, 96)
    X, Y, Z = np.meshgrid(x, x, x, indexing='ij')
    spheres = [((-0.55, 0.0, 0.0), 0.25), ((0.2, 0.3, 0.0), 0.35), ((0.35, -0.55, 0.3), 0.2)]
    vol = np.min([np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - r for c, r in spheres], axis=0).astype(np.float32)
    h = x[1] - x[0]
    mesh = marching_cubes(torch.from_numpy(vol).cuda(), 0.0, (h,) * 3, (x[0],) * 3)
    labels, count = mesh.components()
    assert count == 3
    labels = _np(labels)
    v, f = _np(mesh.vertices), _np(mesh.faces).astype(np.int64)
    want, _ = mc_ref.components(f, len(v))
    assert np.array_equal(labels, want)
    big = mesh.largest_component()
    bv = _np(big.vertices)
    assert np.abs(np.linalg.norm(bv - np.array(spheres[1][0]), axis=1) - spheres[1][1]).max() < h
    assert abs(big.area() / (4 * np.pi * spheres[1][1] ** 2) - 1) < 0.02
    assert mc_ref.directed_edges_ok(_np(big.faces).astype(np.int64), len(bv))


def _shared_edge_labels(f, nv):
    """connected components of the shared-edge (face adjacency) graph, the way trimesh.split forms them"""
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    fid = np.tile(np.arange(len(f)), 3)
    key = e[:, 0] * nv + e[:, 1]
    order = np.argsort(key, kind='stable')
    ks, fs = key[order], fid[order]
    same = ks[1:] == ks[:-1]
    a, b = fs[:-1][same], fs[1:][same]
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        g = coo_matrix((np.ones(len(a)), (a, b)), shape=(len(f), len(f)))
        return connected_components(g, directed=False)[1]
    except ImportError:                                               # a numpy union-find on the face graph
        tri = np.stack([a, b, b], 1)
        return mc_ref.components(tri, len(f))[0] if len(a) else np.arange(len(f))


def _same_partition(x, y):
    pairs = np.unique(np.stack([x, y], 1), axis=0)
    return len(pairs) == len(np.unique(x)) == len(np.unique(y))


@pytest.mark.parametrize('seed', range(3))
def test_components_match_shared_edge_graph(seed):
    from mvsdf_amd.mesh import marching_cubes
    rs = np.random.RandomState(100 + seed)
    shape = [(24, 20, 16), (9, 30, 11), (40, 40, 40)][seed]
    vol = np.ones(shape, np.float32)
    vol[1:-1, 1:-1, 1:-1] = np.where(rs.rand(*[s - 2 for s in shape]) < 0.15, -1.0, 1.0) * rs.rand(*[s - 2 for s in shape])
    mesh = marching_cubes(torch.from_numpy(vol).cuda())
    v, f, n = _np(mesh.vertices), _np(mesh.faces).astype(np.int64), _np(mesh.normals)
    labels, count = mesh.components()
    labels = _np(labels)
    ref, rcount = mc_ref.components(f, len(v))
    assert count == rcount > 10 and np.array_equal(labels, ref)
    assert _same_partition(labels, _shared_edge_labels(f, len(v)))
    best = mc_ref.largest(v, f, labels, count)
    big = mesh.largest_component()
    wv, wf, wn, _ = mc_ref.select(v, f, n, labels, best)
    assert np.array_equal(_np(big.vertices), wv) and np.array_equal(_np(big.faces), wf) and np.array_equal(_np(big.normals), wn)


def _model(W):
    from mvsdf_amd.model.implicit_differentiable_renderer import IDRNetwork
    from mvsdf_amd.utils import synth
    from mvsdf_amd.utils.config import ConfigDict
    m = IDRNetwork(ConfigDict(synth.model_conf(W)))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(W, 0).items()})
    return m.cuda().eval()


def test_surface_mesh_equals_restatement_on_the_surface_volume():
    from mvsdf_amd import mesh as M
    from mvsdf_amd.utils import plots
    m = _model(64)
    res = 48
    mesh = M.surface_mesh(m, res)
    vol = plots.surface_volume(m, res)
    x = np.linspace(-1.0, 1.0, res)
    _check_equal(mesh, vol, 0.0, (x[2] - x[1],) * 3, (x[0],) * 3)
    want = plots.surface_vertex_colors(m, mesh.vertices)
    assert torch.equal(mesh.vertex_colors, want)


def test_extract_world_mesh_writes_the_largest_component(tmp_path):
    from mvsdf_amd import evaluation as ev
    from mvsdf_amd import mesh as M
    m = _model(64)
    scale = np.diag([1.7, 1.7, 1.7, 1.0])
    scale[:3, 3] = [0.1, -0.2, 0.3]
    out = ev.extract_world_mesh(m, scale, resolution=40, path=str(tmp_path), epoch=7)
    full = M.surface_mesh(m, 40)
    v, f, n = _np(full.vertices), _np(full.faces).astype(np.int64), _np(full.normals)
    labels, count = mc_ref.components(f, len(v))
    wv, wf, _, _ = mc_ref.select(v, f, n, labels, mc_ref.largest(v, f, labels, count))
    want = (wv.astype(np.float64) @ scale[:3, :3].T + scale[:3, 3]).astype(np.float32)
    path = tmp_path / 'surface_world_coordinates_7.obj'
    rows = [line.split() for line in open(path)]
    pv = np.array([[float(t) for t in r[1:4]] for r in rows if r[0] == 'v'], np.float32)
    pf = np.array([[int(t.split('//')[0]) - 1 for t in r[1:]] for r in rows if r[0] == 'f'])
    assert np.abs(pv - want).max() <= 1e-6 * max(1.0, np.abs(want).max())
    assert np.array_equal(pf, wf)
    assert np.array_equal(pv, _np(out.vertices))
