"""On-device mesh trimming (Mesh.cut_mask / Mesh.trim, csrc/mesh_cut.hip) against the reference fixtures tests/golden/mesh_cut/*.npz and the
restatement tests/maxflow_ref.py: the removed faces are exactly S*, the flow is the maximum, trim equals the host removal."""
import glob
import os

import numpy as np
import pytest
import torch

import maxflow_ref
import mc_ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, 'mesh_cut', '*.npz')))


def _mesh(v, f, n=None, c=None, device='cuda'):
    from mvsdf_amd.mesh import Mesh
    v = np.asarray(v, np.float32)
    n = np.zeros_like(v) if n is None else np.asarray(n, np.float32)
    m = Mesh(torch.from_numpy(v), torch.from_numpy(np.asarray(f, np.int32)), torch.from_numpy(n), None if c is None else torch.from_numpy(np.asarray(c, np.float32)))
    return m.to(device)


def _random_mesh(seed, n=12):
    rs = np.random.RandomState(seed)
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float32)] * 3, indexing='ij'))
    k = rs.randn(3, 3) * 0.5
    vol = np.sqrt(((g - (n - 1) / 2) ** 2).sum(0)) - rs.uniform(2.5, n / 2 + 1) + np.sin(np.tensordot(k, g, 1)).sum(0)
    v, f, nn = mc_ref.marching_cubes(vol.astype(np.float32))
    s = 1.0 / (1.0 + np.exp(-(rs.uniform(-1, 3) + 3 * np.sin(v @ rs.randn(3) * 0.6))))
    c = np.stack([1 - s, s, 0 * s], 1).astype(np.float32)
    c[rs.rand(len(c)) < 0.05, 0] = np.float32(rs.choice([0, 15, 128, 255]) / 255)   # reds at the thresholds
    return v, f.astype(np.int32), nn, c


@pytest.mark.parametrize('path', FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_fixture_mask_is_s_star(path):
    d = np.load(path)
    m = _mesh(d['vertices'], d['faces'], d['normals'], d['colors'])
    removed, flow = m.cut_mask(int(d['thresh']), int(d['smooth']))
    r = removed.cpu().numpy()
    assert removed.dtype == torch.bool and removed.is_cuda
    assert flow == int(d['flow'])
    assert np.array_equal(r, d['s_star'])
    assert not (d['ref_mask'] & ~r).any()
    print('%s: F %d flow %d removed %d rounds %d relabel launches %d' % (os.path.basename(path), len(r), flow, r.sum(), m.cut_stats['rounds'],
                                                                        m.cut_stats['relabel_launches']))


@pytest.mark.parametrize('seed', range(6))
def test_random_meshes_against_the_restatement(seed):
    v, f, n, c = _random_mesh(seed)
    m = _mesh(v, f, n, c)
    for smooth in (0, 1, 2, 10, 255):
        for thresh in (0, 15, 128, 255):
            flow_ref, s_ref = maxflow_ref.max_flow(f, c, thresh, smooth)
            removed, flow = m.cut_mask(thresh, smooth)
            assert flow == flow_ref, (smooth, thresh)
            assert np.array_equal(removed.cpu().numpy(), s_ref), (smooth, thresh)


def test_trim_equals_the_host_removal():
    d = np.load(os.path.join(GOLDEN, 'mesh_cut', 'smooth2.npz'))
    m = _mesh(d['vertices'], d['faces'], d['normals'], d['colors'])
    out = m.trim(int(d['thresh']), int(d['smooth']))
    ov, of, on, oc = maxflow_ref.remove(d['vertices'], d['faces'], d['normals'], d['colors'], d['s_star'])
    assert out.vertices.is_cuda
    for a, b in ((out.vertices, ov), (out.faces, of), (out.normals, on), (out.vertex_colors, oc)):
        assert np.array_equal(a.cpu().numpy(), b)
    assert m.cut_stats['kept_vertices'] == len(ov)


def test_two_runs_are_bit_identical():
    d = np.load(os.path.join(GOLDEN, 'mesh_cut', 'big_smooth1.npz'))
    m = _mesh(d['vertices'], d['faces'], d['normals'], d['colors'])
    a, fa = m.cut_mask(15, 1)
    b, fb = m.cut_mask(15, 1)
    assert fa == fb and torch.equal(a, b)
    ta, tb = m.trim(15, 1), m.trim(15, 1)
    for x, y in ((ta.vertices, tb.vertices), (ta.faces, tb.faces), (ta.normals, tb.normals), (ta.vertex_colors, tb.vertex_colors)):
        assert torch.equal(x, y)


def test_edge_cases():
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    red = lambda r: np.array([[r, 1 - r, 0]] * 3, np.float32)    # noqa: E731
    m = _mesh(tri, [[0, 1, 2]], c=red(1.0))                         # one bright face: removed
    removed, flow = m.cut_mask()
    assert removed.tolist() == [True] and flow == 0
    assert m.trim() is None
    m = _mesh(tri, [[0, 1, 2]], c=red(0.0))                         # one dark face: kept
    removed, flow = m.cut_mask()
    assert removed.tolist() == [False] and flow == 0
    out = m.trim()
    assert out.faces.tolist() == [[0, 1, 2]] and torch.equal(out.vertices.cpu(), torch.from_numpy(tri))
    v, f, n, c = _random_mesh(3)
    for val, want in ((1.0, True), (0.0, False)):                    # all bright / all dark
        c2 = c.copy()
        c2[:, 0] = val
        removed, flow = _mesh(v, f, n, c2).cut_mask(15, 10)
        assert flow == 0 and bool(removed.all()) == want and bool(removed.any()) == want


def test_boundary_and_two_components():
    # two quads far apart: faces 0, 1 share an edge, faces 2, 3 share an edge; every other edge is a boundary
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [5, 0, 0], [6, 0, 0], [6, 1, 0], [5, 1, 0]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.int32)
    c = np.zeros((8, 3), np.float32)
    c[[1, 2], 0] = 1.0                  # face 0: reds (0, 1, 1) -> 2/3 bright; face 1: (0, 1, 0) -> 1/3 bright
    c[[5], 0] = 0.03                    # face 2: 0.01 <= 15/255: dark; face 3: 0: dark
    for smooth in (0, 1, 10):
        flow_ref, s_ref = maxflow_ref.max_flow(f, c, 15, smooth)
        removed, flow = _mesh(v, f, c=c).cut_mask(15, smooth)
        assert flow == flow_ref and np.array_equal(removed.cpu().numpy(), s_ref)
    assert _mesh(v, f, c=c).cut_mask(15, 1)[0].tolist() == [True, True, False, False]


def test_refusals():
    from mvsdf_amd._lib import MvsdfError
    v = np.zeros((5, 3), np.float32)
    c = np.full((5, 3), 0.5, np.float32)
    with pytest.raises(ValueError, match='directed edge'):
        _mesh(v, [[0, 1, 2], [0, 1, 3]], c=c).cut_mask()            # non-manifold: (0, 1) twice
    with pytest.raises(ValueError, match='directed edge'):
        _mesh(v, [[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 2, 3]], c=c).cut_mask()   # a tetrahedron with one flipped face
    with pytest.raises(ValueError, match='repeats a vertex'):
        _mesh(v, [[0, 1, 1]], c=c).cut_mask()
    with pytest.raises(ValueError, match='out of range'):
        _mesh(v, [[0, 1, 7]], c=c).cut_mask()
    with pytest.raises(ValueError, match='colours'):
        _mesh(v, [[0, 1, 2]]).cut_mask()
    with pytest.raises(MvsdfError, match='GPU'):
        _mesh(v, [[0, 1, 2]], c=c, device='cpu').trim()
    with pytest.raises(ValueError, match='smooth'):
        _mesh(v, [[0, 1, 2]], c=c).cut_mask(15, -1)
    with pytest.raises(ValueError, match='smooth'):
        _mesh(v, [[0, 1, 2]], c=c).cut_mask(15, 2 ** 31 // 6 + 1)
    with pytest.raises(ValueError, match='int'):
        _mesh(v, [[0, 1, 2]], c=c).cut_mask(15.0, 10)
    # a closed tetrahedron with consistent winding is accepted: every face has three neighbours
    removed, flow = _mesh(v, [[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2]], c=c).cut_mask()
    assert removed.all() and flow == 0


def test_model_path_512():
    """surface_mesh(model, 512).largest_component().trim(): the reported flow is the capacity of the returned cut (int64, on the host); against
    scipy where it imports."""
    from mvsdf_amd.mesh import surface_mesh
    from mvsdf_amd.model.implicit_differentiable_renderer import IDRNetwork
    from mvsdf_amd.utils import synth
    from mvsdf_amd.utils.config import ConfigDict
    W = 256
    model = IDRNetwork(ConfigDict(synth.model_conf(W)))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(W, 0).items()})
    model = model.cuda().eval()
    mesh = surface_mesh(model, 512).largest_component()
    out = mesh.trim(15, 10)
    removed, flow = mesh.cut_mask(15, 10)
    f, c = mesh.faces.cpu().numpy(), mesh.vertex_colors.cpu().numpy()
    r = removed.cpu().numpy()
    assert maxflow_ref.cut_capacity(r, f, c, 15, 10) == flow
    nf_out = 0 if out is None else len(out)
    assert nf_out == len(f) - int(r.sum())
    print('512^3 trim: F %d -> %d, flow %d, rounds %d, relabel launches %d' % (len(f), nf_out, flow, mesh.cut_stats['rounds'],
                                                                               mesh.cut_stats['relabel_launches']))
    # the same mesh with colours from a smooth field, so that the cut is not trivial
    s = torch.sigmoid(1.5 + 3.0 * torch.sin(mesh.vertices.double() @ torch.tensor([7.0, -5.0, 4.0], dtype=torch.float64, device='cuda'))).float()
    mesh.vertex_colors = torch.stack([1 - s, s, torch.zeros_like(s)], 1).contiguous()
    removed2, flow2 = mesh.cut_mask(15, 2)
    c2, r2 = mesh.vertex_colors.cpu().numpy(), removed2.cpu().numpy()
    assert flow2 > 0 and 0 < r2.sum() < len(f)
    assert maxflow_ref.cut_capacity(r2, f, c2, 15, 2) == flow2
    print('512^3 field colours, smooth 2: flow %d, removed %d, rounds %d, relabel launches %d' % (flow2, r2.sum(), mesh.cut_stats['rounds'],
                                                                                                  mesh.cut_stats['relabel_launches']))
    try:
        import scipy  # noqa: F401
    except ImportError:
        return
    fl, s_star = maxflow_ref.scipy_max_flow(f, c, 15, 10)
    assert fl == flow and np.array_equal(r, s_star)
    fl, s_star = maxflow_ref.scipy_max_flow(f, c2, 15, 2)
    assert fl == flow2 and np.array_equal(r2, s_star)
