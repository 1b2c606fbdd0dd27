"""Mesh trimming without a GPU: tests/maxflow_ref.py against scipy, the invariants of the reference fixtures tests/golden/mesh_cut/*.npz,
load_mesh / export round trips and the CLI paths of tools/mesh_cut.py that need no GPU."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import maxflow_ref
import mc_ref
from conftest import GOLDEN, ROOT

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, 'mesh_cut', '*.npz')))


def _fixture(path):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def _sphere(n=14, r=5.0):
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float32)] * 3, indexing='ij'))
    v, f, nn = mc_ref.marching_cubes((np.sqrt(((g - (n - 1) / 2) ** 2).sum(0)) - r).astype(np.float32))
    s = 1.0 / (1.0 + np.exp(-3.0 * np.sin(v[:, 0] * 0.7) - 2.0 * np.cos(v[:, 1] * 0.5)))
    c = np.stack([1 - s, s, 0 * s], 1).astype(np.float32)
    return v, f.astype(np.int32), nn, c


def test_fixtures_cover_the_cases():
    names = {os.path.basename(p)[:-4] for p in FIXTURES}
    assert {'default', 'smooth1', 'smooth2', 'open', 'components', 'nothing', 'everything'} <= names
    sizes = sum(os.path.getsize(p) for p in FIXTURES)
    assert sizes < 4e6
    fx = {os.path.basename(p)[:-4]: _fixture(p) for p in FIXTURES}
    assert not fx['nothing']['s_star'].any() and fx['everything']['s_star'].all()
    assert any((d['s_star'] != d['ref_mask']).any() for d in fx.values()), 'no fixture where the reference leaves free faces'


@pytest.mark.parametrize('path', FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_fixture_invariants(path):
    d = _fixture(path)
    f, c, thresh, smooth = d['faces'], d['colors'], int(d['thresh']), int(d['smooth'])
    ref, s_star, flow = d['ref_mask'], d['s_star'], int(d['flow'])
    assert not (ref & ~s_star).any(), 'the reference removed a face outside S*'
    cut_ref = maxflow_ref.cut_capacity(ref, f, c, thresh, smooth)
    assert maxflow_ref.cut_capacity(s_star, f, c, thresh, smooth) == flow
    assert cut_ref >= flow
    assert (cut_ref == flow) == bool(np.array_equal(ref, s_star))
    if len(f) <= 5000:
        fl, ss = maxflow_ref.max_flow(f, c, thresh, smooth)
        assert fl == flow and np.array_equal(ss, s_star)


@pytest.mark.parametrize('smooth', [0, 1, 3, 10])
def test_maxflow_ref_against_scipy(smooth):
    pytest.importorskip('scipy')
    v, f, n, c = _sphere()
    for thresh in (15, 100):
        a = maxflow_ref.max_flow(f, c, thresh, smooth)
        b = maxflow_ref.scipy_max_flow(f, c, thresh, smooth)
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
        assert maxflow_ref.cut_capacity(a[1], f, c, thresh, smooth) == a[0]


def test_smooth_zero_removes_the_bright_faces():
    v, f, n, c = _sphere()
    bright, _ = maxflow_ref.graph(f, c, 15, 0)
    flow, s_star = maxflow_ref.max_flow(f, c, 15, 0)
    assert flow == 0 and np.array_equal(s_star, bright)


def test_graph_rejects_what_open3d_rejects():
    with pytest.raises(ValueError):
        maxflow_ref.half_edge_pairs([[0, 1, 2], [0, 1, 3]])                # the directed edge (0, 1) twice
    with pytest.raises(ValueError):
        maxflow_ref.half_edge_pairs([[0, 1, 1]])
    p = maxflow_ref.half_edge_pairs([[0, 1, 2], [1, 0, 3]])
    assert p.tolist() == [[0, 1], [1, 0]]


def test_remove_restatement():
    v = np.arange(15, dtype=np.float32).reshape(5, 3)
    f = np.array([[0, 1, 2], [2, 1, 3], [3, 1, 4]], np.int32)
    ov, of, on, oc = maxflow_ref.remove(v, f, v + 1, v + 2, np.array([False, True, False]))
    assert np.array_equal(ov, v[[0, 1, 2, 3, 4]]) and of.tolist() == [[0, 1, 2], [3, 1, 4]]
    ov, of, on, oc = maxflow_ref.remove(v, f, v + 1, None, np.array([True, False, True]))
    assert np.array_equal(ov, v[[1, 2, 3]]) and of.tolist() == [[1, 0, 2]] and np.array_equal(on, v[[1, 2, 3]] + 1) and oc is None


@pytest.mark.parametrize('ext', ['.obj', '.ply'])
def test_load_mesh_round_trip(tmp_path, ext):
    from mvsdf_amd.mesh import Mesh, load_mesh
    v, f, n, c = _sphere()
    if ext == '.ply':
        c = np.rint(c * 255).astype(np.float32) / np.float32(255)          # PLY colours are 8-bit
    m = Mesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(n), torch.from_numpy(c))
    p = str(tmp_path / ('m' + ext))
    m.export(p)
    r = load_mesh(p)
    for a, b in ((r.vertices, v), (r.faces, f), (r.normals, n), (r.vertex_colors, c)):
        assert a.numpy().dtype == b.dtype and np.array_equal(a.numpy(), b)
    m.vertex_colors = None
    m.export(p)
    r = load_mesh(p)
    assert r.vertex_colors is None and np.array_equal(r.faces.numpy(), f) and np.array_equal(r.vertices.numpy(), v)


def test_load_obj_tokens_and_errors(tmp_path):
    from mvsdf_amd.mesh import load_mesh
    p = tmp_path / 'a.obj'
    p.write_text('# c\nv 0 0 0 1 0 0\nv 1 0 0 0.5 0.5 0\nv 0 1 0 0 1 0\nv 1 1 0 0 0 0\nvt 0 0\nf 1 2 3\nf 2/1/1 4/1/1 3/1/1\nf -3//-3 -2//-2 -1//-1\n')
    m = load_mesh(str(p))
    assert m.faces.tolist() == [[0, 1, 2], [1, 3, 2], [1, 2, 3]] and m.vertex_colors[1].tolist() == [0.5, 0.5, 0.0]
    p.write_text('v 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nf 1 2 4 3\n')
    with pytest.raises(ValueError, match='triangles only'):
        load_mesh(str(p))
    p.write_text('v 0 0 0\nv 1 0 0\nf 1 2 3\n')
    with pytest.raises(ValueError, match='missing vertex'):
        load_mesh(str(p))
    with pytest.raises(ValueError, match='extension'):
        load_mesh(str(tmp_path / 'a.stl'))


def _cli(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'mesh_cut.py')] + list(args), capture_output=True, text=True, cwd=ROOT)


def test_cli_help_and_argument_errors(tmp_path):
    r = _cli('--help')
    assert r.returncode == 0 and '--thresh' in r.stdout and '--smooth' in r.stdout
    assert _cli().returncode == 2
    assert _cli('a.obj', 'b.obj', '--thresh', 'x').returncode == 2
    r = _cli('a.obj', 'b.obj', '--smooth', '-1')
    assert r.returncode == 2 and 'smooth' in r.stderr
    r = _cli(str(tmp_path / 'missing.obj'), str(tmp_path / 'out.obj'))
    assert r.returncode != 0 and 'missing.obj' in r.stderr
