"""Mesh extraction without a GPU: the generated triangle table, closure / orientation of the table's surfaces (through the numpy restatement
tests/mc_ref.py), the workspace queries of the library, and Mesh.export / apply_transform on host tensors."""
import importlib.util
import os
import struct

import numpy as np
import pytest

from conftest import ROOT
import mc_ref


def _gen():
    spec = importlib.util.spec_from_file_location('gen_mc_tables', os.path.join(ROOT, 'tools', 'gen_mc_tables.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_generator_reproduces_the_committed_header():
    assert _gen().render() == open(mc_ref.HEADER).read()


def _padded(core, pad=1.0):
    v = np.full(tuple(s + 2 for s in core.shape), pad, np.float32)
    v[1:-1, 1:-1, 1:-1] = core
    return v


def _closed(v, level=0.0):
    verts, faces, normals = mc_ref.marching_cubes(v, level)
    inside = v < np.float32(level)
    n_cross = sum(int((np.diff(inside.astype(np.int8), axis=a) != 0).sum()) for a in range(3))
    assert len(verts) == n_cross                                     # every crossing grid edge has a vertex
    assert mc_ref.directed_edges_ok(faces, len(verts))                # ... closed, oriented, every vertex referenced
    return verts, faces


def test_all_256_cube_configurations_are_closed_and_outward():
    for ci in range(256):
        core = np.array([1.0 if not ci >> c & 1 else -1.0 for c in range(8)], np.float32)
        core = core.reshape(2, 2, 2, order='F')                     # corner c = (c & 1, c >> 1 & 1, c >> 2 & 1)
        v = _padded(core)
        assert (v[1 + (5 & 1), 1 + (5 >> 1 & 1), 1 + (5 >> 2 & 1)] < 0) == bool(ci >> 5 & 1)
        verts, faces = _closed(v)
        assert (len(faces) == 0) == (ci == 0)
        if len(faces):
            assert mc_ref.signed_volume(verts, faces) > 0, ci        # right-hand normals point outwards (towards increasing values)


@pytest.mark.parametrize('seed', range(4))
def test_random_volumes_are_closed_manifolds(seed):
    rs = np.random.RandomState(seed)
    for it in range(50):
        shape = rs.randint(3, 11, size=3)
        if it % 3 == 0:
            core = rs.randint(-1, 2, size=shape).astype(np.float32)   # many values exactly at the level
        elif it % 3 == 1:
            core = rs.randn(*shape).astype(np.float32)
        else:
            core = np.where(rs.rand(*shape) < 0.3, np.float32(0.5), rs.randn(*shape).astype(np.float32))
        level = 0.5 if it % 3 == 2 else 0.0
        _closed(_padded(core, pad=2.0), level)


def test_workspace_query_bounds_and_refusals():
    from mvsdf_amd import _lib
    L = _lib.lib()
    for shape in [(2, 2, 2), (17, 31, 9), (64, 64, 64), (512, 512, 512)]:
        pts = int(np.prod(shape))
        blocks = -(-pts // 1024)
        size = L.mvsdf_mc_workspace_bytes(*shape)
        assert 4 * pts <= size <= 4 * pts + 24 * blocks + 6 * 256, shape
    for bad in [(1, 5, 5), (5, 0, 5), (5, 5, -3), (1 << 21, 1 << 21, 1 << 21), (1 << 40, 1 << 40, 2)]:
        assert L.mvsdf_mc_workspace_bytes(*bad) == 0, bad
    assert L.mvsdf_mesh_cc_workspace_bytes(100, 196) > 0
    for bad in [(0, 5), (5, 0), (1 << 31, 5), (5, 1 << 31)]:
        assert L.mvsdf_mesh_cc_workspace_bytes(*bad) == 0, bad


def _sphere_mesh():
    from mvsdf_amd.mesh import Mesh
    x = np.linspace(-1, 1, 16).astype(np.float32)
    X, Y, Z = np.meshgrid(x, x, x, indexing='ij')
    verts, faces, normals = mc_ref.marching_cubes(np.sqrt(X * X + Y * Y + Z * Z) - 0.6, 0.0, (x[1] - x[0],) * 3, (x[0],) * 3)
    cols = np.random.RandomState(0).rand(len(verts), 3).astype(np.float32)
    return Mesh(verts, faces.astype(np.int32), normals, cols), verts, faces, normals, cols


def _parse_obj(path):
    v, vn, f = [], [], []
    for line in open(path):
        tok = line.split()
        if tok[0] == 'v':
            v.append([np.float32(float(x)) for x in tok[1:]])
        elif tok[0] == 'vn':
            vn.append([np.float32(float(x)) for x in tok[1:]])
        elif tok[0] == 'f':
            a = [t.split('//') for t in tok[1:]]
            assert all(p[0] == p[1] for p in a)
            f.append([int(p[0]) - 1 for p in a])
    return np.array(v, np.float32), np.array(vn, np.float32), np.array(f, np.int64)


def test_obj_export_round_trips_exactly(tmp_path):
    m, verts, faces, normals, cols = _sphere_mesh()
    p = str(tmp_path / 'm.obj')
    m.export(p)
    v, vn, f = _parse_obj(p)
    assert np.array_equal(v[:, :3], verts) and np.array_equal(v[:, 3:], cols)
    assert np.array_equal(vn, normals) and np.array_equal(f, faces)


def test_ply_export_round_trips_exactly(tmp_path):
    m, verts, faces, normals, cols = _sphere_mesh()
    p = str(tmp_path / 'm.ply')
    m.export(p)
    data = open(p, 'rb').read()
    head, body = data.split(b'end_header\n', 1)
    lines = head.decode('ascii').split('\n')
    assert lines[0] == 'ply' and lines[1] == 'format binary_little_endian 1.0'
    nv = int([x for x in lines if x.startswith('element vertex')][0].split()[-1])
    nf = int([x for x in lines if x.startswith('element face')][0].split()[-1])
    assert (nv, nf) == (len(verts), len(faces))
    rec = struct.Struct('<6f3B')
    vb = np.array([rec.unpack_from(body, i * rec.size) for i in range(nv)])
    assert np.array_equal(vb[:, :3].astype(np.float32), verts) and np.array_equal(vb[:, 3:6].astype(np.float32), normals)
    assert np.array_equal(vb[:, 6:], np.rint(cols * 255))
    fb = body[nv * rec.size:]
    assert len(fb) == nf * 13
    fr = np.array([struct.unpack_from('<B3i', fb, i * 13) for i in range(nf)])
    assert (fr[:, 0] == 3).all() and np.array_equal(fr[:, 1:], faces)


def test_apply_transform_with_a_reflection_keeps_the_volume_positive():
    m, verts, faces, normals, _ = _sphere_mesh()
    vol0 = mc_ref.signed_volume(verts, faces)
    M = np.diag([-2.0, 1.5, 1.0, 1.0])
    M[:3, 3] = [0.3, -0.1, 2.0]
    m.apply_transform(M)
    v = m.vertices.numpy()
    f = m.faces.numpy().astype(np.int64)
    assert np.array_equal(v, (verts.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32))
    assert np.array_equal(f, faces[:, [0, 2, 1]])
    assert mc_ref.signed_volume(v, f) == pytest.approx(3.0 * vol0, rel=1e-5)
    n = m.normals.numpy()
    assert np.allclose(np.linalg.norm(n, axis=1), 1, atol=1e-6)
    radial = v - M[:3, 3]
    radial = radial / np.array([-2.0, 1.5, 1.0]) ** 2             # gradient direction of the stretched sphere's implicit function
    cos = (n * radial).sum(1) / np.linalg.norm(radial, axis=1)
    assert cos.min() > 0.9


def test_marching_cubes_rejects_bad_shapes():
    from mvsdf_amd.mesh import marching_cubes
    with pytest.raises(ValueError):
        marching_cubes(np.zeros((4, 4), np.float32))
