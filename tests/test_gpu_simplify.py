"""On-device mesh simplification (Mesh.simplify, csrc/mesh_simplify.hip) against its numpy restatement tests/simplify_ref.py, bit for bit: vertices,
normals and colours as uint32 views, faces and statistics exactly, and every case twice in a row with identical bits."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
import mc_ref
import simplify_ref as S

pytestmark = pytest.mark.gpu

BOX = (0.53, 0.47, 0.61)
PLATE = (0.6, 0.55, 0.05)
STAT_KEYS = ('cell', 'clusters', 'vertices', 'faces', 'degenerate', 'duplicates', 'quadric_placed')


def _mesh(v, f, n, c):
    from mvsdf_amd.mesh import Mesh
    return Mesh(torch.from_numpy(np.array(v, np.float32)), torch.from_numpy(np.array(f).astype(np.int32)), torch.from_numpy(np.array(n, np.float32)),
                None if c is None else torch.from_numpy(np.array(c, np.float32))).to('cuda')


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _same_mesh(a, b):
    if a is None or b is None:
        return a is None and b is None
    return (torch.equal(a.faces, b.faces) and np.array_equal(_bits(a.vertices), _bits(b.vertices)) and np.array_equal(_bits(a.normals), _bits(b.normals))
            and (a.vertex_colors is None) == (b.vertex_colors is None)
            and (a.vertex_colors is None or np.array_equal(_bits(a.vertex_colors), _bits(b.vertex_colors))))


def _check(v, f, n, c, cell, origin=None, placement='quadric'):
    """the device result of two runs == the restatement's, bits and statistics -> (Mesh or None, stats)"""
    mesh = _mesh(v, f, n, c)
    out = mesh.simplify(cell, origin=origin, placement=placement)
    stats = dict(mesh.simplify_stats)
    again = mesh.simplify(cell, origin=origin, placement=placement)
    assert _same_mesh(out, again) and stats == mesh.simplify_stats
    rv, rf, rn, rc, rstats = S.simplify(v, f, n, c, cell, origin=origin, placement=placement)
    assert {k: stats[k] for k in STAT_KEYS} == {k: rstats[k] for k in STAT_KEYS}
    if rv is None:
        assert out is None
        return None, stats
    assert out is not None and out.vertices.is_cuda
    assert out.faces.dtype == torch.int32 and np.array_equal(out.faces.cpu().numpy(), rf)
    assert np.array_equal(_bits(out.vertices), rv.view(np.uint32))
    assert np.array_equal(_bits(out.normals), rn.view(np.uint32))
    if c is None:
        assert out.vertex_colors is None
    else:
        assert np.array_equal(_bits(out.vertex_colors), rc.view(np.uint32))
    return out, stats


SHAPE_CASES = ([('sphere', 16, None, m) for m in (1, 2, 3, 4.5)] + [('sphere', 24, None, m) for m in (1, 2, 3)]
               + [('sphere', 40, None, m) for m in (1, 2, 3, 4.5)] + [('box', 24, BOX, 3), ('box', 40, BOX, 3), ('box', 24, PLATE, 2)])


@pytest.mark.parametrize('kind,n,half,mult', SHAPE_CASES)
def test_host_test_shapes_match_the_restatement(kind, n, half, mult):
    v, f, nrm, col, h = S.shape_mesh(kind, n, half)
    if kind == 'sphere':
        assert (len(v), len(f)) == {16: (360, 716), 24: (888, 1772), 40: (2592, 5180)}[n]
    cell = mult * h
    for placement in ('quadric', 'mean'):
        for c in (col, None):
            out, st = _check(v, f, nrm, c, cell, placement=placement)
            of = out.faces.cpu().numpy()
            if half == PLATE:                                           # a double-sided sheet: every face has its opposite
                assert ({tuple(r) for r in S.rotate_min_first(of).tolist()} == {tuple(r) for r in S.rotate_min_first(of[:, [0, 2, 1]]).tolist()}
                        and st['duplicates'] == 0 and st['faces'] == 120)
            else:
                assert mc_ref.directed_edges_ok(of, out.vertices.shape[0])
    if (kind, n, mult) == ('sphere', 40, 1):
        assert st['clusters'] == 1708 and st['faces'] > 2048            # both cross the scan's 2048-item chunk
    origin = v.astype(np.float64).min(0) - np.array([0.3, 0.7, 0.1]) * cell     # not the box's corner
    _check(v, f, nrm, col, cell, origin=origin)


# ---- edge sizes ----
def test_one_face():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    n = np.array([[0, 0, 1]] * 3, np.float32)
    out, st = _check(v, np.array([[0, 1, 2]]), n, None, 0.25)
    assert st['faces'] == 1 and st['vertices'] == 3
    assert np.array_equal(out.vertices.cpu().numpy(), v)


def test_every_vertex_in_one_cell_gives_none():
    v, f, nrm, col, h = S.shape_mesh('sphere', 16)
    out, st = _check(v, f, nrm, col, 4.0)
    assert out is None and st['clusters'] == 1 and st['degenerate'] == len(f) and st['faces'] == 0


def test_cell_so_large_that_eight_clusters_remain():
    v, f, nrm, col, h = S.shape_mesh('sphere', 16)
    extent = float((v.max(0) - v.min(0)).max())
    out, st = _check(v, f, nrm, col, 0.6 * extent)
    assert st['clusters'] == 8 and st['vertices'] == 8


def test_cell_so_small_that_nothing_merges():
    v, f, nrm, col, h = S.shape_mesh('sphere', 16)
    v = np.concatenate([v[:100], [[0.9, 0.9, 0.9]], v[100:]]).astype(np.float32)          # vertex 100 is unreferenced
    nrm = np.concatenate([nrm[:100], [[0, 0, 1]], nrm[100:]]).astype(np.float32)
    col = np.concatenate([col[:100], [[0.5, 0.5, 0.5]], col[100:]]).astype(np.float32)
    f = np.where(f >= 100, f + 1, f)
    ref = np.delete(np.arange(len(v)), 100)
    for placement in ('mean', 'quadric'):
        out, st = _check(v, f, nrm, col, 1e-3 * h, placement=placement)
        assert st['clusters'] == len(v) and st['vertices'] == len(v) - 1 and st['degenerate'] == 0 and st['duplicates'] == 0
        assert np.array_equal(out.faces.cpu().numpy(), np.where(f > 100, f - 1, f))
        got = out.vertices.cpu().numpy()
        if placement == 'mean':
            assert np.array_equal(got, v[ref])                          # the mean of one vertex is the vertex
        else:
            # a single vertex lies on all its faces' planes: b is rounding noise and x = O(1e-13); at most the last bit of an fp32 below 1 moves
            assert np.abs(got - v[ref]).max() <= 2.0 ** -24
        assert np.array_equal(out.vertex_colors.cpu().numpy(), col[ref])


def _soup(rs, nv, nf, scale, lo=0.0, hi=1.0):
    v = (rs.uniform(lo, hi, (nv, 3)) * scale).astype(np.float32)
    f = rs.randint(0, nv, (nf, 3))
    n = rs.randn(nv, 3).astype(np.float32)
    c = rs.rand(nv, 3).astype(np.float32)
    return v, f, n, c


def test_one_cell_holding_3000_of_3100_vertices():
    rs = np.random.RandomState(7)
    v, f, n, c = _soup(rs, 3100, 2500, 1.0, 0.05, 0.95)
    v[3000:] = rs.uniform(1.0, 9.0, (100, 3)).astype(np.float32)
    perm = rs.permutation(3100)                                          # the big cell's members are spread over the vertex ids
    v = v[perm]
    out, st = _check(v, f, n, c, 1.0, origin=(0.0, 0.0, 0.0))
    assert st['clusters'] <= 101


@pytest.mark.parametrize('nv,nf,scale', [(2047, 1365, 1e3), (2048, 1366, 1e-3), (2049, 1365, 1e-3), (2049, 1366, 1e3), (4097, 1366, 1e3), (4097, 1365, 1e-3)])
def test_random_soups_at_the_chunk_sizes(nv, nf, scale):
    """3 F = 4095 / 4098 around the sort's 4096-item chunk, V around the scan's 2048-item chunk and past the sort's; the far origin gives cell
    indices near 1000, so the vertex keys have bits beyond the first radix passes"""
    rs = np.random.RandomState(nv + nf)
    v, f, n, c = _soup(rs, nv, nf, scale)
    cell = scale / 12.0
    for origin in (None, (-1000.0 * cell,) * 3):
        for placement in ('quadric', 'mean'):
            out, st = _check(v, f, n, c, cell, origin=origin, placement=placement)
            assert 1 < st['clusters'] <= 12 ** 3 + 3 * 12 ** 2 + 3 * 12 + 1 and st['faces'] > 0
    out, st = _check(v, f, n, c, scale / 2.0)                          # 8 to 27 clusters: most faces repeat an earlier one
    assert st['clusters'] <= 27 and st['duplicates'] > st['faces'] > 0 and st['degenerate'] > 0


# ---- the hand-built cases of the host test ----
@pytest.mark.parametrize('name', sorted(S.HAND))
def test_hand_built(name):
    (v, f, n, c), cell, org = S.HAND[name]()
    for placement in ('quadric', 'mean'):
        out, st = _check(v, f, n, c, cell, origin=org, placement=placement)
    if name == 'duplicate':
        assert st['duplicates'] == 1 and out.faces.cpu().tolist() == [[0, 2, 1], [0, 1, 2]]
    if name == 'tetrahedron':
        assert st['clusters'] == 4 and st['vertices'] == 3
    if name == 'unreferenced':
        assert st['clusters'] == 4 and st['vertices'] == 3
    if name in ('zero_area', 'candidate_leaves'):
        q, _ = _check(v, f, n, c, cell, origin=org, placement='quadric')
        assert np.array_equal(_bits(q.vertices[0]), _bits(out.vertices[0]))     # the mean


# ---- target_faces ----
@pytest.mark.parametrize('target', [200, 1000, 5180, 10 ** 6])
def test_target_faces(target):
    v, f, nrm, col, h = S.shape_mesh('sphere', 40)
    mesh = _mesh(v, f, nrm, col)
    out = mesh.simplify(target_faces=target)
    st = dict(mesh.simplify_stats)
    assert len(out) <= target and st['passes'] <= 24
    if target >= len(f):
        src = _mesh(v, f, nrm, col)
        assert _same_mesh(out, src) and st['passes'] == 0 and st['cell_rejected'] is None
        assert out.vertices.data_ptr() != mesh.vertices.data_ptr()     # a copy
        return
    assert st['faces'] == len(out)
    assert _same_mesh(out, mesh.simplify(cell=st['cell']))
    assert _same_mesh(out, mesh.simplify(target_faces=target)) and mesh.simplify_stats == st
    _check(v, f, nrm, col, st['cell'])
    assert st['cell_rejected'] is not None and st['cell_rejected'] < st['cell']
    more = mesh.simplify(cell=st['cell_rejected'])
    assert len(more) > target


# ---- refusals ----
def test_refusals():
    from mvsdf_amd._lib import lib, MvsdfError
    from mvsdf_amd.mesh import Mesh
    v, f, nrm, col, h = S.shape_mesh('sphere', 16)
    mesh = _mesh(v, f, nrm, col)
    with pytest.raises(MvsdfError):
        mesh.to('cpu').simplify(2 * h)
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            mesh.simplify(bad)
    with pytest.raises(ValueError):
        mesh.simplify()
    with pytest.raises(ValueError):
        mesh.simplify(2 * h, target_faces=100)
    with pytest.raises(ValueError):
        mesh.simplify(2 * h, placement='median')
    with pytest.raises(ValueError):
        mesh.simplify(2 * h, origin=(0.0, float('nan'), 0.0))
    with pytest.raises(ValueError):
        mesh.simplify(1e-7)                                             # cell indices >= 2^21
    with pytest.raises(ValueError):
        mesh.simplify(2 * h, origin=(0.0, 0.0, 0.0))                    # vertices below the origin: negative indices
    for bad in (np.nan, np.inf):
        w = v.copy()
        w[17, 1] = bad
        with pytest.raises(ValueError):
            _mesh(w, f, nrm, col).simplify(2 * h)
        with pytest.raises(ValueError):
            _mesh(w, f, nrm, col).simplify(target_faces=100)
    for bad in (-1, len(v)):
        g = f.copy()
        g[5, 2] = bad
        with pytest.raises(ValueError):
            _mesh(v, g, nrm, col).simplify(2 * h)
    empty_f = Mesh(torch.from_numpy(v.copy()), torch.zeros(0, 3, dtype=torch.int32), torch.from_numpy(nrm.copy())).to('cuda')
    empty_v = Mesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(0, 3)).to('cuda')
    for m in (empty_f, empty_v):
        with pytest.raises(ValueError):
            m.simplify(2 * h)
    size = lib().mvsdf_mesh_simplify_workspace_bytes
    i31 = 2 ** 31 - 1
    assert size(i31, i31 // 3) > 0 and size(i31 + 1, 1) == 0 and size(1, i31 // 3 + 1) == 0 and size(0, 1) == 0 and size(1, 0) == 0
    with pytest.raises(ValueError):
        mesh.simplify(target_faces=0)
    assert _same_mesh(_mesh(v, f, nrm, None).simplify(2 * h), _mesh(v, f, nrm, None).simplify(2 * h))   # no colours: works


# ---- consumers ----
def test_simplified_sphere_feeds_components_and_the_file_formats(tmp_path):
    from mvsdf_amd.mesh import load_mesh
    v, f, nrm, col, h = S.shape_mesh('sphere', 24)
    out = _mesh(v, f, nrm, col).simplify(2 * h)
    labels, count = out.components()
    assert count == 1 and int(labels.max()) == 0
    out.export(str(tmp_path / 's.obj'))
    assert _same_mesh(load_mesh(str(tmp_path / 's.obj')).to('cuda'), out)               # %.9g round-trips fp32
    out.export(str(tmp_path / 's.ply'))
    back = load_mesh(str(tmp_path / 's.ply')).to('cuda')
    assert torch.equal(back.faces, out.faces) and torch.equal(back.vertices, out.vertices) and torch.equal(back.normals, out.normals)
    c = out.vertex_colors.cpu().numpy()                                                  # PLY colours are 8-bit: the writer's and the reader's rounding
    want = np.clip(np.rint(c * 255.0), 0, 255).astype(np.uint8).astype(np.float32) / np.float32(255.0)
    assert np.array_equal(back.vertex_colors.cpu().numpy(), want)


# ---- commands ----
def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('ext', ['.obj', '.ply'])
def test_simplify_mesh_command(tmp_path, ext, capsys):
    from mvsdf_amd.mesh import load_mesh
    v, f, nrm, col, h = S.shape_mesh('sphere', 24)
    src, dst = str(tmp_path / ('in' + ext)), str(tmp_path / ('out' + ext))
    _mesh(v, f, nrm, col).export(src)
    tool = _tool('simplify_mesh')
    cell = float(2 * h)
    for args, kw in ((['--cell', repr(cell), '--placement', 'mean'], {'cell': cell, 'placement': 'mean'}), (['--faces', '300'], {'target_faces': 300})):
        tool.main([src, dst] + args)
        assert '[simplify] num faces from %d to ' % len(f) in capsys.readouterr().out
        want = load_mesh(src).to('cuda').simplify(**kw)
        want.export(str(tmp_path / ('want' + ext)))                      # through the format's own rounding
        assert _same_mesh(load_mesh(dst), load_mesh(str(tmp_path / ('want' + ext))))
        got = load_mesh(dst)
        assert torch.equal(got.faces, want.faces.cpu()) and torch.equal(got.vertices, want.vertices.cpu())
    with pytest.raises(SystemExit):
        tool.main([src, dst])                                            # neither --cell nor --faces
    with pytest.raises(SystemExit):
        tool.main([src, dst, '--cell', '100'])                           # one cell: nothing survives


def test_eval_writes_the_simplified_mesh_beside_the_usual_one(tmp_path):
    from mvsdf_amd import evaluation as ev
    from mvsdf_amd.mesh import load_mesh
    v, f, nrm, col, h = S.shape_mesh('sphere', 24)
    mesh = _mesh(v, f, nrm, col)
    out = ev.write_simplified_mesh(mesh, str(tmp_path), 7, target_faces=400)
    path = tmp_path / 'surface_world_coordinates_7_simplified.obj'
    assert sorted(os.listdir(tmp_path)) == [path.name] and len(out) <= 400
    assert _same_mesh(load_mesh(str(path)).to('cuda'), out) and _same_mesh(out, mesh.simplify(target_faces=400))
    assert _same_mesh(ev.write_simplified_mesh(mesh, str(tmp_path), 8, cell=2 * h), mesh.simplify(2 * h))
    assert ev.write_simplified_mesh(mesh, str(tmp_path), 9, cell=100.0) is None and len(os.listdir(tmp_path)) == 2
    opt = ev.eval_parser().parse_args(['--simplify_faces', '1000'])
    assert opt.simplify_faces == 1000 and opt.simplify_cell is None
    assert ev.eval_parser().parse_args([]).simplify_cell is None
