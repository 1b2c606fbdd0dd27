"""Seam levelling on the device (mvsdf_amd/seams.py, csrc/seams.hip, the LEVEL fill of csrc/texture.hip) against the numpy restatement
tests/seams_ref.py: every stage and the composed calls equal entry for entry (torch.equal: the sign of a zero is not defined), on the smallest
shapes at which a kernel can still go wrong; then workspaces of poison, the refusals, and the tool."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import seams_ref as SR
import seams_scene as SS
import texture_ref as T
import texture_scene as TS
from conftest import ROOT
from helpers import POISON_PATTERNS
from mvsdf_amd import mesh as M
from mvsdf_amd import seams, texture
from mvsdf_amd.mesh import Mesh

pytestmark = pytest.mark.gpu
HW = TS.HW
GRAPH_FIELDS = (('node_vertex', torch.int32), ('node_view', torch.int32), ('corner_node', torch.int32), ('adj_off', torch.int64),
                ('adj_seam', torch.int32), ('adj_node', torch.int32))


def np_(t):
    return t.cpu().numpy()


def _gpu_mesh(verts, faces, normals=None):
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    normals = np.zeros_like(verts) if normals is None else np.ascontiguousarray(normals, np.float32)
    return Mesh(torch.from_numpy(verts), torch.from_numpy(np.ascontiguousarray(faces, np.int32).reshape(-1, 3)), torch.from_numpy(normals)).to('cuda')


def _same(got, want, what=''):
    want = torch.from_numpy(np.ascontiguousarray(want))
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert torch.equal(got.cpu(), want), (what, int((got.cpu() != want).sum()))


def _same_graph(g, G, what=''):
    for name, dtype in GRAPH_FIELDS:
        assert getattr(g, name).dtype == dtype and getattr(g, name).is_cuda
        _same(getattr(g, name), G[name], (what, name))
    assert g.nodes == len(G['node_vertex']) and g.nnz == len(G['adj_node'])


def _same_solve(got, want, what=''):
    (g, info), (G, INFO) = got, want
    _same(g, G, what)
    assert info['iterations'] == INFO['iterations'], (what, info, INFO)
    assert info['rho'] == INFO['rho'] and info['rho0'] == INFO['rho0'], (what, info, INFO)


def _hand_tm(mesh, a):
    """the TexturedMesh of a texture_ref atlas dict"""
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
    return texture.TexturedMesh(mesh, cu(a['uv']), cu(a['texture']), cu(a['valid']), cu(a['label']), cu(a['patch']), a['density'], None, None,
                                cu(a['screen']), cu(a['order']), [int(c) for c in a['layout']['count']])


def _workspace(pattern, **sizes):
    return torch.full((seams.seam_workspace_bytes(**sizes),), pattern, dtype=torch.uint8, device='cuda')


@pytest.fixture(scope='module')
def cams():
    P = SS.cameras4()
    return P, TS.random_images(len(P))[0]


def _stages(c, P, images, o=0.5, workspace=None, **solve):
    """every stage and the composed call on a hand-labelled mesh against the restatement -> (the device's levelled TexturedMesh, the restatement)"""
    m = _gpu_mesh(c['verts'], c['faces'])
    a = SS.hand_atlas(c, P, images, o)
    L = SR.level_atlas(a, c['verts'], c['faces'], images, P, o, **solve)
    G = L['graph']
    g = seams.seam_graph(m, torch.from_numpy(c['label']).cuda(), views=len(P), workspace=workspace)
    _same_graph(g, G)
    f = seams.node_colors(g, m, images, P=P, pixel_center=o, workspace=workspace)
    _same(f, L['f'], 'f')
    x = np.random.RandomState(4).normal(size=(g.nodes, 3))
    _same(seams.apply_operator(g, torch.from_numpy(x).cuda(), 0.1, 1e-3, workspace=workspace), SR.apply_operator(G, x, 0.1, 1e-3), 'A x')
    _same_solve(seams.solve_levels(g, f, workspace=workspace, **solve), (L['g'], L['info']), 'solve')
    tm = _hand_tm(m, a)
    info = {}
    lev = seams.level_atlas(tm, images, P=P, pixel_center=o, workspace=workspace, info=info, **solve)
    _same(lev.texture, L['texture'], 'texture')
    _same(lev.valid, L['valid'], 'valid')
    assert lev.uv is tm.uv and lev.patch is tm.patch and lev.face_view is tm.face_view and info['iterations'] == L['info']['iterations']
    zero = seams.levelled_fill(tm, images, g, torch.zeros(g.nodes, 3, dtype=torch.float64, device='cuda'), o, workspace=workspace)
    _same(zero[0], a['texture'], 'g = 0 is the plain atlas')
    _same(zero[1], a['valid'])
    return lev, L, a


@pytest.mark.parametrize('name', SS.SMALL)
def test_small_cases(cams, name):
    P, images = cams
    c = SS.small_case(name)
    lev, L, a = _stages(c, P, images, 0.0 if name == 'gaps' else 0.5)
    if name in ('single', 'empty'):                                           # no seam: g = 0 in 0 iterations, the plain atlas byte for byte
        assert L['info']['iterations'] == [0, 0, 0] and not L['g'].any() and not bool(lev.levels.any())
        _same(lev.texture, a['texture'])
    else:
        assert max(L['info']['iterations']) > 0 and (L['texture'] != a['texture']).any()
    if name == 'single':
        m = _gpu_mesh(c['verts'], c['faces'])
        plain = texture._fill(torch.from_numpy(images).cuda(), 0.5, torch.from_numpy(a['label']).cuda(), torch.from_numpy(a['screen']).cuda(),
                              torch.from_numpy(a['order']).cuda(), a['layout']['count'], m.vertices, m.faces, torch.from_numpy(P).cuda(), (128, 128, 128))
        assert torch.equal(plain[0], lev.texture) and torch.equal(plain[1], lev.valid)


@pytest.mark.parametrize('nodes', [63, 64, 65, 2048, 2049])
def test_strips_at_wave_and_tree_chunk_edges(nodes):
    faces, label, m = SS.strip(nodes)
    G = SR.seam_graph(faces, label)
    mesh = _gpu_mesh(np.zeros((m, 3), np.float32), faces)
    g = seams.seam_graph(mesh, torch.from_numpy(label).cuda(), views=2)
    _same_graph(g, G)
    rs = np.random.RandomState(nodes)
    x, f = rs.normal(size=(nodes, 3)), rs.uniform(0, 255, (nodes, 3))
    _same(seams.apply_operator(g, torch.from_numpy(x).cuda(), 0.25, 1e-2), SR.apply_operator(G, x, 0.25, 1e-2))
    want = SR.solve_levels(G, f, cg_iters=25)
    assert want[1]['iterations'] == [25, 25, 25]                               # a budget that ends before convergence
    _same_solve(seams.solve_levels(g, torch.from_numpy(f).cuda(), cg_iters=25), want)


@pytest.mark.parametrize('iters', [0, 1, 7])
def test_budgets(cams, iters):
    P, images = cams
    _, L, _ = _stages(SS.small_case('island'), P, images, cg_iters=iters)
    assert L['info']['iterations'] == [iters] * 3


def test_a_loose_tolerance_ends_the_channels_apart(cams):
    faces, label, m = SS.strip(65)
    G = SR.seam_graph(faces, label)
    f = np.random.RandomState(0).uniform(0, 255, (65, 3))
    f[:, 1] = 7.0                                                             # a constant channel has b = 0: done at the start
    f[:, 2] *= 1e-3
    want = SR.solve_levels(G, f, cg_tol=0.3)
    assert want[1]['iterations'][1] == 0 and 0 < want[1]['iterations'][0] < 200
    g = seams.seam_graph(_gpu_mesh(np.zeros((m, 3), np.float32), faces), torch.from_numpy(label).cuda(), views=2)
    _same_solve(seams.solve_levels(g, torch.from_numpy(f).cuda(), cg_tol=0.3), want)


@pytest.fixture(scope='module', params=['sphere', 'torus'])
def scene(request):
    """texture_scene's marching-cubes mesh from the device, seven cameras, random images, and both atlases"""
    vol, spacing, origin = TS.volume(request.param)
    m = M.marching_cubes(vol, 0.0, spacing, origin)
    P = TS.twin_cameras()
    images = TS.random_images(len(P))[0]
    t = texture.build_atlas(m, images, P=P)
    a = T.build_atlas(np_(m.vertices), np_(m.normals), np_(m.faces), P, np_(t.raster.depth), images, 0.5)
    return dict(mesh=m, P=P, images=images, t=t, a=a)


def test_scene_with_random_images(scene):
    s = scene
    m, a = s['mesh'], s['a']
    assert 1000 <= len(a['label']) <= 4000 and (a['label'] < 0).any()
    _same(s['t'].texture, a['texture'])
    L = SR.level_atlas(a, np_(m.vertices), np_(m.faces), s['images'], s['P'], cg_iters=60)
    assert L['graph']['adj_seam'].max() >= 2
    info = {}
    lev = seams.level_atlas(s['t'], s['images'], cg_iters=60, info=info)
    _same_graph(lev.seam_graph, L['graph'])
    _same(lev.levels, L['g'])
    _same(lev.texture, L['texture'])
    _same(lev.valid, a['valid'])
    assert info['iterations'] == L['info']['iterations'] and info['rho'] == L['info']['rho']
    both = texture.build_atlas(m, s['images'], P=s['P'], level_seams=True, level_options=dict(cg_iters=60))
    assert torch.equal(both.texture, lev.texture) and torch.equal(both.valid, lev.valid) and torch.equal(both.uv, s['t'].uv)
    assert torch.equal(both.patch, s['t'].patch) and torch.equal(both.face_view, s['t'].face_view)


def test_truth_scene():
    verts, faces, normals = SS.sphere_mesh()
    P = SS.S.cameras()
    images = SS.truth_images(P, SS.OFFSETS)
    m = _gpu_mesh(verts, faces, normals)
    info = {}
    lev = texture.build_atlas(m, images, P=P, level_seams=True, level_options=dict(info=info))
    a = T.build_atlas(verts, normals, faces, P, np_(lev.raster.depth), images, 0.5)
    L = SR.level_atlas(a, verts, faces, images, P)
    _same(lev.levels, L['g'])
    _same(lev.texture, L['texture'])
    assert info['iterations'] == L['info']['iterations'] and max(info['iterations']) < 200
    before, _ = SR.seam_rms(L['graph'], L['f'], np.zeros_like(L['g']))
    after, _ = SR.seam_rms(L['graph'], L['f'], np_(lev.levels))
    assert after / before <= 2 * 0.0325                                        # test_seams_host.py's bound, on the device's g


@pytest.mark.parametrize('pattern', POISON_PATTERNS)
def test_workspaces_of_poison(cams, pattern):
    P, images = cams
    c = SS.small_case('fan')
    ws = _workspace(pattern, faces=len(c['faces']), vertices=len(c['verts']), views=len(P), nodes=3 * len(c['faces']))
    _stages(c, P, images, workspace=ws)
    faces, label, m = SS.strip(2049)                                          # two levels of the tree
    G = SR.seam_graph(faces, label)
    ws = _workspace(pattern, faces=len(faces), vertices=m, views=2, nodes=2049)
    g = seams.seam_graph(_gpu_mesh(np.zeros((m, 3), np.float32), faces), torch.from_numpy(label).cuda(), views=2, workspace=ws)
    _same_graph(g, G)
    f = np.random.RandomState(1).uniform(0, 255, (2049, 3))
    ws.fill_(pattern)
    _same_solve(seams.solve_levels(g, torch.from_numpy(f).cuda(), cg_iters=12, workspace=ws), SR.solve_levels(G, f, cg_iters=12))


def test_refusals(cams):
    P, images = cams
    c = SS.small_case('fan')
    m = _gpu_mesh(c['verts'], c['faces'])
    label = torch.from_numpy(c['label']).cuda()
    g = seams.seam_graph(m, label, views=4)
    bad = label.clone()
    bad[3] = 4
    with pytest.raises(ValueError, match='label'):                            # a label >= V, through its error bit
        seams.seam_graph(m, bad, views=4)
    bad[3] = -2
    with pytest.raises(ValueError, match='label'):
        seams.seam_graph(m, bad, views=4)
    g5 = seams.seam_graph(m, (label + 1).contiguous())                        # labels 1 .. 4 are fine without a view count ...
    with pytest.raises(ValueError, match='label'):                            # ... and refused by the colours of four images
        seams.node_colors(g5, m, images, P=P)
    faces = c['faces'].copy()
    faces[2, 1] = len(c['verts'])
    with pytest.raises(ValueError, match='index'):
        seams.seam_graph(_gpu_mesh(c['verts'], faces), label, views=4)
    verts = c['verts'].copy()
    verts[0, 1] = np.nan
    with pytest.raises(ValueError, match='NaN or infinite'):                  # a non-finite vertex
        seams.node_colors(g, _gpu_mesh(verts, c['faces']), images, P=P)
    f = seams.node_colors(g, m, images, P=P)
    # wrong dtypes and shapes: before any launch
    for call in (lambda: seams.seam_graph(m, label.long(), views=4), lambda: seams.seam_graph(m, label[:-1], views=4),
                 lambda: seams.seam_graph(m, label.cpu(), views=4), lambda: seams.seam_graph(m, label, views=0),
                 lambda: seams.node_colors(g, m, images.astype(np.float32), P=P), lambda: seams.node_colors(g, m, images, P=P[:3]),
                 lambda: seams.node_colors(g, m, images, P=P, pixel_center=0.25),
                 lambda: seams.apply_operator(g, f.float(), 0.1, 1e-3), lambda: seams.apply_operator(g, f[:-1], 0.1, 1e-3),
                 lambda: seams.apply_operator(g, f, -0.1, 1e-3), lambda: seams.apply_operator(g, f, 0.1, 0.0),
                 lambda: seams.solve_levels(g, f, cg_iters=-1), lambda: seams.solve_levels(g, f, cg_iters=2.5),
                 lambda: seams.solve_levels(g, f, cg_tol=float('nan')), lambda: seams.solve_levels(g, f.cpu()),
                 lambda: seams.solve_levels(g, f, workspace=torch.zeros(16, dtype=torch.uint8, device='cuda')),
                 lambda: seams.solve_levels(g, f, workspace=torch.zeros(1 << 16, dtype=torch.float32, device='cuda')),
                 lambda: seams.level_atlas(object(), images, P=P)):
        with pytest.raises(ValueError):
            call()
    plain = texture.build_atlas(m, images, P=P)
    with pytest.raises(ValueError, match='level_options'):
        texture.build_atlas(m, images, P=P, level_seams=True, level_options=3)
    plain.screen = None
    with pytest.raises(ValueError, match='TexturedMesh of build_atlas'):
        seams.level_atlas(plain, images, P=P)


def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_' + name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_tool_changes_only_colours(tmp_path):
    from PIL import Image
    verts, faces, normals = SS.sphere_mesh()
    P = SS.S.cameras()
    images = SS.truth_images(P, SS.OFFSETS, o=0.0)
    scene = tmp_path / 'scene'
    os.makedirs(str(scene / 'image_hd'))
    for v in range(len(P)):
        Image.fromarray(images[v]).save(str(scene / 'image_hd' / ('%06d.png' % v)))
    np.savez(str(scene / 'cameras_hd.npz'), **{'world_mat_%d' % v: P[v] for v in range(len(P))})
    src = str(tmp_path / 'in.obj')
    _gpu_mesh(verts, faces, normals).export(src)
    tool = _tool('texture_mesh')
    a = tool.main([src, str(tmp_path / 'plain.obj'), '--data_dir', str(scene), '--no_masks'])
    b = tool.main([src, str(tmp_path / 'level.obj'), '--data_dir', str(scene), '--no_masks', '--level_seams', '--seam_smoothness', '0.2'])
    for name in ('uv', 'valid', 'face_view', 'patch'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert not torch.equal(a.texture, b.texture) and torch.equal(a.texture[a.valid == 0], b.texture[b.valid == 0])
    strip = lambda p: open(str(tmp_path / p)).read().replace('level', 'plain')   # noqa: E731
    assert strip('level.obj') == strip('plain.obj') and strip('level.mtl') == strip('plain.mtl')
    with Image.open(str(tmp_path / 'level.png')) as im:
        assert np.array_equal(np.asarray(im), np_(b.texture))
