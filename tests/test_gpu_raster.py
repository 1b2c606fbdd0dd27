"""Mesh rendering on the device (mvsdf_amd/raster.py, csrc/raster.hip) against the numpy restatement tests/raster_ref.py: every array equal,
no tolerances.  Then the tools and the evaluation command end to end on a small scene."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import raster_ref as R
import raster_scene as S
import train_scene
from conftest import ROOT
from mvsdf_amd import evaluation, mesh, raster, training
from mvsdf_amd._lib import lib
from mvsdf_amd.mesh import Mesh

pytestmark = pytest.mark.gpu


def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_' + name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def np_(t):
    return t.cpu().numpy()


def _gpu_mesh(verts, faces, normals=None):
    n = np.zeros_like(verts) if normals is None else normals
    return Mesh(torch.from_numpy(np.ascontiguousarray(verts)), torch.from_numpy(np.ascontiguousarray(faces)), torch.from_numpy(n)).to('cuda')


def _same_raster(r, depth, face, what=''):
    d, f = np_(r.depth), np_(r.face)
    assert d.dtype == np.float32 and f.dtype == np.int32 and d.shape == depth.shape
    assert np.array_equal(f, face), (what, int((f != face).sum()))
    assert np.array_equal(d.view(np.uint32), depth.view(np.uint32)), (what, int((d != depth).sum()))
    assert np.array_equal(np_(r.silhouette()), face >= 0)


@pytest.fixture(scope='module', params=['sphere', 'torus'])
def mc_scene(request):
    """a marching-cubes mesh from the device, 6 cameras, the restatement's rasters for both pixel centres"""
    kind = request.param
    vol, spacing, origin = S.volume(kind, 64 if kind == 'sphere' else 48)
    m = mesh.marching_cubes(vol, 0.0, spacing, origin)
    P = S.cameras()
    verts, faces, normals = np_(m.vertices), np_(m.faces), np_(m.normals)
    ref = {o: R.rasterize(verts, faces, P, S.HW, o) for o in (0.5, 0.0)}
    return dict(mesh=m, verts=verts, faces=faces, normals=normals, P=P, ref=ref)


@pytest.mark.parametrize('o', [0.5, 0.0])
def test_marching_cubes_meshes_are_drawn_as_the_restatement_draws_them(mc_scene, o):
    s = mc_scene
    depth, face = s['ref'][o]
    for v in range(len(s['P'])):                                              # the inputs exercise the case
        assert (face[v] >= 0).any() and (face[v] < 0).any(), v
    front, sx, sy, z = R.project(s['P'][5], s['verts'])
    assert (~front).any() and (front & ((sx < 0) | (sx > S.HW[1]) | (sy < 0) | (sy > S.HW[0]))).any()
    _same_raster(raster.rasterize(s['mesh'], P=s['P'], hw=S.HW, pixel_center=o), depth, face)
    _same_raster(raster.rasterize(s['mesh'], P=s['P'], hw=S.HW, pixel_center=o, view_chunk=4), depth, face, 'view_chunk=4')
    _same_raster(raster.rasterize(s['mesh'], P=torch.from_numpy(s['P']), hw=S.HW, pixel_center=o, view_chunk=1, pretest=False), depth, face, 'chunk 1')


def test_cams_give_the_raster_of_their_projection_matrices(mc_scene):
    s = mc_scene
    cams = np.zeros((len(s['P']), 2, 4, 4))
    for v, Pv in enumerate(s['P']):                                           # P = K4 @ E with K = I: the extrinsic carries the whole matrix
        cams[v, 0] = Pv
        cams[v, 1, :3, :3] = np.eye(3)
    from mvsdf_amd import fusion
    P = fusion.projection_matrices(cams)[0]
    depth, face = R.rasterize(s['verts'], s['faces'], P, S.HW, 0.5)
    _same_raster(raster.rasterize(s['mesh'], cams=cams, hw=S.HW), depth, face)


def test_triangle_soup():
    verts, faces, P = S.soup()
    st = {}
    depth, face = R.rasterize(verts, faces, P, S.SOUP_HW, 0.5, st)
    assert st['ties'] > 0 and not (face >= len(faces) - 30).any()             # pixels won on a tie, by the lower index
    assert (st['boxes'] == 0).any() and (st['boxes'].max(1) == S.SOUP_HW[0] * S.SOUP_HW[1]).all()
    for Pv in P:
        front = R.project(Pv, verts)[0][faces]
        assert (front.any(1) & ~front.all(1)).any()
    m = _gpu_mesh(verts, faces)
    for o in (0.5, 0.0):
        d, f = (depth, face) if o == 0.5 else R.rasterize(verts, faces, P, S.SOUP_HW, o)
        _same_raster(raster.rasterize(m, P=P, hw=S.SOUP_HW, pixel_center=o), d, f, o)


def test_large_face_path_gives_the_same_raster(mc_scene):
    verts, faces, P = S.soup()
    st = {}
    depth, face = R.rasterize(verts, faces, P, S.SOUP_HW, 0.5, st)
    boxes = st['boxes']
    n_large = int((boxes > raster.LARGE_FACE_PIXELS).sum())
    assert n_large > 0 and ((boxes > 0) & (boxes <= raster.LARGE_FACE_PIXELS)).any()   # faces above and below the default threshold
    m = _gpu_mesh(verts, faces)
    rs = {L: raster.rasterize(m, P=P, hw=S.SOUP_HW, large_face_pixels=L) for L in (0, 2 ** 40, None, 1, 7)}
    for L, r in rs.items():
        _same_raster(r, depth, face, L)
    assert rs[0].stats['large_items'] == int((boxes > 0).sum()) and rs[2 ** 40].stats['large_items'] == 0
    assert rs[None].stats['large_items'] == n_large
    # the marching-cubes mesh, whose faces are mostly a few pixels, with every face on the large path and with none
    s = mc_scene
    _same_raster(raster.rasterize(s['mesh'], P=s['P'], hw=S.HW, large_face_pixels=0), *s['ref'][0.5], 'mc, everything large')
    _same_raster(raster.rasterize(s['mesh'], P=s['P'], hw=S.HW, large_face_pixels=2 ** 40), *s['ref'][0.5], 'mc, nothing large')
    # the atomics that the plain-load test saves change nothing
    a = raster.rasterize(m, P=P, hw=S.SOUP_HW, stats=True)
    b = raster.rasterize(m, P=P, hw=S.SOUP_HW, stats=True, pretest=False)
    _same_raster(a, depth, face)
    _same_raster(b, depth, face)
    assert b.stats['atomics'] == b.stats['covered'] == a.stats['covered'] and 0 < a.stats['atomics'] <= b.stats['atomics']


def _check_visibility_and_colors(m, verts, normals, P, depth, images, masks, o):
    r = raster.rasterize(m, P=P, hw=depth.shape[1:], pixel_center=o)
    out = {}
    for mk in (None, masks):
        vis = R.visibility(verts, P, depth, o, mk)
        got = raster.vertex_visibility(m, r, masks=mk)
        assert got.dtype == torch.uint8 and np.array_equal(np_(got), vis)
        if mk is not None:
            assert np.array_equal(np_(raster.vertex_visibility(m, r, masks=torch.from_numpy(mk).bool())), vis)
        assert np.array_equal(np_(raster.vertex_visibility(m, r, masks=mk, depth_tol=0.0)), R.visibility(verts, P, depth, o, mk, 0.0))
        for kw in (dict(), dict(ignore_normals=True), dict(cos_min=0.5, fallback=(0.1, 0.2, 0.3))):
            col, used = R.colors(verts, normals, P, depth, images, o, mk, **kw)
            c = raster.color_vertices(m, images, P=P, pixel_center=o, masks=mk, **kw)
            assert c.vertex_colors.dtype == torch.float32 and c.n_views.dtype == torch.int32
            assert np.array_equal(np_(c.n_views), used), kw
            assert np.array_equal(np_(c.vertex_colors).view(np.uint32), col.view(np.uint32)), kw
            assert c.vertices is m.vertices and c.faces is m.faces and c.normals is m.normals
            c2 = raster.color_vertices(m, torch.from_numpy(images).cuda(), raster=r, masks=mk, **kw)      # a raster drawn before
            assert torch.equal(c2.vertex_colors, c.vertex_colors) and torch.equal(c2.n_views, c.n_views)
            out[(mk is not None, tuple(kw))] = (vis, col, used)
    return out


@pytest.mark.parametrize('o', [0.5, 0.0])
def test_visibility_and_colours_of_the_marching_cubes_meshes(mc_scene, o):
    s = mc_scene
    rs = np.random.RandomState(3)
    images = rs.randint(0, 256, (len(s['P']),) + S.HW + (3,)).astype(np.uint8)
    masks = (rs.uniform(size=(len(s['P']),) + S.HW) > 0.3).astype(np.uint8)
    normals = s['normals'].copy()
    normals[rs.choice(len(normals), len(normals) // 20, replace=False)] = 0.0
    m = Mesh(s['mesh'].vertices, s['mesh'].faces, torch.from_numpy(normals).cuda())
    out = _check_visibility_and_colors(m, s['verts'], normals, s['P'], s['ref'][o][0], images, masks, o)
    vis, _, used = out[(False, ())]
    vism = out[(True, ())][0]
    assert vis.any() and not vis.all() and ((vis == 1) & (vism == 0)).any()
    assert (used > 0).any() and (used == 0).any()


def test_visibility_and_colours_of_the_two_layer_scene():
    L = S.layers()
    depth, face = R.rasterize(L['verts'], L['faces'], L['P'], S.HW, 0.5)
    m = _gpu_mesh(L['verts'], L['faces'], L['normals'])
    _same_raster(raster.rasterize(m, P=L['P'], hw=S.HW), depth, face)
    out = _check_visibility_and_colors(m, L['verts'], L['normals'], L['P'], depth, L['images'], L['masks'], 0.5)
    vis, col, used = out[(False, ())]
    vism = out[(True, ())][0]
    assert vis.any(0).sum() > 100 and (~vis.any(0)).sum() > 100               # visible and never-seen vertices; hidden ones per view
    assert ((vis == 1) & (vism == 0)).any()                                   # rejected only by the mask
    assert (used == 0).any() and (col[used == 0] == np.float32(0.5)).all() and (used == len(L['P'])).any()
    flat = ~L['normals'].any(1)
    assert flat.any() and out[(False, ('ignore_normals',))][2][flat].any() and not used[flat].any()


def test_error_paths_do_not_fault(mc_scene):
    s = mc_scene
    m, P = s['mesh'], s['P']
    nv, nf, V, (H, W) = len(s['verts']), len(s['faces']), len(P), S.HW
    L = lib()
    size = L.mvsdf_raster_workspace_bytes(nv, nf, V, H, W)
    assert size >= 256 + V * H * W * 8
    for bad in ((-1, 1, 1, 4, 4), (1, 1, 0, 4, 4), (1, 1, 65536, 4, 4), (1, 1, 1, 1, 4), (1, 1, 1, 4, 1), (2 ** 31, 1, 1, 4, 4), (1, 2 ** 30, 2, 4, 4),
                (1, 1, 1, 2 ** 16, 2 ** 15)):
        assert L.mvsdf_raster_workspace_bytes(*bad) == 0, bad
    ws = torch.empty(size, dtype=torch.uint8, device='cuda')
    Pd = torch.from_numpy(P).cuda()
    v, f = m.vertices, m.faces
    depth = torch.empty(V, H, W, dtype=torch.float32, device='cuda')
    face = torch.empty(V, H, W, dtype=torch.int32, device='cuda')

    def draw(v=v, f=f, nv=nv, Pd=Pd, size=size, o=0.5, large=64):
        return L.mvsdf_raster_draw(v.data_ptr(), f.data_ptr(), nv, nf, Pd.data_ptr(), V, H, W, o, large, 0, ws.data_ptr(), size, None)

    def header():
        torch.cuda.synchronize()
        return [int(x) for x in ws[:32].view(torch.int64).cpu()]
    assert draw(size=size - 1) != 0 and draw(size=255) != 0 and draw(o=0.25) != 0 and draw(large=-1) != 0     # refused before any launch
    assert L.mvsdf_raster_resolve(V, H, W, ws.data_ptr(), 256 + V * H * W * 8 - 1, depth.data_ptr(), face.data_ptr(), None) != 0
    assert b'workspace' in L.mvsdf_last_error()
    assert draw() == 0 and header()[0] == 0
    # a face that refers to a missing vertex: its error bit, the face not drawn, no fault
    fb = f.clone()
    fb[5, 1] = nv
    fb[9, 0] = -3
    assert draw(f=fb) == 0 and header()[0] == 2
    with pytest.raises(ValueError, match='face index'):
        raster.rasterize(Mesh(v, fb, m.normals), P=P, hw=S.HW)
    # a NaN camera at the C boundary: its error bit (the Python layer refuses it before)
    Pn = Pd.clone()
    Pn[2, 1, 1] = float('nan')
    assert draw(Pd=Pn) == 0 and header()[0] == 1
    vis = torch.empty(V, nv, dtype=torch.uint8, device='cuda')
    hdr = torch.empty(256, dtype=torch.uint8, device='cuda')
    assert L.mvsdf_raster_visibility(v.data_ptr(), nv, Pn.data_ptr(), V, H, W, 0.5, depth.data_ptr(), None, 0.01, hdr.data_ptr(), 256,
                                     vis.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert int(hdr[:8].view(torch.int64).cpu()[0]) == 1
    assert L.mvsdf_raster_visibility(v.data_ptr(), nv, Pd.data_ptr(), V, H, W, 0.5, depth.data_ptr(), None, 0.01, hdr.data_ptr(), 255,
                                     vis.data_ptr(), None) != 0
    with pytest.raises(ValueError, match='NaN or infinite'):
        raster.rasterize(m, P=np_(Pn), hw=S.HW)
    # the device is fine afterwards, and two runs give equal outputs
    a = raster.rasterize(m, P=P, hw=S.HW)
    b = raster.rasterize(m, P=P, hw=S.HW)
    _same_raster(a, *s['ref'][0.5])
    assert torch.equal(a.depth, b.depth) and torch.equal(a.face, b.face)
    images = torch.randint(0, 256, (V, H, W, 3), dtype=torch.uint8, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    ca, cb = raster.color_vertices(m, images, raster=a), raster.color_vertices(m, images, raster=b)
    assert torch.equal(ca.vertex_colors, cb.vertex_colors) and torch.equal(ca.n_views, cb.n_views)
    assert torch.equal(raster.vertex_visibility(m, a), raster.vertex_visibility(m, b))


def test_an_empty_mesh_gives_an_empty_raster():
    P = S.cameras()
    for nv in (0, 5):
        e = Mesh(torch.zeros(nv, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(nv, 3)).to('cuda')
        r = raster.rasterize(e, P=P, hw=S.HW)
        assert r.depth.shape == (6,) + S.HW and not r.depth.any() and (r.face == -1).all() and not r.silhouette().any()
        vis = raster.vertex_visibility(e, r)
        assert vis.shape == (6, nv) and not vis.any()
        c = raster.color_vertices(e, np.zeros((6,) + S.HW + (3,), np.uint8), P=P)
        assert c.vertex_colors.shape == (nv, 3) and (c.vertex_colors == 0.5).all() and not c.n_views.any()


# ---------------------------------------------------------------- end to end ----------------------------------------------------------------
@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """a scene without pmask/, a two-epoch run on it and its evaluation without rendering"""
    scene = train_scene.write_scene(tmp_path_factory.mktemp('dtu_raster'), 3, pmask=False, seed=1)
    conf = train_scene.write_conf(tmp_path_factory.mktemp('conf_raster') / 'test.conf')
    root = str(tmp_path_factory.mktemp('run_raster'))
    training.main(['--data_dir', scene[0], '--conf', conf, '--batch_size', '2', '--nepoch', '2', '--expname', 'ra', '--gpu', 'ignore',
                   '--exps_root', root, '--seed', '1', '--feat_ckpt', scene[1]], printer=lambda *a: None)
    argv = ['--data_dir', scene[0], '--conf', conf, '--expname', 'ra', '--exps_root', root, '--feat_ckpt', scene[1], '--resolution', '48']
    res = evaluation.main(argv, printer=lambda *a: None)
    return dict(scene=scene, conf=conf, root=root, argv=argv, res=res, obj=os.path.join(res['evaldir'], 'surface_world_coordinates_2.obj'))


def test_color_mesh_in_the_evaluation_and_the_tool(trained, tmp_path):
    t = trained
    assert 'color_mesh' not in t['res']
    obj = open(t['obj'], 'rb').read()
    ply = os.path.join(t['res']['evaldir'], 'surface_world_coordinates_2_color.ply')
    assert not os.path.exists(ply)
    res = evaluation.main(t['argv'] + ['--color_mesh'], printer=lambda *a: None)
    assert open(t['obj'], 'rb').read() == obj                                 # the OBJ as without the option, byte for byte
    got = mesh.load_mesh(ply)
    want = res['color_mesh']
    assert torch.equal(got.vertices, want.vertices.cpu()) and torch.equal(got.faces, want.faces.cpu()) and torch.equal(got.normals, want.normals.cpu())
    assert float(got.vertex_colors.min()) >= 0 and float(got.vertex_colors.max()) <= 1
    assert torch.equal(got.vertex_colors, torch.round(want.vertex_colors.cpu() * 255.0).clamp(0, 255) / 255.0)
    assert int((want.n_views > 0).sum()) > 0
    # against the restatement on the scene's own files
    P, images, masks = raster.scene_views(t['scene'][0])
    m = res['mesh']
    depth, _ = R.rasterize(np_(m.vertices), np_(m.faces), P, images.shape[1:3], 0.0)
    col, used = R.colors(np_(m.vertices), np_(m.normals), P, depth, images, 0.0, masks)
    assert np.array_equal(np_(want.n_views), used) and np.array_equal(np_(want.vertex_colors).view(np.uint32), col.view(np.uint32))
    # the tool on the written OBJ: a PLY that reads back with colours in [0, 1]
    out = str(tmp_path / 'colored.ply')
    c = _tool('color_mesh').main([t['obj'], out, '--data_dir', t['scene'][0]])
    back = mesh.load_mesh(out)
    assert back.vertex_colors is not None and float(back.vertex_colors.min()) >= 0 and float(back.vertex_colors.max()) <= 1
    assert len(back) == len(m) and torch.equal(c.n_views, want.n_views)
    c = _tool('color_mesh').main([t['obj'], str(tmp_path / 'nomask.obj'), '--data_dir', t['scene'][0], '--no_masks'])
    assert int(c.n_views.sum()) >= int(want.n_views.sum()) and mesh.load_mesh(str(tmp_path / 'nomask.obj')).vertex_colors is not None


def test_render_mesh_gives_a_scene_the_masks_eval_rendering_needs(trained, tmp_path):
    t = trained
    pmask = os.path.join(t['scene'][0], 'pmask')
    assert not os.path.exists(pmask)
    with pytest.raises(ValueError, match='pmask'):
        evaluation.main(t['argv'] + ['--eval_rendering'], printer=lambda *a: None)
    out = str(tmp_path / 'render')
    r = _tool('render_mesh').main([t['obj'], '--data_dir', t['scene'][0], '--out', out, '--mask_dir', pmask])
    from mvsdf_amd.utils import io as sio
    P, images, _ = raster.scene_views(t['scene'][0], masks=False)
    m = mesh.load_mesh(t['obj'])
    depth, face = R.rasterize(np_(m.vertices), np_(m.faces), P, images.shape[1:3], 0.0)
    assert (face >= 0).any()
    for i in range(len(P)):
        assert np.array_equal(np.ascontiguousarray(sio.load_pfm(os.path.join(out, 'depth', '%03d.pfm' % i))), depth[i])
        assert np.array_equal(sio.load_mask(os.path.join(pmask, '%03d.png' % i)), face[i] >= 0)
    _same_raster(r, depth, face)
    res = evaluation.main(t['argv'] + ['--eval_rendering'], printer=lambda *a: None)
    assert len(res['psnrs']) == len(P) and os.path.exists(os.path.join(res['evaldir'], 'psnr.txt'))
    with pytest.raises(SystemExit):                                           # the masks are there now: not written over
        _tool('render_mesh').main([t['obj'], '--data_dir', t['scene'][0], '--out', out, '--mask_dir', pmask])


@pytest.mark.parametrize('nf,nviews', [(512, 4), (683, 3)])
def test_large_face_list_across_a_scan_chunk_edge(nf, nviews):
    """faces x views = 2048 and 2049 items: the compaction of the flagged (face, view) items (csrc/geom_prims.h: mv_scan_blocks + mv_chunk_rank in k_ra_emit)
    ends exactly at, and one item beyond, the first 2048-item chunk"""
    verts, faces, P = S.soup()
    faces = np.ascontiguousarray(np.concatenate([faces] * (nf // len(faces) + 1))[:nf])
    faces[-1] = faces[0]                                                      # an ordinary triangle: the last item of the list is a drawn one
    P = np.concatenate([P, np.stack([R.look_at((-2.0, 2.2, 0.6), (0.0, 0.0, 0.0), S.SOUP_HW, 1.2 * S.SOUP_HW[0]),
                                     R.look_at((0.3, 0.4, 3.0), (0.0, 0.0, 0.0), S.SOUP_HW, 1.2 * S.SOUP_HW[0], up=(0.0, 1.0, 0.0))])])[:nviews]
    assert faces.shape[0] * P.shape[0] == (2048 if nviews == 4 else 2049)
    st = {}
    depth, face = R.rasterize(verts, faces, P, S.SOUP_HW, 0.5, st)
    boxes = st['boxes']
    assert (boxes[:, -1] > 0).all() and (boxes == 0).any() and (boxes.reshape(-1)[:2048] > 0).sum() > 1024   # the inputs exercise the case
    m = _gpu_mesh(verts, faces)
    every = raster.rasterize(m, P=P, hw=S.SOUP_HW, large_face_pixels=0)        # every drawn item is flagged and listed
    none = raster.rasterize(m, P=P, hw=S.SOUP_HW, large_face_pixels=2 ** 40)
    _same_raster(every, depth, face, 'large_face_pixels=0')
    _same_raster(none, depth, face, 'large_face_pixels=2**40')
    assert torch.equal(every.depth, none.depth) and torch.equal(every.face, none.face)
    assert every.stats['large_items'] == nf * nviews - int((boxes == 0).sum()) and none.stats['large_items'] == 0
