"""Texture atlases on the device (mvsdf_amd/texture.py, csrc/texture.hip) against the numpy restatement tests/texture_ref.py: every array equal, no
tolerances.  The restatement is given the depth maps the device drew (tests/test_gpu_raster.py holds those to their own restatement).  Then the
tool and the evaluation command end to end on a small scene."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import raster_ref as R
import texture_ref as T
import texture_scene as TS
import train_scene
from conftest import ROOT
from mvsdf_amd import evaluation, mesh, raster, texture, training
from mvsdf_amd._lib import MvsdfError
from mvsdf_amd.mesh import Mesh

pytestmark = pytest.mark.gpu
HW = TS.HW


def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_' + name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def np_(t):
    return t.cpu().numpy()


def _gpu_mesh(verts, faces, normals):
    return Mesh(torch.from_numpy(np.ascontiguousarray(verts, np.float32)), torch.from_numpy(np.ascontiguousarray(faces, np.int32)),
                torch.from_numpy(np.ascontiguousarray(normals, np.float32))).to('cuda')


def _same_atlas(t, a, what=''):
    """a TexturedMesh against the restatement's dict"""
    assert t.uv.dtype == torch.float32 and t.texture.dtype == torch.uint8 and t.valid.dtype == torch.uint8
    assert t.face_view.dtype == torch.int32 and t.patch.dtype == torch.int32
    assert np.array_equal(np_(t.face_view), a['label']), what
    assert np.array_equal(np_(t.score).view(np.uint64), a['score'].view(np.uint64)), what
    assert t.density == a['density'], what
    assert np.array_equal(np_(t.patch), a['patch']), what
    assert np.array_equal(np_(t.uv).view(np.uint32), a['uv'].view(np.uint32)), what
    assert t.texture.shape == a['texture'].shape and np.array_equal(np_(t.valid), a['valid']), what
    assert np.array_equal(np_(t.texture), a['texture']), (what, int((np_(t.texture) != a['texture']).sum()))


@pytest.fixture(scope='module', params=['sphere', 'torus'])
def scene(request):
    """a marching-cubes mesh from the device with gaps in its normals, 7 cameras (the last the twin of the second), random images and masks, and
    the device's rasters for both pixel centres"""
    vol, spacing, origin = TS.volume(request.param)
    m = mesh.marching_cubes(vol, 0.0, spacing, origin)
    normals = TS.normals_with_gaps(np_(m.normals))
    m = Mesh(m.vertices, m.faces, torch.from_numpy(normals).cuda())
    P = TS.twin_cameras()
    images, masks = TS.random_images(len(P))
    rast = {o: raster.rasterize(m, P=P, hw=HW, pixel_center=o) for o in (0.5, 0.0)}
    return dict(mesh=m, verts=np_(m.vertices), faces=np_(m.faces), normals=normals, P=P, images=images, masks=masks, raster=rast,
                depth={o: np_(r.depth) for o, r in rast.items()})


@pytest.mark.parametrize('o', [0.5, 0.0])
def test_face_views(scene, o):
    s = scene
    for mk in (None, s['masks']):
        st = {}
        label, score, _ = T.face_views(s['verts'], s['normals'], s['faces'], s['P'], s['depth'][o], o, mk, stats=st)
        if mk is None:
            TS.check_cases(label, st, twin=(1, 6))                               # the inputs exercise the cases
        got_l, got_s = texture.face_views(s['mesh'], s['raster'][o], masks=mk)
        assert got_l.dtype == torch.int32 and got_s.dtype == torch.float64
        assert np.array_equal(np_(got_l), label) and np.array_equal(np_(got_s).view(np.uint64), score.view(np.uint64))
        if mk is not None:
            assert (label != T.face_views(s['verts'], s['normals'], s['faces'], s['P'], s['depth'][o], o)[0]).any()   # the masks change labels
            got_b = texture.face_views(s['mesh'], s['raster'][o], masks=torch.from_numpy(mk).bool())
            assert torch.equal(got_b[0], got_l) and torch.equal(got_b[1], got_s)
    for kw in (dict(ignore_normals=True), dict(cos_min=0.5, depth_tol=0.0)):
        label, score, _ = T.face_views(s['verts'], s['normals'], s['faces'], s['P'], s['depth'][o], o, s['masks'], **kw)
        got_l, got_s = texture.face_views(s['mesh'], s['raster'][o], masks=s['masks'], **kw)
        assert np.array_equal(np_(got_l), label) and np.array_equal(np_(got_s).view(np.uint64), score.view(np.uint64)), kw


@pytest.mark.parametrize('d', [1.0, 3.0])
def test_build_atlas(scene, d):
    s = scene
    for o, mk in (((0.5, None),) if d == 1.0 else ((0.0, s['masks']),)):
        a = T.build_atlas(s['verts'], s['normals'], s['faces'], s['P'], s['depth'][o], s['images'], o, mk, texel_density=d)
        TS.check_classes(np.asarray(a['layout']['count']))                       # at least three classes, one of them odd
        assert a['valid'].any() and not a['valid'].all() and a['density'] == d
        t = texture.build_atlas(s['mesh'], s['images'], P=s['P'], pixel_center=o, masks=mk, texel_density=d)
        _same_atlas(t, a, (o, d))
        assert t.mesh is s['mesh'] and t.texture.is_cuda and t.uv.is_cuda and t.valid.is_cuda and t.face_view.is_cuda and t.patch.is_cuda


def test_the_schedule_and_the_screen_table_change_nothing(scene):
    s = scene
    a = texture.build_atlas(s['mesh'], s['images'], P=s['P'], masks=s['masks'])
    for kw in (dict(P=s['P'], view_chunk=1), dict(P=s['P'], view_chunk=4, large_face_pixels=0), dict(raster=s['raster'][0.5]),
               dict(P=torch.from_numpy(s['P']), recompute=True)):
        b = texture.build_atlas(s['mesh'], torch.from_numpy(s['images']).cuda(), masks=s['masks'], **kw)
        for name in ('uv', 'texture', 'valid', 'face_view', 'patch', 'score'):
            assert torch.equal(getattr(a, name), getattr(b, name)), (sorted(kw), name)
        assert a.density == b.density


def test_the_max_size_loop(scene):
    s = scene
    full = T.build_atlas(s['verts'], s['normals'], s['faces'], s['P'], s['depth'][0.5], s['images'], 0.5, texel_density=3.0)
    side = full['texture'].shape[1]
    a = T.build_atlas(s['verts'], s['normals'], s['faces'], s['P'], s['depth'][0.5], s['images'], 0.5, texel_density=3.0, max_size=side // 4)
    assert a['density'] < 3.0 and a['texture'].shape[1] <= side // 4
    t = texture.build_atlas(s['mesh'], s['images'], P=s['P'], texel_density=3.0, max_size=side // 4)
    _same_atlas(t, a)
    with pytest.raises(ValueError, match='do not fit'):
        texture.build_atlas(s['mesh'], s['images'], P=s['P'], max_size=16)


def _check(verts, faces, normals, P, images, o=0.5, hw=HW, **kw):
    m = _gpu_mesh(verts, faces, normals)
    r = raster.rasterize(m, P=P, hw=hw, pixel_center=o)
    a = T.build_atlas(verts, normals, faces, P, np_(r.depth), images, o, **kw)
    t = texture.build_atlas(m, images, P=P, pixel_center=o, **kw)
    _same_atlas(t, a)
    return t, a


# A camera whose projection is exact in fp64: a vertex (X, Y, 0) with X, Y multiples of 1/4 lands on the integer pixel (240 + focal X / 2,
# 32 - focal Y / 2) for the focal lengths 40 and 200.  With pixel centres at integers a lone face then covers the pixels of its own corners (two edge functions are exactly 0 there): it is visible
# without a neighbour.
EXACT_HW = (64, 480)


def _exact_camera(focal):
    return R.look_at((0.0, 0.0, 2.0), (0.0, 0.0, 0.0), EXACT_HW, focal, up=(0.0, 1.0, 0.0))[None]


def test_degenerate_meshes():
    P = _exact_camera(40.0)
    images = np.random.RandomState(0).randint(0, 256, (1,) + EXACT_HW + (3,)).astype(np.uint8)
    up = np.array([[0.0, 0.0, 1.0]] * 4, np.float32)
    quad = np.array([[-0.25, -0.25, 0.0], [0.25, -0.25, 0.0], [-0.25, 0.25, 0.0], [0.25, 0.25, 0.0]], np.float32)
    # one face: one cell, its second half empty
    t, a = _check(quad[:3], np.array([[0, 1, 2]], np.int32), up[:3], P, images, o=0.0, hw=EXACT_HW)
    n = int(a['patch'][0, 2])
    assert a['label'][0] == 0 and n > 4 and a['texture'].shape == (n, n, 3) and a['valid'].sum() == n * (n + 1) // 2
    # two faces in one cell
    t, a = _check(quad, np.array([[0, 1, 2], [2, 1, 3]], np.int32), up, P, images, o=0.0, hw=EXACT_HW)
    assert (a['label'] == 0).all() and a['patch'][0, 2] == a['patch'][1, 2] and (a['patch'][:, :2] == 0).all() and a['patch'][:, 3].tolist() == [0, 1]
    assert a['valid'].all()
    # a mesh no camera sees (behind the camera): the fallback everywhere
    t, a = _check(quad + np.float32(50.0), np.array([[0, 1, 2], [2, 1, 3]], np.int32), up, P, images, o=0.0, hw=EXACT_HW, fallback=(1, 2, 3))
    assert (a['label'] == -1).all() and not a['valid'].any() and a['texture'].shape == (4, 4, 3)
    assert not np_(t.valid).any() and (np_(t.texture) == np.array([1, 2, 3], np.uint8)).all() and not np_(t.score).any()
    # an empty mesh
    for nv in (0, 5):
        e = Mesh(torch.zeros(nv, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(nv, 3)).to('cuda')
        t = texture.build_atlas(e, images, P=P)
        assert t.uv.shape == (0, 3, 2) and t.face_view.shape == (0,) and t.patch.shape == (0, 4) and t.density == 1.0
        assert t.texture.shape == (4, 4, 3) and bool((t.texture == 128).all()) and not bool(t.valid.any())
        label, score = texture.face_views(e, raster.rasterize(e, P=P, hw=EXACT_HW))
        assert label.shape == (0,) and score.shape == (0,)


def test_a_face_with_a_400_pixel_edge_is_clamped_to_n_max():
    P = _exact_camera(200.0)
    verts = np.array([[-2.0, -0.25, 0.0], [2.0, -0.25, 0.0], [-2.0, 0.25, 0.0], [1.0, 0.0, 0.0], [1.25, 0.0, 0.0], [1.0, 0.25, 0.0]], np.float32)
    faces = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    normals = np.array([[0.0, 0.0, 1.0]] * 6, np.float32)
    images = np.random.RandomState(0).randint(0, 256, (1,) + EXACT_HW + (3,)).astype(np.uint8)
    t, a = _check(verts, faces, normals, P, images, o=0.0, hw=EXACT_HW)
    s = a['screen'][0]
    assert (a['label'] == 0).all() and abs(s[2] - s[0]) == 400.0              # the edge a-b spans 400 px
    assert a['patch'][0, 2] == T.N_MAX and 4 < a['patch'][1, 2] < T.N_MAX
    assert (2 * T.N_MAX - 7) ** 2 < 4 * 400.0 ** 2                             # the clamp, not the rule, gives 256


def test_a_lookup_of_the_device_atlas_gives_the_image_within_one_grey_level():
    s = TS.inside_scene()
    images = TS.linear_images(len(s['P']))
    m = _gpu_mesh(s['verts'], s['faces'], s['normals'])
    for o in (0.5, 0.0):
        for d in (1.0, 3.0):
            t = texture.build_atlas(m, images, P=s['P'], pixel_center=o, texel_density=d)
            r = t.raster
            a = T.build_atlas(s['verts'], s['normals'], s['faces'], s['P'], np_(r.depth), images, o, texel_density=d)
            _same_atlas(t, a, (o, d))
            dev = dict(label=np_(t.face_view), screen=a['screen'], cls=a['cls'], uv=np_(t.uv), texture=np_(t.texture))
            worst = TS.meaning_error(dev, images, o, np.random.RandomState(4))
            assert worst <= 1.0 + 1e-9, (o, d, worst)


def test_argument_errors(scene):
    s = scene
    m, P, im = s['mesh'], s['P'], s['images']
    with pytest.raises(ValueError, match='images must be uint8'):
        texture.build_atlas(m, im.astype(np.float32), P=P)
    with pytest.raises(ValueError, match='images must be uint8'):
        texture.build_atlas(m, im[0], P=P)
    with pytest.raises(ValueError, match='cameras for'):
        texture.build_atlas(m, im, P=P[:3])
    with pytest.raises(ValueError, match='either P'):
        texture.build_atlas(m, im)
    with pytest.raises(ValueError, match='masks must be'):
        texture.build_atlas(m, im, P=P, masks=s['masks'][:, :-1])
    with pytest.raises(ValueError, match='the raster is'):
        texture.build_atlas(m, im[:, :-2], raster=s['raster'][0.5])
    for bad in (float('nan'), float('inf'), 0.0, -1.0):
        with pytest.raises(ValueError, match='texel_density'):
            texture.build_atlas(m, im, P=P, texel_density=bad)
    for bad in (3, 8.0, True, 2 ** 16, None):
        with pytest.raises(ValueError, match='max_size'):
            texture.build_atlas(m, im, P=P, max_size=bad)
    for bad in ((1, 2), (0, 0, 256), (0.5, 0.5, 0.5)):
        with pytest.raises(ValueError, match='fallback'):
            texture.build_atlas(m, im, P=P, fallback=bad)
    with pytest.raises(ValueError, match='pixel_center'):
        texture.build_atlas(m, im, P=P, pixel_center=0.25)
    with pytest.raises(ValueError, match='Mesh is needed'):
        texture.build_atlas((s['verts'], s['faces']), im, P=P)
    with pytest.raises(ValueError, match='Raster'):
        texture.face_views(m, None)
    with pytest.raises(ValueError, match='cos_min'):
        texture.face_views(m, s['raster'][0.5], cos_min=float('nan'))
    fb = m.faces.clone()
    fb[3, 1] = m.vertices.shape[0]
    with pytest.raises(ValueError, match='face index'):
        texture.face_views(Mesh(m.vertices, fb, m.normals), s['raster'][0.5])
    cpu = Mesh(m.vertices.cpu(), m.faces.cpu(), m.normals.cpu())
    with pytest.raises(MvsdfError, match='runs on the GPU'):
        texture.build_atlas(cpu, im, P=P)
    with pytest.raises(MvsdfError, match='runs on the GPU'):
        texture.face_views(cpu, s['raster'][0.5])
    with pytest.raises(ValueError, match='extension'):
        texture.build_atlas(m, im, P=P).export('/nonexistent/a.ply')


# ---------------------------------------------------------------- end to end ----------------------------------------------------------------
@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """a small scene, a two-epoch run on it and its evaluation with a simplified mesh but without the texture"""
    scene = train_scene.write_scene(tmp_path_factory.mktemp('dtu_texture'), 3, pmask=False, seed=1)
    conf = train_scene.write_conf(tmp_path_factory.mktemp('conf_texture') / 'test.conf')
    root = str(tmp_path_factory.mktemp('run_texture'))
    training.main(['--data_dir', scene[0], '--conf', conf, '--batch_size', '2', '--nepoch', '2', '--expname', 'tx', '--gpu', 'ignore',
                   '--exps_root', root, '--seed', '1', '--feat_ckpt', scene[1]], printer=lambda *a: None)
    argv = ['--data_dir', scene[0], '--conf', conf, '--expname', 'tx', '--exps_root', root, '--feat_ckpt', scene[1], '--resolution', '48',
            '--simplify_faces', '400']
    res = evaluation.main(argv, printer=lambda *a: None)
    return dict(scene=scene, argv=argv, res=res, obj=os.path.join(res['evaldir'], 'surface_world_coordinates_2.obj'))


def test_texture_mesh_in_the_evaluation_and_the_tool(trained, tmp_path):
    from PIL import Image
    t = trained
    stem = os.path.join(t['res']['evaldir'], 'surface_world_coordinates_2_textured')
    assert 'textured_mesh' not in t['res'] and not any(os.path.exists(stem + e) for e in ('.obj', '.mtl', '.png'))
    before = {n: open(os.path.join(t['res']['evaldir'], n), 'rb').read() for n in sorted(os.listdir(t['res']['evaldir']))}
    res = evaluation.main(t['argv'] + ['--texture_mesh'], printer=lambda *a: None)
    for n, data in before.items():                                            # the other outputs as without the option, byte for byte
        assert open(os.path.join(res['evaldir'], n), 'rb').read() == data, n
    assert sorted(set(os.listdir(res['evaldir'])) - set(before)) == ['surface_world_coordinates_2_textured' + e for e in ('.mtl', '.obj', '.png')]
    tm, simp = res['textured_mesh'], res['simplified_mesh']
    assert tm.mesh is simp and 0 < len(simp) <= 400 and int((tm.face_view >= 0).sum()) > 0 and bool(tm.valid.any())
    back = mesh.load_mesh(stem + '.obj')
    assert torch.equal(back.vertices, simp.vertices.cpu()) and torch.equal(back.faces, simp.faces.cpu()) and torch.equal(back.normals, simp.normals.cpu())
    with Image.open(stem + '.png') as im:
        assert np.array_equal(np.asarray(im.convert('RGB')), np_(tm.texture))
    lines = open(stem + '.obj').read().split('\n')
    assert lines[0] == 'mtllib surface_world_coordinates_2_textured.mtl' and lines[1] == 'usemtl surface_world_coordinates_2_textured'
    vt = np.array([ln.split()[1:] for ln in lines if ln.startswith('vt ')], np.float32)
    assert np.array_equal(vt.reshape(-1, 3, 2).view(np.uint32), np_(tm.uv).view(np.uint32))
    ft = [ln.split()[1:] for ln in lines if ln.startswith('f ')]
    assert [int(tok.split('/')[1]) for f in ft for tok in f] == list(range(1, 3 * len(simp) + 1))
    assert 'map_Kd surface_world_coordinates_2_textured.png' in open(stem + '.mtl').read()
    # against the restatement on the scene's own files
    P, images, masks = raster.scene_views(t['scene'][0])
    a = T.build_atlas(np_(simp.vertices), np_(simp.normals), np_(simp.faces), P, np_(tm.raster.depth), images, 0.0, masks)
    _same_atlas(tm, a)
    # the tool on the written OBJ, simplifying as the evaluation did: the same atlas
    out = str(tmp_path / 'tex.obj')
    c = _tool('texture_mesh').main([t['obj'], out, '--data_dir', t['scene'][0], '--faces', '400'])
    for name in ('uv', 'texture', 'valid', 'face_view', 'patch'):
        assert torch.equal(getattr(c, name), getattr(tm, name)), name
    assert all(os.path.exists(str(tmp_path / ('tex' + e))) for e in ('.obj', '.mtl', '.png'))
    c = _tool('texture_mesh').main([t['obj'], str(tmp_path / 'nomask.obj'), '--data_dir', t['scene'][0], '--cell', '0.2', '--no_masks', '--density', '2'])
    assert c.density == 2.0 and int((c.face_view >= 0).sum()) > 0
