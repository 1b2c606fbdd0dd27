"""The numpy restatement of the mesh rendering definition (tests/raster_ref.py) against closed forms, the inputs of tests/test_gpu_raster.py against
the cases they must exercise, the Python layer's argument checks and the tools' parsers.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import mc_ref
import raster_ref as R
import raster_scene as S
from conftest import ROOT
from mvsdf_amd import raster
from mvsdf_amd._lib import MvsdfError
from mvsdf_amd.mesh import Mesh


def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_' + name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _front_camera(hw, focal):
    """at the origin looking down +z: sx = focal * X / Z + W / 2"""
    return R.look_at((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), hw, focal, up=(0.0, -1.0, 0.0))


def _square(x0, x1, y0, y1, d, P, hw):
    """the world square at depth d whose image is [x0, x1] x [y0, y1] under _front_camera, as two triangles"""
    Pinv = np.linalg.inv(P)
    c = [(Pinv @ np.array([sx * d, sy * d, d, 1.0]))[:3] for sx, sy in ((x0, y0), (x1, y0), (x1, y1), (x0, y1))]
    return np.asarray(c, np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int32)


@pytest.mark.parametrize('o', [0.5, 0.0])
def test_a_fronto_parallel_square_covers_the_pixels_whose_centres_lie_inside(o):
    hw = (40, 50)
    P = _front_camera(hw, 64.0)
    d = 2.5
    verts, faces = _square(10.25, 30.75, 5.25, 20.75, d, P, hw)               # image corners a quarter pixel off the lattice: exact in fp32
    front, sx, sy, z = R.project(P, verts)
    assert front.all() and np.array_equal(z, [d] * 4) and np.array_equal(sorted(set(sx)), [10.25, 30.75]) and np.array_equal(sorted(set(sy)), [5.25, 20.75])
    depth, face = R.rasterize(verts, faces, P[None], hw, o)
    ys, xs = np.mgrid[0:hw[0], 0:hw[1]]
    inside = (xs + o >= 10.25) & (xs + o <= 30.75) & (ys + o >= 5.25) & (ys + o <= 20.75)
    assert np.array_equal(face[0] >= 0, inside) and inside.sum() == (21 if o == 0.5 else 20) * (16 if o == 0.5 else 15)
    assert depth.dtype == np.float32 and face.dtype == np.int32
    assert np.array_equal(depth[0][inside], np.full(inside.sum(), np.float32(d))) and not depth[0][~inside].any()
    assert (face[0][~inside] == -1).all() and set(face[0][inside]) == {0, 1}


def test_duplicate_faces_give_the_lower_index_and_the_nearer_face_wins():
    hw = (40, 50)
    P = _front_camera(hw, 64.0)
    verts, faces = _square(10.25, 30.75, 5.25, 20.75, 2.5, P, hw)
    st = {}
    depth, face = R.rasterize(verts, np.concatenate([faces, faces, faces[::-1]]), P[None], hw, 0.5, st)
    assert set(face[0][face[0] >= 0]) == {0, 1} and st['ties'] > 0
    one = R.rasterize(verts, faces, P[None], hw)
    assert np.array_equal(depth, one[0]) and np.array_equal(face, one[1])
    near, nf = _square(15.25, 25.75, 8.25, 12.75, 1.5, P, hw)                 # a nearer, smaller square listed last
    depth, face = R.rasterize(np.concatenate([verts, near]), np.concatenate([faces, nf + 4]), P[None], hw)
    assert (depth[0, 9:13, 15:26] == np.float32(1.5)).all() and (face[0, 9:13, 15:26] >= 2).all() and depth[0, 6, 11] == np.float32(2.5)


def test_faces_behind_degenerate_or_off_screen_draw_nothing():
    hw = (40, 50)
    P = _front_camera(hw, 64.0)
    verts = np.array([[0, 0, 2], [1, 0, 2], [0, 1, -1],                       # one vertex behind: no clipping, the face is skipped
                      [0, 0, 2], [0, 0, 2], [1, 1, 2],                        # zero area
                      [50, 50, 2], [51, 50, 2], [50, 51, 2]], np.float32)     # off screen
    depth, face = R.rasterize(verts, np.arange(9, dtype=np.int32).reshape(3, 3), P[None], hw)
    assert not depth.any() and (face == -1).all()


def _plane_and_point():
    hw = (40, 50)
    front = R.look_at((0.0, 0.0, 3.0), (0.0, 0.0, 0.0), hw, 40.0, up=(0.0, 1.0, 0.0))
    back = R.look_at((0.0, 0.0, -3.0), (0.0, 0.0, 0.0), hw, 40.0, up=(0.0, 1.0, 0.0))
    verts = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0],          # the plane z = 0
                      [0.1, 0.05, -1.0], [0.2, 0.05, -1.0], [0.1, 0.15, -1.0]], np.float32)   # a small triangle below it
    faces = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6]], np.int32)
    return verts, faces, np.stack([front, back]), hw


def test_a_vertex_behind_a_nearer_plane_is_hidden_from_the_front_and_visible_from_the_back():
    verts, faces, P, hw = _plane_and_point()
    depth, face = R.rasterize(verts, faces, P, hw)
    vis = R.visibility(verts, P, depth)
    assert vis.shape == (2, 7) and vis.dtype == np.uint8
    assert not vis[0, 4:].any() and vis[1, 4:].all()
    masks = np.ones((2,) + hw, np.uint8)
    masks[1] = 0
    assert not R.visibility(verts, P, depth, masks=masks)[1].any()
    assert not R.visibility(verts, P, depth * np.float32(0.5))[1, 4:].any()    # a buffer that is nearer than the vertex hides it


def test_a_one_colour_image_gives_exactly_that_colour():
    verts, faces, P, hw = _plane_and_point()
    normals = np.zeros_like(verts)
    normals[:, 2] = -1.0                                                       # towards the back camera
    depth, face = R.rasterize(verts, faces, P, hw)
    images = np.empty((2,) + hw + (3,), np.uint8)
    images[:] = (200, 100, 50)
    col, used = R.colors(verts, normals, P, depth, images)
    assert col.dtype == np.float32 and used.dtype == np.int32
    assert np.array_equal(used[4:], [1, 1, 1])                                 # the back camera alone: the front one is behind the normal
    want = (np.array([200, 100, 50], np.float64) / 255.0).astype(np.float32)
    assert np.array_equal(col[4:], np.tile(want, (3, 1)))
    # two views that both see a vertex: still that colour; the front camera faces +z normals
    normals[:, 2] = 1.0
    col, used = R.colors(verts, normals, P, depth, images, fallback=(0.25, 0.5, 0.75))
    assert not used[4:].any() and np.array_equal(col[4:], np.tile(np.float32([0.25, 0.5, 0.75]), (3, 1)))
    normals[:] = 0.0
    col, used = R.colors(verts, normals, P, depth, images)
    assert not used.any() and (col == np.float32(0.5)).all()                   # zero normals are skipped ...
    col, used = R.colors(verts, normals, P, depth, images, ignore_normals=True)
    assert np.array_equal(used[4:], [1, 1, 1]) and np.array_equal(col[4:], np.tile(want, (3, 1)))   # ... unless asked for, at weight 1


def test_camera_centers():
    eye = np.array([0.3, -1.2, 2.0])
    P = R.look_at(eye, (0.1, 0.0, 0.0), (30, 40), 55.0)
    assert np.allclose(R.camera_centers(P[None])[0], eye, atol=1e-12)
    assert np.array_equal(raster.camera_centers(P[None]), R.camera_centers(P[None]))


# ---------------------------------------------------------------- the GPU tests' inputs exercise their cases ----------------------------------------------------------------
@pytest.mark.parametrize('kind', ['sphere', 'torus'])
def test_marching_cubes_scene_exercises_the_cases(kind):
    vol, spacing, origin = S.volume(kind, 48)
    verts, faces, normals = mc_ref.marching_cubes(vol, 0.0, spacing, origin)
    P = S.cameras()
    st = {}
    depth, face = R.rasterize(verts, faces, P, S.HW, 0.5, st)
    for v in range(len(P)):
        assert (face[v] >= 0).any() and (face[v] < 0).any(), v                # covered and empty pixels in every view
    front, sx, sy, z = R.project(P[5], verts)
    assert (~front).any() and front.any()                                     # part of the mesh is behind the last camera ...
    off = front & ((sx < 0) | (sx > S.HW[1]) | (sy < 0) | (sy > S.HW[0]))
    assert off.any()                                                          # ... and part of it off screen
    vis = R.visibility(verts, P, depth)
    assert vis.any() and not vis.all()


def test_soup_exercises_the_cases():
    verts, faces, P = S.soup()
    st = {}
    depth, face = R.rasterize(verts, faces, P, S.SOUP_HW, 0.5, st)
    assert st['ties'] > 0                                                     # a pixel won on a tie
    dup = face[face >= len(faces) - 30]
    assert dup.size == 0                                                      # ... which the earlier copy took
    boxes = st['boxes']
    assert (boxes > raster.LARGE_FACE_PIXELS).any() and ((boxes > 0) & (boxes <= raster.LARGE_FACE_PIXELS)).any()
    assert (boxes.max(1) == S.SOUP_HW[0] * S.SOUP_HW[1]).all()                # a face over the whole image in both views
    for Pv in P:
        front = R.project(Pv, verts)[0][faces]
        assert (front.any(1) & ~front.all(1)).any()                           # faces partly in front, partly behind
    assert (face >= 0).any() and (face < 0).sum() == 0                        # the huge faces leave no pixel empty


def test_layers_exercise_the_cases():
    L = S.layers()
    depth, face = R.rasterize(L['verts'], L['faces'], L['P'], S.HW, 0.5)
    vis = R.visibility(L['verts'], L['P'], depth)
    vism = R.visibility(L['verts'], L['P'], depth, masks=L['masks'])
    assert vis.any(0).sum() > 100 and (~vis.any(0)).sum() > 100               # seen and never-seen vertices
    assert ((vis == 1) & (vism == 0)).any() and not ((vis == 0) & (vism == 1)).any()   # rejected by the mask alone
    back = np.arange(len(L['verts'])) >= L['n_front']
    hidden = back & (np.abs(L['verts'][:, 0]) < 0.35) & (np.abs(L['verts'][:, 1]) < 0.35)
    assert hidden.sum() > 50 and not vis[:, hidden].any()                     # under the front sheet: hidden in every view
    col, used = R.colors(L['verts'], L['normals'], L['P'], depth, L['images'], masks=L['masks'])
    assert (used == 0).any() and (used == len(L['P'])).any()
    assert (col[used == 0] == np.float32(0.5)).all() and col.min() >= 0 and col.max() <= 1
    flat = ~L['normals'].any(1)
    assert flat.any() and not used[flat].any()
    col2, used2 = R.colors(L['verts'], L['normals'], L['P'], depth, L['images'], masks=L['masks'], ignore_normals=True)
    assert used2[flat].any() and np.array_equal(used2[~flat], used[~flat])


# ---------------------------------------------------------------- the Python layer ----------------------------------------------------------------
def _cpu_mesh():
    verts, faces, P, hw = _plane_and_point()
    n = np.zeros_like(verts)
    n[:, 2] = 1
    return Mesh(torch.from_numpy(verts), torch.from_numpy(faces), torch.from_numpy(n)), P, hw


def test_argument_errors_are_raised_before_the_device_is_touched():
    mesh, P, hw = _cpu_mesh()
    bad_face = Mesh(mesh.vertices, mesh.faces.clone(), mesh.normals)
    bad_face.faces[1, 2] = 7
    neg_face = Mesh(mesh.vertices, mesh.faces.clone(), mesh.normals)
    neg_face.faces[0, 0] = -1
    nan_P = P.copy()
    nan_P[1, 0, 2] = np.nan
    inf_P = P.copy()
    inf_P[0, 2, 3] = np.inf
    wide = Mesh(mesh.vertices, mesh.faces, mesh.normals)
    wide.vertices = torch.zeros(7, 4)
    f64 = Mesh(mesh.vertices, mesh.faces, mesh.normals)
    f64.faces = mesh.faces.long()
    for kw in (dict(mesh=mesh, P=P, hw=(1, 50)), dict(mesh=mesh, P=P, hw=(40, 1)), dict(mesh=mesh, P=P), dict(mesh=mesh, P=P, hw=(40,)),
               dict(mesh=mesh, P=nan_P, hw=hw), dict(mesh=mesh, P=inf_P, hw=hw), dict(mesh=mesh, P=P[:, :3], hw=hw), dict(mesh=mesh, hw=hw),
               dict(mesh=mesh, P=P, cams=np.zeros((2, 2, 4, 4)), hw=hw), dict(mesh=mesh, cams=np.zeros((2, 4, 4)), hw=hw),
               dict(mesh=bad_face, P=P, hw=hw), dict(mesh=neg_face, P=P, hw=hw), dict(mesh=wide, P=P, hw=hw), dict(mesh=f64, P=P, hw=hw),
               dict(mesh=mesh, P=P, hw=hw, pixel_center=0.25), dict(mesh=mesh, P=P, hw=hw, large_face_pixels=-1),
               dict(mesh=mesh, P=P, hw=hw, large_face_pixels=1.5), dict(mesh=mesh, P=P, hw=hw, view_chunk=0), dict(mesh='mesh', P=P, hw=hw)):
        with pytest.raises(ValueError):
            raster.rasterize(**kw)
    with pytest.raises(MvsdfError, match='GPU'):                              # everything is in order, but the mesh is on the CPU
        raster.rasterize(mesh, P=P, hw=hw)
    images = np.zeros((2,) + hw + (3,), np.uint8)
    for kw in (dict(images=images.astype(np.float32)), dict(images=images[..., :2]), dict(images=images[:1]), dict(images=images, P=nan_P),
               dict(images=images, masks=np.ones((2, 3, 3), np.uint8)), dict(images=images, masks=np.ones((2,) + hw, np.float32)),
               dict(images=images, depth_tol=np.nan), dict(images=images, cos_min=np.inf), dict(images=images, fallback=(0.5, 0.5)),
               dict(images=images, pixel_center=1.0), dict(images=images[:, :1])):
        kw.setdefault('P', P)
        with pytest.raises(ValueError):
            raster.color_vertices(mesh, **kw)
    with pytest.raises(ValueError):
        raster.color_vertices(bad_face, images, P=P)
    with pytest.raises(MvsdfError, match='GPU'):
        raster.color_vertices(mesh, images, P=P)
    r = raster.Raster(torch.zeros((2,) + hw), torch.full((2,) + hw, -1, dtype=torch.int32), P, 0.5)
    assert not r.silhouette().any()
    for kw in (dict(masks=np.ones((1,) + hw, np.uint8)), dict(depth_tol=np.inf)):
        with pytest.raises(ValueError):
            raster.vertex_visibility(mesh, r, **kw)
    with pytest.raises(ValueError):
        raster.vertex_visibility(mesh, 'raster')
    with pytest.raises(MvsdfError, match='GPU'):
        raster.vertex_visibility(mesh, r)


def test_cams_are_converted_with_the_fusion_matrices():
    from mvsdf_amd import fusion
    rs = np.random.RandomState(0)
    cams = np.zeros((3, 2, 4, 4))
    for v in range(3):
        cams[v, 0] = np.eye(4)
        cams[v, 0, :3] = rs.normal(size=(3, 4))
        cams[v, 1, :3, :3] = [[100.0 + v, 0, 20], [0, 101.0, 15], [0, 0, 1]]
    assert np.array_equal(raster._cameras(None, cams, 't'), fusion.projection_matrices(cams)[0])


def test_scene_views_reads_a_scene_directory(tmp_path):
    from PIL import Image
    d = tmp_path / 'scan'
    for sub in ('image_hd', 'mask_hd'):
        (d / sub).mkdir(parents=True)
    rs = np.random.RandomState(0)
    imgs = rs.randint(0, 256, (3, 6, 8, 3)).astype(np.uint8)
    masks = rs.randint(0, 2, (3, 6, 8)).astype(np.uint8) * 255
    cams = {}
    for i in range(3):
        Image.fromarray(imgs[i]).save(str(d / 'image_hd' / ('%06d.png' % i)))
        Image.fromarray(np.stack([masks[i]] * 3, -1)).save(str(d / 'mask_hd' / ('%03d.png' % i)))
        cams['world_mat_%d' % i] = rs.normal(size=(4, 4))
        cams['scale_mat_%d' % i] = np.eye(4)
    np.savez(str(d / 'cameras_hd.npz'), **cams)
    P, images, m = raster.scene_views(str(d))
    assert P.dtype == np.float64 and np.array_equal(P, np.stack([cams['world_mat_%d' % i] for i in range(3)]))
    assert np.array_equal(images, imgs) and m.dtype == bool and np.array_equal(m, masks > 0)
    assert raster.scene_views(str(d), masks=False)[2] is None


# ---------------------------------------------------------------- the tools and the ABI ----------------------------------------------------------------
def test_tool_parsers():
    a = _tool('color_mesh').parser().parse_args(['in.obj', 'out.ply', '--data_dir', 'scene'])
    assert (a.in_file, a.out_file, a.data_dir, a.no_masks, a.depth_tol, a.cos_min, a.ignore_normals) == ('in.obj', 'out.ply', 'scene', False, 0.01, 0.0, False)
    a = _tool('color_mesh').parser().parse_args(['i', 'o', '--data_dir', 's', '--no_masks', '--depth_tol', '0.05', '--cos_min', '0.2'])
    assert a.no_masks and a.depth_tol == 0.05 and a.cos_min == 0.2
    with pytest.raises(SystemExit):
        _tool('color_mesh').parser().parse_args(['in.obj', 'out.ply'])        # --data_dir is required
    rp = _tool('render_mesh').parser()
    a = rp.parse_args(['in.obj', '--data_dir', 'scene', '--out', 'dir'])
    assert (a.in_file, a.data_dir, a.out, a.mask_dir) == ('in.obj', 'scene', 'dir', None)
    assert rp.parse_args(['in.obj', '--data_dir', 's', '--out', 'd', '--mask_dir', 's/pmask']).mask_dir == 's/pmask'
    assert "own silhouette" in ' '.join(rp.format_help().split())
    with pytest.raises(SystemExit):
        rp.parse_args(['in.obj', '--data_dir', 'scene'])
    a = _tool('time_raster').parser().parse_args([])
    assert (a.resolutions, a.views, a.hw) == ('512,64', 49, '1200,1600')
    from mvsdf_amd import evaluation
    assert evaluation.eval_parser().parse_args([]).color_mesh is False and evaluation.eval_parser().parse_args(['--color_mesh']).color_mesh is True


def test_render_mesh_refuses_a_mask_dir_that_holds_images(tmp_path):
    from PIL import Image
    (tmp_path / 'pmask').mkdir()
    Image.fromarray(np.zeros((4, 4), np.uint8)).save(str(tmp_path / 'pmask' / '000.png'))
    (tmp_path / 'm.obj').write_text('v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n')
    with pytest.raises(SystemExit) as e:
        _tool('render_mesh').main([str(tmp_path / 'm.obj'), '--data_dir', str(tmp_path), '--out', str(tmp_path / 'o'), '--mask_dir', str(tmp_path / 'pmask')])
    assert e.value.code == 1 and not (tmp_path / 'o').exists()


def test_raster_symbols_are_declared_exported_and_built():
    import ctypes
    import re
    from mvsdf_amd import _lib, build
    names = ['mvsdf_raster_workspace_bytes', 'mvsdf_raster_draw', 'mvsdf_raster_resolve', 'mvsdf_raster_visibility', 'mvsdf_raster_colors']
    hdr = open(os.path.join(ROOT, 'include', 'mvsdf_hip.h')).read()
    L = ctypes.CDLL(build.build())
    for n in names:
        assert n in _lib.EXPORTS and re.search(r'\b%s\s*\(' % n, hdr) and getattr(L, n) is not None
    assert 'raster.hip' in build.SOURCES
    wb = _lib.lib().mvsdf_raster_workspace_bytes                              # a host function: sizes out of range give 0
    assert wb(100, 200, 4, 120, 160) >= 256 + 4 * 120 * 160 * 8 and wb(0, 0, 1, 2, 2) > 0
    for bad in ((-1, 1, 1, 4, 4), (1, -1, 1, 4, 4), (1, 1, 0, 4, 4), (1, 1, 65536, 4, 4), (1, 1, 1, 1, 4), (1, 1, 1, 4, 1), (2 ** 31, 1, 1, 4, 4),
                (1, 2 ** 31, 1, 4, 4), (1, 2 ** 30, 2, 4, 4), (1, 1, 1, 2 ** 16, 2 ** 15), (1, 1, 3, 2 ** 20, 2 ** 19 + 2 ** 18)):
        assert wb(*bad) == 0, bad
