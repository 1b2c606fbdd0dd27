"""Texture atlases on the device: a mesh, typically the simplified one, gets a texture image from the input photographs, so that a few ten thousand
faces keep the photographs' detail.  Every face is labelled with the view that sees it largest, gets a patch sized from that view, the patches
are packed into one atlas, and every texel is gathered from the photograph of its face's view.  Kernels: csrc/texture.hip (the design:
DESIGN.md); tests/texture_ref.py restates every step in numpy.  The reference has no texturing code; the definition below is this project's,
written so that the schedule cannot change a bit of the result.

The definition (fp64 throughout, in the order written, no FMA contraction; fp32 and uint8 inputs are promoted exactly; every integer decision is
an exact comparison).  Cameras, pixel_center o, the projection of a vertex, E(p, q, r), the matrix-vector order, the dot-product order and the
visibility rule are those of raster.py, word for word.

1. Face labels (face_views).  For face f = (a, b, c) and the views v = 0 .. V-1 in order, v is a candidate iff all three vertices are visible in v
   (vertex_visibility's rule, with depth_tol and with masks where given), all three (sx - o, sy - o) lie in [0, W-1] x [0, H-1],
   A = E(sa, sb, sc) != 0, and the normal test passes: n = (n_a + n_b) + n_c (the stored vertex normals, per component),
   X_c = ((X_a + X_b) + X_c) / 3, g = C_v - X_c, cosang = (n.g) / sqrt((g.g) * (n.n)), passing iff cosang > cos_min; n.n == 0 passes with
   ignore_normals=True and fails without.  The score is |A|; the label is the candidate with the largest score, ties to the lowest view, -1
   without a candidate.  label int32 [F], score fp64 [F] (0 where unlabelled).
2. Patch size.  L2 = the largest of the three squared screen-space edge lengths (dx*dx + dy*dy) of the face in its view.  With d = texel_density
   (texels per image pixel) the patch edge n is the smallest power of two in [N_MIN = 4, N_MAX = 256] with (2n - 7)^2 >= ((4*L2)*d)*d, N_MAX if
   there is none; unlabelled faces get N_MIN.  The leg of the patch triangle is l = n - 3.5 texels, so the face's longest edge has a texel per
   image pixel / d along a leg.
3. Packing.  The faces are ordered by n descending, stable in the face index.  The k-th face of a class sits in cell k >> 1 of that class, in half
   k & 1 (an odd class leaves half 1 of its last cell empty).  The classes follow each other in descending order along one Morton curve over
   blocks of N_MIN x N_MIN texels: a cell of edge n takes (n / N_MIN)^2 consecutive block indices starting at `off`, a multiple of that count
   because all earlier cells are at least as large; its origin is N_MIN * (x, y), x made of the even bits of `off`, y of the odd bits.  With T
   blocks in all and B the smallest integer with T <= 2^B the atlas is Wt = N_MIN * 2^ceil(B/2) by Ht = N_MIN * 2^floor(B/2) texels (an empty
   mesh: 4 x 4).  Cells never overlap, each is aligned to its own size, and more than half of the blocks are used once T > 1.
   While Wt > max_size the density is halved and step 2 repeated (a pass that returns the seven class counts); when even F faces of N_MIN do
   not fit: ValueError.  The density finally used is reported.
4. UVs.  In the cell frame [0, n]^2, origin added, corner a at the right angle, with the inset e = 0.75:
       half 0:  a = (e, e)          b = (e + l, e)          c = (e, e + l)
       half 1:  a = (n - e, n - e)  b = (n - e - l, n - e)  c = (n - e, n - e - l)
   uv fp32 [F,3,2] = (x / Wt, 1 - y / Ht), computed in fp64 and rounded once (every value is a multiple of 1/4 over a power of two: exact).  The y
   axis of the image array points down, OBJ's v up.
5. Texel fill.  Texel (i, j) has its centre at (i + 0.5, j + 0.5).  Its owner needs no table: the block (i / N_MIN, j / N_MIN) Morton-encoded is a
   block index; the class and the cell follow from that index and the seven class offsets; with p the centre in the cell frame the texel is of
   half 0 iff floor(p.x) + floor(p.y) <= n - 1.  Blocks at or past T and the empty half of an odd class's last cell get `fallback` and valid = 0,
   as do the texels of unlabelled faces.  For half 1 p is replaced by (n - p.x, n - p.y).  beta = (p.x - e) / l, gamma = (p.y - e) / l,
   alpha = (1 - beta) - gamma; the source position is s = (alpha*s_a + beta*s_b) + gamma*s_c per coordinate, s_* the screen coordinates of the
   face's vertices in its view; u = s.x - o and t = s.y - o are clamped to [0, W-1] and [0, H-1] (the gutter extrapolates) and fusion's
   bilinear rule (raster.py) gives the colour c per channel; texel = uint8(floor(c + 0.5)).  The whole of each half is filled, gutter included.

The copy is AFFINE in the image: the atlas holds the photograph's triangle as it is, which is how atlases of photographs are built; it is not
perspective-correct inside a face (for the small faces of a dense mesh the difference is below a pixel).

Why a bilinear lookup inside a face's UV triangle touches only that face's texels.  A lookup at (x, y) reads the texels floor(x - 0.5) + {0, 1} by
floor(y - 0.5) + {0, 1}.  In half 0 the triangle is x, y >= e and x + y <= 2e + l = n - 2, so both indices are >= floor(e - 0.5) = 0 and their
sum is at most floor(x + y - 1) + 2 <= n - 1: texels of half 0.  In half 1 it is x, y <= n - e and x + y >= n + 2, so both indices are
<= floor(n - e - 0.5) + 1 = n - 1 and their sum exceeds x + y - 3 >= n - 1, i.e. is >= n: texels of half 1.  Both hypotenuses keep 2 (measured
in x + y) from the cell's diagonal.  (With the corner at 1 instead of 0.75, at the same leg, the hypotenuses keep only 1.5 and the argument fails
for half 1: in a cell of n = 8 the lookup at (4.3, 5.3) reads texel (3, 4), which is of half 0.  The argument needs 2e + l <= n - 2, and
0.75 is the largest inset that gives it at this leg; the legs keep a gutter of 0.75 >= 0.5 texels from the cell's edges.)

Argument errors (shapes or dtypes that disagree, V != the number of cameras, texel_density not finite or <= 0, max_size below N_MIN, above 32768 or
not an int, a fallback outside 0 .. 255) raise ValueError before anything is launched; a mesh on the CPU raises MvsdfError.  At most 2^28 faces.
An empty mesh gives an empty result: no faces, the 4 x 4 atlas of the fallback colour.
"""
import ctypes
import os

import numpy as np
import torch

from . import raster as R
from ._lib import check, lib, K, raise_for_bits, _header, _stream, _vp
from .mesh import _write_textured_obj

N_MIN, N_MAX, CLASSES = 4, 256, 7
MAX_SIZE = K.MVSDF_TX_MAX_SIDE
MAX_FACES = 1 << K.MVSDF_TX_MAX_FACES_LOG2


class TexturedMesh:
    """The result of build_atlas: mesh (the Mesh that was textured), uv fp32 [F,3,2], texture uint8 [Ht,Wt,3], valid uint8 [Ht,Wt] (1: the texel
    was gathered from a photograph), face_view int32 [F] (-1: no view), patch int32 [F,4] = (x0, y0, n, half), all on the device; density, the
    texel density finally used; raster, the Raster behind the labels; screen fp64 [F,6], order int32 [F] and counts (seven ints): what the fill
    read, which seams.level_atlas reads again.  An atlas of charts (charts.build_chart_atlas) has patch, order and counts None and carries
    face_chart int32 [F], chart_view int32 [C], chart_rect int32 [C,6] = (X, Y, w, h, u0, t0) and face_map int32 [Ht,Wt] instead."""

    def __init__(self, mesh, uv, texture, valid, face_view, patch, density, raster=None, score=None, screen=None, order=None, counts=None,
                 face_chart=None, chart_view=None, chart_rect=None, face_map=None):
        self.mesh, self.uv, self.texture, self.valid, self.face_view, self.patch = mesh, uv, texture, valid, face_view, patch
        self.density, self.raster, self.score = density, raster, score
        self.screen, self.order, self.counts = screen, order, counts
        self.face_chart, self.chart_view, self.chart_rect, self.face_map = face_chart, chart_view, chart_rect, face_map

    def export(self, path):
        """write `path` (.obj: mtllib, usemtl, v, vn, one vt per face corner, f a/t/a b/t/b c/t/c; floats as %.9g), <stem>.mtl (map_Kd <stem>.png)
        and <stem>.png (the texture, through PIL) beside it"""
        from PIL import Image
        stem, ext = os.path.splitext(path)
        if ext.lower() != '.obj':
            raise ValueError('TexturedMesh.export: unknown extension %r (.obj)' % ext)
        name = os.path.basename(stem)
        m = self.mesh
        _write_textured_obj(path, m.vertices.cpu().numpy().astype(np.float32), m.normals.cpu().numpy().astype(np.float32),
                            m.faces.cpu().numpy().astype(np.int32), self.uv.cpu().numpy().astype(np.float32), name + '.mtl', name)
        with open(stem + '.mtl', 'w') as fh:
            fh.write('newmtl %s\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd %s.png\n' % (name, name))
        Image.fromarray(self.texture.cpu().numpy()).save(stem + '.png')


def _view_args(mesh, raster, masks, depth_tol, cos_min, what):
    """what face_views checks and moves to the device -> (V, H, W, masks, depth_tol, cos_min, P, C, device)"""
    V, H, W, m, tol, dev = R._view_inputs(mesh, raster, masks, depth_tol, what)
    R._mesh(mesh, what)
    cmin = R._tol('cos_min', cos_min, what)
    if mesh.faces.shape[0] > MAX_FACES:
        raise ValueError('%s: %d faces (at most 2^28)' % (what, mesh.faces.shape[0]))
    try:
        C = R.camera_centers(raster.P)
    except np.linalg.LinAlgError as e:
        raise ValueError('%s: a camera has a singular projection' % what) from e
    if not np.isfinite(C).all():
        raise ValueError('%s: a camera centre is NaN or infinite' % what)
    return V, H, W, m, tol, cmin, C, dev


def _face_views(mesh, raster, masks, depth_tol, cos_min, ignore_normals, what):
    """-> (label, score, screen fp64 [F,6]) on the device"""
    V, H, W, m, tol, cmin, C, dev = _view_args(mesh, raster, masks, depth_tol, cos_min, what)
    nv, nf = mesh.vertices.shape[0], mesh.faces.shape[0]
    v, f, n = mesh.vertices.contiguous(), mesh.faces.to(dev).contiguous(), mesh.normals.to(dev).contiguous()
    Pd, Cd = torch.from_numpy(raster.P).to(dev), torch.from_numpy(C).to(dev)
    ws = torch.empty(256, dtype=torch.uint8, device=dev)
    label = torch.empty(nf, dtype=torch.int32, device=dev)
    score = torch.empty(nf, dtype=torch.float64, device=dev)
    screen = torch.empty(nf, 6, dtype=torch.float64, device=dev)
    check(lib().mvsdf_texture_face_views(_vp(v), _vp(n), _vp(f), nv, nf, _vp(Pd), _vp(Cd), V, H, W, raster.pixel_center, _vp(raster.depth.contiguous()),
                                         _vp(m), tol, cmin, 1 if ignore_normals else 0, _vp(ws), 256, _vp(label), _vp(score), _vp(screen),
                                         _stream(v)), 'mvsdf_texture_face_views')
    raise_for_bits(_header(ws, K.MVSDF_TX_H_WORDS)[K.MVSDF_TX_H_ERR], what, R.ERRORS)
    return label, score, screen


def face_views(mesh, raster, masks=None, depth_tol=0.01, cos_min=0.0, ignore_normals=False):
    """(label int32 [F], score fp64 [F]) on the device: step 1 of the module's definition for `mesh` in the views of `raster` (rasterize of this
    mesh: its cameras and pixel_center), optionally inside masks uint8 / bool [V,H,W]."""
    label, score, _ = _face_views(mesh, raster, masks, depth_tol, cos_min, ignore_normals, 'face_views')
    return label, score


def atlas_size(counts):
    """(Wt, Ht, T) of the seven class counts (class k: patches of edge N_MIN << k): step 3's atlas and its blocks in use.  The library derives
    the same from the counts and refuses a fill whose Ht x Wt differs."""
    T = sum(((int(c) + 1) >> 1) << (2 * k) for k, c in enumerate(counts))
    B = 0
    while (1 << B) < T:
        B += 1
    return N_MIN << ((B + 1) // 2), N_MIN << (B // 2), T


def _classify(label, screen, d, ws, cls):
    """one count pass at density d -> the seven class counts (cls is written)"""
    nf = label.shape[0]
    check(lib().mvsdf_texture_classify(_vp(label), _vp(screen), nf, d, _vp(ws), ws.numel(), _vp(cls), _stream(ws)), 'mvsdf_texture_classify')
    return _header(ws, K.MVSDF_TX_H_WORDS)[K.MVSDF_TX_H_COUNTS:]


def _pack(cls, counts, ws):
    """steps 3 and 4 for the classes `cls` with their counts -> (order int32 [F], patch int32 [F,4], uv fp32 [F,3,2])"""
    nf, dev = cls.shape[0], cls.device
    carr = (ctypes.c_int64 * CLASSES)(*counts)
    order = torch.empty(nf, dtype=torch.int32, device=dev)
    patch = torch.empty(nf, 4, dtype=torch.int32, device=dev)
    uv = torch.empty(nf, 3, 2, dtype=torch.float32, device=dev)
    check(lib().mvsdf_texture_pack(_vp(cls), nf, carr, _vp(ws), ws.numel(), _vp(order), _vp(patch), _vp(uv), _stream(ws)), 'mvsdf_texture_pack')
    raise_for_bits(_header(ws, K.MVSDF_TX_H_WORDS)[K.MVSDF_TX_H_ERR], 'build_atlas', [])
    return order, patch, uv


def _fill(img, o, label, screen, order, counts, verts, faces, Pd, fallback, recompute=False):
    """step 5 -> (texture uint8 [Ht,Wt,3], valid uint8 [Ht,Wt]); no wait"""
    V, H, W = img.shape[:3]
    Wt, Ht, _ = atlas_size(counts)
    carr = (ctypes.c_int64 * CLASSES)(*counts)
    texture = torch.empty(Ht, Wt, 3, dtype=torch.uint8, device=img.device)
    valid = torch.empty(Ht, Wt, dtype=torch.uint8, device=img.device)
    check(lib().mvsdf_texture_fill(_vp(img), V, H, W, o, _vp(label), _vp(screen), _vp(order), label.shape[0], carr, _vp(verts), _vp(faces),
                                   verts.shape[0], _vp(Pd), 1 if recompute else 0, int(fallback[0]), int(fallback[1]), int(fallback[2]), Ht, Wt,
                                   _vp(texture), _vp(valid), _stream(img)), 'mvsdf_texture_fill')
    return texture, valid


def build_atlas(mesh, images, P=None, cams=None, pixel_center=0.5, masks=None, raster=None, texel_density=1.0, max_size=8192,
                fallback=(128, 128, 128), depth_tol=0.01, cos_min=0.0, ignore_normals=False, large_face_pixels=None, view_chunk=None,
                recompute=False, level_seams=False, level_options=None, charts=False, chart_options=None):
    """The module's atlas of `mesh` (device tensors, world coordinates) from images uint8 [V,H,W,3] -> TexturedMesh.  The mesh is drawn into the
    cameras first (rasterize with large_face_pixels / view_chunk) unless `raster` holds that already.  recompute=True lets the fill project the
    face's corners again instead of reading the table step 1 wrote (the same bits; for measuring).  level_seams=True corrects the texture with
    seams.level_atlas (level_options: its smoothness, anchor, cg_iters, cg_tol, info); labels, UVs, patches and valid stay as they are.
    charts=True builds the atlas of charts instead (charts.build_chart_atlas; chart_options: its pad, min_faces, smooth_rounds, info); without it
    nothing of that module runs."""
    what = 'build_atlas'
    if chart_options is not None and not isinstance(chart_options, dict):
        raise ValueError('%s: chart_options must be a dict, got %s' % (what, type(chart_options).__name__))
    if charts:
        if recompute:
            raise ValueError('%s: recompute belongs to the per-face fill, not to charts=True' % what)
        from . import charts as CH
        return CH.build_chart_atlas(mesh, images, P=P, cams=cams, pixel_center=pixel_center, masks=masks, raster=raster, texel_density=texel_density,
                                    max_size=max_size, fallback=fallback, depth_tol=depth_tol, cos_min=cos_min, ignore_normals=ignore_normals,
                                    large_face_pixels=large_face_pixels, view_chunk=view_chunk, level_seams=level_seams, level_options=level_options,
                                    **(chart_options or {}))
    if level_options is not None and not isinstance(level_options, dict):
        raise ValueError('%s: level_options must be a dict, got %s' % (what, type(level_options).__name__))
    R._mesh(mesh, what)
    img = torch.as_tensor(images)
    if img.dim() != 4 or img.shape[3] != 3 or img.dtype != torch.uint8:
        raise ValueError('%s: images must be uint8 [V, H, W, 3], got %s %s' % (what, img.dtype, tuple(img.shape)))
    V, H, W = img.shape[:3]
    H, W = R._hw((H, W), what)
    if raster is None:
        Pm = R._cameras(P, cams, what)
        o = R._center(pixel_center, what)
    else:
        if not isinstance(raster, R.Raster):
            raise ValueError('%s: raster must be a Raster, got %s' % (what, type(raster).__name__))
        Pm, o = raster.P, raster.pixel_center
        if tuple(raster.depth.shape) != (V, H, W):
            raise ValueError('%s: the raster is %s, the images %s' % (what, tuple(raster.depth.shape), (V, H, W)))
    if len(Pm) != V:
        raise ValueError('%s: %d cameras for %d images' % (what, len(Pm), V))
    R._masks(masks, V, H, W, what)
    R._tol('depth_tol', depth_tol, what)
    R._tol('cos_min', cos_min, what)
    try:
        d = float(texel_density)
    except (TypeError, ValueError):
        raise ValueError('%s: texel_density must be a number, got %r' % (what, texel_density)) from None
    if not (np.isfinite(d) and d > 0):
        raise ValueError('%s: texel_density must be finite and > 0, got %r' % (what, texel_density))
    if isinstance(max_size, (bool, np.bool_)) or not isinstance(max_size, (int, np.integer)) or not N_MIN <= max_size <= MAX_SIZE:
        raise ValueError('%s: max_size must be an int in [%d, %d], got %r' % (what, N_MIN, MAX_SIZE, max_size))
    max_size = int(max_size)
    fb = np.asarray(fallback)
    if fb.shape != (3,) or not np.issubdtype(fb.dtype, np.integer) or fb.min() < 0 or fb.max() > 255:
        raise ValueError('%s: fallback must be three ints in 0 .. 255, got %r' % (what, fallback))
    nf = mesh.faces.shape[0]
    if nf > MAX_FACES:
        raise ValueError('%s: %d faces (at most 2^28)' % (what, nf))
    if atlas_size([nf] + [0] * (CLASSES - 1))[0] > max_size:                  # every face at N_MIN
        raise ValueError('%s: %d faces do not fit an atlas of %d texels a side, even at %d texels each' % (what, nf, max_size, N_MIN))
    dev = R._on_device(mesh, what)
    if raster is None:
        raster = R.rasterize(mesh, P=Pm, hw=(H, W), pixel_center=o, large_face_pixels=large_face_pixels, view_chunk=view_chunk)
    label, score, screen = _face_views(mesh, raster, masks, depth_tol, cos_min, ignore_normals, what)
    img = img.to(dev).contiguous()
    size = lib().mvsdf_texture_workspace_bytes(nf)
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    cls = torch.empty(nf, dtype=torch.uint8, device=dev)
    while True:
        counts = _classify(label, screen, d, ws, cls)
        if atlas_size(counts)[0] <= max_size:
            break
        d = d / 2.0
    order, patch, uv = _pack(cls, counts, ws)
    v, f = mesh.vertices.contiguous(), mesh.faces.to(dev).contiguous()
    texture, valid = _fill(img, o, label, screen, order, counts, v, f, torch.from_numpy(Pm).to(dev), fb, recompute)
    t = TexturedMesh(mesh, uv, texture, valid, label, patch, d, raster, score, screen, order, [int(c) for c in counts])
    if level_seams:
        from . import seams
        t = seams.level_atlas(t, img, P=Pm, pixel_center=o, fallback=fb, **(level_options or {}))
    return t


def texture_mesh_from_scene(mesh, data_dir, masks=True, **kw):
    """build_atlas of a world-coordinate mesh from a scene directory's image_hd/, cameras_hd.npz and (masks=True) mask_hd/ -> the TexturedMesh"""
    P, images, m = R.scene_views(data_dir, masks)
    return build_atlas(mesh, images, P=P, pixel_center=0.0, masks=m, **kw)
