"""Mesh rendering on the device: a triangle mesh drawn into the scene's cameras (depth maps, face ids, silhouettes), the visibility of its vertices
per view, and vertex colours taken from the input photographs.  Kernels: csrc/raster.hip (the design: DESIGN.md); tests/raster_ref.py restates
every step in numpy.  The reference has no code for this (its plots.py writes the trimming indicator as the colour); the definition below is
this project's, written so that the schedule cannot change a bit of the result.

The definition (fp64 throughout, in the order written, no FMA contraction; fp32 and uint8 inputs are promoted exactly):

- Cameras.  P fp64 [V,4,4] maps world coordinates to pixels; rows 0..2 are used, row 2 gives the camera depth.  cams [V,2,4,4] (utils.io.load_cam)
  are converted with fusion.projection_matrices.  A matrix-vector product is, per row, ((t0*q0 + t1*q1) + t2*q2) + t3*q3.  The camera centre is
  C_v = -inv(P_v[:3,:3]) @ P_v[:3,3] (host, numpy, passed as data).  pixel_center o is 0.5 or 0.0: pixel (x, y) has its centre at image coordinate
  (x + o, y + o).  0.5 is the MVS convention of fusion.py; 0.0 is that of cameras_hd.npz's world_mat_i, whose rays start at integer uv.
- Projection of a vertex X: p = P_v (X0, X1, X2, 1); in front iff p2 > 0; sx = p0 / p2, sy = p1 / p2, z = p2.
- Rasterisation of face f = (a, b, c) in view v.  The face is skipped if any of its vertices is not in front (THERE IS NO CLIPPING: a triangle that
  crosses the camera plane is not drawn at all, so a camera inside the scene loses the faces around it), or if any sx, sy, z is not finite.
  E(p, q, r) = (q.x - p.x)*(r.y - p.y) - (q.y - p.y)*(r.x - p.x); A = E(sa, sb, sc); skipped if A == 0; no back-face culling.  Candidate pixels:
  integers x in [max(0, ceil(min sx - o)), min(W-1, floor(max sx - o))], y likewise.  At the centre c = (x + o, y + o): w0 = E(sb, sc, c),
  w1 = E(sc, sa, c), w2 = E(sa, sb, c), all three and A negated if A < 0; covered iff w0 >= 0 and w1 >= 0 and w2 >= 0 (a pixel centre on a shared
  edge is covered by both faces; the key below decides).  b_i = w_i / A, iz = (b0/za + b1/zb) + b2/zc, zp = 1 / iz; the pixel is skipped unless zp
  is finite and > 0; d32 = fp32(zp) (round to nearest even), skipped if 0 or inf.  Key = (uint64(bits(d32)) << 32) | uint32(f).  The buffer starts at
  all ones and takes the MINIMUM key: the nearest surface wins, equal depths go to the lowest face index, and an integer minimum is the same in any
  order and any grouping.  depth fp32 [V,H,W] is 0 and face int32 [V,H,W] is -1 where nothing was drawn.
- Visibility of vertex i in view v against a depth buffer: in front; x = floor(sx - o + 0.5), y = floor(sy - o + 0.5) (the pixel whose centre is
  nearest) with 0 <= x < W, 0 <= y < H; D = depth[v, y, x] > 0; z <= fp64(D) * (1 + depth_tol); with masks, masks[v, y, x] set.  depth_tol = 0.01 is
  the slack of the reference's own depth test (gathered_depth * 0.99 in carving_t).
- Colours, per vertex over v = 0 .. V-1 in order, where the vertex is visible: g = C_v - X, cosang = (n.g) / sqrt(g.g) with dot products summed as
  (a0*b0 + a1*b1) + a2*b2 and n the normal as stored; wgt = cosang if cosang > cos_min, else the view is skipped.  A zero normal gives wgt = 1 with
  ignore_normals=True and skips the vertex without.  The image is sampled at u = sx - o, t = sy - o with fusion's bilinear rule: 0 <= u <= W-1 and
  0 <= t <= H-1 required, x0 = min(floor(u), W-2), fx = u - x0, y likewise, (c00*(1-fx) + c01*fx)*(1-fy) + (c10*(1-fx) + c11*fx)*fy per channel.
  S += wgt * colour, Wsum += wgt.  colour = fp32(S / Wsum / 255) if Wsum > 0, else the fallback; n_views = the number of views that contributed.

Argument errors (shapes or dtypes that disagree, H or W below 2, non-finite camera entries, face indices outside [0, Nv)) raise ValueError before
anything is launched; a mesh on the CPU raises MvsdfError.  An empty mesh gives an empty raster.
"""
import numpy as np
import torch

from ._lib import check, K, lib, MvsdfError, raise_for_bits, _header, _stream, _vp
from .mesh import Mesh

LARGE_FACE_PIXELS = 16                               # faces whose clamped pixel box holds more go to the wave-per-face path
KEY_BUDGET_PIXELS = 1 << 27                          # default view chunk: at most 1 GiB of keys ...
ITEM_BUDGET = 1 << 26                                # ... and 2^26 (face, view) pairs per draw
MAX_VIEWS = K.MVSDF_RA_MAX_VIEWS
INT32_MAX = 2 ** 31 - 1


class Raster:
    """The result of rasterize: depth fp32 [V,H,W] (0 where nothing was drawn) and face int32 [V,H,W] (-1) on the device; P (numpy fp64 [V,4,4]) and
    pixel_center as they were drawn; stats = {'large_items', 'atomics', 'covered'} summed over the view chunks (the last two only with stats=True)."""

    def __init__(self, depth, face, P, pixel_center, stats=None):
        self.depth, self.face, self.P, self.pixel_center, self.stats = depth, face, P, pixel_center, stats or {}

    def silhouette(self):
        """bool [V,H,W]: the pixels some face was drawn into"""
        return self.face >= 0


def camera_centers(P):
    """C_v = -inv(P_v[:3,:3]) @ P_v[:3,3] -> fp64 numpy [V,3]"""
    P = np.asarray(P, dtype=np.float64)
    C = np.empty((len(P), 3))
    for v in range(len(P)):
        C[v] = -np.linalg.inv(P[v, :3, :3]) @ P[v, :3, 3]
    return C


def _cameras(P, cams, what):
    if (P is None) == (cams is None):
        raise ValueError('%s: give either P [V, 4, 4] or cams [V, 2, 4, 4]' % what)
    if cams is not None:
        cams = np.asarray(cams.cpu() if isinstance(cams, torch.Tensor) else cams, dtype=np.float64)
        if cams.ndim != 4 or cams.shape[1:] != (2, 4, 4):
            raise ValueError('%s: cams must be [V, 2, 4, 4], got shape %s' % (what, cams.shape))
        if not np.isfinite(cams).all():
            raise ValueError('%s: a camera entry is NaN or infinite' % what)
        from .fusion import projection_matrices
        try:
            P = projection_matrices(cams)[0]
        except np.linalg.LinAlgError as e:
            raise ValueError('%s: a camera has a singular projection' % what) from e
    P = np.ascontiguousarray(np.asarray(P.cpu() if isinstance(P, torch.Tensor) else P, dtype=np.float64))
    if P.ndim != 3 or P.shape[1:] != (4, 4) or not 1 <= len(P) <= MAX_VIEWS:
        raise ValueError('%s: P must be [V, 4, 4] with 1 <= V <= %d, got shape %s' % (what, MAX_VIEWS, P.shape))
    if not np.isfinite(P).all():
        raise ValueError('%s: a camera entry is NaN or infinite' % what)
    return P


def _hw(hw, what):
    try:
        H, W = (int(x) for x in hw)
    except (TypeError, ValueError):
        raise ValueError('%s: hw must be (H, W), got %r' % (what, hw)) from None
    if H < 2 or W < 2 or H * W > INT32_MAX:
        raise ValueError('%s: images must be at least 2 x 2 (and H * W < 2^31), got %d x %d' % (what, H, W))
    return H, W


def _center(o, what):
    o = float(o)
    if o not in (0.5, 0.0):
        raise ValueError('%s: pixel_center must be 0.5 or 0.0, got %r' % (what, o))
    return o


def _count(name, x, lo, what):
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) or x < lo:
        raise ValueError('%s: %s must be an int >= %d, got %r' % (what, name, lo, x))
    return int(x)


def _mesh(mesh, what, faces=True):
    if not isinstance(mesh, Mesh):
        raise ValueError('%s: a mvsdf_amd.mesh.Mesh is needed, got %s' % (what, type(mesh).__name__))
    v, f, n = mesh.vertices, mesh.faces, mesh.normals
    if v.dim() != 2 or v.shape[1] != 3 or v.dtype != torch.float32:
        raise ValueError('%s: vertices must be float32 [Nv, 3], got %s %s' % (what, v.dtype, tuple(v.shape)))
    if f.dim() != 2 or f.shape[1] != 3 or f.dtype != torch.int32:
        raise ValueError('%s: faces must be int32 [Nf, 3], got %s %s' % (what, f.dtype, tuple(f.shape)))
    if n.shape != v.shape or n.dtype != torch.float32:
        raise ValueError('%s: normals must be float32 [Nv, 3] like the vertices, got %s %s' % (what, n.dtype, tuple(n.shape)))
    if v.shape[0] > INT32_MAX or f.shape[0] > INT32_MAX:
        raise ValueError('%s: %d vertices / %d faces (at most 2^31 - 1 each)' % (what, v.shape[0], f.shape[0]))
    if faces and f.numel() and (int(f.min()) < 0 or int(f.max()) >= v.shape[0]):
        raise ValueError('%s: a face index is outside [0, %d)' % (what, v.shape[0]))


def _on_device(mesh, what):
    if not mesh.vertices.is_cuda:
        raise MvsdfError('%s runs on the GPU: move the mesh there first (Mesh.to("cuda"))' % what)
    return mesh.vertices.device


def _masks(masks, V, H, W, what):
    if masks is None:
        return None
    m = torch.as_tensor(masks)
    if tuple(m.shape) != (V, H, W) or m.dtype not in (torch.uint8, torch.bool):
        raise ValueError('%s: masks must be uint8 or bool [V, H, W] = %s, got %s %s' % (what, (V, H, W), m.dtype, tuple(m.shape)))
    return m


def _tol(name, x, what):
    x = float(x)
    if not np.isfinite(x):
        raise ValueError('%s: %s must be finite, got %r' % (what, name, x))
    return x


# the error bits of a raster call (csrc/raster.hip), in the order they are looked at
ERRORS = [(K.MVSDF_RA_ERR_FINITE, ValueError, 'a camera entry is NaN or infinite'),
          (K.MVSDF_RA_ERR_INDEX, ValueError, 'a face index is outside the vertices')]


def rasterize(mesh, P=None, cams=None, hw=None, pixel_center=0.5, large_face_pixels=None, view_chunk=None, pretest=True, stats=False):
    """The module's rasterisation of `mesh` (device tensors, world coordinates) into V cameras of hw = (H, W) pixels -> Raster.
    large_face_pixels: faces whose clamped pixel box holds more pixels are drawn by a wave each instead of a lane (None: LARGE_FACE_PIXELS; the
    result does not depend on it).  view_chunk: views drawn at once; the key buffer holds 8 bytes per pixel of a chunk (None: as many as fit 1 GiB
    of keys and 2^26 (face, view) pairs).  pretest=False issues every atomic; stats=True counts atomics and covered pixels (both for measuring)."""
    what = 'rasterize'
    _mesh(mesh, what)
    P = _cameras(P, cams, what)
    if hw is None:
        raise ValueError('%s: hw = (H, W) is needed' % what)
    H, W = _hw(hw, what)
    o = _center(pixel_center, what)
    large = LARGE_FACE_PIXELS if large_face_pixels is None else _count('large_face_pixels', large_face_pixels, 0, what)
    V, nv, nf = len(P), mesh.vertices.shape[0], mesh.faces.shape[0]
    if view_chunk is None:
        vc = max(1, min(V, KEY_BUDGET_PIXELS // (H * W), ITEM_BUDGET // max(nf, 1)))
    else:
        vc = min(V, _count('view_chunk', view_chunk, 1, what))
    dev = _on_device(mesh, what)
    size = lib().mvsdf_raster_workspace_bytes(nv, nf, vc, H, W)
    if size == 0:
        raise ValueError('%s: %d faces in %d views of %d x %d at once are beyond the limits (faces * views < 2^31): lower view_chunk' % (what, nf, vc, H, W))
    depth = torch.empty(V, H, W, dtype=torch.float32, device=dev)
    face = torch.empty(V, H, W, dtype=torch.int32, device=dev)
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    Pd = torch.from_numpy(P).to(dev)
    v, f = mesh.vertices.contiguous(), mesh.faces.contiguous()
    st = _stream(v)
    flags = (0 if pretest else 1) | (2 if stats else 0)
    totals = {'large_items': 0, 'atomics': 0, 'covered': 0}
    for v0 in range(0, V, vc):
        n = min(vc, V - v0)
        check(lib().mvsdf_raster_draw(_vp(v), _vp(f), nv, nf, _vp(Pd[v0:]), n, H, W, o, large, flags, _vp(ws), size, st), 'mvsdf_raster_draw')
        check(lib().mvsdf_raster_resolve(n, H, W, _vp(ws), size, _vp(depth[v0:]), _vp(face[v0:]), st), 'mvsdf_raster_resolve')
        err, items, atomics, covered = _header(ws, K.MVSDF_RA_H_WORDS)                   # one wait per chunk: the next draw reuses the workspace
        raise_for_bits(err, what, ERRORS)
        totals['large_items'] += items
        totals['atomics'] += atomics
        totals['covered'] += covered
    return Raster(depth, face, P, o, totals)


def _view_inputs(mesh, raster, masks, depth_tol, what):
    _mesh(mesh, what, faces=False)
    if not isinstance(raster, Raster):
        raise ValueError('%s: a Raster (rasterize) is needed, got %s' % (what, type(raster).__name__))
    V, H, W = raster.depth.shape
    m = _masks(masks, V, H, W, what)
    tol = _tol('depth_tol', depth_tol, what)
    dev = _on_device(mesh, what)
    if m is not None:
        m = m.to(dev).contiguous().view(torch.uint8)
    return V, H, W, m, tol, dev


def vertex_visibility(mesh, raster, masks=None, depth_tol=0.01):
    """uint8 [V, Nv] on the device: the module's visibility of every vertex of `mesh` in every view of `raster` (its cameras and pixel_center),
    optionally also inside masks uint8 / bool [V,H,W]."""
    what = 'vertex_visibility'
    V, H, W, m, tol, dev = _view_inputs(mesh, raster, masks, depth_tol, what)
    nv = mesh.vertices.shape[0]
    v = mesh.vertices.contiguous()
    Pd = torch.from_numpy(raster.P).to(dev)
    ws = torch.empty(256, dtype=torch.uint8, device=dev)
    vis = torch.empty(V, nv, dtype=torch.uint8, device=dev)
    check(lib().mvsdf_raster_visibility(_vp(v), nv, _vp(Pd), V, H, W, raster.pixel_center, _vp(raster.depth.contiguous()), _vp(m), tol, _vp(ws), 256,
                                        _vp(vis), _stream(v)), 'mvsdf_raster_visibility')
    raise_for_bits(_header(ws, K.MVSDF_RA_H_WORDS)[K.MVSDF_RA_H_ERR], what, ERRORS)
    return vis


def color_vertices(mesh, images, P=None, cams=None, pixel_center=0.5, masks=None, depth_tol=0.01, cos_min=0.0, ignore_normals=False,
                   fallback=(0.5, 0.5, 0.5), raster=None, large_face_pixels=None, view_chunk=None):
    """A new Mesh with the vertices, faces and normals of `mesh` and vertex_colors taken from images uint8 [V,H,W,3] by the module's definition;
    its attribute n_views (int32 [Nv]) counts the views behind each colour.  The mesh is drawn into the cameras first (rasterize with
    large_face_pixels / view_chunk) unless `raster` holds that already."""
    what = 'color_vertices'
    _mesh(mesh, what)
    img = torch.as_tensor(images)
    if img.dim() != 4 or img.shape[3] != 3 or img.dtype != torch.uint8:
        raise ValueError('%s: images must be uint8 [V, H, W, 3], got %s %s' % (what, img.dtype, tuple(img.shape)))
    V, H, W = img.shape[:3]
    H, W = _hw((H, W), what)
    if raster is None:
        Pm = _cameras(P, cams, what)
        o = _center(pixel_center, what)
    else:
        if not isinstance(raster, Raster):
            raise ValueError('%s: raster must be a Raster, got %s' % (what, type(raster).__name__))
        Pm, o = raster.P, raster.pixel_center
        if tuple(raster.depth.shape) != (V, H, W):
            raise ValueError('%s: the raster is %s, the images %s' % (what, tuple(raster.depth.shape), (V, H, W)))
    if len(Pm) != V:
        raise ValueError('%s: %d cameras for %d images' % (what, len(Pm), V))
    m = _masks(masks, V, H, W, what)
    tol, cmin = _tol('depth_tol', depth_tol, what), _tol('cos_min', cos_min, what)
    fb = np.asarray(fallback, dtype=np.float32)
    if fb.shape != (3,) or not np.isfinite(fb).all():
        raise ValueError('%s: fallback must be three finite numbers, got %r' % (what, fallback))
    try:
        C = camera_centers(Pm)
    except np.linalg.LinAlgError as e:
        raise ValueError('%s: a camera has a singular projection' % what) from e
    if not np.isfinite(C).all():
        raise ValueError('%s: a camera centre is NaN or infinite' % what)
    dev = _on_device(mesh, what)
    if raster is None:
        raster = rasterize(mesh, P=Pm, hw=(H, W), pixel_center=o, large_face_pixels=large_face_pixels, view_chunk=view_chunk)
    img = img.to(dev).contiguous()
    if m is not None:
        m = m.to(dev).contiguous().view(torch.uint8)
    nv = mesh.vertices.shape[0]
    v, n = mesh.vertices.contiguous(), mesh.normals.to(dev).contiguous()
    Pd, Cd = torch.from_numpy(Pm).to(dev), torch.from_numpy(C).to(dev)
    ws = torch.empty(256, dtype=torch.uint8, device=dev)
    colors = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    n_views = torch.empty(nv, dtype=torch.int32, device=dev)
    check(lib().mvsdf_raster_colors(_vp(v), _vp(n), nv, _vp(Pd), _vp(Cd), V, H, W, o, _vp(raster.depth.contiguous()), _vp(m), _vp(img), tol, cmin,
                                    1 if ignore_normals else 0, float(fb[0]), float(fb[1]), float(fb[2]), _vp(ws), 256, _vp(colors), _vp(n_views),
                                    _stream(v)), 'mvsdf_raster_colors')
    raise_for_bits(_header(ws, K.MVSDF_RA_H_WORDS)[K.MVSDF_RA_H_ERR], what, ERRORS)
    out = Mesh(mesh.vertices, mesh.faces, mesh.normals, colors)
    out.n_views = n_views
    out.raster = raster
    return out


def scene_views(data_dir, masks=True):
    """What colouring and rendering need of a scene directory (datasets/scene_dataset.py's layout): (P fp64 [V,4,4] = cameras_hd.npz's world_mat_i,
    images uint8 [V,H,W,3] from image_hd/, masks bool [V,H,W] from mask_hd/ or None), numpy, the files sorted by name.  pixel_center is 0.0 for
    these cameras."""
    import os
    from PIL import Image
    from .utils import io as sio
    paths = sorted(sio.glob_imgs(os.path.join(data_dir, 'image_hd')))
    if not paths:
        raise ValueError('scene_views: no images under %s/image_hd' % data_dir)
    images = []
    for p in paths:
        with Image.open(p) as im:
            images.append(np.asarray(im.convert('RGB'), dtype=np.uint8))
    if len({a.shape for a in images}) != 1:
        raise ValueError('scene_views: the images under %s/image_hd differ in size' % data_dir)
    images = np.stack(images)
    cam = np.load(os.path.join(data_dir, 'cameras_hd.npz'))
    P = np.stack([cam['world_mat_%d' % i].astype(np.float64) for i in range(len(paths))])
    m = None
    if masks:
        mpaths = sorted(sio.glob_imgs(os.path.join(data_dir, 'mask_hd')))
        if len(mpaths) != len(paths):
            raise ValueError('scene_views: %d masks under %s/mask_hd for %d images' % (len(mpaths), data_dir, len(paths)))
        m = np.stack([sio.load_mask(p) for p in mpaths])
        if m.shape != images.shape[:3]:
            raise ValueError('scene_views: masks of %s for images of %s' % (m.shape[1:], images.shape[1:3]))
    return P, images, m


def color_mesh_from_scene(mesh, data_dir, masks=True, **kw):
    """color_vertices of a world-coordinate mesh from a scene directory's image_hd/, cameras_hd.npz and (masks=True) mask_hd/ -> the coloured Mesh"""
    P, images, m = scene_views(data_dir, masks)
    return color_vertices(mesh, images, P=P, pixel_center=0.0, masks=m, **kw)
