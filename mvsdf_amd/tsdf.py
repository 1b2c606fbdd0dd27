"""TSDF fusion on the device: depth maps (the natural input: fuse_depths' fused_depths) integrated into a voxel grid of truncated signed distances,
and a mesh from it seconds later (mesh.marching_cubes_masked skips the cells nothing observed).  The classical volumetric method (Curless and
Levoy 1996) with unit weights; there is no reference code for it, so this doc fixes the algorithm, tests/tsdf_ref.py restates it in numpy and the
device is held to that restatement bit for bit.  Kernels: csrc/tsdf.hip (the design: DESIGN.md).

Inputs: cams fp64 [V,2,4,4] as utils.io.load_cam returns them, depths fp32 [V,H,W] (a texel that is <= 0 or not finite is a hole), origin fp64 [3],
voxel h > 0, dims (Nx, Ny, Nz) each >= 2, trunc > 0 (default 4 h), jump >= 0 (default trunc; inf switches the rule off), min_views >= 1, views a
list of view indices (default every view in ascending order; a view listed twice counts twice).

The definition (fp64 throughout, in the order written, no FMA contraction; fp32 depths are promoted exactly):

- Matrices and pixel convention are fusion.py's: P_v = K4_v @ E_v (fusion.projection_matrices), a row times (p, 1) is
  ((t0*p0 + t1*p1) + t2*p2) + t3*1, and pixel (x, y) sits at image coordinate (x + 0.5, y + 0.5).
- The lattice point (i, j, k) is p_a = origin_a + (double)idx_a * h.
- Per lattice point start with D = 0, n = 0 and visit the views in order:
  1. z = row2 . (p, 1); skip the view unless z > 0.
  2. u = row0 . (p, 1) / z - 0.5, v = row1 . (p, 1) / z - 0.5; skip unless 0 <= u <= W-1 and 0 <= v <= H-1.
  3. x0 = min(floor(u), W-2), y0 = min(floor(v), H-2), fx = u - x0, fy = v - y0; the four texels d00 d01 / d10 d11 of the view's depth map at rows
     y0, y0+1 and columns x0, x0+1.  Skip unless all four hold a depth (a hole never bleeds into a distance); skip if max - min of the four is
     > jump (a surface is not interpolated across a depth edge).
  4. ds = (d00*(1-fx) + d01*fx)*(1-fy) + (d10*(1-fx) + d11*fx)*fy; s = ds - z (positive in front of the surface); skip if s < -trunc.
  5. D += min(s / trunc, 1.0); n += 1.
- weight = n; tsdf = fp32(D / n) if n >= min_views else 1.0f; valid = n >= min_views.

The distance is the projective one along the camera's z axis, every sample weighs 1, and space in front of a surface is carved to +1 however far in
front.  Not built: colour in the volume (Volume.mesh() gives geometry; raster.color_vertices colours it from the images), per-pixel confidence
weights, sparse allocation (the grid is dense: 9 bytes per lattice point).
"""
import numpy as np
import torch

from . import mesh as _mesh
from ._lib import check, K, lib, raise_for_bits, _header, _stream, _vp
from .fusion import projection_matrices

INT32_MAX = 2 ** 31 - 1


class Volume:
    """The result of integrate_depths: tsdf fp32 [Nx,Ny,Nz], weight int32 [Nx,Ny,Nz] (the samples taken), valid bool [Nx,Ny,Nz] (weight >=
    min_views), all on the device; origin (fp64 numpy [3]), voxel, dims, trunc, jump, min_views as they were used."""

    def __init__(self, tsdf, weight, valid, origin, voxel, dims, trunc, jump, min_views):
        self.tsdf, self.weight, self.valid = tsdf, weight, valid
        self.origin, self.voxel, self.dims, self.trunc, self.jump, self.min_views = origin, voxel, dims, trunc, jump, min_views

    def valid_share(self):
        """the share of valid lattice points"""
        return float(self.valid.sum()) / self.valid.numel()

    def mesh(self):
        """the level set 0 over the cells whose 8 corners are valid (mesh.marching_cubes_masked, spacing h, the grid's origin) -> Mesh or None"""
        return _mesh.marching_cubes_masked(self.tsdf, self.valid, 0.0, spacing=(self.voxel,) * 3, origin=tuple(self.origin))


# the error bits of a tsdf call (csrc/tsdf.hip), in the order they are looked at
ERRORS = [(K.MVSDF_TS_ERR_FINITE, ValueError, 'a camera entry, the origin, voxel or trunc is NaN or infinite (or jump is NaN)'),
          (K.MVSDF_TS_ERR_VIEW, ValueError, 'a view index is outside [0, V)'),
          (K.MVSDF_TS_ERR_RANGE, ValueError, 'voxel and trunc must be > 0, jump >= 0, min_views >= 1'),
          (K.MVSDF_TS_ERR_SHAPE, ValueError, 'shapes disagree or are out of range (V >= 1, H and W >= 2, every dim >= 2, at least one view)')]


def _int(name, x, what):
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
        raise ValueError('%s: %s must be an int, got %r' % (what, name, x))
    return int(x)


def _dims(dims, what):
    try:
        d = tuple(_int('dims', x, what) for x in dims)
    except TypeError:
        raise ValueError('%s: dims must be (Nx, Ny, Nz), got %r' % (what, dims)) from None
    if len(d) != 3 or min(d) < 2 or max(d) > INT32_MAX:
        raise ValueError('%s: dims must be three ints >= 2, got %r' % (what, dims))
    return d


def integrate_depths(cams, depths, origin, voxel, dims, trunc=None, jump=None, min_views=1, views=None):
    """The module's definition -> Volume.  Device tensors are used where they are (the stream is theirs); numpy / CPU input is copied to the GPU.
    Every argument is checked before the device is touched."""
    what = 'integrate_depths'
    d = torch.as_tensor(depths)
    if d.dim() != 3:
        raise ValueError('%s: depths must be [V, H, W], got shape %s' % (what, tuple(d.shape)))
    V, H, W = d.shape
    dev = d.device if d.is_cuda else torch.device('cuda')
    cams = np.asarray(cams.cpu() if isinstance(cams, torch.Tensor) else cams, dtype=np.float64)
    if cams.shape != (V, 2, 4, 4):
        raise ValueError('%s: cams must be [V, 2, 4, 4] for V = %d depth maps, got shape %s' % (what, V, cams.shape))
    if H < 2 or W < 2 or V < 1:
        raise ValueError('%s: depth maps must be at least 2 x 2 (and V >= 1), got %d views of %d x %d' % (what, V, H, W))
    org = np.asarray(origin.cpu() if isinstance(origin, torch.Tensor) else origin, dtype=np.float64)
    if org.shape != (3,):
        raise ValueError('%s: origin must be [3], got shape %s' % (what, org.shape))
    dims = _dims(dims, what)
    h = float(voxel)
    trunc = 4.0 * h if trunc is None else float(trunc)
    jump = trunc if jump is None else float(jump)
    min_views = _int('min_views', min_views, what)
    if not (np.isfinite(cams).all() and np.isfinite(org).all() and np.isfinite(h) and np.isfinite(trunc)) or np.isnan(jump):
        raise ValueError('%s: a camera entry, the origin, voxel or trunc is NaN or infinite (or jump is NaN)' % what)
    if not (h > 0 and trunc > 0 and jump >= 0 and 1 <= min_views <= INT32_MAX):
        raise ValueError('%s: voxel and trunc must be > 0, jump >= 0, min_views >= 1 (got %r, %r, %r, %r)' % (what, h, trunc, jump, min_views))
    vs = list(range(V)) if views is None else [_int('views', s, what) for s in views]
    if not vs:
        raise ValueError('%s: views is empty' % what)
    if any(s < 0 or s >= V for s in vs):
        raise ValueError('%s: a view index is outside [0, %d)' % (what, V))
    try:
        P, _ = projection_matrices(cams)
    except np.linalg.LinAlgError as e:
        raise ValueError('%s: a camera has a singular projection' % what) from e
    vs = np.asarray(vs, np.int32)
    mats = np.ascontiguousarray(P[vs].reshape(-1))
    dm = np.asarray(dims, np.int64)
    size = lib().mvsdf_tsdf_workspace_bytes(V, H, W, len(vs))
    if size == 0 or dims[0] * dims[1] * dims[2] > 2 ** 40:
        raise ValueError('%s: %d views of %d x %d into %r are beyond the limits (H*W < 2^31, at most 2^40 lattice points)' % (what, V, H, W, dims))
    d = d.to(dev, torch.float32).contiguous()
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    tsdf = torch.empty(dims, dtype=torch.float32, device=dev)
    weight = torch.empty(dims, dtype=torch.int32, device=dev)
    valid = torch.empty(dims, dtype=torch.bool, device=dev)
    check(lib().mvsdf_tsdf_integrate(_vp(d), V, H, W, mats.ctypes.data, vs.ctypes.data, len(vs), org.ctypes.data, h, dm.ctypes.data, trunc, jump,
                                     min_views, _vp(ws), size, _vp(tsdf), _vp(weight), _vp(valid), _stream(d)), 'mvsdf_tsdf_integrate')
    _, err = _header(ws, K.MVSDF_RES_H_WORDS)   # the one wait of the call; mats / vs / org / dm live until here
    raise_for_bits(err, what, ERRORS)
    return Volume(tsdf, weight, valid, org.copy(), h, dims, trunc, jump, min_views)


def grid_from_bbox(lo, hi, voxel=None, resolution=None, pad_voxels=2):
    """A lattice that covers the box [lo, hi] with pad_voxels voxels to spare on every side -> (origin fp64 numpy [3], voxel, dims).  Give exactly
    one of voxel (the edge h) and resolution (h = the box's longest edge / resolution, so that edge spans `resolution` cells before the padding).
    origin = lo - pad_voxels * h; dims_a = ceil((hi_a - lo_a) / h) + 1 + 2 * pad_voxels, so the last lattice point is at or beyond hi_a + pad."""
    what = 'grid_from_bbox'
    lo = np.asarray(lo.cpu() if isinstance(lo, torch.Tensor) else lo, dtype=np.float64)
    hi = np.asarray(hi.cpu() if isinstance(hi, torch.Tensor) else hi, dtype=np.float64)
    if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all()) or (hi < lo).any():
        raise ValueError('%s: lo and hi must be finite [3] with lo <= hi, got %r, %r' % (what, lo, hi))
    if (voxel is None) == (resolution is None):
        raise ValueError('%s: give either voxel or resolution' % what)
    pad = _int('pad_voxels', pad_voxels, what)
    if pad < 0:
        raise ValueError('%s: pad_voxels must be >= 0' % what)
    if resolution is not None:
        res = _int('resolution', resolution, what)
        if res < 1 or not (hi - lo).max() > 0:
            raise ValueError('%s: resolution must be >= 1 and the box must have an extent' % what)
        h = float((hi - lo).max()) / res
    else:
        h = float(voxel)
    if not (np.isfinite(h) and h > 0):
        raise ValueError('%s: the voxel must be finite and > 0, got %r' % (what, h))
    cells = np.ceil((hi - lo) / h)
    if cells.max() + 1 + 2 * pad > INT32_MAX:
        raise ValueError('%s: a voxel of %g gives more than 2^31 lattice points along an axis' % (what, h))
    dims = tuple(max(int(c) + 1 + 2 * pad, 2) for c in cells)
    return lo - pad * h, h, dims


def tsdf_mesh(cams, depths, origin, voxel, dims, trunc=None, jump=None, min_views=1, views=None, largest=False):
    """integrate_depths, Volume.mesh() and, with largest=True, Mesh.largest_component() -> (Mesh or None, Volume)"""
    vol = integrate_depths(cams, depths, origin, voxel, dims, trunc=trunc, jump=jump, min_views=min_views, views=views)
    m = vol.mesh()
    if m is not None and largest:
        m = m.largest_component()
    return m, vol
