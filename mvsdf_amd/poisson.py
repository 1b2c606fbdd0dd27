"""Poisson surface reconstruction of an oriented point cloud on the device: the indicator-like function chi whose gradient best matches the splatted
normal field, solved on a regular grid by multigrid and meshed by mesh.marching_cubes_masked.  The classical method (Kazhdan, Bolitho and Hoppe 2006)
without its octree and without a screening term; there is no reference code for it, so this doc fixes the algorithm, tests/poisson_ref.py restates it
in numpy and the device is held to that restatement bit for bit.  Kernels: csrc/poisson.hip (the design: DESIGN.md).

Inputs: points and normals [n,3] (fp64; fp32 is promoted exactly), origin fp64 [3], voxel h > 0, depth in [2, 10], cycles >= 0, sweeps >= 1.  The grid
is a cube of N = 2^depth + 1 lattice points per axis, p_a = origin_a + idx_a * h as in tsdf.py; its outer layer is the Dirichlet boundary chi = 0.

The definition (fp64 throughout, in the order written, no FMA contraction):

1. Admission.  g = (p - origin) / h, i0 = floor(g), f = g - i0 per axis.  A point takes part iff 1 <= i0_a <= N - 3 on every axis (its 8 corners are
   interior lattice points); the others are counted in n_outside and ignored.  A non-finite coordinate or normal raises ValueError.  A zero normal is
   legal: it adds density and takes part in the isovalue and adds nothing to the field.
2. Splat.  For the 8 corners (dx, dy, dz), dx slowest, the weight is w = ((dx ? fx : 1 - fx) * (dy ? fy : 1 - fy)) * (dz ? fz : 1 - fz).  The integers
   int64(rint((w * n_a) * 2^32)), a = 0..2, and int64(rint(w * 2^32)) are added (64-bit integer atomics: the sums do not depend on the schedule) into
   four int64 volumes V_x, V_y, V_z and density at (i0 + d).  Their values times 2^-32 are the fp64 field and density.  (|n_a| < 2^30.)
3. Right-hand side.  At interior points b = (((V_x[i+1] - V_x[i-1]) + (V_y[j+1] - V_y[j-1])) + (V_z[k+1] - V_z[k-1])) / (2 h); b = 0 on the boundary.
4. Solve Laplace(chi) = b from chi = 0 by `cycles` V-cycles of stencil passes.  One cycle at a level with N > 3 and spacing h:
   - `sweeps` red-black Gauss-Seidel sweeps, colour (i + j + k) & 1 = 0 then 1, the update at an interior point being
     x = ((((((x[i-1] + x[i+1]) + x[j-1]) + x[j+1]) + x[k-1]) + x[k+1]) - (h*h) * b) / 6.0;
   - the residual r = b - (S - 6.0 * x) / (h*h) with S the same neighbour sum;
   - full weighting of r to the coarse level's right-hand side, separably: per axis (0.25 * a[2I-1] + 0.5 * a[2I]) + 0.25 * a[2I+1], along z, then
     y, then x; the coarse boundary is 0;
   - the cycle of the coarse level (spacing 2 h) from x = 0;
   - trilinear prolongation of the coarse x, separably along x, then y, then z (an even index copies, an odd index 2I + 1 takes
     0.5 * (a[I] + a[I+1])), added to x;
   - `sweeps` sweeps again.
   The 3^3 level is solved directly: x = -((h*h) * b) / 6.0 at its one interior point.
5. Isovalue.  c_i = chi interpolated trilinearly at every admitted point, the 8 terms w * chi added one by one from 0.0 in the splat's corner order
   (Field.values, in input order).  iso = T / n_used, T the sum of the c_i over the canonical pairwise tree: pad with +0.0 to a power-of-two length
   and add adjacent pairs, a = a[0::2] + a[1::2], until one value is left.  (No point admitted: iso = NaN and nothing is meshed.)
6. Diagnostics.  residual0 and residual are the largest |r| at the finest level before the first and after the last cycle.
7. Trim and mesh.  valid0 = density > min_density; valid = valid0 dilated `dilate` times over the 6-neighbourhood inside the grid.  Field.mesh() is
   mesh.marching_cubes_masked(fp32(chi - iso), valid, 0.0, spacing (h, h, h), origin).  With outward normals chi grows outwards, so the faces'
   right-hand normals point outwards as for the SDF meshes.  trim=False meshes under an all-true mask: the watertight surface.

Without dilation the cells that cross the surface lack corners (a lattice point gets density only from the samples of its own 8 cells) and the mesh
is full of holes; one step closes a densely sampled sphere while an open surface stays open at its rim instead of growing a cap (tests/
test_poisson_host.py).  Not built: the screening term, an adaptive octree, normals for clouds that come without cameras (fusion.depth_normals makes
them from depth maps), colour (raster.color_vertices), fusing the coarse levels into one launch (every pass of every level is a launch of its own).
"""
import numpy as np
import torch

from . import mesh as _mesh
from ._lib import check, f64_from_bits, K, lib, raise_for_bits, _header, _stream, _vp

MIN_DEPTH, MAX_DEPTH = K.MVSDF_PO_MIN_DEPTH, K.MVSDF_PO_MAX_DEPTH
INT32_MAX = 2 ** 31 - 1
STAGE_SPLAT, STAGE_SOLVE, STAGE_ISO = 1, 2, 4


def _int(name, x, what):
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
        raise ValueError('%s: %s must be an int, got %r' % (what, name, x))
    return int(x)


def _depth(depth, what):
    depth = _int('depth', depth, what)
    if not MIN_DEPTH <= depth <= MAX_DEPTH:
        raise ValueError('%s: depth must be in [%d, %d], got %d' % (what, MIN_DEPTH, MAX_DEPTH, depth))
    return depth


# the error bits of a poisson call (csrc/poisson.hip), in the order they are looked at
ERRORS = [(K.MVSDF_PO_ERR_FINITE, ValueError, 'a coordinate, a normal, the origin or the voxel is NaN or infinite'),
          (K.MVSDF_PO_ERR_RANGE, ValueError, 'depth must be in [2, 10], cycles >= 0, sweeps >= 1, voxel > 0'),
          (K.MVSDF_PO_ERR_SHAPE, ValueError, 'between 1 and 2^31 - 1 points')]


class Field:
    """The result of reconstruct: chi fp64 [N,N,N], density fp64 [N,N,N], values fp64 [n_used] (the c_i), all on the device; iso, residual0, residual
    (floats), n_used, n_outside (ints); origin (fp64 numpy [3]), voxel, depth as they were used."""

    def __init__(self, chi, density, values, iso, n_used, n_outside, residual0, residual, origin, voxel, depth):
        self.chi, self.density, self.values, self.iso = chi, density, values, iso
        self.n_used, self.n_outside, self.residual0, self.residual = n_used, n_outside, residual0, residual
        self.origin, self.voxel, self.depth = origin, voxel, depth

    def valid(self, min_density=0.0, dilate=1):
        """step 7's mask -> bool [N,N,N] on the device"""
        what = 'Field.valid'
        min_density = float(min_density)
        dilate = _int('dilate', dilate, what)
        if np.isnan(min_density) or dilate < 0:
            raise ValueError('%s: min_density must be a number and dilate >= 0, got %r, %r' % (what, min_density, dilate))
        d = self.density
        out = torch.empty(d.shape, dtype=torch.bool, device=d.device)
        tmp = torch.empty(d.shape, dtype=torch.bool, device=d.device) if dilate else None
        check(lib().mvsdf_poisson_valid(_vp(d), self.depth, min_density, dilate, _vp(tmp), _vp(out), _stream(d)), 'mvsdf_poisson_valid')
        return out

    def volume(self):
        """fp32(chi - iso) [N,N,N] on the device: the volume whose level set 0 is the surface"""
        out = torch.empty(self.chi.shape, dtype=torch.float32, device=self.chi.device)
        check(lib().mvsdf_poisson_volume(_vp(self.chi), self.chi.numel(), float(self.iso), _vp(out), _stream(self.chi)), 'mvsdf_poisson_volume')
        return out

    def mesh(self, min_density=0.0, dilate=1, trim=True):
        """step 7 -> Mesh, or None when no point was admitted or nothing crosses the isovalue"""
        if self.n_used == 0:
            return None
        ok = self.valid(min_density, dilate) if trim else torch.ones(self.chi.shape, dtype=torch.bool, device=self.chi.device)
        return _mesh.marching_cubes_masked(self.volume(), ok, 0.0, spacing=(self.voxel,) * 3, origin=tuple(self.origin))


def _cloud(points, normals, what):
    """-> (points, normals) as torch tensors [n,3] of a floating dtype, wherever they live; everything checked without a device"""
    out = []
    for name, a in (('points', points), ('normals', normals)):
        t = torch.as_tensor(a)
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError('%s: %s must be [n, 3], got shape %s' % (what, name, tuple(t.shape)))
        if t.dtype not in (torch.float32, torch.float64):
            raise ValueError('%s: %s must be float32 or float64, got %s' % (what, name, t.dtype))
        out.append(t)
    if out[0].shape[0] != out[1].shape[0]:
        raise ValueError('%s: %d points but %d normals' % (what, out[0].shape[0], out[1].shape[0]))
    if not 1 <= out[0].shape[0] <= INT32_MAX:
        raise ValueError('%s: between 1 and 2^31 - 1 points, got %d' % (what, out[0].shape[0]))
    return out


def _origin(origin, voxel, what):
    org = np.asarray(origin.cpu() if isinstance(origin, torch.Tensor) else origin, dtype=np.float64)
    if org.shape != (3,):
        raise ValueError('%s: origin must be [3], got shape %s' % (what, org.shape))
    h = float(voxel)
    if not (np.isfinite(org).all() and np.isfinite(h)):
        raise ValueError('%s: the origin or the voxel is NaN or infinite' % what)
    if not h > 0:
        raise ValueError('%s: voxel must be > 0, got %r' % (what, h))
    return np.ascontiguousarray(org), h


class _Call:
    """the validated arguments and the device buffers of one reconstruction; run(stages) launches, finish() reads the header (tools/time_poisson.py
    times the stages apart)"""

    def __init__(self, points, normals, origin, voxel, depth, cycles, sweeps, what):
        p, nrm = _cloud(points, normals, what)
        self.org, self.h = _origin(origin, voxel, what)
        self.depth = _depth(depth, what)
        self.cycles, self.sweeps = _int('cycles', cycles, what), _int('sweeps', sweeps, what)
        if self.cycles < 0 or self.sweeps < 1:
            raise ValueError('%s: cycles must be >= 0 and sweeps >= 1, got %d, %d' % (what, self.cycles, self.sweeps))
        self.what = what
        self.n = p.shape[0]
        dev = p.device if p.is_cuda else (nrm.device if nrm.is_cuda else torch.device('cuda'))
        self.p = p.to(dev, torch.float64).contiguous()
        self.nrm = nrm.to(dev, torch.float64).contiguous()
        N = 2 ** self.depth + 1
        self.size = lib().mvsdf_poisson_workspace_bytes(self.n, self.depth)
        if self.size == 0:
            raise ValueError('%s: %d points at depth %d are beyond the limits' % (what, self.n, self.depth))
        self.ws = torch.empty(self.size, dtype=torch.uint8, device=dev)
        self.chi = torch.empty(N, N, N, dtype=torch.float64, device=dev)
        self.density = torch.empty(N, N, N, dtype=torch.float64, device=dev)
        self.values = torch.empty(self.n, dtype=torch.float64, device=dev)

    def run(self, stages=STAGE_SPLAT | STAGE_SOLVE | STAGE_ISO):
        check(lib().mvsdf_poisson_reconstruct(_vp(self.p), _vp(self.nrm), self.n, self.org.ctypes.data, self.h, self.depth, self.cycles, self.sweeps, stages,
                                              _vp(self.ws), self.size, _vp(self.chi), _vp(self.density), _vp(self.values), _stream(self.p)),
              'mvsdf_poisson_reconstruct')

    def finish(self):
        n_used, err, t, r0, r1 = _header(self.ws, K.MVSDF_PO_H_WORDS)                     # the one wait of the call
        raise_for_bits(err, self.what, ERRORS)
        iso = f64_from_bits(t) / n_used if n_used else float('nan')
        return Field(self.chi, self.density, self.values[:n_used], iso, n_used, self.n - n_used, f64_from_bits(r0), f64_from_bits(r1), self.org.copy(),
                     self.h, self.depth)


def reconstruct(points, normals, origin, voxel, depth, cycles=8, sweeps=2):
    """The module's definition -> Field.  Device tensors are used where they are (the stream is theirs); numpy / CPU input is copied to the GPU.
    Every argument is checked before the device is touched."""
    call = _Call(points, normals, origin, voxel, depth, cycles, sweeps, 'reconstruct')
    call.run()
    return call.finish()


def poisson_grid(lo, hi, depth, scale=1.1):
    """The cube of 2^depth cells per axis centred on the box [lo, hi] with edge = scale * the box's longest edge -> (origin fp64 numpy [3], voxel):
    voxel = edge / 2^depth, origin = (lo + hi) / 2 - edge / 2.  scale >= 1.  The box's outermost points are admitted iff the margin
    (scale - 1) / scale * 2^(depth - 1) is above one cell: from depth 5 on at the default 1.1, scale 1.3 at depth 4."""
    what = 'poisson_grid'
    lo = np.asarray(lo.cpu() if isinstance(lo, torch.Tensor) else lo, dtype=np.float64)
    hi = np.asarray(hi.cpu() if isinstance(hi, torch.Tensor) else hi, dtype=np.float64)
    if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all()) or (hi < lo).any():
        raise ValueError('%s: lo and hi must be finite [3] with lo <= hi, got %r, %r' % (what, lo, hi))
    depth = _depth(depth, what)
    scale = float(scale)
    if not (np.isfinite(scale) and scale >= 1):
        raise ValueError('%s: scale must be finite and >= 1, got %r' % (what, scale))
    edge = scale * float((hi - lo).max())
    if not (np.isfinite(edge) and edge > 0):
        raise ValueError('%s: the box must have an extent' % what)
    return (lo + hi) / 2 - edge / 2, edge / 2 ** depth


def poisson_mesh(points, normals, depth=8, scale=1.1, largest=False, cycles=8, sweeps=2, min_density=0.0, dilate=1, trim=True):
    """poisson_grid over the cloud's bounding box, reconstruct, Field.mesh() and, with largest=True, Mesh.largest_component() -> (Mesh or None, Field)"""
    what = 'poisson_mesh'
    p, nrm = _cloud(points, normals, what)
    depth = _depth(depth, what)
    if not bool(torch.isfinite(p).all()):
        raise ValueError('%s: a coordinate is NaN or infinite' % what)
    origin, h = poisson_grid(p.amin(0).double().cpu().numpy(), p.amax(0).double().cpu().numpy(), depth, scale)
    field = reconstruct(p, nrm, origin, h, depth, cycles=cycles, sweeps=sweeps)
    m = field.mesh(min_density=min_density, dilate=dilate, trim=trim)
    if m is not None and largest:
        m = m.largest_component()
    return m, field
