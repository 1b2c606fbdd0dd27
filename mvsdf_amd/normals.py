"""Normals for unoriented point clouds on the device: which points are the k nearest of every point, the eigenproblem of each neighbourhood and a
globally consistent sign.  poisson.poisson_mesh needs an oriented cloud, and the only other producer of normals is fusion.depth_normals, which needs
this project's own fused depth maps; COLMAP's sparse points3D, a voxel-filtered cloud, a ground-truth scan, a lidar PLY or another system's MVS
points carry none.  Kernels: csrc/normals.hip (the design: DESIGN.md); tests/normals_ref.py restates every stage in numpy.  Open3D users know the
stages as estimate_normals + orient_normals_consistent_tangent_plane / orient_normals_towards_camera_location; Open3D is not a dependency and its
numerics are not claimed.  There is no reference code for this step; the definition below is this project's.

The definition.  Input: points fp64 [N,3], all finite.  fp64 throughout, in the order written, no FMA contraction; only + - * / sqrt.

1. knn_indices(points, k).  d2(i,j) = (dx*dx + dy*dy) + dz*dz, the formula of cloud.py.  Row i holds the k points j != i (by index: an exact
   duplicate of i is a neighbour at distance 0) that are smallest under the total order (d2(i,j), j), ascending in that order: ties go to the lower
   input index, so the result is one array, not a multiset.  1 <= k <= 32, k + 1 <= N <= 2^31 - 1.

2. estimate_normals(points, k).  Per point i, with j_1 .. j_k its row:
   - offsets u_0 = 0 and u_t = p_(j_t) - p_i (relative to the point, so coordinates of DTU's size lose nothing);
   - mean m = (((0 + u_1) + u_2) + ... + u_k) / (k + 1) per axis;
   - covariance C_ab = ((0 + (u_0 - m)_a * (u_0 - m)_b) + (u_1 - m)_a * (u_1 - m)_b) + ..., the six entries a <= b, mirrored into a full 3 x 3 A;
     V = the identity;
   - SWEEPS = 6 sweeps of cyclic Jacobi over the pairs (p,q) = (0,1), (0,2), (1,2) (five sweeps already leave every cloud of the test table unchanged
     by a further one).  A rotation whose A[p][q] is exactly 0 is skipped; otherwise, as registration.horn_rotation: theta = (A[q][q] - A[p][p]) /
     (2 * A[p][q]), t = (1 if theta >= 0 else -1) / (|theta| + sqrt(theta * theta + 1)), c = 1 / sqrt(t * t + 1), s = t * c; then for r = 0, 1, 2 the
     columns (A[r][p], A[r][q]) <- (c * xp - s * xq, s * xp + c * xq), then the rows (A[p][r], A[q][r]) likewise, then the columns of V likewise, then
     A[p][q] = A[q][p] = 0;
   - l_c = A[c][c]; the normal is column c of V for the smallest l_c (ties to the lower column), divided by sqrt((x*x + y*y) + z*z), and all three
     components negated iff the component of largest magnitude (ties to the lower axis) is < 0.  That sign is only a canonical form; stage 3 or 4
     gives it meaning;
   - variation = l_min / ((l_0 + l_1) + l_2), and 0 where that sum is 0: the surface-variation measure, a confidence and a trimming key.
   Exact duplicates, collinear points and isotropic lattices have no geometric normal; the definition still yields one bit pattern for them.

3. orient_normals(points, normals, neighbors, up, centers, visibility): the spanning-tree orientation of Hoppe et al. 1992, stated so that the answer
   is unique.
   - Graph: the undirected edges {i,j} with j in row i of neighbors or i in row j; an entry equal to its own row index is no edge.
   - Score a_ij = |(nx_i*nx_j + ny_i*ny_j) + nz_i*nz_j|; the edges are totally ordered by (a descending, min(i,j) ascending, max(i,j) ascending).
     The order is on |dot| itself: a non-negative double orders as its bits.
   - T = the spanning forest Kruskal's algorithm builds in that order; unique because the order is total.
   - Along a tree edge, j is flipped relative to i iff the signed dot of the input normals is < 0; a point's flip relative to the root of its tree
     is the parity of its tree path, whichever root is taken.  A flipped normal has all three components negated.
   - Component sign by up: the reference point of a component is the one with the largest (x*ux + y*uy) + z*uz (-0 equal to +0, ties to the lowest
     index); the component is signed so that this point's normal ends as it came in iff its (nx*ux + ny*uy) + nz*uz is >= 0, and negated iff it is < 0.
     Stated on the reference point's input normal, the rule needs no root: a product of exactly 0 (a zero normal, a zero up) keeps that point.
   - Component sign by views (centers fp64 [V,3] and visibility given): over the component's (point, seeing view) pairs, each pair once, count
     those with (nx*(cx - px) + ny*(cy - py)) + nz*(cz - pz) < 0 and those > 0 for the oriented normal; more negative than positive flips the
     component, fewer leaves it, a tie falls back to the up rule.  visibility: the uint8 / bool [V,N] mask, the CSR tracks (track_off int64 [N+1],
     track_view int32 [nnz]) (both through viewsel.pack_visibility) or an int32 [N] view index such as Fused.view.
   - labels_i = the smallest input index of i's component; n_components; rounds = the number of Boruvka rounds that choose at least one edge when
     every component takes its first outgoing edge of the order and all chosen edges are joined (a property of the graph, which the device's
     rounds reproduce).

4. orient_to_views(points, normals, centers, visibility): each normal is negated iff more of its own point's seeing views give a product < 0 than
   > 0 (the product of 3); a tie or a point nobody sees: unchanged.  The call for sparse COLMAP points, where each point carries its own track.

ValueError before any launch: a dtype other than float64 (nothing is converted silently), a shape other than [N,3] / [N,k] / [V,3], k outside 1 .. 32,
N < k + 1, a non-finite up, a visibility whose shape does not fit.  ValueError through the call's error bits: a non-finite coordinate, normal or
centre, a neighbour index outside [0, N), a view index outside [0, V).
"""
import numpy as np
import torch

from . import viewsel
from ._lib import check, lib, K, MvsdfError, raise_for_bits, _header, _stream, _vp
from .cloud import _device, _neighbors, _points

SWEEPS = 6


# the error bits of a normals call (csrc/normals.hip), in the order they are looked at
ERRORS = [(K.MVSDF_PC_ERR_FINITE, ValueError, 'a coordinate (or a view centre) is NaN or infinite'),
          (K.MVSDF_PC_ERR_NORMAL, ValueError, 'a normal is NaN or infinite'),
          (K.MVSDF_PC_ERR_INDEX, ValueError, 'a neighbour index is outside [0, N)'),
          (K.MVSDF_PC_ERR_ROUNDS, MvsdfError, 'the orientation loop reached its round limit')]


def _knn(points, k, what, want_d2, want_normals):
    p = _points(points, what)
    k = _neighbors(k, p.shape[0], what)
    p = _device(p)
    n, dev = p.shape[0], p.device
    size = lib().mvsdf_normals_knn_workspace_bytes(n)
    if size == 0:
        raise ValueError('%s: %d points (2 .. 2^31 - 1)' % (what, n))
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    idx = torch.empty(n, k, dtype=torch.int32, device=dev)
    d2 = torch.empty(n, k, dtype=torch.float64, device=dev) if want_d2 else None
    nrm = torch.empty(n, 3, dtype=torch.float64, device=dev) if want_normals else None
    var = torch.empty(n, dtype=torch.float64, device=dev) if want_normals else None
    check(lib().mvsdf_normals_knn(_vp(p), n, k, _vp(ws), size, _vp(idx), _vp(d2), _vp(nrm), _vp(var), _stream(p)), 'mvsdf_normals_knn')
    raise_for_bits(_header(ws, K.MVSDF_ERRW_H_WORDS)[K.MVSDF_ERRW_H_ERR], what, ERRORS)
    return idx, d2, nrm, var


def knn_indices(points, k, return_distances=False):
    """stage 1 -> neighbors int32 [N,k] on the device; with return_distances (neighbors, d2 fp64 [N,k])"""
    idx, d2, _, _ = _knn(points, k, 'knn_indices', return_distances, False)
    return (idx, d2) if return_distances else idx


def estimate_normals(points, k=16):
    """stages 1 and 2 -> (normals fp64 [N,3], variation fp64 [N], neighbors int32 [N,k]) on the device"""
    idx, _, nrm, var = _knn(points, k, 'estimate_normals', False, True)
    return nrm, var, idx


def _normals(x, n, what):
    t = _points(x, what)
    if t.shape[0] != n:
        raise ValueError('%s: normals must be [N, 3] for N = %d points, got shape %s' % (what, n, tuple(t.shape)))
    return t


def _centers(x, what):
    if not isinstance(x, (torch.Tensor, np.ndarray)):
        raise ValueError('%s: centers must be a numpy array or a torch tensor of dtype float64' % what)
    c = torch.as_tensor(x)
    if c.dtype != torch.float64 or c.dim() != 2 or c.shape[1] != 3:
        raise ValueError('%s: centers must be float64 [V, 3], got %s %s' % (what, c.dtype, tuple(c.shape)))
    if not 1 <= c.shape[0] <= viewsel.MAX_VIEWS:
        raise ValueError('%s: V must be in [1, %d], got %d' % (what, viewsel.MAX_VIEWS, c.shape[0]))
    return c


def _visibility(visibility, V, n, what):
    """every visibility form, its shape checked on the host -> one of the two forms viewsel.pack_visibility takes"""
    if visibility is None:
        raise ValueError('%s: centers need a visibility (a [V, N] mask, the tracks tuple or an int32 [N] view index)' % what)
    if not isinstance(visibility, tuple):
        vis = torch.as_tensor(visibility)
        if vis.dim() == 1:                                                   # one view per point: tracks of length 1
            if vis.shape[0] != n or vis.is_floating_point() or vis.dtype == torch.bool:
                raise ValueError('%s: a view index must be an integer [N] = [%d], got %s %s' % (what, n, vis.dtype, tuple(vis.shape)))
            visibility = (torch.arange(n + 1, dtype=torch.int64), vis)
        elif tuple(vis.shape) != (V, n) or vis.dtype not in (torch.uint8, torch.bool):
            raise ValueError('%s: visibility must be uint8 or bool [V, N] = %s, got %s %s' % (what, (V, n), vis.dtype, tuple(vis.shape)))
    elif len(visibility) != 2 or tuple(torch.as_tensor(visibility[0]).shape) != (n + 1,):
        raise ValueError('%s: tracks are the tuple (track_off int64 [N + 1] = [%d], track_view int32 [nnz])' % (what, n + 1))
    return visibility


def _pack(visibility, V, n, dev, what):
    """-> the bit matrix of viewsel.pack_visibility (its error bits checked)"""
    bits, hdr = viewsel.pack_visibility(visibility, V, n, dev)
    raise_for_bits(_header(hdr, K.MVSDF_RES_H_WORDS)[K.MVSDF_RES_H_ERR], what, viewsel.ERRORS)
    return bits


def _up(up, what):
    try:
        u = [float(x) for x in up]
    except (TypeError, ValueError):
        raise ValueError('%s: up must be three numbers, got %r' % (what, up)) from None
    if len(u) != 3 or not np.isfinite(u).all():
        raise ValueError('%s: up must be three finite numbers, got %r' % (what, up))
    return u


class Oriented:
    """The result of orient_normals: normals fp64 [N,3] and labels int32 [N] on the device, n_components and rounds (ints).  Unpacks as the
    4-tuple (normals, labels, n_components, rounds)."""

    def __init__(self, normals, labels, n_components, rounds):
        self.normals, self.labels, self.n_components, self.rounds = normals, labels, n_components, rounds

    def __iter__(self):
        return iter((self.normals, self.labels, self.n_components, self.rounds))


def orient_normals(points, normals, neighbors, up=(0.0, 0.0, 1.0), centers=None, visibility=None):
    """stage 3 -> Oriented (normals, labels, n_components, rounds)"""
    what = 'orient_normals'
    p = _points(points, what)
    n = p.shape[0]
    nrm = _normals(normals, n, what)
    if not isinstance(neighbors, (torch.Tensor, np.ndarray)):
        raise ValueError('%s: neighbors must be a numpy array or a torch tensor of dtype int32' % what)
    nb = torch.as_tensor(neighbors)
    if nb.dtype != torch.int32 or nb.dim() != 2 or nb.shape[0] != n or not 1 <= nb.shape[1] <= 32:
        raise ValueError('%s: neighbors must be int32 [N, k] for N = %d points and k in 1 .. 32, got %s %s' % (what, n, nb.dtype, tuple(nb.shape)))
    if not 1 <= n <= 2 ** 31 - 1:
        raise ValueError('%s: %d points (1 .. 2^31 - 1)' % (what, n))
    u = _up(up, what)
    if centers is None and visibility is not None:
        raise ValueError('%s: a visibility needs the centers of its views' % what)
    ctr = None if centers is None else _centers(centers, what)
    V = 0 if ctr is None else ctr.shape[0]
    vis = None if ctr is None else _visibility(visibility, V, n, what)
    p = _device(p)
    dev = p.device
    nrm, nb = nrm.to(dev).contiguous(), nb.to(dev).contiguous()
    bits = None
    if ctr is not None:
        bits = _pack(vis, V, n, dev, what)
        ctr = ctr.to(dev).contiguous()
    size = lib().mvsdf_normals_orient_workspace_bytes(n)
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    out = torch.empty(n, 3, dtype=torch.float64, device=dev)
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    check(lib().mvsdf_normals_orient(_vp(p), _vp(nrm), _vp(nb), n, nb.shape[1], u[0], u[1], u[2], _vp(ctr), _vp(bits), V, _vp(ws), size, _vp(out),
                                     _vp(labels), _stream(p)), 'mvsdf_normals_orient')
    n_components, rounds, err = _header(ws, K.MVSDF_NR_ORIENT_H_WORDS)
    raise_for_bits(err, what, ERRORS)
    return Oriented(out, labels, n_components, rounds)


def orient_to_views(points, normals, centers, visibility):
    """stage 4 -> normals fp64 [N,3] on the device"""
    what = 'orient_to_views'
    p = _points(points, what)
    n = p.shape[0]
    nrm = _normals(normals, n, what)
    ctr = _centers(centers, what)
    if not 1 <= n <= 2 ** 31 - 1:
        raise ValueError('%s: %d points (1 .. 2^31 - 1)' % (what, n))
    V = ctr.shape[0]
    vis = _visibility(visibility, V, n, what)
    p = _device(p)
    dev = p.device
    nrm, ctr = nrm.to(dev).contiguous(), ctr.to(dev).contiguous()
    bits = _pack(vis, V, n, dev, what)
    out = torch.empty(n, 3, dtype=torch.float64, device=dev)
    hdr = torch.empty(256, dtype=torch.uint8, device=dev)
    check(lib().mvsdf_normals_to_views(_vp(p), _vp(nrm), n, _vp(ctr), _vp(bits), V, _vp(out), _vp(hdr), _stream(p)), 'mvsdf_normals_to_views')
    raise_for_bits(_header(hdr, K.MVSDF_ERRW_H_WORDS)[K.MVSDF_ERRW_H_ERR], what, ERRORS)
    return out
