"""Rigid registration and F-score evaluation on the device: what the Tanks and Temples (T&T) benchmark does to a reconstruction, and what
comparing two of our own surfaces needs.  Kernels: csrc/registration.hip (the design: DESIGN.md); tests/registration_ref.py restates every
definition in numpy and the device results equal it bit for bit.

The definitions (fp64 throughout, no FMA contraction, in the order written; a transformation T is a host fp64 4x4 matrix):

1. NearestTree(refs).query(queries, max_dist) -> (dist, index).  d2(q, r) = (dx*dx + dy*dy) + dz*dz.  index = the smallest input index among
   the references at the minimal d2, dist = sqrt(d2); where dist is not < max_dist (which may be +inf): dist = +inf, index = -1.  The tree
   (csrc/nn_tree.h) is built once and kept: a query sorts nothing.
2. transform_points(points, T): row a = ((T[a][0]*x + T[a][1]*y) + T[a][2]*z) + T[a][3].
3. crop_volume(points, axis, axis_min, axis_max, polygon): Open3D's SelectionPolygonVolume as the T&T toolbox uses it, WRITTEN FROM MEMORY of
   Open3D: the rule as written here is the definition.  (u, v, w) = (1, 2, 0) for axis X, (0, 2, 1) for Y, (0, 1, 2) for Z.  A point p is
   kept iff axis_min <= p[w] <= axis_max and the number of polygon edges (P_i, P_j), j = i + 1 mod n, is odd for which both
   (P_i[v] < p[v] and P_j[v] >= p[v]) or (P_j[v] < p[v] and P_i[v] >= p[v]), and
   P_i[u] + (p[v] - P_i[v]) / (P_j[v] - P_i[v]) * (P_j[u] - P_i[u]) < p[u], evaluated left to right.  3 to 4096 vertices.
4. voxel_downsample(points, voxel): origin o_a = min_a - voxel/2, cell g_a = floor((p_a - o_a) / voxel) (g_a >= 2^21: ValueError), key =
   gx | gy << 21 | gz << 42; per occupied voxel in ascending key: mean = s / count with s summed from 0.0 in ascending input index.
   uniform_downsample(points, k) = points[::k].
5. icp(source, tree, init, max_dist, max_iter, rel_fitness, rel_rmse): point-to-point ICP.  An evaluation at T: every source point moved by T
   queries the tree (1.); over the matched pairs (index >= 0), with c = the centre of the tree's bounding box ((lo + hi) * 0.5 per axis),
   p = T s - c and q = refs[index] - c, the 17 sums n, sum d2, sum p [3], sum q [3], sum p_a*q_b [9] are taken in source order: a lane sums 8
   consecutive items from 0.0 (skipping unmatched ones), then a halving tree over 256 lanes (lane t += lane t + w, w = 128 .. 1), then over the
   block partials one lane of 1024 per ceil(blocks / 1024) consecutive partials from 0.0 and a halving tree over the 1024.  fitness = n / |source|,
   inlier_rmse = sqrt(sum d2 / n); n == 0: ValueError.  The update by Horn's closed form, in Python floats with math.sqrt only (horn_update):
   M[a][b] = sum p_a*q_b - (sum p_a * sum q_b) / n; N = the symmetric 4x4
       [Sxx+Syy+Szz  Syz-Szy       Szx-Sxz       Sxy-Syx     ]
       [ .           Sxx-Syy-Szz   Sxy+Syx       Szx+Sxz     ]
       [ .            .            -Sxx+Syy-Szz  Syz+Szy     ]
       [ .            .             .            -Sxx-Syy+Szz]   (every entry summed left to right);
   cyclic Jacobi, 16 sweeps over (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), a rotation whose off-diagonal entry is exactly 0 skipped:
   theta = (A[q][q] - A[p][p]) / (2 * A[p][q]), t = sign(theta) / (|theta| + sqrt(theta*theta + 1)), c = 1 / sqrt(t*t + 1), s = t * c; columns
   then rows p, q of A and the columns of V become (c*xp - s*xq, s*xp + c*xq); A[p][q] = A[q][p] = 0.  The quaternion (w, x, y, z) = the column
   of V at the first largest diagonal entry, divided by sqrt(((w*w + x*x) + y*y) + z*z), negated if w < 0; R from it; with pm = sum p / n + c
   and qm = sum q / n + c: t_a = qm_a - ((R[a][0]*pm_0 + R[a][1]*pm_1) + R[a][2]*pm_2); T <- U T with
   (U T)[a][b] = ((U[a][0]*T[0][b] + U[a][1]*T[1][b]) + U[a][2]*T[2][b]) + U[a][3]*T[3][b], last row (0, 0, 0, 1).
   The loop is Open3D's: evaluate at init; then up to max_iter times: update T, evaluate, stop once |fitness - previous| < rel_fitness and
   |inlier_rmse - previous| < rel_rmse (absolute differences, as in Open3D despite the names).  The reported fitness and inlier_rmse are those
   of the returned transformation.  Degenerate correspondences (collinear pairs, n < 3) are NOT detected: the result is then some rotation.
6. fscore(rec, gt, tau, stretch, bins_per_tau): d(rec -> gt) and d(gt -> rec) by 1. with max_dist = +inf (the device cuts the walks off at
   max(tau, the last edge), beyond which no result below reads a distance); precision = |{d(rec -> gt) < tau}| /
   |rec|, recall likewise from gt to rec, fscore = 2 P R / (P + R), 0 when P + R = 0.  Two int64 histograms over the edges tau*k/bins_per_tau,
   k = 0 .. stretch*bins_per_tau: the bin of d is the number of edges[1:] that are <= d; a d at or beyond the last edge is dropped.
7. tnt_evaluate(rec, gt, crop, init, tau): the toolbox's sequence AS RECALLED; the table here is the definition.  G = crop(gt), T = init.  Per
   stage: S = crop(T rec); both S and G filtered; reg = icp(S', tree over G', identity, max_dist, 20 iterations); T <- reg T.
       stage   filter of both clouds                                   max_dist
       1       voxel_downsample at tau                                 80 tau
       2       voxel_downsample at tau / 2                             20 tau
       3       uniform_downsample, k = ceil(N / max_points) per cloud   2 tau
   Then fscore(voxel(crop(T rec), tau / 2), voxel(G, tau / 2), tau).

Files (load_tnt_scene, load_trajectory) are the benchmark's; align_centres replaces the toolbox's RANSAC over camera centres by the closed form
over all of them (no outlier rejection)."""
import collections
import ctypes as C
import json
import math
import os

import numpy as np
import torch

from ._lib import check, lib, K, raise_for_bits, _header, _stream, _vp, f64_from_bits
from .mesh import Mesh

MAX_POLYGON = K.MVSDF_REG_MAX_POLYGON
MAX_BINS = 4096
IDENTITY = ((1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0))
JACOBI_SWEEPS = 16
JACOBI_PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
TNT_MAX_POINTS = 4000000
# tau per scene of the T&T training set, as recalled from the toolbox (tools/eval_tnt.py --tau overrides)
TNT_TAU = {'Barn': 0.01, 'Caterpillar': 0.005, 'Church': 0.025, 'Courthouse': 0.025, 'Ignatius': 0.003, 'Meetingroom': 0.01, 'Truck': 0.005}

Registration = collections.namedtuple('Registration', 'transformation fitness inlier_rmse iterations')


# the error bits of a registration call (csrc/registration.hip), in the order they are looked at
ERRORS = [(K.MVSDF_PC_ERR_FINITE, ValueError, 'a coordinate is NaN or infinite'),
          (K.MVSDF_PC_ERR_COORD, ValueError, 'the points span 2^21 or more voxels on an axis')]


def _points(x, what, name='points', device=None, empty_ok=False):
    t = torch.as_tensor(x)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError('%s: %s must be [N, 3], got shape %s' % (what, name, tuple(t.shape)))
    if t.shape[0] == 0 and not empty_ok:
        raise ValueError('%s: %s is empty' % (what, name))
    if device is not None:
        t = t.to(device)
    elif not t.is_cuda:
        t = t.cuda()
    return t.to(torch.float64).contiguous()


def _matrix(T, what):
    """a 4x4 transformation as rows of Python floats"""
    m = np.asarray(T, dtype=np.float64)
    if m.shape != (4, 4) or not np.isfinite(m).all():
        raise ValueError('%s: a transformation must be a finite 4x4 matrix' % what)
    return [[float(m[a, b]) for b in range(4)] for a in range(4)]


def _c16(T):
    return (C.c_double * 16)(*[T[a][b] for a in range(4) for b in range(4)])


def _max_dist(x, what):
    x = float(x)
    if not x > 0:
        raise ValueError('%s: max_dist must be positive (it may be inf), got %r' % (what, x))
    return x


class NearestTree:
    """definition 1: the references sorted and boxed once; query() as often as needed.  centre: the centre of their bounding box."""

    def __init__(self, refs):
        what = 'NearestTree'
        r = _points(refs, what, 'refs')
        self.refs = r
        self.n = r.shape[0]
        self._size = lib().mvsdf_reg_tree_workspace_bytes(self.n)
        if self._size == 0:
            raise ValueError('%s: %d references (at most 2^31 - 1)' % (what, self.n))
        self._ws = torch.empty(self._size, dtype=torch.uint8, device=r.device)
        check(lib().mvsdf_reg_tree_build(_vp(r), self.n, _vp(self._ws), self._size, _stream(r)), 'mvsdf_reg_tree_build')
        h = _header(self._ws, K.MVSDF_REG_TREE_H_WORDS)
        raise_for_bits(h[K.MVSDF_REG_TREE_H_ERR], what, ERRORS)
        self.centre = tuple(f64_from_bits(b) for b in h[K.MVSDF_REG_TREE_H_CENTRE:K.MVSDF_REG_TREE_H_WORDS])

    def __len__(self):
        return self.n

    def query(self, queries, max_dist=float('inf'), transform=None, check_finite=True):
        """(dist fp64 [Q], index int32 [Q]) on the device, the queries first moved by `transform` if given.  The launch does not wait for the
        host; with check_finite (the default) the error word is then read, which does, and a NaN or infinite query raises ValueError.  Without
        it such a query gives (+inf, -1)."""
        what = 'NearestTree.query'
        q = _points(queries, what, 'queries', self.refs.device, empty_ok=True)
        max_dist = _max_dist(max_dist, what)
        nq = q.shape[0]
        dist = torch.empty(nq, dtype=torch.float64, device=q.device)
        index = torch.empty(nq, dtype=torch.int32, device=q.device)
        if nq == 0:
            return dist, index
        err = torch.zeros(1, dtype=torch.int32, device=q.device)  # zeros: the kernel only ORs error bits into this word
        T = None if transform is None else _c16(_matrix(transform, what))
        check(lib().mvsdf_reg_tree_query(_vp(self._ws), self._size, self.n, _vp(q), nq, T, max_dist, _vp(dist), None, _vp(index), _vp(err),
                                         _stream(q)), 'mvsdf_reg_tree_query')
        if check_finite:
            raise_for_bits(int(err.item()), what, ERRORS)
        return dist, index


def transform_points(points, T):
    """definition 2 -> fp64 [N, 3] on the device"""
    what = 'transform_points'
    p = _points(points, what, empty_ok=True)
    out = torch.empty_like(p)
    check(lib().mvsdf_reg_transform(_vp(p), p.shape[0], _c16(_matrix(T, what)), _vp(out), _stream(p)), 'mvsdf_reg_transform')
    return out


def _axis(axis, what):
    if isinstance(axis, str) and axis.upper() in ('X', 'Y', 'Z'):
        return 'XYZ'.index(axis.upper())
    if axis in (0, 1, 2):
        return int(axis)
    raise ValueError('%s: axis must be X, Y or Z, got %r' % (what, axis))


def crop_volume(points, axis, axis_min, axis_max, polygon):
    """definition 3 -> (keep bool [N], the kept points fp64 [K, 3] in input order), both on the device"""
    what = 'crop_volume'
    p = _points(points, what)
    a = _axis(axis, what)
    poly = np.asarray(polygon, dtype=np.float64)
    if poly.ndim != 2 or poly.shape[1] != 3 or not 3 <= poly.shape[0] <= MAX_POLYGON or not np.isfinite(poly).all():
        raise ValueError('%s: the polygon must be 3 to %d finite vertices [n, 3]' % (what, MAX_POLYGON))
    axis_min, axis_max = float(axis_min), float(axis_max)
    if math.isnan(axis_min) or math.isnan(axis_max):
        raise ValueError('%s: axis_min / axis_max must not be NaN' % what)
    n = p.shape[0]
    dev_poly = torch.from_numpy(np.ascontiguousarray(poly)).to(p.device)
    size = lib().mvsdf_reg_crop_workspace_bytes(n)
    ws = torch.empty(size, dtype=torch.uint8, device=p.device)
    keep = torch.empty(n, dtype=torch.uint8, device=p.device)
    out = torch.empty(n, 3, dtype=torch.float64, device=p.device)
    check(lib().mvsdf_reg_crop(_vp(p), n, a, axis_min, axis_max, _vp(dev_poly), poly.shape[0], _vp(ws), size, _vp(keep), _vp(out), _stream(p)),
          'mvsdf_reg_crop')
    kept, = _header(ws, K.MVSDF_ROWS_H_WORDS)
    return keep.bool(), out[:kept]


def voxel_downsample(points, voxel):
    """definition 4 -> (means fp64 [M, 3], counts int32 [M]) on the device, in ascending voxel key"""
    what = 'voxel_downsample'
    p = _points(points, what)
    voxel = float(voxel)
    if not (voxel > 0 and math.isfinite(voxel)):
        raise ValueError('%s: voxel must be a positive finite number, got %r' % (what, voxel))
    n = p.shape[0]
    size = lib().mvsdf_reg_voxel_workspace_bytes(n)
    if size == 0:
        raise ValueError('%s: %d points (at most 2^31 - 1)' % (what, n))
    ws = torch.empty(size, dtype=torch.uint8, device=p.device)
    means = torch.empty(n, 3, dtype=torch.float64, device=p.device)
    counts = torch.empty(n, dtype=torch.int32, device=p.device)
    check(lib().mvsdf_reg_voxel(_vp(p), n, voxel, _vp(ws), size, _vp(means), _vp(counts), _stream(p)), 'mvsdf_reg_voxel')
    m, err = _header(ws, K.MVSDF_REG_VOXEL_H_WORDS)
    raise_for_bits(err, what, ERRORS)
    return means[:m], counts[:m]


def uniform_downsample(points, k):
    """points[::k]"""
    k = int(k)
    if k < 1:
        raise ValueError('uniform_downsample: k must be >= 1')
    return _points(points, 'uniform_downsample', empty_ok=True)[::k].contiguous()


# ---------------------------------------------------------------- ICP ----------------------------------------------------------------
def compose(U, T):
    """U T of definition 5, rows of Python floats"""
    out = [[((U[a][0] * T[0][b] + U[a][1] * T[1][b]) + U[a][2] * T[2][b]) + U[a][3] * T[3][b] for b in range(4)] for a in range(3)]
    out.append([0.0, 0.0, 0.0, 1.0])
    return out


def horn_rotation(M):
    """the rotation that maximises sum q . R p for the 3x3 correlation M[a][b] = sum p_a q_b (definition 5: Horn's quaternion by cyclic Jacobi)"""
    Sxx, Sxy, Sxz = M[0]
    Syx, Syy, Syz = M[1]
    Szx, Szy, Szz = M[2]
    A = [[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
         [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
         [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
         [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]]
    V = [[1.0 if a == b else 0.0 for b in range(4)] for a in range(4)]
    for _ in range(JACOBI_SWEEPS):
        for p, q in JACOBI_PAIRS:
            apq = A[p][q]
            if apq == 0.0:
                continue
            theta = (A[q][q] - A[p][p]) / (2 * apq)
            t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1))
            c = 1 / math.sqrt(t * t + 1)
            s = t * c
            for k in range(4):
                xp, xq = A[k][p], A[k][q]
                A[k][p], A[k][q] = c * xp - s * xq, s * xp + c * xq
            for k in range(4):
                xp, xq = A[p][k], A[q][k]
                A[p][k], A[q][k] = c * xp - s * xq, s * xp + c * xq
            for k in range(4):
                xp, xq = V[k][p], V[k][q]
                V[k][p], V[k][q] = c * xp - s * xq, s * xp + c * xq
            A[p][q] = A[q][p] = 0.0
    m = 0
    for k in range(1, 4):
        if A[k][k] > A[m][m]:
            m = k
    w, x, y, z = V[0][m], V[1][m], V[2][m], V[3][m]
    nrm = math.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / nrm, x / nrm, y / nrm, z / nrm
    if w < 0:
        w, x, y, z = -w, -x, -y, -z
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]


def horn_update(n, sums, centre):
    """the rigid update U (rows of Python floats) from the 17 sums of an evaluation: sums = [sum d2, sum p [3], sum q [3], sum p_a q_b [9]]"""
    sp, sq, spq = sums[1:4], sums[4:7], sums[7:16]
    M = [[spq[3 * a + b] - (sp[a] * sq[b]) / n for b in range(3)] for a in range(3)]
    R = horn_rotation(M)
    pm = [sp[a] / n + centre[a] for a in range(3)]
    qm = [sq[a] / n + centre[a] for a in range(3)]
    U = [[R[a][0], R[a][1], R[a][2], qm[a] - ((R[a][0] * pm[0] + R[a][1] * pm[1]) + R[a][2] * pm[2])] for a in range(3)]
    U.append([0.0, 0.0, 0.0, 1.0])
    return U


class _Pairs:
    """the buffers of an ICP's evaluations: one allocation for all iterations"""

    def __init__(self, source, tree, what):
        self.src = _points(source, what, 'source', tree.refs.device)
        self.tree = tree
        self.ns = self.src.shape[0]
        self.size = lib().mvsdf_reg_pairs_workspace_bytes(self.ns)
        self.ws = torch.empty(self.size, dtype=torch.uint8, device=self.src.device)
        self.d2 = torch.empty(self.ns, dtype=torch.float64, device=self.src.device)
        self.index = torch.empty(self.ns, dtype=torch.int32, device=self.src.device)

    def sums(self, T, max_dist, what):
        t = self.tree
        check(lib().mvsdf_reg_icp_step(_vp(t._ws), t._size, t.n, _vp(t.refs), _vp(self.src), self.ns, _c16(T), max_dist, _vp(self.ws), self.size,
                                       _vp(self.d2), _vp(self.index), _stream(self.src)), 'mvsdf_reg_icp_step')
        h = _header(self.ws, K.MVSDF_REG_ICP_H_WORDS)
        raise_for_bits(h[K.MVSDF_REG_ICP_H_ERR], what, ERRORS)
        return h[K.MVSDF_REG_ICP_H_N], [f64_from_bits(b) for b in h[K.MVSDF_REG_ICP_H_SUMS:K.MVSDF_REG_ICP_H_ERR]]


def pair_sums(source, tree, T=IDENTITY, max_dist=float('inf')):
    """one evaluation of definition 5 at T -> (n, [sum d2, sum p [3], sum q [3], sum p_a q_b [9]] as Python floats, d2 fp64 [S], index int32 [S])"""
    what = 'pair_sums'
    pr = _Pairs(source, tree, what)
    n, s = pr.sums(_matrix(T, what), _max_dist(max_dist, what), what)
    return n, s, pr.d2, pr.index


def icp(source, target_tree, init=IDENTITY, max_dist=float('inf'), max_iter=20, rel_fitness=1e-6, rel_rmse=1e-6):
    """definition 5 -> Registration(transformation fp64 numpy [4, 4], fitness, inlier_rmse, iterations = the updates applied).  One host wait
    per evaluation (the 17 sums); the tree stays resident and nothing is sorted."""
    what = 'icp'
    if not isinstance(target_tree, NearestTree):
        raise TypeError('%s: target_tree must be a NearestTree' % what)
    T = _matrix(init, what)
    max_dist = _max_dist(max_dist, what)
    pr = _Pairs(source, target_tree, what)

    def evaluate(T):
        n, s = pr.sums(T, max_dist, what)
        if n == 0:
            raise ValueError('%s: no source point has a target point within max_dist = %g' % (what, max_dist))
        return n, s, n / pr.ns, math.sqrt(s[0] / n)

    n, s, fitness, rmse = evaluate(T)
    iterations = 0
    for _ in range(int(max_iter)):
        T = compose(horn_update(n, s, target_tree.centre), T)
        iterations += 1
        n, s, f2, r2 = evaluate(T)
        done = abs(f2 - fitness) < rel_fitness and abs(r2 - rmse) < rel_rmse
        fitness, rmse = f2, r2
        if done:
            break
    return Registration(np.array(T, dtype=np.float64), fitness, rmse, iterations)


# ---------------------------------------------------------------- the score ----------------------------------------------------------------
def _edges(tau, stretch, bins_per_tau):
    return [tau * k / bins_per_tau for k in range(stretch * bins_per_tau + 1)]


def _hist(dist, edges, tau):
    out = torch.empty(len(edges), dtype=torch.int64, device=dist.device)
    check(lib().mvsdf_reg_hist(_vp(dist), dist.shape[0], _vp(edges), edges.shape[0], tau, _vp(out), _stream(dist)), 'mvsdf_reg_hist')
    return out


def fscore(rec, gt, tau, stretch=5, bins_per_tau=100):
    """definition 6 -> dict: precision, recall, fscore (Python floats), below_rec / below_gt (the counts under tau), n_rec, n_gt, hist_rec /
    hist_gt (int64 numpy [stretch * bins_per_tau]), edges (fp64 numpy), dist_rec / dist_gt (fp64 device tensors, +inf from max(tau, the last edge) on)"""
    what = 'fscore'
    r = _points(rec, what, 'rec')
    g = _points(gt, what, 'gt', r.device)
    tau = float(tau)
    stretch, bins_per_tau = int(stretch), int(bins_per_tau)
    if not (tau > 0 and math.isfinite(tau)):
        raise ValueError('%s: tau must be a positive finite number, got %r' % (what, tau))
    if stretch < 1 or bins_per_tau < 1 or stretch * bins_per_tau > MAX_BINS:
        raise ValueError('%s: stretch * bins_per_tau must be 1 .. %d' % (what, MAX_BINS))
    edges = np.array(_edges(tau, stretch, bins_per_tau), dtype=np.float64)
    dev_edges = torch.from_numpy(edges).to(r.device)
    # no result reads a distance at or beyond both tau and the last edge: cutting the walks off there changes nothing but their time
    cut = max(float(edges[-1]), tau)
    d_rec, _ = NearestTree(g).query(r, cut, check_finite=False)
    d_gt, _ = NearestTree(r).query(g, cut, check_finite=False)           # (both trees checked their references, which are the other's queries)
    h_rec = _hist(d_rec, dev_edges, tau).cpu().numpy()
    h_gt = _hist(d_gt, dev_edges, tau).cpu().numpy()
    n_rec, n_gt = r.shape[0], g.shape[0]
    below_rec, below_gt = int(h_rec[0]), int(h_gt[0])
    P, R = below_rec / n_rec, below_gt / n_gt
    F = 2 * P * R / (P + R) if P + R > 0 else 0.0
    return {'precision': P, 'recall': R, 'fscore': F, 'below_rec': below_rec, 'below_gt': below_gt, 'n_rec': n_rec, 'n_gt': n_gt,
            'hist_rec': h_rec[1:], 'hist_gt': h_gt[1:], 'edges': edges, 'dist_rec': d_rec, 'dist_gt': d_gt}


def tnt_stages(tau, max_points=TNT_MAX_POINTS):
    """the table of definition 7: (filter, its parameter, max_dist) per stage"""
    return [('voxel', tau, 80 * tau), ('voxel', tau / 2, 20 * tau), ('uniform', int(max_points), 2 * tau)]


def _crop_args(crop, what):
    try:
        return crop['orthogonal_axis'], float(crop['axis_min']), float(crop['axis_max']), np.asarray(crop['bounding_polygon'], dtype=np.float64)
    except (KeyError, TypeError) as e:
        raise ValueError('%s: crop must hold orthogonal_axis, axis_min, axis_max and bounding_polygon (%s)' % (what, e)) from None


def _filter(p, kind, value, what):
    if kind == 'voxel':
        return voxel_downsample(p, value)[0]
    if kind == 'uniform':
        return uniform_downsample(p, max(1, -(-p.shape[0] // int(value))))
    raise ValueError('%s: a stage filters by "voxel" or "uniform", got %r' % (what, kind))


def _cropped(p, crop, what, name):
    out = crop_volume(p, *crop)[1]
    if out.shape[0] == 0:
        raise ValueError('%s: the crop volume holds no point of %s' % (what, name))
    return out


def tnt_evaluate(rec, gt, crop, init, tau, stages=None, max_points=TNT_MAX_POINTS, max_iter=20, density=None):
    """definition 7.  rec / gt: a Mesh (sampled by chamfer.sample_mesh at `density`, default tau / 2) or points [N, 3]; crop: the dict of an Open3D
    SelectionPolygonVolume file (orthogonal_axis, axis_min, axis_max, bounding_polygon); init: rec's frame -> gt's frame; stages: a list of
    (filter 'voxel' | 'uniform', voxel edge | point limit, max_dist) that replaces tnt_stages(tau, max_points) -> dict: precision, recall,
    fscore, transformation (fp64 numpy [4, 4], rec -> gt), histograms (hist_rec, hist_gt), edges, registrations (per stage) and points: the
    counts [n_rec, n_gt, n_gt_cropped, then per stage (cropped rec, filtered rec, filtered gt), then cropped rec, filtered rec, filtered gt
    of the score]."""
    what = 'tnt_evaluate'
    tau = float(tau)
    if not (tau > 0 and math.isfinite(tau)):
        raise ValueError('%s: tau must be a positive finite number, got %r' % (what, tau))

    def cloud(x, name):
        if isinstance(x, Mesh):
            from .chamfer import sample_mesh
            return sample_mesh(x, tau / 2 if density is None else density)
        return _points(x, what, name)
    r = cloud(rec, 'rec')
    g = cloud(gt, 'gt').to(r.device)
    crop = _crop_args(crop, what)
    T = _matrix(init, what)
    stages = tnt_stages(tau, max_points) if stages is None else list(stages)
    G = _cropped(g, crop, what, 'gt')
    counts = [r.shape[0], g.shape[0], G.shape[0]]
    regs = []
    for kind, value, max_dist in stages:
        S = _cropped(transform_points(r, T), crop, what, 'rec')
        s, t = _filter(S, kind, value, what), _filter(G, kind, value, what)
        counts += [S.shape[0], s.shape[0], t.shape[0]]
        reg = icp(s, NearestTree(t), IDENTITY, max_dist, max_iter)
        regs.append(reg)
        T = compose(_matrix(reg.transformation, what), T)
    S = _cropped(transform_points(r, T), crop, what, 'rec')
    s, t = voxel_downsample(S, tau / 2)[0], voxel_downsample(G, tau / 2)[0]
    counts += [S.shape[0], s.shape[0], t.shape[0]]
    f = fscore(s, t, tau)
    return {'precision': f['precision'], 'recall': f['recall'], 'fscore': f['fscore'], 'transformation': np.array(T, dtype=np.float64),
            'histograms': (f['hist_rec'], f['hist_gt']), 'edges': f['edges'], 'points': counts, 'registrations': regs,
            'below_rec': f['below_rec'], 'below_gt': f['below_gt']}


# ---------------------------------------------------------------- files ----------------------------------------------------------------
def load_trajectory(path):
    """a T&T .log trajectory: per camera a line of three integers, then the four rows of its camera-to-world matrix -> a list of
    (meta: three ints, pose fp64 numpy [4, 4])"""
    with open(path) as f:
        rows = [ln.split() for ln in f if ln.strip()]
    if len(rows) % 5:
        raise ValueError('load_trajectory: %s: %d non-empty lines, not a multiple of 5' % (path, len(rows)))
    out = []
    for k in range(0, len(rows), 5):
        try:
            if len(rows[k]) != 3 or any(len(r) != 4 for r in rows[k + 1:k + 5]):
                raise ValueError
            meta = tuple(int(x) for x in rows[k])
            pose = np.array([[float(x) for x in r] for r in rows[k + 1:k + 5]], dtype=np.float64)
        except ValueError:
            raise ValueError('load_trajectory: %s: camera %d is not "i j k" followed by a 4x4 matrix' % (path, k // 5)) from None
        out.append((meta, pose))
    return out


def load_tnt_scene(scene_dir, scene):
    """the ground truth of one T&T scene: {scene}.ply (points), {scene}.json (the crop volume), {scene}_trans.txt (COLMAP's frame -> the ground
    truth's, 4x4) and, if present, {scene}_COLMAP_SfM.log -> dict gt (fp64 numpy [N, 3]), crop (the json's dict), trans (fp64 numpy [4, 4]),
    trajectory (load_trajectory's list, or None)"""
    from .chamfer import load_points
    base = os.path.join(scene_dir, scene)
    for ext in ('.ply', '.json', '_trans.txt'):
        if not os.path.exists(base + ext):
            raise FileNotFoundError('load_tnt_scene: %s: no such file' % (base + ext))
    with open(base + '.json') as f:
        crop = json.load(f)
    _crop_args(crop, 'load_tnt_scene')
    trans = np.loadtxt(base + '_trans.txt', dtype=np.float64)
    if trans.shape != (4, 4):
        raise ValueError('load_tnt_scene: %s_trans.txt is not a 4x4 matrix' % base)
    log = base + '_COLMAP_SfM.log'
    return {'gt': load_points(base + '.ply'), 'crop': crop, 'trans': trans, 'trajectory': load_trajectory(log) if os.path.exists(log) else None}


def align_centres(src, dst, with_scale=True):
    """the similarity (fp64 numpy [4, 4]) that takes the points src [N, 3] (camera centres of the user's trajectory) onto dst [N, 3] (COLMAP's) in
    closed form: the rotation by horn_rotation over the centred sets, the scale sqrt(sum |q - qm|^2 / sum |p - pm|^2) (1 without with_scale),
    t = qm - scale R pm.  The toolbox estimates this by RANSAC over the centres; here every camera counts and none is rejected."""
    p, q = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 3 or p.shape != q.shape or len(p) < 3 or not (np.isfinite(p).all() and np.isfinite(q).all()):
        raise ValueError('align_centres: src and dst must be the same [N >= 3, 3] finite points')
    n = len(p)
    pm = [math.fsum(p[:, a]) / n for a in range(3)]
    qm = [math.fsum(q[:, a]) / n for a in range(3)]
    pc = [[float(p[i, a]) - pm[a] for a in range(3)] for i in range(n)]
    qc = [[float(q[i, a]) - qm[a] for a in range(3)] for i in range(n)]
    M = [[math.fsum(pc[i][a] * qc[i][b] for i in range(n)) for b in range(3)] for a in range(3)]
    R = horn_rotation(M)
    sp = math.fsum(x * x for row in pc for x in row)
    sq = math.fsum(x * x for row in qc for x in row)
    if not sp > 0:
        raise ValueError('align_centres: the source centres coincide')
    scale = math.sqrt(sq / sp) if with_scale else 1.0
    T = [[scale * R[a][0], scale * R[a][1], scale * R[a][2], qm[a] - scale * ((R[a][0] * pm[0] + R[a][1] * pm[1]) + R[a][2] * pm[2])] for a in range(3)]
    T.append([0.0, 0.0, 0.0, 1.0])
    return np.array(T, dtype=np.float64)
