"""Point-cloud cleaning on the device: the automatic cut of the fused points.  Step 3 of the reference's BYOD.md is done by hand there ("Copy the
all_torch.ply to cut.ply and cut it": a person deletes floaters and background in a mesh editor); clean_points does it with no person in the
loop, so that Vis-MVSNet output -> imfunc4/ is one command (datasets/prepare.py, range_source='clean').  Kernels: csrc/cloud.hip (the design:
DESIGN.md); tests/cloud_ref.py restates every stage in numpy.  There is no reference code for this step; the definition below is this project's.

The definition.  Input: points fp64 [N,3], all finite.  fp64 throughout, in the order written, no FMA contraction.  The squared distance is
d2(i,j) = (dx*dx + dy*dy) + dz*dz, the formula of the Chamfer metric (chamfer.py).

- Stage A, neighbour distance.  For every point i: the k = nb_neighbors smallest d2(i,j) over all j != i (j != i by index: an exact duplicate of i
  is a neighbour at distance 0).  d_i = (sqrt(s_1) + sqrt(s_2) + ... + sqrt(s_k)) / k with s_1 <= ... <= s_k, summed left to right from 0.  The k
  smallest values are a multiset, ties are equal values and sqrt is correctly rounded, so d_i has one possible bit pattern.
- Stage B, sparse points.  m = the lower median of d: the element of rank (N-1)//2 of d sorted ascending.  Point i passes iff d_i <= knn_ratio * m
  (one fp64 product, one compare).
- Stage C, clusters.  eps = eps_ratio * m.  Among the points that passed B, i and j are adjacent iff d2(i,j) <= eps*eps (inclusive, as the Chamfer
  radius filter).  label_i = the smallest input index in i's connected component; -1 for points that failed B.  A component is kept iff its point
  count >= cluster_frac * (the largest component's count), compared in fp64.  cluster_frac = 1 keeps the largest (and any of exactly the same
  size, so there is no tie rule); a smaller value keeps a scene of several objects whole.
- Result.  keep_i = i passed B and its component is kept.  Points, colours and per-point side arrays are compacted in input order.

Limits: 1 <= nb_neighbors <= 32, nb_neighbors + 1 <= N <= 2^31 - 1, ratios finite and > 0, cluster_frac in (0, 1], shape [N,3], dtype fp64 (numpy
or torch; nothing is converted silently): ValueError before any launch.  A non-finite coordinate: ValueError through the call's error bits.

The defaults nb_neighbors=20, knn_ratio=3.0, eps_ratio=3.0, cluster_frac=1.0 are not tuned on real data.  They are what a CPU prototype of this
definition needed on the synthetic scene of tests/test_gpu_cloud.py (a fused sphere, 300 uniform outliers, a dense 400-point blob well outside):
no injected point kept, under 1 % of the fused points lost.

Where this differs from Open3D's remove_statistical_outlier (which is not a dependency and whose numerics are not claimed): the threshold is a
multiple of the median of d, not mean + std_ratio * sigma.  Far outliers dominate a mean (on the test scene: mean 0.021, sigma 0.125 against a median
of 0.010, so mean + 2 sigma passes everything up to 27 x the surface spacing), and a median is an element of d, so no floating sum's order has
to be tolerated.  And self is excluded by index, not by distance.
"""
import numpy as np
import torch

from ._lib import check, lib, K, MvsdfError, raise_for_bits, _header, _stream, _vp, f64_from_bits

MAX_NEIGHBORS = K.MVSDF_PC_MAX_K
INT32_MAX = 2 ** 31 - 1


# the error bits of a cloud call (csrc/cloud.hip), in the order they are looked at
ERRORS = [(K.MVSDF_PC_ERR_FINITE, ValueError, 'a coordinate is NaN or infinite'),
          (K.MVSDF_PC_ERR_ROUNDS, MvsdfError, 'the components loop reached its round limit')]


def _points(x, what):
    """fp64 [N,3] -> a contiguous device tensor; any other dtype or shape is refused"""
    if not isinstance(x, (torch.Tensor, np.ndarray)):
        raise ValueError('%s: points must be a numpy array or a torch tensor of dtype float64, got %s' % (what, type(x).__name__))
    t = torch.as_tensor(x)
    if t.dtype != torch.float64:
        raise ValueError('%s: points must be float64, got %s' % (what, t.dtype))
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError('%s: points must be [N, 3], got shape %s' % (what, tuple(t.shape)))
    return t


def _ratio(name, x, what):
    x = float(x)
    if not (np.isfinite(x) and x > 0):
        raise ValueError('%s: %s must be a positive finite number, got %r' % (what, name, x))
    return x


def _neighbors(k, n, what):
    if isinstance(k, bool) or int(k) != k:
        raise ValueError('%s: nb_neighbors must be an integer, got %r' % (what, k))
    k = int(k)
    if not 1 <= k <= MAX_NEIGHBORS:
        raise ValueError('%s: nb_neighbors must be in 1 .. %d, got %d' % (what, MAX_NEIGHBORS, k))
    if n < k + 1:
        raise ValueError('%s: %d points are too few for %d neighbours each (N >= nb_neighbors + 1)' % (what, n, k))
    if n > INT32_MAX:
        raise ValueError('%s: %d points (at most 2^31 - 1)' % (what, n))
    return k


def _workspace(p, what):
    size = lib().mvsdf_cloud_clean_workspace_bytes(p.shape[0])
    if size == 0:
        raise ValueError('%s: %d points (2 .. 2^31 - 1)' % (what, p.shape[0]))
    return torch.empty(size, dtype=torch.uint8, device=p.device), size


def _device(t):
    return (t if t.is_cuda else t.cuda()).contiguous()


def knn_mean_distance(points, nb_neighbors=20):
    """stage A: d fp64 [N] on the device"""
    what = 'knn_mean_distance'
    p = _points(points, what)
    k = _neighbors(nb_neighbors, p.shape[0], what)
    p = _device(p)
    n = p.shape[0]
    ws, size = _workspace(p, what)
    d = torch.empty(n, dtype=torch.float64, device=p.device)
    check(lib().mvsdf_cloud_knn(_vp(p), n, k, _vp(ws), size, _vp(d), _stream(p)), 'mvsdf_cloud_knn')
    raise_for_bits(_header(ws, K.MVSDF_CLOUD_H_WORDS)[K.MVSDF_CLOUD_H_ERR], what, ERRORS)
    return d


def radius_components(points, eps):
    """stage C with every point counted as passed: labels int32 [N] on the device, the smallest index of each point's component under
    d2 <= eps*eps"""
    what = 'radius_components'
    p = _points(points, what)
    eps = _ratio('eps', eps, what)
    n = p.shape[0]
    if n < 2 or n > INT32_MAX:
        raise ValueError('%s: %d points (2 .. 2^31 - 1)' % (what, n))
    p = _device(p)
    ws, size = _workspace(p, what)
    labels = torch.empty(n, dtype=torch.int32, device=p.device)
    check(lib().mvsdf_cloud_components(_vp(p), n, eps, _vp(ws), size, _vp(labels), _stream(p)), 'mvsdf_cloud_components')
    raise_for_bits(_header(ws, K.MVSDF_CLOUD_H_WORDS)[K.MVSDF_CLOUD_H_ERR], what, ERRORS)
    return labels


class Cleaned:
    """The result of clean_points: points fp64 [n_kept,3] and colors (uint8 [n_kept,3] or None) compacted in input order; per input point keep
    uint8 [N], d fp64 [N], labels int32 [N]; the scalars median, threshold, eps (floats), n_passed, n_clusters, largest, rounds (ints).  Tensors
    are on the device."""

    def __init__(self, points, colors, keep, d, labels, median, threshold, eps, n_passed, n_clusters, largest, rounds):
        self.points, self.colors, self.keep, self.d, self.labels = points, colors, keep, d, labels
        self.median, self.threshold, self.eps = median, threshold, eps
        self.n_passed, self.n_clusters, self.largest, self.rounds = n_passed, n_clusters, largest, rounds

    def __len__(self):
        return self.points.shape[0]

    def bbox(self):
        """(lo, hi): the exact minimum / maximum of the kept points per axis, fp64 [3] each on the device"""
        return self.points.amin(0), self.points.amax(0)


def compact(points, keep, colors=None, a=None, b=None, n_kept=None):
    """the rows of points fp64 [N,3] / colors uint8 [N,3] / a, b int32 [N] where keep (uint8 [N]) is set, in input order (device tensors)
    -> (points, colors, a, b), None where the input was None"""
    n = points.shape[0]
    dev = points.device
    size = lib().mvsdf_cloud_compact_workspace_bytes(n)
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    cap = n if n_kept is None else int(n_kept)
    out = [torch.empty(cap, 3, dtype=torch.float64, device=dev),
           None if colors is None else torch.empty(cap, 3, dtype=torch.uint8, device=dev),
           None if a is None else torch.empty(cap, dtype=torch.int32, device=dev),
           None if b is None else torch.empty(cap, dtype=torch.int32, device=dev)]
    check(lib().mvsdf_cloud_compact(_vp(points), _vp(colors), _vp(a), _vp(b), _vp(keep), n, _vp(ws), size, _vp(out[0]), _vp(out[1]), _vp(out[2]),
                                    _vp(out[3]), cap, _stream(points)), 'mvsdf_cloud_compact')
    if n_kept is None:
        rows = _header(ws, K.MVSDF_ROWS_H_WORDS)[K.MVSDF_ROWS_H_ROWS]
        out = [None if t is None else t[:rows] for t in out]
    return tuple(out)


def _clean(p, colors, a, b, nb_neighbors, knn_ratio, eps_ratio, cluster_frac, what):
    """p fp64 [N,3] validated by _points -> (Cleaned, a compacted, b compacted)"""
    k = _neighbors(nb_neighbors, p.shape[0], what)
    knn_ratio = _ratio('knn_ratio', knn_ratio, what)
    eps_ratio = _ratio('eps_ratio', eps_ratio, what)
    cluster_frac = _ratio('cluster_frac', cluster_frac, what)
    if cluster_frac > 1:
        raise ValueError('%s: cluster_frac must be in (0, 1], got %r' % (what, cluster_frac))
    n = p.shape[0]
    col = None
    if colors is not None:
        col = torch.as_tensor(colors)
        if tuple(col.shape) != (n, 3) or col.dtype != torch.uint8:
            raise ValueError('%s: colors must be uint8 [N, 3] for N = %d points, got %s %s' % (what, n, col.dtype, tuple(col.shape)))
    p = _device(p)
    dev = p.device
    if col is not None:
        col = col.to(dev).contiguous()
    ws, size = _workspace(p, what)
    d = torch.empty(n, dtype=torch.float64, device=dev)
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    keep = torch.empty(n, dtype=torch.uint8, device=dev)
    check(lib().mvsdf_cloud_clean(_vp(p), n, k, knn_ratio, eps_ratio, cluster_frac, _vp(ws), size, _vp(d), _vp(labels), _vp(keep), _stream(p)),
          'mvsdf_cloud_clean')
    n_passed, n_clusters, largest, n_kept, m, thr, eps, rounds, err = _header(ws, K.MVSDF_CLOUD_H_WORDS)
    raise_for_bits(err, what, ERRORS)
    pts, col, a, b = compact(p, keep, col, a, b, n_kept)
    return Cleaned(pts, col, keep, d, labels, f64_from_bits(m), f64_from_bits(thr), f64_from_bits(eps), n_passed, n_clusters, largest, rounds), a, b


def clean_points(points, colors=None, nb_neighbors=20, knn_ratio=3.0, eps_ratio=3.0, cluster_frac=1.0):
    """The module's definition -> Cleaned.  Device tensors are used where they are (the stream is theirs); numpy / CPU input is copied to the GPU."""
    what = 'clean_points'
    return _clean(_points(points, what), colors, None, None, nb_neighbors, knn_ratio, eps_ratio, cluster_frac, what)[0]


def clean_fused(fused, **kw):
    """fusion.Fused -> a new Fused: points / colors / view / pixel (/ normals) compacted, fused_depths set to 0 at every removed (view, pixel), counts and
    masked_depths as they were; its attribute `cleaned` is the Cleaned of the whole cloud.  kw: clean_points' keywords."""
    from .fusion import Fused
    what = 'clean_fused'
    bad = set(kw) - {'nb_neighbors', 'knn_ratio', 'eps_ratio', 'cluster_frac'}
    if bad:
        raise TypeError('%s: unknown keyword(s) %s' % (what, ', '.join(sorted(bad))))
    args = dict(nb_neighbors=20, knn_ratio=3.0, eps_ratio=3.0, cluster_frac=1.0)
    args.update(kw)
    c, view, pixel = _clean(_points(fused.points, what), fused.colors, fused.view.contiguous(), fused.pixel.contiguous(), what=what, **args)
    depths = fused.fused_depths.clone()
    gone = c.keep == 0
    hw = depths.shape[1] * depths.shape[2]
    depths.view(-1)[fused.view[gone].long() * hw + fused.pixel[gone].long()] = 0
    out = Fused(c.points, c.colors, view, pixel, fused.masked_depths, depths, fused.counts,
                None if fused.normals is None else fused.normals[c.keep != 0])      # the keep mask is in input order, as the compaction
    out.cleaned = c
    return out
