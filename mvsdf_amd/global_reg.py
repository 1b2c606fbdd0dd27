"""Global registration on the device: an alignment of two clouds that nothing relates yet, by FPFH descriptors, nearest descriptors and RANSAC over
the correspondences (PCL and Open3D know the sequence as registration_ransac_based_on_feature_matching).  registration.icp and tnt_evaluate need
an `init`; this module produces one from the clouds alone, so a TSDF mesh can be compared with a Poisson mesh of a COLMAP cloud, a run with a scan
in the scanner's frame, or two runs after a re-calibration.  Kernels: csrc/global_reg.hip (the design: DESIGN.md); tests/global_reg_ref.py restates
every stage in numpy and the device results equal it bit for bit.  PCL's and Open3D's rules are WRITTEN FROM MEMORY: the rules here are the definition.

The definition.  fp64 in the order written, no FMA contraction, only + - * / sqrt and det_math64.h's dm64_atan2_pos; everything else is integers.
d2(a, b) = (dx*dx + dy*dy) + dz*dz with d = a - b; a dot product x . y = (x0*y0 + x1*y1) + x2*y2; a cross product a x b =
(a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0).

1. spfh(points, normals, neighbors, radius=None) -> (hist int32 [N,33], count int32 [N]).  points, normals fp64 [N,3]; neighbors int32 [N,k],
   1 <= k <= 32, normally normals.knn_indices' rows.  For entry j of row i: d = p_j - p_i, d2 = (dx*dx + dy*dy) + dz*dz.  The pair is NEAR iff
   j != i and d2 > 0 and (no radius or d2 <= radius*radius).  For a near pair:
   - dn = d / sqrt(d2) per component; a1 = n_i . dn, a2 = n_j . dn;
   - if |a1| < |a2| the roles swap: the source is j, the target is i and dn is negated (PCL's computePairFeatures); otherwise the source is i;
   - u = n_source; phi = u . dn; v = dn x u, then each component divided by sqrt((vx*vx + vy*vy) + vz*vz): a length that is not > 0 makes the
     pair INVALID (zero normals, a normal along dn); w = u x v;
   - alpha = v . n_target; y = w . n_target, x = u . n_target; theta = atan2_pos(|y|, x), negated when y < 0.
   The bin of a feature f over [lo, hi] is b = floor(11 * ((f - lo) / (hi - lo))), then 0 unless b >= 0 (a NaN counts as 0), then 10 where b > 10.
   Group 0 is theta over [-PI, PI] (PI = 3.141592653589793), group 1 alpha over [-1, 1], group 2 phi over [-1, 1].  hist[i, 11 g + b] counts
   the valid near pairs of row i, count[i] is their number.  An entry that repeats in a row counts each time.

2. fpfh(points, neighbors, hist, count, radius=None) -> (features fp64 [N,33], codes int8 [N,33]).  Per point i and bin c: from 0.0, over the near
   entries j of row i (the test of 1., in row order) whose count[j] > 0, add (1 / d2) * (hist[j,c] / count[j]) (both integers converted to fp64;
   the point's own histogram is not added: the rows do not hold it).  Then per group of 11: s = the sum of its bins from 0.0 in bin order; where
   s > 0 each bin becomes 100 * value / s (left to right), otherwise 0.  The result does not depend on the unit of length.
   codes = min(127, floor(features * 1.27)).
   mirror_codes(codes) reverses the bins of groups 0 and 2 (b -> 10 - b): the codes of the same cloud with every normal negated (theta and phi
   change sign, alpha does not), up to features that lie on a bin edge.  orient_normals cannot know the global sign of an open scan; trying both
   costs one more match.

3. match_features(src_codes, dst_codes, mutual=False) -> (index int32 [Ns], dist int32 [Ns]).  D(i,j) = sum_c (s_ic - t_jc)^2 over codes in
   0 .. 127, an integer; index[i] = the j smallest under the total order (D(i,j), j), dist[i] = that D.  With mutual the same search runs from the
   targets to the sources and index[i] becomes -1 where the match of index[i] is not i (dist stays).

4. ransac(src, dst, corr, max_dist, hypotheses=100000, seed=0, edge_ratio=0.9) -> GlobalRegistration(transformation, inliers, hypothesis, checked,
   mask).  The correspondences m = 0 .. M-1, M >= 3, are the pairs (src[a_m], dst[b_m]): corr int32 [M,2], or an index array of 3. whose -1
   entries are dropped in order (a_m = the position).  Hypothesis h = 0 .. hypotheses-1, sample t = 0, 1, 2:
       x = seed XOR ((3h + t) * 0x9E3779B97F4A7C15 mod 2^64); x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB;
       x ^= x >> 31 (all mod 2^64: splitmix64's finaliser); m_t = ((x >> 32) * M) >> 32.
   Rejected before any fitting: two equal m_t, two equal a, two equal b; and for each of the sample pairs (0,1), (0,2), (1,2), with
   ls = sqrt(d2(s_u, s_v)) and lt = sqrt(d2(t_u, t_v)), unless ls >= edge_ratio*lt and lt >= edge_ratio*ls (Open3D's edge-length checker).
   The fit is registration.horn_update(3, sums, c) with c = the first sample's target point, p = s - c, q = t - c and the sums of p [3], q [3] and
   p_a*q_b [9] taken from 0.0 in sample order: T = [R | t].  A hypothesis survives iff all three samples have d2(T s, t) < max_dist*max_dist,
   T s by registration.transform_points' rule (a fit that is not a number fails this test); `checked` counts the survivors.  The score of a
   survivor is the number of correspondences with d2(T s_a, t_b) < max_dist*max_dist.  The winner is the first under (score descending, h
   ascending); mask marks its inliers.  Nothing survives: the identity, 0 inliers, hypothesis -1, a mask of zeros.  There is no early exit: the
   result is a function of the inputs alone.

5. global_register(source, target, voxel, ...): registration.voxel_downsample of both clouds at `voxel`; normals of each downsampled cloud by
   normals.estimate_normals(k) and normals.orient_normals with the default up (outward on a closed surface whatever the frame), or, where normals
   are given, those of the input point nearest to each voxel mean (registration.NearestTree over the input); the rows of normals.knn_indices(k);
   1. and 2. with feature_radius (default 5 voxel); 3.; 4. with max_dist (default 1.5 voxel) over the index array.  flip='auto' runs 3. and 4. a
   second time with mirror_codes of the source's codes and keeps the run with more inliers (a tie keeps the unmirrored one); flip=False runs
   only the unmirrored, flip=True only the mirrored codes.  A run with fewer than 3 correspondences does not count; none: ValueError.  With
   refine, registration.icp from the winner over the downsampled source against a tree over the downsampled target with max_dist.

ValueError before any launch: a dtype other than float64 / int32 / int8 where the definition names it (nothing is converted silently), a wrong shape,
k outside 1 .. 32, a radius, max_dist or voxel that is not positive, hypotheses outside 1 .. 2^22, a seed outside 0 .. 2^64 - 1, M < 3.  ValueError
through the call's error bits: a non-finite coordinate or normal, a neighbour or correspondence index out of range, a code outside 0 .. 127."""
import collections
import math

import numpy as np
import torch

from . import normals as _normals
from . import registration as _reg
from ._lib import check, lib, K, raise_for_bits, _header, _stream, _vp, f64_from_bits
from .cloud import _device, _points

DIM = 33
BINS = 11
MAX_HYPOTHESES = K.MVSDF_GREG_MAX_HYPOTHESES

GlobalRegistration = collections.namedtuple('GlobalRegistration', 'transformation inliers hypothesis checked mask')
GlobalResult = collections.namedtuple('GlobalResult', 'transformation inliers flipped fitness inlier_rmse')


# the error bits of a global registration call (csrc/global_reg.hip), in the order they are looked at
ERRORS = [(K.MVSDF_PC_ERR_FINITE, ValueError, 'a coordinate is NaN or infinite'),
          (K.MVSDF_PC_ERR_NORMAL, ValueError, 'a normal is NaN or infinite'),
          (K.MVSDF_PC_ERR_INDEX, ValueError, 'an index is out of range'),
          (K.MVSDF_PC_ERR_CODE, ValueError, 'a code is outside 0 .. 127')]


def _array(x, dtype, shape, what, name):
    """a tensor of exactly this dtype whose shape fits (None: any extent); nothing is converted"""
    if not isinstance(x, (torch.Tensor, np.ndarray)):
        raise ValueError('%s: %s must be a numpy array or a torch tensor of dtype %s' % (what, name, dtype))
    t = torch.as_tensor(x)
    if t.dtype != dtype or t.dim() != len(shape) or any(s is not None and s != g for s, g in zip(shape, t.shape)):
        raise ValueError('%s: %s must be %s %s, got %s %s' % (what, name, dtype, list(shape), t.dtype, tuple(t.shape)))
    return t


def _radius2(radius, what):
    if radius is None:
        return math.inf
    r = float(radius)
    if not (r > 0 and math.isfinite(r)):
        raise ValueError('%s: radius must be a positive finite number or None, got %r' % (what, radius))
    return r * r


def _rows(points, neighbors, what):
    p = _points(points, what)
    n = p.shape[0]
    if not 1 <= n <= 2 ** 31 - 1:
        raise ValueError('%s: %d points (1 .. 2^31 - 1)' % (what, n))
    nb = _array(neighbors, torch.int32, (n, None), what, 'neighbors')
    if not 1 <= nb.shape[1] <= 32:
        raise ValueError('%s: neighbors must hold 1 .. 32 entries per row, got %d' % (what, nb.shape[1]))
    p = _device(p)
    return p, nb.to(p.device).contiguous(), n, nb.shape[1]


def spfh(points, normals, neighbors, radius=None):
    """stage 1 -> (hist int32 [N,33], count int32 [N]) on the device"""
    what = 'spfh'
    r2 = _radius2(radius, what)
    p, nb, n, k = _rows(points, neighbors, what)
    nrm = _points(normals, what)
    if nrm.shape[0] != n:
        raise ValueError('%s: normals must be [N, 3] for N = %d points, got shape %s' % (what, n, tuple(nrm.shape)))
    nrm = nrm.to(p.device).contiguous()
    hist = torch.empty(n, DIM, dtype=torch.int32, device=p.device)
    count = torch.empty(n, dtype=torch.int32, device=p.device)
    err = torch.zeros(1, dtype=torch.int32, device=p.device)     # zeros: the kernels only OR error bits into this word
    check(lib().mvsdf_greg_spfh(_vp(p), _vp(nrm), _vp(nb), n, k, r2, _vp(hist), _vp(count), _vp(err), _stream(p)), 'mvsdf_greg_spfh')
    raise_for_bits(int(err.item()), what, ERRORS)
    return hist, count


def fpfh(points, neighbors, hist, count, radius=None):
    """stage 2 -> (features fp64 [N,33], codes int8 [N,33]) on the device"""
    what = 'fpfh'
    r2 = _radius2(radius, what)
    p, nb, n, k = _rows(points, neighbors, what)
    hist = _array(hist, torch.int32, (n, DIM), what, 'hist').to(p.device).contiguous()
    count = _array(count, torch.int32, (n,), what, 'count').to(p.device).contiguous()
    feat = torch.empty(n, DIM, dtype=torch.float64, device=p.device)
    codes = torch.empty(n, DIM, dtype=torch.int8, device=p.device)
    err = torch.zeros(1, dtype=torch.int32, device=p.device)     # zeros: the kernels only OR error bits into this word
    check(lib().mvsdf_greg_fpfh(_vp(p), _vp(nb), _vp(hist), _vp(count), n, k, r2, _vp(feat), _vp(codes), _vp(err), _stream(p)), 'mvsdf_greg_fpfh')
    raise_for_bits(int(err.item()), what, ERRORS)
    return feat, codes


def _codes(x, what, name, device=None):
    t = _array(x, torch.int8, (None, DIM), what, name)
    if not 1 <= t.shape[0] <= 2 ** 31 - 1:
        raise ValueError('%s: %s holds %d rows (1 .. 2^31 - 1)' % (what, name, t.shape[0]))
    return (_device(t) if device is None else t.to(device)).contiguous()


def mirror_codes(codes):
    """the codes with the bins of groups 0 (theta) and 2 (phi) reversed -> int8 [N,33] on the device"""
    c = _codes(codes, 'mirror_codes', 'codes')
    order = list(range(BINS - 1, -1, -1)) + list(range(BINS, 2 * BINS)) + list(range(3 * BINS - 1, 2 * BINS - 1, -1))
    return c[:, torch.tensor(order, device=c.device)].contiguous()


def match_splits(ns, nt):
    """over how many workgroups the matcher splits its walk over nt targets when there are ns sources"""
    return int(lib().mvsdf_greg_match_splits(int(ns), int(nt)))


def match_features(src_codes, dst_codes, mutual=False):
    """stage 3 -> (index int32 [Ns], dist int32 [Ns]) on the device"""
    what = 'match_features'
    s = _codes(src_codes, what, 'src_codes')
    t = _codes(dst_codes, what, 'dst_codes', s.device)
    ns, nt = s.shape[0], t.shape[0]
    size = lib().mvsdf_greg_match_workspace_bytes(ns, nt)
    ws = torch.empty(size, dtype=torch.uint8, device=s.device)
    index = torch.empty(ns, dtype=torch.int32, device=s.device)
    dist = torch.empty(ns, dtype=torch.int32, device=s.device)
    check(lib().mvsdf_greg_match(_vp(s), ns, _vp(t), nt, 1 if mutual else 0, _vp(ws), size, _vp(index), _vp(dist), _stream(s)), 'mvsdf_greg_match')
    raise_for_bits(_header(ws, K.MVSDF_ERRW_H_WORDS)[K.MVSDF_ERRW_H_ERR], what, ERRORS)
    return index, dist


def _correspondences(corr, device, what):
    if not isinstance(corr, (torch.Tensor, np.ndarray)):
        raise ValueError('%s: corr must be a numpy array or a torch tensor of dtype int32' % what)
    c = torch.as_tensor(corr)
    if c.dtype != torch.int32 or not (c.dim() == 1 or (c.dim() == 2 and c.shape[1] == 2)):
        raise ValueError('%s: corr must be int32 [M, 2] or an int32 index array [Ns], got %s %s' % (what, c.dtype, tuple(c.shape)))
    c = c.to(device)
    if c.dim() == 1:
        keep = torch.nonzero(c >= 0).reshape(-1)
        c = torch.stack([keep.to(torch.int32), c[keep]], 1)
    if c.shape[0] < 3:
        raise ValueError('%s: %d correspondences (at least 3)' % (what, c.shape[0]))
    return c.contiguous()


def ransac(src, dst, corr, max_dist, hypotheses=100000, seed=0, edge_ratio=0.9):
    """stage 4 -> GlobalRegistration(transformation fp64 numpy [4,4], inliers, hypothesis, checked (ints), mask bool [M] on the device)"""
    what = 'ransac'
    s = _points(src, what)
    d = _points(dst, what)
    if not (1 <= s.shape[0] <= 2 ** 31 - 1 and 1 <= d.shape[0] <= 2 ** 31 - 1):
        raise ValueError('%s: src and dst must hold 1 .. 2^31 - 1 points' % what)
    max_dist, edge_ratio = float(max_dist), float(edge_ratio)
    if not (max_dist > 0 and math.isfinite(max_dist)):
        raise ValueError('%s: max_dist must be a positive finite number, got %r' % (what, max_dist))
    if not 0 <= edge_ratio <= 1:
        raise ValueError('%s: edge_ratio must be in [0, 1], got %r' % (what, edge_ratio))
    if isinstance(hypotheses, bool) or int(hypotheses) != hypotheses or not 1 <= int(hypotheses) <= MAX_HYPOTHESES:
        raise ValueError('%s: hypotheses must be an integer in 1 .. %d, got %r' % (what, MAX_HYPOTHESES, hypotheses))
    if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
        raise ValueError('%s: seed must be an integer in 0 .. 2^64 - 1, got %r' % (what, seed))
    s = _device(s)
    d = d.to(s.device).contiguous()
    c = _correspondences(corr, s.device, what)
    m, H = c.shape[0], int(hypotheses)
    size = lib().mvsdf_greg_ransac_workspace_bytes(m, H)
    ws = torch.empty(size, dtype=torch.uint8, device=s.device)
    mask = torch.empty(m, dtype=torch.uint8, device=s.device)
    check(lib().mvsdf_greg_ransac(_vp(s), s.shape[0], _vp(d), d.shape[0], _vp(c), m, H, int(seed), edge_ratio, max_dist, _vp(ws), size, _vp(mask),
                                  _stream(s)), 'mvsdf_greg_ransac')
    h = _header(ws, K.MVSDF_GREG_RANSAC_H_WORDS)
    raise_for_bits(h[K.MVSDF_GREG_RANSAC_H_ERR], what, ERRORS)
    T = np.eye(4)
    T[:3, :] = np.array([f64_from_bits(b) for b in h[K.MVSDF_GREG_RANSAC_H_T:K.MVSDF_GREG_RANSAC_H_WORDS]], dtype=np.float64).reshape(3, 4)
    return GlobalRegistration(T, h[K.MVSDF_GREG_RANSAC_H_INLIERS], h[K.MVSDF_GREG_RANSAC_H_HYP], h[K.MVSDF_GREG_RANSAC_H_CHECKED], mask.bool())


def _describe(points, given, voxel, k, radius, what, name):
    """downsample, normals, rows, descriptor -> (points fp64 [n,3], codes int8 [n,33]) on the device"""
    p = _device(_points(points, what))
    ds = _reg.voxel_downsample(p, voxel)[0].contiguous()
    if given is None:
        nrm, _, nb = _normals.estimate_normals(ds, k)
        nrm = _normals.orient_normals(ds, nrm, nb).normals
    else:
        g = _points(given, what)
        if g.shape[0] != p.shape[0]:
            raise ValueError('%s: %s_normals must be [N, 3] for N = %d points, got shape %s' % (what, name, p.shape[0], tuple(g.shape)))
        _, index = _reg.NearestTree(p).query(ds)
        nrm = g.to(p.device)[index.long()].contiguous()
        nb = _normals.knn_indices(ds, k)
    hist, count = spfh(ds, nrm, nb, radius)
    return ds, fpfh(ds, nb, hist, count, radius)[1]


def global_register(source, target, voxel, source_normals=None, target_normals=None, k=32, feature_radius=None, max_dist=None, hypotheses=100000,
                    seed=0, mutual=False, flip='auto', refine=True, return_search=False):
    """definition 5 -> GlobalResult(transformation fp64 numpy [4,4] source -> target, inliers, flipped, fitness, inlier_rmse); the last two are ICP's
    and None without refine.  return_search: (GlobalResult, the winning run's GlobalRegistration) instead."""
    what = 'global_register'
    voxel = float(voxel)
    if not (voxel > 0 and math.isfinite(voxel)):
        raise ValueError('%s: voxel must be a positive finite number, got %r' % (what, voxel))
    if flip not in ('auto', True, False):
        raise ValueError("%s: flip must be 'auto', True or False, got %r" % (what, flip))
    radius = 5 * voxel if feature_radius is None else feature_radius
    max_dist = 1.5 * voxel if max_dist is None else max_dist
    s, sc = _describe(source, source_normals, voxel, k, radius, what, 'source')
    t, tc = _describe(target, target_normals, voxel, k, radius, what, 'target')
    best = None
    for mirrored in ((False, True) if flip == 'auto' else (bool(flip),)):
        index, _ = match_features(mirror_codes(sc) if mirrored else sc, tc, mutual)
        if int((index >= 0).sum()) < 3:
            continue
        reg = ransac(s, t, index, max_dist, hypotheses, seed)
        if best is None or reg.inliers > best[0].inliers:
            best = (reg, mirrored)
    if best is None:
        raise ValueError('%s: fewer than 3 correspondences' % what)
    reg, flipped = best
    if refine:
        r = _reg.icp(s, _reg.NearestTree(t), reg.transformation, max_dist)
        out = GlobalResult(r.transformation, reg.inliers, flipped, r.fitness, r.inlier_rmse)
    else:
        out = GlobalResult(reg.transformation, reg.inliers, flipped, None, None)
    return (out, reg) if return_search else out
