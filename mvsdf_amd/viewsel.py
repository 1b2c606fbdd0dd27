"""View selection on the device: the pairwise view score behind MVSNet-style pair.txt files, the per-view depth ranges of the camera files, and
the pair lists chosen from them -- what the reference's BYOD.md supposes to exist.  The points and tracks it reads come from a COLMAP model, or,
for posed images without one, from keypoints.py (keypoints, matching, verification, tracks and triangulation: keypoints.sparse_points, or
tools/sparse_points.py, which also writes pair.txt and the camera files).  Kernels: csrc/viewsel.hip (the design: DESIGN.md); tests/viewsel_ref.py restates every step in numpy.  The score is the well-known one of
MVSNet's colmap2mvsnet.py (a Gaussian of the triangulation angle, summed over the common points); that script's text is not available to this
project and the reference has no counterpart, so the definition below is this project's own statement of it and no agreement beyond the formula
is claimed.

Inputs: points fp64 [P,3]; centers fp64 [V,3] (raster.camera_centers for P matrices, centers_from_cams for cams [V,2,4,4]); visibility either
uint8 / bool [V,P] (as raster.vertex_visibility returns it) or tracks in CSR form, track_off int64 [P+1] and track_view int32 [track_off[P]],
where a view listed twice in a track counts once.  Either form is packed on the device into one bit matrix uint64 [P, ceil(V/64)], which is
what the score kernel reads.

The definition (fp64 throughout, in the order written, no FMA contraction):

- Unit vectors.  For view v and point p: d = c_v - p (per component), n = sqrt((d0*d0 + d1*d1) + d2*d2), u = (d0/n, d1/n, d2/n) if 0 < n <= the
  largest finite double, else (0, 0, 0) (a point that coincides with the centre, or a distance whose square under- or overflows).  Normalising
  first does not change the angle, lets the kernel compute a point's unit vectors once per tile, and keeps the products below in [-1, 1].
- Angle of the pair (i, j), i < j, at p, with a = u_i, b = u_j: cross = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0);
  nc = sqrt((cross0*cross0 + cross1*cross1) + cross2*cross2); dt = (a0*b0 + a1*b1) + a2*b2; theta = (180/pi) * atan2(nc, dt) with
  atan2(0, 0) = 0 and 180/pi = 57.29577951308232.  (Swapping a and b negates the cross product exactly, so theta is symmetric bit for bit.)
- atan2 and exp are NOT library calls (ocml and the host libm disagree in the last bits): they are written out in csrc/det_math64.h from + - * /,
  compares and bit casts.  atan2(y >= 0, x): z = min(y, |x|) / max(y, |x|); if z > tan(pi/8): z = (z - 1)/(z + 1), base pi/4; atan(z) = z * (1 -
  z^2/3 + ... + z^38/39), Horner in z*z from the highest term down, each step p = p*z2 + c; r = base + z*p; r = pi/2 - r where y > |x|; r = pi - r
  where x < 0.  exp(x <= 0): x is clamped at -708; n = rint(x * log2(e)) (by adding and subtracting 1.5 * 2^52); r = (x - n*LN2_HI) - n*LN2_LO;
  exp(r) = 1 + r + ... + r^14/14! by Horner from the highest term down; n is added to the exponent field.  tests/viewsel_ref.py carries both,
  operation for operation.
- Weight: d = theta - theta0; s = sigma1 if theta <= theta0 else sigma2; q = (d*d) / (2*(s*s)); w = exp(-q).  Defaults theta0 = 5, sigma1 = 1,
  sigma2 = 10.  Quantised: wq = int64(rint(w * 2^32)) (ties to even).
- S[i,j] = the sum of wq over the points both views see, a 64-bit integer sum: exact and associative, so the schedule cannot change it (the idea
  of the rasteriser's integer depth buffer).  scores[i,j] = fp64(S[i,j]) * 2^-32; symmetric, the diagonal is 0.
- counts[i,j] int64 = the number of points both views see; counts[i,i] = the number of points view i sees.
- The written-out w stays within 2^-33 (half a quantum) of np.exp / np.arctan2 (tests/test_viewsel_host.py; the measured maximum: DESIGN.md), so
  wq is at most one quantum from a libm-based value.

select_pairs: for view i the views j != i with counts[i,j] > 0, by score descending then index ascending, the first num_pairs of them.  MVSNet's
script also lists pairs that share no point (with score 0); here they are left out, so a view may get fewer than num_pairs sources, or none.

depth_ranges: per view the camera depths z = ((r20*x + r21*y) + r22*z) + t2 (row 2 of the extrinsic) of the points it sees, sorted ascending;
depth_min = z[int(n*lo)], depth_max = z[int(n*hi)], n their number.

Non-finite points, centres or extrinsics, a track view outside [0, V), V < 1 and P >= 2^31 raise ValueError; the device-side checks travel as
error bits in a header that is read once per call.  P = 0 is valid: zero scores, zero counts, empty pair lists.
"""
import ctypes

import numpy as np
import torch

from ._lib import check, K, lib, raise_for_bits, _header, _stream, _vp

MAX_VIEWS = K.MVSDF_VS_MAX_VIEWS
INT32_MAX = 2 ** 31 - 1
DEPTH_CHUNK = 1 << 25                                # fp64 depths held at once by depth_ranges (256 MiB)


# the error bits of a viewsel call (csrc/viewsel.hip), in the order they are looked at
ERRORS = [(K.MVSDF_VS_ERR_FINITE, ValueError, 'a point, a centre or an extrinsic entry is NaN or infinite'),
          (K.MVSDF_VS_ERR_TRACK, ValueError, 'a track view is outside [0, V) (or the track offsets do not ascend within the view list)'),
          (K.MVSDF_VS_ERR_SHAPE, ValueError, 'V must be in [1, %d] and P below 2^31' % MAX_VIEWS)]


def _params(theta0, sigma1, sigma2, what):
    theta0, sigma1, sigma2 = float(theta0), float(sigma1), float(sigma2)
    if not np.isfinite([theta0, sigma1, sigma2]).all() or sigma1 <= 0 or sigma2 <= 0:
        raise ValueError('%s: theta0 must be finite, sigma1 and sigma2 finite and > 0, got %r, %r, %r' % (what, theta0, sigma1, sigma2))
    return theta0, sigma1, sigma2


def _device(*xs):
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    return torch.device('cuda')


def _points(points, what):
    p = torch.as_tensor(points)
    if p.dim() != 2 or p.shape[1] != 3:
        raise ValueError('%s: points must be [P, 3], got shape %s' % (what, tuple(p.shape)))
    if p.shape[0] > INT32_MAX:
        raise ValueError('%s: %d points (P must be below 2^31)' % (what, p.shape[0]))
    return p


def _rows(x, width, name, what):
    c = torch.as_tensor(x)
    if c.dim() != 2 or c.shape[1] != width:
        raise ValueError('%s: %s must be [V, %d], got shape %s' % (what, name, width, tuple(c.shape)))
    if not 1 <= c.shape[0] <= MAX_VIEWS:
        raise ValueError('%s: V must be in [1, %d], got %d' % (what, MAX_VIEWS, c.shape[0]))
    return c


def _f64(t, dev):
    return t.to(dev, torch.float64).contiguous()


def pack_visibility(visibility, V, P, device=None):
    """Either visibility form -> (bits, hdr): the bit matrix int64 [P, ceil(V/64)] (the uint64 words, bit v mod 64 of word v // 64) and the 256-byte
    device header whose error bits the caller reads.  visibility: uint8 / bool [V, P], or the tuple (track_off int64 [P+1], track_view int32 [nnz])."""
    what = 'pack_visibility'
    if not 1 <= V <= MAX_VIEWS or not 0 <= P <= INT32_MAX:
        raise ValueError('%s: V must be in [1, %d] and P below 2^31, got V = %d, P = %d' % (what, MAX_VIEWS, V, P))
    L = lib()
    tracks = isinstance(visibility, tuple)
    if tracks and len(visibility) != 2:
        raise ValueError('%s: tracks are the tuple (track_off, track_view)' % what)
    if tracks:
        off, view = torch.as_tensor(visibility[0]), torch.as_tensor(visibility[1])
        dev = device or _device(off, view)
        if off.shape != (P + 1,) or view.dim() != 1 or off.is_floating_point() or view.is_floating_point():
            raise ValueError('%s: tracks must be (track_off int64 [P + 1] = [%d], track_view int32 [nnz]), got shapes %s, %s' %
                             (what, P + 1, tuple(off.shape), tuple(view.shape)))
        off, view = off.to(dev, torch.int64).contiguous(), view.to(dev, torch.int32).contiguous()
    else:
        vis = torch.as_tensor(visibility)
        dev = device or _device(vis)
        if tuple(vis.shape) != (V, P) or vis.dtype not in (torch.uint8, torch.bool):
            raise ValueError('%s: visibility must be uint8 or bool [V, P] = %s, got %s %s' % (what, (V, P), vis.dtype, tuple(vis.shape)))
        vis = vis.to(dev).contiguous().view(torch.uint8)
    nw = (V + 63) // 64
    bits = torch.empty(P, nw, dtype=torch.int64, device=dev)
    hdr = torch.empty(256, dtype=torch.uint8, device=dev)
    if tracks:
        check(L.mvsdf_viewsel_pack_tracks(_vp(off), _vp(view) if view.numel() else None, view.numel(), V, P, _vp(bits) if P else None, _vp(hdr), _stream(hdr)),
              'mvsdf_viewsel_pack_tracks')
    else:
        check(L.mvsdf_viewsel_pack_dense(_vp(vis) if P else None, V, P, _vp(bits) if P else None, _vp(hdr), _stream(hdr)), 'mvsdf_viewsel_pack_dense')
    return bits, hdr


def view_scores(points, centers, visibility, theta0=5.0, sigma1=1.0, sigma2=10.0):
    """The module's definition -> (scores fp64 [V,V], counts int64 [V,V]) on the device.  visibility: uint8 / bool [V,P], or the tracks
    (track_off, track_view).  Device tensors are used where they are; numpy / CPU input is copied to the GPU."""
    what = 'view_scores'
    theta0, sigma1, sigma2 = _params(theta0, sigma1, sigma2, what)
    dev = _device(points, centers, *(visibility if isinstance(visibility, tuple) else (visibility,)))
    pts, ctr = _points(points, what), _rows(centers, 3, 'centers', what)             # every shape is checked before the GPU is touched
    pts, ctr = _f64(pts, dev), _f64(ctr, dev)
    V, P = ctr.shape[0], pts.shape[0]
    bits, hdr = pack_visibility(visibility, V, P, dev)
    size = lib().mvsdf_viewsel_workspace_bytes(V)
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    scores = torch.empty(V, V, dtype=torch.float64, device=dev)
    counts = torch.empty(V, V, dtype=torch.int64, device=dev)
    check(lib().mvsdf_viewsel_scores(_vp(pts) if P else None, _vp(ctr), _vp(bits) if P else None, V, P, theta0, sigma1, sigma2, _vp(ws), size, _vp(scores),
                                     _vp(counts), _vp(hdr), _stream(hdr)), 'mvsdf_viewsel_scores')
    raise_for_bits(_header(hdr, K.MVSDF_RES_H_WORDS)[K.MVSDF_RES_H_ERR], what, ERRORS)   # the one wait of the call
    return scores, counts


def weights_host(a, b, theta0=5.0, sigma1=1.0, sigma2=10.0):
    """The definition's (theta fp64 [n], wq int64 [n]) for vectors a = c_i - p and b = c_j - p (fp64 [n,3]) on the CPU, by the very functions the
    kernel runs (csrc/det_math64.h and viewsel.hip's host side); needs no GPU."""
    theta0, sigma1, sigma2 = _params(theta0, sigma1, sigma2, 'weights_host')
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.ndim != 2 or a.shape[1] != 3 or a.shape != b.shape:
        raise ValueError('weights_host: a and b must both be [n, 3], got shapes %s, %s' % (a.shape, b.shape))
    theta, wq = np.empty(len(a), np.float64), np.empty(len(a), np.int64)
    vp = ctypes.c_void_p
    check(lib().mvsdf_viewsel_weights_host(vp(a.ctypes.data), vp(b.ctypes.data), len(a), theta0, sigma1, sigma2, vp(theta.ctypes.data),
                                           vp(wq.ctypes.data)), 'mvsdf_viewsel_weights_host')
    return theta, wq


def centers_from_cams(cams):
    """cams [V,2,4,4] (utils.io.load_cam) or extrinsics [V,4,4] -> the camera centres -R^T t, fp64 numpy [V,3]"""
    E = np.asarray(cams, dtype=np.float64)
    if E.ndim == 4:
        E = E[:, 0]
    if E.ndim != 3 or E.shape[1:] != (4, 4):
        raise ValueError('centers_from_cams: cams must be [V, 2, 4, 4] or [V, 4, 4], got shape %s' % (E.shape,))
    return np.stack([-(e[:3, :3].T @ e[:3, 3]) for e in E]) if len(E) else np.zeros((0, 3))


def select_pairs(scores, counts, num_pairs=10):
    """-> (pairs, pair_scores): per view i the views j != i with counts[i,j] > 0, by score descending then index ascending, the first num_pairs; pairs
    is a list of lists of view indices (what plane_sweep and fuse_depths take), pair_scores the scores beside them."""
    s = np.asarray(scores.cpu() if isinstance(scores, torch.Tensor) else scores, dtype=np.float64)
    c = np.asarray(counts.cpu() if isinstance(counts, torch.Tensor) else counts)
    if s.ndim != 2 or s.shape[0] != s.shape[1] or c.shape != s.shape:
        raise ValueError('select_pairs: scores and counts must both be [V, V], got shapes %s, %s' % (s.shape, c.shape))
    num_pairs = int(num_pairs)
    if num_pairs < 0:
        raise ValueError('select_pairs: num_pairs must be >= 0')
    pairs, pair_scores = [], []
    for i in range(len(s)):
        cand = np.flatnonzero((c[i] > 0) & (np.arange(len(s)) != i))
        order = cand[np.argsort(-s[i, cand], kind='stable')][:num_pairs]    # stable: equal scores stay in index order
        pairs.append([int(j) for j in order])
        pair_scores.append([float(s[i, j]) for j in order])
    return pairs, pair_scores


def _quantile_index(n, q):
    """int(n * q) for an int64 tensor n of counts: the fp64 product, truncated (always below n for q < 1 and n >= 1)"""
    return (n.to(torch.float64) * q).to(torch.int64)


def depth_ranges(points, visibility, extrinsics, lo=0.01, hi=0.99):
    """The module's depth ranges -> fp64 numpy-style tensor [V,2] (depth_min, depth_max) on the device.  extrinsics: fp64 [V,4,4] world -> camera
    (cams[:, 0]); visibility as for view_scores.  A view that sees no point raises ValueError naming it."""
    what = 'depth_ranges'
    lo, hi = float(lo), float(hi)
    if not 0 <= lo <= hi < 1:
        raise ValueError('%s: 0 <= lo <= hi < 1 is needed, got %r, %r' % (what, lo, hi))
    E = torch.as_tensor(extrinsics)
    if E.dim() != 3 or tuple(E.shape[1:]) != (4, 4):
        raise ValueError('%s: extrinsics must be [V, 4, 4], got shape %s' % (what, tuple(E.shape)))
    dev = _device(points, E, *(visibility if isinstance(visibility, tuple) else (visibility,)))
    pts, row2 = _points(points, what), _rows(E[:, 2, :], 4, 'extrinsics[:, 2]', what)
    pts, row2 = _f64(pts, dev), _f64(row2, dev)
    V, P = row2.shape[0], pts.shape[0]
    bits, hdr = pack_visibility(visibility, V, P, dev)
    if P == 0:
        raise_for_bits(_header(hdr, K.MVSDF_RES_H_WORDS)[K.MVSDF_RES_H_ERR], what, ERRORS)
        raise ValueError('%s: view 0 sees no point' % what)
    out = torch.empty(V, 2, dtype=torch.float64, device=dev)
    seen = torch.empty(V, dtype=torch.int64, device=dev)
    chunk = max(1, min(V, DEPTH_CHUNK // P))
    z = torch.empty(chunk, P, dtype=torch.float64, device=dev)
    for v0 in range(0, V, chunk):
        nv = min(chunk, V - v0)
        check(lib().mvsdf_viewsel_depths(_vp(pts), _vp(bits) if P else None, _vp(row2), V, P, v0, nv, _vp(z), _vp(hdr), _stream(hdr)), 'mvsdf_viewsel_depths')
        zs = torch.sort(z[:nv], dim=1).values                               # unseen points are +inf: they sort to the end
        n = torch.isfinite(zs).sum(1)
        seen[v0:v0 + nv] = n
        i0, i1 = _quantile_index(n, lo), _quantile_index(n, hi)
        out[v0:v0 + nv, 0] = zs.gather(1, i0.clamp(max=P - 1).unsqueeze(1)).squeeze(1)
        out[v0:v0 + nv, 1] = zs.gather(1, i1.clamp(max=P - 1).unsqueeze(1)).squeeze(1)
    raise_for_bits(_header(hdr, K.MVSDF_RES_H_WORDS)[K.MVSDF_RES_H_ERR], what, ERRORS)   # the one wait of the call
    empty = torch.nonzero(seen == 0).flatten().cpu()
    if len(empty):
        raise ValueError('%s: view %d sees no point' % (what, int(empty[0])))
    return out


def write_pair(path, ids, pairs, pair_scores):
    """pair.txt in the layout utils.io.load_pair reads: the number of views, then per view its id and `n id_0 score_0 id_1 score_1 ...`.  ids: one
    name per view (written as given); pairs / pair_scores as select_pairs returns them (view indices).  Scores are written with %.17g."""
    if not (len(ids) == len(pairs) == len(pair_scores)):
        raise ValueError('write_pair: ids, pairs and pair_scores must have one entry per view, got %d, %d, %d' % (len(ids), len(pairs), len(pair_scores)))
    lines = ['%d' % len(ids)]
    for vid, q, sc in zip(ids, pairs, pair_scores):
        if len(q) != len(sc):
            raise ValueError('write_pair: view %s has %d sources and %d scores' % (vid, len(q), len(sc)))
        if any(j < 0 or j >= len(ids) for j in q):
            raise ValueError('write_pair: view %s has a source outside [0, %d)' % (vid, len(ids)))
        lines.append(str(vid))
        lines.append(' '.join(['%d' % len(q)] + ['%s %.17g' % (ids[j], x) for j, x in zip(q, sc)]))
    with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
