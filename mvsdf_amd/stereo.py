"""Plane-sweep stereo on the device: the step the reference's BYOD.md calls "Run VisMVSNet" (a depth map and three probability maps per view), as a
classical sweep over descriptor maps.  Vis-MVSNet's cost-volume network and its weights are not part of the reference tree, so this is NOT
Vis-MVSNet: the three maps written here are confidences of a plane sweep, not Vis-MVSNet's probabilities, and BYOD.md's thresholds .8,.7,.8 do not
suit them (the thresholds that do, chosen on the test scene: PTHRESH below and DESIGN.md).  What they share is the file layout, so
prepare.load_mvs_output, tools/fusion.py and tools/vismvsnet2mvsdf.py read the output as they are.  Kernels: csrc/stereo.hip (the design:
DESIGN.md); tests/stereo_ref.py restates every step in numpy.

Inputs: feats fp32 [V,R,S,C] channels-last (features.extract_features(...).permute(0, 2, 3, 1), or patch_descriptors), any C >= 1; cams fp64
[V,2,4,4] at feature-map scale as utils.io.load_cam / scale_camera return them, row 3 of cams[v,1] = depth_min, interval, number of hypotheses D,
depth_max; pairs a list of V lists of view indices (nearest first), of which the first num_src are used.

The definition (fp64 throughout, in the order written, no FMA contraction; fp32 inputs are promoted exactly):

- Descriptors (normalize_descriptors).  n = sqrt(f_0*f_0 + f_1*f_1 + ...) summed in channel order from 0; f^_c = fp32(f_c / n) where n > 0, else 0.
  The descriptor is rounded to fp32 and stored, so a texel of 32 channels is one 128-byte line.  plane_sweep takes descriptors as they are given.
- Hypotheses of reference view r: d_k = depth_min + k*interval, k = 0..D-1, from cams[r,1,3].
- Matrices, pixel convention and the row product are fusion.py's: P_v = K4_v @ E_v, T_rs = P_s @ inv(P_r) (numpy fp64 on the host); pixel (x, y) sits
  at X = x + 0.5, Y = y + 0.5; a matrix row times q is ((t0*q0 + t1*q1) + t2*q2) + t3*q3.
- Score of source s at (x, y, k), d = d_k: p = T_rs (X*d, Y*d, d, 1); the source is valid iff p2 > 0 and, with u = p0/p2 - 0.5, v = p1/p2 - 0.5,
  0 <= u <= S-1 and 0 <= v <= R-1.  x0 = min(floor(u), S-2), y0 = min(floor(v), R-2), fx = u - x0, fy = v - y0;
  t_ij = f^_r[0]*f^_s[y0+i, x0+j][0] + f^_r[1]*f^_s[y0+i, x0+j][1] + ... (from the first product on, in channel order);
  c_s = (t00*(1-fx) + t01*fx)*(1-fy) + (t10*(1-fx) + t11*fx)*fy.
- Aggregate: n_k = the number of valid sources; score_k = (0 + c_s1 + c_s2 + ..., valid sources in pair order) / n_k where n_k >= 1; otherwise the
  hypothesis is invalid (NaN in the score volume).
- Winner: k* = the valid k of greatest score, compared with a strict > from minus infinity on, so the lowest k wins a tie.  No valid k: depth and
  the three confidences are 0, best_k = -1, counts = 0.
- Refinement, only where 0 < k* < D-1 and k*-1 and k*+1 are valid: a, b, c = score[k*-1], score[k*], score[k*+1], den = (a - 2*b) + c,
  off = (0.5*(a - c))/den if den < 0, else 0 (also wherever there is no refinement).  depth = fp32(depth_min + (k* + off)*interval).
- Confidences, fp32 in [0, 1]: prob1 = min(max(b, 0), 1).  prob2 = 0 if b <= 0, else min(max(1 - max(b2, 0)/b, 0), 1) with b2 the greatest score
  over the valid k with |k - k*| >= 2, and 1 where there is no such k.  prob3 = n_k* / (the number of sources used for r = min(num_src,
  len(pairs[r]))).  counts holds n_k*.
- Regularisation (regularize_scores; plane_sweep(regularize=...), off by default): semi-global aggregation of the score volume (SGM,
  Hirschmueller), between the aggregate and the winner.  Input: score[k][y][x], fp64 [D,R,S], NaN where the hypothesis is invalid, every other entry
  finite; the penalties P1, P2 and the number of paths.
  Cost: C(p,k) = 1 - score[k][p] where valid; an invalid entry takes no part in any minimum.
  Directions (dy, dx), in this order: (0,1), (0,-1), (1,0), (-1,0), (1,1), (-1,-1), (1,-1), (-1,1); paths = 4 uses the first four, paths = 8 all.
  Path cost along direction r, with q = p - r: L_r(p,k) is invalid where C(p,k) is.  Otherwise, if q is outside the image or no k is valid at q,
  L_r(p,k) = C(p,k) (the path restarts there).  Otherwise m = the minimum of L_r(q,j) over the valid j,
  best = min(L_r(q,k), L_r(q,k-1) + P1, L_r(q,k+1) + P1, m + P2) over those of the four terms that exist and are valid, and
  L_r(p,k) = C(p,k) + (best - m).
  Sum: T(p,k) = ((L_1 + L_2) + L_3) + ... in direction order, from the first term on.  Regularised score: A(p,k) = 1 - T(p,k)/paths (the division
  by 4 or 8 is exact); A is NaN where C is invalid.
  Winner, refinement and prob2 are the ones above applied to A unchanged (b, a, c and b2 are A's values).  prob1 stays the clamped RAW score at the
  new k*, so a threshold on it keeps its meaning; prob3 and counts stay n_k*.
  P1 and P2 are finite with 0 <= P1 <= P2, paths is 4 or 8 and D <= MAX_D_SGM = 4096 (one path's previous-step costs, held twice, are then 64 KB
  of the CU's 160 KB of LDS); otherwise, and for an infinite score, ValueError.  Every minimum is exact and every sum is one lane's own in a fixed
  order, so the result does not depend on the schedule.  tests/stereo_sgm_ref.py restates it in numpy.
- patch_descriptors: grey = (299 R + 587 G + 114 B)/1000; the (2 radius + 1)^2 grey values around the pixel, rows then columns, coordinates clamped
  to the image; mean = (0 + g_0 + g_1 + ...)/(2 radius + 1)^2; channel i = fp32(g_i - mean).

Non-finite features or cameras, R or S below 2, D < 1 and a pair index outside [0, V) raise ValueError.

Cascade (cascade_sweep, off by default; estimate_scene(cascade=...)): Vis-MVSNet's model_cas sweeps coarse to fine, 64 hypotheses over the whole
range at 1/8 of the image size, then 32 and 16 around the upsampled previous depth at 1/4 and 1/2.  The same here, fp64 in the order written:

- Stages: L of them, 1 <= L <= MAX_STAGES = 4.  Stage l has a descriptor map desc_l fp32 [V,R_l,S_l,C_l], R_l and S_l >= 2, any C_l >= 1, used as
  given; the sizes of different stages need not be in integer ratio.
- Cameras: cams fp64 [V,2,4,4] is at the size of the last stage; the camera of stage l is scale_camera(cams, (S_l/S_L, R_l/R_L)).  Matrices, pixel
  convention and row product are the sweep's.
- Hypotheses: interval and D come from cams[r,1,3].  interval_scales = (g_1..g_L), finite and positive, default (4, 2, 1) for L = 3;
  depth_nums = (D_1..D_L), default (None, 32, 16); None is allowed for D_1 only and means ceil(D/g_1) (64 at max_d 256).  step_l = interval*g_l.
- Stage 1 is the sweep above of desc_1 with the stage-1 cameras, depth_min, interval step_1 and D_1 hypotheses.  regularize= applies to this stage
  only: it is the only one whose hypotheses are shared between pixels, which the path penalties presuppose.
- Centres (upsample_depth), for stage l > 1, at pixel (x, y), from the previous stage's depth and best_k of size r x s:
  u = ((x + 0.5)*s)/S_l - 0.5 clamped to [0, s-1], v likewise with r and R_l; x0 = min(floor(u), s-2), y0 = min(floor(v), r-2), fx = u - x0,
  fy = v - y0.  The taps (dy, dx) = (0,0), (0,1), (1,0), (1,1), in this order, have the weights (1-fx)*(1-fy), fx*(1-fy), (1-fx)*fy, fx*fy; a tap is
  valid iff its best_k >= 0.  num = ((0 + w*d) + ...) and den = ((0 + w) + ...) over the valid taps in that order, d the fp32 depth promoted.  The
  centre is num/den where den > 0, otherwise NaN: no centre.
- Band sweep (band_sweep): given centres fp64 [V,R,S] (NaN: none), D_b >= 1 and step > 0, the hypotheses of pixel p are
  d_k = c_p + (k - floor(D_b/2))*step, k = 0..D_b-1.  A hypothesis is invalid for every source if its pixel has no centre or d_k <= 0.  Otherwise
  score, validity, aggregate, winner, refinement, the three confidences and counts are the sweep's, word for word, over the D_b hypotheses of the
  band; best_k is the index within the band and depth = fp32(c_p + ((k* - floor(D_b/2)) + off)*step).  No valid k: depth and the confidences are
  0, best_k = -1, counts = 0.  D_b <= MAX_D_BAND = 64 (a tile's scores and counts stay in LDS; no score volume is written).
- Result (cascade_sweep): stages[l] is a Sweep at stage l's size.  The final maps, at stage L's size: depths, best_k and counts are stage L's;
  probs[0] and probs[2] are stage L's prob1 and prob3; probs[1] is stage 1's prob2 at the coarse pixel (((2y+1)*R_1)//(2*R_L),
  ((2x+1)*S_1)//(2*S_L)) in integer arithmetic, and 0 where stage L has no winner: the full-range peak ratio is the distinctiveness PTHRESH's second
  threshold was chosen for; inside a 16-step band it means little.  With L = 1 and g_1 = 1 the result is plane_sweep's, bit for bit.
- ValueError, before the GPU is touched: L outside [1, 4]; tuples of the wrong length; a None elsewhere than in D_1; D_b outside [1, MAX_D_BAND]; a
  non-finite or non-positive scale or step; V differing between stages; centres of the wrong shape; infinite centres (NaN is allowed; in a device
  tensor they are found by the kernel); a view listed twice where a band is swept (every view of a band is swept by the one launch, and every
  output has one writer); the sweep's conditions at every stage.  tests/stereo_cascade_ref.py restates all of it in numpy.

Not built: Vis-MVSNet's learned regularisation (the semi-global aggregation above stands in for it), visibility-weighted aggregation,
regularisation of the bands of stages 2 and up.
"""
import os

import numpy as np
import torch

from ._lib import check, K, lib, raise_for_bits, _header, _stream, _vp
from .fusion import projection_matrices

PTHRESH = (0.7, 0.02, 0.9)        # thresholds on prob1, prob2, prob3 that suit these confidences (chosen on tests/stereo_scene.py: DESIGN.md)
MAX_SRC, MAX_D = K.MVSDF_PS_MAX_SRC, K.MVSDF_PS_MAX_D
MAX_D_SGM = K.MVSDF_PS_MAX_D_SGM    # the most hypotheses regularize_scores takes
MAX_D_BAND = K.MVSDF_PS_MAX_D_BAND  # the most hypotheses of a band (band_sweep): the tile's scores and counts are then 36 KB of LDS
MAX_STAGES = 4                    # of a cascade
CASCADE_DEFAULTS = ((None, 32, 16), (4, 2, 1))      # depth_nums, interval_scales: Vis-MVSNet's 64 / 32 / 16 at max_d 256
SGM_DEFAULTS = (0.1, 0.8, 8)      # P1, P2, paths (chosen on the noisy test scene: DESIGN.md)


class Sweep:
    """The result of plane_sweep: depths fp32 [V,R,S], probs fp32 [V,3,R,S], best_k int32 [V,R,S] (-1: no valid hypothesis), counts int32 [V,R,S]
    (n_k*), all on the device and zero (best_k -1) for views that were not swept; scores: fp64 [D,R,S] of the last view swept (NaN where a
    hypothesis is invalid) or None; reg_scores: that view's regularised scores A where the sweep regularised and scores were asked for, else None."""

    def __init__(self, depths, probs, best_k, counts, scores=None, reg_scores=None):
        self.depths, self.probs, self.best_k, self.counts, self.scores, self.reg_scores = depths, probs, best_k, counts, scores, reg_scores


# the error bits of a stereo call (csrc/stereo.hip), in the order they are looked at
ERRORS = [(K.MVSDF_PS_ERR_FINITE, ValueError, 'a feature or a camera entry is NaN or infinite'),
          (K.MVSDF_PS_ERR_PAIR, ValueError, 'a pair or view index is outside [0, V)'),
          (K.MVSDF_PS_ERR_DEPTHS, ValueError, 'the number of depth hypotheses must be in [1, %d]' % MAX_D),
          (K.MVSDF_PS_ERR_SHAPE, ValueError, 'shapes disagree or are out of range (V >= 1, R and S >= 2, C >= 1, at most %d sources)' % MAX_SRC),
          (K.MVSDF_PS_ERR_SGM, ValueError, 'the regularisation needs finite 0 <= P1 <= P2, paths 4 or 8 and at most %d hypotheses' % MAX_D_SGM),
          (K.MVSDF_PS_ERR_BAND, ValueError, 'a band needs 1 to %d hypotheses, finite positive steps and every view at most once' % MAX_D_BAND),
          (K.MVSDF_PS_ERR_CENTRE, ValueError, 'a centre is infinite')]


def _checked_features(feats, what):
    """-> feats as a tensor [V,R,S,C] where it is; host input is checked for finiteness here.  Touches no GPU."""
    f = torch.as_tensor(feats)
    if f.dim() != 4:
        raise ValueError('%s: features must be [V, R, S, C], got shape %s' % (what, tuple(f.shape)))
    V, R, S, C = f.shape
    if V < 1 or R < 2 or S < 2 or C < 1:
        raise ValueError('%s: features must be at least 2 x 2 texels of one channel (and V >= 1), got shape %s' % (what, tuple(f.shape)))
    if not f.is_cuda and not bool(torch.isfinite(f).all()):
        raise ValueError('%s: a feature is NaN or infinite' % what)
    return f


def _feature_tensor(feats, what):
    """-> (fp32 contiguous device tensor [V,R,S,C], device); host input is checked for finiteness here, before the GPU is touched"""
    f = _checked_features(feats, what)
    dev = f.device if f.is_cuda else torch.device('cuda')
    return f.to(dev, torch.float32).contiguous(), dev


def normalize_descriptors(feats):
    """feats [V,R,S,C] -> the definition's unit descriptors, fp32 [V,R,S,C] on the device"""
    what = 'normalize_descriptors'
    f, dev = _feature_tensor(feats, what)
    out = torch.empty_like(f)
    hdr = torch.empty(K.MVSDF_RES_H_WORDS, dtype=torch.int64, device=dev)
    check(lib().mvsdf_stereo_normalize(_vp(f), f.numel() // f.shape[3], f.shape[3], _vp(out), _vp(hdr), _stream(f)), 'mvsdf_stereo_normalize')
    raise_for_bits(int(hdr.cpu()[K.MVSDF_RES_H_ERR]), what, ERRORS)
    return out


def patch_descriptors(images_u8, radius=2):
    """images uint8 [V,H,W,3] -> the definition's mean-free grey patches, fp32 [V,H,W,(2 radius + 1)^2] on the device (not normalised)"""
    what = 'patch_descriptors'
    img = torch.as_tensor(images_u8)
    if img.dim() != 4 or img.shape[3] != 3 or img.dtype != torch.uint8 or min(img.shape[:3]) < 1:
        raise ValueError('%s: images must be uint8 [V, H, W, 3], got %s %s' % (what, img.dtype, tuple(img.shape)))
    radius = int(radius)
    if radius < 0 or radius > 15:
        raise ValueError('%s: radius must be in [0, 15], got %d' % (what, radius))
    img = img.to(img.device if img.is_cuda else torch.device('cuda')).contiguous()
    V, H, W, _ = img.shape
    out = torch.empty(V, H, W, (2 * radius + 1) ** 2, dtype=torch.float32, device=img.device)
    check(lib().mvsdf_stereo_patches(_vp(img), V, H, W, radius, _vp(out), _stream(img)), 'mvsdf_stereo_patches')
    return out


def _sgm_args(regularize, what):
    """None -> None; True -> the defaults; (p1, p2) or (p1, p2, paths) -> (p1, p2, paths), checked"""
    if regularize is None or regularize is False:
        return None
    if regularize is True:
        return SGM_DEFAULTS
    try:
        r = tuple(regularize)
    except TypeError:
        r = ()
    if len(r) not in (2, 3):
        raise ValueError('%s: regularize must be None, True, (p1, p2) or (p1, p2, paths), got %r' % (what, regularize))
    return _sgm_checked(r[0], r[1], r[2] if len(r) == 3 else SGM_DEFAULTS[2], what)


def _sgm_checked(p1, p2, paths, what):
    p1, p2 = float(p1), float(p2)
    if not (np.isfinite(p1) and np.isfinite(p2) and 0.0 <= p1 <= p2):
        raise ValueError('%s: the penalties must be finite with 0 <= p1 <= p2, got %r, %r' % (what, p1, p2))
    if paths != 4 and paths != 8:
        raise ValueError('%s: paths must be 4 or 8, got %r' % (what, paths))
    return p1, p2, int(paths)


def regularize_scores(volume, p1=SGM_DEFAULTS[0], p2=SGM_DEFAULTS[1], paths=SGM_DEFAULTS[2]):
    """volume [D,R,S] (NaN = an invalid hypothesis) -> the definition's regularised scores A, fp64 [D,R,S] on the device"""
    what = 'regularize_scores'
    p1, p2, paths = _sgm_checked(p1, p2, paths, what)
    v = torch.as_tensor(volume)
    if v.dim() != 3:
        raise ValueError('%s: the volume must be [D, R, S], got shape %s' % (what, tuple(v.shape)))
    D, R, S = v.shape
    if D < 1 or R < 1 or S < 1:
        raise ValueError('%s: the volume must hold at least one hypothesis of one pixel, got shape %s' % (what, tuple(v.shape)))
    if D > MAX_D_SGM:
        raise ValueError('%s: at most %d hypotheses, got %d' % (what, MAX_D_SGM, D))
    if R * S > 2 ** 31 - 1 or R * S * D > 2 ** 40:
        raise ValueError('%s: %d x %d pixels of %d hypotheses are beyond the limits (R*S < 2^31, R*S*D <= 2^40)' % (what, R, S, D))
    if not v.is_cuda and bool(torch.isinf(v).any()):
        raise ValueError('%s: a score is infinite' % what)
    v = v.to(v.device if v.is_cuda else torch.device('cuda'), torch.float64).contiguous()
    out = torch.empty_like(v)
    size = lib().mvsdf_stereo_sgm_workspace_bytes(R, S, D)
    ws = torch.empty(size, dtype=torch.uint8, device=v.device)
    check(lib().mvsdf_stereo_regularize(_vp(v), R, S, D, p1, p2, paths, _vp(ws), size, _vp(out), _stream(v)), 'mvsdf_stereo_regularize')
    _, err = _header(ws, K.MVSDF_RES_H_WORDS)
    raise_for_bits(err, what, [(K.MVSDF_PS_ERR_FINITE, ValueError, 'a score is infinite')] + ERRORS)
    return out


def _sweep_args(what, descriptors, cams, pairs, num_src, views):
    """the checks plane_sweep and band_sweep share -> (descriptors as a tensor, cams fp64 numpy, the views to sweep, their sources)"""
    cams = np.asarray(cams.cpu() if isinstance(cams, torch.Tensor) else cams, dtype=np.float64)
    f = torch.as_tensor(descriptors)
    if f.dim() == 4 and cams.shape != (f.shape[0], 2, 4, 4):
        raise ValueError('%s: cams must be [V, 2, 4, 4] for V = %d descriptor maps, got shape %s' % (what, f.shape[0], cams.shape))
    if f.dim() == 4 and len(pairs) != f.shape[0]:
        raise ValueError('%s: pairs must hold one list per view (%d), got %d' % (what, f.shape[0], len(pairs)))
    if not np.isfinite(cams).all():
        raise ValueError('%s: a camera entry is NaN or infinite' % what)
    num_src = int(num_src)
    if num_src < 0:
        raise ValueError('%s: num_src must be >= 0' % what)
    V = len(pairs)
    views = list(range(V)) if views is None else [int(v) for v in views]
    if any(v < 0 or v >= V for v in views):
        raise ValueError('%s: a view index is outside [0, %d)' % (what, V))
    used = [[int(s) for s in pairs[v]][:num_src] for v in views]
    if any(s < 0 or s >= V for q in used for s in q):
        raise ValueError('%s: a pair index is outside [0, %d)' % (what, V))
    if any(len(q) > MAX_SRC for q in used):
        raise ValueError('%s: at most %d sources per view' % (what, MAX_SRC))
    return f, cams, views, used


def _pair_tables(what, cams, views, used):
    """-> (pair_off int32 [len(views) + 1], pair_src int32, the number of pair slots, T_rs per slot as fp64 [slots * 16])"""
    try:
        P, Pinv = projection_matrices(cams)
    except np.linalg.LinAlgError as e:
        raise ValueError('%s: a camera has a singular projection' % what) from e
    off = np.zeros(len(views) + 1, np.int32)
    off[1:] = np.cumsum([len(q) for q in used])
    src = np.asarray([s for q in used for s in q], np.int32)
    npairs = len(src)
    mats = np.empty(max(npairs, 1) * 16, np.float64)
    k = 0
    for r, q in zip(views, used):
        for s in q:
            mats[k * 16:k * 16 + 16] = (P[s] @ Pinv[r]).reshape(-1)
            k += 1
    if not np.isfinite(mats[:npairs * 16]).all():
        raise ValueError('%s: a camera entry is NaN or infinite' % what)
    return off, src, npairs, mats


def plane_sweep(descriptors, cams, pairs, num_src=2, views=None, scores=False, regularize=None):
    """The module's definition -> Sweep.  Device tensors are used where they are (the stream is theirs); numpy / CPU input is copied to the GPU.
    views: the reference views to sweep, in this order (default: all); scores=True also returns the score volume of the last of them.
    regularize: None (winner-take-all on the raw scores), True (the regularisation with SGM_DEFAULTS), (p1, p2) or (p1, p2, paths)."""
    what = 'plane_sweep'
    sgm = _sgm_args(regularize, what)
    f, cams, views, used = _sweep_args(what, descriptors, cams, pairs, num_src, views)
    nhyp = cams[views, 1, 3, 2] if views else np.zeros(0)
    if (nhyp != np.floor(nhyp)).any() or (nhyp < 1).any() or (nhyp > MAX_D).any():
        raise ValueError('%s: the number of depth hypotheses (cams[v, 1, 3, 2]) must be a whole number in [1, %d]' % (what, MAX_D))
    if sgm and (nhyp > MAX_D_SGM).any():
        raise ValueError('%s: the regularisation takes at most %d depth hypotheses' % (what, MAX_D_SGM))
    f, dev = _feature_tensor(f, what)
    V, R, S, C = f.shape
    off, src, npairs, mats = _pair_tables(what, cams, views, used)
    vw = np.asarray(views, np.int32)
    ranges = np.ascontiguousarray(cams[views, 1, 3, :2] if views else np.zeros((0, 2)), np.float64)
    nh = np.asarray(nhyp, np.int32)
    dmax = int(nh.max()) if len(nh) else 1
    size = (lib().mvsdf_stereo_sweep_sgm_workspace_bytes if sgm else lib().mvsdf_stereo_workspace_bytes)(R, S, dmax, npairs)
    if size == 0:
        raise ValueError('%s: %d x %d texels of %d hypotheses are beyond the limits (R*S < 2^31, R*S*D <= 2^40)' % (what, R, S, dmax))
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    # zeros / -1: the kernels write the maps of the views in `views` only; every other view keeps the "no estimate" values it is allocated with
    depths = torch.zeros(V, R, S, dtype=torch.float32, device=dev)
    probs = torch.zeros(V, 3, R, S, dtype=torch.float32, device=dev)
    best_k = torch.full((V, R, S), -1, dtype=torch.int32, device=dev)
    counts = torch.zeros(V, R, S, dtype=torch.int32, device=dev)
    if not views:
        return Sweep(depths, probs, best_k, counts, None)
    head = (_vp(f), V, R, S, C, len(views), vw.ctypes.data, off.ctypes.data, src.ctypes.data if npairs else None, mats.ctypes.data, ranges.ctypes.data,
            nh.ctypes.data)
    tail = (_vp(ws), size, _vp(depths), _vp(probs), _vp(best_k), _vp(counts), _stream(f))
    if sgm:
        check(lib().mvsdf_stereo_sweep_sgm(*head, sgm[0], sgm[1], sgm[2], *tail), 'mvsdf_stereo_sweep_sgm')
    else:
        check(lib().mvsdf_stereo_sweep(*head, *tail), 'mvsdf_stereo_sweep')
    _, err = _header(ws, K.MVSDF_RES_H_WORDS)   # the one wait of the call; the host arrays live until here
    raise_for_bits(err, what, ERRORS)
    vol = reg = None
    if scores:
        at = lib().mvsdf_stereo_volume_offset(R, S, dmax, npairs)
        D = int(nh[-1])
        vol = ws[at:at + D * R * S * 8].view(torch.float64).view(D, R, S).clone()
        if sgm:
            at = lib().mvsdf_stereo_workspace_bytes(R, S, dmax, npairs)
            reg = ws[at:at + D * R * S * 8].view(torch.float64).view(D, R, S).clone()
    return Sweep(depths, probs, best_k, counts, vol, reg)


class Cascade:
    """The result of cascade_sweep: depths fp32 [V,R,S], probs fp32 [V,3,R,S], best_k int32 [V,R,S] and counts int32 [V,R,S] at the last stage's
    size (the module doc, "Cascade": probs[:,1] is stage 1's full-range peak ratio), and stages: the Sweep of every stage at its own size."""

    def __init__(self, depths, probs, best_k, counts, stages):
        self.depths, self.probs, self.best_k, self.counts, self.stages = depths, probs, best_k, counts, stages


def _size_of(size, what):
    try:
        R, S = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError('%s: size must be (R, S), got %r' % (what, size)) from None
    if R < 1 or S < 1 or R * S > 2 ** 31 - 1:
        raise ValueError('%s: size must be at least 1 x 1 (and R*S < 2^31), got %r' % (what, size))
    return R, S


def upsample_depth(depth, best_k, size):
    """The module's centres: depth fp32 [V,r,s] and best_k int32 [V,r,s] of a sweep (-1: no winner), size = (R, S) -> fp64 [V,R,S] on the device,
    NaN where none of a pixel's four parents has a winner."""
    what = 'upsample_depth'
    R, S = _size_of(size, what)
    d, k = torch.as_tensor(depth), torch.as_tensor(best_k)
    if d.dim() != 3 or tuple(k.shape) != tuple(d.shape) or d.shape[0] < 1 or d.shape[1] < 2 or d.shape[2] < 2:
        raise ValueError('%s: depth and best_k must both be [V, r, s] with V >= 1 and r, s >= 2, got %s and %s' % (what, tuple(d.shape), tuple(k.shape)))
    dev = d.device if d.is_cuda else (k.device if k.is_cuda else torch.device('cuda'))
    d, k = d.to(dev, torch.float32).contiguous(), k.to(dev, torch.int32).contiguous()
    V, r, s = d.shape
    out = torch.empty(V, R, S, dtype=torch.float64, device=dev)
    check(lib().mvsdf_stereo_upsample(_vp(d), _vp(k), V, r, s, R, S, _vp(out), _stream(d)), 'mvsdf_stereo_upsample')
    return out


def _band_args(what, depth_num, step, V):
    """-> (D_b, steps fp64 [V]), checked"""
    if isinstance(depth_num, bool) or depth_num != int(depth_num) or not 1 <= int(depth_num) <= MAX_D_BAND:
        raise ValueError('%s: depth_num must be a whole number in [1, %d], got %r' % (what, MAX_D_BAND, depth_num))
    steps = np.asarray(step, np.float64)
    if steps.ndim == 0:
        steps = np.full(V, float(steps))
    if steps.shape != (V,):
        raise ValueError('%s: step must be a number or one per view (%d), got shape %s' % (what, V, steps.shape))
    if not (np.isfinite(steps) & (steps > 0)).all():
        raise ValueError('%s: every step must be finite and positive' % what)
    return int(depth_num), steps


def _checked_centres(what, centres, shape):
    c = torch.as_tensor(centres)
    if tuple(c.shape) != tuple(shape):
        raise ValueError('%s: centres must be [V, R, S] = %s, got shape %s' % (what, tuple(shape), tuple(c.shape)))
    if not c.is_cuda and bool(torch.isinf(c).any()):
        raise ValueError('%s: a centre is infinite' % what)
    return c


def band_sweep(descriptors, cams, pairs, centres, depth_num, step, num_src=2, views=None):
    """The module's band sweep -> Sweep (scores None; best_k the index within the band).  centres fp64 [V,R,S] (NaN: none); depth_num = D_b; step: a
    number or one per view (indexed by the view, as cams is).  Device tensors are used where they are.  views: the reference views to sweep (default:
    all; none twice), all of them in one launch."""
    what = 'band_sweep'
    f, cams, views, used = _sweep_args(what, descriptors, cams, pairs, num_src, views)
    if len(set(views)) != len(views):
        raise ValueError('%s: a view is listed twice' % what)
    if len(views) > 65535:
        raise ValueError('%s: at most 65535 views per call' % what)
    Db, steps = _band_args(what, depth_num, step, len(pairs))
    f = _checked_features(f, what)
    c = _checked_centres(what, centres, f.shape[:3])
    return _band_run(what, f, cams, views, used, c, Db, steps)


def _band_run(what, f, cams, views, used, c, Db, steps):
    """band_sweep once every argument has been checked"""
    f, dev = _feature_tensor(f, what)
    V, R, S, C = f.shape
    off, src, npairs, mats = _pair_tables(what, cams, views, used)
    c = c.to(dev, torch.float64).contiguous()
    # zeros / -1: the kernels write the maps of the views in `views` only; every other view keeps the "no estimate" values it is allocated with
    depths = torch.zeros(V, R, S, dtype=torch.float32, device=dev)
    probs = torch.zeros(V, 3, R, S, dtype=torch.float32, device=dev)
    best_k = torch.full((V, R, S), -1, dtype=torch.int32, device=dev)
    counts = torch.zeros(V, R, S, dtype=torch.int32, device=dev)
    if not views:
        return Sweep(depths, probs, best_k, counts, None)
    size = lib().mvsdf_stereo_band_workspace_bytes(R, S, Db, len(views), npairs)
    if size == 0:
        raise ValueError('%s: %d x %d texels are beyond the limits (R*S < 2^31)' % (what, R, S))
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    vw = np.asarray(views, np.int32)
    st = np.ascontiguousarray(steps[views], np.float64)
    check(lib().mvsdf_stereo_band(_vp(f), V, R, S, C, len(views), vw.ctypes.data, off.ctypes.data, src.ctypes.data if npairs else None, mats.ctypes.data,
                                  st.ctypes.data, _vp(c), Db, _vp(ws), size, _vp(depths), _vp(probs), _vp(best_k), _vp(counts), _stream(f)),
          'mvsdf_stereo_band')
    _, err = _header(ws, K.MVSDF_RES_H_WORDS)   # the one wait of the call; the host arrays live until here
    raise_for_bits(err, what, ERRORS)
    return Sweep(depths, probs, best_k, counts, None)


def _cascade_args(what, depth_nums, interval_scales, stages=None):
    """-> (depth_nums, interval_scales) as tuples of one length L (= stages where given), checked; D_1 may be None"""
    try:
        dn, sc = tuple(depth_nums), tuple(interval_scales)
    except TypeError:
        raise ValueError('%s: depth_nums and interval_scales must be tuples, got %r and %r' % (what, depth_nums, interval_scales)) from None
    L = len(dn) if stages is None else stages
    if not 1 <= L <= MAX_STAGES:
        raise ValueError('%s: a cascade has 1 to %d stages, got %d' % (what, MAX_STAGES, L))
    if len(dn) != L or len(sc) != L:
        raise ValueError('%s: depth_nums and interval_scales must hold one entry per stage (%d), got %d and %d' % (what, L, len(dn), len(sc)))
    for l, d in enumerate(dn):
        if d is None and l == 0:
            continue
        if d is None or isinstance(d, bool) or d != int(d) or not 1 <= int(d) <= (MAX_D if l == 0 else MAX_D_BAND):
            raise ValueError('%s: depth_nums[%d] must be a whole number in [1, %d]%s, got %r' %
                             (what, l, MAX_D if l == 0 else MAX_D_BAND, ' or None' if l == 0 else '', d))
    try:
        sc = tuple(float(g) for g in sc)
    except (TypeError, ValueError):
        raise ValueError('%s: interval_scales must be numbers, got %r' % (what, interval_scales)) from None
    if not all(np.isfinite(g) and g > 0 for g in sc):
        raise ValueError('%s: every interval scale must be finite and positive, got %r' % (what, sc))
    return tuple(None if d is None else int(d) for d in dn), sc


def cascade_sweep(descriptors_per_stage, cams, pairs, num_src=2, views=None, depth_nums=CASCADE_DEFAULTS[0], interval_scales=CASCADE_DEFAULTS[1],
                  regularize=None):
    """The module's cascade -> Cascade.  descriptors_per_stage: one map [V,R_l,S_l,C_l] per stage, coarsest first; cams [V,2,4,4] at the last
    stage's size.  Stage 1 is plane_sweep (regularize applies to it alone), every later stage one upsample_depth and one band_sweep."""
    from .utils.io import scale_camera
    what = 'cascade_sweep'
    try:
        maps = list(descriptors_per_stage)
    except TypeError:
        raise ValueError('%s: descriptors_per_stage must be a list of descriptor maps' % what) from None
    if not 1 <= len(maps) <= MAX_STAGES:
        raise ValueError('%s: a cascade has 1 to %d stages, got %d' % (what, MAX_STAGES, len(maps)))
    L = len(maps)
    dn, sc = _cascade_args(what, depth_nums, interval_scales, L)
    sgm = _sgm_args(regularize, what)
    # ---- every stage's arguments, before the GPU is touched ----
    args = [_sweep_args(what, m, cams, pairs, num_src, views) for m in maps]
    maps = [_checked_features(a[0], what) for a in args]
    if any(m.shape[0] != maps[0].shape[0] for m in maps):
        raise ValueError('%s: the stages differ in their number of views: %s' % (what, [m.shape[0] for m in maps]))
    _, cams, views, used = args[-1]
    if L > 1 and len(set(views)) != len(views):
        raise ValueError('%s: a view is listed twice' % what)
    V = len(pairs)
    nhyp = cams[:, 1, 3, 2]
    if (nhyp[views] != np.floor(nhyp[views])).any() or (nhyp[views] < 1).any() or (nhyp[views] > MAX_D).any():
        raise ValueError('%s: the number of depth hypotheses (cams[v, 1, 3, 2]) must be a whole number in [1, %d]' % (what, MAX_D))
    d1 = np.ceil(nhyp / sc[0]) if dn[0] is None else np.full(V, float(dn[0]))
    if (d1[views] < 1).any() or (d1[views] > MAX_D).any():
        raise ValueError('%s: stage 1 would sweep a number of hypotheses outside [1, %d]' % (what, MAX_D))
    if sgm and (d1[views] > MAX_D_SGM).any():
        raise ValueError('%s: the regularisation takes at most %d depth hypotheses' % (what, MAX_D_SGM))
    interval = cams[:, 1, 3, 1]
    steps = [interval * g for g in sc]
    for l in range(1, L):
        if not (np.isfinite(steps[l][views]) & (steps[l][views] > 0)).all():
            raise ValueError('%s: the step of stage %d (interval * %g) must be finite and positive for every view' % (what, l + 1, sc[l]))
    RL, SL = maps[-1].shape[1:3]
    stage_cams = []
    for l, m in enumerate(maps):
        c = scale_camera(cams, (m.shape[2] / SL, m.shape[1] / RL))
        c[:, 1, 3, 1] = steps[l]
        if l == 0:
            c[:, 1, 3, 2] = np.where(np.isfinite(d1), d1, 0.0)
        stage_cams.append(c)
    # ---- the stages ----
    stages = [plane_sweep(maps[0], stage_cams[0], pairs, num_src=num_src, views=views, regularize=regularize)]
    for l in range(1, L):
        prev = stages[-1]
        centres = upsample_depth(prev.depths, prev.best_k, maps[l].shape[1:3])
        stages.append(_band_run(what, maps[l], stage_cams[l], views, used, centres, dn[l], steps[l]))
    last, first = stages[-1], stages[0]
    R1, S1 = first.depths.shape[1:]
    dev = last.depths.device
    yy = ((2 * torch.arange(RL, device=dev) + 1) * R1) // (2 * RL)
    xx = ((2 * torch.arange(SL, device=dev) + 1) * S1) // (2 * SL)
    probs = last.probs.clone()
    probs[:, 1] = torch.where(last.best_k >= 0, first.probs[:, 1][:, yy][:, :, xx], torch.zeros((), dtype=torch.float32, device=dev))
    return Cascade(last.depths, probs, last.best_k, last.counts, stages)


def _write_cam(path, cam):
    """MVSNet's camera text with the four depth words (depth_min, interval, D, depth_max), which load_cam reads back"""
    txt = 'extrinsic\n' + '\n'.join(' '.join('%.17g' % v for v in r) for r in cam[0]) + '\n\nintrinsic\n'
    txt += '\n'.join(' '.join('%.17g' % v for v in r) for r in cam[1][:3, :3])
    txt += '\n\n%.17g %.17g %d %.17g\n' % (cam[1, 3, 0], cam[1, 3, 1], int(cam[1, 3, 2]), cam[1, 3, 3])
    with open(path, 'w') as f:
        f.write(txt)


def _find(folder, stem, exts):
    for e in exts:
        p = os.path.join(folder, stem + e)
        if os.path.exists(p):
            return p
    raise FileNotFoundError('estimate_scene: none of %s in %s' % (', '.join(stem + e for e in exts), folder))


def estimate_scene(data_root, result_dir, feat_ckpt=None, descriptor='patch', num_src=2, max_d=256, interval_scale=1, resize=None, crop=None,
                   radius=2, regularize=None, cascade=None):
    """BYOD.md's "Run VisMVSNet" step by plane sweep.  Reads <data_root>/images/<id:08>.jpg|png, cams/<id:08>_cam.txt and pair.txt; resizes
    (prepare.resize_bilinear_u8) and centre-crops the images (resize / crop: 'W,H' or (W, H), default: as they are) and moves the cameras along;
    computes descriptors at half that size, as Vis-MVSNet's depth maps are: with feat_ckpt FeatExt.from_checkpoint + extract_features, else
    (descriptor='patch') patch_descriptors(radius) of the image resized to half; sweeps every view and writes into result_dir <id:08>_flow3.pfm,
    <id:08>_flow{1,2,3}_prob.pfm, cam_<id:08>_flow3.txt (at depth-map scale), <id:08>.jpg (the cropped image) and pair.txt -> the Sweep.  regularize: plane_sweep's.
    cascade: None / False (the one full sweep), True (cascade_sweep with CASCADE_DEFAULTS) or (depth_nums, interval_scales): the same files from the
    final maps of the cascade -> the Cascade.  Its finest stage has the size above and every coarser one ((R + 1)//2, (S + 1)//2) of the next; with
    feat_ckpt the stages are FeatExt's maps (features.extract_pyramid, at most three), else patch_descriptors of the image resized to each size."""
    from PIL import Image
    from .datasets import prepare
    from .utils import io as sio
    what = 'estimate_scene'
    if feat_ckpt is None and descriptor != 'patch':
        raise ValueError("%s: descriptor must be 'patch' where no feat_ckpt is given, got %r" % (what, descriptor))
    _sgm_args(regularize, what)
    if cascade is None or cascade is False:
        cascade = None
    else:
        try:
            cascade = _cascade_args(what, *(CASCADE_DEFAULTS if cascade is True else tuple(cascade)))
        except TypeError:
            raise ValueError('%s: cascade must be None, True or (depth_nums, interval_scales), got %r' % (what, cascade)) from None
        if feat_ckpt is not None and len(cascade[0]) > 3:
            raise ValueError('%s: FeatExt has three maps; a cascade over them has at most three stages' % what)
    pair_path = os.path.join(data_root, 'pair.txt')
    pair = sio.load_pair(pair_path)
    ids = pair['id_list']
    images, cams = [], []
    for vid in ids:
        z = vid.zfill(8)
        img = prepare.load_image_u8(_find(os.path.join(data_root, 'images'), z, ('.jpg', '.png')))
        cam = sio.load_cam(os.path.join(data_root, 'cams', '%s_cam.txt' % z), max_d, interval_scale)
        h0, w0 = img.shape[:2]
        rw, rh = prepare._pair_of(resize) if resize is not None else (w0, h0)
        cw, ch = prepare._pair_of(crop) if crop is not None else (rw, rh)
        if cw > rw or ch > rh:
            raise ValueError('%s: crop %d,%d is larger than the resized image %d,%d' % (what, cw, ch, rw, rh))
        img = prepare.center_crop(prepare.resize_bilinear_u8(img, rw, rh), cw, ch)
        cam = sio.scale_camera(cam, (rw / w0, rh / h0))
        cam[1, 0, 2] -= (rw - cw) // 2
        cam[1, 1, 2] -= (rh - ch) // 2
        images.append(np.ascontiguousarray(img))
        cams.append(cam)
    if len({im.shape for im in images}) != 1:
        raise ValueError('%s: the images differ in size after resize / crop; give resize and crop' % what)
    H, W = images[0].shape[:2]
    if feat_ckpt is not None:
        from .features import FeatExt, extract_features, output_hw
        R, S = output_hw(H, W)
        net = FeatExt.from_checkpoint(feat_ckpt).cuda()
        rgb = torch.from_numpy(np.stack(images)).permute(0, 3, 1, 2).float() / 255                # ImageNet normalisation, as SceneDataset feeds FeatExt
        rgb = (rgb - torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)) / torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
        if cascade:
            from .features import extract_pyramid
            feats = list(extract_pyramid(net, rgb))[3 - len(cascade[0]):]
        else:
            feats = extract_features(net, rgb).permute(0, 2, 3, 1).contiguous()
    else:
        R, S = (H + 1) // 2, (W + 1) // 2
        sizes = [(R, S)]
        for _ in range(len(cascade[0]) - 1 if cascade else 0):
            sizes.insert(0, ((sizes[0][0] + 1) // 2, (sizes[0][1] + 1) // 2))
        feats = [patch_descriptors(np.stack([prepare.resize_bilinear_u8(im, s, r) for im in images]), radius) for r, s in sizes]
        if not cascade:
            feats = feats[0]
    cams = np.stack([sio.scale_camera(c, (S / W, R / H)) for c in cams])
    if cascade:
        sweep = cascade_sweep([normalize_descriptors(f) for f in feats], cams, prepare.pair_indices(pair), num_src=num_src, depth_nums=cascade[0],
                              interval_scales=cascade[1], regularize=regularize)
    else:
        sweep = plane_sweep(normalize_descriptors(feats), cams, prepare.pair_indices(pair), num_src=num_src, regularize=regularize)
    os.makedirs(result_dir, exist_ok=True)
    depths, probs = sweep.depths.cpu().numpy(), sweep.probs.cpu().numpy()
    for i, vid in enumerate(ids):
        z = vid.zfill(8)
        sio.write_pfm(os.path.join(result_dir, '%s_flow3.pfm' % z), np.ascontiguousarray(depths[i]))
        for j in range(3):
            sio.write_pfm(os.path.join(result_dir, '%s_flow%d_prob.pfm' % (z, j + 1)), np.ascontiguousarray(probs[i, j]))
        _write_cam(os.path.join(result_dir, 'cam_%s_flow3.txt' % z), cams[i])
        Image.fromarray(images[i]).save(os.path.join(result_dir, '%s.jpg' % z), quality=95)
    with open(pair_path) as fi, open(os.path.join(result_dir, 'pair.txt'), 'w') as fo:
        fo.write(fi.read())
    return sweep
