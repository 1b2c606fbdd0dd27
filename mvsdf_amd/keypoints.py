"""Sparse points from posed images on the device: what COLMAP calls "reconstruct sparse model from known camera poses" -- scale-space keypoints
with 128-d int8 descriptors, all-pairs matching with a ratio test on the int8 matrix cores, epipolar verification from the
known poses, tracks, and multi-view triangulation; `sparse_points` composes them and `sparse_model` puts the result into a COLMAP model dict.  The tracks are what viewsel.view_scores / depth_ranges take
(track_off, track_view).  Kernels: csrc/keypoints.hip (the design: DESIGN.md, "Sparse points"); tests/keypoints_ref.py restates every stage in
numpy and the device results equal it bit for bit.  Lowe's and COLMAP's rules are WRITTEN FROM MEMORY: the rules here are the definition.

The definition.  fp64 in the order written, no FMA contraction, only + - * / sqrt, floor, compares and det_math64.h's atan2_pos / expneg; everything else is integers.  The centre of pixel
(x, y) is X = x + 0.5, Y = y + 0.5.  Keypoints of V views lie one view after the other in a `Keypoints` tuple: xy fp64 [N,2], scale, angle,
response fp64 [N], codes int8 [N,128] (0 .. 127), view_off int64 [V+1] (view v owns rows view_off[v] .. view_off[v+1]).  `concat` joins tuples view
after view.  The stages below read xy, codes and view_off only.

1a. scale_space(images) -> a list over octaves of (L fp64 [V,6,h,w], D fp64 [V,5,h,w]): the first step of the detector.
   images [V,H,W,3] or [V,H,W], uint8 or fp32 (promoted exactly), all of one size.  Grey: (299 R + 587 G + 114 B) / 1000 -- for uint8 the integer
   sum converted to fp64 and divided, for fp32 ((299.0*R + 587.0*G) + 114.0*B) / 1000.0 in fp64; one channel is taken as it is.  Octaves o = 0, 1,
   ... while the smaller side is at least MIN_SIDE = 16 (at least one); S = 3 intervals, levels s = 0 .. 5 with sigma_s = 1.6 * 2^(s/3); the input
   counts as blurred with 0.5 and there is no upsampled octave.  Level 0 of octave 0 is the grey image blurred with sqrt(1.6^2 - 0.5^2), level s
   the level before it blurred with sqrt(sigma_s^2 - sigma_(s-1)^2), level 0 of the next octave is level 3 at every second pixel (x, y = 0, 2,
   ...: [(h+1)//2, (w+1)//2]).  A blur is separable, rows first (along x), then columns: out = the sum from 0.0 over the taps k = 0 .. 2r left to
   right of tap[k] * in[clamp(coordinate + k - r)].  `blur_taps(sigma)` makes the table once on the host in numpy (r = ceil(3 sigma), exp(-(k -
   r)^2 / (2 sigma^2)) divided by their numpy sum): it is an input to the kernel and to the restatement alike.  D_s = L_(s+1) - L_s.

1b. detect_extrema(images, contrast=2.0, edge_ratio=10) -> Extrema(xy fp64 [N,2], scale fp64 [N], response fp64 [N], site int32 [N,4] (octave,
   level, y, x), view_off int64 [V+1]): the detector's second step.  Candidates are the sites (s, y, x) of an octave's D with s = 1 .. 3 and BORDER =
   5 <= x < w - 5, 5 <= y < h - 5.  With v = D_s(y, x), a candidate is kept iff all of: |v| > contrast (in the units of the grey values); v is
   strictly greater, or strictly smaller, than all 26 neighbours in (s, y, x); on D_s, dxx = (D(x+1) + D(x-1)) - 2.0*v, dyy likewise, dxy = 0.25 *
   ((D(y+1,x+1) - D(y+1,x-1)) - (D(y-1,x+1) - D(y-1,x-1))), tr = dxx + dyy, de = dxx*dyy - dxy*dxy: de > 0 and (tr*tr)*r < ((r+1.0)*(r+1.0))*de;
   and the one quadratic step succeeds: g = 0.5 * (D(+1) - D(-1)) along x, y and s; dss, dxs, dys as dxx and dxy with s in place of a coordinate
   (the "+1" row of dys is level s+1: 0.25 * ((D(s+1,y+1) - D(s+1,y-1)) - (D(s-1,y+1) - D(s-1,y-1)))); H = [[dxx, dxy, dxs], [dxy, dyy, dys], [dxs,
   dys, dss]]; det = det3(H) (det3 as in 5.) is finite and not 0; off_k = det3(H with column k replaced by (-gx, -gy, -gs)) / det; every |off_k| <=
   0.5.  Then xy = (((x + off_x) + 0.5) * 2^o, ((y + off_y) + 0.5) * 2^o); scale = sigma_s * 2^o, NOT refined in s (sigma_s from the host table);
   response = |v + 0.5 * ((gx*off_x + gy*off_y) + gs*off_s)|.  The extrema of a view are listed by (octave, level, y, x).

1c. detect(images, max_keypoints=8192, contrast=2.0, edge_ratio=10, upright=False) -> Keypoints.  Orientation and descriptor are taken on level
   L_s of the extremum's octave with its integer site (y, x) as the centre; the gradient at a sample is gx = L(x+1) - L(x-1), gy = L(y+1) - L(y-1),
   mag = sqrt(gx*gx + gy*gy), t = atan2_pos(|gy|, gx), negated where gy < 0 (det_math64.h's atan2_pos and expneg throughout).
   Orientation (skipped with upright=True: angle 0, (cos, sin) = (1, 0)): sigma_w = 1.5 * sigma_s, R_o = ceil(3 sigma_w), g = 1 / (2 sigma_w^2)
   (host).  For (dy, dx) in [-R_o, R_o]^2 (the square window, rows first) with 1 <= x+dx <= w-2 and 1 <= y+dy <= h-2: t plus 2 pi where negative,
   minus 2 pi if >= 2 pi; bin = min(35, floor(t * (36 / (2 pi)))); the bin receives rint((mag * expneg(-(fp64(dx*dx + dy*dy) * g))) * 2^32) as an
   int64.  The largest bin b wins, the lowest at a tie; an empty histogram gives angle 0.  With l, c, r = fp64 of bins b-1, b, b+1 (cyclic): den =
   (l - 2.0*c) + r; p = (0.5 * (l - r)) / den, 0 where den = 0; angle = ((b + 0.5) + p) * (2 pi / 36), plus 2 pi if negative, minus 2 pi if >= 2
   pi.  One orientation per keypoint.  Its cosine and sine are polynomials: u = angle - pi, z = u*u, sin(u) = u * P(z) and cos(u) = Q(z) by Horner
   from the highest term down (p = p*z + c_k) over `trig_table()`'s coefficients (-1)^k / (2k+1)!, k = 0 .. 13, and (-1)^k / (2k)!, k = 0 .. 14
   (a host table, the factorials by repeated fp64 products); cos(angle) = -Q, sin(angle) = -(u * P).
   The descriptor of an extremum at
   site (o, s, y, x), on level L_s of its octave, with its integer site as the centre: cell width hc = 3 * sigma_s, window radius R = ceil(hc *
   sqrt(2) * 2.5) (both from the host).  For (dy, dx) in [-R, R]^2, rows first, with 1 <= x+dx <= w-2 and 1 <= y+dy <= h-2: rx = (c*dx + s*dy) / hc,
   ry = (c*dy - s*dx) / hc with (c, s) = (cos, sin) of the angle ((1, 0) upright); cx = rx + 1.5, cy = ry + 1.5; skipped unless -1 < cx < 4 and -1 <
   cy < 4; mag and t of the sample as above; rel =
   t - angle, plus 2 pi while negative (at most twice), minus 2 pi if >= 2 pi; ob = rel * (8 / (2 pi)); val = mag * expneg(-((rx*rx + ry*ry) *
   0.125)).  With x0 = floor(cx), fx = cx - x0 and likewise y0, fy, o0, fo, each of the 8 corners (i, j, k)
   whose cell (x0+i, y0+j) lies in 0 .. 3 receives ((val * wx) * wy) * wo, w = f for the upper corner and 1.0 - f for the lower, into bin ((y0+j)*4
   + (x0+i))*8 + ((o0+k) mod 8), quantised to an integer as rint(vote * 2^32) (ties to even) and summed as int64.  Then u_c = fp64(sum_c) * 2^-32;
   n1 = sqrt of the sum of u*u from 0.0 in index order; n1 = 0 drops the keypoint; u = min(u / n1, 0.2); n2 likewise; codes = min(127, floor(512 *
   (u / n2))).  Keypoints of a view keep the order of 1b; a view with more than max_keypoints keeps the first max_keypoints under (response
   descending, then that order), listed in that order again (a stable sort; on the device through torch).

2. match_descriptors(kp, pairs=None, ratio=0.8, mutual=True, max_dist=None) -> Matches(pair int32 [M,2] (views a < b), off int64 [M+1], idx int32
   [.,2] (keypoint indices within view a and view b), dist int32 [.]).  pairs=None: every a < b.  For a keypoint i of view a: D(i,j) = sum_c (s_ic -
   t_jc)^2 over the 128 codes, an integer <= 128 * 127^2.  j1 is the smallest j under the total order (D, j), D1 that distance; D2 is the smallest
   D(i,j) over j != j1, a value only; with a single keypoint in view b there is no D2.  The match (i, j1) is kept iff (there is no D2 or fp64(D1) <
   (ratio*ratio) * fp64(D2)) and (max_dist is None or D1 <= max_dist) and (not mutual or the same search from b to a sends j1 back to i: the
   search alone, without the ratio test).  Kept matches of a pair are listed by i ascending; dist = D1.  A view without keypoints gives empty pairs.
   All listed pairs and both directions run in one launch (at most 32767 pairs per call).

3. verify_matches(kp, matches, cams, max_epipolar=2.0) -> Matches.  cams fp64 [V,2,4,4] (extrinsic, intrinsic).  On the host, in numpy fp64
   (`fundamental_matrices`): Kinv_v = [[1/fx, -s/(fx*fy), (s*cy - cx*fy)/(fx*fy)], [0, 1/fy, -cy/fy], [0, 0, 1]] from K_v = [[fx, s, cx], [0, fy,
   cy], [0, 0, 1]]; R_ab = R_b R_a^T; t_ab = t_b - R_ab t_a; F_ab = Kinv_b^T ([t_ab]x (R_ab Kinv_a)), so that x_b^T F x_a = 0.  On the device a match
   is kept iff both point-line distances are <= max_epipolar: that of x_b to l = F x_a and that of x_a to l' = F^T x_b, with l_k = (F[k,0]*Xa +
   F[k,1]*Ya) + F[k,2], l'_k = (F[0,k]*Xb + F[1,k]*Yb) + F[2,k] and the distance of (X, Y) to a line |((l0*X + l1*Y) + l2)| / sqrt(l0*l0 + l1*l1).
   A line with l0 = l1 = 0 fails the test.  Order is preserved.

4. build_tracks(kp, matches, max_rounds=256) -> (track_off int64 [T+1], track_view int32 [nnz], track_kp int32 [nnz]).  Nodes are the global
   keypoint indices view_off[v] + i, edges the matches.  Components by minimum-label propagation (every round hands the smaller label of an edge's
   ends to the other end, then every node follows its label's label; the host reads a "changed" flag every 4 rounds; max_rounds: ValueError).  A
   component that holds two keypoints of one view is dropped; a component of size 1 is no track.  Tracks are listed by their smallest node, their
   entries by node ascending.

5. triangulate_tracks(kp, tracks, cams, max_reproj=2.0, min_angle=1.5) -> (xyz fp64 [T,3], error fp64 [T], keep bool [T], obs_keep bool [nnz]).
   From the host (`camera_arrays`): c_v = -(R^T t), rays_v = R^T Kinv (Kinv as in 3.), proj_v = K [R | t] (rows 0 .. 2 of fusion.projection_matrices),
   cos(min_angle degrees).  For an observation (v, (X, Y)): d_k = (rays[k,0]*X + rays[k,1]*Y) + rays[k,2]; n = sqrt((d0*d0 + d1*d1) + d2*d2);
   r = d / n per component.  The estimate minimises sum |(I - r r^T)(P - c)|^2: a_kl = (1.0 if k == l else 0.0) - r_k*r_l; A_kl and b_k = (a_k0*c0
   + a_k1*c1) + a_k2*c2 are summed from 0.0 in entry order; det3(m) = (m00*(m11*m22 - m12*m21) - m01*(m10*m22 - m12*m20)) + m02*(m10*m21 -
   m11*m20); det = det3(A); a determinant that is not > 0 rejects the track; P_k = det3(A with column k replaced by b) / det.  An observation
   PASSES at P iff z = ((p20*P0 + p21*P1) + p22*P2) + p23 > 0 and e = sqrt(du*du + dv*dv) <= max_reproj, du = (row 0 of proj likewise) / z - X,
   dv = (row 1) / z - Y.  The one refit: the observations that do not pass are dropped; fewer than 2 left rejects the track; if any was dropped
   the estimate is formed once more from the remainder, and then every remaining observation must pass, else the track is rejected.  The angle:
   some pair of remaining rays must have (r_i0*r_j0 + r_i1*r_j1) + r_i2*r_j2 <= cos(min_angle).  error = the mean of e over the remaining
   observations, summed from 0.0 in entry order, divided by their number.  A rejected track has xyz = 0, error = 0, keep = False and no observation
   kept; obs_keep marks the remaining observations of a kept track.

6. sparse_points(images, cams, pairs=None, max_keypoints=8192, contrast=2.0, edge_ratio=10, upright=False, ratio=0.8, max_epipolar=2.0, max_reproj=2.0,
   min_angle=1.5) -> SparsePoints(xyz fp64 [P,3], rgb uint8 [P,3], error fp64 [P], track_off int64 [P+1], track_view, track_kp int32 [nnz],
   keypoints): stages 1 to 5 (mutual matching).  images: one array [V,H,W(,3)] or a list of V arrays [H,W(,3)] of differing sizes; stage 1 runs once
   per size (and dtype / channel) group and the views are put back in their order.  Only the kept tracks and their kept observations are
   returned, in the order of stage 4; rgb is the texel (floor(X), floor(Y)) of the image under a point's first observation (a grey image gives its
   value three times, fp32 images are scaled by 255 and rounded, clipped to 0 .. 255).  report: a dict that receives the counts (views, keypoints,
   matches, verified, tracks, points).
   sparse_model(model, image_dir, ...) -> the model dict of datasets.colmap.load_colmap_model (pinhole cameras, camera_intrinsics' refusal for
   distorted ones; its points3D may be empty) with images[..]['xys'] = the keypoints of that image, ['point3D_ids'] = the point of each keypoint or
   -1, and points replaced: ids 1 .. P, tracks by COLMAP image id and point2D index.  The views are the images by ascending id
   (datasets.colmap.model_views); images are read with PIL as RGB.  `assemble_model` is the host-side part.  write_colmap_text writes it and
   load_colmap_model reads back the same bits.  datasets.colmap.colmap_to_mvs(..., triangulate=True) replaces the model's points by these before
   scores and ranges are computed (tools/colmap2mvs.py --triangulate); tools/sparse_points.py is the command.

NOT BUILT.  Pose estimation (unposed images; bundle.py refines given poses: sparse_model(refine=True)); guided matching that restricts candidates to the epipolar band inside the
matcher; several orientations per keypoint; an upsampled first octave; vocabulary-tree pair selection; a wave-per-keypoint descriptor kernel.

ValueError before any launch: a dtype other than the one named (nothing is converted silently), a wrong shape, view offsets that do not ascend from
0, a pair that is not a < b inside [0, V), more than 32767 pairs, more than 2^20 keypoints in a view, a ratio, max_dist, max_epipolar, max_reproj
or min_angle out of range.  ValueError through the call's error bits: a code outside 0 .. 127, a non-finite coordinate or camera entry, a view or
keypoint index out of range, the round limit."""
import collections
import ctypes
import math

import numpy as np
import torch

from ._lib import check, lib, K, raise_for_bits, _header, _stream, _vp
from .cloud import _device
from .global_reg import _array

DIM = K.MVSDF_KP_DIM
MAX_KEYPOINTS = K.MVSDF_KP_MAX_KEYPOINTS
MAX_PAIRS = K.MVSDF_KP_MAX_PAIRS
MAX_DIST = K.MVSDF_KP_MAX_DIST
MAX_VIEWS = K.MVSDF_VS_MAX_VIEWS
MAX_RADIUS = K.MVSDF_KP_MAX_RADIUS
INTERVALS, SIGMA0, SIGMA_INPUT, MIN_SIDE = 3, 1.6, 0.5, 16

Keypoints = collections.namedtuple('Keypoints', 'xy scale angle response codes view_off')
Matches = collections.namedtuple('Matches', 'pair off idx dist')
SparsePoints = collections.namedtuple('SparsePoints', 'xyz rgb error track_off track_view track_kp keypoints')
Extrema = collections.namedtuple('Extrema', 'xy scale response site view_off')
BORDER = 5
MAX_EXTREMA = 1 << 22                                # extrema of one octave of one call

# the error bits of a keypoints call (csrc/keypoints.hip), in the order they are looked at
ERRORS = [(K.MVSDF_PS_ERR_SHAPE, ValueError, 'a count is outside the limits'),
          (K.MVSDF_PS_ERR_FINITE, ValueError, 'a coordinate or a camera entry is NaN or infinite'),
          (K.MVSDF_PS_ERR_PAIR, ValueError, 'a view index is outside [0, V)'),
          (K.MVSDF_PS_ERR_CODE, ValueError, 'a code is outside 0 .. 127'),
          (K.MVSDF_PS_ERR_INDEX, ValueError, 'a keypoint index is outside its view, or offsets do not ascend'),
          (K.MVSDF_PS_ERR_ROUNDS, ValueError, 'the round limit of the track labelling was reached')]


def make_keypoints(xy, codes, view_off, scale=None, angle=None, response=None):
    """a Keypoints tuple from the fields the stages read (scale 1, angle 0, response 0 where not given); tensors stay where they are"""
    xy = torch.as_tensor(xy)
    n = xy.shape[0]
    fill = [torch.full((n,), v, dtype=torch.float64, device=xy.device) if x is None else torch.as_tensor(x)
            for x, v in ((scale, 1.0), (angle, 0.0), (response, 0.0))]
    return Keypoints(xy, fill[0], fill[1], fill[2], torch.as_tensor(codes), torch.as_tensor(view_off))


def concat(parts):
    """the Keypoints of several calls, view after view -> Keypoints"""
    parts = list(parts)
    if not parts:
        raise ValueError('concat: nothing to join')
    dev = torch.as_tensor(parts[0].xy).device
    fields = [torch.cat([torch.as_tensor(p[f]).to(dev) for p in parts]) for f in range(5)]
    offs, base = [torch.zeros(1, dtype=torch.int64)], 0
    for p in parts:
        vo = torch.as_tensor(p.view_off).cpu()
        offs.append(vo[1:] + base)
        base += int(vo[-1])
    return Keypoints(*fields, torch.cat(offs))


def blur_taps(sigma):
    """the normalised Gaussian taps of the definition, fp64 numpy [2 ceil(3 sigma) + 1]"""
    r = int(math.ceil(3.0 * sigma))
    k = np.arange(-r, r + 1, dtype=np.float64)
    t = np.exp(-(k * k) / (2.0 * sigma * sigma))
    return t / t.sum()


def level_sigmas():
    """(sigma_s for s = 0 .. 5, the blur that leads to each level: from the input for s = 0, from the level before otherwise)"""
    sig = [SIGMA0 * 2.0 ** (s / INTERVALS) for s in range(INTERVALS + 3)]
    inc = [math.sqrt(sig[0] * sig[0] - SIGMA_INPUT * SIGMA_INPUT)] + [math.sqrt(sig[s] * sig[s] - sig[s - 1] * sig[s - 1]) for s in range(1, INTERVALS + 3)]
    return sig, inc


def octave_sizes(h, w):
    out = [(h, w)]
    while min((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2) >= MIN_SIDE:
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def scale_space(images):
    """step 1a -> [(L fp64 [V,6,h,w], D fp64 [V,5,h,w]) per octave] on the device"""
    what = 'scale_space'
    if not isinstance(images, (torch.Tensor, np.ndarray)):
        raise ValueError('%s: images must be a numpy array or a torch tensor' % what)
    img = torch.as_tensor(images)
    if img.dtype not in (torch.uint8, torch.float32) or img.dim() not in (3, 4) or (img.dim() == 4 and img.shape[3] != 3) or min(img.shape) < 1:
        raise ValueError('%s: images must be uint8 or float32 [V,H,W,3] or [V,H,W], got %s %s' % (what, img.dtype, tuple(img.shape)))
    V, H, W = img.shape[:3]
    if H > 2 ** 31 - 1 or W > 2 ** 31 - 1 or V * 6 > 2 ** 31 - 1 or V * 6 * H * W > 2 ** 40:
        raise ValueError('%s: the images are too large' % what)
    img = _device(img)
    dev, L_ = img.device, lib()
    nlev = INTERVALS + 3
    taps = [torch.from_numpy(blur_taps(s)).to(dev) for s in level_sigmas()[1]]
    if any((t.shape[0] - 1) // 2 > MAX_RADIUS for t in taps):
        raise ValueError('%s: a tap radius exceeds %d' % (what, MAX_RADIUS))
    grey = torch.empty(V, H, W, dtype=torch.float64, device=dev)
    st = _stream(img)
    check(L_.mvsdf_kp_grey(_vp(img), 1 if img.dtype == torch.float32 else 0, 3 if img.dim() == 4 else 1, V * H * W, _vp(grey), st), 'mvsdf_kp_grey')
    out, base = [], grey
    for o, (h, w) in enumerate(octave_sizes(H, W)):
        lev = torch.empty(nlev, V, h, w, dtype=torch.float64, device=dev)
        tmp = torch.empty(V, h, w, dtype=torch.float64, device=dev)
        for s in range(nlev):
            if s == 0 and o > 0:
                lev[0].copy_(base)
                continue
            src = base if s == 0 else lev[s - 1]
            check(L_.mvsdf_kp_blur(_vp(src), V, h, w, _vp(taps[s]), (taps[s].shape[0] - 1) // 2, _vp(tmp), _vp(lev[s]), st), 'mvsdf_kp_blur')
        Lv = lev.permute(1, 0, 2, 3).contiguous()
        D = torch.empty(V, nlev - 1, h, w, dtype=torch.float64, device=dev)
        check(L_.mvsdf_kp_dog(_vp(Lv), V, nlev, h * w, _vp(D), st), 'mvsdf_kp_dog')
        out.append((Lv, D))
        base = torch.empty(V, (h + 1) // 2, (w + 1) // 2, dtype=torch.float64, device=dev)
        check(L_.mvsdf_kp_half(_vp(lev[INTERVALS]), V, h, w, _vp(base), st), 'mvsdf_kp_half')
    return out


def detect_extrema(images, contrast=2.0, edge_ratio=10):
    """step 1b -> Extrema on the device (view_off on the host)"""
    what = 'detect_extrema'
    contrast, edge_ratio = _limit(contrast, 'contrast', what), float(edge_ratio)
    if not (edge_ratio >= 1 and math.isfinite(edge_ratio)):
        raise ValueError('%s: edge_ratio must be a finite number >= 1, got %r' % (what, edge_ratio))
    space = scale_space(images)
    V = space[0][1].shape[0]
    dev = space[0][1].device
    per_view = [[] for _ in range(V)]
    for o, (_, D) in enumerate(space):
        cand, out = _extrema_of_octave(D, o, contrast, edge_ratio, what)
        n = cand.shape[0]
        counts = torch.bincount(cand[:, 0].long(), minlength=V).cpu().tolist() if n else [0] * V     # (the list is ordered by view: contiguous runs)
        at = 0
        for v in range(V):
            c = cand[at:at + counts[v]].clone()
            c[:, 0] = o
            per_view[v].append((out[at:at + counts[v]], c))
            at += counts[v]
    outs = torch.cat([p[0] for pv in per_view for p in pv])
    sites = torch.cat([p[1] for pv in per_view for p in pv])
    view_off = torch.tensor([0] + list(np.cumsum([sum(p[0].shape[0] for p in pv) for pv in per_view])), dtype=torch.int64)
    return Extrema(outs[:, :2].contiguous(), outs[:, 2].contiguous(), outs[:, 3].contiguous(), sites, view_off)


def descriptor_tables():
    """(cell width, window radius, 1 / (2 sigma_w^2) and radius of the orientation window) per level 1 .. 3 of the definition, from the host"""
    sig = level_sigmas()[0]
    cell = np.array([3.0 * sig[s] for s in range(1, INTERVALS + 1)], dtype=np.float64)
    radius = np.array([int(math.ceil(c * math.sqrt(2.0) * 2.5)) for c in cell], dtype=np.int32)
    sw = [1.5 * sig[s] for s in range(1, INTERVALS + 1)]
    ogauss = np.array([1.0 / (2.0 * x * x) for x in sw], dtype=np.float64)
    oradius = np.array([int(math.ceil(3.0 * x)) for x in sw], dtype=np.int32)
    return cell, radius, ogauss, oradius


def trig_table():
    """the coefficients (-1)^k / (2k+1)!, k = 0 .. 13, and (-1)^k / (2k)!, k = 0 .. 14, fp64 [29]; the factorials by repeated fp64 products"""
    fact = [1.0]
    for k in range(1, 30):
        fact.append(fact[-1] * float(k))
    return np.array([(1.0 if k % 2 == 0 else -1.0) / fact[2 * k + 1] for k in range(14)] + [(1.0 if k % 2 == 0 else -1.0) / fact[2 * k] for k in range(15)],
                    dtype=np.float64)


def _extrema_of_octave(D, o, contrast, edge_ratio, what):
    """mvsdf_kp_extrema on one octave -> (cand int32 [n,4] (view, level, y, x), out fp64 [n,4])"""
    V, _, h, w = D.shape
    dev = D.device
    sig = np.ascontiguousarray(level_sigmas()[0][1:INTERVALS + 1], dtype=np.float64)
    size = lib().mvsdf_kp_extrema_workspace_bytes(V, h, w)
    if size == 0:
        raise ValueError('%s: the images are too large (V * 3 * H * W must stay below 2^31)' % what)
    cap = min(V * INTERVALS * h * w, MAX_EXTREMA)
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    cand = torch.empty(cap, 4, dtype=torch.int32, device=dev)
    out = torch.empty(cap, 4, dtype=torch.float64, device=dev)
    check(lib().mvsdf_kp_extrema(_vp(D), V, h, w, contrast, edge_ratio, BORDER, float(2 ** o), _hp(sig), cap, _vp(ws), size, _vp(cand), _vp(out),
                                 _stream(D)), 'mvsdf_kp_extrema')
    hd = _header(ws, K.MVSDF_RES_H_WORDS)
    raise_for_bits(hd[K.MVSDF_RES_H_ERR], what, ERRORS)
    n = hd[K.MVSDF_RES_H_COUNT]
    return cand[:n], out[:n]


def detect(images, max_keypoints=8192, contrast=2.0, edge_ratio=10, upright=False):
    """step 1c -> Keypoints on the device (view_off on the host)"""
    what = 'detect'
    if isinstance(max_keypoints, bool) or int(max_keypoints) != max_keypoints or not 1 <= int(max_keypoints) <= MAX_KEYPOINTS:
        raise ValueError('%s: max_keypoints must be an integer in 1 .. %d, got %r' % (what, MAX_KEYPOINTS, max_keypoints))
    contrast, edge_ratio = _limit(contrast, 'contrast', what), float(edge_ratio)
    if not (edge_ratio >= 1 and math.isfinite(edge_ratio)):
        raise ValueError('%s: edge_ratio must be a finite number >= 1, got %r' % (what, edge_ratio))
    space = scale_space(images)
    V = space[0][1].shape[0]
    dev = space[0][1].device
    cell, radius, ogauss, oradius = descriptor_tables()
    trig = torch.from_numpy(trig_table()).to(dev)
    per_view = [[] for _ in range(V)]
    for o, (Lv, D) in enumerate(space):
        cand, out = _extrema_of_octave(D, o, contrast, edge_ratio, what)
        n = cand.shape[0]
        if n == 0:
            continue
        h, w = D.shape[2:]
        cand = cand.contiguous()
        angle = torch.empty(n, dtype=torch.float64, device=dev)
        acc = torch.empty(n, DIM, dtype=torch.int64, device=dev)
        codes = torch.empty(n, DIM, dtype=torch.int8, device=dev)
        valid = torch.empty(n, dtype=torch.uint8, device=dev)
        check(lib().mvsdf_kp_describe(_vp(Lv), V, h, w, _vp(cand), n, 1 if upright else 0, _hp(cell), _hp(radius), _hp(ogauss), _hp(oradius), _vp(trig),
                                      _vp(acc), _vp(angle), _vp(codes), _vp(valid), _stream(Lv)), 'mvsdf_kp_describe')
        out = torch.cat([out, angle[:, None]], 1)
        keep = valid.bool()
        view = cand[:, 0].long()
        for v in range(V):
            m = keep & (view == v)
            per_view[v].append((out[m], codes[m]))
    parts, counts = [], []
    for pv in per_view:
        o_ = torch.cat([p[0] for p in pv]) if pv else torch.zeros(0, 5, dtype=torch.float64, device=dev)
        c_ = torch.cat([p[1] for p in pv]) if pv else torch.zeros(0, DIM, dtype=torch.int8, device=dev)
        if o_.shape[0] > max_keypoints:
            first = torch.sort(o_[:, 3], descending=True, stable=True).indices[:int(max_keypoints)]
            first = torch.sort(first).values
            o_, c_ = o_[first], c_[first]
        parts.append((o_, c_))
        counts.append(o_.shape[0])
    o_, c_ = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    view_off = torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int64)
    return Keypoints(o_[:, :2].contiguous(), o_[:, 2].contiguous(), o_[:, 4].contiguous(), o_[:, 3].contiguous(),
                     c_.contiguous(), view_off)


def _view_off(kp, what):
    """the offsets as a host int64 array, checked"""
    vo = _array(kp.view_off, torch.int64, (None,), what, 'view_off').cpu().numpy()
    V = vo.shape[0] - 1
    if not 1 <= V <= MAX_VIEWS:
        raise ValueError('%s: view_off must hold 2 .. %d offsets, got %d' % (what, MAX_VIEWS + 1, V + 1))
    n = np.diff(vo)
    if vo[0] != 0 or (n < 0).any() or (n > MAX_KEYPOINTS).any() or vo[-1] > 2 ** 31 - 1:
        raise ValueError('%s: view_off must ascend from 0, with at most %d keypoints per view and 2^31 - 1 in all' % (what, MAX_KEYPOINTS))
    return np.ascontiguousarray(vo), V


def _xy(kp, n, what):
    return _device(_array(kp.xy, torch.float64, (n, 2), what, 'xy'))


def _pairs(pairs, V, what, limit):
    if pairs is None:
        pairs = np.array([(a, b) for a in range(V) for b in range(a + 1, V)], dtype=np.int32).reshape(-1, 2)
    p = _array(pairs, torch.int32, (None, 2), what, 'pairs').cpu().numpy()
    if limit is not None and p.shape[0] > limit:
        raise ValueError('%s: %d pairs (at most %d per call)' % (what, p.shape[0], limit))
    if p.shape[0] and not ((p[:, 0] >= 0) & (p[:, 0] < p[:, 1]) & (p[:, 1] < V)).all():
        raise ValueError('%s: every pair must be (a, b) with 0 <= a < b < V = %d' % (what, V))
    return np.ascontiguousarray(p)


def _hp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _limit(x, name, what):
    x = float(x)
    if not (x >= 0 and math.isfinite(x)):
        raise ValueError('%s: %s must be a finite number >= 0, got %r' % (what, name, x))
    return x


def match_splits(view_off, pairs):
    """over how many workgroups the matcher splits its walk over a view's targets at these sizes"""
    vo = np.ascontiguousarray(np.asarray(view_off, dtype=np.int64))
    p = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    return int(lib().mvsdf_kp_match_splits(_hp(vo), vo.shape[0] - 1, _hp(p), p.shape[0]))


def match_descriptors(kp, pairs=None, ratio=0.8, mutual=True, max_dist=None):
    """stage 2 -> Matches on the device"""
    what = 'match_descriptors'
    vo, V = _view_off(kp, what)
    n = int(vo[-1])
    codes = _array(kp.codes, torch.int8, (n, DIM), what, 'codes')
    p = _pairs(pairs, V, what, MAX_PAIRS)
    ratio = float(ratio)
    if not 0 < ratio <= 1:
        raise ValueError('%s: ratio must be in (0, 1], got %r' % (what, ratio))
    if max_dist is None:
        max_dist = MAX_DIST
    elif isinstance(max_dist, bool) or int(max_dist) != max_dist or not 0 <= int(max_dist) <= MAX_DIST:
        raise ValueError('%s: max_dist must be None or an integer in 0 .. %d, got %r' % (what, MAX_DIST, max_dist))
    codes = _device(codes)
    dev = codes.device
    M = p.shape[0]
    pair = torch.from_numpy(p.copy()).to(dev)
    cap = int((vo[p[:, 0] + 1] - vo[p[:, 0]]).sum()) if M else 0
    if cap == 0:                                                  # no kernel runs: the offsets of no match
        none = torch.zeros(M + 1, dtype=torch.int64, device=dev)
        return Matches(pair, none, torch.empty(0, 2, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev))
    size = lib().mvsdf_kp_match_workspace_bytes(_hp(vo), V, _hp(p), M)
    if size == 0:
        raise ValueError('%s: the sizes are outside the limits' % what)
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    off = torch.empty(M + 1, dtype=torch.int64, device=dev)      # k_kp_offsets writes all M + 1
    idx = torch.empty(cap, 2, dtype=torch.int32, device=dev)
    dist = torch.empty(cap, dtype=torch.int32, device=dev)
    check(lib().mvsdf_kp_match(_vp(codes), _hp(vo), V, _hp(p), M, ratio * ratio, int(max_dist), 1 if mutual else 0, _vp(ws), size, _vp(off), _vp(idx),
                               _vp(dist), _stream(codes)), 'mvsdf_kp_match')
    h = _header(ws, K.MVSDF_RES_H_WORDS)
    raise_for_bits(h[K.MVSDF_RES_H_ERR], what, ERRORS)
    count = h[K.MVSDF_RES_H_COUNT]
    return Matches(pair, off, idx[:count], dist[:count])


def _matches(matches, V, dev, what):
    """the Matches on the device, shapes and dtypes checked -> (pair, off, idx, dist, M, E)"""
    pair = _array(matches.pair, torch.int32, (None, 2), what, 'matches.pair').to(dev).contiguous()
    M = pair.shape[0]
    off = _array(matches.off, torch.int64, (M + 1,), what, 'matches.off').to(dev).contiguous()
    idx = _array(matches.idx, torch.int32, (None, 2), what, 'matches.idx').to(dev).contiguous()
    E = idx.shape[0]
    dist = _array(matches.dist, torch.int32, (E,), what, 'matches.dist').to(dev).contiguous()
    if E > 2 ** 31 - 1:
        raise ValueError('%s: %d matches (at most 2^31 - 1)' % (what, E))
    return pair, off, idx, dist, M, E


def _cams(cams, V, what):
    c = np.asarray(cams.cpu() if isinstance(cams, torch.Tensor) else cams)
    if c.dtype != np.float64 or c.shape != (V, 2, 4, 4):
        raise ValueError('%s: cams must be float64 [%d, 2, 4, 4], got %s %s' % (what, V, c.dtype, c.shape))
    return c


def intrinsic_inverse(Kv):
    """Kinv of the definition from an upper-triangular K [3,3] (numpy fp64)"""
    fx, s, cx, fy, cy = Kv[0, 0], Kv[0, 1], Kv[0, 2], Kv[1, 1], Kv[1, 2]
    return np.array([[1 / fx, -s / (fx * fy), (s * cy - cx * fy) / (fx * fy)], [0.0, 1 / fy, -cy / fy], [0.0, 0.0, 1.0]])


def fundamental_matrices(cams, pairs):
    """F fp64 numpy [M,3,3] of the definition: x_b^T F x_a = 0"""
    cams = np.asarray(cams, dtype=np.float64)
    out = np.zeros((len(pairs), 3, 3))
    for m, (a, b) in enumerate(np.asarray(pairs)):
        Ra, ta, Rb, tb = cams[a, 0, :3, :3], cams[a, 0, :3, 3], cams[b, 0, :3, :3], cams[b, 0, :3, 3]
        R = Rb @ Ra.T
        t = tb - R @ ta
        tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
        out[m] = intrinsic_inverse(cams[b, 1, :3, :3]).T @ (tx @ (R @ intrinsic_inverse(cams[a, 1, :3, :3])))
    return out


def camera_arrays(cams):
    """(centers [V,3], rays [V,3,3], proj [V,3,4]) fp64 numpy of the definition"""
    cams = np.asarray(cams, dtype=np.float64)
    V = len(cams)
    centers, rays, proj = np.zeros((V, 3)), np.zeros((V, 3, 3)), np.zeros((V, 3, 4))
    for v, cam in enumerate(cams):
        R, t = cam[0, :3, :3], cam[0, :3, 3]
        centers[v] = -(R.T @ t)
        rays[v] = R.T @ intrinsic_inverse(cam[1, :3, :3])
        K4 = np.eye(4)
        K4[:3, :3] = cam[1, :3, :3]
        proj[v] = (K4 @ cam[0])[:3]
    return centers, rays, proj


def verify_matches(kp, matches, cams, max_epipolar=2.0):
    """stage 3 -> Matches on the device"""
    what = 'verify_matches'
    vo, V = _view_off(kp, what)
    xy = _xy(kp, int(vo[-1]), what)
    dev = xy.device
    pair, off, idx, dist, M, E = _matches(matches, V, dev, what)
    c = _cams(cams, V, what)
    limit = _limit(max_epipolar, 'max_epipolar', what)
    if E == 0 or M == 0:
        return Matches(pair, torch.zeros(M + 1, dtype=torch.int64, device=dev), idx[:0], dist[:0])
    p = _pairs(pair.cpu(), V, what, None)
    F = torch.from_numpy(fundamental_matrices(c, p)).to(dev).contiguous()
    size = lib().mvsdf_kp_verify_workspace_bytes(E)
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    off_out = torch.empty(M + 1, dtype=torch.int64, device=dev)
    idx_out = torch.empty(E, 2, dtype=torch.int32, device=dev)
    dist_out = torch.empty(E, dtype=torch.int32, device=dev)
    vod = torch.from_numpy(vo).to(dev)
    check(lib().mvsdf_kp_verify(_vp(xy), _vp(vod), V, _vp(pair), M, _vp(off), _vp(idx), _vp(dist), E, _vp(F), limit, _vp(ws), size, _vp(off_out),
                                _vp(idx_out), _vp(dist_out), _stream(xy)), 'mvsdf_kp_verify')
    h = _header(ws, K.MVSDF_RES_H_WORDS)
    raise_for_bits(h[K.MVSDF_RES_H_ERR], what, ERRORS)
    count = h[K.MVSDF_RES_H_COUNT]
    return Matches(pair, off_out, idx_out[:count], dist_out[:count])


def build_tracks(kp, matches, max_rounds=256):
    """stage 4 -> (track_off int64 [T+1], track_view int32 [nnz], track_kp int32 [nnz]) on the device"""
    what = 'build_tracks'
    vo, V = _view_off(kp, what)
    N = int(vo[-1])
    dev = _device(_array(matches.idx, torch.int32, (None, 2), what, 'matches.idx')).device
    pair, off, idx, _, M, E = _matches(matches, V, dev, what)
    if isinstance(max_rounds, bool) or int(max_rounds) != max_rounds or not 1 <= int(max_rounds) <= 2 ** 31 - 1:
        raise ValueError('%s: max_rounds must be a positive integer, got %r' % (what, max_rounds))
    if N == 0 or E == 0 or M == 0:
        return torch.zeros(1, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
    size = lib().mvsdf_kp_tracks_workspace_bytes(N, E)
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    track_off = torch.empty(N // 2 + 1, dtype=torch.int64, device=dev)
    track_view = torch.empty(N, dtype=torch.int32, device=dev)
    track_kp = torch.empty(N, dtype=torch.int32, device=dev)
    vod = torch.from_numpy(vo).to(dev)
    check(lib().mvsdf_kp_tracks(_vp(vod), V, N, _vp(pair), M, _vp(off), _vp(idx), E, int(max_rounds), _vp(ws), size, _vp(track_off), _vp(track_view),
                                _vp(track_kp), _stream(idx)), 'mvsdf_kp_tracks')
    h = _header(ws, K.MVSDF_KP_TRACKS_H_WORDS)
    raise_for_bits(h[K.MVSDF_KP_TRACKS_H_ERR], what, ERRORS)
    T, nnz = h[K.MVSDF_KP_TRACKS_H_TRACKS], h[K.MVSDF_KP_TRACKS_H_ENTRIES]
    return track_off[:T + 1], track_view[:nnz], track_kp[:nnz]


def triangulate_tracks(kp, tracks, cams, max_reproj=2.0, min_angle=1.5):
    """stage 5 -> (xyz fp64 [T,3], error fp64 [T], keep bool [T], obs_keep bool [nnz]) on the device"""
    what = 'triangulate_tracks'
    vo, V = _view_off(kp, what)
    xy = _xy(kp, int(vo[-1]), what)
    dev = xy.device
    track_off = _array(tracks[0], torch.int64, (None,), what, 'track_off').to(dev).contiguous()
    T = track_off.shape[0] - 1
    track_view = _array(tracks[1], torch.int32, (None,), what, 'track_view').to(dev).contiguous()
    nnz = track_view.shape[0]
    track_kp = _array(tracks[2], torch.int32, (nnz,), what, 'track_kp').to(dev).contiguous()
    if T < 0 or T > 2 ** 31 - 1 or nnz > 2 ** 31 - 1:
        raise ValueError('%s: track_off must hold at least one offset, and at most 2^31 - 1 tracks and entries' % what)
    c = _cams(cams, V, what)
    max_reproj = _limit(max_reproj, 'max_reproj', what)
    min_angle = float(min_angle)
    if not 0 <= min_angle <= 180:
        raise ValueError('%s: min_angle must be in [0, 180] degrees, got %r' % (what, min_angle))
    if T == 0 or nnz == 0:                                        # no kernel runs: no track is kept, no point is made
        z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)  # noqa: E731
        return z(T, 3), z(T), torch.zeros(T, dtype=torch.bool, device=dev), torch.zeros(nnz, dtype=torch.bool, device=dev)
    xyz = torch.empty(T, 3, dtype=torch.float64, device=dev)      # k_kp_triangulate writes every track's xyz, error and keep
    error = torch.empty(T, dtype=torch.float64, device=dev)
    keep = torch.empty(T, dtype=torch.uint8, device=dev)
    # zeros: the kernel writes obs_keep only at the entries its tracks own, track_off[t] .. track_off[t + 1]; the entries before track_off[0] and
    # behind track_off[T] stay as allocated
    obs_keep = torch.zeros(nnz, dtype=torch.uint8, device=dev)
    centers, rays, proj = (torch.from_numpy(a).to(dev).contiguous() for a in camera_arrays(c))
    hdr = torch.empty(256, dtype=torch.uint8, device=dev)
    vod = torch.from_numpy(vo).to(dev)
    check(lib().mvsdf_kp_triangulate(_vp(xy), _vp(vod), V, _vp(track_off), _vp(track_view), _vp(track_kp), T, nnz, _vp(centers), _vp(rays), _vp(proj),
                                     max_reproj, math.cos(math.radians(min_angle)), _vp(xyz), _vp(error), _vp(keep), _vp(obs_keep), _vp(hdr),
                                     _stream(xy)), 'mvsdf_kp_triangulate')
    raise_for_bits(_header(hdr, K.MVSDF_ERRW_H_WORDS)[K.MVSDF_ERRW_H_ERR], what, ERRORS)
    return xyz, error, keep.bool(), obs_keep.bool()


def _texels(images, view, xy):
    """uint8 [n,3]: the texel under each position of its view's image (host)"""
    out = np.zeros((len(view), 3), np.uint8)
    for q, (v, (X, Y)) in enumerate(zip(view, xy)):
        img = images[v]
        t = img[min(max(int(math.floor(Y)), 0), img.shape[0] - 1), min(max(int(math.floor(X)), 0), img.shape[1] - 1)]
        t = np.asarray(t, dtype=np.float64).reshape(-1)
        if img.dtype != np.uint8:
            t = np.clip(np.rint(t * 255.0), 0, 255)
        out[q] = t if t.shape[0] == 3 else t[0]
    return out


def sparse_points(images, cams, pairs=None, max_keypoints=8192, contrast=2.0, edge_ratio=10, upright=False, ratio=0.8, max_epipolar=2.0,
                  max_reproj=2.0, min_angle=1.5, report=None):
    """definition 6 -> SparsePoints (device tensors; rgb a device tensor too)"""
    what = 'sparse_points'
    views = [np.asarray(i.cpu() if isinstance(i, torch.Tensor) else i) for i in images]
    V = len(views)
    if V < 1 or any(i.ndim not in (2, 3) or i.dtype not in (np.uint8, np.float32) for i in views):
        raise ValueError('%s: images must be V arrays [H,W,3] or [H,W] of dtype uint8 or float32' % what)
    c = _cams(cams, V, what)
    groups = {}
    for v, i in enumerate(views):
        groups.setdefault((i.shape, i.dtype.str), []).append(v)
    single = [None] * V
    for members in groups.values():
        kp = detect(np.stack([views[v] for v in members]), max_keypoints, contrast, edge_ratio, upright)
        vo = kp.view_off.tolist()
        for q, v in enumerate(members):
            single[v] = Keypoints(*(f[vo[q]:vo[q + 1]] for f in kp[:5]), torch.tensor([0, vo[q + 1] - vo[q]], dtype=torch.int64))
    kp = concat(single)
    matches = match_descriptors(kp, pairs, ratio, True)
    verified = verify_matches(kp, matches, c, max_epipolar)
    tracks = build_tracks(kp, verified)
    xyz, error, keep, obs_keep = triangulate_tracks(kp, tracks, c, max_reproj, min_angle)
    if report is not None:
        report.update(views=V, keypoints=int(kp.view_off[-1]), matches=int(matches.idx.shape[0]), verified=int(verified.idx.shape[0]),
                      tracks=int(keep.shape[0]), points=int(keep.sum()))
    return _kept(kp, tracks, xyz, error, keep, obs_keep, views)


def _kept(kp, tracks, xyz, error, keep, obs_keep, views):
    """the kept tracks with their kept observations, and the colour under each point's first observation -> SparsePoints"""
    dev = xyz.device
    track_off, track_view, track_kp = (t.to(dev) for t in tracks)
    T = keep.shape[0]
    owner = torch.repeat_interleave(torch.arange(T, device=dev), track_off[1:] - track_off[:-1])
    counts = torch.zeros(T, dtype=torch.int64, device=dev).index_add_(0, owner, obs_keep.long())[keep]
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(counts, 0)])
    tv, tk = track_view[obs_keep], track_kp[obs_keep]
    first = off[:-1]
    fv = tv[first].cpu().numpy() if len(first) else np.zeros(0, np.int64)
    fxy = kp.xy.to(dev)[kp.view_off.to(dev)[tv[first].long()] + tk[first].long()].cpu().numpy() if len(first) else np.zeros((0, 2))
    rgb = torch.from_numpy(_texels(views, fv, fxy)).to(dev)
    return SparsePoints(xyz[keep], rgb, error[keep], off, tv, tk, kp)


def assemble_model(model, ids, xy, view_off, xyz, rgb, error, track_off, track_view, track_kp):
    """the model dict with the keypoints of view i (numpy arrays, the views in the order of `ids`, COLMAP image ids) as its observations and the
    points with their tracks; host only"""
    xy, view_off, track_off, track_view, track_kp = (np.asarray(a) for a in (xy, view_off, track_off, track_view, track_kp))
    P = len(track_off) - 1
    owner = np.repeat(np.arange(P, dtype=np.int64), np.diff(track_off))
    images = {}
    for i, iid in enumerate(ids):
        pid = np.full(int(view_off[i + 1] - view_off[i]), -1, dtype=np.int64)
        sel = track_view == i
        pid[track_kp[sel]] = owner[sel] + 1
        images[iid] = dict(model['images'][iid], xys=np.ascontiguousarray(xy[view_off[i]:view_off[i + 1]], dtype=np.float64), point3D_ids=pid)
    for iid, im in model['images'].items():
        images.setdefault(iid, im)
    points = {'ids': np.arange(1, P + 1, dtype=np.int64), 'xyz': np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3),
              'rgb': np.ascontiguousarray(rgb, dtype=np.uint8).reshape(-1, 3), 'error': np.ascontiguousarray(error, dtype=np.float64),
              'track_off': track_off.astype(np.int64), 'track_image': np.asarray(ids, dtype=np.int64)[track_view].astype(np.int32),
              'track_point2D': track_kp.astype(np.int32)}
    return {'cameras': model['cameras'], 'images': images, 'points': points}


def refine_points(sp, cams, images, max_reproj=2.0, min_angle=1.5, report=None, **options):
    """bundle.bundle_adjust (options) over the cameras and the points of a SparsePoints, then stage 5 once more over its tracks with the refined
    cameras, so that max_reproj and the angle test hold for the new poses -> (SparsePoints, cams fp64 numpy [V,2,4,4])"""
    from . import bundle
    tracks = (sp.track_off, sp.track_view, sp.track_kp)
    res = bundle.bundle_adjust(cams, sp.xyz, sp.track_off, sp.track_view, bundle.observations(sp.keypoints, tracks), **options)
    xyz, error, keep, obs_keep = triangulate_tracks(sp.keypoints, tracks, res.cams, max_reproj, min_angle)
    if report is not None:
        report.update(refine=dict(cost0=res.cost0, cost=res.cost, iterations=res.iterations, accepted=res.accepted,
                                  cg_iterations=res.cg_iterations, points=int(keep.sum())))
    views = [np.asarray(i.cpu() if isinstance(i, torch.Tensor) else i) for i in images]
    return _kept(sp.keypoints, tracks, xyz, error, keep, obs_keep, views), res.cams


def sparse_model(model, image_dir, report=None, refine=False, refine_options=None, **kw):
    """definition 6 -> the model dict with observations, points and tracks from the images; kw: sparse_points' options.  refine=True: the cameras
    and points then go through `refine_points` (refine_options: bundle.bundle_adjust's) and the images' q / t are the refined poses"""
    import os
    from PIL import Image
    from .datasets import colmap
    empty = colmap._points([], [], [], [], [0], [], [])
    ids, names, cams, _ = colmap.model_views(dict(model, points=empty))     # (camera_intrinsics refuses distorted cameras here)
    if not ids:
        raise ValueError('sparse_model: the model holds no image')
    images = []
    for n in names:
        path = os.path.join(image_dir, n)
        if not os.path.exists(path):
            raise FileNotFoundError('sparse_model: %s (named by the model) does not exist' % path)
        with Image.open(path) as im:
            images.append(np.asarray(im.convert('RGB')))
    sp = sparse_points(images, cams, report=report, **kw)
    if refine:
        from . import bundle
        sp, cams = refine_points(sp, cams, images, kw.get('max_reproj', 2.0), kw.get('min_angle', 1.5), report, **(refine_options or {}))
        model = dict(model, images={iid: dict(model['images'][iid], q=bundle.quaternion(cams[i, 0, :3, :3]), t=cams[i, 0, :3, 3].copy())
                                    for i, iid in enumerate(ids)})
    host = [t.cpu().numpy() for t in (sp.keypoints.xy, sp.keypoints.view_off, sp.xyz, sp.rgb, sp.error, sp.track_off, sp.track_view, sp.track_kp)]
    return assemble_model(model, ids, *host)
