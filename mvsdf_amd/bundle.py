"""Bundle adjustment on the device: Levenberg-Marquardt over the poses of V views and P sparse points, the points eliminated (Schur complement) and
the reduced camera system solved matrix-free by preconditioned conjugate gradients.  It refines what keypoints.py triangulates from given cameras
(keypoints.sparse_model(refine=True), tools/sparse_points.py --refine), or any COLMAP model (`refine_model`, tools/bundle_adjust.py).  Kernels:
csrc/bundle.hip (the design: DESIGN.md, "Bundle adjustment"); tests/bundle_ref.py restates every stage in numpy and the device results equal it
entry for entry.  Intrinsics stay fixed.

Inputs.  cams fp64 [V,2,4,4] (keypoints' layout: extrinsic [R t], K = [[fx, s, cx], [0, fy, cy], [0, 0, 1]]); xyz fp64 [P,3]; the tracks' CSR
track_off int64 [P+1], track_view int32 [nnz], and obs_xy fp64 [nnz,2] (`observations(kp, tracks)` gathers it from Keypoints, `model_problem(model)`
from a COLMAP model dict); fixed_views: a bool mask [V] or a list of indices, default view 0.  With fewer than two fixed views the scale of the
scene is free (the cost still falls; comparisons against a truth need two).

The definition.  fp64, every product and sum its own operation in the order written, no FMA contraction; only + - * / sqrt, max, min and compares.
Equality with the restatement is equality of numbers: the sign of a zero is not part of it.

1. Residual of observation o (point j in view i, pose row-major R and t): q_k = ((R_k0 X_0 + R_k1 X_1) + R_k2 X_2) + t_k; u = q_0 / q_2, v = q_1 /
   q_2; r = (((fx u + s v) + cx) - x, (fy v + cy) - y).  q_2 <= 0 (or not a number) is "behind": at the initial parameters it raises ValueError
   (MVSDF_PS_ERR_BEHIND), at a trial step the cost term is +inf and the step is rejected.  A track shorter than 2 is INACTIVE with its
   observations: r = 0, cost term 0, A = B = 0; the point never moves.
2. Robust weight: s2 = r_0 r_0 + r_1 r_1, n = sqrt(s2); w = 1 if n <= delta else delta / n; cost term 0.5 s2 if n <= delta else delta (n - 0.5
   delta); residual and both Jacobians are multiplied by sqrt(w) (first-order IRLS).  loss_scale=None is delta = +inf: the same code path.
3. Jacobians for the local update q <- q + omega x q + upsilon: D = [[fx / q_2, s / q_2, -((fx u + s v) / q_2)], [0, fy / q_2, -((fy v) / q_2)]];
   A_e = (D_e2 q_1 - D_e1 q_2, D_e0 q_2 - D_e2 q_0, D_e1 q_0 - D_e0 q_1, D_e0, D_e1, D_e2) (2x6, e = 0, 1); B_el = (D_e0 R_0l + D_e1 R_1l) + D_e2
   R_2l (2x3); each entry then times sqrt(w).  The pose update is R <- E R, t <- E t + upsilon, rows as ((a + b) + c) (+ upsilon_k), with z = (w_0 w_0
   + w_1 w_1) + w_2 w_2, a(z) and b(z) the polynomials of sin t / t and (1 - cos t) / t^2 in z = t^2 by Horner from the highest term down over
   `rodrigues_table()` (coefficients (-1)^k / (2k+1)! and (-1)^k / (2k+2)!, k = 0 .. 9, factorials by repeated fp64 products), and E_kl = ((1 if k
   == l else 0) + a [w]x_kl) + b (w_k w_l - z if k == l else w_k w_l).  The table holds for t <= MVSDF_BA_MAX_THETA = 1 radian: a step with z > 1
   for any view counts as rejected.  Sine and cosine are never library calls.
4. Point blocks, sequentially over the track from 0.0: V_j,kl += B_0k B_0l + B_1k B_1l; g_j,k += B_0k r_0 + B_1k r_1.  Damped: diagonal entries
   V_kk + lambda max(V_kk, FLOOR), FLOOR = 1e-6.  Its inverse by the adjugate: det = (m00 (m11 m22 - m12 m12) - m01 (m01 m22 - m12 m02)) + m02
   (m01 m12 - m11 m02); inverse entries (m11 m22 - m12 m12, m02 m12 - m01 m22, m01 m12 - m02 m11, m00 m22 - m02 m02, m01 m02 - m00 m12, m00 m11
   - m01 m01) / det for (00, 01, 02, 11, 12, 22).  A block of an inactive point, or whose det is not finite and > 0, or with a non-finite inverse
   entry, gets the ZERO inverse: the point does not move and contributes nothing to the reduced system.  V^-1 a is ((i_k0 a_0 + i_k1 a_1) + i_k2 a_2).
5. Camera blocks: U_i,kl = tree of A_0k A_0l + A_1k A_1l, g_i,k = tree of A_0k r_0 + A_1k r_1 over the view's observations in the order of a stable
   by-view sort of the observation list.  A TREE is the canonical pairwise sum (poisson's): pad with +0.0 to a power of two, add adjacent pairs.
   Damped as the point blocks.  The inverse by LDL^T: d_j = U_jj - sum_(k<j) (L_jk L_jk) d_k, L_ij = (U_ij - sum_(k<j) (L_ik L_jk) d_k) / d_j,
   subtracting term after term; column c of the inverse: y_i = e_i - sum_(k<i) L_ik y_k, y_i / d_i, then from i = 5 down x_i = y_i - sum_(k>i,
   ascending) L_ki x_k.  A view MOVES iff it is not fixed, every d_j is finite and > 0 and the inverse is finite; for the others the inverse and
   the right-hand side are 0.  These inverses are the block-Jacobi preconditioner M^-1.
6. Reduced system S = U_l - W V_l^-1 W^T with W_o = A^T B never formed: W_o^T x = B^T (A x) with (A x)_e summed from 0.0 over k, and W_o y = A^T
   (B y) with (B y)_e = (B_e0 y_0 + B_e1 y_1) + B_e2 y_2 and entry k = A_0k t_0 + A_1k t_1.  y_j = V_l,j^-1 (sum over the track from 0.0 of W_o^T
   x_i); (S x)_i = (U_l,i x_i, each row summed from 0.0 over the columns) - tree over the view of W_o y_j; 0 for a view that does not move.
   b_i = (-g_i) + tree of W_o (V_l,j^-1 g_j).
7. PCG from x = 0: r = b, z = M^-1 r (rows summed from 0.0), p = z, rho = rho_0 = tree over the 6 V entries of r z; done at once unless rho_0 is
   finite and > 0.  An iteration: q = S p; sigma = tree of p q; done (x kept) unless sigma is finite and > 0; alpha = rho / sigma; x += alpha p; r
   -= alpha q; z = M^-1 r; rho' = tree of r z; p = z + (rho' / rho) p; done unless rho' > cg_tol^2 rho_0.  At most cg_iters iterations.
8. Step: dp_j = V_l,j^-1 ((-g_j) - sum over the track of W_o^T x_i), X + dp; poses by 3.  The trial cost is the tree over the nnz cost terms.
   Accepted iff no rotation beyond the bound, the trial cost is finite and < the cost (strict): lambda <- max(lambda / 10, lambda_min); else
   lambda <- min(10 lambda, lambda_max).  After an accepted step with cost - trial < ftol cost the call has converged and every later launch
   returns at once.  A whole call is enqueued without a host wait; reading the header (MVSDF_BA_H_*) is the one wait.

The stage functions each have their own C entry and are held to the restatement alone: `residuals`, `normal_blocks`, `schur_apply`,
`solve_reduced`, `apply_step`.  `bundle_adjust` composes them on the device; `refine_model` takes and returns a load_colmap_model dict.

NOT BUILT.  Poses from scratch (two-view geometry, resection, incremental mapping); refinement of intrinsics or distortion; a Schur-Jacobi
preconditioner; the second-order robust correction; covariance output.

ValueError before any launch: a dtype or shape other than the one named, an option out of range.  ValueError through the call's error bits: a count
outside the limits (MVSDF_BA_MAX_VIEWS views, MVSDF_BA_MAX_OBS observations), a non-finite input, offsets that do not ascend from 0 to nnz, a view
index outside [0, V), a point behind a camera at the start."""
import collections
import math

import numpy as np
import torch

from ._lib import check, lib, K, raise_for_bits, f64_from_bits, _header, _stream, _vp
from .cloud import _device
from .global_reg import _array

MAX_VIEWS, MAX_OBS, MAX_THETA, ROD_TERMS = K.MVSDF_BA_MAX_VIEWS, K.MVSDF_BA_MAX_OBS, float(K.MVSDF_BA_MAX_THETA), K.MVSDF_BA_ROD_TERMS
FLOOR = 1e-6

ERRORS = [(K.MVSDF_PS_ERR_SHAPE, ValueError, 'a count is outside the limits (views, points or observations)'),
          (K.MVSDF_PS_ERR_FINITE, ValueError, 'a camera entry, a coordinate or an observation is NaN or infinite'),
          (K.MVSDF_PS_ERR_INDEX, ValueError, 'track offsets do not ascend from 0 to nnz, or a view index is outside [0, V)'),
          (K.MVSDF_PS_ERR_BEHIND, ValueError, 'a point lies behind a camera that observes it')]

BundleResult = collections.namedtuple('BundleResult', 'cams xyz residuals cost0 cost iterations accepted cg_iterations lam')
Blocks = collections.namedtuple('Blocks', 'U gc V gp b lam ws sizes cams')


def rodrigues_table():
    """the coefficients of sin t / t and of (1 - cos t) / t^2 in t^2, ascending, fp64 [20]; the factorials by repeated fp64 products"""
    fact = [1.0]
    for k in range(1, 2 * ROD_TERMS + 2):
        fact.append(fact[-1] * float(k))
    sign = [1.0 if k % 2 == 0 else -1.0 for k in range(ROD_TERMS)]
    return np.array([sign[k] / fact[2 * k + 1] for k in range(ROD_TERMS)] + [sign[k] / fact[2 * k + 2] for k in range(ROD_TERMS)], dtype=np.float64)


def pose_arrays(cams):
    """cams [V,2,4,4] -> (pose [V,12]: R row-major then t, intr [V,5]: fx, s, cx, fy, cy), copies without arithmetic"""
    cams = np.asarray(cams, np.float64)
    pose = np.concatenate([cams[:, 0, :3, :3].reshape(-1, 9), cams[:, 0, :3, 3]], 1)
    Km = cams[:, 1]
    return np.ascontiguousarray(pose), np.ascontiguousarray(np.stack([Km[:, 0, 0], Km[:, 0, 1], Km[:, 0, 2], Km[:, 1, 1], Km[:, 1, 2]], 1))


def cams_with(cams, pose):
    """cams with the extrinsics of pose [V,12]"""
    out = np.array(cams, np.float64)
    out[:, 0, :3, :3] = pose[:, :9].reshape(-1, 3, 3)
    out[:, 0, :3, 3] = pose[:, 9:]
    return out


def observations(kp, tracks):
    """obs_xy fp64 [nnz,2]: the keypoint positions under the entries of tracks = (track_off, track_view, track_kp), on the device of kp.xy"""
    xy = torch.as_tensor(kp.xy)
    view, k = torch.as_tensor(tracks[1]).to(xy.device).long(), torch.as_tensor(tracks[2]).to(xy.device).long()
    return xy[torch.as_tensor(kp.view_off).to(xy.device)[view] + k].contiguous()


def model_problem(model):
    """a COLMAP model dict -> (ids, cams [V,2,4,4], xyz, track_off, track_view, obs_xy) as numpy: the views are the images by ascending id"""
    from .datasets import colmap
    ids, _, cams, view = colmap.model_views(model)
    pts = model['points']
    obs = np.zeros((len(view), 2))
    for o, (iid, k) in enumerate(zip(pts['track_image'], pts['track_point2D'])):
        obs[o] = model['images'][int(iid)]['xys'][int(k)]
    return ids, np.asarray(cams, np.float64), np.asarray(pts['xyz'], np.float64).reshape(-1, 3), np.asarray(pts['track_off'], np.int64), view, obs


def _number(x, name, what, low=0.0, inf=False):
    x = float(x)
    if not (x >= low and (inf or math.isfinite(x))):
        raise ValueError('%s: %s must be a%s number >= %g, got %r' % (what, name, '' if inf else ' finite', low, x))
    return x


def _count(x, name, what, high):
    if isinstance(x, bool) or int(x) != x or not 0 <= int(x) <= high:
        raise ValueError('%s: %s must be an integer in 0 .. %d, got %r' % (what, name, high, x))
    return int(x)


def _delta(loss_scale, what):
    if loss_scale is None:
        return math.inf
    d = float(loss_scale)
    if not d > 0:
        raise ValueError('%s: loss_scale must be None or > 0, got %r' % (what, loss_scale))
    return d


Problem = collections.namedtuple('Problem', 'cams pose intr xyz off view obs fixed V P nnz dev')


def _problem(cams, xyz, track_off, track_view, obs_xy, fixed_views, what):
    """shapes and dtypes checked, everything on the device"""
    c = np.asarray(cams.cpu() if isinstance(cams, torch.Tensor) else cams)
    if c.dtype != np.float64 or c.ndim != 4 or c.shape[1:] != (2, 4, 4) or c.shape[0] < 1:
        raise ValueError('%s: cams must be float64 [V, 2, 4, 4], got %s %s' % (what, c.dtype, c.shape))
    V = c.shape[0]
    xyz = _device(_array(xyz, torch.float64, (None, 3), what, 'xyz')).contiguous()
    dev, P = xyz.device, xyz.shape[0]
    off = _array(track_off, torch.int64, (P + 1,), what, 'track_off').to(dev).contiguous()
    view = _array(track_view, torch.int32, (None,), what, 'track_view').to(dev).contiguous()
    nnz = view.shape[0]
    obs = _array(obs_xy, torch.float64, (nnz, 2), what, 'obs_xy').to(dev).contiguous()
    f = np.asarray(fixed_views.cpu() if isinstance(fixed_views, torch.Tensor) else fixed_views)
    if f.dtype == bool:
        if f.shape != (V,):
            raise ValueError('%s: a fixed_views mask must have shape [%d], got %s' % (what, V, f.shape))
        mask = f.copy()
    else:
        if f.ndim != 1 or (f.size and (f.dtype.kind not in 'iu' or f.min() < 0 or f.max() >= V)):
            raise ValueError('%s: fixed_views must be a bool mask or indices in [0, %d)' % (what, V))
        mask = np.zeros(V, bool)
        mask[f.astype(np.int64)] = True
    pose, intr = pose_arrays(c)
    return Problem(c, torch.from_numpy(pose).to(dev), torch.from_numpy(intr).to(dev), xyz, off, view, obs,
                   torch.from_numpy(mask.astype(np.uint8)).to(dev), V, P, nnz, dev)


def _workspace(pr):
    size = lib().mvsdf_ba_workspace_bytes(pr.V, pr.P, pr.nnz)
    return torch.empty(max(size, 512), dtype=torch.uint8, device=pr.dev)


def _head(ws, what):
    h = _header(ws, K.MVSDF_BA_H_WORDS)
    raise_for_bits(h[K.MVSDF_BA_H_ERR], what, ERRORS)
    return h


def residuals(cams, xyz, track_off, track_view, obs_xy, loss_scale=None, trial=False):
    """stage 1 and 2 -> (r fp64 [nnz,2] unweighted, cost terms fp64 [nnz], cost).  trial: behind gives +inf, not ValueError"""
    what = 'residuals'
    pr = _problem(cams, xyz, track_off, track_view, obs_xy, (), what)
    delta = _delta(loss_scale, what)
    ws = _workspace(pr)
    r = torch.empty(pr.nnz, 2, dtype=torch.float64, device=pr.dev)
    terms = torch.empty(pr.nnz, dtype=torch.float64, device=pr.dev)
    check(lib().mvsdf_ba_residuals(_vp(pr.pose), _vp(pr.intr), _vp(pr.xyz), _vp(pr.off), _vp(pr.view), _vp(pr.obs), pr.V, pr.P, pr.nnz, delta,
                                   1 if trial else 0, _vp(ws), ws.numel(), _vp(r), _vp(terms), _stream(ws)), 'mvsdf_ba_residuals')
    h = _head(ws, what)
    return r, terms, f64_from_bits(h[K.MVSDF_BA_H_COST])


def normal_blocks(cams, xyz, track_off, track_view, obs_xy, fixed_views=(0,), lam=1e-4, loss_scale=None):
    """stages 3 to 5 at damping lam -> Blocks(U [V,6,6], gc [V,6], V [P,3,3], gp [P,3] undamped, b [V,6] the reduced right-hand side, ...): what
    schur_apply, solve_reduced and apply_step take"""
    what = 'normal_blocks'
    pr = _problem(cams, xyz, track_off, track_view, obs_xy, fixed_views, what)
    delta, lam = _delta(loss_scale, what), _number(lam, 'lam', what)
    ws = _workspace(pr)
    z = lambda *s: torch.empty(*s, dtype=torch.float64, device=pr.dev)  # noqa: E731  (k_ba_export_blocks writes every entry of all five)
    U, gc, Vb, gp, b = z(pr.V, 6, 6), z(pr.V, 6), z(pr.P, 3, 3), z(pr.P, 3), z(pr.V, 6)
    check(lib().mvsdf_ba_blocks(_vp(pr.pose), _vp(pr.intr), _vp(pr.xyz), _vp(pr.off), _vp(pr.view), _vp(pr.obs), _vp(pr.fixed), pr.V, pr.P, pr.nnz,
                                delta, lam, FLOOR, _vp(ws), ws.numel(), _vp(U), _vp(gc), _vp(Vb), _vp(gp), _vp(b), _stream(ws)), 'mvsdf_ba_blocks')
    _head(ws, what)
    return Blocks(U, gc, Vb, gp, b, lam, ws, (pr.V, pr.P, pr.nnz), pr.cams)


def _vec(x, blocks, what):
    return _array(x, torch.float64, (blocks.sizes[0], 6), what, 'x').to(blocks.ws.device).contiguous()


def schur_apply(blocks, x):
    """stage 6 -> S x fp64 [V,6]"""
    what = 'schur_apply'
    x = _vec(x, blocks, what)
    out = torch.empty_like(x)
    check(lib().mvsdf_ba_schur(*blocks.sizes, _vp(blocks.ws), blocks.ws.numel(), _vp(x), _vp(out), _stream(x)), 'mvsdf_ba_schur')
    _head(blocks.ws, what)
    return out


def solve_reduced(blocks, cg_iters=64, cg_tol=1e-8, b=None):
    """stage 7 -> (x fp64 [V,6], iterations run).  b: another right-hand side than the blocks' own"""
    what = 'solve_reduced'
    cg_iters, cg_tol = _count(cg_iters, 'cg_iters', what, K.MVSDF_BA_MAX_CG), _number(cg_tol, 'cg_tol', what)
    b = None if b is None else _vec(b, blocks, what)
    x = torch.empty(blocks.sizes[0], 6, dtype=torch.float64, device=blocks.ws.device)
    check(lib().mvsdf_ba_solve(*blocks.sizes, _vp(b), cg_iters, cg_tol, _vp(blocks.ws), blocks.ws.numel(), _vp(x), _stream(x)), 'mvsdf_ba_solve')
    return x, _head(blocks.ws, what)[K.MVSDF_BA_H_CG]


def apply_step(blocks, x):
    """stage 8's parameters -> (cams [V,2,4,4] numpy, xyz fp64 [P,3], whether every rotation stayed within the bound)"""
    what = 'apply_step'
    x = _vec(x, blocks, what)
    dev = x.device
    pose = torch.empty(blocks.sizes[0], 12, dtype=torch.float64, device=dev)
    xyz = torch.empty(blocks.sizes[1], 3, dtype=torch.float64, device=dev)
    rod = torch.from_numpy(rodrigues_table()).to(dev)
    check(lib().mvsdf_ba_step(*blocks.sizes, _vp(rod), _vp(blocks.ws), blocks.ws.numel(), _vp(x), _vp(pose), _vp(xyz), _stream(x)), 'mvsdf_ba_step')
    h = _head(blocks.ws, what)
    return cams_with(blocks.cams, pose.cpu().numpy()), xyz, h[K.MVSDF_BA_H_ITER] == 0


def bundle_adjust(cams, xyz, track_off, track_view, obs_xy, fixed_views=(0,), iterations=10, lambda0=1e-4, lambda_min=1e-10, lambda_max=1e10,
                  cg_iters=64, cg_tol=1e-8, ftol=1e-9, loss_scale=None):
    """the whole definition -> BundleResult(cams numpy [V,2,4,4], xyz fp64 [P,3] and residuals fp64 [nnz,2] on the device, cost0, cost, iterations,
    accepted, cg_iterations, lam).  Enqueued without a host wait; reading the header is the one wait."""
    what = 'bundle_adjust'
    pr = _problem(cams, xyz, track_off, track_view, obs_xy, fixed_views, what)
    delta = _delta(loss_scale, what)
    iterations = _count(iterations, 'iterations', what, K.MVSDF_BA_MAX_ITERATIONS)
    cg_iters, cg_tol, ftol = _count(cg_iters, 'cg_iters', what, K.MVSDF_BA_MAX_CG), _number(cg_tol, 'cg_tol', what), _number(ftol, 'ftol', what)
    lambda_min, lambda0, lambda_max = _number(lambda_min, 'lambda_min', what), _number(lambda0, 'lambda0', what), _number(lambda_max, 'lambda_max', what)
    if not 0 < lambda_min <= lambda0 <= lambda_max:
        raise ValueError('%s: 0 < lambda_min <= lambda0 <= lambda_max must hold, got %r, %r, %r' % (what, lambda_min, lambda0, lambda_max))
    ws = _workspace(pr)
    pose = torch.empty(pr.V, 12, dtype=torch.float64, device=pr.dev)
    out = torch.empty(pr.P, 3, dtype=torch.float64, device=pr.dev)
    r = torch.empty(pr.nnz, 2, dtype=torch.float64, device=pr.dev)
    terms = torch.empty(pr.nnz, dtype=torch.float64, device=pr.dev)
    rod = torch.from_numpy(rodrigues_table()).to(pr.dev)
    check(lib().mvsdf_ba_adjust(_vp(pr.pose), _vp(pr.intr), _vp(pr.xyz), _vp(pr.off), _vp(pr.view), _vp(pr.obs), _vp(pr.fixed), pr.V, pr.P, pr.nnz,
                                _vp(rod), delta, iterations, lambda0, lambda_min, lambda_max, FLOOR, cg_iters, cg_tol, ftol, _vp(ws), ws.numel(),
                                _vp(pose), _vp(out), _vp(r), _vp(terms), _stream(ws)), 'mvsdf_ba_adjust')
    h = _head(ws, what)
    return BundleResult(cams_with(pr.cams, pose.cpu().numpy()), out, r, f64_from_bits(h[K.MVSDF_BA_H_COST0]), f64_from_bits(h[K.MVSDF_BA_H_COST]),
                        h[K.MVSDF_BA_H_ITER], h[K.MVSDF_BA_H_ACCEPTED], h[K.MVSDF_BA_H_CG], f64_from_bits(h[K.MVSDF_BA_H_LAMBDA]))


def quaternion(R):
    """(qw, qx, qy, qz) of a rotation matrix, numpy fp64: the branch with the largest of (trace, R00, R11, R22) (the first at a tie); with s = 2
    sqrt(1 + that combination) the leading component is s / 4 and the others differences or sums of off-diagonal pairs over s; qw >= 0 by a
    final change of sign; not normalised further"""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    c = int(np.argmax([t, R[0, 0], R[1, 1], R[2, 2]]))
    if c == 0:
        s = 2.0 * math.sqrt(1.0 + t)
        q = [s / 4, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif c == 1:
        s = 2.0 * math.sqrt(((1.0 + R[0, 0]) - R[1, 1]) - R[2, 2])
        q = [(R[2, 1] - R[1, 2]) / s, s / 4, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif c == 2:
        s = 2.0 * math.sqrt(((1.0 + R[1, 1]) - R[0, 0]) - R[2, 2])
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, s / 4, (R[1, 2] + R[2, 1]) / s]
    else:
        s = 2.0 * math.sqrt(((1.0 + R[2, 2]) - R[0, 0]) - R[1, 1])
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, s / 4]
    q = np.array(q, dtype=np.float64)
    return -q if q[0] < 0 else q


def refine_model(model, report=None, **kw):
    """a load_colmap_model dict -> the same dict with new q / t per image, new points['xyz'], and points['error'] = the mean reprojection error
    (pixels) of each point over its observations, summed from 0.0 in track order; kw: bundle_adjust's options.  The views are the images by
    ascending id; fixed_views counts in that order."""
    ids, cams, xyz, off, view, obs = model_problem(model)
    if len(xyz) == 0 or len(view) == 0:
        raise ValueError('refine_model: the model holds no point with observations')
    res = bundle_adjust(cams, xyz, off, view, obs, **kw)
    r = res.residuals.cpu().numpy()
    e = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1])
    length = np.diff(off)
    err = np.zeros(len(xyz))
    for k in range(int(length.max())):
        sel = length > k
        err[sel] = err[sel] + e[off[:-1][sel] + k]
    err = err / np.maximum(length, 1)
    images = dict(model['images'])
    for i, iid in enumerate(ids):
        E = res.cams[i, 0]
        images[iid] = dict(images[iid], q=quaternion(E[:3, :3]), t=np.ascontiguousarray(E[:3, 3]))
    points = dict(model['points'], xyz=res.xyz.cpu().numpy(), error=err)
    if report is not None:
        report.update(cost0=res.cost0, cost=res.cost, iterations=res.iterations, accepted=res.accepted, cg_iterations=res.cg_iterations,
                      lam=res.lam, observations=len(view), rms0=math.sqrt(2.0 * res.cost0 / max(len(view), 1)),
                      rms=math.sqrt(2.0 * res.cost / max(len(view), 1)))
    return {'cameras': model['cameras'], 'images': images, 'points': points}
