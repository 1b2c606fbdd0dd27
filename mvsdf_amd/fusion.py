"""Depth-map fusion on the device: step 1 of the reference's BYOD.md (the author's separate pcd-fusion script: probability filter, geometric
consistency between a view and its source views, averaged depth, back-projection to one coloured cloud all_torch.ply).  Kernels:
csrc/fusion.hip (the design: DESIGN.md); tests/fusion_ref.py restates every step in numpy.

Inputs: cams fp64 [V,2,4,4] as utils.io.load_cam returns them, depths fp32 [V,H,W], probs fp32 [V,3,H,W] or None, pairs a list of V lists of
view indices (nearest first), images uint8 [V,H,W,3] at depth-map size or None.

The definition (fp64 throughout, in the order written, no FMA contraction; fp32 inputs are promoted exactly):

- Matrices (host, numpy fp64, passed to the kernels as data).  P_v = K4_v @ E_v with E_v = cams[v,0] and K4_v the 4x4 identity with
  cams[v,1,:3,:3] in its corner; Pinv_v = np.linalg.inv(P_v); T_rs = P_s @ Pinv_r.  A matrix-vector product is, per row,
  ((t0*q0 + t1*q1) + t2*q2) + t3*q3.
- Pixel convention: the reference's (my_utils.get_pixel_grids, grid_sample(align_corners=False)): pixel (x, y) sits at image coordinate
  (x + 0.5, y + 0.5).
- Step 1, probability mask.  m = (prob1 > fp32(t1)) & (prob2 > fp32(t2)) & (prob3 > fp32(t3)) & isfinite(depth) & (depth > 0) (fp32 compares,
  as vismvsnet2mvsdf.py:53); probs=None: only the depth conditions.  masked_depth = depth where m, else 0.  Everything below reads masked depths.
- Step 2, per reference pixel with d = masked_depth > 0 and per source s among the first `view` entries of pairs[r], in that order:
  X = x + 0.5, Y = y + 0.5; p = T_rs (X*d, Y*d, d, 1); reject unless p2 > 0; u = p0/p2 - 0.5, v = p1/p2 - 0.5; reject unless 0 <= u <= W-1 and
  0 <= v <= H-1; x0 = min(floor(u), W-2), y0 likewise, fx = u - x0, fy = v - y0; the four texels d00 d01 / d10 d11 of the source's masked depth
  at rows y0, y0+1 and columns x0, x0+1 must all be > 0, else reject (a hole never bleeds a zero into a depth);
  ds = (d00*(1-fx) + d01*fx)*(1-fy) + (d10*(1-fx) + d11*fx)*fy; b = T_sr ((u+0.5)*ds, (v+0.5)*ds, ds, 1); reject unless b2 > 0;
  ex = b0/b2 - X, ey = b1/b2 - Y, zr = b2.  The source is consistent iff ex*ex + ey*ey < pix_thresh*pix_thresh and |zr - d| < dep_thresh * d.
  (H or W below 2: ValueError.)
- Step 3.  n = number of consistent sources (counts); the pixel is kept iff n >= vthresh; df = (d + zr_1 + zr_2 + ...) / (n + 1), the consistent
  sources' zr added in pair order; fused_depth = fp32(df) if kept else 0.
- Step 4.  The point of a kept pixel is rows 0..2 of Pinv_r (X*df, Y*df, df, 1); its colour is images[r, y, x].  Points come out in
  (view, y, x) order.  bbox() is the exact min / max per axis.

Normals (depth_normals, or fuse_depths(normals=True); BYOD.md passes --no_normal, so this is this project's own definition): one per fused
point, from the fused depth map of the point's view.
- For point i in view r at pixel (x, y): d(x, y) = fp64(fused_depths[r, y, x]); Q(x, y) = rows 0..2 of Pinv_r applied to (X d, Y d, d, 1) by the row
  product above, X = x + 0.5, Y = y + 0.5.
- A neighbour pixel is usable iff it is inside the image, its depth d' is > 0 and |d' - d| <= jump * d: no tangent is taken across a hole or a
  depth edge (jump = inf switches the edge rule off).
- tx = Q(x+1, y) - Q(x-1, y) if both are usable, else Q(x+1, y) - Q(x, y) if the right one is, else Q(x, y) - Q(x-1, y) if the left one is, else
  there is none.  ty is the same with y+1 and y-1.
- m = tx x ty = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0) for a = tx, b = ty; len = sqrt((m0 m0 + m1 m1) + m2 m2).
- The normal is (0, 0, 0) when a tangent is missing or len is 0 or not finite.  Otherwise n = m / len, negated when ((n0 c0 + n1 c1) + n2 c2) < 0
  for c = C_r - Q(x, y): it looks at the camera.  C_r = Pinv_r[:3, 3] / Pinv_r[3, 3] is the camera centre (host, passed as data).
It reads only fused_depths, view, pixel and the cameras, so it follows cloud.clean_fused, which zeroes the removed pixels.  A point is without a
normal when both neighbours along an image axis are holes or rejected pixels, so the share follows the holes of the fused maps, not the jump rule:
on the scenes of tests/mvs_scene.py (6 views, 20 x 28 / 37 x 53) it is 0.6 % / 0.7 % for the clean sphere, 18.8 % / 11.7 % with 10 % of the input
texels punched out, and 86 % / 89 % for the default scene with bumps and per-view scale errors, whose cloud is a sparse 199 / 495 points;
jump = inf gives the same shares to within 0.5 points.  What jump = 0.05 buys is at the silhouette: the largest angle to the true normal on the
clean sphere at 37 x 53 is 16.9 degrees with it and 90.6 degrees without.  The record gives no reason to move the default.

Not built: voxel down-sampling (--downsample -1), the script's median fusion, --show_result, normals for clouds that come without depth maps.  The
script's text is not available to this project, so its agreement with this definition beyond BYOD.md's description is not claimed.
"""
import numpy as np
import torch

from ._lib import check, K, lib, raise_for_bits, _header, _stream, _vp


class Fused:
    """The result of fuse_depths: points fp64 [N,3] (world), colors uint8 [N,3] or None, view int32 [N], pixel int32 [N] (y*W + x),
    masked_depths fp32 [V,H,W], fused_depths fp32 [V,H,W] (0 where rejected), counts int32 [V,H,W]; all on the device.  normals: fp64 [N,3]
    (depth_normals) when they were asked for, else None."""

    def __init__(self, points, colors, view, pixel, masked_depths, fused_depths, counts, normals=None):
        self.points, self.colors, self.view, self.pixel = points, colors, view, pixel
        self.masked_depths, self.fused_depths, self.counts = masked_depths, fused_depths, counts
        self.normals = normals

    def __len__(self):
        return self.points.shape[0]

    def bbox(self):
        """(lo, hi): the exact minimum / maximum of the points per axis, fp64 [3] each on the device (NaN for an empty cloud)"""
        if len(self) == 0:
            nan = torch.full((3,), float('nan'), dtype=torch.float64, device=self.points.device)
            return nan, nan.clone()
        return self.points.amin(0), self.points.amax(0)


def projection_matrices(cams):
    """-> (P, Pinv) fp64 numpy [V,4,4] of the definition's matrices"""
    cams = np.asarray(cams, dtype=np.float64)
    P, Pinv = np.empty((len(cams), 4, 4)), np.empty((len(cams), 4, 4))
    for v, cam in enumerate(cams):                                          # one 2-d product / inverse at a time, as the definition writes them
        K4 = np.eye(4)
        K4[:3, :3] = cam[1, :3, :3]
        P[v] = K4 @ cam[0]
        Pinv[v] = np.linalg.inv(P[v])
    return P, Pinv


# the error bits of a fusion call (csrc/fusion.hip), in the order they are looked at
ERRORS = [(K.MVSDF_FU_ERR_FINITE, ValueError, 'a camera entry or a threshold is NaN or infinite'),
          (K.MVSDF_FU_ERR_PAIR, ValueError, 'a pair index is outside [0, V)'),
          (K.MVSDF_FU_ERR_VIEW, ValueError, 'view must be >= 1'),
          (K.MVSDF_FU_ERR_SHAPE, ValueError, 'shapes disagree or are out of range (V >= 1, H and W >= 2)'),
          (K.MVSDF_FU_ERR_INDEX, ValueError, 'a view or pixel index of a point lies outside the depth maps')]


def _jump(jump, what):
    jump = float(jump)
    if np.isnan(jump) or jump < 0:
        raise ValueError('%s: jump must be >= 0 (inf switches the rule off), got %r' % (what, jump))
    return jump


def depth_normals(fused, cams, jump=0.05):
    """The module's definition of the normals -> fp64 [N,3] on the device, aligned with fused.points (a Fused of fuse_depths or cloud.clean_fused)."""
    what = 'depth_normals'
    jump = _jump(jump, what)
    d = fused.fused_depths
    V, H, W = d.shape
    cams = np.asarray(cams.cpu() if isinstance(cams, torch.Tensor) else cams, dtype=np.float64)
    if cams.shape != (V, 2, 4, 4):
        raise ValueError('%s: cams must be [V, 2, 4, 4] for V = %d depth maps, got shape %s' % (what, V, cams.shape))
    if not np.isfinite(cams).all():
        raise ValueError('%s: a camera entry is NaN or infinite' % what)
    n = fused.points.shape[0]
    if fused.view.shape != (n,) or fused.pixel.shape != (n,):
        raise ValueError('%s: view and pixel must be [N] for N = %d points' % (what, n))
    try:
        _, Pinv = projection_matrices(cams)
    except np.linalg.LinAlgError as e:
        raise ValueError('%s: a camera has a singular projection' % what) from e
    mats = np.empty((V, 19), np.float64)
    mats[:, :16] = Pinv.reshape(V, 16)
    with np.errstate(all='ignore'):
        mats[:, 16:] = Pinv[:, :3, 3] / Pinv[:, 3, 3][:, None]
    if not np.isfinite(mats).all():
        raise ValueError('%s: a camera has no finite centre' % what)
    normals = torch.empty(n, 3, dtype=torch.float64, device=d.device)
    if n == 0:
        return normals
    d = d.contiguous()
    view, pixel = fused.view.contiguous(), fused.pixel.contiguous()
    size = lib().mvsdf_fusion_normals_workspace_bytes(V)
    ws = torch.empty(size, dtype=torch.uint8, device=d.device)
    check(lib().mvsdf_fusion_normals(_vp(d), V, H, W, _vp(view), _vp(pixel), n, mats.ctypes.data, jump, _vp(ws), size, _vp(normals), _stream(d)),
          'mvsdf_fusion_normals')
    raise_for_bits(_header(ws, K.MVSDF_RES_H_WORDS)[K.MVSDF_RES_H_ERR], what, ERRORS)   # the one wait of the call; mats lives until here
    return normals


def fuse_depths(cams, depths, pairs, probs=None, images=None, pthresh=(0.8, 0.7, 0.8), view=10, vthresh=2, pix_thresh=1.0, dep_thresh=0.01,
                normals=False, normal_jump=0.05):
    """The module's definition -> Fused.  Device tensors are used where they are (the stream is theirs); numpy / CPU input is copied to the GPU.
    normals=True fills Fused.normals (depth_normals with jump = normal_jump); every other output is the same either way."""
    what = 'fuse_depths'
    if normals:
        _jump(normal_jump, what)
    d = torch.as_tensor(depths)
    if d.dim() != 3:
        raise ValueError('%s: depths must be [V, H, W], got shape %s' % (what, tuple(d.shape)))
    V, H, W = d.shape
    dev = d.device if d.is_cuda else torch.device('cuda')
    cams = np.asarray(cams.cpu() if isinstance(cams, torch.Tensor) else cams, dtype=np.float64)
    if cams.shape != (V, 2, 4, 4):
        raise ValueError('%s: cams must be [V, 2, 4, 4] for V = %d depth maps, got shape %s' % (what, V, cams.shape))
    if len(pairs) != V:
        raise ValueError('%s: pairs must hold one list per view (%d), got %d' % (what, V, len(pairs)))
    if H < 2 or W < 2 or V < 1:
        raise ValueError('%s: depth maps must be at least 2 x 2 (and V >= 1), got %d views of %d x %d' % (what, V, H, W))
    view, vthresh = int(view), int(vthresh)
    if view < 1:
        raise ValueError('%s: view must be >= 1' % what)
    if not np.isfinite(cams).all():
        raise ValueError('%s: a camera entry is NaN or infinite' % what)
    th = np.asarray([float(pix_thresh), float(dep_thresh)])
    if not np.isfinite(th).all():
        raise ValueError('%s: pix_thresh and dep_thresh must be finite' % what)
    pairs = [[int(s) for s in p][:view] for p in pairs]
    if any(s < 0 or s >= V for p in pairs for s in p):
        raise ValueError('%s: a pair index is outside [0, %d)' % (what, V))
    p = None
    if probs is not None:
        p = torch.as_tensor(probs)
        if tuple(p.shape) != (V, 3, H, W):
            raise ValueError('%s: probs must be [V, 3, H, W] = %s, got shape %s' % (what, (V, 3, H, W), tuple(p.shape)))
        p = p.to(dev, torch.float32).contiguous()
    img = None
    if images is not None:
        img = torch.as_tensor(images)
        if tuple(img.shape) != (V, H, W, 3) or img.dtype != torch.uint8:
            raise ValueError('%s: images must be uint8 [V, H, W, 3] = %s, got %s %s' % (what, (V, H, W, 3), img.dtype, tuple(img.shape)))
        img = img.to(dev).contiguous()
    d = d.to(dev, torch.float32).contiguous()
    try:
        P, Pinv = projection_matrices(cams)
    except np.linalg.LinAlgError as e:
        raise ValueError('%s: a camera has a singular projection' % what) from e
    off = np.zeros(V + 1, np.int32)
    off[1:] = np.cumsum([len(q) for q in pairs])
    src = np.asarray([s for q in pairs for s in q], np.int32)
    npairs = len(src)
    mats = np.empty(npairs * 32 + V * 16, np.float64)
    k = 0
    for r, q in enumerate(pairs):                                           # T_rs, T_sr per pair slot
        for s in q:
            mats[k * 32:k * 32 + 16] = (P[s] @ Pinv[r]).reshape(-1)
            mats[k * 32 + 16:k * 32 + 32] = (P[r] @ Pinv[s]).reshape(-1)
            k += 1
    mats[npairs * 32:] = Pinv.reshape(-1)
    pt = np.asarray(pthresh, np.float32).reshape(3)
    size = lib().mvsdf_fusion_workspace_bytes(V, H, W, npairs)
    if size == 0:
        raise ValueError('%s: %d views of %d x %d are beyond the limits (V*H*W <= 2^40, H*W < 2^31)' % (what, V, H, W))
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    masked = torch.empty(V, H, W, dtype=torch.float32, device=dev)
    fused = torch.empty(V, H, W, dtype=torch.float32, device=dev)
    counts = torch.empty(V, H, W, dtype=torch.int32, device=dev)
    st = _stream(d)
    check(lib().mvsdf_fusion_fuse(_vp(d), _vp(p), pt.ctypes.data, V, H, W, off.ctypes.data, src.ctypes.data if npairs else None, mats.ctypes.data,
                                  view, vthresh, float(pix_thresh), float(dep_thresh), _vp(ws), size, _vp(masked), _vp(fused), _vp(counts), st),
          'mvsdf_fusion_fuse')
    total, err = _header(ws, K.MVSDF_RES_H_WORDS)   # the one wait of the call; off / src / mats / pt live until here
    raise_for_bits(err, what, ERRORS)
    points = torch.empty(total, 3, dtype=torch.float64, device=dev)
    colors = torch.empty(total, 3, dtype=torch.uint8, device=dev) if img is not None else None
    vw = torch.empty(total, dtype=torch.int32, device=dev)
    px = torch.empty(total, dtype=torch.int32, device=dev)
    if total:
        check(lib().mvsdf_fusion_emit(_vp(img), V, H, W, npairs, _vp(ws), size, _vp(points), _vp(colors), _vp(vw), _vp(px), total, st),
              'mvsdf_fusion_emit')
    out = Fused(points, colors, vw, px, masked, fused, counts)
    if normals:
        out.normals = depth_normals(out, cams, normal_jump)
    return out


def save_points(path, points, colors=None, normals=None):
    """A binary little-endian PLY point cloud: float x y z (+ float nx ny nz) (+ uchar red green blue); chamfer.load_points and
    chamfer.load_oriented_points read it back."""
    pts = torch.as_tensor(points).detach().cpu().numpy() if isinstance(points, torch.Tensor) else np.asarray(points)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError('save_points: points must be [N, 3], got shape %s' % (pts.shape,))
    fields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
    head = ['ply', 'format binary_little_endian 1.0', 'element vertex %d' % len(pts)] + ['property float %s' % k for k in 'xyz']
    if normals is not None:
        nrm = torch.as_tensor(normals).detach().cpu().numpy() if isinstance(normals, torch.Tensor) else np.asarray(normals)
        if nrm.shape != pts.shape:
            raise ValueError('save_points: normals must be [N, 3] for N points')
        fields += [('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4')]
        head += ['property float n%s' % k for k in 'xyz']
    if colors is not None:
        col = torch.as_tensor(colors).detach().cpu().numpy() if isinstance(colors, torch.Tensor) else np.asarray(colors)
        if col.shape != pts.shape or col.dtype != np.uint8:
            raise ValueError('save_points: colors must be uint8 [N, 3] for N points')
        fields += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
        head += ['property uchar red', 'property uchar green', 'property uchar blue']
    vert = np.empty(len(pts), dtype=fields)
    for i, k in enumerate('xyz'):
        vert[k] = pts[:, i]
    if normals is not None:
        for i, k in enumerate(('nx', 'ny', 'nz')):
            vert[k] = nrm[:, i]
    if colors is not None:
        for i, k in enumerate(('red', 'green', 'blue')):
            vert[k] = col[:, i]
    with open(path, 'wb') as fh:
        fh.write('\n'.join(head + ['end_header', '']).encode('ascii'))
        fh.write(vert.tobytes())
