"""The normals of mvsdf_amd/fusion.py (depth_normals) restated in vectorised numpy (test helper only): fp64, every product and sum a separate numpy
operation in the order the definition writes it.  Written from that module's doc, not from the kernel; the matrices are fusion_ref's."""
import numpy as np

from fusion_ref import _row, matrices


def depth_normals(fused_depths, view, pixel, cams, jump=0.05):
    """fused_depths fp32 [V,H,W], view / pixel int [N] -> normals fp64 [N,3]"""
    depths = np.asarray(fused_depths, np.float32).astype(np.float64)
    V, H, W = depths.shape
    _, Pinv = matrices(cams)
    Pinv = np.stack(Pinv)
    centre = Pinv[:, :3, 3] / Pinv[:, 3, 3][:, None]
    r, p = np.asarray(view, np.int64), np.asarray(pixel, np.int64)
    y, x = p // W, p % W
    T = Pinv[r]                                                             # [N,4,4]

    def Q(xx, yy, dd):
        q0, q1 = (xx + 0.5) * dd, (yy + 0.5) * dd
        return np.stack([_row(T[:, c].T, q0, q1, dd, 1.0) for c in range(3)], 1)

    with np.errstate(all='ignore'):
        d = depths[r, y, x]
        qc = Q(x, y, d)

        def tangent(dx, dy):
            xl, yl, xh, yh = x - dx, y - dy, x + dx, y + dy
            in_lo, in_hi = (xl >= 0) & (yl >= 0), (xh < W) & (yh < H)
            dl = depths[r, np.where(in_lo, yl, 0), np.where(in_lo, xl, 0)]
            dh = depths[r, np.where(in_hi, yh, 0), np.where(in_hi, xh, 0)]
            lo = in_lo & (dl > 0) & (np.abs(dl - d) <= jump * d)
            hi = in_hi & (dh > 0) & (np.abs(dh - d) <= jump * d)
            ql, qh = Q(xl, yl, dl), Q(xh, yh, dh)
            t = np.where(hi[:, None], qh, qc) - np.where(lo[:, None], ql, qc)
            return t, lo | hi

        a, has_a = tangent(1, 0)
        b, has_b = tangent(0, 1)
        m = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
        ln = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
        ok = has_a & has_b & (ln > 0) & np.isfinite(ln)
        n = m / ln[:, None]
        c = centre[r] - qc
        flip = ((n[:, 0] * c[:, 0] + n[:, 1] * c[:, 1]) + n[:, 2] * c[:, 2]) < 0
        n = np.where(flip[:, None], -n, n)
        return np.where(ok[:, None], n, 0.0)
