"""The TSDF integration of mvsdf_amd/tsdf.py and the masked marching cubes of mesh.marching_cubes_masked restated in vectorised numpy (test helper
only).  The integration is fp64 with every product and sum a separate numpy operation in the order the definition writes it, so nothing is
contracted; the extraction follows tests/mc_ref.py (its table and edge owners are imported) with the mask's rules added.  Written from the two docs,
not from the kernels."""
import numpy as np

import mc_ref


def matrices(cams):
    out = []
    for cam in np.asarray(cams, np.float64):
        K4 = np.eye(4)
        K4[:3, :3] = cam[1, :3, :3]
        out.append(K4 @ cam[0])
    return out


def _row(t, q0, q1, q2, q3):
    return ((t[0] * q0 + t[1] * q1) + t[2] * q2) + t[3] * q3


def _holds(d):
    return np.isfinite(d) & (d > 0)


def integrate(cams, depths, origin, voxel, dims, trunc=None, jump=None, min_views=1, views=None):
    """-> dict: tsdf fp32, weight int32, valid bool, each [Nx,Ny,Nz]"""
    depths = np.asarray(depths, np.float32)
    V, H, W = depths.shape
    h = float(voxel)
    trunc = 4.0 * h if trunc is None else float(trunc)
    jump = trunc if jump is None else float(jump)
    origin = np.asarray(origin, np.float64)
    P = matrices(cams)
    i, j, k = np.meshgrid(*[np.arange(n) for n in dims], indexing='ij')
    p0, p1, p2 = origin[0] + i.astype(np.float64) * h, origin[1] + j.astype(np.float64) * h, origin[2] + k.astype(np.float64) * h
    D = np.zeros(dims, np.float64)
    n = np.zeros(dims, np.int32)
    with np.errstate(all='ignore'):
        for s in (range(V) if views is None else views):
            T = P[s]
            z = _row(T[2], p0, p1, p2, 1.0)
            ok = z > 0
            u, v = _row(T[0], p0, p1, p2, 1.0) / z - 0.5, _row(T[1], p0, p1, p2, 1.0) / z - 0.5
            ok &= (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
            x0 = np.minimum(np.floor(np.where(ok, u, 0.0)), W - 2)
            y0 = np.minimum(np.floor(np.where(ok, v, 0.0)), H - 2)
            fx, fy = u - x0, v - y0
            xi, yi = x0.astype(np.int64), y0.astype(np.int64)
            src = depths[s].astype(np.float64)
            d00, d01, d10, d11 = src[yi, xi], src[yi, xi + 1], src[yi + 1, xi], src[yi + 1, xi + 1]
            ok &= _holds(d00) & _holds(d01) & _holds(d10) & _holds(d11)
            mx = np.maximum(np.maximum(d00, d01), np.maximum(d10, d11))
            mn = np.minimum(np.minimum(d00, d01), np.minimum(d10, d11))
            ok &= ~(mx - mn > jump)
            ds = (d00 * (1 - fx) + d01 * fx) * (1 - fy) + (d10 * (1 - fx) + d11 * fx) * fy
            sd = ds - z
            ok &= ~(sd < -trunc)
            D = np.where(ok, D + np.minimum(sd / trunc, 1.0), D)
            n += ok
        valid = n >= min_views
        tsdf = np.where(valid, (D / n).astype(np.float32), np.float32(1))
    return dict(tsdf=tsdf, weight=n, valid=valid)


def smooth_field(shape, seed=0):
    """a smooth random fp32 field with a level set 0 through the grid (a few low-frequency waves)"""
    rs = np.random.RandomState(seed)
    g = np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing='ij')
    f = np.zeros(shape)
    for _ in range(4):
        w, ph = rs.uniform(-3, 3, size=3), rs.uniform(0, 6)
        f += rs.uniform(0.3, 1.0) * np.sin(w[0] * g[0] + w[1] * g[1] + w[2] * g[2] + ph)
    return (f + rs.uniform(-0.2, 0.2)).astype(np.float32)


def _shift(a, axis, step, fill):
    """out[g] = a[g + step * e_axis], `fill` where that is outside the grid"""
    out = np.full_like(a, fill)
    n = a.shape[axis]
    sl = lambda s: tuple(s if b == axis else slice(None) for b in range(3))   # noqa: E731
    if step > 0:
        out[sl(slice(0, n - 1))] = a[sl(slice(1, n))]
    else:
        out[sl(slice(1, n))] = a[sl(slice(0, n - 1))]
    return out


def _gradient(v, ok, spacing):
    """component a at a valid point from its in-grid valid neighbours along a: both -> central over 2h, one -> one-sided over h, none -> 0 (fp32)"""
    g = np.zeros((3,) + v.shape, np.float32)
    for a in range(3):
        h = np.float32(spacing[a])
        has_lo, has_hi = _shift(ok, a, -1, False), _shift(ok, a, 1, False)
        vlo, vhi = _shift(v, a, -1, np.float32(0)), _shift(v, a, 1, np.float32(0))
        g[a] = np.where(has_lo & has_hi, (vhi - vlo) / (np.float32(2) * h),
                        np.where(has_hi, (vhi - v) / h, np.where(has_lo, (v - vlo) / h, np.float32(0))))
    return g


def marching_cubes_masked(vol, valid, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """-> (vertices fp32 [V, 3], faces int64 [F, 3], normals fp32 [V, 3]); V = 0 when nothing valid crosses.  Raises ValueError on a non-finite
    valid value."""
    ok = np.asarray(valid).astype(bool)
    v = np.where(ok, np.asarray(vol, dtype=np.float32), np.float32(0))          # invalid values are never read
    if not np.isfinite(v).all():
        raise ValueError('non-finite valid value')
    lev = np.float32(level)
    sp = np.asarray(spacing, np.float32)
    org = np.asarray(origin, np.float32)
    nx, ny, nz = v.shape
    inside = v < lev
    # valid cells, indexed by their lower corner over the whole grid (False where there is no cell)
    cell = np.zeros((nx, ny, nz), bool)
    cc = np.ones((nx - 1, ny - 1, nz - 1), bool)
    for c in range(8):
        d = (c & 1, c >> 1 & 1, c >> 2 & 1)
        cc &= ok[d[0]:nx - 1 + d[0], d[1]:ny - 1 + d[1], d[2]:nz - 1 + d[2]]
    cell[:nx - 1, :ny - 1, :nz - 1] = cc
    # an edge along a at g touches the cells with lower corners g - m0 e_o0 - m1 e_o1
    cross = np.zeros((nx, ny, nz, 3), bool)
    for a in range(3):
        o0, o1 = [b for b in range(3) if b != a]
        around = cell | _shift(cell, o0, -1, False) | _shift(cell, o1, -1, False) | _shift(_shift(cell, o0, -1, False), o1, -1, False)
        cross[..., a] = around & (inside != _shift(inside, a, 1, False)) & _shift(np.ones_like(ok), a, 1, False)
    flat = cross.reshape(-1)
    vid = np.cumsum(flat) - 1
    idx = np.nonzero(flat)[0]
    p, a = idx // 3, idx % 3
    i, j, k = p // (ny * nz), (p // nz) % ny, p % nz
    ijk = np.stack([i, j, k], 1)
    ijk1 = ijk + np.eye(3, dtype=np.int64)[a]
    v0 = v[i, j, k]
    v1 = v[ijk1[:, 0], ijk1[:, 1], ijk1[:, 2]]
    t = (lev - v0) / (v1 - v0)
    verts = org + ijk.astype(np.float32) * sp
    rows = np.arange(len(a))
    verts[rows, a] = org[a] + (ijk[rows, a].astype(np.float32) + t) * sp[a]
    g = _gradient(v, ok, sp)
    g0 = g[:, i, j, k].T
    g1 = g[:, ijk1[:, 0], ijk1[:, 1], ijk1[:, 2]].T
    n = g0 + t[:, None] * (g1 - g0)
    nn = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    normals = np.where(nn[:, None] > 0, n / np.where(nn > 0, nn, np.float32(1))[:, None], np.float32(0)).astype(np.float32)
    # faces: valid cells in linear order, each cell's triangles in table order
    ci = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for c in range(8):
        d = (c & 1, c >> 1 & 1, c >> 2 & 1)
        ci |= inside[d[0]:nx - 1 + d[0], d[1]:ny - 1 + d[1], d[2]:nz - 1 + d[2]].astype(np.int64) << c
    cells = ci.reshape(-1)
    cnt = np.where(cc.reshape(-1), mc_ref.OFFSET[cells + 1] - mc_ref.OFFSET[cells], 0)
    cell_of = np.repeat(np.arange(cells.size), cnt)
    tri_of = np.repeat(mc_ref.OFFSET[cells], cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    ci_, cj, ck = cell_of // ((ny - 1) * (nz - 1)), (cell_of // (nz - 1)) % (ny - 1), cell_of % (nz - 1)
    faces = np.zeros((len(cell_of), 3), np.int64)
    own = np.array([mc_ref.EDGE_OWNER[x][0] for x in range(12)])
    axis = np.array([mc_ref.EDGE_OWNER[x][1] for x in range(12)])
    for s in range(3):
        e = mc_ref.TRI_EDGES[tri_of, s]
        off, ax = own[e], axis[e]
        q = ((ci_ + off[:, 0]) * ny + (cj + off[:, 1])) * nz + (ck + off[:, 2])
        assert flat[q * 3 + ax].all()                                        # every edge a valid cell's face uses carries a vertex
        faces[:, s] = vid[q * 3 + ax]
    return verts.astype(np.float32), faces, normals
