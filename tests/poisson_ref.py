"""The Poisson reconstruction of mvsdf_amd/poisson.py restated in vectorised numpy (test helper only): fp64, every product and sum a separate numpy
operation in the order the definition writes it, so nothing is contracted; np.add.at on int64 for the splat, strided slices for the stencils.  Written
from that module's doc, not from the kernels.  The mesh of a result is tsdf_ref.marching_cubes_masked(volume(out), valid(out), 0.0, (h, h, h), origin)."""
import numpy as np

CORNERS = [(dx, dy, dz) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)]


def tree_sum(a):
    """the canonical pairwise tree: pad with +0.0 to a power-of-two length, add adjacent pairs until one value is left"""
    a = np.asarray(a, np.float64)
    size = 1
    while size < len(a):
        size *= 2
    a = np.concatenate([a, np.zeros(size - len(a))])
    while len(a) > 1:
        a = a[0::2] + a[1::2]
    return float(a[0])


def _cells(p, origin, h, N):
    """-> (admitted bool [n], i0 int64 [n,3], f fp64 [n,3])"""
    with np.errstate(all='ignore'):
        g = (p - origin) / h
        fl = np.floor(g)
        ok = ((fl >= 1) & (fl <= N - 3)).all(1)
        i0 = np.where(ok[:, None], fl, 1).astype(np.int64)
        return ok, i0, g - fl


def _weight(f, d):
    return ((f[:, 0] if d[0] else 1 - f[:, 0]) * (f[:, 1] if d[1] else 1 - f[:, 1])) * (f[:, 2] if d[2] else 1 - f[:, 2])


def splat(p, n, origin, h, N):
    """-> (int64 [4,N,N,N]: V_x, V_y, V_z, density; admitted bool [n])"""
    ok, i0, f = _cells(p, origin, h, N)
    i0, f, n = i0[ok], f[ok], n[ok]
    V = np.zeros((4, N, N, N), np.int64)
    for d in CORNERS:
        w = _weight(f, d)
        idx = (i0[:, 0] + d[0], i0[:, 1] + d[1], i0[:, 2] + d[2])
        for a in range(3):
            np.add.at(V[a], idx, np.rint((w * n[:, a]) * 2.0 ** 32).astype(np.int64))
        np.add.at(V[3], idx, np.rint(w * 2.0 ** 32).astype(np.int64))
    return V, ok


def rhs(F, h):
    b = np.zeros(F.shape[1:])
    c = slice(1, -1)
    b[c, c, c] = (((F[0][2:, c, c] - F[0][:-2, c, c]) + (F[1][c, 2:, c] - F[1][c, :-2, c])) + (F[2][c, c, 2:] - F[2][c, c, :-2])) / (2 * h)
    return b


def _sum6(x):
    c = slice(1, -1)
    return ((((x[:-2, c, c] + x[2:, c, c]) + x[c, :-2, c]) + x[c, 2:, c]) + x[c, c, :-2]) + x[c, c, 2:]


def smooth(x, b, h2, sweeps):
    N = x.shape[0]
    i, j, k = np.meshgrid(*[np.arange(1, N - 1)] * 3, indexing='ij')
    par = (i + j + k) & 1
    c = slice(1, -1)
    for _ in range(sweeps):
        for colour in (0, 1):
            new = (_sum6(x) - h2 * b[c, c, c]) / 6.0
            x[c, c, c] = np.where(par == colour, new, x[c, c, c])


def residual(x, b, h2):
    r = np.zeros_like(x)
    c = slice(1, -1)
    r[c, c, c] = b[c, c, c] - (_sum6(x) - 6.0 * x[c, c, c]) / h2
    return r


def _restrict1(a, axis):
    a = np.moveaxis(a, axis, 0)
    o = np.zeros(((a.shape[0] - 1) // 2 + 1,) + a.shape[1:])
    o[1:-1] = (0.25 * a[1:-2:2] + 0.5 * a[2:-1:2]) + 0.25 * a[3::2]
    return np.moveaxis(o, 0, axis)


def restrict(r):
    o = _restrict1(_restrict1(_restrict1(r, 2), 1), 0)
    o[0] = o[-1] = 0
    o[:, 0] = o[:, -1] = 0
    o[:, :, 0] = o[:, :, -1] = 0
    return o


def _prolong1(a, axis):
    a = np.moveaxis(a, axis, 0)
    o = np.zeros((2 * (a.shape[0] - 1) + 1,) + a.shape[1:])
    o[0::2] = a
    o[1::2] = 0.5 * (a[:-1] + a[1:])
    return np.moveaxis(o, 0, axis)


def prolong(e):
    return _prolong1(_prolong1(_prolong1(e, 0), 1), 2)


def vcycle(x, b, h, sweeps):
    h2 = h * h
    if x.shape[0] == 3:
        x[1, 1, 1] = -(h2 * b[1, 1, 1]) / 6.0
        return
    smooth(x, b, h2, sweeps)
    rc = restrict(residual(x, b, h2))
    ec = np.zeros_like(rc)
    vcycle(ec, rc, 2 * h, sweeps)
    c = slice(1, -1)
    x[c, c, c] = x[c, c, c] + prolong(ec)[c, c, c]
    smooth(x, b, h2, sweeps)


def interpolate(x, p, origin, h):
    """c_i of the admitted points, in input order"""
    ok, i0, f = _cells(p, origin, h, x.shape[0])
    i0, f = i0[ok], f[ok]
    s = np.zeros(len(f))
    for d in CORNERS:
        s = s + _weight(f, d) * x[i0[:, 0] + d[0], i0[:, 1] + d[1], i0[:, 2] + d[2]]
    return s


def reconstruct(points, normals, origin, voxel, depth, cycles=8, sweeps=2):
    """-> dict: chi, density fp64 [N,N,N], values fp64 [n_used], iso, n_used, n_outside, residual0, residual, origin, voxel, depth"""
    p, n = np.asarray(points, np.float64), np.asarray(normals, np.float64)
    origin, h = np.asarray(origin, np.float64), float(voxel)
    if not (np.isfinite(p).all() and np.isfinite(n).all()):
        raise ValueError('a coordinate or a normal is NaN or infinite')
    N = 2 ** depth + 1
    V, ok = splat(p, n, origin, h, N)
    F = V.astype(np.float64) * 2.0 ** -32
    b = rhs(F[:3], h)
    x = np.zeros((N, N, N))
    r0 = float(np.abs(residual(x, b, h * h)).max())
    for _ in range(cycles):
        vcycle(x, b, h, sweeps)
    r1 = float(np.abs(residual(x, b, h * h)).max())
    values = interpolate(x, p, origin, h)
    n_used = int(ok.sum())
    iso = tree_sum(values) / n_used if n_used else float('nan')
    return dict(chi=x, density=F[3], values=values, iso=iso, n_used=n_used, n_outside=len(p) - n_used, residual0=r0, residual=r1, origin=origin,
                voxel=h, depth=depth)


def valid(out, min_density=0.0, dilate=1):
    v = out['density'] > min_density
    for _ in range(dilate):
        w = v.copy()
        w[1:] |= v[:-1]
        w[:-1] |= v[1:]
        w[:, 1:] |= v[:, :-1]
        w[:, :-1] |= v[:, 1:]
        w[:, :, 1:] |= v[:, :, :-1]
        w[:, :, :-1] |= v[:, :, 1:]
        v = w
    return v


def volume(out):
    return (out['chi'] - out['iso']).astype(np.float32)


def mesh(out, min_density=0.0, dilate=1, trim=True):
    """-> (vertices, faces, normals) of tsdf_ref.marching_cubes_masked (empty arrays when nothing crosses)"""
    import tsdf_ref
    h = out['voxel']
    ok = valid(out, min_density, dilate) if trim else np.ones(out['chi'].shape, bool)
    return tsdf_ref.marching_cubes_masked(volume(out), ok, 0.0, (h, h, h), tuple(out['origin']))


def sphere_cloud(n, seed=0, radius=0.6):
    """n seeded points on the sphere of that radius about 0 with their outward normals"""
    nrm = np.random.RandomState(seed).normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return radius * nrm, nrm


def unit_grid(depth):
    """the cube of half-edge 1 about 0 -> (origin, h)"""
    return np.array([-1.0, -1.0, -1.0]), 2.0 / 2 ** depth
