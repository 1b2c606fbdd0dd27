"""numpy restatement of the sparse marching cubes of mvsdf_amd/csrc/mesh_sparse.hip (mesh.sparse_marching_cubes states the contract; test helper
only, the product never imports it).  Works on a full volume: the seeds from the block corners, the closure over block faces, then the dense
mc_ref.marching_cubes restricted to the cells of the active blocks, in the dense vertex / face order."""
import numpy as np

import mc_ref


def lattice(n):
    """x = fp32(np.linspace(-1, 1, n)), spacing h = x[2] - x[1] (fp64, as the dense path takes it)"""
    x = np.linspace(-1.0, 1.0, n)
    return x.astype(np.float32), x[2] - x[1]


def blocks(n, B):
    return -(-(n - 1) // B)


def seed_blocks(vol, B, level, margin, h):
    """bool [nb, nb, nb]: corners on both sides of the level, or min |v - level| <= tol = fp32(margin * B * h * sqrt(3))"""
    n = vol.shape[0]
    nb = blocks(n, B)
    c = np.minimum(np.arange(nb + 1) * B, n - 1)
    cv = vol[np.ix_(c, c, c)].astype(np.float32)
    lev = np.float32(level)
    tol = np.float32(margin * B * h * np.sqrt(3.0))
    corners = [cv[d0:nb + d0, d1:nb + d1, d2:nb + d2] for d0 in (0, 1) for d1 in (0, 1) for d2 in (0, 1)]
    inside = np.stack([v < lev for v in corners])
    near = np.stack([np.abs(v - lev) <= tol for v in corners]).any(0)
    return (inside.any(0) & ~inside.all(0)) | near


def _blk_any(a, axis, B, nb, closed):
    """any over each block's range along `axis`: [b B, min((b + 1) B, n - 1)) of the edges (closed=False, a has n - 1 entries there) or the closed
    range of the points (closed=True, n entries)"""
    starts = np.arange(nb) * B
    r = np.logical_or.reduceat(a, starts, axis=axis)
    if closed and nb > 1:
        idx = [slice(None)] * a.ndim
        idx[axis] = slice(0, nb - 1)
        r[tuple(idx)] |= np.take(a, starts[1:], axis=axis)
    return r


def _face_crosses(vol, B, level):
    """cross[d] (nb - 1 along d, nb along the others): a grid edge lying in the face between block b and b + e_d (border included) crosses"""
    n = vol.shape[0]
    nb = blocks(n, B)
    inside = vol < np.float32(level)
    out = []
    for d in range(3):
        if nb == 1:
            out.append(np.zeros([0 if a == d else 1 for a in range(3)], bool))
            continue
        planes = np.moveaxis(np.take(inside, (np.arange(nb - 1) + 1) * B, axis=d), d, 0)     # [nb - 1, n (u), n (w)]
        eu = planes[:, 1:, :] != planes[:, :-1, :]
        ew = planes[:, :, 1:] != planes[:, :, :-1]
        hit = _blk_any(_blk_any(eu, 1, B, nb, False), 2, B, nb, True) | _blk_any(_blk_any(ew, 1, B, nb, True), 2, B, nb, False)
        out.append(np.moveaxis(hit, 0, d))
    return out


def closure(seeds, vol, B, level):
    """-> (active bool [nb]^3, rounds): repeat until nothing changes: an inactive block with an active face neighbour across a face with a crossing
    grid edge becomes active.  Rounds as the device counts them (one per batch of new blocks, the last one adding nothing)."""
    cross = _face_crosses(vol, B, level)
    active = seeds.copy()
    new = seeds.copy()
    rounds = 0
    while new.any():
        rounds += 1
        add = np.zeros_like(active)
        for d in range(3):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[d], hi[d] = slice(0, -1), slice(1, None)
            lo, hi = tuple(lo), tuple(hi)
            add[hi] |= new[lo] & cross[d]                                 # new block b flags b + e_d
            add[lo] |= new[hi] & cross[d]                                 # new block b + e_d flags b
        new = add & ~active
        active |= new
    return active, rounds


def sparse_marching_cubes(vol, B, level=0.0, margin=1.0, h=None, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """-> (vertices, faces, normals, info) of the sparse extractor on the full cubic volume vol [n, n, n]; info: seeds, active (bool [nb]^3), rounds,
    active_blocks.  Vertices and faces are the dense ones (mc_ref) of the active cells, in dense order, faces re-indexed; V = 0 when none."""
    vol = np.ascontiguousarray(vol, np.float32)
    n = vol.shape[0]
    if h is None:
        h = float(spacing[0])
    seeds = seed_blocks(vol, B, level, margin, h)
    active, rounds = closure(seeds, vol, B, level)
    info = {'seeds': int(seeds.sum()), 'active': active, 'rounds': rounds, 'active_blocks': int(active.sum())}
    v, f, nrm = mc_ref.marching_cubes(vol, level, spacing, origin)
    if len(f) == 0:
        return v, f, nrm, info
    keep = active_faces(vol, B, level, active)
    return (*select_faces(v, f, nrm, keep), info)


def active_faces(vol, B, level, active):
    """bool per dense face (mc_ref order): its cell lies in an active block"""
    n = vol.shape[0]
    inside = vol < np.float32(level)
    ci = np.zeros((n - 1,) * 3, np.int64)
    for c in range(8):
        d = (c & 1, c >> 1 & 1, c >> 2 & 1)
        ci |= inside[d[0]:n - 1 + d[0], d[1]:n - 1 + d[1], d[2]:n - 1 + d[2]].astype(np.int64) << c
    cnt = (mc_ref.OFFSET[ci + 1] - mc_ref.OFFSET[ci]).reshape(-1)
    cells = np.repeat(np.arange(cnt.size), cnt)
    i, j, k = cells // ((n - 1) ** 2), (cells // (n - 1)) % (n - 1), cells % (n - 1)
    return active[i // B, j // B, k // B]


def select_faces(v, f, nrm, keep):
    """the kept faces and the vertices they use, both in their original order, faces re-indexed"""
    used = np.zeros(len(v), bool)
    used[f[keep].reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return v[used], remap[f[keep]], nrm[used]


def grazing_sphere_volume(n=129):
    """a sphere (centre (0, 0.125, 0.125), radius 0.51) on the n = 129 lattice whose caps past x = +-0.5 poke into blocks of B = 16 cells between
    their corners: with margin 0 those blocks are no seeds and only the closure reaches them -> (volume fp32 [n]^3, h)"""
    x, h = lattice(n)
    X, Y, Z = np.meshgrid(x.astype(np.float64), x, x, indexing='ij')
    return (np.sqrt(X ** 2 + (Y - 0.125) ** 2 + (Z - 0.125) ** 2) - 0.51).astype(np.float32), h
