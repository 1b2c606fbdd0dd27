"""numpy restatement of Mesh.simplify (mvsdf_amd/mesh.py; GPU: csrc/mesh_simplify.hip): vertex clustering on a uniform grid with quadric-error
placement (Lindstrom 2000).  Every operation is a scalar-wise fp64 one in the definition's order (numpy's elementwise +, -, *, /, sqrt and floor are
IEEE operations, and np.add.at adds its items one by one in array order, which is ascending vertex id / ascending corner index 3 f + k), so the
device must give the same bits.  This file is the arbiter for them.

simplify(verts fp32 [V, 3], faces int [F, 3], normals fp32 [V, 3], colors fp32 [V, 3] or None, cell, origin=None, placement='quadric')
  -> (verts, faces int32, normals, colors or None, stats); verts is None when no face survives (stats is still filled).
"""
import numpy as np

LAMBDA = 1e-3
CELL_BITS = 21


def cell_index(p, origin, cell):
    """floor((p - origin) / cell) as fp64 (p: [..., 3] fp64)"""
    return np.floor((p - origin) / cell)


def clusters(verts, cell, origin=None):
    """-> (cluster id per vertex, number of clusters, origin fp64 [3], cell index fp64 [V, 3]); clusters numbered by their lowest vertex id"""
    p = np.asarray(verts, np.float32).astype(np.float64)
    if not np.isfinite(p).all():
        raise ValueError('simplify: non-finite vertex')
    if not (np.isfinite(cell) and cell > 0):
        raise ValueError('simplify: cell must be finite and > 0')
    o = p.min(0) if origin is None else np.asarray(origin, np.float64).reshape(3)
    idx = cell_index(p, o, np.float64(cell))
    if (idx < 0).any() or (idx >= 2 ** CELL_BITS).any():
        raise ValueError('simplify: cell indices outside [0, 2^21)')
    ii = idx.astype(np.int64)
    key = (ii[:, 0] << (2 * CELL_BITS)) | (ii[:, 1] << CELL_BITS) | ii[:, 2]
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)     # first = the lowest member of every cell
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind='stable')] = np.arange(len(first))
    return rank[inv.reshape(-1)], len(first), o, idx


def rotate_min_first(t):
    """every row's cyclic rotation with its smallest entry first (rows with distinct entries)"""
    t = np.asarray(t, np.int64)
    s = np.argmin(t, axis=1)
    r = np.arange(len(t))
    return np.stack([t[r, s], t[r, (s + 1) % 3], t[r, (s + 2) % 3]], 1)


def simplify(verts, faces, normals, colors, cell, origin=None, placement='quadric'):
    if placement not in ('quadric', 'mean'):
        raise ValueError('simplify: placement %r' % (placement,))
    v32 = np.asarray(verts, np.float32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    nv = len(v32)
    if f.size and (f.min() < 0 or f.max() >= nv):
        raise ValueError('simplify: a vertex id outside [0, nv)')
    cell = np.float64(cell)
    vcl, nc, o, idx = clusters(v32, cell, origin)
    p = v32.astype(np.float64)
    # ---- faces: remap, drop degenerate ones, keep the first of every rotated triple ----
    t = vcl[f]
    deg = (t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2])
    cand = np.nonzero(~deg)[0]
    keep = np.zeros(len(f), bool)
    if len(cand):
        _, first = np.unique(rotate_min_first(t[cand]), axis=0, return_index=True)
        keep[cand[first]] = True
    stats = {'cell': float(cell), 'clusters': int(nc), 'degenerate': int(deg.sum()), 'duplicates': int(len(cand) - keep.sum()),
             'vertices': 0, 'faces': int(keep.sum()), 'quadric_placed': 0}
    if not keep.any():
        return None, None, None, None, stats
    used = np.zeros(nc, bool)
    used[t[keep].reshape(-1)] = True
    # ---- per-cluster sums over the members in ascending vertex id ----
    cnt = np.bincount(vcl, minlength=nc).astype(np.float64)
    ps = np.zeros((nc, 3))
    np.add.at(ps, vcl, p)
    m = ps / cnt[:, None]
    ns = np.zeros((nc, 3))
    np.add.at(ns, vcl, np.asarray(normals, np.float32).astype(np.float64))
    nl = np.sqrt((ns[:, 0] * ns[:, 0] + ns[:, 1] * ns[:, 1]) + ns[:, 2] * ns[:, 2])
    with np.errstate(invalid='ignore', divide='ignore'):
        nrm = np.where(nl[:, None] > 0, ns / nl[:, None], 0.0)
    col = None
    if colors is not None:
        cs = np.zeros((nc, 3))
        np.add.at(cs, vcl, np.asarray(colors, np.float32).astype(np.float64))
        col = cs / cnt[:, None]
    pos = m.copy()
    placed = np.zeros(nc, bool)
    if placement == 'quadric':
        # ---- quadric: every corner 3 f + k, ascending, adds its face's n n^T and (n . (p0 - m)) n to its cluster ----
        p0, p1, p2 = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
        e1, e2 = p1 - p0, p2 - p0
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        ccl = t.reshape(-1)                                            # cluster of corner 3 f + k
        n3 = np.repeat(n, 3, axis=0)
        p03 = np.repeat(p0, 3, axis=0)
        mc = m[ccl]
        d = (n3[:, 0] * (p03[:, 0] - mc[:, 0]) + n3[:, 1] * (p03[:, 1] - mc[:, 1])) + n3[:, 2] * (p03[:, 2] - mc[:, 2])
        A = np.zeros((nc, 6))                                          # 00 01 02 11 12 22
        np.add.at(A, ccl, np.stack([n3[:, 0] * n3[:, 0], n3[:, 0] * n3[:, 1], n3[:, 0] * n3[:, 2], n3[:, 1] * n3[:, 1], n3[:, 1] * n3[:, 2],
                                    n3[:, 2] * n3[:, 2]], 1))
        b = np.zeros((nc, 3))
        np.add.at(b, ccl, d[:, None] * n3)
        tr = (A[:, 0] + A[:, 3]) + A[:, 5]
        lam = LAMBDA * tr
        m00, m01, m02, m11, m12, m22 = A[:, 0] + lam, A[:, 1], A[:, 2], A[:, 3] + lam, A[:, 4], A[:, 5] + lam
        with np.errstate(all='ignore'):
            c00 = m11 * m22 - m12 * m12
            c01 = m02 * m12 - m01 * m22
            c02 = m01 * m12 - m02 * m11
            c11 = m00 * m22 - m02 * m02
            c12 = m01 * m02 - m00 * m12
            c22 = m00 * m11 - m01 * m01
            det = (m00 * c00 + m01 * c01) + m02 * c02
            x = np.stack([((c00 * b[:, 0] + c01 * b[:, 1]) + c02 * b[:, 2]) / det,
                          ((c01 * b[:, 0] + c11 * b[:, 1]) + c12 * b[:, 2]) / det,
                          ((c02 * b[:, 0] + c12 * b[:, 1]) + c22 * b[:, 2]) / det], 1)
            q = m + x
            head = np.zeros(nc, np.int64)
            head[vcl[::-1]] = np.arange(nv)[::-1]                      # the lowest member
            own = idx[head]
            placed = (tr > 0) & (cell_index(q, o, cell) == own).all(1)   # a NaN candidate compares unequal
        pos = np.where(placed[:, None], q, m)
    # ---- vertices: the clusters a kept face uses, ascending ----
    new_id = np.cumsum(used) - 1
    out_f = new_id[t[keep]].astype(np.int32)
    stats['vertices'] = int(used.sum())
    stats['quadric_placed'] = int((placed & used).sum())
    return (pos[used].astype(np.float32), out_f, nrm[used].astype(np.float32), None if col is None else col[used].astype(np.float32), stats)


# ---- the test shapes: marching-cubes meshes (tests/mc_ref.py) of analytic solids on an N^3 grid over [-1, 1]^3; computed once per shape ----
_SHAPES = {}


def box_sdf(p, half):
    q = np.abs(np.asarray(p, np.float64)) - np.asarray(half, np.float64)
    return np.linalg.norm(np.maximum(q, 0), axis=-1) + np.minimum(q.max(-1), 0)


def shape_mesh(kind, n, half=None):
    """kind 'sphere' (radius 0.6) or 'box' (half-extents `half`) -> (verts, faces int64, normals, colors, h); colours are a smooth field"""
    key = (kind, n, half)
    if key not in _SHAPES:
        import mc_ref
        x = np.linspace(-1.0, 1.0, n)
        g = np.stack(np.meshgrid(x, x, x, indexing='ij'), -1)
        vol = (np.linalg.norm(g, axis=-1) - 0.6 if kind == 'sphere' else box_sdf(g, half)).astype(np.float32)
        h = x[1] - x[0]
        v, f, nrm = mc_ref.marching_cubes(vol, 0.0, (h,) * 3, (x[0],) * 3)
        s = 1.0 / (1.0 + np.exp(-(1.5 + 3.0 * np.sin(v.astype(np.float64) @ np.array([7.0, -5.0, 4.0])))))
        col = np.stack([1 - s, s, 0.25 + 0.5 * s * s], 1).astype(np.float32)
        for a in (v, f, nrm, col):
            a.setflags(write=False)
        _SHAPES[key] = (v, f, nrm, col, h)
    return _SHAPES[key]


# ---- hand-built meshes: name -> ((verts, faces, normals, colors), cell, origin) ----
def _mesh(v, f):
    v = np.asarray(v, np.float32)
    n = np.tile(np.array([0, 0, 1], np.float32), (len(v), 1))
    return v, np.asarray(f, np.int64), n, None


def hand_duplicate():
    """faces 1 and 2 map to rotations of one triple (vertices 3 and 4 share vertex 0's cell); face 0 is its mirror image and stays; face 3 is degenerate"""
    v = [[0.1, 0.1, 0.1], [1.5, 0.1, 0.1], [0.1, 1.5, 0.1], [0.3, 0.2, 0.1], [0.2, 0.3, 0.4]]
    return _mesh(v, [[0, 2, 1], [0, 1, 2], [1, 2, 3], [0, 4, 1]]), 1.0, (0.0, 0.0, 0.0)


def hand_tetrahedron():
    """a tetrahedron inside one cell beside a large triangle: its cluster has only degenerate faces and is dropped"""
    v = [[0.1, 0.1, 0.1], [2.5, 0.1, 0.1], [0.1, 2.5, 0.1], [5.1, 5.1, 5.1], [5.4, 5.1, 5.1], [5.1, 5.4, 5.1], [5.1, 5.1, 5.4]]
    return _mesh(v, [[3, 4, 5], [3, 5, 6], [0, 1, 2], [3, 6, 4], [4, 6, 5]]), 1.0, (0.0, 0.0, 0.0)


def hand_unreferenced():
    v = [[0.5, 0.5, 0.5], [7.5, 7.5, 7.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [7.6, 7.5, 7.5]]
    return _mesh(v, [[0, 2, 3]]), 1.0, (0.0, 0.0, 0.0)


def hand_zero_area():
    """vertices 0 and 4 share a cell whose only faces are collinear (n = 0, tr(A) = 0): the position is the mean"""
    v = [[0.25, 0.5, 0.5], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5], [3.5, 0.5, 0.5], [0.75, 0.5, 0.5]]
    return _mesh(v, [[0, 1, 2], [4, 2, 3], [0, 3, 1]]), 1.0, (0.0, 0.0, 0.0)


def hand_candidate_leaves():
    """the cluster of vertices 0 and 1 sees two steep planes that meet far above its cell: the candidate leaves the cell, the mean stays"""
    v = [[0.1, 0.5, 0.1], [0.9, 0.5, 0.1], [-0.8, 0.5, -2.9], [0.1, 2.5, 0.1], [1.8, 0.5, -2.9], [0.9, -1.5, 0.1]]
    return _mesh(v, [[0, 2, 3], [1, 4, 5]]), 1.0, (-1.0, -2.0, -3.0)


HAND = {'duplicate': hand_duplicate, 'tetrahedron': hand_tetrahedron, 'unreferenced': hand_unreferenced, 'zero_area': hand_zero_area,
        'candidate_leaves': hand_candidate_leaves}
