"""numpy restatement of the marching cubes of mvsdf_amd/csrc/mesh_kernels.hip (test helper only; the product never imports it).

It reads the triangle table from the committed mvsdf_amd/csrc/mc_tables.h and follows the conventions stated in mvsdf_amd/mesh.py:
one vertex per crossing grid edge, owned by the edge's lower grid point, ordered by (owner's linear index, axis); faces ordered by (cell, table order)."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'mvsdf_amd', 'csrc', 'mc_tables.h')


def load_tables(path=HEADER):
    txt = open(path).read()

    def arr(name):
        body = re.search(r'%s\[\d+\]\s*=\s*\{(.*?)\};' % name, txt, flags=re.S).group(1)
        return np.array([int(v) for v in body.replace('\n', ' ').split(',') if v.strip()], dtype=np.int64)
    return arr('mc_tri_offset'), arr('mc_tri_edges').reshape(-1, 3)


OFFSET, TRI_EDGES = load_tables()


def edge_owner(e):
    """cube edge e -> (corner offset of its lower end (d0, d1, d2), axis)"""
    a, m = divmod(int(e), 4)
    o = [b for b in range(3) if b != a]
    off = [0, 0, 0]
    off[o[0]], off[o[1]] = m & 1, (m >> 1) & 1
    return tuple(off), a


EDGE_OWNER = [edge_owner(e) for e in range(12)]


def _gradient(v, spacing):
    """central differences inside, one-sided at the border, divided by spacing (fp32 throughout)"""
    g = np.zeros((3,) + v.shape, np.float32)
    for a in range(3):
        n = v.shape[a]
        if n < 2:
            continue
        h = np.float32(spacing[a])
        sl = lambda s: tuple(s if b == a else slice(None) for b in range(3))   # noqa: E731
        g[a][sl(slice(1, n - 1))] = (v[sl(slice(2, n))] - v[sl(slice(0, n - 2))]) / (np.float32(2) * h)
        g[a][sl(slice(0, 1))] = (v[sl(slice(1, 2))] - v[sl(slice(0, 1))]) / h
        g[a][sl(slice(n - 1, n))] = (v[sl(slice(n - 1, n))] - v[sl(slice(n - 2, n - 1))]) / h
    return g


def marching_cubes(vol, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """-> (vertices fp32 [V, 3], faces int64 [F, 3], normals fp32 [V, 3]); V = 0 when nothing crosses."""
    v = np.ascontiguousarray(vol, dtype=np.float32)
    lev = np.float32(level)
    sp = np.asarray(spacing, np.float32)
    org = np.asarray(origin, np.float32)
    nx, ny, nz = v.shape
    inside = v < lev
    cross = np.zeros((nx, ny, nz, 3), bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    flat = cross.reshape(-1)
    vid = np.cumsum(flat) - 1                                        # vertex id of every (point, axis) slot that crosses
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
    g = _gradient(v, sp)
    g0 = g[:, i, j, k].T
    g1 = g[:, ijk1[:, 0], ijk1[:, 1], ijk1[:, 2]].T
    n = g0 + t[:, None] * (g1 - g0)
    nn = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    normals = np.where(nn[:, None] > 0, n / np.where(nn > 0, nn, np.float32(1))[:, None], np.float32(0)).astype(np.float32)
    # faces: cells in linear order, each cell's triangles in table order
    ci = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for c in range(8):
        d = (c & 1, c >> 1 & 1, c >> 2 & 1)
        ci |= inside[d[0]:nx - 1 + d[0], d[1]:ny - 1 + d[1], d[2]:nz - 1 + d[2]].astype(np.int64) << c
    cells = ci.reshape(-1)
    cnt = OFFSET[cells + 1] - OFFSET[cells]
    cell_of = np.repeat(np.arange(cells.size), cnt)
    tri_of = np.repeat(OFFSET[cells], cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    ci_, cj, ck = cell_of // ((ny - 1) * (nz - 1)), (cell_of // (nz - 1)) % (ny - 1), cell_of % (nz - 1)
    faces = np.zeros((len(cell_of), 3), np.int64)
    for s in range(3):
        e = TRI_EDGES[tri_of, s]
        off = np.array([EDGE_OWNER[x][0] for x in range(12)])[e]
        ax = np.array([EDGE_OWNER[x][1] for x in range(12)])[e]
        q = ((ci_ + off[:, 0]) * ny + (cj + off[:, 1])) * nz + (ck + off[:, 2])
        faces[:, s] = vid[q * 3 + ax]
    return verts.astype(np.float32), faces, normals


def face_areas(verts, faces):
    p = verts.astype(np.float64)[faces]
    return 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)


def signed_volume(verts, faces):
    p = verts.astype(np.float64)[faces]
    return np.einsum('ij,ij->i', p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0


def directed_edges_ok(faces, n_vertices):
    """closed and consistently oriented: every directed edge (a, b) once and (b, a) once; every vertex referenced"""
    f = np.asarray(faces, np.int64)
    if len(f) == 0:
        return n_vertices == 0
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = e[:, 0] * n_vertices + e[:, 1]
    rkey = e[:, 1] * n_vertices + e[:, 0]
    uniq, counts = np.unique(key, return_counts=True)
    if (counts != 1).any() or (e[:, 0] == e[:, 1]).any():
        return False
    if not np.array_equal(np.sort(key), np.sort(rkey)):
        return False
    return np.unique(f).size == n_vertices


def components(faces, n_vertices):
    """per-face component labels numbered by each component's lowest vertex id (dense, ascending), and the count.
    Vertex connectivity by a numpy union-find (min-label propagation)."""
    f = np.asarray(faces, np.int64)
    lab = np.arange(n_vertices)
    while True:
        m = np.minimum(np.minimum(lab[f[:, 0]], lab[f[:, 1]]), lab[f[:, 2]])
        new = lab.copy()
        for s in range(3):
            np.minimum.at(new, f[:, s], m)
        new = new[new]
        if np.array_equal(new, lab):
            break
        lab = new
    roots, dense = np.unique(lab, return_inverse=True)
    return dense[f[:, 0]], len(roots)


def largest(verts, faces, labels, count):
    """label of the component with the largest area; ties -> the component with the lowest face index"""
    area = np.zeros(count)
    np.add.at(area, labels, face_areas(verts, faces))
    best = np.flatnonzero(area == area.max())
    first = np.array([np.flatnonzero(labels == b)[0] for b in best])
    return int(best[np.argmin(first)])


def select(verts, faces, normals, labels, label):
    """trimesh submesh semantics: kept vertices and faces in their original relative order, faces re-indexed"""
    keepf = labels == label
    keepv = np.zeros(len(verts), bool)
    keepv[faces[keepf].reshape(-1)] = True
    remap = np.cumsum(keepv) - 1
    return verts[keepv], remap[faces[keepf]], normals[keepv], keepv
