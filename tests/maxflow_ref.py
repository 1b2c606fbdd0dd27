"""numpy / plain-Python restatement of mesh trimming (reference code/mesh_cut/mesh_cut.py; GPU: csrc/mesh_cut.hip via Mesh.cut_mask / Mesh.trim).

* graph(): the network exactly as mesh_cut.py assembles it -- face values, terminal arcs, and one arc pair (f, g, smooth, smooth) per half-edge
  whose twin lies in face g (both half-edges of an interior edge are enumerated);
* max_flow(): Dinic, exact, fine up to a few thousand faces, and S* = the faces reachable from the source in its residual graph;
* cut_capacity(): the int64 capacity of the cut whose source side is a face mask;
* remove(): the faces of a mask removed, then the vertices no kept face uses, both in their original order.
"""
from collections import deque

import numpy as np


def face_values(faces, colors):
    """c_f = (r_a + r_b + r_c) / 3 in float64, summed left to right (numpy's mean over three values)"""
    r = np.asarray(colors, dtype=np.float32)[:, 0].astype(np.float64)[np.asarray(faces, dtype=np.int64)]
    return ((r[:, 0] + r[:, 1]) + r[:, 2]) / 3.0


def half_edge_pairs(faces):
    """-> int64 [E, 2] (f, g): one row per half-edge of f whose twin (v, u) lies in face g, in half-edge order (face, then slot).  ValueError for
    a duplicate directed edge or a face that repeats a vertex id (open3d's HalfEdgeTriangleMesh refuses both)."""
    faces = np.asarray(faces, dtype=np.int64)
    owner = {}
    for f, tri in enumerate(faces.tolist()):
        if len(set(tri)) != 3:
            raise ValueError('face %d repeats a vertex id' % f)
        for k in range(3):
            e = (tri[k], tri[(k + 1) % 3])
            if e in owner:
                raise ValueError('directed edge %s in two faces' % (e,))
            owner[e] = f
    pairs = []
    for f, tri in enumerate(faces.tolist()):
        for k in range(3):
            g = owner.get((tri[(k + 1) % 3], tri[k]))
            if g is not None:
                pairs.append((f, g))
    return np.array(pairs, dtype=np.int64).reshape(-1, 2)


def graph(faces, colors, thresh=15, smooth=10):
    """-> (bright bool [F]: arc source -> f of capacity 1, else f -> sink; pairs [E, 2]: each row adds capacity `smooth` both ways)"""
    return face_values(faces, colors) > thresh / 255, half_edge_pairs(faces)


class _Net:
    def __init__(self, n):
        self.n = n
        self.head = [[] for _ in range(n)]
        self.to, self.cap = [], []

    def add(self, u, v, c_uv, c_vu):
        self.head[u].append(len(self.to))
        self.to.append(v)
        self.cap.append(c_uv)
        self.head[v].append(len(self.to))
        self.to.append(u)
        self.cap.append(c_vu)


def _network(bright, pairs, smooth):
    nf = len(bright)
    s, t = nf, nf + 1
    net = _Net(nf + 2)
    for f in range(nf):
        if bright[f]:
            net.add(s, f, 1, 0)
        else:
            net.add(f, t, 1, 0)
    for f, g in pairs.tolist():
        net.add(f, g, int(smooth), int(smooth))
    return net, s, t


def _dinic(net, s, t):
    flow = 0
    while True:
        level = [-1] * net.n
        level[s] = 0
        q = deque([s])
        while q:
            u = q.popleft()
            for a in net.head[u]:
                if net.cap[a] > 0 and level[net.to[a]] < 0:
                    level[net.to[a]] = level[u] + 1
                    q.append(net.to[a])
        if level[t] < 0:
            return flow
        it = [0] * net.n
        while True:                                             # blocking flow by iterative DFS
            path, u = [], s
            while u != t:
                arcs = net.head[u]
                while it[u] < len(arcs):
                    a = arcs[it[u]]
                    if net.cap[a] > 0 and level[net.to[a]] == level[u] + 1:
                        break
                    it[u] += 1
                if it[u] == len(arcs):
                    if not path:
                        break
                    level[u] = -1                               # dead end
                    a = path.pop()
                    u = net.to[a ^ 1]
                    it[u] += 1
                    continue
                path.append(arcs[it[u]])
                u = net.to[arcs[it[u]]]
            if u != t:
                break
            d = min(net.cap[a] for a in path)
            for a in path:
                net.cap[a] -= d
                net.cap[a ^ 1] += d
            flow += d


def max_flow(faces, colors, thresh=15, smooth=10):
    """-> (flow value, S* bool [F]: the faces reachable from the source in the residual graph)"""
    bright, pairs = graph(faces, colors, thresh, smooth)
    net, s, t = _network(bright, pairs, smooth)
    flow = _dinic(net, s, t)
    seen = np.zeros(net.n, dtype=bool)
    seen[s] = True
    q = deque([s])
    while q:
        u = q.popleft()
        for a in net.head[u]:
            v = net.to[a]
            if net.cap[a] > 0 and not seen[v]:
                seen[v] = True
                q.append(v)
    return flow, seen[:len(bright)]


def cut_capacity(removed, faces, colors, thresh=15, smooth=10):
    """int64 capacity of the cut with source side {source} + removed"""
    removed = np.asarray(removed, dtype=bool)
    bright, pairs = graph(faces, colors, thresh, smooth)
    term = int(np.count_nonzero(bright & ~removed)) + int(np.count_nonzero(~bright & removed))
    cross = int(np.count_nonzero(removed[pairs[:, 0]] != removed[pairs[:, 1]])) if len(pairs) else 0
    return np.int64(term) + np.int64(cross) * np.int64(smooth)   # each crossing half-edge pair row carries `smooth` in the cut's direction


def remove(verts, faces, normals, colors, removed):
    """mesh_cut.py's output: remove_triangles_by_index(removed), then remove_unreferenced_vertices (order kept, faces re-indexed)"""
    faces = np.asarray(faces, dtype=np.int64)
    keep_f = ~np.asarray(removed, dtype=bool)
    kf = faces[keep_f]
    used = np.zeros(len(verts), dtype=bool)
    used[kf.ravel()] = True
    remap = np.cumsum(used) - 1
    out = [np.asarray(verts)[used], remap[kf].astype(np.int32)]
    out += [None if a is None else np.asarray(a)[used] for a in (normals, colors)]
    return tuple(out)


def scipy_max_flow(faces, colors, thresh=15, smooth=10):
    """the same (flow value, S*) through scipy.sparse.csgraph.maximum_flow (ImportError without scipy)"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import maximum_flow
    bright, pairs = graph(faces, colors, thresh, smooth)
    nf = len(bright)
    s, t = nf, nf + 1
    idx = np.arange(nf)
    rows = np.concatenate([np.full(int(bright.sum()), s), idx[~bright], pairs[:, 0], pairs[:, 1]])
    cols = np.concatenate([idx[bright], np.full(int((~bright).sum()), t), pairs[:, 1], pairs[:, 0]])
    caps = np.concatenate([np.ones(nf, np.int64), np.full(2 * len(pairs), int(smooth), np.int64)])
    keep = caps > 0
    cap = csr_matrix((caps[keep].astype(np.int32), (rows[keep], cols[keep])), shape=(nf + 2, nf + 2))
    res = maximum_flow(cap, s, t)
    flow = res.flow.tocsr() if hasattr(res, 'flow') else res.residual.tocsr()
    resid = _residual_lists(cap, flow)
    seen = np.zeros(nf + 2, dtype=bool)
    seen[s] = True
    q = deque([s])
    while q:
        u = q.popleft()
        for v in resid[u]:
            if not seen[v]:
                seen[v] = True
                q.append(v)
    return int(res.flow_value), seen[:nf]


def _residual_lists(cap, flow):
    """adjacency of the residual graph: u -> v when cap(u, v) - flow(u, v) > 0 (flow is antisymmetric, so reverse arcs appear by themselves)"""
    c = cap.tocoo()
    f = flow.tocoo()
    r = {}
    for u, v, x in zip(c.row.tolist(), c.col.tolist(), c.data.tolist()):
        r[(u, v)] = r.get((u, v), 0) + x
    for u, v, x in zip(f.row.tolist(), f.col.tolist(), f.data.tolist()):
        r[(u, v)] = r.get((u, v), 0) - x
    adj = [[] for _ in range(cap.shape[0])]
    for (u, v), x in r.items():
        if x > 0:
            adj[u].append(v)
    return adj
