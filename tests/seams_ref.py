"""The numpy restatement of mvsdf_amd/seams.py's definition, written from its docstring: nodes, node colours, the graph, the operator, the
preconditioned conjugate gradients over the canonical tree, and the levelled fill.  fp64 throughout, every operation in the order the definition
writes it (numpy never contracts a product and a sum).  The yardstick of tests/test_gpu_seams.py, which holds the device to it entry for entry;
tests/test_seams_host.py checks it against dense linear algebra and a truth scene on this file alone."""
import numpy as np

import raster_ref as R
import texture_ref as T


def tree_sum(a):
    """the canonical pairwise sum of a 1-d array: padded with +0.0 to a power of two, adjacent pairs added until one value is left"""
    a = np.asarray(a, np.float64)
    n = 1
    while n < len(a):
        n *= 2
    a = np.concatenate([a, np.zeros(n - len(a))])
    while len(a) > 1:
        a = a[0::2] + a[1::2]
    return float(a[0])


def seam_graph(faces, label):
    """steps 1 and 3 -> dict(node_vertex, node_view int32 [K], corner_node int32 [F,3], adj_off int64 [K+1], adj_seam int32 [K], adj_node int32)"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    label = np.asarray(label, np.int64)
    F = len(faces)
    pairs = sorted({(int(faces[f, e]), int(label[f])) for f in range(F) if label[f] >= 0 for e in range(3)})
    index = {p: k for k, p in enumerate(pairs)}
    K = len(pairs)
    corner = np.full((F, 3), -1, np.int32)
    for f in range(F):
        if label[f] >= 0:
            for e in range(3):
                corner[f, e] = index[(int(faces[f, e]), int(label[f]))]
    lists = [[] for _ in range(K)]
    by_vertex = {}
    for k, (i, _) in enumerate(pairs):
        by_vertex.setdefault(i, []).append(k)
    seam = np.zeros(K, np.int32)
    for k, (i, _) in enumerate(pairs):
        lists[k] = [g for g in by_vertex[i] if g != k]                        # ascending: the nodes are listed by (i, v)
        seam[k] = len(lists[k])
    for f in range(F):                                                        # (f, e) ascending
        if label[f] < 0:
            continue
        for e in range(3):
            lists[corner[f, e]] += [int(corner[f, (e + 1) % 3]), int(corner[f, (e + 2) % 3])]
    off = np.zeros(K + 1, np.int64)
    off[1:] = np.cumsum([len(li) for li in lists])
    node = np.asarray([g for li in lists for g in li], np.int32).reshape(-1)
    return dict(node_vertex=np.asarray([p[0] for p in pairs], np.int32).reshape(-1), node_view=np.asarray([p[1] for p in pairs], np.int32).reshape(-1),
                corner_node=corner, adj_off=off, adj_seam=seam, adj_node=node)


def node_colors(G, verts, images, P, o=0.5):
    """step 2 -> f fp64 [K,3]"""
    images = np.asarray(images)
    V, H, W = images.shape[:3]
    K = len(G['node_vertex'])
    f = np.zeros((K, 3))
    for v in np.unique(G['node_view']):
        k = np.nonzero(G['node_view'] == v)[0]
        front, sx, sy, _ = R.project(np.asarray(P, np.float64)[v], np.asarray(verts)[G['node_vertex'][k]])
        with np.errstate(all='ignore'):
            u, t = np.where(front, sx - o, 0.0), np.where(front, sy - o, 0.0)
            u, t = np.where(u > 0.0, u, 0.0), np.where(t > 0.0, t, 0.0)       # max(., 0), a NaN becoming 0
            u, t = np.minimum(u, float(W - 1)), np.minimum(t, float(H - 1))
        f[k] = T.bilinear(images[v], u, t)
    return f


def weights(G, smoothness):
    """the weight of every adjacency entry: 1 for a node's leading seam partners, smoothness behind them"""
    w = np.full(len(G['adj_node']), float(smoothness))
    for k in range(len(G['adj_seam'])):
        w[G['adj_off'][k]:G['adj_off'][k] + G['adj_seam'][k]] = 1.0
    return w


def _rows(G):
    """the longest list's length and, per position in a list, (nodes that have that entry, the entries' indices)"""
    off, K = G['adj_off'], len(G['adj_seam'])
    deg = off[1:] - off[:-1]
    out = []
    for j in range(int(deg.max()) if K else 0):
        k = np.nonzero(deg > j)[0]
        out.append((k, off[k] + j))
    return out


def apply_operator(G, x, smoothness, anchor, w=None, rows=None):
    """step 4: A x for x [K] or [K,C]; the sum runs from 0.0 in list order"""
    x = np.asarray(x, np.float64)
    w = weights(G, smoothness) if w is None else w
    acc = np.zeros_like(x)
    for k, e in (_rows(G) if rows is None else rows):
        nb = G['adj_node'][e]
        we = w[e] if x.ndim == 1 else w[e][:, None]
        acc[k] = acc[k] + we * (x[k] - x[nb])
    return anchor * x + acc


def rhs(G, f):
    """b: the sum from 0.0 over the seam partners, in list order, of (f_nb - f_k)"""
    f = np.asarray(f, np.float64)
    b = np.zeros_like(f)
    for j in range(int(G['adj_seam'].max()) if len(f) else 0):
        k = np.nonzero(G['adj_seam'] > j)[0]
        nb = G['adj_node'][G['adj_off'][k] + j]
        b[k] = b[k] + (f[nb] - f[k])
    return b


def diagonal(G, smoothness, anchor):
    w = weights(G, smoothness)
    s = np.zeros(len(G['adj_seam']))
    for k, e in _rows(G):
        s[k] = s[k] + w[e]
    return anchor + s


def dense_matrix(G, smoothness, anchor):
    """A as a dense matrix, built entry by entry from the graph (for the small cases of the host test)"""
    K = len(G['adj_seam'])
    A = np.zeros((K, K))
    w = weights(G, smoothness)
    for k in range(K):
        A[k, k] += anchor
        for e in range(G['adj_off'][k], G['adj_off'][k + 1]):
            A[k, k] += w[e]
            A[k, G['adj_node'][e]] -= w[e]
    return A


def solve_levels(G, f, smoothness=0.1, anchor=1e-3, cg_iters=200, cg_tol=1e-6):
    """step 5 -> (g [K,3], dict(iterations, rho, rho0))"""
    f = np.asarray(f, np.float64)
    K = len(f)
    g = np.zeros((K, 3))
    info = dict(iterations=[0, 0, 0], rho=[0.0, 0.0, 0.0], rho0=[0.0, 0.0, 0.0])
    if K == 0:
        return g, info
    B, d = rhs(G, f), diagonal(G, smoothness, anchor)
    w, rows = weights(G, smoothness), _rows(G)
    tol2 = cg_tol * cg_tol
    for c in range(3):
        x, r = np.zeros(K), B[:, c].copy()
        z = r / d
        p = z.copy()
        rho = rho0 = tree_sum(r * z)
        done = not (np.isfinite(rho0) and rho0 > 0.0)
        it = 0
        for _ in range(cg_iters):
            if done:
                break
            q = apply_operator(G, p, smoothness, anchor, w, rows)
            sigma = tree_sum(p * q)
            if not (np.isfinite(sigma) and sigma > 0.0):
                break
            alpha = rho / sigma
            x = x + alpha * p
            r = r - alpha * q
            z = r / d
            rhon = tree_sum(r * z)
            beta = rhon / rho
            p = z + beta * p
            rho = rhon
            it += 1
            done = not (rhon > tol2 * rho0)
        g[:, c] = x
        info['iterations'][c], info['rho'][c], info['rho0'][c] = it, rho, rho0
    return g, info


def fill(images, o, label, screen, order, L, corner_node, g, fallback=(128, 128, 128)):
    """step 6 -> (texture uint8 [Ht,Wt,3], valid uint8 [Ht,Wt]): texture_ref.fill with the correction before the rounding"""
    images = np.asarray(images)
    V, H, W = images.shape[:3]
    Ht, Wt = L['Ht'], L['Wt']
    jj, ii = np.meshgrid(np.arange(Ht), np.arange(Wt), indexing='ij')
    pl, n, li, lj, half = T.owner(L, ii, jj)
    texture = np.empty((Ht, Wt, 3), np.uint8)
    texture[:] = np.asarray(fallback, np.uint8)
    f = np.where(pl >= 0, np.asarray(order, np.int64)[np.maximum(pl, 0)] if len(order) else 0, -1)
    view = np.where(f >= 0, np.asarray(label, np.int64)[np.maximum(f, 0)] if len(order) else -1, -1)
    valid = (view >= 0).astype(np.uint8)
    at = np.nonzero(valid)
    if len(at[0]):
        f, view, n, half = f[at], view[at], n[at].astype(np.float64), half[at] != 0
        qx, qy = li[at] + 0.5, lj[at] + 0.5
        qx, qy = np.where(half, n - qx, qx), np.where(half, n - qy, qy)
        leg = n - T.LEG_LOSS
        beta, gamma = (qx - T.INSET) / leg, (qy - T.INSET) / leg
        alpha = (1.0 - beta) - gamma
        s = np.asarray(screen, np.float64)[f]
        sx = (alpha * s[:, 0] + beta * s[:, 2]) + gamma * s[:, 4]
        sy = (alpha * s[:, 1] + beta * s[:, 3]) + gamma * s[:, 5]
        u, t = np.minimum(np.maximum(sx - o, 0.0), float(W - 1)), np.minimum(np.maximum(sy - o, 0.0), float(H - 1))
        col = np.empty((len(f), 3))
        for v in np.unique(view):
            k = view == v
            col[k] = T.bilinear(images[v], u[k], t[k])
        cn = np.asarray(corner_node, np.int64)[f]
        g = np.asarray(g, np.float64)
        ga, gb, gc = g[cn[:, 0]], g[cn[:, 1]], g[cn[:, 2]]
        col = col + ((alpha[:, None] * ga + beta[:, None] * gb) + gamma[:, None] * gc)
        with np.errstate(invalid='ignore'):
            col = np.where(col > 0.0, col, 0.0)                               # max(., 0), a NaN becoming 0
        col = np.minimum(col, 255.0)
        texture[at] = np.floor(col + 0.5).astype(np.uint8)
    return texture, valid


def level_atlas(a, verts, faces, images, P, o=0.5, smoothness=0.1, anchor=1e-3, cg_iters=200, cg_tol=1e-6, fallback=(128, 128, 128)):
    """the whole definition on a texture_ref atlas dict -> dict(graph, f, g, info, texture, valid)"""
    G = seam_graph(faces, a['label'])
    f = node_colors(G, verts, images, P, o)
    g, info = solve_levels(G, f, smoothness, anchor, cg_iters, cg_tol)
    texture, valid = fill(images, o, a['label'], a['screen'], a['order'], a['layout'], G['corner_node'], g, fallback)
    return dict(graph=G, f=f, g=g, info=info, texture=texture, valid=valid)


def seam_rms(G, f, g):
    """the RMS over (node, seam partner) pairs of |(f_k + g_k) - (f_nb + g_nb)| over the three channels, and the number of pairs"""
    c = np.asarray(f, np.float64) + np.asarray(g, np.float64)
    d = []
    for k in range(len(G['adj_seam'])):
        for e in range(G['adj_off'][k], G['adj_off'][k] + G['adj_seam'][k]):
            d.append(c[k] - c[G['adj_node'][e]])
    d = np.asarray(d).reshape(-1, 3)
    return (float(np.sqrt((d * d).mean())) if len(d) else 0.0), len(d)
