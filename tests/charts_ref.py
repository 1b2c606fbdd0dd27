"""The numpy restatement of mvsdf_amd/charts.py's definition, written from its module doc: the score of a face in a named view, neighbours, charts,
the absorption of small charts, rectangles, the shelf packing, UVs, the chart fill, the face map with its dilation, and the levelled fill.  fp64
throughout, every operation in the order the definition writes it (numpy never contracts a product and a sum).  The yardstick of
tests/test_gpu_charts.py, which holds the device to it entry for entry; tests/test_charts_host.py checks what the atlas means on this file alone.
Nothing here searches a table the way the device does: owners come from painting the rectangles, components from a flood over the links."""
import numpy as np

import raster_ref as R
import texture_ref as T

CAP = 65536                                                                   # the cap of a rectangle's side: 2 * MVSDF_TX_MAX_SIDE


def view_tables(verts, normals, faces, P, depth, o=0.5, masks=None, depth_tol=0.01, cos_min=0.0, ignore_normals=False):
    """step 1 of texture.py's definition for every (view, face) -> (score fp64 [V,F]: |A| where the view is a candidate, else 0; screen fp64 [V,F,6])"""
    P = np.asarray(P, np.float64)
    X = np.asarray(verts, np.float32).astype(np.float64)
    n = np.asarray(normals, np.float32).astype(np.float64)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = faces[:, 0], faces[:, 1], faces[:, 2]
    V, H, W = depth.shape
    F = len(faces)
    ns = (n[a] + n[b]) + n[c]
    xc = ((X[a] + X[b]) + X[c]) / 3.0
    nn = (ns[:, 0] * ns[:, 0] + ns[:, 1] * ns[:, 1]) + ns[:, 2] * ns[:, 2]
    flat = nn == 0
    C = R.camera_centers(P)
    score, screen = np.zeros((V, F)), np.zeros((V, F, 6))
    for v in range(V):
        vis, sx, sy = R._visible(P[v], verts, depth[v], o, None if masks is None else masks[v], depth_tol)
        with np.errstate(all='ignore'):
            u, t = sx - o, sy - o
            inside = (u >= 0) & (u <= W - 1) & (t >= 0) & (t <= H - 1)
            A = R._edge(sx[a], sy[a], sx[b], sy[b], sx[c], sy[c])
            g = C[v][None, :] - xc
            cosang = ((ns[:, 0] * g[:, 0] + ns[:, 1] * g[:, 1]) + ns[:, 2] * g[:, 2]) / np.sqrt(((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]) * nn)
            normal = np.where(flat, bool(ignore_normals), cosang > cos_min)
            cand = vis[a] & vis[b] & vis[c] & inside[a] & inside[b] & inside[c] & (A != 0) & normal
        score[v] = np.where(cand, np.abs(A), 0.0)
        screen[v] = np.where(cand[:, None], np.stack([sx[a], sy[a], sx[b], sy[b], sx[c], sy[c]], 1), 0.0)
    return score, screen


def face_scores(tables, view):
    """-> (score fp64 [F], screen fp64 [F,6]) of the one view named per face (-1: none) from view_tables' result"""
    score, screen = tables
    view = np.asarray(view, np.int64)
    F = len(view)
    f = np.arange(F)
    v = np.maximum(view, 0)
    if F == 0:
        return np.zeros(0), np.zeros((0, 6))
    return np.where(view >= 0, score[v, f], 0.0), np.where((view >= 0)[:, None], screen[v, f], 0.0)


def face_neighbors(faces):
    """-> int32 [F,3]: across edge e (corners e, (e+1) % 3) the other face, where exactly two of the 3F edges have these two (different) vertex ids
    and they belong to two faces"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(faces)
    users = {}
    for f in range(F):
        for e in range(3):
            p, q = int(faces[f, e]), int(faces[f, (e + 1) % 3])
            if p != q:
                users.setdefault((min(p, q), max(p, q)), []).append((f, e))
    nbr = np.full((F, 3), -1, np.int32)
    for u in users.values():
        if len(u) == 2 and u[0][0] != u[1][0]:
            (f, e), (g, k) = u
            nbr[f, e], nbr[g, k] = g, f
    return nbr


def face_charts(labels, nbr):
    """-> (face_chart int32 [F], chart_view int32 [C], chart_faces int32 [C])"""
    labels = np.asarray(labels, np.int64)
    nbr = np.asarray(nbr, np.int64).reshape(-1, 3)
    F = len(labels)
    chart = np.full(F, -1, np.int32)
    views, sizes = [], []
    for f in range(F):                                                        # ascending: a new chart starts at its lowest face
        if labels[f] < 0 or chart[f] >= 0:
            continue
        c = len(views)
        chart[f] = c
        todo, n = [f], 0
        while todo:
            x = todo.pop()
            n += 1
            for g in nbr[x]:
                if g >= 0 and labels[g] == labels[f] and chart[g] < 0:
                    chart[g] = c
                    todo.append(int(g))
        views.append(int(labels[f]))
        sizes.append(n)
    return chart, np.asarray(views, np.int32).reshape(-1), np.asarray(sizes, np.int32).reshape(-1)


def smooth_labels(tables, labels, nbr, min_faces=4, rounds=2):
    """step 3 -> (labels int32 [F], score, screen, the changes of every round)"""
    score_all = tables[0]
    labels = np.asarray(labels, np.int32).copy()
    nbr = np.asarray(nbr, np.int64).reshape(-1, 3)
    changes = []
    for _ in range(rounds):
        chart, _, size = face_charts(labels, nbr)
        new = labels.copy()
        for f in np.nonzero(chart >= 0)[0]:
            if size[chart[f]] >= min_faces:
                continue
            best, bs = -1, 0.0
            for g in nbr[f]:
                if g < 0 or labels[g] < 0 or labels[g] == labels[f] or size[chart[g]] < min_faces:
                    continue
                v = int(labels[g])
                sc = score_all[v, f]
                if sc > 0.0 and (sc > bs or (sc == bs and v < best)):
                    best, bs = v, sc
            if best >= 0:
                new[f] = best
        changes.append(int((new != labels).sum()))
        labels = new
    score, screen = face_scores(tables, labels)
    return labels, score, screen, changes


def roundup(x, m):
    return (x + m - 1) // m * m


def chart_rects(face_chart, n_charts, screen, o, d, pad, hw):
    """step 4 -> int64 [C,4] = (w, h, u0, t0)"""
    H, W = hw
    out = np.zeros((n_charts, 4), np.int64)
    s = np.asarray(screen, np.float64).reshape(-1, 3, 2)
    fc = np.asarray(face_chart)
    for c in range(n_charts):
        k = fc == c
        u, t = s[k, :, 0] - o, s[k, :, 1] - o
        with np.errstate(invalid='ignore'):                                   # clamped into the image, a NaN becoming 0
            u, t = np.minimum(np.where(u > 0.0, u, 0.0), float(W - 1)), np.minimum(np.where(t > 0.0, t, 0.0), float(H - 1))
        u0, u1 = int(np.floor(u.min())), int(np.ceil(u.max()))
        t0, t1 = int(np.floor(t.min())), int(np.ceil(t.max()))
        assert 0 <= u0 <= u1 <= W - 1 and 0 <= t0 <= t1 <= H - 1
        w = roundup(int(np.ceil(float(u1 - u0) * d)) + 1 + 2 * pad, pad)
        h = roundup(int(np.ceil(float(t1 - t0) * d)) + 1 + 2 * pad, pad)
        out[c] = (min(w, CAP), min(h, CAP), u0, t0)
    return out


def pack(wh):
    """step 5 for the sizes wh int [C,2] -> dict(X, Y int64 [C], Wt, Ht, order int32 [C], xs int32 [C], shelves int32 [S+1,2] = (first, Y), the last
    (C, Ht))"""
    wh = np.asarray(wh, np.int64).reshape(-1, 2)
    C = len(wh)
    assert C > 0
    order = np.argsort(-wh[:, 1], kind='stable')
    area = int((wh[:, 0] * wh[:, 1]).sum())
    Wt = 1
    while Wt < wh[:, 0].max() or Wt * Wt < area:
        Wt *= 2
    X, Y = np.zeros(C, np.int64), np.zeros(C, np.int64)
    xs = np.zeros(C, np.int32)
    shelves = []
    x = y = 0
    hs = 0
    for k, c in enumerate(order):
        w, h = wh[c]
        if k == 0 or x + w > Wt:
            y += hs
            x, hs = 0, h
            shelves.append((k, y))
        X[c], Y[c], xs[k] = x, y, x
        x += w
    Ht = y + hs
    shelves.append((C, Ht))
    return dict(X=X, Y=Y, Wt=int(Wt), Ht=int(Ht), order=order.astype(np.int32), xs=xs, shelves=np.asarray(shelves, np.int32).reshape(-1, 2))


def layout(face_chart, n_charts, screen, o, texel_density, pad, hw, max_size):
    """steps 4 and 5 with the halving -> (chart_rect int32 [C,6] = (X, Y, w, h, u0, t0), the packing dict, the density used)"""
    d = float(texel_density)
    least = roundup(2 + 2 * pad, pad)
    while True:
        r = chart_rects(face_chart, n_charts, screen, o, d, pad, hw)
        p = pack(r[:, :2])
        if p['Wt'] <= max_size and p['Ht'] <= max_size:
            break
        if r[:, 0].max() <= least and r[:, 1].max() <= least:
            raise ValueError('%d charts do not fit an atlas of %d texels a side' % (n_charts, max_size))
        d = d / 2.0
    rect = np.stack([p['X'], p['Y'], r[:, 0], r[:, 1], r[:, 2], r[:, 3]], 1).astype(np.int32)
    return rect, p, d


def corners(face_chart, rect, screen, o, d, pad):
    """the atlas coordinates of every face corner -> fp64 [F,3,2] (texel (0, 0)'s centre on faces without a chart)"""
    fc = np.asarray(face_chart, np.int64)
    s = np.asarray(screen, np.float64).reshape(-1, 3, 2)
    out = np.full((len(fc), 3, 2), 0.5)
    k = fc >= 0
    r = np.asarray(rect, np.int64).reshape(-1, 6)[fc[k]].astype(np.float64)
    out[k, :, 0] = ((r[:, 0] + pad) + 0.5)[:, None] + ((s[k, :, 0] - o) - r[:, 4][:, None]) * d
    out[k, :, 1] = ((r[:, 1] + pad) + 0.5)[:, None] + ((s[k, :, 1] - o) - r[:, 5][:, None]) * d
    return out


def uvs(xy, Wt, Ht):
    return np.stack([xy[..., 0] / float(Wt), 1.0 - xy[..., 1] / float(Ht)], -1).astype(np.float32)


def owners(rect, Wt, Ht):
    """int32 [Ht,Wt]: the chart whose rectangle holds the texel, -1 outside every rectangle (painted; the rectangles are disjoint)"""
    own = np.full((Ht, Wt), -1, np.int32)
    for c, (X, Y, w, h, _, _) in enumerate(np.asarray(rect).reshape(-1, 6)):
        assert (own[Y:Y + h, X:X + w] == -1).all() and X >= 0 and Y >= 0 and X + w <= Wt and Y + h <= Ht
        own[Y:Y + h, X:X + w] = c
    return own


def _source(rect, chart_view, own, d, pad, hw):
    """per texel of a rectangle: (rows j, columns i, chart, view, u, t) with the clamped source position"""
    H, W = hw
    j, i = np.nonzero(own >= 0)
    c = own[j, i].astype(np.int64)
    r = np.asarray(rect, np.int64).reshape(-1, 6)[c]
    u = r[:, 4].astype(np.float64) + (i - r[:, 0] - pad).astype(np.float64) / d
    t = r[:, 5].astype(np.float64) + (j - r[:, 1] - pad).astype(np.float64) / d
    u, t = np.minimum(np.maximum(u, 0.0), float(W - 1)), np.minimum(np.maximum(t, 0.0), float(H - 1))
    return j, i, c, np.asarray(chart_view, np.int64)[c], u, t


def _colors(images, view, u, t):
    col = np.zeros((len(view), 3))
    for v in np.unique(view):
        k = view == v
        col[k] = T.bilinear(images[v], u[k], t[k])
    return col


def fill(images, rect, chart_view, Wt, Ht, d, pad, fallback=(128, 128, 128), own=None):
    """step 6 -> (texture uint8 [Ht,Wt,3], valid uint8 [Ht,Wt])"""
    images = np.asarray(images)
    own = owners(rect, Wt, Ht) if own is None else own
    texture = np.zeros((Ht, Wt, 3), np.uint8)
    texture[:] = np.asarray(fallback, np.uint8)
    valid = (own >= 0).astype(np.uint8)
    j, i, c, view, u, t = _source(rect, chart_view, own, d, pad, images.shape[1:3])
    if len(j):
        texture[j, i] = np.floor(_colors(images, view, u, t) + 0.5).astype(np.uint8)
    return texture, valid


def _edges(xy, f, px, py):
    """(A, wa, wb, wc) of faces f at the points (px, py): wa = E(b, c, p), wb = E(c, a, p), wc = E(a, b, p)"""
    a, b, c = xy[f, 0], xy[f, 1], xy[f, 2]
    A = R._edge(a[..., 0], a[..., 1], b[..., 0], b[..., 1], c[..., 0], c[..., 1])
    wa = R._edge(b[..., 0], b[..., 1], c[..., 0], c[..., 1], px, py)
    wb = R._edge(c[..., 0], c[..., 1], a[..., 0], a[..., 1], px, py)
    wc = R._edge(a[..., 0], a[..., 1], b[..., 0], b[..., 1], px, py)
    return A, wa, wb, wc


def face_map(face_chart, rect, xy, Wt, Ht, pad, own=None, dilate=True):
    """step 7 -> int32 [Ht,Wt]: the lowest face whose UV triangle covers the texel centre (inside its chart's rectangle), then `pad` dilation rounds"""
    own = owners(rect, Wt, Ht) if own is None else own
    fmap = np.full((Ht, Wt), -1, np.int32)
    rect = np.asarray(rect, np.int64).reshape(-1, 6)
    for f in range(len(face_chart) - 1, -1, -1):                              # descending: the lowest face writes last
        c = face_chart[f]
        if c < 0:
            continue
        X, Y, w, h = rect[c, :4]
        x, y = xy[f, :, 0], xy[f, :, 1]
        i0, i1 = max(X, int(np.floor(x.min())) - 1), min(X + w - 1, int(np.ceil(x.max())) + 1)
        j0, j1 = max(Y, int(np.floor(y.min())) - 1), min(Y + h - 1, int(np.ceil(y.max())) + 1)
        if i1 < i0 or j1 < j0:
            continue
        jj, ii = np.meshgrid(np.arange(j0, j1 + 1), np.arange(i0, i1 + 1), indexing='ij')
        A, wa, wb, wc = _edges(xy, f, ii + 0.5, jj + 0.5)
        cov = ((A > 0) & (wa >= 0) & (wb >= 0) & (wc >= 0)) | ((A < 0) & (wa <= 0) & (wb <= 0) & (wc <= 0))
        fmap[jj[cov], ii[cov]] = f
    for _ in range(pad if dilate else 0):
        prev = fmap
        best = np.full((Ht, Wt), np.iinfo(np.int32).max, np.int32)
        for dj, di in ((0, -1), (0, 1), (-1, 0), (1, 0)):
            nb = np.full((Ht, Wt), -1, np.int32)
            no = np.full((Ht, Wt), -2, np.int32)
            dst = (slice(max(0, -dj), Ht - max(0, dj)), slice(max(0, -di), Wt - max(0, di)))
            src = (slice(max(0, dj), Ht - max(0, -dj)), slice(max(0, di), Wt - max(0, -di)))
            nb[dst], no[dst] = prev[src], own[src]
            ok = (nb >= 0) & (no == own)
            best = np.where(ok & (nb < best), nb, best)
        take = (own >= 0) & (prev < 0) & (best != np.iinfo(np.int32).max)
        fmap = np.where(take, best, prev)
    return fmap


def levelled_fill(images, rect, chart_view, Wt, Ht, d, pad, fmap, xy, corner_node, g, fallback=(128, 128, 128), own=None):
    """step 7's fill -> (texture, valid)"""
    images = np.asarray(images)
    own = owners(rect, Wt, Ht) if own is None else own
    texture = np.zeros((Ht, Wt, 3), np.uint8)
    texture[:] = np.asarray(fallback, np.uint8)
    valid = (own >= 0).astype(np.uint8)
    j, i, c, view, u, t = _source(rect, chart_view, own, d, pad, images.shape[1:3])
    if len(j):
        col = _colors(images, view, u, t)
        f = fmap[j, i].astype(np.int64)
        k = f >= 0
        A, wa, wb, wc = _edges(xy, f[k], i[k] + 0.5, j[k] + 0.5)
        alpha, beta, gamma = wa / A, wb / A, wc / A
        cn = np.asarray(corner_node, np.int64)[f[k]]
        g = np.asarray(g, np.float64)
        cc = col[k] + ((alpha[:, None] * g[cn[:, 0]] + beta[:, None] * g[cn[:, 1]]) + gamma[:, None] * g[cn[:, 2]])
        with np.errstate(invalid='ignore'):
            cc = np.where(cc > 0.0, cc, 0.0)                                  # max(., 0), a NaN becoming 0
        col[k] = np.minimum(cc, 255.0)
        texture[j, i] = np.floor(col + 0.5).astype(np.uint8)
    return texture, valid


def atlas_of_labels(tables, faces, labels, images, o=0.5, texel_density=1.0, max_size=8192, pad=4, min_faces=4, smooth_rounds=2,
                    fallback=(128, 128, 128)):
    """the definition from the labels on -> dict(label, score, screen, nbr, face_chart, chart_view, chart_faces, chart_rect, pack, density, xy, uv,
    texture, valid, face_map, own, changes, Wt, Ht)"""
    images = np.asarray(images)
    hw = images.shape[1:3]
    nbr = face_neighbors(faces)
    label, score, screen, changes = smooth_labels(tables, labels, nbr, min_faces, smooth_rounds)
    fc, cv, cf = face_charts(label, nbr)
    out = dict(label=label, score=score, screen=screen, nbr=nbr, face_chart=fc, chart_view=cv, chart_faces=cf, changes=changes, pad=pad)
    if len(cv) == 0:
        tex = np.zeros((pad, pad, 3), np.uint8)
        tex[:] = np.asarray(fallback, np.uint8)
        xy = np.full((len(fc), 3, 2), 0.5)
        out.update(chart_rect=np.zeros((0, 6), np.int32), pack=None, density=float(texel_density), xy=xy, uv=uvs(xy, pad, pad), texture=tex,
                   valid=np.zeros((pad, pad), np.uint8), face_map=np.full((pad, pad), -1, np.int32), own=np.full((pad, pad), -1, np.int32), Wt=pad, Ht=pad)
        return out
    rect, p, d = layout(fc, len(cv), screen, o, texel_density, pad, hw, max_size)
    Wt, Ht = p['Wt'], p['Ht']
    own = owners(rect, Wt, Ht)
    xy = corners(fc, rect, screen, o, d, pad)
    texture, valid = fill(images, rect, cv, Wt, Ht, d, pad, fallback, own)
    out.update(chart_rect=rect, pack=p, density=d, xy=xy, uv=uvs(xy, Wt, Ht), texture=texture, valid=valid,
               face_map=face_map(fc, rect, xy, Wt, Ht, pad, own), own=own, Wt=Wt, Ht=Ht)
    return out
