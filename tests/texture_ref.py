"""The numpy restatement of mvsdf_amd/texture.py's definition: face labels, patch classes, the packing along the Morton curve, UVs, the texel
owner lookup and the texel fill.  fp64 throughout, every operation in the order the definition writes it (numpy never contracts a product and a
sum).  The yardstick of tests/test_gpu_texture.py, which holds the device to it bit for bit; tests/test_texture_host.py checks its packing,
its owner lookup, the bilinear footprint and what the atlas means on this file alone."""
import numpy as np

import raster_ref as R

N_MIN, N_MAX, CLASSES = 4, 256, 7
INSET = 0.75                                                                  # the right-angle corner's distance from the cell's edges
LEG_LOSS = 3.5                                                                # leg = n - LEG_LOSS


def face_views(verts, normals, faces, P, depth, o=0.5, masks=None, depth_tol=0.01, cos_min=0.0, ignore_normals=False, stats=None):
    """-> (label int32 [F], score fp64 [F], screen fp64 [F,6]).  stats (a dict) gets bool [V,F] arrays: 'visible' (all three vertices visible),
    'in_image', 'normal' (the normal test), 'area' (A != 0) and fp64 [V,F] 'scores' (|A| where the view is a candidate, else 0)."""
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
    label = np.full(F, -1, np.int32)
    score = np.zeros(F)
    screen = np.zeros((F, 6))
    keep = {k: np.zeros((V, F), bool) for k in ('visible', 'in_image', 'normal', 'area')}
    scores = np.zeros((V, F))
    for v in range(V):
        vis, sx, sy = R._visible(P[v], verts, depth[v], o, None if masks is None else masks[v], depth_tol)
        with np.errstate(all='ignore'):
            u, t = sx - o, sy - o
            inside = (u >= 0) & (u <= W - 1) & (t >= 0) & (t <= H - 1)
            A = R._edge(sx[a], sy[a], sx[b], sy[b], sx[c], sy[c])
            g = C[v][None, :] - xc
            cosang = ((ns[:, 0] * g[:, 0] + ns[:, 1] * g[:, 1]) + ns[:, 2] * g[:, 2]) / np.sqrt(((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]) * nn)
            normal = np.where(flat, bool(ignore_normals), cosang > cos_min)
            allvis = vis[a] & vis[b] & vis[c]
            allin = inside[a] & inside[b] & inside[c]
            area = A != 0
            cand = allvis & allin & area & normal
            sc = np.abs(A)
            take = cand & (sc > score)                                        # strictly: a tie stays with the lower view
        idx = np.nonzero(take)[0]
        label[idx] = v
        score[idx] = sc[idx]
        screen[idx] = np.stack([sx[a], sy[a], sx[b], sy[b], sx[c], sy[c]], 1)[idx]
        keep['visible'][v], keep['in_image'][v], keep['normal'][v], keep['area'][v] = allvis, allvis & allin, normal, area
        scores[v] = np.where(cand, sc, 0.0)
    if stats is not None:
        stats.update(keep)
        stats['scores'] = scores
    return label, score, screen


def classify(label, screen, d):
    """-> (cls uint8 [F], counts int64 [7]): class k is the patch edge N_MIN << k"""
    s = np.asarray(screen, np.float64)
    abx, aby, bcx, bcy, cax, cay = s[:, 2] - s[:, 0], s[:, 3] - s[:, 1], s[:, 4] - s[:, 2], s[:, 5] - s[:, 3], s[:, 0] - s[:, 4], s[:, 1] - s[:, 5]
    L2 = np.maximum(np.maximum(abx * abx + aby * aby, bcx * bcx + bcy * bcy), cax * cax + cay * cay)
    need = ((4.0 * L2) * d) * d
    cls = np.full(len(s), CLASSES - 1, np.uint8)
    for q in range(CLASSES - 2, -1, -1):
        e = float(2 * (N_MIN << q) - 7)
        cls[e * e >= need] = q
    cls[np.asarray(label) < 0] = 0
    return cls, np.bincount(cls, minlength=CLASSES).astype(np.int64)


def layout(counts):
    """the classes along the Morton curve, in descending order -> dict(count, start, off, end [7], T, Wt, Ht)"""
    counts = [int(x) for x in counts]
    start, off, end = [0] * CLASSES, [0] * CLASSES, [0] * CLASSES
    at = blocks = 0
    for k in range(CLASSES - 1, -1, -1):
        start[k], off[k] = at, blocks
        at += counts[k]
        blocks += ((counts[k] + 1) >> 1) << (2 * k)
        end[k] = blocks
    B = 0
    while (1 << B) < blocks:
        B += 1
    return dict(count=counts, start=start, off=off, end=end, T=blocks, Wt=N_MIN << ((B + 1) // 2), Ht=N_MIN << (B // 2))


def even_bits(x):
    """the even bits of x (int64 array), packed"""
    x = np.asarray(x, np.uint64)
    out = np.zeros_like(x)
    for b in range(32):
        out |= ((x >> np.uint64(2 * b)) & np.uint64(1)) << np.uint64(b)
    return out.astype(np.int64)


def spread_bits(x):
    x = np.asarray(x, np.uint64)
    out = np.zeros_like(x)
    for b in range(32):
        out |= ((x >> np.uint64(b)) & np.uint64(1)) << np.uint64(2 * b)
    return out.astype(np.int64)


def place(L):
    """the forward placement: for every place of the order -> int64 [F,4] = (x0, y0, n, half)"""
    out = np.zeros((sum(L['count']), 4), np.int64)
    for k in range(CLASSES):
        rank = np.arange(L['count'][k], dtype=np.int64)
        blk = L['off'][k] + ((rank >> 1) << (2 * k))
        rows = slice(L['start'][k], L['start'][k] + L['count'][k])
        out[rows, 0] = N_MIN * even_bits(blk)
        out[rows, 1] = N_MIN * even_bits(blk >> 1)
        out[rows, 2] = N_MIN << k
        out[rows, 3] = rank & 1
    return out


def corners(n, half):
    """the UV triangle's corners a, b, c in the cell frame -> fp64 [..., 3, 2]"""
    n = np.asarray(n, np.float64)
    half = np.asarray(half) != 0
    leg = n - LEG_LOSS
    ca = np.where(half, n - INSET, INSET)
    cb = np.where(half, (n - INSET) - leg, INSET + leg)
    return np.stack([np.stack([ca, ca], -1), np.stack([cb, ca], -1), np.stack([ca, cb], -1)], -2)


def pack(cls):
    """-> (order int32 [F], patch int32 [F,4], uv fp32 [F,3,2], layout)"""
    cls = np.asarray(cls, np.int64)
    L = layout(np.bincount(cls, minlength=CLASSES))
    order = np.argsort(-cls, kind='stable').astype(np.int32)
    patch = np.zeros((len(cls), 4), np.int64)
    patch[order] = place(L)
    xy = patch[:, None, :2].astype(np.float64) + corners(patch[:, 2], patch[:, 3])
    uv = np.stack([xy[..., 0] / float(L['Wt']), 1.0 - xy[..., 1] / float(L['Ht'])], -1).astype(np.float32)
    return order, patch.astype(np.int32), uv, L


def owner(L, i, j):
    """the inverse: texels (i, j) (int arrays) -> (place int64, -1 where nobody owns the texel; n; local li, lj; half)"""
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    m = spread_bits(i // N_MIN) | (spread_bits(j // N_MIN) << 1)
    c = np.full(i.shape, -1, np.int64)
    for k in range(CLASSES):
        c[(m >= L['off'][k]) & (m < L['end'][k])] = k
    ck = np.maximum(c, 0)
    n = N_MIN << ck
    li, lj = i - (i & ~(n - 1)), j - (j & ~(n - 1))
    half = (li + lj > n - 1).astype(np.int64)
    rank = 2 * ((m - np.asarray(L['off'])[ck]) >> (2 * ck)) + half
    ok = (c >= 0) & (rank < np.asarray(L['count'])[ck])
    return np.where(ok, np.asarray(L['start'])[ck] + rank, -1), n, li, lj, half


def bilinear(im, u, t):
    """fusion's bilinear rule on im [H,W,C] at u in [0, W-1], t in [0, H-1] (arrays) -> fp64 [..., C]"""
    H, W = im.shape[:2]
    x0, y0 = np.minimum(np.floor(u), float(W - 2)), np.minimum(np.floor(t), float(H - 2))
    fx, fy = (u - x0)[..., None], (t - y0)[..., None]
    xi, yi = x0.astype(np.int64), y0.astype(np.int64)
    c00, c01, c10, c11 = (im[yi, xi].astype(np.float64), im[yi, xi + 1].astype(np.float64), im[yi + 1, xi].astype(np.float64),
                          im[yi + 1, xi + 1].astype(np.float64))
    return (c00 * (1.0 - fx) + c01 * fx) * (1.0 - fy) + (c10 * (1.0 - fx) + c11 * fx) * fy


def fill(images, o, label, screen, order, L, fallback=(128, 128, 128)):
    """-> (texture uint8 [Ht,Wt,3], valid uint8 [Ht,Wt])"""
    V, H, W = images.shape[:3]
    Ht, Wt = L['Ht'], L['Wt']
    jj, ii = np.meshgrid(np.arange(Ht), np.arange(Wt), indexing='ij')
    pl, n, li, lj, half = owner(L, ii, jj)
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
        leg = n - LEG_LOSS
        beta, gamma = (qx - INSET) / leg, (qy - INSET) / leg
        alpha = (1.0 - beta) - gamma
        s = np.asarray(screen, np.float64)[f]
        sx = (alpha * s[:, 0] + beta * s[:, 2]) + gamma * s[:, 4]
        sy = (alpha * s[:, 1] + beta * s[:, 3]) + gamma * s[:, 5]
        u, t = np.minimum(np.maximum(sx - o, 0.0), float(W - 1)), np.minimum(np.maximum(sy - o, 0.0), float(H - 1))
        col = np.empty((len(f), 3))
        for v in np.unique(view):
            k = view == v
            col[k] = bilinear(images[v], u[k], t[k])
        texture[at] = np.floor(col + 0.5).astype(np.uint8)
    return texture, valid


def build_atlas(verts, normals, faces, P, depth, images, o=0.5, masks=None, depth_tol=0.01, cos_min=0.0, ignore_normals=False, texel_density=1.0,
                max_size=8192, fallback=(128, 128, 128)):
    """the whole definition -> dict(label, score, screen, cls, order, patch, uv, texture, valid, density, layout)"""
    label, score, screen = face_views(verts, normals, faces, P, depth, o, masks, depth_tol, cos_min, ignore_normals)
    return atlas_of_labels(label, score, screen, images, o, texel_density, max_size, fallback)


def atlas_of_labels(label, score, screen, images, o=0.5, texel_density=1.0, max_size=8192, fallback=(128, 128, 128)):
    F = len(label)
    if layout([F] + [0] * (CLASSES - 1))['Wt'] > max_size:
        raise ValueError('%d faces do not fit an atlas of %d texels a side' % (F, max_size))
    d = float(texel_density)
    while True:
        cls, counts = classify(label, screen, d)
        if layout(counts)['Wt'] <= max_size:
            break
        d = d / 2.0
    order, patch, uv, L = pack(cls)
    texture, valid = fill(images, o, label, screen, order, L, fallback)
    return dict(label=label, score=score, screen=screen, cls=cls, order=order, patch=patch, uv=uv, texture=texture, valid=valid, density=d, layout=L)


def lookup(texture, x, y):
    """a bilinear lookup of the atlas at texel coordinates (x, y) (texel (i, j) has its centre at (i + 0.5, j + 0.5); arrays) -> (value fp64
    [..., C], the 2 x 2 footprint as int64 i0, j0: the texels i0, i0 + 1 by j0, j0 + 1)"""
    a, b = x - 0.5, y - 0.5
    i0, j0 = np.floor(a).astype(np.int64), np.floor(b).astype(np.int64)
    fx, fy = (a - i0)[..., None], (b - j0)[..., None]
    t = texture.astype(np.float64)
    val = (t[j0, i0] * (1.0 - fx) + t[j0, i0 + 1] * fx) * (1.0 - fy) + (t[j0 + 1, i0] * (1.0 - fx) + t[j0 + 1, i0 + 1] * fx) * fy
    return val, i0, j0
