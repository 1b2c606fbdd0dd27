"""The texture atlas definition on its numpy restatement alone (tests/texture_ref.py; no GPU): the packing, the texel owner lookup, the bilinear
footprint, what the atlas means, the max_size loop, and that tests/texture_scene.py's scenes exercise the cases tests/test_gpu_texture.py needs."""
import numpy as np
import pytest

import mc_ref
import raster_ref as R
import texture_ref as T
import texture_scene as TS


def _forward_map(L):
    """the atlas painted from the forward placement: int64 [Ht,Wt] = the place that owns the texel, -1 where nobody does; also asserts that the
    cells are disjoint, aligned to their own size and inside the atlas"""
    owner = np.full((L['Ht'], L['Wt']), -1, np.int64)
    cells = np.zeros((L['Ht'] // T.N_MIN, L['Wt'] // T.N_MIN), np.int64)
    for p, (x0, y0, n, half) in enumerate(T.place(L)):
        assert x0 % n == 0 and y0 % n == 0 and 0 <= x0 and x0 + n <= L['Wt'] and 0 <= y0 and y0 + n <= L['Ht'], (p, x0, y0, n)
        if half == 0:
            cells[y0 // 4:(y0 + n) // 4, x0 // 4:(x0 + n) // 4] += 1
        lj, li = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
        mine = (li + lj <= n - 1) if half == 0 else (li + lj > n - 1)
        sub = owner[y0:y0 + n, x0:x0 + n]
        assert (sub[mine] == -1).all(), p
        sub[mine] = p
    assert cells.max() <= 1                                                   # no two cells share a block
    assert int(cells.sum()) == L['T']
    return owner


HISTOGRAMS = TS.histograms()


def test_the_histograms_hold_the_named_cases():
    Ls = [T.layout(h) for h in HISTOGRAMS]
    assert any(sum(h) == 1 for h in HISTOGRAMS)
    assert any(sum(c > 0 for c in h) == 1 and sum(h) > 1 for h in HISTOGRAMS)
    assert any(any(h[k] > 0 and h[k + 1] == 0 and any(h[k + 2:]) for k in range(5)) for h in HISTOGRAMS)
    assert any(sum(c % 2 for c in h) >= 3 for h in HISTOGRAMS)
    assert any(L['T'] > 1 and L['T'] == 4 ** round(np.log(L['T']) / np.log(4)) for L in Ls)
    assert any(L['Wt'] == 2 * L['Ht'] for L in Ls) and any(L['Wt'] == L['Ht'] for L in Ls)


@pytest.mark.parametrize('h', HISTOGRAMS, ids=lambda h: '-'.join(str(c) for c in h))
def test_packing_and_owner_lookup(h):
    L = T.layout(h)
    B = int(np.log2(L['Wt'] // 4)) + int(np.log2(L['Ht'] // 4))
    assert L['T'] <= 2 ** B and (B == 0 or L['T'] > 2 ** (B - 1)) and L['Wt'] in (L['Ht'], 2 * L['Ht'])
    if L['T'] > 1:
        assert 2 * L['T'] >= (L['Wt'] // 4) * (L['Ht'] // 4)                   # at least half of the blocks are used
    forward = _forward_map(L)
    jj, ii = np.meshgrid(np.arange(L['Ht']), np.arange(L['Wt']), indexing='ij')
    got = T.owner(L, ii, jj)[0]
    assert np.array_equal(got, forward)                                       # the inverse agrees with the placement at every texel
    # the order behind the places: by class descending, stable in the face index
    rs = np.random.RandomState(sum(h))
    cls = rs.permutation(np.repeat(np.arange(7), h))
    order, patch, uv, L2 = T.pack(cls)
    assert L2 == L and sorted(order.tolist()) == list(range(len(cls)))
    key = [(-int(cls[f]), int(f)) for f in order]
    assert key == sorted(key)
    assert np.array_equal(patch[order], T.place(L).astype(np.int32)) and (patch[:, 2] == 4 << cls).all()
    assert uv.dtype == np.float32 and uv.min() >= 0 and uv.max() <= 1


def test_the_bilinear_footprint_of_a_uv_triangle_stays_in_its_own_texels():
    h = [5, 3, 3, 3, 3, 1, 1]
    L = T.layout(h)
    pl = T.place(L)
    rs = np.random.RandomState(1)
    w = rs.dirichlet((0.4, 0.4, 0.4), 600)                                    # barycentric points, many near the edges and corners
    w = np.concatenate([np.eye(3), [[0.5, 0.5, 0], [0, 0.5, 0.5], [0.5, 0, 0.5]], w])
    assert (pl[:, 3] == 1).any() and set(pl[:, 2]) == {4, 8, 16, 32, 64, 128, 256}
    for p, (x0, y0, n, half) in enumerate(pl):
        tri = T.corners(n, half) + np.array([x0, y0], np.float64)
        xy = w @ tri
        _, i0, j0 = T.lookup(np.zeros((L['Ht'], L['Wt'], 1), np.uint8), xy[:, 0], xy[:, 1])
        for di in (0, 1):
            for dj in (0, 1):
                own = T.owner(L, i0 + di, j0 + dj)[0]
                assert (own == p).all(), (p, n, half, xy[own != p][:3])


def test_a_lookup_of_the_atlas_gives_the_image_within_one_grey_level():
    s = TS.inside_scene()
    V = len(s['P'])
    images = TS.linear_images(V)
    depth, _ = R.rasterize(s['verts'], s['faces'], s['P'], TS.HW, 0.5)
    for d in (1.0, 3.0):
        a = T.build_atlas(s['verts'], s['normals'], s['faces'], s['P'], depth, images, 0.5, texel_density=d)
        worst = TS.meaning_error(a, images, 0.5, np.random.RandomState(2))
        assert worst <= 1.0 + 1e-9, (d, worst)


def test_the_density_is_halved_until_the_atlas_fits():
    F = 8
    label = np.zeros(F, np.int32)
    screen = np.tile(np.array([10.0, 10.0, 110.0, 10.0, 10.0, 40.0]), (F, 1))  # the longest edge: about 104 px
    images = np.zeros((1, 64, 128, 3), np.uint8)
    a = T.atlas_of_labels(label, np.ones(F), screen, images, 0.5, 1.0, 8192)
    assert a['density'] == 1.0 and (a['cls'] == 5).all() and a['texture'].shape[:2] == (256, 256)
    b = T.atlas_of_labels(label, np.ones(F), screen, images, 0.5, 1.0, 64)    # 256 -> 128 -> 64 texels a side: two halvings
    assert b['density'] == 0.25 and (b['cls'] == 3).all() and b['texture'].shape[:2] == (64, 64)
    with pytest.raises(ValueError, match='do not fit'):
        T.atlas_of_labels(np.zeros(1000, np.int32), np.ones(1000), np.tile(screen[:1], (1000, 1)), images, 0.5, 1.0, 16)


@pytest.mark.parametrize('kind', ['sphere', 'torus'])
def test_the_scenes_exercise_the_cases(kind):
    vol, spacing, origin = TS.volume(kind)
    verts, faces, normals = mc_ref.marching_cubes(vol, 0.0, spacing, origin)
    assert 500 < len(faces) < 4000
    normals = TS.normals_with_gaps(normals)
    P = TS.twin_cameras()
    depth, _ = R.rasterize(verts, faces, P, TS.HW, 0.5)
    images, masks = TS.random_images(len(P))
    st = {}
    label, score, screen = T.face_views(verts, normals, faces, P, depth, 0.5, stats=st)
    TS.check_cases(label, st, twin=(1, 6))
    for d in (1.0, 3.0):
        TS.check_classes(T.classify(label, screen, d)[1])
