"""What a chart atlas means, on the numpy restatement tests/charts_ref.py alone (no GPU): neighbours and charts of hand-made meshes, the absorption
of small charts on the truth scene, the shelf packing, the two properties of the fill (a verbatim crop at density 1; a bilinear footprint that
stays inside the face's rectangle at level 0 and at level log2(pad)), the fidelity of lookups, and seam levelling through the face map.
tests/test_gpu_charts.py then holds the device to the restatement entry for entry."""
import numpy as np
import pytest

import charts_ref as C
import charts_scene as CS
import seams_ref as SR
import seams_scene as SS
import texture_ref as T

# measured on the restatement (this file prints them with -s); the assertions below allow twice as much, rounding to uint8 and resampling being
# the only sources of a difference
FIDELITY = {2.0: 0.5001, 0.5: 68.21}


@pytest.fixture(scope='module')
def truth():
    return CS.truth()


@pytest.fixture(scope='module')
def atlases(truth):
    """the chart atlas of the truth scene's labels at every pad (density 1), and at densities 2 and 0.5 with pad 4"""
    s = truth
    out = {('pad', p): C.atlas_of_labels(s['tables'], s['faces'], s['label'], s['images'], pad=p) for p in CS.PADS}
    for d in FIDELITY:
        out[('d', d)] = C.atlas_of_labels(s['tables'], s['faces'], s['label'], s['images'], texel_density=d)
    return out


# ---------------------------------------------------------------- neighbours and charts
@pytest.mark.parametrize('name', CS.HAND)
def test_hand_meshes(name):
    faces, label, nv, nbr, chart = CS.hand_mesh(name)
    got = C.face_neighbors(faces)
    assert got.dtype == np.int32 and got.shape == (len(faces), 3)
    if nbr is not None:
        assert np.array_equal(got, nbr)
    for f in range(len(faces)):                                               # the relation is symmetric and never names the face itself
        for g in got[f]:
            assert g != f and (g < 0 or f in got[g])
    fc, cv, cf = C.face_charts(label, got)
    if chart is not None:
        assert np.array_equal(fc, chart)
    assert np.array_equal(fc >= 0, label >= 0) and cf.sum() == (label >= 0).sum() and len(cv) == len(cf) == fc.max(initial=-1) + 1
    first = [int(np.nonzero(fc == c)[0][0]) for c in range(len(cv))]
    assert first == sorted(first)                                             # numbered by their lowest face
    for c in range(len(cv)):
        assert (label[fc == c] == cv[c]).all() and (fc == c).sum() == cf[c]
    for f in range(len(faces)):                                               # linked faces share their chart
        for g in got[f]:
            if g >= 0 and label[f] >= 0 and label[f] == label[g]:
                assert fc[f] == fc[g]


def test_unlabelled_faces_split_charts():
    faces, label, nv, _, _ = CS.hand_mesh('unlabelled')
    fc, cv, cf = C.face_charts(label, C.face_neighbors(faces))
    assert (label < 0).sum() > 0 and len(cv) > 3 and set(cv) == {0, 1, 3}


# ---------------------------------------------------------------- absorption
def _small(label, nbr, min_faces=4):
    return int((C.face_charts(label, nbr)[2] < min_faces).sum())


def test_absorption_on_the_truth_scene(truth):
    s = truth
    nbr = C.face_neighbors(s['faces'])
    score_all = s['tables'][0]
    flipped = s['flipped']
    assert len(s['faces']) == 2492 and 60 <= (flipped != s['label']).sum() <= 200
    before = _small(flipped, nbr)
    fc0, _, size0 = C.face_charts(flipped, nbr)
    label, score, screen, changes = C.smooth_labels(s['tables'], flipped, nbr, 4, 2)
    after = _small(label, nbr)
    print('charts below 4 faces: %d -> %d; changes per round %s; charts %d -> %d' % (before, after, changes, len(size0), len(C.face_charts(label, nbr)[1])))
    assert after < before and changes[0] > 0
    on = label >= 0
    assert np.array_equal(on, flipped >= 0)                                   # unlabelled stays unlabelled
    assert (score[on] > 0).all() and (score_all[label[on], np.nonzero(on)[0]] > 0).all()
    large = (fc0 >= 0) & (size0[np.maximum(fc0, 0)] >= 4)
    assert np.array_equal(label[large], flipped[large])                       # large charts are untouched
    clean, _, _, ch = C.smooth_labels(s['tables'], s['label'], nbr, 4, 2)
    print('on the labels as they are: %d changes, %d charts below 4 faces' % (sum(ch), _small(s['label'], nbr)))
    for lab in (flipped, s['label']):                                         # the identities
        assert np.array_equal(C.smooth_labels(s['tables'], lab, nbr, 1, 2)[0], lab)
        assert np.array_equal(C.smooth_labels(s['tables'], lab, nbr, 4, 0)[0], lab)
    again = C.smooth_labels(s['tables'], label, nbr, 4, 1)                    # nothing oscillates: a further round only shrinks the count again
    assert _small(again[0], nbr) <= after


def test_an_island_nobody_sees_stays():
    verts, faces = SS.grid(5)
    label = np.zeros(len(faces), np.int32)
    label[13] = 1
    nbr = C.face_neighbors(faces)
    score = np.ones((2, len(faces)))
    screen = np.zeros((2, len(faces), 6))
    score[0, 13] = 0.0                                                        # view 0 does not see face 13
    out, sc, _, changes = C.smooth_labels((score, screen), label, nbr, 4, 2)
    assert np.array_equal(out, label) and changes == [0, 0]
    score[0, 13] = 0.5
    out, sc, _, changes = C.smooth_labels((score, screen), label, nbr, 4, 2)
    assert out[13] == 0 and changes == [1, 0] and sc[13] == 0.5
    label[14] = 2                                                             # two small islands side by side do not absorb each other
    score = np.ones((3, len(faces)))
    score[0, 13] = score[0, 14] = 0.0
    out, _, _, changes = C.smooth_labels((score, np.zeros((3, len(faces), 6))), label, nbr, 4, 2)
    assert np.array_equal(out, label)


def test_ties_go_to_the_lower_view():
    verts, faces = SS.grid(5)
    nbr = C.face_neighbors(faces)
    base = np.where(np.arange(len(faces)) < len(faces) // 2, 1, 2).astype(np.int32)
    f = next(f for f in range(len(faces)) if {1, 2} <= set(base[nbr[f][nbr[f] >= 0]]))      # a face between the two halves
    label = base.copy()
    label[f] = 0
    assert C.face_charts(label, nbr)[2].min() == 1 and sorted(C.face_charts(label, nbr)[2])[1] >= 4
    score = np.ones((3, len(faces)))
    out = C.smooth_labels((score, np.zeros((3, len(faces), 6))), label, nbr, 4, 1)[0]
    assert out[f] == 1                                                        # views 1 and 2 tie: the lower one
    score[2, f] = 2.0
    assert C.smooth_labels((score, np.zeros((3, len(faces), 6))), label, nbr, 4, 1)[0][f] == 2


# ---------------------------------------------------------------- packing
def _check_packing(wh, p, pad):
    X, Y, Wt, Ht = p['X'], p['Y'], p['Wt'], p['Ht']
    assert Wt & (Wt - 1) == 0 and Wt >= wh[:, 0].max() and Wt * Wt >= (wh[:, 0] * wh[:, 1]).sum()
    assert Wt == 1 or Wt // 2 < wh[:, 0].max() or (Wt // 2) ** 2 < (wh[:, 0] * wh[:, 1]).sum()         # the smallest such
    assert (X >= 0).all() and (Y >= 0).all() and (X + wh[:, 0] <= Wt).all() and (Y + wh[:, 1] <= Ht).all()
    assert not (X % pad).any() and not (Y % pad).any() and not (wh % pad).any()
    rect = np.concatenate([X[:, None], Y[:, None], wh, np.zeros_like(wh)], 1)
    own = C.owners(rect, Wt, Ht)                                              # asserts that the rectangles are disjoint and inside
    assert (own >= 0).sum() == (wh[:, 0] * wh[:, 1]).sum()
    o = p['order']
    assert (np.diff(wh[o, 1]) <= 0).all() and all(o[k] < o[k + 1] for k in range(len(o) - 1) if wh[o[k], 1] == wh[o[k + 1], 1])
    assert np.array_equal(p['xs'], X[o]) and p['shelves'][0].tolist() == [0, 0] and p['shelves'][-1].tolist() == [len(wh), Ht]


@pytest.mark.parametrize('pad', CS.PADS)
def test_packing(pad, truth):
    rs = np.random.RandomState(pad)
    for n in (1, 2, 7, 300):
        wh = np.stack([C.roundup(rs.randint(1, 120, n) + 1 + 2 * pad, pad), C.roundup(rs.randint(1, 90, n) + 1 + 2 * pad, pad)], 1)
        _check_packing(wh, C.pack(wh), pad)
    wh = np.asarray([[64, 16], [24, 16], [64, 16], [8, 24]])                  # charts exactly Wt wide take a shelf each; equal heights keep the id order
    p = C.pack(wh)
    assert p['Wt'] == 64 and p['order'].tolist() == [3, 0, 1, 2] and p['X'].tolist() == [0, 0, 0, 0] and p['Y'].tolist() == [24, 40, 56, 0]
    assert p['Ht'] == 72 and p['shelves'].tolist() == [[0, 0], [1, 24], [2, 40], [3, 56], [4, 72]]
    _check_packing(wh, p, 8)
    wh = np.asarray([[32, 16], [32, 16], [8, 16]])                            # x + w == Wt still fits
    p = C.pack(wh)
    assert p['Wt'] == 64 and p['X'].tolist() == [0, 32, 0] and p['Y'].tolist() == [0, 0, 16]
    s = truth
    a = C.atlas_of_labels(s['tables'], s['faces'], s['label'], s['images'], pad=pad)
    _check_packing(a['chart_rect'][:, 2:4].astype(np.int64), a['pack'], pad)
    assert np.array_equal(a['chart_rect'][:, 0], a['pack']['X']) and a['density'] == 1.0
    if pad == 8:                                                              # seven rectangles of 24 x 24, the least at pad 8, need 64 x 96: refused
        with pytest.raises(ValueError):
            C.atlas_of_labels(s['tables'], s['faces'], s['label'], s['images'], pad=pad, max_size=64)
    limit = 128 if pad == 8 else 64
    small = C.atlas_of_labels(s['tables'], s['faces'], s['label'], s['images'], pad=pad, max_size=limit)   # forces a halving
    assert small['density'] < 1.0 and max(small['Wt'], small['Ht']) <= limit and max(a['Wt'], a['Ht']) > limit
    _check_packing(small['chart_rect'][:, 2:4].astype(np.int64), small['pack'], pad)
    with pytest.raises(ValueError):
        C.atlas_of_labels(s['tables'], s['faces'], s['label'], s['images'], pad=pad, max_size=8)


def test_no_chart_gives_the_fallback(truth):
    s = truth
    a = C.atlas_of_labels(s['tables'], s['faces'], np.full(len(s['faces']), -1, np.int32), s['images'], pad=2, fallback=(1, 2, 3))
    assert a['texture'].shape == (2, 2, 3) and (a['texture'] == (1, 2, 3)).all() and not a['valid'].any() and (a['uv'] == (0.25, 0.75)).all()


# ---------------------------------------------------------------- the two properties
@pytest.mark.parametrize('pad', CS.PADS)
def test_a_verbatim_crop_at_density_one(pad, truth, atlases):
    a, images = atlases[('pad', pad)], truth['images']
    H, W = images.shape[1:3]
    assert a['density'] == 1.0
    j, i = np.nonzero(a['valid'])
    assert np.array_equal(a['valid'] != 0, a['own'] >= 0) and len(j) > 0
    r = a['chart_rect'][a['own'][j, i]].astype(np.int64)
    u, t = np.clip(r[:, 4] + i - r[:, 0] - pad, 0, W - 1), np.clip(r[:, 5] + j - r[:, 1] - pad, 0, H - 1)
    assert np.array_equal(a['texture'][j, i], images[a['chart_view'][a['own'][j, i]], t, u])
    assert (a['texture'][a['valid'] == 0] == 128).all()


@pytest.mark.parametrize('pad', CS.PADS)
def test_the_bilinear_footprint_stays_in_the_rectangle(pad, atlases):
    """every face with a chart, 200 random points each, at level 0 and at level log2(pad): the 2 x 2 texels (blocks) read belong to the face's chart"""
    for key in [('pad', pad)] + ([('d', 2.0), ('d', 0.5)] if pad == 4 else []):
        a = atlases[key]
        rs = np.random.RandomState(pad)
        faces = np.nonzero(a['face_chart'] >= 0)[0]
        assert len(faces) > 2000
        f = np.repeat(faces, 200)
        w = CS.bary(rs, len(f))
        w[::200] = (1.0, 0.0, 0.0)                                            # and the corners themselves
        w[1::200] = (0.0, 1.0, 0.0)
        w[2::200] = (0.0, 0.0, 1.0)
        x, y = CS.uv_points(a, f, w)
        chart = a['face_chart'][f]
        for level in sorted({1, pad}):
            assert not a['Wt'] % level and not a['Ht'] % level
            own = a['own'][::level, ::level]                                  # rectangles are aligned to pad: a block has one owner
            assert np.array_equal(np.repeat(np.repeat(own, level, 0), level, 1), a['own'])
            i0, j0 = np.floor(x / level - 0.5).astype(np.int64), np.floor(y / level - 0.5).astype(np.int64)
            for dj in (0, 1):
                for di in (0, 1):
                    assert (i0 + di >= 0).all() and (j0 + dj >= 0).all() and (i0 + di < own.shape[1]).all() and (j0 + dj < own.shape[0]).all()
                    assert np.array_equal(own[j0 + dj, i0 + di], chart), (key, level)


# ---------------------------------------------------------------- fidelity
def _source_colour(a, images, f, w):
    s = a['screen'].reshape(-1, 3, 2)[f]
    p = (w[:, :, None] * s).sum(1) - 0.5
    H, W = images.shape[1:3]
    col = np.zeros((len(f), 3))
    view = a['label'][f]
    for v in np.unique(view):
        k = view == v
        col[k] = T.bilinear(images[v], np.clip(p[k, 0], 0, W - 1), np.clip(p[k, 1], 0, H - 1))
    return col


@pytest.mark.parametrize('d', sorted(FIDELITY))
def test_lookups_return_the_photograph(d, truth, atlases):
    a, images = atlases[('d', d)], truth['images']
    assert a['density'] == d
    rs = np.random.RandomState(7)
    faces = np.nonzero(a['face_chart'] >= 0)[0]
    f = np.repeat(faces, 20)
    w = CS.bary(rs, len(f))
    x, y = CS.uv_points(a, f, w)
    got, _, _ = T.lookup(a['texture'], x, y)
    worst = float(np.abs(got - _source_colour(a, images, f, w)).max())
    print('density %g: the largest difference of a lookup from the photograph is %.4f grey levels' % (d, worst))
    assert worst <= 2 * FIDELITY[d]


def test_texel_centres_are_pixels_at_density_one(truth, atlases):
    a, images = atlases[('pad', 4)], truth['images']
    fmap = C.face_map(a['face_chart'], a['chart_rect'], a['xy'], a['Wt'], a['Ht'], 4, a['own'], dilate=False)
    j, i = np.nonzero(fmap >= 0)
    assert len(j) > 10000
    got, _, _ = T.lookup(a['texture'], i + 0.5, j + 0.5)
    r = a['chart_rect'][a['own'][j, i]].astype(np.int64)
    u, t = r[:, 4] + i - r[:, 0] - 4, r[:, 5] + j - r[:, 1] - 4                 # under a face: inside the image without a clamp
    assert np.array_equal(got, images[a['label'][fmap[j, i]], t, u].astype(np.float64))


# ---------------------------------------------------------------- the face map and levelling
def test_the_face_map(atlases):
    a = atlases[('pad', 4)]
    plain = C.face_map(a['face_chart'], a['chart_rect'], a['xy'], a['Wt'], a['Ht'], 4, a['own'], dilate=False)
    fmap = a['face_map']
    under = plain >= 0
    assert np.array_equal(fmap[under], plain[under]) and (fmap[a['own'] < 0] == -1).all()
    assert np.array_equal(a['face_chart'][fmap[fmap >= 0]], a['own'][fmap >= 0])                       # a texel's face is of its rectangle's chart
    share = under.sum() / under.size
    print('texels under a face: %.3f of the atlas, %.3f after %d dilation rounds; %.3f inside a rectangle' % (share, (fmap >= 0).mean(), 4, (a['own'] >= 0).mean()))
    assert (fmap >= 0).sum() > under.sum()
    # every texel within 4 steps (inside the rectangle) of a covered one has been reached; here: every texel a bilinear lookup in a face reads
    rs = np.random.RandomState(3)
    covered = np.isin(np.arange(len(a['chart_view'])), a['own'][under])       # a sliver chart may cover no texel centre: nothing to dilate from
    assert covered.sum() >= len(covered) - 1
    f = np.repeat(np.nonzero((a['face_chart'] >= 0) & covered[np.maximum(a['face_chart'], 0)])[0], 50)
    x, y = CS.uv_points(a, f, CS.bary(rs, len(f)))
    i0, j0 = np.floor(x - 0.5).astype(np.int64), np.floor(y - 0.5).astype(np.int64)
    for dj in (0, 1):
        for di in (0, 1):
            assert (fmap[j0 + dj, i0 + di] >= 0).all()


def _boundary_difference(a, texture, nbr):
    """the mean absolute colour difference of lookups on the two sides of label boundaries: at three points of every edge between two neighbours
    with different labels, once through each face's UVs"""
    label = a['label']
    f, e = np.nonzero((nbr >= 0) & (label[:, None] >= 0) & (label[np.maximum(nbr, 0)] >= 0) & (label[:, None] != label[np.maximum(nbr, 0)]))
    keep = f < nbr[f, e]
    f, e = f[keep], e[keep]
    g = nbr[f, e]
    k = np.asarray([list(nbr[gg]).index(ff) for ff, gg in zip(f, g)])
    diffs = []
    for s in (0.25, 0.5, 0.75):
        wf = np.zeros((len(f), 3))
        wf[np.arange(len(f)), e], wf[np.arange(len(f)), (e + 1) % 3] = 1.0 - s, s
        wg = np.zeros((len(f), 3))
        wg[np.arange(len(f)), k], wg[np.arange(len(f)), (k + 1) % 3] = s, 1.0 - s      # the neighbour runs along the edge the other way
        cf = T.lookup(texture, *CS.uv_points(a, f, wf))[0]
        cg = T.lookup(texture, *CS.uv_points(a, g, wg))[0]
        diffs.append(np.abs(cf - cg))
    return float(np.mean(diffs)), len(f)


def test_levelling_through_the_face_map(truth, atlases):
    s, a = truth, atlases[('pad', 4)]
    G = SR.seam_graph(s['faces'], a['label'])
    f = SR.node_colors(G, s['verts'], s['images'], s['P'])
    g, info = SR.solve_levels(G, f)
    args = (s['images'], a['chart_rect'], a['chart_view'], a['Wt'], a['Ht'], a['density'], 4, a['face_map'], a['xy'], G['corner_node'])
    zero, valid = C.levelled_fill(*args, np.zeros_like(g), own=a['own'])
    assert np.array_equal(zero, a['texture']) and np.array_equal(valid, a['valid'])                    # g = 0: byte for byte
    lev, valid = C.levelled_fill(*args, g, own=a['own'])
    assert np.array_equal(valid, a['valid']) and (lev != a['texture']).any() and np.array_equal(lev[a['face_map'] < 0], a['texture'][a['face_map'] < 0])
    before, n = _boundary_difference(a, a['texture'], a['nbr'])
    after, _ = _boundary_difference(a, lev, a['nbr'])
    print('mean absolute difference across %d label boundaries: %.3f before, %.3f after levelling' % (n, before, after))
    assert n > 100 and after < before


# ---------------------------------------------------------------- the option is off by default, everywhere
def test_the_option_is_off_by_default():
    import importlib.util
    import inspect
    import os
    from conftest import ROOT
    from mvsdf_amd import evaluation, texture
    sig = inspect.signature(texture.build_atlas).parameters
    assert sig['charts'].default is False and sig['chart_options'].default is None
    assert inspect.signature(evaluation.evaluate).parameters['charts'].default is False
    p = evaluation.eval_parser()
    assert p.parse_args([]).charts is False and p.parse_args(['--texture_mesh', '--charts', '--chart_pad', '8']).chart_pad == 8
    for name in ('texture_mesh', 'time_texture'):
        spec = importlib.util.spec_from_file_location('tool_' + name, os.path.join(ROOT, 'tools', name + '.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        extra = ['in.obj', 'out.obj', '--data_dir', 'd'] if name == 'texture_mesh' else []
        assert mod.parser().parse_args(extra).charts is False
        got = mod.parser().parse_args(extra + ['--charts', '--chart_pad', '2', '--min_chart_faces', '6'])
        assert got.charts is True and got.chart_pad == 2 and got.min_chart_faces == 6
        with pytest.raises(SystemExit):
            mod.parser().parse_args(extra + ['--charts', '--chart_pad', '3'])
