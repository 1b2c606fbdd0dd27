"""Chart atlases on the device (mvsdf_amd/charts.py, csrc/charts.hip) against the numpy restatement tests/charts_ref.py: every stage and the
composed call equal entry for entry (torch.equal), on the truth scene, the hand-made meshes, the degenerate inputs, both ends of the pad range,
a forced halving, the levelled fill with g = 0 and with the solved g, and workspaces of poison.  What the atlas means is checked on the
restatement alone (tests/test_charts_host.py)."""
import numpy as np
import pytest
import torch

import charts_ref as C
import charts_scene as CS
import seams_ref as SR
import seams_scene as SS
import texture_scene as TS
from helpers import POISON_PATTERNS
from mvsdf_amd import charts, raster, seams, texture
from mvsdf_amd.mesh import Mesh

pytestmark = pytest.mark.gpu
HW = TS.HW


def np_(t):
    return t.cpu().numpy()


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _gpu_mesh(verts, faces, normals=None):
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    normals = np.zeros_like(verts) if normals is None else np.ascontiguousarray(normals, np.float32)
    return Mesh(torch.from_numpy(verts), torch.from_numpy(np.ascontiguousarray(faces, np.int32).reshape(-1, 3)), torch.from_numpy(normals)).to('cuda')


def _same(got, want, what=''):
    want = torch.from_numpy(np.ascontiguousarray(want))
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert torch.equal(got.cpu(), want), (what, int((got.cpu() != want).sum()))


@pytest.fixture(scope='module')
def truth():
    """the truth scene on the device: the mesh, its raster, and the restatement's view tables from the device's depth maps"""
    s = CS.truth()
    m = _gpu_mesh(s['verts'], s['faces'], s['normals'])
    ra = raster.rasterize(m, P=s['P'], hw=HW)
    tables = C.view_tables(s['verts'], s['normals'], s['faces'], s['P'], np_(ra.depth))
    label = np_(texture.face_views(m, ra)[0])
    assert np.array_equal(label, s['label'])
    return dict(s, mesh=m, raster=ra, tables=tables, flipped=CS.flipped_labels(label, tables[0]), ignore_normals=False)


@pytest.fixture(scope='module')
def hand():
    """seams_scene's fan in four cameras with random images: a hand-labelled mesh whose labels are not all candidates"""
    c = SS.small_case('fan')
    P = SS.cameras4()
    m = _gpu_mesh(c['verts'], c['faces'])
    ra = raster.rasterize(m, P=P, hw=HW)
    tables = C.view_tables(c['verts'], np.zeros_like(c['verts']), c['faces'], P, np_(ra.depth), ignore_normals=True)
    return dict(verts=c['verts'], faces=c['faces'], P=P, images=TS.random_images(len(P))[0], mesh=m, raster=ra, tables=tables, label=c['label'],
                ignore_normals=True)


def _stages(s, labels, pad=4, d=1.0, max_size=8192, min_faces=4, rounds=2, o=0.5, workspace=None, level=True):
    """every stage on the device against the restatement, from the labels on -> (the restatement's atlas, the device's packing or None)"""
    m, ra, images, ign = s['mesh'], s['raster'], s['images'], s['ignore_normals']
    a = C.atlas_of_labels(s['tables'], s['faces'], labels, images, o, d, max_size, pad, min_faces, rounds)
    ws = workspace
    lab = cu(np.asarray(labels, np.int32))
    nbr = charts.face_neighbors(m, workspace=ws)
    _same(nbr, a['nbr'], 'nbr')
    sc, scr = charts.face_scores(m, ra, lab, ignore_normals=ign, workspace=ws)
    want = C.face_scores(s['tables'], labels)
    _same(sc, want[0], 'score')
    _same(scr, want[1], 'screen')
    for got, ref in zip(charts.face_charts(lab, nbr, workspace=ws), C.face_charts(labels, a['nbr'])):
        _same(got, ref, 'charts of the labels')
    lab2, sc2, scr2, changes = charts.smooth_labels(m, ra, lab, min_faces, rounds, ignore_normals=ign, nbr=nbr, workspace=ws)
    _same(lab2, a['label'], 'smoothed labels')
    _same(sc2, a['score'], 'smoothed score')
    _same(scr2, a['screen'], 'smoothed screen')
    assert changes == a['changes']
    fc, cv, cf = charts.face_charts(lab2, nbr, workspace=ws)
    _same(fc, a['face_chart'], 'face_chart')
    _same(cv, a['chart_view'], 'chart_view')
    _same(cf, a['chart_faces'], 'chart_faces')
    if len(a['chart_view']) == 0:
        return a, None
    p = charts.pack_charts(fc, cv.shape[0], scr2, HW, o, d, max_size, pad, workspace=ws)
    assert (p.Wt, p.Ht, p.density, p.pad) == (a['Wt'], a['Ht'], a['density'], pad)
    _same(p.chart_rect, a['chart_rect'], 'chart_rect')
    _same(p.order, a['pack']['order'], 'order')
    _same(p.xs, a['pack']['xs'], 'xs')
    _same(p.shelves, a['pack']['shelves'], 'shelves')
    _same(charts.chart_uvs(fc, scr2, p, o, workspace=ws), a['uv'], 'uv')
    tex, valid = charts.chart_fill(images, cv, p, workspace=ws)
    _same(tex, a['texture'], 'texture')
    _same(valid, a['valid'], 'valid')
    fmap = charts.face_map(fc, scr2, p, o, workspace=ws)
    _same(fmap, a['face_map'], 'face_map')
    if level:
        G = SR.seam_graph(s['faces'], a['label'])
        f = SR.node_colors(G, s['verts'], images, s['P'], o)
        g, _ = SR.solve_levels(G, f)
        graph = seams.seam_graph(m, lab2, views=len(s['P']))
        gd = seams.solve_levels(graph, seams.node_colors(graph, m, images, P=s['P'], pixel_center=o))[0]
        _same(gd, g, 'g')
        zero = charts.levelled_chart_fill(images, cv, p, fmap, fc, scr2, graph, torch.zeros_like(gd), o, workspace=ws)
        _same(zero[0], a['texture'], 'g = 0 is the plain fill')
        _same(zero[1], a['valid'])
        lev = charts.levelled_chart_fill(images, cv, p, fmap, fc, scr2, graph, gd, o, workspace=ws)
        want = C.levelled_fill(images, a['chart_rect'], a['chart_view'], a['Wt'], a['Ht'], a['density'], pad, a['face_map'], a['xy'], G['corner_node'], g,
                               own=a['own'])
        _same(lev[0], want[0], 'levelled texture')
        _same(lev[1], want[1])
        a['levelled'] = want[0]
    return a, p


def test_truth_scene(truth):
    a, p = _stages(truth, truth['label'])
    assert len(a['chart_view']) == 7 and (a['levelled'] != a['texture']).any()
    info, linfo = {}, {}
    t = texture.build_atlas(truth['mesh'], truth['images'], P=truth['P'], charts=True, level_seams=True, level_options=dict(info=linfo),
                            chart_options=dict(info=info))
    for name in ('uv', 'valid', 'face_chart', 'chart_view', 'chart_rect', 'face_map', 'score', 'screen'):
        _same(getattr(t, name), a[name], name)
    _same(t.face_view, a['label'])
    _same(t.texture, a['levelled'])
    assert t.patch is None and t.order is None and t.counts is None and t.density == 1.0 and info == dict(charts_before=7, charts=7, changes=[0, 0])
    assert max(linfo['iterations']) > 0
    plain = charts.build_chart_atlas(truth['mesh'], truth['images'], raster=truth['raster'])
    _same(plain.texture, a['texture'])
    assert tuple(plain.texture.shape) == (a['Ht'], a['Wt'], 3)


def test_flipped_labels_are_absorbed(truth):
    a, _ = _stages(truth, truth['flipped'], level=False)
    assert a['changes'][0] > 50 and len(a['chart_view']) < 20
    b, _ = _stages(truth, truth['flipped'], min_faces=1, level=False)         # the identity: every island keeps its chart
    assert b['changes'] == [0, 0] and len(b['chart_view']) > 50 and np.array_equal(b['label'], truth['flipped'])
    _stages(truth, truth['flipped'], min_faces=9, rounds=1, level=False)


@pytest.mark.parametrize('pad', [1, 8])
def test_both_ends_of_the_pad_range(truth, pad):
    a, _ = _stages(truth, truth['label'], pad=pad)
    assert not (a['chart_rect'][:, :4] % pad).any()


@pytest.mark.parametrize('d', [2.0, 0.37])
def test_other_densities(truth, d):
    _stages(truth, truth['label'], d=d, pad=2, level=(d < 1))


def test_a_forced_halving(truth):
    a, p = _stages(truth, truth['label'], max_size=64)
    assert a['density'] < 1.0 and p.Wt <= 64 and p.Ht <= 64
    fc, cv, _ = charts.face_charts(cu(a['label']), cu(a['nbr']))
    with pytest.raises(ValueError, match='do not fit'):                       # seven rectangles of 24 x 24 need 64 x 96
        charts.pack_charts(fc, cv.shape[0], cu(a['screen']), HW, max_size=64, pad=8)
    with pytest.raises(ValueError, match='do not fit'):
        texture.build_atlas(truth['mesh'], truth['images'], raster=truth['raster'], charts=True, max_size=8)


def test_hand_labels(hand):
    a, _ = _stages(hand, hand['label'], min_faces=1)                          # labels that are no candidates: score 0, corners clamped
    assert len(a['chart_view']) == 4
    _stages(hand, hand['label'], min_faces=3, pad=2, o=0.5)
    _stages(hand, np.full(len(hand['faces']), -1, np.int32))                  # all faces unlabelled: no chart
    one = dict(hand, faces=hand['faces'][:1], mesh=_gpu_mesh(hand['verts'], hand['faces'][:1]))
    one['raster'] = raster.rasterize(one['mesh'], P=hand['P'], hw=HW)
    one['tables'] = C.view_tables(hand['verts'], np.zeros_like(hand['verts']), one['faces'], hand['P'], np_(one['raster'].depth), ignore_normals=True)
    a, _ = _stages(one, np.asarray([2], np.int32))                            # one face (the corners of an open mesh are not drawn: no candidate)
    assert len(a['chart_view']) == 1


def test_one_face_from_its_screen_triangle(hand):
    """one chart of one face with a real triangle, from the tables alone, at every pad and three densities"""
    images = hand['images']
    screen = np.asarray([[20.3, 30.9, 61.5, 40.2, 33.0, 77.7]])
    fc, cv = np.zeros(1, np.int32), np.asarray([3], np.int32)
    for pad in CS.PADS:
        for d in (1.0, 2.5, 0.3):
            rect, pk, dd = C.layout(fc, 1, screen, 0.5, d, pad, HW, 8192)
            p = charts.pack_charts(cu(fc), 1, cu(screen), HW, 0.5, d, 8192, pad)
            assert (p.Wt, p.Ht, p.density) == (pk['Wt'], pk['Ht'], dd)
            _same(p.chart_rect, rect)
            xy = C.corners(fc, rect, screen, 0.5, dd, pad)
            _same(charts.chart_uvs(cu(fc), cu(screen), p), C.uvs(xy, p.Wt, p.Ht))
            tex, valid = charts.chart_fill(images, cu(cv), p)
            want = C.fill(images, rect, cv, p.Wt, p.Ht, dd, pad)
            _same(tex, want[0])
            _same(valid, want[1])
            _same(charts.face_map(cu(fc), cu(screen), p), C.face_map(fc, rect, xy, p.Wt, p.Ht, pad))


@pytest.mark.parametrize('name', CS.HAND)
def test_neighbours_and_charts_of_hand_meshes(name):
    faces, label, nv, _, _ = CS.hand_mesh(name)
    m = _gpu_mesh(np.zeros((nv, 3), np.float32), faces)
    nbr = charts.face_neighbors(m)
    _same(nbr, C.face_neighbors(faces), 'nbr')
    for got, want in zip(charts.face_charts(cu(label), nbr), C.face_charts(label, np_(nbr))):
        _same(got, want)


@pytest.mark.parametrize('nf', [255, 256, 257, 2048, 6000])
def test_long_strips_settle(nf):
    """chains are the hard case of the component rounds: a strip in order (one long walk to the root) and with its faces shuffled (a local minimum of
    the face index survives every round), cut into charts of every length and as one chart"""
    rs = np.random.RandomState(nf)
    faces = np.stack([np.arange(nf), np.arange(nf) + 1, np.arange(nf) + 2], 1).astype(np.int32)
    if nf % 2 == 0:
        faces = faces[rs.permutation(nf)]
    label = np.cumsum(rs.uniform(size=nf) < 0.01).astype(np.int32) % 3 - (rs.uniform(size=nf) < 0.002)
    label = label.astype(np.int32)
    m = _gpu_mesh(np.zeros((nf + 2, 3), np.float32), faces)
    nbr = charts.face_neighbors(m)
    _same(nbr, C.face_neighbors(faces))
    for lab in (label, np.zeros(nf, np.int32)):                               # and the whole strip as one chart
        for got, want in zip(charts.face_charts(cu(lab), nbr), C.face_charts(lab, np_(nbr))):
            _same(got, want)


def test_a_shelf_beyond_the_lds_table():
    """a shelf of 1024 charts: more than the 512 whose x table the fill keeps in LDS, beside one of 76 that fits, and a face 4090 texels wide, which a
    wave draws into the face map; from tables alone, no mesh"""
    rs = np.random.RandomState(11)
    H, W, n = 4, 5000, 1100
    cell = np.stack([rs.randint(0, W - 1, n), rs.randint(0, H - 1, n)], 1).astype(np.float64)
    tri = cell[:, None, :] + rs.uniform(0.05, 0.95, (n, 3, 2)) + 0.5         # inside one pixel cell: rectangles of 4 x 4 at pad 1
    tri[0] = [[0.7, 0.9], [4090.2, 1.1], [2000.0, 3.4]]
    screen = tri.reshape(n, 6)
    fc = np.arange(n, dtype=np.int32)
    cv = rs.randint(0, 2, n).astype(np.int32)
    images = rs.randint(0, 256, (2, H, W, 3)).astype(np.uint8)
    rect, pk, d = C.layout(fc, n, screen, 0.5, 1.0, 1, (H, W), 8192)
    assert pk['Wt'] == 4096 and sorted(np.diff(pk['shelves'][:, 0]).tolist()) == [1, 75, 1024] and d == 1.0
    p = charts.pack_charts(cu(fc), n, cu(screen), (H, W), 0.5, 1.0, 8192, 1)
    assert (p.Wt, p.Ht) == (pk['Wt'], pk['Ht'])
    _same(p.chart_rect, rect)
    _same(p.shelves, pk['shelves'])
    _same(p.xs, pk['xs'])
    xy = C.corners(fc, rect, screen, 0.5, d, 1)
    _same(charts.chart_uvs(cu(fc), cu(screen), p), C.uvs(xy, p.Wt, p.Ht))
    tex, valid = charts.chart_fill(images, cu(cv), p)
    want = C.fill(images, rect, cv, p.Wt, p.Ht, d, 1)
    _same(tex, want[0])
    _same(valid, want[1])
    fmap = C.face_map(fc, rect, xy, p.Wt, p.Ht, 1)
    assert (fmap == 0).sum() > 256
    _same(charts.face_map(cu(fc), cu(screen), p), fmap)


def test_empty_mesh_and_no_labels(truth):
    e = _gpu_mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    t = charts.build_chart_atlas(e, truth['images'], P=truth['P'], pad=2, fallback=(1, 2, 3))
    assert tuple(t.texture.shape) == (2, 2, 3) and tuple(t.uv.shape) == (0, 3, 2) and not bool(t.valid.any())
    assert tuple(t.face_chart.shape) == (0,) and tuple(t.chart_rect.shape) == (0, 6) and bool((t.face_map == -1).all())
    none = charts.build_chart_atlas(truth['mesh'], truth['images'], raster=truth['raster'], masks=np.zeros((6,) + HW, np.uint8), pad=8, fallback=(1, 2, 3))
    a = C.atlas_of_labels(truth['tables'], truth['faces'], np.full(len(truth['faces']), -1, np.int32), truth['images'], pad=8, fallback=(1, 2, 3))
    assert bool((none.face_view == -1).all())
    for name in ('uv', 'texture', 'valid', 'face_chart', 'chart_view', 'chart_rect', 'face_map'):
        _same(getattr(none, name), a[name], name)


@pytest.mark.parametrize('pattern', POISON_PATTERNS)
def test_workspaces_of_poison(truth, hand, pattern):
    nf = len(truth['faces'])
    ws = torch.full((charts.chart_workspace_bytes(nf, 512 * 512),), pattern, dtype=torch.uint8, device='cuda')
    a, p = _stages(truth, truth['flipped'], workspace=ws)
    assert p.Wt * p.Ht <= 512 * 512
    ws.fill_(pattern)
    _stages(hand, hand['label'], pad=1, min_faces=2, workspace=ws)
    ws.fill_(pattern)
    t = charts.build_chart_atlas(truth['mesh'], truth['images'], raster=truth['raster'], workspace=ws)
    b = C.atlas_of_labels(truth['tables'], truth['faces'], truth['label'], truth['images'])
    _same(t.texture, b['texture'])
    _same(t.face_map, b['face_map'])


def test_charts_off_is_todays_atlas(truth):
    t = texture.build_atlas(truth['mesh'], truth['images'], P=truth['P'])
    a = truth['atlas']
    for name in ('uv', 'texture', 'valid', 'patch', 'order', 'score', 'screen'):
        _same(getattr(t, name), a[name], name)
    _same(t.face_view, a['label'])
    assert t.face_chart is None and t.chart_view is None and t.chart_rect is None and t.face_map is None
    off = texture.build_atlas(truth['mesh'], truth['images'], P=truth['P'], charts=False, chart_options=dict(pad=8))
    assert torch.equal(off.texture, t.texture) and torch.equal(off.uv, t.uv)


def test_refusals(truth):
    m, ra = truth['mesh'], truth['raster']
    lab = cu(truth['label'])
    nbr = charts.face_neighbors(m)
    bad = lab.clone()
    bad[5] = 6
    with pytest.raises(ValueError, match='label'):                            # a view >= V, through its error bit
        charts.face_scores(m, ra, bad)
    bad[5] = -2
    with pytest.raises(ValueError, match='label'):
        charts.face_charts(bad, nbr)
    wrong = nbr.clone()
    wrong[int(np.nonzero(truth['label'] >= 0)[0][3]), 1] = len(truth['faces'])
    with pytest.raises(ValueError, match='index'):
        charts.face_charts(lab, wrong)
    fc, cv, cf = charts.face_charts(lab, nbr)
    scr = cu(truth['atlas']['screen'])
    with pytest.raises(ValueError, match='index'):                            # a face of a chart beyond the count
        charts.pack_charts(fc, cv.shape[0] - 1, scr, HW)
    p = charts.pack_charts(fc, cv.shape[0], scr, HW)
    for call in (lambda: charts.face_scores(m, ra, lab.long()), lambda: charts.face_scores(m, ra, lab[:-1]), lambda: charts.face_charts(lab.cpu(), nbr),
                 lambda: charts.face_charts(lab, nbr[:-1]), lambda: charts.smooth_labels(m, ra, lab, min_faces=0),
                 lambda: charts.smooth_labels(m, ra, lab, rounds=-1), lambda: charts.pack_charts(fc, cv.shape[0], scr, HW, pad=3),
                 lambda: charts.pack_charts(fc, 0, scr, HW), lambda: charts.pack_charts(fc, cv.shape[0], scr, HW, texel_density=0.0),
                 lambda: charts.pack_charts(fc, cv.shape[0], scr, HW, max_size=1 << 16), lambda: charts.chart_uvs(fc, scr, object()),
                 lambda: charts.chart_fill(truth['images'].astype(np.float32), cv, p), lambda: charts.chart_fill(truth['images'], cv[:-1], p),
                 lambda: charts.chart_fill(truth['images'], cv, p, fallback=(0, 0, 256)),
                 lambda: charts.face_map(fc, scr, p, workspace=torch.zeros(16, dtype=torch.uint8, device='cuda')),
                 lambda: texture.build_atlas(m, truth['images'], P=truth['P'], charts=True, chart_options=3),
                 lambda: texture.build_atlas(m, truth['images'], P=truth['P'], charts=True, recompute=True),
                 lambda: charts.build_chart_atlas(m, truth['images'], P=truth['P'], pad=16)):
        with pytest.raises(ValueError):
            call()
