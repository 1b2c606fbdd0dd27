"""On-device cloud cleaning (mvsdf_amd/cloud.py, csrc/cloud.hip) against the numpy restatement tests/cloud_ref.py, bit for bit: every comparison
is np.array_equal on the uint64 / int32 views, and every call is made twice."""
import importlib.util
import os
import shutil

import numpy as np
import pytest
import torch

import cloud_ref as R
import cloud_scene as CS
from conftest import ROOT
from mvsdf_amd import chamfer, cloud, fusion
from mvsdf_amd.datasets import prepare
from mvsdf_amd.utils import io as sio

pytestmark = pytest.mark.gpu
JOBS = 16                                                                    # threads of the restatement's brute force
SIZES = (17, 257, 4099, 30011)
KS = (1, 8, 20, 32)


def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_' + name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def np_(t):
    return t.cpu().numpy()


def make_cloud(kind, n, seed=0):
    rs = np.random.RandomState(seed + n)
    if kind == 'uniform':
        return rs.uniform(-1, 1, size=(n, 3)) * np.array([1.0, 0.6, 0.3])
    if kind == 'plane':                                                      # a degenerate box: z constant
        return np.concatenate([rs.uniform(-1, 1, size=(n, 2)), np.full((n, 1), 0.25)], 1)
    if kind == 'line':                                                       # two flat axes
        return np.stack([rs.uniform(-5, 5, size=n), np.full(n, -1.5), np.full(n, 2.0)], 1)
    if kind == 'offset':                                                     # the size of DTU world coordinates
        return rs.uniform(-300, 300, size=(n, 3)) + np.array([3e5, -2e5, 7e4])
    if kind == 'duplicates':                                                 # 5 % exact duplicates
        p = rs.uniform(-1, 1, size=(n, 3))
        m = max(1, n // 20)
        p[rs.choice(n, m, replace=False)] = p[rs.choice(n, m, replace=True)]
        return p
    if kind == 'lattice':                                                    # massive ties
        side = int(np.ceil(n ** (1 / 3)))
        g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing='ij'), -1).reshape(-1, 3).astype(np.float64)
        return np.ascontiguousarray(g[rs.permutation(len(g))[:n]] * 0.125)
    raise ValueError(kind)


def twice(fn):
    a, b = fn(), fn()
    return a, b


@pytest.mark.parametrize('kind', ['uniform', 'plane', 'line', 'offset', 'duplicates', 'lattice'])
def test_knn_mean_distance_is_the_restatement(kind):
    for n in SIZES:
        P = make_cloud(kind, n)
        ks = [k for k in KS if k + 1 <= n]
        s = R.k_smallest(P, max(ks), jobs=JOBS)
        for k in ks:
            want = R.mean_of_smallest(s, k)
            a, b = twice(lambda: np_(cloud.knn_mean_distance(torch.from_numpy(P).cuda() if k == 8 else P, k)))
            assert same_bits(a, want), (kind, n, k, int((bits(a) != bits(want)).sum()))
            assert same_bits(a, b), (kind, n, k)
    for k in KS:                                                             # the smallest cloud a k allows
        P = make_cloud(kind, k + 1, seed=5)
        a, b = twice(lambda: np_(cloud.knn_mean_distance(P, k)))
        assert same_bits(a, R.knn_mean_distance(P, k)) and same_bits(a, b), (kind, k)


def test_knn_at_every_list_capacity():
    """the kernel keeps its list in 8 / 16 / 24 / 32 registers: k at and beside each capacity"""
    P = make_cloud('duplicates', 4099, seed=3)
    s = R.k_smallest(P, 32, jobs=JOBS)
    for k in (7, 9, 12, 16, 17, 24, 25, 31):
        a, b = twice(lambda: np_(cloud.knn_mean_distance(P, k)))
        assert same_bits(a, R.mean_of_smallest(s, k)) and same_bits(a, b), k


def _labels(P, eps):
    a, b = twice(lambda: np_(cloud.radius_components(P, eps)))
    assert a.dtype == np.int32 and np.array_equal(a, b)
    return a


def test_radius_components_on_lattices_is_inclusive_at_eps():
    rs = np.random.RandomState(2)
    step = 0.125
    g = np.stack(np.meshgrid(np.arange(12), np.arange(9), np.arange(7), indexing='ij'), -1).reshape(-1, 3).astype(np.float64) * step
    far = g + np.array([40.0, 0, 0]) * step
    P = np.concatenate([g, far[:200]])[rs.permutation(len(g) + 200)]
    for eps in (np.nextafter(step, 0), step, np.nextafter(step, 1), 0.99 * step, 1.5 * step):
        got = _labels(P, eps)
        assert np.array_equal(got, R.radius_components(P, eps)), eps
    assert len(np.unique(_labels(P, np.nextafter(step, 0)))) == len(P)       # just below the step: every point alone
    assert len(np.unique(_labels(P, step))) == 2                             # exactly at it: the two lattices


@pytest.mark.parametrize('kind', ['uniform', 'lattice'])
@pytest.mark.parametrize('n', [2, 16, 17, 129, 2049])
def test_radius_components_at_the_tree_shape_edges(kind, n):
    """one leaf, a leaf's edge, a partly filled last child at two and at three levels: the walk that stops at the point's own position.  eps: the
    lattice's step; for the uniform cloud the median nearest-neighbour distance, which joins about half the points to their nearest one"""
    P = make_cloud(kind, n)
    if kind == 'lattice':
        eps = 0.125
    else:
        d = np.sqrt(((P[:, None] - P[None]) ** 2).sum(-1))
        np.fill_diagonal(d, np.inf)
        eps = float(np.median(d.min(1)))
    want = R.radius_components(P, eps)
    if kind == 'uniform' and n > 2:
        assert 1 < len(np.unique(want)) < n
    assert np.array_equal(_labels(P, eps), want)


def test_radius_components_on_blobs():
    rs = np.random.RandomState(4)
    centres = rs.uniform(-2, 2, size=(12, 3))
    P = np.concatenate([c + rs.normal(size=(400, 3)) * 0.05 for c in centres] + [rs.uniform(-3, 3, size=(500, 3))])
    P = np.ascontiguousarray(P[rs.permutation(len(P))])
    for eps in (0.01, 0.03, 0.08, 0.5):
        assert np.array_equal(_labels(P, eps), R.radius_components(P, eps)), eps


def test_radius_components_on_one_long_chain():
    """N points along a helix, each within eps of the next only, in shuffled order: one component whose label is index 0.  The worst case for
    the rounds of a hook / compress scheme; it must finish and be right."""
    n = 30011
    t = np.arange(n) * 0.01
    P = np.stack([np.cos(t) * (1 + 0.002 * t), np.sin(t) * (1 + 0.002 * t), 0.05 * t], 1)
    gap = np.sqrt(((P[1:] - P[:-1]) ** 2).sum(1))
    eps = float(gap.max() * 1.2)
    assert eps < 2 * gap.min()                                               # the next point only
    P = np.ascontiguousarray(P[np.random.RandomState(6).permutation(n)])
    got = _labels(P, eps)
    assert np.array_equal(got, np.zeros(n, np.int32))
    assert np.array_equal(got, R.radius_components(P, eps))
    broken = np.delete(P, 12345, 0)                                          # one link out: two components
    assert np.array_equal(_labels(broken, eps), R.radius_components(broken, eps))


def _assert_clean_is(c, want, P, colors):
    assert same_bits(np_(c.d), want['d'])
    assert same_bits([c.median, c.threshold, c.eps], [want['median'], want['threshold'], want['eps']])
    assert np_(c.labels).dtype == np.int32 and np.array_equal(np_(c.labels), want['labels'])
    assert np_(c.keep).dtype == np.uint8 and np.array_equal(np_(c.keep), want['keep'])
    sel = want['keep'] != 0
    assert same_bits(np_(c.points), P[sel]) and np.array_equal(np_(c.colors), colors[sel])
    assert (c.n_passed, c.n_clusters, c.largest, len(c)) == (want['n_passed'], want['n_clusters'], want['largest'], int(sel.sum()))
    lo, hi = c.bbox()
    assert same_bits(np_(lo), P[sel].min(0)) and same_bits(np_(hi), P[sel].max(0))


def test_clean_points_on_the_scene():
    """The scene of the issue: the fused sphere, 300 uniform outliers, a dense 400-point blob.  Equality with the restatement in everything, and
    the condition on the outcome: no injected point kept, at most 1 % of the fused points lost (the restatement: 81 of 22 096)."""
    P, injected = CS.injected()
    colors = np.random.RandomState(8).randint(0, 256, size=(len(P), 3)).astype(np.uint8)
    want = R.clean(P, jobs=JOBS)
    a, b = twice(lambda: cloud.clean_points(torch.from_numpy(P).cuda(), torch.from_numpy(colors).cuda()))
    _assert_clean_is(a, want, P, colors)
    _assert_clean_is(b, want, P, colors)
    keep = np_(a.keep)
    lost = int((keep[~injected] == 0).sum())
    print('fused %d, injected kept %d, fused lost %d, rounds %d' % (int((~injected).sum()), int(keep[injected].sum()), lost, a.rounds))
    assert int(keep[injected].sum()) == 0
    assert lost <= 0.01 * int((~injected).sum())


def test_clean_points_on_the_scene_with_holes():
    P, _ = CS.injected(hole_frac=0.3)
    colors = np.random.RandomState(9).randint(0, 256, size=(len(P), 3)).astype(np.uint8)
    want = R.clean(P, jobs=JOBS)
    a, b = twice(lambda: cloud.clean_points(P, colors))                       # numpy in
    _assert_clean_is(a, want, P, colors)
    _assert_clean_is(b, want, P, colors)


def test_clean_points_other_parameters():
    P, _ = CS.injected()
    P = np.ascontiguousarray(P[::4])
    colors = np.zeros((len(P), 3), np.uint8)
    for kw in (dict(nb_neighbors=12, knn_ratio=2.0, eps_ratio=4.0, cluster_frac=0.01), dict(nb_neighbors=32, knn_ratio=1.5, eps_ratio=2.0, cluster_frac=0.5)):
        want = R.clean(P, k=kw['nb_neighbors'], knn_ratio=kw['knn_ratio'], eps_ratio=kw['eps_ratio'], cluster_frac=kw['cluster_frac'], jobs=JOBS)
        _assert_clean_is(cloud.clean_points(P, colors, **kw), want, P, colors)
    assert cloud.clean_points(P).colors is None


def test_clean_fused_removes_the_floater_and_its_depths():
    cams, depths, pairs = CS.two_spheres(6, (60, 80))
    images = np.random.RandomState(10).randint(0, 256, size=depths.shape + (3,)).astype(np.uint8)
    f = fusion.fuse_depths(cams, depths, pairs, images=images)
    pts = np_(f.points)
    fl = CS.near_floater(pts)
    assert int(fl.sum()) >= 50                                               # geometrically consistent: fusion keeps the floater
    want = R.clean(pts, jobs=JOBS)
    a, b = twice(lambda: cloud.clean_fused(f))
    for g in (a, b):
        sel = want['keep'] != 0
        assert isinstance(g, fusion.Fused) and len(g) == int(sel.sum()) == int(np_(g.cleaned.keep).sum())
        assert np.array_equal(np_(g.cleaned.keep), want['keep']) and same_bits(np_(g.cleaned.d), want['d'])
        assert same_bits(np_(g.points), pts[sel]) and np.array_equal(np_(g.colors), np_(f.colors)[sel])
        assert np.array_equal(np_(g.view), np_(f.view)[sel]) and np.array_equal(np_(g.pixel), np_(f.pixel)[sel])
        assert not CS.near_floater(np_(g.points)).any() and not want['keep'][fl].any()
        assert int((want['keep'][~fl] == 0).sum()) <= 0.01 * int((~fl).sum())
        expect = np_(f.fused_depths).copy()
        v, p = np_(f.view)[~sel], np_(f.pixel)[~sel]
        assert (expect[v, p // 80, p % 80] > 0).all()
        expect[v, p // 80, p % 80] = 0
        assert np.array_equal(np_(g.fused_depths), expect)                    # zero exactly at the removed (view, pixel) pairs
        assert g.masked_depths is f.masked_depths and g.counts is f.counts
    assert int((np_(f.fused_depths) > 0).sum()) == len(f)                     # the input is untouched
    with pytest.raises(TypeError):
        cloud.clean_fused(f, radius=1.0)


def _scale_mat(points_f32):
    lo, hi = points_f32.min(0), points_f32.max(0)
    sm = np.eye(4, dtype=np.float32)
    sm[:3, :3] *= (torch.from_numpy(hi - lo).max() * 1.1).item() / 2
    sm[:3, 3] = (lo + hi) / 2
    return sm


def test_convert_scene_clean_writes_the_cut_and_a_tighter_box(tmp_path, capsys):
    """What the feature is for: from Vis-MVSNet output with a floater to imfunc4/ in one command, cut.ply = the restatement's kept points, scale_mat
    = their box, smaller than the box of the whole fused cloud."""
    root, ids = CS.write_two_spheres(tmp_path / 'mvs')
    pair, cams, depths, probs = prepare.load_mvs_output(root)
    f = fusion.fuse_depths(cams, depths, prepare.pair_indices(pair), probs=probs, pthresh=(0.8, 0.7, 0.8))
    pts = np_(f.points)
    assert int(CS.near_floater(pts).sum()) >= 50
    common = dict(prob_mask=True, pthresh='.8,.7,.8', resize='128,96', crop='128,96', ext_image_path=os.path.join(root, '{:08}.jpg'))
    prepare.convert_scene(root, range_source='fused', **common)
    whole = np.load(os.path.join(root, 'imfunc4', 'cameras_hd.npz'))['scale_mat_0']
    out = prepare.convert_scene(root, range_source='clean', **common)
    want = R.clean(pts, jobs=JOBS)
    kept = pts[want['keep'] != 0].astype(np.float32)
    assert np.array_equal(chamfer.load_points(os.path.join(root, 'all_torch.ply')).astype(np.float32), pts.astype(np.float32))
    cut = chamfer.load_points(os.path.join(root, 'cut.ply'))
    assert np.array_equal(cut.astype(np.float32), kept) and np.array_equal(cut, kept.astype(np.float64))
    cams_hd = dict(np.load(os.path.join(out, 'cameras_hd.npz')))
    assert np.array_equal(cams_hd['scale_mat_0'], _scale_mat(kept))
    assert cams_hd['scale_mat_0'][0, 0] < whole[0, 0]                         # size / 2: the floater no longer inflates the box
    for i in range(len(ids)):                                                 # without fused_depth: the masked depths, as every other range_source
        assert np.array_equal(sio.load_pfm(os.path.join(out, 'depth', '%03d.pfm' % i)), np_(f.masked_depths[i]))
    pcd = prepare.convert_scene(root, range_source='pcd', **common)           # a later pcd run on the cut.ply it wrote reproduces the box
    assert np.array_equal(np.load(os.path.join(pcd, 'cameras_hd.npz'))['scale_mat_0'], cams_hd['scale_mat_0'])
    # the two tools, once each through main([...])
    root2 = str(tmp_path / 'mvs2')
    shutil.copytree(root, root2, ignore=shutil.ignore_patterns('imfunc4', '*.ply'))
    _tool('vismvsnet2mvsdf').main(['--data_root', root2, '--range_source', 'clean', '--prob_mask', '--pthresh', '.8,.7,.8', '--resize', '128,96',
                                   '--crop', '128,96', '--ext_image_path', os.path.join(root2, '{:08}.jpg'), '--fused_depth', '--cluster_frac', '0.9'])
    assert np.array_equal(chamfer.load_points(os.path.join(root2, 'cut.ply')).astype(np.float32), kept)
    g = cloud.clean_fused(f, cluster_frac=0.9)
    for i in range(len(ids)):
        assert np.array_equal(sio.load_pfm(os.path.join(root2, 'imfunc4', 'depth', '%03d.pfm' % i)), np_(g.fused_depths[i]))
    capsys.readouterr()
    _tool('clean_points').main([os.path.join(root, 'all_torch.ply'), str(tmp_path / 'cut_tool.ply')])
    printed = capsys.readouterr().out
    ply32 = chamfer.load_points(os.path.join(root, 'all_torch.ply'))          # the tool cleans what the file holds: fp32 coordinates
    want32 = R.clean(ply32, jobs=JOBS)
    assert '%d -> %d points' % (len(ply32), int(want32['keep'].sum())) in printed and '%d clusters' % want32['n_clusters'] in printed
    assert np.array_equal(chamfer.load_points(str(tmp_path / 'cut_tool.ply')), ply32[want32['keep'] != 0])
    from mvsdf_amd.mesh import _ply_elements
    vert = _ply_elements(str(tmp_path / 'cut_tool.ply'))['vertex']
    src = _ply_elements(os.path.join(root, 'all_torch.ply'))['vertex']
    assert np.array_equal(vert['red'], src['red'][want32['keep'] != 0])       # colours are kept


# ---------------------------------------------------------------- large: where brute force cannot follow
def _large_cloud(n=3_000_000):
    g = torch.Generator(device='cuda').manual_seed(11)
    uni = torch.rand(n - 10 * 100_000, 3, dtype=torch.float64, device='cuda', generator=g)
    cen = torch.rand(10, 3, dtype=torch.float64, device='cuda', generator=g)
    blobs = (cen[:, None] + 0.01 * torch.randn(10, 100_000, 3, dtype=torch.float64, device='cuda', generator=g)).reshape(-1, 3)
    P = torch.cat([uni, blobs])
    return P[torch.randperm(n, device='cuda', generator=g)].contiguous()


def _d2_rows(P, idx):
    q = P[idx]
    dx = q[:, None, 0] - P[None, :, 0]
    dy = q[:, None, 1] - P[None, :, 1]
    dz = q[:, None, 2] - P[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz                                      # separate elementwise kernels: nothing is contracted


def test_millions_of_points_knn_and_components():
    P = _large_cloud()
    n, k = P.shape[0], 20
    d, d_again = twice(lambda: cloud.knn_mean_distance(P, k))
    assert torch.equal(d, d_again) and bool(torch.isfinite(d).all())
    sample = torch.randperm(n, device='cuda', generator=torch.Generator(device='cuda').manual_seed(12))[:4096]
    for lo in range(0, 4096, 64):
        idx = sample[lo:lo + 64]
        D = _d2_rows(P, idx)
        D[torch.arange(len(idx), device='cuda'), idx] = float('inf')         # j != i by index
        s = torch.sort(torch.topk(D, k, dim=1, largest=False).values, dim=1).values.sqrt()
        acc = torch.zeros(len(idx), dtype=torch.float64, device='cuda')
        for j in range(k):
            acc = acc + s[:, j]
        want = acc / torch.full_like(acc, k)                                  # a tensor divisor: dividing by a Python number multiplies by 1 / k
        assert torch.equal(d[idx], want), (lo, int((d[idx] != want).sum()))
    eps = 0.004
    lab, lab_again = twice(lambda: cloud.radius_components(P, eps))
    assert torch.equal(lab, lab_again)
    ll = lab.long()
    assert torch.equal(ll[ll], ll) and bool((ll <= torch.arange(n, device='cuda')).all())
    for lo in range(0, 512, 64):
        idx = sample[lo:lo + 64]
        near = _d2_rows(P, idx) <= eps * eps
        r, c = torch.nonzero(near, as_tuple=True)
        assert torch.equal(ll[c], ll[idx][r]), lo                             # every point within eps of a sampled point has its label


def test_millions_of_points_in_lattices_of_known_components():
    side, count = 36, 64
    g = torch.stack(torch.meshgrid(*[torch.arange(side, dtype=torch.float64, device='cuda')] * 3, indexing='ij'), -1).reshape(-1, 3)
    origin = torch.stack(torch.meshgrid(*[torch.arange(4, dtype=torch.float64, device='cuda')] * 3, indexing='ij'), -1).reshape(-1, 3) * 100.0
    P = (origin[:, None] + g[None]).reshape(-1, 3)
    which = torch.arange(count, device='cuda').repeat_interleave(side ** 3)
    perm = torch.randperm(len(P), device='cuda', generator=torch.Generator(device='cuda').manual_seed(13))
    P, which = P[perm].contiguous(), which[perm]
    first = torch.full((count,), len(P), dtype=torch.int64, device='cuda').scatter_reduce(0, which, torch.arange(len(P), device='cuda'), 'amin')
    lab, lab_again = twice(lambda: cloud.radius_components(P, 1.0))           # eps = the lattice step, inclusive: a component per lattice
    assert torch.equal(lab, lab_again) and torch.equal(lab.long(), first[which])
    alone = cloud.radius_components(P, float(np.nextafter(1.0, 0)))
    assert torch.equal(alone.long(), torch.arange(len(P), device='cuda'))


def test_errors():
    P = np.random.RandomState(0).uniform(size=(500, 3))
    for bad in (np.nan, np.inf, -np.inf):
        Q = P.copy()
        Q[123, 1] = bad
        with pytest.raises(ValueError, match='NaN or infinite'):
            cloud.knn_mean_distance(Q, 8)
        with pytest.raises(ValueError, match='NaN or infinite'):
            cloud.radius_components(Q, 0.1)
        with pytest.raises(ValueError, match='NaN or infinite'):
            cloud.clean_points(Q)
    assert bool(torch.isfinite(cloud.knn_mean_distance(P, 8)).all())          # the device is fine afterwards
    for kw in (dict(points=P[:20], nb_neighbors=20), dict(points=P, nb_neighbors=33), dict(points=P.astype(np.float32)), dict(points=P[:, :2]),
               dict(points=torch.from_numpy(P).cuda().float()), dict(points=torch.from_numpy(P).cuda().reshape(-1))):
        with pytest.raises(ValueError):
            cloud.clean_points(**kw)
        with pytest.raises(ValueError):
            cloud.knn_mean_distance(**kw)
    from mvsdf_amd._lib import lib
    ws = torch.empty(1 << 20, dtype=torch.uint8, device='cuda')               # the C entry validates again
    p = torch.from_numpy(P).cuda()
    d = torch.empty(500, dtype=torch.float64, device='cuda')
    assert lib().mvsdf_cloud_knn(p.data_ptr(), 500, 33, ws.data_ptr(), 1 << 20, d.data_ptr(), None) != 0
    assert lib().mvsdf_cloud_knn(p.data_ptr(), 8, 8, ws.data_ptr(), 1 << 20, d.data_ptr(), None) != 0
    assert lib().mvsdf_cloud_knn(p.data_ptr(), 500, 8, ws.data_ptr(), 1024, d.data_ptr(), None) != 0
    assert lib().mvsdf_cloud_clean_workspace_bytes(1) == 0 and lib().mvsdf_cloud_clean_workspace_bytes(2 ** 31) == 0


# ---- the compaction's scan (csrc/geom_prims.h: mv_scan) at its chunk edges: 2048 items per workgroup, 1024 lanes in the top scan ----
def _compact_case(n, keep):
    """cloud.compact == torch boolean indexing in every carried array, and the header's n_kept == the number of set flags"""
    g = torch.Generator().manual_seed(n)
    pts = torch.rand(n, 3, dtype=torch.float64, generator=g).cuda()
    col = torch.randint(0, 256, (n, 3), dtype=torch.uint8, generator=g).cuda()
    a = torch.arange(n, dtype=torch.int32).cuda()
    b = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), dtype=torch.int32, generator=g).cuda()
    keep = keep.cuda()
    sel = keep.bool()
    want = int(sel.sum())
    got = cloud.compact(pts, keep, colors=col, a=a, b=b)                      # n_kept read from the header
    for t, src in zip(got, (pts, col, a, b)):
        assert t.shape[0] == want and torch.equal(t, src[sel])
    again = cloud.compact(pts, keep, colors=col, a=a, b=b, n_kept=want)       # the caller's capacity: nothing beyond it is written
    for t, src in zip(again, (pts, col, a, b)):
        assert torch.equal(t, src[sel])
    only = cloud.compact(pts, keep)
    assert only[1] is None and only[2] is None and only[3] is None and torch.equal(only[0], pts[sel])


@pytest.mark.parametrize('n', [1, 255, 256, 257, 2047, 2048, 2049, 4097])
def test_compact_at_the_scan_chunk_edges(n):
    i = torch.arange(n)
    for keep in (torch.ones(n), torch.zeros(n), i % 2, (i + 1) % 2, i == 0, i == n - 1):
        _compact_case(n, keep.to(torch.uint8))


def test_compact_with_more_chunks_than_top_scan_lanes():
    """n = 2048 * 1024 + 2049 makes 1026 chunks: every lane of the one-workgroup top scan owns two chunk totals (per = 2) and the last lanes none"""
    n = 2048 * 1024 + 2049
    keep = (torch.rand(n, generator=torch.Generator().manual_seed(7)) < 0.37).to(torch.uint8)
    _compact_case(n, keep)
    _compact_case(n, (torch.arange(n) == n - 1).to(torch.uint8))
