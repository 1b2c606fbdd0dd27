"""Cloud cleaning without a GPU: the numpy restatement (tests/cloud_ref.py) on hand-made clouds with known answers, the scene condition of
tests/test_gpu_cloud.py asserted on the restatement alone, the tools' argument parsing and the host-side refusals of mvsdf_amd/cloud.py."""
import importlib.util
import os

import numpy as np
import pytest

import cloud_ref as R
import cloud_scene as CS
from conftest import ROOT


def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_' + name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def lattice(nx, ny, nz, step=1.0, origin=(0.0, 0.0, 0.0)):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing='ij'), -1).reshape(-1, 3).astype(np.float64)
    return g * step + np.asarray(origin, np.float64)


def two_lattices():
    """a 5x5x5 lattice (125 points, indices 0..124), a 4x4x4 one 100 away (64 points, 125..188) and 3 far points (189..191)"""
    far = np.array([[1000.0, 0, 0], [0, 1000.0, 0], [0, 0, -1000.0]])
    return np.concatenate([lattice(5, 5, 5), lattice(4, 4, 4, origin=(100.0, 0, 0)), far])


def test_knn_of_a_lattice_and_an_exact_duplicate():
    P = lattice(5, 5, 5)
    d = R.knn_mean_distance(P, 3)
    assert np.array_equal(d, np.ones(125))                                   # every lattice point has at least 3 neighbours at distance 1
    d6 = R.knn_mean_distance(P, 6)
    centre = 2 * 25 + 2 * 5 + 2
    assert d6[centre] == 1.0
    corner = ((np.sqrt(1.0) + np.sqrt(1.0)) + np.sqrt(1.0) + np.sqrt(2.0) + np.sqrt(2.0) + np.sqrt(2.0)) / 6
    assert d6[0] == corner                                                   # 3 at distance 1, then 3 at sqrt 2, summed left to right
    Q = np.concatenate([P, P[7:8]])                                          # an exact duplicate of point 7: a neighbour at distance 0, not self
    dq = R.knn_mean_distance(Q, 1)
    assert dq[7] == 0.0 and dq[125] == 0.0 and dq[8] == 1.0
    dq2 = R.knn_mean_distance(Q, 2)
    assert dq2[7] == 0.5 and dq2[125] == 0.5


def test_lower_median_is_an_element():
    assert R.lower_median(np.array([4.0, 1.0, 3.0, 2.0])) == 2.0             # rank (4 - 1) // 2 = 1
    assert R.lower_median(np.array([5.0, 1.0, 3.0])) == 3.0


def test_components_are_inclusive_at_eps():
    P = lattice(4, 3, 2, step=0.5)
    assert np.array_equal(R.radius_components(P, 0.5), np.zeros(24, np.int32))                # d2 == eps * eps counts
    assert np.array_equal(R.radius_components(P, np.nextafter(0.5, 0)), np.arange(24, dtype=np.int32))
    line = np.stack([np.arange(50.0), np.zeros(50), np.zeros(50)], 1)[np.random.RandomState(0).permutation(50)]
    assert np.array_equal(R.radius_components(line, 1.0), np.zeros(50, np.int32))             # a chain: one component, label = index 0


def test_clean_two_lattices_labels_counts_and_cluster_frac():
    P = two_lattices()
    c = R.clean(P, k=3, knn_ratio=3.0, eps_ratio=1.5, cluster_frac=1.0)
    assert c['median'] == 1.0 and c['threshold'] == 3.0 and c['eps'] == 1.5
    assert c['n_passed'] == 189 and not c['passed'][189:].any()             # the far points are sparse
    assert np.array_equal(c['labels'], np.concatenate([np.zeros(125), np.full(64, 125), np.full(3, -1)]).astype(np.int32))
    assert (c['n_clusters'], c['largest']) == (2, 125)
    assert np.array_equal(c['keep'], np.concatenate([np.ones(125), np.zeros(67)]).astype(np.uint8))      # 64 < 1.0 * 125
    c3 = R.clean(P, k=3, knn_ratio=3.0, eps_ratio=1.5, cluster_frac=0.3)
    assert np.array_equal(c3['keep'], np.concatenate([np.ones(189), np.zeros(3)]).astype(np.uint8))      # 64 >= 0.3 * 125 = 37.5
    c6 = R.clean(P, k=3, knn_ratio=3.0, eps_ratio=1.5, cluster_frac=0.52)
    assert int(c6['keep'].sum()) == 125                                      # 64 < 65
    order = np.random.RandomState(1).permutation(len(P))                     # labels follow the input index, whatever the order
    cs = R.clean(P[order], k=3, knn_ratio=3.0, eps_ratio=1.5)
    inv = np.argsort(order)
    assert cs['labels'][inv[0]] == min(inv[:125]) and cs['labels'][inv[125]] == min(inv[125:189])
    assert np.array_equal(cs['keep'][inv], c['keep'])


def test_two_components_of_equal_size_are_both_kept():
    P = np.concatenate([lattice(3, 3, 3), lattice(3, 3, 3, origin=(50.0, 0, 0)), lattice(2, 2, 2, origin=(0, 50.0, 0))])
    c = R.clean(P, k=3, knn_ratio=3.0, eps_ratio=1.5, cluster_frac=1.0)
    assert (c['n_clusters'], c['largest']) == (3, 27)
    assert np.array_equal(c['keep'], np.concatenate([np.ones(54), np.zeros(8)]).astype(np.uint8))


def test_the_scene_condition_holds_for_the_restatement():
    """The condition of test_gpu_cloud.py's scene, on the restatement alone: none of the 700 injected points is kept and at most 1 % of the fused
    points are lost.  A CPU prototype of the definition counted 22 096 fused points and 81 lost (58 in stage B, 23 in stage C)."""
    P, injected = CS.injected()
    assert int(injected.sum()) == 700 and int((~injected).sum()) == 22096
    c = R.clean(P)
    lost = int((c['keep'][~injected] == 0).sum())
    print('fused %d, injected kept %d, fused lost %d (stage B %d)' % (int((~injected).sum()), int(c['keep'][injected].sum()), lost,
                                                                       int((~c['passed'][~injected]).sum())))
    assert int(c['keep'][injected].sum()) == 0
    assert lost <= 0.01 * int((~injected).sum())
    assert lost == 81 and int((~c['passed'][~injected]).sum()) == 58


def test_two_sphere_scene_has_a_consistent_floater_that_the_cut_removes():
    import fusion_ref
    cams, depths, pairs = CS.two_spheres(6, (48, 64))
    f = fusion_ref.fuse(cams, depths, pairs)
    fl = CS.near_floater(f['points'])
    assert int(fl.sum()) >= 50                                               # fusion keeps it: every view sees it
    c = R.clean(f['points'])
    assert int(c['keep'][fl].sum()) == 0 and int((c['keep'][~fl] == 0).sum()) <= 0.01 * int((~fl).sum())


def test_converter_parse_args_clean_flags():
    t = _tool('vismvsnet2mvsdf')
    a = t.parse_args('--data_root D --range_source clean'.split())
    assert a.range_source == 'clean' and a.clean == {}
    a = t.parse_args('--range_source clean --nb_neighbors 12 --knn_ratio 2.5 --eps_ratio 4 --cluster_frac 0.3'.split())
    assert a.clean == {'nb_neighbors': 12, 'knn_ratio': 2.5, 'eps_ratio': 4.0, 'cluster_frac': 0.3}
    assert t.parse_args([]).clean == {} and t.parse_args([]).range_source == 'pcd'
    for bad in (['--range_source', 'fused', '--knn_ratio', '2'], ['--nb_neighbors', '8'], ['--range_source', 'cleaned']):
        with pytest.raises(SystemExit):
            t.parse_args(bad)


def test_clean_points_tool_parse_args():
    t = _tool('clean_points')
    a = t.parse_args(['in.ply', 'out.ply'])
    assert (a.input, a.output, a.nb_neighbors, a.knn_ratio, a.eps_ratio, a.cluster_frac) == ('in.ply', 'out.ply', 20, 3.0, 3.0, 1.0)
    a = t.parse_args('a.ply b.ply --nb_neighbors 8 --knn_ratio 2 --eps_ratio 5 --cluster_frac 0.5'.split())
    assert (a.nb_neighbors, a.knn_ratio, a.eps_ratio, a.cluster_frac) == (8, 2.0, 5.0, 0.5)
    for bad in (['a.ply'], ['a.ply', 'a.ply'], ['a.ply', 'b.ply', '--nb_neighbors', '33'], ['a.ply', 'b.ply', '--nb_neighbors', '0'],
                ['a.ply', 'b.ply', '--knn_ratio', '0'], ['a.ply', 'b.ply', '--eps_ratio', '-1'], ['a.ply', 'b.ply', '--eps_ratio', 'nan'],
                ['a.ply', 'b.ply', '--cluster_frac', '1.5'], ['a.ply', 'b.ply', '--cluster_frac', '0']):
        with pytest.raises(SystemExit):
            t.parse_args(bad)


def test_clean_points_refuses_bad_arguments_before_any_launch():
    """every one of these is a ValueError raised on the host: none needs the library or a GPU"""
    from mvsdf_amd import cloud
    P = np.random.RandomState(0).uniform(size=(40, 3))
    bad = [dict(points=P.astype(np.float32)), dict(points=P.reshape(-1)), dict(points=P[:, :2]), dict(points=np.zeros((0, 3))),
           dict(points=P.tolist()), dict(points=P[:20], nb_neighbors=20), dict(points=P, nb_neighbors=33), dict(points=P, nb_neighbors=0),
           dict(points=P, nb_neighbors=2.5), dict(points=P, knn_ratio=0.0), dict(points=P, knn_ratio=float('nan')),
           dict(points=P, eps_ratio=float('inf')), dict(points=P, eps_ratio=-1.0), dict(points=P, cluster_frac=0.0),
           dict(points=P, cluster_frac=1.0001), dict(points=P, colors=np.zeros((40, 3), np.float32)), dict(points=P, colors=np.zeros((39, 3), np.uint8))]
    for kw in bad:
        with pytest.raises(ValueError):
            cloud.clean_points(**kw)
    for kw in (dict(points=P.astype(np.float32)), dict(points=P[:8], nb_neighbors=8), dict(points=P, nb_neighbors=33)):
        with pytest.raises(ValueError):
            cloud.knn_mean_distance(**kw)
    for kw in (dict(points=P.astype(np.float32), eps=1.0), dict(points=P, eps=0.0), dict(points=P, eps=float('nan')), dict(points=P[:1], eps=1.0)):
        with pytest.raises(ValueError):
            cloud.radius_components(**kw)


def test_convert_scene_refuses_clean_keywords_without_clean(tmp_path):
    from mvsdf_amd.datasets import prepare
    with pytest.raises(ValueError):
        prepare.convert_scene(str(tmp_path), range_source='fused', clean={'knn_ratio': 2.0})
    with pytest.raises(ValueError):
        prepare.convert_scene(str(tmp_path), range_source='cleaned')
