"""mvsdf_amd/normals.py on the GPU against its numpy restatement (tests/normals_ref.py): neighbour rows, normals and variation, the oriented normals,
labels and counts are compared bit for bit (np.array_equal on uint64 / int32 views), every call made twice.  The sign stages are fed the restatement's
normals, so each is judged on its own.  `rounds` IS asserted: it equals the restatement's Boruvka count, a property of the graph."""
import functools
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normals_ref as R  # noqa: E402
from mvsdf_amd import chamfer, fusion, normals, poisson  # noqa: E402

pytestmark = pytest.mark.gpu
JOBS = 16                                                                    # threads of the restatement's brute force
KINDS = ['uniform', 'plane', 'line', 'offset', 'duplicates', 'lattice']
KS = (1, 8, 20, 32)


def _tool(name):
    spec = importlib.util.spec_from_file_location('tool_' + name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def np_(t):
    return t.cpu().numpy()


def make_cloud(kind, n, seed=0):
    """the clouds of tests/test_gpu_cloud.py"""
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


def sphere(n, seed, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """-> (points, analytic outward normals)"""
    x = np.random.RandomState(seed).normal(size=(n, 3))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x * radius + np.asarray(centre), x


def twice(fn):
    a, b = fn(), fn()
    return a, b


# ================================================================ neighbours and normals ================================================================
def _check_rows(P, k, idx, d2, device_input):
    """knn_indices and estimate_normals at k against the restatement's rows idx / d2 ([N, >= k]: a shorter row is a prefix under a total order)"""
    tag = (len(P), k)
    src = torch.from_numpy(P).cuda() if device_input else P
    want_i, want_d = np.ascontiguousarray(idx[:, :k]), np.ascontiguousarray(d2[:, :k])
    (gi, gd), (gi2, gd2) = twice(lambda: [np_(t) for t in normals.knn_indices(src, k, return_distances=True)])
    assert gi.dtype == np.int32 and np.array_equal(gi, want_i), (tag, int((gi != want_i).sum()))
    assert same_bits(gd, want_d), tag
    assert np.array_equal(gi, gi2) and same_bits(gd, gd2), tag
    assert np.array_equal(np_(normals.knn_indices(src, k)), want_i), tag
    want_n, want_v = R.normals_from_covariance(R.covariance(P, want_i))
    (n1, v1, i1), (n2, v2, i2) = twice(lambda: [np_(t) for t in normals.estimate_normals(src, k)])
    assert np.array_equal(i1, want_i) and np.array_equal(i2, want_i), tag
    assert same_bits(n1, want_n), (tag, int((bits(n1) != bits(want_n)).any(1).sum()))
    assert same_bits(v1, want_v), (tag, int((bits(v1) != bits(want_v)).sum()))
    assert same_bits(n1, n2) and same_bits(v1, v2), tag


@pytest.mark.parametrize('kind', KINDS)
def test_rows_and_normals_are_the_restatement(kind):
    sizes = (17, 257, 4099) + ((30011,) if kind in ('uniform', 'lattice') else ())
    for n in sizes:
        P = make_cloud(kind, n)
        ks = [k for k in KS if k + 1 <= n]
        idx, d2 = R.knn_indices(P, max(ks), jobs=JOBS)
        for k in ks:
            _check_rows(P, k, idx, d2, device_input=k == 8)
    for k in KS:                                                             # the smallest cloud a k allows
        P = make_cloud(kind, k + 1, seed=5)
        idx, d2 = R.knn_indices(P, k)
        _check_rows(P, k, idx, d2, device_input=False)


def test_rows_at_every_list_capacity():
    """the kernel keeps its pairs in 8 / 16 / 24 / 32 slots: k at and beside each capacity, on the cloud with exact duplicates"""
    P = make_cloud('duplicates', 4099, seed=3)
    idx, d2 = R.knn_indices(P, 32, jobs=JOBS)
    for k in (7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32):
        _check_rows(P, k, idx, d2, device_input=k % 2 == 0)


# ================================================================ the sign, on the restatement's normals ================================================================
def _check_orient(P, N, nb, **kw):
    """orient_normals twice against the restatement -> the restatement's (normals, labels, n_components, rounds)"""
    want = R.orient_normals(P, N, nb, **kw)
    a, b = twice(lambda: normals.orient_normals(P, N, nb, **kw))
    for got in (a, b):
        out, labels, n_components, rounds = got
        assert labels.dtype == torch.int32 and np.array_equal(np_(labels), want[1])
        assert same_bits(np_(out), want[0]), int((bits(np_(out)) != bits(want[0])).any(1).sum())
        assert (n_components, rounds) == (want[2], want[3]), (n_components, rounds, want[2], want[3])
    return want


@functools.lru_cache(None)
def _sphere_case():
    P, want = sphere(4099, 11)
    nb, _ = R.knn_indices(P, 12, jobs=JOBS)
    return P, want, nb


def test_orient_random_signs_on_a_sphere():
    P, want, nb = _sphere_case()
    sign = np.where(np.random.RandomState(0).uniform(size=(len(P), 1)) < 0.5, -1.0, 1.0)
    out, labels, n_components, rounds = _check_orient(P, want * sign, nb)
    assert n_components == 1 and (labels == 0).all() and same_bits(out, want)           # all outward: the analytic normals themselves
    out, _, _, _ = _check_orient(P, want * sign, nb, up=(0.3, -1.0, 0.2))
    assert same_bits(out, want)
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (P, want * sign, nb)]
    got = normals.orient_normals(*dev)                                       # device tensors in
    assert same_bits(np_(got.normals), want) and got.n_components == 1


def test_orient_rows_of_zero_normals():
    P, want, nb = _sphere_case()
    rs = np.random.RandomState(1)
    N = want * np.where(rs.uniform(size=(len(P), 1)) < 0.5, -1.0, 1.0)
    N[rs.choice(len(P), 60, replace=False)] = 0.0
    N[np.argmax(P[:, 2])] = 0.0                                              # the reference point of the up rule among them
    _check_orient(P, N, nb)


def test_orient_plane_with_identical_normals():
    """every |dot| is exactly 1: the tree is decided by the index order alone; every height under `up` is equal: the reference point is the lowest index"""
    P = make_cloud('plane', 4099)
    nb, _ = R.knn_indices(P, 8, jobs=JOBS)
    N = np.tile(np.array([[0.0, 0.0, 1.0]]), (len(P), 1))
    out, labels, n_components, _ = _check_orient(P, N, nb)
    assert n_components == 1 and same_bits(out, N)
    out, _, _, _ = _check_orient(P, N, nb, up=(0.0, 0.0, -1.0))
    assert same_bits(out, -N)
    N2 = N.copy()
    N2[0] = -N2[0]                                                           # the lowest index decides: the others follow it
    out, _, _, _ = _check_orient(P, N2, nb)
    assert same_bits(out, N)
    _check_orient(P, N2, nb, up=(0.0, 0.0, 0.0))                             # every product with `up` is 0: nothing is < 0


def test_orient_three_components():
    k = 10
    a, na = sphere(1201, 21)
    b, nb_ = sphere(1303, 22, radius=0.5, centre=(40.0, 0.0, 0.0))
    c = np.random.RandomState(23).uniform(-0.01, 0.01, size=(k + 1, 3)) + np.array([0.0, 90.0, 0.0])
    P = np.concatenate([a, c, b])
    want = np.concatenate([na, np.tile([[0.0, 0.0, 1.0]], (k + 1, 1)), nb_])
    nb, _ = R.knn_indices(P, k, jobs=JOBS)
    N = want * np.where(np.random.RandomState(24).uniform(size=(len(P), 1)) < 0.5, -1.0, 1.0)
    out, labels, n_components, _ = _check_orient(P, N, nb)
    assert n_components == 3 and sorted(set(labels.tolist())) == [0, 1201, 1201 + k + 1]
    assert same_bits(out, want)


@pytest.mark.parametrize('k', [1, 2, 8, 32])
def test_orient_smallest_cloud(k):
    rs = np.random.RandomState(k)
    P, N = rs.uniform(-1, 1, (k + 1, 3)), rs.normal(size=(k + 1, 3))
    nb, _ = R.knn_indices(P, k)
    _check_orient(P, N, nb)


def test_orient_chain():
    """4,099 points on a line, k = 2, normals turning by ever smaller steps: every point's best edge leads to its right neighbour, so the first round
    hooks one chain of N roots -- beyond the hop bound of one lane -- and ends everything; the flips alternate at random"""
    n = 4099
    P = np.stack([np.arange(n, dtype=np.float64), np.zeros(n), np.zeros(n)], 1)
    nb, _ = R.knn_indices(P, 2, jobs=JOBS)
    assert np.array_equal(nb[1:-1], np.stack([np.arange(0, n - 2), np.arange(2, n)], 1))
    t = np.concatenate([[0.0], np.cumsum(np.linspace(0.5, 0.1, n - 1))])
    N = np.stack([np.cos(t), np.sin(t), np.zeros(n)], 1) * np.where(np.random.RandomState(2).uniform(size=(n, 1)) < 0.5, -1.0, 1.0)
    lo, hi, _ = R.edges(N, nb)
    first = np.full(n, -1)                                                   # the premise: every point's first edge of the order is the one to its right
    for e in range(len(lo) - 1, -1, -1):
        first[lo[e]] = first[hi[e]] = e
    assert np.array_equal(lo[first[:-1]], np.arange(n - 1)) and np.array_equal(hi[first[:-1]], np.arange(1, n))
    assert (lo[first[-1]], hi[first[-1]]) == (n - 2, n - 1)
    out, labels, n_components, rounds = _check_orient(P, N, nb)
    assert (n_components, rounds) == (1, 1)
    assert (R.dot3(out[:-1], out[1:]) > 0).all()


@functools.lru_cache(None)
def _cap_case():
    """the lower cap of a sphere, whose rim makes the up rule turn it inward, two centres below it"""
    P, want = sphere(4099, 6)
    keep = P[:, 2] < -0.2
    P, want = np.ascontiguousarray(P[keep]), np.ascontiguousarray(want[keep])
    nb, _ = R.knn_indices(P, 12, jobs=JOBS)
    return P, want, nb, np.array([[0.5, 0.0, -4.0], [-0.5, 0.3, -5.0], [0.1, 0.2, 6.0]])


def test_orient_view_vote_in_all_three_visibility_forms():
    P, want, nb, C = _cap_case()
    n = len(P)
    N = want * np.where(np.random.RandomState(3).uniform(size=(n, 1)) < 0.5, -1.0, 1.0)
    by_up, _, _, _ = _check_orient(P, N, nb)
    assert same_bits(by_up, -want)                                           # the wrong way
    view = np.random.RandomState(4).randint(0, 2, n).astype(np.int32)        # one seeing view per point, never the one above
    mask = np.zeros((3, n), np.uint8)
    mask[view, np.arange(n)] = 1
    tracks = (np.arange(n + 1, dtype=np.int64), view)
    outs = [_check_orient(P, N, nb, centers=C, visibility=v)[0] for v in (mask, mask.astype(bool), tracks, view)]
    assert all(same_bits(o, want) for o in outs)
    got = normals.orient_normals(P, N, nb, centers=torch.from_numpy(C).cuda(), visibility=torch.from_numpy(view).cuda())
    assert same_bits(np_(got.normals), want)
    rs = np.random.RandomState(5)                                            # several views per point, some seen by none, a view listed twice
    mask = (rs.uniform(size=(3, n)) < 0.5).astype(np.uint8)
    off = np.concatenate([[0], np.cumsum(mask.sum(0))]).astype(np.int64)
    tv = np.nonzero(mask.T)[1].astype(np.int32)
    a = _check_orient(P, N, nb, centers=C, visibility=mask)[0]
    b = _check_orient(P, N, nb, centers=C, visibility=(off, tv))[0]
    assert same_bits(a, b)
    off2, tv2 = off.copy(), np.concatenate([tv[:1], tv])
    off2[1:] += 1
    if off[1] > 0:
        assert same_bits(_check_orient(P, N, nb, centers=C, visibility=(off2, tv2))[0], a)


def test_orient_view_vote_tie_falls_back_to_up():
    P = np.array([[0.0, 0, 0], [1.0, 0, 0]])
    N = np.array([[0.0, 0, 1], [0.0, 0, 1]])
    nb = np.array([[1], [0]], np.int32)
    C = np.array([[0.5, 0, 2.0], [0.5, 0, -2.0]])
    vis = np.array([[1, 0], [0, 1]], np.uint8)
    for up, sign in (((0, 0, 1), 1.0), ((0, 0, -1), -1.0)):
        out, _, _, _ = _check_orient(P, N, nb, up=up, centers=C, visibility=vis)
        assert same_bits(out, sign * N)


def test_orient_to_views():
    P, want, nb, C = _cap_case()
    n = len(P)
    rs = np.random.RandomState(7)
    N = want * np.where(rs.uniform(size=(n, 1)) < 0.5, -1.0, 1.0)
    mask = (rs.uniform(size=(3, n)) < 0.6).astype(np.uint8)
    mask[:, :40] = 0                                                         # seen by nobody: unchanged
    mask[:, 40:80] = np.array([[1], [0], [1]])                               # one centre below and the one above: mostly one vote each way, a tie
    off = np.concatenate([[0], np.cumsum(mask.sum(0))]).astype(np.int64)
    tv = np.nonzero(mask.T)[1].astype(np.int32)
    ref = R.orient_to_views(P, N, C, mask)
    neg, pos = R.votes(P, N, C, mask != 0)
    assert (neg[40:80] == pos[40:80]).sum() > 20 and (neg > pos).sum() > 100 and (neg < pos).sum() > 100
    assert same_bits(ref[:80][neg[:80] == pos[:80]], N[:80][neg[:80] == pos[:80]])
    for vis in (mask, mask.astype(bool), (off, tv)):
        a, b = twice(lambda: np_(normals.orient_to_views(P, N, C, vis)))
        assert same_bits(a, ref) and same_bits(a, b)
    view = rs.randint(0, 3, n).astype(np.int32)
    got = np_(normals.orient_to_views(torch.from_numpy(P).cuda(), torch.from_numpy(N).cuda(), C, view))
    assert same_bits(got, R.orient_to_views(P, N, C, view))


# ================================================================ end to end ================================================================
def _closed(faces):
    f = np.asarray(faces, np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    return len(f) > 0 and (counts == 2).all()


def test_sphere_to_poisson_mesh():
    """estimate_normals -> orient_normals -> poisson_mesh(depth=5, trim=False) on a unit sphere of 4,099 points: a closed mesh whose vertices lie as
    near the sphere as those of the mesh from the analytic normals x / |x| on the same cloud and grid, plus one voxel (the estimated normals differ
    from the analytic ones by under 4 degrees, and the grid resolves no less than a voxel).  Measured on an MI355X: max | |v| - 1 | = 0.011613
    from the analytic normals, 0.012494 from the estimated ones, the voxel is 0.068743 (8,044 faces)."""
    P, want = sphere(4099, 31)
    nrm, var, nb = normals.estimate_normals(P, 16)
    o = normals.orient_normals(P, nrm, nb)
    assert o.n_components == 1
    est = np_(o.normals)
    assert ((est * want).sum(1) > 0).all()
    m_ref, f_ref = poisson.poisson_mesh(P, want, depth=5, trim=False)
    m_est, f_est = poisson.poisson_mesh(P, o.normals, depth=5, trim=False)
    assert m_ref is not None and m_est is not None and len(m_est) > 0 and f_est.voxel == f_ref.voxel
    assert _closed(np_(m_est.faces)) and _closed(np_(m_ref.faces))
    dev_ref = float(np.abs(np.linalg.norm(np_(m_ref.vertices).astype(np.float64), axis=1) - 1).max())
    dev_est = float(np.abs(np.linalg.norm(np_(m_est.vertices).astype(np.float64), axis=1) - 1).max())
    print('sphere -> poisson: analytic %.6f estimated %.6f voxel %.6f faces %d' % (dev_ref, dev_est, f_ref.voxel, len(m_est)))
    assert dev_est <= dev_ref + f_ref.voxel


def test_poisson_tool_on_a_cloud_without_normals(tmp_path, capsys):
    P, _ = sphere(4099, 32)
    ply, out = str(tmp_path / 'bare.ply'), str(tmp_path / 'mesh.ply')
    fusion.save_points(ply, P)
    tool = _tool('poisson_mesh')
    with pytest.raises(SystemExit) as e:
        tool.main([ply, out, '--depth', '5'])
    assert str(e.value.code) == 'poisson_mesh: %s has no nx / ny / nz (tools/fusion.py --normals writes them)' % ply and not os.path.exists(out)
    tool.main([ply, out, '--depth', '5', '--estimate_normals'])
    assert 'normals: estimated from 16 neighbours, 1 components' in capsys.readouterr().out
    from mvsdf_amd.mesh import load_mesh
    assert len(load_mesh(out)) > 100


def test_estimate_normals_tool_on_a_colmap_model(tmp_path):
    import colmap_scene as S                                                 # the synthetic model of the view-selection tests, read only
    model = S.make_scene(n_views=6, n_points=300, seed=3)
    d, out = str(tmp_path / 'sparse'), str(tmp_path / 'oriented.ply')
    S.write_binary(model, d)
    _tool('estimate_normals').main(['--colmap', d, out, '--k', '10'])
    pts, centres, _, vis = S.scene_arrays(model)
    N, _, _ = R.estimate_normals(pts, 10)
    want = R.orient_to_views(pts, N, centres, vis)
    got_p, got_n = chamfer.load_oriented_points(out)
    assert np.array_equal(got_p.astype(np.float32), pts.astype(np.float32))
    assert np.array_equal(got_n.astype(np.float32).view(np.uint32), want.astype(np.float32).view(np.uint32))      # the file holds floats
    assert (np.abs(want - N).sum(1) > 0).sum() > 20                           # the tracks did turn some



def test_estimate_normals_tool_on_mvs_output(tmp_path):
    """--data_root fuses the directory and signs the tree's components by the views the points came from: the file holds what the calls give"""
    import mvs_scene as MS                                                   # the synthetic Vis-MVSNet output of the fusion tests, read only
    from mvsdf_amd import viewsel
    from mvsdf_amd.datasets import prepare
    root, _ = MS.write_mvs_scene(tmp_path / 'scene', n_views=4, depth_hw=(20, 28), img_wh=(96, 72))
    out = str(tmp_path / 'oriented.ply')
    _tool('estimate_normals').main(['--data_root', root, out, '--k', '8'])
    pair, cams, depths, probs = prepare.load_mvs_output(root)
    fused = fusion.fuse_depths(cams, depths, prepare.pair_indices(pair), probs=probs)
    nrm, _, nb = normals.estimate_normals(fused.points, 8)
    want = normals.orient_normals(fused.points, nrm, nb, centers=np.ascontiguousarray(viewsel.centers_from_cams(cams)), visibility=fused.view)
    got_p, got_n = chamfer.load_oriented_points(out)
    assert len(got_p) == len(fused.points) > 100
    assert np.array_equal(got_n.astype(np.float32).view(np.uint32), np_(want.normals).astype(np.float32).view(np.uint32))
    ref = R.orient_normals(np_(fused.points), np_(nrm), np_(nb), centers=viewsel.centers_from_cams(cams), visibility=np_(fused.view))
    assert same_bits(np_(want.normals), ref[0]) and np.array_equal(np_(want.labels), ref[1])


# ================================================================ error paths ================================================================
def test_non_finite_input_raises_through_the_error_bits():
    P, want, nb = _sphere_case()
    for bad in (np.nan, np.inf):
        Q = P.copy()
        Q[1234, 1] = bad
        for f in (lambda: normals.knn_indices(Q, 8), lambda: normals.estimate_normals(Q, 8), lambda: normals.orient_normals(Q, want, nb),
                  lambda: normals.orient_to_views(Q, want, np.zeros((1, 3)), np.ones((1, len(P)), np.uint8))):
            with pytest.raises(ValueError, match='coordinate'):
                f()
        M = want.copy()
        M[4000, 2] = bad
        with pytest.raises(ValueError, match='normal'):
            normals.orient_normals(P, M, nb)
        with pytest.raises(ValueError, match='normal'):
            normals.orient_to_views(P, M, np.zeros((1, 3)), np.ones((1, len(P)), np.uint8))
        with pytest.raises(ValueError, match='centre'):
            normals.orient_normals(P, want, nb, centers=np.array([[0.0, bad, 0.0]]), visibility=np.ones((1, len(P)), np.uint8))
    for j in (-1, len(P)):
        nb2 = nb.copy()
        nb2[77, 3] = j
        with pytest.raises(ValueError, match='neighbour index'):
            normals.orient_normals(P, want, nb2)
    with pytest.raises(ValueError):                                          # a view index outside [0, V)
        normals.orient_to_views(P, want, np.zeros((2, 3)), np.full(len(P), 2, np.int32))
    got = normals.orient_normals(P, want, nb)                                # and the next good call is unaffected
    assert same_bits(np_(got.normals), want)
