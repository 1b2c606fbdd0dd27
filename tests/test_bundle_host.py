"""tests/bundle_ref.py, the numpy restatement of mvsdf_amd/bundle.py's definition, held to truth on the CPU: its Jacobians against autograd, its
exponential against numpy's sine and cosine, its matrix-free Schur product and solver against dense linear algebra, and the whole adjustment
against scenes with known cameras and points.  The device is held to the restatement in tests/test_gpu_bundle.py.

Bounds measured on the restatement (the assertions take twice these, as the definition's issue asks):
  exponential against np.sin / np.cos Rodrigues over [0, 1]: worst entry difference 2.3e-16;
  noise-free 4-view scene, seed 0, 15 iterations: centres return to 1.8e-15, points to 1.8e-15 -> the floor of 1e-12 applies."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bundle_ref as ref  # noqa: E402
import bundle_scene as bs  # noqa: E402
from mvsdf_amd import bundle  # noqa: E402

EXP_MEASURED = 2.3e-16
TRUTH_BOUND = 1e-12


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def test_tables_and_host_helpers_agree_with_the_module():
    assert np.array_equal(ref.rodrigues_table(), bundle.rodrigues_table())
    assert (ref.MAX_THETA, ref.ROD_TERMS, ref.FLOOR) == (bundle.MAX_THETA, bundle.ROD_TERMS, bundle.FLOOR)
    s = bs.make_scene(skew=0.7)
    for a, b in zip(ref.pose_arrays(s.cams), bundle.pose_arrays(s.cams)):
        assert np.array_equal(a, b)
    pose, _ = ref.pose_arrays(s.cams)
    assert np.array_equal(bundle.cams_with(s.cams_true, pose), s.cams)


def test_quaternion_round_trip():
    from mvsdf_amd.datasets.colmap import rotation
    rs = np.random.RandomState(3)
    for k in range(12):
        w = rs.normal(size=3)
        w = w / np.linalg.norm(w) * [0.01, 1.0, 2.0, 3.1, np.pi, 3.0][k % 6]
        R = bs.rotation(w)
        q = bundle.quaternion(R)
        assert q[0] >= 0 and abs(np.linalg.norm(q) - 1) < 1e-14
        assert np.abs(rotation(q) - R).max() < 1e-14


def test_jacobians_against_autograd():
    s = bs.make_scene(skew=0.7, shuffle=True, seed=2)
    assert (s.cams[:, 1, 0, 1] != 0).all() and (s.cams[:, 1, 0, 0] != s.cams[:, 1, 1, 1]).all()
    pose, intr = ref.pose_arrays(s.cams)
    lin = ref.linearise(pose, intr, s.xyz, s.off, s.view, s.obs)
    owner = np.repeat(np.arange(len(s.off) - 1), np.diff(s.off))

    def residual(p, R, t, k, xy):
        w, u, X = p[:3], p[3:6], p[6:]
        th = torch.sqrt((w * w).sum() + 1e-300)
        Kx = torch.zeros(3, 3, dtype=torch.float64)
        Kx[0, 1], Kx[0, 2], Kx[1, 0], Kx[1, 2], Kx[2, 0], Kx[2, 1] = -w[2], w[1], w[2], -w[0], -w[1], w[0]
        E = torch.eye(3, dtype=torch.float64) + torch.sin(th) / th * Kx + (1 - torch.cos(th)) / (th * th) * (Kx @ Kx)
        q = E @ (R @ X + t) + u
        return torch.stack([k[0] * q[0] / q[2] + k[1] * q[1] / q[2] + k[2] - xy[0], k[3] * q[1] / q[2] + k[4] - xy[1]])

    worst = 0.0
    for o in range(0, len(s.view), 7):
        v, j = s.view[o], owner[o]
        R, t = torch.from_numpy(pose[v, :9].reshape(3, 3).copy()), torch.from_numpy(pose[v, 9:].copy())
        p0 = torch.cat([torch.zeros(6, dtype=torch.float64), torch.from_numpy(s.xyz[j].copy())])
        J = torch.autograd.functional.jacobian(lambda p: residual(p, R, t, torch.from_numpy(intr[v].copy()), torch.from_numpy(s.obs[o].copy())), p0).numpy()
        worst = max(worst, _rel(lin.A[o], J[:, :6]), _rel(lin.B[o], J[:, 6:]))
    print('worst relative Jacobian difference', worst)
    assert worst <= 1e-9


def test_exponential_polynomial():
    rs = np.random.RandomState(5)
    worst = orth = 0.0
    for k in range(400):
        w = rs.normal(size=3)
        w = w / np.linalg.norm(w) * (k / 399.0) * ref.MAX_THETA
        if (w * w).sum() > 1.0:
            w = w * (1 - 1e-15)
        E = ref.exp_rotation(w)
        worst = max(worst, np.abs(E - bs.rotation(w)).max())
        orth = max(orth, np.abs(E @ E.T - np.eye(3)).max())
    print('exponential: worst difference', worst, 'orthogonality', orth)
    assert worst <= 2 * EXP_MEASURED
    assert orth <= 1e-14
    assert np.array_equal(ref.exp_rotation(np.zeros(3)), np.eye(3))
    assert ref.exp_rotation(np.array([0.8, 0.5, 0.4])) is None                   # beyond the bound


def _dense(bl, lam, floor):
    """the damped normal matrix of the restatement's A and B, points eliminated with np.linalg -> (S over all 6 V, b)"""
    A, B, r = bl.lin.A, bl.lin.B, bl.lin.r
    V, P = len(bl.pose), len(bl.xyz)
    owner = np.repeat(np.arange(P), np.diff(bl.off))
    J = np.zeros((2 * len(owner), 6 * V + 3 * P))
    for o in range(len(owner)):
        J[2 * o:2 * o + 2, 6 * bl.view[o]:6 * bl.view[o] + 6] = A[o]
        J[2 * o:2 * o + 2, 6 * V + 3 * owner[o]:6 * V + 3 * owner[o] + 3] = B[o]
    H, g = J.T @ J, J.T @ r.reshape(-1)
    d = np.diag(H).copy()
    H[np.diag_indices_from(H)] = d + lam * np.maximum(d, floor)
    n = 6 * V
    Hpp_inv = np.linalg.inv(H[n:, n:])
    return H[:n, :n] - H[:n, n:] @ Hpp_inv @ H[n:, :n], -g[:n] + H[:n, n:] @ Hpp_inv @ g[n:]


def test_schur_product_and_solver_against_dense_algebra():
    s = bs.make_scene(views=3, n_points=7, seed=4, fixed=(0,), skew=0.5)
    assert len(s.xyz) == 7
    lam = 1e-3
    bl = ref.normal_blocks(s.cams, s.xyz, s.off, s.view, s.obs, fixed_views=(0,), lam=lam)
    S, b = _dense(bl, lam, ref.FLOOR)
    free = np.repeat(bl.moves, 6)
    assert list(bl.moves) == [False, True, True]
    assert _rel(bl.b.reshape(-1)[free], b[free]) <= 1e-10
    rs = np.random.RandomState(0)
    for _ in range(3):
        x = rs.normal(size=(3, 6)) * bl.moves[:, None]
        assert _rel(ref.schur_apply(bl, x).reshape(-1)[free], (S @ x.reshape(-1))[free]) <= 1e-10
    x, n = ref.solve_reduced(bl, cg_iters=200, cg_tol=1e-12)
    assert 0 < n < 200
    assert _rel(x.reshape(-1)[free], np.linalg.solve(S[np.ix_(free, free)], b[free])) <= 1e-8
    assert not x[0].any()


def test_truth_noise_free_four_views():
    s = bs.make_scene(noise=0.0, seed=0)
    res = ref.bundle_adjust(s.cams, s.xyz, s.off, s.view, s.obs, fixed_views=(0, 1), iterations=15)
    ec, ep = np.abs(bs.centres(res.cams) - bs.centres(s.cams_true)).max(), np.abs(res.xyz - s.xyz_true).max()
    print('noise-free: centres', ec, 'points', ep, 'cost', res.cost)
    assert ec <= TRUTH_BOUND and ep <= TRUTH_BOUND


def test_truth_noisy_four_views():
    s = bs.make_scene(noise=0.3, seed=0)
    res = ref.bundle_adjust(s.cams, s.xyz, s.off, s.view, s.obs, fixed_views=(0, 1), iterations=10)
    at_truth = bs.cost_of(ref, s.cams_true, s.xyz_true, s)
    print('noisy: cost', res.cost0, '->', res.cost, 'at truth', at_truth)
    assert res.cost <= at_truth
    e0 = np.linalg.norm(bs.centres(s.cams) - bs.centres(s.cams_true), axis=1)
    e1 = np.linalg.norm(bs.centres(res.cams) - bs.centres(s.cams_true), axis=1)
    assert (e1[2:] < e0[2:]).all()
    assert np.array_equal(res.cams[:2], s.cams[:2])                              # the fixed cameras, bit for bit
    assert np.array_equal(res.cams[:, 1], s.cams[:, 1])


def test_one_fixed_view_eight_views():
    s = bs.make_scene(views=8, n_points=300, seed=1, fixed=(0,))
    res = ref.bundle_adjust(s.cams, s.xyz, s.off, s.view, s.obs, fixed_views=(0,), iterations=10)
    assert res.accepted >= 3 and len(res.costs) == res.accepted + 1
    assert all(b < a for a, b in zip(res.costs, res.costs[1:]))
    assert res.cost < bs.cost_of(ref, s.cams_true, s.xyz_true, s)


def test_huber_against_outliers():
    s = bs.make_scene(noise=0.3, seed=0)
    rs = np.random.RandomState(11)
    obs = s.obs.copy()
    hit = rs.permutation(len(obs))[:len(obs) // 10]
    ang = rs.uniform(0, 2 * np.pi, len(hit))
    obs[hit] += 20.0 * np.stack([np.cos(ang), np.sin(ang)], 1)
    run = lambda d: ref.bundle_adjust(s.cams, s.xyz, s.off, s.view, obs, fixed_views=(0, 1), iterations=15, loss_scale=d)    # noqa: E731
    plain, huber, inf = run(None), run(1.0), run(np.inf)
    err = lambda r: np.linalg.norm(bs.centres(r.cams) - bs.centres(s.cams_true), axis=1)[2:]                               # noqa: E731
    print('centre errors: plain', err(plain), 'huber', err(huber))
    assert (err(huber) < err(plain)).all()
    assert np.array_equal(plain.cams, inf.cams) and np.array_equal(plain.xyz, inf.xyz) and plain.cost == inf.cost and plain.lam == inf.lam


def test_edges_unobserved_view_short_track_all_fixed():
    s = bs.make_scene(seed=0)
    # a fifth view nobody observes, and a point with a single observation
    cams = np.concatenate([s.cams, s.cams[3:4]])
    xyz = np.concatenate([s.xyz, [[0.1, 0.2, -4.0]]])
    off = np.concatenate([s.off, [s.off[-1] + 1]])
    view = np.concatenate([s.view, [2]]).astype(np.int32)
    obs = np.concatenate([s.obs, [[50.0, 60.0]]])
    res = ref.bundle_adjust(cams, xyz, off, view, obs, fixed_views=(0, 1), iterations=6)
    assert np.array_equal(res.cams[4], cams[4]) and np.array_equal(res.xyz[-1], xyz[-1])
    assert np.isfinite(res.cams).all() and np.isfinite(res.xyz).all() and np.isfinite(res.residuals).all() and np.isfinite(res.cost)
    assert not res.residuals[-1].any()
    assert res.cost < res.cost0
    fixed = ref.bundle_adjust(s.cams, s.xyz, s.off, s.view, s.obs, fixed_views=np.ones(4, bool), iterations=4)
    assert np.array_equal(fixed.cams, s.cams) and not np.array_equal(fixed.xyz, s.xyz) and fixed.cost < fixed.cost0


def test_edges_behind_a_camera():
    s = bs.make_scene(seed=0)
    xyz = s.xyz.copy()
    xyz[5] = bs.centres(s.cams)[s.view[s.off[5]]] - (xyz[5] - bs.centres(s.cams)[s.view[s.off[5]]])     # mirrored through its first camera
    with pytest.raises(ValueError):
        ref.bundle_adjust(s.cams, xyz, s.off, s.view, s.obs, fixed_views=(0, 1), iterations=1)
    with pytest.raises(ValueError):
        ref.residuals(s.cams, xyz, s.off, s.view, s.obs)
    r, terms, cost = ref.residuals(s.cams, xyz, s.off, s.view, s.obs, trial=True)
    assert cost == np.inf and np.isinf(terms[s.off[5]]) and not r[s.off[5]].any()
    # a trial step that lands behind is rejected: a step so long that points cross their cameras
    bl = ref.normal_blocks(s.cams, s.xyz, s.off, s.view, s.obs, fixed_views=(0, 1), lam=1e-4)
    x = np.zeros((4, 6))
    x[2, 5] = x[3, 5] = -50.0
    pose, trial_xyz, ok = ref.apply_step(bl, x)
    trial = ref.residuals(ref.cams_with(s.cams, pose), trial_xyz, s.off, s.view, s.obs, trial=True)[2]
    assert ok and trial == np.inf and not ref.accepts(1e300, trial, ok)
    assert ref.accepts(2.0, 1.0, True) and not ref.accepts(1.0, 1.0, True) and not ref.accepts(2.0, 1.0, False) and not ref.accepts(2.0, np.nan, True)


def test_observation_helpers():
    """`observations` gathers the keypoint positions under the tracks' entries; `model_problem` reads the same problem out of a model dict"""
    from mvsdf_amd import keypoints
    from mvsdf_amd.datasets.colmap import _points
    from colmap_scene import quaternion
    s = bs.make_scene(seed=0)
    V, rs = 4, np.random.RandomState(2)
    count = np.bincount(s.view, minlength=V)
    view_off = np.concatenate([[0], np.cumsum(count + 3)]).astype(np.int64)           # three keypoints per view belong to no track
    xy, kp_of = rs.uniform(0, 100, size=(view_off[-1], 2)), np.zeros(len(s.view), np.int32)
    for v in range(V):
        slots = rs.permutation(count[v] + 3)[:count[v]]
        kp_of[s.view == v] = slots
        xy[view_off[v] + slots] = s.obs[s.view == v]
    kp = keypoints.make_keypoints(xy, np.zeros((len(xy), 128), np.int8), view_off)
    got = bundle.observations(kp, (s.off, s.view, kp_of))
    assert got.dtype == torch.float64 and np.array_equal(got.numpy(), s.obs)
    ids = [3, 5, 7, 9]
    model = {'cameras': {1: {'model': 'PINHOLE', 'width': 192, 'height': 128, 'params': np.array([300.0, 300.0, 96.0, 64.0])}},
             'images': {i: {'q': quaternion(s.cams[v, 0, :3, :3]), 't': s.cams[v, 0, :3, 3].copy(), 'camera_id': 1, 'name': '%d.png' % v,
                            'xys': np.zeros((0, 2)), 'point3D_ids': np.zeros(0, np.int64)} for v, i in enumerate(ids)},
             'points': _points([], [], [], [], [0], [], [])}
    full = keypoints.assemble_model(model, ids, xy, view_off, s.xyz, np.zeros((len(s.xyz), 3), np.uint8), np.zeros(len(s.xyz)), s.off, s.view, kp_of)
    mids, cams, xyz, off, view, obs = bundle.model_problem(full)
    assert mids == ids and np.array_equal(xyz, s.xyz) and np.array_equal(off, s.off) and np.array_equal(view, s.view) and np.array_equal(obs, s.obs)
    assert cams.shape == (4, 2, 4, 4) and np.abs(cams[:, 0, :3] - s.cams[:, 0, :3]).max() < 1e-12
