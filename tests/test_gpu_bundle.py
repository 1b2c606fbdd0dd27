"""mvsdf_amd/bundle.py on the GPU against its numpy restatement (tests/bundle_ref.py): every stage alone and the composed adjustment, every fp64
result entry for entry with torch.equal (equality of numbers: the definition leaves the sign of a zero open), counts and header words as integers,
costs and lambda as the same fp64 values."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bundle_ref as R  # noqa: E402
import bundle_scene as BS  # noqa: E402
from mvsdf_amd import bundle as BA  # noqa: E402
from mvsdf_amd._lib import K  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = {(2, 1): 0, (3, 7): 4, (4, 120): 0, (8, 300): 1}                        # (views, points) -> the scene's seed


def eq(got, want):
    got = got.cpu() if isinstance(got, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(got))
    want = want.cpu() if isinstance(want, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(want))
    return got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want)


def scene_of(V, P, outliers=False, **kw):
    """tracks of 2 .. V views in shuffled order, skewed K with fx != fy; outliers: every ninth observation moved by 20 pixels"""
    s = BS.make_scene(views=V, n_points=P, seed=CASES.get((V, P), 0), skew=0.7, shuffle=True, **dict(dict(fixed=(0,)), **kw))
    if outliers:
        obs = s.obs.copy()
        obs[::9] += [12.0, -16.0]
        s = s._replace(obs=obs)
    return s


def args(s):
    return s.cams, s.xyz, s.off, s.view, s.obs


_STAGES = {}


def stages(V, P, huber):
    """the restatement's stages of one case, computed once"""
    key = (V, P, huber)
    if key not in _STAGES:
        s = scene_of(V, P, outliers=huber is not None)
        bl = R.normal_blocks(*args(s), fixed_views=(0,), lam=1e-3, loss_scale=huber)
        x, n = R.solve_reduced(bl, 64, 1e-8)
        _STAGES[key] = (s, R.residuals(*args(s), loss_scale=huber), bl, x, n, R.apply_step(bl, x))
    return _STAGES[key]


@pytest.mark.parametrize('huber', [None, 1.0])
@pytest.mark.parametrize('V,P', list(CASES))
def test_every_stage_equals_the_restatement(V, P, huber):
    s, (r, terms, cost), bl, x, n, (pose, xyz, ok) = stages(V, P, huber)
    assert len(s.xyz) == P and set(np.diff(s.off)) <= set(range(2, V + 1))
    got = BA.residuals(*args(s), loss_scale=huber)
    assert eq(got[0], r) and eq(got[1], terms) and got[2] == cost
    g = BA.normal_blocks(*args(s), fixed_views=(0,), lam=1e-3, loss_scale=huber)
    assert eq(g.U, bl.U) and eq(g.gc, bl.gc) and eq(g.V, bl.V) and eq(g.gp, bl.gp) and eq(g.b, bl.b)
    probe = np.random.RandomState(V * P).normal(size=(V, 6))
    assert eq(BA.schur_apply(g, probe), R.schur_apply(bl, probe))
    gx, gn = BA.solve_reduced(g, 64, 1e-8)
    assert gn == n and eq(gx, x) and (V == 2 or 0 < n < 64)
    gc, gxyz, gok = BA.apply_step(g, x)
    assert gok == ok and eq(gc, R.cams_with(s.cams, pose)) and eq(gxyz, xyz)
    assert eq(BA.schur_apply(g, probe), R.schur_apply(bl, probe))                # the blocks outlive the calls made on them


def _tree_case(n):
    """3 views, 2100 points seen by views 0 and 1; the first n also by view 2 (n = 0: a view nobody observes)"""
    s = BS.make_scene(views=3, n_points=40, seed=3, fixed=(0,))
    rs = np.random.RandomState(n + 1)
    P = 2100
    xyz = s.xyz_true[rs.randint(0, len(s.xyz_true), P)] + rs.normal(scale=0.05, size=(P, 3))
    view, off = [], [0]
    for j in range(P):
        view += [0, 1, 2] if j < n else [1, 0]
        off.append(len(view))
    view, off = np.asarray(view, np.int32), np.asarray(off, np.int64)
    owner = np.repeat(np.arange(P), np.diff(off))
    obs = np.zeros((len(view), 2))
    for v in range(3):
        m = view == v
        obs[m] = BS.project(s.cams_true[v], xyz[owner[m]])[0]
    return s.cams, xyz + rs.normal(scale=0.01, size=xyz.shape), off, view, obs + rs.normal(scale=0.3, size=obs.shape)


@pytest.mark.parametrize('n', [0, 1, 2, 2047, 2048, 2049])
def test_view_sums_at_the_tree_chunk_boundary(n):
    """the per-view tree reduces chunks of 2048: one observation more or less must not change a bit elsewhere, and the cost's tree spans chunks"""
    a = _tree_case(n)
    assert int((a[3] == 2).sum()) == n and len(a[3]) > 2 * 2048
    bl = R.normal_blocks(*a, fixed_views=(0,), lam=1e-4)
    g = BA.normal_blocks(*a, fixed_views=(0,), lam=1e-4)
    assert eq(g.U, bl.U) and eq(g.gc, bl.gc) and eq(g.b, bl.b) and eq(g.V, bl.V)
    x = np.random.RandomState(n).normal(size=(3, 6))
    assert eq(BA.schur_apply(g, x), R.schur_apply(bl, x))
    assert BA.residuals(*a)[2] == R.residuals(*a)[2]
    if n == 0:
        assert not bl.U[2].any() and bl.moves[2] and not bl.b[2].any()


@pytest.mark.parametrize('cg_iters', [0, 1, 2, 64])
def test_solver_state_and_frozen_launches(cg_iters):
    """fewer iterations than convergence needs, and many more: the launches after "done" must leave x alone"""
    s, _, bl, _, full, _ = stages(4, 120, None)
    x, n = R.solve_reduced(bl, cg_iters, 1e-8)
    assert n == min(cg_iters, full) and full < 64
    g = BA.normal_blocks(*args(s), fixed_views=(0,), lam=1e-3)
    gx, gn = BA.solve_reduced(g, cg_iters, 1e-8)
    assert gn == n and eq(gx, x)
    zx, zn = BA.solve_reduced(g, 8, 1e-8, b=np.zeros((4, 6)))
    assert zn == 0 and not zx.cpu().numpy().any()
    gx, gn = BA.solve_reduced(g, cg_iters, 1e-8)                                 # the state is fresh for every solve
    assert gn == n and eq(gx, x)


def _same_result(got, want):
    assert eq(got.cams, want.cams) and eq(got.xyz, want.xyz) and eq(got.residuals, want.residuals)
    assert (got.cost0, got.cost, got.lam) == (want.cost0, want.cost, want.lam)
    assert (got.iterations, got.accepted, got.cg_iterations) == (want.iterations, want.accepted, want.cg_iterations)


COMPOSED = {'plain': dict(), 'huber': dict(loss_scale=1.0), 'converges': dict(ftol=1e-2),
            'rejects': dict(lambda0=1e-10, scene=dict(angle=20.0, shift=2.0, jitter=0.5)), 'at_the_optimum': dict(ftol=0.0)}


@pytest.mark.parametrize('case', list(COMPOSED))
def test_bundle_adjust_equals_the_restatement(case):
    kw = dict(COMPOSED[case])
    s = scene_of(4, 120, outliers=case == 'huber', fixed=(0, 1), **kw.pop('scene', {}))
    a = args(s)
    if case == 'at_the_optimum':
        first = R.bundle_adjust(*a, fixed_views=(0, 1), iterations=10, ftol=0.0)
        a = (first.cams, first.xyz) + a[2:]
    want = R.bundle_adjust(*a, fixed_views=(0, 1), iterations=6, **kw)
    if case in ('rejects', 'at_the_optimum'):
        assert 0 < want.accepted < want.iterations == 6                          # a step is rejected, lambda goes up
    if case == 'converges':
        assert want.iterations < 6                                               # the launches after convergence change nothing
    _same_result(BA.bundle_adjust(*a, fixed_views=(0, 1), iterations=6, **kw), want)


def test_launch_invariance_and_streams():
    s = scene_of(8, 300)
    one = BA.bundle_adjust(*args(s), iterations=4)
    two = BA.bundle_adjust(*args(s), iterations=4)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        three = BA.bundle_adjust(*args(s), iterations=4)
    side.synchronize()
    _same_result(two, one)
    _same_result(three, one)
    assert one.cost < one.cost0


def test_error_bits_and_refusals():
    s = scene_of(4, 120)
    bad = s.xyz.copy()
    bad[7, 1] = np.nan
    with pytest.raises(ValueError, match='NaN or infinite'):
        BA.bundle_adjust(s.cams, bad, s.off, s.view, s.obs)
    obs = s.obs.copy()
    obs[3, 0] = np.inf
    with pytest.raises(ValueError, match='NaN or infinite'):
        BA.residuals(s.cams, s.xyz, s.off, s.view, obs)
    view = s.view.copy()
    view[11] = 4
    with pytest.raises(ValueError, match='view index'):
        BA.bundle_adjust(s.cams, s.xyz, s.off, view, s.obs)
    view[11] = -1
    with pytest.raises(ValueError, match='view index'):
        BA.normal_blocks(s.cams, s.xyz, s.off, view, s.obs)
    off = s.off.copy()
    off[5], off[6] = off[6], off[5]
    with pytest.raises(ValueError, match='do not ascend'):
        BA.bundle_adjust(s.cams, s.xyz, off, s.view, s.obs)
    off = s.off.copy()
    off[-1] -= 1
    with pytest.raises(ValueError, match='do not ascend'):
        BA.residuals(s.cams, s.xyz, off, s.view, s.obs)
    many = np.concatenate([s.cams] * 86)[:K.MVSDF_BA_MAX_VIEWS + 1]
    with pytest.raises(ValueError, match='outside the limits'):
        BA.bundle_adjust(many, s.xyz, s.off, s.view, s.obs)
    assert BA.bundle_adjust(many[:-1], s.xyz, s.off, s.view, s.obs, iterations=1).cost0 > 0      # the limit itself is served
    with pytest.raises(ValueError, match='float64'):
        BA.bundle_adjust(s.cams.astype(np.float32), s.xyz, s.off, s.view, s.obs)
    with pytest.raises(ValueError, match='lambda_min'):
        BA.bundle_adjust(*args(s), lambda0=1e-12)
    with pytest.raises(ValueError, match='fixed_views'):
        BA.bundle_adjust(*args(s), fixed_views=(4,))


def test_behind_a_camera_is_a_value_not_a_trap():
    s = scene_of(4, 120)
    xyz = s.xyz.copy()
    c = BS.centres(s.cams)[s.view[s.off[5]]]
    xyz[5] = c - (xyz[5] - c)
    with pytest.raises(ValueError, match='behind'):
        BA.bundle_adjust(s.cams, xyz, s.off, s.view, s.obs)
    with pytest.raises(ValueError, match='behind'):
        BA.residuals(s.cams, xyz, s.off, s.view, s.obs)
    want = R.residuals(s.cams, xyz, s.off, s.view, s.obs, trial=True)
    got = BA.residuals(s.cams, xyz, s.off, s.view, s.obs, trial=True)
    assert got[2] == want[2] == np.inf and eq(got[0], want[0]) and eq(got[1], want[1])


def test_unobserved_view_short_track_and_all_fixed():
    s = scene_of(4, 120)
    cams = np.concatenate([s.cams, s.cams[3:4]])
    xyz = np.concatenate([s.xyz, [[0.1, 0.2, -4.0]]])
    off = np.concatenate([s.off, [s.off[-1] + 1]])
    view = np.concatenate([s.view, [2]]).astype(np.int32)
    obs = np.concatenate([s.obs, [[50.0, 60.0]]])
    want = R.bundle_adjust(cams, xyz, off, view, obs, fixed_views=(0, 1), iterations=4)
    got = BA.bundle_adjust(cams, xyz, off, view, obs, fixed_views=(0, 1), iterations=4)
    _same_result(got, want)
    assert eq(got.cams[4], cams[4]) and eq(got.xyz[-1], xyz[-1]) and torch.isfinite(got.xyz).all() and got.cost < got.cost0
    mask = np.ones(4, bool)
    _same_result(BA.bundle_adjust(*args(s), fixed_views=mask, iterations=3), R.bundle_adjust(*args(s), fixed_views=mask, iterations=3))


def _scene_model(cams, hw):
    """a COLMAP model dict of these cameras (image ids 3, 5, ...) without observations or points"""
    from colmap_scene import quaternion
    from mvsdf_amd.datasets.colmap import _points
    cameras = {1: {'model': 'PINHOLE', 'width': hw[1], 'height': hw[0], 'params': np.array([cams[0, 1, 0, 0], cams[0, 1, 1, 1], cams[0, 1, 0, 2], cams[0, 1, 1, 2]])}}
    images = {3 + 2 * v: {'q': quaternion(cams[v, 0, :3, :3]), 't': cams[v, 0, :3, 3].copy(), 'camera_id': 1, 'name': 'view_%d.png' % v,
                          'xys': np.zeros((0, 2)), 'point3D_ids': np.zeros(0, np.int64)} for v in range(len(cams))}
    return {'cameras': cameras, 'images': images, 'points': _points([], [], [], [], [0], [], [])}


def _tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name + '_tool', os.path.join(os.path.dirname(__file__), '..', 'tools', name + '.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_chain_from_images_through_colmap_files(tmp_path):
    """rendered images with slightly wrong cameras -> sparse_model(refine=True) -> write_colmap_text -> load_colmap_model: the same bits; the
    refinement lowers the cost; colmap_to_mvs takes the result"""
    from PIL import Image
    import keypoints_scene as S
    from colmap_scene import assert_models_equal
    from mvsdf_amd import keypoints as KP
    from mvsdf_amd.datasets.colmap import colmap_to_mvs, load_colmap_model, write_colmap_text
    cams, _ = S.make_cams(S.VIEWS, S.HW, S.FOCAL)
    images, _ = S.render(cams, S.HW, 0)
    rs = np.random.RandomState(8)
    wrong = cams.copy()
    for v in range(1, S.VIEWS):
        Rv = BS.rotation(rs.normal(size=3) * np.radians(0.1)) @ cams[v, 0, :3, :3]
        wrong[v, 0, :3, :3] = Rv
        wrong[v, 0, :3, 3] = -Rv @ (BS.centres(cams[v:v + 1])[0] + rs.normal(size=3) * 0.004)
    img_dir, posed, out = tmp_path / 'images', tmp_path / 'posed', tmp_path / 'refined'
    img_dir.mkdir()
    for v in range(S.VIEWS):
        Image.fromarray(images[v]).save(img_dir / ('view_%d.png' % v))
    write_colmap_text(_scene_model(wrong, S.HW), str(posed))
    rep = {}
    options = dict(max_epipolar=4.0, max_reproj=4.0)
    plain = KP.sparse_model(load_colmap_model(str(posed)), str(img_dir), **options)
    full = KP.sparse_model(load_colmap_model(str(posed)), str(img_dir), report=rep, refine=True, refine_options=dict(fixed_views=(0,)), **options)
    print('refine:', rep['refine'], 'points before', len(plain['points']['xyz']))
    assert rep['refine']['cost'] < rep['refine']['cost0'] and rep['refine']['accepted'] >= 1
    assert len(full['points']['xyz']) == rep['refine']['points'] >= 30
    assert np.array_equal(full['images'][3]['t'], plain['images'][3]['t']) and not np.array_equal(full['images'][5]['t'], plain['images'][5]['t'])
    assert full['points']['error'].mean() < plain['points']['error'].mean()
    write_colmap_text(full, str(out))
    assert_models_equal(load_colmap_model(str(out)), full)
    again = BA.refine_model(load_colmap_model(str(out)), iterations=2)
    assert set(again) == set(full) and np.isfinite(again['points']['xyz']).all() and again['points']['xyz'].shape == full['points']['xyz'].shape
    tool = _tool('sparse_points')
    tool.main([str(posed), str(img_dir), str(tmp_path / 'refined_tool'), '--refine', '--max_epipolar', '4', '--max_reproj', '4'])
    assert_models_equal(load_colmap_model(str(tmp_path / 'refined_tool')), full)
    done = _tool('bundle_adjust').main([str(out), str(tmp_path / 'again'), '--fixed', '0', '--iterations', '2'])
    assert_models_equal(load_colmap_model(str(tmp_path / 'again')), again)
    assert done['report']['cost'] <= done['report']['cost0'] and done['report']['observations'] == len(full['points']['track_image'])
    res = colmap_to_mvs(str(out), str(img_dir), str(tmp_path / 'mvs'), max_d=32, num_pairs=3)
    assert res['cams'].shape[0] == S.VIEWS
