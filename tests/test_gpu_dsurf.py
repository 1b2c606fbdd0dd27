"""The phase-0 depth-surface sampler (csrc/sample_kernels.hip: k_dsurf_select, k_dsurf_points) against tests/dsurf_ref.py.

SELECTION: exact.  Given the seed, which pixels are drawn and in which order is integer arithmetic; the idx of mvsdf_dsurf_select must equal
dsurf_ref's walk element for element in both sets, counts included, and ops.dsurf_samples' idx must be its sort.  The only condition is on the
INPUT: dsurf_ref.clear_band has set the depth to 0 wherever a point lies within 10 x the point tolerance of a face of the box (at most 2 % of the
valid pixels, asserted in every case), so float32 rounding cannot decide a pixel's eligibility.  No selected index is excused.  The band also covers
ops.dsurf_samples' own inputs: it inverts the camera matrices in float32 on the device while the reference holds float64 inverses rounded to float32,
which moves a point by about 1e-7 against a band of 2e-4 -- so its sorted selection is compared exactly too.

POINTS: tol = max(2e-5, 4 e32), e32 = max |points32 - points64| over the case's valid pixels (dsurf_ref.point_tolerance: from the reference's own
float32 evaluation, never from the kernel).  pts_on = points64[idx] and pts_jit = points64[idx] + (uniform * 2 jitter_rad - jitter_rad) within tol:
the jitter is checked itself -- pixel, coordinate and seed.  Measured on an MI355X (printed by every case; worst over the case's n):

    case             e32        tol      kernel: max |pts_on - ref|   max |pts_jit - ref|
    mega             1.3e-07    2e-05    4.78e-07                     5.3e-07
    mega_nojitter    1.29e-07   2e-05    4.73e-07                     4.73e-07
    mega_sparse      1.29e-07   2e-05    4.73e-07                     5.11e-07
    t1               5.16e-08   2e-05    5.16e-08                     4.09e-08
    t1023            1.84e-07   2e-05    2.88e-07                     2.77e-07
    t1023_sparse     1.14e-07   2e-05    2.13e-07                     2.44e-07
    t1024            1.18e-07   2e-05    2.03e-07                     2.57e-07
    t1025            1.18e-07   2e-05    2.04e-07                     2.82e-07
    t2049            1.17e-07   2e-05    2.01e-07                     2.71e-07
    t2049_sparse     1.05e-07   2e-05    1.81e-07                     2.03e-07
    t2304_faces      2.34e-07   2e-05    3.53e-07                     3.31e-07
    t2304_holes      1.68e-07   2e-05    3.06e-07                     3.17e-07
    t2304_nojitter   1.68e-07   2e-05    3.06e-07                     3.06e-07
    t3               7.59e-08   2e-05    1.35e-07                     1.71e-07
    t5               7e-08      2e-05    1.3e-07                      1.4e-07

(The larger of the two routes is listed: ops.dsurf_samples inverts the camera matrices in float32 on the device, the reference holds float64 inverses
rounded to float32, which adds about one float32 rounding of the inverse; mvsdf_dsurf_points on the reference's own inverses stays within 1.6 e32, the jitter included.)

The cases (dsurf_ref.CASES) are the places where the ballot / popcount compaction over sixteen waves can go wrong: fewer than 1024 pixels in all
(lanes past the end), a power of four and one past it (no cycle walking / 75 % rejected), half widths 1 and 2, two full rounds of 1024 candidates and a third with one, the cut
`pos < n` inside a wave (n = 65) and between waves (n = 64), n above 1024, n equal to the eligible count and one past it, 5 % valid pixels (many
rounds), a million-pixel pool at half width 11, and counts that differ between the two sets."""
import ctypes as C

import numpy as np
import pytest
import torch

import dsurf_ref as R
from helpers import t
from mvsdf_amd import ops
from mvsdf_amd._lib import lib, ptr

pytestmark = pytest.mark.gpu

_dev_cache = {}
_measured = {}


def _dev(case):
    """the case's scene on the device, uploaded once"""
    if case not in _dev_cache:
        scene = R.prepare(case)[0]
        _dev_cache[case] = {k: t(v.copy()) for k, v in scene.items()}         # (the prepared arrays are read-only)
    return _dev_cache[case]


def _geo(dv, bb, jr, seed, n):
    N, H, W = dv['depths'].shape
    return (ptr(dv['depths']), ptr(dv['kinv']), ptr(dv['einv']), N, H, W, ptr(dv['size']), ptr(dv['center']), C.c_float(bb), C.c_float(jr),
            C.c_ulonglong(seed), n)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _select(dv, bb, jr, seed, n):
    """mvsdf_dsurf_select directly: the unsorted walk order, idx prefilled like ops.dsurf_samples does -> (rc, idx [2,n], counts [2]).  Both outputs are
    followed by slack that must stay as it was: a rank one past the end of set 1 would land there."""
    idx = torch.full((2 * n + 64,), R.FILL, dtype=torch.int64, device='cuda')
    counts = torch.full((2 + 64,), -7, dtype=torch.int64, device='cuda')
    rc = lib().mvsdf_dsurf_select(*_geo(dv, bb, jr, seed, n), ptr(idx), ptr(counts), _stream())
    idx, counts = idx.cpu().numpy(), counts.cpu().numpy()
    assert (idx[2 * n:] == R.FILL).all() and (counts[2:] == -7).all(), 'mvsdf_dsurf_select wrote past the end of an output'
    return rc, idx[:2 * n].reshape(2, n), counts[:2]


def _points(dv, bb, jr, seed, n, idx, counts):
    """mvsdf_dsurf_points directly, outputs prefilled with NaN -> (rc, pts_on, pts_jit)"""
    on = torch.full((n, 3), float('nan'), device='cuda')
    jit = torch.full((n, 3), float('nan'), device='cuda')
    rc = lib().mvsdf_dsurf_points(*_geo(dv, bb, jr, seed, n), ptr(idx), ptr(counts), ptr(on), ptr(jit), _stream())
    return rc, on.cpu().numpy(), jit.cpu().numpy()


_walk_cache = {}


def _first_n(case, s, n):
    """dsurf_ref.first_n of the case's set s; a set is a prefix of the walk's eligible pixels, so a longer walk already made serves a shorter one"""
    elig, seed = R.prepare(case)[4], R.CASES[case][3]
    c = _walk_cache.get((case, s))
    if c is None or not (c[2] >= n or c[1] < c[2]):                                 # nothing yet, or a shorter walk that did not run out of pixels
        c = _walk_cache[case, s] = R.first_n(elig[s], seed, s, n) + (n,)
    idx, m = np.full(n, R.FILL, np.int64), min(n, c[1])
    idx[:m] = c[0][:m]
    return idx, m


def _reference(case, n):
    cleared = R.prepare(case)[3]
    assert cleared <= 0.02, cleared                                                 # the one condition on the input
    r = [_first_n(case, s, n) for s in range(2)]
    return np.stack([r[0][0], r[1][0]]), np.array([r[0][1], r[1][1]], np.int64)


def _ref_points(case, idx_sorted, counts):
    """what the two point arrays must hold for sorted indices: points64 (+ the exact jitter for set 1), zero rows past the counts"""
    _, _, _, _, _, p64 = R.prepare(case)
    _, bb, jr, seed, _ = R.CASES[case]
    n = idx_sorted.shape[1]
    on, jit = np.zeros((n, 3)), np.zeros((n, 3))
    i0, i1 = idx_sorted[0, :counts[0]], idx_sorted[1, :counts[1]]
    on[:counts[0]] = p64[i0]
    jit[:counts[1]] = p64[i1] + R.jitter64(seed, i1, jr)
    return on, jit


def _check_points(case, what, on, jit, idx_sorted, counts):
    tol, e32 = R.prepare(case)[1:3]
    ref_on, ref_jit = _ref_points(case, idx_sorted, counts)
    d_on, d_jit = float(np.abs(on - ref_on).max()), float(np.abs(jit - ref_jit).max())
    m = _measured.setdefault(case, [0.0, 0.0])
    m[0], m[1] = max(m[0], d_on), max(m[1], d_jit)
    print('%-16s %-8s n %-6d e32 %.3g  tol %.3g  max |pts_on - ref| %.3g  max |pts_jit - ref| %.3g  (case so far: %.3g %.3g)'
          % (case, what, idx_sorted.shape[1], e32, tol, d_on, d_jit, m[0], m[1]))
    assert d_on <= tol and d_jit <= tol, (d_on, d_jit, tol)
    assert not on[counts[0]:].any() and not jit[counts[1]:].any()                   # the rows past the counts are zero, not merely small
    assert not np.signbit(on[counts[0]:]).any() and not np.signbit(jit[counts[1]:]).any()


CASE_N = [(case, n) for case in sorted(R.CASES) for n in R.case_ns(case)]


@pytest.mark.parametrize('case,n', CASE_N, ids=['%s-%s' % cn for cn in CASE_N])
def test_selection_is_exact_and_points_match(case, n):
    scene, tol, e32, cleared, elig, p64 = R.prepare(case)
    _, bb, jr, seed, _ = R.CASES[case]
    sym, n = n, R.resolve_n(n, elig)
    ref_idx, ref_counts = _reference(case, n)
    e = [int(elig[0].sum()), int(elig[1].sum())]
    assert ref_counts.tolist() == [min(n, e[0]), min(n, e[1])]
    if sym == 'all':
        assert ref_counts[0] == n == e[0]
    if sym == 'all+1':
        assert ref_counts[0] == n - 1                                               # the shortfall is there, the case is not vacuous
    if sym == 'min+1':
        assert ref_counts.min() == n - 1 and ref_counts[0] != ref_counts[1]
    dv = _dev(case)
    rc, idx, counts = _select(dv, bb, jr, seed, n)
    assert rc == 0
    assert np.array_equal(counts, ref_counts), (counts, ref_counts)
    assert np.array_equal(idx, ref_idx), 'first differing position per set: %s' % [int(np.argmax(idx[s] != ref_idx[s])) for s in range(2)]
    for s in range(2):
        assert (idx[s, counts[s]:] == R.FILL).all()                                 # the tail keeps the caller's fill value
    # ops.dsurf_samples: the same selection sorted, and the points of the sorted pixels
    on, jit, c2, idx_sorted = ops.dsurf_samples(dv['depths'], dv['depth_cams'], dv['size'], dv['center'], bb, jr, seed, n)
    idx_sorted = idx_sorted.cpu().numpy()
    assert c2.tolist() == ref_counts.tolist()
    assert np.array_equal(idx_sorted, np.sort(ref_idx, axis=1))
    assert on.shape == (n, 3) and jit.shape == (n, 3) and on.dtype == torch.float32
    _check_points(case, 'ops', on.cpu().numpy().astype(np.float64), jit.cpu().numpy().astype(np.float64), idx_sorted, ref_counts)
    # mvsdf_dsurf_points on the very inverses the reference was given
    rc, on2, jit2 = _points(dv, bb, jr, seed, n, t(idx_sorted), t(ref_counts))
    assert rc == 0
    _check_points(case, 'direct', on2.astype(np.float64), jit2.astype(np.float64), idx_sorted, ref_counts)
    if jr == 0.0:                                                                   # no jitter: the "jittered" points are the on-surface points of the same pixels
        both = np.stack([idx_sorted[1], idx_sorted[1]])
        rc, a, b = _points(dv, bb, jr, seed, n, t(both), t(np.array([ref_counts[1]] * 2, np.int64)))
        assert rc == 0 and np.array_equal(a, b)


def test_the_two_sets_differ_near_the_faces():
    """bb = 1 on a scene with surface near the faces: the two sets hold different numbers of eligible pixels, counts say so when n exceeds the smaller
    one, and set 1 is decided by THIS seed's jitter: it holds pixels whose on-surface point is in the box and which another seed's jitter pushes out."""
    case = 't2304_faces'
    scene, tol, e32, cleared, elig, p64 = R.prepare(case)
    _, bb, jr, seed, _ = R.CASES[case]
    e0, e1 = int(elig[0].sum()), int(elig[1].sum())
    assert e0 != e1
    n = min(e0, e1) + 1
    ref_idx, ref_counts = _reference(case, n)
    assert ref_counts[0] != ref_counts[1]
    rc, idx, counts = _select(_dev(case), bb, jr, seed, n)
    assert rc == 0 and np.array_equal(counts, ref_counts) and np.array_equal(idx, ref_idx)
    other = seed + 1
    q_other = p64 + R.jitter64(other, np.arange(p64.shape[0]), jr)
    out_other = ~(np.abs(q_other) < bb).all(-1)
    sel1 = ref_idx[1, :ref_counts[1]]
    witness = elig[0][sel1] & out_other[sel1] & (np.abs(np.abs(q_other[sel1]) - bb).min(-1) > 10 * tol)
    assert witness.sum() >= 3, 'the scene no longer has pixels that one seed keeps and another pushes out'
    # under the other seed those pixels are not drawn into set 1 (their point there is outside by more than the band)
    rc, idx_o, counts_o = _select(_dev(case), bb, jr, other, n)
    assert rc == 0 and not np.isin(sel1[witness], idx_o[1, :counts_o[1]]).any()
    # and set 1 holds pixels whose on-surface point is OUTSIDE the box (the jitter pulled them in): set 1 is not a subset of set 0's pool
    assert (~elig[0][sel1]).any()


@pytest.mark.parametrize('name', ['t1023', 't2049', 't5'])
def test_no_valid_pixel(name):
    scene = R.make_scene(*R.SCENES[name])
    scene['depths'][:] = 0.0
    scene['depths'].reshape(-1)[::7] = -1.0                                         # a negative depth is no depth either (depth > 0)
    dv = {k: t(v) for k, v in scene.items()}
    for n in (1, 65):
        rc, idx, counts = _select(dv, R.BIG_BB, 0.1, 3, n)
        assert rc == 0 and counts.tolist() == [0, 0] and (idx == R.FILL).all()
        on, jit, c2, idx_sorted = ops.dsurf_samples(dv['depths'], dv['depth_cams'], dv['size'], dv['center'], R.BIG_BB, 0.1, 3, n)
        assert c2.tolist() == [0, 0] and not on.any() and not jit.any() and (idx_sorted == R.FILL).all()


def test_points_kernel_guards():
    """An index list with -1 and N H W inside the counted prefix (and a good index past the count): those rows come out zero, every other row is what
    the clean list gives, and no error is raised."""
    case = 't2304_holes'
    scene, tol, e32, cleared, elig, p64 = R.prepare(case)
    _, bb, jr, seed, _ = R.CASES[case]
    dv, n = _dev(case), 200
    total = p64.shape[0]
    ref_idx, ref_counts = _reference(case, n)
    clean = np.sort(ref_idx, axis=1)
    counts = np.array([n, n - 10], np.int64)
    rc, on0, jit0 = _points(dv, bb, jr, seed, n, t(clean), t(counts))
    assert rc == 0
    bad = clean.copy()
    bad[0, [0, 63, 64, 199]] = [-1, total, 1 << 40, -(1 << 33)]
    bad[1, [1, 100, 189]] = [total, -1, R.FILL]
    rc, on1, jit1 = _points(dv, bb, jr, seed, n, t(bad), t(counts))
    assert rc == 0
    torch.cuda.synchronize()
    exp_on, exp_jit = on0.copy(), jit0.copy()
    exp_on[[0, 63, 64, 199]] = 0.0
    exp_jit[[1, 100, 189]] = 0.0
    assert np.array_equal(on1, exp_on) and np.array_equal(jit1, exp_jit)
    assert not jit0[n - 10:].any() and np.abs(jit0[:n - 10]).max() > 0               # rows past the count: zero although their index is a good pixel
    _check_points(case, 'guards', on0.astype(np.float64), jit0.astype(np.float64), clean, counts)


def test_refusals_then_a_valid_call():
    case = 't1025'
    scene, tol, e32, cleared, elig, p64 = R.prepare(case)
    _, bb, jr, seed, _ = R.CASES[case]
    dv, n = _dev(case), 65
    L = lib()
    idx = torch.full((2, n), R.FILL, dtype=torch.int64, device='cuda')
    counts = torch.full((2,), -7, dtype=torch.int64, device='cuda')
    on, jit = torch.full((n, 3), 7.0, device='cuda'), torch.full((n, 3), 7.0, device='cuda')
    good = list(_geo(dv, bb, jr, seed, n))

    def refused(fn, args, name):
        rc = fn(*args, _stream())
        assert rc != 0, name
        assert name in L.mvsdf_last_error().decode(), L.mvsdf_last_error().decode()

    sel_tail, pts_tail = [ptr(idx), ptr(counts)], [ptr(idx), ptr(counts), ptr(on), ptr(jit)]
    for fn, tail, name in ((L.mvsdf_dsurf_select, sel_tail, 'mvsdf_dsurf_select'), (L.mvsdf_dsurf_points, pts_tail, 'mvsdf_dsurf_points')):
        refused(fn, good[:11] + [0] + tail, name)                                   # n = 0
        refused(fn, good[:11] + [-3] + tail, name)
        for N, H, W in ((1, 32768, 32768), (4, 16384, 16384), (1 << 10, 1 << 10, 1 << 11), (0, 25, 41), (1, -25, 41)):   # N H W >= 2^30 (sizes only: refused before
            refused(fn, good[:3] + [N, H, W] + good[6:] + tail, name)                                                    # any launch), or not positive
        for i in (0, 1, 2, 6, 7):                                                   # a null input pointer
            refused(fn, good[:i] + [None] + good[i + 1:] + tail, name)
        for i in range(len(tail)):                                                  # a null output pointer
            refused(fn, good + tail[:i] + [None] + tail[i + 1:], name)
    torch.cuda.synchronize()
    assert (idx == R.FILL).all() and (counts == -7).all() and (on == 7.0).all() and (jit == 7.0).all()   # nothing was launched
    ref_idx, ref_counts = _reference(case, n)
    rc, got, c = _select(dv, bb, jr, seed, n)
    assert rc == 0 and np.array_equal(got, ref_idx) and np.array_equal(c, ref_counts)


def test_reproducible_and_seed_dependent():
    case = 'mega_sparse'
    scene, tol, e32, cleared, elig, p64 = R.prepare(case)
    _, bb, jr, seed, _ = R.CASES[case]
    dv, n = _dev(case), 1500
    a = ops.dsurf_samples(dv['depths'], dv['depth_cams'], dv['size'], dv['center'], bb, jr, seed, n)
    b = ops.dsurf_samples(dv['depths'], dv['depth_cams'], dv['size'], dv['center'], bb, jr, seed, n)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    c = ops.dsurf_samples(dv['depths'], dv['depth_cams'], dv['size'], dv['center'], bb, jr, seed + 1, n)
    d = ops.dsurf_samples(dv['depths'], dv['depth_cams'], dv['size'], dv['center'], bb, jr, seed + (1 << 32), n)
    for o in (c, d):                                                                # the low and the high half of the seed both matter
        assert not torch.equal(o[3][0], a[3][0]) and not torch.equal(o[3][1], a[3][1])
        assert np.intersect1d(o[3][0].cpu().numpy(), a[3][0].cpu().numpy()).size < n // 4     # 1500 of ~40000: two independent draws share about 55
    r1 = _select(dv, bb, jr, seed, n)
    r2 = _select(dv, bb, jr, seed, n)
    assert np.array_equal(r1[1], r2[1]) and np.array_equal(r1[2], r2[2])


# ---- the model's error path (idr.py:244: np.random.choice raises when the depth maps hold fewer eligible pixels than the step draws)
def _phase0_model_and_input():
    from conftest import golden
    from mvsdf_amd.model.implicit_differentiable_renderer import IDRNetwork
    from mvsdf_amd.utils import synth
    from mvsdf_amd.utils.config import ConfigDict
    g = golden('idr_w64_phase0')
    W, B, P, V, seed, tp = int(g['W']), int(g['B']), int(g['P']), int(g['V']), int(g['seed']), float(g['tp'])
    m = IDRNetwork(ConfigDict(synth.model_conf(W)))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(W, seed).items()})
    inp, gt = synth.make_batch(B, P, V, seed=seed, size=float(g['scene_size']), center=tuple(g['scene_center']),
                               feat_hw=tuple(int(v) for v in g['feat_hw']), focal_scale=float(g['focal_scale']))
    inp['depths'] = gt['depths'] = synth.make_depth_maps(inp['depth_cams'], float(g['scene_size']), tuple(g['scene_center']), seed=seed, hole_frac=0.05)
    return m.cuda().train(), inp, gt, tp, B, P


@pytest.mark.parametrize('native', [False, True], ids=['python_route', 'native_step'])
def test_model_raises_like_np_random_choice_when_the_depth_maps_are_too_sparse(native):
    from mvsdf_amd.model.loss import IDRLoss
    m, inp, gt, tp, B, P = _phase0_model_and_input()
    m.native_step = native                                                          # the switch test_gpu_native_step.py selects the route with
    drawn = []
    inner = m._dsurf_samples

    def recording(input, n_dsurf_points, bb):
        r = inner(input, n_dsurf_points, bb)
        drawn.append((n_dsurf_points, r[0].clone(), r[1].clone(), r[2].clone()))
        return r
    m._dsurf_samples = recording
    few = np.zeros_like(inp['depths'])
    flat, src = few.reshape(-1), inp['depths'].reshape(-1)
    keep = np.nonzero(src > 0)[0][[10, 500, 900, 2000, 3000]]
    flat[keep] = src[keep]
    sparse = dict(inp, depths=few)
    torch.manual_seed(5)
    with pytest.raises(ValueError, match='Cannot take a larger sample than population'):
        m({k: t(v) for k, v in sparse.items()}, tp)
    n_ds = B * P // 2
    assert drawn[-1][0] == n_ds and max(drawn[-1][3].tolist()) <= 5 < n_ds
    assert (getattr(m, '_last_step', None) is not None) == native, 'the route asked for did not run'
    # The same model with the original depths then steps normally.  Reusing the model is deliberate: on the native route the error is raised after the step
    # was enqueued and run (materialize, behind NativeStep's run_step), so this checks that the driver's state survives the exception, not only the error.
    dev_in, dev_gt = {k: t(v) for k, v in inp.items()}, {k: t(v) for k, v in gt.items()}
    loss_fn = IDRLoss()
    loss_fn.native = native
    torch.manual_seed(5)
    out = m(dev_in, tp)
    assert drawn[-1][3].tolist() == [n_ds, n_ds]
    R_ = B * P
    assert out['eikonal_points_hom'].shape[1] == int(out['network_object_mask'].sum()) + R_ // 2 + 2 * n_ds
    lo = loss_fn(out, dict(dev_gt), tp, B)
    m.zero_grad()
    lo['loss'].backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(lo['loss']))
    gsum = sum(float(p.grad.abs().sum()) for p in m.parameters() if p.grad is not None)
    assert np.isfinite(gsum) and gsum > 0
    # under one torch.manual_seed, two forwards draw identical depth-surface samples; another seed draws others
    first = drawn[-1]
    torch.manual_seed(5)
    m(dev_in, tp)
    for a, b in zip(first[1:], drawn[-1][1:]):
        assert torch.equal(a, b)
    torch.manual_seed(6)
    m(dev_in, tp)
    assert not torch.equal(first[1], drawn[-1][1]) and not torch.equal(first[2], drawn[-1][2])
