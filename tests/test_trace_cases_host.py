"""The tracer's case table (tests/trace_cases.py) against the C oracle, on the CPU: every row does what it declares -- the lists it is there to fill are
filled, the ones it is there to leave empty are empty -- so that a later edit of the table cannot quietly empty a branch tests/test_gpu_trace_edges.py relies
on.  Conditions, not measurements: the counts the rows produced when written are comments in the table.  Also the oracle's own argument checks."""
import numpy as np
import pytest

import trace_cases as TC
from mvsdf_amd.utils import synth


def _isect(oracle, c):
    return oracle.sphere_intersection(c.cam_loc, c.ray_dirs, c.params['object_bounding_sphere'])[1].reshape(-1)


def _check_outputs(c, out):
    pts, mask, dists, rows = out
    R = c.object_mask.size
    assert pts.shape == (R, 3) and mask.shape == (R,) and dists.shape == (R,) and mask.dtype == bool
    assert np.isfinite(pts).all() and np.isfinite(dists).all()
    assert (rows >= 0).all()


def _check_declared(name, declared, counts, rows, params):
    for what, want, got in zip(('sampler', 'secant', 'min-sdf'), declared, counts):
        if want is None:
            continue
        if got is None:                                           # no secant steps: rows[2] says nothing about the list
            continue
        assert (got > 0) == want, '%s: the %s list holds %d rays' % (name, what, got)


@pytest.mark.parametrize('name', TC.ANALYTIC)
def test_analytic_rows_do_what_they_declare(oracle, name):
    c = TC.case(name)
    assert c.intervals.shape == (c.params['n_steps'],) and (c.intervals[0] == 0) == (name != TC.WRAP) and c.intervals[-1] == 1 and (np.diff(c.intervals) > 0).all()
    assert c.minsdf_steps.shape == (c.params['n_steps'],) and c.object_mask.shape == (c.ray_dirs.shape[0] * c.ray_dirs.shape[1],)
    tr, ev = TC.oracle_analytic(name, True), TC.oracle_analytic(name, False)
    _check_outputs(c, tr)
    _check_outputs(c, ev)
    assert ev[3][3] == 0 and ev[3][0] == tr[3][0] and ev[3][1] == tr[3][1]           # eval: no min-sdf rows; sphere tracing and the sampler do not depend on the mode
    counts = TC.list_counts(tr[3], c.params)
    _check_declared(name, c.lists, counts, tr[3], c.params)
    if name in TC.LONG_LISTS:
        k = ('sampler', 'secant', 'minsdf').index(TC.LONG_LISTS[name])
        assert counts[k] > 1024
        # ... with entries on both sides of the first 1024-ray chunk: more listed rays than the first chunk holds, more than the later chunks hold
        assert counts[k] > c.object_mask.size - 1024


@pytest.mark.parametrize('name', TC.FUSED)
def test_network_rows_do_what_they_declare(oracle, name):
    c = TC.case(name)
    net = oracle.Net(synth.make_state_dict(64, 0))
    for training in (True, False):
        out = oracle.trace(net, c.cam_loc, c.ray_dirs, c.object_mask, training, c.minsdf_steps, c.intervals, **c.params)
        _check_outputs(c, out)
        if training:
            _check_declared(name, c.fused, TC.list_counts(out[3], c.params), out[3], c.params)


@pytest.mark.parametrize('W', TC.WIDE_WIDTHS)
@pytest.mark.parametrize('name', list(TC.WIDE))
def test_wide_network_rows_do_what_they_declare(oracle, name, W):
    """the per-width declarations (W = 256, W = 512): the same row fills other lists on another network"""
    c = TC.case(name)
    assert TC.declared(name, W) is not None and TC.declared(name, 64) is not None       # a row of the wide table is a row of the fused table
    net = oracle.Net(synth.make_state_dict(W, 0))
    for training in (True, False):
        out = oracle.trace(net, c.cam_loc, c.ray_dirs, c.object_mask, training, c.minsdf_steps, c.intervals, **c.params)
        _check_outputs(c, out)
        if training:
            _check_declared('%s at W = %d' % (name, W), TC.declared(name, W), TC.list_counts(out[3], c.params), out[3], c.params)


@pytest.mark.parametrize('W', (64,) + TC.WIDE_WIDTHS)
def test_rounded_weights_keep_the_declared_lists_filled(oracle, W):
    """tests/test_gpu_trace_edges.py asserts on the split engines, which run on bf16-rounded weights and have no exact CPU model, that the lists a row declares
    filled (for fp32 weights) hold rays.  On the oracle of the rounded weights that is so on every row but the ones of ROUNDED_EMPTY, which are empty there."""
    net = oracle.Net(synth.make_state_dict(W, 0), bf16='weights')
    for name in (TC.FUSED if W == 64 else TC.WIDE):
        c = TC.case(name)
        counts = TC.list_counts(oracle.trace(net, c.cam_loc, c.ray_dirs, c.object_mask, True, c.minsdf_steps, c.intervals, **c.params)[3], c.params)
        filled = [got > 0 for want, got in zip(TC.declared(name, W), counts) if want is True]
        assert not any(filled) if (W, name) in TC.ROUNDED_EMPTY else all(filled), (name, W, counts)
    assert all(k[1] in TC.FUSED for k in TC.ROUNDED_EMPTY)


def test_the_wide_table_fills_every_list_at_both_widths():
    """each of the three lists is declared filled on several rows and empty on one, at W = 256 and at W = 512; 'inside' is declared per width"""
    for k in range(len(TC.WIDE_WIDTHS)):
        for lst in range(3):
            assert sum(v[k][lst] is True for v in TC.WIDE.values()) >= 3 and any(v[k][lst] is False for v in TC.WIDE.values())
    assert TC.WIDE['inside'][0] != TC.WIDE['inside'][1]
    assert set(TC.WIDE) <= set(TC.FUSED)


def test_the_table_reaches_every_branch(oracle):
    """Over the whole table (analytic SDF, training): each of the three lists is empty in one row and filled in another, both lists of the generic route's
    compaction kernel grow past a 1024-ray chunk, rays that miss the sphere take the -(d . c) projection, a camera sits inside the sphere, and the
    parameter edges the issue names are rows."""
    seen = {(k, v): [] for k in range(3) for v in (False, True)}
    longest = [0, 0, 0]
    for name in TC.ANALYTIC:
        c = TC.case(name)
        counts = TC.list_counts(TC.oracle_analytic(name, True)[3], c.params)
        for k, n in enumerate(counts):
            if n is not None:
                seen[(k, n > 0)].append(name)
                longest[k] = max(longest[k], n)
    for key, names in seen.items():
        assert names, key
    assert longest[0] > 1024 and longest[2] > 1024
    # non-intersecting rays that are projected in training: in-mask and out-mask ones
    c = TC.case(TC.ALL_MISS)
    assert not _isect(oracle, c).any() and c.object_mask.any() and not c.object_mask.all()
    pts, mask, dists, rows = TC.oracle_analytic(TC.ALL_MISS, True)
    d, cam = c.ray_dirs.reshape(-1, 3), c.cam_loc[0]
    want = -((d[:, 0] * cam[0] + d[:, 1] * cam[1]) + d[:, 2] * cam[2])
    assert np.array_equal(dists, want) and (dists != 0).any() and not mask.any() and rows.sum() == 0
    assert np.array_equal(TC.oracle_analytic(TC.ALL_MISS, False)[2], np.zeros(7, np.float32))          # eval: no projection
    c = TC.case('r08')                                            # a mixed row: some rays miss, some of those are inside the object mask
    miss = ~_isect(oracle, c)
    assert miss.any() and not miss.all()
    # the camera inside the sphere: every ray intersects and starts at t0 = 0
    c = TC.case('inside')
    t, m = oracle.sphere_intersection(c.cam_loc, c.ray_dirs, 1.0)
    assert m.all() and (t[..., 0] == 0).all() and (np.linalg.norm(c.cam_loc, axis=1) < 1).all()
    # the negative-index wrap of the secant hand-off: rays inside the object mask whose FIRST sample is negative (both SDFs)
    c = TC.case(TC.WRAP)
    assert c.params['sphere_tracing_iters'] == 0 and c.intervals[0] > 0
    t, m = oracle.sphere_intersection(c.cam_loc, c.ray_dirs, 1.0)
    t, m = t.reshape(-1, 2), m.reshape(-1)
    z0 = t[:, 0] + c.intervals[0] * (t[:, 1] - t[:, 0])
    x0 = (np.repeat(c.cam_loc, c.ray_dirs.shape[1], axis=0) + z0[:, None] * c.ray_dirs.reshape(-1, 3)).astype(np.float32)
    for sv0 in (oracle.analytic_sdf(x0), oracle.sdf_forward(oracle.Net(synth.make_state_dict(64, 0)), x0, ncols=1)[:, 0]):
        assert (m & c.object_mask & (sv0 < 0)).sum() >= 16
    # parameter edges
    n_steps = {TC.case(n).params['n_steps'] for n in TC.NAMES}
    assert {2, 12, 13, 64, 65, 129, 512, 1024} <= n_steps
    rays = {TC.case(n).object_mask.size for n in TC.NAMES}
    assert {1, 7, 8, 9, 15, 16, 17, 1023, 1024, 2048, 2049} <= rays
    assert {TC.case(n).params['object_bounding_sphere'] for n in TC.NAMES} >= {0.8, 1.0, 2.0}
    assert any(TC.case(n).params['n_secant_steps'] == 0 for n in TC.NAMES) and any(TC.case(n).params['sphere_tracing_iters'] == 0 for n in TC.NAMES)
    assert any(TC.case(n).params['dist_clip'] == 0.05 for n in TC.NAMES)
    assert any(not TC.case(n).object_mask.any() and TC.case(n).object_mask.size > 7 for n in TC.NAMES)
    b4 = TC.case('b4')
    assert b4.ray_dirs.shape[0] == 4 and b4.ray_dirs.shape[1] % 2 == 1


def test_oracle_trace_refuses_what_the_kernels_refuse(oracle):
    """oracle.trace accepts exactly the ranges mvsdf_trace accepts (n_steps in [2, 1024], line_step_iters in [0, 30]): trace_ray keeps its per-ray sample arrays
    on the stack, sized for 1024."""
    c = TC.case('r7')

    def run(**over):
        p = dict(c.params, **over)
        n = p['n_steps']
        return oracle.trace(None, c.cam_loc, c.ray_dirs, c.object_mask, True, np.full(max(n, 1), 0.5, np.float32), np.linspace(0, 1, max(n, 2), dtype=np.float32), analytic=True, **p)
    for bad in (dict(n_steps=1), dict(n_steps=0), dict(n_steps=1025), dict(n_steps=4096), dict(line_step_iters=-1), dict(line_step_iters=31)):
        with pytest.raises(ValueError):
            run(**bad)
    for ok in (dict(n_steps=2), dict(n_steps=1024), dict(line_step_iters=0), dict(line_step_iters=30)):
        pts, mask, dists, rows = run(**ok)
        assert np.isfinite(dists).all() and (rows >= 0).all()


def test_oracle_trace_past_512_samples(oracle):
    """600 samples per ray (the sample arrays held 512 once): the sampler's values are all there -- on a ray whose samples are all positive the P_out argmin is
    the first minimum over ALL n analytic values, also where that lies past sample 512."""
    c = TC.case('default')
    n = 600
    p = dict(c.params, n_steps=n, sphere_tracing_iters=0)          # no sphere tracing: every intersecting ray is sampled between t0 and t1
    rs = np.random.RandomState(600)
    steps = rs.uniform(size=n).astype(np.float32)
    iv = np.linspace(0, 1, n, dtype=np.float32)
    pts, mask, dists, rows = oracle.trace(None, c.cam_loc, c.ray_dirs, c.object_mask, False, steps, iv, analytic=True, **p)
    t, isect = oracle.sphere_intersection(c.cam_loc, c.ray_dirs, 1.0)
    t, isect = t.reshape(-1, 2), isect.reshape(-1)
    assert rows[1] == n * isect.sum()
    d, cam = c.ray_dirs.reshape(-1, 3), np.repeat(c.cam_loc, c.ray_dirs.shape[1], axis=0)
    checked = 0
    for q in np.nonzero(isect & ~mask)[0][:40]:                    # no negative sample: dist = z at the first minimum of the n values
        z = (t[q, 0] + iv * (t[q, 1] - t[q, 0])).astype(np.float32)
        x = (cam[q][None] + z[:, None] * d[q][None]).astype(np.float32)
        sv = oracle.analytic_sdf(x)
        if (sv > 0).all():
            assert dists[q] == z[int(np.argmin(sv))]
            checked += int(np.argmin(sv) >= 512)
    assert checked > 0                                            # some of those minima lie past sample 512
