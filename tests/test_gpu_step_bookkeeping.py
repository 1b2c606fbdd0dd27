"""The bookkeeping kernels of one training step (csrc/step_kernels.hip: mvsdf_step_outputs, mvsdf_step_backward_inputs stages 0 / 1 / 2,
mvsdf_step_backward_fbar) through ops, against tests/step_ref.py (numpy, written from the reference's boolean-mask / torch.cat expressions and pinned
to float64 autograd by tests/test_step_ref.py): ALL 256 (d_mask, e_mask) pairs of the point-group switches, with and without depth-surface samples,
at N = 0, N = R, n_true = 0 and n_true = N.  Index / copy work is compared bit for bit (a cell that is a copy or ONE addition of given fp32 numbers is
exact, 0 + a and a + 0 included); SampleNetwork's scalar is held to a bound derived from its operation count.

Every buffer a kernel writes starts as NaN: the valid prefix of each output holds no NaN afterwards and the rest is still NaN (nothing is written
beyond the rows the counts select).  Nout = 1 has no column 1: surf_indicator_output does not exist for such a network (the reference's
sdf_output_full[:, 1] raises), so surf / d_si are left out there and y_eval carries one float of padding behind its last row."""
import numpy as np
import pytest
import torch

import step_ref as SR
from mvsdf_amd import ops

pytestmark = pytest.mark.gpu

CONFIGS = [(1, 0, 0), (300, 150, 0), (300, 150, 150), (1025, 512, 7), (4096, 2048, 2048)]       # (R, n_eik, n_ds)
PATTERNS = ['none', 'all', 'p30', 'p70', 'no_true', 'all_true']
U = 2.0 ** -24


@pytest.fixture
def nan_alloc(monkeypatch):
    """every CUDA float tensor torch.empty hands out (every output ops allocates) starts as NaN"""
    e0 = torch.empty

    def empty(*a, **k):
        t = e0(*a, **k)
        return t.fill_(float('nan')) if t.is_cuda and t.is_floating_point() else t
    monkeypatch.setattr(torch, 'empty', empty)


def _masks(R, pattern, rng):
    hit = {'none': np.zeros(R, bool), 'all': np.ones(R, bool), 'p30': rng.random(R) < 0.3, 'p70': rng.random(R) < 0.7}.get(pattern)
    if hit is None:
        hit = rng.random(R) < 0.5
        if R == 1:
            hit[:] = True
    true = {'no_true': np.zeros(R, bool), 'all_true': np.ones(R, bool)}.get(pattern)
    if true is None:
        true = rng.random(R) < 0.6
    return hit, true


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _partition(hit, true, R, rng):
    dirs = rng.standard_normal((R, 3)).astype(np.float32)
    perm, inv, true_rows, counts, view = ops.partition_rays(_cu(hit), None, _cu(true), _cu(dirs))
    N, n_true = int(hit.sum()), int((hit & true).sum())
    assert counts.tolist() == [N, n_true]
    assert np.array_equal(perm.cpu().numpy(), SR.sorted_rays(hit))
    return inv, true_rows, counts, view, N, n_true


def _prefix(name, got, want):
    """got: the worst-case sized output; its first rows equal `want` bit for bit, without NaN, and the remainder was never written (still NaN)"""
    got = got.cpu().numpy()
    got = got.reshape((got.shape[0],) + want.shape[1:])
    k = want.shape[0]
    assert k <= got.shape[0], name
    assert not np.isnan(got[:k]).any(), name + ': NaN inside the valid prefix'
    assert np.array_equal(got[:k], want), name
    assert np.isnan(got[k:]).all(), name + ': written beyond the valid prefix'


# ------------------------------------------------------------------------------------------------ 1. step_outputs
@pytest.mark.parametrize('Nout', [1, 2, 258])
@pytest.mark.parametrize('R,n_eik,n_ds', CONFIGS, ids=['R%d-e%d-d%d' % c for c in CONFIGS])
def test_step_outputs_every_mask_pair(R, n_eik, n_ds, Nout, nan_alloc):
    rng = np.random.default_rng(R * 7 + n_ds + Nout)
    E = n_eik + 2 * n_ds
    x = rng.standard_normal((E + R, 3)).astype(np.float32)
    y = rng.standard_normal((E + R, Nout)).astype(np.float32)
    n = rng.standard_normal((E + R, 3)).astype(np.float32)
    rgb_sorted = rng.random((R, 3)).astype(np.float32)
    y_store = torch.zeros((E + R) * Nout + 1, dtype=torch.float32, device='cuda')                # (+ 1 float: see the module docstring, Nout = 1)
    y_dev = y_store[:(E + R) * Nout].view(E + R, Nout)
    y_dev.copy_(torch.from_numpy(y))
    x_dev, n_dev, rgb_dev = _cu(x), _cu(n), _cu(rgb_sorted)
    compared = 0
    for pattern in PATTERNS:
        hit, true = _masks(R, pattern, rng)
        inv, true_rows, counts, _, N, n_true = _partition(hit, true, R, rng)
        for d_mask in range(16):
            for e_mask in range(16):
                got = ops.step_outputs(R, n_eik, n_ds, counts, x_dev, y_dev, n_dev, inv, true_rows, rgb_dev, d_mask, e_mask)
                ref = SR.outputs(hit, true, n_eik, n_ds, x, y, n, rgb_sorted, d_mask, e_mask)
                names = ('rgb_values', 'sdf_output', 'diff_pts', 'eikonal_output', 'points_hom', 'grad_theta', 'surf')
                for name, g in zip(names, got):
                    if name in ref:
                        _prefix('%s %s d%d e%d' % (name, pattern, d_mask, e_mask), g, ref[name])
                assert ref['diff_pts'].shape[0] == N and (Nout == 1 or ref['surf'].shape[0] == n_true + n_eik)
                rv = got[0].cpu().numpy()
                assert (rv[~hit] == 1.0).all() and np.array_equal(rv[hit], rgb_sorted[:N])        # exactly 1 on the rays that miss
                compared += 1
    assert compared == len(PATTERNS) * 256


# ------------------------------------------------------------------------------------------------ 2. step_backward_inputs / step_backward_fbar
def fbar_bound(xbar_parts, v, n0):
    """First-order bound on |fbar_fp32 - fbar| for fbar = -(xbar . v) / (n . v), u = 2^-24, from the operation count:
      xbar_c = (d_c + p_c) + x_c: two roundings, relative 2u on each component (first order)         -> 2u S1 / |n.v|,  S1 = sum_c |xbar_c v_c|
      xbar . v: three products, two additions (any contraction into fma only removes roundings)     -> 3u S1 / |n.v|
      n . v likewise: 3u S2 on the denominator, S2 = sum_c |n_c v_c|                                  -> 3u |xbar.v| S2 / (n.v)^2
      the division: one rounding                                                                      -> u |xbar.v| / |n.v|
    times 2 for contraction differences and the second-order terms."""
    xbar = sum(p.astype(np.float64) for p in xbar_parts)
    v, n0 = v.astype(np.float64), n0.astype(np.float64)
    num, dot = (xbar * v).sum(-1), (n0 * v).sum(-1)
    s1, s2 = np.abs(xbar * v).sum(-1), np.abs(n0 * v).sum(-1)
    with np.errstate(all='ignore'):
        return 2 * U * (5 * s1 / np.abs(dot) + 3 * np.abs(num) * s2 / dot ** 2 + np.abs(num / dot)), -num / dot


# (use_geo, din present, nrm0 >= 0, d_diff, dx, d_eo, d_gth, d_si)
VARIANTS = [(1, 1, 1, 1, 1, 1, 1, 1), (0, 1, 1, 1, 1, 1, 1, 1), (1, 1, 0, 1, 0, 1, 1, 1), (1, 0, 1, 1, 1, 1, 1, 1), (1, 1, 1, 0, 1, 0, 1, 1),
            (0, 1, 1, 0, 0, 1, 0, 1), (1, 1, 1, 1, 1, 1, 1, 0), (0, 0, 1, 1, 0, 0, 0, 0)]
BWD_CASES = [(c, 6) for c in CONFIGS] + [((300, 150, 150), 258), ((1025, 512, 7), 1), ((1025, 512, 7), 2)]


@pytest.mark.parametrize('cfg,Nout', BWD_CASES, ids=['R%d-e%d-d%d-Nout%d' % (c + (o,)) for c, o in BWD_CASES])
def test_step_backward_inputs_every_mask_pair(cfg, Nout):
    R, n_eik, n_ds = cfg
    rng = np.random.default_rng(R * 13 + n_ds + Nout)
    E = n_eik + 2 * n_ds
    n_eval = rng.standard_normal((E + R, 3)).astype(np.float32)
    n_dev = _cu(n_eval)
    ld, nrm_col, feat0 = 3 + 5 + 3 + max(Nout - 2, 0), 8, 11
    ran = 0
    for pattern in ('none', 'all', 'p50'):
        hit, true = _masks(R, pattern, rng)
        _, true_rows, _, view, N, n_true = _partition(hit, true, R, rng)
        if E + N == 0:
            continue                                                                        # no row at all: nothing to assemble (the entry point refuses Mb = 0)
        view_np, tr_np = view.cpu().numpy(), true_rows.cpu().numpy()
        f = lambda *s: rng.standard_normal(s).astype(np.float32)
        din_np, d_diff_np, dx_np = f(N, ld), f(N, 3), f(N, 3)
        for d_mask in range(16):
            for e_mask in range(16):
                sizes = (N, n_eik, n_ds, n_ds)
                nd = sum(c for g, c in enumerate(sizes) if d_mask >> g & 1)
                ne = sum(c for g, c in enumerate(sizes) if e_mask >> g & 1)
                d_eo_np, d_gth_np, d_si_np = f(nd), f(ne, 3), f(n_true + n_eik)
                for vi in ((d_mask * 16 + e_mask) % len(VARIANTS), (d_mask + 3 * e_mask + 1) % len(VARIANTS)):
                    use_geo, has_din, has_nrm, has_dd, has_dx, has_eo, has_gth, has_si = VARIANTS[vi]
                    pick = lambda a, on: a if on else None
                    din = pick(din_np, has_din and N > 0)
                    d_diff, dx = pick(d_diff_np, has_dd and N > 0), pick(dx_np, has_dx and N > 0)
                    d_eo, d_gth, d_si = pick(d_eo_np, has_eo), pick(d_gth_np, has_gth), pick(d_si_np, has_si and Nout >= 2)
                    nrm0 = nrm_col if has_nrm else -1
                    dev = lambda a: None if a is None else _cu(a)
                    common = (n_eik, n_ds, N, Nout, n_true, dev(din), feat0, nrm0, bool(use_geo))
                    ref = lambda up, **kw: SR.backward_inputs(N, n_true, n_eik, n_ds, Nout, tr_np, view_np, n_eval, din, feat0, nrm0, bool(use_geo),
                                                              *up, d_mask, e_mask, dtype=np.float32, **kw)
                    what = '%s d%d e%d variant %d' % (pattern, d_mask, e_mask, vi)
                    # stage 0: the rendering net's adjoints alone, every cell written
                    dy = torch.full((E + N, Nout), float('nan'), device='cuda')
                    dn = torch.full((E + N, 3), float('nan'), device='cuda')
                    ops.step_backward_inputs(0, *common, None, None, view, n_dev, true_rows, None, None, None, d_mask, e_mask, dy, dn)
                    dy0, dn0, _ = ref((None, None, None, None, None), with_fbar=False)
                    assert np.array_equal(dy.cpu().numpy(), dy0) and np.array_equal(dn.cpu().numpy(), dn0), 'stage 0 ' + what
                    ups = (dev(d_diff), dev(dx), view, n_dev, true_rows, dev(d_eo), dev(d_gth), dev(d_si), d_mask, e_mask)
                    dy1, dn1 = dy.clone(), dn.clone()
                    ops.step_backward_inputs(1, *common, *ups, dy1, dn1)
                    ops.step_backward_inputs(2, *common, *ups, dy, dn)
                    r_dy2, r_dn, _ = ref((d_diff, dx, d_eo, d_gth, d_si), with_fbar=False)
                    assert np.array_equal(dy.cpu().numpy(), r_dy2) and np.array_equal(dn.cpu().numpy(), r_dn), 'stage 2 ' + what
                    assert torch.equal(dn1, dn), 'stage 1 dn ' + what
                    if N > 0:
                        fbar = ops.step_backward_fbar(n_eik, n_ds, N, Nout, dev(din), bool(use_geo), dev(d_diff), dev(dx), view, n_dev, dy)
                        assert torch.equal(dy1, dy), 'stage 2 + fbar != stage 1: ' + what
                        # everything but SampleNetwork's cells is exact; those are held to the derived bound
                        got = dy1.cpu().numpy()
                        rest = np.ones_like(got, bool)
                        rest[E:, 0] = False
                        assert np.array_equal(got[rest], r_dy2[rest]), 'stage 1 ' + what
                        parts = [a for a in (d_diff, din[:, :3] if din is not None and use_geo else None, dx) if a is not None] or [np.zeros((N, 3))]
                        bound, f64 = fbar_bound(parts, -view_np[:N], n_eval[E:E + N])
                        fb = fbar.cpu().numpy().astype(np.float64)
                        assert (np.abs(fb - f64) <= bound).all(), 'fbar ' + what
                        assert np.array_equal(got[E:, 0], (r_dy2[E:, 0] + fbar.cpu().numpy()).astype(np.float32)), 'fbar cell ' + what
                    else:
                        assert torch.equal(dy1, dy)
                    ran += 1
    assert ran >= 2 * 512


def test_step_backward_fbar_refuses_no_hit():
    z = torch.zeros(4, 3, device='cuda')
    with pytest.raises(RuntimeError):
        ops.step_backward_fbar(2, 0, 0, 3, None, True, None, None, z, z, torch.zeros(2, 3, device='cuda'))


# ------------------------------------------------------------------------------------------------ 3. SampleNetwork's scalar at grazing angles
@pytest.mark.parametrize('N', [1, 255, 256, 257, 4096])
def test_fbar_at_grazing_angles(N):
    """fbar = -(xbar . v) / (n . v) against float64 under `fbar_bound` (derived there, not measured), with n . v log-uniform in 1e-6 .. 1 on both
    signs.  Rows with n . v EXACTLY zero (v = e_z, n_z = 0: every product is a zero whatever the contraction) give what IEEE gives, -+inf by the sign of
    xbar . v or NaN for 0 / 0, the float32 restatement's bits; the rows around them are unaffected."""
    rng = np.random.default_rng(N)
    n_eik, n_ds, Nout = 3, 0, 4
    E = n_eik
    v = rng.standard_normal((N, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    w = rng.standard_normal((N, 3)); w -= (w * v).sum(-1, keepdims=True) * v
    t = 10.0 ** rng.uniform(-6, 0, N) * rng.choice([-1.0, 1.0], N)
    n0 = (t[:, None] * v + w).astype(np.float32)
    v = v.astype(np.float32)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    d_diff, dx, din = f(N, 3), f(N, 3), f(N, 13)
    zero_rows = [r for r in (7, 100, 200) if r < N]
    for r in zero_rows:
        v[r] = (0, 0, 1); n0[r, 2] = 0.0
    if N > 200:
        d_diff[200] = 0; dx[200] = 0; din[200, :3] = 0                                      # 0 / 0
    n_eval = np.concatenate([f(E, 3), n0, f(5, 3)]).astype(np.float32)
    view = np.concatenate([-v, f(5, 3)]).astype(np.float32)
    dy0 = f(E + N, Nout)
    dy = _cu(dy0)
    fbar = ops.step_backward_fbar(n_eik, n_ds, N, Nout, _cu(din), True, _cu(d_diff), _cu(dx), _cu(view), _cu(n_eval), dy).cpu().numpy()
    bound, f64 = fbar_bound([d_diff, din[:, :3], dx], v, n0)
    ok = np.ones(N, bool); ok[zero_rows] = False
    assert np.isfinite(fbar[ok]).all() and (np.abs(fbar[ok].astype(np.float64) - f64[ok]) <= bound[ok]).all()
    assert float(np.abs(f64[ok]).max()) > 1e3 or N == 1                                    # the grazing rows really are there
    _, _, f32 = SR.backward_inputs(N, 0, n_eik, n_ds, Nout, np.zeros(0, np.int64), view, n_eval, din, 11, 8, True, d_diff, dx, None, None, None, 1, 1,
                                   dtype=np.float32)
    for r in zero_rows:
        assert not np.isfinite(fbar[r]) and np.array_equal(fbar[r:r + 1].view(np.uint32) >> 23, f32[r:r + 1].view(np.uint32) >> 23), (r, fbar[r], f32[r])
        assert np.isnan(fbar[r]) == np.isnan(f32[r])
    if N > 200:
        assert np.isnan(fbar[200]) and np.isinf(fbar[7]) and np.isinf(fbar[100])
    got = dy.cpu().numpy()
    assert np.array_equal(got[E:, 0][ok], (dy0[E:, 0] + fbar)[ok]) and np.array_equal(got[:, 1:], dy0[:, 1:]) and np.array_equal(got[:E], dy0[:E])
    # stage 1 computes the same scalar in its own kernel: same bound, same non-finite rows
    dy1, dn1 = torch.zeros(E + N, Nout, device='cuda'), torch.zeros(E + N, 3, device='cuda')
    ops.step_backward_inputs(1, n_eik, n_ds, N, Nout, 0, _cu(din), 11, 8, True, _cu(d_diff), _cu(dx), _cu(view), _cu(n_eval),
                             torch.zeros(1, dtype=torch.int64, device='cuda'), None, None, None, 3, 3, dy1, dn1)
    s1 = dy1.cpu().numpy()[E:, 0]
    assert (np.abs(s1[ok].astype(np.float64) - f64[ok]) <= bound[ok]).all() and np.array_equal(np.isnan(s1), np.isnan(fbar)) and \
        np.array_equal(np.isinf(s1), np.isinf(fbar))
