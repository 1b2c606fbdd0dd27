"""The loss kernels (csrc/loss_kernels.hip) where their edge branches fire, against the float64 oracle (oracle/oracle_np.py, pinned to the reference by
tests/test_oracle_np_golden.py), point by point:
  * k_feat_corr on projections inside the map, in the half-pixel border band (zeros-padded taps), out of range, clamped and behind a source camera, a
    zero-feature patch (norm clamp) and anti-correlated features; C = 1 / 8 / 17 / 32 (idle lanes), V = 1 / 2 / 5 (an idle half-wave), maps from 1 x 1 to
    60 x 80, NCHW, channels_last and a strided feat_src view;
  * k_carve with 1 to 37 depth views, an all-zero depth map, points outside every frustum and behind a camera, carving_t2 and carving_t; the fused
    k_loss_prep_carve (the native IDRLoss) equal to k_carve bit for bit;
  * k_loss_terms on extreme BCE logits, SmoothL1 arguments one ulp either side of 1, exact rgb ties and a zero gradient row against float64 autograd, and
    its 16-workgroup form (the native IDRLoss) equal to its one-workgroup form bit for bit across the slice boundaries;
  * one IDRLoss forward + backward on 20 views (the prep kernel's views beyond 16) with hits near the source-image borders."""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

from conftest import golden
from helpers import t
from mvsdf_amd import ops
from mvsdf_amd.model import conf as conf_mod
from mvsdf_amd.model.loss import IDRLoss
from mvsdf_amd.utils import synth
from oracle import oracle_np as ON

pytestmark = pytest.mark.gpu

SIZE, CENTER = 2.5, (0.1, -0.2, 0.05)                            # the scene of synth.make_feat_edges


# ------------------------------------------------------------------------------------------------ k_feat_corr
def _layouts(feat, fsrc):
    """NCHW, channels_last, and feat_src as every other view of a larger tensor whose other views are NaN (a wrong stride reads them)."""
    yield 'nchw', feat, fsrc
    yield 'channels_last', feat.contiguous(memory_format=torch.channels_last), fsrc.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    big = torch.full((fsrc.shape[0], 2 * fsrc.shape[1]) + tuple(fsrc.shape[2:]), float('nan'), device=fsrc.device)
    big[:, ::2] = fsrc
    yield 'strided', feat, big[:, ::2]


def _check_feat_corr(d, expect_inside=True):
    """k_feat_corr vs the oracle on the inputs of synth.make_feat_edges, per point, in every layout.  -> number of ties."""
    B, C, H, W = d['feat'].shape
    V = d['feat_src'].shape[1]
    counts = d['hits'].reshape(B, -1).sum(1)
    args = (counts, d['feat'], d['cam'], d['feat_src'], d['src_cams'], d['size'][0], d['center'][0])
    _, dp, pp = ON.feat_corr_loss(d['points'], *args, with_grad=True, per_point=True)
    gr, depth, cl = ON.feat_corr_decisions(d['points'], *args)
    zones = ON.feat_corr_zones(gr, depth, H, W)
    for z in ON.FEAT_ZONES:                                      # the case reaches every zone (a 1 x 1 map has no tap-free inside)
        assert zones[z].any() or (z == 'inside' and not expect_inside), z
    ties = ON.feat_corr_ties(gr, cl)
    print('B %d C %d V %d %dx%d: %d points, %d ties' % (B, C, V, H, W, len(pp), ties.sum()))
    assert ties.sum() <= 2, ties.sum()
    ok = ~ties
    m_b = np.repeat(counts, counts).astype(np.float64)
    scale = B * V * m_b                                          # undo the weight of loss_pp: the point's corr_loss summed over its source views
    # with C = 1 (corr = +-1) or a 1 x 1 map (every sample a multiple of the one pixel) the loss is piecewise constant: the analytic gradient is 0
    # and the kernel's is fp32 noise (measured: 5.6e-7), bounded by the floor 2e-4 * 1e-2, which lies below every other case's largest entry
    gmax = np.abs(dp).max()
    assert C == 1 or H * W == 1 or gmax > 1e-2, gmax
    # points 0.2-0.7 from the reference camera (the 'behind source view 0' zone) are ill-conditioned in fp32: rounding their coordinates by one ulp
    # moves the oracle's sum by up to 2.0e-5 (measured: kernel error 2.1e-5 at C = 32, V = 5, 60 x 80).  2e-5 holds for the others; 5e-5 for these
    tol = np.where(depth[:, 0] < 1.0, 5e-5, 2e-5)
    vs = t(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))
    for name, feat, fsrc in _layouts(t(d['feat']), t(d['feat_src'])):
        lpp, dpts = ops.feat_corr(t(d['points']), vs, feat, fsrc, t(d['cam']), t(d['src_cams']), t(d['size']), t(d['center']))
        lpp, dpts = lpp.double().cpu().numpy(), dpts.double().cpu().numpy()
        err = np.abs(lpp * scale - pp * scale)
        print('  %-13s max |sum corr_loss - oracle| %.3g (far points %.3g), max |dpts - oracle| %.3g of %.3g'
              % (name, err[ok].max(), err[ok & (tol < 3e-5)].max(), np.abs(dpts - dp)[ok].max(), gmax))
        assert (err <= tol)[ok].all(), (name, err[ok].max())
        gerr = np.abs(dpts - dp)[ok].max()
        assert gerr <= 2e-4 * max(gmax, 1e-2), (name, gerr, gmax)
    return int(ties.sum())


def test_feat_corr_edges_fixture():
    """The reference fixture feat_corr_edges (C = 17, V = 5, 37 x 53, a view without hits): per point against the oracle, and the total against the
    reference's loss."""
    g = golden('feat_corr_edges')
    d = synth.make_feat_edges(int(g['seed']))
    assert np.array_equal(d['points'], g['points'])
    _check_feat_corr(d)
    counts = g['hits'].reshape(int(g['B']), -1).sum(1)
    vs = t(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))
    lpp, dpts = ops.feat_corr(t(d['points']), vs, t(d['feat']), t(d['feat_src']), t(d['cam']), t(d['src_cams']), t(d['size']), t(d['center']))
    assert abs(float(lpp.double().sum()) - float(g['loss'])) <= 1e-4 * float(g['loss'])
    assert np.abs(dpts.cpu().numpy() - g['dpoints64']).max() <= 2e-4 * np.abs(g['dpoints64']).max()


@pytest.mark.parametrize('hw', [(1, 1), (7, 5), (37, 53), (60, 80)])
@pytest.mark.parametrize('V', [1, 2, 5])
@pytest.mark.parametrize('C', [1, 8, 17, 32])
def test_feat_corr_edges_shapes(C, V, hw):
    d = synth.make_feat_edges(1, B=3, P=120, V=V, C=C, H=hw[0], W=hw[1])
    _check_feat_corr(d, expect_inside=min(hw) > 1)


# ------------------------------------------------------------------------------------------------ depth carving
def _depth_scene(dB, seed=0, M=3000):
    """dB depth views on a circle (bumpy depth maps with holes; view dB // 2 all zero when dB > 1) and M normalised points: around the surface,
    uniform, outside every frustum, and behind depth camera 0."""
    inp, _ = synth.make_batch(dB, 8, 1, seed=seed, size=SIZE, center=CENTER, feat_hw=(48, 64), focal_scale=1.4, with_features=False)
    dcams = inp['depth_cams']
    depths = synth.make_depth_maps(dcams, SIZE, CENTER, seed=seed)
    if dB > 1:
        depths[dB // 2] = 0.0
    rs = np.random.RandomState(seed + 77)
    pts = rs.uniform(-1.3, 1.3, size=(M, 3))
    n = rs.normal(size=(M // 2, 3))
    pts[:M // 2] = n / np.linalg.norm(n, axis=1, keepdims=True) * (0.6 + 0.05 * rs.normal(size=(M // 2, 1)))
    nf, nb = min(200, M // 8), min(100, M // 8)
    pts[M - nf:] *= 4.0
    E = dcams[0, 0, 0].astype(np.float64)
    cw = -E[:3, :3].T @ E[:3, 3]                                  # camera 0's centre (world) and its viewing axis
    behind = cw[None] - E[2, :3][None] * rs.uniform(0.1, 1.0, size=(nb, 1)) + 0.2 * rs.normal(size=(nb, 3))
    pts[M // 2:M // 2 + nb] = (behind - np.asarray(CENTER)) / SIZE * 2
    eo = (0.3 * rs.normal(size=M)).astype(np.float32)
    return depths, dcams, pts.astype(np.float32), eo


@pytest.mark.parametrize('use_invalid', [False, True])
@pytest.mark.parametrize('dB', [1, 5, 17, 37])
def test_depth_carve_many_views_vs_oracle(dB, use_invalid):
    """k_carve vs oracle_np.depth_loss (carving_t2 / carving_t + the weighting of get_depth_loss), with the boundary-flip allowance of
    test_gpu_loss.py::test_depth_carve_vs_reference."""
    depths, dcams, pts, eo = _depth_scene(dB)
    size, center = np.array([SIZE], np.float32), np.asarray(CENTER, np.float32)[None]
    pw = pts.astype(np.float64) / 2 * SIZE + np.asarray(CENTER)
    E = dcams[0, 0, 0].astype(np.float64)
    assert ((pw @ E[2, :3] + E[2, 3]) < 0).sum() >= 50                                      # behind camera 0
    for fa, na in ((1.0, 1.0), (0.5, 0.01)):
        loss_ref, dr_ref, w_ref = ON.depth_loss(pts, eo, depths, dcams, SIZE, CENTER[0:3], 0.25, fa, 0.1, na, use_invalid=use_invalid)
        assert (w_ref == 0).sum() > 200 and (w_ref > 0).sum() > 200                          # points no view sees, and seen ones
        dist_r, w = ops.depth_carve(t(pts), t(depths[:, 0, 0]), t(dcams[:, 0]), t(size), t(center), 1 / 8, 0.25, fa, 0.1, na, use_invalid=use_invalid)
        dist_r, w = dist_r.cpu().numpy(), w.cpu().numpy()
        bad = np.abs(dist_r - dr_ref) > 1e-5
        assert bad.sum() <= 4, bad.sum()
        assert np.array_equal((w > 0)[~bad], (w_ref > 0)[~bad]) and np.abs(w - w_ref)[~bad].max() < 1e-6
        loss = float((np.abs(eo.astype(np.float64) + dist_r) * w).mean())
        assert abs(loss - loss_ref) <= 2e-3 * loss_ref * max(1, bad.sum()) + 1e-6, (loss, loss_ref)


# ------------------------------------------------------------------------------------------------ IDRLoss on a hand-made output dict
def _outputs(B, P, dB, seed=0, V=2, C=8, hw=(37, 53), M=None):
    """An output dict of plain tensors with autograd leaves (any producer may feed IDRLoss) and its ground truth: feature-consistency inputs from
    synth.make_feat_edges (hits near the map borders), the depth scene of _depth_scene, extreme surface logits, exact rgb ties, a zero gradient row."""
    d = synth.make_feat_edges(seed, B=B, P=P, V=V, C=C, H=hw[0], W=hw[1])
    R = B * P
    rs = np.random.RandomState(seed + 99)
    M = M if M is not None else max(R, 64)
    depths, dcams, pts, eo = _depth_scene(dB, seed, M)
    rgb = rs.uniform(-1, 1, size=(R, 3)).astype(np.float32)
    rgb_gt = rs.uniform(-1, 1, size=(R, 3)).astype(np.float32)
    rgb_gt[::3] = rgb[::3]                                                                     # exact ties
    n_eik = max(1, R // 2)
    gth = rs.normal(size=(n_eik, 3)).astype(np.float32)
    gth[0] = 0.0
    surf = np.resize(np.array([0, 1e-3, -1e-3, 20, -20, 60, -60, 100, -100, 1e4, -1e4], np.float32), R)
    hits = d['hits']
    true = hits & (rs.uniform(size=R) < 0.7)
    hom = np.concatenate([pts, np.ones((M, 1), np.float32)], 1).reshape(1, M, 4, 1)
    leaves = dict(diff_surf_pts=t(d['points']), rgb_values=t(rgb), grad_theta=t(gth), eikonal_output=t(eo.reshape(M, 1)), surf_indicator_output=t(surf))
    leaves = {k: v.requires_grad_(True) for k, v in leaves.items()}
    out = dict(leaves, network_object_mask=t(hits), object_mask=t(np.ones(R, bool)), object_mask_true=t(true), eikonal_points_hom=t(hom))
    gt = dict(rgb=t(rgb_gt.reshape(B, P, 3)), depths=t(depths), depth_cams=t(dcams), size=t(np.full(B, SIZE, np.float32)),
              center=t(np.tile(np.asarray(CENTER, np.float32)[None], (B, 1))), feat=t(d['feat']), feat_src=t(d['feat_src']), cam=t(d['cam']),
              src_cams=t(d['src_cams']))
    return out, leaves, gt, d, (depths, dcams, pts, eo)


def _run_loss(native, out, leaves, gt, tp=0.3):
    o = dict(out)
    o['eikonal_points_hom'] = out['eikonal_points_hom'].clone()                               # rescaled in place by the loss
    lf = IDRLoss()
    lf.native = native
    lo = lf(o, dict(gt), tp, 2)
    grads = torch.autograd.grad(lo['loss'], list(leaves.values()))
    return lo, dict(zip(leaves, grads)), o['eikonal_points_hom']


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    assert torch.equal(a, b), '%s differs: max |d| = %g' % (what, float((a.double() - b.double()).abs().max()))


def _native_vs_python(out, leaves, gt):
    la, ga, ha = _run_loss(True, out, leaves, gt)
    lb, gb, hb = _run_loss(False, out, leaves, gt)
    for k in la:
        _same(la[k].detach().reshape(-1), lb[k].detach().reshape(-1), k)
    for k in ga:
        _same(ga[k], gb[k], 'd loss / d ' + k)
    _same(ha, hb, 'world-space eikonal_points_hom')
    return la, ga


@pytest.mark.parametrize('use_invalid', [False, True])
@pytest.mark.parametrize('dB', [1, 5, 17, 37])
def test_prep_carve_equals_carve(dB, use_invalid, monkeypatch):
    """The native IDRLoss carves with k_loss_prep_carve (16 waves split the views: w, w + 16, ...), native = False with k_carve: depth_loss and
    d loss / d eikonal_output identical, with 1 to 37 depth views (more than one view per wave from 17 on)."""
    monkeypatch.setattr(conf_mod, 'use_invalid', use_invalid)
    out, leaves, gt, _, _ = _outputs(2, 64, dB, M=2500)
    la, ga = _native_vs_python(out, leaves, gt)
    assert float(la['depth_loss']) > 0 and (ga['eikonal_output'] != 0).sum() > 500


# ------------------------------------------------------------------------------------------------ k_loss_terms
def _terms64(rgb, rgb_gt, mask, gth, eo, dr, dw, surf, n_pos, fpp, w, smooth):
    """The IDRLoss terms (loss.py:21-35, 57-61, 167-174) and their gradients w.r.t. each term's input, float64 autograd on the CPU."""
    x = [torch.tensor(np.asarray(a, np.float64), requires_grad=True) for a in (rgb, gth, eo, surf)]
    R = rgb.shape[0]
    m = torch.tensor(mask)
    rgb_l = ((x[0] - torch.tensor(rgb_gt, dtype=torch.float64)).abs() * m[:, None]).sum() / R
    eik = ((x[1].norm(2, dim=1) - 1) ** 2).mean()
    dr_, dw_ = torch.tensor(dr, dtype=torch.float64), torch.tensor(dw, dtype=torch.float64)
    if smooth > 0:
        el = F.smooth_l1_loss(x[2] / smooth, -dr_ / smooth, reduction='none') * smooth
    else:
        el = (x[2] + dr_).abs()
    depth = (el * dw_).mean()
    tgt = (torch.arange(len(surf)) < n_pos).to(torch.float64)
    surf_l = F.binary_cross_entropy_with_logits(x[3], tgt)
    feat = float(np.sum(fpp, dtype=np.float64))
    terms = [rgb_l, eik, depth, surf_l]
    grads = [torch.autograd.grad(v, xi)[0].numpy() for v, xi in zip(terms, x)]
    vals = [float(v) for v in terms] + [feat]
    total = vals[0] * w[0] + vals[1] * w[1] + vals[3] * w[2] + feat * w[3] + vals[2] * w[4]
    return [total] + vals[:3] + [feat, vals[3]], grads


@pytest.mark.parametrize('smooth', [0.0, 0.5])
@pytest.mark.parametrize('R', [1, 383, 384, 385, 6145, 32768])
def test_loss_terms_vs_float64(R, smooth):
    rs = np.random.RandomState(R)
    rgb = rs.uniform(-1, 1, size=(R, 3)).astype(np.float32)
    rgb_gt = rs.uniform(-1, 1, size=(R, 3)).astype(np.float32)
    rgb_gt[::4] = rgb[::4]                                                                      # exact ties: no gradient
    rgb_gt[1::4, 1] = rgb[1::4, 1]
    mask = rs.uniform(size=R) < 0.8
    n_eik = max(1, R // 2 + 1)
    gth = rs.normal(size=(n_eik, 3)).astype(np.float32)
    gth[0] = 0.0                                                                                # zero norm
    n_d = R + 3
    one = np.float32(1.0)
    x = np.resize(np.array([np.nextafter(one, np.float32(0)), one, np.nextafter(one, np.float32(2))], np.float32), n_d)
    x *= np.resize(np.array([1, -1], np.float32), n_d)
    eo = (x * np.float32(0.5)).astype(np.float32)                                              # SmoothL1 argument eo / 0.5 + dist_r / 0.5 = +-(1 +- 1 ulp)
    dr = np.zeros(n_d, np.float32)
    dr[3::4] = rs.uniform(-1, 1, size=dr[3::4].shape)
    dw = np.where(rs.uniform(size=n_d) < 0.2, 0.0, rs.choice([1.0, 0.1, 0.01], size=n_d)).astype(np.float32)
    surf = np.resize(np.array([0, 1e-3, -1e-3, 20, -20, 60, -60, 100, -100, 1e4, -1e4], np.float32), R + 5)
    rs.shuffle(surf)
    n_pos = (R + 5) // 2
    fpp = rs.uniform(0, 1e-3, size=R).astype(np.float32)
    w = (0.5, 0.1, 0.01, 0.1, 1.0)
    out, d_rgb, d_grad, d_eo, d_sf = ops.loss_terms(t(rgb), t(rgb_gt), t(mask), t(gth), t(eo), t(dr), t(dw), t(surf),
                                                    torch.tensor(n_pos, device='cuda'), t(fpp), w + (smooth,), True, True)
    ref, gref = _terms64(rgb, rgb_gt, mask, gth, eo, dr, dw, surf, n_pos, fpp, w, smooth)
    got = out.double().cpu().numpy()
    for k, name in enumerate(('loss', 'rgb', 'eikonal', 'depth', 'feat', 'surf')):
        assert abs(got[k] - ref[k]) <= 1e-5 * abs(ref[k]) + 1e-9, (name, got[k], ref[k])
    for name, a, b in zip(('rgb', 'grad_theta', 'eikonal_output', 'surf'), (d_rgb, d_grad, d_eo, d_sf), gref):
        a = a.double().cpu().numpy().reshape(b.shape)
        assert np.isfinite(a).all(), name
        assert np.abs(a - b).max() <= 2e-6 * np.abs(b).max(), (name, np.abs(a - b).max(), np.abs(b).max())
    assert (d_rgb.cpu().numpy()[::4] == 0).all() and (d_grad.cpu().numpy()[0] == 0).all()


@pytest.mark.parametrize('R', [1, 383, 384, 385, 6145, 32768])
def test_loss_terms_sixteen_workgroups_equal_one(R):
    """mvsdf_loss_forward (the native IDRLoss: 16 workgroups, slice sums through a ticket) vs mvsdf_loss_terms (native = False: one workgroup walks
    the 16 slices): every term and every gradient identical, at row counts either side of the slice boundaries and at the shipped batch size."""
    out, leaves, gt, _, _ = _outputs(1, R, 3, seed=1, V=2, C=8, hw=(7, 5), M=R + 7)
    la, ga = _native_vs_python(out, leaves, gt)
    for k in la:
        assert torch.isfinite(la[k]).all(), k
    assert float(la['surf_loss']) > 0 and float(la['eikonal_loss']) > 0


# ------------------------------------------------------------------------------------------------ end to end
def test_idr_loss_twenty_views_vs_oracle():
    """One IDRLoss forward + backward on 20 views x 24 rays whose hits project near the source-image borders (both routes, identical), its
    feat_loss, depth_loss and d loss / d diff_surf_pts against the oracle evaluated on the same outputs."""
    B, P = 20, 24
    out, leaves, gt, d, (depths, dcams, pts, eo) = _outputs(B, P, 20, seed=2, V=5, C=17)
    la, ga = _native_vs_python(out, leaves, gt)
    counts = d['hits'].reshape(B, P).sum(1)
    assert (counts == 0).any() and B > 16
    args = (counts, d['feat'], d['cam'], d['feat_src'], d['src_cams'], SIZE, np.asarray(CENTER))
    gr, depth, cl = ON.feat_corr_decisions(d['points'], *args)
    assert not ON.feat_corr_ties(gr, cl).any()
    assert ON.feat_corr_zones(gr, depth, *d['feat'].shape[2:])['band'].any()
    floss, dp = ON.feat_corr_loss(d['points'], *args, with_grad=True)
    assert abs(float(la['feat_loss']) - floss) <= 2e-5 / 5, (float(la['feat_loss']), floss)
    w_feat = conf_mod.feat_weight(0.3)
    gd = ga['diff_surf_pts'].double().cpu().numpy()
    assert np.abs(gd - w_feat * dp).max() <= 2e-4 * w_feat * np.abs(dp).max()
    near_att = conf_mod.near_att(0.3)
    dl, _, _ = ON.depth_loss(pts, eo, depths, dcams, SIZE, np.asarray(CENTER), 0.25, 1, 0.1, near_att)
    assert abs(float(la['depth_loss']) - dl) <= 2e-3 * dl
