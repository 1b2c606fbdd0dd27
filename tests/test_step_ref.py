"""tests/step_ref.py::backward_inputs (the numpy adjoint the GPU bookkeeping tests compare with) against torch.autograd through a float64 torch
restatement of the step's outputs (idr.py:253-304: boolean masks, torch.cat of the selected groups) composed with SampleNetwork (sample_network.py:10-20),
to 1e-12; and step_ref.outputs against the same restatement's forward values."""
import numpy as np
import pytest
import torch

import step_ref as SR


def _case(seed, R, n_eik, n_ds, Nout, p_hit=0.6):
    rng = np.random.default_rng(seed)
    E = n_eik + 2 * n_ds
    surface = rng.random(R) < p_hit
    true = rng.random(R) < 0.7
    N = int(surface.sum())
    perm = SR.sorted_rays(surface)
    true_rows = np.nonzero(true[perm[:N]])[0]
    f = lambda *s: rng.standard_normal(s)
    c = dict(R=R, n_eik=n_eik, n_ds=n_ds, E=E, N=N, Nout=Nout, surface=surface, true=true, perm=perm, true_rows=true_rows, n_true=true_rows.size,
             x=f(E + R, 3), y=f(E + R, Nout), n=f(E + R, 3), rgb_sorted=rng.random((R, 3)), view_sorted=f(R, 3))
    ld = 3 + 5 + 3 + (Nout - 2)                                    # [points | view encoding (5 here) | normals | features]
    c.update(ld=ld, nrm0=8, feat0=11, din=f(N, ld), d_diff=f(N, 3), dx=f(N, 3))
    return c


def _torch_outputs(c, y, n, d_mask, e_mask):
    """the reference's expressions on per-ray tensors, float64, differentiable in (y, n): rows [samples | rays hit first] as leaves"""
    E, N, n_eik, n_ds = c['E'], c['N'], c['n_eik'], c['n_ds']
    surface = torch.from_numpy(c['surface'])
    inv = torch.from_numpy(np.argsort(c['perm']))
    sdf_full = y[E:][inv]                                         # per ray
    normals_ray = n[E:][inv]
    points = torch.from_numpy(c['x'])[E:][inv]
    surface_output = sdf_full[surface][:, :1]
    surface_points = points[surface]
    g_hit = normals_ray[surface]
    output, g_samples, pts_samples = y[:E], n[:E], torch.from_numpy(c['x'])[:E]
    d_sw = [bool(d_mask >> g & 1) for g in range(4)]
    e_sw = [bool(e_mask >> g & 1) for g in range(4)]
    eo, gt = [], []
    if d_sw[0]: eo.append((surface_output, surface_points))
    if d_sw[1]: eo.append((output[:n_eik, :1], pts_samples[:n_eik]))
    if d_sw[2]: eo.append((output[n_eik:n_eik + n_ds, :1], pts_samples[n_eik:n_eik + n_ds]))
    if d_sw[3]: eo.append((output[n_eik + n_ds:n_eik + 2 * n_ds, :1], pts_samples[n_eik + n_ds:n_eik + 2 * n_ds]))
    eikonal_output = torch.cat([a for a, _ in eo], 0).view(1, -1) if eo else torch.zeros(1, 0, dtype=torch.float64)
    hom = torch.cat([b for _, b in eo], 0) if eo else torch.zeros(0, 3, dtype=torch.float64)
    hom = torch.cat([hom, torch.ones_like(hom[:, -1:])], -1)
    surf = torch.cat([sdf_full[:, 1][surface & torch.from_numpy(c['true'])], output[:n_eik, 1]], 0)
    if e_sw[0]: gt.append(g_hit)
    if e_sw[1]: gt.append(g_samples[:n_eik])
    if e_sw[2]: gt.append(g_samples[n_eik:n_eik + n_ds])
    if e_sw[3]: gt.append(g_samples[n_eik + n_ds:n_eik + 2 * n_ds])
    grad_theta = torch.cat(gt, 0) if gt else torch.zeros(0, 3, dtype=torch.float64)
    # SampleNetwork (sample_network.py:12-18) with cam_loc + dists * dirs = the traced point
    dirs = -torch.from_numpy(c['view_sorted'])[:N]                # rows of the hit rays are the first N sorted rows, in ray order
    dot = (g_hit.detach() * dirs).sum(-1, keepdim=True)
    diff = surface_points + (-(surface_output - surface_output.detach()) / dot) * dirs
    return dict(diff_pts=diff, eikonal_output=eikonal_output, points_hom=hom, grad_theta=grad_theta, surf=surf, sdf_output=sdf_full[:, :1],
                features=sdf_full[surface][:, 2:], normals=g_hit)


PAIRS = [(15, 15), (3, 3), (1, 2), (2, 1), (4, 8), (8, 4), (5, 10), (15, 0), (0, 15), (9, 6), (7, 11), (12, 3), (14, 13)]


@pytest.mark.parametrize('d_mask,e_mask', PAIRS)
@pytest.mark.parametrize('use_geo,nrm0', [(True, 8), (False, 8), (True, -1)])
def test_backward_inputs_is_the_autograd_adjoint(d_mask, e_mask, use_geo, nrm0):
    c = _case(d_mask * 16 + e_mask, R=40, n_eik=20, n_ds=7, Nout=6)
    E, N = c['E'], c['N']
    y = torch.from_numpy(c['y']).requires_grad_(True)
    n = torch.from_numpy(c['n']).requires_grad_(True)
    o = _torch_outputs(c, y, n, d_mask, e_mask)
    rng = np.random.default_rng(5)
    d_eo, d_gth, d_si = (rng.standard_normal(tuple(o[k].shape)) for k in ('eikonal_output', 'grad_theta', 'surf'))
    din = torch.from_numpy(c['din'])
    xbar_up = torch.from_numpy(c['d_diff']) + torch.from_numpy(c['dx']) + (din[:, :3] if use_geo else 0)
    loss = (o['diff_pts'] * xbar_up).sum() + (o['features'] * din[:, c['feat0']:]).sum() + (o['eikonal_output'] * torch.from_numpy(d_eo)).sum() + \
        (o['grad_theta'] * torch.from_numpy(d_gth)).sum() + (o['surf'] * torch.from_numpy(d_si)).sum()
    if use_geo and nrm0 >= 0:
        loss = loss + (o['normals'] * din[:, nrm0:nrm0 + 3]).sum()
    gy, gn = torch.autograd.grad(loss, (y, n), allow_unused=True)
    gn = torch.zeros_like(n) if gn is None else gn
    dy, dn, fbar = SR.backward_inputs(N, c['n_true'], c['n_eik'], c['n_ds'], c['Nout'], c['true_rows'], c['view_sorted'], c['n'], c['din'], c['feat0'],
                                      nrm0, use_geo, c['d_diff'], c['dx'], d_eo, d_gth, d_si, d_mask, e_mask)
    assert not gy[E + N:].abs().max() > 0 and not gn[E + N:].abs().max() > 0          # rays that miss receive nothing
    for got, want in ((dy, gy[:E + N].numpy()), (dn, gn[:E + N].numpy())):
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    # without the terms: stage 2 of the kernels is the same minus fbar on column 0 of the hit rows
    dy2, _, _ = SR.backward_inputs(N, c['n_true'], c['n_eik'], c['n_ds'], c['Nout'], c['true_rows'], c['view_sorted'], c['n'], c['din'], c['feat0'],
                                   nrm0, use_geo, c['d_diff'], c['dx'], d_eo, d_gth, d_si, d_mask, e_mask, with_fbar=False)
    dy2[E:, 0] += fbar
    assert np.abs(dy2 - dy).max() <= 1e-12 * np.abs(dy).max()


@pytest.mark.parametrize('d_mask,e_mask', PAIRS)
def test_outputs_are_the_reference_expressions(d_mask, e_mask):
    c = _case(d_mask * 16 + e_mask + 1000, R=33, n_eik=16, n_ds=5, Nout=4)
    o = _torch_outputs(c, torch.from_numpy(c['y']), torch.from_numpy(c['n']), d_mask, e_mask)
    got = SR.outputs(c['surface'], c['true'], c['n_eik'], c['n_ds'], c['x'], c['y'], c['n'], c['rgb_sorted'], d_mask, e_mask)
    for k in ('diff_pts', 'eikonal_output', 'points_hom', 'grad_theta', 'surf', 'sdf_output'):
        want = o[k].detach().numpy()
        assert got[k].reshape(-1).shape == want.reshape(-1).shape, k
        assert np.array_equal(got[k].reshape(want.shape), want), k
    assert np.array_equal(got['rgb_values'][c['surface']], c['rgb_sorted'][:c['N']]) and (got['rgb_values'][~c['surface']] == 1).all()
