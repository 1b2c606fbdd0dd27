"""The float64 restatement of tests/diff_ref.py (torch autograd) against the closed-form numpy oracle (oracle/oracle_np.py) on the inputs of the
differentiable goldens: two independent statements of the same passes must agree to rounding, so the GPU tests that hold the kernels to
diff_ref are anchored to the reference's formulas."""
import numpy as np
import pytest
import torch

import diff_ref as R
from conftest import golden
from mvsdf_amd.utils import synth
from oracle import oracle_np as ON

TOL = 1e-12


def _params(sd, prefix):
    out, l = [], 0
    while '%s.lin%d.weight_v' % (prefix, l) in sd:
        out.append(tuple(torch.from_numpy(sd['%s.lin%d.%s' % (prefix, l, k)]) for k in ('weight_v', 'weight_g', 'bias')))
        l += 1
    return out


def _close(a, b, what):
    a = a.detach().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape, what
    err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
    assert err < TOL, (what, err)


@pytest.mark.parametrize('W', [64, 256, 512])
def test_sdf_forward_matches_oracle(W):
    g = golden('sdf_w%d' % W)
    sd = synth.make_state_dict(W, int(g['seed']))
    x = torch.from_numpy(g['x'])
    y, n = R.sdf_forward(_params(sd, 'implicit_network'), x, x.shape[0], 6, (4,))
    oy, on, _ = ON.sdf_forward(ON.sdf_net(sd), g['x'])
    _close(y, oy, 'y')
    _close(n, on, 'n')


@pytest.mark.parametrize('name', ['sdf_bwd_w64', 'sdf_bwd_w64_skip8', 'sdf_bwd_w64_skips36'])
def test_sdf_double_backward_matches_oracle(name):
    g = golden(name)
    skip = tuple(int(s) for s in g['skip_in'])
    sd = synth.make_state_dict(int(g['W']), int(g['seed']), skip_in=skip)
    params = _params(sd, 'implicit_network')
    onet = ON.sdf_net(sd, skip_in=skip)
    x, dy, dn = (torch.from_numpy(g[k]) for k in ('x', 'dy', 'dn'))
    _, _, cache = ON.sdf_forward(onet, g['x'])
    for use_dn in (True, False):
        dWs, dbs, dx = R.sdf_backward(params, x, 0, dy, dn if use_dn else None, 6, skip)
        oW, ob, odx = ON.sdf_backward(onet, cache, g['dy'], g['dn'] if use_dn else None)
        _close(dx, odx, 'dx')
        for l in range(len(params)):
            _close(dWs[l], oW[l], 'dW%d' % l)
            _close(dbs[l], ob[l], 'db%d' % l)
            dv, dgg = R.fold_backward(params[l][0], params[l][1], dWs[l])
            ov, og = ON.fold_backward(params[l][0].numpy(), params[l][1].numpy(), oW[l])
            _close(dv, ov, 'dv%d' % l)
            _close(dgg, og, 'dg%d' % l)
    # a row window: rows [row0, row0 + Mb) alone
    row0, Mb = 5, 60
    _, _, c2 = ON.sdf_forward(onet, g['x'][row0:row0 + Mb])
    oW, ob, odx = ON.sdf_backward(onet, c2, g['dy'][row0:row0 + Mb], g['dn'][row0:row0 + Mb])
    dWs, dbs, dx = R.sdf_backward(params, x, row0, dy[row0:row0 + Mb], dn[row0:row0 + Mb], 6, skip)
    _close(dx, odx, 'dx window')
    for l in range(len(params)):
        _close(dWs[l], oW[l], 'dW%d window' % l)


def test_render_forward_backward_matches_oracle():
    g = golden('render_bwd_w64')
    sd = synth.make_state_dict(int(g['W']), int(g['seed']))
    params = _params(sd, 'rendering_network')
    pts, view, nrm, feat, drgb = (torch.from_numpy(g[k]) for k in ('points', 'view', 'normals', 'feat', 'drgb'))
    rgb, dWs, dbs, din = R.render_forward_backward(params, pts, view, nrm, feat, 4, 'idr', drgb)
    onet = ON.render_net(sd)
    orgb, cache = ON.render_forward(onet, g['points'], g['normals'], g['view'], g['feat'])
    oW, ob, dp, dnn, df = ON.render_backward(onet, cache, g['drgb'])
    _close(rgb, orgb, 'rgb')
    dv = 3 + 6 * 4
    _close(din[:, :3], dp, 'dpoints')
    _close(din[:, 3 + dv:6 + dv], dnn, 'dnormals')
    _close(din[:, 6 + dv:], df, 'dfeat')
    for l in range(len(params)):
        _close(dWs[l], oW[l], 'dW%d' % l)
        _close(dbs[l], ob[l], 'db%d' % l)


def test_render_modes_drop_their_columns():
    """'no_view_dir' / 'no_normal' are the 'idr' network without the view (+ PE) / normal columns (idr.py:149-154): with those columns of the first
    layer zeroed, 'idr' computes the same colour, and the other columns' adjoints agree."""
    gen = torch.Generator().manual_seed(2)
    N, F_, mv = 40, 32, 4
    pts, view, nrm = (torch.randn(N, 3, generator=gen, dtype=torch.float64) for _ in range(3))
    feat = torch.randn(N, F_, generator=gen, dtype=torch.float64)
    drgb = torch.randn(N, 3, generator=gen, dtype=torch.float64)
    full = R.render_params(R.render_dims(32, 2, mv, F_, 'idr'), 3)
    dv = 3 + 6 * mv
    for mode, cols in (('no_view_dir', list(range(3, 3 + dv))), ('no_normal', list(range(3 + dv, 6 + dv)))):
        keep = [c for c in range(full[0][0].shape[1]) if c not in cols]
        v0 = full[0][0].clone(); v0[:, cols] = 0
        g0 = torch.linalg.vector_norm(v0.double(), dim=1, keepdim=True).float()
        a = [(v0, g0, full[0][2])] + full[1:]
        b = [(v0[:, keep].contiguous(), g0, full[0][2])] + full[1:]
        rgb_a, _, _, din_a = R.render_forward_backward(a, pts, view, nrm, feat, mv, 'idr', drgb)
        rgb_b, _, _, din_b = R.render_forward_backward(b, pts, view, nrm, feat, mv, mode, drgb)
        _close(rgb_b, rgb_a, mode)
        _close(din_b, din_a[:, keep], mode)
