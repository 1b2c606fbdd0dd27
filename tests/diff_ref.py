"""A float64 restatement of the differentiable MLP passes (SDF value + normal and its first- and second-order backward, the rendering network's
forward and backward, the weight-norm fold backward) with plain torch autograd, plus the seeded parameters the tests of tests/test_gpu_diff_fp64.py use.

The formulas are the reference's (idr.py:33-107 and 121-167): the positional encoding [x, sin(2^m x), cos(2^m x)]_m, the skip concatenation
cat([h, PE]) / sqrt(2), Softplus(beta=100) with torch's threshold, weight norm w = g v / |v|, ReLU / tanh in the rendering network and its three modes.
The normal is autograd's gradient of output 0 with create_graph=True, so the backward through it is autograd's double backward.

Every function takes `dtype`: torch.float64 is the reference; torch.float32 is PyTorch's own fp32 CPU evaluation of the same formulas, the error
yardstick of the GPU tests (tests/test_gpu_featext.py's rule).  The weight gradients are those of the FOLDED weights W = g v / |v| (what
ops.sdf_backward / ops.render_backward return); fold_backward maps them to (dv, dg)."""
import numpy as np
import torch
import torch.nn.functional as F

SQRT2 = float(np.float32(np.sqrt(2.0)))      # torch divides the float32 skip concatenation by fl32(np.sqrt(2)) (idr.py:87); the kernels use the same constant


# ------------------------------------------------------------------------------------------------ parameters
def sdf_dims(W, n_hidden=8, multires=6, feat=256, skip_in=(4,)):
    """[(in, out)] per Linear of the SDF net (idr.py:33-51): input PE(x), output 1 + feat columns (the value, then the feature vector)."""
    d0 = 3 + 6 * multires if multires > 0 else 3
    dims = [d0] + [W] * n_hidden + [1 + feat]
    return [(dims[l], dims[l + 1] - d0 if (l + 1) in skip_in else dims[l + 1]) for l in range(len(dims) - 1)]


def render_dims(W, n_hidden=4, multires_view=4, feat=256, mode='idr'):
    """[(in, out)] per Linear of the rendering net (idr.py:121-131) in one of its modes."""
    d0 = 3 + (0 if mode == 'no_view_dir' else 3 + 6 * multires_view) + (0 if mode == 'no_normal' else 3) + feat
    dims = [d0] + [W] * n_hidden + [3]
    return [(dims[l], dims[l + 1]) for l in range(len(dims) - 1)]


def sdf_params(W, seed, n_hidden=8, multires=6, feat=256, skip_in=(4,)):
    """float32 (v, g, b) per layer, geometric-init-like (mvsdf_amd/utils/synth.py::make_state_dict at any width, PE order, skip set and feature
    size): the first output is near |x| - 0.6, so the Softplus inputs straddle 0 and every regime of sigma(100 z) occurs."""
    rs = np.random.RandomState(seed)
    dims = sdf_dims(W, n_hidden, multires, feat, skip_in)
    d0, L, out = dims[0][0], len(dims), []
    for l, (i, o) in enumerate(dims):
        if l == L - 1:
            w = rs.normal(0.0, 0.3 / np.sqrt(i), size=(o, i))
            w[0] = rs.normal(np.sqrt(np.pi) / np.sqrt(i), 1e-4, size=i)
            b = rs.normal(0.0, 0.1, size=o); b[0] = -0.6
            if l in skip_in:
                w[:, -d0:] = rs.normal(0.0, 0.01, size=(o, d0))
        elif l == 0:
            w = np.zeros((o, i))
            w[:, :3] = rs.normal(0.0, np.sqrt(2) / np.sqrt(o), size=(o, 3))
            w[:, 3:] = rs.normal(0.0, 0.02, size=(o, i - 3))
            b = rs.normal(0.0, 0.02, size=o)
        else:
            w = rs.normal(0.0, np.sqrt(2) / np.sqrt(o), size=(o, i))
            b = rs.normal(0.0, 0.02, size=o)
        g = np.sqrt((w * w).sum(1, keepdims=True)) * rs.uniform(0.9, 1.1, size=(o, 1))
        v = w + 0.02 * np.abs(w).mean() * rs.normal(size=w.shape)
        out.append(tuple(torch.from_numpy(a.astype(np.float32)) for a in (v, g, b)))
    return out


def render_params(dims, seed):
    """float32 (v, g, b) per layer of a rendering net (torch.nn.Linear's uniform init)."""
    rs = np.random.RandomState(seed)
    out = []
    for i, o in dims:
        k = 1.0 / np.sqrt(i)
        w = rs.uniform(-k, k, size=(o, i))
        out.append(tuple(torch.from_numpy(a.astype(np.float32)) for a in (w, np.sqrt((w * w).sum(1, keepdims=True)), rs.uniform(-k, k, size=o))))
    return out


def state_dict(params, prefix):
    """(v, g, b) per layer -> {prefix.lin{l}.weight_v / weight_g / bias: numpy} (the key layout tests/helpers.py::sdf_packed_net reads)."""
    sd = {}
    for l, (v, g, b) in enumerate(params):
        sd['%s.lin%d.weight_v' % (prefix, l)] = v.numpy()
        sd['%s.lin%d.weight_g' % (prefix, l)] = g.numpy()
        sd['%s.lin%d.bias' % (prefix, l)] = b.numpy()
    return sd


# ------------------------------------------------------------------------------------------------ building blocks
def fold(v, g):
    """weight norm (torch.nn.utils.weight_norm, dim 0): W = g v / |v| per output row."""
    return v * (g.reshape(-1, 1) / torch.linalg.vector_norm(v, dim=1, keepdim=True))


def pe(x, multires):
    """[x, sin(2^m x), cos(2^m x)]_m  (model/embedder.py)."""
    out = [x]
    for m in range(multires):
        out += [torch.sin(x * 2.0 ** m), torch.cos(x * 2.0 ** m)]
    return torch.cat(out, 1)


def softplus100(z):
    return F.softplus(z, beta=100)                  # torch's threshold: beta * z > 20 -> z


def folded(params, dtype, requires_grad=False):
    """-> [(W, b)] in dtype (W folded in dtype from the fp32 v, g)."""
    out = []
    for v, g, b in params:
        W = fold(v.to(dtype), g.to(dtype)).detach().requires_grad_(requires_grad)
        out.append((W, b.to(dtype).detach().requires_grad_(requires_grad)))
    return out


def sdf_value(Wb, x, multires, skip_in):
    h0 = pe(x, multires)
    a, L = h0, len(Wb)
    for l, (W, b) in enumerate(Wb):
        if l in skip_in:
            a = torch.cat([a, h0], 1) / SQRT2
        z = a @ W.t() + b
        a = softplus100(z) if l < L - 1 else z
    return a


# ------------------------------------------------------------------------------------------------ the passes
def sdf_forward(params, x, Mg, multires, skip_in, dtype=torch.float64):
    """ops.sdf_forward: x[M,3] -> (y[M, 1 + feat], n[Mg, 3]) with n = d y[:, 0] / dx."""
    Wb = folded(params, dtype)
    x = x.to(dtype).detach().requires_grad_(True)
    y = sdf_value(Wb, x, multires, skip_in)
    n, = torch.autograd.grad(y[:, 0].sum(), x)
    return y.detach(), n[:Mg].detach()


def sdf_backward(params, x, row0, dy, dn, multires, skip_in, dtype=torch.float64):
    """ops.sdf_backward over the rows [row0, row0 + Mb) (Mb = dy's rows): the gradients of sum(y . dy) + sum(n . dn) (dn None: the first term only)
    -> (dWs, dbs, dx[Mb,3]) (dW of the folded weights)."""
    Wb = folded(params, dtype, requires_grad=True)
    Mb = dy.shape[0]
    x = x[row0:row0 + Mb].to(dtype).detach().requires_grad_(True)
    y = sdf_value(Wb, x, multires, skip_in)
    loss = (y * dy.to(dtype)).sum()
    if dn is not None:
        n, = torch.autograd.grad(y[:, 0].sum(), x, create_graph=True)
        loss = loss + (n * dn.to(dtype)).sum()
    leaves = [t for wb in Wb for t in wb] + [x]
    gr = torch.autograd.grad(loss, leaves)
    return list(gr[0:-1:2]), list(gr[1:-1:2]), gr[-1]


def render_input(points, view, normals, feat, multires_view, mode='idr'):
    """cat[points, (view, PE(view)), normals, feat] per the mode (idr.py:145-154)."""
    parts = [points]
    if mode != 'no_view_dir':
        parts.append(pe(view, multires_view))
    if mode != 'no_normal':
        parts.append(normals)
    parts.append(feat)
    return torch.cat(parts, 1)


def render_forward_backward(params, points, view, normals, feat, multires_view, mode, drgb, dtype=torch.float64):
    """ops.render_forward + ops.render_backward: -> (rgb, dWs, dbs, din) with din the adjoint of the concatenated input row (render_input)."""
    Wb = folded(params, dtype, requires_grad=True)
    a = render_input(*(t.to(dtype) for t in (points, view, normals, feat)), multires_view, mode).detach().requires_grad_(True)
    h, L = a, len(Wb)
    for l, (W, b) in enumerate(Wb):
        h = h @ W.t() + b
        h = torch.relu(h) if l < L - 1 else torch.tanh(h)
    gr = torch.autograd.grad((h * drgb.to(dtype)).sum(), [t for wb in Wb for t in wb] + [a])
    return h.detach(), list(gr[0:-1:2]), list(gr[1:-1:2]), gr[-1]


def fold_backward(v, g, dW, dtype=torch.float64):
    """backward of W = g v / |v|: dW -> (dv, dg[N,1])."""
    v = v.to(dtype).detach().requires_grad_(True)
    g = g.to(dtype).reshape(-1, 1).detach().requires_grad_(True)
    return torch.autograd.grad((fold(v, g) * dW.to(dtype)).sum(), [v, g])
