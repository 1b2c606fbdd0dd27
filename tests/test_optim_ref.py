"""tests/optim_ref.py (the numpy restatement the GPU optimiser tests compare with) against torch.optim.Adam + torch.nn.utils.clip_grad_norm_ in float64
on the CPU, to 1e-12 of each tensor's largest entry (the tolerance tests/test_diff_ref.py uses for its restatement); and its non-finite rule against
torch 1.7.1's, restated here because the installed torch behaves differently."""
import numpy as np
import pytest
import torch

import optim_ref as OR


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize('cap', [0.0, 1e6, 0.05, 3.0])
@pytest.mark.parametrize('grad_scale', [1.0, 1.0 / 3.0])
def test_adam_tail_matches_torch_float64(cap, grad_scale):
    rng = np.random.default_rng(int(cap * 100) + 7)
    shapes = [(37, 5), (5,), (1,), (64, 3)]
    n = sum(int(np.prod(s)) for s in shapes)
    params = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(s) * 0.1)) for s in shapes]
    opt = torch.optim.Adam(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, foreach=False)
    p = np.concatenate([q.detach().numpy().ravel() for q in params])
    m, v = np.zeros(n), np.zeros(n)
    for step in range(1, 8):
        g = rng.standard_normal(n) * 10.0 ** rng.uniform(-12, 2, n)
        g[rng.random(n) < 0.1] = 0.0
        off = 0
        for q in params:
            q.grad = torch.from_numpy(g[off:off + q.numel()].reshape(q.shape) * grad_scale)   # the scaled gradient is what torch clips and applies
            off += q.numel()
        norm_t = float(torch.cat([q.grad.flatten() for q in params]).norm())
        if cap > 0:
            torch.nn.utils.clip_grad_norm_(params, cap)
        opt.step()
        p, g1, m, v, norm, coef = OR.adam_tail(p, g, m, v, step, 1e-3, (0.9, 0.999), 1e-8, cap, grad_scale)
        assert abs(float(norm) - norm_t) <= 1e-12 * norm_t
        assert float(coef) == 1.0 if cap <= 0 or cap > norm_t else abs(float(coef) - cap / (norm_t + 1e-6)) <= 1e-12
        cat = lambda f: np.concatenate([f(q).numpy().ravel() for q in params])
        assert _rel(g1, cat(lambda q: q.grad)) <= 1e-12
        assert _rel(p, cat(lambda q: q.detach())) <= 1e-12, step
        assert _rel(m, cat(lambda q: opt.state[q]['exp_avg'])) <= 1e-12
        assert _rel(v, cat(lambda q: opt.state[q]['exp_avg_sq'])) <= 1e-12


def _clip_1_7_1(g, max_norm):
    """torch 1.7.1 clip_grad_norm_ (torch/nn/utils/clip_grad.py), the reference's pinned version, in three lines"""
    clip_coef = max_norm / (np.sqrt(np.sum(g * g)) + 1e-6)
    return g * clip_coef if clip_coef < 1 else g


@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf])
def test_non_finite_rule_is_torch_1_7_1(bad):
    rng = np.random.default_rng(3)
    g = rng.standard_normal(100)
    g[17] = bad
    with np.errstate(all='ignore'):
        want = _clip_1_7_1(g, 0.5)
        _, g1, m1, _, norm, coef = OR.adam_tail(np.zeros(100), g, np.zeros(100), np.zeros(100), 1, max_norm=0.5)
    assert np.array_equal(g1, want, equal_nan=True)
    if np.isnan(bad):                                            # NaN norm: nothing is clipped, the NaN stays where it was
        assert np.isnan(norm) and coef == 1.0
        assert np.array_equal(np.isnan(g1), np.arange(100) == 17) and np.array_equal(g1[np.arange(100) != 17], g[np.arange(100) != 17])
        assert np.array_equal(np.isnan(m1), np.arange(100) == 17)
    else:                                                        # infinite norm: coefficient 0 -- finite gradients vanish, inf * 0 = NaN
        assert np.isinf(norm) and coef == 0.0
        assert np.array_equal(np.isnan(g1), np.arange(100) == 17) and not g1[np.arange(100) != 17].any()
    # the installed torch clamps the coefficient and multiplies unconditionally: a NaN norm reaches every gradient (why the rule is written down)
    q = torch.nn.Parameter(torch.zeros(100, dtype=torch.float64))
    q.grad = torch.from_numpy(g.copy())
    torch.nn.utils.clip_grad_norm_([q], 0.5)
    if np.isnan(bad) and tuple(int(x) for x in torch.__version__.split('.')[:2]) >= (1, 10):
        assert bool(torch.isnan(q.grad).all())
    # without a cap nothing is touched at all
    with np.errstate(all='ignore'):
        _, g0, _, _, _, c0 = OR.adam_tail(np.zeros(100), g, np.zeros(100), np.zeros(100), 1, max_norm=0.0)
    assert c0 == 1.0 and np.array_equal(g0, g, equal_nan=True)


def test_float32_flavour_stays_float32_and_overflows_like_float32():
    g = np.full(10, 1e20, np.float32)
    z = np.zeros(10, np.float32)
    out32 = OR.adam_tail(z, g, z, z, 1, max_norm=2.0, dtype=np.float32)
    out64 = OR.adam_tail(z, g, z, z, 1, max_norm=2.0, dtype=np.float64)
    assert all(a.dtype == np.float32 for a in out32[:4]) and np.isinf(out32[4]) and out32[5] == 0.0 and not out32[1].any()
    assert np.isfinite(out64[4]) and 0 < out64[5] < 1
