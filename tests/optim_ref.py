"""Plain numpy restatement of the optimiser tail of one training step (reference code/training/idr_train.py:289-302 with its pinned torch 1.7.1):

    all_norm = ||grad||_2 ; clip_grad_norm_(params, grad_cap) ; Adam.step()

on flat arrays, in ONE chosen dtype (float64: the reference of tests/test_gpu_optim_fp64.py; float32: the same formulas at the kernel's precision, whose
distance from float64 sizes that test's bound).  It keeps the operation order of csrc/optim_kernels.hip and nothing else of it: no blocks, no partial sums,
no float-rounded betas -- `1 - beta` and both bias corrections are formed in double from the Python floats and rounded once to the dtype.

torch 1.7.1, torch/nn/utils/clip_grad.py::clip_grad_norm_:
    clip_coef = max_norm / (total_norm + 1e-6)
    if clip_coef < 1:
        for p in parameters: p.grad.detach().mul_(clip_coef)
torch 1.7.1, torch/optim/_functional.py::adam (weight_decay = 0, amsgrad = False):
    exp_avg.mul_(beta1).add_(grad, alpha=1 - beta1)                    (here in the lerp form m + (g - m)(1 - beta1), the kernel's)
    exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    denom = (exp_avg_sq.sqrt() / math.sqrt(bias_correction2)).add_(eps)
    param.addcdiv_(exp_avg, denom, value=-(lr / bias_correction1))

THE NON-FINITE RULE (`clip_coefficient`, the one place that states it): the coefficient is applied only when `coef < 1`.  A NaN norm makes that
comparison false, so a step whose gradient holds a NaN clips NOTHING and the NaN stays in its own elements (and in the moments / parameters they update);
an infinite norm gives coef = 0, which zeroes every finite gradient and turns the infinite ones into NaN.  That is torch 1.7.1's `if clip_coef < 1:`;
torch >= 1.10 multiplies every gradient by clamp(clip_coef, max=1.0) instead, which spreads a NaN norm over all of them."""
import math

import numpy as np


def clip_coefficient(norm, max_norm, dtype=np.float64):
    """-> the factor every gradient is multiplied by (1 = untouched).  max_norm <= 0: no clipping."""
    dt = np.dtype(dtype).type
    if not max_norm > 0:
        return dt(1.0)
    with np.errstate(all='ignore'):
        coef = dt(max_norm) / (dt(norm) + dt(1e-6))
    return coef if coef < 1 else dt(1.0)                         # torch 1.7.1: `if clip_coef < 1:` -- false for NaN


def adam_tail(p, g, m, v, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_norm=0.0, grad_scale=1.0, dtype=np.float64):
    """-> (p', g', m', v', norm, coef): norm = ||g * grad_scale||, g' = the scaled / clipped gradient, step >= 1 = Adam's count AFTER this update."""
    dt = np.dtype(dtype).type
    p, g, m, v = (np.asarray(a).astype(dtype) for a in (p, g, m, v))
    b1, b2 = float(betas[0]), float(betas[1])
    one_m_b1, one_m_b2 = dt(1.0 - b1), dt(1.0 - b2)
    bc1 = dt(1.0 - b1 ** step)
    bc2_sqrt = dt(math.sqrt(1.0 - b2 ** step))
    with np.errstate(all='ignore'):
        norm = np.sqrt(np.sum(g * g, dtype=dtype)) * dt(grad_scale)
        coef = clip_coefficient(norm, max_norm, dtype)
        g1 = g * dt(grad_scale) * coef
        m1 = m + (g1 - m) * one_m_b1
        v1 = v * dt(b2) + one_m_b2 * g1 * g1
        denom = np.sqrt(v1) / bc2_sqrt + dt(eps)
        p1 = p - (dt(lr) / bc1) * (m1 / denom)
    assert all(a.dtype == np.dtype(dtype) for a in (p1, g1, m1, v1)) and norm.dtype == np.dtype(dtype)
    return p1, g1, m1, v1, norm, coef
