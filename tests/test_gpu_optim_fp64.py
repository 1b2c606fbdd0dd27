"""The optimiser tail (csrc/optim_kernels.hip: k_sqnorm_partials, k_adam_flat; mvsdf_amd/optim.py) against the float64 restatement of tests/optim_ref.py
(pinned to float64 torch by tests/test_optim_ref.py), called through lib().mvsdf_adam_step_fused on buffers this file owns: sizes on both sides of every
launch-shape edge (one workgroup, the partial loop's second trip at 64 workgroups, the 1024-workgroup cap and its longer grid stride), buffers that are
not 16-byte aligned (the scalar route), n < 4, every bias-correction regime, the clip coefficient's edges, non-finite gradients.

Error rule (tests/test_gpu_diff_fp64.py::_check): for every output tensor, max |ours - fp64| <= 4 max |fp32 - fp64| + 1e-6 max |fp64|, fp64 / fp32 being
optim_ref in the two dtypes from the same fp32 inputs.  The parameters start at ZERO, so p' is the update itself and its largest entry (about lr) is the
scale: elements whose gradient is at or below eps (where eps, the bias corrections and the clip coefficient's + 1e-6 decide the result) are then held to
~1e-9 of an update.  Norm and coefficient: 1e-6 relative against float64.  Gradients: normal sign / mantissa, magnitude 10^U(-12, 2), a block of exact zeros.

Every buffer, the workspace and norm_out sit between guard bands of NaN (checked by value afterwards: unchanged), and the workspace / norm_out start as
NaN: a read past n, or of an unwritten partial, reaches an output as NaN."""
import json
import math
import os

import numpy as np
import pytest
import torch

import optim_ref as OR
from mvsdf_amd._lib import lib, check
from mvsdf_amd.optim import FlatAdam
from mvsdf_amd.utils import synth

pytestmark = pytest.mark.gpu

RATIOS = {}                       # (case family, output) -> worst err / bound seen (MVSDF_OPTIM_FP64_REPORT=path: written as JSON at the end)
GUARD = 64                        # floats of NaN on both sides of every buffer (a multiple of 4: the band does not change the alignment)
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
BLOCK_ELEMS, BLOCKS_MAX = 2048, 1024      # launch shape of csrc/optim_kernels.hip: one workgroup per 2048 elements, at most 1024 workgroups
NET_SIZES = {W: sum(int(v.size) for v in synth.make_state_dict(W, 0).values()) for W in (64, 256, 512)}


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    path = os.environ.get('MVSDF_OPTIM_FP64_REPORT')
    if path:
        with open(path, 'w') as f:
            json.dump({'%s/%s' % k: v for k, v in sorted(RATIOS.items())}, f, indent=1)


def _blocks(n):
    return max(1, min(BLOCKS_MAX, (n + BLOCK_ELEMS - 1) // BLOCK_ELEMS))


def _log_uniform(rng, n, lo=-12.0, hi=2.0):
    """normal sign and mantissa, magnitude 10^U(lo, hi)"""
    mant, _ = np.frexp(rng.standard_normal(n))
    mant[mant == 0] = 0.5
    return (2.0 * mant * 10.0 ** rng.uniform(lo, hi, n)).astype(np.float32)


def _grad(rng, n):
    g = _log_uniform(rng, n)
    if n >= 8:
        g[n // 3:n // 3 + n // 8] = 0.0                          # a block of exact zeros
    return g


def _state(n, step, seed):
    """-> fp32 (p = 0, g, m, v): both moments zero at step 1; later m is zero on half the elements and log-uniform like g elsewhere, v = (|m| 10^U(-1,1))^2"""
    rng = np.random.default_rng(seed)
    g = _grad(rng, n)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    if step > 1:
        m = np.where(rng.random(n) < 0.5, 0.0, _log_uniform(rng, n)).astype(np.float32)
        v = ((np.abs(m.astype(np.float64)) * 10.0 ** rng.uniform(-1, 1, n)) ** 2).astype(np.float32)
    return np.zeros(n, np.float32), g, m, v


class _Banded:
    """n floats at `offset` floats past a 16-byte boundary, NaN bands on both sides"""

    def __init__(self, data, offset=0, n=None):
        n = data.size if data is not None else n
        self.whole = torch.full((GUARD + offset + n + GUARD + 4,), float('nan'), dtype=torch.float32, device='cuda')
        assert self.whole.data_ptr() % 16 == 0
        self.lo, self.hi = GUARD + offset, GUARD + offset + n
        self.view = self.whole[self.lo:self.hi]
        if data is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data)))

    def bands_untouched(self):
        return bool(torch.isnan(self.whole[:self.lo]).all()) and bool(torch.isnan(self.whole[self.hi:]).all())


def _launch(p, g, m, v, step, max_norm=0.0, grad_scale=1.0, zero_grad=0, offsets=(0, 0, 0, 0), ws_fill=float('nan'), lr=LR):
    """one mvsdf_adam_step_fused on fresh banded copies -> fp32 numpy (p', g', m', v', norm, coef)"""
    n = p.size
    bufs = [_Banded(a, o) for a, o in zip((p, g, m, v), offsets)]
    ws_n = int(lib().mvsdf_adam_ws_floats())
    assert ws_n >= _blocks(n)
    ws, no = _Banded(None, 0, ws_n), _Banded(None, 0, 2)
    ws.view.fill_(ws_fill); no.view.fill_(ws_fill)
    for b, o in zip(bufs, offsets):
        assert b.view.data_ptr() % 16 == 4 * o
    check(lib().mvsdf_adam_step_fused(bufs[0].view.data_ptr(), bufs[1].view.data_ptr(), bufs[2].view.data_ptr(), bufs[3].view.data_ptr(), n, lr, BETAS[0],
                                      BETAS[1], EPS, step, float(max_norm), float(grad_scale), int(zero_grad), no.view.data_ptr(), ws.view.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream), 'mvsdf_adam_step_fused')
    torch.cuda.synchronize()
    for b in bufs + [ws, no]:
        assert b.bands_untouched(), 'a guard band was written'
    assert not bool(torch.isnan(ws.view[:_blocks(n)]).any()) or not np.isfinite(g).all()
    out = [b.view.cpu().numpy().copy() for b in bufs]
    norm, coef = (float(x) for x in no.view.cpu().numpy())
    return out[0], out[1], out[2], out[3], np.float32(norm), np.float32(coef)


def _refs(p, g, m, v, step, max_norm=0.0, grad_scale=1.0, lr=LR):
    return tuple(OR.adam_tail(p, g, m, v, step, lr, BETAS, EPS, max_norm, grad_scale, dtype=dt) for dt in (np.float64, np.float32))


def _record(family, kind, err, bound):
    RATIOS[(family, kind)] = max(RATIOS.get((family, kind), 0.0), err / bound if bound > 0 else (0.0 if err == 0 else math.inf))
    print('%s/%s err %.3e bound %.3e ratio %.3f' % (family, kind, err, bound, err / bound if bound > 0 else 0.0))


def _check(family, kind, got, ref64, ref32, where=None):
    got, ref32 = np.asarray(got, np.float64), np.asarray(ref32, np.float64)
    if where is not None:
        got, ref64, ref32 = got[where], ref64[where], ref32[where]
    if ref64.size == 0:
        return
    assert not np.isnan(got).any(), (family, kind, 'NaN in an output')
    scale = float(np.abs(ref64).max())
    err, e32 = float(np.abs(got - ref64).max()), float(np.abs(ref32 - ref64).max())
    bound = 4 * e32 + 1e-6 * scale
    _record(family, kind, err, bound)
    assert err <= bound, (family, kind, err, e32, scale)


def _check_scalar(family, kind, got, ref64):
    err, bound = abs(float(got) - float(ref64)), 1e-6 * abs(float(ref64))
    _record(family, kind, err, bound)
    assert err <= bound, (family, kind, float(got), float(ref64))


def _check_all(family, got, r64, r32, zero_grad=False):
    for kind, a, b, c in zip(('p', 'g', 'm', 'v'), got, r64, r32):
        if kind == 'g' and zero_grad:
            assert not a.any()
        else:
            _check(family, kind, a, b, c)
    _check_scalar(family, 'norm', got[4], r64[4])
    _check_scalar(family, 'coef', got[5], r64[5])


def _bits_equal(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ 1. sizes
# workgroups = min(1024, ceil(n / 2048)): 1 up to 2048; 64 / 65 around 64 * 2048 (k_adam_flat's loop over the partials takes a second trip beyond 64);
# the three shipped networks (W = 512: 1424 > 1024, capped); 1024 * 2048 -+ (the cap's edge, a second grid-stride trip) and 3 * 1024 * 2048 + 5 (a third)
SIZES = [1, 2, 3, 4, 5, 7, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 64 * 2048 - 1, 64 * 2048, 64 * 2048 + 1,
         NET_SIZES[64], NET_SIZES[256], NET_SIZES[512], 1024 * 2048 - 1, 1024 * 2048, 1024 * 2048 + 1, 1024 * 2048 + 4, 3 * 1024 * 2048 + 5]


def test_network_sizes_are_the_shipped_ones():
    assert NET_SIZES == {64: 78140, 256: 802748, 512: 2915772}
    assert _blocks(NET_SIZES[256]) == 392 and _blocks(NET_SIZES[512]) == 1024 < (NET_SIZES[512] + 2047) // 2048
    assert [_blocks(n) for n in (1, 2048, 2049, 64 * 2048, 64 * 2048 + 1, 1024 * 2048, 1024 * 2048 + 1)] == [1, 1, 2, 64, 65, 1024, 1024]


@pytest.mark.parametrize('n', SIZES)
def test_sizes(n):
    for step, cap in ((1, 0.0), (10, 50.0)):
        st = _state(n, step, seed=n % 100003 + step)
        got = _launch(*st, step, max_norm=cap)
        _check_all('sizes', got, *_refs(*st, step, max_norm=cap))


# ------------------------------------------------------------------------------------------------ 2. steps
@pytest.mark.parametrize('step', [1, 2, 10, 1000, 200000])
@pytest.mark.parametrize('n', [2049, NET_SIZES[64]])
def test_steps(step, n):
    """bias corrections 1 - 0.9^t, sqrt(1 - 0.999^t) from 0.1 / 0.0316 (t = 1) to 1"""
    st = _state(n, step, seed=step % 977 + n)
    _check_all('steps', _launch(*st, step), *_refs(*st, step))
    _check_all('steps', _launch(*st, step, max_norm=0.5), *_refs(*st, step, max_norm=0.5))


# ------------------------------------------------------------------------------------------------ 3. clip
def _norm64(g, scale=1.0):
    return float(np.sqrt(np.sum(g.astype(np.float64) ** 2)) * scale)


@pytest.mark.parametrize('n', [2049, NET_SIZES[256]])
def test_clip_caps(n):
    st = _state(n, 10, seed=n + 5)
    norm = _norm64(st[1])
    ulp = float(np.spacing(np.float32(norm)))
    caps = [0.0, -1.0, 1e9 * norm, 1e-9 * norm, norm, norm - 3 * ulp, norm - ulp, norm + ulp, norm + 3 * ulp]
    ps = []
    for cap in caps:
        got = _launch(*st, 10, max_norm=cap)
        r64, r32 = _refs(*st, 10, max_norm=cap)
        _check_all('clip', got, r64, r32)
        assert abs(float(got[4]) - norm) <= 1e-6 * norm
        if cap <= 0 or cap > 2 * norm:
            assert float(got[5]) == 1.0                          # no cap / a cap far above: the coefficient is exactly 1
            assert _bits_equal(got[1:2], st[1:2])                # and the gradient comes back as it went in
        ps.append(got[0].astype(np.float64))
    # the coefficient is continuous at cap = norm: nothing jumps across the five caps around it
    scale = np.abs(ps[4]).max()
    for q in ps[5:]:
        assert np.abs(q - ps[4]).max() <= 1e-5 * scale


@pytest.mark.parametrize('target', [1e-5, 1e-6])
def test_clip_small_norm(target):
    """a gradient of norm ~1e-5 / ~1e-6 under a cap of 1e-6: the coefficient's + 1e-6 is a tenth / half of its denominator"""
    n = 2049
    rng = np.random.default_rng(11)
    g = (rng.standard_normal(n) * target / math.sqrt(n)).astype(np.float32)
    z = np.zeros(n, np.float32)
    for step in (1, 10):
        got = _launch(z, g, z, z, step, max_norm=1e-6)
        r64, r32 = _refs(z, g, z, z, step, max_norm=1e-6)
        _check_all('clip_small', got, r64, r32)
        assert abs(float(r64[5]) - 1e-6 / (_norm64(g) + 1e-6)) < 1e-12 and 0.05 < float(r64[5]) < 0.6


@pytest.mark.parametrize('scale', [1.0, 0.5, 1.0 / 3.0, 1.0 / 6.0, 1.0 / 8.0])
@pytest.mark.parametrize('cap', [0.0, 2.0])
def test_grad_scale(scale, cap):
    n = NET_SIZES[64]
    st = _state(n, 10, seed=int(scale * 1000))
    got = _launch(*st, 10, max_norm=cap, grad_scale=scale)
    r64, r32 = _refs(*st, 10, max_norm=cap, grad_scale=scale)
    _check_all('grad_scale', got, r64, r32)
    assert abs(float(got[4]) - _norm64(st[1], scale)) <= 1e-6 * _norm64(st[1], scale)      # norm_out[0] = norm * grad_scale


# ------------------------------------------------------------------------------------------------ 4. alignment
OFFSETS = [(o, o, o, o) for o in (1, 2, 3)] + [(0, o, 0, 0) for o in (1, 2, 3)]


@pytest.mark.parametrize('n', [1, 2, 3, 5, 2049, NET_SIZES[256]])
def test_alignment(n):
    """The scalar route (any buffer off a 16-byte boundary) does the same per-element arithmetic as the float4 route: identical bits.  n < 4 also runs
    aligned, where the float4 prefetch of k_adam_flat loads 16 bytes at index 0 of buffers shorter than that: the NaN bands sit right behind the n
    floats, so anything of that load reaching an output would show."""
    st = _state(n, 10, seed=n + 77)
    base = _launch(*st, 10, max_norm=0.5)
    _check_all('alignment', base, *_refs(*st, 10, max_norm=0.5))
    for offs in OFFSETS:
        got = _launch(*st, 10, max_norm=0.5, offsets=offs)
        assert all(not np.isnan(a).any() for a in got[:4])
        assert _bits_equal(got, base), ('scalar route != float4 route', n, offs)


# ------------------------------------------------------------------------------------------------ 5. zero_grad
@pytest.mark.parametrize('n', [5, 2049, NET_SIZES[512]])
@pytest.mark.parametrize('offs', [(0, 0, 0, 0), (1, 1, 1, 1)])
def test_zero_grad(n, offs):
    st = _state(n, 2, seed=n + 9)
    keep = _launch(*st, 2, max_norm=0.5, offsets=offs)
    zero = _launch(*st, 2, max_norm=0.5, offsets=offs, zero_grad=1)
    assert not zero[1].any() and np.array_equal(np.signbit(zero[1]), np.zeros(n, bool))
    assert _bits_equal(keep[:1] + keep[2:], zero[:1] + zero[2:])
    _check_all('zero_grad', zero, *_refs(*st, 2, max_norm=0.5), zero_grad=True)


# ------------------------------------------------------------------------------------------------ 6. repeatability, 7. workspace hygiene
@pytest.mark.parametrize('n,offs', [(3 * 1024 * 2048 + 5, (0, 0, 0, 0)), (NET_SIZES[256], (0, 3, 0, 0))])
def test_same_bits_twice_and_with_any_workspace_content(n, offs):
    """fixed-order sums: the same call from the same state gives the same bits; and neither the workspace nor norm_out is read before it is written
    (NaN-filled, zero-filled and 1e30-filled workspaces give the same bits)"""
    st = _state(n, 10, seed=n % 1000)
    a = _launch(*st, 10, max_norm=0.5, offsets=offs)
    b = _launch(*st, 10, max_norm=0.5, offsets=offs)
    assert _bits_equal(a, b)
    for fill in (0.0, 1e30):
        assert _bits_equal(a, _launch(*st, 10, max_norm=0.5, offsets=offs, ws_fill=fill))


# ------------------------------------------------------------------------------------------------ 8. non-finite gradients
@pytest.mark.parametrize('cap', [0.0, 0.5])
@pytest.mark.parametrize('bad', ['nan', 'inf', 'overflow'])
def test_non_finite_gradients(bad, cap):
    """Ordinary floating-point inputs.  The rule (optim_ref.clip_coefficient, torch 1.7.1): the coefficient applies only when coef < 1, so a NaN norm clips
    nothing and the NaN stays in its own element; an infinite norm gives coef = 0.  Compared with optim_ref's FLOAT32 flavour: its sum of squares overflows
    like the kernel's (1e20^2 = inf in fp32, finite in float64), so norm / coef / the finite pattern are the float32 flavour's, exactly; the elements that
    stay finite are held to the usual bound against float64 run with the float32 flavour's coefficient."""
    n = 2049
    p, g, m, v = _state(n, 10, seed=31)
    if bad == 'nan':
        g[700] = np.nan
    elif bad == 'inf':
        g[700] = np.inf
    else:
        g[700], g[1500] = 1e20, -1e20
    got = _launch(p, g, m, v, 10, max_norm=cap)
    _, r32 = _refs(p, g, m, v, 10, max_norm=cap)
    assert np.array_equal(np.float32(got[4]), np.float32(r32[4]), equal_nan=True), (got[4], r32[4])
    assert float(got[5]) == float(r32[5])
    with np.errstate(all='ignore'):
        # float64 restatement under the float32 flavour's clip decision (with an overflowed fp32 norm the float64 norm is finite and would clip differently)
        g_eff = g.astype(np.float64) * float(r32[5])
        r64 = OR.adam_tail(p, g_eff, m, v, 10, LR, BETAS, EPS, 0.0, 1.0)
    for kind, a, b64, b32 in zip(('p', 'g', 'm', 'v'), got, r64, r32):
        fin = np.isfinite(b32)
        assert np.array_equal(np.isfinite(a), fin), (kind, 'finite pattern differs')
        assert np.array_equal(np.isnan(a), np.isnan(b32)), (kind, 'NaN pattern differs')
        assert fin.sum() >= n - 2
        _check('non_finite', kind, a, b64, b32, where=fin)


# ------------------------------------------------------------------------------------------------ 9. several steps at a real size
def test_fifty_steps_w256():
    """The one case where error may compound: 50 steps at the W = 256 size, a fresh gradient per step, grad_cap on, p from zero; the kernel's fp32 state
    against optim_ref float64 carried forward in float64, optim_ref float32 carried alongside for the fp32 error; checked at steps 1, 2, 10 and 50."""
    n = NET_SIZES[256]
    rng = np.random.default_rng(256)
    z = np.zeros(n, np.float32)
    k, s64, s32 = (z, z, z), (z.astype(np.float64),) * 3, (z, z, z)            # (p, m, v)
    for step in range(1, 51):
        g = _grad(rng, n)
        got = _launch(k[0], g, k[1], k[2], step, max_norm=2.0)
        r64 = OR.adam_tail(s64[0], g, s64[1], s64[2], step, LR, BETAS, EPS, 2.0, 1.0, dtype=np.float64)
        r32 = OR.adam_tail(s32[0], g, s32[1], s32[2], step, LR, BETAS, EPS, 2.0, 1.0, dtype=np.float32)
        k, s64, s32 = (got[0], got[2], got[3]), (r64[0], r64[2], r64[3]), (r32[0], r32[2], r32[3])
        if step in (1, 2, 10, 50):
            _check_all('fifty_steps@%d' % step, got, r64, r32)


# ------------------------------------------------------------------------------------------------ the Python layer
def _flat_adam_w512():
    from mvsdf_amd.model.implicit_differentiable_renderer import IDRNetwork
    from mvsdf_amd.utils.config import ConfigDict
    model = IDRNetwork(ConfigDict(synth.model_conf(512)))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(512, 0).items()})
    model = model.cuda()
    return model, FlatAdam(model.parameters(), lr=LR)


def _check_update(family, p0, p1, r64, r32):
    """p != 0 here, so the update p' - p is compared (in float64 from the fp32 before / after values).  The kernel rounds p - update to fp32 once: half an
    ulp of max |p| on top of the usual bound on the update, whose scale is max |update|; the float32 flavour's error is taken on its own update
    likewise (it contains the same final rounding, so the half ulp is not counted twice beyond the factor 4)."""
    up, u64, u32 = p1.astype(np.float64) - p0, r64 - p0.astype(np.float64), r32.astype(np.float64) - p0
    err, e32 = float(np.abs(up - u64).max()), float(np.abs(u32 - u64).max())
    bound = 4 * e32 + 1e-6 * float(np.abs(u64).max()) + 0.5 * float(np.spacing(np.float32(np.abs(p0).max())))
    _record(family, 'update', err, bound)
    assert err <= bound, (family, err, e32)


@pytest.mark.parametrize('cap', [None, 0.5])
def test_flat_adam_one_step_on_the_w512_network(cap):
    model, opt = _flat_adam_w512()
    n = opt.flat_p.numel()
    assert n == NET_SIZES[512] and sum(c for _, c in opt._slices) == n
    g = _grad(np.random.default_rng(512), n)
    opt.flat_g.copy_(torch.from_numpy(g))
    p0 = opt.flat_p.cpu().numpy().copy()
    opt.step(grad_cap=cap)
    z = np.zeros(n, np.float32)
    r64, r32 = _refs(p0, g, z, z, 1, max_norm=cap or 0.0)
    _check_update('flat_adam', p0, opt.flat_p.cpu().numpy(), r64[0], r32[0])
    for kind, a, i in (('g', opt.flat_g, 1), ('m', opt.flat_m, 2), ('v', opt.flat_v, 3)):
        _check('flat_adam', kind, a.cpu().numpy(), r64[i], r32[i])
    _check_scalar('flat_adam', 'norm', opt.norm_and_coef[0], r64[4])
    _check_scalar('flat_adam', 'coef', opt.norm_and_coef[1], r64[5])
    # the Parameters are views of the flat buffer, in order: the step reached every one of them
    off = 0
    for q in model.parameters():
        assert torch.equal(q.detach().reshape(-1), opt.flat_p[off:off + q.numel()])
        off += q.numel()


def test_flat_adam_after_loading_a_torch_adam_checkpoint_at_step_1000():
    model, opt = _flat_adam_w512()
    n = opt.flat_p.numel()
    _, g, m, v = _state(n, 1001, seed=1001)
    params = list(model.parameters())
    ref_opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros_like(q)) for q in params], lr=LR)
    off = 0
    for q in ref_opt.param_groups[0]['params']:
        c = q.numel()
        ref_opt.state[q] = {'step': torch.tensor(1000.0), 'exp_avg': torch.from_numpy(m[off:off + c]).view(q.shape).cuda(),
                            'exp_avg_sq': torch.from_numpy(v[off:off + c]).view(q.shape).cuda()}
        off += c
    opt.load_state_dict(ref_opt.state_dict())
    assert opt._t == 1000
    assert np.array_equal(opt.flat_m.cpu().numpy(), m) and np.array_equal(opt.flat_v.cpu().numpy(), v)
    opt.flat_g.copy_(torch.from_numpy(g))
    p0 = opt.flat_p.cpu().numpy().copy()
    opt.step(grad_cap=2.0)
    r64, r32 = _refs(p0, g, m, v, 1001, max_norm=2.0)
    _check_update('flat_adam_ckpt', p0, opt.flat_p.cpu().numpy(), r64[0], r32[0])
    for kind, a, i in (('m', opt.flat_m, 2), ('v', opt.flat_v, 3)):
        _check('flat_adam_ckpt', kind, a.cpu().numpy(), r64[i], r32[i])
