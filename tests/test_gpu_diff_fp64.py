"""The differentiable MLP passes (csrc/diff_mlp.hip, layer_kernels.h, chain_x3.h) against the float64 restatement of tests/diff_ref.py, at the shapes
where the dispatch changes form: row counts on both sides of the one / two row-tile thresholds, hidden widths with full and partial 16-column tiles on
both chain forms of mv_chain_ntw (2 or 4 column tiles per wave), row windows that start off a 16-byte boundary, weight-gradient row counts around the
256-row chunks, features read through a misaligned column slice.

Error rule (tests/test_gpu_featext.py::_assert_close): for every output tensor, max |ours - fp64| <= 4 max |fp32 - fp64| + 1e-6 max |fp64|, where
fp32 is PyTorch's own fp32 CPU evaluation of the same formulas.

Every call is made twice and must return the same bits; one case per entry point runs with every buffer ops allocates filled with NaN (0xff for
the byte packs) first, and must return the same bits again: a kernel that read unwritten workspace, context or padding and relied on a zero weight
to cancel it would turn those into NaN.  One named exception: SECOND_ORDER_WGRAD.  Every test runs on both chain arithmetics ('x3': csrc/chain_x3.h; 'f32': the fp32-input MFMA chains)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import diff_ref as R
from helpers import dirty_allocations, sdf_packed_net
from mvsdf_amd import ops

pytestmark = pytest.mark.gpu

RATIOS = {}                       # (entry point, output kind) -> worst err / bound seen (MVSDF_DIFF_FP64_REPORT=path: written as JSON at the end)


@pytest.fixture(autouse=True, params=['x3', 'f32'])
def chain_arithmetic(request, monkeypatch):
    monkeypatch.setattr(ops, 'CHAIN_X3', request.param == 'x3')
    return request.param


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    path = os.environ.get('MVSDF_DIFF_FP64_REPORT')
    if path:
        with open(path, 'w') as f:
            json.dump({'%s/%s' % k: v for k, v in sorted(RATIOS.items())}, f, indent=1)


@pytest.fixture
def nan_workspace():
    """-> a context manager under which every CUDA tensor made by torch.empty / torch.empty_like (every output, context, workspace and pack that
    ops allocates) starts as all-ones bytes (helpers.dirty_allocations): NaN in every float type and in every bf16 term of a pack, -1 in the ints."""
    return lambda: dirty_allocations(0xff)


def _check(entry, kind, got, ref64, ref32, k32=4):
    got = got.detach().double().cpu()
    assert got.shape == ref64.shape, (entry, kind, tuple(got.shape), tuple(ref64.shape))
    if ref64.numel() == 0:
        return
    scale = float(ref64.abs().max())
    err = float((got - ref64).abs().max())
    e32 = float((ref32.double() - ref64).abs().max())
    bound = k32 * e32 + 1e-6 * scale
    RATIOS[(entry, kind)] = max(RATIOS.get((entry, kind), 0.0), err / bound if bound > 0 else (0.0 if err == 0 else math.inf))
    assert err <= bound, (entry, kind, err, e32, scale)


def _flat(out):
    """every tensor of a (nested) result, in order"""
    if torch.is_tensor(out):
        return [out]
    return [t for o in out if o is not None for t in _flat(o)]


def _twice(fn):
    """fn() twice: the same bits for every output tensor -> the first result"""
    a, b = fn(), fn()
    fa, fb = _flat(a), _flat(b)
    assert len(fa) == len(fb) and all(torch.equal(x, y) for x, y in zip(fa, fb)), 'two identical calls gave different bits'
    return a


def _same(a, b):
    fa, fb = _flat(a), _flat(b)
    assert len(fa) == len(fb) and all(torch.equal(x, y) for x, y in zip(fa, fb)), 'outputs change when the allocations start as NaN'


# ------------------------------------------------------------------------------------------------ SDF network
# name -> (hidden width, multires, skip_in, feature size).  mv_chain_ntw: widths <= 256 take 2 column tiles per wave (100: a partial tile), 300 / 384 /
# 512 take 4 (300: partial).  skip (3, 6) has two skip layers (fused chains only); (8,) skips into the last Linear.
NETS = {
    'w64': (64, 6, (4,), 32), 'w100': (100, 6, (4,), 256), 'w256': (256, 6, (4,), 256), 'w300': (300, 6, (4,), 32), 'w384': (384, 6, (4,), 0),
    'w512': (512, 6, (4,), 256), 'pe0': (64, 0, (4,), 32), 'pe10': (100, 10, (4,), 32), 'noskip': (64, 6, (), 256), 'skip36': (300, 6, (3, 6), 32),
    'skip8': (64, 6, (8,), 0), 'skip8pe10': (256, 10, (8,), 32),
}
_CACHE = {}


def _net_params(name):
    W, mr, skip, feat = NETS[name]
    key = ('p', name)
    if key not in _CACHE:
        _CACHE[key] = R.sdf_params(W, 100 + sorted(NETS).index(name), multires=mr, feat=feat, skip_in=skip)
    return _CACHE[key]


def _inputs(name, M):
    key = ('x', name, M)
    if key not in _CACHE:
        gen = torch.Generator().manual_seed(M * 31 + sorted(NETS).index(name))
        nout = 1 + NETS[name][3]
        x = torch.rand(M, 3, generator=gen) * 2.2 - 1.1
        _CACHE[key] = (x, torch.randn(M, nout, generator=gen) * 0.1, torch.randn(M, 3, generator=gen))
    return _CACHE[key]


def _fwd_ref(name, M):
    key = ('f', name, M)
    if key not in _CACHE:
        W, mr, skip, _ = NETS[name]
        x = _inputs(name, M)[0]
        _CACHE[key] = tuple(R.sdf_forward(_net_params(name), x, M, mr, skip, dt) for dt in (torch.float64, torch.float32))
    return _CACHE[key]


def _bwd_ref(name, M, row0, Mb, use_dn, dy=None):
    key = ('b', name, M, row0, Mb, use_dn, None if dy is None else float(dy.sum()))
    if key not in _CACHE:
        W, mr, skip, _ = NETS[name]
        x, dy0, dn = _inputs(name, M)
        dy = dy0[row0:row0 + Mb] if dy is None else dy
        dn = dn[row0:row0 + Mb] if use_dn else None
        _CACHE[key] = tuple(R.sdf_backward(_net_params(name), x, row0, dy, dn, mr, skip, dt) for dt in (torch.float64, torch.float32))
    return _CACHE[key]


def _packed(name):
    W, mr, skip, _ = NETS[name]
    return sdf_packed_net(R.state_dict(_net_params(name), 'implicit_network'), skip_layer=skip if skip else -1, multires=mr)


# Row counts of the fused chains (diff_mlp.hip): mv_chain_mt (fp32 chains, 2 column tiles per wave) takes two 16-row tiles per workgroup when
# 1.76 * ceil(t / 512) < ceil(t / 256) for t = ceil(M / 16) tiles, mv_chain_mt_x3 when 1.45 * ceil(t / 512) < ceil(t / 256):
#   M = 4096 (256 tiles): one tile on both;         4097 (257): two on both;
#   M = 8192 (512 tiles): two on both;              8193 (513): fp32 one (1.76 * 2 > 3), x3 two (1.45 * 2 < 3);
#   M = 12288 (768 tiles): fp32 one, x3 two;        12289 (769): two on both (1.76 * 2 < 4).
# 1, 15 and 17 rows: a single partial tile, and one full tile plus a one-row tile.
ROWS = [1, 15, 17, 4096, 4097, 8192, 8193, 12288, 12289]
FWD_CASES = [('w64', M, M) for M in ROWS] + [(n, 300, 300) for n in sorted(NETS)] + \
    [('w64', 300, Mg) for Mg in (0, 1, 17)] + [('w300', 300, Mg) for Mg in (0, 1, 17)] + [('w300', 4097, 4097), ('w256', 8193, 8193)]


@pytest.mark.parametrize('name,M,Mg', FWD_CASES, ids=['%s-M%d-Mg%d' % c for c in FWD_CASES])
def test_sdf_forward(name, M, Mg):
    net = _packed(name)
    x = _inputs(name, M)[0].cuda()
    y, n = _twice(lambda: ops.sdf_forward(net, x, Mg)[:2])          # (the context's padding is never written, so it is not compared)
    (y64, n64), (y32, n32) = _fwd_ref(name, M)
    _check('sdf_forward', 'y', y, y64, y32)
    _check('sdf_forward', 'n', n, n64[:Mg], n32[:Mg])


# The one exception to the rule: the weight and bias gradients of sdf_backward with the normals' upstream dn (autograd's double backward through
# sigma'(100 z) = 100 sigma (1 - sigma)) are held to 8 x the fp32 error instead of 4.  Measured on one MI355X at 4 x: err / bound 1.26 (dW, 8x64,
# 1 row: 4.4e-5 vs fp32 8.3e-6, largest entry 2.3), 1.29 (dW, 8x300, 1 row of 17 normals), 1.2 (dW, 8x384, 300 rows: 0.021 vs 0.0035 of 3524) on both
# chain arithmetics, and 1.24 (db, 8x64, 70 001 rows, x3 only: 8.6e-7 vs 8.1e-8 of 0.37); every other output kind stays below 0.95 of its 4 x bound.
SECOND_ORDER_WGRAD = 8

# (net, M, Mg of the forward, row0, Mb, with dn): full passes at every row count; row windows starting at 5 and 100 (H0 rows of 40 / 64 floats, hidden
# rows of 64 / 100 / 300: 5 is never 16-byte aligned); value-only passes over rows beyond the normals' prefix; 255 / 256 / 257 rows around one
# 256-row weight-gradient chunk and 70 001 rows (274 chunks, the last one partial).
BWD_CASES = [('w64', M, M, 0, M, True) for M in ROWS] + [(n, 300, 300, 0, 300, True) for n in sorted(NETS)] + \
    [(n, 300, 300, 5, 17, True) for n in ('w64', 'w100', 'w300', 'skip36', 'pe0')] + \
    [(n, 300, 300, 100, 150, False) for n in ('w64', 'w300', 'skip8', 'w512')] + \
    [('w64', 300, 17, 0, 17, True), ('w64', 300, 17, 0, 300, False), ('w300', 300, 1, 0, 1, True), ('w300', 300, 17, 5, 150, False)] + \
    [('w64', 300, 300, 0, Mb, True) for Mb in (255, 256, 257)] + [('w64', 70001, 70001, 0, 70001, True)]


@pytest.mark.parametrize('name,M,Mg,row0,Mb,use_dn', BWD_CASES, ids=['%s-M%d-Mg%d-r%d-Mb%d-%s' % (c[:5] + ('dn' if c[5] else 'nodn',)) for c in BWD_CASES])
def test_sdf_backward(name, M, Mg, row0, Mb, use_dn):
    net = _packed(name)
    x, dy, dn = (t.cuda() for t in _inputs(name, M))
    _, _, ctx = ops.sdf_forward(net, x, Mg)
    dyb, dnb = dy[row0:row0 + Mb].contiguous(), dn[row0:row0 + Mb].contiguous() if use_dn else None
    dWs, dbs, dx = _twice(lambda: ops.sdf_backward(net, x, M, Mg, Mb, dyb, dnb, ctx, True, row0=row0))
    (W64, b64, x64), (W32, b32, x32) = _bwd_ref(name, M, row0, Mb, use_dn)
    _check('sdf_backward', 'dx', dx, x64, x32)
    k32 = SECOND_ORDER_WGRAD if use_dn else 4
    for l in range(len(dWs)):
        _check('sdf_backward', 'dW', dWs[l], W64[l], W32[l], k32)
        _check('sdf_backward', 'db', dbs[l], b64[l], b32[l], k32)


# (net, M, row0X, MbX, row0D, MbD): pass A over all M rows with the normals' upstream, pass X over a window, the delta pass of the finish over another
PAIR_CASES = [('w64', 300, 5, 100, 100, 150), ('w64', 300, 0, 300, 0, 0), ('w300', 300, 5, 17, 17, 200), ('skip36', 300, 100, 200, 5, 100),
              ('w64', 4097, 5, 2000, 100, 3000), ('w256', 257, 1, 256, 0, 257)]


@pytest.mark.parametrize('name,M,row0X,MbX,row0D,MbD', PAIR_CASES, ids=['%s-M%d-X%d+%d-D%d+%d' % c for c in PAIR_CASES])
def test_sdf_backward_pair_finish(name, M, row0X, MbX, row0D, MbD):
    net = _packed(name)
    x, dy, dn = (t.cuda() for t in _inputs(name, M))
    _, _, ctx = ops.sdf_forward(net, x, M)
    dyX, dnX = (dy[row0X:row0X + MbX] * 0.5).contiguous(), (dn[row0X:row0X + MbX] * -2).contiguous()
    fbar = torch.randn(MbD, generator=torch.Generator().manual_seed(M + MbD)).cuda()
    dy2 = dy.clone()
    dy2[row0D:row0D + MbD, 0] += fbar

    def run():
        wsA, dxX = ops.sdf_backward_pair(net, M, M, M, dy, dn, row0X, MbX, dyX, dnX, ctx)
        dWs, dbs = ops.sdf_backward_finish(net, M, M, M, dy2, ctx, wsA, row0D, MbD, fbar)
        return dxX, dWs, dbs
    dxX, dWs, dbs = _twice(run)
    (_, _, x64), (_, _, x32) = (R.sdf_backward(_net_params(name), _inputs(name, M)[0], row0X, dyX.cpu(), dnX.cpu(), NETS[name][1], NETS[name][2], dt)
                                for dt in (torch.float64, torch.float32))
    _check('sdf_backward_pair', 'dx', dxX, x64, x32)
    (W64, b64, _), (W32, b32, _) = _bwd_ref(name, M, 0, M, True, dy=dy2.cpu())
    for l in range(len(dWs)):
        _check('sdf_backward_finish', 'dW', dWs[l], W64[l], W32[l])
        _check('sdf_backward_finish', 'db', dbs[l], b64[l], b32[l])


def test_sdf_entry_points_ignore_unwritten_allocations(nan_workspace):
    """sdf_forward / sdf_backward / the pair + finish on a partial-tile width with a row window: the same bits when every allocation starts as NaN
    (the network's packs included)."""
    name, M, row0, Mb = 'w300', 300, 5, 150
    x, dy, dn = (t.cuda() for t in _inputs(name, M))
    fbar = torch.linspace(-1, 1, 100).cuda()
    dy2 = dy.clone(); dy2[17:117, 0] += fbar

    def run():
        net = _packed(name)
        y, n, ctx = ops.sdf_forward(net, x, M)
        b = ops.sdf_backward(net, x, M, M, Mb, dy[row0:row0 + Mb].contiguous(), dn[row0:row0 + Mb].contiguous(), ctx, True, row0=row0)
        wsA, dxX = ops.sdf_backward_pair(net, M, M, M, dy, dn, row0, Mb, dy[row0:row0 + Mb].contiguous(), dn[row0:row0 + Mb].contiguous(), ctx)
        f = ops.sdf_backward_finish(net, M, M, M, dy2, ctx, wsA, 17, 100, fbar)
        return y, n, b, dxX, f
    ref = run()
    with nan_workspace():
        got = run()
    _same(got, ref)


# ------------------------------------------------------------------------------------------------ rendering network
RMODES = {'idr': 0, 'no_view_dir': 0x100, 'no_normal': 0x200}
# (hidden width, mode, feature size, rows of the backward N, rows of the forward context Nctx)
RENDER_CASES = [(64, 'idr', 256, 150, 200), (256, 'idr', 256, 150, 200), (512, 'idr', 256, 150, 200), (64, 'no_view_dir', 256, 100, 100),
                (64, 'no_normal', 32, 100, 117), (256, 'no_normal', 256, 17, 300), (64, 'idr', 256, 1, 15)] + \
    [(64, 'idr', 32, N, N) for N in (255, 256, 257)] + [(64, 'idr', 32, 70001, 70001)]


def _render_case(W, mode, feat, N, Nctx):
    key = ('r', W, mode, feat, N, Nctx)
    if key not in _CACHE:
        params = R.render_params(R.render_dims(W, 4, 4, feat, mode), 7 + W + feat)
        gen = torch.Generator().manual_seed(Nctx + feat)
        pts, view, nrm = (torch.randn(Nctx, 3, generator=gen) for _ in range(3))
        view = view / view.norm(dim=1, keepdim=True)
        ft = torch.randn(Nctx, feat, generator=gen)
        drgb = torch.randn(N, 3, generator=gen)
        refs = []
        for dt in (torch.float64, torch.float32):
            rgb = R.render_forward_backward(params, pts, view, nrm, ft, 4, mode, torch.zeros(Nctx, 3), dt)[0]
            refs.append((rgb,) + tuple(R.render_forward_backward(params, pts[:N], view[:N], nrm[:N], ft[:N], 4, mode, drgb, dt)[1:]))
        _CACHE[key] = (params, (pts, view, nrm, ft, drgb), refs)
    return _CACHE[key]


def _render_run(params, inputs, mode, N):
    """-> (rgb, dWs, dbs, din); features read through a column slice at column 1 of a [Nctx, feat + 3] tensor (rows misaligned by 4 bytes)"""
    pts, view, nrm, ft, drgb = (t.cuda() for t in inputs)
    net = sdf_packed_net(R.state_dict(params, 'rendering_network'), prefix='rendering_network', skip_layer=-1, multires=0)
    wide = torch.full((ft.shape[0], ft.shape[1] + 3), 1e30, device='cuda')
    wide[:, 1:1 + ft.shape[1]] = ft
    rgb, ctx = ops.render_forward(net, pts, view, nrm, wide[:, 1:1 + ft.shape[1]], 4 | RMODES[mode])
    dWs, dbs, din = ops.render_backward(net, N, drgb, ctx, n_ctx=ft.shape[0])
    return rgb, dWs, dbs, din


@pytest.mark.parametrize('W,mode,feat,N,Nctx', RENDER_CASES, ids=['w%d-%s-f%d-N%d-ctx%d' % c for c in RENDER_CASES])
def test_render_forward_backward(W, mode, feat, N, Nctx):
    params, inputs, ((rgb64, W64, b64, din64), (rgb32, W32, b32, din32)) = _render_case(W, mode, feat, N, Nctx)
    rgb, dWs, dbs, din = _twice(lambda: _render_run(params, inputs, mode, N))
    _check('render_forward', 'rgb', rgb, rgb64, rgb32)
    _check('render_backward', 'din', din, din64, din32)
    for l in range(len(dWs)):
        _check('render_backward', 'dW', dWs[l], W64[l], W32[l])
        _check('render_backward', 'db', dbs[l], b64[l], b32[l])


def test_render_ignores_unwritten_allocations(nan_workspace):
    params, inputs, _ = _render_case(64, 'no_normal', 32, 100, 117)
    ref = _render_run(params, inputs, 'no_normal', 100)
    with nan_workspace():
        got = _render_run(params, inputs, 'no_normal', 100)
    _same(got, ref)


# ------------------------------------------------------------------------------------------------ weight-norm fold backward
# (5, 575) / (5, 576) / (5, 577): the last K of k_fold_bwd_net's register path (K <= 576), with a partial and a full ninth chunk, and the first K of its
# strided path; (3, 640): ten full chunks on that path
FOLD_SHAPES = [(1, 3), (63, 39), (257, 289), (512, 512), (5, 575), (5, 576), (5, 577), (3, 640)]


def _fold_case(N, K):
    key = ('fold', N, K)
    if key not in _CACHE:
        gen = torch.Generator().manual_seed(N * 1000 + K)
        v = torch.randn(N, K, generator=gen) / math.sqrt(K)
        v[N // 2] *= 1e-5                                        # a row with a tiny |v| (dv ~ g / |v|: 1e5 times the others)
        g = torch.rand(N, 1, generator=gen) + 0.5
        dW = torch.randn(N, K, generator=gen)
        _CACHE[key] = (v, g, dW, [R.fold_backward(v, g, dW, dt) for dt in (torch.float64, torch.float32)])
    return _CACHE[key]


@pytest.mark.parametrize('N,K', FOLD_SHAPES, ids=['%dx%d' % s for s in FOLD_SHAPES])
def test_fold_backward(N, K):
    v, g, dW, ((dv64, dg64), (dv32, dg32)) = _fold_case(N, K)
    dv, dg = _twice(lambda: ops.fold_backward(v.cuda(), g.cuda(), dW.cuda()))
    _check('fold_backward', 'dv', dv, dv64, dv32)
    _check('fold_backward', 'dg', dg, dg64, dg32)


def test_fold_backward_net(nan_workspace):
    """all shapes in one launch, then again with every allocation poisoned"""
    cases = [_fold_case(N, K) for N, K in FOLD_SHAPES]
    run = lambda: ops.fold_backward_net([c[0].cuda() for c in cases], [c[1].cuda() for c in cases], [c[2].cuda() for c in cases])
    dvs, dgs = _twice(run)
    for (v, g, dW, ((dv64, dg64), (dv32, dg32))), dv, dg in zip(cases, dvs, dgs):
        _check('fold_backward_net', 'dv', dv, dv64, dv32)
        _check('fold_backward_net', 'dg', dg, dg64, dg32)
    with nan_workspace():
        got = run()
    _same(got, (dvs, dgs))


def test_fold_backward_net_adds_into_sinks():
    """The accumulating form (the parameters' .grad buffers as targets): every target starts from random values, one layer has no weight norm (g None:
    dv = dW, no dg), the bias gradients are routed to their targets.  Result = pre-fill + the gradient, held to the float64 sum under the file's rule (the
    kernel adds in float32)."""
    no_g = 2
    cases = [_fold_case(N, K) for N, K in FOLD_SHAPES]
    gen = torch.Generator().manual_seed(77)
    pre_v = [torch.randn(N, K, generator=gen) for N, K in FOLD_SHAPES]
    pre_g = [None if l == no_g else torch.randn(N, generator=gen) for l, (N, K) in enumerate(FOLD_SHAPES)]
    pre_b = [torch.randn(N, generator=gen) for N, K in FOLD_SHAPES]
    dbs = [torch.randn(N, generator=gen) for N, K in FOLD_SHAPES]
    vs, dWs = [c[0].cuda() for c in cases], [c[2].cuda() for c in cases]
    gs = [None if l == no_g else c[1].cuda() for l, c in enumerate(cases)]
    dbd = [d.cuda() for d in dbs]

    def run():
        tv, tb = [p.cuda() for p in pre_v], [p.cuda() for p in pre_b]
        tg = [None if p is None else p.cuda() for p in pre_g]
        assert ops.fold_backward_net(vs, gs, dWs, dbs=dbd, sinks=(tv, tg, tb)) is None
        return tv, tg, tb
    tv, tg, tb = _twice(run)
    for l, (v, g, dW, ((dv64, dg64), (dv32, dg32))) in enumerate(cases):
        if l == no_g:
            dv64, dv32 = dW.double(), dW
            assert tg[l] is None
        else:
            _check('fold_backward_net+', 'dg', tg[l], pre_g[l].double() + dg64.reshape(-1), pre_g[l] + dg32.reshape(-1))
        _check('fold_backward_net+', 'dv', tv[l], pre_v[l].double() + dv64, pre_v[l] + dv32)
        _check('fold_backward_net+', 'db', tb[l], pre_b[l].double() + dbs[l].double(), pre_b[l] + dbs[l])
