"""The weight gradients in the three-term bf16 arithmetic (csrc/wgrad_x3.h: k_wgrad_net_x3) beside the fp32-input form (layer_kernels.h: k_wgrad_net), both
reached in one process through ops.set_wgrad_x3, at the edges of the new kernel:
  * rows of the contraction around one matrix instruction (32), the kernel's stage depth S (mvsdf_wgrad_x3_stage_rows, read from the library) and the
    256-row chunks, full passes and row windows starting at row 5 (no 16-byte alignment), with and without the normals' upstream (one or two operand pairs);
  * columns: partial 16-column tiles (width 100), a partial 128 x 128 block (width 300), the last layer's 257 outputs, first layers of 3 / 39 / 63 inputs,
    skips into other layers, the rendering net (single pair, no SDF descriptor: only the setter reaches the three-term form there).
Every dW / db is held to the float64 restatement of tests/diff_ref.py by the rule of tests/test_gpu_diff_fp64.py (err <= k |fp32 - fp64|max + 1e-6 |fp64|max,
k = 4, SECOND_ORDER_WGRAD = 8 with the normals' upstream); every call is made twice and returns the same bits; one SDF and one rendering case run again with
every allocation poisoned (NaN / 0xff).  Last: a native training step whose true row count is no multiple of 32 and leaves a whole chunk empty gives the same
gradient bits with device-side counts (deferred) as with host counts (classic), the three-term form on."""
import pytest
import torch

import test_gpu_deferred as DEF
import test_gpu_diff_fp64 as D
from test_gpu_diff_fp64 import nan_workspace  # noqa: F401  (the fixture: every torch.empty allocation starts as NaN / 0xff)
from mvsdf_amd import ops

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=['x3', 'f32'])
def wgrad_form(request):
    ops.set_wgrad_x3(request.param == 'x3')
    yield request.param
    ops.set_wgrad_x3(None)


def _rows(label):
    S = ops.wgrad_x3_stage_rows()
    return {'S-1': S - 1, 'S': S, 'S+1': S + 1}.get(label, label)


def _sdf_case(name, M, row0, Mb, use_dn, run_twice=True):
    """sdf_backward over rows [row0, row0 + Mb) of an M-row forward -> (dWs, dbs), checked against float64"""
    net = D._packed(name)
    x, dy, dn = (t.cuda() for t in D._inputs(name, M))
    _, _, ctx = ops.sdf_forward(net, x, M)
    dyb, dnb = dy[row0:row0 + Mb].contiguous(), dn[row0:row0 + Mb].contiguous() if use_dn else None
    run = lambda: ops.sdf_backward(net, x, M, M, Mb, dyb, dnb, ctx, True, row0=row0)[:2]
    dWs, dbs = D._twice(run) if run_twice else run()
    (W64, b64, _), (W32, b32, _) = D._bwd_ref(name, M, row0, Mb, use_dn)
    k32 = D.SECOND_ORDER_WGRAD if use_dn else 4
    for l in range(len(dWs)):
        D._check('wgrad_x3_sdf', 'dW', dWs[l], W64[l], W32[l], k32)
        D._check('wgrad_x3_sdf', 'db', dbs[l], b64[l], b32[l], k32)
    return dWs, dbs


# ---- 1. row edges of the contraction
ROW_LABELS = [1, 31, 32, 33, 'S-1', 'S', 'S+1', 255, 256, 257, 513]


@pytest.mark.parametrize('use_dn', [True, False], ids=['dn', 'nodn'])
@pytest.mark.parametrize('row0', [0, 5])
@pytest.mark.parametrize('label', ROW_LABELS, ids=[str(r) for r in ROW_LABELS])
def test_row_edges(label, row0, use_dn):
    _sdf_case('w64', 520, row0, _rows(label), use_dn)


# ---- 2. column edges
@pytest.mark.parametrize('name,Mb', [('w100', 300), ('w300', 300), ('pe0', 300), ('pe10', 300), ('skip8', 33), ('skip36', 33)])
def test_column_edges_sdf(name, Mb):
    dWs, _ = _sdf_case(name, 300, 0, Mb, True)
    if name == 'w100':
        assert dWs[-1].shape[0] == 257 and dWs[1].shape == (100, 100)
    if name == 'pe0':
        assert dWs[0].shape[1] == 3
    if name == 'pe10':
        assert dWs[0].shape[1] == 63


def _render_check(N, run_twice=True):
    params, inputs, ((_, W64, b64, _), (_, W32, b32, _)) = D._render_case(64, 'idr', 32, N, N)
    run = lambda: D._render_run(params, inputs, 'idr', N)[1:3]
    dWs, dbs = D._twice(run) if run_twice else run()
    for l in range(len(dWs)):
        D._check('wgrad_x3_render', 'dW', dWs[l], W64[l], W32[l])
        D._check('wgrad_x3_render', 'db', dbs[l], b64[l], b32[l])
    return dWs, dbs


@pytest.mark.parametrize('N', [1, 33, 257])
def test_column_edges_render(N):
    _render_check(N)


# ---- 4. unwritten memory
def test_sdf_ignores_unwritten_allocations(nan_workspace):  # noqa: F811
    ref = _sdf_case('w300', 300, 5, 257, True)
    with nan_workspace():
        got = _sdf_case('w300', 300, 5, 257, True, run_twice=False)
    D._same(got, ref)


def test_render_ignores_unwritten_allocations(nan_workspace):  # noqa: F811
    ref = _render_check(257)
    with nan_workspace():
        got = _render_check(257, run_twice=False)
    D._same(got, ref)


# ---- 5. device-side row counts
def test_deferred_step_equals_classic_with_empty_chunks(wgrad_form):
    """2 x 175 rays, width 64: the SDF layers' weight gradients cover E + N rows (E = 175 eikonal points + N hits, about nine rays in ten) of at most E + 350 = 525
    -- the deferred step sizes the launch for that bound (three chunks) and the workgroups of the chunk beyond the true rows return at once.  (2 x 100 rays: 280 true
    rows of at most 300, no empty chunk.)"""
    o, _, g = DEF._compare(W=64, B=2, P=175)
    n_hit = int(o['network_object_mask'].sum())
    rays = o['network_object_mask'].numel()
    true_rows = o['grad_theta'].shape[0]
    bound = true_rows - n_hit + rays
    assert true_rows % 32 != 0 and (true_rows + 255) // 256 < (bound + 255) // 256, (true_rows, bound)
    assert float(g.abs().max()) > 0
