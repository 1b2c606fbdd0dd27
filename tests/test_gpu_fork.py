"""GPU (pytest -m gpu): the fork of a forward with the sphere cut (csrc/step_driver.hip: mvsdf_step_set_fork; csrc/trace.hip: k_row_chunks, mvsdf_trace_rows_stage)
against the launches it replaces.  The reference is always the existing launch -- k_ray_samples<2, 2, 8> over the SAME lists, the step with all three parts off --
never the new code.

  1. The sixteen-wave rows form alone.  The limited sphere launch and its resume launch run once per (network, rays, limit); the workspace, the counters and the outputs
     they leave are the common start of every pass.  From there mvsdf_trace_stage 3 + mvsdf_trace_cut_stage 3 (the reference) and mvsdf_trace_rows_stage 1 + 2 with
     grid caps 1, 2 and none: the first sampler window of nf = 12 samples over the first list, the single pass of 100 samples over the late list.  Compared byte for
     byte: both sample-value buffers, points / masks / dists after the reductions; as sorted sets with what belongs to their rays: the rest list and the secant list;
     the counters 0-8 and 13-15.  W = 64 (four column tiles on sixteen waves: twelve waves without a tile) and W = 256, the three-weight-term engine; 8 / 24 / 64 /
     257 rays under limits 1, 2 (nearly every ray spills: a long late list) and st_iters + 1; an empty late list (limit 1000: every workgroup leaves).
  2. The step: the cut forced on with a limit of 2 rounds (the late branch has the rows) and with the step's own limit (the windows have them), each part alone and all three forced on against all three off: every entry of
     the output dict, the six losses, every gradient entry, both call orders; `points` / `sdf_output` resolved after three further optimiser steps; the count record
     of the host ring against the forward block's; MVSDF_FORK=0: the launches of the step without the fork (last tracer grid, counters)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from helpers import sdf_packed_net, t, trace_params
from mvsdf_amd import ops
from mvsdf_amd.model.implicit_differentiable_renderer import IDRNetwork
from mvsdf_amd.model.loss import IDRLoss
from mvsdf_amd.optim import FlatAdam
from mvsdf_amd.utils import synth
from mvsdf_amd.utils.config import ConfigDict

pytestmark = pytest.mark.gpu

N_SPILL, N_LATE = 13, 14                                          # include/mvsdf_hip.h MVSDF_CNT_N_SPILL, MVSDF_CNT_N_SAMPLER_LATE
N_MISS = 3                                                        # rays at the front of every batch that miss the sphere
NF = 12                                                           # the first sampler window (csrc/trace_route.h: MvTraceSwitches.nfirst)
ST_ITERS = trace_params(64)[4]
LIMITS = {'one': 1, 'two': 2, 'step': ST_ITERS + 1}
CAPS = (1, 2, 0)
CNT_COMPARED = list(range(9)) + [13, 14, 15]
# the step: without counters[15], "evaluations the slowest resume workgroup still ran" -- the resume launch groups the spilled rays in arrival order, and how many rounds
# a group shares depends on its members: the figure differs between two runs of the SAME launches (the rows tests above share one resume launch and do compare it)
CNT_STEP = list(range(9)) + [13, 14]


@functools.lru_cache(maxsize=None)
def _net(W):
    return ops.pack_trace_net(sdf_packed_net(synth.make_state_dict(W, 0)), 'f32x3')


@functools.lru_cache(maxsize=None)
def _rays(R):
    """the rays of tests/test_gpu_sphere_cut.py: one view, the first N_MISS turned past the sphere; object mask ~70 % true; shared, never modified"""
    inp, _ = synth.make_batch(1, R, 0, seed=100 + R, with_features=False, focal_scale=1.4)
    dirs, cam = ops.camera_rays(t(inp['uv']), t(inp['pose']), t(inp['intrinsics']))
    dirs = dirs.clone()
    for i in range(N_MISS):
        e = torch.zeros(3, device='cuda'); e[i] = 1.0
        v = torch.linalg.cross(cam[0], e)
        dirs[0, i] = v / v.norm()
    rs = np.random.RandomState(R)
    om = t((rs.uniform(size=R) < 0.7).astype(np.uint8))
    steps = t(rs.uniform(size=trace_params(64)[5]).astype(np.float32))
    return cam.contiguous(), dirs.contiguous(), om, steps


@functools.lru_cache(maxsize=None)
def _sampler_rays_uncut(W, R):
    """sampler rays of the batch under the uncut sphere launch (mvsdf_trace_stage 1): a batch without any has none for a late list either"""
    from mvsdf_amd._lib import check, lib
    s = _start(W, R, 1000)
    b = _Bufs(s)
    check(lib().mvsdf_trace_stage(1, *s.args(b)), 'mvsdf_trace_stage(1)')
    torch.cuda.synchronize()
    return int(b.cnt[5])


def _offsets(R, n):
    """byte offsets of the regions the comparison reads (csrc/trace_route.h: mv_trace_ws, and mv_trace_cut_ws behind it)"""
    r = 4 * R
    base = (r * (11 + 2 * n) + 256 + 255) & ~255
    return dict(w_zmin=0, w_zmax=r, sec_state=2 * r, w_list=6 * r, sec_list=8 * r, sv=9 * r, list_rest=(9 + n) * r, src_rest=(10 + n) * r,
                list_late=base + 16 * r, sv_late=base + 17 * r)


class _Start:
    """what the limited sphere launch and its resume launch left: the common start of every rows pass (never modified: every pass works on clones)"""

    def __init__(self, W, R, limit):
        from mvsdf_amd._lib import TraceParams, check, lib
        self.W, self.R = W, R
        self.tp = TraceParams(*trace_params(W))
        self.n = n = self.tp.n_steps
        assert n == 100 and NF < n
        self.iv = torch.linspace(0, 1, n).cuda()
        self.pts = torch.zeros(R, 3, device='cuda'); self.mask = torch.zeros(R, dtype=torch.uint8, device='cuda'); self.dists = torch.zeros(R, device='cuda')
        self.cnt = torch.zeros(16, dtype=torch.int64, device='cuda')
        self.wsb = lib().mvsdf_trace_cut_workspace_bytes(R, n)
        self.ws = torch.zeros(self.wsb, dtype=torch.uint8, device='cuda')
        for stage, rounds in ((1, limit), (2, 0)):
            check(lib().mvsdf_trace_cut_stage(stage, rounds, *self.args(self)), 'mvsdf_trace_cut_stage(%d)' % stage)
        torch.cuda.synchronize()

    def args(self, bufs):
        from mvsdf_amd._lib import ptr, stream_of
        cam, dirs, om, steps = _rays(self.R)
        return (C.byref(_net(self.W).desc()), C.byref(self.tp), ptr(cam), ptr(dirs), ptr(om), 1, self.R, 1, ptr(self.iv), ptr(steps), ptr(bufs.pts), ptr(bufs.mask),
                ptr(bufs.dists), ptr(bufs.cnt), ptr(bufs.ws), C.c_size_t(self.wsb), 1, 4, stream_of(dirs))


@functools.lru_cache(maxsize=None)
def _start(W, R, limit):
    return _Start(W, R, limit)


class _Bufs:
    def __init__(self, s):
        self.pts, self.mask, self.dists, self.cnt, self.ws = s.pts.clone(), s.mask.clone(), s.dists.clone(), s.cnt.clone(), s.ws.clone()


@functools.lru_cache(maxsize=None)
def _rows_pass(W, R, limit, rows16, cap):
    """the sampler windows of the first list + the late list's pass and reduction from the common start: rows16 = 0 the existing launches, 1 the sixteen-wave form"""
    from mvsdf_amd._lib import check, lib
    s = _start(W, R, limit)
    b = _Bufs(s)
    a = s.args(b)
    if rows16:
        check(lib().mvsdf_trace_rows_stage(1, 1, cap, *a), 'mvsdf_trace_rows_stage(1)')
        check(lib().mvsdf_trace_rows_stage(2, 1, cap, *a), 'mvsdf_trace_rows_stage(2)')
    else:
        check(lib().mvsdf_trace_stage(3, *a), 'mvsdf_trace_stage(3)')
        check(lib().mvsdf_trace_cut_stage(3, 0, *a), 'mvsdf_trace_cut_stage(3)')
    torch.cuda.synchronize()
    n, off, c = s.n, _offsets(R, s.n), b.cnt.cpu().numpy()
    raw = lambda key, words: b.ws[off[key]:off[key] + 4 * words].cpu().numpy().tobytes()
    i32 = lambda key, k: b.ws[off[key]:off[key] + 4 * R].view(torch.int32)[:k].cpu().numpy()
    f32 = lambda key, rows: b.ws[off[key]:off[key] + 4 * R * rows].view(torch.float32).view(rows, R).cpu().numpy()
    rest_order = np.argsort(i32('list_rest', int(c[7])), kind='stable')
    rest, rest_src = i32('list_rest', int(c[7]))[rest_order], i32('src_rest', int(c[7]))[rest_order]
    secant = np.sort(i32('sec_list', int(c[4])))
    zmin, zmax, sec_state = f32('w_zmin', 1)[0], f32('w_zmax', 1)[0], f32('sec_state', 4)
    g = rest & 0x0fffffff
    return dict(sv=raw('sv', R * n), sv_late=raw('sv_late', R * n), points=b.pts.cpu().numpy().tobytes(), mask=b.mask.cpu().numpy().tobytes(),
                dists=b.dists.cpu().numpy().tobytes(), rest=rest.tobytes(), rest_src=rest_src.tobytes(), rest_z=np.stack([zmin[g], zmax[g]]).tobytes(),
                secant=secant.tobytes(), secant_state=sec_state[:, secant].tobytes(), cnt=c)


def _assert_same_pass(got, ref, what):
    for k in ref:
        if k != 'cnt':
            assert got[k] == ref[k], (what, k)
    assert got['cnt'][CNT_COMPARED].tolist() == ref['cnt'][CNT_COMPARED].tolist(), (what, got['cnt'].tolist(), ref['cnt'].tolist())


def _last_chunks(cnt):
    """rows of the last 32-row chunk of the first window and of the late pass (0: the list is empty)"""
    return [(int(k) * ni - 1) % 32 + 1 if k else 0 for k, ni in ((cnt[5], NF), (cnt[N_LATE], 100))]


@pytest.mark.parametrize('cap', CAPS, ids=['cap1', 'cap2', 'nocap'])
@pytest.mark.parametrize('limit', sorted(LIMITS))
@pytest.mark.parametrize('R', [8, 24, 64, 257])
@pytest.mark.parametrize('W', [64, 256])
def test_rows_form_equals_the_row_kernel(W, R, limit, cap):
    ref = _rows_pass(W, R, LIMITS[limit], 0, 0)
    got = _rows_pass(W, R, LIMITS[limit], 1, cap)
    _assert_same_pass(got, ref, (W, R, limit, cap))
    c = ref['cnt']
    if _sampler_rays_uncut(W, R) == 0:                            # (W = 256 at 8 rays: every ray that meets the sphere converges -- both lists stay empty under any limit)
        assert (W, R) == (256, 8) and int(c[5]) + int(c[N_LATE]) == 0
        return
    assert int(c[5]) + int(c[N_LATE]) > 0 and int(c[8]) > 0, 'no sampler row was evaluated'      # (under limit 1 every sampler ray may be a late one)
    if limit in ('one', 'two'):
        assert int(c[N_LATE]) > 0, 'the late list is empty'
        assert any(v != 0 for v in np.frombuffer(ref['sv_late'], np.float32)[:100])
    if cap and limit == 'one' and R >= 24:
        assert int(c[N_LATE]) * 100 > 32 * cap, 'the stride loop ran one trip only'


def test_rows_form_cases_cover_both_ragged_last_chunks():
    """some compared launch ends in a chunk whose second row tile is empty (<= 16 rows), and some in a chunk with a ragged second tile (17 .. 31 rows)"""
    lasts = []
    for W in (64, 256):
        for R in (8, 24, 64, 257):
            for limit in LIMITS.values():
                lasts += _last_chunks(_rows_pass(W, R, limit, 0, 0)['cnt'])
    assert any(1 <= v <= 16 for v in lasts), lasts
    assert any(17 <= v <= 31 for v in lasts), lasts


@pytest.mark.parametrize('W', [64, 256])
def test_rows_form_over_an_empty_late_list(W):
    ref = _rows_pass(W, 64, 1000, 0, 0)
    assert int(ref['cnt'][N_SPILL]) == 0 and int(ref['cnt'][N_LATE]) == 0 and int(ref['cnt'][5]) > 0
    for cap in CAPS:
        _assert_same_pass(_rows_pass(W, 64, 1000, 1, cap), ref, (W, 'empty', cap))
    assert set(ref['sv_late']) == {0}                            # nothing was written


def test_rows_form_is_refused_where_the_engine_has_none():
    from mvsdf_amd._lib import lib
    s = _start(64, 8, 1)
    b = _Bufs(s)
    a = list(s.args(b))
    a[0] = C.byref(ops.pack_trace_net(sdf_packed_net(synth.make_state_dict(64, 0)), 'f32').desc())
    assert lib().mvsdf_trace_rows_stage(2, 1, 0, *a) == -3
    a = list(s.args(b))
    a[17] = 1                                                     # mt_samples 1: 16-row chunks, no two-tile instance to stand for
    assert lib().mvsdf_trace_rows_stage(1, 1, 0, *a) == -3


# ---------------------------------------------------------------------------------------------------------------------------------------------
TP = 0.3
LATE = ('points', 'sdf_output')
OFF, ALL_ON = (0, 0, 0, 0), (1, 1, 1, 0)
CONFIGS = {'late_on_main': (1, 0, 0, 0), 'partition_beside_secant': (0, 1, 0, 0), 'rows16': (0, 0, 1, 0), 'rows16_cap2': (0, 0, 1, 2), 'all': ALL_ON}
SHAPES = {'64': (64, 1, 64, 3), 'ragged111': (64, 1, 111, 7), '257': (64, 1, 257, 5), 'w256_64': (256, 1, 64, 3)}


@functools.lru_cache(maxsize=None)
def _batch(B, P, seed):
    inp, _ = synth.make_batch(B, P, 0, seed, with_features=False, focal_scale=1.4)
    _, gt = synth.make_batch(B, P, 2, seed=seed, feat_hw=(60, 80), focal_scale=1.4)
    return {k: t(v) for k, v in inp.items()}, {k: t(v) for k, v in gt.items()}


def _model(W, fork, rounds=2):
    m = IDRNetwork(ConfigDict(synth.model_conf(W)))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(W, 0).items()})
    m = m.cuda().train()
    m.sphere_cut, m.sphere_cut_rounds = 2, rounds                 # the cut forced on; two rounds: nearly every ray is a late one; 0: the step's own limit
    if fork is not None:
        m.fork = fork
    return m


@functools.lru_cache(maxsize=None)
def _step(shape, fork, order, further=0, rounds=2):
    """one training step (forward, loss, backward) -> outputs (the two late keys apart), losses, gradients, counters, the late keys read last (after `further` more
    training steps with lr > 0), the count record of the host ring and of the forward block, the last tracer grid"""
    W, B, P, seed = SHAPES[shape]
    m = _model(W, fork, rounds)
    inp, gt = _batch(B, P, seed)
    loss_fn, opt = IDRLoss(), FlatAdam(m.parameters(), lr=1e-3)
    torch.manual_seed(11)
    out = m(dict(inp), TP)
    counters, st, rec = m.last_stats['counters'], m._last_step, m._last_rec()
    grid = st.last_tracer_grid()
    outs = {}

    def read():
        outs.update({k: out[k].detach().clone() for k in out.keys() if k not in LATE and torch.is_tensor(out[k])})
    if order == 'outputs_first':
        read()
    lo = loss_fn(out, dict(gt), TP, B)
    opt.zero_grad()
    opt.backward(lo['loss'])
    if order == 'loss_first':
        read()
    g = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).flatten() for p in m.parameters()]).clone()
    losses = {k: v.detach().clone() for k, v in lo.items()}
    torch.cuda.synchronize()
    cnt_fwd = counters.cpu().numpy().copy()
    ring = tuple(int(v) for v in st.wait_counts_seq(rec.seq, rec.fwd))
    block = tuple(int(v) for v in rec.fwd.u8[st.counts_off:st.counts_off + 32].view(torch.int64).cpu())
    for _ in range(further):                                      # the network moves on; the first forward's block must still resolve at ITS network
        opt.step()
        o2 = m(dict(inp), TP)
        opt.zero_grad()
        opt.backward(loss_fn(o2, dict(gt), TP, B)['loss'])
    late = {k: out[k].detach().clone() for k in LATE}              # mvsdf_step_resolve_unhit
    torch.cuda.synchronize()
    return outs, losses, g, cnt_fwd, late, ring, block, grid


def _assert_same_step(got, ref, what):
    for a, b in zip(got[:2], ref[:2]):
        assert a.keys() == b.keys() and len(a) >= 6
        for k in b:
            assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (what, k)
    assert torch.equal(got[2], ref[2]) and float(ref[2].abs().max()) > 0, what
    assert got[3][CNT_STEP].tolist() == ref[3][CNT_STEP].tolist(), (what, got[3].tolist(), ref[3].tolist())
    for k in LATE:
        assert torch.equal(got[4][k], ref[4][k]), (what, k)
    assert got[5] == got[6] == ref[5] == ref[6], (what, got[5:7], ref[5:7])
    assert got[7] == ref[7], (what, got[7], ref[7])


@pytest.mark.parametrize('order', ['outputs_first', 'loss_first'])
@pytest.mark.parametrize('rounds', [2, 0], ids=['limit2', 'step_limit'])
@pytest.mark.parametrize('config', sorted(CONFIGS))
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_step_with_the_fork_equals_the_step_without(shape, config, rounds, order):
    ref = _step(shape, OFF, order, 0, rounds)
    got = _step(shape, CONFIGS[config], order, 0, rounds)
    # A sampler ray of these batches is one that never converges: it wants all st_iters + 1 evaluations, so under a limit of two rounds every one of them is a late
    # ray (the late branch has the rows, the windows' launches leave at once), and under the step's own limit none is (the windows have the rows).
    if rounds == 2:
        assert int(ref[3][N_SPILL]) > 0 and int(ref[3][N_LATE]) > 0, 'the late branch has no rows: %s' % ref[3].tolist()
    else:
        assert int(ref[3][5]) > 0, 'the windows have no rows: %s' % ref[3].tolist()
    assert ref[5][0] > 0 and len(ref[0]) >= 6
    _assert_same_step(got, ref, (shape, config, rounds, order))


def test_unhit_rays_resolved_three_steps_later_equal_the_step_without_the_fork():
    ref = _step('64', OFF, 'loss_first', 3)
    got = _step('64', ALL_ON, 'loss_first', 3)
    assert int(ref[3][6]) > 0, 'no ray without a hit'
    _assert_same_step(got, ref, 'three steps later')
    first = _step('64', OFF, 'loss_first')
    for k in LATE:
        assert torch.equal(ref[4][k], first[4][k]), k            # ... at the FIRST forward's network


def test_fork_env_0_is_the_step_without_the_fork(monkeypatch):
    monkeypatch.setenv('MVSDF_FORK', '0')
    assert _model(64, None).fork == OFF
    monkeypatch.delenv('MVSDF_FORK')
    assert _model(64, None).fork == (-1, -1, -1, 0)
    monkeypatch.setenv('MVSDF_FORK', '0')
    got = _step('ragged111', None, 'loss_first')                  # (fork None: the attribute as the constructor read it from the environment)
    ref = _step('ragged111', OFF, 'loss_first')
    _assert_same_step(got, ref, 'MVSDF_FORK=0')
    assert np.delete(got[3], 15).tolist() == np.delete(ref[3], 15).tolist()                      # every counter but [15] (CNT_STEP): the same launches counted the same rows
