"""GPU (pytest -m gpu): the sphere cut (csrc/trace.hip: k_sphere_trace with a round limit + its resume launch; mvsdf_trace_cut_stage, mvsdf_step_set_sphere_cut)
against the launches it replaces.  The reference is always the UNCUT kernel and the step without the cut, never the new code.

  1. The tracer alone: mvsdf_trace_cut_stage 1 (limit), 2 (resume), mvsdf_trace_stage 3 (sampler windows of the first list), mvsdf_trace_cut_stage 3 (the late
     list in one pass), mvsdf_trace_stage 7 (secant chains), 5 (min-sdf rows) against mvsdf_trace_stage 1, 3, 7, 5: points, masks and dists byte for byte, the
     sampler (first + late), min-sdf and secant lists equal as sorted sets with the z ranges / secant brackets of their rays, the row counters 0..3 and the list
     lengths.  R = 8, 24 (a ragged last workgroup of the resume launch whenever the spill count is no multiple of 8), 64, 257 (a ragged last workgroup of the limited
     launch); limits 1 (every intersecting ray spills), 2, st_iters + 1 (the step's) and 1000 (nothing spills); the first rays of every batch miss the
     sphere (never an evaluation, never a spill).  The W = 64 network on the three-term engine (k_sphere_trace<1, 1, 16>) and the fmaf-chain engine (<1, 4, 4>), the
     W = 256 network on the three-term engine.  One more test walks the limits 1 .. st_iters + 3 at R = 257 and asserts that a workgroup with exactly ONE spilled ray
     occurred (the spill list names its rays: ray gid belongs to workgroup gid // 8).
  2. The step: IDRNetwork.sphere_cut = 2 (always) with a limit of 3 rounds -- small batches spill nothing under the step's own limit -- and with the default limit,
     against sphere_cut = False: every output, the six losses, every gradient entry with torch.equal, outputs read before the loss and after the backward.
     2 x 300 rays (the shape of tests/test_gpu_lazy.py) and a ragged batch of 111.
  3. `points` / `sdf_output` read after a cut step (mvsdf_step_resolve_unhit over a min-sdf list both launches appended to) equal the eager step's.

Every cut run asserts from the device counters that it spilled where it claims to (counters[13]); a comparison that spilled nothing would compare a kernel with itself."""
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
UNCUT = (('s', 1), ('s', 3), ('s', 7), ('s', 5))


def _cut(limit):
    return (('c', 1, limit), ('c', 2, 0), ('s', 3), ('c', 3, 0), ('s', 7), ('s', 5))


@functools.lru_cache(maxsize=None)
def _net(W, engine):
    return ops.pack_trace_net(sdf_packed_net(synth.make_state_dict(W, 0)), engine)


@functools.lru_cache(maxsize=None)
def _rays(R):
    """camera rays of one view, the first N_MISS turned past the sphere; object mask ~70 % true; shared, never modified"""
    inp, _ = synth.make_batch(1, R, 0, seed=100 + R, with_features=False, focal_scale=1.4)
    dirs, cam = ops.camera_rays(t(inp['uv']), t(inp['pose']), t(inp['intrinsics']))
    dirs = dirs.clone()
    for i in range(N_MISS):                                       # at a right angle to the line camera -> origin, the camera outside the sphere: no intersection
        e = torch.zeros(3, device='cuda'); e[i] = 1.0
        v = torch.linalg.cross(cam[0], e)
        dirs[0, i] = v / v.norm()
    rs = np.random.RandomState(R)
    om = t((rs.uniform(size=R) < 0.7).astype(np.uint8))
    steps = t(rs.uniform(size=trace_params(64)[5]).astype(np.float32))
    c, d = cam.cpu().numpy().astype(np.float64)[0], dirs.cpu().numpy().astype(np.float64)[0]
    dot = d @ c
    n_isect = int((dot * dot - (c @ c - 1.0) > 1e-6).sum())         # (the batches have no ray near the tangent: asserted against the kernel's own count below)
    return cam.contiguous(), dirs.contiguous(), om, steps, n_isect


def _offsets(R, n):
    """byte offsets of the regions the comparison reads (csrc/trace_route.h: mv_trace_ws, and mv_trace_cut_ws behind it)"""
    r = 4 * R
    base = (r * (11 + 2 * n) + 256 + 255) & ~255
    return dict(w_zmin=0, w_zmax=r, sec_state=2 * r, w_list=6 * r, w_list_min=7 * r, sec_list=8 * r, spill=base, list_late=base + 16 * r)


def _run(W, engine, R, seq):
    """the launches of `seq` through the C ABI on a zeroed workspace -> numpy points, mask, dists, counters and the lists with what belongs to their rays"""
    from mvsdf_amd._lib import TraceParams, check, lib, ptr, stream_of
    net = _net(W, engine)
    cam, dirs, om, steps, _ = _rays(R)
    tp = TraceParams(*trace_params(W))
    n = tp.n_steps
    iv = torch.linspace(0, 1, n).cuda()
    desc = net.desc()
    pts = torch.zeros(R, 3, device='cuda'); mask = torch.zeros(R, dtype=torch.uint8, device='cuda'); dists = torch.zeros(R, device='cuda')
    cnt = torch.zeros(16, dtype=torch.int64, device='cuda')
    wsb = lib().mvsdf_trace_cut_workspace_bytes(R, n)
    assert wsb > lib().mvsdf_trace_workspace_bytes_n(R, n)
    off = _offsets(R, n)
    assert wsb >= off['list_late'] + 4 * R * (1 + n)
    ws = torch.zeros(wsb, dtype=torch.uint8, device='cuda')
    common = (C.byref(desc), C.byref(tp), ptr(cam), ptr(dirs), ptr(om), 1, R, 1, ptr(iv), ptr(steps), ptr(pts), ptr(mask), ptr(dists), ptr(cnt), ptr(ws),
              C.c_size_t(wsb), 1, 4, stream_of(dirs))
    spill_gids = None
    for s in seq:
        if s[0] == 's':
            check(lib().mvsdf_trace_stage(s[1], *common), 'mvsdf_trace_stage(%d)' % s[1])
        else:
            check(lib().mvsdf_trace_cut_stage(s[1], s[2], *common), 'mvsdf_trace_cut_stage(%d)' % s[1])
            if s[1] == 1:                                         # the spill list as the limited launch left it: word 10 of a ray's 16 is its id
                torch.cuda.synchronize()
                k = int(cnt[N_SPILL])
                spill_gids = ws[off['spill']:off['spill'] + 64 * R].view(torch.int32).view(R, 16)[:k, 10].cpu().numpy().copy()
    torch.cuda.synchronize()
    c = cnt.cpu().numpy()
    i32 = lambda key, k: ws[off[key]:off[key] + 4 * R].view(torch.int32)[:k].cpu().numpy()
    f32 = lambda key, rows=1: ws[off[key]:off[key] + 4 * R * rows].view(torch.float32).view(rows, R).cpu().numpy()
    zmin, zmax, sec_state = f32('w_zmin')[0], f32('w_zmax')[0], f32('sec_state', 4)
    sampler = np.sort(np.concatenate([i32('w_list', int(c[5])), i32('list_late', int(c[N_LATE]))]))
    minsdf = np.sort(i32('w_list_min', int(c[6])))
    secant = np.sort(i32('sec_list', int(c[4])))

    def ranges(entries):
        g = entries & 0x0fffffff
        return np.stack([zmin[g], zmax[g]])
    return dict(points=pts.cpu().numpy(), mask=mask.cpu().numpy(), dists=dists.cpu().numpy(), cnt=c, sampler=sampler, minsdf=minsdf, secant=secant,
                sampler_z=ranges(sampler), minsdf_z=ranges(minsdf), secant_state=sec_state[:, secant], spill_gids=spill_gids)


@functools.lru_cache(maxsize=None)
def _uncut(W, engine, R):
    return _run(W, engine, R, UNCUT)


def _assert_equals_the_uncut_kernel(got, ref, what):
    for k in ('points', 'mask', 'dists'):
        assert got[k].tobytes() == ref[k].tobytes(), (what, k, int((got[k] != ref[k]).sum()))
    for k in ('sampler', 'minsdf', 'secant', 'sampler_z', 'minsdf_z', 'secant_state'):
        assert got[k].shape == ref[k].shape and got[k].tobytes() == ref[k].tobytes(), (what, k)
    g, r = got['cnt'], ref['cnt']
    assert np.array_equal(g[:4], r[:4]), (what, g[:4].tolist(), r[:4].tolist())
    assert (int(g[4]), int(g[5] + g[N_LATE]), int(g[6])) == (int(r[4]), int(r[5]), int(r[6])), (what, g.tolist(), r.tolist())
    assert int(r[N_SPILL]) == 0 and int(r[N_LATE]) == 0
    assert len(np.unique(got['sampler'] & 0x0fffffff)) == len(got['sampler'])                  # no ray on both sampler lists


ST_ITERS = trace_params(64)[4]
LIMITS = {'one': 1, 'two': 2, 'step': ST_ITERS + 1, 'none': 1000}


@pytest.mark.parametrize('limit', sorted(LIMITS))
@pytest.mark.parametrize('R', [8, 24, 64, 257])
@pytest.mark.parametrize('engine', ['f32x3', 'f32'])
def test_cut_and_resume_equal_the_uncut_kernel(engine, R, limit):
    ref = _uncut(64, engine, R)
    got = _run(64, engine, R, _cut(LIMITS[limit]))
    what = (engine, R, limit)
    _assert_equals_the_uncut_kernel(got, ref, what)
    n_isect, spilled = _rays(R)[4], int(got['cnt'][N_SPILL])
    assert int(ref['cnt'][0]) > 0 and (int(ref['cnt'][1]), int(ref['cnt'][4]), int(ref['cnt'][3])) != (0, 0, 0), 'the batch exercises nothing'
    assert n_isect <= R - N_MISS
    if limit == 'none':
        assert spilled == 0 and int(got['cnt'][N_LATE]) == 0
    elif limit == 'one':
        assert spilled == n_isect, (what, spilled, n_isect)       # every ray that intersects the sphere wants a second evaluation: all of them spill
        assert not np.isin(np.arange(N_MISS), got['spill_gids']).any()                         # ... and none that misses it
    else:
        assert 0 <= spilled <= n_isect
    if limit == 'two':
        assert spilled > 0, what
    assert sorted(got['spill_gids'].tolist()) == sorted(set(got['spill_gids'].tolist())) and len(got['spill_gids']) == spilled


def test_cut_at_width_256():
    ref = _uncut(256, 'f32x3', 64)
    for limit in (2, ST_ITERS + 1):
        got = _run(256, 'f32x3', 64, _cut(limit))
        _assert_equals_the_uncut_kernel(got, ref, (256, limit))
        assert limit != 2 or int(got['cnt'][N_SPILL]) > 0


def test_a_workgroup_with_one_spilled_ray():
    """limits 1 .. st_iters + 3 at 257 rays: every one equals the uncut kernel, the spill counts fall, and somewhere a workgroup spills exactly one of its eight rays"""
    ref = _uncut(64, 'f32x3', 257)
    singles, counts = 0, []
    for limit in range(1, ST_ITERS + 4):
        got = _run(64, 'f32x3', 257, _cut(limit))
        _assert_equals_the_uncut_kernel(got, ref, limit)
        per_wg = np.bincount(got['spill_gids'] // 8, minlength=33)
        singles += int((per_wg == 1).sum())
        counts.append(len(got['spill_gids']))
    assert counts == sorted(counts, reverse=True) and counts[0] > 0, counts
    assert singles > 0, counts


# ---------------------------------------------------------------------------------------------------------------------------------------------
TP = 0.3
LATE = ('points', 'sdf_output')


def _batch(B, P, seed):
    inp, _ = synth.make_batch(B, P, 0, seed, with_features=False, focal_scale=1.4)
    _, gt = synth.make_batch(B, P, 2, seed=seed, feat_hw=(60, 80), focal_scale=1.4)
    return {k: t(v) for k, v in inp.items()}, {k: t(v) for k, v in gt.items()}


def _step(shape, cut, rounds, order, eager=False):
    """one training step (forward, loss, backward) -> outputs (the two late keys apart), losses, gradients, counters, the late keys read last"""
    B, P, seed = shape
    m = IDRNetwork(ConfigDict(synth.model_conf(64)))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(64, 0).items()})
    m = m.cuda().train()
    m.sphere_cut, m.sphere_cut_rounds, m.eager_unhit_rows = cut, rounds, eager
    inp, gt = _batch(B, P, seed)
    loss_fn, opt = IDRLoss(), FlatAdam(m.parameters(), lr=1e-3)
    torch.manual_seed(11)
    out = m(inp, TP)
    counters = m.last_stats['counters']
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
    late = {k: out[k].detach().clone() for k in LATE}              # mvsdf_step_resolve_unhit (or, eager, the values of the forward)
    torch.cuda.synchronize()
    return outs, losses, g, cnt_fwd, late


@functools.lru_cache(maxsize=None)
def _step_without_cut(shape, order):
    return _step(shape, False, 0, order)


def _assert_same_step(got, ref, what):
    for a, b in zip(got[:2], ref[:2]):
        assert a.keys() == b.keys() and len(a) >= 6
        for k in b:
            assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (what, k)
    assert torch.equal(got[2], ref[2]) and float(ref[2].abs().max()) > 0, what
    assert np.array_equal(got[3][:5], ref[3][:5]) and got[3][6] == ref[3][6] and got[3][5] + got[3][N_LATE] == ref[3][5], (what, got[3].tolist(), ref[3].tolist())
    for k in LATE:
        assert torch.equal(got[4][k], ref[4][k]), (what, k)


@pytest.mark.parametrize('order', ['outputs_first', 'loss_first'])
@pytest.mark.parametrize('rounds', [3, 0], ids=['limit3', 'step_limit'])
@pytest.mark.parametrize('shape', [(2, 300, 3), (1, 111, 7)], ids=['2x300', 'ragged111'])
def test_step_with_the_cut_equals_the_step_without(shape, rounds, order):
    ref = _step_without_cut(shape, order)
    got = _step(shape, 2, rounds, order)
    assert int(ref[3][N_SPILL]) == 0
    assert rounds == 0 or int(got[3][N_SPILL]) > 0, 'nothing spilled under a limit of %d rounds' % rounds
    _assert_same_step(got, ref, (shape, rounds, order))


def test_unhit_rays_resolved_after_a_cut_step_equal_the_eager_step():
    """min-sdf list entries appended by BOTH sphere launches, evaluated when `points` / `sdf_output` are read: the eager step's values"""
    shape = (2, 300, 3)
    eager = _step(shape, False, 0, 'loss_first', eager=True)
    got = _step(shape, 2, 3, 'loss_first')
    assert int(got[3][N_SPILL]) > 0 and int(got[3][6]) > 0 and int(got[3][3]) == 0 and int(eager[3][3]) == 100 * int(eager[3][6])
    for k in LATE:
        assert torch.equal(got[4][k], eager[4][k]), k
    assert torch.equal(got[2], eager[2])
    for k in eager[0]:
        assert torch.equal(got[0][k], eager[0][k]), k
