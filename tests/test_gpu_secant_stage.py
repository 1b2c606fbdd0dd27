"""Stage 7 of mvsdf_trace_stage: the secant chains alone in the sphere tracer's engine form (k_secant_chains<1, 1, 16> for the three-weight-term engine up to
hidden width 256, csrc/trace_route.h::mv_route_secant; the stage-6 instance for every other engine and, at width 512, for that engine too: the part-8 launch of
k_ray_samples<., 4, 8>, one 16-ray workgroup per 16 rays of the batch, bounded by the device-side secant count).

* 'f32x3': stages 1, 3, 7 against oracle.trace (the CPU model of that arithmetic) BIT FOR BIT on points / dists / mask of the secant rays and on the secant row
  counter -- the reference is the oracle, not another stage of the library under test.  Shapes: 4 secant rays (under one tile), 13, 17 (one ray into the second
  workgroup), 60 (four workgroups, the last one partial) at width 64; 5 and 17 at width 256; 12 (under one 16-ray workgroup) and 21 (one workgroup and five
  rays) at width 512.  The counts are asserted from the device counters first: an input
  that stopped exercising an edge fails instead of passing empty.
* every other tracing arithmetic: stage 7 == stage 6 bit for bit (it runs the same instance)."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import sdf_packed_net, t, trace_params
from mvsdf_amd import ops
from mvsdf_amd._lib import TraceParams, check, lib, ptr, stream_of
from mvsdf_amd.utils import synth

pytestmark = pytest.mark.gpu
N_STEPS = 100
# (W, B, P, seed) -> (secant rays, rays on the min-sdf list), from the CPU oracle on the 'f32x3' arithmetic
CASES = {(64, 1, 24, 1): (4, 0), (64, 2, 40, 5): (13, 6), (64, 1, 64, 3): (17, 11), (64, 1, 200, 3): (60, 27), (256, 1, 64, 3): (5, 42), (256, 2, 40, 5): (17, 44),
         (512, 1, 24, 1): (12, 6), (512, 1, 64, 3): (21, 33)}


def _rays(B, P, seed):
    inp, _ = synth.make_batch(B, P, 0, seed, with_features=False, focal_scale=1.4)
    dirs, cam = ops.camera_rays(t(inp['uv']), t(inp['pose']), t(inp['intrinsics']))
    return dirs, cam


def _stages(net, W, B, P, dirs, cam, steps, stages):
    """-> points, mask, dists, counters, the secant list (ray ids) after the given stages of mvsdf_trace_stage on a fresh workspace"""
    R = B * P
    om = torch.ones(R, dtype=torch.uint8, device='cuda')
    iv = torch.linspace(0, 1, N_STEPS).cuda()
    tp = TraceParams(*trace_params(W))
    d = net.desc()
    pts, mask, dists = torch.zeros(R, 3, device='cuda'), torch.zeros(R, dtype=torch.uint8, device='cuda'), torch.zeros(R, device='cuda')
    cnt = torch.zeros(16, dtype=torch.int64, device='cuda')
    wsb = lib().mvsdf_trace_workspace_bytes_n(R, N_STEPS)
    ws = torch.zeros(wsb, dtype=torch.uint8, device='cuda')
    for stage in stages:
        check(lib().mvsdf_trace_stage(stage, C.byref(d), C.byref(tp), ptr(cam), ptr(dirs), ptr(om), B, P, 1, ptr(iv), ptr(steps), ptr(pts), ptr(mask), ptr(dists),
                                      ptr(cnt), ptr(ws), C.c_size_t(wsb), 1, 2, stream_of(dirs)), 'stage %d' % stage)
    torch.cuda.synchronize()
    n_sec = int(cnt[4])
    sec = ws[8 * 4 * R:9 * 4 * R].view(torch.int32)[:n_sec].long()  # trace_route.h::mv_trace_ws: sec_list is the ninth [R] region of 4-byte words
    return pts, mask, dists, cnt, sec


@pytest.mark.parametrize('W,B,P,seed', sorted(CASES))
def test_stage7_secant_rays_equal_the_oracle(oracle, W, B, P, seed):
    n_sec, n_min = CASES[(W, B, P, seed)]
    sd = synth.make_state_dict(W, 0)
    net = ops.pack_bf16_net(sdf_packed_net(sd), terms=3, weight_terms=3)
    dirs, cam = _rays(B, P, seed)
    steps_np = np.random.RandomState(0).uniform(size=N_STEPS).astype(np.float32)
    pts, mask, dists, cnt, sec = _stages(net, W, B, P, dirs, cam, t(steps_np), (1, 3, 7))
    assert (int(cnt[4]), int(cnt[6])) == (n_sec, n_min), 'the input no longer gives %d secant rays / %d min-sdf rays: %s' % (n_sec, n_min, cnt[:9].tolist())
    p_o, m_o, d_o, rows = oracle.trace(oracle.Net(sd, bf16='f32x3'), cam.cpu().numpy(), dirs.cpu().numpy(), np.ones(B * P, bool), True, steps_np,
                                       np.linspace(0, 1, N_STEPS).astype(np.float32), **synth.model_conf(W)['ray_tracer'])
    assert int(cnt[2]) == int(rows[2]) == 8 * n_sec                # the secant row counter
    assert int(cnt[3]) == 0                                        # no min-sdf row was evaluated
    assert sec.numel() == n_sec and len(set(sec.tolist())) == n_sec
    s = sec.cpu().numpy()
    assert np.array_equal(mask.cpu().numpy()[s], m_o[s]) and m_o[s].all()
    assert np.array_equal(dists.cpu().numpy()[s], d_o[s]), 'secant dists != oracle'
    assert np.array_equal(pts.cpu().numpy()[s], p_o[s]), 'secant points != oracle'
    assert np.array_equal(mask.cpu().numpy(), m_o)                 # (the hit mask is final after stage 3)


@pytest.mark.parametrize('dtype', ['f32', 'bf16w', 'bf16x2', 'bf16x3'])
def test_stage7_equals_stage6_on_the_other_engines(dtype):
    W, B, P, seed = 64, 1, 200, 3
    for Wn in (W, 256, 512):
        net = ops.pack_trace_net(sdf_packed_net(synth.make_state_dict(Wn, 0)), dtype)
        dirs, cam = _rays(B, P, seed)
        steps = t(np.random.RandomState(0).uniform(size=N_STEPS).astype(np.float32))
        a = _stages(net, Wn, B, P, dirs, cam, steps, (1, 3, 6))
        b = _stages(net, Wn, B, P, dirs, cam, steps, (1, 3, 7))
        assert int(a[3][4]) > 0 and int(a[3][2]) == 8 * int(a[3][4])
        for x, y in zip(a[:3], b[:3]):
            assert torch.equal(x, y)
        assert torch.equal(a[3][:9], b[3][:9]) and sorted(a[4].tolist()) == sorted(b[4].tolist())
