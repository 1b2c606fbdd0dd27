"""The native training step leaves what only the rays WITHOUT a hit need -- minimal_sdf_points (ray_tracing.py:280-308), their evaluation rows and their
sdf_output -- to the first reader of `points` / `sdf_output` (mvsdf_step_resolve_unhit; IDRNetwork.eager_unhit_rows = True is the launch sequence that evaluates
them inside the forward).  Nothing a caller can observe may differ: every output key, the six loss scalars, every gradient entry and the next draw of the CPU
generator equal the eager run's with torch.equal, whether the two keys are read before the loss, after the backward, or after THREE further forward + optimiser
steps with lr > 0 (the late evaluation runs at the weights, biases and min-sdf steps of ITS forward, all kept in the forward block).  Both the deferred and the
classic step.  With the keys never read no min-sdf row is evaluated (counters[3] == 0, no row workgroups in the last tracer launch); a second read launches
nothing; an empty min-sdf list resolves to the same values.

Shapes (synth.make_batch(B, P, 0, seed, with_features=False, focal_scale=1.4) rays, all-ones object mask; counts from the CPU oracle on 'f32x3', asserted from the
device counters before anything else): width 64: 4 secant rays / empty min-sdf list, 13 / 6 (under one tile), 17 / 11 (one ray into the second secant
workgroup), 60 / 27, 103 / 53 (the shape of tests/test_gpu_lazy.py); width 256: 17 / 44; width 512 (the secant chains as the part-8 launch of k_ray_samples): 12 / 6
(under one 16-ray workgroup), 21 / 33 (one workgroup and five rays).  The split engines ('bf16x2', 'bf16x3': no exact oracle, so no tabulated counts) run the
width-256 shape of 2 x 40 rays: both lists non-empty and the same in the eager and the late run."""
import pytest
import torch

from helpers import t
from mvsdf_amd.model.implicit_differentiable_renderer import IDRNetwork, PendingOutputs, StepOutputs
from mvsdf_amd.model.loss import IDRLoss
from mvsdf_amd.optim import FlatAdam
from mvsdf_amd.utils import synth
from mvsdf_amd.utils.config import ConfigDict

pytestmark = pytest.mark.gpu
TP = 0.3
LATE = ('points', 'sdf_output')
# (W, B, P, seed) -> (secant rays, rays on the min-sdf list)
CASES = {(64, 1, 24, 1): (4, 0), (64, 2, 40, 5): (13, 6), (64, 1, 64, 3): (17, 11), (64, 1, 200, 3): (60, 27), (64, 2, 300, 3): (103, 53), (256, 2, 40, 5): (17, 44),
         (512, 1, 24, 1): (12, 6), (512, 1, 64, 3): (21, 33)}
SPLIT_CASE = (256, 2, 40, 5)


def _batch(B, P, seed):
    inp, _ = synth.make_batch(B, P, 0, seed, with_features=False, focal_scale=1.4)          # the rays of the table above ...
    _, gt = synth.make_batch(B, P, 2, seed=seed, feat_hw=(60, 80), focal_scale=1.4)         # ... and a ground truth with source views for the feature term
    return {k: t(v) for k, v in inp.items()}, {k: t(v) for k, v in gt.items()}


def _grads(m):
    return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).flatten() for p in m.parameters()]).clone()


def _run(case, deferred, eager, when, dtype=None):
    """One model, step 0 + three further steps with lr > 0.  when: 'before' (the loss) / 'after' (the backward) / 'late' (after the further steps) -- when
    `points` / `sdf_output` of step 0 are read first.  dtype: another tracing arithmetic than the default (its list lengths are not tabulated: returned in info)."""
    W, B, P, seed = case
    m = IDRNetwork(ConfigDict(synth.model_conf(W)))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(W, 0).items()})
    m = m.cuda().train()
    if dtype is not None:
        m.set_trace_dtype(dtype)
    m.deferred_step, m.eager_unhit_rows = deferred, eager
    inp, gt = _batch(B, P, seed)
    loss_fn, opt = IDRLoss(), FlatAdam(m.parameters(), lr=1e-3)
    torch.manual_seed(11)
    out = m(inp, TP)
    st, counters = m._last_step, m.last_stats['counters']
    torch.cuda.synchronize()
    assert dtype is not None or (int(counters[4]), int(counters[6])) == CASES[case], 'the input no longer gives %s secant / min-sdf rays: %s' % (CASES[case], counters[:9].tolist())
    grid = st.last_tracer_grid()
    info = {'type': type(out), 'grid': grid, 'rows_minsdf_at_forward': int(counters[3]), 'lists': (int(counters[4]), int(counters[6]))}
    snap = {}

    def read():
        snap.update({k: out[k].clone() for k in LATE})
    if when == 'before':
        read()
    lo = loss_fn(out, dict(gt), TP, B)
    opt.zero_grad()
    opt.backward(lo['loss'])
    if when == 'after':
        read()
    g = _grads(m)
    rng = torch.rand(4)                                            # the next draw from the CPU generator
    losses = {k: v.detach().clone() for k, v in lo.items()}
    rest = {k: out[k].detach().clone() for k in out.keys() if k not in LATE and torch.is_tensor(out[k])}    # (resolves the N-shaped keys of a deferred step, not the two late ones)
    opt.step()
    for _ in range(3):                                             # the parameters move on: three further forward + optimiser steps
        o2 = m(inp, TP)
        opt.zero_grad()
        opt.backward(loss_fn(o2, dict(gt), TP, B)['loss'])
        opt.step()
    torch.cuda.synchronize()
    info['rows_minsdf_before_late_read'] = int(counters[3])
    if when == 'late':
        read()
    torch.cuda.synchronize()
    info['rows_minsdf_after_read'] = int(counters[3])
    _ = out['points'], out.get('sdf_output'), dict(out)            # a second read
    torch.cuda.synchronize()
    info['rows_minsdf_after_second_read'] = int(counters[3])
    return snap, rest, losses, g, rng, info


_eager = {}


def _eager_run(case, deferred):
    """the eager partner, snapshot taken at step 0 (shared by the three reading orders; never modified)"""
    key = (case, deferred)
    if key not in _eager:
        _eager[key] = _run(case, deferred, True, 'before')
    return _eager[key]


def _assert_equals_the_eager_step(late_run, eager_run, n_min, deferred, when):
    snap_e, rest_e, loss_e, g_e, rng_e, info_e = eager_run
    snap, rest, loss, g, rng, info = late_run
    # the eager partner ran the old launch sequence: row workgroups in the last tracer launch, the min-sdf rows counted inside the forward
    assert info_e['grid'][1] > 0 and info_e['rows_minsdf_at_forward'] == 100 * n_min
    assert info_e['type'] is (PendingOutputs if deferred else dict)
    assert info['type'] is (PendingOutputs if deferred else StepOutputs)
    # the new default: the secant chains alone, no min-sdf row until somebody reads
    assert info['grid'][0] > 0 and info['grid'][1] == 0 and info['rows_minsdf_at_forward'] == 0
    if when == 'late':
        assert info['rows_minsdf_before_late_read'] == 0           # three further steps later: still nothing evaluated
    assert info['rows_minsdf_after_read'] == 100 * n_min
    assert info['rows_minsdf_after_second_read'] == 100 * n_min    # a second read launched nothing (the reduction would have counted the rows again)
    for k in LATE:
        assert snap[k].shape == snap_e[k].shape and torch.equal(snap[k], snap_e[k]), (k, when)
    assert rest.keys() == rest_e.keys()
    for k in rest_e:
        assert torch.equal(rest[k], rest_e[k]), k
    assert loss.keys() == loss_e.keys() and len(loss) >= 6
    for k in loss_e:
        assert torch.equal(loss[k], loss_e[k]), k
    assert torch.equal(g, g_e) and float(g.abs().max()) > 0
    assert torch.equal(rng, rng_e)


@pytest.mark.parametrize('when', ['before', 'after', 'late'])
@pytest.mark.parametrize('deferred', [True, False])
@pytest.mark.parametrize('case', sorted(CASES))
def test_unhit_rays_resolved_when_read_equal_the_eager_step(case, deferred, when):
    _assert_equals_the_eager_step(_run(case, deferred, False, when), _eager_run(case, deferred), CASES[case][1], deferred, when)


@pytest.mark.parametrize('dtype', ['bf16x2', 'bf16x3'])
def test_unhit_rays_resolved_late_on_the_split_engines(dtype):
    """the deferred step on a split engine, `points` / `sdf_output` read three steps later: both lists hold rays, the same ones as in the eager run, and everything
    a caller can observe equals the eager run's"""
    eager_run = _run(SPLIT_CASE, True, True, 'before', dtype)
    late_run = _run(SPLIT_CASE, True, False, 'late', dtype)
    n_sec, n_min = late_run[5]['lists']
    assert n_sec > 0 and n_min > 0 and (n_sec, n_min) == eager_run[5]['lists']
    _assert_equals_the_eager_step(late_run, eager_run, n_min, True, 'late')
