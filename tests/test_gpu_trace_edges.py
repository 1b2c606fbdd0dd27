"""GPU (pytest -m gpu): both routes of the HIP tracer against the C oracle at the ray, sample and geometry edges of tests/trace_cases.py, bit for bit.

  * the GENERIC route (ops.trace_generic: k_gen_init / k_gen_step / k_gen_finish / k_gen_lists / k_gen_rows / k_gen_secant / k_gen_sort_list around an opaque
    `sdf` callable) with the analytic SDF, every row of the table, training and eval;
  * the FUSED route (ops.trace) with the W = 64 network on the fmaf-chain engine ('f32'), the three-term engine ('f32x3') and bf16-rounded weights ('bf16w'),
    at (mt, mt_samples) in {(1, 1), (2, 3), (4, 4)};
  * the two routes against each other with `sdf = ops.sdf_col0(net, .)`;
  * the host-side refusals of the C ABI.

Every comparison is np.array_equal on points, mask, dists and the row counters over ALL rays (the oracle's sphere intersection is the kernel's): the project's
rule for the bit-exact arithmetics, no tolerance.  tests/test_trace_cases_host.py holds the table to the branches these tests rely on."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import trace_cases as TC
from helpers import analytic_sdf, sdf_packed_net
from mvsdf_amd import ops
from mvsdf_amd.utils import synth

pytestmark = pytest.mark.gpu

CNT_N_SECANT, CNT_N_SAMPLER, CNT_N_MINSDF = 4, 5, 6               # include/mvsdf_hip.h MVSDF_CNT_*
TILINGS = ((1, 1), (2, 3), (4, 4))
ENGINES = {'f32': False, 'f32x3': 'f32x3', 'bf16w': 'weights'}    # ops.TRACE_DTYPES name -> oracle.Net(bf16=...)


def dev(a):
    return torch.tensor(np.asarray(a)).cuda()                     # (a copy: the table's arrays are shared and read-only)


def dev_case(c):
    B, P = c.ray_dirs.shape[:2]
    return dict(cam_loc=dev(c.cam_loc), ray_dirs=dev(c.ray_dirs).reshape(B, P, 3), object_mask=dev(c.object_mask), intervals=dev(c.intervals),
                minsdf_steps=dev(c.minsdf_steps))


def to_np(out):
    pts, mask, dists, cnt = out
    torch.cuda.synchronize()
    return pts.cpu().numpy(), mask.cpu().numpy(), dists.cpu().numpy(), cnt.cpu().numpy()


def assert_same(got, want, what):
    """points, mask, dists of all rays and the four row counters, bit for bit"""
    (pts, mask, dists, cnt), (p_o, m_o, d_o, rows_o) = got, want
    assert np.array_equal(mask, m_o), what
    assert np.array_equal(dists, d_o), (what, int((dists != d_o).sum()))
    assert np.array_equal(pts, p_o), what
    assert np.array_equal(cnt[:4], rows_o), (what, cnt[:4].tolist(), rows_o.tolist())


def list_counts(oracle, net, c, training, rows):
    """(sampler, secant, min-sdf) rays of the oracle run.  Without secant steps rows[2] is 0 whatever the list holds: who is on the secant list does not depend
    on the number of steps, so that count comes from a run with one step."""
    n_s, n_sec, n_m = TC.list_counts(rows, c.params)
    if n_sec is None:
        rows1 = oracle.trace(net, c.cam_loc, c.ray_dirs, c.object_mask, training, c.minsdf_steps, c.intervals, analytic=net is None,
                             **dict(c.params, n_secant_steps=1))[3]
        assert np.array_equal(rows1[[0, 1, 3]], rows[[0, 1, 3]])
        n_sec = int(rows1[2])
    return n_s, n_sec, n_m


def assert_list_counters(cnt, counts, what):
    assert (int(cnt[CNT_N_SAMPLER]), int(cnt[CNT_N_SECANT]), int(cnt[CNT_N_MINSDF])) == tuple(counts), (what, cnt[:7].tolist(), counts)


class Counting:
    """An opaque `sdf` callable that records how many rows each call got"""

    def __init__(self, fn, column=False):
        self.fn, self.calls, self.column = fn, [], column

    def __call__(self, x):
        assert x.dim() == 2 and x.shape[1] == 3 and x.shape[0] > 0
        self.calls.append(int(x.shape[0]))
        y = self.fn(x)
        return y.reshape(-1, 1) if self.column else y


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the generic route against the oracle
@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('name', TC.ANALYTIC)
def test_generic_route_bit_exact_vs_oracle(oracle, name, training):
    c = TC.case(name)
    want = TC.oracle_analytic(name, training)
    sdf = Counting(analytic_sdf)
    d = dev_case(c)
    got = to_np(ops.trace_generic(sdf, d['cam_loc'], d['ray_dirs'], d['object_mask'], TC.params_tuple(c.params), training, d['intervals'], d['minsdf_steps']))
    assert_same(got, want, name)
    assert_list_counters(got[3], list_counts(oracle, None, c, training, want[3]), name)
    assert sum(sdf.calls) == int(want[3].sum())                   # the callable saw exactly the rows the reference evaluates


def test_generic_route_chunked_callable(oracle):
    """chunk = 97: the same bits, the same rows, never more than 97 of them in one call (ray_tracing.py:217,300 split at 100 000)"""
    c = TC.case('default')
    want = TC.oracle_analytic('default', True)
    sdf = Counting(analytic_sdf)
    d = dev_case(c)
    got = to_np(ops.trace_generic(sdf, d['cam_loc'], d['ray_dirs'], d['object_mask'], TC.params_tuple(c.params), True, d['intervals'], d['minsdf_steps'],
                                  chunk=97))
    assert_same(got, want, 'chunk=97')
    assert sum(sdf.calls) == int(want[3].sum()) and max(sdf.calls) <= 97 and sdf.calls.count(97) > 100


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
def test_generic_route_through_the_module(oracle, training):
    """RayTracing(...)(sdf=<callable returning [M, 1]>, ...): the reference's signature, a bounding sphere other than 1, no line search"""
    from mvsdf_amd.model.ray_tracing import RayTracing
    c = TC.case('r08')
    assert c.params['dist_clip'] == 0.5                           # (the module takes dist_clip from the IDR_RENDER switch, not from its constructor)
    rt = RayTracing(**{k: v for k, v in c.params.items() if k != 'dist_clip'}).cuda()
    rt.train(training)
    sdf = Counting(analytic_sdf, column=True)
    d = dev_case(c)
    with torch.no_grad():
        pts, mask, dists = rt(sdf=sdf, cam_loc=d['cam_loc'], object_mask=d['object_mask'], ray_directions=d['ray_dirs'],
                              minsdf_steps=d['minsdf_steps'] if training else None)
    want = TC.oracle_analytic('r08', training)
    assert_same(to_np((pts, mask, dists, rt.last_counters)), want, 'RayTracing')
    assert sum(sdf.calls) == int(want[3].sum())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the fused route against the oracle
@functools.lru_cache(maxsize=None)
def _nets(W, engine):
    """(the packed device network on `engine`, the oracle's network of that arithmetic); shared, never modified"""
    from oracle import oracle as O
    sd = synth.make_state_dict(W, 0)
    return ops.pack_trace_net(sdf_packed_net(sd), engine), O.Net(sd, bf16=ENGINES[engine])


@functools.lru_cache(maxsize=None)
def _oracle_net_run(name, W, engine, training):
    from oracle import oracle as O
    c = TC.case(name)
    out = O.trace(_nets(W, engine)[1], c.cam_loc, c.ray_dirs, c.object_mask, training, c.minsdf_steps, c.intervals, **c.params)
    for a in out:
        a.setflags(write=False)
    return out


def _fused_vs_oracle(oracle, name, W, engine, tilings):
    c = TC.case(name)
    net, onet = _nets(W, engine)
    assert net.trace_dtype == ops.TRACE_DTYPES[engine]
    d = dev_case(c)
    for training in (True, False):
        want = _oracle_net_run(name, W, engine, training)
        counts = list_counts(oracle, onet, c, training, want[3])
        for mt, mts in tilings:
            what = (name, engine, 'train' if training else 'eval', mt, mts)
            got = to_np(ops.trace(net, d['cam_loc'], d['ray_dirs'], d['object_mask'], TC.params_tuple(c.params), training, d['intervals'], d['minsdf_steps'],
                                  mt=mt, mt_samples=mts))
            assert_same(got, want, what)
            assert_list_counters(got[3], counts, what)


BIG = ('r2048', 'r2049', 'r4096', 'r4097', 'r8192', 'r8193')
SMALL = tuple(n for n in TC.FUSED if n not in BIG)
# the ray counts around one sphere-tracing workgroup per compute unit (tail filling on at 2048 * mt rays, off one ray later): the oracle's time for the network
# dominates these, so each engine gets the pairs where ITS rule changes -- the fmaf-chain engine at mt = 1, 2, 4 (bf16-rounded weights: mt = 1); 'f32x3' (on above
# 2048 rays only) at mt = 2
BIG_RUNS = [('r2048', 'f32', TILINGS), ('r2049', 'f32', TILINGS), ('r4096', 'f32', ((2, 3), (4, 4))), ('r4097', 'f32', ((2, 3), (4, 4))),
            ('r8192', 'f32', ((4, 4),)), ('r8193', 'f32', ((4, 4),)),
            ('r2048', 'bf16w', ((1, 1),)), ('r2049', 'bf16w', ((1, 1),)), ('r4096', 'f32x3', ((2, 3),)), ('r4097', 'f32x3', ((2, 3),))]


@pytest.mark.parametrize('engine', list(ENGINES))
@pytest.mark.parametrize('name', SMALL)
def test_fused_route_bit_exact_vs_oracle(oracle, name, engine):
    _fused_vs_oracle(oracle, name, 64, engine, TILINGS)


@pytest.mark.parametrize('name,engine,tilings', BIG_RUNS, ids=['%s-%s' % r[:2] for r in BIG_RUNS])
def test_fused_route_around_one_workgroup_per_compute_unit(oracle, name, engine, tilings):
    _fused_vs_oracle(oracle, name, 64, engine, tilings)


def test_fused_route_width_256_three_term_engine(oracle):
    """W = 256 'f32x3' at 65 rays of 129 samples (past the 128 mvsdf_trace_workspace_bytes assumes; two 64-lane steps and one sample of the per-ray scans)"""
    _fused_vs_oracle(oracle, 'n129', 256, 'f32x3', ((2, 3),))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the two routes against each other
@pytest.mark.parametrize('engine', ['f32', 'f32x3'])
@pytest.mark.parametrize('name', ['default', 'r08', 'render', 'st0', 'wrap'])
def test_generic_route_equals_fused_route(oracle, name, engine):
    """csrc/trace.hip promises that the generic route's decisions are bit-identical to the fused path's: with the network's own column 0 as the opaque callable
    (ops.sdf_col0: the same engine arithmetic) both routes and the oracle agree on every output and on counters[:7] (rows per stage, list lengths)."""
    c = TC.case(name)
    net, onet = _nets(64, engine)
    d = dev_case(c)
    for training in (True, False):
        want = _oracle_net_run(name, 64, engine, training)
        counts = list_counts(oracle, onet, c, training, want[3])
        sdf = Counting(lambda x: ops.sdf_col0(net, x))
        args = (d['cam_loc'], d['ray_dirs'], d['object_mask'], TC.params_tuple(c.params), training, d['intervals'], d['minsdf_steps'])
        gen = to_np(ops.trace_generic(sdf, *args))
        fus = to_np(ops.trace(net, *args))
        what = (name, engine, training)
        assert_same(gen, want, what + ('generic',))
        assert_same(fus, want, what + ('fused',))
        assert_list_counters(gen[3], counts, what + ('generic',))
        assert np.array_equal(gen[3][:7], fus[3][:7]), (what, gen[3][:7].tolist(), fus[3][:7].tolist())
        assert sum(sdf.calls) == int(want[3].sum())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# refusals: host-side checks that return before any launch (every call below still gets valid buffers of the full size)
def _refused(rc, word):
    """a negative return code and a message that names the refusal (mvsdf_last_error keeps the last one: `word` tells this one from an earlier one)"""
    from mvsdf_amd._lib import lib
    msg = lib().mvsdf_last_error()
    return rc < 0 and msg is not None and len(msg) > 0 and word in msg.decode()


def test_refusals_of_the_c_abi():
    from mvsdf_amd._lib import TraceParams, check, lib, ptr, stream_of
    L = lib()
    c = TC.case('r17')
    d = dev_case(c)
    B, P = c.ray_dirs.shape[:2]
    R = B * P
    n = c.params['n_steps']
    net, _onet = _nets(64, 'f32')
    desc = net.desc()
    om = d['object_mask'].view(torch.uint8)
    pts = torch.empty(R, 3, device='cuda'); mask = torch.empty(R, dtype=torch.uint8, device='cuda'); dists = torch.empty(R, device='cuda')
    cnt = torch.zeros(16, dtype=torch.int64, device='cuda')
    wsb_max = L.mvsdf_trace_workspace_bytes_n(R, 1025)
    ws = torch.empty(wsb_max, dtype=torch.uint8, device='cuda')
    iv = torch.linspace(0, 1, 1025).cuda()                        # long enough for every n_steps tried
    steps = torch.rand(1025).cuda()
    st = stream_of(d['ray_dirs'])

    def trace(wsb=wsb_max, **over):
        tp = TraceParams(*TC.params_tuple(dict(c.params, **over)))
        return L.mvsdf_trace(C.byref(desc), C.byref(tp), ptr(d['cam_loc']), ptr(d['ray_dirs']), ptr(om), B, P, 1, ptr(iv), ptr(steps), ptr(pts), ptr(mask),
                             ptr(dists), ptr(cnt), ptr(ws), C.c_size_t(wsb), 1, 1, st)
    assert _refused(trace(n_steps=1), 'mvsdf_trace: tracer parameters')
    assert _refused(trace(n_steps=1025), 'mvsdf_trace: tracer parameters')
    assert _refused(trace(line_step_iters=31), 'mvsdf_trace: tracer parameters')
    need = L.mvsdf_trace_workspace_bytes_n(R, n)
    assert _refused(trace(wsb=need - 1), 'mvsdf_trace: workspace')
    check(trace(wsb=need), 'mvsdf_trace')                         # ... and exactly enough is accepted

    # the generic route's entry points
    tp = TraceParams(*TC.params_tuple(c.params))
    state = torch.empty(L.mvsdf_tracegen_state_bytes(R), dtype=torch.uint8, device='cuda')
    req = torch.empty(R, 2, dtype=torch.uint8, device='cuda')
    rpts = torch.empty(R, 2, 3, device='cuda')
    geo = (ptr(d['cam_loc']), ptr(d['ray_dirs']))
    for bad in (dict(n_steps=1), dict(n_steps=1025), dict(line_step_iters=31)):
        tpb = TraceParams(*TC.params_tuple(dict(c.params, **bad)))
        assert _refused(L.mvsdf_tracegen_init(C.byref(tpb), *geo, ptr(om), B, P, ptr(state), ptr(req), ptr(rpts), ptr(cnt), st), 'mvsdf_tracegen: tracer parameters')
    check(L.mvsdf_tracegen_init(C.byref(tp), *geo, ptr(om), B, P, ptr(state), ptr(req), ptr(rpts), ptr(cnt), st), 'mvsdf_tracegen_init')
    finish = lambda wsb: L.mvsdf_tracegen_finish(C.byref(tp), *geo, B, P, 1, ptr(state), ptr(pts), ptr(mask), ptr(dists), ptr(cnt), ptr(ws), C.c_size_t(wsb), st)
    assert _refused(finish(need - 1), 'mvsdf_tracegen_finish: workspace')
    check(finish(need), 'mvsdf_tracegen_finish')
    rows = torch.empty(R * n, 3, device='cuda')
    assert _refused(L.mvsdf_tracegen_rows(C.byref(tp), 0, *geo, B, P, ptr(d['intervals']), 0, ptr(ws), ptr(rows), st), 'mvsdf_tracegen_rows')
    assert _refused(L.mvsdf_tracegen_rows(C.byref(tp), 0, *geo, B, P, ptr(d['intervals']), R + 1, ptr(ws), ptr(rows), st), 'mvsdf_tracegen_rows')
    sp = torch.empty(R, 3, device='cuda')
    vals = torch.zeros(R, device='cuda')
    assert _refused(L.mvsdf_tracegen_secant(C.byref(tp), 3, *geo, B, P, 1, ptr(vals), ptr(sp), ptr(pts), ptr(dists), ptr(cnt), ptr(ws), st), 'mvsdf_tracegen_secant')
    assert _refused(L.mvsdf_tracegen_secant(C.byref(tp), 0, *geo, B, P, 0, ptr(vals), ptr(sp), ptr(pts), ptr(dists), ptr(cnt), ptr(ws), st), 'mvsdf_tracegen_secant')
    torch.cuda.synchronize()


def test_largest_n_steps_is_accepted_on_both_routes(oracle):
    """n_steps = 1024 (the last size mvsdf_trace accepts) on 20 rays: both routes agree with the oracle"""
    c = TC.case('n1024')
    assert c.params['n_steps'] == 1024 and c.object_mask.size == 20
    d = dev_case(c)
    args = (d['cam_loc'], d['ray_dirs'], d['object_mask'], TC.params_tuple(c.params), True, d['intervals'], d['minsdf_steps'])
    assert_same(to_np(ops.trace_generic(analytic_sdf, *args)), TC.oracle_analytic('n1024', True), 'generic')
    net, _onet = _nets(64, 'f32')
    assert_same(to_np(ops.trace(net, *args)), _oracle_net_run('n1024', 64, 'f32', True), 'fused')
