"""GPU (pytest -m gpu): both routes of the HIP tracer against the C oracle at the ray, sample and geometry edges of tests/trace_cases.py, bit for bit.

  * the GENERIC route (ops.trace_generic: k_gen_init / k_gen_step / k_gen_finish / k_gen_lists / k_gen_rows / k_gen_secant / k_gen_sort_list around an opaque
    `sdf` callable) with the analytic SDF, every row of the table, training and eval;
  * the FUSED route (ops.trace) with the W = 64, 256 and 512 networks on the fmaf-chain engine ('f32'), the three-term engine ('f32x3') and bf16-rounded
    weights ('bf16w'), at (mt, mt_samples) in {(1, 1), (2, 3), (4, 4)} -- at W = 512 a request of 4 row tiles is clamped to 2 -- both as the one call and as its
    launches one by one with the secant chains alone (mvsdf_trace_stage 1, 3, 7, 5: what the native step launches);
  * the two routes against each other with `sdf = ops.sdf_col0(net, .)`;
  * the split engines ('bf16x2', 'bf16x3'), which have no bit-level CPU model (their softplus uses the hardware exp / log): the exact identities that remain --
    every tiling and the staged form give the same bits, the generic route around ops.sdf_col0 equals the fused route -- with the lists the table declares
    filled asserted non-empty from the device counters, so that no identity passes empty.  (Their arithmetic is held to the oracle by
    tests/test_gpu_bf16s.py; its tracer comparison exempts every ray within 1e-6 of a decision, which is every secant ray: DESIGN.md.)
  * the host-side refusals of the C ABI.

Where each instance csrc/trace_route.h can return runs (<row tiles, column tiles per wave, waves>; every id below covers r7 ... r33, n13, n129 and wrap):
    k_sphere_trace (mv_route_sphere)          F32 W < 256   <1|2|4, 4, 4>   test_fused_route_bit_exact_vs_oracle[*-f32], [*-bf16w]
                                              F32 W = 256   <1|2|4, 2, 8>   test_fused_route_wide_bit_exact_vs_oracle[*-f32-256], [*-bf16w-256]
                                              X3  W <= 256  <1, 1, 16>, <2|4, 2, 8>   test_fused_route_bit_exact_vs_oracle[*-f32x3], ..._wide_...[*-f32x3-256]
                                              BS2 / BS3 W <= 256   <1|2|4, 2, 8>   test_split_engines_tilings_give_the_same_bits[64-*-bf16x2], [256-*-bf16x3], ...
                                              any W = 512   <1|2, 4, 8>   ..._wide_...[*-f32-512], [*-bf16w-512], [*-f32x3-512], test_split_engines_...[512-*-bf16x2], ...
    k_ray_samples (mv_route_samples)          the same ladder over mt_samples = 1, 3 (-> 2), 4, in the same tests (part 1: one row tile up to 4096 rays, X3 at most two)
    the secant chains alone (mv_route_secant) X3 W <= 256   k_secant_chains<1, 1, 16>; every other engine and width: the k_ray_samples instance of mt_samples --
                                              the staged run (stage 7) of the same tests

Every comparison is np.array_equal on points, mask, dists and the row counters over ALL rays (the oracle's sphere intersection is the kernel's): the project's
rule for the bit-exact arithmetics, no tolerance.  tests/test_trace_cases_host.py holds the table to the branches these tests rely on."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import trace_cases as TC
from helpers import analytic_sdf, sdf_packed_net
from mvsdf_amd import ops
from mvsdf_amd.utils import synth

pytestmark = pytest.mark.gpu

CNT_N_SECANT, CNT_N_SAMPLER, CNT_N_MINSDF, CNT_TAIL_WGS = 4, 5, 6, 11        # include/mvsdf_hip.h MVSDF_CNT_*
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


def assert_tail_counter(cnt, engine, W, R, mt, training, what):
    """counters[MVSDF_CNT_TAIL_WGS]: under tail filling every sphere-tracing workgroup counts itself once when its rays are done, without it nobody does.  So the
    counter is the sphere kernel's grid at the EFFECTIVE row tiles (W = 512: at most 2) where csrc/trace_route.h::mv_tail_on says on -- training, the fp32-MFMA
    engines always, 'f32x3' above 2048 rays, the split engines only under MVSDF_TAIL=2, and at most one workgroup per compute unit -- and 0 elsewhere."""
    grid = -(-R // (8 * (min(mt, 2) if W > 256 else mt)))
    need = 1 if engine in ('f32', 'bf16w') or (engine == 'f32x3' and R > 2048) else 2
    on = training and int(os.environ.get('MVSDF_TAIL', '1')) >= need and grid <= torch.cuda.get_device_properties(0).multi_processor_count
    assert int(cnt[CNT_TAIL_WGS]) == (grid if on else 0), (what, 'tail filling', on, grid, int(cnt[CNT_TAIL_WGS]))


class Counting:
    """An opaque `sdf` callable that records how many rows each call got"""

    def __init__(self, fn, column=False):
        self.fn, self.calls, self.column = fn, [], column

    def __call__(self, x):
        assert x.dim() == 2 and x.shape[1] == 3 and x.shape[0] > 0
        self.calls.append(int(x.shape[0]))
        y = self.fn(x)
        return y.reshape(-1, 1) if self.column else y


def trace_staged(net, d, c, training, mt, mts, stages=(1, 3, 7, 5)):
    """The launches of ops.trace one by one through the C ABI: sphere tracing (1), the sampler rows (3), the secant chains ALONE in the form
    csrc/trace_route.h::mv_route_secant picks (7), the min-sdf rows alone (5).  Same outputs, same counters as the one call."""
    from mvsdf_amd._lib import TraceParams, check, lib, ptr, stream_of
    B, P = c.ray_dirs.shape[:2]
    R = B * P
    tp = TraceParams(*TC.params_tuple(c.params))
    desc = net.desc()
    om = d['object_mask'].view(torch.uint8)
    pts = torch.empty(R, 3, device='cuda'); mask = torch.empty(R, dtype=torch.uint8, device='cuda'); dists = torch.empty(R, device='cuda')
    cnt = torch.empty(16, dtype=torch.int64, device='cuda')
    wsb = lib().mvsdf_trace_workspace_bytes_n(R, tp.n_steps)
    ws = torch.empty(wsb, dtype=torch.uint8, device='cuda')
    for stage in stages:
        check(lib().mvsdf_trace_stage(stage, C.byref(desc), C.byref(tp), ptr(d['cam_loc']), ptr(d['ray_dirs']), ptr(om), B, P, 1 if training else 0, ptr(d['intervals']),
                                      ptr(d['minsdf_steps']), ptr(pts), ptr(mask), ptr(dists), ptr(cnt), ptr(ws), C.c_size_t(wsb), mt, mts, stream_of(d['ray_dirs'])),
              'mvsdf_trace_stage(%d)' % stage)
    return pts, mask.view(torch.bool), dists, cnt


def assert_identical(got, ref, what):
    """two runs of the library: points, mask, dists of all rays and counters[:7] (rows per stage, list lengths), bit for bit"""
    for a, b, k in zip(got[:3], ref[:3], ('points', 'mask', 'dists')):
        assert np.array_equal(a, b), (what, k, int((a != b).sum()))
    assert np.array_equal(got[3][:7], ref[3][:7]), (what, got[3][:7].tolist(), ref[3][:7].tolist())


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
        ref = None
        for mt, mts in tilings:
            what = (name, W, engine, 'train' if training else 'eval', mt, mts)
            got = to_np(ops.trace(net, d['cam_loc'], d['ray_dirs'], d['object_mask'], TC.params_tuple(c.params), training, d['intervals'], d['minsdf_steps'],
                                  mt=mt, mt_samples=mts))
            assert_same(got, want, what)
            assert_list_counters(got[3], counts, what)
            assert_tail_counter(got[3], engine, W, c.object_mask.size, mt, training, what)
            staged = to_np(trace_staged(net, d, c, training, mt, mts))
            assert_tail_counter(staged[3], engine, W, c.object_mask.size, mt, training, what + ('staged',))
            assert_same(staged, want, what + ('staged',))
            assert_identical(staged, got, what + ('staged',))
            ref = got if ref is None else ref
            assert_identical(got, ref, what + tilings[0])        # (follows from the above; at W = 512 this is the clamped request (4, 4) against (2, 3))


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


# W = 256 and W = 512 (the reference's shipped width): the rows of trace_cases.WIDE.  The instruction model of 'f32x3' is slow at W = 512: a subset there, and no big row.
WIDE = tuple(TC.WIDE)
X3_512 = ('one', 'r7', 'r8', 'r9', 'r15', 'r16', 'r17', 'r31', 'r33', 'n2', 'n13', 'n129', 'wrap', 'miss7')
WIDE_RUNS = [(n, e, W) for W in TC.WIDE_WIDTHS for e in ('f32', 'bf16w') for n in WIDE] + [(n, 'f32x3', 256) for n in WIDE] + [(n, 'f32x3', 512) for n in X3_512]
# tail filling on / off one ray later (assert_tail_counter holds the pair to on / off on a device of 256 compute units): 'f32x3' (above 2048 rays only) at mt = 2, W = 256: a grid of 256 / 257; 'f32' at W = 512, where the EFFECTIVE mt of a request
# of 4 is 2 -- the same on / off pair for (2, 3) and (4, 4); 'f32' at W = 256 and mt = 1
WIDE_BIG_RUNS = [('r4096', 'f32x3', 256, ((2, 3),)), ('r4097', 'f32x3', 256, ((2, 3),)), ('r4096', 'f32', 512, ((2, 3), (4, 4))), ('r4097', 'f32', 512, ((2, 3), (4, 4))),
                 ('r2048', 'f32', 256, ((1, 1),)), ('r2049', 'f32', 256, ((1, 1),))]


@pytest.mark.parametrize('name,engine,W', WIDE_RUNS, ids=['%s-%s-%d' % r for r in WIDE_RUNS])
def test_fused_route_wide_bit_exact_vs_oracle(oracle, name, engine, W):
    assert TC.declared(name, W) is not None
    _fused_vs_oracle(oracle, name, W, engine, TILINGS)


@pytest.mark.parametrize('name,engine,W,tilings', WIDE_BIG_RUNS, ids=['%s-%s-%d' % r[:3] for r in WIDE_BIG_RUNS])
def test_fused_route_wide_around_one_workgroup_per_compute_unit(oracle, name, engine, W, tilings):
    _fused_vs_oracle(oracle, name, W, engine, tilings)


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
# the split engines: exact identities on the edge rows
SPLIT = ('bf16x2', 'bf16x3')
SPLIT_WIDE = X3_512 + ('st0', 'b4', 'om_none')
SPLIT_TILING_RUNS = [(64, n) for n in SMALL] + [(W, n) for W in TC.WIDE_WIDTHS for n in SPLIT_WIDE]
SPLIT_ROUTE_RUNS = [(64, n) for n in ('default', 'r08', 'render', 'st0', 'wrap', 'n129', 'r17', 'b4')] + [(W, n) for W in TC.WIDE_WIDTHS for n in ('r17', 'n13', 'wrap')]


@functools.lru_cache(maxsize=None)
def _split_net(W, engine):
    return ops.pack_trace_net(sdf_packed_net(synth.make_state_dict(W, 0)), engine)


def assert_declared_lists_filled(cnt, name, W, training, what):
    """The non-vacuity guard: the lists the table declares filled for the width-W network (on fp32 arithmetic, training) hold rays on this engine too.  The
    rounded weights move a count by a ray or two, never to zero where the table says Y (Y: at least 3 rays at the wide networks) -- but for the single ray of the
    rows in trace_cases.ROUNDED_EMPTY (tests/test_trace_cases_host.py holds both statements on the oracle of the rounded weights).  Eval has no min-sdf list."""
    if (W, name) in TC.ROUNDED_EMPTY:
        return
    for k, want, in_eval in zip((CNT_N_SAMPLER, CNT_N_SECANT, CNT_N_MINSDF), TC.declared(name, W), (True, True, False)):
        if want is True and (training or in_eval):
            assert int(cnt[k]) > 0, (what, 'the list of counter %d is empty' % k, cnt[:7].tolist())


@pytest.mark.parametrize('engine', SPLIT)
@pytest.mark.parametrize('W,name', SPLIT_TILING_RUNS, ids=['%d-%s' % r for r in SPLIT_TILING_RUNS])
def test_split_engines_tilings_give_the_same_bits(W, name, engine):
    """(a) every (mt, mt_samples) of TILINGS, as one call and as the staged launches: the same points, mask, dists and counters[:7]"""
    c = TC.case(name)
    net = _split_net(W, engine)
    assert net.trace_dtype == ops.TRACE_DTYPES[engine]
    d = dev_case(c)
    for training in (True, False):
        ref = None
        for mt, mts in TILINGS:
            what = (name, W, engine, 'train' if training else 'eval', mt, mts)
            got = to_np(ops.trace(net, d['cam_loc'], d['ray_dirs'], d['object_mask'], TC.params_tuple(c.params), training, d['intervals'], d['minsdf_steps'],
                                  mt=mt, mt_samples=mts))
            assert_declared_lists_filled(got[3], name, W, training, what)
            assert_tail_counter(got[3], engine, W, c.object_mask.size, mt, training, what)
            ref = got if ref is None else ref
            assert_identical(got, ref, what + TILINGS[0])
            assert_identical(to_np(trace_staged(net, d, c, training, mt, mts)), ref, what + ('staged',))


@pytest.mark.parametrize('engine', SPLIT)
@pytest.mark.parametrize('W,name', SPLIT_ROUTE_RUNS, ids=['%d-%s' % r for r in SPLIT_ROUTE_RUNS])
def test_split_engines_generic_route_equals_fused_route(W, name, engine):
    """(b) csrc/trace.hip's promise for ONE engine arithmetic, on the split engines: the generic route around ops.sdf_col0 (the row-sample kernels' weight fetch)
    and the fused route (k_sphere_trace carries its weights across layers) agree on every output and on counters[:7]; the callable saw exactly the rows counted."""
    c = TC.case(name)
    net = _split_net(W, engine)
    d = dev_case(c)
    for training in (True, False):
        sdf = Counting(lambda x: ops.sdf_col0(net, x))
        args = (d['cam_loc'], d['ray_dirs'], d['object_mask'], TC.params_tuple(c.params), training, d['intervals'], d['minsdf_steps'])
        gen = to_np(ops.trace_generic(sdf, *args))
        fus = to_np(ops.trace(net, *args))
        what = (name, W, engine, 'train' if training else 'eval')
        assert_declared_lists_filled(fus[3], name, W, training, what)
        assert_identical(gen, fus, what)
        assert sum(sdf.calls) == int(gen[3][:4].sum()) == int(fus[3][:4].sum())


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
