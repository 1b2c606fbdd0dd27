"""The weight preparation every matrix-core kernel reads, element by element: the weight-norm fold w = g v / |v| and the lane-order packs of w (csrc/basic.hip).

Part one holds the stand-alone kernels (mvsdf_fold_pack, mvsdf_fold_pack_net, mvsdf_pack_bf16w_net, mvsdf_pack_bf16s_net, mvsdf_pack_bf16x3_net,
mvsdf_pack_bf16x3t_net) bit for bit to the numpy restatement of tests/pack_ref.py, at shapes on both sides of every tile, k-block and fold-chunk edge
(pack_ref.SHAPE_GROUPS) and on values at the edges of the three-term split (pack_ref.VALUES).  Every output buffer is allocated larger than its size function
says and pre-filled with a byte pattern, twice with two patterns: the bytes beyond the stated size must keep the pattern, the bytes inside it must come out
the same under both patterns (so each of them was written), dense content must equal the restatement and every pad element must be +0.

Part two holds the native step's prologue (k_step_prologue: fold, five packs, camera rays in one launch) to those stand-alone kernels, on networks
away from the geometric initialisation, through the inspection offsets of NativeStep.pack_offsets.  Nothing is asserted on what the step computes from them.
Both sides take the layout, the split, the fold chain and the camera ray from one definition each (csrc/pack_layout.h, basic.hip::mv_norm_chain,
mv_camera_ray; the layout is held to pack_ref on the CPU by tests/test_pack_layout_host.py): what this part alone holds is the prologue's own schedule --
where its row groups' blocks go in every pack, its register-resident form of the fold chain, the index arithmetic of its ray workgroups.

Input domain of the bf16 packs: finite weights with a finite bf16 rounding (|w| <= 0x7f7f7fff as a bit pattern)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import pack_ref as PR
from helpers import t
from mvsdf_amd import ops
from mvsdf_amd._lib import check, lib, stream_of

pytestmark = pytest.mark.gpu

PATTERNS = (0xa5, 0x5a)
TAIL = 256                                       # bytes allocated beyond what the size function states
GROUPS = [0, 1]
SCALES = (-40, -10, 0, 10, 40)


def _bf16_bytes(N, K):
    return int(lib().mvsdf_packed_bf16_bytes(N, K))


def _f32_bytes(N, K):
    return 4 * int(lib().mvsdf_packed_floats(N, K))


def test_size_functions_match_the_restatement():
    for N, K in PR.SHAPES:
        assert _f32_bytes(N, K) == 4 * PR.packed_floats(N, K) and _f32_bytes(K, N) == 4 * PR.packed_floats(K, N)
        assert _bf16_bytes(N, K) == 2 * PR.packed_bf16_elems(N, K) and _bf16_bytes(K, N) == 2 * PR.packed_bf16_elems(K, N)


def _guarded(call, sizes, dtype):
    """call(list of device uint8 buffers) under both fill patterns -> the buffers' contents inside their stated sizes, as numpy arrays of `dtype`.
    sizes: one list of byte counts per output kind (call receives one list of buffers per kind)."""
    results = []
    for pattern in PATTERNS:
        bufs = [[torch.full((n + TAIL,), pattern, dtype=torch.uint8, device='cuda') for n in kind] for kind in sizes]
        call(*bufs)
        torch.cuda.synchronize()
        res = []
        for kind, bk in zip(sizes, bufs):
            row = []
            for n, b in zip(kind, bk):
                h = b.cpu().numpy()
                assert (h[n:] == pattern).all(), 'a byte beyond the stated size was written'
                row.append(h[:n].copy())
            res.append(row)
        results.append(res)
    for ka, kb in zip(*results):
        for a, b in zip(ka, kb):
            assert np.array_equal(a, b), 'a byte inside the stated size keeps the fill pattern (never written)'
    return [[a.view(dtype) for a in kind] for kind in results[0]]


def _ints(vals):
    return (C.c_int * len(vals))(*vals)


_CACHE = {}


def _weights(group):
    """the group's matrices with pack_ref.VALUES planted (host float32 arrays) and their device copies"""
    if ('w', group) not in _CACHE:
        ws = []
        for l, (N, K) in enumerate(PR.SHAPE_GROUPS[group]):
            rng = np.random.default_rng(100 * group + l)
            w = (rng.standard_normal((N, K)) * np.exp2(rng.integers(-3, 4, (N, 1)))).astype(np.float32)
            ws.append(PR.plant(w, l))
        _CACHE[('w', group)] = (ws, [t(w) for w in ws])
    return _CACHE[('w', group)]


def _check_f32_pack(wp, N, K, dense_bits, what):
    got, pads = PR.unpack_f32(wp.view(np.uint32), N, K)
    assert np.array_equal(got, dense_bits), what
    assert not wp.view(np.uint32)[pads].any(), what + ': a pad element is not +0'


def _check_x3_pack(wp, N, K, w, what):
    got, pads = PR.unpack_bf16x3(wp, N, K)
    assert np.array_equal(got, PR.split3(w)), what
    assert not wp[pads].any(), what + ': a pad element is not +0'


# ================================================================================================ the bf16 / rounded packs: w fed directly
@pytest.mark.parametrize('group', GROUPS)
def test_pack_bf16w_net(group):
    """fp32 pack of the bf16-rounded weights (trace_dtype 2)"""
    shapes = PR.SHAPE_GROUPS[group]
    ws, wd = _weights(group)
    N, K = _ints([s[0] for s in shapes]), _ints([s[1] for s in shapes])
    call = lambda out: check(lib().mvsdf_pack_bf16w_net(len(shapes), ops._ptr_array(wd), N, K, ops._ptr_array(out), stream_of(wd[0])), 'mvsdf_pack_bf16w_net')
    (packs,) = _guarded(call, [[_f32_bytes(n, k) for n, k in shapes]], np.float32)
    for (n, k), w, wp in zip(shapes, ws, packs):
        _check_f32_pack(wp, n, k, PR.bits(PR.bf16_value(PR.bf16_bits(w))), 'bf16w %dx%d' % (n, k))


@pytest.mark.parametrize('group', GROUPS)
def test_pack_bf16s_net(group):
    """the one-term bf16 pack (trace_dtype 3 / 4)"""
    shapes = PR.SHAPE_GROUPS[group]
    ws, wd = _weights(group)
    N, K = _ints([s[0] for s in shapes]), _ints([s[1] for s in shapes])
    call = lambda out: check(lib().mvsdf_pack_bf16s_net(len(shapes), ops._ptr_array(wd), N, K, ops._ptr_array(out), stream_of(wd[0])), 'mvsdf_pack_bf16s_net')
    (packs,) = _guarded(call, [[_bf16_bytes(n, k) for n, k in shapes]], np.uint16)
    for (n, k), w, wp in zip(shapes, ws, packs):
        got, pads = PR.unpack_bf16(wp, n, k)
        assert np.array_equal(got, PR.bf16_bits(w)), (n, k)
        assert not wp[pads].any(), (n, k)


@pytest.mark.parametrize('group', GROUPS)
def test_pack_bf16x3_net(group):
    """the three-term pack of W (trace_dtype 5, the x3 chains): dense terms == split3(w), which carries the flush rule and the exactness"""
    shapes = PR.SHAPE_GROUPS[group]
    ws, wd = _weights(group)
    N, K = _ints([s[0] for s in shapes]), _ints([s[1] for s in shapes])
    call = lambda out: check(lib().mvsdf_pack_bf16x3_net(len(shapes), ops._ptr_array(wd), N, K, ops._ptr_array(out), stream_of(wd[0])), 'mvsdf_pack_bf16x3_net')
    (packs,) = _guarded(call, [[3 * _bf16_bytes(n, k) for n, k in shapes]], np.uint16)
    for (n, k), w, wp in zip(shapes, ws, packs):
        _check_x3_pack(wp, n, k, w, 'x3 %dx%d' % (n, k))


@pytest.mark.parametrize('group', GROUPS)
def test_pack_bf16x3t_net(group):
    """the three-term pack of W^T from W: equal to the restatement of the transposed matrix"""
    shapes = PR.SHAPE_GROUPS[group]
    ws, wd = _weights(group)
    N, K = _ints([s[0] for s in shapes]), _ints([s[1] for s in shapes])
    call = lambda out: check(lib().mvsdf_pack_bf16x3t_net(len(shapes), ops._ptr_array(wd), N, K, ops._ptr_array(out), stream_of(wd[0])), 'mvsdf_pack_bf16x3t_net')
    (packs,) = _guarded(call, [[3 * _bf16_bytes(k, n) for n, k in shapes]], np.uint16)
    for (n, k), w, wp in zip(shapes, ws, packs):
        _check_x3_pack(wp, k, n, np.ascontiguousarray(w.T), 'x3t %dx%d' % (n, k))


# ================================================================================================ the fold and the fp32 packs of W and W^T
def _fold_inputs(N, K, seed, zero_row=None, row_scales=True):
    """v with magnitudes in [0.25, 1] and random signs (so that every partial sum of squares is a normal number at every scale of SCALES), rows scaled by
    2^s with s cycling through SCALES; g in +-[0.5, 2] with one zero where there are three rows or more"""
    rng = np.random.default_rng(seed)
    v = (rng.uniform(0.25, 1.0, (N, K)) * rng.choice([-1.0, 1.0], (N, K))).astype(np.float32)
    if row_scales:
        v = (v * np.exp2(np.array(SCALES, dtype=np.float64)[np.arange(N) % len(SCALES)])[:, None]).astype(np.float32)
    g = (rng.uniform(0.5, 2.0, (N, 1)) * np.where(np.arange(N)[:, None] % 2 == 0, 1.0, -1.0)).astype(np.float32)
    if N >= 3:
        g[N // 2] = 0.0
    if zero_row is not None:
        v[zero_row] = 0.0
    return v, g


def _assert_ss_normal(v, skip_row=None):
    """Every partial sum of the oracle's k-ascending chain ss = fmaf(v_k, v_k, ss) is a normal float32: the chain grows monotonically, so it lies between the
    first square and the full sum, both taken here in float64 (exact squares of float32 values)."""
    sq = v.astype(np.float64) ** 2
    rows = np.ones(v.shape[0], bool)
    if skip_row is not None:
        rows[skip_row] = False
    assert (sq[rows, 0] >= 2.0 ** -125).all() and (sq[rows].sum(1) <= 2.0 ** 126).all()


def _assert_fold_equal(got, ref, nan_row=None):
    """bit for bit; the all-zero row: NaN on both sides (payloads not compared)"""
    nan = np.isnan(ref)
    if nan_row is None:
        assert not nan.any()
    else:
        expect = np.zeros(ref.shape, bool)
        expect[nan_row] = True
        assert np.array_equal(nan, expect)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(PR.bits(got)[~nan], PR.bits(ref)[~nan])


@pytest.mark.parametrize('N,K', PR.SHAPES, ids=['%dx%d' % s for s in PR.SHAPES])
def test_fold_pack(N, K):
    """mvsdf_fold_pack: w == orc_fold bit for bit (rows at five scales, g of both signs and zero), wp / wpT == the restatement of W / W^T"""
    v, g = _fold_inputs(N, K, 7 * N + K)
    _assert_ss_normal(v)
    ref = PR.fold(v, g)
    vd, gd = t(v), t(g.reshape(-1))
    call = lambda w, wp, wpT: check(lib().mvsdf_fold_pack(C.c_void_p(vd.data_ptr()), C.c_void_p(gd.data_ptr()), N, K, C.c_void_p(w[0].data_ptr()),
                                                          C.c_void_p(wp[0].data_ptr()), C.c_void_p(wpT[0].data_ptr()), stream_of(vd)), 'mvsdf_fold_pack')
    (w,), (wp,), (wpT,) = _guarded(call, [[4 * N * K], [_f32_bytes(N, K)], [_f32_bytes(K, N)]], np.float32)
    w = w.reshape(N, K)
    _assert_fold_equal(w, ref)
    _check_f32_pack(wp, N, K, PR.bits(ref), 'wp')
    _check_f32_pack(wpT, K, N, PR.bits(np.ascontiguousarray(ref.T)), 'wpT')


# layer of each group without weight norm (g = None: w = v) and (layer, row) of the all-zero row
NO_G = {0: 3, 1: 4}
ZERO_ROW = {0: (6, 9), 1: (7, 17)}             # (rows with g != 0: g / 0 = inf, 0 * inf = NaN)


def _net_case(group):
    if ('net', group) not in _CACHE:
        shapes = PR.SHAPE_GROUPS[group]
        vs, gs = [], []
        for l, (N, K) in enumerate(shapes):
            zl, zr = ZERO_ROW[group]
            v, g = _fold_inputs(N, K, 1000 * group + l, zero_row=zr if l == zl else None)
            _assert_ss_normal(v, zr if l == zl else None)
            vs.append(v)
            gs.append(None if l == NO_G[group] else g)
        refs = [PR.fold(v, g) for v, g in zip(vs, gs)]
        _CACHE[('net', group)] = (vs, gs, refs)
    return _CACHE[('net', group)]


@pytest.mark.parametrize('group', GROUPS)
def test_fold_pack_net(group):
    """mvsdf_fold_pack_net on a whole group in one call: w == orc_fold (one layer without g: w == v; one all-zero row: NaN there on both sides, its
    neighbours untouched), wp / wpT == the restatement; then ops.fold_pack_net and the flat route (ops.fold_pack_net_flat with a FoldPlan): the same bits.

    Subnormal intermediates are kept out of these cases (see _fold_inputs and _assert_ss_normal).  Observed on one MI355X with rows scaled by 2^-55 .. 2^-80
    (17 x 39, 5 x 256, 5 x 577; squares and sums of squares down to 2^-156, far into the subnormals and to the underflow of the first squares, where the
    quotient g / sqrt(ss) overflows to inf): mvsdf_fold_pack and mvsdf_fold_pack_net gave orc_fold's bits there too -- no difference to report."""
    shapes = PR.SHAPE_GROUPS[group]
    vs, gs, refs = _net_case(group)
    n = len(shapes)
    vd = [t(v) for v in vs]
    gd = [None if g is None else t(g.reshape(-1)) for g in gs]
    N, K = _ints([s[0] for s in shapes]), _ints([s[1] for s in shapes])
    call = lambda w, wp, wpT: check(lib().mvsdf_fold_pack_net(n, ops._ptr_array(vd), ops._ptr_array(gd), N, K, ops._ptr_array(w), ops._ptr_array(wp),
                                                              ops._ptr_array(wpT), stream_of(vd[0])), 'mvsdf_fold_pack_net')
    ws, wps, wpTs = _guarded(call, [[4 * a * b for a, b in shapes], [_f32_bytes(a, b) for a, b in shapes], [_f32_bytes(b, a) for a, b in shapes]], np.float32)
    zl, zr = ZERO_ROW[group]
    for l, (a, b) in enumerate(shapes):
        w = ws[l].reshape(a, b)
        _assert_fold_equal(w, refs[l], zr if l == zl else None)
        if gs[l] is None:
            assert np.array_equal(PR.bits(w), PR.bits(vs[l]))
        _check_f32_pack(wps[l], a, b, PR.bits(w), 'wp of layer %d' % l)                   # (bits of the device's own w: the NaN row travels as it is)
        _check_f32_pack(wpTs[l], b, a, PR.bits(np.ascontiguousarray(w.T)), 'wpT of layer %d' % l)
    # the per-layer route of ops
    w2, wp2, wpT2 = ops.fold_pack_net(vd, [None if g is None else g.reshape(-1, 1) for g in gd])
    for l in range(n):
        assert np.array_equal(w2[l].cpu().numpy().view(np.uint32).reshape(-1), ws[l].view(np.uint32))
        assert np.array_equal(wp2[l].cpu().numpy().view(np.uint32), wps[l].view(np.uint32))
        assert np.array_equal(wpT2[l].cpu().numpy().view(np.uint32), wpTs[l].view(np.uint32))
    # the flat route
    plan = ops.FoldPlan([tuple(s) for s in shapes], [n])
    layers = [ops.PackedLayer() for _ in shapes]
    bs = [torch.zeros(a, device='cuda') for a, _ in shapes]
    flat, packs = ops.fold_pack_net_flat(plan, vd, gd, bs, layers)
    flat, packs = flat.cpu().numpy().view(np.uint32), packs.cpu().numpy().view(np.uint32)
    for l, (a, b) in enumerate(shapes):
        assert np.array_equal(flat[plan.woff[l]:plan.woff[l] + a * b], ws[l].view(np.uint32))
        assert np.array_equal(packs[plan.poff[l]:plan.poff[l] + PR.packed_floats(a, b)], wps[l].view(np.uint32))
        assert np.array_equal(packs[plan.pToff[l]:plan.pToff[l] + PR.packed_floats(b, a)], wpTs[l].view(np.uint32))


@pytest.mark.parametrize('group', GROUPS)
def test_fold_is_invariant_under_power_of_two_scales(group):
    """fold(2^s v, g) == fold(v, g) bit for bit for s in SCALES (ss scales by 4^s exactly while it stays a normal number), on the device and in the oracle"""
    shapes = PR.SHAPE_GROUPS[group]
    base = [_fold_inputs(N, K, 50 * group + l, row_scales=False) for l, (N, K) in enumerate(shapes)]
    gd = [t(g) for _, g in base]
    ref = None
    for s in SCALES:
        vs = [(v * np.float32(2.0 ** s)).astype(np.float32) for v, _ in base]
        for v in vs:
            _assert_ss_normal(v)
        w, _, _ = ops.fold_pack_net([t(v) for v in vs], gd)
        w = [x.cpu().numpy() for x in w]
        for l, (v, (_, g)) in enumerate(zip(vs, base)):
            assert np.array_equal(PR.bits(w[l]), PR.bits(PR.fold(v, g))), (s, l)
        if ref is None:
            ref = w
        for l in range(len(shapes)):
            assert np.array_equal(PR.bits(w[l]), PR.bits(ref[l])), (s, l)


# ================================================================================================ the step prologue against the stand-alone kernels
TRACE_DTYPES = ['f32', 'bf16w', 'bf16x2', 'f32x3']
B, P = 1, 96


def _trained_like(W):
    """synth.make_state_dict(W, 0) moved away from the geometric initialisation: every row of every weight_v scaled by 2^s, |s| <= 8, every weight_g by a
    factor in +-[0.5, 2]; about 1 % of the entries of v set to 2^-50 of their row's norm (their folded values fall below the 2^-40 flush of the three-term
    packs) and about 1 % so that their folded values fall into [2^-40, 2^-39) (kept; a flush threshold one binade off would lose them)."""
    from mvsdf_amd.utils import synth
    sd = synth.make_state_dict(W, 0)
    rng = np.random.default_rng(W)
    for key in [k for k in sd if k.endswith('weight_v')]:
        v = sd[key].astype(np.float64) * np.exp2(rng.integers(-8, 9, (sd[key].shape[0], 1)))
        gk = key[:-1] + 'g'
        g = sd[gk].astype(np.float64) * rng.uniform(0.5, 2.0, sd[gk].shape) * rng.choice([-1.0, 1.0], sd[gk].shape)
        nrm = np.sqrt((v * v).sum(1, keepdims=True))
        u = rng.random(v.shape)
        v = np.where(u < 0.01, 2.0 ** -50 * nrm, v)
        v = np.where((u >= 0.01) & (u < 0.02), 1.5 * 2.0 ** -40 * nrm / np.abs(g), v)
        sd[key], sd[gk] = v.astype(np.float32), g.astype(np.float32)
        assert np.isfinite(sd[key]).all() and np.isfinite(sd[gk]).all() and (np.abs(sd[key]).max(1) > 0).all()
    return sd


def _region(u8, off, nbytes, dtype):
    return u8[off:off + nbytes].view(dtype)


@pytest.mark.parametrize('dtype', TRACE_DTYPES)
@pytest.mark.parametrize('W', [64, 256, 512])
def test_step_prologue_equals_the_standalone_kernels(W, dtype):
    """One training forward (B = 1, 96 rays) of an IDRNetwork on trained-like parameters; then, for every layer of both networks, the forward block's
    w == orc_fold(v, g) and its wp, wpT, wp16, wx3, wx3T == what the stand-alone entry points write for that w (all bit for bit, pads +0), the bias copy ==
    the bias, and the block's ray_dirs / cam_loc == ops.camera_rays.  The trace dtypes cover the prologue's wp16 forms (absent, rounded fp32 pack, one-term
    bf16 pack, three-term pack) and wx3 separate from / shared with wp16."""
    _prologue_case(W, dtype, B, P)


@pytest.mark.parametrize('B,P', [(1, 1025), (2, 513)], ids=['1x1025', '2x513'])
def test_step_prologue_at_ray_workgroup_edges(B, P):
    """The same comparison, every region, at the two edges of the prologue's 1024-lane ray workgroups that 96 rays of one view do not reach: a second ray
    workgroup that holds a single ray (1 x 1025), and the view boundary inside the first workgroup, where lane 513 writes the cam_loc of view 1 (2 x 513)."""
    _prologue_case(64, 'f32x3', B, P)


def _prologue_case(W, dtype, B, P):
    from mvsdf_amd.model.implicit_differentiable_renderer import IDRNetwork
    from mvsdf_amd.utils import synth
    from mvsdf_amd.utils.config import ConfigDict
    sd = _trained_like(W)
    model = IDRNetwork(ConfigDict(synth.model_conf(W)))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.cuda()
    model.set_trace_dtype(dtype)
    model.train()
    inp, _ = synth.make_batch(B, P, 0, seed=0, with_features=False)
    torch.manual_seed(5)
    out = model({k: t(v) for k, v in inp.items()}, 0.3)
    rec = getattr(model, '_last_rec', lambda: None)()
    assert rec is not None, 'the native step refused this model (width %d, %d rays)' % (W, B * P)
    torch.cuda.synchronize()
    st, fwd = rec.step, rec.fwd
    u8 = fwd.u8.cpu().numpy()
    vs, gs, bs = rec.vs, rec.gs, rec.bs
    n_sdf, nl = st.desc.n_sdf, st.nl
    assert nl == len(vs) == 14 and n_sdf == 9
    shapes = [tuple(v.shape) for v in vs]
    Ks = [k for _, k in shapes]
    # the three cases of the prologue's fold chain: a partial 64-chunk alone, full chunks alone, a partial chunk after full ones
    assert any(k < 64 for k in Ks) and any(k % 64 == 0 for k in Ks) and any(k > 64 and k % 64 for k in Ks)
    assert Ks[0] == 39 and Ks[n_sdf] == 289 and W in Ks
    offs = [st.pack_offsets(l) for l in range(nl)]
    td = ops.TRACE_DTYPES[dtype]
    below = kept = 0
    w_dev = []
    for l, (N, K) in enumerate(shapes):
        o = offs[l]
        ref = PR.fold(vs[l].detach().cpu().numpy(), gs[l].detach().cpu().numpy())
        w = _region(u8, o['w'], 4 * N * K, np.float32).reshape(N, K)
        assert np.isfinite(ref).all() and np.array_equal(PR.bits(w), PR.bits(ref)), 'w of layer %d' % l
        below += int(((np.abs(ref) < 2.0 ** -40) & (ref != 0)).sum())
        kept += int(((np.abs(ref) >= 2.0 ** -40) & (np.abs(ref) < 2.0 ** -39)).sum())
        w_dev.append(fwd.f(o['w'], (N, K)).clone())
    assert below > 100 and kept > 100                                   # values on both sides of the flush threshold reached the packs
    # what the stand-alone entry points write for the block's w
    _, wp_ref, wpT_ref = ops.fold_pack_net(w_dev, [None] * nl)
    for l, (N, K) in enumerate(shapes):
        o = offs[l]
        for name, ref_pack, (a, b) in (('wp', wp_ref[l], (N, K)), ('wpT', wpT_ref[l], (K, N))):
            got = _region(u8, o[name], _f32_bytes(a, b), np.uint32)
            assert np.array_equal(got, ref_pack.cpu().numpy().view(np.uint32)), '%s of layer %d' % (name, l)
            assert not got[PR.unpack_f32(got, a, b)[1]].any()
    sdf = list(range(n_sdf))
    Ns, Kk = _ints([shapes[l][0] for l in sdf]), _ints([shapes[l][1] for l in sdf])
    wptr = ops._ptr_array([w_dev[l] for l in sdf])
    s = stream_of(w_dev[0])

    def standalone(fn, sizes):
        bufs = [torch.full((n,), 0xa5, dtype=torch.uint8, device='cuda') for n in sizes]
        check(getattr(lib(), fn)(n_sdf, wptr, Ns, Kk, ops._ptr_array(bufs), s), fn)
        return [b.cpu().numpy() for b in bufs]

    for l in range(n_sdf, nl):                                              # the rendering net: no tracing pack, no chain packs, no bias copy
        assert offs[l]['wp16'] is None and offs[l]['wx3'] is None and offs[l]['wx3T'] is None and offs[l]['bias'] is None
    if td == 0:
        assert all(offs[l]['wp16'] is None for l in sdf)
    else:
        fn, size = {2: ('mvsdf_pack_bf16w_net', _f32_bytes), 3: ('mvsdf_pack_bf16s_net', _bf16_bytes),
                    5: ('mvsdf_pack_bf16x3_net', lambda a, b: 3 * _bf16_bytes(a, b))}[td]
        sizes = [size(*shapes[l]) for l in sdf]
        for l, ref_pack in zip(sdf, standalone(fn, sizes)):
            assert np.array_equal(_region(u8, offs[l]['wp16'], sizes[l], np.uint8), ref_pack), 'wp16 of layer %d' % l
    assert all(offs[l]['wx3'] is not None and offs[l]['wx3T'] is not None for l in sdf), 'the x3 chains are the product default: their packs belong to the block'
    assert all((offs[l]['wx3'] == offs[l]['wp16']) == (td == 5) for l in sdf)
    sizes = [3 * _bf16_bytes(*shapes[l]) for l in sdf]
    for l, ref_pack in zip(sdf, standalone('mvsdf_pack_bf16x3_net', sizes)):
        got = _region(u8, offs[l]['wx3'], sizes[l], np.uint8)
        assert np.array_equal(got, ref_pack), 'wx3 of layer %d' % l
        assert not got.view(np.uint16)[PR.unpack_bf16x3(got.view(np.uint16), *shapes[l])[1]].any()
    sizes = [3 * _bf16_bytes(shapes[l][1], shapes[l][0]) for l in sdf]
    for l, ref_pack in zip(sdf, standalone('mvsdf_pack_bf16x3t_net', sizes)):
        got = _region(u8, offs[l]['wx3T'], sizes[l], np.uint8)
        assert np.array_equal(got, ref_pack), 'wx3T of layer %d' % l
        assert not got.view(np.uint16)[PR.unpack_bf16x3(got.view(np.uint16), shapes[l][1], shapes[l][0])[1]].any()
    # this forward's own copy of the SDF net's biases (a forward that defers the rays without a hit keeps one)
    assert all(offs[l]['bias'] is not None for l in sdf)
    if os.environ.get('MVSDF_EAGER_UNHIT', '0') in ('', '0'):
        assert st.can_defer_unhit and not rec.eager_unhit, 'these networks defer the rays without a hit: the block holds a bias copy'
    if not rec.eager_unhit:
        for l in sdf:
            assert np.array_equal(_region(u8, offs[l]['bias'], 4 * shapes[l][0], np.uint32), PR.bits(bs[l].detach().cpu().numpy())), 'bias copy of layer %d' % l
    # the camera rays of the same launch
    uv, pose, intr = rec.inputs_keep[:3]
    dirs, cam = ops.camera_rays(uv, pose, intr)
    L = st.layout
    assert np.array_equal(_region(u8, L.ray_dirs, 12 * B * P, np.uint32), dirs.cpu().numpy().view(np.uint32).reshape(-1))
    assert np.array_equal(_region(u8, L.cam_loc, 12 * B, np.uint32), cam.cpu().numpy().view(np.uint32).reshape(-1))
    del out
