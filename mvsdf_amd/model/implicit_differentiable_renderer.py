"""IDRNetwork / ImplicitNetwork / RenderingNetwork with the reference's constructors, forward signatures, output dict
and state_dict layout (reference code/model/implicit_differentiable_renderer.py:19-338), executed by HIP kernels.

What differs from the reference internally (results are the same, see tests/):
  * weight_norm is folded once per forward by a HIP kernel (the reference refolds in each of ~57 network calls);
  * the whole RayTracing.forward is 7 kernel launches without a host synchronisation (csrc/trace.hip: k_sphere_trace, 3 x k_ray_samples,
    3 x k_reduce_items);
  * the five autograd MLP passes of idr.py:202,256,275,325,326 over overlapping point sets are ONE fused
    value + normal evaluation on rows ordered [hit rays | sample points | non-hit rays]; the re-evaluation at the
    differentiable surface points (idr.py:325-326) re-uses it, and both backward passes run the hand-written
    first/second-order backward on row prefixes.
"""
import importlib
import os
import weakref

import numpy as np
import torch
import torch.nn as nn

from .. import functional as Fn
from .. import native_step as NS
from ..utils.general import PinnedUniform
from .. import ops
from ..utils import rend_util
from . import conf as _default_conf
from .ray_tracing import NativeSDF, RayTracing
from .sample_network import SampleNetwork

conf = _default_conf
if os.environ.get('IDR_USE_ENV', '0') == '1' and os.environ.get('IDR_CONF', '') != '':
    print('override conf: ', os.environ.get('IDR_CONF'))
    conf = importlib.import_module(os.environ.get('IDR_CONF'))

# Arithmetic of the no-grad tracing MLP of every IDRNetwork / ImplicitNetwork.native_sdf() built afterwards (IDRNetwork.set_trace_dtype changes one model).
# 'f32x3' since round 5: bit-exact against its own CPU oracle at the full BASELINE batch sizes (tests/test_gpu_f32x3.py), hit masks identical to the fmaf-chain
# arithmetic 'f32' on every reference fixture, 1.3x faster.  (Tests switch it through tests/conftest.py, not through the environment.)
DEFAULT_TRACE_DTYPE = 'f32x3'


class _WNLinear(nn.Module):
    """Parameters of a weight-normed nn.Linear in torch.nn.utils.weight_norm's layout: bias, weight_g [out,1], weight_v [out,in]."""

    def __init__(self, weight, bias):
        super().__init__()
        self.bias = nn.Parameter(bias)
        self.weight_g = nn.Parameter(weight.norm(dim=1, keepdim=True))
        self.weight_v = nn.Parameter(weight)

    @property
    def weight(self):
        return self.weight_v * (self.weight_g / self.weight_v.norm(dim=1, keepdim=True))


class _PlainLinear(nn.Module):
    """weight_norm=False (idr.py:70-71,137-138 skipped): the parameters of a plain nn.Linear, same state_dict keys (weight, bias).  The fold
    kernels take a NULL g as "w = v"."""

    def __init__(self, weight, bias):
        super().__init__()
        self.weight = nn.Parameter(weight)
        self.bias = nn.Parameter(bias)

    weight_v = property(lambda self: self.weight)
    weight_g = None


def _linear_default_init(in_f, out_f):
    lin = nn.Linear(in_f, out_f)
    return lin.weight.detach().clone(), lin.bias.detach().clone()


class ImplicitNetwork(nn.Module):
    def __init__(self, feature_vector_size, d_in, d_out, dims, geometric_init=True, bias=1.0, skip_in=(), weight_norm=True, multires=0):
        super().__init__()
        if d_in != 3:
            raise NotImplementedError('the native SDF kernels trace 3-D points (d_in=3, mvsdf_dtu.conf:22)')
        dims = [d_in] + list(dims) + [d_out + 1 + feature_vector_size]
        self.multires = multires                                 # 0: the raw point is the input (no positional encoding), idr.py:36-40
        dims[0] = 3 + 6 * multires
        self.num_layers = len(dims)
        self.skip_in = tuple(skip_in)
        if len([s for s in self.skip_in if 0 < s < self.num_layers - 1]) > 1 and max(dims[1:-1]) > 512:
            raise NotImplementedError('several skip connections need the fused chain kernels (hidden width <= 512)')
        self.d_out = d_out
        for l in range(self.num_layers - 1):
            out_dim = dims[l + 1] - dims[0] if (l + 1) in self.skip_in else dims[l + 1]
            w, b = _linear_default_init(dims[l], out_dim)
            if geometric_init:                                   # idr.py:53-68
                if l == self.num_layers - 2:
                    nn.init.normal_(w, mean=np.sqrt(np.pi) / np.sqrt(dims[l]), std=0.0001)
                    nn.init.constant_(b, -bias)
                elif multires > 0 and l == 0:
                    nn.init.constant_(b, 0.0)
                    nn.init.constant_(w[:, 3:], 0.0)
                    nn.init.normal_(w[:, :3], 0.0, np.sqrt(2) / np.sqrt(out_dim))
                elif multires > 0 and l in self.skip_in:
                    nn.init.constant_(b, 0.0)
                    nn.init.normal_(w, 0.0, np.sqrt(2) / np.sqrt(out_dim))
                    nn.init.constant_(w[:, -(dims[0] - 3):], 0.0)
                else:
                    nn.init.constant_(b, 0.0)
                    nn.init.normal_(w, 0.0, np.sqrt(2) / np.sqrt(out_dim))
            setattr(self, 'lin' + str(l), _WNLinear(w, b) if weight_norm else _PlainLinear(w, b))

    def _lins(self):
        return [getattr(self, 'lin' + str(l)) for l in range(self.num_layers - 1)]

    def fold_spec(self):
        lins = self._lins()
        skips = tuple(sorted(s for s in set(self.skip_in) if 0 < s < self.num_layers - 1))      # idr.py:86: `if l in self.skip_in`
        return ([m.weight_v for m in lins], [m.weight_g for m in lins], [m.bias for m in lins], skips if len(skips) != 1 else skips[0],
                self.multires)

    def fold(self):
        """-> (PackedNet, folded weights linked to autograd, biases)."""
        return Fn.fold_network(*self.fold_spec())

    def native_sdf(self):
        net = self.fold()[0]
        td = getattr(self, 'trace_dtype', None) or DEFAULT_TRACE_DTYPE
        ops.pack_trace_net(net, td)
        return NativeSDF(net)

    def forward(self, input, compute_grad=False):
        net, ws, bs = self.fold()
        y, _, _ = Fn.sdf_value_normal(net, ws, bs, input, 0)
        return y

    def gradient(self, x):
        x.requires_grad_(True)                                  # side effect kept (idr.py:97)
        net, ws, bs = self.fold()
        _, n, _ = Fn.sdf_value_normal(net, ws, bs, x, x.shape[0])
        return n.unsqueeze(1)


class RenderingNetwork(nn.Module):
    def __init__(self, feature_vector_size, mode, d_in, d_out, dims, weight_norm=True, multires_view=0):
        super().__init__()
        if mode not in ('idr', 'no_view_dir', 'no_normal'):
            raise ValueError("mode must be 'idr', 'no_view_dir' or 'no_normal' (idr.py:149-154)")
        if multires_view < 0 or multires_view > 16:
            raise ValueError('multires_view out of range')
        self.mode = mode
        self.multires_view = multires_view
        # input layout handed to the kernels: PE frequencies | 0x100 (no view direction) | 0x200 (no normal)
        self.view_spec = multires_view | (0x100 if mode == 'no_view_dir' else 0) | (0x200 if mode == 'no_normal' else 0)
        dims = [d_in + feature_vector_size] + list(dims) + [d_out]
        if multires_view > 0:
            dims[0] += 6 * multires_view
        expect = 3 + (0 if mode == 'no_view_dir' else 3 + 6 * multires_view) + (0 if mode == 'no_normal' else 3) + feature_vector_size
        if dims[0] != expect:                                     # the reference would fail inside lin0 with a shape error
            raise ValueError('d_in=%d does not match the inputs of mode %r (first layer takes %d columns, the inputs have %d)' % (d_in, mode, dims[0], expect))
        self.num_layers = len(dims)
        for l in range(self.num_layers - 1):
            w, b = _linear_default_init(dims[l], dims[l + 1])
            setattr(self, 'lin' + str(l), _WNLinear(w, b) if weight_norm else _PlainLinear(w, b))

    def fold_spec(self):
        lins = [getattr(self, 'lin' + str(l)) for l in range(self.num_layers - 1)]
        return ([m.weight_v for m in lins], [m.weight_g for m in lins], [m.bias for m in lins], -1, 0)

    def fold(self):
        return Fn.fold_network(*self.fold_spec())

    def forward(self, points, normals, view_dirs, feature_vectors, folded=None):
        net, ws, bs = folded if folded is not None else self.fold()
        return Fn.render(net, ws, bs, points, normals, view_dirs, feature_vectors, self.view_spec)


class LazyOutputs(dict):
    """The output dict of a training forward with `IDRNetwork.lazy_unused_outputs`: `points` and `sdf_output` of the rays WITHOUT a hit come
    from minimal_sdf_points (ray_tracing.py:280-308) -- 100 SDF evaluations per such ray, ~44 % of the tracer's rows at the bench shape --
    and nothing in the training loop reads them (the loss reads neither key, loss.py:176-219; `use_mask` is off in this fork).  They are
    computed the first time one of the two keys is read, by the same kernels on the same inputs: every value a caller can observe equals the
    eager one.  Any access path (`[]`, get, items, values, iteration, dict(...), copy) goes through `_materialize` first when it may touch them."""
    _LAZY = ('points', 'sdf_output')
    # A second group with its own resolver, for the native step (`late`: mvsdf_step_resolve_unhit through StepRecord.resolve_unhit -- the same deferral without the
    # Python-orchestrated route and without an expiry: the forward block holds everything the late evaluation reads).  Every access path below serves both groups.
    _LATE = ('points', 'sdf_output')

    def __init__(self, data, materialize, late=None):
        super().__init__(data)
        self._pending = materialize
        self._late = late

    def _materialize(self):
        if self._pending is not None:
            self._pending()                  # (an expired one raises and stays in place)
            self._pending = None

    def _need(self, k=None):
        """Before key k (None: any key) is observed or moved."""
        if self._late is not None and (k is None or k in self._LATE):
            late, self._late = self._late, None
            late()
        if k is None or k in self._LAZY:
            self._materialize()

    def _expire(self):
        """The next forward re-folds the weights into the same packed buffers: the deferred rows can no longer be evaluated at this step's
        weights.  Reading them after that is an error, not a silently different value."""
        if self._pending is not None:
            def stale(*_):
                raise RuntimeError("lazy_unused_outputs: 'points' / 'sdf_output' of a previous step were first read after the next forward "
                                   "started; read them before it, or set model.lazy_unused_outputs = False")
            self._pending = stale

    def __getitem__(self, k):
        self._need(k)
        return super().__getitem__(k)

    def get(self, k, default=None):
        self._need(k)
        return super().get(k, default)

    def __iter__(self):                      # also makes dict(self) / {**self} take the generic (keys + __getitem__) route
        return super().__iter__()

    def items(self):
        self._need()
        return super().items()

    def values(self):
        self._need()
        return super().values()

    def copy(self):
        self._need()
        return dict(super().items())

    def pop(self, k, *a):
        self._need(k)
        return super().pop(k, *a)

    # every remaining way to observe or move the values goes through the eager ones
    def setdefault(self, k, default=None):
        self._need(k)
        return super().setdefault(k, default)

    def popitem(self):
        self._need()
        return super().popitem()

    def update(self, *a, **k):
        self._need()                         # an update may replace a lazy key: the pending evaluation must not overwrite it afterwards
        return super().update(*a, **k)

    def __eq__(self, other):
        self._need()
        return super().__eq__(other)

    __hash__ = None

    def __ne__(self, other):
        return not self.__eq__(other)

    def __or__(self, other):
        self._need()
        return dict(super().items()) | other

    def __ror__(self, other):
        self._need()
        return other | dict(super().items())

    def __ior__(self, other):
        self._need()
        return super().__ior__(other)

    def __copy__(self):
        return self.copy()

    def __deepcopy__(self, memo):
        import copy as _copy
        return _copy.deepcopy(self.copy(), memo)

    def __reduce__(self):                    # pickle / copy.copy: a plain dict of the eager values
        return (dict, (self.copy(),))


class PendingOutputs(LazyOutputs):
    """The output dict of a DEFERRED training forward (IDRNetwork.deferred_step): the forward is enqueued, the host has not waited for the hit counts.  The
    keys whose shapes follow the counts -- and `rgb_values`, which carries the autograd link -- become tensors the first time any of them is read (one wait
    for the counts, the classic autograd node over the same forward block); `IDRLoss.forward` does not read them: it recognises the pending step (`_mv_rec`)
    and runs loss and backward with the counts taken on the device (native_step._DeferredStepLossFn).  Same values either way."""
    _LAZY = ('diff_surf_pts', 'rgb_values', 'grad_theta', 'eikonal_points_hom', 'eikonal_output', 'surf_indicator_output')

    def __init__(self, data, fill, rec, late=None):
        super().__init__(data, fill, late)                       # fill(target): NO reference back to this object inside it -- a closure over the dict it fills
        self._mv_rec = rec                                       # would make dict, record and forward block (3.6 GB in the shipped workload) wait for the cyclic collector

    def _materialize(self):
        if self._pending is not None:
            self._pending(self)
            self._pending = None

    def pending_rec(self):
        """The step record while no N-shaped output has been read, else None."""
        return self._mv_rec if self._pending is not None else None

    def raw(self, k):
        """The entry as it stands, without resolving the N-shaped keys (`points` / `sdf_output` are still made final first)."""
        if self._late is not None and k in self._LATE:
            self._need(k)
        return dict.__getitem__(self, k)


class StepOutputs(LazyOutputs):
    """The output dict of a CLASSIC native training forward whose rays without a hit wait for their first reader (`late`); every other key is final."""
    _LAZY = ()

    def __init__(self, data, late):
        super().__init__(data, None, late)


class _StepStats(dict):
    """IDRNetwork.last_stats of a deferred step: 'N' is looked up (one wait for the counts) when somebody reads it."""

    def __init__(self, rec, **kw):
        super().__init__(**kw)
        self._rec = rec

    def __getitem__(self, k):
        if k == 'N' and not dict.__contains__(self, 'N'):
            dict.__setitem__(self, 'N', self._rec.resolve()[0])
        return dict.__getitem__(self, k)

    def get(self, k, default=None):
        return self[k] if (k == 'N' or k in self) else default


class IDRNetwork(nn.Module):
    HOST_STAGE = True                                            # default of self.host_stage (see __init__)
    DEFERRED_STEP = os.environ.get('MVSDF_DEFERRED_STEP', '1') != '0'   # default of self.deferred_step

    def __init__(self, conf):
        super().__init__()
        self.feature_vector_size = conf.get_int('feature_vector_size')
        self.implicit_network = ImplicitNetwork(self.feature_vector_size, **conf.get_config('implicit_network'))
        self.rendering_network = RenderingNetwork(self.feature_vector_size, **conf.get_config('rendering_network'))
        self.ray_tracer = RayTracing(**conf.get_config('ray_tracer'))
        self.sample_network = SampleNetwork()
        self.object_bounding_sphere = conf.get_float('ray_tracer.object_bounding_sphere')
        self.last_stats = {}
        self.set_trace_dtype(DEFAULT_TRACE_DTYPE)                # arithmetic of the no-grad tracing MLP (see set_trace_dtype)
        self._counts_host = None                                 # pinned [N hit, N hit & true mask], filled while the tracer still runs
        self._counts_event = None
        self._draw = PinnedUniform()
        self._fold_cache = {}                                    # ops.FoldPlan of the training step's flat fold
        self._lazy_prev = None
        self.lazy_unused_outputs = False                         # training: evaluate the min-sdf points of non-hit rays only if `points` / `sdf_output` are read (LazyOutputs)
        # training forward / backward through the native step driver (csrc/step_driver.hip: one C call each instead of ~45 ctypes calls and
        # autograd glue).  False: the Python-orchestrated route over the same kernels (kept for A/B tests and the launch-path experiments).
        self.native_step = os.environ.get('MVSDF_NATIVE_STEP', '1') != '0'
        self.host_stage = type(self).HOST_STAGE                  # the step's CPU-generator draws are read from pinned memory by its first kernel (False: an async copy)
        # training forward without the host wait for the hit counts (PendingOutputs; IDRLoss + backward then read them on the device): the step's rate no longer
        # depends on host latency.  False: the classic step (one wait per forward).  Phase 0 (depth-surface samples, idr.py:226-247) always waits.
        self.deferred_step = type(self).DEFERRED_STEP
        # The native step leaves minimal_sdf_points (~44 % of the tracer's rows at the bench shape), the evaluation rows and sdf_output of the rays WITHOUT a hit to the
        # first reader of `points` / `sdf_output` (mvsdf_step_resolve_unhit: nothing in a training step reads them; no expiry, same values).  True, or MVSDF_EAGER_UNHIT=1:
        # everything inside the forward, the launch sequence up to round 6.
        self.eager_unhit_rows = os.environ.get('MVSDF_EAGER_UNHIT', '0') not in ('', '0')
        # The deferring forward cuts the sphere launch after st_iters + 1 rounds: the few rays that need more finish on a second stream beside the sampler windows of
        # the others (mvsdf_trace_cut_stage; same values).  True: where the tracer's route says it pays; False, or MVSDF_SPHERE_CUT=0: the launch sequence without it;
        # 2: always.  sphere_cut_rounds > 0: another round limit (development: a small one makes small batches spill).
        self.sphere_cut = {'0': False, '': False, '2': 2}.get(os.environ.get('MVSDF_SPHERE_CUT', '1'), True)
        self.sphere_cut_rounds = 0
        # The fork of a forward with the cut (mvsdf_step_set_fork; same values): (late branch on the launch stream, ray partition beside the secant chains, sixteen-wave
        # rows form, its grid cap), each -1: by its rule, 0: the launch sequence without it, 1: on wherever the cut is on.  MVSDF_FORK=0: all three off;
        # MVSDF_FORK=a,b,c: the three parts as given (A/B runs of one part: profiles/fork_ab.txt).
        e = os.environ.get('MVSDF_FORK', '1')
        self.fork = (tuple(int(v) for v in e.split(',')) + (0,))[:4] if e.count(',') == 2 else ((0, 0, 0, 0) if e in ('', '0') else (-1, -1, -1, 0))
        self._steps = {}                                         # NativeStep per batch shape / phase configuration
        self._ones = None                                        # all-ones object mask handed to the tracer when conf.use_mask is off

    def set_trace_dtype(self, dtype):
        """'f32x3' (the default, DEFAULT_TRACE_DTYPE): the reference's fp32 arithmetic (idr.py:77-94 inside ray_tracing.py:27-98, fp32 weights unrounded) from
        six exact bf16 products per element pair on v_mfma_f32_16x16x32_bf16, bit-exact against its CPU oracle (a model of that instruction).
        'f32': the same arithmetic as a k-ascending fmaf chain on v_mfma_f32_16x16x4_f32, bit-exact against the fmaf-chain oracle (the default of rounds
        1-4; 1.3x slower, slightly further from an fp64 evaluation).  BASELINE configs[4] ("bf16 MLP weights"; outside the 1e-4 parity claim against the fp32
        reference, see DESIGN.md for the accuracy budget; the differentiable passes keep fp32):
        'bf16w': only the tracing MLP's WEIGHTS are rounded to bf16 (BASELINE configs[4] says "bf16 MLP weights"), activations and arithmetic
        stay fp32 on the fp32 MFMA: bit-exact against the oracle on the rounded weights; the control that prices the activation rounding.
        'bf16x2' / 'bf16x3': bf16 weights on the bf16 MFMA, every activation carried as 2 / 3 bf16 terms (16 / all 24 mantissa bits,
        csrc/tile_engine_bf16s.h): the arithmetic of 'bf16w' up to the order of the fp32 additions inside the matrix core -- the configs[4] mode
        that is fast AND parity-checked (hit masks equal to the oracle's on the rounded weights except at recorded ties, depths 1e-4).
        'f32x3': the fp32 weights unrounded, as three bf16 terms like the activations: the reference's fp32 arithmetic from six exact bf16 products per
        element pair on the bf16 MFMA -- fp32-accurate (measured closer to an fp64 evaluation than the 'f32' fmaf chain), bit-exact against its own
        CPU oracle (a model of the matrix instruction) and parity-checked against the fmaf-chain oracle and the reference fixtures; not bit-identical to 'f32'.
        ('bf16' -- bf16 weights AND 8-bit activations, rounds 2-4 -- was removed in round 5: 'bf16x2' runs at its speed with the oracle's masks.)"""
        if dtype not in ops.TRACE_DTYPES:
            raise ValueError('IDRNetwork.set_trace_dtype(%r): expected one of %s' % (dtype, ', '.join(sorted(ops.TRACE_DTYPES))))
        self.trace_dtype = dtype
        self.implicit_network.trace_dtype = dtype
        return self

    # ------------------------------------------------------------------------------------------------------------
    def _dsurf_samples(self, input, n_dsurf_points, bb):
        """Phase-0 depth-surface sampling (idr.py:226-247): two random n-subsets of the depth pixels whose unprojected (resp. jittered)
        point lies in the eikonal box, sorted by pixel.  -> (on-surface [n,3], jittered [n,3], counts [2] on the device).
        One selection launch + a sort + one unprojection launch (csrc/sample_kernels.hip) instead of unprojecting every pixel and a
        host-side np.random.choice; the seed comes from torch's CPU generator (torch.manual_seed reproduces a run)."""
        depths, depth_cams = input['depths'], input['depth_cams']
        depths_pack = depths.reshape(-1, depths.shape[-2], depths.shape[-1])
        cams_pack = depth_cams.reshape(-1, 2, 4, 4)
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        jitter_rad = 0.1                                         # hard-coded in the reference (idr.py:228)
        on, jit, counts, _ = ops.dsurf_samples(depths_pack, cams_pack, input['size'][:1], input['center'][:1], bb, jitter_rad, seed, n_dsurf_points)
        return on, jit, counts

    def forward(self, input, train_progress=None):
        intrinsics, uv, pose = input['intrinsics'], input['uv'], input['pose']
        object_mask_true = input['object_mask'].reshape(-1)
        prev = self._lazy_prev() if self._lazy_prev is not None else None
        if prev is not None:
            prev._expire()
        self._lazy_prev = None
        if self.training:
            self._check_point_groups(train_progress)
        if self.training and self.native_step and not self.lazy_unused_outputs and self.ray_tracer.events is None and not ops._MINSDF_SIDE_STREAM:
            out = self._forward_native(input, train_progress, object_mask_true)
            if out is not None:
                return out
        object_mask = object_mask_true if conf.use_mask else torch.ones_like(object_mask_true)

        ray_dirs, cam_loc = rend_util.get_camera_params(uv, pose, intrinsics)
        batch_size, num_pixels, _ = ray_dirs.shape
        R = batch_size * num_pixels
        dev = ray_dirs.device

        # one weight-norm fold per step, both networks in one launch pair (and one backward launch).  Training: the folded parameters are ONE
        # flat tensor (one autograd edge, pointer arithmetic instead of per-layer tensors); eval keeps the per-layer form the stand-alone
        # Functions take.
        flat = None
        if self.training:
            flat, plan, (net, rnet) = Fn.fold_networks_flat([self.implicit_network.fold_spec(), self.rendering_network.fold_spec()], self._fold_cache)
            ws = bs = rws = rbs = None
        else:
            (net, ws, bs), (rnet, rws, rbs) = Fn.fold_networks([self.implicit_network.fold_spec(), self.rendering_network.fold_spec()])
        ops.pack_trace_net(net, self.trace_dtype)                                  # one more launch per step: bf16 / rounded packs for the tracer
        n_dsurf_points, dsurf = 0, None
        if self.training:
            assert train_progress is not None
            if any([conf.d_use_dsurf_on(train_progress), conf.d_use_dsurf_jitter(train_progress),
                    conf.eik_use_dsurf_on(train_progress), conf.eik_use_dsurf_jitter(train_progress)]):
                n_dsurf_points = R // 2                          # independent of the tracer: enqueued ahead of it
                dsurf = self._dsurf_samples(input, n_dsurf_points, self.object_bounding_sphere)
        # The hit mask is final once the ray sampler has run; the secant / min-sdf launch that follows only moves points.  In training
        # the hit counts are copied to pinned host memory between the two, so the host learns them while that launch (and the fused
        # evaluation enqueued behind it) still runs.
        sync = {}

        def on_mask(net_mask):
            # stable row partition (hit rays first) + both counts in one launch; the counts travel to pinned memory right away
            sync['part'] = ops.partition_rays(net_mask, object_mask if conf.use_mask else None, object_mask_true, ray_dirs)
            if self._counts_host is None:
                self._counts_host = torch.empty(4, dtype=torch.int64).pin_memory()
                self._counts_event = torch.cuda.Event()
            if dsurf is None:
                self._counts_host[:2].copy_(sync['part'][3], non_blocking=True)
            else:                                                # + how many depth-surface samples each set found
                self._counts_host.copy_(torch.cat([sync['part'][3], dsurf[2]]), non_blocking=True)
            self._counts_event.record()

        deferred = [] if (self.training and self.lazy_unused_outputs) else None
        with torch.no_grad():
            points, network_object_mask, dists = self.ray_tracer(sdf=NativeSDF(net), cam_loc=cam_loc, object_mask=object_mask,
                                                                 ray_directions=ray_dirs, mask_ready=on_mask if self.training else None,
                                                                 defer_minsdf=deferred)
        ray_dirs = ray_dirs.reshape(-1, 3)

        if self.training:
            perm, inv, true_rows, _, view_sorted = sync['part']
        else:
            # rows: [surface rays | the other rays]  (stable order inside each group = the reference's boolean-mask order)
            surface_mask = network_object_mask
            perm = torch.sort((~surface_mask).to(torch.int8), stable=True).indices
            n_hit_dev = surface_mask.sum()
            inv = torch.empty_like(perm)
            inv[perm] = torch.arange(R, device=dev)
        pts_sorted = points[perm]                                # hit rays first, then the others

        if self.training:
            bb = self.object_bounding_sphere
            n_eik_points = R // 2
            eikonal_points = self._draw((n_eik_points, 3), -bb, bb, dev)            # idr.py:216-221 (CPU generator, async copy)
            if dsurf is not None:
                dsurf_on_sample, dsurf_jitter_sample = dsurf[0], dsurf[1]
            else:
                dsurf_on_sample = torch.zeros(0, 3, device=dev)
                dsurf_jitter_sample = torch.zeros(0, 3, device=dev)
            E = n_eik_points + 2 * n_dsurf_points
            # One fused value + normal evaluation, launched BEFORE the host learns the hit count N (its shapes do not depend on N):
            # rows [sample points | all rays, hit ones first]; normals on every row (those of non-hit rays are never read).
            # Rows that receive gradients form the prefix [0, E + N): the backward skips the non-hit rays.
            x_eval = torch.cat([eikonal_points, dsurf_on_sample, dsurf_jitter_sample, pts_sorted], 0)
            y_eval, n_eval, saved = ops.sdf_forward(net, x_eval, R + E)
            st = Fn.StepState()
            st.net, st.x_eval, st.y_eval, st.n_eval, st.saved = net, x_eval, y_eval, n_eval, saved
            st.R, st.E, st.n_eik, st.n_ds = R, E, n_eik_points, n_dsurf_points
            st.perm, st.inv, st.true_rows, st.view_sorted, st.counts_dev = perm, inv, true_rows, view_sorted, sync['part'][3]
            # point groups in the reference's row order [hit | eikonal | on-surface | jittered] (idr.py:253-257): bit g of a mask selects
            # group g for the depth term / the eikonal term (idr.py:258-286)
            d_flags = (conf.d_use_rt_surf, conf.d_use_eik, conf.d_use_dsurf_on, conf.d_use_dsurf_jitter)
            e_flags = (conf.eik_use_rt_surf, conf.eik_use_eik, conf.eik_use_dsurf_on, conf.eik_use_dsurf_jitter)
            has = (True, n_eik_points > 0, n_dsurf_points > 0, n_dsurf_points > 0)
            st.d_mask = sum(1 << g for g in range(4) if has[g] and d_flags[g](train_progress))
            st.e_mask = sum(1 << g for g in range(4) if has[g] and e_flags[g](train_progress))
            st.detach_geo = bool(train_progress < conf.phase[0] or conf.disable_rgb_grad)                     # idr.py:331-334
            st.rnet, st.multires_view = rnet, self.rendering_network.view_spec

            def wait_counts():
                self._counts_event.synchronize()                 # output shapes depend on the counts
                if dsurf is not None and min(int(self._counts_host[2]), int(self._counts_host[3])) < n_dsurf_points:
                    raise ValueError("Cannot take a larger sample than population when 'replace=False'")   # np.random.choice, idr.py:244
                return int(self._counts_host[0]), int(self._counts_host[1])
            st.wait_counts = wait_counts
            st.plan = plan
            differentiable_surface_points, rgb_values, grad_theta, eikonal_output, surf_indicator_output = Fn.idr_step_flat(st, flat)
            N = st.N
            hit_idx = perm[:N]
            sdf_output, eikonal_points_hom = st.sdf_output, st.points_hom           # no gradient: the loss never differentiates them
            x_all, shared, row0 = x_eval, None, E
        else:
            y_all, n_all, shared = Fn.sdf_value_normal(net, ws, bs, pts_sorted, R)
            N = int(n_hit_dev.item())
            hit_idx, rest_idx = perm[:N], perm[N:]
            x_all = pts_sorted
            row0 = 0
            sdf_output = y_all[:, :1][inv]
            differentiable_surface_points = x_all[:N]
            grad_theta = None

        if not self.training:
            view = -ray_dirs[hit_idx]
            rgb_values = torch.ones_like(points)
            if N > 0:
                rgb = self._rgb_from_shared(shared, ws, bs, differentiable_surface_points, view, N, train_progress, row0,
                                            folded=(rnet, rws, rbs))
                rgb_values = rgb_values.index_put((hit_idx,), rgb)                                           # idr.py:302-304

        out = {
            'points': points,
            'diff_surf_pts': differentiable_surface_points,
            'rgb_values': rgb_values,
            'sdf_output': sdf_output,
            'network_object_mask': network_object_mask,
            'object_mask': object_mask,
            'object_mask_true': object_mask_true,
            'grad_theta': grad_theta,
        }
        if self.training:
            out['eikonal_points_hom'] = eikonal_points_hom
            out['eikonal_output'] = eikonal_output
            out['surf_indicator_output'] = surf_indicator_output
        self.last_stats = {'R': R, 'N': N, 'E': (x_all.shape[0] - R), 'counters': self.ray_tracer.last_counters}
        if deferred:
            finish = deferred[0]

            def materialize(points=points, sdf_output=sdf_output, mask=network_object_mask, net=net):
                with torch.no_grad():
                    finish()                                     # min-sdf rows: rewrites points / dists of the listed rays in place
                    rows = torch.nonzero(~mask).flatten()        # their sdf_output = implicit_network(points)[:, :1] through the same forward kernel
                    if rows.numel():
                        y, _, _ = ops.sdf_forward(net, points[rows].contiguous(), 0)
                        sdf_output[rows] = y[:, :1]
            out = LazyOutputs(out, materialize)
            self._lazy_prev = weakref.ref(out)
        return out


    # ------------------------------------------------------------------------------------------------------------
    def _native_step_for(self, B, P, n_ds, dev):
        """The NativeStep of this batch shape (created on first use: host-side state only)."""
        inet, rnet, rt = self.implicit_network, self.rendering_network, self.ray_tracer
        R = B * P
        mt, mt_samples = rt.tiling(R, ops.TRACE_DTYPES[self.trace_dtype])
        tpv = rt._params()
        key = (B, P, n_ds, str(dev), self.trace_dtype, mt, mt_samples, tpv, bool(conf.use_mask))
        st = self._steps.get(key)
        if st is None:
            vs, gs, bs, skips, multires = inet.fold_spec()
            rvs, rgs, rbs, _, _ = rnet.fold_spec()
            if len(vs) + len(rvs) > NS.STEP_MAX_LAYERS or max(v.shape[0] for v in vs[:-1]) > 512:
                self._steps[key] = False                          # outside what the driver covers: the Python-orchestrated route
                return None
            d = NS.StepDesc()
            d.B, d.P, d.n_eik, d.n_ds = B, P, R // 2, n_ds
            d.n_sdf, d.n_render = len(vs), len(rvs)
            for l, v in enumerate(list(vs) + list(rvs)):
                d.N[l], d.K[l] = v.shape
            skips = skips if isinstance(skips, (tuple, list)) else ((skips,) if skips >= 0 else ())
            d.skip_mask = sum(1 << int(sk) for sk in skips)
            d.multires, d.view_spec = multires, rnet.view_spec
            d.trace_dtype = ops.TRACE_DTYPES[self.trace_dtype]
            d.use_object_mask = 1 if conf.use_mask else 0
            d.tp = NS.TraceParams(*tpv)
            d.mt, d.mt_samples = mt, mt_samples
            st = self._steps[key] = NS.NativeStep(d, dev)
        return st or None

    def _forward_native(self, input, train_progress, object_mask_true):
        """Training forward through the native step driver: ONE C call enqueues fold -> rays -> tracer -> partition -> fused value + normal
        evaluation -> rendering net -> output gather; the host then waits for the hit counts (copied out right after the partition, i.e. while
        the last tracer launch and the evaluation still run) and wraps regions of the forward block as the output tensors.
        Returns None when the configuration is outside what the driver covers."""
        assert train_progress is not None
        uv, pose, intrinsics = input['uv'], input['pose'], input['intrinsics']
        dev = uv.device
        if not (uv.is_cuda and uv.dtype == torch.float32 and pose.dtype == torch.float32 and intrinsics.dtype == torch.float32 and pose.shape[1:] == (4, 4)):
            return None
        B, P = uv.shape[0], uv.shape[1]
        R = B * P
        use_ds = any([conf.d_use_dsurf_on(train_progress), conf.d_use_dsurf_jitter(train_progress),
                      conf.eik_use_dsurf_on(train_progress), conf.eik_use_dsurf_jitter(train_progress)])
        n_ds = R // 2 if use_ds else 0
        st = self._native_step_for(B, P, n_ds, dev)
        if st is None:
            return None
        rt = self.ray_tracer
        vs, gs, bs, params, live = self._step_params()
        # random draws in the order of the Python route: depth-surface seed, min-sdf steps, eikonal points (all from torch's CPU generator)
        dsurf = self._dsurf_samples(input, n_ds, self.object_bounding_sphere) if use_ds else None
        bb = self.object_bounding_sphere
        n_eik = R // 2
        stage_slot = None
        if isinstance(self._draw, PinnedUniform) and isinstance(rt._draw, PinnedUniform):
            # one pinned staging buffer, NO copy: the step's first kernel reads it (MvsdfStepInputs.host_stage)
            # (self.host_stage = False: one async copy in front of the step instead -- the A/B partner, tests/test_gpu_alt_paths.py)
            if self.host_stage:
                minsdf_steps, eik, stage, stage_slot = self._draw.pair_staged((rt.n_steps,), 0.0, 1.0, (n_eik, 3), -bb, bb, dev)
            else:
                (minsdf_steps, eik), stage = self._draw.pair((rt.n_steps,), 0.0, 1.0, (n_eik, 3), -bb, bb, dev), None
        else:                                                    # (someone replaced a draw hook: the two separate draws of the Python route)
            minsdf_steps = rt._draw((rt.n_steps,), 0.0, 1.0, dev)
            eik = self._draw((n_eik, 3), -bb, bb, dev)
            minsdf_steps, eik = minsdf_steps.float().contiguous(), eik.float().contiguous()
            stage = None
        true_u8 = object_mask_true if object_mask_true.dtype == torch.uint8 else (
            object_mask_true.view(torch.uint8) if object_mask_true.dtype == torch.bool else object_mask_true.to(torch.uint8))
        if not true_u8.is_contiguous():
            true_u8 = true_u8.contiguous()
        if conf.use_mask:
            om_u8 = true_u8
        else:
            if self._ones is None or self._ones.numel() != R or self._ones.device != dev:
                self._ones = torch.ones(R, dtype=torch.uint8, device=dev)
            om_u8 = self._ones
        iv = rt.intervals(dev)
        i = st.inputs
        uv_c, pose_c, intr_c = (uv if uv.is_contiguous() else uv.contiguous()), (pose if pose.is_contiguous() else pose.contiguous()), (
            intrinsics if intrinsics.is_contiguous() else intrinsics.contiguous())
        keep = (uv_c, pose_c, intr_c, true_u8, om_u8, iv, minsdf_steps, eik, dsurf)
        i.uv, i.pose, i.intrinsics = uv_c.data_ptr(), pose_c.data_ptr(), intr_c.data_ptr()
        i.object_mask, i.object_mask_true = om_u8.data_ptr(), true_u8.data_ptr()
        i.intervals, i.minsdf_steps, i.eik_points = iv.data_ptr(), minsdf_steps.data_ptr(), eik.data_ptr()
        i.host_stage = stage.data_ptr() if stage is not None else None
        if dsurf is not None:
            i.ds_on, i.ds_jit, i.ds_counts = dsurf[0].data_ptr(), dsurf[1].data_ptr(), dsurf[2].data_ptr()
        else:
            i.ds_on = i.ds_jit = i.ds_counts = None
        rec = NS.StepRecord()
        rec.step, rec.vs, rec.gs, rec.bs, rec.params, rec.live = st, vs, gs, bs, params, live
        rec.prm = st.params(vs, gs, bs)
        rec.d_mask, rec.e_mask = self._group_masks(train_progress, n_eik, n_ds)
        rec.use_geo = not bool(train_progress < conf.phase[0] or conf.disable_rgb_grad)                       # idr.py:331-334
        rec.inputs_keep = keep                                   # the inputs stay alive as long as the step's record does
        rec.eager_unhit = bool(self.eager_unhit_rows) or not st.can_defer_unhit
        st.set_sphere_cut(self.sphere_cut, self.sphere_cut_rounds)
        st.set_fork(*self.fork)
        NS.enqueue_forward(rec)                                 # everything of this forward is on the stream now; nothing waited for
        if stage_slot is not None:                               # the pinned draws may be rewritten once this forward's first kernel has read them
            stage_slot[2] = (st, rec.seq)
        L, f = st.layout, rec.fwd
        counters = f.b(L.counters, (128,)).view(torch.int64)
        rt.last_counters = counters
        d_ = self.__dict__                                        # (plain attributes: nn.Module.__setattr__ costs 4 us each, three of them per step)
        d_['_last_step'] = st
        d_['_last_rec'] = weakref.ref(rec)                        # (inspection: tests read what the forward saved through NativeStep.saved_offsets)
        eager = {
            'points': f.f(L.points, (R, 3)),
            'diff_surf_pts': None,
            'rgb_values': None,
            'sdf_output': f.f(L.sdf_output, (R, 1)),
            'network_object_mask': f.b(L.mask, (R,)).view(torch.bool),
            'object_mask': object_mask_true if conf.use_mask else f.b(L.object_mask_out, (R,)).view(torch.bool),
            'object_mask_true': object_mask_true,
            'grad_theta': None,
            'eikonal_points_hom': None,
            'eikonal_output': None,
            'surf_indicator_output': None,
        }

        def materialize(target):
            diff_pts, rgb_values, grad_theta, eik_out, surf = NS.run_step(rec)      # waits for the counts; the autograd node over this forward block
            if dsurf is not None and min(int(rec.counts[2]), int(rec.counts[3])) < n_ds:
                raise ValueError("Cannot take a larger sample than population when 'replace=False'")          # np.random.choice, idr.py:244
            nd, _ = rec.keep
            dict.update(target, {'diff_surf_pts': diff_pts, 'rgb_values': rgb_values, 'grad_theta': grad_theta,
                                 'eikonal_points_hom': f.f(L.points_hom, (1, nd, 4, 1)), 'eikonal_output': eik_out, 'surf_indicator_output': surf})

        late = rec.resolve_unhit if rec.unhit_pending else None   # (a bound method of the record: no reference back to the dict)
        if self.deferred_step and st.can_defer and dsurf is None and torch.is_grad_enabled():
            out = PendingOutputs(eager, materialize, rec, late)
            d_['last_stats'] = _StepStats(rec, R=R, E=st.E, counters=counters)
            return out
        materialize(eager)                                       # the classic step: its one host wait
        d_['last_stats'] = {'R': R, 'N': rec.N, 'E': st.E, 'counters': counters}
        return StepOutputs(eager, late) if late is not None else eager

    def _step_params(self):
        """(weight_v list, weight_g list, bias list, all of them as one tuple) of both networks, SDF layers first.  The Parameter OBJECTS of a
        module are stable (load_state_dict, .to() and optimizers change their .data), so the lists are built once per set of objects."""
        c = getattr(self, '_param_cache', None)
        inet, rnet = self.implicit_network, self.rendering_network
        if c is not None:
            lins, objs = c[0], c[1]
            if all(m._parameters.get(n) is o for (m, n), o in zip(lins, objs)):      # nobody re-assigned a Parameter
                return c[2]
        vs, gs, bs, _, _ = inet.fold_spec()
        rvs, rgs, rbs, _, _ = rnet.fold_spec()
        vs, gs, bs = list(vs) + list(rvs), list(gs) + list(rgs), list(bs) + list(rbs)
        lins, objs = [], []
        mods = inet._lins() + [getattr(rnet, 'lin' + str(l)) for l in range(rnet.num_layers - 1)]
        for m in mods:
            for n, o in m._parameters.items():
                lins.append((m, n)); objs.append(o)
        params = tuple(vs) + tuple(gs) + tuple(bs)
        res = (vs, gs, bs, params, [p for p in params if p is not None])
        self._param_cache = (lins, objs, res)
        return res

    @staticmethod
    def _check_point_groups(train_progress):
        """The reference concatenates the selected point groups of each term with torch.cat and raises on an empty list (idr.py:258-286): so does
        this, before anything is launched, instead of handing a zero-row term to the loss kernels."""
        for term, flags in (('depth', ('d_use_rt_surf', 'd_use_eik', 'd_use_dsurf_on', 'd_use_dsurf_jitter')),
                            ('eikonal', ('eik_use_rt_surf', 'eik_use_eik', 'eik_use_dsurf_on', 'eik_use_dsurf_jitter'))):
            if not any(getattr(conf, f)(train_progress) for f in flags):
                raise ValueError('IDRNetwork.forward: every point group of the %s term is switched off at train_progress %g (conf.%s): '
                                 'the reference fails here (torch.cat of an empty list, idr.py:258-286)' % (term, train_progress, ' / '.join(flags)))

    def _group_masks(self, train_progress, n_eik, n_ds):
        """Point groups in the reference's row order [hit | eikonal | on-surface | jittered] (idr.py:253-257): bit g selects group g for the
        depth term / the eikonal term (idr.py:258-286)."""
        d_flags = (conf.d_use_rt_surf, conf.d_use_eik, conf.d_use_dsurf_on, conf.d_use_dsurf_jitter)
        e_flags = (conf.eik_use_rt_surf, conf.eik_use_eik, conf.eik_use_dsurf_on, conf.eik_use_dsurf_jitter)
        has = (True, n_eik > 0, n_ds > 0, n_ds > 0)
        return (sum(1 << g for g in range(4) if has[g] and d_flags[g](train_progress)),
                sum(1 << g for g in range(4) if has[g] and e_flags[g](train_progress)))

    def _rgb_from_shared(self, shared, ws, bs, points, view_dirs, N, train_progress, row0=0, folded=None):
        defer = self.training and points.requires_grad and points.grad_fn is not None
        y2, normals = Fn.sdf_reuse(shared, ws, bs, points, N, defer_dw=defer, row0=row0)                               # idr.py:325-327
        feature_vectors = y2[:, 2:]
        if (train_progress is not None and train_progress < conf.phase[0]) or conf.disable_rgb_grad:         # idr.py:331-334
            points, normals, view_dirs = [a.detach() for a in (points, normals, view_dirs)]
        return self.rendering_network(points, normals, view_dirs, feature_vectors, folded=folded)

    def get_rbg_value(self, points, view_dirs, train_progress):
        """Stand-alone form (idr.py:324-338): evaluates the SDF net at `points` afresh."""
        net, ws, bs = self.implicit_network.fold()
        N = points.shape[0]
        y, normals, _ = Fn.sdf_value_normal(net, ws, bs, points, N)
        feature_vectors = y[:, 2:]
        if (train_progress is not None and train_progress < conf.phase[0]) or conf.disable_rgb_grad:
            points, normals, view_dirs = [a.detach() for a in (points, normals, view_dirs)]
        return self.rendering_network(points, normals, view_dirs, feature_vectors)
