"""Every entry point of the library that allocates a workspace or an output, run on dirty memory: under helpers.dirty_allocations every
torch.empty / torch.empty_like the library makes is filled, by bytes, with 0xff, with 0x00 and with 0x5a before it is handed out, and the result is
held to the numpy / float64 restatement exactly as that module's own test file holds it on clean memory -- the same comparison helpers, the same
masks, against the restatement and never against a clean run of the device code.  A counter that is never cleared, a key that is never set to
EMPTY, a flag array cleared one chunk short: each reads plausible values on fresh or recycled memory and garbage here.

The cases are small: the sizes at which a workspace first has a second leaf, a second tree level (17, 129 points) or a second scan chunk (2049
items), and otherwise the smallest case of the module's own file.  Each is a function `case_*` below, registered with the entry points it covers
(CASES: 'module.entry' -> the names of its cases); tests/test_dirty_memory_table_host.py holds that table to the library's source.  Two guards keep
a case from passing vacuously: test_poison_reads_back_as_bytes, and _guarded: every registered entry point that returns under the context must have
drawn at least one poisoned allocation during that very call (KEEPS_ITS_ALLOCATION names the few that may reuse one: for them, during the case),
and every entry a case registers must have been called by it.

The restatements are computed once per case and kept for the three patterns (_memo_refs: the functions of the *_ref modules, keyed by their
arguments' bytes; every caller receives its own copy).

Objects that keep a workspace across calls (the nearest-neighbour tree and the ICP pairs on it, bundle's blocks, the Poisson call, the matcher's
batches, the feature extractor) have a sequence on one object each -- a larger problem, then a smaller one; a refused call, then a valid one --
whose last call equals the restatement of that call alone: stale state of the library's own making, which a poisoned fresh allocation cannot
reach."""
import collections
import contextlib
import copy
import functools
import hashlib
import importlib
import inspect
import pickle
import pkgutil
import sys
import types

import numpy as np
import pytest
import torch

from helpers import POISON_PATTERNS, clean_allocations, dirty_allocations

pytestmark = pytest.mark.gpu

# the modules whose scratch is carved from one byte buffer (csrc/geom_prims.h: WsCursor): none of their entries may be exempt
MODULES = ('chamfer', 'cloud', 'normals', 'poisson', 'registration', 'global_reg', 'keypoints', 'bundle', 'fusion', 'tsdf', 'stereo', 'raster',
           'texture', 'viewsel', 'undistort', 'features', 'mesh')
CASES = collections.defaultdict(list)          # 'module.entry' -> [case function names]
CASE_KEYS = {}                                 # case function name -> the entries it must call
NOT_COVERED = {}                               # 'module.entry' -> reason (filled below)
REF_MODULES = ('bundle_ref', 'chamfer_ref', 'cloud_ref', 'fusion_normals_ref', 'fusion_ref', 'global_reg_ref', 'keypoints_ref', 'maxflow_ref',
               'mc_ref', 'normals_ref', 'poisson_ref', 'raster_ref', 'registration_ref', 'simplify_ref', 'smc_ref', 'stereo_cascade_ref',
               'stereo_ref', 'stereo_sgm_ref', 'texture_ref', 'tsdf_ref', 'undistort_ref', 'viewsel_ref')


def case(*keys):
    def register(fn):
        assert fn.__name__.startswith('case_') and fn.__name__ not in CASE_KEYS
        CASE_KEYS[fn.__name__] = keys
        for k in keys:
            CASES[k].append(fn.__name__)
        return fn
    return register


# the test files whose helpers, scenes and assertions the cases use
TEST_MODULES = ('test_gpu_bundle', 'test_gpu_chamfer', 'test_gpu_cloud', 'test_gpu_diff_fp64', 'test_gpu_dsurf', 'test_gpu_f32x3', 'test_gpu_featext',
                'test_gpu_fusion', 'test_gpu_global_reg', 'test_gpu_keypoints', 'test_gpu_loss', 'test_gpu_loss_edges', 'test_gpu_mesh',
                'test_gpu_mesh_cut', 'test_gpu_mesh_sparse', 'test_gpu_native_step', 'test_gpu_normals', 'test_gpu_poisson', 'test_gpu_raster',
                'test_gpu_registration', 'test_gpu_simplify', 'test_gpu_step', 'test_gpu_step_bookkeeping', 'test_gpu_stereo',
                'test_gpu_stereo_cascade', 'test_gpu_stereo_sgm', 'test_gpu_texture', 'test_gpu_trace', 'test_gpu_trace_edges', 'test_gpu_tsdf',
                'test_gpu_undistort', 'test_gpu_viewsel', 'test_gpu_weight_packs')


def T(name):
    """the module's own test file (imported late: the table above is read without a device)"""
    assert name in TEST_MODULES, name
    return importlib.import_module(name)


# ------------------------------------------------------------------------------------------------ the guards
def _entry(key):
    """'module.fn' or 'module.Class.method' -> (owner object, attribute name, the raw attribute)"""
    parts = key.split('.')
    mod = importlib.import_module('mvsdf_amd.' + parts[0])
    if len(parts) == 2:
        return mod, parts[1], getattr(mod, parts[1])
    cls = getattr(mod, parts[1])
    return cls, parts[2], vars(cls)[parts[2]]


# entry points that may return without allocating: an object that keeps its allocation across calls, or a call that declines its work.  For these
# the guard is per case: at least one of their calls allocated.
KEEPS_ITS_ALLOCATION = {'features.FeatExt.packed': 'the packed weights live until a parameter changes',
                        'features.FeatExt.run': 'the activation workspace is kept while it is large enough; the outputs are the caller\'s',
                        'ops.fold_backward_net_flat': 'adds into the gradient sink when the caller gives one',
                        'native_step.direct_backward': 'returns False at once for a loss that is not the native step\'s'}


@contextlib.contextmanager
def _guarded(log, calls, allocating):
    """every entry point of CASES, wrapped: a call that returns must have drawn a poisoned allocation of its own.  A function that a test file
    or another module of the library bound by `from ... import` is wrapped under that name too."""
    def wrap(key, f):
        @functools.wraps(f)
        def g(*a, **k):
            if _SETUP[0]:
                return f(*a, **k)
            before = log.count
            out = f(*a, **k)
            if key in KEEPS_ITS_ALLOCATION:
                allocating[key] += log.count > before
            else:
                assert log.count > before, '%s returned without a poisoned allocation' % key
            calls[key] += 1
            return out
        return g

    saved = []
    try:
        users = [m for n, m in list(sys.modules.items()) if m is not None and (n.startswith('test_gpu_') or n.startswith('mvsdf_amd'))]
        for key in list(CASES):
            owner, name, raw = _entry(key)
            if isinstance(raw, property):
                new = property(wrap(key, raw.fget), raw.fset, raw.fdel)
            elif isinstance(raw, (staticmethod, classmethod)):
                new = type(raw)(wrap(key, raw.__func__))
            else:
                new = wrap(key, raw)
            saved.append((owner, name, raw))
            setattr(owner, name, new)
            if inspect.isfunction(raw) and not inspect.isclass(owner):
                for m in users:
                    for attr, val in list(vars(m).items()):
                        if val is raw and m is not owner:
                            saved.append((m, attr, raw))
                            setattr(m, attr, new)
        yield
    finally:
        for owner, name, raw in saved:
            setattr(owner, name, raw)


_REFS = {}
_PLAIN = (np.ndarray, np.generic, int, float, complex, str, bytes, bool, type(None))


def _plain(x):
    if isinstance(x, (tuple, list)):
        return all(_plain(y) for y in x)
    return isinstance(x, _PLAIN)                                   # (a dict argument may be one the function fills: computed afresh)


@contextlib.contextmanager
def _memo_refs():
    """the public functions of the restatement modules, called from a test, return what they returned before for the same arguments (arrays and
    numbers only; anything else is computed afresh), as a copy of their own for every caller.  The calls a restatement makes itself are left alone:
    some of its helpers work in place.  This rests on one property of tests/*_ref.py: a public restatement called from a test is a pure function
    of its array and number arguments -- no global random state, no result written into an argument (a dict it fills is never cached).  A
    restatement that breaks this must be left out of REF_MODULES."""
    depth = [0]

    def wrap(mod, f):
        @functools.wraps(f)
        def g(*a, **k):
            if depth[0] or not (_plain(a) and _plain(list(k.values()))):
                return f(*a, **k)
            key = (mod, f.__name__, hashlib.sha1(pickle.dumps((a, sorted(k.items())), protocol=4)).hexdigest())
            if key not in _REFS:
                depth[0] += 1
                try:
                    _REFS[key] = f(*a, **k)
                finally:
                    depth[0] -= 1
            return copy.deepcopy(_REFS[key])
        return g

    saved = []
    try:
        for name in REF_MODULES:
            mod = importlib.import_module(name)
            for attr, f in list(vars(mod).items()):
                if isinstance(f, types.FunctionType) and f.__module__ == name and not attr.startswith('_'):
                    saved.append((mod, attr, f))
                    setattr(mod, attr, wrap(name, f))
        yield
    finally:
        for mod, attr, f in saved:
            setattr(mod, attr, f)


def _import_everything():
    """the test files the cases use and every module of the library: none is imported for the first time while the entry points are wrapped"""
    import mvsdf_amd
    for module in TEST_MODULES:
        importlib.import_module(module)
    for info in pkgutil.walk_packages(mvsdf_amd.__path__, 'mvsdf_amd.'):
        if info.name.rsplit('.', 1)[-1] != 'build' and not info.name.rsplit('.', 1)[-1].startswith('lib'):    # (not the shared libraries)
            importlib.import_module(info.name)


def run_dirty(name, pattern):
    """-> the number of guarded calls per entry point"""
    fn = globals()[name]
    _import_everything()                                           # before the guards go up: what a module binds with `from ... import` is found and wrapped
    calls, allocating = collections.Counter(), collections.Counter()
    with _memo_refs(), dirty_allocations(pattern) as log, _guarded(log, calls, allocating):
        fn(pattern) if inspect.signature(fn).parameters else fn()
    torch.cuda.synchronize()
    assert log.count > 0 and log.bytes > 0, name
    missed = [key for key in CASE_KEYS[name] if calls[key] < 1 or (key in KEEPS_ITS_ALLOCATION and allocating[key] < 1)]
    assert not missed, '%s never called %s, or never with an allocation (called: %s)' % (name, missed, sorted(calls))
    return calls


_FIXTURES = {}
_SETUP = [False]


@contextlib.contextmanager
def setup():
    """a case's own set-up: clean allocations, and the entry points unguarded"""
    _SETUP[0] = True
    try:
        with clean_allocations():
            yield
    finally:
        _SETUP[0] = False


@contextlib.contextmanager
def launches_nothing():
    """a call that is answered before any kernel or allocation: the per-call guard stands aside, the poison stays"""
    _SETUP[0] = True
    try:
        yield
    finally:
        _SETUP[0] = False


def fixture_value(module, name, param=None):
    """the value of a (module-scoped) fixture of another test file, made once and on clean memory"""
    key = (module, name, repr(param))
    if key not in _FIXTURES:
        f = getattr(T(module), name)
        raw = getattr(f, '__wrapped__', None) or f.__pytest_wrapped__.obj
        with setup():
            _FIXTURES[key] = raw(types.SimpleNamespace(param=param)) if inspect.signature(raw).parameters else raw()
    return _FIXTURES[key]


def bits64(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def np_(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ the helper itself
DTYPES = (torch.uint8, torch.bool, torch.int32, torch.int64, torch.float32, torch.float64, torch.bfloat16)


@pytest.mark.parametrize('pattern', POISON_PATTERNS, ids=lambda p: '0x%02x' % p)
def test_poison_reads_back_as_bytes(pattern):
    """every dtype the library allocates, a length that is no multiple of 8, a zero-length tensor, empty_like of a strided view, a host tensor"""
    e0, el0 = torch.empty, torch.empty_like
    with dirty_allocations(pattern) as log:
        assert torch.empty is not e0
        want_count = want_bytes = 0
        for dt in DTYPES:
            for shape in ((13,), (3, 5, 7), (0,), (2049,)):
                x = torch.empty(shape, dtype=dt, device='cuda')
                raw = x.view(-1).view(torch.uint8)
                assert raw.numel() == x.numel() * x.element_size() and bool((raw == pattern).all()), (dt, shape)
                want_count += 1
                want_bytes += raw.numel()
            y = torch.empty_like(torch.zeros(6, 10, dtype=dt, device='cuda')[:, 1:8:2])
            assert bool((y.contiguous().view(-1).view(torch.uint8) == pattern).all()), dt
            want_count += 1
            want_bytes += y.numel() * y.element_size()
        assert torch.empty(5, 3, device='cuda', dtype=torch.int32).tolist() == [[int.from_bytes(bytes([pattern] * 4), 'little', signed=True)] * 3] * 5
        want_count, want_bytes = want_count + 1, want_bytes + 60
        host = torch.empty(16)                                                # host allocations are handed out as they are, and not counted
        assert not host.is_cuda
        assert (log.count, log.bytes) == (want_count, want_bytes)
        f = torch.empty(4, device='cuda')
        assert bool(torch.isnan(f).all()) if pattern == 0xff else bool((f == 0).all()) if pattern == 0 else bool((f > 1e16).all())
    assert torch.empty is e0 and torch.empty_like is el0


# ------------------------------------------------------------------------------------------------ cloud
@case('cloud.knn_mean_distance')
def case_cloud_knn():
    """17 and 129 points: a second leaf, a second tree level; k beside two list capacities; the cloud with exact duplicates"""
    from mvsdf_amd import cloud
    C = T('test_gpu_cloud')
    for n, k in ((17, 8), (129, 9), (129, 20)):
        P = C.make_cloud('duplicates', n)
        want = C.R.knn_mean_distance(P, k)
        assert len(np.unique(want)) > n // 2 and (want > 0).all()
        got = np_(cloud.knn_mean_distance(torch.from_numpy(P).cuda() if k == 9 else P, k))
        assert C.same_bits(got, want), (n, k, int((C.bits(got) != C.bits(want)).sum()))


@case('cloud.radius_components')
def case_cloud_components():
    C = T('test_gpu_cloud')
    for kind in ('uniform', 'lattice'):
        for n in (17, 129, 2049):
            C.test_radius_components_at_the_tree_shape_edges(kind, n)             # (asserts 1 < components < n for the uniform cloud)


@case('cloud.compact')
def case_cloud_compact():
    """2049 flags: a second scan chunk holding one item; some kept, some dropped"""
    C = T('test_gpu_cloud')
    i = torch.arange(2049)
    for keep in (i % 2, i == 2048, (i * 7) % 5 == 0):
        assert 0 < int(keep.sum()) < 2049
        C._compact_case(2049, keep.to(torch.uint8))


@case('cloud.clean_points')
def case_cloud_clean_points():
    from mvsdf_amd import cloud
    C = T('test_gpu_cloud')
    P, injected = C.CS.injected()
    P, injected = np.ascontiguousarray(P[::4]), injected[::4]
    colors = np.random.RandomState(8).randint(0, 256, size=(len(P), 3)).astype(np.uint8)
    kw = dict(nb_neighbors=12, knn_ratio=2.0, eps_ratio=4.0, cluster_frac=0.01)
    want = C.R.clean(P, k=12, knn_ratio=2.0, eps_ratio=4.0, cluster_frac=0.01, jobs=C.JOBS)
    assert 0 < int(want['keep'].sum()) < len(P) and want['n_clusters'] > 1 and 0 < want['n_passed'] < len(P)
    C._assert_clean_is(cloud.clean_points(P, colors, **kw), want, P, colors)


@case('cloud.clean_fused', 'fusion.fuse_depths')
def case_cloud_clean_fused():
    T('test_gpu_cloud').test_clean_fused_removes_the_floater_and_its_depths()     # (asserts that the floater is there and goes, and the sphere stays)


# ------------------------------------------------------------------------------------------------ chamfer
@case('chamfer.nearest_distance')
def case_chamfer_nearest():
    C = T('test_gpu_chamfer')
    for nr in (17, 129, 2049):
        C.test_nearest_at_the_tree_shape_edges(nr)                                # (asserts zeros at the references and +inf beyond max_dist)


@case('chamfer.downsample')
def case_chamfer_downsample():
    """3002 points, two of them far away: a second chunk; the chain whose every other point falls"""
    from mvsdf_amd import chamfer
    C = T('test_gpu_chamfer')
    for name, density in (('outliers', 0.2), ('chain', 0.2), ('one_cell', 0.05)):
        p = C._cases()[name]
        want = C.chamfer_ref.downsample(p, density, 1)
        assert want.dtype == bool and 0 < int(want.sum()) < len(p)
        assert np.array_equal(np_(chamfer.downsample(torch.from_numpy(p).cuda(), density, 1)), want)


@case('chamfer.sample_mesh', 'chamfer.masks', 'chamfer.dtu_chamfer', 'chamfer.downsample')
def case_chamfer_fixture_mesh():
    C = T('test_gpu_chamfer')
    path = [p for p in C.FIXTURES if p.endswith('mesh.npz')][0]
    z = C._fixture(path)
    assert 0 < z['in'].sum() < len(z['in']) and 0 < z['above'].sum() < len(z['above']) and 0 < z['kept'].sum() < len(z['kept'])
    C.test_fixture_every_step(path)


@case('chamfer.dtu_chamfer')
def case_chamfer_fixture_points():
    C = T('test_gpu_chamfer')
    C.test_fixture_every_step([p for p in C.FIXTURES if p.endswith('pcd_seed7.npz')][0])


# ------------------------------------------------------------------------------------------------ normals
@case('normals.knn_indices', 'normals.estimate_normals')
def case_normals_rows():
    N = T('test_gpu_normals')
    for kind, n, k in (('duplicates', 17, 8), ('uniform', 129, 9), ('lattice', 129, 16)):
        P = N.make_cloud(kind, n)
        idx, d2 = N.R.knn_indices(P, k)
        assert len(np.unique(idx)) > n // 2 and (d2[:, -1] > 0).all()
        N._check_rows(P, k, idx, d2, device_input=k == 9)


@case('normals.orient_normals')
def case_normals_orient():
    """17 and 129 points with random signs (flips and keeps, asserted), the smallest clouds, three components, the view vote"""
    N = T('test_gpu_normals')
    for n, k in ((17, 4), (129, 8)):
        P, out = N.sphere(n, n)
        nb, _ = N.R.knn_indices(P, k)
        flipped = out * np.where(np.random.RandomState(n).uniform(size=(n, 1)) < 0.5, -1.0, 1.0)
        want = N._check_orient(P, flipped, nb)
        changed = (bits64(want[0]) != bits64(flipped)).any(1)
        assert changed.any() and not changed.all() and want[3] >= 1
    N.test_orient_smallest_cloud(1)
    N.test_orient_smallest_cloud(8)
    N.test_orient_three_components()                                              # 2515 points: a second chunk of the edge sort
    N.test_orient_view_vote_tie_falls_back_to_up()


@case('normals.orient_to_views')
def case_normals_orient_to_views():
    T('test_gpu_normals').test_orient_to_views()                                  # (asserts ties, majorities either way and unseen points)


# ------------------------------------------------------------------------------------------------ registration
@case('registration.NearestTree.__init__', 'registration.NearestTree.query')
def case_registration_query():
    G = T('test_gpu_registration')
    for nr in (17, 129, 2049):
        G.test_query_sizes(nr)                                                    # (asserts finite and infinite distances)
    G.test_query_ties_and_the_strict_cut_off()


@case('registration.NearestTree.query')
def case_registration_tree_sequence():
    """one tree object: a large query, then a smaller different one, a refused one (NaN), then a valid one -- each the restatement of itself alone"""
    G = T('test_gpu_registration')
    rs = np.random.RandomState(5)
    refs = rs.uniform(-1, 1, (2049, 3))
    tree = G.G.NearestTree(refs)
    big, small = rs.uniform(-1.3, 1.3, (2049, 3)), rs.uniform(-1.3, 1.3, (17, 3))
    rd = G._check_query(tree, refs, big, 0.1)
    assert np.isinf(rd).any() and np.isfinite(rd).any()
    rd = G._check_query(tree, refs, small, 0.2)
    assert np.isinf(rd).any() and np.isfinite(rd).any()
    bad = big.copy()
    bad[2048, 2] = np.nan
    with pytest.raises(ValueError):
        tree.query(bad, 0.1)
    G._check_query(tree, refs, small[:5] * 0.5, float('inf'))
    G._check_query(tree, refs, big, 0.1)


@case('registration.transform_points')
def case_registration_transform():
    T('test_gpu_registration').test_transform_points()


@case('registration.crop_volume')
def case_registration_crop():
    T('test_gpu_registration').test_crop_volume()                                 # (asserts kept counts strictly between none and all)


@case('registration.voxel_downsample')
def case_registration_voxel():
    T('test_gpu_registration').test_voxel_downsample()


@case('registration.pair_sums')
def case_registration_pair_sums():
    G = T('test_gpu_registration')
    G.test_the_17_sums_of_an_iteration(2049)                                      # (asserts that about half the pairs match)
    G.test_the_17_sums_of_an_iteration(257)
    G.test_no_matched_pair()


@case('registration.pair_sums', 'registration.icp')
def case_registration_icp_sequence():
    """one target tree: the ICP of a larger source, the sums of a smaller different one, a refused ICP (no pair within reach), the first again"""
    G = T('test_gpu_registration')
    R, H = G.R, G.H
    src, tgt = H.rigid_copy()
    tree = G.G.NearestTree(tgt)

    def icp_is_the_restatement():
        reg = G.G.icp(src, tree, max_dist=0.3)
        Tm, fitness, rmse, iterations = R.icp(src, tgt, max_dist=0.3)
        assert G._same(reg.transformation, Tm) and G._same(reg.fitness, fitness) and G._same(reg.inlier_rmse, rmse) and reg.iterations == iterations
        assert iterations > 1 and 0 < fitness <= 1 and not np.array_equal(Tm, np.eye(4))
    icp_is_the_restatement()
    small = G._half_matched(257, 3)
    cnt, sums, d2, index = G.G.pair_sums(small, tree, np.eye(4), 0.3)
    rc, rsums, rd2, rindex = R.pair_sums(small, tgt, np.eye(4), 0.3)
    assert 0 < rc < 257 and cnt == rc and np.array_equal(np_(index), rindex) and G._same(np_(d2), rd2) and G._same(sums, rsums)
    with pytest.raises(ValueError):
        G.G.icp(small + [0, 0, 50.0], tree, max_dist=0.3)
    icp_is_the_restatement()


@case('registration.fscore')
def case_registration_fscore():
    T('test_gpu_registration').test_fscore()


@case('registration.tnt_evaluate')
def case_registration_tnt():
    """the scene of the file's end-to-end test with its one-stage table: every field of the result"""
    G = T('test_gpu_registration')
    rec, gt, _ = G.scene()
    one = [('voxel', G.TAU, 80 * G.TAU)]
    r = G.G.tnt_evaluate(rec, gt, G.H.CROP, np.eye(4), G.TAU, stages=one)
    ref = G.R.tnt_evaluate(rec, gt, G.H.CROP, np.eye(4), G.TAU, stages=one)
    assert r['points'] == ref['points'] and r['points'][2] < 6000 and r['points'][3] < 5000
    assert G._same(r['transformation'], ref['transformation']) and not np.array_equal(ref['transformation'], np.eye(4))
    for k in ('precision', 'recall', 'fscore'):
        assert G._same(r[k], ref[k]), k
    assert np.array_equal(r['histograms'][0], ref['histograms'][0]) and np.array_equal(r['histograms'][1], ref['histograms'][1])
    assert G._same(r['edges'], ref['edges']) and (r['below_rec'], r['below_gt']) == (ref['below_rec'], ref['below_gt'])
    assert 0 < ref['fscore'] < 1


# ------------------------------------------------------------------------------------------------ global_reg
@case('global_reg.spfh', 'global_reg.fpfh')
def case_global_reg_descriptors():
    Gr = T('test_gpu_global_reg')
    for n, k in ((17, 8), (129, 8), (129, 32)):
        P = Gr.make_cloud('uniform', n, seed=1)
        rs = np.random.RandomState(n)
        N = rs.normal(size=(n, 3))
        N /= np.linalg.norm(N, axis=1, keepdims=True)
        N[rs.uniform(size=n) < 0.05] = 0.0
        rows, d2 = Gr.NR.knn_indices(P, k)
        radius = float(np.sqrt(np.median(d2[:, 0])))
        nb = np.ascontiguousarray(rows)
        nb[::7, 0] = np.arange(n, dtype=np.int32)[::7]
        Gr._check_descriptor(P, N, nb, None, (n, k, None))
        count = Gr._check_descriptor(P, N, nb, radius, (n, k, radius))
        assert (count == 0).any() and (count > 0).any()


@case('global_reg.match_features')
def case_global_reg_match():
    """the matcher's smallest crosswise sizes, both orders, mutual (kept and rejected matches), the split targets (atomicMin keys), then the same
    sizes again in falling order: a smaller problem after a larger one"""
    Gr = T('test_gpu_global_reg')
    sizes = (1, 15, 16, 17, 65)
    for ns in sizes:
        for nt in sizes:
            Gr._check_match(Gr._codes(ns, 1), Gr._codes(nt, 2))
    want_i, _ = Gr._check_match(Gr._codes(257, 6), Gr._codes(63, 7), mutual=True)
    assert (want_i >= 0).any() and (want_i < 0).any()
    t = Gr._codes(2049, 9).copy()
    t[2046] = t[7]
    s = Gr._codes(130, 10).copy()
    s[0] = t[7]
    assert Gr.global_reg.match_splits(130, 2049) >= 2
    want_i, want_d = Gr._check_match(s, t)
    assert want_i[0] == 7 and want_d[0] == 0
    Gr._check_match(Gr._codes(17, 1), Gr._codes(15, 2))
    Gr.test_match_extremes_and_ties()


@case('global_reg.ransac')
def case_global_reg_ransac():
    Gr = T('test_gpu_global_reg')
    src, dst, motion = Gr._motion_case()
    for M, H in ((257, 65), (257, 4096), (4, 64)):
        want = Gr._check_ransac(src, dst, Gr._corr(M, 0), 0.03, H, seed=H)
    want = Gr._check_ransac(src, dst, Gr._corr(257, 0), 0.03, 4096, seed=4096)
    assert want.hypothesis >= 0 and 0.25 * 257 <= want.inliers < 257 and 0 < want.mask.sum() < 257
    one = np.stack([np.arange(300), np.zeros(300, np.int64)], 1).astype(np.int32)
    want = Gr._check_ransac(src, dst, one, 0.5, 4096, seed=1)                      # every hypothesis rejected, after a call that found one
    assert want.hypothesis == -1 and want.checked == 0


# ------------------------------------------------------------------------------------------------ bundle
BUNDLE = ('bundle.residuals', 'bundle.normal_blocks', 'bundle.schur_apply', 'bundle.solve_reduced', 'bundle.apply_step')


@case(*BUNDLE)
def case_bundle_stages():
    B = T('test_gpu_bundle')
    for V, P in ((3, 7), (4, 120)):
        for huber in (None, 1.0):
            s, (r, terms, cost), bl, x, n, (pose, xyz, ok) = B.stages(V, P, huber)
            assert cost > 0 and np.abs(r).max() > 0 and np.abs(x).max() > 0 and not np.array_equal(xyz, s.xyz)
            assert not np.abs(x[0]).any() and np.abs(x[1:]).min() > 0               # the fixed view does not move, the others do
            B.test_every_stage_equals_the_restatement(V, P, huber)


@case('bundle.normal_blocks', 'bundle.schur_apply', 'bundle.residuals')
def case_bundle_view_sums():
    B = T('test_gpu_bundle')
    B.test_view_sums_at_the_tree_chunk_boundary(2049)
    B.test_view_sums_at_the_tree_chunk_boundary(0)                                 # (asserts the unobserved view's zero block)


@case('bundle.bundle_adjust')
def case_bundle_adjust():
    B = T('test_gpu_bundle')
    for name in ('plain', 'huber', 'rejects', 'converges'):
        B.test_bundle_adjust_equals_the_restatement(name)                         # (asserts rejected steps and early convergence)
    B.test_unobserved_view_short_track_and_all_fixed()                            # the entries the step kernels copy: fixed views, a short track
    s = B.scene_of(3, 7, fixed=(0,))
    want = B.R.bundle_adjust(*B.args(s), fixed_views=(0,), iterations=3)
    assert want.cost < want.cost0 and want.accepted > 0
    B._same_result(B.BA.bundle_adjust(*B.args(s), fixed_views=(0,), iterations=3), want)


@case('bundle.normal_blocks', 'bundle.solve_reduced', 'bundle.schur_apply', 'bundle.apply_step')
def case_bundle_blocks_sequence():
    """blocks.ws across calls: solves of many and of few iterations, another right-hand side, a refused vector (wrong shape), then the stages
    again on the same object; then a smaller problem's blocks, while the larger one's stay valid"""
    B = T('test_gpu_bundle')
    for cg in (64, 1, 0):
        B.test_solver_state_and_frozen_launches(cg)
    s, _, bl, x, n, (pose, xyz, ok) = B.stages(4, 120, None)
    g = B.BA.normal_blocks(*B.args(s), fixed_views=(0,), lam=1e-3)
    probe = np.random.RandomState(1).normal(size=(4, 6))
    assert B.eq(B.BA.schur_apply(g, probe), B.R.schur_apply(bl, probe))
    with pytest.raises(ValueError):
        B.BA.schur_apply(g, probe[:3])
    with pytest.raises(ValueError):
        B.BA.solve_reduced(g, cg_iters=-1)
    s2, _, bl2, x2, n2, (pose2, xyz2, ok2) = B.stages(3, 7, None)
    g2 = B.BA.normal_blocks(*B.args(s2), fixed_views=(0,), lam=1e-3)
    gx2, gn2 = B.BA.solve_reduced(g2, 64, 1e-8)
    assert gn2 == n2 and B.eq(gx2, x2)
    gx, gn = B.BA.solve_reduced(g, 64, 1e-8)
    assert gn == n and B.eq(gx, x) and 0 < n < 64
    gc, gxyz, gok = B.BA.apply_step(g, x)
    assert gok == ok and B.eq(gc, B.R.cams_with(s.cams, pose)) and B.eq(gxyz, xyz)
    assert B.eq(B.BA.schur_apply(g, probe), B.R.schur_apply(bl, probe))


@case('bundle.bundle_adjust', 'bundle.residuals')
def case_bundle_refusal_then_valid():
    """an error bit (a point behind its camera, a NaN), then the valid call equals the restatement"""
    B = T('test_gpu_bundle')
    B.test_behind_a_camera_is_a_value_not_a_trap()
    s = B.scene_of(4, 120)
    bad = s.xyz.copy()
    bad[7, 1] = np.nan
    with pytest.raises(ValueError, match='NaN or infinite'):
        B.BA.bundle_adjust(s.cams, bad, s.off, s.view, s.obs)
    want = B.R.bundle_adjust(*B.args(s), iterations=2)
    assert want.cost < want.cost0
    B._same_result(B.BA.bundle_adjust(*B.args(s), iterations=2), want)


# ------------------------------------------------------------------------------------------------ poisson
@case('poisson.reconstruct', 'poisson.Field.valid', 'poisson.Field.volume', 'mesh.marching_cubes_masked')
def case_poisson_reconstruct():
    Pn = T('test_gpu_poisson')
    Pn.test_reconstruct_equals_the_restatement(2, 6, 1, 1)
    Pn.test_reconstruct_equals_the_restatement(3, 200, 8, 2)
    ref = Pn._ref(3, 200, 8, 2)
    assert ref['residual'] < ref['residual0'] and ref['chi'].any() and (ref['density'] > 0).any() and not (ref['density'] > 0).all()
    assert len(Pn.R.mesh(ref)[1]) > 0                                              # the mesh the first call compared is not empty
    Pn.test_valid_masks(3, 200)                                                   # (asserts that the masks differ)
    Pn.test_point_counts_around_the_tree_chunk(2049)


@case('poisson.reconstruct')
def case_poisson_sequence():
    """a larger cloud, then a smaller one on another grid, a refused one (a NaN coordinate; then nothing admitted), then the first again"""
    from mvsdf_amd import poisson
    Pn = T('test_gpu_poisson')
    p, nrm, o, h = Pn._cloud(3, 200)
    Pn._check(*Pn._cloud(4, 4000), 4, ref=Pn._ref(4, 4000, 1, 1), cycles=1, sweeps=1)
    Pn._check(p, nrm, o, h, 3, ref=Pn._ref(3, 200, 8, 2))
    q = p.copy()
    q[17, 1] = np.nan
    with pytest.raises(ValueError):
        poisson.reconstruct(q, nrm, o, h, 3)
    Pn.test_edge_points()                                                          # (points outside the grid are counted; none admitted at all)
    Pn._check(p, nrm, o, h, 3, ref=Pn._ref(3, 200, 8, 2))
    call = poisson._Call(p, nrm, o, h, 3, 8, 2, 'reconstruct')                     # the object the stages share: its workspace, chi, density, values
    for _ in range(2):                                                             # the second run starts on what the first one left
        call.run()
        Pn._check_field(call.finish(), Pn._ref(3, 200, 8, 2))
    for stage in (poisson.STAGE_SPLAT, poisson.STAGE_SOLVE, poisson.STAGE_ISO):    # and stage by stage, as tools/time_poisson.py runs them
        call.run(stage)
    Pn._check_field(call.finish(), Pn._ref(3, 200, 8, 2))


# ------------------------------------------------------------------------------------------------ fusion
@case('fusion.fuse_depths')
def case_fusion_fuse():
    Fu = T('test_gpu_fusion')
    Fu.test_equals_the_restatement((20, 28), True)                                # (asserts more than 50 points)
    cams, depths, pairs = Fu.S.make_views(6, (20, 28), clean=False)
    ref = Fu.R.fuse(cams, depths, pairs)
    assert 0 < len(ref['points']) < int((depths > 0).sum()) and (ref['counts'] > 0).any() and (ref['fused_depths'] == 0).any()
    Fu._check(cams, depths, pairs)
    Fu.test_emit_across_a_scan_chunk_edge((1, 3, 683))                            # 2049 pixels: a second chunk holding one
    Fu.test_emit_across_a_scan_chunk_edge((2, 32, 33))


@case('fusion.depth_normals', 'fusion.fuse_depths')
def case_fusion_normals():
    Pn = T('test_gpu_poisson')
    Pn.test_fused_normals_equal_the_restatement((20, 28), True)                   # (asserts a kept pixel without a normal)
    Pn.test_normals_at_borders_lonely_pixels_and_depth_steps()


# ------------------------------------------------------------------------------------------------ tsdf
@case('tsdf.integrate_depths', 'mesh.marching_cubes_masked')
def case_tsdf():
    Ts = T('test_gpu_tsdf')
    Ts.test_integration_and_mesh_equal_the_restatement((17, 17, 17), (20, 28), True, 1)     # (asserts valid and invalid voxels and a mesh)
    Ts.test_integration_and_mesh_equal_the_restatement((17, 17, 17), (20, 28), False, 2)
    Ts.test_jump_views_single_view_and_the_smallest_grid()
    Ts.test_masked_extraction_on_random_fields((5, 9, 66))


# ------------------------------------------------------------------------------------------------ stereo
@case('stereo.patch_descriptors', 'stereo.normalize_descriptors', 'stereo.plane_sweep')
def case_stereo_sweep():
    St = T('test_gpu_stereo')
    St.test_odd_shapes((17, 16))                                                  # 4 views, two sources each (asserts that some pixel has an estimate)
    St.test_odd_shapes((37, 53))
    St.test_channel_counts(25)                                                    # views=[2]: the other views keep "no estimate"
    St.test_hypotheses_behind_and_outside_a_source()                              # (asserts pixels with 0, 1 and 2 sources)


@case('stereo.regularize_scores')
def case_stereo_regularize():
    Sg = T('test_gpu_stereo_sgm')
    volumes = fixture_value('test_gpu_stereo_sgm', 'volumes')
    for shape in ((2, 3, 5), (24, 17, 33), (300, 6, 11)):
        assert np.isnan(volumes[shape]).any() and not np.isnan(volumes[shape]).all()
        for paths in (4, 8):
            Sg.test_regularize_scores_is_the_restatement(volumes, shape, paths)
    Sg.test_defaults_and_an_infinite_score()                                      # a refusal, then a valid call


@case('stereo.plane_sweep')
def case_stereo_sweep_sgm():
    Sg = T('test_gpu_stereo_sgm')
    noisy = fixture_value('test_gpu_stereo_sgm', 'noisy')
    Sg.test_regularize_forms_and_the_unregularised_sweep(noisy)
    cams, pairs, desc = noisy
    desc, cams = desc[:, :24, :40], cams.copy()
    cams[:, 1, 0, 2], cams[:, 1, 1, 2] = 20.0, 12.0
    ref = Sg.G.sweep(desc, cams, pairs, 2, None, *Sg.G.DEFAULTS)
    plain = Sg.R.sweep(desc, cams, pairs, 2)
    assert (ref['best_k'] >= 0).any() and (ref['best_k'] != plain['best_k']).any()   # the regularisation decides pixels


@case('stereo.upsample_depth')
def case_stereo_upsample():
    Sc = T('test_gpu_stereo_cascade')
    Sc.test_upsample_depth_is_the_restatement((3, 5), (6, 10))                    # (asserts NaN and finite centres)
    Sc.test_upsample_depth_is_the_restatement((4, 6), (7, 13))


@case('stereo.band_sweep')
def case_stereo_band():
    Sc = T('test_gpu_stereo_cascade')
    Sc.test_band_sweep_is_the_restatement(Sc.BANDS[1])                            # (asserts estimates, unseen hypotheses and untouched views)
    Sc.test_band_sweep_is_the_restatement(Sc.BANDS[3])
    Sc.test_an_infinite_centre_raises_and_the_workspace_is_small()                # a refusal, then a valid call


@case('stereo.cascade_sweep')
def case_stereo_cascade():
    Sc = T('test_gpu_stereo_cascade')
    rendered = fixture_value('test_gpu_stereo_cascade', 'rendered', [(7, 11), (16, 24), (33, 47)])
    Sc.test_cascade_sweep_is_the_restatement(rendered, None)                      # (asserts estimates at most pixels)
    Sc.test_cascade_sweep_is_the_restatement(rendered, True)
    Sc.test_cascade_views_and_device_tensors(rendered)


# ------------------------------------------------------------------------------------------------ raster
@case('raster.rasterize')
def case_raster_rasterize():
    Ra = T('test_gpu_raster')
    Ra.test_triangle_soup()                                                       # (asserts ties, empty boxes, faces partly behind the camera)
    verts, faces, P = Ra.S.soup()
    depth, face = Ra.R.rasterize(verts, faces, P, Ra.S.SOUP_HW, 0.5)
    assert (face >= 0).all() and len(np.unique(face)) > 20                        # the soup covers every pixel, with many faces
    Ra.test_large_face_list_across_a_scan_chunk_edge(683, 3)                      # 2049 (face, view) items
    Ra.test_large_face_list_across_a_scan_chunk_edge(512, 4)


@case('raster.rasterize', 'raster.vertex_visibility', 'raster.color_vertices')
def case_raster_visibility_and_colours():
    Ra = T('test_gpu_raster')
    L = Ra.S.layers()
    face = Ra.R.rasterize(L['verts'], L['faces'], L['P'], Ra.S.HW, 0.5)[1]
    assert 0.2 < (face >= 0).mean() < 0.8                                         # pixels drawn and pixels empty
    Ra.test_visibility_and_colours_of_the_two_layer_scene()                       # (asserts seen, hidden, masked and never-coloured vertices)


# ------------------------------------------------------------------------------------------------ texture
@case('texture.face_views')
def case_texture_face_views():
    Tx = T('test_gpu_texture')
    Tx.test_face_views(fixture_value('test_gpu_texture', 'scene', 'sphere'), 0.5)  # (check_cases: the inputs exercise every label rule; masks change labels)


@case('texture.build_atlas')
def case_texture_build_atlas():
    Tx = T('test_gpu_texture')
    scene = fixture_value('test_gpu_texture', 'scene', 'sphere')
    Tx.test_build_atlas(scene, 1.0)                                               # (asserts valid and invalid texels, three size classes)
    Tx.test_build_atlas(scene, 3.0)
    Tx.test_the_max_size_loop(scene)                                              # a refusal ('do not fit') after a valid atlas


# ------------------------------------------------------------------------------------------------ viewsel
@case('viewsel.view_scores', 'viewsel.pack_visibility')
def case_viewsel_scores():
    Vs = T('test_gpu_viewsel')
    for V, P, pattern in ((3, 63, 'random'), (65, 63, 'blind'), (65, 1000, 'random'), (2, 1, 'all')):
        Vs.test_view_scores_equal_restatement(V, P, pattern)
    points, centers = Vs._scene(65, 1000, seed=65 * 7 + 1000)
    s, c = Vs.R.view_scores(points, centers, Vs._visibility('random', 65, 1000, seed=1065), 5.0, 1.0, 10.0)
    assert (s > 0).any() and (s == 0).any() and (c > 0).any()
    Vs.test_coincident_point_shared_centre_and_duplicate_track_entries()


@case('viewsel.depth_ranges')
def case_viewsel_depth_ranges():
    T('test_gpu_viewsel').test_depth_ranges_equal_restatement_and_name_the_blind_view()     # (a refusal is its last call; the ranges differ per view)


# ------------------------------------------------------------------------------------------------ undistort
@case('undistort.undistort_points', 'undistort.distort_points')
def case_undistort_points():
    Un = T('test_gpu_undistort')
    Un.test_undistort_points_equal_restatement(Un.R.CAMERAS[5])
    Un.test_undistort_points_equal_restatement(Un.R.CAMERAS[9])
    p = Un.R.border_samples(Un.R.W, Un.R.H)[0]
    assert np.abs(Un.R.undistort_points(p, Un.R.CAMERAS[5], None) - p).max() > 0.5     # the model moves points


@case('undistort.undistort_images')
def case_undistort_images():
    Un = T('test_gpu_undistort')
    blank = [c for c in Un.R.CAMERAS if not Un.R.undistort_images(np.zeros((1, Un.R.H, Un.R.W, 1), np.uint8), c, Un._out_camera(c, 1.0))[1].all()]
    assert blank                                                                   # valid and invalid output pixels
    Un.test_undistort_images_equal_restatement(blank[0])
    Un.test_float32_images_equal_restatement(Un.R.CAMERAS[9])


# ------------------------------------------------------------------------------------------------ features
@case('features.conv_layer')
def case_features_layers():
    Fe = T('test_gpu_featext')
    by_name = {c[0]: c for c in Fe.LAYER_CASES}
    for name in ('init_conv5_s2', 'conv1_s2', 'deconv_64_32', 'concat_32_32'):
        Fe.test_layer_alone(by_name[name], (3, 9, 17), (True, True, True))        # _assert_close: against fp64 within the fp32 evaluation's own error
        Fe.test_layer_alone(by_name[name], (1, 13, 21), (False, False, False))


@case('features.FeatExt.forward', 'features.FeatExt.run', 'features.FeatExt.packed', 'features.extract_features', 'features.extract_pyramid')
def case_features_net_sequence():
    """one FeatExt object, whose workspace and packs live across calls: a larger batch, a smaller image, a refused size, a valid one; then the two
    batched readers against the fp64 evaluation"""
    from mvsdf_amd.features import FeatExt, extract_features, extract_pyramid
    Fe = T('test_gpu_featext')
    net = FeatExt()                                                               # its own object: the packs and the workspace are allocated dirty
    net.load_state_dict(Fe.R.make_state_dict(Fe.SEED))
    net = net.cuda().eval()
    Fe.test_featext_vs_reference_fixtures(net, 'featext_3x40x56')
    Fe.test_odd_input_size(net)                                                   # 39 x 57 refused, then 47 x 63
    Fe.test_featext_vs_reference_fixtures(net, 'featext_3x40x56')
    x = torch.randn((3, 3, 40, 56), generator=torch.Generator().manual_seed(9))
    sd = Fe.R.make_state_dict(Fe.SEED)
    r64, r32 = Fe.R.featext64(sd, x), Fe.R.featext64(sd, x, torch.float32)
    assert float(r64[2].abs().max()) > 0
    Fe._assert_close(extract_features(net, x.cuda(), batch=2), r64[2], r32[2], 'extract_features')
    for got, a, b in zip(extract_pyramid(net, x, batch=2), r64, r32):
        Fe._assert_close(got.permute(0, 3, 1, 2), a, b, 'extract_pyramid')


# ------------------------------------------------------------------------------------------------ mesh
@case('mesh.marching_cubes')
def case_mesh_marching_cubes():
    Me = T('test_gpu_mesh')
    Me.test_random_volumes_match_the_restatement((2, 2, 2))
    Me.test_random_volumes_match_the_restatement((5, 6, 7))
    Me.test_random_volumes_match_the_restatement((17, 31, 9))                     # (_check_equal: the restatement's mesh, which is not empty)
    Me.test_no_crossing_gives_none()


@case('mesh.marching_cubes', 'mesh.Mesh.components', 'mesh.Mesh.largest_component')
def case_mesh_components():
    Me = T('test_gpu_mesh')
    Me.test_components_match_shared_edge_graph(1)                                 # (asserts more than 10 components)
    Me.test_components_match_shared_edge_graph(0)


@case('mesh.sparse_marching_cubes')
def case_mesh_sparse():
    Ms = T('test_gpu_mesh_sparse')
    Ms.test_analytic_fields_equal_the_dense_mesh('three_spheres', 33)             # (the dense mesh and the restatement's, four brick sizes)
    Ms.test_analytic_fields_equal_the_dense_mesh('box', 33)
    Ms.test_analytic_fields_equal_the_dense_mesh('sphere', 3)
    Ms.test_edge_cases()                                                          # nothing to extract, a refusal, then a valid call


@case('mesh.Mesh.cut_mask')
def case_mesh_cut_mask():
    Mc = T('test_gpu_mesh_cut')
    v, f, n, c = Mc._random_mesh(0)
    removed = [Mc.maxflow_ref.max_flow(f, c, 15, smooth)[1] for smooth in (0, 2, 10)]
    assert any(r.any() and not r.all() for r in removed)                          # some faces cut, some kept
    Mc.test_random_meshes_against_the_restatement(0)
    Mc.test_boundary_and_two_components()
    Mc.test_fixture_mask_is_s_star([p for p in Mc.FIXTURES if p.endswith('smooth2.npz')][0])


@case('mesh.Mesh.trim', 'mesh.Mesh.cut_mask')
def case_mesh_trim():
    Mc = T('test_gpu_mesh_cut')
    d = np.load([p for p in Mc.FIXTURES if p.endswith('smooth2.npz')][0])
    assert d['s_star'].any() and not d['s_star'].all()
    Mc.test_trim_equals_the_host_removal()
    Mc.test_edge_cases()


@case('mesh.Mesh.simplify')
def case_mesh_simplify():
    Si = T('test_gpu_simplify')
    Si.test_host_test_shapes_match_the_restatement('sphere', 16, None, 2)
    v, f, nrm, col, h = Si.S.shape_mesh('sphere', 16)
    st = Si.S.simplify(v, f, nrm, col, 2 * h)[4]
    assert 1 < st['clusters'] < len(v) and 0 < st['faces'] < len(f)               # vertices merged, faces dropped, a mesh left
    Si.test_random_soups_at_the_chunk_sizes(2049, 1365, 1e-3)                     # (asserts duplicates and degenerate faces)
    Si.test_every_vertex_in_one_cell_gives_none()
    Si.test_target_faces(200)


# ------------------------------------------------------------------------------------------------ keypoints
@case('keypoints.scale_space')
def case_keypoints_scale_space():
    T('test_gpu_keypoints').test_scale_space_equals_the_restatement((33, 47))


@case('keypoints.detect_extrema')
def case_keypoints_extrema():
    T('test_gpu_keypoints').test_extrema_equal_the_restatement((33, 47))          # (asserts more than 20 extrema; a flat image has none)


@case('keypoints.detect')
def case_keypoints_detect():
    Kp = T('test_gpu_keypoints')
    Kp.test_detect_equals_the_restatement((33, 47), 0)                            # (asserts that the caps bite and the angles differ)
    Kp.test_detect_equals_the_restatement((33, 47), 2)


@case('keypoints.match_descriptors')
def case_keypoints_match():
    """the matcher's smallest sizes crosswise (kept and rejected matches, asserted), the split targets, the batches of several pairs, a refusal
    (a negative code) and then the smallest sizes again"""
    Kp = T('test_gpu_keypoints')

    def crosswise():
        kept = dropped = 0
        for ns in (1, 15, 16, 17):
            for nt in (1, 15, 16, 17):
                rs = np.random.RandomState(1000 * ns + nt)
                wide = rs.randint(0, 128, size=(ns + nt, 128))
                narrow = rs.randint(0, 2, size=(ns + nt, 128)) * (rs.uniform(size=(1, 128)) < 0.06)
                for name, codes in (('wide', wide), ('narrow', narrow)):
                    for mutual in (False, True):
                        want = Kp.check_match(codes, [0, ns, ns + nt], (name, ns, nt, mutual), ratio=0.95, mutual=mutual)
                        kept, dropped = kept + len(want[2]), dropped + ns - len(want[2])
        assert kept > 0 and dropped > 0
    crosswise()
    Kp.test_matcher_equals_the_restatement_at_every_size(63)
    Kp.test_matcher_splits_and_batches()
    Kp.test_matcher_refuses_negative_codes()
    crosswise()
    Kp.test_matcher_extremes_ties_and_single_targets()


@case('keypoints.verify_matches', 'keypoints.match_descriptors')
def case_keypoints_verify():
    Kp = T('test_gpu_keypoints')
    Kp.test_verify_equals_the_restatement(fixture_value('test_gpu_keypoints', 'scene'))     # (asserts that matches are rejected)
    Kp.test_verify_pure_x_translation_is_the_row_difference()                     # ends with a refusal


@case('keypoints.build_tracks')
def case_keypoints_tracks():
    Kp = T('test_gpu_keypoints')
    scene = fixture_value('test_gpu_keypoints', 'scene')
    assert 0 < len(scene['tracks'][0]) - 1 < int(scene['vo'][-1])
    Kp.test_build_tracks_cases_scene_and_random_lists(scene)                      # ends with a refusal (the round limit) ...
    Kp.assert_tracks(Kp.KP.build_tracks(scene['kp'], Kp.as_matches(scene['verified'])), scene['tracks'], 'after the refusal')


@case('keypoints.triangulate_tracks')
def case_keypoints_triangulate():
    Kp = T('test_gpu_keypoints')
    Kp.test_triangulate_cases_and_scene(fixture_value('test_gpu_keypoints', 'scene'))       # (asserts kept and dropped tracks; ends with a refusal)
    cams, xy, vo, tracks, max_reproj, _ = Kp.S.triangulation_case()
    kp = Kp.kp_of(np.zeros((len(xy), 128), int), vo, xy)
    none = (np.zeros(3, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32))   # two tracks without an observation: no launch, and still the restatement
    want = Kp.R.triangulate_tracks(xy, vo, none, Kp.KP.camera_arrays(cams), max_reproj, 1.5)
    assert want[0].shape == (2, 3) and not want[2].any()
    torch.empty(64, dtype=torch.float64, device='cuda')                            # (a dirty block of the outputs' size back in the allocator's pool)
    with launches_nothing():
        got = Kp.KP.triangulate_tracks(kp, tuple(torch.from_numpy(t) for t in none), cams, max_reproj, 1.5)
    Kp.assert_triangulation(got, want, 'no observation')
    tt = tuple(torch.from_numpy(t) for t in tracks)
    Kp.assert_triangulation(Kp.KP.triangulate_tracks(kp, tt, cams, max_reproj, 1.5), Kp.R.triangulate_tracks(xy, vo, tracks, Kp.KP.camera_arrays(cams), max_reproj, 1.5))


# ------------------------------------------------------------------------------------------------ the tracer and the native step
def _oracle():
    from oracle import oracle as O
    O.lib()
    return O


@case('ops.trace', 'ops.fold_pack', 'ops.pack_bf16_net', 'ops.pack_x3_chain')
def case_trace_edge_row():
    """row 'r17' of the edge table (17 rays: a second 16-ray tile holding one) on the bit-exact route, every tiling, staged and in one call; the
    network's folded weights and its bf16 packs are made under the context too, and a wrong pack is a wrong trace"""
    Te = T('test_gpu_trace_edges')
    Te._nets.cache_clear()                                                         # the file shares its packed networks: here they are packed anew, dirty
    try:
        want = Te._oracle_net_run('r17', 64, 'f32', True)
        assert want[1].any() and want[3].sum() > 0                                 # rays hit, and the network was evaluated
        Te._fused_vs_oracle(_oracle(), 'r17', 64, 'f32', Te.TILINGS)
        Te._fused_vs_oracle(_oracle(), 'default', 64, 'f32x3', ((2, 3),))
    finally:
        Te._nets.cache_clear()                                                     # and that file's own tests pack theirs


@case('ops.trace_generic')
def case_trace_generic_row():
    Te = T('test_gpu_trace_edges')
    Te.test_generic_route_bit_exact_vs_oracle(_oracle(), 'r17', True)
    Te.test_generic_route_bit_exact_vs_oracle(_oracle(), 'default', False)


NATIVE = ('native_step.Block.__init__', 'native_step.NativeStep.forward', 'native_step.NativeStep.bwd_block', 'native_step.direct_backward',
          'native_step.enqueue_forward', 'optim.FlatAdam.__init__', 'ops.camera_rays', 'ops.trace', 'ops.loss_prep', 'ops.loss_scale', 'ops.loss_terms',
          'ops.partition_rays', 'ops.step_outputs', 'ops.step_backward_fbar', 'ops.fold_pack_net_flat', 'ops.fold_backward_net_flat',
          'ops.pack_x3_chain', 'ops.feat_corr', 'ops.depth_carve')


@case(*NATIVE)
def case_native_step():
    """test_gpu_native_step's first configuration, with the gradient sink: the step's workspace blocks, its outputs and the optimiser's flat
    buffers all allocated dirty; the native route against the Python route (whose allocations are dirty too), bit for bit"""
    Ns = T('test_gpu_native_step')
    Ns.test_native_equals_python_route(64, 0.3, True)                             # (asserts rays that hit and rays that miss, a non-zero gradient)
    Ns.test_native_equals_python_route(64, 0.3, False)                            # without the sink: the gradients are allocations too
    Ns.test_native_phase0_with_depth_surface_samples()


# ------------------------------------------------------------------------------------------------ the remaining entry points of ops
@case('ops.feat_corr')
def case_ops_feat_corr():
    T('test_gpu_loss_edges').test_feat_corr_edges_shapes(8, 2, (7, 5))


@case('ops.depth_carve')
def case_ops_depth_carve():
    T('test_gpu_loss_edges').test_depth_carve_many_views_vs_oracle(5, False)


@case('ops.loss_terms')
def case_ops_loss_terms():
    T('test_gpu_loss_edges').test_loss_terms_vs_float64(385, 0.5)


@case('ops.det_math')
def case_ops_det_math():
    T('test_gpu_trace').test_det_math_bitwise(_oracle())


@case('ops.sphere_intersection')
def case_ops_sphere_intersection():
    T('test_gpu_loss').test_sphere_intersection_vs_reference(_oracle())           # (asserts rays that miss the sphere)


@case('ops.partition_rays')
def case_ops_partition_rays():
    St = T('test_gpu_step')
    St.test_partition_rays_matches_boolean_mask_order(3000, 0.3, True)
    St.test_partition_rays_matches_boolean_mask_order(1025, 0.0, True)


@case('ops.dsurf_samples')
def case_ops_dsurf():
    Ds = T('test_gpu_dsurf')
    Ds.test_selection_is_exact_and_points_match(*Ds.CASE_N[0])
    Ds.test_reproducible_and_seed_dependent()


@case('ops.step_outputs')
def case_ops_step_outputs(pattern):
    """The file's own check reads "never written" off the NaN its fixture fills the outputs with; here the fill is `pattern`, so beyond the valid
    prefix every byte must still be `pattern` (for 0xff: the same NaN bits)."""
    Sb = T('test_gpu_step_bookkeeping')

    def prefix(name, got, want):
        got = got.cpu().numpy()
        got = got.reshape((got.shape[0],) + want.shape[1:])
        k = want.shape[0]
        assert k <= got.shape[0], name
        assert not np.isnan(got[:k]).any(), name + ': NaN inside the valid prefix'
        assert np.array_equal(got[:k], want), name
        assert (np.ascontiguousarray(got[k:]).view(np.uint8) == pattern).all(), name + ': written beyond the valid prefix'
    saved, Sb._prefix = Sb._prefix, prefix
    try:
        Sb.test_step_outputs_every_mask_pair(300, 150, 150, 2, None)
    finally:
        Sb._prefix = saved


@case('ops.step_backward_fbar')
def case_ops_fbar():
    T('test_gpu_step_bookkeeping').test_fbar_at_grazing_angles(257)


@case('ops.fold_pack_net', 'ops.fold_pack_net_flat')
def case_ops_fold_pack_net():
    T('test_gpu_weight_packs').test_fold_pack_net(0)


@case('ops.fold_backward')
def case_ops_fold_backward():
    Df = T('test_gpu_diff_fp64')
    Df.test_fold_backward(63, 39)
    Df.test_fold_backward(5, 577)


@case('ops.sdf_col0', 'ops.fold_pack', 'ops.pack_bf16_net', 'ops.pack_x3_chain')
def case_ops_sdf_col0():
    T('test_gpu_f32x3').test_three_term_mlp_bit_exact_vs_its_oracle(_oracle(), 512, 600)


NOT_COVERED.update({
    'ops.sdf_forward': 'covered by test_gpu_diff_fp64::test_sdf_entry_points_ignore_unwritten_allocations (the same byte-level poison)',
    'ops.sdf_backward': 'covered by test_gpu_diff_fp64::test_sdf_entry_points_ignore_unwritten_allocations',
    'ops.sdf_backward_pair': 'covered by test_gpu_diff_fp64::test_sdf_entry_points_ignore_unwritten_allocations',
    'ops.sdf_backward_finish': 'covered by test_gpu_diff_fp64::test_sdf_entry_points_ignore_unwritten_allocations',
    'ops.render_forward': 'covered by test_gpu_diff_fp64::test_render_ignores_unwritten_allocations',
    'ops.render_backward': 'covered by test_gpu_diff_fp64::test_render_ignores_unwritten_allocations',
    'ops.fold_backward_net': 'covered by test_gpu_diff_fp64::test_fold_backward_net',
    'training.LaggedLog.push': 'allocates on the host only (a pinned staging buffer)',
})


# ------------------------------------------------------------------------------------------------ the test
_IDS = ['%s-0x%02x' % (name[5:], p) for name in CASE_KEYS for p in POISON_PATTERNS]


@pytest.mark.parametrize('name,pattern', [(name, p) for name in CASE_KEYS for p in POISON_PATTERNS], ids=_IDS)
def test_on_dirty_memory(name, pattern):
    run_dirty(name, pattern)
