"""The tracer's edge-case table (numpy on the CPU, no GPU): rays, masks, tracer parameters and geometry at the sizes where the launch shapes and the
list logic of csrc/trace.hip change.  tests/test_trace_cases_host.py runs every row through the C oracle and holds it to what it declares here;
tests/test_gpu_trace_edges.py runs the same rows through both routes of the HIP tracer, bit for bit against that oracle.

A row is built like tests/test_gpu_trace.py::test_trace_fuzz_bit_exact_vs_oracle builds its scenes: synth.make_batch(..., with_features=False), the oracle's
camera_rays, np.random.RandomState(seed) for the object mask (uniform < p) and then the n_steps min-sdf draws, torch.linspace(0, 1, n_steps) for the intervals
(one row excepted: `_wrap`).

`lists` declares, for TRAINING mode with the analytic SDF (helpers.analytic_sdf), which work lists the row is there to populate (True), to leave empty (False) or
does not care about (None): (sampler, secant, min-sdf).  `fused` declares the same for the W = 64 network (synth.make_state_dict(64, 0), fp32 arithmetic) on the
rows the fused-route tests use; `WIDE` declares it for the W = 256 and the W = 512 network (synth.make_state_dict(W, 0), fp32 arithmetic) on the rows the
fused-route tests run at those widths.  The comment behind each row records the oracle's counts when the row was written:
    isect / sampler / secant / min-sdf rays   (sampler = rows[1] / n_steps, secant = rows[2] / n_secant_steps, min-sdf = rows[3] / n_steps)
-- a record for the reader; the tests assert the declarations, not these numbers."""
import functools
from collections import namedtuple

import numpy as np

from mvsdf_amd.utils import synth

Row = namedtuple('Row', 'B P seed radius height focal r n_steps st_iters line_iters n_secant dist_clip p lists fused')
Case = namedtuple('Case', 'name cam_loc ray_dirs object_mask minsdf_steps intervals params lists fused')

Y, N, _ = True, False, None
SDF_THRESHOLD, LINE_SEARCH_STEP = 5.0e-5, 0.5                       # mvsdf_dtu.conf; no row varies them

#                 B    P  seed radius height focal   r    n   st  ls sec  clip    p    lists (analytic)  fused (W = 64)
ROWS = {
    # ---- the rows of the issue                                                                                         analytic | W = 64 (training)
    'default':      Row(2, 300, 1, 2.5, 0.8, 1.4, 1.0, 100, 10, 3, 8, 0.5, 0.7, (Y, Y, Y), (Y, Y, Y)),                 # 591 / 98 / 66 / 346 | 591 / 113 / 65 / 169
    'inside':       Row(2, 300, 2, 0.5, 0.1, 0.6, 1.0, 37, 3, 1, 3, 0.5, 0.7, (N, N, Y), (N, N, Y)),                   # 600 / 0 / 0 / 167 | 600 / 0 / 0 / 167  (camera inside the sphere: t0 clamps to 0)
    'r08':          Row(3, 171, 3, 2.0, 0.5, 1.0, 0.8, 9, 1, 0, 3, 0.5, 1.1, (Y, Y, Y), (Y, Y, Y)),                    # 370 / 103 / 36 / 99 | 370 / 87 / 67 / 4  (mv_sphere_isect's r * r, no line search)
    'r2':           Row(1, 1025, 4, 3.0, 1.0, 1.0, 2.0, 129, 10, 3, 8, 0.5, 0.6, (Y, Y, Y), None),                     # 1025 / 10 / 7 / 664 | -
    'render':       Row(2, 513, 5, 2.5, 0.8, 2.2, 1.0, 200, 40, 3, 8, 0.05, 1.1, (Y, Y, Y), (N, N, N)),                # 1026 / 8 / 7 / 54 | 1026 / 0 / 0 / 0  (the IDR_RENDER variant: dist_clip 0.05, 40 iterations)
    'n2':           Row(1, 65, 6, 2.5, 0.8, 1.4, 1.0, 2, 10, 3, 8, 0.5, 0.7, (Y, N, Y), (Y, Y, Y)),                    # 64 / 11 / 0 / 43 | 64 / 22 / 7 / 20
    'n512':         Row(1, 63, 7, 2.5, 0.8, 1.4, 1.0, 512, 2, 5, 0, 0.5, 0.7, (Y, _, Y), None),                        # 62 / 42 / (0 steps) / 20 | -  (no secant steps)
    'one':          Row(1, 1, 8, 2.5, 0.8, 1.4, 1.0, 16, 10, 3, 8, 0.5, 1.1, (N, N, N), (Y, Y, N)),                    # 1 / 0 / 0 / 0 | 1 / 1 / 1 / 0
    'one_s':        Row(1, 1, 100, 2.5, 0.8, 1.4, 1.0, 16, 10, 3, 8, 0.5, 1.1, None, (Y, Y, N)),                       # - | 1 / 1 / 1 / 0  ('one' with another seed: sampled on the bf16-rounded weights too, ROUNDED_EMPTY)
    'st0':          Row(1, 200, 9, 2.5, 0.8, 1.4, 1.0, 16, 0, 3, 8, 0.5, 0.7, (Y, Y, N), (Y, Y, N)),                   # 196 / 196 / 55 / 0 | 196 / 196 / 114 / 0  (no sphere tracing: every intersecting ray is sampled)
    # ---- the sampler's window (12 samples first, then the rest) and the 64-lane steps of the per-ray scans
    'n12':          Row(1, 301, 12, 2.5, 0.8, 1.4, 1.0, 12, 3, 1, 3, 0.5, 0.7, (Y, Y, Y), (Y, Y, Y)),                  # 298 / 102 / 55 / 149 | 298 / 275 / 181 / 18  (single pass)
    'n13':          Row(1, 301, 13, 2.5, 0.8, 1.4, 1.0, 13, 3, 1, 3, 0.5, 0.7, (Y, Y, Y), (Y, Y, Y)),                  # 296 / 97 / 60 / 162 | 296 / 272 / 172 / 18  (a rest segment of one sample)
    'n64':          Row(1, 301, 64, 2.5, 0.8, 1.4, 1.0, 64, 3, 1, 3, 0.5, 0.7, (Y, Y, Y), (Y, Y, Y)),                  # 300 / 93 / 53 / 170 | 300 / 282 / 182 / 12
    'n65':          Row(1, 301, 65, 2.5, 0.8, 1.4, 1.0, 65, 3, 1, 3, 0.5, 0.7, (Y, Y, Y), (Y, Y, Y)),                  # 297 / 98 / 67 / 146 | 297 / 278 / 194 / 15
    'n129':         Row(1, 65, 129, 2.5, 0.8, 1.4, 1.0, 129, 3, 1, 3, 0.5, 0.7, (Y, Y, Y), (Y, Y, Y)),                 # 63 / 26 / 13 / 27 | 63 / 58 / 39 / 3  (past the 128 samples mvsdf_trace_workspace_bytes assumes)
    'n1024':        Row(1, 20, 1024, 2.5, 0.8, 1.4, 1.0, 1024, 2, 1, 3, 0.5, 0.7, (Y, Y, Y), (Y, Y, N)),               # 20 / 12 / 4 / 5 | 20 / 20 / 12 / 0  (the largest n_steps the kernels accept)
    # ---- an all-false object mask: in training every intersecting ray the sampler does not take goes on the min-sdf list, no secant
    'om_none':      Row(2, 150, 21, 2.5, 0.8, 1.4, 1.0, 16, 10, 3, 8, 0.5, -1.0, (Y, N, Y), (Y, N, Y)),                # 298 / 44 / 0 / 254 | 298 / 57 / 0 / 241
    # ---- ray counts around a wave, 8 * mt rays per sphere-tracing workgroup, 16 rays per reduction workgroup, the 1024-ray chunks of the generic route's
    #      compaction kernels and one workgroup per compute unit (2048 * mt rays: tail filling on / off)
    'r7':           Row(1, 7, 31, 2.5, 0.8, 1.4, 1.0, 16, 3, 1, 3, 0.5, 0.7, (_, _, _), (_, _, _)),                    # 7 / 0 / 0 / 6 | 7 / 7 / 2 / 0
    'r8':           Row(1, 8, 32, 2.5, 0.8, 1.4, 1.0, 16, 3, 1, 3, 0.5, 0.7, (_, _, _), (_, _, _)),                    # 8 / 2 / 1 / 5 | 8 / 8 / 2 / 0
    'r9':           Row(1, 9, 33, 2.5, 0.8, 1.4, 1.0, 16, 3, 1, 3, 0.5, 0.7, (_, _, _), (_, _, _)),                    # 9 / 5 / 3 / 2 | 9 / 8 / 5 / 0
    'r15':          Row(1, 15, 34, 2.5, 0.8, 1.4, 1.0, 16, 3, 1, 3, 0.5, 0.7, (_, _, _), (_, _, _)),                   # 15 / 6 / 1 / 9 | 15 / 13 / 10 / 2
    'r16':          Row(1, 16, 35, 2.5, 0.8, 1.4, 1.0, 16, 3, 1, 3, 0.5, 0.7, (_, _, _), (_, _, _)),                   # 15 / 5 / 4 / 8 | 15 / 14 / 9 / 1
    'r17':          Row(1, 17, 36, 2.5, 0.8, 1.4, 1.0, 16, 3, 1, 3, 0.5, 0.7, (_, _, _), (_, _, _)),                   # 17 / 6 / 3 / 10 | 17 / 17 / 10 / 0
    'r31':          Row(1, 31, 37, 2.5, 0.8, 1.4, 1.0, 16, 3, 1, 3, 0.5, 0.7, (_, _, _), (_, _, _)),                   # 31 / 8 / 5 / 19 | 31 / 24 / 14 / 6
    'r33':          Row(1, 33, 38, 2.5, 0.8, 1.4, 1.0, 16, 3, 1, 3, 0.5, 0.7, (_, _, _), (_, _, _)),                   # 33 / 12 / 9 / 21 | 33 / 32 / 16 / 0
    'r1023':        Row(1, 1023, 39, 2.5, 0.8, 1.4, 1.0, 16, 3, 1, 3, 0.5, 0.7, (Y, Y, Y), None),                      # 1013 / 374 / 207 / 516 | -
    'r1024':        Row(1, 1024, 40, 2.5, 0.8, 1.4, 1.0, 16, 3, 1, 3, 0.5, 0.7, (Y, Y, Y), None),                      # 1010 / 363 / 187 / 525 | -
    'r2048':        Row(1, 2048, 41, 2.5, 0.8, 1.4, 1.0, 16, 3, 1, 3, 0.5, 0.7, (Y, Y, Y), (Y, Y, Y)),                 # 2020 / 730 / 394 / 1030 | 2020 / 1856 / 1167 / 130
    'r2049':        Row(1, 2049, 42, 2.5, 0.8, 1.4, 1.0, 16, 3, 1, 3, 0.5, 0.7, (Y, Y, Y), (Y, Y, Y)),                 # 2012 / 721 / 386 / 1016 | 2012 / 1875 / 1184 / 110
    'r4096':        Row(2, 2048, 43, 2.5, 0.8, 1.4, 1.0, 16, 3, 1, 3, 0.5, 0.7, None, (Y, Y, Y)),                      # - | 4053 / 2076 / 1230 / 701
    'r4097':        Row(1, 4097, 44, 2.5, 0.8, 1.4, 1.0, 16, 3, 1, 3, 0.5, 0.7, None, (Y, Y, Y)),                      # - | 4040 / 3708 / 2279 / 267
    'r8192':        Row(4, 2048, 45, 2.5, 0.8, 1.4, 1.0, 16, 3, 1, 3, 0.5, 0.7, None, (Y, Y, Y)),                      # - | 8091 / 4788 / 2856 / 1377
    'r8193':        Row(1, 8193, 46, 2.5, 0.8, 1.4, 1.0, 16, 3, 1, 3, 0.5, 0.7, None, (Y, Y, Y)),                      # - | 8077 / 7488 / 4728 / 481
    # ---- lists longer than one 1024-ray chunk, with entries on both sides of the chunk border
    'st0_2049':     Row(1, 2049, 51, 2.5, 0.8, 1.4, 1.0, 16, 0, 3, 8, 0.5, 0.7, (Y, Y, N), None),                      # 2027 / 2027 / 663 / 0 | -  (sampler list > 1024)
    'om_none_2049': Row(1, 2049, 52, 2.5, 0.8, 1.4, 1.0, 16, 10, 3, 8, 0.5, -1.0, (Y, N, Y), None),                    # 2024 / 320 / 0 / 1704 | -  (min-sdf list > 1024)
    # ---- four cameras, an odd number of rays each (gid / P picks the camera)
    'b4':           Row(4, 77, 61, 2.2, -0.3, 1.1, 1.0, 37, 3, 1, 3, 0.5, 0.6, (Y, Y, Y), (Y, Y, Y)),                  # 300 / 135 / 70 / 161 | 300 / 169 / 97 / 65
}
# ---- the wider networks: (sampler, secant, min-sdf) of synth.make_state_dict(W, 0) on fp32 arithmetic, training, per width -- the same row does different things at
#      different widths ('inside': the W = 512 network is negative at the camera, the W = 256 one is not).  Y: at least 3 rays, N: none, _: one or two rays (the engines on
#      bf16-rounded weights, whose lists tests/test_gpu_trace_edges.py holds to these declarations, move a count by a ray or two) and the rows that are there for their
#      ray COUNT (r7 ... r33, as in `fused`).  Recorded counts: sampler / secant / min-sdf rays.
#                   W = 256    W = 512
WIDE = {
    'one':      ((_, N, N), (_, _, N)),                             # 1 / 0 / 0 | 1 / 1 / 0
    'r7':       ((_, _, _), (_, _, _)),                             # 1 / 0 / 5 | 3 / 1 / 4
    'r8':       ((_, _, _), (_, _, _)),                             # 5 / 2 / 3 | 5 / 2 / 3
    'r9':       ((_, _, _), (_, _, _)),                             # 7 / 4 / 2 | 8 / 5 / 1
    'r15':      ((_, _, _), (_, _, _)),                             # 7 / 0 / 8 | 14 / 3 / 1
    'r16':      ((_, _, _), (_, _, _)),                             # 9 / 3 / 6 | 11 / 6 / 4
    'r17':      ((_, _, _), (_, _, _)),                             # 3 / 1 / 14 | 12 / 2 / 5
    'r31':      ((_, _, _), (_, _, _)),                             # 12 / 5 / 19 | 17 / 10 / 14
    'r33':      ((_, _, _), (_, _, _)),                             # 14 / 2 / 19 | 24 / 9 / 9
    'n2':       ((Y, N, Y), (Y, N, Y)),                             # 9 / 0 / 46 | 22 / 0 / 37
    'n12':      ((Y, Y, Y), (Y, Y, Y)),                             # 145 / 66 / 148 | 231 / 104 / 67
    'n13':      ((Y, Y, Y), (Y, Y, Y)),                             # 140 / 67 / 154 | 226 / 94 / 70
    'n64':      ((Y, Y, Y), (Y, Y, Y)),                             # 133 / 63 / 167 | 222 / 92 / 78
    'n65':      ((Y, Y, Y), (Y, Y, Y)),                             # 143 / 74 / 149 | 228 / 110 / 69
    'n129':     ((Y, Y, Y), (Y, Y, Y)),                             # 35 / 14 / 28 | 48 / 23 / 15
    'st0':      ((Y, Y, N), (Y, Y, N)),                             # 196 / 36 / 0 | 196 / 54 / 0
    'wrap':     ((Y, Y, N), (Y, Y, N)),                             # 196 / 37 / 0 | 196 / 55 / 0
    'om_none':  ((Y, N, Y), (Y, N, Y)),                             # 41 / 0 / 257 | 115 / 0 / 183
    'b4':       ((Y, Y, Y), (Y, Y, Y)),                             # 136 / 52 / 163 | 214 / 74 / 86
    'inside':   ((Y, Y, Y), (N, N, Y)),                             # 227 / 164 / 104 | 0 / 0 / 167
    'r08':      ((Y, Y, Y), (Y, Y, Y)),                             # 320 / 138 / 50 | 357 / 192 / 13
    'miss7':    ((N, N, N), (N, N, N)),                             # 0 / 0 / 0 | 0 / 0 / 0
}
WIDE_WIDTHS = (256, 512)
# (W, row): the lists the row declares filled are EMPTY on the bf16-rounded weights (oracle.Net(sd, bf16='weights'), the arithmetic the 'bf16x2' / 'bf16x3' engines
# follow up to the order of their fp32 additions): the one ray of 'one' converges in sphere tracing there.  'one_s' is the row that keeps a single sampled ray.
ROUNDED_EMPTY = {(64, 'one')}
LONG_LISTS = {'st0_2049': 'sampler', 'om_none_2049': 'minsdf'}      # rows whose named list must hold more than 1024 rays (analytic SDF, training)
WRAP = 'wrap'                                                        # intervals that start inside the object: the first sign change at sample 0
ALL_MISS = 'miss7'                                                   # every ray misses the sphere: the -(d . c) projection in training, no evaluation at all

ANALYTIC = tuple(k for k, v in ROWS.items() if v.lists is not None) + (ALL_MISS, WRAP)
FUSED = tuple(k for k, v in ROWS.items() if v.fused is not None) + (ALL_MISS, WRAP)
NAMES = tuple(ROWS) + (ALL_MISS, WRAP)


def declared(name, W):
    """the (sampler, secant, min-sdf) declaration of a row for the width-W network on fp32 arithmetic, or None where the table declares nothing"""
    if W == 64:
        return case(name).fused
    return WIDE[name][WIDE_WIDTHS.index(W)] if name in WIDE else None


def _intervals(n):
    import torch                                                     # CPU values, like the reference (ray_tracing.py:206)
    return torch.linspace(0, 1, steps=n).numpy()


def _params(r, n_steps, st_iters, line_iters, n_secant, dist_clip):
    return dict(object_bounding_sphere=r, sdf_threshold=SDF_THRESHOLD, line_search_step=LINE_SEARCH_STEP, line_step_iters=line_iters,
                sphere_tracing_iters=st_iters, n_steps=n_steps, n_secant_steps=n_secant, dist_clip=dist_clip)


def _from_row(name):
    from oracle import oracle as O
    w = ROWS[name]
    rs = np.random.RandomState(w.seed)
    inp, _gt = synth.make_batch(w.B, w.P, 0, seed=w.seed, radius=w.radius, height=w.height, focal_scale=w.focal, with_features=False)
    dirs, cam = O.camera_rays(inp['uv'], inp['pose'], inp['intrinsics'])
    om = rs.uniform(size=w.B * w.P) < w.p
    steps = rs.uniform(size=w.n_steps).astype(np.float32)
    return Case(name, cam, dirs, om, steps, _intervals(w.n_steps), _params(w.r, w.n_steps, w.st_iters, w.line_iters, w.n_secant, w.dist_clip),
                w.lists, w.fused)


def _miss7():
    """The rig of tests/test_gpu_shapes.py::test_empty_and_ragged_inputs -- a camera at (0, 0, 5) looking along +x: all 7 rays miss the unit sphere -- with the
    rays after the first tilted a little, so that -(d . c) is not zero on them.            0 / 0 / 0 / 0"""
    rs = np.random.RandomState(7)
    d = np.array([[1.0, 0.1 * i, 0.05 * i] for i in range(7)])
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    cam = np.array([[0.0, 0.0, 5.0]], np.float32)
    om = rs.uniform(size=7) < 0.6                                    # both the in-mask and the out-mask projection
    steps = rs.uniform(size=16).astype(np.float32)
    return Case(ALL_MISS, cam, d[None], om, steps, _intervals(16), _params(1.0, 16, 10, 3, 8, 0.5), (N, N, N), (N, N, N))


def _wrap():
    """The one row whose intervals are NOT torch.linspace(0, 1, n).  With intervals that start at 0 the sampler's sample 0 repeats the last evaluation of sphere
    tracing, which was above the threshold or the ray would not be sampled: the first negative sample is never sample 0, and the negative index of
    ray_tracing.py:248-249 (`sampler_pts_ind[secant_pts] - 1` = -1: the LAST sample) is out of reach of any pure `sdf`.  The kernels and the oracle restate that wrap, and the
    C ABI takes the intervals from its caller: here they run from 0.4 to 1 over the chord of the 'st0' rig (no sphere tracing), so the first sample of the
    central rays lies inside the object and their secant starts from the bracket (sample n - 1, sample 0).            196 / 196 / 55 / 0 | 196 / 196 / 114 / 0"""
    c = _from_row('st0')
    iv = (np.float32(0.4) + np.float32(0.6) * c.intervals).astype(np.float32)
    return c._replace(name=WRAP, intervals=iv, lists=(Y, Y, N), fused=(Y, Y, N))


@functools.lru_cache(maxsize=None)
def case(name):
    """-> Case(name, cam_loc [B,3], ray_dirs [B,P,3], object_mask [R] bool, minsdf_steps [n], intervals [n], params (the keywords of oracle.trace), lists, fused).
    Cached: the arrays are shared between tests and must not be written to."""
    c = _miss7() if name == ALL_MISS else (_wrap() if name == WRAP else _from_row(name))
    for a in c[1:6]:
        a.setflags(write=False)
    return c


CASES = {k: functools.partial(case, k) for k in NAMES}              # one function per case


def params_tuple(params):
    """The tracer-parameter tuple of ops.trace / ops.trace_generic (the fields of MvsdfTraceParams, in order)."""
    return (params['object_bounding_sphere'], params['sdf_threshold'], params['line_search_step'], params['line_step_iters'],
            params['sphere_tracing_iters'], params['n_steps'], params['n_secant_steps'], params['dist_clip'])


def list_counts(rows, params):
    """(sampler, secant, min-sdf) ray counts from the oracle's rows.  n_secant_steps == 0: the secant count cannot be read from rows -> None."""
    n, ns = params['n_steps'], params['n_secant_steps']
    assert rows[1] % n == 0 and rows[3] % n == 0 and (ns == 0 or rows[2] % ns == 0)
    return int(rows[1]) // n, (int(rows[2]) // ns if ns else None), int(rows[3]) // n


@functools.lru_cache(maxsize=None)
def oracle_analytic(name, training):
    """(points, mask, dists, rows) of the C oracle with the analytic SDF.  Computed once per process and shared: read-only."""
    from oracle import oracle as O
    c = case(name)
    out = O.trace(None, c.cam_loc, c.ray_dirs, c.object_mask, training, c.minsdf_steps, c.intervals, analytic=True, **c.params)
    for a in out:
        a.setflags(write=False)
    return out
