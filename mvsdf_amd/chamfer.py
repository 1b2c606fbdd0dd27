"""DTU Chamfer evaluation on the device: the steps of DTUeval-python (the script the reference's README sends users to for the Chamfer distance),
with its random shuffle replaced by a seeded order.  Kernels: csrc/chamfer.hip (the design: DESIGN.md); tests/chamfer_ref.py restates every step
in numpy.

The metric (fp64 throughout, no FMA contraction, in the order written; mesh vertices are fp32 promoted to fp64):

1. Sampling (a Mesh only).  Per face (a, b, c) in face order: v1 = b - a, v2 = c - a, l1 = sqrt((v1x*v1x + v1y*v1y) + v1z*v1z), l2 likewise,
   area2 = the same norm of cross(v1, v2).  Faces with area2 > 0: thr = density * sqrt(l1 * l2 / area2), n1 = floor(l1 / thr),
   n2 = floor(l2 / thr); for i = 0..n1, j = 0..n2 (i outer, np.mgrid[:n1 + 1, :n2 + 1]) with s = (i + 0.5) / max(n1, 1e-7),
   t = (j + 0.5) / max(n2, 1e-7) and s + t < 1, the sample (v1*s + v2*t) + a.  P = every vertex, then the samples.  Points: P = the input.
2. Order: point i has the key splitmix64(seed ^ i) (a bijection: no ties), visited in ascending key (the script: an unseeded shuffle).
3. Downsampling: keep a point unless an already kept point lies within density, (dx*dx + dy*dy) + dz*dz <= density*density (inclusive, as
   scikit-learn's radius_neighbors).  D = the lexicographically-first maximal independent set under that order, in input order.
4. Masks: lo = bb[0] - patch, hi = bb[1] + 2*patch in fp32; D_in = the points of D with lo <= p < hi on every axis; g = rint((p - bb[0]) / res)
   (half to even, np.around); D_obs = the points of D_in with 0 <= g < obs_mask.shape and obs_mask[g].
5. S_above = the stl points with ((P0*x + P1*y) + P2*z) + P3 > 0.
6. d(q, R) = min over R of sqrt((dx*dx + dy*dy) + dz*dz), +inf where it is not < max_dist (exact).  mean_d2s = the mean of d(q, stl) over D_obs,
   mean_s2d = the mean of d(s, D_in) over S_above, each over the finite distances (NaN over none); overall = (mean_d2s + mean_s2d) / 2.
   The sums are fp64 in a fixed order: a repeated call returns the same bits.
"""
import os

import numpy as np
import torch

from ._lib import check, lib, K, MvsdfError, raise_for_bits, _header, _stream, _vp, f64_from_bits
from .mesh import Mesh, _ply_elements

U64 = 2 ** 64


# the error bits of a chamfer call (csrc/chamfer.hip), in the order they are looked at
ERRORS = [(K.MVSDF_PC_ERR_FINITE, ValueError, 'a coordinate is NaN or infinite'),
          (K.MVSDF_PC_ERR_RANGE, ValueError, 'a face refers to a missing vertex'),
          (K.MVSDF_PC_ERR_COORD, ValueError, 'a coordinate is more than 2^31 cells (of edge density) from the origin')]


def _points(x, what, name='points'):
    t = torch.as_tensor(x)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError('%s: %s must be [N, 3], got shape %s' % (what, name, tuple(t.shape)))
    if t.shape[0] == 0:
        raise ValueError('%s: %s is empty' % (what, name))
    if not t.is_cuda:
        t = t.cuda()
    return t.to(torch.float64).contiguous()


def _positive(name, x, what):
    x = float(x)
    if not (x > 0 and np.isfinite(x)):
        raise ValueError('%s: %s must be a positive finite number, got %r' % (what, name, x))
    return x


def sample_mesh(mesh, density=0.2, max_points=2 ** 31 - 1):
    """step 1: the mesh's vertices followed by its face samples, fp64 [N, 3] on the device.  More than max_points points: ValueError, before
    anything is emitted."""
    what = 'sample_mesh'
    density = _positive('density', density, what)
    if int(max_points) < 1:
        raise ValueError('%s: max_points must be >= 1' % what)
    v = torch.as_tensor(mesh.vertices)
    f = torch.as_tensor(mesh.faces)
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
        raise ValueError('%s: vertices and faces must be [N, 3]' % what)
    if v.shape[0] == 0 or f.shape[0] == 0:
        raise ValueError('%s: the mesh has no %s' % (what, 'vertices' if v.shape[0] == 0 else 'faces'))
    dev = v.device if v.is_cuda else torch.device('cuda')
    v = v.to(dev, torch.float32).contiguous()
    f = f.to(dev, torch.int32).contiguous()
    nv, nf = v.shape[0], f.shape[0]
    size = lib().mvsdf_chamfer_sample_workspace_bytes(nv, nf)
    if size == 0:
        raise ValueError('%s: %d vertices / %d faces (1 .. 2^31 - 1 each)' % (what, nv, nf))
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    st = _stream(v)
    check(lib().mvsdf_chamfer_sample_count(_vp(v), _vp(f), nv, nf, density, int(max_points), _vp(ws), size, st), 'mvsdf_chamfer_sample_count')
    total, _, err = _header(ws, K.MVSDF_CH_SAMPLE_H_WORDS)
    raise_for_bits(err, what, [(K.MVSDF_PC_ERR_POINTS, ValueError,
                                'the mesh gives more than max_points = %d points at density %g' % (int(max_points), density))] + ERRORS)
    out = torch.empty(total, 3, dtype=torch.float64, device=dev)
    check(lib().mvsdf_chamfer_sample_emit(_vp(v), _vp(f), nv, nf, density, _vp(ws), size, _vp(out), total, st), 'mvsdf_chamfer_sample_emit')
    return out


def _downsample(p, density, seed, max_rounds):
    what = 'downsample'
    density = _positive('density', density, what)
    seed = int(seed)
    if not 0 <= seed < U64:
        raise ValueError('%s: seed must be in [0, 2^64)' % what)
    n = p.shape[0]
    max_rounds = n if max_rounds is None else int(max_rounds)
    if max_rounds < 1:
        raise ValueError('%s: max_rounds must be >= 1' % what)
    size = lib().mvsdf_chamfer_downsample_workspace_bytes(n)
    if size == 0:
        raise ValueError('%s: %d points (1 .. 2^29 - 1)' % (what, n))
    ws = torch.empty(size, dtype=torch.uint8, device=p.device)
    kept = torch.empty(n, dtype=torch.uint8, device=p.device)
    check(lib().mvsdf_chamfer_downsample(_vp(p), n, density, seed, max_rounds, _vp(ws), size, _vp(kept), _stream(p)), 'mvsdf_chamfer_downsample')
    n_kept, rounds, err = _header(ws, K.MVSDF_CH_DOWN_H_WORDS)
    raise_for_bits(err, what, [(K.MVSDF_PC_ERR_ROUNDS, MvsdfError, 'not decided after %d rounds (the limit)' % rounds)] + ERRORS)
    return kept, n_kept, rounds


def downsample(points, density=0.2, seed=0, max_rounds=None):
    """steps 2-3: the greedy radius filter in the order of the keys splitmix64(seed ^ i) -> kept bool [N] on the device.  max_rounds (default N,
    which always suffices) bounds the parallel rounds: reaching it raises MvsdfError."""
    p = _points(points, 'downsample')
    return _downsample(p, density, seed, max_rounds)[0].bool()


def _nearest(q, r, max_dist):
    what = 'nearest_distance'
    nq, nr = q.shape[0], r.shape[0]
    size = lib().mvsdf_chamfer_nearest_workspace_bytes(nq, nr)
    if size == 0:
        raise ValueError('%s: %d queries / %d references (at most 2^31 - 1 references)' % (what, nq, nr))
    ws = torch.empty(size, dtype=torch.uint8, device=r.device)
    dist = torch.empty(nq, dtype=torch.float64, device=r.device)
    check(lib().mvsdf_chamfer_nearest(_vp(q), nq, _vp(r), nr, float(max_dist), _vp(ws), size, _vp(dist), _stream(r)), 'mvsdf_chamfer_nearest')
    used, total, err = _header(ws, K.MVSDF_CH_NEAR_H_WORDS)
    raise_for_bits(err, what, ERRORS)
    return dist, used, f64_from_bits(total)


def nearest_distance(queries, refs, max_dist=20.0):
    """step 6's d(q, refs) for every query: fp64 [Q] on the device, exact, +inf where the nearest reference is not closer than max_dist."""
    what = 'nearest_distance'
    q = _points(queries, what, 'queries')
    r = _points(refs, what, 'refs')
    dist, _, _ = _nearest(q, r, _positive('max_dist', max_dist, what))
    return dist


def _mean(total, used):
    return total / used if used else float('nan')


def _masks(pts, kept, s, obs_mask, bb, res, plane, patch, what):
    dev = pts.device
    obs = torch.as_tensor(obs_mask)
    if obs.dim() != 3 or obs.numel() == 0:
        raise ValueError('%s: obs_mask must be a non-empty 3-d volume, got shape %s' % (what, tuple(obs.shape)))
    obs = obs.to(dev).bool().to(torch.uint8).contiguous()
    bb = np.asarray(bb, dtype=np.float32).reshape(2, 3)
    pl = np.asarray(plane, dtype=np.float64).reshape(4)
    res = _positive('res', res, what)
    if not (np.isfinite(bb).all() and np.isfinite(pl).all() and np.isfinite(float(patch))):
        raise ValueError('%s: bb, plane and patch must be finite' % what)
    n, m = pts.shape[0], s.shape[0]
    box = np.concatenate([bb[0] - np.float32(patch), bb[1] + np.float32(patch * 2), bb[0]]).astype(np.float32)   # fp32, as the script's BB
    shape = np.array(obs.shape, dtype=np.int64)
    size = lib().mvsdf_chamfer_mask_workspace_bytes(n, m)
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    d_in = torch.empty(n, 3, dtype=torch.float64, device=dev)
    d_obs = torch.empty(n, 3, dtype=torch.float64, device=dev)
    s_above = torch.empty(m, 3, dtype=torch.float64, device=dev)
    check(lib().mvsdf_chamfer_mask(_vp(pts), _vp(kept), n, _vp(s), m, box.ctypes.data, res, _vp(obs), shape.ctypes.data, pl.ctypes.data, _vp(ws), size,
                                   _vp(d_in), _vp(d_obs), _vp(s_above), _stream(pts)), 'mvsdf_chamfer_mask')
    n_in, n_obs, n_above, err = _header(ws, K.MVSDF_CH_MASK_H_WORDS)
    raise_for_bits(err, what, ERRORS)
    return d_in[:n_in], d_obs[:n_obs], s_above[:n_above]


def masks(points, kept, stl, obs_mask, bb, res, plane, patch=60):
    """steps 4-5: (D_in, D_obs, S_above), fp64 device tensors in input order; kept: bool [N] over points (downsample's mask)"""
    what = 'masks'
    p = _points(points, what)
    k = torch.as_tensor(kept)
    if k.shape != (p.shape[0],):
        raise ValueError('%s: kept must be [N] for N points' % what)
    return _masks(p, k.to(p.device).bool().to(torch.uint8).contiguous(), _points(stl, what, 'stl').to(p.device), obs_mask, bb, res, plane, patch, what)


def dtu_chamfer(geometry, stl, obs_mask, bb, res, plane, density=0.2, patch=60, max_dist=20.0, seed=0, return_distances=False):
    """The DTU Chamfer numbers of a Mesh (mode 'mesh') or of points [N, 3] (mode 'pcd') against the ground-truth points stl [M, 3], with DTU's
    observation mask obs_mask (bool [X, Y, Z]), its box bb ([2, 3], used as fp32), grid step res and ground plane ([4]) -> dict with mean_d2s,
    mean_s2d, overall and the counts n_points, n_down, n_in, n_obs, n_stl_above, n_d2s_used, n_s2d_used (and rounds, the downsampling's parallel
    rounds); with return_distances also dist_d2s [n_obs] and dist_s2d [n_stl_above] (fp64 device tensors, +inf beyond max_dist)."""
    what = 'dtu_chamfer'
    density = _positive('density', density, what)
    max_dist = _positive('max_dist', max_dist, what)
    _positive('res', res, what)
    if isinstance(geometry, Mesh):
        pts = sample_mesh(geometry, density)
    else:
        pts = _points(geometry, what, 'points')
    dev = pts.device
    s = _points(stl, what, 'stl').to(dev)
    kept, n_down, rounds = _downsample(pts, density, seed, None)
    d_in, d_obs, s_above = _masks(pts, kept, s, obs_mask, bb, res, plane, patch, what)
    if len(d_obs):
        dist_d2s, used_d2s, sum_d2s = _nearest(d_obs, s, max_dist)
    else:
        dist_d2s, used_d2s, sum_d2s = torch.empty(0, dtype=torch.float64, device=dev), 0, 0.0
    if len(s_above) and len(d_in):
        dist_s2d, used_s2d, sum_s2d = _nearest(s_above, d_in, max_dist)
    else:
        dist_s2d, used_s2d, sum_s2d = torch.full((len(s_above),), float('inf'), dtype=torch.float64, device=dev), 0, 0.0
    mean_d2s, mean_s2d = _mean(sum_d2s, used_d2s), _mean(sum_s2d, used_s2d)
    out = {'mean_d2s': mean_d2s, 'mean_s2d': mean_s2d, 'overall': (mean_d2s + mean_s2d) / 2,
           'n_points': pts.shape[0], 'n_down': n_down, 'n_in': len(d_in), 'n_obs': len(d_obs), 'n_stl_above': len(s_above),
           'n_d2s_used': used_d2s, 'n_s2d_used': used_s2d, 'rounds': rounds}
    if return_distances:
        out['dist_d2s'] = dist_d2s
        out['dist_s2d'] = dist_s2d
    return out


def load_dtu_obs(dataset_dir, scan):
    """DTU's observation mask and ground plane of one scan: <dataset_dir>/ObsMask/ObsMask{scan}_10.mat (ObsMask, BB, Res) and Plane{scan}.mat (P)
    -> (obs_mask bool [X, Y, Z], bb fp32 [2, 3], res float, plane fp64 [4]), the trailing arguments of dtu_chamfer.  Needs scipy."""
    try:
        import scipy.io as sio
    except ImportError as e:
        raise ImportError('load_dtu_obs reads MATLAB files with scipy.io.loadmat; scipy is not installed') from e
    obs = sio.loadmat(os.path.join(dataset_dir, 'ObsMask', 'ObsMask{}_10.mat'.format(scan)))
    pl = sio.loadmat(os.path.join(dataset_dir, 'ObsMask', 'Plane{}.mat'.format(scan)))
    return (np.asarray(obs['ObsMask']).astype(bool), np.asarray(obs['BB']).astype(np.float32).reshape(2, 3),
            float(np.asarray(obs['Res'], dtype=np.float64).reshape(-1)[0]), np.asarray(pl['P'], dtype=np.float64).reshape(4))


def load_points(path):
    """the x / y / z of a binary little-endian point-cloud PLY (such as DTU's Points/stl/stl{scan:03}_total.ply; any vertex properties, float or
    double coordinates) -> fp64 numpy [N, 3]"""
    arrays = _ply_elements(path, 'load_points')
    vert = arrays.get('vertex')
    if vert is None or not all(k in vert.dtype.names for k in 'xyz'):
        raise ValueError('load_points: %s has no vertex x / y / z' % path)
    return np.stack([vert[k].astype(np.float64) for k in 'xyz'], 1)


def load_oriented_points(path):
    """load_points and the file's normals -> (points fp64 numpy [N, 3], normals fp64 numpy [N, 3] or None when the vertices carry no nx / ny / nz)"""
    arrays = _ply_elements(path, 'load_oriented_points')
    vert = arrays.get('vertex')
    if vert is None or not all(k in vert.dtype.names for k in 'xyz'):
        raise ValueError('load_oriented_points: %s has no vertex x / y / z' % path)
    pts = np.stack([vert[k].astype(np.float64) for k in 'xyz'], 1)
    if not all(k in vert.dtype.names for k in ('nx', 'ny', 'nz')):
        return pts, None
    return pts, np.stack([vert[k].astype(np.float64) for k in ('nx', 'ny', 'nz')], 1)
