"""fuse_depths (csrc/fusion.hip) against the numpy restatement tests/fusion_ref.py, bit for bit, and its argument errors."""
import numpy as np
import pytest
import torch

import fusion_ref as R
import mvs_scene as S
from mvsdf_amd import fusion

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32 if a.dtype in (np.float32, np.int32) else np.uint8)


def _check(cams, depths, pairs, want_points=None, **kw):
    """fuse_depths == fusion_ref.fuse in every output, bit for bit, twice in a row; -> the Fused"""
    ref = R.fuse(cams, depths, pairs, **kw)
    out = None
    for _ in range(2):
        f = fusion.fuse_depths(cams, depths, pairs, **kw)
        n = len(ref['points'])
        assert len(f) == n and f.points.shape == (n, 3) and f.points.dtype == torch.float64 and f.points.is_cuda
        assert f.view.dtype == torch.int32 and f.pixel.dtype == torch.int32 and f.counts.dtype == torch.int32
        assert f.masked_depths.dtype == torch.float32 and f.fused_depths.dtype == torch.float32
        for name in ('points', 'view', 'pixel', 'masked_depths', 'fused_depths', 'counts'):
            got = getattr(f, name).cpu().numpy()
            assert got.shape == ref[name].shape and np.array_equal(_bits(got), _bits(ref[name])), name
        if kw.get('images') is not None:
            assert f.colors.dtype == torch.uint8 and np.array_equal(f.colors.cpu().numpy(), ref['colors'])
        else:
            assert f.colors is None
        lo, hi = f.bbox()
        if n:
            assert np.array_equal(_bits(lo.cpu().numpy()), _bits(ref['lo'])) and np.array_equal(_bits(hi.cpu().numpy()), _bits(ref['hi']))
        else:
            assert bool(torch.isnan(lo).all()) and bool(torch.isnan(hi).all())
        out = f
    if want_points is not None:
        assert want_points(len(out)), len(out)
    return out


@pytest.mark.parametrize('hw', [(20, 28), (37, 53), (75, 100)])
@pytest.mark.parametrize('clean', [True, False])
def test_equals_the_restatement(hw, clean):
    cams, depths, pairs = S.make_views(6, hw, clean=clean)
    images = np.random.RandomState(1).randint(0, 256, (6,) + hw + (3,)).astype(np.uint8)
    _check(cams, depths, pairs, images=images, want_points=lambda n: n > 50)
    _check(cams, depths, pairs, want_points=lambda n: n > 50)


def test_holes_and_probabilities():
    cams, depths, pairs = S.make_views(6, (37, 53), clean=True, hole_frac=0.3)
    _check(cams, depths, pairs, want_points=lambda n: n > 0)
    cams, depths, pairs = S.make_views(6, (37, 53), clean=True)
    probs = S.make_probs(depths, cut=1.0 / 3)
    f = _check(cams, depths, pairs, probs=probs, want_points=lambda n: n > 0)
    cut = 1 - float((f.masked_depths > 0).sum()) / (depths > 0).sum()
    assert 0.25 < cut < 0.42                                                    # a third of the pixels, give or take
    _check(cams, depths, pairs, probs=probs, pthresh=(0.9, 0.0, 0.95), vthresh=1)


def test_pair_lists():
    cams, depths, pairs = S.make_views(6, (20, 28), clean=True)
    some = [list(p) for p in pairs]
    some[2] = []                                                                # a view without sources keeps nothing (vthresh = 2) ...
    f = _check(cams, depths, some)
    assert int((f.view == 2).sum()) == 0 and int(f.counts[2].abs().sum()) == 0
    f = _check(cams, depths, some, vthresh=0)                                   # ... and everything it has at vthresh = 0
    assert int((f.view == 2).sum()) == int((depths[2] > 0).sum())
    _check(cams, depths, pairs, view=3)                                         # a pair list longer than view
    _check(cams, depths, pairs, view=1, vthresh=1)
    _check(cams, depths, [p + p for p in pairs], view=7, vthresh=6)             # a source may be listed twice: it counts twice
    f = _check(cams, depths, pairs, vthresh=6)                                  # more than the five sources: N = 0
    assert len(f) == 0 and f.points.shape == (0, 3) and bool(torch.isnan(f.bbox()[0]).all()) and int(f.fused_depths.abs().sum()) == 0
    f = _check(cams, depths, [[] for _ in pairs])
    assert len(f) == 0


def test_points_behind_and_outside_a_source():
    """source camera 1 sits between the sphere and the other cameras looking away from it (the reference points are behind it: p2 <= 0); source
    camera 2 is turned sideways (they fall outside its image)"""
    cams, depths, pairs = S.make_views(6, (37, 53), clean=True)
    c0 = -cams[0, 0, :3, :3].T @ cams[0, 0, :3, 3]                              # camera 0's centre
    behind = cams[0].copy()
    behind[0, :3, 3] = -behind[0, :3, :3] @ (S.CENTER + 0.3 * (S.CENTER - c0))     # beyond the sphere's centre, same orientation: the near side is behind
    cams[1] = behind
    side = cams[0].copy()
    rot = np.array([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])
    side[0, :3, :3] = rot @ side[0, :3, :3]
    side[0, :3, 3] = -side[0, :3, :3] @ c0
    cams[2] = side
    ref = R.fuse(cams, depths, pairs, vthresh=0)
    P, Pi = R.matrices(cams)
    q = Pi[0] @ np.array([26.5 * depths[0, 18, 26], 18.5 * depths[0, 18, 26], depths[0, 18, 26], 1.0])   # view 0's centre pixel, in the world
    assert depths[0, 18, 26] > 0 and (P[1] @ q)[2] < 0                          # behind camera 1
    p2 = P[2] @ q
    assert p2[2] <= 0 or not (0 <= p2[0] / p2[2] <= 53 and 0 <= p2[1] / p2[2] <= 37)   # not in camera 2's image
    _check(cams, depths, pairs, vthresh=0)
    _check(cams, depths, pairs, vthresh=1)
    assert ref['counts'][0].max() <= 3


def test_strict_thresholds_on_exact_transforms():
    cams, depths, pairs = S.exact_self_pair()
    f = _check(cams, depths, pairs, vthresh=1)
    assert bool((f.counts == 1).all()) and len(f) == depths.size
    assert bool((_check(cams, depths, pairs, vthresh=1, pix_thresh=0.0).counts == 0).all())
    assert bool((_check(cams, depths, pairs, vthresh=1, dep_thresh=0.0).counts == 0).all())


def test_device_input_and_nonfinite_depths():
    cams, depths, pairs = S.make_views(6, (20, 28))
    depths = depths.copy()
    depths[0, 3, 4], depths[1, 5, 6], depths[2, 7, 8] = np.nan, np.inf, -1.0
    ref = R.fuse(cams, depths, pairs, vthresh=1)
    f = fusion.fuse_depths(torch.from_numpy(cams).cuda(), torch.from_numpy(depths).cuda(), pairs, vthresh=1)
    assert np.array_equal(_bits(f.points.cpu().numpy()), _bits(ref['points'])) and np.array_equal(f.masked_depths.cpu().numpy(), ref['masked_depths'])
    assert float(f.masked_depths[0, 3, 4]) == 0 and float(f.masked_depths[1, 5, 6]) == 0 and float(f.masked_depths[2, 7, 8]) == 0


def test_errors_raise_and_leave_the_device_usable():
    cams, depths, pairs = S.make_views(4, (20, 28), clean=True)
    good = fusion.fuse_depths(cams, depths, pairs)
    bad_cam = cams.copy()
    bad_cam[2, 1, 0, 0] = np.nan
    inf_cam = cams.copy()
    inf_cam[1, 0, 0, 3] = np.inf
    for args, kw in (((bad_cam, depths, pairs), {}), ((inf_cam, depths, pairs), {}), ((cams, depths, [[1], [4], [0], [2]]), {}),
                     ((cams, depths, [[1], [-1], [0], [2]]), {}), ((cams[:3], depths, pairs), {}), ((cams, depths, pairs[:3]), {}),
                     ((cams, depths, pairs), dict(probs=np.ones((4, 3, 20, 27), np.float32))),
                     ((cams, depths, pairs), dict(images=np.zeros((4, 28, 20, 3), np.uint8))),
                     ((cams, depths[:, :1], pairs), {}), ((cams, depths, pairs), dict(view=0))):
        with pytest.raises(ValueError):
            fusion.fuse_depths(*args, **kw)
        again = fusion.fuse_depths(cams, depths, pairs)
        assert torch.equal(again.points, good.points)


def test_the_library_refuses_what_the_binding_would_let_through():
    """the C entry validates on the host as well: its error bits reach the header without a launch"""
    from mvsdf_amd._lib import K, lib
    from mvsdf_amd.mesh import _header
    V, H, W = 2, 4, 4
    d = torch.ones(V, H, W, device='cuda')
    outs = [torch.zeros(V, H, W, device='cuda') for _ in range(2)] + [torch.zeros(V, H, W, dtype=torch.int32, device='cuda')]
    size = lib().mvsdf_fusion_workspace_bytes(V, H, W, 2)
    assert size > 0 and lib().mvsdf_fusion_workspace_bytes(V, 1, W, 2) == 0
    ws = torch.zeros(size, dtype=torch.uint8, device='cuda')
    pt = np.zeros(3, np.float32)
    eye = np.tile(np.eye(4).reshape(-1), 2 * 2 + V)

    def call(off, src, mats, view):
        off, src = np.asarray(off, np.int32), np.asarray(src, np.int32)
        rc = lib().mvsdf_fusion_fuse(d.data_ptr(), None, pt.ctypes.data, V, H, W, off.ctypes.data, src.ctypes.data, mats.ctypes.data, view, 1, 1.0, 0.01,
                                     ws.data_ptr(), size, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        return _header(ws, K.MVSDF_RES_H_WORDS)
    nan = eye.copy()
    nan[5] = np.nan
    assert call([0, 1, 2], [1, 0], nan, 10) == [0, K.MVSDF_FU_ERR_FINITE]
    assert call([0, 1, 2], [1, 2], eye, 10) == [0, K.MVSDF_FU_ERR_PAIR]
    assert call([0, 1, 2], [1, 0], eye, 0) == [0, K.MVSDF_FU_ERR_VIEW]
    assert call([0, 2, 2], [1, 0], eye, 1) == [0, K.MVSDF_FU_ERR_SHAPE]                          # a pair list longer than view
    n, err = call([0, 1, 2], [1, 0], eye, 10)
    assert err == 0 and n == V * H * W                                          # identity transforms: every pixel sees itself


@pytest.mark.parametrize('vhw', [(1, 2, 1024), (1, 3, 683), (2, 32, 33)])
def test_emit_across_a_scan_chunk_edge(vhw):
    """2048, 2049 and 2112 pixels: the kept pixels end at, one beyond, and well beyond the first 2048-pixel chunk of the keep-flag scan
    (csrc/geom_prims.h: mv_scan_blocks, and mv_chunk_rank in k_fu_emit).  The two-view scene with every hole filled, so vthresh = 0 keeps every pixel"""
    V, H, W = vhw
    cams, depths, _ = S.make_views(2, (H, W), clean=True)
    depths = np.where(depths > 0, depths, np.float32(2.5))[:V]
    cams, pairs = cams[:V], [[1], [0]][:V] if V == 2 else [[]]
    rs = np.random.RandomState(V * H * W)
    images = rs.randint(0, 256, (V, H, W, 3)).astype(np.uint8)
    _check(cams, depths, pairs, images=images, vthresh=0, want_points=lambda n: n == V * H * W)
    holes = np.where(rs.uniform(size=depths.shape) < 0.4, np.float32(0), depths)
    holes.reshape(-1)[[2047, -1]] = depths.reshape(-1)[[2047, -1]]              # both sides of the chunk edge are kept
    _check(cams, holes, pairs, images=images, vthresh=0, want_points=lambda n: V * H * W // 2 < n < V * H * W)
    if V == 2:
        _check(cams, depths, pairs, vthresh=1, want_points=lambda n: 0 < n < V * H * W)
    last = np.zeros_like(depths)
    last[-1, -1, -1] = depths[-1, -1, -1]
    f = _check(cams, last, pairs, images=images, vthresh=0, want_points=lambda n: n == 1)   # only the last pixel survives
    assert int(f.view[0]) == V - 1 and int(f.pixel[0]) == H * W - 1
