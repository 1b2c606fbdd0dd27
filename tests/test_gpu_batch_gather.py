"""mvsdf_batch_gather (csrc/batch_kernels.hip: k_batch_gather) called directly on synthetic device pools, against plain torch indexing of the same
pools.  Every output is a copy, so every comparison is bit-equal.

test_gpu_training.py compares the kernel with SceneDataset + collate_fn through one small scene; here are the places that scene does not reach: the
tail of the 16-byte feature copy (fmap_floats / 4 around the 1024-item unroll block, below one workgroup, a second block with one item), num_src = 0,
a view repeated in a batch, the whole-image route (pix NULL), an image width that is no power of two, a batch whose camera floats alone need the
grid-stride loop, more sampled pixels than 4096 workgroups hold, the guards that skip an out-of-range view, source view or pixel id, and the
argument refusals.

Every output buffer is prefilled with a sentinel and followed by a slack region that must keep it: a store past the end of an output, or into an
output a guard should have skipped, shows."""
import ctypes as C

import pytest
import torch

from mvsdf_amd._lib import lib
from mvsdf_amd.datasets.device_batches import BatchArgs

pytestmark = pytest.mark.gpu

F_SENT, B_SENT = -12345.678, 0xAB                # no pool holds them: the float pools are in (-1, 1) or integers >= 0, the masks 0 / 1
SLACK = 4096                                     # elements behind every output (feature maps: 1024 16-byte items, a whole unroll block)
OUT_B = ('o_omask', 'o_pmask')


def make_pools(n, img_w, img_h, depth_floats, fmap_floats, num_src, pmask=True, seed=0):
    g = torch.Generator().manual_seed(seed * 1000 + fmap_floats + 7 * num_src)
    TP = img_w * img_h
    u = lambda *s: (torch.rand(*s, generator=g) * 1.9 - 0.95).cuda()
    p = {'n': n, 'img_w': img_w, 'total_pixels': TP, 'depth_floats': depth_floats, 'fmap_floats': fmap_floats, 'num_src': num_src,
         'rgb': u(n, TP, 3), 'omask': (torch.rand(n, TP, generator=g) < 0.5).cuda(), 'pmask': (torch.rand(n, TP, generator=g) < 0.5).cuda() if pmask else None,
         'pose': u(n, 16), 'intrinsics': u(n, 16), 'cams_hd': u(n, 32), 'depth_cams': u(n, 32), 'depths': u(n, depth_floats),
         'size': u(1), 'center': u(3), 'feats': u(n, fmap_floats),
         'src': torch.stack([torch.randperm(n, generator=g)[:num_src] if num_src <= n else torch.randint(0, n, (num_src,), generator=g)
                             for _ in range(n)]).reshape(n, num_src).cuda()}
    return p


def out_shapes(p, B, P):
    V = p['num_src']
    return {'o_rgb': (B, P, 3), 'o_uv': (B, P, 2), 'o_omask': (B, P), 'o_pmask': (B, P), 'o_pose': (B, 16), 'o_intrinsics': (B, 16), 'o_cam': (B, 32),
            'o_src_cams': (B, V, 32), 'o_depths': (B, p['depth_floats']), 'o_depth_cams': (B, 32), 'o_size': (B,), 'o_center': (B, 3),
            'o_feat': (B, p['fmap_floats']), 'o_feat_src': (B, V, p['fmap_floats'])}


def alloc_outputs(p, B, P):
    """name -> (whole buffer = the output + SLACK, the output's view), all at the sentinel"""
    outs = {}
    for k, shape in out_shapes(p, B, P).items():
        numel = 1
        for s in shape:
            numel *= s
        if k in OUT_B:
            buf = torch.full((numel + SLACK,), B_SENT, dtype=torch.uint8, device='cuda')
        else:
            buf = torch.full((numel + SLACK,), F_SENT, dtype=torch.float32, device='cuda')
        outs[k] = (buf, buf[:numel].view(shape))
    return outs


def make_args(p, views, pix, outs, P, over=None):
    dp = lambda x: None if x is None else x.data_ptr()
    kw = dict(B=int(views.numel()), n=p['n'], num_src=p['num_src'], P=P, img_w=p['img_w'], total_pixels=p['total_pixels'],
              depth_floats=p['depth_floats'], fmap_floats=p['fmap_floats'], views=dp(views), pix=dp(pix), src=dp(p['src']) if p['num_src'] else None)
    for k in ('rgb', 'omask', 'pmask', 'pose', 'intrinsics', 'cams_hd', 'depth_cams', 'depths', 'size', 'center', 'feats'):
        kw[k] = dp(p[k])
    for k, (buf, _) in outs.items():
        kw[k] = buf.data_ptr()
    if p['pmask'] is None:
        kw['o_pmask'] = None
    if not p['num_src']:                                                            # (zero-sized outputs: the kernel needs no pointer for them)
        kw['o_src_cams'] = kw['o_feat_src'] = None
    kw.update(over or {})
    return BatchArgs(**kw)


def call(a):
    rc = lib().mvsdf_batch_gather(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc


def expected(p, views, pix, B, P):
    """What the header of mvsdf_batch_gather documents, by torch indexing; outputs of a skipped view, source view or pixel id keep the sentinel."""
    n, TP, V, W = p['n'], p['total_pixels'], p['num_src'], p['img_w']
    exp = {}
    for k, shape in out_shapes(p, B, P).items():
        exp[k] = torch.full(shape, B_SENT, dtype=torch.uint8, device='cuda') if k in OUT_B else torch.full(shape, F_SENT, dtype=torch.float32, device='cuda')
    ids = torch.arange(TP, device='cuda') if pix is None else pix
    ok = (ids >= 0) & (ids < TP)
    good = ids[ok]
    for b, v in enumerate(views.tolist()):
        if not 0 <= v < n:
            continue                                                                # everything of this view stays unwritten
        exp['o_rgb'][b, ok] = p['rgb'][v, good]
        exp['o_uv'][b, ok] = torch.stack([good % W, good // W], -1).float()
        exp['o_omask'][b, ok] = p['omask'][v, good].view(torch.uint8)
        if p['pmask'] is not None:
            exp['o_pmask'][b, ok] = p['pmask'][v, good].view(torch.uint8)
        for k, src in (('o_pose', 'pose'), ('o_intrinsics', 'intrinsics'), ('o_cam', 'cams_hd'), ('o_depth_cams', 'depth_cams'), ('o_depths', 'depths'),
                       ('o_feat', 'feats')):
            exp[k][b] = p[src][v]
        exp['o_size'][b] = p['size'][0]
        exp['o_center'][b] = p['center']
        for s in range(V):
            sv = int(p['src'][v, s])
            if 0 <= sv < n:
                exp['o_src_cams'][b, s] = p['cams_hd'][sv]
                exp['o_feat_src'][b, s] = p['feats'][sv]
    return exp


def check(p, outs, exp):
    torch.cuda.synchronize()
    for k, (buf, view) in outs.items():
        numel = view.numel()
        sent = B_SENT if k in OUT_B else F_SENT
        assert bool((buf[numel:] == sent).all()), '%s: written past its end' % k
        if (k == 'o_pmask' and p['pmask'] is None) or (k in ('o_src_cams', 'o_feat_src') and not p['num_src']):
            assert bool((view == sent).all()), k
            continue
        if not torch.equal(view, exp[k]):
            bad = torch.nonzero((view != exp[k]).reshape(-1)).flatten()
            raise AssertionError('%s: %d of %d elements differ, first at flat index %d' % (k, bad.numel(), numel, int(bad[0])))


def run(p, views, pix):
    views = torch.as_tensor(views, dtype=torch.int64).cuda()
    B = int(views.numel())
    P = p['total_pixels'] if pix is None else int(pix.numel())
    outs = alloc_outputs(p, B, P)
    rc = call(make_args(p, views, pix, outs, P))
    assert rc == 0, lib().mvsdf_last_error().decode()
    check(p, outs, expected(p, views, pix, B, P))
    return outs


def _pix(p, P, seed=1):
    if P is None:
        return None
    return torch.randint(0, p['total_pixels'], (P,), generator=torch.Generator().manual_seed(seed + P)).cuda()


FMAPS = (4, 1020, 1024, 4092, 4096, 4100, 4 * (4 * 1024 + 1))                       # m4 = 1, 255, 256, 1023, 1024, 1025, 4097
PS = (1, 100, 257, None)                                                            # None: the whole image, pix NULL
# (fmap_floats, num_src, B, P, pmask): every tail with no, one and three source views; B, P and the perfect mask rotate so that every value of each
# appears with small and large maps
TAILS = [(f, v, (1, 3)[i % 2], PS[(i // 2) % 4], bool((i // 3) % 2)) for i, (f, v) in enumerate((f, v) for f in FMAPS for v in (0, 1, 3))]


@pytest.mark.parametrize('fmap_floats,num_src,B,P,pmask', TAILS, ids=['f%d-src%d-B%d-P%s-%s' % (f, v, B, P or 'all', 'pmask' if pm else 'nopmask')
                                                                      for f, v, B, P, pm in TAILS])
def test_feature_copy_tails(fmap_floats, num_src, B, P, pmask):
    """The 16-byte copy at every tail of its 4 x 256-item unroll block."""
    p = make_pools(5, 7, 43, 15, fmap_floats, num_src, pmask=pmask, seed=fmap_floats + num_src)
    views = [3] if B == 1 else [4, 0, 4]                                            # a view twice in one batch
    run(p, views, _pix(p, P))


@pytest.mark.parametrize('pmask', [True, False])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('P', PS)
@pytest.mark.parametrize('num_src', [0, 1, 3])
def test_pixels_views_and_masks(num_src, P, B, pmask):
    """7 x 43 pixels (the width divides no power of two: o_uv is x = id mod W, y = id div W), 15 depth floats, every P with every B and num_src."""
    p = make_pools(4, 7, 43, 15, 1024, num_src, pmask=pmask, seed=11)
    outs = run(p, [2] if B == 1 else [1, 3, 1], _pix(p, P))
    uv = outs['o_uv'][1]
    ids = torch.arange(p['total_pixels'], device='cuda') if P is None else _pix(p, P)
    assert torch.equal(uv[..., 0] + 7 * uv[..., 1], ids.float().expand(B, -1))     # (exact: ids < 2^24)
    assert float(uv[..., 0].max()) <= 6


def test_camera_floats_alone_need_the_grid_stride():
    """B = 3, P = 1, one depth float, 4 feature floats: the launch has one workgroup per role (256 threads) for 6 + 3 x 196 items."""
    p = make_pools(6, 1, 1, 1, 4, 3, seed=3)
    run(p, [5, 0, 2], None)
    p = make_pools(3, 2, 1, 1, 4, 8, seed=4)                                        # more source views than views: 356 camera floats per view
    run(p, [1], _pix(p, 1))


def test_more_pixels_than_the_grid_holds():
    """Whole images of 700 x 501 pixels, B = 3: 1,052,100 sampled pixels against 4096 workgroups x 256 threads -- the second role's grid-stride loop."""
    p = make_pools(3, 700, 501, 35, 4100, 1, seed=5)
    assert 3 * p['total_pixels'] > 4096 * 256
    run(p, [2, 0, 2], None)


def test_guards_leave_exactly_the_documented_outputs_unwritten():
    """A view id of -1 or n: every output of that batch row.  A source id out of range: that source's camera and feature map, nothing else.  A pixel id
    of -1 or total_pixels: rgb, uv and both masks of that sample in every view.  `expected` models exactly that; everything else must be correct."""
    P = 100
    for bad_view in (-1, 5, 1 << 40):
        p = make_pools(5, 7, 43, 15, 4100, 3, seed=21)
        run(p, [2, bad_view, 4], _pix(p, P))
        run(p, [bad_view], None)
    for bad_src in (-1, 5, -(1 << 35)):
        p = make_pools(5, 7, 43, 15, 4100, 3, seed=22)
        p['src'][2, 1] = bad_src                                                    # view 2's second source
        p['src'][4, 0] = bad_src
        outs = run(p, [2, 0, 4], _pix(p, P))
        assert bool((outs['o_feat_src'][1][0, 1] == F_SENT).all()) and bool((outs['o_src_cams'][1][2, 0] == F_SENT).all())   # (the model above did skip them)
        assert not bool((outs['o_feat_src'][1][0, 0] == F_SENT).any()) and not bool((outs['o_feat'][1] == F_SENT).any())
    p = make_pools(5, 7, 43, 15, 1024, 1, seed=23)
    pix = _pix(p, P)
    pix[[0, 17, 63, 64, 99]] = torch.tensor([-1, p['total_pixels'], 1 << 40, -(1 << 33), p['total_pixels'] + 6], device='cuda')
    outs = run(p, [3, 1, 3], pix)
    for k in ('o_rgb', 'o_uv', 'o_omask', 'o_pmask'):
        sent = B_SENT if k in OUT_B else F_SENT
        assert bool((outs[k][1][:, [0, 17, 63, 64, 99]] == sent).all()) and not bool((outs[k][1][:, 1:17] == sent).any())
    # all three at once
    p = make_pools(5, 7, 43, 15, 4092, 3, pmask=False, seed=24)
    p['src'][0, 2] = 5
    pix = _pix(p, 257)
    pix[256] = -1
    run(p, [0, 5, 0], pix)


def test_refusals_launch_nothing_and_a_valid_call_follows():
    p = make_pools(5, 7, 43, 15, 1024, 3, seed=31)
    views = torch.tensor([1, 4], device='cuda')
    pix = _pix(p, 100)
    outs = alloc_outputs(p, 2, 100)
    good = make_args(p, views, pix, outs, 100)
    ptr_fields = [k for k, _ in BatchArgs._fields_ if k not in ('B', 'n', 'num_src', 'P', 'img_w', 'total_pixels', 'depth_floats', 'fmap_floats')]
    refusals = [('fmap_floats 6', dict(fmap_floats=6)), ('fmap_floats 0', dict(fmap_floats=0)), ('fmap_floats 2', dict(fmap_floats=2)),
                ('fmap_floats -4', dict(fmap_floats=-4)),
                ('feats + 4 bytes', dict(feats=good.feats + 4)), ('o_feat + 4 bytes', dict(o_feat=good.o_feat + 4)),
                ('o_feat_src + 4 bytes', dict(o_feat_src=good.o_feat_src + 4)), ('feats + 8 bytes', dict(feats=good.feats + 8)),
                ('B (1 + num_src) = 65535', dict(B=65535, num_src=0)), ('B (1 + num_src) = 65535, num_src 2', dict(B=21845, num_src=2)),
                ('pix NULL, P != total_pixels', dict(pix=None)), ('total_pixels % img_w', dict(img_w=8)),
                ('B 0', dict(B=0)), ('n 0', dict(n=0)), ('num_src -1', dict(num_src=-1)), ('P 0', dict(P=0)), ('img_w 0', dict(img_w=0)),
                ('total_pixels 0', dict(total_pixels=0)), ('depth_floats 0', dict(depth_floats=0))]
    refusals += [('%s NULL' % k, {k: None}) for k in ptr_fields if k not in ('pix', 'pmask')]
    assert len(ptr_fields) == 28 and len(refusals) == 19 + 26
    for what, over in refusals:
        a = make_args(p, views, pix, outs, 100, over)
        rc = call(a)
        assert rc != 0, what
        assert 'mvsdf_batch_gather' in lib().mvsdf_last_error().decode(), what
    assert lib().mvsdf_batch_gather(None, None) != 0
    torch.cuda.synchronize()
    for k, (buf, _) in outs.items():
        assert bool((buf == (B_SENT if k in OUT_B else F_SENT)).all()), '%s was written by a refused call' % k
    # the optional pointers are optional: no perfect mask pool -> its output is left alone; then the plain valid call
    rc = call(make_args(p, views, pix, outs, 100, dict(pmask=None, o_pmask=None)))
    assert rc == 0
    exp = expected(p, views, pix, 2, 100)
    exp['o_pmask'][:] = B_SENT
    check(p, outs, exp)
    run(p, [1, 4], pix)
