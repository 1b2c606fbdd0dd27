"""Chart atlases on the device: the stage between face labels and texels that makes a texture atlas of photographs usable in a viewer.  texture.py
gives every face a patch of its own: a UV seam along every edge, two fifths of the atlas gutter, a one-texel guarantee that holds at mip level 0
only, and label islands of one face.  Texture tools for photographs (Waechter et al., "Let there be color") avoid all four the same way, and so does
this module: a CHART is a connected region of faces that took the same photograph, its patch is a rectangle cut from that photograph with a margin
of `pad` texels, and small islands are absorbed by their neighbours first.  Kernels: csrc/charts.hip (the design: DESIGN.md);
tests/charts_ref.py restates every step in numpy.  The reference has no texturing code; the definition below is this project's, written so that the
schedule cannot change a bit of the result.

The definition (fp64 throughout, in the order written, no FMA contraction; fp32 and uint8 inputs are promoted exactly; every integer decision is
an exact comparison; every sum or extremum over faces is one of integers).  Cameras, pixel_center o, the projection, E(p, q, r), the visibility
rule and the bilinear rule are those of raster.py / texture.py, word for word.

1. Score of a face in a named view (face_scores).  Step 1 of texture.py's definition for the one view view[f]: score = |A| where that view is a
   candidate for f, else 0; screen holds the six screen coordinates (0 where the score is 0).  view = -1 gives 0.
2. Neighbours (face_neighbors).  Edge e of face f joins corners e and (e + 1) % 3.  Among the 3F edges, those with the same two vertex ids (in
   either order) form a group; an edge whose two ids are equal is in no group.  nbr[f, e] = g where the group of (f, e) has exactly two edges and
   the other belongs to another face g; otherwise -1 (a boundary, a non-manifold edge, a repeated vertex, or a face that holds both edges itself).
   Charts (face_charts).  Faces f ~ g are linked iff they are neighbours and label_f == label_g >= 0.  The charts are the connected components of
   the linked faces, numbered ascending by their lowest face; face_chart is -1 on unlabelled faces; chart_view[c] is the label, chart_faces[c] the
   number of faces.
3. Absorption (smooth_labels).  In each of `rounds` rounds the charts and their sizes are computed from the current labels.  A labelled face f in a
   chart with fewer than min_faces faces considers, over its three edges in order, every neighbour g with label_g >= 0, label_g != label_f, whose
   chart has at least min_faces faces, and for which the score of f in view label_g (step 1) is > 0.  It takes the view with the largest such
   score, ties to the lower view; without such a neighbour it stays.  All faces decide from the round's starting state.  Charts of min_faces faces
   or more never change, so nothing oscillates; min_faces = 1 or rounds = 0 is the identity; unlabelled faces stay unlabelled.  Score and screen
   are those of step 1 for the final labels.
4. Rectangles.  With d = texel_density and pad in {1, 2, 4, 8}: over the corners of a chart's faces in its view, u = sx - o and t = sy - o (in
   [0, W-1] x [0, H-1] by the candidate rule; a value outside, or a NaN, is clamped into it first), u0 = floor(min u), u1 = ceil(max u), likewise
   t0, t1; w = roundup(ceil((u1 - u0) * d) + 1 + 2 * pad, pad), h likewise.  A side is capped at RECT_CAP = 65536 (a multiple of every pad and above
   every max_size, so a capped chart always forces a halving).
5. Packing.  The charts are ordered by h descending, stable in the chart id.  Wt is the smallest power of two with Wt >= max w and Wt * Wt >= the
   sum of w * h.  The shelves are filled in that order: a chart whose x + w > Wt opens a new shelf at x = 0; a shelf's height is the h of its first
   chart; Y is the sum of the earlier shelves' heights; Ht is the sum of all.  While Wt or Ht exceeds max_size, d is halved and step 4 repeated;
   when that happens although no side exceeds roundup(2 + 2 * pad, pad): ValueError.  The density finally used is reported.  chart_rect int32
   [C,6] = (X, Y, w, h, u0, t0); origins and sizes are multiples of pad.  No chart: a pad x pad atlas of the fallback colour.
6. UVs.  A corner with (u, t) in its chart's view lies at x = (X + pad + 0.5) + (u - u0) * d, y = (Y + pad + 0.5) + (t - t0) * d;
   uv fp32 [F,3,2] = (x / Wt, 1 - y / Ht), computed in fp64 and rounded once.  Faces without a chart get texel (0, 0)'s centre, (0.5, 0.5).
   Fill.  Texel (i, j) outside every rectangle gets `fallback` and valid = 0.  Inside the rectangle of chart c with view v:
   u = u0 + (i - X - pad) / d, t = t0 + (j - Y - pad) / d, both clamped to the image (a NaN becomes 0); the bilinear rule gives the colour c per
   channel; texel = uint8(floor(c + 0.5)), valid = 1.  The whole rectangle is filled: the margin is the photograph's own continuation.
7. Face map.  face_map int32 [Ht,Wt] starts at -1.  The centre (i + 0.5, j + 0.5) of a texel of chart c's rectangle is covered by face f of that
   chart iff, with a, b, c the face's corners in the fp64 atlas coordinates of step 6 and A = E(a, b, c): A > 0 and E(b, c, p), E(c, a, p),
   E(a, b, p) are all >= 0, or A < 0 and all are <= 0 (A == 0 covers nothing); only the texels floor(min x) - 1 <= i <= ceil(max x) + 1 over the
   face's corners, likewise j, are asked (rounding lets the test pass a centre a hair outside the corners' box, so the box is part of the
   definition).  The lowest covering face wins.  Then `pad` dilation rounds: a
   texel inside a rectangle that holds -1 takes the lowest non-negative entry among its 4-neighbours inside the same rectangle, read from the
   round before.  Levelled fill: for a texel with face f, alpha = E(b, c, p) / A, beta = E(c, a, p) / A, gamma = E(a, b, p) / A (they extrapolate
   in the margin); c' = c + ((alpha * g_a + beta * g_b) + gamma * g_c) with seams.py's corrections of the face's three nodes; c' is clamped to
   [0, 255] (a NaN becomes 0) and rounded as above.  Texels with -1 keep c.  With g = 0 the result is the plain fill byte for byte.

Two properties follow.  At d = 1 every valid texel is a pixel of the photograph, byte for byte (u and t are integers: a verbatim crop).  And a
bilinear lookup at (x, y) inside a face's UV triangle reads the texels floor(x - 0.5) + {0, 1}: x >= X + pad + 0.5 gives an index >= X + pad, and
x <= X + pad + 0.5 + ceil((u1 - u0) * d) <= X + w - pad - 0.5 gives an index <= X + w - pad: inside the rectangle, with pad - 1 texels to spare
at the top.  At mip level m = log2(pad) the same holds for the 2^m x 2^m blocks, because origins and sizes are multiples of pad: the block indices
lie in [X / pad, (X + w) / pad - 1].

Nothing here allocates uninitialised memory: outputs and workspaces come from torch.zeros / torch.full, and every stage takes an optional
workspace= byte tensor (chart_workspace_bytes) whose contents it does not rely on.  Argument errors raise ValueError before anything is launched; a
mesh on the CPU raises MvsdfError; what the device finds (ERRORS) raises ValueError after the call.
"""
import numpy as np
import torch

from . import raster as R
from . import texture as T
from ._lib import check, lib, K, raise_for_bits, _header, _stream, _vp
from .seams import _tensor

PADS = (1, 2, 4, 8)
RECT_CAP = K.MVSDF_CA_RECT_CAP
MAX_ROUNDS = K.MVSDF_CA_MAX_ROUNDS

# the error bits of a chart call (csrc/charts.hip), in the order they are looked at
ERRORS = [(K.MVSDF_TX_ERR_FINITE, ValueError, 'a camera or centre entry is NaN or infinite'),
          (K.MVSDF_TX_ERR_INDEX, ValueError, 'an index (face -> vertex, face -> neighbour, face -> chart, a table entry, corner -> node) is out of range'),
          (K.MVSDF_TX_ERR_LABEL, ValueError, 'a face label is outside [-1, V)'),
          (K.MVSDF_TX_ERR_COUNTS, ValueError, 'a chart has no face: face_chart is not the one of these charts'),
          (K.MVSDF_TX_ERR_ROUNDS, RuntimeError, 'the components did not settle within %d rounds' % K.MVSDF_CA_MAX_ROUNDS)]


class ChartPacking:
    """The result of pack_charts, on the device: chart_rect int32 [C,6] = (X, Y, w, h, u0, t0); order int32 [C], the charts by h descending, id
    ascending; xs int32 [C], X by place in that order; shelves int32 [S+1,2] = (first place, Y), the last entry (C, Ht); and the ints Wt, Ht, pad
    and the density finally used."""

    def __init__(self, chart_rect, order, xs, shelves, Wt, Ht, density, pad):
        self.chart_rect, self.order, self.xs, self.shelves = chart_rect, order, xs, shelves
        self.Wt, self.Ht, self.density, self.pad = Wt, Ht, density, pad

    @property
    def charts(self):
        return self.chart_rect.shape[0]


def chart_workspace_bytes(faces=0, texels=0):
    """bytes of a workspace= that serves every stage on a mesh of that many faces, and face_map on an atlas of `texels` texels"""
    size = lib().mvsdf_charts_workspace_bytes(int(faces), int(texels))
    if size == 0:
        raise ValueError('chart_workspace_bytes: %d faces, %d texels are beyond the limits' % (faces, texels))
    return size


def _workspace(workspace, faces, texels, dev, what):
    """the caller's byte tensor, checked, or a zeroed one"""
    size = lib().mvsdf_charts_workspace_bytes(int(faces), int(texels))
    if size == 0:
        raise ValueError('%s: %d faces (at most 2^28), %d texels' % (what, faces, texels))
    if workspace is None:
        return torch.zeros(size, dtype=torch.uint8, device=dev)
    if not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.dim() != 1 or not workspace.is_contiguous():
        raise ValueError('%s: workspace must be a contiguous uint8 vector' % what)
    if workspace.device != dev:
        raise ValueError('%s: the workspace is on %s, the data on %s' % (what, workspace.device, dev))
    if workspace.numel() < size:
        raise ValueError('%s: the workspace holds %d bytes, %d are needed (chart_workspace_bytes)' % (what, workspace.numel(), size))
    if workspace.data_ptr() % 256:
        raise ValueError('%s: the workspace must be 256-byte aligned' % what)
    return workspace


def _raise(ws, what):
    hdr = _header(ws, K.MVSDF_CA_H_WORDS)
    raise_for_bits(hdr[K.MVSDF_CA_H_ERR], what, ERRORS)
    return hdr


def _pad(pad, what):
    if isinstance(pad, (bool, np.bool_)) or not isinstance(pad, (int, np.integer)) or pad not in PADS:
        raise ValueError('%s: pad must be 1, 2, 4 or 8, got %r' % (what, pad))
    return int(pad)


def _int(name, x, lo, hi, what):
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) or not lo <= x <= hi:
        raise ValueError('%s: %s must be an int in [%d, %d], got %r' % (what, name, lo, hi, x))
    return int(x)


def _fallback(fallback, what):
    fb = np.asarray(fallback)
    if fb.shape != (3,) or not np.issubdtype(fb.dtype, np.integer) or fb.min() < 0 or fb.max() > 255:
        raise ValueError('%s: fallback must be three ints in 0 .. 255, got %r' % (what, fallback))
    return [int(c) for c in fb]


def _images(images, dev, what):
    img = torch.as_tensor(images)
    if img.dim() != 4 or img.shape[3] != 3 or img.dtype != torch.uint8:
        raise ValueError('%s: images must be uint8 [V, H, W, 3], got %s %s' % (what, img.dtype, tuple(img.shape)))
    V, H, W = img.shape[:3]
    H, W = R._hw((H, W), what)
    return img.to(dev).contiguous(), V, H, W


def _view_call(mesh, raster, masks, depth_tol, cos_min, ignore_normals, what):
    """what the test of a face in a view reads, as the leading arguments of the two calls that run it -> (args, nf, device)"""
    V, H, W, m, tol, cmin, C, dev = T._view_args(mesh, raster, masks, depth_tol, cos_min, what)
    nv, nf = mesh.vertices.shape[0], mesh.faces.shape[0]
    keep = (mesh.vertices.contiguous(), mesh.normals.to(dev).contiguous(), mesh.faces.to(dev).contiguous(), torch.from_numpy(raster.P).to(dev),
            torch.from_numpy(C).to(dev), raster.depth.contiguous(), m)
    v, n, f, Pd, Cd, depth, m = keep
    args = (_vp(v), _vp(n), _vp(f), nv, nf, _vp(Pd), _vp(Cd), V, H, W, raster.pixel_center, _vp(depth), _vp(m), tol, cmin, 1 if ignore_normals else 0)
    return args, keep, nf, V, dev


def face_scores(mesh, raster, view, masks=None, depth_tol=0.01, cos_min=0.0, ignore_normals=False, workspace=None):
    """step 1: (score fp64 [F], screen fp64 [F,6]) of every face in the one view view int32 [F] names for it (-1: none)"""
    what = 'face_scores'
    args, keep, nf, V, dev = _view_call(mesh, raster, masks, depth_tol, cos_min, ignore_normals, what)
    view = _tensor('view', view, torch.int32, (nf,), dev, what)
    ws = _workspace(workspace, nf, 0, dev, what)
    score = torch.zeros(nf, dtype=torch.float64, device=dev)
    screen = torch.zeros(nf, 6, dtype=torch.float64, device=dev)
    check(lib().mvsdf_charts_face_scores(*args, _vp(view), _vp(ws), ws.numel(), _vp(score), _vp(screen), _stream(ws)), 'mvsdf_charts_face_scores')
    _raise(ws, what)
    return score, screen


def face_neighbors(mesh, workspace=None):
    """step 2: nbr int32 [F,3], the face across every edge or -1"""
    what = 'face_neighbors'
    R._mesh(mesh, what, faces=False)
    dev = R._on_device(mesh, what)
    nv, nf = mesh.vertices.shape[0], mesh.faces.shape[0]
    faces = _tensor('faces', mesh.faces, torch.int32, (nf, 3), dev, what)
    ws = _workspace(workspace, nf, 0, dev, what)
    nbr = torch.full((nf, 3), -1, dtype=torch.int32, device=dev)
    check(lib().mvsdf_charts_neighbors(_vp(faces), nv, nf, _vp(ws), ws.numel(), _vp(nbr), _stream(ws)), 'mvsdf_charts_neighbors')
    _raise(ws, what)
    return nbr


def _labels(labels, nbr, what):
    if not isinstance(labels, torch.Tensor) or not labels.is_cuda:
        raise ValueError('%s: labels must be an int32 tensor on the GPU' % what)
    dev = labels.device
    nf = labels.shape[0] if labels.dim() == 1 else None
    labels = _tensor('labels', labels, torch.int32, (nf,), dev, what)
    nbr = _tensor('nbr', nbr, torch.int32, (nf, 3), dev, what)
    return labels, nbr, nf, dev


def face_charts(labels, nbr, workspace=None):
    """step 2: (face_chart int32 [F], chart_view int32 [C], chart_faces int32 [C]) of labels int32 [F] and face_neighbors' nbr"""
    what = 'face_charts'
    labels, nbr, nf, dev = _labels(labels, nbr, what)
    ws = _workspace(workspace, nf, 0, dev, what)
    face_chart = torch.full((nf,), -1, dtype=torch.int32, device=dev)
    chart_view = torch.zeros(nf, dtype=torch.int32, device=dev)
    chart_faces = torch.zeros(nf, dtype=torch.int32, device=dev)
    if nf == 0:
        return face_chart, chart_view, chart_faces
    check(lib().mvsdf_charts_components(_vp(labels), _vp(nbr), nf, _vp(ws), ws.numel(), _vp(face_chart), _vp(chart_view), _vp(chart_faces), _stream(ws)),
          'mvsdf_charts_components')
    c = _raise(ws, what)[K.MVSDF_CA_H_CHARTS]
    return face_chart, chart_view[:c], chart_faces[:c]


def smooth_labels(mesh, raster, labels, min_faces=4, rounds=2, masks=None, depth_tol=0.01, cos_min=0.0, ignore_normals=False, nbr=None,
                  workspace=None):
    """step 3: (labels int32 [F], score fp64 [F], screen fp64 [F,6], the number of labels each round changed) from labels int32 [F]"""
    what = 'smooth_labels'
    min_faces = _int('min_faces', min_faces, 1, 2 ** 31 - 1, what)
    rounds = _int('rounds', rounds, 0, 1024, what)
    args, keep, nf, V, dev = _view_call(mesh, raster, masks, depth_tol, cos_min, ignore_normals, what)
    labels = _tensor('labels', labels, torch.int32, (nf,), dev, what)
    ws = _workspace(workspace, nf, 0, dev, what)
    if nbr is None:
        nbr = face_neighbors(mesh, workspace=ws)
    nbr = _tensor('nbr', nbr, torch.int32, (nf, 3), dev, what)
    score, screen = face_scores(mesh, raster, labels, masks, depth_tol, cos_min, ignore_normals, workspace=ws)
    changes = []
    for _ in range(rounds if nf and min_faces > 1 else 0):
        face_chart, chart_view, chart_faces = face_charts(labels, nbr, workspace=ws)
        out = torch.full((nf,), -1, dtype=torch.int32, device=dev)
        if chart_faces.shape[0]:
            check(lib().mvsdf_charts_absorb(*args, _vp(labels), _vp(nbr), _vp(face_chart), _vp(chart_faces), chart_faces.shape[0], min_faces, _vp(ws),
                                            ws.numel(), _vp(out), _vp(score), _vp(screen), _stream(ws)), 'mvsdf_charts_absorb')
            changes.append(_raise(ws, what)[K.MVSDF_CA_H_CHANGES])
            labels = out
        else:
            changes.append(0)
    changes += [0] * (rounds - len(changes))
    return labels, score, screen, changes


def pack_charts(face_chart, charts, screen, hw, pixel_center=0.5, texel_density=1.0, max_size=8192, pad=4, workspace=None):
    """steps 4 and 5 for face_chart int32 [F] with `charts` charts (at least one) and the screen table of their labels, in images of hw = (H, W)
    -> ChartPacking"""
    what = 'pack_charts'
    pad = _pad(pad, what)
    H, W = R._hw(hw, what)
    o = R._center(pixel_center, what)
    max_size = _int('max_size', max_size, pad, T.MAX_SIZE, what)
    d = _density(texel_density, what)
    if not isinstance(face_chart, torch.Tensor) or not face_chart.is_cuda or face_chart.dim() != 1:
        raise ValueError('%s: face_chart must be an int32 vector on the GPU' % what)
    dev, nf = face_chart.device, face_chart.shape[0]
    face_chart = _tensor('face_chart', face_chart, torch.int32, (nf,), dev, what)
    screen = _tensor('screen', screen, torch.float64, (nf, 6), dev, what)
    nc = _int('charts', charts, 1, max(nf, 1), what)
    ws = _workspace(workspace, nf, 0, dev, what)
    rect = torch.zeros(nc, 6, dtype=torch.int32, device=dev)
    order = torch.zeros(nc, dtype=torch.int32, device=dev)
    xs = torch.zeros(nc, dtype=torch.int32, device=dev)
    shelves = torch.zeros(nc + 1, 2, dtype=torch.int32, device=dev)
    least = (2 + 2 * pad + pad - 1) // pad * pad
    while True:
        check(lib().mvsdf_charts_pack(_vp(face_chart), _vp(screen), nf, nc, o, H, W, d, pad, _vp(ws), ws.numel(), _vp(rect), _vp(order), _vp(xs),
                                      _vp(shelves), _stream(ws)), 'mvsdf_charts_pack')
        hdr = _raise(ws, what)
        Wt, Ht, ns = hdr[K.MVSDF_CA_H_WT], hdr[K.MVSDF_CA_H_HT], hdr[K.MVSDF_CA_H_SHELVES]
        if Wt <= max_size and Ht <= max_size:
            break
        if hdr[K.MVSDF_CA_H_MAXW] <= least and hdr[K.MVSDF_CA_H_MAXH] <= least:
            raise ValueError('%s: %d charts do not fit an atlas of %d texels a side, even at %d texels each' % (what, nc, max_size, least))
        d = d / 2.0
    return ChartPacking(rect, order, xs, shelves[:ns + 1], Wt, Ht, d, pad)


def _density(texel_density, what):
    try:
        d = float(texel_density)
    except (TypeError, ValueError):
        raise ValueError('%s: texel_density must be a number, got %r' % (what, texel_density)) from None
    if not (np.isfinite(d) and d > 0):
        raise ValueError('%s: texel_density must be finite and > 0, got %r' % (what, texel_density))
    return d


def _packing(p, what):
    if not isinstance(p, ChartPacking):
        raise ValueError('%s: a ChartPacking (pack_charts) is needed, got %s' % (what, type(p).__name__))
    dev = p.chart_rect.device
    nc = p.chart_rect.shape[0]
    ns = p.shelves.shape[0] - 1
    _tensor('chart_rect', p.chart_rect, torch.int32, (nc, 6), dev, what)
    _tensor('order', p.order, torch.int32, (nc,), dev, what)
    _tensor('xs', p.xs, torch.int32, (nc,), dev, what)
    _tensor('shelves', p.shelves, torch.int32, (ns + 1, 2), dev, what)
    if not dev.type == 'cuda' or nc < 1 or not 1 <= ns <= nc or p.Wt % 4 or not 4 <= p.Wt <= T.MAX_SIZE or not 1 <= p.Ht <= T.MAX_SIZE:
        raise ValueError('%s: the packing is not one of pack_charts' % what)
    _pad(p.pad, what)
    return dev, nc, ns


def chart_uvs(face_chart, screen, packing, pixel_center=0.5, workspace=None):
    """step 6: uv fp32 [F,3,2]"""
    what = 'chart_uvs'
    dev, nc, ns = _packing(packing, what)
    o = R._center(pixel_center, what)
    nf = face_chart.shape[0] if isinstance(face_chart, torch.Tensor) and face_chart.dim() == 1 else None
    face_chart = _tensor('face_chart', face_chart, torch.int32, (nf,), dev, what)
    screen = _tensor('screen', screen, torch.float64, (nf, 6), dev, what)
    ws = _workspace(workspace, nf, 0, dev, what)
    uv = torch.zeros(nf, 3, 2, dtype=torch.float32, device=dev)
    p = packing
    check(lib().mvsdf_charts_uv(_vp(face_chart), _vp(screen), nf, _vp(p.chart_rect), nc, o, p.density, p.pad, p.Ht, p.Wt, _vp(ws), ws.numel(), _vp(uv),
                                _stream(ws)), 'mvsdf_charts_uv')
    _raise(ws, what)
    return uv


def face_map(face_chart, screen, packing, pixel_center=0.5, workspace=None):
    """step 7: face_map int32 [Ht,Wt], the face under every texel of a rectangle (dilated `pad` rounds), -1 elsewhere"""
    what = 'face_map'
    dev, nc, ns = _packing(packing, what)
    o = R._center(pixel_center, what)
    nf = face_chart.shape[0] if isinstance(face_chart, torch.Tensor) and face_chart.dim() == 1 else None
    face_chart = _tensor('face_chart', face_chart, torch.int32, (nf,), dev, what)
    screen = _tensor('screen', screen, torch.float64, (nf, 6), dev, what)
    p = packing
    ws = _workspace(workspace, nf, p.Ht * p.Wt, dev, what)
    fmap = torch.full((p.Ht, p.Wt), -1, dtype=torch.int32, device=dev)
    check(lib().mvsdf_charts_face_map(_vp(face_chart), _vp(screen), nf, o, _vp(p.chart_rect), _vp(p.order), _vp(p.xs), _vp(p.shelves), nc, ns, p.density,
                                      p.pad, p.Ht, p.Wt, _vp(ws), ws.numel(), _vp(fmap), _stream(ws)), 'mvsdf_charts_face_map')
    _raise(ws, what)
    return fmap


def _fill(what, images, chart_view, packing, fallback, workspace, level=None):
    dev, nc, ns = _packing(packing, what)
    img, V, H, W = _images(images, dev, what)
    fb = _fallback(fallback, what)
    chart_view = _tensor('chart_view', chart_view, torch.int32, (nc,), dev, what)
    p = packing
    if level is None:
        extra, nf = (None, None, None, 0.5, 0, None, None, 0), 0
    else:
        fmap, face_chart, screen, graph, g, o = level
        o = R._center(o, what)
        nf = face_chart.shape[0] if isinstance(face_chart, torch.Tensor) and face_chart.dim() == 1 else None
        fmap = _tensor('face_map', fmap, torch.int32, (p.Ht, p.Wt), dev, what)
        face_chart = _tensor('face_chart', face_chart, torch.int32, (nf,), dev, what)
        screen = _tensor('screen', screen, torch.float64, (nf, 6), dev, what)
        corner = _tensor('corner_node', graph.corner_node, torch.int32, (nf, 3), dev, what)
        g = _tensor('g', g, torch.float64, (graph.nodes, 3), dev, what)
        extra = (_vp(fmap), _vp(face_chart), _vp(screen), o, nf, _vp(corner), _vp(g), graph.nodes)
    ws = _workspace(workspace, nf, 0, dev, what)
    texture = torch.zeros(p.Ht, p.Wt, 3, dtype=torch.uint8, device=dev)
    valid = torch.zeros(p.Ht, p.Wt, dtype=torch.uint8, device=dev)
    check(lib().mvsdf_charts_fill(_vp(img), V, H, W, _vp(chart_view), _vp(p.chart_rect), _vp(p.order), _vp(p.xs), _vp(p.shelves), nc, ns, p.density, p.pad,
                                  fb[0], fb[1], fb[2], p.Ht, p.Wt, *extra, _vp(ws), ws.numel(), _vp(texture), _vp(valid), _stream(ws)), 'mvsdf_charts_fill')
    _raise(ws, what)
    return texture, valid


def chart_fill(images, chart_view, packing, fallback=(128, 128, 128), workspace=None):
    """step 6: (texture uint8 [Ht,Wt,3], valid uint8 [Ht,Wt]) from images uint8 [V,H,W,3]"""
    return _fill('chart_fill', images, chart_view, packing, fallback, workspace)


def levelled_chart_fill(images, chart_view, packing, face_map, face_chart, screen, graph, g, pixel_center=0.5, fallback=(128, 128, 128),
                        workspace=None):
    """step 7: the fill with seams.py's corrections g fp64 [K,3] of the SeamGraph `graph` of the same labels, through face_map"""
    from .seams import SeamGraph
    if not isinstance(graph, SeamGraph):
        raise ValueError('levelled_chart_fill: a SeamGraph is needed, got %s' % type(graph).__name__)
    return _fill('levelled_chart_fill', images, chart_view, packing, fallback, workspace, (face_map, face_chart, screen, graph, g, pixel_center))


def build_chart_atlas(mesh, images, P=None, cams=None, pixel_center=0.5, masks=None, raster=None, texel_density=1.0, max_size=8192,
                      fallback=(128, 128, 128), depth_tol=0.01, cos_min=0.0, ignore_normals=False, large_face_pixels=None, view_chunk=None, pad=4,
                      min_faces=4, smooth_rounds=2, level_seams=False, level_options=None, workspace=None, info=None):
    """The module's atlas of `mesh` from images uint8 [V,H,W,3] -> texture.TexturedMesh with uv, texture, valid, face_view (the smoothed labels),
    density, raster, score, screen and the new fields face_chart, chart_view, chart_rect, face_map (and packing); patch, order and counts are None.
    level_seams=True runs seams.py's graph, colours and solve on the smoothed labels and fills through the face map (level_options: smoothness,
    anchor, cg_iters, cg_tol, info).  info (a dict) receives the charts before and after the absorption and the changes of every round."""
    what = 'build_chart_atlas'
    if level_options is not None and not isinstance(level_options, dict):
        raise ValueError('%s: level_options must be a dict, got %s' % (what, type(level_options).__name__))
    pad = _pad(pad, what)
    R._mesh(mesh, what)
    dev = R._on_device(mesh, what)
    img, V, H, W = _images(images, dev, what)
    if raster is None:
        Pm = R._cameras(P, cams, what)
        o = R._center(pixel_center, what)
    else:
        if not isinstance(raster, R.Raster):
            raise ValueError('%s: raster must be a Raster, got %s' % (what, type(raster).__name__))
        Pm, o = raster.P, raster.pixel_center
        if tuple(raster.depth.shape) != (V, H, W):
            raise ValueError('%s: the raster is %s, the images %s' % (what, tuple(raster.depth.shape), (V, H, W)))
    if len(Pm) != V:
        raise ValueError('%s: %d cameras for %d images' % (what, len(Pm), V))
    R._masks(masks, V, H, W, what)
    d = _density(texel_density, what)
    max_size = _int('max_size', max_size, pad, T.MAX_SIZE, what)
    fb = _fallback(fallback, what)
    min_faces = _int('min_faces', min_faces, 1, 2 ** 31 - 1, what)
    smooth_rounds = _int('smooth_rounds', smooth_rounds, 0, 1024, what)
    nf = mesh.faces.shape[0]
    if nf > T.MAX_FACES:
        raise ValueError('%s: %d faces (at most 2^28)' % (what, nf))
    if raster is None:
        raster = R.rasterize(mesh, P=Pm, hw=(H, W), pixel_center=o, large_face_pixels=large_face_pixels, view_chunk=view_chunk)
    ws = _workspace(workspace, nf, 0, dev, what)
    view = dict(masks=masks, depth_tol=depth_tol, cos_min=cos_min, ignore_normals=ignore_normals)
    label, _ = T.face_views(mesh, raster, **view)
    nbr = face_neighbors(mesh, workspace=ws)
    if info is not None:
        info['charts_before'] = face_charts(label, nbr, workspace=ws)[1].shape[0]
    label, score, screen, changes = smooth_labels(mesh, raster, label, min_faces, smooth_rounds, nbr=nbr, workspace=ws, **view)
    face_chart, chart_view, chart_faces = face_charts(label, nbr, workspace=ws)
    nc = chart_view.shape[0]
    if info is not None:
        info.update(charts=nc, changes=changes)
    if nc == 0:
        texture = torch.tensor(fb, dtype=torch.uint8, device=dev).expand(pad, pad, 3).contiguous()
        t = T.TexturedMesh(mesh, torch.full((nf, 3, 2), 0.5 / pad, dtype=torch.float32, device=dev), texture,
                           torch.zeros(pad, pad, dtype=torch.uint8, device=dev), label, None, d, raster, score, screen, face_chart=face_chart,
                           chart_view=chart_view, chart_rect=torch.zeros(0, 6, dtype=torch.int32, device=dev),
                           face_map=torch.full((pad, pad), -1, dtype=torch.int32, device=dev))
        t.uv[:, :, 1] = 1.0 - 0.5 / pad
        return t
    p = pack_charts(face_chart, nc, screen, (H, W), o, d, max_size, pad, workspace=ws)
    uv = chart_uvs(face_chart, screen, p, o, workspace=ws)
    roomy = workspace is not None and workspace.numel() >= chart_workspace_bytes(nf, p.Ht * p.Wt)          # the face map needs a second map behind the rest
    fmap = face_map(face_chart, screen, p, o, workspace=ws if roomy else None)
    if level_seams:
        from . import seams
        opts = dict(level_options or {})
        linfo = opts.pop('info', None)
        graph = seams.seam_graph(mesh, label, views=V)
        f = seams.node_colors(graph, mesh, img, P=Pm, pixel_center=o)
        g, solve = seams.solve_levels(graph, f, **opts)
        if linfo is not None:
            linfo.update(solve, nodes=graph.nodes, nnz=graph.nnz)
        texture, valid = levelled_chart_fill(img, chart_view, p, fmap, face_chart, screen, graph, g, o, fb, workspace=ws)
    else:
        texture, valid = chart_fill(img, chart_view, p, fb, workspace=ws)
    t = T.TexturedMesh(mesh, uv, texture, valid, label, None, p.density, raster, score, screen, face_chart=face_chart, chart_view=chart_view,
                       chart_rect=p.chart_rect, face_map=fmap)
    t.packing, t.chart_faces = p, chart_faces
    if level_seams:
        t.levels, t.seam_graph = g, graph
    return t
