"""Seam levelling on the device: a texture atlas whose neighbouring faces took their texels from different photographs keeps each photograph's
exposure, white balance and vignetting, a patchwork along every label boundary.  Global seam levelling (in the sense of Lempitsky and Ivanov, and
of Waechter et al., "Let there be color") computes an additive colour correction g per (vertex, label) pair so that the corrected colours agree
where labels meet and vary smoothly inside a label's region; the texel fill then applies g with the barycentric weights it already has.
Kernels: csrc/seams.hip and the LEVEL flag of csrc/texture.hip's fill (the design: DESIGN.md); tests/seams_ref.py restates every step in numpy.
The reference has no texturing code; the definition below is this project's, written so that the schedule cannot change a bit of the result.

The definition (fp64 throughout, in the order written, no FMA contraction; only + - * /, comparisons and floor; fp32 and uint8 inputs are
promoted exactly; every integer decision is exact).  A sum "over the tree" is geom_prims.h's canonical pairwise sum: the terms are padded with
+0.0 to a power of two and adjacent pairs are added until one value is left.  The sign of a zero is not defined.

1. Nodes (seam_graph).  A node is a pair (vertex i, view v) such that some face with label v >= 0 has corner i.  The K nodes are listed by (i, v)
   ascending: node_vertex int32 [K], node_view int32 [K]; corner_node int32 [F,3] is the node of every face corner, -1 on unlabelled faces.
2. Node colours (node_colors).  f fp64 [K,3]: vertex i is projected into view v (raster.py's projection); u = sx - o and t = sy - o are clamped to
   [0, W-1] and [0, H-1] as the fill clamps them (a NaN becomes 0; a vertex that is not in front, !(z > 0), takes u = t = 0) and fusion's bilinear
   rule (raster.py) gives the colour per channel.
3. Graph.  Every node k has a list adj_node[adj_off[k] : adj_off[k+1]] (adj_off int64 [K+1], adj_node int32 [nnz]).  First its adj_seam[k] seam
   partners: the other nodes of the same vertex, ascending, each with weight 1.  Then its smoothness entries with weight `smoothness`: for every
   (face f, corner e), in (f, e) ascending order, such that corner_node[f, e] == k, the two entries corner_node[f, (e+1) % 3] and
   corner_node[f, (e+2) % 3], in this order.  An interior edge is counted once per incident face on purpose; nothing is de-duplicated.  (A face
   that repeats a vertex gives a node entries to itself: they add 0 to A x and their weight to the diagonal.)
4. Operator and right-hand side, per colour channel.  (A x)_k = anchor * x_k + S, S the sum from 0.0, in list order, of w * (x_k - x_nb).
   b_k = the sum from 0.0 over the seam partners, in list order, of (f_nb - f_k).  d_k = anchor + s, s the sum from 0.0, in list order, of w.
   A is symmetric; it is positive definite for anchor > 0, so no gauge is left over.  d is A's diagonal (for faces without a repeated vertex).
5. Solve (solve_levels): conjugate gradients preconditioned by d, the three channels side by side, each with its own scalars.  x = 0, r = b,
   z = r / d, p = z, rho = rho_0 = the tree over k of r_k * z_k; the channel is done at once unless rho_0 is finite and > 0.  An iteration of a
   channel that is not done: q = A p; sigma = the tree of p_k * q_k; unless sigma is finite and > 0 the channel is done and nothing else
   happens (the iteration is not counted); alpha = rho / sigma; x = x + alpha * p; r = r - alpha * q; z = r / d; rho' = the tree of r_k * z_k;
   beta = rho' / rho; p = z + beta * p; rho = rho'; the iteration is counted; the channel is done unless rho' > cg_tol^2 * rho_0 (which also
   catches NaN).  At most cg_iters iterations.  g = x.  The result reports the iterations, the final rho and rho_0 per channel.
6. Levelled fill (level_atlas).  Step 5 of texture.py's definition up to its unrounded colour c; then per channel
   c' = c + ((alpha * g_a + beta * g_b) + gamma * g_c) with the g of the face's three nodes (alpha, beta, gamma the texel's weights, which
   extrapolate in the gutter as the source position does); c' is clamped to [0, 255] (a NaN becomes 0) and the texel is uint8(floor(c' + 0.5)).
   valid, fallback texels, UVs, patches and the atlas size are untouched.  With g = 0 the texture equals build_atlas's byte for byte.

Nothing here allocates uninitialised memory: outputs and workspaces come from torch.zeros / torch.full (DESIGN.md names the cost), and every
stage takes an optional workspace= byte tensor (seam_workspace_bytes) whose contents it does not rely on.

Argument errors (wrong dtypes or shapes, arrays on another device, smoothness < 0, anchor <= 0, cg_iters outside [0, 100000], cg_tol < 0, a
non-finite number) raise ValueError before anything is launched; nothing is converted silently.  A mesh on the CPU raises MvsdfError.  What the
device finds (ERRORS) raises ValueError after the call.
"""
import ctypes

import numpy as np
import torch

from . import raster as R
from ._lib import check, lib, K, raise_for_bits, _header, _stream, _vp, f64_from_bits

MAX_CG = K.MVSDF_SL_MAX_CG
CLASSES = 7

# the error bits of a seam-levelling call (csrc/seams.hip), in the order they are looked at
ERRORS = [(K.MVSDF_TX_ERR_FINITE, ValueError, 'a camera entry or a vertex is NaN or infinite'),
          (K.MVSDF_TX_ERR_INDEX, ValueError, 'an index (face -> vertex, corner -> node, adjacency -> node) is out of range'),
          (K.MVSDF_TX_ERR_LABEL, ValueError, 'a face label is outside [-1, V)'),
          (K.MVSDF_TX_ERR_COUNTS, ValueError, 'the workspace is not the one the node pass left')]


class SeamGraph:
    """The result of seam_graph, all on the device: node_vertex int32 [K], node_view int32 [K], corner_node int32 [F,3], adj_off int64 [K+1],
    adj_seam int32 [K], adj_node int32 [nnz]; views, the number of views the labels were checked against."""

    def __init__(self, node_vertex, node_view, corner_node, adj_off, adj_seam, adj_node, views):
        self.node_vertex, self.node_view, self.corner_node = node_vertex, node_view, corner_node
        self.adj_off, self.adj_seam, self.adj_node, self.views = adj_off, adj_seam, adj_node, views

    @property
    def nodes(self):
        return self.node_vertex.shape[0]

    @property
    def nnz(self):
        return self.adj_node.shape[0]


def seam_workspace_bytes(faces=0, vertices=0, views=1, nodes=0):
    """bytes of a workspace= that serves seam_graph on a mesh of that size and the other stages on `nodes` nodes"""
    size = lib().mvsdf_seams_workspace_bytes(int(faces), int(vertices), int(views), int(nodes))
    if size == 0:
        raise ValueError('seam_workspace_bytes: %d faces, %d vertices, %d views, %d nodes are beyond the limits' % (faces, vertices, views, nodes))
    return size


def _workspace(workspace, size, dev, what):
    """the caller's byte tensor, checked, or a zeroed one"""
    if workspace is None:
        return torch.zeros(size, dtype=torch.uint8, device=dev)
    if not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.dim() != 1 or not workspace.is_contiguous():
        raise ValueError('%s: workspace must be a contiguous uint8 vector' % what)
    if workspace.device != dev:
        raise ValueError('%s: the workspace is on %s, the data on %s' % (what, workspace.device, dev))
    if workspace.numel() < size:
        raise ValueError('%s: the workspace holds %d bytes, %d are needed (seam_workspace_bytes)' % (what, workspace.numel(), size))
    if workspace.data_ptr() % 256:
        raise ValueError('%s: the workspace must be 256-byte aligned' % what)
    return workspace


def _tensor(name, x, dtype, shape, dev, what):
    """x as it is, if it is a contiguous tensor of that dtype, shape (None: any length) and device"""
    if not isinstance(x, torch.Tensor) or x.dtype != dtype:
        raise ValueError('%s: %s must be a %s tensor, got %s' % (what, name, dtype, x.dtype if isinstance(x, torch.Tensor) else type(x).__name__))
    if x.dim() != len(shape) or any(s is not None and s != n for s, n in zip(shape, x.shape)):
        raise ValueError('%s: %s must be %s, got %s' % (what, name, list(shape), tuple(x.shape)))
    if x.device != dev:
        raise ValueError('%s: %s is on %s, not on %s' % (what, name, x.device, dev))
    if not x.is_contiguous():
        raise ValueError('%s: %s must be contiguous' % (what, name))
    return x


def _number(name, x, what, lo=None, strict=False):
    try:
        v = float(x)
    except (TypeError, ValueError):
        raise ValueError('%s: %s must be a number, got %r' % (what, name, x)) from None
    if not np.isfinite(v) or (lo is not None and (v <= lo if strict else v < lo)):
        raise ValueError('%s: %s must be finite and %s %g, got %r' % (what, name, '>' if strict else '>=', lo if lo is not None else 0.0, x))
    return v


def _graph(graph, what):
    if not isinstance(graph, SeamGraph):
        raise ValueError('%s: a SeamGraph is needed, got %s' % (what, type(graph).__name__))
    dev = graph.node_vertex.device
    k = graph.node_vertex.shape[0] if graph.node_vertex.dim() == 1 else None
    _tensor('node_vertex', graph.node_vertex, torch.int32, (None,), dev, what)
    _tensor('node_view', graph.node_view, torch.int32, (k,), dev, what)
    _tensor('corner_node', graph.corner_node, torch.int32, (None, 3), dev, what)
    _tensor('adj_off', graph.adj_off, torch.int64, (k + 1,), dev, what)
    _tensor('adj_seam', graph.adj_seam, torch.int32, (k,), dev, what)
    _tensor('adj_node', graph.adj_node, torch.int32, (None,), dev, what)
    if not dev.type == 'cuda':
        raise ValueError('%s: the graph must be on the GPU' % what)
    return dev


def _raise(ws, what):
    raise_for_bits(_header(ws, K.MVSDF_SL_H_WORDS)[K.MVSDF_SL_H_ERR], what, ERRORS)


def seam_graph(mesh, face_view, views=None, workspace=None):
    """steps 1 and 3 of the module's definition for `mesh` with the labels face_view int32 [F] (-1: no view) -> SeamGraph.  views: the number of
    views V the labels index (None: the most a call takes); a label outside [-1, V) is refused."""
    what = 'seam_graph'
    R._mesh(mesh, what, faces=False)
    dev = R._on_device(mesh, what)
    nv, nf = mesh.vertices.shape[0], mesh.faces.shape[0]
    label = _tensor('face_view', face_view, torch.int32, (nf,), dev, what)
    if views is None:
        views = R.MAX_VIEWS
    if isinstance(views, (bool, np.bool_)) or not isinstance(views, (int, np.integer)) or not 1 <= views <= R.MAX_VIEWS:
        raise ValueError('%s: views must be an int in [1, %d], got %r' % (what, R.MAX_VIEWS, views))
    views = int(views)
    faces = _tensor('faces', mesh.faces, torch.int32, (nf, 3), dev, what)
    size = lib().mvsdf_seams_workspace_bytes(nf, nv, views, 0)
    if size == 0:
        raise ValueError('%s: %d faces (at most 2^28)' % (what, nf))
    ws = _workspace(workspace, size, dev, what)
    corner_node = torch.full((nf, 3), -1, dtype=torch.int32, device=dev)
    check(lib().mvsdf_seams_nodes(_vp(faces), _vp(label), nv, nf, views, _vp(ws), ws.numel(), _vp(corner_node), _stream(ws)), 'mvsdf_seams_nodes')
    hdr = _header(ws, K.MVSDF_SL_H_WORDS)
    raise_for_bits(hdr[K.MVSDF_SL_H_ERR], what, ERRORS)
    k, nnz = hdr[K.MVSDF_SL_H_NODES], hdr[K.MVSDF_SL_H_NNZ]
    node_vertex = torch.zeros(k, dtype=torch.int32, device=dev)
    node_view = torch.zeros(k, dtype=torch.int32, device=dev)
    adj_off = torch.zeros(k + 1, dtype=torch.int64, device=dev)
    adj_seam = torch.zeros(k, dtype=torch.int32, device=dev)
    adj_node = torch.zeros(nnz, dtype=torch.int32, device=dev)
    check(lib().mvsdf_seams_graph(nv, nf, views, k, nnz, _vp(corner_node), _vp(ws), ws.numel(), _vp(node_vertex), _vp(node_view), _vp(adj_off),
                                  _vp(adj_seam), _vp(adj_node), _stream(ws)), 'mvsdf_seams_graph')
    _raise(ws, what)
    return SeamGraph(node_vertex, node_view, corner_node, adj_off, adj_seam, adj_node, views)


def _images(images, dev, what):
    """images uint8 [V,H,W,3], moved to the device if they are not there -> (tensor, V, H, W)"""
    img = torch.as_tensor(images)
    if img.dim() != 4 or img.shape[3] != 3 or img.dtype != torch.uint8:
        raise ValueError('%s: images must be uint8 [V, H, W, 3], got %s %s' % (what, img.dtype, tuple(img.shape)))
    V, H, W = img.shape[:3]
    H, W = R._hw((H, W), what)
    return img.to(dev).contiguous(), V, H, W


def node_colors(graph, mesh, images, P=None, pixel_center=0.5, cams=None, workspace=None):
    """step 2: f fp64 [K,3], the colour of every node's vertex in its view (images uint8 [V,H,W,3], P [V,4,4] or cams [V,2,4,4])"""
    what = 'node_colors'
    dev = _graph(graph, what)
    R._mesh(mesh, what, faces=False)
    if R._on_device(mesh, what) != dev:
        raise ValueError('%s: the mesh is on %s, the graph on %s' % (what, mesh.vertices.device, dev))
    img, V, H, W = _images(images, dev, what)
    Pm = R._cameras(P, cams, what)
    o = R._center(pixel_center, what)
    if len(Pm) != V:
        raise ValueError('%s: %d cameras for %d images' % (what, len(Pm), V))
    ws = _workspace(workspace, lib().mvsdf_seams_workspace_bytes(0, 0, 1, 0), dev, what)
    k = graph.nodes
    f = torch.zeros(k, 3, dtype=torch.float64, device=dev)
    v = mesh.vertices.contiguous()
    Pd = torch.from_numpy(Pm).to(dev)
    check(lib().mvsdf_seams_colors(_vp(graph.node_vertex), _vp(graph.node_view), k, _vp(v), v.shape[0], _vp(Pd), V, H, W, o, _vp(img), _vp(ws),
                                   ws.numel(), _vp(f), _stream(ws)), 'mvsdf_seams_colors')
    _raise(ws, what)
    return f


def apply_operator(graph, x, smoothness, anchor, workspace=None):
    """step 4: A x for x fp64 [K,3] -> fp64 [K,3]"""
    what = 'apply_operator'
    dev = _graph(graph, what)
    k = graph.nodes
    x = _tensor('x', x, torch.float64, (k, 3), dev, what)
    lam, anc = _number('smoothness', smoothness, what, 0.0), _number('anchor', anchor, what, 0.0, strict=True)
    ws = _workspace(workspace, lib().mvsdf_seams_workspace_bytes(0, 0, 1, 0), dev, what)
    out = torch.zeros(k, 3, dtype=torch.float64, device=dev)
    check(lib().mvsdf_seams_apply(_vp(graph.adj_off), _vp(graph.adj_seam), _vp(graph.adj_node), k, graph.nnz, _vp(x), lam, anc, _vp(ws), ws.numel(),
                                  _vp(out), _stream(ws)), 'mvsdf_seams_apply')
    _raise(ws, what)
    return out


def solve_levels(graph, f, smoothness=0.1, anchor=1e-3, cg_iters=200, cg_tol=1e-6, workspace=None):
    """step 5 for the node colours f fp64 [K,3] -> (g fp64 [K,3], dict(iterations, rho, rho0: three values each, one per colour channel)).  The
    whole solve is enqueued without a wait; the header is the one read."""
    what = 'solve_levels'
    dev = _graph(graph, what)
    k = graph.nodes
    f = _tensor('f', f, torch.float64, (k, 3), dev, what)
    lam, anc = _number('smoothness', smoothness, what, 0.0), _number('anchor', anchor, what, 0.0, strict=True)
    tol = _number('cg_tol', cg_tol, what, 0.0)
    if isinstance(cg_iters, (bool, np.bool_)) or not isinstance(cg_iters, (int, np.integer)) or not 0 <= cg_iters <= MAX_CG:
        raise ValueError('%s: cg_iters must be an int in [0, %d], got %r' % (what, MAX_CG, cg_iters))
    ws = _workspace(workspace, lib().mvsdf_seams_workspace_bytes(0, 0, 1, k), dev, what)
    g = torch.zeros(k, 3, dtype=torch.float64, device=dev)
    check(lib().mvsdf_seams_solve(_vp(graph.adj_off), _vp(graph.adj_seam), _vp(graph.adj_node), k, graph.nnz, _vp(f), lam, anc, int(cg_iters), tol,
                                  _vp(ws), ws.numel(), _vp(g), _stream(ws)), 'mvsdf_seams_solve')
    hdr = _header(ws, K.MVSDF_SL_H_WORDS)
    raise_for_bits(hdr[K.MVSDF_SL_H_ERR], what, ERRORS)
    info = dict(iterations=[hdr[K.MVSDF_SL_H_ITERS + c] for c in range(3)], rho=[f64_from_bits(hdr[K.MVSDF_SL_H_RHO + c]) for c in range(3)],
                rho0=[f64_from_bits(hdr[K.MVSDF_SL_H_RHO0 + c]) for c in range(3)])
    return g, info


def levelled_fill(textured_mesh, images, graph, g, pixel_center=0.5, fallback=(128, 128, 128), workspace=None):
    """step 6 -> (texture uint8 [Ht,Wt,3], valid uint8 [Ht,Wt]) for a TexturedMesh of build_atlas (which carries the screen table, the face order and
    the class counts of its fill), the graph of its labels and the corrections g fp64 [K,3]"""
    from . import texture as T
    what = 'levelled_fill'
    tm = textured_mesh
    if not isinstance(tm, T.TexturedMesh) or tm.screen is None or tm.order is None or tm.counts is None:
        raise ValueError('%s: a TexturedMesh of build_atlas is needed (with its screen table, order and counts)' % what)
    dev = _graph(graph, what)
    nf = tm.face_view.shape[0]
    label = _tensor('face_view', tm.face_view, torch.int32, (nf,), dev, what)
    screen = _tensor('screen', tm.screen, torch.float64, (nf, 6), dev, what)
    order = _tensor('order', tm.order, torch.int32, (nf,), dev, what)
    corner = _tensor('corner_node', graph.corner_node, torch.int32, (nf, 3), dev, what)
    g = _tensor('g', g, torch.float64, (graph.nodes, 3), dev, what)
    img, V, H, W = _images(images, dev, what)
    o = R._center(pixel_center, what)
    fb = np.asarray(fallback)
    if fb.shape != (3,) or not np.issubdtype(fb.dtype, np.integer) or fb.min() < 0 or fb.max() > 255:
        raise ValueError('%s: fallback must be three ints in 0 .. 255, got %r' % (what, fallback))
    counts = [int(c) for c in tm.counts]
    Wt, Ht, _ = T.atlas_size(counts)
    if len(counts) != CLASSES or tuple(tm.texture.shape) != (Ht, Wt, 3):
        raise ValueError('%s: the class counts do not give the atlas of this TexturedMesh' % what)
    ws = _workspace(workspace, lib().mvsdf_seams_workspace_bytes(0, 0, 1, 0), dev, what)
    carr = (ctypes.c_int64 * CLASSES)(*counts)
    texture = torch.zeros(Ht, Wt, 3, dtype=torch.uint8, device=dev)
    valid = torch.zeros(Ht, Wt, dtype=torch.uint8, device=dev)
    check(lib().mvsdf_seams_fill(_vp(img), V, H, W, o, _vp(label), _vp(screen), _vp(order), nf, carr, _vp(corner), _vp(g), graph.nodes, int(fb[0]),
                                 int(fb[1]), int(fb[2]), _vp(ws), ws.numel(), Ht, Wt, _vp(texture), _vp(valid), _stream(ws)), 'mvsdf_seams_fill')
    _raise(ws, what)
    return texture, valid


def level_atlas(textured_mesh, images, P=None, cams=None, pixel_center=None, smoothness=0.1, anchor=1e-3, cg_iters=200, cg_tol=1e-6,
                fallback=(128, 128, 128), workspace=None, info=None):
    """The whole of the definition for a TexturedMesh of build_atlas and the images it was built from -> a TexturedMesh with the corrected texture
    and the same UVs, patches, labels and valid.  Cameras and pixel_center default to those of the TexturedMesh's raster.  info (a dict) receives
    the solve's iterations, rho and rho0 and the graph's nodes and nnz."""
    from . import texture as T
    what = 'level_atlas'
    tm = textured_mesh
    if not isinstance(tm, T.TexturedMesh):
        raise ValueError('%s: a TexturedMesh is needed, got %s' % (what, type(tm).__name__))
    if P is None and cams is None:
        if tm.raster is None:
            raise ValueError('%s: give P or cams (the TexturedMesh carries no raster)' % what)
        P = tm.raster.P
    if pixel_center is None:
        pixel_center = tm.raster.pixel_center if tm.raster is not None else 0.5
    Pm = R._cameras(P, cams, what)
    dev = R._on_device(tm.mesh, what)
    img, V, H, W = _images(images, dev, what)
    if len(Pm) != V:
        raise ValueError('%s: %d cameras for %d images' % (what, len(Pm), V))
    graph = seam_graph(tm.mesh, tm.face_view, views=V, workspace=workspace)
    f = node_colors(graph, tm.mesh, img, P=Pm, pixel_center=pixel_center, workspace=workspace)
    g, solve = solve_levels(graph, f, smoothness, anchor, cg_iters, cg_tol, workspace=workspace)
    texture, valid = levelled_fill(tm, img, graph, g, pixel_center, fallback, workspace=workspace)
    if info is not None:
        info.update(solve, nodes=graph.nodes, nnz=graph.nnz)
    out = T.TexturedMesh(tm.mesh, tm.uv, texture, valid, tm.face_view, tm.patch, tm.density, tm.raster, tm.score, tm.screen, tm.order, tm.counts)
    out.levels, out.seam_graph = g, graph
    return out
