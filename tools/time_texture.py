"""Device time of the texture atlas stages (mvsdf_amd/texture.py, csrc/texture.hip): face labels, the class count pass, the packing and the
texel fill, each between two device events after a warm-up, the work ending in a synchronise; the median of --repeats runs, one JSON line.

The scene is synthetic and its size is stated in the output: mesh.sparse_marching_cubes of the synthetic model (--width) at --resolution,
simplified to --faces faces (Mesh.simplify), drawn into --views cameras on three rings around the origin at --hw pixels (pixel centres at +0.5),
textured from random images at --density texels per pixel.  The fill is timed twice within every repeat, alternating: reading the per-face table
of screen coordinates that the label pass wrote, and projecting the three corners again per texel (the A/B behind DESIGN.md's choice); the two
atlases are compared.  For the fill the bytes written (4 per texel: colour and valid) plus gathered (12 per valid texel: 2 x 2 pixels of 3
bytes) over its time are also given as a share of the 6.3e12 B/s that tools/time_poisson.py uses.  The count and pack stages include the read
of their header, which waits for the stream.  For the split by kernel run the script under rocprofv3 --kernel-trace --stats in a run of its
own (--repeats 1).

With --level_seams the stages of seam levelling (mvsdf_amd/seams.py) are timed in the same repeats: the graph build (it includes the read of its
header), the node colours, one A x, a whole solve (with its iteration counts) and the levelled fill, which stands next to the plain fill of the
same repeat.  One A x is also given in bytes moved (per adjacency entry 4 bytes of index and 24 of gathered x; per node 16 of offsets, 4 of the
seam count, 24 of x and 24 written) as a share of 6.3e12 B/s, and next to the same product by torch.sparse_csr's fp64 mat-vec on the same
graph, with the largest difference between the two.

With --charts the stages of the chart atlas (mvsdf_amd/charts.py) are timed in the same repeats on the same labels: the neighbours, the components,
the absorption (its score pass, and per round the components and one absorb pass; the reads of the headers included), the components of the
smoothed labels, the packing (every halving pass), the UVs, the chart fill, which stands next to the per-face fill of the same repeat with the
same byte model, and the face map.  Both atlases report their size and the share of their area that lies under a face (the sum of the UV
triangles' areas); the charts before and after the absorption are given.

    python tools/time_texture.py [--resolution 512 --faces 50000 --views 49 --hw 1200,1600 --density 1.0 --max_size 8192 --repeats 5]
                                 [--level_seams [--seam_smoothness 0.1 --cg_iters 200]] [--charts [--chart_pad 4 --min_chart_faces 4]]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))                       # time_raster's cameras

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_BYTES_PER_S = 6.3e12


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--resolution', type=int, default=512)
    ap.add_argument('--faces', type=int, default=50000, help='simplify the extracted mesh to at most this many faces (0: not at all)')
    ap.add_argument('--views', type=int, default=49)
    ap.add_argument('--hw', type=str, default='1200,1600')
    ap.add_argument('--density', type=float, default=1.0)
    ap.add_argument('--max_size', type=int, default=8192)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--width', type=int, default=256, help='hidden width of the synthetic model')
    ap.add_argument('--level_seams', default=False, action='store_true', help='also time the stages of seam levelling')
    ap.add_argument('--seam_smoothness', type=float, default=0.1)
    ap.add_argument('--cg_iters', type=int, default=200)
    ap.add_argument('--charts', default=False, action='store_true', help='also time the stages of the chart atlas')
    ap.add_argument('--chart_pad', type=int, default=4, choices=(1, 2, 4, 8))
    ap.add_argument('--min_chart_faces', type=int, default=4)
    return ap


def _events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def main(argv=None):
    a = parser().parse_args(argv)
    assert torch.cuda.is_available(), 'time_texture.py measures on the GPU'
    from time_raster import ring_cameras
    from mvsdf_amd import mesh as M
    from mvsdf_amd import raster as R
    from mvsdf_amd import texture as X
    from mvsdf_amd._lib import lib
    from mvsdf_amd.model.implicit_differentiable_renderer import IDRNetwork
    from mvsdf_amd.utils import synth
    from mvsdf_amd.utils.config import ConfigDict
    hw = tuple(int(v) for v in a.hw.split(','))
    m = IDRNetwork(ConfigDict(synth.model_conf(a.width)))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(a.width, 0).items()})
    m = m.cuda().eval()
    mesh = M.sparse_marching_cubes(m.implicit_network.native_sdf(), a.resolution, 0.0)
    extracted = len(mesh)
    if a.faces and a.faces < extracted:
        mesh = mesh.simplify(target_faces=a.faces)
    P = ring_cameras(a.views, hw)
    g = torch.Generator(device='cuda').manual_seed(0)
    images = torch.randint(0, 256, (a.views, hw[0], hw[1], 3), dtype=torch.uint8, device='cuda', generator=g)
    raster = R.rasterize(mesh, P=P, hw=hw)
    nf = len(mesh)
    ws = torch.empty(lib().mvsdf_texture_workspace_bytes(nf), dtype=torch.uint8, device='cuda')
    cls = torch.empty(nf, dtype=torch.uint8, device='cuda')
    v, f = mesh.vertices.contiguous(), mesh.faces.contiguous()
    Pd = torch.from_numpy(P).cuda()
    names = ('face_views_ms', 'count_pass_ms', 'pack_ms', 'fill_table_ms', 'fill_recompute_ms')
    runs = {k: [] for k in names}
    if a.level_seams:
        from mvsdf_amd import seams as SL
    lnames = ('seam_graph_ms', 'node_colors_ms', 'apply_ms', 'solve_ms', 'fill_levelled_ms', 'sparse_csr_ms')
    lruns = {k: [] for k in lnames}
    anchor = 1e-3
    passes = 0
    if a.charts:
        from mvsdf_amd import charts as CH
        cws, big = torch.zeros(CH.chart_workspace_bytes(nf, 0), dtype=torch.uint8, device='cuda'), None
    cnames = ('chart_neighbors_ms', 'chart_components_ms', 'chart_absorb_ms', 'chart_components_smoothed_ms', 'chart_pack_ms', 'chart_uv_ms',
              'chart_fill_ms', 'chart_face_map_ms')
    cruns = {k: [] for k in cnames}
    for rep in range(a.repeats + 1):                                  # the first round warms up
        ev = _events(6)
        ev[0].record()
        label, score, screen = X._face_views(mesh, raster, None, 0.01, 0.0, False, 'time_texture')
        ev[1].record()
        d, passes = a.density, 0
        while True:                                                   # build_atlas's loop; the event pair spans its last pass only
            ev[1].record()
            counts = X._classify(label, screen, d, ws, cls)
            passes += 1
            if X.atlas_size(counts)[0] <= a.max_size:
                break
            d = d / 2.0
        ev[2].record()
        order, patch, uv = X._pack(cls, counts, ws)
        ev[3].record()
        tex, valid = X._fill(images, 0.5, label, screen, order, counts, v, f, Pd, (128, 128, 128), False)
        ev[4].record()
        tex2, valid2 = X._fill(images, 0.5, label, screen, order, counts, v, f, Pd, (128, 128, 128), True)
        ev[5].record()
        torch.cuda.synchronize()
        assert torch.equal(tex, tex2) and torch.equal(valid, valid2)
        if rep:
            for k, name in enumerate(names):
                runs[name].append(ev[k].elapsed_time(ev[k + 1]))
        if a.level_seams:
            tm = X.TexturedMesh(mesh, uv, tex, valid, label, patch, d, raster, score, screen, order, [int(c) for c in counts])
            le = _events(7)
            le[0].record()
            graph = SL.seam_graph(mesh, label, views=a.views)
            le[1].record()
            fcol = SL.node_colors(graph, mesh, images, P=P)
            le[2].record()
            ax = SL.apply_operator(graph, fcol, a.seam_smoothness, anchor)
            le[3].record()
            gsol, sinfo = SL.solve_levels(graph, fcol, a.seam_smoothness, anchor, a.cg_iters)
            le[4].record()
            tex3, valid3 = SL.levelled_fill(tm, images, graph, gsol)
            if rep == 0:                                              # the yardstick's matrix, built once: A as torch.sparse_csr
                K = graph.nodes
                deg = (graph.adj_off[1:] - graph.adj_off[:-1])
                rows = torch.repeat_interleave(torch.arange(K, device='cuda'), deg)
                pos = torch.arange(graph.nnz, device='cuda') - graph.adj_off[:-1][rows]
                w = torch.where(pos < graph.adj_seam.long()[rows], 1.0, a.seam_smoothness).double()
                diag = torch.zeros(K, dtype=torch.float64, device='cuda').index_add_(0, rows, w) + anchor
                A = torch.sparse_coo_tensor(torch.stack([torch.cat([rows, torch.arange(K, device='cuda')]), torch.cat([graph.adj_node.long(), torch.arange(K, device='cuda')])]),
                                            torch.cat([-w, diag]), (K, K)).coalesce().to_sparse_csr()
            le[5].record()
            ax2 = A @ fcol
            le[6].record()
            torch.cuda.synchronize()
            assert torch.equal(valid3, valid)
            if rep:
                for k, name in enumerate(lnames):
                    lruns[name].append(le[k].elapsed_time(le[k + 1]))
        if a.charts:
            ce = _events(9)
            ce[0].record()
            nbr = CH.face_neighbors(mesh, workspace=cws)
            ce[1].record()
            before = CH.face_charts(label, nbr, workspace=cws)
            ce[2].record()
            lab2, sc2, scr2, changes = CH.smooth_labels(mesh, raster, label, a.min_chart_faces, 2, nbr=nbr, workspace=cws)
            ce[3].record()
            fc, cv, cf = CH.face_charts(lab2, nbr, workspace=cws)
            ce[4].record()
            pk = CH.pack_charts(fc, cv.shape[0], scr2, hw, 0.5, a.density, a.max_size, a.chart_pad, workspace=cws)
            ce[5].record()
            cuv = CH.chart_uvs(fc, scr2, pk, 0.5, workspace=cws)
            ce[6].record()
            ctex, cvalid = CH.chart_fill(images, cv, pk, workspace=cws)
            ce[7].record()
            if big is None:                                           # the face map's second map lies behind the rest of the workspace
                big = torch.zeros(CH.chart_workspace_bytes(nf, pk.Ht * pk.Wt), dtype=torch.uint8, device='cuda')
                torch.cuda.synchronize()
                ce[7].record()
            fmap = CH.face_map(fc, scr2, pk, 0.5, workspace=big)
            ce[8].record()
            torch.cuda.synchronize()
            if rep:
                for k, name in enumerate(cnames):
                    cruns[name].append(ce[k].elapsed_time(ce[k + 1]))
    med = lambda x: round(float(np.median(x)), 3)                     # noqa: E731
    Wt, Ht, T = X.atlas_size(counts)
    n_valid = int(valid.sum())
    nbytes = 4 * Wt * Ht + 12 * n_valid
    res = {'resolution': a.resolution, 'extracted_faces': extracted, 'faces': nf, 'views': a.views, 'hw': hw, 'repeats': a.repeats,
           'density_asked': a.density, 'density_used': d, 'count_passes': passes, 'class_counts': [int(c) for c in counts], 'atlas': [Wt, Ht],
           'blocks_used_fraction': round(T / ((Wt // 4) * (Ht // 4)), 4), 'labelled_fraction': round(float((label >= 0).float().mean()), 4),
           'valid_texels': n_valid, 'valid_fraction': round(n_valid / (Wt * Ht), 4), 'fill_bytes': nbytes}
    for name in names:
        res[name] = {'median': med(runs[name]), 'runs': [round(x, 3) for x in runs[name]]}
    for name in ('fill_table_ms', 'fill_recompute_ms'):
        rate = nbytes / (res[name]['median'] * 1e-3)
        res[name]['bytes_per_s'] = float('%.4g' % rate)
        res[name]['share_of_6.3e12'] = round(rate / PEAK_BYTES_PER_S, 4)
        res[name]['texels_per_s'] = float('%.4g' % (Wt * Ht / (res[name]['median'] * 1e-3)))
    def under(uvs):                                             # the share of a w x h atlas under a face: the UV triangles' areas
        q = uvs.double()
        e1, e2 = q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]
        return round(float((e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]).abs().sum()) / 2.0, 4)
    res['area_under_faces'] = under(uv[label >= 0])
    if a.charts:
        for name in cnames:
            res[name] = {'median': med(cruns[name]), 'runs': [round(x, 3) for x in cruns[name]]}
        cvalid_n = int(cvalid.sum())
        cbytes = 4 * pk.Wt * pk.Ht + 12 * cvalid_n
        rate = cbytes / (res['chart_fill_ms']['median'] * 1e-3)
        res['chart_fill_ms'].update({'bytes': cbytes, 'bytes_per_s': float('%.4g' % rate), 'share_of_6.3e12': round(rate / PEAK_BYTES_PER_S, 4),
                                     'texels_per_s': float('%.4g' % (pk.Wt * pk.Ht / (res['chart_fill_ms']['median'] * 1e-3)))})
        res.update({'chart_pad': a.chart_pad, 'min_chart_faces': a.min_chart_faces, 'charts_before': int(before[1].shape[0]), 'charts': int(cv.shape[0]),
                    'charts_below_min_before': int((before[2] < a.min_chart_faces).sum()), 'charts_below_min': int((cf < a.min_chart_faces).sum()),
                    'absorb_changes': changes, 'chart_atlas': [pk.Wt, pk.Ht], 'chart_density_used': pk.density, 'chart_valid_texels': cvalid_n,
                    'chart_valid_fraction': round(cvalid_n / (pk.Wt * pk.Ht), 4), 'chart_area_under_faces': under(cuv[fc >= 0]),
                    'chart_face_map_fraction': round(float((fmap >= 0).float().mean()), 4), 'largest_chart_faces': int(cf.max()) if cf.numel() else 0})
    if a.level_seams:
        K, nnz = graph.nodes, graph.nnz
        for name in lnames:
            res[name] = {'median': med(lruns[name]), 'runs': [round(x, 3) for x in lruns[name]]}
        abytes = 28 * nnz + 68 * K
        rate = abytes / (res['apply_ms']['median'] * 1e-3)
        res['apply_ms'].update({'bytes': abytes, 'bytes_per_s': float('%.4g' % rate), 'share_of_6.3e12': round(rate / PEAK_BYTES_PER_S, 4)})
        res['sparse_csr_ms']['max_abs_difference'] = float((ax - ax2).abs().max())
        res['sparse_csr_ms']['max_abs_value'] = float(ax.abs().max())
        res.update({'nodes': K, 'adjacency_entries': nnz, 'seam_nodes': int((graph.adj_seam > 0).sum()), 'cg_iterations': sinfo['iterations'],
                    'cg_rho': sinfo['rho'], 'cg_rho0': sinfo['rho0'], 'seam_smoothness': a.seam_smoothness, 'anchor': anchor,
                    'levelled_texels_changed': int((tex3 != tex).any(-1).sum())})
    print(json.dumps(res), flush=True)
    return res


if __name__ == '__main__':
    main()
