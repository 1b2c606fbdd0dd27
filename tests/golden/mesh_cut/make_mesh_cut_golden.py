#!/usr/bin/env python3
"""Generate the mesh-trimming fixtures tests/golden/mesh_cut/*.npz (tests/test_mesh_cut_host.py, tests/test_gpu_mesh_cut.py).

Meshes come from tests/mc_ref.py (marching cubes in numpy) over seeded volumes; vertex colours are (1 - s, s, 0) with s the sigmoid of a smooth
random field, like surface_mesh's.  Each fixture stores the mesh, thresh and smooth, and
  * ref_mask: the faces the reference's mesh_cut_ext (code/mesh_cut, IBFS) removes for the network mesh_cut.py assembles;
  * s_star, flow: S* and the maximum-flow value from scipy.sparse.csgraph.maximum_flow (checked against tests/maxflow_ref.py's Dinic).
The reference extension is compiled into a temporary directory (g++ and the pybind11 headers), so this runs only where the reference sources are;
nothing of them is written here.

    python tests/golden/mesh_cut/make_mesh_cut_golden.py [--ref-dir DIR]     # DIR: the reference's code/mesh_cut (default: $MVSDF_REFERENCE/code/mesh_cut)
"""
import argparse
import importlib
import os
import subprocess
import sys
import sysconfig
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..'))
import maxflow_ref  # noqa: E402
import mc_ref  # noqa: E402


def compile_reference(ref_dir, out_dir):
    import pybind11
    suffix = sysconfig.get_config_var('EXT_SUFFIX')
    so = os.path.join(out_dir, 'mesh_cut_ext' + suffix)
    subprocess.check_call(['g++', '-O2', '-shared', '-fPIC', '-std=c++14', '-I' + pybind11.get_include(), '-I' + sysconfig.get_paths()['include'],
                           '-I' + ref_dir, os.path.join(ref_dir, 'mesh_cut_ext.cpp'), os.path.join(ref_dir, 'IBFS', 'ibfs.cpp'), '-o', so])
    sys.path.insert(0, out_dir)
    return importlib.import_module('mesh_cut_ext')


def field(rs, n_terms=6, freq=0.35):
    """a smooth random scalar field: a sum of sinusoids"""
    k = rs.randn(n_terms, 3) * freq
    ph = rs.uniform(0, 2 * np.pi, n_terms)
    amp = rs.uniform(0.5, 1.0, n_terms)
    return lambda p: (amp * np.sin(p.astype(np.float64) @ k.T + ph)).sum(1)


def colours(rs, verts, bias, scale):
    f = field(rs)
    s = (1.0 / (1.0 + np.exp(-(bias + scale * f(verts))))).astype(np.float32)
    return np.stack([np.float32(1) - s, s, np.zeros_like(s)], 1).astype(np.float32)


def blobs(shape, centres, radii):
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float32) for n in shape], indexing='ij'))
    d = [np.sqrt(((g - np.asarray(c, np.float32)[:, None, None, None]) ** 2).sum(0)) - r for c, r in zip(centres, radii)]
    return np.min(d, axis=0).astype(np.float32)


def bumpy_sphere(rs, n, r, amp):
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float32)] * 3, indexing='ij'))
    c = (n - 1) / 2.0
    f = field(rs, freq=0.3)
    pts = g.reshape(3, -1).T
    return (np.sqrt(((g - c) ** 2).sum(0)) - r + amp * f(pts).reshape(g.shape[1:])).astype(np.float32)


def cases():
    rs = np.random.RandomState(20261015)
    sph = bumpy_sphere(rs, 28, 10.0, 1.0)
    v, f, n = mc_ref.marching_cubes(sph)
    c = colours(rs, v, 2.0, 2.5)
    yield 'default', v, f, n, c, 15, 10
    yield 'smooth1', v, f, n, c, 15, 1
    yield 'smooth2', v, f, n, c, 15, 2
    big = bumpy_sphere(rs, 40, 15.0, 1.5)
    v, f, n = mc_ref.marching_cubes(big)
    yield 'big_smooth1', v, f, n, colours(rs, v, 1.5, 3.0), 15, 1
    # the surface leaves the grid: an open sheet with a boundary
    g = np.stack(np.meshgrid(*[np.arange(24, dtype=np.float32)] * 3, indexing='ij'))
    fs = field(rs, freq=0.25)
    sheet = (g[2] - 11.5 + 2.0 * fs(g.reshape(3, -1).T).reshape(g.shape[1:])).astype(np.float32)
    v, f, n = mc_ref.marching_cubes(sheet)
    yield 'open', v, f, n, colours(rs, v, 2.0, 3.0), 15, 2
    vol = blobs((30, 30, 30), [(7, 7, 7), (21, 20, 8), (14, 15, 22)], [4.5, 5.5, 6.0])
    v, f, n = mc_ref.marching_cubes(vol)
    yield 'components', v, f, n, colours(rs, v, 1.5, 3.0), 15, 2
    v, f, n = mc_ref.marching_cubes(sph)
    c = colours(rs, v, 2.0, 2.5)
    yield 'nothing', v, f, n, c, 255, 10                          # c_f <= 1: no bright face, nothing removed
    yield 'everything', v, f, n, np.maximum(c, np.float32(0.2)), 0, 10    # every red > 0: every face bright, all removed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref-dir', default=os.path.join(os.environ.get('MVSDF_REFERENCE', ''), 'code', 'mesh_cut'))
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        ext = compile_reference(os.path.abspath(args.ref_dir), tmp)
        free_seen = False
        for name, v, f, n, c, thresh, smooth in cases():
            bright, pairs = maxflow_ref.graph(f, c, thresh, smooth)
            edges = np.concatenate([pairs, np.full((len(pairs), 1), smooth)], 1).astype(np.uint32)
            ref = np.asarray(ext.mesh_cut(bright, edges), dtype=bool)
            flow, s_star = maxflow_ref.scipy_max_flow(f, c, thresh, smooth)
            flow_d, s_d = maxflow_ref.max_flow(f, c, thresh, smooth)
            assert flow == flow_d and np.array_equal(s_star, s_d), name
            assert maxflow_ref.cut_capacity(s_star, f, c, thresh, smooth) == flow, name
            assert not (ref & ~s_star).any(), name
            free = int((s_star & ~ref).sum())
            free_seen |= free > 0
            print('%-12s F %5d  bright %5d  flow %5d  S* %5d  ref %5d  cut(ref) %d' % (name, len(f), bright.sum(), flow, s_star.sum(), ref.sum(),
                                                                                     maxflow_ref.cut_capacity(ref, f, c, thresh, smooth)))
            np.savez_compressed(os.path.join(HERE, name + '.npz'), vertices=v, faces=f, normals=n, colors=c, thresh=np.int64(thresh),
                                smooth=np.int64(smooth), ref_mask=ref, s_star=s_star, flow=np.int64(flow))
        assert free_seen, 'no case where the reference leaves free faces'


if __name__ == '__main__':
    main()
