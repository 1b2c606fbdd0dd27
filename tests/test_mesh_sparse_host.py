"""The sparse mesh extractor's contract on the host (mvsdf_amd/mesh.py sparse_marching_cubes, restated in tests/smc_ref.py): the kept faces are a
union of whole components of the dense mesh, a large margin keeps all of them, the closure matches a block-by-block statement of it, the
workspace queries refuse what the kernels cannot do, and the eval command's new flags."""
import numpy as np
import pytest

import mc_ref
import smc_ref


def _smooth_field(rs, n, modes=6):
    """a random smooth field: a sum of a few low-frequency cosines, sampled on the [-1, 1]^3 lattice (fp32)"""
    x, _ = smc_ref.lattice(n)
    X, Y, Z = np.meshgrid(x.astype(np.float64), x, x, indexing='ij')
    f = np.full(X.shape, rs.uniform(-0.3, 0.3))
    for _ in range(modes):
        k = rs.uniform(-4, 4, 3)
        f += rs.uniform(0.1, 0.5) * np.cos(k[0] * X + k[1] * Y + k[2] * Z + rs.uniform(0, 2 * np.pi))
    return f.astype(np.float32)


def _spheres(n, spheres):
    x, h = smc_ref.lattice(n)
    X, Y, Z = np.meshgrid(x.astype(np.float64), x, x, indexing='ij')
    d = np.min([np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - r for c, r in spheres], axis=0)
    return d.astype(np.float32), h


def _check_union_of_components(vol, B, margin, h):
    x, _ = smc_ref.lattice(vol.shape[0])
    v, f, nrm = mc_ref.marching_cubes(vol, 0.0, (h,) * 3, (x[0],) * 3)
    sv, sf, sn, info = smc_ref.sparse_marching_cubes(vol, B, 0.0, margin, h, (h,) * 3, (x[0],) * 3)
    if len(f) == 0:
        assert len(sf) == 0
        return info, 0, 0
    labels, count = mc_ref.components(f, len(v))
    keep = smc_ref.active_faces(vol, B, 0.0, info['active'])
    kept_labels = np.unique(labels[keep])
    assert np.array_equal(keep, np.isin(labels, kept_labels)), 'a component is cut by the active blocks'
    # every component with a face in a seed block is kept
    seeds = smc_ref.seed_blocks(vol, B, 0.0, margin, h)
    seeded = smc_ref.active_faces(vol, B, 0.0, seeds)
    assert np.isin(np.unique(labels[seeded]), kept_labels).all()
    wv, wf, wn = smc_ref.select_faces(v, f, nrm, keep)
    assert np.array_equal(sv, wv) and np.array_equal(sf, wf) and np.array_equal(sn, wn)
    return info, len(kept_labels), count


@pytest.mark.parametrize('seed', range(6))
def test_random_smooth_fields_keep_whole_components(seed):
    rs = np.random.RandomState(seed)
    n = [17, 24, 33, 40, 29, 33][seed]
    vol = _smooth_field(rs, n)
    _, h = smc_ref.lattice(n)
    for B in (2, 3, 5, 8):
        for margin in (0.0, 0.3, 1.0):
            _check_union_of_components(vol, B, margin, h)


@pytest.mark.parametrize('n,B', [(33, 4), (40, 8), (57, 16), (24, 5)])
def test_large_margin_keeps_the_dense_mesh(n, B):
    vol, h = _spheres(n, [((-0.4, 0.1, 0.0), 0.3), ((0.35, -0.2, 0.25), 0.25), ((0.1, 0.5, -0.5), 0.03 + 0.3 * B * 2.0 / (n - 1))])
    x, _ = smc_ref.lattice(n)
    v, f, nrm = mc_ref.marching_cubes(vol, 0.0, (h,) * 3, (x[0],) * 3)
    sv, sf, sn, info = smc_ref.sparse_marching_cubes(vol, B, 0.0, 1.0, h, (h,) * 3, (x[0],) * 3)
    assert np.array_equal(sv, v) and np.array_equal(sf, f) and np.array_equal(sn, nrm)


def test_tiny_sphere_is_missed_without_margin():
    n, B = 65, 8
    x, h = smc_ref.lattice(n)
    c = float(x[6 * B + B // 2]) + 0.3 * h                              # inside block 6, away from its corners
    vol, _ = _spheres(n, [((-0.2, 0.0, 0.1), 0.45), ((c, c, c), 0.3 * B * h)])
    info, kept, count = _check_union_of_components(vol, B, 0.0, h)
    assert count == 2 and kept == 1
    info, kept, count = _check_union_of_components(vol, B, 1.0, h)
    assert count == 2 and kept == 2


def _closure_by_blocks(seeds, vol, B):
    """the closure block by block, face by face, edge by edge (the statement smc_ref.closure vectorises)"""
    n = vol.shape[0]
    nb = smc_ref.blocks(n, B)
    inside = vol < 0
    active = seeds.copy()

    def rng(b):
        return b * B, min((b + 1) * B, n - 1)
    changed = True
    while changed:
        changed = False
        for b in zip(*np.nonzero(active)):
            for d in range(3):
                for s in (-1, 1):
                    nbr = list(b)
                    nbr[d] += s
                    if not 0 <= nbr[d] < nb or active[tuple(nbr)]:
                        continue
                    u, w = [a for a in range(3) if a != d]
                    plane = rng(b[d])[1] if s > 0 else rng(b[d])[0]
                    (lu, hu), (lw, hw) = rng(b[u]), rng(b[w])
                    hit = False
                    for pu in range(lu, hu + 1):
                        for pw in range(lw, hw + 1):
                            p = [0, 0, 0]
                            p[d], p[u], p[w] = plane, pu, pw
                            for a, lim in ((u, hu), (w, hw)):
                                if p[a] < lim:
                                    q = list(p)
                                    q[a] += 1
                                    hit |= inside[tuple(p)] != inside[tuple(q)]
                    if hit:
                        active[tuple(nbr)] = True
                        changed = True
    return active


@pytest.mark.parametrize('n,B,seed', [(17, 4, 0), (22, 3, 1), (26, 8, 2), (19, 2, 3)])
def test_closure_matches_the_block_by_block_statement(n, B, seed):
    vol = _smooth_field(np.random.RandomState(10 + seed), n, modes=8)
    _, h = smc_ref.lattice(n)
    seeds = smc_ref.seed_blocks(vol, B, 0.0, 0.0, h)
    active, _ = smc_ref.closure(seeds, vol, B, 0.0)
    assert np.array_equal(active, _closure_by_blocks(seeds, vol, B))


def test_closure_grows_a_grazed_block():
    """the GPU test's closure case: margin 0, B = 16, a sphere grazing blocks whose corners all lie outside it"""
    vol, h = smc_ref.grazing_sphere_volume()
    seeds = smc_ref.seed_blocks(vol, 16, 0.0, 0.0, h)
    active, rounds = smc_ref.closure(seeds, vol, 16, 0.0)
    assert active.sum() > seeds.sum() and rounds >= 2
    x, _ = smc_ref.lattice(vol.shape[0])
    v, f, nrm = mc_ref.marching_cubes(vol, 0.0, (h,) * 3, (x[0],) * 3)
    sv, sf, sn, _ = smc_ref.sparse_marching_cubes(vol, 16, 0.0, 0.0, h, (h,) * 3, (x[0],) * 3)
    assert np.array_equal(sv, v) and np.array_equal(sf, f)


def test_workspace_queries_refuse():
    from mvsdf_amd._lib import lib
    L = lib()
    assert L.mvsdf_smc_workspace_bytes(2, 8) == 0                       # N < 3
    assert L.mvsdf_smc_workspace_bytes(3, 1) == 0                       # B < 2
    assert L.mvsdf_smc_workspace_bytes(100, 0) == 0
    assert L.mvsdf_smc_workspace_bytes(100, -4) == 0
    assert L.mvsdf_smc_workspace_bytes(100, 2000) == 0                  # B > 1024
    assert L.mvsdf_smc_workspace_bytes(1 << 40, 8) == 0                 # blocks that overflow
    assert L.mvsdf_smc_workspace_bytes(3000, 2) == 0                    # more than 2^31 - 3 blocks
    assert L.mvsdf_smc_workspace_bytes(3, 2) > 0 and L.mvsdf_smc_workspace_bytes(2048, 8) > 0
    assert L.mvsdf_smc_workspace_bytes(2048, 16) < L.mvsdf_smc_workspace_bytes(2048, 8)
    assert L.mvsdf_smc_emit_workspace_bytes(100, 8, 0) == 0             # no active block
    assert L.mvsdf_smc_emit_workspace_bytes(100, 8, 13 ** 3 + 1) == 0    # more active blocks than blocks
    assert L.mvsdf_smc_emit_workspace_bytes(100, 8, 5) >= 5 * 9 ** 3 * 4
    assert L.mvsdf_smc_emit_workspace_bytes(2, 8, 1) == 0


def test_sparse_arguments_are_checked_before_the_device():
    from mvsdf_amd import mesh as M
    for kw in ({'resolution': 2}, {'block': 1}, {'block': 2.0}, {'margin': -1.0}, {'margin': float('nan')}, {'chunk': 0}, {'resolution': True}):
        args = dict(resolution=16, block=4)
        args.update(kw)
        with pytest.raises(ValueError):
            M.sparse_marching_cubes(lambda p: p[:, 0], **args)


def test_eval_flags_parse_and_are_off_by_default():
    from mvsdf_amd import evaluation as ev
    a = ev.eval_parser().parse_args([])
    assert a.sparse_mesh is False and a.mesh_block == 8 and a.mesh_margin == 0.5
    a = ev.eval_parser().parse_args(['--sparse_mesh', '--mesh_block', '16', '--mesh_margin', '0.5'])
    assert a.sparse_mesh is True and a.mesh_block == 16 and a.mesh_margin == 0.5
    import inspect
    from mvsdf_amd import mesh as M
    assert inspect.signature(M.surface_mesh).parameters['sparse'].default is False
    assert inspect.signature(ev.extract_world_mesh).parameters['sparse'].default is False
    assert inspect.signature(ev.evaluate).parameters['sparse_mesh'].default is False
