"""The numpy restatement of seam levelling (tests/seams_ref.py) against truth, and the source-level facts of mvsdf_amd/seams.py.  No GPU needed.

Measured on the restatement (the bounds below are twice these, the project's convention; DESIGN.md records them):
* the solve against numpy.linalg.solve on the truth scene (1307 nodes, cg_tol = 1e-6, 135 iterations): largest |g - x| 2.48e-4 grey levels;
* the truth scene (offsets 0, +12, -9, +6, -12, +9): seam RMS 15.38 before, 0.500 after, ratio 0.0325;
* all offsets 0: seam RMS 3.11 before, 0.498 after; largest |g| 11.83; the levelled atlas differs from the plain one by at most 17 grey levels.
"""
import os
import re

import numpy as np
import pytest

import seams_ref as SR
import seams_scene as SS
import texture_scene as TS
from conftest import ROOT

SOLVE_GAP = 2.48e-4
TRUTH_RATIO = 0.0325
ZERO_G, ZERO_ATLAS, ZERO_RATIO = 11.83, 17, 0.498 / 3.11


@pytest.fixture(scope='module')
def truth():
    s = SS.truth_scene()
    G = SR.seam_graph(s['faces'], s['atlas']['label'])
    f = SR.node_colors(G, s['verts'], s['images'], s['P'])
    g, info = SR.solve_levels(G, f)
    return dict(s, G=G, f=f, g=g, info=info)


def test_tree_sum_is_the_padded_pairwise_sum():
    a = np.asarray([1e16, 1.0, -1e16, 1.0, 3.0])
    assert SR.tree_sum(a) == (((1e16 + 1.0) + (-1e16 + 1.0)) + ((3.0 + 0.0) + (0.0 + 0.0)))
    assert SR.tree_sum([]) == 0.0 and SR.tree_sum([2.5]) == 2.5


@pytest.mark.parametrize('name', SS.SMALL)
def test_small_cases_have_the_graph_they_are_named_for(name):
    c = SS.small_case(name)
    G = SR.seam_graph(c['faces'], c['label'])
    K = len(G['node_vertex'])
    key = G['node_vertex'].astype(np.int64) * 100 + G['node_view']
    assert (np.diff(key) > 0).all()                                           # listed by (i, v) ascending, no node twice
    assert ((G['corner_node'] >= 0).all(1) == (c['label'] >= 0)).all()
    assert G['adj_off'][-1] == len(G['adj_node']) == G['adj_seam'].sum() + 6 * (c['label'] >= 0).sum()
    want = dict(two_faces=(6, 1), fan=(16, 3), single=(16, 0), empty=(0, 0)).get(name)
    if want:
        assert (K, int(G['adj_seam'].max()) if K else 0) == want
    if name == 'gaps':
        assert (c['label'] < 0).any() and G['adj_seam'].max() >= 1
    if name == 'island':
        k = G['corner_node'][13]
        assert (G['node_view'][k] == 1).all() and (G['adj_seam'][k] == 1).all() and (G['node_view'] == 1).sum() == 3


@pytest.mark.parametrize('nodes', [63, 64, 65, 2048, 2049])
def test_strips_have_the_node_count_they_are_built_for(nodes):
    faces, label, m = SS.strip(nodes)
    G = SR.seam_graph(faces, label)
    assert len(G['node_vertex']) == nodes and (G['adj_seam'] > 0).sum() == 4 and faces.max() == m - 1


@pytest.mark.parametrize('name', ['two_faces', 'fan', 'gaps', 'island'])
def test_the_operator_is_symmetric_positive_definite_and_the_dense_matrix_agrees(name):
    c = SS.small_case(name)
    G = SR.seam_graph(c['faces'], c['label'])
    A = SR.dense_matrix(G, 0.1, 1e-3)
    assert np.abs(A - A.T).max() <= 1e-12 and np.linalg.eigvalsh(A).min() > 0.0
    x = np.random.RandomState(1).normal(size=(len(A), 3))
    assert np.abs(A @ x - SR.apply_operator(G, x, 0.1, 1e-3)).max() <= 1e-12
    assert np.abs(np.diag(A) - SR.diagonal(G, 0.1, 1e-3)).max() <= 1e-12
    f = np.random.RandomState(2).uniform(0, 255, (len(A), 3))
    g, info = SR.solve_levels(G, f, cg_iters=500, cg_tol=1e-12)
    assert np.abs(g - np.linalg.solve(A, SR.rhs(G, f))).max() <= 1e-6 and max(info['iterations']) <= len(A) + 5


def test_a_single_label_has_no_seam_and_needs_no_iteration():
    c = SS.small_case('single')
    G = SR.seam_graph(c['faces'], c['label'])
    g, info = SR.solve_levels(G, np.random.RandomState(0).uniform(0, 255, (16, 3)))
    assert not g.any() and info['iterations'] == [0, 0, 0] and info['rho0'] == [0.0, 0.0, 0.0]


def test_the_budget_ends_the_solve(truth):
    g1, i1 = SR.solve_levels(truth['G'], truth['f'], cg_iters=1)
    g0, i0 = SR.solve_levels(truth['G'], truth['f'], cg_iters=0)
    assert i0['iterations'] == [0, 0, 0] and not g0.any() and i0['rho'] == i0['rho0']
    assert i1['iterations'] == [1, 1, 1] and g1.any() and all(r < r0 for r, r0 in zip(i1['rho'], i1['rho0']))


def test_the_solve_meets_the_dense_solution(truth):
    G, f, g, info = truth['G'], truth['f'], truth['g'], truth['info']
    A = SR.dense_matrix(G, 0.1, 1e-3)
    assert np.abs(A - A.T).max() <= 1e-12 and np.linalg.eigvalsh(A).min() > 0.0
    gap = float(np.abs(g - np.linalg.solve(A, SR.rhs(G, f))).max())
    print('solve gap', gap, info)
    assert max(info['iterations']) < 200 and all(r <= 1e-12 * r0 for r, r0 in zip(info['rho'], info['rho0']))
    assert gap <= 2 * SOLVE_GAP


def test_truth_scene_levelling_removes_the_exposure_steps(truth):
    G, f, g, a = truth['G'], truth['f'], truth['g'], truth['atlas']
    seam_vertices = np.unique(G['node_vertex'][G['adj_seam'] > 0])
    assert len(seam_vertices) >= 100 and G['adj_seam'].max() >= 2 and (a['label'] < 0).any()      # the premises
    assert (f + g).min() > 0.5 and (f + g).max() < 254.5                     # no corrected value at the clamp
    before, pairs = SR.seam_rms(G, f, np.zeros_like(g))
    after, _ = SR.seam_rms(G, f, g)
    print('seam rms before', before, 'after', after, 'ratio', after / before, 'pairs', pairs)
    assert before > 10.0 and after / before <= 2 * TRUTH_RATIO


def test_without_offsets_little_is_changed():
    s = SS.truth_scene((0.0,) * 6)
    a = s['atlas']
    L = SR.level_atlas(a, s['verts'], s['faces'], s['images'], s['P'])
    before, _ = SR.seam_rms(L['graph'], L['f'], np.zeros_like(L['g']))
    after, _ = SR.seam_rms(L['graph'], L['f'], L['g'])
    diff = int(np.abs(L['texture'].astype(np.int64) - a['texture'].astype(np.int64)).max())
    print('max |g|', np.abs(L['g']).max(), 'atlas difference', diff, 'seam rms', before, after)
    assert np.abs(L['g']).max() <= 2 * ZERO_G and diff <= 2 * ZERO_ATLAS and after / before <= 2 * ZERO_RATIO
    assert np.array_equal(L['valid'], a['valid'])
    zero = SR.fill(s['images'], 0.5, a['label'], a['screen'], a['order'], a['layout'], L['graph']['corner_node'], np.zeros_like(L['g']))
    assert np.array_equal(zero[0], a['texture']) and np.array_equal(zero[1], a['valid'])         # g = 0: the plain atlas byte for byte


def test_hand_atlases_fill_and_level():
    P = SS.cameras4()
    images = TS.random_images(len(P))[0]
    for name in SS.SMALL:
        c = SS.small_case(name)
        a = SS.hand_atlas(c, P, images)
        L = SR.level_atlas(a, c['verts'], c['faces'], images, P)
        assert np.array_equal(L['valid'], a['valid']) and L['texture'].shape == a['texture'].shape
        if name in ('two_faces', 'fan', 'gaps', 'island'):
            assert (L['texture'] != a['texture']).any()
        else:
            assert np.array_equal(L['texture'], a['texture'])


# ---------------------------------------------------------------- the source-level facts
def test_the_module_allocates_no_uninitialised_memory_and_is_built():
    import test_dirty_memory_table_host as DM
    from mvsdf_amd import build, seams
    from mvsdf_amd._lib import K, PROTOTYPES
    with open(os.path.join(ROOT, 'mvsdf_amd', 'seams.py')) as fh:
        src = fh.read()
    assert 'torch.empty' not in src and not DM.OTHER_SPELLINGS.search(src) and not re.search(r'from torch import', src)
    assert 'seams.hip' in build.SOURCES
    bits = [row[0] for row in seams.ERRORS]
    block = {v for k, v in vars(K).items() if k.startswith('MVSDF_TX_ERR_')}
    assert set(bits) <= block and len(set(bits)) == len(bits) and K.MVSDF_TX_ERR_LABEL == 8
    for name in ('workspace_bytes', 'nodes', 'graph', 'colors', 'apply', 'solve', 'fill'):
        assert 'mvsdf_seams_' + name in PROTOTYPES
    assert K.MVSDF_SL_H_WORDS <= 32
    for fn in ('seam_graph', 'node_colors', 'apply_operator', 'solve_levels', 'level_atlas'):
        assert callable(getattr(seams, fn))
    found = DM.allocating_entries()
    assert not [k for k in found if k.startswith('seams.')] and 'texture.build_atlas' in found


def test_the_option_is_wired_and_off_by_default():
    import importlib.util
    import inspect
    from mvsdf_amd import evaluation, texture
    sig = inspect.signature(texture.build_atlas).parameters
    assert sig['level_seams'].default is False and sig['level_options'].default is None
    assert inspect.signature(evaluation.evaluate).parameters['level_seams'].default is False
    p = evaluation.eval_parser()
    base = ['--data_dir', 'd', '--conf', 'c', '--expname', 'e']
    assert p.parse_args(base).level_seams is False and p.parse_args(base + ['--texture_mesh', '--level_seams']).level_seams is True
    for name in ('texture_mesh', 'time_texture'):
        spec = importlib.util.spec_from_file_location('tool_' + name, os.path.join(ROOT, 'tools', name + '.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        extra = ['in.obj', 'out.obj', '--data_dir', 'd'] if name == 'texture_mesh' else []
        assert mod.parser().parse_args(extra).level_seams is False and mod.parser().parse_args(extra + ['--level_seams']).level_seams is True


def test_argument_errors_come_before_any_launch():
    import torch
    from mvsdf_amd import seams
    from mvsdf_amd.mesh import Mesh
    m = Mesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), torch.zeros(3, 3))
    with pytest.raises(Exception, match='GPU'):
        seams.seam_graph(m, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match='SeamGraph'):
        seams.solve_levels(None, torch.zeros(0, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match='TexturedMesh'):
        seams.level_atlas(None, np.zeros((1, 2, 2, 3), np.uint8))
