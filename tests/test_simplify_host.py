"""Mesh simplification without a GPU: what the definition (tests/simplify_ref.py, the numpy restatement of Mesh.simplify) promises on analytic solids
-- quadric placement keeps sharp features, spheres stay closed and oriented, a thin plate becomes a double-sided sheet -- and on hand-built meshes.

Measured with this file (RMS distance of the output vertices to the true box, quadric / mean, cell = 3 h): N = 24: 0.178, N = 40: 0.143."""
import numpy as np
import pytest

import mc_ref
import simplify_ref as S

BOX = (0.53, 0.47, 0.61)
PLATE = (0.6, 0.55, 0.05)
SPHERE_CASES = [(16, 1), (16, 2), (16, 3), (16, 4.5), (24, 1), (24, 2), (24, 3), (40, 1), (40, 2), (40, 3), (40, 4.5)]


def _rms_to_box(v, half):
    d = S.box_sdf(v.astype(np.float64), half)
    return float(np.sqrt((d * d).mean()))


@pytest.mark.parametrize('n', [24, 40])
def test_quadric_placement_keeps_the_box_sharp(n):
    v, f, nrm, col, h = S.shape_mesh('box', n, BOX)
    rms = {}
    for placement in ('quadric', 'mean'):
        ov, of, _, _, st = S.simplify(v, f, nrm, col, 3 * h, placement=placement)
        assert mc_ref.directed_edges_ok(of, len(ov))
        rms[placement] = _rms_to_box(ov, BOX)
    print('box N = %d: rms quadric %.6g, mean %.6g, ratio %.4f' % (n, rms['quadric'], rms['mean'], rms['quadric'] / rms['mean']))
    assert rms['quadric'] <= 0.5 * rms['mean']


@pytest.mark.parametrize('n,mult', SPHERE_CASES)
def test_sphere_stays_closed_and_oriented(n, mult):
    v, f, nrm, col, h = S.shape_mesh('sphere', n)
    for placement in ('quadric', 'mean'):
        ov, of, on, oc, st = S.simplify(v, f, nrm, col, mult * h, placement=placement)
        assert mc_ref.directed_edges_ok(of, len(ov))
        assert st['faces'] == len(of) and st['vertices'] == len(ov) and st['clusters'] >= len(ov)
        assert st['degenerate'] + st['duplicates'] + st['faces'] == len(f)
    assert mc_ref.signed_volume(ov, of) > 0


def test_thin_plate_becomes_a_double_sided_sheet():
    v, f, nrm, col, h = S.shape_mesh('box', 24, PLATE)
    ov, of, _, _, st = S.simplify(v, f, nrm, col, 2 * h)
    have = {tuple(r) for r in S.rotate_min_first(of).tolist()}
    opposite = {tuple(r) for r in S.rotate_min_first(of[:, [0, 2, 1]]).tolist()}
    print('plate: %d faces, %d with opposites' % (len(of), len(have & opposite)))
    assert len(have) == len(of) and have == opposite
    assert st['duplicates'] == 0


HAND = S.HAND


def _run(name, placement='quadric'):
    (v, f, n, c), cell, org = HAND[name]()
    return (v, f), S.simplify(v, f, n, c, cell, origin=org, placement=placement)


def test_duplicate_keeps_the_lower_face():
    (v, f), (ov, of, _, _, st) = _run('duplicate')
    assert st['duplicates'] == 1 and st['degenerate'] == 1 and st['clusters'] == 3
    assert of.tolist() == [[0, 2, 1], [0, 1, 2]]                       # faces 0 and 1, in their own corner order; face 2 repeats face 1


def test_tetrahedron_in_one_cell_is_dropped():
    (v, f), (ov, of, _, _, st) = _run('tetrahedron')
    assert st['clusters'] == 4 and st['vertices'] == 3 and st['degenerate'] == 4 and of.tolist() == [[0, 1, 2]]
    assert np.array_equal(ov, v[:3])


def test_unreferenced_vertex_is_dropped():
    (v, f), (ov, of, _, _, st) = _run('unreferenced')
    assert st['clusters'] == 4 and st['vertices'] == 3 and of.tolist() == [[0, 1, 2]]
    assert np.array_equal(ov, v[[0, 2, 3]])


def test_zero_area_faces_give_the_mean():
    (v, f), (ov, of, _, _, st) = _run('zero_area')
    assert st['quadric_placed'] == 0 and st['faces'] == 3
    assert np.array_equal(ov[0], np.array([0.5, 0.5, 0.5], np.float32))


def test_candidate_that_leaves_its_cell_falls_back_to_the_mean():
    (v, f), (ov, of, _, _, st) = _run('candidate_leaves')
    (_, _), (mv, _, _, _, _) = _run('candidate_leaves', 'mean')
    assert np.array_equal(ov[0], mv[0]) and np.array_equal(ov[0], np.array([0.5, 0.5, 0.1], np.float32))
    assert st['quadric_placed'] == st['vertices'] - 1                 # single-vertex clusters sit on their planes: x = 0 is accepted


def test_refusals():
    (v, f, n, c), cell, org = HAND['duplicate']()
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            S.simplify(v, f, n, c, bad)
    with pytest.raises(ValueError):
        S.simplify(v, f, n, c, 1.0, placement='median')
    with pytest.raises(ValueError):
        S.simplify(v, f, n, c, 1e-7)                                   # cell indices beyond 2^21
    with pytest.raises(ValueError):
        S.simplify(v, f, n, c, 1.0, origin=(0.2, 0.0, 0.0))            # a vertex below the origin
    w = v.copy()
    w[1, 1] = np.nan
    with pytest.raises(ValueError):
        S.simplify(w, f, n, c, 1.0)
    g = f.copy()
    g[0, 0] = 5
    with pytest.raises(ValueError):
        S.simplify(v, g, n, c, 1.0)
