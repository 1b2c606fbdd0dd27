"""Inputs of the chart-atlas tests (numpy only): hand-made meshes for neighbours and charts, the truth scene of seams_scene with its labels and
with 8 % of them flipped, and the sampling helpers both test files use."""
import numpy as np

import charts_ref as C
import seams_scene as SS

PADS = (1, 2, 4, 8)


def hand_mesh(name):
    """-> (faces int32 [F,3], labels int32 [F], vertices, expected nbr int32 [F,3] or None, expected face_chart or None)"""
    if name == 'two_strips':                                                  # a strip whose halves carry two labels: two charts
        faces, label, nv = SS.strip(14)
        F = len(faces)
        nbr = np.full((F, 3), -1, np.int32)
        for f in range(F):                                                    # face f = (f, f+1, f+2): edge 1 = (f+1, f+2) is shared with f+1, edge 0 with f-1
            if f + 1 < F:
                nbr[f, 1] = f + 1
            if f > 0:
                nbr[f, 0] = f - 1
        return faces, label, nv, nbr, label.copy()
    if name == 'three_on_an_edge':                                            # faces 0, 1, 2 share edge (0, 1): no neighbour there; 2 and 3 share (1, 4)
        faces = np.asarray([[0, 1, 2], [1, 0, 3], [0, 1, 4], [4, 1, 5]], np.int32)
        nbr = np.asarray([[-1, -1, -1], [-1, -1, -1], [-1, 3, -1], [2, -1, -1]], np.int32)
        return faces, np.zeros(4, np.int32), 6, nbr, np.asarray([0, 1, 2, 2], np.int32)
    if name == 'repeated_vertex':                                             # face 1 = (1, 2, 1): its edges 0 and 1 are both (1, 2), edge 2 joins 1 with 1
        faces = np.asarray([[0, 1, 2], [1, 2, 1], [2, 1, 3]], np.int32)
        nbr = np.full((3, 3), -1, np.int32)                                   # (1, 2) has four edges: nobody pairs
        return faces, np.zeros(3, np.int32), 4, nbr, np.asarray([0, 1, 2], np.int32)
    if name == 'own_pair':                                                    # face 0 = (0, 1, 0) holds both edges of (0, 1): exactly two, one face
        faces = np.asarray([[0, 1, 0], [1, 2, 3]], np.int32)
        return faces, np.asarray([0, 0], np.int32), 4, np.full((2, 3), -1, np.int32), np.asarray([0, 1], np.int32)
    if name == 'unlabelled':                                                  # a grid with unlabelled faces between labelled ones
        verts, faces = SS.grid(5)
        label = np.asarray([(-1, 0, 0, 1, 3)[f % 5] for f in range(len(faces))], np.int32)
        return faces, label, len(verts), None, None
    if name == 'none_labelled':
        verts, faces = SS.grid(3)
        return faces, np.full(len(faces), -1, np.int32), len(verts), None, np.full(len(faces), -1, np.int32)
    if name == 'one_face':
        return np.asarray([[0, 1, 2]], np.int32), np.asarray([1], np.int32), 3, np.full((1, 3), -1, np.int32), np.asarray([0], np.int32)
    if name == 'empty':
        return np.zeros((0, 3), np.int32), np.zeros(0, np.int32), 0, np.zeros((0, 3), np.int32), np.zeros(0, np.int32)
    raise ValueError(name)


HAND = ('two_strips', 'three_on_an_edge', 'repeated_vertex', 'own_pair', 'unlabelled', 'none_labelled', 'one_face', 'empty')


def flipped_labels(label, score_all, share=0.08, seed=0):
    """`share` of the labelled faces, drawn with RandomState(seed), take a random one of their other candidate views (score > 0); a face with one
    candidate keeps it"""
    rs = np.random.RandomState(seed)
    label = np.asarray(label, np.int32).copy()
    on = np.nonzero(label >= 0)[0]
    for f in rs.choice(on, int(round(share * len(on))), replace=False):
        cand = np.nonzero((score_all[:, f] > 0) & (np.arange(len(score_all)) != label[f]))[0]
        if len(cand):
            label[f] = cand[rs.randint(len(cand))]
    return label


_TRUTH = {}


def truth():
    """seams_scene's truth scene with the view tables of the restatement and the flipped labels (computed once)"""
    if not _TRUTH:
        s = SS.truth_scene()
        tables = C.view_tables(s['verts'], s['normals'], s['faces'], s['P'], s['depth'])
        _TRUTH.update(s, tables=tables, label=s['atlas']['label'], flipped=flipped_labels(s['atlas']['label'], tables[0]))
    return _TRUTH


def bary(rs, n):
    """n random barycentric weights [n,3], uniform over the triangle"""
    r1, r2 = np.sqrt(rs.uniform(size=n)), rs.uniform(size=n)
    return np.stack([1.0 - r1, r1 * (1.0 - r2), r1 * r2], 1)


def uv_points(a, f, w):
    """the atlas positions (x, y) a viewer computes from the fp32 UVs of faces f at the weights w [n,3]"""
    uv = a['uv'].astype(np.float64)[f]
    p = (w[:, :, None] * uv).sum(1)
    return p[:, 0] * a['Wt'], (1.0 - p[:, 1]) * a['Ht']
