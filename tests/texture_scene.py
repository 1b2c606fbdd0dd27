"""Inputs of the texture atlas tests (numpy only): small marching-cubes meshes of raster_scene's volumes, its cameras with and without a twin, images
that are a linear function of the pixel coordinates, a mesh inside the image for the meaning test, and class histograms for the packing tests.
tests/test_texture_host.py checks on the restatement that they exercise the cases tests/test_gpu_texture.py needs."""
import numpy as np

import raster_ref as R
import raster_scene as S
import texture_ref as T

HW = S.HW
RES = {'sphere': 24, 'torus': 28}                                             # lattice points a side: one to two thousand faces


def volume(kind):
    return S.volume(kind, RES[kind])


def normals_with_gaps(normals, seed=5):
    """the mesh's normals with a run of vertices zeroed and a run reversed: faces inside the runs fail the normal test in views that see them"""
    n = np.array(normals, np.float32)
    rs = np.random.RandomState(seed)
    k = len(n) // 12
    a, b = rs.randint(0, len(n) - k, 2)
    n[a:a + k] = 0.0
    n[b:b + k] *= -1.0
    return n


def twin_cameras():
    """raster_scene's six cameras with the second one repeated at the end: every face scores the same in views 1 and 6"""
    P = S.cameras()
    return np.concatenate([P, P[1:2]])


def random_images(V, hw=HW, seed=3):
    rs = np.random.RandomState(seed)
    images = rs.randint(0, 256, (V,) + tuple(hw) + (3,)).astype(np.uint8)
    masks = (rs.uniform(size=(V,) + tuple(hw)) > 0.15).astype(np.uint8)
    return images, masks


# the linear images of the meaning test: value_c(x, y) = a_c + b_c * x + c_c * y per view, inside [3, 252] over the image
LINEAR = np.array([[20.0, 1.0, 0.4], [240.0, -0.9, -0.6], [40.0, 0.3, 1.1]])


def linear_value(v, u, t):
    """the linear function of view v at pixel coordinates (u, t) (arrays) -> fp64 [..., 3]"""
    k = LINEAR * (1.0 + 0.03 * (v % 3))
    return k[:, 0] + k[:, 1] * np.asarray(u)[..., None] + k[:, 2] * np.asarray(t)[..., None]


def linear_images(V, hw=HW):
    y, x = np.meshgrid(np.arange(hw[0], dtype=np.float64), np.arange(hw[1], dtype=np.float64), indexing='ij')
    im = np.stack([linear_value(v, x, y) for v in range(V)])
    assert im.min() >= 0.0 and im.max() <= 255.0
    return np.floor(im + 0.5).astype(np.uint8)


def inside_scene(seed=0):
    """-> dict(verts, faces, normals, P): a bumpy sheet of about 400 faces of very different sizes, seen whole by three cameras, every projected
    vertex at least 4 pixels inside the 160 x 120 images"""
    rs = np.random.RandomState(seed)
    step = np.geomspace(0.01, 0.2, 15)                                        # cells from about one pixel to about twenty
    t = -0.5 + np.concatenate([[0.0], np.cumsum(step) / step.sum()])
    X, Y = np.meshgrid(t, t * 0.75, indexing='ij')
    Z = 0.05 * np.sin(5.0 * X) * np.cos(4.0 * Y) + 0.01 * rs.uniform(-1, 1, X.shape)
    n = len(t)
    verts = np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1).astype(np.float32)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing='ij')
    a = (i * n + j).ravel()
    faces = np.concatenate([np.stack([a, a + n, a + 1], 1), np.stack([a + 1, a + n, a + n + 1], 1)]).astype(np.int32)
    normals = np.zeros_like(verts)
    normals[:, 2] = 1.0
    P = np.stack([R.look_at(e, (0.0, 0.0, 0.0), HW, 1.5 * HW[0], up=(0.0, 1.0, 0.0)) for e in ((0.0, 0.0, 1.7), (0.5, 0.2, 1.9), (-0.6, -0.1, 2.2))])
    return dict(verts=verts, faces=faces, normals=normals, P=P)


def histograms(seed=0, n_random=24):
    """class histograms (faces per class, class k = edge 4 << k) for the packing tests: the named cases, then random ones"""
    rs = np.random.RandomState(seed)
    out = [[1, 0, 0, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0, 0],                      # a single face
           [37, 0, 0, 0, 0, 0, 0], [0, 0, 12, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 3],   # all faces in one class
           [9, 0, 5, 0, 0, 0, 0], [3, 0, 0, 0, 2, 0, 0],                      # an empty class between two occupied ones
           [1, 3, 5, 7, 1, 1, 1],                                             # odd counts
           [32, 0, 0, 0, 0, 0, 0], [0, 8, 0, 0, 0, 0, 0], [8, 6, 0, 0, 0, 0, 0],  # T = 16: an exact power of 4
           [4, 0, 0, 0, 0, 0, 0], [3, 0, 0, 0, 0, 0, 0], [0, 3, 0, 0, 0, 0, 0]]   # T = 2, 2, 8: B odd, a non-square atlas
    for _ in range(n_random):
        top = rs.randint(1, 8)
        h = [int(rs.randint(0, 40) * (rs.uniform() < 0.7)) if k < top else 0 for k in range(7)]
        h = [c if k < 5 else min(c, 2) for k, c in enumerate(h)]              # keep the atlases to a few hundred texels a side
        if sum(h) == 0:
            h[0] = 1
        out.append(h)
    return out


def meaning_error(a, images, o, rs, per_face=12):
    """the largest difference between a bilinear lookup of the atlas at the UV of random barycentric points of the labelled faces and the linear
    function of the face's view at the corresponding screen point; asserts the test's premises (labelled faces, every projected vertex at least
    4 px inside the image, no patch at the N_MAX clamp)"""
    H, W = images.shape[1:3]
    lab = a['label'] >= 0
    assert lab.sum() > 100 and len(np.unique(a['label'][lab])) >= 2 and len(np.unique(a['cls'][lab])) >= 3
    s = a['screen'][lab]
    assert (s[:, 0::2] - o).min() >= 4 and (s[:, 0::2] - o).max() <= W - 5 and (s[:, 1::2] - o).min() >= 4 and (s[:, 1::2] - o).max() <= H - 5
    assert (a['cls'] < T.CLASSES - 1).all()
    Ht, Wt = a['texture'].shape[:2]
    worst = 0.0
    for f in np.nonzero(lab)[0]:
        w = rs.dirichlet((0.6, 0.6, 0.6), per_face)
        uv = w @ a['uv'][f].astype(np.float64)
        val, _, _ = T.lookup(a['texture'], uv[:, 0] * Wt, (1.0 - uv[:, 1]) * Ht)
        sc = w @ a['screen'][f].reshape(3, 2)
        want = linear_value(int(a['label'][f]), sc[:, 0] - o, sc[:, 1] - o)
        worst = max(worst, float(np.abs(val - want).max()))
    return worst


def check_cases(label, st, twin=None):
    """what tests/test_gpu_texture.py asserts of its scenes before it compares"""
    V = st['scores'].shape[0]
    wins = np.bincount(label[label >= 0], minlength=V)
    views = [v for v in range(V) if twin is None or v != twin[1]]
    assert all(wins[v] > 0 for v in views), wins                              # every view wins some face (the twin never can: it loses every tie)
    assert (label < 0).any()
    assert (st['visible'] & ~(st['in_image'] & st['normal'])).any()          # all vertices visible, but the in-image or the normal test fails
    if twin is not None:
        a, b = twin
        top = st['scores'].max(0)
        tie = (st['scores'][a] == top) & (st['scores'][b] == top) & (top > 0)
        assert tie.any() and (label[tie] == a).all() and wins[b] == 0         # ties broken by the index


def check_classes(counts):
    assert (counts > 0).sum() >= 3 and (counts % 2 == 1).any(), counts
