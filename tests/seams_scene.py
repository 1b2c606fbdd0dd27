"""Inputs of the seam-levelling tests (numpy only): small hand-labelled meshes, strips built for a node count, and the truth scene (the sphere of
texture_scene with images of one smooth world-space texture plus a per-view exposure offset).  tests/test_seams_host.py checks on the restatement
that they exercise the cases tests/test_gpu_seams.py needs."""
import numpy as np

import mc_ref
import raster_ref as R
import raster_scene as S
import stereo_scene
import texture_ref as T
import texture_scene as TS

HW = TS.HW
OFFSETS = (0.0, 12.0, -9.0, 6.0, -12.0, 9.0)                                  # grey levels added to view v of the truth scene
RADIUS = 0.7                                                                  # raster_scene's sphere


def cameras4():
    """four cameras that see the whole of the small meshes (|x|, |y| <= 0.4 around the origin) well inside their 160 x 120 images"""
    eyes = ((0.0, 0.0, 1.7), (0.5, 0.2, 1.9), (-0.6, -0.1, 2.2), (0.1, -0.5, 2.0))
    return np.stack([R.look_at(e, (0.0, 0.0, 0.0), HW, 1.5 * HW[0], up=(0.0, 1.0, 0.0)) for e in eyes])


def grid(n, seed=0):
    """n x n vertices over [-0.4, 0.4]^2 with a small bump in z -> (verts fp32, faces int32 [2 (n-1)^2, 3])"""
    rs = np.random.RandomState(seed)
    t = np.linspace(-0.4, 0.4, n)
    X, Y = np.meshgrid(t, t, indexing='ij')
    Z = 0.03 * rs.uniform(-1, 1, X.shape)
    verts = np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1).astype(np.float32)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing='ij')
    a = (i * n + j).ravel()
    faces = np.stack([np.stack([a, a + n, a + 1], 1), np.stack([a + 1, a + n, a + n + 1], 1)], 1).reshape(-1, 3).astype(np.int32)
    return verts, faces


def small_case(name):
    """-> dict(verts, faces, label int32 [F], views): the hand-labelled meshes"""
    if name == 'two_faces':                                                   # two faces with two labels
        verts, faces = grid(2)
        label = [0, 1]
    elif name == 'fan':                                                       # the centre vertex carries four labels: three seam partners per node
        ang = 2.0 * np.pi * np.arange(8) / 8
        verts = np.concatenate([[[0.0, 0.0, 0.02]], np.stack([0.35 * np.cos(ang), 0.3 * np.sin(ang), 0.01 * np.cos(3 * ang)], 1)]).astype(np.float32)
        faces = np.asarray([[0, 1 + k, 1 + (k + 1) % 8] for k in range(8)], np.int32)
        label = [0, 0, 1, 1, 2, 2, 3, 3]
    elif name == 'single':                                                    # one label: no seam
        verts, faces = grid(4)
        label = [2] * len(faces)
    elif name == 'gaps':                                                      # unlabelled faces between labelled ones
        verts, faces = grid(5)
        label = [(-1, 0, -1, 1, 3)[f % 5] for f in range(len(faces))]
    elif name == 'island':                                                    # a label island of one face
        verts, faces = grid(5)
        label = [0] * len(faces)
        label[13] = 1
    elif name == 'empty':
        verts, faces, label = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), []
    else:
        raise ValueError(name)
    return dict(verts=verts, faces=faces, label=np.asarray(label, np.int32).reshape(-1), views=4)


SMALL = ('two_faces', 'fan', 'single', 'gaps', 'island', 'empty')


def strip(nodes):
    """a triangle strip whose first half has label 0 and second half label 1 -> (faces int32, label int32, number of vertices): exactly `nodes`
    nodes (every vertex one, the two vertices the halves share two each)"""
    m = nodes - 2
    assert m >= 5
    faces = np.stack([np.arange(m - 2), np.arange(m - 2) + 1, np.arange(m - 2) + 2], 1).astype(np.int32)
    label = (np.arange(m - 2) >= (m - 2) // 2).astype(np.int32)
    return faces, label, m


def hand_atlas(case, P, images, o=0.5, texel_density=1.0):
    """the plain atlas (texture_ref's dict) of a hand-labelled mesh: every face's screen triangle is its corners' projection into its label's view"""
    verts, faces, label = case['verts'], case['faces'], case['label']
    screen = np.zeros((len(faces), 6))
    for v in np.unique(label[label >= 0]):
        _, sx, sy, _ = R.project(P[v], verts)
        k = np.nonzero(label == v)[0]
        screen[k] = np.stack([sx[faces[k, 0]], sy[faces[k, 0]], sx[faces[k, 1]], sy[faces[k, 1]], sx[faces[k, 2]], sy[faces[k, 2]]], 1)
    return T.atlas_of_labels(label, np.zeros(len(faces)), screen, images, o, texel_density)


# ---------------------------------------------------------------- the truth scene
def sphere_mesh():
    vol, spacing, origin = TS.volume('sphere')
    return mc_ref.marching_cubes(vol, 0.0, spacing, origin)


def truth_images(P, offsets, hw=HW, o=0.5):
    """uint8 [V,H,W,3]: stereo_scene.texture at the ray-sphere hit of every pixel (at the ray's point nearest the centre where it misses), scaled
    to [40, 215], plus the view's offset"""
    H, W = hw
    y, x = np.meshgrid(np.arange(H) + o, np.arange(W) + o, indexing='ij')
    C = R.camera_centers(P)
    out = []
    for v in range(len(P)):
        d = np.stack([x, y, np.ones_like(x)], -1) @ np.linalg.inv(P[v][:3, :3]).T
        dd, cd, cc = (d * d).sum(-1), d @ C[v], C[v] @ C[v]
        disc = cd * cd - dd * (cc - RADIUS * RADIUS)
        s = np.where(disc > 0, (-cd - np.sqrt(np.maximum(disc, 0.0))) / dd, -cd / dd)
        X = C[v] + s[..., None] * d
        im = 40.0 + 175.0 * stereo_scene.texture(X) + offsets[v]
        assert im.min() >= 0.0 and im.max() <= 255.0
        out.append(np.floor(im + 0.5).astype(np.uint8))
    return np.stack(out)


def truth_scene(offsets=OFFSETS):
    """-> dict(verts, faces, normals, P, depth, images, atlas): the sphere in raster_scene's six cameras with the plain atlas of the restatement"""
    verts, faces, normals = sphere_mesh()
    P = S.cameras()
    depth, _ = R.rasterize(verts, faces, P, HW, 0.5)
    images = truth_images(P, offsets)
    atlas = T.build_atlas(verts, normals, faces, P, depth, images, 0.5)
    return dict(verts=verts, faces=faces, normals=normals, P=P, depth=depth, images=images, atlas=atlas)
