"""Inputs of the mesh rendering tests (numpy only): analytic volumes for marching cubes, cameras around them, a seeded triangle soup and a
two-layer occlusion scene.  tests/test_raster_host.py checks on the restatement that they exercise the cases tests/test_gpu_raster.py needs."""
import numpy as np

import raster_ref as R

HW = (120, 160)                                                               # 160 x 120 pixels
SOUP_HW = (48, 64)


def volume(kind, res):
    """fp32 [res,res,res] on the [-1, 1]^3 lattice: a sphere of radius 0.7 or a torus (R = 0.55, r = 0.22) around z"""
    x = np.linspace(-1.0, 1.0, res)
    X, Y, Z = np.meshgrid(x, x, x, indexing='ij')
    if kind == 'sphere':
        v = np.sqrt(X * X + Y * Y + Z * Z) - 0.7
    elif kind == 'torus':
        v = np.sqrt((np.sqrt(X * X + Y * Y) - 0.55) ** 2 + Z * Z) - 0.22
    else:
        raise ValueError(kind)
    return v.astype(np.float32), (x[2] - x[1],) * 3, (x[0],) * 3


def cameras(hw=HW):
    """6 cameras: five around the origin that see the whole object, and one just outside it looking along its flank, so that part of the mesh
    is behind the camera and part off screen"""
    P = []
    for i, el in enumerate((-0.6, 0.1, 0.5, 0.9, -0.2)):
        az = 0.3 + 2.0 * np.pi * i / 5
        eye = 2.6 * np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
        P.append(R.look_at(eye, (0.0, 0.0, 0.0), hw, 1.3 * hw[0]))
    P.append(R.look_at((0.9, 0.0, 0.1), (0.0, 0.9, 0.0), hw, 1.6 * hw[0]))
    return np.stack(P)


def soup(seed=0, hw=SOUP_HW):
    """-> (verts fp32, faces int32, P [2,4,4]): random triangles in front of two cameras, with zero-area faces, faces that straddle the camera
    plane, huge faces over the whole image, sub-pixel faces and exact duplicates"""
    rs = np.random.RandomState(seed)
    P = np.stack([R.look_at((0.0, -3.0, 0.2), (0.0, 0.0, 0.0), hw, 1.2 * hw[0]), R.look_at((2.5, 1.5, -0.5), (0.0, 0.0, 0.0), hw, 1.2 * hw[0])])
    verts, faces = [], []

    def tri(p):
        faces.append([len(verts), len(verts) + 1, len(verts) + 2])
        verts.extend(p)
    for _ in range(60):                                                       # ordinary triangles, a few to a few hundred pixels
        c = rs.uniform(-0.8, 0.8, 3)
        tri(c + rs.uniform(-0.35, 0.35, (3, 3)))
    for _ in range(40):                                                       # sub-pixel
        c = rs.uniform(-0.8, 0.8, 3)
        tri(c + rs.uniform(-0.004, 0.004, (3, 3)))
    for _ in range(6):                                                        # zero area: a repeated vertex id, and three collinear points
        c = rs.uniform(-0.8, 0.8, 3)
        d = rs.uniform(-0.3, 0.3, 3)
        n = len(verts)
        verts.extend([c, c + d, c + 2 * d])
        faces.append([n, n, n + 1])
        faces.append([n, n + 1, n + 1])
    for _ in range(8):                                                        # partly behind the first camera (y < -3) and / or the second
        c = np.array([rs.uniform(-0.5, 0.5), -3.0, rs.uniform(-0.5, 0.5)])
        tri(c + rs.uniform(-1.5, 1.5, (3, 3)))
    for eye in ((0.0, -3.0, 0.2), (2.5, 1.5, -0.5)):                          # huge: behind the scene, over the whole image of one camera each
        eye = np.array(eye)
        d = -eye / np.linalg.norm(eye)
        u = np.cross(d, [0.0, 0.0, 1.0])
        u /= np.linalg.norm(u)
        w = np.cross(d, u)
        for k in range(2):
            c = eye + d * (np.linalg.norm(eye) + 0.9 + 0.3 * k)
            tri(np.array([c - 60.0 * u - 50.0 * w, c + 60.0 * u - 50.0 * w, c + (70.0 + 10.0 * k) * w + 5.0 * (k - 0.5) * d]))
    n_unique = len(faces)
    for f in rs.choice(n_unique, 30, replace=False):                          # exact duplicates, later in the list
        faces.append(list(faces[f]))
    return np.asarray(verts, np.float32), np.asarray(faces, np.int32), P


def layers(hw=HW, seed=0):
    """The two-layer occlusion scene -> dict: a front sheet (z = 0.3, |x|, |y| <= 0.5) over a larger back sheet (z = -0.3, |x|, |y| <= 0.9), both
    fine grids with normals +z, seen by four cameras above them.  Back vertices under the front sheet are seen by no camera.  A tenth of the normals
    are zero.  Random images; masks that cut a band out of every view."""
    rs = np.random.RandomState(seed)

    def sheet(half, z, n):
        t = np.linspace(-half, half, n)
        X, Y = np.meshgrid(t, t, indexing='ij')
        v = np.stack([X.ravel(), Y.ravel(), np.full(X.size, z)], 1)
        i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing='ij')
        a = (i * n + j).ravel()
        f = np.concatenate([np.stack([a, a + n, a + 1], 1), np.stack([a + 1, a + n, a + n + 1], 1)])
        return v, f
    v0, f0 = sheet(0.5, 0.3, 31)
    v1, f1 = sheet(0.9, -0.3, 41)
    verts = np.concatenate([v0, v1]).astype(np.float32)
    faces = np.concatenate([f0, f1 + len(v0)]).astype(np.int32)
    normals = np.zeros_like(verts)
    normals[:, 2] = 1.0
    normals[rs.choice(len(verts), len(verts) // 10, replace=False)] = 0.0
    P = np.stack([R.look_at(e, (0.0, 0.0, 0.0), hw, 1.5 * hw[0], up=(0.0, 1.0, 0.0))
                  for e in ((0.0, 0.0, 3.0), (0.25, 0.1, 3.0), (-0.2, 0.2, 2.8), (0.1, -0.25, 3.2))])
    images = rs.randint(0, 256, (len(P), hw[0], hw[1], 3)).astype(np.uint8)
    masks = np.ones((len(P), hw[0], hw[1]), np.uint8)
    for v in range(len(P)):
        masks[v, :, 20 + 7 * v:35 + 7 * v] = 0
    return dict(verts=verts, faces=faces, normals=normals, P=P, images=images, masks=masks, n_front=len(v0))
