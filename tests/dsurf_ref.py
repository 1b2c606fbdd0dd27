"""The phase-0 depth-surface sampler (mvsdf_amd/csrc/sample_kernels.hip) restated in numpy.  No GPU, no torch.

Given the seed the SELECTION is integer arithmetic (lowbias32, a 4-round Feistel network, cycle walking, "the first n eligible pixels of the walk"),
restated here in 64-bit integers masked to 32 bits, so every wrap-around of the kernel's uint32 is explicit.  The JITTER is an integer hash scaled by
2^-24: exact in float32.  Only the unprojection is floating point: `points64` is the float64 value of the formula on the kernel's own float32 inputs,
`points32` the same formula in float32 in the order ds_point writes it, one rounding per operation, nothing fused -- it sizes the tolerance
(`point_tolerance`), it is never compared with the kernel.

Which pixels are eligible is decided from `points64`.  A pixel whose point lies within float32 rounding of a face of the box could be decided either
way by the kernel; `clear_band` removes those pixels from the INPUT (depth 0), after which the kernel's selection must equal `select` index for index."""
import numpy as np

M32 = 0xFFFFFFFF
FILL = 1 << 62                         # what ops.dsurf_samples fills idx with before the selection (ops.py::dsurf_samples)


def _u(x):
    return np.asarray(x, np.uint64) & np.uint64(M32)


def hash32(x):
    """ds_hash (sample_kernels.hip:32-35): lowbias32 on uint32, every product wrapped to 32 bits."""
    x = _u(x)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(16))
    return x


def feistel(v, hb, k0, k1):
    """ds_feistel (sample_kernels.hip:37-47): the keyed bijection of [0, 2^(2 hb)), four balanced rounds."""
    v = _u(v)
    mask = np.uint64((1 << hb) - 1)
    l, r = v >> np.uint64(hb), v & mask
    for rnd in range(4):
        key = ((int(k0) + 0x9e3779b9 * rnd) & M32) ^ ((int(k1) << (rnd & 3)) & M32)
        f = hash32(r ^ np.uint64(key)) & mask
        l, r = r, l ^ f
    return (l << np.uint64(hb)) | r


def keys(seed, set):
    """(k0, k1) of k_dsurf_select (sample_kernels.hip:88): the two sets walk different permutations of one seed."""
    seed = int(seed)
    k0 = int(hash32((seed & M32) ^ (0xa511e9b3 if set else 0x1f83d9ab)))
    k1 = int(hash32(((seed >> 32) + 0x5be0cd19 * (set + 1)) & M32))
    return k0, k1


def half_bits(total):
    """fill_dsurf (sample_kernels.hip:141-143): the smallest hb >= 1 with 4^hb >= total."""
    hb = 1
    while (1 << (2 * hb)) < total:
        hb += 1
    return hb


def permute(k, total, seed, set):
    """The pixel the walk visits at position k (sample_kernels.hip:96-97): feistel, repeated while the value is >= total (cycle walking)."""
    hb = half_bits(total)
    k0, k1 = keys(seed, set)
    v = feistel(k, hb, k0, k1)
    out = np.atleast_1d(v).copy()
    todo = np.nonzero(out >= total)[0]
    while todo.size:
        out[todo] = feistel(out[todo], hb, k0, k1)
        todo = todo[out[todo] >= total]
    return out.astype(np.int64).reshape(np.shape(v))


def permutation(total, seed, set):
    """The whole walk: a bijection of [0, total)."""
    return permute(np.arange(total, dtype=np.uint64), total, seed, set)


def uniform(seed, pix, c):
    """ds_uniform (sample_kernels.hip:48-51): float32 in [0, 1), a multiple of 2^-24 -- exact, (h >> 8) has 24 bits."""
    seed = int(seed)
    h = hash32((hash32(_u(pix) ^ np.uint64(seed & M32)) + np.uint64((0x632be5ab * (c + 1) + (seed >> 32)) & M32)) & np.uint64(M32))
    return ((h >> np.uint64(8)).astype(np.float64) / 16777216.0).astype(np.float32)


def jitter64(seed, pix, jitter_rad):
    """ds_jitter (sample_kernels.hip:75-77) in float64 on the float32 value of jitter_rad: uniform * 2 jitter_rad - jitter_rad, [len(pix),3]."""
    jr = float(np.float32(jitter_rad))
    return np.stack([uniform(seed, pix, c).astype(np.float64) * (2.0 * jr) - jr for c in range(3)], -1)


def _unproject(depths, kinv, einv, size, center, dt):
    """ds_point (sample_kernels.hip:54-74) on every pixel in the number type `dt`, one numpy operation per operation of the kernel in its order."""
    d = np.asarray(depths).astype(dt)
    N, H, W = d.shape
    K = np.asarray(kinv).astype(dt).reshape(N, 9)[:, :, None, None]
    E = np.asarray(einv).astype(dt).reshape(N, 16)[:, :, None, None]
    cen = np.asarray(center).astype(dt).reshape(-1)
    s = np.asarray(size).astype(dt).reshape(-1)[0]
    eps = np.float32(1e-9).astype(dt)                                               # the kernel's 1e-9f
    half, two = dt(0.5), dt(2.0)
    u = (np.arange(W).astype(dt) + half)[None, None, :]
    v = (np.arange(H).astype(dt) + half)[None, :, None]
    ic = [K[:, 3 * i] * u + K[:, 3 * i + 1] * v + K[:, 3 * i + 2] for i in range(3)]
    zi = ic[2] + eps
    hom = [ic[i] / zi * d for i in range(3)]
    wv = [E[:, 4 * i] * hom[0] + E[:, 4 * i + 1] * hom[1] + E[:, 4 * i + 2] * hom[2] + E[:, 4 * i + 3] for i in range(4)]   # hom[3] = 1: the product is exact
    ww = wv[3] + eps
    p = np.stack([(wv[i] / ww - cen[i]) / s * two for i in range(3)], -1)
    assert p.dtype == dt
    return p


def points64(depths, kinv, einv, size, center):
    """-> (points float64 [N,H,W,3], valid bool [N,H,W] = depth > 0): ds_point's formula in float64 on the inputs as given (the kernel's float32 ones)."""
    return _unproject(depths, kinv, einv, size, center, np.float64), np.asarray(depths) > 0


def points32(depths, kinv, einv, size, center):
    """The same in float32, unfused: how far one float32 evaluation of the formula lies from its float64 value.  Sizes the tolerance only."""
    return _unproject(np.asarray(depths, np.float32), np.asarray(kinv, np.float32), np.asarray(einv, np.float32), np.asarray(size, np.float32),
                      np.asarray(center, np.float32), np.float32)


def point_tolerance(scene):
    """-> (tol, e32): e32 = max |points32 - points64| over the valid pixels; tol = max(2e-5, 4 e32).  2e-5 is what test_gpu_step.py allows at this scale;
    the factor 4 covers the compiler contracting multiply-adds, which changes which roundings happen but not their size."""
    a = (scene['depths'], scene['kinv'], scene['einv'], scene['size'], scene['center'])
    p64, valid = points64(*a)
    e32 = float(np.abs(points32(*a).astype(np.float64) - p64)[valid].max()) if valid.any() else 0.0
    return max(2e-5, 4.0 * e32), e32


def eligible(depths, kinv, einv, size, center, bb, jitter_rad, seed):
    """-> (elig bool [2][total], points64 [total,3], valid [total]): set 0 = valid and on-surface point inside the box (ds_inbound, sample_kernels.hip:78-80),
    set 1 = valid and the jittered point inside it (sample_kernels.hip:99-102)."""
    p, valid = points64(depths, kinv, einv, size, center)
    p, valid = p.reshape(-1, 3), valid.reshape(-1)
    bb = float(np.float32(bb))
    q = p + jitter64(seed, np.arange(p.shape[0]), jitter_rad)
    return np.stack([valid & (np.abs(p) < bb).all(-1), valid & (np.abs(q) < bb).all(-1)]), p, valid


def first_n(elig, seed, set, n, chunk=1 << 16):
    """The first n eligible pixels in walk order (k_dsurf_select's compaction, sample_kernels.hip:91-116) -> (idx int64 [n] padded with FILL, count)."""
    total = elig.shape[0]
    got, have = [], 0
    for k0 in range(0, total, chunk):
        pix = permute(np.arange(k0, min(k0 + chunk, total), dtype=np.uint64), total, seed, set)
        pix = pix[elig[pix]]
        got.append(pix)
        have += pix.size
        if have >= n:
            break
    sel = np.concatenate(got)[:n] if got else np.zeros(0, np.int64)
    idx = np.full(n, FILL, np.int64)
    idx[:sel.size] = sel
    return idx, int(sel.size)


def select(depths, kinv, einv, size, center, bb, jitter_rad, seed, n):
    """-> (idx int64 [2][n] in walk order, FILL past the count; counts int64 [2])."""
    elig, _, _ = eligible(depths, kinv, einv, size, center, bb, jitter_rad, seed)
    r = [first_n(elig[s], seed, s, n) for s in range(2)]
    return np.stack([r[0][0], r[1][0]]), np.array([r[0][1], r[1][1]], np.int64)


def select_scene(scene, bb, jitter_rad, seed, n):
    return select(scene['depths'], scene['kinv'], scene['einv'], scene['size'], scene['center'], bb, jitter_rad, seed, n)


def _look_at(eye, up=(0.0, 0.0, 1.0)):
    z = -eye / np.linalg.norm(eye)
    x = np.cross(z, np.asarray(up))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    E = np.eye(4)
    E[:3, :3] = np.stack([x, y, z])
    E[:3, 3] = -E[:3, :3] @ eye
    return E


def make_scene(N, H, W, seed, valid_fraction):
    """Float32 depth maps of the unit sphere (bumpy: the depth of every pixel scaled by 0.94 .. 1.06) seen by N distinct cameras, with holes.
    Scale of the dsurf_unproject fixture: size 2, center 0 (normalised = world coordinates), depths of about 1 to 3, meant for bb = 1.  Every view has its
    own focal length, principal point, distance, height and azimuth, so the unprojection of a pixel through another view's matrices is far off.  The focal
    length puts the whole image inside the sphere's outline (every pixel has a depth before the holes); view 0 looks along -x at the point (1, 0, 0),
    so its surface straddles the face x = 1 of the box: part outside, part within the jitter radius of the face.
    -> dict: depths [N,H,W], depth_cams [N,2,4,4], kinv [N,3,3], einv [N,4,4] (the inverses ops.dsurf_samples takes of depth_cams), size [1], center [3]."""
    rs = np.random.RandomState(seed)
    depths = np.zeros((N, H, W), np.float32)
    cams = np.zeros((N, 2, 4, 4), np.float32)
    xs, ys = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    for n in range(N):
        az = 0.05 + 2 * np.pi * n / N + 0.37 * n
        dist, height = 2.5 + 0.2 * n, 0.1 + 0.25 * n
        eye = np.array([dist * np.cos(az), dist * np.sin(az), height])
        E = _look_at(eye)
        f = (1.9 + 0.15 * n) * max(H, W)
        K = np.array([[f, 0.0, W / 2.0 + 0.3 * n], [0.0, f * (1.0 + 0.02 * n), H / 2.0 - 0.2 * n], [0.0, 0.0, 1.0]])
        cams[n, 0] = E
        cams[n, 1, :3, :3] = K
        cams[n, 1, 3, 3] = 1.0
        dirs = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs)], -1) @ E[:3, :3]      # world directions, camera z = 1
        a, b, c = (dirs * dirs).sum(-1), 2 * (dirs @ eye), eye @ eye - 1.0
        disc = b * b - 4 * a * c
        tz = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0.0))) / (2 * a), 0.0)
        tz = tz * rs.uniform(0.94, 1.06, size=tz.shape)
        tz[rs.uniform(size=tz.shape) >= valid_fraction] = 0.0
        depths[n] = tz
    c64 = cams.astype(np.float64)
    return {'depths': depths, 'depth_cams': cams, 'kinv': np.linalg.inv(c64[:, 1, :3, :3]).astype(np.float32),
            'einv': np.linalg.inv(c64[:, 0]).astype(np.float32), 'size': np.array([2.0], np.float32), 'center': np.zeros(3, np.float32)}


def clear_band(scene, seed, bb, jitter_rad, band):
    """Set the depth to 0 (in place) at every valid pixel whose on-surface or jittered point has a coordinate within `band` of +-bb in float64: afterwards
    no float32 rounding below `band` changes any pixel's eligibility.  A condition on the input; -> the fraction of the valid pixels cleared."""
    p, valid = points64(scene['depths'], scene['kinv'], scene['einv'], scene['size'], scene['center'])
    shape = valid.shape
    p, valid = p.reshape(-1, 3), valid.reshape(-1)
    q = p + jitter64(seed, np.arange(p.shape[0]), jitter_rad)
    bb = float(np.float32(bb))
    near = (np.abs(np.abs(p) - bb) < band).any(-1) | (np.abs(np.abs(q) - bb) < band).any(-1)
    clear = valid & near
    scene['depths'][clear.reshape(shape)] = 0.0
    return float(clear.sum()) / max(int(valid.sum()), 1)


# The scenes of tests/test_gpu_dsurf.py: name -> (N, H, W, seed, valid_fraction)
SCENES = {
    't1': (1, 1, 1, 1, 1.0),                      # half width 1
    't3': (1, 1, 3, 2, 1.0),                      # half width 1, one value of the domain rejected
    't5': (1, 1, 5, 3, 1.0),                      # half width 2
    't1023': (3, 11, 31, 4, 1.0),                 # below one round of 1024 candidates: lanes past the end
    't1023_sparse': (3, 11, 31, 5, 0.05),
    't1024': (1, 32, 32, 6, 1.0),                 # 4^5: no cycle walking
    't1025': (1, 25, 41, 7, 1.0),                 # 4^5 + 1: three quarters of the domain rejected
    't2049': (1, 3, 683, 8, 1.0),                 # two full rounds of 1024 candidates and a third with one
    't2049_sparse': (1, 3, 683, 9, 0.05),
    't2304': (3, 24, 32, 10, 1.0),                # the shape of the dsurf_unproject fixture
    't2304_holes': (3, 24, 32, 11, 0.7),
    'mega': (2, 1025, 512, 12, 1.0),              # 2^20 + 1024 pixels: half width 11, a real scene's pool
    'mega_sparse': (2, 1025, 512, 13, 0.05),
}

BIG_BB = 1e3                                       # every valid pixel in the box, nothing near a face
LISTED_N = (1, 63, 64, 65, 1023, 1024, 1025, 2500)  # around one wave (64 lanes), one round (1024 candidates) and the workload's n above it
# The selection cases: name -> (scene, bb, jitter_rad, sampler seed, e_min).  e_min is the smaller of the two sets' eligible counts once the band is
# cleared (tests/test_dsurf_ref_host.py holds it to what `prepare` finds); `case_ns` derives the n of a case from it.
CASES = {
    't1': ('t1', BIG_BB, 0.1, 5, 1),
    't3': ('t3', BIG_BB, 0.1, 0, 3),
    't5': ('t5', BIG_BB, 0.1, (1 << 62) - 1, 5),
    't1023': ('t1023', BIG_BB, 0.1, 0x123456789abcdef, 1023),
    't1023_sparse': ('t1023_sparse', BIG_BB, 0.1, 77, 45),
    't1024': ('t1024', BIG_BB, 0.1, 5, 1024),
    't1025': ('t1025', BIG_BB, 0.1, 0, 1025),
    't2049': ('t2049', BIG_BB, 0.1, 1234567, 2049),
    't2049_sparse': ('t2049_sparse', 1.0, 0.1, 31337, 50),
    't2304_faces': ('t2304', 1.0, 0.1, 424242, 1891),
    't2304_holes': ('t2304_holes', 1.0, 0.1, (7 << 32) | 9, 1273),
    't2304_nojitter': ('t2304_holes', 1.0, 0.0, 99, 1352),
    'mega': ('mega', BIG_BB, 0.1, 2024, 1049600),
    'mega_sparse': ('mega_sparse', 1.0, 0.1, (3 << 40) | 17, 40866),
    'mega_nojitter': ('mega_sparse', 1.0, 0.0, 4, 42958),
}
DIFFERING = ('t2049_sparse', 't2304_faces', 't2304_holes', 'mega_sparse')           # bb = 1 with jitter: the two sets hold different numbers of pixels


def case_ns(case):
    """The n a case is drawn with: every LISTED_N the smaller set can fill, then 'all' = the eligible count of set 0 (the walk's last eligible candidate
    completes the set), 'all+1' = one more (counts report the shortfall) and, where the sets differ in size, 'min+1' = one more than the smaller set."""
    e_min = CASES[case][4]
    return tuple(n for n in LISTED_N if n <= e_min) + ('all', 'all+1') + (('min+1',) if case in DIFFERING else ())


_prepared = {}


def prepare(case):
    """-> (scene with the band cleared, tol, e32, cleared fraction, elig [2][total], points64 [total,3]) of a CASES entry; built once per process and
    shared (read-only) by the tests that need it."""
    if case not in _prepared:
        name, bb, jr, seed, _ = CASES[case]
        scene = {k: v.copy() for k, v in make_scene(*SCENES[name]).items()}
        tol, e32 = point_tolerance(scene)
        cleared = clear_band(scene, seed, bb, jr, 10.0 * tol)
        elig, p64, _ = eligible(scene['depths'], scene['kinv'], scene['einv'], scene['size'], scene['center'], bb, jr, seed)
        for v in scene.values():
            v.setflags(write=False)
        _prepared[case] = (scene, tol, e32, cleared, elig, p64)
    return _prepared[case]


def resolve_n(n, elig):
    """'all' / 'all+1' / 'min+1' of a CASES entry -> int"""
    e0, e1 = int(elig[0].sum()), int(elig[1].sum())
    return {'all': e0, 'all+1': e0 + 1, 'min+1': min(e0, e1) + 1}.get(n, n)
