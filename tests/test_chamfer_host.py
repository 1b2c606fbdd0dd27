"""DTU Chamfer evaluation without a GPU: tests/chamfer_ref.py against the fixtures tests/golden/chamfer/*.npz (DTUeval-python's formulation under
the seeded order), the kept set's invariants and border cases, the loaders and the CLI paths of tools/eval_dtu.py that need no GPU."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import chamfer_ref
from conftest import GOLDEN, ROOT

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, 'chamfer', '*.npz')))


def _fixture(path):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def test_fixtures_exist():
    assert {os.path.basename(p) for p in FIXTURES} >= {'mesh.npz', 'pcd_seed0.npz', 'pcd_seed7.npz'}


@pytest.mark.parametrize('path', FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_restatement_equals_the_fixture(path):
    z = _fixture(path)
    kw = dict(density=float(z['density']), patch=z['patch'].item(), max_dist=float(z['max_dist']), seed=int(z['seed']))
    r = chamfer_ref.dtu_chamfer(z.get('points'), z['stl'], z['obs_mask'], z['bb'], float(z['res']), z['plane'], verts=z.get('verts'),
                                faces=z.get('faces'), **kw)
    assert np.array_equal(r['points'].view(np.int64), z['samples'].view(np.int64))
    assert np.array_equal(r['kept'], z['kept']) and np.array_equal(r['in'], z['in']) and np.array_equal(r['obs'], z['obs'])
    assert np.array_equal(chamfer_ref.above(z['stl'], z['plane']), z['above'])
    for name in ('d2s', 's2d'):
        got, fix = r['dist_' + name], z['dist_' + name]
        assert np.array_equal(np.isinf(got), np.isinf(fix))
        fin = np.isfinite(fix)
        assert np.all(np.abs(got[fin] - fix[fin]) <= 1e-12 * fix[fin])
        assert abs(r['mean_' + name] - float(z['mean_' + name])) <= 1e-12 * float(z['mean_' + name])
    assert abs(r['overall'] - float(z['overall'])) <= 1e-12 * float(z['overall'])
    # the fixtures reach the cases they are meant to: distances beyond the cut-off, points outside the box and outside the mask
    assert np.isinf(z['dist_d2s']).any() or np.isinf(z['dist_s2d']).any()
    assert (~z['in']).any() and (z['in'] & ~z['obs']).any()


def test_fixture_border_cases_are_present():
    z = _fixture(os.path.join(GOLDEN, 'chamfer', 'pcd_seed0.npz'))
    d = z['samples'][z['kept']][z['in']]
    q = (d - z['bb'][0].astype(np.float32).astype(np.float64)) / float(z['res'])
    assert (np.abs(q - np.floor(q) - 0.5) == 0).any()                       # grid coordinates exactly half-way
    on = ((z['plane'][0] * z['stl'][:, 0] + z['plane'][1] * z['stl'][:, 1]) + z['plane'][2] * z['stl'][:, 2]) + z['plane'][3] == 0
    assert on.any() and not z['above'][on].any()                            # stl points exactly on the plane are not above it
    m = _fixture(os.path.join(GOLDEN, 'chamfer', 'mesh.npz'))
    v, f = m['verts'].astype(np.float64), m['faces']
    cr = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert (np.linalg.norm(cr, axis=1) == 0).any()                          # zero-area faces


def test_splitmix64():
    assert int(chamfer_ref.splitmix64(np.uint64(0))) == 0xE220A8397B1DCDAF   # the generator's first output from state 0
    for seed in (0, 1, 2 ** 63 + 5, 2 ** 64 - 1):
        k = chamfer_ref.keys(200000, seed)
        assert len(np.unique(k)) == len(k)
    x = np.random.RandomState(0).randint(0, 2 ** 63, 100000, dtype=np.int64).astype(np.uint64) * np.uint64(2)
    assert len(np.unique(chamfer_ref.splitmix64(x))) == len(np.unique(x))


def test_library_key_is_splitmix64():
    from mvsdf_amd._lib import lib
    for seed, i in ((0, 0), (0, 12345), (7, 3), (2 ** 64 - 1, 2 ** 40)):
        assert lib().mvsdf_chamfer_key(seed, i) == int(chamfer_ref.splitmix64(np.uint64(seed) ^ np.uint64(i)))


def _check_kept(p, kept, density, seed):
    start, idx = chamfer_ref.neighbours(p, density)
    keys = chamfer_ref.keys(len(p), seed)
    for i in range(len(p)):
        nb = idx[start[i]:start[i + 1]]
        if kept[i]:
            assert not kept[nb].any()                                        # kept points are more than density apart
        else:
            assert (kept[nb] & (keys[nb] < keys[i])).any()                   # a removed point has a lower-key kept point within density


@pytest.mark.parametrize('seed', [0, 3])
def test_kept_set_invariants(seed):
    rs = np.random.RandomState(seed)
    p = np.concatenate([rs.uniform(0, 4, (4000, 3)) * [1, 1, 0.1], rs.uniform(0, 0.05, (50, 3))])
    kept = chamfer_ref.downsample(p, 0.2, seed)
    _check_kept(p, kept, 0.2, seed)
    d = p[kept][:, None, :] - p[kept][None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    np.fill_diagonal(d2, np.inf)
    assert d2.min() > 0.2 * 0.2


def test_downsample_border_cases():
    # exactly at density: inclusive, so only one of the pair survives
    p = np.array([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0]])
    assert chamfer_ref.downsample(p, 0.25, 0).sum() == 1
    assert chamfer_ref.downsample(np.array([[0.0, 0, 0], [0.2500001, 0, 0]]), 0.25, 0).sum() == 2
    # duplicates: the lower key survives
    p = np.array([[1.0, 2.0, 3.0]] * 5)
    kept = chamfer_ref.downsample(p, 0.2, 4)
    assert kept.sum() == 1 and np.argmin(chamfer_ref.keys(5, 4)) == np.nonzero(kept)[0][0]
    # a chain 0.9 * density apart: no two neighbours kept, no gap of three removed
    p = np.zeros((500, 3))
    p[:, 0] = np.arange(500) * 0.18
    kept = chamfer_ref.downsample(p, 0.2, 1)
    assert not (kept[1:] & kept[:-1]).any()
    _check_kept(p, kept, 0.2, 1)


def test_mask_half_way_rounding():
    bb = np.array([[0.0, 0.0, 0.0], [10.0, 10.0, 10.0]])
    d = np.array([[0.25, 0.75, 1.25], [0.5, 0.5, 0.5], [-0.25, 0.0, 0.0], [10.0, 10.0, 10.0]])
    obs = np.zeros((20, 20, 20), bool)
    obs[0, 2, 2] = True                                                      # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2 (half to even)
    obs[1, 1, 1] = True
    inb, ob = chamfer_ref.masks(d, bb, 0.5, obs, patch=0)
    assert inb.tolist() == [True, True, False, False] and ob.tolist() == [True, True, False, False]


def test_sampling_border_cases():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.5, 0, 0], [2, 0, 0], [0, 0.01, 0], [3, 0, 0]], np.float32)
    # a zero-area face (collinear) and a repeated corner add nothing
    assert len(chamfer_ref.sample_mesh(v, [[0, 3, 4]], 0.2)) == len(v)
    assert len(chamfer_ref.sample_mesh(v, [[0, 0, 1]], 0.2)) == len(v)
    # a sliver: l2 < thr gives n2 = 0, so t = 0.5 / 1e-7 and nothing is emitted
    f = np.array([[0, 6, 5]])
    a, b, c = v[0].astype(np.float64), v[6].astype(np.float64), v[5].astype(np.float64)
    l1, l2 = np.linalg.norm(b - a), np.linalg.norm(c - a)
    thr = 0.2 * np.sqrt(l1 * l2 / np.linalg.norm(np.cross(b - a, c - a)))
    assert np.floor(l2 / thr) == 0 and np.floor(l1 / thr) > 0
    assert len(chamfer_ref.sample_mesh(v, f, 0.2)) == len(v)
    # a right triangle with unit legs at density 0.2: n1 = n2 = 5, the (i, j) with (i + 0.5) / 5 + (j + 0.5) / 5 < 1
    s = chamfer_ref.sample_mesh(v, [[0, 1, 2]], 0.2)
    assert len(s) == len(v) + sum(1 for i in range(6) for j in range(6) if (i + 0.5) / 5 + (j + 0.5) / 5 < 1)


def test_nearest_paths_agree():
    rs = np.random.RandomState(2)
    r = rs.uniform(-5, 5, (3000, 3))
    q = np.concatenate([rs.uniform(-6, 6, (2000, 3)), r[:20], r[:20] + [3.0, 0, 0]])
    a = chamfer_ref.nearest(q, r, 1.5)
    b = chamfer_ref.nearest(q, r, 1.5, chunk=128)
    assert np.array_equal(np.isinf(a), np.isinf(b)) and np.array_equal(a[np.isfinite(a)], b[np.isfinite(b)])


def _write_ply(path, fields, rows, faces=None):
    head = ['ply', 'format binary_little_endian 1.0', 'element vertex %d' % len(rows)]
    head += ['property %s %s' % (t, n) for n, t in fields]
    dt = np.dtype([(n, {'float': '<f4', 'double': '<f8', 'uchar': 'u1', 'int': '<i4'}[t]) for n, t in fields])
    a = np.zeros(len(rows), dt)
    for k, (n, _) in enumerate(fields):
        a[n] = [r[k] for r in rows]
    body = a.tobytes()
    if faces is not None:
        head += ['element face %d' % len(faces), 'property list uchar int vertex_indices']
        fa = np.zeros(len(faces), [('n', 'u1'), ('v', '<i4', (3,))])
        fa['n'], fa['v'] = 3, faces
        body += fa.tobytes()
    head += ['end_header', '']
    with open(path, 'wb') as fh:
        fh.write('\n'.join(head).encode('ascii') + body)


def test_load_points(tmp_path):
    from mvsdf_amd.chamfer import load_points
    rows = [(1.5, -2.25, 3.0000001, 255, 7, 0.1), (1e3, 2e-3, -7.0, 0, 0, 0.2)]
    p = tmp_path / 'stl001_total.ply'
    _write_ply(str(p), [('x', 'double'), ('y', 'double'), ('z', 'double'), ('red', 'uchar'), ('green', 'uchar'), ('nx', 'float')], rows)
    got = load_points(str(p))
    assert got.dtype == np.float64 and np.array_equal(got, np.array([r[:3] for r in rows]))
    q = tmp_path / 'f.ply'
    _write_ply(str(q), [('nx', 'float'), ('x', 'float'), ('y', 'float'), ('z', 'float')], [(0, 0.1, 0.2, 0.3), (1, 1.1, 1.2, 1.3)], faces=[[0, 1, 0]])
    assert np.array_equal(load_points(str(q)), np.array([[0.1, 0.2, 0.3], [1.1, 1.2, 1.3]], np.float32).astype(np.float64))
    bad = tmp_path / 'bad.ply'
    bad.write_bytes(b'not a ply')
    with pytest.raises(ValueError):
        load_points(str(bad))


def test_load_dtu_obs(tmp_path):
    sio = pytest.importorskip('scipy.io')
    from mvsdf_amd.chamfer import load_dtu_obs
    (tmp_path / 'ObsMask').mkdir()
    obs = np.random.RandomState(0).rand(5, 6, 7) < 0.5
    bb = np.array([[-1.5, -2.0, 3.0], [4.0, 5.0, 6.25]])
    sio.savemat(str(tmp_path / 'ObsMask' / 'ObsMask24_10.mat'), {'ObsMask': obs.astype(np.uint8), 'BB': bb, 'Res': np.array([[0.2]])})
    sio.savemat(str(tmp_path / 'ObsMask' / 'Plane24.mat'), {'P': np.array([[0.1], [0.2], [0.97], [-3.0]])})
    o, b, res, plane = load_dtu_obs(str(tmp_path), 24)
    assert o.dtype == bool and np.array_equal(o, obs)
    assert b.dtype == np.float32 and np.array_equal(b, bb.astype(np.float32))
    assert res == 0.2 and np.array_equal(plane, [0.1, 0.2, 0.97, -3.0])


def test_product_does_not_import_scipy_at_load():
    code = 'import sys; import mvsdf_amd.chamfer; assert "scipy" not in sys.modules and "sklearn" not in sys.modules'
    subprocess.check_call([sys.executable, '-c', code], cwd=ROOT)


def test_eval_dtu_cli_without_a_gpu(tmp_path):
    tool = os.path.join(ROOT, 'tools', 'eval_dtu.py')
    out = subprocess.run([sys.executable, tool, '--help'], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and '--downsample_density' in out.stdout and '--dataset_dir' in out.stdout
    out = subprocess.run([sys.executable, tool, str(tmp_path / 'missing.ply'), '--scan', '24', '--dataset_dir', str(tmp_path)], capture_output=True,
                         text=True, cwd=ROOT)
    assert out.returncode != 0 and 'no such file' in out.stderr
