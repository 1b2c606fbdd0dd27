"""tests/dsurf_ref.py, the numpy restatement of the phase-0 depth-surface sampler, checked on the CPU: the walk is a bijection, the jitter is what
it claims, the unprojection agrees with the oracle that is pinned to the reference, and the scenes of tests/test_gpu_dsurf.py lose at most 2 % of
their valid pixels to the band that makes an exact comparison of the selection possible."""
import numpy as np
import pytest

import dsurf_ref as R
from conftest import golden

SEEDS = (0, 5, (1 << 62) - 1, (0x9d2c5680 << 32) | 0x3c6ef372)
TOTALS = (1, 2, 3, 4, 5, 16, 17, 1023, 1024, 1025, 2304, 4096, 4097, 65537, (1 << 20) + 1)


@pytest.mark.parametrize('total', TOTALS)
def test_permutation_is_a_bijection(total):
    perms = {}
    for seed in SEEDS:                                                              # (the million-element walk: about half a second per seed and set)
        for s in (0, 1):
            p = R.permutation(total, seed, s)
            assert p.shape == (total,) and p.dtype == np.int64
            assert np.array_equal(np.sort(p), np.arange(total)), (total, seed, s)
            perms[seed, s] = p
    if total >= 17:                                                                 # the two sets, and two seeds, walk different permutations
        for seed in SEEDS:
            assert not np.array_equal(perms[seed, 0], perms[seed, 1])
        for seed in SEEDS[1:]:
            assert not np.array_equal(perms[0, 0], perms[seed, 0])


def test_half_bits_and_hash():
    assert [R.half_bits(n) for n in (1, 4, 5, 16, 17, 1024, 1025, 4096, 4097, (1 << 20) + 1, (1 << 30) - 1)] == [1, 1, 2, 2, 3, 5, 6, 6, 7, 11, 15]
    assert int(R.hash32(0)) == 0                                                    # lowbias32 is xor-shifts and odd multiplications: 0 stays 0
    x = np.arange(1 << 16, dtype=np.uint64) * np.uint64(65537)
    assert np.unique(R.hash32(x)).size == x.size                                    # a bijection of uint32: no collisions
    assert int(R.hash32(x).max()) <= R.M32
    for hb in (1, 2, 5):                                                            # the Feistel network alone is a bijection of its domain
        dom = np.arange(1 << (2 * hb), dtype=np.uint64)
        assert np.array_equal(np.sort(R.feistel(dom, hb, 0xdeadbeef, 0x12345678)), dom)


def test_uniform():
    pix = np.arange(5000)
    us = {}
    for seed in SEEDS:
        for c in range(3):
            u = R.uniform(seed, pix, c)
            assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
            assert np.array_equal(u.astype(np.float64) * 16777216.0, np.round(u.astype(np.float64) * 16777216.0))   # multiples of 2^-24
            assert 0.45 < float(u.mean()) < 0.55
            us[seed, c] = u
        assert (us[seed, 0] != us[seed, 1]).mean() > 0.99 and (us[seed, 1] != us[seed, 2]).mean() > 0.99 and (us[seed, 0] != us[seed, 2]).mean() > 0.99
    assert (us[0, 0] != us[5, 0]).mean() > 0.99                                     # the low half of the seed
    assert (R.uniform(5, pix, 0) != R.uniform(5 | (1 << 40), pix, 0)).mean() > 0.99  # and the high half
    j = R.jitter64(5, pix, 0.1)
    assert j.shape == (5000, 3) and np.abs(j).max() <= float(np.float32(0.1)) and np.abs(j).max() > 0.099
    assert np.all(R.jitter64(5, pix, 0.0) == 0.0)


def _fixture():
    from oracle import oracle_np as ON
    g = golden('dsurf_unproject')
    depths = g['depths'].reshape(-1, *g['depths'].shape[-2:])
    cams = g['depth_cams'].reshape(-1, 2, 4, 4).astype(np.float64)
    kinv, einv = np.linalg.inv(cams[:, 1, :3, :3]), np.linalg.inv(cams[:, 0])
    ref, valid = ON.dsurf_unproject(depths, cams, g['size'][:1], g['center'][:1])
    return g, depths, kinv, einv, ref, valid


def test_points64_vs_oracle_np_on_the_fixture():
    """oracle_np.dsurf_unproject is pinned to the reference by test_oracle_np_golden.py; points64 on the same float64 inverses is the same formula."""
    g, depths, kinv, einv, ref, valid = _fixture()
    p, v = R.points64(depths, kinv, einv, g['size'][:1], g['center'][:1])
    assert np.array_equal(v, valid) and np.array_equal(v, g['valid'])
    assert np.abs(p - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    # float32 inverses (what the kernel gets) move the points by float32 rounding only, and points32 stays within a few ulp of points64
    k32, e32_ = kinv.astype(np.float32), einv.astype(np.float32)
    p_in, _ = R.points64(depths, k32, e32_, g['size'][:1], g['center'][:1])
    assert np.abs(p_in - ref)[valid].max() < 2e-6
    p32 = R.points32(depths, k32, e32_, g['size'][:1], g['center'][:1])
    assert p32.dtype == np.float32 and np.abs(p32 - p_in)[valid].max() < 2e-6


def test_select_on_the_fixture():
    g, depths, kinv, einv, ref, valid = _fixture()
    k32, e32_ = kinv.astype(np.float32), einv.astype(np.float32)
    scene = {'depths': depths.copy(), 'kinv': k32, 'einv': e32_, 'size': g['size'][:1], 'center': g['center'][:1]}
    bb, jr, seed, n = float(g['bb']), 0.1, 1234567, 256
    cleared = R.clear_band(scene, seed, bb, jr, 1e-3)
    print('dsurf_unproject fixture: a band of 1e-3 clears %.4f of the valid pixels' % cleared)
    assert 0 < cleared <= 0.02
    idx, counts = R.select_scene(scene, bb, jr, seed, n)
    assert counts.tolist() == [n, n] and idx.shape == (2, n)
    p = ref.reshape(-1, 3)
    inb = (np.abs(p) < bb).all(-1) & (scene['depths'].reshape(-1) > 0)
    for s in range(2):
        assert np.unique(idx[s]).size == n and idx[s].min() >= 0 and idx[s].max() < p.shape[0]
        assert (scene['depths'].reshape(-1)[idx[s]] > 0).all()
    assert inb[idx[0]].all()
    q = p[idx[1]] + np.stack([R.uniform(seed, idx[1], c).astype(np.float64) * 0.2 - 0.1 for c in range(3)], -1)
    assert (np.abs(q) < bb).all()
    assert not np.array_equal(np.sort(idx[0]), np.sort(idx[1]))
    # a set is a prefix of the walk's eligible pixels: a smaller n is a prefix of a larger one, and asking for too many reports the shortfall
    idx2, counts2 = R.select_scene(scene, bb, jr, seed, 100)
    assert np.array_equal(idx2, idx[:, :100]) and counts2.tolist() == [100, 100]
    idx3, counts3 = R.select_scene(scene, bb, jr, seed, 5000)
    assert counts3[0] == inb.sum() and np.array_equal(np.sort(idx3[0, :counts3[0]]), np.nonzero(inb)[0]) and (idx3[0, counts3[0]:] == R.FILL).all()


@pytest.mark.parametrize('case', sorted(R.CASES))
def test_clear_band_clears_at_most_two_percent(case):
    scene, tol, e32, cleared, elig, p64 = R.prepare(case)
    name, bb, jr, seed, e_min = R.CASES[case]
    print('%s: e32 %.3g, tol %.3g, band %.3g clears %.4f of the valid pixels; eligible %d / %d' % (case, e32, tol, 10 * tol, cleared, elig[0].sum(), elig[1].sum()))
    assert tol >= 2e-5 and tol >= 4 * e32 and e32 < 1e-6
    assert cleared <= 0.02
    # nothing eligible or not by less than the band any more
    valid = scene['depths'].reshape(-1) > 0
    q = p64 + R.jitter64(seed, np.arange(p64.shape[0]), jr)
    assert np.abs(np.abs(p64[valid]) - bb).min() >= 10 * tol and np.abs(np.abs(q[valid]) - bb).min() >= 10 * tol
    # the table's eligible count is the scene's, so case_ns draws every listed n the scene can fill and no other
    e0, e1 = int(elig[0].sum()), int(elig[1].sum())
    assert e_min == min(e0, e1) >= 1 and (e0 != e1) == (case in R.DIFFERING)
    ns = R.case_ns(case)
    assert [n for n in ns if isinstance(n, int)] == [n for n in R.LISTED_N if n <= min(e0, e1)]
    assert set(ns) - set(R.LISTED_N) == {'all', 'all+1'} | ({'min+1'} if e0 != e1 else set())
    if bb == 1.0:                                                                   # the scene does what make_scene promises: surface outside the box ...
        out = valid & ~(np.abs(p64) < bb).all(-1)
        assert out.sum() > 0.02 * valid.sum()
        if jr > 0:                                                                  # ... and within the jitter radius of a face, so that the two sets differ
            assert (elig[0] & ~elig[1]).any() and (elig[1] & ~elig[0]).any()


def test_make_scene_views_are_distinct():
    s = R.make_scene(3, 24, 32, 10, 1.0)
    assert s['depths'].dtype == np.float32 and (s['depths'] > 0).all() and 1.0 < s['depths'].min() and s['depths'].max() < 3.0
    for a in range(3):
        for b in range(a + 1, 3):
            assert np.abs(s['kinv'][a] - s['kinv'][b]).max() > 1e-4 and np.abs(s['einv'][a] - s['einv'][b]).max() > 0.1
    p, _ = R.points64(s['depths'], s['kinv'], s['einv'], s['size'], s['center'])
    r = np.linalg.norm(p, axis=-1)
    assert 0.85 < r.min() and r.max() < 1.15                                        # the bumpy unit sphere, seen from every view
    wrong, _ = R.points64(s['depths'], np.roll(s['kinv'], 1, 0), np.roll(s['einv'], 1, 0), s['size'], s['center'])
    assert np.abs(wrong - p).max(-1).min() > 0.05                                   # a wrong view index moves every point
