"""tests/pack_ref.py against itself, without a GPU: its unpackers (gather: where does the pack hold element (o, k)?) against packers written the other way
round (scatter: which element does flat pack index i hold?), and the three-term split against exact float64 arithmetic on pack_ref.VALUES."""
import numpy as np
import pytest

import pack_ref as PR


def _mat(N, K, seed=0):
    rng = np.random.default_rng(1000 * N + K + seed)
    return PR.plant(rng.standard_normal((N, K)).astype(np.float32), seed)


def _take(W, o, k):
    """W[o, k] where (o, k) lies inside W, +0 elsewhere"""
    N, K = W.shape[-2:]
    inside = (o < N) & (k < K)
    return np.where(inside, W[..., np.minimum(o, N - 1), np.minimum(k, K - 1)], W.dtype.type(0))


def pack_f32(W):
    N, K = W.shape
    KB = PR.kpad(K) // 16
    i = np.arange(PR.ceil16(N) * PR.kpad(K), dtype=np.int64)
    s, lane, blk = i & 3, (i >> 2) & 63, i >> 8
    kb, ct = blk % KB, blk // KB
    return _take(W, 16 * ct + (lane & 15), 16 * kb + 4 * s + (lane >> 4))


def pack_bf16(Wb, terms=1):
    """Wb: uint16 [terms, N, K]"""
    N, K = Wb.shape[-2:]
    KB = PR.kpad(K) // 32
    i = np.arange(terms * PR.ceil16(N) * PR.kpad(K), dtype=np.int64)
    e, lane, blk = i & 7, (i >> 3) & 63, i >> 9
    term, kb, ct = blk % terms, (blk // terms) % KB, blk // terms // KB
    o, k = 16 * ct + (lane & 15), 32 * kb + 8 * (lane >> 4) + e
    inside = (o < N) & (k < K)
    return np.where(inside, Wb[term, np.minimum(o, N - 1), np.minimum(k, K - 1)], np.uint16(0))


@pytest.mark.parametrize('N,K', PR.SHAPES, ids=['%dx%d' % s for s in PR.SHAPES])
def test_unpack_inverts_pack(N, K):
    W = _mat(N, K)
    # fp32
    wp = pack_f32(W)
    assert wp.size == PR.packed_floats(N, K)
    where = PR.where_f32(N, K)
    assert np.array_equal(np.sort(where.reshape(-1)), np.arange(wp.size))               # every pack element holds exactly one (o, k) of the padded matrix
    dense, pads = PR.unpack_f32(wp, N, K)
    assert np.array_equal(PR.bits(dense), PR.bits(W))
    assert pads.size == wp.size - N * K and not PR.bits(wp)[pads].any()
    mark = np.arange(wp.size, dtype=np.int64)                                           # dense and pad indices partition the pack
    dm, pm = PR.unpack_f32(mark, N, K)
    assert np.array_equal(np.sort(np.concatenate([dm.reshape(-1), pm])), mark)
    # bf16, one and three terms
    t3 = PR.split3(W)
    for terms, unpack in ((1, PR.unpack_bf16), (3, PR.unpack_bf16x3)):
        Wb = t3[:terms]
        wp16 = pack_bf16(Wb, terms)
        assert wp16.size == terms * PR.packed_bf16_elems(N, K)
        where = PR.where_bf16(N, K, terms)
        assert np.array_equal(np.sort(where.reshape(-1)), np.arange(wp16.size))
        dense, pads = unpack(wp16, N, K)
        assert np.array_equal(dense.reshape(Wb.shape), Wb)
        assert pads.size == wp16.size - terms * N * K and not wp16[pads].any()
        mark = np.arange(wp16.size, dtype=np.int64)
        dm, pm = unpack(mark, N, K)
        assert np.array_equal(np.sort(np.concatenate([dm.reshape(-1), pm])), mark)


def test_transposed_layouts_differ():
    """a pack of W^T is not a pack of W read differently: the restatement tells them apart (a guard against an unpacker that ignores its dims)"""
    W = _mat(17, 33)
    assert not np.array_equal(pack_f32(W), pack_f32(np.ascontiguousarray(W.T)))
    assert PR.packed_floats(17, 33) != PR.packed_floats(33, 17)


def test_bf16_rounding_ties_to_even():
    b = lambda x: int(PR.bf16_bits(np.array([x], dtype=np.uint32).view(np.float32))[0])
    assert b(0x3f807fff) == 0x3f80 and b(0x3f808000) == 0x3f80 and b(0x3f808001) == 0x3f81      # even bit 16: the tie goes down
    assert b(0x3f817fff) == 0x3f81 and b(0x3f818000) == 0x3f82 and b(0x3f818001) == 0x3f82      # odd bit 16: the tie goes up
    assert b(0x3f7fffff) == 0x3f80 and b(0x7f7f7fff) == 0x7f7f and b(0x7f7f8000) == 0x7f80      # carry into the next binade; the domain's upper end
    assert np.array_equal(PR.bf16_value(PR.bf16_bits(PR.VALUES)), oracle_bf16(PR.VALUES))


def oracle_bf16(a):
    from oracle import oracle
    return oracle.bf16_round(a)


def test_split3_is_exact_and_flushes():
    w = PR.VALUES
    t = PR.split3(w)
    tv = PR.bf16_value(t).astype(np.float64)
    a = np.abs(w.astype(np.float64))
    kept = (a >= 2.0 ** -40) & (a < 2.0 ** 127)
    assert kept.sum() >= 20 and (~kept).sum() >= 10
    assert np.array_equal(tv[0][kept] + tv[1][kept] + tv[2][kept], w.astype(np.float64)[kept])     # float64 holds the three-term sum exactly (<= 3 x 8 bits within 2^-48 of the lead)
    small = a < 2.0 ** -40
    assert small.sum() >= 10 and not t[:, small].any()                                               # +0 bit patterns in every term, for -0 and negative values too
    for s in (0x2b800000, 0xab800000):                                                                # +-2^-40 exactly is kept
        x = np.array([s], dtype=np.uint32).view(np.float32)
        assert PR.split3(x)[:, 0].tolist() == [s >> 16, 0, 0]
    x = np.array([0x3f7fffff], dtype=np.uint32).view(np.float32)                                      # t0 = 1.0, t1 = -2^-24
    assert PR.split3(x)[:, 0].tolist() == [0x3f80, 0xb380, 0]
    big = np.array([0x7f7f7fff, 0xff7f7fff], dtype=np.uint32).view(np.float32)                        # the top of the domain: finite terms that still add up
    tb = PR.bf16_value(PR.split3(big)).astype(np.float64)
    assert np.isfinite(tb).all() and np.array_equal(tb.sum(0), big.astype(np.float64))


def test_split3_on_random_values_is_exact():
    rng = np.random.default_rng(5)
    w = (rng.standard_normal(100000) * np.exp2(rng.integers(-39, 100, 100000))).astype(np.float32)
    w = w[np.abs(w) >= 2.0 ** -40]
    tv = PR.bf16_value(PR.split3(w)).astype(np.float64)
    assert np.array_equal(tv.sum(0), w.astype(np.float64))


def test_fold_is_the_oracle_and_passes_v_through_without_g():
    rng = np.random.default_rng(2)
    v = rng.standard_normal((5, 39)).astype(np.float32)
    g = rng.standard_normal((5, 1)).astype(np.float32)
    w = PR.fold(v, g)
    ref = g.astype(np.float64) * v.astype(np.float64) / np.sqrt((v.astype(np.float64) ** 2).sum(1, keepdims=True))
    assert np.abs(w - ref).max() <= 4 * np.finfo(np.float32).eps * np.abs(ref).max()
    w0 = PR.fold(v, None)
    assert np.array_equal(PR.bits(w0), PR.bits(v)) and w0 is not v


def test_plant_reaches_edges_and_interiors():
    for N, K in ((33, 65), (1, 256), (15, 1)):
        w = PR.plant(np.ones((N, K), dtype=np.float32), 3)
        hit = PR.bits(w) != PR.bits(np.ones((N, K), dtype=np.float32))
        assert hit[0].any() and hit[-1].any() and hit[:, 0].any() and hit[:, -1].any()
    w = PR.plant(np.ones((257, 256), dtype=np.float32), 0)
    assert set(PR.bits(w).reshape(-1).tolist()) >= set(PR.VALUE_BITS.tolist())
    inner = PR.bits(w)[1:15, 1:15] != 0x3f800000
    assert inner.any()
