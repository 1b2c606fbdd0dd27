"""numpy restatement of the weight preparation every matrix-core kernel reads (csrc/basic.hip): the weight-norm fold and the lane-order packs of the folded
weights.  Written from the layout comments of the kernels' headers, as integer index arithmetic over whole arrays (no loop over elements):

  fp32 pack        wp[ct][kb][lane][s]       = W[16 ct + (lane & 15)][16 kb + 4 s + (lane >> 4)],   padded to mv_ceil16(N) x mv_kpad(K)
  bf16 pack        wp16[ct][kb][lane][i]     = bf16(W[16 ct + (lane & 15)][32 kb + 8 (lane >> 4) + i]),   padded to mv_ceil16(N) x 32 ceil(K / 32)
  three-term pack  wp[((ct KB + kb) 3 + term) 64 + lane][i]: the bf16 pack's layout with the three term fragments of a k-block behind each other

The unpackers GATHER: for every element (o, k) of the padded matrix they compute where the pack holds it.  tests/test_pack_ref_host.py checks them against
packers that SCATTER from the flat pack index (written the other way round).  TEST INFRASTRUCTURE: numpy only, no GPU."""
import numpy as np

from oracle import oracle

FLUSH = np.float32(2.0 ** -40)                   # |w| < 2^-40 counts as zero in the three-term packs (pack_layout.h, MV_X3_FLUSH)


def ceil16(x):
    return (x + 15) & ~15


def kpad(x):
    return (x + 31) & ~31


def packed_floats(N, K):
    return ceil16(N) * kpad(K)


def packed_bf16_elems(N, K):
    return ceil16(N) * kpad(K)                   # 32-wide k-blocks: the same padded area, other lane order


# ------------------------------------------------------------------------------------------------ layouts
def _grid(No, Ko):
    return np.meshgrid(np.arange(No, dtype=np.int64), np.arange(Ko, dtype=np.int64), indexing='ij')


def _pads(where, N, K):
    o, k = _grid(*where.shape[-2:])
    return np.sort(where[..., (o >= N) | (k >= K)].reshape(-1))


def where_f32(N, K):
    """[ceil16(N), kpad(K)] -> flat index of element (o, k) inside the fp32 pack"""
    o, k = _grid(ceil16(N), kpad(K))
    KB = kpad(K) // 16
    ct, row, kb, r = o >> 4, o & 15, k >> 4, k & 15
    s, q = r >> 2, r & 3                                        # k = 16 kb + 4 s + q with q = lane >> 4
    lane = 16 * q + row
    return ((ct * KB + kb) * 64 + lane) * 4 + s


def where_bf16(N, K, terms=1):
    """[terms, ceil16(N), 32 ceil(K / 32)] -> flat index of term `term` of element (o, k) inside a bf16 pack with `terms` fragments per k-block"""
    o, k = _grid(ceil16(N), kpad(K))
    KB = kpad(K) // 32
    ct, row, kb, r = o >> 4, o & 15, k >> 5, k & 31
    q, i = r >> 3, r & 7                                        # k = 32 kb + 8 q + i with q = lane >> 4
    lane = 16 * q + row
    term = np.arange(terms, dtype=np.int64)[:, None, None]
    return ((((ct * KB + kb) * terms + term) * 64 + lane) * 8 + i)


def unpack_f32(wp, N, K):
    """fp32 pack (flat array of packed_floats(N, K) elements, any 4-byte dtype) -> (dense [N, K], flat indices of the pad elements)"""
    wp = np.asarray(wp).reshape(-1)
    assert wp.size == packed_floats(N, K), (wp.size, N, K)
    where = where_f32(N, K)
    return wp[where][:N, :K], _pads(where, N, K)


def unpack_bf16(wp16, N, K):
    """bf16 pack (flat uint16 array) -> (dense [N, K] of bf16 bit patterns, flat indices of the pad elements)"""
    wp16 = np.asarray(wp16).reshape(-1)
    assert wp16.size == packed_bf16_elems(N, K), (wp16.size, N, K)
    where = where_bf16(N, K)[0]
    return wp16[where][:N, :K], _pads(where, N, K)


def unpack_bf16x3(wp, N, K):
    """three-term bf16 pack (flat uint16 array) -> (dense [3, N, K] of bf16 bit patterns, term first; flat indices of the pad elements)"""
    wp = np.asarray(wp).reshape(-1)
    assert wp.size == 3 * packed_bf16_elems(N, K), (wp.size, N, K)
    where = where_bf16(N, K, 3)
    return wp[where][:, :N, :K], _pads(where, N, K)


# ------------------------------------------------------------------------------------------------ arithmetic
def bf16_bits(a):
    """float32 -> bf16 bit patterns (uint16), round to nearest even; finite inputs whose rounding stays finite"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf16_value(bits):
    """bf16 bit patterns -> float32"""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def split3(w):
    """The three-term pack's definition: r = +0 where |w| < 2^-40, t0 = bf16(r), t1 = bf16(r - t0), t2 = bf16(r - t0 - t1), every subtraction in
    float32 -> uint16 [3, ...] bit patterns"""
    w = np.ascontiguousarray(w, dtype=np.float32)
    r = np.where(np.abs(w) < FLUSH, np.float32(0.0), w).astype(np.float32)
    t0 = bf16_bits(r)
    r1 = (r - bf16_value(t0)).astype(np.float32)
    t1 = bf16_bits(r1)
    r2 = (r1 - bf16_value(t1)).astype(np.float32)
    t2 = bf16_bits(r2)
    return np.stack([t0, t1, t2])


def fold(v, g):
    """w = g v / |v| per row with orc_fold's operation order (k-ascending fmaf chain, one sqrtf, one division, one multiply per element); g None: w = v"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    return v.copy() if g is None else oracle.fold(v, g)


def bits(a):
    """float32 array -> its uint32 bit patterns (comparisons that tell -0 from +0 and compare NaN payloads)"""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ test shapes and values
# (N, K) of the layers of two multi-layer calls (the bf16 entry points take at most MV_MAXL = 12 layers).  Every N of {1, 3, 15, 16, 17, 31, 32, 33, 217, 257}
# and every K of {1, 3, 31, 32, 33, 39, 63, 64, 65, 217, 256, 289, 512, 575, 576, 577, 640} occurs, plus the pairs (1, 256), (217, 256), (257, 256), (64, 39),
# (512, 512), (3, 577): the smallest shapes on both sides of the fold's 4 rows per workgroup, the 16-row tiles, the 16- and 32-wide k-blocks, the fold's
# 64-lane chunks and the 576-element register path.
SHAPE_GROUPS = (
    ((1, 256), (217, 256), (257, 256), (64, 39), (15, 1), (16, 3), (17, 31), (31, 32), (32, 33), (33, 63)),
    ((512, 512), (3, 577), (15, 64), (16, 65), (17, 217), (31, 289), (32, 575), (33, 576), (3, 640)),
)
SHAPES = SHAPE_GROUPS[0] + SHAPE_GROUPS[1]


def _b(*patterns):
    return [p & 0xffffffff for p in patterns]


_POS = _b(
    0x2b800000,                                     # 2^-40: the flush threshold itself (kept)
    0x2b7ffffe, 0x2b7fffff, 0x2b800001, 0x2b800002,  # its two float32 neighbours on each side
    0x21800000, 0x26c00000, 0x2a123456, 0x2b000000,  # 2^-60, 1.5 * 2^-50, ~2^-43, 2^-41: below the flush
    0x3f7fffff,                                     # t0 rounds up to 1.0 (the next binade), t1 is negative
    0x3f807fff, 0x3f808000, 0x3f808001,             # low halves around the tie under an even bit 16 ...
    0x3f817fff, 0x3f818000, 0x3f818001,             # ... and under an odd one
    0x00800000,                                     # the smallest normal
    0x71800000,                                     # 2^100
    0x7f7f7fff,                                     # the largest float32 whose bf16 rounding stays finite
)
VALUE_BITS = np.array([0x00000000, 0x80000000] + _POS + [p | 0x80000000 for p in _POS], dtype=np.uint32)
VALUES = VALUE_BITS.view(np.float32)


def plant(w, seed=0):
    """VALUES written into a copy of `w` ([N, K] float32): cyclically along the first and last row and column and beside every 16-row / 16-column tile
    edge, and over a random tenth of the rest, so that every pack sees them at tile edges and in interiors."""
    w = np.array(w, dtype=np.float32)
    N, K = w.shape
    o, k = _grid(N, K)
    edge = (o == 0) | (o == N - 1) | (k == 0) | (k == K - 1) | ((o & 15) == 15) | ((o & 15) == 0) | ((k & 15) == 15) | ((k & 15) == 0)
    rng = np.random.default_rng(seed * 7919 + N * 1000 + K)
    sel = edge | (rng.random((N, K)) < 0.1)
    n = int(sel.sum())
    w[sel] = VALUES[(np.arange(n) + seed) % VALUES.size]
    return w
