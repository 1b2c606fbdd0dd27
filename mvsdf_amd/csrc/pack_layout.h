// pack_layout.h -- THE definition of the operand layout every matrix-core kernel reads: the sizes of the packs, the lane-order fragment maps, the bf16 rounding
// and the three-term split.  basic.hip's pack kernels and every pack loop of k_step_prologue take their (row, k) and their values from here; the tile engines,
// the x3 chains and k_wgrad read what they write.  No HIP in here: tests/test_pack_layout_host.py compiles this header alone with the host compiler and holds
// packs built from it to tests/pack_ref.py.
//
// A pack of a matrix W (out = N, in = K; 0 outside N x K) is a row-major array of BLOCKS of 16 rows; inside a block the elements stand in FRAGMENT order:
//   fp32 (v_mfma_f32_16x16x4_f32): N padded to 16, K to 32 (an EVEN number of 16-wide k-blocks: the 2x-unrolled pipelined loop has no tail), 256-element blocks,
//       wp[ct][kb][lane][s] = W[16 ct + (lane & 15)][16 kb + 4 s + (lane >> 4)]
//     one 16-byte load per lane yields the B operands of the four k-steps of a k-block, issued in ascending k: a k-ascending fmaf chain from 0;
//   bf16 (v_mfma_f32_16x16x32_bf16): N padded to 16, K to 32, 512-element blocks,
//       wp16[ct][kb][lane][i] = bf16(W[16 ct + (lane & 15)][32 kb + 8 (lane >> 4) + i])
//   three-term bf16: the bf16 layout with the three term fragments of a k-block behind each other, block ((ct KB + kb) 3 + term).
// The pack of W^T (contraction over the OUT dimension) is the same formula on W^T.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MV_LAYOUT_FN __host__ __device__ static inline
#else
#define MV_LAYOUT_FN static inline
#endif

// ---- sizes
MV_LAYOUT_FN int mv_ceil16(int x) { return (x + 15) & ~15; }
MV_LAYOUT_FN int mv_kpad(int x) { return (x + 31) & ~31; }
MV_LAYOUT_FN size_t mv_packed_floats(int N, int K) { return (size_t)mv_ceil16(N) * mv_kpad(K); }
MV_LAYOUT_FN int mv_bf_kb(int K) { return (K + 31) / 32; }                                          // k-blocks of 32
MV_LAYOUT_FN size_t mv_packed_bf16_elems(int N, int K) { return (size_t)mv_ceil16(N) * mv_bf_kb(K) * 32; }   // x 3 for the three-term pack

// ---- fragment maps: element e of a block <-> (row 0..15, k offset inside the k-block)
struct MvFrag { int row, k; };
MV_LAYOUT_FN MvFrag mv_frag_f32(int e) { const int s = e & 3, lane = e >> 2; return MvFrag{lane & 15, 4 * s + (lane >> 4)}; }                // e < 256, k < 16
MV_LAYOUT_FN int mv_frag_f32_at(int row, int k) { return (16 * (k & 3) + row) * 4 + (k >> 2); }
MV_LAYOUT_FN MvFrag mv_frag_bf16(int e) { const int i = e & 7, lane = e >> 3; return MvFrag{lane & 15, 8 * (lane >> 4) + i}; }               // e < 512, k < 32
MV_LAYOUT_FN int mv_frag_bf16_at(int row, int k) { return (16 * (k >> 3) + row) * 8 + (k & 7); }
// ---- block order: block (ct, kb[, term]) of a pack with KB k-blocks per tile row <-> its index.  (k_step_prologue knows its ct or kb and never divides.)
struct MvBlock { int ct, kb, term; };
MV_LAYOUT_FN size_t mv_block_index(int ct, int kb, int KB, int term = 0, int terms = 1) { return ((size_t)ct * KB + kb) * terms + term; }
MV_LAYOUT_FN MvBlock mv_block_at(size_t blk, int KB, int terms = 1) { return MvBlock{(int)(blk / terms / KB), (int)(blk / terms % KB), (int)(blk % terms)}; }

// ---- values
MV_LAYOUT_FN uint16_t mv_f2bf(float f) {     // round to nearest even (finite inputs)
    uint32_t u;
#ifdef __HIP_DEVICE_COMPILE__
    u = __float_as_uint(f);
#else
    __builtin_memcpy(&u, &f, 4);
#endif
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
MV_LAYOUT_FN float mv_bf2f(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
#ifdef __HIP_DEVICE_COMPILE__
    return __uint_as_float(u);
#else
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
#endif
}
MV_LAYOUT_FN float mv_bf_round(float w) { return mv_bf2f(mv_f2bf(w)); }     // the rounded fp32 pack's value (trace_dtype 2)
// Every value that enters the three-term arithmetic is first flushed to zero below 2^-40: no bf16 term is ever denormal and every product stays above 2^-112,
// the range on which the oracle's model of the matrix instruction is verified (tile_engine_bf16s.h).
#define MV_X3_FLUSH 9.094947017729282e-13f                          // 2^-40
MV_LAYOUT_FN float mv_x3_flush(float v) { return fabsf(v) < MV_X3_FLUSH ? 0.0f : v; }
// term 0..2 of the three-term split  w = t0 + t1 + t2:  t0 = bf16(flush(w)), t1 = bf16(w - t0), t2 = bf16(w - t0 - t1); every subtraction is exact in fp32
MV_LAYOUT_FN uint16_t mv_x3_term(float w, int term) {
    float r = mv_x3_flush(w);
    uint16_t v = mv_f2bf(r);
    for (int t = 0; t < term; ++t) { r = r - mv_bf2f(v); v = mv_f2bf(r); }
    return v;
}
