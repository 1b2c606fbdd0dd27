// wgrad_x3.h -- the network-wide weight gradients (layer_kernels.h: k_wgrad_net) on gfx950's bf16 matrix cores in the THREE-TERM fp32 arithmetic of
// tile_engine_bf16s.h / chain_x3.h ("f32x3"): dW[No][Ki] = sum_rows P[row][o] . Q[row][i], every fp32 element of P and Q split into three bf16 terms
// (mv_split_pk<3>: p = p0 + p1 + p2 exactly; no flush, as in the chains), a product the six exact term products p_s q_j, s + j <= 2, of
// v_mfma_f32_16x16x32_bf16 accumulated in fp32.  The contraction runs over ROWS, 32 per instruction.
//
// The form WG_X3 of the skeleton in layer_kernels.h (block decode, stage loop, slab store, column-sum workgroups, fp32 bias sums); its own:
//   * workgroup = (layer, chunk, 128 x 128 output block), 8 waves, wave (wo, wi) = (w >> 1, w & 1) owns the 2 x 4 accumulator tiles of output rows
//     32 wo .. + 31 and columns 64 wi .. + 63: a quarter of k_wgrad_net's blocks, half its operand re-reads and half the split work per product;
//   * operands are loaded with lane <-> COLUMN: thread (col, g) = (tid & 127, tid >> 7) reads the 8 consecutive rows 8 g .. 8 g + 7 of its column with dword
//     loads (a wave-instruction is 256 contiguous bytes of one row), so leading dimensions and row windows need no alignment and there is ONE staging.  Rows
//     beyond the chunk's end and columns beyond the layer's are CLAMPED to a valid element when read and enter as zero terms (never a padded value times zero);
//   * each element is split ONCE per workgroup, in registers, and its 8 rows x 3 terms go to LDS as three 16-byte pieces: the matrix instruction wants, per
//     lane (q, r), rows 8 q .. 8 q + 7 of column r.  LDS image per operand and term: [g][col] pieces (48 KiB in all) -- the 16 lanes of a ds_read_b128 group
//     read 256 contiguous bytes, the 8 lanes of a ds_write_b128 group write 128: both free of bank conflicts;
//   * one stage = 32 rows = one matrix instruction's contraction.
// Measured on one MI355X (profiles/wgrad_x3_ab.txt): c2 90.8 -> 52.2 us, c3 272.5 -> 176.3 us, the 8x512 shipped step 4.17 -> 2.49 ms per launch.
// Measured and NOT kept:
//   * all twelve Q fragments of a stage in registers at once (130 VGPRs: one workgroup per CU instead of two) -- not run: the form below needs 106;
//   * TWO stages requested ahead in two register sets (126 VGPRs, still two workgroups per CU): 55.2 vs 53.5 us at c2, 188.8 vs 183.9 us at c3 in one job --
//     the exposed load latency is not what bounds the kernel (as k_wgrad_net found).
// Not measured yet: ds_read_b64_tr_b16 on row-major term tiles, 64-row stages, other tiles than 128 x 128.
#pragma once
#include "layer_kernels.h"
#include "tile_engine_bf16s.h"

__global__ __launch_bounds__(WG_X3.THREADS, 2) void k_wgrad_net_x3(WgradNetArgs a) {
    constexpr int TILE = WG_X3.TILE, STAGE = WG_X3.STAGE;
    __shared__ __attribute__((aligned(16))) uint4 T[2][3][4][TILE];               // [P | Q][term][row group g][column]: rows 8 g .. 8 g + 7 of the column, one term
    WgBlock b;
    if (!mv_wg_decode<WG_X3.RUN>(a, (float*)T, b)) return;
    const WgradLayer& L = a.L[b.l];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), r = lane & 15, q = lane >> 4;
    const int i0 = b.bx * TILE, o0 = b.by * TILE, No = L.No, Ki = L.Ki, rbeg = b.rbeg, rend = b.rend;
    const int wo = w >> 1, wi = w & 1;
    f32x4 acc[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.0f;
    const bool do_bias = b.bx == 0;
    CH_PH_DECL
    const int nrb = rend > rbeg ? (rend - rbeg + STAGE - 1) / STAGE : 0, nst = (L.P2 ? 2 : 1) * nrb;
    // staging role: column scol of both operand tiles, rows 8 sg .. 8 sg + 7 of the stage
    const int scol = tid & (TILE - 1), sg = tid >> 7;
    const bool p_in = o0 + scol < No, q_in = i0 + scol < Ki;
    const int pc = min(o0 + scol, No - 1), qc = min(i0 + scol, Ki - 1);
    // a wave whose 32 x 64 corner lies outside the layer has no products to form (it still stages)
    const bool wave_on = o0 + 32 * wo < No && i0 + 64 * wi < Ki;
    float pv[8], qv[8];
    auto issue = [&](int st) {
        const WgOperands s = mv_wg_operands(L, st, nrb, rbeg, STAGE);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int row = min(s.rb + 8 * sg + e, rend - 1);
            pv[e] = s.P[(size_t)row * s.ldp + pc];
            qv[e] = s.Q[(size_t)row * s.ldq + qc];
        }
    };
    auto store = [&](int st) {
        const WgOperands s = mv_wg_operands(L, st, nrb, rbeg, STAGE);
        const int rb = s.rb + 8 * sg;
        uint32_t tp[3][4], tq[3][4];
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
            const bool in0 = rb + e < rend, in1 = rb + e + 1 < rend;
            const dm_f2 hp = dm_f2{(p_in && in0) ? pv[e] : 0.0f, (p_in && in1) ? pv[e + 1] : 0.0f};
            const dm_f2 hq = dm_f2{(q_in && in0) ? qv[e] : 0.0f, (q_in && in1) ? qv[e + 1] : 0.0f};
            if (do_bias && s.pair == 0) bsum += hp.x + hp.y;
            uint32_t sp[3], sq[3];
            mv_split_pk<3>(hp, sp);
            mv_split_pk<3>(hq, sq);
#pragma unroll
            for (int t = 0; t < 3; ++t) { tp[t][e >> 1] = sp[t]; tq[t][e >> 1] = sq[t]; }
        }
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            T[0][t][sg][scol] = uint4{tp[t][0], tp[t][1], tp[t][2], tp[t][3]};
            T[1][t][sg][scol] = uint4{tq[t][0], tq[t][1], tq[t][2], tq[t][3]};
        }
    };
    auto compute = [&](int) {
        if (!wave_on) return;
        // the P fragments of both row tiles stay in registers; the Q fragments of one column tile at a time (all of them at once: 130 VGPRs, one workgroup per CU)
        mv_bf8 pa[2][3];
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int m = 0; m < 2; ++m) pa[m][s] = __builtin_bit_cast(mv_bf8, T[0][s][q][32 * wo + 16 * m + r]);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            mv_bf8 qb[3];
#pragma unroll
            for (int s = 0; s < 3; ++s) qb[s] = __builtin_bit_cast(mv_bf8, T[1][s][q][64 * wi + 16 * t + r]);
            // the six term products, smallest first
#pragma unroll
            for (int o = 2; o >= 0; --o)
#pragma unroll
                for (int s = 0; s <= o; ++s)
#pragma unroll
                    for (int m = 0; m < 2; ++m) acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa[m][s], qb[o - s], acc[m][t], 0, 0, 0);
        }
    };
    mv_wg_pipeline(nst, chp_, issue, store, compute);
    float* slab = L.slab + (size_t)b.ch * No * Ki;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t = 0; t < 4; ++t) mv_wg_slab_store(slab, acc[m][t], o0 + 32 * wo + 16 * m + 4 * q, i0 + 64 * wi + 16 * t + r, No, Ki);
    if (do_bias) {                                                // bias sums: plain fp32, the four row groups of a column added in a fixed order
        float* red = (float*)T;
        __syncthreads();
        red[sg * TILE + scol] = bsum;
        __syncthreads();
        if (tid < TILE && o0 + tid < No) L.bslab[(size_t)b.ch * No + o0 + tid] = (red[tid] + red[TILE + tid]) + (red[2 * TILE + tid] + red[3 * TILE + tid]);
    }
}
