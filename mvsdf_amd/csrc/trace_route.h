// trace_route.h -- what the tracer (trace.hip) and mvsdf_sdf_col0 (basic.hip) launch: the switches in ONE struct, pure functions from plain integers to a
// template instance, a grid or a byte count, and the layout of the tracer's workspace.  No HIP in here: tests/test_trace_route_host.py compiles this header
// alone with the host compiler and holds every rule to a committed table.
#pragma once
#include <stddef.h>
#include <stdlib.h>

// The switches of the tracer -- THE list.  `tail` is a product switch (read by every library); the others are development switches (capi_util.h::mv_dev_env: read
// only by a library built with -DMVSDF_DEV_SWITCHES).  The defaults are the product's values.  Filled once per process by trace.hip::mv_trace_switches().
struct MvTraceSwitches {
    int tail = 1;            // MVSDF_TAIL=0: no tail filling; =2: also for the bf16-weight engines (measured slower there: mv_tail_on)
    int tail_stop = -1;      // MVSDF_TAIL_STOP=n: helpers take no new tile once at most n workgroups still trace (< 0: mv_tail_stop_left's rule)
    int nfirst = 12;         // MVSDF_NFIRST=n: size of the first sampler window (at least 2)
    int mt_first = 0;        // MVSDF_MT_FIRST=n: row tiles of the first sampler window's workgroups (<= 0: mv_route_samples' rule)
    int bf_carry = 0;        // MVSDF_BF_CARRY=1: mvsdf_sdf_col0 of the bf16-term engines with k_sphere_trace's weight fetch (tile_engine_bf16.h, CARRIED) instead
                             // of the row-sample kernels' (ROLLING); same arithmetic, bit-identical results (tests/test_gpu_bf16.py)
};
inline MvTraceSwitches mv_trace_switches_from_env(const char* (*product_env)(const char*), const char* (*dev_env)(const char*)) {
    MvTraceSwitches v;
    const char* e;
    if ((e = product_env("MVSDF_TAIL"))) v.tail = atoi(e);
    if ((e = dev_env("MVSDF_TAIL_STOP"))) v.tail_stop = atoi(e);
    if ((e = dev_env("MVSDF_NFIRST"))) v.nfirst = atoi(e);
    if (v.nfirst < 2) v.nfirst = 2;
    if ((e = dev_env("MVSDF_MT_FIRST"))) v.mt_first = atoi(e);
    if ((e = dev_env("MVSDF_BF_CARRY"))) v.bf_carry = atoi(e) != 0;
    return v;
}

// ---- the engine class: the net type a trace_dtype runs on ----
enum MvTraceEngine {
    MV_ENG_F32 = 0,          // MvNet: fp32 weights, fp32-input MFMA (trace_dtype 0, and 2 = its packs of the bf16-rounded weights)
    MV_ENG_BS2,              // MvNetBs<2>: bf16 weights, activations as two bf16 terms (3)
    MV_ENG_BS3,              // MvNetBs<3>: ... as three bf16 terms (4)
    MV_ENG_X3                // MvNetBs<3, 3>: fp32 weights as three bf16 terms too (5): the one engine with weight_terms == 3
};
inline int mv_engine_weight_terms(int engine) { return engine == MV_ENG_X3 ? 3 : 1; }
struct MvEngineClass { int rc, engine; const char* why; };          // rc != 0: refused, with the message of the entry point
#define MV_DTYPE1_GONE "trace_dtype 1 (bf16 weights AND 8-bit activations) was removed in round 5: use 3 (bf16x2: same speed, parity-checked)"
inline MvEngineClass mv_trace_engine(int trace_dtype, bool col0) {
    switch (trace_dtype) {
        case 1: return {-2, 0, col0 ? "mvsdf_sdf_col0: " MV_DTYPE1_GONE : "mvsdf_trace: " MV_DTYPE1_GONE};
        case 3: return {0, MV_ENG_BS2, nullptr};
        case 4: return {0, MV_ENG_BS3, nullptr};
        case 5: return {0, MV_ENG_X3, nullptr};
        default: return {0, MV_ENG_F32, nullptr};
    }
}

// ---- the instances ----
// <MT, NTW, NW> = row tiles per workgroup, column tiles per wave, waves; xr (mvsdf_sdf_col0 only): the weight fetch carried across layers.  rc != 0: refused.
// The functions below return nothing else than the instances the launchers instantiate (tests/test_trace_route_host.py lists them).
struct MvInst { int rc, mt, ntw, nw, xr; const char* why; };
inline MvInst mv_inst_refuse(int rc, const char* why) { return {rc, 0, 0, 0, 0, why}; }
constexpr int mv_inst_key(int mt, int ntw, int nw) { return (mt * 100 + ntw) * 100 + nw * 2; }        // for the launchers' switches (+ xr where it matters)
// The ladder: (engine, maxnt = 16-column tiles of the widest hidden layer, requested row tiles) -> instance.  Waves per workgroup: 8 (two per SIMD) once there are
// >= 2 column tiles per wave to share (width 256 up; forcing 4 there measured 0.78 -> 0.99 ms); the bf16-MFMA engines are built for 8-wave workgroups only.
// Above width 256 (maxnt > 16, always 8 waves) there are four column tiles per wave and at most two row tiles.
inline MvInst mv_inst_ladder(int engine, int maxnt, int mt) {
    if (maxnt > 16) return {0, mt >= 2 ? 2 : 1, 4, 8, 0, nullptr};
    const int m = mt >= 4 ? 4 : (mt >= 2 ? 2 : 1);
    return (engine != MV_ENG_F32 || maxnt >= 16) ? MvInst{0, m, 2, 8, 0, nullptr} : MvInst{0, m, 4, 4, 0, nullptr};
}
#ifndef MV_SPHERE_NW16
#define MV_SPHERE_NW16 1                                            // (-DMV_SPHERE_NW16=0: the 8-wave x 2-tile form, for A/B builds -- tools/pp_ab.sh)
#endif
// k_sphere_trace; mt: row tiles per workgroup (8 * mt rays).  Its .mt is the "effective mt" of the decisions below.
inline MvInst mv_route_sphere(int engine, int maxnt, int mt) {
    if (maxnt > 32) return mv_inst_refuse(1, "network too wide");   // (the launcher's hipErrorInvalidValue)
    const MvInst r = mv_inst_ladder(engine, maxnt, mt);
    // one 16-row tile per workgroup, three weight terms: SIXTEEN waves x one column tile.  The evaluations of this kernel wait for each other, a wave's share of a
    // layer is a latency chain (k-blocks of 3 x 2 dependent instructions, then the softplus epilogue): half the chain per wave.  tools/micro/x3_engine_rounds.hip:
    // 38.4 (8 waves x 2 tiles) -> 33.7 us per evaluation with the ping-pong tiles.  Same instruction sequence per output column: same bits.
    if (MV_SPHERE_NW16 != 0 && engine == MV_ENG_X3 && r.mt == 1 && r.ntw == 2) return {0, 1, 1, 16, 0, nullptr};
    return r;
}
// k_ray_samples of part 1 (sampler rows), 2 (secant + min-sdf rows), 4 (min-sdf rows alone) or 8 (secant alone); mt_samples: row tiles per chunk.
// Part 1: the two sampler launches are small (about one wave of workgroups at a few thousand rays): 16-row chunks spread them over more CUs (measured 285 ->
// 241 us at 2048 rays).  Three weight terms: a 16-row evaluation is bound by its 3.1 MB weight stream, two tiles share it (c2 1.687 -> 1.664 ms, c5 share
// 2.539 -> 2.483).
inline MvInst mv_route_samples(int engine, int maxnt, int mt_samples, int R, int part, const MvTraceSwitches& sw) {
    if (maxnt > 32) return mv_inst_refuse(1, "network too wide");
    int mt = mt_samples;
    if (part == 1) mt = sw.mt_first > 0 ? sw.mt_first : (engine == MV_ENG_X3 ? (mt_samples > 2 ? 2 : mt_samples) : (R <= 4096 ? 1 : mt_samples));
    return mv_inst_ladder(engine, maxnt, mt);
}
// The secant chains alone (stage 7 of mvsdf_trace_stage): n_secant dependent evaluations of 16 listed rays per workgroup -- the sphere tracer's shape of work, so
// where mv_route_sphere has the sixteen-wave form for one row tile (three weight terms) the chains take it as k_secant_chains<1, 1, 16>; every other engine and
// width keeps the part-8 instance of k_ray_samples.  (nw == 16 in the answer names the k_secant_chains instance; anything else is launch_stage2's part 8.)
#ifndef MV_SECANT_NW16
#define MV_SECANT_NW16 1                                            // (-DMV_SECANT_NW16=0: the part-8 instance everywhere, for A/B builds)
#endif
inline MvInst mv_route_secant(int engine, int maxnt, int mt_samples, int R, const MvTraceSwitches& sw) {
    const MvInst s = mv_route_sphere(engine, maxnt, 1);
    if (MV_SECANT_NW16 != 0 && s.rc == 0 && s.mt == 1 && s.ntw == 1 && s.nw == 16) return s;
    return mv_route_samples(engine, maxnt, mt_samples, R, 8, sw);
}
// mvsdf_sdf_col0; mt = 49: the sphere tracer's engine, the weight ring carried across layers (two column tiles per wave: width <= 256).
// Historical, kept: only the fp32 engine checks mt (the bf16-term engines take any mt down the ladder), only the bf16-term engines refuse maxnt > 32.
inline MvInst mv_route_col0(int engine, int maxnt, int mt, const MvTraceSwitches& sw) {
    if (engine != MV_ENG_F32) {
        if (maxnt > 32) return mv_inst_refuse(-1, "mvsdf_sdf_col0: network too wide");
        MvInst r = mv_inst_ladder(engine, maxnt, mt);
        r.xr = sw.bf_carry != 0;
        return r;
    }
    if (mt != 1 && mt != 2 && mt != 4 && mt != 49) return mv_inst_refuse(-1, "mvsdf_sdf_col0: mt must be 1, 2, 4 (row tiles per workgroup) or 49 (the sphere tracer's carried-ring engine)");
    if (mt != 49) return mv_inst_ladder(engine, maxnt, mt);
    if (maxnt > 16) return mv_inst_refuse(-1, "mvsdf_sdf_col0: mt = 49 needs a hidden width <= 256");
    return {0, 1, 2, 8, 1, nullptr};
}

// ---- the decisions.  mt1: mv_route_sphere(...).mt; cus: compute units of the device (256 on an unpartitioned MI355X) ----
inline int mv_sphere_grid(int R, int mt1) { return (R + 8 * mt1 - 1) / (8 * mt1); }
// Tail filling: sphere-tracing workgroups whose rays are done evaluate min-sdf rows (trace.hip, "tail filling of k_sphere_trace").  Only for grids of at most one
// workgroup per compute unit: with more, a finished workgroup's slot is wanted by a tracing workgroup that has not started yet -- helping would delay it.  The bound
// is also what makes the helpers' one wait safe (a helper that over-claimed a tile sleeps until the rows it owns are published): every workgroup of the grid can be
// resident at once, so the tracing workgroups a waiting helper depends on never wait for its slot.  (A partitioned device reports fewer compute units and gets no
// tail filling at c2.)  On by default for the fp32 engine and -- above 2048 rays -- for the three-weight-term engine (three alternating runs each: c3 4.012 -> 3.961
// ms, c5 share 2.270 -> 2.238; c2 1.470 vs 1.473: no difference, left off).  The bf16-weight engines lose (a tile takes half the time, the launch that follows is
// bound by its secant chains and the helpers cost the sphere kernel more than they save: c2 +10 us, c5 share bf16x2 1.506 -> 1.545): MVSDF_TAIL=2 only.
inline bool mv_tail_on(int engine, int training, bool steps_given, int R, int mt1, int cus, const MvTraceSwitches& sw) {
    const int need = engine == MV_ENG_F32 ? 1 : ((engine == MV_ENG_X3 && R > 2048) ? 1 : 2);
    return training && steps_given && sw.tail >= need && mv_sphere_grid(R, mt1) <= cus;
}
// helpers take no new tile once at most this many workgroups still trace (swept at c2: 0 / 16 / 32 / 48 / 64 of 256 -> tracer 1575 / 1527 / 1521 / 1507 / 1507 us, off: 1549)
inline int mv_tail_stop_left(int R, int mt1, const MvTraceSwitches& sw) { return sw.tail_stop >= 0 ? sw.tail_stop : mv_sphere_grid(R, mt1) / 4; }
inline int mv_first_window(int n_steps, const MvTraceSwitches& sw) { return sw.nfirst < n_steps ? sw.nfirst : n_steps; }   // nf: the first sampler window (n_steps: single pass)
// Worst-case grids of launch_stage2 (every ray listed; blocks beyond the device-side counts exit at once) for chunks of mt row tiles: the sampler's first window, the
// rest, the min-sdf rows (a queue under tail filling: one more workgroup), the secant chains (16 rays each), k_reduce_items (a wave per listed ray, red_waves each).
struct MvSampleGrids { int first, rest, minsdf, sec, red; };
inline int mv_row_blocks(int R, int per_item, int mt) { return (int)(((long long)R * per_item + 16 * mt - 1) / (16 * mt)); }
inline MvSampleGrids mv_sample_grids(int R, int n_steps, int nf, int mt, int training, bool tail, int red_waves) {
    return {mv_row_blocks(R, nf, mt), nf < n_steps ? mv_row_blocks(R, n_steps - nf, mt) : 0, training ? mv_row_blocks(R, n_steps, mt) + (tail ? 1 : 0) : 0,
            (R + 15) / 16, (R + red_waves - 1) / red_waves};
}
// Dynamic LDS bytes of a kernel over mt row tiles: act_rows (trace.hip::mv_act_rows of the net type) activation rows of S floats, the PE tile, points, values.
inline size_t mv_tile_lds_floats(int S, int multires, int mt, int act_rows) { return (size_t)act_rows * S + ((16 * mt * (3 + 6 * multires) + 3) & ~3) + 16 * mt * 4 + 16 * mt; }
inline size_t mv_trace_lds_bytes(int S, int multires, int mt, int act_rows) { return mv_tile_lds_floats(S, multires, mt, act_rows) * 4 + 32; }   // (+ the counters)
inline size_t mv_col0_lds_bytes(int S, int multires, int mt) { return mv_tile_lds_floats(S, multires, mt, 16 * mt) * 4; }

// ---- the workspace of mvsdf_trace / mvsdf_tracegen_*: every region, in order (byte offsets; each region is 4-byte words per ray) ----
struct MvTraceWs {
    size_t w_zmin, w_zmax;             // [R] each: sample range of a listed ray
    size_t sec_state;                  // [4][R] z_low, z_high, sdf_low, sdf_high of secant rays
    size_t w_list, w_list_min;         // [R] each: the sampler / min-sdf work lists
    size_t sec_list;                   // [R] rays that need the secant
    size_t sv;                         // [R][n_steps] sample values of the sampler rows
    size_t list_rest, src_rest;        // [R] each: sampler rays the first window left open: list entry, sv row
    size_t sv_min;                     // [R][n_steps] the min-sdf rows' own sample values (they may run beside the sampler, and tail filling writes them early)
    size_t total;                      // + 256 bytes of slack
};
inline MvTraceWs mv_trace_ws(int R, int n_steps) {
    const size_t r = 4 * (size_t)(R > 0 ? R : 0), n = n_steps > 0 ? n_steps : 0;
    return {0, r, 2 * r, 6 * r, 7 * r, 8 * r, 9 * r, (9 + n) * r, (10 + n) * r, (11 + n) * r, (11 + 2 * n) * r + 256};
}
// ---- the sphere cut ----
// k_sphere_trace's rounds wait for each other, and the whole rest of the tracer waits for its slowest workgroup: at c2 most workgroups are done after st_iters + 1
// evaluations (no unspeculated back-off), a few need three more.  The cut stops the launch after that many; the rays that still want an evaluation go to a spill list
// and finish in a resume launch of the same kernel on a second stream, regrouped eight * mt per workgroup, beside the sampler windows of the rays that are final.
// On where it was measured to pay (profiles/sphere_cut_ab.txt): the three-weight-term engine, ONE row tile per sphere workgroup, at most one workgroup per compute unit and
// more than one per two -- 4 * cus < R <= 8 * cus, 1025 .. 2048 rays on an unpartitioned MI355X (c2: 1.329 -> 1.301 ms).  Below that the sampler windows it hides the late
// branch under shrink towards one evaluation each, while the branch keeps its fixed cost (two event hand-offs, a dependent row evaluation, a reduction: ~100 us), and a
// step of a few hundred rays is bound by its launches, of which the cut adds three.  With more row tiles per workgroup a round costs more and 32 rays seldom finish together
// (c3, 4 tiles x 256 workgroups: 3.075 -> 3.092 ms with the cut); with more workgroups than compute units the grid runs in waves, a finished workgroup's CU goes to the next
// one and there is no idle tail to move; the bf16-weight engines' rounds take half the time and their tail with them (c5share bf16x2 forced on: 1.388 -> 1.416 ms).
inline bool mv_sphere_cut_on(int engine, int R, int mt1, int cus) {
    const int grid = mv_sphere_grid(R, mt1);
    return engine == MV_ENG_X3 && mt1 == 1 && grid <= cus && 2 * grid > cus;
}
// its regions, BEHIND mv_trace_ws(R, n_steps) (mvsdf_trace_cut_workspace_bytes covers both; mvsdf_trace_workspace_bytes_n stays what mvsdf_trace needs): the spill list (16 words per ray), the late sampler list and its sample values
struct MvTraceCutWs {
    size_t spill;                      // [R][16] state of the rays the cut launch left unfinished (trace.hip: CutCtx)
    size_t list_late;                  // [R] sampler rays of the resume launch (the first list is being read beside it)
    size_t sv_late;                    // [R][n_steps] their sample values
    size_t total;
};
inline MvTraceCutWs mv_trace_cut_ws(int R, int n_steps) {
    const size_t r = 4 * (size_t)(R > 0 ? R : 0), n = n_steps > 0 ? n_steps : 0, b = (mv_trace_ws(R, n_steps).total + 255) & ~(size_t)255;
    return {b, b + 16 * r, b + 17 * r, b + (17 + n) * r + 256};
}
// ---- the sixteen-wave rows form (trace.hip: k_row_chunks<2, 1, 16>) ----
// Sample rows of a launch with at most about one 32-row chunk per compute unit are ONE dependent evaluation that nothing shares the CU with: a latency launch, like a
// round of k_sphere_trace.  Such a launch takes that kernel's shape -- sixteen waves x one column tile, ping-pong tiles, the weight ring carried across layers -- over the
// two row tiles of mv_route_samples' <2, 2, 8> instance.  Only the step's sphere-cut sequence has such launches (the late list's rows, the first sampler window), and the
// form exists for the three-weight-term engine up to hidden width 256: the rule is the cut's rule and the width.  The step consults it; mv_route_samples keeps its answers.
inline bool mv_rows16_on(int engine, int maxnt, int R, int mt1, int cus) { return mv_sphere_cut_on(engine, R, mt1, cus) && maxnt <= 16; }
// which of its two uses the rule turns on (bit 0: the first sampler window, bit 1: the late list's rows): each by its own A/B at c2 (profiles/fork_ab.txt, medians of
// three against the fork switched off, 1.2940 ms).  The late rows: 1.2820, every run faster -- on.  The first window: 1.2968, every run SLOWER -- off (the windows' own event slot
// falls, 0.4415 -> 0.4228 ms, and the step still loses: the window shares the chip with the resume launch, whose rounds are the critical path; not looked into further).
inline int mv_rows16_uses() { return 2; }
// its grid: worst-case chunks of 32 rows, at most one workgroup per compute unit (cap > 0: at most cap); workgroup b takes the chunks b, b + grid, ... -- a static stride
inline int mv_rows16_grid(int R, int per_item, int cus, int cap) {
    const int chunks = mv_row_blocks(R, per_item, 2), lim = cap > 0 ? cap : (cus > 0 ? cus : 1);
    return chunks < lim ? chunks : lim;
}
// its dynamic LDS: the sphere kernel's formula for two row tiles with the second pair of activation tiles (trace.hip: mv_act_rows<NET>(32, true) = 64 rows)
inline size_t mv_rows16_lds_bytes(int S, int multires) { return mv_trace_lds_bytes(S, multires, 2, 64); }
template <class T> inline T* mv_ws_at(void* ws, size_t offset) { return (T*)((char*)ws + offset); }
