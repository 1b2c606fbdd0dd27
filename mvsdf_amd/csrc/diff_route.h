// diff_route.h -- which kernel family and template instance each differentiable MLP pass (diff_mlp.hip) launches: the development switches in ONE struct and
// pure functions from plain integers to a route.  No HIP in here: tests/test_diff_route_host.py compiles this header alone with the host compiler and holds
// every route to a committed table.
#pragma once
#include <stddef.h>
#include <stdlib.h>

// The development A/B switches of diff_mlp.hip -- THE list (capi_util.h::mv_dev_env: read only by a library built with -DMVSDF_DEV_SWITCHES).  The defaults are
// the product's values.  Filled once per process by diff_mlp.hip::mv_dev_switches().
struct MvDevSwitches {
    int fuse = 1;            // MVSDF_FUSE=0: the per-layer kernels (k_layer) instead of the fused chain kernels
    int split_chains = 0;    // MVSDF_SPLIT_CHAINS (set): mvsdf_sdf_backward as the separate E.1 / E.2 chain launches
    int chain_w8 = 0;        // MVSDF_CHAIN_W8=1: 8-wave workgroups in the fp32 chains
    int chain_mt = 0;        // MVSDF_CHAIN_MT=1|2: row tiles per chain workgroup, overriding the cost models below
    int chain_x3 = 1;        // MVSDF_CHAIN_X3=0: the fp32-input MFMA chains although the three-term bf16 packs exist
    int delta_chain = 0;     // MVSDF_DELTA_CHAIN=1: the delta pass as a first-order chain instead of the scaling of the saved s_l
    int layer_mt = 0;        // MVSDF_LAYER_MT=1|2: row tiles per workgroup of the per-layer kernels
    int wg_xcd = 1;          // MVSDF_WG_XCD=0: k_wgrad_net's blocks in launch order instead of the XCD-aware order
    int wgrad_x3 = -1;       // MVSDF_WGRAD_X3=0|1: the weight gradients on the fp32-input MFMA (k_wgrad_net) / in the three-term bf16 arithmetic (wgrad_x3.h)
                             // whatever the descriptor carries; -1: by rule (mv_wgrad_uses_x3).  mvsdf_set_wgrad_x3 overrides it at run time.
};
// The struct from the environment (env: capi_util.h::mv_dev_env in the library, getenv in the route test).  The switches that pick the per-layer / split /
// 8-wave fp32 launches mean the fp32 arithmetic everywhere: applied here and nowhere else.
inline MvDevSwitches mv_switches_from_env(const char* (*env)(const char*)) {
    MvDevSwitches v;
    const char* e;
    if ((e = env("MVSDF_FUSE"))) v.fuse = atoi(e) != 0;
    if ((e = env("MVSDF_CHAIN_MT"))) v.chain_mt = atoi(e);
    if ((e = env("MVSDF_CHAIN_X3"))) v.chain_x3 = atoi(e) != 0;
    if ((e = env("MVSDF_DELTA_CHAIN"))) v.delta_chain = atoi(e) != 0;
    if ((e = env("MVSDF_LAYER_MT"))) v.layer_mt = atoi(e);
    if ((e = env("MVSDF_WG_XCD")) && *e && atoi(e) >= 0) v.wg_xcd = atoi(e) != 0;
    if ((e = env("MVSDF_WGRAD_X3")) && *e) v.wgrad_x3 = atoi(e) < 0 ? -1 : atoi(e) != 0;
    v.split_chains = env("MVSDF_SPLIT_CHAINS") != nullptr;          // (set at all, whatever its value -- historical, kept)
    const bool w8_set = (e = env("MVSDF_CHAIN_W8")) != nullptr;
    if (w8_set) v.chain_w8 = atoi(e) != 0;
    if (!v.fuse || v.split_chains || w8_set) v.chain_x3 = 0;        // (MVSDF_CHAIN_W8 set at all, even to 0 -- historical, kept)
    return v;
}

enum MvFamily {
    MV_FAM_REFUSE = 0,       // not here: the entry point returns MvRoute::rc and launches nothing
    MV_FAM_LAYERS,           // one k_layer launch per layer
    MV_FAM_SPLIT,            // k_chain_e1 + k_chain_e2
    MV_FAM_F32,              // one fused chain on the fp32-input MFMA (layer_kernels.h)
    MV_FAM_X3,               // one fused chain in the three-term bf16 arithmetic (chain_x3.h)
    MV_FAM_SCALE             // delta pass only: zbar_l += fbar . s_l (k_delta_apply)
};
// family + the template instance <MT, NTW, NW(, PD)> of its chain kernel: row tiles per workgroup, column tiles per wave, waves, carried-ring depth
struct MvRoute { int family, rc, mt, ntw, nw, pd; };
inline bool mv_route_takes_cnt(const MvRoute& r) { return r.family == MV_FAM_F32 || r.family == MV_FAM_X3 || r.family == MV_FAM_SCALE; }

// Carried-ring depth (k-blocks of the next phase's weights requested early, chain_x3.h) of the x3 chains.  One row tile per workgroup (<= 256 tiles: c2): 4 --
// k_chain_fwd_x3 111 -> 97 us, the c2 step 1.503 -> 1.485 ms.  Two row tiles: 0 (the rolling fetch): with 2 the c5-share step went 1.51-1.55 -> 1.57-1.61 ms and c3
// 4.04 -> 4.20 ms -- at those sizes the sample rows' chain runs BESIDE the tracer (mv_chain_split_pays), and a chain that keeps the L2 busy through its epilogues
// takes that bandwidth from the tracer's own weight stream (k_ray_samples 0.446 -> 0.478 ms, k_sphere_trace 1.17 -> 1.27 ms at c3).
#ifndef MV_X3_PD1
#define MV_X3_PD1 4
#endif
#ifndef MV_X3_PD2
#define MV_X3_PD2 0
#endif

// ---- row tiles per workgroup: cost of a launch over tiles16 16-row tiles in rounds of the 256 CUs, a round of two-tile workgroups costing `two` rounds ----
inline double mv_chain_cost(int tiles16, int mt, double two) { return mt == 2 ? two * ((tiles16 + 511) / 512) : 1.0 * ((tiles16 + 255) / 256); }
inline int mv_chain_mt_model(int tiles16, double two, const MvDevSwitches& sw) {
    if (sw.chain_mt == 1 || sw.chain_mt == 2) return sw.chain_mt;
    return mv_chain_cost(tiles16, 2, two) < mv_chain_cost(tiles16, 1, two) ? 2 : 1;
}
// The fp32 chains (the W <= 256, 16-wave instantiations).  A workgroup with two 16-row tiles takes ~1.76x one tile (measured at c3: the phases are bound by the
// per-row loads / stores of the saved activations, not by the shared weight fragments), so two tiles pay only when they save a round of the 256 CUs: 257..512
// tiles (c5's per-GPU share: 248 -> 215 us), not 513..768 (c3).  Four tiles never pay (3.8x).
inline int mv_chain_mt(int tiles16, const MvDevSwitches& sw) { return mv_chain_mt_model(tiles16, 1.76, sw); }
// The x3 chains: two tiles share the weight stream that bounds a phase (tile_engine_bf16s.h: 56 vs 41 us per evaluation), so they pay as soon as they save a round
inline int mv_chain_mt_x3(int tiles16, const MvDevSwitches& sw) { return mv_chain_mt_model(tiles16, 1.45, sw); }
// Is the fp32 forward chain over tiles_part tiles a shorter launch than over tiles_all?  (mv_chain_split_pays; each at the cheaper of its two forms -- the
// model alone: MVSDF_CHAIN_MT does not enter, historical)
inline bool mv_chain_shorter(int tiles_part, int tiles_all) {
    auto best = [](int t) { const double c1 = mv_chain_cost(t, 1, 1.76), c2 = mv_chain_cost(t, 2, 1.76); return c2 < c1 ? c2 : c1; };
    return best(tiles_part) < best(tiles_all);
}

// row tiles per workgroup of the per-layer kernels: 16 rows while that still leaves the chip under-subscribed (one workgroup per CU), else 32 (weights
// reused by two row tiles)
inline int mv_layer_mt(int rows, const MvDevSwitches& sw) { return (sw.layer_mt ? sw.layer_mt == 1 : rows <= 16 * 512) ? 1 : 2; }

// ---- the instances ----
// fp32 chains, one row tile: 16 waves per workgroup (one or two column tiles each) -- these launches are single waves of one-tile workgroups, i.e. chains of
// dependent layer phases; twice the waves halve every wave's share of the global loads / stores and of the epilogue between two GEMMs (measured 148 -> 127 us
// for the forward, 173 -> 143 us for the backward pass).  MVSDF_CHAIN_W8=1: 8 waves (dev A/B).  Two row tiles (two_tile: the family has that form) exist only
// for hidden width <= 256 at 16 waves.
inline MvRoute mv_route_f32(int net_ntw, int tiles16, bool two_tile, const MvDevSwitches& sw) {
    const bool w8 = sw.chain_w8 != 0;
    const int mt = (two_tile && net_ntw == 2 && !w8) ? mv_chain_mt(tiles16, sw) : 1;
    if (mt == 2) return {MV_FAM_F32, 0, 2, 1, 16, 0};
    return {MV_FAM_F32, 0, 1, w8 ? net_ntw : net_ntw / 2, w8 ? 8 : 16, 0};
}
// x3 chains.  Hidden width <= 256: 16 waves x 1 column tile; up to 512: 16 waves x 2.  Hidden width 257 .. 512 with two row tiles: 8 waves x 4 column tiles -- a
// 16-row tile streams 1.57 MB of weight terms per phase, more than its matrix instructions take; at 37 000 rows of the 8x512 network 4208 (fp32 chain) / 3842
// (one tile) / 2761 us (two tiles).
inline MvRoute mv_route_x3(int net_ntw, int tiles16, bool two_tile, const MvDevSwitches& sw) {
    const int mt = two_tile ? mv_chain_mt_x3(tiles16, sw) : 1;
    if (mt == 2) return net_ntw == 4 ? MvRoute{MV_FAM_X3, 0, 2, 4, 8, 0} : MvRoute{MV_FAM_X3, 0, 2, 1, 16, MV_X3_PD2};
    return net_ntw == 2 ? MvRoute{MV_FAM_X3, 0, 1, 1, 16, MV_X3_PD1} : MvRoute{MV_FAM_X3, 0, 1, 2, 16, 0};
}
// weight gradients (k_wgrad_net / k_reduce_net): the three-term form wherever the x3 chains run -- the SDF descriptor of the call carries the three-term packs
// (has_packs) and chain_x3 is on -- unless `mode` (the run-time setter, else MvDevSwitches::wgrad_x3) says 0 or 1
inline bool mv_wgrad_uses_x3(bool has_packs, int mode, const MvDevSwitches& sw) {
    if (mode < 0) mode = sw.wgrad_x3;
    return mode < 0 ? (has_packs && sw.chain_x3 != 0) : mode != 0;
}
inline MvRoute mv_route_refuse(int rc) { return {MV_FAM_REFUSE, rc, 0, 0, 0, 0}; }
inline MvRoute mv_route_layers() { return {MV_FAM_LAYERS, 0, 0, 0, 0, 0}; }

// ---- one function per pass.  net_ntw: capi_util.h::mv_chain_ntw of the network (0: too wide for the chains); tiles16: 16-row tiles of the launch; x3: the caller
// has (or will try for) the three-term packs of every layer -- it asks with x3 = true first and again with false when the packs are missing ----

// SDF forward (value + normal).  last_nt: 16-column tiles of the last layer; gather_or_sub: rows gathered in the kernel or a proper sub-range of the rows.
inline MvRoute mv_route_sdf_forward(int net_ntw, int tiles16, int last_nt, bool x3, bool gather_or_sub, const MvDevSwitches& sw) {
    if (sw.fuse && net_ntw && last_nt <= 8 * net_ntw * 4) return (x3 && sw.chain_x3) ? mv_route_x3(net_ntw, tiles16, true, sw) : mv_route_f32(net_ntw, tiles16, true, sw);
    return gather_or_sub ? mv_route_refuse(1) : mv_route_layers();     // per-layer route: the caller materialises the rows, all of them at once
}
// SDF backward, single pass (mvsdf_sdf_backward).  several_skips: the per-layer kernels and the split chains' PE kernel know one skip layer.
// One row tile per workgroup in both arithmetics -- historical: the pass predates the two-tile forms and the step's big launches go through the pair.
inline MvRoute mv_route_sdf_backward(int net_ntw, int tiles16, bool x3, bool several_skips, const MvDevSwitches& sw) {
    if (sw.fuse && !sw.split_chains && net_ntw) return (x3 && sw.chain_x3) ? mv_route_x3(net_ntw, tiles16, false, sw) : mv_route_f32(net_ntw, tiles16, false, sw);
    if (several_skips) return mv_route_refuse(-4);
    if (sw.fuse && net_ntw) return {MV_FAM_SPLIT, 0, 1, net_ntw, 8, 0};     // k_chain_e1 / k_chain_e2 have the 8-wave forms only (historical)
    return mv_route_layers();
}
// SDF backward, passes A + X in one grid (the training step).  Chains only; MVSDF_FUSE / MVSDF_SPLIT_CHAINS do not reach it except through the arithmetic
// (historical: the step's per-layer route is the caller's fall-back to mvsdf_sdf_backward after -3).
inline MvRoute mv_route_sdf_backward_pair(int net_ntw, int tiles16, bool x3, const MvDevSwitches& sw) {
    if (!net_ntw) return mv_route_refuse(-3);
    return (x3 && sw.chain_x3) ? mv_route_x3(net_ntw, tiles16, true, sw) : mv_route_f32(net_ntw, tiles16, true, sw);
}
// delta pass.  The chain form (fp32 always, two row tiles where they pay: deliberate, it was the step's critical path) has no device-count form: with cnt
// the answer under MVSDF_DELTA_CHAIN is "not here".  That is a predicate for mv_route_can_defer, not a code any caller sees -- a step that cannot defer never
// passes cnt, and mv_sdf_backward_delta_fbar, the one entry point that takes cnt, always scales.  (-3 without cnt is the callers' "network too wide".)
inline MvRoute mv_route_delta(int net_ntw, int tiles16, bool cnt, const MvDevSwitches& sw) {
    if (!net_ntw) return mv_route_refuse(-3);
    if (!sw.delta_chain) return {MV_FAM_SCALE, 0, 0, 0, 0, 0};
    return cnt ? mv_route_refuse(-3) : mv_route_f32(net_ntw, tiles16, true, sw);
}
// rendering net: no two-tile forms (deliberate: its launches are the hit rows only).  Forward: the last layer fits one wave's column tiles.
inline MvRoute mv_route_render_forward(int net_ntw, int last_nt, const MvDevSwitches& sw) {
    return (sw.fuse && net_ntw && last_nt <= 2) ? mv_route_f32(net_ntw, 0, false, sw) : mv_route_layers();
}
// backward: one column-tile group per wave above the first layer (upper_nt: the most 16-column tiles of a transposed layer l >= 1).
// rows_or_cnt: row indirection of the upstream or device-side counts, which only the chain takes.
inline MvRoute mv_route_render_backward(int net_ntw, int upper_nt, bool rows_or_cnt, const MvDevSwitches& sw) {
    if (sw.fuse && net_ntw && upper_nt <= 8 * net_ntw) return mv_route_f32(net_ntw, 0, false, sw);
    return rows_or_cnt ? mv_route_refuse(-3) : mv_route_layers();
}
// Can the step's backward run with device-side counts?  Every pass of it must land in a family that takes them (the per-layer fall-backs size their grids
// from host numbers: a step on such a network waits for the counts as before).
inline bool mv_route_can_defer(int sdf_ntw, int render_ntw, int render_upper_nt, const MvDevSwitches& sw) {
    return mv_route_takes_cnt(mv_route_sdf_backward_pair(sdf_ntw, 1, true, sw)) && mv_route_takes_cnt(mv_route_delta(sdf_ntw, 1, true, sw)) &&
           mv_route_takes_cnt(mv_route_render_backward(render_ntw, render_upper_nt, true, sw));
}

// ---- dynamic LDS bytes, one function per family.  S: LDS row stride (fp32 chains: floats; x3: bf16 elements of one term tile); d0: PE width ----
inline size_t mv_lds_fwd_f32(int mt, int S, int d0) { return ((size_t)16 * mt * S + 2 * ((16 * mt * d0 + 3) & ~3) + 16 * mt * 4) * sizeof(float); }
inline size_t mv_lds_fwd_x3(int mt, int S, int d0) { return (size_t)3 * 16 * mt * S * 2 + ((size_t)2 * ((16 * mt * d0 + 3) & ~3) + 16 * mt * 4) * sizeof(float); }
inline size_t mv_lds_bwd_f32(int mt, int S, int d0) { return (size_t)16 * mt * (S + d0) * sizeof(float); }
inline size_t mv_lds_bwd_x3(int mt, int S, int d0) { return (size_t)3 * 16 * mt * S * 2 + (size_t)16 * mt * d0 * sizeof(float); }
inline size_t mv_lds_render(int S) { return (size_t)16 * S * sizeof(float); }
