// step_driver.hip -- the native step driver: IDRNetwork.forward (training mode, idr.py:179-322) and the backward through it as ONE C call
// each.  Every launch of a phase is enqueued from here, in the order functional._IdrStep / IDRNetwork.forward used to issue them from Python
// through ~45 ctypes calls (1.6 ms of host time per step); the kernels are the library's own entry points (mvsdf_hip.h), reached
// directly instead of through the interpreter.  No allocation, no synchronisation: the caller hands in one `fwd` block per forward (outputs +
// everything the backward reads) and a `bwd` scratch block; the one host wait of a step is mvsdf_step_wait_counts.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include "capi_util.h"
#include "step_internal.h"
#include <sched.h>
#include <time.h>

namespace {

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

struct FwdOffsets {
    size_t w[MVSDF_STEP_MAX_LAYERS], wp[MVSDF_STEP_MAX_LAYERS], wpT[MVSDF_STEP_MAX_LAYERS], wp16[MVSDF_STEP_MAX_LAYERS];
    size_t wx3[MVSDF_STEP_MAX_LAYERS], wx3T[MVSDF_STEP_MAX_LAYERS];   // SDF layers: three-term bf16 packs of W_l / W_l^T for the differentiable chains (chain_x3.h); wx3 == wp16 under trace_dtype 5
    int chain_x3;
    size_t trace_ws, trace_ws_bytes;
    size_t inv, true_rows, true_rank, counts, view_sorted;
    size_t bias[MVSDF_STEP_MAX_LAYERS], steps;                     // SDF layers: this forward's copy of the biases; its min-sdf steps (what mvsdf_step_resolve_unhit reads later)
    size_t x_eval, y_eval, n_eval, sdf_ctx, rgb_sorted, render_ctx;
};
struct BwdOffsets {
    size_t dy, dn, dy_x, dn_x, din, drgb_sorted, render_ws, wsA, wsX, dx, fbar;
};

struct Step {
    MvsdfStepDesc d;
    MvsdfStepLayout lay;
    FwdOffsets fo;
    BwdOffsets bo;
    int R, E, M, Nout, K0r, nl;                      // rays, sample rows, evaluation rows, SDF output width, rendering-net input width, layers in total
    size_t woff[MVSDF_STEP_MAX_LAYERS], boff[MVSDF_STEP_MAX_LAYERS];   // float offsets inside dflat: [W | b of the SDF net | W | b of the rendering net]
    size_t seg[2][3];                                // per network: first weight, first bias, end
    long long* counts_host;                          // pinned, host-mapped ring [MVSDF_STEP_COUNT_RING][8]: per slot the 4 counts + (entry 4) the sequence number of the
                                                     // forward that wrote them; forward `seq` owns slot seq % RING (a host that runs steps ahead can still ask for older ones)
    long long* counts_host_dev;                      // its device address (nullptr: not mapped, the counts travel by a copy + ev_counts into slot 0)
    int can_defer;                                   // every launch of the backward has a device-count form for these networks (mv_step_can_defer)
    hipEvent_t ev_counts;
    bool counts_pending;
    long long counts_seq;                            // forwards so far: the number the host waits for in counts_host[4]
    hipStream_t counts_stream;                       // the stream of the forward in flight (queried if the number does not arrive)
    int timing;
    hipEvent_t ev_t[9];                              // 0-4: around the tracer's launches; 5: end of the forward; 6 / 7: around the backward; 8: entry of the forward
    bool timed, timed_bwd;
    hipStream_t side;                                // the sample rows of the fused evaluation run here, beside the tracer (created on first use)
    hipEvent_t ev_fork, ev_join;
    int split_rows;                                  // -1 undecided, 0 one launch over all rows, 1 samples beside the tracer + rays after it
    int can_lazy;                                    // the rows of the rays without a hit can be left to mvsdf_step_resolve_unhit (the fused forward chain covers the SDF network)
    int last_grid[2];                                // {secant workgroups, sample-row workgroups} of the last forward's last tracer launch
    // the sphere cut of the deferring forward (mvsdf_step_set_sphere_cut): the late rays finish on `late` beside the sampler windows
    int cut_enable, cut_rounds, cut_on;              // cut_enable < 0: by the route's rule; cut_on: -1 undecided, 0 / 1 (streams and events exist)
    hipStream_t late;                                // normal priority: its few workgroups are latency chains like the main stream's
    hipEvent_t ev_cut, ev_late;
    // the fork of a forward with the cut, part by part (mvsdf_step_set_fork; < 0: by rule): the late branch on the launch stream and the windows on `late`, the ray
    // partition on `late` beside the secant chains, the sixteen-wave rows form (0 / 1 both uses / 2 late rows / 3 first window)
    int fork_late_main, fork_part_side, fork_rows16, fork_rows16_cap;
    hipEvent_t ev_main, ev_part;                     // launch stream -> `late` in front of the partition; the partition's record
};

// descriptors of the two networks over the packs inside a forward block
void make_descs(const Step& st, const MvsdfStepParams* prm, const char* fwd, MvsdfNetDesc* sdf, MvsdfNetDesc* sdfT, MvsdfNetDesc* rnd, MvsdfNetDesc* rndT) {
    const MvsdfStepDesc& d = st.d;
    auto fill = [&](MvsdfNetDesc* o, MvsdfNetDesc* oT, int l0, int n, bool is_sdf) {
        memset(o, 0, sizeof(*o));
        memset(oT, 0, sizeof(*oT));
        o->n_layers = oT->n_layers = n;
        for (int i = 0; i < n; ++i) {
            const int l = l0 + i;
            o->K[i] = d.K[l]; o->N[i] = d.N[l];
            oT->K[i] = d.N[l]; oT->N[i] = d.K[l];
            o->wp[i] = (const float*)(fwd + st.fo.wp[l]);
            oT->wp[i] = (const float*)(fwd + st.fo.wpT[l]);
            o->bias[i] = oT->bias[i] = prm->b[l];
            o->w[i] = oT->w[i] = (const float*)(fwd + st.fo.w[l]);
            if (is_sdf && d.trace_dtype != 0) o->wp16[i] = fwd + st.fo.wp16[l];
            if (is_sdf && st.fo.chain_x3) { o->wx3[i] = fwd + st.fo.wx3[l]; oT->wx3[i] = fwd + st.fo.wx3T[l]; }
        }
        if (is_sdf) {
            const unsigned m = d.skip_mask;
            const int single = (m && !(m & (m - 1))) ? __builtin_ctz(m) : -1;
            o->skip_layer = oT->skip_layer = m ? (single >= 0 ? single : __builtin_ctz(m)) : -1;
            o->skip_mask = (m && single < 0) ? m : 0;
            o->multires = oT->multires = d.multires;
            o->trace_dtype = (d.trace_dtype >= 1 && d.trace_dtype <= 5) ? d.trace_dtype : 0;
        } else {
            o->skip_layer = oT->skip_layer = -1;
        }
    };
    fill(sdf, sdfT, 0, d.n_sdf, true);
    fill(rnd, rndT, d.n_sdf, d.n_render, false);
}

// x_eval = [eikonal points | on-surface samples | jittered samples | traced points of the rays, hit rays first] (idr.py:253-257 evaluates these
// sets in five separate network calls); also fills the all-ones object mask handed back in the output dict (idr.py:187)
__global__ void k_step_gather_x(const float* __restrict__ eik, int n_eik, const float* __restrict__ ds_on, const float* __restrict__ ds_jit, int n_ds,
                                const float* __restrict__ points, const long long* __restrict__ perm, int R, float* __restrict__ x_eval,
                                uint8_t* __restrict__ ones) {
    const int E = n_eik + 2 * n_ds, total = (E + R) * 3;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int row = i / 3, c = i - 3 * row;
        float v;
        if (row < n_eik) v = eik[i];
        else if (row < n_eik + n_ds) v = ds_on[3 * (size_t)(row - n_eik) + c];
        else if (row < E) v = ds_jit[3 * (size_t)(row - n_eik - n_ds) + c];
        else v = points[3 * (size_t)perm[row - E] + c];
        x_eval[i] = v;
        if (ones && i < R) ones[i] = 1;
    }
}

// drgb_sorted[i] = d_rgb[perm[i]] for the N hit rows (the rendering net ran on the sorted rows; idr.py:302-304 scatters its output)
__global__ void k_step_gather_drgb(const float* __restrict__ d_rgb, const long long* __restrict__ perm, int N, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3 * N) return;
    const int row = i / 3, c = i - 3 * row;
    out[i] = d_rgb[3 * (size_t)perm[row] + c];
}

#define ST_TRY(expr) do { int rc_ = (expr); if (rc_) return rc_; } while (0)
#define ST_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return mv_check(e_, #expr); } while (0)

}  // namespace

extern "C" {

int mvsdf_step_create(const MvsdfStepDesc* desc, MvsdfStepLayout* layout, void** out) {
    if (!desc || !layout || !out) return mv_fail(-1, "mvsdf_step_create: null argument");
    if (desc->trace_dtype == 1) return mv_fail(-2, "mvsdf_step_create: trace_dtype 1 (bf16 weights AND 8-bit activations) was removed in round 5: use 3 (bf16x2)");
    const MvsdfStepDesc& d = *desc;
    const int nl = d.n_sdf + d.n_render;
    if (d.B <= 0 || d.P <= 0 || d.n_eik < 0 || d.n_ds < 0 || d.n_sdf < 2 || d.n_render < 1 || d.n_sdf > MVSDF_MAX_LAYERS || d.n_render > MVSDF_MAX_LAYERS ||
        nl > MVSDF_STEP_MAX_LAYERS || (long long)d.B * d.P > (1ll << 24))
        return mv_fail(-1, "mvsdf_step_create: bad sizes");
    Step* st = new (std::nothrow) Step;
    if (!st) return mv_fail(-1, "mvsdf_step_create: out of host memory");
    memset(st, 0, sizeof(*st));
    st->d = d;
    st->R = d.B * d.P; st->E = d.n_eik + 2 * d.n_ds; st->M = st->R + st->E; st->nl = nl;
    st->Nout = d.N[d.n_sdf - 1]; st->K0r = d.K[d.n_sdf];
    st->split_rows = -1;
    st->cut_enable = -1; st->cut_on = -1;
    st->fork_late_main = st->fork_part_side = st->fork_rows16 = -1;
    const int R = st->R, M = st->M;
    // probe descriptors (sizes only; the size functions do not dereference the pack pointers but the validity checks want non-null ones)
    MvsdfNetDesc sdf, sdfT, rnd, rndT;
    MvsdfStepParams fake;
    memset(&fake, 0, sizeof(fake));
    static const float dummy = 0.f;
    for (int l = 0; l < nl; ++l) fake.b[l] = &dummy;
    MvsdfStepLayout& L = st->lay;
    FwdOffsets& fo = st->fo;
    size_t p = 0;
    auto take = [&](size_t bytes) { const size_t o = p; p += al256(bytes ? bytes : 4); return o; };
    L.ray_dirs = take((size_t)R * 12); L.cam_loc = take((size_t)d.B * 12);
    L.points = take((size_t)R * 12); L.mask = take((size_t)R); L.dists = take((size_t)R * 4); L.counters = take(16 * 8);
    L.object_mask_out = take((size_t)R);
    fo.trace_ws_bytes = mvsdf_trace_cut_workspace_bytes(R, d.tp.n_steps);         // (the tracer's regions + the sphere cut's)
    fo.trace_ws = take(fo.trace_ws_bytes);
    fo.chain_x3 = mv_dev_switches().chain_x3;
    for (int l = 0; l < nl; ++l) {
        fo.w[l] = take((size_t)d.N[l] * d.K[l] * 4);
        fo.wp[l] = take(mvsdf_packed_floats(d.N[l], d.K[l]) * 4);
        fo.wpT[l] = take(mvsdf_packed_floats(d.K[l], d.N[l]) * 4);
        if (l < d.n_sdf && d.trace_dtype == 2) {
            fo.wp16[l] = take(mvsdf_packed_floats(d.N[l], d.K[l]) * 4);
        } else if (l < d.n_sdf && (d.trace_dtype == 3 || d.trace_dtype == 4)) {
            fo.wp16[l] = take(mvsdf_packed_bf16_bytes(d.N[l], d.K[l]));      // no duplicated columns: the activations are split into bf16 terms in LDS
        } else if (l < d.n_sdf && d.trace_dtype == 5) {
            fo.wp16[l] = take(3 * mvsdf_packed_bf16_bytes(d.N[l], d.K[l]));  // ... and so are the fp32 weights (three terms)
        }
        if (l < d.n_sdf && fo.chain_x3) {                                     // the differentiable chains' three-term packs (the tracer's own under trace_dtype 5)
            fo.wx3[l] = d.trace_dtype == 5 ? fo.wp16[l] : take(3 * mvsdf_packed_bf16_bytes(d.N[l], d.K[l]));
            fo.wx3T[l] = take(3 * mvsdf_packed_bf16_bytes(d.K[l], d.N[l]));
        }
    }
    L.perm = take((size_t)R * 8); fo.inv = take((size_t)R * 8); fo.true_rows = take((size_t)R * 8); fo.true_rank = take((size_t)R * 4); fo.counts = take(4 * 8 + 4 * 4);   // int64 counts[4], then float term_rows[3] (mvsdf_step_counts_offset + 32)
    fo.view_sorted = take((size_t)R * 12);
    for (int l = 0; l < d.n_sdf; ++l) fo.bias[l] = take((size_t)d.N[l] * 4);
    fo.steps = take((size_t)(d.tp.n_steps > 0 ? d.tp.n_steps : 0) * 4);
    fo.x_eval = take((size_t)M * 12); fo.y_eval = take((size_t)M * st->Nout * 4); fo.n_eval = take((size_t)M * 12);
    // the size functions need structurally valid descriptors: point every pack at the dummy
    make_descs(*st, &fake, (const char*)nullptr, &sdf, &sdfT, &rnd, &rndT);
    for (int i = 0; i < d.n_sdf; ++i) { sdf.wp[i] = sdfT.wp[i] = &dummy; sdf.w[i] = &dummy; }
    for (int i = 0; i < d.n_render; ++i) { rnd.wp[i] = rndT.wp[i] = &dummy; }
    const size_t ctx_f = mvsdf_sdf_ctx_floats(&sdf, M, M), rctx_f = mvsdf_render_ctx_floats(&rnd, R);
    if (!ctx_f || !rctx_f) { delete st; return mv_fail(-2, "mvsdf_step_create: network descriptor rejected (layer dims / skip mask)"); }
    st->can_lazy = mv_chain_fwd_covers(&sdf);
    st->can_defer = (d.n_ds == 0 && mv_step_can_defer(&sdf, &sdfT, &rnd, &rndT)) ? 1 : 0;   // (phase 0 checks its depth-surface sample counts on the host: idr.py:244)
    fo.sdf_ctx = take(ctx_f * 4);
    fo.rgb_sorted = take((size_t)R * 12);
    fo.render_ctx = take(rctx_f * 4);
    L.rgb_values = take((size_t)R * 12); L.sdf_output = take((size_t)R * 4); L.diff_pts = take((size_t)R * 12);
    L.eik_out = take((size_t)M * 4); L.points_hom = take((size_t)M * 16); L.grad_theta = take((size_t)M * 12);
    L.surf = take((size_t)(R + d.n_eik) * 4);
    L.fwd_bytes = p;
    // backward scratch
    BwdOffsets& bo = st->bo;
    p = 0;
    bo.dy = take((size_t)M * st->Nout * 4); bo.dn = take((size_t)M * 12);
    bo.dy_x = take((size_t)R * st->Nout * 4); bo.dn_x = take((size_t)R * 12);
    bo.din = take((size_t)R * st->K0r * 4); bo.drgb_sorted = take((size_t)R * 12);
    bo.render_ws = take(mvsdf_render_bwd_ws_floats(&rnd, R) * 4);
    bo.wsA = take(mvsdf_sdf_bwd_ws_floats(&sdf, M) * 4);
    bo.wsX = take(mvsdf_sdf_bwd_ws_floats(&sdf, R) * 4);
    bo.dx = take((size_t)R * 12); bo.fbar = take((size_t)R * 4);
    size_t off = 0;
    int lo = 0;
    const int cuts[2] = {d.n_sdf, nl};
    for (int net = 0; net < 2; ++net) {
        st->seg[net][0] = off;
        for (int l = lo; l < cuts[net]; ++l) { st->woff[l] = off; off += (size_t)d.N[l] * d.K[l]; }
        st->seg[net][1] = off;
        for (int l = lo; l < cuts[net]; ++l) { st->boff[l] = off; off += (size_t)d.N[l]; }
        st->seg[net][2] = off;
        lo = cuts[net];
    }
    L.dflat_floats = off;
    L.dflat = take(off * 4);
    L.bwd_bytes = p;
    // the pinned count buffer and the event are made by the first forward (creating a step needs no GPU: layouts can be inspected anywhere)
    *layout = L;
    *out = st;
    return 0;
}

void mvsdf_step_destroy(void* step) {
    Step* st = (Step*)step;
    if (!st) return;
    if (st->timing) for (int i = 0; i < 9; ++i) hipEventDestroy(st->ev_t[i]);
    if (st->counts_host) { hipEventDestroy(st->ev_counts); hipHostFree(st->counts_host); }
    if (st->side) { hipStreamSynchronize(st->side); hipEventDestroy(st->ev_fork); hipEventDestroy(st->ev_join); hipStreamDestroy(st->side); }
    if (st->late) { hipStreamSynchronize(st->late); hipEventDestroy(st->ev_cut); hipEventDestroy(st->ev_late); hipEventDestroy(st->ev_main); hipEventDestroy(st->ev_part); hipStreamDestroy(st->late); }
    delete st;
}

int mvsdf_step_set_timing(void* step, int enable) {
    Step* st = (Step*)step;
    if (!st) return mv_fail(-1, "mvsdf_step_set_timing: null step");
    if (enable && !st->timing) {
        for (int i = 0; i < 9; ++i) ST_HIP(hipEventCreate(&st->ev_t[i]));
        st->timing = 1;
    } else if (!enable && st->timing) {
        for (int i = 0; i < 9; ++i) hipEventDestroy(st->ev_t[i]);
        st->timing = 0;
    }
    st->timed = false; st->timed_bwd = false;
    return 0;
}

int mvsdf_step_set_sphere_cut(void* step, int enable, int max_rounds) {
    Step* st = (Step*)step;
    if (!st) return mv_fail(-1, "mvsdf_step_set_sphere_cut: null step");
    st->cut_enable = enable < 0 ? -1 : (enable ? 1 : 0);
    st->cut_rounds = max_rounds > 0 ? max_rounds : 0;
    st->cut_on = -1;                                              // decided again by the next forward (a stream that exists stays)
    return 0;
}

int mvsdf_step_set_fork(void* step, int late_on_main, int partition_beside_secant, int rows16, int rows16_grid_cap) {
    Step* st = (Step*)step;
    if (!st) return mv_fail(-1, "mvsdf_step_set_fork: null step");
    if (rows16 > 3) return mv_fail(-1, "mvsdf_step_set_fork: rows16 must be < 0 (rule), 0, 1 (both uses), 2 (late rows) or 3 (first window)");
    st->fork_late_main = late_on_main < 0 ? -1 : (late_on_main ? 1 : 0);
    st->fork_part_side = partition_beside_secant < 0 ? -1 : (partition_beside_secant ? 1 : 0);
    st->fork_rows16 = rows16 < 0 ? -1 : rows16;
    st->fork_rows16_cap = rows16_grid_cap > 0 ? rows16_grid_cap : 0;
    return 0;
}

int mvsdf_step_trace_times(void* step, float ms[3]) {
    Step* st = (Step*)step;
    if (!st || !ms || !st->timing || !st->timed) return mv_fail(-1, "mvsdf_step_trace_times: timing is off or no forward has run");
    float a = 0.f, b = 0.f, c = 0.f;
    ST_HIP(hipEventElapsedTime(&a, st->ev_t[0], st->ev_t[1]));
    ST_HIP(hipEventElapsedTime(&b, st->ev_t[1], st->ev_t[2]));
    ST_HIP(hipEventElapsedTime(&c, st->ev_t[3], st->ev_t[4]));
    ms[0] = a; ms[1] = b; ms[2] = c;
    return 0;
}

int mvsdf_step_times(void* step, float ms[6]) {
    Step* st = (Step*)step;
    if (!st || !ms || !st->timing || !st->timed) return mv_fail(-1, "mvsdf_step_times: timing is off or no forward has run");
    if (int rc = mvsdf_step_trace_times(step, ms)) return rc;
    ST_HIP(hipEventElapsedTime(&ms[3], st->ev_t[4], st->ev_t[5]));
    ms[4] = 0.f;
    if (st->timed_bwd) ST_HIP(hipEventElapsedTime(&ms[4], st->ev_t[6], st->ev_t[7]));
    ST_HIP(hipEventElapsedTime(&ms[5], st->ev_t[8], st->ev_t[5]));
    return 0;
}

int mvsdf_step_forward(void* step, const MvsdfStepParams* prm, const MvsdfStepInputs* in, int d_mask, int e_mask, int mode, void* fwd_, void* stream) {
    Step* st = (Step*)step;
    if (!st || !prm || !in || !fwd_) return mv_fail(-1, "mvsdf_step_forward: null argument");
    if (mode != MVSDF_STEP_UNHIT_DEFER && mode != MVSDF_STEP_UNHIT_EAGER) return mv_fail(-1, "mvsdf_step_forward: mode must be MVSDF_STEP_UNHIT_DEFER or MVSDF_STEP_UNHIT_EAGER");
    // lazy: minimal_sdf_points of the rays without a hit (ray_tracing.py:280-308), their evaluation rows [E + N, E + R) and their sdf_output are left to
    // mvsdf_step_resolve_unhit: nothing in a training step reads them (loss.py:176-219 takes neither `points` nor `sdf_output`; the backward covers [0, E + N))
    const bool lazy = mode == MVSDF_STEP_UNHIT_DEFER;
    if (lazy && !st->can_lazy) return mv_fail(-3, "mvsdf_step_forward: MVSDF_STEP_UNHIT_DEFER is not available for this step (mvsdf_step_can_defer_unhit)");
    const MvsdfStepDesc& d = st->d;
    if (!in->uv || !in->pose || !in->intrinsics || !in->object_mask || !in->object_mask_true || !in->intervals || !in->minsdf_steps ||
        (d.n_eik > 0 && !in->eik_points) || (d.n_ds > 0 && (!in->ds_on || !in->ds_jit || !in->ds_counts)))
        return mv_fail(-1, "mvsdf_step_forward: missing input");
    hipStream_t s = (hipStream_t)stream;
    if (!st->counts_host) {                                       // first forward: host-side staging for the hit counts
        ST_HIP(hipHostMalloc((void**)&st->counts_host, MVSDF_STEP_COUNT_RING * 8 * sizeof(long long), hipHostMallocMapped | hipHostMallocCoherent));
        memset(st->counts_host, 0, MVSDF_STEP_COUNT_RING * 8 * sizeof(long long));
        // the partition kernel writes the counts straight into this buffer (no D2H copy node between two kernels)
        if (hipHostGetDevicePointer((void**)&st->counts_host_dev, st->counts_host, 0) != hipSuccess) { (void)hipGetLastError(); st->counts_host_dev = nullptr; }
        if (hipEventCreateWithFlags(&st->ev_counts, hipEventDisableTiming) != hipSuccess) {
            hipHostFree(st->counts_host); st->counts_host = nullptr;
            return mv_fail(-1, "mvsdf_step_forward: hipEventCreate failed");
        }
    }
    char* fwd = (char*)fwd_;
    const MvsdfStepLayout& L = st->lay;
    const FwdOffsets& fo = st->fo;
    const int R = st->R, E = st->E, M = st->M, nl = st->nl;
    if (st->timing) ST_HIP(hipEventRecord(st->ev_t[8], s));
    // 1. weight-norm fold + MFMA packs of both networks (idr.py:70-71; one fold per step instead of one per network call)
    float* w[MVSDF_STEP_MAX_LAYERS]; float* wp[MVSDF_STEP_MAX_LAYERS]; float* wpT[MVSDF_STEP_MAX_LAYERS];
    for (int l = 0; l < nl; ++l) { w[l] = (float*)(fwd + fo.w[l]); wp[l] = (float*)(fwd + fo.wp[l]); wpT[l] = (float*)(fwd + fo.wpT[l]); }
    float* ray_dirs = (float*)(fwd + L.ray_dirs); float* cam_loc = (float*)(fwd + L.cam_loc);
    {
        void* wp16[MVSDF_STEP_MAX_LAYERS];
        void* wx3[MVSDF_STEP_MAX_LAYERS]; void* wx3T[MVSDF_STEP_MAX_LAYERS];
        for (int l = 0; l < nl; ++l) {
            const bool bf = l < d.n_sdf && d.trace_dtype != 0;
            wp16[l] = bf ? (void*)(fwd + fo.wp16[l]) : nullptr;
            const bool x3 = l < d.n_sdf && fo.chain_x3;
            wx3[l] = (x3 && d.trace_dtype != 5) ? (void*)(fwd + fo.wx3[l]) : nullptr;       // (trace_dtype 5: the tracer's pack IS this pack)
            wx3T[l] = x3 ? (void*)(fwd + fo.wx3T[l]) : nullptr;
        }
        const MvWp16Mode wp16_mode = d.trace_dtype == 2 ? MV_WP16_ROUNDED_F32 : (d.trace_dtype == 5 ? MV_WP16_X3 : MV_WP16_BF16);
        // ... and the camera rays (idr.py:190), all in one launch
        // the CPU-generator draws (min-sdf steps, eikonal points) may arrive in pinned host memory: the prologue reads them from there
        const float* stage_dev = nullptr;
        if (in->host_stage) {
            if (hipHostGetDevicePointer((void**)&stage_dev, (void*)in->host_stage, 0) != hipSuccess || !stage_dev) {
                (void)hipGetLastError();
                return mv_fail(-1, "mvsdf_step_forward: host_stage is not device-visible pinned memory");
            }
        }
        // what a later mvsdf_step_resolve_unhit reads and the caller does not keep: the SDF net's biases (the parameters move on with the optimiser) and the min-sdf steps
        float* bias_copy[MVSDF_STEP_MAX_LAYERS];
        for (int l = 0; l < nl; ++l) bias_copy[l] = (lazy && l < d.n_sdf) ? (float*)(fwd + fo.bias[l]) : nullptr;
        float* steps_copy = lazy ? (float*)(fwd + fo.steps) : nullptr;
        if (lazy && !stage_dev) ST_HIP(hipMemcpyAsync(steps_copy, in->minsdf_steps, (size_t)d.tp.n_steps * 4, hipMemcpyDeviceToDevice, s));
        ST_TRY(mv_step_prologue(nl, prm->v, prm->g, d.N, d.K, w, wp, wpT, wp16, wp16_mode, wx3, wx3T, in->uv, in->pose, in->intrinsics, d.B, d.P, ray_dirs, cam_loc,
                                (uint8_t*)(fwd + L.object_mask_out), (unsigned long long*)(fwd + L.counters), stage_dev, (float*)in->minsdf_steps, d.tp.n_steps,
                                (float*)in->eik_points, 3 * d.n_eik, steps_copy, prm->b, bias_copy, stream));
    }
    MvsdfNetDesc sdf, sdfT, rnd, rndT;
    make_descs(*st, prm, fwd, &sdf, &sdfT, &rnd, &rndT);
    float* x_eval = (float*)(fwd + fo.x_eval); float* y_eval = (float*)(fwd + fo.y_eval); float* n_eval = (float*)(fwd + fo.n_eval);
    FwdGather g;                                                  // the evaluation rows [samples | traced points of the rays, hit first]
    g.eik = in->eik_points; g.on = in->ds_on; g.jit = in->ds_jit; g.pts = (float*)(fwd + L.points); g.perm = (long long*)(fwd + L.perm);
    g.n_eik = d.n_eik; g.n_ds = d.n_ds; g.x_out = x_eval;
    // 1b. the E sample rows of the fused value + normal evaluation (idr.py:240-275) depend on the folded weights only: where the rows of the rays
    // alone make a shorter launch (mv_chain_split_pays), the samples run NOW on a side stream, on the CUs the sphere tracer's latency chains
    // leave idle, and join before the rays' launch.  Rows are independent: no bit changes.  MVSDF_SPLIT_ROWS=0 / 1 forces one launch / the split.
    if (st->split_rows < 0) {
        const char* e = getenv("MVSDF_SPLIT_ROWS");
        st->split_rows = (e && *e) ? (atoi(e) != 0 && E >= 1) : mv_chain_split_pays(&sdf, E, M);
        if (st->split_rows) {
            // lowest priority: the samples fill what the tracer leaves idle, they must not take CUs from its latency chains
            int prio_least = 0, prio_greatest = 0;
            if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess) { (void)hipGetLastError(); prio_least = 0; }
            if (hipStreamCreateWithPriority(&st->side, hipStreamNonBlocking, prio_least) != hipSuccess) { (void)hipGetLastError(); st->side = nullptr; st->split_rows = 0; }
            else if (hipEventCreateWithFlags(&st->ev_fork, hipEventDisableTiming) != hipSuccess ||
                     hipEventCreateWithFlags(&st->ev_join, hipEventDisableTiming) != hipSuccess) {
                // no events: run without the side stream from now on (every later forward would otherwise find split_rows == 1 with null events)
                (void)hipGetLastError();
                if (st->ev_fork) { (void)hipEventDestroy(st->ev_fork); st->ev_fork = nullptr; }
                if (st->ev_join) { (void)hipEventDestroy(st->ev_join); st->ev_join = nullptr; }
                (void)hipStreamDestroy(st->side);
                st->side = nullptr; st->split_rows = 0;
            }
        }
    }
    bool split = st->split_rows == 1;
    // Work enqueued on the side stream writes into `fwd`.  If anything fails between the fork and the join, the caller drops the block while that work may
    // still run, and the caching allocator (which knows the block on the MAIN stream only) could hand the memory out again: wait for the side stream first.
    struct SideGuard {
        hipStream_t side; bool armed;
        ~SideGuard() { if (armed && side) (void)hipStreamSynchronize(side); }
    } side_guard{st->side, false};
    if (split) ST_HIP(hipEventRecord(st->ev_fork, s));             // (the folded weights are ready here)
    // 1c. the sphere cut (deferring forward only: the eager sequence keeps its launches).  The sphere launch stops after st_iters + 1 evaluations; the rays that
    // are not done finish, with their sampler rows, beside the sampler windows of the others (on two streams: 1d); the streams join in front of the secant chains.
    if (st->cut_on < 0) {
        st->cut_on = st->cut_enable > 0 || (st->cut_enable < 0 && mv_trace_cut_pays(&sdf, R, d.mt));
        if (st->cut_on && !st->late) {
            if (hipStreamCreateWithFlags(&st->late, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); st->late = nullptr; st->cut_on = 0; }
            else if (hipEventCreateWithFlags(&st->ev_cut, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&st->ev_late, hipEventDisableTiming) != hipSuccess ||
                     hipEventCreateWithFlags(&st->ev_main, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&st->ev_part, hipEventDisableTiming) != hipSuccess) {
                (void)hipGetLastError();
                if (st->ev_cut) { (void)hipEventDestroy(st->ev_cut); st->ev_cut = nullptr; }
                if (st->ev_late) { (void)hipEventDestroy(st->ev_late); st->ev_late = nullptr; }
                if (st->ev_main) { (void)hipEventDestroy(st->ev_main); st->ev_main = nullptr; }
                if (st->ev_part) { (void)hipEventDestroy(st->ev_part); st->ev_part = nullptr; }
                (void)hipStreamDestroy(st->late);
                st->late = nullptr; st->cut_on = 0;
            }
        }
    }
    const bool cut = lazy && st->cut_on == 1;
    SideGuard late_guard{st->late, false};
    // 1d. the fork of a forward with the cut (mvsdf_step_set_fork; every other forward keeps its launches).  The late branch -- resume launch, late rows, their
    // reduction -- is the longer one and paid both event hand-offs: it stays on the launch stream behind the cut launch, with no event, and the sampler windows, which
    // have the slack, go to `late`.  The ray partition feeds the fused evaluation, not the secant chains: it runs on `late` beside them.  The late list's rows (and,
    // where measured to pay, the first window) are one chunk per compute unit at most: the sixteen-wave rows form (trace_route.h: mv_rows16_on).
    const bool late_main = cut && st->fork_late_main != 0, part_side = cut && st->fork_part_side != 0;
    int rows16 = 0;                                               // bit 0: first window, bit 1: late rows (the parts of mvsdf_trace_rows_stage)
    if (cut && st->fork_rows16 != 0) {
        if (st->fork_rows16 < 0) rows16 = mv_trace_rows16_pays(&sdf, R, d.mt, d.mt_samples) ? mv_rows16_uses() : 0;
        else if (!mv_trace_rows16_has(&sdf, d.mt_samples)) return mv_fail(-3, "mvsdf_step_forward: the sixteen-wave rows form was forced on for a network without it (mvsdf_step_set_fork)");
        else rows16 = st->fork_rows16 == 1 ? 3 : (st->fork_rows16 == 2 ? 2 : 1);
    }
    // 2. rays + RayTracing.forward (idr.py:190-199)
    float* points = (float*)(fwd + L.points); uint8_t* mask = (uint8_t*)(fwd + L.mask); float* dists = (float*)(fwd + L.dists);
    unsigned long long* counters = (unsigned long long*)(fwd + L.counters);
    auto stage = [&](int which) {
        if (lazy && which != 3)                                     // (no tail filling: the sphere kernel still writes the min-sdf work list and ranges)
            return mv_trace_stage_notail(which, &sdf, &d.tp, cam_loc, ray_dirs, in->object_mask, d.B, d.P, 1, in->intervals, in->minsdf_steps, points, mask, dists,
                                         counters, fwd + fo.trace_ws, fo.trace_ws_bytes, d.mt, d.mt_samples, stream);
        return mvsdf_trace_stage(which, &sdf, &d.tp, cam_loc, ray_dirs, in->object_mask, d.B, d.P, 1, in->intervals, in->minsdf_steps, points, mask, dists,
                                 counters, fwd + fo.trace_ws, fo.trace_ws_bytes, d.mt, d.mt_samples, stream);
    };
    if (st->timing) ST_HIP(hipEventRecord(st->ev_t[0], s));
    auto cut_stage = [&](int which, void* strm) {
        return mv_trace_cut_stage(which, st->cut_rounds, 1, &sdf, &d.tp, cam_loc, ray_dirs, in->object_mask, d.B, d.P, 1, in->intervals, in->minsdf_steps, points, mask, dists,
                                  counters, fwd + fo.trace_ws, fo.trace_ws_bytes, d.mt, d.mt_samples, strm);
    };
    // the sampler windows (stage 3) and the late list's rows + reduction (cut stage 3), each with its rows in the sixteen-wave form where `rows16` says so
    auto windows = [&](void* strm) {
        if (rows16 & 1) return mvsdf_trace_rows_stage(1, 1, st->fork_rows16_cap, &sdf, &d.tp, cam_loc, ray_dirs, in->object_mask, d.B, d.P, 1, in->intervals, in->minsdf_steps, points,
                                                      mask, dists, counters, fwd + fo.trace_ws, fo.trace_ws_bytes, d.mt, d.mt_samples, strm);
        return mvsdf_trace_stage(3, &sdf, &d.tp, cam_loc, ray_dirs, in->object_mask, d.B, d.P, 1, in->intervals, in->minsdf_steps, points, mask, dists,
                                 counters, fwd + fo.trace_ws, fo.trace_ws_bytes, d.mt, d.mt_samples, strm);
    };
    auto late_rows = [&](void* strm) {
        if (rows16 & 2) return mvsdf_trace_rows_stage(2, 1, st->fork_rows16_cap, &sdf, &d.tp, cam_loc, ray_dirs, in->object_mask, d.B, d.P, 1, in->intervals, in->minsdf_steps, points,
                                                      mask, dists, counters, fwd + fo.trace_ws, fo.trace_ws_bytes, d.mt, d.mt_samples, strm);
        return cut_stage(3, strm);
    };
    if (cut) {
        // the resume launch is enqueued BEFORE the first sampler window: its few one-per-CU workgroups are placed first.  late_main: it follows the cut launch on the
        // launch stream (no event in between) and `late` takes the windows; else it is the late branch that waits for ev_cut on `late`
        ST_TRY(cut_stage(1, stream));
        ST_HIP(hipEventRecord(st->ev_cut, s));
        if (late_main && st->timing) ST_HIP(hipEventRecord(st->ev_t[1], s));   // (behind the cut launch, as without the fork)
        ST_HIP(hipStreamWaitEvent(st->late, st->ev_cut, 0));
        late_guard.armed = true;
        void* branch = late_main ? stream : (void*)st->late;
        ST_TRY(cut_stage(2, branch));
        ST_TRY(late_rows(branch));
        if (!late_main) ST_HIP(hipEventRecord(st->ev_late, st->late));
    } else if (lazy) ST_TRY(stage(1));
    else ST_TRY(mv_trace_stage1_prezeroed(&sdf, &d.tp, cam_loc, ray_dirs, in->object_mask, d.B, d.P, 1, in->intervals, in->minsdf_steps, points, mask, dists,
                                     counters, fwd + fo.trace_ws, fo.trace_ws_bytes, d.mt, d.mt_samples, stream));   // counters zeroed by the prologue
    if (st->timing && !late_main) ST_HIP(hipEventRecord(st->ev_t[1], s));
    if (split) {                                                  // enqueued AFTER the sphere tracer: its workgroups take the CUs first
        ST_HIP(hipStreamWaitEvent(st->side, st->ev_fork, 0));
        side_guard.armed = true;
        const int rcs = mv_sdf_forward_gather(&sdf, &sdfT, nullptr, &g, M, M, 0, E, y_eval, n_eval, (float*)(fwd + fo.sdf_ctx), st->side);
        if (rcs == 1) { split = false; side_guard.armed = false; }   // per-layer route: nothing was launched, one pass over all rows below
        else if (rcs) return rcs;
        else ST_HIP(hipEventRecord(st->ev_join, st->side));
    }
    ST_TRY(windows(late_main ? (void*)st->late : stream));        // the hit mask is final here (ray_tracing.py:61)
    if (late_main) ST_HIP(hipEventRecord(st->ev_late, st->late));
    // the partition beside the secant chains: `late` gets the launch stream's share of the mask (ev_main) behind its own and runs it; the launch stream goes on to the
    // secant chains, which read the lists both branches appended to and nothing the partition writes, and waits for ev_part in front of the fused evaluation
    if (part_side) { ST_HIP(hipEventRecord(st->ev_main, s)); ST_HIP(hipStreamWaitEvent(st->late, st->ev_main, 0)); }
    if (cut) { ST_HIP(hipStreamWaitEvent(s, st->ev_late, 0)); late_guard.armed = part_side; }   // ... with the other branch's share of it (`late` is still written to while it owes the partition)
    if (st->timing) ST_HIP(hipEventRecord(st->ev_t[2], s));
    hipStream_t ps = part_side ? st->late : s;                    // the partition's stream
    // 3. stable partition (hit rays first) + both counts; they start travelling to the host while the rest of the forward runs
    long long* perm = (long long*)(fwd + L.perm); long long* inv = (long long*)(fwd + fo.inv); long long* true_rows = (long long*)(fwd + fo.true_rows);
    long long* counts = (long long*)(fwd + fo.counts); float* view_sorted = (float*)(fwd + fo.view_sorted);
    ST_TRY(mv_partition_rays_step(mask, d.use_object_mask ? in->object_mask : nullptr, in->object_mask_true, ray_dirs, R, perm, inv, true_rows, counts,
                                  view_sorted, (int*)(fwd + fo.true_rank), d.n_ds > 0 ? in->ds_counts : nullptr,
                                  st->counts_host_dev ? st->counts_host_dev + 8 * ((st->counts_seq + 1) % MVSDF_STEP_COUNT_RING) : nullptr, st->counts_seq + 1,
                                  (float*)(fwd + fo.counts + 32), d.n_eik, d.n_ds, d_mask, e_mask, (void*)ps));
    ++st->counts_seq;
    if (!st->counts_host_dev) {                                   // (pinned memory not mapped: a copy and an event)
        ST_HIP(hipMemcpyAsync(st->counts_host, counts, 4 * sizeof(long long), hipMemcpyDeviceToHost, ps));
        ST_HIP(hipEventRecord(st->ev_counts, ps));
    }
    if (part_side) ST_HIP(hipEventRecord(st->ev_part, st->late));
    // counts_stream: a stream whose completion implies that the partition has run.  The launch stream is one also when the partition runs on `late`: it waits for
    // ev_part below, inside this forward
    st->counts_pending = true; st->counts_stream = s;
    if (st->timing) ST_HIP(hipEventRecord(st->ev_t[3], s));
    ST_TRY(stage(lazy ? 7 : 4));                                  // secant (+ min-sdf rows unless they are left to mvsdf_step_resolve_unhit): only points / dists still move
    mv_trace_last_grid(st->last_grid);
    if (st->timing) { ST_HIP(hipEventRecord(st->ev_t[4], s)); st->timed = true; }
    // 4. ONE fused value + normal evaluation over [samples | rays, hit first], rendering net on every sorted ray, output gather
    {
        // (the rows are gathered inside the chain kernel, which also leaves them in x_eval)
        if (split) { ST_HIP(hipStreamWaitEvent(s, st->ev_join, 0)); side_guard.armed = false; }   // the main stream is ordered behind the side work from here on
        if (part_side) { ST_HIP(hipStreamWaitEvent(s, st->ev_part, 0)); late_guard.armed = false; }   // perm / inv / counts / view_sorted are read from here on
        // lazy: the rays' rows end at E + N on the device (cnt_mode 1); workgroups wholly beyond leave at once
        int rcf = mv_sdf_forward_gather_cnt(&sdf, &sdfT, nullptr, &g, M, M, split ? E : 0, M, lazy ? counts : nullptr, E, 1, y_eval, n_eval, (float*)(fwd + fo.sdf_ctx), stream);
        if (rcf == 1 && lazy) return mv_fail(-3, "mvsdf_step_forward: the fused forward chain refused a step it was said to cover");
        if (rcf == 1) {                                           // per-layer route: materialise the rows first
            const int total = M * 3;
            hipLaunchKernelGGL(k_step_gather_x, dim3((total + 255) / 256), dim3(256), 0, s, in->eik_points, d.n_eik, in->ds_on, in->ds_jit, d.n_ds, points, perm,
                               R, x_eval, (uint8_t*)nullptr);
            ST_HIP(hipGetLastError());
            rcf = mvsdf_sdf_forward(&sdf, &sdfT, x_eval, M, M, y_eval, n_eval, (float*)(fwd + fo.sdf_ctx), stream);
        }
        if (rcf) return rcf;
    }
    float* rgb_sorted = (float*)(fwd + fo.rgb_sorted);
    ST_TRY(mvsdf_render_forward(&rnd, x_eval + 3 * (size_t)E, view_sorted, n_eval + 3 * (size_t)E, y_eval + (size_t)E * st->Nout + 2, st->Nout, R,
                                d.view_spec, rgb_sorted, (float*)(fwd + fo.render_ctx), stream));
    ST_TRY((lazy ? mv_step_outputs_hit : mvsdf_step_outputs)(R, d.n_eik, d.n_ds, st->Nout, counts, x_eval, y_eval, n_eval, inv, true_rows, rgb_sorted, d_mask, e_mask,
                              (float*)(fwd + L.rgb_values), (float*)(fwd + L.sdf_output), (float*)(fwd + L.diff_pts), (float*)(fwd + L.eik_out),
                              (float*)(fwd + L.points_hom), (float*)(fwd + L.grad_theta), (float*)(fwd + L.surf), stream));
    if (st->timing) ST_HIP(hipEventRecord(st->ev_t[5], s));
    return 0;
}

// What a forward in MVSDF_STEP_UNHIT_DEFER mode left out, from its forward block alone: the folded weights and packs, this forward's copy of the biases and of the
// min-sdf steps, the tracer's workspace (min-sdf work list, ranges) and counters, rays, perm and counts all live there.  Same kernels as the eager step, rows
// independent of their chunk / tile: the same bits, at that step's network, however many optimiser steps later.
int mvsdf_step_resolve_unhit(void* step, void* fwd_, void* stream) {
    Step* st = (Step*)step;
    if (!st || !fwd_) return mv_fail(-1, "mvsdf_step_resolve_unhit: null argument");
    if (!st->can_lazy) return mv_fail(-3, "mvsdf_step_resolve_unhit: not available for this step (mvsdf_step_can_defer_unhit)");
    const MvsdfStepDesc& d = st->d;
    char* fwd = (char*)fwd_;
    const MvsdfStepLayout& L = st->lay;
    const FwdOffsets& fo = st->fo;
    const int R = st->R, E = st->E, M = st->M;
    MvsdfStepParams prm;
    memset(&prm, 0, sizeof(prm));
    for (int l = 0; l < d.n_sdf; ++l) prm.b[l] = (const float*)(fwd + fo.bias[l]);
    MvsdfNetDesc sdf, sdfT, rnd, rndT;
    make_descs(*st, &prm, fwd, &sdf, &sdfT, &rnd, &rndT);            // (the rendering net's descriptors are not used)
    float* points = (float*)(fwd + L.points); uint8_t* mask = (uint8_t*)(fwd + L.mask); float* dists = (float*)(fwd + L.dists);
    const float* steps = (const float*)(fwd + fo.steps);
    // 1. minimal_sdf_points: the min-sdf rows alone + their reduction (points / dists of the listed rays); the all-ones mask of the block stands in for the object
    //    mask, which these launches do not read (the list entries carry what the sphere kernel decided from it)
    ST_TRY(mv_trace_stage_notail(5, &sdf, &d.tp, (const float*)(fwd + L.cam_loc), (const float*)(fwd + L.ray_dirs), (const uint8_t*)(fwd + L.object_mask_out), d.B, d.P, 1,
                                 steps, steps, points, mask, dists, (unsigned long long*)(fwd + L.counters), fwd + fo.trace_ws, fo.trace_ws_bytes, d.mt, d.mt_samples, stream));
    // 2. the evaluation rows of the rays without a hit: [E + N, E + R), N on the device (cnt_mode 2), through the chain kernel of the eager step
    FwdGather g;
    memset(&g, 0, sizeof(g));
    g.pts = points; g.perm = (long long*)(fwd + L.perm); g.n_eik = d.n_eik; g.n_ds = d.n_ds; g.x_out = (float*)(fwd + fo.x_eval);
    const long long* counts = (const long long*)(fwd + fo.counts);
    float* y_eval = (float*)(fwd + fo.y_eval);
    const int rcf = mv_sdf_forward_gather_cnt(&sdf, &sdfT, nullptr, &g, M, M, E, M, counts, E, 2, y_eval, (float*)(fwd + fo.n_eval), (float*)(fwd + fo.sdf_ctx), stream);
    if (rcf) return rcf == 1 ? mv_fail(-3, "mvsdf_step_resolve_unhit: the fused forward chain refused a step it was said to cover") : rcf;
    // 3. their sdf_output
    return mv_step_unhit_scatter(R, E, st->Nout, counts, y_eval, g.perm, (float*)(fwd + L.sdf_output), stream);
}
int mvsdf_step_can_defer_unhit(void* step) { Step* st = (Step*)step; return (st && st->can_lazy) ? 1 : 0; }
int mvsdf_step_last_tracer_grid(void* step, int out[2]) {
    Step* st = (Step*)step;
    if (!st || !out) return mv_fail(-1, "mvsdf_step_last_tracer_grid: null argument");
    out[0] = st->last_grid[0]; out[1] = st->last_grid[1];
    return 0;
}

// wait (bounded spin, then short sleeps: a rank that shares its cores with others must not burn them) until forward `seq` has stored its record
static int step_wait_seq(Step* st, long long seq, long long counts[4]) {
    long long* slot = st->counts_host + 8 * (seq % MVSDF_STEP_COUNT_RING);
    // the partition kernel stores the forward's sequence number behind the counts (release, system scope): poll it.  Should it never arrive
    // (the stream drained or failed without the kernel having run), the stream's status ends the wait.
    for (unsigned long long it = 1;; ++it) {
        const long long have = __atomic_load_n(&slot[4], __ATOMIC_ACQUIRE);
        if (have == seq) break;
        if (have > seq) return mv_fail(-4, "mvsdf_step_wait_counts_seq: the record of that forward was overwritten (read the counts from its forward block)");
        if (it < 5000) { __builtin_ia32_pause(); continue; }       // ~50-100 us of spinning: the common case (the kernel is about to run)
        struct timespec ts = {0, 20000};                            // then 20 us naps
        nanosleep(&ts, nullptr);
        if ((it & 0x3ff) == 0 && seq == st->counts_seq) {
            const hipError_t q = hipStreamQuery(st->counts_stream);
            if (q == hipSuccess) {
                if (__atomic_load_n(&slot[4], __ATOMIC_ACQUIRE) == seq) break;
                return mv_fail(-1, "mvsdf_step_wait_counts: the forward finished without delivering its counts");
            }
            if (q != hipErrorNotReady) return mv_check(q, "mvsdf_step_wait_counts (hipStreamQuery)");
        }
    }
    for (int i = 0; i < 4; ++i) counts[i] = slot[i];
    // the slot may have been rewritten while we copied (a forward RING steps later): the number decides
    if (__atomic_load_n(&slot[4], __ATOMIC_ACQUIRE) != seq) return mv_fail(-4, "mvsdf_step_wait_counts_seq: the record of that forward was overwritten (read the counts from its forward block)");
    return 0;
}

int mvsdf_step_wait_counts(void* step, long long counts[4]) {
    Step* st = (Step*)step;
    if (!st || !counts) return mv_fail(-1, "mvsdf_step_wait_counts: null argument");
    if (!st->counts_pending) return mv_fail(-1, "mvsdf_step_wait_counts: no forward is in flight");
    if (!st->counts_host_dev) {
        ST_HIP(hipEventSynchronize(st->ev_counts));
        for (int i = 0; i < 4; ++i) counts[i] = st->counts_host[i];
        st->counts_pending = false;
        return 0;
    }
    const int rc = step_wait_seq(st, st->counts_seq, counts);
    st->counts_pending = false;
    return rc;
}

long long mvsdf_step_seq(void* step) { return step ? ((Step*)step)->counts_seq : -1; }
size_t mvsdf_step_counts_offset(void* step) { return step ? ((Step*)step)->fo.counts : 0; }
int mvsdf_step_can_defer(void* step) { Step* st = (Step*)step; return (st && st->can_defer) ? 1 : 0; }
int mvsdf_step_saved_offsets(void* step, size_t out[6]) {
    Step* st = (Step*)step;
    if (!st || !out) return mv_fail(-1, "mvsdf_step_saved_offsets: null argument");
    out[0] = st->fo.x_eval; out[1] = st->fo.y_eval; out[2] = st->fo.n_eval; out[3] = st->fo.view_sorted; out[4] = st->fo.render_ctx; out[5] = st->fo.rgb_sorted;
    return 0;
}
int mvsdf_step_pack_offsets(void* step, int layer, size_t out[7]) {
    Step* st = (Step*)step;
    if (!st || !out || layer < 0 || layer >= st->nl) return mv_fail(-1, "mvsdf_step_pack_offsets: null argument / no such layer");
    const FwdOffsets& fo = st->fo;
    const int l = layer, td = st->d.trace_dtype;
    const bool sdf = l < st->d.n_sdf, x3 = sdf && fo.chain_x3;
    const size_t none = (size_t)-1;
    out[0] = fo.w[l]; out[1] = fo.wp[l]; out[2] = fo.wpT[l];
    out[3] = (sdf && td >= 2 && td <= 5) ? fo.wp16[l] : none;
    out[4] = x3 ? fo.wx3[l] : none; out[5] = x3 ? fo.wx3T[l] : none;
    out[6] = sdf ? fo.bias[l] : none;
    return 0;
}

int mvsdf_step_wait_counts_seq(void* step, long long seq, long long counts[4]) {
    Step* st = (Step*)step;
    if (!st || !counts) return mv_fail(-1, "mvsdf_step_wait_counts_seq: null argument");
    if (seq <= 0 || seq > st->counts_seq || !st->counts_host) return mv_fail(-1, "mvsdf_step_wait_counts_seq: no such forward");
    if (!st->counts_host_dev) {                                   // (unmapped pinned memory: one record, the last forward's)
        if (seq != st->counts_seq) return mv_fail(-4, "mvsdf_step_wait_counts_seq: the record of that forward was overwritten (read the counts from its forward block)");
        ST_HIP(hipEventSynchronize(st->ev_counts));
        for (int i = 0; i < 4; ++i) counts[i] = st->counts_host[i];
        return 0;
    }
    if (seq + MVSDF_STEP_COUNT_RING <= st->counts_seq) return mv_fail(-4, "mvsdf_step_wait_counts_seq: the record of that forward was overwritten (read the counts from its forward block)");
    const int rc = step_wait_seq(st, seq, counts);
    if (rc == 0 && seq == st->counts_seq) st->counts_pending = false;
    return rc;
}

long long mvsdf_step_done_seq(void* step, long long counts[4]) {
    Step* st = (Step*)step;
    if (!st || !st->counts_host || !st->counts_host_dev) return 0;
    // kernels of one stream finish in order: walk back from the newest forward to the first slot that carries its own number
    for (long long seq = st->counts_seq; seq > 0 && seq + MVSDF_STEP_COUNT_RING > st->counts_seq; --seq) {
        long long* slot = st->counts_host + 8 * (seq % MVSDF_STEP_COUNT_RING);
        if (__atomic_load_n(&slot[4], __ATOMIC_ACQUIRE) != seq) continue;
        if (counts) {
            for (int i = 0; i < 4; ++i) counts[i] = slot[i];
            if (__atomic_load_n(&slot[4], __ATOMIC_ACQUIRE) != seq) continue;
        }
        return seq;
    }
    return 0;
}

static int step_backward_impl(void* step, const MvsdfStepParams* prm, int N, int n_true, int d_mask, int e_mask, int use_geo, const float* d_diff,
                        const float* d_rgb, const float* d_gth, const float* d_eo, const float* d_si, const void* fwd_, void* bwd_,
                        float* const* dv, float* const* dg, float* const* db, int accumulate, void* stream) {
    Step* st = (Step*)step;
    if (!st || !prm || !fwd_ || !bwd_ || !dv || !dg || !db) return mv_fail(-1, "mvsdf_step_backward: null argument");
    const MvsdfStepDesc& d = st->d;
    const int R = st->R, E = st->E, M = st->M, nl = st->nl, Nout = st->Nout;
    hipStream_t s = (hipStream_t)stream;
    const char* fwd = (const char*)fwd_;
    // N < 0: the deferred step.  {N, n_true} stay on the device (`cnt`, written by this forward's ray partition); every launch below is sized for N = R and bounds
    // its rows by them (step_internal.h, "device-side counts").  n_true then carries a hint of N that only selects kernel forms.
    const long long* cnt = nullptr;
    int n_hint = -1;
    if (N < 0) {
        if (!st->can_defer) return mv_fail(-3, "mvsdf_step_backward: N < 0 (device-side counts) is not available for this step (mvsdf_step_can_defer)");
        cnt = (const long long*)(fwd + st->fo.counts);
        n_hint = (n_true >= 0 && n_true <= R) ? n_true : R;
        N = R; n_true = R;
    }
    if (N < 0 || N > R || n_true < 0 || n_true > N) return mv_fail(-1, "mvsdf_step_backward: bad counts");
    char* bwd = (char*)bwd_;
    const MvsdfStepLayout& L = st->lay;
    const FwdOffsets& fo = st->fo;
    const BwdOffsets& bo = st->bo;
    MvsdfNetDesc sdf, sdfT, rnd, rndT;
    make_descs(*st, prm, fwd, &sdf, &sdfT, &rnd, &rndT);
    const int Mb = E + N;
    float* dflat = (float*)(bwd + L.dflat);
    float* dW_s = dflat + st->seg[0][0]; float* db_s = dflat + st->seg[0][1];
    float* dW_r = dflat + st->seg[1][0]; float* db_r = dflat + st->seg[1][1];
    float* dy = (float*)(bwd + bo.dy); float* dn = (float*)(bwd + bo.dn);
    const float* x_eval = (const float*)(fwd + fo.x_eval); const float* n_eval = (const float*)(fwd + fo.n_eval);
    const float* view_sorted = (const float*)(fwd + fo.view_sorted); const long long* true_rows = (const long long*)(fwd + fo.true_rows);
    const float* ctx = (const float*)(fwd + fo.sdf_ctx);
    const int dv_ = (d.view_spec & 0x100) ? 0 : 3 + 6 * (d.view_spec & 0xff), dnr = (d.view_spec & 0x200) ? 0 : 3;
    const int nrm0 = dnr ? 3 + dv_ : -1, feat0 = 3 + dv_ + dnr;                          // column layout of the rendering net's input (functional.render_offsets)
    if (Mb == 0) {                                                                      // nothing was evaluated with a gradient
        ST_HIP(hipMemsetAsync(dflat, 0, L.dflat_floats * 4, s));
    } else {
        const float* din = nullptr;
        // rendering-net backward over the N hit rows (idr.py:302-304: only they reach rgb_values): the descending chain now, its weight
        // gradients together with the SDF net's further down
        const bool with_r = N > 0 && d_rgb;
        if (with_r) {
            // (the upstream arrives in ray order; the net ran on the sorted rows: the chain kernel reads row r from d_rgb[perm[r]])
            float* drgb_sorted = (float*)(bwd + bo.drgb_sorted);
            float* din_w = (float*)(bwd + bo.din);
            int rcb = mv_render_backward_chain(&rnd, &rndT, N, R, d_rgb, (const long long*)(fwd + L.perm), (const float*)(fwd + fo.render_ctx), din_w,
                                               (float*)(bwd + bo.render_ws), cnt, stream);
            if (rcb == -3 && !cnt) {                                                            // per-layer route: gather first
                hipLaunchKernelGGL(k_step_gather_drgb, dim3((3 * N + 255) / 256), dim3(256), 0, s, d_rgb, (const long long*)(fwd + L.perm), N, drgb_sorted);
                rcb = mv_render_backward_chain(&rnd, &rndT, N, R, drgb_sorted, nullptr, (const float*)(fwd + fo.render_ctx), din_w, (float*)(bwd + bo.render_ws), nullptr, stream);
            }
            if (rcb) return rcb;
            din = din_w;
        } else {
            ST_HIP(hipMemsetAsync(dflat + st->seg[1][0], 0, (st->seg[1][2] - st->seg[1][0]) * 4, s));
        }
        const float* rctx = with_r ? (const float*)(fwd + fo.render_ctx) : nullptr;
        float* rws = with_r ? (float*)(bwd + bo.render_ws) : nullptr;
        float* wsA = (float*)(bwd + bo.wsA);
        bool done = false;
        if (cnt && !(din && N > 0)) return mv_fail(-3, "mvsdf_step_backward: device-side counts need the upstream of rgb_values (the fused route)");
        if (din && N > 0) {
            // (X) input adjoint of the surface points for the rendering net's upstream alone, (A) the full pass with every upstream except
            // SampleNetwork's scalar: independent, one grid; then fbar = -xbar.v / n.v and a first-order delta pass.
            // Both upstreams come out of ONE gather pass (the staged route: zero-fill + rendering-net adjoints, two row-block copies, scatter).
            float* dy_x = (float*)(bwd + bo.dy_x); float* dn_x = (float*)(bwd + bo.dn_x);
            ST_TRY(mv_step_backward_assemble(d.n_eik, d.n_ds, N, Nout, n_true, din, st->K0r, feat0, nrm0, use_geo, (const int*)(fwd + fo.true_rank), d_eo,
                                             d_gth, d_si, d_mask, e_mask, dy, dn, dy_x, dn_x, cnt, stream));
            float* dx = (float*)(bwd + bo.dx);
            int rc = mv_sdf_backward_pair_cnt(&sdf, &sdfT, M, M, Mb, dy, dn, wsA, E, N, dy_x, use_geo ? dn_x : nullptr, (float*)(bwd + bo.wsX), dx, ctx, cnt, n_hint, stream);
            if (rc == 0) {
                // SampleNetwork's scalar (f = -xbar.v / n.v, App. E.6), its adjoints as fbar x s_l (one elementwise launch: the forward saved s_l), then the
                // weight gradients of BOTH networks in one k_wgrad_net / k_reduce_net pair.  (Round 3 ran the chunks that do not depend on fbar on a
                // second stream beside a 9-phase delta chain; with the delta reduced to ~10 us the split measured no gain and is gone.)
                float* fbar = (float*)(bwd + bo.fbar);
                if (mv_dev_switches().delta_chain && !cnt) {                                      // MVSDF_DELTA_CHAIN=1: the cross-check route
                    ST_TRY(mvsdf_step_backward_fbar(d.n_eik, d.n_ds, N, Nout, din, st->K0r, use_geo, d_diff, dx, view_sorted, n_eval, dy, fbar, stream));
                    ST_TRY(mv_sdf_backward_delta(&sdf, &sdfT, M, M, Mb, ctx, wsA, E, N, fbar, stream));
                } else {
                    ST_TRY(mv_sdf_backward_delta_fbar(&sdf, M, M, Mb, ctx, wsA, E, N, Nout, din, st->K0r, use_geo, d_diff, dx, view_sorted, n_eval, dy, fbar, cnt, stream));
                }
                ST_TRY(mv_step_wgrad(&sdf, &rnd, M, M, Mb, dy, ctx, wsA, with_r ? N : 0, R, rctx, rws, dW_s, db_s, dW_r, db_r, cnt, E, stream));
                done = true;
            } else if (rc == -3 && !cnt) {                                                      // network too wide for the fused chains: the sequential route
                ST_TRY(mvsdf_sdf_backward(&sdf, &sdfT, x_eval + 3 * (size_t)E, M, M, E, N, dy_x, use_geo ? dn_x : nullptr, ctx, nullptr, nullptr, dx, wsA, stream));
                float* fbar = (float*)(bwd + bo.fbar);
                ST_TRY(mvsdf_step_backward_fbar(d.n_eik, d.n_ds, N, Nout, din, st->K0r, use_geo, d_diff, dx, view_sorted, n_eval, dy, fbar, stream));
            } else {
                return rc;
            }
        } else {
            ST_TRY(mvsdf_step_backward_inputs(0, d.n_eik, d.n_ds, N, Nout, n_true, din, st->K0r, feat0, nrm0, use_geo, nullptr, nullptr, view_sorted, n_eval,
                                              true_rows, nullptr, nullptr, nullptr, d_mask, e_mask, dy, dn, stream));
            ST_TRY(mvsdf_step_backward_inputs(1, d.n_eik, d.n_ds, N, Nout, n_true, din, st->K0r, feat0, nrm0, use_geo, d_diff, nullptr, view_sorted, n_eval,
                                              true_rows, d_eo, d_gth, d_si, d_mask, e_mask, dy, dn, stream));
        }
        if (!done) {
            // (routes without the split: the SDF net's gradients by the general backward, the rendering net's by its own wgrad pair)
            ST_TRY(mvsdf_sdf_backward(&sdf, &sdfT, x_eval, M, M, 0, Mb, dy, dn, ctx, dW_s, db_s, nullptr, wsA, stream));
            if (with_r) {
                // the rendering net alone: its slabs through the general entry point would redo the chain; reduce them with the shared helper instead
                // (an SDF-less call of mv_step_wgrad is not defined, so: the classic full call)
                float* drgb_sorted = (float*)(bwd + bo.drgb_sorted);
                hipLaunchKernelGGL(k_step_gather_drgb, dim3((3 * N + 255) / 256), dim3(256), 0, s, d_rgb, (const long long*)(fwd + L.perm), N, drgb_sorted);
                ST_TRY(mvsdf_render_backward(&rnd, &rndT, N, R, drgb_sorted, rctx, dW_r, db_r, (float*)(bwd + bo.din), rws, stream));
            }
        }
    }
    // weight-norm fold backward of both networks: dW / db -> dv, dg, db, added into the targets when accumulate
    const float* dWl[MVSDF_STEP_MAX_LAYERS]; const float* dbl[MVSDF_STEP_MAX_LAYERS];
    for (int l = 0; l < nl; ++l) { dWl[l] = dflat + st->woff[l]; dbl[l] = dflat + st->boff[l]; }
    return mvsdf_fold_backward_net(nl, prm->v, prm->g, dWl, dbl, d.N, d.K, dv, dg, db, accumulate ? 1 : 0, stream);
}

int mvsdf_step_backward(void* step, const MvsdfStepParams* prm, int N, int n_true, int d_mask, int e_mask, int use_geo, const float* d_diff,
                        const float* d_rgb, const float* d_gth, const float* d_eo, const float* d_si, const void* fwd_, void* bwd_,
                        float* const* dv, float* const* dg, float* const* db, int accumulate, void* stream) {
    Step* st = (Step*)step;
    const bool timing = st && st->timing;
    if (timing) ST_HIP(hipEventRecord(st->ev_t[6], (hipStream_t)stream));
    const int rc = step_backward_impl(step, prm, N, n_true, d_mask, e_mask, use_geo, d_diff, d_rgb, d_gth, d_eo, d_si, fwd_, bwd_, dv, dg, db, accumulate, stream);
    if (rc) return rc;
    if (timing) { ST_HIP(hipEventRecord(st->ev_t[7], (hipStream_t)stream)); st->timed_bwd = true; }
    return 0;
}

}  // extern "C"

extern "C" int mvsdf_abi_struct_sizes(size_t* out) {
    if (!out) return mv_fail(-1, "mvsdf_abi_struct_sizes: null argument");
    out[0] = sizeof(MvsdfNetDesc); out[1] = sizeof(MvsdfTraceParams); out[2] = sizeof(MvsdfStepDesc); out[3] = sizeof(MvsdfStepParams);
    out[4] = sizeof(MvsdfStepInputs); out[5] = sizeof(MvsdfStepLayout); out[6] = sizeof(MvsdfLossArgs); out[7] = sizeof(MvsdfLossLayout);
    return 8;
}

