// capi_util.h -- helpers shared by the extern "C" entry points.
#pragma once
#include <hip/hip_runtime.h>
#include "mlp_common.h"
#include "tile_engine_bf16.h"
#include "tile_engine_bf16s.h"
#include "trace_route.h"
#include "../../include/mvsdf_hip.h"

#include <stdlib.h>
int mv_fail(int code, const char* msg);          // records msg, returns code
// Development / A-B switches (alternative launch paths that are independent implementations of the same passes) exist only in a library built with
// -DMVSDF_DEV_SWITCHES (mvsdf_amd/build.py: build(tag='dev'); tests/test_gpu_alt_paths.py and the sweep tools load it through MVSDF_LIB).  The product library never
// reads them: its behaviour does not depend on stray environment variables.  The list: diff_route.h::MvDevSwitches for the differentiable passes,
// trace_route.h::MvTraceSwitches for the tracer (with its product switch MVSDF_TAIL); MVSDF_SGM_LGH / _LGV where they are read.  (The other product switch, read
// with getenv directly: MVSDF_SPLIT_ROWS.)
static inline const char* mv_dev_env(const char* name) {
#ifdef MVSDF_DEV_SWITCHES
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}
const MvTraceSwitches& mv_trace_switches();       // the tracer's switches (trace_route.h), read once per process (trace.hip)
int mv_check(hipError_t e, const char* where);   // 0 on success
// mode 0: SDF net (PE input + skip chaining checked); 1: plain chain; 2: transposed packs (no chaining check)
int mv_make_net_mode(const MvsdfNetDesc* d, MvNet* net, int mode);
static inline int mv_make_net(const MvsdfNetDesc* d, MvNet* net) { return mv_make_net_mode(d, net, 0); }
int mv_make_net_bs(const MvsdfNetDesc* d, MvNetBf* net, int ns); // SDF net on the bf16 packs without duplicated columns, activations as ns bf16 terms (trace_dtype 3 / 4; net = an MvNetBs<ns>)
int mv_make_net_x3(const MvsdfNetDesc* d, MvNetBf* net);        // the three-term packs d->wx3 of the differentiable chains (chain_x3.h); 1: a layer has none (-> the fp32 chains)
int mv_make_net_trace(const MvsdfNetDesc* d, MvNet* net);     // the fp32-engine tracing net: the fp32 packs, or (trace_dtype == 2) the fp32 packs of the bf16-rounded weights
// skip layers of a descriptor as a bit mask (skip_mask wins; else the single skip_layer)
static inline unsigned mv_desc_skip_mask(const MvsdfNetDesc* d) { return d->skip_mask ? d->skip_mask : (d->skip_layer >= 0 ? 1u << d->skip_layer : 0u); }

// column tiles per wave the fused chain kernels need for this network (8 waves per workgroup): 2 up to width 256, 4 up to 512,
// 0 = too wide for them (per-layer kernels take over).  Width = the widest tile row ANY phase of a chain produces: the hidden layers' outputs N_l (value /
// E.1 chains over W_l) AND their inputs K_l (normal / E.2 chains over W_l^T produce K_l columns) -- a skip layer fed by a wider-than-hidden layer
// (dims[skip] > the other hidden widths) has K_skip > every N_l.
static inline int mv_chain_ntw(const MvNet& net) {
    int maxnt = 0;
    for (int l = 0; l < net.n_layers - 1; ++l) maxnt = net.L[l].NT > maxnt ? net.L[l].NT : maxnt;
    for (int l = 1; l < net.n_layers; ++l) { const int kt = (net.L[l].K + 15) / 16; maxnt = kt > maxnt ? kt : maxnt; }
    return maxnt <= 16 ? 2 : (maxnt <= 32 ? 4 : 0);
}

// 16-column tiles of the widest hidden layer (the maxnt of trace_route.h)
template <class NET> static inline int mv_hidden_nt(const NET& net) {
    int maxnt = 0;
    for (int l = 0; l < net.n_layers - 1; ++l) maxnt = net.L[l].NT > maxnt ? net.L[l].NT : maxnt;
    return maxnt;
}
// f(the tracing net of a descriptor in its engine's type: trace_route.h::MvTraceEngine), or the code of the descriptor's refusal
template <class F> static inline int mv_with_trace_net(const MvsdfNetDesc* d, int engine, F&& f) {
    int rc;
    switch (engine) {
        case MV_ENG_BS2: { MvNetBs<2> n; return (rc = mv_make_net_bs(d, &n, 2)) ? rc : f(n); }
        case MV_ENG_BS3: { MvNetBs<3> n; return (rc = mv_make_net_bs(d, &n, 3)) ? rc : f(n); }
        case MV_ENG_X3: { MvNetBs<3, 3> n; return (rc = mv_make_net_bs(d, &n, 3)) ? rc : f(n); }
        default: { MvNet n; return (rc = mv_make_net_trace(d, &n)) ? rc : f(n); }
    }
}
