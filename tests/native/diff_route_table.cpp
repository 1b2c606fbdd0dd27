// Prints the route of every differentiable-MLP pass (mvsdf_amd/csrc/diff_route.h, host C++ only) over the cross product that
// tests/test_diff_route_host.py holds to tests/golden/diff_routes.txt: one line per (switch, net width class, 16-row tiles, x3 packs, option).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "diff_route.h"

static void put(const char* pass, const MvRoute& r) {
    static const char* fam[] = {"refuse", "layers", "split", "f32", "x3", "scale"};
    if (r.family == MV_FAM_REFUSE) printf(" %s=refuse(%d)", pass, r.rc);
    else printf(" %s=%s<%d,%d,%d,%d>", pass, fam[r.family], r.mt, r.ntw, r.nw, r.pd);
}

static const char* env_of(const char* name) { return getenv(name); }
// the switches with the one variable "NAME=value" set ("": none)
static MvDevSwitches with_env(const char* var) {
    char name[64];
    const char* eq = strchr(var, '=');
    if (eq) { snprintf(name, sizeof name, "%.*s", (int)(eq - var), var); setenv(name, eq + 1, 1); }
    const MvDevSwitches sw = mv_switches_from_env(env_of);
    if (eq) unsetenv(name);
    return sw;
}

int main() {
    // each switch alone, through the environment the library reads them from (MVSDF_CHAIN_W8=0: set, so the fp32 arithmetic, but 16 waves)
    static const char* names[] = {"none", "fuse=0", "split_chains=1", "chain_w8=1", "chain_mt=1", "chain_mt=2", "chain_x3=0", "delta_chain=1", "layer_mt=1", "wg_xcd=0", "chain_w8=0"};
    static const char* vars[] = {"", "MVSDF_FUSE=0", "MVSDF_SPLIT_CHAINS=1", "MVSDF_CHAIN_W8=1", "MVSDF_CHAIN_MT=1", "MVSDF_CHAIN_MT=2", "MVSDF_CHAIN_X3=0", "MVSDF_DELTA_CHAIN=1",
                                 "MVSDF_LAYER_MT=1", "MVSDF_WG_XCD=0", "MVSDF_CHAIN_W8=0"};
    const int ntws[] = {0, 2, 4}, tiles[] = {1, 256, 257, 512, 513};
    for (int k = 0; k < 11; ++k) {
        const MvDevSwitches sw = with_env(vars[k]);
        for (int ntw : ntws) for (int t : tiles) for (int x3 = 0; x3 < 2; ++x3) for (int opt = 0; opt < 2; ++opt) {   // opt: gather / sub-range / cnt / row indirection asked for
            printf("%s ntw=%d tiles=%d x3=%d opt=%d :", names[k], ntw, t, x3, opt);
            put("fwd", mv_route_sdf_forward(ntw, t, 1, x3, opt, sw));
            put("bwd", mv_route_sdf_backward(ntw, t, x3, false, sw));
            put("pair", mv_route_sdf_backward_pair(ntw, t, x3, sw));
            put("delta", mv_route_delta(ntw, t, opt, sw));
            put("rfwd", mv_route_render_forward(ntw, 1, sw));
            put("rbwd", mv_route_render_backward(ntw, 8 * ntw, opt, sw));
            printf(" layer_mt=%d xcd=%d defer=%d\n", mv_layer_mt(16 * t, sw), sw.wg_xcd, mv_route_can_defer(ntw, ntw, 8 * ntw, sw) ? 1 : 0);
        }
    }
    // the width limits of the chains and the several-skips refusal, product switches and the two that reach the refusal
    const MvDevSwitches sw = with_env(""), nofuse = with_env("MVSDF_FUSE=0"), split = with_env("MVSDF_SPLIT_CHAINS=1");
    for (int ntw = 2; ntw <= 4; ntw += 2) for (int over = 0; over < 2; ++over) for (int opt = 0; opt < 2; ++opt) {
        printf("edge ntw=%d over=%d opt=%d :", ntw, over, opt);
        put("fwd", mv_route_sdf_forward(ntw, 1, 32 * ntw + over, true, opt, sw));
        put("rfwd", mv_route_render_forward(ntw, 2 + over, sw));
        put("rbwd", mv_route_render_backward(ntw, 8 * ntw + over, opt, sw));
        printf(" defer=%d", mv_route_can_defer(ntw, ntw, 8 * ntw + over, sw) ? 1 : 0);
        put("bwd_skips", mv_route_sdf_backward(ntw, 1, true, true, sw));
        put("bwd_skips_fuse0", mv_route_sdf_backward(ntw, 1, true, true, nofuse));
        put("bwd_skips_split", mv_route_sdf_backward(ntw, 1, true, true, split));
        printf("\n");
    }
    return 0;
}
