// Prints what the tracer launches (mvsdf_amd/csrc/trace_route.h, host C++ only) over the cross product that tests/test_trace_route_host.py holds to
// tests/golden/trace_routes.txt.xz: one line per (switch, engine, maxnt, mt = mt_samples, R, training, steps given, n_steps, compute units), then the
// workspace layouts.  Columns (tests/test_trace_route_host.py::COLUMNS): the instance <mt.ntw.nw> of the sphere kernel, of the sample-row parts 1 / 2 / 4 / 8 and
// of mvsdf_sdf_col0 (<mt.ntw.nw.xr>; r<code>: refused); then, unless the tracer refuses the network, tail filling on, stop_left, nf, the grids (sphere,
// first window, rest, part 2 = secant + min-sdf, part 4 = min-sdf alone, secant, reduction) and the dynamic LDS bytes at S = 68 and 260 (multires 6) of the
// sphere and part-2 instances with 16 * mt and 32 * mt activation rows and of col0.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "trace_route.h"

static const char* env_of(const char* name) { return getenv(name); }
// the switches with the one variable "NAME=value" set ("": none)
static MvTraceSwitches with_env(const char* var) {
    char name[64];
    const char* eq = strchr(var, '=');
    if (eq) { snprintf(name, sizeof name, "%.*s", (int)(eq - var), var); setenv(name, eq + 1, 1); }
    const MvTraceSwitches sw = mv_trace_switches_from_env(env_of, env_of);
    if (eq) unsetenv(name);
    return sw;
}
static void put(const MvInst& r, bool col0 = false) {
    if (r.rc) printf(" r%d", r.rc);
    else if (col0) printf(" %d.%d.%d.%d", r.mt, r.ntw, r.nw, r.xr);
    else printf(" %d.%d.%d", r.mt, r.ntw, r.nw);
}

int main() {
    static const char* names[] = {"none", "tail=0", "tail=2", "tail_stop=0", "nfirst=1", "nfirst=100", "nfirst=200", "mt_first=2", "bf_carry=1"};
    static const char* vars[] = {"", "MVSDF_TAIL=0", "MVSDF_TAIL=2", "MVSDF_TAIL_STOP=0", "MVSDF_NFIRST=1", "MVSDF_NFIRST=100", "MVSDF_NFIRST=200", "MVSDF_MT_FIRST=2",
                                 "MVSDF_BF_CARRY=1"};
    const int maxnts[] = {4, 15, 16, 17, 32, 33}, mts[] = {0, 1, 2, 3, 4, 49}, n_stepss[] = {2, 12, 13, 100}, cuss[] = {256, 64};
    for (int k = 0; k < 9; ++k) {
        const MvTraceSwitches sw = with_env(vars[k]);
        for (int eng = MV_ENG_F32; eng <= MV_ENG_X3; ++eng) for (int maxnt : maxnts) for (int mt : mts) {
            const MvInst s1 = mv_route_sphere(eng, maxnt, mt), p2 = mv_route_samples(eng, maxnt, mt, 1, 2, sw);
            const int mt1 = s1.rc ? 1 : s1.mt;
            const int Rs[] = {1, 17, 2048, 2049, 4096, 4097, 8192, 8193, 256 * 8 * mt1 - 1, 256 * 8 * mt1 + 1};   // the last two: the tail bound at 256 compute units
            for (int R : Rs) for (int tr = 0; tr < 2; ++tr) for (int st = 0; st < 2; ++st) for (int n : n_stepss) for (int cus : cuss) {
                printf("%s %d %d %d %d %d %d %d %d :", names[k], eng, maxnt, mt, R, tr, st, n, cus);
                const MvInst p1 = mv_route_samples(eng, maxnt, mt, R, 1, sw);
                put(s1); put(p1); put(mv_route_samples(eng, maxnt, mt, R, 2, sw)); put(mv_route_samples(eng, maxnt, mt, R, 4, sw));
                put(mv_route_samples(eng, maxnt, mt, R, 8, sw)); put(mv_route_col0(eng, maxnt, mt, sw), true);
                if (!s1.rc) {
                    const bool tail = mv_tail_on(eng, tr, st != 0, R, s1.mt, cus, sw);
                    const int nf = mv_first_window(n, sw);
                    const MvSampleGrids g1 = mv_sample_grids(R, n, nf, p1.mt, tr, tail, 16), g2 = mv_sample_grids(R, n, nf, p2.mt, tr, tail, 16);
                    printf(" %d %d %d %d %d %d %d %d %d %d", tail ? 1 : 0, mv_tail_stop_left(R, s1.mt, sw), nf, mv_sphere_grid(R, s1.mt), g1.first, g1.rest,
                           g2.sec + g2.minsdf, g2.minsdf, g2.sec, g2.red);
                    for (int S = 68; S <= 260; S += 192)
                        printf(" %zu %zu %zu %zu %zu", mv_trace_lds_bytes(S, 6, s1.mt, 16 * s1.mt), mv_trace_lds_bytes(S, 6, s1.mt, 32 * s1.mt),
                               mv_trace_lds_bytes(S, 6, p2.mt, 16 * p2.mt), mv_trace_lds_bytes(S, 6, p2.mt, 32 * p2.mt), mv_col0_lds_bytes(S, 6, p2.mt));
                }
                printf("\n");
            }
        }
    }
    const int shapes[][2] = {{1, 2}, {17, 100}, {2048, 128}, {8193, 1024}, {0, 100}, {-5, 100}, {17, 0}, {17, -3}};
    for (const auto& s : shapes) {
        const MvTraceWs w = mv_trace_ws(s[0], s[1]);
        printf("ws %d %d : %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", s[0], s[1], w.w_zmin, w.w_zmax, w.sec_state, w.w_list, w.w_list_min, w.sec_list, w.sv,
               w.list_rest, w.src_rest, w.sv_min, w.total);
    }
    return 0;
}
