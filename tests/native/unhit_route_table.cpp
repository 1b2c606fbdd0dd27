// Prints the route of the secant-only launch (mvsdf_amd/csrc/trace_route.h::mv_route_secant, host C++ only) beside the sphere route and the part-8 route it is
// built from: one line per (engine, maxnt, mt_samples, R) "eng maxnt mt R : secant sphere1 part8" with instances as <mt.ntw.nw> (r<code>: refused).
// tests/test_unhit_route_host.py reads it.
#include <stdio.h>
#include "trace_route.h"

static void put(const MvInst& r) {
    if (r.rc) printf(" r%d", r.rc);
    else printf(" %d.%d.%d", r.mt, r.ntw, r.nw);
}

int main() {
    const MvTraceSwitches sw;
    const int maxnts[] = {4, 15, 16, 17, 32, 33}, mts[] = {0, 1, 2, 3, 4, 49}, Rs[] = {1, 17, 2048, 2049, 4096, 4097, 8193};
    for (int eng = MV_ENG_F32; eng <= MV_ENG_X3; ++eng) for (int maxnt : maxnts) for (int mt : mts) for (int R : Rs) {
        printf("%d %d %d %d :", eng, maxnt, mt, R);
        put(mv_route_secant(eng, maxnt, mt, R, sw));
        put(mv_route_sphere(eng, maxnt, 1));
        put(mv_route_samples(eng, maxnt, mt, R, 8, sw));
        printf("\n");
    }
    return 0;
}
