// fork_rule.cpp -- prints the rule, the grid and the LDS bytes of the sixteen-wave rows form (mvsdf_amd/csrc/trace_route.h: mv_rows16_on, mv_rows16_grid,
// mv_rows16_lds_bytes) for tests/test_trace_fork_rule_host.py.  The header has no HIP in it: this program includes it alone and builds with the host compiler.
#include <stdio.h>
#include "trace_route.h"

int main() {
    const int maxnts[] = {4, 16, 17, 32}, Rs[] = {1, 1024, 1025, 2048, 2049}, cus[] = {256, 64}, mts[] = {1, 2};
    for (int e = 0; e < 4; ++e) for (int nt : maxnts) for (int R : Rs) for (int mt : mts) for (int cu : cus)
        printf("rule %d %d %d %d %d : %d %d\n", e, nt, R, mt, cu, (int)mv_rows16_on(e, nt, R, mt, cu), (int)mv_sphere_cut_on(e, R, mt, cu));
    const int per[] = {12, 100}, caps[] = {0, 1, 2, 300};
    for (int R : Rs) for (int p : per) for (int cu : cus) for (int cap : caps)
        printf("grid %d %d %d %d : %d %d\n", R, p, cu, cap, mv_rows16_grid(R, p, cu, cap), mv_row_blocks(R, p, 2));
    const int nets[][2] = {{72, 0}, {104, 6}, {264, 0}, {296, 6}};   // {S, multires}
    for (auto& n : nets) printf("lds %d %d : %zu %zu\n", n[0], n[1], mv_rows16_lds_bytes(n[0], n[1]), mv_trace_lds_bytes(n[0], n[1], 2, 64));
    printf("uses %d\n", mv_rows16_uses());
    return 0;
}
