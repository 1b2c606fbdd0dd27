// tsdf.hip -- on-device TSDF fusion of depth maps into a voxel grid.  Python: mvsdf_amd/tsdf.py, which states the integration's definition;
// tests/tsdf_ref.py restates it in numpy.  The volume is meshed by mesh.marching_cubes_masked (mesh_kernels.hip: the extraction passes under McMask).
//
// * k_ts_integrate: a gather.  One lane owns one lattice point and visits the views in order with two fp64 accumulators' worth of state (the sum, and
//   the count as an int), so there are no float atomics and the result cannot depend on the schedule.  A workgroup is a brick of 4 x 8 x 8 lattice
//   points with k fastest: a wave's 64 points (one 8 x 8 slab in j, k) project to a compact patch of every depth map.  The 4x4 matrices P_v and the
//   view list are kernel data indexed by the loop counter alone, the same for every lane, so they come through the scalar cache; the four texels are
//   plain gathers.  The projection and the 2x2 sample are view_prims.h's mv_project_texel / mv_cell2, the ones fusion.hip's k_fu_fuse uses: the depth
//   maps this reads are the ones that writes.  One pass writes tsdf, weight and valid.  All arithmetic is fp64 without contraction, in the order the
//   definition writes it.
//
// Every argument of the integration is validated on the host before anything is launched: an error leaves {0, error bits} in the header.
#include "view_prims.h"

#define TS_HDR 256                                    // bytes at the start of the integration workspace: MVSDF_RES_H_*
static_assert(MVSDF_RES_H_WORDS * 8 <= TS_HDR, "the result words fit the header");
#define TS_BI 4                                       // the brick: TS_BI x TS_BJ x TS_BK lattice points, one per lane, k fastest
#define TS_BJ 8
#define TS_BK 8
#define TS_THREADS (TS_BI * TS_BJ * TS_BK)
static_assert(TS_BJ * TS_BK == 64, "a wave owns one j-k slab of the brick");

struct TsLayout {
    size_t mats, views, total;
    long long npts, bricks[3], nbricks;
};

static bool ts_layout(long long V, long long H, long long W, long long nviews, const int64_t* dims, TsLayout* L) {
    if (V < 1 || H < 2 || W < 2 || V > INT_MAX || H > INT_MAX || W > INT_MAX || H * W > INT_MAX || nviews < 1 || nviews > INT_MAX) return false;
    if (dims) {
        for (int a = 0; a < 3; ++a)
            if (dims[a] < 2 || dims[a] > INT_MAX) return false;
        const long long lim = 1ll << 40;
        if (dims[0] > lim / dims[1] || dims[0] * dims[1] > lim / dims[2]) return false;
        L->npts = dims[0] * dims[1] * dims[2];
        L->bricks[0] = mv_ceil_div(dims[0], TS_BI);
        L->bricks[1] = mv_ceil_div(dims[1], TS_BJ);
        L->bricks[2] = mv_ceil_div(dims[2], TS_BK);
        L->nbricks = L->bricks[0] * L->bricks[1] * L->bricks[2];
        if (L->nbricks > INT_MAX) return false;
    }
    WsCursor c{TS_HDR};
    L->mats = c.take((size_t)nviews * 16 * 8);
    L->views = c.take((size_t)nviews * 4);
    L->total = c.o;
    return true;
}

struct TsGrid {
    double org[3], h, trunc, jump;
    int n[3], by, bz;                                 // extents; bricks along j and k
    int H, W, nviews, min_views;
};

// a texel holds a depth iff it is finite and > 0
__device__ __forceinline__ bool ts_depth_ok(double d) { return d > 0.0 && d < (double)INFINITY; }

__global__ __launch_bounds__(TS_THREADS) void k_ts_integrate(const float* __restrict__ depths, const double* __restrict__ mats, const int* __restrict__ views,
                                                              TsGrid g, float* __restrict__ tsdf, int* __restrict__ weight, unsigned char* __restrict__ valid) {
    const int b = blockIdx.x;
    const int bk = b % g.bz, bj = (b / g.bz) % g.by, bi = b / (g.bz * g.by);
    const int t = threadIdx.x;
    const int i = bi * TS_BI + t / (TS_BJ * TS_BK), j = bj * TS_BJ + (t / TS_BK) % TS_BJ, k = bk * TS_BK + t % TS_BK;
    if (i >= g.n[0] || j >= g.n[1] || k >= g.n[2]) return;
    const double p0 = g.org[0] + (double)i * g.h, p1 = g.org[1] + (double)j * g.h, p2 = g.org[2] + (double)k * g.h;
    const long long hw = (long long)g.H * g.W;
    double D = 0.0;
    int n = 0;
    for (int q = 0; q < g.nviews; ++q) {
        MvProj pr;
        if (!mv_project_texel(mats + (long long)q * 16, p0, p1, p2, g.W, g.H, &pr)) continue;
        const MvCell2 c = mv_cell2(depths + (long long)views[q] * hw, g.W, g.H, pr.u, pr.v);
        if (!(ts_depth_ok(c.d00) && ts_depth_ok(c.d01) && ts_depth_ok(c.d10) && ts_depth_ok(c.d11))) continue;
        const double mx = fmax(fmax(c.d00, c.d01), fmax(c.d10, c.d11)), mn = fmin(fmin(c.d00, c.d01), fmin(c.d10, c.d11));
        if (mx - mn > g.jump) continue;
        const double s = c.bilinear() - pr.z;
        if (s < -g.trunc) continue;
        D += fmin(s / g.trunc, 1.0);
        ++n;
    }
    const long long at = ((long long)i * g.n[1] + j) * g.n[2] + k;
    const bool ok = n >= g.min_views;
    weight[at] = n;
    tsdf[at] = ok ? (float)(D / (double)n) : 1.0f;
    valid[at] = ok ? 1 : 0;
}

extern "C" {

size_t mvsdf_tsdf_workspace_bytes(int64_t V, int64_t H, int64_t W, int64_t nviews) {
    TsLayout L;
    return ts_layout(V, H, W, nviews, nullptr, &L) ? L.total : 0;
}

int mvsdf_tsdf_integrate(const float* depths, int64_t V, int64_t H, int64_t W, const double* mats, const int32_t* views, int64_t nviews, const double* origin,
                         double voxel, const int64_t* dims, double trunc, double jump, int32_t min_views, void* ws, size_t ws_bytes, float* tsdf,
                         int32_t* weight, uint8_t* valid, void* stream) {
    const char* what = "mvsdf_tsdf_integrate";
    if (!depths || !mats || !views || !origin || !dims || !ws || !tsdf || !weight || !valid || ws_bytes < TS_HDR)
        return mv_fail(-1, "mvsdf_tsdf_integrate: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    // ---- validation, all of it before the first launch ----
    long long err = 0;
    TsLayout L;
    if (!ts_layout(V, H, W, nviews, dims, &L)) err |= MVSDF_TS_ERR_SHAPE;
    if (!(err & MVSDF_TS_ERR_SHAPE)) {
        for (long long q = 0; q < nviews; ++q)
            if (views[q] < 0 || views[q] >= V) err |= MVSDF_TS_ERR_VIEW;
        if (!mv_all_finite(mats, nviews * 16)) err |= MVSDF_TS_ERR_FINITE;
    }
    if (!isfinite(origin[0]) || !isfinite(origin[1]) || !isfinite(origin[2]) || !isfinite(voxel) || !isfinite(trunc) || isnan(jump)) err |= MVSDF_TS_ERR_FINITE;
    if (!(err & MVSDF_TS_ERR_FINITE) && (!(voxel > 0.0) || !(trunc > 0.0) || !(jump >= 0.0))) err |= MVSDF_TS_ERR_RANGE;
    if (min_views < 1) err |= MVSDF_TS_ERR_RANGE;
    if (err) return mv_refuse_header(ws, err, s, what);
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_tsdf_integrate: workspace too small (mvsdf_tsdf_workspace_bytes)");
    // ---- uploads and the launch ----
    char* w = (char*)ws;
    int rc;
    if ((rc = mv_check(hipMemsetAsync(ws, 0, TS_HDR, s), what))) return rc;
    if ((rc = mv_check(hipMemcpyAsync(w + L.mats, mats, (size_t)nviews * 16 * 8, hipMemcpyHostToDevice, s), what))) return rc;
    if ((rc = mv_check(hipMemcpyAsync(w + L.views, views, (size_t)nviews * 4, hipMemcpyHostToDevice, s), what))) return rc;
    TsGrid g;
    for (int a = 0; a < 3; ++a) {
        g.org[a] = origin[a];
        g.n[a] = (int)dims[a];
    }
    g.h = voxel;
    g.trunc = trunc;
    g.jump = jump;
    g.by = (int)L.bricks[1];
    g.bz = (int)L.bricks[2];
    g.H = (int)H;
    g.W = (int)W;
    g.nviews = (int)nviews;
    g.min_views = min_views;
    hipLaunchKernelGGL(k_ts_integrate, dim3((unsigned)L.nbricks), dim3(TS_THREADS), 0, s, depths, (const double*)(w + L.mats), (const int*)(w + L.views), g,
                       tsdf, weight, valid);
    return mv_check(hipGetLastError(), what);                   // no wait here: the caller keeps the host arrays until it has read the header
}

}  // extern "C"
