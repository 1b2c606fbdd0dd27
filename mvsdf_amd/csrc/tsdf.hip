// tsdf.hip -- on-device TSDF fusion of depth maps into a voxel grid, and marching cubes under a validity mask.  Python: mvsdf_amd/tsdf.py, which states
// the integration's definition, and mesh.marching_cubes_masked (conventions: mvsdf_amd/mesh.py); tests/tsdf_ref.py restates both in numpy.
//
// * k_ts_integrate: a gather.  One lane owns one lattice point and visits the views in order with two fp64 accumulators' worth of state (the sum, and
//   the count as an int), so there are no float atomics and the result cannot depend on the schedule.  A workgroup is a brick of 4 x 8 x 8 lattice
//   points with k fastest: a wave's 64 points (one 8 x 8 slab in j, k) project to a compact patch of every depth map.  The 4x4 matrices P_v and the
//   view list are kernel data indexed by the loop counter alone, the same for every lane, so they come through the scalar cache; the four texels are
//   plain gathers.  One pass writes tsdf, weight and valid.  All arithmetic is fp64 without contraction, in the order the definition writes it.
// * k_mcm_*: the dense extractor's passes (mesh_kernels.hip) under a per-point validity mask, with mesh_common.h's table, ranks and scan.  A first pass
//   marks the valid cells (all 8 corners valid); the count pass keeps every point's crossing edges that touch a valid cell (one byte per point), which
//   the vertex and the face pass read back, so the three passes cannot disagree about what carries a vertex.
//
// Every argument of the integration is validated on the host before anything is launched: an error leaves {0, error bits} in the header.
#include "mesh_common.h"

#define TS_HDR 256                                    // bytes at the start of the integration workspace: int64 {0, error bits}
#define TS_BI 4                                       // the brick: TS_BI x TS_BJ x TS_BK lattice points, one per lane, k fastest
#define TS_BJ 8
#define TS_BK 8
#define TS_THREADS (TS_BI * TS_BJ * TS_BK)
static_assert(TS_BJ * TS_BK == 64, "a wave owns one j-k slab of the brick");

enum {
    TS_ERR_FINITE = 1,      // a non-finite matrix entry, origin, voxel, trunc, or a NaN jump
    TS_ERR_VIEW = 2,        // a view index outside [0, V)
    TS_ERR_RANGE = 4,       // voxel <= 0, trunc <= 0, jump < 0, min_views < 1
    TS_ERR_SHAPE = 8,       // V < 1, H or W < 2, a dim below 2, no views, sizes beyond the limits
};

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
    const double wmax = (double)(g.W - 1), hmax = (double)(g.H - 1);
    const long long hw = (long long)g.H * g.W;
    double D = 0.0;
    int n = 0;
    for (int q = 0; q < g.nviews; ++q) {
        const double* __restrict__ P = mats + (long long)q * 16;
        const double z = mv_row4(P + 8, p0, p1, p2, 1.0);
        if (!(z > 0.0)) continue;
        const double u = mv_row4(P, p0, p1, p2, 1.0) / z - 0.5;
        const double v = mv_row4(P + 4, p0, p1, p2, 1.0) / z - 0.5;
        if (!(u >= 0.0 && u <= wmax && v >= 0.0 && v <= hmax)) continue;
        const double x0 = fmin(floor(u), (double)(g.W - 2)), y0 = fmin(floor(v), (double)(g.H - 2));
        const double fx = u - x0, fy = v - y0;
        const float* __restrict__ tx = depths + (long long)views[q] * hw + (long long)(int)y0 * g.W + (int)x0;
        const double d00 = (double)tx[0], d01 = (double)tx[1], d10 = (double)tx[g.W], d11 = (double)tx[g.W + 1];
        if (!(ts_depth_ok(d00) && ts_depth_ok(d01) && ts_depth_ok(d10) && ts_depth_ok(d11))) continue;
        const double mx = fmax(fmax(d00, d01), fmax(d10, d11)), mn = fmin(fmin(d00, d01), fmin(d10, d11));
        if (mx - mn > g.jump) continue;
        const double ds = (d00 * (1.0 - fx) + d01 * fx) * (1.0 - fy) + (d10 * (1.0 - fx) + d11 * fx) * fy;
        const double s = ds - z;
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

// ================================================================ marching cubes under a validity mask ================================================================
struct McmVol {
    const float* p;
    const unsigned char* ok;                          // valid[i][j][k], contiguous
    long long n[3], s[3];                             // extents and element strides of vol[i, j, k]
    float level;
};

struct McmVal {
    const McmVol& v;
    __device__ __forceinline__ float operator()(long long i, long long j, long long k) const { return v.p[i * v.s[0] + j * v.s[1] + k * v.s[2]]; }
};

__device__ __forceinline__ long long mcm_at(const McmVol& v, long long i, long long j, long long k) { return (i * v.n[1] + j) * v.n[2] + k; }

__device__ __forceinline__ void mcm_ijk(const McmVol& v, long long p, long long* g) {
    const long long nyz = v.n[1] * v.n[2];
    g[0] = p / nyz;
    const long long r = p - g[0] * nyz;
    g[1] = r / v.n[2];
    g[2] = r - g[1] * v.n[2];
}

// pass 0: cell[p] = the cell with lower corner p exists and its 8 corners are valid
__global__ __launch_bounds__(MESH_THREADS) void k_mcm_cells(McmVol v, long long npts, unsigned char* __restrict__ cell) {
    const long long p = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
    if (p >= npts) return;
    long long g[3];
    mcm_ijk(v, p, g);
    bool ok = g[0] + 1 < v.n[0] && g[1] + 1 < v.n[1] && g[2] + 1 < v.n[2];
    if (ok) {
#pragma unroll
        for (int c = 0; c < 8; ++c) ok = ok && v.ok[mcm_at(v, g[0] + (c & 1), g[1] + (c >> 1 & 1), g[2] + (c >> 2 & 1))];
    }
    cell[p] = ok ? 1 : 0;
}

// bit a: one of the up to four cells around the grid edge (g, g + e_a) is valid (then both of its ends are)
__device__ __forceinline__ int mcm_edge_cells(const McmVol& v, const unsigned char* __restrict__ cell, const long long* g) {
    int bits = 0;
    for (int a = 0; a < 3; ++a) {
        const int o0 = a == 0 ? 1 : 0, o1 = a == 2 ? 1 : 2;
        bool any = false;
        for (int m = 0; m < 4; ++m) {
            long long q[3] = {g[0], g[1], g[2]};
            q[o0] -= m & 1;
            q[o1] -= m >> 1;
            if (q[o0] >= 0 && q[o1] >= 0) any = any || cell[mcm_at(v, q[0], q[1], q[2])];
        }
        if (any) bits |= 1 << a;
    }
    return bits;
}

// pass 1: per point, the crossing edges it owns that touch a valid cell (ebits), and the triangles of its cell when that is valid -> per-workgroup
// totals bv / bf, bf = -1 when the workgroup saw a non-finite VALID value
__global__ __launch_bounds__(MESH_THREADS) void k_mcm_count(McmVol v, long long npts, const unsigned char* __restrict__ cell, unsigned char* __restrict__ ebits,
                                                            int* __restrict__ bv, int* __restrict__ bf) {
    __shared__ int s_w[MESH_THREADS / 64];
    long long rv = 0, rf = 0;
    int bad = 0;
    for (int r = 0; r < MESH_ROUNDS; ++r) {
        const long long p = (long long)blockIdx.x * MESH_CHUNK + r * MESH_THREADS + threadIdx.x;
        int bits = 0, nt = 0;
        if (p < npts) {
            long long g[3];
            mcm_ijk(v, p, g);
            if (v.ok[p]) {
                const float x = McmVal{v}(g[0], g[1], g[2]);
                bad |= !isfinite(x);
                const int around = mcm_edge_cells(v, cell, g);
                if (around) bits = mc_point_edges(McmVal{v}, v.n, g[0], g[1], g[2], x < v.level, v.level) & around;
                if (cell[p]) nt = mc_ntri(mc_cube_index(McmVal{v}, g[0], g[1], g[2], v.level));
            }
            ebits[p] = (unsigned char)bits;
        }
        block_excl(__popc(bits), 2, s_w, rv);
        block_excl(nt, 3, s_w, rf);
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        bv[blockIdx.x] = (int)rv;
        bf[blockIdx.x] = bad ? -1 : (int)rf;
    }
}

// gradient component c at the valid grid point g from its neighbours g -+ e_c that are in the grid and valid: both -> central difference over 2h, one ->
// one-sided over h, none -> 0 (with every point valid: mc_grad_c)
__device__ __forceinline__ float mcm_grad_c(const McmVol& v, const long long* g, int c, float h) {
    long long lo[3] = {g[0], g[1], g[2]}, hi[3] = {g[0], g[1], g[2]};
    lo[c] -= 1;
    hi[c] += 1;
    const bool has_lo = lo[c] >= 0 && v.ok[mcm_at(v, lo[0], lo[1], lo[2])];
    const bool has_hi = hi[c] < v.n[c] && v.ok[mcm_at(v, hi[0], hi[1], hi[2])];
    if (!has_lo && !has_hi) return 0.0f;
    if (!has_lo) lo[c] = g[c];
    if (!has_hi) hi[c] = g[c];
    const float den = has_lo && has_hi ? 2.0f * h : h;
    const McmVal val{v};
    return (val(hi[0], hi[1], hi[2]) - val(lo[0], lo[1], lo[2])) / den;
}

// mc_vertex with the masked gradient: the vertex on the crossing edge (g, g + e_a), x = the value at g
__device__ __forceinline__ void mcm_vertex(const McmVol& v, const long long* g, int a, float x, const McGeom& gm, float* vert, float* normal) {
    long long g1[3] = {g[0], g[1], g[2]};
    g1[a] += 1;
    const float x1 = McmVal{v}(g1[0], g1[1], g1[2]);
    const float t = (v.level - x) / (x1 - x);
    float nr[3];
    for (int c = 0; c < 3; ++c) {
        vert[c] = c == a ? gm.org[c] + ((float)g[c] + t) * gm.sp[c] : gm.org[c] + (float)g[c] * gm.sp[c];
        const float d0 = mcm_grad_c(v, g, c, gm.sp[c]), d1 = mcm_grad_c(v, g1, c, gm.sp[c]);
        nr[c] = d0 + t * (d1 - d0);
    }
    const float nn = sqrtf((nr[0] * nr[0] + nr[1] * nr[1]) + nr[2] * nr[2]);
    for (int c = 0; c < 3; ++c) normal[c] = nn > 0.0f ? nr[c] / nn : 0.0f;
}

// pass 2: the vertex id map (id of each point's first vertex), vertices and normals
__global__ __launch_bounds__(MESH_THREADS) void k_mcm_vertices(McmVol v, long long npts, McGeom gm, const unsigned char* __restrict__ ebits,
                                                               const long long* __restrict__ ov, int* __restrict__ idmap, float* __restrict__ verts,
                                                               float* __restrict__ normals, long long nv_cap) {
    __shared__ int s_w[MESH_THREADS / 64];
    long long run = ov[blockIdx.x];
    for (int r = 0; r < MESH_ROUNDS; ++r) {
        const long long p = (long long)blockIdx.x * MESH_CHUNK + r * MESH_THREADS + threadIdx.x;
        const int bits = p < npts ? ebits[p] : 0;
        long long id = block_excl(__popc(bits), 2, s_w, run);
        if (p >= npts) continue;
        idmap[p] = (int)id;
        if (!bits) continue;
        long long g[3];
        mcm_ijk(v, p, g);
        const float x = McmVal{v}(g[0], g[1], g[2]);
        for (int a = 0; a < 3; ++a) {
            if (!(bits >> a & 1)) continue;
            if (id < nv_cap) mcm_vertex(v, g, a, x, gm, verts + id * 3, normals + id * 3);
            ++id;
        }
    }
}

// pass 3: faces of the valid cells in linear order, each cell's triangles in table order
__global__ __launch_bounds__(MESH_THREADS) void k_mcm_faces(McmVol v, long long npts, const unsigned char* __restrict__ cell, const unsigned char* __restrict__ ebits,
                                                            const long long* __restrict__ of, const int* __restrict__ idmap, int* __restrict__ faces,
                                                            long long nf_cap) {
    __shared__ int s_w[MESH_THREADS / 64];
    long long run = of[blockIdx.x];
    for (int r = 0; r < MESH_ROUNDS; ++r) {
        const long long p = (long long)blockIdx.x * MESH_CHUNK + r * MESH_THREADS + threadIdx.x;
        long long g[3] = {0, 0, 0};
        int ci = 0, nt = 0;
        if (p < npts && cell[p]) {
            mcm_ijk(v, p, g);
            ci = mc_cube_index(McmVal{v}, g[0], g[1], g[2], v.level);
            nt = mc_ntri(ci);
        }
        const long long fid = block_excl(nt, 3, s_w, run);
        for (int t = 0; t < nt; ++t) {
            if (fid + t >= nf_cap) break;
            const int base = (mc_tri_offset[ci] + t) * 3;
            for (int s = 0; s < 3; ++s) {
                long long q[3] = {g[0], g[1], g[2]};
                const int a = mc_edge_owner(mc_tri_edges[base + s], q);
                const long long o = mcm_at(v, q[0], q[1], q[2]);
                faces[(fid + t) * 3 + s] = idmap[o] + __popc(ebits[o] & ((1 << a) - 1));
            }
        }
    }
}

struct McmLayout {
    long long npts, nb;
    size_t idmap, cell, ebits, bv, bf, ov, of, total;
};

static bool mcm_layout(long long nx, long long ny, long long nz, McmLayout* L) {
    if (nx < 2 || ny < 2 || nz < 2) return false;
    const long long lim = 1ll << 40;
    if (nx > lim / ny || nx * ny > lim / nz) return false;
    L->npts = nx * ny * nz;
    L->nb = mv_ceil_div(L->npts, MESH_CHUNK);
    if (L->nb > INT_MAX || mv_ceil_div(L->npts, MESH_THREADS) > INT_MAX) return false;
    WsCursor c{MESH_HDR};
    L->idmap = c.take((size_t)L->npts * 4);
    L->cell = c.take((size_t)L->npts);
    L->ebits = c.take((size_t)L->npts);
    L->bv = c.take((size_t)L->nb * 4);
    L->bf = c.take((size_t)L->nb * 4);
    L->ov = c.take((size_t)L->nb * 8);
    L->of = c.take((size_t)L->nb * 8);
    L->total = c.o;
    return true;
}

static bool mcm_vol(const float* vol, const uint8_t* valid, const int64_t* shape, const int64_t* strides, float level, McmLayout* L, McmVol* v) {
    if (!vol || !valid || !shape || !strides || !mcm_layout(shape[0], shape[1], shape[2], L)) return false;
    v->p = vol;
    v->ok = valid;
    v->level = level;
    for (int a = 0; a < 3; ++a) {
        v->n[a] = shape[a];
        v->s[a] = strides[a];
    }
    return true;
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
    if (!ts_layout(V, H, W, nviews, dims, &L)) err |= TS_ERR_SHAPE;
    if (!(err & TS_ERR_SHAPE)) {
        for (long long q = 0; q < nviews; ++q)
            if (views[q] < 0 || views[q] >= V) err |= TS_ERR_VIEW;
        for (long long q = 0; q < nviews * 16; ++q)
            if (!isfinite(mats[q])) err |= TS_ERR_FINITE;
    }
    if (!isfinite(origin[0]) || !isfinite(origin[1]) || !isfinite(origin[2]) || !isfinite(voxel) || !isfinite(trunc) || isnan(jump)) err |= TS_ERR_FINITE;
    if (!(err & TS_ERR_FINITE) && (!(voxel > 0.0) || !(trunc > 0.0) || !(jump >= 0.0))) err |= TS_ERR_RANGE;
    if (min_views < 1) err |= TS_ERR_RANGE;
    if (err) {
        const long long hdr[2] = {0, err};
        return mv_write_header(ws, hdr, 2, s, what);
    }
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

size_t mvsdf_mcm_workspace_bytes(int64_t nx, int64_t ny, int64_t nz) {
    McmLayout L;
    return mcm_layout(nx, ny, nz, &L) ? L.total : 0;
}

int mvsdf_mcm_count(const float* vol, const uint8_t* valid, const int64_t* shape, const int64_t* strides, float level, void* ws, size_t ws_bytes, void* stream) {
    McmLayout L;
    McmVol v;
    if (!mcm_vol(vol, valid, shape, strides, level, &L, &v) || !ws) return mv_fail(-1, "mvsdf_mcm_count: bad arguments (every extent must be >= 2)");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_mcm_count: workspace too small (mvsdf_mcm_workspace_bytes)");
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mcm_cells, dim3(mv_grid(L.npts, MESH_THREADS)), dim3(MESH_THREADS), 0, s, v, L.npts, (unsigned char*)(w + L.cell));
    hipLaunchKernelGGL(k_mcm_count, dim3((unsigned)L.nb), dim3(MESH_THREADS), 0, s, v, L.npts, (const unsigned char*)(w + L.cell), (unsigned char*)(w + L.ebits),
                       (int*)(w + L.bv), (int*)(w + L.bf));
    hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(MESH_SCAN_THREADS), 0, s, (const int*)(w + L.bv), (const int*)(w + L.bf), (int)L.nb,
                       (long long*)(w + L.ov), (long long*)(w + L.of), (long long*)w);
    return mv_check(hipGetLastError(), "mvsdf_mcm_count");
}

int mvsdf_mcm_emit(const float* vol, const uint8_t* valid, const int64_t* shape, const int64_t* strides, float level, const float* spacing, const float* origin,
                   void* ws, size_t ws_bytes, float* verts, float* normals, int32_t* faces, int64_t nv_cap, int64_t nf_cap, void* stream) {
    McmLayout L;
    McmVol v;
    if (!mcm_vol(vol, valid, shape, strides, level, &L, &v) || !ws || !spacing || !origin || nv_cap < 0 || nf_cap < 0 || (nv_cap && (!verts || !normals)) ||
        (nf_cap && !faces))
        return mv_fail(-1, "mvsdf_mcm_emit: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_mcm_emit: workspace too small (mvsdf_mcm_workspace_bytes)");
    McGeom gm;
    for (int a = 0; a < 3; ++a) {
        gm.sp[a] = spacing[a];
        gm.org[a] = origin[a];
    }
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mcm_vertices, dim3((unsigned)L.nb), dim3(MESH_THREADS), 0, s, v, L.npts, gm, (const unsigned char*)(w + L.ebits),
                       (const long long*)(w + L.ov), (int*)(w + L.idmap), verts, normals, (long long)nv_cap);
    hipLaunchKernelGGL(k_mcm_faces, dim3((unsigned)L.nb), dim3(MESH_THREADS), 0, s, v, L.npts, (const unsigned char*)(w + L.cell),
                       (const unsigned char*)(w + L.ebits), (const long long*)(w + L.of), (const int*)(w + L.idmap), faces, (long long)nf_cap);
    return mv_check(hipGetLastError(), "mvsdf_mcm_emit");
}

}  // extern "C"
