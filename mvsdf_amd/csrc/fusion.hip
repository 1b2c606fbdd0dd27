// fusion.hip -- on-device depth-map fusion (the point-cloud fusion step of the reference's BYOD.md): probability mask, geometric consistency of every
// reference pixel against its source views, averaged depth, back-projection to one cloud.  Python: mvsdf_amd/fusion.py, which states the definition;
// tests/fusion_ref.py restates it in numpy.  All arithmetic is fp64 without contraction, in the order the definition writes it.
//
// * k_fu_mask: masked depth of every pixel (fp32 compares against the probability thresholds).
// * k_fu_fuse: one lane per reference pixel, the source loop inside.  The 4x4 transforms T_rs / T_sr are kernel data indexed by (view, source slot),
//   the same for every lane of a workgroup, so they come through the scalar cache; the four source texels are plain gathers (the projection and the
//   2x2 sample are view_prims.h's mv_project_texel / mv_cell2, which tsdf.hip's integration uses too; the way back is its mv_project).  Writes
//   counts, the fp32 fused depth, the fp64 fused depth (the emit pass back-projects at it) and a keep flag.
// * an int64 exclusive scan of the keep flags over all views (geom_prims.h: mv_scan_blocks, i.e. k_scan_block_sum and k_scan_top); the emit pass ranks
//   its own chunk (mv_chunk_rank), so no per-pixel offset is stored.  Points come out in (view, y, x) order.  No float atomics anywhere.
// * k_fu_normals (fusion.py: depth_normals): one lane per fused point; the tangents are differences of back-projected neighbour texels of the fused
//   depth map, never taken across a hole or a depth edge, their cross product is oriented towards the camera.
//
// Every argument is validated on the host before anything is launched: an error leaves {0, error bits} in the header and the device untouched.
#include "view_prims.h"

#define FU_THREADS 256
#define FU_HDR 256                                    // bytes at the start of the workspace: MVSDF_RES_H_*
static_assert(MVSDF_RES_H_WORDS * 8 <= FU_HDR, "the result words fit the header");
#define FU_MAX_PIXELS (1ll << 40)

struct FuLayout {
    size_t mats, pinv, src, off, df, keep, bsum, total;
    long long nb;
};

static bool fu_layout(long long V, long long H, long long W, long long npairs, FuLayout* L) {
    if (V < 1 || H < 2 || W < 2 || npairs < 0 || V > INT_MAX || H > INT_MAX || W > INT_MAX || H * W > INT_MAX || npairs > INT_MAX) return false;
    const long long n = V * H * W;
    if (n > FU_MAX_PIXELS || V * mv_ceil_div(H * W, FU_THREADS) > INT_MAX) return false;
    L->nb = mv_ceil_div(n, MV_CHUNK);
    WsCursor c{FU_HDR};
    L->mats = c.take((size_t)(npairs > 0 ? npairs : 1) * 32 * 8);
    L->pinv = c.take((size_t)V * 16 * 8);
    L->src = c.take((size_t)(npairs > 0 ? npairs : 1) * 4);
    L->off = c.take((size_t)(V + 1) * 4);
    L->df = c.take((size_t)n * 8);
    L->keep = c.take((size_t)n);
    L->bsum = c.take(mv_scan_tmp_bytes(n));
    L->total = c.o;
    return true;
}

// step 1
__global__ __launch_bounds__(FU_THREADS) void k_fu_mask(const float* __restrict__ depth, const float* __restrict__ prob, long long V, long long hw,
                                                         float t1, float t2, float t3, float* __restrict__ masked) {
    const long long i = (long long)blockIdx.x * FU_THREADS + threadIdx.x;
    if (i >= V * hw) return;
    const float d = depth[i];
    bool m = isfinite(d) && d > 0.0f;
    if (prob) {
        const long long v = i / hw, p = i - v * hw;
        const float* q = prob + v * 3 * hw + p;
        m = m && q[0] > t1 && q[hw] > t2 && q[2 * hw] > t3;
    }
    masked[i] = m ? d : 0.0f;
}

// steps 2 and 3.  Workgroup b: view b / tiles, pixels (b % tiles) * FU_THREADS ...
__global__ __launch_bounds__(FU_THREADS) void k_fu_fuse(const float* __restrict__ masked, int V, int H, int W, int tiles, const int* __restrict__ off,
                                                         const int* __restrict__ src, const double* __restrict__ mats, int vthresh, double pix2,
                                                         double dep_thresh, int* __restrict__ counts, float* __restrict__ fused,
                                                         double* __restrict__ dfo, unsigned char* __restrict__ keep) {
    const int r = blockIdx.x / tiles;
    const int hw = H * W;
    const int p = (blockIdx.x - r * tiles) * FU_THREADS + threadIdx.x;
    if (r >= V || p >= hw) return;
    const long long at = (long long)r * hw + p;
    const double d = (double)masked[at];
    int n = 0;
    double acc = d;
    if (d > 0.0) {
        const int y = p / W, x = p - y * W;
        const double X = (double)x + 0.5, Y = (double)y + 0.5;
        const double q0 = X * d, q1 = Y * d;
        const int s0 = off[r], s1 = off[r + 1];
        for (int k = s0; k < s1; ++k) {
            const int s = src[k];
            const double* __restrict__ T = mats + (long long)k * 32;          // T_rs, then T_sr
            MvProj pr;
            if (!mv_project_texel(T, q0, q1, d, W, H, &pr)) continue;
            const MvCell2 c = mv_cell2(masked + (long long)s * hw, W, H, pr.u, pr.v);
            if (!(c.d00 > 0.0 && c.d01 > 0.0 && c.d10 > 0.0 && c.d11 > 0.0)) continue;
            const double ds = c.bilinear();
            const double b0q = (pr.u + 0.5) * ds, b1q = (pr.v + 0.5) * ds;
            const double* __restrict__ B = T + 16;
            double bx = 0.0, by = 0.0, b2;                                     // set: nothing is carried around the loop (view_prims.h: mv_project)
            if (!mv_project(B, b0q, b1q, ds, bx, by, b2)) continue;
            const double ex = bx - X, ey = by - Y;
            if (ex * ex + ey * ey < pix2 && fabs(b2 - d) < dep_thresh * d) {
                ++n;
                acc += b2;
            }
        }
    }
    const bool kept = d > 0.0 && n >= vthresh;
    const double df = acc / (double)(n + 1);
    counts[at] = n;
    fused[at] = kept ? (float)df : 0.0f;
    dfo[at] = df;
    keep[at] = kept ? 1 : 0;
}

// step 4: the kept pixels of chunk blockIdx.x, in order, from row boff[blockIdx.x] on; nothing is written at or beyond row cap
__global__ __launch_bounds__(MV_THREADS) void k_fu_emit(const unsigned char* __restrict__ keep, const double* __restrict__ dfi, long long n, int H, int W,
                                                         const double* __restrict__ pinv, const long long* __restrict__ boff,
                                                         const unsigned char* __restrict__ images, double* __restrict__ points,
                                                         unsigned char* __restrict__ colors, int* __restrict__ view, int* __restrict__ pixel, long long cap) {
    __shared__ int sh[MV_THREADS];
    const long long base = (long long)blockIdx.x * MV_CHUNK + (long long)threadIdx.x * MV_ITEMS;
    int k[MV_ITEMS];
    long long row = mv_chunk_rank<MV_THREADS, MV_ITEMS>(keep, n, boff, k, sh);
    const long long hw = (long long)H * W;
#pragma unroll
    for (int q = 0; q < MV_ITEMS; ++q) {
        if (!k[q]) continue;
        if (row < cap) {
            const long long at = base + q;
            const int r = (int)(at / hw), p = (int)(at - (long long)r * hw);
            const int y = p / W, x = p - y * W;
            const double df = dfi[at];
            const double q0 = ((double)x + 0.5) * df, q1 = ((double)y + 0.5) * df;
            const double* __restrict__ T = pinv + (long long)r * 16;
            for (int c = 0; c < 3; ++c) points[row * 3 + c] = mv_row4(T + 4 * c, q0, q1, df, 1.0);
            if (images)
                for (int c = 0; c < 3; ++c) colors[row * 3 + c] = images[at * 3 + c];
            view[row] = r;
            pixel[row] = p;
        }
        ++row;
    }
}

// ---- normals of the fused points (fusion.py: depth_normals) ----
#define FU_NM_ROW 19                                  // doubles per view: Pinv (16), the camera centre (3)

// Q(x, y): rows 0..2 of Pinv applied to (X d, Y d, d, 1)
__device__ __forceinline__ void fu_backproject(const double* __restrict__ T, int x, int y, double d, double* q) {
    const double q0 = ((double)x + 0.5) * d, q1 = ((double)y + 0.5) * d;
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = mv_row4(T + 4 * c, q0, q1, d, 1.0);
}

// the tangent along one image axis from the neighbours at -step / +step texels: central, else forward, else backward; false when neither is usable
__device__ __forceinline__ bool fu_tangent(const float* __restrict__ map, const double* __restrict__ T, int W, int x, int y, int dx, int dy, bool in_lo, bool in_hi,
                                           double d, const double* qc, double jump, double* t) {
    double ql[3], qh[3];
    bool lo = false, hi = false;
    if (in_lo) {
        const double dn = (double)map[(long long)(y - dy) * W + (x - dx)];
        lo = dn > 0.0 && fabs(dn - d) <= jump * d;
        if (lo) fu_backproject(T, x - dx, y - dy, dn, ql);
    }
    if (in_hi) {
        const double dn = (double)map[(long long)(y + dy) * W + (x + dx)];
        hi = dn > 0.0 && fabs(dn - d) <= jump * d;
        if (hi) fu_backproject(T, x + dx, y + dy, dn, qh);
    }
    if (!lo && !hi) return false;
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = (hi ? qh[c] : qc[c]) - (lo ? ql[c] : qc[c]);
    return true;
}

// one lane per point; an index outside the maps sets MVSDF_FU_ERR_INDEX and gives a zero normal
__global__ __launch_bounds__(FU_THREADS) void k_fu_normals(const float* __restrict__ fused, int V, int H, int W, const int* __restrict__ view,
                                                            const int* __restrict__ pixel, long long n, const double* __restrict__ mats, double jump,
                                                            double* __restrict__ normals, unsigned long long* __restrict__ word) {
    const long long i = (long long)blockIdx.x * FU_THREADS + threadIdx.x;
    if (i >= n) return;
    const int r = view[i], p = pixel[i];
    double o[3] = {0.0, 0.0, 0.0};
    if (r < 0 || r >= V || p < 0 || p >= H * W) {
        atomicOr(word, (unsigned long long)MVSDF_FU_ERR_INDEX);
    } else {
        const int y = p / W, x = p - y * W;
        const float* __restrict__ map = fused + (long long)r * H * W;
        const double* __restrict__ T = mats + (long long)r * FU_NM_ROW;
        const double d = (double)map[p];
        double qc[3], tx[3], ty[3];
        fu_backproject(T, x, y, d, qc);
        if (fu_tangent(map, T, W, x, y, 1, 0, x > 0, x < W - 1, d, qc, jump, tx) && fu_tangent(map, T, W, x, y, 0, 1, y > 0, y < H - 1, d, qc, jump, ty)) {
            const double m0 = tx[1] * ty[2] - tx[2] * ty[1], m1 = tx[2] * ty[0] - tx[0] * ty[2], m2 = tx[0] * ty[1] - tx[1] * ty[0];
            const double len = sqrt((m0 * m0 + m1 * m1) + m2 * m2);
            if (len > 0.0 && len < (double)INFINITY) {
                const double n0 = m0 / len, n1 = m1 / len, n2 = m2 / len;
                const double c0 = T[16] - qc[0], c1 = T[17] - qc[1], c2 = T[18] - qc[2];
                const bool flip = ((n0 * c0 + n1 * c1) + n2 * c2) < 0.0;
                o[0] = flip ? -n0 : n0;
                o[1] = flip ? -n1 : n1;
                o[2] = flip ? -n2 : n2;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) normals[i * 3 + c] = o[c];
}

extern "C" {

size_t mvsdf_fusion_normals_workspace_bytes(int64_t V) {
    if (V < 1 || V > INT_MAX) return 0;
    return FU_HDR + mv_align256((size_t)V * FU_NM_ROW * 8);
}

// mats: host, [V][19] = Pinv_v row-major, then the camera centre.  Leaves int64 {0, error bits} at the start of the workspace; no host wait.
int mvsdf_fusion_normals(const float* fused, int64_t V, int64_t H, int64_t W, const int32_t* view, const int32_t* pixel, int64_t n, const double* mats,
                         double jump, void* ws, size_t ws_bytes, double* normals, void* stream) {
    const char* what = "mvsdf_fusion_normals";
    if (!fused || !view || !pixel || !mats || !ws || !normals || ws_bytes < FU_HDR) return mv_fail(-1, "mvsdf_fusion_normals: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    long long err = 0;
    if (V < 1 || H < 2 || W < 2 || V > INT_MAX || H > INT_MAX || W > INT_MAX || H * W > INT_MAX || n < 1 || n > FU_MAX_PIXELS) err |= MVSDF_FU_ERR_SHAPE;
    if (!(err & MVSDF_FU_ERR_SHAPE) && !mv_all_finite(mats, V * FU_NM_ROW)) err |= MVSDF_FU_ERR_FINITE;
    if (isnan(jump) || jump < 0.0) err |= MVSDF_FU_ERR_FINITE;
    if (err) return mv_refuse_header(ws, err, s, what);
    if (ws_bytes < mvsdf_fusion_normals_workspace_bytes(V)) return mv_fail(-1, "mvsdf_fusion_normals: workspace too small (mvsdf_fusion_normals_workspace_bytes)");
    char* w = (char*)ws;
    int rc;
    if ((rc = mv_check(hipMemsetAsync(ws, 0, FU_HDR, s), what))) return rc;
    if ((rc = mv_check(hipMemcpyAsync(w + FU_HDR, mats, (size_t)V * FU_NM_ROW * 8, hipMemcpyHostToDevice, s), what))) return rc;
    hipLaunchKernelGGL(k_fu_normals, dim3(mv_grid(n, FU_THREADS)), dim3(FU_THREADS), 0, s, fused, (int)V, (int)H, (int)W, view, pixel, (long long)n,
                       (const double*)(w + FU_HDR), jump, normals, (unsigned long long*)w + MVSDF_RES_H_ERR);
    return mv_check(hipGetLastError(), what);                   // no wait here: the caller keeps mats until it has read the header
}

size_t mvsdf_fusion_workspace_bytes(int64_t V, int64_t H, int64_t W, int64_t npairs) {
    FuLayout L;
    return fu_layout(V, H, W, npairs, &L) ? L.total : 0;
}

int mvsdf_fusion_fuse(const float* depths, const float* probs, const float* pthresh, int64_t V, int64_t H, int64_t W, const int32_t* pair_off,
                      const int32_t* pair_src, const double* mats, int32_t view, int32_t vthresh, double pix_thresh, double dep_thresh, void* ws,
                      size_t ws_bytes, float* masked, float* fused, int32_t* counts, void* stream) {
    const char* what = "mvsdf_fusion_fuse";
    if (!depths || !pair_off || !mats || !ws || !masked || !fused || !counts || (probs && !pthresh) || ws_bytes < FU_HDR)
        return mv_fail(-1, "mvsdf_fusion_fuse: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    // ---- validation, all of it before the first launch ----
    long long err = 0;
    if (view < 1) err |= MVSDF_FU_ERR_VIEW;
    long long npairs = 0;
    if (V < 1 || V > INT_MAX || pair_off[0] != 0) err |= MVSDF_FU_ERR_SHAPE;
    else {
        for (long long r = 0; r < V && !(err & MVSDF_FU_ERR_SHAPE); ++r) {
            const long long len = (long long)pair_off[r + 1] - pair_off[r];
            if (len < 0 || (view >= 1 && len > view)) err |= MVSDF_FU_ERR_SHAPE;
        }
        npairs = pair_off[V];
    }
    FuLayout L;
    if (!(err & MVSDF_FU_ERR_SHAPE) && (!fu_layout(V, H, W, npairs, &L) || (npairs > 0 && !pair_src))) err |= MVSDF_FU_ERR_SHAPE;
    if (!(err & MVSDF_FU_ERR_SHAPE)) {
        for (long long k = 0; k < npairs; ++k)
            if (pair_src[k] < 0 || pair_src[k] >= V) err |= MVSDF_FU_ERR_PAIR;
        if (!mv_all_finite(mats, npairs * 32 + V * 16)) err |= MVSDF_FU_ERR_FINITE;
        if (!isfinite(pix_thresh) || !isfinite(dep_thresh)) err |= MVSDF_FU_ERR_FINITE;
        if (probs && !(isfinite(pthresh[0]) && isfinite(pthresh[1]) && isfinite(pthresh[2]))) err |= MVSDF_FU_ERR_FINITE;
    }
    if (err) return mv_refuse_header(ws, err, s, what);
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_fusion_fuse: workspace too small (mvsdf_fusion_workspace_bytes)");
    // ---- uploads and launches ----
    char* w = (char*)ws;
    const long long hw = H * W, n = V * hw;
    int rc;
    if ((rc = mv_check(hipMemsetAsync(ws, 0, FU_HDR, s), what))) return rc;
    if (npairs > 0) {
        if ((rc = mv_check(hipMemcpyAsync(w + L.mats, mats, (size_t)npairs * 32 * 8, hipMemcpyHostToDevice, s), what))) return rc;
        if ((rc = mv_check(hipMemcpyAsync(w + L.src, pair_src, (size_t)npairs * 4, hipMemcpyHostToDevice, s), what))) return rc;
    }
    if ((rc = mv_check(hipMemcpyAsync(w + L.pinv, mats + npairs * 32, (size_t)V * 16 * 8, hipMemcpyHostToDevice, s), what))) return rc;
    if ((rc = mv_check(hipMemcpyAsync(w + L.off, pair_off, (size_t)(V + 1) * 4, hipMemcpyHostToDevice, s), what))) return rc;
    const float t1 = probs ? pthresh[0] : 0.f, t2 = probs ? pthresh[1] : 0.f, t3 = probs ? pthresh[2] : 0.f;
    hipLaunchKernelGGL(k_fu_mask, dim3(mv_grid(n, FU_THREADS)), dim3(FU_THREADS), 0, s, depths, probs, (long long)V, hw, t1, t2, t3, masked);
    const int tiles = (int)mv_ceil_div(hw, FU_THREADS);
    hipLaunchKernelGGL(k_fu_fuse, dim3((unsigned)(V * tiles)), dim3(FU_THREADS), 0, s, (const float*)masked, (int)V, (int)H, (int)W, tiles,
                       (const int*)(w + L.off), (const int*)(w + L.src), (const double*)(w + L.mats), (int)vthresh, pix_thresh * pix_thresh, dep_thresh,
                       counts, fused, (double*)(w + L.df), (unsigned char*)(w + L.keep));
    mv_scan_blocks((const unsigned char*)(w + L.keep), n, (long long*)(w + L.bsum), L.nb, (long long*)ws + MVSDF_RES_H_COUNT, s);
    return mv_check(hipGetLastError(), what);                   // no wait here: the caller keeps the host arrays until it has read the header
}

int mvsdf_fusion_emit(const uint8_t* images, int64_t V, int64_t H, int64_t W, int64_t npairs, void* ws, size_t ws_bytes, double* points,
                      uint8_t* colors, int32_t* view, int32_t* pixel, int64_t cap, void* stream) {
    FuLayout L;
    if (!ws || !points || !view || !pixel || (images && !colors) || cap < 1 || !fu_layout(V, H, W, npairs, &L))
        return mv_fail(-1, "mvsdf_fusion_emit: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_fusion_emit: workspace too small (mvsdf_fusion_workspace_bytes)");
    char* w = (char*)ws;
    hipLaunchKernelGGL(k_fu_emit, dim3((unsigned)L.nb), dim3(MV_THREADS), 0, (hipStream_t)stream, (const unsigned char*)(w + L.keep),
                       (const double*)(w + L.df), (long long)(V * H * W), (int)H, (int)W, (const double*)(w + L.pinv), (const long long*)(w + L.bsum),
                       images, points, colors, view, pixel, (long long)cap);
    return mv_check(hipGetLastError(), "mvsdf_fusion_emit");
}

}  // extern "C"
