// raster.hip -- on-device mesh rendering: a triangle mesh drawn into the scene's cameras (depth and face id per pixel), the visibility of its vertices
// per view against those depth maps, and vertex colours gathered from the input photographs.  Python: mvsdf_amd/raster.py, which states the
// definition; tests/raster_ref.py restates it in numpy.  All arithmetic is fp64 without contraction, in the order the definition writes it.
//
// * The depth buffer is a 64-bit key per pixel and view, (bits(fp32 depth) << 32) | face id, that starts at all ones and takes the minimum: positive
//   floats order as their bits, so the nearest surface wins and equal depths go to the lowest face id.  An integer minimum is the same in any order
//   and any grouping, so the result does not depend on the schedule.  Before each atomic the key is read with a plain load and the atomic is skipped
//   when the new key is not smaller: the buffer only decreases, so a stale (larger) value read there only costs an atomic, never a pixel.
// * k_ra_draw_small: one lane per (face, view) (blockIdx.y = the view, so the camera comes through the scalar cache), projecting its three vertices and
//   walking its clamped pixel box.  A face whose box holds more than large_face_pixels pixels is flagged instead of drawn.
// * the flags go through a count / scan / emit compaction (geom_prims.h: mv_scan_blocks over the uint8 flags, then k_ra_emit ranks its own chunk with
//   mv_chunk_rank) to a list of (face, view) items; k_ra_draw_large gives each item to one wave, whose lanes stride over the box.  The grid is
//   fixed and strides over the list, whose length it reads on the device: no host wait between the two paths.
// * k_ra_resolve: keys -> depth fp32 (0 where nothing was drawn) and face int32 (-1).
// * k_ra_visibility: one lane per (vertex, view); k_ra_colors: one lane per vertex, the views in order inside, so the weighted sum has one order.
//
// There is no clipping: a face with a vertex not in front of the camera is skipped.  Every device loop is bounded by the clamped pixel box or the
// view count; every index read from the caller (face -> vertex) is range-checked before it is used.  The projection, the visibility test, the edge
// function and the colour gather are view_prims.h's (mv_project, mv_visible, mv_edge, mv_cell / mv_gather_rgb), which texture.hip uses too.
#include "view_prims.h"

#define RA_THREADS 256
#define RA_HDR 256                                    // bytes at the start of the workspace: MVSDF_RA_H_*
static_assert(MVSDF_RA_H_WORDS * 8 <= RA_HDR, "the result words fit the header");
#define RA_WAVES (RA_THREADS / 64)
#define RA_LARGE_BLOCKS 4096                          // workgroups of the large path (it strides over the list)
#define RA_MAX_PIXELS (1ll << MVSDF_RA_MAX_PIXELS_LOG2)

enum { RA_FLAG_NO_PRETEST = 1, RA_FLAG_STATS = 2 };

struct RaLayout {
    size_t keys, flags, list, bsum, total;
    long long items, nb;
};

static bool ra_shape(long long views, long long H, long long W) { return mv_view_shape(views, H, W) && views * H * W <= RA_MAX_PIXELS; }

static bool ra_layout(long long nv, long long nf, long long views, long long H, long long W, RaLayout* L) {
    if (nv < 0 || nf < 0 || nv > INT_MAX || nf > INT_MAX || !ra_shape(views, H, W) || nf * views > INT_MAX) return false;
    L->items = nf * views;
    L->nb = mv_ceil_div(L->items, MV_CHUNK);
    WsCursor c{RA_HDR};
    L->keys = c.take((size_t)(views * H * W) * 8);
    L->flags = c.take((size_t)(L->items > 0 ? L->items : 1));
    L->list = c.take((size_t)(L->items > 0 ? L->items : 1) * 4);
    L->bsum = c.take(mv_scan_tmp_bytes(L->items));
    L->total = c.o;
    return true;
}

struct RaFace {
    double ax, ay, az, bx, by, bz, cx, cy, cz, A;
    bool flip;
    int x0, x1, y0, y1;
};

// the face's projected corners, signed area and clamped pixel box; false: the face draws nothing in this view
__device__ __forceinline__ bool ra_setup(const float* __restrict__ verts, const int* __restrict__ faces, long long nv, long long f,
                                         const double* __restrict__ P, double o, int H, int W, RaFace& g, unsigned long long* hdr) {
    const int a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
    if (a < 0 || b < 0 || c < 0 || a >= nv || b >= nv || c >= nv) {
        atomicOr(hdr + MVSDF_RA_H_ERR, (unsigned long long)MVSDF_RA_ERR_INDEX);
        return false;
    }
    if (!mv_project(P, verts + (long long)a * 3, g.ax, g.ay, g.az)) return false;
    if (!mv_project(P, verts + (long long)b * 3, g.bx, g.by, g.bz)) return false;
    if (!mv_project(P, verts + (long long)c * 3, g.cx, g.cy, g.cz)) return false;
    if (!(isfinite(g.ax) && isfinite(g.ay) && isfinite(g.az) && isfinite(g.bx) && isfinite(g.by) && isfinite(g.bz) && isfinite(g.cx) &&
          isfinite(g.cy) && isfinite(g.cz)))
        return false;
    const double A = mv_edge(g.ax, g.ay, g.bx, g.by, g.cx, g.cy);
    if (A == 0.0) return false;
    g.flip = A < 0.0;
    g.A = g.flip ? -A : A;
    const double lx = fmax(0.0, ceil(fmin(fmin(g.ax, g.bx), g.cx) - o)), hx = fmin((double)(W - 1), floor(fmax(fmax(g.ax, g.bx), g.cx) - o));
    const double ly = fmax(0.0, ceil(fmin(fmin(g.ay, g.by), g.cy) - o)), hy = fmin((double)(H - 1), floor(fmax(fmax(g.ay, g.by), g.cy) - o));
    if (!(lx <= hx && ly <= hy)) return false;
    g.x0 = (int)lx;                                   // all four lie in [0, W - 1] / [0, H - 1]
    g.x1 = (int)hx;
    g.y0 = (int)ly;
    g.y1 = (int)hy;
    return true;
}

template <bool PRE, bool STATS>
__device__ __forceinline__ void ra_pixel(const RaFace& g, int x, int y, double o, unsigned f, unsigned long long* __restrict__ keys, int W,
                                         unsigned& n_atomic, unsigned& n_covered) {
    const double px = (double)x + o, py = (double)y + o;
    double w0 = mv_edge(g.bx, g.by, g.cx, g.cy, px, py);
    double w1 = mv_edge(g.cx, g.cy, g.ax, g.ay, px, py);
    double w2 = mv_edge(g.ax, g.ay, g.bx, g.by, px, py);
    if (g.flip) {
        w0 = -w0;
        w1 = -w1;
        w2 = -w2;
    }
    if (!(w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0)) return;
    const double b0 = w0 / g.A, b1 = w1 / g.A, b2 = w2 / g.A;
    const double iz = (b0 / g.az + b1 / g.bz) + b2 / g.cz;
    const double zp = 1.0 / iz;
    if (!(isfinite(zp) && zp > 0.0)) return;
    const float d32 = (float)zp;
    if (d32 == 0.0f || isinf(d32)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(d32) << 32) | (unsigned long long)f;
    unsigned long long* p = keys + (long long)y * W + x;
    if (STATS) ++n_covered;
    if (PRE && *p <= key) return;
    if (STATS) ++n_atomic;
    atomicMin(p, key);
}

__device__ __forceinline__ void ra_stats(unsigned long long* hdr, unsigned n_atomic, unsigned n_covered) {
    if (n_atomic) atomicAdd(hdr + MVSDF_RA_H_ATOMICS, (unsigned long long)n_atomic);
    if (n_covered) atomicAdd(hdr + MVSDF_RA_H_COVERED, (unsigned long long)n_covered);
}

// the small path.  blockIdx.y = view; flags[view * nf + f] = 1 where the face is left to the large path
template <bool PRE, bool STATS>
__global__ __launch_bounds__(RA_THREADS) void k_ra_draw_small(const float* __restrict__ verts, const int* __restrict__ faces, long long nv, long long nf,
                                                               const double* __restrict__ P, double o, int H, int W, long long large,
                                                               unsigned long long* __restrict__ keys, unsigned char* __restrict__ flags,
                                                               unsigned long long* hdr) {
    const long long f = (long long)blockIdx.x * RA_THREADS + threadIdx.x;
    const int v = blockIdx.y;
    if (f >= nf) return;
    RaFace g;
    unsigned char big = 0;
    unsigned na = 0, nc = 0;
    if (ra_setup(verts, faces, nv, f, P + (long long)v * 16, o, H, W, g, hdr)) {
        const long long npix = (long long)(g.x1 - g.x0 + 1) * (g.y1 - g.y0 + 1);
        if (npix > large) big = 1;
        else {
            unsigned long long* kv = keys + (long long)v * H * W;
            for (int y = g.y0; y <= g.y1; ++y)
                for (int x = g.x0; x <= g.x1; ++x) ra_pixel<PRE, STATS>(g, x, y, o, (unsigned)f, kv, W, na, nc);
        }
    }
    flags[(long long)v * nf + f] = big;
    if (STATS) ra_stats(hdr, na, nc);
}

// the large path: one wave per listed (face, view), its lanes over the pixel box
template <bool PRE, bool STATS>
__global__ __launch_bounds__(RA_THREADS) void k_ra_draw_large(const float* __restrict__ verts, const int* __restrict__ faces, long long nv, long long nf,
                                                               const double* __restrict__ P, double o, int H, int W,
                                                               unsigned long long* __restrict__ keys, const int* __restrict__ list,
                                                               unsigned long long* hdr) {
    const int lane = threadIdx.x & 63;
    const long long n = (long long)hdr[MVSDF_RA_H_ITEMS], stride = (long long)gridDim.x * RA_WAVES;
    unsigned na = 0, nc = 0;
    for (long long e = (long long)blockIdx.x * RA_WAVES + (threadIdx.x >> 6); e < n; e += stride) {
        const long long item = list[e];
        const long long v = item / nf, f = item - v * nf;
        RaFace g;
        if (!ra_setup(verts, faces, nv, f, P + v * 16, o, H, W, g, hdr)) continue;
        const long long bw = g.x1 - g.x0 + 1, npix = bw * (g.y1 - g.y0 + 1);
        unsigned long long* kv = keys + v * H * W;
        for (long long q = lane; q < npix; q += 64) {
            const long long r = q / bw;
            ra_pixel<PRE, STATS>(g, g.x0 + (int)(q - r * bw), g.y0 + (int)r, o, (unsigned)f, kv, W, na, nc);
        }
    }
    if (STATS) ra_stats(hdr, na, nc);
}

// the flagged items of chunk blockIdx.x, in order, from entry boff[blockIdx.x] on
__global__ __launch_bounds__(MV_THREADS) void k_ra_emit(const unsigned char* __restrict__ flags, long long n, const long long* __restrict__ boff,
                                                         int* __restrict__ list) {
    __shared__ int sh[MV_THREADS];
    const long long base = (long long)blockIdx.x * MV_CHUNK + (long long)threadIdx.x * MV_ITEMS;
    int k[MV_ITEMS];
    long long row = mv_chunk_rank<MV_THREADS, MV_ITEMS>(flags, n, boff, k, sh);
#pragma unroll
    for (int q = 0; q < MV_ITEMS; ++q)
        if (k[q]) list[row++] = (int)(base + q);                  // row < the flags' total <= n, the list's length
}

__global__ __launch_bounds__(RA_THREADS) void k_ra_resolve(const unsigned long long* __restrict__ keys, long long n, float* __restrict__ depth,
                                                            int* __restrict__ face) {
    const long long i = (long long)blockIdx.x * RA_THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = keys[i];
    const bool drawn = k != ~0ull;
    depth[i] = drawn ? __uint_as_float((unsigned)(k >> 32)) : 0.0f;
    face[i] = drawn ? (int)(unsigned)(k & 0xffffffffull) : -1;
}

// blockIdx.y = view
__global__ __launch_bounds__(RA_THREADS) void k_ra_visibility(const float* __restrict__ verts, long long nv, const double* __restrict__ P, double o, int H,
                                                               int W, const float* __restrict__ depth, const unsigned char* __restrict__ masks,
                                                               double depth_tol, unsigned char* __restrict__ vis) {
    const long long i = (long long)blockIdx.x * RA_THREADS + threadIdx.x;
    const long long v = blockIdx.y, hw = (long long)H * W;
    if (i >= nv) return;
    double sx, sy;
    vis[v * nv + i] = mv_visible(P + v * 16, verts + i * 3, o, H, W, depth + v * hw, masks ? masks + v * hw : nullptr, depth_tol, sx, sy) ? 1 : 0;
}

__global__ __launch_bounds__(RA_THREADS) void k_ra_colors(const float* __restrict__ verts, const float* __restrict__ normals, long long nv,
                                                           const double* __restrict__ P, const double* __restrict__ C, int V, double o, int H, int W,
                                                           const float* __restrict__ depth, const unsigned char* __restrict__ masks,
                                                           const unsigned char* __restrict__ images, double depth_tol, double cos_min,
                                                           int ignore_normals, float f0, float f1, float f2, float* __restrict__ colors,
                                                           int* __restrict__ n_views) {
    const long long i = (long long)blockIdx.x * RA_THREADS + threadIdx.x;
    if (i >= nv) return;
    const long long hw = (long long)H * W;
    const float* X = verts + i * 3;
    const double X0 = (double)X[0], X1 = (double)X[1], X2 = (double)X[2];
    const double n0 = (double)normals[i * 3], n1 = (double)normals[i * 3 + 1], n2 = (double)normals[i * 3 + 2];
    const bool flat = n0 == 0.0 && n1 == 0.0 && n2 == 0.0;
    double S0 = 0.0, S1 = 0.0, S2 = 0.0, Wsum = 0.0;
    int used = 0;
    const double wmax = (double)(W - 1), hmax = (double)(H - 1);
    if (!(flat && !ignore_normals)) {
        for (int v = 0; v < V; ++v) {
            double sx, sy;
            if (!mv_visible(P + (long long)v * 16, X, o, H, W, depth + v * hw, masks ? masks + v * hw : nullptr, depth_tol, sx, sy)) continue;
            double wgt = 1.0;
            if (!flat) {
                const double g0 = C[v * 3] - X0, g1 = C[v * 3 + 1] - X1, g2 = C[v * 3 + 2] - X2;
                const double cosang = ((n0 * g0 + n1 * g1) + n2 * g2) / sqrt((g0 * g0 + g1 * g1) + g2 * g2);
                if (!(cosang > cos_min)) continue;
                wgt = cosang;
            }
            if (!mv_in_image(sx, sy, o, wmax, hmax)) continue;
            double col[3];
            mv_gather_rgb(images, v * hw, W, mv_cell(sx - o, sy - o, W, H), col);
            S0 += wgt * col[0];
            S1 += wgt * col[1];
            S2 += wgt * col[2];
            Wsum += wgt;
            ++used;
        }
    }
    const bool have = Wsum > 0.0;
    colors[i * 3] = have ? (float)(S0 / Wsum / 255.0) : f0;
    colors[i * 3 + 1] = have ? (float)(S1 / Wsum / 255.0) : f1;
    colors[i * 3 + 2] = have ? (float)(S2 / Wsum / 255.0) : f2;
    n_views[i] = used;
}

// MVSDF_RA_ERR_FINITE into the header where an entry of the cameras or centres m[n] is NaN or infinite
static void ra_check_finite(const double* m, long long n, void* ws, hipStream_t s) {
    hipLaunchKernelGGL(k_any_nonfinite<double>, dim3(1), dim3(MV_THREADS), 0, s, m, n, (unsigned long long*)ws + MVSDF_RA_H_ERR,
                       (unsigned long long)MVSDF_RA_ERR_FINITE);
}

template <bool PRE, bool STATS>
static void ra_launch_draw(const float* verts, const int32_t* faces, long long nv, long long nf, const double* P, long long views, double o, int H, int W,
                           long long large, char* w, const RaLayout& L, hipStream_t s) {
    unsigned long long* hdr = (unsigned long long*)w;
    unsigned long long* keys = (unsigned long long*)(w + L.keys);
    unsigned char* flags = (unsigned char*)(w + L.flags);
    int* list = (int*)(w + L.list);
    long long* bsum = (long long*)(w + L.bsum);
    hipLaunchKernelGGL((k_ra_draw_small<PRE, STATS>), dim3(mv_grid(nf, RA_THREADS), (unsigned)views), dim3(RA_THREADS), 0, s, verts, faces, nv,
                       nf, P, o, H, W, large, keys, flags, hdr);
    mv_scan_blocks((const unsigned char*)flags, L.items, bsum, L.nb, (long long*)(hdr + MVSDF_RA_H_ITEMS), s);
    hipLaunchKernelGGL(k_ra_emit, dim3((unsigned)L.nb), dim3(MV_THREADS), 0, s, (const unsigned char*)flags, L.items, (const long long*)bsum, list);
    const long long waves = mv_ceil_div(L.items, RA_WAVES);
    hipLaunchKernelGGL((k_ra_draw_large<PRE, STATS>), dim3((unsigned)(waves < RA_LARGE_BLOCKS ? waves : RA_LARGE_BLOCKS)), dim3(RA_THREADS), 0, s, verts,
                       faces, nv, nf, P, o, H, W, keys, (const int*)list, hdr);
}

extern "C" {

size_t mvsdf_raster_workspace_bytes(int64_t nv, int64_t nf, int64_t views, int64_t H, int64_t W) {
    RaLayout L;
    return ra_layout(nv, nf, views, H, W, &L) ? L.total : 0;
}

int mvsdf_raster_draw(const float* verts, const int32_t* faces, int64_t nv, int64_t nf, const double* P, int64_t views, int64_t H, int64_t W,
                      double pixel_center, int64_t large_face_pixels, int32_t flags, void* ws, size_t ws_bytes, void* stream) {
    const char* what = "mvsdf_raster_draw";
    RaLayout L;
    if (!P || !ws || (nf > 0 && (!verts || !faces)) || !mv_pixel_center(pixel_center) || large_face_pixels < 0 || !ra_layout(nv, nf, views, H, W, &L))
        return mv_fail(-1, "mvsdf_raster_draw: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_raster_draw: workspace too small (mvsdf_raster_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)ws;
    int rc;
    if ((rc = mv_check(hipMemsetAsync(ws, 0, RA_HDR, s), what))) return rc;
    if ((rc = mv_check(hipMemsetAsync(w + L.keys, 0xff, (size_t)(views * H * W) * 8, s), what))) return rc;
    ra_check_finite(P, views * 16, ws, s);
    if (nf > 0) {
        const bool pre = !(flags & RA_FLAG_NO_PRETEST), stats = (flags & RA_FLAG_STATS) != 0;
        if (pre && !stats) ra_launch_draw<true, false>(verts, faces, nv, nf, P, views, pixel_center, (int)H, (int)W, large_face_pixels, w, L, s);
        else if (pre) ra_launch_draw<true, true>(verts, faces, nv, nf, P, views, pixel_center, (int)H, (int)W, large_face_pixels, w, L, s);
        else if (!stats) ra_launch_draw<false, false>(verts, faces, nv, nf, P, views, pixel_center, (int)H, (int)W, large_face_pixels, w, L, s);
        else ra_launch_draw<false, true>(verts, faces, nv, nf, P, views, pixel_center, (int)H, (int)W, large_face_pixels, w, L, s);
    }
    return mv_check(hipGetLastError(), what);
}

int mvsdf_raster_resolve(int64_t views, int64_t H, int64_t W, void* ws, size_t ws_bytes, float* depth, int32_t* face, void* stream) {
    if (!ws || !depth || !face || !ra_shape(views, H, W)) return mv_fail(-1, "mvsdf_raster_resolve: bad arguments");
    const long long n = views * H * W;
    if (ws_bytes < RA_HDR + (size_t)n * 8) return mv_fail(-1, "mvsdf_raster_resolve: workspace too small (mvsdf_raster_workspace_bytes)");
    hipLaunchKernelGGL(k_ra_resolve, dim3(mv_grid(n, RA_THREADS)), dim3(RA_THREADS), 0, (hipStream_t)stream,
                       (const unsigned long long*)((char*)ws + RA_HDR), n, depth, face);
    return mv_check(hipGetLastError(), "mvsdf_raster_resolve");
}

int mvsdf_raster_visibility(const float* verts, int64_t nv, const double* P, int64_t views, int64_t H, int64_t W, double pixel_center,
                            const float* depth, const uint8_t* masks, double depth_tol, void* ws, size_t ws_bytes, uint8_t* vis, void* stream) {
    const char* what = "mvsdf_raster_visibility";
    if (!P || !depth || !ws || ws_bytes < RA_HDR || nv < 0 || nv > INT_MAX || (nv > 0 && (!verts || !vis)) || !mv_pixel_center(pixel_center) ||
        !isfinite(depth_tol) || !ra_shape(views, H, W))
        return mv_fail(-1, "mvsdf_raster_visibility: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = mv_check(hipMemsetAsync(ws, 0, RA_HDR, s), what)) return rc;
    ra_check_finite(P, views * 16, ws, s);
    if (nv > 0)
        hipLaunchKernelGGL(k_ra_visibility, dim3(mv_grid(nv, RA_THREADS), (unsigned)views), dim3(RA_THREADS), 0, s, verts, (long long)nv, P,
                           pixel_center, (int)H, (int)W, depth, masks, depth_tol, vis);
    return mv_check(hipGetLastError(), what);
}

int mvsdf_raster_colors(const float* verts, const float* normals, int64_t nv, const double* P, const double* centers, int64_t views, int64_t H,
                        int64_t W, double pixel_center, const float* depth, const uint8_t* masks, const uint8_t* images, double depth_tol,
                        double cos_min, int32_t ignore_normals, float fallback_r, float fallback_g, float fallback_b, void* ws, size_t ws_bytes,
                        float* colors, int32_t* n_views, void* stream) {
    const char* what = "mvsdf_raster_colors";
    if (!P || !centers || !depth || !images || !ws || ws_bytes < RA_HDR || nv < 0 || nv > INT_MAX || (nv > 0 && (!verts || !normals || !colors || !n_views)) ||
        !mv_pixel_center(pixel_center) || !isfinite(depth_tol) || !isfinite(cos_min) || !ra_shape(views, H, W))
        return mv_fail(-1, "mvsdf_raster_colors: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = mv_check(hipMemsetAsync(ws, 0, RA_HDR, s), what)) return rc;
    ra_check_finite(P, views * 16, ws, s);
    ra_check_finite(centers, views * 3, ws, s);
    if (nv > 0)
        hipLaunchKernelGGL(k_ra_colors, dim3(mv_grid(nv, RA_THREADS)), dim3(RA_THREADS), 0, s, verts, normals, (long long)nv, P, centers,
                           (int)views, pixel_center, (int)H, (int)W, depth, masks, images, depth_tol, cos_min, (int)ignore_normals, fallback_r, fallback_g,
                           fallback_b, colors, n_views);
    return mv_check(hipGetLastError(), what);
}

}  // extern "C"
