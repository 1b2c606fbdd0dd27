// texture.hip -- on-device texture atlases: every face of a mesh labelled with the view that sees it largest, a patch per face packed along one
// Morton curve, and the texels of the atlas gathered from the photographs.  Python: mvsdf_amd/texture.py, which states the definition;
// tests/texture_ref.py restates it in numpy.  All arithmetic is fp64 without contraction, in the order the definition writes it; every integer
// decision is an exact comparison, so no schedule can move a bit.
//
// * k_tx_face_views: one lane per face, the views in order inside (the label takes the first view of the largest |A|, so there is one order).  It
//   also writes the six screen coordinates of the face in its view, which the later stages read (the fill can project them again instead:
//   TX_FLAG_RECOMPUTE, the A/B of DESIGN.md).  The projection, the visibility test, the edge function and the texel gather are the ones raster.hip
//   uses: view_prims.h's mv_project, mv_visible, mv_edge and mv_cell / mv_gather_rgb.  The test of one face in one view is tx_prims.h's
//   tx_face_in_view, which charts.hip asks for the one view it names.
// * k_tx_classify: the size class of every face at a texel density, and the seven class counts (integer atomics).  The host reads the counts: the
//   atlas size follows from them alone (tx_layout), and the max_size loop repeats only this pass.
// * the stable counting sort is ONE scan: flags[(6 - class) * nf + f] over 7 * nf bytes, so the exclusive prefix of a set flag is the face's place in
//   the order by class descending, face ascending (mv_scan_blocks, then k_tx_emit ranks its own chunk with mv_chunk_rank).  k_tx_emit writes the
//   order, the patch and the UVs of its faces.
// * k_tx_fill: one lane per four texels of a row (they share their 4 x 4 block, hence their cell), rows along the wave: 12-byte stores side by side.
//   The owner of a texel follows from the Morton index of its block and the class offsets; no per-texel table exists.  Its LEVEL flag adds the seam
//   levelling correction of the face's three nodes before the rounding (mvsdf_seams_fill, the last entry below; the rest of that module: seams.hip).
//
// Every index read from the caller (face -> vertex, order -> face, label -> view) is range-checked before it is used; the image position is clamped
// before it becomes an address; all offsets into the images are 64-bit.
#include "tx_prims.h"

#define TX_THREADS 256
#define TX_HDR 256                                    // bytes at the start of the workspace: MVSDF_TX_H_*
#define TX_CLASSES 7
static_assert(MVSDF_TX_H_WORDS * 8 <= TX_HDR && MVSDF_SL_H_WORDS * 8 <= TX_HDR && MVSDF_TX_H_COUNTS + TX_CLASSES == MVSDF_TX_H_WORDS, "the result words fit the header");
#define TX_NMIN 4
#define TX_MAX_FACES (1ll << MVSDF_TX_MAX_FACES_LOG2)
#define TX_INSET 0.75                                 // the right-angle corner's distance from the cell's edges, in texels
#define TX_LEG_LOSS 3.5                               // leg = n - TX_LEG_LOSS

enum { TX_FLAG_RECOMPUTE = 1 };

// where the classes lie, by value to the kernels.  Class k holds the patches of edge TX_NMIN << k; the classes follow each other in DESCENDING order
struct TxLayout {
    long long count[TX_CLASSES];      // faces
    long long start[TX_CLASSES];      // place of the class's first face in the order
    long long off[TX_CLASSES];        // first block index (blocks of TX_NMIN x TX_NMIN texels along the Morton curve)
    long long end[TX_CLASSES];        // one past its last block
    long long T;                      // blocks in use
    int Wt, Ht;
};

// false: counts that are negative, do not sum to nf, or an atlas beyond MVSDF_TX_MAX_SIDE
static bool tx_layout(const int64_t* counts, long long nf, TxLayout* L) {
    long long sum = 0, at = 0, blocks = 0;
    if (!counts || nf < 0 || nf > TX_MAX_FACES) return false;
    for (int k = TX_CLASSES - 1; k >= 0; --k) {
        const long long c = counts[k];
        if (c < 0 || c > nf) return false;
        L->count[k] = c;
        L->start[k] = at;
        L->off[k] = blocks;
        at += c;
        blocks += ((c + 1) >> 1) << (2 * k);
        L->end[k] = blocks;
        sum += c;
    }
    if (sum != nf) return false;
    L->T = blocks;
    int B = 0;
    while (B < 62 && (1ll << B) < blocks) ++B;
    const long long Wt = (long long)TX_NMIN << ((B + 1) / 2), Ht = (long long)TX_NMIN << (B / 2);
    if (Wt > MVSDF_TX_MAX_SIDE) return false;
    L->Wt = (int)Wt;
    L->Ht = (int)Ht;
    return true;
}

struct TxWs {
    size_t flags, bsum, total;
    long long items, nb;
};

static bool tx_ws(long long nf, TxWs* w) {
    if (nf < 0 || nf > TX_MAX_FACES) return false;
    w->items = nf * TX_CLASSES;
    w->nb = mv_ceil_div(w->items, MV_CHUNK);
    WsCursor c{TX_HDR};
    w->flags = c.take((size_t)(w->items > 0 ? w->items : 1));
    w->bsum = c.take(mv_scan_tmp_bytes(w->items));
    w->total = c.o;
    return true;
}

__global__ __launch_bounds__(TX_THREADS) void k_tx_face_views(const float* __restrict__ verts, const float* __restrict__ normals,
                                                               const int* __restrict__ faces, long long nv, long long nf,
                                                               const double* __restrict__ P, const double* __restrict__ C, int V, double o, int H, int W,
                                                               const float* __restrict__ depth, const unsigned char* __restrict__ masks,
                                                               double depth_tol, double cos_min, int ignore_normals, int* __restrict__ label,
                                                               double* __restrict__ score, double* __restrict__ screen, unsigned long long* hdr) {
    const long long f = (long long)blockIdx.x * TX_THREADS + threadIdx.x;
    if (f >= nf) return;
    const long long hw = (long long)H * W;
    const int a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
    int best = -1;
    double bs = 0.0, s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (a < 0 || b < 0 || c < 0 || a >= nv || b >= nv || c >= nv) {
        atomicOr(hdr + MVSDF_TX_H_ERR, (unsigned long long)MVSDF_TX_ERR_INDEX);
    } else {
        const TxFace F = tx_face(verts, normals, a, b, c);
        if (!(F.flat && !ignore_normals)) {
            for (int v = 0; v < V; ++v) {
                double sc, sv[6];
                if (!tx_face_in_view(F, P + (long long)v * 16, C + (long long)v * 3, o, H, W, depth + v * hw, masks ? masks + v * hw : nullptr, depth_tol,
                                     cos_min, sc, sv))
                    continue;
                if (sc > bs) {                                    // strictly: a tie stays with the lower view
                    bs = sc;
                    best = v;
#pragma unroll
                    for (int q = 0; q < 6; ++q) s[q] = sv[q];
                }
            }
        }
    }
    label[f] = best;
    score[f] = bs;
#pragma unroll
    for (int q = 0; q < 6; ++q) screen[f * 6 + q] = s[q];
}

// the size class of a face: the smallest k with (2 n - 7)^2 >= ((4 L2) d) d, n = TX_NMIN << k
__global__ __launch_bounds__(TX_THREADS) void k_tx_classify(const int* __restrict__ label, const double* __restrict__ screen, long long nf, double d,
                                                             unsigned char* __restrict__ cls, unsigned long long* hdr) {
    const long long f = (long long)blockIdx.x * TX_THREADS + threadIdx.x;
    int k = f < nf ? 0 : -1;                                      // every lane stays for the ballots below
    if (f < nf && label[f] >= 0) {
        const double* s = screen + f * 6;
        const double abx = s[2] - s[0], aby = s[3] - s[1], bcx = s[4] - s[2], bcy = s[5] - s[3], cax = s[0] - s[4], cay = s[1] - s[5];
        const double L2 = fmax(fmax(abx * abx + aby * aby, bcx * bcx + bcy * bcy), cax * cax + cay * cay);
        const double need = ((4.0 * L2) * d) * d;
        k = TX_CLASSES - 1;
#pragma unroll
        for (int q = TX_CLASSES - 2; q >= 0; --q) {
            const double e = (double)(2 * (TX_NMIN << q) - 7);
            if (e * e >= need) k = q;
        }
    }
    if (f < nf) cls[f] = (unsigned char)k;
    // one global atomic per workgroup and class: a mesh whose faces nearly all share a class would otherwise queue every lane on one address
    // (measured: 7.5 ms for 641 172 faces with an atomic per lane)
    __shared__ unsigned cnt[TX_CLASSES];
    if (threadIdx.x < TX_CLASSES) cnt[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < TX_CLASSES; ++q) {
        const unsigned long long b = __ballot(k == q);
        if (b && (threadIdx.x & 63) == 0) atomicAdd(&cnt[q], (unsigned)__popcll(b));
    }
    __syncthreads();
    if (threadIdx.x < TX_CLASSES && cnt[threadIdx.x]) atomicAdd(hdr + MVSDF_TX_H_COUNTS + threadIdx.x, (unsigned long long)cnt[threadIdx.x]);
}

// flags[r * nf + f] = the face is of class 6 - r
__global__ __launch_bounds__(TX_THREADS) void k_tx_flags(const unsigned char* __restrict__ cls, long long nf, long long items,
                                                          unsigned char* __restrict__ flags) {
    const long long i = (long long)blockIdx.x * TX_THREADS + threadIdx.x;
    if (i >= items) return;
    const long long r = i / nf, f = i - r * nf;
    flags[i] = cls[f] == (unsigned char)(TX_CLASSES - 1 - r) ? 1 : 0;
}

// the even bits of x, packed
__device__ __forceinline__ unsigned tx_even_bits(unsigned long long x) {
    x &= 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x >> 4)) & 0x00ff00ff00ff00ffull;
    x = (x | (x >> 8)) & 0x0000ffff0000ffffull;
    x = (x | (x >> 16)) & 0x00000000ffffffffull;
    return (unsigned)x;
}

// x spread over the even bits (x < 2^16)
__device__ __forceinline__ unsigned tx_spread_bits(unsigned x) {
    x = (x | (x << 8)) & 0x00ff00ffu;
    x = (x | (x << 4)) & 0x0f0f0f0fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}

// the set flags of chunk blockIdx.x are the places boff[blockIdx.x] .. of the order: order, patch and uv of those faces
__global__ __launch_bounds__(MV_THREADS) void k_tx_emit(const unsigned char* __restrict__ flags, long long nf, long long items,
                                                         const long long* __restrict__ boff, TxLayout L, int* __restrict__ order,
                                                         int* __restrict__ patch, float* __restrict__ uv, unsigned long long* hdr) {
    __shared__ int sh[MV_THREADS];
    const long long base = (long long)blockIdx.x * MV_CHUNK + (long long)threadIdx.x * MV_ITEMS;
    int k[MV_ITEMS];
    long long row = mv_chunk_rank<MV_THREADS, MV_ITEMS>(flags, items, boff, k, sh);
#pragma unroll
    for (int q = 0; q < MV_ITEMS; ++q) {
        if (!k[q]) continue;
        const long long pos = row++, i = base + q;
        const long long r = i / nf, f = i - r * nf;
        const int c = TX_CLASSES - 1 - (int)r;
        const long long rank = pos - L.start[c];
        if (rank < 0 || rank >= L.count[c]) {                     // the counts are not those of cls: nothing is written (start + count <= nf)
            atomicOr(hdr + MVSDF_TX_H_ERR, (unsigned long long)MVSDF_TX_ERR_COUNTS);
            continue;
        }
        order[pos] = (int)f;
        const unsigned long long blk = (unsigned long long)(L.off[c] + ((rank >> 1) << (2 * c)));
        const int n = TX_NMIN << c, half = (int)(rank & 1);
        const int x0 = TX_NMIN * (int)tx_even_bits(blk), y0 = TX_NMIN * (int)tx_even_bits(blk >> 1);
        patch[f * 4] = x0;
        patch[f * 4 + 1] = y0;
        patch[f * 4 + 2] = n;
        patch[f * 4 + 3] = half;
        const double leg = (double)n - TX_LEG_LOSS, lo = TX_INSET, hi = (double)n - TX_INSET;
        const double ca = half ? hi : lo, cb = half ? hi - leg : lo + leg;
        const double cx[3] = {ca, cb, ca}, cy[3] = {ca, ca, cb};
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            uv[f * 6 + e * 2] = (float)(((double)x0 + cx[e]) / (double)L.Wt);
            uv[f * 6 + e * 2 + 1] = (float)(1.0 - ((double)y0 + cy[e]) / (double)L.Ht);
        }
    }
}

struct TxTexel {
    unsigned r, g, b, valid;
};

// LEVEL (seam levelling, seams.py's step 6): the unrounded colour gets the face's three node corrections g blended with the texel's barycentric
// weights, and is clamped to [0, 255] before it is rounded.  A face whose nodes are out of range raises MVSDF_TX_ERR_INDEX and stays unlevelled.
template <bool RECOMPUTE, bool LEVEL>
__global__ __launch_bounds__(TX_THREADS) void k_tx_fill(const unsigned char* __restrict__ images, int V, int H, int W, double o,
                                                         const int* __restrict__ label, const double* __restrict__ screen,
                                                         const int* __restrict__ order, long long nf, const float* __restrict__ verts,
                                                         const int* __restrict__ faces, long long nv, const double* __restrict__ P, TxLayout L,
                                                         unsigned fr, unsigned fg, unsigned fb, unsigned* __restrict__ texture,
                                                         unsigned* __restrict__ valid, const int* __restrict__ corner_node,
                                                         const double* __restrict__ g, long long K, unsigned long long* hdr) {
    const long long t = (long long)blockIdx.x * TX_THREADS + threadIdx.x;
    const int Wq = L.Wt / 4;
    if (t >= (long long)Wq * L.Ht) return;
    const int j = (int)(t / Wq), i0 = 4 * (int)(t - (long long)j * Wq);
    const long long m = (long long)(tx_spread_bits((unsigned)(i0 >> 2)) | (tx_spread_bits((unsigned)(j >> 2)) << 1));
    int c = -1;
#pragma unroll
    for (int k = 0; k < TX_CLASSES; ++k)
        if (m >= L.off[k] && m < L.end[k]) c = k;
    TxTexel px[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) px[e] = {fr, fg, fb, 0u};
    if (c >= 0) {
        const int n = TX_NMIN << c, x0 = i0 & ~(n - 1), y0 = j & ~(n - 1), lj = j - y0;
        const long long cell = (m - L.off[c]) >> (2 * c);
        const double leg = (double)n - TX_LEG_LOSS, wmax = (double)(W - 1), hmax = (double)(H - 1);
        const long long hw = (long long)H * W;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int li = i0 + e - x0;
            const int half = li + lj <= n - 1 ? 0 : 1;
            const long long rank = 2 * cell + half;
            if (rank >= L.count[c]) continue;                     // the empty half of an odd class's last cell
            const long long f = order[L.start[c] + rank];
            if (f < 0 || f >= nf) continue;
            const int v = label[f];
            if (v < 0 || v >= V) continue;
            double s[6];
            if (RECOMPUTE) {
                const int a = faces[f * 3], b = faces[f * 3 + 1], cc = faces[f * 3 + 2];
                if (a < 0 || b < 0 || cc < 0 || a >= nv || b >= nv || cc >= nv) continue;
                const double* Pv = P + (long long)v * 16;
                double z;
                if (!mv_project(Pv, verts + (long long)a * 3, s[0], s[1], z)) continue;
                if (!mv_project(Pv, verts + (long long)b * 3, s[2], s[3], z)) continue;
                if (!mv_project(Pv, verts + (long long)cc * 3, s[4], s[5], z)) continue;
            } else {
#pragma unroll
                for (int q = 0; q < 6; ++q) s[q] = screen[f * 6 + q];
            }
            double qx = (double)li + 0.5, qy = (double)lj + 0.5;
            if (half) {
                qx = (double)n - qx;
                qy = (double)n - qy;
            }
            const double beta = (qx - TX_INSET) / leg, gamma = (qy - TX_INSET) / leg, alpha = (1.0 - beta) - gamma;
            const double sx = (alpha * s[0] + beta * s[2]) + gamma * s[4], sy = (alpha * s[1] + beta * s[3]) + gamma * s[5];
            const double u = fmin(fmax(sx - o, 0.0), wmax), w = fmin(fmax(sy - o, 0.0), hmax);      // a NaN becomes 0: always an address inside
            double col[3];
            mv_gather_rgb(images, v * hw, W, mv_cell(u, w, W, H), col);
            if (LEVEL) {
                const int na = corner_node[f * 3], nb = corner_node[f * 3 + 1], nc = corner_node[f * 3 + 2];
                if (na < 0 || nb < 0 || nc < 0 || na >= K || nb >= K || nc >= K) {
                    atomicOr(hdr + MVSDF_SL_H_ERR, (unsigned long long)MVSDF_TX_ERR_INDEX);
                } else {
                    const double *ga = g + (long long)na * 3, *gb = g + (long long)nb * 3, *gc = g + (long long)nc * 3;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch)
                        col[ch] = fmin(fmax(col[ch] + ((alpha * ga[ch] + beta * gb[ch]) + gamma * gc[ch]), 0.0), 255.0);   // a NaN becomes 0
                }
            }
            unsigned out[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) out[ch] = (unsigned)floor(col[ch] + 0.5) & 0xffu;
            px[e] = {out[0], out[1], out[2], 1u};
        }
    }
    // twelve bytes r g b r g b ... of four texels as three words, the valid bytes as one (Wt is a multiple of 4: every row starts on a word)
    const long long at = (long long)j * Wq + (i0 >> 2);
    texture[at * 3] = px[0].r | (px[0].g << 8) | (px[0].b << 16) | (px[1].r << 24);
    texture[at * 3 + 1] = px[1].g | (px[1].b << 8) | (px[2].r << 16) | (px[2].g << 24);
    texture[at * 3 + 2] = px[2].b | (px[3].r << 8) | (px[3].g << 16) | (px[3].b << 24);
    valid[at] = px[0].valid | (px[1].valid << 8) | (px[2].valid << 16) | (px[3].valid << 24);
}

extern "C" {

size_t mvsdf_texture_workspace_bytes(int64_t nf) {
    TxWs w;
    return tx_ws(nf, &w) ? w.total : 0;
}

int mvsdf_texture_face_views(const float* verts, const float* normals, const int32_t* faces, int64_t nv, int64_t nf, const double* P,
                             const double* centers, int64_t views, int64_t H, int64_t W, double pixel_center, const float* depth, const uint8_t* masks,
                             double depth_tol, double cos_min, int32_t ignore_normals, void* ws, size_t ws_bytes, int32_t* label, double* score,
                             double* screen, void* stream) {
    const char* what = "mvsdf_texture_face_views";
    if (!P || !centers || !depth || !ws || ws_bytes < TX_HDR || nv < 0 || nv > INT_MAX || nf < 0 || nf > TX_MAX_FACES ||
        (nf > 0 && (!verts || !normals || !faces || !label || !score || !screen)) || !mv_pixel_center(pixel_center) || !isfinite(depth_tol) ||
        !isfinite(cos_min) || !mv_view_shape(views, H, W))
        return mv_fail(-1, "mvsdf_texture_face_views: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = mv_check(hipMemsetAsync(ws, 0, TX_HDR, s), what)) return rc;
    unsigned long long* errword = (unsigned long long*)ws + MVSDF_TX_H_ERR;
    hipLaunchKernelGGL(k_any_nonfinite<double>, dim3(1), dim3(MV_THREADS), 0, s, P, (long long)views * 16, errword, (unsigned long long)MVSDF_TX_ERR_FINITE);
    hipLaunchKernelGGL(k_any_nonfinite<double>, dim3(1), dim3(MV_THREADS), 0, s, centers, (long long)views * 3, errword, (unsigned long long)MVSDF_TX_ERR_FINITE);
    if (nf > 0)
        hipLaunchKernelGGL(k_tx_face_views, dim3(mv_grid(nf, TX_THREADS)), dim3(TX_THREADS), 0, s, verts, normals, faces, (long long)nv, (long long)nf, P,
                           centers, (int)views, pixel_center, (int)H, (int)W, depth, masks, depth_tol, cos_min, (int)ignore_normals, label, score, screen,
                           (unsigned long long*)ws);
    return mv_check(hipGetLastError(), what);
}

int mvsdf_texture_classify(const int32_t* label, const double* screen, int64_t nf, double density, void* ws, size_t ws_bytes, uint8_t* cls,
                           void* stream) {
    const char* what = "mvsdf_texture_classify";
    if (!ws || ws_bytes < TX_HDR || nf < 0 || nf > TX_MAX_FACES || (nf > 0 && (!label || !screen || !cls)) || !isfinite(density) || !(density > 0.0))
        return mv_fail(-1, "mvsdf_texture_classify: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = mv_check(hipMemsetAsync(ws, 0, TX_HDR, s), what)) return rc;
    if (nf > 0)
        hipLaunchKernelGGL(k_tx_classify, dim3(mv_grid(nf, TX_THREADS)), dim3(TX_THREADS), 0, s, label, screen, (long long)nf, density, cls,
                           (unsigned long long*)ws);
    return mv_check(hipGetLastError(), what);
}

int mvsdf_texture_pack(const uint8_t* cls, int64_t nf, const int64_t* counts, void* ws, size_t ws_bytes, int32_t* order, int32_t* patch, float* uv,
                       void* stream) {
    const char* what = "mvsdf_texture_pack";
    TxLayout L;
    TxWs w;
    if (!ws || !tx_ws(nf, &w) || (nf > 0 && (!cls || !order || !patch || !uv)) || !tx_layout(counts, nf, &L))
        return mv_fail(-1, "mvsdf_texture_pack: bad arguments (the counts must be those of the classes and give an atlas of at most 32768 texels a side)");
    if (ws_bytes < w.total) return mv_fail(-1, "mvsdf_texture_pack: workspace too small (mvsdf_texture_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    char* b = (char*)ws;
    if (int rc = mv_check(hipMemsetAsync(ws, 0, TX_HDR, s), what)) return rc;
    if (nf > 0) {
        unsigned char* flags = (unsigned char*)(b + w.flags);
        long long* bsum = (long long*)(b + w.bsum);
        hipLaunchKernelGGL(k_tx_flags, dim3(mv_grid(w.items, TX_THREADS)), dim3(TX_THREADS), 0, s, cls, (long long)nf, w.items, flags);
        mv_scan_blocks((const unsigned char*)flags, w.items, bsum, w.nb, (long long*)ws + MVSDF_TX_H_COUNTS, s);   // the flagged total
        hipLaunchKernelGGL(k_tx_emit, dim3((unsigned)w.nb), dim3(MV_THREADS), 0, s, (const unsigned char*)flags, (long long)nf, w.items,
                           (const long long*)bsum, L, order, patch, uv, (unsigned long long*)ws);
    }
    return mv_check(hipGetLastError(), what);
}

int mvsdf_texture_fill(const uint8_t* images, int64_t views, int64_t H, int64_t W, double pixel_center, const int32_t* label, const double* screen,
                       const int32_t* order, int64_t nf, const int64_t* counts, const float* verts, const int32_t* faces, int64_t nv, const double* P,
                       int32_t flags, int32_t fallback_r, int32_t fallback_g, int32_t fallback_b, int64_t Ht, int64_t Wt, uint8_t* texture,
                       uint8_t* valid, void* stream) {
    const char* what = "mvsdf_texture_fill";
    TxLayout L;
    const bool re = (flags & TX_FLAG_RECOMPUTE) != 0;
    if (!images || !texture || !valid || !mv_pixel_center(pixel_center) || !mv_view_shape(views, H, W) || nv < 0 || nv > INT_MAX ||
        (nf > 0 && (!label || !order || (re ? (!verts || !faces || !P) : !screen))) || fallback_r < 0 || fallback_r > 255 || fallback_g < 0 ||
        fallback_g > 255 || fallback_b < 0 || fallback_b > 255 || !tx_layout(counts, nf, &L))
        return mv_fail(-1, "mvsdf_texture_fill: bad arguments");
    if (Ht != L.Ht || Wt != L.Wt) return mv_fail(-1, "mvsdf_texture_fill: Ht x Wt is not the atlas of these counts");
    const long long quads = (long long)(L.Wt / 4) * L.Ht;
    hipStream_t s = (hipStream_t)stream;
    if (re)
        hipLaunchKernelGGL((k_tx_fill<true, false>), dim3(mv_grid(quads, TX_THREADS)), dim3(TX_THREADS), 0, s, images, (int)views, (int)H, (int)W, pixel_center,
                           label, screen, order, (long long)nf, verts, faces, (long long)nv, P, L, (unsigned)fallback_r, (unsigned)fallback_g,
                           (unsigned)fallback_b, (unsigned*)texture, (unsigned*)valid, (const int*)nullptr, (const double*)nullptr, 0ll,
                           (unsigned long long*)nullptr);
    else
        hipLaunchKernelGGL((k_tx_fill<false, false>), dim3(mv_grid(quads, TX_THREADS)), dim3(TX_THREADS), 0, s, images, (int)views, (int)H, (int)W, pixel_center,
                           label, screen, order, (long long)nf, verts, faces, (long long)nv, P, L, (unsigned)fallback_r, (unsigned)fallback_g,
                           (unsigned)fallback_b, (unsigned*)texture, (unsigned*)valid, (const int*)nullptr, (const double*)nullptr, 0ll,
                           (unsigned long long*)nullptr);
    return mv_check(hipGetLastError(), what);
}

int mvsdf_seams_fill(const uint8_t* images, int64_t views, int64_t H, int64_t W, double pixel_center, const int32_t* label, const double* screen,
                     const int32_t* order, int64_t nf, const int64_t* counts, const int32_t* corner_node, const double* g, int64_t nodes,
                     int32_t fallback_r, int32_t fallback_g, int32_t fallback_b, void* ws, size_t ws_bytes, int64_t Ht, int64_t Wt, uint8_t* texture,
                     uint8_t* valid, void* stream) {
    const char* what = "mvsdf_seams_fill";
    TxLayout L;
    if (!images || !texture || !valid || !ws || ws_bytes < TX_HDR || !mv_pixel_center(pixel_center) || !mv_view_shape(views, H, W) || nodes < 0 ||
        nodes > 3 * TX_MAX_FACES || (nf > 0 && (!label || !order || !screen || !corner_node)) || (nodes > 0 && !g) || fallback_r < 0 ||
        fallback_r > 255 || fallback_g < 0 || fallback_g > 255 || fallback_b < 0 || fallback_b > 255 || !tx_layout(counts, nf, &L))
        return mv_fail(-1, "mvsdf_seams_fill: bad arguments");
    if (Ht != L.Ht || Wt != L.Wt) return mv_fail(-1, "mvsdf_seams_fill: Ht x Wt is not the atlas of these counts");
    const long long quads = (long long)(L.Wt / 4) * L.Ht;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = mv_check(hipMemsetAsync(ws, 0, TX_HDR, s), what)) return rc;
    hipLaunchKernelGGL((k_tx_fill<false, true>), dim3(mv_grid(quads, TX_THREADS)), dim3(TX_THREADS), 0, s, images, (int)views, (int)H, (int)W,
                       pixel_center, label, screen, order, (long long)nf, (const float*)nullptr, (const int*)nullptr, 0ll, (const double*)nullptr, L,
                       (unsigned)fallback_r, (unsigned)fallback_g, (unsigned)fallback_b, (unsigned*)texture, (unsigned*)valid, corner_node, g,
                       (long long)nodes, (unsigned long long*)ws);
    return mv_check(hipGetLastError(), what);
}

}  // extern "C"
