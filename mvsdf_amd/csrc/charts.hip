// charts.hip -- on-device chart atlases: the stage between face labels and texels.  A chart is a connected region of faces that took the same
// photograph; its patch is a rectangle cut from that photograph with a margin; the rectangles are packed on shelves.  Python: mvsdf_amd/charts.py,
// which states the definition; tests/charts_ref.py restates it in numpy.  All arithmetic is fp64 without contraction, in the order the definition
// writes it; every integer decision is an exact comparison; every sum or extremum over faces is an integer atomic, so no schedule can move a bit.
//
// * k_ca_scores / k_ca_absorb: tx_prims.h's test of one face in one view, the same code the label pass of texture.hip runs.
// * neighbours: ONE stable radix sort (nn_tree.h) of the 3 nf undirected edge keys; a run of exactly two equal keys is a pair.
// * components: hook-and-jump rounds over parent[] (parent[x] <= x always, every value a face of x's component).  k_ca_hook lowers the parents of two
//   linked faces' parents to the smaller one (atomicMin), k_ca_jump replaces every parent by its root.  A round that hooks nothing has settled; its
//   word switches the later rounds of the batch off.  The root of a component is its lowest face, whatever the schedule was.
// * pack: integer atomicMin / atomicMax of floor and ceil of the corners per chart (floor(min u) = min floor(u)), one sort by height, one scan of the
//   sorted widths, ONE lane that walks the shelves by binary search over the prefix, then every chart finds its shelf by binary search.
// * k_ca_fill: one lane per four texels of a row, blockIdx.y = the row, so the shelf is uniform per workgroup and its x table sits in LDS (up to
//   CA_LDS_X charts a shelf; beyond that the search reads global memory).  12-byte stores side by side, as k_tx_fill.
// * face map: k_ca_map_small gives a face to one lane over its texel box; a box above MVSDF_CA_LARGE_FACE texels is flagged and k_ca_map_large gives
//   it to one wave (raster.hip's route; no list: the waves stride over the flags).  The lowest face wins by a 32-bit atomicMin.
//
// Every index read from memory (face -> vertex, face -> chart, place -> chart, chart -> view, texel -> face, corner -> node) is range-checked before
// it is used; searches run over ranges the host passed; the image position is clamped before it becomes an address; image offsets are 64-bit.
#include "nn_tree.h"
#include "tx_prims.h"

#define CA_T 256
#define CA_HDR 256
#define CA_MAX_FACES (1ll << MVSDF_TX_MAX_FACES_LOG2)
#define CA_LDS_X 512                                  // charts of one shelf whose x table fits the fill's LDS
#define CA_LARGE_BLOCKS 1024
#define CA_NONE 0x7fffffff
static_assert(MVSDF_CA_H_WORDS <= 32 && MVSDF_CA_H_WORDS * 8 <= CA_HDR, "the result words fit the header");
static_assert(MVSDF_CA_RECT_CAP == 2 * MVSDF_TX_MAX_SIDE, "a capped rectangle never fits");

typedef unsigned long long ca_u64;
__device__ __forceinline__ void ca_raise(ca_u64* hdr, long long bit) { atomicOr(hdr + MVSDF_CA_H_ERR, (ca_u64)bit); }

static int ca_bits(long long x) {                     // the bits that hold 0 .. x
    int b = 1;
    while (b < 62 && (1ll << b) <= x) ++b;
    return b;
}

// one workspace layout for every call: sized for the 3 nf edge keys, which is more than any other stage needs
struct CaWs {
    size_t k0, k1, v0, v1, parent, flags, rank, changed, bounds, pre, map2, total;
    long long n3;
    ChSortLayout S;
};

static bool ca_ws(long long nf, long long texels, CaWs* w) {
    if (nf < 0 || nf > CA_MAX_FACES || texels < 0 || texels > (long long)MVSDF_TX_MAX_SIDE * MVSDF_TX_MAX_SIDE) return false;
    const long long m = nf > 0 ? 3 * nf : 1, f1 = nf > 0 ? nf : 1;
    w->n3 = 3 * nf;
    WsCursor c{CA_HDR};
    w->k0 = c.take((size_t)m * 8);
    w->k1 = c.take((size_t)m * 8);
    w->v0 = c.take((size_t)m * 4);
    w->v1 = c.take((size_t)m * 4);
    w->parent = c.take((size_t)f1 * 4);
    w->flags = c.take((size_t)f1);
    w->rank = c.take((size_t)f1 * 8);
    w->changed = c.take((size_t)(MVSDF_CA_MAX_ROUNDS + 1) * 4);
    w->bounds = c.take((size_t)f1 * 16);
    w->pre = c.take((size_t)(f1 + 1) * 8);
    ch_sort_layout(m, m, c, &w->S);
    w->map2 = c.take((size_t)(texels > 0 ? texels : 1) * 4);
    w->total = c.o;
    return true;
}

static bool ca_pad(int pad) { return pad == 1 || pad == 2 || pad == 4 || pad == 8; }

// ================================================================ scores ================================================================
__global__ __launch_bounds__(CA_T) void k_ca_scores(const float* __restrict__ verts, const float* __restrict__ normals, const int* __restrict__ faces,
                                                     long long nv, long long nf, const double* __restrict__ P, const double* __restrict__ C, int V, double o,
                                                     int H, int W, const float* __restrict__ depth, const unsigned char* __restrict__ masks,
                                                     double depth_tol, double cos_min, int ignore_normals, const int* __restrict__ view,
                                                     double* __restrict__ score, double* __restrict__ screen, ca_u64* hdr) {
    const long long f = (long long)blockIdx.x * CA_T + threadIdx.x;
    if (f >= nf) return;
    const long long hw = (long long)H * W;
    const int a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2], v = view[f];
    double sc = 0.0, s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (a < 0 || b < 0 || c < 0 || a >= nv || b >= nv || c >= nv) {
        ca_raise(hdr, MVSDF_TX_ERR_INDEX);
    } else if (v < -1 || v >= V) {
        ca_raise(hdr, MVSDF_TX_ERR_LABEL);
    } else if (v >= 0) {
        const TxFace F = tx_face(verts, normals, a, b, c);
        double q, sv[6];
        if (!(F.flat && !ignore_normals) &&
            tx_face_in_view(F, P + (long long)v * 16, C + (long long)v * 3, o, H, W, depth + v * hw, masks ? masks + v * hw : nullptr, depth_tol, cos_min, q, sv)) {
            sc = q;
#pragma unroll
            for (int k = 0; k < 6; ++k) s[k] = sv[k];
        }
    }
    score[f] = sc;
#pragma unroll
    for (int k = 0; k < 6; ++k) screen[f * 6 + k] = s[k];
}

// ================================================================ neighbours ================================================================
// key of edge 3 f + e: (lo << bits) | hi of its two vertex ids, 0 (which no edge with lo < hi has) where the ids are equal or out of range
__global__ __launch_bounds__(CA_T) void k_ca_edge_keys(const int* __restrict__ faces, long long nv, long long n3, int bits, ca_u64* __restrict__ key,
                                                        int* __restrict__ val, int* __restrict__ nbr, ca_u64* hdr) {
    const long long i = (long long)blockIdx.x * CA_T + threadIdx.x;
    if (i >= n3) return;
    const long long f = i / 3;
    const int e = (int)(i - f * 3);
    const int p = faces[i], q = faces[f * 3 + (e + 1) % 3];
    ca_u64 k = 0;
    if (p < 0 || q < 0 || p >= nv || q >= nv)
        ca_raise(hdr, MVSDF_TX_ERR_INDEX);
    else if (p != q)
        k = ((ca_u64)min(p, q) << bits) | (ca_u64)max(p, q);
    key[i] = k;
    val[i] = (int)i;
    nbr[i] = -1;
}

// sorted position i starts a run of exactly two equal keys: the two edges are each other's neighbours, unless one face holds both
__global__ __launch_bounds__(CA_T) void k_ca_pairs(const ca_u64* __restrict__ key, const int* __restrict__ val, long long n3, int* __restrict__ nbr) {
    const long long i = (long long)blockIdx.x * CA_T + threadIdx.x;
    if (i + 1 >= n3) return;
    const ca_u64 k = key[i];
    if (k == 0 || key[i + 1] != k || (i > 0 && key[i - 1] == k) || (i + 2 < n3 && key[i + 2] == k)) return;
    const int a = val[i], b = val[i + 1];
    if (a < 0 || b < 0 || a >= n3 || b >= n3 || a / 3 == b / 3) return;
    nbr[a] = b / 3;
    nbr[b] = a / 3;
}

// ================================================================ components ================================================================
__global__ __launch_bounds__(CA_T) void k_ca_parent_init(const int* __restrict__ label, long long nf, int* __restrict__ parent, int* __restrict__ chart_view,
                                                          int* __restrict__ chart_faces, ca_u64* hdr) {
    const long long f = (long long)blockIdx.x * CA_T + threadIdx.x;
    if (f >= nf) return;
    const int l = label[f];
    if (l < -1) ca_raise(hdr, MVSDF_TX_ERR_LABEL);
    parent[f] = l >= 0 ? (int)f : -1;
    chart_view[f] = 0;
    chart_faces[f] = 0;
}

__global__ __launch_bounds__(CA_T) void k_ca_hook(const int* __restrict__ label, const int* __restrict__ nbr, long long nf, int* parent, int* changed,
                                                   int round, ca_u64* hdr) {
    if (round > 0 && changed[round - 1] == 0) return;
    const long long f = (long long)blockIdx.x * CA_T + threadIdx.x;
    if (f >= nf) return;
    const int l = label[f];
    if (l < 0) return;
    bool hooked = false;
    for (int e = 0; e < 3; ++e) {
        const int g = nbr[f * 3 + e];
        if (g < -1 || g >= nf) {
            if (round == 0) ca_raise(hdr, MVSDF_TX_ERR_INDEX);
            continue;
        }
        if (g < 0 || label[g] != l) continue;
        const int pf = parent[f], pg = parent[g];                 // both >= 0: the faces are labelled
        if (pg < pf) {
            atomicMin(&parent[pf], pg);
            hooked = true;
        } else if (pf < pg) {
            atomicMin(&parent[pg], pf);
            hooked = true;
        }
    }
    if (hooked) atomicOr(&changed[round], 1);
}

__global__ __launch_bounds__(CA_T) void k_ca_jump(long long nf, int* parent, const int* changed, int round) {
    if (changed[round] == 0) return;
    const long long f = (long long)blockIdx.x * CA_T + threadIdx.x;
    if (f >= nf) return;
    int p = parent[f];
    if (p < 0) return;
    for (long long step = 0; step < nf; ++step) {                 // parents only decrease: the walk ends at a root
        const int q = parent[p];
        if (q == p) break;
        p = q;
    }
    parent[f] = p;
}

// the rounds enqueued, and the bit of a walk that did not settle
__global__ __launch_bounds__(64) void k_ca_note(ca_u64* hdr, ca_u64 rounds, ca_u64 bit) {
    if (threadIdx.x != 0) return;
    hdr[MVSDF_CA_H_ROUNDS] = rounds;
    if (bit) atomicOr(hdr + MVSDF_CA_H_ERR, bit);
}

__global__ __launch_bounds__(CA_T) void k_ca_heads(const int* __restrict__ parent, long long nf, unsigned char* __restrict__ flags) {
    const long long f = (long long)blockIdx.x * CA_T + threadIdx.x;
    if (f < nf) flags[f] = parent[f] == (int)f ? 1 : 0;
}

__global__ __launch_bounds__(CA_T) void k_ca_number(const int* __restrict__ label, const int* __restrict__ parent, const long long* __restrict__ rank,
                                                     long long nf, int* __restrict__ face_chart, int* __restrict__ chart_view, int* chart_faces) {
    const long long f = (long long)blockIdx.x * CA_T + threadIdx.x;
    if (f >= nf) return;
    const int p = parent[f];
    int c = -1;
    if (p >= 0 && p < nf) {
        c = (int)rank[p];
        if (p == f) chart_view[c] = label[f];
        atomicAdd(&chart_faces[c], 1);
    }
    face_chart[f] = c;
}

// ================================================================ absorption ================================================================
__global__ __launch_bounds__(CA_T) void k_ca_absorb(const float* __restrict__ verts, const float* __restrict__ normals, const int* __restrict__ faces,
                                                     long long nv, long long nf, const double* __restrict__ P, const double* __restrict__ C, int V, double o,
                                                     int H, int W, const float* __restrict__ depth, const unsigned char* __restrict__ masks,
                                                     double depth_tol, double cos_min, int ignore_normals, const int* __restrict__ label,
                                                     const int* __restrict__ nbr, const int* __restrict__ face_chart, const int* __restrict__ chart_faces,
                                                     long long nc, int min_faces, int* __restrict__ label_out, double* __restrict__ score,
                                                     double* __restrict__ screen, ca_u64* hdr) {
    const long long f = (long long)blockIdx.x * CA_T + threadIdx.x;
    if (f >= nf) return;
    const long long hw = (long long)H * W;
    const int lf = label[f], cf = face_chart[f];
    int best = -1;
    double bs = 0.0, s[6];
    if (lf >= 0 && cf >= nc) ca_raise(hdr, MVSDF_TX_ERR_INDEX);
    if (lf >= 0 && cf >= 0 && cf < nc && chart_faces[cf] < min_faces) {
        const int a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
        if (a < 0 || b < 0 || c < 0 || a >= nv || b >= nv || c >= nv) {
            ca_raise(hdr, MVSDF_TX_ERR_INDEX);
        } else {
            const TxFace F = tx_face(verts, normals, a, b, c);
            for (int e = 0; e < 3; ++e) {
                const int g = nbr[f * 3 + e];
                if (g < 0 || g >= nf) continue;
                const int v = label[g], cg = face_chart[g];
                if (v < 0 || v == lf || cg < 0 || cg >= nc || chart_faces[cg] < min_faces) continue;
                if (v >= V) {
                    ca_raise(hdr, MVSDF_TX_ERR_LABEL);
                    continue;
                }
                if (F.flat && !ignore_normals) continue;
                double sc, sv[6];
                if (!tx_face_in_view(F, P + (long long)v * 16, C + (long long)v * 3, o, H, W, depth + v * hw, masks ? masks + v * hw : nullptr, depth_tol,
                                     cos_min, sc, sv))
                    continue;
                if (sc > 0.0 && (sc > bs || (sc == bs && v < best))) {
                    bs = sc;
                    best = v;
#pragma unroll
                    for (int k = 0; k < 6; ++k) s[k] = sv[k];
                }
            }
        }
    }
    label_out[f] = best >= 0 ? best : lf;
    if (best >= 0) {
        score[f] = bs;
#pragma unroll
        for (int k = 0; k < 6; ++k) screen[f * 6 + k] = s[k];
        atomicAdd(hdr + MVSDF_CA_H_CHANGES, 1ull);
    }
}

// ================================================================ rectangles and shelves ================================================================
__global__ __launch_bounds__(CA_T) void k_ca_bounds_init(long long nc, int* __restrict__ bounds) {
    const long long c = (long long)blockIdx.x * CA_T + threadIdx.x;
    if (c >= nc) return;
    bounds[c * 4] = bounds[c * 4 + 2] = INT_MAX;
    bounds[c * 4 + 1] = bounds[c * 4 + 3] = INT_MIN;
}

// a screen coordinate as u = s - o inside [0, m] (a NaN becomes 0)
__device__ __forceinline__ double ca_inside(double s, double o, double m) { return fmin(fmax(s - o, 0.0), m); }

__global__ __launch_bounds__(CA_T) void k_ca_bounds(const int* __restrict__ face_chart, const double* __restrict__ screen, long long nf, long long nc,
                                                     double o, int H, int W, int* bounds, ca_u64* hdr) {
    const long long f = (long long)blockIdx.x * CA_T + threadIdx.x;
    if (f >= nf) return;
    const int c = face_chart[f];
    if (c < 0) {
        if (c < -1) ca_raise(hdr, MVSDF_TX_ERR_INDEX);
        return;
    }
    if (c >= nc) {
        ca_raise(hdr, MVSDF_TX_ERR_INDEX);
        return;
    }
    int lo[2] = {INT_MAX, INT_MAX}, hi[2] = {INT_MIN, INT_MIN};
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const double u = ca_inside(screen[f * 6 + k * 2 + a], o, (double)((a ? H : W) - 1));
            lo[a] = min(lo[a], (int)floor(u));
            hi[a] = max(hi[a], (int)ceil(u));
        }
    atomicMin(&bounds[c * 4], lo[0]);
    atomicMax(&bounds[c * 4 + 1], hi[0]);
    atomicMin(&bounds[c * 4 + 2], lo[1]);
    atomicMax(&bounds[c * 4 + 3], hi[1]);
}

// roundup(ceil(extent * d) + 1 + 2 pad, pad), capped
__device__ __forceinline__ int ca_side(int lo, int hi, double d, int pad) {
    const double t = fmin(ceil((double)(hi - lo) * d), (double)MVSDF_CA_RECT_CAP);      // a NaN becomes the cap
    const long long n = (long long)t + 1 + 2 * pad;
    return (int)min((long long)MVSDF_CA_RECT_CAP, (n + pad - 1) / pad * pad);
}

__global__ __launch_bounds__(CA_T) void k_ca_sizes(const int* __restrict__ bounds, long long nc, double d, int pad, int* __restrict__ rect,
                                                    ca_u64* __restrict__ key, int* __restrict__ val, ca_u64* hdr) {
    const long long c = (long long)blockIdx.x * CA_T + threadIdx.x;
    if (c >= nc) return;
    int u0 = bounds[c * 4], u1 = bounds[c * 4 + 1], t0 = bounds[c * 4 + 2], t1 = bounds[c * 4 + 3];
    if (u0 > u1 || t0 > t1) {                                     // no face named this chart
        ca_raise(hdr, MVSDF_TX_ERR_COUNTS);
        u0 = u1 = t0 = t1 = 0;
    }
    const int w = ca_side(u0, u1, d, pad), h = ca_side(t0, t1, d, pad);
    rect[c * 6] = 0;
    rect[c * 6 + 1] = 0;
    rect[c * 6 + 2] = w;
    rect[c * 6 + 3] = h;
    rect[c * 6 + 4] = u0;
    rect[c * 6 + 5] = t0;
    key[c] = (ca_u64)(MVSDF_CA_RECT_CAP - h);
    val[c] = (int)c;
    atomicMax(hdr + MVSDF_CA_H_MAXW, (ca_u64)w);
    atomicMax(hdr + MVSDF_CA_H_MAXH, (ca_u64)h);
    atomicAdd(hdr + MVSDF_CA_H_AREA, (ca_u64)w * (ca_u64)h);
}

__global__ __launch_bounds__(CA_T) void k_ca_widths(const int* __restrict__ val, const int* __restrict__ rect, long long nc, long long* __restrict__ wsorted) {
    const long long k = (long long)blockIdx.x * CA_T + threadIdx.x;
    if (k >= nc) return;
    const int c = val[k];
    wsorted[k] = c >= 0 && c < nc ? rect[(long long)c * 6 + 2] : 0;
}

// one lane: the atlas width, then the shelves.  pre[k] = the widths before place k, pre[nc] = all of them.
__global__ __launch_bounds__(64) void k_ca_shelves(const long long* __restrict__ pre, const int* __restrict__ val, const int* __restrict__ rect, long long nc,
                                                    int* __restrict__ shelves, ca_u64* hdr) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const long long maxw = (long long)hdr[MVSDF_CA_H_MAXW], area = (long long)hdr[MVSDF_CA_H_AREA];
    long long Wt = 1;
    while (Wt < maxw || Wt * Wt < area) Wt *= 2;                  // maxw <= 2^16, area <= 2^60
    long long k = 0, y = 0, s = 0;
    while (k < nc) {
        const int c = val[k];
        const long long hs = c >= 0 && c < nc ? rect[(long long)c * 6 + 3] : 0, limit = pre[k] + Wt;
        long long lo = k + 1, hi = nc;                            // the largest e in [k + 1, nc] with pre[e] <= limit (pre[k + 1] <= limit: w <= Wt)
        while (lo < hi) {
            const long long mid = (lo + hi + 1) >> 1;
            if (pre[mid] <= limit) lo = mid;
            else hi = mid - 1;
        }
        shelves[s * 2] = (int)k;
        shelves[s * 2 + 1] = (int)min(y, (long long)INT_MAX);
        y += hs;
        ++s;
        k = lo;
    }
    shelves[s * 2] = (int)nc;
    shelves[s * 2 + 1] = (int)min(y, (long long)INT_MAX);
    hdr[MVSDF_CA_H_WT] = (ca_u64)Wt;
    hdr[MVSDF_CA_H_HT] = (ca_u64)y;
    hdr[MVSDF_CA_H_SHELVES] = (ca_u64)s;
}

// the largest s in [0, ns) with shelves[s][col] <= x (shelves[0] = {0, 0})
__device__ __forceinline__ int ca_shelf_of(const int* __restrict__ shelves, int ns, int col, int x) {
    int lo = 0, hi = ns - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (shelves[mid * 2 + col] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(CA_T) void k_ca_place(const long long* __restrict__ pre, const int* __restrict__ val, long long nc, const int* __restrict__ shelves,
                                                    const ca_u64* __restrict__ hdr, int* __restrict__ rect, int* __restrict__ order, int* __restrict__ xs) {
    const long long k = (long long)blockIdx.x * CA_T + threadIdx.x;
    if (k >= nc) return;
    const int ns = (int)hdr[MVSDF_CA_H_SHELVES];                  // 1 .. nc
    const int s = ca_shelf_of(shelves, ns, 0, (int)k), first = shelves[s * 2];
    const int x = (int)min(pre[k] - pre[first], (long long)INT_MAX), c = val[k];
    order[k] = c;
    xs[k] = x;
    if (c >= 0 && c < nc) {
        rect[(long long)c * 6] = x;
        rect[(long long)c * 6 + 1] = shelves[s * 2 + 1];
    }
}

// ================================================================ UVs ================================================================
// the atlas coordinate of a corner: (X + pad + 0.5) + ((s - o) - u0) * d
__device__ __forceinline__ double ca_coord(int X, int pad, double s, double o, int u0, double d) {
    return ((double)(X + pad) + 0.5) + ((s - o) - (double)u0) * d;
}

__global__ __launch_bounds__(CA_T) void k_ca_uv(const int* __restrict__ face_chart, const double* __restrict__ screen, long long nf, const int* __restrict__ rect,
                                                 long long nc, double o, double d, int pad, double Wt, double Ht, float* __restrict__ uv, ca_u64* hdr) {
    const long long f = (long long)blockIdx.x * CA_T + threadIdx.x;
    if (f >= nf) return;
    const int c = face_chart[f];
    if (c < -1 || c >= nc) ca_raise(hdr, MVSDF_TX_ERR_INDEX);
    const bool has = c >= 0 && c < nc;
    const int* r = rect + (has ? (long long)c * 6 : 0);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double x = has ? ca_coord(r[0], pad, screen[f * 6 + k * 2], o, r[4], d) : 0.5;
        const double y = has ? ca_coord(r[1], pad, screen[f * 6 + k * 2 + 1], o, r[5], d) : 0.5;
        uv[f * 6 + k * 2] = (float)(x / Wt);
        uv[f * 6 + k * 2 + 1] = (float)(1.0 - y / Ht);
    }
}

// ================================================================ owners ================================================================
struct CaTables {
    const int *rect, *order, *xs, *shelves;
    int nc, ns, Wt, Ht;
};

// the place in [first, end) of the last chart of a shelf that starts at or before column i (x table xt indexed from `first`, xt[0] = 0)
__device__ __forceinline__ int ca_place_in_shelf(const int* xt, int first, int end, int i) {
    int lo = first, hi = end - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (xt[mid - first] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the chart whose rectangle holds texel (i, j) of that shelf, -1: none
__device__ __forceinline__ int ca_owner_in_shelf(const CaTables& T, const int* xt, int first, int end, int i, int j) {
    const int c = T.order[ca_place_in_shelf(xt, first, end, i)];
    if (c < 0 || c >= T.nc) return -1;
    const int* r = T.rect + (long long)c * 6;
    return i >= r[0] && i < r[0] + r[2] && j >= r[1] && j < r[1] + r[3] ? c : -1;
}

// the places [first, end) of the shelf that holds row j; false: the tables are not a packing's
__device__ __forceinline__ bool ca_row_shelf(const CaTables& T, int j, int& first, int& end) {
    const int s = ca_shelf_of(T.shelves, T.ns, 1, j);
    first = T.shelves[s * 2];
    end = T.shelves[s * 2 + 2];
    return first >= 0 && first < end && end <= T.nc;
}

__device__ __forceinline__ int ca_owner(const CaTables& T, int i, int j) {
    int first, end;
    if (!ca_row_shelf(T, j, first, end)) return -1;
    return ca_owner_in_shelf(T, T.xs + first, first, end, i, j);
}

// ================================================================ fill ================================================================
struct CaLevel {
    const int *face_map, *face_chart, *corner_node;
    const double *screen, *g;
    double o;
    long long nf, K;
};

template <bool LEVEL>
__global__ __launch_bounds__(CA_T) void k_ca_fill(const unsigned char* __restrict__ images, int V, int H, int W, const int* __restrict__ chart_view, CaTables T,
                                                   double d, int pad, unsigned fr, unsigned fg, unsigned fb, CaLevel L, unsigned* __restrict__ texture,
                                                   unsigned* __restrict__ valid, ca_u64* hdr) {
    __shared__ int sx[CA_LDS_X];
    __shared__ int range[3];
    const int j = blockIdx.y, Wq = T.Wt / 4;
    if (threadIdx.x == 0) {
        int first, end;
        range[2] = ca_row_shelf(T, j, first, end) ? 1 : 0;
        range[0] = first;
        range[1] = end;
    }
    __syncthreads();
    const int first = range[0], end = range[1];
    const bool ok = range[2] != 0, lds = ok && end - first <= CA_LDS_X;
    if (lds)
        for (int k = threadIdx.x; k < end - first; k += CA_T) sx[k] = T.xs[first + k];
    __syncthreads();
    const int q = blockIdx.x * CA_T + threadIdx.x;
    if (q >= Wq) return;
    const int i0 = 4 * q;
    if (!ok && threadIdx.x == 0) ca_raise(hdr, MVSDF_TX_ERR_INDEX);
    const double wmax = (double)(W - 1), hmax = (double)(H - 1);
    const long long hw = (long long)H * W;
    unsigned pr[4], pg[4], pb[4], pv[4];
    // the four texels of a lane mostly share their chart: one search for the first, a step to the next place where a later texel has left the
    // chart, and the chart's row (view, rectangle, t) is read again only when the place has moved
    const int* xt = lds ? sx : T.xs + first;
    int k = -1, loaded = -2, c = -1, v = 0;
    const int* r = T.rect;
    double t = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        pr[e] = fr, pg[e] = fg, pb[e] = fb, pv[e] = 0u;
        const int i = i0 + e;
        if (!ok) continue;
        if (e == 0) {
            k = ca_place_in_shelf(xt, first, end, i);
        } else {
            while (k + 1 < end && xt[k + 1 - first] <= i) ++k;
        }
        if (k != loaded) {
            loaded = k;
            c = T.order[k];
            if (c < 0 || c >= T.nc) {
                c = -1;
            } else {
                r = T.rect + (long long)c * 6;
                v = chart_view[c];
                if (j < r[1] || j >= r[1] + r[3]) {
                    c = -1;
                } else if (v < 0 || v >= V) {
                    ca_raise(hdr, MVSDF_TX_ERR_INDEX);
                    c = -1;
                } else {
                    t = fmin(fmax((double)r[5] + (double)(j - r[1] - pad) / d, 0.0), hmax);       // a NaN becomes 0: always an address inside
                }
            }
        }
        if (c < 0 || i < r[0] || i >= r[0] + r[2]) continue;
        const double u = fmin(fmax((double)r[4] + (double)(i - r[0] - pad) / d, 0.0), wmax);
        double col[3];
        mv_gather_rgb(images, v * hw, W, mv_cell(u, t, W, H), col);
        if (LEVEL) {
            const int f = L.face_map[(long long)j * T.Wt + i];
            if (f >= L.nf || f < -1) ca_raise(hdr, MVSDF_TX_ERR_INDEX);
            if (f >= 0 && f < L.nf) {
                const int na = L.corner_node[(long long)f * 3], nb = L.corner_node[(long long)f * 3 + 1], nc = L.corner_node[(long long)f * 3 + 2];
                if (na < 0 || nb < 0 || nc < 0 || na >= L.K || nb >= L.K || nc >= L.K || L.face_chart[f] != c) {
                    ca_raise(hdr, MVSDF_TX_ERR_INDEX);
                } else {
                    const double* s = L.screen + (long long)f * 6;
                    const double ax = ca_coord(r[0], pad, s[0], L.o, r[4], d), ay = ca_coord(r[1], pad, s[1], L.o, r[5], d);
                    const double bx = ca_coord(r[0], pad, s[2], L.o, r[4], d), by = ca_coord(r[1], pad, s[3], L.o, r[5], d);
                    const double cx = ca_coord(r[0], pad, s[4], L.o, r[4], d), cy = ca_coord(r[1], pad, s[5], L.o, r[5], d);
                    const double px = (double)i + 0.5, py = (double)j + 0.5, A = mv_edge(ax, ay, bx, by, cx, cy);
                    const double alpha = mv_edge(bx, by, cx, cy, px, py) / A, beta = mv_edge(cx, cy, ax, ay, px, py) / A,
                                 gamma = mv_edge(ax, ay, bx, by, px, py) / A;
                    const double *ga = L.g + (long long)na * 3, *gb = L.g + (long long)nb * 3, *gc = L.g + (long long)nc * 3;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch)
                        col[ch] = fmin(fmax(col[ch] + ((alpha * ga[ch] + beta * gb[ch]) + gamma * gc[ch]), 0.0), 255.0);   // a NaN becomes 0
                }
            }
        }
        pr[e] = (unsigned)floor(col[0] + 0.5) & 0xffu;
        pg[e] = (unsigned)floor(col[1] + 0.5) & 0xffu;
        pb[e] = (unsigned)floor(col[2] + 0.5) & 0xffu;
        pv[e] = 1u;
    }
    // twelve bytes r g b r g b ... of four texels as three words, the valid bytes as one (Wt is a multiple of 4: every row starts on a word)
    const long long at = (long long)j * Wq + q;
    texture[at * 3] = pr[0] | (pg[0] << 8) | (pb[0] << 16) | (pr[1] << 24);
    texture[at * 3 + 1] = pg[1] | (pb[1] << 8) | (pr[2] << 16) | (pg[2] << 24);
    texture[at * 3 + 2] = pb[2] | (pr[3] << 8) | (pg[3] << 16) | (pb[3] << 24);
    valid[at] = pv[0] | (pv[1] << 8) | (pv[2] << 16) | (pv[3] << 24);
}

// ================================================================ face map ================================================================
struct CaTri {
    double ax, ay, bx, by, cx, cy, A;
    int i0, i1, j0, j1;                               // the texel box, clamped to the chart's rectangle; empty when i1 < i0 or j1 < j0
};

// the texels floor(lo) - 1 .. ceil(hi) + 1 (the definition's box: rounding can let the edge functions pass a centre just outside [lo, hi]), inside
// [x, x + n): first and last index (a NaN gives an empty or clamped range, never one outside)
__device__ __forceinline__ void ca_span(double lo, double hi, int x, int n, int& first, int& last) {
    first = (int)fmin(fmax(floor(lo) - 1.0, (double)x), (double)(x + n));
    last = (int)fmin(fmax(ceil(hi) + 1.0, (double)(x - 1)), (double)(x + n - 1));
}

__device__ __forceinline__ bool ca_tri(const int* __restrict__ face_chart, const double* __restrict__ screen, long long f, const int* __restrict__ rect,
                                       long long nc, double o, double d, int pad, int Wt, int Ht, CaTri& t) {
    const int c = face_chart[f];
    if (c < 0 || c >= nc) return false;
    const int* r = rect + (long long)c * 6;
    if (r[0] < 0 || r[1] < 0 || r[2] < 1 || r[3] < 1 || r[0] > Wt - r[2] || r[1] > Ht - r[3]) return false;      // a rectangle outside the atlas
    const double* s = screen + f * 6;
    t.ax = ca_coord(r[0], pad, s[0], o, r[4], d), t.ay = ca_coord(r[1], pad, s[1], o, r[5], d);
    t.bx = ca_coord(r[0], pad, s[2], o, r[4], d), t.by = ca_coord(r[1], pad, s[3], o, r[5], d);
    t.cx = ca_coord(r[0], pad, s[4], o, r[4], d), t.cy = ca_coord(r[1], pad, s[5], o, r[5], d);
    t.A = mv_edge(t.ax, t.ay, t.bx, t.by, t.cx, t.cy);
    if (!(t.A != 0.0)) return false;
    ca_span(fmin(fmin(t.ax, t.bx), t.cx), fmax(fmax(t.ax, t.bx), t.cx), r[0], r[2], t.i0, t.i1);
    ca_span(fmin(fmin(t.ay, t.by), t.cy), fmax(fmax(t.ay, t.by), t.cy), r[1], r[3], t.j0, t.j1);
    return t.i1 >= t.i0 && t.j1 >= t.j0;
}

// the texel centre is covered: no edge function opposes the sign of the area (edges inclusive)
__device__ __forceinline__ bool ca_covers(const CaTri& t, int i, int j) {
    const double px = (double)i + 0.5, py = (double)j + 0.5;
    const double wa = mv_edge(t.bx, t.by, t.cx, t.cy, px, py), wb = mv_edge(t.cx, t.cy, t.ax, t.ay, px, py), wc = mv_edge(t.ax, t.ay, t.bx, t.by, px, py);
    return t.A > 0.0 ? (wa >= 0.0 && wb >= 0.0 && wc >= 0.0) : (wa <= 0.0 && wb <= 0.0 && wc <= 0.0);
}

__global__ __launch_bounds__(CA_T) void k_ca_map_fill(int* __restrict__ map, long long n, int v) {
    const long long i = (long long)blockIdx.x * CA_T + threadIdx.x;
    if (i < n) map[i] = v;
}

__global__ __launch_bounds__(CA_T) void k_ca_map_small(const int* __restrict__ face_chart, const double* __restrict__ screen, long long nf,
                                                        const int* __restrict__ rect, long long nc, double o, double d, int pad, int Wt, int Ht, int* map,
                                                        unsigned char* __restrict__ large, ca_u64* hdr) {
    const long long f = (long long)blockIdx.x * CA_T + threadIdx.x;
    if (f >= nf) return;
    CaTri t;
    unsigned char big = 0;
    const int c = face_chart[f];
    if (c < -1 || c >= nc) ca_raise(hdr, MVSDF_TX_ERR_INDEX);
    if (ca_tri(face_chart, screen, f, rect, nc, o, d, pad, Wt, Ht, t)) {
        if ((long long)(t.i1 - t.i0 + 1) * (t.j1 - t.j0 + 1) > MVSDF_CA_LARGE_FACE) {
            big = 1;
        } else {
            for (int j = t.j0; j <= t.j1; ++j)
                for (int i = t.i0; i <= t.i1; ++i)
                    if (ca_covers(t, i, j)) atomicMin(&map[(long long)j * Wt + i], (int)f);
        }
    }
    large[f] = big;
}

// one wave per flagged face, the waves striding over the faces, the lanes over the box
__global__ __launch_bounds__(CA_T) void k_ca_map_large(const int* __restrict__ face_chart, const double* __restrict__ screen, long long nf,
                                                        const int* __restrict__ rect, long long nc, double o, double d, int pad, int Wt, int Ht, int* map,
                                                        const unsigned char* __restrict__ large) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * (CA_T / 64) + (threadIdx.x >> 6), waves = (long long)gridDim.x * (CA_T / 64);
    for (long long f = wave; f < nf; f += waves) {
        if (!large[f]) continue;
        CaTri t;
        if (!ca_tri(face_chart, screen, f, rect, nc, o, d, pad, Wt, Ht, t)) continue;
        const long long bw = t.i1 - t.i0 + 1, n = bw * (t.j1 - t.j0 + 1);
        for (long long k = lane; k < n; k += 64) {
            const int j = t.j0 + (int)(k / bw), i = t.i0 + (int)(k % bw);
            if (ca_covers(t, i, j)) atomicMin(&map[(long long)j * Wt + i], (int)f);
        }
    }
}

// FIRST: the coverage pass left CA_NONE where nobody covers: that becomes -1 before the round looks at it
template <bool FIRST>
__global__ __launch_bounds__(CA_T) void k_ca_dilate(const int* __restrict__ src, int* __restrict__ dst, CaTables T) {
    const long long at = (long long)blockIdx.x * CA_T + threadIdx.x;
    if (at >= (long long)T.Wt * T.Ht) return;
    const int j = (int)(at / T.Wt), i = (int)(at - (long long)j * T.Wt);
    auto get = [&](long long k) {
        const int v = src[k];
        return FIRST && v == CA_NONE ? -1 : v;
    };
    int v = get(at);
    if (v < 0) {
        const int c = ca_owner(T, i, j);
        if (c >= 0) {
            const int* r = T.rect + (long long)c * 6;             // inside the atlas: ca_owner found (i, j) in it, and the neighbours are checked against both
            int best = CA_NONE;
            if (i - 1 >= r[0] && i >= 1) { const int n = get(at - 1); if (n >= 0) best = min(best, n); }
            if (i + 1 < r[0] + r[2] && i + 1 < T.Wt) { const int n = get(at + 1); if (n >= 0) best = min(best, n); }
            if (j - 1 >= r[1] && j >= 1) { const int n = get(at - T.Wt); if (n >= 0) best = min(best, n); }
            if (j + 1 < r[1] + r[3] && j + 1 < T.Ht) { const int n = get(at + T.Wt); if (n >= 0) best = min(best, n); }
            if (best != CA_NONE) v = best;
        }
    }
    dst[at] = v;
}

// ================================================================ entry points ================================================================
static bool ca_tables_ok(const int32_t* rect, const int32_t* order, const int32_t* xs, const int32_t* shelves, int64_t nc, int64_t ns, int64_t Ht, int64_t Wt) {
    return rect && order && xs && shelves && nc >= 1 && nc <= CA_MAX_FACES && ns >= 1 && ns <= nc && Ht >= 1 && Ht <= MVSDF_TX_MAX_SIDE && Wt >= 4 &&
           Wt <= MVSDF_TX_MAX_SIDE && Wt % 4 == 0;
}

extern "C" {

size_t mvsdf_charts_workspace_bytes(int64_t nf, int64_t texels) {
    CaWs w;
    return ca_ws(nf, texels, &w) ? w.total : 0;
}

int mvsdf_charts_face_scores(const float* verts, const float* normals, const int32_t* faces, int64_t nv, int64_t nf, const double* P,
                             const double* centers, int64_t views, int64_t H, int64_t W, double pixel_center, const float* depth, const uint8_t* masks,
                             double depth_tol, double cos_min, int32_t ignore_normals, const int32_t* view, void* ws, size_t ws_bytes, double* score,
                             double* screen, void* stream) {
    const char* what = "mvsdf_charts_face_scores";
    if (!P || !centers || !depth || !ws || ws_bytes < CA_HDR || nv < 0 || nv > INT_MAX || nf < 0 || nf > CA_MAX_FACES ||
        (nf > 0 && (!verts || !normals || !faces || !view || !score || !screen)) || !mv_pixel_center(pixel_center) || !isfinite(depth_tol) ||
        !isfinite(cos_min) || !mv_view_shape(views, H, W))
        return mv_fail(-1, "mvsdf_charts_face_scores: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = mv_check(hipMemsetAsync(ws, 0, CA_HDR, s), what)) return rc;
    ca_u64* hdr = (ca_u64*)ws;
    hipLaunchKernelGGL(k_any_nonfinite<double>, dim3(1), dim3(MV_THREADS), 0, s, P, (long long)views * 16, hdr + MVSDF_CA_H_ERR, (ca_u64)MVSDF_TX_ERR_FINITE);
    hipLaunchKernelGGL(k_any_nonfinite<double>, dim3(1), dim3(MV_THREADS), 0, s, centers, (long long)views * 3, hdr + MVSDF_CA_H_ERR, (ca_u64)MVSDF_TX_ERR_FINITE);
    if (nf > 0)
        hipLaunchKernelGGL(k_ca_scores, dim3(mv_grid(nf, CA_T)), dim3(CA_T), 0, s, verts, normals, faces, (long long)nv, (long long)nf, P, centers, (int)views,
                           pixel_center, (int)H, (int)W, depth, masks, depth_tol, cos_min, (int)ignore_normals, view, score, screen, hdr);
    return mv_check(hipGetLastError(), what);
}

int mvsdf_charts_neighbors(const int32_t* faces, int64_t nv, int64_t nf, void* ws, size_t ws_bytes, int32_t* nbr, void* stream) {
    const char* what = "mvsdf_charts_neighbors";
    CaWs L;
    if (!ws || nv < 0 || nv > INT_MAX || !ca_ws(nf, 0, &L) || (nf > 0 && (!faces || !nbr))) return mv_fail(-1, "mvsdf_charts_neighbors: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_charts_neighbors: workspace too small (mvsdf_charts_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = mv_check(hipMemsetAsync(ws, 0, CA_HDR, s), what)) return rc;
    if (nf > 0) {
        char* w = (char*)ws;
        ca_u64* k[2] = {(ca_u64*)(w + L.k0), (ca_u64*)(w + L.k1)};
        int* v[2] = {(int*)(w + L.v0), (int*)(w + L.v1)};
        const int bits = ca_bits(nv > 0 ? nv - 1 : 0);
        const unsigned gr = mv_grid(L.n3, CA_T);
        hipLaunchKernelGGL(k_ca_edge_keys, dim3(gr), dim3(CA_T), 0, s, faces, (long long)nv, L.n3, bits, k[0], v[0], nbr, (ca_u64*)ws);
        const int cur = ch_radix_sort(k, v, L.n3, 2 * bits, w, L.S, s);
        hipLaunchKernelGGL(k_ca_pairs, dim3(gr), dim3(CA_T), 0, s, (const ca_u64*)k[cur], (const int*)v[cur], L.n3, nbr);
    }
    return mv_check(hipGetLastError(), what);
}

int mvsdf_charts_components(const int32_t* label, const int32_t* nbr, int64_t nf, void* ws, size_t ws_bytes, int32_t* face_chart,
                            int32_t* chart_view, int32_t* chart_faces, void* stream) {
    const char* what = "mvsdf_charts_components";
    CaWs L;
    if (!ws || !ca_ws(nf, 0, &L) || (nf > 0 && (!label || !nbr || !face_chart || !chart_view || !chart_faces)))
        return mv_fail(-1, "mvsdf_charts_components: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_charts_components: workspace too small (mvsdf_charts_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = mv_check(hipMemsetAsync(ws, 0, CA_HDR, s), what)) return rc;
    if (nf == 0) return 0;
    char* w = (char*)ws;
    ca_u64* hdr = (ca_u64*)ws;
    int *parent = (int*)(w + L.parent), *changed = (int*)(w + L.changed);
    const unsigned gr = mv_grid(nf, CA_T);
    if (int rc = mv_check(hipMemsetAsync(changed, 0, (MVSDF_CA_MAX_ROUNDS + 1) * 4, s), what)) return rc;
    hipLaunchKernelGGL(k_ca_parent_init, dim3(gr), dim3(CA_T), 0, s, label, (long long)nf, parent, chart_view, chart_faces, hdr);
    int round = 0, last = 1;
    while (round < MVSDF_CA_MAX_ROUNDS && last) {
        for (int b = 0; b < MVSDF_CA_ROUND_BATCH; ++b, ++round) {
            hipLaunchKernelGGL(k_ca_hook, dim3(gr), dim3(CA_T), 0, s, label, nbr, (long long)nf, parent, changed, round, hdr);
            hipLaunchKernelGGL(k_ca_jump, dim3(gr), dim3(CA_T), 0, s, (long long)nf, parent, (const int*)changed, round);
        }
        if (int rc = mv_check(hipGetLastError(), what)) return rc;
        if (int rc = mv_read(&last, changed + round - 1, 4, s, what)) return rc;
    }
    unsigned char* flags = (unsigned char*)(w + L.flags);
    long long* rank = (long long*)(w + L.rank);
    hipLaunchKernelGGL(k_ca_heads, dim3(gr), dim3(CA_T), 0, s, (const int*)parent, (long long)nf, flags);
    mv_scan((const unsigned char*)flags, (long long)nf, rank, w + L.S.tmp, (long long*)ws + MVSDF_CA_H_CHARTS, s);
    hipLaunchKernelGGL(k_ca_number, dim3(gr), dim3(CA_T), 0, s, label, (const int*)parent, (const long long*)rank, (long long)nf, face_chart, chart_view,
                       chart_faces);
    hipLaunchKernelGGL(k_ca_note, dim3(1), dim3(64), 0, s, hdr, (ca_u64)round, (ca_u64)(last ? MVSDF_TX_ERR_ROUNDS : 0));
    return mv_check(hipGetLastError(), what);
}

int mvsdf_charts_absorb(const float* verts, const float* normals, const int32_t* faces, int64_t nv, int64_t nf, const double* P,
                        const double* centers, int64_t views, int64_t H, int64_t W, double pixel_center, const float* depth, const uint8_t* masks,
                        double depth_tol, double cos_min, int32_t ignore_normals, const int32_t* label, const int32_t* nbr, const int32_t* face_chart,
                        const int32_t* chart_faces, int64_t charts, int64_t min_faces, void* ws, size_t ws_bytes, int32_t* label_out, double* score,
                        double* screen, void* stream) {
    const char* what = "mvsdf_charts_absorb";
    if (!P || !centers || !depth || !ws || ws_bytes < CA_HDR || nv < 0 || nv > INT_MAX || nf < 0 || nf > CA_MAX_FACES || charts < 0 || charts > nf ||
        min_faces < 1 || min_faces > INT_MAX ||
        (nf > 0 && (!verts || !normals || !faces || !label || !nbr || !face_chart || !chart_faces || !label_out || !score || !screen)) ||
        !mv_pixel_center(pixel_center) || !isfinite(depth_tol) || !isfinite(cos_min) || !mv_view_shape(views, H, W))
        return mv_fail(-1, "mvsdf_charts_absorb: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = mv_check(hipMemsetAsync(ws, 0, CA_HDR, s), what)) return rc;
    ca_u64* hdr = (ca_u64*)ws;
    hipLaunchKernelGGL(k_any_nonfinite<double>, dim3(1), dim3(MV_THREADS), 0, s, P, (long long)views * 16, hdr + MVSDF_CA_H_ERR, (ca_u64)MVSDF_TX_ERR_FINITE);
    hipLaunchKernelGGL(k_any_nonfinite<double>, dim3(1), dim3(MV_THREADS), 0, s, centers, (long long)views * 3, hdr + MVSDF_CA_H_ERR, (ca_u64)MVSDF_TX_ERR_FINITE);
    if (nf > 0)
        hipLaunchKernelGGL(k_ca_absorb, dim3(mv_grid(nf, CA_T)), dim3(CA_T), 0, s, verts, normals, faces, (long long)nv, (long long)nf, P, centers, (int)views,
                           pixel_center, (int)H, (int)W, depth, masks, depth_tol, cos_min, (int)ignore_normals, label, nbr, face_chart, chart_faces,
                           (long long)charts, (int)min_faces, label_out, score, screen, hdr);
    return mv_check(hipGetLastError(), what);
}

int mvsdf_charts_pack(const int32_t* face_chart, const double* screen, int64_t nf, int64_t charts, double pixel_center, int64_t H, int64_t W,
                      double density, int32_t pad, void* ws, size_t ws_bytes, int32_t* chart_rect, int32_t* order, int32_t* xs, int32_t* shelves,
                      void* stream) {
    const char* what = "mvsdf_charts_pack";
    CaWs L;
    if (!ws || !ca_ws(nf, 0, &L) || charts < 1 || charts > nf || !face_chart || !screen || !chart_rect || !order || !xs || !shelves ||
        !mv_pixel_center(pixel_center) || !mv_view_shape(1, H, W) || !isfinite(density) || !(density >= 0.0) || !ca_pad(pad))
        return mv_fail(-1, "mvsdf_charts_pack: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_charts_pack: workspace too small (mvsdf_charts_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = mv_check(hipMemsetAsync(ws, 0, CA_HDR, s), what)) return rc;
    char* w = (char*)ws;
    ca_u64* hdr = (ca_u64*)ws;
    const long long nc = charts;
    ca_u64* k[2] = {(ca_u64*)(w + L.k0), (ca_u64*)(w + L.k1)};
    int* v[2] = {(int*)(w + L.v0), (int*)(w + L.v1)};
    int* bounds = (int*)(w + L.bounds);
    long long* pre = (long long*)(w + L.pre);
    const unsigned gc = mv_grid(nc, CA_T);
    hipLaunchKernelGGL(k_ca_bounds_init, dim3(gc), dim3(CA_T), 0, s, nc, bounds);
    hipLaunchKernelGGL(k_ca_bounds, dim3(mv_grid(nf, CA_T)), dim3(CA_T), 0, s, face_chart, screen, (long long)nf, nc, pixel_center, (int)H, (int)W, bounds, hdr);
    hipLaunchKernelGGL(k_ca_sizes, dim3(gc), dim3(CA_T), 0, s, (const int*)bounds, nc, density, (int)pad, chart_rect, k[0], v[0], hdr);
    const int cur = ch_radix_sort(k, v, nc, ca_bits(MVSDF_CA_RECT_CAP), w, L.S, s);
    hipLaunchKernelGGL(k_ca_widths, dim3(gc), dim3(CA_T), 0, s, (const int*)v[cur], (const int*)chart_rect, nc, pre);
    mv_scan((const long long*)pre, nc, pre, w + L.S.tmp, pre + nc, s);
    hipLaunchKernelGGL(k_ca_shelves, dim3(1), dim3(64), 0, s, (const long long*)pre, (const int*)v[cur], (const int*)chart_rect, nc, shelves, hdr);
    hipLaunchKernelGGL(k_ca_place, dim3(gc), dim3(CA_T), 0, s, (const long long*)pre, (const int*)v[cur], nc, (const int*)shelves, (const ca_u64*)hdr,
                       chart_rect, order, xs);
    return mv_check(hipGetLastError(), what);
}

int mvsdf_charts_uv(const int32_t* face_chart, const double* screen, int64_t nf, const int32_t* chart_rect, int64_t charts, double pixel_center,
                    double density, int32_t pad, int64_t Ht, int64_t Wt, void* ws, size_t ws_bytes, float* uv, void* stream) {
    const char* what = "mvsdf_charts_uv";
    if (!ws || ws_bytes < CA_HDR || nf < 0 || nf > CA_MAX_FACES || charts < 0 || charts > nf || (charts > 0 && !chart_rect) ||
        (nf > 0 && (!face_chart || !screen || !uv)) || !mv_pixel_center(pixel_center) || !isfinite(density) || !(density >= 0.0) || !ca_pad(pad) || Ht < 1 ||
        Wt < 1 || Ht > MVSDF_TX_MAX_SIDE || Wt > MVSDF_TX_MAX_SIDE)
        return mv_fail(-1, "mvsdf_charts_uv: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = mv_check(hipMemsetAsync(ws, 0, CA_HDR, s), what)) return rc;
    if (nf > 0)
        hipLaunchKernelGGL(k_ca_uv, dim3(mv_grid(nf, CA_T)), dim3(CA_T), 0, s, face_chart, screen, (long long)nf, chart_rect, (long long)charts, pixel_center,
                           density, (int)pad, (double)Wt, (double)Ht, uv, (ca_u64*)ws);
    return mv_check(hipGetLastError(), what);
}

int mvsdf_charts_face_map(const int32_t* face_chart, const double* screen, int64_t nf, double pixel_center, const int32_t* chart_rect,
                          const int32_t* order, const int32_t* xs, const int32_t* shelves, int64_t charts, int64_t nshelves, double density,
                          int32_t pad, int64_t Ht, int64_t Wt, void* ws, size_t ws_bytes, int32_t* face_map, void* stream) {
    const char* what = "mvsdf_charts_face_map";
    CaWs L;
    if (!ws || !face_map || !face_chart || !screen || !ca_tables_ok(chart_rect, order, xs, shelves, charts, nshelves, Ht, Wt) || charts > nf ||
        !ca_ws(nf, Ht * Wt, &L) || !mv_pixel_center(pixel_center) || !isfinite(density) || !(density >= 0.0) || !ca_pad(pad))
        return mv_fail(-1, "mvsdf_charts_face_map: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_charts_face_map: workspace too small (mvsdf_charts_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = mv_check(hipMemsetAsync(ws, 0, CA_HDR, s), what)) return rc;
    char* w = (char*)ws;
    const long long n = (long long)Ht * Wt;
    int* buf[2] = {face_map, (int*)(w + L.map2)};
    int cur = pad & 1;                                            // `pad` rounds flip the buffer: the last one lands in face_map
    unsigned char* large = (unsigned char*)(w + L.flags);
    const CaTables T = {chart_rect, order, xs, shelves, (int)charts, (int)nshelves, (int)Wt, (int)Ht};
    hipLaunchKernelGGL(k_ca_map_fill, dim3(mv_grid(n, CA_T)), dim3(CA_T), 0, s, buf[cur], n, CA_NONE);
    hipLaunchKernelGGL(k_ca_map_small, dim3(mv_grid(nf, CA_T)), dim3(CA_T), 0, s, face_chart, screen, (long long)nf, chart_rect, (long long)charts,
                       pixel_center, density, (int)pad, (int)Wt, (int)Ht, buf[cur], large, (ca_u64*)ws);
    const long long waves = mv_ceil_div(nf, CA_T / 64 * 16);      // up to 16 faces a wave before the grid is capped
    hipLaunchKernelGGL(k_ca_map_large, dim3((unsigned)(waves < CA_LARGE_BLOCKS ? (waves > 0 ? waves : 1) : CA_LARGE_BLOCKS)), dim3(CA_T), 0, s, face_chart,
                       screen, (long long)nf, chart_rect, (long long)charts, pixel_center, density, (int)pad, (int)Wt, (int)Ht, buf[cur],
                       (const unsigned char*)large);
    for (int r = 0; r < pad; ++r, cur ^= 1) {
        if (r == 0)
            hipLaunchKernelGGL(k_ca_dilate<true>, dim3(mv_grid(n, CA_T)), dim3(CA_T), 0, s, (const int*)buf[cur], buf[cur ^ 1], T);
        else
            hipLaunchKernelGGL(k_ca_dilate<false>, dim3(mv_grid(n, CA_T)), dim3(CA_T), 0, s, (const int*)buf[cur], buf[cur ^ 1], T);
    }
    return mv_check(hipGetLastError(), what);
}

int mvsdf_charts_fill(const uint8_t* images, int64_t views, int64_t H, int64_t W, const int32_t* chart_view, const int32_t* chart_rect,
                      const int32_t* order, const int32_t* xs, const int32_t* shelves, int64_t charts, int64_t nshelves, double density, int32_t pad,
                      int32_t fallback_r, int32_t fallback_g, int32_t fallback_b, int64_t Ht, int64_t Wt, const int32_t* face_map,
                      const int32_t* face_chart, const double* screen, double pixel_center, int64_t nf, const int32_t* corner_node, const double* g,
                      int64_t nodes, void* ws, size_t ws_bytes, uint8_t* texture, uint8_t* valid, void* stream) {
    const char* what = "mvsdf_charts_fill";
    const bool level = face_map != nullptr;
    if (!images || !texture || !valid || !chart_view || !ws || ws_bytes < CA_HDR || !mv_view_shape(views, H, W) ||
        !ca_tables_ok(chart_rect, order, xs, shelves, charts, nshelves, Ht, Wt) || !isfinite(density) || !(density > 0.0) || !ca_pad(pad) || fallback_r < 0 ||
        fallback_r > 255 || fallback_g < 0 || fallback_g > 255 || fallback_b < 0 || fallback_b > 255 ||
        (level && (!face_chart || !screen || !corner_node || nf < 1 || nf > CA_MAX_FACES || nodes < 0 || nodes > 3 * CA_MAX_FACES || (nodes > 0 && !g) ||
                   !mv_pixel_center(pixel_center))))
        return mv_fail(-1, "mvsdf_charts_fill: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = mv_check(hipMemsetAsync(ws, 0, CA_HDR, s), what)) return rc;
    const CaTables T = {chart_rect, order, xs, shelves, (int)charts, (int)nshelves, (int)Wt, (int)Ht};
    const CaLevel L = {face_map, face_chart, corner_node, screen, g, pixel_center, (long long)nf, (long long)nodes};
    const dim3 grid(mv_grid(Wt / 4, CA_T), (unsigned)Ht);
    if (level)
        hipLaunchKernelGGL((k_ca_fill<true>), grid, dim3(CA_T), 0, s, images, (int)views, (int)H, (int)W, chart_view, T, density, (int)pad, (unsigned)fallback_r,
                           (unsigned)fallback_g, (unsigned)fallback_b, L, (unsigned*)texture, (unsigned*)valid, (ca_u64*)ws);
    else
        hipLaunchKernelGGL((k_ca_fill<false>), grid, dim3(CA_T), 0, s, images, (int)views, (int)H, (int)W, chart_view, T, density, (int)pad, (unsigned)fallback_r,
                           (unsigned)fallback_g, (unsigned)fallback_b, L, (unsigned*)texture, (unsigned*)valid, (ca_u64*)ws);
    return mv_check(hipGetLastError(), what);
}

}  // extern "C"
