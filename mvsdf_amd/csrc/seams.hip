// seams.hip -- global seam levelling of a texture atlas: an additive colour correction g per (vertex, label) node, chosen so that the corrected
// colours agree where labels meet and vary smoothly inside a label's region.  Python: mvsdf_amd/seams.py, which states the definition;
// tests/seams_ref.py restates it in numpy.  All arithmetic is fp64 without contraction, in the order the definition writes it; sums run in list
// order or over geom_prims.h's canonical tree; the only atomics are integer ones (error bits).  No result depends on the schedule.
//
// * Nodes: one key (vertex, view) per face corner (unlabelled corners get a sentinel past every vertex), nn_tree.h's stable radix sort with the
//   corner slot 3 f + e as the value, segment heads, geom_prims.h's scan: the rank of a head is the node id, listed by (vertex, view) ascending.
//   Because the sort is stable a node's corner slots stand together in (face, corner) order: they ARE its smoothness entries' owners, so the one
//   sort builds the whole graph.  The nodes of a vertex stand together too: they are each other's seam partners.
// * k_sl_degree / k_sl_emit: one lane per node; the list lengths are scanned (mv_scan) into the CSR offsets.
// * k_sl_colors: one lane per node, view_prims.h's mv_project, mv_cell and mv_gather_rgb.
// * A x (sl_apply): one lane per node, a gather over its list, three channels in registers.
// * The solve: Jacobi-preconditioned conjugate gradients, three channels side by side, the state in the header (MVSDF_SL_H_*), every dot product
//   over the canonical tree (k_sl_tree, a level per launch, grid.y = channel).  A whole solve is enqueued without a host wait; once a channel is done
//   its part of every launch is a flag-reading no-op.
// * The levelled fill is texture.hip's k_tx_fill with its LEVEL flag (mvsdf_seams_fill is defined there).
//
// Every index read from memory (face -> vertex, label -> view, node -> vertex / view, adjacency offsets and entries) is range-checked before it
// becomes an address.
#include "nn_tree.h"
#include "view_prims.h"

#define SL_T 256
#define SL_HDR 256                                    // bytes at the start of the workspace: MVSDF_SL_H_*
static_assert(MVSDF_SL_H_WORDS * 8 <= SL_HDR && MVSDF_SL_H_WORDS <= 32, "the result words fit the header");
static_assert(SL_T == MV_THREADS, "the chunk of geom_prims.h's tree");
#define SL_MAX_FACES (1ll << MVSDF_TX_MAX_FACES_LOG2)

__device__ __forceinline__ double sl_get(const long long* st, int w) { return __longlong_as_double(st[w]); }
__device__ __forceinline__ void sl_put(long long* st, int w, double v) { st[w] = __double_as_longlong(v); }
__device__ __forceinline__ void sl_raise(long long* st, long long bit) { atomicOr((unsigned long long*)st + MVSDF_SL_H_ERR, (unsigned long long)bit); }

static int sl_bits(long long x) {                     // the bits that hold 0 .. x
    int b = 1;
    while (b < 62 && (1ll << b) <= x) ++b;
    return b;
}

// ================================================================ the workspaces ================================================================
struct SlGraphWs {
    long long n3;                                     // corner slots
    int bv, bits;                                     // bits of a view, of a key
    size_t k0, k1, v0, v1, flags, rank, nvert, nview, npos, nend, deg, total;
    ChSortLayout S;
};

static bool sl_graph_ws(long long nf, long long nv, long long views, SlGraphWs* w) {
    if (nf < 0 || nf > SL_MAX_FACES || nv < 0 || nv > INT_MAX || views < 1 || views > MVSDF_RA_MAX_VIEWS) return false;
    const long long n = 3 * nf, m = n > 0 ? n : 1;
    w->n3 = n;
    w->bv = sl_bits(views - 1);
    w->bits = w->bv + sl_bits(nv);
    WsCursor c{SL_HDR};
    w->k0 = c.take((size_t)m * 8);
    w->k1 = c.take((size_t)m * 8);
    w->v0 = c.take((size_t)m * 4);
    w->v1 = c.take((size_t)m * 4);
    w->flags = c.take((size_t)m);
    w->rank = c.take((size_t)m * 8);
    w->nvert = c.take((size_t)m * 4);
    w->nview = c.take((size_t)m * 4);
    w->npos = c.take((size_t)m * 4);
    w->nend = c.take((size_t)m * 4);
    w->deg = c.take((size_t)m * 8);
    ch_sort_layout(m, m, c, &w->S);
    w->total = c.o;
    return true;
}

#define SL_MAX_LEVELS 4
struct SlSolveWs {
    size_t r, p, q, d, terms, level[SL_MAX_LEVELS], total;
    long long n[SL_MAX_LEVELS + 1];                   // n[0] = K values per channel, n[l + 1] = the chunks of level l; the last is 1
    int levels;
};

static bool sl_solve_ws(long long K, SlSolveWs* w) {
    if (K < 0 || K > 3 * SL_MAX_FACES) return false;
    const long long m = K > 0 ? K : 1;
    WsCursor c{SL_HDR};
    w->r = c.take((size_t)m * 24);
    w->p = c.take((size_t)m * 24);
    w->q = c.take((size_t)m * 24);
    w->d = c.take((size_t)m * 8);
    w->terms = c.take((size_t)m * 24);
    w->n[0] = m;
    w->levels = 0;
    do {
        if (w->levels >= SL_MAX_LEVELS) return false;
        w->n[w->levels + 1] = mv_ceil_div(w->n[w->levels], MV_CHUNK);
        w->level[w->levels] = c.take((size_t)w->n[w->levels + 1] * 24);
        ++w->levels;
    } while (w->n[w->levels] > 1);
    w->total = c.o;
    return true;
}

// ================================================================ nodes ================================================================
// slot j = 3 f + e: key = vertex << bv | view of a labelled corner, nv << bv (past every node) otherwise
static __global__ __launch_bounds__(SL_T) void k_sl_keys(const int* __restrict__ faces, const int* __restrict__ label, long long nv, long long n3,
                                                         int V, int bv, unsigned long long* __restrict__ key, int* __restrict__ val, long long* st) {
    const long long j = (long long)blockIdx.x * SL_T + threadIdx.x;
    if (j >= n3) return;
    const long long f = j / 3;
    const int a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2], v = label[f];
    bool ok = true;
    if (a < 0 || b < 0 || c < 0 || a >= nv || b >= nv || c >= nv) {
        sl_raise(st, MVSDF_TX_ERR_INDEX);
        ok = false;
    }
    if (v < -1 || v >= V) {
        sl_raise(st, MVSDF_TX_ERR_LABEL);
        ok = false;
    }
    const int i = faces[j];
    key[j] = ok && v >= 0 ? ((unsigned long long)i << bv) | (unsigned long long)v : (unsigned long long)nv << bv;
    val[j] = (int)j;
}

static __global__ __launch_bounds__(SL_T) void k_sl_heads(const unsigned long long* __restrict__ key, long long n3, unsigned long long none,
                                                          unsigned char* __restrict__ flags) {
    const long long j = (long long)blockIdx.x * SL_T + threadIdx.x;
    if (j >= n3) return;
    const unsigned long long k = key[j];
    flags[j] = k < none && (j == 0 || key[j - 1] != k) ? 1 : 0;
}

// rank[j] = the heads before j: the node of slot j is rank[j] + flags[j] - 1
static __global__ __launch_bounds__(SL_T) void k_sl_nodes(const unsigned long long* __restrict__ key, const int* __restrict__ val,
                                                          const unsigned char* __restrict__ flags, const long long* __restrict__ rank, long long n3,
                                                          unsigned long long none, int bv, int* __restrict__ nvert, int* __restrict__ nview,
                                                          int* __restrict__ npos, int* __restrict__ nend, int* __restrict__ corner_node) {
    const long long j = (long long)blockIdx.x * SL_T + threadIdx.x;
    if (j >= n3) return;
    const unsigned long long k = key[j];
    const int slot = val[j];
    if (slot < 0 || slot >= n3) return;                           // cannot happen: the sort permutes 0 .. n3 - 1
    if (!(k < none)) {
        corner_node[slot] = -1;
        return;
    }
    const long long id = rank[j] + flags[j] - 1;
    if (id < 0 || id >= n3) return;                               // cannot happen: slot 0 of a labelled run is a head
    corner_node[slot] = (int)id;
    if (flags[j]) {
        nvert[id] = (int)(k >> bv);
        nview[id] = (int)(k & ((1ull << bv) - 1));
        npos[id] = (int)j;
    }
    if (j == n3 - 1 || key[j + 1] != k) nend[id] = (int)(j + 1);
}

// the nodes of k's vertex: [lo, hi)
__device__ __forceinline__ void sl_group(const int* __restrict__ nvert, long long K, long long k, long long& lo, long long& hi) {
    const int i = nvert[k];
    lo = k;
    hi = k + 1;
    while (lo > 0 && nvert[lo - 1] == i) --lo;
    while (hi < K && nvert[hi] == i) ++hi;
}

// deg[k] = seam partners + two entries per corner slot (0 past the last node: the scan runs over all n3 words)
static __global__ __launch_bounds__(SL_T) void k_sl_degree(const int* __restrict__ nvert, const int* __restrict__ npos, const int* __restrict__ nend,
                                                           long long n3, const long long* __restrict__ st, long long* __restrict__ deg) {
    const long long k = (long long)blockIdx.x * SL_T + threadIdx.x;
    if (k >= n3) return;
    const long long K = st[MVSDF_SL_H_NODES];
    long long d = 0;
    if (k < K && K <= n3) {
        long long lo, hi;
        sl_group(nvert, K, k, lo, hi);
        d = (hi - lo - 1) + 2 * (long long)(nend[k] - npos[k]);
    }
    deg[k] = d;
}

// off: deg after its scan.  Nothing is written unless K and nnz are the header's.
static __global__ __launch_bounds__(SL_T) void k_sl_emit(const int* __restrict__ val, const int* __restrict__ nvert, const int* __restrict__ nview,
                                                         const int* __restrict__ npos, const int* __restrict__ nend, const long long* __restrict__ off,
                                                         long long n3, long long K, long long nnz, const int* __restrict__ corner_node,
                                                         long long* st, int* __restrict__ node_vertex, int* __restrict__ node_view,
                                                         long long* __restrict__ adj_off, int* __restrict__ adj_seam, int* __restrict__ adj_node) {
    const long long k = (long long)blockIdx.x * SL_T + threadIdx.x;
    if (k >= K) return;
    if (st[MVSDF_SL_H_NODES] != K || st[MVSDF_SL_H_NNZ] != nnz || K > n3) {
        if (k == 0) sl_raise(st, MVSDF_TX_ERR_COUNTS);
        return;
    }
    long long lo, hi;
    sl_group(nvert, K, k, lo, hi);
    const long long j0 = npos[k], j1 = nend[k];
    long long at = off[k];
    if (at < 0 || j0 < 0 || j1 < j0 || j1 > n3 || at + (hi - lo - 1) + 2 * (j1 - j0) > nnz) {
        sl_raise(st, MVSDF_TX_ERR_COUNTS);
        return;
    }
    node_vertex[k] = nvert[k];
    node_view[k] = nview[k];
    adj_off[k] = at;
    if (k == K - 1) adj_off[K] = nnz;
    adj_seam[k] = (int)(hi - lo - 1);
    for (long long g = lo; g < hi; ++g)
        if (g != k) adj_node[at++] = (int)g;
    for (long long j = j0; j < j1; ++j) {
        const int slot = val[j];
        int n1 = -1, n2 = -1;
        if (slot >= 0 && slot < n3) {
            const int f = slot / 3, e = slot - 3 * f;
            n1 = corner_node[f * 3 + (e + 1) % 3];
            n2 = corner_node[f * 3 + (e + 2) % 3];
        }
        if (n1 < 0 || n2 < 0 || n1 >= K || n2 >= K) {             // corner_node is not what mvsdf_seams_nodes wrote
            sl_raise(st, MVSDF_TX_ERR_COUNTS);
            n1 = n2 = (int)k;
        }
        adj_node[at++] = n1;
        adj_node[at++] = n2;
    }
}

// ================================================================ node colours ================================================================
static __global__ __launch_bounds__(SL_T) void k_sl_colors(const int* __restrict__ node_vertex, const int* __restrict__ node_view, long long K,
                                                           const float* __restrict__ verts, long long nv, const double* __restrict__ P, int V, int H,
                                                           int W, double o, const unsigned char* __restrict__ images, double* __restrict__ f,
                                                           long long* st) {
    const long long k = (long long)blockIdx.x * SL_T + threadIdx.x;
    if (k >= K) return;
    const int i = node_vertex[k], v = node_view[k];
    double col[3] = {0.0, 0.0, 0.0};
    if (i < 0 || i >= nv) {
        sl_raise(st, MVSDF_TX_ERR_INDEX);
    } else if (v < 0 || v >= V) {
        sl_raise(st, MVSDF_TX_ERR_LABEL);
    } else {
        const float* X = verts + (long long)i * 3;
        if (!(isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]))) sl_raise(st, MVSDF_TX_ERR_FINITE);
        double sx = 0.0, sy = 0.0, z;
        double u = 0.0, t = 0.0;                                  // a vertex that is not in front reads the image at (0, 0)
        if (mv_project(P + (long long)v * 16, X, sx, sy, z)) {
            u = fmin(fmax(sx - o, 0.0), (double)(W - 1));         // a NaN becomes 0: always an address inside
            t = fmin(fmax(sy - o, 0.0), (double)(H - 1));
        }
        mv_gather_rgb(images, (long long)v * H * W, W, mv_cell(u, t, W, H), col);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) f[k * 3 + c] = col[c];
}

// ================================================================ the operator ================================================================
struct SlGraph {
    const long long* off;
    const int* seam;
    const int* node;
    long long K, nnz;
};

struct SlList {
    long long lo, mid, hi;
};

// node k's list; an offset or a seam count that does not fit raises MVSDF_TX_ERR_INDEX and gives the empty list
__device__ __forceinline__ SlList sl_list(const SlGraph& G, long long k, long long* st) {
    const long long lo = G.off[k], hi = G.off[k + 1];
    const long long sc = G.seam[k];
    if (lo < 0 || hi < lo || hi > G.nnz || sc < 0 || sc > hi - lo) {
        sl_raise(st, MVSDF_TX_ERR_INDEX);
        return {0, 0, 0};
    }
    return {lo, lo + sc, hi};
}

// out = (A x)_k: anchor * x_k + the sum from 0.0, in list order, of w * (x_k - x_nb)
__device__ __forceinline__ void sl_apply(const SlGraph& G, const double* __restrict__ x, long long k, double smooth, double anchor, double* out,
                                         long long* st) {
    const SlList L = sl_list(G, k, st);
    const double x0 = x[k * 3], x1 = x[k * 3 + 1], x2 = x[k * 3 + 2];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (long long e = L.lo; e < L.hi; ++e) {
        const int nb = G.node[e];
        if (nb < 0 || nb >= G.K) {
            sl_raise(st, MVSDF_TX_ERR_INDEX);
            continue;
        }
        const double w = e < L.mid ? 1.0 : smooth;
        const double* __restrict__ y = x + (long long)nb * 3;
        a0 = a0 + w * (x0 - y[0]);
        a1 = a1 + w * (x1 - y[1]);
        a2 = a2 + w * (x2 - y[2]);
    }
    out[0] = anchor * x0 + a0;
    out[1] = anchor * x1 + a1;
    out[2] = anchor * x2 + a2;
}

static __global__ __launch_bounds__(SL_T) void k_sl_apply(SlGraph G, const double* __restrict__ x, double smooth, double anchor,
                                                          double* __restrict__ out, long long* st) {
    const long long k = (long long)blockIdx.x * SL_T + threadIdx.x;
    if (k >= G.K) return;
    double o[3];
    sl_apply(G, x, k, smooth, anchor, o, st);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[k * 3 + c] = o[c];
}

// ================================================================ the tree ================================================================
// out[c * out_stride + b] = the tree sum of chunk b of in[c * in_stride .. + n); grid (chunks, 3); guard: nothing for a channel that is done
static __global__ __launch_bounds__(SL_T) void k_sl_tree(const double* __restrict__ in, long long n, long long in_stride, double* __restrict__ out,
                                                         long long out_stride, const long long* __restrict__ st, int guard) {
    __shared__ double sh[SL_T];
    const int c = blockIdx.y;
    if (guard && st[MVSDF_SL_H_DONE + c]) return;
    const long long base = (long long)blockIdx.x * MV_CHUNK + (long long)threadIdx.x * MV_ITEMS;
    const double* __restrict__ src = in + c * in_stride;
    double a[MV_ITEMS];
#pragma unroll
    for (int q = 0; q < MV_ITEMS; ++q) a[q] = base + q < n ? src[base + q] : 0.0;
    const double v = mv_tree_chunk(a, sh);
    if (threadIdx.x == 0) out[c * out_stride + blockIdx.x] = v;
}

// ================================================================ the solve ================================================================
struct SlCg {
    double *x, *r, *p, *q, *d, *terms;
    long long* st;
};

__device__ __forceinline__ bool sl_all_done(const long long* st) {
    return st[MVSDF_SL_H_DONE] && st[MVSDF_SL_H_DONE + 1] && st[MVSDF_SL_H_DONE + 2];
}

// a channel takes part in this iteration's updates: not done, and sigma = p . A p finite and > 0
__device__ __forceinline__ bool sl_live(const long long* st, int c) {
    const double sigma = sl_get(st, MVSDF_SL_H_SIGMA + c);
    return !st[MVSDF_SL_H_DONE + c] && sigma > 0.0 && isfinite(sigma);
}

// d = anchor + the sum of w; r = b; p = z = r / d; x = 0; terms = r z
static __global__ __launch_bounds__(SL_T) void k_sl_init(SlGraph G, const double* __restrict__ f, double smooth, double anchor, SlCg S) {
    const long long k = (long long)blockIdx.x * SL_T + threadIdx.x;
    if (k >= G.K) return;
    const SlList L = sl_list(G, k, S.st);
    const double f0 = f[k * 3], f1 = f[k * 3 + 1], f2 = f[k * 3 + 2];
    double s = 0.0, b[3] = {0.0, 0.0, 0.0};
    for (long long e = L.lo; e < L.hi; ++e) {
        const int nb = G.node[e];
        if (nb < 0 || nb >= G.K) {
            sl_raise(S.st, MVSDF_TX_ERR_INDEX);
            continue;
        }
        s = s + (e < L.mid ? 1.0 : smooth);
        if (e < L.mid) {
            const double* __restrict__ y = f + (long long)nb * 3;
            b[0] = b[0] + (y[0] - f0);
            b[1] = b[1] + (y[1] - f1);
            b[2] = b[2] + (y[2] - f2);
        }
    }
    const double d = anchor + s;
    S.d[k] = d;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double z = b[c] / d;
        S.x[k * 3 + c] = 0.0;
        S.r[k * 3 + c] = b[c];
        S.p[k * 3 + c] = z;
        S.q[k * 3 + c] = 0.0;
        S.terms[c * G.K + k] = b[c] * z;
    }
}

// after the tree left rho in the header: rho0 = rho, no iterations yet, done at once unless rho0 is finite and > 0
static __global__ void k_sl_begin(long long* st) {
    const int c = threadIdx.x;
    if (c >= 3) return;
    const double rho = sl_get(st, MVSDF_SL_H_RHO + c);
    st[MVSDF_SL_H_RHO0 + c] = st[MVSDF_SL_H_RHO + c];
    st[MVSDF_SL_H_ITERS + c] = 0;
    st[MVSDF_SL_H_SIGMA + c] = 0;
    st[MVSDF_SL_H_RHON + c] = 0;
    st[MVSDF_SL_H_DONE + c] = (rho > 0.0 && isfinite(rho)) ? 0 : 1;
}

// q = A p, terms = p q
static __global__ __launch_bounds__(SL_T) void k_sl_apq(SlGraph G, double smooth, double anchor, SlCg S) {
    const long long k = (long long)blockIdx.x * SL_T + threadIdx.x;
    if (k >= G.K || sl_all_done(S.st)) return;
    double o[3];
    sl_apply(G, S.p, k, smooth, anchor, o, S.st);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (S.st[MVSDF_SL_H_DONE + c]) continue;
        S.q[k * 3 + c] = o[c];
        S.terms[c * G.K + k] = S.p[k * 3 + c] * o[c];
    }
}

// alpha = rho / sigma; x += alpha p; r -= alpha q; terms = r (r / d)
static __global__ __launch_bounds__(SL_T) void k_sl_update(long long K, SlCg S) {
    const long long k = (long long)blockIdx.x * SL_T + threadIdx.x;
    if (k >= K || sl_all_done(S.st)) return;
    const double d = S.d[k];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (!sl_live(S.st, c)) continue;
        const double alpha = sl_get(S.st, MVSDF_SL_H_RHO + c) / sl_get(S.st, MVSDF_SL_H_SIGMA + c);
        const long long at = k * 3 + c;
        S.x[at] = S.x[at] + alpha * S.p[at];
        const double r = S.r[at] - alpha * S.q[at];
        S.r[at] = r;
        S.terms[c * K + k] = r * (r / d);
    }
}

// beta = rho' / rho; p = r / d + beta p
static __global__ __launch_bounds__(SL_T) void k_sl_direction(long long K, SlCg S) {
    const long long k = (long long)blockIdx.x * SL_T + threadIdx.x;
    if (k >= K || sl_all_done(S.st)) return;
    const double d = S.d[k];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (!sl_live(S.st, c)) continue;
        const double beta = sl_get(S.st, MVSDF_SL_H_RHON + c) / sl_get(S.st, MVSDF_SL_H_RHO + c);
        const long long at = k * 3 + c;
        S.p[at] = S.r[at] / d + beta * S.p[at];
    }
}

// the end of an iteration, one lane per channel
static __global__ void k_sl_step(long long* st, double tol2) {
    const int c = threadIdx.x;
    if (c >= 3 || st[MVSDF_SL_H_DONE + c]) return;
    if (!sl_live(st, c)) {
        st[MVSDF_SL_H_DONE + c] = 1;
        return;
    }
    const double rhon = sl_get(st, MVSDF_SL_H_RHON + c);
    st[MVSDF_SL_H_RHO + c] = st[MVSDF_SL_H_RHON + c];
    st[MVSDF_SL_H_ITERS + c] += 1;
    st[MVSDF_SL_H_DONE + c] = rhon > tol2 * sl_get(st, MVSDF_SL_H_RHO0 + c) ? 0 : 1;
}

// the tree sums of terms[3][K] into the three header words from `word`
static void sl_dots(const SlSolveWs& L, char* w, int word, int guard, hipStream_t s) {
    const double* in = (const double*)(w + L.terms);
    for (int l = 0; l < L.levels; ++l) {
        const bool last = l == L.levels - 1;
        double* out = last ? (double*)w + word : (double*)(w + L.level[l]);
        hipLaunchKernelGGL(k_sl_tree, dim3((unsigned)L.n[l + 1], 3), dim3(SL_T), 0, s, in, L.n[l], L.n[l], out, last ? 1ll : L.n[l + 1],
                           (const long long*)w, guard);
        in = out;
    }
}

static bool sl_graph_args(const int64_t* adj_off, const int32_t* adj_seam, const int32_t* adj_node, int64_t nodes, int64_t nnz) {
    return nodes >= 0 && nodes <= 3 * SL_MAX_FACES && nnz >= 0 && (nodes == 0 || (adj_off && adj_seam)) && (nnz == 0 || adj_node);
}

extern "C" {

size_t mvsdf_seams_workspace_bytes(int64_t nf, int64_t nv, int64_t views, int64_t nodes) {
    SlGraphWs g;
    SlSolveWs c;
    if (!sl_graph_ws(nf, nv, views, &g) || !sl_solve_ws(nodes, &c)) return 0;
    return g.total > c.total ? g.total : c.total;
}

int mvsdf_seams_nodes(const int32_t* faces, const int32_t* label, int64_t nv, int64_t nf, int64_t views, void* ws, size_t ws_bytes,
                      int32_t* corner_node, void* stream) {
    const char* what = "mvsdf_seams_nodes";
    SlGraphWs L;
    if (!ws || !sl_graph_ws(nf, nv, views, &L) || (nf > 0 && (!faces || !label || !corner_node))) return mv_fail(-1, "mvsdf_seams_nodes: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_seams_nodes: workspace too small (mvsdf_seams_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)ws;
    long long* st = (long long*)ws;
    if (int rc = mv_check(hipMemsetAsync(ws, 0, SL_HDR, s), what)) return rc;
    if (nf > 0) {
        const long long n3 = L.n3;
        const unsigned gr = mv_grid(n3, SL_T);
        unsigned long long* k[2] = {(unsigned long long*)(w + L.k0), (unsigned long long*)(w + L.k1)};
        int* v[2] = {(int*)(w + L.v0), (int*)(w + L.v1)};
        const unsigned long long none = (unsigned long long)nv << L.bv;
        hipLaunchKernelGGL(k_sl_keys, dim3(gr), dim3(SL_T), 0, s, faces, label, (long long)nv, n3, (int)views, L.bv, k[0], v[0], st);
        const int cur = ch_radix_sort(k, v, n3, L.bits, w, L.S, s);
        unsigned char* flags = (unsigned char*)(w + L.flags);
        long long* rank = (long long*)(w + L.rank);
        long long* deg = (long long*)(w + L.deg);
        int *nvert = (int*)(w + L.nvert), *nview = (int*)(w + L.nview), *npos = (int*)(w + L.npos), *nend = (int*)(w + L.nend);
        hipLaunchKernelGGL(k_sl_heads, dim3(gr), dim3(SL_T), 0, s, (const unsigned long long*)k[cur], n3, none, flags);
        mv_scan((const unsigned char*)flags, n3, rank, w + L.S.tmp, st + MVSDF_SL_H_NODES, s);
        hipLaunchKernelGGL(k_sl_nodes, dim3(gr), dim3(SL_T), 0, s, (const unsigned long long*)k[cur], (const int*)v[cur], (const unsigned char*)flags,
                           (const long long*)rank, n3, none, L.bv, nvert, nview, npos, nend, corner_node);
        hipLaunchKernelGGL(k_sl_degree, dim3(gr), dim3(SL_T), 0, s, (const int*)nvert, (const int*)npos, (const int*)nend, n3, (const long long*)st, deg);
        mv_scan((const long long*)deg, n3, deg, w + L.S.tmp, st + MVSDF_SL_H_NNZ, s);
    }
    return mv_check(hipGetLastError(), what);
}

int mvsdf_seams_graph(int64_t nv, int64_t nf, int64_t views, int64_t nodes, int64_t nnz, const int32_t* corner_node, void* ws, size_t ws_bytes,
                      int32_t* node_vertex, int32_t* node_view, int64_t* adj_off, int32_t* adj_seam, int32_t* adj_node, void* stream) {
    const char* what = "mvsdf_seams_graph";
    SlGraphWs L;
    if (!ws || !sl_graph_ws(nf, nv, views, &L) || nodes < 0 || nodes > L.n3 || nnz < 0 || !adj_off ||
        (nodes > 0 && (!corner_node || !node_vertex || !node_view || !adj_seam)) || (nnz > 0 && !adj_node))
        return mv_fail(-1, "mvsdf_seams_graph: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_seams_graph: workspace too small (mvsdf_seams_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)ws;
    if (nodes == 0) {
        if (int rc = mv_check(hipMemsetAsync(adj_off, 0, 8, s), what)) return rc;
        return mv_check(hipGetLastError(), what);
    }
    const int cur = ch_sort_passes(L.bits) % 2;                    // where mvsdf_seams_nodes's sort ended
    hipLaunchKernelGGL(k_sl_emit, dim3(mv_grid(nodes, SL_T)), dim3(SL_T), 0, s, (const int*)(w + (cur ? L.v1 : L.v0)), (const int*)(w + L.nvert),
                       (const int*)(w + L.nview), (const int*)(w + L.npos), (const int*)(w + L.nend), (const long long*)(w + L.deg), L.n3,
                       (long long)nodes, (long long)nnz, corner_node, (long long*)ws, node_vertex, node_view, (long long*)adj_off, adj_seam, adj_node);
    return mv_check(hipGetLastError(), what);
}

int mvsdf_seams_colors(const int32_t* node_vertex, const int32_t* node_view, int64_t nodes, const float* verts, int64_t nv, const double* P,
                       int64_t views, int64_t H, int64_t W, double pixel_center, const uint8_t* images, void* ws, size_t ws_bytes, double* f,
                       void* stream) {
    const char* what = "mvsdf_seams_colors";
    if (!ws || ws_bytes < SL_HDR || nodes < 0 || nodes > 3 * SL_MAX_FACES || nv < 0 || nv > INT_MAX || !P || !images ||
        !mv_pixel_center(pixel_center) || !mv_view_shape(views, H, W) || (nodes > 0 && (!node_vertex || !node_view || !verts || !f)))
        return mv_fail(-1, "mvsdf_seams_colors: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = mv_check(hipMemsetAsync(ws, 0, SL_HDR, s), what)) return rc;
    hipLaunchKernelGGL(k_any_nonfinite<double>, dim3(1), dim3(MV_THREADS), 0, s, P, (long long)views * 16, (unsigned long long*)ws + MVSDF_SL_H_ERR,
                       (unsigned long long)MVSDF_TX_ERR_FINITE);
    if (nodes > 0)
        hipLaunchKernelGGL(k_sl_colors, dim3(mv_grid(nodes, SL_T)), dim3(SL_T), 0, s, node_vertex, node_view, (long long)nodes, verts, (long long)nv, P,
                           (int)views, (int)H, (int)W, pixel_center, images, f, (long long*)ws);
    return mv_check(hipGetLastError(), what);
}

int mvsdf_seams_apply(const int64_t* adj_off, const int32_t* adj_seam, const int32_t* adj_node, int64_t nodes, int64_t nnz, const double* x,
                      double smoothness, double anchor, void* ws, size_t ws_bytes, double* out, void* stream) {
    const char* what = "mvsdf_seams_apply";
    if (!ws || ws_bytes < SL_HDR || !sl_graph_args(adj_off, adj_seam, adj_node, nodes, nnz) || (nodes > 0 && (!x || !out)) || !isfinite(smoothness) ||
        smoothness < 0.0 || !isfinite(anchor) || !(anchor > 0.0))
        return mv_fail(-1, "mvsdf_seams_apply: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = mv_check(hipMemsetAsync(ws, 0, SL_HDR, s), what)) return rc;
    const SlGraph G = {(const long long*)adj_off, adj_seam, adj_node, (long long)nodes, (long long)nnz};
    if (nodes > 0) hipLaunchKernelGGL(k_sl_apply, dim3(mv_grid(nodes, SL_T)), dim3(SL_T), 0, s, G, x, smoothness, anchor, out, (long long*)ws);
    return mv_check(hipGetLastError(), what);
}

int mvsdf_seams_solve(const int64_t* adj_off, const int32_t* adj_seam, const int32_t* adj_node, int64_t nodes, int64_t nnz, const double* f,
                      double smoothness, double anchor, int32_t cg_iters, double cg_tol, void* ws, size_t ws_bytes, double* g, void* stream) {
    const char* what = "mvsdf_seams_solve";
    SlSolveWs L;
    if (!ws || !sl_solve_ws(nodes, &L) || !sl_graph_args(adj_off, adj_seam, adj_node, nodes, nnz) || (nodes > 0 && (!f || !g)) ||
        !isfinite(smoothness) || smoothness < 0.0 || !isfinite(anchor) || !(anchor > 0.0) || cg_iters < 0 || cg_iters > MVSDF_SL_MAX_CG ||
        !(cg_tol >= 0.0))
        return mv_fail(-1, "mvsdf_seams_solve: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_seams_solve: workspace too small (mvsdf_seams_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)ws;
    long long* st = (long long*)ws;
    if (int rc = mv_check(hipMemsetAsync(ws, 0, SL_HDR, s), what)) return rc;
    if (nodes == 0) {                                              // nothing to solve: every channel done, rho = 0
        hipLaunchKernelGGL(k_sl_begin, dim3(1), dim3(64), 0, s, st);
        return mv_check(hipGetLastError(), what);
    }
    const SlGraph G = {(const long long*)adj_off, adj_seam, adj_node, (long long)nodes, (long long)nnz};
    const SlCg S = {g, (double*)(w + L.r), (double*)(w + L.p), (double*)(w + L.q), (double*)(w + L.d), (double*)(w + L.terms), st};
    const unsigned gr = mv_grid(nodes, SL_T);
    hipLaunchKernelGGL(k_sl_init, dim3(gr), dim3(SL_T), 0, s, G, f, smoothness, anchor, S);
    sl_dots(L, w, MVSDF_SL_H_RHO, 0, s);
    hipLaunchKernelGGL(k_sl_begin, dim3(1), dim3(64), 0, s, st);
    for (int it = 0; it < cg_iters; ++it) {
        hipLaunchKernelGGL(k_sl_apq, dim3(gr), dim3(SL_T), 0, s, G, smoothness, anchor, S);
        sl_dots(L, w, MVSDF_SL_H_SIGMA, 1, s);
        hipLaunchKernelGGL(k_sl_update, dim3(gr), dim3(SL_T), 0, s, (long long)nodes, S);
        sl_dots(L, w, MVSDF_SL_H_RHON, 1, s);
        hipLaunchKernelGGL(k_sl_direction, dim3(gr), dim3(SL_T), 0, s, (long long)nodes, S);
        hipLaunchKernelGGL(k_sl_step, dim3(1), dim3(64), 0, s, st, cg_tol * cg_tol);
    }
    return mv_check(hipGetLastError(), what);
}

}  // extern "C"
