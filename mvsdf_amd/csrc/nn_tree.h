// nn_tree.h -- what the point-cloud files share (chamfer.hip, cloud.hip, normals.hip, registration.hip; mesh_simplify.hip takes the sort alone):
// * the constants and the error bits;
// * the stable 64-bit LSD radix sort (ChSortLayout, ch_radix_sort; its int64 scan is geom_prims.h's mv_scan);
// * the Morton-sorted points with their implicit 8-ary tree of fp64 boxes (ChTreeLayout, ch_tree_begin = ch_tree_frame + one read of the error
//   word + ch_tree_build), which also says where the permutation sorted position -> input index lies;
// * the traversals, each written once: ch_walk (depth first without a stack, over a bound and a leaf visitor the caller gives), ch_descend (the
//   greedy way to one leaf for a first bound) and ch_knn_lane (the k nearest of a sorted point into a list the caller gives), with ch_knn_dispatch
//   for the list capacities.  The bit-for-bit results of every file above rest on these.
// Kernels are static: each including file gets its own copies.
#pragma once
#include <type_traits>
#include "geom_prims.h"

#define CH_THREADS 256
#define CH_ITEMS 8                                    // consecutive items per lane in the scans and sums
#define CH_CHUNK (CH_THREADS * CH_ITEMS)
#define CH_TOP_THREADS 1024
#define CH_HDR 256                                    // bytes at the start of every workspace: int64 results the host reads
#define CH_EMPTY 0xffffffffffffffffull
#define CH_LEAF 16                                    // reference points per leaf
#define CH_ARITY 8
#define CH_MAX_LEVELS 16
#define CH_RS_BINS 16                                 // radix sort: 4 bits per pass
#define CH_RS_ITEMS 16
#define CH_RS_CHUNK (CH_THREADS * CH_RS_ITEMS)
#define CH_MORTON_BITS 21
#define CH_DS_BATCH 4                                 // downsampling rounds per host check
#define CH_MARGIN2 (1.0 + 4e-9)                       // relative margin of a box prune on squared distances
#define CH_CELL_LIMIT 2147483648.0                    // |coordinate / cell| bound that keeps the 27-cell search exact

__device__ __forceinline__ double ch_d2(double ax, double ay, double az, double bx, double by, double bz) {
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ bool ch_finite3(const double* p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// ================================================================ the tree ================================================================
// per-workgroup box of the references (k_nn_bbox_final combines them); a non-finite coordinate raises MVSDF_PC_ERR_FINITE
static __global__ __launch_bounds__(CH_THREADS) void k_nn_bbox_part(const double* __restrict__ R, long long n, double* __restrict__ part, int* err) {
    __shared__ double sh[6][CH_THREADS];
    const long long base = (long long)blockIdx.x * CH_CHUNK;
    double b[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int bad = 0;
    for (int q = 0; q < CH_ITEMS; ++q) {
        const long long i = base + (long long)q * CH_THREADS + threadIdx.x;
        if (i >= n) break;
        const double* p = R + i * 3;
        if (!ch_finite3(p)) {
            bad = 1;
            continue;
        }
        for (int a = 0; a < 3; ++a) {
            b[a] = fmin(b[a], p[a]);
            b[3 + a] = fmax(b[3 + a], p[a]);
        }
    }
    if (bad) atomicOr(err, MVSDF_PC_ERR_FINITE);
    for (int a = 0; a < 6; ++a) sh[a][threadIdx.x] = b[a];
    __syncthreads();
    for (int d = CH_THREADS / 2; d; d >>= 1) {
        if ((int)threadIdx.x < d)
            for (int a = 0; a < 6; ++a)
                sh[a][threadIdx.x] = a < 3 ? fmin(sh[a][threadIdx.x], sh[a][threadIdx.x + d]) : fmax(sh[a][threadIdx.x], sh[a][threadIdx.x + d]);
        __syncthreads();
    }
    if (threadIdx.x < 6) part[blockIdx.x * 6 + threadIdx.x] = sh[threadIdx.x][0];
}

// frame[0..2] = the box's low corner, frame[3..5] = 2^21 / extent (1 for a flat axis)
static __global__ __launch_bounds__(64) void k_nn_bbox_final(const double* __restrict__ part, long long nb, double* __restrict__ frame) {
    const int a = threadIdx.x;
    if (a >= 3) return;
    double lo = INFINITY, hi = -INFINITY;
    for (long long b = 0; b < nb; ++b) {
        lo = fmin(lo, part[b * 6 + a]);
        hi = fmax(hi, part[b * 6 + 3 + a]);
    }
    frame[a] = lo;
    frame[3 + a] = hi > lo ? (double)(1 << CH_MORTON_BITS) / (hi - lo) : 1.0;
}

__device__ __forceinline__ unsigned long long ch_spread3(unsigned long long x) {   // 21 bits -> every third bit of 63
    x &= 0x1fffff;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

static __global__ __launch_bounds__(CH_THREADS) void k_nn_morton(const double* __restrict__ R, long long n, const double* __restrict__ frame,
                                                           unsigned long long* __restrict__ key, int* __restrict__ val) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n) return;
    unsigned long long m = 0;
    for (int a = 0; a < 3; ++a) {
        const double x = (R[i * 3 + a] - frame[a]) * frame[3 + a];
        const double c = x >= 0.0 ? fmin(x, (double)((1 << CH_MORTON_BITS) - 1)) : 0.0;
        m |= ch_spread3((unsigned long long)c) << a;
    }
    key[i] = m;
    val[i] = (int)i;
}

// radix sort, pass `shift`: per-workgroup digit counts, digit-major: hist[d * nb + b]
static __global__ __launch_bounds__(CH_THREADS) void k_rs_hist(const unsigned long long* __restrict__ key, long long n, int shift, long long* __restrict__ hist, int nb) {
    __shared__ int c[CH_RS_BINS];
    if (threadIdx.x < CH_RS_BINS) c[threadIdx.x] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * CH_RS_CHUNK;
    for (int q = 0; q < CH_RS_ITEMS; ++q) {
        const long long i = base + (long long)q * CH_THREADS + threadIdx.x;
        if (i < n) atomicAdd(&c[(key[i] >> shift) & (CH_RS_BINS - 1)], 1);
    }
    __syncthreads();
    if (threadIdx.x < CH_RS_BINS) hist[(long long)threadIdx.x * nb + blockIdx.x] = c[threadIdx.x];
}

// stable scatter: lane t owns items [base + t * CH_RS_ITEMS, + CH_RS_ITEMS); its place among equal digits of the workgroup is the count of those
// digits in lanes < t (an exclusive scan over the lanes in LDS) plus its own running count
static __global__ __launch_bounds__(CH_THREADS) void k_rs_scatter(const unsigned long long* __restrict__ kin, const int* __restrict__ vin, long long n, int shift,
                                                            const long long* __restrict__ off, int nb, unsigned long long* __restrict__ kout, int* __restrict__ vout) {
    __shared__ int c[CH_RS_BINS][CH_THREADS];
    const int t = threadIdx.x;
    const long long base = (long long)blockIdx.x * CH_RS_CHUNK + (long long)t * CH_RS_ITEMS;
#pragma unroll
    for (int d = 0; d < CH_RS_BINS; ++d) c[d][t] = 0;
    for (int q = 0; q < CH_RS_ITEMS; ++q)
        if (base + q < n) ++c[(kin[base + q] >> shift) & (CH_RS_BINS - 1)][t];
    __syncthreads();
    int own[CH_RS_BINS];
#pragma unroll
    for (int d = 0; d < CH_RS_BINS; ++d) own[d] = c[d][t];
    for (int s = 1; s < CH_THREADS; s <<= 1) {                   // inclusive Hillis-Steele scan over the lanes, every digit at once
        int x[CH_RS_BINS];
#pragma unroll
        for (int d = 0; d < CH_RS_BINS; ++d) x[d] = t >= s ? c[d][t - s] : 0;
        __syncthreads();
#pragma unroll
        for (int d = 0; d < CH_RS_BINS; ++d) c[d][t] += x[d];
        __syncthreads();
    }
#pragma unroll
    for (int d = 0; d < CH_RS_BINS; ++d) c[d][t] -= own[d];    // exclusive; from here lane t alone uses column t as its running position
    for (int q = 0; q < CH_RS_ITEMS; ++q) {
        const long long i = base + q;
        if (i >= n) break;
        const unsigned long long k = kin[i];
        const int d = (k >> shift) & (CH_RS_BINS - 1);
        const long long dst = off[(long long)d * nb + blockIdx.x] + c[d][t]++;
        kout[dst] = k;
        vout[dst] = vin[i];
    }
}

static __global__ __launch_bounds__(CH_THREADS) void k_nn_gather(const double* __restrict__ R, long long n, const int* __restrict__ val, double* __restrict__ sp) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n) return;
    const long long j = val[i];
    for (int c = 0; c < 3; ++c) sp[i * 3 + c] = R[j * 3 + c];
}

static __global__ __launch_bounds__(CH_THREADS) void k_nn_leaf_box(const double* __restrict__ sp, long long n, long long nleaf, double* __restrict__ box) {
    const long long l = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (l >= nleaf) return;
    double b[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    const long long e = min(n, (l + 1) * CH_LEAF);
    for (long long i = l * CH_LEAF; i < e; ++i)
        for (int a = 0; a < 3; ++a) {
            b[a] = fmin(b[a], sp[i * 3 + a]);
            b[3 + a] = fmax(b[3 + a], sp[i * 3 + a]);
        }
    for (int a = 0; a < 6; ++a) box[l * 6 + a] = b[a];
}

// node i of a level = the union of children [8 i, min(8 i + 8, nchild)) of the level below
static __global__ __launch_bounds__(CH_THREADS) void k_nn_node_box(const double* __restrict__ child, long long nchild, long long nnode, double* __restrict__ box) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= nnode) return;
    double b[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    const long long e = min(nchild, (i + 1) * CH_ARITY);
    for (long long k = i * CH_ARITY; k < e; ++k)
        for (int a = 0; a < 3; ++a) {
            b[a] = fmin(b[a], child[k * 6 + a]);
            b[3 + a] = fmax(b[3 + a], child[k * 6 + 3 + a]);
        }
    for (int a = 0; a < 6; ++a) box[i * 6 + a] = b[a];
}

struct ChTree {
    int top;                                          // root level (level 0 = the leaves)
    long long cnt[CH_MAX_LEVELS], off[CH_MAX_LEVELS]; // nodes per level, their first box
    long long n, nodes;
};

__device__ __forceinline__ double ch_box_lb2(const double* __restrict__ b, double x, double y, double z) {
    const double gx = x < b[0] ? b[0] - x : (x > b[3] ? x - b[3] : 0.0);
    const double gy = y < b[1] ? b[1] - y : (y > b[4] ? y - b[4] : 0.0);
    const double gz = z < b[2] ? b[2] - z : (z > b[5] ? z - b[5] : 0.0);
    return (gx * gx + gy * gy) + gz * gz;
}

// ---- the traversals ----
// Depth first over the implicit tree, children in index order, no stack (parent = i / 8, next sibling = i + 1).  A node is entered when the lower
// bound of its box is <= bound() -- the caller's current bound on squared distances, CH_MARGIN2 already in it; inclusive, so a box that may hold an
// equal distance is never passed over -- and leaf(l) is called for every leaf entered.  The walk ends at the first node whose sorted positions all
// lie above `last` (every later node's do too).  false: the step bound was reached (cannot happen; the caller raises MVSDF_PC_ERR_WALK).
template <class Bound, class Leaf>
__device__ __forceinline__ bool ch_walk(const double* __restrict__ box, const ChTree& T, double x, double y, double z, Bound bound, Leaf leaf,
                                        long long last = LLONG_MAX) {
    int lv = T.top;
    long long i = 0;
    const long long max_steps = 2 * T.nodes + 4;
    long long step = 0;
    for (; step < max_steps; ++step) {
        if ((i << (3 * lv)) * CH_LEAF > last) break;
        const double b = bound();
        if (ch_box_lb2(box + (T.off[lv] + i) * 6, x, y, z) <= b) {
            if (lv > 0) {
                --lv;
                i *= CH_ARITY;
                continue;
            }
            leaf(i);
        }
        while (lv < T.top && (i % CH_ARITY == CH_ARITY - 1 || i + 1 >= T.cnt[lv])) {
            i /= CH_ARITY;
            ++lv;
        }
        if (lv == T.top) break;
        ++i;
    }
    return step < max_steps;
}

// A first bound: from the root to one leaf by the child of the nearest box.  CENTRE: among children as near (the query lies inside several boxes: all
// 0) the one whose centre is nearest, which only makes the bound better -- the walk decides the result either way.
template <bool CENTRE>
__device__ __forceinline__ long long ch_descend(const double* __restrict__ box, const ChTree& T, double x, double y, double z) {
    long long i = 0;
    for (int k = T.top; k > 0; --k) {
        const long long b = i * CH_ARITY, e = min(T.cnt[k - 1], b + CH_ARITY);
        long long pick = b;
        double lbest = INFINITY, cbest = INFINITY;
        for (long long c = b; c < e; ++c) {
            const double* __restrict__ bx = box + (T.off[k - 1] + c) * 6;
            const double lb = ch_box_lb2(bx, x, y, z);
            double cd = 0.0;
            if constexpr (CENTRE) cd = ch_d2(x, y, z, (bx[0] + bx[3]) * 0.5, (bx[1] + bx[4]) * 0.5, (bx[2] + bx[5]) * 0.5);
            if (lb < lbest || (CENTRE && lb == lbest && cd < cbest)) {
                lbest = lb;
                cbest = cd;
                pick = c;
            }
        }
        i = pick;
    }
    return i;
}

// The k nearest of sorted point p, one lane: `list` (kept in registers by its owner) answers kth(), the squared distance of its k-th entry, and
// takes offer(d2, q), the candidate at sorted position q.  Seeds are the point's own leaf and the two beside it; the walk passes those over, so
// every other point is offered once.  false: see ch_walk.
template <class List>
__device__ __forceinline__ bool ch_knn_lane(const double* __restrict__ sp, const double* __restrict__ box, const ChTree& T, long long p, List& list) {
    const double x = sp[p * 3], y = sp[p * 3 + 1], z = sp[p * 3 + 2];
    auto offer = [&](long long b, long long e, long long self) {
        for (long long q = b; q < e; ++q) {
            if (q == self) continue;
            list.offer(ch_d2(x, y, z, sp[q * 3], sp[q * 3 + 1], sp[q * 3 + 2]), q);
        }
    };
    const long long leaf = p / CH_LEAF, l0 = leaf > 0 ? leaf - 1 : 0, l1 = min(leaf + 1, T.cnt[0] - 1);
    offer(l0 * CH_LEAF, min(T.n, (l1 + 1) * CH_LEAF), p);
    return ch_walk(
        box, T, x, y, z, [&] { return list.kth() * CH_MARGIN2; },
        [&](long long i) {
            if (i < l0 || i > l1) offer(i * CH_LEAF, min(T.n, (i + 1) * CH_LEAF), -1);
        });
}

// launch(std::integral_constant<int, CAP>) for the smallest list capacity CAP = 8 / 16 / 24 / 32 that holds k
template <class Launch>
static void ch_knn_dispatch(int k, Launch launch) {
    if (k <= 8)
        launch(std::integral_constant<int, 8>());
    else if (k <= 16)
        launch(std::integral_constant<int, 16>());
    else if (k <= 24)
        launch(std::integral_constant<int, 24>());
    else
        launch(std::integral_constant<int, 32>());
}

// ---- the workspace ----
// what a radix sort of up to nb * CH_RS_CHUNK keys needs beside the keys and values
struct ChSortLayout {
    long long nb;
    size_t hist, tmp, tot;
};

// scan_n: the scratch also serves the owner's other scans of up to scan_n items (0: the sort's alone)
static void ch_sort_layout(long long n, long long scan_n, WsCursor& c, ChSortLayout* S) {
    S->nb = mv_ceil_div(n, CH_RS_CHUNK);
    S->hist = c.take((size_t)S->nb * CH_RS_BINS * 8);
    S->tmp = c.take(mv_scan_tmp_bytes(scan_n > S->nb * CH_RS_BINS ? scan_n : S->nb * CH_RS_BINS));
    S->tot = c.take(8);                                           // the scan's total, which nobody reads
}

static int ch_sort_passes(int bits) { return (bits + 3) / 4; }

struct ChTreeLayout {
    ChTree T;
    long long nbr;
    ChSortLayout rs;
    size_t part, frame, k0, k1, v0, v1, sp, box;
    size_t perm;                                      // v0 or v1: where ch_tree_build leaves the permutation (sorted position -> input index)
};

// the tree's shape over nr points and its buffers from the cursor on
static bool ch_tree_layout(long long nr, WsCursor& c, ChTreeLayout* L) {
    if (nr < 1 || nr > INT_MAX) return false;
    ChTree& T = L->T;
    T.n = nr;
    T.cnt[0] = (nr + CH_LEAF - 1) / CH_LEAF;
    T.off[0] = 0;
    T.top = 0;
    while (T.cnt[T.top] > 1) {
        if (T.top + 1 >= CH_MAX_LEVELS) return false;
        T.cnt[T.top + 1] = (T.cnt[T.top] + CH_ARITY - 1) / CH_ARITY;
        T.off[T.top + 1] = T.off[T.top] + T.cnt[T.top];
        ++T.top;
    }
    T.nodes = T.off[T.top] + 1;
    L->nbr = mv_ceil_div(nr, CH_CHUNK);
    L->part = c.take((size_t)L->nbr * 48);
    L->frame = c.take(6 * 8);
    L->k0 = c.take((size_t)nr * 8);
    L->k1 = c.take((size_t)nr * 8);
    L->v0 = c.take((size_t)nr * 4);
    L->v1 = c.take((size_t)nr * 4);
    ch_sort_layout(nr, 0, c, &L->rs);
    L->sp = c.take((size_t)nr * 24);
    L->box = c.take((size_t)T.nodes * 48);
    L->perm = ch_sort_passes(3 * CH_MORTON_BITS) % 2 ? L->v1 : L->v0;   // the sort ping-pongs from v0 once per pass
    return true;
}

// the box of the points -> frame; a non-finite coordinate raises MVSDF_PC_ERR_FINITE in *err
static void ch_tree_frame(const double* refs, long long nr, char* w, const ChTreeLayout& L, int* err, hipStream_t s) {
    hipLaunchKernelGGL(k_nn_bbox_part, dim3((unsigned)L.nbr), dim3(CH_THREADS), 0, s, refs, nr, (double*)(w + L.part), err);
    hipLaunchKernelGGL(k_nn_bbox_final, dim3(1), dim3(64), 0, s, (const double*)(w + L.part), L.nbr, (double*)(w + L.frame));
}

// stable LSD radix sort of n 64-bit keys (bits [0, bits), 4 per pass) with their int values, ping-pong between k / v [0] and [1] -> the index
// (0 / 1) that holds the sorted arrays.  n is at most what S was laid out for; the histogram is as wide as n's own workgroups (<= S.nb).
static int ch_radix_sort(unsigned long long* const k[2], int* const v[2], long long n, int bits, char* w, const ChSortLayout& S, hipStream_t s) {
    const int nb = (int)mv_ceil_div(n, CH_RS_CHUNK);
    long long* hist = (long long*)(w + S.hist);
    long long* tot = (long long*)(w + S.tot);
    int cur = 0;
    for (int pass = 0; pass < ch_sort_passes(bits); ++pass) {
        const int shift = 4 * pass;
        hipLaunchKernelGGL(k_rs_hist, dim3(nb), dim3(CH_THREADS), 0, s, (const unsigned long long*)k[cur], n, shift, hist, nb);
        mv_scan(hist, (long long)nb * CH_RS_BINS, hist, w + S.tmp, tot, s);
        hipLaunchKernelGGL(k_rs_scatter, dim3(nb), dim3(CH_THREADS), 0, s, (const unsigned long long*)k[cur], (const int*)v[cur], n, shift,
                           (const long long*)hist, nb, k[cur ^ 1], v[cur ^ 1]);
        cur ^= 1;
    }
    return cur;
}

// after ch_tree_frame found no error: Morton keys, the sort, the sorted points (w + L.sp) and the boxes (w + L.box) -> the permutation at w + L.perm
static const int* ch_tree_build(const double* refs, long long nr, char* w, const ChTreeLayout& L, hipStream_t s) {
    unsigned long long* k[2] = {(unsigned long long*)(w + L.k0), (unsigned long long*)(w + L.k1)};
    int* v[2] = {(int*)(w + L.v0), (int*)(w + L.v1)};
    const int* perm = (const int*)(w + L.perm);
    const unsigned gr = mv_grid(nr, CH_THREADS);
    hipLaunchKernelGGL(k_nn_morton, dim3(gr), dim3(CH_THREADS), 0, s, refs, nr, (const double*)(w + L.frame), k[0], v[0]);
    ch_radix_sort(k, v, nr, 3 * CH_MORTON_BITS, w, L.rs, s);
    double* sp = (double*)(w + L.sp);
    double* box = (double*)(w + L.box);
    const ChTree& T = L.T;
    hipLaunchKernelGGL(k_nn_gather, dim3(gr), dim3(CH_THREADS), 0, s, refs, nr, perm, sp);
    hipLaunchKernelGGL(k_nn_leaf_box, dim3(mv_grid(T.cnt[0], CH_THREADS)), dim3(CH_THREADS), 0, s, (const double*)sp, nr, T.cnt[0], box);
    for (int lv = 1; lv <= T.top; ++lv)
        hipLaunchKernelGGL(k_nn_node_box, dim3(mv_grid(T.cnt[lv], CH_THREADS)), dim3(CH_THREADS), 0, s, (const double*)(box + T.off[lv - 1] * 6),
                           T.cnt[lv - 1], T.cnt[lv], box + T.off[lv] * 6);
    return perm;
}

struct ChBuilt {
    int rc, err;                                      // the HIP status (mv_check's); the error bits the frame raised
    const int* perm;                                  // the permutation, once rc == 0 && err == 0
};

// The frame, its launch check, the one 4-byte read of *err (which the caller has zeroed), and where that is 0 the tree and its launch check.  The
// caller writes its own header for rc == 0 && err != 0: nothing was built.
static ChBuilt ch_tree_begin(const double* pts, long long n, char* w, const ChTreeLayout& L, int* err, hipStream_t s, const char* what) {
    ChBuilt b = {0, 0, nullptr};
    ch_tree_frame(pts, n, w, L, err, s);
    if ((b.rc = mv_check(hipGetLastError(), what))) return b;
    if ((b.rc = mv_read(&b.err, err, 4, s, what)) || b.err) return b;
    b.perm = ch_tree_build(pts, n, w, L, s);
    b.rc = mv_check(hipGetLastError(), what);
    return b;
}
