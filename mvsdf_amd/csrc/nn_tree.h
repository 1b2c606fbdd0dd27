// nn_tree.h -- what chamfer.hip and cloud.hip share: the constants and error bits, the 64-bit LSD radix sort passes (their int64 scan is geom_prims.h's mv_scan) and the
// Morton-sorted points with their implicit 8-ary tree of fp64 boxes (built by ch_tree_frame + ch_tree_build, walked without a stack by the
// query kernels of either file).  Kernels are static: each including file gets its own copies.
#pragma once
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

enum {
    CH_ERR_POINTS = 1,      // sampling: more points than max_points
    CH_ERR_RANGE = 2,       // sampling: a vertex id outside [0, nv)
    CH_ERR_FINITE = 4,      // a non-finite coordinate
    CH_ERR_COORD = 8,       // downsampling: a coordinate too far from the origin for the cell grid
    CH_ERR_HASH = 16,       // the cell table's probe bound (cannot happen at load factor 1/2)
    CH_ERR_ROUNDS = 32,     // downsampling: the round limit was reached
    CH_ERR_WALK = 64,       // nearest: a tree walk hit its bound (cannot happen)
};

__device__ __forceinline__ double ch_d2(double ax, double ay, double az, double bx, double by, double bz) {
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ bool ch_finite3(const double* p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// ================================================================ the tree ================================================================
// per-workgroup box of the references (k_nn_bbox_final combines them); a non-finite coordinate raises CH_ERR_FINITE
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
    if (bad) atomicOr(err, CH_ERR_FINITE);
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

struct ChTreeLayout {
    ChTree T;
    long long nbr, rs_nb;
    size_t part, frame, k0, k1, v0, v1, hist, tmp, tot, sp, box;
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
    L->rs_nb = mv_ceil_div(nr, CH_RS_CHUNK);
    L->part = c.take((size_t)L->nbr * 48);
    L->frame = c.take(6 * 8);
    L->k0 = c.take((size_t)nr * 8);
    L->k1 = c.take((size_t)nr * 8);
    L->v0 = c.take((size_t)nr * 4);
    L->v1 = c.take((size_t)nr * 4);
    L->hist = c.take((size_t)L->rs_nb * CH_RS_BINS * 8);
    L->tmp = c.take(mv_scan_tmp_bytes(L->rs_nb * CH_RS_BINS));
    L->tot = c.take(8);                                           // the scan's total, which nobody reads
    L->sp = c.take((size_t)nr * 24);
    L->box = c.take((size_t)T.nodes * 48);
    return true;
}

// the box of the points -> frame; a non-finite coordinate raises CH_ERR_FINITE in *err
static void ch_tree_frame(const double* refs, long long nr, char* w, const ChTreeLayout& L, int* err, hipStream_t s) {
    hipLaunchKernelGGL(k_nn_bbox_part, dim3((unsigned)L.nbr), dim3(CH_THREADS), 0, s, refs, nr, (double*)(w + L.part), err);
    hipLaunchKernelGGL(k_nn_bbox_final, dim3(1), dim3(64), 0, s, (const double*)(w + L.part), L.nbr, (double*)(w + L.frame));
}

// stable LSD radix sort of n 64-bit keys (bits [0, bits), 4 per pass) with their int values, ping-pong between k / v [0] and [1] -> the index
// (0 / 1) that holds the sorted arrays
static int ch_radix_sort(unsigned long long* const k[2], int* const v[2], long long n, int bits, char* w, const ChTreeLayout& L, hipStream_t s) {
    const int nb = (int)L.rs_nb;
    long long* hist = (long long*)(w + L.hist);
    long long* tot = (long long*)(w + L.tot);
    int cur = 0;
    for (int shift = 0; shift < bits; shift += 4) {
        hipLaunchKernelGGL(k_rs_hist, dim3(nb), dim3(CH_THREADS), 0, s, (const unsigned long long*)k[cur], n, shift, hist, nb);
        mv_scan(hist, L.rs_nb * CH_RS_BINS, hist, w + L.tmp, tot, s);
        hipLaunchKernelGGL(k_rs_scatter, dim3(nb), dim3(CH_THREADS), 0, s, (const unsigned long long*)k[cur], (const int*)v[cur], n, shift,
                           (const long long*)hist, nb, k[cur ^ 1], v[cur ^ 1]);
        cur ^= 1;
    }
    return cur;
}

// after ch_tree_frame found no error: Morton keys, the sort, the sorted points (w + L.sp) and the boxes (w + L.box) -> the permutation
// (sorted position -> input index)
static const int* ch_tree_build(const double* refs, long long nr, char* w, const ChTreeLayout& L, hipStream_t s) {
    unsigned long long* k[2] = {(unsigned long long*)(w + L.k0), (unsigned long long*)(w + L.k1)};
    int* v[2] = {(int*)(w + L.v0), (int*)(w + L.v1)};
    const unsigned gr = mv_grid(nr, CH_THREADS);
    hipLaunchKernelGGL(k_nn_morton, dim3(gr), dim3(CH_THREADS), 0, s, refs, nr, (const double*)(w + L.frame), k[0], v[0]);
    const int cur = ch_radix_sort(k, v, nr, 3 * CH_MORTON_BITS, w, L, s);
    double* sp = (double*)(w + L.sp);
    double* box = (double*)(w + L.box);
    const ChTree& T = L.T;
    hipLaunchKernelGGL(k_nn_gather, dim3(gr), dim3(CH_THREADS), 0, s, refs, nr, (const int*)v[cur], sp);
    hipLaunchKernelGGL(k_nn_leaf_box, dim3(mv_grid(T.cnt[0], CH_THREADS)), dim3(CH_THREADS), 0, s, (const double*)sp, nr, T.cnt[0], box);
    for (int lv = 1; lv <= T.top; ++lv)
        hipLaunchKernelGGL(k_nn_node_box, dim3(mv_grid(T.cnt[lv], CH_THREADS)), dim3(CH_THREADS), 0, s, (const double*)(box + T.off[lv - 1] * 6),
                           T.cnt[lv - 1], T.cnt[lv], box + T.off[lv] * 6);
    return v[cur];
}
