// registration.hip -- on-device registration and F-score evaluation (the Tanks and Temples protocol): a kept nearest-neighbour tree that returns the
// neighbour's index, the rigid transform, the polygon-prism crop, the voxel filter, the 17 sums of a point-to-point ICP iteration and the distance
// histograms.  Python: mvsdf_amd/registration.py, which states every definition; tests/registration_ref.py restates them in numpy.  All arithmetic
// is fp64 without contraction, in the order the definitions write it.
//
// * The tree is nn_tree.h's (Morton sort, leaves of CH_LEAF points, implicit 8-ary tree of fp64 boxes), built once into a workspace the caller
//   keeps: the sorted points, the boxes and the permutation sorted position -> input index stay resident, so a query sorts nothing.
// * The query is one lane per query over nn_tree.h's traversals (ch_descend, ch_walk), as in chamfer.hip, with a leaf visitor that orders
//   candidates by (d2, input index): a box is pruned only when its lower bound exceeds min(best, max_dist^2) by a relative 4e-9, so every box that could hold an equal distance is visited and the
//   smallest input index among the references at the exact minimum wins, whatever the visiting order.  The visitor keeps the sorted position of
//   the best candidate and reads the permutation only on an exact tie; the first bound comes from the leaf under the nearest box centres.
// * The ICP sums follow k_nn_sum_part / k_nn_sum_final: source order, 8 consecutive items per lane from 0, a 256-lane halving tree, block partials,
//   a 1024-lane final (one quantity after the other through one LDS array: the order of each sum is the same as with 17 arrays).
// * The voxel filter: keys, nn_tree.h's stable radix sort, segment heads, the shared scan, one lane per voxel walking its segment (stable sort:
//   ascending input index).
// * The histogram uses integer atomics only (LDS counters per workgroup, then one global add per touched bin).
//
// Every device loop is bounded; no kernel waits on another.
#include "nn_tree.h"

#define RG_MAX_EDGES 4097
#define RG_SUMS 16                                    // fp64 sums of an ICP iteration (the 17th quantity is the int64 pair count)
#define RG_VOXEL_BITS 21
static_assert(MVSDF_REG_TREE_H_ERR < MVSDF_REG_TREE_H_CENTRE && MVSDF_REG_ICP_H_ERR - MVSDF_REG_ICP_H_SUMS == RG_SUMS, "the header words as the kernels write them");
static_assert(MVSDF_REG_TREE_H_WORDS * 8 <= CH_HDR && MVSDF_REG_ICP_H_WORDS * 8 <= CH_HDR && MVSDF_REG_VOXEL_H_WORDS * 8 <= CH_HDR &&
                  MVSDF_ROWS_H_WORDS * 8 <= CH_HDR,
              "the result words fit the header");

struct RgXform {
    double m[12];
    int on;
};

static RgXform rg_xform(const double* t) {
    RgXform X;
    X.on = t != nullptr;
    for (int k = 0; k < 12; ++k) X.m[k] = t ? t[k] : 0.0;
    return X;
}

__device__ __forceinline__ void rg_apply(const RgXform& X, const double* __restrict__ p, double* o) {
    const double x = p[0], y = p[1], z = p[2];
    if (!X.on) {
        o[0] = x;
        o[1] = y;
        o[2] = z;
        return;
    }
    for (int a = 0; a < 3; ++a) o[a] = ((X.m[a * 4] * x + X.m[a * 4 + 1] * y) + X.m[a * 4 + 2] * z) + X.m[a * 4 + 3];
}

// ================================================================ the kept tree ================================================================
struct RgTreeLayout {
    ChTreeLayout t;
    size_t flags, total;
};

static bool rg_tree_layout(long long nr, RgTreeLayout* L) {
    WsCursor c{CH_HDR};
    if (!ch_tree_layout(nr, c, &L->t)) return false;
    L->flags = c.take(4 * 8);
    L->total = c.o;
    return true;
}

// the centre of the root box, as three fp64 words behind the error word of the header
static __global__ __launch_bounds__(64) void k_rg_centre(const double* __restrict__ root, double* __restrict__ hdr) {
    const int a = threadIdx.x;
    if (a < 3) hdr[MVSDF_REG_TREE_H_CENTRE + a] = (root[a] + root[3 + a]) * 0.5;
}

// the leaf's candidates against (best, bi), bi = the sorted position of the best one: a smaller d2 wins without a look at the permutation; an equal
// one (rare outside lattices) wins if its input index is smaller.  i != bi: the walk meets the first-bound leaf a second time.
__device__ __forceinline__ void rg_leaf_min(const double* __restrict__ sp, const int* __restrict__ perm, long long n, long long l, double x, double y, double z,
                                            double& best, int& bi) {
    const int e = (int)min(n, (l + 1) * CH_LEAF);
    for (int i = (int)(l * CH_LEAF); i < e; ++i) {
        const double d = ch_d2(x, y, z, sp[(long long)i * 3], sp[(long long)i * 3 + 1], sp[(long long)i * 3 + 2]);
        if (d < best) {
            best = d;
            bi = i;
        } else if (d == best && i != bi) {
            if (bi < 0 || perm[i] < perm[bi]) bi = i;
        }
    }
}

// per query (moved by X): the minimum squared distance over the references and the smallest input index that attains it; +inf / -1 where the distance
// is not < max_dist.  dist, d2out and index may each be NULL.
static __global__ __launch_bounds__(CH_THREADS) void k_rg_query(const double* __restrict__ Q, long long nq, RgXform X, const double* __restrict__ sp,
                                                                const double* __restrict__ box, const int* __restrict__ perm, ChTree T, double max_dist,
                                                                double* __restrict__ dist, double* __restrict__ d2out, int* __restrict__ index, int* err) {
    const long long qi = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (qi >= nq) return;
    double p[3];
    rg_apply(X, Q + qi * 3, p);
    const double x = p[0], y = p[1], z = p[2];
    if (!ch_finite3(p)) {
        atomicOr(err, MVSDF_PC_ERR_FINITE);
        if (dist) dist[qi] = INFINITY;
        if (d2out) d2out[qi] = INFINITY;
        if (index) index[qi] = -1;
        return;
    }
    const double cut2 = max_dist * max_dist;
    double best = INFINITY;
    int bi = -1;
    // a first bound from the leaf under the nearest boxes (ties by the nearest centre), then the full walk: its inclusive prune keeps a box whose
    // lower bound equals the best distance, which may hold an equal distance under a smaller input index
    const long long first = ch_descend<true>(box, T, x, y, z);
    if (ch_box_lb2(box + first * 6, x, y, z) <= cut2 * CH_MARGIN2) rg_leaf_min(sp, perm, T.n, first, x, y, z, best, bi);
    if (!ch_walk(
            box, T, x, y, z, [&] { return fmin(best, cut2) * CH_MARGIN2; }, [&](long long l) { rg_leaf_min(sp, perm, T.n, l, x, y, z, best, bi); }))
        atomicOr(err, MVSDF_PC_ERR_WALK);
    const double d = sqrt(best);
    const bool hit = d < max_dist && bi >= 0;                     // (a finite best always has its position)
    if (dist) dist[qi] = hit ? d : INFINITY;
    if (d2out) d2out[qi] = hit ? best : INFINITY;
    if (index) index[qi] = hit ? perm[bi] : -1;
}

static void rg_launch_query(const char* tree, const RgTreeLayout& L, const double* queries, long long nq, const double* transform, double max_dist,
                            double* dist, double* d2, int* index, int* err, hipStream_t s) {
    hipLaunchKernelGGL(k_rg_query, dim3(mv_grid(nq, CH_THREADS)), dim3(CH_THREADS), 0, s, queries, nq, rg_xform(transform), (const double*)(tree + L.t.sp),
                       (const double*)(tree + L.t.box), (const int*)(tree + L.t.perm), L.t.T, max_dist, dist, d2, index, err);
}

// ================================================================ the sums of an ICP iteration ================================================================
// over the matched pairs (index >= 0) in source order: [0] d2, [1..3] p, [4..6] q, [7 + 3 a + b] p_a q_b, with p = X src - c and q = refs[index] - c.
// Partials: psum[a * nb + block], pcnt[block].
static __global__ __launch_bounds__(CH_THREADS) void k_rg_sum_part(const double* __restrict__ src, long long ns, RgXform X, const double* __restrict__ refs,
                                                                   const double* __restrict__ d2, const int* __restrict__ index,
                                                                   const double* __restrict__ centre, double* __restrict__ psum, long long* __restrict__ pcnt,
                                                                   long long nb) {
    __shared__ double ss[RG_SUMS][CH_THREADS];
    __shared__ long long sc[CH_THREADS];
    const int t = threadIdx.x;
    const long long base = (long long)blockIdx.x * CH_CHUNK + (long long)t * CH_ITEMS;
    const double c[3] = {centre[0], centre[1], centre[2]};
    double acc[RG_SUMS];
    for (int a = 0; a < RG_SUMS; ++a) acc[a] = 0.0;
    long long cnt = 0;
    for (int k = 0; k < CH_ITEMS; ++k) {
        const long long i = base + k;
        if (i >= ns) break;
        const int j = index[i];
        if (j < 0) continue;
        double p[3], q[3];
        rg_apply(X, src + i * 3, p);
        for (int a = 0; a < 3; ++a) {
            p[a] = p[a] - c[a];
            q[a] = refs[(long long)j * 3 + a] - c[a];
        }
        acc[0] += d2[i];
        for (int a = 0; a < 3; ++a) {
            acc[1 + a] += p[a];
            acc[4 + a] += q[a];
            for (int b = 0; b < 3; ++b) acc[7 + 3 * a + b] += p[a] * q[b];
        }
        ++cnt;
    }
    for (int a = 0; a < RG_SUMS; ++a) ss[a][t] = acc[a];
    sc[t] = cnt;
    __syncthreads();
    for (int w = CH_THREADS / 2; w; w >>= 1) {
        if (t < w) {
            for (int a = 0; a < RG_SUMS; ++a) ss[a][t] += ss[a][t + w];
            sc[t] += sc[t + w];
        }
        __syncthreads();
    }
    if (t < RG_SUMS) psum[(long long)t * nb + blockIdx.x] = ss[t][0];
    if (t == 0) pcnt[blockIdx.x] = sc[0];
}

// the count and the sums (as their bits) of MVSDF_REG_ICP_H_*
static __global__ __launch_bounds__(CH_TOP_THREADS) void k_rg_sum_final(const double* __restrict__ psum, const long long* __restrict__ pcnt, long long nb,
                                                                        long long* __restrict__ hdr) {
    __shared__ double ss[CH_TOP_THREADS];
    __shared__ long long sc[CH_TOP_THREADS];
    const int t = threadIdx.x;
    const long long per = (nb + CH_TOP_THREADS - 1) / CH_TOP_THREADS;
    const long long lo = min(nb, t * per), hi = min(nb, lo + per);
    long long c = 0;
    for (long long q = lo; q < hi; ++q) c += pcnt[q];
    sc[t] = c;
    __syncthreads();
    for (int w = CH_TOP_THREADS / 2; w; w >>= 1) {
        if (t < w) sc[t] += sc[t + w];
        __syncthreads();
    }
    if (t == 0) hdr[MVSDF_REG_ICP_H_N] = sc[0];
    for (int a = 0; a < RG_SUMS; ++a) {
        double s = 0.0;
        for (long long q = lo; q < hi; ++q) s += psum[(long long)a * nb + q];
        ss[t] = s;
        __syncthreads();
        for (int w = CH_TOP_THREADS / 2; w; w >>= 1) {
            if (t < w) ss[t] += ss[t + w];
            __syncthreads();
        }
        if (t == 0) hdr[MVSDF_REG_ICP_H_SUMS + a] = __double_as_longlong(ss[0]);
        __syncthreads();
    }
}

struct RgPairsLayout {
    long long nb;
    size_t psum, pcnt, total;
};

static bool rg_pairs_layout(long long ns, RgPairsLayout* L) {
    if (ns < 1 || ns > (1ll << 40)) return false;
    WsCursor c{CH_HDR};
    L->nb = mv_ceil_div(ns, CH_CHUNK);
    L->psum = c.take((size_t)L->nb * RG_SUMS * 8);
    L->pcnt = c.take((size_t)L->nb * 8);
    L->total = c.o;
    return true;
}

// ================================================================ transform, crop ================================================================
static __global__ __launch_bounds__(CH_THREADS) void k_rg_transform(const double* P, long long n, RgXform X, double* out) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n) return;
    double o[3];
    rg_apply(X, P + i * 3, o);
    for (int a = 0; a < 3; ++a) out[i * 3 + a] = o[a];
}

// keep[i] = inside the prism: between the axis bounds (inclusive) and an odd number of polygon edges crossed by the ray towards -u
static __global__ __launch_bounds__(CH_THREADS) void k_rg_crop_flags(const double* __restrict__ P, long long n, int u, int v, int w, double amin, double amax,
                                                                     const double* __restrict__ poly, int nverts, unsigned char* __restrict__ keep) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n) return;
    const double pu = P[i * 3 + u], pv = P[i * 3 + v], pw = P[i * 3 + w];
    int odd = 0;
    for (int a = 0; a < nverts; ++a) {
        const int b = a + 1 == nverts ? 0 : a + 1;
        const double iu = poly[a * 3 + u], iv = poly[a * 3 + v], ju = poly[b * 3 + u], jv = poly[b * 3 + v];
        if ((iv < pv && jv >= pv) || (jv < pv && iv >= pv))
            if (iu + (pv - iv) / (jv - iv) * (ju - iu) < pu) odd ^= 1;
    }
    keep[i] = (pw >= amin && pw <= amax && odd) ? 1 : 0;
}

// out[off[i]] = P[i] where keep[i]
static __global__ __launch_bounds__(CH_THREADS) void k_rg_scatter(const double* __restrict__ P, long long n, const unsigned char* __restrict__ keep,
                                                                  const long long* __restrict__ off, double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const long long o = off[i];
    for (int c = 0; c < 3; ++c) out[o * 3 + c] = P[i * 3 + c];
}

struct RgCropLayout {
    size_t off, tmp, tot, total;
};

static bool rg_crop_layout(long long n, RgCropLayout* L) {
    if (n < 1 || n > (1ll << 40)) return false;
    WsCursor c{CH_HDR};
    L->off = c.take((size_t)n * 8);
    L->tmp = c.take(mv_scan_tmp_bytes(n));
    L->tot = c.take(8);
    L->total = c.o;
    return true;
}

// ================================================================ the voxel filter ================================================================
// key = gx | gy << 21 | gz << 42 with g = floor((p - (min - voxel / 2)) / voxel); a g outside [0, 2^21) raises MVSDF_PC_ERR_COORD (MVSDF_PC_ERR_FINITE for a
// non-finite point) and counts as 0
static __global__ __launch_bounds__(CH_THREADS) void k_rg_voxel_key(const double* __restrict__ P, long long n, const double* __restrict__ frame, double voxel,
                                                                    unsigned long long* __restrict__ key, int* __restrict__ val, int* err) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n) return;
    unsigned long long k = 0;
    int bad = 0;
    for (int a = 0; a < 3; ++a) {
        const double p = P[i * 3 + a];
        const double o = frame[a] - voxel / 2;
        const double g = floor((p - o) / voxel);
        if (!(g >= 0.0 && g < (double)(1 << RG_VOXEL_BITS))) {
            bad |= isfinite(p) ? MVSDF_PC_ERR_COORD : MVSDF_PC_ERR_FINITE;
            continue;
        }
        k |= (unsigned long long)g << (RG_VOXEL_BITS * a);
    }
    if (bad) atomicOr(err, bad);
    key[i] = k;
    val[i] = (int)i;
}

static __global__ __launch_bounds__(CH_THREADS) void k_rg_heads(const unsigned long long* __restrict__ key, long long n, unsigned char* __restrict__ head) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n) return;
    head[i] = (i == 0 || key[i] != key[i - 1]) ? 1 : 0;
}

// one lane per voxel: from its head it walks the sorted segment (ascending input index: the sort is stable) and sums from 0.0
static __global__ __launch_bounds__(CH_THREADS) void k_rg_voxel_mean(const double* __restrict__ P, const unsigned long long* __restrict__ key,
                                                                     const int* __restrict__ val, const unsigned char* __restrict__ head,
                                                                     const long long* __restrict__ off, long long n, double* __restrict__ means,
                                                                     int* __restrict__ counts) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n || !head[i]) return;
    const unsigned long long k = key[i];
    double s[3] = {0.0, 0.0, 0.0};
    long long j = i;
    for (; j < n && key[j] == k; ++j) {
        const double* p = P + (long long)val[j] * 3;
        for (int a = 0; a < 3; ++a) s[a] += p[a];
    }
    const long long row = off[i];
    const double c = (double)(j - i);
    for (int a = 0; a < 3; ++a) means[row * 3 + a] = s[a] / c;
    counts[row] = (int)(j - i);
}

struct RgVoxelLayout {
    ChTreeLayout t;
    size_t head, off, tmp2, flags, total;
};

static bool rg_voxel_layout(long long n, RgVoxelLayout* L) {
    WsCursor c{CH_HDR};
    if (!ch_tree_layout(n, c, &L->t)) return false;
    L->head = c.take((size_t)n);
    L->off = c.take((size_t)n * 8);
    L->tmp2 = c.take(mv_scan_tmp_bytes(n));
    L->flags = c.take(4 * 8);
    L->total = c.o;
    return true;
}

// ================================================================ the histograms ================================================================
// out[0] += the distances < tau; out[1 + b] += the distances whose bin (the number of edges[1..] <= d) is b < nbins
static __global__ __launch_bounds__(CH_THREADS) void k_rg_hist(const double* __restrict__ d, long long n, const double* __restrict__ edges, int nbins, double tau,
                                                               unsigned long long* out) {
    __shared__ unsigned int h[RG_MAX_EDGES];                      // [nbins] = the count below tau
    for (int b = threadIdx.x; b <= nbins; b += CH_THREADS) h[b] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * CH_CHUNK;
    for (int q = 0; q < CH_ITEMS; ++q) {
        const long long i = base + (long long)q * CH_THREADS + threadIdx.x;
        if (i >= n) break;
        const double x = d[i];
        if (x < tau) atomicAdd(&h[nbins], 1u);
        int lo = 0, hi = nbins;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (edges[1 + mid] <= x)
                lo = mid + 1;
            else
                hi = mid;
        }
        if (lo < nbins) atomicAdd(&h[lo], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b <= nbins; b += CH_THREADS)
        if (h[b]) atomicAdd(out + (b == nbins ? 0 : 1 + b), (unsigned long long)h[b]);
}

extern "C" {

size_t mvsdf_reg_tree_workspace_bytes(int64_t nr) {
    RgTreeLayout L;
    return rg_tree_layout(nr, &L) ? L.total : 0;
}

int mvsdf_reg_tree_build(const double* refs, int64_t nr, void* ws, size_t ws_bytes, void* stream) {
    RgTreeLayout L;
    if (!refs || !ws || !rg_tree_layout(nr, &L)) return mv_fail(-1, "mvsdf_reg_tree_build: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_reg_tree_build: workspace too small (mvsdf_reg_tree_workspace_bytes)");
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    int* fl = (int*)(w + L.flags);
    long long hdr[MVSDF_REG_TREE_H_WORDS] = {};
    int rc;
    if ((rc = mv_check(hipMemsetAsync(fl, 0, 4 * 8, s), "mvsdf_reg_tree_build"))) return rc;
    const ChBuilt tree = ch_tree_begin(refs, (long long)nr, w, L.t, fl, s, "mvsdf_reg_tree_build");
    if (tree.rc) return tree.rc;
    if (tree.err) {
        hdr[MVSDF_REG_TREE_H_ERR] = tree.err;
        return mv_write_header(ws, hdr, MVSDF_REG_TREE_H_WORDS, s, "mvsdf_reg_tree_build");
    }
    const ChTree& T = L.t.T;
    hipLaunchKernelGGL(k_rg_centre, dim3(1), dim3(64), 0, s, (const double*)(w + L.t.box) + T.off[T.top] * 6, (double*)w);
    if ((rc = mv_check(hipGetLastError(), "mvsdf_reg_tree_build"))) return rc;
    return mv_write_header(ws, hdr, MVSDF_REG_TREE_H_CENTRE, s, "mvsdf_reg_tree_build");   // the words in front of the centre the kernel wrote
}

int mvsdf_reg_tree_query(const void* tree, size_t tree_bytes, int64_t nr, const double* queries, int64_t nq, const double* transform, double max_dist,
                         double* dist, double* d2, int32_t* index, int32_t* err, void* stream) {
    RgTreeLayout L;
    if (!tree || !err || nq < 0 || nq > (1ll << 40) || (nq > 0 && !queries) || !rg_tree_layout(nr, &L) || !(max_dist > 0))
        return mv_fail(-1, "mvsdf_reg_tree_query: bad arguments");
    if (tree_bytes < L.total) return mv_fail(-1, "mvsdf_reg_tree_query: not a tree over nr references (mvsdf_reg_tree_workspace_bytes)");
    if (nq == 0) return 0;
    rg_launch_query((const char*)tree, L, queries, (long long)nq, transform, max_dist, dist, d2, index, err, (hipStream_t)stream);
    return mv_check(hipGetLastError(), "mvsdf_reg_tree_query");
}

size_t mvsdf_reg_pairs_workspace_bytes(int64_t ns) {
    RgPairsLayout L;
    return rg_pairs_layout(ns, &L) ? L.total : 0;
}

int mvsdf_reg_icp_step(const void* tree, size_t tree_bytes, int64_t nr, const double* refs, const double* src, int64_t ns, const double* transform,
                       double max_dist, void* ws, size_t ws_bytes, double* d2, int32_t* index, void* stream) {
    RgTreeLayout L;
    RgPairsLayout P;
    if (!tree || !refs || !src || !ws || !d2 || !index || !rg_tree_layout(nr, &L) || !rg_pairs_layout(ns, &P) || !(max_dist > 0))
        return mv_fail(-1, "mvsdf_reg_icp_step: bad arguments");
    if (tree_bytes < L.total) return mv_fail(-1, "mvsdf_reg_icp_step: not a tree over nr references (mvsdf_reg_tree_workspace_bytes)");
    if (ws_bytes < P.total) return mv_fail(-1, "mvsdf_reg_icp_step: workspace too small (mvsdf_reg_pairs_workspace_bytes)");
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    long long* hdr = (long long*)w;
    int rc;
    if ((rc = mv_check(hipMemsetAsync(w, 0, CH_HDR, s), "mvsdf_reg_icp_step"))) return rc;
    rg_launch_query((const char*)tree, L, src, (long long)ns, transform, max_dist, nullptr, d2, index, (int*)(hdr + MVSDF_REG_ICP_H_ERR), s);
    hipLaunchKernelGGL(k_rg_sum_part, dim3((unsigned)P.nb), dim3(CH_THREADS), 0, s, src, (long long)ns, rg_xform(transform), refs, (const double*)d2,
                       (const int*)index, (const double*)tree + 1, (double*)(w + P.psum), (long long*)(w + P.pcnt), P.nb);
    hipLaunchKernelGGL(k_rg_sum_final, dim3(1), dim3(CH_TOP_THREADS), 0, s, (const double*)(w + P.psum), (const long long*)(w + P.pcnt), P.nb, hdr);
    if ((rc = mv_check(hipGetLastError(), "mvsdf_reg_icp_step"))) return rc;
    return mv_check(hipStreamSynchronize(s), "mvsdf_reg_icp_step");
}

int mvsdf_reg_transform(const double* pts, int64_t n, const double* transform, double* out, void* stream) {
    if (n < 0 || n > (1ll << 40) || !transform || (n > 0 && (!pts || !out))) return mv_fail(-1, "mvsdf_reg_transform: bad arguments");
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_rg_transform, dim3(mv_grid(n, CH_THREADS)), dim3(CH_THREADS), 0, (hipStream_t)stream, pts, (long long)n, rg_xform(transform), out);
    return mv_check(hipGetLastError(), "mvsdf_reg_transform");
}

size_t mvsdf_reg_crop_workspace_bytes(int64_t n) {
    RgCropLayout L;
    return rg_crop_layout(n, &L) ? L.total : 0;
}

int mvsdf_reg_crop(const double* pts, int64_t n, int32_t axis, double axis_min, double axis_max, const double* polygon, int32_t nverts, void* ws,
                   size_t ws_bytes, uint8_t* keep, double* out, void* stream) {
    RgCropLayout L;
    if (!pts || !polygon || !ws || !keep || !out || !rg_crop_layout(n, &L) || axis < 0 || axis > 2 || nverts < 3 || nverts > MVSDF_REG_MAX_POLYGON)
        return mv_fail(-1, "mvsdf_reg_crop: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_reg_crop: workspace too small (mvsdf_reg_crop_workspace_bytes)");
    static const int UV[3][2] = {{1, 2}, {0, 2}, {0, 1}};
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    long long* off = (long long*)(w + L.off);
    const unsigned g = mv_grid(n, CH_THREADS);
    hipLaunchKernelGGL(k_rg_crop_flags, dim3(g), dim3(CH_THREADS), 0, s, pts, (long long)n, UV[axis][0], UV[axis][1], (int)axis, axis_min, axis_max, polygon,
                       (int)nverts, keep);
    mv_scan((const unsigned char*)keep, (long long)n, off, w + L.tmp, (long long*)(w + L.tot), s);
    hipLaunchKernelGGL(k_rg_scatter, dim3(g), dim3(CH_THREADS), 0, s, pts, (long long)n, (const unsigned char*)keep, (const long long*)off, out);
    if (int rc = mv_check(hipGetLastError(), "mvsdf_reg_crop")) return rc;
    return mv_check(hipMemcpyAsync(ws, w + L.tot, MVSDF_ROWS_H_WORDS * 8, hipMemcpyDeviceToDevice, s), "mvsdf_reg_crop");
}

size_t mvsdf_reg_voxel_workspace_bytes(int64_t n) {
    RgVoxelLayout L;
    return rg_voxel_layout(n, &L) ? L.total : 0;
}

int mvsdf_reg_voxel(const double* pts, int64_t n, double voxel, void* ws, size_t ws_bytes, double* means, int32_t* counts, void* stream) {
    RgVoxelLayout L;
    if (!pts || !ws || !means || !counts || !rg_voxel_layout(n, &L) || !(voxel > 0) || !isfinite(voxel)) return mv_fail(-1, "mvsdf_reg_voxel: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_reg_voxel: workspace too small (mvsdf_reg_voxel_workspace_bytes)");
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    long long* fl = (long long*)(w + L.flags);                    // MVSDF_REG_VOXEL_H_*: the voxels (the scan's total), the error bits (int)
    unsigned long long* k[2] = {(unsigned long long*)(w + L.t.k0), (unsigned long long*)(w + L.t.k1)};
    int* v[2] = {(int*)(w + L.t.v0), (int*)(w + L.t.v1)};
    unsigned char* head = (unsigned char*)(w + L.head);
    long long* off = (long long*)(w + L.off);
    const unsigned g = mv_grid(n, CH_THREADS);
    int rc;
    if ((rc = mv_check(hipMemsetAsync(fl, 0, 4 * 8, s), "mvsdf_reg_voxel"))) return rc;
    ch_tree_frame(pts, (long long)n, w, L.t, (int*)(fl + MVSDF_REG_VOXEL_H_ERR), s);
    hipLaunchKernelGGL(k_rg_voxel_key, dim3(g), dim3(CH_THREADS), 0, s, pts, (long long)n, (const double*)(w + L.t.frame), voxel, k[0], v[0], (int*)(fl + MVSDF_REG_VOXEL_H_ERR));
    const int cur = ch_radix_sort(k, v, (long long)n, 3 * RG_VOXEL_BITS, w, L.t.rs, s);
    hipLaunchKernelGGL(k_rg_heads, dim3(g), dim3(CH_THREADS), 0, s, (const unsigned long long*)k[cur], (long long)n, head);
    mv_scan((const unsigned char*)head, (long long)n, off, w + L.tmp2, fl + MVSDF_REG_VOXEL_H_VOXELS, s);
    hipLaunchKernelGGL(k_rg_voxel_mean, dim3(g), dim3(CH_THREADS), 0, s, pts, (const unsigned long long*)k[cur], (const int*)v[cur], (const unsigned char*)head,
                       (const long long*)off, (long long)n, means, counts);
    if ((rc = mv_check(hipGetLastError(), "mvsdf_reg_voxel"))) return rc;
    return mv_check(hipMemcpyAsync(ws, fl, MVSDF_REG_VOXEL_H_WORDS * 8, hipMemcpyDeviceToDevice, s), "mvsdf_reg_voxel");
}

int mvsdf_reg_hist(const double* dist, int64_t n, const double* edges, int32_t nedges, double tau, int64_t* out, void* stream) {
    if (n < 0 || n > (1ll << 40) || (n > 0 && !dist) || !edges || !out || nedges < 2 || nedges > RG_MAX_EDGES) return mv_fail(-1, "mvsdf_reg_hist: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = mv_check(hipMemsetAsync(out, 0, (size_t)nedges * 8, s), "mvsdf_reg_hist")) return rc;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_rg_hist, dim3(mv_grid(n, CH_CHUNK)), dim3(CH_THREADS), 0, s, dist, (long long)n, edges, (int)nedges - 1, tau, (unsigned long long*)out);
    return mv_check(hipGetLastError(), "mvsdf_reg_hist");
}

}  // extern "C"
