// cloud.hip -- on-device point-cloud cleaning, the automatic cut of the fused points: the k-nearest mean distance of every point, the median
// test on it, fixed-radius connected components over the points that pass and an order-preserving compaction.  Python: mvsdf_amd/cloud.py, which
// states the definition; tests/cloud_ref.py restates it in numpy.  All arithmetic is fp64 without contraction, in the order the definition writes it.
//
// * Tree: the Morton-sorted points and the implicit 8-ary box tree of nn_tree.h, built over the cloud itself, and that header's traversals.
// * k_cl_knn: one lane per point, lanes in Morton order (lane t of workgroup b owns sorted point b * 256 + t), so a wave walks nearly the same
//   boxes.  The lane keeps its k smallest squared distances as a sorted list of CAP registers (CAP = 8 / 16 / 24 / 32, a template argument; the CAP - k
//   slots in front hold -1, below every distance, so the k-th smallest is always the last register and no index is computed at run time).  The list
//   goes through ch_knn_lane: seeded from the point's own leaf and the two beside it, then the tree is walked without a stack; a box is pruned when
//   its lower bound exceeds the k-th smallest by the relative CH_MARGIN2, every other point is compared with the metric's formula.  The k smallest
//   values are a multiset and sqrt is correctly rounded, so d has one possible bit pattern.
// * Median: the bit patterns of d (non-negative doubles order as their bits) through the 64-bit radix sort; one lane reads rank (N - 1) / 2 and
//   forms threshold = knn_ratio * m, eps = eps_ratio * m, eps * eps on the device.
// * Components: a union-find forest over sorted positions in a 32-bit parent word.  Every passed point walks the tree with the fixed bound
//   eps^2 (positions above its own end the walk: an edge is united from its higher end) and unites with each neighbour by hooking the larger
//   root under the smaller with atomicCAS; finds halve their path.  Parents only ever decrease, so every find ends.  A find or a union that
//   reaches its step bound raises a pending flag and the round is run again (the host reads the flag once per round); then every point is
//   pointed at its root, roots get the smallest input index (atomicMin) and the count (atomicAdd) of their component, the lanes of a wave that
//   share a root combined first, and the largest count decides what is kept.  Integer atomics only: labels and counts are a property of the
//   graph, not of the schedule.
// * Compaction: int64 flags, the house scan (geom_prims.h: mv_scan), a scatter in input order.
//
// Every device loop is bounded; the round loop on the host stops at CL_MAX_ROUNDS with MVSDF_PC_ERR_ROUNDS.
#include "nn_tree.h"

#define CL_MAX_ROUNDS 64
#define CL_FIND_STEPS 4096                            // parent hops of one find before it gives the round up
#define CL_UNION_TRIES 64
static_assert(MVSDF_CLOUD_H_WORDS * 8 <= CH_HDR && MVSDF_ROWS_H_WORDS * 8 <= CH_HDR, "the result words fit the header");

// flags (int): [0] error bits, [1] pending, [2] n_passed, [3] n_clusters, [4] largest, [5] n_kept
// par (double): [0] m, [1] threshold, [2] eps, [3] eps * eps
enum { CL_F_ERR = 0, CL_F_PENDING = 1, CL_F_PASSED = 2, CL_F_CLUSTERS = 3, CL_F_LARGEST = 4, CL_F_KEPT = 5, CL_F_WORDS = 8 };

// ================================================================ k nearest ================================================================
// v into the ascending list (the caller has checked v < best[CAP - 1]); compile-time indices only, so the list stays in registers
template <int CAP>
__device__ __forceinline__ void cl_insert(double (&best)[CAP], double v) {
#pragma unroll
    for (int j = CAP - 1; j > 0; --j) {
        const double lo = best[j - 1];
        best[j] = v < lo ? lo : (v < best[j] ? v : best[j]);
    }
    best[0] = v < best[0] ? v : best[0];
}

// ch_knn_lane's list: the k smallest squared distances, a multiset
template <int CAP>
struct ClList {
    double best[CAP];
    __device__ __forceinline__ double kth() const { return best[CAP - 1]; }
    __device__ __forceinline__ void offer(double v, long long) {
        if (v < best[CAP - 1]) cl_insert<CAP>(best, v);
    }
};

// d[perm[p]] = (sqrt(s_1) + ... + sqrt(s_k)) / k over the k smallest d2 from sorted point p to every other point
template <int CAP>
__global__ __launch_bounds__(CH_THREADS) void k_cl_knn(const double* __restrict__ sp, const double* __restrict__ box, ChTree T, const int* __restrict__ perm,
                                                        int k, double* __restrict__ d, int* err) {
    const long long p = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (p >= T.n) return;
    ClList<CAP> list;
#pragma unroll
    for (int j = 0; j < CAP; ++j) list.best[j] = j < CAP - k ? -1.0 : INFINITY;
    if (!ch_knn_lane(sp, box, T, p, list)) atomicOr(err, MVSDF_PC_ERR_WALK);
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < CAP; ++j)
        if (j >= CAP - k) s += sqrt(list.best[j]);
    d[perm[p]] = s / (double)k;
}

// ================================================================ median ================================================================
__global__ __launch_bounds__(CH_THREADS) void k_cl_keys(const double* __restrict__ d, long long n, unsigned long long* __restrict__ key) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i < n) key[i] = (unsigned long long)__double_as_longlong(d[i]);
}

__global__ __launch_bounds__(64) void k_cl_median(const unsigned long long* __restrict__ sorted, long long n, double knn_ratio, double eps_ratio,
                                                   double* __restrict__ par) {
    if (threadIdx.x) return;
    const double m = __longlong_as_double((long long)sorted[(n - 1) / 2]);
    const double eps = eps_ratio * m;
    par[0] = m;
    par[1] = knn_ratio * m;
    par[2] = eps;
    par[3] = eps * eps;
}

// radius_components: no distances, no median; every point passes
__global__ __launch_bounds__(64) void k_cl_set_eps(double eps, double* __restrict__ par) {
    if (threadIdx.x) return;
    par[0] = 0.0;
    par[1] = 0.0;
    par[2] = eps;
    par[3] = eps * eps;
}

// ================================================================ stage B ================================================================
// parent[p] = p where sorted point p passes (d == NULL: every point does), else -1; minidx / count start empty
__global__ __launch_bounds__(CH_THREADS) void k_cl_flag(const double* __restrict__ d, const int* __restrict__ perm, long long n, const double* __restrict__ par,
                                                         int* __restrict__ parent, int* __restrict__ minidx, int* __restrict__ count, int* flags) {
    const long long p = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    const bool pass = p < n && (!d || d[perm[p]] <= par[1]);
    if (p < n) {
        parent[p] = pass ? (int)p : -1;
        minidx[p] = INT_MAX;
        count[p] = 0;
    }
    unsigned long long b = __ballot(pass);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(flags + CL_F_PASSED, __popcll(b));
}

// ================================================================ components ================================================================
__device__ __forceinline__ int cl_ld(const int* a) { return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cl_st(int* a, int v) { __hip_atomic_store(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x with path halving, or -1 after CL_FIND_STEPS hops.  parent[y] <= y everywhere, so the hops strictly descend.
__device__ __forceinline__ int cl_find(int* parent, int x) {
    for (int step = 0; step < CL_FIND_STEPS; ++step) {
        const int px = cl_ld(parent + x);
        if (px == x) return x;
        const int ppx = cl_ld(parent + px);
        if (ppx == px) return px;
        cl_st(parent + x, ppx);
        x = ppx;
    }
    return -1;
}

// unite the sets of a and b: the larger root is hooked under the smaller.  false: a bound was reached, run the round again.
__device__ __forceinline__ bool cl_union(int* parent, int a, int b) {
    int ra = cl_find(parent, a), rb = cl_find(parent, b);
    for (int t = 0; t < CL_UNION_TRIES; ++t) {
        if (ra < 0 || rb < 0) return false;
        if (ra == rb) return true;
        if (ra < rb) {
            const int s = ra;
            ra = rb;
            rb = s;
        }
        const int old = atomicCAS(parent + ra, ra, rb);
        if (old == ra) return true;
        ra = cl_find(parent, old);                                // ra was no root any more: go on from where it points
    }
    return false;
}

// one round: every passed sorted point p unites with the passed points q < p within eps
__global__ __launch_bounds__(CH_THREADS) void k_cl_hook(const double* __restrict__ sp, const double* __restrict__ box, ChTree T, const double* __restrict__ par,
                                                         int* parent, int* flags) {
    const long long p = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (p >= T.n || cl_ld(parent + p) < 0) return;
    const double x = sp[p * 3], y = sp[p * 3 + 1], z = sp[p * 3 + 2];
    const double eps2 = par[3], bound = eps2 * CH_MARGIN2;
    int bad = 0;                                                  // a union gave up (an or, not `ok = union && ok`: that form compiles 1.4 % slower here)
    const bool walked = ch_walk(
        box, T, x, y, z, [=] { return bound; },
        [&](long long l) {
            const long long e = min(p, (l + 1) * CH_LEAF);
            for (long long q = l * CH_LEAF; q < e; ++q) {
                if (ch_d2(x, y, z, sp[q * 3], sp[q * 3 + 1], sp[q * 3 + 2]) <= eps2 && cl_ld(parent + q) >= 0) bad |= !cl_union(parent, (int)p, (int)q);
            }
        },
        p);                                                       // nodes that hold positions above p only end the walk
    if (!walked) atomicOr(flags + CL_F_ERR, MVSDF_PC_ERR_WALK);
    if (bad) atomicOr(flags + CL_F_PENDING, 1);
}

// parent[p] = its root; the root learns the smallest input index and the size of its component.  Neighbours in Morton order mostly share a root
// (one component can hold nearly every point), so a wave first combines the lanes of equal root (at most 64 turns, one per distinct root) and
// sends one atomicMin and one atomicAdd per root: integer min and sum, the same result in any grouping.
__global__ __launch_bounds__(CH_THREADS) void k_cl_roots(const int* __restrict__ perm, long long n, int* parent, int* minidx, int* count, int* flags) {
    const long long p = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    int x = p < n ? cl_ld(parent + p) : -1, idx = INT_MAX;
    if (x >= 0) {
        long long step = 0;
        for (; step <= n; ++step) {
            const int px = cl_ld(parent + x);
            if (px == x) break;
            x = px;
        }
        if (step > n) atomicOr(flags + CL_F_ERR, MVSDF_PC_ERR_WALK);
        cl_st(parent + p, x);
        idx = perm[p];
    }
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(x >= 0);
    for (int turn = 0; turn < 64 && todo; ++turn) {               // uniform over the wave: todo is the same in every lane
        const int lead = __ffsll((long long)todo) - 1;
        const int r = __shfl(x, lead);
        const bool mine = x == r;
        int v = mine ? idx : INT_MAX;
        for (int o = 32; o; o >>= 1) v = min(v, __shfl_xor(v, o));
        const unsigned long long m = __ballot(mine);
        if (lane == lead) {
            atomicMin(minidx + r, v);
            atomicAdd(count + r, __popcll(m));
        }
        todo &= ~m;
    }
}

__global__ __launch_bounds__(CH_THREADS) void k_cl_largest(long long n, const int* __restrict__ parent, const int* __restrict__ count, int* flags) {
    const long long p = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (p >= n || parent[p] != p) return;
    atomicMax(flags + CL_F_LARGEST, count[p]);
    atomicAdd(flags + CL_F_CLUSTERS, 1);
}

// labels / keep in input order (keep may be NULL); a component is kept iff count >= cluster_frac * largest, in fp64
__global__ __launch_bounds__(CH_THREADS) void k_cl_out(const int* __restrict__ perm, long long n, const int* __restrict__ parent, const int* __restrict__ minidx,
                                                        const int* __restrict__ count, double cluster_frac, int* __restrict__ labels,
                                                        unsigned char* __restrict__ keep, int* flags) {
    const long long p = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    bool k = false;
    if (p < n) {
        const int r = parent[p], i = perm[p];
        k = r >= 0 && (double)count[r] >= cluster_frac * (double)flags[CL_F_LARGEST];
        labels[i] = r >= 0 ? minidx[r] : -1;
        if (keep) keep[i] = k;
    }
    unsigned long long b = __ballot(k);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(flags + CL_F_KEPT, __popcll(b));
}

__global__ __launch_bounds__(64) void k_cl_header(const int* __restrict__ flags, const double* __restrict__ par, long long rounds, long long* __restrict__ hdr) {
    if (threadIdx.x) return;
    hdr[MVSDF_CLOUD_H_PASSED] = flags[CL_F_PASSED];
    hdr[MVSDF_CLOUD_H_CLUSTERS] = flags[CL_F_CLUSTERS];
    hdr[MVSDF_CLOUD_H_LARGEST] = flags[CL_F_LARGEST];
    hdr[MVSDF_CLOUD_H_KEPT] = flags[CL_F_KEPT];
    hdr[MVSDF_CLOUD_H_M] = __double_as_longlong(par[0]);
    hdr[MVSDF_CLOUD_H_THRESHOLD] = __double_as_longlong(par[1]);
    hdr[MVSDF_CLOUD_H_EPS] = __double_as_longlong(par[2]);
    hdr[MVSDF_CLOUD_H_ROUNDS] = rounds;
    hdr[MVSDF_CLOUD_H_ERR] = flags[CL_F_ERR];
}

// ================================================================ compaction ================================================================
__global__ __launch_bounds__(CH_THREADS) void k_cl_keep_flags(const unsigned char* __restrict__ keep, long long n, long long* __restrict__ f) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i < n) f[i] = keep[i] != 0;
}

// row off[i] of the outputs = row i of the inputs where keep[i]; colors / a / b may be NULL
__global__ __launch_bounds__(CH_THREADS) void k_cl_compact(const double* __restrict__ P, const unsigned char* __restrict__ colors, const int* __restrict__ a,
                                                            const int* __restrict__ b, const unsigned char* __restrict__ keep, long long n,
                                                            const long long* __restrict__ off, long long cap, double* __restrict__ oP,
                                                            unsigned char* __restrict__ ocolors, int* __restrict__ oa, int* __restrict__ ob) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const long long o = off[i];
    if (o >= cap) return;
    for (int c = 0; c < 3; ++c) oP[o * 3 + c] = P[i * 3 + c];
    if (colors)
        for (int c = 0; c < 3; ++c) ocolors[o * 3 + c] = colors[i * 3 + c];
    if (a) oa[o] = a[i];
    if (b) ob[o] = b[i];
}

// ================================================================ host ================================================================
struct ClLayout {
    ChTreeLayout t;
    size_t v2, parent, minidx, count, flags, par, total;
};

static bool cl_layout(long long n, ClLayout* L) {
    if (n < 2 || n > INT_MAX) return false;
    WsCursor c{CH_HDR};
    if (!ch_tree_layout(n, c, &L->t)) return false;
    L->v2 = c.take((size_t)n * 4);  // the median sort carries values nobody reads: the one of v0 / v1 without the permutation and this
    L->parent = c.take((size_t)n * 4);
    L->minidx = c.take((size_t)n * 4);
    L->count = c.take((size_t)n * 4);
    L->flags = c.take(CL_F_WORDS * 4);
    L->par = c.take(4 * 8);
    L->total = c.o;
    return true;
}

struct ClCompactLayout {
    size_t f, tmp, tot, total;
};

static bool cl_compact_layout(long long n, ClCompactLayout* L) {
    if (n < 1 || n > INT_MAX) return false;
    WsCursor c{CH_HDR};
    L->f = c.take((size_t)n * 8);
    L->tmp = c.take(mv_scan_tmp_bytes(n));
    L->tot = c.take(8);
    L->total = c.o;
    return true;
}

static int cl_fail_header(void* ws, long long err, hipStream_t s, const char* what) {
    long long hdr[MVSDF_CLOUD_H_WORDS] = {};
    hdr[MVSDF_CLOUD_H_ERR] = err;
    return mv_write_header(ws, hdr, MVSDF_CLOUD_H_WORDS, s, what);
}

// flags zeroed, the frame, one header read for MVSDF_PC_ERR_FINITE, the tree -> 0 and *perm, or nonzero after the failure header / a HIP error (*done set)
static int cl_begin(const double* pts, long long n, char* w, const ClLayout& L, hipStream_t s, const char* what, const int** perm, bool* done) {
    int* fl = (int*)(w + L.flags);
    int rc;
    *done = true;
    if ((rc = mv_check(hipMemsetAsync(fl, 0, CL_F_WORDS * 4, s), what))) return rc;
    const ChBuilt tree = ch_tree_begin(pts, n, w, L.t, fl + CL_F_ERR, s, what);
    if (tree.rc) return tree.rc;
    if (tree.err) return cl_fail_header(w, tree.err, s, what);
    *perm = tree.perm;
    *done = false;
    return 0;
}

static void cl_knn(long long n, int k, char* w, const ClLayout& L, const int* perm, double* d, hipStream_t s) {
    const double* sp = (const double*)(w + L.t.sp);
    const double* box = (const double*)(w + L.t.box);
    int* err = (int*)(w + L.flags) + CL_F_ERR;
    const dim3 g(mv_grid(n, CH_THREADS)), b(CH_THREADS);
    ch_knn_dispatch(k, [&](auto cap) { hipLaunchKernelGGL(k_cl_knn<decltype(cap)::value>, g, b, 0, s, sp, box, L.t.T, perm, k, d, err); });
}

// stages B (d == NULL: every point passes) and C with par already on the device; leaves the header.  One header read per round.
static int cl_components(const double* d, long long n, double cluster_frac, char* w, const ClLayout& L, const int* perm, int32_t* labels, uint8_t* keep,
                         hipStream_t s, const char* what) {
    const double* sp = (const double*)(w + L.t.sp);
    const double* box = (const double*)(w + L.t.box);
    int* fl = (int*)(w + L.flags);
    const double* par = (const double*)(w + L.par);
    int* parent = (int*)(w + L.parent);
    int* minidx = (int*)(w + L.minidx);
    int* count = (int*)(w + L.count);
    const dim3 g(mv_grid(n, CH_THREADS)), b(CH_THREADS);
    int rc;
    hipLaunchKernelGGL(k_cl_flag, g, b, 0, s, d, perm, n, par, parent, minidx, count, fl);
    long long rounds = 0;
    for (;;) {
        if (rounds >= CL_MAX_ROUNDS) return cl_fail_header(w, MVSDF_PC_ERR_ROUNDS, s, what);
        if ((rc = mv_check(hipMemsetAsync(fl + CL_F_PENDING, 0, 4, s), what))) return rc;
        hipLaunchKernelGGL(k_cl_hook, g, b, 0, s, sp, box, L.t.T, par, parent, fl);
        if ((rc = mv_check(hipGetLastError(), what))) return rc;
        int r[2];
        if ((rc = mv_read(r, fl, sizeof(r), s, what))) return rc;
        ++rounds;
        if (r[CL_F_ERR]) return cl_fail_header(w, r[CL_F_ERR], s, what);
        if (!r[CL_F_PENDING]) break;
    }
    hipLaunchKernelGGL(k_cl_roots, g, b, 0, s, perm, n, parent, minidx, count, fl);
    hipLaunchKernelGGL(k_cl_largest, g, b, 0, s, n, (const int*)parent, (const int*)count, fl);
    hipLaunchKernelGGL(k_cl_out, g, b, 0, s, perm, n, (const int*)parent, (const int*)minidx, (const int*)count, cluster_frac, labels, keep, fl);
    hipLaunchKernelGGL(k_cl_header, dim3(1), dim3(64), 0, s, (const int*)fl, par, rounds, (long long*)w);
    return mv_check(hipGetLastError(), what);
}

static bool cl_ratio(double x) { return isfinite(x) && x > 0; }

extern "C" {

size_t mvsdf_cloud_clean_workspace_bytes(int64_t n) {
    ClLayout L;
    return cl_layout(n, &L) ? L.total : 0;
}

size_t mvsdf_cloud_compact_workspace_bytes(int64_t n) {
    ClCompactLayout L;
    return cl_compact_layout(n, &L) ? L.total : 0;
}

int mvsdf_cloud_knn(const double* pts, int64_t n, int32_t k, void* ws, size_t ws_bytes, double* d, void* stream) {
    const char* what = "mvsdf_cloud_knn";
    ClLayout L;
    if (!pts || !ws || !d || k < 1 || k > MVSDF_PC_MAX_K || n < (int64_t)k + 1 || !cl_layout(n, &L)) return mv_fail(-1, "mvsdf_cloud_knn: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_cloud_knn: workspace too small (mvsdf_cloud_clean_workspace_bytes)");
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    const int* perm = nullptr;
    bool done;
    int rc = cl_begin(pts, n, w, L, s, what, &perm, &done);
    if (rc || done) return rc;
    cl_knn(n, k, w, L, perm, d, s);
    if ((rc = mv_check(hipMemsetAsync(w + L.par, 0, 4 * 8, s), what))) return rc;
    hipLaunchKernelGGL(k_cl_header, dim3(1), dim3(64), 0, s, (const int*)(w + L.flags), (const double*)(w + L.par), 0ll, (long long*)w);
    return mv_check(hipGetLastError(), what);
}

int mvsdf_cloud_components(const double* pts, int64_t n, double eps, void* ws, size_t ws_bytes, int32_t* labels, void* stream) {
    const char* what = "mvsdf_cloud_components";
    ClLayout L;
    if (!pts || !ws || !labels || !cl_ratio(eps) || !cl_layout(n, &L)) return mv_fail(-1, "mvsdf_cloud_components: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_cloud_components: workspace too small (mvsdf_cloud_clean_workspace_bytes)");
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    const int* perm = nullptr;
    bool done;
    int rc = cl_begin(pts, n, w, L, s, what, &perm, &done);
    if (rc || done) return rc;
    hipLaunchKernelGGL(k_cl_set_eps, dim3(1), dim3(64), 0, s, eps, (double*)(w + L.par));
    return cl_components(nullptr, n, 1.0, w, L, perm, labels, nullptr, s, what);
}

int mvsdf_cloud_clean(const double* pts, int64_t n, int32_t k, double knn_ratio, double eps_ratio, double cluster_frac, void* ws, size_t ws_bytes,
                      double* d, int32_t* labels, uint8_t* keep, void* stream) {
    const char* what = "mvsdf_cloud_clean";
    ClLayout L;
    if (!pts || !ws || !d || !labels || !keep || k < 1 || k > MVSDF_PC_MAX_K || n < (int64_t)k + 1 || !cl_ratio(knn_ratio) || !cl_ratio(eps_ratio) ||
        !cl_ratio(cluster_frac) || cluster_frac > 1.0 || !cl_layout(n, &L))
        return mv_fail(-1, "mvsdf_cloud_clean: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_cloud_clean: workspace too small (mvsdf_cloud_clean_workspace_bytes)");
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    const int* perm = nullptr;
    bool done;
    int rc = cl_begin(pts, n, w, L, s, what, &perm, &done);
    if (rc || done) return rc;
    cl_knn(n, k, w, L, perm, d, s);
    // the median: perm lives in one of v0 / v1, so the sort of d's bits carries the other and v2 along
    unsigned long long* keys[2] = {(unsigned long long*)(w + L.t.k0), (unsigned long long*)(w + L.t.k1)};
    int* vals[2] = {(int*)(w + (L.t.perm == L.t.v0 ? L.t.v1 : L.t.v0)), (int*)(w + L.v2)};
    hipLaunchKernelGGL(k_cl_keys, dim3(mv_grid(n, CH_THREADS)), dim3(CH_THREADS), 0, s, (const double*)d, (long long)n, keys[0]);
    const int cur = ch_radix_sort(keys, vals, n, 64, w, L.t.rs, s);
    hipLaunchKernelGGL(k_cl_median, dim3(1), dim3(64), 0, s, (const unsigned long long*)keys[cur], (long long)n, knn_ratio, eps_ratio, (double*)(w + L.par));
    return cl_components(d, n, cluster_frac, w, L, perm, labels, keep, s, what);
}

int mvsdf_cloud_compact(const double* pts, const uint8_t* colors, const int32_t* a, const int32_t* b, const uint8_t* keep, int64_t n, void* ws,
                        size_t ws_bytes, double* out_pts, uint8_t* out_colors, int32_t* out_a, int32_t* out_b, int64_t cap, void* stream) {
    const char* what = "mvsdf_cloud_compact";
    ClCompactLayout L;
    if (!pts || !keep || !ws || cap < 0 || (cap > 0 && !out_pts) || (colors && cap > 0 && !out_colors) || (a && cap > 0 && !out_a) ||
        (b && cap > 0 && !out_b) || !cl_compact_layout(n, &L))
        return mv_fail(-1, "mvsdf_cloud_compact: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_cloud_compact: workspace too small (mvsdf_cloud_compact_workspace_bytes)");
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    long long* f = (long long*)(w + L.f);
    const dim3 g(mv_grid(n, CH_THREADS)), blk(CH_THREADS);
    hipLaunchKernelGGL(k_cl_keep_flags, g, blk, 0, s, keep, (long long)n, f);
    mv_scan(f, n, f, w + L.tmp, (long long*)(w + L.tot), s);
    hipLaunchKernelGGL(k_cl_compact, g, blk, 0, s, pts, colors, a, b, keep, (long long)n, (const long long*)f, (long long)cap, out_pts, out_colors, out_a,
                       out_b);
    if (int rc = mv_check(hipGetLastError(), what)) return rc;
    return mv_check(hipMemcpyAsync(ws, w + L.tot, MVSDF_ROWS_H_WORDS * 8, hipMemcpyDeviceToDevice, s), what);
}

}  // extern "C"
