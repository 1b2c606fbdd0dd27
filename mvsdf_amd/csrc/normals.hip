// normals.hip -- normals for unoriented clouds on the device: which points are the k nearest of every point, the eigenproblem of each neighbourhood and a
// globally consistent sign.  Python: mvsdf_amd/normals.py, which states the definition; tests/normals_ref.py restates it in numpy.  All arithmetic is
// fp64 without contraction, in the order the definition writes it.
//
// * k_nr_knn: k_cl_knn's lane (cloud.hip; both go through nn_tree.h's ch_knn_lane) with a list of pairs.  One lane per Morton-sorted point; the list
//   is CAP doubles and CAP ints (CAP = 8 / 16 / 24 / 32, a template argument) ordered by (d2, input index), the CAP - k slots in front hold (-1, -1),
//   below every pair, so the k-th pair is always the last slot and every list index is a compile-time one.  The seeds are the point's own leaf and
//   the two beside it, the walk is stackless; a box is pruned when its lower bound exceeds the last slot's d2 by the relative CH_MARGIN2 (inclusive: a box at exactly that
//   distance may hold a tie of lower index), every other point is compared as a pair.  Each point is met once, so no pair is inserted twice and the
//   row is one array, not a multiset.
// * k_nr_pca: one lane per point in input order reads its row: mean and covariance of the offsets, NR_SWEEPS cyclic Jacobi sweeps over a full
//   symmetric 3 x 3 in registers, the column of the smallest diagonal entry.
// * Orientation: Boruvka rounds over the symmetric closure of the rows.  state[i] = root << 1 | flip of i against its root, flat at every round's
//   start.  k_nr_best_a / k_nr_best_e: every lane offers each of its k edges to the components of both ends; atomicMax on the bits of |dot| + 1
//   (0 = no edge), then atomicMin on lo << 32 | hi among the edges that reach it.  k_nr_hook: every root with an edge hooks under the other end's root
//   (link[r] = root << 1 | flip); two roots that chose the same edge keep the lower one.  The order of the edges is total, so the hooks form a
//   forest.  k_nr_jump flattens it in place: a link word is read and written whole (one 32-bit atomic), so whatever a lane reads is a true
//   (ancestor, flip against it) pair and hops only ascend; a lane that reaches NR_JUMP_STEPS raises pending and the launch is repeated.
//   k_nr_apply folds the links into state.  The host reads {error bits, pending, hooks} once per round and stops at the first round without a hook.
// * Component sign: smallest index, highest point along `up` (the bits of the height, then the index among those that reach it) and the view votes
//   are integer atomics, the lanes of a wave that share a root combined first (k_cl_roots' scheme).
//
// Every device loop is bounded; the round loop on the host stops at NR_MAX_ROUNDS with MVSDF_PC_ERR_ROUNDS.  Integer atomics only.
#include "nn_tree.h"

#define NR_SWEEPS 6
#define NR_MAX_ROUNDS 64
#define NR_MAX_JUMPS 64                               // repeats of the jump launch in one round
#define NR_JUMP_STEPS 4096                            // hops of one lane before it gives the launch up

typedef unsigned long long nr_u64;
static_assert(MVSDF_NR_ORIENT_H_WORDS * 8 <= CH_HDR && MVSDF_ERRW_H_WORDS <= MVSDF_NR_ORIENT_H_WORDS, "the result words fit the header");

// flags (int): [0] error bits, [1] pending, [2] hooks of the round, [3] n_components
enum { NR_F_ERR = 0, NR_F_PENDING = 1, NR_F_HOOKS = 2, NR_F_COMPONENTS = 3, NR_F_WORDS = 8 };

// ================================================================ k nearest, with indices ================================================================
__device__ __forceinline__ bool nr_less(double va, int ia, double vb, int ib) { return va < vb || (va == vb && ia < ib); }

// (v, id) into the ascending list (the caller has checked that it is below the last slot); compile-time indices only
template <int CAP>
__device__ __forceinline__ void nr_insert(double (&bd)[CAP], int (&bi)[CAP], double v, int id) {
#pragma unroll
    for (int j = CAP - 1; j > 0; --j) {
        const double ld = bd[j - 1];
        const int li = bi[j - 1];
        const bool below_prev = nr_less(v, id, ld, li), below_here = nr_less(v, id, bd[j], bi[j]);
        bd[j] = below_prev ? ld : (below_here ? v : bd[j]);
        bi[j] = below_prev ? li : (below_here ? id : bi[j]);
    }
    const bool first = nr_less(v, id, bd[0], bi[0]);
    bd[0] = first ? v : bd[0];
    bi[0] = first ? id : bi[0];
}

// ch_knn_lane's list: the k smallest pairs (d2, input index); the permutation is read only for a candidate not above the k-th distance
template <int CAP>
struct NrList {
    double bd[CAP];
    int bi[CAP];
    const int* __restrict__ perm;
    __device__ __forceinline__ double kth() const { return bd[CAP - 1]; }
    __device__ __forceinline__ void offer(double v, long long q) {
        if (v <= bd[CAP - 1]) {
            const int id = perm[q];
            if (nr_less(v, id, bd[CAP - 1], bi[CAP - 1])) nr_insert<CAP>(bd, bi, v, id);
        }
    }
};

// row perm[p] of idx (and of d2 when given) = the k pairs (d2, input index) smallest from sorted point p to every other point, ascending
template <int CAP>
__global__ __launch_bounds__(CH_THREADS) void k_nr_knn(const double* __restrict__ sp, const double* __restrict__ box, ChTree T, const int* __restrict__ perm,
                                                        int k, int* __restrict__ idx, double* __restrict__ d2, int* err) {
    const long long p = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (p >= T.n) return;
    NrList<CAP> list;
    list.perm = perm;
#pragma unroll
    for (int j = 0; j < CAP; ++j) {
        list.bd[j] = j < CAP - k ? -1.0 : INFINITY;
        list.bi[j] = j < CAP - k ? -1 : INT_MAX;
    }
    if (!ch_knn_lane(sp, box, T, p, list)) atomicOr(err, MVSDF_PC_ERR_WALK);
    const long long row = (long long)perm[p] * k;
#pragma unroll
    for (int j = 0; j < CAP; ++j)
        if (j >= CAP - k) {
            idx[row + (j - (CAP - k))] = list.bi[j];
            if (d2) d2[row + (j - (CAP - k))] = list.bd[j];
        }
}

// ================================================================ the eigenproblem ================================================================
// one Jacobi rotation of the pair (P, Q): horn_rotation's formula (registration.py) on a 3 x 3
template <int P, int Q>
__device__ __forceinline__ void nr_rotate(double (&A)[3][3], double (&V)[3][3]) {
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double xp = A[k][P], xq = A[k][Q];
        A[k][P] = c * xp - s * xq;
        A[k][Q] = s * xp + c * xq;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double xp = A[P][k], xq = A[Q][k];
        A[P][k] = c * xp - s * xq;
        A[Q][k] = s * xp + c * xq;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double xp = V[k][P], xq = V[k][Q];
        V[k][P] = c * xp - s * xq;
        V[k][Q] = s * xp + c * xq;
    }
    A[P][Q] = 0.0;
    A[Q][P] = 0.0;
}

__global__ __launch_bounds__(CH_THREADS) void k_nr_pca(const double* __restrict__ pts, long long n, const int* __restrict__ idx, int k,
                                                        double* __restrict__ normals, double* __restrict__ variation) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n) return;
    const double px = pts[i * 3], py = pts[i * 3 + 1], pz = pts[i * 3 + 2];
    const int* __restrict__ row = idx + i * k;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int j = 0; j < k; ++j) {
        const long long q = row[j];
        sx = sx + (pts[q * 3] - px);
        sy = sy + (pts[q * 3 + 1] - py);
        sz = sz + (pts[q * 3 + 2] - pz);
    }
    const double cnt = (double)(k + 1);
    const double mx = sx / cnt, my = sy / cnt, mz = sz / cnt;
    double dx = 0.0 - mx, dy = 0.0 - my, dz = 0.0 - mz;                 // u_0 = 0
    double cxx = 0.0 + dx * dx, cxy = 0.0 + dx * dy, cxz = 0.0 + dx * dz, cyy = 0.0 + dy * dy, cyz = 0.0 + dy * dz, czz = 0.0 + dz * dz;
    for (int j = 0; j < k; ++j) {
        const long long q = row[j];
        dx = (pts[q * 3] - px) - mx;
        dy = (pts[q * 3 + 1] - py) - my;
        dz = (pts[q * 3 + 2] - pz) - mz;
        cxx = cxx + dx * dx;
        cxy = cxy + dx * dy;
        cxz = cxz + dx * dz;
        cyy = cyy + dy * dy;
        cyz = cyz + dy * dz;
        czz = czz + dz * dz;
    }
    double A[3][3] = {{cxx, cxy, cxz}, {cxy, cyy, cyz}, {cxz, cyz, czz}};
    double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
#pragma unroll
    for (int sweep = 0; sweep < NR_SWEEPS; ++sweep) {
        nr_rotate<0, 1>(A, V);
        nr_rotate<0, 2>(A, V);
        nr_rotate<1, 2>(A, V);
    }
    const double l0 = A[0][0], l1 = A[1][1], l2 = A[2][2];
    const double v00 = V[0][0], v01 = V[0][1], v02 = V[0][2], v10 = V[1][0], v11 = V[1][1], v12 = V[1][2], v20 = V[2][0], v21 = V[2][1], v22 = V[2][2];
    const bool c1 = l1 < l0;                                            // the smallest diagonal entry, ties to the lower column
    const double lm1 = c1 ? l1 : l0;
    const bool c2 = l2 < lm1;
    const double lm = c2 ? l2 : lm1;
    double vx = c2 ? v02 : (c1 ? v01 : v00), vy = c2 ? v12 : (c1 ? v11 : v10), vz = c2 ? v22 : (c1 ? v21 : v20);
    const double nrm = sqrt((vx * vx + vy * vy) + vz * vz);
    vx = vx / nrm;
    vy = vy / nrm;
    vz = vz / nrm;
    double big = vx, mag = fabs(vx);
    if (fabs(vy) > mag) {
        big = vy;
        mag = fabs(vy);
    }
    if (fabs(vz) > mag) big = vz;
    if (big < 0.0) {
        vx = -vx;
        vy = -vy;
        vz = -vz;
    }
    normals[i * 3] = vx;
    normals[i * 3 + 1] = vy;
    normals[i * 3 + 2] = vz;
    const double den = (l0 + l1) + l2;
    variation[i] = den == 0.0 ? 0.0 : lm / den;
}

// ================================================================ orientation ================================================================
__device__ __forceinline__ unsigned nr_ld(const unsigned* a) { return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void nr_st(unsigned* a, unsigned v) { __hip_atomic_store(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ double nr_dot(const double* __restrict__ a, const double* __restrict__ b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// every point its own root; the finite and range checks of the whole call
__global__ __launch_bounds__(CH_THREADS) void k_nr_init(const double* __restrict__ pts, const double* __restrict__ nrm, const int* __restrict__ nbr, long long n,
                                                         int k, unsigned* __restrict__ state, unsigned* __restrict__ link, int* __restrict__ minidx,
                                                         nr_u64* __restrict__ hkey, int* __restrict__ hidx, nr_u64* __restrict__ neg, nr_u64* __restrict__ pos,
                                                         int* flags) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n) return;
    state[i] = (unsigned)i << 1;
    link[i] = (unsigned)i << 1;
    minidx[i] = INT_MAX;
    hkey[i] = 0;
    hidx[i] = INT_MAX;
    neg[i] = 0;
    pos[i] = 0;
    int bad = 0;
    if (!ch_finite3(pts + i * 3)) bad |= MVSDF_PC_ERR_FINITE;
    if (!ch_finite3(nrm + i * 3)) bad |= MVSDF_PC_ERR_NORMAL;
    for (int j = 0; j < k; ++j) {
        const int q = nbr[i * k + j];
        if (q < 0 || q >= n) bad |= MVSDF_PC_ERR_INDEX;
    }
    if (bad) atomicOr(flags + NR_F_ERR, bad);
}

__global__ __launch_bounds__(CH_THREADS) void k_nr_round_begin(const unsigned* __restrict__ state, long long n, nr_u64* __restrict__ best_a,
                                                                nr_u64* __restrict__ best_e) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n || (state[i] >> 1) != (unsigned)i) return;
    best_a[i] = 0;
    best_e[i] = CH_EMPTY;
}

// pass 1: the largest |dot| (its bits + 1) among the edges that leave each component
__global__ __launch_bounds__(CH_THREADS) void k_nr_best_a(const double* __restrict__ nrm, const int* __restrict__ nbr, long long n, int k,
                                                           const unsigned* __restrict__ state, nr_u64* __restrict__ best_a) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned ci = state[i] >> 1;
    for (int j = 0; j < k; ++j) {
        const long long q = nbr[i * k + j];
        if (q < 0 || q >= n || q == i) continue;
        const unsigned cq = state[q] >> 1;
        if (cq == ci) continue;
        const nr_u64 a = (nr_u64)__double_as_longlong(fabs(nr_dot(nrm + i * 3, nrm + q * 3))) + 1;
        atomicMax(best_a + ci, a);
        atomicMax(best_a + cq, a);
    }
}

// pass 2: among the edges that reach it, the smallest lo << 32 | hi
__global__ __launch_bounds__(CH_THREADS) void k_nr_best_e(const double* __restrict__ nrm, const int* __restrict__ nbr, long long n, int k,
                                                           const unsigned* __restrict__ state, const nr_u64* __restrict__ best_a, nr_u64* __restrict__ best_e) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned ci = state[i] >> 1;
    for (int j = 0; j < k; ++j) {
        const long long q = nbr[i * k + j];
        if (q < 0 || q >= n || q == i) continue;
        const unsigned cq = state[q] >> 1;
        if (cq == ci) continue;
        const nr_u64 a = (nr_u64)__double_as_longlong(fabs(nr_dot(nrm + i * 3, nrm + q * 3))) + 1;
        const nr_u64 e = (nr_u64)min(i, q) << 32 | (nr_u64)max(i, q);
        if (a == best_a[ci]) atomicMin(best_e + ci, e);
        if (a == best_a[cq]) atomicMin(best_e + cq, e);
    }
}

// every root with an edge hooks under the root of the edge's other end; of two roots that chose the same edge the lower stays
__global__ __launch_bounds__(CH_THREADS) void k_nr_hook(const double* __restrict__ nrm, long long n, const unsigned* __restrict__ state,
                                                         const nr_u64* __restrict__ best_e, unsigned* __restrict__ link, int* flags) {
    const long long r = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    bool hooked = false;
    if (r < n && (state[r] >> 1) == (unsigned)r) {
        const nr_u64 e = best_e[r];
        if (e != CH_EMPTY) {
            const long long lo = (long long)(e >> 32), hi = (long long)(e & 0xffffffffull);
            const unsigned slo = state[lo], shi = state[hi];
            const unsigned r2 = (slo >> 1) == (unsigned)r ? shi >> 1 : slo >> 1;
            if (!(best_e[r2] == e && r < (long long)r2)) {
                const unsigned f = ((slo ^ shi) & 1u) ^ (nr_dot(nrm + lo * 3, nrm + hi * 3) < 0.0 ? 1u : 0u);
                nr_st(link + r, r2 << 1 | f);
                hooked = true;
            }
        }
    }
    const nr_u64 b = __ballot(hooked);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(flags + NR_F_HOOKS, __popcll(b));
}

// pointer jumping over the roots of the round's start: link[r] ends at a root that stayed, with the flip of r against it
__global__ __launch_bounds__(CH_THREADS) void k_nr_jump(long long n, const unsigned* __restrict__ state, unsigned* link, int* flags) {
    const long long r = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (r >= n || (state[r] >> 1) != (unsigned)r) return;
    int step = 0;
    for (; step < NR_JUMP_STEPS; ++step) {
        const unsigned w = nr_ld(link + r);
        const unsigned p = w >> 1;
        if (p == (unsigned)r) return;
        const unsigned wp = nr_ld(link + p);
        if ((wp >> 1) == p) return;
        nr_st(link + r, (wp & ~1u) | ((w ^ wp) & 1u));
    }
    atomicOr(flags + NR_F_PENDING, 1);
}

__global__ __launch_bounds__(CH_THREADS) void k_nr_apply(long long n, unsigned* __restrict__ state, const unsigned* __restrict__ link) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned s = state[i];
    const unsigned w = link[s >> 1];
    state[i] = (w & ~1u) | ((s ^ w) & 1u);
}

// k_nr_apply writes state[i] from link[state[i] >> 1] alone, but k_nr_jump tells a root by state: a hooked root's link must be taken back once
// every point has been folded
__global__ __launch_bounds__(CH_THREADS) void k_nr_unlink(long long n, const unsigned* __restrict__ state, unsigned* __restrict__ link) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i < n && (link[i] >> 1) != (unsigned)i) link[i] = (unsigned)i << 1;
}

// a non-negative order of the doubles as integers: -0 counts as +0
__device__ __forceinline__ nr_u64 nr_order_key(double h) {
    if (h == 0.0) h = 0.0;
    const nr_u64 b = (nr_u64)__double_as_longlong(h);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// the seeing views of point i with n . (c_v - p) < 0 and > 0
__device__ __forceinline__ void nr_votes(const double* __restrict__ pts, const double* __restrict__ nrm, const double* __restrict__ centers,
                                         const nr_u64* __restrict__ bits, int nw, int V, long long i, unsigned* neg, unsigned* pos) {
    const double px = pts[i * 3], py = pts[i * 3 + 1], pz = pts[i * 3 + 2];
    const double nx = nrm[i * 3], ny = nrm[i * 3 + 1], nz = nrm[i * 3 + 2];
    unsigned a = 0, b = 0;
    for (int w = 0; w < nw; ++w) {
        nr_u64 word = bits[i * nw + w];
        for (int t = 0; t < 64 && word; ++t) {
            const int v = w * 64 + __ffsll((long long)word) - 1;
            word &= word - 1;
            if (v >= V) break;
            const double s = (nx * (centers[v * 3] - px) + ny * (centers[v * 3 + 1] - py)) + nz * (centers[v * 3 + 2] - pz);
            a += s < 0.0;
            b += s > 0.0;
        }
    }
    *neg = a;
    *pos = b;
}

// per root: the smallest index, the largest height key, the votes (those of a flipped point change sides).  The lanes of a wave that share a root
// are combined first.
__global__ __launch_bounds__(CH_THREADS) void k_nr_gather(const double* __restrict__ pts, const double* __restrict__ nrm, long long n,
                                                           const unsigned* __restrict__ state, double ux, double uy, double uz,
                                                           const double* __restrict__ centers, const nr_u64* __restrict__ bits, int nw, int V,
                                                           int* minidx, nr_u64* hkey, nr_u64* neg, nr_u64* pos, int* flags) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    const bool live = i < n;
    unsigned root = 0xffffffffu, vn = 0, vp = 0;
    nr_u64 key = 0;
    if (live) {
        const unsigned s = state[i];
        root = s >> 1;
        key = nr_order_key((pts[i * 3] * ux + pts[i * 3 + 1] * uy) + pts[i * 3 + 2] * uz);
        if (centers) {
            unsigned a, b;
            nr_votes(pts, nrm, centers, bits, nw, V, i, &a, &b);
            vn = (s & 1u) ? b : a;
            vp = (s & 1u) ? a : b;
        }
    }
    const nr_u64 roots = __ballot(live && root == (unsigned)i);
    const int lane = threadIdx.x & 63;
    if (lane == 0 && roots) atomicAdd(flags + NR_F_COMPONENTS, __popcll(roots));
    nr_u64 todo = __ballot(live);
    for (int turn = 0; turn < 64 && todo; ++turn) {               // uniform over the wave
        const int lead = __ffsll((long long)todo) - 1;
        const unsigned r = __shfl(root, lead);
        const bool mine = live && root == r;
        int mi = mine ? (int)i : INT_MAX;
        nr_u64 mk = mine ? key : 0;
        nr_u64 sn = mine ? vn : 0, spos = mine ? vp : 0;
        for (int o = 32; o; o >>= 1) {
            mi = min(mi, __shfl_xor(mi, o));
            const nr_u64 ok = __shfl_xor(mk, o);
            mk = ok > mk ? ok : mk;
            sn += __shfl_xor(sn, o);
            spos += __shfl_xor(spos, o);
        }
        if (lane == lead) {
            atomicMin(minidx + r, mi);
            atomicMax(hkey + r, mk);
            if (sn) atomicAdd(neg + r, sn);
            if (spos) atomicAdd(pos + r, spos);
        }
        todo &= ~__ballot(mine);
    }
}

// the lowest index among the points that reach their component's largest height
__global__ __launch_bounds__(CH_THREADS) void k_nr_highest(const double* __restrict__ pts, long long n, const unsigned* __restrict__ state, double ux, double uy,
                                                            double uz, const nr_u64* __restrict__ hkey, int* hidx) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned root = state[i] >> 1;
    if (nr_order_key((pts[i * 3] * ux + pts[i * 3 + 1] * uy) + pts[i * 3 + 2] * uz) == hkey[root]) atomicMin(hidx + root, (int)i);
}

__global__ __launch_bounds__(CH_THREADS) void k_nr_orient_out(const double* __restrict__ nrm, long long n, const unsigned* __restrict__ state, double ux, double uy,
                                                               double uz, bool views, const int* __restrict__ minidx, const int* __restrict__ hidx,
                                                               const nr_u64* __restrict__ neg, const nr_u64* __restrict__ pos, double* __restrict__ out,
                                                               int* __restrict__ labels) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned s = state[i], root = s >> 1;
    const long long h = hidx[root] < n ? hidx[root] : i;              // (always set: some point of the component holds its largest height)
    const double d = (nrm[h * 3] * ux + nrm[h * 3 + 1] * uy) + nrm[h * 3 + 2] * uz;
    bool turn = ((state[h] & 1u) != 0) != (d < 0.0);                    // the reference point ends as it came iff its product with up is >= 0
    if (views && neg[root] != pos[root]) turn = neg[root] > pos[root];
    const bool flip = ((s & 1u) != 0) != turn;
    for (int c = 0; c < 3; ++c) out[i * 3 + c] = flip ? -nrm[i * 3 + c] : nrm[i * 3 + c];
    labels[i] = minidx[root];
}

__global__ __launch_bounds__(64) void k_nr_orient_header(const int* __restrict__ flags, long long rounds, long long* __restrict__ hdr) {
    if (threadIdx.x) return;
    hdr[MVSDF_NR_ORIENT_H_COMPONENTS] = flags[NR_F_COMPONENTS];
    hdr[MVSDF_NR_ORIENT_H_ROUNDS] = rounds;
    hdr[MVSDF_NR_ORIENT_H_ERR] = flags[NR_F_ERR];
}

__global__ __launch_bounds__(64) void k_nr_knn_header(const int* __restrict__ flags, long long* __restrict__ hdr) {
    if (threadIdx.x) return;
    hdr[MVSDF_ERRW_H_ERR] = flags[NR_F_ERR];
}

// each normal flipped iff more of its own seeing views lie behind it than before it; hdr = the error word
__global__ __launch_bounds__(CH_THREADS) void k_nr_to_views(const double* __restrict__ pts, const double* __restrict__ nrm, long long n,
                                                             const double* __restrict__ centers, const nr_u64* __restrict__ bits, int nw, int V,
                                                             double* __restrict__ out, nr_u64* hdr) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n) return;
    int bad = 0;
    if (!ch_finite3(pts + i * 3)) bad |= MVSDF_PC_ERR_FINITE;
    if (!ch_finite3(nrm + i * 3)) bad |= MVSDF_PC_ERR_NORMAL;
    if (bad) atomicOr(hdr, (nr_u64)bad);
    unsigned a, b;
    nr_votes(pts, nrm, centers, bits, nw, V, i, &a, &b);
    for (int c = 0; c < 3; ++c) out[i * 3 + c] = a > b ? -nrm[i * 3 + c] : nrm[i * 3 + c];
}

__global__ __launch_bounds__(CH_THREADS) void k_nr_centers_finite(const double* __restrict__ centers, int V, nr_u64* err) {
    const int v = blockIdx.x * CH_THREADS + threadIdx.x;
    if (v < V && !ch_finite3(centers + v * 3)) atomicOr(err, (nr_u64)MVSDF_PC_ERR_FINITE);
}

// ================================================================ host ================================================================
struct NrKnnLayout {
    ChTreeLayout t;
    size_t flags, total;
};

static bool nr_knn_layout(long long n, NrKnnLayout* L) {
    if (n < 2 || n > INT_MAX) return false;
    WsCursor c{CH_HDR};
    if (!ch_tree_layout(n, c, &L->t)) return false;
    L->flags = c.take(NR_F_WORDS * 4);
    L->total = c.o;
    return true;
}

struct NrOrientLayout {
    size_t state, link, best_a, best_e, minidx, hkey, hidx, neg, pos, flags, err64, total;
};

static bool nr_orient_layout(long long n, NrOrientLayout* L) {
    if (n < 1 || n > INT_MAX) return false;
    WsCursor c{CH_HDR};
    L->state = c.take((size_t)n * 4);
    L->link = c.take((size_t)n * 4);
    L->best_a = c.take((size_t)n * 8);
    L->best_e = c.take((size_t)n * 8);
    L->minidx = c.take((size_t)n * 4);
    L->hkey = c.take((size_t)n * 8);
    L->hidx = c.take((size_t)n * 4);
    L->neg = c.take((size_t)n * 8);
    L->pos = c.take((size_t)n * 8);
    L->flags = c.take(NR_F_WORDS * 4);
    L->err64 = c.take(8);
    L->total = c.o;
    return true;
}

// a header of zeros but for its error word
static int nr_fail_header(void* ws, int words, int err_word, long long err, hipStream_t s, const char* what) {
    long long hdr[MVSDF_NR_ORIENT_H_WORDS] = {};
    hdr[err_word] = err;
    return mv_write_header(ws, hdr, words, s, what);
}

static int nr_words(long long V) { return (int)((V + 63) / 64); }

extern "C" {

size_t mvsdf_normals_knn_workspace_bytes(int64_t n) {
    NrKnnLayout L;
    return nr_knn_layout(n, &L) ? L.total : 0;
}

size_t mvsdf_normals_orient_workspace_bytes(int64_t n) {
    NrOrientLayout L;
    return nr_orient_layout(n, &L) ? L.total : 0;
}

int mvsdf_normals_knn(const double* pts, int64_t n, int32_t k, void* ws, size_t ws_bytes, int32_t* idx, double* d2, double* normals, double* variation,
                      void* stream) {
    const char* what = "mvsdf_normals_knn";
    NrKnnLayout L;
    if (!pts || !ws || !idx || (!normals != !variation) || k < 1 || k > MVSDF_PC_MAX_K || n < (int64_t)k + 1 || !nr_knn_layout(n, &L))
        return mv_fail(-1, "mvsdf_normals_knn: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_normals_knn: workspace too small (mvsdf_normals_knn_workspace_bytes)");
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    int* fl = (int*)(w + L.flags);
    int rc;
    if ((rc = mv_check(hipMemsetAsync(fl, 0, NR_F_WORDS * 4, s), what))) return rc;
    const ChBuilt tree = ch_tree_begin(pts, n, w, L.t, fl + NR_F_ERR, s, what);
    if (tree.rc) return tree.rc;
    if (tree.err) return nr_fail_header(w, MVSDF_ERRW_H_WORDS, MVSDF_ERRW_H_ERR, tree.err, s, what);
    const double* sp = (const double*)(w + L.t.sp);
    const double* box = (const double*)(w + L.t.box);
    ch_knn_dispatch(k, [&](auto cap) {
        hipLaunchKernelGGL(k_nr_knn<decltype(cap)::value>, dim3(mv_grid(n, CH_THREADS)), dim3(CH_THREADS), 0, s, sp, box, L.t.T, tree.perm, (int)k, idx, d2,
                           fl + NR_F_ERR);
    });
    if (normals)
        hipLaunchKernelGGL(k_nr_pca, dim3(mv_grid(n, CH_THREADS)), dim3(CH_THREADS), 0, s, pts, (long long)n, (const int*)idx, (int)k, normals, variation);
    hipLaunchKernelGGL(k_nr_knn_header, dim3(1), dim3(64), 0, s, (const int*)fl, (long long*)w);
    return mv_check(hipGetLastError(), what);
}

int mvsdf_normals_orient(const double* pts, const double* normals, const int32_t* neighbors, int64_t n, int32_t k, double ux, double uy, double uz,
                         const double* centers, const void* bits, int64_t V, void* ws, size_t ws_bytes, double* out, int32_t* labels, void* stream) {
    const char* what = "mvsdf_normals_orient";
    NrOrientLayout L;
    if (!pts || !normals || !neighbors || !ws || !out || !labels || out == normals || k < 1 || k > MVSDF_PC_MAX_K || !isfinite(ux) || !isfinite(uy) ||
        !isfinite(uz) || (!centers != !bits) || (centers && (V < 1 || V > MVSDF_VS_MAX_VIEWS)) || !nr_orient_layout(n, &L))
        return mv_fail(-1, "mvsdf_normals_orient: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_normals_orient: workspace too small (mvsdf_normals_orient_workspace_bytes)");
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    int* fl = (int*)(w + L.flags);
    unsigned* state = (unsigned*)(w + L.state);
    unsigned* link = (unsigned*)(w + L.link);
    nr_u64* best_a = (nr_u64*)(w + L.best_a);
    nr_u64* best_e = (nr_u64*)(w + L.best_e);
    int* minidx = (int*)(w + L.minidx);
    nr_u64* hkey = (nr_u64*)(w + L.hkey);
    int* hidx = (int*)(w + L.hidx);
    nr_u64* neg = (nr_u64*)(w + L.neg);
    nr_u64* pos = (nr_u64*)(w + L.pos);
    nr_u64* err64 = (nr_u64*)(w + L.err64);
    const long long N = n;
    const int K = k, nw = centers ? nr_words(V) : 0, nv = centers ? (int)V : 0;
    const dim3 g(mv_grid(n, CH_THREADS)), b(CH_THREADS);
    int rc;
    if ((rc = mv_check(hipMemsetAsync(fl, 0, NR_F_WORDS * 4, s), what))) return rc;
    if ((rc = mv_check(hipMemsetAsync(err64, 0, 8, s), what))) return rc;
    hipLaunchKernelGGL(k_nr_init, g, b, 0, s, pts, normals, neighbors, N, K, state, link, minidx, hkey, hidx, neg, pos, fl);
    if (centers) hipLaunchKernelGGL(k_nr_centers_finite, dim3(mv_grid(V, CH_THREADS)), b, 0, s, centers, nv, err64);
    long long rounds = 0;
    for (int turn = 0;; ++turn) {
        if (turn >= NR_MAX_ROUNDS) return nr_fail_header(w, MVSDF_NR_ORIENT_H_WORDS, MVSDF_NR_ORIENT_H_ERR, MVSDF_PC_ERR_ROUNDS, s, what);
        if ((rc = mv_check(hipMemsetAsync(fl + NR_F_PENDING, 0, 8, s), what))) return rc;       // pending and hooks
        hipLaunchKernelGGL(k_nr_round_begin, g, b, 0, s, (const unsigned*)state, N, best_a, best_e);
        hipLaunchKernelGGL(k_nr_best_a, g, b, 0, s, normals, neighbors, N, K, (const unsigned*)state, best_a);
        hipLaunchKernelGGL(k_nr_best_e, g, b, 0, s, normals, neighbors, N, K, (const unsigned*)state, (const nr_u64*)best_a, best_e);
        hipLaunchKernelGGL(k_nr_hook, g, b, 0, s, normals, N, (const unsigned*)state, (const nr_u64*)best_e, link, fl);
        int r[3];
        for (int jump = 0;; ++jump) {
            if (jump >= NR_MAX_JUMPS) return nr_fail_header(w, MVSDF_NR_ORIENT_H_WORDS, MVSDF_NR_ORIENT_H_ERR, MVSDF_PC_ERR_ROUNDS, s, what);
            hipLaunchKernelGGL(k_nr_jump, g, b, 0, s, N, (const unsigned*)state, link, fl);
            if ((rc = mv_check(hipGetLastError(), what))) return rc;
            if ((rc = mv_read(r, fl, sizeof(r), s, what))) return rc;
            if (r[NR_F_ERR] || !r[NR_F_PENDING]) break;
            if ((rc = mv_check(hipMemsetAsync(fl + NR_F_PENDING, 0, 4, s), what))) return rc;
        }
        if (r[NR_F_ERR]) return nr_fail_header(w, MVSDF_NR_ORIENT_H_WORDS, MVSDF_NR_ORIENT_H_ERR, r[NR_F_ERR], s, what);
        if (!r[NR_F_HOOKS]) break;
        ++rounds;
        hipLaunchKernelGGL(k_nr_apply, g, b, 0, s, N, state, (const unsigned*)link);
        hipLaunchKernelGGL(k_nr_unlink, g, b, 0, s, N, (const unsigned*)state, link);
    }
    if (centers) {
        nr_u64 e = 0;
        if ((rc = mv_read(&e, err64, 8, s, what))) return rc;
        if (e) return nr_fail_header(w, MVSDF_NR_ORIENT_H_WORDS, MVSDF_NR_ORIENT_H_ERR, (long long)e, s, what);
    }
    hipLaunchKernelGGL(k_nr_gather, g, b, 0, s, pts, normals, N, (const unsigned*)state, ux, uy, uz, centers, (const nr_u64*)bits, nw, nv, minidx, hkey, neg,
                       pos, fl);
    hipLaunchKernelGGL(k_nr_highest, g, b, 0, s, pts, N, (const unsigned*)state, ux, uy, uz, (const nr_u64*)hkey, hidx);
    hipLaunchKernelGGL(k_nr_orient_out, g, b, 0, s, normals, N, (const unsigned*)state, ux, uy, uz, centers != nullptr, (const int*)minidx, (const int*)hidx,
                       (const nr_u64*)neg, (const nr_u64*)pos, out, labels);
    hipLaunchKernelGGL(k_nr_orient_header, dim3(1), dim3(64), 0, s, (const int*)fl, rounds, (long long*)w);
    return mv_check(hipGetLastError(), what);
}

int mvsdf_normals_to_views(const double* pts, const double* normals, int64_t n, const double* centers, const void* bits, int64_t V, double* out, void* hdr,
                           void* stream) {
    const char* what = "mvsdf_normals_to_views";
    if (!pts || !normals || !centers || !bits || !out || !hdr || out == normals || n < 1 || n > INT_MAX || V < 1 || V > MVSDF_VS_MAX_VIEWS)
        return mv_fail(-1, "mvsdf_normals_to_views: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = mv_check(hipMemsetAsync(hdr, 0, MVSDF_ERRW_H_WORDS * 8, s), what)) return rc;
    hipLaunchKernelGGL(k_nr_centers_finite, dim3(mv_grid(V, CH_THREADS)), dim3(CH_THREADS), 0, s, centers, (int)V, (nr_u64*)hdr);
    hipLaunchKernelGGL(k_nr_to_views, dim3(mv_grid(n, CH_THREADS)), dim3(CH_THREADS), 0, s, pts, normals, (long long)n, centers, (const nr_u64*)bits,
                       nr_words(V), (int)V, out, (nr_u64*)hdr);
    return mv_check(hipGetLastError(), what);
}

}  // extern "C"
