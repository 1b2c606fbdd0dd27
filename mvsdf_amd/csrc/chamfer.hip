// chamfer.hip -- on-device DTU Chamfer evaluation (the DTUeval-python steps the reference's README points to): mesh sampling, the greedy radius
// filter, the observation / ground-plane masks and exact nearest distances with a cut-off.  Python: mvsdf_amd/chamfer.py, which states the metric;
// tests/chamfer_ref.py restates it in numpy.  All arithmetic is fp64 without contraction, in the order the metric writes it.
//
// * Sampling: per-face counts, an int64 exclusive scan (geom_prims.h: mv_scan), an emit pass; output = the vertices, then the samples in face order.
// * Downsampling: points binned into cells of edge density * (1 + 1e-6) in an open-addressing table keyed by a hash of the int64 cell coordinates
//   (a collision only merges two buckets, which adds candidates and never hides one).  The kept set is the lexicographically-first maximal
//   independent set under the keys splitmix64(seed ^ i): synchronous rounds (states ping-pong) keep a point once every lower-key neighbour is
//   removed and remove it once one is kept.  The lowest undecided key is decided in every round, so N rounds always suffice.
// * Masks: flags, int64 scans and an order-preserving scatter.
// * Nearest distance (the sort, the tree and its traversals live in nn_tree.h, shared with the other point-cloud files): the references are sorted
//   by a 63-bit Morton code (stable LSD radix sort, 4 bits per pass), cut into leaves of CH_LEAF consecutive points, and an implicit 8-ary tree of
//   fp64 boxes is built over the leaves.  A query descends greedily to one leaf for a first bound (ch_descend), then walks the tree without a stack
//   (ch_walk), pruning a box only when its lower bound exceeds min(best, max_dist)^2 by a relative 4e-9.  The minimum squared distance is exact
//   (every point not pruned is compared with the metric's formula) and sqrt is monotonic, so the result is sqrt(min d^2) bit for bit.  A query with nothing within max_dist only
//   meets boxes farther than the cut-off, which stops it near the root.
// * Sums: fixed-order block reductions in fp64, no float atomics.
//
// Every device loop is bounded; the downsampling round loop on the host stops at the caller's limit and reports it.
#include "nn_tree.h"

static_assert(MVSDF_CH_SAMPLE_H_WORDS * 8 <= CH_HDR && MVSDF_CH_DOWN_H_WORDS * 8 <= CH_HDR && MVSDF_CH_MASK_H_WORDS * 8 <= CH_HDR &&
                  MVSDF_CH_NEAR_H_WORDS * 8 <= CH_HDR,
              "the result words fit the header");

enum { DS_UNDECIDED = 0, DS_KEPT = 1, DS_REMOVED = 2 };

__host__ __device__ __forceinline__ uint64_t ch_splitmix64(uint64_t x) {
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// ================================================================ sampling ================================================================
struct ChFace {
    double a[3], v1[3], v2[3], n1, n2;
};

// the face's geometry; 0 = it samples nothing (zero area), else 1.  bad |= MVSDF_PC_ERR_RANGE / MVSDF_PC_ERR_FINITE.
__device__ __forceinline__ int ch_face(const float* __restrict__ V, const int* __restrict__ F, long long f, long long nv, double density, ChFace* g,
                                       int* bad) {
    double p[3][3];
    for (int s = 0; s < 3; ++s) {
        const int id = F[f * 3 + s];
        if (id < 0 || id >= nv) {
            *bad |= MVSDF_PC_ERR_RANGE;
            return 0;
        }
        for (int c = 0; c < 3; ++c) p[s][c] = (double)V[(long long)id * 3 + c];
        if (!ch_finite3(p[s])) {
            *bad |= MVSDF_PC_ERR_FINITE;
            return 0;
        }
    }
    for (int c = 0; c < 3; ++c) {
        g->a[c] = p[0][c];
        g->v1[c] = p[1][c] - p[0][c];
        g->v2[c] = p[2][c] - p[0][c];
    }
    const double* v1 = g->v1;
    const double* v2 = g->v2;
    const double l1 = sqrt((v1[0] * v1[0] + v1[1] * v1[1]) + v1[2] * v1[2]);
    const double l2 = sqrt((v2[0] * v2[0] + v2[1] * v2[1]) + v2[2] * v2[2]);
    const double cx = v1[1] * v2[2] - v1[2] * v2[1], cy = v1[2] * v2[0] - v1[0] * v2[2], cz = v1[0] * v2[1] - v1[1] * v2[0];
    const double area2 = sqrt((cx * cx + cy * cy) + cz * cz);
    if (!(area2 > 0)) return 0;
    const double thr = density * sqrt(l1 * l2 / area2);
    g->n1 = floor(l1 / thr);
    g->n2 = floor(l2 / thr);
    return 1;
}

// samples (i, j), i = 0..n1, j = 0..n2 (np.mgrid[:n1 + 1, :n2 + 1]) with s + t < 1.  s and t grow with i and j and fp addition is monotonic, so a row
// ends at its first miss and the rows end at the first row that keeps nothing: the loops take at most 2 k + 2 steps for k samples.  out == NULL:
// count only, stopping once the count passes `limit`.
__device__ __forceinline__ long long ch_face_samples(const ChFace& g, double* __restrict__ out, long long at, long long cap, long long limit) {
    const double d1 = fmax(g.n1, 1e-7), d2 = fmax(g.n2, 1e-7);
    long long k = 0;
    for (long long i = 0; (double)i <= g.n1 && k <= limit; ++i) {
        const double s = ((double)i + 0.5) / d1;
        long long row = 0;
        for (long long j = 0; (double)j <= g.n2 && k <= limit; ++j) {
            const double t = ((double)j + 0.5) / d2;
            if (!(s + t < 1.0)) break;
            if (out && at + k < cap) {
                double* o = out + (at + k) * 3;
                for (int c = 0; c < 3; ++c) o[c] = (g.v1[c] * s + g.v2[c] * t) + g.a[c];
            }
            ++k;
            ++row;
        }
        if (!row) break;
    }
    return k;
}

// per-face sample counts; a face with more than max_points samples stops counting there and raises MVSDF_PC_ERR_POINTS
__global__ __launch_bounds__(CH_THREADS) void k_ch_sample_count(const float* __restrict__ V, const int* __restrict__ F, long long nv, long long nf,
                                                                 double density, long long max_points, long long* __restrict__ cnt, int* err) {
    const long long f = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (f >= nf) return;
    int bad = 0;
    ChFace g;
    long long k = 0;
    if (ch_face(V, F, f, nv, density, &g, &bad)) {
        k = ch_face_samples(g, nullptr, 0, 0, max_points);
        if (k > max_points) {
            bad |= MVSDF_PC_ERR_POINTS;
            k = 0;
        }
    }
    cnt[f] = k;
    if (bad) atomicOr(err, bad);
}

// the vertices as fp64 (out may be NULL: check only)
__global__ __launch_bounds__(CH_THREADS) void k_ch_vert_copy(const float* __restrict__ V, long long nv, double* __restrict__ out, int* err) {
    const long long v = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (v >= nv) return;
    double p[3];
    for (int c = 0; c < 3; ++c) p[c] = (double)V[v * 3 + c];
    if (out)
        for (int c = 0; c < 3; ++c) out[v * 3 + c] = p[c];
    if (!ch_finite3(p)) atomicOr(err, MVSDF_PC_ERR_FINITE);
}

__global__ __launch_bounds__(CH_THREADS) void k_ch_sample_emit(const float* __restrict__ V, const int* __restrict__ F, long long nv, long long nf,
                                                                double density, const long long* __restrict__ off, double* __restrict__ out, long long cap) {
    const long long f = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (f >= nf) return;
    int bad = 0;
    ChFace g;
    if (ch_face(V, F, f, nv, density, &g, &bad)) ch_face_samples(g, out, nv + off[f], cap, LLONG_MAX - 1);
}

struct ChSampleLayout {
    size_t cnt, tmp, flags, total;
};

static bool ch_sample_layout(long long nv, long long nf, ChSampleLayout* L) {
    if (nv < 1 || nf < 1 || nv > INT_MAX || nf > INT_MAX) return false;
    WsCursor c{CH_HDR};
    L->cnt = c.take((size_t)nf * 8);
    L->tmp = c.take(mv_scan_tmp_bytes(nf));
    L->flags = c.take(4 * 8);
    L->total = c.o;
    return true;
}

// ================================================================ downsampling ================================================================
__device__ __forceinline__ unsigned long long ch_cell_key(long long x, long long y, long long z) {
    unsigned long long k = (unsigned long long)x * 0x9e3779b97f4a7c15ull ^ (unsigned long long)y * 0xc2b2ae3d27d4eb4full ^ (unsigned long long)z * 0x165667b19e3779f9ull;
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k == CH_EMPTY ? 0 : k;
}

__device__ __forceinline__ bool ch_cell(const double* p, double h, long long* c) {
    for (int a = 0; a < 3; ++a) {
        const double q = floor(p[a] / h);
        if (!(fabs(q) < CH_CELL_LIMIT)) return false;
        c[a] = (long long)q;
    }
    return true;
}

// the table slot holding key, or -1
__device__ __forceinline__ long long ch_find(const unsigned long long* __restrict__ keys, unsigned long long tmask, unsigned long long key) {
    unsigned long long slot = key & tmask;
    for (unsigned long long probe = 0; probe <= tmask; ++probe) {
        const unsigned long long k = keys[slot];
        if (k == key) return (long long)slot;
        if (k == CH_EMPTY) return -1;
        slot = (slot + 1) & tmask;
    }
    return -1;
}

__global__ __launch_bounds__(CH_THREADS) void k_ds_insert(const double* __restrict__ P, long long n, double h, unsigned long long* keys, unsigned long long tmask,
                                                           int* __restrict__ pslot, unsigned long long* cnt, int* err) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n) return;
    pslot[i] = -1;
    const double* p = P + i * 3;
    if (!ch_finite3(p)) {
        atomicOr(err, MVSDF_PC_ERR_FINITE);
        return;
    }
    long long c[3];
    if (!ch_cell(p, h, c)) {
        atomicOr(err, MVSDF_PC_ERR_COORD);
        return;
    }
    const unsigned long long key = ch_cell_key(c[0], c[1], c[2]);
    unsigned long long slot = key & tmask;
    for (unsigned long long probe = 0; probe <= tmask; ++probe) {
        const unsigned long long prev = atomicCAS(keys + slot, CH_EMPTY, key);
        if (prev == CH_EMPTY || prev == key) {
            pslot[i] = (int)slot;
            atomicAdd(cnt + slot, 1ull);
            return;
        }
        slot = (slot + 1) & tmask;
    }
    atomicOr(err, MVSDF_PC_ERR_HASH);
}

__global__ __launch_bounds__(CH_THREADS) void k_ds_fill(long long n, const int* __restrict__ pslot, const long long* __restrict__ start, unsigned long long* cur,
                                                         int* __restrict__ order) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n) return;
    const int s = pslot[i];
    order[start[s] + (long long)atomicAdd(cur + s, 1ull)] = (int)i;
}

// One synchronous round: a decided point keeps its state; an undecided one is removed if a lower-key neighbour (d^2 <= density^2) is kept, kept if
// every lower-key neighbour is removed, else it waits.  Reads only `old`, so the round is the same whatever the schedule.  left: undecided after it.
__global__ __launch_bounds__(CH_THREADS) void k_ds_round(const double* __restrict__ P, long long n, double h, double r2, unsigned long long seed,
                                                          const unsigned long long* __restrict__ keys, unsigned long long tmask, const unsigned long long* __restrict__ cnt,
                                                          const long long* __restrict__ start, const int* __restrict__ order, const unsigned char* __restrict__ old,
                                                          unsigned char* __restrict__ nxt, int* left) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned char st = old[i];
    if (st != DS_UNDECIDED) {
        nxt[i] = st;
        return;
    }
    const double* p = P + i * 3;
    long long c[3];
    ch_cell(p, h, c);                                             // the insert pass refused every point where this fails
    const unsigned long long ki = ch_splitmix64(seed ^ (unsigned long long)i);
    bool removed = false, blocked = false;
    for (int d = 0; d < 27 && !removed; ++d) {
        const long long s = ch_find(keys, tmask, ch_cell_key(c[0] + d / 9 - 1, c[1] + (d / 3) % 3 - 1, c[2] + d % 3 - 1));
        if (s < 0) continue;
        const long long b = start[s], e = b + (long long)cnt[s];
        for (long long q = b; q < e; ++q) {
            const int j = order[q];
            if (j == i) continue;
            const unsigned char sj = old[j];
            if (sj == DS_REMOVED) continue;
            if (ch_splitmix64(seed ^ (unsigned long long)j) >= ki) continue;
            const double* pj = P + (long long)j * 3;
            if (ch_d2(p[0], p[1], p[2], pj[0], pj[1], pj[2]) <= r2) {
                if (sj == DS_KEPT) {
                    removed = true;
                    break;
                }
                blocked = true;
            }
        }
    }
    nxt[i] = removed ? DS_REMOVED : (blocked ? DS_UNDECIDED : DS_KEPT);
    if (!removed && blocked) atomicAdd(left, 1);
}

__global__ __launch_bounds__(CH_THREADS) void k_ds_out(long long n, const unsigned char* __restrict__ st, unsigned char* __restrict__ kept,
                                                        unsigned long long* nkept) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    const bool k = i < n && st[i] == DS_KEPT;
    if (i < n) kept[i] = k;
    unsigned long long v = k;
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(nkept, v);
}

struct ChDsLayout {
    unsigned long long tsize;
    size_t keys, cnt, start, cur, pslot, order, st0, st1, tmp, flags, total;
};

static bool ch_ds_layout(long long n, ChDsLayout* L) {
    if (n < 1 || n > INT_MAX / 4) return false;
    L->tsize = 1;
    while (L->tsize < (unsigned long long)(2 * n)) L->tsize <<= 1;
    WsCursor c{CH_HDR};
    L->keys = c.take(L->tsize * 8);
    L->cnt = c.take(L->tsize * 8);
    L->start = c.take(L->tsize * 8);
    L->cur = c.take(L->tsize * 8);
    L->pslot = c.take((size_t)n * 4);
    L->order = c.take((size_t)n * 4);
    L->st0 = c.take((size_t)n);
    L->st1 = c.take((size_t)n);
    L->tmp = c.take(mv_scan_tmp_bytes((long long)L->tsize));
    L->flags = c.take((CH_DS_BATCH + 2) * 8);
    L->total = c.o;
    return true;
}

// ================================================================ masks ================================================================
struct ChMaskArgs {
    double lo[3], hi[3], bb0[3], res, plane[4];
    long long dim[3];
};

__global__ __launch_bounds__(CH_THREADS) void k_mask_flags(const double* __restrict__ P, const unsigned char* __restrict__ kept, long long n, ChMaskArgs m,
                                                            const unsigned char* __restrict__ obs, long long* __restrict__ fin, long long* __restrict__ fobs) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n) return;
    const double* p = P + i * 3;
    bool in = kept[i] != 0;
    for (int a = 0; a < 3; ++a) in = in && p[a] >= m.lo[a] && p[a] < m.hi[a];
    bool ob = in;
    long long g[3];
    for (int a = 0; a < 3 && ob; ++a) {
        const double x = rint((p[a] - m.bb0[a]) / m.res);        // round half to even (np.around)
        ob = x >= 0.0 && x < (double)m.dim[a];
        g[a] = ob ? (long long)x : 0;
    }
    if (ob) ob = obs[(g[0] * m.dim[1] + g[1]) * m.dim[2] + g[2]] != 0;
    fin[i] = in;
    fobs[i] = ob;
}

__global__ __launch_bounds__(CH_THREADS) void k_mask_plane(const double* __restrict__ S, long long m, ChMaskArgs a, long long* __restrict__ fab,
                                                            long long* err) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= m) return;
    const double* p = S + i * 3;
    if (!ch_finite3(p)) atomicOr((unsigned long long*)err, (unsigned long long)MVSDF_PC_ERR_FINITE);
    fab[i] = ((a.plane[0] * p[0] + a.plane[1] * p[1]) + a.plane[2] * p[2]) + a.plane[3] > 0.0;
}

// out[off[i]] = P[i] where the flag is set (flags are re-derived from off: off[i + 1] - off[i], and the total for the last item)
__global__ __launch_bounds__(CH_THREADS) void k_mask_scatter(const double* __restrict__ P, long long n, const long long* __restrict__ off,
                                                              const long long* __restrict__ total, double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n) return;
    const long long o = off[i], nx = i + 1 < n ? off[i + 1] : *total;
    if (nx > o)
        for (int c = 0; c < 3; ++c) out[o * 3 + c] = P[i * 3 + c];
}

struct ChMaskLayout {
    size_t fin, fobs, fab, tmp1, tmp2, tmp3, tot, total;
};

static bool ch_mask_layout(long long n, long long m, ChMaskLayout* L) {
    if (n < 1 || m < 1 || n > (1ll << 40) || m > (1ll << 40)) return false;
    WsCursor c{CH_HDR};
    L->fin = c.take((size_t)n * 8);
    L->fobs = c.take((size_t)n * 8);
    L->fab = c.take((size_t)m * 8);
    L->tmp1 = c.take(mv_scan_tmp_bytes(n));
    L->tmp2 = c.take(mv_scan_tmp_bytes(n));
    L->tmp3 = c.take(mv_scan_tmp_bytes(m));
    L->tot = c.take(4 * 8);
    L->total = c.o;
    return true;
}

// ================================================================ nearest distance ================================================================
__device__ __forceinline__ double ch_leaf_min(const double* __restrict__ sp, long long n, long long l, double x, double y, double z, double best) {
    const long long e = min(n, (l + 1) * CH_LEAF);
    for (long long i = l * CH_LEAF; i < e; ++i) best = fmin(best, ch_d2(x, y, z, sp[i * 3], sp[i * 3 + 1], sp[i * 3 + 2]));
    return best;
}

// dist[i] = min over the references of sqrt((dx dx + dy dy) + dz dz), +inf where that is not < max_dist
__global__ __launch_bounds__(CH_THREADS) void k_nn_query(const double* __restrict__ Q, long long nq, const double* __restrict__ sp, const double* __restrict__ box,
                                                          ChTree T, double max_dist, double* __restrict__ dist, int* err) {
    const long long qi = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (qi >= nq) return;
    const double x = Q[qi * 3], y = Q[qi * 3 + 1], z = Q[qi * 3 + 2];
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) {
        atomicOr(err, MVSDF_PC_ERR_FINITE);
        dist[qi] = INFINITY;
        return;
    }
    const double cut2 = max_dist * max_dist;
    double best = INFINITY;
    const long long first = ch_descend<false>(box, T, x, y, z);   // a first bound from one leaf, then the full walk
    if (ch_box_lb2(box + first * 6, x, y, z) <= cut2 * CH_MARGIN2) best = ch_leaf_min(sp, T.n, first, x, y, z, best);
    if (!ch_walk(
            box, T, x, y, z, [&] { return fmin(best, cut2) * CH_MARGIN2; }, [&](long long l) { best = ch_leaf_min(sp, T.n, l, x, y, z, best); }))
        atomicOr(err, MVSDF_PC_ERR_WALK);
    const double d = sqrt(best);
    dist[qi] = d < max_dist ? d : INFINITY;
}

// fixed-order sums of the finite distances: per-workgroup (sum, count), then one workgroup over those
__global__ __launch_bounds__(CH_THREADS) void k_nn_sum_part(const double* __restrict__ d, long long n, double* __restrict__ psum, long long* __restrict__ pcnt) {
    __shared__ double ss[CH_THREADS];
    __shared__ long long sc[CH_THREADS];
    const long long base = (long long)blockIdx.x * CH_CHUNK + (long long)threadIdx.x * CH_ITEMS;
    double s = 0.0;
    long long c = 0;
    for (int q = 0; q < CH_ITEMS; ++q)
        if (base + q < n && isfinite(d[base + q])) {
            s += d[base + q];
            ++c;
        }
    ss[threadIdx.x] = s;
    sc[threadIdx.x] = c;
    __syncthreads();
    for (int w = CH_THREADS / 2; w; w >>= 1) {
        if ((int)threadIdx.x < w) {
            ss[threadIdx.x] += ss[threadIdx.x + w];
            sc[threadIdx.x] += sc[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        psum[blockIdx.x] = ss[0];
        pcnt[blockIdx.x] = sc[0];
    }
}

__global__ __launch_bounds__(CH_TOP_THREADS) void k_nn_sum_final(const double* __restrict__ psum, const long long* __restrict__ pcnt, long long nb,
                                                                  long long* __restrict__ hdr) {
    __shared__ double ss[CH_TOP_THREADS];
    __shared__ long long sc[CH_TOP_THREADS];
    const int t = threadIdx.x;
    const long long per = (nb + CH_TOP_THREADS - 1) / CH_TOP_THREADS;
    const long long lo = min(nb, t * per), hi = min(nb, lo + per);
    double s = 0.0;
    long long c = 0;
    for (long long q = lo; q < hi; ++q) {
        s += psum[q];
        c += pcnt[q];
    }
    ss[t] = s;
    sc[t] = c;
    __syncthreads();
    for (int w = CH_TOP_THREADS / 2; w; w >>= 1) {
        if (t < w) {
            ss[t] += ss[t + w];
            sc[t] += sc[t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        hdr[0] = sc[0];
        hdr[1] = __double_as_longlong(ss[0]);
    }
}

struct ChNnLayout {
    ChTreeLayout t;
    long long nbq;
    size_t psum, pcnt, flags, total;
};

static bool ch_nn_layout(long long nq, long long nr, ChNnLayout* L) {
    if (nq < 0 || nr < 1 || nq > (1ll << 40) || nr > INT_MAX) return false;
    WsCursor c{CH_HDR};
    if (!ch_tree_layout(nr, c, &L->t)) return false;
    L->nbq = mv_ceil_div(nq > 0 ? nq : 1, CH_CHUNK);
    L->psum = c.take((size_t)L->nbq * 8);
    L->pcnt = c.take((size_t)L->nbq * 8);
    L->flags = c.take(4 * 8);
    L->total = c.o;
    return true;
}

extern "C" {

uint64_t mvsdf_chamfer_key(uint64_t seed, int64_t i) { return ch_splitmix64(seed ^ (uint64_t)i); }

size_t mvsdf_chamfer_sample_workspace_bytes(int64_t nv, int64_t nf) {
    ChSampleLayout L;
    return ch_sample_layout(nv, nf, &L) ? L.total : 0;
}

int mvsdf_chamfer_sample_count(const float* verts, const int32_t* faces, int64_t nv, int64_t nf, double density, int64_t max_points, void* ws, size_t ws_bytes,
                               void* stream) {
    ChSampleLayout L;
    if (!verts || !faces || !ws || !ch_sample_layout(nv, nf, &L) || !(density > 0) || !isfinite(density) || max_points < 1)
        return mv_fail(-1, "mvsdf_chamfer_sample_count: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_chamfer_sample_count: workspace too small (mvsdf_chamfer_sample_workspace_bytes)");
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    long long* cnt = (long long*)(w + L.cnt);
    long long* fl = (long long*)(w + L.flags);                    // [0]: error bits (int), [1]: the scan's total
    int rc;
    if ((rc = mv_check(hipMemsetAsync(fl, 0, 4 * 8, s), "mvsdf_chamfer_sample_count"))) return rc;
    hipLaunchKernelGGL(k_ch_vert_copy, dim3(mv_grid(nv, CH_THREADS)), dim3(CH_THREADS), 0, s, verts, (long long)nv, (double*)nullptr, (int*)fl);
    hipLaunchKernelGGL(k_ch_sample_count, dim3(mv_grid(nf, CH_THREADS)), dim3(CH_THREADS), 0, s, verts, faces, (long long)nv, (long long)nf, density,
                       (long long)max_points, cnt, (int*)fl);
    mv_scan(cnt, nf, cnt, w + L.tmp, fl + 1, s);
    if ((rc = mv_check(hipGetLastError(), "mvsdf_chamfer_sample_count"))) return rc;
    long long h[2];
    if ((rc = mv_read(h, fl, sizeof(h), s, "mvsdf_chamfer_sample_count"))) return rc;
    const long long err = (int)h[0], samples = h[1];
    long long hdr[MVSDF_CH_SAMPLE_H_WORDS];
    hdr[MVSDF_CH_SAMPLE_H_POINTS] = nv + samples;
    hdr[MVSDF_CH_SAMPLE_H_SAMPLES] = samples;
    hdr[MVSDF_CH_SAMPLE_H_ERR] = !err && nv + samples > max_points ? MVSDF_PC_ERR_POINTS : err;
    return mv_write_header(ws, hdr, MVSDF_CH_SAMPLE_H_WORDS, s, "mvsdf_chamfer_sample_count");
}

int mvsdf_chamfer_sample_emit(const float* verts, const int32_t* faces, int64_t nv, int64_t nf, double density, void* ws, size_t ws_bytes, double* out,
                              int64_t cap, void* stream) {
    ChSampleLayout L;
    if (!verts || !faces || !ws || !out || !ch_sample_layout(nv, nf, &L) || !(density > 0) || cap < nv)
        return mv_fail(-1, "mvsdf_chamfer_sample_emit: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_chamfer_sample_emit: workspace too small (mvsdf_chamfer_sample_workspace_bytes)");
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ch_vert_copy, dim3(mv_grid(nv, CH_THREADS)), dim3(CH_THREADS), 0, s, verts, (long long)nv, out, (int*)(w + L.flags));
    hipLaunchKernelGGL(k_ch_sample_emit, dim3(mv_grid(nf, CH_THREADS)), dim3(CH_THREADS), 0, s, verts, faces, (long long)nv, (long long)nf, density,
                       (const long long*)(w + L.cnt), out, (long long)cap);
    return mv_check(hipGetLastError(), "mvsdf_chamfer_sample_emit");
}

size_t mvsdf_chamfer_downsample_workspace_bytes(int64_t n) {
    ChDsLayout L;
    return ch_ds_layout(n, &L) ? L.total : 0;
}

int mvsdf_chamfer_downsample(const double* pts, int64_t n, double density, uint64_t seed, int64_t max_rounds, void* ws, size_t ws_bytes, uint8_t* kept,
                             void* stream) {
    ChDsLayout L;
    if (!pts || !ws || !kept || !ch_ds_layout(n, &L) || !(density > 0) || !isfinite(density) || max_rounds < 1)
        return mv_fail(-1, "mvsdf_chamfer_downsample: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_chamfer_downsample: workspace too small (mvsdf_chamfer_downsample_workspace_bytes)");
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    const double h = density * (1.0 + 1e-6), r2 = density * density;
    const unsigned long long tmask = L.tsize - 1;
    const unsigned gn = mv_grid(n, CH_THREADS);
    unsigned long long* keys = (unsigned long long*)(w + L.keys);
    unsigned long long* cnt = (unsigned long long*)(w + L.cnt);
    long long* start = (long long*)(w + L.start);
    unsigned char* st[2] = {(unsigned char*)(w + L.st0), (unsigned char*)(w + L.st1)};
    int* fl = (int*)(w + L.flags);                                // [0]: error bits, [1]: kept (int64 at +8), [4..]: undecided after each round of a batch
    long long hdr[MVSDF_CH_DOWN_H_WORDS] = {};
    int rc;
    if ((rc = mv_check(hipMemsetAsync(keys, 0xff, L.tsize * 8, s), "mvsdf_chamfer_downsample"))) return rc;
    if ((rc = mv_check(hipMemsetAsync(cnt, 0, L.tsize * 8, s), "mvsdf_chamfer_downsample"))) return rc;
    if ((rc = mv_check(hipMemsetAsync(w + L.cur, 0, L.tsize * 8, s), "mvsdf_chamfer_downsample"))) return rc;
    if ((rc = mv_check(hipMemsetAsync(st[0], DS_UNDECIDED, (size_t)n, s), "mvsdf_chamfer_downsample"))) return rc;
    if ((rc = mv_check(hipMemsetAsync(fl, 0, (CH_DS_BATCH + 2) * 8, s), "mvsdf_chamfer_downsample"))) return rc;
    hipLaunchKernelGGL(k_ds_insert, dim3(gn), dim3(CH_THREADS), 0, s, pts, (long long)n, h, keys, tmask, (int*)(w + L.pslot), cnt, fl);
    if ((rc = mv_check(hipGetLastError(), "mvsdf_chamfer_downsample"))) return rc;
    int e = 0;
    if ((rc = mv_read(&e, fl, 4, s, "mvsdf_chamfer_downsample"))) return rc;
    hdr[MVSDF_CH_DOWN_H_ERR] = e;
    if (!e) {
        mv_scan((const long long*)cnt, (long long)L.tsize, start, w + L.tmp, (long long*)(fl + 2), s);
        hipLaunchKernelGGL(k_ds_fill, dim3(gn), dim3(CH_THREADS), 0, s, (long long)n, (const int*)(w + L.pslot), (const long long*)start,
                           (unsigned long long*)(w + L.cur), (int*)(w + L.order));
        int cur = 0;
        bool done = false;
        while (!done) {
            if (hdr[MVSDF_CH_DOWN_H_ROUNDS] >= max_rounds) {
                hdr[MVSDF_CH_DOWN_H_ERR] |= MVSDF_PC_ERR_ROUNDS;
                break;
            }
            const int batch = (int)(max_rounds - hdr[MVSDF_CH_DOWN_H_ROUNDS] < CH_DS_BATCH ? max_rounds - hdr[MVSDF_CH_DOWN_H_ROUNDS] : CH_DS_BATCH);
            if ((rc = mv_check(hipMemsetAsync(fl + 4, 0, CH_DS_BATCH * 4, s), "mvsdf_chamfer_downsample"))) return rc;
            for (int b = 0; b < batch; ++b) {
                hipLaunchKernelGGL(k_ds_round, dim3(gn), dim3(CH_THREADS), 0, s, pts, (long long)n, h, r2, (unsigned long long)seed,
                                   (const unsigned long long*)keys, tmask, (const unsigned long long*)cnt, (const long long*)start,
                                   (const int*)(w + L.order), (const unsigned char*)st[cur], st[cur ^ 1], fl + 4 + b);
                cur ^= 1;
            }
            if ((rc = mv_check(hipGetLastError(), "mvsdf_chamfer_downsample"))) return rc;
            int left[CH_DS_BATCH];
            if ((rc = mv_read(left, fl + 4, sizeof(left), s, "mvsdf_chamfer_downsample"))) return rc;
            for (int b = 0; b < batch && !done; ++b) {
                ++hdr[MVSDF_CH_DOWN_H_ROUNDS];
                done = left[b] == 0;
            }
        }
        if (done) {
            if ((rc = mv_check(hipMemsetAsync(fl + 2, 0, 8, s), "mvsdf_chamfer_downsample"))) return rc;   // (the table scan's total)
            hipLaunchKernelGGL(k_ds_out, dim3(gn), dim3(CH_THREADS), 0, s, (long long)n, (const unsigned char*)st[cur], kept,
                               (unsigned long long*)(fl + 2));
            if ((rc = mv_check(hipGetLastError(), "mvsdf_chamfer_downsample"))) return rc;
            if ((rc = mv_read(&hdr[MVSDF_CH_DOWN_H_KEPT], fl + 2, 8, s, "mvsdf_chamfer_downsample"))) return rc;
        }
    }
    return mv_write_header(ws, hdr, MVSDF_CH_DOWN_H_WORDS, s, "mvsdf_chamfer_downsample");
}

size_t mvsdf_chamfer_mask_workspace_bytes(int64_t n, int64_t m) {
    ChMaskLayout L;
    return ch_mask_layout(n, m, &L) ? L.total : 0;
}

int mvsdf_chamfer_mask(const double* pts, const uint8_t* kept, int64_t n, const double* stl, int64_t m, const float* box, double res, const uint8_t* obs,
                       const int64_t* obs_shape, const double* plane, void* ws, size_t ws_bytes, double* d_in, double* d_obs, double* s_above, void* stream) {
    ChMaskLayout L;
    if (!pts || !kept || !stl || !box || !obs || !obs_shape || !plane || !ws || !d_in || !d_obs || !s_above || !ch_mask_layout(n, m, &L) || !(res > 0))
        return mv_fail(-1, "mvsdf_chamfer_mask: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_chamfer_mask: workspace too small (mvsdf_chamfer_mask_workspace_bytes)");
    ChMaskArgs a;
    for (int k = 0; k < 3; ++k) {
        a.lo[k] = (double)box[k];
        a.hi[k] = (double)box[3 + k];
        a.bb0[k] = (double)box[6 + k];
        a.dim[k] = obs_shape[k];
        if (obs_shape[k] < 1) return mv_fail(-1, "mvsdf_chamfer_mask: empty observation mask");
    }
    for (int k = 0; k < 4; ++k) a.plane[k] = plane[k];
    a.res = res;
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    long long* fin = (long long*)(w + L.fin);
    long long* fobs = (long long*)(w + L.fobs);
    long long* fab = (long long*)(w + L.fab);
    long long* tot = (long long*)(w + L.tot);
    hipLaunchKernelGGL(k_mask_flags, dim3(mv_grid(n, CH_THREADS)), dim3(CH_THREADS), 0, s, pts, kept, (long long)n, a, obs, fin, fobs);
    if (int rc = mv_check(hipMemsetAsync(tot, 0, MVSDF_CH_MASK_H_WORDS * 8, s), "mvsdf_chamfer_mask")) return rc;
    hipLaunchKernelGGL(k_mask_plane, dim3(mv_grid(m, CH_THREADS)), dim3(CH_THREADS), 0, s, stl, (long long)m, a, fab, tot + MVSDF_CH_MASK_H_ERR);
    mv_scan(fin, n, fin, w + L.tmp1, tot + MVSDF_CH_MASK_H_IN, s);
    mv_scan(fobs, n, fobs, w + L.tmp2, tot + MVSDF_CH_MASK_H_OBS, s);
    mv_scan(fab, m, fab, w + L.tmp3, tot + MVSDF_CH_MASK_H_ABOVE, s);
    hipLaunchKernelGGL(k_mask_scatter, dim3(mv_grid(n, CH_THREADS)), dim3(CH_THREADS), 0, s, pts, (long long)n, (const long long*)fin, (const long long*)(tot + MVSDF_CH_MASK_H_IN), d_in);
    hipLaunchKernelGGL(k_mask_scatter, dim3(mv_grid(n, CH_THREADS)), dim3(CH_THREADS), 0, s, pts, (long long)n, (const long long*)fobs,
                       (const long long*)(tot + MVSDF_CH_MASK_H_OBS), d_obs);
    hipLaunchKernelGGL(k_mask_scatter, dim3(mv_grid(m, CH_THREADS)), dim3(CH_THREADS), 0, s, stl, (long long)m, (const long long*)fab,
                       (const long long*)(tot + MVSDF_CH_MASK_H_ABOVE), s_above);
    if (int rc = mv_check(hipGetLastError(), "mvsdf_chamfer_mask")) return rc;
    return mv_check(hipMemcpyAsync(ws, tot, MVSDF_CH_MASK_H_WORDS * 8, hipMemcpyDeviceToDevice, s), "mvsdf_chamfer_mask");
}

size_t mvsdf_chamfer_nearest_workspace_bytes(int64_t nq, int64_t nr) {
    ChNnLayout L;
    return ch_nn_layout(nq, nr, &L) ? L.total : 0;
}

int mvsdf_chamfer_nearest(const double* queries, int64_t nq, const double* refs, int64_t nr, double max_dist, void* ws, size_t ws_bytes, double* dist,
                          void* stream) {
    ChNnLayout L;
    if (!refs || !ws || (nq > 0 && (!queries || !dist)) || !ch_nn_layout(nq, nr, &L) || !(max_dist > 0))
        return mv_fail(-1, "mvsdf_chamfer_nearest: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_chamfer_nearest: workspace too small (mvsdf_chamfer_nearest_workspace_bytes)");
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    int* fl = (int*)(w + L.flags);
    long long hdr[MVSDF_CH_NEAR_H_WORDS] = {};
    int rc;
    if ((rc = mv_check(hipMemsetAsync(fl, 0, 4 * 8, s), "mvsdf_chamfer_nearest"))) return rc;
    const ChBuilt tree = ch_tree_begin(refs, (long long)nr, w, L.t, fl, s, "mvsdf_chamfer_nearest");
    if (tree.rc) return tree.rc;
    hdr[MVSDF_CH_NEAR_H_ERR] = tree.err;
    if (!tree.err) {
        const double* sp = (const double*)(w + L.t.sp);
        const double* box = (const double*)(w + L.t.box);
        const ChTree& T = L.t.T;
        if (nq > 0) {
            hipLaunchKernelGGL(k_nn_query, dim3(mv_grid(nq, CH_THREADS)), dim3(CH_THREADS), 0, s, queries, (long long)nq, sp, box, T, max_dist, dist, fl);
            hipLaunchKernelGGL(k_nn_sum_part, dim3((unsigned)L.nbq), dim3(CH_THREADS), 0, s, (const double*)dist, (long long)nq, (double*)(w + L.psum),
                               (long long*)(w + L.pcnt));
            hipLaunchKernelGGL(k_nn_sum_final, dim3(1), dim3(CH_TOP_THREADS), 0, s, (const double*)(w + L.psum), (const long long*)(w + L.pcnt), L.nbq,
                               (long long*)(fl + 2));
        }
        if ((rc = mv_check(hipGetLastError(), "mvsdf_chamfer_nearest"))) return rc;
        long long r[3];                                           // error bits (int) at byte 0, k_nn_sum_final's count and sum at bytes 8 and 16
        if ((rc = mv_read(r, fl, sizeof(r), s, "mvsdf_chamfer_nearest"))) return rc;
        hdr[MVSDF_CH_NEAR_H_COUNT] = nq > 0 ? r[1] : 0;
        hdr[MVSDF_CH_NEAR_H_SUM] = nq > 0 ? r[2] : 0;
        hdr[MVSDF_CH_NEAR_H_ERR] = (int)r[0];
    }
    return mv_write_header(ws, hdr, MVSDF_CH_NEAR_H_WORDS, s, "mvsdf_chamfer_nearest");
}

}  // extern "C"
