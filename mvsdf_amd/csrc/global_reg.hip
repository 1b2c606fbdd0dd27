// global_reg.hip -- global registration on the device: the simplified point feature histograms of every point, their weighted sums (FPFH) quantised to
// int8 codes, the all-pairs nearest code on the int8 matrix cores, and the hypothesis search over correspondences (sample, prune, Horn's closed form,
// score).  Python: mvsdf_amd/global_reg.py, which states every definition; tests/global_reg_ref.py restates them in numpy.  fp64 arithmetic is
// uncontracted and in the order the definitions write it; everything else is integers.
//
// * k_gg_spfh / k_gg_fpfh: one lane per point over its neighbour row.  The lane owns its histogram row in global memory (plain read-modify-write); the
//   33 fp64 sums of the FPFH stay in registers (every index is a compile-time constant).
// * The matcher.  D(i,j) = |s_i|^2 + |t_j|^2 - 2 s_i . t_j on integers.  k_gg_pack writes every code row as 48 bytes (33 codes, 15 zeros; the rows
//   padded to a multiple of 16 with zero rows) and minus its squared norm.  k_gg_match: a wave owns 16 sources and one v_mfma_i32_16x16x64_i8 gives the
//   16 x 16 dot products of a target tile: A = the targets (rows of the result), B = the sources (columns, `lane & 15`).  Lane l carries bytes
//   16 (l >> 4) .. + 15 of row / column l & 15 for both operands, so lanes 48..63 (k = 48..63) carry zeros and read nothing.  The sources' fragment
//   and norms stay in registers for the whole walk; every lane keeps a running (D, j) over its four rows per tile, ascending j with a strict
//   comparison (held as the maximum of e = 2 s.t - |t|^2: one shift-add per pair, a max tree per tile, the index only when the maximum moves); at
//   the end the four lane groups are combined by the packed key D << 32 | j (two xor shuffles) and lane group 0 issues one 64-bit atomicMin per
//   source.  A workgroup is 4 waves = 64 sources; when there are few sources the target tiles are split over blockIdx.y (gg_match_splits) and the
//   atomicMin combines the splits.  No distance reaches memory.  Registers: 4 (B) + GG_UNROLL x (4 (A) + 4 (target norms)) + 4 (acc) + the running
//   pair and addresses, below the 64 that let 8 waves share a SIMD; LDS: none (a target tile is 768 contiguous bytes that the four waves of a
//   workgroup read at about the same time, so three of the four reads hit the cache).
// * The search.  k_gg_hyp: one lane per hypothesis draws its three correspondences (splitmix64 of the counter), applies the cheap rejections, fits
//   (16 cyclic Jacobi sweeps on Horn's 4 x 4 matrix, all in registers) and checks its own three pairs; survivors append (h, T) to a list through
//   an integer atomic counter (the order of the list is arbitrary and no result depends on it).  k_gg_score: workgroups stride over the list, T in
//   LDS, integer counts, one 64-bit atomicMax of count << 32 | ~h per hypothesis.  k_gg_winner / k_gg_mask unpack the best key.
//
// Every device loop is bounded; no kernel waits on another.  Integer atomics only.
#include "det_math64.h"
#include "nn_tree.h"

#define GG_DIM 33
#define GG_BINS 11
#define GG_ROW 48                                     // bytes of a packed code row: three 16-byte operand chunks
#define GG_WAVES 4                                    // waves of a matcher workgroup, 16 sources each
#define GG_UNROLL 4                                   // target tiles whose loads a wave keeps in flight
#define GG_TARGET_BLOCKS 2048                         // the matcher splits the targets until about this many workgroups exist (8 waves per SIMD) ...
#define GG_MIN_TILES 64                               // ... but no split walks fewer than this many 16-target tiles
#define GG_PAD_NORM (-0x3fffffff)                      // the "norm" of a padding row: below every 2 s.t - |t|^2, and |s|^2 minus it still fits an int
#define GG_SCORE_BLOCKS 2048

typedef int gg_v4i __attribute__((ext_vector_type(4)));
typedef unsigned long long gg_u64;

__device__ __forceinline__ double gg_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ __forceinline__ void gg_cross(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// clamp(floor(11 * ((f - lo) / (hi - lo))), 0, 10); a NaN counts as bin 0
__device__ __forceinline__ int gg_bin(double f, double lo, double hi) {
    double b = floor(GG_BINS * ((f - lo) / (hi - lo)));
    if (!(b >= 0.0)) b = 0.0;
    if (b > GG_BINS - 1) b = GG_BINS - 1;
    return (int)b;
}

// the pair (i, j) of a row: d = p_j - p_i and d2; near iff j != i, d2 > 0 and d2 <= r2
__device__ __forceinline__ bool gg_near(const double* __restrict__ P, long long i, long long j, double r2, double* d, double& d2) {
    for (int a = 0; a < 3; ++a) d[a] = P[j * 3 + a] - P[i * 3 + a];
    d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    return j != i && d2 > 0.0 && d2 <= r2;
}

// ================================================================ stage 1 ================================================================
static __global__ __launch_bounds__(CH_THREADS) void k_gg_spfh(const double* __restrict__ P, const double* __restrict__ Nrm, const int* __restrict__ nb,
                                                               long long n, int k, double r2, int* __restrict__ hist, int* __restrict__ count, int* err) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n) return;
    int* h = hist + i * GG_DIM;
    for (int c = 0; c < GG_DIM; ++c) h[c] = 0;
    int bad = 0, cnt = 0;
    if (!ch_finite3(P + i * 3)) bad |= MVSDF_PC_ERR_FINITE;
    if (!ch_finite3(Nrm + i * 3)) bad |= MVSDF_PC_ERR_NORMAL;
    const double ni[3] = {Nrm[i * 3], Nrm[i * 3 + 1], Nrm[i * 3 + 2]};
    for (int t = 0; t < k; ++t) {
        const long long j = nb[i * k + t];
        if (j < 0 || j >= n) {
            bad |= MVSDF_PC_ERR_INDEX;
            continue;
        }
        double d[3], d2;
        if (!gg_near(P, i, j, r2, d, d2)) continue;
        const double s = sqrt(d2);
        double dn[3] = {d[0] / s, d[1] / s, d[2] / s};
        const double nj[3] = {Nrm[j * 3], Nrm[j * 3 + 1], Nrm[j * 3 + 2]};
        const double a1 = gg_dot(ni, dn), a2 = gg_dot(nj, dn);
        const bool sw = fabs(a1) < fabs(a2);
        double u[3], nt[3];
        for (int a = 0; a < 3; ++a) {
            u[a] = sw ? nj[a] : ni[a];
            nt[a] = sw ? ni[a] : nj[a];
            dn[a] = sw ? -dn[a] : dn[a];
        }
        const double phi = gg_dot(u, dn);
        double v[3], w[3];
        gg_cross(dn, u, v);
        const double ln = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
        if (!(ln > 0.0)) continue;                                // invalid: no frame
        for (int a = 0; a < 3; ++a) v[a] = v[a] / ln;
        gg_cross(u, v, w);
        const double alpha = gg_dot(v, nt);
        const double y = gg_dot(w, nt), x = gg_dot(u, nt);
        double theta = dm64_atan2_pos(fabs(y), x);
        if (y < 0.0) theta = -theta;
        h[gg_bin(theta, -DM64_PI, DM64_PI)] += 1;
        h[GG_BINS + gg_bin(alpha, -1.0, 1.0)] += 1;
        h[2 * GG_BINS + gg_bin(phi, -1.0, 1.0)] += 1;
        ++cnt;
    }
    count[i] = cnt;
    if (bad) atomicOr(err, bad);
}

// ================================================================ stage 2 ================================================================
static __global__ __launch_bounds__(CH_THREADS) void k_gg_fpfh(const double* __restrict__ P, const int* __restrict__ nb, const int* __restrict__ hist,
                                                               const int* __restrict__ count, long long n, int k, double r2, double* __restrict__ feat,
                                                               signed char* __restrict__ codes, int* err) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n) return;
    int bad = 0;
    if (!ch_finite3(P + i * 3)) bad |= MVSDF_PC_ERR_FINITE;
    double acc[GG_DIM];
#pragma unroll
    for (int c = 0; c < GG_DIM; ++c) acc[c] = 0.0;
    for (int t = 0; t < k; ++t) {
        const long long j = nb[i * k + t];
        if (j < 0 || j >= n) {
            bad |= MVSDF_PC_ERR_INDEX;
            continue;
        }
        double d[3], d2;
        if (!gg_near(P, i, j, r2, d, d2)) continue;
        const int cj = count[j];
        if (cj <= 0) continue;
        const double wgt = 1.0 / d2, cd = (double)cj;
        const int* hj = hist + j * GG_DIM;
#pragma unroll
        for (int c = 0; c < GG_DIM; ++c) acc[c] = acc[c] + wgt * ((double)hj[c] / cd);
    }
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < GG_BINS; ++c) s = s + acc[g * GG_BINS + c];
#pragma unroll
        for (int c = 0; c < GG_BINS; ++c) {
            const double f = s > 0.0 ? 100.0 * acc[g * GG_BINS + c] / s : 0.0;
            feat[i * GG_DIM + g * GG_BINS + c] = f;
            double q = floor(f * 1.27);
            if (!(q >= 0.0)) q = 0.0;                             // (a NaN from non-finite input; the error bit is raised)
            codes[i * GG_DIM + g * GG_BINS + c] = (signed char)(q > 127.0 ? 127.0 : q);
        }
    }
    if (bad) atomicOr(err, bad);
}

// ================================================================ stage 3: the matcher ================================================================
// row i of packed [npad][48] = the 33 codes of point i and 15 zeros (all zeros for i >= n); norm[i] = minus the sum of its squares, GG_PAD_NORM for i >= n
static __global__ __launch_bounds__(CH_THREADS) void k_gg_pack(const signed char* __restrict__ codes, long long n, long long npad, int* __restrict__ packed,
                                                               int* __restrict__ norm, long long* err) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= npad) return;
    int word[GG_ROW / 4];
#pragma unroll
    for (int q = 0; q < GG_ROW / 4; ++q) word[q] = 0;
    int s = 0, bad = 0;
    if (i < n) {
#pragma unroll
        for (int c = 0; c < GG_DIM; ++c) {
            const int v = codes[i * GG_DIM + c];
            if (v < 0) bad = MVSDF_PC_ERR_CODE;
            const int u = v & 127;
            word[c >> 2] |= u << (8 * (c & 3));
            s += u * u;
        }
    }
#pragma unroll
    for (int q = 0; q < GG_ROW / 4; ++q) packed[i * (GG_ROW / 4) + q] = word[q];
    norm[i] = i < n ? -s : GG_PAD_NORM;
    if (bad) atomicOr((gg_u64*)err, (gg_u64)bad);
}

// best[i] = min over the targets of the split of D(i, j) << 32 | j
static __global__ __launch_bounds__(GG_WAVES * 64) void k_gg_match(const gg_v4i* __restrict__ S, const int* __restrict__ sn, long long ns,
                                                                   const gg_v4i* __restrict__ T, const int* __restrict__ tn, long long nt,
                                                                   long long tiles, long long tiles_per_split, gg_u64* __restrict__ best) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, grp = lane >> 4;
    const long long s0 = ((long long)blockIdx.x * GG_WAVES + wave) * 16;
    if (s0 >= ns) return;                                         // (the whole wave; the rows up to the next multiple of 16 exist as zero rows)
    const long long srow = s0 + col;
    const gg_v4i zero = {0, 0, 0, 0};
    const gg_v4i b = grp < 3 ? S[srow * 3 + grp] : zero;
    const int mine = -sn[srow];                                   // |s|^2
    const long long tile0 = (long long)blockIdx.y * tiles_per_split;
    const long long tile1 = min(tiles, tile0 + tiles_per_split);
    // the smallest D is the largest e = 2 s.t - |t|^2 (|s|^2 is the lane's constant).  A padding row has e = GG_PAD_NORM exactly, which the strict >
    // never takes.  Most tiles change nothing: the index is worked out only when the maximum of the lane's four rows beats the running one.
    int be = GG_PAD_NORM, bj = INT_MAX;
    auto visit = [&](long long base, const gg_v4i& a, const gg_v4i& neg) {
        const gg_v4i acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, zero, 0, 0, 0);
        const int e0 = 2 * acc[0] + neg[0], e1 = 2 * acc[1] + neg[1], e2 = 2 * acc[2] + neg[2], e3 = 2 * acc[3] + neg[3];
        const int m = max(max(e0, e1), max(e2, e3));
        if (m > be) {                                             // ascending tiles, strict: the first of equal distances stays
            be = m;
            bj = (int)base + 4 * grp + (e0 == m ? 0 : e1 == m ? 1 : e2 == m ? 2 : 3);   // ascending rows: the first at the maximum
        }
    };
    long long tile = tile0;
    for (; tile + GG_UNROLL <= tile1; tile += GG_UNROLL) {        // the loads of GG_UNROLL tiles in flight before the first product
        gg_v4i a[GG_UNROLL], nrm[GG_UNROLL];
#pragma unroll
        for (int u = 0; u < GG_UNROLL; ++u) {
            const long long base = (tile + u) * 16;
            a[u] = grp < 3 ? T[(base + col) * 3 + grp] : zero;
            nrm[u] = *(const gg_v4i*)(tn + base + 4 * grp);
        }
#pragma unroll
        for (int u = 0; u < GG_UNROLL; ++u) visit((tile + u) * 16, a[u], nrm[u]);
    }
    for (; tile < tile1; ++tile) {
        const long long base = tile * 16;
        visit(base, grp < 3 ? T[(base + col) * 3 + grp] : zero, *(const gg_v4i*)(tn + base + 4 * grp));
    }
    gg_u64 key = (gg_u64)(unsigned)(mine - be) << 32 | (unsigned)bj;
    gg_u64 o = __shfl_xor(key, 16);
    key = o < key ? o : key;
    o = __shfl_xor(key, 32);
    key = o < key ? o : key;
    if (grp == 0 && srow < ns && (unsigned)key != (unsigned)INT_MAX) atomicMin(best + srow, key);
}

// index / dist from the keys; with back (the keys of the search from the targets) index = -1 where the match's own match is another point
static __global__ __launch_bounds__(CH_THREADS) void k_gg_match_final(const gg_u64* __restrict__ fwd, const gg_u64* __restrict__ back, long long ns,
                                                                      long long nt, int* __restrict__ index, int* __restrict__ dist) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= ns) return;
    const gg_u64 key = fwd[i];
    long long j = (long long)(unsigned)key;
    if (j >= nt)                                                  // (an untouched key: cannot happen, every source meets every target)
        j = -1;
    else if (back && (long long)(unsigned)back[j] != i)
        j = -1;
    index[i] = (int)j;
    dist[i] = (int)(key >> 32);
}

static inline long long gg_pad16(long long n) { return (n + 15) / 16 * 16; }

// the number of target splits and the tiles of each
static void gg_match_splits(long long ns, long long nt, long long* splits, long long* per) {
    const long long blocks = mv_ceil_div(ns, GG_WAVES * 16), tiles = mv_ceil_div(nt, 16);
    long long want = GG_TARGET_BLOCKS / blocks;
    const long long most = mv_ceil_div(tiles, GG_MIN_TILES);
    if (want > most) want = most;
    if (want < 1) want = 1;
    *per = mv_ceil_div(tiles, want);
    *splits = mv_ceil_div(tiles, *per);
}

struct GgMatchLayout {
    size_t sp, sn, tp, tn, fwd, back, total;
};

static bool gg_match_layout(long long ns, long long nt, GgMatchLayout* L) {
    if (ns < 1 || nt < 1 || ns > INT_MAX || nt > INT_MAX) return false;
    WsCursor c{CH_HDR};
    L->sp = c.take((size_t)gg_pad16(ns) * GG_ROW);
    L->sn = c.take((size_t)gg_pad16(ns) * 4);
    L->tp = c.take((size_t)gg_pad16(nt) * GG_ROW);
    L->tn = c.take((size_t)gg_pad16(nt) * 4);
    L->fwd = c.take((size_t)ns * 8);
    L->back = c.take((size_t)nt * 8);
    L->total = c.o;
    return true;
}

static void gg_launch_match(const char* w, size_t sp, size_t sn, long long ns, size_t tp, size_t tn, long long nt, gg_u64* best, hipStream_t s) {
    long long splits, per;
    gg_match_splits(ns, nt, &splits, &per);
    hipLaunchKernelGGL(k_gg_match, dim3(mv_grid(ns, GG_WAVES * 16), (unsigned)splits), dim3(GG_WAVES * 64), 0, s, (const gg_v4i*)(w + sp), (const int*)(w + sn), ns,
                       (const gg_v4i*)(w + tp), (const int*)(w + tn), nt, mv_ceil_div(nt, 16), per, best);
}

// ================================================================ stage 4: the hypothesis search ================================================================
__device__ __forceinline__ gg_u64 gg_mix(gg_u64 seed, gg_u64 counter) {
    gg_u64 x = seed ^ (counter * 0x9E3779B97F4A7C15ull);
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

__device__ __forceinline__ double gg_d2(const double* q, const double* r) {
    const double dx = q[0] - r[0], dy = q[1] - r[1], dz = q[2] - r[2];
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ void gg_move(const double* T, const double* p, double* o) {
    for (int a = 0; a < 3; ++a) o[a] = ((T[a * 4] * p[0] + T[a * 4 + 1] * p[1]) + T[a * 4 + 2] * p[2]) + T[a * 4 + 3];
}

// one Jacobi rotation of registration.horn_rotation at the constant pair (P, Q)
template <int P, int Q>
__device__ __forceinline__ void gg_rotate(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2 * apq);
    const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1));
    const double c = 1 / sqrt(t * t + 1);
    const double s = t * c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double xp = A[k][P], xq = A[k][Q];
        A[k][P] = c * xp - s * xq;
        A[k][Q] = s * xp + c * xq;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double xp = A[P][k], xq = A[Q][k];
        A[P][k] = c * xp - s * xq;
        A[Q][k] = s * xp + c * xq;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double xp = V[k][P], xq = V[k][Q];
        V[k][P] = c * xp - s * xq;
        V[k][Q] = s * xp + c * xq;
    }
    A[P][Q] = 0.0;
    A[Q][P] = 0.0;
}

// registration.horn_update with n = 3 over the pairs (s[i], t[i]), centred at t[0] -> T (3 x 4, row-major)
__device__ __forceinline__ void gg_fit3(const double (&s)[3][3], const double (&t)[3][3], double* T) {
    const double n = 3.0;
    double sp[3] = {0.0, 0.0, 0.0}, sq[3] = {0.0, 0.0, 0.0}, spq[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const double ctr[3] = {t[0][0], t[0][1], t[0][2]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double p[3], q[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            p[a] = s[i][a] - ctr[a];
            q[a] = t[i][a] - ctr[a];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            sp[a] = sp[a] + p[a];
            sq[a] = sq[a] + q[a];
#pragma unroll
            for (int b = 0; b < 3; ++b) spq[3 * a + b] = spq[3 * a + b] + p[a] * q[b];
        }
    }
    double M[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) M[a][b] = spq[3 * a + b] - (sp[a] * sq[b]) / n;
    const double Sxx = M[0][0], Sxy = M[0][1], Sxz = M[0][2], Syx = M[1][0], Syy = M[1][1], Syz = M[1][2], Szx = M[2][0], Szy = M[2][1], Szz = M[2][2];
    double A[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
    double V[4][4] = {{1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}, {0.0, 0.0, 0.0, 1.0}};
#pragma unroll 1
    for (int sweep = 0; sweep < 16; ++sweep) {
        gg_rotate<0, 1>(A, V);
        gg_rotate<0, 2>(A, V);
        gg_rotate<0, 3>(A, V);
        gg_rotate<1, 2>(A, V);
        gg_rotate<1, 3>(A, V);
        gg_rotate<2, 3>(A, V);
    }
    double top = A[0][0], w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (A[k][k] > top) {
            top = A[k][k];
            w = V[0][k];
            x = V[1][k];
            y = V[2][k];
            z = V[3][k];
        }
    const double nrm = sqrt(((w * w + x * x) + y * y) + z * z);
    w = w / nrm;
    x = x / nrm;
    y = y / nrm;
    z = z / nrm;
    if (w < 0) {
        w = -w;
        x = -x;
        y = -y;
        z = -z;
    }
    const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)},
                            {2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)},
                            {2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)}};
    double pm[3], qm[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        pm[a] = sp[a] / n + ctr[a];
        qm[a] = sq[a] / n + ctr[a];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        T[a * 4] = R[a][0];
        T[a * 4 + 1] = R[a][1];
        T[a * 4 + 2] = R[a][2];
        T[a * 4 + 3] = qm[a] - ((R[a][0] * pm[0] + R[a][1] * pm[1]) + R[a][2] * pm[2]);
    }
}

// every correspondence: its indices in range (MVSDF_PC_ERR_INDEX), its two points finite (MVSDF_PC_ERR_FINITE)
static __global__ __launch_bounds__(CH_THREADS) void k_gg_corr_check(const double* __restrict__ src, long long ns, const double* __restrict__ dst, long long nd,
                                                                     const int* __restrict__ corr, long long m, long long* err) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= m) return;
    const long long a = corr[2 * i], b = corr[2 * i + 1];
    int bad = 0;
    if (a < 0 || a >= ns || b < 0 || b >= nd)
        bad = MVSDF_PC_ERR_INDEX;
    else if (!ch_finite3(src + a * 3) || !ch_finite3(dst + b * 3))
        bad = MVSDF_PC_ERR_FINITE;
    if (bad) atomicOr((gg_u64*)err, (gg_u64)bad);
}

// the workspace header (int64 words): the results the host reads (MVSDF_GREG_RANSAC_H_*), then the two words the kernels combine into
enum { GG_H_BEST = 16, GG_H_COUNT = 17 };
static_assert(GG_H_BEST >= MVSDF_GREG_RANSAC_H_WORDS && GG_H_COUNT >= MVSDF_GREG_RANSAC_H_WORDS && (GG_H_COUNT + 1) * 8 <= CH_HDR &&
                  MVSDF_GREG_RANSAC_H_WORDS * 8 <= CH_HDR && MVSDF_ERRW_H_WORDS * 8 <= CH_HDR,
              "the private words lie behind the public ones, inside the header");

static __global__ __launch_bounds__(CH_THREADS) void k_gg_hyp(const double* __restrict__ src, long long ns, const double* __restrict__ dst, long long nd,
                                                              const int* __restrict__ corr, long long m, long long hyps, gg_u64 seed, double ratio,
                                                              double max_dist, int* __restrict__ list, double* __restrict__ Ts, unsigned int* count) {
    const long long h = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (h >= hyps) return;
    long long mm[3], a[3], b[3];
    for (int t = 0; t < 3; ++t) {
        mm[t] = (long long)(((gg_mix(seed, 3ull * (gg_u64)h + t) >> 32) * (gg_u64)m) >> 32);
        a[t] = corr[2 * mm[t]];
        b[t] = corr[2 * mm[t] + 1];
        if (a[t] < 0 || a[t] >= ns || b[t] < 0 || b[t] >= nd) return;   // (k_gg_corr_check raises the error bit)
    }
    if (mm[0] == mm[1] || mm[0] == mm[2] || mm[1] == mm[2] || a[0] == a[1] || a[0] == a[2] || a[1] == a[2] || b[0] == b[1] || b[0] == b[2] || b[1] == b[2])
        return;
    double s[3][3], t[3][3];
    for (int i = 0; i < 3; ++i)
        for (int c = 0; c < 3; ++c) {
            s[i][c] = src[a[i] * 3 + c];
            t[i][c] = dst[b[i] * 3 + c];
        }
    for (int e = 0; e < 3; ++e) {
        const int u = e == 2 ? 1 : 0, v = e == 0 ? 1 : 2;
        const double ls = sqrt(gg_d2(s[u], s[v])), lt = sqrt(gg_d2(t[u], t[v]));
        if (!(ls >= ratio * lt && lt >= ratio * ls)) return;
    }
    double T[12];
    gg_fit3(s, t, T);
    const double md2 = max_dist * max_dist;
    for (int i = 0; i < 3; ++i) {
        double moved[3];
        gg_move(T, s[i], moved);
        if (!(gg_d2(moved, t[i]) < md2)) return;
    }
    const unsigned slot = atomicAdd(count, 1u);
    list[slot] = (int)h;
    for (int q = 0; q < 12; ++q) Ts[(long long)slot * 12 + q] = T[q];
}

static __global__ __launch_bounds__(CH_THREADS) void k_gg_score(const double* __restrict__ src, long long ns, const double* __restrict__ dst, long long nd,
                                                                const int* __restrict__ corr, long long m, double max_dist, const int* __restrict__ list,
                                                                const double* __restrict__ Ts, const unsigned int* __restrict__ count, gg_u64* best) {
    __shared__ double T[12];
    __shared__ unsigned int total;
    const double md2 = max_dist * max_dist;
    const unsigned int entries = *count;
    for (unsigned int e = blockIdx.x; e < entries; e += gridDim.x) {
        if (threadIdx.x < 12) T[threadIdx.x] = Ts[(long long)e * 12 + threadIdx.x];
        if (threadIdx.x == 0) total = 0;
        __syncthreads();
        unsigned int mine = 0;
        for (long long i = threadIdx.x; i < m; i += CH_THREADS) {
            const long long a = corr[2 * i], b = corr[2 * i + 1];
            if (a < 0 || a >= ns || b < 0 || b >= nd) continue;
            double moved[3];
            gg_move(T, src + a * 3, moved);
            if (gg_d2(moved, dst + b * 3) < md2) ++mine;
        }
        if (mine) atomicAdd(&total, mine);
        __syncthreads();
        if (threadIdx.x == 0) atomicMax(best, (gg_u64)total << 32 | (unsigned)~list[e]);
        __syncthreads();
    }
}

// the header's results from the best key; the winner's T (the identity when nothing survived)
static __global__ __launch_bounds__(CH_THREADS) void k_gg_winner(const int* __restrict__ list, const double* __restrict__ Ts, long long* hdr) {
    const long long e = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    const gg_u64 best = (gg_u64)hdr[GG_H_BEST];
    const long long entries = hdr[GG_H_COUNT] & 0xffffffffll;
    const int h = best ? (int)~(unsigned)best : -1;
    if (e == 0) {
        hdr[MVSDF_GREG_RANSAC_H_HYP] = h;
        hdr[MVSDF_GREG_RANSAC_H_INLIERS] = (long long)(best >> 32);
        hdr[MVSDF_GREG_RANSAC_H_CHECKED] = entries;
        if (!best)
            for (int q = 0; q < 12; ++q) hdr[MVSDF_GREG_RANSAC_H_T + q] = __double_as_longlong(q % 5 == 0 ? 1.0 : 0.0);
    }
    if (best && e < entries && list[e] == h)
        for (int q = 0; q < 12; ++q) hdr[MVSDF_GREG_RANSAC_H_T + q] = __double_as_longlong(Ts[e * 12 + q]);
}

static __global__ __launch_bounds__(CH_THREADS) void k_gg_mask(const double* __restrict__ src, long long ns, const double* __restrict__ dst, long long nd,
                                                               const int* __restrict__ corr, long long m, double max_dist, const long long* __restrict__ hdr,
                                                               unsigned char* __restrict__ mask) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= m) return;
    unsigned char in = 0;
    const long long a = corr[2 * i], b = corr[2 * i + 1];
    if (hdr[GG_H_BEST] && a >= 0 && a < ns && b >= 0 && b < nd) {
        double T[12], moved[3];
        for (int q = 0; q < 12; ++q) T[q] = __longlong_as_double(hdr[MVSDF_GREG_RANSAC_H_T + q]);
        gg_move(T, src + a * 3, moved);
        in = gg_d2(moved, dst + b * 3) < max_dist * max_dist ? 1 : 0;
    }
    mask[i] = in;
}

struct GgRansacLayout {
    size_t list, Ts, total;
};

static bool gg_ransac_layout(long long m, long long hyps, GgRansacLayout* L) {
    if (m < 3 || m > INT_MAX || hyps < 1 || hyps > MVSDF_GREG_MAX_HYPOTHESES) return false;
    WsCursor c{CH_HDR};
    L->list = c.take((size_t)hyps * 4);
    L->Ts = c.take((size_t)hyps * 12 * 8);
    L->total = c.o;
    return true;
}

extern "C" {

int mvsdf_greg_spfh(const double* pts, const double* normals, const int32_t* neighbors, int64_t n, int32_t k, double radius2, int32_t* hist,
                    int32_t* count, int32_t* err, void* stream) {
    if (!pts || !normals || !neighbors || !hist || !count || !err || n < 1 || n > INT_MAX || k < 1 || k > MVSDF_PC_MAX_K || !(radius2 > 0))
        return mv_fail(-1, "mvsdf_greg_spfh: bad arguments");
    hipLaunchKernelGGL(k_gg_spfh, dim3(mv_grid(n, CH_THREADS)), dim3(CH_THREADS), 0, (hipStream_t)stream, pts, normals, (const int*)neighbors, (long long)n,
                       (int)k, radius2, (int*)hist, (int*)count, (int*)err);
    return mv_check(hipGetLastError(), "mvsdf_greg_spfh");
}

int mvsdf_greg_fpfh(const double* pts, const int32_t* neighbors, const int32_t* hist, const int32_t* count, int64_t n, int32_t k, double radius2,
                    double* features, int8_t* codes, int32_t* err, void* stream) {
    if (!pts || !neighbors || !hist || !count || !features || !codes || !err || n < 1 || n > INT_MAX || k < 1 || k > MVSDF_PC_MAX_K || !(radius2 > 0))
        return mv_fail(-1, "mvsdf_greg_fpfh: bad arguments");
    hipLaunchKernelGGL(k_gg_fpfh, dim3(mv_grid(n, CH_THREADS)), dim3(CH_THREADS), 0, (hipStream_t)stream, pts, (const int*)neighbors, (const int*)hist,
                       (const int*)count, (long long)n, (int)k, radius2, features, (signed char*)codes, (int*)err);
    return mv_check(hipGetLastError(), "mvsdf_greg_fpfh");
}

size_t mvsdf_greg_match_workspace_bytes(int64_t ns, int64_t nt) {
    GgMatchLayout L;
    return gg_match_layout(ns, nt, &L) ? L.total : 0;
}

int32_t mvsdf_greg_match_splits(int64_t ns, int64_t nt) {
    if (ns < 1 || nt < 1 || ns > INT_MAX || nt > INT_MAX) return 0;
    long long splits, per;
    gg_match_splits(ns, nt, &splits, &per);
    return (int32_t)splits;
}

int mvsdf_greg_match(const int8_t* src, int64_t ns, const int8_t* dst, int64_t nt, int32_t mutual, void* ws, size_t ws_bytes, int32_t* index,
                     int32_t* dist, void* stream) {
    GgMatchLayout L;
    if (!src || !dst || !ws || !index || !dist || !gg_match_layout(ns, nt, &L)) return mv_fail(-1, "mvsdf_greg_match: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_greg_match: workspace too small (mvsdf_greg_match_workspace_bytes)");
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    const long long sp = gg_pad16(ns), tp = gg_pad16(nt);
    int rc;
    if ((rc = mv_check(hipMemsetAsync(w, 0, CH_HDR, s), "mvsdf_greg_match"))) return rc;
    if ((rc = mv_check(hipMemsetAsync(w + L.fwd, 0xff, (size_t)ns * 8, s), "mvsdf_greg_match"))) return rc;
    hipLaunchKernelGGL(k_gg_pack, dim3(mv_grid(sp, CH_THREADS)), dim3(CH_THREADS), 0, s, (const signed char*)src, (long long)ns, sp, (int*)(w + L.sp),
                       (int*)(w + L.sn), (long long*)w);
    hipLaunchKernelGGL(k_gg_pack, dim3(mv_grid(tp, CH_THREADS)), dim3(CH_THREADS), 0, s, (const signed char*)dst, (long long)nt, tp, (int*)(w + L.tp),
                       (int*)(w + L.tn), (long long*)w);
    gg_launch_match(w, L.sp, L.sn, (long long)ns, L.tp, L.tn, (long long)nt, (gg_u64*)(w + L.fwd), s);
    if (mutual) {
        if ((rc = mv_check(hipMemsetAsync(w + L.back, 0xff, (size_t)nt * 8, s), "mvsdf_greg_match"))) return rc;
        gg_launch_match(w, L.tp, L.tn, (long long)nt, L.sp, L.sn, (long long)ns, (gg_u64*)(w + L.back), s);
    }
    hipLaunchKernelGGL(k_gg_match_final, dim3(mv_grid(ns, CH_THREADS)), dim3(CH_THREADS), 0, s, (const gg_u64*)(w + L.fwd),
                       mutual ? (const gg_u64*)(w + L.back) : (const gg_u64*)nullptr, (long long)ns, (long long)nt, (int*)index, (int*)dist);
    return mv_check(hipGetLastError(), "mvsdf_greg_match");
}

size_t mvsdf_greg_ransac_workspace_bytes(int64_t m, int64_t hypotheses) {
    GgRansacLayout L;
    return gg_ransac_layout(m, hypotheses, &L) ? L.total : 0;
}

int mvsdf_greg_ransac(const double* src, int64_t ns, const double* dst, int64_t nd, const int32_t* corr, int64_t m, int64_t hypotheses, uint64_t seed,
                      double edge_ratio, double max_dist, void* ws, size_t ws_bytes, uint8_t* mask, void* stream) {
    GgRansacLayout L;
    if (!src || !dst || !corr || !ws || !mask || ns < 1 || nd < 1 || ns > INT_MAX || nd > INT_MAX || !gg_ransac_layout(m, hypotheses, &L) ||
        !(max_dist > 0) || !(edge_ratio >= 0))
        return mv_fail(-1, "mvsdf_greg_ransac: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_greg_ransac: workspace too small (mvsdf_greg_ransac_workspace_bytes)");
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    long long* hdr = (long long*)w;
    int* list = (int*)(w + L.list);
    double* Ts = (double*)(w + L.Ts);
    const long long H = (long long)hypotheses, M = (long long)m;
    int rc;
    if ((rc = mv_check(hipMemsetAsync(w, 0, CH_HDR, s), "mvsdf_greg_ransac"))) return rc;
    hipLaunchKernelGGL(k_gg_corr_check, dim3(mv_grid(M, CH_THREADS)), dim3(CH_THREADS), 0, s, src, (long long)ns, dst, (long long)nd, (const int*)corr, M,
                       hdr + MVSDF_GREG_RANSAC_H_ERR);
    hipLaunchKernelGGL(k_gg_hyp, dim3(mv_grid(H, CH_THREADS)), dim3(CH_THREADS), 0, s, src, (long long)ns, dst, (long long)nd, (const int*)corr, M, H,
                       (gg_u64)seed, edge_ratio, max_dist, list, Ts, (unsigned int*)(hdr + GG_H_COUNT));
    const unsigned blocks = (unsigned)(H < GG_SCORE_BLOCKS ? H : GG_SCORE_BLOCKS);
    hipLaunchKernelGGL(k_gg_score, dim3(blocks), dim3(CH_THREADS), 0, s, src, (long long)ns, dst, (long long)nd, (const int*)corr, M, max_dist, (const int*)list,
                       (const double*)Ts, (const unsigned int*)(hdr + GG_H_COUNT), (gg_u64*)(hdr + GG_H_BEST));
    hipLaunchKernelGGL(k_gg_winner, dim3(mv_grid(H, CH_THREADS)), dim3(CH_THREADS), 0, s, (const int*)list, (const double*)Ts, hdr);
    hipLaunchKernelGGL(k_gg_mask, dim3(mv_grid(M, CH_THREADS)), dim3(CH_THREADS), 0, s, src, (long long)ns, dst, (long long)nd, (const int*)corr, M, max_dist,
                       (const long long*)hdr, (unsigned char*)mask);
    return mv_check(hipGetLastError(), "mvsdf_greg_ransac");
}

}  // extern "C"
