// bundle.hip -- bundle adjustment on the device: Levenberg-Marquardt over poses and points, the points eliminated (Schur complement), the reduced
// camera system solved matrix-free by conjugate gradients with a block-Jacobi preconditioner.  Python: mvsdf_amd/bundle.py, which states the
// definition; tests/bundle_ref.py restates it in numpy.  fp64 in the order the definition writes it, no contraction, no float atomics.
//
// * one lane per observation: k_ba_cost (residual, robust cost term), k_ba_lin (weighted residual, A 2x6, B 2x3 in track order; the 21 + 6 terms of
//   U and g_c at the observation's place in view order);
// * one lane per point: k_ba_point (V, g_p, the damped inverse, the terms of W V^-1 g_p), k_ba_sx_point (y = V^-1 sum W^T x, the terms of W y),
//   k_ba_step_point;
// * one workgroup per (view, quantity): k_ba_seg_tree, the canonical pairwise tree over a segment (chunks of 2048 in adjacent-pair order, then the
//   chunk sums likewise: geom_prims.h's mv_tree_chunk, which poisson.hip's k_po_tree shares); k_ba_chunk_tree is its first level over one long array (the cost);
// * one workgroup: k_ba_cg_init, k_ba_cg_update (the 6 V entry trees and the solver's state), k_ba_accept (one lane: the step's acceptance).
// The state block at the start of the workspace (BA_ST_*) holds lambda, the costs, which of the two parameter buffers is current, and the stop and
// done flags; every kernel reads them and returns when there is nothing left to do, so a whole call is enqueued without a host wait.  State words
// are written by ordinary stores of one lane; the error word by integer atomicOr.
//
// Bounds: k_ba_check runs first and every later kernel returns while an error bit is set, so offsets ascend within [0, nnz] and views lie in
// [0, V) wherever they index; sorted values are a permutation of [0, nnz); a view's chunk count is at most 2048 by MVSDF_BA_MAX_OBS.
#include "nn_tree.h"

#define BA_T 256
#define BA_ITEMS 8
#define BA_CHUNK (BA_T * BA_ITEMS)
#define BA_HDR 512                                    // bytes of the state block
#define BA_UG 27                                      // 21 entries of the upper triangle of U, 6 of g_c

enum {                                                // state words after MVSDF_BA_H_*
    BA_ST_CUR = 8,                                    // which parameter buffer is current
    BA_ST_STOP = 9,                                   // converged: every later launch returns
    BA_ST_TRIAL = 10,                                 // the trial cost
    BA_ST_THETA = 11,                                 // the trial step rotates a view beyond the bound
    BA_ST_CGDONE = 12,                                // the solve is done: its remaining launches return
    BA_ST_RHO = 13,
    BA_ST_RHO0 = 14,
    BA_ST_SEG = 16                                    // {0, nnz, 0, chunks of nnz}: the segments of the cost's tree
};

struct BaP {
    long long V, P, nnz;
    long long* st;
    double* pose[2];
    double* X[2];
    double* intr;
    long long* toff;
    int* tview;
    const double* obs;
    unsigned char* fixed;
    int* owner;
    int* pos;
    long long* voff;
    double *A, *B, *rw, *cterm, *T, *part;
    double *Vraw, *Vinv, *gp;
    double *Ug, *Wt, *Ud, *Minv, *b;
    double *x, *r, *z, *p;
};

__device__ __forceinline__ bool ba_off(const long long* st) { return st[MVSDF_BA_H_ERR] != 0 || st[BA_ST_STOP] != 0; }
__device__ __forceinline__ double ba_get(const long long* st, int w) { return __longlong_as_double(st[w]); }
__device__ __forceinline__ void ba_put(long long* st, int w, double v) { st[w] = __double_as_longlong(v); }
__host__ __device__ constexpr int ba_sym(int k, int l) { return k <= l ? k * 6 - k * (k - 1) / 2 + (l - k) : l * 6 - l * (l - 1) / 2 + (k - l); }

// ================================================================ the trees ================================================================
static_assert(BA_T == MV_THREADS && BA_ITEMS == MV_ITEMS, "the chunk of geom_prims.h's tree");

// out[seg * K + k] = the tree sum of in[k * stride + seg_off[seg] .. seg_off[seg + 1]); grid (segments, K)
static __global__ __launch_bounds__(BA_T) void k_ba_seg_tree(const double* __restrict__ in, long long stride, const long long* __restrict__ seg_off,
                                                             double* __restrict__ out, const long long* __restrict__ st, int guard) {
    __shared__ double sh[BA_T];
    __shared__ double chunk[BA_CHUNK];
    if (ba_off(st) || (guard && st[BA_ST_CGDONE])) return;
    const int t = threadIdx.x, k = blockIdx.y, K = gridDim.y;
    const long long s0 = seg_off[blockIdx.x], n = seg_off[blockIdx.x + 1] - s0;
    const double* __restrict__ src = in + (long long)k * stride + s0;
    long long nc = (n + BA_CHUNK - 1) / BA_CHUNK;
    nc = nc < 1 ? 1 : (nc > BA_CHUNK ? BA_CHUNK : nc);
    double a[BA_ITEMS], v = 0.0;
    for (long long c = 0; c < nc; ++c) {
        const long long base = c * BA_CHUNK + (long long)t * BA_ITEMS;
#pragma unroll
        for (int q = 0; q < BA_ITEMS; ++q) a[q] = base + q < n ? src[base + q] : 0.0;
        v = mv_tree_chunk(a, sh);
        if (t == 0) chunk[c] = v;
    }
    if (nc > 1) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < BA_ITEMS; ++q) a[q] = t * BA_ITEMS + q < nc ? chunk[t * BA_ITEMS + q] : 0.0;
        v = mv_tree_chunk(a, sh);
    }
    if (t == 0) out[(long long)blockIdx.x * K + k] = v;
}

// out[b] = the tree sum of chunk b of in[n]
static __global__ __launch_bounds__(BA_T) void k_ba_chunk_tree(const double* __restrict__ in, long long n, double* __restrict__ out,
                                                               const long long* __restrict__ st) {
    __shared__ double sh[BA_T];
    if (ba_off(st)) return;
    const long long base = (long long)blockIdx.x * BA_CHUNK + (long long)threadIdx.x * BA_ITEMS;
    double a[BA_ITEMS];
#pragma unroll
    for (int q = 0; q < BA_ITEMS; ++q) a[q] = base + q < n ? in[base + q] : 0.0;
    const double v = mv_tree_chunk(a, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = v;
}

// ================================================================ checks and orders ================================================================
static __global__ __launch_bounds__(BA_T) void k_ba_check(const long long* __restrict__ toff, const int* __restrict__ tview, long long V, long long P,
                                                          long long nnz, long long* st) {
    const long long i = (long long)blockIdx.x * BA_T + threadIdx.x;
    bool bad = false;
    if (i < P) {
        const long long a = toff[i], b = toff[i + 1];
        bad = a < 0 || b < a || b > nnz || (i == 0 && a != 0) || (i == P - 1 && b != nnz);
    }
    if (i < nnz) bad = bad || tview[i] < 0 || tview[i] >= V;
    if (bad) atomicOr((unsigned long long*)st + MVSDF_BA_H_ERR, (unsigned long long)MVSDF_PS_ERR_INDEX);
}

// one lane per point: the owner of its observations, and the sort's keys (view) and values (observation)
static __global__ __launch_bounds__(BA_T) void k_ba_owner(BaP p, unsigned long long* __restrict__ key, int* __restrict__ val) {
    const long long j = (long long)blockIdx.x * BA_T + threadIdx.x;
    if (ba_off(p.st) || j >= p.P) return;
    for (long long o = p.toff[j]; o < p.toff[j + 1]; ++o) {
        p.owner[o] = (int)j;
        key[o] = (unsigned long long)p.tview[o];
        val[o] = (int)o;
    }
}

// one lane per sorted place (and one past the end): where every view begins, and the place of every observation
static __global__ __launch_bounds__(BA_T) void k_ba_segments(BaP p, const unsigned long long* __restrict__ key, const int* __restrict__ val) {
    const long long i = (long long)blockIdx.x * BA_T + threadIdx.x;
    if (ba_off(p.st) || i > p.nnz) return;
    const long long lo = i == 0 ? 0 : (long long)key[i - 1] + 1, hi = i == p.nnz ? p.V : (long long)key[i];
    for (long long v = lo; v <= hi && v <= p.V; ++v) p.voff[v] = i;
    if (i < p.nnz) p.pos[val[i]] = (int)i;
}

// ================================================================ one lane per observation ================================================================
struct BaProj {
    double q0, q1, q2, u, v, r0, r1;
};

// q = R X + t, each row ((a + b) + c) + t; r as the definition writes it; false: behind
__device__ __forceinline__ bool ba_project(const double* __restrict__ ps, const double* __restrict__ in, const double* __restrict__ X,
                                           const double* __restrict__ xy, BaProj& o) {
    const double x0 = X[0], x1 = X[1], x2 = X[2];
    o.q0 = ((ps[0] * x0 + ps[1] * x1) + ps[2] * x2) + ps[9];
    o.q1 = ((ps[3] * x0 + ps[4] * x1) + ps[5] * x2) + ps[10];
    o.q2 = ((ps[6] * x0 + ps[7] * x1) + ps[8] * x2) + ps[11];
    if (!(o.q2 > 0.0)) return false;
    o.u = o.q0 / o.q2;
    o.v = o.q1 / o.q2;
    o.r0 = ((in[0] * o.u + in[1] * o.v) + in[2]) - xy[0];
    o.r1 = (in[3] * o.v + in[4]) - xy[1];
    return true;
}

// which: 0 the current parameters, 1 the other buffer.  force: also after convergence (the final residuals).  trial != 0: behind gives +inf; else the error bit.  r (may be null): [nnz][2]
static __global__ __launch_bounds__(BA_T) void k_ba_cost(BaP p, int which, int trial, int force, double delta, double* __restrict__ r,
                                                         double* __restrict__ terms) {
    const long long o = (long long)blockIdx.x * BA_T + threadIdx.x;
    if (p.st[MVSDF_BA_H_ERR] != 0 || (!force && p.st[BA_ST_STOP] != 0) || o >= p.nnz) return;
    const int buf = (int)(p.st[BA_ST_CUR] & 1) ^ which, j = p.owner[o], v = p.tview[o];
    double r0 = 0.0, r1 = 0.0, c = 0.0;
    if (p.toff[j + 1] - p.toff[j] >= 2) {
        BaProj m;
        if (ba_project(p.pose[buf] + 12 * v, p.intr + 5 * v, p.X[buf] + 3 * (long long)j, p.obs + 2 * o, m)) {
            r0 = m.r0;
            r1 = m.r1;
            const double s2 = r0 * r0 + r1 * r1, n = sqrt(s2);
            c = n <= delta ? 0.5 * s2 : delta * (n - 0.5 * delta);
        } else if (trial) {
            c = INFINITY;
        } else {
            atomicOr((unsigned long long*)p.st + MVSDF_BA_H_ERR, (unsigned long long)MVSDF_PS_ERR_BEHIND);
        }
    }
    if (r) {
        r[2 * o] = r0;
        r[2 * o + 1] = r1;
    }
    terms[o] = c;
}

static __global__ __launch_bounds__(BA_T) void k_ba_lin(BaP p, double delta) {
    const long long o = (long long)blockIdx.x * BA_T + threadIdx.x;
    if (ba_off(p.st) || o >= p.nnz) return;
    const int buf = (int)(p.st[BA_ST_CUR] & 1), j = p.owner[o], v = p.tview[o];
    const long long n = p.nnz, at = p.pos[o];
    const double* __restrict__ ps = p.pose[buf] + 12 * v;
    const double* __restrict__ in = p.intr + 5 * v;
    double A[2][6], B[2][3], r[2];
    BaProj m;
    const bool active = p.toff[j + 1] - p.toff[j] >= 2 && ba_project(ps, in, p.X[buf] + 3 * (long long)j, p.obs + 2 * o, m);
    if (active) {
        const double nr = sqrt(m.r0 * m.r0 + m.r1 * m.r1), w = nr <= delta ? 1.0 : delta / nr, sw = sqrt(w);
        double D[2][3];
        D[0][0] = in[0] / m.q2;
        D[0][1] = in[1] / m.q2;
        D[0][2] = -((in[0] * m.u + in[1] * m.v) / m.q2);
        D[1][0] = 0.0;
        D[1][1] = in[3] / m.q2;
        D[1][2] = -((in[3] * m.v) / m.q2);
        r[0] = m.r0 * sw;
        r[1] = m.r1 * sw;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            A[e][0] = (D[e][2] * m.q1 - D[e][1] * m.q2) * sw;
            A[e][1] = (D[e][0] * m.q2 - D[e][2] * m.q0) * sw;
            A[e][2] = (D[e][1] * m.q0 - D[e][0] * m.q1) * sw;
#pragma unroll
            for (int l = 0; l < 3; ++l) {
                A[e][3 + l] = D[e][l] * sw;
                B[e][l] = ((D[e][0] * ps[l] + D[e][1] * ps[3 + l]) + D[e][2] * ps[6 + l]) * sw;
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            r[e] = 0.0;
#pragma unroll
            for (int l = 0; l < 6; ++l) A[e][l] = 0.0;
#pragma unroll
            for (int l = 0; l < 3; ++l) B[e][l] = 0.0;
        }
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        p.rw[e * n + o] = r[e];
#pragma unroll
        for (int l = 0; l < 6; ++l) p.A[(e * 6 + l) * n + o] = A[e][l];
#pragma unroll
        for (int l = 0; l < 3; ++l) p.B[(e * 3 + l) * n + o] = B[e][l];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
        for (int l = k; l < 6; ++l) p.T[ba_sym(k, l) * n + at] = A[0][k] * A[0][l] + A[1][k] * A[1][l];
        p.T[(21 + k) * n + at] = A[0][k] * r[0] + A[1][k] * r[1];
    }
}

// ================================================================ one lane per point ================================================================
// the terms of W_o y over a track, at the observations' places in view order: A^T (B y)
__device__ __forceinline__ void ba_emit_wy(const BaP& p, long long j, const double* y) {
    const long long n = p.nnz;
    for (long long o = p.toff[j]; o < p.toff[j + 1]; ++o) {
        const long long at = p.pos[o];
        const double t0 = (p.B[0 * n + o] * y[0] + p.B[1 * n + o] * y[1]) + p.B[2 * n + o] * y[2];
        const double t1 = (p.B[3 * n + o] * y[0] + p.B[4 * n + o] * y[1]) + p.B[5 * n + o] * y[2];
#pragma unroll
        for (int k = 0; k < 6; ++k) p.T[k * n + at] = p.A[k * n + o] * t0 + p.A[(6 + k) * n + o] * t1;
    }
}

// acc = the sum over the track, from 0.0, of W_o^T x_view = B^T (A x)
__device__ __forceinline__ void ba_wtx(const BaP& p, long long j, const double* __restrict__ x, double* acc) {
    const long long n = p.nnz;
    acc[0] = acc[1] = acc[2] = 0.0;
    for (long long o = p.toff[j]; o < p.toff[j + 1]; ++o) {
        const double* __restrict__ xv = x + 6 * (long long)p.tview[o];
        double u0 = 0.0, u1 = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            u0 = u0 + p.A[k * n + o] * xv[k];
            u1 = u1 + p.A[(6 + k) * n + o] * xv[k];
        }
#pragma unroll
        for (int l = 0; l < 3; ++l) acc[l] = acc[l] + (p.B[l * n + o] * u0 + p.B[(3 + l) * n + o] * u1);
    }
}

// y = Vinv a with the symmetric Vinv of point j
__device__ __forceinline__ void ba_vinv_mul(const BaP& p, long long j, const double* a, double* y) {
    const long long P = p.P;
    const double i00 = p.Vinv[j], i01 = p.Vinv[P + j], i02 = p.Vinv[2 * P + j], i11 = p.Vinv[3 * P + j], i12 = p.Vinv[4 * P + j], i22 = p.Vinv[5 * P + j];
    y[0] = (i00 * a[0] + i01 * a[1]) + i02 * a[2];
    y[1] = (i01 * a[0] + i11 * a[1]) + i12 * a[2];
    y[2] = (i02 * a[0] + i12 * a[1]) + i22 * a[2];
}

static __global__ __launch_bounds__(BA_T) void k_ba_point(BaP p, double floor_diag) {
    const long long j = (long long)blockIdx.x * BA_T + threadIdx.x;
    if (ba_off(p.st) || j >= p.P) return;
    const long long n = p.nnz, P = p.P;
    const double lam = ba_get(p.st, MVSDF_BA_H_LAMBDA);
    double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};      // 00 01 02 11 12 22
    for (long long o = p.toff[j]; o < p.toff[j + 1]; ++o) {
        const double b00 = p.B[o], b01 = p.B[n + o], b02 = p.B[2 * n + o], b10 = p.B[3 * n + o], b11 = p.B[4 * n + o], b12 = p.B[5 * n + o];
        const double r0 = p.rw[o], r1 = p.rw[n + o];
        m[0] = m[0] + (b00 * b00 + b10 * b10);
        m[1] = m[1] + (b00 * b01 + b10 * b11);
        m[2] = m[2] + (b00 * b02 + b10 * b12);
        m[3] = m[3] + (b01 * b01 + b11 * b11);
        m[4] = m[4] + (b01 * b02 + b11 * b12);
        m[5] = m[5] + (b02 * b02 + b12 * b12);
        g[0] = g[0] + (b00 * r0 + b10 * r1);
        g[1] = g[1] + (b01 * r0 + b11 * r1);
        g[2] = g[2] + (b02 * r0 + b12 * r1);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) p.Vraw[k * P + j] = m[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) p.gp[k * P + j] = g[k];
    const double m00 = m[0] + lam * fmax(m[0], floor_diag), m11 = m[3] + lam * fmax(m[3], floor_diag), m22 = m[5] + lam * fmax(m[5], floor_diag);
    const double m01 = m[1], m02 = m[2], m12 = m[4];
    const double det = (m00 * (m11 * m22 - m12 * m12) - m01 * (m01 * m22 - m12 * m02)) + m02 * (m01 * m12 - m11 * m02);
    double inv[6];
    inv[0] = (m11 * m22 - m12 * m12) / det;
    inv[1] = (m02 * m12 - m01 * m22) / det;
    inv[2] = (m01 * m12 - m02 * m11) / det;
    inv[3] = (m00 * m22 - m02 * m02) / det;
    inv[4] = (m01 * m02 - m00 * m12) / det;
    inv[5] = (m00 * m11 - m01 * m01) / det;
    bool ok = p.toff[j + 1] - p.toff[j] >= 2 && det > 0.0 && isfinite(det);
#pragma unroll
    for (int k = 0; k < 6; ++k) ok = ok && isfinite(inv[k]);
#pragma unroll
    for (int k = 0; k < 6; ++k) p.Vinv[k * P + j] = ok ? inv[k] : 0.0;
    double y[3];
    ba_vinv_mul(p, j, g, y);
    ba_emit_wy(p, j, y);
}

// cg != 0: x is the solver's direction p and the launch returns once the solver is done
static __global__ __launch_bounds__(BA_T) void k_ba_sx_point(BaP p, const double* __restrict__ x, int cg) {
    const long long j = (long long)blockIdx.x * BA_T + threadIdx.x;
    if (ba_off(p.st) || (cg && p.st[BA_ST_CGDONE]) || j >= p.P) return;
    double acc[3], y[3];
    ba_wtx(p, j, x, acc);
    ba_vinv_mul(p, j, acc, y);
    ba_emit_wy(p, j, y);
}

static __global__ __launch_bounds__(BA_T) void k_ba_step_point(BaP p, const double* __restrict__ x) {
    const long long j = (long long)blockIdx.x * BA_T + threadIdx.x;
    if (ba_off(p.st) || j >= p.P) return;
    const int buf = (int)(p.st[BA_ST_CUR] & 1);
    double acc[3], d[3];
    ba_wtx(p, j, x, acc);
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] = (-p.gp[k * p.P + j]) - acc[k];
    ba_vinv_mul(p, j, acc, d);
#pragma unroll
    for (int k = 0; k < 3; ++k) p.X[buf ^ 1][3 * j + k] = p.X[buf][3 * j + k] + d[k];
}

// ================================================================ one lane per view ================================================================
static __global__ __launch_bounds__(64) void k_ba_cam(BaP p, double floor_diag) {
    const long long v = (long long)blockIdx.x * 64 + threadIdx.x;
    if (ba_off(p.st) || v >= p.V) return;
    const double lam = ba_get(p.st, MVSDF_BA_H_LAMBDA);
    const double* __restrict__ ug = p.Ug + BA_UG * v;
    double U[6][6], L[6][6], d[6];
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int l = 0; l < 6; ++l) U[k][l] = ug[ba_sym(k, l)];
#pragma unroll
    for (int k = 0; k < 6; ++k) U[k][k] = U[k][k] + lam * fmax(U[k][k], floor_diag);
    bool ok = !p.fixed[v];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double s = U[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s = s - (L[j][k] * L[j][k]) * d[k];
        d[j] = s;
        ok = ok && s > 0.0 && isfinite(s);
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double e = U[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) e = e - (L[i][k] * L[j][k]) * d[k];
            L[i][j] = e / s;
        }
    }
    double M[6][6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double y[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double s = i == c ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
            y[i] = s;
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) y[i] = y[i] / d[i];
#pragma unroll
        for (int i = 5; i >= 0; --i) {
            double s = y[i];
#pragma unroll
            for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * y[k];
            y[i] = s;
            M[i][c] = s;
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int l = 0; l < 6; ++l) ok = ok && isfinite(M[k][l]);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
        for (int l = 0; l < 6; ++l) {
            p.Minv[36 * v + 6 * k + l] = ok ? M[k][l] : 0.0;
            p.Ud[36 * v + 6 * k + l] = U[k][l];
        }
        p.b[6 * v + k] = ok ? (-ug[21 + k]) + p.Wt[6 * v + k] : 0.0;
    }
}

// the pose of a view after its step (omega, upsilon) -> the other buffer; a fixed view and a step beyond the bound copy
static __global__ __launch_bounds__(64) void k_ba_step_cam(BaP p, const double* __restrict__ x, const double* __restrict__ rod) {
    const long long v = (long long)blockIdx.x * 64 + threadIdx.x;
    if (ba_off(p.st) || v >= p.V) return;
    const int buf = (int)(p.st[BA_ST_CUR] & 1);
    const double* __restrict__ ps = p.pose[buf] + 12 * v;
    double* __restrict__ out = p.pose[buf ^ 1] + 12 * v;
    const double w0 = x[6 * v], w1 = x[6 * v + 1], w2 = x[6 * v + 2];
    const double z = (w0 * w0 + w1 * w1) + w2 * w2;
    const bool far = !(z <= (double)MVSDF_BA_MAX_THETA * (double)MVSDF_BA_MAX_THETA);
    if (far) p.st[BA_ST_THETA] = 1;
    if (far || p.fixed[v]) {
#pragma unroll
        for (int k = 0; k < 12; ++k) out[k] = ps[k];
        return;
    }
    double a = rod[MVSDF_BA_ROD_TERMS - 1], b = rod[2 * MVSDF_BA_ROD_TERMS - 1];
#pragma unroll
    for (int k = MVSDF_BA_ROD_TERMS - 2; k >= 0; --k) {
        a = a * z + rod[k];
        b = b * z + rod[MVSDF_BA_ROD_TERMS + k];
    }
    const double w[3] = {w0, w1, w2};
    const double Kx[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
    double E[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int l = 0; l < 3; ++l) E[k][l] = ((k == l ? 1.0 : 0.0) + a * Kx[k][l]) + b * (k == l ? w[k] * w[l] - z : w[k] * w[l]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int l = 0; l < 3; ++l) out[3 * k + l] = (E[k][0] * ps[l] + E[k][1] * ps[3 + l]) + E[k][2] * ps[6 + l];
        out[9 + k] = ((E[k][0] * ps[9] + E[k][1] * ps[10]) + E[k][2] * ps[11]) + x[6 * v + 3 + k];
    }
}

// ================================================================ one workgroup: the solver's state ================================================================
// entry idx = 6 v + k of S vec: the damped U_v vec_v from 0.0 in column order, minus the view's tree sum of W y; +0.0 where the view does not move
__device__ __forceinline__ double ba_sx_entry(const BaP& p, const double* __restrict__ vec, const double* __restrict__ wy, int idx) {
    const int v = idx / 6, k = idx - 6 * v;
    bool moves = false;
    double s = 0.0;
#pragma unroll
    for (int l = 0; l < 6; ++l) {
        s = s + p.Ud[36 * v + 6 * k + l] * vec[6 * v + l];
        moves = moves || p.Minv[36 * v + 7 * l] != 0.0;
    }
    return moves ? s - wy[idx] : 0.0;
}

__device__ __forceinline__ double ba_minv_entry(const BaP& p, const double* __restrict__ vec, int idx) {
    const int v = idx / 6, k = idx - 6 * v;
    double s = 0.0;
#pragma unroll
    for (int l = 0; l < 6; ++l) s = s + p.Minv[36 * v + 6 * k + l] * vec[6 * v + l];
    return s;
}

static __global__ __launch_bounds__(BA_T) void k_ba_sx_cam(BaP p, const double* __restrict__ x, double* __restrict__ out) {
    if (ba_off(p.st)) return;
    for (int idx = threadIdx.x; idx < 6 * p.V; idx += BA_T) out[idx] = ba_sx_entry(p, x, p.Wt, idx);
}

// x = 0, r = b (bsrc), z = Minv r, p = z, rho = rho0 = the tree of r z; done at once unless rho0 is finite and > 0
static __global__ __launch_bounds__(BA_T) void k_ba_cg_init(BaP p, const double* __restrict__ bsrc, int reset_total) {
    __shared__ double sh[BA_T];
    if (ba_off(p.st)) return;
    const int t = threadIdx.x, n6 = 6 * (int)p.V;
    double a[BA_ITEMS];
#pragma unroll
    for (int q = 0; q < BA_ITEMS; ++q) {
        const int idx = t * BA_ITEMS + q;
        if (idx < n6) {
            p.x[idx] = 0.0;
            p.r[idx] = p.Minv[36 * (idx / 6)] != 0.0 ? bsrc[idx] : 0.0;
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < BA_ITEMS; ++q) {
        const int idx = t * BA_ITEMS + q;
        a[q] = 0.0;
        if (idx < n6) {
            const double z = ba_minv_entry(p, p.r, idx);
            p.z[idx] = z;
            p.p[idx] = z;
            a[q] = p.r[idx] * z;
        }
    }
    const double rho = mv_tree_chunk(a, sh);
    if (t == 0) {
        ba_put(p.st, BA_ST_RHO, rho);
        ba_put(p.st, BA_ST_RHO0, rho);
        if (reset_total) p.st[MVSDF_BA_H_CG] = 0;
        p.st[BA_ST_CGDONE] = (rho > 0.0 && isfinite(rho)) ? 0 : 1;
    }
}

static __global__ __launch_bounds__(BA_T) void k_ba_cg_update(BaP p, double tol2) {
    __shared__ double sh[BA_T];
    if (ba_off(p.st) || p.st[BA_ST_CGDONE]) return;
    const int t = threadIdx.x, n6 = 6 * (int)p.V;
    const double rho = ba_get(p.st, BA_ST_RHO), rho0 = ba_get(p.st, BA_ST_RHO0);
    double a[BA_ITEMS], qv[BA_ITEMS];
#pragma unroll
    for (int q = 0; q < BA_ITEMS; ++q) {
        const int idx = t * BA_ITEMS + q;
        a[q] = 0.0;
        qv[q] = 0.0;
        if (idx < n6) {
            qv[q] = ba_sx_entry(p, p.p, p.Wt, idx);
            a[q] = p.p[idx] * qv[q];
        }
    }
    const double sigma = mv_tree_chunk(a, sh);
    if (!(sigma > 0.0) || !isfinite(sigma)) {
        if (t == 0) p.st[BA_ST_CGDONE] = 1;
        return;
    }
    const double alpha = rho / sigma;
#pragma unroll
    for (int q = 0; q < BA_ITEMS; ++q) {
        const int idx = t * BA_ITEMS + q;
        if (idx < n6) {
            p.x[idx] = p.x[idx] + alpha * p.p[idx];
            p.r[idx] = p.r[idx] - alpha * qv[q];
        }
    }
    __syncthreads();
    double zv[BA_ITEMS];
#pragma unroll
    for (int q = 0; q < BA_ITEMS; ++q) {
        const int idx = t * BA_ITEMS + q;
        a[q] = 0.0;
        zv[q] = 0.0;
        if (idx < n6) {
            zv[q] = ba_minv_entry(p, p.r, idx);
            a[q] = p.r[idx] * zv[q];
        }
    }
    const double rhon = mv_tree_chunk(a, sh), beta = rhon / rho;
#pragma unroll
    for (int q = 0; q < BA_ITEMS; ++q) {
        const int idx = t * BA_ITEMS + q;
        if (idx < n6) p.p[idx] = zv[q] + beta * p.p[idx];
    }
    if (t == 0) {
        ba_put(p.st, BA_ST_RHO, rhon);
        p.st[MVSDF_BA_H_CG] += 1;
        p.st[BA_ST_CGDONE] = rhon > tol2 * rho0 ? 0 : 1;
    }
}

// the step's acceptance, one lane
static __global__ void k_ba_accept(long long* st, double lmin, double lmax, double ftol) {
    if (threadIdx.x != 0 || ba_off(st)) return;
    const double cost = ba_get(st, MVSDF_BA_H_COST), trial = ba_get(st, BA_ST_TRIAL), lam = ba_get(st, MVSDF_BA_H_LAMBDA);
    st[MVSDF_BA_H_ITER] += 1;
    if (!st[BA_ST_THETA] && isfinite(trial) && trial < cost) {
        st[BA_ST_CUR] ^= 1;
        st[MVSDF_BA_H_ACCEPTED] += 1;
        ba_put(st, MVSDF_BA_H_COST, trial);
        ba_put(st, MVSDF_BA_H_LAMBDA, fmax(lam / 10.0, lmin));
        if (cost - trial < ftol * cost) st[BA_ST_STOP] = 1;
    } else {
        ba_put(st, MVSDF_BA_H_LAMBDA, fmin(lam * 10.0, lmax));
    }
    st[BA_ST_THETA] = 0;
}

static __global__ void k_ba_copy_word(long long* st, int dst, int src) {
    if (threadIdx.x == 0) st[dst] = st[src];
}

// mvsdf_ba_step's report: MVSDF_BA_H_ITER = 1 where a rotation went beyond the bound
static __global__ void k_ba_theta_word(long long* st) {
    if (threadIdx.x == 0) {
        st[MVSDF_BA_H_ITER] = st[BA_ST_THETA];
        st[BA_ST_THETA] = 0;
    }
}

// the parameters of buffer cur ^ which -> the caller's arrays (also after convergence; not with an error bit set)
static __global__ __launch_bounds__(BA_T) void k_ba_export(BaP p, int which, double* __restrict__ pose, double* __restrict__ xyz) {
    const long long i = (long long)blockIdx.x * BA_T + threadIdx.x;
    if (p.st[MVSDF_BA_H_ERR] != 0) return;
    const int buf = (int)(p.st[BA_ST_CUR] & 1) ^ which;
    if (i < 12 * p.V) pose[i] = p.pose[buf][i];
    if (i < 3 * p.P) xyz[i] = p.X[buf][i];
}

// mvsdf_ba_blocks' outputs in the caller's layouts
static __global__ __launch_bounds__(BA_T) void k_ba_export_blocks(BaP p, double* __restrict__ U, double* __restrict__ gc, double* __restrict__ Vb,
                                                                  double* __restrict__ gp, double* __restrict__ bvec) {
    const long long i = (long long)blockIdx.x * BA_T + threadIdx.x;
    if (p.st[MVSDF_BA_H_ERR] != 0) return;
    if (i < p.V) {
        for (int k = 0; k < 6; ++k) {
            for (int l = 0; l < 6; ++l) U[36 * i + 6 * k + l] = p.Ug[BA_UG * i + ba_sym(k, l)];
            gc[6 * i + k] = p.Ug[BA_UG * i + 21 + k];
            bvec[6 * i + k] = p.b[6 * i + k];
        }
    }
    if (i < p.P) {
        for (int k = 0; k < 3; ++k) {
            for (int l = 0; l < 3; ++l) Vb[9 * i + 3 * k + l] = p.Vraw[(k <= l ? (k == 0 ? l : k + l + 1) : (l == 0 ? k : k + l + 1)) * p.P + i];
            gp[3 * i + k] = p.gp[k * p.P + i];
        }
    }
}

// ================================================================ the host side ================================================================
struct BaLayout {
    ChSortLayout S;
    size_t k0, k1, v0, v1, total;
    BaP p;                                            // offsets as pointers from a null base until ba_bind
};

static bool ba_layout(long long V, long long P, long long nnz, char* w, BaLayout* L) {
    if (V < 1 || V > MVSDF_BA_MAX_VIEWS || P < 1 || P > INT_MAX || nnz < 1 || nnz > MVSDF_BA_MAX_OBS) return false;
    WsCursor c{0};
    BaP& p = L->p;
    p.V = V;
    p.P = P;
    p.nnz = nnz;
    auto f64 = [&](size_t count) { return (double*)(w + c.take(count * 8)); };
    p.st = (long long*)(w + c.take(BA_HDR));
    for (int q = 0; q < 2; ++q) {
        p.pose[q] = f64((size_t)V * 12);
        p.X[q] = f64((size_t)P * 3);
    }
    p.intr = f64((size_t)V * 5);
    p.toff = (long long*)(w + c.take((size_t)(P + 1) * 8));
    p.fixed = (unsigned char*)(w + c.take((size_t)V));
    p.tview = (int*)(w + c.take((size_t)nnz * 4));
    p.obs = nullptr;                                  // the caller's, where a call linearises
    p.owner = (int*)(w + c.take((size_t)nnz * 4));
    p.pos = (int*)(w + c.take((size_t)nnz * 4));
    p.voff = (long long*)(w + c.take((size_t)(V + 1) * 8));
    p.A = f64((size_t)nnz * 12);
    p.B = f64((size_t)nnz * 6);
    p.rw = f64((size_t)nnz * 2);
    p.cterm = f64((size_t)nnz);
    p.T = f64((size_t)nnz * BA_UG);
    p.part = f64((size_t)mv_ceil_div(nnz, BA_CHUNK));
    p.Vraw = f64((size_t)P * 6);
    p.Vinv = f64((size_t)P * 6);
    p.gp = f64((size_t)P * 3);
    p.Ug = f64((size_t)V * BA_UG);
    p.Wt = f64((size_t)V * 6);
    p.Ud = f64((size_t)V * 36);
    p.Minv = f64((size_t)V * 36);
    p.b = f64((size_t)V * 6);
    p.x = f64((size_t)V * 6);
    p.r = f64((size_t)V * 6);
    p.z = f64((size_t)V * 6);
    p.p = f64((size_t)V * 6);
    L->k0 = c.take((size_t)nnz * 8);
    L->k1 = c.take((size_t)nnz * 8);
    L->v0 = c.take((size_t)nnz * 4);
    L->v1 = c.take((size_t)nnz * 4);
    ch_sort_layout(nnz, 0, c, &L->S);
    L->total = c.o;
    return true;
}

// the header of a call that stops at its argument checks (then a wait: nothing else is enqueued)
static int ba_refuse(char* w, long long err, hipStream_t s, const char* what) {
    long long h[MVSDF_BA_H_WORDS] = {};
    h[MVSDF_BA_H_ERR] = err;
    return mv_write_header(w, h, MVSDF_BA_H_WORDS, s, what);
}

// the fresh state of an accepted call
static __global__ void k_ba_state(long long* st, double lambda, long long nnz) {
    if (threadIdx.x != 0) return;
    ba_put(st, MVSDF_BA_H_LAMBDA, lambda);
    st[BA_ST_SEG + 1] = nnz;
    st[BA_ST_SEG + 3] = (nnz + BA_CHUNK - 1) / BA_CHUNK;
}

static int ba_state(char* w, double lambda, long long nnz, hipStream_t s, const char* what) {
    if (int rc = mv_check(hipMemsetAsync(w, 0, BA_HDR, s), what)) return rc;
    hipLaunchKernelGGL(k_ba_state, dim3(1), dim3(64), 0, s, (long long*)w, lambda, nnz);
    return 0;
}

static unsigned ba_views_grid(const BaP& p) { return (unsigned)mv_ceil_div(p.V, 64); }

// the cost of the parameters in buffer cur ^ which -> state word `word`
static void ba_cost(const BaP& p, int which, int trial, double delta, double* r, double* terms, int word, hipStream_t s) {
    hipLaunchKernelGGL(k_ba_cost, dim3(mv_grid(p.nnz, BA_T)), dim3(BA_T), 0, s, p, which, trial, 0, delta, r, terms);
    const long long nc = mv_ceil_div(p.nnz, BA_CHUNK);
    hipLaunchKernelGGL(k_ba_chunk_tree, dim3((unsigned)nc), dim3(BA_T), 0, s, (const double*)terms, p.nnz, p.part, (const long long*)p.st);
    hipLaunchKernelGGL(k_ba_seg_tree, dim3(1, 1), dim3(BA_T), 0, s, (const double*)p.part, 0LL, (const long long*)(p.st + BA_ST_SEG + 2),
                       (double*)(p.st + word), (const long long*)p.st, 0);
}

// the inputs into the workspace, the checks, the owners, the view order, the initial cost
static int ba_begin(const BaLayout& L, char* w, const double* pose, const double* intr, const double* xyz, const int64_t* track_off,
                    const int32_t* track_view, const double* obs, const uint8_t* fixed, double lambda, double delta, int trial, double* r, double* terms,
                    hipStream_t s, const char* what) {
    const BaP& p = L.p;
    int rc;
    if ((rc = ba_state(w, lambda, p.nnz, s, what))) return rc;
    if ((rc = mv_check(hipMemcpyAsync(p.pose[0], pose, (size_t)p.V * 96, hipMemcpyDeviceToDevice, s), what))) return rc;
    if ((rc = mv_check(hipMemcpyAsync(p.X[0], xyz, (size_t)p.P * 24, hipMemcpyDeviceToDevice, s), what))) return rc;
    if ((rc = mv_check(hipMemcpyAsync(p.intr, intr, (size_t)p.V * 40, hipMemcpyDeviceToDevice, s), what))) return rc;
    if ((rc = mv_check(hipMemcpyAsync(p.toff, track_off, (size_t)(p.P + 1) * 8, hipMemcpyDeviceToDevice, s), what))) return rc;
    if ((rc = mv_check(hipMemcpyAsync(p.tview, track_view, (size_t)p.nnz * 4, hipMemcpyDeviceToDevice, s), what))) return rc;
    if (fixed) {
        if ((rc = mv_check(hipMemcpyAsync(p.fixed, fixed, (size_t)p.V, hipMemcpyDeviceToDevice, s), what))) return rc;
    } else if ((rc = mv_check(hipMemsetAsync(p.fixed, 0, (size_t)p.V, s), what))) {
        return rc;
    }
    unsigned long long* err = (unsigned long long*)p.st + MVSDF_BA_H_ERR;
    const unsigned long long bit = MVSDF_PS_ERR_FINITE;
    hipLaunchKernelGGL(k_any_nonfinite<double>, dim3(1), dim3(MV_THREADS), 0, s, pose, p.V * 12, err, bit);
    hipLaunchKernelGGL(k_any_nonfinite<double>, dim3(1), dim3(MV_THREADS), 0, s, intr, p.V * 5, err, bit);
    hipLaunchKernelGGL(k_any_nonfinite<double>, dim3(64), dim3(MV_THREADS), 0, s, xyz, p.P * 3, err, bit);
    hipLaunchKernelGGL(k_any_nonfinite<double>, dim3(64), dim3(MV_THREADS), 0, s, obs, p.nnz * 2, err, bit);
    const long long most = p.P > p.nnz ? p.P : p.nnz;
    hipLaunchKernelGGL(k_ba_check, dim3(mv_grid(most, BA_T)), dim3(BA_T), 0, s, (const long long*)track_off, (const int*)track_view, p.V, p.P, p.nnz, p.st);
    unsigned long long* k[2] = {(unsigned long long*)(w + L.k0), (unsigned long long*)(w + L.k1)};
    int* v[2] = {(int*)(w + L.v0), (int*)(w + L.v1)};
    if ((rc = mv_check(hipMemsetAsync(k[0], 0, (size_t)p.nnz * 8, s), what))) return rc;
    if ((rc = mv_check(hipMemsetAsync(v[0], 0, (size_t)p.nnz * 4, s), what))) return rc;
    hipLaunchKernelGGL(k_ba_owner, dim3(mv_grid(p.P, BA_T)), dim3(BA_T), 0, s, p, k[0], v[0]);
    int bits = 1;
    while ((1LL << bits) < p.V) ++bits;
    const int cur = ch_radix_sort(k, v, p.nnz, bits, w, L.S, s);
    hipLaunchKernelGGL(k_ba_segments, dim3(mv_grid(p.nnz + 1, BA_T)), dim3(BA_T), 0, s, p, (const unsigned long long*)k[cur], (const int*)v[cur]);
    ba_cost(p, 0, trial, delta, r, terms, MVSDF_BA_H_COST, s);
    hipLaunchKernelGGL(k_ba_copy_word, dim3(1), dim3(64), 0, s, p.st, (int)MVSDF_BA_H_COST0, (int)MVSDF_BA_H_COST);
    return 0;
}

// the linearisation at the current parameters and lambda: U, g_c, the point blocks, the camera blocks, the right-hand side
static void ba_linearise(const BaP& p, double delta, double floor_diag, hipStream_t s) {
    hipLaunchKernelGGL(k_ba_lin, dim3(mv_grid(p.nnz, BA_T)), dim3(BA_T), 0, s, p, delta);
    hipLaunchKernelGGL(k_ba_seg_tree, dim3((unsigned)p.V, BA_UG), dim3(BA_T), 0, s, (const double*)p.T, p.nnz, (const long long*)p.voff, p.Ug,
                       (const long long*)p.st, 0);
    hipLaunchKernelGGL(k_ba_point, dim3(mv_grid(p.P, BA_T)), dim3(BA_T), 0, s, p, floor_diag);
    hipLaunchKernelGGL(k_ba_seg_tree, dim3((unsigned)p.V, 6), dim3(BA_T), 0, s, (const double*)p.T, p.nnz, (const long long*)p.voff, p.Wt,
                       (const long long*)p.st, 0);
    hipLaunchKernelGGL(k_ba_cam, dim3(ba_views_grid(p)), dim3(64), 0, s, p, floor_diag);
}

// the tree sums of W y for the vector x: p.Wt
static void ba_wy(const BaP& p, const double* x, int cg, hipStream_t s) {
    hipLaunchKernelGGL(k_ba_sx_point, dim3(mv_grid(p.P, BA_T)), dim3(BA_T), 0, s, p, x, cg);
    hipLaunchKernelGGL(k_ba_seg_tree, dim3((unsigned)p.V, 6), dim3(BA_T), 0, s, (const double*)p.T, p.nnz, (const long long*)p.voff, p.Wt,
                       (const long long*)p.st, cg);
}

static void ba_solve(const BaP& p, const double* b, int cg_iters, double cg_tol, int reset_total, hipStream_t s) {
    hipLaunchKernelGGL(k_ba_cg_init, dim3(1), dim3(BA_T), 0, s, p, b, reset_total);
    for (int it = 0; it < cg_iters; ++it) {
        ba_wy(p, p.p, 1, s);
        hipLaunchKernelGGL(k_ba_cg_update, dim3(1), dim3(BA_T), 0, s, p, cg_tol * cg_tol);
    }
}

static void ba_step(const BaP& p, const double* x, const double* rod, hipStream_t s) {
    hipLaunchKernelGGL(k_ba_step_point, dim3(mv_grid(p.P, BA_T)), dim3(BA_T), 0, s, p, x);
    hipLaunchKernelGGL(k_ba_step_cam, dim3(ba_views_grid(p)), dim3(64), 0, s, p, x, rod);
}

extern "C" {

size_t mvsdf_ba_workspace_bytes(int64_t V, int64_t P, int64_t nnz) {
    BaLayout L;
    return ba_layout(V, P, nnz, nullptr, &L) ? L.total : 0;
}

#define BA_ENTER(what_, need_)                                                                                         \
    const char* what = what_;                                                                                          \
    if (!(need_) || !ws || ws_bytes < BA_HDR) return mv_fail(-1, what_ ": bad arguments");                             \
    hipStream_t s = (hipStream_t)stream;                                                                               \
    char* w = (char*)ws;                                                                                               \
    BaLayout L;                                                                                                        \
    if (!ba_layout(V, P, nnz, w, &L)) return ba_refuse(w, MVSDF_PS_ERR_SHAPE, s, what);                               \
    if (ws_bytes < L.total) return mv_fail(-1, what_ ": the workspace is too small");                                  \
    BaP& p = L.p;                                                                                                      \
    (void)p

int mvsdf_ba_residuals(const double* pose, const double* intr, const double* xyz, const int64_t* track_off, const int32_t* track_view, const double* obs,
                       int64_t V, int64_t P, int64_t nnz, double loss_scale, int32_t trial, void* ws, size_t ws_bytes, double* r, double* terms,
                       void* stream) {
    BA_ENTER("mvsdf_ba_residuals", pose && intr && xyz && track_off && track_view && obs && r && terms && loss_scale > 0);
    p.obs = obs;
    if (int rc = ba_begin(L, w, pose, intr, xyz, track_off, track_view, obs, nullptr, 0.0, loss_scale, trial, r, terms, s, what)) return rc;
    return mv_check(hipGetLastError(), what);
}

int mvsdf_ba_blocks(const double* pose, const double* intr, const double* xyz, const int64_t* track_off, const int32_t* track_view, const double* obs,
                    const uint8_t* fixed, int64_t V, int64_t P, int64_t nnz, double loss_scale, double lambda, double floor_diag, void* ws,
                    size_t ws_bytes, double* U, double* gc, double* Vb, double* gp, double* bvec, void* stream) {
    BA_ENTER("mvsdf_ba_blocks", pose && intr && xyz && track_off && track_view && obs && fixed && U && gc && Vb && gp && bvec && loss_scale > 0 &&
                                    lambda >= 0 && floor_diag > 0);
    p.obs = obs;
    if (int rc = ba_begin(L, w, pose, intr, xyz, track_off, track_view, obs, fixed, lambda, loss_scale, 0, nullptr, p.cterm, s, what)) return rc;
    ba_linearise(p, loss_scale, floor_diag, s);
    const long long most = p.P > p.V ? p.P : p.V;
    hipLaunchKernelGGL(k_ba_export_blocks, dim3(mv_grid(most, BA_T)), dim3(BA_T), 0, s, p, U, gc, Vb, gp, bvec);
    return mv_check(hipGetLastError(), what);
}

int mvsdf_ba_schur(int64_t V, int64_t P, int64_t nnz, void* ws, size_t ws_bytes, const double* x, double* out, void* stream) {
    BA_ENTER("mvsdf_ba_schur", x && out);
    ba_wy(p, x, 0, s);
    hipLaunchKernelGGL(k_ba_sx_cam, dim3(1), dim3(BA_T), 0, s, p, x, out);
    return mv_check(hipGetLastError(), what);
}

int mvsdf_ba_solve(int64_t V, int64_t P, int64_t nnz, const double* b, int32_t cg_iters, double cg_tol, void* ws, size_t ws_bytes, double* x,
                   void* stream) {
    BA_ENTER("mvsdf_ba_solve", x && cg_iters >= 0 && cg_iters <= MVSDF_BA_MAX_CG && cg_tol >= 0);
    ba_solve(p, b ? b : p.b, cg_iters, cg_tol, 1, s);
    if (int rc = mv_check(hipMemcpyAsync(x, p.x, (size_t)V * 48, hipMemcpyDeviceToDevice, s), what)) return rc;
    return mv_check(hipGetLastError(), what);
}

int mvsdf_ba_step(int64_t V, int64_t P, int64_t nnz, const double* rod, void* ws, size_t ws_bytes, const double* x, double* pose_out,
                  double* xyz_out, void* stream) {
    BA_ENTER("mvsdf_ba_step", rod && x && pose_out && xyz_out);
    ba_step(p, x, rod, s);
    const long long most = 3 * p.P > 12 * p.V ? 3 * p.P : 12 * p.V;
    hipLaunchKernelGGL(k_ba_export, dim3(mv_grid(most, BA_T)), dim3(BA_T), 0, s, p, 1, pose_out, xyz_out);
    hipLaunchKernelGGL(k_ba_theta_word, dim3(1), dim3(64), 0, s, p.st);
    return mv_check(hipGetLastError(), what);
}

int mvsdf_ba_adjust(const double* pose, const double* intr, const double* xyz, const int64_t* track_off, const int32_t* track_view, const double* obs,
                    const uint8_t* fixed, int64_t V, int64_t P, int64_t nnz, const double* rod, double loss_scale, int32_t iterations, double lambda0,
                    double lambda_min, double lambda_max, double floor_diag, int32_t cg_iters, double cg_tol, double ftol, void* ws, size_t ws_bytes,
                    double* pose_out, double* xyz_out, double* r, double* terms, void* stream) {
    BA_ENTER("mvsdf_ba_adjust", pose && intr && xyz && track_off && track_view && obs && fixed && rod && pose_out && xyz_out && r && terms &&
                                    loss_scale > 0 && iterations >= 0 && iterations <= MVSDF_BA_MAX_ITERATIONS && lambda_min > 0 &&
                                    lambda0 >= lambda_min && lambda_max >= lambda0 && isfinite(lambda_max) && floor_diag > 0 && cg_iters >= 0 &&
                                    cg_iters <= MVSDF_BA_MAX_CG && cg_tol >= 0 && ftol >= 0);
    p.obs = obs;
    if (int rc = ba_begin(L, w, pose, intr, xyz, track_off, track_view, obs, fixed, lambda0, loss_scale, 0, nullptr, p.cterm, s, what)) return rc;
    for (int it = 0; it < iterations; ++it) {
        ba_linearise(p, loss_scale, floor_diag, s);
        ba_solve(p, p.b, cg_iters, cg_tol, 0, s);
        ba_step(p, p.x, rod, s);
        ba_cost(p, 1, 1, loss_scale, nullptr, p.cterm, BA_ST_TRIAL, s);
        hipLaunchKernelGGL(k_ba_accept, dim3(1), dim3(64), 0, s, p.st, lambda_min, lambda_max, ftol);
    }
    const long long most = 3 * p.P > 12 * p.V ? 3 * p.P : 12 * p.V;
    hipLaunchKernelGGL(k_ba_export, dim3(mv_grid(most, BA_T)), dim3(BA_T), 0, s, p, 0, pose_out, xyz_out);
    hipLaunchKernelGGL(k_ba_cost, dim3(mv_grid(p.nnz, BA_T)), dim3(BA_T), 0, s, p, 0, 1, 1, loss_scale, r, terms);
    return mv_check(hipGetLastError(), what);
}

}  // extern "C"
