// poisson.hip -- on-device Poisson surface reconstruction of an oriented cloud on a regular grid of N = 2^depth + 1 lattice points per axis.  Python:
// mvsdf_amd/poisson.py, which states the definition; tests/poisson_ref.py restates it in numpy.  The level set is meshed by mesh.marching_cubes_masked.
// All arithmetic is fp64 without contraction, in the order the definition writes it; no float atomics anywhere.
//
// * k_po_splat: one lane per point; the trilinear weights times the normal, quantised to int64 multiples of 2^-32 (viewsel.hip's trick), go into four
//   int64 volumes with 64-bit integer atomics, so the sums cannot depend on the schedule.  k_po_rhs turns them into the fp64 density and the divergence b.
// * the solve: a fixed number of V-cycles made of stencil passes only, one launch per pass and level.  A workgroup is 64 lattice points along k (a wave
//   reads contiguous 512-byte runs) by 4 along j; blockIdx.z is i.  k_po_smooth is one colour of a red-black Gauss-Seidel sweep in place (a lane of the
//   colour reads six neighbours of the other colour, so a pass has no race), k_po_resid the residual (and, for the diagnostics, its largest magnitude
//   by an integer atomic max over the bit patterns), k_po_restrict the separable full weighting z, y, x evaluated per coarse point, k_po_prolong the
//   separable trilinear interpolation x, y, z evaluated per fine point and added, k_po_direct the 3^3 level.  The levels that would fit one workgroup's
//   LDS are not fused: every level is a launch of its own.
// * the isovalue: k_po_values interpolates chi at every admitted point into a compacted array (an int64 scan of the admission flags, geom_prims.h),
//   k_po_tree sums it over the canonical pairwise tree: a workgroup reduces an aligned chunk of 2048 in adjacent-pair order, the levels above repeat it.
// * k_po_valid0 / k_po_dilate / k_po_volume: the trimming mask and the fp32 volume chi - iso that the extractor reads.
//
// Every argument is validated on the host before anything is launched: an error leaves {0, error bits} in the header.  A non-finite coordinate or normal
// is found on the device (k_any_nonfinite) and comes back as an error bit too; the passes after it stay inside their arrays whatever the values are.
#include "geom_prims.h"

#define PO_HDR 256                                    // bytes at the start of the workspace: MVSDF_PO_H_*
static_assert(MVSDF_PO_H_WORDS * 8 <= PO_HDR && MVSDF_PO_H_ERR == MVSDF_RES_H_ERR, "the result words fit the header; mv_refuse_header writes its error word");
#define PO_BK 64                                      // the workgroup of the stencil passes: PO_BK lattice points along k, PO_BJ along j
#define PO_BJ 4
#define PO_THREADS (PO_BK * PO_BJ)
#define PO_TREE_ITEMS 8
#define PO_TREE (PO_THREADS * PO_TREE_ITEMS)          // the chunk of the tree sum: a power of two
#define PO_SCALE 4294967296.0                         // 2^32
#define PO_UNSCALE (1.0 / 4294967296.0)
static_assert((PO_TREE & (PO_TREE - 1)) == 0 && (PO_THREADS & (PO_THREADS - 1)) == 0, "the tree sum needs power-of-two chunks");

enum { PO_STAGE_SPLAT = 1, PO_STAGE_SOLVE = 2, PO_STAGE_ISO = 4 };

typedef unsigned long long po_u64;

struct PoLayout {
    size_t vq[4], b0, lx[MVSDF_PO_MAX_DEPTH], lb[MVSDF_PO_MAX_DEPTH], flags, off, scan, tree[2], total;
    long long N, vol;
};

static inline long long po_side(int depth, int level) { return (1ll << (depth - level)) + 1; }

static bool po_layout(long long n, int depth, PoLayout* L) {
    if (depth < MVSDF_PO_MIN_DEPTH || depth > MVSDF_PO_MAX_DEPTH || n < 1 || n > INT_MAX) return false;
    L->N = po_side(depth, 0);
    L->vol = L->N * L->N * L->N;
    WsCursor c{PO_HDR};
    for (int a = 0; a < 4; ++a) L->vq[a] = c.take((size_t)L->vol * 8);      // V_x (later the residual of the level at work), V_y, V_z, density
    L->b0 = c.take((size_t)L->vol * 8);
    for (int l = 1; l < depth; ++l) {
        const long long m = po_side(depth, l);
        L->lx[l] = c.take((size_t)(m * m * m) * 8);
        L->lb[l] = c.take((size_t)(m * m * m) * 8);
    }
    L->flags = c.take((size_t)n);
    L->off = c.take((size_t)n * 8);
    L->scan = c.take(mv_scan_tmp_bytes(n));
    L->tree[0] = c.take((size_t)mv_ceil_div(n, PO_TREE) * 8);
    L->tree[1] = c.take((size_t)mv_ceil_div(n, PO_TREE) * 8);
    L->total = c.o;
    return true;
}

struct PoGrid {
    double org[3], h;
    int N;
};

// g = (p - origin) / h, i0 = floor(g), f = g - i0; admitted iff 1 <= i0 <= N - 3 on every axis (a NaN fails the compare)
__device__ __forceinline__ bool po_cell(const double* __restrict__ p, const PoGrid& g, int* i0, double* f) {
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double q = (p[a] - g.org[a]) / g.h;
        const double fl = floor(q);
        const bool in = fl >= 1.0 && fl <= (double)(g.N - 3);
        ok = ok && in;
        i0[a] = in ? (int)fl : 1;
        f[a] = q - fl;
    }
    return ok;
}

// the weight of corner (dx, dy, dz): the factors in x, y, z order
__device__ __forceinline__ double po_weight(const double* f, int dx, int dy, int dz) {
    return ((dx ? f[0] : 1.0 - f[0]) * (dy ? f[1] : 1.0 - f[1])) * (dz ? f[2] : 1.0 - f[2]);
}

__device__ __forceinline__ long long po_quantise(double v) { return (long long)rint(v * PO_SCALE); }

__global__ __launch_bounds__(PO_THREADS) void k_po_splat(const double* __restrict__ points, const double* __restrict__ normals, long long n, PoGrid g,
                                                          po_u64* __restrict__ vx, po_u64* __restrict__ vy, po_u64* __restrict__ vz, po_u64* __restrict__ vd,
                                                          unsigned char* __restrict__ flags) {
    const long long i = (long long)blockIdx.x * PO_THREADS + threadIdx.x;
    if (i >= n) return;
    int i0[3];
    double f[3];
    const bool ok = po_cell(points + i * 3, g, i0, f);
    flags[i] = ok ? 1 : 0;
    if (!ok) return;
    const double n0 = normals[i * 3], n1 = normals[i * 3 + 1], n2 = normals[i * 3 + 2];
    for (int dx = 0; dx < 2; ++dx)
        for (int dy = 0; dy < 2; ++dy)
            for (int dz = 0; dz < 2; ++dz) {
                const double w = po_weight(f, dx, dy, dz);
                const long long at = ((long long)(i0[0] + dx) * g.N + (i0[1] + dy)) * g.N + (i0[2] + dz);
                const long long q0 = po_quantise(w * n0), q1 = po_quantise(w * n1), q2 = po_quantise(w * n2), qd = po_quantise(w);
                if (q0) atomicAdd(vx + at, (po_u64)q0);
                if (q1) atomicAdd(vy + at, (po_u64)q1);
                if (q2) atomicAdd(vz + at, (po_u64)q2);
                if (qd) atomicAdd(vd + at, (po_u64)qd);
            }
}

// the lattice point of a lane of the stencil passes; false beyond the grid
__device__ __forceinline__ bool po_point(int N, int* i, int* j, int* k) {
    *k = blockIdx.x * PO_BK + threadIdx.x;
    *j = blockIdx.y * PO_BJ + threadIdx.y;
    *i = blockIdx.z;
    return *k < N && *j < N && *i < N;
}

__device__ __forceinline__ bool po_interior(int N, int i, int j, int k) { return i >= 1 && i <= N - 2 && j >= 1 && j <= N - 2 && k >= 1 && k <= N - 2; }

__device__ __forceinline__ double po_field(const long long* __restrict__ v, long long at) { return (double)v[at] * PO_UNSCALE; }

// density and the right-hand side from the int64 volumes
__global__ __launch_bounds__(PO_THREADS) void k_po_rhs(const long long* __restrict__ vx, const long long* __restrict__ vy, const long long* __restrict__ vz,
                                                        const long long* __restrict__ vd, int N, double twoh, double* __restrict__ b,
                                                        double* __restrict__ density) {
    int i, j, k;
    if (!po_point(N, &i, &j, &k)) return;
    const long long sj = N, si = (long long)N * N, at = (long long)i * si + (long long)j * sj + k;
    density[at] = po_field(vd, at);
    double r = 0.0;
    if (po_interior(N, i, j, k))
        r = (((po_field(vx, at + si) - po_field(vx, at - si)) + (po_field(vy, at + sj) - po_field(vy, at - sj))) + (po_field(vz, at + 1) - po_field(vz, at - 1))) / twoh;
    b[at] = r;
}

// the neighbour sum of the smoother and the residual
__device__ __forceinline__ double po_sum6(const double* x, long long at, long long si, long long sj) {
    return ((((x[at - si] + x[at + si]) + x[at - sj]) + x[at + sj]) + x[at - 1]) + x[at + 1];
}

// one colour of a red-black Gauss-Seidel sweep, in place
__global__ __launch_bounds__(PO_THREADS) void k_po_smooth(double* x, const double* __restrict__ b, int N, double h2, int colour) {
    int i, j, k;
    if (!po_point(N, &i, &j, &k) || !po_interior(N, i, j, k) || ((i + j + k) & 1) != colour) return;
    const long long sj = N, si = (long long)N * N, at = (long long)i * si + (long long)j * sj + k;
    x[at] = (po_sum6(x, at, si, sj) - h2 * b[at]) / 6.0;
}

// r = b - (S - 6 x) / h^2 at the interior points into r (or nowhere); with word, the largest |r| as an integer max over the bit patterns
__global__ __launch_bounds__(PO_THREADS) void k_po_resid(const double* __restrict__ x, const double* __restrict__ b, int N, double h2, double* __restrict__ r,
                                                          po_u64* __restrict__ word) {
    __shared__ po_u64 sh[PO_THREADS];
    int i, j, k;
    double v = 0.0;
    if (po_point(N, &i, &j, &k) && po_interior(N, i, j, k)) {
        const long long sj = N, si = (long long)N * N, at = (long long)i * si + (long long)j * sj + k;
        v = b[at] - (po_sum6(x, at, si, sj) - 6.0 * x[at]) / h2;
        if (r) r[at] = v;
    }
    if (!word) return;                                            // uniform over the launch
    const int t = threadIdx.y * PO_BK + threadIdx.x;
    sh[t] = (po_u64)__double_as_longlong(fabs(v));
    __syncthreads();
    for (int d = PO_THREADS / 2; d; d >>= 1) {
        if (t < d) sh[t] = sh[t] > sh[t + d] ? sh[t] : sh[t + d];
        __syncthreads();
    }
    if (t == 0 && sh[0]) atomicMax(word, sh[0]);
}

// full weighting, separable: z, then y, then x; the coarse boundary is 0.  One lane per coarse point (Nc = (N - 1) / 2 + 1).
__global__ __launch_bounds__(PO_THREADS) void k_po_restrict(const double* __restrict__ r, int N, double* __restrict__ bc, int Nc) {
    int I, J, K;
    if (!po_point(Nc, &I, &J, &K)) return;
    const long long out = ((long long)I * Nc + J) * Nc + K;
    if (!po_interior(Nc, I, J, K)) {
        bc[out] = 0.0;
        return;
    }
    double c[3];
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
        double a[3];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const double* __restrict__ q = r + ((long long)(2 * I - 1 + dx) * N + (2 * J - 1 + dy)) * N + 2 * K;
            a[dy] = (0.25 * q[-1] + 0.5 * q[0]) + 0.25 * q[1];
        }
        c[dx] = (0.25 * a[0] + 0.5 * a[1]) + 0.25 * a[2];
    }
    bc[out] = (0.25 * c[0] + 0.5 * c[1]) + 0.25 * c[2];
}

// trilinear prolongation, separable: x, then y, then z (an even index copies, an odd one takes 0.5 (a[I] + a[I + 1])), added to x at the interior points
__global__ __launch_bounds__(PO_THREADS) void k_po_prolong(const double* __restrict__ e, int Nc, double* __restrict__ x, int N) {
    int i, j, k;
    if (!po_point(N, &i, &j, &k) || !po_interior(N, i, j, k)) return;
    const int I = i >> 1, J = j >> 1, K = k >> 1, ox = i & 1, oy = j & 1, oz = k & 1;
    const long long sI = (long long)Nc * Nc;
    auto along_x = [&](int dj, int dk) {
        const double* __restrict__ q = e + (long long)I * sI + (long long)(J + dj) * Nc + (K + dk);
        return ox ? 0.5 * (q[0] + q[sI]) : q[0];
    };
    auto along_y = [&](int dk) {
        const double v0 = along_x(0, dk);
        return oy ? 0.5 * (v0 + along_x(1, dk)) : v0;
    };
    const double u0 = along_y(0);
    const double w = oz ? 0.5 * (u0 + along_y(1)) : u0;
    const long long at = ((long long)i * N + j) * N + k;
    x[at] = x[at] + w;
}

// the 3^3 level: its one interior point
__global__ void k_po_direct(double* __restrict__ x, const double* __restrict__ b, double h2) {
    if (threadIdx.x == 0 && blockIdx.x == 0) x[13] = -(h2 * b[13]) / 6.0;
}

// c_i of every admitted point into its compacted row
__global__ __launch_bounds__(PO_THREADS) void k_po_values(const double* __restrict__ points, long long n, PoGrid g, const unsigned char* __restrict__ flags,
                                                           const long long* __restrict__ off, const double* __restrict__ chi, double* __restrict__ values) {
    const long long i = (long long)blockIdx.x * PO_THREADS + threadIdx.x;
    if (i >= n || !flags[i]) return;
    int i0[3];
    double f[3];
    if (!po_cell(points + i * 3, g, i0, f)) return;
    double c = 0.0;
    for (int dx = 0; dx < 2; ++dx)
        for (int dy = 0; dy < 2; ++dy)
            for (int dz = 0; dz < 2; ++dz)
                c = c + po_weight(f, dx, dy, dz) * chi[((long long)(i0[0] + dx) * g.N + (i0[1] + dy)) * g.N + (i0[2] + dz)];
    const long long row = off[i];
    if (row >= 0 && row < n) values[row] = c;
}

// out[b] = the pairwise-tree sum of in[b * PO_TREE ...) (+0.0 beyond n), adjacent pairs first
__global__ __launch_bounds__(PO_THREADS) void k_po_tree(const double* __restrict__ in, long long n, double* __restrict__ out) {
    __shared__ double sh[PO_THREADS];
    const int t = threadIdx.x;
    const long long base = (long long)blockIdx.x * PO_TREE + (long long)t * PO_TREE_ITEMS;
    double a[PO_TREE_ITEMS];
#pragma unroll
    for (int q = 0; q < PO_TREE_ITEMS; ++q) a[q] = base + q < n ? in[base + q] : 0.0;
    static_assert(PO_THREADS == MV_THREADS && PO_TREE_ITEMS == MV_ITEMS, "k_po_tree reduces one chunk of geom_prims.h's tree");
    const double v = mv_tree_chunk(a, sh);
    if (t == 0) out[blockIdx.x] = v;
}

__global__ __launch_bounds__(PO_THREADS) void k_po_valid0(const double* __restrict__ density, long long n, double min_density, unsigned char* __restrict__ out) {
    const long long i = (long long)blockIdx.x * PO_THREADS + threadIdx.x;
    if (i < n) out[i] = density[i] > min_density ? 1 : 0;
}

// one step of the dilation over the 6-neighbourhood inside the grid
__global__ __launch_bounds__(PO_THREADS) void k_po_dilate(const unsigned char* __restrict__ in, int N, unsigned char* __restrict__ out) {
    int i, j, k;
    if (!po_point(N, &i, &j, &k)) return;
    const long long sj = N, si = (long long)N * N, at = (long long)i * si + (long long)j * sj + k;
    unsigned char v = in[at];
    if (i > 0) v |= in[at - si];
    if (i < N - 1) v |= in[at + si];
    if (j > 0) v |= in[at - sj];
    if (j < N - 1) v |= in[at + sj];
    if (k > 0) v |= in[at - 1];
    if (k < N - 1) v |= in[at + 1];
    out[at] = v ? 1 : 0;
}

__global__ __launch_bounds__(PO_THREADS) void k_po_volume(const double* __restrict__ chi, long long n, double iso, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * PO_THREADS + threadIdx.x;
    if (i < n) out[i] = (float)(chi[i] - iso);
}

static inline dim3 po_grid3(long long N) { return dim3((unsigned)mv_ceil_div(N, PO_BK), (unsigned)mv_ceil_div(N, PO_BJ), (unsigned)N); }
static inline dim3 po_block3() { return dim3(PO_BK, PO_BJ, 1); }

extern "C" {

size_t mvsdf_poisson_workspace_bytes(int64_t n, int32_t depth) {
    PoLayout L;
    return po_layout(n, depth, &L) ? L.total : 0;
}

int mvsdf_poisson_reconstruct(const double* points, const double* normals, int64_t n, const double* origin, double voxel, int32_t depth, int32_t cycles,
                              int32_t sweeps, int32_t stages, void* ws, size_t ws_bytes, double* chi, double* density, double* values, void* stream) {
    const char* what = "mvsdf_poisson_reconstruct";
    if (!points || !normals || !origin || !ws || !chi || !density || !values || ws_bytes < PO_HDR) return mv_fail(-1, "mvsdf_poisson_reconstruct: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    // ---- validation, all of it before the first launch ----
    long long err = 0;
    PoLayout L;
    if (depth < MVSDF_PO_MIN_DEPTH || depth > MVSDF_PO_MAX_DEPTH || cycles < 0 || sweeps < 1) err |= MVSDF_PO_ERR_RANGE;
    if (n < 1 || n > INT_MAX) err |= MVSDF_PO_ERR_SHAPE;
    if (!isfinite(origin[0]) || !isfinite(origin[1]) || !isfinite(origin[2]) || !isfinite(voxel)) err |= MVSDF_PO_ERR_FINITE;
    else if (!(voxel > 0.0)) err |= MVSDF_PO_ERR_RANGE;
    if (!err && !po_layout(n, depth, &L)) err |= MVSDF_PO_ERR_SHAPE;
    if (err) return mv_refuse_header(ws, err, s, what);
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_poisson_reconstruct: workspace too small (mvsdf_poisson_workspace_bytes)");
    char* w = (char*)ws;
    int rc;
    PoGrid g;
    for (int a = 0; a < 3; ++a) g.org[a] = origin[a];
    g.h = voxel;
    g.N = (int)L.N;
    const size_t volb = (size_t)L.vol * 8;
    po_u64* hdr = (po_u64*)ws;
    const unsigned pgrid = mv_grid(n, PO_THREADS);
    if (stages & PO_STAGE_SPLAT) {
        if ((rc = mv_check(hipMemsetAsync(ws, 0, PO_HDR, s), what))) return rc;
        if ((rc = mv_check(hipMemsetAsync(w + L.vq[0], 0, L.b0 - L.vq[0], s), what))) return rc;   // the four int64 volumes are one run
        const unsigned cap = pgrid < 4096u ? pgrid : 4096u;
        hipLaunchKernelGGL(k_any_nonfinite<double>, dim3(cap), dim3(MV_THREADS), 0, s, points, (long long)n * 3, hdr + MVSDF_PO_H_ERR, (po_u64)MVSDF_PO_ERR_FINITE);
        hipLaunchKernelGGL(k_any_nonfinite<double>, dim3(cap), dim3(MV_THREADS), 0, s, normals, (long long)n * 3, hdr + MVSDF_PO_H_ERR, (po_u64)MVSDF_PO_ERR_FINITE);
        hipLaunchKernelGGL(k_po_splat, dim3(pgrid), dim3(PO_THREADS), 0, s, points, normals, (long long)n, g, (po_u64*)(w + L.vq[0]), (po_u64*)(w + L.vq[1]),
                           (po_u64*)(w + L.vq[2]), (po_u64*)(w + L.vq[3]), (unsigned char*)(w + L.flags));
        hipLaunchKernelGGL(k_po_rhs, po_grid3(L.N), po_block3(), 0, s, (const long long*)(w + L.vq[0]), (const long long*)(w + L.vq[1]),
                           (const long long*)(w + L.vq[2]), (const long long*)(w + L.vq[3]), g.N, 2.0 * voxel, (double*)(w + L.b0), density);
        mv_scan((const unsigned char*)(w + L.flags), (long long)n, (long long*)(w + L.off), w + L.scan, (long long*)ws + MVSDF_PO_H_USED, s);
    }
    if (stages & PO_STAGE_SOLVE) {
        double* x[MVSDF_PO_MAX_DEPTH];
        double* b[MVSDF_PO_MAX_DEPTH];
        double h2[MVSDF_PO_MAX_DEPTH];
        long long side[MVSDF_PO_MAX_DEPTH];
        for (int l = 0; l < depth; ++l) {
            x[l] = l ? (double*)(w + L.lx[l]) : chi;
            b[l] = l ? (double*)(w + L.lb[l]) : (double*)(w + L.b0);
            side[l] = po_side(depth, l);
            const double hl = voxel * (double)(1ll << l);             // h doubled per level: exact
            h2[l] = hl * hl;
        }
        double* r = (double*)(w + L.vq[0]);                           // V_x is spent once the right-hand side exists
        if ((rc = mv_check(hipMemsetAsync(chi, 0, volb, s), what))) return rc;
        if ((rc = mv_check(hipMemsetAsync(x[depth - 1], 0, 27 * 8, s), what))) return rc;
        hipLaunchKernelGGL(k_po_resid, po_grid3(side[0]), po_block3(), 0, s, (const double*)x[0], (const double*)b[0], (int)side[0], h2[0], (double*)nullptr,
                           hdr + MVSDF_PO_H_RESIDUAL0);
        auto smooth = [&](int l) {
            for (int q = 0; q < sweeps; ++q)
                for (int colour = 0; colour < 2; ++colour)
                    hipLaunchKernelGGL(k_po_smooth, po_grid3(side[l]), po_block3(), 0, s, x[l], (const double*)b[l], (int)side[l], h2[l], colour);
        };
        for (int cyc = 0; cyc < cycles; ++cyc) {
            for (int l = 0; l < depth - 1; ++l) {
                if (l && (rc = mv_check(hipMemsetAsync(x[l], 0, (size_t)(side[l] * side[l] * side[l]) * 8, s), what))) return rc;
                smooth(l);
                hipLaunchKernelGGL(k_po_resid, po_grid3(side[l]), po_block3(), 0, s, (const double*)x[l], (const double*)b[l], (int)side[l], h2[l], r,
                                   (po_u64*)nullptr);
                hipLaunchKernelGGL(k_po_restrict, po_grid3(side[l + 1]), po_block3(), 0, s, (const double*)r, (int)side[l], b[l + 1], (int)side[l + 1]);
            }
            hipLaunchKernelGGL(k_po_direct, dim3(1), dim3(64), 0, s, x[depth - 1], (const double*)b[depth - 1], h2[depth - 1]);
            for (int l = depth - 2; l >= 0; --l) {
                hipLaunchKernelGGL(k_po_prolong, po_grid3(side[l]), po_block3(), 0, s, (const double*)x[l + 1], (int)side[l + 1], x[l], (int)side[l]);
                smooth(l);
            }
        }
        hipLaunchKernelGGL(k_po_resid, po_grid3(side[0]), po_block3(), 0, s, (const double*)x[0], (const double*)b[0], (int)side[0], h2[0], (double*)nullptr,
                           hdr + MVSDF_PO_H_RESIDUAL);
    }
    if (stages & PO_STAGE_ISO) {
        if ((rc = mv_check(hipMemsetAsync(values, 0, (size_t)n * 8, s), what))) return rc;
        hipLaunchKernelGGL(k_po_values, dim3(pgrid), dim3(PO_THREADS), 0, s, points, (long long)n, g, (const unsigned char*)(w + L.flags),
                           (const long long*)(w + L.off), (const double*)chi, values);
        const double* in = values;
        long long len = n;
        for (int turn = 0;; ++turn) {
            const long long nb = mv_ceil_div(len, PO_TREE);
            double* out = nb == 1 ? (double*)(hdr + MVSDF_PO_H_T) : (double*)(w + L.tree[turn & 1]);
            hipLaunchKernelGGL(k_po_tree, dim3((unsigned)nb), dim3(PO_THREADS), 0, s, in, len, out);
            if (nb == 1) break;
            in = out;
            len = nb;
        }
    }
    return mv_check(hipGetLastError(), what);                   // no wait here: the caller reads the header
}

int mvsdf_poisson_valid(const double* density, int32_t depth, double min_density, int32_t dilate, uint8_t* tmp, uint8_t* valid, void* stream) {
    const char* what = "mvsdf_poisson_valid";
    if (!density || !valid || depth < MVSDF_PO_MIN_DEPTH || depth > MVSDF_PO_MAX_DEPTH || dilate < 0 || (dilate > 0 && !tmp) || isnan(min_density))
        return mv_fail(-1, "mvsdf_poisson_valid: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    const long long N = po_side(depth, 0), vol = N * N * N;
    uint8_t* cur = (dilate & 1) ? tmp : valid;                      // the last step lands in valid
    hipLaunchKernelGGL(k_po_valid0, dim3(mv_grid(vol, PO_THREADS)), dim3(PO_THREADS), 0, s, density, vol, min_density, cur);
    for (int q = 0; q < dilate; ++q) {
        uint8_t* nxt = cur == valid ? tmp : valid;
        hipLaunchKernelGGL(k_po_dilate, po_grid3(N), po_block3(), 0, s, (const unsigned char*)cur, (int)N, nxt);
        cur = nxt;
    }
    return mv_check(hipGetLastError(), what);
}

int mvsdf_poisson_volume(const double* chi, int64_t count, double iso, float* out, void* stream) {
    if (!chi || !out || count < 1) return mv_fail(-1, "mvsdf_poisson_volume: bad arguments");
    hipLaunchKernelGGL(k_po_volume, dim3(mv_grid(count, PO_THREADS)), dim3(PO_THREADS), 0, (hipStream_t)stream, chi, (long long)count, iso, out);
    return mv_check(hipGetLastError(), "mvsdf_poisson_volume");
}

}  // extern "C"
