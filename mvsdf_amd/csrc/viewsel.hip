// viewsel.hip -- on-device view selection: the pairwise score of MVSNet-style pair.txt files from points, camera centres and visibility, and the camera
// depths behind the depth ranges.  Python: mvsdf_amd/viewsel.py, which states the definition; tests/viewsel_ref.py restates it in numpy.  All arithmetic
// is fp64 without contraction, in the order the definition writes it; atan2 and exp are the written-out ones of det_math64.h (no library call).
//
// * k_vs_pack_dense / k_vs_pack_tracks: both visibility forms become one bit matrix, uint64 [P][nw], nw = ceil(V / 64): bit (v mod 64) of word v / 64 of
//   row p is set iff view v sees point p.  A lane owns whole words (dense) or a whole row (tracks), so no atomics; a duplicate track entry sets its bit again.
// * k_vs_score: a 256-lane workgroup owns one tile of 64 x 64 view pairs (I, J), I <= J, and a slice of the points.  A wave takes a point at a time and
//   reads its two words; lane l holds the centres of views 64 I + l and 64 J + l in registers and computes the unit vectors from the point to them ONCE per
//   point and tile.  The wave then walks the set bits i of word I (a scalar loop), broadcasts unit vector i, and every lane j whose bit of word J is set
//   evaluates the pair and adds its quantised weight to the tile's int64 cell [i][j] in LDS (ds_add_u64; the lanes of a wave hit 64 different cells) and 1
//   to the count cell.  On the diagonal tile only j >= i is visited (j == i: the count alone).  The tile (32 KB of scores + 16 KB of counts) is flushed with
//   64-bit global atomics, mirrored on write, cells with a zero count skipped.  Integer sums are exact and associative: the schedule cannot change a bit.
// * k_vs_finish: scores = fp64(S) * 2^-32.  k_vs_depths: the camera depth of every point a view sees (+inf elsewhere), sorted by the caller.
//
// Error bits (int64 {0, bits} in the 256-byte header; the pack calls reset it, the others OR into it): 1 a non-finite point, centre or extrinsic entry,
// 2 a track entry outside [0, V) or track offsets that are not ascending within [0, nnz], 4 V < 1, V > 65535 or P >= 2^31 (nothing is launched).
#include <float.h>
#include "geom_prims.h"
#include "det_math64.h"

#define VS_THREADS 256
#define VS_TILE 64
#define VS_HDR 256
static_assert(MVSDF_RES_H_WORDS * 8 <= VS_HDR, "the result words fit the header");
#define VS_TARGET_WGS 1024                            // workgroups the score kernel aims for (4 per CU: three tiles of 48 KB fit a CU's LDS)

typedef unsigned long long vs_u64;

static inline long long vs_min(long long a, long long b) { return a < b ? a : b; }

// ---- the definition's arithmetic, host and device (mvsdf_viewsel_weights_host runs the same functions on the CPU) ----

struct VsVec {
    double x, y, z;
};

// the unit vector of d; (0, 0, 0) unless its norm is a positive finite double
__host__ __device__ static inline VsVec vs_unit(double dx, double dy, double dz) {
    const double n = sqrt((dx * dx + dy * dy) + dz * dz);
    VsVec u = {0.0, 0.0, 0.0};
    if (n > 0.0 && n <= DBL_MAX) {
        u.x = dx / n;
        u.y = dy / n;
        u.z = dz / n;
    }
    return u;
}

// the angle between unit vectors a and b in degrees
__host__ __device__ static inline double vs_theta(const VsVec a, const VsVec b) {
    const double cx = a.y * b.z - a.z * b.y;
    const double cy = a.z * b.x - a.x * b.z;
    const double cz = a.x * b.y - a.y * b.x;
    const double nc = sqrt((cx * cx + cy * cy) + cz * cz);
    const double dt = (a.x * b.x + a.y * b.y) + a.z * b.z;
    return DM64_DEG * dm64_atan2_pos(nc, dt);
}

__host__ __device__ static inline double vs_weight(double theta, double theta0, double s1, double s2) {
    const double d = theta - theta0;
    const double s = theta <= theta0 ? s1 : s2;
    const double q = (d * d) / (2.0 * (s * s));
    return dm64_expneg(-q);
}

__host__ __device__ static inline long long vs_quantise(double w) { return (long long)dm64_rint(w * 4294967296.0); }

// ---- kernels ----

// ORs MVSDF_VS_ERR_FINITE into the header when an entry of f[n] is not finite
static void vs_finite(const double* f, long long n, void* hdr, hipStream_t s) {
    hipLaunchKernelGGL(k_any_nonfinite<double>, dim3((unsigned)vs_min(mv_ceil_div(n, MV_THREADS), 1024ll)), dim3(MV_THREADS), 0, s, f, n, (vs_u64*)hdr + MVSDF_RES_H_ERR,
                       (vs_u64)MVSDF_VS_ERR_FINITE);
}

// vis uint8 [V][P] -> bits [P][nw]; consecutive lanes take consecutive points of one word, so the 64 byte reads of a lane are coalesced over the wave
__global__ __launch_bounds__(VS_THREADS) void k_vs_pack_dense(const unsigned char* __restrict__ vis, int V, long long P, int nw, vs_u64* __restrict__ bits) {
    const long long idx = (long long)blockIdx.x * VS_THREADS + threadIdx.x;
    if (idx >= P * nw) return;
    const int w = (int)(idx / P);
    const long long p = idx - (long long)w * P;
    vs_u64 word = 0;
    const int v0 = w * 64, n = min(64, V - v0);
    for (int b = 0; b < n; ++b)
        if (vis[(long long)(v0 + b) * P + p]) word |= 1ull << b;
    bits[p * nw + w] = word;
}

// tracks (CSR) -> bits [P][nw]; one lane per point
__global__ __launch_bounds__(VS_THREADS) void k_vs_pack_tracks(const long long* __restrict__ off, const int* __restrict__ view, long long nnz, int V, long long P,
                                                               int nw, vs_u64* __restrict__ bits, long long* __restrict__ hdr) {
    const long long p = (long long)blockIdx.x * VS_THREADS + threadIdx.x;
    if (p >= P) return;
    vs_u64* __restrict__ row = bits + p * nw;
    for (int w = 0; w < nw; ++w) row[w] = 0;
    const long long b = off[p], e = off[p + 1];
    bool bad = b < 0 || e < b || e > nnz;
    if (!bad)
        for (long long k = b; k < e; ++k) {
            const int v = view[k];
            if (v < 0 || v >= V) { bad = true; continue; }
            row[v >> 6] |= 1ull << (v & 63);
        }
    if (bad) atomicOr((vs_u64*)(hdr + MVSDF_RES_H_ERR), (vs_u64)MVSDF_VS_ERR_TRACK);
}

__device__ __forceinline__ vs_u64 vs_uniform(vs_u64 x) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)x), hi = __builtin_amdgcn_readfirstlane((unsigned)(x >> 32));
    return ((vs_u64)hi << 32) | lo;
}

__global__ __launch_bounds__(VS_THREADS) void k_vs_score(const double* __restrict__ pts, const double* __restrict__ ctr, const vs_u64* __restrict__ bits, int V,
                                                         long long P, int nw, long long per, double theta0, double s1, double s2, vs_u64* __restrict__ S,
                                                         vs_u64* __restrict__ C) {
    __shared__ vs_u64 sS[VS_TILE * VS_TILE];
    __shared__ unsigned sC[VS_TILE * VS_TILE];
    int I = 0, rest = (int)blockIdx.x;                                   // tile number -> (I, J), I <= J, row by row
    while (rest >= nw - I) { rest -= nw - I; ++I; }
    const int J = I + rest;
    for (int c = threadIdx.x; c < VS_TILE * VS_TILE; c += VS_THREADS) { sS[c] = 0; sC[c] = 0; }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int vi = I * 64 + lane, vj = J * 64 + lane;
    double cix = 0.0, ciy = 0.0, ciz = 0.0, cjx = 0.0, cjy = 0.0, cjz = 0.0;
    if (vi < V) { cix = ctr[3 * vi]; ciy = ctr[3 * vi + 1]; ciz = ctr[3 * vi + 2]; }
    if (vj < V) { cjx = ctr[3 * vj]; cjy = ctr[3 * vj + 1]; cjz = ctr[3 * vj + 2]; }
    const bool diag = I == J;
    const long long p0 = (long long)blockIdx.y * per, p1 = min(P, p0 + per);
    for (long long p = p0 + wave; p < p1; p += VS_THREADS / 64) {
        const vs_u64 wI = vs_uniform(bits[p * nw + I]), wJ = vs_uniform(bits[p * nw + J]);
        if (wI == 0 || wJ == 0) continue;
        const double px = pts[3 * p], py = pts[3 * p + 1], pz = pts[3 * p + 2];
        const bool mine = (wJ >> lane) & 1;
        const VsVec ui = vs_unit(cix - px, ciy - py, ciz - pz);         // lanes without the bit compute a vector nobody reads
        const VsVec uj = diag ? ui : vs_unit(cjx - px, cjy - py, cjz - pz);
        for (vs_u64 m = wI; m; m &= m - 1) {
            const int i = __builtin_ctzll(m);
            VsVec a;
            a.x = __shfl(ui.x, i);
            a.y = __shfl(ui.y, i);
            a.z = __shfl(ui.z, i);
            if (mine && !(diag && lane < i)) {
                atomicAdd(&sC[i * VS_TILE + lane], 1u);
                if (!(diag && lane == i)) {
                    const double theta = vs_theta(a, uj);                // a belongs to the view of the lower index
                    atomicAdd(&sS[i * VS_TILE + lane], (vs_u64)vs_quantise(vs_weight(theta, theta0, s1, s2)));
                }
            }
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < VS_TILE * VS_TILE; c += VS_THREADS) {
        const unsigned n = sC[c];
        if (!n) continue;
        const long long gi = I * 64 + (c >> 6), gj = J * 64 + (c & 63);     // both < V: bits beyond V are never set
        atomicAdd(&C[gi * V + gj], (vs_u64)n);
        if (gi != gj) {
            atomicAdd(&C[gj * V + gi], (vs_u64)n);
            atomicAdd(&S[gi * V + gj], sS[c]);
            atomicAdd(&S[gj * V + gi], sS[c]);
        }
    }
}

__global__ __launch_bounds__(VS_THREADS) void k_vs_finish(const vs_u64* __restrict__ S, long long n, double* __restrict__ scores) {
    const long long i = (long long)blockIdx.x * VS_THREADS + threadIdx.x;
    if (i < n) scores[i] = (double)(long long)S[i] * 2.3283064365386963e-10;       // 2^-32
}

// z[v - v0][p] = ((r20*x + r21*y) + r22*z) + t2 where view v sees p, +inf elsewhere; E fp64 [V][4] = row 2 of the extrinsics
__global__ __launch_bounds__(VS_THREADS) void k_vs_depths(const double* __restrict__ pts, const vs_u64* __restrict__ bits, const double* __restrict__ E, int v0,
                                                          int nv, long long P, int nw, double* __restrict__ z) {
    const long long idx = (long long)blockIdx.x * VS_THREADS + threadIdx.x;
    if (idx >= nv * P) return;
    const int k = (int)(idx / P);
    const long long p = idx - (long long)k * P;
    const int v = v0 + k;
    double out = INFINITY;
    if ((bits[p * nw + (v >> 6)] >> (v & 63)) & 1) {
        out = mv_row4(E + 4 * v, pts[3 * p], pts[3 * p + 1], pts[3 * p + 2], 1.0);
    }
    z[idx] = out;
}

static inline bool vs_shape_ok(int64_t V, int64_t P) { return V >= 1 && V <= MVSDF_VS_MAX_VIEWS && P >= 0 && P <= INT_MAX; }
static inline int vs_words(int64_t V) { return (int)((V + 63) / 64); }

extern "C" {

size_t mvsdf_viewsel_bits_bytes(int64_t V, int64_t P) {
    if (!vs_shape_ok(V, P)) return 0;
    const size_t b = (size_t)P * (size_t)vs_words(V) * 8;
    return b ? b : 8;
}

size_t mvsdf_viewsel_workspace_bytes(int64_t V) {
    if (V < 1 || V > MVSDF_VS_MAX_VIEWS) return 0;
    return VS_HDR + (size_t)V * (size_t)V * 8;
}

int mvsdf_viewsel_pack_dense(const uint8_t* vis, int64_t V, int64_t P, void* bits, void* hdr, void* stream) {
    const char* what = "mvsdf_viewsel_pack_dense";
    if (!hdr || (P > 0 && (!bits || !vis))) return mv_fail(-1, "mvsdf_viewsel_pack_dense: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (!vs_shape_ok(V, P)) return mv_refuse_header(hdr, MVSDF_VS_ERR_SHAPE, s, what);
    if (int rc = mv_check(hipMemsetAsync(hdr, 0, VS_HDR, s), what)) return rc;
    if (P == 0) return 0;
    const int nw = vs_words(V);
    const long long blocks = mv_ceil_div((long long)P * nw, VS_THREADS);
    if (blocks > INT_MAX) return mv_fail(-1, "mvsdf_viewsel_pack_dense: P * ceil(V / 64) beyond the grid limit");
    hipLaunchKernelGGL(k_vs_pack_dense, dim3((unsigned)blocks), dim3(VS_THREADS), 0, s, vis, (int)V, (long long)P, nw, (vs_u64*)bits);
    return mv_check(hipGetLastError(), what);
}

int mvsdf_viewsel_pack_tracks(const int64_t* track_off, const int32_t* track_view, int64_t nnz, int64_t V, int64_t P, void* bits, void* hdr, void* stream) {
    const char* what = "mvsdf_viewsel_pack_tracks";
    if (!hdr || !track_off || (P > 0 && !bits) || nnz < 0 || (nnz > 0 && !track_view)) return mv_fail(-1, "mvsdf_viewsel_pack_tracks: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (!vs_shape_ok(V, P)) return mv_refuse_header(hdr, MVSDF_VS_ERR_SHAPE, s, what);
    if (int rc = mv_check(hipMemsetAsync(hdr, 0, VS_HDR, s), what)) return rc;
    if (P == 0) return 0;
    hipLaunchKernelGGL(k_vs_pack_tracks, dim3(mv_grid(P, VS_THREADS)), dim3(VS_THREADS), 0, s, (const long long*)track_off, track_view,
                       (long long)nnz, (int)V, (long long)P, vs_words(V), (vs_u64*)bits, (long long*)hdr);
    return mv_check(hipGetLastError(), what);
}

int mvsdf_viewsel_scores(const double* points, const double* centers, const void* bits, int64_t V, int64_t P, double theta0, double sigma1, double sigma2,
                         void* ws, size_t ws_bytes, double* scores, int64_t* counts, void* hdr, void* stream) {
    const char* what = "mvsdf_viewsel_scores";
    if (!vs_shape_ok(V, P) || !centers || !ws || !scores || !counts || !hdr || (P > 0 && (!points || !bits)) || !isfinite(theta0) || !(sigma1 > 0.0) ||
        !(sigma2 > 0.0) || !isfinite(sigma1) || !isfinite(sigma2))
        return mv_fail(-1, "mvsdf_viewsel_scores: bad arguments");
    if (ws_bytes < mvsdf_viewsel_workspace_bytes(V)) return mv_fail(-1, "mvsdf_viewsel_scores: workspace too small (mvsdf_viewsel_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    const long long vv = (long long)V * V;
    vs_u64* S = (vs_u64*)((char*)ws + VS_HDR);
    int rc;
    if ((rc = mv_check(hipMemsetAsync(S, 0, (size_t)vv * 8, s), what))) return rc;
    if ((rc = mv_check(hipMemsetAsync(counts, 0, (size_t)vv * 8, s), what))) return rc;
    vs_finite(centers, 3 * V, hdr, s);
    if (P > 0) {
        vs_finite(points, 3 * P, hdr, s);
        const int nw = vs_words(V);
        const long long tiles = (long long)nw * (nw + 1) / 2;
        long long slices = vs_min(vs_min(mv_ceil_div(VS_TARGET_WGS, tiles), mv_ceil_div(P, VS_THREADS)), 65535ll);       // >= 1: P > 0
        const long long per = mv_ceil_div(P, slices);
        slices = mv_ceil_div(P, per);
        hipLaunchKernelGGL(k_vs_score, dim3((unsigned)tiles, (unsigned)slices), dim3(VS_THREADS), 0, s, points, centers, (const vs_u64*)bits, (int)V, (long long)P, nw,
                           per, theta0, sigma1, sigma2, S, (vs_u64*)counts);
    }
    hipLaunchKernelGGL(k_vs_finish, dim3(mv_grid(vv, VS_THREADS)), dim3(VS_THREADS), 0, s, S, vv, scores);
    return mv_check(hipGetLastError(), what);
}

int mvsdf_viewsel_depths(const double* points, const void* bits, const double* ext_row2, int64_t V, int64_t P, int64_t first, int64_t nviews, double* z,
                         void* hdr, void* stream) {
    const char* what = "mvsdf_viewsel_depths";
    if (!vs_shape_ok(V, P) || P < 1 || !points || !bits || !ext_row2 || !z || !hdr || first < 0 || nviews < 1 || first + nviews > V)
        return mv_fail(-1, "mvsdf_viewsel_depths: bad arguments");
    const long long blocks = mv_ceil_div((long long)nviews * P, VS_THREADS);
    if (blocks > INT_MAX) return mv_fail(-1, "mvsdf_viewsel_depths: nviews * P beyond the grid limit");
    hipStream_t s = (hipStream_t)stream;
    vs_finite(ext_row2 + 4 * first, 4 * nviews, hdr, s);
    if (first == 0) vs_finite(points, 3 * P, hdr, s);
    hipLaunchKernelGGL(k_vs_depths, dim3((unsigned)blocks), dim3(VS_THREADS), 0, s, points, (const vs_u64*)bits, ext_row2, (int)first, (int)nviews, (long long)P,
                       vs_words(V), z);
    return mv_check(hipGetLastError(), what);
}

// HOST: the definition's theta and quantised weight for n pairs of vectors a = c_i - p, b = c_j - p (fp64 [n][3] each, host memory), by the same functions
// the kernel runs.  The library loads without a GPU, so the non-GPU suite pins det_math64.h to the numpy restatement through this.
int mvsdf_viewsel_weights_host(const double* a, const double* b, int64_t n, double theta0, double sigma1, double sigma2, double* theta, int64_t* wq) {
    if (n < 0 || (n > 0 && (!a || !b || !theta || !wq))) return mv_fail(-1, "mvsdf_viewsel_weights_host: bad arguments");
    for (int64_t k = 0; k < n; ++k) {
        const VsVec ua = vs_unit(a[3 * k], a[3 * k + 1], a[3 * k + 2]), ub = vs_unit(b[3 * k], b[3 * k + 1], b[3 * k + 2]);
        theta[k] = vs_theta(ua, ub);
        wq[k] = vs_quantise(vs_weight(theta[k], theta0, sigma1, sigma2));
    }
    return 0;
}

}  // extern "C"
