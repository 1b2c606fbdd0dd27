// geom_prims.h -- what the scene-side modules (mesh extraction and trimming, Chamfer, cloud cleaning, fusion, rasterisation, stereo, view selection)
// share: workspace arithmetic, the header copies, the 4x4 row product, the two-level exclusive scan with its in-chunk rank, and the finite check.  What
// looks through a camera into an image (projection, the 2x2 bilinear cell, visibility) is view_prims.h, which includes this file.
// Everything here is integer or order-fixed fp64 arithmetic, so every caller gets the same bits.  Kernels are static: each including file gets its own copies.
#pragma once
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include "capi_util.h"

#define MV_THREADS 256
#define MV_ITEMS 8                                    // consecutive items per lane in the scans and the emit passes
#define MV_CHUNK (MV_THREADS * MV_ITEMS)
#define MV_TOP_THREADS 1024

// ================================================================ host: sizes, workspace regions, header copies ================================================================
static inline size_t mv_align256(size_t b) { return (b + 255) & ~(size_t)255; }
static inline long long mv_ceil_div(long long n, long long per) { return (n + per - 1) / per; }
// mv_ceil_div as a grid size; a count the grid cannot hold gives 0, which the launch refuses (hipGetLastError reports it)
static inline unsigned mv_grid(long long n, long long per) {
    const long long g = mv_ceil_div(n, per);
    return g >= 0 && g <= INT_MAX ? (unsigned)g : 0u;
}

// regions of a workspace, one after the other, every one 256-byte aligned: x = c.take(bytes) ...; total = c.o
struct WsCursor {
    size_t o;
    size_t take(size_t bytes) {
        const size_t at = o;
        o += mv_align256(bytes);
        return at;
    }
};

// n int64 words to the start of the workspace, then a wait: hdr may live on the caller's stack frame
static inline int mv_write_header(void* ws, const long long* hdr, int n, hipStream_t s, const char* what) {
    if (int rc = mv_check(hipMemcpyAsync(ws, hdr, (size_t)n * 8, hipMemcpyHostToDevice, s), what)) return rc;
    return mv_check(hipStreamSynchronize(s), what);
}

// the header of a call that leaves MVSDF_RES_H_* and stops at its argument checks: {0, error bits}, then a wait
static inline int mv_refuse_header(void* ws, long long err, hipStream_t s, const char* what) {
    long long hdr[MVSDF_RES_H_WORDS] = {};
    hdr[MVSDF_RES_H_ERR] = err;
    return mv_write_header(ws, hdr, MVSDF_RES_H_WORDS, s, what);
}

// bytes from the device, then a wait
static inline int mv_read(void* host, const void* dev, size_t bytes, hipStream_t s, const char* what) {
    if (int rc = mv_check(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s), what)) return rc;
    return mv_check(hipStreamSynchronize(s), what);
}

// ================================================================ device ================================================================
// one row of a 4x4 matrix times q, in the definitions' order
__device__ __forceinline__ double mv_row4(const double* __restrict__ t, double q0, double q1, double q2, double q3) {
    return ((t[0] * q0 + t[1] * q1) + t[2] * q2) + t[3] * q3;
}

// inclusive Hillis-Steele scan of x over the THREADS lanes of the workgroup (sh: THREADS entries; T() is zero)
template <int THREADS, class T>
__device__ __forceinline__ T mv_block_scan_incl(T x, T* sh) {
    const int t = threadIdx.x;
    sh[t] = x;
    __syncthreads();
    for (int d = 1; d < THREADS; d <<= 1) {
        const T y = t >= d ? sh[t - d] : T();
        __syncthreads();
        sh[t] += y;
        __syncthreads();
    }
    return sh[t];
}

// lane t of workgroup b owns items [b * THREADS * ITEMS + t * ITEMS, + ITEMS) of a[n]: loads them into k (0 beyond n) -> boff[b] + the sum of the
// workgroup's items before the lane's first, i.e. the output row of that first item
template <int THREADS, int ITEMS, class T, class S>
__device__ __forceinline__ long long mv_chunk_rank(const T* a, long long n, const long long* __restrict__ boff, S (&k)[ITEMS], S* sh) {
    const long long base = (long long)blockIdx.x * (THREADS * ITEMS) + (long long)threadIdx.x * ITEMS;
    S s = 0;
#pragma unroll
    for (int q = 0; q < ITEMS; ++q) {
        k[q] = base + q < n ? a[base + q] : 0;
        s += k[q];
    }
    return boff[blockIdx.x] + (mv_block_scan_incl<THREADS>(s, sh) - s);
}

// ================================================================ exclusive scan of a[n] -> int64 (uint8 flags or int64 counts) ================================================================
// per-workgroup totals of a[n]
template <class T>
static __global__ __launch_bounds__(MV_THREADS) void k_scan_block_sum(const T* __restrict__ a, long long n, long long* __restrict__ bsum) {
    typedef decltype(T() + 0) S;                                  // int for the flags, int64 for the counts
    __shared__ S sh[MV_THREADS];
    const long long base = (long long)blockIdx.x * MV_CHUNK + (long long)threadIdx.x * MV_ITEMS;
    S s = 0;
    for (int q = 0; q < MV_ITEMS; ++q)
        if (base + q < n) s += a[base + q];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int d = MV_THREADS / 2; d; d >>= 1) {
        if ((int)threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum[blockIdx.x] = sh[0];
}

// in place: exclusive scan of bsum[nb]; *total = the sum (one workgroup of THREADS = MV_TOP_THREADS lanes, serial ranges per lane; a template so that
// only the files that scan carry it)
template <int THREADS>
static __global__ __launch_bounds__(THREADS) void k_scan_top(long long* __restrict__ bsum, long long nb, long long* __restrict__ total) {
    __shared__ long long sh[THREADS];
    const int t = threadIdx.x;
    const long long per = (nb + THREADS - 1) / THREADS;
    const long long lo = min(nb, t * per), hi = min(nb, lo + per);
    long long s = 0;
    for (long long q = lo; q < hi; ++q) s += bsum[q];
    const long long incl = mv_block_scan_incl<THREADS>(s, sh);
    long long r = incl - s;
    for (long long q = lo; q < hi; ++q) {
        const long long v = bsum[q];
        bsum[q] = r;
        r += v;
    }
    if (t == THREADS - 1) *total = incl;
}

// out[i] = boff[block] + the exclusive prefix of a inside the block (out may alias a)
template <class T>
static __global__ __launch_bounds__(MV_THREADS) void k_scan_apply(const T* a, long long n, const long long* __restrict__ boff, long long* out) {
    __shared__ long long sh[MV_THREADS];
    const long long base = (long long)blockIdx.x * MV_CHUNK + (long long)threadIdx.x * MV_ITEMS;
    long long v[MV_ITEMS];
    long long r = mv_chunk_rank<MV_THREADS, MV_ITEMS>(a, n, boff, v, sh);
#pragma unroll
    for (int q = 0; q < MV_ITEMS; ++q) {
        if (base + q < n) out[base + q] = r;
        r += v[q];
    }
}

static inline size_t mv_scan_tmp_bytes(long long n) { return mv_align256((size_t)(mv_ceil_div(n, MV_CHUNK) + 1) * 8); }

// the first two launches: bsum[nb] = the exclusive offsets of the nb = ceil(n / MV_CHUNK) chunks of a, *total = the sum (on the device).  A consumer that
// ranks its own chunk (mv_chunk_rank) needs no third one.
template <class T>
static inline void mv_scan_blocks(const T* a, long long n, long long* bsum, long long nb, long long* total, hipStream_t s) {
    hipLaunchKernelGGL(k_scan_block_sum<T>, dim3((unsigned)nb), dim3(MV_THREADS), 0, s, a, n, bsum);
    hipLaunchKernelGGL(k_scan_top<MV_TOP_THREADS>, dim3(1), dim3(MV_TOP_THREADS), 0, s, bsum, nb, total);
}

// exclusive scan of a[n] (n >= 1) into out (may alias a); tmp: mv_scan_tmp_bytes(n); total: one int64 on the device
template <class T>
static inline void mv_scan(const T* a, long long n, long long* out, void* tmp, long long* total, hipStream_t s) {
    const long long nb = mv_ceil_div(n, MV_CHUNK);
    long long* bsum = (long long*)tmp;
    mv_scan_blocks(a, n, bsum, nb, total, s);
    hipLaunchKernelGGL(k_scan_apply<T>, dim3((unsigned)nb), dim3(MV_THREADS), 0, s, a, n, (const long long*)bsum, out);
}

// ================================================================ finite check ================================================================
// ORs bit into *word when an entry of f[n] is NaN or infinite (grid-stride: the caller caps the grid; one atomic per wave that saw one)
template <class T>
static __global__ __launch_bounds__(MV_THREADS) void k_any_nonfinite(const T* __restrict__ f, long long n, unsigned long long* __restrict__ word,
                                                                     unsigned long long bit) {
    bool bad = false;
    for (long long i = (long long)blockIdx.x * MV_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * MV_THREADS) bad = bad || !isfinite(f[i]);
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(word, bit);
}

// ================================================================ the canonical pairwise sum ================================================================
// A sum over the canonical tree pads its terms with +0.0 to a power of two and adds adjacent pairs until one value is left, so the result depends on
// neither the workgroup size nor the schedule.  One chunk of it: a workgroup of MV_THREADS lanes over MV_CHUNK values, lane t holding values
// MV_ITEMS t .. MV_ITEMS t + MV_ITEMS - 1 in a[] (adjacent pairs in registers, then in LDS); every lane receives the sum.  Chunk sums are reduced the
// same way (poisson.hip: the isovalue; bundle.hip: the sums over a view's observations, the cost, the solver's dot products).  sh: MV_THREADS doubles
// of LDS, free to be reused at once by another call.
__device__ __forceinline__ double mv_tree_chunk(double* a, double* sh) {
    const int t = threadIdx.x;
#pragma unroll
    for (int m = MV_ITEMS / 2; m; m >>= 1)
#pragma unroll
        for (int q = 0; q < m; ++q) a[q] = a[2 * q] + a[2 * q + 1];
    __syncthreads();
    sh[t] = a[0];
    __syncthreads();
    for (int m = MV_THREADS / 2; m; m >>= 1) {
        double v = 0.0;
        if (t < m) v = sh[2 * t] + sh[2 * t + 1];
        __syncthreads();
        if (t < m) sh[t] = v;
        __syncthreads();
    }
    return sh[0];
}
