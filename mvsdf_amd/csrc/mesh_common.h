// mesh_common.h -- the marching-cubes formulas the dense (mesh_kernels.hip: plain and masked) and the sparse (mesh_sparse.hip) extractors share: the
// table decode, the crossing tests, the vertex position and the normal.  Both call these with an accessor val(i, j, k) -> the value at grid point
// (i, j, k), so they cannot drift apart: the sparse path's output is pinned bit for bit to the dense one (tests/test_gpu_mesh_sparse.py).  mc_vertex
// takes its gradient rule from the caller: McGrad (mc_grad_c, every point holds a value) unless a mask says otherwise (mesh_kernels.hip: McMaskGrad).
// Conventions: mvsdf_amd/mesh.py; the table: tools/gen_mc_tables.py -> mc_tables.h.
#pragma once
#include "geom_prims.h"

#define MC_TABLE static __constant__ const
#include "mc_tables.h"

// Every counting pass maps items to workgroups in linear order: workgroup b owns items [b * MESH_CHUNK, (b + 1) * MESH_CHUNK), its 256 lanes take
// MESH_CHUNK / 256 consecutive rounds of 256 (block_excl ranks them), and k_mesh_scan turns the per-workgroup totals into int64 offsets.  Workspace
// regions are 256-byte aligned (WsCursor).
#define MESH_THREADS 256
#define MESH_ROUNDS 4
#define MESH_CHUNK (MESH_THREADS * MESH_ROUNDS)
#define MESH_SCAN_THREADS 1024
#define MESH_HDR 256                                  // bytes at the start of every workspace: int64 results the host reads
static_assert(MVSDF_MC_H_VERTS == 0 && MVSDF_MC_H_FACES == 1 && MVSDF_MC_H_BAD == 2 && MVSDF_MC_H_WORDS * 8 <= MESH_HDR && MVSDF_CC_H_WORDS * 8 <= MESH_HDR,
              "k_mesh_scan's totals are the words of mvsdf_mc_count");

static_assert(MC_MAX_TRIS < 8, "k_mc_* count triangles per cell with 3 ballots");

struct McGeom {
    float sp[3], org[3];
};

__device__ __forceinline__ int mc_ntri(int ci) { return mc_tri_offset[ci + 1] - mc_tri_offset[ci]; }

// cube edge e (of the cell whose lower corner q holds): q becomes the edge's lower end (its owner); returns the edge's axis
__device__ __forceinline__ int mc_edge_owner(int e, long long* q) {
    const int a = e >> 2, m = e & 3;
    const int o0 = a == 0 ? 1 : 0, o1 = a == 2 ? 1 : 2;         // the two other axes, lower first
    q[o0] += m & 1;
    q[o1] += m >> 1 & 1;
    return a;
}

// crossing edges owned by grid point (i, j, k) of an n[0] x n[1] x n[2] grid: bit a = the edge to (i, j, k) + e_a crosses the level
template <class V>
__device__ __forceinline__ int mc_point_edges(const V& val, const long long* n, long long i, long long j, long long k, bool in0, float level) {
    int bits = 0;
    if (i + 1 < n[0] && in0 != (val(i + 1, j, k) < level)) bits |= 1;
    if (j + 1 < n[1] && in0 != (val(i, j + 1, k) < level)) bits |= 2;
    if (k + 1 < n[2] && in0 != (val(i, j, k + 1) < level)) bits |= 4;
    return bits;
}

// cube index of the cell with lower corner (i, j, k), which must exist (bit c: corner (c & 1, c >> 1 & 1, c >> 2 & 1) is inside)
template <class V>
__device__ __forceinline__ int mc_cube_index(const V& val, long long i, long long j, long long k, float level) {
    int ci = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) ci |= (val(i + (c & 1), j + (c >> 1 & 1), k + (c >> 2 & 1)) < level) << c;
    return ci;
}

// gradient component c at grid point g: central difference inside, one-sided at the border, over the spacing
template <class V>
__device__ __forceinline__ float mc_grad_c(const V& val, const long long* n, const long long* g, int c, float h) {
    const long long nc = n[c], x = g[c];
    if (nc < 2) return 0.0f;
    long long lo[3] = {g[0], g[1], g[2]}, hi[3] = {g[0], g[1], g[2]};
    float den = h;
    if (x == 0) {
        hi[c] = 1;
    } else if (x == nc - 1) {
        lo[c] = nc - 2;
    } else {
        lo[c] = x - 1;
        hi[c] = x + 1;
        den = 2.0f * h;
    }
    return (val(hi[0], hi[1], hi[2]) - val(lo[0], lo[1], lo[2])) / den;
}

// the gradient rule of a grid whose every point holds a value: mc_grad_c
struct McGrad {
    template <class V>
    __device__ __forceinline__ float operator()(const V& val, const long long* n, const long long* g, int c, float h) const {
        return mc_grad_c(val, n, g, c, h);
    }
};

// the vertex on the crossing edge (g, g + e_a), x = the value at g: position and normal -> vert[3], normal[3].  grad(val, n, g, c, h) is the gradient
// rule at the edge's two ends.
template <class V, class G = McGrad>
__device__ __forceinline__ void mc_vertex(const V& val, const long long* n, const long long* g, int a, float x, float level, const McGeom& gm,
                                          float* vert, float* normal, const G& grad = G()) {
    long long g1[3] = {g[0], g[1], g[2]};
    g1[a] += 1;
    const float x1 = val(g1[0], g1[1], g1[2]);
    const float t = (level - x) / (x1 - x);
    float nr[3];
    for (int c = 0; c < 3; ++c) {
        vert[c] = c == a ? gm.org[c] + ((float)g[c] + t) * gm.sp[c] : gm.org[c] + (float)g[c] * gm.sp[c];
        const float d0 = grad(val, n, g, c, gm.sp[c]), d1 = grad(val, n, g1, c, gm.sp[c]);
        nr[c] = d0 + t * (d1 - d0);
    }
    const float nn = sqrtf((nr[0] * nr[0] + nr[1] * nr[1]) + nr[2] * nr[2]);
    for (int c = 0; c < 3; ++c) normal[c] = nn > 0.0f ? nr[c] / nn : 0.0f;
}

// exclusive rank of x (0 <= x < 2^nbits) among the block's items so far, in item order; `running` (uniform) carries the block's total across rounds.
// Every lane of the block calls it the same number of times.
__device__ __forceinline__ long long block_excl(int x, int nbits, int* s_w, long long& running) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    int pre = 0, tot = 0;
    for (int b = 0; b < nbits; ++b) {
        const unsigned long long m = __ballot((x >> b) & 1);
        pre += __popcll(m & lt) << b;
        tot += __popcll(m) << b;
    }
    if (lane == 0) s_w[w] = tot;
    __syncthreads();
    long long base = running;
    int all = 0;
    for (int q = 0; q < MESH_THREADS / 64; ++q) {
        const int t = s_w[q];
        if (q < w) base += t;
        all += t;
    }
    __syncthreads();
    running += all;
    return base + pre;
}

// the running sums of k_mesh_scan's two arrays, scanned together
struct MeshSum2 {
    long long a, b;
    __device__ MeshSum2& operator+=(const MeshSum2& o) {
        a += o.a;
        b += o.b;
        return *this;
    }
};

// exclusive int64 offsets of one or two per-workgroup count arrays (b may be NULL) -> oa / ob; tot[0] / tot[1] = the sums, tot[2] = 1 if a count was negative
static __global__ __launch_bounds__(MESH_SCAN_THREADS) void k_mesh_scan(const int* __restrict__ a, const int* __restrict__ b, int nb, long long* __restrict__ oa,
                                                                 long long* __restrict__ ob, long long* __restrict__ tot) {
    __shared__ MeshSum2 sh[MESH_SCAN_THREADS];
    __shared__ int s_bad;
    const int t = threadIdx.x, per = (nb + MESH_SCAN_THREADS - 1) / MESH_SCAN_THREADS;
    const int lo = min(nb, t * per), hi = min(nb, lo + per);
    if (t == 0) s_bad = 0;
    MeshSum2 own = {0, 0};
    int bad = 0;
    for (int q = lo; q < hi; ++q) {
        bad |= a[q] < 0 || (b && b[q] < 0);
        own.a += a[q];
        if (b) own.b += b[q];
    }
    const MeshSum2 incl = mv_block_scan_incl<MESH_SCAN_THREADS>(own, sh);   // (its barriers order s_bad = 0 before the line below)
    if (bad) s_bad = 1;
    long long ra = incl.a - own.a, rb = incl.b - own.b;
    for (int q = lo; q < hi; ++q) {
        oa[q] = ra;
        ra += a[q];
        if (b) {
            ob[q] = rb;
            rb += b[q];
        }
    }
    if (t == MESH_SCAN_THREADS - 1) {
        tot[0] = incl.a;
        tot[1] = incl.b;
    }
    __syncthreads();
    if (t == 0) tot[2] = s_bad;
}
