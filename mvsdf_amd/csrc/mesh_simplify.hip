// mesh_simplify.hip -- on-device mesh simplification: vertex clustering on a uniform grid with quadric-error placement (Lindstrom 2000).
// Python: mvsdf_amd/mesh.py (Mesh.simplify), whose doc states the definition; tests/simplify_ref.py restates it in numpy and is the arbiter for the bits.
//
// Everything that decides a bit is integer work or fp64 arithmetic in a fixed order (the build passes -ffp-contract=off), so the result does not depend
// on the schedule.  The sorts are nn_tree.h's stable LSD radix sort, the scans geom_prims.h's mv_scan.  Passes of the count call (mvsdf_mesh_simplify):
//   1  k_sp_bbox_part / _final: the box of the vertices (min / max are order-free) and the finite check; k_sp_face_check: vertex ids in range.
//      The host reads the box (48 bytes): it gives the default origin, refuses cell indices outside [0, 2^21) without another launch and tells
//      how many bits each axis' index needs, so that the vertex sort runs over those bits only.
//   2  k_sp_vkeys: key = the packed cell index, value = the vertex id; stable sort -> every cell is a segment with ascending vertex ids.
//   3  k_sp_heads, two scans, k_sp_segs, k_sp_assign: the segment of every sorted position, and the clusters numbered by their lowest vertex id
//      (the head of a segment is its lowest member; a flag per head VERTEX, scanned over the vertex ids, numbers the clusters).
//   4  k_sp_fkeys_lo, sort, k_sp_fkeys_hi, sort: the faces by their cluster triple rotated smallest-first, (r0, r1, r2): LSD over r2 and then
//      r0 << b | r1 (b = the bits of a cluster id).  One route for every size: the second key is rebuilt from the face ids the first sort
//      moved, which costs one elementwise launch and at most one more digit pass than a single 3 b-bit key, and needs no 63-bit limit.
//      k_sp_dups: a face is kept iff it is not degenerate and its predecessor in that order has another triple (the sort is stable: the
//      lowest face id leads its run); used-cluster flags; two scans -> output rows of faces and clusters.
//   5  (not for a counts-only call) k_sp_ckeys, sort: the 3 F corners by cluster, corner index ascending inside a cluster; k_sp_cseg: each
//      cluster's corner range.  k_sp_cluster: ONE LANE PER USED CLUSTER walks its vertex segment (sums in ascending vertex id) and its corner
//      segment (each corner's face normal is recomputed from the three vertices: nothing per corner is staged), then solves the 3x3 system by
//      the written-out adjugate and tests the candidate's cell.  Results: fp32 position / normal / colour per cluster in the workspace.
// mvsdf_mesh_simplify_emit compacts them and the kept faces into the caller's arrays.
//
// A cell that holds thousands of vertices is one long segment in one lane of k_sp_cluster.  That is accepted (such a cell is a user's choice of a
// very coarse grid, where few clusters exist anyway); there is no second path for it.
//
// Bounds: vertex ids are checked before anything reads through them; cluster ids come from scans over nv flags, so they lie in [0, nc), nc <= nv;
// sorted values are permutations of [0, n).  Every loop is bounded by a segment length.
#include "nn_tree.h"

#define SP_THREADS 256
#define SP_HDR 256                                    // bytes at the start of the workspace: int64 results the host reads
static_assert(MVSDF_SP_H_WORDS * 8 <= SP_HDR, "the result words fit the header");
#define SP_CELL_BITS 21
#define SP_LAMBDA 1e-3

// words of the device counters (uint64 each)
enum { SP_C_ERR = 0, SP_C_DEG, SP_C_DUP, SP_C_PLACED, SP_C_NC, SP_C_NC2, SP_C_NF_OUT, SP_C_NV_OUT, SP_C_WORDS };

// ---- pass 1 ----
static __global__ __launch_bounds__(SP_THREADS) void k_sp_bbox_part(const float* __restrict__ v, long long nv, double* __restrict__ part, unsigned long long* cnt) {
    __shared__ double sh[6][SP_THREADS];
    const long long base = (long long)blockIdx.x * CH_CHUNK;
    double b[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int bad = 0;
    for (int q = 0; q < CH_ITEMS; ++q) {
        const long long i = base + (long long)q * SP_THREADS + threadIdx.x;
        if (i >= nv) break;
        const double p[3] = {(double)v[i * 3], (double)v[i * 3 + 1], (double)v[i * 3 + 2]};
        if (!ch_finite3(p)) {
            bad = 1;
            continue;
        }
        for (int a = 0; a < 3; ++a) {
            b[a] = fmin(b[a], p[a]);
            b[3 + a] = fmax(b[3 + a], p[a]);
        }
    }
    if (bad) atomicOr(cnt + SP_C_ERR, (unsigned long long)MVSDF_SP_ERR_FINITE);
    for (int a = 0; a < 6; ++a) sh[a][threadIdx.x] = b[a];
    __syncthreads();
    for (int d = SP_THREADS / 2; d; d >>= 1) {
        if ((int)threadIdx.x < d)
            for (int a = 0; a < 6; ++a)
                sh[a][threadIdx.x] = a < 3 ? fmin(sh[a][threadIdx.x], sh[a][threadIdx.x + d]) : fmax(sh[a][threadIdx.x], sh[a][threadIdx.x + d]);
        __syncthreads();
    }
    if (threadIdx.x < 6) part[blockIdx.x * 6 + threadIdx.x] = sh[threadIdx.x][0];
}

// box[0..2] = the low corner, box[3..5] = the high corner
static __global__ __launch_bounds__(64) void k_sp_bbox_final(const double* __restrict__ part, long long nb, double* __restrict__ box) {
    const int a = threadIdx.x;
    if (a >= 6) return;
    double r = a < 3 ? INFINITY : -INFINITY;
    for (long long b = 0; b < nb; ++b) r = a < 3 ? fmin(r, part[b * 6 + a]) : fmax(r, part[b * 6 + a]);
    box[a] = r;
}

static __global__ __launch_bounds__(SP_THREADS) void k_sp_face_check(const int* __restrict__ faces, long long ncorner, int nv, unsigned long long* cnt) {
    const long long c = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    const bool bad = c < ncorner && (faces[c] < 0 || faces[c] >= nv);
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(cnt + SP_C_ERR, (unsigned long long)MVSDF_SP_ERR_RANGE);
}

// ---- pass 2 ----
struct SpGrid {
    double o[3], cell;
    int sh0, sh1;                                     // key = i << sh0 | j << sh1 | k
};

__device__ __forceinline__ double sp_cell(double x, double o, double cell) { return floor((x - o) / cell); }

static __global__ __launch_bounds__(SP_THREADS) void k_sp_vkeys(const float* __restrict__ v, long long nv, SpGrid g, unsigned long long* __restrict__ key,
                                                               int* __restrict__ val) {
    const long long i = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (i >= nv) return;
    // the host checked the box: every index lies in [0, 2^21)
    const unsigned long long a = (unsigned long long)sp_cell((double)v[i * 3], g.o[0], g.cell);
    const unsigned long long b = (unsigned long long)sp_cell((double)v[i * 3 + 1], g.o[1], g.cell);
    const unsigned long long c = (unsigned long long)sp_cell((double)v[i * 3 + 2], g.o[2], g.cell);
    key[i] = a << g.sh0 | b << g.sh1 | c;
    val[i] = (int)i;
}

// ---- pass 3 ----
// hs[p] = sorted position p starts a segment; headv[v] = vertex v is the lowest member of its cell (headv pre-zeroed)
static __global__ __launch_bounds__(SP_THREADS) void k_sp_heads(const unsigned long long* __restrict__ key, const int* __restrict__ val, long long nv,
                                                               unsigned char* __restrict__ hs, unsigned char* __restrict__ headv) {
    const long long p = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (p >= nv) return;
    const bool h = p == 0 || key[p] != key[p - 1];
    hs[p] = h;
    if (h) headv[val[p]] = 1;
}

// segidx = the exclusive scan of hs; segstart[s] = the first sorted position of segment s; segstart[segments] = nv
static __global__ __launch_bounds__(SP_THREADS) void k_sp_segs(const unsigned char* __restrict__ hs, const long long* __restrict__ segidx, long long nv,
                                                              int* __restrict__ segstart) {
    const long long p = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (p >= nv) return;
    if (hs[p]) segstart[segidx[p]] = (int)p;
    if (p == nv - 1) segstart[segidx[p] + hs[p]] = (int)nv;         // the exclusive scan counts the heads before p: + its own = the segments
}

// vcl[v] = the cluster of vertex v (the rank of its segment's head among the head vertices); vsort = the sorted vertex ids (the sort buffers are reused);
// cseg[cluster] = its segment
static __global__ __launch_bounds__(SP_THREADS) void k_sp_assign(const unsigned char* __restrict__ hs, const long long* __restrict__ segidx,
                                                                const int* __restrict__ segstart, const int* __restrict__ val,
                                                                const long long* __restrict__ vrank, long long nv, int* __restrict__ vcl,
                                                                int* __restrict__ vsort, int* __restrict__ cseg) {
    const long long p = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (p >= nv) return;
    const long long s = segidx[p] + hs[p] - 1;                   // heads up to and including p, minus one
    const int cid = (int)vrank[val[segstart[s]]];
    const int v = val[p];
    vcl[v] = cid;
    vsort[p] = v;
    if (hs[p]) cseg[cid] = (int)s;
}

// ---- pass 4 ----
// the face's cluster triple, rotated smallest-first when its entries differ -> true when two of them are equal (degenerate)
__device__ __forceinline__ bool sp_triple(const int* __restrict__ faces, const int* __restrict__ vcl, long long f, int* r) {
    const int a = vcl[faces[f * 3]], b = vcl[faces[f * 3 + 1]], c = vcl[faces[f * 3 + 2]];
    if (a < b && a < c) {
        r[0] = a, r[1] = b, r[2] = c;
    } else if (b < a && b < c) {
        r[0] = b, r[1] = c, r[2] = a;
    } else {
        r[0] = c, r[1] = a, r[2] = b;
    }
    return a == b || b == c || a == c;
}

static __global__ __launch_bounds__(SP_THREADS) void k_sp_fkeys_lo(const int* __restrict__ faces, const int* __restrict__ vcl, long long nf,
                                                                  unsigned long long* __restrict__ key, int* __restrict__ val) {
    const long long f = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (f >= nf) return;
    int r[3];
    sp_triple(faces, vcl, f, r);
    key[f] = (unsigned long long)r[2];
    val[f] = (int)f;
}

static __global__ __launch_bounds__(SP_THREADS) void k_sp_fkeys_hi(const int* __restrict__ faces, const int* __restrict__ vcl, long long nf, int bits,
                                                                  const int* __restrict__ val, unsigned long long* __restrict__ key) {
    const long long q = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (q >= nf) return;
    int r[3];
    sp_triple(faces, vcl, val[q], r);
    key[q] = (unsigned long long)r[0] << bits | (unsigned long long)r[1];
}

// keep[f], used[cluster] (pre-zeroed; every writer stores 1), the degenerate and duplicate counts
static __global__ __launch_bounds__(SP_THREADS) void k_sp_dups(const int* __restrict__ faces, const int* __restrict__ vcl, long long nf, const int* __restrict__ val,
                                                              unsigned char* __restrict__ keep, unsigned char* __restrict__ used, unsigned long long* cnt) {
    const long long q = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    unsigned long long deg = 0, dup = 0;
    if (q < nf) {
        const int f = val[q];
        int r[3], s[3];
        deg = sp_triple(faces, vcl, f, r);
        if (!deg && q > 0) dup = !sp_triple(faces, vcl, val[q - 1], s) && s[0] == r[0] && s[1] == r[1] && s[2] == r[2];
        const bool k = !deg && !dup;
        keep[f] = k;
        if (k) used[r[0]] = used[r[1]] = used[r[2]] = 1;
    }
    for (int o = 32; o; o >>= 1) {
        deg += __shfl_xor(deg, o);
        dup += __shfl_xor(dup, o);
    }
    if ((threadIdx.x & 63) == 0) {
        if (deg) atomicAdd(cnt + SP_C_DEG, deg);
        if (dup) atomicAdd(cnt + SP_C_DUP, dup);
    }
}

// ---- pass 5 ----
static __global__ __launch_bounds__(SP_THREADS) void k_sp_ckeys(const int* __restrict__ faces, const int* __restrict__ vcl, long long ncorner,
                                                               unsigned long long* __restrict__ key, int* __restrict__ val) {
    const long long c = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (c >= ncorner) return;
    key[c] = (unsigned long long)vcl[faces[c]];
    val[c] = (int)c;
}

// corners [cbeg[cluster], cend[cluster]) of the sorted order belong to the cluster (both pre-zeroed: a cluster without corners keeps an empty range)
static __global__ __launch_bounds__(SP_THREADS) void k_sp_cseg(const unsigned long long* __restrict__ key, long long ncorner, int* __restrict__ cbeg,
                                                              int* __restrict__ cend) {
    const long long q = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (q >= ncorner) return;
    const unsigned long long k = key[q];
    if (q == 0 || key[q - 1] != k) cbeg[k] = (int)q;
    if (q == ncorner - 1 || key[q + 1] != k) cend[k] = (int)(q + 1);
}

struct SpMesh {
    const float *v, *n, *c;                           // n, c may be null
    const int* faces;
};

// one lane per used cluster: the definition's steps 3 to 5
static __global__ __launch_bounds__(SP_THREADS) void k_sp_cluster(SpMesh M, SpGrid g, int quadric, long long nc, const unsigned char* __restrict__ used,
                                                                 const int* __restrict__ cseg,
                                                                 const int* __restrict__ segstart, const int* __restrict__ vsort, const int* __restrict__ cbeg,
                                                                 const int* __restrict__ cend, const int* __restrict__ csort, float* __restrict__ cpos,
                                                                 float* __restrict__ cnrm, float* __restrict__ ccol, unsigned long long* cnt) {
    const long long cid = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    unsigned long long placed = 0;
    if (cid < nc && used[cid]) {
        const int s = cseg[cid], p0 = segstart[s], p1 = segstart[s + 1];
        double ps[3] = {0, 0, 0}, ns[3] = {0, 0, 0}, cs[3] = {0, 0, 0};
        for (int p = p0; p < p1; ++p) {
            const long long v = vsort[p];
            for (int a = 0; a < 3; ++a) {
                ps[a] += (double)M.v[v * 3 + a];
                if (M.n) ns[a] += (double)M.n[v * 3 + a];
                if (M.c) cs[a] += (double)M.c[v * 3 + a];
            }
        }
        const double count = (double)(p1 - p0);
        const double m[3] = {ps[0] / count, ps[1] / count, ps[2] / count};
        const double nl = sqrt((ns[0] * ns[0] + ns[1] * ns[1]) + ns[2] * ns[2]);
        for (int a = 0; a < 3; ++a) {
            cnrm[cid * 3 + a] = nl > 0.0 ? (float)(ns[a] / nl) : 0.0f;
            ccol[cid * 3 + a] = M.c ? (float)(cs[a] / count) : 0.0f;
        }
        double pos[3] = {m[0], m[1], m[2]};
        if (quadric) {
            double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0, b0 = 0, b1 = 0, b2 = 0;
            const int q1 = cend[cid];
            for (int q = cbeg[cid]; q < q1; ++q) {
                const long long f = csort[q] / 3;
                const float* u0 = M.v + (long long)M.faces[f * 3] * 3;
                const float* u1 = M.v + (long long)M.faces[f * 3 + 1] * 3;
                const float* u2 = M.v + (long long)M.faces[f * 3 + 2] * 3;
                const double x0 = u0[0], y0 = u0[1], z0 = u0[2];
                const double e1x = (double)u1[0] - x0, e1y = (double)u1[1] - y0, e1z = (double)u1[2] - z0;
                const double e2x = (double)u2[0] - x0, e2y = (double)u2[1] - y0, e2z = (double)u2[2] - z0;
                const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
                const double d = (nx * (x0 - m[0]) + ny * (y0 - m[1])) + nz * (z0 - m[2]);
                a00 += nx * nx;
                a01 += nx * ny;
                a02 += nx * nz;
                a11 += ny * ny;
                a12 += ny * nz;
                a22 += nz * nz;
                b0 += d * nx;
                b1 += d * ny;
                b2 += d * nz;
            }
            const double tr = (a00 + a11) + a22;
            if (tr > 0.0) {
                const double lam = SP_LAMBDA * tr;
                const double m00 = a00 + lam, m01 = a01, m02 = a02, m11 = a11 + lam, m12 = a12, m22 = a22 + lam;
                const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
                const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
                const double det = (m00 * c00 + m01 * c01) + m02 * c02;
                const double x[3] = {((c00 * b0 + c01 * b1) + c02 * b2) / det, ((c01 * b0 + c11 * b1) + c12 * b2) / det,
                                     ((c02 * b0 + c12 * b1) + c22 * b2) / det};
                const long long head = vsort[p0];
                bool same = true;
                double cand[3];
                for (int a = 0; a < 3; ++a) {
                    cand[a] = m[a] + x[a];
                    same = same && sp_cell(cand[a], g.o[a], g.cell) == sp_cell((double)M.v[head * 3 + a], g.o[a], g.cell);   // NaN: unequal
                }
                if (same) {
                    placed = 1;
                    for (int a = 0; a < 3; ++a) pos[a] = cand[a];
                }
            }
        }
        for (int a = 0; a < 3; ++a) cpos[cid * 3 + a] = (float)pos[a];
    }
    for (int o = 32; o; o >>= 1) placed += __shfl_xor(placed, o);
    if ((threadIdx.x & 63) == 0 && placed) atomicAdd(cnt + SP_C_PLACED, placed);
}

// ---- emit ----
static __global__ __launch_bounds__(SP_THREADS) void k_sp_emit_verts(long long nv, const unsigned char* __restrict__ used, const long long* __restrict__ urank,
                                                                    const float* __restrict__ cpos, const float* __restrict__ cnrm,
                                                                    const float* __restrict__ ccol, float* __restrict__ ov, float* __restrict__ on,
                                                                    float* __restrict__ oc, long long cap) {
    const long long cid = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (cid >= nv || !used[cid]) return;                          // used is zero beyond the clusters
    const long long row = urank[cid];
    if (row >= cap) return;
    for (int a = 0; a < 3; ++a) {
        ov[row * 3 + a] = cpos[cid * 3 + a];
        if (on) on[row * 3 + a] = cnrm[cid * 3 + a];
        if (oc) oc[row * 3 + a] = ccol[cid * 3 + a];
    }
}

static __global__ __launch_bounds__(SP_THREADS) void k_sp_emit_faces(const int* __restrict__ faces, long long nf, const unsigned char* __restrict__ keep,
                                                                    const long long* __restrict__ frank, const int* __restrict__ vcl,
                                                                    const long long* __restrict__ urank, int* __restrict__ of, long long cap) {
    const long long f = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (f >= nf || !keep[f]) return;
    const long long row = frank[f];
    if (row >= cap) return;
    for (int k = 0; k < 3; ++k) of[row * 3 + k] = (int)urank[vcl[faces[f * 3 + k]]];
}

// ---- workspace layout ----
struct SpLayout {
    long long n, nbv;                                             // items of the sort buffers; bbox workgroups
    ChSortLayout S;                                               // the radix sort's part of it (tmp also serves the other scans)
    size_t cnt, part, box, k0, k1, v0, v1, hs, headv, segidx, vrank, segstart, cseg, vcl, vsort, keep, frank, used, urank, cbeg, cend, cpos, cnrm, ccol, total;
};

// 1 <= nv <= INT_MAX, 1 <= 3 nf <= INT_MAX (the sort carries corner indices as int32)
static bool sp_layout(long long nv, long long nf, SpLayout* L) {
    if (nv < 1 || nf < 1 || nv > INT_MAX || nf > INT_MAX / 3) return false;
    const long long n = nv > 3 * nf ? nv : 3 * nf;
    L->n = n;
    L->nbv = mv_ceil_div(nv, CH_CHUNK);
    WsCursor c{SP_HDR};
    L->cnt = c.take(SP_C_WORDS * 8);
    L->part = c.take((size_t)L->nbv * 48);
    L->box = c.take(6 * 8);
    L->k0 = c.take((size_t)n * 8);
    L->k1 = c.take((size_t)n * 8);
    L->v0 = c.take((size_t)n * 4);
    L->v1 = c.take((size_t)n * 4);
    ch_sort_layout(n, n, c, &L->S);
    L->hs = c.take((size_t)nv);
    L->headv = c.take((size_t)nv);
    L->segidx = c.take((size_t)nv * 8);
    L->vrank = c.take((size_t)nv * 8);
    L->segstart = c.take((size_t)(nv + 1) * 4);
    L->cseg = c.take((size_t)nv * 4);
    L->vcl = c.take((size_t)nv * 4);
    L->vsort = c.take((size_t)nv * 4);
    L->keep = c.take((size_t)nf);
    L->frank = c.take((size_t)nf * 8);
    L->used = c.take((size_t)nv);
    L->urank = c.take((size_t)nv * 8);
    L->cbeg = c.take((size_t)nv * 4);
    L->cend = c.take((size_t)nv * 4);
    L->cpos = c.take((size_t)nv * 12);
    L->cnrm = c.take((size_t)nv * 12);
    L->ccol = c.take((size_t)nv * 12);
    L->total = c.o;
    return true;
}

static int sp_bits(long long x) {                                 // bits that hold 0 .. x
    int b = 0;
    while (x >> b) ++b;
    return b;
}

extern "C" {

size_t mvsdf_mesh_simplify_workspace_bytes(int64_t nv, int64_t nf) {
    SpLayout L;
    return sp_layout(nv, nf, &L) ? L.total : 0;
}

int mvsdf_mesh_simplify(const float* verts, const float* normals, const float* colors, const int32_t* faces, int64_t nv, int64_t nf, double cell,
                        const double* origin, int32_t quadric, int32_t counts_only, void* ws, size_t ws_bytes, void* stream) {
    const char* what = "mvsdf_mesh_simplify";
    SpLayout L;
    if (!verts || !faces || !ws || !sp_layout(nv, nf, &L)) return mv_fail(-1, "mvsdf_mesh_simplify: bad arguments");
    if (!(cell > 0.0) || !isfinite(cell)) return mv_fail(-1, "mvsdf_mesh_simplify: cell must be finite and > 0");
    if (origin && !(isfinite(origin[0]) && isfinite(origin[1]) && isfinite(origin[2]))) return mv_fail(-1, "mvsdf_mesh_simplify: non-finite origin");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_mesh_simplify: workspace too small (mvsdf_mesh_simplify_workspace_bytes)");
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    const long long V = nv, F = nf, C = 3 * nf;
    unsigned long long* cnt = (unsigned long long*)(w + L.cnt);
    long long* tot = (long long*)cnt;                             // the scans' totals land in the counter words
    unsigned long long* k[2] = {(unsigned long long*)(w + L.k0), (unsigned long long*)(w + L.k1)};
    int* v[2] = {(int*)(w + L.v0), (int*)(w + L.v1)};
    unsigned char* hs = (unsigned char*)(w + L.hs);
    unsigned char* headv = (unsigned char*)(w + L.headv);
    long long* segidx = (long long*)(w + L.segidx);
    long long* vrank = (long long*)(w + L.vrank);
    int* segstart = (int*)(w + L.segstart);
    int* cseg = (int*)(w + L.cseg);
    int* vcl = (int*)(w + L.vcl);
    int* vsort = (int*)(w + L.vsort);
    unsigned char* keep = (unsigned char*)(w + L.keep);
    unsigned char* used = (unsigned char*)(w + L.used);
    void* tmp = w + L.S.tmp;
    const unsigned gv = mv_grid(V, SP_THREADS), gf = mv_grid(F, SP_THREADS), gc = mv_grid(C, SP_THREADS);
    long long hdr[MVSDF_SP_H_WORDS] = {};
    int rc;
    // ---- 1: box, finite check, id check ----
    if ((rc = mv_check(hipMemsetAsync(cnt, 0, SP_C_WORDS * 8, s), what))) return rc;
    hipLaunchKernelGGL(k_sp_bbox_part, dim3((unsigned)L.nbv), dim3(SP_THREADS), 0, s, verts, V, (double*)(w + L.part), cnt);
    hipLaunchKernelGGL(k_sp_bbox_final, dim3(1), dim3(64), 0, s, (const double*)(w + L.part), L.nbv, (double*)(w + L.box));
    hipLaunchKernelGGL(k_sp_face_check, dim3(gc), dim3(SP_THREADS), 0, s, faces, C, (int)V, cnt);
    if ((rc = mv_check(hipGetLastError(), what))) return rc;
    double box[6];
    unsigned long long e = 0;
    if ((rc = mv_check(hipMemcpyAsync(box, w + L.box, sizeof(box), hipMemcpyDeviceToHost, s), what))) return rc;
    if ((rc = mv_read(&e, cnt + SP_C_ERR, 8, s, what))) return rc;
    SpGrid g;
    g.cell = cell;
    int bits[3] = {0, 0, 0};
    if (!e)
        for (int a = 0; a < 3; ++a) {
            g.o[a] = origin ? origin[a] : box[a];
            // the index is monotone in the coordinate: the box's corners bound every vertex's
            const double lo = floor((box[a] - g.o[a]) / cell), hi = floor((box[3 + a] - g.o[a]) / cell);
            if (!(lo >= 0.0) || !(hi < (double)(1 << SP_CELL_BITS))) {
                e |= MVSDF_SP_ERR_CELLS;
                break;
            }
            bits[a] = sp_bits((long long)hi);
        }
    if (e) {
        hdr[MVSDF_SP_H_ERR] = (long long)e;
        return mv_write_header(w, hdr, MVSDF_SP_H_WORDS, s, what);
    }
    g.sh1 = bits[2];
    g.sh0 = bits[2] + bits[1];
    // ---- 2: the vertices by cell ----
    hipLaunchKernelGGL(k_sp_vkeys, dim3(gv), dim3(SP_THREADS), 0, s, verts, V, g, k[0], v[0]);
    int cur = ch_radix_sort(k, v, V, bits[0] + bits[1] + bits[2], w, L.S, s);
    // ---- 3: segments and clusters ----
    if ((rc = mv_check(hipMemsetAsync(headv, 0, (size_t)V, s), what))) return rc;
    hipLaunchKernelGGL(k_sp_heads, dim3(gv), dim3(SP_THREADS), 0, s, (const unsigned long long*)k[cur], (const int*)v[cur], V, hs, headv);
    mv_scan((const unsigned char*)hs, V, segidx, tmp, tot + SP_C_NC, s);
    mv_scan((const unsigned char*)headv, V, vrank, tmp, tot + SP_C_NC2, s);
    hipLaunchKernelGGL(k_sp_segs, dim3(gv), dim3(SP_THREADS), 0, s, (const unsigned char*)hs, (const long long*)segidx, V, segstart);
    hipLaunchKernelGGL(k_sp_assign, dim3(gv), dim3(SP_THREADS), 0, s, (const unsigned char*)hs, (const long long*)segidx, (const int*)segstart,
                       (const int*)v[cur], (const long long*)vrank, V, vcl, vsort, cseg);
    if ((rc = mv_check(hipGetLastError(), what))) return rc;
    long long nc = 0;
    if ((rc = mv_read(&nc, tot + SP_C_NC, 8, s, what))) return rc;
    if (nc < 1 || nc > V) return mv_fail(-2, "mvsdf_mesh_simplify: cluster count out of range");
    const int b = sp_bits(nc - 1);
    // ---- 4: duplicate faces by two stable sorts, kept faces, used clusters ----
    hipLaunchKernelGGL(k_sp_fkeys_lo, dim3(gf), dim3(SP_THREADS), 0, s, faces, (const int*)vcl, F, k[0], v[0]);
    cur = ch_radix_sort(k, v, F, b, w, L.S, s);
    hipLaunchKernelGGL(k_sp_fkeys_hi, dim3(gf), dim3(SP_THREADS), 0, s, faces, (const int*)vcl, F, b, (const int*)v[cur], k[cur]);
    {
        unsigned long long* k2[2] = {k[cur], k[cur ^ 1]};
        int* v2[2] = {v[cur], v[cur ^ 1]};
        cur ^= ch_radix_sort(k2, v2, F, 2 * b, w, L.S, s);
    }
    if ((rc = mv_check(hipMemsetAsync(used, 0, (size_t)V, s), what))) return rc;
    hipLaunchKernelGGL(k_sp_dups, dim3(gf), dim3(SP_THREADS), 0, s, faces, (const int*)vcl, F, (const int*)v[cur], keep, used, cnt);
    mv_scan((const unsigned char*)keep, F, (long long*)(w + L.frank), tmp, tot + SP_C_NF_OUT, s);
    mv_scan((const unsigned char*)used, nc, (long long*)(w + L.urank), tmp, tot + SP_C_NV_OUT, s);
    // ---- 5: the corners by cluster, the cluster walk ----
    if (!counts_only) {
        hipLaunchKernelGGL(k_sp_ckeys, dim3(gc), dim3(SP_THREADS), 0, s, faces, (const int*)vcl, C, k[0], v[0]);
        cur = ch_radix_sort(k, v, C, b, w, L.S, s);
        if ((rc = mv_check(hipMemsetAsync(w + L.cbeg, 0, (size_t)nc * 4, s), what))) return rc;
        if ((rc = mv_check(hipMemsetAsync(w + L.cend, 0, (size_t)nc * 4, s), what))) return rc;
        hipLaunchKernelGGL(k_sp_cseg, dim3(gc), dim3(SP_THREADS), 0, s, (const unsigned long long*)k[cur], C, (int*)(w + L.cbeg), (int*)(w + L.cend));
        const SpMesh M = {verts, normals, colors, faces};
        hipLaunchKernelGGL(k_sp_cluster, dim3(mv_grid(nc, SP_THREADS)), dim3(SP_THREADS), 0, s, M, g, (int)(quadric != 0), nc, (const unsigned char*)used,
                           (const int*)cseg, (const int*)segstart, (const int*)vsort, (const int*)(w + L.cbeg),
                           (const int*)(w + L.cend), (const int*)v[cur], (float*)(w + L.cpos), (float*)(w + L.cnrm), (float*)(w + L.ccol), cnt);
    }
    if ((rc = mv_check(hipGetLastError(), what))) return rc;
    unsigned long long res[SP_C_WORDS];
    if ((rc = mv_read(res, cnt, sizeof(res), s, what))) return rc;
    hdr[MVSDF_SP_H_CLUSTERS] = nc;
    hdr[MVSDF_SP_H_VERTS] = (long long)res[SP_C_NV_OUT];
    hdr[MVSDF_SP_H_FACES] = (long long)res[SP_C_NF_OUT];
    hdr[MVSDF_SP_H_DEGENERATE] = (long long)res[SP_C_DEG];
    hdr[MVSDF_SP_H_DUPLICATES] = (long long)res[SP_C_DUP];
    hdr[MVSDF_SP_H_PLACED] = (long long)res[SP_C_PLACED];
    hdr[MVSDF_SP_H_ERR] = (long long)res[SP_C_ERR];
    return mv_write_header(w, hdr, MVSDF_SP_H_WORDS, s, what);
}

int mvsdf_mesh_simplify_emit(const int32_t* faces, int64_t nv, int64_t nf, void* ws, size_t ws_bytes, float* out_verts, float* out_normals,
                             float* out_colors, int32_t* out_faces, int64_t nv_cap, int64_t nf_cap, void* stream) {
    SpLayout L;
    if (!faces || !ws || !out_verts || !out_faces || nv_cap < 0 || nf_cap < 0 || !sp_layout(nv, nf, &L))
        return mv_fail(-1, "mvsdf_mesh_simplify_emit: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_mesh_simplify_emit: workspace too small (mvsdf_mesh_simplify_workspace_bytes)");
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_sp_emit_verts, dim3(mv_grid(nv, SP_THREADS)), dim3(SP_THREADS), 0, s, (long long)nv, (const unsigned char*)(w + L.used),
                       (const long long*)(w + L.urank), (const float*)(w + L.cpos), (const float*)(w + L.cnrm), (const float*)(w + L.ccol), out_verts,
                       out_normals, out_colors, (long long)nv_cap);
    hipLaunchKernelGGL(k_sp_emit_faces, dim3(mv_grid(nf, SP_THREADS)), dim3(SP_THREADS), 0, s, faces, (long long)nf, (const unsigned char*)(w + L.keep),
                       (const long long*)(w + L.frank), (const int*)(w + L.vcl), (const long long*)(w + L.urank), out_faces, (long long)nf_cap);
    return mv_check(hipGetLastError(), "mvsdf_mesh_simplify_emit");
}

}  // extern "C"
