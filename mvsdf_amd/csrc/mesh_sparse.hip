// mesh_sparse.hip -- sparse marching cubes over surface bricks: the dense extractor's mesh (mesh_kernels.hip) from the SDF evaluated only in blocks of
// B^3 cells that can hold surface.  The contract (lattice, seeds, closure, output) is stated in mvsdf_amd/mesh.py and restated in numpy in
// tests/smc_ref.py; the marching-cubes formulas are mesh_common.h's, shared with the dense path.
//
// Blocks: nb = ceil((N - 1) / B) per axis; block b holds the cells c with c_a / B = b_a, its corners lie at lattice indices b_a B and
// min((b_a + 1) B, N - 1).  State per block (int32 map, nb^3): 0 inactive, 1 flagged, s + 2 = active in brick slot s.  A brick holds the block's
// (B + 3)^3 values: lattice indices b_a B - 1 .. b_a B + B + 1, clamped to the volume (the one-point halo the central differences need).
//
// Host flow (mesh.py): coarse points -> seed (+ compaction: slots for the seeds) -> per round: brick points of the new slots, evaluated by the
// caller, then the closure test on their faces (+ compaction of the newly flagged blocks) until a round flags nothing -> count -> emit.
//
// Output order without sorting: a grid point (and the vertices on its edges) is owned by block min(p_a / B, nb - 1) on every axis, a cell by
// its block.  The active blocks in linear order (sblk) are cut into rows (block, i_l, j_l) of R = B + 1 points along k; the row ranked
//     rank = s_i R^2 + i_l n_i R + (s_j - s_i) R + j_l n_j + (r - s_j)
// (r = the block's place in sblk, [s_i, s_i + n_i) = the active blocks of its i-slab, [s_j, s_j + n_j) = those of its (i, j)-column) holds points
// and cells in the dense path's (i, j, k) order, so the rows in rank order carry the vertices and faces in the dense order.  Counting, scanning
// and emitting rows is the dense path's ballot / popcount structure (block_excl, k_mesh_scan) over these items.
// Face vertex ids come from a brick-local id map (R^3 int32 per slot: each owned point's first vertex id).  The closure guarantees that every
// edge a kept face uses is owned by an active block.
#include "mesh_common.h"

#define SMC_THREADS 256

// the workspace header is MVSDF_SMC_H_*; k_mesh_scan leaves three totals from _COUNT on (compactions) and from _VERTS on (the count pass)
static_assert(MVSDF_SMC_H_COUNT + 3 <= MVSDF_SMC_H_BAD && MVSDF_SMC_H_FACES == MVSDF_SMC_H_VERTS + 1 && MVSDF_SMC_H_NEGATIVE == MVSDF_SMC_H_VERTS + 2 &&
                  MVSDF_SMC_H_WORDS * 8 <= MESH_HDR,
              "k_mesh_scan's totals are header words");

struct SmcGrid {
    long long n;                // lattice points per axis
    int B, nb, P, R;            // block edge in cells, blocks per axis, brick edge (B + 3), row length (B + 1)
    float level;
};

__device__ __forceinline__ void blk_ijk(long long b, int nb, int* q) {
    q[2] = (int)(b % nb);
    b /= nb;
    q[1] = (int)(b % nb);
    q[0] = (int)(b / nb);
}

__device__ __forceinline__ long long blk_lin(const int* q, int nb) { return ((long long)q[0] * nb + q[1]) * nb + q[2]; }

// the values of one brick, read by lattice index (mesh_common.h's accessor)
struct BrickVal {
    const float* p;
    long long lo[3];            // the block's first lattice index per axis (b_a B)
    int P;
    __device__ __forceinline__ float operator()(long long i, long long j, long long k) const {
        return p[((i - lo[0] + 1) * P + (j - lo[1] + 1)) * P + (k - lo[2] + 1)];
    }
};

__device__ __forceinline__ BrickVal brick_at(const float* vals, const SmcGrid& g, long long slot, const int* q) {
    BrickVal v;
    v.p = vals + slot * (long long)g.P * g.P * g.P;
    for (int a = 0; a < 3; ++a) v.lo[a] = (long long)q[a] * g.B;
    v.P = g.P;
    return v;
}

// ---- the coarse lattice: point t of the (nb + 1)^3 block corners (k fastest) at lattice indices min(q B, N - 1) ----
__global__ __launch_bounds__(SMC_THREADS) void k_smc_coarse_points(const float* __restrict__ ax, SmcGrid g, long long start, long long count,
                                                                   float* __restrict__ pts) {
    const long long t = (long long)blockIdx.x * SMC_THREADS + threadIdx.x;
    if (t >= count) return;
    const long long p = start + t, m = g.nb + 1;
    const long long q[3] = {p / (m * m), (p / m) % m, p % m};
    for (int c = 0; c < 3; ++c) pts[t * 3 + c] = ax[min(q[c] * g.B, g.n - 1)];
}

// ---- seeds: a block whose corners lie on both sides of the level, or one of them within tol of it ----
__global__ __launch_bounds__(SMC_THREADS) void k_smc_seed(const float* __restrict__ cv, SmcGrid g, float tol, int* __restrict__ map, long long nblk,
                                                          unsigned long long* __restrict__ hdr) {
    const long long b = (long long)blockIdx.x * SMC_THREADS + threadIdx.x;
    if (b >= nblk) return;
    int q[3];
    blk_ijk(b, g.nb, q);
    const long long m = g.nb + 1;
    bool in_any = false, out_any = false, near = false, bad = false;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float v = cv[((q[0] + (c & 1)) * m + q[1] + (c >> 1 & 1)) * m + q[2] + (c >> 2 & 1)];
        bad |= !isfinite(v);
        const bool in = v < g.level;
        in_any |= in;
        out_any |= !in;
        near |= fabsf(v - g.level) <= tol;
    }
    map[b] = (in_any && out_any) || near ? 1 : 0;
    if (bad) atomicOr(hdr + MVSDF_SMC_H_BAD, 1ull);
}

// ---- compaction: per-workgroup counts of flagged (mode 0: state 1) or active (mode 1: state >= 2) blocks ----
__global__ __launch_bounds__(MESH_THREADS) void k_smc_flag_count(const int* __restrict__ map, long long nblk, int mode, int* __restrict__ bc) {
    __shared__ int s_w[MESH_THREADS / 64];
    long long run = 0;
    for (int r = 0; r < MESH_ROUNDS; ++r) {
        const long long x = (long long)blockIdx.x * MESH_CHUNK + r * MESH_THREADS + threadIdx.x;
        const int st = x < nblk ? map[x] : 0;
        block_excl(mode ? st >= 2 : st == 1, 1, s_w, run);
    }
    if (threadIdx.x == 0) bc[blockIdx.x] = (int)run;
}

// mode 0: the flagged blocks, in linear order, take slots base, base + 1, ... (list[slot] = block, state = slot + 2);
// mode 1: sblk = the active blocks in linear order
__global__ __launch_bounds__(MESH_THREADS) void k_smc_compact(int* __restrict__ map, long long nblk, int mode, const long long* __restrict__ off, long long base,
                                                             int* __restrict__ list, int* __restrict__ sblk) {
    __shared__ int s_w[MESH_THREADS / 64];
    long long run = off[blockIdx.x];
    for (int r = 0; r < MESH_ROUNDS; ++r) {
        const long long x = (long long)blockIdx.x * MESH_CHUNK + r * MESH_THREADS + threadIdx.x;
        const int st = x < nblk ? map[x] : 0;
        const bool sel = mode ? st >= 2 : st == 1;
        const long long id = block_excl(sel, 1, s_w, run);
        if (!sel) continue;
        if (mode == 0) {
            list[base + id] = (int)x;
            map[x] = (int)(base + id + 2);
        } else {
            sblk[id] = (int)x;
        }
    }
}

// ---- brick points: item t = slot * P^3 + local (k fastest), lattice index b_a B - 1 + local_a clamped to [0, N - 1] ----
__global__ __launch_bounds__(SMC_THREADS) void k_smc_brick_points(const float* __restrict__ ax, SmcGrid g, const int* __restrict__ list, long long start,
                                                                  long long count, float* __restrict__ pts) {
    const long long t = (long long)blockIdx.x * SMC_THREADS + threadIdx.x;
    if (t >= count) return;
    const long long P = g.P, P3 = P * P * P, p = start + t;
    const long long slot = p / P3, l = p - slot * P3;
    int q[3];
    blk_ijk(list[slot], g.nb, q);
    const long long loc[3] = {l / (P * P), (l / P) % P, l % P};
    for (int c = 0; c < 3; ++c) {
        const long long x = (long long)q[c] * g.B - 1 + loc[c];
        pts[t * 3 + c] = ax[x < 0 ? 0 : (x > g.n - 1 ? g.n - 1 : x)];
    }
}

// ---- closure: item (slot, face, row) of the bricks [slot0, slot0 + count).  An inactive neighbour across the face is flagged when a grid edge
// lying in the shared face crosses the level.  Thread v walks the face's row v along its first in-face axis u, testing the u-edges and the
// edges to row v + 1.  Flag stores are idempotent (several faces may flag one block); a per-wave sum of them goes to the header. ----
__global__ __launch_bounds__(SMC_THREADS) void k_smc_closure(const float* __restrict__ vals, SmcGrid g, const int* __restrict__ list, int* map, long long slot0,
                                                             long long count, unsigned long long* __restrict__ hdr) {
    const long long t = (long long)blockIdx.x * SMC_THREADS + threadIdx.x;
    const long long per = 6ll * g.R;
    bool hit = false;
    if (t < count * per) {
        const long long slot = slot0 + t / per;
        const int rem = (int)(t % per), f = rem / g.R, v = rem % g.R;
        const int d = f >> 1, up = f & 1;
        int q[3];
        blk_ijk(list[slot], g.nb, q);
        int nq[3] = {q[0], q[1], q[2]};
        nq[d] += up ? 1 : -1;
        if (nq[d] >= 0 && nq[d] < g.nb) {
            const long long nbl = blk_lin(nq, g.nb);
            if (map[nbl] == 0) {
                const int u = d == 0 ? 1 : 0, w = d == 2 ? 1 : 2;          // the in-face axes
                long long lo[3], hi[3];
                for (int a = 0; a < 3; ++a) {
                    lo[a] = (long long)q[a] * g.B;
                    hi[a] = min(lo[a] + g.B, g.n - 1);
                }
                long long p[3];
                p[d] = up ? hi[d] : lo[d];
                p[w] = lo[w] + v;
                if (p[w] <= hi[w]) {
                    const BrickVal bv = brick_at(vals, g, slot, q);
                    for (p[u] = lo[u]; p[u] <= hi[u] && !hit; ++p[u]) {
                        const bool in = bv(p[0], p[1], p[2]) < g.level;
                        long long e[3] = {p[0], p[1], p[2]};
                        if (p[u] < hi[u]) {
                            e[u] += 1;
                            hit |= in != (bv(e[0], e[1], e[2]) < g.level);
                            e[u] -= 1;
                        }
                        if (p[w] < hi[w]) {
                            e[w] += 1;
                            hit |= in != (bv(e[0], e[1], e[2]) < g.level);
                        }
                    }
                    if (hit) map[nbl] = 1;
                }
            }
        }
    }
    const unsigned long long m = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(hdr + MVSDF_SMC_H_STORES, (unsigned long long)__popcll(m));
}

// ---- row metadata: per place r of sblk, the active blocks of its i-slab [x, y) and of its (i, j)-column [z, w) ----
__device__ __forceinline__ int lower_bound_i(const int* __restrict__ a, int n, long long key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(SMC_THREADS) void k_smc_meta(const int* __restrict__ sblk, int nact, int nb, int4* __restrict__ meta) {
    const int r = blockIdx.x * SMC_THREADS + threadIdx.x;
    if (r >= nact) return;
    int q[3];
    blk_ijk(sblk[r], nb, q);
    const long long nb2 = (long long)nb * nb, col = (long long)q[0] * nb + q[1];
    meta[r] = make_int4(lower_bound_i(sblk, nact, q[0] * nb2), lower_bound_i(sblk, nact, (q[0] + 1) * nb2), lower_bound_i(sblk, nact, col * nb),
                        lower_bound_i(sblk, nact, (col + 1) * nb));
}

// one row: its block (place r in sblk), the row's lattice (i, j), its first k, and the extents of the block's owned points and cells
struct SmcRow {
    bool valid;                 // the row holds owned points
    long long slot, i, j, k0;
    int q[3], il, jl, ep, ec;   // ep / ec: owned points / cells along k
    bool cells;                 // the row holds cells (i_l, j_l below the cell extents)
};

__device__ __forceinline__ SmcRow smc_row(long long rank, const SmcGrid& g, const int* __restrict__ map, const int* __restrict__ sblk,
                                          const int4* __restrict__ meta) {
    SmcRow w;
    const long long R = g.R, R2 = R * R;
    const int4 m0 = meta[rank / R2];
    const long long nslab = m0.y - m0.x, rr = rank - m0.x * R2;
    w.il = (int)(rr / (nslab * R));
    const long long rr2 = rr - w.il * nslab * R;
    const int4 m1 = meta[m0.x + rr2 / R];
    const long long ncol = m1.w - m1.z, rr3 = rr2 - (m1.z - m0.x) * R;
    w.jl = (int)(rr3 / ncol);
    const int r = (int)(m1.z + rr3 % ncol);
    const int blk = sblk[r];
    blk_ijk(blk, g.nb, w.q);
    w.slot = map[blk] - 2;
    int ep[3], ec[3];
    for (int a = 0; a < 3; ++a) {
        const long long lo = (long long)w.q[a] * g.B;
        ep[a] = w.q[a] == g.nb - 1 ? (int)(g.n - lo) : g.B;
        ec[a] = (int)min((long long)g.B, g.n - 1 - lo);
    }
    w.i = (long long)w.q[0] * g.B + w.il;
    w.j = (long long)w.q[1] * g.B + w.jl;
    w.k0 = (long long)w.q[2] * g.B;
    w.valid = w.il < ep[0] && w.jl < ep[1];
    w.cells = w.il < ec[0] && w.jl < ec[1];
    w.ep = ep[2];
    w.ec = ec[2];
    return w;
}

__device__ __forceinline__ int row_vertices(const SmcRow& w, const BrickVal& bv, const long long* nn, float level) {
    int nv = 0;
    if (!w.valid) return 0;
    for (int kl = 0; kl < w.ep; ++kl) {
        const long long k = w.k0 + kl;
        nv += __popc(mc_point_edges(bv, nn, w.i, w.j, k, bv(w.i, w.j, k) < level, level));
    }
    return nv;
}

__device__ __forceinline__ int row_faces(const SmcRow& w, const BrickVal& bv, float level) {
    int nt = 0;
    if (!w.cells) return 0;
    for (int kl = 0; kl < w.ec; ++kl) nt += mc_ntri(mc_cube_index(bv, w.i, w.j, w.k0 + kl, level));
    return nt;
}

// ---- count: vertices and faces per workgroup of rows ----
__global__ __launch_bounds__(MESH_THREADS) void k_smc_count(const float* __restrict__ vals, SmcGrid g, const int* __restrict__ map, const int* __restrict__ sblk,
                                                           const int4* __restrict__ meta, long long nrows, int vbits, int fbits, int* __restrict__ bv,
                                                           int* __restrict__ bf) {
    __shared__ int s_w[MESH_THREADS / 64];
    const long long nn[3] = {g.n, g.n, g.n};
    long long rv = 0, rf = 0;
    for (int r = 0; r < MESH_ROUNDS; ++r) {
        const long long rank = (long long)blockIdx.x * MESH_CHUNK + r * MESH_THREADS + threadIdx.x;
        int nv = 0, nt = 0;
        if (rank < nrows) {
            const SmcRow w = smc_row(rank, g, map, sblk, meta);
            const BrickVal b = brick_at(vals, g, w.slot, w.q);
            nv = row_vertices(w, b, nn, g.level);
            nt = row_faces(w, b, g.level);
        }
        block_excl(nv, vbits, s_w, rv);
        block_excl(nt, fbits, s_w, rf);
    }
    if (threadIdx.x == 0) {
        bv[blockIdx.x] = (int)rv;
        bf[blockIdx.x] = (int)rf;
    }
}

// ---- emit, vertices: every owned point's first vertex id into the brick-local id map, and the vertices of its crossing edges ----
__global__ __launch_bounds__(MESH_THREADS) void k_smc_vertices(const float* __restrict__ vals, SmcGrid g, McGeom gm, const int* __restrict__ map,
                                                              const int* __restrict__ sblk, const int4* __restrict__ meta, long long nrows, int vbits,
                                                              const long long* __restrict__ ov, int* __restrict__ idmap, float* __restrict__ verts,
                                                              float* __restrict__ normals, long long nv_cap) {
    __shared__ int s_w[MESH_THREADS / 64];
    const long long nn[3] = {g.n, g.n, g.n}, R = g.R;
    long long run = ov[blockIdx.x];
    for (int r = 0; r < MESH_ROUNDS; ++r) {
        const long long rank = (long long)blockIdx.x * MESH_CHUNK + r * MESH_THREADS + threadIdx.x;
        SmcRow w;
        w.valid = false;
        BrickVal b;
        int nv = 0;
        if (rank < nrows) {
            w = smc_row(rank, g, map, sblk, meta);
            b = brick_at(vals, g, w.slot, w.q);
            nv = row_vertices(w, b, nn, g.level);
        }
        long long id = block_excl(nv, vbits, s_w, run);
        if (!w.valid) continue;
        int* ids = idmap + (w.slot * R + w.il) * R * R + w.jl * R;
        for (int kl = 0; kl < w.ep; ++kl) {
            const long long gp[3] = {w.i, w.j, w.k0 + kl};
            const float x = b(gp[0], gp[1], gp[2]);
            const int bits = mc_point_edges(b, nn, gp[0], gp[1], gp[2], x < g.level, g.level);
            ids[kl] = (int)id;
            for (int a = 0; a < 3; ++a) {
                if (!(bits >> a & 1)) continue;
                if (id < nv_cap) mc_vertex(b, nn, gp, a, x, g.level, gm, verts + id * 3, normals + id * 3);
                ++id;
            }
        }
    }
}

// vertex id of cube edge e of the cell at c: the owner point's block (min(q_a / B, nb - 1)), its slot, its id-map entry plus the owner's crossing
// edges along lower axes; -1 (and the error flag) if the owner's block is not active
__device__ __forceinline__ int smc_edge_vertex(const float* __restrict__ vals, const SmcGrid& g, const int* __restrict__ map, const int* __restrict__ idmap,
                                               const long long* c, int e, unsigned long long* __restrict__ hdr) {
    const long long nn[3] = {g.n, g.n, g.n}, R = g.R;
    long long q[3] = {c[0], c[1], c[2]};
    const int a = mc_edge_owner(e, q);
    int ob[3];
    for (int x = 0; x < 3; ++x) ob[x] = (int)min(q[x] / g.B, (long long)g.nb - 1);
    const int st = map[blk_lin(ob, g.nb)];
    if (st < 2) {
        atomicOr(hdr + MVSDF_SMC_H_OWNER, 1ull);
        return -1;
    }
    const long long slot = st - 2;
    const BrickVal b = brick_at(vals, g, slot, ob);
    const int bits = mc_point_edges(b, nn, q[0], q[1], q[2], b(q[0], q[1], q[2]) < g.level, g.level);
    const long long l[3] = {q[0] - b.lo[0], q[1] - b.lo[1], q[2] - b.lo[2]};
    return idmap[((slot * R + l[0]) * R + l[1]) * R + l[2]] + __popc(bits & ((1 << a) - 1));
}

// ---- emit, faces: cells in row order, each cell's triangles in table order ----
__global__ __launch_bounds__(MESH_THREADS) void k_smc_faces(const float* __restrict__ vals, SmcGrid g, const int* __restrict__ map, const int* __restrict__ sblk,
                                                           const int4* __restrict__ meta, long long nrows, int fbits, const long long* __restrict__ of,
                                                           const int* __restrict__ idmap, int* __restrict__ faces, long long nf_cap,
                                                           unsigned long long* __restrict__ hdr) {
    __shared__ int s_w[MESH_THREADS / 64];
    long long run = of[blockIdx.x];
    for (int r = 0; r < MESH_ROUNDS; ++r) {
        const long long rank = (long long)blockIdx.x * MESH_CHUNK + r * MESH_THREADS + threadIdx.x;
        SmcRow w;
        w.cells = false;
        BrickVal b;
        int nt = 0;
        if (rank < nrows) {
            w = smc_row(rank, g, map, sblk, meta);
            b = brick_at(vals, g, w.slot, w.q);
            nt = row_faces(w, b, g.level);
        }
        long long fid = block_excl(nt, fbits, s_w, run);
        if (!w.cells) continue;
        for (int kl = 0; kl < w.ec && fid < nf_cap; ++kl) {
            const long long c[3] = {w.i, w.j, w.k0 + kl};
            const int ci = mc_cube_index(b, c[0], c[1], c[2], g.level);
            const int ntri = mc_ntri(ci);
            for (int t = 0; t < ntri; ++t, ++fid) {
                if (fid >= nf_cap) break;
                const int base = (mc_tri_offset[ci] + t) * 3;
                for (int s = 0; s < 3; ++s) faces[fid * 3 + s] = smc_edge_vertex(vals, g, map, idmap, c, mc_tri_edges[base + s], hdr);
            }
        }
    }
}

// ---- workspace layouts (every region 256-byte aligned) ----
static inline int smc_bits(long long x) {
    int b = 0;
    while ((1ll << b) <= x) ++b;
    return b;
}

struct SmcLayout {
    SmcGrid g;
    long long nblk, nwg;
    size_t map, list, sblk, meta, bc, bo, total;
};

// false: N < 3, B < 2, or a lattice whose blocks, bricks or rows the kernels cannot index
static bool smc_layout(int64_t n, int64_t block, SmcLayout* L) {
    if (n < 3 || block < 2 || n > (1ll << 24) || block > 1024) return false;
    const long long nb = (n - 1 + block - 1) / block;
    if (nb > 1290 || nb * nb * nb > INT_MAX - 2) return false;      // block ids and slots + 2 are int32
    L->g.n = n;
    L->g.B = (int)block;
    L->g.nb = (int)nb;
    L->g.P = (int)block + 3;
    L->g.R = (int)block + 1;
    L->g.level = 0.0f;
    L->nblk = nb * nb * nb;
    L->nwg = mv_ceil_div(L->nblk, MESH_CHUNK);
    WsCursor c{MESH_HDR};
    L->map = c.take((size_t)L->nblk * 4);
    L->list = c.take((size_t)L->nblk * 4);
    L->sblk = c.take((size_t)L->nblk * 4);
    L->meta = c.take((size_t)L->nblk * 16);
    L->bc = c.take((size_t)L->nwg * 4);
    L->bo = c.take((size_t)L->nwg * 8);
    L->total = c.o;
    return true;
}

struct SmcEmitLayout {
    long long nrows, nwg;
    size_t idmap, bv, bf, ov, of, total;
};

static bool smc_emit_layout(const SmcLayout& L, int64_t nact, SmcEmitLayout* E) {
    if (nact < 1 || nact > L.nblk) return false;
    const long long R = L.g.R;
    E->nrows = nact * R * R;
    E->nwg = mv_ceil_div(E->nrows, MESH_CHUNK);
    if (E->nwg > INT_MAX) return false;
    WsCursor c{0};
    E->idmap = c.take((size_t)nact * R * R * R * 4);
    E->bv = c.take((size_t)E->nwg * 4);
    E->bf = c.take((size_t)E->nwg * 4);
    E->ov = c.take((size_t)E->nwg * 8);
    E->of = c.take((size_t)E->nwg * 8);
    E->total = c.o;
    return true;
}

// the flagged blocks (state 1) take the slots base, base + 1, ... in linear order; the count lands in the header
static void smc_compact(const SmcLayout& L, char* w, int mode, long long base, hipStream_t s) {
    int* map = (int*)(w + L.map);
    hipLaunchKernelGGL(k_smc_flag_count, dim3((unsigned)L.nwg), dim3(MESH_THREADS), 0, s, (const int*)map, L.nblk, mode, (int*)(w + L.bc));
    hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(MESH_SCAN_THREADS), 0, s, (const int*)(w + L.bc), (const int*)nullptr, (int)L.nwg, (long long*)(w + L.bo),
                       (long long*)nullptr, (long long*)w + MVSDF_SMC_H_COUNT);
    hipLaunchKernelGGL(k_smc_compact, dim3((unsigned)L.nwg), dim3(MESH_THREADS), 0, s, map, L.nblk, mode, (const long long*)(w + L.bo), base,
                       (int*)(w + L.list), (int*)(w + L.sblk));
}

extern "C" {

size_t mvsdf_smc_workspace_bytes(int64_t n, int64_t block) {
    SmcLayout L;
    return smc_layout(n, block, &L) ? L.total : 0;
}

size_t mvsdf_smc_emit_workspace_bytes(int64_t n, int64_t block, int64_t nactive) {
    SmcLayout L;
    SmcEmitLayout E;
    return smc_layout(n, block, &L) && smc_emit_layout(L, nactive, &E) ? E.total : 0;
}

int mvsdf_smc_coarse_points(const float* axis, int64_t n, int64_t block, int64_t start, int64_t count, float* pts, void* stream) {
    SmcLayout L;
    if (!axis || !pts || !smc_layout(n, block, &L)) return mv_fail(-1, "mvsdf_smc_coarse_points: bad arguments");
    const long long m = L.g.nb + 1;
    if (start < 0 || count < 1 || start > m * m * m - count) return mv_fail(-1, "mvsdf_smc_coarse_points: the range leaves the coarse lattice");
    hipLaunchKernelGGL(k_smc_coarse_points, dim3(mv_grid(count, SMC_THREADS)), dim3(SMC_THREADS), 0, (hipStream_t)stream, axis, L.g, (long long)start,
                       (long long)count, pts);
    return mv_check(hipGetLastError(), "mvsdf_smc_coarse_points");
}

int mvsdf_smc_seed(const float* coarse, int64_t n, int64_t block, float level, float tol, void* ws, size_t ws_bytes, void* stream) {
    SmcLayout L;
    if (!coarse || !ws || !smc_layout(n, block, &L) || !(tol >= 0.0f)) return mv_fail(-1, "mvsdf_smc_seed: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_smc_seed: workspace too small (mvsdf_smc_workspace_bytes)");
    L.g.level = level;
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(w, 0, MESH_HDR, s);
    if (e != hipSuccess) return mv_check(e, "mvsdf_smc_seed");
    hipLaunchKernelGGL(k_smc_seed, dim3(mv_grid(L.nblk, SMC_THREADS)), dim3(SMC_THREADS), 0, s, coarse, L.g, tol, (int*)(w + L.map), L.nblk,
                       (unsigned long long*)w);
    smc_compact(L, w, 0, 0, s);
    return mv_check(hipGetLastError(), "mvsdf_smc_seed");
}

int mvsdf_smc_brick_points(const float* axis, int64_t n, int64_t block, const void* ws, size_t ws_bytes, int64_t start, int64_t count, float* pts,
                           void* stream) {
    SmcLayout L;
    if (!axis || !ws || !pts || !smc_layout(n, block, &L)) return mv_fail(-1, "mvsdf_smc_brick_points: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_smc_brick_points: workspace too small (mvsdf_smc_workspace_bytes)");
    const long long P3 = (long long)L.g.P * L.g.P * L.g.P;
    if (start < 0 || count < 1 || start > L.nblk * P3 - count) return mv_fail(-1, "mvsdf_smc_brick_points: the range leaves the slots");
    hipLaunchKernelGGL(k_smc_brick_points, dim3(mv_grid(count, SMC_THREADS)), dim3(SMC_THREADS), 0, (hipStream_t)stream, axis, L.g,
                       (const int*)((const char*)ws + L.list), (long long)start, (long long)count, pts);
    return mv_check(hipGetLastError(), "mvsdf_smc_brick_points");
}

int mvsdf_smc_closure(const float* values, int64_t n, int64_t block, float level, int64_t slot0, int64_t count, void* ws, size_t ws_bytes, void* stream) {
    SmcLayout L;
    if (!values || !ws || !smc_layout(n, block, &L) || slot0 < 0 || count < 1 || slot0 > L.nblk - count)
        return mv_fail(-1, "mvsdf_smc_closure: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_smc_closure: workspace too small (mvsdf_smc_workspace_bytes)");
    L.g.level = level;
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_smc_closure, dim3(mv_grid(count * 6 * L.g.R, SMC_THREADS)), dim3(SMC_THREADS), 0, s, values, L.g, (const int*)(w + L.list),
                       (int*)(w + L.map), (long long)slot0, (long long)count, (unsigned long long*)w);
    smc_compact(L, w, 0, slot0 + count, s);
    return mv_check(hipGetLastError(), "mvsdf_smc_closure");
}

int mvsdf_smc_count(const float* values, int64_t n, int64_t block, float level, int64_t nactive, void* ws, size_t ws_bytes, void* ews, size_t ews_bytes,
                    void* stream) {
    SmcLayout L;
    SmcEmitLayout E;
    if (!values || !ws || !ews || !smc_layout(n, block, &L) || !smc_emit_layout(L, nactive, &E)) return mv_fail(-1, "mvsdf_smc_count: bad arguments");
    if (ws_bytes < L.total || ews_bytes < E.total) return mv_fail(-1, "mvsdf_smc_count: workspace too small (mvsdf_smc_workspace_bytes / _emit_workspace_bytes)");
    L.g.level = level;
    char* w = (char*)ws;
    char* x = (char*)ews;
    hipStream_t s = (hipStream_t)stream;
    const long long P3 = (long long)L.g.P * L.g.P * L.g.P;
    smc_compact(L, w, 1, 0, s);
    hipLaunchKernelGGL(k_smc_meta, dim3(mv_grid(nactive, SMC_THREADS)), dim3(SMC_THREADS), 0, s, (const int*)(w + L.sblk), (int)nactive, L.g.nb,
                       (int4*)(w + L.meta));
    const unsigned fin_wgs = mv_grid(nactive * P3, MV_THREADS) < 4096u ? mv_grid(nactive * P3, MV_THREADS) : 4096u;
    hipLaunchKernelGGL(k_any_nonfinite<float>, dim3(fin_wgs), dim3(MV_THREADS), 0, s, values, nactive * P3, (unsigned long long*)w + MVSDF_SMC_H_BAD, 1ull);   // one flag for the whole pool
    hipLaunchKernelGGL(k_smc_count, dim3((unsigned)E.nwg), dim3(MESH_THREADS), 0, s, values, L.g, (const int*)(w + L.map), (const int*)(w + L.sblk),
                       (const int4*)(w + L.meta), E.nrows, smc_bits(3ll * L.g.R), smc_bits((long long)MC_MAX_TRIS * L.g.B), (int*)(x + E.bv), (int*)(x + E.bf));
    hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(MESH_SCAN_THREADS), 0, s, (const int*)(x + E.bv), (const int*)(x + E.bf), (int)E.nwg, (long long*)(x + E.ov),
                       (long long*)(x + E.of), (long long*)w + MVSDF_SMC_H_VERTS);
    return mv_check(hipGetLastError(), "mvsdf_smc_count");
}

int mvsdf_smc_emit(const float* values, int64_t n, int64_t block, float level, const float* spacing, const float* origin, int64_t nactive, void* ws,
                   size_t ws_bytes, void* ews, size_t ews_bytes, float* verts, float* normals, int32_t* faces, int64_t nv_cap, int64_t nf_cap, void* stream) {
    SmcLayout L;
    SmcEmitLayout E;
    if (!values || !ws || !ews || !spacing || !origin || !smc_layout(n, block, &L) || !smc_emit_layout(L, nactive, &E) || nv_cap < 0 || nf_cap < 0 ||
        (nv_cap && (!verts || !normals)) || (nf_cap && !faces))
        return mv_fail(-1, "mvsdf_smc_emit: bad arguments");
    if (ws_bytes < L.total || ews_bytes < E.total) return mv_fail(-1, "mvsdf_smc_emit: workspace too small (mvsdf_smc_workspace_bytes / _emit_workspace_bytes)");
    L.g.level = level;
    McGeom gm;
    for (int a = 0; a < 3; ++a) {
        gm.sp[a] = spacing[a];
        gm.org[a] = origin[a];
    }
    char* w = (char*)ws;
    char* x = (char*)ews;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_smc_vertices, dim3((unsigned)E.nwg), dim3(MESH_THREADS), 0, s, values, L.g, gm, (const int*)(w + L.map), (const int*)(w + L.sblk),
                       (const int4*)(w + L.meta), E.nrows, smc_bits(3ll * L.g.R), (const long long*)(x + E.ov), (int*)(x + E.idmap), verts, normals,
                       (long long)nv_cap);
    hipLaunchKernelGGL(k_smc_faces, dim3((unsigned)E.nwg), dim3(MESH_THREADS), 0, s, values, L.g, (const int*)(w + L.map), (const int*)(w + L.sblk),
                       (const int4*)(w + L.meta), E.nrows, smc_bits((long long)MC_MAX_TRIS * L.g.B), (const long long*)(x + E.of), (const int*)(x + E.idmap),
                       faces, (long long)nf_cap, (unsigned long long*)w);
    return mv_check(hipGetLastError(), "mvsdf_smc_emit");
}

}  // extern "C"
