// mesh_kernels.hip -- on-device mesh extraction (reference code/evaluation/eval.py:109-125, code/utils/plots.py:150-205):
// marching cubes over an fp32 volume with arbitrary element strides, plain (mesh.marching_cubes) or under a per-point validity mask
// (mesh.marching_cubes_masked, which meshes tsdf.hip's volumes): one set of passes, templates on a mask policy (McNoMask / McMask below); connected
// components of the mesh by union-find, and the compaction of one component.  Conventions (vertex / face order, positions, normals, the mask's
// additions): mvsdf_amd/mesh.py; tests/mc_ref.py and tests/tsdf_ref.py restate them in numpy; the triangle table: tools/gen_mc_tables.py -> mc_tables.h.
//
// Every pass maps items (grid points, vertices or faces) to workgroups in linear order: workgroup b owns items [b * MESH_CHUNK, (b + 1) * MESH_CHUNK),
// its 256 lanes take MESH_CHUNK / 256 consecutive rounds of 256.  A count pass writes one small total per workgroup, k_mesh_scan turns them into
// int64 workgroup offsets, and the emit pass recounts the same items (per wave with __ballot / __popcll) to place each one.  Outputs therefore come
// in item order and do not depend on scheduling.
#include <string.h>
#include "mesh_common.h"

struct MeshVol {
    const float* p;
    long long n[3], s[3];                             // extents and element strides of vol[i, j, k]
    float level;
};

// the accessor of mesh_common.h's formulas
struct VolVal {
    const MeshVol& v;
    __device__ __forceinline__ float operator()(long long i, long long j, long long k) const { return v.p[i * v.s[0] + j * v.s[1] + k * v.s[2]]; }
};

// linear index (k fastest) of grid point (i, j, k), and back
__device__ __forceinline__ long long point_at(const MeshVol& v, long long i, long long j, long long k) { return (i * v.n[1] + j) * v.n[2] + k; }

__device__ __forceinline__ void point_ijk(const MeshVol& v, long long p, long long* g) {
    const long long nyz = v.n[1] * v.n[2];
    g[0] = p / nyz;
    const long long r = p - g[0] * nyz;
    g[1] = r / v.n[2];
    g[2] = r - g[1] * v.n[2];
}

// crossing edges owned by grid point g: bit a = the edge to g + e_a crosses the level (in0: the value at g is inside)
__device__ __forceinline__ int point_edges(const MeshVol& v, const long long* g, bool in0) {
    return mc_point_edges(VolVal{v}, v.n, g[0], g[1], g[2], in0, v.level);
}

// g = p's (i, j, k); true iff the cell with lower corner p lies in the grid
__device__ __forceinline__ bool cell_ijk(const MeshVol& v, long long p, long long* g) {
    point_ijk(v, p, g);
    return g[0] + 1 < v.n[0] && g[1] + 1 < v.n[1] && g[2] + 1 < v.n[2];
}

// ================================================================ marching cubes: one set of passes, two mask policies ================================================================
// The passes k_mc_count / k_mc_vertices / k_mc_faces are templates on a mask policy M, which says which points and cells take part:
//   point(p)               grid point p holds a value
//   cell_at(v, p, g)       the cell with lower corner p exists and its 8 corners hold values; g = p's (i, j, k) (the face pass splits p only then)
//   around(v, g)           bit a: the grid edge (g, g + e_a) may carry a vertex
//   keep(p, bits)          the count pass hands over point p's vertex-carrying edges
//   bits(v, g, p), kStored the later passes ask for them: recomputed from the values, or (kStored) the byte keep stored -- then a value is read only
//                          where a bit is set
//   grad()                 mc_vertex's gradient rule
// McNoMask (marching_cubes) is empty: a kernel instance carries no pointer and loads or stores nothing for it.  McMask (marching_cubes_masked) never
// reads the value of an invalid point.

struct McNoMask {
    static constexpr bool kStored = false;
    __device__ __forceinline__ bool point(long long) const { return true; }
    __device__ __forceinline__ bool cell_at(const MeshVol& v, long long p, long long* g) const { return cell_ijk(v, p, g); }
    __device__ __forceinline__ int around(const MeshVol&, const long long*) const { return 7; }
    __device__ __forceinline__ void keep(long long, int) const {}
    __device__ __forceinline__ int bits(const MeshVol& v, const long long* g, long long) const {
        return point_edges(v, g, VolVal{v}(g[0], g[1], g[2]) < v.level);
    }
    __device__ __forceinline__ McGrad grad() const { return McGrad(); }
};

// gradient component c at the valid grid point g from its neighbours g -+ e_c that are in the grid and valid: both -> central difference over 2h, one ->
// one-sided over h, none -> 0 (with every point valid: mc_grad_c)
struct McMaskGrad {
    const unsigned char* ok;
    template <class V>
    __device__ __forceinline__ float operator()(const V& val, const long long* n, const long long* g, int c, float h) const {
        long long lo[3] = {g[0], g[1], g[2]}, hi[3] = {g[0], g[1], g[2]};
        lo[c] -= 1;
        hi[c] += 1;
        const bool has_lo = lo[c] >= 0 && ok[(lo[0] * n[1] + lo[1]) * n[2] + lo[2]];
        const bool has_hi = hi[c] < n[c] && ok[(hi[0] * n[1] + hi[1]) * n[2] + hi[2]];
        if (!has_lo && !has_hi) return 0.0f;
        if (!has_lo) lo[c] = g[c];
        if (!has_hi) hi[c] = g[c];
        const float den = has_lo && has_hi ? 2.0f * h : h;
        return (val(hi[0], hi[1], hi[2]) - val(lo[0], lo[1], lo[2])) / den;
    }
};

struct McMask {
    const unsigned char* valid;                       // valid[i][j][k], contiguous
    unsigned char* cell;                              // k_mcm_cells: the cell with this lower corner is valid
    unsigned char* ebits;                             // k_mc_count: the point's crossing edges that touch a valid cell
    static constexpr bool kStored = true;
    __device__ __forceinline__ bool point(long long p) const { return valid[p]; }
    __device__ __forceinline__ bool cell_at(const MeshVol& v, long long p, long long* g) const {
        if (!cell[p]) return false;
        point_ijk(v, p, g);
        return true;
    }
    // bit a: one of the up to four cells around the grid edge (g, g + e_a) is valid (then both of its ends are)
    __device__ __forceinline__ int around(const MeshVol& v, const long long* g) const {
        int bits = 0;
        for (int a = 0; a < 3; ++a) {
            const int o0 = a == 0 ? 1 : 0, o1 = a == 2 ? 1 : 2;
            bool any = false;
            for (int m = 0; m < 4; ++m) {
                long long q[3] = {g[0], g[1], g[2]};
                q[o0] -= m & 1;
                q[o1] -= m >> 1;
                if (q[o0] >= 0 && q[o1] >= 0) any = any || cell[point_at(v, q[0], q[1], q[2])];
            }
            if (any) bits |= 1 << a;
        }
        return bits;
    }
    __device__ __forceinline__ void keep(long long p, int bits) const { ebits[p] = (unsigned char)bits; }
    __device__ __forceinline__ int bits(const MeshVol&, const long long*, long long p) const { return ebits[p]; }
    __device__ __forceinline__ McMaskGrad grad() const { return McMaskGrad{valid}; }
};

// ---- pass 0, McMask only: cell[p] = the cell with lower corner p exists and its 8 corners are valid ----
__global__ __launch_bounds__(MESH_THREADS) void k_mcm_cells(MeshVol v, long long npts, McMask m) {
    const long long p = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
    if (p >= npts) return;
    long long g[3];
    bool ok = cell_ijk(v, p, g);
    if (ok) {
#pragma unroll
        for (int c = 0; c < 8; ++c) ok = ok && m.valid[point_at(v, g[0] + (c & 1), g[1] + (c >> 1 & 1), g[2] + (c >> 2 & 1))];
    }
    m.cell[p] = ok ? 1 : 0;
}

// ---- pass 1: vertices and triangles per workgroup (bv / bf), or -1 in bf when the workgroup saw a non-finite value at a point that holds one ----
template <class M>
__global__ __launch_bounds__(MESH_THREADS) void k_mc_count(MeshVol v, long long npts, M m, int* __restrict__ bv, int* __restrict__ bf) {
    __shared__ int s_w[MESH_THREADS / 64];
    long long rv = 0, rf = 0;
    int bad = 0;
    for (int r = 0; r < MESH_ROUNDS; ++r) {
        const long long p = (long long)blockIdx.x * MESH_CHUNK + r * MESH_THREADS + threadIdx.x;
        int bits = 0, nt = 0;
        if (p < npts) {
            long long g[3];
            point_ijk(v, p, g);
            if (m.point(p)) {
                const float x = VolVal{v}(g[0], g[1], g[2]);
                bad |= !isfinite(x);
                const int around = m.around(v, g);
                if (around) bits = point_edges(v, g, x < v.level) & around;
                if (m.cell_at(v, p, g)) nt = mc_ntri(mc_cube_index(VolVal{v}, g[0], g[1], g[2], v.level));
            }
            m.keep(p, bits);
        }
        block_excl(__popc(bits), 2, s_w, rv);
        block_excl(nt, 3, s_w, rf);
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        bv[blockIdx.x] = (int)rv;
        bf[blockIdx.x] = bad ? -1 : (int)rf;
    }
}

// ---- pass 2: the vertex id map (id of each point's first vertex), vertices and normals ----
template <class M>
__global__ __launch_bounds__(MESH_THREADS) void k_mc_vertices(MeshVol v, long long npts, M m, McGeom gm, const long long* __restrict__ ov, int* __restrict__ idmap,
                                                              float* __restrict__ verts, float* __restrict__ normals, long long nv_cap) {
    __shared__ int s_w[MESH_THREADS / 64];
    long long run = ov[blockIdx.x];
    for (int r = 0; r < MESH_ROUNDS; ++r) {
        const long long p = (long long)blockIdx.x * MESH_CHUNK + r * MESH_THREADS + threadIdx.x;
        int bits = 0;
        long long g[3] = {0, 0, 0};
        float x = 0.0f;
        if (p < npts) {
            if (!M::kStored) {                                       // recomputed bits need the point and its value
                point_ijk(v, p, g);
                x = VolVal{v}(g[0], g[1], g[2]);
            }
            bits = m.bits(v, g, p);
        }
        long long id = block_excl(__popc(bits), 2, s_w, run);
        if (p >= npts) continue;
        idmap[p] = (int)id;
        if (M::kStored) {                                            // stored bits: the value is read only where an edge carries a vertex
            if (!bits) continue;
            point_ijk(v, p, g);
            x = VolVal{v}(g[0], g[1], g[2]);
        }
        for (int a = 0; a < 3; ++a) {
            if (!(bits >> a & 1)) continue;
            if (id < nv_cap) mc_vertex(VolVal{v}, v.n, g, a, x, v.level, gm, verts + id * 3, normals + id * 3, m.grad());
            ++id;
        }
    }
}

// ---- pass 3: faces (int32 vertex ids), cells in linear order, each cell's triangles in table order.  The vertex id of a cube edge: its owner's first
// id plus the owner's vertex-carrying edges along lower axes ----
template <class M>
__global__ __launch_bounds__(MESH_THREADS) void k_mc_faces(MeshVol v, long long npts, M m, const long long* __restrict__ of, const int* __restrict__ idmap,
                                                           int* __restrict__ faces, long long nf_cap) {
    __shared__ int s_w[MESH_THREADS / 64];
    long long run = of[blockIdx.x];
    for (int r = 0; r < MESH_ROUNDS; ++r) {
        const long long p = (long long)blockIdx.x * MESH_CHUNK + r * MESH_THREADS + threadIdx.x;
        long long g[3] = {0, 0, 0};
        int ci = 0, nt = 0;
        if (p < npts && m.cell_at(v, p, g)) {
            ci = mc_cube_index(VolVal{v}, g[0], g[1], g[2], v.level);
            nt = mc_ntri(ci);
        }
        const long long fid = block_excl(nt, 3, s_w, run);
        for (int t = 0; t < nt; ++t) {
            if (fid + t >= nf_cap) break;
            const int base = (mc_tri_offset[ci] + t) * 3;
            for (int s = 0; s < 3; ++s) {
                long long q[3] = {g[0], g[1], g[2]};
                const int a = mc_edge_owner(mc_tri_edges[base + s], q);
                const long long o = point_at(v, q[0], q[1], q[2]);
                faces[(fid + t) * 3 + s] = idmap[o] + __popc(m.bits(v, q, o) & ((1 << a) - 1));
            }
        }
    }
}

// ---- connected components: union-find over vertex ids (a root is the lowest id of its set: parent[x] <= x always) ----
__device__ __forceinline__ int uf_find(int* parent, int x, int n, int* err) {
    for (int it = 0; it < n; ++it) {
        const int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        x = p;
    }
    atomicOr(err, 1);
    return x;
}

__global__ __launch_bounds__(MESH_THREADS) void k_cc_init(int nv, int* __restrict__ parent, unsigned long long* __restrict__ acc, int* __restrict__ minface,
                                                          int* __restrict__ cv, int* __restrict__ cf, unsigned long long* __restrict__ scal, int* __restrict__ err) {
    const long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (x < nv) {
        parent[x] = (int)x;
        acc[x] = 0;
        minface[x] = INT_MAX;
        cv[x] = 0;
        cf[x] = 0;
    }
    if (x < 4) scal[x] = 0;
    if (x == 0) *err = 0;
}

__global__ __launch_bounds__(MESH_THREADS) void k_cc_hook(const int* __restrict__ faces, int nf, int nv, int* parent, int* err) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    const int a = faces[f * 3];
    for (int s = 1; s < 3; ++s) {
        int x = a, y = faces[f * 3 + s];
        int it = 0;
        for (; it < nv; ++it) {
            x = uf_find(parent, x, nv, err);
            y = uf_find(parent, y, nv, err);
            if (x == y) break;
            const int hi = max(x, y), lo = min(x, y);
            if (atomicCAS(parent + hi, hi, lo) == hi) break;
        }
        if (it == nv) atomicOr(err, 1);
    }
}

__global__ __launch_bounds__(MESH_THREADS) void k_cc_flatten(int nv, int* parent, int* err) {
    const long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (x < nv) parent[x] = uf_find(parent, (int)x, nv, err);
}

// per-workgroup count of items whose label is `want` (self != 0: whose entry equals its own index, i.e. union-find roots)
__global__ __launch_bounds__(MESH_THREADS) void k_flag_count(const int* __restrict__ lab, long long n, int want, int self, int* __restrict__ bc) {
    __shared__ int s_w[MESH_THREADS / 64];
    long long run = 0;
    for (int r = 0; r < MESH_ROUNDS; ++r) {
        const long long x = (long long)blockIdx.x * MESH_CHUNK + r * MESH_THREADS + threadIdx.x;
        block_excl(x < n && lab[x] == (self ? (int)x : want), 1, s_w, run);
    }
    if (threadIdx.x == 0) bc[blockIdx.x] = (int)run;
}

// dense component ids: roots numbered in ascending vertex order
__global__ __launch_bounds__(MESH_THREADS) void k_cc_dense(const int* __restrict__ parent, int nv, const long long* __restrict__ off, int* __restrict__ dense) {
    __shared__ int s_w[MESH_THREADS / 64];
    long long run = off[blockIdx.x];
    for (int r = 0; r < MESH_ROUNDS; ++r) {
        const long long x = (long long)blockIdx.x * MESH_CHUNK + r * MESH_THREADS + threadIdx.x;
        const bool root = x < nv && parent[x] == (int)x;
        const long long id = block_excl(root, 1, s_w, run);
        if (root) dense[x] = (int)id;
    }
}

// Per-component accumulations go through one atomic per wave when the wave's valid lanes share the component (one large component would
// otherwise send every lane of the grid to the same address).  Every lane of the wave calls these; invalid lanes pass neutral values.
struct WaveKey {
    bool any, uniform;
    int first, key, count;                                           // first valid lane, its key, number of valid lanes
};

__device__ __forceinline__ WaveKey wave_key(bool valid, int key) {
    WaveKey w;
    const unsigned long long vm = __ballot(valid);
    w.any = vm != 0;
    w.count = __popcll(vm);
    w.first = w.any ? __ffsll((long long)vm) - 1 : 0;
    w.key = __shfl(key, w.first);
    w.uniform = __ballot(valid && key == w.key) == vm;
    return w;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x) {
    for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long x) {
    for (int o = 32; o; o >>= 1) {
        const unsigned long long y = __shfl_xor(x, o);
        x = y > x ? y : x;
    }
    return x;
}

__global__ __launch_bounds__(MESH_THREADS) void k_cc_label_vertices(const int* __restrict__ parent, const int* __restrict__ dense, int nv, int* __restrict__ vlab,
                                                                    int* __restrict__ cv) {
    const long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = x < nv;
    const int l = valid ? dense[parent[x]] : 0;
    if (valid) vlab[x] = l;
    const WaveKey w = wave_key(valid, l);
    if (!w.any) return;
    if (w.uniform) {
        if ((threadIdx.x & 63) == w.first) atomicAdd(cv + l, w.count);
    } else if (valid) {
        atomicAdd(cv + l, 1);
    }
}

__device__ __forceinline__ double tri_area(const float* __restrict__ vs, const int* __restrict__ faces, long long f) {
    const float* p0 = vs + (long long)faces[f * 3] * 3;
    const float* p1 = vs + (long long)faces[f * 3 + 1] * 3;
    const float* p2 = vs + (long long)faces[f * 3 + 2] * 3;
    const double ux = (double)p1[0] - p0[0], uy = (double)p1[1] - p0[1], uz = (double)p1[2] - p0[2];
    const double wx = (double)p2[0] - p0[0], wy = (double)p2[1] - p0[1], wz = (double)p2[2] - p0[2];
    const double cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
    return 0.5 * sqrt(cx * cx + cy * cy + cz * cz);
}

// face labels, face counts, lowest face per component, and the largest triangle area (non-negative doubles order like their bit patterns)
__global__ __launch_bounds__(MESH_THREADS) void k_cc_faces(const float* __restrict__ vs, const int* __restrict__ faces, int nf, const int* __restrict__ vlab,
                                                           int* __restrict__ flab, int* __restrict__ cf, int* __restrict__ minface, unsigned long long* scal) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = f < nf;
    const int l = valid ? vlab[faces[f * 3]] : 0;
    const unsigned long long abits = valid ? (unsigned long long)__double_as_longlong(tri_area(vs, faces, f)) : 0ull;
    if (valid) flab[f] = l;
    const WaveKey w = wave_key(valid, l);
    if (!w.any) return;
    const unsigned long long amax = wave_max(abits);
    const bool leader = (threadIdx.x & 63) == w.first;
    if (leader) atomicMax(scal, amax);
    if (w.uniform) {
        if (leader) {                                                // faces ascend with the lane: the first valid lane has the lowest index
            atomicAdd(cf + l, w.count);
            atomicMin(minface + l, (int)f);
        }
    } else if (valid) {
        atomicAdd(cf + l, 1);
        atomicMin(minface + l, (int)f);
    }
}

// fixed-point scale 2^S with nf * max area * 2^S <= 2^61: the int64 sums are exact, so they do not depend on the order of the atomics
__device__ __forceinline__ double area_scale(unsigned long long amax_bits, int nf) {
    const double amax = __longlong_as_double((long long)amax_bits);
    if (!(amax > 0.0)) return 1.0;
    int lf = 0;
    while ((1ll << lf) < nf) ++lf;
    return ldexp(1.0, 60 - ilogb(amax) - lf);
}

__global__ __launch_bounds__(MESH_THREADS) void k_cc_area(const float* __restrict__ vs, const int* __restrict__ faces, int nf, const int* __restrict__ flab,
                                                          unsigned long long* __restrict__ acc, const unsigned long long* __restrict__ scal) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = f < nf;
    const int l = valid ? flab[f] : 0;
    const unsigned long long q = valid ? (unsigned long long)llrint(tri_area(vs, faces, f) * area_scale(scal[0], nf)) : 0ull;
    const WaveKey w = wave_key(valid, l);
    if (!w.any) return;
    if (w.uniform) {
        const unsigned long long sum = wave_sum(q);
        if ((threadIdx.x & 63) == w.first) atomicAdd(acc + l, sum);
    } else if (valid) {
        atomicAdd(acc + l, q);
    }
}

// scal[1] = the largest area sum; then scal[2] = the lowest face index among the components that reach it, as its complement (scal[2] starts at 0)
__global__ __launch_bounds__(MESH_THREADS) void k_cc_best_area(const unsigned long long* __restrict__ acc, const long long* __restrict__ ncomp, unsigned long long* scal) {
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < ncomp[0]) atomicMax(scal + 1, acc[c]);
}

__global__ __launch_bounds__(MESH_THREADS) void k_cc_best_face(const unsigned long long* __restrict__ acc, const int* __restrict__ minface, const long long* __restrict__ ncomp,
                                                               unsigned long long* scal) {
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < ncomp[0] && acc[c] == scal[1]) atomicMax(scal + 2, ~0ull - (unsigned long long)minface[c]);
}

// the results, MVSDF_CC_H_*
__global__ void k_cc_result(const long long* __restrict__ ncomp, const unsigned long long* __restrict__ scal, const int* __restrict__ flab, const int* __restrict__ cv,
                            const int* __restrict__ cf, const int* __restrict__ err, int nf, long long* __restrict__ out) {
    const long long f = nf ? (long long)(~0ull - scal[2]) : -1;
    const int l = f >= 0 && f < nf ? flab[f] : -1;
    out[MVSDF_CC_H_COMPONENTS] = ncomp[0];
    out[MVSDF_CC_H_LABEL] = l;
    out[MVSDF_CC_H_VERTS] = l >= 0 ? cv[l] : 0;
    out[MVSDF_CC_H_FACES] = l >= 0 ? cf[l] : 0;
    out[MVSDF_CC_H_BOUND] = *err;
}

// ---- compaction of one component: kept vertices / faces in their original order, faces re-indexed ----
__global__ __launch_bounds__(MESH_THREADS) void k_sel_vertices(const int* __restrict__ vlab, int nv, int label, const long long* __restrict__ off,
                                                               const float* __restrict__ vs, const float* __restrict__ ns, const float* __restrict__ cs,
                                                               int* __restrict__ vmap, float* __restrict__ ovs, float* __restrict__ ons, float* __restrict__ ocs,
                                                               long long cap) {
    __shared__ int s_w[MESH_THREADS / 64];
    long long run = off[blockIdx.x];
    for (int r = 0; r < MESH_ROUNDS; ++r) {
        const long long x = (long long)blockIdx.x * MESH_CHUNK + r * MESH_THREADS + threadIdx.x;
        const bool keep = x < nv && vlab[x] == label;
        const long long id = block_excl(keep, 1, s_w, run);
        if (!keep || id >= cap) continue;
        vmap[x] = (int)id;
        for (int c = 0; c < 3; ++c) {
            ovs[id * 3 + c] = vs[x * 3 + c];
            if (ns) ons[id * 3 + c] = ns[x * 3 + c];
            if (cs) ocs[id * 3 + c] = cs[x * 3 + c];
        }
    }
}

__global__ __launch_bounds__(MESH_THREADS) void k_sel_faces(const int* __restrict__ flab, int nf, int label, const long long* __restrict__ off,
                                                            const int* __restrict__ faces, const int* __restrict__ vmap, int* __restrict__ ofaces, long long cap) {
    __shared__ int s_w[MESH_THREADS / 64];
    long long run = off[blockIdx.x];
    for (int r = 0; r < MESH_ROUNDS; ++r) {
        const long long x = (long long)blockIdx.x * MESH_CHUNK + r * MESH_THREADS + threadIdx.x;
        const bool keep = x < nf && flab[x] == label;
        const long long id = block_excl(keep, 1, s_w, run);
        if (!keep || id >= cap) continue;
        for (int s = 0; s < 3; ++s) ofaces[id * 3 + s] = vmap[faces[x * 3 + s]];
    }
}

// ---- workspace layouts (every region 256-byte aligned) ----

struct McLayout {
    long long npts, nb;
    size_t idmap, cell, ebits, bv, bf, ov, of, total;           // cell, ebits: McMask's two byte arrays (masked only)
};

// false: a dimension below 2, or a grid whose points or workgroups the kernels cannot index (masked: k_mcm_cells takes one lane per point)
static bool mc_layout(long long nx, long long ny, long long nz, bool masked, McLayout* L) {
    if (nx < 2 || ny < 2 || nz < 2) return false;
    const long long lim = 1ll << (masked ? 40 : 60);
    if (nx > lim / ny || nx * ny > lim / nz) return false;
    L->npts = nx * ny * nz;
    L->nb = mv_ceil_div(L->npts, MESH_CHUNK);
    if (L->nb > INT_MAX || (masked && mv_ceil_div(L->npts, MESH_THREADS) > INT_MAX)) return false;
    WsCursor c{MESH_HDR};
    L->idmap = c.take((size_t)L->npts * 4);
    L->cell = L->ebits = 0;
    if (masked) {
        L->cell = c.take((size_t)L->npts);
        L->ebits = c.take((size_t)L->npts);
    }
    L->bv = c.take((size_t)L->nb * 4);
    L->bf = c.take((size_t)L->nb * 4);
    L->ov = c.take((size_t)L->nb * 8);
    L->of = c.take((size_t)L->nb * 8);
    L->total = c.o;
    return true;
}

struct CcLayout {
    long long nbv, nbf;
    size_t parent, dense, acc, minface, cv, cf, bc, bo, bc2, bo2, scal, err, vmap, total;
};

static bool cc_layout(long long nv, long long nf, CcLayout* L) {
    if (nv < 1 || nf < 1 || nv > INT_MAX || nf > INT_MAX) return false;
    L->nbv = mv_ceil_div(nv, MESH_CHUNK);
    L->nbf = mv_ceil_div(nf, MESH_CHUNK);
    WsCursor c{MESH_HDR};
    L->parent = c.take((size_t)nv * 4);
    L->dense = c.take((size_t)nv * 4);
    L->acc = c.take((size_t)nv * 8);
    L->minface = c.take((size_t)nv * 4);
    L->cv = c.take((size_t)nv * 4);
    L->cf = c.take((size_t)nv * 4);
    L->bc = c.take((size_t)L->nbv * 4);
    L->bo = c.take((size_t)L->nbv * 8);
    L->bc2 = c.take((size_t)L->nbf * 4);
    L->bo2 = c.take((size_t)L->nbf * 8);
    L->scal = c.take(4 * 8);
    L->err = c.take(4);
    L->vmap = L->dense;                                          // mvsdf_mesh_select reuses the dense-id region
    L->total = c.o;
    return true;
}

// the volume and its workspace layout from a call's arguments; false: a NULL pointer or a shape mc_layout refuses
static bool mc_vol(const float* vol, const int64_t* shape, const int64_t* strides, float level, bool masked, McLayout* L, MeshVol* v) {
    if (!vol || !shape || !strides || !mc_layout(shape[0], shape[1], shape[2], masked, L)) return false;
    v->p = vol;
    v->level = level;
    for (int a = 0; a < 3; ++a) {
        v->n[a] = shape[a];
        v->s[a] = strides[a];
    }
    return true;
}

static McMask mc_mask(const uint8_t* valid, const McLayout& L, void* ws) { return McMask{valid, (unsigned char*)ws + L.cell, (unsigned char*)ws + L.ebits}; }

template <class M>
static int mc_count(const MeshVol& v, const McLayout& L, M m, void* ws, void* stream, const char* what) {
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mc_count<M>, dim3((unsigned)L.nb), dim3(MESH_THREADS), 0, s, v, L.npts, m, (int*)(w + L.bv), (int*)(w + L.bf));
    hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(MESH_SCAN_THREADS), 0, s, (const int*)(w + L.bv), (const int*)(w + L.bf), (int)L.nb,
                       (long long*)(w + L.ov), (long long*)(w + L.of), (long long*)w + MVSDF_MC_H_VERTS);
    return mv_check(hipGetLastError(), what);
}

static bool mc_emit_args(const float* spacing, const float* origin, const float* verts, const float* normals, const int32_t* faces, int64_t nv_cap,
                         int64_t nf_cap, McGeom* gm) {
    if (!spacing || !origin || nv_cap < 0 || nf_cap < 0 || (nv_cap && (!verts || !normals)) || (nf_cap && !faces)) return false;
    for (int a = 0; a < 3; ++a) {
        gm->sp[a] = spacing[a];
        gm->org[a] = origin[a];
    }
    return true;
}

template <class M>
static int mc_emit(const MeshVol& v, const McLayout& L, M m, const McGeom& gm, void* ws, float* verts, float* normals, int32_t* faces, int64_t nv_cap,
                   int64_t nf_cap, void* stream, const char* what) {
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mc_vertices<M>, dim3((unsigned)L.nb), dim3(MESH_THREADS), 0, s, v, L.npts, m, gm, (const long long*)(w + L.ov), (int*)(w + L.idmap),
                       verts, normals, (long long)nv_cap);
    hipLaunchKernelGGL(k_mc_faces<M>, dim3((unsigned)L.nb), dim3(MESH_THREADS), 0, s, v, L.npts, m, (const long long*)(w + L.of), (const int*)(w + L.idmap),
                       faces, (long long)nf_cap);
    return mv_check(hipGetLastError(), what);
}

extern "C" {

size_t mvsdf_mc_workspace_bytes(int64_t nx, int64_t ny, int64_t nz) {
    McLayout L;
    return mc_layout(nx, ny, nz, false, &L) ? L.total : 0;
}

int mvsdf_mc_count(const float* vol, const int64_t* shape, const int64_t* strides, float level, void* ws, size_t ws_bytes, void* stream) {
    McLayout L;
    MeshVol v;
    if (!mc_vol(vol, shape, strides, level, false, &L, &v) || !ws) return mv_fail(-1, "mvsdf_mc_count: bad arguments (every extent must be >= 2)");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_mc_count: workspace too small (mvsdf_mc_workspace_bytes)");
    return mc_count(v, L, McNoMask(), ws, stream, "mvsdf_mc_count");
}

int mvsdf_mc_emit(const float* vol, const int64_t* shape, const int64_t* strides, float level, const float* spacing, const float* origin, void* ws, size_t ws_bytes,
                  float* verts, float* normals, int32_t* faces, int64_t nv_cap, int64_t nf_cap, void* stream) {
    McLayout L;
    MeshVol v;
    McGeom gm;
    if (!mc_vol(vol, shape, strides, level, false, &L, &v) || !ws || !mc_emit_args(spacing, origin, verts, normals, faces, nv_cap, nf_cap, &gm))
        return mv_fail(-1, "mvsdf_mc_emit: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_mc_emit: workspace too small (mvsdf_mc_workspace_bytes)");
    return mc_emit(v, L, McNoMask(), gm, ws, verts, normals, faces, nv_cap, nf_cap, stream, "mvsdf_mc_emit");
}

size_t mvsdf_mcm_workspace_bytes(int64_t nx, int64_t ny, int64_t nz) {
    McLayout L;
    return mc_layout(nx, ny, nz, true, &L) ? L.total : 0;
}

int mvsdf_mcm_count(const float* vol, const uint8_t* valid, const int64_t* shape, const int64_t* strides, float level, void* ws, size_t ws_bytes, void* stream) {
    McLayout L;
    MeshVol v;
    if (!mc_vol(vol, shape, strides, level, true, &L, &v) || !valid || !ws) return mv_fail(-1, "mvsdf_mcm_count: bad arguments (every extent must be >= 2)");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_mcm_count: workspace too small (mvsdf_mcm_workspace_bytes)");
    const McMask m = mc_mask(valid, L, ws);
    hipLaunchKernelGGL(k_mcm_cells, dim3(mv_grid(L.npts, MESH_THREADS)), dim3(MESH_THREADS), 0, (hipStream_t)stream, v, L.npts, m);
    return mc_count(v, L, m, ws, stream, "mvsdf_mcm_count");
}

int mvsdf_mcm_emit(const float* vol, const uint8_t* valid, const int64_t* shape, const int64_t* strides, float level, const float* spacing, const float* origin,
                   void* ws, size_t ws_bytes, float* verts, float* normals, int32_t* faces, int64_t nv_cap, int64_t nf_cap, void* stream) {
    McLayout L;
    MeshVol v;
    McGeom gm;
    if (!mc_vol(vol, shape, strides, level, true, &L, &v) || !valid || !ws || !mc_emit_args(spacing, origin, verts, normals, faces, nv_cap, nf_cap, &gm))
        return mv_fail(-1, "mvsdf_mcm_emit: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_mcm_emit: workspace too small (mvsdf_mcm_workspace_bytes)");
    return mc_emit(v, L, mc_mask(valid, L, ws), gm, ws, verts, normals, faces, nv_cap, nf_cap, stream, "mvsdf_mcm_emit");
}

size_t mvsdf_mesh_cc_workspace_bytes(int64_t nv, int64_t nf) {
    CcLayout L;
    return cc_layout(nv, nf, &L) ? L.total : 0;
}

int mvsdf_mesh_components(const float* verts, const int32_t* faces, int64_t nv, int64_t nf, void* ws, size_t ws_bytes, int32_t* vert_label, int32_t* face_label,
                          void* stream) {
    CcLayout L;
    if (!verts || !faces || !ws || !vert_label || !face_label || !cc_layout(nv, nf, &L)) return mv_fail(-1, "mvsdf_mesh_components: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_mesh_components: workspace too small (mvsdf_mesh_cc_workspace_bytes)");
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    int* parent = (int*)(w + L.parent);
    int* dense = (int*)(w + L.dense);
    unsigned long long* acc = (unsigned long long*)(w + L.acc);
    int* minface = (int*)(w + L.minface);
    int* cv = (int*)(w + L.cv);
    int* cf = (int*)(w + L.cf);
    unsigned long long* scal = (unsigned long long*)(w + L.scal);
    int* err = (int*)(w + L.err);
    long long* ncomp = (long long*)(w + L.bo2);                  // k_mesh_scan's totals (3 int64) land in the face-offset region, unused here
    const int V = (int)nv, F = (int)nf;
    hipLaunchKernelGGL(k_cc_init, dim3(mv_grid(V > 4 ? V : 4, MESH_THREADS)), dim3(MESH_THREADS), 0, s, V, parent, acc, minface, cv, cf, scal, err);
    hipLaunchKernelGGL(k_cc_hook, dim3(mv_grid(F, MESH_THREADS)), dim3(MESH_THREADS), 0, s, faces, F, V, parent, err);
    hipLaunchKernelGGL(k_cc_flatten, dim3(mv_grid(V, MESH_THREADS)), dim3(MESH_THREADS), 0, s, V, parent, err);
    hipLaunchKernelGGL(k_flag_count, dim3((unsigned)L.nbv), dim3(MESH_THREADS), 0, s, (const int*)parent, (long long)V, 0, 1, (int*)(w + L.bc));
    hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(MESH_SCAN_THREADS), 0, s, (const int*)(w + L.bc), (const int*)nullptr, (int)L.nbv,
                       (long long*)(w + L.bo), (long long*)nullptr, ncomp);
    hipLaunchKernelGGL(k_cc_dense, dim3((unsigned)L.nbv), dim3(MESH_THREADS), 0, s, (const int*)parent, V, (const long long*)(w + L.bo), dense);
    hipLaunchKernelGGL(k_cc_label_vertices, dim3(mv_grid(V, MESH_THREADS)), dim3(MESH_THREADS), 0, s, (const int*)parent, (const int*)dense, V, vert_label, cv);
    hipLaunchKernelGGL(k_cc_faces, dim3(mv_grid(F, MESH_THREADS)), dim3(MESH_THREADS), 0, s, verts, faces, F, (const int*)vert_label, face_label, cf, minface, scal);
    hipLaunchKernelGGL(k_cc_area, dim3(mv_grid(F, MESH_THREADS)), dim3(MESH_THREADS), 0, s, verts, faces, F, (const int*)face_label, acc,
                       (const unsigned long long*)scal);
    hipLaunchKernelGGL(k_cc_best_area, dim3(mv_grid(V, MESH_THREADS)), dim3(MESH_THREADS), 0, s, (const unsigned long long*)acc, (const long long*)ncomp, scal);
    hipLaunchKernelGGL(k_cc_best_face, dim3(mv_grid(V, MESH_THREADS)), dim3(MESH_THREADS), 0, s, (const unsigned long long*)acc, (const int*)minface,
                       (const long long*)ncomp, scal);
    hipLaunchKernelGGL(k_cc_result, dim3(1), dim3(1), 0, s, (const long long*)ncomp, (const unsigned long long*)scal, (const int*)face_label, (const int*)cv,
                       (const int*)cf, (const int*)err, F, (long long*)w);
    return mv_check(hipGetLastError(), "mvsdf_mesh_components");
}

int mvsdf_mesh_select(const int32_t* vert_label, const int32_t* face_label, int64_t nv, int64_t nf, int32_t label, const float* verts, const float* normals,
                      const float* colors, const int32_t* faces, void* ws, size_t ws_bytes, float* out_verts, float* out_normals, float* out_colors,
                      int32_t* out_faces, int64_t nv_cap, int64_t nf_cap, void* stream) {
    CcLayout L;
    if (!vert_label || !face_label || !verts || !faces || !ws || !out_verts || !out_faces || !cc_layout(nv, nf, &L) || (normals && !out_normals) ||
        (colors && !out_colors) || nv_cap < 0 || nf_cap < 0)
        return mv_fail(-1, "mvsdf_mesh_select: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_mesh_select: workspace too small (mvsdf_mesh_cc_workspace_bytes)");
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    long long* tot = (long long*)(w + L.scal);
    hipLaunchKernelGGL(k_flag_count, dim3((unsigned)L.nbv), dim3(MESH_THREADS), 0, s, (const int*)vert_label, (long long)nv, (int)label, 0, (int*)(w + L.bc));
    hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(MESH_SCAN_THREADS), 0, s, (const int*)(w + L.bc), (const int*)nullptr, (int)L.nbv, (long long*)(w + L.bo),
                       (long long*)nullptr, tot);
    hipLaunchKernelGGL(k_flag_count, dim3((unsigned)L.nbf), dim3(MESH_THREADS), 0, s, (const int*)face_label, (long long)nf, (int)label, 0, (int*)(w + L.bc2));
    hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(MESH_SCAN_THREADS), 0, s, (const int*)(w + L.bc2), (const int*)nullptr, (int)L.nbf, (long long*)(w + L.bo2),
                       (long long*)nullptr, tot);
    hipLaunchKernelGGL(k_sel_vertices, dim3((unsigned)L.nbv), dim3(MESH_THREADS), 0, s, (const int*)vert_label, (int)nv, (int)label, (const long long*)(w + L.bo),
                       verts, normals, colors, (int*)(w + L.vmap), out_verts, out_normals, out_colors, (long long)nv_cap);
    hipLaunchKernelGGL(k_sel_faces, dim3((unsigned)L.nbf), dim3(MESH_THREADS), 0, s, (const int*)face_label, (int)nf, (int)label, (const long long*)(w + L.bo2),
                       faces, (const int*)(w + L.vmap), out_faces, (long long)nf_cap);
    return mv_check(hipGetLastError(), "mvsdf_mesh_select");
}

}  // extern "C"
