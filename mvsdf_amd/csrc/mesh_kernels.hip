// mesh_kernels.hip -- on-device mesh extraction (reference code/evaluation/eval.py:109-125, code/utils/plots.py:150-205):
// marching cubes over an fp32 volume with arbitrary element strides, connected components of the mesh by union-find, and the compaction of one
// component.  Conventions (vertex / face order, positions, normals): mvsdf_amd/mesh.py; the triangle table: tools/gen_mc_tables.py -> mc_tables.h.
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

__device__ __forceinline__ float vat(const MeshVol& v, long long i, long long j, long long k) { return v.p[i * v.s[0] + j * v.s[1] + k * v.s[2]]; }

// the accessor of mesh_common.h's formulas
struct VolVal {
    const MeshVol& v;
    __device__ __forceinline__ float operator()(long long i, long long j, long long k) const { return vat(v, i, j, k); }
};

__device__ __forceinline__ void point_ijk(const MeshVol& v, long long p, long long& i, long long& j, long long& k) {
    const long long nyz = v.n[1] * v.n[2];
    i = p / nyz;
    const long long r = p - i * nyz;
    j = r / v.n[2];
    k = r - j * v.n[2];
}

// crossing edges owned by grid point (i, j, k): bit a = the edge to (i, j, k) + e_a crosses the level
__device__ __forceinline__ int point_edges(const MeshVol& v, long long i, long long j, long long k, bool in0) {
    return mc_point_edges(VolVal{v}, v.n, i, j, k, in0, v.level);
}

// cube index of the cell with lower corner (i, j, k) (bit c: corner (c & 1, c >> 1 & 1, c >> 2 & 1) is inside); -1 if there is no such cell
__device__ __forceinline__ int cell_index(const MeshVol& v, long long i, long long j, long long k) {
    if (i + 1 >= v.n[0] || j + 1 >= v.n[1] || k + 1 >= v.n[2]) return -1;
    return mc_cube_index(VolVal{v}, i, j, k, v.level);
}

// ---- marching cubes, pass 1: vertices and triangles per workgroup (bv / bf), or -1 in bf when the workgroup saw a non-finite value ----
__global__ __launch_bounds__(MESH_THREADS) void k_mc_count(MeshVol v, long long npts, int* __restrict__ bv, int* __restrict__ bf) {
    __shared__ int s_w[MESH_THREADS / 64];
    long long rv = 0, rf = 0;
    int bad = 0;
    for (int r = 0; r < MESH_ROUNDS; ++r) {
        const long long p = (long long)blockIdx.x * MESH_CHUNK + r * MESH_THREADS + threadIdx.x;
        int nv = 0, nt = 0;
        if (p < npts) {
            long long i, j, k;
            point_ijk(v, p, i, j, k);
            const float x = vat(v, i, j, k);
            bad |= !isfinite(x);
            nv = __popc(point_edges(v, i, j, k, x < v.level));
            const int ci = cell_index(v, i, j, k);
            if (ci >= 0) nt = mc_ntri(ci);
        }
        block_excl(nv, 2, s_w, rv);
        block_excl(nt, 3, s_w, rf);
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        bv[blockIdx.x] = (int)rv;
        bf[blockIdx.x] = bad ? -1 : (int)rf;
    }
}

// ---- pass 2: the vertex id map (id of each point's first vertex), vertices and normals ----
__global__ __launch_bounds__(MESH_THREADS) void k_mc_vertices(MeshVol v, long long npts, McGeom gm, const long long* __restrict__ ov, int* __restrict__ idmap,
                                                              float* __restrict__ verts, float* __restrict__ normals, long long nv_cap) {
    __shared__ int s_w[MESH_THREADS / 64];
    long long run = ov[blockIdx.x];
    for (int r = 0; r < MESH_ROUNDS; ++r) {
        const long long p = (long long)blockIdx.x * MESH_CHUNK + r * MESH_THREADS + threadIdx.x;
        int bits = 0;
        long long g[3] = {0, 0, 0};
        float x = 0.0f;
        if (p < npts) {
            point_ijk(v, p, g[0], g[1], g[2]);
            x = vat(v, g[0], g[1], g[2]);
            bits = point_edges(v, g[0], g[1], g[2], x < v.level);
        }
        long long id = block_excl(__popc(bits), 2, s_w, run);
        if (p >= npts) continue;
        idmap[p] = (int)id;
        for (int a = 0; a < 3; ++a) {
            if (!(bits >> a & 1)) continue;
            if (id < nv_cap) mc_vertex(VolVal{v}, v.n, g, a, x, v.level, gm, verts + id * 3, normals + id * 3);
            ++id;
        }
    }
}

// vertex id of cube edge e of the cell at (i, j, k): the owner's first id plus its crossing edges along lower axes
__device__ __forceinline__ int edge_vertex(const MeshVol& v, const int* __restrict__ idmap, long long i, long long j, long long k, int e) {
    long long q[3] = {i, j, k};
    const int a = mc_edge_owner(e, q);
    const bool in0 = vat(v, q[0], q[1], q[2]) < v.level;
    const int bits = point_edges(v, q[0], q[1], q[2], in0);
    return idmap[(q[0] * v.n[1] + q[1]) * v.n[2] + q[2]] + __popc(bits & ((1 << a) - 1));
}

// ---- pass 3: faces (int32 vertex ids), cells in linear order, each cell's triangles in table order ----
__global__ __launch_bounds__(MESH_THREADS) void k_mc_faces(MeshVol v, long long npts, const long long* __restrict__ of, const int* __restrict__ idmap,
                                                           int* __restrict__ faces, long long nf_cap) {
    __shared__ int s_w[MESH_THREADS / 64];
    long long run = of[blockIdx.x];
    for (int r = 0; r < MESH_ROUNDS; ++r) {
        const long long p = (long long)blockIdx.x * MESH_CHUNK + r * MESH_THREADS + threadIdx.x;
        long long i = 0, j = 0, k = 0;
        int ci = -1, nt = 0;
        if (p < npts) {
            point_ijk(v, p, i, j, k);
            ci = cell_index(v, i, j, k);
            if (ci >= 0) nt = mc_ntri(ci);
        }
        const long long fid = block_excl(nt, 3, s_w, run);
        for (int t = 0; t < nt; ++t) {
            if (fid + t >= nf_cap) break;
            const int base = (mc_tri_offset[ci] + t) * 3;
            for (int s = 0; s < 3; ++s) faces[(fid + t) * 3 + s] = edge_vertex(v, idmap, i, j, k, mc_tri_edges[base + s]);
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

// results: out[0] = components, out[1] = the largest one's label, out[2] / out[3] = its vertex / face counts, out[4] = 1 if a union-find loop hit its bound
__global__ void k_cc_result(const long long* __restrict__ ncomp, const unsigned long long* __restrict__ scal, const int* __restrict__ flab, const int* __restrict__ cv,
                            const int* __restrict__ cf, const int* __restrict__ err, int nf, long long* __restrict__ out) {
    const long long f = nf ? (long long)(~0ull - scal[2]) : -1;
    const int l = f >= 0 && f < nf ? flab[f] : -1;
    out[0] = ncomp[0];
    out[1] = l;
    out[2] = l >= 0 ? cv[l] : 0;
    out[3] = l >= 0 ? cf[l] : 0;
    out[4] = *err;
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
    size_t idmap, bv, bf, ov, of, total;
};

// false: a dimension below 2, or a grid whose points or workgroups the kernels cannot index
static bool mc_layout(long long nx, long long ny, long long nz, McLayout* L) {
    if (nx < 2 || ny < 2 || nz < 2) return false;
    const long long lim = 1ll << 60;
    if (nx > lim / ny || nx * ny > lim / nz) return false;
    L->npts = nx * ny * nz;
    L->nb = mv_ceil_div(L->npts, MESH_CHUNK);
    if (L->nb > INT_MAX) return false;
    WsCursor c{MESH_HDR};
    L->idmap = c.take((size_t)L->npts * 4);
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

static bool mc_vol(const float* vol, const int64_t* shape, const int64_t* strides, float level, McLayout* L, MeshVol* v) {
    if (!vol || !shape || !strides || !mc_layout(shape[0], shape[1], shape[2], L)) return false;
    v->p = vol;
    v->level = level;
    for (int a = 0; a < 3; ++a) {
        v->n[a] = shape[a];
        v->s[a] = strides[a];
    }
    return true;
}

extern "C" {

size_t mvsdf_mc_workspace_bytes(int64_t nx, int64_t ny, int64_t nz) {
    McLayout L;
    return mc_layout(nx, ny, nz, &L) ? L.total : 0;
}

int mvsdf_mc_count(const float* vol, const int64_t* shape, const int64_t* strides, float level, void* ws, size_t ws_bytes, void* stream) {
    McLayout L;
    MeshVol v;
    if (!mc_vol(vol, shape, strides, level, &L, &v) || !ws) return mv_fail(-1, "mvsdf_mc_count: bad arguments (every extent must be >= 2)");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_mc_count: workspace too small (mvsdf_mc_workspace_bytes)");
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mc_count, dim3((unsigned)L.nb), dim3(MESH_THREADS), 0, s, v, L.npts, (int*)(w + L.bv), (int*)(w + L.bf));
    hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(MESH_SCAN_THREADS), 0, s, (const int*)(w + L.bv), (const int*)(w + L.bf), (int)L.nb,
                       (long long*)(w + L.ov), (long long*)(w + L.of), (long long*)w);
    return mv_check(hipGetLastError(), "mvsdf_mc_count");
}

int mvsdf_mc_emit(const float* vol, const int64_t* shape, const int64_t* strides, float level, const float* spacing, const float* origin, void* ws, size_t ws_bytes,
                  float* verts, float* normals, int32_t* faces, int64_t nv_cap, int64_t nf_cap, void* stream) {
    McLayout L;
    MeshVol v;
    if (!mc_vol(vol, shape, strides, level, &L, &v) || !ws || !spacing || !origin || nv_cap < 0 || nf_cap < 0 || (nv_cap && (!verts || !normals)) || (nf_cap && !faces))
        return mv_fail(-1, "mvsdf_mc_emit: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_mc_emit: workspace too small (mvsdf_mc_workspace_bytes)");
    McGeom gm;
    for (int a = 0; a < 3; ++a) {
        gm.sp[a] = spacing[a];
        gm.org[a] = origin[a];
    }
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mc_vertices, dim3((unsigned)L.nb), dim3(MESH_THREADS), 0, s, v, L.npts, gm, (const long long*)(w + L.ov), (int*)(w + L.idmap),
                       verts, normals, (long long)nv_cap);
    hipLaunchKernelGGL(k_mc_faces, dim3((unsigned)L.nb), dim3(MESH_THREADS), 0, s, v, L.npts, (const long long*)(w + L.of), (const int*)(w + L.idmap),
                       faces, (long long)nf_cap);
    return mv_check(hipGetLastError(), "mvsdf_mc_emit");
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
