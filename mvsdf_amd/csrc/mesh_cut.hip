// mesh_cut.hip -- on-device mesh trimming (reference code/mesh_cut/mesh_cut.py): a minimum s-t cut over the faces of a mesh, then the compaction of the
// faces that stay.  Python: mvsdf_amd/mesh.py (Mesh.cut_mask / Mesh.trim), which states the semantics; tests/maxflow_ref.py restates them in numpy.
//
// The network (mesh_cut.py): face f is a node; c_f = (r_a + r_b + r_c) / 3 in fp64 over its vertices' red channels; c_f > thresh / 255 gives an arc
// source -> f of capacity 1, else f -> sink of capacity 1.  Every half-edge of f whose twin lies in face g gives the arc pair f <-> g of capacity smooth,
// so faces sharing one edge are joined by 2 * smooth each way.  The faces removed are S* = the faces reachable from the source in the residual graph of
// a maximum flow (the source side of the smallest minimum cut; the same for every maximum flow).
//
// Algorithm: lock-free push-relabel (Hong) on the REVERSED network -- every dark face (c_f <= thresh / 255) starts with excess 1, every bright face
// drains 1 into the target (the original source), the pairwise arcs are symmetric and stay as they are.  One residual slot per half-edge (slot k of f
// is the arc to its twin's face; the twin's slot is the reverse arc), plus each bright face's target arc.  Rounds alternate an exact global relabel
// (BFS distance to the target over residual arcs, by Bellman-Ford relaxation: every workgroup relaxes a contiguous face range in LDS until it is stable,
// launches repeat until one changes nothing) with one push launch of at most CUT_PUSH_ITERS push / relabel steps per face.  The loop ends when the
// relabel finds no face with excess that can reach the target: the preflow is then maximum, its value is the flow into the target, and the faces
// that can still reach the target are exactly S* (phase 2, returning the excess, changes no residual arc on that side).  Heights only steer progress;
// the result rests on the capacity / excess bookkeeping (atomics) and the exact final relabel.
//
// Every device loop is bounded; the host loop is bounded by a limit derived from F and reports running into it instead of spinning.
#include "geom_prims.h"

#define CUT_THREADS 256
#define CUT_GR_ITEMS 8                                // faces per lane in the relabel launch
#define CUT_GR_CHUNK (CUT_THREADS * CUT_GR_ITEMS)     // faces per relabel workgroup
#define CUT_GR_BATCH 4                                // relabel launches per host check
#define CUT_PUSH_ITERS 64
#define CUT_HDR 256                                   // bytes at the start of the workspace: int64 results the host reads
static_assert(MVSDF_CUT_H_WORDS * 8 <= CUT_HDR, "the result words fit the header");
#define CUT_EMPTY 0xffffffffffffffffull

#define RLX(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define RLX_ST(p, x) __hip_atomic_store((p), (x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

__device__ __forceinline__ unsigned long long he_key(int u, int v) { return ((unsigned long long)(unsigned)u << 32) | (unsigned)v; }

__device__ __forceinline__ unsigned long long he_hash(unsigned long long k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    return k ^ (k >> 33);
}

// a face's vertex ids, and the error bits they raise (0: usable)
__device__ __forceinline__ int face_ids(const int* __restrict__ faces, long long f, int nv, int* id) {
    int bad = 0;
    for (int s = 0; s < 3; ++s) {
        id[s] = faces[f * 3 + s];
        if (id[s] < 0 || id[s] >= nv) bad |= MVSDF_CUT_ERR_RANGE;
    }
    if (!bad && (id[0] == id[1] || id[1] == id[2] || id[0] == id[2])) bad |= MVSDF_CUT_ERR_REPEATED;
    return bad;
}

// ---- adjacency, pass 1: every half-edge (id[k], id[k + 1]) of every usable face into an open-addressing table (keys are unique, else MVSDF_CUT_ERR_DUP_EDGE) ----
__global__ __launch_bounds__(CUT_THREADS) void k_cut_insert(const int* __restrict__ faces, int nf, int nv, unsigned long long* keys, int* __restrict__ vals,
                                                             unsigned long long tmask, int* err) {
    const long long f = (long long)blockIdx.x * CUT_THREADS + threadIdx.x;
    if (f >= nf) return;
    int id[3];
    const int bad = face_ids(faces, f, nv, id);
    if (bad) {
        atomicOr(err, bad);
        return;
    }
    for (int k = 0; k < 3; ++k) {
        const unsigned long long key = he_key(id[k], id[(k + 1) % 3]);
        unsigned long long slot = he_hash(key) & tmask;
        bool done = false;
        for (unsigned long long probe = 0; probe <= tmask; ++probe) {
            const unsigned long long prev = atomicCAS(keys + slot, CUT_EMPTY, key);
            if (prev == CUT_EMPTY) {
                vals[slot] = (int)(f * 3 + k);
                done = true;
                break;
            }
            if (prev == key) {
                atomicOr(err, MVSDF_CUT_ERR_DUP_EDGE);
                done = true;
                break;
            }
            slot = (slot + 1) & tmask;
        }
        if (!done) atomicOr(err, MVSDF_CUT_ERR_HASH);
    }
}

// ---- pass 2: twins (twin[f * 3 + k] = the reverse half-edge's id g * 3 + k', or -1 on the boundary), residual capacities, terminal classes ----
// tcap[f] = 1 for a bright face (its arc to the target), excess[f] = 1 for a dark one.
__global__ __launch_bounds__(CUT_THREADS) void k_cut_link(const int* __restrict__ faces, const float* __restrict__ colors, int nf, int nv, double thr, int cap2,
                                                           const unsigned long long* __restrict__ keys, const int* __restrict__ vals, unsigned long long tmask,
                                                           int* __restrict__ twin, int* __restrict__ cf, int* __restrict__ tcap, int* __restrict__ excess) {
    const long long f = (long long)blockIdx.x * CUT_THREADS + threadIdx.x;
    if (f >= nf) return;
    int id[3];
    if (face_ids(faces, f, nv, id)) return;                       // pass 1 raised the error; nothing below reads through bad ids
    for (int k = 0; k < 3; ++k) {
        const unsigned long long key = he_key(id[(k + 1) % 3], id[k]);
        unsigned long long slot = he_hash(key) & tmask;
        int t = -1;
        for (unsigned long long probe = 0; probe <= tmask; ++probe) {
            const unsigned long long kk = keys[slot];
            if (kk == key) {
                t = vals[slot];
                break;
            }
            if (kk == CUT_EMPTY) break;
            slot = (slot + 1) & tmask;
        }
        twin[f * 3 + k] = t;
        cf[f * 3 + k] = t >= 0 ? cap2 : 0;
    }
    const double c = ((double)colors[(long long)id[0] * 3] + (double)colors[(long long)id[1] * 3] + (double)colors[(long long)id[2] * 3]) / 3.0;
    const bool bright = c > thr;
    tcap[f] = bright ? 1 : 0;
    excess[f] = bright ? 0 : 1;
}

// ---- global relabel: h = BFS distance to the target over residual arcs (1 for a face whose target arc is open), inf = cannot reach it ----
__global__ __launch_bounds__(CUT_THREADS) void k_cut_gr_init(int nf, const int* __restrict__ tcap, int* __restrict__ h, int inf) {
    const long long f = (long long)blockIdx.x * CUT_THREADS + threadIdx.x;
    if (f < nf) h[f] = tcap[f] > 0 ? 1 : inf;
}

// One relaxation launch.  Values only decrease and every value is h[g] + 1 for a value some neighbour held, so each stays an upper bound of the
// distance, and a launch in which no workgroup changes anything has reached the fixed point.  Neighbours outside the workgroup's range are read
// once, at the start (a later launch sees what they become); the in-range neighbours are resolved to LDS slots once, so the loop runs in LDS.
// changed / active: this launch's flags (pre-zeroed); active counts the faces with excess that can reach the target (exact once the launch
// changes nothing).
__global__ __launch_bounds__(CUT_THREADS) void k_cut_gr_relax(int nf, const int* __restrict__ twin, const int* __restrict__ cf, const int* __restrict__ excess,
                                                               int* h, int inf, int* __restrict__ changed, int* __restrict__ active) {
    __shared__ int sh[CUT_GR_CHUNK];
    const long long base = (long long)blockIdx.x * CUT_GR_CHUNK;
    int nb[CUT_GR_ITEMS][3];                                      // LDS slot of each in-range residual neighbour, -1 for none
#pragma unroll
    for (int q = 0; q < CUT_GR_ITEMS; ++q) {
        const int i = q * CUT_THREADS + threadIdx.x;
        const long long f = base + i;
        int v = inf;
        if (f < nf) {
            v = RLX(h + f);
            for (int k = 0; k < 3; ++k) {
                nb[q][k] = -1;
                const int t = twin[f * 3 + k];
                if (t < 0 || cf[f * 3 + k] <= 0) continue;
                const long long g = t / 3;
                if (g >= base && g < base + CUT_GR_CHUNK) {
                    nb[q][k] = (int)(g - base);
                } else {
                    const int hg = RLX(h + g);
                    if (hg < inf && hg + 1 < v) v = hg + 1;
                }
            }
        } else {
            nb[q][0] = nb[q][1] = nb[q][2] = -1;
        }
        sh[i] = v;
    }
    __syncthreads();
    int any_change = 0;
#pragma unroll
    for (int q = 0; q < CUT_GR_ITEMS; ++q) {
        const long long f = base + q * CUT_THREADS + threadIdx.x;
        if (f < nf && sh[q * CUT_THREADS + threadIdx.x] != RLX(h + f)) any_change = 1;   // an outside neighbour lowered it
    }
    any_change = __syncthreads_or(any_change);
    for (int it = 0; it < CUT_GR_CHUNK; ++it) {                   // a chain inside the range is at most CUT_GR_CHUNK long
        int moved = 0;
#pragma unroll
        for (int q = 0; q < CUT_GR_ITEMS; ++q) {
            const int i = q * CUT_THREADS + threadIdx.x;
            int best = sh[i];
            if (best <= 1) continue;
            for (int k = 0; k < 3; ++k) {
                if (nb[q][k] < 0) continue;
                const int hg = sh[nb[q][k]];
                if (hg < inf && hg + 1 < best) best = hg + 1;
            }
            if (best < sh[i]) {
                sh[i] = best;
                moved = 1;
            }
        }
        if (!__syncthreads_or(moved)) break;
        any_change = 1;
    }
    int act = 0;
    for (int q = 0; q < CUT_GR_ITEMS; ++q) {
        const int i = q * CUT_THREADS + threadIdx.x;
        const long long f = base + i;
        if (f >= nf) continue;
        if (any_change) RLX_ST(h + f, sh[i]);
        act += excess[f] > 0 && sh[i] < inf;
    }
    for (int o = 32; o; o >>= 1) act += __shfl_xor(act, o);
    if ((threadIdx.x & 63) == 0 && act) atomicAdd(active, act);
    if (threadIdx.x == 0 && any_change) atomicOr(changed, 1);
}

// ---- push / relabel (Hong's lock-free rule): an active face pushes to its lowest residual neighbour if it is higher than it, else relabels to it + 1.
// Only face f lowers excess[f], cf[f * 3 + k] and tcap[f]; others only raise the first two (atomics), so every push keeps the preflow valid. ----
__global__ __launch_bounds__(CUT_THREADS) void k_cut_push(int nf, const int* __restrict__ twin, int* cf, int* __restrict__ tcap, int* excess, int* h, int inf) {
    const long long f = (long long)blockIdx.x * CUT_THREADS + threadIdx.x;
    for (int it = 0; it < CUT_PUSH_ITERS; ++it) {
        int e = 0, hu = inf;
        if (f < nf) {
            e = RLX(excess + f);
            hu = RLX(h + f);
        }
        const bool act = e > 0 && hu < inf;
        if (!__any(act)) break;
        if (!act) continue;
        int hmin = inf, slot = -1, cap = 0;
        if (tcap[f] > 0) {
            hmin = 0;
            slot = 3;
            cap = tcap[f];
        } else {
            for (int k = 0; k < 3; ++k) {
                const int t = twin[f * 3 + k];
                if (t < 0) continue;
                const int c = RLX(cf + f * 3 + k);
                if (c <= 0) continue;
                const int hg = RLX(h + t / 3);
                if (hg < hmin) {
                    hmin = hg;
                    slot = k;
                    cap = c;
                }
            }
        }
        if (slot < 0 || hmin >= inf) {
            RLX_ST(h + f, inf);                                   // no residual arc to a face that can reach the target
        } else if (hu > hmin) {
            const int d = e < cap ? e : cap;
            if (slot == 3) {
                tcap[f] -= d;
            } else {
                const int t = twin[f * 3 + slot];
                atomicSub(cf + f * 3 + slot, d);
                atomicAdd(cf + t, d);
                atomicAdd(excess + t / 3, d);
            }
            atomicSub(excess + f, d);
        } else {
            RLX_ST(h + f, hmin + 1 < inf ? hmin + 1 : inf);
        }
    }
}

// ---- results: removed[f] = f can reach the target (f in S*); face labels (1 = kept), vertex labels (1 = used by a kept face) for the compaction ----
__global__ __launch_bounds__(CUT_THREADS) void k_cut_mark(int nf, const int* __restrict__ faces, const int* __restrict__ h, int inf,
                                                           unsigned char* __restrict__ removed, int* __restrict__ flab, int* __restrict__ vlab,
                                                           unsigned long long* __restrict__ sums) {
    const long long f = (long long)blockIdx.x * CUT_THREADS + threadIdx.x;
    unsigned long long rm = 0;
    if (f < nf) {
        const bool r = h[f] < inf;
        removed[f] = r;
        flab[f] = !r;
        if (!r)
            for (int s = 0; s < 3; ++s) vlab[faces[f * 3 + s]] = 1;   // every writer stores the same value
        rm = r;
    }
    for (int o = 32; o; o >>= 1) rm += __shfl_xor(rm, o);
    if ((threadIdx.x & 63) == 0 && rm) atomicAdd(sums + 1, rm);
}

// flow = the bright faces whose target arc is saturated (the preflow's value); kept vertices = the labels set above
__global__ __launch_bounds__(CUT_THREADS) void k_cut_sums(int nf, int nv, const int* __restrict__ tcap, const int* __restrict__ excess0, const int* __restrict__ vlab,
                                                           unsigned long long* __restrict__ sums) {
    const long long x = (long long)blockIdx.x * CUT_THREADS + threadIdx.x;
    unsigned long long fl = x < nf && excess0[x] == 0 && tcap[x] == 0, kv = x < nv && vlab[x] == 1;
    for (int o = 32; o; o >>= 1) {
        fl += __shfl_xor(fl, o);
        kv += __shfl_xor(kv, o);
    }
    if ((threadIdx.x & 63) == 0) {
        if (fl) atomicAdd(sums, fl);
        if (kv) atomicAdd(sums + 2, kv);
    }
}

__global__ __launch_bounds__(CUT_THREADS) void k_cut_zero(int n, int* __restrict__ a) {
    const long long x = (long long)blockIdx.x * CUT_THREADS + threadIdx.x;
    if (x < n) a[x] = 0;
}

// ---- workspace layout (every region 256-byte aligned) ----
struct CutLayout {
    unsigned long long tsize;                                     // half-edge table slots (a power of two >= 6 F)
    size_t keys, vals, twin, cf, tcap, excess0, excess, h, flags, flab, vlab, sel, sel_bytes, total;
};

// 1 <= nv, nf; F <= INT_MAX / 8 so that half-edge ids and heights fit int32
static bool cut_layout(long long nv, long long nf, CutLayout* L) {
    if (nv < 1 || nf < 1 || nv > INT_MAX || nf > INT_MAX / 8) return false;
    L->tsize = 1;
    while (L->tsize < (unsigned long long)(6 * nf)) L->tsize <<= 1;
    L->sel_bytes = mvsdf_mesh_cc_workspace_bytes(nv, nf);
    if (!L->sel_bytes) return false;
    WsCursor c{CUT_HDR};
    L->keys = c.take(L->tsize * 8);
    L->vals = c.take(L->tsize * 4);
    L->twin = c.take((size_t)nf * 12);
    L->cf = c.take((size_t)nf * 12);
    L->tcap = c.take((size_t)nf * 4);
    L->excess0 = c.take((size_t)nf * 4);
    L->excess = c.take((size_t)nf * 4);
    L->h = c.take((size_t)nf * 4);
    L->flags = c.take(2 * CUT_GR_BATCH * 4 + 4 * 8);
    L->flab = c.take((size_t)nf * 4);
    L->vlab = c.take((size_t)nv * 4);
    L->sel = c.take(L->sel_bytes);
    L->total = c.o;
    return true;
}

extern "C" {

size_t mvsdf_mesh_cut_workspace_bytes(int64_t nv, int64_t nf) {
    CutLayout L;
    return cut_layout(nv, nf, &L) ? L.total : 0;
}

int mvsdf_mesh_cut(const float* colors, const int32_t* faces, int64_t nv, int64_t nf, int32_t thresh, int32_t smooth, void* ws, size_t ws_bytes,
                   uint8_t* removed, void* stream) {
    CutLayout L;
    if (!colors || !faces || !ws || !removed || !cut_layout(nv, nf, &L)) return mv_fail(-1, "mvsdf_mesh_cut: bad arguments");
    if (smooth < 0 || smooth > INT_MAX / 6) return mv_fail(-1, "mvsdf_mesh_cut: smooth must be in [0, INT_MAX / 6]");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_mesh_cut: workspace too small (mvsdf_mesh_cut_workspace_bytes)");
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    const int F = (int)nf, V = (int)nv, inf = F + 1;
    unsigned long long* keys = (unsigned long long*)(w + L.keys);
    int* vals = (int*)(w + L.vals);
    int* twin = (int*)(w + L.twin);
    int* cf = (int*)(w + L.cf);
    int* tcap = (int*)(w + L.tcap);
    int* excess0 = (int*)(w + L.excess0);                         // the initial excess (1 = dark face), kept for the flow sum
    int* excess = (int*)(w + L.excess);
    int* h = (int*)(w + L.h);
    int* flags = (int*)(w + L.flags);                             // [0, B): changed per relabel launch, [B, 2B): active per launch
    int* err = flags + 2 * CUT_GR_BATCH;
    unsigned long long* sums = (unsigned long long*)(w + L.flags + 2 * CUT_GR_BATCH * 4 + 8);
    long long hdr[MVSDF_CUT_H_WORDS] = {};
    const unsigned gf = mv_grid(F, CUT_THREADS), gr = mv_grid(F, CUT_GR_CHUNK);
    int rc;
    if ((rc = mv_check(hipMemsetAsync(keys, 0xff, L.tsize * 8, s), "mvsdf_mesh_cut"))) return rc;
    if ((rc = mv_check(hipMemsetAsync(w + L.flags, 0, 2 * CUT_GR_BATCH * 4 + 4 * 8, s), "mvsdf_mesh_cut"))) return rc;
    hipLaunchKernelGGL(k_cut_insert, dim3(gf), dim3(CUT_THREADS), 0, s, faces, F, V, keys, vals, (unsigned long long)(L.tsize - 1), err);
    hipLaunchKernelGGL(k_cut_link, dim3(gf), dim3(CUT_THREADS), 0, s, faces, colors, F, V, (double)thresh / 255.0, 2 * smooth,
                       (const unsigned long long*)keys, (const int*)vals, (unsigned long long)(L.tsize - 1), twin, cf, tcap, excess);
    if ((rc = mv_check(hipGetLastError(), "mvsdf_mesh_cut"))) return rc;
    int e = 0;
    if ((rc = mv_read(&e, err, 4, s, "mvsdf_mesh_cut"))) return rc;
    hdr[MVSDF_CUT_H_ERR] = e;
    if (!e) {
        if ((rc = mv_check(hipMemcpyAsync(excess0, excess, (size_t)F * 4, hipMemcpyDeviceToDevice, s), "mvsdf_mesh_cut"))) return rc;
        // Each round either moves excess or raises a height; the limit is a safety net far above what the meshes we know need.
        const long long max_rounds = 4ll * F + 64, max_relabel = (long long)F + 2;
        bool done = false;
        while (!done) {
            hipLaunchKernelGGL(k_cut_gr_init, dim3(gf), dim3(CUT_THREADS), 0, s, F, (const int*)tcap, h, inf);
            long long launches = 0;
            bool settled = false;
            int active = 0;
            while (!settled) {
                if (launches >= max_relabel) {
                    hdr[MVSDF_CUT_H_ERR] |= MVSDF_CUT_ERR_RELABEL;
                    break;
                }
                if ((rc = mv_check(hipMemsetAsync(flags, 0, 2 * CUT_GR_BATCH * 4, s), "mvsdf_mesh_cut"))) return rc;
                for (int b = 0; b < CUT_GR_BATCH; ++b)
                    hipLaunchKernelGGL(k_cut_gr_relax, dim3(gr), dim3(CUT_THREADS), 0, s, F, (const int*)twin, (const int*)cf, (const int*)excess, h, inf,
                                       flags + b, flags + CUT_GR_BATCH + b);
                if ((rc = mv_check(hipGetLastError(), "mvsdf_mesh_cut"))) return rc;
                int fl[2 * CUT_GR_BATCH];
                if ((rc = mv_read(fl, flags, sizeof(fl), s, "mvsdf_mesh_cut"))) return rc;
                for (int b = 0; b < CUT_GR_BATCH && !settled; ++b) {
                    ++launches;
                    if (!fl[b]) {
                        settled = true;
                        active = fl[CUT_GR_BATCH + b];
                    }
                }
            }
            hdr[MVSDF_CUT_H_RELABELS] += launches;
            if (!settled) break;
            if (!active) {
                done = true;
                break;
            }
            if (hdr[MVSDF_CUT_H_ROUNDS] >= max_rounds) {
                hdr[MVSDF_CUT_H_ERR] |= MVSDF_CUT_ERR_ROUNDS;
                break;
            }
            hipLaunchKernelGGL(k_cut_push, dim3(gf), dim3(CUT_THREADS), 0, s, F, (const int*)twin, cf, tcap, excess, h, inf);
            ++hdr[MVSDF_CUT_H_ROUNDS];
        }
        if (done) {
            hipLaunchKernelGGL(k_cut_zero, dim3(mv_grid(V, CUT_THREADS)), dim3(CUT_THREADS), 0, s, V, (int*)(w + L.vlab));
            hipLaunchKernelGGL(k_cut_mark, dim3(gf), dim3(CUT_THREADS), 0, s, F, faces, (const int*)h, inf, (unsigned char*)removed,
                               (int*)(w + L.flab), (int*)(w + L.vlab), sums);
            hipLaunchKernelGGL(k_cut_sums, dim3(mv_grid(F > V ? F : V, CUT_THREADS)), dim3(CUT_THREADS), 0, s, F, V, (const int*)tcap, (const int*)excess0,
                               (const int*)(w + L.vlab), sums);
            if ((rc = mv_check(hipGetLastError(), "mvsdf_mesh_cut"))) return rc;
            unsigned long long sm[3];
            if ((rc = mv_read(sm, sums, sizeof(sm), s, "mvsdf_mesh_cut"))) return rc;
            hdr[MVSDF_CUT_H_FLOW] = (long long)sm[0];
            hdr[MVSDF_CUT_H_REMOVED] = (long long)sm[1];
            hdr[MVSDF_CUT_H_KEPT_VERTS] = (long long)sm[2];
        }
    }
    return mv_write_header(w, hdr, MVSDF_CUT_H_WORDS, s, "mvsdf_mesh_cut");
}

int mvsdf_mesh_trim(const float* verts, const float* normals, const float* colors, const int32_t* faces, int64_t nv, int64_t nf, void* ws, size_t ws_bytes,
                    float* out_verts, float* out_normals, float* out_colors, int32_t* out_faces, int64_t nv_cap, int64_t nf_cap, void* stream) {
    CutLayout L;
    if (!verts || !faces || !ws || !cut_layout(nv, nf, &L)) return mv_fail(-1, "mvsdf_mesh_trim: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_mesh_trim: workspace too small (mvsdf_mesh_cut_workspace_bytes)");
    char* w = (char*)ws;
    return mvsdf_mesh_select((const int32_t*)(w + L.vlab), (const int32_t*)(w + L.flab), nv, nf, 1, verts, normals, colors, faces, w + L.sel, L.sel_bytes,
                             out_verts, out_normals, out_colors, out_faces, nv_cap, nf_cap, stream);
}

}  // extern "C"
