// basic.hip -- weight-norm fold + MFMA packing, camera rays, the stand-alone tracing-MLP kernel and the device self-test of det_math.  The packs' layout and
// values are pack_layout.h's: the kernels here only choose where an element comes from (global W, its transpose, or k_step_prologue's LDS tile) and where
// the block goes.  C ABI entry points for these live in the middle (see include/mvsdf_hip.h), the training step's prologue at the bottom.
#include <stdlib.h>
#include <string.h>
#include <type_traits>
#include "tile_engine.h"
#include "trace_params.h"
#include "capi_util.h"
#include "det_math_pk.h"
#include "step_internal.h"

// ---- weight norm (idr.py:70-71): sum of squares of one row [K] by one wave.  The row is loaded coalesced in chunks of 64; every lane then walks a chunk through
// v_readlane in ascending k (uniform i) -- the SAME k-ascending fmaf chain as the CPU restatement (bit-exact), at ~1 us per row. ----
__device__ __forceinline__ float mv_norm_chain(const float* __restrict__ vr, int K, int lane) {
    float ss = 0.0f;
    for (int k0 = 0; k0 < K; k0 += 64) {
        const float mine = (k0 + lane < K) ? vr[k0 + lane] : 0.0f;
        const int n = min(64, K - k0);
        for (int i = 0; i < n; ++i) {
            const float x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine), i));
            ss = fmaf(x, x, ss);
        }
    }
    return ss;
}

// ---- packs.  Element sources: (o, k) of the matrix being packed -> its value, +0 outside it.
struct MvSrcW {                                     // global W [N][K], or (tr) its transpose: out = K, in = N
    const float* w; int N, K, tr;
    __device__ int No() const { return tr ? K : N; }
    __device__ int Ko() const { return tr ? N : K; }
    __device__ float operator()(int o, int k) const { return (o < No() && k < Ko()) ? (tr ? w[(size_t)k * K + o] : w[(size_t)o * K + k]) : 0.0f; }
};
// A whole pack, grid-stride over its flat index: KW = 16 (fp32 fragments) or 32 (bf16), TERMS fragments per k-block; val(w, term) -> the stored element
template <int KW, int TERMS, class T, class SRC, class VAL>
__device__ __forceinline__ void mv_pack_flat(T* __restrict__ dst, const SRC src, const VAL val) {
    const int KB = KW == 16 ? mv_kpad(src.Ko()) / 16 : mv_bf_kb(src.Ko());
    const size_t total = (size_t)TERMS * mv_ceil16(src.No()) * KB * KW;
    constexpr int SH = KW == 16 ? 8 : 9;                                     // 256- / 512-element blocks
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const MvBlock b = mv_block_at(idx >> SH, KB, TERMS);
        const int e = (int)idx & ((1 << SH) - 1);
        const MvFrag f = KW == 16 ? mv_frag_f32(e) : mv_frag_bf16(e);
        dst[idx] = val(src(b.ct * 16 + f.row, b.kb * KW + f.k), b.term);
    }
}
// One tile row of a pack (all KB k-blocks of 16 rows) from k_step_prologue's LDS tile [16][ld] of those rows (rows beyond the matrix are zero there)
template <int KW, int TERMS, class T, class VAL>
__device__ __forceinline__ void mv_pack_tile_row(T* __restrict__ dst, int KB, const float* tile, int ld, int K, int tid, const VAL val) {
    constexpr int SH = KW == 16 ? 8 : 9;
    for (int idx = tid; idx < (KB * TERMS) << SH; idx += 1024) {
        const int blk = idx >> SH, term = blk % TERMS, kb = blk / TERMS, e = idx & ((1 << SH) - 1);      // (TERMS is a constant: no division instruction)
        const MvFrag f = KW == 16 ? mv_frag_f32(e) : mv_frag_bf16(e);
        const int k = kb * KW + f.k;
        dst[idx] = val(k < K ? tile[f.row * ld + k] : 0.0f, term);
    }
}
struct MvValF32 { __device__ float operator()(float w, int) const { return w; } };
struct MvValRound { __device__ float operator()(float w, int) const { return mv_bf_round(w); } };
struct MvValBf16 { __device__ uint16_t operator()(float w, int) const { return mv_f2bf(w); } };
struct MvValX3 { __device__ uint16_t operator()(float w, int term) const { return mv_x3_term(w, term); } };

// ---- whole-network variants: one launch folds / packs every layer (blockIdx.y selects the layer); the layer list may span several
// networks (SDF + rendering net of a step: 9 + 5 layers) ----
#define MV_FOLD_MAXL 24
struct FoldNetArgs {
    int n_layers;
    const float* v[MV_FOLD_MAXL]; const float* g[MV_FOLD_MAXL]; const float* dW[MV_FOLD_MAXL];
    float* w[MV_FOLD_MAXL]; float* wp[MV_FOLD_MAXL]; float* wpT[MV_FOLD_MAXL]; float* dv[MV_FOLD_MAXL]; float* dg[MV_FOLD_MAXL];
    const float* db[MV_FOLD_MAXL]; float* dbias[MV_FOLD_MAXL];      // backward only: bias gradients routed to their sink (optional)
    int N[MV_FOLD_MAXL], K[MV_FOLD_MAXL];
    int accumulate;                                       // backward only: add into dv / dg / dbias instead of overwriting
};

__global__ __launch_bounds__(256) void k_fold_net(FoldNetArgs a) {
    const int l = blockIdx.y, N = a.N[l], K = a.K[l];
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= N) return;
    const float* vr = a.v[l] + (size_t)j * K;
    if (!a.g[l]) {                                              // no weight norm for this layer (weight_norm=False): w = v
        float* wr0 = a.w[l] + (size_t)j * K;
        for (int k = lane; k < K; k += 64) wr0[k] = vr[k];
        return;
    }
    const float s = a.g[l][j] / sqrtf(mv_norm_chain(vr, K, lane));
    float* wr = a.w[l] + (size_t)j * K;
    for (int k = lane; k < K; k += 64) wr[k] = vr[k] * s;
}

__global__ void k_pack_net(FoldNetArgs a) {
    const int l = blockIdx.y >> 1, transposed = blockIdx.y & 1;
    float* wp = transposed ? a.wpT[l] : a.wp[l];
    if (wp) mv_pack_flat<16, 1>(wp, MvSrcW{a.w[l], a.N[l], a.K[l], transposed}, MvValF32());
}

__global__ void k_fold_bwd_net(FoldNetArgs a) {
    const int l = blockIdx.y, N = a.N[l], K = a.K[l];
    const int j = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= N) return;
    const float* vr = a.v[l] + (size_t)j * K;
    const float* dr = a.dW[l] + (size_t)j * K;
    if (!a.g[l]) {                                              // w = v: dv = dW, no dg
        float* dv0 = a.dv[l] + (size_t)j * K;
        for (int k = lane; k < K; k += 64) dv0[k] = a.accumulate ? dv0[k] + dr[k] : dr[k];
        if (lane == 0 && a.db[l]) a.dbias[l][j] = a.accumulate ? a.dbias[l][j] + a.db[l][j] : a.db[l][j];
        return;
    }
    float* dvr = a.dv[l] + (size_t)j * K;
    const bool acc = a.accumulate != 0;
    if (K <= 64 * 9) {                                          // the row's three operands once, all requested up front (clamped addresses), kept in registers
        float vv[9], dd[9], old[9];
        const float gj = a.g[l][j];
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            const int k = 64 * c + lane, kc = k < K ? k : K - 1;
            const float x = vr[kc], y = dr[kc], z = acc ? dvr[kc] : 0.0f;
            vv[c] = k < K ? x : 0.0f; dd[c] = k < K ? y : 0.0f; old[c] = z;
        }
        float ss = 0.f, dot = 0.f;
#pragma unroll
        for (int c = 0; c < 9; ++c) if (64 * c < K) { ss = fmaf(vv[c], vv[c], ss); dot = fmaf(dd[c], vv[c], dot); }
        for (int o = 32; o > 0; o >>= 1) { ss += __shfl_xor(ss, o); dot += __shfl_xor(dot, o); }
        const float inv = 1.0f / sqrtf(ss);
        const float dgj = dot * inv, s = gj * inv;
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            const int k = 64 * c + lane;
            if (k < K) { const float t = s * (dd[c] - dgj * vv[c] * inv); dvr[k] = acc ? old[c] + t : t; }
        }
        if (lane == 0) {
            a.dg[l][j] = acc ? a.dg[l][j] + dgj : dgj;
            if (a.db[l]) a.dbias[l][j] = acc ? a.dbias[l][j] + a.db[l][j] : a.db[l][j];
        }
        return;
    }
    float ss = 0.f, dot = 0.f;
    for (int k = lane; k < K; k += 64) { ss = fmaf(vr[k], vr[k], ss); dot = fmaf(dr[k], vr[k], dot); }
    for (int o = 32; o > 0; o >>= 1) { ss += __shfl_xor(ss, o); dot += __shfl_xor(dot, o); }
    const float inv = 1.0f / sqrtf(ss);
    const float dgj = dot * inv, s = a.g[l][j] * inv;
    for (int k = lane; k < K; k += 64) {
        const float t = s * (dr[k] - dgj * vr[k] * inv);
        dvr[k] = acc ? dvr[k] + t : t;
    }
    if (lane == 0) {
        a.dg[l][j] = acc ? a.dg[l][j] + dgj : dgj;
        if (a.db[l]) a.dbias[l][j] = acc ? a.dbias[l][j] + a.db[l][j] : a.db[l][j];
    }
}

// backward of the fold: one wave per row.
__global__ void k_fold_bwd(const float* __restrict__ v, const float* __restrict__ g, const float* __restrict__ dW, int N, int K,
                           float* __restrict__ dv, float* __restrict__ dg) {
    const int j = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= N) return;
    const float* vr = v + (size_t)j * K;
    const float* dr = dW + (size_t)j * K;
    float ss = 0.f, dot = 0.f;
    for (int k = lane; k < K; k += 64) { ss = fmaf(vr[k], vr[k], ss); dot = fmaf(dr[k], vr[k], dot); }
    for (int o = 32; o > 0; o >>= 1) { ss += __shfl_xor(ss, o); dot += __shfl_xor(dot, o); }
    const float nrm = sqrtf(ss), inv = 1.0f / nrm;
    const float dgj = dot * inv;                         // dW . v_hat
    const float a = g[j] * inv;
    for (int k = lane; k < K; k += 64) dv[(size_t)j * K + k] = a * (dr[k] - dgj * vr[k] * inv);
    if (lane == 0) dg[j] = dgj;
}

// ---- rend_util.get_camera_params + lift (rend_util.py:48-75, 87-100): ray idx of B * P; the first ray of a view writes the view's camera centre ----
__device__ __forceinline__ void mv_camera_ray(const float* __restrict__ uv, const float* __restrict__ pose, const float* __restrict__ Kin, int P, int idx,
                                              float* __restrict__ dirs, float* __restrict__ cam_loc) {
    const int b = idx / P;
    const float* p = pose + 16 * b;
    const float* k = Kin + 16 * b;
    const float fx = k[0], fy = k[5], cx = k[2], cy = k[6], sk = k[1];
    const float cl[3] = {p[3], p[7], p[11]};
    if (idx == b * P) { cam_loc[3 * b] = cl[0]; cam_loc[3 * b + 1] = cl[1]; cam_loc[3 * b + 2] = cl[2]; }
    const float x = uv[2 * (size_t)idx] + 0.5f, y = uv[2 * (size_t)idx + 1] + 0.5f, z = 1.0f;
    const float xl = (x - cx + cy * sk / fy - sk * y / fy) / fx * z;
    const float yl = (y - cy) / fy * z;
    const float h[4] = {xl, yl, z, 1.0f};
    float wv[3];
    for (int r = 0; r < 3; ++r) {
        float acc = 0.0f;
        for (int c = 0; c < 4; ++c) acc = fmaf(p[4 * r + c], h[c], acc);
        wv[r] = acc - cl[r];
    }
    float nn = sqrtf(wv[0] * wv[0] + wv[1] * wv[1] + wv[2] * wv[2]);
    if (nn < 1e-12f) nn = 1e-12f;
    dirs[3 * (size_t)idx] = wv[0] / nn;
    dirs[3 * (size_t)idx + 1] = wv[1] / nn;
    dirs[3 * (size_t)idx + 2] = wv[2] / nn;
}
__global__ void k_camera_rays(const float* __restrict__ uv, const float* __restrict__ pose, const float* __restrict__ Kin, int B, int P,
                              float* __restrict__ dirs, float* __restrict__ cam_loc) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < B * P) mv_camera_ray(uv, pose, Kin, P, idx, dirs, cam_loc);
}

// ---- rend_util.get_sphere_intersection (rend_util.py:141-162), same op order as the tracer's fused copy ----
__global__ void k_sphere_intersection(const float* __restrict__ cam_loc, const float* __restrict__ dirs, int B, int P, float r,
                                      float* __restrict__ t, uint8_t* __restrict__ mask) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * P) return;
    const float* c = cam_loc + 3 * (idx / P);
    const float* d = dirs + 3 * (size_t)idx;
    const float dot = fmaf(d[2], c[2], fmaf(d[1], c[1], d[0] * c[0]));
    const float nrm = sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    const float under = dot * dot - (nrm * nrm - r * r);
    const bool hit = under > 0.0f;
    float a = 0.0f, b = 0.0f;
    if (hit) { const float s = sqrtf(under); a = s * -1.0f - dot; b = s * 1.0f - dot; }
    t[2 * (size_t)idx] = a < 0.0f ? 0.0f : a;
    t[2 * (size_t)idx + 1] = b < 0.0f ? 0.0f : b;
    mask[idx] = hit ? 1 : 0;
}

// ---- the tracing MLP alone: y[i] = ImplicitNetwork(x[i])[0] ----
template <int MT, int NTW, int NW, bool XR = false>
__global__ __launch_bounds__(64 * NW) void k_sdf_col0(MvNet net, const float* __restrict__ x, int n, float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int ROWS = 16 * MT;
    const int tid = threadIdx.x, d0 = 3 + 6 * net.multires;
    float* act = smem;
    float* pe = act + ROWS * net.S;
    float* pts = pe + ((ROWS * d0 + 3) & ~3);
    float* out = pts + ROWS * 4;
    const int row0 = blockIdx.x * ROWS;
    for (int i = tid; i < ROWS * 3; i += 64 * NW) {
        const int row = row0 + i / 3;
        pts[i] = row < n ? x[3 * (size_t)row0 + i] : 0.0f;
    }
    __syncthreads();
    mv_sdf_eval_col0<MT, NTW, NW, XR>(net, act, pe, pts, out, tid);
    if (tid < ROWS && row0 + tid < n) y[row0 + tid] = out[tid];
}

// the packs of the bf16 engines and the rounded fp32 pack: blockIdx.y selects the layer
struct PackBfArgs { const float* w[MV_MAXL]; uint16_t* wp[MV_MAXL]; int N[MV_MAXL], K[MV_MAXL]; int tr; };   // tr (k_pack_bf16x3_net): pack W^T (N, K stay W's dims)
// trace_dtype = 3 / 4: one bf16 term
__global__ void k_pack_bf16_net(PackBfArgs a) {
    const int l = blockIdx.y;
    mv_pack_flat<32, 1>(a.wp[l], MvSrcW{a.w[l], a.N[l], a.K[l], 0}, MvValBf16());
}
// trace_dtype = 5 and the x3 chains: w = t0 + t1 + t2 exactly, a k-block's three term fragments behind each other
__global__ void k_pack_bf16x3_net(PackBfArgs a) {
    const int l = blockIdx.y;
    mv_pack_flat<32, 3>(a.wp[l], MvSrcW{a.w[l], a.N[l], a.K[l], a.tr}, MvValX3());
}
// trace_dtype = 2: fp32 packs of the bf16-rounded weights (layout of k_pack_net, non-transposed)
__global__ void k_pack_round_net(PackBfArgs a) {
    const int l = blockIdx.y;
    mv_pack_flat<16, 1>((float*)a.wp[l], MvSrcW{a.w[l], a.N[l], a.K[l], 0}, MvValRound());
}

template <int MT, int NTW, bool CARRY, class NET>
__global__ __launch_bounds__(512) void k_sdf_col0_bf(NET net, const float* __restrict__ x, int n, float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int ROWS = 16 * MT;
    const int tid = threadIdx.x, d0 = 3 + 6 * net.multires;
    float* act = smem;
    float* pe = act + ROWS * net.S;
    float* pts = pe + ((ROWS * d0 + 3) & ~3);
    float* out = pts + ROWS * 4;
    const int row0 = blockIdx.x * ROWS;
    for (int i = tid; i < ROWS * 3; i += 512) {
        const int row = row0 + i / 3;
        pts[i] = row < n ? x[3 * (size_t)row0 + i] : 0.0f;
    }
    __syncthreads();
    mv_sdf_eval_col0<MT, NTW, 8, CARRY>(net, act, pe, pts, out, tid);
    if (tid < ROWS && row0 + tid < n) y[row0 + tid] = out[tid];
}

__global__ void k_det_math(int op, const float* __restrict__ x, int n, float* __restrict__ y0, float* __restrict__ y1) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    float a = 0.f, b = 0.f;
    switch (op) {
        case 0: a = dm_softplus100(v); b = dm_sigmoid100(v); break;
        case 1: a = dm_expneg(v); break;
        case 2: a = dm_log1p01(v); break;
        case 3: dm_sincos(v, &a, &b); break;
        case 4: a = dm_div100(v); b = dm_div_sqrt2(v); break;
        case 6: { const dm_f2 h = dm2_softplus100(dm_f2{v, -v}); a = h.x; b = h.y; break; }   // two-wide softplus: y0 = f(x), y1 = f(-x)
        case 7: a = dm_softplus100_lean(v); b = dm_softplus100_lean(-v); break;                  // the f32x3 engine's activation, scalar form
        case 8: { const dm_f2 h = dm2_softplus100_lean(dm_f2{v, -v}); a = h.x; b = h.y; break; }   // ... and the two-wide form the epilogue runs
        default: a = sqrtf(fabsf(v)); b = 1.0f / v; break;
    }
    y0[i] = a;
    if (y1) y1[i] = b;
}

// one launch of a k_sdf_col0 / k_sdf_col0_bf instance over mt row tiles (the dynamic-LDS cap is raised on every call)
template <class K, class NET>
static int launch_col0(K kernel, int mt, int nw, const NET& net, const float* x, int n, float* y, hipStream_t s, const char* where) {
    const int rows = 16 * mt;
    const size_t lds = mv_col0_lds_bytes(net.S, net.multires, mt);
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return mv_check(e, "mvsdf_sdf_col0: LDS attribute");
    hipLaunchKernelGGL(kernel, dim3((n + rows - 1) / rows), dim3(64 * nw), lds, s, net, x, n, y);
    return mv_check(hipGetLastError(), where);
}
// mvsdf_sdf_col0's route (trace_route.h::mv_route_col0) mapped to its template instance of k_sdf_col0 (MvNet) or k_sdf_col0_bf (MvNetBs<NS, WT>; xr: bf_carry)
template <class NET>
static int dispatch_col0(const NET& net, int engine, const float* x, int n, float* y, int mt, hipStream_t s) {
    const MvInst r = mv_route_col0(engine, mv_hidden_nt(net), mt, mv_trace_switches());
    if (r.rc) return mv_fail(r.rc, r.why);
#define MV_COL0(MT_, NTW_, NW_, XR_) case mv_inst_key(MT_, NTW_, NW_) + XR_: return launch_col0(k_sdf_col0<MT_, NTW_, NW_, XR_>, MT_, NW_, net, x, n, y, s, "mvsdf_sdf_col0")
#define MV_COL0_BF(MT_, NTW_) case mv_inst_key(MT_, NTW_, 8): return r.xr ? launch_col0(k_sdf_col0_bf<MT_, NTW_, true, NET>, MT_, 8, net, x, n, y, s, "mvsdf_sdf_col0 (bf16)") \
                                                                       : launch_col0(k_sdf_col0_bf<MT_, NTW_, false, NET>, MT_, 8, net, x, n, y, s, "mvsdf_sdf_col0 (bf16)")
    if constexpr (std::is_same<NET, MvNet>::value) {
        switch (mv_inst_key(r.mt, r.ntw, r.nw) + r.xr) {
            MV_COL0(1, 2, 8, true); MV_COL0(1, 2, 8, false); MV_COL0(2, 2, 8, false); MV_COL0(4, 2, 8, false); MV_COL0(1, 4, 8, false); MV_COL0(2, 4, 8, false);
            MV_COL0(1, 4, 4, false); MV_COL0(2, 4, 4, false); MV_COL0(4, 4, 4, false);
        }
    } else {
        switch (mv_inst_key(r.mt, r.ntw, r.nw)) { MV_COL0_BF(1, 2); MV_COL0_BF(2, 2); MV_COL0_BF(4, 2); MV_COL0_BF(1, 4); MV_COL0_BF(2, 4); }
    }
    return mv_fail(-1, "mvsdf_sdf_col0: no such kernel instance");
}

// =============================================================================================================
extern "C" {

int mvsdf_version(void) { return 100; }

size_t mvsdf_packed_floats(int N, int K) { return mv_packed_floats(N, K); }

static int fill_fold_args(FoldNetArgs& a, int n_layers, const int* N, const int* K, int* maxN, size_t* maxTot) {
    if (n_layers < 1 || n_layers > MV_FOLD_MAXL || !N || !K) return mv_fail(-1, "fold (net): bad layer count / dims");
    memset(&a, 0, sizeof(a));
    a.n_layers = n_layers;
    *maxN = 0; *maxTot = 0;
    for (int l = 0; l < n_layers; ++l) {
        if (N[l] <= 0 || K[l] <= 0) return mv_fail(-1, "fold (net): bad dims");
        a.N[l] = N[l]; a.K[l] = K[l];
        if (N[l] > *maxN) *maxN = N[l];
        const size_t t = mv_packed_floats(N[l], K[l]) > mv_packed_floats(K[l], N[l]) ? mv_packed_floats(N[l], K[l]) : mv_packed_floats(K[l], N[l]);
        if (t > *maxTot) *maxTot = t;
    }
    return 0;
}

// fold (one launch) + pack of W and W^T (one launch) of the layers of `a`
static int launch_fold_pack(const FoldNetArgs& a, int maxN, size_t maxTot, void* stream, const char* where) {
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_fold_net, dim3((maxN + 3) / 4, a.n_layers), dim3(256), 0, s, a);
    const int blocks = (int)((maxTot + 255) / 256 < 256 ? (maxTot + 255) / 256 : 256);
    hipLaunchKernelGGL(k_pack_net, dim3(blocks, 2 * a.n_layers), dim3(256), 0, s, a);
    return mv_check(hipGetLastError(), where);
}

/* one layer: mvsdf_fold_pack_net's kernels on a one-layer list (g is required here; wp / wpT may be NULL) */
int mvsdf_fold_pack(const float* v, const float* g, int N, int K, float* w, float* wp, float* wpT, void* stream) {
    if (!v || !g || N <= 0 || K <= 0 || !w) return mv_fail(-1, "mvsdf_fold_pack: bad arguments (w must be given)");
    FoldNetArgs a;
    int maxN; size_t maxTot;
    int rc = fill_fold_args(a, 1, &N, &K, &maxN, &maxTot);
    if (rc) return rc;
    a.v[0] = v; a.g[0] = g; a.w[0] = w; a.wp[0] = wp; a.wpT[0] = wpT;
    return launch_fold_pack(a, maxN, maxTot, stream, "mvsdf_fold_pack");
}

/* every layer of a network in one call: fold (one launch) + pack W and W^T (one launch).  Pointer arrays are HOST arrays of
 * device pointers; wp / wpT entries may be NULL. */
int mvsdf_fold_pack_net(int n_layers, const float* const* v, const float* const* g, const int* N, const int* K, float* const* w,
                        float* const* wp, float* const* wpT, void* stream) {
    FoldNetArgs a;
    int maxN; size_t maxTot;
    int rc = fill_fold_args(a, n_layers, N, K, &maxN, &maxTot);
    if (rc) return rc;
    if (!v || !g || !w || !wp || !wpT) return mv_fail(-1, "mvsdf_fold_pack_net: null argument");
    for (int l = 0; l < n_layers; ++l) {
        if (!v[l] || !w[l]) return mv_fail(-1, "mvsdf_fold_pack_net: null layer pointer");    // g[l] NULL: layer without weight norm (w = v)
        a.v[l] = v[l]; a.g[l] = g[l]; a.w[l] = w[l]; a.wp[l] = wp[l]; a.wpT[l] = wpT[l];
    }
    return launch_fold_pack(a, maxN, maxTot, stream, "mvsdf_fold_pack_net");
}

int mvsdf_fold_backward_net(int n_layers, const float* const* v, const float* const* g, const float* const* dW, const float* const* db,
                            const int* N, const int* K, float* const* dv, float* const* dg, float* const* dbias, int accumulate,
                            void* stream) {
    FoldNetArgs a;
    int maxN; size_t maxTot;
    int rc = fill_fold_args(a, n_layers, N, K, &maxN, &maxTot);
    if (rc) return rc;
    if (!v || !g || !dW || !dv || !dg || ((db == nullptr) != (dbias == nullptr))) return mv_fail(-1, "mvsdf_fold_backward_net: null argument");
    a.accumulate = accumulate;
    for (int l = 0; l < n_layers; ++l) {
        if (!v[l] || !dW[l] || !dv[l] || (g[l] && !dg[l])) return mv_fail(-1, "mvsdf_fold_backward_net: null layer pointer");
        a.v[l] = v[l]; a.g[l] = g[l]; a.dW[l] = dW[l]; a.dv[l] = dv[l]; a.dg[l] = dg[l];
        if (db) {
            if ((db[l] == nullptr) != (dbias[l] == nullptr)) return mv_fail(-1, "mvsdf_fold_backward_net: db / dbias must pair up");
            a.db[l] = db[l]; a.dbias[l] = dbias[l];
        }
    }
    hipLaunchKernelGGL(k_fold_bwd_net, dim3((maxN + 3) / 4, n_layers), dim3(256), 0, (hipStream_t)stream, a);
    return mv_check(hipGetLastError(), "mvsdf_fold_backward_net");
}

int mvsdf_fold_backward(const float* v, const float* g, const float* dW, int N, int K, float* dv, float* dg, void* stream) {
    if (!v || !g || !dW || !dv || !dg || N <= 0 || K <= 0) return mv_fail(-1, "mvsdf_fold_backward: bad arguments");
    hipLaunchKernelGGL(k_fold_bwd, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, v, g, dW, N, K, dv, dg);
    return mv_check(hipGetLastError(), "mvsdf_fold_backward");
}

int mvsdf_camera_rays(const float* uv, const float* pose, const float* intrinsics, int B, int P, float* ray_dirs, float* cam_loc,
                      void* stream) {
    if (!uv || !pose || !intrinsics || !ray_dirs || !cam_loc || B <= 0 || P <= 0) return mv_fail(-1, "mvsdf_camera_rays: bad arguments");
    hipLaunchKernelGGL(k_camera_rays, dim3((B * P + 255) / 256), dim3(256), 0, (hipStream_t)stream, uv, pose, intrinsics, B, P, ray_dirs,
                       cam_loc);
    return mv_check(hipGetLastError(), "mvsdf_camera_rays");
}

int mvsdf_sphere_intersection(const float* cam_loc, const float* ray_dirs, int B, int P, float r, float* t, uint8_t* mask, void* stream) {
    if (!cam_loc || !ray_dirs || !t || !mask || B <= 0 || P <= 0) return mv_fail(-1, "mvsdf_sphere_intersection: bad arguments");
    hipLaunchKernelGGL(k_sphere_intersection, dim3((B * P + 255) / 256), dim3(256), 0, (hipStream_t)stream, cam_loc, ray_dirs, B, P, r, t, mask);
    return mv_check(hipGetLastError(), "mvsdf_sphere_intersection");
}

size_t mvsdf_packed_bf16_bytes(int N, int K) { return mv_packed_bf16_elems(N, K) * 2; }

/* trace_dtype = 3 / 4: the bf16 packs without duplicated columns (every activation, the positional encoding included, is split into bf16
 * terms in LDS: tile_engine_bf16s.h) */
int mvsdf_pack_bf16s_net(int n_layers, const float* const* w, const int* N, const int* K, void* const* wp16, void* stream) {
    if (n_layers < 1 || n_layers > MV_MAXL || !w || !N || !K || !wp16) return mv_fail(-1, "mvsdf_pack_bf16s_net: bad arguments");
    PackBfArgs a;
    memset(&a, 0, sizeof(a));
    size_t maxTot = 0;
    for (int l = 0; l < n_layers; ++l) {
        if (!w[l] || !wp16[l] || N[l] <= 0 || K[l] <= 0) return mv_fail(-1, "mvsdf_pack_bf16s_net: null layer pointer / bad dims");
        a.w[l] = w[l]; a.wp[l] = (uint16_t*)wp16[l]; a.N[l] = N[l]; a.K[l] = K[l];
        const size_t t = mv_packed_bf16_elems(N[l], K[l]);
        if (t > maxTot) maxTot = t;
    }
    const int blocks = (int)((maxTot + 255) / 256 < 256 ? (maxTot + 255) / 256 : 256);
    hipLaunchKernelGGL(k_pack_bf16_net, dim3(blocks, n_layers), dim3(256), 0, (hipStream_t)stream, a);
    return mv_check(hipGetLastError(), "mvsdf_pack_bf16s_net");
}

/* trace_dtype = 5: three-term bf16 packs of the fp32 weights (3 x mvsdf_packed_bf16_bytes(N, K) bytes per layer) */
static int pack_x3_net(int n_layers, const float* const* w, const int* N, const int* K, void* const* out, int tr, void* stream) {
    if (n_layers < 1 || n_layers > MV_MAXL || !w || !N || !K || !out) return mv_fail(-1, "mvsdf_pack_bf16x3_net / mvsdf_pack_bf16x3t_net: bad arguments");
    PackBfArgs a;
    memset(&a, 0, sizeof(a));
    a.tr = tr;
    size_t maxTot = 0;
    for (int l = 0; l < n_layers; ++l) {
        if (!w[l] || !out[l] || N[l] <= 0 || K[l] <= 0) return mv_fail(-1, "mvsdf_pack_bf16x3_net / mvsdf_pack_bf16x3t_net: null layer pointer / bad dims");
        a.w[l] = w[l]; a.wp[l] = (uint16_t*)out[l]; a.N[l] = N[l]; a.K[l] = K[l];
        const size_t t = 3 * (tr ? mv_packed_bf16_elems(K[l], N[l]) : mv_packed_bf16_elems(N[l], K[l]));
        if (t > maxTot) maxTot = t;
    }
    const int blocks = (int)((maxTot + 255) / 256 < 512 ? (maxTot + 255) / 256 : 512);
    hipLaunchKernelGGL(k_pack_bf16x3_net, dim3(blocks, n_layers), dim3(256), 0, (hipStream_t)stream, a);
    return mv_check(hipGetLastError(), "mvsdf_pack_bf16x3_net");
}
int mvsdf_pack_bf16x3_net(int n_layers, const float* const* w, const int* N, const int* K, void* const* wp16, void* stream) {
    return pack_x3_net(n_layers, w, N, K, wp16, 0, stream);
}
/* the same pack of W^T (N, K: W's dims; 3 x mvsdf_packed_bf16_bytes(K, N) bytes per layer): MvsdfNetDesc.wx3 of the transposed descriptor */
int mvsdf_pack_bf16x3t_net(int n_layers, const float* const* w, const int* N, const int* K, void* const* wx3t, void* stream) {
    return pack_x3_net(n_layers, w, N, K, wx3t, 1, stream);
}

int mvsdf_pack_bf16w_net(int n_layers, const float* const* w, const int* N, const int* K, float* const* wp_rounded, void* stream) {
    if (n_layers < 1 || n_layers > MV_MAXL || !w || !N || !K || !wp_rounded) return mv_fail(-1, "mvsdf_pack_bf16w_net: bad arguments");
    PackBfArgs a;
    memset(&a, 0, sizeof(a));
    size_t maxTot = 0;
    for (int l = 0; l < n_layers; ++l) {
        if (!w[l] || !wp_rounded[l] || N[l] <= 0 || K[l] <= 0) return mv_fail(-1, "mvsdf_pack_bf16w_net: null layer pointer / bad dims");
        a.w[l] = w[l]; a.wp[l] = (uint16_t*)wp_rounded[l]; a.N[l] = N[l]; a.K[l] = K[l];
        const size_t t = mv_packed_floats(N[l], K[l]);
        if (t > maxTot) maxTot = t;
    }
    const int blocks = (int)((maxTot + 255) / 256 < 256 ? (maxTot + 255) / 256 : 256);
    hipLaunchKernelGGL(k_pack_round_net, dim3(blocks, n_layers), dim3(256), 0, (hipStream_t)stream, a);
    return mv_check(hipGetLastError(), "mvsdf_pack_bf16w_net");
}

int mvsdf_sdf_col0(const MvsdfNetDesc* desc, const float* x, int n, float* y, int mt, void* stream) {
    if (!x || !y || n <= 0) return mv_fail(-1, "mvsdf_sdf_col0: bad arguments");
    const MvEngineClass ec = mv_trace_engine(desc ? desc->trace_dtype : 0, true);
    if (ec.rc) return mv_fail(ec.rc, ec.why);
    return mv_with_trace_net(desc, ec.engine, [&](const auto& net) { return dispatch_col0(net, ec.engine, x, n, y, mt, (hipStream_t)stream); });
}

int mvsdf_det_math(int op, const float* x, int n, float* y0, float* y1, void* stream) {
    if (!x || !y0 || n <= 0) return mv_fail(-1, "mvsdf_det_math: bad arguments");
    hipLaunchKernelGGL(k_det_math, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, op, x, n, y0, y1);
    return mv_check(hipGetLastError(), "mvsdf_det_math");
}

}  // extern "C"

// ================================================================================================ step prologue (step_internal.h)
// Everything a training forward needs before the tracer, in ONE launch: the weight-norm fold of every layer of both networks (idr.py:70-71),
// the MFMA packs of W and W^T, the tracing MLP's pack (MvWp16Mode), the three-term packs of the differentiable chains and the camera rays
// (rend_util.py:48-75,87-100) -- the work of k_fold_net, k_pack_net, k_pack_round_net / k_pack_bf16_net / k_pack_bf16x3_net and k_camera_rays, over the
// same definitions: pack_layout.h's maps and values, mv_norm_chain's fold chain (in a second, register-resident schedule for K <= 576) and mv_camera_ray.
// What is this kernel's own is where the blocks go (rg, kbt) -- tests/test_gpu_weight_packs.py holds it to the stand-alone entries end to end.
// A workgroup owns 16 rows of one layer: its sixteen waves fold one row each, the 16 folded rows stay in LDS and the workgroup writes its tile row of the
// W pack, its k-block column of the W^T pack and its tile row of the bf16 packs from there.  The last workgroups compute the rays.
// 16 waves per workgroup, one row each: a row's norm is a serial fmaf chain of ~K steps (~10 us), so the rows must all run side by side.
struct ProloArgs {
    FoldNetArgs f;
    int blk0[MV_FOLD_MAXL + 1];          // first workgroup of each layer; blk0[n_layers] = first ray workgroup
    uint16_t* wp16[MV_FOLD_MAXL];        // optional: the tracing MLP's pack of W_l, in the form wp16_mode names
    uint16_t* wx3[MV_FOLD_MAXL]; uint16_t* wx3T[MV_FOLD_MAXL];   // optional three-term bf16 packs of W_l / W_l^T (the differentiable chains of chain_x3.h)
    int wp16_mode;                       // MvWp16Mode
    const float* uv; const float* pose; const float* Kin; int B, P; float* dirs; float* cam_loc;
    uint8_t* ones;                       // optional [B * P]: filled with 1 (the all-ones object mask of the output dict, idr.py:187)
    unsigned long long* counters;        // optional [16]: zeroed (the tracer's device counters: saves its memset node)
    const float* stage_src; float* stage_a; float* stage_b; int stage_na, stage_nb;   // optional: pinned host memory [na | nb] -> two device buffers
    float* stage_a2;                     // optional: a second copy of the first buffer (the forward block's own min-sdf steps)
    int ld;                              // LDS row stride (floats) >= max K
};
__global__ __launch_bounds__(1024) void k_step_prologue(ProloArgs a) {
    extern __shared__ __attribute__((aligned(16))) float tile[];              // [16][ld]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nl = a.f.n_layers;
    if ((int)blockIdx.x >= a.blk0[nl]) {                                       // ---- camera rays
        const int idx = ((int)blockIdx.x - a.blk0[nl]) * 1024 + tid;
        if (a.counters && idx < 16) a.counters[idx] = 0ull;
        if (a.stage_src) {                                                      // the step's CPU-generator draws, read straight from pinned host memory
            const int nthr = ((int)gridDim.x - a.blk0[nl]) * 1024, ntot = a.stage_na + a.stage_nb;
            for (int i = idx; i < ntot; i += nthr) {
                const float x = a.stage_src[i];
                if (i < a.stage_na) { a.stage_a[i] = x; if (a.stage_a2) a.stage_a2[i] = x; } else a.stage_b[i - a.stage_na] = x;
            }
        }
        if (idx >= a.B * a.P) return;
        if (a.ones) a.ones[idx] = 1;
        mv_camera_ray(a.uv, a.pose, a.Kin, a.P, idx, a.dirs, a.cam_loc);
        return;
    }
    int l = 0;
    while (l + 1 < nl && (int)blockIdx.x >= a.blk0[l + 1]) ++l;
    const int rg = (int)blockIdx.x - a.blk0[l];                                // 16-row group of layer l (groups beyond the rows: pack padding only)
    const int N = a.f.N[l], K = a.f.K[l], ld = a.ld;
    // ---- fold: wave wv takes row 16 rg + wv
    {
        const int jl = wv, j = 16 * rg + jl;
        float* tr = tile + jl * ld;
        if (j >= N) { for (int k = lane; k < K; k += 64) tr[k] = 0.0f; }
        else {
            // this forward's own copy of the bias (optional: a.f.db -> a.f.dbias, the backward's fields): the parameters move on with the optimiser, an evaluation
            // at THIS step's network that runs later (the step's deferred rows) reads the copy
            if (lane == 0 && a.f.dbias[l]) a.f.dbias[l][j] = a.f.db[l][j];
            const float* vr = a.f.v[l] + (size_t)j * K;
            float* wr = a.f.w[l] + (size_t)j * K;
            if (!a.f.g[l]) {                                                   // weight_norm=False: w = v
                for (int k = lane; k < K; k += 64) { const float x = vr[k]; wr[k] = x; tr[k] = x; }
            } else if (K <= 64 * 9) {
                // the whole row is requested before the k-ordered chain starts (chunk by chunk inside the chain, every chunk's load round trip sat
                // between two pieces of it: 4 x ~2 us of the launch's 20 at K = 256) and is reused for the scaling pass
                float mine[9];
                const float gj = a.f.g[l][j];
#pragma unroll
                for (int c = 0; c < 9; ++c) { const int k = 64 * c + lane; const float x = vr[k < K ? k : K - 1]; mine[c] = k < K ? x : 0.0f; }
                // mv_norm_chain's k-ascending fmaf chain (orc_fold's, bit for bit) in another schedule.  Full 64-blocks are unrolled with constant lane numbers: the v_readlane of the
                // elements ahead are independent of the chain and get issued early, so a step costs the fma's latency and not the
                // readlane -> SGPR -> VALU round trip of a rolled loop (which made this chain ~10 us of the launch's 18)
                float ss = 0.0f;
#pragma unroll
                for (int c = 0; c < 9; ++c) {
                    if (64 * (c + 1) <= K) {
#pragma unroll
                        for (int i = 0; i < 64; ++i) {
                            const float x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine[c]), i));
                            ss = fmaf(x, x, ss);
                        }
                    } else if (64 * c < K) {
                        const int n = K - 64 * c;
                        for (int i = 0; i < n; ++i) {
                            const float x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine[c]), i));
                            ss = fmaf(x, x, ss);
                        }
                    }
                }
                const float sc = gj / sqrtf(ss);
#pragma unroll
                for (int c = 0; c < 9; ++c) { const int k = 64 * c + lane; if (k < K) { const float x = mine[c] * sc; wr[k] = x; tr[k] = x; } }
            } else {
                const float sc = a.f.g[l][j] / sqrtf(mv_norm_chain(vr, K, lane));
                for (int k = lane; k < K; k += 64) { const float x = vr[k] * sc; wr[k] = x; tr[k] = x; }
            }
        }
    }
    __syncthreads();
    // ---- pack of W: tile row ct = rg, every k-block
    const int NT = mv_ceil16(N) / 16, KB = mv_kpad(K) / 16, KB32 = mv_bf_kb(K);
    if (a.f.wp[l] && rg < NT) mv_pack_tile_row<16, 1>(a.f.wp[l] + (size_t)rg * KB * 256, KB, tile, ld, K, tid, MvValF32());
    // ---- pack of W^T: k-block kb' = rg of every tile row ct' (columns of W); the tile is W^T's block read across: (row, k) of W^T = tile[k][row]
    if (a.f.wpT[l]) {
        const int NTt = mv_ceil16(K) / 16, KBt = mv_kpad(N) / 16;
        for (int idx = tid; idx < NTt * 256; idx += 1024) {
            const int e = idx & 255, ct = idx >> 8;
            const MvFrag f = mv_frag_f32(e);
            const int o = ct * 16 + f.row;
            a.f.wpT[l][mv_block_index(ct, rg, KBt) * 256 + e] = (o < K) ? tile[f.k * ld + o] : 0.0f;
        }
    }
    // ---- the tracing MLP's pack, tile row ct = rg: the W pack again with values rounded to bf16, one bf16 term, or three
    if (a.wp16[l] && rg < NT) {
        if (a.wp16_mode == MV_WP16_ROUNDED_F32) mv_pack_tile_row<16, 1>((float*)a.wp16[l] + (size_t)rg * KB * 256, KB, tile, ld, K, tid, MvValRound());
        else if (a.wp16_mode == MV_WP16_X3) mv_pack_tile_row<32, 3>(a.wp16[l] + (size_t)rg * KB32 * 3 * 512, KB32, tile, ld, K, tid, MvValX3());
        else mv_pack_tile_row<32, 1>(a.wp16[l] + (size_t)rg * KB32 * 512, KB32, tile, ld, K, tid, MvValBf16());
    }
    // ---- the three-term packs of the differentiable chains
    if (a.wx3[l] && rg < NT) mv_pack_tile_row<32, 3>(a.wx3[l] + (size_t)rg * KB32 * 3 * 512, KB32, tile, ld, K, tid, MvValX3());
    if (a.wx3T[l]) {                                                            // ... of W^T: this workgroup's 16 rows of W are half a k-block of every column tile
        const int NTt = mv_ceil16(K) / 16, KBt = mv_bf_kb(N);
        const int kbt = rg >> 1, k0 = 16 * (rg & 1);                            // k-block of W^T, and where in it the tile's first row stands
        for (int g = tid; g < NTt * 3 * 32; g += 1024) {                        // one 16-byte group (8 consecutive k of one lane) per iteration
            const int jh = g & 1, rl = (g >> 1) & 15, term = (g >> 5) % 3, ct = (g >> 5) / 3;
            const int o = ct * 16 + rl;                                         // column of W = row of W^T
            uint16_t v8[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v8[i] = mv_x3_term(o < K ? tile[(8 * jh + i) * ld + o] : 0.0f, term);      // (rows >= N are zero in the tile)
            uint4 pk;
            pk.x = v8[0] | ((uint32_t)v8[1] << 16); pk.y = v8[2] | ((uint32_t)v8[3] << 16); pk.z = v8[4] | ((uint32_t)v8[5] << 16); pk.w = v8[6] | ((uint32_t)v8[7] << 16);
            if (kbt < KBt) *(uint4*)(a.wx3T[l] + mv_block_index(ct, kbt, KBt, term, 3) * 512 + mv_frag_bf16_at(rl, k0 + 8 * jh)) = pk;
        }
    }
}

int mv_step_prologue(int n_layers, const float* const* v, const float* const* g, const int* N, const int* K, float* const* w, float* const* wp,
                     float* const* wpT, void* const* wp16, MvWp16Mode wp16_mode, void* const* wx3, void* const* wx3T, const float* uv, const float* pose,
                     const float* intrinsics, int B, int P,
                     float* ray_dirs, float* cam_loc, uint8_t* ones, unsigned long long* counters, const float* stage_src, float* stage_a, int stage_na,
                     float* stage_b, int stage_nb, float* stage_a2, const float* const* bias, float* const* bias_copy, void* stream) {
    ProloArgs a;
    int maxN; size_t maxTot;
    int rc = fill_fold_args(a.f, n_layers, N, K, &maxN, &maxTot);
    if (rc) return rc;
    if (!v || !g || !w || !wp || !wpT || !uv || !pose || !intrinsics || !ray_dirs || !cam_loc || B <= 0 || P <= 0) return mv_fail(-1, "mv_step_prologue: null argument");
    int blk = 0, maxK = 0;
    for (int l = 0; l < n_layers; ++l) {
        if (!v[l] || !w[l] || !wp[l] || !wpT[l]) return mv_fail(-1, "mv_step_prologue: null layer pointer");
        a.f.v[l] = v[l]; a.f.g[l] = g[l]; a.f.w[l] = w[l]; a.f.wp[l] = wp[l]; a.f.wpT[l] = wpT[l];
        a.wp16[l] = wp16 ? (uint16_t*)wp16[l] : nullptr;
        a.wx3[l] = wx3 ? (uint16_t*)wx3[l] : nullptr; a.wx3T[l] = wx3T ? (uint16_t*)wx3T[l] : nullptr;
        if (bias && bias_copy && bias[l] && bias_copy[l]) { a.f.db[l] = bias[l]; a.f.dbias[l] = bias_copy[l]; }
        a.blk0[l] = blk; blk += mv_kpad(N[l]) / 16;                              // row groups incl. the W^T pack's zero padding (N padded to 32)
        if (K[l] > maxK) maxK = K[l];
    }
    for (int l = n_layers; l < MV_FOLD_MAXL; ++l) { a.wp16[l] = nullptr; a.wx3[l] = a.wx3T[l] = nullptr; a.blk0[l] = blk; }
    a.blk0[n_layers] = blk;
    a.uv = uv; a.pose = pose; a.Kin = intrinsics; a.B = B; a.P = P; a.dirs = ray_dirs; a.cam_loc = cam_loc;
    a.wp16_mode = wp16_mode;
    a.ones = ones; a.counters = counters;
    a.stage_a2 = stage_src ? stage_a2 : nullptr;
    a.stage_src = stage_src; a.stage_a = stage_a; a.stage_b = stage_b; a.stage_na = stage_src ? stage_na : 0; a.stage_nb = stage_src ? stage_nb : 0;
    if (stage_src && (!stage_a || !stage_b || stage_na < 0 || stage_nb < 0)) return mv_fail(-1, "mv_step_prologue: staged inputs without targets");
    a.ld = ((maxK + 3) & ~3) + 4;
    const size_t lds = (size_t)16 * a.ld * sizeof(float);
    blk += (B * P + 1023) / 1024;
    hipLaunchKernelGGL(k_step_prologue, dim3(blk), dim3(1024), lds, (hipStream_t)stream, a);
    return mv_check(hipGetLastError(), "mv_step_prologue");
}
