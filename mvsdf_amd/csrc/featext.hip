// featext.hip -- inference of the Vis-MVSNet feature CNN `FeatExt` (reference code/utils/my_utils.py:499-708) on the fp32 matrix cores.
// Python: mvsdf_amd/features.py (FeatExt, extract_features), which states the network; tests/featext_ref.py restates it in float64.
//
// Every layer is an implicit GEMM over NHWC fp32 activations: M = output pixels, N = output channels, K = taps x input channels, on
// v_mfma_f32_16x16x4_f32 (exact fp32 products, one rounding per product; gfx950 has no xf32).  A wave owns 16*MT pixels x all Cout (NT = Cout / 16
// column tiles, MT * NT = 16 accumulator tiles = 64 registers); four waves per workgroup, no LDS, no synchronisation.  Each lane reads one float4 of
// the A operand (4 consecutive channels of one pixel) and one float4 of every B tile per 16 input channels: the four MFMA steps of a 16-channel block
// take element s of the lanes' float4s, so step s sums channels {4kq + s : kq = 0..3} of the block and the packed weights hold, per (tap, 16-channel
// block, output channel), the 16 channels contiguously.  The first layer (3 input channels, 5x5) takes the generic path: K = 75 padded to 76,
// one float per lane and step.
//
// * Eval BatchNorm is folded at pack time (fp64: s = gamma / sqrt(var + 1e-5), w' = w s, b' = beta - mean s, each rounded once to fp32).
// * Epilogue: + bias, + residual (NHWC, same shape as the output), ReLU, in that order.
// * The decoder concat is never formed: post_concat reads two sources along K (channels [0, c1) from the deconv output, [c1, c1 + c2) from the
//   encoder output), each 16-channel block from one of them.
// * ConvTranspose2d(3, stride 2, pad 1, output_padding 1) is four gathers, one per output parity class (oy % 2, ox % 2): out[2a + py][2b + px]
//   collects the taps ky with 2a + py = 2 iy - 1 + ky, i.e. py = 0: ky = 1 at iy = a; py = 1: ky = 0 at iy = a + 1 and ky = 2 at iy = a (same in x).
//   Every output pixel is written by exactly one lane of one pass: no atomics.
// * Determinism: every output element is one fixed-order fma chain over K computed by one lane; nothing depends on the batch or on the launch.
#include <math.h>
#include <stdint.h>
#include "capi_util.h"

#define FX_THREADS 256
#define FX_WAVES (FX_THREADS / 64)
#define FX_MAXT 25
#define FX_NLAYERS 27
#define FX_STAGES 7

// one GEMM pass: grid (n, ha, wa) -> output (oy, ox) = (a osy + oy0, b osx + ox0), taps read input (a sy + dy[t], b sx + dx[t])
struct FxPass {
    const float* src1;
    const float* src2;
    const float* w;
    const float* bias;
    const float* res;
    float* out;
    int c1, c2, cout, relu, n, ntaps;
    int hin, win, ha, wa, sy, sx, osy, osx, oy0, ox0, hout, wout;
    signed char dy[FX_MAXT], dx[FX_MAXT];
};

template <int NT, int MT, bool GEN>
__global__ __launch_bounds__(FX_THREADS) void k_fx_conv(const FxPass p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const long long hw = (long long)p.ha * p.wa, M = (long long)p.n * hw;
    const long long p0 = ((long long)blockIdx.x * FX_WAVES + wave) * (16 * MT);
    if (p0 >= M) return;
    int an[MT], ay[MT], ax[MT];
    bool inb[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const long long q = p0 + m * 16 + li;
        inb[m] = q < M;
        const long long qq = inb[m] ? q : 0;
        const long long nn = qq / hw, r = qq - nn * hw;
        const int a = (int)(r / p.wa), b = (int)(r - (long long)a * p.wa);
        an[m] = (int)nn;
        ay[m] = a * p.sy;
        ax[m] = b * p.sx;
    }
    f32x4 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int cin = p.c1 + p.c2;
    if (!GEN) {
        const int nb = cin >> 4;
        for (int t = 0; t < p.ntaps; ++t) {
            long long pix[MT];
            bool ok[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int iy = ay[m] + p.dy[t], ix = ax[m] + p.dx[t];
                ok[m] = inb[m] && iy >= 0 && iy < p.hin && ix >= 0 && ix < p.win;
                pix[m] = ok[m] ? ((long long)an[m] * p.hin + iy) * p.win + ix : 0;     // clamped: the load stays in bounds, the value is dropped
            }
            const float* wt = p.w + ((size_t)t * nb * p.cout + li) * 16 + 4 * kq;
            for (int blk = 0; blk < nb; ++blk) {
                const bool first = blk * 16 < p.c1;
                const float* src = first ? p.src1 : p.src2;
                const int cs = first ? p.c1 : p.c2, c0 = (first ? blk * 16 : blk * 16 - p.c1) + 4 * kq;
                f32x4 av[MT], bv[NT];
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const f32x4 v = *(const f32x4*)(src + pix[m] * cs + c0);
                    av[m] = ok[m] ? v : f32x4{0.f, 0.f, 0.f, 0.f};
                }
#pragma unroll
                for (int j = 0; j < NT; ++j) bv[j] = *(const f32x4*)(wt + ((size_t)blk * p.cout + j * 16) * 16);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int j = 0; j < NT; ++j)
#pragma unroll
                        for (int m = 0; m < MT; ++m) acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m][s], bv[j][s], acc[m][j], 0, 0, 0);
            }
        }
    } else {
        const int K = p.ntaps * cin, Kp = (K + 3) & ~3;
        for (int k0 = 0; k0 < Kp; k0 += 4) {
            const int k = k0 + kq;
            float av[MT];
            const int t = k < K ? k / cin : 0, ci = k < K ? k - t * cin : 0;
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int iy = ay[m] + p.dy[t], ix = ax[m] + p.dx[t];
                const bool ok = k < K && inb[m] && iy >= 0 && iy < p.hin && ix >= 0 && ix < p.win;
                const long long pix = ok ? ((long long)an[m] * p.hin + iy) * p.win + ix : 0;
                const float v = p.src1[pix * cin + ci];
                av[m] = ok ? v : 0.f;
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const float bw = p.w[(size_t)k * p.cout + j * 16 + li];          // rows [K, Kp) of the pack are zero
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bw, acc[m][j], 0, 0, 0);
            }
        }
    }
    // C/D: column (output channel) = lane & 15, row (pixel) = 4 (lane >> 4) + r
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long q = p0 + m * 16 + 4 * kq + r;
            if (q >= M) continue;
            const long long nn = q / hw, rr = q - nn * hw;
            const int a = (int)(rr / p.wa), b = (int)(rr - (long long)a * p.wa);
            const long long opix = (nn * p.hout + (long long)a * p.osy + p.oy0) * p.wout + (long long)b * p.osx + p.ox0;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int c = j * 16 + li;
                float v = acc[m][j][r];
                if (p.bias) v = v + p.bias[c];
                if (p.res) v = v + p.res[opix * p.cout + c];
                if (p.relu) v = v < 0.f ? 0.f : v;
                p.out[opix * p.cout + c] = v;
            }
        }
}

// ------------------------------------------------------------------ layer table and packing ------------------------------------------------------------------
enum { FX_CONV = 0, FX_DECONV = 1 };

struct FxLayer {
    int kind, cin, cout, k, stride, bn;
};

// the order of mvsdf_amd/features.py::LAYERS: init_conv, enc_blocks 2d2_0 / 2d4_1 / 2d8_2 (block 0: conv1, conv2, downsample; block 1: conv1, conv2),
// dec_blocks 2d16_3 / 2d8_4 (deconv, post_concat, res conv1, conv2), final_conv_1/2/3
static const FxLayer FX_LAYERS[FX_NLAYERS] = {
    {FX_CONV, 3, 16, 5, 2, 1},
    {FX_CONV, 16, 32, 3, 1, 1}, {FX_CONV, 32, 32, 3, 1, 1}, {FX_CONV, 16, 32, 1, 1, 1}, {FX_CONV, 32, 32, 3, 1, 1}, {FX_CONV, 32, 32, 3, 1, 1},
    {FX_CONV, 32, 64, 3, 2, 1}, {FX_CONV, 64, 64, 3, 1, 1}, {FX_CONV, 32, 64, 1, 2, 1}, {FX_CONV, 64, 64, 3, 1, 1}, {FX_CONV, 64, 64, 3, 1, 1},
    {FX_CONV, 64, 128, 3, 2, 1}, {FX_CONV, 128, 128, 3, 1, 1}, {FX_CONV, 64, 128, 1, 2, 1}, {FX_CONV, 128, 128, 3, 1, 1}, {FX_CONV, 128, 128, 3, 1, 1},
    {FX_DECONV, 128, 64, 3, 2, 0}, {FX_CONV, 128, 64, 3, 1, 0}, {FX_CONV, 64, 64, 3, 1, 1}, {FX_CONV, 64, 64, 3, 1, 1},
    {FX_DECONV, 64, 32, 3, 2, 0}, {FX_CONV, 64, 32, 3, 1, 0}, {FX_CONV, 32, 32, 3, 1, 1}, {FX_CONV, 32, 32, 3, 1, 1},
    {FX_CONV, 128, 32, 3, 1, 0}, {FX_CONV, 64, 32, 3, 1, 0}, {FX_CONV, 32, 32, 3, 1, 0},
};

static inline size_t fx_raw_floats(const FxLayer& L) { return (size_t)L.cin * L.cout * L.k * L.k + (L.bn ? 4 * (size_t)L.cout : 0); }
static inline bool fx_generic(int cin) { return cin % 16 != 0; }
// packed floats of one layer: weights (K padded to 4 on the generic path) + bias[cout]
static inline size_t fx_pack_floats(const FxLayer& L) {
    const size_t K = (size_t)L.k * L.k * L.cin;
    return (fx_generic(L.cin) ? ((K + 3) & ~(size_t)3) : K) * L.cout + L.cout;
}
static inline size_t fx_align(size_t floats) { return (floats + 63) & ~(size_t)63; }   // 256-byte offsets

// taps of a conv, or of deconv parity class cls = 2 py + px; ky/kx index the source weight, dy/dx the input offset
static int fx_taps(const FxLayer& L, int cls, int* ky, int* kx, signed char* dy, signed char* dx) {
    int n = 0;
    if (L.kind == FX_CONV) {
        const int pad = L.k / 2;
        for (int y = 0; y < L.k; ++y)
            for (int x = 0; x < L.k; ++x, ++n) { ky[n] = y; kx[n] = x; dy[n] = (signed char)(y - pad); dx[n] = (signed char)(x - pad); }
        return n;
    }
    const int py = cls >> 1, px = cls & 1;
    const int nyt = py ? 2 : 1, nxt = px ? 2 : 1;
    const int kys[2] = {py ? 0 : 1, 2}, dys[2] = {py ? 1 : 0, 0}, kxs[2] = {px ? 0 : 1, 2}, dxs[2] = {px ? 1 : 0, 0};
    for (int i = 0; i < nyt; ++i)
        for (int j = 0; j < nxt; ++j, ++n) { ky[n] = kys[i]; kx[n] = kxs[j]; dy[n] = (signed char)dys[i]; dx[n] = (signed char)dxs[j]; }
    return n;
}

struct FxTapIdx {
    int ky[FX_MAXT], kx[FX_MAXT];
};

// one thread per packed weight element (+ cout bias threads at the end); raw: PyTorch layout [cout][cin][k][k] (deconv: [cin][cout][k][k]),
// then (bn) gamma, beta, mean, var [cout]; bias_in (no bn): added as it is, may be NULL
__global__ __launch_bounds__(FX_THREADS) void k_fx_pack(const float* __restrict__ raw, const float* __restrict__ bias_in, int kind, int cin, int cout,
                                                      int k, int bn, int ntaps, const FxTapIdx taps, int generic, float* __restrict__ wout,
                                                      float* __restrict__ bout, long long nw) {
    const long long e = (long long)blockIdx.x * FX_THREADS + threadIdx.x;
    const float* g = raw + (size_t)cin * cout * k * k;
    if (e >= nw) {
        const long long c = e - nw;
        if (c < cout) {
            double b = bias_in ? (double)bias_in[c] : 0.0;
            if (bn) {
                const double s = (double)g[c] / sqrt((double)g[3 * cout + c] + 1e-5);
                b = (double)g[cout + c] - (double)g[2 * cout + c] * s;
            }
            bout[c] = (float)b;
        }
        return;
    }
    int t, ci, co;
    if (generic) {                                             // [k = t cin + ci][co]
        const long long kk = e / cout;
        co = (int)(e - kk * cout);
        t = (int)(kk / cin);
        ci = (int)(kk - (long long)t * cin);
        if (t >= ntaps) { wout[e] = 0.f; return; }
    } else {                                                   // [t][cin / 16][co][16]
        const int cc = (int)(e & 15);
        const long long r = e >> 4;
        co = (int)(r % cout);
        const long long tb = r / cout;
        const int nb = cin >> 4;
        t = (int)(tb / nb);
        ci = (int)(tb - (long long)t * nb) * 16 + cc;
    }
    const int ky = taps.ky[t], kx = taps.kx[t];
    const double w = kind == FX_CONV ? (double)raw[(((size_t)co * cin + ci) * k + ky) * k + kx] : (double)raw[(((size_t)ci * cout + co) * k + ky) * k + kx];
    double s = 1.0;
    if (bn) s = (double)g[co] / sqrt((double)g[3 * cout + co] + 1e-5);
    wout[e] = (float)(w * s);
}

// packed floats of one layer incl. the four deconv passes
static size_t fx_layer_floats(const FxLayer& L) {
    if (L.kind == FX_CONV) return fx_align(fx_pack_floats(L));
    size_t f = 0;
    int ky[FX_MAXT], kx[FX_MAXT];
    signed char dy[FX_MAXT], dx[FX_MAXT];
    for (int c = 0; c < 4; ++c) f += fx_align((size_t)fx_taps(L, c, ky, kx, dy, dx) * L.cin * L.cout + L.cout);
    return f;
}

static int fx_pack_layer(const FxLayer& L, const float* raw, const float* bias, float* dst, hipStream_t s) {
    int ky[FX_MAXT], kx[FX_MAXT];
    signed char dy[FX_MAXT], dx[FX_MAXT];
    for (int c = 0; c < (L.kind == FX_CONV ? 1 : 4); ++c) {
        const int nt = fx_taps(L, c, ky, kx, dy, dx);
        FxTapIdx ti;
        for (int t = 0; t < nt; ++t) { ti.ky[t] = ky[t]; ti.kx[t] = kx[t]; }
        const bool gen = fx_generic(L.cin);
        const size_t K = (size_t)nt * L.cin, nw = (gen ? ((K + 3) & ~(size_t)3) : K) * L.cout;
        const long long tot = (long long)nw + L.cout;
        hipLaunchKernelGGL(k_fx_pack, dim3((unsigned)((tot + FX_THREADS - 1) / FX_THREADS)), dim3(FX_THREADS), 0, s, raw, bias, L.kind, L.cin, L.cout, L.k,
                           L.bn, nt, ti, (int)gen, dst, dst + nw, (long long)nw);
        dst += fx_align(nw + L.cout);
    }
    return mv_check(hipGetLastError(), "featext pack");
}

// ------------------------------------------------------------------ launching ------------------------------------------------------------------
template <int NT, int MT, bool GEN>
static void fx_launch(const FxPass& p, hipStream_t s) {
    const long long M = (long long)p.n * p.ha * p.wa, per = (long long)FX_WAVES * 16 * MT;
    hipLaunchKernelGGL((k_fx_conv<NT, MT, GEN>), dim3((unsigned)((M + per - 1) / per)), dim3(FX_THREADS), 0, s, p);
}

static int fx_dispatch(const FxPass& p, bool gen, hipStream_t s) {
    if (gen) {
        if (p.cout == 16) fx_launch<1, 8, true>(p, s);
        else if (p.cout == 32) fx_launch<2, 8, true>(p, s);
        else return mv_fail(-1, "featext: generic path supports 16 or 32 output channels");
    } else {
        switch (p.cout) {
            case 16: fx_launch<1, 8, false>(p, s); break;
            case 32: fx_launch<2, 8, false>(p, s); break;
            case 64: fx_launch<4, 4, false>(p, s); break;
            case 128: fx_launch<8, 2, false>(p, s); break;
            default: return mv_fail(-1, "featext: output channels must be 16, 32, 64 or 128");
        }
    }
    return mv_check(hipGetLastError(), "featext conv");
}

// one layer: conv (k x k, stride, pad k / 2) or deconv (3, 2, 1, output_padding 1) over NHWC x1 (c1 channels) [+ x2 (c2 channels) along K];
// packed: its pack (fx_pack_layer); res: NHWC [n][ho][wo][cout] or NULL
static int fx_run_layer(const FxLayer& L, const float* packed, const float* x1, int c1, const float* x2, int c2, int n, int h, int w, const float* res,
                        int relu, float* out, hipStream_t s) {
    int ky[FX_MAXT], kx[FX_MAXT];
    const bool gen = fx_generic(c1 + c2);
    if (gen && c2) return mv_fail(-1, "featext: two sources need input channels in multiples of 16");
    if (!gen && (c1 % 16 || c2 % 16)) return mv_fail(-1, "featext: each source's channels must be a multiple of 16");
    FxPass p;
    p.src1 = x1;
    p.src2 = x2;
    p.res = res;
    p.out = out;
    p.c1 = c1;
    p.c2 = c2;
    p.cout = L.cout;
    p.relu = relu;
    p.n = n;
    p.hin = h;
    p.win = w;
    if (L.kind == FX_CONV) {
        const int pad = L.k / 2;
        p.ha = p.hout = (h + 2 * pad - L.k) / L.stride + 1;
        p.wa = p.wout = (w + 2 * pad - L.k) / L.stride + 1;
        p.sy = p.sx = L.stride;
        p.osy = p.osx = 1;
        p.oy0 = p.ox0 = 0;
        p.ntaps = fx_taps(L, 0, ky, kx, p.dy, p.dx);
        const size_t K = (size_t)p.ntaps * L.cin, nw = (gen ? ((K + 3) & ~(size_t)3) : K) * L.cout;
        p.w = packed;
        p.bias = packed + nw;
        return fx_dispatch(p, gen, s);
    }
    p.ha = h;
    p.wa = w;
    p.hout = 2 * h;
    p.wout = 2 * w;
    p.sy = p.sx = 1;
    p.osy = p.osx = 2;
    for (int c = 0; c < 4; ++c) {
        p.oy0 = c >> 1;
        p.ox0 = c & 1;
        p.ntaps = fx_taps(L, c, ky, kx, p.dy, p.dx);
        const size_t nw = (size_t)p.ntaps * L.cin * L.cout;
        p.w = packed;
        p.bias = packed + nw;
        const int rc = fx_dispatch(p, gen, s);
        if (rc) return rc;
        packed += fx_align(nw + L.cout);
    }
    return 0;
}

struct FxWs {
    size_t x0, e0, e1, e2, o2, o3, t1, t2, t3, total;   // float offsets
};

static bool fx_shape(int64_t n, int64_t h, int64_t w) {
    if (n < 1 || h < 1 || w < 1 || h > 65536 || w > 65536) return false;
    const int64_t R = (h + 1) / 2, S = (w + 1) / 2;
    return R % 4 == 0 && S % 4 == 0 && n * R * S * 32 < (int64_t)1 << 40;
}

static FxWs fx_ws(int64_t n, int64_t h, int64_t w) {
    const size_t R = (size_t)(h + 1) / 2, S = (size_t)(w + 1) / 2, rs = (size_t)n * R * S;
    FxWs L;
    size_t o = 0;
    L.x0 = o; o += fx_align(rs * 16);
    L.e0 = o; o += fx_align(rs * 32);
    L.e1 = o; o += fx_align(rs / 4 * 64);
    L.e2 = o; o += fx_align(rs / 16 * 128);
    L.o2 = o; o += fx_align(rs / 4 * 64);
    L.o3 = o; o += fx_align(rs * 32);
    L.t1 = o; o += fx_align(rs * 32);
    L.t2 = o; o += fx_align(rs * 32);
    L.t3 = o; o += fx_align(rs * 32);
    L.total = o;
    return L;
}

extern "C" {

size_t mvsdf_featext_raw_floats(void) {
    size_t f = 0;
    for (int l = 0; l < FX_NLAYERS; ++l) f += fx_raw_floats(FX_LAYERS[l]);
    return f;
}

size_t mvsdf_featext_pack_bytes(void) {
    size_t f = 0;
    for (int l = 0; l < FX_NLAYERS; ++l) f += fx_layer_floats(FX_LAYERS[l]);
    return f * sizeof(float);
}

int mvsdf_featext_pack(const float* raw, void* packed, size_t packed_bytes, void* stream) {
    if (!raw || !packed) return mv_fail(-1, "mvsdf_featext_pack: bad arguments");
    if (packed_bytes < mvsdf_featext_pack_bytes()) return mv_fail(-1, "mvsdf_featext_pack: buffer too small (mvsdf_featext_pack_bytes)");
    hipStream_t s = (hipStream_t)stream;
    float* dst = (float*)packed;
    for (int l = 0; l < FX_NLAYERS; ++l) {
        const int rc = fx_pack_layer(FX_LAYERS[l], raw, nullptr, dst, s);
        if (rc) return rc;
        raw += fx_raw_floats(FX_LAYERS[l]);
        dst += fx_layer_floats(FX_LAYERS[l]);
    }
    return 0;
}

size_t mvsdf_featext_workspace_bytes(int64_t n, int64_t h, int64_t w) {
    if (!fx_shape(n, h, w)) return 0;
    return fx_ws(n, h, w).total * sizeof(float);
}

int mvsdf_featext_forward(const float* packed, const float* x, int64_t n, int64_t h, int64_t w, void* ws, size_t ws_bytes, float* out1, float* out2,
                          float* out3, int first_stage, int last_stage, void* stream) {
    if (!packed || !x || !ws || !fx_shape(n, h, w) || first_stage < 0 || last_stage > FX_STAGES || first_stage > last_stage)
        return mv_fail(-1, "mvsdf_featext_forward: bad arguments (ceil(h / 2) and ceil(w / 2) must be multiples of 4)");
    const FxWs L = fx_ws(n, h, w);
    if (ws_bytes < L.total * sizeof(float)) return mv_fail(-1, "mvsdf_featext_forward: workspace too small (mvsdf_featext_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    float* W = (float*)ws;
    const float* P[FX_NLAYERS];
    for (int l = 0; l < FX_NLAYERS; ++l) P[l] = l ? P[l - 1] + fx_layer_floats(FX_LAYERS[l - 1]) : packed;
    const int N = (int)n, R = (int)((h + 1) / 2), S = (int)((w + 1) / 2);
    float *x0 = W + L.x0, *e0 = W + L.e0, *e1 = W + L.e1, *e2 = W + L.e2, *o2 = W + L.o2, *o3 = W + L.o3, *t1 = W + L.t1, *t2 = W + L.t2, *t3 = W + L.t3;
    const FxLayer* F = FX_LAYERS;
    int rc = 0;
#define FX_RUN(l, a, ca, b, cb, hh, ww, res, relu, out) \
    do { if ((rc = fx_run_layer(F[l], P[l], a, ca, b, cb, N, hh, ww, res, relu, out, s))) return rc; } while (0)
    // encoder stage: block 0 (conv1, conv2, downsample at l0, l0 + 1, l0 + 2), block 1 (l0 + 3, l0 + 4); input hi x wi, output ho x wo
    auto enc = [&](int l0, const float* in, int cin, int hi, int wi, float* out) -> int {
        const int cout = F[l0].cout, ho = F[l0].stride == 2 ? (hi + 1) / 2 : hi, wo = F[l0].stride == 2 ? (wi + 1) / 2 : wi;
        FX_RUN(l0, in, cin, nullptr, 0, hi, wi, nullptr, 1, t1);
        FX_RUN(l0 + 2, in, cin, nullptr, 0, hi, wi, nullptr, 0, t2);
        FX_RUN(l0 + 1, t1, cout, nullptr, 0, ho, wo, t2, 1, t3);
        FX_RUN(l0 + 3, t3, cout, nullptr, 0, ho, wo, nullptr, 1, t1);
        FX_RUN(l0 + 4, t1, cout, nullptr, 0, ho, wo, t3, 1, out);
        return 0;
    };
    // decoder stage: deconv, post_concat over (deconv output, skip), one residual block; input hi x wi (cin channels), output 2hi x 2wi
    auto dec = [&](int l0, const float* in, int cin, int hi, int wi, const float* skip, float* out) -> int {
        const int cout = F[l0].cout;
        FX_RUN(l0, in, cin, nullptr, 0, hi, wi, nullptr, 0, t1);
        FX_RUN(l0 + 1, t1, cout, skip, cout, 2 * hi, 2 * wi, nullptr, 0, t2);
        FX_RUN(l0 + 2, t2, cout, nullptr, 0, 2 * hi, 2 * wi, nullptr, 1, t3);
        FX_RUN(l0 + 3, t3, cout, nullptr, 0, 2 * hi, 2 * wi, t2, 1, out);
        return 0;
    };
    for (int st = first_stage; st < last_stage; ++st) {
        switch (st) {
            case 0: FX_RUN(0, x, 3, nullptr, 0, (int)h, (int)w, nullptr, 1, x0); break;
            case 1: rc = enc(1, x0, 16, R, S, e0); break;
            case 2: rc = enc(6, e0, 32, R, S, e1); break;
            case 3: rc = enc(11, e1, 64, R / 2, S / 2, e2); break;
            case 4: rc = dec(16, e2, 128, R / 4, S / 4, e1, o2); break;
            case 5: rc = dec(20, o2, 64, R / 2, S / 2, e0, o3); break;
            case 6:
                if (out1) FX_RUN(24, e2, 128, nullptr, 0, R / 4, S / 4, nullptr, 0, out1);
                if (out2) FX_RUN(25, o2, 64, nullptr, 0, R / 2, S / 2, nullptr, 0, out2);
                if (out3) FX_RUN(26, o3, 32, nullptr, 0, R, S, nullptr, 0, out3);
                break;
        }
        if (rc) return rc;
    }
#undef FX_RUN
    return 0;
}

// ---- one layer alone (tests, timing) ----
static bool fx_layer_desc(int kind, int cin, int cout, int k, int stride, FxLayer* L) {
    if (kind != FX_CONV && kind != FX_DECONV) return false;
    if (cin < 1 || cin > 4096 || (cout != 16 && cout != 32 && cout != 64 && cout != 128)) return false;
    if (kind == FX_CONV && !((k == 1 || k == 3 || k == 5) && (stride == 1 || stride == 2))) return false;
    if (kind == FX_DECONV && !(k == 3 && stride == 2 && cin % 16 == 0)) return false;
    if (fx_generic(cin) && (kind != FX_CONV || cout > 32)) return false;
    *L = FxLayer{kind, cin, cout, k, stride, 0};
    return true;
}

size_t mvsdf_featext_layer_workspace_bytes(int kind, int cin, int cout, int k, int stride) {
    FxLayer L;
    if (!fx_layer_desc(kind, cin, cout, k, stride, &L)) return 0;
    return fx_layer_floats(L) * sizeof(float);
}

int mvsdf_featext_layer(int kind, const float* weight, const float* bias, int cout, int k, int stride, const float* x1, int c1, const float* x2, int c2,
                        int64_t n, int64_t h, int64_t w, const float* res, int relu, void* ws, size_t ws_bytes, float* out, void* stream) {
    FxLayer L;
    if (!weight || !x1 || !out || !ws || (c2 && !x2) || c1 < 1 || c2 < 0 || !fx_layer_desc(kind, c1 + c2, cout, k, stride, &L) || n < 1 || h < 1 ||
        w < 1 || h > 65536 || w > 65536 || n * h * w > ((int64_t)1 << 31) || (kind == FX_CONV && (h + 2 * (k / 2) < k || w + 2 * (k / 2) < k)))
        return mv_fail(-1, "mvsdf_featext_layer: bad arguments");
    if (ws_bytes < fx_layer_floats(L) * sizeof(float)) return mv_fail(-1, "mvsdf_featext_layer: workspace too small (mvsdf_featext_layer_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    int rc = fx_pack_layer(L, weight, bias, (float*)ws, s);
    if (rc) return rc;
    return fx_run_layer(L, (const float*)ws, x1, c1, x2, c2, (int)n, (int)h, (int)w, res, relu, out, s);
}

}  // extern "C"
