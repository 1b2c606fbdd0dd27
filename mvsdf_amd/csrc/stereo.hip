// stereo.hip -- on-device plane-sweep stereo: per reference view a depth map and three confidence maps from descriptor maps, cameras and pair lists (the
// step BYOD.md calls "Run VisMVSNet", as a classical sweep).  Python: mvsdf_amd/stereo.py, which states the definition; tests/stereo_ref.py restates it
// in numpy.  All arithmetic is fp64 without contraction, in the order the definition writes it.
//
// * k_ps_normalize: one lane per texel, unit descriptors rounded to fp32 (a texel of 32 channels is one 128-byte line); sets the error bit on a non-finite
//   feature.  k_any_nonfinite (geom_prims.h): the same check alone, on descriptors that come from the caller.  k_ps_patches: the mean-free grey patch descriptor.
// * k_ps_score: a 256-lane workgroup owns a 16 x 16 tile of reference pixels (four waves of 8 x 8) and PS_KCHUNK consecutive hypotheses; a lane keeps its
//   pixel's descriptor in registers as doubles and walks k.  The 8 x 8 pixels of a wave at one k read a patch of about 9 x 9 source texels, and the next k
//   moves that patch along the epipolar lines by about a texel, so the four-tap gathers are served by the CU's L1 and the XCD's L2 after the first touch.
//   The dot products use fma(): the product of two fp32 values is exact in fp64, so fma(a, b, t) is t + a*b rounded once, the definition's value bit for
//   bit (signed zeros included); nothing else is contracted.  The projection of a hypothesis into a source, its 2x2 cell and the blend of the four dot
//   products (ps_sample) are view_prims.h's mv_project_texel and MvCell, the ones fusion.hip and tsdf.hip sample depth maps with.  Writes
//   score[k][y][x] (a quiet NaN where no source is valid) and the count n_k as a byte.
// * k_ps_pick: one lane per pixel walks the volume (coalesced over the lanes): winner, refinement, b2, the three confidences.
// * k_sg_path: one direction of the semi-global regularisation (stereo.py: "Regularisation").  A 256-lane workgroup owns a bundle of G adjacent paths and
//   walks them step by step; lane t owns path t % G and the hypotheses t / G, t / G + 256 / G, ...  The previous step's path costs L live in LDS, k-major
//   ([k + 1][path], rows 0 and D + 1 hold +inf, so k - 1 and k + 1 need no branch and consecutive lanes touch consecutive words), double-buffered: one
//   barrier per step.  An invalid L is +inf there, so every minimum skips it by itself; a path's minimum m is reduced over the wave by shuffles and over
//   the four waves through LDS, and m = +inf is the definition's restart (q outside the image or without a valid k).  The costs and the running sum T of
//   the next step are loaded before the barrier of this one.  Launch r adds L_r into T in place (out), the last one turns T into A; stream order is the
//   summation order, and every element is written by one lane per launch.  For the six directions with dy != 0 a step is an image row and the G paths of
//   a bundle are G consecutive x (8 doubles = 64 bytes per k at D <= 256); the two horizontal directions step along x with bundles of adjacent rows, their
//   reads are strided by S and served by L2 for the 16 steps a 128-byte line lasts, so they take the smallest G that fills the lanes (more workgroups).
//
// One call sweeps every requested view in turn on the caller's stream; the score volume in the workspace is reused from view to view and holds the last
// view's scores afterwards.  Every argument is validated on the host before anything is launched; only the finiteness of the descriptors is checked on the
// device.  No atomics on floating point (the only atomic is the OR of an error bit).
#include "view_prims.h"

#define PS_THREADS 256
#define PS_TILE 16
#define PS_KCHUNK 32
#define PS_HDR 256                                    // bytes at the start of the workspace: MVSDF_RES_H_*
static_assert(MVSDF_RES_H_WORDS * 8 <= PS_HDR, "the result words fit the header");
#define PS_MAX_ELEMS (1ll << MVSDF_PS_MAX_ELEMS_LOG2)

#define SG_MAX_ITEMS 2048                             // G * D at most this where G > 1: the two LDS buffers then take 32 KB
#define SG_MAX_G 8

struct PsLayout {
    size_t mats, src, vol, cnt, total;
};

static bool ps_layout(long long R, long long S, long long D, long long npairs, PsLayout* L) {
    if (R < 2 || S < 2 || D < 1 || D > MVSDF_PS_MAX_D || npairs < 0 || npairs > INT_MAX || R > INT_MAX || S > INT_MAX || R * S > INT_MAX) return false;
    if (R * S * D > PS_MAX_ELEMS) return false;
    WsCursor c{PS_HDR};
    L->mats = c.take((size_t)(npairs > 0 ? npairs : 1) * 16 * 8);
    L->src = c.take((size_t)(npairs > 0 ? npairs : 1) * 4);
    L->vol = c.take((size_t)(R * S * D) * 8);
    L->cnt = c.take((size_t)(R * S * D));
    L->total = c.o;
    return true;
}

__device__ __forceinline__ double ps_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

__global__ __launch_bounds__(PS_THREADS) void k_ps_normalize(const float* __restrict__ f, long long n, int C, float* __restrict__ out, long long* __restrict__ hdr) {
    const long long i = (long long)blockIdx.x * PS_THREADS + threadIdx.x;
    if (i >= n) return;
    const float* __restrict__ p = f + i * C;
    float* __restrict__ o = out + i * C;
    double s = 0.0;
    bool bad = false;
    for (int c = 0; c < C; ++c) {
        const double v = (double)p[c];
        bad = bad || !isfinite(v);
        s = s + v * v;
    }
    const double nrm = sqrt(s);
    for (int c = 0; c < C; ++c) o[c] = nrm > 0.0 ? (float)((double)p[c] / nrm) : 0.0f;
    if (bad) atomicOr((unsigned long long*)(hdr + MVSDF_RES_H_ERR), (unsigned long long)MVSDF_PS_ERR_FINITE);
}

// grey = (299 R + 587 G + 114 B) / 1000; the (2 rad + 1)^2 patch around the pixel, border clamped, rows then columns, minus its mean
__global__ __launch_bounds__(PS_THREADS) void k_ps_patches(const unsigned char* __restrict__ img, long long V, int H, int W, int rad, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * PS_THREADS + threadIdx.x;
    const long long hw = (long long)H * W;
    if (i >= V * hw) return;
    const long long v = i / hw;
    const int p = (int)(i - v * hw), y = p / W, x = p - y * W;
    const unsigned char* __restrict__ im = img + v * hw * 3;
    const int side = 2 * rad + 1;
    double s = 0.0;
    for (int dy = -rad; dy <= rad; ++dy) {
        const int yy = min(max(y + dy, 0), H - 1);
        for (int dx = -rad; dx <= rad; ++dx) {
            const int xx = min(max(x + dx, 0), W - 1);
            const unsigned char* q = im + ((long long)yy * W + xx) * 3;
            s = s + (double)(299 * (int)q[0] + 587 * (int)q[1] + 114 * (int)q[2]) / 1000.0;
        }
    }
    const double mean = s / (double)(side * side);
    float* __restrict__ o = out + i * side * side;
    for (int dy = -rad; dy <= rad; ++dy) {
        const int yy = min(max(y + dy, 0), H - 1);
        for (int dx = -rad; dx <= rad; ++dx) {
            const int xx = min(max(x + dx, 0), W - 1);
            const unsigned char* q = im + ((long long)yy * W + xx) * 3;
            *o++ = (float)((double)(299 * (int)q[0] + 587 * (int)q[1] + 114 * (int)q[2]) / 1000.0 - mean);
        }
    }
}

// the four dot products of the reference descriptor with the texels g, g + C (next column), g + row, g + row + C, in channel order
template <int CFIX>
__device__ __forceinline__ void ps_dots(const double* ref, const float* __restrict__ fr, const float* __restrict__ g, long long row, int C, double& t00,
                                        double& t01, double& t10, double& t11) {
    if (CFIX == 32) {
        const float4* __restrict__ a = (const float4*)g;
        const float4* __restrict__ b = (const float4*)(g + 32);
        const float4* __restrict__ c = (const float4*)(g + row);
        const float4* __restrict__ d = (const float4*)(g + row + 32);
        float4 va = a[0], vb = b[0], vc = c[0], vd = d[0];
        t00 = ref[0] * (double)va.x; t01 = ref[0] * (double)vb.x; t10 = ref[0] * (double)vc.x; t11 = ref[0] * (double)vd.x;
#define PS_STEP(i, m) t00 = fma(ref[i], (double)va.m, t00); t01 = fma(ref[i], (double)vb.m, t01); t10 = fma(ref[i], (double)vc.m, t10); t11 = fma(ref[i], (double)vd.m, t11);
        PS_STEP(1, y) PS_STEP(2, z) PS_STEP(3, w)
#pragma unroll
        for (int q = 1; q < 8; ++q) {
            va = a[q]; vb = b[q]; vc = c[q]; vd = d[q];
            PS_STEP(4 * q, x) PS_STEP(4 * q + 1, y) PS_STEP(4 * q + 2, z) PS_STEP(4 * q + 3, w)
        }
#undef PS_STEP
    } else {
        double r = (double)fr[0];
        t00 = r * (double)g[0]; t01 = r * (double)g[C]; t10 = r * (double)g[row]; t11 = r * (double)g[row + C];
        for (int q = 1; q < C; ++q) {
            r = (double)fr[q];
            t00 = fma(r, (double)g[q], t00);
            t01 = fma(r, (double)g[C + q], t01);
            t10 = fma(r, (double)g[row + q], t10);
            t11 = fma(r, (double)g[row + C + q], t11);
        }
    }
}

// one hypothesis of one reference pixel (X, Y = its centre, d = the depth, ref / fr = its descriptor): the sum of c_s over the valid sources in pair
// order, n = their number.  k_ps_score and k_ps_band share it, so both give the same bits.
template <int CFIX>
__device__ __forceinline__ double ps_sample(const float* __restrict__ desc, long long hw, long long row, int R, int S, int C, const double* ref,
                                            const float* __restrict__ fr, double X, double Y, double d, int nsrc, const int* __restrict__ src,
                                            const double* __restrict__ mats, int& n) {
    const double q0 = X * d, q1 = Y * d;
    double acc = 0.0;
    for (int j = 0; j < nsrc; ++j) {
        MvProj pr = {};                                                   // set: nothing is carried around the loop (view_prims.h: mv_project)
        if (!mv_project_texel(mats + (long long)j * 16, q0, q1, d, S, R, &pr)) continue;
        const MvCell at = mv_cell(pr.u, pr.v, S, R);
        const float* __restrict__ g = desc + ((long long)src[j] * hw + (long long)at.y0 * S + at.x0) * C;
        double t00, t01, t10, t11;
        ps_dots<CFIX>(ref, fr, g, row, C, t00, t01, t10, t11);
        acc = acc + at.blend(t00, t01, t10, t11);
        ++n;
    }
    return acc;
}

// scores of view r.  Grid: (tiles in x, tiles in y, chunks of PS_KCHUNK hypotheses); src / mats: the nsrc pair slots of this view (T_rs, row-major 4x4)
template <int CFIX>
__global__ __launch_bounds__(PS_THREADS) void k_ps_score(const float* __restrict__ desc, int R, int S, int C, int r, int nsrc, const int* __restrict__ src,
                                                          const double* __restrict__ mats, double dmin, double interval, int D, double* __restrict__ vol,
                                                          unsigned char* __restrict__ cnt) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int x = blockIdx.x * PS_TILE + ((w & 1) << 3) + (l & 7), y = blockIdx.y * PS_TILE + ((w >> 1) << 3) + (l >> 3);
    if (x >= S || y >= R) return;
    const int k0 = blockIdx.z * PS_KCHUNK, k1 = min(D, k0 + PS_KCHUNK);
    const long long hw = (long long)R * S, row = (long long)S * C;
    const long long pix = (long long)y * S + x;
    const float* __restrict__ fr = desc + ((long long)r * hw + pix) * C;
    double ref[CFIX ? CFIX : 1];
    if (CFIX) {
#pragma unroll
        for (int c = 0; c < CFIX; ++c) ref[c] = (double)fr[c];
    }
    const double X = (double)x + 0.5, Y = (double)y + 0.5;
    for (int k = k0; k < k1; ++k) {
        int n = 0;
        const double acc = ps_sample<CFIX>(desc, hw, row, R, S, C, ref, fr, X, Y, dmin + (double)k * interval, nsrc, src, mats, n);
        const long long at = (long long)k * hw + pix;
        vol[at] = n ? acc / (double)n : ps_nan();
        cnt[at] = (unsigned char)n;
    }
}

// the definition's winner, refinement and confidences of one pixel from its scores vol[k * stride] (NaN = invalid), k < D; used = the number of sources
// the view sweeps.  REG: vol holds regularised scores and prob1 is the raw score (raw) at their winner.  k_ps_pick walks the volume in global memory,
// k_ps_band its tile's band in LDS.
struct PsPick {
    int ks, nk;             // k* (-1: no valid hypothesis) and n_k*
    double off;             // the refinement
    float p1, p2, p3;
};

template <bool REG>
__device__ __forceinline__ PsPick ps_pick(const double* vol, const double* raw, const unsigned char* cnt, long long stride, int D, int used) {
    PsPick o = {-1, 0, 0.0, 0.0f, 0.0f, 0.0f};
    double b = -INFINITY;
    for (int k = 0; k < D; ++k) {
        const double s = vol[(long long)k * stride];
        if (s > b) { b = s; o.ks = k; }                                         // NaN (invalid) never compares greater
    }
    const int ks = o.ks;
    if (ks < 0) return o;
    bool any = false;
    double b2 = -INFINITY;
    for (int k = 0; k < D; ++k) {
        if (k >= ks - 1 && k <= ks + 1) continue;
        const double s = vol[(long long)k * stride];
        if (s == s) {
            any = true;
            if (s > b2) b2 = s;
        }
    }
    if (ks > 0 && ks < D - 1) {
        const double a = vol[(long long)(ks - 1) * stride], c = vol[(long long)(ks + 1) * stride];
        if (a == a && c == c) {
            const double den = (a - 2.0 * b) + c;
            if (den < 0.0) o.off = 0.5 * (a - c) / den;
        }
    }
    o.p1 = (float)fmin(fmax(REG ? raw[(long long)ks * stride] : b, 0.0), 1.0);
    if (b <= 0.0) o.p2 = 0.0f;
    else if (!any) o.p2 = 1.0f;
    else o.p2 = (float)fmin(fmax(1.0 - fmax(b2, 0.0) / b, 0.0), 1.0);
    o.nk = cnt[(long long)ks * stride];
    o.p3 = (float)((double)o.nk / (double)used);
    return o;
}

// winner, refinement and confidences of every pixel of one view, one lane per pixel (coalesced over the lanes)
template <bool REG>
__global__ __launch_bounds__(PS_THREADS) void k_ps_pick(const double* __restrict__ vol, const double* __restrict__ raw, const unsigned char* __restrict__ cnt,
                                                         int hw, int D, double dmin, double interval, int used, float* __restrict__ depth,
                                                         float* __restrict__ prob, int* __restrict__ best_k, int* __restrict__ counts) {
    const int p = blockIdx.x * PS_THREADS + threadIdx.x;
    if (p >= hw) return;
    const PsPick o = ps_pick<REG>(vol + p, raw + p, cnt + p, hw, D, used);
    depth[p] = o.ks >= 0 ? (float)(dmin + ((double)o.ks + o.off) * interval) : 0.0f;
    prob[p] = o.p1;
    prob[hw + p] = o.p2;
    prob[2 * (long long)hw + p] = o.p3;
    best_k[p] = o.ks;
    counts[p] = o.nk;
}

// ================================================================ the cascade: centres and the band sweep ================================================================
// stereo.py: "Cascade".  k_ps_upsample: one lane per pixel of the finer size, the centre from the four parents that have a winner.
__global__ __launch_bounds__(PS_THREADS) void k_ps_upsample(const float* __restrict__ depth, const int* __restrict__ best_k, long long V, int r, int s, int R,
                                                             int S, double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * PS_THREADS + threadIdx.x;
    const long long HW = (long long)R * S;
    if (i >= V * HW) return;
    const long long v = i / HW;
    const int p = (int)(i - v * HW), y = p / S, x = p - y * S;
    const double u = fmin(fmax((((double)x + 0.5) * (double)s) / (double)S - 0.5, 0.0), (double)(s - 1));
    const double w = fmin(fmax((((double)y + 0.5) * (double)r) / (double)R - 0.5, 0.0), (double)(r - 1));
    const MvCell c = mv_cell(u, w, s, r);                                 // the cell alone: the weights below are renormalised over the parents with a winner
    const double fx = c.fx, fy = c.fy;
    const long long at = v * ((long long)r * s) + (long long)c.y0 * s + c.x0;
    const double wt[4] = {(1.0 - fx) * (1.0 - fy), fx * (1.0 - fy), (1.0 - fx) * fy, fx * fy};
    double num = 0.0, den = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long long t = at + (q >> 1) * s + (q & 1);
        if (best_k[t] >= 0) {
            num = num + wt[q] * (double)depth[t];
            den = den + wt[q];
        }
    }
    out[i] = den > 0.0 ? num / den : ps_nan();
}

// k_ps_band: a 256-lane workgroup owns an 8 x 8 tile of reference pixels of one view (blockIdx.z: the slot in the view list) and the whole band of Db
// hypotheses around every pixel's centre.  Lane l of every wave owns pixel l of the tile; wave w scores the hypotheses w, w + 4, ... with ps_sample
// (the four waves walk neighbouring depths at the same time, so their gathers meet in L1) into the tile's LDS image: score[k][pixel] fp64 and
// n_k[k][pixel] as bytes, 9 * 64 * Db bytes, 36 KB at MVSDF_PS_MAX_D_BAND, conflict-free (consecutive lanes, consecutive words).  After the one barrier wave 0
// picks from LDS (ps_pick) and writes the pixel's outputs: no score leaves the CU, every output element has one writer, no atomics but the error bit.
#define PB_TILE 8

template <int CFIX>
__global__ __launch_bounds__(PS_THREADS) void k_ps_band(const float* __restrict__ desc, int R, int S, int C, const int* __restrict__ views,
                                                         const int* __restrict__ pair_off, const double* __restrict__ steps,
                                                         const int* __restrict__ src, const double* __restrict__ mats, const double* __restrict__ centres,
                                                         int Db, float* __restrict__ depths, float* __restrict__ probs, int* __restrict__ best_k,
                                                         int* __restrict__ counts, unsigned long long* __restrict__ errword) {
    extern __shared__ double pb_score[];                                  // [Db][64], then the counts [Db][64] as bytes
    unsigned char* pb_cnt = (unsigned char*)(pb_score + Db * 64);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int r = views[blockIdx.z], off = pair_off[blockIdx.z], nsrc = pair_off[blockIdx.z + 1] - off;
    const double step = steps[blockIdx.z];
    const int x = blockIdx.x * PB_TILE + (l & 7), y = blockIdx.y * PB_TILE + (l >> 3);
    const bool inside = x < S && y < R;
    const long long hw = (long long)R * S, row = (long long)S * C;
    const long long pix = inside ? (long long)y * S + x : 0;
    const double c = centres[(long long)r * hw + pix];
    const bool has = inside && isfinite(c);                               // NaN: no centre (an infinite one is refused below)
    const int half = Db >> 1;
    if (w < Db) {
        const float* __restrict__ fr = desc + ((long long)r * hw + pix) * C;
        double ref[CFIX ? CFIX : 1];
        if (CFIX) {
#pragma unroll
            for (int q = 0; q < CFIX; ++q) ref[q] = (double)fr[q];
        }
        const double X = (double)x + 0.5, Y = (double)y + 0.5;
        for (int k = w; k < Db; k += PS_THREADS / 64) {
            const double d = c + (double)(k - half) * step;
            int n = 0;
            double acc = 0.0;
            if (has && d > 0.0) acc = ps_sample<CFIX>(desc, hw, row, R, S, C, ref, fr, X, Y, d, nsrc, src + off, mats + (long long)off * 16, n);
            pb_score[k * 64 + l] = n ? acc / (double)n : ps_nan();
            pb_cnt[k * 64 + l] = (unsigned char)n;
        }
    }
    __syncthreads();
    if (w) return;
    if (__ballot(inside && isinf(c)) && l == 0) atomicOr(errword, (unsigned long long)MVSDF_PS_ERR_CENTRE);
    if (!inside) return;
    const PsPick o = ps_pick<false>(pb_score + l, pb_score + l, pb_cnt + l, 64, Db, nsrc);
    const long long at = (long long)r * hw + pix;
    depths[at] = o.ks >= 0 ? (float)(c + ((double)(o.ks - half) + o.off) * step) : 0.0f;
    probs[3 * at - 2 * pix] = o.p1;                                       // [r][0][pix]
    probs[3 * at - 2 * pix + hw] = o.p2;
    probs[3 * at - 2 * pix + 2 * hw] = o.p3;
    best_k[at] = o.ks;
    counts[at] = o.nk;
}

// ================================================================ semi-global regularisation ================================================================
// one direction: step t of path c visits pixel (py0 + cy*c + ty*t, px0 + cx*c + tx*t); c = c0 + 0 .. npaths - 1
struct SgDir {
    int py0, cy, ty, px0, cx, tx, c0, npaths, nsteps;
};
enum { SG_FIRST = 0, SG_ADD = 1, SG_LAST = 2 };       // what a launch does with T: write L, add L, add L and turn the sum into A

__device__ __forceinline__ double sg_min(double a, double b) { return b < a ? b : a; }          // no NaN reaches it

// the steps at which p0 + cc*c + tt*t can be inside [0, n) for some c in [ca, cb]
__device__ __forceinline__ void sg_clip(int p0, int cc, int tt, int ca, int cb, int n, int& lo, int& hi) {
    const int a = p0 + cc * ca, b = p0 + cc * cb;
    if (tt > 0) { lo = max(lo, -b); hi = min(hi, n - 1 - a); }
    else if (tt < 0) { lo = max(lo, a - (n - 1)); hi = min(hi, b); }
}

template <int ITEMS>
__global__ __launch_bounds__(PS_THREADS) void k_sg_path(const double* __restrict__ score, double* __restrict__ out, int R, int S, int D, SgDir dir, int lg,
                                                         double p1, double p2, int mode, double inv_paths, unsigned long long* __restrict__ errword) {
    extern __shared__ double sg_lds[];
    const int G = 1 << lg, kstride = PS_THREADS >> lg;
    const int t = threadIdx.x, g = t & (G - 1), kq = t >> lg, wave = t >> 6;
    const int rows = (D + 2) * G;                                         // doubles per buffer
    double* __restrict__ red = sg_lds + 2 * rows;                         // [2][4 waves][G]: the waves' minima of every path
    const double inf = INFINITY;
    for (int i = t; i < 2 * rows; i += PS_THREADS) sg_lds[i] = inf;
    if (t < 2 * 4 * SG_MAX_G) red[t] = inf;
    const int pi = blockIdx.x * G + g;
    const bool active = pi < dir.npaths;
    const int c = dir.c0 + pi;
    int lo = 0, hi = dir.nsteps - 1;
    {
        const int ca = dir.c0 + blockIdx.x * G, cb = min(ca + G - 1, dir.c0 + dir.npaths - 1);
        sg_clip(dir.py0, dir.cy, dir.ty, ca, cb, R, lo, hi);
        sg_clip(dir.px0, dir.cx, dir.tx, ca, cb, S, lo, hi);
    }
    const long long hw = (long long)R * S;
    const int py = dir.py0 + dir.cy * c, px = dir.px0 + dir.cx * c;
    double cn[ITEMS], tn[ITEMS];                                          // the next step's scores and running sums
    bool in_n = false;
    long long pix_n = 0;
#define SG_FETCH(step)                                                                                      \
    {                                                                                                       \
        const int y_ = py + dir.ty * (step), x_ = px + dir.tx * (step);                                     \
        in_n = active && (step) <= hi && y_ >= 0 && y_ < R && x_ >= 0 && x_ < S;                            \
        pix_n = (long long)y_ * S + x_;                                                                     \
        _Pragma("unroll") for (int j = 0; j < ITEMS; ++j) {                                                 \
            const int k_ = kq + j * kstride;                                                                \
            const bool ok_ = in_n && k_ < D;                                                                \
            cn[j] = ok_ ? score[(long long)k_ * hw + pix_n] : ps_nan();                                     \
            tn[j] = ok_ && mode != SG_FIRST ? out[(long long)k_ * hw + pix_n] : 0.0;                        \
        }                                                                                                   \
    }
    SG_FETCH(lo)
    __syncthreads();
    bool bad = false;
    int cur = 0;
    for (int step = lo; step <= hi; ++step) {
        const double* __restrict__ prev = sg_lds + cur * rows;
        double* __restrict__ next = sg_lds + (cur ^ 1) * rows;
        const double* __restrict__ rp = red + cur * 4 * SG_MAX_G;
        const double m = sg_min(sg_min(rp[g], rp[SG_MAX_G + g]), sg_min(rp[2 * SG_MAX_G + g], rp[3 * SG_MAX_G + g]));
        const bool restart = !(m < inf);
        const double jump = m + p2;
        const bool in = in_n;
        const long long pix = pix_n;
        double cc[ITEMS], tt[ITEMS];
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) { cc[j] = cn[j]; tt[j] = tn[j]; }
        if (step < hi) SG_FETCH(step + 1)
        double mine = inf;
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const int k = kq + j * kstride;
            if (k < D) {
                const double s = cc[j];
                double L = inf;
                if (s == s) {
                    bad = bad || isinf(s);
                    const double cost = 1.0 - s;
                    if (restart) L = cost;
                    else {
                        const double best = sg_min(sg_min(prev[(k + 1) * G + g], prev[k * G + g] + p1), sg_min(prev[(k + 2) * G + g] + p1, jump));
                        L = cost + (best - m);
                    }
                    const long long at = (long long)k * hw + pix;
                    if (mode == SG_FIRST) out[at] = L;
                    else if (mode == SG_ADD) out[at] = tt[j] + L;
                    else out[at] = 1.0 - (tt[j] + L) * inv_paths;              // inv_paths is 1/4 or 1/8: the product is the exact quotient
                    mine = sg_min(mine, L);
                } else if (in && mode == SG_FIRST) out[(long long)k * hw + pix] = ps_nan();
                next[(k + 1) * G + g] = L;
            }
        }
        for (int d = G; d < 64; d <<= 1) mine = sg_min(mine, __shfl_xor(mine, d));
        if ((t & 63) < G) red[(cur ^ 1) * 4 * SG_MAX_G + wave * SG_MAX_G + g] = mine;
        __syncthreads();
        cur ^= 1;
    }
#undef SG_FETCH
    if (__ballot(bad) && (t & 63) == 0) atomicOr(errword, (unsigned long long)MVSDF_PS_ERR_FINITE);
}

// ---- host side of the regularisation ----
static bool sg_limits(long long R, long long S, long long D) {
    return R >= 1 && S >= 1 && D >= 1 && D <= MVSDF_PS_MAX_D_SGM && R <= INT_MAX && S <= INT_MAX && R * S <= INT_MAX && R * S * D <= PS_MAX_ELEMS;
}

static bool sg_args(double p1, double p2, int paths) { return isfinite(p1) && isfinite(p2) && p1 >= 0.0 && p1 <= p2 && (paths == 4 || paths == 8); }

template <int ITEMS>
static int sg_launch(unsigned grid, size_t lds, hipStream_t s, const double* score, double* out, int R, int S, int D, const SgDir& dir, int lg, double p1,
                     double p2, int mode, double inv_paths, unsigned long long* errword) {
    static size_t allowed = 48 * 1024;                                    // above it the kernel has to be told (once per size)
    if (lds > allowed) {
        if (int rc = mv_check(hipFuncSetAttribute((const void*)k_sg_path<ITEMS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "mvsdf_stereo_regularize"))
            return rc;
        allowed = lds;
    }
    hipLaunchKernelGGL(k_sg_path<ITEMS>, dim3(grid), dim3(PS_THREADS), lds, s, score, out, R, S, D, dir, lg, p1, p2, mode, inv_paths, errword);
    return 0;
}

// the launches of one volume: out = A(score).  The limits and the arguments have been checked.
static int sg_run(const double* score, double* out, long long R, long long S, long long D, double p1, double p2, int paths, unsigned long long* errword,
                  hipStream_t s) {
    static const int DIRS[8][2] = {{0, 1}, {0, -1}, {1, 0}, {-1, 0}, {1, 1}, {-1, -1}, {1, -1}, {-1, 1}};       // (dy, dx), the definition's order
    int lgv = 0, lgh = 0;                                                 // log2 G of the directions with dy != 0 / of the horizontal ones
    while ((2 << lgv) <= SG_MAX_G && (long long)(2 << lgv) * D <= SG_MAX_ITEMS) ++lgv;
    while (lgh < lgv && (long long)(1 << lgh) * D < PS_THREADS) ++lgh;
    for (int h = 0; h < 2; ++h)                                           // development library only: MVSDF_SGM_LGV / MVSDF_SGM_LGH = log2 G, for timing other bundles
        if (const char* e = mv_dev_env(h ? "MVSDF_SGM_LGH" : "MVSDF_SGM_LGV")) {
            const int v = atoi(e);
            if (v >= 0 && (1 << v) <= SG_MAX_G && ((long long)D << v) <= 16 * PS_THREADS && (v == 0 || ((long long)D << v) <= SG_MAX_ITEMS)) (h ? lgh : lgv) = v;
        }
    for (int r = 0; r < paths; ++r) {
        const int dy = DIRS[r][0], dx = DIRS[r][1];
        SgDir d;
        int lg;
        if (dy != 0) {
            d.py0 = dy > 0 ? 0 : (int)R - 1; d.cy = 0; d.ty = dy;
            d.px0 = 0; d.cx = 1; d.tx = dx;
            d.c0 = dx > 0 ? -((int)R - 1) : 0;
            d.npaths = (int)S + (dx != 0 ? (int)R - 1 : 0);
            d.nsteps = (int)R;
            lg = lgv;
        } else {
            d.py0 = 0; d.cy = 1; d.ty = 0;
            d.px0 = dx > 0 ? 0 : (int)S - 1; d.cx = 0; d.tx = dx;
            d.c0 = 0;
            d.npaths = (int)R;
            d.nsteps = (int)S;
            lg = lgh;
        }
        const unsigned grid = (unsigned)mv_ceil_div(d.npaths, 1 << lg);
        const size_t lds = (size_t)(2 * (D + 2) * (1 << lg) + 2 * 4 * SG_MAX_G) * 8;
        const long long need = mv_ceil_div(D << lg, PS_THREADS);          // hypotheses per lane
        const int mode = r == 0 ? SG_FIRST : r == paths - 1 ? SG_LAST : SG_ADD;
        const double inv = 1.0 / (double)paths;
        int rc;
#define SG_GO(N) sg_launch<N>(grid, lds, s, score, out, (int)R, (int)S, (int)D, d, lg, p1, p2, mode, inv, errword)
        if (need <= 1) rc = SG_GO(1);
        else if (need <= 2) rc = SG_GO(2);
        else if (need <= 4) rc = SG_GO(4);
        else if (need <= 8) rc = SG_GO(8);
        else rc = SG_GO(16);
#undef SG_GO
        if (rc) return rc;
    }
    return 0;
}

// mvsdf_stereo_sweep (sgm false) and mvsdf_stereo_sweep_sgm: per view the scores, the regularisation where asked for, the pick
static int ps_sweep(const char* what, bool sgm, double p1, double p2, int paths, const float* desc, int64_t V, int64_t R, int64_t S, int64_t C, int64_t nviews,
                    const int32_t* views, const int32_t* pair_off, const int32_t* pair_src, const double* mats, const double* ranges, const int32_t* nhyp,
                    void* ws, size_t ws_bytes, float* depths, float* probs, int32_t* best_k, int32_t* counts, void* stream) {
    if (!desc || !views || !pair_off || !mats || !ranges || !nhyp || !ws || !depths || !probs || !best_k || !counts || nviews < 0 || ws_bytes < PS_HDR)
        return mv_fail(-1, "mvsdf_stereo_sweep: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    // ---- validation, all of it before the first launch ----
    long long err = 0, npairs = 0, dmax = 1;
    if (V < 1 || V > INT_MAX || R < 2 || S < 2 || C < 1 || C > INT_MAX || nviews > INT_MAX || pair_off[0] != 0) err |= MVSDF_PS_ERR_SHAPE;
    else {
        for (long long i = 0; i < nviews; ++i) {
            const long long len = (long long)pair_off[i + 1] - pair_off[i];
            if (len < 0 || len > MVSDF_PS_MAX_SRC) err |= MVSDF_PS_ERR_SHAPE;
            if (views[i] < 0 || views[i] >= V) err |= MVSDF_PS_ERR_PAIR;
            if (nhyp[i] < 1 || nhyp[i] > MVSDF_PS_MAX_D) err |= MVSDF_PS_ERR_DEPTHS;
            else if (nhyp[i] > dmax) dmax = nhyp[i];
            if (!isfinite(ranges[2 * i]) || !isfinite(ranges[2 * i + 1])) err |= MVSDF_PS_ERR_FINITE;
        }
        npairs = pair_off[nviews];
    }
    PsLayout L;
    if (!(err & MVSDF_PS_ERR_SHAPE) && (!ps_layout(R, S, dmax, npairs, &L) || (npairs > 0 && !pair_src) || R * S > PS_MAX_ELEMS / C || V > PS_MAX_ELEMS / (R * S * C)))
        err |= MVSDF_PS_ERR_SHAPE;
    if (sgm && (!sg_args(p1, p2, paths) || dmax > MVSDF_PS_MAX_D_SGM)) err |= MVSDF_PS_ERR_SGM;
    if (!(err & MVSDF_PS_ERR_SHAPE)) {
        for (long long k = 0; k < npairs; ++k)
            if (pair_src[k] < 0 || pair_src[k] >= V) err |= MVSDF_PS_ERR_PAIR;
        if (!mv_all_finite(mats, npairs * 16)) err |= MVSDF_PS_ERR_FINITE;
    }
    if (err) return mv_refuse_header(ws, err, s, what);
    if (ws_bytes < L.total + (sgm ? mv_align256((size_t)(R * S * dmax) * 8) : 0))
        return mv_fail(-1, "mvsdf_stereo_sweep: workspace too small (mvsdf_stereo_workspace_bytes / mvsdf_stereo_sweep_sgm_workspace_bytes)");
    // ---- uploads and launches ----
    char* w = (char*)ws;
    int rc;
    if ((rc = mv_check(hipMemsetAsync(ws, 0, PS_HDR, s), what))) return rc;
    if (npairs > 0) {
        if ((rc = mv_check(hipMemcpyAsync(w + L.mats, mats, (size_t)npairs * 16 * 8, hipMemcpyHostToDevice, s), what))) return rc;
        if ((rc = mv_check(hipMemcpyAsync(w + L.src, pair_src, (size_t)npairs * 4, hipMemcpyHostToDevice, s), what))) return rc;
    }
    const long long hw = R * S, total = V * hw * C;
    long long fb = mv_ceil_div(total, MV_THREADS);
    if (fb > 2048) fb = 2048;
    hipLaunchKernelGGL(k_any_nonfinite<float>, dim3((unsigned)fb), dim3(MV_THREADS), 0, s, desc, total, (unsigned long long*)ws + MVSDF_RES_H_ERR, (unsigned long long)MVSDF_PS_ERR_FINITE);
    const bool fast = C == 32 && ((uintptr_t)desc & 15) == 0;                 // 128-byte texels read as float4
    double* vol = (double*)(w + L.vol);
    unsigned char* cnt = (unsigned char*)(w + L.cnt);
    double* reg = (double*)(w + L.total);                                    // the regularised volume (sgm)
    for (long long i = 0; i < nviews; ++i) {
        const int r = views[i], D = nhyp[i], nsrc = pair_off[i + 1] - pair_off[i];
        const int* src = (const int*)(w + L.src) + pair_off[i];
        const double* T = (const double*)(w + L.mats) + (long long)pair_off[i] * 16;
        const dim3 grid((unsigned)mv_ceil_div(S, PS_TILE), (unsigned)mv_ceil_div(R, PS_TILE), (unsigned)mv_ceil_div(D, PS_KCHUNK));
        if (grid.y > 65535) return mv_fail(-1, "mvsdf_stereo_sweep: R beyond the grid limit");
        if (fast)
            hipLaunchKernelGGL(k_ps_score<32>, grid, dim3(PS_THREADS), 0, s, desc, (int)R, (int)S, (int)C, r, nsrc, src, T, ranges[2 * i], ranges[2 * i + 1], D,
                               vol, cnt);
        else
            hipLaunchKernelGGL(k_ps_score<0>, grid, dim3(PS_THREADS), 0, s, desc, (int)R, (int)S, (int)C, r, nsrc, src, T, ranges[2 * i], ranges[2 * i + 1], D,
                               vol, cnt);
        if (sgm) {
            if ((rc = sg_run(vol, reg, R, S, D, p1, p2, paths, (unsigned long long*)ws + MVSDF_RES_H_ERR, s))) return rc;
            hipLaunchKernelGGL(k_ps_pick<true>, dim3(mv_grid(hw, PS_THREADS)), dim3(PS_THREADS), 0, s, (const double*)reg, (const double*)vol,
                               (const unsigned char*)cnt, (int)hw, D, ranges[2 * i], ranges[2 * i + 1], nsrc, depths + (long long)r * hw,
                               probs + (long long)r * 3 * hw, best_k + (long long)r * hw, counts + (long long)r * hw);
        } else
            hipLaunchKernelGGL(k_ps_pick<false>, dim3(mv_grid(hw, PS_THREADS)), dim3(PS_THREADS), 0, s, (const double*)vol, (const double*)vol,
                               (const unsigned char*)cnt, (int)hw, D, ranges[2 * i], ranges[2 * i + 1], nsrc, depths + (long long)r * hw,
                               probs + (long long)r * 3 * hw, best_k + (long long)r * hw, counts + (long long)r * hw);
    }
    return mv_check(hipGetLastError(), what);                   // no wait here: the caller keeps the host arrays until it has read the header
}


// ---- host side of the band sweep ----
struct PbLayout {
    size_t views, off, steps, mats, src, total;
};

// header, per view its index, first pair slot and step, matrices and source indices: nothing that grows with the band, R or S
static bool pb_layout(long long R, long long S, long long Db, long long nviews, long long npairs, PbLayout* L) {
    if (R < 2 || S < 2 || R > INT_MAX || S > INT_MAX || R * S > INT_MAX || Db < 1 || Db > MVSDF_PS_MAX_D_BAND || nviews < 0 || nviews > 65535 || npairs < 0 ||
        npairs > INT_MAX)
        return false;
    WsCursor c{PS_HDR};
    L->views = c.take((size_t)(nviews > 0 ? nviews : 1) * 4);
    L->off = c.take((size_t)(nviews + 1) * 4);
    L->steps = c.take((size_t)(nviews > 0 ? nviews : 1) * 8);
    L->mats = c.take((size_t)(npairs > 0 ? npairs : 1) * 16 * 8);
    L->src = c.take((size_t)(npairs > 0 ? npairs : 1) * 4);
    L->total = c.o;
    return true;
}


extern "C" {

size_t mvsdf_stereo_workspace_bytes(int64_t R, int64_t S, int64_t D, int64_t npairs) {
    PsLayout L;
    return ps_layout(R, S, D, npairs, &L) ? L.total : 0;
}

size_t mvsdf_stereo_volume_offset(int64_t R, int64_t S, int64_t D, int64_t npairs) {
    PsLayout L;
    return ps_layout(R, S, D, npairs, &L) ? L.vol : 0;
}

int mvsdf_stereo_normalize(const float* feats, int64_t n, int64_t C, float* out, void* hdr, void* stream) {
    const char* what = "mvsdf_stereo_normalize";
    if (!feats || !out || !hdr || n < 1 || C < 1 || C > INT_MAX || n > PS_MAX_ELEMS / C || mv_ceil_div(n, PS_THREADS) > INT_MAX)
        return mv_fail(-1, "mvsdf_stereo_normalize: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = mv_check(hipMemsetAsync(hdr, 0, MVSDF_RES_H_WORDS * 8, s), what)) return rc;
    hipLaunchKernelGGL(k_ps_normalize, dim3(mv_grid(n, PS_THREADS)), dim3(PS_THREADS), 0, s, feats, (long long)n, (int)C, out, (long long*)hdr);
    return mv_check(hipGetLastError(), what);
}

int mvsdf_stereo_patches(const uint8_t* images, int64_t V, int64_t H, int64_t W, int32_t radius, float* out, void* stream) {
    if (!images || !out || V < 1 || H < 1 || W < 1 || H > INT_MAX || W > INT_MAX || H * W > INT_MAX || radius < 0 || radius > 15 ||
        V > PS_MAX_ELEMS / (H * W) / ((2 * radius + 1) * (2 * radius + 1)) || mv_ceil_div(V * H * W, PS_THREADS) > INT_MAX)
        return mv_fail(-1, "mvsdf_stereo_patches: bad arguments");
    hipLaunchKernelGGL(k_ps_patches, dim3(mv_grid(V * H * W, PS_THREADS)), dim3(PS_THREADS), 0, (hipStream_t)stream, images, (long long)V, (int)H,
                       (int)W, (int)radius, out);
    return mv_check(hipGetLastError(), "mvsdf_stereo_patches");
}

int mvsdf_stereo_sweep(const float* desc, int64_t V, int64_t R, int64_t S, int64_t C, int64_t nviews, const int32_t* views, const int32_t* pair_off,
                       const int32_t* pair_src, const double* mats, const double* ranges, const int32_t* nhyp, void* ws, size_t ws_bytes, float* depths,
                       float* probs, int32_t* best_k, int32_t* counts, void* stream) {
    return ps_sweep("mvsdf_stereo_sweep", false, 0.0, 0.0, 0, desc, V, R, S, C, nviews, views, pair_off, pair_src, mats, ranges, nhyp, ws, ws_bytes, depths,
                    probs, best_k, counts, stream);
}

size_t mvsdf_stereo_sgm_workspace_bytes(int64_t R, int64_t S, int64_t D) { return sg_limits(R, S, D) ? PS_HDR : 0; }

int mvsdf_stereo_regularize(const double* score, int64_t R, int64_t S, int64_t D, double p1, double p2, int32_t paths, void* ws, size_t ws_bytes,
                            double* out, void* stream) {
    const char* what = "mvsdf_stereo_regularize";
    if (!score || !out || !ws || ws_bytes < PS_HDR) return mv_fail(-1, "mvsdf_stereo_regularize: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (!sg_limits(R, S, D) || !sg_args(p1, p2, paths)) return mv_refuse_header(ws, MVSDF_PS_ERR_SGM, s, what);
    const size_t bytes = (size_t)(R * S * D) * 8;
    if ((const char*)score < (const char*)out + bytes && (const char*)out < (const char*)score + bytes)
        return mv_fail(-1, "mvsdf_stereo_regularize: out overlaps score");
    if (int rc = mv_check(hipMemsetAsync(ws, 0, PS_HDR, s), what)) return rc;
    if (int rc = sg_run(score, out, R, S, D, p1, p2, paths, (unsigned long long*)ws + MVSDF_RES_H_ERR, s)) return rc;
    return mv_check(hipGetLastError(), what);
}

size_t mvsdf_stereo_sweep_sgm_workspace_bytes(int64_t R, int64_t S, int64_t D, int64_t npairs) {
    PsLayout L;
    return ps_layout(R, S, D, npairs, &L) && D <= MVSDF_PS_MAX_D_SGM ? L.total + mv_align256((size_t)(R * S * D) * 8) : 0;
}

int mvsdf_stereo_sweep_sgm(const float* desc, int64_t V, int64_t R, int64_t S, int64_t C, int64_t nviews, const int32_t* views,
                           const int32_t* pair_off, const int32_t* pair_src, const double* mats, const double* ranges, const int32_t* nhyp, double p1,
                           double p2, int32_t paths, void* ws, size_t ws_bytes, float* depths, float* probs, int32_t* best_k, int32_t* counts,
                           void* stream) {
    return ps_sweep("mvsdf_stereo_sweep_sgm", true, p1, p2, paths, desc, V, R, S, C, nviews, views, pair_off, pair_src, mats, ranges, nhyp, ws, ws_bytes,
                    depths, probs, best_k, counts, stream);
}

int mvsdf_stereo_upsample(const float* depth, const int32_t* best_k, int64_t V, int64_t r, int64_t s, int64_t R, int64_t S, double* out, void* stream) {
    if (!depth || !best_k || !out || V < 1 || r < 2 || s < 2 || R < 1 || S < 1 || r > INT_MAX || s > INT_MAX || r * s > INT_MAX || R > INT_MAX ||
        S > INT_MAX || R * S > INT_MAX || V > PS_MAX_ELEMS / (R * S) || V > PS_MAX_ELEMS / (r * s) || mv_ceil_div(V * R * S, PS_THREADS) > INT_MAX)
        return mv_fail(-1, "mvsdf_stereo_upsample: bad arguments");
    hipLaunchKernelGGL(k_ps_upsample, dim3(mv_grid(V * R * S, PS_THREADS)), dim3(PS_THREADS), 0, (hipStream_t)stream, depth, best_k, (long long)V, (int)r,
                       (int)s, (int)R, (int)S, out);
    return mv_check(hipGetLastError(), "mvsdf_stereo_upsample");
}

size_t mvsdf_stereo_band_workspace_bytes(int64_t R, int64_t S, int64_t depth_num, int64_t nviews, int64_t npairs) {
    PbLayout L;
    return pb_layout(R, S, depth_num, nviews, npairs, &L) ? L.total : 0;
}

int mvsdf_stereo_band(const float* desc, int64_t V, int64_t R, int64_t S, int64_t C, int64_t nviews, const int32_t* views, const int32_t* pair_off,
                      const int32_t* pair_src, const double* mats, const double* steps, const double* centres, int32_t depth_num, void* ws,
                      size_t ws_bytes, float* depths, float* probs, int32_t* best_k, int32_t* counts, void* stream) {
    const char* what = "mvsdf_stereo_band";
    if (!desc || !views || !pair_off || !mats || !steps || !centres || !ws || !depths || !probs || !best_k || !counts || nviews < 1 || ws_bytes < PS_HDR)
        return mv_fail(-1, "mvsdf_stereo_band: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    // ---- validation, all of it before the first launch ----
    long long err = 0, npairs = 0;
    if (V < 1 || V > INT_MAX || R < 2 || S < 2 || C < 1 || C > INT_MAX || nviews > 65535 || pair_off[0] != 0) err |= MVSDF_PS_ERR_SHAPE;
    else {
        for (long long i = 0; i < nviews; ++i) {
            const long long len = (long long)pair_off[i + 1] - pair_off[i];
            if (len < 0 || len > MVSDF_PS_MAX_SRC) err |= MVSDF_PS_ERR_SHAPE;
            if (views[i] < 0 || views[i] >= V) err |= MVSDF_PS_ERR_PAIR;
            for (long long j = 0; j < i; ++j)
                if (views[j] == views[i]) err |= MVSDF_PS_ERR_BAND;                  // two workgroups would write the same maps
            if (!(isfinite(steps[i]) && steps[i] > 0.0)) err |= MVSDF_PS_ERR_BAND;
        }
        npairs = pair_off[nviews];
    }
    if (depth_num < 1 || depth_num > MVSDF_PS_MAX_D_BAND) err |= MVSDF_PS_ERR_BAND;
    PbLayout L;
    if (!(err & (MVSDF_PS_ERR_SHAPE | MVSDF_PS_ERR_BAND)) &&
        (!pb_layout(R, S, depth_num, nviews, npairs, &L) || (npairs > 0 && !pair_src) || R * S > PS_MAX_ELEMS / C || V > PS_MAX_ELEMS / (R * S * C)))
        err |= MVSDF_PS_ERR_SHAPE;
    if (!(err & MVSDF_PS_ERR_SHAPE)) {
        for (long long k = 0; k < npairs; ++k)
            if (pair_src[k] < 0 || pair_src[k] >= V) err |= MVSDF_PS_ERR_PAIR;
        if (!mv_all_finite(mats, npairs * 16)) err |= MVSDF_PS_ERR_FINITE;
    }
    if (err) return mv_refuse_header(ws, err, s, what);
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_stereo_band: workspace too small (mvsdf_stereo_band_workspace_bytes)");
    const dim3 grid((unsigned)mv_ceil_div(S, PB_TILE), (unsigned)mv_ceil_div(R, PB_TILE), (unsigned)nviews);
    if (grid.y > 65535) return mv_fail(-1, "mvsdf_stereo_band: R beyond the grid limit");
    // ---- uploads and the one launch ----
    char* w = (char*)ws;
    int rc;
    if ((rc = mv_check(hipMemsetAsync(ws, 0, PS_HDR, s), what))) return rc;
    if ((rc = mv_check(hipMemcpyAsync(w + L.views, views, (size_t)nviews * 4, hipMemcpyHostToDevice, s), what))) return rc;
    if ((rc = mv_check(hipMemcpyAsync(w + L.off, pair_off, (size_t)(nviews + 1) * 4, hipMemcpyHostToDevice, s), what))) return rc;
    if ((rc = mv_check(hipMemcpyAsync(w + L.steps, steps, (size_t)nviews * 8, hipMemcpyHostToDevice, s), what))) return rc;
    if (npairs > 0) {
        if ((rc = mv_check(hipMemcpyAsync(w + L.mats, mats, (size_t)npairs * 16 * 8, hipMemcpyHostToDevice, s), what))) return rc;
        if ((rc = mv_check(hipMemcpyAsync(w + L.src, pair_src, (size_t)npairs * 4, hipMemcpyHostToDevice, s), what))) return rc;
    }
    const long long total = V * R * S * C;
    long long fb = mv_ceil_div(total, MV_THREADS);
    if (fb > 2048) fb = 2048;
    hipLaunchKernelGGL(k_any_nonfinite<float>, dim3((unsigned)fb), dim3(MV_THREADS), 0, s, desc, total, (unsigned long long*)ws + MVSDF_RES_H_ERR, (unsigned long long)MVSDF_PS_ERR_FINITE);
    const size_t lds = (size_t)depth_num * 64 * 9;
    if (C == 32 && ((uintptr_t)desc & 15) == 0)                               // 128-byte texels read as float4
        hipLaunchKernelGGL(k_ps_band<32>, grid, dim3(PS_THREADS), lds, s, desc, (int)R, (int)S, (int)C, (const int*)(w + L.views), (const int*)(w + L.off),
                           (const double*)(w + L.steps), (const int*)(w + L.src),
                           (const double*)(w + L.mats), centres, (int)depth_num, depths, probs, best_k, counts, (unsigned long long*)ws + MVSDF_RES_H_ERR);
    else
        hipLaunchKernelGGL(k_ps_band<0>, grid, dim3(PS_THREADS), lds, s, desc, (int)R, (int)S, (int)C, (const int*)(w + L.views), (const int*)(w + L.off),
                           (const double*)(w + L.steps), (const int*)(w + L.src),
                           (const double*)(w + L.mats), centres, (int)depth_num, depths, probs, best_k, counts, (unsigned long long*)ws + MVSDF_RES_H_ERR);
    return mv_check(hipGetLastError(), what);                   // no wait here: the caller keeps the host arrays until it has read the header
}

}  // extern "C"
