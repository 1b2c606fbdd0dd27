// keypoints.hip -- sparse points from posed images on the device, the stages behind the detector: all-pairs matching of 128-d int8 descriptors with a
// ratio test on the int8 matrix cores, epipolar verification, tracks, multi-view triangulation.  Python: mvsdf_amd/keypoints.py, which states every
// definition; tests/keypoints_ref.py restates them in numpy.  fp64 arithmetic is uncontracted and in the order the definitions write it; everything
// else is integers.
//
// * The matcher.  D(i,j) = |s_i|^2 + |t_j|^2 - 2 s_i . t_j on integers.  k_kp_pack writes every code row as 128 bytes and minus its squared norm;
//   the rows of a view start at a multiple of 16 (pad_off) and the gap is filled with zero rows of "norm" KP_PAD_NORM, so no tile crosses a view.
//   k_kp_match: a wave owns 16 sources of one directed job (pair m, direction d: blockIdx.z = 2 m + d) and two v_mfma_i32_16x16x64_i8 into one
//   accumulator give the 16 x 16 dot products of a target tile: A = the targets (rows of the result), B = the sources (columns, `lane & 15`).
//   Lane l carries bytes 64 q + 16 (l >> 4) .. + 15 of row / column l & 15 for k-step q.  The sources' fragments and norms stay in registers for
//   the whole walk; every lane keeps the best (e, j) and the second-best e over its four rows per tile, e = 2 s.t - |t|^2, ascending j with strict
//   comparisons (so an equal distance later in the walk becomes the second, never the best); at the end the four lane groups merge by two xor
//   shuffles and lane group 0 writes (D1 << 32 | j1, D2) to the slot of (source, split): an atomicMin cannot carry a second-best.  The target tiles
//   are split over blockIdx.y while the grid is small.  k_kp_match_final merges the splits of a source, applies the ratio test, max_dist and the
//   mutual check (the merged slots of the other direction), and the shared scan compacts.  No distance matrix reaches memory.
// * k_kp_verify: one lane per match.  * Tracks: minimum-label rounds over the edges with pointer jumping, the stable radix sort of (label, node),
//   integer atomics for the size and the conflict of a component, two scans, one emit.  * k_kp_triangulate: one lane per track.
//
// Every device loop is bounded; no kernel waits on another.  Integer atomics only.
#include <vector>
#include "det_math64.h"
#include "nn_tree.h"

#define KP_ROW MVSDF_KP_DIM                           // bytes of a packed code row: two k-steps of four 16-byte operand chunks
#define KP_WAVES 4                                    // waves of a matcher workgroup, 16 sources each
#define KP_UNROLL 2                                   // target tiles whose loads a wave keeps in flight
#define KP_TARGET_BLOCKS 2048                         // the matcher splits the targets until about this many workgroups exist ...
#define KP_MIN_TILES 16                               // ... but no split walks fewer than this many 16-target tiles
#define KP_PAD_NORM (-0x3fffffff)                     // the "norm" of a padding row: below every 2 s.t - |t|^2, and |s|^2 minus it still fits an int
#define KP_SEARCH 32                                  // steps of a binary search over at most 2^31 offsets
#define KP_JUMPS 64                                   // pointer jumps of a node per round

typedef int kp_v4i __attribute__((ext_vector_type(4)));
typedef unsigned long long kp_u64;

// one directed search: the sources and targets as packed rows (starts are multiples of 16), and where its (source, split) slots begin
struct KpJob {
    long long s0, ns, t0, nt, slot;
};

// the largest v in [0, n) with off[v] <= x, given off[0] <= x < off[n]
__device__ __forceinline__ long long kp_find(const long long* __restrict__ off, long long n, long long x) {
    long long lo = 0, hi = n;
    for (int it = 0; it < KP_SEARCH && hi - lo > 1; ++it) {
        const long long mid = lo + (hi - lo) / 2;
        if (off[mid] <= x)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// ================================================================ the scale space ================================================================
template <class T>
static __global__ __launch_bounds__(CH_THREADS) void k_kp_grey(const T* __restrict__ img, int channels, long long n, double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n) return;
    if (channels == 1) {
        out[i] = (double)img[i];
        return;
    }
    const T* q = img + 3 * i;
    if (sizeof(T) == 1)
        out[i] = (double)(299 * (int)q[0] + 587 * (int)q[1] + 114 * (int)q[2]) / 1000.0;
    else
        out[i] = ((299.0 * (double)q[0] + 587.0 * (double)q[1]) + 114.0 * (double)q[2]) / 1000.0;
}

// one pass of the separable blur: along x (ALONG_X) or along y, the sum from 0.0 over the taps in their order, the coordinate clamped
template <bool ALONG_X>
static __global__ __launch_bounds__(CH_THREADS) void k_kp_blur(const double* __restrict__ src, long long planes, long long h, long long w,
                                                               const double* __restrict__ taps, int r, double* __restrict__ dst) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= planes * h * w) return;
    const long long x = i % w, y = (i / w) % h;
    const double* __restrict__ row = ALONG_X ? src + (i - x) : src + (i - y * w);     // the pixel's row, or the top of its column
    double s = 0.0;
    for (int k = 0; k <= 2 * r; ++k) {                           // bounded: 2 MVSDF_KP_MAX_RADIUS + 1
        long long c = (ALONG_X ? x : y) + k - r;
        c = c < 0 ? 0 : c;
        c = c > (ALONG_X ? w : h) - 1 ? (ALONG_X ? w : h) - 1 : c;
        s = s + taps[k] * (ALONG_X ? row[c] : row[c * w]);
    }
    dst[i] = s;
}

static __global__ __launch_bounds__(CH_THREADS) void k_kp_half(const double* __restrict__ src, long long planes, long long h, long long w,
                                                               double* __restrict__ dst) {
    const long long h2 = (h + 1) / 2, w2 = (w + 1) / 2;
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= planes * h2 * w2) return;
    const long long x = i % w2, y = (i / w2) % h2, p = i / (w2 * h2);
    dst[i] = src[(p * h + 2 * y) * w + 2 * x];
}

static __global__ __launch_bounds__(CH_THREADS) void k_kp_dog(const double* __restrict__ L, long long planes, long long levels, long long hw,
                                                              double* __restrict__ D) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= planes * (levels - 1) * hw) return;
    const long long q = i % hw, s = (i / hw) % (levels - 1), p = i / (hw * (levels - 1));
    const double* __restrict__ a = L + (p * levels + s) * hw + q;
    D[i] = a[hw] - a[0];
}

// ---- extrema of the differences with their one quadratic step ----
__device__ __forceinline__ double kp_det3(double a00, double a01, double a02, double a10, double a11, double a12, double a20, double a21, double a22) {
    return (a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20)) + a02 * (a10 * a21 - a11 * a20);
}

// site (s, y, x) of one view's D [5][h][w], 1 <= s <= 3, inside the border: is it a kept extremum, and its offsets and response
__device__ __forceinline__ bool kp_extremum(const double* __restrict__ D, long long h, long long w, int s, long long y, long long x, double contrast,
                                            double edge_r, double* o, double* resp) {
    const long long hw = h * w;
    const double* __restrict__ c = D + s * hw + y * w + x;
    const double v = c[0];
    if (!(fabs(v) > contrast)) return false;
    bool gt = true, lt = true;
    for (int ds = -1; ds <= 1; ++ds)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if (!ds && !dy && !dx) continue;
                const double q = c[ds * hw + dy * w + dx];
                gt = gt && v > q;
                lt = lt && v < q;
            }
    if (!gt && !lt) return false;
    const double dxx = (c[1] + c[-1]) - 2.0 * v, dyy = (c[w] + c[-w]) - 2.0 * v, dss = (c[hw] + c[-hw]) - 2.0 * v;
    const double dxy = 0.25 * ((c[w + 1] - c[w - 1]) - (c[-w + 1] - c[-w - 1]));
    const double dxs = 0.25 * ((c[hw + 1] - c[hw - 1]) - (c[-hw + 1] - c[-hw - 1]));
    const double dys = 0.25 * ((c[hw + w] - c[hw - w]) - (c[-hw + w] - c[-hw - w]));
    const double tr = dxx + dyy, de = dxx * dyy - dxy * dxy;
    if (!(de > 0.0) || !((tr * tr) * edge_r < ((edge_r + 1.0) * (edge_r + 1.0)) * de)) return false;
    const double gx = 0.5 * (c[1] - c[-1]), gy = 0.5 * (c[w] - c[-w]), gs = 0.5 * (c[hw] - c[-hw]);
    const double det = kp_det3(dxx, dxy, dxs, dxy, dyy, dys, dxs, dys, dss);
    if (det == 0.0 || !isfinite(det)) return false;
    o[0] = kp_det3(-gx, dxy, dxs, -gy, dyy, dys, -gs, dys, dss) / det;
    o[1] = kp_det3(dxx, -gx, dxs, dxy, -gy, dys, dxs, -gs, dss) / det;
    o[2] = kp_det3(dxx, dxy, -gx, dxy, dyy, -gy, dxs, dys, -gs) / det;
    if (!(fabs(o[0]) <= 0.5 && fabs(o[1]) <= 0.5 && fabs(o[2]) <= 0.5)) return false;
    *resp = fabs(v + 0.5 * ((gx * o[0] + gy * o[1]) + gs * o[2]));
    return true;
}

struct KpSite {
    long long v, y, x;
    int s;
    bool inside;
};

// flat site i of [V][3][h][w] (levels 1 .. 3)
__device__ __forceinline__ KpSite kp_site(long long i, long long h, long long w, int border) {
    KpSite q;
    q.x = i % w;
    q.y = (i / w) % h;
    q.s = (int)((i / (w * h)) % 3) + 1;
    q.v = i / (w * h * 3);
    q.inside = q.x >= border && q.x < w - border && q.y >= border && q.y < h - border;
    return q;
}

static __global__ __launch_bounds__(CH_THREADS) void k_kp_extrema_flag(const double* __restrict__ D, long long n, long long h, long long w, double contrast,
                                                                       double edge_r, int border, unsigned char* __restrict__ flag) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n) return;
    const KpSite q = kp_site(i, h, w, border);
    double o[3], resp;
    flag[i] = q.inside && kp_extremum(D + q.v * 5 * h * w, h, w, q.s, q.y, q.x, contrast, edge_r, o, &resp) ? 1 : 0;
}

static __global__ __launch_bounds__(CH_THREADS) void k_kp_extrema_emit(const double* __restrict__ D, long long n, long long h, long long w, double contrast,
                                                                       double edge_r, int border, double step, double s1, double s2, double s3,
                                                                       const unsigned char* __restrict__ flag, const long long* __restrict__ rank,
                                                                       long long cap, int* __restrict__ cand, double* __restrict__ out, long long* err) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const long long r = rank[i];
    if (r >= cap) {
        atomicOr((kp_u64*)err, (kp_u64)MVSDF_PS_ERR_SHAPE);
        return;
    }
    const KpSite q = kp_site(i, h, w, border);
    double o[3], resp = 0.0;
    kp_extremum(D + q.v * 5 * h * w, h, w, q.s, q.y, q.x, contrast, edge_r, o, &resp);
    cand[4 * r] = (int)q.v;
    cand[4 * r + 1] = q.s;
    cand[4 * r + 2] = (int)q.y;
    cand[4 * r + 3] = (int)q.x;
    out[4 * r] = (((double)q.x + o[0]) + 0.5) * step;
    out[4 * r + 1] = (((double)q.y + o[1]) + 0.5) * step;
    out[4 * r + 2] = (q.s == 1 ? s1 : q.s == 2 ? s2 : s3) * step;
    out[4 * r + 3] = resp;
}

// ---- the descriptor: 4 x 4 cells x 8 directions, trilinear votes quantised to 2^-32 and summed as integers; one lane per keypoint, its row of acc its own ----
#define KP_TWO_PI 6.283185307179586
struct KpDescTables {
    double cell[3], ogauss[3];
    int radius[3], oradius[3];
};

// the gradient of L at (py, px): magnitude and direction in (-pi, pi]
__device__ __forceinline__ void kp_gradient(const double* __restrict__ L, long long w, long long py, long long px, double* mag, double* t) {
    const double gx = L[py * w + px + 1] - L[py * w + px - 1], gy = L[(py + 1) * w + px] - L[(py - 1) * w + px];
    *mag = sqrt(gx * gx + gy * gy);
    const double a = dm64_atan2_pos(fabs(gy), gx);
    *t = gy < 0.0 ? -a : a;
}

static __global__ __launch_bounds__(CH_THREADS) void k_kp_describe(const double* __restrict__ Lv, long long V, long long h, long long w,
                                                                   const int* __restrict__ cand, long long n, int upright, KpDescTables tab,
                                                                   const double* __restrict__ trig, long long* __restrict__ acc,
                                                                   double* __restrict__ angle, signed char* __restrict__ codes,
                                                                   unsigned char* __restrict__ valid) {
    const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= n) return;
    long long* a = acc + i * MVSDF_KP_DIM;
    for (int q = 0; q < MVSDF_KP_DIM; ++q) {
        a[q] = 0;
        codes[i * MVSDF_KP_DIM + q] = 0;
    }
    valid[i] = 0;
    angle[i] = 0.0;
    const long long v = cand[4 * i], y = cand[4 * i + 2], x = cand[4 * i + 3];
    const int s = cand[4 * i + 1];
    if (v < 0 || v >= V || s < 1 || s > 3 || y < 0 || y >= h || x < 0 || x >= w) return;
    const double* __restrict__ L = Lv + (v * 6 + s) * h * w;
    const double hc = s == 1 ? tab.cell[0] : s == 2 ? tab.cell[1] : tab.cell[2];
    const int R = s == 1 ? tab.radius[0] : s == 2 ? tab.radius[1] : tab.radius[2];
    double co = 1.0, si = 0.0, ang = 0.0;
    if (!upright) {                                               // the 36-bin histogram lives in the first words of the lane's own row
        const double og = s == 1 ? tab.ogauss[0] : s == 2 ? tab.ogauss[1] : tab.ogauss[2];
        const int Ro = s == 1 ? tab.oradius[0] : s == 2 ? tab.oradius[1] : tab.oradius[2];
        for (int dy = -Ro; dy <= Ro; ++dy)
            for (int dx = -Ro; dx <= Ro; ++dx) {
                const long long px = x + dx, py = y + dy;
                if (px < 1 || px > w - 2 || py < 1 || py > h - 2) continue;
                double mag, t;
                kp_gradient(L, w, py, px, &mag, &t);
                if (t < 0.0) t = t + KP_TWO_PI;
                if (t >= KP_TWO_PI) t = t - KP_TWO_PI;
                int b = (int)floor(t * 5.729577951308232);      // 36 / (2 pi)
                b = b > 35 ? 35 : b;
                const double val = mag * dm64_expneg(-((double)(dx * dx + dy * dy) * og));
                a[b] += (long long)((val * 4294967296.0 + DM64_MAGIC) - DM64_MAGIC);
            }
        int best = 0;
        for (int b = 1; b < 36; ++b)
            if (a[b] > a[best]) best = b;                         // strict: the lowest bin wins a tie
        if (a[best] > 0) {
            const double l = (double)a[(best + 35) % 36], c = (double)a[best], r = (double)a[(best + 1) % 36];
            const double den = (l - 2.0 * c) + r;
            const double p = den == 0.0 ? 0.0 : (0.5 * (l - r)) / den;
            ang = (((double)best + 0.5) + p) * 0.17453292519943295;   // 2 pi / 36
            if (ang < 0.0) ang = ang + KP_TWO_PI;
            if (ang >= KP_TWO_PI) ang = ang - KP_TWO_PI;
            const double u = ang - DM64_PI, z = u * u;            // cos(ang) = -cos(u), sin(ang) = -sin(u), |u| <= pi
            double ps = trig[13], pc = trig[14 + 14];
            for (int k = 12; k >= 0; --k) ps = ps * z + trig[k];
            for (int k = 13; k >= 0; --k) pc = pc * z + trig[14 + k];
            si = -(u * ps);
            co = -pc;
        }
        for (int q = 0; q < 36; ++q) a[q] = 0;
        angle[i] = ang;
    }
    for (int dy = -R; dy <= R; ++dy)
        for (int dx = -R; dx <= R; ++dx) {                        // bounded: (8 MVSDF_KP_MAX_RADIUS + 1)^2
            const long long px = x + dx, py = y + dy;
            if (px < 1 || px > w - 2 || py < 1 || py > h - 2) continue;
            const double rx = (co * (double)dx + si * (double)dy) / hc, ry = (co * (double)dy - si * (double)dx) / hc;
            const double cx = rx + 1.5, cy = ry + 1.5;
            if (!(cx > -1.0 && cx < 4.0 && cy > -1.0 && cy < 4.0)) continue;
            double mag, t;
            kp_gradient(L, w, py, px, &mag, &t);
            double rel = t - ang;
            if (rel < 0.0) rel = rel + KP_TWO_PI;
            if (rel < 0.0) rel = rel + KP_TWO_PI;
            if (rel >= KP_TWO_PI) rel = rel - KP_TWO_PI;
            const double ob = rel * 1.2732395447351628;           // 8 / (2 pi)
            const double val = mag * dm64_expneg(-((rx * rx + ry * ry) * 0.125));
            const double x0 = floor(cx), y0 = floor(cy), o0 = floor(ob);
            const double fx = cx - x0, fy = cy - y0, fo = ob - o0;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int ix = (int)x0 + (q & 1), iy = (int)y0 + ((q >> 1) & 1), io = ((int)o0 + (q >> 2)) & 7;
                if (ix < 0 || ix > 3 || iy < 0 || iy > 3) continue;
                const double vote = ((val * ((q & 1) ? fx : 1.0 - fx)) * ((q & 2) ? fy : 1.0 - fy)) * ((q & 4) ? fo : 1.0 - fo);
                const double rq = (vote * 4294967296.0 + DM64_MAGIC) - DM64_MAGIC;
                a[(iy * 4 + ix) * 8 + io] += (long long)rq;
            }
        }
    double n1 = 0.0;
    for (int q = 0; q < MVSDF_KP_DIM; ++q) {
        const double u = (double)a[q] * 2.3283064365386963e-10;
        n1 = n1 + u * u;
    }
    n1 = sqrt(n1);
    if (!(n1 > 0.0)) return;
    double n2 = 0.0;
    for (int q = 0; q < MVSDF_KP_DIM; ++q) {
        double u = ((double)a[q] * 2.3283064365386963e-10) / n1;
        u = u > 0.2 ? 0.2 : u;
        n2 = n2 + u * u;
    }
    n2 = sqrt(n2);
    for (int q = 0; q < MVSDF_KP_DIM; ++q) {
        double u = ((double)a[q] * 2.3283064365386963e-10) / n1;
        u = u > 0.2 ? 0.2 : u;
        const double f = floor(512.0 * (u / n2));
        codes[i * MVSDF_KP_DIM + q] = (signed char)(f > 127.0 ? 127.0 : f);
    }
    valid[i] = 1;
}

// ================================================================ the matcher ================================================================
// packed row p of [npad][128]: the codes of keypoint view_off[v] + (p - pad_off[v]) of its view v, zeros (norm KP_PAD_NORM) in the gap behind the view
static __global__ __launch_bounds__(CH_THREADS) void k_kp_pack(const int* __restrict__ codes, const long long* __restrict__ view_off,
                                                               const long long* __restrict__ pad_off, long long V, long long npad,
                                                               int* __restrict__ packed, int* __restrict__ norm, long long* err) {
    const long long p = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (p >= npad) return;
    const long long v = kp_find(pad_off, V, p);
    const long long i = p - pad_off[v], n = view_off[v + 1] - view_off[v];
    const bool real = i < n;
    const int* row = codes + (view_off[v] + i) * (KP_ROW / 4);
    int s = 0, bad = 0;
    for (int q = 0; q < KP_ROW / 4; ++q) {
        int w = real ? row[q] : 0;
        if (w & 0x80808080) bad = MVSDF_PS_ERR_CODE;
        w &= 0x7f7f7f7f;
        const int c0 = w & 255, c1 = (w >> 8) & 255, c2 = (w >> 16) & 255, c3 = (w >> 24) & 255;
        s += (c0 * c0 + c1 * c1) + (c2 * c2 + c3 * c3);
        packed[p * (KP_ROW / 4) + q] = w;
    }
    norm[p] = real ? -s : KP_PAD_NORM;
    if (bad) atomicOr((kp_u64*)err, (kp_u64)bad);
}

// slot (source i, split y) of job z: key = D1 << 32 | j1 and second = D2 over the targets of the split (j1 within the target view; no target or no
// second: a distance above MVSDF_KP_MAX_DIST).  The slots start as all ones.
static __global__ __launch_bounds__(KP_WAVES * 64) void k_kp_match(const kp_v4i* __restrict__ P, const int* __restrict__ nrm,
                                                                   const KpJob* __restrict__ jobs, int splits, long long tiles_per_split,
                                                                   kp_u64* __restrict__ keys, unsigned* __restrict__ seconds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, grp = lane >> 4;
    const KpJob job = jobs[blockIdx.z];
    const long long i0 = ((long long)blockIdx.x * KP_WAVES + wave) * 16;
    if (i0 >= job.ns) return;                                     // (the whole wave; the rows up to the next multiple of 16 exist as zero rows)
    const long long tiles = (job.nt + 15) / 16;
    const long long tile0 = (long long)blockIdx.y * tiles_per_split;
    const long long tile1 = min(tiles, tile0 + tiles_per_split);
    if (tile0 >= tile1) return;
    const long long srow = job.s0 + i0 + col;
    const kp_v4i zero = {0, 0, 0, 0};
    const kp_v4i b0 = P[srow * 8 + grp], b1 = P[srow * 8 + 4 + grp];
    const int mine = -nrm[srow];                                  // |s|^2
    const kp_v4i* __restrict__ T = P + job.t0 * 8;
    const int* __restrict__ tn = nrm + job.t0;
    // the smallest D is the largest e = 2 s.t - |t|^2.  A padding row has e = KP_PAD_NORM exactly, which the strict > never takes.
    int be = KP_PAD_NORM, se = KP_PAD_NORM, bj = INT_MAX;
    auto visit = [&](long long base, const kp_v4i& a0, const kp_v4i& a1, const kp_v4i& neg) {
        kp_v4i acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b0, zero, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b1, acc, 0, 0, 0);
        const int e[4] = {2 * acc[0] + neg[0], 2 * acc[1] + neg[1], 2 * acc[2] + neg[2], 2 * acc[3] + neg[3]};
        if (max(max(e[0], e[1]), max(e[2], e[3])) > se) {         // most tiles change nothing
#pragma unroll
            for (int r = 0; r < 4; ++r) {                         // ascending rows, strict: the first of equal distances stays the best
                if (e[r] > be) {
                    se = be;
                    be = e[r];
                    bj = (int)base + 4 * grp + r;
                } else if (e[r] > se) {
                    se = e[r];
                }
            }
        }
    };
    long long tile = tile0;
    for (; tile + KP_UNROLL <= tile1; tile += KP_UNROLL) {        // the loads of KP_UNROLL tiles in flight before the first product
        kp_v4i a0[KP_UNROLL], a1[KP_UNROLL], neg[KP_UNROLL];
#pragma unroll
        for (int u = 0; u < KP_UNROLL; ++u) {
            const long long base = (tile + u) * 16;
            a0[u] = T[(base + col) * 8 + grp];
            a1[u] = T[(base + col) * 8 + 4 + grp];
            neg[u] = *(const kp_v4i*)(tn + base + 4 * grp);
        }
#pragma unroll
        for (int u = 0; u < KP_UNROLL; ++u) visit((tile + u) * 16, a0[u], a1[u], neg[u]);
    }
    for (; tile < tile1; ++tile) {
        const long long base = tile * 16;
        visit(base, T[(base + col) * 8 + grp], T[(base + col) * 8 + 4 + grp], *(const kp_v4i*)(tn + base + 4 * grp));
    }
    kp_u64 key = (kp_u64)(unsigned)(mine - be) << 32 | (unsigned)bj;
    unsigned sec = (unsigned)(mine - se);
#pragma unroll
    for (int d = 16; d <= 32; d <<= 1) {                          // the second of a union: the smallest of the losing best and the two seconds
        const kp_u64 ok = __shfl_xor(key, d);
        const unsigned os = __shfl_xor(sec, d);
        const unsigned lose = (unsigned)((ok < key ? key : ok) >> 32);
        key = ok < key ? ok : key;
        sec = min(min(sec, os), lose);
    }
    if (grp == 0 && i0 + col < job.ns) {
        const long long at = job.slot + (i0 + col) * splits + blockIdx.y;
        keys[at] = key;
        seconds[at] = sec;
    }
}

// the splits of one source merged: key, and through *second the second distance
__device__ __forceinline__ kp_u64 kp_merge(const kp_u64* __restrict__ keys, const unsigned* __restrict__ seconds, long long at, int splits, unsigned* second) {
    kp_u64 key = keys[at];
    unsigned sec = seconds[at];
    for (int y = 1; y < splits; ++y) {
        const kp_u64 ok = keys[at + y];
        const unsigned lose = (unsigned)((ok < key ? key : ok) >> 32);
        key = ok < key ? ok : key;
        sec = min(min(sec, seconds[at + y]), lose);
    }
    *second = sec;
    return key;
}

// element e = source i of pair m (elem_off): its candidate (i, j1), D1 and whether it is kept
static __global__ __launch_bounds__(CH_THREADS) void k_kp_match_final(const KpJob* __restrict__ jobs, const long long* __restrict__ elem_off, long long M,
                                                                      long long E, int splits, const kp_u64* __restrict__ keys,
                                                                      const unsigned* __restrict__ seconds, double ratio2, int max_dist, int mutual,
                                                                      unsigned char* __restrict__ flag, int* __restrict__ cidx, int* __restrict__ cdist) {
    const long long e = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (e >= E) return;
    const long long m = kp_find(elem_off, M, e);
    const long long i = e - elem_off[m];
    const KpJob fwd = jobs[2 * m], back = jobs[2 * m + 1];
    bool keep = false;
    long long j = 0;
    unsigned d1 = 0;
    if (fwd.nt > 0) {
        unsigned d2;
        const kp_u64 key = kp_merge(keys, seconds, fwd.slot + i * splits, splits, &d2);
        j = (long long)(unsigned)key;
        d1 = (unsigned)(key >> 32);
        keep = j < fwd.nt && d1 <= (unsigned)MVSDF_KP_MAX_DIST;   // (always: every source meets every target)
        if (keep && d2 <= (unsigned)MVSDF_KP_MAX_DIST) keep = (double)d1 < ratio2 * (double)d2;
        if (keep) keep = d1 <= (unsigned)max_dist;
        if (keep && mutual) {
            unsigned unused;
            keep = (long long)(unsigned)kp_merge(keys, seconds, back.slot + j * splits, splits, &unused) == i;
        }
    }
    flag[e] = keep ? 1 : 0;
    cidx[2 * e] = (int)i;
    cidx[2 * e + 1] = keep ? (int)j : -1;
    cdist[e] = (int)d1;
}

// ================================================================ compaction (the matcher's and the verifier's) ================================================================
static __global__ __launch_bounds__(CH_THREADS) void k_kp_emit(const unsigned char* __restrict__ flag, const long long* __restrict__ rank, long long E,
                                                               const int* __restrict__ cidx, const int* __restrict__ cdist, int* __restrict__ idx,
                                                               int* __restrict__ dist) {
    const long long e = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (e >= E || !flag[e]) return;
    const long long r = rank[e];
    idx[2 * r] = cidx[2 * e];
    idx[2 * r + 1] = cidx[2 * e + 1];
    dist[r] = cdist[e];
}

// off[m] = the rows kept before the first element of pair m
static __global__ __launch_bounds__(CH_THREADS) void k_kp_offsets(const long long* __restrict__ elem_off, long long M, long long E,
                                                                  const long long* __restrict__ rank, const long long* __restrict__ total,
                                                                  long long* __restrict__ off) {
    const long long m = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (m > M) return;
    const long long at = elem_off[m];
    off[m] = at >= 0 && at < E ? rank[at] : (at <= 0 ? 0 : *total);
}

struct KpCompact {
    size_t flag, rank, cidx, cdist, tmp;
};

static void kp_compact_layout(long long E, WsCursor& c, KpCompact* L) {
    L->flag = c.take((size_t)E);
    L->rank = c.take((size_t)E * 8);
    L->cidx = c.take((size_t)E * 8);
    L->cdist = c.take((size_t)E * 4);
    L->tmp = c.take(mv_scan_tmp_bytes(E));
}

// flags and candidates -> (off, idx, dist); the number kept -> hdr[MVSDF_RES_H_COUNT]
static void kp_compact(char* w, const KpCompact& L, const long long* elem_off, long long M, long long E, long long* off, int* idx, int* dist, hipStream_t s) {
    long long* hdr = (long long*)w;
    mv_scan((const unsigned char*)(w + L.flag), E, (long long*)(w + L.rank), w + L.tmp, hdr + MVSDF_RES_H_COUNT, s);
    hipLaunchKernelGGL(k_kp_emit, dim3(mv_grid(E, CH_THREADS)), dim3(CH_THREADS), 0, s, (const unsigned char*)(w + L.flag), (const long long*)(w + L.rank), E,
                       (const int*)(w + L.cidx), (const int*)(w + L.cdist), idx, dist);
    hipLaunchKernelGGL(k_kp_offsets, dim3(mv_grid(M + 1, CH_THREADS)), dim3(CH_THREADS), 0, s, elem_off, M, E, (const long long*)(w + L.rank),
                       (const long long*)(hdr + MVSDF_RES_H_COUNT), off);
}

// ---- the matcher's tables and workspace (host) ----
static inline long long kp_pad16(long long n) { return (n + 15) / 16 * 16; }

struct KpMatchLayout {
    long long npad, E, slots, tiles_per_split, gx;
    int splits;
    size_t view_off, pad_off, elem_off, jobs, tables_end, packed, norm, keys, seconds, total;
    KpCompact c;
};

// validates the host arrays and sizes everything; tables (optional) receives view_off [V+1], pad_off [V+1], elem_off [M+1] and the 2 M jobs, as they lie
// in the workspace from L->view_off on
static bool kp_match_layout(const int64_t* view_off, long long V, const int32_t* pairs, long long M, KpMatchLayout* L, std::vector<long long>* tables) {
    if (!view_off || !pairs || V < 1 || V > MVSDF_VS_MAX_VIEWS || M < 1 || M > MVSDF_KP_MAX_PAIRS || view_off[0] != 0) return false;
    for (long long v = 0; v < V; ++v) {
        const long long n = view_off[v + 1] - view_off[v];
        if (n < 0 || n > MVSDF_KP_MAX_KEYPOINTS) return false;
    }
    if (view_off[V] > INT_MAX) return false;
    std::vector<long long> pad(V + 1, 0), elem(M + 1, 0);
    for (long long v = 0; v < V; ++v) pad[v + 1] = pad[v] + kp_pad16(view_off[v + 1] - view_off[v]);
    long long blocks = 0, max_tiles = 0, gx = 0;
    for (long long m = 0; m < M; ++m) {
        const long long a = pairs[2 * m], b = pairs[2 * m + 1];
        if (a < 0 || b <= a || b >= V) return false;
        const long long na = view_off[a + 1] - view_off[a], nb = view_off[b + 1] - view_off[b];
        elem[m + 1] = elem[m] + na;
        if (na > 0 && nb > 0) {
            const long long ba = mv_ceil_div(na, KP_WAVES * 16), bb = mv_ceil_div(nb, KP_WAVES * 16);
            blocks += ba + bb;
            gx = ba > gx ? ba : gx;
            gx = bb > gx ? bb : gx;
            const long long t = mv_ceil_div(na > nb ? na : nb, 16);
            max_tiles = t > max_tiles ? t : max_tiles;
        }
    }
    if (elem[M] > INT_MAX) return false;
    long long want = blocks > 0 ? KP_TARGET_BLOCKS / blocks : 1;
    const long long most = mv_ceil_div(max_tiles, KP_MIN_TILES);
    if (want > most) want = most;
    if (want < 1) want = 1;
    L->tiles_per_split = max_tiles > 0 ? mv_ceil_div(max_tiles, want) : 1;
    L->splits = max_tiles > 0 ? (int)mv_ceil_div(max_tiles, L->tiles_per_split) : 1;
    L->gx = gx;
    L->npad = pad[V];
    L->E = elem[M];
    std::vector<long long> jobs((size_t)M * 10);
    long long slot = 0;
    for (long long m = 0; m < M; ++m)
        for (int d = 0; d < 2; ++d) {
            const long long sv = pairs[2 * m + d], tv = pairs[2 * m + 1 - d];
            const long long ns = view_off[sv + 1] - view_off[sv], nt = view_off[tv + 1] - view_off[tv];
            long long* j = jobs.data() + (2 * m + d) * 5;
            j[0] = pad[sv];
            j[1] = ns;
            j[2] = pad[tv];
            j[3] = nt;
            j[4] = slot;
            slot += nt > 0 ? ns * L->splits : 0;
        }
    L->slots = slot;
    static_assert(sizeof(KpJob) == 40, "a job is five int64 words");
    WsCursor c{CH_HDR};
    L->view_off = c.o;
    L->pad_off = L->view_off + (size_t)(V + 1) * 8;
    L->elem_off = L->pad_off + (size_t)(V + 1) * 8;
    L->jobs = L->elem_off + (size_t)(M + 1) * 8;
    L->tables_end = L->jobs + (size_t)M * 80;
    c.take(L->tables_end - L->view_off);
    L->packed = c.take((size_t)(L->npad + 16) * KP_ROW);          // (+ 16: never read, keeps an empty region addressable)
    L->norm = c.take((size_t)(L->npad + 16) * 4);
    L->keys = c.take((size_t)(L->slots + 1) * 8);
    L->seconds = c.take((size_t)(L->slots + 1) * 4);
    kp_compact_layout(L->E > 0 ? L->E : 1, c, &L->c);
    L->total = c.o;
    if (tables) {
        tables->clear();
        tables->insert(tables->end(), view_off, view_off + V + 1);
        tables->insert(tables->end(), pad.begin(), pad.end());
        tables->insert(tables->end(), elem.begin(), elem.end());
        tables->insert(tables->end(), jobs.begin(), jobs.end());
    }
    return true;
}

// ================================================================ verification ================================================================
__device__ __forceinline__ bool kp_line_ok(double l0, double l1, double l2, double X, double Y, double limit) {
    if (l0 == 0.0 && l1 == 0.0) return false;
    return fabs((l0 * X + l1 * Y) + l2) / sqrt(l0 * l0 + l1 * l1) <= limit;
}

static __global__ __launch_bounds__(CH_THREADS) void k_kp_verify(const double* __restrict__ xy, const long long* __restrict__ view_off, long long V,
                                                                 const int* __restrict__ pairs, long long M, const long long* __restrict__ off,
                                                                 const int* __restrict__ idx, const int* __restrict__ dist, long long E,
                                                                 const double* __restrict__ Fs, double limit, unsigned char* __restrict__ flag,
                                                                 int* __restrict__ cidx, int* __restrict__ cdist, long long* err) {
    const long long e = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (e >= E) return;
    cidx[2 * e] = idx[2 * e];
    cidx[2 * e + 1] = idx[2 * e + 1];
    cdist[e] = dist[e];
    flag[e] = 0;
    if (!(off[0] <= e && e < off[M])) {                           // (offsets that do not cover the matches)
        atomicOr((kp_u64*)err, (kp_u64)MVSDF_PS_ERR_INDEX);
        return;
    }
    const long long m = kp_find(off, M, e);
    const long long a = pairs[2 * m], b = pairs[2 * m + 1];
    if (a < 0 || a >= V || b < 0 || b >= V) {
        atomicOr((kp_u64*)err, (kp_u64)MVSDF_PS_ERR_PAIR);
        return;
    }
    const long long ia = idx[2 * e], ib = idx[2 * e + 1];
    if (ia < 0 || ia >= view_off[a + 1] - view_off[a] || ib < 0 || ib >= view_off[b + 1] - view_off[b]) {
        atomicOr((kp_u64*)err, (kp_u64)MVSDF_PS_ERR_INDEX);
        return;
    }
    const double* F = Fs + m * 9;
    const double Xa = xy[2 * (view_off[a] + ia)], Ya = xy[2 * (view_off[a] + ia) + 1];
    const double Xb = xy[2 * (view_off[b] + ib)], Yb = xy[2 * (view_off[b] + ib) + 1];
    bool fin = isfinite(Xa) && isfinite(Ya) && isfinite(Xb) && isfinite(Yb);
    for (int q = 0; q < 9; ++q) fin = fin && isfinite(F[q]);
    if (!fin) {
        atomicOr((kp_u64*)err, (kp_u64)MVSDF_PS_ERR_FINITE);
        return;
    }
    const bool in_b = kp_line_ok((F[0] * Xa + F[1] * Ya) + F[2], (F[3] * Xa + F[4] * Ya) + F[5], (F[6] * Xa + F[7] * Ya) + F[8], Xb, Yb, limit);
    const bool in_a = kp_line_ok((F[0] * Xb + F[3] * Yb) + F[6], (F[1] * Xb + F[4] * Yb) + F[7], (F[2] * Xb + F[5] * Yb) + F[8], Xa, Ya, limit);
    flag[e] = in_b && in_a ? 1 : 0;
}

// ================================================================ tracks ================================================================
// the two nodes of every match (-1, -1 and an error bit where an index is out of range); label[n] = n
static __global__ __launch_bounds__(CH_THREADS) void k_kp_edges(const long long* __restrict__ view_off, long long V, const int* __restrict__ pairs, long long M,
                                                                const long long* __restrict__ off, const int* __restrict__ idx, long long E,
                                                                int* __restrict__ eu, int* __restrict__ ev, long long* err) {
    const long long e = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (e >= E) return;
    eu[e] = -1;
    ev[e] = -1;
    if (!(off[0] <= e && e < off[M])) {
        atomicOr((kp_u64*)err, (kp_u64)MVSDF_PS_ERR_INDEX);
        return;
    }
    const long long m = kp_find(off, M, e);
    const long long a = pairs[2 * m], b = pairs[2 * m + 1];
    if (a < 0 || a >= V || b < 0 || b >= V) {
        atomicOr((kp_u64*)err, (kp_u64)MVSDF_PS_ERR_PAIR);
        return;
    }
    const long long ia = idx[2 * e], ib = idx[2 * e + 1];
    if (ia < 0 || ia >= view_off[a + 1] - view_off[a] || ib < 0 || ib >= view_off[b + 1] - view_off[b]) {
        atomicOr((kp_u64*)err, (kp_u64)MVSDF_PS_ERR_INDEX);
        return;
    }
    eu[e] = (int)(view_off[a] + ia);
    ev[e] = (int)(view_off[b] + ib);
}

static __global__ __launch_bounds__(CH_THREADS) void k_kp_label_init(int* __restrict__ label, long long N) {
    const long long n = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (n < N) label[n] = (int)n;
}

// one round: the smaller label of an edge's ends goes to the other end.  label[] is read with plain loads while other lanes run atomicMin on it, and
// `changed` is a plain store of the same value by every lane that saw a difference.  Both are safe for the result: a label only ever decreases and is
// always a node of its own component, so a stale read can only delay a hand-over to a later round, never invent one; and a launch in which some edge
// still had two different labels at the time a lane read them sets the flag, so the host loop ends only after a round that saw every edge equal --
// the fixed point, in which each node carries the smallest node of its component whatever the schedule was.
static __global__ __launch_bounds__(CH_THREADS) void k_kp_round(const int* __restrict__ eu, const int* __restrict__ ev, long long E, int* label, int* changed) {
    const long long e = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (e >= E) return;
    const int u = eu[e], v = ev[e];
    if (u < 0) return;
    const int lu = label[u], lv = label[v];
    if (lu < lv) {
        atomicMin(label + v, lu);
        *changed = 1;
    } else if (lv < lu) {
        atomicMin(label + u, lv);
        *changed = 1;
    }
}

// label[n] follows the labels of its label downwards (labels are nodes of the same component and never exceed their node)
static __global__ __launch_bounds__(CH_THREADS) void k_kp_jump(int* label, long long N) {
    const long long n = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (n >= N) return;
    const int first = label[n];
    int l = first;
    for (int it = 0; it < KP_JUMPS; ++it) {
        const int ll = label[l];
        if (ll >= l) break;
        l = ll;
    }
    if (l < first) atomicMin(label + n, l);
}

static __global__ __launch_bounds__(CH_THREADS) void k_kp_sort_keys(const int* __restrict__ label, long long N, kp_u64* __restrict__ key, int* __restrict__ val) {
    const long long n = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (n >= N) return;
    key[n] = (kp_u64)(unsigned)label[n];
    val[n] = (int)n;
}

// over the nodes sorted by (label, node): the size of every component, and whether two neighbours in it share a view (the nodes of a view are one
// interval, so two nodes of one view in a component are neighbours in this order, or enclose a third of that view)
static __global__ __launch_bounds__(CH_THREADS) void k_kp_segments(const kp_u64* __restrict__ key, const int* __restrict__ val, long long N,
                                                                   const long long* __restrict__ view_off, long long V, int* cnt, int* bad) {
    const long long p = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (p >= N) return;
    const kp_u64 k = key[p];
    atomicAdd(cnt + k, 1);
    if (p > 0 && key[p - 1] == k && kp_find(view_off, V, val[p - 1]) == kp_find(view_off, V, val[p])) atomicOr(bad + k, 1);
}

static __global__ __launch_bounds__(CH_THREADS) void k_kp_track_flags(const kp_u64* __restrict__ key, long long N, const int* __restrict__ cnt,
                                                                      const int* __restrict__ bad, unsigned char* __restrict__ fe,
                                                                      unsigned char* __restrict__ fh) {
    const long long p = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (p >= N) return;
    const kp_u64 k = key[p];
    const bool in = cnt[k] >= 2 && !bad[k];
    fe[p] = in ? 1 : 0;
    fh[p] = in && (p == 0 || key[p - 1] != k) ? 1 : 0;
}

static __global__ __launch_bounds__(CH_THREADS) void k_kp_track_emit(const int* __restrict__ val, long long N, const unsigned char* __restrict__ fe,
                                                                     const unsigned char* __restrict__ fh, const long long* __restrict__ re,
                                                                     const long long* __restrict__ rh, const long long* __restrict__ view_off, long long V,
                                                                     const long long* __restrict__ hdr, long long* __restrict__ track_off,
                                                                     int* __restrict__ track_view, int* __restrict__ track_kp) {
    const long long p = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (p >= N) return;
    if (p == 0) track_off[hdr[MVSDF_KP_TRACKS_H_TRACKS]] = hdr[MVSDF_KP_TRACKS_H_ENTRIES];
    if (!fe[p]) return;
    const long long node = val[p], v = kp_find(view_off, V, node);
    track_view[re[p]] = (int)v;
    track_kp[re[p]] = (int)(node - view_off[v]);
    if (fh[p]) track_off[rh[p]] = re[p];
}

enum { KP_H_CHANGED = 8 };                                        // the private header word of the labelling rounds
static_assert(KP_H_CHANGED >= MVSDF_KP_TRACKS_H_WORDS && (KP_H_CHANGED + 1) * 8 <= CH_HDR, "the private word lies behind the public ones, inside the header");

struct KpTracksLayout {
    size_t eu, ev, label, k0, k1, v0, v1, cnt, bad, fe, fh, re, rh, tmp, total;
    ChSortLayout rs;
};

static bool kp_tracks_layout(long long N, long long E, KpTracksLayout* L) {
    if (N < 1 || N > INT_MAX || E < 1 || E > INT_MAX) return false;
    WsCursor c{CH_HDR};
    L->eu = c.take((size_t)E * 4);
    L->ev = c.take((size_t)E * 4);
    L->label = c.take((size_t)N * 4);
    L->k0 = c.take((size_t)N * 8);
    L->k1 = c.take((size_t)N * 8);
    L->v0 = c.take((size_t)N * 4);
    L->v1 = c.take((size_t)N * 4);
    ch_sort_layout(N, 0, c, &L->rs);
    L->cnt = c.take((size_t)N * 4);
    L->bad = c.take((size_t)N * 4);
    L->fe = c.take((size_t)N);
    L->fh = c.take((size_t)N);
    L->re = c.take((size_t)N * 8);
    L->rh = c.take((size_t)N * 8);
    L->tmp = c.take(mv_scan_tmp_bytes(N));
    L->total = c.o;
    return true;
}

// ================================================================ triangulation ================================================================
// the unit ray of pixel (X, Y) through rays = R^T K^-1 (row-major)
__device__ __forceinline__ void kp_ray(const double* __restrict__ Mr, double X, double Y, double* r) {
    const double d0 = (Mr[0] * X + Mr[1] * Y) + Mr[2], d1 = (Mr[3] * X + Mr[4] * Y) + Mr[5], d2 = (Mr[6] * X + Mr[7] * Y) + Mr[8];
    const double n = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
    r[0] = d0 / n;
    r[1] = d1 / n;
    r[2] = d2 / n;
}

struct KpObs {
    const double* __restrict__ xy;
    const long long* __restrict__ view_off;
    const int* __restrict__ tv;
    const int* __restrict__ tk;
    const double* __restrict__ centers;
    const double* __restrict__ rays;
    const double* __restrict__ proj;
    __device__ __forceinline__ void pixel(long long q, int* v, double* X, double* Y) const {
        *v = tv[q];
        const long long g = view_off[*v] + tk[q];
        *X = xy[2 * g];
        *Y = xy[2 * g + 1];
    }
};

// the point nearest to the rays of the entries [q0, q1) whose mask byte is set (mask == NULL: all) -> false when the determinant is not > 0
__device__ __forceinline__ bool kp_fit(const KpObs& o, long long q0, long long q1, const unsigned char* mask, double* P) {
    double A[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
    for (long long q = q0; q < q1; ++q) {
        if (mask && !mask[q]) continue;
        int v;
        double X, Y, r[3];
        o.pixel(q, &v, &X, &Y);
        kp_ray(o.rays + 9 * (long long)v, X, Y, r);
        const double* c = o.centers + 3 * (long long)v;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double a[3];
#pragma unroll
            for (int l = 0; l < 3; ++l) {
                a[l] = (k == l ? 1.0 : 0.0) - r[k] * r[l];
                A[3 * k + l] = A[3 * k + l] + a[l];
            }
            b[k] = b[k] + ((a[0] * c[0] + a[1] * c[1]) + a[2] * c[2]);
        }
    }
    const double det = kp_det3(A[0], A[1], A[2], A[3], A[4], A[5], A[6], A[7], A[8]);
    if (!(det > 0.0)) return false;
    P[0] = kp_det3(b[0], A[1], A[2], b[1], A[4], A[5], b[2], A[7], A[8]) / det;
    P[1] = kp_det3(A[0], b[0], A[2], A[3], b[1], A[5], A[6], b[2], A[8]) / det;
    P[2] = kp_det3(A[0], A[1], b[0], A[3], A[4], b[1], A[6], A[7], b[2]) / det;
    return true;
}

// the reprojection error of entry q at P; false when the depth is not positive or the error exceeds the limit (or is not a number)
__device__ __forceinline__ bool kp_reproject(const KpObs& o, long long q, const double* P, double limit, double* error) {
    int v;
    double X, Y;
    o.pixel(q, &v, &X, &Y);
    const double* Pm = o.proj + 12 * (long long)v;
    const double z = mv_row4(Pm + 8, P[0], P[1], P[2], 1.0);
    if (!(z > 0.0)) return false;
    const double du = mv_row4(Pm, P[0], P[1], P[2], 1.0) / z - X, dv = mv_row4(Pm + 4, P[0], P[1], P[2], 1.0) / z - Y;
    *error = sqrt(du * du + dv * dv);
    return *error <= limit;
}

static __global__ __launch_bounds__(CH_THREADS) void k_kp_triangulate(KpObs o, long long V, const long long* __restrict__ track_off, long long T, long long nnz,
                                                                      double max_reproj, double cos_min, double* __restrict__ xyz,
                                                                      double* __restrict__ error, unsigned char* __restrict__ keep,
                                                                      unsigned char* __restrict__ obs_keep, long long* err) {
    const long long t = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
    if (t >= T) return;
    xyz[3 * t] = xyz[3 * t + 1] = xyz[3 * t + 2] = 0.0;
    error[t] = 0.0;
    keep[t] = 0;
    const long long q0 = track_off[t], q1 = track_off[t + 1];
    if (q0 < 0 || q1 < q0 || q1 > nnz || q1 - q0 > V) {           // (a track holds at most one entry per view: the loops below are bounded by V)
        atomicOr((kp_u64*)err, (kp_u64)MVSDF_PS_ERR_INDEX);
        return;
    }
    int bad = 0;
    for (long long q = q0; q < q1; ++q) {
        obs_keep[q] = 0;
        const long long v = o.tv[q];
        if (v < 0 || v >= V)
            bad |= MVSDF_PS_ERR_PAIR;
        else if (o.tk[q] < 0 || o.tk[q] >= o.view_off[v + 1] - o.view_off[v])
            bad |= MVSDF_PS_ERR_INDEX;
        else {
            const long long g = o.view_off[v] + o.tk[q];
            if (!isfinite(o.xy[2 * g]) || !isfinite(o.xy[2 * g + 1])) bad |= MVSDF_PS_ERR_FINITE;
        }
    }
    if (bad) {
        atomicOr((kp_u64*)err, (kp_u64)bad);
        return;
    }
    if (q1 - q0 < 2) return;
    double P[3], e;
    if (!kp_fit(o, q0, q1, nullptr, P)) return;
    long long ok = 0;
    for (long long q = q0; q < q1; ++q) {
        const bool in = kp_reproject(o, q, P, max_reproj, &e);
        obs_keep[q] = in ? 1 : 0;
        ok += in ? 1 : 0;
    }
    bool good = ok >= 2;
    if (good && ok < q1 - q0) {                                   // the one refit
        good = kp_fit(o, q0, q1, obs_keep, P);
        for (long long q = q0; good && q < q1; ++q)
            if (obs_keep[q] && !kp_reproject(o, q, P, max_reproj, &e)) good = false;
    }
    if (good) {                                                   // the largest angle between two remaining rays
        bool wide = false;
        for (long long qi = q0; qi < q1; ++qi) {
            if (!obs_keep[qi]) continue;
            int v;
            double X, Y, ri[3], rj[3];
            o.pixel(qi, &v, &X, &Y);
            kp_ray(o.rays + 9 * (long long)v, X, Y, ri);
            for (long long qj = qi + 1; qj < q1; ++qj) {
                if (!obs_keep[qj]) continue;
                o.pixel(qj, &v, &X, &Y);
                kp_ray(o.rays + 9 * (long long)v, X, Y, rj);
                if ((ri[0] * rj[0] + ri[1] * rj[1]) + ri[2] * rj[2] <= cos_min) wide = true;
            }
        }
        good = wide;
    }
    if (!good) {
        for (long long q = q0; q < q1; ++q) obs_keep[q] = 0;
        return;
    }
    double sum = 0.0, cnt = 0.0;
    for (long long q = q0; q < q1; ++q)
        if (obs_keep[q]) {
            kp_reproject(o, q, P, max_reproj, &e);
            sum = sum + e;
            cnt = cnt + 1.0;
        }
    xyz[3 * t] = P[0];
    xyz[3 * t + 1] = P[1];
    xyz[3 * t + 2] = P[2];
    error[t] = sum / cnt;
    keep[t] = 1;
}

extern "C" {

static bool kp_planes_ok(long long planes, long long h, long long w) {
    return planes >= 1 && h >= 1 && w >= 1 && h <= INT_MAX && w <= INT_MAX && planes <= INT_MAX && (double)planes * (double)h * (double)w <= 1099511627776.0;
}

int mvsdf_kp_grey(const void* images, int32_t is_float, int32_t channels, int64_t n, double* out, void* stream) {
    if (!images || !out || n < 1 || n > (1ll << 40) || (channels != 1 && channels != 3)) return mv_fail(-1, "mvsdf_kp_grey: bad arguments");
    if (is_float)
        hipLaunchKernelGGL(k_kp_grey<float>, dim3(mv_grid(n, CH_THREADS)), dim3(CH_THREADS), 0, (hipStream_t)stream, (const float*)images, (int)channels,
                           (long long)n, out);
    else
        hipLaunchKernelGGL(k_kp_grey<unsigned char>, dim3(mv_grid(n, CH_THREADS)), dim3(CH_THREADS), 0, (hipStream_t)stream, (const unsigned char*)images,
                           (int)channels, (long long)n, out);
    return mv_check(hipGetLastError(), "mvsdf_kp_grey");
}

int mvsdf_kp_blur(const double* src, int64_t planes, int64_t h, int64_t w, const double* taps, int32_t radius, double* tmp, double* dst, void* stream) {
    if (!src || !taps || !tmp || !dst || tmp == src || tmp == dst || !kp_planes_ok(planes, h, w) || radius < 0 || radius > MVSDF_KP_MAX_RADIUS)
        return mv_fail(-1, "mvsdf_kp_blur: bad arguments");
    const long long n = (long long)planes * h * w;
    hipLaunchKernelGGL(k_kp_blur<true>, dim3(mv_grid(n, CH_THREADS)), dim3(CH_THREADS), 0, (hipStream_t)stream, src, (long long)planes, (long long)h, (long long)w,
                       taps, (int)radius, tmp);
    hipLaunchKernelGGL(k_kp_blur<false>, dim3(mv_grid(n, CH_THREADS)), dim3(CH_THREADS), 0, (hipStream_t)stream, (const double*)tmp, (long long)planes, (long long)h,
                       (long long)w, taps, (int)radius, dst);
    return mv_check(hipGetLastError(), "mvsdf_kp_blur");
}

int mvsdf_kp_half(const double* src, int64_t planes, int64_t h, int64_t w, double* dst, void* stream) {
    if (!src || !dst || !kp_planes_ok(planes, h, w)) return mv_fail(-1, "mvsdf_kp_half: bad arguments");
    const long long n = (long long)planes * ((h + 1) / 2) * ((w + 1) / 2);
    hipLaunchKernelGGL(k_kp_half, dim3(mv_grid(n, CH_THREADS)), dim3(CH_THREADS), 0, (hipStream_t)stream, src, (long long)planes, (long long)h, (long long)w, dst);
    return mv_check(hipGetLastError(), "mvsdf_kp_half");
}

int mvsdf_kp_dog(const double* L, int64_t planes, int64_t levels, int64_t hw, double* D, void* stream) {
    if (!L || !D || levels < 2 || levels > 64 || !kp_planes_ok(planes, levels, hw)) return mv_fail(-1, "mvsdf_kp_dog: bad arguments");
    const long long n = (long long)planes * (levels - 1) * hw;
    hipLaunchKernelGGL(k_kp_dog, dim3(mv_grid(n, CH_THREADS)), dim3(CH_THREADS), 0, (hipStream_t)stream, L, (long long)planes, (long long)levels, (long long)hw, D);
    return mv_check(hipGetLastError(), "mvsdf_kp_dog");
}

int mvsdf_kp_describe(const double* L, int64_t V, int64_t h, int64_t w, const int32_t* cand, int64_t n, int32_t upright, const double* cell,
                      const int32_t* radius, const double* ogauss, const int32_t* oradius, const double* trig, int64_t* acc, double* angle,
                      int8_t* codes, uint8_t* valid, void* stream) {
    if (!L || !cand || !cell || !radius || !ogauss || !oradius || !trig || !acc || !angle || !codes || !valid || !kp_planes_ok(V * 6, h, w) || n < 1 ||
        n > INT_MAX)
        return mv_fail(-1, "mvsdf_kp_describe: bad arguments");
    KpDescTables tab;
    for (int q = 0; q < 3; ++q) {
        if (!(cell[q] > 0) || radius[q] < 0 || radius[q] > 4 * MVSDF_KP_MAX_RADIUS || !(ogauss[q] >= 0) || oradius[q] < 0 || oradius[q] > 4 * MVSDF_KP_MAX_RADIUS)
            return mv_fail(-1, "mvsdf_kp_describe: bad arguments");
        tab.cell[q] = cell[q];
        tab.radius[q] = radius[q];
        tab.ogauss[q] = ogauss[q];
        tab.oradius[q] = oradius[q];
    }
    hipLaunchKernelGGL(k_kp_describe, dim3(mv_grid(n, CH_THREADS)), dim3(CH_THREADS), 0, (hipStream_t)stream, L, (long long)V, (long long)h, (long long)w,
                       (const int*)cand, (long long)n, (int)upright, tab, trig, (long long*)acc, angle, (signed char*)codes, (unsigned char*)valid);
    return mv_check(hipGetLastError(), "mvsdf_kp_describe");
}

struct KpExtremaLayout {
    long long n;
    size_t flag, rank, tmp, total;
};

static bool kp_extrema_layout(long long V, long long h, long long w, KpExtremaLayout* L) {
    if (!kp_planes_ok(V, h, w) || (double)V * 3.0 * (double)h * (double)w > (double)INT_MAX) return false;
    L->n = V * 3 * h * w;
    WsCursor c{CH_HDR};
    L->flag = c.take((size_t)L->n);
    L->rank = c.take((size_t)L->n * 8);
    L->tmp = c.take(mv_scan_tmp_bytes(L->n));
    L->total = c.o;
    return true;
}

size_t mvsdf_kp_extrema_workspace_bytes(int64_t V, int64_t h, int64_t w) {
    KpExtremaLayout L;
    return kp_extrema_layout(V, h, w, &L) ? L.total : 0;
}

int mvsdf_kp_extrema(const double* D, int64_t V, int64_t h, int64_t w, double contrast, double edge_ratio, int32_t border, double step,
                     const double* sigma, int64_t cap, void* ws, size_t ws_bytes, int32_t* cand, double* out, void* stream) {
    KpExtremaLayout L;
    if (!D || !sigma || !ws || !cand || !out || !kp_extrema_layout(V, h, w, &L) || !(contrast >= 0) || !(edge_ratio >= 1) || border < 1 || !(step > 0) || cap < 1)
        return mv_fail(-1, "mvsdf_kp_extrema: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_kp_extrema: workspace too small (mvsdf_kp_extrema_workspace_bytes)");
    char* w_ = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    long long* hdr = (long long*)w_;
    if (int rc = mv_check(hipMemsetAsync(w_, 0, CH_HDR, s), "mvsdf_kp_extrema")) return rc;
    hipLaunchKernelGGL(k_kp_extrema_flag, dim3(mv_grid(L.n, CH_THREADS)), dim3(CH_THREADS), 0, s, D, L.n, (long long)h, (long long)w, contrast, edge_ratio,
                       (int)border, (unsigned char*)(w_ + L.flag));
    mv_scan((const unsigned char*)(w_ + L.flag), L.n, (long long*)(w_ + L.rank), w_ + L.tmp, hdr + MVSDF_RES_H_COUNT, s);
    hipLaunchKernelGGL(k_kp_extrema_emit, dim3(mv_grid(L.n, CH_THREADS)), dim3(CH_THREADS), 0, s, D, L.n, (long long)h, (long long)w, contrast, edge_ratio,
                       (int)border, step, sigma[0], sigma[1], sigma[2], (const unsigned char*)(w_ + L.flag), (const long long*)(w_ + L.rank), (long long)cap,
                       (int*)cand, out, hdr + MVSDF_RES_H_ERR);
    return mv_check(hipGetLastError(), "mvsdf_kp_extrema");
}

size_t mvsdf_kp_match_workspace_bytes(const int64_t* view_off, int64_t V, const int32_t* pairs, int64_t M) {
    KpMatchLayout L;
    return kp_match_layout(view_off, V, pairs, M, &L, nullptr) ? L.total : 0;
}

int32_t mvsdf_kp_match_splits(const int64_t* view_off, int64_t V, const int32_t* pairs, int64_t M) {
    KpMatchLayout L;
    return kp_match_layout(view_off, V, pairs, M, &L, nullptr) ? L.splits : 0;
}

int mvsdf_kp_match(const int8_t* codes, const int64_t* view_off, int64_t V, const int32_t* pairs, int64_t M, double ratio2, int32_t max_dist,
                   int32_t mutual, void* ws, size_t ws_bytes, int64_t* off, int32_t* idx, int32_t* dist, void* stream) {
    KpMatchLayout L;
    std::vector<long long> tables;
    if (!ws || !off || !kp_match_layout(view_off, V, pairs, M, &L, &tables) || !(ratio2 >= 0) || max_dist < 0)
        return mv_fail(-1, "mvsdf_kp_match: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_kp_match: workspace too small (mvsdf_kp_match_workspace_bytes)");
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if ((rc = mv_check(hipMemsetAsync(w, 0, CH_HDR, s), "mvsdf_kp_match"))) return rc;
    if (L.E == 0) {                                               // no keypoint in any first view: M + 1 zeros
        if ((rc = mv_check(hipMemsetAsync(off, 0, (size_t)(M + 1) * 8, s), "mvsdf_kp_match"))) return rc;
        return mv_check(hipStreamSynchronize(s), "mvsdf_kp_match");
    }
    if (!codes || !idx || !dist) return mv_fail(-1, "mvsdf_kp_match: bad arguments");
    if ((rc = mv_check(hipMemcpyAsync(w + L.view_off, tables.data(), tables.size() * 8, hipMemcpyHostToDevice, s), "mvsdf_kp_match"))) return rc;
    if ((rc = mv_check(hipMemsetAsync(w + L.keys, 0xff, (size_t)(L.slots + 1) * 8, s), "mvsdf_kp_match"))) return rc;
    if ((rc = mv_check(hipMemsetAsync(w + L.seconds, 0xff, (size_t)(L.slots + 1) * 4, s), "mvsdf_kp_match"))) return rc;
    const KpJob* jobs = (const KpJob*)(w + L.jobs);
    const long long* elem_off = (const long long*)(w + L.elem_off);
    hipLaunchKernelGGL(k_kp_pack, dim3(mv_grid(L.npad, CH_THREADS)), dim3(CH_THREADS), 0, s, (const int*)codes, (const long long*)(w + L.view_off),
                       (const long long*)(w + L.pad_off), (long long)V, L.npad, (int*)(w + L.packed), (int*)(w + L.norm), (long long*)w + MVSDF_RES_H_ERR);
    if (L.gx > 0)
        hipLaunchKernelGGL(k_kp_match, dim3((unsigned)L.gx, (unsigned)L.splits, (unsigned)(2 * M)), dim3(KP_WAVES * 64), 0, s, (const kp_v4i*)(w + L.packed),
                           (const int*)(w + L.norm), jobs, L.splits, L.tiles_per_split, (kp_u64*)(w + L.keys), (unsigned*)(w + L.seconds));
    hipLaunchKernelGGL(k_kp_match_final, dim3(mv_grid(L.E, CH_THREADS)), dim3(CH_THREADS), 0, s, jobs, elem_off, (long long)M, L.E, L.splits,
                       (const kp_u64*)(w + L.keys), (const unsigned*)(w + L.seconds), ratio2, (int)max_dist, (int)mutual, (unsigned char*)(w + L.c.flag),
                       (int*)(w + L.c.cidx), (int*)(w + L.c.cdist));
    kp_compact(w, L.c, elem_off, (long long)M, L.E, (long long*)off, (int*)idx, (int*)dist, s);
    if ((rc = mv_check(hipGetLastError(), "mvsdf_kp_match"))) return rc;
    return mv_check(hipStreamSynchronize(s), "mvsdf_kp_match");  // (the tables leave the host's memory with this call)
}

size_t mvsdf_kp_verify_workspace_bytes(int64_t E) {
    if (E < 1 || E > INT_MAX) return 0;
    WsCursor c{CH_HDR};
    KpCompact L;
    kp_compact_layout(E, c, &L);
    return c.o;
}

int mvsdf_kp_verify(const double* xy, const int64_t* view_off, int64_t V, const int32_t* pairs, int64_t M, const int64_t* off, const int32_t* idx,
                    const int32_t* dist, int64_t E, const double* F, double max_epipolar, void* ws, size_t ws_bytes, int64_t* off_out,
                    int32_t* idx_out, int32_t* dist_out, void* stream) {
    if (!xy || !view_off || !pairs || !off || !idx || !dist || !F || !ws || !off_out || !idx_out || !dist_out || V < 1 || V > MVSDF_VS_MAX_VIEWS || M < 1 ||
        M > INT_MAX || E < 1 || E > INT_MAX || !(max_epipolar >= 0))
        return mv_fail(-1, "mvsdf_kp_verify: bad arguments");
    if (ws_bytes < mvsdf_kp_verify_workspace_bytes(E)) return mv_fail(-1, "mvsdf_kp_verify: workspace too small (mvsdf_kp_verify_workspace_bytes)");
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    WsCursor c{CH_HDR};
    KpCompact L;
    kp_compact_layout(E, c, &L);
    if (int rc = mv_check(hipMemsetAsync(w, 0, CH_HDR, s), "mvsdf_kp_verify")) return rc;
    hipLaunchKernelGGL(k_kp_verify, dim3(mv_grid(E, CH_THREADS)), dim3(CH_THREADS), 0, s, xy, (const long long*)view_off, (long long)V, (const int*)pairs,
                       (long long)M, (const long long*)off, (const int*)idx, (const int*)dist, (long long)E, F, max_epipolar, (unsigned char*)(w + L.flag),
                       (int*)(w + L.cidx), (int*)(w + L.cdist), (long long*)w + MVSDF_RES_H_ERR);
    kp_compact(w, L, (const long long*)off, (long long)M, (long long)E, (long long*)off_out, (int*)idx_out, (int*)dist_out, s);
    return mv_check(hipGetLastError(), "mvsdf_kp_verify");
}

size_t mvsdf_kp_tracks_workspace_bytes(int64_t N, int64_t E) {
    KpTracksLayout L;
    return kp_tracks_layout(N, E, &L) ? L.total : 0;
}

int mvsdf_kp_tracks(const int64_t* view_off, int64_t V, int64_t N, const int32_t* pairs, int64_t M, const int64_t* off, const int32_t* idx, int64_t E,
                    int32_t max_rounds, void* ws, size_t ws_bytes, int64_t* track_off, int32_t* track_view, int32_t* track_kp, void* stream) {
    KpTracksLayout L;
    if (!view_off || !pairs || !off || !idx || !ws || !track_off || !track_view || !track_kp || V < 1 || V > MVSDF_VS_MAX_VIEWS || M < 1 || M > INT_MAX ||
        max_rounds < 1 || !kp_tracks_layout(N, E, &L))
        return mv_fail(-1, "mvsdf_kp_tracks: bad arguments");
    if (ws_bytes < L.total) return mv_fail(-1, "mvsdf_kp_tracks: workspace too small (mvsdf_kp_tracks_workspace_bytes)");
    char* w = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    long long* hdr = (long long*)w;
    int* label = (int*)(w + L.label);
    const int* eu = (const int*)(w + L.eu);
    const int* ev = (const int*)(w + L.ev);
    const long long* vo = (const long long*)view_off;
    const unsigned gn = mv_grid(N, CH_THREADS), ge = mv_grid(E, CH_THREADS);
    int rc;
    if ((rc = mv_check(hipMemsetAsync(w, 0, CH_HDR, s), "mvsdf_kp_tracks"))) return rc;
    hipLaunchKernelGGL(k_kp_edges, dim3(ge), dim3(CH_THREADS), 0, s, vo, (long long)V, (const int*)pairs, (long long)M, (const long long*)off, (const int*)idx,
                       (long long)E, (int*)(w + L.eu), (int*)(w + L.ev), hdr + MVSDF_KP_TRACKS_H_ERR);
    hipLaunchKernelGGL(k_kp_label_init, dim3(gn), dim3(CH_THREADS), 0, s, label, (long long)N);
    long long rounds = 0, changed = 1;
    while (changed && rounds < max_rounds) {                      // bounded: max_rounds
        if ((rc = mv_check(hipMemsetAsync(hdr + KP_H_CHANGED, 0, 8, s), "mvsdf_kp_tracks"))) return rc;
        for (int q = 0; q < MVSDF_KP_ROUND_BATCH && rounds < max_rounds; ++q, ++rounds) {
            hipLaunchKernelGGL(k_kp_round, dim3(ge), dim3(CH_THREADS), 0, s, eu, ev, (long long)E, label, (int*)(hdr + KP_H_CHANGED));
            hipLaunchKernelGGL(k_kp_jump, dim3(gn), dim3(CH_THREADS), 0, s, label, (long long)N);
        }
        if ((rc = mv_read(&changed, hdr + KP_H_CHANGED, 8, s, "mvsdf_kp_tracks"))) return rc;
    }
    long long head[2] = {changed ? MVSDF_PS_ERR_ROUNDS : 0, rounds};
    if (changed) {                                                // the labels are not final: nothing else is valid
        long long e0 = 0;
        if ((rc = mv_read(&e0, hdr + MVSDF_KP_TRACKS_H_ERR, 8, s, "mvsdf_kp_tracks"))) return rc;
        head[0] |= e0;
        return mv_write_header(hdr + MVSDF_KP_TRACKS_H_ERR, head, 2, s, "mvsdf_kp_tracks");
    }
    if ((rc = mv_write_header(hdr + MVSDF_KP_TRACKS_H_ROUNDS, head + 1, 1, s, "mvsdf_kp_tracks"))) return rc;
    kp_u64* const k[2] = {(kp_u64*)(w + L.k0), (kp_u64*)(w + L.k1)};
    int* const v[2] = {(int*)(w + L.v0), (int*)(w + L.v1)};
    hipLaunchKernelGGL(k_kp_sort_keys, dim3(gn), dim3(CH_THREADS), 0, s, (const int*)label, (long long)N, k[0], v[0]);
    int bits = 1;
    while (bits < 32 && (1ll << bits) < N) ++bits;
    const int cur = ch_radix_sort(k, v, (long long)N, bits, w, L.rs, s);
    if ((rc = mv_check(hipMemsetAsync(w + L.cnt, 0, (size_t)N * 4, s), "mvsdf_kp_tracks"))) return rc;
    if ((rc = mv_check(hipMemsetAsync(w + L.bad, 0, (size_t)N * 4, s), "mvsdf_kp_tracks"))) return rc;
    hipLaunchKernelGGL(k_kp_segments, dim3(gn), dim3(CH_THREADS), 0, s, (const kp_u64*)k[cur], (const int*)v[cur], (long long)N, vo, (long long)V,
                       (int*)(w + L.cnt), (int*)(w + L.bad));
    hipLaunchKernelGGL(k_kp_track_flags, dim3(gn), dim3(CH_THREADS), 0, s, (const kp_u64*)k[cur], (long long)N, (const int*)(w + L.cnt), (const int*)(w + L.bad),
                       (unsigned char*)(w + L.fe), (unsigned char*)(w + L.fh));
    mv_scan((const unsigned char*)(w + L.fe), (long long)N, (long long*)(w + L.re), w + L.tmp, hdr + MVSDF_KP_TRACKS_H_ENTRIES, s);
    mv_scan((const unsigned char*)(w + L.fh), (long long)N, (long long*)(w + L.rh), w + L.tmp, hdr + MVSDF_KP_TRACKS_H_TRACKS, s);
    hipLaunchKernelGGL(k_kp_track_emit, dim3(gn), dim3(CH_THREADS), 0, s, (const int*)v[cur], (long long)N, (const unsigned char*)(w + L.fe),
                       (const unsigned char*)(w + L.fh), (const long long*)(w + L.re), (const long long*)(w + L.rh), vo, (long long)V, (const long long*)hdr,
                       (long long*)track_off, (int*)track_view, (int*)track_kp);
    return mv_check(hipGetLastError(), "mvsdf_kp_tracks");
}

int mvsdf_kp_triangulate(const double* xy, const int64_t* view_off, int64_t V, const int64_t* track_off, const int32_t* track_view,
                         const int32_t* track_kp, int64_t T, int64_t nnz, const double* centers, const double* rays, const double* proj,
                         double max_reproj, double cos_min_angle, double* xyz, double* error, uint8_t* keep, uint8_t* obs_keep, void* hdr,
                         void* stream) {
    if (!xy || !view_off || !track_off || !track_view || !track_kp || !centers || !rays || !proj || !xyz || !error || !keep || !obs_keep || !hdr || V < 1 ||
        V > MVSDF_VS_MAX_VIEWS || T < 1 || T > INT_MAX || nnz < 1 || nnz > INT_MAX || !(max_reproj >= 0) || !(cos_min_angle >= -1 && cos_min_angle <= 1))
        return mv_fail(-1, "mvsdf_kp_triangulate: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = mv_check(hipMemsetAsync(hdr, 0, CH_HDR, s), "mvsdf_kp_triangulate")) return rc;
    hipLaunchKernelGGL(k_any_nonfinite<double>, dim3(1), dim3(MV_THREADS), 0, s, centers, (long long)V * 3, (unsigned long long*)hdr + MVSDF_ERRW_H_ERR,
                       (unsigned long long)MVSDF_PS_ERR_FINITE);
    hipLaunchKernelGGL(k_any_nonfinite<double>, dim3(1), dim3(MV_THREADS), 0, s, rays, (long long)V * 9, (unsigned long long*)hdr + MVSDF_ERRW_H_ERR,
                       (unsigned long long)MVSDF_PS_ERR_FINITE);
    hipLaunchKernelGGL(k_any_nonfinite<double>, dim3(1), dim3(MV_THREADS), 0, s, proj, (long long)V * 12, (unsigned long long*)hdr + MVSDF_ERRW_H_ERR,
                       (unsigned long long)MVSDF_PS_ERR_FINITE);
    const KpObs o{xy, (const long long*)view_off, (const int*)track_view, (const int*)track_kp, centers, rays, proj};
    hipLaunchKernelGGL(k_kp_triangulate, dim3(mv_grid(T, CH_THREADS)), dim3(CH_THREADS), 0, s, o, (long long)V, (const long long*)track_off, (long long)T,
                       (long long)nnz, max_reproj, cos_min_angle, xyz, error, (unsigned char*)keep, (unsigned char*)obs_keep,
                       (long long*)hdr + MVSDF_ERRW_H_ERR);
    return mv_check(hipGetLastError(), "mvsdf_kp_triangulate");
}

}  // extern "C"
