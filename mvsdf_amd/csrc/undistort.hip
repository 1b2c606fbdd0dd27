// undistort.hip -- on-device image undistortion: COLMAP's distorted camera models to pinhole views.  Python: mvsdf_amd/undistort.py, which states the
// definition operation by operation; tests/undistort_ref.py restates it in numpy.  All arithmetic is fp64 without contraction, in the order the
// definition writes it; the fisheye models' atan2 is the written-out one of det_math64.h (no library call).
//
// * ud_distort / ud_undistort / ud_source / ud_blend: the definition's arithmetic, host and device (the mvsdf_undistort_*_host entry points run the same
//   functions on the CPU, so the non-GPU suite pins them to the numpy restatement).
// * k_undistort_points: one lane per point; the forward map D, or the Newton iteration of the inverse map U (at most 32 updates, five evaluations of D
//   each).  A lane that meets a non-finite value, a zero determinant or a final residual above the bound ORs its error bit into the header.
// * k_undistort_images<T, C>: a wave owns 64 consecutive output pixels (row-major over the whole output image, so a run may cross a row end) and every
//   view of the chunk.  Lane l evaluates the source coordinate of pixel l of the run ONCE per launch and writes the mask byte.  The wave then turns the
//   64 pixels into 64 C output elements: in pass j lane l owns element e = 64 j + l of the run, pixel e / C, channel e % C, and fetches that pixel's
//   first texel offset, the two neighbour strides and the two weights from the lane that computed them (ds_bpermute, once per launch, C sets of eight
//   registers).  The view loop then does, per pass, four loads, the blend and ONE store whose 64 lanes write 64 consecutive elements -- for uint8 RGB
//   three stores of 64 contiguous bytes per 64 pixels, however the 3-byte pixels fall -- and neighbouring lanes load neighbouring bytes of the same
//   texels.  No coordinate map goes through memory.  All offsets are 64-bit (views * H * W * C passes 2^31 for a real scene).
//
// Error bits of the points call (int64 {0, bits} in the 256-byte header, which the call resets): 1 a non-finite value or a zero determinant in the
// iteration (or a non-finite result of the forward map), 2 a final residual above 1e-10 px.
#include <float.h>
#include "geom_prims.h"
#include "det_math64.h"

#define UD_THREADS 256
#define UD_HDR 256
static_assert(MVSDF_RES_H_WORDS * 8 <= UD_HDR, "the result words fit the header");
#define UD_MAX_UPDATES 32
#define UD_STEP 1e-6                                  // the central differences' step, in normalised coordinates
#define UD_STOP_PX 1e-13                              // a lane stops updating at a residual of at most this (pixels)
#define UD_BOUND_PX 1e-10                             // a final residual above this is an error
#define UD_FISHEYE_EPS 1e-8

enum { UD_PINHOLE = 0, UD_RADIAL = 1, UD_OPENCV = 2, UD_FISHEYE = 3 };
enum { UD_U8 = 0, UD_F32 = 1 };

struct UdCam {
    double fx, fy, cx, cy, k[8];
    int model;
};

struct UdPin {
    double fx, fy, cx, cy;
};

struct UdXY {
    double x, y;
};

// ---- the definition's arithmetic, host and device ----

// the forward map D on normalised coordinates
__host__ __device__ static inline UdXY ud_distort(const UdCam& c, double u, double v) {
    const double r2 = u * u + v * v;
    UdXY o = {u, v};
    if (c.model == UD_RADIAL) {
        const double r4 = r2 * r2;
        const double s = (1.0 + c.k[0] * r2) + c.k[1] * r4;
        o.x = u * s;
        o.y = v * s;
    } else if (c.model == UD_OPENCV) {
        const double r4 = r2 * r2;
        const double r6 = r4 * r2;
        const double num = ((1.0 + c.k[0] * r2) + c.k[1] * r4) + c.k[4] * r6;
        const double den = ((1.0 + c.k[5] * r2) + c.k[6] * r4) + c.k[7] * r6;
        const double s = num / den;
        const double tx = ((2.0 * c.k[2]) * u) * v + c.k[3] * (r2 + (2.0 * u) * u);
        const double ty = ((2.0 * c.k[3]) * u) * v + c.k[2] * (r2 + (2.0 * v) * v);
        o.x = u * s + tx;
        o.y = v * s + ty;
    } else if (c.model == UD_FISHEYE) {
        const double r = sqrt(r2);
        const double theta = dm64_atan2_pos(r, 1.0);
        const double t2 = theta * theta;
        double p = c.k[3];
        p = p * t2 + c.k[2];
        p = p * t2 + c.k[1];
        p = p * t2 + c.k[0];
        p = p * t2 + 1.0;
        const double thetad = theta * p;
        const double s = r > UD_FISHEYE_EPS ? thetad / r : 1.0;
        o.x = u * s;
        o.y = v * s;
    }
    return o;
}

__host__ __device__ static inline double ud_abs(double a) { return a < 0.0 ? -a : a; }
__host__ __device__ static inline bool ud_finite(double a) { return ud_abs(a) <= DBL_MAX; }          // false for NaN

// the inverse map U: Newton on D from (xd, yd) -> *o; returns the lane's error bits
__host__ __device__ static inline int ud_undistort(const UdCam& c, double xd, double yd, UdXY* o) {
    const double h = UD_STEP, h2 = 2.0 * UD_STEP;
    double x = xd, y = yd, res = 0.0;
    int err = 0;
    for (int it = 0; it <= UD_MAX_UPDATES; ++it) {
        const UdXY f = ud_distort(c, x, y);
        const double ex = f.x - xd, ey = f.y - yd;
        if (!ud_finite(ex) || !ud_finite(ey)) { err = MVSDF_UD_ERR_FINITE; break; }
        const double rx = ud_abs(ex) * c.fx, ry = ud_abs(ey) * c.fy;
        res = rx > ry ? rx : ry;
        if (res <= UD_STOP_PX || it == UD_MAX_UPDATES) break;
        const UdXY a = ud_distort(c, x + h, y), b = ud_distort(c, x - h, y), p = ud_distort(c, x, y + h), q = ud_distort(c, x, y - h);
        const double j00 = (a.x - b.x) / h2, j01 = (p.x - q.x) / h2, j10 = (a.y - b.y) / h2, j11 = (p.y - q.y) / h2;
        const double det = j00 * j11 - j01 * j10;
        if (!ud_finite(det) || det == 0.0) { err = MVSDF_UD_ERR_FINITE; break; }
        const double sx = (j11 * ex - j01 * ey) / det, sy = (j00 * ey - j10 * ex) / det;
        x = x - sx;
        y = y - sy;
    }
    if (!err && res > UD_BOUND_PX) err = MVSDF_UD_ERR_CONVERGE;
    o->x = x;
    o->y = y;
    return err;
}

// one point of the points call: source pixels -> pinhole pixels through U (inverse), or pinhole pixels -> source pixels through D
__host__ __device__ static inline int ud_point(const UdCam& c, const UdPin& p, int inverse, double X, double Y, UdXY* o) {
    if (inverse) {
        UdXY r;
        const int err = ud_undistort(c, (X - c.cx) / c.fx, (Y - c.cy) / c.fy, &r);
        o->x = p.fx * r.x + p.cx;
        o->y = p.fy * r.y + p.cy;
        return err;
    }
    const UdXY r = ud_distort(c, (X - p.cx) / p.fx, (Y - p.cy) / p.fy);
    o->x = c.fx * r.x + c.cx;
    o->y = c.fy * r.y + c.cy;
    return ud_finite(o->x) && ud_finite(o->y) ? 0 : MVSDF_UD_ERR_FINITE;
}

// where output pixel (x, y) of the pinhole p looks in the source image [H][W]: the first texel (y0 * W + x0, in pixels; -1 = invalid), the steps to
// the x and the y neighbour (0 where the neighbour is clamped onto the texel itself) and the weights
struct UdTap {
    long long first;
    int dx, dy;
    double tx, ty;
};

__host__ __device__ static inline UdTap ud_source(const UdCam& c, const UdPin& p, long long W, long long H, long long x, long long y) {
    const double u = (((double)x + 0.5) - p.cx) / p.fx, v = (((double)y + 0.5) - p.cy) / p.fy;
    const UdXY d = ud_distort(c, u, v);
    const double Xs = c.fx * d.x + c.cx, Ys = c.fy * d.y + c.cy;
    UdTap t = {-1, 0, 0, 0.0, 0.0};
    if (!(Xs >= 0.0 && Xs <= (double)W && Ys >= 0.0 && Ys <= (double)H)) return t;         // NaN is invalid
    const double a = Xs - 0.5, b = Ys - 0.5;
    const double fx0 = floor(a), fy0 = floor(b);
    t.tx = a - fx0;
    t.ty = b - fy0;
    const long long x0 = (long long)fx0, y0 = (long long)fy0;                             // in [-1, W - 1] and [-1, H - 1]
    const long long x0c = x0 < 0 ? 0 : x0, y0c = y0 < 0 ? 0 : y0;
    const long long x1c = x0 + 1 > W - 1 ? W - 1 : x0 + 1, y1c = y0 + 1 > H - 1 ? H - 1 : y0 + 1;
    t.first = y0c * W + x0c;
    t.dx = (int)(x1c - x0c);
    t.dy = (int)(y1c - y0c);
    return t;
}

__host__ __device__ static inline double ud_blend(double tx, double ty, double p00, double p10, double p01, double p11) {
    return (1.0 - ty) * ((1.0 - tx) * p00 + tx * p10) + ty * ((1.0 - tx) * p01 + tx * p11);
}

__host__ __device__ static inline unsigned char ud_round(double v, unsigned char) { return (unsigned char)(int)floor(v + 0.5); }
__host__ __device__ static inline float ud_round(double v, float) { return (float)v; }

// ---- kernels ----

__global__ __launch_bounds__(UD_THREADS) void k_undistort_points(const double* __restrict__ pts, long long n, UdCam cam, UdPin pin, int inverse,
                                                                 double* __restrict__ out, unsigned long long* __restrict__ hdr) {
    const long long i = (long long)blockIdx.x * UD_THREADS + threadIdx.x;
    if (i >= n) return;
    UdXY o;
    const int err = ud_point(cam, pin, inverse, pts[2 * i], pts[2 * i + 1], &o);
    out[2 * i] = o.x;
    out[2 * i + 1] = o.y;
    if (err) atomicOr(hdr + MVSDF_RES_H_ERR, (unsigned long long)err);
}

__device__ __forceinline__ double ud_shfl(double v, int lane) {
    const long long b = __double_as_longlong(v);
    const int lo = __shfl((int)b, lane), hi = __shfl((int)(b >> 32), lane);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

__device__ __forceinline__ long long ud_shfl(long long b, int lane) {
    const int lo = __shfl((int)b, lane), hi = __shfl((int)(b >> 32), lane);
    return ((long long)hi << 32) | (unsigned)lo;
}

// src [views][H][W][C], dst [views][oH][oW][C], mask [oH][oW] or null
template <class T, int C>
__global__ __launch_bounds__(UD_THREADS) void k_undistort_images(const T* __restrict__ src, long long views, long long H, long long W, UdCam cam, UdPin pin,
                                                                 long long oH, long long oW, T* __restrict__ dst, unsigned char* __restrict__ mask) {
    const int lane = threadIdx.x & 63;
    const long long npix = oH * oW;
    const long long run = ((long long)blockIdx.x * UD_THREADS + threadIdx.x) - lane;       // the first pixel of the wave's run; below npix (the grid)
    const long long pix = run + lane;
    UdTap t = {-1, 0, 0, 0.0, 0.0};
    if (pix < npix) {
        const long long y = pix / oW;
        t = ud_source(cam, pin, W, H, pix - y * oW, y);
        if (mask) mask[pix] = t.first >= 0;
    }
    // pass j: this lane's element 64 j + lane of the run's 64 C elements
    long long first[C];
    int dx[C], dy[C];
    double tx[C], ty[C];
    const long long nel = (npix - run < 64 ? npix - run : 64) * C;                         // elements of the run that exist
#pragma unroll
    for (int j = 0; j < C; ++j) {
        const int e = j * 64 + lane, p = e / C, ch = e - p * C;
        const long long f = ud_shfl(t.first, p);
        dx[j] = __shfl(t.dx, p) * C;
        dy[j] = __shfl(t.dy, p);
        tx[j] = ud_shfl(t.tx, p);
        ty[j] = ud_shfl(t.ty, p);
        first[j] = e >= nel ? -2 : (f < 0 ? -1 : f * C + ch);                               // -2: no such element, -1: an invalid pixel's element
    }
    const long long sstride = H * W * C, dstride = npix * C, rowstep = W * C;
    const long long at = run * C + lane;
    for (long long v = 0; v < views; ++v) {
        const T* __restrict__ s = src + v * sstride;
        T* __restrict__ d = dst + v * dstride + at;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            if (first[j] == -2) continue;
            T o = 0;
            if (first[j] >= 0) {
                const T* __restrict__ q = s + first[j];
                const long long down = (long long)dy[j] * rowstep;
                o = ud_round(ud_blend(tx[j], ty[j], (double)q[0], (double)q[dx[j]], (double)q[down], (double)q[down + dx[j]]), T());
            }
            d[j * 64] = o;
        }
    }
}

template <class T>
static int ud_launch_images(int C, unsigned blocks, hipStream_t s, const void* src, long long views, long long H, long long W, const UdCam& cam, const UdPin& pin,
                            long long oH, long long oW, void* dst, unsigned char* mask) {
    const dim3 g(blocks), b(UD_THREADS);
    switch (C) {
        case 1: hipLaunchKernelGGL((k_undistort_images<T, 1>), g, b, 0, s, (const T*)src, views, H, W, cam, pin, oH, oW, (T*)dst, mask); break;
        case 2: hipLaunchKernelGGL((k_undistort_images<T, 2>), g, b, 0, s, (const T*)src, views, H, W, cam, pin, oH, oW, (T*)dst, mask); break;
        case 3: hipLaunchKernelGGL((k_undistort_images<T, 3>), g, b, 0, s, (const T*)src, views, H, W, cam, pin, oH, oW, (T*)dst, mask); break;
        default: hipLaunchKernelGGL((k_undistort_images<T, 4>), g, b, 0, s, (const T*)src, views, H, W, cam, pin, oH, oW, (T*)dst, mask); break;
    }
    return mv_check(hipGetLastError(), "mvsdf_undistort_images");
}

// params: host fp64 [12] = fx, fy, cx, cy and the model's eight coefficients; false when the model or a value cannot be used
static bool ud_camera(int model, const double* params, UdCam* c) {
    if (!params || model < UD_PINHOLE || model > UD_FISHEYE) return false;
    for (int i = 0; i < 12; ++i)
        if (!isfinite(params[i])) return false;
    if (!(params[0] > 0.0) || !(params[1] > 0.0)) return false;
    c->fx = params[0];
    c->fy = params[1];
    c->cx = params[2];
    c->cy = params[3];
    for (int i = 0; i < 8; ++i) c->k[i] = params[4 + i];
    c->model = model;
    return true;
}

static bool ud_pinhole(const double* p, UdPin* o) {
    if (!p || !isfinite(p[0]) || !isfinite(p[1]) || !isfinite(p[2]) || !isfinite(p[3]) || !(p[0] > 0.0) || !(p[1] > 0.0)) return false;
    o->fx = p[0];
    o->fy = p[1];
    o->cx = p[2];
    o->cy = p[3];
    return true;
}

static const long long UD_MAX_SIDE = 1ll << 24;       // per image side; H * W * C then stays far inside int64, and a row step inside int32

static bool ud_image_shape(int64_t views, int64_t H, int64_t W, int64_t C, int dtype, int64_t oH, int64_t oW) {
    return views >= 0 && H >= 1 && W >= 1 && H <= UD_MAX_SIDE && W <= UD_MAX_SIDE && C >= 1 && C <= 4 && oH >= 1 && oW >= 1 && oH <= UD_MAX_SIDE && oW <= UD_MAX_SIDE &&
           (dtype == UD_U8 || dtype == UD_F32);
}

extern "C" {

int mvsdf_undistort_points(const double* points, int64_t n, int model, const double* params, const double* pinhole, int inverse, double* out, void* hdr,
                           void* stream) {
    const char* what = "mvsdf_undistort_points";
    UdCam cam;
    UdPin pin;
    if (!hdr || n < 0 || (n > 0 && (!points || !out)) || !ud_camera(model, params, &cam) || !ud_pinhole(pinhole, &pin))
        return mv_fail(-1, "mvsdf_undistort_points: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = mv_check(hipMemsetAsync(hdr, 0, UD_HDR, s), what)) return rc;
    if (n == 0) return 0;
    const unsigned blocks = mv_grid(n, UD_THREADS);
    if (!blocks) return mv_fail(-1, "mvsdf_undistort_points: n beyond the grid limit");
    hipLaunchKernelGGL(k_undistort_points, dim3(blocks), dim3(UD_THREADS), 0, s, points, (long long)n, cam, pin, inverse ? 1 : 0, out, (unsigned long long*)hdr);
    return mv_check(hipGetLastError(), what);
}

int mvsdf_undistort_images(const void* src, int64_t views, int64_t H, int64_t W, int64_t C, int dtype, int model, const double* params, const double* out_pinhole,
                           int64_t oH, int64_t oW, void* dst, uint8_t* mask, void* stream) {
    UdCam cam;
    UdPin pin;
    if (!ud_image_shape(views, H, W, C, dtype, oH, oW) || (views > 0 && (!src || !dst)) || !ud_camera(model, params, &cam) || !ud_pinhole(out_pinhole, &pin))
        return mv_fail(-1, "mvsdf_undistort_images: bad arguments");
    if (views == 0 && !mask) return 0;
    const unsigned blocks = mv_grid((long long)oH * oW, UD_THREADS);
    if (!blocks) return mv_fail(-1, "mvsdf_undistort_images: the output image is beyond the grid limit");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == UD_U8) return ud_launch_images<unsigned char>((int)C, blocks, s, src, views, H, W, cam, pin, oH, oW, dst, mask);
    return ud_launch_images<float>((int)C, blocks, s, src, views, H, W, cam, pin, oH, oW, dst, mask);
}

// HOST: the points call on the CPU (host memory), by the same functions the kernel runs; *err receives the OR of the error bits.  The library loads
// without a GPU, so the non-GPU suite pins the arithmetic to the numpy restatement through this.
int mvsdf_undistort_points_host(const double* points, int64_t n, int model, const double* params, const double* pinhole, int inverse, double* out, int64_t* err) {
    UdCam cam;
    UdPin pin;
    if (!err || n < 0 || (n > 0 && (!points || !out)) || !ud_camera(model, params, &cam) || !ud_pinhole(pinhole, &pin))
        return mv_fail(-1, "mvsdf_undistort_points_host: bad arguments");
    *err = 0;
    for (int64_t i = 0; i < n; ++i) {
        UdXY o;
        *err |= ud_point(cam, pin, inverse ? 1 : 0, points[2 * i], points[2 * i + 1], &o);
        out[2 * i] = o.x;
        out[2 * i + 1] = o.y;
    }
    return 0;
}

// HOST: the images call on the CPU (host memory), pixel by pixel through the same functions
int mvsdf_undistort_images_host(const void* src, int64_t views, int64_t H, int64_t W, int64_t C, int dtype, int model, const double* params,
                                const double* out_pinhole, int64_t oH, int64_t oW, void* dst, uint8_t* mask) {
    UdCam cam;
    UdPin pin;
    if (!ud_image_shape(views, H, W, C, dtype, oH, oW) || (views > 0 && (!src || !dst)) || !ud_camera(model, params, &cam) || !ud_pinhole(out_pinhole, &pin))
        return mv_fail(-1, "mvsdf_undistort_images_host: bad arguments");
    const long long rowstep = W * C;
    for (long long y = 0; y < oH; ++y)
        for (long long x = 0; x < oW; ++x) {
            const UdTap t = ud_source(cam, pin, W, H, x, y);
            if (mask) mask[y * oW + x] = t.first >= 0;
            for (long long v = 0; v < views; ++v)
                for (int ch = 0; ch < C; ++ch) {
                    const long long o = ((v * oH + y) * oW + x) * C + ch, down = t.dy * rowstep, right = t.dx * C;
                    const long long q = t.first < 0 ? 0 : v * H * rowstep + t.first * C + ch;
                    if (dtype == UD_U8) {
                        const unsigned char* p = (const unsigned char*)src + q;
                        ((unsigned char*)dst)[o] = t.first < 0 ? 0 : ud_round(ud_blend(t.tx, t.ty, p[0], p[right], p[down], p[down + right]), (unsigned char)0);
                    } else {
                        const float* p = (const float*)src + q;
                        ((float*)dst)[o] = t.first < 0 ? 0.0f : ud_round(ud_blend(t.tx, t.ty, p[0], p[right], p[down], p[down + right]), 0.0f);
                    }
                }
        }
    return 0;
}

}  // extern "C"
