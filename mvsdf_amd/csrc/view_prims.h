// view_prims.h -- what a module that looks through a 4x4 projection P (rows u z, v z, z) into an image[H][W] shares, each rule once: the projection to
// pixel coordinates, the 2x2 bilinear cell with its blend, the RGB gather, the visibility test against a depth map, the signed edge function, and on
// the host the view shape, the pixel-centre convention and the finite check of uploaded matrices.  Users: fusion.hip, tsdf.hip, stereo.hip,
// raster.hip, texture.hip.  Every one of them is held bit for bit to a numpy restatement under tests/, so the order of operations written here is
// the definitions' and must not move: which side the last column belongs to, or what z <= 0 means, is decided in this file alone.
//
// Left alone on purpose:
// * undistort.hip: its tap clamps both neighbours and blends in another order; those are other bits, pinned by its own reference.
// * loss_kernels.hip: fp32, with forward-mode derivatives.
// * bundle.hip::ba_project and keypoints.hip::kp_reproject: pose plus intrinsics, and a residual that is not a pixel.
// * the numpy references under tests/ are not merged: their independence from the device code is what makes them a check.
#pragma once
#include "geom_prims.h"

// ================================================================ host ================================================================
// the views and the image size a raster or texture call takes (a module's further caps stand beside its call)
static inline bool mv_view_shape(long long views, long long H, long long W) {
    return views >= 1 && views <= MVSDF_RA_MAX_VIEWS && H >= 2 && W >= 2 && H <= INT_MAX && W <= INT_MAX && H * W <= INT_MAX;
}

// pixel (x, y) has its centre at (x + o, y + o): 0.5, or 0 for integer centres
static inline bool mv_pixel_center(double o) { return o == 0.5 || o == 0.0; }

// host matrices before they are uploaded
static inline bool mv_all_finite(const double* m, long long n) {
    for (long long k = 0; k < n; ++k)
        if (!isfinite(m[k])) return false;
    return true;
}

// ================================================================ device: projection ================================================================
// (q0, q1, q2, 1) through P -> the depth z, then the pixel coordinates sx, sy; false (sx, sy unset): not in front, !(z > 0).  A caller whose loop is
// tight on registers initialises the outputs it declares inside the loop (MvProj pr = {}): what a failed call leaves unset the compiler otherwise
// carries from one iteration to the next, 12 VGPRs in k_ps_score<32> and a wave of occupancy in k_ps_band<32> by its resource report.
__device__ __forceinline__ bool mv_project(const double* __restrict__ P, double q0, double q1, double q2, double& sx, double& sy, double& z) {
    z = mv_row4(P + 8, q0, q1, q2, 1.0);
    if (!(z > 0.0)) return false;
    sx = mv_row4(P, q0, q1, q2, 1.0) / z;
    sy = mv_row4(P + 4, q0, q1, q2, 1.0) / z;
    return true;
}

// the same of an fp32 vertex
__device__ __forceinline__ bool mv_project(const double* __restrict__ P, const float* __restrict__ X, double& sx, double& sy, double& z) {
    return mv_project(P, (double)X[0], (double)X[1], (double)X[2], sx, sy, z);
}

// The depth-map sample of fusion.hip and tsdf.hip, which must agree: TSDF fusion consumes what the depth-map fusion produces; stereo.hip samples its
// descriptor maps the same way.  Coordinates are texel-centre ones: texel (x, y) of map[H][W] has its centre at u = x, v = y.
struct MvProj {
    double z, u, v;
};

// mv_project in texel-centre coordinates -> o; false when z <= 0 or (u, v) lies outside [0, W - 1] x [0, H - 1], the area the 2x2 cells cover
__device__ __forceinline__ bool mv_project_texel(const double* __restrict__ P, double q0, double q1, double q2, int W, int H, MvProj* o) {
    if (!mv_project(P, q0, q1, q2, o->u, o->v, o->z)) return false;
    o->u = o->u - 0.5;
    o->v = o->v - 0.5;
    return o->u >= 0.0 && o->u <= (double)(W - 1) && o->v >= 0.0 && o->v <= (double)(H - 1);
}

// ================================================================ device: the 2x2 cell ================================================================
// the 2x2 cell of an image[H][W] that holds (u, v) in [0, W - 1] x [0, H - 1], the last column / row belonging to the cell before it: its first texel
// and the weights.  What the four values are, and which of them count as valid, is the caller's.
struct MvCell {
    int x0, y0;
    double fx, fy;
    __device__ __forceinline__ double blend(double v00, double v01, double v10, double v11) const {
        return (v00 * (1.0 - fx) + v01 * fx) * (1.0 - fy) + (v10 * (1.0 - fx) + v11 * fx) * fy;
    }
};

__device__ __forceinline__ MvCell mv_cell(double u, double v, int W, int H) {
    const double x0 = fmin(floor(u), (double)(W - 2)), y0 = fmin(floor(v), (double)(H - 2));
    return {(int)x0, (int)y0, u - x0, v - y0};
}

// the cell of a float map with its four texels
struct MvCell2 {
    double d00, d01, d10, d11;
    MvCell at;
    __device__ __forceinline__ double bilinear() const { return at.blend(d00, d01, d10, d11); }
};

__device__ __forceinline__ MvCell2 mv_cell2(const float* __restrict__ map, int W, int H, double u, double v) {
    const MvCell at = mv_cell(u, v, W, H);
    const float* __restrict__ t = map + (long long)at.y0 * W + at.x0;
    return {(double)t[0], (double)t[1], (double)t[W], (double)t[W + 1], at};
}

// the blend of the cell's four texels, per channel, in the image of images[..][H][W][3] (uint8) whose first texel has index first
__device__ __forceinline__ void mv_gather_rgb(const unsigned char* __restrict__ images, long long first, int W, const MvCell& at, double* col) {
    const unsigned char* __restrict__ q = images + (first + (long long)at.y0 * W + at.x0) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) col[c] = at.blend((double)q[c], (double)q[3 + c], (double)q[(long long)W * 3 + c], (double)q[(long long)W * 3 + 3 + c]);
}

// ================================================================ device: visibility and coverage ================================================================
// (sx, sy) lies where the 2x2 cells of an image with pixel centre o reach: (sx - o, sy - o) in [0, wmax] x [0, hmax], wmax = W - 1, hmax = H - 1
__device__ __forceinline__ bool mv_in_image(double sx, double sy, double o, double wmax, double hmax) {
    const double u = sx - o, t = sy - o;
    return u >= 0.0 && u <= wmax && t >= 0.0 && t <= hmax;
}

// X is seen in one view: in front, its nearest pixel inside the image and drawn (D > 0), z <= D (1 + depth_tol), and the mask (or none) set there;
// sx, sy are valid when it returns true
__device__ __forceinline__ bool mv_visible(const double* __restrict__ P, const float* __restrict__ X, double o, int H, int W,
                                           const float* __restrict__ depth, const unsigned char* __restrict__ mask, double depth_tol, double& sx,
                                           double& sy) {
    double z;
    if (!mv_project(P, X, sx, sy, z)) return false;
    const double x = floor(sx - o + 0.5), y = floor(sy - o + 0.5);
    if (!(x >= 0.0 && x < (double)W && y >= 0.0 && y < (double)H)) return false;
    const long long at = (long long)(int)y * W + (int)x;
    const float D = depth[at];
    if (!(D > 0.0f)) return false;
    if (!(z <= (double)D * (1.0 + depth_tol))) return false;
    return !mask || mask[at] != 0;
}

// twice the signed area of (p, q, r)
__device__ __forceinline__ double mv_edge(double px, double py, double qx, double qy, double rx, double ry) {
    return (qx - px) * (ry - py) - (qy - py) * (rx - px);
}
