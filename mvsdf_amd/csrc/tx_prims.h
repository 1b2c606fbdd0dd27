// tx_prims.h -- what texture.hip and charts.hip share, each rule once: the test of one face in one view (step 1 of texture.py's definition), which
// both the label pass (every view, the largest score) and the chart stages (the one view named) run, so a score is the same bits wherever it is asked for.
#pragma once
#include "view_prims.h"

// what the test of a face needs in every view: its corners, the summed normal and the centroid
struct TxFace {
    const float *Xa, *Xb, *Xc;
    double n0, n1, n2, m0, m1, m2, nn;
    bool flat;                                        // n.n == 0: passes the normal test with ignore_normals, fails without
};

// corners a, b, c must be inside [0, nv)
__device__ __forceinline__ TxFace tx_face(const float* __restrict__ verts, const float* __restrict__ normals, int a, int b, int c) {
    TxFace F;
    F.Xa = verts + (long long)a * 3, F.Xb = verts + (long long)b * 3, F.Xc = verts + (long long)c * 3;
    const float *Na = normals + (long long)a * 3, *Nb = normals + (long long)b * 3, *Nc = normals + (long long)c * 3;
    F.n0 = ((double)Na[0] + (double)Nb[0]) + (double)Nc[0], F.n1 = ((double)Na[1] + (double)Nb[1]) + (double)Nc[1];
    F.n2 = ((double)Na[2] + (double)Nb[2]) + (double)Nc[2];
    F.m0 = (((double)F.Xa[0] + (double)F.Xb[0]) + (double)F.Xc[0]) / 3.0, F.m1 = (((double)F.Xa[1] + (double)F.Xb[1]) + (double)F.Xc[1]) / 3.0;
    F.m2 = (((double)F.Xa[2] + (double)F.Xb[2]) + (double)F.Xc[2]) / 3.0;
    F.nn = (F.n0 * F.n0 + F.n1 * F.n1) + F.n2 * F.n2;
    F.flat = F.nn == 0.0;
    return F;
}

// view v (its P, centre Cv, depth map dv and mask mv) is a candidate for the face: all three corners visible and inside the image, A != 0, the normal
// test -> true with the score |A| and the six screen coordinates in s; the caller has passed over a flat face without ignore_normals
__device__ __forceinline__ bool tx_face_in_view(const TxFace& F, const double* __restrict__ Pv, const double* __restrict__ Cv, double o, int H, int W,
                                                const float* __restrict__ dv, const unsigned char* __restrict__ mv, double depth_tol, double cos_min,
                                                double& sc, double* s) {
    const double wmax = (double)(W - 1), hmax = (double)(H - 1);
    double ax, ay, bx, by, cx, cy;
    if (!mv_visible(Pv, F.Xa, o, H, W, dv, mv, depth_tol, ax, ay)) return false;
    if (!mv_visible(Pv, F.Xb, o, H, W, dv, mv, depth_tol, bx, by)) return false;
    if (!mv_visible(Pv, F.Xc, o, H, W, dv, mv, depth_tol, cx, cy)) return false;
    if (!(mv_in_image(ax, ay, o, wmax, hmax) && mv_in_image(bx, by, o, wmax, hmax) && mv_in_image(cx, cy, o, wmax, hmax))) return false;
    const double A = mv_edge(ax, ay, bx, by, cx, cy);
    if (!(A != 0.0)) return false;
    if (!F.flat) {
        const double g0 = Cv[0] - F.m0, g1 = Cv[1] - F.m1, g2 = Cv[2] - F.m2;
        const double cosang = ((F.n0 * g0 + F.n1 * g1) + F.n2 * g2) / sqrt(((g0 * g0 + g1 * g1) + g2 * g2) * F.nn);
        if (!(cosang > cos_min)) return false;
    }
    sc = fabs(A);
    s[0] = ax, s[1] = ay, s[2] = bx, s[3] = by, s[4] = cx, s[5] = cy;
    return true;
}
