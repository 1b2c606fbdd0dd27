/* det_math64.h -- deterministic fp64 atan2 and exp (host + gfx950 device), for mvsdf_amd/viewsel.py.
 *
 * Built ONLY from +, -, *, /, compares / selects, one double -> int64 conversion of a whole number and bit casts: every one of them is correctly
 * rounded (or exact) under IEEE-754, so a gfx950 kernel, the host compiler and a numpy restatement (tests/viewsel_ref.py) give identical bits.  ocml's
 * and the host libm's atan2 / exp do not agree bit for bit, which is why they are not used.  Unlike det_math.h there is NO fma here: every step is a
 * plain multiplication followed by a plain addition, so that numpy can restate it operation for operation.  Compile with -ffp-contract=off
 * (mvsdf_amd/build.py::FLAGS); the constants written as quotients are folded by the compiler with one correctly rounded division, as numpy does.
 *
 * Accuracy (tests/test_viewsel_host.py): a few ulp; what viewsel needs is an absolute 2^-33 on the weight.
 */
#ifndef MVSDF_DET_MATH64_H
#define MVSDF_DET_MATH64_H
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DM64_FN __host__ __device__ static inline
#else
#define DM64_FN static inline
#endif

DM64_FN double dm64_from_bits(uint64_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __longlong_as_double((long long)u);
#else
    double f; memcpy(&f, &u, 8); return f;
#endif
}

DM64_FN uint64_t dm64_to_bits(double f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint64_t)__double_as_longlong(f);
#else
    uint64_t u; memcpy(&u, &f, 8); return u;
#endif
}

#define DM64_MAGIC 6755399441055744.0               /* 1.5 * 2^52: t = x + MAGIC, t - MAGIC is x rounded to the nearest integer (ties to even), |x| < 2^51 */
#define DM64_TAN_PI_8 0.41421356237309503
#define DM64_PI 3.141592653589793
#define DM64_PI_2 1.5707963267948966
#define DM64_PI_4 0.7853981633974483
#define DM64_DEG 57.29577951308232                  /* 180 / pi */
#define DM64_LOG2E 1.4426950408889634
#define DM64_LN2_HI 0.6931471803691238              /* 0x3fe62e42fee00000: the low 21 mantissa bits are 0, n * LN2_HI is exact for |n| < 2^21 */
#define DM64_LN2_LO 1.9082149292705877e-10
#define DM64_EXP_MIN (-708.0)                       /* exp(-708) = 3.3e-308 is still a normal double */

/* round to the nearest integer, ties to even; |x| < 2^51 */
DM64_FN double dm64_rint(double x) {
    double t = x + DM64_MAGIC;
    return t - DM64_MAGIC;
}

/* atan2(y, x) in radians for y >= 0 (any finite x): [0, pi]; atan2(0, 0) = 0 whatever the sign of x.
 * z = min(y, |x|) / max(y, |x|) in [0, 1]; above tan(pi/8) the argument becomes (z - 1) / (z + 1) in [-tan(pi/8), 0) and pi/4 is added;
 * atan(z) = z * (1 - z^2/3 + z^4/5 - ... + z^38/39) by Horner in z^2 from the highest term down (the first omitted term is below 1.2e-17 relative);
 * then pi/2 - r where y > |x|, and pi - r where x < 0. */
DM64_FN double dm64_atan2_pos(double y, double x) {
    const double ax = x < 0.0 ? -x : x;
    if (y == 0.0 && ax == 0.0) return 0.0;
    const bool swap = y > ax;
    const double num = swap ? ax : y, den = swap ? y : ax;
    double z = num / den;
    const bool hi = z > DM64_TAN_PI_8;
    if (hi) z = (z - 1.0) / (z + 1.0);
    const double z2 = z * z;
    double p = -1.0 / 39.0;
    p = p * z2 + 1.0 / 37.0;
    p = p * z2 + -1.0 / 35.0;
    p = p * z2 + 1.0 / 33.0;
    p = p * z2 + -1.0 / 31.0;
    p = p * z2 + 1.0 / 29.0;
    p = p * z2 + -1.0 / 27.0;
    p = p * z2 + 1.0 / 25.0;
    p = p * z2 + -1.0 / 23.0;
    p = p * z2 + 1.0 / 21.0;
    p = p * z2 + -1.0 / 19.0;
    p = p * z2 + 1.0 / 17.0;
    p = p * z2 + -1.0 / 15.0;
    p = p * z2 + 1.0 / 13.0;
    p = p * z2 + -1.0 / 11.0;
    p = p * z2 + 1.0 / 9.0;
    p = p * z2 + -1.0 / 7.0;
    p = p * z2 + 1.0 / 5.0;
    p = p * z2 + -1.0 / 3.0;
    p = p * z2 + 1.0;
    double r = z * p;
    if (hi) r = DM64_PI_4 + r;
    if (swap) r = DM64_PI_2 - r;
    if (x < 0.0) r = DM64_PI - r;
    return r;
}

/* exp(x) for x <= 0, clamped at x = -708 (anything that is not > -708, a NaN included, counts as -708).
 * n = rint(x * log2(e)); r = (x - n * LN2_HI) - n * LN2_LO in [-0.35, 0.35]; exp(r) = 1 + r + r^2/2! + ... + r^14/14! by Horner from the highest
 * term down (the first omitted term is below 2e-19); the result is that sum with n added to its exponent field (it stays a normal number). */
DM64_FN double dm64_expneg(double x) {
    if (!(x > DM64_EXP_MIN)) x = DM64_EXP_MIN;
    const double n = dm64_rint(x * DM64_LOG2E);
    const double r = (x - n * DM64_LN2_HI) - n * DM64_LN2_LO;
    double p = 1.0 / 87178291200.0;
    p = p * r + 1.0 / 6227020800.0;
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    return dm64_from_bits(dm64_to_bits(p) + ((uint64_t)(int64_t)n << 52));
}

#endif
