// The 57 kHz mixer of BFMDemod::feed with m_rdsActive set (bfmdemod.cpp:172):
//     Complex r(demod * 2.0 * std::cos(3.0 * m_pilotPLLSamples[3]), 0.0);
// a double product narrowed to float.  std::cos is the host libm's double cosine, which is not correctly rounded and whose
// source this project does not restate.  So the mixer is computed with a cosine of our own with an argued and measured error bound, and every
// sample is checked: if any double within the distance the two bounds allow would give another float r, the sample counts as
// `unsure`.  A feed without unsure samples has mixed exactly as the reference did on any libm that keeps its documented 1 ulp.
// Compiles for the host too (tests/rds_mix_check.cpp), no HIP header needed.
//
// rds_cos(t), |t| <= 32 (t = 3.0 * m_phase is exact in double, and m_phase stays within [0, 2 pi + m_maxfreq]):
//   k = rint(t * 2 / pi), |k| <= 21.  The reduction y = t - k * pi / 2 is done in two Cody-Waite stages with the constants of
//   fdlibm's e_rem_pio2.c: pio2_1 and pio2_2 carry 33 bits each, so k * pio2_1 and k * pio2_2 are exact (38 bits), and
//   t - k * pio2_1 is exact as well: for k != 0, t >= pi / 4 has at most 26 significant bits on a grid of 2^-27 or coarser,
//   k * pio2_1 lies on the grid 2^-32, and the difference is below 2^5.  What remains is the tail pio2_2t, whose own
//   representation error is below 2^-118 * k, and the compensated subtraction that yields y as head + tail with the pair
//   accurate to about 2^-105 relative to the head.  The closest a t of this form comes to a multiple of pi / 2 is 2^-24.7
//   (tests/test_bfm_rds_mix_math.py lists every multiple's neighbours), so y keeps a relative error below 2^-70 at the zeros:
//   nothing against the kernels' own error.
//   The kernels are fdlibm's k_sin.c and k_cos.c on |y| <= pi / 4 (minimax polynomials with error below 2^-58, evaluated with the
//   tail as a first-order correction).  Their documented bound is below 1 ulp, which is what this argument leans on; the last operation of each
//   (x - (...), 1 - (...)) rounds once (0.5 ulp), and everything in front of it enters scaled by at most y^2 / 2 <= 0.31 with at
//   most three roundings of its own, which gives E <= 0.5 + 0.31 * 1.5 + 2^-5 < 1.  That sum is an estimate with little margin, not a proof.  RDS_COS_E = 1 is what the code relies on;
//   the test measures 0.82 ulp at worst over its arguments
//   (the host libm differs from rds_cos on 3 % of them, by one ulp each time).
//   Outside |t| <= 32, or for a NaN, the guard takes the slow path: the same steps on fmod(t, 2 pi)'s exact remainder, where
//   only the sample's `unsure` mark is relied on (rds_mix reports every such sample as unsure).
// The libm's result c' then lies within floor(E + 1) = 1 ulp of ours: |c' - c| < 2 ulp and both are doubles.  The ulp is taken
// from c's binade, so that below a power of two the enclosure is two of the finer steps wide, never one too few.
#pragma once
#include <stdint.h>
#include "udpsrc_scan.hpp"

namespace sdrx {

// std::fmod on doubles is exact by definition: any correct routine returns the same bits
#ifdef __HIP_DEVICE_COMPILE__
__device__ __forceinline__ double rds_fmod(double x, double y) { return ::fmod(x, y); }
#else
inline double rds_fmod(double x, double y) { return __builtin_fmod(x, y); }
#endif

constexpr int RDS_COS_E = 1;            // the bound relied on: |rds_cos(t) - cos(t)| < RDS_COS_E ulp

AM_HD uint64_t rds_dbits(double v) { uint64_t i; __builtin_memcpy(&i, &v, 8); return i; }
AM_HD double rds_dfrom(uint64_t i) { double v; __builtin_memcpy(&v, &i, 8); return v; }

AM_HD double rds_ksin(double x, double y)                    // fdlibm __kernel_sin(x, y, 1)
{
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double z = x * x, v = z * x;
    const double r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    return x - ((z * (0.5 * y - v * r) - y) - v * S1);
}

AM_HD double rds_kcos(double x, double y)                    // fdlibm __kernel_cos(x, y)
{
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double z = x * x;
    const double r = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
    const double ax = __builtin_fabs(x);
    if (ax < 0.3) return 1.0 - (0.5 * z - (z * r - x * y));
    // x / 4 with the low word cleared: 1 - qx and 0.5 * z - qx are then exact
    const double qx = ax > 0.78125 ? 0.28125 : rds_dfrom(((rds_dbits(ax) >> 32) - 0x00200000u) << 32);
    const double hz = 0.5 * z - qx, a = 1.0 - qx;
    return a - (hz - (z * r - x * y));
}

AM_HD double rds_cos_reduced(double t)
{
    const double invpio2 = 6.36619772367581382433e-01;
    const double pio2_1 = 1.57079632673412561417e+00, pio2_2 = 6.07710050630396597660e-11, pio2_2t = 2.02226624879595063154e-21;
    const double fn = __builtin_rint(t * invpio2);
    const int n = (int)fn;
    const double t1 = t - fn * pio2_1;                       // exact
    const double w1 = fn * pio2_2;                           // exact
    const double r = t1 - w1;
    const double w = fn * pio2_2t - ((t1 - r) - w1);
    const double y0 = r - w, y1 = (r - y0) - w;
    switch (n & 3) {
    case 0: return rds_kcos(y0, y1);
    case 1: return -rds_ksin(y0, y1);
    case 2: return -rds_kcos(y0, y1);
    default: return rds_ksin(y0, y1);
    }
}

AM_HD bool rds_cos_in_range(double t) { return __builtin_fabs(t) <= 32.0; }      // false for a NaN

AM_HD double rds_cos(double t)
{
    if (rds_cos_in_range(t)) return rds_cos_reduced(t);
    if (!(__builtin_fabs(t) < 1.0e300)) return t - t;        // inf, NaN: NaN, as cos gives
    return rds_cos_reduced(rds_fmod(t, 2.0 * 3.14159265358979323846));   // slow path: no bound claimed
}

// one ulp of c's binade (c finite); a subnormal c has the subnormals' spacing
AM_HD double rds_ulp(double c)
{
    const uint64_t e = (rds_dbits(c) >> 52) & 0x7ff;
    if (e <= 52) return rds_dfrom(1);
    return rds_dfrom((e - 52) << 52);
}

AM_HD uint32_t rds_fbits(float v) { uint32_t i; __builtin_memcpy(&i, &v, 4); return i; }

// r of a stereo channel from demod and the carried phase; *unsure is set where a cosine within RDS_COS_E ulp of ours (the
// enclosure's two ends: the product is monotonic in the cosine) narrows to another float, -0 and +0 being two floats
AM_HD float rds_mix(float demod, float phase, bool* unsure)
{
    const double t = 3.0 * (double)phase;
    const double c = rds_cos(t);
    const double d2 = (double)demod * 2.0;
    const float r = (float)(d2 * c);
    const double u = rds_ulp(c) * RDS_COS_E;
    const float lo = (float)(d2 * (c - u)), hi = (float)(d2 * (c + u));
    *unsure = !rds_cos_in_range(t) || rds_fbits(lo) != rds_fbits(r) || rds_fbits(hi) != rds_fbits(r);
    return r;
}

} // namespace sdrx
