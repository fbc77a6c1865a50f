/* PhaseLockComplex (sdrbase/dsp/phaselockcomplex.cpp) and FreqLockComplex (freqlockcomplex.cpp) in strict-IEEE C with the libm
 * routines they call written out, shared by tests/chana_pll_oracle.c and tests/am_oracle.c, which include it as text.
 *
 * The loops feed back, so no tolerance means anything and nothing here may come from whatever libm the machine has: cosf, sinf
 * (glibc 2.28+, the build a CPU with FMA is given: every a + b * c one fma()) and atan2f (fdlibm's float routines, glibc up to
 * 2.40) are written out below.  fma() itself is correctly rounded wherever it runs.
 *
 * loops.probe: saturations above / below, normalizeAngle with more than one turn, lock counter ups / downs, cos / sin arguments
 * past 120, arg(0), steps (counted by the caller) */
#ifndef TESTS_PLL_ORACLE_H
#define TESTS_PLL_ORACLE_H
#include <math.h>
#include <stdint.h>
#include <string.h>

/* ---------------------------------------------------------------- libm, restated */
static uint32_t f_bits(float v) { uint32_t i; memcpy(&i, &v, 4); return i; }
static uint32_t top12(float v) { return (f_bits(v) >> 20) & 0x7ff; }

static float sincos_poly(double x, double x2, double cs, int n)
{
    const double c0 = 0x1p0, c1 = -0x1.ffffffd0c621cp-2, c2 = 0x1.55553e1068f19p-5, c3 = -0x1.6c087e89a359dp-10, c4 = 0x1.99343027bf8c3p-16;
    const double s1 = -0x1.555545995a603p-3, s2 = 0x1.1107605230bc4p-7, s3 = -0x1.994eb3774cf24p-13;
    if ((n & 1) == 0) {
        const double x3 = x * x2;
        const double t1 = fma(x2, s3, s2);
        const double x7 = x3 * x2;
        const double s = fma(x3, s1, x);
        return (float)fma(x7, t1, s);
    }
    const double x4 = x2 * x2;
    const double t2 = fma(x2, cs * c4, cs * c3);
    const double t1 = fma(x2, cs * c1, cs * c0);
    const double x6 = x4 * x2;
    const double c = fma(x4, cs * c2, t1);
    return (float)fma(x6, t2, c);
}

static const uint32_t g_inv_pio4[24] = { 0xa2, 0xa2f9, 0xa2f983, 0xa2f9836e, 0xf9836e4e, 0x836e4e44, 0x6e4e4415, 0x4e441529,
                                         0x441529fc, 0x1529fc27, 0x29fc2757, 0xfc2757d1, 0x2757d1f5, 0x57d1f534, 0xd1f534dd, 0xf534ddc0,
                                         0x34ddc0db, 0xddc0db62, 0xc0db6295, 0xdb629599, 0x6295993c, 0x95993c43, 0x993c4390, 0x3c439041 };

static float o_sincosf(float y, int shift)
{
    const double hpi_inv = 0x1.45F306DC9C883p+23, hpi = 0x1.921FB54442D18p0;
    double x = (double)y;
    int n, q;
    if (top12(y) < top12(0x1.921FB6p-1f)) {
        if (top12(y) < top12(0x1p-12f)) return shift ? 1.0f : y;
        return sincos_poly(x, x * x, 1.0, shift);
    }
    if (top12(y) < top12(120.0f)) {
        const double r = x * hpi_inv;
        n = ((int32_t)r + 0x800000) >> 24;
        x = fma(-(double)n, hpi, x);
        q = n;
    } else if (top12(y) < top12(INFINITY)) {
        const uint32_t xi = f_bits(y);
        const uint32_t* arr = &g_inv_pio4[(xi >> 26) & 15];
        const int sh = (int)((xi >> 23) & 7);
        const uint32_t m = ((xi & 0xffffff) | 0x800000) << sh;
        uint64_t r0 = (uint32_t)(m * arr[0]);
        const uint64_t r1 = (uint64_t)m * arr[4], r2 = (uint64_t)m * arr[8];
        r0 = (r2 >> 32) | (r0 << 32);
        r0 += r1;
        const uint64_t k = (r0 + (1ULL << 61)) >> 62;
        r0 -= k << 62;
        x = (double)(int64_t)r0 * 0x1.921FB54442D18p-62;
        n = (int)k;
        q = n + (int)(xi >> 31);
    } else return y - y;
    const double s = ((q ^ (q >> 1)) & 1) ? -1.0 : 1.0;
    return sincos_poly(x * s, x * x, (q & 2) ? -1.0 : 1.0, n ^ shift);
}

static int f2i(float v) { int i; memcpy(&i, &v, 4); return i; }
static float o_atanf(float x)
{
    static const float hi[4] = { 4.6364760399e-01f, 7.8539812565e-01f, 9.8279368877e-01f, 1.5707962513e+00f };
    static const float lo[4] = { 5.0121582440e-09f, 3.7748947079e-08f, 3.4473217170e-08f, 7.5497894159e-08f };
    const float t0 = 3.3333334327e-01f, t1 = -2.0000000298e-01f, t2 = 1.4285714924e-01f, t3 = -1.1111110449e-01f, t4 = 9.0908870101e-02f,
                t5 = -7.6918758452e-02f, t6 = 6.6610731184e-02f, t7 = -5.8335702866e-02f, t8 = 4.9768779427e-02f, t9 = -3.6531571299e-02f,
                t10 = 1.6285819933e-02f;
    const int hx = f2i(x), ix = hx & 0x7fffffff;
    int id = -1;
    if (ix >= 0x4c000000) {
        if (ix > 0x7f800000) return x + x;
        return hx > 0 ? hi[3] + lo[3] : -hi[3] - lo[3];
    }
    if (ix < 0x3ee00000) {
        if (ix < 0x31000000) return x;
    } else {
        x = fabsf(x);
        if (ix < 0x3f980000) {
            if (ix < 0x3f300000) { id = 0; x = (2.0f * x - 1.0f) / (2.0f + x); }
            else { id = 1; x = (x - 1.0f) / (x + 1.0f); }
        } else {
            if (ix < 0x401c0000) { id = 2; x = (x - 1.5f) / (1.0f + 1.5f * x); }
            else { id = 3; x = -1.0f / x; }
        }
    }
    const float z = x * x, w = z * z;
    const float s1 = z * (t0 + w * (t2 + w * (t4 + w * (t6 + w * (t8 + w * t10)))));
    const float s2 = w * (t1 + w * (t3 + w * (t5 + w * (t7 + w * t9))));
    if (id < 0) return x - x * (s1 + s2);
    const float r = hi[id] - ((x * (s1 + s2) - lo[id]) - x);
    return hx < 0 ? -r : r;
}
static float o_atan2f(float y, float x)
{
    const float tiny = 1.0e-30f, pi_o_4 = 7.8539818525e-01f, pi_o_2 = 1.5707963705e+00f, pi = 3.1415927410e+00f, pi_lo = -8.7422776573e-08f;
    const int hx = f2i(x), ix = hx & 0x7fffffff, hy = f2i(y), iy = hy & 0x7fffffff;
    if (ix > 0x7f800000 || iy > 0x7f800000) return x + y;
    if (hx == 0x3f800000) return o_atanf(y);
    const int m = ((hy >> 31) & 1) | ((hx >> 30) & 2);
    if (iy == 0) return m < 2 ? y : (m == 2 ? pi + tiny : -pi - tiny);
    if (ix == 0) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
    if (ix == 0x7f800000) {
        if (iy == 0x7f800000) return m == 0 ? pi_o_4 + tiny : (m == 1 ? -pi_o_4 - tiny : (m == 2 ? 3.0f * pi_o_4 + tiny : -3.0f * pi_o_4 - tiny));
        return m == 0 ? 0.0f : (m == 1 ? -0.0f : (m == 2 ? pi + tiny : -pi - tiny));
    }
    if (iy == 0x7f800000) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
    const int k = (iy - ix) >> 23;
    float z;
    if (k > 60) z = pi_o_2 + 0.5f * pi_lo;
    else if (hx < 0 && k < -60) z = 0.0f;
    else z = o_atanf(fabsf(y / x));
    return m == 0 ? z : (m == 1 ? -z : (m == 2 ? pi - (z - pi_lo) : (z - pi_lo) - pi));
}

/* ---------------------------------------------------------------- the two loops */
#define O_PI 3.14159265358979323846
#define O_TURNS_MAX 65536        /* the reference's loops do not end on an infinite angle */

typedef struct {
    /* PhaseLockComplex */
    float a1, a2, b0, b1, b2, v0, v1, v2, dphi, phi_hat, phi_prev, y_re, y_im, freq, freq_prev, freq_test, lock_freq, ea_y1;
    int lock_count, lock_time, lock_time_count; unsigned order;
    /* FreqLockComplex */
    float f_a0, f_a1, f_y_re, f_y_im, f_phi, f_phix0, f_phix1, f_y1;
    long probe[8];
} loops;

static float normalize_angle(float angle, int* turns)
{
    int t = 0;
    while (angle <= -O_PI && t < O_TURNS_MAX) { angle += 2.0 * O_PI; t++; }
    while (angle > O_PI && t < O_TURNS_MAX) { angle -= 2.0 * O_PI; t++; }
    if (turns) *turns = t;
    return angle;
}

static void pll_compute_coefficients(loops* l, float wn, float zeta, float K)
{
    double t1 = K / (wn * wn);
    double t2 = 2 * zeta / wn - 1 / K;
    double b0 = 2 * K * (1. + t2 / 2.0f), b1 = 2 * K * 2., b2 = 2 * K * (1. - t2 / 2.0f);
    double a0 = 1 + t1 / 2.0f, a1 = -t1, a2 = -1 + t1 / 2.0f;
    l->b0 = b0 / a0; l->b1 = b1 / a0; l->b2 = b2 / a0;
    l->a1 = a1 / a0; l->a2 = a2 / a0;
}
static void set_sample_rate(loops* l, unsigned rate)
{
    l->lock_time = rate / 100;
    l->lock_freq = (2.0 * O_PI * (l->order > 1 ? 6.0 : 1.0)) / rate;
    l->f_a1 = 10.0f / rate;
    l->f_a0 = 1.0f - l->f_a1;
}

static void pll_feed(loops* l, float re, float im)
{
    if (top12(l->phi_hat) >= top12(120.0f)) l->probe[5]++;
    l->y_re = o_sincosf(l->phi_hat, 1);
    l->y_im = o_sincosf(l->phi_hat, 0);
    /* x * std::conj(m_y) */
    const float cr = l->y_re, ci = -l->y_im;
    const float pr = re * cr - im * ci, pi = re * ci + im * cr;
    if (pr == 0.0f && pi == 0.0f) l->probe[6]++;
    l->dphi = o_atan2f(pi, pr);
    if (l->order > 1) {
        int t;
        l->dphi = normalize_angle(l->order * l->dphi, &t);
        if (t > 1) l->probe[2]++;
    }
    l->v2 = l->v1;
    l->v1 = l->v0;
    l->v0 = l->dphi - l->v1 * l->a1 - l->v2 * l->a2;
    l->phi_hat = l->v0 * l->b0 + l->v1 * l->b1 + l->v2 * l->b2;
    if (l->phi_hat > 2.0 * O_PI) {
        l->v0 *= (l->phi_hat - 2.0 * O_PI) / l->phi_hat;
        l->v1 *= (l->phi_hat - 2.0 * O_PI) / l->phi_hat;
        l->v2 *= (l->phi_hat - 2.0 * O_PI) / l->phi_hat;
        l->phi_hat -= 2.0 * O_PI;
        l->probe[0]++;
    }
    if (l->phi_hat < -2.0 * O_PI) {
        l->v0 *= (l->phi_hat + 2.0 * O_PI) / l->phi_hat;
        l->v1 *= (l->phi_hat + 2.0 * O_PI) / l->phi_hat;
        l->v2 *= (l->phi_hat + 2.0 * O_PI) / l->phi_hat;
        l->phi_hat += 2.0 * O_PI;
        l->probe[1]++;
    }
    const float ea_a0 = 0.999, ea_a1 = 0.001;
    if (l->order > 1) {
        float dPhi = normalize_angle(l->phi_hat - l->phi_prev, 0);
        l->freq = l->ea_y1 = ea_a1 * dPhi + ea_a0 * l->ea_y1;
        if (l->lock_time_count < l->lock_time - 1) l->lock_time_count++;
        else {
            float dF = l->freq - l->freq_test;
            if ((dF > -l->lock_freq) && (dF < l->lock_freq)) { if (l->lock_count < 20) { l->lock_count++; l->probe[3]++; } }
            else { if (l->lock_count > 0) { l->lock_count--; l->probe[4]++; } }
            l->freq_test = l->freq;
            l->lock_time_count = 0;
        }
        l->phi_prev = l->phi_hat;
    } else {
        l->freq_test = normalize_angle(l->phi_hat - l->phi_prev, 0);
        l->freq = l->ea_y1 = ea_a1 * l->freq_test + ea_a0 * l->ea_y1;
        float dFreq = l->freq_test - l->freq_prev;
        if ((dFreq > -0.01) && (dFreq < 0.01)) { if (l->lock_count < (l->lock_time - 1)) { l->lock_count++; l->probe[3]++; } }
        else { if (l->lock_count > 0) l->probe[4]++; l->lock_count = 0; }
        l->phi_prev = l->phi_hat;
        l->freq_prev = l->freq_test;
    }
}

static void fll_feed(loops* l, float re, float im)
{
    if (top12(l->f_phi) >= top12(120.0f)) l->probe[5]++;
    l->f_y_re = o_sincosf(l->f_phi, 1);
    l->f_y_im = o_sincosf(l->f_phi, 0);
    if (re == 0.0f && im == 0.0f) l->probe[6]++;
    l->f_phix0 = o_atan2f(im, re);
    float eF = normalize_angle(l->f_phix0 - l->f_phix1, 0);
    float fHat = l->f_a1 * eF + l->f_a0 * l->f_y1;
    l->f_y1 = fHat;
    l->f_phi += fHat;
    l->f_phix1 = l->f_phix0;
}

#endif
