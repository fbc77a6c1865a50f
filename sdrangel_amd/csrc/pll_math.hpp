// The arithmetic of PhaseLockComplex::feed (sdrbase/dsp/phaselockcomplex.cpp:119-225) and FreqLockComplex::feed
// (freqlockcomplex.cpp:64-91) for the host and the device: one step of either loop in the reference's operand order and
// float / double promotions, and the libm routines a step calls.  Compiles for the host too (tests/pll_math_check.cpp), no
// HIP header needed.
//
// cos / sin of a float are cosf / sinf (GCC folds the pair into sincosf, which is the same routine).  pll_sinf / pll_cosf are
// glibc's from 2.28 on (sysdeps/ieee754/flt-32/s_sinf.c, s_cosf.c, sincosf.h: double inside, rounded once), the build an
// x86-64 CPU with FMA is given by the ifunc: every a + b * c there is one fused operation, written out here since this
// project compiles with contraction off.  They return that libm's bits (tests/test_pll_math.py), which inside a feedback loop
// is the only agreement that means anything.  std::arg is udp_atan2f (udpsrc_scan.hpp), unchanged.
#pragma once
#include <stdint.h>
#include "udpsrc_scan.hpp"

namespace sdrx {

AM_HD uint32_t pll_bits(float v) { uint32_t i; __builtin_memcpy(&i, &v, 4); return i; }
AM_HD uint32_t pll_top12(float v) { return (pll_bits(v) >> 20) & 0x7ff; }

// sinf_poly: the sine polynomial on even n, the cosine's on odd n; cs is -1 where the second table (c0 .. c4 negated) is in use
AM_HD float pll_sincos_poly(double x, double x2, double cs, int n)
{
    const double c0 = 0x1p0, c1 = -0x1.ffffffd0c621cp-2, c2 = 0x1.55553e1068f19p-5, c3 = -0x1.6c087e89a359dp-10, c4 = 0x1.99343027bf8c3p-16;
    const double s1 = -0x1.555545995a603p-3, s2 = 0x1.1107605230bc4p-7, s3 = -0x1.994eb3774cf24p-13;
    if ((n & 1) == 0) {
        const double x3 = x * x2;
        const double t1 = __builtin_fma(x2, s3, s2);
        const double x7 = x3 * x2;
        const double s = __builtin_fma(x3, s1, x);
        return (float)__builtin_fma(x7, t1, s);
    }
    const double x4 = x2 * x2;
    const double t2 = __builtin_fma(x2, cs * c4, cs * c3);
    const double t1 = __builtin_fma(x2, cs * c1, cs * c0);
    const double x6 = x4 * x2;
    const double c = __builtin_fma(x4, cs * c2, t1);
    return (float)__builtin_fma(x6, t2, c);
}

// reduce_large: |y| >= 120, finite.  The bits of 4 / pi, one byte apart
AM_HD double pll_reduce_large(uint32_t xi, int* np)
{
    const uint32_t inv_pio4[24] = { 0xa2, 0xa2f9, 0xa2f983, 0xa2f9836e, 0xf9836e4e, 0x836e4e44, 0x6e4e4415, 0x4e441529,
                                    0x441529fc, 0x1529fc27, 0x29fc2757, 0xfc2757d1, 0x2757d1f5, 0x57d1f534, 0xd1f534dd, 0xf534ddc0,
                                    0x34ddc0db, 0xddc0db62, 0xc0db6295, 0xdb629599, 0x6295993c, 0x95993c43, 0x993c4390, 0x3c439041 };
    const int at = (int)((xi >> 26) & 15), shift = (int)((xi >> 23) & 7);
    const uint32_t m = ((xi & 0xffffff) | 0x800000) << shift;
    uint64_t r0 = (uint32_t)(m * inv_pio4[at]);
    const uint64_t r1 = (uint64_t)m * inv_pio4[at + 4], r2 = (uint64_t)m * inv_pio4[at + 8];
    r0 = (r2 >> 32) | (r0 << 32);
    r0 += r1;
    const uint64_t n = (r0 + (1ULL << 61)) >> 62;
    r0 -= n << 62;
    *np = (int)n;
    return (double)(int64_t)r0 * 0x1.921FB54442D18p-62;
}

// both routines: shift is 0 for the sine, 1 for the cosine (sinf_poly(..., n ^ 1))
AM_HD float pll_sincosf(float y, int shift)
{
    const double hpi_inv = 0x1.45F306DC9C883p+23, hpi = 0x1.921FB54442D18p0;
    double x = (double)y;
    if (pll_top12(y) < pll_top12(0x1.921FB6p-1f)) {
        if (pll_top12(y) < pll_top12(0x1p-12f)) return shift ? 1.0f : y;
        return pll_sincos_poly(x, x * x, 1.0, shift);
    }
    int n, q;
    if (pll_top12(y) < pll_top12(120.0f)) {
        const double r = x * hpi_inv;
        n = ((int32_t)r + 0x800000) >> 24;
        x = __builtin_fma(-(double)n, hpi, x);
        q = n;
    } else if (pll_top12(y) < pll_top12(__builtin_inff())) {
        const uint32_t xi = pll_bits(y);
        x = pll_reduce_large(xi, &n);
        q = n + (int)(xi >> 31);
    } else return y - y;
    const double s = ((q ^ (q >> 1)) & 1) ? -1.0 : 1.0;             // sign[q & 3] = { 1, -1, -1, 1 }
    return pll_sincos_poly(x * s, x * x, (q & 2) ? -1.0 : 1.0, n ^ shift);
}
AM_HD float pll_sinf(float y) { return pll_sincosf(y, 0); }
AM_HD float pll_cosf(float y) { return pll_sincosf(y, 1); }

// normalizeAngle of either class: a float compared and moved in double.  The reference's loops do not end on an infinite
// angle; this one gives up after PLL_TURNS_MAX turns, far beyond what any finite input reaches
constexpr int PLL_TURNS_MAX = 1 << 16;
AM_HD float pll_normalize(float angle, int* turns)
{
    const double pi = 3.14159265358979323846;
    int t = 0;
    while ((double)angle <= -pi && t < PLL_TURNS_MAX) { angle = (float)((double)angle + 2.0 * pi); t++; }
    while ((double)angle > pi && t < PLL_TURNS_MAX) { angle = (float)((double)angle - 2.0 * pi); t++; }
    if (turns) *turns = t;
    return angle;
}

enum { PLL_OFF = 0, PLL_PHASE = 1, PLL_FREQ = 2 };

struct PllCfg {
    int mode;                               // PLL_OFF: m_pll clear; PLL_PHASE: m_pll; PLL_FREQ: m_pll and m_fll
    unsigned order;                         // m_pskOrder
    int lock_time;                          // m_lockTime
    float lock_freq;                        // m_lockFreq
    float a1, a2, b0, b1, b2;               // computeCoefficients(0.002f, 0.5f, 10.0f)
    float f_a0, f_a1;                       // FreqLockComplex's m_a0, m_a1
};

struct PllState {
    float v0, v1, v2, dphi, phi_hat, phi_prev, freq, freq_prev, freq_test;
    float ea_y1;                            // m_expAvg's m_y1
    int lock_count, lock_time_count;
    float f_phi, f_phix1, f_y1;             // FreqLockComplex: m_phi, m_phiX1, m_y1 (m_freq is m_y1)
};

struct PllProbe {                           // what a step went through, for the tests that name their cases after it
    long sat_hi, sat_lo, turns_many, lock_up, lock_down, big_arg, arg_zero;
};

// PhaseLockComplex::feed; returns m_y = (cos, sin) of the phase before the step
template <class Probe>
AM_HD void pll_phase_step(const PllCfg& k, PllState& s, float re, float im, float* y_re, float* y_im, Probe* pr)
{
    const double two_pi = 2.0 * 3.14159265358979323846;
    const float yr = pll_cosf(s.phi_hat), yi = pll_sinf(s.phi_hat);
    *y_re = yr; *y_im = yi;
    // x * std::conj(m_y)
    const float cj = -yi;
    const float pr_ = re * yr - im * cj, pi_ = re * cj + im * yr;
    if (pr && pr_ == 0.0f && pi_ == 0.0f) pr->arg_zero++;
    s.dphi = udp_atan2f(pi_, pr_);
    if (k.order > 1) {
        int t;
        s.dphi = pll_normalize((float)k.order * s.dphi, &t);
        if (pr && t > 1) pr->turns_many++;
    }
    s.v2 = s.v1;
    s.v1 = s.v0;
    s.v0 = s.dphi - s.v1 * k.a1 - s.v2 * k.a2;
    s.phi_hat = s.v0 * k.b0 + s.v1 * k.b1 + s.v2 * k.b2;
    if ((double)s.phi_hat > two_pi) {
        const double f = ((double)s.phi_hat - two_pi) / (double)s.phi_hat;
        s.v0 = (float)((double)s.v0 * f); s.v1 = (float)((double)s.v1 * f); s.v2 = (float)((double)s.v2 * f);
        s.phi_hat = (float)((double)s.phi_hat - two_pi);
        if (pr) pr->sat_hi++;
    }
    if ((double)s.phi_hat < -two_pi) {
        const double f = ((double)s.phi_hat + two_pi) / (double)s.phi_hat;
        s.v0 = (float)((double)s.v0 * f); s.v1 = (float)((double)s.v1 * f); s.v2 = (float)((double)s.v2 * f);
        s.phi_hat = (float)((double)s.phi_hat + two_pi);
        if (pr) pr->sat_lo++;
    }
    const float ea_a0 = 0.999f, ea_a1 = 0.001f;             // ExpAvg() : m_a0(0.999), m_a1(0.001)
    if (k.order > 1) {
        const float d = pll_normalize(s.phi_hat - s.phi_prev, nullptr);
        s.freq = s.ea_y1 = ea_a1 * d + ea_a0 * s.ea_y1;
        if (s.lock_time_count < k.lock_time - 1) s.lock_time_count++;
        else {
            const float df = s.freq - s.freq_test;
            if (df > -k.lock_freq && df < k.lock_freq) { if (s.lock_count < 20) { s.lock_count++; if (pr) pr->lock_up++; } }
            else if (s.lock_count > 0) { s.lock_count--; if (pr) pr->lock_down++; }
            s.freq_test = s.freq;
            s.lock_time_count = 0;
        }
        s.phi_prev = s.phi_hat;
    } else {
        s.freq_test = pll_normalize(s.phi_hat - s.phi_prev, nullptr);
        s.freq = s.ea_y1 = ea_a1 * s.freq_test + ea_a0 * s.ea_y1;
        const float df = s.freq_test - s.freq_prev;
        if ((double)df > -0.01 && (double)df < 0.01) { if (s.lock_count < k.lock_time - 1) { s.lock_count++; if (pr) pr->lock_up++; } }
        else { if (pr && s.lock_count > 0) pr->lock_down++; s.lock_count = 0; }
        s.phi_prev = s.phi_hat;
        s.freq_prev = s.freq_test;
    }
}

// FreqLockComplex::feed
template <class Probe>
AM_HD void pll_freq_step(const PllCfg& k, PllState& s, float re, float im, float* y_re, float* y_im, Probe* pr)
{
    if (pr && pll_top12(s.f_phi) >= pll_top12(120.0f)) pr->big_arg++;
    *y_re = pll_cosf(s.f_phi); *y_im = pll_sinf(s.f_phi);
    const float x0 = udp_atan2f(im, re);
    if (pr && re == 0.0f && im == 0.0f) pr->arg_zero++;
    const float ef = pll_normalize(x0 - s.f_phix1, nullptr);
    const float fhat = k.f_a1 * ef + k.f_a0 * s.f_y1;
    s.f_y1 = fhat;
    s.f_phi += fhat;
    s.f_phix1 = x0;
}

// locked(): isPllLocked is this and m_settings.m_pll
AM_HD bool pll_locked(const PllCfg& k, const PllState& s) { return k.order > 1 ? s.lock_count > 10 : s.lock_count > k.lock_time - 2; }

// ---- the configuration sequence, replayed call for call (host)
struct PllDesign {
    PllCfg k;
    void coefficients(float wn, float zeta, float K)        // PhaseLockComplex::computeCoefficients
    {
        const double t1 = K / (wn * wn);
        const double t2 = 2 * zeta / wn - 1 / K;
        const double b0 = 2 * K * (1. + t2 / 2.0f), b1 = 2 * K * 2., b2 = 2 * K * (1. - t2 / 2.0f);
        const double a0 = 1 + t1 / 2.0f, a1 = -t1, a2 = -1 + t1 / 2.0f;
        k.b0 = (float)(b0 / a0); k.b1 = (float)(b1 / a0); k.b2 = (float)(b2 / a0);
        k.a1 = (float)(a1 / a0); k.a2 = (float)(a2 / a0);
    }
    void sample_rate(unsigned rate)                         // both classes' setSampleRate
    {
        k.lock_time = (int)(rate / 100);
        k.lock_freq = (float)((2.0 * 3.14159265358979323846 * (k.order > 1 ? 6.0 : 1.0)) / rate);
        k.f_a1 = 10.0f / rate;
        k.f_a0 = 1.0f - k.f_a1;
    }
    void psk_order(unsigned order) { k.order = order > 0 ? order : 1; }
};

// The object after the constructor, applySettings(settings, true), applyChannelSettings(in_rate, offset) and start()
// (chanalyzer.cpp:35-65, 247-392): every setSampleRate and setPskOrder in the order they run.  applySettings' own call
// (:363) divides by the span of the settings before (the defaults': 0), and setPskOrder comes after it, so only a channel
// without the Interpolator, whose applyChannelSettings calls setSampleRate once more, sees its own span and order there.
inline PllCfg pll_design(int in_rate, bool down_sample, unsigned down_sample_rate, int span_log2, bool pll, bool fll, unsigned order)
{
    PllDesign d;
    d.k = PllCfg();
    // the constructor: members, computeCoefficients, applyChannelSettings(48000, 0, true), applySettings(defaults, true)
    d.k.order = 1; d.k.lock_time = 480; d.k.lock_freq = 0.026f; d.k.f_a0 = (float)0.998; d.k.f_a1 = (float)0.002;
    d.coefficients(0.002f, 0.5f, 10.0f);
    d.sample_rate((unsigned)(48000 / (1 << 0)));
    d.sample_rate((unsigned)(48000 / (1 << 0)));
    d.sample_rate((unsigned)(48000 / (1 << 0)));
    d.psk_order(1);
    // applySettings(settings, true); m_inputSampleRate is still 48000, m_settings the defaults
    const int rate = down_sample ? (int)down_sample_rate : 48000;
    d.sample_rate((unsigned)(rate / (1 << span_log2)));
    d.sample_rate((unsigned)((int)(down_sample ? down_sample_rate : 48000u) / (1 << 0)));
    if (order < 32) d.psk_order(order);
    // applyChannelSettings(in_rate, offset), then start()'s forced one
    if (!down_sample) {
        if (in_rate != 48000) d.sample_rate((unsigned)(in_rate / (1 << span_log2)));
        d.sample_rate((unsigned)(in_rate / (1 << span_log2)));
    }
    d.k.mode = pll ? (fll ? PLL_FREQ : PLL_PHASE) : PLL_OFF;
    return d.k;
}

} // namespace sdrx
