// The arithmetic of the stereo pilot loop of BFMDemod for the host and the device: PhaseLock::process(const Real&, Real*) with
// process_phasor (sdrbase/dsp/phaselock.cpp:253-367) and RDSPhaseLock::processPhase (phaselock.h:171-180), one step in the
// reference's operand order and float / double promotions, PhaseLock::configure (phaselock.cpp:86-143) and LowPassFilterRC
// (filterrc.cpp:31-56).  sin / cos of the float phase are sinf / cosf: pll_sinf / pll_cosf (pll_math.hpp).  Compiles for the host
// too (tests/bfm_pll_check.cpp), no HIP header needed.
#pragma once
#include "pll_math.hpp"

namespace sdrx {

struct BfmPllCfg {
    float minfreq, maxfreq;                 // m_minfreq, m_maxfreq
    float b0, a1, a2;                       // m_phasor_b0, m_phasor_a1, m_phasor_a2
    float lf_b0, lf_b1;                     // m_loopfilter_b0, m_loopfilter_b1
    float minsignal;                        // m_minsignal
    int lock_delay;                         // m_lock_delay
};

struct BfmPllState {
    float phase, freq;                      // m_phase, m_freq
    float i1, i2, q1, q2;                   // m_phasor_i1 .. m_phasor_q2
    float x1;                               // m_loopfilter_x1
    float level;                            // m_pilot_level
    int lock_cnt, periods;                  // m_lock_cnt, m_pilot_periods
};

struct BfmPllProbe {                        // the branches a step went through
    long ratio, plus, minus, clamp_lo, clamp_hi, wrap, lock_up, lock_reset;
};

// one sample; returns m_psin and m_pcos, what processPhase makes its outputs from
template <class Probe>
AM_HD void bfm_pll_step(const BfmPllCfg& k, BfmPllState& s, float x, float* psin, float* pcos, Probe* pr)
{
    const double two_pi = 2.0 * 3.14159265358979323846;
    const float sn = pll_sinf(s.phase), cs = pll_cosf(s.phase);
    *psin = sn; *pcos = cs;
    float pi_ = sn * x, pq = cs * x;
    pi_ = k.b0 * pi_ - k.a1 * s.i1 - k.a2 * s.i2;
    pq = k.b0 * pq - k.a1 * s.q1 - k.a2 * s.q2;
    s.i2 = s.i1; s.i1 = pi_;
    s.q2 = s.q1; s.q1 = pq;
    float err;
    if (pi_ > __builtin_fabsf(pq)) { err = pq / pi_; if (pr) pr->ratio++; }
    else if (pq > 0) { err = 1; if (pr) pr->plus++; }
    else { err = -1; if (pr) pr->minus++; }
    s.level = pi_;
    s.freq += k.lf_b0 * err + k.lf_b1 * s.x1;
    s.x1 = err;
    // std::max(m_minfreq, std::min(m_maxfreq, m_freq))
    if (pr && s.freq < k.minfreq) pr->clamp_lo++;
    if (pr && k.maxfreq < s.freq) pr->clamp_hi++;
    const float lim = s.freq < k.maxfreq ? s.freq : k.maxfreq;
    s.freq = k.minfreq < lim ? lim : k.minfreq;
    s.phase += s.freq;
    if ((double)s.phase > two_pi) {
        s.phase = (float)((double)s.phase - two_pi);
        s.periods++;
        if (s.periods == 19000) s.periods = 0;              // pilot_frequency
        if (pr) pr->wrap++;
    }
    if (2 * s.level > k.minsignal) { if (s.lock_cnt < k.lock_delay) { s.lock_cnt += 1; if (pr) pr->lock_up++; } }
    else { if (pr && s.lock_cnt > 0) pr->lock_reset++; s.lock_cnt = 0; }
    if (s.lock_cnt < k.lock_delay) s.periods = 0;
}

// RDSPhaseLock::processPhase: samples_out[1] and samples_out[2]
AM_HD float bfm_pilot_sin2(float psin, float pcos) { return (float)(2.0 * (double)psin * (double)pcos); }
AM_HD float bfm_pilot_cos2(float pcos) { return (float)((2.0 * (double)pcos * (double)pcos) - 1.0); }

AM_HD bool bfm_pll_locked(const BfmPllCfg& k, const BfmPllState& s) { return s.lock_cnt >= k.lock_delay; }

// LowPassFilterRC::process
AM_HD float bfm_rc_step(float x, float b0, float a1, float* y1) { *y1 = (x * b0) - (*y1 * a1); return *y1; }

// PhaseLock::configure(freq, bandwidth, minsignal): the Real arguments are what the caller's doubles convert to
inline void bfm_pll_design(double freq_d, double bandwidth_d, double minsignal_d, BfmPllCfg* k, BfmPllState* s)
{
    const double pi = 3.14159265358979323846;
    const float freq = (float)freq_d, bandwidth = (float)bandwidth_d;
    k->minfreq = (float)((freq - bandwidth) * 2.0 * pi);
    k->maxfreq = (float)((freq + bandwidth) * 2.0 * pi);
    k->minsignal = (float)minsignal_d;
    k->lock_delay = (int)(20.0 / bandwidth);
    const double p1 = __builtin_exp(-1.146 * bandwidth * 2.0 * pi);
    const double p2 = __builtin_exp(-5.331 * bandwidth * 2.0 * pi);
    k->a1 = (float)(-p1 - p2);
    k->a2 = (float)(p1 * p2);
    k->b0 = 1 + k->a1 + k->a2;
    const double q1 = __builtin_exp(-0.1153 * bandwidth * 2.0 * pi);
    k->lf_b0 = (float)(0.62 * bandwidth * 2.0 * pi);
    k->lf_b1 = (float)(-k->lf_b0 * q1);
    *s = BfmPllState();
    s->freq = (float)(freq * 2.0 * pi);
}

// LowPassFilterRC::configure(timeconst)
inline void bfm_rc_design(double timeconst_d, float* b0, float* a1)
{
    const float timeconst = (float)timeconst_d;
    *a1 = (float)(-__builtin_exp(-1 / timeconst));
    *b0 = 1 + *a1;
}

} // namespace sdrx
