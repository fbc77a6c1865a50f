// The synchronous-AM chain of AMDemod::processOneSample (plugins/channelrx/demodam/amdemod.cpp:191-238, m_pll set) cut into
// terms that can be computed in parallel, and the index arithmetic that goes with them.  Stream indexing (am_stream_at /
// am_hist_next) is am_scan.hpp's.  Compiles for the host too (tests/am_sync_check.cpp), no HIP header needed; a complex value
// is any type with float members x and y.
//
// The whole chain runs on open, unmuted samples only, so every stream below is indexed in the compacted sequence of open
// samples (am_gate_kernel's aidx), K = open samples since creation.
// 1. m_pllFilt, Lowpass<std::complex<float>> with 101 taps: X(k) = the (re, im) k open samples back; the ring walk pairs the
//    new sample with the one before it, then the oldest with the next one back, and so on (ams_prefilter, as am_bandpass).
// 2. m_pll.feed(): one dependent chain per channel, pll_phase_step (pll_math.hpp) with order 1.
// 3. The UNfiltered sample turned by (m_yIm, m_yRe) (ams_rotate) goes into fftfilt runDSB / runSSB with getDC = false: blocks
//    of B = flen / 2 inputs (DSB 1024, SSB 512), block m made of open samples m * B .. m * B + B - 1 and complete on the last
//    of them.  A feed that starts `pend` samples into a block finds element j of its block x at compacted index
//    x * B + j - pend; negative ones were carried (ams_block_source).
// 4. m_syncAMAGC, MagAGC with the threshold off: per filter output magsq = re * re + im * im in float, the MovingAverage<double>
//    of hn = rate / 4 entries `sum += magsq[o] - magsq[o - hn]`, history 0: a rounded prefix sum of terms known in advance
//    (ams_agc_term, psum_rows); m_u0 = R / sqrt(sum / hn), pointwise (ams_u0); zsum = z.re + z.im with z = sb * (float) m_u0.
// 5. m_syncAMBuff / m_syncAMBuffIndex: a fill on every B-th open sample resets the index to 0 before the read, so open sample K
//    reads zsum[K + 1 - B] (and 0.0f, what the array is pinned to, while that is negative): ams_select_index gives the place
//    relative to the first filter output of this feed.
#pragma once
#include <cmath>
#include "am_scan.hpp"
#include "pll_math.hpp"

namespace sdrx {

constexpr int AMS_PF_TAPS = 101, AMS_PF_H = 50;            // m_pllFilt.create(101, rate, 200.0), folded to 51
constexpr int AMS_PF_HIST = AMS_PF_TAPS - 1;               // ring entries older than the current sample
constexpr int AMS_DSB_FLEN = 2048, AMS_SSB_FLEN = 1024;    // DSBFilter, SSBFilter
constexpr int AMS_BLOCK_MAX = AMS_DSB_FLEN / 2;
enum { AMS_OFF = 0, AMS_DSB = 1, AMS_USB = 2, AMS_LSB = 3 };   // AmChan::sync: sync_op + 1 where m_pll is set

AM_HD int ams_flen(int sync) { return sync == AMS_DSB ? AMS_DSB_FLEN : AMS_SSB_FLEN; }
AM_HD int ams_block(int sync) { return ams_flen(sync) / 2; }
AM_HD int ams_agc_len(int rate) { return rate / 4; }       // m_syncAMAGC.resize(rate / 4, rate / 8, 0.1)
AM_HD double ams_agc_target() { return (double)(float)0.1; }   // resize(int, int, Real R)

// Lowpass<std::complex<float>>::filter (lowpass.h:55-100): (m_samples[a] + m_samples[b]) * m_taps[i] accumulated in complex<float>
template <class C, class F> AM_HD C ams_prefilter(const float* taps, F X)
{
    C acc; acc.x = 0.0f; acc.y = 0.0f;
    const C x0 = X(0), x1 = X(1);
    acc.x += (x0.x + x1.x) * taps[0]; acc.y += (x0.y + x1.y) * taps[0];
    for (int i = 1; i < AMS_PF_H; i++) {
        const C a = X(AMS_PF_TAPS - i), b = X(1 + i);
        acc.x += (a.x + b.x) * taps[i]; acc.y += (a.y + b.y) * taps[i];
    }
    const C m = X(AMS_PF_H + 1);
    acc.x += m.x * taps[AMS_PF_H]; acc.y += m.y * taps[AMS_PF_H];
    return acc;
}

// yr = re * m_pll.getImag() - im * m_pll.getReal();  yi = re * m_pll.getReal() + im * m_pll.getImag()
template <class C> AM_HD C ams_rotate(C v, C osc)
{
    C r;
    r.x = v.x * osc.y - v.y * osc.x;
    r.y = v.x * osc.x + v.y * osc.y;
    return r;
}

AM_HD int ams_blocks(int pend, int n_act, int B) { return (pend + n_act) / B; }
AM_HD int ams_left(int pend, int n_act, int B) { return (pend + n_act) % B; }
// element j of block x of this feed: its index in the feed's compacted sequence; q < 0 is carried element pend + q
AM_HD int ams_block_source(int pend, int B, int x, int j) { return x * B + j - pend; }

template <class C> AM_HD float ams_magsq(C sb) { return sb.x * sb.x + sb.y * sb.y; }        // MagAGC::feedAndGetValue: in Real
AM_HD double ams_agc_term(float p, float old_hn) { return (double)p - (double)old_hn; }
AM_HD double ams_u0(double sum, int hn) { return ams_agc_target() / __builtin_sqrt(sum / (double)hn); }
// float agcVal = feedAndGetValue(sb);  z = sb * agcVal;  m_syncAMBuff[i] = z.real() + z.imag()
template <class C> AM_HD float ams_zsum(C sb, double u0)
{
    const float a = (float)u0;
    return sb.x * a + sb.y * a;
}

// open sample a of a feed that began `pend` samples into a block reads filter output ams_select_index of this feed; a negative
// one is that far back in the outputs of earlier feeds (never more than B - 1)
AM_HD int ams_select_index(int pend, int a, int B) { return pend + a + 1 - B; }

// ---- design (host)
// Lowpass<>::create(101, rate, 200.0) (lowpass.h:15-53): the folded 51 taps.  The arithmetic of ct_lowpass_design
// (nfm_tone_scan.hpp) with the tap count as an argument
inline void ams_lowpass_design(double rate, double cutoff, float* t)
{
    const double PI = 3.14159265358979323846;
    const int ntaps = AMS_PF_TAPS, nt = AMS_PF_H + 1;
    const double mid = ((double)ntaps - 1.0) / 2.0;
    const double Wc = (2.0 * PI * cutoff) / rate;
    for (int i = 0; i < nt; i++)
        t[i] = (i == (ntaps - 1) / 2) ? (float)(Wc / PI) : (float)(std::sin(((double)i - mid) * Wc) / (((double)i - mid) * PI));
    for (int i = 0; i < nt; i++) t[i] = (float)(t[i] * (0.54 + 0.46 * std::cos((2.0 * PI * ((double)i - mid)) / (double)ntaps)));
    float sum = 0; int i;
    for (i = 0; i < nt - 1; i++) sum += t[i] * 2;
    sum += t[i];
    for (i = 0; i < nt; i++) t[i] /= sum;
}

// m_pll after the constructor and applyAudioSampleRate: computeCoefficients(0.05, 0.707, 1000), setSampleRate(rate), order 1
inline PllCfg ams_pll_design(int rate)
{
    PllDesign d;
    d.k = PllCfg();
    d.k.order = 1; d.k.f_a0 = (float)0.998; d.k.f_a1 = (float)0.002;
    d.coefficients(0.05f, 0.707f, 1000.0f);
    d.sample_rate((unsigned)rate);
    d.k.mode = PLL_PHASE;
    return d.k;
}

} // namespace sdrx
