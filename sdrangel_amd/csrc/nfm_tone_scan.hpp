// The CTCSS branch of NFMDemod::feed (plugins/channelrx/demodnfm/nfmdemod.cpp:235-296, m_ctcssOn) cut into terms that can be
// computed in parallel, on top of nfm_scan.hpp's; and, further down, the AF squelch (m_deltaSquelch) as the containers it walks.  Compiles for the host too (tests/nfm_tone_scan_check.cpp).
//
// Per audio sample, after the squelch counter (nfm_scan.hpp 1-3), unmuted:
//   open:   ctcss_sample = m_lowpass.filter(demod * comp)                       every open sample advances the Lowpass ring
//           if ((m_sampleCount & 7) == 7 && m_ctcssDetector.analyze(&ctcss_sample))
//               m_ctcssIndex = toneDetected ? maxPowerIndex + 1 : 0
//           if (selected && selected != m_ctcssIndex) sample = 0                the Bandpass does not advance
//           else sample = (qint16)(m_bandpass.filter(readBack(gate)) * volume)
//   closed: m_ctcssIndex = 0
// m_sampleCount counts every audio sample, muted ones too; a muted channel runs none of the above.
//
// 1. Compaction A: open, unmuted samples (nfm_gate_kernel's aidx).  Lowpass<Real>(301 taps, 250 Hz) sees demod * comp of
//    exactly those; its ring is the last 300 of that compacted sequence.  Its output is used only on detector samples.
// 2. Detector samples: members of A whose m_sampleCount, already incremented, has its low three bits set.  Only those bits
//    of the counter are carried (ct_detector_sample).  Compaction C is their Lowpass outputs in order.
// 3. CTCSSDetector (sdrbase/dsp/ctcssdetector.cpp): a block is N = audio_rate / 16 consecutive members of C, wherever the
//    feeds are cut: member d of this feed lies in block (fill + d) / N, fill = samplesProcessed carried in.  Goertzel feedback
//    per tone (ct_feedback) starts from 0 in every block but the one carried in; feedForward (ct_power) and evaluatePower
//    (ct_evaluate) run at a block's last member.  32 tones x blocks are independent chains.
// 4. m_ctcssIndex after sample i = the value of the last event at or before i, else the carried value: events are block ends
//    (value from the detector) and closed unmuted samples (value 0).  A last-writer scan (CtLast).  Within a sample the
//    detector's update comes before the mismatch test.
// 5. Compaction B: members of A that pass the mismatch test.  The Bandpass sees those; nfm_out_kernel runs on B as it does on A.
#pragma once
#include "nfm_scan.hpp"
#include <cmath>
#include <stdint.h>

namespace sdrx {

constexpr int CT_TONES = 32;
constexpr int CT_LP_H = AM_BP_H, CT_LP_HIST = AM_BP_HIST;   // Lowpass<Real>: 301 taps folded to 151, as the Bandpass
// one channel's row of the tap table: the 151 Bandpass taps, the 151 Lowpass taps, the 32 Goertzel coefficients
constexpr int NFM_TAB_LP = AM_BP_H + 1, NFM_TAB_COEF = 2 * (AM_BP_H + 1), NFM_TAB = 2 * (AM_BP_H + 1) + CT_TONES;

// the 32 EIA tones of CTCSSDetector's constructor, as the Reals it stores
inline const float* ct_tone_set()
{
    static const float t[CT_TONES] = {67.0f, 71.9f, 74.4f, 77.0f, 79.7f, 82.5f, 85.4f, 88.5f, 91.5f, 94.8f, 97.4f, 100.0f, 103.5f, 107.2f,
                                      110.9f, 114.8f, 118.8f, 123.0f, 127.3f, 131.8f, 136.5f, 141.3f, 146.2f, 151.4f, 156.7f, 162.2f,
                                      167.9f, 173.8f, 179.9f, 186.2f, 192.8f, 203.5f};
    return t;
}
// m_ctcssDetector.setCoefficients(m_audioSampleRate / 16, m_audioSampleRate / 8.0f): a uint32 quotient and a float one cut to int
inline int ct_block_n(int audio_rate) { return (int)((uint32_t)audio_rate / 16u); }
inline int ct_rate(int audio_rate) { return (int)((float)(uint32_t)audio_rate / 8.0f); }
inline float ct_coef(float tone, int rate) { return (float)(2.0 * std::cos((2.0 * 3.14159265358979323846 * (double)tone) / (double)rate)); }

// Lowpass<Real>::create(301, rate, cutoff) (sdrbase/dsp/lowpass.h:15-53), the folded 151 taps
inline void ct_lowpass_design(double rate, double cutoff, float* t)
{
    const double PI = 3.14159265358979323846;
    const int ntaps = 301, nt = 151;
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

// AFSquelch's design as NFMDemod's constructor asks for it: setCoefficients(audio_rate / 2000, 600, audio_rate, 200, 0, {1000.0,
// 6000.0}), each tone capped at 0.4 * rate, coef = 2.0 * cos((2.0 * M_PI * tone) / (double) rate), all in double, the rate a uint32.
// setCoefficients leaves the threshold at 0.0; only applySettings with m_deltaSquelch on sets another (sdrx_nfm_get_tone_design)
inline int af_block_n(int audio_rate) { return (int)((uint32_t)audio_rate / 2000u); }
inline double af_tone(int j, int audio_rate)
{
    const double t = j == 0 ? 1000.0 : 6000.0, top = ((double)(uint32_t)audio_rate) * 0.4;
    return t < top ? t : top;
}
inline double af_coef(double tone, int audio_rate) { return 2.0 * std::cos((2.0 * 3.14159265358979323846 * tone) / (double)(uint32_t)audio_rate); }

// ---- the AF squelch (m_deltaSquelch; sdrbase/dsp/afsquelch.cpp, sdrbase/util/doublebufferfifo.h, nfmdemod.cpp:179-206), all in
// double.  Its parts keep the reference's containers as they are, in the channel's carried memory, and one lane per channel walks
// the feed's samples through them in order (nfm_af_walk_kernel): the state after a feed is the reference's state, whatever the
// cuts.  Per sample: analyze(demod * comp) = feedback on both tones; a block is N + 1 samples (the test is samplesProcessed < N
// before the increment); at a block end feedForward computes the powers, feeds the two MovingAverage<double> (128 entries, see AF_MA) (sum += value -
// oldest: the difference first, then one rounded add), zeroes u and calls evaluate() itself; for the first 600 block ends analyze
// returns false, from then on true, and NFMDemod calls evaluate() a second time: m_afSquelchOpen = its result, and if that is
// false zeroBack(audio_rate / 10), which clears ONE of the delay line's two copies of each element it reaches.  Then the write
// (demod * comp if m_afSquelchOpen, else 0), the squelch counter and readBack(gate) as in nfm_scan.hpp.
constexpr int AF_AVG = 600;                                 // nbAvg: block ends before analyze returns true
// the MovingAverage histories keep the 128 entries of AFSquelch's constructor: setCoefficients' m_movingAverages.resize(m_nTones,
// MovingAverage<double>(600, 0.0)) finds the vector at that size and leaves its elements alone
constexpr int AF_MA = 128;
constexpr int AF_ATTACK = 200;                              // samplesAttack; samplesDecay is 0
struct AfState {                                            // what moves in AFSquelch, and NFMDemod's m_afSquelchOpen
    double u0[2], u1[2], sum[2];                            // Goertzel state, MovingAverage::m_sum
    int processed, avg_processed, ma_index;                 // m_samplesProcessed, m_samplesAvgProcessed, MovingAverage::m_index
    int count, is_open, af_open;                            // m_squelchCount, m_isOpen, m_afSquelchOpen
};
struct AfDelay { int write, cur; };                         // DoubleBufferFIFO::m_writeIndex, m_currentIndex
struct AfProbe { long block_ends, max_zero, second_eval, zero_events; };

// AFSquelch::evaluate
AM_HD bool af_evaluate(AfState& a, double thr, AfProbe* p)
{
    double max_power = 0.0, min_power;
    int min_index = 0, max_index = 0;
    for (int j = 0; j < 2; j++) if (a.sum[j] > max_power) { max_power = a.sum[j]; max_index = j; }
    if (max_power == 0.0) { if (p) p->max_zero++; return a.is_open != 0; }
    min_power = max_power;
    for (int j = 0; j < 2; j++) if (a.sum[j] < min_power) { min_power = a.sum[j]; min_index = j; }
    if ((min_power / max_power < thr) && (min_index > max_index)) { if (a.count < AF_ATTACK) a.count++; }
    else { if (a.count > AF_ATTACK) a.count--; else a.count = 0; }
    a.is_open = a.count >= AF_ATTACK;
    return a.is_open != 0;
}
// AFSquelch::analyze; hist: the two MovingAverage histories, [2][AF_MA]
AM_HD bool af_analyze(AfState& a, double* hist, int N, const double* coef, double thr, double in, AfProbe* p)
{
    for (int j = 0; j < 2; j++) { const double t = a.u0[j]; a.u0[j] = in + (coef[j] * a.u0[j]) - a.u1[j]; a.u1[j] = t; }
    if (a.processed < N) { a.processed++; return false; }
    for (int j = 0; j < 2; j++) {                           // feedForward
        const double power = (a.u0[j] * a.u0[j]) + (a.u1[j] * a.u1[j]) - (coef[j] * a.u0[j] * a.u1[j]);
        double& oldest = hist[j * AF_MA + a.ma_index];
        a.sum[j] += power - oldest;
        oldest = power;
        a.u0[j] = 0.0; a.u1[j] = 0.0;
    }
    a.ma_index = a.ma_index < AF_MA - 1 ? a.ma_index + 1 : 0;
    if (p) p->block_ends++;
    af_evaluate(a, thr, p);
    a.processed = 0;
    if (a.avg_processed < AF_AVG) { a.avg_processed++; return false; }
    return true;
}
// DoubleBufferFIFO<Real>(24000): d has 2 * NFM_DL entries
AM_HD void af_dl_write(float* d, AfDelay& q, float v)
{
    d[q.write] = v; d[q.write + NFM_DL] = v;
    q.cur = q.write;
    q.write = q.write < NFM_DL - 1 ? q.write + 1 : 0;
}
AM_HD int af_dl_read_slot(const AfDelay& q, int delay) { return q.cur + NFM_DL - (delay > NFM_DL ? NFM_DL : delay); }
AM_HD void af_dl_zero_back(float* d, const AfDelay& q, int delay)
{
    if (delay > NFM_DL) delay = NFM_DL;
    for (int i = 0; i < delay; i++) d[q.cur + NFM_DL - i] = 0.0f;
}
// one audio sample of the delta-mode squelch up to the delay line's write: returns `up` = m_afSquelchOpen
AM_HD bool af_sample(AfState& a, double* hist, float* d, AfDelay& q, int N, const double* coef, double thr, int Z, float wraw, AfProbe* p)
{
    if (af_analyze(a, hist, N, coef, thr, (double)wraw, p)) {
        if (p) p->second_eval++;
        a.af_open = af_evaluate(a, thr, p) ? 1 : 0;
        if (!a.af_open) { af_dl_zero_back(d, q, Z); if (p) p->zero_events++; }
    }
    af_dl_write(d, q, a.af_open ? wraw : 0.0f);
    return a.af_open != 0;
}
// m_squelchLevel with m_deltaSquelch: (Real)((-m_squelch) / 1000.0), m_squelch a Real; the threshold is its double
inline float af_level(float squelch) { return (float)((double)(-squelch) / 1000.0); }

// sample i of a feed that starts with (m_sampleCount & 7) == sc: the count is incremented before it is tested
AM_HD bool ct_detector_sample(int sc, long i) { return ((sc + i + 1) & 7) == 7; }
AM_HD int ct_count_after(int sc, long n) { return (int)((sc + n) & 7); }

// CTCSSDetector::feedback for one tone: u0 = in + (coef * u0) - u1
AM_HD void ct_feedback(float in, float coef, float& u0, float& u1)
{
    const float t = u0;
    u0 = (in + (coef * u0)) - u1;
    u1 = t;
}
// feedForward: (u0 * u0) + (u1 * u1) - (coef * u0 * u1)
AM_HD float ct_power(float coef, float u0, float u1) { return ((u0 * u0) + (u1 * u1)) - ((coef * u0) * u1); }

// evaluatePower over the 32 powers in order.  max_index: the first strict maximum above 0, -1 where no power is above 0
// (maxPowerIndex then keeps the value it had).  Returns toneDetected.
AM_HD bool ct_evaluate(const float* power, int* max_index)
{
    float sum = 0.0f, max_power = 0.0f;
    int mi = -1;
    for (int j = 0; j < CT_TONES; j++) {
        sum += power[j];
        if (power[j] > max_power) { max_power = power[j]; mi = j; }
    }
    *max_index = mi;
    return max_power > (sum / (float)CT_TONES) + 2.0f;
}

// block geometry of compaction C: `fill` members of the open block came with earlier feeds, this feed brings nd
AM_HD int ct_blocks_touched(int fill, int nd, int N) { return nd > 0 ? (fill + nd + N - 1) / N : 0; }
AM_HD int ct_blocks_done(int fill, int nd, int N) { return (fill + nd) / N; }
AM_HD long ct_block_first(int fill, int b, int N) { return b == 0 ? 0 : (long)b * N - fill; }    // member of this feed
AM_HD long ct_block_end(int fill, int b, int N) { return ((long)b + 1) * N - fill; }             // one past its last member

// last-writer maps: -1 leaves the index as it is, v >= 0 sets it
AM_HD int ct_last_compose(int f, int g) { return g >= 0 ? g : f; }
AM_HD int ct_last_apply(int f, int carried) { return f >= 0 ? f : carried; }
// the event of a sample outside the block ends: closed and unmuted zeroes the index
AM_HD int ct_closed_event(bool in_a, bool mute) { return (!in_a && !mute) ? 0 : -1; }
AM_HD bool ct_mismatch(int selected, int index) { return selected != 0 && selected != index; }

} // namespace sdrx
