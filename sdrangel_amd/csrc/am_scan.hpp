// The recurrences of AMDemod::processOneSample (plugins/channelrx/demodam/amdemod.cpp:152-276, envelope mode) cut into
// terms that can be computed in parallel, and the index arithmetic that goes with them.  Compiles for the host too
// (tests/am_scan_check.cpp), no HIP header needed.
//
// 1. MovingAverageUtil<Real, double, 16>: `total += sample` while filling up, `total += sample - oldest` (the difference in
//    float) after.  With the power before the stream taken as 0 both are  total += (double)(magsq[i] - magsq[i - 16]),
//    since x - 0.0f == x: a rounded prefix sum of terms known in advance (am_ma_term).
// 2. Squelch counter: `if (m_magsq < level) { if (count > 0) count--; } else { if (count < rate / 10) count++; }` -- the
//    clamp maps of wfm_scan.hpp with the integer cap rate / 10; open = count >= rate / 20.
// 3. SimpleAGC / MovingAverage<double>: fed only on open, unmuted samples whose delayed root is > 0.  The fed values are
//    compacted into a sequence v; `sum += v[j] - v[j - H]` in double, H = rate / 10, the history before the first fed value
//    being (double) 0.003f: again a rounded prefix sum of known terms (am_agc_term).
// 4. Bandpass<Real>: sees open, unmuted samples only; its ring is the last 300 of the compacted demod sequence.
//
// A stream that carries across feeds is kept as [hist: its last K elements before this feed | cur: this feed's elements];
// am_stream_at indexes it with j < 0 reaching into the history, am_hist_next builds the next feed's history.
#pragma once
#include "wfm_scan.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AM_HD __host__ __device__ __forceinline__
#else
#define AM_HD inline
#endif

namespace sdrx {

constexpr int AM_MA = 16;                                  // MovingAverageUtil<Real, double, 16>
constexpr int AM_BP_TAPS = 301, AM_BP_H = 150;             // Bandpass: 301 taps, folded to 151
constexpr int AM_BP_HIST = AM_BP_TAPS - 1;                 // ring entries older than the current sample

template <class T> AM_HD T am_stream_at(const T* hist, int K, const T* cur, long j) { return j < 0 ? hist[K + j] : cur[j]; }
// entry i of the history after a feed of n elements: stream element n - K + i (>= -K)
template <class T> AM_HD T am_hist_next(const T* hist, int K, const T* cur, long n, int i) { return am_stream_at(hist, K, cur, n - K + i); }

AM_HD double am_ma_term(float cur, float old16) { return (double)(cur - old16); }
AM_HD double am_agc_term(double v, double oldH) { return v - oldH; }
AM_HD double am_agc_initial() { return (double)0.003f; }   // m_volumeAGC.resizeNew(rate / 10, 0.003): a Real argument

// m_magsq = total / 16 (asDouble) against the Real level: the counter goes up unless m_magsq < level
AM_HD bool am_up(double total, float level) { return !(total / (double)AM_MA < (double)level); }
AM_HD bool am_open(int count, int rate) { return count >= rate / 20; }
AM_HD bool am_fed(bool open, bool mute, float delayed_root) { return open && !mute && delayed_root > 0.0f; }

// one sample of the gate: counter step, then where the sample lands in the compacted sequences
struct AmGate {
    int count;      // squelch counter
    int n_act;      // open, unmuted samples so far (this feed): the next one's index in the demod sequence
    int n_fed;      // fed samples so far (this feed): the AGC sum a sample sees is the prefix sum at n_fed - 1
};
struct AmSlot { int count, act_idx, fed_cnt; bool fed; };  // act_idx -1: closed or muted
AM_HD AmSlot am_gate_step(AmGate& g, bool up, int rate, bool mute, float delayed_root)
{
    g.count = wfm_apply(wfm_step(up, rate / 10), g.count);
    const bool open = am_open(g.count, rate);
    AmSlot r;
    r.count = g.count;
    r.act_idx = open && !mute ? g.n_act++ : -1;
    r.fed = am_fed(open, mute, delayed_root);
    if (r.fed) g.n_fed++;
    r.fed_cnt = g.n_fed;
    return r;
}

// Bandpass<Real>::filter (bandpass.h:77-122) on the compacted sequence: X(k) = the demod value k open samples back.  The
// ring walk pairs the new sample with the one before it, then the oldest with the next one back, and so on.
template <class F> AM_HD float am_bandpass(const float* taps, F X)
{
    float acc = 0.0f;
    acc += (X(0) + X(1)) * taps[0];
    for (int i = 1; i < AM_BP_H; i++) acc += (X(AM_BP_TAPS - i) + X(1 + i)) * taps[i];
    acc += X(AM_BP_H + 1) * taps[AM_BP_H];
    return acc;
}

} // namespace sdrx
