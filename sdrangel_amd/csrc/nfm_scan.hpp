// The recurrences of NFMDemod::feed's per-sample loop (plugins/channelrx/demodnfm/nfmdemod.cpp:157-300, m_deltaSquelch and
// m_ctcssOn off) cut into terms that can be computed in parallel.  A subset of am_scan.hpp's, whose stream indexing
// (am_stream_at / am_hist_next) and Bandpass walk (am_bandpass) are used as they are.  Compiles for the host too.
//
// 1. MovingAverageUtil<Real, double, 32>: total += (double)(magsq[i] - magsq[i - 32]) with the power before the stream taken
//    as 0 (am_ma_term): a rounded prefix sum of terms known in advance.
// 2. Squelch counter: `if ((Real) m_movingAverage < level) { if (count > 0) count--; } else { if (count < 2 * gate) count++; }`
//    -- the clamp maps of wfm_scan.hpp with cap 2 * gate; open = count > gate.
// 3. DoubleBufferFIFO<Real>(24000): w[i] = below ? 0 : demod * comp is written BEFORE readBack(gate), and readBack clamps its
//    delay to the line's size, where m_data[m_currentIndex + size - size] is the slot just written.  So the sample read is
//    w[i - gate] for gate < 24000 and w[i] itself from there on (nfm_delay).
// 4. Bandpass<Real>: sees open, unmuted samples only; its ring is the last 300 of the compacted sequence of delayed samples.
#pragma once
#include "am_scan.hpp"

namespace sdrx {

constexpr int NFM_MA = 32;                                  // MovingAverageUtil<Real, double, 32>
constexpr int NFM_DL = 24000;                               // m_squelchDelayLine(24000)

AM_HD int nfm_delay(int gate) { return gate >= NFM_DL ? 0 : gate; }
// Real magsq = magsqRaw / (SDR_RX_SCALED * SDR_RX_SCALED), magsqRaw the double of a float sum of squares
AM_HD float nfm_magsq(float raw) { return (float)((double)raw / (32768.0 * 32768.0)); }
// (Real) m_movingAverage = (Real)(m_total / 32) against the Real level: the counter goes up unless it is below
AM_HD bool nfm_up(double total, float level) { return !((float)(total / NFM_MA) < level); }
AM_HD bool nfm_open(int count, int gate) { return count > gate; }
// phaseDiscriminatorDelta (phasediscri.h:61-78) from this sample's and the previous sample's argument
AM_HD float nfm_demod(float cur, float prev, float fm_scaling)
{
    float dev = (float)((double)(cur - prev) / 3.14159265358979323846);
    if (dev < -1.0f) dev += 2.0f; else if (dev > 1.0f) dev -= 2.0f;
    return dev * fm_scaling;
}

} // namespace sdrx
