/* Strict-IEEE scalar restatement of ATVDemod::feed with demod(), processClassic() and processHSkip()
 * (plugins/channelrx/demodatv/atvdemod.cpp:167-444, atvdemod.h:498-744) and of applySettings / applyStandard (:539-732),
 * streaming, one demodulator per object, in the reference's statement order and with its member names.  The screen is the
 * recording image TVScreen is to the demodulator (sdrgui/gui/glshadertvarray.cpp:294-328).  The NCO's table and increment,
 * FM3's discriminator, the Interpolator's taps (sdro_backend_new_at: create(24, tvRate, rf_bw / 2.2f, 3.0)) and m_DSBFilter
 * (sdro_fftfilt_new_asym, runAsym) are oracle/libsdro.so's; decimate() and the walk through m_DSBFilterBuffer are restated here.
 * Nothing of the device code is used: atv_scan.hpp is included for the branch numbers only.  The checker of sdrx_atv_*: tests build it with `g++ -O2 -ffp-contract=off -fno-fast-math -shared` and call it
 * through ctypes (tests/atv_cases.py); the product never links it.
 *
 * Pinned as include/sdrx.h pins it: m_intAvgColIndex starts at 0; the screen counts as initialised, starts as zeros with a null
 * row; a float that no int holds, NaN included, converts to INT_MIN, and the scope Sample keeps the low 16 bits of that int;
 * m_DSBFilterBuffer starts as zeros and demod reads its slot index - 1; FM3 takes the unfiltered sample.
 *
 *   ato_create(cfg)                 a sdrx_atv_cfg; NULL where sdrx_atv_create refuses it
 *   ato_feed(h, iq, n)              feed(); returns the renderImage calls
 *   ato_events(h, out, cap)         the sample index of each render of the last feed; returns their count
 *   ato_frame(h, k, buf)            the screen at render k < frames_cap of the last feed; returns rows * cols or -1
 *   ato_screen(h, buf)              the screen now
 *   ato_scope(h, out, cap)          the scope Samples' real parts of the last feed; returns their count
 *   ato_state(h, out)               sdrx_atv_state_t
 *   ato_design(h, out)              sdrx_atv_design_t
 *   ato_hits(h, out[ATV_N_HITS + 1])  the branch counters since creation, then the most renders within one line
 *   ato_geo(h, out[ATO_N_GEO])      the geometry counters of processClassic since creation: what a 64-sample partition of the
 *                                   stream can get wrong, each defined on the reference's own variables (the GEO_ enum below)
 */
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/sdrx.h"
#include "../oracle/sdro.h"
#include "atv_scan.hpp"

namespace {

using namespace sdrx;                                           /* the ATV_HIT_ numbers */

const float SDR_RX_SCALEF = 32768.0f;

/* the geometry counters, in the order of tests/atv_cases.py's GEO; all of processClassic, a sample being one call of it */
enum {
    GEO_DETECT_HELD,        /* m_blnSynchroDetected true on the sample directly after one where it was true */
    GEO_DETECT_TWICE_NEAR,  /* a detection 2 .. 63 samples after the one before */
    GEO_POINTS_FROM_FAR,    /* a detection whose counted run (the first increment behind the last reset) began >= 64 samples earlier */
    GEO_VSYNC_TIE,          /* a vsync check with m_fltAmpLineAverage == fltSynchroTrameLevel: it fires */
    GEO_VSYNC_FIRST_COL,    /* the vsync fires on the sample where m_intColIndex reaches intSynchroTimeSamples */
    GEO_VSYNC_LAST_COL,     /* the vsync fires on the last sample before a new line */
    GEO_VSYNC_AGAIN,        /* the sum at or under the level while m_blnVerticalSynchroDetected is set: cleared, no event */
    GEO_COL_NEGATIVE,       /* the line-0 correction leaves m_intColIndex < 0 */
    GEO_COL_PAST_LINE,      /* ... or >= samples per line + per top */
    GEO_LINE_PAST_FRAME,    /* the half-frame branch with vsync on: m_intLineIndex reached m_intNumberOfLines */
    GEO_ROW_STAYS,          /* a new line with m_intRowIndex >= m_intNumberOfLines: no selectRow */
    GEO_NAN_AT_CHECK,       /* a vsync check with a NaN sum */
    GEO_DETECT_AT_HALF,     /* a detection with m_intColIndex == samples per line / 2: the first column where the -150 term is left out */
    ATO_N_GEO
};

int f2i(float v)                                                /* cvttss2si */
{
    if (v != v || v >= 2147483648.0f || v < -2147483648.0f) return INT_MIN;
    return (int)v;
}

struct Screen {
    int cols, rows, row;                                        /* row -1: m_objCurrentRow == 0 */
    std::vector<uint8_t> img;
};

struct Ato {
    sdrx_atv_cfg k;
    /* NCO */
    float table[4096];
    int phase, inc;
    float prev_c[2];                                            /* the sample before, for the stateless sdro_discri */
    /* Interpolator: m_taps of all phases, m_samples as a ring, m_ptr; the distance */
    sdro_backend* ip;
    int m_nTaps, m_ptr;
    std::vector<float> m_samples;                               /* (re, im) pairs */
    float m_interpolatorDistance, m_interpolatorDistanceRemain;
    /* m_DSBFilter, m_DSBFilterBuffer, m_DSBFilterBufferIndex */
    sdro_fftfilt* m_DSBFilter;
    float m_DSBFilterBuffer[2 * 1024];
    int m_DSBFilterBufferIndex;
    /* ATV PARAMETERS */
    int m_intNumberSamplePerLine, m_intNumberSamplePerTop, m_intNumberOfLines, m_intNumberOfSyncLines, m_intNumberOfBlackLines,
        m_intNumberOfEqLines, m_intNumberSamplePerLineSignals, m_intNumberSaplesPerHSync, m_intTVSampleRate;
    bool m_interleaved;
    /* PROCESSING */
    int m_intImageIndex, m_intSynchroPoints;
    bool m_blnSynchroDetected, m_blnVerticalSynchroDetected;
    float m_fltAmpLineAverage, m_fltEffMin, m_fltEffMax, m_fltAmpMin, m_fltAmpMax, m_fltAmpDelta;
    float m_fltBufferI[6], m_fltBufferQ[6];
    int m_intColIndex, m_intSampleIndex, m_intRowIndex, m_intLineIndex, m_intAvgColIndex;
    Screen screen;
    /* per feed */
    long at;
    std::vector<int32_t> events;
    std::vector<std::vector<uint8_t> > frames;
    std::vector<int16_t> scope;
    /* probes */
    int64_t hits[ATV_N_HITS];
    int64_t renders_in_line, max_renders_in_line;
    int64_t geo[ATO_N_GEO];
    int64_t tick, last_detection, run_start;                    /* processClassic calls; the call of the last detection, of the run's first increment (-1: none) */

    void selectRow(int line)
    {
        if (line < 0) hits[ATV_HIT_ROW_NEG]++; else if (line >= screen.rows) hits[ATV_HIT_ROW_BIG]++;
        if (line < screen.rows && line >= 0) screen.row = line; else screen.row = -1;
    }
    void setDataColor(int col, int v)
    {
        if (col < 0) hits[ATV_HIT_COL_NEG]++; else if (col >= screen.cols) hits[ATV_HIT_COL_BIG]++;
        if (screen.row < 0) hits[ATV_HIT_NULL_ROW]++;
        if (col < screen.cols && col >= 0 && screen.row >= 0) screen.img[(size_t)screen.row * screen.cols + col] = (uint8_t)v;
    }
    void renderImage()
    {
        if ((int)frames.size() < k.frames_cap) frames.push_back(screen.img);
        events.push_back((int32_t)at);
        if (++renders_in_line > max_renders_in_line) max_renders_in_line = renders_in_line;
    }
    void amUpdate()
    {
        m_fltAmpMin = m_fltEffMin;
        m_fltAmpMax = m_fltEffMax;
        m_fltAmpDelta = m_fltEffMax - m_fltEffMin;
        if (m_fltAmpDelta <= 0.0) { m_fltAmpDelta = 1.0f; hits[ATV_HIT_DELTA_ONE]++; }
        m_fltEffMin = 2000000.0f;
        m_fltEffMax = -2000000.0f;
    }

    void processHSkip(float& fltVal, int& intVal)
    {
        setDataColor(m_intColIndex - m_intNumberSaplesPerHSync + m_intNumberSamplePerTop, intVal);
        if (fltVal < k.level_synchro_top) m_intSynchroPoints++;
        else if (fltVal > k.level_black) m_intSynchroPoints = 0;
        m_blnSynchroDetected = (m_intSynchroPoints == m_intNumberSamplePerTop);
        if (m_blnSynchroDetected) {
            if (m_intSampleIndex >= (3 * m_intNumberSamplePerLine) / 2) {
                m_intAvgColIndex = m_intColIndex;
                hits[ATV_HIT_HSKIP_RENDER]++;
                renderImage();
                m_intImageIndex++;
                m_intLineIndex = 0;
                m_intRowIndex = 0;
            }
            m_intSampleIndex = 0;
        } else {
            m_intSampleIndex++;
        }
        if (m_intColIndex < m_intNumberSamplePerLine + m_intNumberSamplePerTop - 1) {
            m_intColIndex++;
        } else {
            if (k.hsync && (m_intLineIndex == 0)) {
                hits[ATV_HIT_HCORR_HSKIP]++;
                m_intColIndex = m_intNumberSamplePerTop + (m_intNumberSamplePerLine - m_intAvgColIndex) / 2;
            } else {
                m_intColIndex = m_intNumberSamplePerTop;
            }
            if (k.modulation == ATV_AM) amUpdate();
            renders_in_line = 0;
            selectRow(m_intRowIndex);
            m_intLineIndex++;
            m_intRowIndex++;
        }
    }

    void processClassic(float& fltVal, int& intVal)
    {
        int intSynchroTimeSamples = (3 * m_intNumberSamplePerLine) / 4;
        float fltSynchroTrameLevel = 0.5f * ((float)intSynchroTimeSamples) * k.level_black;
        tick++;
        if (fltVal < k.level_synchro_top) { if (run_start < 0) run_start = tick; m_intSynchroPoints++; }
        else if (fltVal > k.level_black) { m_intSynchroPoints = 0; run_start = -1; }
        m_blnSynchroDetected = (m_intSynchroPoints == m_intNumberSamplePerTop);
        bool blnNewLine = false;
        if (m_blnSynchroDetected) {
            if (last_detection >= 0) {
                const int64_t gap = tick - last_detection;
                if (gap == 1) geo[GEO_DETECT_HELD]++;
                else if (gap <= 63) geo[GEO_DETECT_TWICE_NEAR]++;
            }
            if (run_start >= 0 && tick - run_start >= 64) geo[GEO_POINTS_FROM_FAR]++;
            last_detection = tick;
            if (m_intColIndex == m_intNumberSamplePerLine / 2) geo[GEO_DETECT_AT_HALF]++;
            if (m_intColIndex < m_intNumberSamplePerLine / 2) hits[ATV_HIT_MINUS150]++;
            m_intAvgColIndex = m_intSampleIndex - m_intColIndex - (m_intColIndex < m_intNumberSamplePerLine / 2 ? 150 : 0);
            m_intSampleIndex = 0;
        } else {
            m_intSampleIndex++;
        }
        if (!k.hsync && (m_intColIndex >= m_intNumberSamplePerLine)) {
            m_intColIndex = 0;
            blnNewLine = true;
        } else if (m_intColIndex >= m_intNumberSamplePerLine + m_intNumberSamplePerTop) {
            hits[ATV_HIT_NO_HSYNC]++;
            if (k.hsync && (m_intLineIndex == 0)) {
                hits[ATV_HIT_HCORR_CLASSIC]++;
                m_intColIndex = m_intNumberSamplePerTop + m_intAvgColIndex / 4;
                if (m_intColIndex < 0) geo[GEO_COL_NEGATIVE]++;
                else if (m_intColIndex >= m_intNumberSamplePerLine + m_intNumberSamplePerTop) geo[GEO_COL_PAST_LINE]++;
            } else {
                m_intColIndex = m_intNumberSamplePerTop;
            }
            blnNewLine = true;
        }
        if (blnNewLine) {
            if (k.modulation == ATV_AM) amUpdate();
            m_fltAmpLineAverage = 0.0f;
            m_intRowIndex += m_interleaved ? 2 : 1;
            if (m_intRowIndex < m_intNumberOfLines) selectRow(m_intRowIndex - m_intNumberOfSyncLines);
            else geo[GEO_ROW_STAYS]++;
            m_intLineIndex++;
            renders_in_line = 0;
        }
        setDataColor(m_intColIndex - m_intNumberSaplesPerHSync + m_intNumberSamplePerTop + 4, intVal);
        m_intColIndex++;
        if (k.vsync && (m_intLineIndex < m_intNumberOfLines)) {
            if (m_intColIndex >= intSynchroTimeSamples) {
                if (m_fltAmpLineAverage != m_fltAmpLineAverage) geo[GEO_NAN_AT_CHECK]++;
                if (m_fltAmpLineAverage <= fltSynchroTrameLevel) {
                    if (m_fltAmpLineAverage == fltSynchroTrameLevel) geo[GEO_VSYNC_TIE]++;
                    if (m_blnVerticalSynchroDetected) geo[GEO_VSYNC_AGAIN]++;
                    else {
                        if (m_intColIndex == intSynchroTimeSamples) geo[GEO_VSYNC_FIRST_COL]++;
                        if (m_intColIndex >= m_intNumberSamplePerLine + (k.hsync ? m_intNumberSamplePerTop : 0)) geo[GEO_VSYNC_LAST_COL]++;
                    }
                    m_fltAmpLineAverage = 0.0f;
                    if (!m_blnVerticalSynchroDetected) {
                        m_blnVerticalSynchroDetected = true;
                        if ((m_intLineIndex % 2 == 0) || !m_interleaved) {
                            hits[ATV_HIT_VSYNC_EVEN]++;
                            renderImage();
                            m_intRowIndex = 1;
                        } else {
                            hits[ATV_HIT_VSYNC_ODD]++;
                            m_intRowIndex = 0;
                        }
                        selectRow(m_intRowIndex - m_intNumberOfSyncLines);
                        m_intLineIndex = 0;
                        m_intImageIndex++;
                    }
                } else {
                    m_blnVerticalSynchroDetected = false;
                }
            }
        } else {
            if (m_intLineIndex >= m_intNumberOfLines / 2) {
                hits[ATV_HIT_HALF_FRAME]++;
                if (k.vsync) geo[GEO_LINE_PAST_FRAME]++;
                if (m_intImageIndex % 2 == 1) {
                    renderImage();
                    if (k.modulation == ATV_AM) { hits[ATV_HIT_HALF_FRAME_AM]++; amUpdate(); }
                    m_intRowIndex = 1;
                } else {
                    m_intRowIndex = 0;
                }
                selectRow(m_intRowIndex - m_intNumberOfSyncLines);
                m_intLineIndex = 0;
                m_intImageIndex++;
            }
        }
    }

    /* Interpolator::decimate (interpolator.h:23-36) with the scalar doInterpolate */
    bool decimate(float* distance, float cr, float ci, float* rr, float* ri)
    {
        m_ptr--;
        if (m_ptr < 0) m_ptr = m_nTaps - 1;
        m_samples[2 * m_ptr] = cr; m_samples[2 * m_ptr + 1] = ci;
        *distance -= 1.0;
        if (*distance >= 1.0) return false;
        int phase = (int)floor(*distance * (float)24);
        if (phase < 0) phase = 0;
        const float* coeff = sdro_backend_taps(ip) + phase * m_nTaps;
        float rAcc = 0, iAcc = 0;
        int sample = m_ptr;
        for (int i = 0; i < m_nTaps; i++) {
            rAcc += *coeff * m_samples[2 * sample];
            iAcc += *coeff * m_samples[2 * sample + 1];
            sample = (sample + 1) % m_nTaps;
            coeff++;
        }
        *rr = rAcc; *ri = iAcc;
        return true;
    }

    void demod(float cr, float ci)
    {
        float fltDivSynchroBlack = 1.0f - k.level_black;
        float fltNormI, fltNormQ, fltNorm, fltVal;
        int intVal;
        if (k.fft_filtering) {
            const float in[2] = { cr, ci };
            static float filtered[2 * 2048];
            const int n_out = (int)sdro_fftfilt_run(m_DSBFilter, 4, in, 1, filtered);        /* runAsym(c, &filtered, true) */
            if (n_out > 0) {
                memcpy(m_DSBFilterBuffer, filtered, (size_t)n_out * 2 * sizeof(float));
                m_DSBFilterBufferIndex = 0;
            }
            m_DSBFilterBufferIndex++;
        }
        const float fltI = k.fft_filtering ? m_DSBFilterBuffer[2 * (m_DSBFilterBufferIndex - 1)] : cr;
        const float fltQ = k.fft_filtering ? m_DSBFilterBuffer[2 * (m_DSBFilterBufferIndex - 1) + 1] : ci;
        double magSq;
        if (k.modulation == ATV_FM1 || k.modulation == ATV_FM2) {
            magSq = fltI * fltI + fltQ * fltQ;
            fltNorm = sqrt(magSq);
            fltNormI = fltI / fltNorm;
            fltNormQ = fltQ / fltNorm;
            if (k.modulation == ATV_FM1) {
                fltVal = m_fltBufferI[0] * (fltNormQ - m_fltBufferQ[1]);
                fltVal -= m_fltBufferQ[0] * (fltNormI - m_fltBufferI[1]);
                fltVal += 2.0f;
                fltVal /= 4.0f;
            } else {
                fltVal = m_fltBufferI[2] * ((m_fltBufferQ[5] - fltNormQ) / 16.0f + m_fltBufferQ[1] - m_fltBufferQ[3]);
                fltVal -= m_fltBufferQ[2] * ((m_fltBufferI[5] - fltNormI) / 16.0f + m_fltBufferI[1] - m_fltBufferI[3]);
                fltVal += 2.125f;
                fltVal /= 4.25f;
                m_fltBufferI[5] = m_fltBufferI[4]; m_fltBufferQ[5] = m_fltBufferQ[4];
                m_fltBufferI[4] = m_fltBufferI[3]; m_fltBufferQ[4] = m_fltBufferQ[3];
                m_fltBufferI[3] = m_fltBufferI[2]; m_fltBufferQ[3] = m_fltBufferQ[2];
                m_fltBufferI[2] = m_fltBufferI[1]; m_fltBufferQ[2] = m_fltBufferQ[1];
            }
            m_fltBufferI[1] = m_fltBufferI[0]; m_fltBufferQ[1] = m_fltBufferQ[0];
            m_fltBufferI[0] = fltNormI; m_fltBufferQ[0] = fltNormQ;
            if (k.fm_deviation != 1.0f) fltVal = ((fltVal - 0.5f) / k.fm_deviation) + 0.5f;
        } else if (k.modulation == ATV_AM) {
            magSq = fltI * fltI + fltQ * fltQ;
            fltNorm = sqrt(magSq);
            fltVal = fltNorm / SDR_RX_SCALEF;
            if (fltVal < m_fltEffMin) m_fltEffMin = fltVal;
            if (fltVal > m_fltEffMax) m_fltEffMax = fltVal;
            fltVal -= m_fltAmpMin;
            fltVal /= m_fltAmpDelta;
        } else {                                                /* ATV_FM3: setFMScaling(1.0f / m_fmDeviation) */
            const float pair[4] = { prev_c[0], prev_c[1], cr, ci };
            float out[2];
            sdro_discri(0, 1.0f / k.fm_deviation, pair, 2, out);
            fltVal = out[1] + 0.5f;
        }
        prev_c[0] = cr; prev_c[1] = ci;

        fltVal = k.invert_video ? 1.0f - fltVal : fltVal;
        fltVal = (fltVal < -1.0f) ? -1.0f : (fltVal > 1.0f) ? 1.0f : fltVal;
        if (k.scope) scope.push_back((int16_t)(uint16_t)((uint32_t)f2i(fltVal * SDR_RX_SCALEF) & 0xffffu));
        m_fltAmpLineAverage += fltVal;
        {
            const float t = (int)255.0 * (fltVal - k.level_black) / fltDivSynchroBlack;
            intVal = f2i(t);
        }
        if (intVal < 0) intVal = 0; else if (intVal > 255) intVal = 255;
        if (k.standard == ATV_STD_HSKIP) processHSkip(fltVal, intVal); else processClassic(fltVal, intVal);
    }
};

bool apply_settings(Ato* h)
{
    const sdrx_atv_cfg& k = h->k;
    if (k.in_rate <= 0) return false;
    if (k.modulation < ATV_FM1 || k.modulation > ATV_AM) return false;
    if (k.standard < 0 || k.standard > ATV_STD_HSKIP) return false;
    if (!(k.level_black < 1.0f)) return false;
    if (k.frames_cap < 1) return false;
    if ((k.fft_filtering || k.decimator_enable) && !(k.rf_bw > 0.0f && k.rf_bw < 1.0e9f)) return false;
    if (k.fft_filtering && !(k.rf_opp_bw >= 0.0f && k.rf_opp_bw < 1.0e9f)) return false;
    if (k.n_lines < 1 || !(k.frames_per_s > 0.0f)) return false;
    if (!(k.line_duration >= 0.0f) || !(k.top_duration >= 0.0f) || !(k.fm_deviation == k.fm_deviation) || k.fm_deviation == 0.0f) return false;
    h->m_intNumberOfLines = k.n_lines;
    switch (k.standard) {
    case ATV_STD_HSKIP:             h->m_intNumberOfSyncLines = 0;  h->m_intNumberOfBlackLines = 0;  h->m_intNumberOfEqLines = 0; h->m_interleaved = false; break;
    case ATV_STD_SHORT:             h->m_intNumberOfSyncLines = 4;  h->m_intNumberOfBlackLines = 4;  h->m_intNumberOfEqLines = 0; h->m_interleaved = false; break;
    case ATV_STD_SHORT_INTERLEAVED: h->m_intNumberOfSyncLines = 4;  h->m_intNumberOfBlackLines = 4;  h->m_intNumberOfEqLines = 0; h->m_interleaved = true; break;
    case ATV_STD_405:               h->m_intNumberOfSyncLines = 24; h->m_intNumberOfBlackLines = 28; h->m_intNumberOfEqLines = 3; h->m_interleaved = true; break;
    case ATV_STD_PAL525:            h->m_intNumberOfSyncLines = 40; h->m_intNumberOfBlackLines = 44; h->m_intNumberOfEqLines = 3; h->m_interleaved = true; break;
    default:                        h->m_intNumberOfSyncLines = 44; h->m_intNumberOfBlackLines = 48; h->m_intNumberOfEqLines = 3; h->m_interleaved = true;
    }
    h->m_intNumberSamplePerLineSignals = (int)((12.0f / 64.0f) * k.line_duration * k.in_rate);
    h->m_intNumberSaplesPerHSync = (int)((9.6f / 64.0f) * k.line_duration * k.in_rate);
    int linesPerSecond = k.n_lines * k.frames_per_s;
    if (linesPerSecond < 1) return false;
    int maxPoints = k.in_rate / linesPerSecond;
    int i = maxPoints;
    for (; i > 0; i--) {
        if ((i * linesPerSecond) % 10 == 0) break;
    }
    int nbPointsPerRateUnit = i == 0 ? maxPoints : i;
    h->m_intTVSampleRate = nbPointsPerRateUnit * linesPerSecond;
    if (!(h->m_intTVSampleRate > 0)) h->m_intTVSampleRate = k.in_rate;
    h->m_intNumberSamplePerLine = (int)(k.line_duration * k.in_rate);
    h->m_intNumberSamplePerTop = (int)(k.top_duration * k.in_rate);
    h->screen.cols = h->m_intNumberSamplePerLine - h->m_intNumberSamplePerLineSignals;
    h->screen.rows = h->m_intNumberOfLines - h->m_intNumberOfBlackLines;
    return h->screen.cols >= 1 && h->screen.rows >= 1;
}

uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }

} // namespace

extern "C" {

void* ato_create(const sdrx_atv_cfg* cfg)
{
    Ato* h = new Ato;
    h->k = *cfg;
    if (!apply_settings(h)) { delete h; return 0; }
    sdro_nco_table(h->table);
    h->phase = 0;
    h->inc = sdro_nco_inc((float)cfg->nco_freq, (float)cfg->in_rate);
    h->prev_c[0] = h->prev_c[1] = 0.0f;
    /* m_interpolatorDistance = (Real) tvRate / (Real) rate; m_interpolator.create(24, tvRate, rf_bw / divisor, 3.0) */
    h->m_interpolatorDistance = (float)h->m_intTVSampleRate / (float)cfg->in_rate;
    h->m_interpolatorDistanceRemain = 0;
    h->ip = 0; h->m_nTaps = 0; h->m_ptr = 0;
    if (cfg->decimator_enable) {
        h->ip = sdro_backend_new_at(0.0f, (double)h->m_intTVSampleRate, 24, (double)(cfg->rf_bw / 2.2f), 3.0, 0.0f, 1.0f);
        h->m_nTaps = sdro_backend_ntaps(h->ip);
        h->m_samples.assign((size_t)2 * (h->m_nTaps + 2), 0.0f);
    }
    /* create_asym_filter(rf_opp_bw / tvRate, rf_bw / tvRate), the quotients floats */
    h->m_DSBFilter = 0;
    if (cfg->fft_filtering)
        h->m_DSBFilter = sdro_fftfilt_new_asym(cfg->rf_opp_bw / h->m_intTVSampleRate, cfg->rf_bw / h->m_intTVSampleRate, 2048);
    memset(h->m_DSBFilterBuffer, 0, sizeof h->m_DSBFilterBuffer);
    h->m_DSBFilterBufferIndex = 0;
    h->m_intImageIndex = 0; h->m_intSynchroPoints = 0;
    h->m_blnSynchroDetected = false; h->m_blnVerticalSynchroDetected = false;
    h->m_fltAmpLineAverage = 0.0f;
    h->m_fltEffMin = 2000000000.0f; h->m_fltEffMax = -2000000000.0f;
    h->m_fltAmpMin = -2000000000.0f; h->m_fltAmpMax = 2000000000.0f; h->m_fltAmpDelta = 1.0;
    memset(h->m_fltBufferI, 0, sizeof h->m_fltBufferI);
    memset(h->m_fltBufferQ, 0, sizeof h->m_fltBufferQ);
    h->m_intColIndex = 0; h->m_intSampleIndex = 0; h->m_intRowIndex = 0; h->m_intLineIndex = 0;
    h->m_intAvgColIndex = 0;
    h->screen.row = -1;
    h->screen.img.assign((size_t)h->screen.rows * h->screen.cols, 0);
    h->at = 0;
    memset(h->hits, 0, sizeof h->hits);
    h->renders_in_line = h->max_renders_in_line = 0;
    memset(h->geo, 0, sizeof h->geo);
    h->tick = 0; h->last_detection = -1; h->run_start = -1;
    return h;
}

void ato_destroy(void* p)
{
    Ato* h = (Ato*)p;
    if (!h) return;
    if (h->ip) sdro_backend_free(h->ip);
    if (h->m_DSBFilter) sdro_fftfilt_free(h->m_DSBFilter);
    delete h;
}

/* the decimator's phase-0 row (taps_cap floats at most) and the two spectra (2048 (re, im) pairs each); returns the taps per phase */
int ato_filters(void* p, float* taps, int taps_cap, float* filter, float* filter_opp)
{
    Ato* h = (Ato*)p;
    for (int i = 0; i < h->m_nTaps && i < taps_cap; i++) taps[i] = sdro_backend_taps(h->ip)[i];
    if (h->m_DSBFilter) {
        memcpy(filter, sdro_fftfilt_filter(h->m_DSBFilter), sizeof(float) * 2 * 2048);
        memcpy(filter_opp, sdro_fftfilt_filter_opp(h->m_DSBFilter), sizeof(float) * 2 * 2048);
    }
    return h->m_nTaps;
}

long ato_feed(void* p, const int16_t* iq, long n)
{
    Ato* h = (Ato*)p;
    h->events.clear(); h->frames.clear(); h->scope.clear();
    for (long j = 0; j < n; j++) {
        h->at = j;
        float cr = iq[2 * j], ci = iq[2 * j + 1];
        if (h->k.nco_freq != 0) {                               /* c *= m_nco.nextIQ() */
            h->phase += h->inc;
            while (h->phase >= 4096) h->phase -= 4096;
            while (h->phase < 0) h->phase += 4096;
            const float u = h->table[h->phase], v = -h->table[(h->phase + 1024) % 4096];
            const float x = cr * u - ci * v, y = cr * v + ci * u;
            cr = x; ci = y;
        }
        if (h->k.decimator_enable) {
            float rr, ri;
            if (h->decimate(&h->m_interpolatorDistanceRemain, cr, ci, &rr, &ri)) {
                h->demod(rr, ri);
                h->m_interpolatorDistanceRemain += h->m_interpolatorDistance;
            }
        } else {
            h->demod(cr, ci);
        }
    }
    return (long)h->events.size();
}

long ato_events(void* p, int32_t* out, long cap)
{
    Ato* h = (Ato*)p;
    const long n = (long)h->events.size();
    for (long i = 0; i < n && i < cap; i++) out[i] = h->events[(size_t)i];
    return n;
}

long ato_frame(void* p, long k, uint8_t* buf)
{
    Ato* h = (Ato*)p;
    if (k < 0 || k >= (long)h->frames.size()) return -1;
    memcpy(buf, h->frames[(size_t)k].data(), h->frames[(size_t)k].size());
    return (long)h->frames[(size_t)k].size();
}

long ato_screen(void* p, uint8_t* buf)
{
    Ato* h = (Ato*)p;
    memcpy(buf, h->screen.img.data(), h->screen.img.size());
    return (long)h->screen.img.size();
}

long ato_scope(void* p, int16_t* out, long cap)
{
    Ato* h = (Ato*)p;
    const long n = (long)h->scope.size();
    for (long i = 0; i < n && i < cap; i++) out[i] = h->scope[(size_t)i];
    return n;
}

void ato_state(void* p, sdrx_atv_state_t* s)
{
    Ato* h = (Ato*)p;
    s->image_index = h->m_intImageIndex; s->synchro_points = h->m_intSynchroPoints; s->synchro_detected = h->m_blnSynchroDetected;
    s->vertical_synchro_detected = h->m_blnVerticalSynchroDetected; s->col_index = h->m_intColIndex; s->sample_index = h->m_intSampleIndex;
    s->row_index = h->m_intRowIndex; s->line_index = h->m_intLineIndex; s->avg_col_index = h->m_intAvgColIndex; s->screen_row = h->screen.row;
    s->amp_line_average = bits(h->m_fltAmpLineAverage); s->eff_min = bits(h->m_fltEffMin); s->eff_max = bits(h->m_fltEffMax);
    s->amp_min = bits(h->m_fltAmpMin); s->amp_max = bits(h->m_fltAmpMax); s->amp_delta = bits(h->m_fltAmpDelta);
    for (int i = 0; i < 6; i++) { s->buffer_i[i] = bits(h->m_fltBufferI[i]); s->buffer_q[i] = bits(h->m_fltBufferQ[i]); }
}

void ato_design(void* p, sdrx_atv_design_t* d)
{
    Ato* h = (Ato*)p;
    d->samples_per_line = h->m_intNumberSamplePerLine; d->samples_per_top = h->m_intNumberSamplePerTop;
    d->samples_per_line_signals = h->m_intNumberSamplePerLineSignals; d->samples_per_hsync = h->m_intNumberSaplesPerHSync;
    d->sync_lines = h->m_intNumberOfSyncLines; d->black_lines = h->m_intNumberOfBlackLines; d->eq_lines = h->m_intNumberOfEqLines;
    d->interleaved = h->m_interleaved; d->tv_rate = h->m_intTVSampleRate; d->cols = h->screen.cols; d->rows = h->screen.rows;
    d->nco_inc = h->inc;
}

void ato_hits(void* p, int64_t* out)
{
    Ato* h = (Ato*)p;
    memcpy(out, h->hits, sizeof h->hits);
    out[ATV_N_HITS] = h->max_renders_in_line;
}

void ato_geo(void* p, int64_t* out)
{
    Ato* h = (Ato*)p;
    memcpy(out, h->geo, sizeof h->geo);
}

} // extern "C"
