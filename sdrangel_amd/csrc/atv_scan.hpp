// The part of ATVDemod that is neither the front nor the discriminators (plugins/channelrx/demodatv/atvdemod.cpp:411-443,
// atvdemod.h:498-744): AM's line-by-line normalisation, the inversion, the clamp, the scope Sample, the grey level, and the two
// sync state machines processClassic and processHSkip with the three calls they make on the screen.  Also applySettings' and
// applyStandard's integers (atvdemod.cpp:563-617, 681-732).  Compiles for the host too (tests/atv_check.cpp, tests/atv_oracle.cpp),
// no HIP header needed.  On the device the walk's wave runs atv_step, or for FM atv_sync alone, with wave-uniform values (atv_kernels.hpp).
//
// The screen is what TVScreen / GLShaderTVArray are to the demodulator (sdrgui/gui/glshadertvarray.cpp:294-328): a byte image of
// rows x cols grey levels and a current row.  selectRow in range sets the row, out of range makes it null (-1 here); setDataColor
// writes one pixel if the row is not null and the column is in range; renderImage is an event.  `Out` receives them:
//     out.pixel(row, col, grey)   out.render()   out.scope(sample)   out.hit(branch)
//
// Pinned where the reference leaves it open (include/sdrx.h): m_intAvgColIndex starts at 0; the screen starts as zeros with a null
// row; a float that no int holds, NaN included, converts to INT_MIN as on x86-64; a NaN in the state has x86-64's bits (atv_x86_nan).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ATV_HD __host__ __device__ __forceinline__
#else
#define ATV_HD inline
#endif

namespace sdrx {

enum { ATV_FM1 = 0, ATV_FM2 = 1, ATV_FM3 = 2, ATV_AM = 3, ATV_USB = 4, ATV_LSB = 5 };                       // ATVModulation
enum { ATV_STD_PAL625 = 0, ATV_STD_PAL525 = 1, ATV_STD_405 = 2, ATV_STD_SHORT_INTERLEAVED = 3, ATV_STD_SHORT = 4, ATV_STD_HSKIP = 5 };  // ATVStd

// the branches the cases have to reach (tests/atv_cases.py): indices of the oracle's counters
enum {
    ATV_HIT_HCORR_CLASSIC, ATV_HIT_HCORR_HSKIP, ATV_HIT_MINUS150, ATV_HIT_NO_HSYNC, ATV_HIT_ROW_NEG, ATV_HIT_ROW_BIG, ATV_HIT_COL_NEG,
    ATV_HIT_COL_BIG, ATV_HIT_VSYNC_EVEN, ATV_HIT_VSYNC_ODD, ATV_HIT_HALF_FRAME, ATV_HIT_HALF_FRAME_AM, ATV_HIT_DELTA_ONE, ATV_HIT_HSKIP_RENDER,
    ATV_HIT_NULL_ROW, ATV_N_HITS
};

struct AtvDesign {                          // one channel's configuration as the per-sample code reads it
    int modulation, hskip, hsync, vsync, invert, scope, interleaved;
    int n_lines, sync_lines, black_lines, eq_lines;
    int spl, spt, sp_signals, sp_hsync;     // m_intNumberSamplePerLine, ..PerTop, ..PerLineSignals, m_intNumberSaplesPerHSync
    int tv_rate, cols, rows;
    float level_top, level_black, fm_deviation;
};

struct AtvState {                           // the PROCESSING block of atvdemod.h and the screen's current row
    int image_index, synchro_points, synchro_detected, vsynchro_detected;
    int col_index, sample_index, row_index, line_index, avg_col_index;
    int screen_row;                         // -1: null
    float amp_line_average, eff_min, eff_max, amp_min, amp_max, amp_delta;
};

ATV_HD void atv_fresh(AtvState& s)          // the constructor's values
{
    s.image_index = 0; s.synchro_points = 0; s.synchro_detected = 0; s.vsynchro_detected = 0;
    s.col_index = 0; s.sample_index = 0; s.row_index = 0; s.line_index = 0; s.avg_col_index = 0;
    s.screen_row = -1;
    s.amp_line_average = 0.0f; s.eff_min = 2000000000.0f; s.eff_max = -2000000000.0f;
    s.amp_min = -2000000000.0f; s.amp_max = 2000000000.0f; s.amp_delta = 1.0f;
}

// cvttss2si: what no int holds, NaN included, is INT_MIN
ATV_HD int atv_f2i(float v) { return (v >= -2147483648.0f && v < 2147483648.0f) ? (int)v : (int)0x80000000u; }
// Every NaN of this pipeline is born of 0 / 0 (a (0, 0) sample normalised), which on x86-64 is the default NaN 0xffc00000, and SSE
// hands a NaN operand on as it is; the device's default NaN is 0x7fc00000 and a subtraction may flip the sign.  Where a NaN can
// reach the state it is therefore set to x86's.
ATV_HD float atv_x86_nan(float v)
{
    if (v == v) return v;
    union { unsigned u; float f; } x;
    x.u = 0xffc00000u;
    return x.f;
}
// a counter's ++ without the overflow being undefined
ATV_HD int atv_inc(int v) { return (int)((unsigned)v + 1u); }

// applyStandard and the integers of applySettings.  The durations are in seconds, as the GUI passes them.  Samples per line and
// per top come from the channel rate, and linesPerSecond is an int product with a float: both as written in the reference.
// Returns 0, or the number of the first thing that does not hold (atv_design_error has the text).
inline int atv_design(int in_rate, int modulation, int standard, int n_lines, float line_duration, float top_duration, float frames_per_s,
                      float level_top, float level_black, float fm_deviation, int hsync, int vsync, int invert, int scope, AtvDesign& d)
{
    if (in_rate <= 0) return 1;
    if (modulation == ATV_USB || modulation == ATV_LSB) return 2;
    if (modulation < 0 || modulation > ATV_LSB) return 3;
    if (standard < 0 || standard > ATV_STD_HSKIP) return 4;
    if (!(level_black < 1.0f)) return 5;
    if (n_lines < 1 || !(frames_per_s > 0.0f) || !((float)n_lines * frames_per_s < 2147483648.0f)) return 6;
    const int lines_per_second = (int)((float)n_lines * frames_per_s);          // int linesPerSecond = m_intNumberOfLines * m_fltFramePerS
    if (lines_per_second < 1) return 6;
    if (!(line_duration >= 0.0f) || !(top_duration >= 0.0f) || !(line_duration * (float)in_rate < 1.0e9f) || !(top_duration * (float)in_rate < 1.0e9f)) return 7;
    if (!(fm_deviation == fm_deviation) || fm_deviation == 0.0f) return 8;
    d.modulation = modulation; d.hskip = standard == ATV_STD_HSKIP; d.hsync = hsync != 0; d.vsync = vsync != 0; d.invert = invert != 0; d.scope = scope != 0;
    d.n_lines = n_lines; d.level_top = level_top; d.level_black = level_black; d.fm_deviation = fm_deviation;
    switch (standard) {
    case ATV_STD_HSKIP:             d.sync_lines = 0;  d.black_lines = 0;  d.eq_lines = 0; d.interleaved = 0; break;
    case ATV_STD_SHORT:             d.sync_lines = 4;  d.black_lines = 4;  d.eq_lines = 0; d.interleaved = 0; break;
    case ATV_STD_SHORT_INTERLEAVED: d.sync_lines = 4;  d.black_lines = 4;  d.eq_lines = 0; d.interleaved = 1; break;
    case ATV_STD_405:               d.sync_lines = 24; d.black_lines = 28; d.eq_lines = 3; d.interleaved = 1; break;
    case ATV_STD_PAL525:            d.sync_lines = 40; d.black_lines = 44; d.eq_lines = 3; d.interleaved = 1; break;
    default:                        d.sync_lines = 44; d.black_lines = 48; d.eq_lines = 3; d.interleaved = 1; break;
    }
    const int max_points = in_rate / lines_per_second;
    int i = max_points;
    for (; i > 0; i--)
        if (((long long)i * lines_per_second) % 10 == 0) break;
    const int per_unit = i == 0 ? max_points : i;
    d.tv_rate = per_unit * lines_per_second;
    if (d.tv_rate <= 0) d.tv_rate = in_rate;
    d.spl = (int)(line_duration * (float)in_rate);
    d.spt = (int)(top_duration * (float)in_rate);
    d.sp_signals = (int)((12.0f / 64.0f) * line_duration * (float)in_rate);
    d.sp_hsync = (int)((9.6f / 64.0f) * line_duration * (float)in_rate);
    d.cols = d.spl - d.sp_signals;
    d.rows = n_lines - d.black_lines;
    if (d.cols < 1 || d.rows < 1) return 9;
    return 0;
}

inline const char* atv_design_error(int e)
{
    switch (e) {
    case 1: return "bad rate (need in_rate >= 1)";
    case 2: return "modulations USB and LSB are left out (the BFO's phase lock and its filter)";
    case 3: return "bad modulation (0 FM1, 1 FM2, 2 FM3, 3 AM)";
    case 4: return "bad standard (0 .. 5)";
    case 5: return "level_black >= 1 divides the grey level by zero";
    case 6: return "n_lines * frames_per_s < 1";
    case 7: return "bad line or top duration";
    case 8: return "bad fm_deviation";
    case 9: return "the screen has no rows or no columns";
    default: return "";
    }
}

template <class Out> ATV_HD void atv_select_row(const AtvDesign& d, AtvState& s, int row, Out& out)
{
    if (row < 0) out.hit(ATV_HIT_ROW_NEG); else if (row >= d.rows) out.hit(ATV_HIT_ROW_BIG);
    s.screen_row = (row < d.rows && row >= 0) ? row : -1;
}
template <class Out> ATV_HD void atv_set_pixel(const AtvDesign& d, const AtvState& s, int col, int grey, Out& out)
{
    if (col < 0) out.hit(ATV_HIT_COL_NEG); else if (col >= d.cols) out.hit(ATV_HIT_COL_BIG);
    if (s.screen_row < 0) out.hit(ATV_HIT_NULL_ROW);
    if (col < d.cols && col >= 0 && s.screen_row >= 0) out.pixel(s.screen_row, col, grey);
}

// m_fltAmpMin / Max / Delta from the extrema of the line just ended, and fresh extrema
template <class Out> ATV_HD void atv_am_update(AtvState& s, Out& out)
{
    s.amp_min = s.eff_min; s.amp_max = s.eff_max;
    s.amp_delta = s.eff_max - s.eff_min;
    if (s.amp_delta <= 0.0f) { s.amp_delta = 1.0f; out.hit(ATV_HIT_DELTA_ONE); }
    s.eff_min = 2000000.0f; s.eff_max = -2000000.0f;
}

template <class Out> ATV_HD void atv_process_hskip(const AtvDesign& d, AtvState& s, float v, int grey, Out& out)
{
    atv_set_pixel(d, s, s.col_index - d.sp_hsync + d.spt, grey, out);
    if (v < d.level_top) s.synchro_points = atv_inc(s.synchro_points);
    else if (v > d.level_black) s.synchro_points = 0;
    s.synchro_detected = s.synchro_points == d.spt;
    if (s.synchro_detected) {
        if (s.sample_index >= (3 * d.spl) / 2) {            // first after skip
            s.avg_col_index = s.col_index;
            out.hit(ATV_HIT_HSKIP_RENDER);
            out.render();
            s.image_index = atv_inc(s.image_index);
            s.line_index = 0; s.row_index = 0;
        }
        s.sample_index = 0;
    } else {
        s.sample_index = atv_inc(s.sample_index);
    }
    if (s.col_index < d.spl + d.spt - 1) {
        s.col_index++;
    } else {
        if (d.hsync && s.line_index == 0) { s.col_index = d.spt + (d.spl - s.avg_col_index) / 2; out.hit(ATV_HIT_HCORR_HSKIP); }
        else s.col_index = d.spt;
        if (d.modulation == ATV_AM) atv_am_update(s, out);
        atv_select_row(d, s, s.row_index, out);
        s.line_index = atv_inc(s.line_index);
        s.row_index = atv_inc(s.row_index);
    }
}

template <class Out> ATV_HD void atv_process_classic(const AtvDesign& d, AtvState& s, float v, int grey, Out& out)
{
    const int sync_time = (3 * d.spl) / 4;
    const float trame_level = 0.5f * ((float)sync_time) * d.level_black;
    if (v < d.level_top) s.synchro_points = atv_inc(s.synchro_points);
    else if (v > d.level_black) s.synchro_points = 0;
    s.synchro_detected = s.synchro_points == d.spt;
    bool new_line = false;
    if (s.synchro_detected) {
        const bool early = s.col_index < d.spl / 2;
        if (early) out.hit(ATV_HIT_MINUS150);
        s.avg_col_index = s.sample_index - s.col_index - (early ? 150 : 0);
        s.sample_index = 0;
    } else {
        s.sample_index = atv_inc(s.sample_index);
    }
    if (!d.hsync && s.col_index >= d.spl) {
        s.col_index = 0;
        new_line = true;
    } else if (s.col_index >= d.spl + d.spt) {              // no valid H sync
        out.hit(ATV_HIT_NO_HSYNC);
        if (d.hsync && s.line_index == 0) { s.col_index = d.spt + s.avg_col_index / 4; out.hit(ATV_HIT_HCORR_CLASSIC); }
        else s.col_index = d.spt;
        new_line = true;
    }
    if (new_line) {
        if (d.modulation == ATV_AM) atv_am_update(s, out);
        s.amp_line_average = 0.0f;
        s.row_index += d.interleaved ? 2 : 1;
        if (s.row_index < d.n_lines) atv_select_row(d, s, s.row_index - d.sync_lines, out);
        s.line_index = atv_inc(s.line_index);
    }
    atv_set_pixel(d, s, s.col_index - d.sp_hsync + d.spt + 4, grey, out);
    s.col_index++;
    if (d.vsync && s.line_index < d.n_lines) {
        if (s.col_index >= sync_time) {
            if (s.amp_line_average <= trame_level) {
                s.amp_line_average = 0.0f;
                if (!s.vsynchro_detected) {
                    s.vsynchro_detected = 1;
                    if ((s.line_index % 2 == 0) || !d.interleaved) { out.hit(ATV_HIT_VSYNC_EVEN); out.render(); s.row_index = 1; }
                    else { out.hit(ATV_HIT_VSYNC_ODD); s.row_index = 0; }
                    atv_select_row(d, s, s.row_index - d.sync_lines, out);
                    s.line_index = 0;
                    s.image_index = atv_inc(s.image_index);
                }
            } else {
                s.vsynchro_detected = 0;
            }
        }
    } else if (s.line_index >= d.n_lines / 2) {             // no VSync or lines out of range => arbitrary
        out.hit(ATV_HIT_HALF_FRAME);
        if (s.image_index % 2 == 1) {
            out.render();
            if (d.modulation == ATV_AM) { out.hit(ATV_HIT_HALF_FRAME_AM); atv_am_update(s, out); }
            s.row_index = 1;
        } else {
            s.row_index = 0;
        }
        atv_select_row(d, s, s.row_index - d.sync_lines, out);
        s.line_index = 0;
        s.image_index = atv_inc(s.image_index);
    }
}

// One demodulated sample behind the discriminator, in four parts so that the device can take the three that hang on nothing but
// the sample itself out of the serial walk where the modulation allows it (FM: atv_kernels.hpp).
// 1. fltVal: `v` is FM's value (the deviation scaling applied) or AM's fltNorm / SDR_RX_SCALEF, which the extrema of the line follow
// and the extrema of the line before normalise; then the inversion and the clamp.  Only AM touches the state.
ATV_HD float atv_level(const AtvDesign& d, AtvState& s, float v)
{
    if (d.modulation == ATV_AM) {
        if (v < s.eff_min) s.eff_min = v;
        if (v > s.eff_max) s.eff_max = v;
        v -= s.amp_min;
        v /= s.amp_delta;
    }
    v = d.invert ? 1.0f - v : v;
    return (v < -1.0f) ? -1.0f : (v > 1.0f) ? 1.0f : v;
}
// 2. Sample(fltVal * SDR_RX_SCALEF, 0): through int32, the low 16 bits
ATV_HD int16_t atv_scope_sample(float v) { return (int16_t)(uint16_t)((unsigned)atv_f2i(v * 32768.0f) & 0xffffu); }
// 3. intVal = (int) 255.0*(fltVal - black) / (1.0f - black): the cast binds to 255.0, the rest is float
ATV_HD int atv_grey(const AtvDesign& d, float v)
{
    const int grey = atv_f2i(((float)255 * (v - d.level_black)) / (1.0f - d.level_black));
    return grey < 0 ? 0 : grey > 255 ? 255 : grey;
}
// 4. the running sum and the sync state machine
template <class Out> ATV_HD void atv_sync(const AtvDesign& d, AtvState& s, float v, int grey, Out& out)
{
    s.amp_line_average = atv_x86_nan(s.amp_line_average + v);
    if (d.hskip) atv_process_hskip(d, s, v, grey, out);
    else atv_process_classic(d, s, v, grey, out);
}
// all four in the reference's order
template <class Out> ATV_HD void atv_step(const AtvDesign& d, AtvState& s, float raw, Out& out)
{
    const float v = atv_level(d, s, raw);
    if (d.scope) out.scope(atv_scope_sample(v));
    atv_sync(d, s, v, atv_grey(d, v), out);
}

// the discriminators' value of one sample (atvdemod.cpp:279-332): (i, q) is the sample, h[k] the normalised sample k + 1 steps
// earlier (m_fltBufferI / Q [k]), n receives this sample's normalised value.  FM1 reads h[0 .. 1], FM2 h[1 .. 5].
struct AtvNorm { float i, q; };
ATV_HD AtvNorm atv_normalise(float i, float q)
{
    const double mag_sq = (double)(i * i + q * q);          // a double that holds a float sum
#if defined(__HIP_DEVICE_COMPILE__)
    const float norm = (float)__dsqrt_rn(mag_sq);
#else
    const float norm = (float)__builtin_sqrt(mag_sq);
#endif
    AtvNorm n; n.i = atv_x86_nan(i / norm); n.q = atv_x86_nan(q / norm);        // (0, 0): NaN, as in the reference
    return n;
}
ATV_HD float atv_fm1(AtvNorm n, AtvNorm h0, AtvNorm h1)
{
    float v = h0.i * (n.q - h1.q);
    v -= h0.q * (n.i - h1.i);
    v += 2.0f;
    v /= 4.0f;
    return v;
}
ATV_HD float atv_fm2(AtvNorm n, AtvNorm h1, AtvNorm h2, AtvNorm h3, AtvNorm h5)
{
    float v = h2.i * ((h5.q - n.q) / 16.0f + h1.q - h3.q);
    v -= h2.q * ((h5.i - n.i) / 16.0f + h1.i - h3.i);
    v += 2.125f;
    v /= 4.25f;
    return v;
}
ATV_HD float atv_fm_deviation(float v, float dev) { return dev != 1.0f ? ((v - 0.5f) / dev) + 0.5f : v; }
// AM's fltVal before the normalisation
ATV_HD float atv_am_raw(float i, float q)
{
    const double mag_sq = (double)(i * i + q * q);
#if defined(__HIP_DEVICE_COMPILE__)
    const float norm = (float)__dsqrt_rn(mag_sq);
#else
    const float norm = (float)__builtin_sqrt(mag_sq);
#endif
    return norm / 32768.0f;                                  // SDR_RX_SCALEF
}

} // namespace sdrx
