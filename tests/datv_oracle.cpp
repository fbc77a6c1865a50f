/* Strict-IEEE scalar restatement of the sample-rate half of DATVDemod (plugins/channelrx/demoddatv/datvdemod.cpp:182-237, 422-667,
 * 767-863) with leansdr's trig16, cstln_lut<256>, make_dvbs2_constellation, the three samplers, filtergen::root_raised_cosine and
 * cstln_receiver<f32>::run (leansdr/math.h, sdr.h, dvb.h, filtergen.h), streaming, one receiver per object, in the reference's
 * statement order and with its member names.  The scheduler is gone: a chunk runs whenever 128 + readahead samples are there,
 * which is what p_symbols has received once the scheduler has run dry.  The NCO's table and increment, g_fft and runFilt are
 * oracle/libsdro.so's; create_filter with a negative f1 is restated here on sdro_gfft.  Nothing of the device code is used:
 * datv_scan.hpp is included for the enums and limits only.  The tables use this machine's sinf / cosf / atan2f, as the reference
 * does, unless dto_create is handed tables (the GPU parity tests hand it the bank's own, so that a libm difference shows in the
 * design test alone).  Tests build it with `g++ -O2 -ffp-contract=off -fno-fast-math -shared` (tests/datv_cases.py).
 *
 * Pinned as include/sdrx.h pins it: a float that no int32 holds converts to INT_MIN; lookup's loop stops after 300 halvings.
 *
 *   dto_create(cfg, trig, lut, symbols, coeffs)   a sdrx_datv_cfg and optional tables; NULL where sdrx_datv_create refuses it
 *   dto_feed(h, iq, n)                  feed(); returns the soft symbols of this feed
 *   dto_symbols(h, cost, symbol)        dto_points(h, iq) -> count      dto_meas(h, sdrx_datv_meas_t*) -> count
 *   dto_state(h, sdrx_datv_state_t*)    dto_design(h, sdrx_datv_design_t*)
 *   dto_tables(h, coeffs, trig, lut, symbols) -> ncoeffs
 *   dto_written(h, iq) -> count         the filtered samples the last feed handed to the receiver
 *   dto_hits(h, out[DTO_N_HITS])        the branch counters since creation (the HIT_ enum below)
 */
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/sdrx.h"
#include "../oracle/sdro.h"
#include "datv_scan.hpp"

namespace {

using namespace sdrx;

enum {
    HIT_CLAMP_LOW,          /* mucorr < -max_mucorr */
    HIT_CLAMP_HIGH,         /* mucorr > max_mucorr */
    HIT_DRIFT_RESET,        /* the !allow_drift limit put freqw back */
    HIT_TWO_MEAS,           /* a chunk that emitted two or more measurements */
    HIT_NO_SYMBOL,          /* a chunk without a symbol */
    HIT_MU_NEGATIVE,        /* interp with mu < 0 */
    HIT_HALVED,             /* lookup halved at least once */
    HIT_MAX_HALVINGS,       /* the most halvings one lookup needed (a maximum, not a count) */
    HIT_COEFFS_REBUILT,     /* do_update_freq */
    HIT_FEWER_TAPS,         /* fir interp whose start index exceeds subsampling */
    HIT_SYMBOLS,            /* soft symbols */
    HIT_MAX_TAPS,           /* the most taps one fir interp summed (a maximum, not a count) */
    DTO_N_HITS
};

const float cstln_amp = 75;

int f2i(float v) { if (v != v || v >= 2147483648.0f || v < -2147483648.0f) return INT_MIN; return (int)v; }

struct cf { float re, im; };
cf mul(cf a, cf b) { cf r = { a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re }; return r; }

struct Dto {
    sdrx_datv_cfg k;
    /* NCO, fftfilt */
    float table[4096];
    int nco_phase, nco_inc;
    sdro_fftfilt* m_objRFFilter;
    /* tables */
    std::vector<cf> trig;                       /* trig16::lut */
    std::vector<DatvLutEntry> lut;              /* cstln_lut<256>::lut[I][Q] at I * 256 + Q */
    signed char symbols[512];
    int nsymbols;
    /* fir_sampler */
    int sampler_kind, ncoeffs, subsampling, update_freq_phase;
    std::vector<float> coeffs;
    std::vector<cf> shifted_coeffs;
    float sampler_freqw;                        /* linear_sampler::freqw */
    /* cstln_receiver */
    unsigned long meas_decimation;
    float omega, min_omega, max_omega, freqw, min_freqw, max_freqw, pll_adjustment, kest;
    bool allow_drift;
    float est_insp, agc_gain, mu, phase, est_sp, est_ep, freq_tap;
    unsigned long meas_count;
    struct { cf p, c; } hist[3];
    std::vector<cf> in;                         /* p_rawiq: what the receiver has not read yet */
    std::vector<cf> written;                    /* what the last feed wrote to p_rawiq */
    long long chunks, n_in, n_symbols;
    /* per feed */
    std::vector<int16_t> cost; std::vector<uint8_t> symbol; std::vector<cf> points; std::vector<sdrx_datv_meas_t> meas;
    int64_t hits[DTO_N_HITS];

    int readahead() const { return sampler_kind == DATV_SAMP_RRC ? ncoeffs - 1 : (sampler_kind == DATV_SAMP_LINEAR ? 1 : 0); }
    cf expi(float a) const { return trig[(uint16_t)(int16_t)f2i(a)]; }

    void update_freq_limits()
    {
        int n = 4;
        switch (nsymbols) { case 2: n = 2; break; case 4: n = 4; break; case 8: n = 8; break; case 16: n = 12; break; case 32: n = 16; break; default: n = 4; break; }
        min_freqw = freqw - 65536 / max_omega / n / 2;
        max_freqw = freqw + 65536 / max_omega / n / 2;
    }
    void set_omega(float _omega, float tol = 10e-6)
    {
        omega = _omega;
        min_omega = omega * (1 - tol);
        max_omega = omega * (1 + tol);
        update_freq_limits();
    }

    void do_update_freq(float fw)
    {
        hits[HIT_COEFFS_REBUILT]++;
        float f = fw / subsampling;
        for (int i = 0; i < ncoeffs; ++i) {
            cf e = expi(-f * (i - ncoeffs / 2));
            shifted_coeffs[i].re = e.re * coeffs[i]; shifted_coeffs[i].im = e.im * coeffs[i];
        }
    }
    void update_freq(float fw)
    {
        if (sampler_kind == DATV_SAMP_LINEAR) sampler_freqw = fw;
        if (sampler_kind != DATV_SAMP_RRC) return;
        update_freq_phase -= 128;
        if (update_freq_phase <= 0) { update_freq_phase = ncoeffs * 16; do_update_freq(fw); }
    }
    cf interp(const cf* pin, float mu_, float phase_)
    {
        if (sampler_kind == DATV_SAMP_NEAREST) return mul(pin[0], expi(-phase_));
        if (sampler_kind == DATV_SAMP_LINEAR) {
            cf s0 = mul(pin[0], expi(-phase_));
            cf s1 = mul(pin[1], expi(-(phase_ + sampler_freqw)));
            cf r = { s0.re * (1 - mu_) + s1.re * mu_, s0.im * (1 - mu_) + s1.im * mu_ };
            return r;
        }
        cf acc = { 0, 0 };
        const int start = f2i((1 - mu_) * subsampling);
        if (start > subsampling) hits[HIT_FEWER_TAPS]++;
        if (start >= 0)
        {
            int taps = 0;
            for (long pc = start; pc < ncoeffs; pc += subsampling, ++pin, ++taps) { cf t = mul(shifted_coeffs[pc], *pin); acc.re += t.re; acc.im += t.im; }
            if (taps > hits[HIT_MAX_TAPS]) hits[HIT_MAX_TAPS] = taps;
        }
        return mul(expi(-phase_), acc);
    }
    const DatvLutEntry* lookup(float I, float Q)
    {
        int k = 0;
        while (k < 300 && (I < -128 || I > 127 || Q < -128 || Q > 127)) { I *= 0.5; Q *= 0.5; k++; }
        if (k) hits[HIT_HALVED]++;
        if (k > hits[HIT_MAX_HALVINGS]) hits[HIT_MAX_HALVINGS] = k;
        return &lut[(size_t)((uint8_t)(int8_t)f2i(I)) * 256 + (uint8_t)(int8_t)f2i(Q)];
    }

    /* one pass of run()'s outer loop: the caller has checked that chunk_size + readahead samples are there */
    void chunk(const cf* pin0)
    {
        float freq_alpha = 0.04;
        float freq_beta = 0.0012 / omega * pll_adjustment;
        float gain_mu = 0.02 / (cstln_amp * cstln_amp) * 2;
        update_freq(freqw);
        const cf* pin = pin0; const cf* pend = pin + 128;
        cf sg = { 0, 0 }, s = { 0, 0 };
        const signed char* cstln_point = NULL;
        while (pin < pend) {
            if (mu < 1) {
                if (mu < 0) hits[HIT_MU_NEGATIVE]++;
                sg = interp(pin, mu, phase);
                s.re = sg.re * agc_gain; s.im = sg.im * agc_gain;
                const DatvLutEntry* cr = lookup(s.re, s.im);
                cost.push_back(cr->cost); symbol.push_back(cr->symbol);
                hits[HIT_SYMBOLS]++;
                phase += cr->phase_error * freq_alpha;
                freqw += cr->phase_error * freq_beta;
                hist[2] = hist[1];
                hist[1] = hist[0];
                hist[0].p.re = s.re;
                hist[0].p.im = s.im;
                cstln_point = &symbols[2 * cr->symbol];
                hist[0].c.re = cstln_point[0];
                hist[0].c.im = cstln_point[1];
                float muerr = ((hist[0].p.re - hist[2].p.re) * hist[1].c.re + (hist[0].p.im - hist[2].p.im) * hist[1].c.im)
                            - ((hist[0].c.re - hist[2].c.re) * hist[1].p.re + (hist[0].c.im - hist[2].c.im) * hist[1].p.im);
                float mucorr = muerr * gain_mu;
                const float max_mucorr = 0.1;
                if (mucorr < -max_mucorr) { mucorr = -max_mucorr; hits[HIT_CLAMP_LOW]++; }
                if (mucorr > max_mucorr) { mucorr = max_mucorr; hits[HIT_CLAMP_HIGH]++; }
                mu += mucorr;
                mu += omega;
            }
            ++pin;
            --mu;
            phase += freqw;
        }
        phase = fmodf(phase, 65536);
        if (cstln_point) {
            points.push_back(s);
            float insp = sg.re * sg.re + sg.im * sg.im;
            est_insp = insp * kest + est_insp * (1 - kest);
            if (est_insp) agc_gain = cstln_amp / sqrtf(est_insp);
            cf ev = { s.re - cstln_point[0], s.im - cstln_point[1] };
            float sig_power, ev_power;
            if (nsymbols == 2) {
                float sig_real = (cstln_point[0] + cstln_point[1]) * 0.707;
                float ev_real = (ev.re + ev.im) * 0.707;
                sig_power = sig_real * sig_real;
                ev_power = ev_real * ev_real;
            } else {
                sig_power = (int)cstln_point[0] * cstln_point[0] + (int)cstln_point[1] * cstln_point[1];
                ev_power = ev.re * ev.re + ev.im * ev.im;
            }
            est_sp = sig_power * kest + est_sp * (1 - kest);
            est_ep = ev_power * kest + est_ep * (1 - kest);
        } else hits[HIT_NO_SYMBOL]++;
        if (!allow_drift) {
            if (freqw < min_freqw || freqw > max_freqw) { freqw = (max_freqw + min_freqw) / 2; hits[HIT_DRIFT_RESET]++; }
        }
        freq_tap = freqw / 65536;
        meas_count += 128;
        int emitted = 0;
        while (meas_count >= meas_decimation) {
            meas_count -= meas_decimation;
            sdrx_datv_meas_t m;
            m.freq = freq_tap;
            m.ss = sqrtf(est_insp);
            m.mer = est_ep ? 10 * logf(est_sp / est_ep) / logf(10) : 0;
            m.est_insp = est_insp; m.est_sp = est_sp; m.est_ep = est_ep;
            meas.push_back(m);
            emitted++;
        }
        if (emitted >= 2) hits[HIT_TWO_MEAS]++;
        chunks++;
    }
};

/* fftfilt.h's fsinc and _blackman, and create_filter(f1, f2) (fftfilt.cpp:108-146) for any sign of f1, on sdro_gfft */
float fsinc(float fc, int i, int len)
{
    const int len2 = len / 2;
    return (i == len2) ? (float)(2.0 * fc) : (float)(sin(2 * M_PI * fc * (i - len2)) / (M_PI * (i - len2)));
}
float blackman(int i, int len) { return (float)(0.42 - 0.50 * cos(2.0 * M_PI * i / len) + 0.08 * cos(4.0 * M_PI * i / len)); }

void create_filter(float f1, float f2, int flen, std::vector<float>& filter)
{
    const int flen2 = flen >> 1;
    filter.assign((size_t)2 * flen, 0.0f);
    const bool b_lowpass = (f2 != 0), b_highpass = (f1 != 0);
    for (int i = 0; i < flen2; i++) {
        float v = 0;
        if (b_lowpass) v += fsinc(f2, i, flen2);
        if (b_highpass) v -= fsinc(f1, i, flen2);
        filter[(size_t)2 * i] = v;
    }
    if (b_highpass && f2 < f1) filter[(size_t)2 * (flen2 / 2)] += 1;
    for (int i = 0; i < flen2; i++) { const float w = blackman(i, flen2); filter[(size_t)2 * i] *= w; filter[(size_t)2 * i + 1] *= w; }
    sdro_gfft(filter.data(), flen, 0);
    float scale = 0;
    for (int i = 0; i < flen2; i++) { const float mag = hypotf(filter[(size_t)2 * i], filter[(size_t)2 * i + 1]); if (mag > scale) scale = mag; }
    if (scale != 0) for (int i = 0; i < 2 * flen; i++) filter[(size_t)i] /= scale;
}

bool gammas(int c, int r, float* gamma1, float* gamma2, float* gamma3)
{
    *gamma1 = *gamma2 = *gamma3 = 1;
    if (c == DATV_APSK16) {
        switch (r) {
        case DATV_FEC23: case DATV_FEC46: *gamma1 = 3.15; break;
        case DATV_FEC34: *gamma1 = 2.85; break;
        case DATV_FEC45: *gamma1 = 2.75; break;
        case DATV_FEC56: *gamma1 = 2.70; break;
        case DATV_FEC89: *gamma1 = 2.60; break;
        case DATV_FEC910: *gamma1 = 2.57; break;
        default: return false;
        }
    } else if (c == DATV_APSK32) {
        switch (r) {
        case DATV_FEC34: *gamma1 = 2.84; *gamma2 = 5.27; break;
        case DATV_FEC45: *gamma1 = 2.72; *gamma2 = 4.87; break;
        case DATV_FEC56: *gamma1 = 2.64; *gamma2 = 4.64; break;
        case DATV_FEC89: *gamma1 = 2.54; *gamma2 = 4.33; break;
        case DATV_FEC910: *gamma1 = 2.53; *gamma2 = 4.30; break;
        default: return false;
        }
    } else if (c == DATV_APSK64E) { *gamma1 = 2.4; *gamma2 = 4.3; *gamma3 = 7; }
    return true;
}

struct Cstln {
    signed char* symbols; int nsymbols;
    void polar(int s, float r, int n, float i)
    {
        float a = i * 2 * M_PI / n;
        symbols[2 * s] = (signed char)(r * cosf(a) * cstln_amp); symbols[2 * s + 1] = (signed char)(r * sinf(a) * cstln_amp);
    }
    void polar2(int i, float r, float a0, float a1, float a2, float a3)
    {
        float a[] = { a0, a1, a2, a3 };
        for (int j = 0; j < 4; ++j) {
            float phi = a[j] * M_PI;
            symbols[2 * (i + j)] = (signed char)(r * cosf(phi) * cstln_amp); symbols[2 * (i + j) + 1] = (signed char)(r * sinf(phi) * cstln_amp);
        }
    }
    void make_qam(int n)
    {
        nsymbols = n;
        int m = sqrtl(n);
        float scale;
        {
            int q = m / 2;
            float avgpower = 2 * (q * 0.25 + (q - 1) * (q / 2) + (q - 1) * q * (2 * q - 1) / 6) / q;
            scale = 1.0 / sqrtf(avgpower);
        }
        int s = 0;
        for (int x = 0; x < m; ++x)
            for (int y = 0; y < m; ++y) {
                float I = x - (float)(m - 1) / 2;
                float Q = y - (float)(m - 1) / 2;
                symbols[2 * s] = (signed char)(I * scale * cstln_amp);
                symbols[2 * s + 1] = (signed char)(Q * scale * cstln_amp);
                ++s;
            }
    }
};

void make_constellation(int type, float gamma1, float gamma2, float gamma3, signed char* symbols, int* nsymbols)
{
    Cstln c; c.symbols = symbols; c.nsymbols = 0;
    memset(symbols, 0, 512);
    switch (type) {
    case DATV_BPSK: c.nsymbols = 2; c.polar(0, 1, 8, 1); c.polar(1, 1, 8, 5); break;
    case DATV_QPSK: c.nsymbols = 4; c.polar(0, 1, 4, 0.5); c.polar(1, 1, 4, 3.5); c.polar(2, 1, 4, 1.5); c.polar(3, 1, 4, 2.5); break;
    case DATV_PSK8:
        c.nsymbols = 8;
        c.polar(0, 1, 8, 1); c.polar(1, 1, 8, 0); c.polar(2, 1, 8, 4); c.polar(3, 1, 8, 5);
        c.polar(4, 1, 8, 2); c.polar(5, 1, 8, 7); c.polar(6, 1, 8, 3); c.polar(7, 1, 8, 6);
        break;
    case DATV_APSK16: {
        float r1 = sqrtf(4 / (1 + 3 * gamma1 * gamma1));
        float r2 = gamma1 * r1;
        c.nsymbols = 16;
        c.polar(0, r2, 12, 1.5); c.polar(1, r2, 12, 10.5); c.polar(2, r2, 12, 4.5); c.polar(3, r2, 12, 7.5);
        c.polar(4, r2, 12, 0.5); c.polar(5, r2, 12, 11.5); c.polar(6, r2, 12, 5.5); c.polar(7, r2, 12, 6.5);
        c.polar(8, r2, 12, 2.5); c.polar(9, r2, 12, 9.5); c.polar(10, r2, 12, 3.5); c.polar(11, r2, 12, 8.5);
        c.polar(12, r1, 4, 0.5); c.polar(13, r1, 4, 3.5); c.polar(14, r1, 4, 1.5); c.polar(15, r1, 4, 2.5);
        break;
    }
    case DATV_APSK32: {
        float r1 = sqrtf(8 / (1 + 3 * gamma1 * gamma1 + 4 * gamma2 * gamma2));
        float r2 = gamma1 * r1;
        float r3 = gamma2 * r1;
        c.nsymbols = 32;
        c.polar(0, r2, 12, 1.5); c.polar(1, r2, 12, 2.5); c.polar(2, r2, 12, 10.5); c.polar(3, r2, 12, 9.5);
        c.polar(4, r2, 12, 4.5); c.polar(5, r2, 12, 3.5); c.polar(6, r2, 12, 7.5); c.polar(7, r2, 12, 8.5);
        c.polar(8, r3, 16, 1); c.polar(9, r3, 16, 3); c.polar(10, r3, 16, 14); c.polar(11, r3, 16, 12);
        c.polar(12, r3, 16, 6); c.polar(13, r3, 16, 4); c.polar(14, r3, 16, 9); c.polar(15, r3, 16, 11);
        c.polar(16, r2, 12, 0.5); c.polar(17, r1, 4, 0.5); c.polar(18, r2, 12, 11.5); c.polar(19, r1, 4, 3.5);
        c.polar(20, r2, 12, 5.5); c.polar(21, r1, 4, 1.5); c.polar(22, r2, 12, 6.5); c.polar(23, r1, 4, 2.5);
        c.polar(24, r3, 16, 0); c.polar(25, r3, 16, 2); c.polar(26, r3, 16, 15); c.polar(27, r3, 16, 13);
        c.polar(28, r3, 16, 7); c.polar(29, r3, 16, 5); c.polar(30, r3, 16, 8); c.polar(31, r3, 16, 10);
        break;
    }
    case DATV_APSK64E: {
        float r1 = sqrtf(64 / (4 + 12 * gamma1 * gamma1 + 20 * gamma2 * gamma2 + 28 * gamma3 * gamma3));
        float r2 = gamma1 * r1;
        float r3 = gamma2 * r1;
        float r4 = gamma3 * r1;
        c.nsymbols = 64;
        c.polar2(0, r4, 1.0 / 4, 7.0 / 4, 3.0 / 4, 5.0 / 4);
        c.polar2(4, r4, 13.0 / 28, 43.0 / 28, 15.0 / 28, 41.0 / 28);
        c.polar2(8, r4, 1.0 / 28, 55.0 / 28, 27.0 / 28, 29.0 / 28);
        c.polar2(12, r1, 1.0 / 4, 7.0 / 4, 3.0 / 4, 5.0 / 4);
        c.polar2(16, r4, 9.0 / 28, 47.0 / 28, 19.0 / 28, 37.0 / 28);
        c.polar2(20, r4, 11.0 / 28, 45.0 / 28, 17.0 / 28, 39.0 / 28);
        c.polar2(24, r3, 1.0 / 20, 39.0 / 20, 19.0 / 20, 21.0 / 20);
        c.polar2(28, r2, 1.0 / 12, 23.0 / 12, 11.0 / 12, 13.0 / 12);
        c.polar2(32, r4, 5.0 / 28, 51.0 / 28, 23.0 / 28, 33.0 / 28);
        c.polar2(36, r3, 9.0 / 20, 31.0 / 20, 11.0 / 20, 29.0 / 20);
        c.polar2(40, r4, 3.0 / 28, 53.0 / 28, 25.0 / 28, 31.0 / 28);
        c.polar2(44, r2, 5.0 / 12, 19.0 / 12, 7.0 / 12, 17.0 / 12);
        c.polar2(48, r3, 1.0 / 4, 7.0 / 4, 3.0 / 4, 5.0 / 4);
        c.polar2(52, r3, 7.0 / 20, 33.0 / 20, 13.0 / 20, 27.0 / 20);
        c.polar2(56, r3, 3.0 / 20, 37.0 / 20, 17.0 / 20, 23.0 / 20);
        c.polar2(60, r2, 1.0 / 4, 7.0 / 4, 3.0 / 4, 5.0 / 4);
        break;
    }
    case DATV_QAM16: c.make_qam(16); break;
    case DATV_QAM64: c.make_qam(64); break;
    default: c.make_qam(256); break;
    }
    *nsymbols = c.nsymbols;
}

void make_lut_from_symbols(const signed char* symbols, int nsymbols, bool harden, std::vector<DatvLutEntry>& lut)
{
    const int R = 256;
    DatvLutEntry zero; memset(&zero, 0, sizeof zero);
    lut.assign((size_t)R * R, zero);
    for (int I = -R / 2; I < R / 2; ++I)
        for (int Q = -R / 2; Q < R / 2; ++Q) {
            DatvLutEntry* pr = &lut[(size_t)(I & (R - 1)) * R + (Q & (R - 1))];
            uint8_t nearest = 0;
            int32_t cost = R * R * 2, cost2 = R * R * 2;
            for (int s = 0; s < nsymbols; ++s) {
                int32_t d2 = (I - symbols[2 * s]) * (I - symbols[2 * s]) + (Q - symbols[2 * s + 1]) * (Q - symbols[2 * s + 1]);
                if (d2 < cost) { cost2 = cost; cost = d2; nearest = s; }
                else if (d2 < cost2) cost2 = d2;
            }
            if (cost > 32767) cost = 32767;
            if (cost2 > 32767) cost2 = 32767;
            pr->cost = cost - cost2;
            pr->symbol = nearest;
            float ph_symbol = atan2f(symbols[2 * pr->symbol + 1], symbols[2 * pr->symbol]);
            float ph_err = atan2f(Q, I) - ph_symbol;
            pr->phase_error = (int16_t)(int32_t)(ph_err * 65536 / (2 * M_PI));
            if (harden) { if (pr->cost < 0) pr->cost = -1; if (pr->cost > 0) pr->cost = 1; }
        }
}

int root_raised_cosine(int order, float Fs, float rolloff, std::vector<float>& coeffs)
{
    float B = rolloff, pi = M_PI;
    int ncoeffs = (order + 1) | 1;
    coeffs.resize((size_t)ncoeffs);
    for (int i = 0; i < ncoeffs; ++i) {
        int t = i - ncoeffs / 2;
        float c;
        if (t == 0) c = sqrtf(Fs) * (1 - B + 4 * B / pi);
        else {
            float tT = t * Fs;
            float den = pi * tT * (1 - (4 * B * tT) * (4 * B * tT));
            if (!den) c = B * sqrtf(Fs / 2) * ((1 + 2 / pi) * sinf(pi / (4 * B)) + (1 - 2 / pi) * cosf(pi / (4 * B)));
            else c = sqrtf(Fs) * (sinf(pi * tT * (1 - B)) + 4 * B * tT * cosf(pi * tT * (1 + B))) / den;
        }
        coeffs[i] = c;
    }
    float s = 0, gain = 1;
    for (int i = 0; i < ncoeffs; ++i) s = s + coeffs[i];
    if (s) gain /= s;
    for (int i = 0; i < ncoeffs; ++i) coeffs[i] = coeffs[i] * gain;
    return ncoeffs;
}

uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }

} // namespace

extern "C" {

void* dto_create(const sdrx_datv_cfg* cfg, const float* trig, const void* lut, const int8_t* symbols, const float* coeffs)
{
    const sdrx_datv_cfg& k = *cfg;
    if (k.msps <= 0 || k.sample_rate <= 0 || k.symbol_rate <= 0 || k.symbol_rate > k.sample_rate || k.rf_bandwidth < 0) return 0;
    if (k.modulation < 0 || k.modulation >= DATV_N_MOD || k.fec < 0 || k.fec >= DATV_N_FEC || k.sampler < 0 || k.sampler > 2) return 0;
    if (k.notch_filters > 0 || !(k.finfo >= 0.0f)) return 0;
    float gamma1, gamma2, gamma3;
    if (!gammas(k.modulation, k.fec, &gamma1, &gamma2, &gamma3)) return 0;
    Dto* h = new Dto;
    h->k = k;
    const float Fs = (float)k.sample_rate, Fm = (float)k.symbol_rate;
    h->sampler_kind = k.sampler; h->ncoeffs = 0; h->subsampling = 1; h->update_freq_phase = 0; h->sampler_freqw = 0;
    if (k.sampler == DATV_SAMP_RRC) {
        if (!(k.rolloff > 0.0f) || !(k.rolloff <= 1.0f) || k.excursion < 1) { delete h; return 0; }
        int rrc_steps = std::max(1, (int)(64 * Fm / Fs));
        float Frrc = Fs * rrc_steps;
        float transition = (Fm / 2) * k.rolloff;
        float forder = (float)k.excursion * Frrc / (22 * transition);
        if (!(forder < 1.0e6f)) { delete h; return 0; }
        int order = forder;
        h->ncoeffs = root_raised_cosine(order, Fm / Frrc, k.rolloff, h->coeffs);
        h->subsampling = rrc_steps;
        if (h->ncoeffs > DATV_NCOEFFS_MAX || (h->ncoeffs + rrc_steps - 1) / rrc_steps > DATV_TAPS_MAX) { delete h; return 0; }
        if (coeffs) memcpy(h->coeffs.data(), coeffs, (size_t)h->ncoeffs * 4);
        h->shifted_coeffs.assign((size_t)h->ncoeffs, cf{ 0, 0 });
    }
    const float finfo = k.finfo == 0.0f ? 5.0f : k.finfo;
    { int d = (int)std::min(2.0e9f, Fs / finfo); h->meas_decimation = (unsigned long)std::max(d, 1); }
    if (h->meas_decimation < (unsigned long)DATV_MEAS_MIN) { delete h; return 0; }
    /* the tables */
    h->trig.resize(65536);
    if (trig) memcpy(h->trig.data(), trig, 65536 * 8);
    else for (int a = 0; a < 65536; ++a) { float af = a * 2 * M_PI / 65536; h->trig[a].re = cosf(af); h->trig[a].im = sinf(af); }
    make_constellation(k.modulation, gamma1, gamma2, gamma3, h->symbols, &h->nsymbols);
    if (symbols) memcpy(h->symbols, symbols, 512);
    if (lut) { h->lut.resize(65536); memcpy(h->lut.data(), lut, 65536 * sizeof(DatvLutEntry)); }
    else make_lut_from_symbols(h->symbols, h->nsymbols, k.hard_metric != 0, h->lut);
    /* InitDATVParameters */
    sdro_nco_table(h->table);
    h->nco_phase = 0;
    h->nco_inc = sdro_nco_inc(-(float)k.centre_frequency, (float)k.msps);
    float fltLowCut = -((float)k.rf_bandwidth / 2.0) / (float)k.msps;
    float fltHiCut = ((float)k.rf_bandwidth / 2.0) / (float)k.msps;
    std::vector<float> filter;
    create_filter(fltLowCut, fltHiCut, 1024, filter);
    h->m_objRFFilter = sdro_fftfilt_new(0.1f, 0.2f, 1024);                  /* runFilt's carrier: its filter is replaced */
    memcpy(const_cast<float*>(sdro_fftfilt_filter(h->m_objRFFilter)), filter.data(), filter.size() * 4);
    /* cstln_receiver's constructor, then InitDATVFramework's settings */
    h->meas_count = 0; h->pll_adjustment = 1.0; h->allow_drift = false; h->kest = 0.01;
    h->est_insp = cstln_amp * cstln_amp; h->agc_gain = 1; h->mu = 0; h->phase = 0; h->est_sp = 0; h->est_ep = 0;
    h->freqw = 0;
    memset(h->hist, 0, sizeof h->hist);
    h->set_omega(Fs / Fm);
    if (k.allow_drift) h->allow_drift = true;
    if (k.viterbi) h->pll_adjustment /= 6;
    h->freq_tap = h->freqw / 65536;
    h->chunks = 0; h->n_in = 0; h->n_symbols = 0;
    memset(h->hits, 0, sizeof h->hits);
    return h;
}

void dto_destroy(void* p)
{
    Dto* h = (Dto*)p;
    if (!h) return;
    sdro_fftfilt_free(h->m_objRFFilter);
    delete h;
}

long dto_feed(void* p, const int16_t* iq, long n)
{
    Dto* h = (Dto*)p;
    h->cost.clear(); h->symbol.clear(); h->points.clear(); h->meas.clear(); h->written.clear();
    static float filtered[2 * 1024];
    for (long j = 0; j < n; j++) {
        float cr = iq[2 * j], ci = iq[2 * j + 1];
        h->nco_phase += h->nco_inc;
        while (h->nco_phase >= 4096) h->nco_phase -= 4096;
        while (h->nco_phase < 0) h->nco_phase += 4096;
        const float u = h->table[h->nco_phase], v = -h->table[(h->nco_phase + 1024) % 4096];
        const float in[2] = { cr * u - ci * v, cr * v + ci * u };
        const int n_out = (int)sdro_fftfilt_run(h->m_objRFFilter, 0, in, 1, filtered);
        for (int i = 0; i < n_out; i++) { cf s = { filtered[2 * i], filtered[2 * i + 1] }; h->in.push_back(s); h->written.push_back(s); }
        h->n_in += n_out;
    }
    size_t at = 0;
    const size_t need = 128 + (size_t)h->readahead();
    while (h->in.size() - at >= need) { h->chunk(h->in.data() + at); at += 128; }
    h->in.erase(h->in.begin(), h->in.begin() + (long)at);
    h->n_symbols += (long long)h->cost.size();
    return (long)h->cost.size();
}

void dto_symbols(void* p, int16_t* cost, uint8_t* symbol)
{
    Dto* h = (Dto*)p;
    if (!h->cost.empty()) { memcpy(cost, h->cost.data(), h->cost.size() * 2); memcpy(symbol, h->symbol.data(), h->symbol.size()); }
}
long dto_points(void* p, float* iq)
{
    Dto* h = (Dto*)p;
    if (iq && !h->points.empty()) memcpy(iq, h->points.data(), h->points.size() * 8);
    return (long)h->points.size();
}
/* the filtered samples the last feed handed to the receiver: the trace tests/datv_check.cpp runs on */
long dto_written(void* p, float* iq)
{
    Dto* h = (Dto*)p;
    if (iq && !h->written.empty()) memcpy(iq, h->written.data(), h->written.size() * 8);
    return (long)h->written.size();
}
long dto_meas(void* p, sdrx_datv_meas_t* out)
{
    Dto* h = (Dto*)p;
    if (out && !h->meas.empty()) memcpy(out, h->meas.data(), h->meas.size() * sizeof(sdrx_datv_meas_t));
    return (long)h->meas.size();
}

void dto_state(void* p, sdrx_datv_state_t* s)
{
    Dto* h = (Dto*)p;
    memset(s, 0, sizeof *s);
    s->mu = bits(h->mu); s->phase = bits(h->phase); s->freqw = bits(h->freqw); s->agc_gain = bits(h->agc_gain);
    s->est_insp = bits(h->est_insp); s->est_sp = bits(h->est_sp); s->est_ep = bits(h->est_ep);
    s->meas_count = (uint32_t)h->meas_count; s->update_freq_phase = h->update_freq_phase;
    for (int k = 0; k < 3; k++) {
        s->hist_p[k][0] = bits(h->hist[k].p.re); s->hist_p[k][1] = bits(h->hist[k].p.im);
        s->hist_c[k][0] = bits(h->hist[k].c.re); s->hist_c[k][1] = bits(h->hist[k].c.im);
    }
    s->held = (int32_t)h->in.size(); s->chunks = h->chunks; s->n_in = h->n_in; s->n_symbols = h->n_symbols;
}

void dto_design(void* p, sdrx_datv_design_t* d)
{
    Dto* h = (Dto*)p;
    d->omega = h->omega; d->min_omega = h->min_omega; d->max_omega = h->max_omega; d->min_freqw = h->min_freqw; d->max_freqw = h->max_freqw;
    d->freq_beta = 0.0012 / h->omega * h->pll_adjustment;
    d->meas_decimation = (int32_t)h->meas_decimation; d->rrc_steps = h->sampler_kind == DATV_SAMP_RRC ? h->subsampling : 0;
    d->ncoeffs = h->ncoeffs; d->readahead = h->readahead(); d->nsymbols = h->nsymbols; d->nco_inc = h->nco_inc;
}

int dto_tables(void* p, float* coeffs, float* trig, void* lut, int8_t* symbols)
{
    Dto* h = (Dto*)p;
    if (coeffs && h->ncoeffs) memcpy(coeffs, h->coeffs.data(), (size_t)h->ncoeffs * 4);
    if (trig) memcpy(trig, h->trig.data(), 65536 * 8);
    if (lut) memcpy(lut, h->lut.data(), 65536 * sizeof(DatvLutEntry));
    if (symbols) memcpy(symbols, h->symbols, 512);
    return h->ncoeffs;
}

void dto_hits(void* p, int64_t* out) { memcpy(out, ((Dto*)p)->hits, sizeof ((Dto*)p)->hits); }

} // extern "C"
