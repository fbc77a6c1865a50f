// What DATVDemod::InitDATVFramework (plugins/channelrx/demoddatv/datvdemod.cpp:422-667) designs before the first sample: the
// receiver's constants, trig16's table (leansdr/math.h:78-94), cstln_lut<256> for the nine constellations with
// make_dvbs2_constellation's radii (leansdr/sdr.h:362-681, dvb.h:33-106) and filtergen::root_raised_cosine's coefficients
// (filtergen.h:51-75).  Host code, no HIP header needed.  Every expression keeps the reference's widths: where it calls sqrt, sin
// or cos on a float inside namespace leansdr, <math.h> gives the float overloads.  sinf / cosf are pll_math.hpp's, atan2f is
// udp_atan2f, so the tables do not follow the machine's libm.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "datv_scan.hpp"
#include "pll_math.hpp"

namespace sdrx {

struct DatvCfgView {                        // sdrx_datv_cfg's fields the design reads
    int msps, sample_rate, centre_frequency, rf_bandwidth, symbol_rate, modulation, fec, standard, sampler;
    float rolloff;
    int excursion, hard_metric, viterbi, allow_drift, notch_filters;
    float finfo;
};

// make_dvbs2_constellation's radii; false where it fails ("Code rate not supported with APSK16 / APSK32")
inline bool datv_gammas(int modulation, int fec, float* g1, float* g2, float* g3)
{
    *g1 = *g2 = *g3 = 1;
    if (modulation == DATV_APSK16) {
        switch (fec) {
        case DATV_FEC23: case DATV_FEC46: *g1 = 3.15; break;
        case DATV_FEC34: *g1 = 2.85; break;
        case DATV_FEC45: *g1 = 2.75; break;
        case DATV_FEC56: *g1 = 2.70; break;
        case DATV_FEC89: *g1 = 2.60; break;
        case DATV_FEC910: *g1 = 2.57; break;
        default: return false;
        }
    } else if (modulation == DATV_APSK32) {
        switch (fec) {
        case DATV_FEC34: *g1 = 2.84; *g2 = 5.27; break;
        case DATV_FEC45: *g1 = 2.72; *g2 = 4.87; break;
        case DATV_FEC56: *g1 = 2.64; *g2 = 4.64; break;
        case DATV_FEC89: *g1 = 2.54; *g2 = 4.33; break;
        case DATV_FEC910: *g1 = 2.53; *g2 = 4.30; break;
        default: return false;
        }
    } else if (modulation == DATV_APSK64E) {
        *g1 = 2.4; *g2 = 4.3; *g3 = 7;
    }
    return true;
}

inline int datv_nsymbols(int modulation)
{
    static const int n[DATV_N_MOD] = { 2, 4, 8, 16, 32, 64, 16, 64, 256 };
    return n[modulation];
}

// the refusal's text, or nullptr; on success d holds the design
inline const char* datv_design(const DatvCfgView& k, DatvDesign& d)
{
    std::memset(&d, 0, sizeof d);
    if (k.msps <= 0 || k.sample_rate <= 0 || k.symbol_rate <= 0) return "msps, sample_rate and symbol_rate must be positive";
    if (k.symbol_rate > k.sample_rate) return "symbol_rate exceeds sample_rate (omega < 1)";
    if (k.rf_bandwidth < 0) return "negative rf_bandwidth";
    if (k.modulation < 0 || k.modulation >= DATV_N_MOD) return "no such modulation";
    if (k.fec < 0 || k.fec >= DATV_N_FEC) return "no such code rate";
    if (k.sampler < DATV_SAMP_NEAREST || k.sampler > DATV_SAMP_RRC) return "no such sampler";
    if (k.notch_filters > 0) return "notch_filters > 0: auto_notch is not part of the bank";
    if (!(k.finfo >= 0.0f)) return "bad finfo";
    float g1, g2, g3;
    if (!datv_gammas(k.modulation, k.fec, &g1, &g2, &g3))
        return k.modulation == DATV_APSK16 ? "Code rate not supported with APSK16" : "Code rate not supported with APSK32";
    const float Fs = (float)k.sample_rate, Fm = (float)k.symbol_rate;
    d.sampler = k.sampler; d.nsymbols = datv_nsymbols(k.modulation); d.allow_drift = k.allow_drift != 0;
    d.ncoeffs = 0; d.subsampling = 1; d.readahead = k.sampler == DATV_SAMP_LINEAR ? 1 : 0;
    if (k.sampler == DATV_SAMP_RRC) {
        if (!(k.rolloff > 0.0f)) return "rolloff <= 0 with the RRC sampler: its order is a division by zero";
        if (!(k.rolloff <= 1.0f) || k.excursion < 1) return "bad rolloff or excursion";
        const int rrc_steps = std::max(1, (int)(64 * Fm / Fs));
        const float Frrc = Fs * rrc_steps;
        const float transition = (Fm / 2) * k.rolloff;
        const float forder = (float)k.excursion * Frrc / (22 * transition);
        if (!(forder < 1.0e6f)) return "the RRC sampler has more than 4096 coefficients";
        const int order = (int)forder;
        const int ncoeffs = (order + 1) | 1;
        if (ncoeffs > DATV_NCOEFFS_MAX) return "the RRC sampler has more than 4096 coefficients";
        if ((ncoeffs + rrc_steps - 1) / rrc_steps > DATV_TAPS_MAX) return "the RRC sampler has more than 64 taps per symbol";
        d.ncoeffs = ncoeffs; d.subsampling = rrc_steps; d.readahead = ncoeffs - 1;
    }
    // set_omega(Fs / Fm) behind cstln: tol = 10e-6
    const float tol = 10e-6;
    d.omega = Fs / Fm;
    d.min_omega = d.omega * (1 - tol);
    d.max_omega = d.omega * (1 + tol);
    int n = 4;
    switch (d.nsymbols) { case 2: n = 2; break; case 4: n = 4; break; case 8: n = 8; break; case 16: n = 12; break; case 32: n = 16; break; default: n = 4; }
    const float freqw = 0.0f;
    d.min_freqw = freqw - 65536 / d.max_omega / n / 2;
    d.max_freqw = freqw + 65536 / d.max_omega / n / 2;
    float pll_adjustment = 1.0;
    if (k.viterbi) pll_adjustment /= 6;
    d.freq_alpha = 0.04;
    d.freq_beta = 0.0012 / d.omega * pll_adjustment;
    d.gain_mu = 0.02 / (75.0f * 75.0f) * 2;
    d.kest = 0.01;
    const float finfo = k.finfo == 0.0f ? 5.0f : k.finfo;
    const int dec = (int)std::min(2.0e9f, Fs / finfo);
    d.meas_decimation = (unsigned int)std::max(dec, 1);
    if (d.meas_decimation < (unsigned int)DATV_MEAS_MIN) return "meas_decimation under 64 (finfo too high)";
    return nullptr;
}

// trig16::trig16(): 65536 (cos, sin)
inline void datv_trig_table(std::vector<float>& t)
{
    t.resize(2 * 65536);
    for (int a = 0; a < 65536; ++a) {
        const float af = a * 2 * M_PI / 65536;
        t[(size_t)(2 * a)] = pll_cosf(af);
        t[(size_t)(2 * a + 1)] = pll_sinf(af);
    }
}

struct DatvCstln {
    int nsymbols;
    signed char symbols[2 * 256];
    std::vector<DatvLutEntry> lut;          // [I & 255][Q & 255]
};

namespace datv_detail {
inline void polar(DatvCstln& c, int s, float r, int n, float i)
{
    const float a = i * 2 * M_PI / n;
    c.symbols[2 * s] = (signed char)(r * pll_cosf(a) * 75.0f);
    c.symbols[2 * s + 1] = (signed char)(r * pll_sinf(a) * 75.0f);
}
inline void polar2(DatvCstln& c, int i, float r, float a0, float a1, float a2, float a3)
{
    const float a[] = { a0, a1, a2, a3 };
    for (int j = 0; j < 4; ++j) {
        const float phi = a[j] * M_PI;
        c.symbols[2 * (i + j)] = (signed char)(r * pll_cosf(phi) * 75.0f);
        c.symbols[2 * (i + j) + 1] = (signed char)(r * pll_sinf(phi) * 75.0f);
    }
}
inline void qam(DatvCstln& c, int n)
{
    const int m = (int)sqrtl(n);
    float scale;
    {
        const int q = m / 2;
        const float avgpower = 2 * (q * 0.25 + (q - 1) * (q / 2) + (q - 1) * q * (2 * q - 1) / 6) / q;
        scale = 1.0 / sqrtf(avgpower);
    }
    int s = 0;
    for (int x = 0; x < m; ++x)
        for (int y = 0; y < m; ++y) {
            const float I = x - (float)(m - 1) / 2;
            const float Q = y - (float)(m - 1) / 2;
            c.symbols[2 * s] = (signed char)(I * scale * 75.0f);
            c.symbols[2 * s + 1] = (signed char)(Q * scale * 75.0f);
            ++s;
        }
}
} // namespace datv_detail

// make_dvbs2_constellation(c, r), then harden() where hard_metric is set
inline void datv_constellation(int modulation, int fec, int hard_metric, DatvCstln& c)
{
    using namespace datv_detail;
    float gamma1, gamma2, gamma3;
    (void)datv_gammas(modulation, fec, &gamma1, &gamma2, &gamma3);
    std::memset(c.symbols, 0, sizeof c.symbols);
    c.nsymbols = datv_nsymbols(modulation);
    switch (modulation) {
    case DATV_BPSK: polar(c, 0, 1, 8, 1); polar(c, 1, 1, 8, 5); break;
    case DATV_QPSK: polar(c, 0, 1, 4, 0.5); polar(c, 1, 1, 4, 3.5); polar(c, 2, 1, 4, 1.5); polar(c, 3, 1, 4, 2.5); break;
    case DATV_PSK8: {
        static const int at[8] = { 1, 0, 4, 5, 2, 7, 3, 6 };
        for (int s = 0; s < 8; s++) polar(c, s, 1, 8, (float)at[s]);
        break;
    }
    case DATV_APSK16: {
        const float r1 = sqrtf(4 / (1 + 3 * gamma1 * gamma1));
        const float r2 = gamma1 * r1;
        static const float a12[12] = { 1.5, 10.5, 4.5, 7.5, 0.5, 11.5, 5.5, 6.5, 2.5, 9.5, 3.5, 8.5 };
        static const float a4[4] = { 0.5, 3.5, 1.5, 2.5 };
        for (int s = 0; s < 12; s++) polar(c, s, r2, 12, a12[s]);
        for (int s = 0; s < 4; s++) polar(c, 12 + s, r1, 4, a4[s]);
        break;
    }
    case DATV_APSK32: {
        const float r1 = sqrtf(8 / (1 + 3 * gamma1 * gamma1 + 4 * gamma2 * gamma2));
        const float r2 = gamma1 * r1;
        const float r3 = gamma2 * r1;
        static const float a12[8] = { 1.5, 2.5, 10.5, 9.5, 4.5, 3.5, 7.5, 8.5 };
        static const float a16[8] = { 1, 3, 14, 12, 6, 4, 9, 11 };
        for (int s = 0; s < 8; s++) polar(c, s, r2, 12, a12[s]);
        for (int s = 0; s < 8; s++) polar(c, 8 + s, r3, 16, a16[s]);
        static const float b12[4] = { 0.5, 11.5, 5.5, 6.5 };
        static const float b4[4] = { 0.5, 3.5, 1.5, 2.5 };
        for (int s = 0; s < 4; s++) { polar(c, 16 + 2 * s, r2, 12, b12[s]); polar(c, 17 + 2 * s, r1, 4, b4[s]); }
        static const float b16[8] = { 0, 2, 15, 13, 7, 5, 8, 10 };
        for (int s = 0; s < 8; s++) polar(c, 24 + s, r3, 16, b16[s]);
        break;
    }
    case DATV_APSK64E: {
        const float r1 = sqrtf(64 / (4 + 12 * gamma1 * gamma1 + 20 * gamma2 * gamma2 + 28 * gamma3 * gamma3));
        const float r2 = gamma1 * r1;
        const float r3 = gamma2 * r1;
        const float r4 = gamma3 * r1;
        polar2(c, 0, r4, 1.0 / 4, 7.0 / 4, 3.0 / 4, 5.0 / 4);
        polar2(c, 4, r4, 13.0 / 28, 43.0 / 28, 15.0 / 28, 41.0 / 28);
        polar2(c, 8, r4, 1.0 / 28, 55.0 / 28, 27.0 / 28, 29.0 / 28);
        polar2(c, 12, r1, 1.0 / 4, 7.0 / 4, 3.0 / 4, 5.0 / 4);
        polar2(c, 16, r4, 9.0 / 28, 47.0 / 28, 19.0 / 28, 37.0 / 28);
        polar2(c, 20, r4, 11.0 / 28, 45.0 / 28, 17.0 / 28, 39.0 / 28);
        polar2(c, 24, r3, 1.0 / 20, 39.0 / 20, 19.0 / 20, 21.0 / 20);
        polar2(c, 28, r2, 1.0 / 12, 23.0 / 12, 11.0 / 12, 13.0 / 12);
        polar2(c, 32, r4, 5.0 / 28, 51.0 / 28, 23.0 / 28, 33.0 / 28);
        polar2(c, 36, r3, 9.0 / 20, 31.0 / 20, 11.0 / 20, 29.0 / 20);
        polar2(c, 40, r4, 3.0 / 28, 53.0 / 28, 25.0 / 28, 31.0 / 28);
        polar2(c, 44, r2, 5.0 / 12, 19.0 / 12, 7.0 / 12, 17.0 / 12);
        polar2(c, 48, r3, 1.0 / 4, 7.0 / 4, 3.0 / 4, 5.0 / 4);
        polar2(c, 52, r3, 7.0 / 20, 33.0 / 20, 13.0 / 20, 27.0 / 20);
        polar2(c, 56, r3, 3.0 / 20, 37.0 / 20, 17.0 / 20, 23.0 / 20);
        polar2(c, 60, r2, 1.0 / 4, 7.0 / 4, 3.0 / 4, 5.0 / 4);
        break;
    }
    case DATV_QAM16: qam(c, 16); break;
    case DATV_QAM64: qam(c, 64); break;
    default: qam(c, 256); break;
    }
    // make_lut_from_symbols, R = 256
    const int R = 256;
    c.lut.assign((size_t)R * R, DatvLutEntry{});
    for (int I = -R / 2; I < R / 2; ++I)
        for (int Q = -R / 2; Q < R / 2; ++Q) {
            DatvLutEntry* pr = &c.lut[(size_t)(I & (R - 1)) * R + (size_t)(Q & (R - 1))];
            uint8_t nearest = 0;
            int32_t cost = R * R * 2, cost2 = R * R * 2;
            for (int s = 0; s < c.nsymbols; ++s) {
                const int re = c.symbols[2 * s], im = c.symbols[2 * s + 1];
                const int32_t d2 = (I - re) * (I - re) + (Q - im) * (Q - im);
                if (d2 < cost) { cost2 = cost; cost = d2; nearest = (uint8_t)s; }
                else if (d2 < cost2) cost2 = d2;
            }
            if (cost > 32767) cost = 32767;
            if (cost2 > 32767) cost2 = 32767;
            pr->cost = (int16_t)(cost - cost2);
            pr->symbol = nearest;
            const float ph_symbol = udp_atan2f(c.symbols[2 * nearest + 1], c.symbols[2 * nearest]);
            const float ph_err = udp_atan2f(Q, I) - ph_symbol;
            pr->phase_error = (int16_t)(int32_t)(ph_err * 65536 / (2 * M_PI));
            if (hard_metric) { if (pr->cost < 0) pr->cost = -1; if (pr->cost > 0) pr->cost = 1; }
        }
}

// filtergen::root_raised_cosine(order, Fm / Frrc, rolloff) as InitDATVFramework calls it; d.ncoeffs of them
inline void datv_rrc_coeffs(const DatvCfgView& k, const DatvDesign& d, std::vector<float>& coeffs)
{
    const float Fm = (float)k.symbol_rate, Frrc = (float)k.sample_rate * d.subsampling;
    const float Fs = Fm / Frrc;             // the function's own Fs
    const float B = k.rolloff, pi = M_PI;
    const int ncoeffs = d.ncoeffs;
    coeffs.resize((size_t)ncoeffs);
    for (int i = 0; i < ncoeffs; ++i) {
        const int t = i - ncoeffs / 2;
        float c;
        if (t == 0)
            c = sqrtf(Fs) * (1 - B + 4 * B / pi);
        else {
            const float tT = t * Fs;
            const float den = pi * tT * (1 - (4 * B * tT) * (4 * B * tT));
            if (!den)
                c = B * sqrtf(Fs / 2) * ((1 + 2 / pi) * pll_sinf(pi / (4 * B)) + (1 - 2 / pi) * pll_cosf(pi / (4 * B)));
            else
                c = sqrtf(Fs) * (pll_sinf(pi * tT * (1 - B)) + 4 * B * tT * pll_cosf(pi * tT * (1 + B))) / den;
        }
        coeffs[(size_t)i] = c;
    }
    // normalize_dcgain(ncoeffs, coeffs, 1)
    float s = 0, gain = 1;
    for (int i = 0; i < ncoeffs; ++i) s = s + coeffs[(size_t)i];
    if (s) gain /= s;
    for (int i = 0; i < ncoeffs; ++i) coeffs[(size_t)i] = coeffs[(size_t)i] * gain;
}

} // namespace sdrx
