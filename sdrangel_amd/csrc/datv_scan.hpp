// The serial part of leansdr's cstln_receiver<f32>::run (plugins/channelrx/demoddatv/leansdr/sdr.h:943-1105) as DATVDemod wires
// it (datvdemod.cpp:422-667): what one symbol does to the loop (the AGC product, the table index, the two PLL adds, the modified
// Mueller and Mueller error with its clamp) and what the end of a 128-sample chunk does (fmodf, the AGC, the two estimates, the
// drift limit, freq_tap, the measurement counter).  The samplers' interp is the caller's: it is where the lanes help
// (datv_kernels.hpp).  Compiles for the host too (tests/datv_check.cpp), no HIP header needed.  On the device every lane of the
// channel's wave runs this with the same values.
//
// Every float expression keeps the reference's operand order and widths; the file is compiled with -ffp-contract=off.
// Pinned (include/sdrx.h): a float that no int32 holds, NaN included, converts to INT_MIN as cvttss2si does, so trig16::expi and
// cstln_lut::lookup index as on x86-64 for every input; lookup's halving loop stops after DATV_HALVINGS rounds, which no finite
// value needs, where the reference would spin on an infinity.
#pragma once
#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__)
#define DATV_HD __host__ __device__ __forceinline__
#else
#define DATV_HD inline
#endif

namespace sdrx {

enum { DATV_BPSK = 0, DATV_QPSK, DATV_PSK8, DATV_APSK16, DATV_APSK32, DATV_APSK64E, DATV_QAM16, DATV_QAM64, DATV_QAM256, DATV_N_MOD };  // DATVModulation
enum { DATV_SAMP_NEAREST = 0, DATV_SAMP_LINEAR = 1, DATV_SAMP_RRC = 2 };                                                           // dvb_sampler
enum { DATV_FEC12 = 0, DATV_FEC23, DATV_FEC46, DATV_FEC34, DATV_FEC56, DATV_FEC78, DATV_FEC45, DATV_FEC89, DATV_FEC910, DATV_N_FEC }; // leansdr::code_rate

constexpr int DATV_CHUNK = 128;             // cstln_receiver::chunk_size
constexpr int DATV_NCOEFFS_MAX = 4096;      // RRC coefficients a channel's wave keeps shifted in LDS
constexpr int DATV_TAPS_MAX = 64;           // taps of one interp: one lane each
constexpr int DATV_HOLD = DATV_CHUNK + DATV_NCOEFFS_MAX;    // filtered samples a channel can hold back: < 128 + readahead
constexpr int DATV_MEAS_MIN = 64;           // least meas_decimation: at most three measurements per chunk
constexpr int DATV_HALVINGS = 300;          // lookup's loop: 2^-300 brings every finite float under 128

struct DatvLutEntry {                       // cstln_lut<256>::result, 8 bytes: lut[(u8) I][(u8) Q] is entry I * 256 + Q
    int16_t cost;
    int16_t phase_error;
    uint8_t symbol;
    uint8_t pad[3];
};

struct DatvDesign {                         // what InitDATVFramework leaves in the receiver and its sampler
    int sampler, nsymbols, allow_drift;
    int ncoeffs, subsampling, readahead;    // fir_sampler's; 0, 1, 0 / 1 without it
    unsigned int meas_decimation;
    float omega, min_omega, max_omega;
    float min_freqw, max_freqw;
    float freq_alpha, freq_beta, gain_mu, kest;
};

struct DatvHist { float pr, pi, cr, ci; };  // hist[k].p, hist[k].c

struct DatvState {                          // cstln_receiver's members that move, and fir_sampler's throttle
    float mu, phase, freqw, agc_gain;
    float est_insp, est_sp, est_ep, freq_tap;
    unsigned int meas_count;
    int update_freq_phase;
    float sampler_freqw;                    // what the last do_update_freq (RRC) or update_freq (linear) was given
    int coeffs_built;                       // shifted_coeffs exists: rebuilt from sampler_freqw where a feed begins
    DatvHist hist[3];
    long long chunks;                       // chunks run since creation or reset
    int held;                               // filtered samples held back for the next chunk
    long long n_in, n_symbols;              // filtered samples taken, symbols written, since creation or reset
};

struct DatvMeas { float freq_tap, est_insp, est_sp, est_ep; };      // one measurement as the device leaves it

DATV_HD void datv_fresh(const DatvDesign&, DatvState& s)        // the constructors' values
{
    s.mu = 0.0f; s.phase = 0.0f; s.freqw = 0.0f; s.agc_gain = 1.0f;
    s.est_insp = 75.0f * 75.0f; s.est_sp = 0.0f; s.est_ep = 0.0f; s.freq_tap = 0.0f;
    s.meas_count = 0; s.update_freq_phase = 0; s.sampler_freqw = 0.0f; s.coeffs_built = 0;
    for (int k = 0; k < 3; k++) { s.hist[k].pr = s.hist[k].pi = s.hist[k].cr = s.hist[k].ci = 0.0f; }
    s.chunks = 0; s.held = 0; s.n_in = 0; s.n_symbols = 0;
}

// cvttss2si: what no int holds, NaN included, is INT_MIN
DATV_HD int datv_f2i(float v) { return (v >= -2147483648.0f && v < 2147483648.0f) ? (int)v : (int)0x80000000u; }

// trig16::expi(float): (uint16_t)(int16_t)(int32_t) a
DATV_HD unsigned int datv_angle(float a) { return (unsigned int)datv_f2i(a) & 0xffffu; }

// cstln_lut<256>::lookup(float I, float Q): the index of lut[(u8)(s8) I][(u8)(s8) Q]
DATV_HD unsigned int datv_lut_index(float I, float Q)
{
    for (int k = 0; k < DATV_HALVINGS && (I < -128 || I > 127 || Q < -128 || Q > 127); k++) {
        I = (float)(I * 0.5);
        Q = (float)(Q * 0.5);
    }
    return (((unsigned int)datv_f2i(I) & 0xffu) << 8) | ((unsigned int)datv_f2i(Q) & 0xffu);
}

// the mu < 1 branch behind interp and the look-up: s = sg * agc_gain is the caller's, (cr, ci) is symbols[ss.symbol]
DATV_HD void datv_symbol(const DatvDesign& d, DatvState& s, float sre, float sim, int phase_error, float cre, float cim, int* clamped)
{
    s.phase += phase_error * d.freq_alpha;
    s.freqw += phase_error * d.freq_beta;
    s.hist[2] = s.hist[1];
    s.hist[1] = s.hist[0];
    s.hist[0].pr = sre; s.hist[0].pi = sim;
    s.hist[0].cr = cre; s.hist[0].ci = cim;
    const float muerr = ((s.hist[0].pr - s.hist[2].pr) * s.hist[1].cr + (s.hist[0].pi - s.hist[2].pi) * s.hist[1].ci)
                      - ((s.hist[0].cr - s.hist[2].cr) * s.hist[1].pr + (s.hist[0].ci - s.hist[2].ci) * s.hist[1].pi);
    float mucorr = muerr * d.gain_mu;
    const float max_mucorr = 0.1f;
    if (mucorr < -max_mucorr) { mucorr = -max_mucorr; if (clamped) *clamped |= 1; }
    if (mucorr > max_mucorr) { mucorr = max_mucorr; if (clamped) *clamped |= 2; }
    s.mu += mucorr;
    s.mu += d.omega;
}

// behind a chunk's 128 samples.  had: a symbol fell into the chunk; sg, sv: the last one before and behind the AGC; (cre, cim):
// its constellation point.  Returns the measurements the chunk emits (0 .. 3), written to m; *reset: the drift limit fired.
DATV_HD int datv_chunk_end(const DatvDesign& d, DatvState& s, int had, float sgre, float sgim, float sre, float sim, int cre, int cim,
                           DatvMeas* m, int* reset)
{
    s.phase = fmodf(s.phase, 65536.0f);
    if (had) {
        const float insp = sgre * sgre + sgim * sgim;
        s.est_insp = insp * d.kest + s.est_insp * (1 - d.kest);
        if (s.est_insp) s.agc_gain = 75.0f / sqrtf(s.est_insp);
        const float evre = sre - cre, evim = sim - cim;
        float sig_power, ev_power;
        if (d.nsymbols == 2) {
            const float sig_real = (float)((cre + cim) * 0.707);
            const float ev_real = (float)((evre + evim) * 0.707);
            sig_power = sig_real * sig_real;
            ev_power = ev_real * ev_real;
        } else {
            sig_power = (float)(cre * cre + cim * cim);
            ev_power = evre * evre + evim * evim;
        }
        s.est_sp = sig_power * d.kest + s.est_sp * (1 - d.kest);
        s.est_ep = ev_power * d.kest + s.est_ep * (1 - d.kest);
    }
    if (!d.allow_drift) {
        if (s.freqw < d.min_freqw || s.freqw > d.max_freqw) { s.freqw = (d.max_freqw + d.min_freqw) / 2; if (reset) *reset = 1; }
    }
    s.freq_tap = s.freqw / 65536;
    s.meas_count += DATV_CHUNK;
    int n = 0;
    while (s.meas_count >= d.meas_decimation) {
        s.meas_count -= d.meas_decimation;
        m[n].freq_tap = s.freq_tap; m[n].est_insp = s.est_insp; m[n].est_sp = s.est_sp; m[n].est_ep = s.est_ep;
        n++;
    }
    return n;
}

// the host's half of a measurement: ss_out and mer_out (sdr.h:1097-1101).  logf of the quotient is the libm's of the process
// that calls this; logf(10) is a constant, folded by whichever compiler builds the caller (the reference's is folded the same way)
DATV_HD float datv_meas_ss(const DatvMeas& m) { return sqrtf(m.est_insp); }
DATV_HD float datv_meas_mer(const DatvMeas& m) { return m.est_ep ? 10 * logf(m.est_sp / m.est_ep) / logf(10) : 0; }

} // namespace sdrx
