/* Host check of sdrangel_amd/csrc/datv_scan.hpp and datv_design.hpp: the per-symbol and per-chunk step and the design, with a
 * scalar interp in place of the walk's lanes, on a trace of filtered samples (what p_rawiq is given; tests/datv_oracle.cpp's
 * dto_written) against the outputs the oracle gave for it.  A stand-alone program: tests/test_datv_host.py builds it plain and
 * with -fsanitize=address,undefined and runs it; nothing is preloaded.
 *
 *   datv_check TRACE      TRACE: sdrx_datv_cfg; int64 n, nsym, npts, nmeas; n (re, im) floats; nsym int16 cost; nsym uint8 symbol;
 *                         npts (re, im) as uint32; nmeas x 4 uint32 (freq_tap, est_insp, est_sp, est_ep); sdrx_datv_state_t
 *   exit 0 and "ok ..." where everything is equal, 1 with the first difference otherwise
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/sdrx.h"
#include "datv_design.hpp"

using namespace sdrx;

namespace {

template <class T> std::vector<T> take(FILE* f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short trace\n"); exit(2); }
    return v;
}
uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
int fail(const char* what, long at) { printf("FAIL %s at %ld\n", what, at); return 1; }

struct Rx {
    DatvDesign d; DatvState s;
    std::vector<float> trig, coeffs;
    DatvCstln c;
    std::vector<float> sh;                      /* shifted_coeffs as (re, im) */
    void shift(float freqw)
    {
        const float f = freqw / d.subsampling;
        for (int i = 0; i < d.ncoeffs; i++) {
            const unsigned a = datv_angle(-f * (i - d.ncoeffs / 2));
            sh[(size_t)2 * i] = trig[2 * a] * coeffs[(size_t)i]; sh[(size_t)2 * i + 1] = trig[2 * a + 1] * coeffs[(size_t)i];
        }
    }
    void interp(const float* pin, float* re, float* im) const
    {
        const unsigned a0 = datv_angle(-s.phase);
        const float er = trig[2 * a0], ei = trig[2 * a0 + 1];
        if (d.sampler == DATV_SAMP_NEAREST) { *re = pin[0] * er - pin[1] * ei; *im = pin[0] * ei + pin[1] * er; return; }
        if (d.sampler == DATV_SAMP_LINEAR) {
            const unsigned a1 = datv_angle(-(s.phase + s.sampler_freqw));
            const float fr = trig[2 * a1], fi = trig[2 * a1 + 1];
            const float s0r = pin[0] * er - pin[1] * ei, s0i = pin[0] * ei + pin[1] * er;
            const float s1r = pin[2] * fr - pin[3] * fi, s1i = pin[2] * fi + pin[3] * fr;
            *re = s0r * (1 - s.mu) + s1r * s.mu; *im = s0i * (1 - s.mu) + s1i * s.mu;
            return;
        }
        float ar = 0.0f, ai = 0.0f;
        const int start = datv_f2i((1 - s.mu) * d.subsampling);
        if (start >= 0)
            for (long pc = start; pc < d.ncoeffs; pc += d.subsampling, pin += 2) {
                ar += sh[(size_t)2 * pc] * pin[0] - sh[(size_t)2 * pc + 1] * pin[1];
                ai += sh[(size_t)2 * pc] * pin[1] + sh[(size_t)2 * pc + 1] * pin[0];
            }
        *re = er * ar - ei * ai; *im = er * ai + ei * ar;
    }
};

} // namespace

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const sdrx_datv_cfg k = take<sdrx_datv_cfg>(f, 1)[0];
    const std::vector<int64_t> cnt = take<int64_t>(f, 4);
    const std::vector<float> x = take<float>(f, (size_t)2 * cnt[0]);
    const std::vector<int16_t> cost = take<int16_t>(f, (size_t)cnt[1]);
    const std::vector<uint8_t> symbol = take<uint8_t>(f, (size_t)cnt[1]);
    const std::vector<uint32_t> pts = take<uint32_t>(f, (size_t)2 * cnt[2]);
    const std::vector<uint32_t> meas = take<uint32_t>(f, (size_t)4 * cnt[3]);
    const sdrx_datv_state_t want = take<sdrx_datv_state_t>(f, 1)[0];
    fclose(f);

    const DatvCfgView v = { k.msps, k.sample_rate, k.centre_frequency, k.rf_bandwidth, k.symbol_rate, k.modulation, k.fec, k.standard, k.sampler,
                            k.rolloff, k.excursion, k.hard_metric, k.viterbi, k.allow_drift, k.notch_filters, k.finfo };
    Rx r;
    const char* text = datv_design(v, r.d);
    if (text) { printf("FAIL refused: %s\n", text); return 1; }
    datv_fresh(r.d, r.s);
    datv_trig_table(r.trig);
    datv_constellation(k.modulation, k.fec, k.hard_metric != 0, r.c);
    if (r.d.sampler == DATV_SAMP_RRC) datv_rrc_coeffs(v, r.d, r.coeffs);
    r.sh.assign((size_t)2 * r.d.ncoeffs + 2, 0.0f);

    long n_sym = 0, n_pts = 0, n_meas = 0, at = 0;
    const long total = (long)cnt[0];
    while (total - at >= DATV_CHUNK + r.d.readahead) {
        if (r.d.sampler == DATV_SAMP_RRC) {
            r.s.update_freq_phase -= DATV_CHUNK;
            if (r.s.update_freq_phase <= 0) { r.s.update_freq_phase = r.d.ncoeffs * 16; r.s.sampler_freqw = r.s.freqw; r.s.coeffs_built = 1; r.shift(r.s.freqw); }
        } else if (r.d.sampler == DATV_SAMP_LINEAR) r.s.sampler_freqw = r.s.freqw;
        int had = 0, cre = 0, cim = 0;
        float sgre = 0, sgim = 0, sre = 0, sim = 0;
        for (int pin = 0; pin < DATV_CHUNK; pin++) {
            if (r.s.mu < 1) {
                r.interp(&x[(size_t)2 * (at + pin)], &sgre, &sgim);
                sre = sgre * r.s.agc_gain; sim = sgim * r.s.agc_gain;
                const DatvLutEntry& e = r.c.lut[datv_lut_index(sre, sim)];
                if (n_sym >= cnt[1] || e.cost != cost[(size_t)n_sym] || e.symbol != symbol[(size_t)n_sym]) return fail("symbol", n_sym);
                n_sym++;
                cre = r.c.symbols[2 * e.symbol]; cim = r.c.symbols[2 * e.symbol + 1];
                datv_symbol(r.d, r.s, sre, sim, e.phase_error, (float)cre, (float)cim, nullptr);
                had = 1;
            }
            r.s.mu = r.s.mu - 1;
            r.s.phase += r.s.freqw;
        }
        DatvMeas m[3];
        const int nm = datv_chunk_end(r.d, r.s, had, sgre, sgim, sre, sim, cre, cim, m, nullptr);
        if (had) {
            if (n_pts >= cnt[2] || bits(sre) != pts[(size_t)2 * n_pts] || bits(sim) != pts[(size_t)2 * n_pts + 1]) return fail("point", n_pts);
            n_pts++;
        }
        for (int j = 0; j < nm; j++, n_meas++) {
            if (n_meas >= cnt[3]) return fail("measurement count", n_meas);
            const uint32_t* w = &meas[(size_t)4 * n_meas];
            if (bits(m[j].freq_tap) != w[0] || bits(m[j].est_insp) != w[1] || bits(m[j].est_sp) != w[2] || bits(m[j].est_ep) != w[3]) return fail("measurement", n_meas);
        }
        at += DATV_CHUNK;
        r.s.chunks++;
    }
    if (n_sym != cnt[1] || n_pts != cnt[2] || n_meas != cnt[3]) return fail("counts", n_sym);
    const DatvState& s = r.s;
    const uint32_t got[9] = { bits(s.mu), bits(s.phase), bits(s.freqw), bits(s.agc_gain), bits(s.est_insp), bits(s.est_sp), bits(s.est_ep), s.meas_count, (uint32_t)s.update_freq_phase };
    const uint32_t exp[9] = { want.mu, want.phase, want.freqw, want.agc_gain, want.est_insp, want.est_sp, want.est_ep, want.meas_count, (uint32_t)want.update_freq_phase };
    for (int i = 0; i < 9; i++) if (got[i] != exp[i]) return fail("state word", i);
    for (int h = 0; h < 3; h++)
        if (bits(s.hist[h].pr) != want.hist_p[h][0] || bits(s.hist[h].pi) != want.hist_p[h][1] || bits(s.hist[h].cr) != want.hist_c[h][0] || bits(s.hist[h].ci) != want.hist_c[h][1])
            return fail("hist", h);
    if (total - at != want.held || s.chunks != want.chunks) return fail("held or chunks", total - at);
    printf("ok %ld symbols %ld points %ld measurements %lld chunks\n", n_sym, n_pts, n_meas, s.chunks);
    return 0;
}
