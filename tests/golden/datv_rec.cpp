/* Recorder of the sample-rate half of DATVDemod (plugins/channelrx/demoddatv/datvdemod.cpp), down to p_symbols.  DATVDemod itself
 * drags in Qt threads, ffmpeg and a video player, so this is a program of its own: it CALLS the reference's classes, compiled
 * where they lie with strict-IEEE flags -- NCO (sdrbase/dsp/nco.cpp), fftfilt (sdrbase/dsp/fftfilt.cpp) and leansdr's headers
 * (scheduler, pipebuf, trig16, cstln_lut, the three samplers, filtergen, cstln_receiver, make_dvbs2_constellation) -- and copies
 * none of their text.  What is restated here is the WIRING alone: the objects and pipes InitDATVFramework constructs and the values
 * it gives them (datvdemod.cpp:422-667), InitDATVParameters' filter and oscillator (:208-211), and feed()'s loop with its stepping
 * rule (:826-859).  `private` is defined away around the leansdr headers so that the receiver's state can be read.
 *
 * The pipes behind the receiver get readers that drain them after every step: in DATVDemod p_freq, p_ss and p_mer have none and
 * empty themselves when full, which moves WHEN the receiver runs and not what it computes.  After each feed the scheduler is
 * stepped until nothing moves, then the feed is recorded.  `step N` replaces feed()'s rule by a step every N samples.
 *
 *   datv_rec IN OUT < commands      IN: int16 I/Q; OUT: the records below, in command order
 *     new msps sample_rate centre rf_bw symbol_rate modulation fec standard sampler rolloff excursion hard viterbi drift notch finfo
 *     step N                          (before the first feed; 0: feed()'s own rule)
 *     design                          6 floats, 5 int32, ncoeffs floats, trig 131072 floats, lut 65536 x 8 bytes, symbols 512 bytes
 *     feed N                          int64 n; n x int16 cost; n x uint8 symbol; int64 np; np x (re, im); int64 nm; nm x (freq, ss, mer);
 *                                     the state: 7 float words, meas_count, update_freq_phase, hist[k].p of the three, then hist[k].c (12 words), held (int32),
 *                                     chunks, n_in, n_symbols (int64)
 */
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <complex>
#include "dsp/nco.h"
#include "dsp/fftfilt.h"
#define private public
#define protected public
#include "leansdr/framework.h"
#include "leansdr/sdr.h"
#include "leansdr/dvb.h"
#include "leansdr/filtergen.h"
#undef private
#undef protected

using namespace leansdr;

namespace {

/* the fields of DATVDemod's config that InitDATVFramework reads on the way to p_symbols, with its constructor's values */
enum { SAMP_NEAREST = 0, SAMP_LINEAR = 1, SAMP_RRC = 2 };
struct Wiring {
    int sampler, buf_factor, rrc_steps;
    float Fs, Fm, rolloff, rrc_rej, Finfo;
    cstln_lut<256>::predef constellation;
    code_rate fec;
    bool allow_drift, hard_metric, viterbi;
    Wiring() : sampler(SAMP_NEAREST), buf_factor(4), rrc_steps(0), Fs(2.4e6), Fm(2e6), rolloff(0.35), rrc_rej(10), Finfo(5),
               constellation(cstln_lut<256>::QPSK), fec(FEC12), allow_drift(false), hard_metric(false), viterbi(false) {}
};
inline int decimation(float Fin, float Fout) { int d = Fin / Fout; return std::max(d, 1); }

struct Rec {
    Wiring cfg;
    int msps, centre, rf_bw, notch;
    NCO nco;
    fftfilt* rf;
    scheduler* sch;
    pipebuf<cf32>* p_rawiq;
    pipewriter<cf32>* p_rawiq_writer;
    pipebuf<softsymbol>* p_symbols;
    pipebuf<f32>* p_freq; pipebuf<f32>* p_ss; pipebuf<f32>* p_mer;
    pipebuf<cf32>* p_sampled;
    sampler_interface<f32>* sampler;
    float* coeffs_sampler; int ncoeffs_sampler;
    cstln_receiver<f32>* demod;
    pipereader<softsymbol>* r_symbols; pipereader<f32>* r_freq; pipereader<f32>* r_ss; pipereader<f32>* r_mer; pipereader<cf32>* r_sampled;
    long lngReadIQ;
    int step_every;
    std::vector<softsymbol> symbols; std::vector<cf32> points; std::vector<float> meas;
};

void drain(Rec& r)
{
    unsigned long n = r.r_symbols->readable();
    r.symbols.insert(r.symbols.end(), r.r_symbols->rd(), r.r_symbols->rd() + n); r.r_symbols->read(n);
    n = r.r_sampled->readable();
    r.points.insert(r.points.end(), r.r_sampled->rd(), r.r_sampled->rd() + n); r.r_sampled->read(n);
    n = r.r_freq->readable();                                   /* the three are written together */
    for (unsigned long i = 0; i < n; i++) { r.meas.push_back(r.r_freq->rd()[i]); r.meas.push_back(r.r_ss->rd()[i]); r.meas.push_back(r.r_mer->rd()[i]); }
    r.r_freq->read(n); r.r_ss->read(n); r.r_mer->read(n);
}

/* InitDATVParameters' two lines and InitDATVFramework down to the receiver */
void init(Rec& r)
{
    const int rfFilterFftLength = 1024;
    r.rf = new fftfilt(-256000.0 / 1000000.0, 256000.0 / 1000000.0, rfFilterFftLength);
    Real fltLowCut = -((float)r.rf_bw / 2.0) / (float)r.msps;
    Real fltHiCut = ((float)r.rf_bw / 2.0) / (float)r.msps;
    r.rf->create_filter(fltLowCut, fltHiCut);
    r.nco.setFreq(-(float)r.centre, (float)r.msps);

    Wiring& c = r.cfg;
    c.rrc_steps = 0;
    const unsigned long BUF_BASEBAND = 4096 * c.buf_factor, BUF_SYMBOLS = 1024 * c.buf_factor, BUF_SLOW = c.buf_factor;
    r.sch = new scheduler();
    r.p_rawiq = new pipebuf<cf32>(r.sch, "rawiq", BUF_BASEBAND);
    r.p_rawiq_writer = new pipewriter<cf32>(*r.p_rawiq);
    r.p_symbols = new pipebuf<softsymbol>(r.sch, "PSK soft-symbols", BUF_SYMBOLS);
    r.p_freq = new pipebuf<f32>(r.sch, "freq", BUF_SLOW);
    r.p_ss = new pipebuf<f32>(r.sch, "SS", BUF_SLOW);
    r.p_mer = new pipebuf<f32>(r.sch, "MER", BUF_SLOW);
    r.p_sampled = new pipebuf<cf32>(r.sch, "PSK symbols", BUF_BASEBAND);
    r.coeffs_sampler = 0; r.ncoeffs_sampler = 0;
    switch (c.sampler) {
    case SAMP_NEAREST: r.sampler = new nearest_sampler<float>(); break;
    case SAMP_LINEAR: r.sampler = new linear_sampler<float>(); break;
    default: {
        if (c.rrc_steps == 0) c.rrc_steps = std::max(1, (int)(64 * c.Fm / c.Fs));
        float Frrc = c.Fs * c.rrc_steps;
        float transition = (c.Fm / 2) * c.rolloff;
        int order = c.rrc_rej * Frrc / (22 * transition);
        r.ncoeffs_sampler = filtergen::root_raised_cosine(order, c.Fm / Frrc, c.rolloff, &r.coeffs_sampler);
        r.sampler = new fir_sampler<float, float>(r.ncoeffs_sampler, r.coeffs_sampler, c.rrc_steps);
    }
    }
    r.demod = new cstln_receiver<f32>(r.sch, r.sampler, *r.p_rawiq, *r.p_symbols, r.p_freq, r.p_ss, r.p_mer, r.p_sampled);
    r.demod->cstln = make_dvbs2_constellation(c.constellation, c.fec);
    if (!r.demod->cstln) { fprintf(stderr, "no constellation\n"); exit(3); }
    if (c.hard_metric) r.demod->cstln->harden();
    r.demod->set_omega(c.Fs / c.Fm);
    if (c.allow_drift) r.demod->set_allow_drift(true);
    if (c.viterbi) r.demod->pll_adjustment /= 6;
    r.demod->meas_decimation = decimation(c.Fs, c.Finfo);
    r.r_symbols = new pipereader<softsymbol>(*r.p_symbols);
    r.r_freq = new pipereader<f32>(*r.p_freq); r.r_ss = new pipereader<f32>(*r.p_ss); r.r_mer = new pipereader<f32>(*r.p_mer);
    r.r_sampled = new pipereader<cf32>(*r.p_sampled);
    r.lngReadIQ = 0;
}

/* A drained pipe keeps its write position until a writer that wants more than is left asks: writable() packs it then, and still
 * answers with the old room once.  The writer made here wants the whole pipe, so every drained pipe is empty again before the next
 * step.  In DATVDemod p_freq, p_ss and p_mer (4 slots, no reader) empty themselves when full; with a meas_decimation of 128 or
 * less the receiver asks for 2 slots, finds 1 left after three measurements and never runs again.  The recorder's readers and
 * this writer take that wiring accident away and nothing else: what the receiver computes per chunk is untouched. */
template <class T> void pack_if_full(pipebuf<T>* p) { pipewriter<T> w(*p, (unsigned long)(p->end - p->buf)); (void)w.writable(); }

void step(Rec& r)
{
    r.sch->step();
    drain(r);
    pack_if_full(r.p_symbols); pack_if_full(r.p_sampled); pack_if_full(r.p_freq); pack_if_full(r.p_ss); pack_if_full(r.p_mer);
}

/* feed()'s loop; the magnitude average is GUI only */
void feed(Rec& r, const int16_t* iq, long n)
{
    for (long j = 0; j < n; j++) {
        Complex objC((float)iq[2 * j], (float)iq[2 * j + 1]);
        objC *= r.nco.nextIQ();
        fftfilt::cmplx* objRF;
        int intRFOut = r.rf->runFilt(objC, &objRF);
        for (int i = 0; i < intRFOut; i++) {
            cf32 objIQ;
            objIQ.re = objRF->real();
            objIQ.im = objRF->imag();
            objRF++;
            r.p_rawiq_writer->write(objIQ);
            r.lngReadIQ++;
            const long room = (long)r.p_rawiq_writer->writable();         /* asked after every sample, as feed() does: it packs the pipe */
            const bool now = r.step_every ? (r.lngReadIQ >= r.step_every || room <= 1) : ((r.lngReadIQ + 1) >= room);
            if (now) {
                step(r);
                r.lngReadIQ = 0;
                delete r.p_rawiq_writer;
                r.p_rawiq_writer = new pipewriter<cf32>(*r.p_rawiq);
            }
        }
    }
    /* until nothing moves: a full pipe makes writable() pack it and still answer 0 once, so one idle step proves nothing */
    for (int idle = 0; idle < 2;) {
        const unsigned long long before = r.sch->hash();
        step(r);
        idle = r.sch->hash() == before ? idle + 1 : 0;
    }
}

uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
template <class T> void put(FILE* f, const T* p, size_t n) { if (n && fwrite(p, sizeof(T), n, f) != n) exit(4); }

} // namespace

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    FILE* fin = fopen(argv[1], "rb"); FILE* fout = fopen(argv[2], "wb");
    if (!fin || !fout) return 2;
    Rec* r = 0;
    int step_every = 0;
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        char cmd[32];
        if (sscanf(line, "%31s", cmd) != 1) continue;
        if (!strcmp(cmd, "new")) {
            r = new Rec;
            int sr, fm, mod, fec, std_, samp, exc, hard, vit, drift; float roll, finfo;
            if (sscanf(line, "%*s %d %d %d %d %d %d %d %d %d %f %d %d %d %d %d %f", &r->msps, &sr, &r->centre, &r->rf_bw, &fm, &mod, &fec, &std_, &samp,
                       &roll, &exc, &hard, &vit, &drift, &r->notch, &finfo) != 16) return 2;
            Wiring& c = r->cfg;
            (void)std_; c.fec = (code_rate)fec; c.Fs = (float)sr; c.Fm = (float)fm; c.sampler = samp;
            c.rolloff = roll; c.rrc_rej = (float)exc; c.allow_drift = drift; c.hard_metric = hard; c.viterbi = vit;
            if (finfo != 0.0f) c.Finfo = finfo;
            static const cstln_lut<256>::predef map[9] = { cstln_lut<256>::BPSK, cstln_lut<256>::QPSK, cstln_lut<256>::PSK8, cstln_lut<256>::APSK16,
                cstln_lut<256>::APSK32, cstln_lut<256>::APSK64E, cstln_lut<256>::QAM16, cstln_lut<256>::QAM64, cstln_lut<256>::QAM256 };
            c.constellation = map[mod];
            r->step_every = step_every;
            init(*r);
        } else if (!strcmp(cmd, "step")) {
            sscanf(line, "%*s %d", &step_every);
            if (r) r->step_every = step_every;
        } else if (!strcmp(cmd, "design")) {
            cstln_receiver<f32>* d = r->demod;
            const float freq_beta = 0.0012 / d->omega * d->pll_adjustment;
            const float fl[6] = { d->omega, d->min_omega, d->max_omega, d->min_freqw, d->max_freqw, freq_beta };
            const int32_t in[5] = { (int32_t)d->meas_decimation, r->ncoeffs_sampler ? r->cfg.rrc_steps : 0, r->ncoeffs_sampler, r->sampler->readahead(), d->cstln->nsymbols };
            put(fout, fl, 6); put(fout, in, 5); put(fout, r->coeffs_sampler, (size_t)r->ncoeffs_sampler);
            trig16* t = new trig16;
            put(fout, &t->lut[0].re, 2 * 65536);
            delete t;
            for (int I = 0; I < 256; I++)
                for (int Q = 0; Q < 256; Q++) {
                    cstln_lut<256>::result* e = d->cstln->lookup(I, Q);
                    uint8_t rec[8] = { 0 };
                    memcpy(rec, &e->ss.cost, 2); memcpy(rec + 2, &e->phase_error, 2); rec[4] = e->ss.symbol;
                    put(fout, rec, 8);
                }
            int8_t sy[512] = { 0 };
            for (int s = 0; s < d->cstln->nsymbols; s++) { sy[2 * s] = d->cstln->symbols[s].re; sy[2 * s + 1] = d->cstln->symbols[s].im; }
            put(fout, sy, 512);
        } else if (!strcmp(cmd, "feed")) {
            long n = 0;
            sscanf(line, "%*s %ld", &n);
            std::vector<int16_t> iq((size_t)2 * n + 2);
            if (n && fread(iq.data(), 4, (size_t)n, fin) != (size_t)n) return 5;
            r->symbols.clear(); r->points.clear(); r->meas.clear();
            feed(*r, iq.data(), n);
            int64_t k = (int64_t)r->symbols.size();
            put(fout, &k, 1);
            for (const softsymbol& s : r->symbols) put(fout, &s.cost, 1);
            for (const softsymbol& s : r->symbols) put(fout, &s.symbol, 1);
            k = (int64_t)r->points.size(); put(fout, &k, 1);
            for (const cf32& p : r->points) { put(fout, &p.re, 1); put(fout, &p.im, 1); }
            k = (int64_t)r->meas.size() / 3; put(fout, &k, 1);
            put(fout, r->meas.data(), r->meas.size());
            cstln_receiver<f32>* d = r->demod;
            uint32_t w[21];
            w[0] = bits(d->mu); w[1] = bits(d->phase); w[2] = bits(d->freqw); w[3] = bits(d->agc_gain);
            w[4] = bits(d->est_insp); w[5] = bits(d->est_sp); w[6] = bits(d->est_ep);
            w[7] = (uint32_t)d->meas_count;
            w[8] = r->ncoeffs_sampler ? (uint32_t)static_cast<fir_sampler<float, float>*>(r->sampler)->update_freq_phase : 0u;
            for (int h = 0; h < 3; h++) { w[9 + 2 * h] = bits(d->hist[h].p.re); w[10 + 2 * h] = bits(d->hist[h].p.im); w[15 + 2 * h] = bits(d->hist[h].c.re); w[16 + 2 * h] = bits(d->hist[h].c.im); }
            put(fout, w, 21);
            const int32_t held = (int32_t)d->in.readable();
            put(fout, &held, 1);
            const int64_t tail[3] = { (int64_t)(r->p_rawiq->total_read / 128), (int64_t)r->p_rawiq->total_written, (int64_t)r->p_symbols->total_written };
            put(fout, tail, 3);
        }
    }
    fclose(fout);
    return 0;
}
