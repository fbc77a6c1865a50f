/* Strict-IEEE C restatement of ChannelAnalyzer::feed, processOneSample and feedOneSample with m_pll, m_fll, m_pllPskOrder and
 * InputPLL (plugins/channelrx/chanalyzer/chanalyzer.cpp:92-182, chanalyzer.h:250-287), of PhaseLockComplex (sdrbase/dsp/
 * phaselockcomplex.cpp) and FreqLockComplex (freqlockcomplex.cpp), and of the state the constructor, applySettings(settings, true),
 * applyChannelSettings(in_rate, offset) and start() leave behind.  The front and fftcorr are tests/chana_oracle.c's, included as
 * text.  The checker of sdrx_chanapll_*: tests build it with `cc -O2 -ffp-contract=off -shared` and call it through ctypes; the
 * product never links it.
 *
 * The loops feed back, so no tolerance means anything and nothing here may come from whatever libm the machine has: the two loop
 * steps and the cosf, sinf and atan2f they call are written out in tests/pll_oracle.h, which tests/am_oracle.c includes too.
 *
 *   chapo_create(the 11 arguments of chao_create, pll, fll, psk_order)
 *   chapo_feed(h, iq, n, samples, cap)
 *   chapo_state(h, out[5])      isPllLocked, getPllFrequency, getPllDeltaPhase, getPllPhase as float bits in doubles' low words
 *                                (out[1..3] hold the uint32 bit patterns), out[4] = m_magsq
 *   chapo_probe(h, out[8])      saturations above / below, normalizeAngle with more than one turn, lock counter ups / downs,
 *                                cos / sin arguments past 120, arg(0), steps
 *   chapo_seek(h, filtered_samples)   chao_seek of the front; the loops do not depend on the stream position
 */
#include "chana_oracle.c"

#include "pll_oracle.h"

typedef struct { chao* a; loops l; int pll, fll; } chapo;

void* chapo_create(int in_rate, int nco_freq, int down_sample, int down_sample_rate, int bandwidth, int low_cutoff, int span_log2, int ssb, int rrc,
                   int rrc_rolloff, int input_type, int pll, int fll, int psk_order)
{
    chapo* h = (chapo*)calloc(1, sizeof(chapo));
    /* chao_create reads input_type only in its feed, which is not used here */
    h->a = (chao*)chao_create(in_rate, nco_freq, down_sample, down_sample_rate, bandwidth, low_cutoff, span_log2, ssb, rrc, rrc_rolloff, input_type);
    h->pll = pll; h->fll = fll;
    loops* l = &h->l;
    /* the constructors and the constructor of the analyzer at 48000 with the default settings */
    l->order = 1; l->lock_time = 480; l->lock_freq = 0.026f; l->y_re = 1.0f; l->f_y_re = 1.0f; l->f_a0 = 0.998; l->f_a1 = 0.002;
    pll_compute_coefficients(l, 0.002f, 0.5f, 10.0f);
    set_sample_rate(l, 48000 / (1 << 0));               /* applyChannelSettings(48000, 0, true) */
    set_sample_rate(l, 48000 / (1 << 0));               /* applySettings(defaults, true): m_downSample */
    set_sample_rate(l, 48000 / (1 << 0));               /*                                m_spanLog2 */
    l->order = 1;
    /* applySettings(settings, true): m_inputSampleRate is 48000, m_settings the defaults */
    {
        int rate = down_sample ? down_sample_rate : 48000;
        set_sample_rate(l, rate / (1 << span_log2));
        int rate2 = (down_sample ? (uint32_t)down_sample_rate : (uint32_t)48000) / (1 << 0);     /* :363, the settings before */
        set_sample_rate(l, rate2);
        if ((unsigned)psk_order < 32) l->order = psk_order > 0 ? (unsigned)psk_order : 1;
    }
    /* applyChannelSettings(in_rate, offset) and start() */
    if (!down_sample) {
        if (in_rate != 48000) set_sample_rate(l, in_rate / (1 << span_log2));
        set_sample_rate(l, in_rate / (1 << span_log2));
    }
    return h;
}

void chapo_destroy(void* p) { chapo* h = (chapo*)p; if (!h) return; chao_destroy(h->a); free(h); }

long chapo_feed(void* p, const int16_t* iq, long n, int16_t* out, long cap)
{
    chapo* g = (chapo*)p;
    chao* h = g->a;
    loops* l = &g->l;
    if (n > h->ci_cap) {
        free(h->ci); free(h->sb); h->ci_cap = n + 1024;
        h->ci = (float*)malloc(sizeof(float) * 2 * (size_t)h->ci_cap); h->sb = (float*)malloc(sizeof(float) * 2 * (size_t)(h->ci_cap + 2048));
    }
    long k = 0;
    for (long j = 0; j < n; j++) {
        const int phase = ncof_next_phase(h);
        const float or_ = g_ncof[phase], oi = -g_ncof[(phase + NCOF_N / 4) % NCOF_N];
        const float a = (float)iq[2 * j], b = (float)iq[2 * j + 1];
        cf c; c.r = a * or_ - b * oi; c.i = a * oi + b * or_;
        if (h->use_interp) {
            cf ci;
            if (interp_decimate(&h->ip, &h->remain, c, &ci)) {
                h->ci[2 * k] = ci.r; h->ci[2 * k + 1] = ci.i; k++;
                h->remain += h->distance;
            }
        } else { h->ci[2 * k] = c.r; h->ci[2 * k + 1] = c.i; k++; }
    }
    const long n_out = k > 0 ? (long)sdro_fftfilt_run(h->filt, h->filt_mode, h->ci, k, h->sb) : 0;
    const int decim = 1 << h->span_log2;
    long fill = 0;
    for (long i = 0; i < n_out; i++) {
        h->sum_re += h->sb[2 * i]; h->sum_im += h->sb[2 * i + 1];
        h->filtered++;
        if (!(h->undersample++ & (uint32_t)(decim - 1))) {
            h->sum_re /= decim; h->sum_im /= decim;
            float re = h->sum_re / 32768.0f;
            float im = h->sum_im / 32768.0f;
            h->magsq = re * re + im * im;
            cf s; s.r = h->sum_re; s.i = h->sum_im;
            cf mix; mix.r = 0; mix.i = 0;
            if (g->pll) {
                cf y;
                if (g->fll) { fll_feed(l, re, im); y.r = l->f_y_re; y.i = -l->f_y_im; }
                else { pll_feed(l, re, im); y.r = l->y_re; y.i = -l->y_im; }
                mix = c_mul(s, y);                          /* m_sum * std::conj(getComplex()) */
                l->probe[7]++;
                s = mix;
            }
            cf osc; osc.r = g->fll ? l->f_y_re : l->y_re; osc.i = g->fll ? l->f_y_im : l->y_im;
            if (h->input_type == 1) { s.r = osc.r * 32768.0f; s.i = osc.i * 32768.0f; }
            else if (h->input_type == 2) {
                cf q; q.r = s.r / (32768.0f / 768.0f); q.i = s.i / (32768.0f / 768.0f);
                s = corr_run(h, q);
            }
            if (fill < cap) {
                if (h->ssb & !h->usb) { out[2 * fill] = to_q16(s.i); out[2 * fill + 1] = to_q16(s.r); }
                else { out[2 * fill] = to_q16(s.r); out[2 * fill + 1] = to_q16(s.i); }
            }
            fill++;
            h->sum_re = 0; h->sum_im = 0;
        }
    }
    return fill;
}

void chapo_state(void* p, double* out)
{
    chapo* g = (chapo*)p;
    const loops* l = &g->l;
    const int locked = g->pll && (l->order > 1 ? l->lock_count > 10 : l->lock_count > l->lock_time - 2);
    out[0] = locked; out[1] = f_bits(l->freq); out[2] = f_bits(l->dphi); out[3] = f_bits(l->phi_hat); out[4] = g->a->magsq;
}

void chapo_probe(void* p, long* out) { memcpy(out, ((chapo*)p)->l.probe, sizeof(long) * 8); }

/* the stream position is the front's alone: the loop state does not depend on it */
void chapo_seek(void* p, uint64_t filtered) { chao_seek(((chapo*)p)->a, filtered); }
