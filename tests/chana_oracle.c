/* Strict-IEEE C restatement of ChannelAnalyzer::feed, processOneSample and feedOneSample with m_pll off
 * (plugins/channelrx/chanalyzer/chanalyzer.cpp:92-182, chanalyzer.h:250-287) and of the state the constructor,
 * applySettings(settings, true), applyChannelSettings(in_rate, offset) and start() leave behind (:35-65, 247-392), streaming, one
 * analyzer per object, in the reference's statement order.  The Interpolator, fftfilt's block loop and g_fft are
 * oracle/sdro_float.c's, included as text so that its Interpolator can be fed with NCOF's output; restated here:
 *   NCOF      sdrbase/dsp/ncof.cpp, ncof.h:45-55     a float phase and a float increment, a table of 4097 entries
 *   frrc      sdrbase/dsp/fftfilt.h:68-87 with create_rrc_filter (fftfilt.cpp:223-246)
 *   fftcorr   sdrbase/dsp/fftcorr.cpp                run(inA, 0) on an 8192-point g_fft
 *   create_filter for a low cutoff of either sign (sdro_fftfilt_new reads a negative f1 as the DSB constructor)
 * The checker of sdrx_chana_*: tests build it with `cc -O2 -ffp-contract=off -shared` and call it through ctypes; the product
 * never links it.
 *
 *   chao_create(in_rate, nco_freq, down_sample, down_sample_rate, bandwidth, low_cutoff, span_log2, ssb, rrc, rrc_rolloff, input_type)
 *   chao_feed(h, iq, n, samples, cap)     feed(); returns the number of Samples
 *   chao_magsq(h)
 *   chao_seek(h, filtered_samples)        a fresh object whose filter has already put out that many samples of silence
 *   chao_state(h, out[4])                 m_undersampleCount (low 32 bits), fftcorr's inptrA, its completed blocks, filtered samples
 *   chao_design(h, taps, filter, &nco_inc)   returns taps per phase
 */
#include "../oracle/sdro_float.c"
#include <stdint.h>

#define NCOF_N 4096
#define CORR_N 8192

typedef struct {
    /* NCOF */
    float nco_inc, nco_phase;
    /* Interpolator */
    int use_interp;
    interp ip;
    float distance, remain;
    /* filters */
    sdro_fftfilt* filt; int filt_mode, flen;
    int ssb, usb, span_log2, input_type;
    float sum_re, sum_im; uint32_t undersample;
    double magsq;
    /* fftcorr */
    gfft cg; cf* dataA; cf* dataP; int inptrA, outptr; long blocks;
    long filtered;
    float* ci; float* sb; long ci_cap;
} chao;

static float g_ncof[NCOF_N + 1];
static int g_ncof_ok = 0;
static void ncof_init(void)
{
    if (g_ncof_ok) return;
    for (int i = 0; i <= NCOF_N; i++) g_ncof[i] = (float)cos((2.0 * 3.14159265358979323846 * i) / NCOF_N);
    g_ncof_ok = 1;
}

static int ncof_next_phase(chao* h)
{
    h->nco_phase += h->nco_inc;
    while (h->nco_phase >= (float)NCOF_N) h->nco_phase -= NCOF_N;
    while (h->nco_phase < 0.0) h->nco_phase += NCOF_N;
    return (int)h->nco_phase;
}

/* (qint16) of a float on x86-64: cvttss2si, low 16 bits */
static int16_t to_q16(float v)
{
    const int32_t i = (v >= -2147483648.0f && v < 2147483648.0f) ? (int32_t)v : (int32_t)0x80000000u;
    return (int16_t)(uint16_t)(uint32_t)i;
}

/* fftfilt::frrc */
static cf frrc(float fb, float a, int i, int len)
{
    cf r; r.i = 0.0f;
    float x = i / (float)len;
    x = 0.5 - fabs(x - 0.5);
    float tr = fb * a;
    if (x < fb - tr) r.r = 1.0;
    else if (x < fb + tr) {
        float y = ((x - (fb - tr)) / (2.0 * tr)) * 3.14159265358979323846;
        r.r = (cosf(y) + 1.0f) / 2.0f;                      /* C++ picks cos(float) */
    } else r.r = 0.0;
    return r;
}

static void create_rrc_filter(sdro_fftfilt* f, float fb, float a)
{
    for (int i = 0; i < f->flen; i++) f->filter[i] = frrc(fb, a, i, f->flen);
    float scale = 0;
    for (int i = 0; i < f->flen; i++) { const float mag = hypotf(f->filter[i].r, f->filter[i].i); if (mag > scale) scale = mag; }
    if (scale != 0) for (int i = 0; i < f->flen; i++) { f->filter[i].r /= scale; f->filter[i].i /= scale; }
}

/* fftfilt::create_filter (fftfilt.cpp:108-146) */
static void create_filter(sdro_fftfilt* f, float f1, float f2)
{
    memset(f->filter, 0, sizeof(cf) * (size_t)f->flen);
    const int lp = f2 != 0, hp = f1 != 0;
    for (int i = 0; i < f->flen2; i++) {
        f->filter[i].r = 0; f->filter[i].i = 0;
        if (lp) f->filter[i].r += fsinc(f2, i, f->flen2);
        if (hp) f->filter[i].r -= fsinc(f1, i, f->flen2);
    }
    if (hp && f2 < f1) f->filter[f->flen2 / 2].r += 1;
    for (int i = 0; i < f->flen2; i++) { const float w = blackman(i, f->flen2); f->filter[i].r *= w; f->filter[i].i *= w; }
    gfft_run(&f->g, f->filter, 0);
    float scale = 0;
    for (int i = 0; i < f->flen2; i++) { const float mag = hypotf(f->filter[i].r, f->filter[i].i); if (mag > scale) scale = mag; }
    if (scale != 0) for (int i = 0; i < f->flen; i++) { f->filter[i].r /= scale; f->filter[i].i /= scale; }
}

void* chao_create(int in_rate, int nco_freq, int down_sample, int down_sample_rate, int bandwidth, int low_cutoff, int span_log2, int ssb, int rrc,
                  int rrc_rolloff, int input_type)
{
    ncof_init();
    chao* h = (chao*)calloc(1, sizeof(chao));
    h->nco_inc = ((float)nco_freq * NCOF_N) / (float)in_rate;
    h->use_interp = down_sample != 0;
    interp_create(&h->ip, 16, in_rate, in_rate / 2.2f, 4.5);
    h->remain = 0;
    h->distance = (float)in_rate / (float)(uint32_t)down_sample_rate;
    /* setFilters(sampleRate, bandwidth, lowCutoff) */
    const int rate = down_sample ? down_sample_rate : in_rate;
    float band = bandwidth, low = low_cutoff;
    h->usb = 1;
    if (band < 0) { band = -band; low = -low; h->usb = 0; }
    if (band < 100.0f) { band = 100.0f; low = 0; }
    h->ssb = ssb; h->span_log2 = span_log2; h->input_type = input_type;
    if (ssb) {
        h->flen = 1024; h->filt = sdro_fftfilt_new(0.0f, 0.1f, 1024); h->filt_mode = h->usb ? 1 : 2;
        create_filter(h->filt, low / rate, band / rate);
    } else if (rrc) {
        h->flen = 2048; h->filt = sdro_fftfilt_new(-1.0f, band / rate, 2048); h->filt_mode = 0;
        /* with the Interpolator the last design is applySettings' own: the settings' bandwidth over a float rate */
        const float fb = down_sample ? bandwidth / (float)(uint32_t)down_sample_rate : band / rate;
        create_rrc_filter(h->filt, fb, (uint32_t)rrc_rolloff / 100.0);
    } else {
        h->flen = 2048; h->filt = sdro_fftfilt_new(-1.0f, band / rate, 2048); h->filt_mode = 3;
    }
    gfft_init(&h->cg, CORR_N);
    h->dataA = (cf*)calloc(CORR_N, sizeof(cf)); h->dataP = (cf*)calloc(CORR_N, sizeof(cf));
    return h;
}

void chao_destroy(void* p)
{
    chao* h = (chao*)p;
    if (!h) return;
    interp_free(&h->ip); sdro_fftfilt_free(h->filt);
    free(h->cg.u); free(h->dataA); free(h->dataP); free(h->ci); free(h->sb); free(h);
}

/* fftcorr::run(inA, 0) (fftcorr.cpp:61-111) */
static cf corr_run(chao* h, cf in)
{
    h->dataA[h->inptrA++] = in;
    if (h->inptrA >= CORR_N / 2) {
        gfft_run(&h->cg, h->dataA, 0);
        for (int i = 0; i < CORR_N; i++) {
            cf bj; bj.r = h->dataA[i].r; bj.i = -h->dataA[i].i;       /* std::conj */
            h->dataP[i] = c_mul(h->dataA[i], bj);
        }
        gfft_run(&h->cg, h->dataP, 1);
        memset(h->dataA, 0, sizeof(cf) * CORR_N);
        h->inptrA = 0;
        h->outptr = 0;
        h->blocks++;
    }
    return h->dataP[h->outptr++];
}

long chao_feed(void* p, const int16_t* iq, long n, int16_t* out, long cap)
{
    chao* h = (chao*)p;
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
    /* the filter's blocks come out in the order processOneSample meets them */
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
            if (h->input_type == 2) {
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

double chao_magsq(void* p) { return ((chao*)p)->magsq; }

void chao_seek(void* p, uint64_t filtered)
{
    chao* h = (chao*)p;
    const uint64_t decim = (uint64_t)1 << h->span_log2;
    const uint64_t calls = (filtered + decim - 1) / decim;
    h->undersample = (uint32_t)filtered;
    h->filtered = (long)filtered;
    if (h->input_type == 2) { h->inptrA = (int)(calls % (CORR_N / 2)); h->outptr = h->inptrA; }
}

void chao_state(void* p, double* out)
{
    chao* h = (chao*)p;
    out[0] = h->undersample; out[1] = h->inptrA; out[2] = h->blocks; out[3] = h->filtered;
}

int chao_design(void* p, float* taps, float* filter, float* nco_inc)
{
    chao* h = (chao*)p;
    memcpy(taps, h->ip.taps, sizeof(float) * 16 * (size_t)h->ip.ntaps);
    memcpy(filter, h->filt->filter, sizeof(float) * 2 * (size_t)h->flen);
    *nco_inc = h->nco_inc;
    return h->ip.ntaps;
}
