/* Strict-IEEE C restatement of WFMDemod::feed with applyChannelSettings / applySettings
 * (plugins/channelrx/demodwfm/wfmdemod.cpp:90-183, 277-345), streaming, one demodulator per object: NCO, fftfilt::create_filter
 * with a negative f1 and runFilt (sdrbase/dsp/fftfilt.cpp:108-146, 261-282), the squelch counter, the gated
 * phaseDiscriminatorDelta (phasediscri.h:61-78, 172-197), Interpolator::create / decimate on a real signal
 * (interpolator.cpp:21-129, interpolator.h:23-36, 182-195) and the qint16 conversion.  The checker of sdrx_wfm_*: tests build
 * it with `cc -O2 -ffp-contract=off -shared` against oracle/libsdro.so (NCO table, NCO increment, g_fft) and call it through
 * ctypes; the product never links it.  m_prevArg starts at 0 (uninitialised in the reference, phasediscri.h:139);
 * m_movingAverage (GUI only) is left out.
 *
 *   wfo_create(in_rate, nco_freq, audio_rate, rf_bw, af_bw, volume, squelch_db, mute)
 *   wfo_feed(h, iq, n, audio, cap)        feed(); audio samples (the value written to .l and .r) go to audio, returns their count
 *   wfo_levels(h, &sum, &peak, &count)    m_magsqSum, m_magsqPeak, m_magsqCount
 *   wfo_squelch_open(h), wfo_squelch_state(h), wfo_count_ge(h) (samples at or above the squelch level: a test probe)
 *   wfo_design(h, taps[16 * ntaps], filter[2048], &nco_inc, &squelch_level)   returns taps per phase
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../oracle/sdro.h"

#define NCO_N 4096
#define FLEN 1024
#define FLEN2 512
#define PHASES 16
static const double PI_D = 3.14159265358979323846;

typedef struct { float r, i; } cf;

typedef struct {
    /* settings */
    float rf_bw, volume, squelch_level, fm_scaling;
    int mute;
    /* NCO */
    float nco[NCO_N];
    int nco_inc, nco_phase;
    /* fftfilt */
    cf filter[FLEN], data[FLEN], ovl[FLEN2], out[FLEN2];
    int inptr;
    /* squelch, discriminator, levels */
    int sq_state, sq_open;
    float prev_arg;
    double magsq_sum, magsq_peak;
    int magsq_count;
    long n_ge;                        /* samples with magsq >= m_squelchLevel (test probe) */
    /* Interpolator */
    int ntaps, ptr;
    float* taps;                      /* [phase][ntaps] */
    cf* ring;
    float distance, step;
} wfo;

static cf c_mul(cf a, cf b) { cf t; t.r = a.r * b.r - a.i * b.i; t.i = a.r * b.i + a.i * b.r; return t; }   /* std::complex<float> *= */

/* fftfilt.h:52-64: double expressions returned as float */
static float fsinc(float fc, int i, int len)
{
    const int len2 = len / 2;
    return (i == len2) ? (float)(2.0 * fc) : (float)(sin(2 * PI_D * fc * (i - len2)) / (PI_D * (i - len2)));
}
static float blackman(int i, int len)
{
    return (float)(0.42 - 0.50 * cos(2.0 * PI_D * i / len) + 0.08 * cos(4.0 * PI_D * i / len));
}

/* fftfilt::create_filter(f1, f2), any sign of f1 (fftfilt.cpp:108-146) */
static void create_filter(wfo* h, float f1, float f2)
{
    memset(h->filter, 0, sizeof h->filter);
    const int lp = f2 != 0, hp = f1 != 0;
    for (int i = 0; i < FLEN2; i++) {
        h->filter[i].r = 0; h->filter[i].i = 0;
        if (lp) h->filter[i].r += fsinc(f2, i, FLEN2);
        if (hp) h->filter[i].r -= fsinc(f1, i, FLEN2);
    }
    if (hp && f2 < f1) h->filter[FLEN2 / 2].r += 1;
    for (int i = 0; i < FLEN2; i++) { const float w = blackman(i, FLEN2); h->filter[i].r *= w; h->filter[i].i *= w; }
    sdro_gfft((float*)h->filter, FLEN, 0);
    float scale = 0;
    for (int i = 0; i < FLEN2; i++) { const float mag = hypotf(h->filter[i].r, h->filter[i].i); if (mag > scale) scale = mag; }   /* bins 0 .. flen2-1 only */
    if (scale != 0) for (int i = 0; i < FLEN; i++) { h->filter[i].r /= scale; h->filter[i].i /= scale; }
}

/* Interpolator::create(phaseSteps, sampleRate, cutoff, 4.5) */
static void interp_create(wfo* h, double sample_rate, double cutoff)
{
    const double tpp = 4.5;
    double gain = 1.0;
    const double fs = PHASES * sample_rate;
    int ntaps = (int)(tpp * PHASES);
    if (ntaps % 2) ntaps++;
    ntaps *= PHASES;
    float* taps = (float*)calloc((size_t)ntaps, sizeof(float));
    float* window = (float*)calloc((size_t)ntaps, sizeof(float));
    for (int n = 0; n < ntaps; n++) window[n] = (float)(0.54 - 0.46 * cos((2 * PI_D * n) / (ntaps - 1)));
    const int M = (ntaps - 1) / 2;
    const double fwT0 = 2 * PI_D * cutoff / fs;
    for (int n = -M; n <= M; n++) {
        if (n == 0) taps[n + M] = (float)(fwT0 / PI_D * window[n + M]);
        else taps[n + M] = (float)(sin(n * fwT0) / (n * PI_D) * window[n + M]);
    }
    double mx = taps[M];
    for (int n = 1; n <= M; n++) mx += 2.0 * taps[n + M];
    gain /= mx;
    for (int i = 0; i < ntaps; i++) taps[i] = (float)(taps[i] * gain);
    h->ntaps = ntaps / PHASES;
    h->taps = (float*)malloc(sizeof(float) * (size_t)ntaps);
    for (int ph = 0; ph < PHASES; ph++)
        for (int i = 0; i < h->ntaps; i++) h->taps[ph * h->ntaps + i] = taps[i * PHASES + ph];
    for (int ph = 0; ph < PHASES; ph++) {
        float sum = 0;
        for (int i = 0; i < h->ntaps; i++) sum += h->taps[ph * h->ntaps + i];
        for (int i = 0; i < h->ntaps; i++) h->taps[ph * h->ntaps + i] /= sum;
    }
    h->ring = (cf*)calloc((size_t)h->ntaps + 2, sizeof(cf));
    h->ptr = 0;
    free(taps); free(window);
}

/* phasediscri.h:172-197 */
static float atan2_approx2(float y, float x)
{
    const float PI_F = 3.14159265f, PIBY2_F = 1.5707963f;
    if (x == 0.0f) { if (y > 0.0f) return PIBY2_F; if (y == 0.0f) return 0.0f; return -PIBY2_F; }
    float at;
    const float z = y / x;
    if (fabsf(z) < 1.0f) {
        at = z / (1.0f + 0.28f * z * z);
        if (x < 0.0f) { if (y < 0.0f) return at - PI_F; return at + PI_F; }
    } else {
        at = PIBY2_F - z / (z * z + 0.28f);
        if (y < 0.0f) return at - PI_F;
    }
    return at;
}

/* (qint16) of a float on x86-64: cvttss2si (0x80000000 when out of range or NaN), then the low 16 bits */
static int16_t to_q16(float v)
{
    const int32_t i = (v >= -2147483648.0f && v < 2147483648.0f) ? (int32_t)v : (int32_t)0x80000000u;
    return (int16_t)(uint16_t)((uint32_t)i & 0xffffu);
}

wfo* wfo_create(int in_rate, int nco_freq, int audio_rate, float rf_bw, float af_bw, float volume, float squelch_db, int mute)
{
    wfo* h = (wfo*)calloc(1, sizeof *h);
    h->rf_bw = rf_bw; h->volume = volume; h->mute = mute;
    h->squelch_level = (float)pow(10.0, squelch_db / 10.0);
    sdro_nco_table(h->nco);
    h->nco_inc = sdro_nco_inc((float)nco_freq, (float)in_rate);           /* m_nco.setFreq(-inputFrequencyOffset, inputSampleRate) */
    interp_create(h, in_rate, af_bw);
    h->distance = (float)in_rate / (float)audio_rate;                     /* m_interpolatorDistanceRemain */
    h->step = (float)in_rate / (float)audio_rate;                         /* m_interpolatorDistance */
    const float low = (float)(-(rf_bw / 2.0) / in_rate), hi = (float)((rf_bw / 2.0) / in_rate);
    create_filter(h, low, hi);
    const float excursion = rf_bw / (float)in_rate;                       /* m_fmExcursion */
    h->fm_scaling = 1.0f / excursion;
    return h;
}

void wfo_destroy(wfo* h) { if (h) { free(h->taps); free(h->ring); free(h); } }

long wfo_feed(wfo* h, const int16_t* iq, long n, int16_t* audio, long cap)
{
    long n_out = 0;
    for (long k = 0; k < n; k++) {
        /* NCO::nextIQ: phase += inc, wrapped into [0, 4096) */
        h->nco_phase += h->nco_inc;
        while (h->nco_phase >= NCO_N) h->nco_phase -= NCO_N;
        while (h->nco_phase < 0) h->nco_phase += NCO_N;
        const cf osc = { h->nco[h->nco_phase], -h->nco[(h->nco_phase + NCO_N / 4) % NCO_N] };
        const cf s = { (float)iq[2 * k], (float)iq[2 * k + 1] };
        /* runFilt */
        h->data[h->inptr++] = c_mul(s, osc);
        if (h->inptr < FLEN2) continue;
        h->inptr = 0;
        sdro_gfft((float*)h->data, FLEN, 0);
        for (int i = 0; i < FLEN; i++) h->data[i] = c_mul(h->data[i], h->filter[i]);
        sdro_gfft((float*)h->data, FLEN, 1);
        for (int i = 0; i < FLEN2; i++) {
            h->out[i].r = h->ovl[i].r + h->data[i].r; h->out[i].i = h->ovl[i].i + h->data[i].i;
            h->ovl[i] = h->data[FLEN2 + i];
        }
        memset(h->data, 0, sizeof h->data);
        for (int i = 0; i < FLEN2; i++) {
            const cf rf = h->out[i];
            const double msq = rf.r * rf.r + rf.i * rf.i;                 /* float expression, widened */
            const float magsq = (float)(msq / (32768.0 * 32768.0));
            h->magsq_sum += magsq;
            if (magsq > h->magsq_peak) h->magsq_peak = magsq;
            h->magsq_count++;
            if (magsq >= h->squelch_level) {
                h->n_ge++;
                if (h->sq_state < h->rf_bw / 10) h->sq_state++;          /* int against float */
            } else {
                if (h->sq_state > 0) h->sq_state--;
            }
            h->sq_open = h->sq_state > (h->rf_bw / 20);
            float demod;
            if (h->sq_open && !h->mute) {
                const float cur = atan2_approx2(rf.i, rf.r);
                float dev = (float)((cur - h->prev_arg) / PI_D);
                h->prev_arg = cur;
                if (dev < -1.0f) dev += 2.0f; else if (dev > 1.0f) dev -= 2.0f;
                demod = dev * h->fm_scaling;
            } else {
                demod = 0;                                                /* m_prevArg is left alone */
            }
            /* Interpolator::decimate(&distance, Complex(demod, 0), &ci) */
            h->ptr--; if (h->ptr < 0) h->ptr = h->ntaps - 1;
            h->ring[h->ptr].r = demod; h->ring[h->ptr].i = 0;
            h->distance = (float)((double)h->distance - 1.0);
            if (h->distance >= 1.0) continue;
            int phase = (int)floor(h->distance * (float)PHASES);
            if (phase < 0) phase = 0;
            const float* c = h->taps + phase * h->ntaps;
            float ra = 0, ia = 0;
            int sp = h->ptr;
            for (int t = 0; t < h->ntaps; t++) {
                ra += c[t] * h->ring[sp].r;
                ia += c[t] * h->ring[sp].i;
                sp = (sp + 1) % h->ntaps;
            }
            (void)ia;
            const int16_t sample = to_q16(ra * 3276.8f * h->volume);
            if (n_out < cap) audio[n_out] = sample;
            n_out++;
            h->distance += h->step;
        }
    }
    return n_out;
}

void wfo_levels(const wfo* h, double* sum, double* peak, long* count)
{
    *sum = h->magsq_sum; *peak = h->magsq_peak; *count = h->magsq_count;
}
int wfo_squelch_open(const wfo* h) { return h->sq_open; }
int wfo_squelch_state(const wfo* h) { return h->sq_state; }
long wfo_count_ge(const wfo* h) { return h->n_ge; }

int wfo_design(const wfo* h, float* taps, float* filter, int* nco_inc, float* squelch_level)
{
    if (taps) memcpy(taps, h->taps, sizeof(float) * (size_t)(PHASES * h->ntaps));
    if (filter) memcpy(filter, h->filter, sizeof h->filter);
    if (nco_inc) *nco_inc = h->nco_inc;
    if (squelch_level) *squelch_level = h->squelch_level;
    return h->ntaps;
}
