/* Strict-IEEE C restatement of AMDemod::feed / AMDemod::processOneSample in envelope mode (m_pll = false) with the derivations
 * of applyChannelSettings / applyAudioSampleRate / applySettings (plugins/channelrx/demodam/amdemod.cpp:101-276, 360-475),
 * streaming, one demodulator per object, in the reference's statement order with its containers as they are: the
 * MovingAverageUtil<Real, double, 16> fill-up and roll branches, the DoubleBufferFIFO with its doubled array, the
 * MovingAverage<double> ring of SimpleAGC, the Bandpass ring walk (bandpass.h:77-122), StepFunctions::smootherstep.
 * The front (NCO, Interpolator::create / decimate) is oracle/libsdro.so's sdro_backend_*.  The checker of sdrx_am_*: tests
 * build it with `cc -O2 -ffp-contract=off -shared` and call it through ctypes; the product never links it.
 * The delay line starts zeroed (DoubleBufferFIFO leaves it uninitialised; include/sdrx.h states the ruling).
 *
 *   amo_create(in_rate, nco_freq, audio_rate, rf_bw, volume, squelch_db, mute, bandpass)
 *   amo_feed(h, iq, n, audio, cap)        feed(); audio samples (the value written to .l and .r) go to audio, returns their count
 *   amo_levels(h, &magsq, &sum, &peak, &count)    m_magsq, m_magsqSum, m_magsqPeak, m_magsqCount
 *   amo_squelch_open(h), amo_squelch_count(h)
 *   amo_probe(h, out[10])                 test probes, see the enum below
 *   amo_design(h, taps[16 * ntaps], bandpass[151], &nco_inc, &squelch_level)   returns taps per phase
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../oracle/sdro.h"

#define MA_N 16
#define BP_TAPS 301
static const double PI_D = 3.14159265358979323846;

enum { P_TRANSITIONS, P_BELOW_CHANGES, P_COUNT_ZERO, P_COUNT_CAP, P_FED, P_OPEN_ROOT_ZERO, P_FIRST_OPEN, P_UNWRITTEN_READS, P_OPEN,
       P_FED_AFTER_CLOSURE, P_N };

typedef struct {
    sdro_backend* front;
    float* ci; long ci_cap;
    uint32_t rate;
    float level, volume;
    int mute, bandpass;
    /* MovingAverageUtil */
    float ma_samples[MA_N]; int ma_num; unsigned ma_index; double ma_total;
    double magsq, magsq_sum, magsq_peak; long magsq_count;
    /* DoubleBufferFIFO */
    float* dl; unsigned char* dl_written; int dl_size, dl_write, dl_cur;
    uint32_t sq_count; int sq_open;
    /* SimpleAGC: MovingAverage<double> */
    double* agc_hist; int agc_size; uint32_t agc_index; double agc_sum;
    /* Bandpass */
    float bp_taps[BP_TAPS / 2 + 1], bp_samples[BP_TAPS]; int bp_ptr;
    /* probes */
    long probe[P_N]; long n_audio; int last_below, closed_since_fed;
    int32_t nco_inc;
} amo;

static void bandpass_create(amo* h, int nTaps, double sampleRate, double lowCutoff, double highCutoff)
{
    const int nt = nTaps / 2 + 1;
    float lp[BP_TAPS / 2 + 1], hp[BP_TAPS / 2 + 1];
    const double Wcl = 2.0 * PI_D * lowCutoff / sampleRate, Wch = 2.0 * PI_D * highCutoff / sampleRate;
    const double mid = ((double)nTaps - 1.0) / 2.0;
    for (int i = 0; i < nt; i++) {
        if (i == (nTaps - 1) / 2) { lp[i] = (float)(Wch / PI_D); hp[i] = (float)(-(Wcl / PI_D)); }
        else { lp[i] = (float)(sin(((double)i - mid) * Wch) / (((double)i - mid) * PI_D)); hp[i] = (float)(-sin(((double)i - mid) * Wcl) / (((double)i - mid) * PI_D)); }
    }
    hp[(nTaps - 1) / 2] += 1;
    for (int i = 0; i < nt; i++) {
        lp[i] = (float)(lp[i] * (0.54 + 0.46 * cos((2.0 * PI_D * ((double)i - mid)) / (double)nTaps)));
        hp[i] = (float)(hp[i] * (0.54 + 0.46 * cos((2.0 * PI_D * ((double)i - mid)) / (double)nTaps)));
        h->bp_taps[i] = -(lp[i] + hp[i]);
    }
    h->bp_taps[(nTaps - 1) / 2] += 1;
    float sum = 0; int i;
    for (i = 0; i < nt - 1; i++) sum += h->bp_taps[i] * 2;
    sum += h->bp_taps[i];
    for (i = 0; i < nt; i++) h->bp_taps[i] /= sum;
    memset(h->bp_samples, 0, sizeof h->bp_samples);
    h->bp_ptr = 0;
}

static float bandpass_filter(amo* h, float sample)
{
    float acc = 0;
    int a = h->bp_ptr, b = a - 1, i;
    const int size = BP_TAPS, n_taps = BP_TAPS / 2;
    h->bp_samples[h->bp_ptr] = sample;
    while (b < 0) b += size;
    for (i = 0; i < n_taps; i++) {
        acc += (h->bp_samples[a] + h->bp_samples[b]) * h->bp_taps[i];
        a++; while (a >= size) a -= size;
        b--; while (b < 0) b += size;
    }
    acc += h->bp_samples[a] * h->bp_taps[i];
    h->bp_ptr++; while (h->bp_ptr >= size) h->bp_ptr -= size;
    return acc;
}

static float smootherstep(float x)
{
    if (x == 1.0f) return 1.0f; else if (x == 0.0f) return 0.0f;
    double x3 = x * x * x;
    double x4 = x * x3;
    double x5 = x * x4;
    return (float)(6.0 * x5 - 15.0 * x4 + 10.0 * x3);
}

/* (qint16) of a float on x86-64: cvttss2si, low 16 bits */
static int16_t to_q16(float v)
{
    const int32_t i = (v >= -2147483648.0f && v < 2147483648.0f) ? (int32_t)v : (int32_t)0x80000000u;
    return (int16_t)(uint16_t)(uint32_t)i;
}

void* amo_create(int in_rate, int nco_freq, int audio_rate, float rf_bw, float volume, float squelch_db, int mute, int bandpass)
{
    amo* h = (amo*)calloc(1, sizeof(amo));
    h->rate = (uint32_t)audio_rate;
    h->front = sdro_backend_new((float)nco_freq, (float)in_rate, (float)audio_rate, 16, rf_bw / 2.2f, 4.5f);
    h->nco_inc = sdro_nco_inc((float)nco_freq, (float)in_rate);
    h->level = (float)pow(10.0, (double)squelch_db / 10.0);
    h->volume = volume; h->mute = mute; h->bandpass = bandpass;
    bandpass_create(h, BP_TAPS, (double)audio_rate, 300.0, (double)(rf_bw / 2.0f));
    h->dl_size = audio_rate / 5;
    h->dl = (float*)calloc((size_t)(2 * h->dl_size), sizeof(float));
    h->dl_written = (unsigned char*)calloc((size_t)(2 * h->dl_size), 1);
    h->agc_size = audio_rate / 10;
    h->agc_hist = (double*)malloc(sizeof(double) * (size_t)h->agc_size);
    const float initial = 0.003f;                        /* SimpleAGC::resizeNew(newSize, Real initial) */
    for (int i = 0; i < h->agc_size; i++) h->agc_hist[i] = (double)initial;
    h->agc_sum = (double)h->agc_size * (double)initial;
    h->probe[P_FIRST_OPEN] = -1; h->last_below = -1;
    return h;
}

void amo_destroy(void* p)
{
    amo* h = (amo*)p;
    if (!h) return;
    sdro_backend_free(h->front);
    free(h->ci); free(h->dl); free(h->dl_written); free(h->agc_hist); free(h);
}

static int16_t process_one(amo* h, float ci_re, float ci_im)
{
    float re = ci_re / 32768.0f;
    float im = ci_im / 32768.0f;
    float magsq = re * re + im * im;
    if (h->ma_num < MA_N) { h->ma_samples[h->ma_num++] = magsq; h->ma_total += magsq; }
    else {
        float* oldest = &h->ma_samples[h->ma_index];
        h->ma_total += magsq - *oldest;
        *oldest = magsq;
        h->ma_index = (h->ma_index + 1) % MA_N;
    }
    h->magsq = h->ma_total / MA_N;
    h->magsq_sum += magsq;
    if (magsq > h->magsq_peak) h->magsq_peak = magsq;
    h->magsq_count++;
    /* m_squelchDelayLine.write(magsq) */
    h->dl[h->dl_write] = magsq; h->dl[h->dl_write + h->dl_size] = magsq;
    h->dl_written[h->dl_write] = 1; h->dl_written[h->dl_write + h->dl_size] = 1;
    h->dl_cur = h->dl_write;
    if (h->dl_write < h->dl_size - 1) h->dl_write++; else h->dl_write = 0;

    const int below = h->magsq < h->level;
    if (h->last_below >= 0 && below != h->last_below) h->probe[P_BELOW_CHANGES]++;
    h->last_below = below;
    if (below) { if (h->sq_count > 0) h->sq_count--; }
    else { if (h->sq_count < h->rate / 10) h->sq_count++; }
    if (h->sq_count == 0) h->probe[P_COUNT_ZERO]++;
    if (h->sq_count == h->rate / 10) h->probe[P_COUNT_CAP]++;

    int16_t sample;
    const int open = h->sq_count >= h->rate / 20;
    if (open != h->sq_open) { h->probe[P_TRANSITIONS]++; if (!open) h->closed_since_fed = 1; }
    h->sq_open = open;
    if (open && !h->mute) {
        h->probe[P_OPEN]++;
        if (h->probe[P_FIRST_OPEN] < 0) h->probe[P_FIRST_OPEN] = h->n_audio;
        int delay = (int)(h->rate / 20);
        if (delay > h->dl_size) delay = h->dl_size;
        const int at = h->dl_cur + h->dl_size - delay;
        if (!h->dl_written[at]) h->probe[P_UNWRITTEN_READS]++;
        float demod = sqrtf(h->dl[at]);
        if (demod > 0.0f) {                              /* SimpleAGC::feed, m_cutoff = 0 */
            double* oldest = &h->agc_hist[h->agc_index];
            h->agc_sum += (double)demod - *oldest;
            *oldest = (double)demod;
            if (h->agc_index < (uint32_t)h->agc_size - 1) h->agc_index++; else h->agc_index = 0;
            h->probe[P_FED]++;
            if (h->closed_since_fed && h->probe[P_FED] > h->agc_size) h->probe[P_FED_AFTER_CLOSURE]++;
        } else h->probe[P_OPEN_ROOT_ZERO]++;
        const float avg = (float)(h->agc_sum / (double)h->agc_size);
        const float g = avg > 0.0f ? avg : 0.0f;         /* SimpleAGC::getValue, m_clip = 0 */
        demod = (demod - g) / g;
        if (h->bandpass) { demod = bandpass_filter(h, demod); demod /= 301.0f; }
        float attack = ((float)h->sq_count - 0.05f * (float)h->rate) / (0.05f * (float)h->rate);
        sample = to_q16(demod * smootherstep(attack) * (float)(h->rate / 24) * h->volume);
    } else sample = 0;
    h->n_audio++;
    return sample;
}

long amo_feed(void* p, const int16_t* iq, long n, int16_t* audio, long cap)
{
    amo* h = (amo*)p;
    if (n > h->ci_cap) { free(h->ci); h->ci_cap = n + 1024; h->ci = (float*)malloc(sizeof(float) * 2 * (size_t)h->ci_cap); }
    const long k = n > 0 ? (long)sdro_backend_feed(h->front, iq, n, h->ci) : 0;
    for (long i = 0; i < k && i < cap; i++) audio[i] = process_one(h, h->ci[2 * i], h->ci[2 * i + 1]);
    return k;
}

void amo_levels(void* p, double* magsq, double* sum, double* peak, long* count)
{
    amo* h = (amo*)p;
    *magsq = h->magsq; *sum = h->magsq_sum; *peak = h->magsq_peak; *count = h->magsq_count;
}
int amo_squelch_open(void* p) { return ((amo*)p)->sq_open; }
int amo_squelch_count(void* p) { return (int)((amo*)p)->sq_count; }
void amo_probe(void* p, long* out) { memcpy(out, ((amo*)p)->probe, sizeof(long) * P_N); }

int amo_design(void* p, float* taps, float* bandpass, int* nco_inc, float* level)
{
    amo* h = (amo*)p;
    const int nt = sdro_backend_ntaps(h->front);
    memcpy(taps, sdro_backend_taps(h->front), sizeof(float) * 16 * (size_t)nt);
    memcpy(bandpass, h->bp_taps, sizeof h->bp_taps);
    *nco_inc = h->nco_inc; *level = h->level;
    return nt;
}
