/* Strict-IEEE C restatement of NFMDemod::feed (plugins/channelrx/demodnfm/nfmdemod.cpp:140-332) with m_deltaSquelch and
 * m_ctcssOn off, and of the derivations of the constructor, applySettings(settings, true) and start() (:50-97, 334-342,
 * 478-559), streaming, one demodulator per object, in the reference's statement order with its containers as they are:
 * PhaseDiscriminators::phaseDiscriminatorDelta with atan2_approximation2 (phasediscri.h:61-78, 172-197), the
 * MovingAverageUtil<Real, double, 32> fill-up and roll branches, the DoubleBufferFIFO(24000) with its doubled array and its
 * clamped readBack, the Bandpass ring walk (bandpass.h:77-122).  The front (NCO, Interpolator::create / decimate) is
 * oracle/libsdro.so's sdro_backend_*.  The checker of sdrx_nfm_*: tests build it with `cc -O2 -ffp-contract=off -shared` and
 * call it through ctypes; the product never links it.
 * m_prevArg starts at 0 and the delay line starts zeroed (the reference leaves both uninitialised; include/sdrx.h states
 * the rulings).
 *
 *   nfmo_create(in_rate, nco_freq, audio_rate, rf_bw, af_bw, fm_deviation, volume, squelch, squelch_gate, mute)
 *   nfmo_feed(h, iq, n, audio, cap)       feed(); audio samples (the value written to .l and .r) go to audio, returns their count
 *   nfmo_levels(h, &magsq, &sum, &peak, &count)   m_movingAverage.asDouble(), m_magsqSum, m_magsqPeak, m_magsqCount
 *   nfmo_squelch_open(h), nfmo_squelch_count(h)
 *   nfmo_probe(h, out[8])                 test probes, see the enum below
 *   nfmo_design(h, taps[16 * ntaps], bandpass[151], &nco_inc, &squelch_level, &gate)   returns taps per phase
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../oracle/sdro.h"

#define MA_N 32
#define BP_TAPS 301
#define DL_SIZE 24000
static const double PI_D = 3.14159265358979323846;

enum { P_TRANSITIONS, P_BELOW_CHANGES, P_COUNT_ZERO, P_COUNT_CAP, P_OPEN, P_CLAMPED_READS, P_WRAPS, P_ZERO_CI, P_N };

typedef struct {
    sdro_backend* front;
    float* ci; long ci_cap;
    int rate;
    float fm_scaling, prev_arg, comp, level, volume;
    int mute, gate;
    /* MovingAverageUtil */
    float ma_samples[MA_N]; int ma_num; unsigned ma_index; double ma_total;
    double magsq_sum, magsq_peak; long magsq_count;
    /* DoubleBufferFIFO */
    float* dl; int dl_size, dl_write, dl_cur;
    int sq_count, sq_open;
    /* Bandpass */
    float bp_taps[BP_TAPS / 2 + 1], bp_samples[BP_TAPS]; int bp_ptr;
    /* probes */
    long probe[P_N]; int last_below; int16_t last_sample; int have_last;
    int32_t nco_inc;
} nfmo;

static void bandpass_create(nfmo* h, int nTaps, double sampleRate, double lowCutoff, double highCutoff)
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

static float bandpass_filter(nfmo* h, float sample)
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

static float atan2_approximation2(float y, float x)          /* phasediscri.h:172-197 */
{
    const float PI_F = 3.14159265f, PIBY2_F = 1.5707963f;
    if (x == 0.0f) {
        if (y > 0.0f) return PIBY2_F;
        if (y == 0.0f) return 0.0f;
        return -PIBY2_F;
    }
    float atan;
    float z = y / x;
    if (fabsf(z) < 1.0f) {
        atan = z / (1.0f + 0.28f * z * z);
        if (x < 0.0f) {
            if (y < 0.0f) return atan - PI_F;
            return atan + PI_F;
        }
    } else {
        atan = PIBY2_F - z / (z * z + 0.28f);
        if (y < 0.0f) return atan - PI_F;
    }
    return atan;
}

/* (qint16) of a float on x86-64: cvttss2si, low 16 bits */
static int16_t to_q16(float v)
{
    const int32_t i = (v >= -2147483648.0f && v < 2147483648.0f) ? (int32_t)v : (int32_t)0x80000000u;
    return (int16_t)(uint16_t)(uint32_t)i;
}

void* nfmo_create(int in_rate, int nco_freq, int audio_rate, float rf_bw, float af_bw, int fm_deviation, float volume, float squelch,
                  int squelch_gate, int mute)
{
    nfmo* h = (nfmo*)calloc(1, sizeof(nfmo));
    h->rate = audio_rate;
    h->front = sdro_backend_new((float)nco_freq, (float)in_rate, (float)audio_rate, 16, rf_bw / 2.2f, 4.5f);
    h->nco_inc = sdro_nco_inc((float)nco_freq, (float)in_rate);
    h->comp = (float)(uint32_t)audio_rate / 48000.0f;     /* nfmdemod.cpp:82-83 */
    h->comp *= sqrtf(h->comp);
    h->fm_scaling = (8.0f * (float)(uint32_t)audio_rate) / (float)fm_deviation;
    bandpass_create(h, BP_TAPS, (double)audio_rate, 300.0, (double)af_bw);
    h->gate = (audio_rate / 100) * squelch_gate;
    h->level = (float)pow(10.0, (double)squelch / 100.0);
    h->volume = volume; h->mute = mute;
    h->dl_size = DL_SIZE;
    h->dl = (float*)calloc((size_t)(2 * h->dl_size), sizeof(float));
    h->last_below = -1;
    return h;
}

void nfmo_destroy(void* p)
{
    nfmo* h = (nfmo*)p;
    if (!h) return;
    sdro_backend_free(h->front);
    free(h->ci); free(h->dl); free(h);
}

static int16_t process_one(nfmo* h, float ci_re, float ci_im)
{
    /* phaseDiscriminatorDelta */
    const float fltI = ci_re, fltQ = ci_im;
    const double magsqRaw = (double)(fltI * fltI + fltQ * fltQ);
    const float curArg = atan2_approximation2(fltQ, fltI);
    if (fltI == 0.0f && fltQ == 0.0f) h->probe[P_ZERO_CI]++;
    float fmDev = (float)((double)(curArg - h->prev_arg) / PI_D);
    h->prev_arg = curArg;
    if (fmDev < -1.0f) fmDev += 2.0f; else if (fmDev > 1.0f) fmDev -= 2.0f;
    const float demod = fmDev * h->fm_scaling;

    const float magsq = (float)(magsqRaw / (32768.0 * 32768.0));
    if (h->ma_num < MA_N) { h->ma_samples[h->ma_num++] = magsq; h->ma_total += magsq; }
    else {
        float* oldest = &h->ma_samples[h->ma_index];
        h->ma_total += magsq - *oldest;
        *oldest = magsq;
        h->ma_index = (h->ma_index + 1) % MA_N;
    }
    h->magsq_sum += magsq;
    if (magsq > h->magsq_peak) h->magsq_peak = magsq;
    h->magsq_count++;

    const int below = (float)(h->ma_total / MA_N) < h->level;
    if (h->last_below >= 0 && below != h->last_below) h->probe[P_BELOW_CHANGES]++;
    h->last_below = below;
    const float w = below ? 0.0f : demod * h->comp;
    h->dl[h->dl_write] = w; h->dl[h->dl_write + h->dl_size] = w;       /* DoubleBufferFIFO::write */
    h->dl_cur = h->dl_write;
    if (h->dl_write < h->dl_size - 1) h->dl_write++; else h->dl_write = 0;
    if (below) { if (h->sq_count > 0) h->sq_count--; }
    else { if (h->sq_count < 2 * h->gate) h->sq_count++; }
    if (h->sq_count == 0) h->probe[P_COUNT_ZERO]++;
    if (h->sq_count == 2 * h->gate) h->probe[P_COUNT_CAP]++;

    const int open = h->sq_count > h->gate;
    if (open != h->sq_open) h->probe[P_TRANSITIONS]++;
    h->sq_open = open;
    int16_t sample;
    if (h->mute) sample = 0;
    else if (open) {
        h->probe[P_OPEN]++;
        int delay = h->gate;                                 /* readBack(m_squelchGate) */
        if (delay > h->dl_size) { delay = h->dl_size; h->probe[P_CLAMPED_READS]++; }
        sample = to_q16(bandpass_filter(h, h->dl[h->dl_cur + h->dl_size - delay]) * h->volume);
    } else sample = 0;
    if (h->have_last && abs((int)sample - (int)h->last_sample) > 40000) h->probe[P_WRAPS]++;
    h->last_sample = sample; h->have_last = 1;
    return sample;
}

long nfmo_feed(void* p, const int16_t* iq, long n, int16_t* audio, long cap)
{
    nfmo* h = (nfmo*)p;
    if (n > h->ci_cap) { free(h->ci); h->ci_cap = n + 1024; h->ci = (float*)malloc(sizeof(float) * 2 * (size_t)h->ci_cap); }
    const long k = n > 0 ? (long)sdro_backend_feed(h->front, iq, n, h->ci) : 0;
    for (long i = 0; i < k && i < cap; i++) audio[i] = process_one(h, h->ci[2 * i], h->ci[2 * i + 1]);
    return k;
}

void nfmo_levels(void* p, double* magsq, double* sum, double* peak, long* count)
{
    nfmo* h = (nfmo*)p;
    *magsq = h->ma_total / MA_N; *sum = h->magsq_sum; *peak = h->magsq_peak; *count = h->magsq_count;
}
int nfmo_squelch_open(void* p) { return ((nfmo*)p)->sq_open; }
int nfmo_squelch_count(void* p) { return ((nfmo*)p)->sq_count; }
void nfmo_probe(void* p, long* out) { memcpy(out, ((nfmo*)p)->probe, sizeof(long) * P_N); }

int nfmo_design(void* p, float* taps, float* bandpass, int* nco_inc, float* level, int* gate)
{
    nfmo* h = (nfmo*)p;
    const int nt = sdro_backend_ntaps(h->front);
    memcpy(taps, sdro_backend_taps(h->front), sizeof(float) * 16 * (size_t)nt);
    memcpy(bandpass, h->bp_taps, sizeof h->bp_taps);
    *nco_inc = h->nco_inc; *level = h->level; *gate = h->gate;
    return nt;
}
