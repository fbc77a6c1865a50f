/* Strict-IEEE C restatement of SSBDemod::feed (plugins/channelrx/demodssb/ssbdemod.cpp:147-285) and of the derivations of the
 * constructor, applyAudioSampleRate, applySettings(settings, true) and start() (:46-101, 401-422, 457-533), streaming, one
 * demodulator per object, in the reference's statement order with its containers as they are: MovingAverage<double> with its
 * ring and index (movingaverage.h:24-35), MagAGC::feedAndGetValue with its four counters (agc.cpp:98-182), getStepValue
 * (:196-206), StepFunctions::smootherstep, the DoubleBufferFIFO(96000) with its doubled array and its clamped readBack.  The
 * front (NCO, Interpolator::create / decimate, fftfilt runSSB / runDSB) is oracle/libsdro.so's sdro_backend_* and
 * sdro_fftfilt_*.  The checker of sdrx_ssb_*: tests build it with `cc -O2 -ffp-contract=off -shared` and call it through
 * ctypes; the product never links it.
 * The delay line starts zeroed (the reference leaves it uninitialised; include/sdrx.h states the ruling).
 *
 *   ssbo_create(in_rate, nco_freq, audio_rate, rf_bw, low_cutoff, volume, span_log2, binaural, flip, dsb, mute, agc, clamping,
 *               agc_time_log2, agc_power_threshold, agc_threshold_gate)
 *   ssbo_feed(h, iq, n, audio_lr, cap, spec_iq, spec_cap, &n_spec)   feed(); returns the number of AudioSamples
 *   ssbo_levels(h, &magsq, &sum, &peak, &count)
 *   ssbo_audio_active(h)
 *   ssbo_state(h, out[10])                g, count, U, D, m_undersampleCount, delay-line write index; m_u0 and the sum as doubles;
 *                                         getStepValue(), getStepDownValue()
 *   ssbo_probe(h, out[P_N])               test probes, see the enum below
 *   ssbo_design(h, taps, filter, &nco_inc, &hn, &gate, &threshold, &volume)   returns taps per phase
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../oracle/sdro.h"

#define DL_SIZE (2 * 48000)

enum { P_RESETS, P_GATE_FULL, P_COUNT_FULL, P_UP_TO_DOWN, P_DOWN_TO_UP, P_DOWN_TO_UP_EARLY, P_CLAMPED, P_DL_WRAPS, P_NAN_WRITES, P_GROUPS,
       P_STEP_UP_FULL, P_STEP_DOWN_ZERO, P_N };

typedef struct {
    sdro_backend* front; sdro_fftfilt* filt;
    int filt_mode, flen;
    float* ci; float* sb; long ci_cap;
    int rate, usb, dsb, mute, binaural, flip, agc_active, span_log2;
    float volume;
    /* spectrum */
    float sum_re, sum_im; int undersample;
    double magsq, magsq_sum, magsq_peak; int magsq_count;
    /* MagAGC */
    double u0, R, agc_magsq, threshold, step_delta, clamp_max;
    double* hist; int hist_n; uint32_t hist_index; double ma_sum;
    int threshold_enable, gate, step_length, step_up, step_down, gate_counter, step_down_delay, clamping, count;
    /* DoubleBufferFIFO<cmplx> */
    float* dl; int dl_size, dl_write, dl_cur;
    int audio_active;
    long probe[P_N]; int last_mode;
    int32_t nco_inc;
} ssbo;

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

static double agc_feed_and_get_value(ssbo* h, float re, float im)
{
    h->agc_magsq = re * re + im * im;
    {   /* m_moving_average.feed(m_magsq) */
        double* oldest = &h->hist[h->hist_index];
        h->ma_sum += h->agc_magsq - *oldest;
        *oldest = h->agc_magsq;
        if (h->hist_index < (uint32_t)h->hist_n - 1) h->hist_index++; else h->hist_index = 0;
    }
    const double average = h->ma_sum / (double)h->hist_n;
    if (h->clamping) {
        if (sqrt(h->agc_magsq) > h->clamp_max) { h->u0 = h->clamp_max / sqrt(h->agc_magsq); h->probe[P_CLAMPED]++; }
        else h->u0 = h->R / sqrt(average);
    } else h->u0 = h->R / sqrt(average);

    if (!h->threshold_enable) return h->u0;
    if (h->agc_magsq > h->threshold) {
        if (h->gate_counter < h->gate) { h->gate_counter++; if (h->gate_counter == h->gate) h->probe[P_GATE_FULL]++; }
        else { h->count = 0; h->probe[P_RESETS]++; }
    } else {
        if (h->count < h->step_down_delay) { h->count++; if (h->count == h->step_down_delay) h->probe[P_COUNT_FULL]++; }
        h->gate_counter = 0;
    }
    if (h->count < h->step_down_delay) {
        if (h->last_mode == 0) { h->probe[P_DOWN_TO_UP]++; if (h->step_down > 0) h->probe[P_DOWN_TO_UP_EARLY]++; }
        h->last_mode = 1;
        h->step_down = h->step_up;
        if (h->step_up < h->step_length) {
            h->step_up++;
            if (h->step_up == h->step_length) h->probe[P_STEP_UP_FULL]++;
            return h->u0 * smootherstep(h->step_up * h->step_delta);
        }
        return h->u0;
    } else {
        if (h->last_mode == 1) h->probe[P_UP_TO_DOWN]++;
        h->last_mode = 0;
        h->step_up = h->step_down;
        if (h->step_down > 0) {
            h->step_down--;
            if (h->step_down == 0) h->probe[P_STEP_DOWN_ZERO]++;
            return h->u0 * smootherstep(h->step_down * h->step_delta);
        }
        return 0.0;
    }
}

static float agc_step_value(const ssbo* h)
{
    if (h->count < h->step_down_delay) return smootherstep(h->step_up * h->step_delta);
    return smootherstep(h->step_down * h->step_delta);
}

void* ssbo_create(int in_rate, int nco_freq, int audio_rate, float rf_bw, float low_cutoff, float volume, int span_log2, int binaural, int flip,
                  int dsb, int mute, int agc, int clamping, int agc_time_log2, int agc_power_threshold, int agc_threshold_gate)
{
    ssbo* h = (ssbo*)calloc(1, sizeof(ssbo));
    float band = rf_bw, low = low_cutoff;
    h->usb = 1;
    if (band < 0) { band = -band; low = -low; h->usb = 0; }
    if (band < 100.0f) { band = 100.0f; low = 0; }
    h->rate = audio_rate; h->dsb = dsb; h->mute = mute; h->binaural = binaural; h->flip = flip; h->agc_active = agc; h->span_log2 = span_log2;
    h->front = sdro_backend_new((float)nco_freq, (float)in_rate, (float)audio_rate, 16, band * 1.5f, 2.0f);
    h->nco_inc = sdro_nco_inc((float)nco_freq, (float)in_rate);
    if (dsb) { h->flen = 2048; h->filt = sdro_fftfilt_new(-1.0f, (2.0f * band) / (float)(uint32_t)audio_rate, 2048); h->filt_mode = 3; }
    else { h->flen = 1024; h->filt = sdro_fftfilt_new(low / (float)(uint32_t)audio_rate, band / (float)(uint32_t)audio_rate, 1024); h->filt_mode = h->usb ? 1 : 2; }
    h->volume = volume; h->volume /= 4.0;
    /* MagAGC(12000, agcTarget, 1e-2), then resize(n, n / 2, agcTarget) + fill(0), setStepDownDelay(n), setClampMax */
    const int n = (audio_rate / 1000) * (1 << agc_time_log2);
    const float Rf = (float)3276.8;
    h->R = Rf; h->u0 = 1.0;
    h->hist_n = n; h->hist = (double*)calloc((size_t)n, sizeof(double)); h->hist_index = 0; h->ma_sum = 0.0;
    h->step_length = n / 2; h->step_delta = 1.0 / h->step_length; h->step_up = 0; h->step_down = h->step_length;
    h->step_down_delay = n; h->count = 0; h->gate_counter = 0;
    h->clamp_max = 32768.0 / 100.0; h->clamping = clamping;
    h->threshold_enable = agc_power_threshold != 100;     /* != -m_minPowerThresholdDB (-100 in the 16-bit build) */
    h->threshold = pow(10.0, agc_power_threshold / 10.0) * (32768.0 * 32768.0);
    h->gate = (audio_rate / 1000) * agc_threshold_gate;
    h->dl_size = DL_SIZE;
    h->dl = (float*)calloc((size_t)(4 * h->dl_size), sizeof(float));
    h->last_mode = -1;
    return h;
}

void ssbo_destroy(void* p)
{
    ssbo* h = (ssbo*)p;
    if (!h) return;
    sdro_backend_free(h->front); sdro_fftfilt_free(h->filt);
    free(h->ci); free(h->sb); free(h->hist); free(h->dl); free(h);
}

long ssbo_feed(void* p, const int16_t* iq, long n, int16_t* audio, long cap, int16_t* spec, long spec_cap, long* n_spec_out)
{
    ssbo* h = (ssbo*)p;
    if (n > h->ci_cap) {
        free(h->ci); free(h->sb); h->ci_cap = n + 1024;
        h->ci = (float*)malloc(sizeof(float) * 2 * (size_t)h->ci_cap); h->sb = (float*)malloc(sizeof(float) * 2 * (size_t)(h->ci_cap + 2048));
    }
    const long k = n > 0 ? (long)sdro_backend_feed(h->front, iq, n, h->ci) : 0;
    const long n_out = k > 0 ? (long)sdro_fftfilt_run(h->filt, h->filt_mode, h->ci, k, h->sb) : 0;
    const int decim = 1 << (h->span_log2 - 1);
    const unsigned char decim_mask = (unsigned char)(decim - 1);
    long n_spec = 0, fill = 0;
    for (long i = 0; i < n_out; i++) {
        const float sre = h->sb[2 * i], sim = h->sb[2 * i + 1];
        h->sum_re += sre; h->sum_im += sim;
        if (!(h->undersample++ & decim_mask)) {
            float avgr = h->sum_re / decim;
            float avgi = h->sum_im / decim;
            h->magsq = (avgr * avgr + avgi * avgi) / (32768.0 * 32768.0);
            h->magsq_sum += h->magsq;
            if (h->magsq > h->magsq_peak) h->magsq_peak = h->magsq;
            h->magsq_count++;
            h->probe[P_GROUPS]++;
            if (n_spec < spec_cap) {
                if (!h->dsb & !h->usb) { spec[2 * n_spec] = to_q16(avgi); spec[2 * n_spec + 1] = to_q16(avgr); }
                else { spec[2 * n_spec] = to_q16(avgr); spec[2 * n_spec + 1] = to_q16(avgi); }
            }
            n_spec++;
            h->sum_re = 0.0f; h->sum_im = 0.0f;
        }
        float agcVal = h->agc_active ? agc_feed_and_get_value(h, sre, sim) : 10.0;
        /* readBack(m_agc.getStepDownDelay()) */
        int delay = h->step_down_delay;
        if (delay > h->dl_size) delay = h->dl_size;
        const float* delayed = &h->dl[2 * (h->dl_cur + h->dl_size - delay)];
        const float dre = delayed[0], dim = delayed[1];
        h->audio_active = dre != 0.0;
        {   /* write(sideband[i] * agcVal) */
            const float wre = sre * agcVal, wim = sim * agcVal;
            if (wre != wre || wim != wim) h->probe[P_NAN_WRITES]++;
            h->dl[2 * h->dl_write] = wre; h->dl[2 * h->dl_write + 1] = wim;
            h->dl[2 * (h->dl_write + h->dl_size)] = wre; h->dl[2 * (h->dl_write + h->dl_size) + 1] = wim;
            h->dl_cur = h->dl_write;
            if (h->dl_write < h->dl_size - 1) h->dl_write++; else { h->dl_write = 0; h->probe[P_DL_WRAPS]++; }
        }
        int16_t l, r;
        if (h->mute) { r = 0; l = 0; }
        else {
            const float sv = agc_step_value(h);
            const float zre = dre * sv, zim = dim * sv;
            if (h->binaural) {
                if (h->flip) { r = to_q16(zim * h->volume); l = to_q16(zre * h->volume); }
                else { r = to_q16(zre * h->volume); l = to_q16(zim * h->volume); }
            } else {
                float demod = (zre + zim) * 0.7;
                int16_t sample = to_q16(demod * h->volume);
                l = sample; r = sample;
            }
        }
        if (fill < cap) { audio[2 * fill] = l; audio[2 * fill + 1] = r; }
        fill++;
    }
    *n_spec_out = n_spec;
    return fill;
}

void ssbo_levels(void* p, double* magsq, double* sum, double* peak, long* count)
{
    ssbo* h = (ssbo*)p;
    *magsq = h->magsq; *sum = h->magsq_sum; *peak = h->magsq_peak; *count = h->magsq_count;
}
int ssbo_audio_active(void* p) { return ((ssbo*)p)->audio_active; }
void ssbo_state(void* p, double* out)
{
    ssbo* h = (ssbo*)p;
    out[0] = h->gate_counter; out[1] = h->count; out[2] = h->step_up; out[3] = h->step_down; out[4] = h->undersample; out[5] = h->dl_write;
    out[6] = h->u0; out[7] = h->ma_sum;
    out[8] = agc_step_value(h);
    out[9] = h->count < h->step_down_delay ? 1.0f : smootherstep(h->step_down * h->step_delta);
}
void ssbo_probe(void* p, long* out) { memcpy(out, ((ssbo*)p)->probe, sizeof(long) * P_N); }

int ssbo_design(void* p, float* taps, float* filter, int* nco_inc, int* hn, int* gate, double* threshold, float* volume)
{
    ssbo* h = (ssbo*)p;
    const int nt = sdro_backend_ntaps(h->front);
    memcpy(taps, sdro_backend_taps(h->front), sizeof(float) * 16 * (size_t)nt);
    memcpy(filter, sdro_fftfilt_filter(h->filt), sizeof(float) * 2 * (size_t)h->flen);
    *nco_inc = h->nco_inc; *hn = h->hist_n; *gate = h->gate; *threshold = h->threshold; *volume = h->volume;
    return nt;
}
