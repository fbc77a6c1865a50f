/* Strict-IEEE C restatement of AMDemod::feed / AMDemod::processOneSample, in envelope mode (m_pll = false) and in synchronous
 * mode (m_pll = true, the three operations), with the derivations of the constructor and of
 * applyChannelSettings / applyAudioSampleRate / applySettings (plugins/channelrx/demodam/amdemod.cpp:47-88, 101-276, 360-475),
 * streaming, one demodulator per object, in the reference's statement order with its containers as they are: the
 * MovingAverageUtil<Real, double, 16> fill-up and roll branches, the DoubleBufferFIFO with its doubled array, the
 * MovingAverage<double> ring of SimpleAGC, the Bandpass ring walk (bandpass.h:77-122), StepFunctions::smootherstep.
 * The front (NCO, Interpolator::create / decimate) is oracle/libsdro.so's sdro_backend_*.  The checker of sdrx_am_*: tests
 * build it with `cc -O2 -ffp-contract=off -shared` and call it through ctypes; the product never links it.
 * The delay line starts zeroed (DoubleBufferFIFO leaves it uninitialised; include/sdrx.h states the ruling).
 *
 * The synchronous branch (amdemod.cpp:191-238) is stated one open sample at a time, as the reference runs it: the ring of m_pllFilt
 * (Lowpass<std::complex<float>>, 101 taps, lowpass.h's walk), one step of m_pll (tests/pll_oracle.h), the turn of the unfiltered
 * sample, fftfilt's runDSB / runSSB with getDC false (oracle/libsdro.so's sdro_fftfilt_run, one sample per call), MagAGC with the
 * threshold off over its MovingAverage<double> ring, m_syncAMBuff and m_syncAMBuffIndex.  m_syncAMBuff starts at 0.0f (the
 * reference never initialises it; include/sdrx.h states the ruling).  SSBFilter is designed once from ssb_design_rate and
 * ssb_design_bw; DSBFilter, m_pllFilt, the AGC lengths and the loop's lock time follow rf_bw and audio_rate.  Nothing here comes
 * from sdrangel_amd/csrc: no compaction, no block arithmetic, no prefix sum.
 *
 *   amo_create(in_rate, nco_freq, audio_rate, rf_bw, volume, squelch_db, mute, bandpass)       amo_create_ex with pll = 0
 *   amo_create_ex(the same eight, pll, sync_op, ssb_design_rate, ssb_design_bw)   sync_op 0 DSB, 1 USB, 2 LSB; 0 = 48000 and 5000
 *   amo_feed(h, iq, n, audio, cap)        feed(); audio samples (the value written to .l and .r) go to audio, returns their count
 *   amo_levels(h, &magsq, &sum, &peak, &count)    m_magsq, m_magsqSum, m_magsqPeak, m_magsqCount
 *   amo_squelch_open(h), amo_squelch_count(h)
 *   amo_probe(h, out[10])                 test probes, see the enum below
 *   amo_design(h, taps[16 * ntaps], bandpass[151], &nco_inc, &squelch_level)   returns taps per phase
 *   amo_pll(h, &locked, &freq)            getPllLocked(), getPllFrequency() (an envelope demodulator: 0 and 0.0f)
 *   amo_sync_design(h, taps[51], filter[2 * 2048], &flen, coef[5])      m_pllFilt's folded taps, the filter bins in use, a1 a2 b0 b1 b2
 *   amo_sync_probe(h, out[13])            see the second enum below
 *   amo_trace(h, path, path_sb)           from now on, per open sample re, im, the filtered pair, m_yRe, m_yIm and demod before the
 *                                         Bandpass go to path (7 floats), per filter output the sideband pair to path_sb
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../oracle/sdro.h"
#include "pll_oracle.h"

#define MA_N 16
#define BP_TAPS 301
static const double PI_D = 3.14159265358979323846;

enum { P_TRANSITIONS, P_BELOW_CHANGES, P_COUNT_ZERO, P_COUNT_CAP, P_FED, P_OPEN_ROOT_ZERO, P_FIRST_OPEN, P_UNWRITTEN_READS, P_OPEN,
       P_FED_AFTER_CLOSURE, P_N };
/* the sync probe: open samples; blocks completed; reopenings of the squelch; closures inside a block (the open-sample count k at the
 * closure has k % B outside {0, 1, B - 1}); the loop's saturations above and below and its lock counter's ups and downs; feeds that
 * gave audio, completed no block and left samples pending; feeds that brought open samples and ended on a block boundary; filter
 * outputs beyond the AGC history's length; samples non-finite or not strictly inside the int16 range before the conversion, and the
 * non-finite ones among them */
enum { S_OPEN, S_BLOCKS, S_REOPEN, S_CLOSE_INSIDE, S_SAT_HI, S_SAT_LO, S_LOCK_UP, S_LOCK_DOWN, S_FEED_NO_BLOCK, S_FEED_ON_EDGE, S_WRAPPED,
       S_BAD, S_NONFINITE, S_N };
#define PF_TAPS 101
#define SYNC_BUFF (2 * 1024)

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
    /* synchronous AM */
    int pll, sync_op, block;
    float pf_taps[PF_TAPS / 2 + 1], pf_samples[PF_TAPS][2]; int pf_ptr;
    loops loop;
    sdro_fftfilt* filt; int filt_mode, flen; float* sideband;
    double* sagc_hist; int sagc_size; uint32_t sagc_index; double sagc_sum, sagc_r;
    float sync_buff[SYNC_BUFF]; uint32_t sync_index;
    long sprobe[S_N]; long outputs; int ever_open, was_open, gate_was_open;
    FILE* trace; FILE* trace_sb;
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

/* Lowpass<>::create(nTaps, sampleRate, cutoff), nTaps odd: the folded taps */
static void lowpass_create(float* taps, int nTaps, double sampleRate, double cutoff)
{
    const double Wc = (2.0 * PI_D * cutoff) / sampleRate;
    const double mid = ((double)nTaps - 1.0) / 2.0;
    const int nt = nTaps / 2 + 1;
    int i;
    for (i = 0; i < nt; i++) {
        if (i == (nTaps - 1) / 2) taps[i] = (float)(Wc / PI_D);
        else taps[i] = (float)(sin(((double)i - mid) * Wc) / (((double)i - mid) * PI_D));
    }
    for (i = 0; i < nt; i++) taps[i] = (float)(taps[i] * (0.54 + 0.46 * cos((2.0 * PI_D * ((double)i - mid)) / (double)nTaps)));
    float sum = 0;
    for (i = 0; i < nt - 1; i++) sum += taps[i] * 2;
    sum += taps[i];
    for (i = 0; i < nt; i++) taps[i] /= sum;
}

/* the m_pll branch of processOneSample for one open sample: demod before the Bandpass */
static float sync_one(amo* h, float re, float im)
{
    /* s = m_pllFilt.filter(s): complex<float> sums and products by a real tap, component by component */
    float acc_re = 0, acc_im = 0;
    int a = h->pf_ptr, b = a - 1, i;
    h->pf_samples[h->pf_ptr][0] = re; h->pf_samples[h->pf_ptr][1] = im;
    while (b < 0) b += PF_TAPS;
    for (i = 0; i < PF_TAPS / 2; i++) {
        acc_re += (h->pf_samples[a][0] + h->pf_samples[b][0]) * h->pf_taps[i];
        acc_im += (h->pf_samples[a][1] + h->pf_samples[b][1]) * h->pf_taps[i];
        a++; while (a >= PF_TAPS) a -= PF_TAPS;
        b--; while (b < 0) b += PF_TAPS;
    }
    acc_re += h->pf_samples[a][0] * h->pf_taps[i];
    acc_im += h->pf_samples[a][1] * h->pf_taps[i];
    h->pf_ptr++; while (h->pf_ptr >= PF_TAPS) h->pf_ptr -= PF_TAPS;

    pll_feed(&h->loop, acc_re, acc_im);
    float cs[2];
    cs[0] = re * h->loop.y_im - im * h->loop.y_re;
    cs[1] = re * h->loop.y_re + im * h->loop.y_im;
    const int n_out = (int)sdro_fftfilt_run(h->filt, h->filt_mode, cs, 1, h->sideband);
    for (i = 0; i < n_out; i++) {
        const float sb_re = h->sideband[2 * i], sb_im = h->sideband[2 * i + 1];
        /* m_syncAMAGC.feedAndGetValue: the threshold off, neither squared nor clamping */
        const double magsq = sb_re * sb_re + sb_im * sb_im;
        double* oldest = &h->sagc_hist[h->sagc_index];
        h->sagc_sum += magsq - *oldest;
        *oldest = magsq;
        if (h->sagc_index < (uint32_t)h->sagc_size - 1) h->sagc_index++; else h->sagc_index = 0;
        const double u0 = h->sagc_r / sqrt(h->sagc_sum / (double)h->sagc_size);
        const float agc = (float)u0;
        const float z_re = sb_re * agc, z_im = sb_im * agc;
        h->sync_buff[i] = z_re + z_im;
        h->sync_index = 0;
        h->outputs++;
        if (h->trace_sb) { const float t[2] = { sb_re, sb_im }; fwrite(t, 4, 2, h->trace_sb); }
    }
    if (n_out) h->sprobe[S_BLOCKS]++;
    h->sync_index = h->sync_index < SYNC_BUFF ? h->sync_index : 0;
    const float demod = h->sync_buff[h->sync_index++] * 4.0f;
    if (h->trace) { const float t[7] = { re, im, acc_re, acc_im, h->loop.y_re, h->loop.y_im, demod }; fwrite(t, 4, 7, h->trace); }
    return demod;
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

void* amo_create_ex(int in_rate, int nco_freq, int audio_rate, float rf_bw, float volume, float squelch_db, int mute, int bandpass,
                    int pll, int sync_op, int ssb_design_rate, float ssb_design_bw)
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
    /* the loop as PhaseLockComplex() leaves it, then computeCoefficients(0.05, 0.707, 1000) and setSampleRate(audio_rate); an envelope
     * demodulator never steps it */
    h->pll = pll != 0; h->sync_op = sync_op;
    h->loop.order = 1; h->loop.y_re = 1.0f;
    pll_compute_coefficients(&h->loop, 0.05f, 0.707f, 1000.0f);
    set_sample_rate(&h->loop, (unsigned)audio_rate);
    if (h->pll) {
        const uint32_t ctor_rate = (uint32_t)(ssb_design_rate ? ssb_design_rate : 48000);
        const float ctor_bw = ssb_design_bw != 0.0f ? ssb_design_bw : 5000.0f;
        lowpass_create(h->pf_taps, PF_TAPS, (double)audio_rate, 200.0);
        if (sync_op == 0) { h->flen = 2 * 1024; h->filt_mode = 8; h->filt = sdro_fftfilt_new(-1.0f, (2.0f * rf_bw) / (float)audio_rate, h->flen); }
        else { h->flen = 1024; h->filt_mode = sync_op == 1 ? 6 : 7; h->filt = sdro_fftfilt_new(0.0f, ctor_bw / ctor_rate, h->flen); }
        h->block = h->flen / 2;
        h->sideband = (float*)calloc((size_t)h->flen, sizeof(float));
        /* m_syncAMAGC.resize(rate / 4, rate / 8, 0.1): Real R, history filled with 0 */
        h->sagc_size = audio_rate / 4;
        h->sagc_hist = (double*)calloc((size_t)h->sagc_size, sizeof(double));
        h->sagc_r = (double)0.1f;
    }
    return h;
}

void* amo_create(int in_rate, int nco_freq, int audio_rate, float rf_bw, float volume, float squelch_db, int mute, int bandpass)
{
    return amo_create_ex(in_rate, nco_freq, audio_rate, rf_bw, volume, squelch_db, mute, bandpass, 0, 0, 0, 0.0f);
}

void amo_destroy(void* p)
{
    amo* h = (amo*)p;
    if (!h) return;
    sdro_backend_free(h->front);
    if (h->filt) sdro_fftfilt_free(h->filt);
    if (h->trace) fclose(h->trace);
    if (h->trace_sb) fclose(h->trace_sb);
    free(h->sideband); free(h->sagc_hist);
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
    if (open && !h->was_open) { if (h->ever_open) h->sprobe[S_REOPEN]++; h->ever_open = 1; }
    h->was_open = open;
    const int gate = open && !h->mute;
    if (h->pll && h->gate_was_open && !gate) {
        const long k = h->sprobe[S_OPEN] % h->block;
        if (k != 0 && k != 1 && k != h->block - 1) h->sprobe[S_CLOSE_INSIDE]++;
    }
    h->gate_was_open = gate;
    if (gate && h->pll) {
        float demod = sync_one(h, re, im);
        h->sprobe[S_OPEN]++;
        if (h->bandpass) { demod = bandpass_filter(h, demod); demod /= 301.0f; }
        float attack = ((float)h->sq_count - 0.05f * (float)h->rate) / (0.05f * (float)h->rate);
        const float v = demod * smootherstep(attack) * (float)(h->rate / 24) * h->volume;
        if (!(fabsf(v) < 32767.0f)) { h->sprobe[S_BAD]++; if (!isfinite(v)) h->sprobe[S_NONFINITE]++; }
        sample = to_q16(v);
    } else if (gate) {
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
    const long open_before = h->sprobe[S_OPEN], blocks_before = h->sprobe[S_BLOCKS];
    for (long i = 0; i < k && i < cap; i++) audio[i] = process_one(h, h->ci[2 * i], h->ci[2 * i + 1]);
    if (h->pll) {
        const long left = h->sprobe[S_OPEN] % h->block;
        if (k > 0 && h->sprobe[S_BLOCKS] == blocks_before && left > 0) h->sprobe[S_FEED_NO_BLOCK]++;
        if (h->sprobe[S_OPEN] > open_before && left == 0) h->sprobe[S_FEED_ON_EDGE]++;
    }
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

void amo_pll(void* p, int* locked, float* freq)
{
    const amo* h = (const amo*)p;
    *locked = h->pll && h->loop.lock_count > h->loop.lock_time - 2;         /* locked(), order 1 */
    *freq = h->loop.freq;
}

int amo_sync_design(void* p, float* taps, float* filter, int* flen, float* coef)
{
    const amo* h = (const amo*)p;
    if (!h->pll) return -1;
    memcpy(taps, h->pf_taps, sizeof h->pf_taps);
    memcpy(filter, sdro_fftfilt_filter(h->filt), sizeof(float) * 2 * (size_t)h->flen);
    *flen = h->flen;
    coef[0] = h->loop.a1; coef[1] = h->loop.a2; coef[2] = h->loop.b0; coef[3] = h->loop.b1; coef[4] = h->loop.b2;
    return 0;
}

void amo_sync_probe(void* p, long* out)
{
    amo* h = (amo*)p;
    h->sprobe[S_SAT_HI] = h->loop.probe[0]; h->sprobe[S_SAT_LO] = h->loop.probe[1];
    h->sprobe[S_LOCK_UP] = h->loop.probe[3]; h->sprobe[S_LOCK_DOWN] = h->loop.probe[4];
    h->sprobe[S_WRAPPED] = h->outputs > h->sagc_size ? h->outputs - h->sagc_size : 0;
    memcpy(out, h->sprobe, sizeof(long) * S_N);
}

int amo_trace(void* p, const char* path, const char* path_sb)
{
    amo* h = (amo*)p;
    h->trace = fopen(path, "wb"); h->trace_sb = fopen(path_sb, "wb");
    return h->trace && h->trace_sb ? 0 : -1;
}
