/* Strict-IEEE C restatement of UDPSrc::feed (plugins/channelrx/udpsrc/udpsrc.cpp:136-321) for the formats IQ16, IQ24, NFM,
 * NFMMono, AMMono, AMNoDCMono and AMBPFMono, m_agc included, and of the derivations of the constructor, applySettings(settings,
 * true), applyChannelSettings(.., true) and start() (:44-113, 323-327, 463-621), streaming, one channel per object, in the
 * reference's statement order with its containers as they are: MovingAverage<double> with its history and index
 * (movingaverage.h), calculateSquelch with its flag and two counters (udpsrc.h:238-278), PhaseDiscriminators::
 * phaseDiscriminator (phasediscri.h:50-55), the Bandpass<double> ring walk (bandpass.h:77-122), the udpWrite* conversions
 * (udpsrc.h:296-340), MagAGC::feedAndGetValue with its history, four counters and smootherstep (agc.cpp:98-182,
 * stepfunctions.h:23-36) set up as UDPSrc does (udpsrc.cpp:60, 101-102, 531-534, 579).  The checker of sdrx_udpsrc_*: tests build it with `cc -O2 -ffp-contract=off -shared` and call it
 * through ctypes; the product never links it.
 *
 * The front (NCO, Interpolator::create / decimate) is the oracle's, oracle/sdro_float.c, whose sdro_backend_new starts the
 * distance at 0 as the demodulators do.  UDPSrc starts it at one step (m_sampleDistanceRemain = inputSampleRate /
 * outputSampleRate), so this file compiles that source in and sets the field after the constructor; it links no libsdro.
 *
 *   udpo_create(in_rate, nco_freq, output_sample_rate, sample_format, rf_bw, fm_deviation, gain, squelch_db, squelch_gate, squelch_enabled, agc)
 *   udpo_feed(h, iq, n, payload, spectrum, cap)   feed(); payload samples (element size by format) and spectrum Samples; returns their count
 *   udpo_state(h, &in_magsq, st[4])       m_inMagsq; m_squelchOpen, m_squelchOpenCount, m_squelchCloseCount, samples so far
 *   udpo_last_open(h, flags, cap)         m_squelchOpen after calculateSquelch for every sample of the last feed
 *   udpo_probe(h, out[8])                 test probes, see the enum below
 *   udpo_design(h, taps[16 * ntaps], bandpass[151], &nco_inc, windows[3], &gate, &release, &level, &fm_scaling, &step, agc_ints[4], &agc_threshold)   returns taps per phase
 */
#include "../oracle/sdro_float.c"
#include <stdint.h>

#define BP_TAPS 301

enum { P_TRANSITIONS, P_OPEN, P_ABOVE_CHANGES, P_CONV_WRAPS, P_ZERO_CI, P_RELEASE_HITS, P_GATE_HITS, P_CLOSED_ABOVE, P_AGC_UP_RAMP, P_AGC_DOWN_RAMP,
       P_AGC_MODE_CHANGES, P_AGC_CUT, P_N };

typedef struct { double* hist; int size; unsigned index; double sum; } mavg;

static void mavg_resize(mavg* m, int n, double initial)
{
    free(m->hist);
    m->hist = (double*)malloc(sizeof(double) * (size_t)n);
    for (int i = 0; i < n; i++) m->hist[i] = initial;
    m->size = n;
    m->sum = (double)n * initial;
    m->index = 0;
}
static void mavg_feed(mavg* m, double v)
{
    double* oldest = &m->hist[m->index];
    m->sum += v - *oldest;
    *oldest = v;
    if (m->index < (unsigned)m->size - 1) m->index++; else m->index = 0;
}
static double mavg_average(const mavg* m) { return m->sum / (double)m->size; }

/* MagAGC (m_squared false) */
typedef struct {
    mavg avg; double u0, R, magsq, threshold, step_delta, clamp_max;
    int count, gate, step_length, step_up, step_down, gate_counter, step_down_delay, clamping, last_up;
    long* probe;
} magagc;

static float smootherstep(float x)
{
    if (x == 1.0f) return 1.0f; else if (x == 0.0f) return 0.0f;
    const double x3 = x * x * x, x4 = x * x3, x5 = x * x4;
    return (float)(6.0 * x5 - 15.0 * x4 + 10.0 * x3);
}

static double magagc_feed(magagc* a, float re, float im)
{
    a->magsq = (double)(re * re + im * im);
    mavg_feed(&a->avg, a->magsq);
    if (a->clamping && sqrt(a->magsq) > a->clamp_max) a->u0 = a->clamp_max / sqrt(a->magsq);
    else a->u0 = a->R / sqrt(mavg_average(&a->avg));
    if (a->magsq > a->threshold) {
        if (a->gate_counter < a->gate) a->gate_counter++; else a->count = 0;
    } else {
        if (a->count < a->step_down_delay) a->count++;
        a->gate_counter = 0;
    }
    const int up = a->count < a->step_down_delay;
    if (a->last_up >= 0 && up != a->last_up) a->probe[10]++;
    a->last_up = up;
    if (up) {
        a->step_down = a->step_up;
        if (a->step_up < a->step_length) { a->step_up++; a->probe[8]++; return a->u0 * smootherstep((float)(a->step_up * a->step_delta)); }
        return a->u0;
    }
    a->step_up = a->step_down;
    if (a->step_down > 0) { a->step_down--; a->probe[9]++; return a->u0 * smootherstep((float)(a->step_down * a->step_delta)); }
    a->probe[11]++;
    return 0.0;
}

typedef struct {
    sdro_backend* front;
    float* ci; long ci_cap;
    int fmt, in_rate;
    float rate, gain, fm_scaling, m1r, m1i;
    int sq_enabled, sq_open, sq_open_count, sq_close_count, sq_gate, sq_release;
    double squelch, in_magsq;
    mavg in_avg, am_avg;
    int agc_on; magagc agc;
    float bp_taps[BP_TAPS / 2 + 1]; double bp_samples[BP_TAPS]; int bp_ptr;
    long total, probe[P_N]; int last_above;
    unsigned char* open_flags; long n_flags;     /* m_squelchOpen per sample of the last feed */
    int32_t nco_inc;
} udpo;

static void bandpass_create(udpo* h, int nTaps, double sampleRate, double lowCutoff, double highCutoff)
{
    const double PI_D = 3.14159265358979323846;
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

static double bandpass_filter(udpo* h, double sample)      /* Bandpass<double>: Real taps, double ring and accumulator */
{
    double acc = 0;
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

/* implicit float -> qint16 on x86-64: cvttss2si, low 16 bits */
static int16_t f_to_q16(float v)
{
    const int32_t i = (v >= -2147483648.0f && v < 2147483648.0f) ? (int32_t)v : (int32_t)0x80000000u;
    return (int16_t)(uint16_t)(uint32_t)i;
}
/* implicit double -> int16_t on x86-64: cvttsd2si, low 16 bits */
static int16_t d_to_q16(double v)
{
    const int32_t i = (v > -2147483649.0 && v < 2147483648.0) ? (int32_t)v : (int32_t)0x80000000u;
    return (int16_t)(uint16_t)(uint32_t)i;
}

static int elem_size(int fmt) { return fmt == 1 ? 8 : (fmt == 0 || fmt == 2 ? 4 : 2); }

void* udpo_create(int in_rate, int nco_freq, float rate, int fmt, float rf_bw, int fm_deviation, float gain, int squelch_db, int squelch_gate,
                  int squelch_enabled, int agc)
{
    udpo* h = (udpo*)calloc(1, sizeof(udpo));
    h->fmt = fmt; h->in_rate = in_rate; h->rate = rate; h->gain = gain; h->sq_enabled = squelch_enabled;
    h->front = sdro_backend_new((float)nco_freq, (float)in_rate, rate, 16, rf_bw / 2.0f, 4.5f);
    h->front->distance = h->front->step;                   /* m_sampleDistanceRemain = inputSampleRate / m_outputSampleRate */
    h->nco_inc = sdro_nco_inc((float)nco_freq, (float)in_rate);
    h->sq_gate = (int)((rate * (float)squelch_gate) / 100);
    h->sq_release = (int)((rate * (float)squelch_gate) / 100);
    bandpass_create(h, BP_TAPS, (double)rate, 300.0, (double)(rf_bw / 2.0f));
    mavg_resize(&h->in_avg, (int)(rate * 0.01), 1e-10);
    mavg_resize(&h->am_avg, (int)(rate * 0.005), 1e-10);
    h->squelch = pow(10.0, (double)squelch_db / 10.0);
    h->fm_scaling = rate / (2.0f * (float)fm_deviation);
    h->last_above = -1;
    /* m_agc(9600, m_agcTarget, 1e-6), setClampMax(2^30), setClamping(true); then resize(rate / 5, rate / 20, m_agcTarget) with fill(0),
     * setStepDownDelay, setGate, setThreshold(m_squelch * (1 << 23)) */
    h->agc_on = agc && fmt >= 8;
    h->agc.R = (double)16384.0f; h->agc.clamp_max = 32768.0 * 32768.0; h->agc.clamping = 1;
    mavg_resize(&h->agc.avg, (int)(rate / 5), 0.0);
    h->agc.step_length = (int)(rate / 20); h->agc.step_delta = 1.0 / h->agc.step_length;
    h->agc.step_up = 0; h->agc.step_down = h->agc.step_length; h->agc.count = 0; h->agc.gate_counter = 0;
    h->agc.step_down_delay = (int)((rate * (float)(squelch_gate == 0 ? 1 : squelch_gate)) / 100);
    h->agc.gate = (int)(rate * 0.05);
    h->agc.threshold = h->squelch * (1 << 23);
    h->agc.u0 = 1.0; h->agc.last_up = -1; h->agc.probe = h->probe;
    return h;
}

void udpo_destroy(void* p)
{
    udpo* h = (udpo*)p;
    if (!h) return;
    sdro_backend_free(h->front);
    free(h->ci); free(h->open_flags); free(h->in_avg.hist); free(h->am_avg.hist); free(h->agc.avg.hist); free(h);
}

static void calculate_squelch(udpo* h, double value)
{
    const int above = !h->sq_enabled || value > h->squelch;
    if (h->last_above >= 0 && above != h->last_above) h->probe[P_ABOVE_CHANGES]++;
    h->last_above = above;
    const int was = h->sq_open;
    if (above) {
        if (h->sq_gate == 0) h->sq_open = 1;
        else if (h->sq_open_count < h->sq_gate) { h->sq_open_count++; if (!h->sq_open) h->probe[P_CLOSED_ABOVE]++; }
        else { h->sq_close_count = h->sq_release; h->sq_open = 1; h->probe[P_GATE_HITS]++; }
    } else {
        if (h->sq_gate == 0) h->sq_open = 0;
        else if (h->sq_close_count > 0) h->sq_close_count--;
        else { h->sq_open_count = 0; h->sq_open = 0; if (was) h->probe[P_RELEASE_HITS]++; }
    }
    if (was != h->sq_open) h->probe[P_TRANSITIONS]++;
}

static void note_wrap(udpo* h, double wanted, int16_t got) { if (wanted != (double)got && !(wanted > -1.0 && wanted < 1.0 && got == 0)) h->probe[P_CONV_WRAPS]++; }

static void process_one(udpo* h, float re, float im, char* payload, int16_t* spectrum)
{
    double agcFactor = 1.0, inMagSq;
    if (h->agc_on) { agcFactor = magagc_feed(&h->agc, re, im); inMagSq = h->agc.magsq; }
    else inMagSq = (double)(re * re + im * im);
    if (re == 0.0f && im == 0.0f) h->probe[P_ZERO_CI]++;
    mavg_feed(&h->in_avg, inMagSq / (32768.0 * 32768.0));
    h->in_magsq = mavg_average(&h->in_avg);
    spectrum[0] = f_to_q16(re); spectrum[1] = f_to_q16(im);
    calculate_squelch(h, h->in_magsq);
    const int open = h->sq_open;
    if (open) h->probe[P_OPEN]++;
    if (h->fmt == 2 || h->fmt == 3) {
        float discri = 0;
        if (open) {
            const float dr = h->m1r * re - (-h->m1i) * im, di = h->m1r * im + (-h->m1i) * re;     /* std::conj(m_m1Sample) * sample */
            h->m1r = re; h->m1i = im;
            discri = (float)(((double)atan2f(di, dr) / 3.14159265358979323846) * (double)h->fm_scaling) * h->gain;
        }
        const int16_t q = d_to_q16((double)discri * 32768.0);
        note_wrap(h, trunc((double)discri * 32768.0), q);
        if (h->fmt == 2) { ((int16_t*)payload)[0] = q; ((int16_t*)payload)[1] = q; } else ((int16_t*)payload)[0] = q;
    } else if (h->fmt == 8) {
        const float amplitude = open ? (float)(sqrt(inMagSq) * agcFactor * (double)h->gain) : 0;
        ((int16_t*)payload)[0] = f_to_q16(amplitude);
        note_wrap(h, trunc((double)amplitude), ((int16_t*)payload)[0]);
    } else if (h->fmt == 9) {
        int16_t q = 0;
        if (open) {
            const double demodf = sqrt(inMagSq);
            mavg_feed(&h->am_avg, demodf);
            const float amplitude = (float)((demodf - mavg_average(&h->am_avg)) * agcFactor * (double)h->gain);
            q = f_to_q16(amplitude);
            note_wrap(h, trunc((double)amplitude), q);
        }
        ((int16_t*)payload)[0] = q;
    } else if (h->fmt == 10) {
        int16_t q = 0;
        if (open) {
            double demodf = sqrt(inMagSq);
            demodf = bandpass_filter(h, demodf);
            demodf /= 301.0;
            const float amplitude = (float)(demodf * agcFactor * (double)h->gain);
            q = f_to_q16(amplitude);
            note_wrap(h, trunc((double)amplitude), q);
        }
        ((int16_t*)payload)[0] = q;
    } else {                                                /* raw I/Q: udpWrite(FixReal, FixReal) */
        int16_t r = 0, i = 0;
        if (open) {
            r = f_to_q16(re * h->gain); i = f_to_q16(im * h->gain);
            note_wrap(h, trunc((double)(re * h->gain)), r);
        }
        if (h->fmt == 0) { ((int16_t*)payload)[0] = r; ((int16_t*)payload)[1] = i; }
        else { ((int32_t*)payload)[0] = (int32_t)r * 256; ((int32_t*)payload)[1] = (int32_t)i * 256; }     /* Sample24(real << 8, imag << 8) */
    }
    h->total++;
}

long udpo_feed(void* p, const int16_t* iq, long n, void* payload, int16_t* spectrum, long cap)
{
    udpo* h = (udpo*)p;
    if (n > h->ci_cap) {
        free(h->ci); free(h->open_flags); h->ci_cap = n + 1024;
        h->ci = (float*)malloc(sizeof(float) * 2 * (size_t)h->ci_cap); h->open_flags = (unsigned char*)malloc((size_t)h->ci_cap);
    }
    const long k = n > 0 ? (long)sdro_backend_feed(h->front, iq, n, h->ci) : 0;
    const int es = elem_size(h->fmt);
    h->n_flags = 0;
    for (long i = 0; i < k && i < cap; i++) {
        process_one(h, h->ci[2 * i], h->ci[2 * i + 1], (char*)payload + i * es, spectrum + 2 * i);
        h->open_flags[h->n_flags++] = (unsigned char)h->sq_open;
    }
    return k;
}

void udpo_state(void* p, double* in_magsq, long* st)
{
    udpo* h = (udpo*)p;
    *in_magsq = h->in_magsq;
    st[0] = h->sq_open; st[1] = h->sq_open_count; st[2] = h->sq_close_count; st[3] = h->total;
}
long udpo_last_open(void* p, unsigned char* flags, long cap)
{
    udpo* h = (udpo*)p;
    const long n = h->n_flags < cap ? h->n_flags : cap;
    if (n > 0) memcpy(flags, h->open_flags, (size_t)n);
    return n;
}
void udpo_probe(void* p, long* out) { memcpy(out, ((udpo*)p)->probe, sizeof(long) * P_N); }

int udpo_design(void* p, float* taps, float* bandpass, int* nco_inc, int* windows, int* gate, int* release, double* level, float* fm_scaling, float* step,
                int* agc_ints, double* agc_threshold)
{
    udpo* h = (udpo*)p;
    const int nt = sdro_backend_ntaps(h->front);
    memcpy(taps, sdro_backend_taps(h->front), sizeof(float) * 16 * (size_t)nt);
    memcpy(bandpass, h->bp_taps, sizeof h->bp_taps);
    *nco_inc = h->nco_inc; windows[0] = h->in_avg.size; windows[1] = h->am_avg.size; windows[2] = (int)(h->rate * 0.01);
    *gate = h->sq_gate; *release = h->sq_release; *level = h->squelch; *fm_scaling = h->fm_scaling; *step = h->front->step;
    agc_ints[0] = h->agc.avg.size; agc_ints[1] = h->agc.step_length; agc_ints[2] = h->agc.step_down_delay; agc_ints[3] = h->agc.gate;
    *agc_threshold = h->agc.threshold;
    return nt;
}
