/* Strict-IEEE C restatement of BFMDemod::feed with m_rdsActive clear, and of what the constructor, applyChannelSettings(force) and
 * applySettings(force) leave behind (plugins/channelrx/demodbfm/bfmdemod.cpp:50-103, 116-281, 396-515), streaming, one demodulator
 * per object: NCO on scaled samples, fftfilt::create_filter and runFilt (sdrbase/dsp/fftfilt.cpp:108-146, 261-282), the squelch
 * counter, the gated phaseDiscriminator (phasediscri.h:50-55), PhaseLock::configure and process with RDSPhaseLock::processPhase
 * (phaselock.cpp:86-143, 253-367, phaselock.h:171-180), the two Interpolators (interpolator.cpp:21-129, interpolator.h:23-36,
 * 182-195), the two LowPassFilterRC (filterrc.cpp:31-56) and the qint16 conversion.  The checker of sdrx_bfm_*: tests build it
 * with `cc -O2 -ffp-contract=off -shared` against oracle/libsdro.so (NCO table, NCO increment, g_fft) and call it through ctypes;
 * the product never links it.  m_m1Sample starts at 0 (value-initialised; the reference leaves it to the allocator).
 *
 * The pilot loop feeds back, so no tolerance means anything and nothing in it may come from whatever libm the machine has: sinf,
 * cosf (glibc 2.28+, the build a CPU with FMA is given: every a + b * c one fma()) and atan2f (fdlibm's float routines, glibc up
 * to 2.40) are written out below.  fma() itself is correctly rounded wherever it runs.  exp() is only called at creation.
 *
 *   bfo_create(in_rate, nco_freq, audio_rate, rf_bw, af_bw, volume, squelch_db, stereo, lsb, show_pilot)
 *   bfo_feed(h, iq, n, audio_lr, cap_pairs, sink, cap_sink, &n_sink)   feed(); returns the number of l, r pairs; sink takes the
 *                                                                       real parts of m_sampleBuffer (the imaginary ones are 0)
 *   bfo_state(h, &sum, &peak, &count, ints[3], bits[5])    m_magsqSum, m_magsqPeak, m_magsqCount; m_squelchState, locked(),
 *                                                           m_lock_cnt; bits of m_pilot_level, m_freq, m_phase, X.m_y1, Y.m_y1
 *   bfo_probe(h, out[10])    steps through: the ratio, +1, -1, clamp low, clamp high, phase wrap, lock counter up, lock counter
 *                            reset; emissions on which the two resamplers disagreed; samples at or above the squelch level
 *   bfo_design(h, taps[16 * ntaps], filter[2048], &nco_inc, &squelch_level, pll7, &lock_delay, rc2)   returns taps per phase
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
    int stereo, lsb, show_pilot;
    /* NCO */
    float nco[NCO_N];
    int nco_inc, nco_phase;
    /* fftfilt */
    cf filter[FLEN], data[FLEN], ovl[FLEN2], out[FLEN2];
    int inptr;
    /* squelch, discriminator, levels */
    int sq_state;
    cf m1;
    double magsq_sum, magsq_peak;
    int magsq_count;
    /* PhaseLock */
    float minfreq, maxfreq, ph_b0, ph_a1, ph_a2, lf_b0, lf_b1, minsignal;
    float phase, freq, i1, i2, q1, q2, x1, pilot_level, psin, pcos;
    int lock_delay, lock_cnt, pilot_periods;
    float p[4];                       /* m_pilotPLLSamples */
    /* both Interpolators: one set of taps (the same create), two rings */
    int ntaps, ptr, ptr_s;
    float* taps;                      /* [phase][ntaps] */
    cf* ring; cf* ring_s;
    float distance, step, distance_s, step_s;
    /* LowPassFilterRC X, Y */
    float rc_b0, rc_a1, y1x, y1y;
    long probe[10];
} bfo;

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
static void create_filter(bfo* h, float f1, float f2)
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
static void interp_create(bfo* h, double sample_rate, double cutoff)
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

/* (qint16) of a float on x86-64: cvttss2si (0x80000000 when out of range or NaN), then the low 16 bits */
static int16_t to_q16(float v)
{
    const int32_t i = (v >= -2147483648.0f && v < 2147483648.0f) ? (int32_t)v : (int32_t)0x80000000u;
    return (int16_t)(uint16_t)((uint32_t)i & 0xffffu);
}

/* ---------------------------------------------------------------- libm, restated */
static uint32_t f_bits(float v) { uint32_t i; memcpy(&i, &v, 4); return i; }
static uint32_t top12(float v) { return (f_bits(v) >> 20) & 0x7ff; }

static float sincos_poly(double x, double x2, double cs, int n)
{
    const double c0 = 0x1p0, c1 = -0x1.ffffffd0c621cp-2, c2 = 0x1.55553e1068f19p-5, c3 = -0x1.6c087e89a359dp-10, c4 = 0x1.99343027bf8c3p-16;
    const double s1 = -0x1.555545995a603p-3, s2 = 0x1.1107605230bc4p-7, s3 = -0x1.994eb3774cf24p-13;
    if ((n & 1) == 0) {
        const double x3 = x * x2;
        const double t1 = fma(x2, s3, s2);
        const double x7 = x3 * x2;
        const double s = fma(x3, s1, x);
        return (float)fma(x7, t1, s);
    }
    const double x4 = x2 * x2;
    const double t2 = fma(x2, cs * c4, cs * c3);
    const double t1 = fma(x2, cs * c1, cs * c0);
    const double x6 = x4 * x2;
    const double c = fma(x4, cs * c2, t1);
    return (float)fma(x6, t2, c);
}

static const uint32_t g_inv_pio4[24] = { 0xa2, 0xa2f9, 0xa2f983, 0xa2f9836e, 0xf9836e4e, 0x836e4e44, 0x6e4e4415, 0x4e441529,
                                         0x441529fc, 0x1529fc27, 0x29fc2757, 0xfc2757d1, 0x2757d1f5, 0x57d1f534, 0xd1f534dd, 0xf534ddc0,
                                         0x34ddc0db, 0xddc0db62, 0xc0db6295, 0xdb629599, 0x6295993c, 0x95993c43, 0x993c4390, 0x3c439041 };

static float o_sincosf(float y, int shift)
{
    const double hpi_inv = 0x1.45F306DC9C883p+23, hpi = 0x1.921FB54442D18p0;
    double x = (double)y;
    int n, q;
    if (top12(y) < top12(0x1.921FB6p-1f)) {
        if (top12(y) < top12(0x1p-12f)) return shift ? 1.0f : y;
        return sincos_poly(x, x * x, 1.0, shift);
    }
    if (top12(y) < top12(120.0f)) {
        const double r = x * hpi_inv;
        n = ((int32_t)r + 0x800000) >> 24;
        x = fma(-(double)n, hpi, x);
        q = n;
    } else if (top12(y) < top12(INFINITY)) {
        const uint32_t xi = f_bits(y);
        const uint32_t* arr = &g_inv_pio4[(xi >> 26) & 15];
        const int sh = (int)((xi >> 23) & 7);
        const uint32_t m = ((xi & 0xffffff) | 0x800000) << sh;
        uint64_t r0 = (uint32_t)(m * arr[0]);
        const uint64_t r1 = (uint64_t)m * arr[4], r2 = (uint64_t)m * arr[8];
        r0 = (r2 >> 32) | (r0 << 32);
        r0 += r1;
        const uint64_t k = (r0 + (1ULL << 61)) >> 62;
        r0 -= k << 62;
        x = (double)(int64_t)r0 * 0x1.921FB54442D18p-62;
        n = (int)k;
        q = n + (int)(xi >> 31);
    } else return y - y;
    const double s = ((q ^ (q >> 1)) & 1) ? -1.0 : 1.0;
    return sincos_poly(x * s, x * x, (q & 2) ? -1.0 : 1.0, n ^ shift);
}

static int f2i(float v) { int i; memcpy(&i, &v, 4); return i; }
static float o_atanf(float x)
{
    static const float hi[4] = { 4.6364760399e-01f, 7.8539812565e-01f, 9.8279368877e-01f, 1.5707962513e+00f };
    static const float lo[4] = { 5.0121582440e-09f, 3.7748947079e-08f, 3.4473217170e-08f, 7.5497894159e-08f };
    const float t0 = 3.3333334327e-01f, t1 = -2.0000000298e-01f, t2 = 1.4285714924e-01f, t3 = -1.1111110449e-01f, t4 = 9.0908870101e-02f,
                t5 = -7.6918758452e-02f, t6 = 6.6610731184e-02f, t7 = -5.8335702866e-02f, t8 = 4.9768779427e-02f, t9 = -3.6531571299e-02f,
                t10 = 1.6285819933e-02f;
    const int hx = f2i(x), ix = hx & 0x7fffffff;
    int id = -1;
    if (ix >= 0x4c000000) {
        if (ix > 0x7f800000) return x + x;
        return hx > 0 ? hi[3] + lo[3] : -hi[3] - lo[3];
    }
    if (ix < 0x3ee00000) {
        if (ix < 0x31000000) return x;
    } else {
        x = fabsf(x);
        if (ix < 0x3f980000) {
            if (ix < 0x3f300000) { id = 0; x = (2.0f * x - 1.0f) / (2.0f + x); }
            else { id = 1; x = (x - 1.0f) / (x + 1.0f); }
        } else {
            if (ix < 0x401c0000) { id = 2; x = (x - 1.5f) / (1.0f + 1.5f * x); }
            else { id = 3; x = -1.0f / x; }
        }
    }
    const float z = x * x, w = z * z;
    const float s1 = z * (t0 + w * (t2 + w * (t4 + w * (t6 + w * (t8 + w * t10)))));
    const float s2 = w * (t1 + w * (t3 + w * (t5 + w * (t7 + w * t9))));
    if (id < 0) return x - x * (s1 + s2);
    const float r = hi[id] - ((x * (s1 + s2) - lo[id]) - x);
    return hx < 0 ? -r : r;
}
static float o_atan2f(float y, float x)
{
    const float tiny = 1.0e-30f, pi_o_4 = 7.8539818525e-01f, pi_o_2 = 1.5707963705e+00f, pi = 3.1415927410e+00f, pi_lo = -8.7422776573e-08f;
    const int hx = f2i(x), ix = hx & 0x7fffffff, hy = f2i(y), iy = hy & 0x7fffffff;
    if (ix > 0x7f800000 || iy > 0x7f800000) return x + y;
    if (hx == 0x3f800000) return o_atanf(y);
    const int m = ((hy >> 31) & 1) | ((hx >> 30) & 2);
    if (iy == 0) return m < 2 ? y : (m == 2 ? pi + tiny : -pi - tiny);
    if (ix == 0) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
    if (ix == 0x7f800000) {
        if (iy == 0x7f800000) return m == 0 ? pi_o_4 + tiny : (m == 1 ? -pi_o_4 - tiny : (m == 2 ? 3.0f * pi_o_4 + tiny : -3.0f * pi_o_4 - tiny));
        return m == 0 ? 0.0f : (m == 1 ? -0.0f : (m == 2 ? pi + tiny : -pi - tiny));
    }
    if (iy == 0x7f800000) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
    const int k = (iy - ix) >> 23;
    float z;
    if (k > 60) z = pi_o_2 + 0.5f * pi_lo;
    else if (hx < 0 && k < -60) z = 0.0f;
    else z = o_atanf(fabsf(y / x));
    return m == 0 ? z : (m == 1 ? -z : (m == 2 ? pi - (z - pi_lo) : (z - pi_lo) - pi));
}

#define O_PI 3.14159265358979323846

/* PhaseLock::configure(Real freq, Real bandwidth, Real minsignal) */
static void pll_configure(bfo* h, float freq, float bandwidth, float minsignal)
{
    h->minfreq = (freq - bandwidth) * 2.0 * O_PI;
    h->maxfreq = (freq + bandwidth) * 2.0 * O_PI;
    h->minsignal = minsignal;
    h->lock_delay = (int)(20.0 / bandwidth);
    h->lock_cnt = 0;
    h->pilot_level = 0;
    double p1 = exp(-1.146 * bandwidth * 2.0 * O_PI);
    double p2 = exp(-5.331 * bandwidth * 2.0 * O_PI);
    h->ph_a1 = -p1 - p2;
    h->ph_a2 = p1 * p2;
    h->ph_b0 = 1 + h->ph_a1 + h->ph_a2;
    double q1 = exp(-0.1153 * bandwidth * 2.0 * O_PI);
    h->lf_b0 = 0.62 * bandwidth * 2.0 * O_PI;
    h->lf_b1 = -h->lf_b0 * q1;
    h->freq = freq * 2.0 * O_PI;
    h->phase = 0;
    h->i1 = h->i2 = h->q1 = h->q2 = 0;
    h->x1 = 0;
    h->pilot_periods = 0;
}

/* PhaseLock::process(const Real& sample_in, Real* samples_out), processPhase of RDSPhaseLock, process_phasor */
static void pll_process(bfo* h, float sample_in, float* out)
{
    h->psin = o_sincosf(h->phase, 0);
    h->pcos = o_sincosf(h->phase, 1);
    out[0] = h->psin;
    out[1] = 2.0 * h->psin * h->pcos;
    out[2] = (2.0 * h->pcos * h->pcos) - 1.0;
    out[3] = h->phase;
    float phasor_i = h->psin * sample_in;
    float phasor_q = h->pcos * sample_in;
    phasor_i = h->ph_b0 * phasor_i - h->ph_a1 * h->i1 - h->ph_a2 * h->i2;
    phasor_q = h->ph_b0 * phasor_q - h->ph_a1 * h->q1 - h->ph_a2 * h->q2;
    h->i2 = h->i1; h->i1 = phasor_i;
    h->q2 = h->q1; h->q1 = phasor_q;
    float phase_err;
    if (phasor_i > fabsf(phasor_q)) { phase_err = phasor_q / phasor_i; h->probe[0]++; }
    else if (phasor_q > 0) { phase_err = 1; h->probe[1]++; }
    else { phase_err = -1; h->probe[2]++; }
    h->pilot_level = phasor_i;
    h->freq += h->lf_b0 * phase_err + h->lf_b1 * h->x1;
    h->x1 = phase_err;
    if (h->freq < h->minfreq) h->probe[3]++;
    if (h->maxfreq < h->freq) h->probe[4]++;
    {   /* std::max(m_minfreq, std::min(m_maxfreq, m_freq)) */
        const float mn = h->freq < h->maxfreq ? h->freq : h->maxfreq;
        h->freq = h->minfreq < mn ? mn : h->minfreq;
    }
    h->phase += h->freq;
    if (h->phase > 2.0 * O_PI) {
        h->phase -= 2.0 * O_PI;
        h->pilot_periods++;
        if (h->pilot_periods == 19000) h->pilot_periods = 0;
        h->probe[5]++;
    }
    if (2 * h->pilot_level > h->minsignal) {
        if (h->lock_cnt < h->lock_delay) { h->lock_cnt += 1; h->probe[6]++; }
    } else {
        if (h->lock_cnt > 0) h->probe[7]++;
        h->lock_cnt = 0;
    }
    if (h->lock_cnt < h->lock_delay) h->pilot_periods = 0;
}

/* LowPassFilterRC::configure */
static void rc_configure(bfo* h, float timeconst)
{
    h->rc_a1 = -exp(-1 / timeconst);
    h->rc_b0 = 1 + h->rc_a1;
    h->y1x = h->y1y = 0;
}

/* Interpolator::decimate(&distance, next, &result) on one of the two rings */
static int decimate(const bfo* h, cf* ring, int* ptr, float* distance, cf next, cf* result)
{
    (*ptr)--; if (*ptr < 0) *ptr = h->ntaps - 1;
    ring[*ptr] = next;
    *distance = (float)((double)*distance - 1.0);
    if (*distance >= 1.0) return 0;
    int phase = (int)floor(*distance * (float)PHASES);
    if (phase < 0) phase = 0;
    const float* c = h->taps + phase * h->ntaps;
    float ra = 0, ia = 0;
    int sp = *ptr;
    for (int t = 0; t < h->ntaps; t++) {
        ra += c[t] * ring[sp].r;
        ia += c[t] * ring[sp].i;
        sp = (sp + 1) % h->ntaps;
    }
    result->r = ra; result->i = ia;
    return 1;
}

bfo* bfo_create(int in_rate, int nco_freq, int audio_rate, float rf_bw, float af_bw, float volume, float squelch_db, int stereo, int lsb,
                int show_pilot)
{
    bfo* h = (bfo*)calloc(1, sizeof *h);
    const float fm_excursion = 750000;                                     /* m_fmExcursion(default_excursion) */
    const float default_deemphasis = 50.0;
    h->rf_bw = rf_bw; h->volume = volume; h->stereo = stereo; h->lsb = lsb; h->show_pilot = show_pilot;
    h->pcos = 1.0;
    sdro_nco_table(h->nco);
    h->nco_inc = sdro_nco_inc((float)nco_freq, (float)in_rate);           /* m_nco.setFreq(-inputFrequencyOffset, inputSampleRate) */
    pll_configure(h, 19000.0 / in_rate, 50.0 / in_rate, 0.01);
    interp_create(h, in_rate, af_bw);                                      /* both create(16, inputSampleRate, afBandwidth) */
    h->ring_s = (cf*)calloc((size_t)h->ntaps + 2, sizeof(cf));
    h->distance = (float)in_rate / (unsigned)audio_rate;                   /* m_interpolatorDistanceRemain = (Real) rate / m_audioSampleRate */
    h->step = (float)in_rate / (float)(unsigned)audio_rate;
    h->distance_s = (float)in_rate / (unsigned)audio_rate;
    h->step_s = (float)in_rate / (float)(unsigned)audio_rate;
    const float low = -(rf_bw / 2.0) / in_rate, hi = (rf_bw / 2.0) / in_rate;
    create_filter(h, low, hi);
    h->fm_scaling = in_rate / fm_excursion;
    rc_configure(h, default_deemphasis * (unsigned)audio_rate * 1.0e-6);
    h->squelch_level = pow(10.0, squelch_db / 10.0);
    return h;
}

void bfo_destroy(bfo* h) { if (h) { free(h->taps); free(h->ring); free(h->ring_s); free(h); } }

long bfo_feed(bfo* h, const int16_t* iq, long n, int16_t* audio_lr, long cap_pairs, int16_t* sink, long cap_sink, long* n_sink_out)
{
    long n_out = 0, n_sink = 0;
    for (long k = 0; k < n; k++) {
        /* NCO::nextIQ: phase += inc, wrapped into [0, 4096) */
        h->nco_phase += h->nco_inc;
        while (h->nco_phase >= NCO_N) h->nco_phase -= NCO_N;
        while (h->nco_phase < 0) h->nco_phase += NCO_N;
        const cf osc = { h->nco[h->nco_phase], -h->nco[(h->nco_phase + NCO_N / 4) % NCO_N] };
        const cf s = { iq[2 * k] / 32768.0f, iq[2 * k + 1] / 32768.0f };  /* it->real() / SDR_RX_SCALEF */
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
            h->magsq_sum += msq;
            if (msq > h->magsq_peak) h->magsq_peak = msq;
            h->magsq_count++;
            if (msq >= h->squelch_level) {
                h->probe[9]++;
                if (h->sq_state < h->rf_bw / 10) h->sq_state++;          /* int against float */
            } else {
                if (h->sq_state > 0) h->sq_state--;
            }
            float demod;
            if (h->sq_state > h->rf_bw / 20) {
                /* Complex d(std::conj(m_m1Sample) * sample) */
                const cf cj = { h->m1.r, -h->m1.i };
                const cf d = c_mul(cj, rf);
                h->m1 = rf;
                demod = (o_atan2f(d.i, d.r) / O_PI) * h->fm_scaling;
            } else {
                demod = 0;
            }
            if (!h->show_pilot) {
                if (n_sink < cap_sink) sink[n_sink] = to_q16(demod * 32768.0f);
                n_sink++;
            }
            float sample_stereo = 0.0f;
            int fired_s = -1;
            if (h->stereo) {
                pll_process(h, demod, h->p);
                if (h->show_pilot) {
                    if (n_sink < cap_sink) sink[n_sink] = to_q16(h->p[1] * 32768.0f);
                    n_sink++;
                }
                cf sd, cs;
                if (h->lsb) { sd.r = demod * h->p[1]; sd.i = demod * h->p[2]; }
                else { sd.r = demod * 1.17 * h->p[1]; sd.i = 0; }
                fired_s = decimate(h, h->ring_s, &h->ptr_s, &h->distance_s, sd, &cs);
                if (fired_s) {
                    sample_stereo = h->lsb ? cs.r + cs.i : cs.r;
                    h->distance_s += h->step_s;
                }
            }
            const cf e = { demod, 0 };
            cf ci;
            const int fired = decimate(h, h->ring, &h->ptr, &h->distance, e, &ci);
            if (fired_s >= 0 && fired_s != fired) h->probe[8]++;
            if (!fired) continue;
            int16_t l, r;
            if (h->stereo) {
                h->y1x = ((ci.r + sample_stereo) * h->rc_b0) - (h->y1x * h->rc_a1);
                h->y1y = ((ci.r - sample_stereo) * h->rc_b0) - (h->y1y * h->rc_a1);
                l = to_q16(h->y1x * (1 << 12) * h->volume);
                r = to_q16(h->y1y * (1 << 12) * h->volume);
            } else {
                h->y1x = (ci.r * h->rc_b0) - (h->y1x * h->rc_a1);
                l = r = to_q16(h->y1x * (1 << 12) * h->volume);
            }
            if (n_out < cap_pairs) { audio_lr[2 * n_out] = l; audio_lr[2 * n_out + 1] = r; }
            n_out++;
            h->distance += h->step;
        }
    }
    *n_sink_out = n_sink;
    return n_out;
}

void bfo_state(const bfo* h, double* sum, double* peak, long* count, int* ints, uint32_t* bits)
{
    *sum = h->magsq_sum; *peak = h->magsq_peak; *count = h->magsq_count;
    ints[0] = h->sq_state; ints[1] = h->lock_cnt >= h->lock_delay; ints[2] = h->lock_cnt;
    bits[0] = f_bits(h->pilot_level); bits[1] = f_bits(h->freq); bits[2] = f_bits(h->phase); bits[3] = f_bits(h->y1x); bits[4] = f_bits(h->y1y);
}

void bfo_probe(const bfo* h, long* out) { memcpy(out, h->probe, sizeof h->probe); }

int bfo_design(const bfo* h, float* taps, float* filter, int* nco_inc, float* squelch_level, float* pll7, int* lock_delay, float* rc2)
{
    if (taps) memcpy(taps, h->taps, sizeof(float) * (size_t)(PHASES * h->ntaps));
    if (filter) memcpy(filter, h->filter, sizeof h->filter);
    if (nco_inc) *nco_inc = h->nco_inc;
    if (squelch_level) *squelch_level = h->squelch_level;
    if (pll7) { pll7[0] = h->minfreq; pll7[1] = h->maxfreq; pll7[2] = h->ph_b0; pll7[3] = h->ph_a1; pll7[4] = h->ph_a2; pll7[5] = h->lf_b0; pll7[6] = h->lf_b1; }
    if (lock_delay) *lock_delay = h->lock_delay;
    if (rc2) { rc2[0] = h->rc_b0; rc2[1] = h->rc_a1; }
    return h->ntaps;
}
