/* Strict-IEEE C restatement of UDPSrc::feed (plugins/channelrx/udpsrc/udpsrc.cpp:136-321) for the formats FormatLSB, FormatUSB,
 * FormatLSBMono and FormatUSBMono (4 .. 7), streaming, one channel per object, in the reference's statement order: the AGC and
 * the input average on the unscaled ci, calculateSquelch, `ci *= agcFactor`, fftfilt::runSSB (fftfilt.cpp:285-325) on the
 * 512-point g_fft -- bitrevR2 / scbitrevR2, ONE radix-4 stage bfR4 / ibfR4 with NDiffU = 2 (gfft.h:637-841, 1683-1887), two
 * radix-8 stages with D = 8 and 64 -- and FormatLSB's unchained `if`, behind which the ladder's raw I/Q branch runs as well.
 * The checker of sdrx_udpsrc_create_ex(.., SDRX_UDPSRC_SSB_FORMATS): tests build it with `cc -O2 -ffp-contract=off -shared` and
 * call it through ctypes; the product never links it.
 *
 * Everything in front of the filter (the front, MovingAverage, MagAGC, calculateSquelch, the conversions) is
 * tests/udpsrc_oracle.c's, compiled in; a channel is one of its objects with the two settings that differ for these formats
 * put right (m_squelchGate, the AGC being fed).  oracle/sdro_float.c's g_fft has no radix-4 stage, so the 512-point network is
 * restated here in full.
 *
 *   udso_create(in_rate, nco_freq, output_sample_rate, sample_format, rf_bw, fm_deviation, gain, squelch_db, squelch_gate, squelch_enabled, agc)
 *   udso_feed(h, iq, n, payload, cap_elements, spectrum, &n_payload)   returns the resampled samples (= spectrum Samples)
 *   udso_state(h, &in_magsq, st[7])   m_squelchOpen, open count, close count, resampled samples, inptr, blocks, payload elements so far
 *   udso_filter(h, out[1024])         the design: fftfilt(0.0, (12500 / 2.0) / 48000, 512)
 *   udso_design(h, ints[2])           m_squelchGate, m_squelchRelease
 *   udso_probe(h, out[6])             see the enum
 */
#include "udpsrc_oracle.c"

#define SSB_N 512
#define SSB_H 256

enum { Q_BLOCKS, Q_BLOCKS_OPEN, Q_FLIPS_IN_BLOCK, Q_NAN_BLOCKS, Q_WRAPS, Q_PAST_INT32, Q_N };

typedef struct {
    udpo* u;
    float utbl[SSB_N / 4 + 1];
    cf filter[SSB_N], data[SSB_N], ovl[SSB_H], out[SSB_H];
    int inptr, flips_now, last_open;
    long blocks, total_pay, probe[Q_N];
} udso;

/* g_fft<float> at M = 9 */
static void fft512(const float* u, cf* x, int inverse)
{
    const int N = SSB_N, M = 9;
    cf y[SSB_N];
    const float scale = (float)(1.0 / N);
    for (int j = 0; j < N / 2; j++) {
        const unsigned r = bitrev((unsigned)(2 * j), M);
        const cf a = x[r], b = x[r + N / 2];
        cf s, d; s.r = a.r + b.r; s.i = a.i + b.i; d.r = a.r - b.r; d.i = a.i - b.i;
        if (inverse) { s.r = scale * s.r; s.i = scale * s.i; d.r = scale * d.r; d.i = scale * d.i; }
        y[2 * j] = s; y[2 * j + 1] = d;
    }
    /* bfR4 / ibfR4, NDiffU = 2: points p, p + 2, p + 4, p + 6; p even with twiddles 1 and -+i, p odd with -+i and w1 */
    const float w1r = (float)(1.0 / 1.414213562373095048801688724209698078569);
    for (int k = 0; k < N; k += 8) {
        float f0r = y[k].r, f0i = y[k].i, f1r = y[k + 2].r, f1i = y[k + 2].i, f2r = y[k + 4].r, f2i = y[k + 4].i, f3r = y[k + 6].r, f3i = y[k + 6].i;
        float f4r, f4i, f5r, f5i, f6r, f6i, f7r, f7i, t1r, t1i;
        f5r = f0r - f1r; f5i = f0i - f1i; f0r = f0r + f1r; f0i = f0i + f1i;
        f6r = f2r + f3r; f6i = f2i + f3i; f3r = f2r - f3r; f3i = f2i - f3i;
        if (!inverse) { f7r = f5r - f3i; f7i = f5i + f3r; f5r = f5r + f3i; f5i = f5i - f3r; }
        else          { f7r = f5r + f3i; f7i = f5i - f3r; f5r = f5r - f3i; f5i = f5i + f3r; }
        f4r = f0r + f6r; f4i = f0i + f6i; f6r = f0r - f6r; f6i = f0i - f6i;
        y[k].r = f4r; y[k].i = f4i; y[k + 2].r = f5r; y[k + 2].i = f5i; y[k + 4].r = f6r; y[k + 4].i = f6i; y[k + 6].r = f7r; y[k + 6].i = f7i;

        f0r = y[k + 1].r; f0i = y[k + 1].i; f1r = y[k + 3].r; f1i = y[k + 3].i; f2r = y[k + 5].r; f2i = y[k + 5].i; f3r = y[k + 7].r; f3i = y[k + 7].i;
        if (!inverse) {
            f7r = f2r - f3i; f7i = f2i + f3r; f2r = f2r + f3i; f2i = f2i - f3r;
            f4r = f0r + f1i; f4i = f0i - f1r; t1r = f0r - f1i; t1i = f0i + f1r;
            f5r = t1r - f7r * w1r + f7i * w1r; f5i = t1i - f7r * w1r - f7i * w1r;
            f7r = t1r * 2.0f - f5r; f7i = t1i * 2.0f - f5i;
            f6r = f4r - f2r * w1r - f2i * w1r; f6i = f4i + f2r * w1r - f2i * w1r;
        } else {
            f7r = f2r + f3i; f7i = f2i - f3r; f2r = f2r - f3i; f2i = f2i + f3r;
            f4r = f0r - f1i; f4i = f0i + f1r; t1r = f0r + f1i; t1i = f0i - f1r;
            f5r = t1r - f7r * w1r - f7i * w1r; f5i = t1i + f7r * w1r - f7i * w1r;
            f7r = t1r * 2.0f - f5r; f7i = t1i * 2.0f - f5i;
            f6r = f4r - f2r * w1r + f2i * w1r; f6i = f4i - f2r * w1r - f2i * w1r;
        }
        f4r = f4r * 2.0f - f6r; f4i = f4i * 2.0f - f6i;
        y[k + 1].r = f4r; y[k + 1].i = f4i; y[k + 3].r = f5r; y[k + 3].i = f5i; y[k + 5].r = f6r; y[k + 5].i = f6i; y[k + 7].r = f7r; y[k + 7].i = f7i;
    }
    /* bfstages / ibfstages: the radix-8 butterfly of oracle/sdro_float.c's gfft_run, D = 8 and 64 */
    const float sg = inverse ? 1.0f : -1.0f;
    for (int D = 8; D < N; D *= 8) {
        const int uinc = N / 8 / D;
        for (int uu = 0; uu < D; uu++) {
            const int i2 = uu * uinc, i1 = 2 * i2;
            int i0 = 4 * i2; float w0r;
            if (uu < D / 2) w0r = u[i0]; else { i0 = N / 2 - i0; w0r = -u[i0]; }
            const float w0i = u[N / 4 - i0];
            const float w1c = u[i1], w1i = u[N / 4 - i1];
            const float w2r = u[i2], w2i = u[N / 4 - i2];
            const float w3r = u[i2 + N / 8], w3i = u[N / 4 - i2 - N / 8];
            for (int g = 0; g < N / 8 / D; g++) {
                cf* p = y + (size_t)g * 8 * D + uu;
                cf f0 = p[0], f1 = p[D], f2 = p[2 * D], f3 = p[3 * D], f4 = p[4 * D], f5 = p[5 * D], f6 = p[6 * D], f7 = p[7 * D];
                cf t0, t1;
                t0 = c_plus(f0, f1, w0r, sg * w0i);  f1 = c_two_minus(f0, t0);
                t1 = c_minus(f2, f3, w0r, sg * w0i); f2 = c_two_minus(f2, t1);
                f0 = c_plus(t0, f2, w1c, sg * w1i);  f2 = c_two_minus(t0, f0);
                f3 = c_plus(f1, t1, w1i, -sg * w1c); f1 = c_two_minus(f1, f3);
                t0 = c_plus(f4, f5, w0r, sg * w0i);  f5 = c_two_minus(f4, t0);
                t1 = c_minus(f6, f7, w0r, sg * w0i); f6 = c_two_minus(f6, t1);
                f4 = c_plus(t0, f6, w1c, sg * w1i);  f6 = c_two_minus(t0, f4);
                f7 = c_plus(f5, t1, w1i, -sg * w1c); f5 = c_two_minus(f5, f7);
                t0 = c_minus(f0, f4, w2r, sg * w2i); f0 = c_two_minus(f0, t0);
                t1 = c_minus(f1, f5, w3r, sg * w3i); f1 = c_two_minus(f1, t1);
                p[4 * D] = t0; p[5 * D] = t1; p[0] = f0; p[D] = f1;
                { const cf n4 = c_minus(f2, f6, w2i, -sg * w2r); f6 = c_two_minus(f2, n4); f4 = n4; }
                { const cf n5 = c_minus(f3, f7, w3i, -sg * w3r); f7 = c_two_minus(f3, n5); f5 = n5; }
                p[2 * D] = f4; p[3 * D] = f5; p[6 * D] = f6; p[7 * D] = f7;
            }
        }
    }
    memcpy(x, y, sizeof y);
}

void* udso_create(int in_rate, int nco_freq, float rate, int fmt, float rf_bw, int fm_deviation, float gain, int squelch_db, int squelch_gate,
                  int squelch_enabled, int agc)
{
    if (fmt < 4 || fmt > 7) return 0;
    udso* h = (udso*)calloc(1, sizeof(udso));
    h->u = (udpo*)udpo_create(in_rate, nco_freq, rate, fmt, rf_bw, fm_deviation, gain, squelch_db, squelch_gate, squelch_enabled, agc);
    h->u->sq_gate = (int)(rate * 0.05);                     /* m_squelchGate = settings.m_outputSampleRate * 0.05; the release stays */
    h->u->agc_on = agc != 0;                                /* udpsrc.cpp:155-163 excludes formats 0 .. 3 only */
    h->last_open = -1;
    /* fftCosInit for 512 points */
    h->utbl[0] = 1.0f;
    for (int i = 1; i < SSB_N / 4; i++) h->utbl[i] = (float)cos((2.0 * 3.141592653589793238462643383279502884197 * (float)i) / (float)SSB_N);
    h->utbl[SSB_N / 4] = 0.0f;
    /* UDPFilter = new fftfilt(0.0, (m_settings.m_rfBandwidth / 2.0) / m_settings.m_outputSampleRate, udpBlockSize) in the constructor,
     * where m_settings holds the defaults 12500 and 48000; create_filter(0, f2): low pass, Blackman, forward FFT, max |H| of bins 0 .. 255 */
    const float f2 = (float)((12500.0f / 2.0) / 48000.0f);
    for (int i = 0; i < SSB_H; i++) {
        h->filter[i].r = 0; h->filter[i].i = 0;
        if (f2 != 0) h->filter[i].r += fsinc(f2, i, SSB_H);
    }
    for (int i = 0; i < SSB_H; i++) { const float w = blackman(i, SSB_H); h->filter[i].r *= w; h->filter[i].i *= w; }
    fft512(h->utbl, h->filter, 0);
    float scale = 0;
    for (int i = 0; i < SSB_H; i++) { const float mag = hypotf(h->filter[i].r, h->filter[i].i); if (mag > scale) scale = mag; }
    if (scale != 0) for (int i = 0; i < SSB_N; i++) { h->filter[i].r /= scale; h->filter[i].i /= scale; }
    return h;
}

void udso_destroy(void* p)
{
    udso* h = (udso*)p;
    if (!h) return;
    udpo_destroy(h->u);
    free(h);
}

/* fftfilt::runSSB(in, &out, usb), getDC = true */
static int run_ssb(udso* h, cf in, int usb)
{
    h->data[h->inptr++] = in;
    if (h->inptr < SSB_H) return 0;
    h->inptr = 0;
    fft512(h->utbl, h->data, 0);
    h->data[0] = c_mul(h->data[0], h->filter[0]);
    if (usb) for (int i = 1; i < SSB_H; i++) { h->data[i] = c_mul(h->data[i], h->filter[i]); h->data[SSB_H + i].r = 0; h->data[SSB_H + i].i = 0; }
    else     for (int i = 1; i < SSB_H; i++) { h->data[i].r = 0; h->data[i].i = 0; h->data[SSB_H + i] = c_mul(h->data[SSB_H + i], h->filter[SSB_H + i]); }
    fft512(h->utbl, h->data, 1);
    for (int i = 0; i < SSB_H; i++) {
        h->out[i].r = h->ovl[i].r + h->data[i].r; h->out[i].i = h->ovl[i].i + h->data[i].i;
        h->ovl[i] = h->data[SSB_H + i];
    }
    memset(h->data, 0, sizeof h->data);
    return SSB_H;
}

static void note(udso* h, double wanted, int16_t got)
{
    if (!(wanted > -2147483649.0 && wanted < 2147483648.0)) h->probe[Q_PAST_INT32]++;
    else if (trunc(wanted) != (double)got) h->probe[Q_WRAPS]++;
}

long udso_feed(void* p, const int16_t* iq, long n, void* payload, long cap, int16_t* spectrum, long* n_payload)
{
    udso* h = (udso*)p;
    udpo* u = h->u;
    if (n > u->ci_cap) {
        free(u->ci); free(u->open_flags); u->ci_cap = n + 1024;
        u->ci = (float*)malloc(sizeof(float) * 2 * (size_t)u->ci_cap); u->open_flags = (unsigned char*)malloc((size_t)u->ci_cap);
    }
    const long k = n > 0 ? (long)sdro_backend_feed(u->front, iq, n, u->ci) : 0;
    const int fmt = u->fmt, mono = fmt >= 6, usb = fmt == 5 || fmt == 7;
    int16_t* out = (int16_t*)payload;
    long w = 0;                                             /* payload elements written */
    u->n_flags = 0;
    for (long s = 0; s < k; s++) {
        float re = u->ci[2 * s], im = u->ci[2 * s + 1];
        double agcFactor = 1.0, inMagSq;
        if (u->agc_on) { agcFactor = magagc_feed(&u->agc, re, im); inMagSq = u->agc.magsq; }
        else inMagSq = (double)(re * re + im * im);
        mavg_feed(&u->in_avg, inMagSq / (32768.0 * 32768.0));
        u->in_magsq = mavg_average(&u->in_avg);
        spectrum[2 * s] = f_to_q16(re); spectrum[2 * s + 1] = f_to_q16(im);
        calculate_squelch(u, u->in_magsq);
        const int open = u->sq_open;
        u->open_flags[u->n_flags++] = (unsigned char)open;
        if (h->last_open >= 0 && open != h->last_open && h->inptr > 0) h->flips_now = 1;
        h->last_open = open;
        /* ci *= agcFactor: std::complex<float>::operator*=(float) */
        const float f = (float)agcFactor;
        re *= f; im *= f;
        cf ci; ci.r = re; ci.i = im;
        if (run_ssb(h, ci, usb)) {
            h->blocks++; h->probe[Q_BLOCKS]++; h->probe[Q_BLOCKS_OPEN] += open; h->probe[Q_FLIPS_IN_BLOCK] += h->flips_now; h->flips_now = 0;
            if (h->out[0].r != h->out[0].r) h->probe[Q_NAN_BLOCKS]++;
            for (int i = 0; i < SSB_H; i++, w++) {
                if (w >= cap) continue;
                if (!mono) {
                    const double l = open ? (double)(h->out[i].r * u->gain) : 0, r = open ? (double)(h->out[i].i * u->gain) : 0;
                    out[2 * w] = d_to_q16(l); out[2 * w + 1] = d_to_q16(r);
                    note(h, l, out[2 * w]);
                } else {
                    const double l = open ? (double)(h->out[i].r + h->out[i].i) * 0.7 * (double)u->gain : 0;
                    out[w] = d_to_q16(l);
                    note(h, l, out[w]);
                }
            }
        }
        if (fmt == 4) {                                     /* the ladder behind the unchained `if`: raw I/Q of the scaled ci */
            if (w < cap) {
                out[2 * w] = open ? f_to_q16(re * u->gain) : 0;
                out[2 * w + 1] = open ? f_to_q16(im * u->gain) : 0;
            }
            w++;
        }
        u->total++;
    }
    h->total_pay += w;
    *n_payload = w;
    return k;
}

void udso_state(void* p, double* in_magsq, long* st)
{
    udso* h = (udso*)p;
    *in_magsq = h->u->in_magsq;
    st[0] = h->u->sq_open; st[1] = h->u->sq_open_count; st[2] = h->u->sq_close_count; st[3] = h->u->total;
    st[4] = h->inptr; st[5] = h->blocks; st[6] = h->total_pay;
}
long udso_last_open(void* p, unsigned char* flags, long cap) { return udpo_last_open(((udso*)p)->u, flags, cap); }
void udso_filter(void* p, float* out) { memcpy(out, ((udso*)p)->filter, sizeof(cf) * SSB_N); }
void udso_design(void* p, int* ints) { ints[0] = ((udso*)p)->u->sq_gate; ints[1] = ((udso*)p)->u->sq_release; }
void udso_probe(void* p, long* out) { memcpy(out, ((udso*)p)->probe, sizeof(long) * Q_N); }
