/* Strict-IEEE C restatement of SpectrumVis::feed / handleConfigure (sdrgui/dsp/spectrumvis.cpp:70-300, v4.0.6) with the
 * kissfft engine (sdrbase/dsp/kissfft.h), FFTWindow (fftwindow.{h,cpp}), MovingAverage2D<double> and FixedAverage2D<double>
 * (util/movingaverage2d.h, util/fixedaverage2d.h).  The checker of sdrx_spectrum_*: tests build it with
 * `cc -O2 -ffp-contract=off -shared` and call it through ctypes; the product never links it.
 *
 *   spo_create(scalef)                                   SpectrumVis(scalef): zero buffer, handleConfigure(1024, 0, 0, None, BlackmanHarris, false)
 *   spo_configure(h, N, pct, avg_nb, mode, window, lin)  handleConfigure; returns 0, or -1 where sdrx_spectrum_* rejects the configuration
 *   spo_feed(h, iq, n, positive_only, out, cap)          feed(); every newSpectrum frame (N floats) goes to out, returns the frame count
 *   spo_window(h, out)                                   m_window; returns N
 *   spo_set_log2_double(h, on)                           on: log2f(v) evaluated as (float)log2((double)v), the device's choice; off
 *                                                        (default): glibc's log2f, as the reference
 */
#include <complex.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define MAX_FFT 4096

typedef struct { float re, im; } cpx;

typedef struct {
    float scalef;
    cpx buf[MAX_FFT];                 /* m_fftBuffer */
    cpx in[MAX_FFT], out[MAX_FFT];    /* KissEngine m_in / m_out */
    float power[MAX_FFT];             /* m_powerSpectrum */
    float window[MAX_FFT];
    cpx tw[MAX_FFT];
    int radix[16], remain[16];
    int n, ov, refill, fill, mode, linear, log2_double;
    unsigned avg_nb;
    float ofs, powdiv, mult;
    /* MovingAverage2D<double> */
    double *mdata, *msum; unsigned mwidth, mdepth, midx;
    /* FixedAverage2D<double> */
    double *fsum; unsigned fwidth, fsize, fidx;
} spo;

static cpx cadd(cpx a, cpx b) { cpx c = { a.re + b.re, a.im + b.im }; return c; }
static cpx csub(cpx a, cpx b) { cpx c = { a.re - b.re, a.im - b.im }; return c; }
static cpx cmul(cpx a, cpx b) { cpx c = { a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re }; return c; }

/* ---- FFTWindow: Real arguments, double arithmetic ---- */
static const double PI_D = 3.14159265358979323846;
static float win_fn(int fn, float n, float i)
{
    switch (fn) {
    case 0: return (float)((2.0 / (n - 1.0)) * ((n - 1.0) / 2.0 - fabs(i - (n - 1.0) / 2.0)) * 2.0);
    case 1: return (float)((0.35875 - 0.48829 * cos((2.0 * PI_D * i) / n) + 0.14128 * cos((4.0 * PI_D * i) / n) - 0.01168 * cos((6.0 * PI_D * i) / n)) * 2.79);
    case 2: return (float)(1.0 - 1.93 * cos((2.0 * PI_D * i) / n) + 1.29 * cos((4.0 * PI_D * i) / n) - 0.388 * cos((6.0 * PI_D * i) / n) + 0.03222 * cos((8.0 * PI_D * i) / n));
    case 3: return (float)((0.54 - 0.46 * cos((2.0 * PI_D * i) / n)) * 1.855);
    case 4: return (float)((0.5 - 0.5 * cos((2.0 * PI_D * i) / n)) * 2.0);
    default: return 1.0f;
    }
}

/* ---- kissfft, forward, float ---- */
static void kiss_prepare(spo* h)
{
    const int nfft = h->n;
    const float phinc = -2 * acosf(-1.0f) / nfft;
    for (int i = 0; i < nfft; i++) {
        const float complex t = cexpf(CMPLXF(0.0f, i * phinc));
        h->tw[i].re = crealf(t); h->tw[i].im = cimagf(t);
    }
    int n = nfft, p = 4, s = 0;
    do {
        while (n % p) {
            p = p == 4 ? 2 : p == 2 ? 3 : p + 2;
            if (p * p > n) p = n;
        }
        n /= p;
        h->radix[s] = p; h->remain[s] = n; s++;
    } while (n > 1);
}

static void bfly2(spo* h, cpx* F, size_t fstride, int m)
{
    for (int k = 0; k < m; ++k) {
        const cpx t = cmul(F[m + k], h->tw[k * fstride]);
        F[m + k] = csub(F[k], t);
        F[k] = cadd(F[k], t);
    }
}

static void bfly4(spo* h, cpx* F, size_t fstride, size_t m)
{
    cpx s[7];
    for (size_t k = 0; k < m; ++k) {
        s[0] = cmul(F[k + m], h->tw[k * fstride]);
        s[1] = cmul(F[k + 2 * m], h->tw[k * fstride * 2]);
        s[2] = cmul(F[k + 3 * m], h->tw[k * fstride * 3]);
        s[5] = csub(F[k], s[1]);
        F[k] = cadd(F[k], s[1]);
        s[3] = cadd(s[0], s[2]);
        s[4] = csub(s[0], s[2]);
        { const cpx t = { s[4].im * 1, -s[4].re * 1 }; s[4] = t; }   /* negative_if_inverse = 1 */
        F[k + 2 * m] = csub(F[k], s[3]);
        F[k] = cadd(F[k], s[3]);
        F[k + m] = cadd(s[5], s[4]);
        F[k + 3 * m] = csub(s[5], s[4]);
    }
}

static void kf_work(spo* h, int stage, cpx* Fout, const cpx* f, size_t fstride)
{
    const int p = h->radix[stage], m = h->remain[stage];
    cpx* beg = Fout;
    cpx* end = Fout + p * m;
    if (m == 1) {
        do { *Fout = *f; f += fstride; } while (++Fout != end);
    } else {
        do { kf_work(h, stage + 1, Fout, f, fstride * p); f += fstride; } while ((Fout += m) != end);
    }
    if (p == 2) bfly2(h, beg, fstride, m); else bfly4(h, beg, fstride, (size_t)m);   /* powers of two only */
}

/* ---- averaging ---- */
static double mov_store_get(spo* h, double v, unsigned i)
{
    if (h->mdepth <= 1) return v;
    if (i >= h->mwidth) return 0;
    const double first = h->mdata[h->midx * h->mwidth + i];
    h->msum[i] += (v - first);
    h->mdata[h->midx * h->mwidth + i] = v;
    return h->msum[i] / h->mdepth;
}
static void mov_next(spo* h) { h->midx = h->midx == h->mdepth - 1 ? 0 : h->midx + 1; }
static int fix_store_get(spo* h, double* avg, double v, unsigned i)
{
    if (h->fsize <= 1) { *avg = v; return 1; }
    h->fsum[i] += v;
    if (h->fidx == h->fsize - 1) { *avg = h->fsum[i] / h->fsize; return 1; }
    return 0;
}
static int fix_next(spo* h)
{
    if (h->fsize <= 1) return 1;
    if (h->fidx == h->fsize - 1) { h->fidx = 0; memset(h->fsum, 0, sizeof(double) * h->fwidth); return 1; }
    h->fidx++;
    return 0;
}

/* ---- API ---- */
int spo_configure(spo* h, int fft_size, int pct, unsigned avg_nb, int mode, int window, int linear)
{
    if (fft_size > MAX_FFT) fft_size = MAX_FFT; else if (fft_size < 64) fft_size = 64;
    pct = pct > 100 ? 100 : pct < 0 ? 0 : pct;
    const int ov = fft_size * pct / 100;
    if ((fft_size & (fft_size - 1)) || 2 * ov >= fft_size || window < 0 || window > 5 || mode < 0 || mode > 2) return -1;
    h->n = fft_size;
    kiss_prepare(h);
    for (int i = 0; i < fft_size; i++) h->window[i] = win_fn(window, (float)fft_size, (float)i);
    h->ov = ov;
    h->refill = fft_size - ov;
    h->fill = ov;
    /* MovingAverage2D::resize(fftSize, averageNb) / FixedAverage2D::resize(fftSize, averageNb) */
    free(h->mdata); free(h->msum); free(h->fsum);
    h->mdata = (double*)calloc((size_t)fft_size * (avg_nb ? avg_nb : 1), sizeof(double));
    h->msum = (double*)calloc((size_t)fft_size, sizeof(double));
    h->fsum = (double*)calloc((size_t)fft_size, sizeof(double));
    h->mwidth = h->fwidth = (unsigned)fft_size;
    h->mdepth = h->fsize = avg_nb;
    h->midx = h->fidx = 0;
    h->avg_nb = avg_nb;
    h->mode = mode;
    h->linear = linear;
    h->ofs = 20.0f * log10f(1.0f / fft_size);
    h->powdiv = (float)(fft_size * fft_size);
    return 0;
}

spo* spo_create(float scalef)
{
    spo* h = (spo*)calloc(1, sizeof(spo));
    h->scalef = scalef;
    h->mult = 10.0f / log2f(10.0f);
    spo_configure(h, 1024, 0, 0, 0, 1, 0);
    return h;
}

void spo_destroy(spo* h)
{
    if (!h) return;
    free(h->mdata); free(h->msum); free(h->fsum); free(h);
}

int spo_window(const spo* h, float* out)
{
    memcpy(out, h->window, sizeof(float) * (size_t)h->n);
    return h->n;
}

static float lg2(const spo* h, float v) { return h->log2_double ? (float)log2((double)v) : log2f(v); }
static float db_or_lin(const spo* h, float v) { return h->linear ? v / h->powdiv : h->mult * lg2(h, v) + h->ofs; }
void spo_set_log2_double(spo* h, int on) { h->log2_double = on; }

long spo_feed(spo* h, const int16_t* iq, long n, int positive_only, float* out, long cap_frames)
{
    long pos = 0, emitted = 0;
    const size_t half = (size_t)h->n / 2;
    while (pos < n) {
        const size_t todo = (size_t)(n - pos);
        const size_t needed = (size_t)(h->refill - h->fill);
        if (todo >= needed) {
            for (size_t i = 0; i < needed; ++i, ++pos) {
                h->buf[h->fill + i].re = iq[2 * pos] / h->scalef;
                h->buf[h->fill + i].im = iq[2 * pos + 1] / h->scalef;
            }
            for (int i = 0; i < h->n; i++) { h->in[i].re = h->buf[i].re * h->window[i]; h->in[i].im = h->buf[i].im * h->window[i]; }
            kf_work(h, 0, h->out, h->in, 1);
            const cpx* o = h->out;
            int emit = 1;
            for (size_t i = 0; i < half; i++) {
                /* positiveOnly: bin i -> 2i, 2i+1;  else bin i + half -> i, bin i -> i + half (the reference's visiting order) */
                for (int part = 0; part < (positive_only ? 1 : 2); part++) {
                    const size_t bin = positive_only ? i : (part == 0 ? i + half : i);
                    const cpx c = o[bin];
                    float v = c.re * c.re + c.im * c.im;
                    float val;
                    int have = 1;
                    if (h->mode == 0) {
                        val = db_or_lin(h, v);
                    } else if (h->mode == 1) {
                        v = (float)mov_store_get(h, v, (unsigned)bin);
                        val = db_or_lin(h, v);
                    } else {
                        double avg;
                        have = fix_store_get(h, &avg, v, (unsigned)bin);
                        if (have) avg = h->linear ? v / h->powdiv : h->mult * lg2(h, (float)avg) + h->ofs;
                        val = (float)avg;
                    }
                    if (!have) continue;
                    if (positive_only) { h->power[2 * i] = val; h->power[2 * i + 1] = val; }
                    else h->power[part == 0 ? i : i + half] = val;
                }
            }
            if (h->mode == 1) mov_next(h);
            else if (h->mode == 2) emit = fix_next(h);
            if (emit) {
                if (emitted < cap_frames) memcpy(out + (size_t)emitted * (size_t)h->n, h->power, sizeof(float) * (size_t)h->n);
                emitted++;
            }
            memmove(h->buf, h->buf + h->refill, sizeof(cpx) * (size_t)(MAX_FFT - h->refill));
            h->fill = h->ov;
        } else {
            for (size_t i = 0; pos < n; ++pos, ++i) {
                h->buf[h->fill + i].re = iq[2 * pos] / h->scalef;
                h->buf[h->fill + i].im = iq[2 * pos + 1] / h->scalef;
            }
            h->fill += (int)todo;
        }
    }
    return emitted;
}
