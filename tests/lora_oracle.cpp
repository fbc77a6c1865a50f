/* Strict-IEEE scalar restatement of LoRaDemod::feed with detect(), synch() and dumpRaw() (plugins/channelrx/demodlora/
 * lorademod.cpp:94-288) and of the sliding FFT sfft (sdrbase/dsp/fftfilt.cpp:411-457), streaming, one demodulator per object,
 * in the reference's statement order: m_chirp and m_angle as running sums, both sliding FFTs as a loop over their bins per
 * sample with a 128-deep delay line and k2, a fetch on every 64th output, detect's loop of 128 over mov, peak, negpeak and
 * the first strict maximum, then finetune, the squelch, synch and dumpRaw.  The front (NCO, Interpolator::create / decimate)
 * is oracle/libsdro.so's sdro_backend_new_at; its output is divided by SDR_RX_SCALEF here, a power of two, which commutes
 * with the front exactly.  Nothing of the device code is used but the host versions of the four lorabits functions in
 * lora_scan.hpp (prng6, interleave6, hamming6, toGray), which tests/lora_check.cpp proves against the recording.  The
 * checker of sdrx_lora_*: tests build it with `g++ -O2 -ffp-contract=off -fno-fast-math -shared` and call it through
 * ctypes (tests/lora_cases.py); the product never links it.
 *
 * Four things the reference leaves open are pinned as include/sdrx.h and tests/golden/lora_rec.cpp pin them: mov starts as
 * zeros; mag[127] and rev[127], which fetch does not write, are 0; dumpRaw's text starts as zeros; m_count is 64 bits wide.
 *
 *   lro_create(in_rate, nco_freq, bandwidth)
 *   lro_feed(h, iq, n, samples, cap)      feed(); Samples (re, im as int16) go to samples, returns their count
 *   lro_text(h, buf, cap)                 what dumpRaw printed during the last feed; returns its length
 *   lro_state(h, out[14])                 m_tune, m_time, m_result, m_bin, m_count, lines so far; preamble locks with the
 *                                         finetune sum below zero, ... at or above, squelch closures with m_time <= 70, preamble
 *                                         locks, wraps of m_time; then the probes: most lines in one feed; fetches with
 *                                         negpeak > 0 and peak / (3 negpeak) in [0.5, 2]; fetches whose largest rev[] or largest
 *                                         five-term sum is above 0 and stands at more than one index
 *   lro_design(h, taps, &nco_inc, vrot[256], &k2, chirp[512], sample[256])    returns the taps per phase
 */
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include "../oracle/sdro.h"
#include "lora_scan.hpp"

namespace {

const int SPREAD = 256, LEN = 128, SQUELCH = 3, DATA_BITS = 6;
const double K1 = 0.99999;                                      /* fftfilt.h */

struct cf { float r, i; };

struct Sfft {                                                   /* sfft(len = 128): first = 0, last = 127 */
    cf vrot[LEN], bins[LEN], delay[LEN];
    int ptr;
    float k2;
    Sfft()
    {
        double phi = 0.0;
        const double tau = 2.0 * M_PI / LEN;
        ptr = 0;
        k2 = 1.0;
        for (int i = 0; i < LEN; i++) {
            vrot[i].r = (float)(K1 * cos(phi)); vrot[i].i = (float)(K1 * sin(phi));
            phi += tau;
            delay[i].r = delay[i].i = bins[i].r = bins[i].i = 0.0f;
            k2 = (float)(k2 * K1);
        }
    }
    void run(cf in)
    {
        cf& de = delay[ptr];
        cf z; z.r = in.r - k2 * de.r; z.i = in.i - k2 * de.i;
        de = in;
        if (++ptr >= LEN) ptr = 0;
        for (int k = 0; k < LEN - 1; k++) {                     /* first .. last - 1: bin 127 never moves */
            const float tr = bins[k].r + z.r, ti = bins[k].i + z.i;
            bins[k].r = tr * vrot[k].r - ti * vrot[k].i;
            bins[k].i = tr * vrot[k].i + ti * vrot[k].r;
        }
    }
    void fetch(float* out) const
    {
        for (int k = 0; k < LEN - 1; k++) out[k] = bins[k].r * bins[k].r + bins[k].i * bins[k].i;
    }
};

struct Lro {
    sdro_backend* front;
    float* ci; long ci_cap;
    int32_t nco_inc;
    int chirp, angle, bin, result, time;
    int64_t count;
    short tune;
    Sfft lora, nega;
    float mov[4 * LEN];
    short history[1024], finetune[16];
    std::string text;
    int64_t lines, tuned_up, tuned_plain, short_closes, locks, wraps;
    int64_t lines_in_feed, max_lines_in_feed, squelch_near, ties;
};

void dump_raw(Lro* h)
{
    char text[256];
    memset(text, 0, sizeof text);
    short max = (short)(h->time / 4 - 3), j;
    if (max > 140) max = 140;
    for (j = 0; j < max; j++) {
        const short bin = (short)((h->history[(j + 1) * 4] + h->tune) & (LEN - 1));
        text[j] = (char)sdrx::lora_to_gray((short)(bin >> 1));
    }
    sdrx::lora_prng6(text, max);
    sdrx::lora_interleave6(text, 6);
    sdrx::lora_interleave6(&text[8], max);
    sdrx::lora_hamming6(text, 6);
    sdrx::lora_hamming6(&text[8], max);
    for (j = 0; j < max / 2; j++) {
        const signed char v = (signed char)(((signed char)text[j * 2 + 1] << 4) | (0xf & (signed char)text[j * 2 + 0]));
        text[j] = (v < 32 || v > 126) ? (char)0x5f : (char)v;
    }
    text[3] = text[2];
    text[2] = text[1];
    text[1] = text[0];
    text[j] = 0;
    h->text += &text[1];
    h->text += "\n";
    h->lines++;
    h->lines_in_feed++;
}

short synch(Lro* h, short bin)
{
    if (bin < 0) {
        if (h->time > 70) dump_raw(h); else h->short_closes++;
        h->time = 0;
        return -1;
    }
    h->history[h->time] = bin;
    if (h->time > 12 && bin == h->history[h->time - 6] && bin == h->history[h->time - 12]) {
        h->tune = (short)(LEN - bin);
        short j = 0;
        for (short i = 0; i < 12; i++) j = (short)(j + h->finetune[15 & (h->time - i)]);
        if (j < 0) { h->tune = (short)(h->tune + 1); h->tuned_up++; } else h->tuned_plain++;
        h->tune &= (LEN - 1);
        h->time = 0;
        h->locks++;
        return -1;
    }
    h->time++;
    if (h->time > 1023) h->wraps++;
    h->time &= 1023;
    if (h->time & 3) return -1;
    return (short)((bin + h->tune) & (LEN - 1));
}

int detect(Lro* h, cf c, cf a)
{
    cf up, dn;                                                  /* c * a and c * conj(a), std::complex<float> products */
    up.r = c.r * a.r - c.i * a.i; up.i = c.r * a.i + c.i * a.r;
    const float nai = -a.i;
    dn.r = c.r * a.r - c.i * nai; dn.i = c.r * nai + c.i * a.r;
    h->lora.run(up);
    h->nega.run(dn);
    if (++h->count & ((1 << DATA_BITS) - 1)) return h->result;

    const int movpoint = (int)(3 & (h->count >> DATA_BITS));
    float mag[LEN], rev[LEN], sum[LEN];
    mag[LEN - 1] = rev[LEN - 1] = 0.0f;
    h->lora.fetch(mag);
    h->nega.fetch(rev);
    float peak = 0.0f, negpeak = 0.0f;
    short result = 0, negresult = 0;
    for (short i = 0; i < LEN; i++) {
        if (rev[i] > negpeak) { negpeak = rev[i]; negresult = i; }
        const float t = h->mov[i] + h->mov[LEN + i] + h->mov[2 * LEN + i] + h->mov[3 * LEN + i] + mag[i];
        sum[i] = t;
        if (t > peak) { peak = t; result = i; }
        h->mov[movpoint * LEN + i] = mag[i];
    }
    (void)negresult;
    /* probes */
    int at_peak = 0, at_negpeak = 0;
    for (int i = 0; i < LEN; i++) { at_peak += sum[i] == peak; at_negpeak += rev[i] == negpeak; }
    if ((peak > 0.0f && at_peak > 1) || (negpeak > 0.0f && at_negpeak > 1)) h->ties++;
    if (negpeak > 0.0f) {
        const double q = (double)peak / (3.0 * (double)negpeak);
        if (q >= 0.5 && q <= 2.0) h->squelch_near++;
    }
    const int p = (result - 1 + LEN) & (LEN - 1), q = (result + 1) & (LEN - 1);
    h->finetune[15 & h->time] = (mag[p] > mag[q]) ? -1 : 1;
    if (peak < negpeak * SQUELCH) result = -1;
    result = synch(h, result);
    if (result >= 0) h->result = result;
    return h->result;
}

} // namespace

extern "C" {

void* lro_create(int in_rate, int nco_freq, int bandwidth)
{
    Lro* h = new Lro;
    const float bw = (float)bandwidth;                          /* Real m_Bandwidth */
    const float step = (float)in_rate / bw;
    h->front = sdro_backend_new_at((float)nco_freq, (double)in_rate, 16, bw / 1.9, 4.5, step, step);
    h->nco_inc = sdro_nco_inc((float)nco_freq, (float)in_rate);
    h->ci = 0; h->ci_cap = 0;
    h->chirp = h->angle = h->bin = h->result = h->time = 0;
    h->count = 0;
    h->tune = 0;
    memset(h->mov, 0, sizeof h->mov);
    memset(h->history, 0, sizeof h->history);
    memset(h->finetune, 0, sizeof h->finetune);
    h->lines = h->tuned_up = h->tuned_plain = h->short_closes = h->locks = h->wraps = 0;
    h->lines_in_feed = h->max_lines_in_feed = h->squelch_near = h->ties = 0;
    return h;
}

void lro_destroy(void* p)
{
    Lro* h = (Lro*)p;
    if (!h) return;
    sdro_backend_free(h->front);
    free(h->ci);
    delete h;
}

long lro_feed(void* p, const int16_t* iq, long n, int16_t* samples, long cap)
{
    Lro* h = (Lro*)p;
    if (n + 4 > h->ci_cap) {
        free(h->ci);
        h->ci_cap = n + 4;
        h->ci = (float*)malloc(sizeof(float) * 2 * (size_t)h->ci_cap);
    }
    h->text.clear();
    h->lines_in_feed = 0;
    const long k = (long)sdro_backend_feed(h->front, iq, n, h->ci);         /* the step is >= 1: at most one output per input */
    long out = 0;
    for (long g = 0; g < k; g++) {
        cf c; c.r = h->ci[2 * g] / 32768.0f; c.i = h->ci[2 * g + 1] / 32768.0f;
        h->chirp = (h->chirp + 1) & (SPREAD - 1);
        h->angle = (h->angle + h->chirp) & (SPREAD - 1);
        cf a; a.r = (float)cos(M_PI * 2 * h->angle / SPREAD); a.i = (float)-sin(M_PI * 2 * h->angle / SPREAD);
        const int newangle = detect(h, c, a);
        h->bin = (h->bin + newangle) & (LEN - 1);
        const float re = (float)cos(M_PI * 2 * h->bin / LEN), im = (float)sin(M_PI * 2 * h->bin / LEN);
        if (out < cap) { samples[2 * out] = (int16_t)(re * 100); samples[2 * out + 1] = (int16_t)(im * 100); }
        out++;
    }
    if (h->lines_in_feed > h->max_lines_in_feed) h->max_lines_in_feed = h->lines_in_feed;
    return out;
}

long lro_text(void* p, char* buf, long cap)
{
    Lro* h = (Lro*)p;
    const long n = (long)h->text.size();
    if (n <= cap) memcpy(buf, h->text.data(), (size_t)n);
    return n;
}

void lro_state(void* p, int64_t* out)
{
    Lro* h = (Lro*)p;
    const int64_t v[14] = { h->tune, h->time, h->result, h->bin, h->count, h->lines, h->tuned_up, h->tuned_plain, h->short_closes,
                            h->locks, h->wraps, h->max_lines_in_feed, h->squelch_near, h->ties };
    memcpy(out, v, sizeof v);
}

int lro_design(void* p, float* taps, int32_t* nco_inc, float* vrot, float* k2, float* chirp, int16_t* sample)
{
    Lro* h = (Lro*)p;
    const int nt = sdro_backend_ntaps(h->front);
    memcpy(taps, sdro_backend_taps(h->front), sizeof(float) * 16 * (size_t)nt);
    *nco_inc = h->nco_inc;
    for (int i = 0; i < LEN; i++) { vrot[2 * i] = h->lora.vrot[i].r; vrot[2 * i + 1] = h->lora.vrot[i].i; }
    *k2 = h->lora.k2;
    for (int a = 0; a < SPREAD; a++) {
        chirp[2 * a] = (float)cos(M_PI * 2 * a / SPREAD);
        chirp[2 * a + 1] = (float)-sin(M_PI * 2 * a / SPREAD);
    }
    for (int m = 0; m < LEN; m++) {
        const float re = (float)cos(M_PI * 2 * m / LEN), im = (float)sin(M_PI * 2 * m / LEN);
        sample[2 * m] = (int16_t)(re * 100); sample[2 * m + 1] = (int16_t)(im * 100);
    }
    return nt;
}

} // extern "C"
