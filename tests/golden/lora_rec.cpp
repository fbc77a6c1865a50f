// Recorder around the reference's own NCO, Interpolator and sfft, compiled where they lie by tests/golden/make_golden_lora.py
// (strict IEEE, scalar: -O2 -fno-fast-math -ffp-contract=off, USE_SSE2 undefined), and its lorabits.h, included from the
// reference tree into the stand-in class below, which declares the four functions that header defines.  LoRaDemod itself
// cannot be instantiated outside the application, so feed / detect / synch / dumpRaw are written here line for line around the
// real members, in the state the constructor leaves them in.  Four things the reference leaves open are pinned (include/sdrx.h):
// mov starts as zeros; mag[127] and rev[127], which sfft::fetch does not write, are 0; dumpRaw's text starts as zeros; m_count
// is 64 bits wide.  dumpRaw's printf goes to the feed's text.
//
//   lora_rec <input.bin> <output.bin> [trace.bin]     commands on stdin, one per line:
//     new in_rate nco_freq bandwidth       a fresh demodulator
//     feed n                               the next n Samples of input.bin (int16 I, Q)
//     end                                  the state
//     design                               the design products
//   output.bin: per feed an int64 count, the Samples (re, im as int16), an int64 byte count and the text; per end: int64 m_tune,
//     m_time, m_result, m_bin, m_count, lines so far, fetches at which the last twelve finetune summed below zero at a preamble
//     lock, ... at or above zero, squelch closures with m_time <= 70, preamble locks, wraps of m_time; per design: int64 taps per
//     phase, the 16 * that polyphase taps, vrot[128] as pairs, k2, the dechirp table [256] as pairs, the Sample table [128] as pairs
//   trace.bin (optional), per fetch 261 floats: mag[128], rev[128], result before the squelch, after it, m_time, m_tune, m_result
//     after synch()
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "dsp/dsptypes.h"
#include "dsp/nco.h"
#define private public
#define protected public
#include "dsp/interpolator.h"
#include "dsp/fftfilt.h"
#undef protected
#undef private

#define SPREADFACTOR (1<<8)
#define LORA_SFFT_LEN (SPREADFACTOR / 2)
#define LORA_SQUELCH (3)
#define DATA_BITS (6)

class LoRaDemod {
public:
    LoRaDemod(int sampleRate, int frequency, int bandwidth, FILE* tr);
    ~LoRaDemod();
    void feed(const std::vector<Sample>& in);
    int detect(Complex sample, Complex angle);
    void dumpRaw(void);
    short synch(short bin);
    void interleave6(char* inout, int size);
    short toGray(short bin);
    void hamming6(char* inout, int size);
    void prng6(char* inout, int size);

    Real m_Bandwidth;
    int m_sampleRate;
    int m_chirp, m_angle, m_bin, m_result;
    int64_t m_count;
    int m_time;
    short m_tune;
    sfft* loraFilter;
    sfft* negaFilter;
    float* mov;
    short* history;
    short* finetune;
    NCO m_nco;
    Interpolator m_interpolator;
    Real m_sampleDistanceRemain;
    std::vector<Sample> m_sampleBuffer;
    std::string text;
    int64_t lines, tunedUp, tunedPlain, shortCloses, locks, wraps;
    FILE* trace;
};

#include "lorabits.h"

LoRaDemod::LoRaDemod(int sampleRate, int frequency, int bandwidth, FILE* tr) :
    lines(0), tunedUp(0), tunedPlain(0), shortCloses(0), locks(0), wraps(0), trace(tr)
{
    m_Bandwidth = bandwidth;
    m_sampleRate = sampleRate;
    m_nco.setFreq(frequency, m_sampleRate);
    m_interpolator.create(16, m_sampleRate, m_Bandwidth/1.9);
    m_sampleDistanceRemain = (Real)m_sampleRate / m_Bandwidth;
    m_chirp = 0; m_angle = 0; m_bin = 0; m_result = 0; m_count = 0; m_time = 0; m_tune = 0;
    loraFilter = new sfft(LORA_SFFT_LEN);
    negaFilter = new sfft(LORA_SFFT_LEN);
    mov = new float[4*LORA_SFFT_LEN]();         // pinned: zeros
    history = new short[1024];
    finetune = new short[16];
}

LoRaDemod::~LoRaDemod()
{
    delete loraFilter; delete negaFilter;
    delete [] mov; delete [] history; delete [] finetune;
}

void LoRaDemod::dumpRaw()
{
    short bin, j, max;
    char text[256];
    std::memset(text, 0, sizeof text);          // pinned: zeros

    max = m_time / 4 - 3;
    if (max > 140)
        max = 140;
    for ( j=0; j < max; j++)
    {
        bin = (history[(j + 1)  * 4] + m_tune ) & (LORA_SFFT_LEN - 1);
        text[j] = toGray(bin >> 1);
    }
    prng6(text, max);
    interleave6(text, 6);
    interleave6(&text[8], max);
    hamming6(text, 6);
    hamming6(&text[8], max);
    for ( j=0; j < max / 2; j++)
    {
        text[j] = (text[j * 2 + 1] << 4) | (0xf & text[j * 2 + 0]);
        if ((text[j] < 32 )||( text[j] > 126))
            text[j] = 0x5f;
    }
    text[3] = text[2];
    text[2] = text[1];
    text[1] = text[0];
    text[j] = 0;
    this->text += &text[1];
    this->text += "\n";
    lines++;
}

short LoRaDemod::synch(short bin)
{
    short i, j;
    if (bin < 0)
    {
        if (m_time > 70)
            dumpRaw();
        else
            shortCloses++;
        m_time = 0;
        return -1;
    }
    history[m_time] = bin;
    if (m_time > 12)
    {
        if (bin == history[m_time - 6])
        {
            if (bin == history[m_time - 12])
            {
                m_tune = LORA_SFFT_LEN - bin;
                j = 0;
                for (i=0; i<12; i++)
                    j += finetune[15 & (m_time - i)];
                if (j < 0)
                {
                    m_tune += 1;
                    tunedUp++;
                }
                else
                    tunedPlain++;
                m_tune &= (LORA_SFFT_LEN - 1);
                m_time = 0;
                locks++;
                return -1;
            }
        }
    }
    m_time++;
    if (m_time > 1023) wraps++;
    m_time &= 1023;
    if (m_time & 3)
        return -1;
    return (bin + m_tune) & (LORA_SFFT_LEN - 1);
}

int LoRaDemod::detect(Complex c, Complex a)
{
    int p, q;
    short i, result, negresult, movpoint;
    float peak, negpeak, tfloat;
    float mag[LORA_SFFT_LEN];
    float rev[LORA_SFFT_LEN];

    loraFilter->run(c * a);
    negaFilter->run(c * conj(a));

    if (++m_count & ((1 << DATA_BITS) - 1))
        return m_result;

    movpoint = 3 & (m_count >> DATA_BITS);
    mag[LORA_SFFT_LEN - 1] = rev[LORA_SFFT_LEN - 1] = 0.0f;     // pinned: fetch writes 127 values
    loraFilter->fetch(mag);
    negaFilter->fetch(rev);
    peak = negpeak = 0.0f;
    result = negresult = 0;
    for (i = 0; i < LORA_SFFT_LEN; i++)
    {
        if (rev[i] > negpeak)
        {
            negpeak = rev[i];
            negresult = i;
        }
        tfloat = mov[i] + mov[LORA_SFFT_LEN + i] +mov[2 * LORA_SFFT_LEN + i]
                + mov[3 * LORA_SFFT_LEN + i] + mag[i];
        if (tfloat > peak)
        {
            peak = tfloat;
            result = i;
        }
        mov[movpoint * LORA_SFFT_LEN + i] = mag[i];
    }
    p = (result - 1 + LORA_SFFT_LEN) & (LORA_SFFT_LEN -1);
    q = (result + 1) & (LORA_SFFT_LEN -1);
    finetune[15 & m_time] = (mag[p] > mag[q]) ? -1 : 1;
    const short before = result;
    if (peak < negpeak * LORA_SQUELCH)
        result = -1;
    const short after = result;
    result = synch(result);
    if (result >= 0)
        m_result = result;
    if (trace) {
        std::fwrite(mag, 4, LORA_SFFT_LEN, trace); std::fwrite(rev, 4, LORA_SFFT_LEN, trace);
        const float t[5] = { (float)before, (float)after, (float)m_time, (float)m_tune, (float)m_result };
        std::fwrite(t, 4, 5, trace);
    }
    return m_result;
}

void LoRaDemod::feed(const std::vector<Sample>& in)
{
    int newangle;
    Complex ci;
    m_sampleBuffer.clear();
    text.clear();
    for (std::vector<Sample>::const_iterator it = in.begin(); it < in.end(); ++it)
    {
        Complex c(it->real() / SDR_RX_SCALEF, it->imag() / SDR_RX_SCALEF);
        c *= m_nco.nextIQ();
        if(m_interpolator.decimate(&m_sampleDistanceRemain, c, &ci))
        {
            m_chirp = (m_chirp + 1) & (SPREADFACTOR - 1);
            m_angle = (m_angle + m_chirp) & (SPREADFACTOR - 1);
            Complex cangle(cos(M_PI*2*m_angle/SPREADFACTOR),-sin(M_PI*2*m_angle/SPREADFACTOR));
            newangle = detect(ci, cangle);
            m_bin = (m_bin + newangle) & (LORA_SFFT_LEN - 1);
            Complex nangle(cos(M_PI*2*m_bin/LORA_SFFT_LEN),sin(M_PI*2*m_bin/LORA_SFFT_LEN));
            m_sampleBuffer.push_back(Sample(nangle.real() * 100, nangle.imag() * 100));
            m_sampleDistanceRemain += (Real)m_sampleRate / m_Bandwidth;
        }
    }
}

struct sfft::vrot_bins_pair { cmplx vrot; cmplx bins; };        // as fftfilt.cpp has it, for the design dump

int main(int argc, char** argv)
{
    if (argc != 3 && argc != 4) { std::fprintf(stderr, "usage: lora_rec input.bin output.bin [trace.bin]\n"); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    FILE* tr = argc == 4 ? std::fopen(argv[3], "wb") : 0;
    if (!in || !out || (argc == 4 && !tr)) { std::perror("open"); return 2; }
    LoRaDemod* d = 0;
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        char cmd[16] = "";
        if (std::sscanf(line, "%15s", cmd) != 1) continue;
        if (!std::strcmp(cmd, "new")) {
            int inRate, ncoFreq, bw;
            if (std::sscanf(line, "%*s %d %d %d", &inRate, &ncoFreq, &bw) != 3) return 3;
            delete d;
            d = new LoRaDemod(inRate, ncoFreq, bw, tr);
        } else if (!std::strcmp(cmd, "feed") && d) {
            long n;
            if (std::sscanf(line, "%*s %ld", &n) != 1) return 3;
            std::vector<Sample> s((size_t)n);
            for (long i = 0; i < n; i++) {
                int16_t iq[2];
                if (std::fread(iq, 2, 2, in) != 2) return 4;
                s[(size_t)i] = Sample(iq[0], iq[1]);
            }
            d->feed(s);
            const int64_t k = (int64_t)d->m_sampleBuffer.size(), nb = (int64_t)d->text.size();
            std::fwrite(&k, 8, 1, out);
            for (int64_t i = 0; i < k; i++) { const int16_t v[2] = { d->m_sampleBuffer[(size_t)i].real(), d->m_sampleBuffer[(size_t)i].imag() }; std::fwrite(v, 2, 2, out); }
            std::fwrite(&nb, 8, 1, out);
            if (nb) std::fwrite(d->text.data(), 1, (size_t)nb, out);
        } else if (!std::strcmp(cmd, "end") && d) {
            const int64_t st[11] = { d->m_tune, d->m_time, d->m_result, d->m_bin, d->m_count, d->lines, d->tunedUp, d->tunedPlain, d->shortCloses, d->locks, d->wraps };
            std::fwrite(st, 8, 11, out);
        } else if (!std::strcmp(cmd, "design") && d) {
            const int64_t nt = d->m_interpolator.m_nTaps;
            std::fwrite(&nt, 8, 1, out);
            for (int64_t i = 0; i < nt * 16; i++) std::fwrite(&d->m_interpolator.m_alignedTaps[2 * i], 4, 1, out);
            for (int i = 0; i < LORA_SFFT_LEN; i++) { const float v[2] = { d->loraFilter->vrot_bins[i].vrot.real(), d->loraFilter->vrot_bins[i].vrot.imag() }; std::fwrite(v, 4, 2, out); }
            std::fwrite(&d->loraFilter->k2, 4, 1, out);
            for (int a = 0; a < SPREADFACTOR; a++) { Complex cangle(cos(M_PI*2*a/SPREADFACTOR),-sin(M_PI*2*a/SPREADFACTOR)); const float v[2] = { cangle.real(), cangle.imag() }; std::fwrite(v, 4, 2, out); }
            for (int m = 0; m < LORA_SFFT_LEN; m++) {
                Complex nangle(cos(M_PI*2*m/LORA_SFFT_LEN),sin(M_PI*2*m/LORA_SFFT_LEN));
                Sample s(nangle.real() * 100, nangle.imag() * 100);
                const int16_t v[2] = { s.real(), s.imag() };
                std::fwrite(v, 2, 2, out);
            }
        }
    }
    delete d;
    std::fclose(out);
    if (tr) std::fclose(tr);
    return 0;
}
