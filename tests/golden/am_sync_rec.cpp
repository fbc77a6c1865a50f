// Recorder around the reference's own NCO, Interpolator, Lowpass, PhaseLockComplex, fftfilt, MagAGC, Bandpass, MovingAverageUtil,
// DoubleBufferFIFO and StepFunctions, compiled where they lie by tests/golden/make_golden_am_sync.py (strict IEEE, scalar: -O2
// -fno-fast-math -ffp-contract=off, USE_SSE2 undefined).  AMDemod itself cannot be instantiated outside the application (see
// am_rec.cpp), so the loop of AMDemod::feed / processOneSample in its m_pll form and the derivations of the constructor,
// applyChannelSettings / applyAudioSampleRate / applySettings are written here around the real members, in the state start()
// leaves them in.  Two things the reference leaves open are pinned: the delay line starts at zeros (as am_rec.cpp), and
// m_syncAMBuff, which AMDemod never initialises, starts at 0.0f.  SSBFilter is built once from the two construction-time values
// (ssb_rate, ssb_bw) and never redesigned; DSBFilter follows rf_bw and audio_rate, as in the reference.
//
//   am_sync_rec <input.bin> <output.bin> [trace.bin]     commands on stdin, one per line:
//     new in_rate nco_freq audio_rate rf_bw volume squelch_db mute bandpass sync_op ssb_rate ssb_bw [pll]    a fresh demodulator; pll 0 (the
//                                          default is 1) takes the envelope branch with m_volumeAGC, as am_rec.cpp
//     feed n                               the next n Samples of input.bin (int16 I, Q)
//     end                                  level accumulators, squelch and loop state
//     design                               the design products
//   output.bin: per feed an int64 count, the qint16 audio and an int64, the open samples so far; per end: double magsq, sum, peak, int64 count, open, squelch count,
//     locked, the bits of getFreq(), open samples so far, reopenings so far, out-of-range or non-finite samples so far, open samples before the first reopening; double
//     largest |sample| before the conversion; per design: 51 taps, int64 flen, flen complex bins, a1 a2 b0 b1 b2
//   trace.bin (optional), per open sample: re, im, the filtered pair, m_yRe, m_yIm, demod (before the Bandpass): 7 floats; then per
//     filter output as they come, appended to a second file trace.bin.sb: the sideband pair
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "dsp/dsptypes.h"
#include "dsp/nco.h"
#include "dsp/interpolator.h"
#include "dsp/agc.h"
#include "dsp/bandpass.h"
#define private public
#define protected public
#include "dsp/lowpass.h"
#include "dsp/phaselockcomplex.h"
#include "dsp/fftfilt.h"
#undef protected
#undef private
#include "util/movingaverage.h"
#include "util/doublebufferfifo.h"
#include "util/stepfunctions.h"

namespace {

struct Demod {
    NCO nco;
    Interpolator interp;
    Real distance, distanceRemain, squelchLevel, volume;
    uint32_t audioRate, squelchCount;
    bool mute, bandpassEnable, squelchOpen;
    int syncOp;                                             // 0 DSB, 1 USB, 2 LSB
    DoubleBufferFIFO<Real> delayLine;
    MovingAverageUtil<Real, double, 16> movingAverage;
    MagAGC syncAMAGC;
    SimpleAGC<4800> volumeAGC;
    bool usePll;
    Bandpass<Real> bandpass;
    Lowpass<std::complex<float> > pllFilt;
    PhaseLockComplex pll;
    fftfilt* DSBFilter;
    fftfilt* SSBFilter;
    Real syncAMBuff[2 * 1024];
    uint32_t syncAMBuffIndex;
    double magsq, magsqSum, magsqPeak;
    int magsqCount;
    int64_t opens, reopenings, opensAtReopen, bad;
    double largest;
    bool everOpen, wasOpen;
    FILE* trace;
    FILE* traceSb;

    Demod(int inRate, int ncoFreq, int audioRateArg, Real rfBw, Real vol, Real squelchDb, bool muted, bool bp, int op, int ssbRate, Real ssbBw,
          bool pllOn, FILE* tr, FILE* trSb) :
        volume(vol), audioRate(audioRateArg), squelchCount(0), mute(muted), bandpassEnable(bp), squelchOpen(false), syncOp(op),
        delayLine(9600), syncAMAGC(12000, 0.1, 1e-2), volumeAGC(0.003), usePll(pllOn), magsq(0.0), magsqSum(0.0), magsqPeak(0.0), magsqCount(0),
        opens(0), reopenings(0), opensAtReopen(-1), bad(0), largest(0.0), everOpen(false), wasOpen(false), trace(tr), traceSb(trSb)
    {
        // the constructor, at the audio rate and bandwidth of that moment
        uint32_t ctorRate = ssbRate;
        DSBFilter = new fftfilt((2.0f * ssbBw) / ctorRate, 2 * 1024);
        SSBFilter = new fftfilt(0.0f, ssbBw / ctorRate, 1024);
        syncAMAGC.setThresholdEnable(false);
        syncAMAGC.resize(12000, 6000, 0.1);
        pllFilt.create(101, ctorRate, 200.0);
        pll.computeCoefficients(0.05, 0.707, 1000);
        syncAMBuffIndex = 0;
        for (int i = 0; i < 2 * 1024; i++) syncAMBuff[i] = 0.0f;
        // applySettings, applyAudioSampleRate, applyChannelSettings
        nco.setFreq(ncoFreq, inRate);
        interp.create(16, inRate, rfBw / 2.2f);
        distanceRemain = 0;
        distance = (Real) inRate / (Real) audioRate;
        bandpass.create(301, audioRate, 300.0, rfBw / 2.0f);
        delayLine.resize(audioRate / 5);
        for (uint32_t i = 0; i < audioRate / 5; i++) delayLine.write(0);
        DSBFilter->create_dsb_filter((2.0f * rfBw) / (float) audioRate);
        pllFilt.create(101, audioRate, 200.0);
        syncAMAGC.resize(audioRate / 4, audioRate / 8, 0.1);
        volumeAGC.resizeNew(audioRate / 10, 0.003);
        pll.setSampleRate(audioRate);
        squelchLevel = pow(10.0, squelchDb / 10.0);
    }
    ~Demod() { delete DSBFilter; delete SSBFilter; }

    qint16 one(Complex& ci)
    {
        Real re = ci.real() / SDR_RX_SCALEF;
        Real im = ci.imag() / SDR_RX_SCALEF;
        Real msq = re * re + im * im;
        movingAverage(msq);
        magsq = movingAverage.asDouble();
        magsqSum += msq;
        if (msq > magsqPeak) magsqPeak = msq;
        magsqCount++;
        delayLine.write(msq);
        if (magsq < squelchLevel) { if (squelchCount > 0) squelchCount--; }
        else { if (squelchCount < audioRate / 10) squelchCount++; }
        qint16 sample;
        squelchOpen = (squelchCount >= audioRate / 20);
        if (squelchOpen && !wasOpen) { if (everOpen) { reopenings++; if (opensAtReopen < 0) opensAtReopen = opens; } everOpen = true; }
        wasOpen = squelchOpen;
        if (squelchOpen && !mute) {
            Real demod;
            if (!usePll) {
                demod = sqrt(delayLine.readBack(audioRate / 20));
                volumeAGC.feed(demod);
                demod = (demod - volumeAGC.getValue()) / volumeAGC.getValue();
            } else {
            std::complex<float> s(re, im);
            s = pllFilt.filter(s);
            pll.feed(s.real(), s.imag());
            float yr = re * pll.getImag() - im * pll.getReal();
            float yi = re * pll.getReal() + im * pll.getImag();
            fftfilt::cmplx *sideband;
            std::complex<float> cs(yr, yi);
            int n_out;
            if (syncOp == 0) {
                n_out = DSBFilter->runDSB(cs, &sideband, false);
            } else {
                n_out = SSBFilter->runSSB(cs, &sideband, syncOp == 1, false);
            }
            for (int i = 0; i < n_out; i++) {
                float agcVal = syncAMAGC.feedAndGetValue(sideband[i]);
                fftfilt::cmplx z = sideband[i] * agcVal;
                syncAMBuff[i] = (z.real() + z.imag());
                syncAMBuffIndex = 0;
                if (traceSb) { const float t[2] = { sideband[i].real(), sideband[i].imag() }; std::fwrite(t, 4, 2, traceSb); }
            }
            syncAMBuffIndex = syncAMBuffIndex < 2 * 1024 ? syncAMBuffIndex : 0;
            demod = syncAMBuff[syncAMBuffIndex++] * 4.0f;
            if (trace) { const float t[7] = { re, im, s.real(), s.imag(), pll.getReal(), pll.getImag(), demod }; std::fwrite(t, 4, 7, trace); }
            opens++;
            }
            if (bandpassEnable) { demod = bandpass.filter(demod); demod /= 301.0f; }
            Real attack = (squelchCount - 0.05f * audioRate) / (0.05f * audioRate);
            Real v = demod * StepFunctions::smootherstep(attack) * (audioRate / 24) * volume;
            if (!(std::fabs(v) < 32767.0f)) bad++;         // the conversion of such a value is undefined
            else if (std::fabs(v) > largest) largest = std::fabs(v);
            sample = v;
        } else {
            sample = 0;
        }
        return sample;
    }

    void feed(const std::vector<Sample>& in, std::vector<qint16>& audio)
    {
        Complex ci;
        for (std::vector<Sample>::const_iterator it = in.begin(); it != in.end(); ++it) {
            Complex c(it->real(), it->imag());
            c *= nco.nextIQ();
            if (interp.decimate(&distanceRemain, c, &ci)) {
                audio.push_back(one(ci));
                distanceRemain += distance;
            }
        }
    }
};

} // namespace

int main(int argc, char** argv)
{
    if (argc != 3 && argc != 4) { std::fprintf(stderr, "usage: am_sync_rec input.bin output.bin [trace.bin]\n"); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    FILE* tr = 0;
    FILE* trSb = 0;
    if (argc == 4) {
        char name[1024];
        std::snprintf(name, sizeof name, "%s.sb", argv[3]);
        tr = std::fopen(argv[3], "wb"); trSb = std::fopen(name, "wb");
        if (!tr || !trSb) { std::perror("open"); return 2; }
    }
    if (!in || !out) { std::perror("open"); return 2; }
    Demod* d = 0;
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        char cmd[16] = "";
        if (std::sscanf(line, "%15s", cmd) != 1) continue;
        if (!std::strcmp(cmd, "new")) {
            int inRate, ncoFreq, audioRate, mute, bp, op, ssbRate, pllOn = 1; float rf, vol, sq, ssbBw;
            if (std::sscanf(line, "%*s %d %d %d %f %f %f %d %d %d %d %f %d", &inRate, &ncoFreq, &audioRate, &rf, &vol, &sq, &mute, &bp, &op, &ssbRate, &ssbBw, &pllOn) < 11) return 3;
            delete d;
            d = new Demod(inRate, ncoFreq, audioRate, rf, vol, sq, mute != 0, bp != 0, op, ssbRate, ssbBw, pllOn != 0, tr, trSb);
        } else if (!std::strcmp(cmd, "feed") && d) {
            long n;
            if (std::sscanf(line, "%*s %ld", &n) != 1) return 3;
            std::vector<Sample> s((size_t)n);
            for (long i = 0; i < n; i++) {
                int16_t iq[2];
                if (std::fread(iq, 2, 2, in) != 2) return 4;
                s[(size_t)i] = Sample(iq[0], iq[1]);
            }
            std::vector<qint16> audio;
            d->feed(s, audio);
            const int64_t k = (int64_t)audio.size();
            std::fwrite(&k, 8, 1, out);
            if (k) std::fwrite(audio.data(), 2, audio.size(), out);
            std::fwrite(&d->opens, 8, 1, out);
        } else if (!std::strcmp(cmd, "end") && d) {
            const float freq = d->pll.getFreq();
            uint32_t fbits; std::memcpy(&fbits, &freq, 4);
            const int64_t tail[9] = { d->magsqCount, d->squelchOpen ? 1 : 0, (int64_t)d->squelchCount, d->pll.locked() ? 1 : 0, (int64_t)fbits,
                                      d->opens, d->reopenings, d->bad, d->opensAtReopen };
            std::fwrite(&d->magsq, 8, 1, out); std::fwrite(&d->magsqSum, 8, 1, out); std::fwrite(&d->magsqPeak, 8, 1, out); std::fwrite(tail, 8, 9, out);
            std::fwrite(&d->largest, 8, 1, out);
        } else if (!std::strcmp(cmd, "design") && d) {
            fftfilt* f = d->syncOp == 0 ? d->DSBFilter : d->SSBFilter;
            const int64_t flen = f->flen;
            std::fwrite(d->pllFilt.m_taps.data(), 4, 51, out);
            std::fwrite(&flen, 8, 1, out);
            std::fwrite(f->filter, 8, (size_t)flen, out);
            const float k[5] = { d->pll.m_a1, d->pll.m_a2, d->pll.m_b0, d->pll.m_b1, d->pll.m_b2 };
            std::fwrite(k, 4, 5, out);
        }
    }
    delete d;
    std::fclose(out);
    if (tr) std::fclose(tr);
    if (trSb) std::fclose(trSb);
    return 0;
}
