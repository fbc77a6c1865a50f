// Recorder around the reference's own NCO, Interpolator, MovingAverageUtil, DoubleBufferFIFO, SimpleAGC, Bandpass and
// StepFunctions, compiled where they lie by tests/golden/make_golden_am.py (strict IEEE, scalar: -O2 -fno-fast-math
// -ffp-contract=off, USE_SSE2 undefined).  AMDemod itself cannot be instantiated outside the application (it attaches to a
// DeviceSourceAPI, the audio device manager and a threaded channelizer), so the loop of AMDemod::feed / processOneSample in
// envelope mode (m_pll = false) and the derivations of applyChannelSettings / applyAudioSampleRate / applySettings are
// written here around the real members, in the state start() leaves them in.  DoubleBufferFIFO does not clear its array:
// before the first sample the delay line is filled with `size` zeros through its own write(), which leaves the indices as
// on a fresh object (size writes wrap m_writeIndex back to 0) and pins what the never-written slots hold.
//
//   am_rec <input.bin> <output.bin>     commands on stdin, one per line:
//     new in_rate nco_freq audio_rate rf_bw volume squelch_db mute bandpass    a fresh demodulator
//     feed n                               the next n Samples of input.bin (int16 I, Q)
//     end                                  level accumulators and squelch state
//   output.bin: per feed an int64 count and the qint16 audio; per end: double magsq, sum, peak, int64 count, open, squelch count
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
    DoubleBufferFIFO<Real> delayLine;
    MovingAverageUtil<Real, double, 16> movingAverage;
    SimpleAGC<4800> volumeAGC;
    Bandpass<Real> bandpass;
    double magsq, magsqSum, magsqPeak;
    int magsqCount;

    Demod(int inRate, int ncoFreq, int audioRateArg, Real rfBw, Real vol, Real squelchDb, bool muted, bool bp) :
        volume(vol), audioRate(audioRateArg), squelchCount(0), mute(muted), bandpassEnable(bp), squelchOpen(false),
        delayLine(9600), volumeAGC(0.003), magsq(0.0), magsqSum(0.0), magsqPeak(0.0), magsqCount(0)
    {
        nco.setFreq(ncoFreq, inRate);
        interp.create(16, inRate, rfBw / 2.2f);
        distanceRemain = 0;
        distance = (Real) inRate / (Real) audioRate;
        bandpass.create(301, audioRate, 300.0, rfBw / 2.0f);
        delayLine.resize(audioRate / 5);
        for (uint32_t i = 0; i < audioRate / 5; i++) delayLine.write(0);
        volumeAGC.resizeNew(audioRate / 10, 0.003);
        squelchLevel = pow(10.0, squelchDb / 10.0);
    }

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
        if (squelchOpen && !mute) {
            Real demod = sqrt(delayLine.readBack(audioRate / 20));
            volumeAGC.feed(demod);
            demod = (demod - volumeAGC.getValue()) / volumeAGC.getValue();
            if (bandpassEnable) { demod = bandpass.filter(demod); demod /= 301.0f; }
            Real attack = (squelchCount - 0.05f * audioRate) / (0.05f * audioRate);
            sample = demod * StepFunctions::smootherstep(attack) * (audioRate / 24) * volume;
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
    if (argc != 3) { std::fprintf(stderr, "usage: am_rec input.bin output.bin\n"); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::perror("open"); return 2; }
    Demod* d = 0;
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        char cmd[16] = "";
        if (std::sscanf(line, "%15s", cmd) != 1) continue;
        if (!std::strcmp(cmd, "new")) {
            int inRate, ncoFreq, audioRate, mute, bp; float rf, vol, sq;
            if (std::sscanf(line, "%*s %d %d %d %f %f %f %d %d", &inRate, &ncoFreq, &audioRate, &rf, &vol, &sq, &mute, &bp) != 8) return 3;
            delete d;
            d = new Demod(inRate, ncoFreq, audioRate, rf, vol, sq, mute != 0, bp != 0);
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
        } else if (!std::strcmp(cmd, "end") && d) {
            const int64_t tail[3] = { d->magsqCount, d->squelchOpen ? 1 : 0, (int64_t)d->squelchCount };
            std::fwrite(&d->magsq, 8, 1, out); std::fwrite(&d->magsqSum, 8, 1, out); std::fwrite(&d->magsqPeak, 8, 1, out); std::fwrite(tail, 8, 3, out);
        }
    }
    delete d;
    std::fclose(out);
    return 0;
}
