// Recorder around the reference's own NCO, Interpolator, PhaseDiscriminators, MovingAverageUtil, DoubleBufferFIFO and
// Bandpass, compiled where they lie by tests/golden/make_golden_nfm.py (strict IEEE, scalar: -O2 -fno-fast-math
// -ffp-contract=off, USE_SSE2 undefined).  NFMDemod itself cannot be instantiated outside the application (it attaches to a
// DeviceSourceAPI, the audio device manager and a threaded channelizer), so the loop of NFMDemod::feed with m_deltaSquelch
// and m_ctcssOn off and the derivations of the constructor, applySettings(settings, true) and start() are written here
// around the real members.  Two members have no defined starting value in the reference and are pinned through their own
// interfaces: PhaseDiscriminators::m_prevArg by one phaseDiscriminatorDelta of (1, 0), whose argument is 0, and the delay
// line's array by `size` writes of 0, which leave the indices as on a fresh object.
//
//   nfm_rec <input.bin> <output.bin>     commands on stdin, one per line:
//     new in_rate nco_freq audio_rate rf_bw af_bw fm_deviation volume squelch squelch_gate mute     a fresh demodulator
//     feed n                               the next n Samples of input.bin (int16 I, Q)
//     end                                  level accumulators and squelch state
//   output.bin: per feed an int64 count and the qint16 audio; per end: double moving average, sum, peak, int64 count, open,
//   squelch count
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "dsp/dsptypes.h"
#include "dsp/nco.h"
#include "dsp/interpolator.h"
#include "dsp/phasediscri.h"
#include "dsp/bandpass.h"
#include "util/movingaverage.h"
#include "util/doublebufferfifo.h"

namespace {

struct Demod {
    NCO nco;
    Interpolator interp;
    Real distance, distanceRemain, squelchLevel, volume, discriCompensation;
    int audioRate, squelchCount, squelchGate;
    bool mute, squelchOpen;
    PhaseDiscriminators phaseDiscri;
    MovingAverageUtil<Real, double, 32> movingAverage;
    DoubleBufferFIFO<Real> delayLine;
    Bandpass<Real> bandpass;
    double magsqSum, magsqPeak;
    int magsqCount;

    Demod(int inRate, int ncoFreq, int audioRateArg, Real rfBw, Real afBw, int fmDeviation, Real vol, Real squelch, int gate, bool muted) :
        volume(vol), audioRate(audioRateArg), squelchCount(0), mute(muted), squelchOpen(false),
        delayLine(24000), magsqSum(0.0), magsqPeak(0.0), magsqCount(0)
    {
        discriCompensation = (audioRate / 48000.0f);
        discriCompensation *= std::sqrt(discriCompensation);          // the Real overload, as sdrx_audiotail_* rules it (include/sdrx.h)
        nco.setFreq(ncoFreq, inRate);
        interp.create(16, inRate, rfBw / 2.2f);
        distanceRemain = 0;
        distance = (Real) inRate / (Real) audioRate;
        phaseDiscri.setFMScaling((8.0f * audioRate) / static_cast<float>(fmDeviation));
        bandpass.create(301, audioRate, 300.0, afBw);
        squelchGate = (audioRate / 100) * gate;
        squelchLevel = std::pow(10.0, squelch / 100.0);
        double m; Real dev;
        phaseDiscri.phaseDiscriminatorDelta(Complex(1.0f, 0.0f), m, dev);
        for (int i = 0; i < 24000; i++) delayLine.write(0);
    }

    qint16 one(Complex& ci)
    {
        qint16 sample;
        double magsqRaw;
        Real deviation;
        Real demod = phaseDiscri.phaseDiscriminatorDelta(ci, magsqRaw, deviation);
        Real magsq = magsqRaw / (SDR_RX_SCALED*SDR_RX_SCALED);
        movingAverage(magsq);
        magsqSum += magsq;
        if (magsq > magsqPeak) magsqPeak = magsq;
        magsqCount++;
        if ((Real) movingAverage < squelchLevel) {
            delayLine.write(0);
            if (squelchCount > 0) squelchCount--;
        } else {
            delayLine.write(demod * discriCompensation);
            if (squelchCount < 2*squelchGate) squelchCount++;
        }
        squelchOpen = (squelchCount > squelchGate);
        if (mute) sample = 0;
        else if (squelchOpen) sample = bandpass.filter(delayLine.readBack(squelchGate)) * volume;
        else sample = 0;
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
    if (argc != 3) { std::fprintf(stderr, "usage: nfm_rec input.bin output.bin\n"); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::perror("open"); return 2; }
    Demod* d = 0;
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        char cmd[16] = "";
        if (std::sscanf(line, "%15s", cmd) != 1) continue;
        if (!std::strcmp(cmd, "new")) {
            int inRate, ncoFreq, audioRate, fmDev, gate, mute; float rf, af, vol, sq;
            if (std::sscanf(line, "%*s %d %d %d %f %f %d %f %f %d %d", &inRate, &ncoFreq, &audioRate, &rf, &af, &fmDev, &vol, &sq, &gate, &mute) != 10) return 3;
            delete d;
            d = new Demod(inRate, ncoFreq, audioRate, rf, af, fmDev, vol, sq, gate, mute != 0);
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
            const double avg = d->movingAverage.asDouble();
            const int64_t tail[3] = { d->magsqCount, d->squelchOpen ? 1 : 0, (int64_t)d->squelchCount };
            std::fwrite(&avg, 8, 1, out); std::fwrite(&d->magsqSum, 8, 1, out); std::fwrite(&d->magsqPeak, 8, 1, out); std::fwrite(tail, 8, 3, out);
        }
    }
    delete d;
    std::fclose(out);
    return 0;
}
