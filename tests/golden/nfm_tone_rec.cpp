// Recorder around the reference's own NCO, Interpolator, PhaseDiscriminators, MovingAverageUtil, DoubleBufferFIFO, Bandpass,
// Lowpass and CTCSSDetector, compiled where they lie by tests/golden/make_golden_nfm_tone.py (strict IEEE, scalar: -O2
// -fno-fast-math -ffp-contract=off, USE_SSE2 undefined): tests/golden/nfm_rec.cpp with the m_ctcssOn branch.  NFMDemod itself
// cannot be instantiated outside the application (it attaches to a DeviceSourceAPI, the audio device manager and a threaded
// channelizer), so the loop of NFMDemod::feed with m_deltaSquelch off and the derivations of the constructor,
// applySettings(settings, true) and start() are written here around the real members.  Two members have no defined starting
// value in the reference and are pinned through their own interfaces: PhaseDiscriminators::m_prevArg by one
// phaseDiscriminatorDelta of (1, 0), whose argument is 0, and the delay line's array by `size` writes of 0, which leave the
// indices as on a fresh object.  The detector's u0, u1 and power come from new Real[] and NFMDemod never resets them: pinned
// by CTCSSDetector::reset() right after setCoefficients.  Its power array and coefficients are private and have no getter:
// the header is included with `private` opened, which changes no layout.
//
//   nfm_tone_rec <input.bin> <output.bin>     commands on stdin, one per line:
//     new in_rate nco_freq audio_rate rf_bw af_bw fm_deviation volume squelch squelch_gate mute ctcss_on ctcss_index delta_squelch
//     feed n                               the next n Samples of input.bin (int16 I, Q)
//     end                                  level accumulators and squelch state
//   output.bin: per feed an int64 count, the qint16 audio, an int64 count of index changes and per change two int64 (audio
//   sample position in the feed, new m_ctcssIndex); per end: double moving average, sum, peak, int64 count, open, squelch
//   count, m_ctcssIndex, changes, completed blocks, toneDetected, maxPowerIndex, then float power[32], coef[32], int32 N, rate,
//   then ten doubles of the AFSquelch: N, tones[2], coef[2], threshold, 1000 * isOpen + squelchCount, m_afSquelchOpen, sums[2]
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
#include "dsp/lowpass.h"
#define private public
#include "dsp/ctcssdetector.h"
#include "dsp/afsquelch.h"
#undef private
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
    bool ctcssOn, deltaSquelch, afSquelchOpen;
    int ctcssIndex, ctcssIndexSelected, sampleCount;
    Lowpass<Real> lowpass;
    CTCSSDetector ctcssDetector;
    AFSquelch afSquelch;
    Real squelchLevelDelta;
    int64_t changes, blocks;
    std::vector<int64_t> events;

    Demod(int inRate, int ncoFreq, int audioRateArg, Real rfBw, Real afBw, int fmDeviation, Real vol, Real squelch, int gate, bool muted,
          bool ctcss, int selected, bool delta) :
        volume(vol), audioRate(audioRateArg), squelchCount(0), mute(muted), squelchOpen(false),
        delayLine(24000), magsqSum(0.0), magsqPeak(0.0), magsqCount(0),
        ctcssOn(ctcss), deltaSquelch(delta), afSquelchOpen(false), ctcssIndex(0), ctcssIndexSelected(selected), sampleCount(0), changes(0), blocks(0)
    {
        uint32_t audioSampleRate = audioRate;
        ctcssDetector.setCoefficients(audioSampleRate/16, audioSampleRate/8.0f);
        ctcssDetector.reset();
        const double afSqTones[2] = {1000.0, 6000.0};
        afSquelch.setCoefficients(audioSampleRate/2000, 600, audioSampleRate, 200, 0, afSqTones);
        if (deltaSquelch) {                                 // applySettings
            squelchLevelDelta = (- squelch) / 1000.0;
            afSquelch.setThreshold(squelchLevelDelta);
            afSquelch.reset();
        }
        lowpass.create(301, audioSampleRate, 250.0);
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

    void setIndex(int v, int64_t pos)
    {
        ctcssIndex = v; changes++;
        events.push_back(pos); events.push_back(v);
    }

    qint16 one(Complex& ci, int64_t pos)
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
        sampleCount++;
        if (deltaSquelch) {
            if (afSquelch.analyze(demod * discriCompensation)) {
                afSquelchOpen = afSquelch.evaluate();
                if (!afSquelchOpen) delayLine.zeroBack(((uint32_t) audioRate)/10);
            }
            if (afSquelchOpen) {
                delayLine.write(demod * discriCompensation);
                if (squelchCount < 2*squelchGate) squelchCount++;
            } else {
                delayLine.write(0);
                if (squelchCount > 0) squelchCount--;
            }
        } else if ((Real) movingAverage < squelchLevel) {
            delayLine.write(0);
            if (squelchCount > 0) squelchCount--;
        } else {
            delayLine.write(demod * discriCompensation);
            if (squelchCount < 2*squelchGate) squelchCount++;
        }
        squelchOpen = (squelchCount > squelchGate);
        if (mute) sample = 0;
        else if (squelchOpen) {
            if (ctcssOn) {
                Real ctcss_sample = lowpass.filter(demod * discriCompensation);
                if ((sampleCount & 7) == 7) {
                    if (ctcssDetector.analyze(&ctcss_sample)) {
                        blocks++;
                        int maxToneIndex;
                        if (ctcssDetector.getDetectedTone(maxToneIndex)) {
                            if (maxToneIndex+1 != ctcssIndex) setIndex(maxToneIndex+1, pos);
                        } else {
                            if (ctcssIndex != 0) setIndex(0, pos);
                        }
                    }
                }
            }
            if (ctcssOn && ctcssIndexSelected && (ctcssIndexSelected != ctcssIndex)) sample = 0;
            else sample = bandpass.filter(delayLine.readBack(squelchGate)) * volume;
        } else {
            if (ctcssIndex != 0) setIndex(0, pos);
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
                audio.push_back(one(ci, (int64_t)audio.size()));
                distanceRemain += distance;
            }
        }
    }
};

} // namespace

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: nfm_tone_rec input.bin output.bin\n"); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::perror("open"); return 2; }
    Demod* d = 0;
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        char cmd[16] = "";
        if (std::sscanf(line, "%15s", cmd) != 1) continue;
        if (!std::strcmp(cmd, "new")) {
            int inRate, ncoFreq, audioRate, fmDev, gate, mute, ctcss, selected, delta; float rf, af, vol, sq;
            if (std::sscanf(line, "%*s %d %d %d %f %f %d %f %f %d %d %d %d %d", &inRate, &ncoFreq, &audioRate, &rf, &af, &fmDev, &vol, &sq, &gate, &mute,
                            &ctcss, &selected, &delta) != 13) return 3;
            delete d;
            d = new Demod(inRate, ncoFreq, audioRate, rf, af, fmDev, vol, sq, gate, mute != 0, ctcss != 0, selected, delta != 0);
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
            d->events.clear();
            d->feed(s, audio);
            const int64_t k = (int64_t)audio.size();
            std::fwrite(&k, 8, 1, out);
            if (k) std::fwrite(audio.data(), 2, audio.size(), out);
            const int64_t ne = (int64_t)d->events.size() / 2;
            std::fwrite(&ne, 8, 1, out);
            if (ne) std::fwrite(d->events.data(), 8, d->events.size(), out);
        } else if (!std::strcmp(cmd, "end") && d) {
            const double avg = d->movingAverage.asDouble();
            const int64_t tail[3] = { d->magsqCount, d->squelchOpen ? 1 : 0, (int64_t)d->squelchCount };
            std::fwrite(&avg, 8, 1, out); std::fwrite(&d->magsqSum, 8, 1, out); std::fwrite(&d->magsqPeak, 8, 1, out); std::fwrite(tail, 8, 3, out);
            int maxTone;
            const bool det = d->ctcssDetector.getDetectedTone(maxTone);
            const int64_t tone[5] = { d->ctcssIndex, d->changes, d->blocks, det ? 1 : 0, maxTone };
            const int32_t nr[2] = { d->ctcssDetector.N, d->ctcssDetector.sampleRate };
            std::fwrite(tone, 8, 5, out);
            std::fwrite(d->ctcssDetector.power, 4, 32, out); std::fwrite(d->ctcssDetector.coef, 4, 32, out); std::fwrite(nr, 4, 2, out);
            const double af[10] = { (double)d->afSquelch.m_N, d->afSquelch.m_toneSet[0], d->afSquelch.m_toneSet[1], d->afSquelch.m_coef[0],
                                    d->afSquelch.m_coef[1], d->afSquelch.m_threshold, (double)((d->afSquelch.m_isOpen ? 1000 : 0) + (int)d->afSquelch.m_squelchCount),
                                    d->afSquelchOpen ? 1.0 : 0.0, d->afSquelch.m_movingAverages[0].sum(), d->afSquelch.m_movingAverages[1].sum() };
            std::fwrite(af, 8, 10, out);
        }
    }
    delete d;
    std::fclose(out);
    return 0;
}
