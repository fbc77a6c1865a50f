// Recorder around the reference's own NCO, fftfilt (g_fft), PhaseDiscriminators and Interpolator, compiled where they lie
// by tests/golden/make_golden_wfm.py (strict IEEE, scalar: -O2 -fno-fast-math -ffp-contract=off, USE_SSE2 undefined).
// WFMDemod itself cannot be instantiated outside the application (it attaches to a DeviceSourceAPI, the audio device
// manager and a threaded channelizer), so the per-sample loop of WFMDemod::feed and the derivations of
// applyChannelSettings / applySettings are written here around the real members.  m_prevArg of PhaseDiscriminators has
// no initialiser in the reference; value-initialisation pins it to 0.  m_movingAverage (GUI only) is left out.
//
//   wfm_rec <input.bin> <output.bin>     commands on stdin, one per line:
//     new in_rate nco_freq audio_rate rf_bw af_bw volume squelch_db mute    a fresh demodulator
//     feed n                               the next n Samples of input.bin (int16 I, Q)
//     end                                  level accumulators and squelch state
//   output.bin: per feed an int64 count and the qint16 audio; per end: double sum, double peak, int64 count, int64 open, int64 state
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "dsp/dsptypes.h"
#include "dsp/nco.h"
#include "dsp/fftfilt.h"
#include "dsp/phasediscri.h"
#include "dsp/interpolator.h"

namespace {

struct Demod {
    NCO nco;
    fftfilt* rfFilter;
    PhaseDiscriminators discri;
    Interpolator interp;
    Real distance, distanceRemain, squelchLevel, rfBandwidth, volume;
    bool mute, squelchOpen;
    int squelchState, magsqCount;
    double magsqSum, magsqPeak;

    Demod(int inRate, int ncoFreq, int audioRate, Real rfBw, Real afBw, Real vol, Real squelchDb, bool muted) :
        rfFilter(new fftfilt(-50000.0 / 384000.0, 50000.0 / 384000.0, 1024)), discri(),
        rfBandwidth(rfBw), volume(vol), mute(muted), squelchOpen(false), squelchState(0), magsqCount(0), magsqSum(0.0), magsqPeak(0.0)
    {
        nco.setFreq(ncoFreq, inRate);
        interp.create(16, inRate, afBw);
        distanceRemain = (Real) inRate / (Real) audioRate;
        distance = (Real) inRate / (Real) audioRate;
        Real lowCut = -(rfBw / 2.0) / inRate;
        Real hiCut = (rfBw / 2.0) / inRate;
        rfFilter->create_filter(lowCut, hiCut);
        Real excursion = rfBw / (Real) inRate;
        discri.setFMScaling(1.0f / excursion);
        squelchLevel = pow(10.0, squelchDb / 10.0);
    }
    ~Demod() { delete rfFilter; }

    void feed(const std::vector<Sample>& in, std::vector<qint16>& audio)
    {
        for (std::vector<Sample>::const_iterator it = in.begin(); it != in.end(); ++it) {
            Complex c(it->real(), it->imag());
            c *= nco.nextIQ();
            fftfilt::cmplx* rf;
            const int rfOut = rfFilter->runFilt(c, &rf);
            for (int i = 0; i < rfOut; i++) {
                double msq = rf[i].real() * rf[i].real() + rf[i].imag() * rf[i].imag();
                Real magsq = msq / (SDR_RX_SCALED * SDR_RX_SCALED);
                magsqSum += magsq;
                if (magsq > magsqPeak) magsqPeak = magsq;
                magsqCount++;
                if (magsq >= squelchLevel) {
                    if (squelchState < rfBandwidth / 10) squelchState++;
                } else if (squelchState > 0) {
                    squelchState--;
                }
                squelchOpen = squelchState > (rfBandwidth / 20);
                Real demod = 0;
                Real fmDev;
                if (squelchOpen && !mute) demod = discri.phaseDiscriminatorDelta(rf[i], msq, fmDev);
                Complex e(demod, 0), ci;
                if (interp.decimate(&distanceRemain, e, &ci)) {
                    audio.push_back((qint16)(ci.real() * 3276.8f * volume));
                    distanceRemain += distance;
                }
            }
        }
    }
};

} // namespace

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: wfm_rec input.bin output.bin\n"); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::perror("open"); return 2; }
    Demod* d = 0;
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        char cmd[16] = "";
        if (std::sscanf(line, "%15s", cmd) != 1) continue;
        if (!std::strcmp(cmd, "new")) {
            int inRate, ncoFreq, audioRate, mute; float rf, af, vol, sq;
            if (std::sscanf(line, "%*s %d %d %d %f %f %f %f %d", &inRate, &ncoFreq, &audioRate, &rf, &af, &vol, &sq, &mute) != 8) return 3;
            delete d;
            d = new Demod(inRate, ncoFreq, audioRate, rf, af, vol, sq, mute != 0);
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
            const int64_t tail[3] = { d->magsqCount, d->squelchOpen ? 1 : 0, d->squelchState };
            std::fwrite(&d->magsqSum, 8, 1, out); std::fwrite(&d->magsqPeak, 8, 1, out); std::fwrite(tail, 8, 3, out);
        }
    }
    delete d;
    std::fclose(out);
    return 0;
}
