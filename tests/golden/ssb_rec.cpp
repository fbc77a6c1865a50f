// Recorder around the reference's own NCO, Interpolator, fftfilt, MagAGC, DoubleBufferFIFO and StepFunctions, compiled where
// they lie by tests/golden/make_golden_ssb.py (strict IEEE, scalar: -O2 -fno-fast-math -ffp-contract=off, USE_SSE2
// undefined).  SSBDemod itself cannot be instantiated outside the application (it attaches to a DeviceSourceAPI, the audio
// device manager and a threaded channelizer), so the loop of SSBDemod::feed and the derivations of the constructor,
// applyAudioSampleRate and applySettings(settings, true) are written here around the real members, in the order the
// application reaches them: MagAGC(12000, agcTarget, 1e-2), setClampMax, setClamping, then setThresholdEnable, resize +
// setStepDownDelay (hn != 12000), setThreshold, setGate, setClamping.  One member has no defined starting value in the
// reference and is pinned through its own interface: the delay line's array by `size` writes of 0, which leave the indices
// as on a fresh object.
//
//   ssb_rec <input.bin> <output.bin>     commands on stdin, one per line:
//     new in_rate nco_freq audio_rate rf_bw low_cutoff volume span_log2 binaural flip dsb mute agc clamping time_log2 thr_db gate_ms
//     feed n                               the next n Samples of input.bin (int16 I, Q)
//     end                                  level accumulators and final state
//   output.bin: per feed an int64 audio count, the AudioSamples (l, r), an int64 Sample count, the Samples (re, im); per end:
//   double m_magsq, sum, peak, then int64 count, m_audioActive, m_undersampleCount, then double getValue() as m_u0's Real,
//   getStepValue(), getStepDownValue()
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "dsp/dsptypes.h"
#include "dsp/nco.h"
#include "dsp/interpolator.h"
#include "dsp/fftfilt.h"
#include "dsp/agc.h"
#include "util/doublebufferfifo.h"
#include "util/db.h"

namespace {

const double kAgcTarget = 3276.8;

struct Demod {
    NCO nco;
    Interpolator interp;
    Real distance, distanceRemain, bandwidth, lowCutoff, volume;
    int audioRate, spanLog2, undersampleCount, magsqCount;
    bool usb, binaural, flip, dsb, mute, agcActive, audioActive;
    fftfilt* ssbFilter;
    fftfilt* dsbFilter;
    fftfilt::cmplx sum;
    MagAGC agc;
    DoubleBufferFIFO<fftfilt::cmplx> delayLine;
    double magsq, magsqSum, magsqPeak;

    Demod(int inRate, int ncoFreq, int rate, Real rfBw, Real low, Real vol, int span, bool bin, bool fl, bool ds, bool mu, bool agcOn, bool clamping,
          int timeLog2, int thrDb, int gateMs) :
        audioRate(rate), spanLog2(span), undersampleCount(0), magsqCount(0), binaural(bin), flip(fl), dsb(ds), mute(mu), agcActive(agcOn),
        audioActive(false), sum(0), agc(12000, kAgcTarget, 1e-2), delayLine(2 * 48000), magsq(0.0f), magsqSum(0.0f), magsqPeak(0.0f)
    {
        agc.setClampMax(SDR_RX_SCALED / 100.0);
        agc.setClamping(false);
        bandwidth = rfBw; lowCutoff = low; usb = true;
        if (bandwidth < 0) { bandwidth = -bandwidth; lowCutoff = -lowCutoff; usb = false; }
        if (bandwidth < 100.0f) { bandwidth = 100.0f; lowCutoff = 0; }
        nco.setFreq(ncoFreq, inRate);
        interp.create(16, inRate, bandwidth * 1.5f, 2.0f);
        distanceRemain = 0;
        distance = (Real) inRate / (Real) (unsigned) audioRate;
        ssbFilter = new fftfilt(lowCutoff / (float) (unsigned) audioRate, bandwidth / (float) (unsigned) audioRate, 1024);
        dsbFilter = new fftfilt((2.0f * bandwidth) / (float) (unsigned) audioRate, 2 * 1024);
        volume = vol;
        volume /= 4.0;
        const int nbSamples = (audioRate / 1000) * (1 << timeLog2);
        agc.setThresholdEnable(thrDb != 100);             // -SSBDemodSettings::m_minPowerThresholdDB of the 16-bit build
        const double threshold = CalcDb::powerFromdB(thrDb) * (SDR_RX_SCALED * SDR_RX_SCALED);
        if (nbSamples != 12000) { agc.resize(nbSamples, nbSamples / 2, kAgcTarget); agc.setStepDownDelay(nbSamples); }
        agc.setThreshold(threshold);
        agc.setGate((audioRate / 1000) * gateMs);
        agc.setClamping(clamping);
        for (int i = 0; i < 2 * 48000; i++) delayLine.write(fftfilt::cmplx(0, 0));
    }
    ~Demod() { delete ssbFilter; delete dsbFilter; }

    void feed(const std::vector<Sample>& in, std::vector<AudioSample>& audio, std::vector<Sample>& spectrum)
    {
        Complex ci;
        fftfilt::cmplx* sideband;
        const int decim = 1 << (spanLog2 - 1);
        const unsigned char mask = decim - 1;
        for (std::vector<Sample>::const_iterator it = in.begin(); it != in.end(); ++it) {
            Complex c(it->real(), it->imag());
            c *= nco.nextIQ();
            int n = 0;
            if (interp.decimate(&distanceRemain, c, &ci)) {
                n = dsb ? dsbFilter->runDSB(ci, &sideband) : ssbFilter->runSSB(ci, &sideband, usb);
                distanceRemain += distance;
            }
            for (int i = 0; i < n; i++) {
                sum += sideband[i];
                if (!(undersampleCount++ & mask)) {
                    Real avgr = sum.real() / decim;
                    Real avgi = sum.imag() / decim;
                    magsq = (avgr * avgr + avgi * avgi) / (SDR_RX_SCALED * SDR_RX_SCALED);
                    magsqSum += magsq;
                    if (magsq > magsqPeak) magsqPeak = magsq;
                    magsqCount++;
                    spectrum.push_back((!dsb & !usb) ? Sample(avgi, avgr) : Sample(avgr, avgi));
                    sum.real(0.0);
                    sum.imag(0.0);
                }
                float agcVal = agcActive ? agc.feedAndGetValue(sideband[i]) : 10.0;
                fftfilt::cmplx& delayed = delayLine.readBack(agc.getStepDownDelay());
                audioActive = delayed.real() != 0.0;
                delayLine.write(sideband[i] * agcVal);
                AudioSample a;
                if (mute) { a.r = 0; a.l = 0; }
                else {
                    fftfilt::cmplx z = delayed * agc.getStepValue();
                    if (binaural) {
                        if (flip) { a.r = (qint16)(z.imag() * volume); a.l = (qint16)(z.real() * volume); }
                        else { a.r = (qint16)(z.real() * volume); a.l = (qint16)(z.imag() * volume); }
                    } else {
                        Real demod = (z.real() + z.imag()) * 0.7;
                        qint16 sample = (qint16)(demod * volume);
                        a.l = sample; a.r = sample;
                    }
                }
                audio.push_back(a);
            }
        }
    }
};

} // namespace

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: ssb_rec input.bin output.bin\n"); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::perror("open"); return 2; }
    Demod* d = 0;
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        char cmd[16] = "";
        if (std::sscanf(line, "%15s", cmd) != 1) continue;
        if (!std::strcmp(cmd, "new")) {
            int v[13]; float rf, low, vol;
            if (std::sscanf(line, "%*s %d %d %d %f %f %f %d %d %d %d %d %d %d %d %d %d", &v[0], &v[1], &v[2], &rf, &low, &vol, &v[3], &v[4], &v[5], &v[6],
                            &v[7], &v[8], &v[9], &v[10], &v[11], &v[12]) != 16) return 3;
            delete d;
            d = new Demod(v[0], v[1], v[2], rf, low, vol, v[3], v[4] != 0, v[5] != 0, v[6] != 0, v[7] != 0, v[8] != 0, v[9] != 0, v[10], v[11], v[12]);
        } else if (!std::strcmp(cmd, "feed") && d) {
            long n;
            if (std::sscanf(line, "%*s %ld", &n) != 1) return 3;
            std::vector<Sample> s((size_t)n);
            for (long i = 0; i < n; i++) {
                int16_t iq[2];
                if (std::fread(iq, 2, 2, in) != 2) return 4;
                s[(size_t)i] = Sample(iq[0], iq[1]);
            }
            std::vector<AudioSample> audio;
            std::vector<Sample> spectrum;
            d->feed(s, audio, spectrum);
            int64_t k = (int64_t)audio.size();
            std::fwrite(&k, 8, 1, out);
            if (k) std::fwrite(audio.data(), sizeof(AudioSample), audio.size(), out);
            k = (int64_t)spectrum.size();
            std::fwrite(&k, 8, 1, out);
            if (k) std::fwrite(spectrum.data(), sizeof(Sample), spectrum.size(), out);
        } else if (!std::strcmp(cmd, "end") && d) {
            const int64_t tail[3] = { d->magsqCount, d->audioActive ? 1 : 0, (int64_t)d->undersampleCount };
            const double agcs[3] = { (double)d->agc.getValue(), (double)d->agc.getStepValue(), (double)d->agc.getStepDownValue() };
            std::fwrite(&d->magsq, 8, 1, out); std::fwrite(&d->magsqSum, 8, 1, out); std::fwrite(&d->magsqPeak, 8, 1, out);
            std::fwrite(tail, 8, 3, out); std::fwrite(agcs, 8, 3, out);
        }
    }
    delete d;
    std::fclose(out);
    return 0;
}
