// Recorder around the reference's own NCO, fftfilt (g_fft), PhaseDiscriminators, RDSPhaseLock, Interpolator and LowPassFilterRC,
// compiled where they lie by tests/golden/make_golden_bfm.py (strict IEEE, scalar: -O2 -fno-fast-math -ffp-contract=off,
// USE_SSE2 undefined).  BFMDemod itself cannot be instantiated outside the application (it attaches to a DeviceSourceAPI, the
// audio device manager and a threaded channelizer), so the per-sample loop of BFMDemod::feed with m_rdsActive clear and the
// calls of its constructor, applyChannelSettings(rate, offset, true) and applySettings(settings, true) are written here around
// the real members, in that order.  m_m1Sample of PhaseDiscriminators has no initialiser in the reference; value-initialisation
// pins it to 0.  The state the fixture keeps sits in private members: the two headers are read with them opened.
//
//   bfm_rec <input.bin> <output.bin>     commands on stdin, one per line:
//     new in_rate nco_freq audio_rate rf_bw af_bw volume squelch_db stereo lsb show_pilot     a fresh demodulator
//     feed n                               the next n Samples of input.bin (int16 I, Q)
//   output.bin, per feed: int64 pairs, the qint16 l, r pairs; int64 sink Samples, their real parts (the imaginary ones are
//   checked to be 0); double m_magsqSum, m_magsqPeak; int64 m_magsqCount, m_squelchState, locked(), m_lock_cnt; the bits of
//   m_pilot_level, m_freq, m_phase, X.m_y1, Y.m_y1
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
#define private public
#define protected public
#include "dsp/phaselock.h"
#include "dsp/filterrc.h"
#undef private
#undef protected

namespace {

struct Settings { Real m_rfBandwidth, m_afBandwidth, m_volume, m_squelch; bool m_audioStereo, m_lsbStereo, m_showPilot; };

struct Demod {
    int m_inputSampleRate;
    Settings m_settings;
    quint32 m_audioSampleRate;
    NCO m_nco;
    Interpolator m_interpolator;
    Real m_interpolatorDistance, m_interpolatorDistanceRemain;
    Interpolator m_interpolatorStereo;
    Real m_interpolatorStereoDistance, m_interpolatorStereoDistanceRemain;
    fftfilt* m_rfFilter;
    Real m_squelchLevel;
    int m_squelchState;
    double m_magsqSum, m_magsqPeak;
    int m_magsqCount;
    std::vector<Sample> m_sampleBuffer;
    RDSPhaseLock m_pilotPLL;
    Real m_pilotPLLSamples[4];
    LowPassFilterRC m_deemphasisFilterX, m_deemphasisFilterY;
    Real m_fmExcursion;
    PhaseDiscriminators m_phaseDiscri;
    static const int default_excursion = 750000;

    Demod(int inRate, int ncoFreq, quint32 audioRate, const Settings& settings) :
        m_inputSampleRate(384000), m_audioSampleRate(audioRate),
        m_pilotPLL(19000/384000, 50/384000, 0.01),
        m_deemphasisFilterX(50.0f * 48000 * 1.0e-6), m_deemphasisFilterY(50.0f * 48000 * 1.0e-6),
        m_fmExcursion(default_excursion), m_phaseDiscri()
    {
        const Real default_deemphasis = 50.0;
        m_magsqSum = 0.0f; m_magsqPeak = 0.0f; m_magsqCount = 0;
        m_squelchLevel = 0; m_squelchState = 0;
        m_interpolatorDistance = 0.0f; m_interpolatorDistanceRemain = 0.0f;
        m_interpolatorStereoDistance = 0.0f; m_interpolatorStereoDistanceRemain = 0.0f;
        m_pilotPLLSamples[0] = m_pilotPLLSamples[1] = m_pilotPLLSamples[2] = m_pilotPLLSamples[3] = 0;
        m_rfFilter = new fftfilt(-50000.0 / 384000.0, 50000.0 / 384000.0, 1024);
        m_deemphasisFilterX.configure(default_deemphasis * m_audioSampleRate * 1.0e-6);
        m_deemphasisFilterY.configure(default_deemphasis * m_audioSampleRate * 1.0e-6);
        m_phaseDiscri.setFMScaling(384000/m_fmExcursion);
        m_settings = settings;
        applyChannelSettings(inRate, ncoFreq);
        applySettings(settings);
    }
    ~Demod() { delete m_rfFilter; }

    void applyChannelSettings(int inputSampleRate, int ncoFreq)             // force
    {
        m_nco.setFreq(ncoFreq, inputSampleRate);
        m_pilotPLL.configure(19000.0/inputSampleRate, 50.0/inputSampleRate, 0.01);
        m_interpolator.create(16, inputSampleRate, m_settings.m_afBandwidth);
        m_interpolatorDistanceRemain = (Real) inputSampleRate / m_audioSampleRate;
        m_interpolatorDistance =  (Real) inputSampleRate / (Real) m_audioSampleRate;
        m_interpolatorStereo.create(16, inputSampleRate, m_settings.m_afBandwidth);
        m_interpolatorStereoDistanceRemain = (Real) inputSampleRate / m_audioSampleRate;
        m_interpolatorStereoDistance =  (Real) inputSampleRate / (Real) m_audioSampleRate;
        Real lowCut = -(m_settings.m_rfBandwidth / 2.0) / inputSampleRate;
        Real hiCut  = (m_settings.m_rfBandwidth / 2.0) / inputSampleRate;
        m_rfFilter->create_filter(lowCut, hiCut);
        m_phaseDiscri.setFMScaling(inputSampleRate / m_fmExcursion);
        m_inputSampleRate = inputSampleRate;
    }

    void applySettings(const Settings& settings)                            // force
    {
        m_pilotPLL.configure(19000.0/m_inputSampleRate, 50.0/m_inputSampleRate, 0.01);
        m_interpolator.create(16, m_inputSampleRate, settings.m_afBandwidth);
        m_interpolatorDistanceRemain = (Real) m_inputSampleRate / m_audioSampleRate;
        m_interpolatorDistance =  (Real) m_inputSampleRate / (Real) m_audioSampleRate;
        m_interpolatorStereo.create(16, m_inputSampleRate, settings.m_afBandwidth);
        m_interpolatorStereoDistanceRemain = (Real) m_inputSampleRate / m_audioSampleRate;
        m_interpolatorStereoDistance =  (Real) m_inputSampleRate / (Real) m_audioSampleRate;
        Real lowCut = -(settings.m_rfBandwidth / 2.0) / m_inputSampleRate;
        Real hiCut  = (settings.m_rfBandwidth / 2.0) / m_inputSampleRate;
        m_rfFilter->create_filter(lowCut, hiCut);
        m_phaseDiscri.setFMScaling(m_inputSampleRate / m_fmExcursion);
        m_squelchLevel = std::pow(10.0, settings.m_squelch / 10.0);
        m_settings = settings;
    }

    void feed(const std::vector<Sample>& in, std::vector<qint16>& audio)
    {
        Complex ci, cs;
        fftfilt::cmplx *rf;
        int rf_out;
        double msq;
        Real demod;
        m_sampleBuffer.clear();
        for (std::vector<Sample>::const_iterator it = in.begin(); it != in.end(); ++it) {
            Complex c(it->real() / SDR_RX_SCALEF, it->imag() / SDR_RX_SCALEF);
            c *= m_nco.nextIQ();
            rf_out = m_rfFilter->runFilt(c, &rf);
            for (int i = 0; i < rf_out; i++) {
                msq = rf[i].real()*rf[i].real() + rf[i].imag()*rf[i].imag();
                m_magsqSum += msq;
                if (msq > m_magsqPeak) m_magsqPeak = msq;
                m_magsqCount++;
                if (msq >= m_squelchLevel) {
                    if (m_squelchState < m_settings.m_rfBandwidth / 10) m_squelchState++;
                } else {
                    if (m_squelchState > 0) m_squelchState--;
                }
                if (m_squelchState > m_settings.m_rfBandwidth / 20) demod = m_phaseDiscri.phaseDiscriminator(rf[i]);
                else demod = 0;
                if (!m_settings.m_showPilot) m_sampleBuffer.push_back(Sample(demod * SDR_RX_SCALEF, 0.0));
                Real sampleStereo = 0.0f;
                if (m_settings.m_audioStereo) {
                    m_pilotPLL.process(demod, m_pilotPLLSamples);
                    if (m_settings.m_showPilot) m_sampleBuffer.push_back(Sample(m_pilotPLLSamples[1] * SDR_RX_SCALEF, 0.0));
                    if (m_settings.m_lsbStereo) {
                        Complex s(demod * m_pilotPLLSamples[1], demod * m_pilotPLLSamples[2]);
                        if (m_interpolatorStereo.decimate(&m_interpolatorStereoDistanceRemain, s, &cs)) {
                            sampleStereo = cs.real() + cs.imag();
                            m_interpolatorStereoDistanceRemain += m_interpolatorStereoDistance;
                        }
                    } else {
                        Complex s(demod * 1.17 * m_pilotPLLSamples[1], 0);
                        if (m_interpolatorStereo.decimate(&m_interpolatorStereoDistanceRemain, s, &cs)) {
                            sampleStereo = cs.real();
                            m_interpolatorStereoDistanceRemain += m_interpolatorStereoDistance;
                        }
                    }
                }
                Complex e(demod, 0);
                if (m_interpolator.decimate(&m_interpolatorDistanceRemain, e, &ci)) {
                    qint16 l, r;
                    if (m_settings.m_audioStereo) {
                        Real deemph_l, deemph_r;
                        m_deemphasisFilterX.process(ci.real() + sampleStereo, deemph_l);
                        m_deemphasisFilterY.process(ci.real() - sampleStereo, deemph_r);
                        l = (qint16)(deemph_l * (1<<12) * m_settings.m_volume);
                        r = (qint16)(deemph_r * (1<<12) * m_settings.m_volume);
                    } else {
                        Real deemph;
                        m_deemphasisFilterX.process(ci.real(), deemph);
                        quint16 sample = (qint16)(deemph * (1<<12) * m_settings.m_volume);
                        l = sample;
                        r = sample;
                    }
                    audio.push_back(l); audio.push_back(r);
                    m_interpolatorDistanceRemain += m_interpolatorDistance;
                }
            }
        }
    }
};

uint32_t bits(float v) { uint32_t i; std::memcpy(&i, &v, 4); return i; }

} // namespace

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: bfm_rec input.bin output.bin\n"); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::perror("open"); return 2; }
    Demod* d = 0;
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        char cmd[16] = "";
        if (std::sscanf(line, "%15s", cmd) != 1) continue;
        if (!std::strcmp(cmd, "new")) {
            int inRate, ncoFreq, audioRate, stereo, lsb, pilot; float rf, af, vol, sq;
            if (std::sscanf(line, "%*s %d %d %d %f %f %f %f %d %d %d", &inRate, &ncoFreq, &audioRate, &rf, &af, &vol, &sq, &stereo, &lsb, &pilot) != 10) return 3;
            delete d;
            Settings s = { rf, af, vol, sq, stereo != 0, lsb != 0, pilot != 0 };
            d = new Demod(inRate, ncoFreq, (quint32)audioRate, s);
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
            const int64_t k = (int64_t)(audio.size() / 2), m = (int64_t)d->m_sampleBuffer.size();
            std::fwrite(&k, 8, 1, out);
            if (k) std::fwrite(audio.data(), 2, audio.size(), out);
            std::fwrite(&m, 8, 1, out);
            for (int64_t i = 0; i < m; i++) {
                if (d->m_sampleBuffer[(size_t)i].imag() != 0) return 5;
                const qint16 re = d->m_sampleBuffer[(size_t)i].real();
                std::fwrite(&re, 2, 1, out);
            }
            const int64_t tail[4] = { d->m_magsqCount, d->m_squelchState, d->m_pilotPLL.locked() ? 1 : 0, d->m_pilotPLL.m_lock_cnt };
            const uint32_t b[5] = { bits(d->m_pilotPLL.m_pilot_level), bits(d->m_pilotPLL.m_freq), bits(d->m_pilotPLL.m_phase),
                                    bits(d->m_deemphasisFilterX.m_y1), bits(d->m_deemphasisFilterY.m_y1) };
            std::fwrite(&d->m_magsqSum, 8, 1, out); std::fwrite(&d->m_magsqPeak, 8, 1, out); std::fwrite(tail, 8, 4, out); std::fwrite(b, 4, 5, out);
        }
    }
    delete d;
    std::fclose(out);
    return 0;
}
