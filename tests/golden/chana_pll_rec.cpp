// Recorder around the reference's own PhaseLockComplex, FreqLockComplex, NCOF, Interpolator, fftfilt and fftcorr, compiled where
// they lie by tests/golden/make_golden_chana_pll.py (strict IEEE, scalar: -O2 -fno-fast-math -ffp-contract=off, USE_SSE2
// undefined).  As tests/golden/chana_rec.cpp, with m_pll, m_fll, m_pllPskOrder and InputPLL: ChannelAnalyzer itself cannot be
// instantiated outside the application, so the loops of feed, processOneSample and feedOneSample and the configuration paths
// are written here around the real members, in the order the application reaches them: the constructor (input rate 48000,
// default settings, computeCoefficients), applySettings(settings, true), applyChannelSettings(in_rate, offset) and start().
//
//   chana_pll_rec <input.bin> <output.bin>     commands on stdin, one per line:
//     new in_rate nco_freq down_sample down_sample_rate bandwidth low_cutoff span_log2 ssb rrc rrc_rolloff input_type pll fll psk_order
//     feed n                               the next n Samples of input.bin (int16 I, Q)
//     time                                 prints the seconds spent in feed() since `new`
//   output.bin: per feed an int64 Sample count, the Samples (re, im), double m_magsq, int32 isPllLocked, float getPllFrequency,
//   getPllDeltaPhase, getPllPhase
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "dsp/dsptypes.h"
#include "dsp/ncof.h"
#include "dsp/interpolator.h"
#include "dsp/fftfilt.h"
#include "dsp/fftcorr.h"
#include "dsp/phaselockcomplex.h"
#include "dsp/freqlockcomplex.h"

#define ssbFftLen 1024

namespace {

struct Settings {
    bool downSample; quint32 downSampleRate; int bandwidth, lowCutoff, spanLog2; bool ssb, pll, fll, rrc; quint32 rrcRolloff; unsigned int pllPskOrder;
    int inputType;
    Settings() : downSample(false), downSampleRate(0), bandwidth(5000), lowCutoff(300), spanLog2(0), ssb(false), pll(false), fll(false), rrc(false),
                 rrcRolloff(35), pllPskOrder(1), inputType(0) {}
};

struct Analyzer {
    Settings m_settings;
    int m_inputSampleRate, m_inputFrequencyOffset, m_undersampleCount;
    fftfilt::cmplx m_sum;
    bool m_usb, m_useInterpolator;
    double m_magsq;
    NCOF m_nco;
    PhaseLockComplex m_pll;
    FreqLockComplex m_fll;
    Interpolator m_interpolator;
    Real m_interpolatorDistance, m_interpolatorDistanceRemain;
    fftfilt* SSBFilter; fftfilt* DSBFilter; fftfilt* RRCFilter;
    fftcorr* m_corr;
    std::vector<Sample> m_sampleBuffer;

    Analyzer()
    {
        m_undersampleCount = 0; m_sum = 0; m_usb = true; m_magsq = 0; m_useInterpolator = false;
        m_interpolatorDistance = 1.0f; m_interpolatorDistanceRemain = 0.0f;
        m_inputSampleRate = 48000; m_inputFrequencyOffset = 0;
        SSBFilter = new fftfilt(m_settings.lowCutoff / m_inputSampleRate, m_settings.bandwidth / m_inputSampleRate, ssbFftLen);
        DSBFilter = new fftfilt(m_settings.bandwidth / m_inputSampleRate, 2 * ssbFftLen);
        RRCFilter = new fftfilt(m_settings.bandwidth / m_inputSampleRate, 2 * ssbFftLen);
        m_corr = new fftcorr(8 * ssbFftLen);
        m_pll.computeCoefficients(0.002f, 0.5f, 10.0f);
        applyChannelSettings(m_inputSampleRate, m_inputFrequencyOffset, true);
        applySettings(m_settings, true);
    }
    ~Analyzer() { delete SSBFilter; delete DSBFilter; delete RRCFilter; delete m_corr; }

    void start() { applyChannelSettings(m_inputSampleRate, m_inputFrequencyOffset, true); }

    void applyChannelSettings(int inputSampleRate, int inputFrequencyOffset, bool force = false)
    {
        if ((m_inputFrequencyOffset != inputFrequencyOffset) || (m_inputSampleRate != inputSampleRate) || force)
            m_nco.setFreq(-inputFrequencyOffset, inputSampleRate);
        if ((m_inputSampleRate != inputSampleRate) || force) {
            m_interpolator.create(16, inputSampleRate, inputSampleRate / 2.2f);
            m_interpolatorDistanceRemain = 0;
            m_interpolatorDistance = (Real) inputSampleRate / (Real) m_settings.downSampleRate;
            if (!m_settings.downSample) {
                setFilters(inputSampleRate, m_settings.bandwidth, m_settings.lowCutoff);
                m_pll.setSampleRate(inputSampleRate / (1 << m_settings.spanLog2));
                m_fll.setSampleRate(inputSampleRate / (1 << m_settings.spanLog2));
            }
        }
        m_inputSampleRate = inputSampleRate;
        m_inputFrequencyOffset = inputFrequencyOffset;
    }

    void setFilters(int sampleRate, float bandwidth, float lowCutoff)
    {
        if (bandwidth < 0) { bandwidth = -bandwidth; lowCutoff = -lowCutoff; m_usb = false; }
        else m_usb = true;
        if (bandwidth < 100.0f) { bandwidth = 100.0f; lowCutoff = 0; }
        SSBFilter->create_filter(lowCutoff / sampleRate, bandwidth / sampleRate);
        DSBFilter->create_dsb_filter(bandwidth / sampleRate);
        RRCFilter->create_rrc_filter(bandwidth / sampleRate, m_settings.rrcRolloff / 100.0);
    }

    void applySettings(const Settings& settings, bool force = false)
    {
        if ((settings.downSampleRate != m_settings.downSampleRate) || force) {
            m_interpolator.create(16, m_inputSampleRate, m_inputSampleRate / 2.2);
            m_interpolatorDistanceRemain = 0.0f;
            m_interpolatorDistance = (Real) m_inputSampleRate / (Real) settings.downSampleRate;
        }
        if ((settings.downSample != m_settings.downSample) || force) {
            int sampleRate = settings.downSample ? settings.downSampleRate : m_inputSampleRate;
            m_useInterpolator = settings.downSample;
            setFilters(sampleRate, settings.bandwidth, settings.lowCutoff);
            m_pll.setSampleRate(sampleRate / (1 << settings.spanLog2));
            m_fll.setSampleRate(sampleRate / (1 << settings.spanLog2));
        }
        if ((settings.bandwidth != m_settings.bandwidth) || (settings.lowCutoff != m_settings.lowCutoff) || force)
            setFilters(settings.downSample ? settings.downSampleRate : m_inputSampleRate, settings.bandwidth, settings.lowCutoff);
        if ((settings.rrcRolloff != m_settings.rrcRolloff) || force) {
            float sampleRate = settings.downSample ? (float) settings.downSampleRate : (float) m_inputSampleRate;
            RRCFilter->create_rrc_filter(settings.bandwidth / sampleRate, settings.rrcRolloff / 100.0);
        }
        if ((settings.spanLog2 != m_settings.spanLog2) || force) {
            int sampleRate = (settings.downSample ? settings.downSampleRate : m_inputSampleRate) / (1 << m_settings.spanLog2);
            m_pll.setSampleRate(sampleRate);
            m_fll.setSampleRate(sampleRate);
        }
        if (settings.pll != m_settings.pll || force) {
            if (settings.pll) { m_pll.reset(); m_fll.reset(); }
        }
        if (settings.fll != m_settings.fll || force) {
            if (settings.fll) m_fll.reset();
        }
        if (settings.pllPskOrder != m_settings.pllPskOrder || force) {
            if (settings.pllPskOrder < 32) m_pll.setPskOrder(settings.pllPskOrder);
        }
        m_settings = settings;
    }

    void feedOneSample(const fftfilt::cmplx& s, const fftfilt::cmplx& pll)
    {
        switch (m_settings.inputType) {
        case 1:
            if (m_settings.ssb & !m_usb) m_sampleBuffer.push_back(Sample(pll.imag() * SDR_RX_SCALEF, pll.real() * SDR_RX_SCALEF));
            else m_sampleBuffer.push_back(Sample(pll.real() * SDR_RX_SCALEF, pll.imag() * SDR_RX_SCALEF));
            break;
        case 2: {
            std::complex<float> a = m_corr->run(s / (SDR_RX_SCALEF / 768.0f), 0);
            if (m_settings.ssb & !m_usb) m_sampleBuffer.push_back(Sample(a.imag(), a.real()));
            else m_sampleBuffer.push_back(Sample(a.real(), a.imag()));
        } break;
        default:
            if (m_settings.ssb & !m_usb) m_sampleBuffer.push_back(Sample(s.imag(), s.real()));
            else m_sampleBuffer.push_back(Sample(s.real(), s.imag()));
            break;
        }
    }

    void processOneSample(Complex& c, fftfilt::cmplx* sideband)
    {
        int n_out;
        int decim = 1 << m_settings.spanLog2;
        if (m_settings.ssb) n_out = SSBFilter->runSSB(c, &sideband, m_usb);
        else if (m_settings.rrc) n_out = RRCFilter->runFilt(c, &sideband);
        else n_out = DSBFilter->runDSB(c, &sideband);
        for (int i = 0; i < n_out; i++) {
            m_sum += sideband[i];
            if (!(m_undersampleCount++ & (decim - 1))) {
                m_sum /= decim;
                Real re = m_sum.real() / SDR_RX_SCALEF;
                Real im = m_sum.imag() / SDR_RX_SCALEF;
                m_magsq = re * re + im * im;
                std::complex<float> mix;
                if (m_settings.pll) {
                    if (m_settings.fll) {
                        m_fll.feed(re, im);
                        mix = m_sum * std::conj(m_fll.getComplex());
                    } else {
                        m_pll.feed(re, im);
                        mix = m_sum * std::conj(m_pll.getComplex());
                    }
                }
                feedOneSample(m_settings.pll ? mix : m_sum, m_settings.fll ? m_fll.getComplex() : m_pll.getComplex());
                m_sum = 0;
            }
        }
    }

    void feed(const std::vector<Sample>& in)
    {
        fftfilt::cmplx* sideband = 0;
        Complex ci;
        for (std::vector<Sample>::const_iterator it = in.begin(); it < in.end(); ++it) {
            Complex c(it->real(), it->imag());
            c *= m_nco.nextIQ();
            if (m_useInterpolator) {
                if (m_interpolator.decimate(&m_interpolatorDistanceRemain, c, &ci)) {
                    processOneSample(ci, sideband);
                    m_interpolatorDistanceRemain += m_interpolatorDistance;
                }
            } else processOneSample(c, sideband);
        }
    }
};

} // namespace

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: chana_pll_rec input.bin output.bin\n"); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::perror("open"); return 2; }
    Analyzer* d = 0;
    double spent = 0;
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        char cmd[16] = "";
        if (std::sscanf(line, "%15s", cmd) != 1) continue;
        if (!std::strcmp(cmd, "new")) {
            int v[14];
            if (std::sscanf(line, "%*s %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7], &v[8], &v[9],
                            &v[10], &v[11], &v[12], &v[13]) != 14) return 3;
            delete d;
            d = new Analyzer;
            spent = 0;
            Settings s;
            s.downSample = v[2] != 0; s.downSampleRate = (quint32) v[3]; s.bandwidth = v[4]; s.lowCutoff = v[5]; s.spanLog2 = v[6];
            s.ssb = v[7] != 0; s.rrc = v[8] != 0; s.rrcRolloff = (quint32) v[9]; s.inputType = v[10];
            s.pll = v[11] != 0; s.fll = v[12] != 0; s.pllPskOrder = (unsigned int) v[13];
            d->applySettings(s, true);
            d->applyChannelSettings(v[0], -v[1]);           // the analyzer is told the offset; its NCO runs at minus that
            d->start();
        } else if (!std::strcmp(cmd, "feed") && d) {
            long n;
            if (std::sscanf(line, "%*s %ld", &n) != 1) return 3;
            std::vector<Sample> s((size_t)n);
            for (long i = 0; i < n; i++) {
                int16_t iq[2];
                if (std::fread(iq, 2, 2, in) != 2) return 4;
                s[(size_t)i] = Sample(iq[0], iq[1]);
            }
            const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
            d->feed(s);
            spent += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            int64_t k = (int64_t)d->m_sampleBuffer.size();
            std::fwrite(&k, 8, 1, out);
            if (k) std::fwrite(d->m_sampleBuffer.data(), sizeof(Sample), d->m_sampleBuffer.size(), out);
            d->m_sampleBuffer.clear();
            const int32_t locked = d->m_settings.pll && d->m_pll.locked();
            const float st[3] = { d->m_pll.getFreq(), d->m_pll.getDeltaPhi(), d->m_pll.getPhiHat() };
            std::fwrite(&d->m_magsq, 8, 1, out); std::fwrite(&locked, 4, 1, out); std::fwrite(st, 4, 3, out);
        } else if (!std::strcmp(cmd, "time") && d) {
            std::printf("%.6f\n", spent);
        }
    }
    delete d;
    std::fclose(out);
    return 0;
}
