// Recorder around the reference's own classes for BFMDemod::feed with m_rdsActive set: what tests/golden/bfm_rec.cpp wraps (NCO,
// fftfilt, PhaseDiscriminators, RDSPhaseLock, Interpolator, LowPassFilterRC) plus m_interpolatorRDS, RDSDemod (a QObject: its
// header goes through moc) and RDSDecoder, compiled where they lie by tests/golden/make_golden_bfm_rds.py (strict IEEE, scalar).
// The per-sample loop of BFMDemod::feed (bfmdemod.cpp:116-281) and the calls of the constructor, applyChannelSettings(rate,
// offset, true) and applySettings(settings, true) are written here around the real members, as in bfm_rec.cpp; RDSParser stays
// out (the groups are recorded instead of parsed).  Private members are read with the headers opened.
//
//   bfm_rds_rec <input.bin> <output.bin>     commands on stdin, one per line:
//     new in_rate nco_freq audio_rate rf_bw af_bw volume squelch_db stereo lsb show_pilot rds     a fresh demodulator
//     feed n                                   the next n Samples of input.bin (int16 I, Q)
//   output.bin, per feed: int64 pairs, the l, r pairs; int64 sink Samples, their real parts; int64 bits, one byte each, then the
//   index among the feed's RDS samples each came out at (int32); int64 groups, four uint16 each, then their indices; int64 RDS samples, subcarr_bb of each (float); int64 unsure (rds_mix.hpp's mark, on the recorder's
//   own demod and phase) and int64 mixer samples whose r differs from rds_mix's; the report (acc, qua, fclk, m_qua as float bits,
//   synced()); N_STATE 64-bit words of state in the order of tests/bfm_rds_cases.py's STATE_FIELDS.
//   bfm_rds_rec --framesync <bits.bin> <output.bin>    a fresh RDSDecoder on the bytes of bits.bin; per step 10 bytes:
//   group_ready, synced(), getGroup()[0..3] as uint16
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
#include <QObject>
#include "rdsdemod.h"
#include "rdsdecoder.h"
#undef private
#undef protected
#include "rds_mix.hpp"

namespace {

struct Settings { Real m_rfBandwidth, m_afBandwidth, m_volume, m_squelch; bool m_audioStereo, m_lsbStereo, m_showPilot, m_rdsActive; };

struct Demod {
    int m_inputSampleRate;
    Settings m_settings;
    quint32 m_audioSampleRate;
    NCO m_nco;
    Interpolator m_interpolator;
    Real m_interpolatorDistance, m_interpolatorDistanceRemain;
    Interpolator m_interpolatorStereo;
    Real m_interpolatorStereoDistance, m_interpolatorStereoDistanceRemain;
    Interpolator m_interpolatorRDS;
    Real m_interpolatorRDSDistance, m_interpolatorRDSDistanceRemain;
    RDSDemod m_rdsDemod;
    RDSDecoder m_rdsDecoder;
    std::vector<uint8_t> m_bits;
    std::vector<uint16_t> m_groups;
    std::vector<Real> m_bb, m_cr;                          // subcarr_bb and cr.real() of every RDS sample
    std::vector<int32_t> m_bitAt, m_groupAt;               // index among the feed's RDS samples
    int64_t m_unsure, m_mixDiffers;
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
        m_interpolatorRDSDistance = 0.0f; m_interpolatorRDSDistanceRemain = 0.0f;
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
        m_interpolatorRDS.create(4, inputSampleRate, 600.0);
        m_interpolatorRDSDistanceRemain = (Real) inputSampleRate / 250000.0;
        m_interpolatorRDSDistance =  (Real) inputSampleRate / 250000.0;
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
        m_interpolatorRDS.create(4, m_inputSampleRate, 600.0);
        m_interpolatorRDSDistanceRemain = (Real) m_inputSampleRate / 250000.0;
        m_interpolatorRDSDistance =  (Real) m_inputSampleRate / 250000.0;
        Real lowCut = -(settings.m_rfBandwidth / 2.0) / m_inputSampleRate;
        Real hiCut  = (settings.m_rfBandwidth / 2.0) / m_inputSampleRate;
        m_rfFilter->create_filter(lowCut, hiCut);
        m_phaseDiscri.setFMScaling(m_inputSampleRate / m_fmExcursion);
        m_squelchLevel = std::pow(10.0, settings.m_squelch / 10.0);
        m_settings = settings;
    }

    void feed(const std::vector<Sample>& in, std::vector<qint16>& audio)
    {
        Complex ci, cs, cr;
        fftfilt::cmplx *rf;
        int rf_out;
        double msq;
        Real demod;
        m_sampleBuffer.clear();
        m_bits.clear(); m_groups.clear(); m_bb.clear(); m_cr.clear(); m_bitAt.clear(); m_groupAt.clear(); m_unsure = 0; m_mixDiffers = 0;
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
                if (m_settings.m_rdsActive) {
                    Complex r(demod * 2.0 * std::cos(3.0 * m_pilotPLLSamples[3]), 0.0);
                    bool unsure;
                    const float ours = m_settings.m_audioStereo ? sdrx::rds_mix(demod, m_pilotPLLSamples[3], &unsure) : (unsure = false, demod + demod);
                    if (unsure) m_unsure++;
                    const float theirs = r.real();
                    if (std::memcmp(&ours, &theirs, 4)) m_mixDiffers++;
                    if (m_interpolatorRDS.decimate(&m_interpolatorRDSDistanceRemain, r, &cr)) {
                        bool bit;
                        const bool got = m_rdsDemod.process(cr.real(), bit);
                        m_bb.push_back(m_rdsDemod.m_parms.subcarr_bb[0]);
                        m_cr.push_back(cr.real());
                        if (got) {
                            m_bits.push_back(bit ? 1 : 0);
                            m_bitAt.push_back((int32_t)m_bb.size() - 1);
                            if (m_rdsDecoder.frameSync(bit)) m_groupAt.push_back((int32_t)m_bb.size() - 1);
                            if (m_groupAt.size() * 4 > m_groups.size()) for (int g = 0; g < 4; g++) m_groups.push_back((uint16_t)m_rdsDecoder.getGroup()[g]);
                        }
                        m_interpolatorRDSDistanceRemain += m_interpolatorRDSDistance;
                    }
                }
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
uint64_t dbits(double v) { uint64_t i; std::memcpy(&i, &v, 8); return i; }

int framesync(const char* fin, const char* fout)
{
    FILE* in = std::fopen(fin, "rb");
    FILE* out = std::fopen(fout, "wb");
    if (!in || !out) { std::perror("open"); return 2; }
    RDSDecoder dec;
    int c;
    while ((c = std::fgetc(in)) != EOF) {
        const uint8_t ready = dec.frameSync(c != 0) ? 1 : 0, synced = dec.synced() ? 1 : 0;
        uint16_t g[4];
        for (int i = 0; i < 4; i++) g[i] = (uint16_t)dec.getGroup()[i];
        std::fwrite(&ready, 1, 1, out); std::fwrite(&synced, 1, 1, out); std::fwrite(g, 2, 4, out);
    }
    std::fclose(in); std::fclose(out);
    return 0;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc == 4 && !std::strcmp(argv[1], "--framesync")) return framesync(argv[2], argv[3]);
    if (argc != 3) { std::fprintf(stderr, "usage: bfm_rds_rec input.bin output.bin | --framesync bits.bin output.bin\n"); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::perror("open"); return 2; }
    Demod* d = 0;
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        char cmd[16] = "";
        if (std::sscanf(line, "%15s", cmd) != 1) continue;
        if (!std::strcmp(cmd, "new")) {
            int inRate, ncoFreq, audioRate, stereo, lsb, pilot, rds; float rf, af, vol, sq;
            if (std::sscanf(line, "%*s %d %d %d %f %f %f %f %d %d %d %d", &inRate, &ncoFreq, &audioRate, &rf, &af, &vol, &sq, &stereo, &lsb, &pilot, &rds) != 11) return 3;
            delete d;
            Settings s = { rf, af, vol, sq, stereo != 0, lsb != 0, pilot != 0, rds != 0 };
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
            const int64_t nb = (int64_t)d->m_bits.size(), ng = (int64_t)(d->m_groups.size() / 4), nr = (int64_t)d->m_bb.size();
            std::fwrite(&nb, 8, 1, out); if (nb) { std::fwrite(d->m_bits.data(), 1, (size_t)nb, out); std::fwrite(d->m_bitAt.data(), 4, (size_t)nb, out); }
            std::fwrite(&ng, 8, 1, out); if (ng) { std::fwrite(d->m_groups.data(), 2, (size_t)ng * 4, out); std::fwrite(d->m_groupAt.data(), 4, (size_t)ng, out); }
            std::fwrite(&nr, 8, 1, out); if (nr) { std::fwrite(d->m_bb.data(), 4, (size_t)nr, out); std::fwrite(d->m_cr.data(), 4, (size_t)nr, out); }
            std::fwrite(&d->m_unsure, 8, 1, out); std::fwrite(&d->m_mixDiffers, 8, 1, out);
            const RDSDemod& q = d->m_rdsDemod;
            const RDSDecoder& dk = d->m_rdsDecoder;
            const uint32_t rep[5] = { bits(q.m_report.acc), bits(q.m_report.qua), bits(q.m_report.fclk), bits(dk.m_qua), dk.synced() ? 1u : 0u };
            std::fwrite(rep, 4, 5, out);
            const uint64_t st[] = {
                dbits(q.m_parms.subcarr_phi), dbits(q.m_parms.clock_offset), dbits(q.m_parms.clock_phi), dbits(q.m_parms.prev_clock_phi), dbits(q.m_parms.d_cphi),
                bits(q.m_xv[0][0]), bits(q.m_xv[0][1]), bits(q.m_xv[0][2]), bits(q.m_yv[0][0]), bits(q.m_yv[0][1]), bits(q.m_yv[0][2]),
                bits(q.m_parms.prev_bb), bits(q.m_parms.acc), bits(q.m_parms.prev_acc), bits(q.m_parms.lo_clock), bits(q.m_parms.prev_lo_clock),
                (uint64_t)(int64_t)q.m_parms.numsamples, (uint64_t)(int64_t)q.m_parms.counter, (uint64_t)(int64_t)q.m_parms.reading_frame,
                (uint64_t)(int64_t)q.m_parms.tot_errs[0], (uint64_t)(int64_t)q.m_parms.tot_errs[1], (uint64_t)(int64_t)q.m_parms.dbit,
                bits(d->m_interpolatorRDSDistanceRemain), bits(d->m_pilotPLLSamples[3]), (uint64_t)nr,
                (uint64_t)dk.m_reg, (uint64_t)dk.m_lastseenOffsetCounter, (uint64_t)dk.m_bitCounter,
                dk.m_blockBitCounter, dk.m_wrongBlocksCounter, dk.m_blocksCounter, dk.m_groupGoodBlocksCounter,
                dk.m_group[0], dk.m_group[1], dk.m_group[2], dk.m_group[3],
                (uint64_t)(dk.m_sync == RDSDecoder::SYNC ? 1 : 0), (uint64_t)dk.m_presync, (uint64_t)dk.m_lastseenOffset, (uint64_t)dk.m_blockNumber,
                (uint64_t)dk.m_groupAssemblyStarted, (uint64_t)dk.m_goodBlock, bits(dk.m_qua) };
            std::fwrite(st, 8, sizeof st / sizeof st[0], out);
        }
    }
    delete d;
    std::fclose(out);
    return 0;
}
