// Recorder around the reference's own NCO, Interpolator, MagAGC, MovingAverage, PhaseDiscriminators and Bandpass, compiled where
// they lie by tests/golden/make_golden_udpsrc.py (strict IEEE, scalar: -O2 -fno-fast-math -ffp-contract=off, USE_SSE2 undefined).
// UDPSrc itself cannot be instantiated outside the application (it attaches to a DeviceSourceAPI, binds a socket and creates
// a threaded channelizer), so what UDPSrc::feed does per resampled sample for the formats IQ16, IQ24, NFM, NFMMono, AMMono,
// AMNoDCMono and AMBPFMono is restated here in this project's words around those members, set up as the constructor,
// applySettings(settings, true), applyChannelSettings(.., true) and start() set them up.  Every value that the reference
// converts implicitly on the way into its UDPSink passes through a function parameter or a member of the same type here
// (FixReal, Real, int16_t, int32_t), so the compiler emits the conversion it emits there.
//
//   udpsrc_rec <input.bin> <output.bin>     commands on stdin, one per line:
//     new in_rate nco_freq output_sample_rate sample_format rf_bw fm_deviation gain squelch_db squelch_gate squelch_enabled agc
//     feed n                               the next n Samples of input.bin (int16 I, Q)
//     end                                  m_inMagsq and the squelch state
//   output.bin: per feed an int64 count, the payload bytes and the spectrum Samples; per end: double m_inMagsq, int64 open,
//   open count, close count
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
#include "dsp/movingaverage.h"
#include "dsp/agc.h"

namespace {

enum Format { IQ16 = 0, IQ24 = 1, NFM = 2, NFM_MONO = 3, AM_MONO = 8, AM_NODC_MONO = 9, AM_BPF_MONO = 10 };

// the bytes a UDPSink<T> would be handed, T by T
struct Payload {
    std::vector<char> bytes;
    struct Pair16 { int16_t re, im; Pair16(int16_t r, int16_t i) : re(r), im(i) {} };
    struct Pair32 { int32_t re, im; Pair32(int32_t r, int32_t i) : re(r), im(i) {} };
    template <class T> void append(const T& v) { const char* p = reinterpret_cast<const char*>(&v); bytes.insert(bytes.end(), p, p + sizeof(T)); }
    void mono(const int16_t& v) { append(v); }
    // the three entry points differ in their parameter types, which is where the reference's conversions happen
    void fixed_pair(FixReal re, FixReal im, bool wide) { if (wide) append(Pair32(re << 8, im << 8)); else append(Pair16(re, im)); }
    void fixed_mono(FixReal v) { mono(v); }
    void unit_pair(Real re, Real im) { append(Pair16(re * 32768.0, im * 32768.0)); }
    void unit_mono(Real v) { mono(v * 32768.0); }
};

// flag, opening count and closing count; gate 0 is the stateless form
struct Squelch {
    bool enabled, open; double level; int gate, release, opening, closing;
    void step(double power)
    {
        const bool above = !enabled || power > level;
        if (gate == 0) { open = above; return; }
        if (above) {
            if (opening < gate) opening++;
            else { closing = release; open = true; }
        } else if (closing > 0) closing--;
        else { opening = 0; open = false; }
    }
};

struct Channel {
    int inRate, format;
    float outRate, gain;
    bool agcOn;
    NCO nco;
    Interpolator resampler;
    Real distance;
    PhaseDiscriminators discri;
    MovingAverage<double> inputPower, envelopeMean;
    Bandpass<double> bandpass;
    MagAGC agc;
    Squelch squelch;
    double inMagsq;
    Payload payload;
    std::vector<Sample> spectrum;

    Channel(int inRateArg, int ncoFreq, float rate, int fmt, float rfBw, int fmDeviation, float g, int squelchdB, int gateSetting, bool enabled, bool agcFlag) :
        inRate(inRateArg), format(fmt), outRate(rate), gain(g), agcOn(agcFlag && fmt >= AM_MONO),
        inputPower(480, 1e-10), envelopeMean(1200, 1e-10), agc(9600, 16384.0f, 1e-6), inMagsq(0)
    {
        agc.setClampMax(SDR_RX_SCALED*SDR_RX_SCALED);
        agc.setClamping(true);
        nco.setFreq(ncoFreq, inRate);
        resampler.create(16, inRate, rfBw / 2.0);
        distance = inRate / outRate;
        squelch.enabled = enabled; squelch.open = false; squelch.opening = 0; squelch.closing = 0;
        squelch.gate = (outRate * gateSetting) / 100;
        squelch.release = (outRate * gateSetting) / 100;
        squelch.level = std::pow(10.0, squelchdB / 10.0);
        agc.resize(outRate/5, outRate/20, 16384.0f);
        agc.setStepDownDelay((outRate * (gateSetting == 0 ? 1 : gateSetting))/100);
        agc.setGate(outRate * 0.05);
        agc.setThreshold(squelch.level*(1<<23));
        bandpass.create(301, outRate, 300.0, rfBw / 2.0f);
        inputPower.resize(outRate * 0.01, 1e-10);
        envelopeMean.resize(outRate * 0.005, 1e-10);
        discri.setFMScaling((float) outRate / (2.0f * fmDeviation));
        discri.reset();
    }

    void sample(Complex& ci)
    {
        double factor = 1.0, power;
        if (agcOn) { factor = agc.feedAndGetValue(ci); power = agc.getMagSq(); }
        else power = ci.real()*ci.real() + ci.imag()*ci.imag();
        inputPower.feed(power / (SDR_RX_SCALED*SDR_RX_SCALED));
        inMagsq = inputPower.average();
        spectrum.push_back(Sample(ci.real(), ci.imag()));
        squelch.step(inMagsq);
        const bool open = squelch.open;
        switch (format) {
        case NFM: case NFM_MONO: {
            Real d = open ? discri.phaseDiscriminator(ci) * gain : 0;
            if (format == NFM) payload.unit_pair(d, d); else payload.unit_mono(d);
            break; }
        case AM_MONO: {
            Real a = open ? sqrt(power) * factor * gain : 0;
            payload.fixed_mono((FixReal) a);
            break; }
        case AM_NODC_MONO: case AM_BPF_MONO: {
            if (!open) { payload.fixed_mono(0); break; }
            double e = sqrt(power);
            if (format == AM_NODC_MONO) { envelopeMean.feed(e); e = e - envelopeMean.average(); }
            else { e = bandpass.filter(e); e /= 301.0; }
            Real a = e * factor * gain;
            payload.fixed_mono((FixReal) a);
            break; }
        default:
            if (open) payload.fixed_pair(ci.real() * gain, ci.imag() * gain, format == IQ24);
            else payload.fixed_pair(0, 0, format == IQ24);
        }
    }

    void feed(const std::vector<Sample>& in)
    {
        Complex ci;
        payload.bytes.clear();
        spectrum.clear();
        for (size_t k = 0; k < in.size(); k++) {
            Complex c(in[k].real(), in[k].imag());
            c *= nco.nextIQ();
            if (resampler.decimate(&distance, c, &ci)) {
                sample(ci);
                distance += inRate / outRate;
            }
        }
    }
};

} // namespace

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: udpsrc_rec input.bin output.bin\n"); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::perror("open"); return 2; }
    Channel* d = 0;
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        char cmd[16] = "";
        if (std::sscanf(line, "%15s", cmd) != 1) continue;
        if (!std::strcmp(cmd, "new")) {
            int inRate, ncoFreq, fmt, fmDev, sqdb, gate, enabled, agc; float rate, rf, gain;
            if (std::sscanf(line, "%*s %d %d %f %d %f %d %f %d %d %d %d", &inRate, &ncoFreq, &rate, &fmt, &rf, &fmDev, &gain, &sqdb, &gate, &enabled, &agc) != 11) return 3;
            delete d;
            d = new Channel(inRate, ncoFreq, rate, fmt, rf, fmDev, gain, sqdb, gate, enabled != 0, agc != 0);
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
            const int64_t k = (int64_t)d->spectrum.size();
            std::fwrite(&k, 8, 1, out);
            if (k) {
                std::fwrite(d->payload.bytes.data(), 1, d->payload.bytes.size(), out);
                for (int64_t i = 0; i < k; i++) {
                    const int16_t iq[2] = { (int16_t)d->spectrum[(size_t)i].real(), (int16_t)d->spectrum[(size_t)i].imag() };
                    std::fwrite(iq, 2, 2, out);
                }
            }
        } else if (!std::strcmp(cmd, "end") && d) {
            const int64_t tail[3] = { d->squelch.open ? 1 : 0, (int64_t)d->squelch.opening, (int64_t)d->squelch.closing };
            std::fwrite(&d->inMagsq, 8, 1, out); std::fwrite(tail, 8, 3, out);
        }
    }
    delete d;
    std::fclose(out);
    return 0;
}
