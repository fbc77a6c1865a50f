// Recorder for UDPSrc's SSB formats (FormatLSB, FormatUSB, FormatLSBMono, FormatUSBMono) around the reference's own fftfilt,
// g_fft, MagAGC, MovingAverage, NCO and Interpolator, compiled where they lie by tests/golden/make_golden_udpsrc_ssb.py (strict
// IEEE, scalar: -O2 -fno-fast-math -ffp-contract=off, USE_SSE2 undefined).  The shape of udpsrc_rec.cpp: UDPSrc itself
// cannot be instantiated outside the application, so what UDPSrc::feed does per resampled sample for these formats is
// restated here in this project's words around those members, set up as the constructor, applySettings(settings, true),
// applyChannelSettings(.., true) and start() set them up.  Three things are kept exactly as the reference has them, because
// they are what this recorder is for:
//   - the filter is made once, from the default settings (12500 Hz, 48000 S/s), before the channel's own settings arrive, and
//     nothing afterwards touches it;
//   - `ci *= factor` is written on a Complex with a double on the right, so the compiler picks the operator it picks there;
//   - the branch of format 4 is an `if` of its own, and the ladder that starts at format 5 runs behind it down to its last
//     branch, the raw I/Q one.
// Values converted implicitly on the way into the UDPSink pass through parameters of the reference's types (FixReal).
//
//   udpsrc_ssb_rec <input.bin> <output.bin>     commands on stdin, one per line:
//     new in_rate nco_freq output_sample_rate sample_format rf_bw fm_deviation gain squelch_db squelch_gate squelch_enabled agc
//     feed n                               the next n Samples of input.bin (int16 I, Q)
//     end                                  state and the filter design
//   output.bin: per feed two int64 (resampled samples, payload elements), the payload bytes and the spectrum Samples; per end:
//   double m_inMagsq, int64 open, open count, close count, gate, release, inptr; 1024 floats of the filter
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "dsp/dsptypes.h"
#include "dsp/nco.h"
#include "dsp/interpolator.h"
#include "dsp/movingaverage.h"
#include "dsp/agc.h"
#include "dsp/fftfilt.h"

namespace {

enum Format { LSB = 4, USB = 5, LSB_MONO = 6, USB_MONO = 7 };

struct Payload {
    std::vector<char> bytes;
    struct Pair16 { int16_t re, im; Pair16(int16_t r, int16_t i) : re(r), im(i) {} };
    template <class T> void append(const T& v) { const char* p = reinterpret_cast<const char*>(&v); bytes.insert(bytes.end(), p, p + sizeof(T)); }
    void fixed_pair(FixReal re, FixReal im) { append(Pair16(re, im)); }
    void fixed_mono(FixReal v) { const int16_t s = v; append(s); }
};

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

// the filter's protected members, read only
struct Filter : fftfilt {
    Filter(float f1, float f2, int len) : fftfilt(f1, f2, len) {}
    int waiting() const { return inptr; }
    const cmplx* design() const { return filter; }
};

struct Defaults { float rfBandwidth, outputSampleRate; Defaults() : rfBandwidth(12500), outputSampleRate(48000) {} };

struct Channel {
    int inRate, format;
    float outRate, gain;
    bool agcOn;
    NCO nco;
    Interpolator resampler;
    Real distance;
    MovingAverage<double> inputPower;
    MagAGC agc;
    Squelch squelch;
    double inMagsq;
    Filter* filter;
    Payload payload;
    std::vector<Sample> spectrum;

    Channel(int inRateArg, int ncoFreq, float rate, int fmt, float rfBw, int, float g, int squelchdB, int gateSetting, bool enabled, bool agcFlag) :
        inRate(inRateArg), format(fmt), outRate(rate), gain(g), agcOn(agcFlag),
        inputPower(480, 1e-10), agc(9600, 16384.0f, 1e-6), inMagsq(0)
    {
        const Defaults first;                               // the constructor's m_settings
        filter = new Filter(0.0, (first.rfBandwidth / 2.0) / first.outputSampleRate, 512);
        agc.setClampMax(SDR_RX_SCALED*SDR_RX_SCALED);
        agc.setClamping(true);
        nco.setFreq(ncoFreq, inRate);
        resampler.create(16, inRate, rfBw / 2.0);
        distance = inRate / outRate;
        squelch.enabled = enabled; squelch.open = false; squelch.opening = 0; squelch.closing = 0;
        squelch.gate = outRate * 0.05;
        squelch.release = (outRate * gateSetting) / 100;
        squelch.level = std::pow(10.0, squelchdB / 10.0);
        agc.resize(outRate/5, outRate/20, 16384.0f);
        agc.setStepDownDelay((outRate * (gateSetting == 0 ? 1 : gateSetting))/100);
        agc.setGate(outRate * 0.05);
        agc.setThreshold(squelch.level*(1<<23));
        inputPower.resize(outRate * 0.01, 1e-10);
    }
    ~Channel() { delete filter; }

    void block(fftfilt::cmplx* side, int count, bool mono)
    {
        double l, r;
        for (int i = 0; i < count; i++) {
            if (mono) {
                l = squelch.open ? (side[i].real() + side[i].imag()) * 0.7 * gain : 0;
                payload.fixed_mono(l);
            } else {
                l = squelch.open ? side[i].real() * gain : 0;
                r = squelch.open ? side[i].imag() * gain : 0;
                payload.fixed_pair(l, r);
            }
        }
    }

    void sample(Complex& ci)
    {
        fftfilt::cmplx* side;
        double factor = 1.0, power;
        if (agcOn) { factor = agc.feedAndGetValue(ci); power = agc.getMagSq(); }
        else power = ci.real()*ci.real() + ci.imag()*ci.imag();
        inputPower.feed(power / (SDR_RX_SCALED*SDR_RX_SCALED));
        inMagsq = inputPower.average();
        spectrum.push_back(Sample(ci.real(), ci.imag()));
        squelch.step(inMagsq);

        if (format == LSB)
        {
            ci *= factor;
            const int count = filter->runSSB(ci, &side, false);
            block(side, count, false);
        }
        if (format == USB)
        {
            ci *= factor;
            const int count = filter->runSSB(ci, &side, true);
            block(side, count, false);
        }
        else if (format == LSB_MONO)
        {
            ci *= factor;
            const int count = filter->runSSB(ci, &side, false);
            block(side, count, true);
        }
        else if (format == USB_MONO)
        {
            ci *= factor;
            const int count = filter->runSSB(ci, &side, true);
            block(side, count, true);
        }
        else
        {
            if (squelch.open) payload.fixed_pair(ci.real() * gain, ci.imag() * gain);
            else payload.fixed_pair(0, 0);
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
    if (argc != 3) { std::fprintf(stderr, "usage: udpsrc_ssb_rec input.bin output.bin\n"); return 2; }
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
            if (fmt < LSB || fmt > USB_MONO) return 3;
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
            const int elem = d->format >= LSB_MONO ? 2 : 4;
            const int64_t k[2] = { (int64_t)d->spectrum.size(), (int64_t)(d->payload.bytes.size() / elem) };
            std::fwrite(k, 8, 2, out);
            if (!d->payload.bytes.empty()) std::fwrite(d->payload.bytes.data(), 1, d->payload.bytes.size(), out);
            for (int64_t i = 0; i < k[0]; i++) {
                const int16_t iq[2] = { (int16_t)d->spectrum[(size_t)i].real(), (int16_t)d->spectrum[(size_t)i].imag() };
                std::fwrite(iq, 2, 2, out);
            }
        } else if (!std::strcmp(cmd, "end") && d) {
            const int64_t tail[6] = { d->squelch.open ? 1 : 0, (int64_t)d->squelch.opening, (int64_t)d->squelch.closing, (int64_t)d->squelch.gate,
                                      (int64_t)d->squelch.release, (int64_t)d->filter->waiting() };
            std::fwrite(&d->inMagsq, 8, 1, out); std::fwrite(tail, 8, 6, out);
            std::fwrite(d->filter->design(), 8, 512, out);
        }
    }
    delete d;
    std::fclose(out);
    return 0;
}
