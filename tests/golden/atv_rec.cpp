// Recorder for tests/golden/atv_golden.npz: the reference's own ATVDemod (plugins/channelrx/demodatv/atvdemod.cpp and its moc output,
// compiled where they lie, strict IEEE, scalar) instantiated and driven through handleMessage, so that applySettings and feed are
// the reference's.  Stand-ins of our own (tests/golden/atv_stubs/) take the place of TVScreen -- the recording image -- and of
// DeviceSourceAPI, ThreadedBasebandSampleSink and DownChannelizer.  Built by tests/golden/make_golden_atv.py.
//
// Pinned as include/sdrx.h pins it: m_intAvgColIndex, which the constructor leaves unset, is set to 0 before the first sample; the
// screen counts as initialised and starts as zeros with a null row.
//
//   atv_rec in.bin out.bin      commands on stdin:
//     new <the 20 fields of sdrx_atv_cfg>     configureRF, configure, then the channelizer's notification
//     design                                  12 int32: the integers of sdrx_atv_design_t
//     feed n                                  n samples from in.bin, one feed() call per sample so that a render knows its index;
//                                             writes int64 n_events, int32 event[], int64 n_stored, frames, the screen, int64
//                                             n_scope, int16 scope[], uint32 state[28], int64 counters[6] (selectRow < 0, too large,
//                                             setDataColor < 0, too large, on a null row, scope Samples with an imaginary part;
//                                             since `new`)
#include <QObject>
#include <QString>
#include <QMutex>
#include <QElapsedTimer>
#include <emmintrin.h>
#include <unistd.h>
#include <math.h>
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "dsp/dsptypes.h"
#include "util/message.h"
#include "util/messagequeue.h"
#include "dsp/basebandsamplesink.h"
#include "channel/channelsinkapi.h"
#include "device/devicesourceapi.h"
#include "dsp/threadedbasebandsamplesink.h"
#include "dsp/downchannelizer.h"
#include "gui/tvscreen.h"
#define private public                      // the state and the design integers are private members
#include "dsp/nco.h"
#include "atvdemod.h"
#undef private

MESSAGE_CLASS_DEFINITION(DownChannelizer::MsgChannelizerNotification, Message)

// in place of sdrbase/channel/channelsinkapi.cpp, whose unique id needs QtNetwork: nothing here reads the id
ChannelSinkAPI::ChannelSinkAPI(const QString& name) : m_name(name), m_indexInDeviceSet(-1), m_uid(0) {}

namespace {

struct ScopeSink : public BasebandSampleSink {
    std::vector<int16_t> re;
    long long nonzero_im;
    ScopeSink() : nonzero_im(0) {}
    virtual void start() {}
    virtual void stop() {}
    virtual void feed(const SampleVector::const_iterator& begin, const SampleVector::const_iterator& end, bool)
    {
        for (SampleVector::const_iterator it = begin; it != end; ++it) { re.push_back((int16_t)it->real()); nonzero_im += it->imag() != 0; }
    }
    virtual bool handleMessage(const Message&) { return false; }
};

struct Rec {
    DeviceSourceAPI api;
    TVScreen screen;
    ScopeSink scope;
    ATVDemod* demod;
    int frames_cap;
    long at;
    std::vector<int32_t> events;
    std::vector<std::vector<uint8_t> > frames;
};

void on_render(void* p)
{
    Rec* r = (Rec*)p;
    if ((int)r->frames.size() < r->frames_cap) r->frames.push_back(r->screen.m_image);
    r->events.push_back((int32_t)r->at);
}

void drain(ATVDemod* d, MessageQueue* q)
{
    Message* m;
    while ((m = q->pop()) != 0) { d->handleMessage(*m); delete m; }
}

uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
template <class T> void put(FILE* f, const T* p, size_t n) { if (n && fwrite(p, sizeof(T), n, f) != n) { perror("write"); exit(2); } }

} // namespace

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: atv_rec in.bin out.bin < commands\n"); return 2; }
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) { perror("open"); return 2; }
    Rec* r = 0;
    MessageQueue queue;
    char word[32];
    while (scanf("%31s", word) == 1) {
        const std::string cmd(word);
        if (cmd == "new") {
            int in_rate, nco_freq, modulation, fft, decim, standard, n_lines, hsync, vsync, invert, scope, frames_cap;
            float rf_bw, rf_opp, dev, line, top, fps, ltop, lblack;
            if (scanf("%d %d %d %f %f %d %d %f %f %f %f %d %d %f %f %d %d %d %d %d", &in_rate, &nco_freq, &modulation, &rf_bw, &rf_opp, &fft, &decim, &dev,
                      &line, &top, &fps, &standard, &n_lines, &ltop, &lblack, &hsync, &vsync, &invert, &scope, &frames_cap) != 20) return 2;
            r = new Rec;
            r->frames_cap = frames_cap; r->at = 0;
            r->screen.m_onRender = on_render; r->screen.m_ctx = r;
            r->demod = new ATVDemod(&r->api);
            r->demod->m_intAvgColIndex = 0;
            r->demod->setTVScreen(&r->screen);
            if (scope) r->demod->setScopeSink(&r->scope);
            r->demod->configureRF(&queue, -(int64_t)nco_freq, (ATVDemod::ATVModulation)modulation, rf_bw, rf_opp, fft != 0, decim != 0, 0.0f, dev);
            r->demod->configure(&queue, line, top, fps, (ATVDemod::ATVStd)standard, n_lines, 0.0f, ltop, lblack, hsync != 0, vsync != 0, invert != 0, scope ? 1 : 0);
            drain(r->demod, &queue);                            // the rate is still 0: applySettings returns at once
            DownChannelizer::MsgChannelizerNotification note(in_rate, -(int64_t)nco_freq);
            r->demod->handleMessage(note);
            if (r->screen.m_resizes != 1) { fprintf(stderr, "resizeTVScreen ran %lld times\n", r->screen.m_resizes); return 3; }
        } else if (cmd == "design") {
            ATVDemod* d = r->demod;
            const int32_t v[12] = { d->m_runningPrivate.m_intNumberSamplePerLine, d->m_intNumberSamplePerTop, d->m_intNumberSamplePerLineSignals,
                                    d->m_intNumberSaplesPerHSync, d->m_intNumberOfSyncLines, d->m_intNumberOfBlackLines, d->m_intNumberOfEqLines,
                                    d->m_interleaved ? 1 : 0, d->m_runningPrivate.m_intTVSampleRate, r->screen.m_cols, r->screen.m_rows,
                                    d->m_nco.m_phaseIncrement };
            put(fo, v, 12);
        } else if (cmd == "feed") {
            long n;
            if (scanf("%ld", &n) != 1) return 2;
            std::vector<int16_t> iq((size_t)(2 * n));
            if (n && fread(iq.data(), 4, (size_t)n, fi) != (size_t)n) { fprintf(stderr, "short input\n"); return 2; }
            r->events.clear(); r->frames.clear(); r->scope.re.clear();
            SampleVector one(1);
            for (long j = 0; j < n; j++) {
                r->at = j;
                one[0] = Sample(iq[(size_t)(2 * j)], iq[(size_t)(2 * j + 1)]);
                r->demod->feed(one.begin(), one.end(), false);
            }
            ATVDemod* d = r->demod;
            const int64_t ne = (int64_t)r->events.size(), ns = (int64_t)r->frames.size(), nsc = (int64_t)r->scope.re.size();
            put(fo, &ne, 1); put(fo, r->events.data(), (size_t)ne);
            put(fo, &ns, 1);
            for (size_t i = 0; i < r->frames.size(); i++) put(fo, r->frames[i].data(), r->frames[i].size());
            put(fo, r->screen.m_image.data(), r->screen.m_image.size());
            put(fo, &nsc, 1); put(fo, r->scope.re.data(), (size_t)nsc);
            uint32_t st[28] = { (uint32_t)d->m_intImageIndex, (uint32_t)d->m_intSynchroPoints, (uint32_t)d->m_blnSynchroDetected,
                                (uint32_t)d->m_blnVerticalSynchroDetected, (uint32_t)d->m_intColIndex, (uint32_t)d->m_intSampleIndex,
                                (uint32_t)d->m_intRowIndex, (uint32_t)d->m_intLineIndex, (uint32_t)d->m_intAvgColIndex, (uint32_t)r->screen.m_row,
                                bits(d->m_fltAmpLineAverage), bits(d->m_fltEffMin), bits(d->m_fltEffMax), bits(d->m_fltAmpMin), bits(d->m_fltAmpMax),
                                bits(d->m_fltAmpDelta) };
            for (int i = 0; i < 6; i++) { st[16 + i] = bits(d->m_fltBufferI[i]); st[22 + i] = bits(d->m_fltBufferQ[i]); }
            put(fo, st, 28);
            const int64_t counters[6] = { r->screen.m_rowNeg, r->screen.m_rowBig, r->screen.m_colNeg, r->screen.m_colBig, r->screen.m_nullRow, r->scope.nonzero_im };
            put(fo, counters, 6);
        } else {
            fprintf(stderr, "unknown command %s\n", word);
            return 2;
        }
    }
    fclose(fo);
    return 0;
}
