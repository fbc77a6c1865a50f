// Host check of sdrangel_amd/csrc/am_scan.hpp (built with plain g++ by tests/test_am_scan.py): the cut of
// AMDemod::processOneSample's recurrences -- moving-average terms, the gate's compaction, the AGC terms with their 0.003f
// prefix, the Bandpass over the compacted sequence, and the [history | feed] indexing across feeds -- against a serial loop
// that keeps the reference's containers (fill-up / roll moving average, delay line ring, AGC ring, Bandpass ring), on random
// power sequences with bursts and exact zeros, cut into random feeds (empty and one-sample feeds included).
//   am_scan_check <seed> <rounds>     prints "ok <checked samples>" or the first mismatch, exit status 0 / 1
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "am_scan.hpp"

using namespace sdrx;

static uint64_t g_s;
static uint64_t rnd() { uint64_t z = (g_s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static int rnd_int(int lo, int hi) { return lo + (int)(rnd() % (uint64_t)(hi - lo + 1)); }

struct Out { int count; bool act; float demod; };          // demod: after the Bandpass when enabled
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// the serial loop, with the reference's containers
struct Serial {
    int rate; float level; bool mute, bp; const float* taps;
    float ma[AM_MA]; int ma_num = 0; unsigned ma_idx = 0; double total = 0;
    std::vector<float> dl; int dl_w = 0, dl_cur = 0, dl_size;
    int count = 0;
    std::vector<double> hist; unsigned hi = 0; double sum;
    float ring[AM_BP_TAPS]; int ptr = 0;
    Serial(int r, float l, bool m, bool b, const float* t) : rate(r), level(l), mute(m), bp(b), taps(t), dl((size_t)(2 * (r / 5)), 0.0f), dl_size(r / 5),
        hist((size_t)(r / 10), am_agc_initial()), sum((double)(r / 10) * am_agc_initial()) { memset(ring, 0, sizeof ring); }
    Out one(float magsq)
    {
        if (ma_num < AM_MA) { ma[ma_num++] = magsq; total += magsq; }
        else { float& o = ma[ma_idx]; total += magsq - o; o = magsq; ma_idx = (ma_idx + 1) % AM_MA; }
        const double avg = total / AM_MA;
        dl[(size_t)dl_w] = magsq; dl[(size_t)(dl_w + dl_size)] = magsq; dl_cur = dl_w; dl_w = dl_w < dl_size - 1 ? dl_w + 1 : 0;
        if (avg < level) { if (count > 0) count--; } else { if (count < rate / 10) count++; }
        Out r; r.count = count; r.act = count >= rate / 20 && !mute; r.demod = 0;
        if (!r.act) return r;
        float d = sqrtf(dl[(size_t)(dl_cur + dl_size - rate / 20)]);
        if (d > 0) { double& o = hist[hi]; sum += (double)d - o; o = (double)d; hi = hi < hist.size() - 1 ? hi + 1 : 0; }
        const float a = (float)(sum / (double)hist.size());
        const float g = a > 0 ? a : 0;
        d = (d - g) / g;
        if (bp) {
            float acc = 0; int a_ = ptr, b_ = ptr - 1, i;
            ring[ptr] = d;
            while (b_ < 0) b_ += AM_BP_TAPS;
            for (i = 0; i < AM_BP_H; i++) {
                acc += (ring[a_] + ring[b_]) * taps[i];
                a_++; while (a_ >= AM_BP_TAPS) a_ -= AM_BP_TAPS;
                b_--; while (b_ < 0) b_ += AM_BP_TAPS;
            }
            acc += ring[a_] * taps[i];
            ptr++; while (ptr >= AM_BP_TAPS) ptr -= AM_BP_TAPS;
            d = acc;
        }
        r.demod = d;
        return r;
    }
};

// the cut: per feed the passes of am_kernels.hpp, histories carried with am_hist_next
struct Cut {
    int rate, D, H; float level; bool mute, bp; const float* taps;
    std::vector<float> mh, rh, dh; std::vector<double> vh;
    double total = 0, agc; int count = 0;
    Cut(int r, float l, bool m, bool b, const float* t) : rate(r), D(r / 20), H(r / 10), level(l), mute(m), bp(b), taps(t), mh(AM_MA, 0.0f), rh((size_t)D, 0.0f),
        dh(AM_BP_HIST, 0.0f), vh((size_t)H, am_agc_initial()), agc((double)H * am_agc_initial()) {}
    void feed(const float* msq, int n, std::vector<Out>& out)
    {
        std::vector<float> root((size_t)n), dem; std::vector<double> tot((size_t)n), vnew, S;
        std::vector<AmSlot> slot((size_t)n);
        double t = total;
        for (int i = 0; i < n; i++) {
            root[(size_t)i] = sqrtf(msq[i]);
            t += am_ma_term(msq[i], am_stream_at(mh.data(), AM_MA, msq, (long)i - AM_MA));
            tot[(size_t)i] = t;
        }
        AmGate g; g.count = count; g.n_act = 0; g.n_fed = 0;
        for (int i = 0; i < n; i++) {
            const float r = am_stream_at(rh.data(), D, (const float*)root.data(), (long)i - D);
            slot[(size_t)i] = am_gate_step(g, am_up(tot[(size_t)i], level), rate, mute, r);
            if (slot[(size_t)i].fed) vnew.push_back((double)r);
        }
        double s = agc;
        for (int j = 0; j < g.n_fed; j++) { s += am_agc_term(vnew[(size_t)j], am_stream_at(vh.data(), H, (const double*)vnew.data(), (long)j - H)); S.push_back(s); }
        dem.resize((size_t)g.n_act);
        for (int i = 0; i < n; i++) {
            const AmSlot& q = slot[(size_t)i];
            if (q.act_idx < 0) continue;
            const float r = am_stream_at(rh.data(), D, (const float*)root.data(), (long)i - D);
            const double sum = q.fed_cnt > 0 ? S[(size_t)q.fed_cnt - 1] : agc;
            const float a = (float)(sum / (double)H);
            const float gg = a > 0 ? a : 0;
            dem[(size_t)q.act_idx] = (r - gg) / gg;
        }
        for (int i = 0; i < n; i++) {
            const AmSlot& q = slot[(size_t)i];
            Out o; o.count = q.count; o.act = q.act_idx >= 0; o.demod = 0;
            if (o.act) {
                const int a = q.act_idx;
                o.demod = bp ? am_bandpass(taps, [&](int k) { return am_stream_at(dh.data(), AM_BP_HIST, (const float*)dem.data(), (long)a - k); }) : dem[(size_t)a];
            }
            out.push_back(o);
        }
        std::vector<float> mh2(AM_MA), rh2((size_t)D), dh2(AM_BP_HIST); std::vector<double> vh2((size_t)H);
        for (int i = 0; i < AM_MA; i++) mh2[(size_t)i] = am_hist_next(mh.data(), AM_MA, msq, n, i);
        for (int i = 0; i < D; i++) rh2[(size_t)i] = am_hist_next(rh.data(), D, (const float*)root.data(), n, i);
        for (int i = 0; i < H; i++) vh2[(size_t)i] = am_hist_next(vh.data(), H, (const double*)vnew.data(), g.n_fed, i);
        for (int i = 0; i < AM_BP_HIST; i++) dh2[(size_t)i] = am_hist_next(dh.data(), AM_BP_HIST, (const float*)dem.data(), g.n_act, i);
        mh.swap(mh2); rh.swap(rh2); dh.swap(dh2); vh.swap(vh2);
        if (n > 0) total = tot[(size_t)n - 1];
        if (g.n_fed > 0) agc = S.back();
        count = g.count;
    }
};

int main(int argc, char** argv)
{
    g_s = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int rounds = argc > 2 ? atoi(argv[2]) : 100;
    long checked = 0;
    float taps[AM_BP_H + 1];
    for (int i = 0; i <= AM_BP_H; i++) taps[i] = (float)((double)(rnd() % 2001) / 1000.0 - 1.0) / 151.0f;
    const int rates[] = { 1000, 1001, 1999, 3000, 8000, 44100 };
    for (int r = 0; r < rounds; r++) {
        const int rate = rates[r % 6];
        const float level = 1.0e-3f;
        const bool mute = r % 11 == 10, bp = r % 2 == 1;
        const int n = rnd_int(1, 8 * rate / 10) * (r % 5 == 0 ? 4 : 1);
        std::vector<float> msq((size_t)n);
        // stretches above, below and around the level, with exact zeros, longer and shorter than rate / 20 and rate / 10
        for (int i = 0; i < n;) {
            const int kind = rnd_int(0, 4);
            int len = kind == 4 ? rnd_int(1, 30) : rnd_int(1, rate / 4);
            for (; len > 0 && i < n; len--, i++) {
                const float u = (float)(rnd() % 100000) / 100000.0f;
                msq[(size_t)i] = kind == 0 ? 0.05f + u : kind == 1 ? 1.0e-5f * u : kind == 2 ? level * (0.9f + 0.2f * u) : kind == 3 ? (rnd() % 3 ? 0.2f * u : 0.0f) : 0.0f;
            }
        }
        Serial ser(rate, level, mute, bp, taps);
        Cut cut(rate, level, mute, bp, taps);
        std::vector<Out> got;
        for (int pos = 0; pos < n;) {
            const int kind = rnd_int(0, 5);
            int m = kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? rnd_int(1, 40) : kind == 3 ? rnd_int(1, rate / 10) : rnd_int(1, n);
            if (m > n - pos) m = n - pos;
            cut.feed(msq.data() + pos, m, got);
            pos += m;
        }
        if ((int)got.size() != n) { printf("round %d: %zu outputs for %d samples\n", r, got.size(), n); return 1; }
        for (int i = 0; i < n; i++) {
            const Out w = ser.one(msq[(size_t)i]);
            const Out& g = got[(size_t)i];
            if (w.count != g.count || w.act != g.act || bits(w.demod) != bits(g.demod)) {
                printf("round %d rate %d sample %d: count %d/%d act %d/%d demod %08x/%08x\n", r, rate, i, g.count, w.count, (int)g.act, (int)w.act, bits(g.demod), bits(w.demod));
                return 1;
            }
        }
        if (cut.total != ser.total || cut.agc != ser.sum || cut.count != ser.count) { printf("round %d: carried state differs\n", r); return 1; }
        checked += n;
    }
    printf("ok %ld\n", checked);
    return 0;
}
