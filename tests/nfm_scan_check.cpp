// Host check of sdrangel_amd/csrc/nfm_scan.hpp (built with plain g++ by tests/test_nfm_scan.py): the cut of NFMDemod::feed's
// recurrences -- discriminator from neighbouring arguments, moving-average terms, the counter as composed clamp maps in the
// kernel's grouping (4 per lane, 1024 per trip), the delay-line stream with its clamped readBack, the compaction, the Bandpass
// over the compacted sequence, and the [history | feed] indexing across feeds -- against a serial loop that keeps the
// reference's containers (fill-up / roll moving average, DoubleBufferFIFO(24000) with its doubled array, Bandpass ring), on
// random power and argument sequences with bursts and exact zeros, cut into random feeds (empty and one-sample feeds included).
//   nfm_scan_check <seed> <rounds>     prints "ok <checked samples>" or the first mismatch, exit status 0 / 1
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "nfm_scan.hpp"

using namespace sdrx;

static uint64_t g_s;
static uint64_t rnd() { uint64_t z = (g_s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static int rnd_int(int lo, int hi) { return lo + (int)(rnd() % (uint64_t)(hi - lo + 1)); }

struct In { float raw, arg; };                             // |ci|^2 as the float sum of squares, atan2_approximation2(ci)
struct Out { int count; bool act; float y; };              // y: the Bandpass output
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// the serial loop, with the reference's containers
struct Serial {
    int gate; float level, fms, comp; bool mute; const float* taps;
    float prev = 0;
    float ma[NFM_MA]; int ma_num = 0; unsigned ma_idx = 0; double total = 0;
    std::vector<float> dl; int dl_w = 0, dl_cur = 0;
    int count = 0;
    float ring[AM_BP_TAPS]; int ptr = 0;
    Serial(int g, float l, float f, float c, bool m, const float* t) : gate(g), level(l), fms(f), comp(c), mute(m), taps(t), dl((size_t)(2 * NFM_DL), 0.0f)
    { memset(ring, 0, sizeof ring); }
    Out one(In s)
    {
        float dev = (float)((double)(s.arg - prev) / 3.14159265358979323846);
        prev = s.arg;
        if (dev < -1.0f) dev += 2.0f; else if (dev > 1.0f) dev -= 2.0f;
        const float demod = dev * fms;
        const float magsq = (float)((double)s.raw / (32768.0 * 32768.0));
        if (ma_num < NFM_MA) { ma[ma_num++] = magsq; total += magsq; }
        else { float& o = ma[ma_idx]; total += magsq - o; o = magsq; ma_idx = (ma_idx + 1) % NFM_MA; }
        const bool below = (float)(total / NFM_MA) < level;
        const float w = below ? 0.0f : demod * comp;
        dl[(size_t)dl_w] = w; dl[(size_t)(dl_w + NFM_DL)] = w; dl_cur = dl_w; dl_w = dl_w < NFM_DL - 1 ? dl_w + 1 : 0;
        if (below) { if (count > 0) count--; } else { if (count < 2 * gate) count++; }
        Out r; r.count = count; r.act = count > gate && !mute; r.y = 0;
        if (!r.act) return r;
        int delay = gate; if (delay > NFM_DL) delay = NFM_DL;
        const float x = dl[(size_t)(dl_cur + NFM_DL - delay)];
        float acc = 0; int a_ = ptr, b_ = ptr - 1, i;
        ring[ptr] = x;
        while (b_ < 0) b_ += AM_BP_TAPS;
        for (i = 0; i < AM_BP_H; i++) {
            acc += (ring[a_] + ring[b_]) * taps[i];
            a_++; while (a_ >= AM_BP_TAPS) a_ -= AM_BP_TAPS;
            b_--; while (b_ < 0) b_ += AM_BP_TAPS;
        }
        acc += ring[a_] * taps[i];
        ptr++; while (ptr >= AM_BP_TAPS) ptr -= AM_BP_TAPS;
        r.y = acc;
        return r;
    }
};

// the cut: per feed the passes of nfm_kernels.hpp, histories carried with am_hist_next
struct Cut {
    int gate, D; float level, fms, comp; bool mute; const float* taps;
    std::vector<float> mh, wh, xh;
    double total = 0; int count = 0; float prev = 0;
    Cut(int g, float l, float f, float c, bool m, const float* t) : gate(g), D(nfm_delay(g)), level(l), fms(f), comp(c), mute(m), taps(t),
        mh(NFM_MA, 0.0f), wh((size_t)D, 0.0f), xh(AM_BP_HIST, 0.0f) {}
    void feed(const In* s, int n, std::vector<Out>& out)
    {
        std::vector<float> msq((size_t)n), wraw((size_t)n), w((size_t)n), x;
        std::vector<double> tot((size_t)n);
        std::vector<int> cnt((size_t)n), aidx((size_t)n);
        for (int i = 0; i < n; i++) msq[(size_t)i] = nfm_magsq(s[i].raw);
        double t = total;
        for (int i = 0; i < n; i++) {
            wraw[(size_t)i] = nfm_demod(s[i].arg, i > 0 ? s[i - 1].arg : prev, fms) * comp;
            t += am_ma_term(msq[(size_t)i], am_stream_at(mh.data(), NFM_MA, (const float*)msq.data(), (long)i - NFM_MA));
            tot[(size_t)i] = t;
        }
        // the counter: trips of 1024, 4 samples per lane, the lanes' maps composed in order, applied to the carried state
        const int cap = 2 * gate;
        int carry = count, n_act = 0;
        for (int base = 0; base < n; base += 1024) {
            WfmClamp pre = wfm_identity(cap);
            for (int lane = 0; lane < 256; lane++) {
                int st = wfm_apply(pre, carry);
                WfmClamp m = wfm_identity(cap);
                for (int k = 0; k < 4; k++) {
                    const int i = base + lane * 4 + k;
                    if (i >= n) break;
                    const bool up = nfm_up(tot[(size_t)i], level);
                    m = wfm_compose(m, wfm_step(up, cap));
                    st = wfm_apply(wfm_step(up, cap), st);
                    cnt[(size_t)i] = st;
                    w[(size_t)i] = up ? wraw[(size_t)i] : 0.0f;
                    aidx[(size_t)i] = nfm_open(st, gate) && !mute ? n_act++ : -1;
                }
                pre = wfm_compose(pre, m);
            }
            carry = wfm_apply(pre, carry);
        }
        x.resize((size_t)n_act);
        for (int i = 0; i < n; i++)
            if (aidx[(size_t)i] >= 0) x[(size_t)aidx[(size_t)i]] = am_stream_at(wh.data(), D, (const float*)w.data(), (long)i - D);
        for (int i = 0; i < n; i++) {
            Out o; o.count = cnt[(size_t)i]; o.act = aidx[(size_t)i] >= 0; o.y = 0;
            if (o.act) {
                const int a = aidx[(size_t)i];
                o.y = am_bandpass(taps, [&](int k) { return am_stream_at(xh.data(), AM_BP_HIST, (const float*)x.data(), (long)a - k); });
            }
            out.push_back(o);
        }
        std::vector<float> mh2(NFM_MA), wh2((size_t)D), xh2(AM_BP_HIST);
        for (int i = 0; i < NFM_MA; i++) mh2[(size_t)i] = am_hist_next(mh.data(), NFM_MA, (const float*)msq.data(), n, i);
        for (int i = 0; i < D; i++) wh2[(size_t)i] = am_hist_next(wh.data(), D, (const float*)w.data(), n, i);
        for (int i = 0; i < AM_BP_HIST; i++) xh2[(size_t)i] = am_hist_next(xh.data(), AM_BP_HIST, (const float*)x.data(), n_act, i);
        mh.swap(mh2); wh.swap(wh2); xh.swap(xh2);
        if (n > 0) { total = tot[(size_t)n - 1]; prev = s[n - 1].arg; }
        count = carry;
    }
};

int main(int argc, char** argv)
{
    g_s = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int rounds = argc > 2 ? atoi(argv[2]) : 100;
    long checked = 0;
    float taps[AM_BP_H + 1];
    for (int i = 0; i <= AM_BP_H; i++) taps[i] = (float)((double)(rnd() % 2001) / 1000.0 - 1.0) / 151.0f;
    // gates around the scan's grouping, 0, and on both sides of the delay line's 24000 entries
    const int gates[] = { 0, 1, 3, 100, 480, 1023, 2400, NFM_DL - 1, NFM_DL, NFM_DL + 1, 28800 };
    for (int r = 0; r < rounds; r++) {
        const int gate = gates[r % 11];
        const float level = 1.0e-3f, scale = 32768.0f * 32768.0f;
        const bool mute = r % 13 == 12;
        const int n = gate >= 10000 ? rnd_int(2 * gate, 3 * gate) : rnd_int(1, 8 * (gate + 300));
        std::vector<In> s((size_t)n);
        // stretches above, below and around the level, with exact zeros, longer and shorter than gate and 2 * gate
        for (int i = 0; i < n;) {
            const int kind = gate >= 10000 && i < gate + 2000 ? 0 : rnd_int(0, 4);
            int len = kind == 4 ? rnd_int(1, 40) : rnd_int(1, 3 * gate + 50);
            for (; len > 0 && i < n; len--, i++) {
                const float u = (float)(rnd() % 100000) / 100000.0f;
                const float m = kind == 0 ? 0.05f + u : kind == 1 ? 1.0e-5f * u : kind == 2 ? level * (0.9f + 0.2f * u) : kind == 3 ? (rnd() % 3 ? 0.2f * u : 0.0f) : 0.0f;
                s[(size_t)i].raw = m * scale;
                s[(size_t)i].arg = m == 0.0f ? 0.0f : ((float)(rnd() % 200001) / 100000.0f - 1.0f) * 3.14159265f;
            }
        }
        const float fms = 192.0f, comp = 0.88059f;
        Serial ser(gate, level, fms, comp, mute, taps);
        Cut cut(gate, level, fms, comp, mute, taps);
        std::vector<Out> got;
        for (int pos = 0; pos < n;) {
            const int kind = rnd_int(0, 5);
            int m = kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? rnd_int(1, 40) : kind == 3 ? rnd_int(1, 2000) : rnd_int(1, n);
            if (m > n - pos) m = n - pos;
            cut.feed(s.data() + pos, m, got);
            pos += m;
        }
        if ((int)got.size() != n) { printf("round %d: %zu outputs for %d samples\n", r, got.size(), n); return 1; }
        long open = 0;
        for (int i = 0; i < n; i++) {
            const Out w = ser.one(s[(size_t)i]);
            const Out& g = got[(size_t)i];
            open += w.act;
            if (w.count != g.count || w.act != g.act || bits(w.y) != bits(g.y)) {
                printf("round %d gate %d sample %d: count %d/%d act %d/%d y %08x/%08x\n", r, gate, i, g.count, w.count, (int)g.act, (int)w.act, bits(g.y), bits(w.y));
                return 1;
            }
        }
        if (cut.total != ser.total || cut.count != ser.count || bits(cut.prev) != bits(ser.prev)) { printf("round %d: carried state differs\n", r); return 1; }
        if (gate >= 10000 && !mute && open == 0) { printf("round %d gate %d: never open\n", r, gate); return 1; }
        checked += n;
    }
    printf("ok %ld\n", checked);
    return 0;
}
