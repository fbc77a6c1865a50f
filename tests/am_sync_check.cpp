// Host check of sdrangel_amd/csrc/am_sync_scan.hpp (built with plain g++ by tests/test_am_sync_host.py and by
// tests/golden/make_golden_am_sync.py): the cut of the synchronous-AM chain against what the reference recorded per open sample
// (tests/golden/am_sync_rec.cpp's trace): (re, im), m_pllFilt's output, (m_yRe, m_yIm) after m_pll.feed(), the demod value, and
// per filter output the sideband pair.
//   am_sync_check probe <rate> <trace.bin>
//       pll_phase_step (pll_math.hpp, the step the device walk runs) over the recorded loop input; prints
//       "probe <samples> <sat_hi> <sat_lo> <lock_up> <lock_down> <oscillator mismatches> <locked> <bits of freq>"
//   am_sync_check chain <rate> <sync> <seed> <trace.bin> <trace.bin.sb>
//       the open samples cut into random feeds (empty, one sample, B - 1, B, B + 1 among them), every stream kept as
//       [history | feed] across them exactly as the device kernels keep it: the prefilter's pairing order, the walk, the AGC terms as
//       a rounded prefix sum, the delay selection and every carry; prints "ok <samples> <blocks> <feeds>" or the first mismatch
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "am_sync_scan.hpp"

using namespace sdrx;

struct Cf { float x, y; };
struct Rec { float re, im, sr, si, yr, yi, dem; };

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static uint64_t g_s;
static uint64_t rnd() { uint64_t z = (g_s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }

template <class T> static bool load(const char* path, std::vector<T>& v)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / sizeof(T));
    const bool ok = v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size();
    std::fclose(f);
    return ok;
}

static int probe(int rate, const char* path)
{
    std::vector<Rec> tr;
    if (!load(path, tr)) { std::printf("cannot read %s\n", path); return 2; }
    const PllCfg k = ams_pll_design(rate);
    PllState st = PllState();
    PllProbe pr = PllProbe();
    long bad = 0;
    for (const Rec& r : tr) {
        float yr, yi;
        pll_phase_step(k, st, r.sr, r.si, &yr, &yi, &pr);
        if (bits(yr) != bits(r.yr) || bits(yi) != bits(r.yi)) bad++;
    }
    std::printf("probe %zu %ld %ld %ld %ld %ld %d %u\n", tr.size(), pr.sat_hi, pr.sat_lo, pr.lock_up, pr.lock_down, bad, pll_locked(k, st) ? 1 : 0, bits(st.freq));
    return 0;
}

static int chain(int rate, int sync, uint64_t seed, const char* path, const char* path_sb)
{
    std::vector<Rec> tr;
    std::vector<Cf> sb;
    if (!load(path, tr) || !load(path_sb, sb)) { std::printf("cannot read the trace\n"); return 2; }
    g_s = seed;
    const int B = ams_block(sync), hn = ams_agc_len(rate);
    float taps[AMS_PF_H + 1];
    ams_lowpass_design((double)rate, 200.0, taps);
    const PllCfg k = ams_pll_design(rate);
    // the carried state, as the device keeps it
    std::vector<Cf> xhist(AMS_PF_HIST, Cf{0.0f, 0.0f});
    std::vector<float> phist((size_t)hn, 0.0f), zhist((size_t)B, 0.0f);
    PllState st = PllState();
    int pend = 0;
    double total = 0.0;
    size_t at = 0, sb_at = 0;
    long blocks = 0, feeds = 0;
    const int pick[] = { 0, 1, 2, B - 1, B, B + 1, 99, 100, 101 };
    while (at < tr.size()) {
        int m = rnd() % 3 ? (int)(rnd() % (uint64_t)(B + B / 2)) : pick[rnd() % 9];
        if ((size_t)m > tr.size() - at) m = (int)(tr.size() - at);
        feeds++;
        std::vector<Cf> xc((size_t)m), pf((size_t)m), osc((size_t)m);
        for (int a = 0; a < m; a++) xc[(size_t)a] = Cf{tr[at + a].re, tr[at + a].im};
        // the prefilter, one open sample at a time and in any order
        for (int a = m - 1; a >= 0; a--) {
            pf[(size_t)a] = ams_prefilter<Cf>(taps, [&](int q) { return am_stream_at(xhist.data(), AMS_PF_HIST, xc.data(), (long)a - q); });
            if (bits(pf[(size_t)a].x) != bits(tr[at + a].sr) || bits(pf[(size_t)a].y) != bits(tr[at + a].si)) {
                std::printf("prefilter differs at open sample %zu\n", at + a); return 1;
            }
        }
        for (int a = 0; a < m; a++) {
            pll_phase_step(k, st, pf[(size_t)a].x, pf[(size_t)a].y, &osc[(size_t)a].x, &osc[(size_t)a].y, (PllProbe*)nullptr);
            if (bits(osc[(size_t)a].x) != bits(tr[at + a].yr) || bits(osc[(size_t)a].y) != bits(tr[at + a].yi)) {
                std::printf("oscillator differs at open sample %zu\n", at + a); return 1;
            }
        }
        // the blocks this feed completes: their outputs are the recording's (the transforms are device code)
        const int nb = ams_blocks(pend, m, B), no = nb * B;
        if (sb_at + (size_t)no > sb.size()) { std::printf("the recording has fewer filter outputs than the cut expects\n"); return 1; }
        for (int x = 0; x < nb; x++) {
            if (ams_block_source(pend, B, x, 0) != x * B - pend || ams_block_source(pend, B, x, B - 1) >= m) { std::printf("block source out of the feed\n"); return 1; }
        }
        const Cf* out = sb.data() + sb_at;
        std::vector<float> pw((size_t)no), zs((size_t)no);
        std::vector<double> term((size_t)no);
        for (int o = no - 1; o >= 0; o--) {
            pw[(size_t)o] = ams_magsq(out[o]);
            term[(size_t)o] = ams_agc_term(pw[(size_t)o], o >= hn ? ams_magsq(out[o - hn]) : phist[(size_t)o]);
        }
        double acc = total;
        for (int o = 0; o < no; o++) { acc += term[(size_t)o]; zs[(size_t)o] = ams_zsum(out[o], ams_u0(acc, hn)); }
        total = acc;
        auto zs_at = [&](int o) { return o < 0 ? zhist[(size_t)(B + o)] : zs[(size_t)o]; };
        for (int a = 0; a < m; a++) {
            const int o = ams_select_index(pend, a, B);
            if (o < -B + 1 || o >= no) { std::printf("selection out of range at open sample %zu\n", at + a); return 1; }
            const float dem = zs_at(o) * 4.0f;
            if (bits(dem) != bits(tr[at + a].dem)) { std::printf("demod differs at open sample %zu: %a against %a\n", at + a, dem, tr[at + a].dem); return 1; }
        }
        // the carries
        std::vector<Cf> xnext(AMS_PF_HIST);
        for (int i = 0; i < AMS_PF_HIST; i++) xnext[(size_t)i] = am_hist_next(xhist.data(), AMS_PF_HIST, xc.data(), m, i);
        std::vector<float> pnext((size_t)hn), znext((size_t)B);
        for (int i = 0; i < hn; i++) pnext[(size_t)i] = am_hist_next(phist.data(), hn, pw.data(), no, i);
        for (int i = 0; i < B; i++) znext[(size_t)i] = zs_at(no - B + i);
        xhist.swap(xnext); phist.swap(pnext); zhist.swap(znext);
        pend = ams_left(pend, m, B);
        at += (size_t)m; sb_at += (size_t)no; blocks += nb;
    }
    if (sb_at != sb.size()) { std::printf("the recording has %zu filter outputs, the cut %zu\n", sb.size(), sb_at); return 1; }
    std::printf("ok %zu %ld %ld\n", tr.size(), blocks, feeds);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && !std::strcmp(argv[1], "probe")) return probe(std::atoi(argv[2]), argv[3]);
    if (argc == 7 && !std::strcmp(argv[1], "chain")) return chain(std::atoi(argv[2]), std::atoi(argv[3]), std::strtoull(argv[4], 0, 10), argv[5], argv[6]);
    std::fprintf(stderr, "usage: am_sync_check probe <rate> <trace.bin> | chain <rate> <sync> <seed> <trace.bin> <trace.bin.sb>\n");
    return 2;
}
