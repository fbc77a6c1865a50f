// Host check of the cut in sdrangel_amd/csrc/ssb_scan.hpp: the four MagAGC counters (agc.cpp:127-176) as three scans of
// composed maps against the serial loop written with plain ifs, the spectrum-group index arithmetic against a counter, and
// the delay-line index against a DoubleBufferFIFO-shaped array.
//   ssb_scan_check SEED ROUNDS   ->  "ok <samples checked>"
// Each round draws hn from {2, 16, 6144}, gate from {0, small, around hn}, a carried state, an above/below sequence made of
// runs on both sides of gate and hn, and a chunking: fixed chunk sizes with the boundary at every offset, or random chunks.
#include "ssb_scan.hpp"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace sdrx;

static uint64_t rng_state;
static uint64_t rnd()
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint64_t)(hi - lo + 1)); }

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s line %d (round %d)\n", #c, __LINE__, round_no); return 1; } } while (0)
static int round_no;

// agc.cpp:127-176 with its own ifs; returns the mode (count < stepDownDelay) and leaves the counters stepped
struct Serial { int gc, count, up, down; };
static bool serial_step(Serial& s, bool above, int gate, int hn, int L, int* up_old, int* down_old)
{
    if (above) { if (s.gc < gate) s.gc++; else s.count = 0; }
    else { if (s.count < hn) s.count++; s.gc = 0; }
    *up_old = s.up; *down_old = s.down;
    if (s.count < hn) { s.down = s.up; if (s.up < L) s.up++; return true; }
    s.up = s.down; if (s.down > 0) s.down--; return false;
}

// one chunk [a, b) by the cut: per-sample maps, inclusive prefix compositions applied to the carried state
static void chunk_by_scan(const std::vector<char>& above, int a, int b, int gate, int hn, SsbCounters& carry,
                          std::vector<SsbCounters>& after, std::vector<SsbUD>& was, std::vector<char>& mode)
{
    const int L = hn / 2, n = b - a;
    std::vector<int> g((size_t)n), cnt((size_t)n);
    WfmClamp acc = wfm_identity(gate);
    for (int i = 0; i < n; i++) { acc = wfm_compose(acc, ssb_gate_step(above[(size_t)(a + i)], gate)); g[(size_t)i] = wfm_apply(acc, carry.g); }
    acc = wfm_identity(hn);
    for (int i = 0; i < n; i++) {
        const bool rst = ssb_reset(above[(size_t)(a + i)], i ? g[(size_t)i - 1] : carry.g, gate);
        acc = wfm_compose(acc, ssb_count_step(rst, above[(size_t)(a + i)], hn));
        cnt[(size_t)i] = wfm_apply(acc, carry.count);
    }
    SsbPair pacc = ssb_pair_identity(L);
    SsbUD prev = carry.ud;
    for (int i = 0; i < n; i++) {
        const bool up = ssb_up(cnt[(size_t)i], hn);
        pacc = ssb_pair_compose(pacc, ssb_pair_step(up, L));
        const SsbUD now = ssb_pair_apply(pacc, carry.ud);
        SsbCounters s; s.g = g[(size_t)i]; s.count = cnt[(size_t)i]; s.ud = now;
        after[(size_t)(a + i)] = s; was[(size_t)(a + i)] = prev; mode[(size_t)(a + i)] = up;
        prev = now;
    }
    if (n > 0) carry = after[(size_t)(b - 1)];
}

int main(int argc, char** argv)
{
    const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
    const int rounds = argc > 2 ? std::atoi(argv[2]) : 30;
    rng_state = seed;
    long checked = 0;
    static const int HN[3] = { 2, 16, 6144 };
    for (round_no = 0; round_no < rounds; round_no++) {
        const int hn = HN[round_no % 3], L = hn / 2;
        const int gsel = (round_no / 3) % 4;
        const int gate = gsel == 0 ? 0 : gsel == 1 ? rnd_in(1, 5) : gsel == 2 ? rnd_in(hn / 2, hn + 3) : rnd_in(1, 300);
        const int n = hn == 6144 ? 60000 : 4000;
        std::vector<char> above((size_t)n);
        for (int i = 0; i < n;) {
            // runs on both sides of the gate and of hn, and single samples
            const int kind = rnd_in(0, 5);
            int len = kind == 0 ? 1 : kind == 1 ? rnd_in(1, gate + 2) : kind == 2 ? rnd_in(gate, 2 * gate + 3) : kind == 3 ? rnd_in(1, L + 2) : kind == 4 ? rnd_in(hn - 1, hn + L + 5) : rnd_in(1, 8);
            const char v = (char)(rnd() & 1);
            for (; len > 0 && i < n; len--) above[(size_t)i++] = v;
        }
        // a carried state, reachable or not: the maps must be right on all of [0, gate] x [0, hn] x [0, L]^2
        Serial s0; s0.gc = rnd_in(0, gate); s0.count = (round_no & 1) ? rnd_in(0, hn) : 0; s0.up = (round_no & 2) ? rnd_in(0, L) : 0; s0.down = (round_no & 2) ? rnd_in(0, L) : L;
        // serial reference
        std::vector<Serial> ref((size_t)n); std::vector<int> ruo((size_t)n), rdo((size_t)n); std::vector<char> rmode((size_t)n);
        Serial s = s0;
        for (int i = 0; i < n; i++) { rmode[(size_t)i] = serial_step(s, above[(size_t)i], gate, hn, L, &ruo[(size_t)i], &rdo[(size_t)i]); ref[(size_t)i] = s; }
        // ssb_counters_step is the same serial loop
        {
            SsbCounters t; t.g = s0.gc; t.count = s0.count; t.ud.U = s0.up; t.ud.D = s0.down;
            for (int i = 0; i < n; i++) {
                SsbUD w;
                const bool up = ssb_counters_step(t, above[(size_t)i], gate, hn, &w);
                CHECK(up == (bool)rmode[(size_t)i] && t.g == ref[(size_t)i].gc && t.count == ref[(size_t)i].count && t.ud.U == ref[(size_t)i].up && t.ud.D == ref[(size_t)i].down);
                CHECK(w.U == ruo[(size_t)i] && w.D == rdo[(size_t)i]);
            }
        }
        // chunkings: a fixed chunk with the first boundary at every offset, then random chunks
        const int chunk = hn == 6144 ? 1024 : 7;
        const int n_off = hn == 6144 ? 3 : chunk;              // the long rounds take three offsets drawn at random
        for (int t = 0; t <= n_off; t++) {
            std::vector<SsbCounters> after((size_t)n); std::vector<SsbUD> was((size_t)n); std::vector<char> mode((size_t)n);
            SsbCounters carry; carry.g = s0.gc; carry.count = s0.count; carry.ud.U = s0.up; carry.ud.D = s0.down;
            int a = 0;
            const int off = t == n_off ? -1 : (hn == 6144 ? rnd_in(0, chunk - 1) : t);
            while (a < n) {
                int len = off < 0 ? rnd_in(0, 3000) : (a == 0 && off > 0 ? off : chunk);
                if (a + len > n) len = n - a;
                chunk_by_scan(above, a, a + len, gate, hn, carry, after, was, mode);
                a += len;
            }
            for (int i = 0; i < n; i++) {
                CHECK(after[(size_t)i].g == ref[(size_t)i].gc);
                CHECK(after[(size_t)i].count == ref[(size_t)i].count);
                CHECK(after[(size_t)i].ud.U == ref[(size_t)i].up && after[(size_t)i].ud.D == ref[(size_t)i].down);
                CHECK((bool)mode[(size_t)i] == (bool)rmode[(size_t)i]);
                CHECK(was[(size_t)i].U == ruo[(size_t)i] && was[(size_t)i].D == rdo[(size_t)i]);
                // the factor and the step value from the cut's (was, now, mode) against the branches of agc.cpp
                const double sd = 1.0 / L, u0 = 3.25;
                double want;
                if (rmode[(size_t)i]) want = ruo[(size_t)i] < L ? u0 * ssb_smootherstep((float)(ref[(size_t)i].up * sd)) : u0;
                else want = rdo[(size_t)i] > 0 ? u0 * ssb_smootherstep((float)(ref[(size_t)i].down * sd)) : 0.0;
                CHECK(ssb_agc_value(mode[(size_t)i], was[(size_t)i], after[(size_t)i].ud, L, sd, u0) == want);
                checked++;
            }
        }
        // composition is associative on random triples of pair maps, applied to every state when L is small
        for (int t = 0; t < 200; t++) {
            SsbPair m[3];
            for (auto& q : m) { q = ssb_pair_identity(L); for (int k = rnd_in(0, 4); k > 0; k--) q = ssb_pair_compose(q, ssb_pair_step(rnd() & 1, L)); }
            const SsbPair left = ssb_pair_compose(ssb_pair_compose(m[0], m[1]), m[2]), right = ssb_pair_compose(m[0], ssb_pair_compose(m[1], m[2]));
            for (int k = 0; k < 20; k++) {
                SsbUD x; x.U = rnd_in(0, L); x.D = rnd_in(0, L);
                const SsbUD serial = ssb_pair_apply(m[2], ssb_pair_apply(m[1], ssb_pair_apply(m[0], x)));
                const SsbUD a1 = ssb_pair_apply(left, x), a2 = ssb_pair_apply(right, x);
                CHECK(a1.U == serial.U && a1.D == serial.D && a2.U == serial.U && a2.D == serial.D);
            }
        }
        // spectrum groups: closes by ssb_first_close / ssb_closes against the counter itself, across feeds
        {
            const int decim = 1 << rnd_in(0, 7);
            unsigned usc = (unsigned)rnd_in(0, 1000);
            if (round_no % 5 == 0) usc = 0;
            for (int f = 0; f < 50; f++) {
                const int len = rnd_in(0, 3 * decim + 2);
                const int i0 = ssb_first_close(usc, decim), ncl = ssb_closes(len, i0, decim);
                int q = 0;
                unsigned u = usc;
                for (int i = 0; i < len; i++) if (!(u++ & (unsigned char)(decim - 1))) { CHECK(i == i0 + q * decim); q++; }
                CHECK(q == ncl);
                usc = u;
            }
        }
    }
    // delay line: a DoubleBufferFIFO(96000)-shaped array (doubled, write index, current index, readBack's clamp), read before
    // the write as ssbdemod.cpp:217-219 does, against w[j - 1 - ssb_delay(hn)] with the stream before the start taken as 0
    {
        static const int DELAYS[6] = { 2, 16, 6144, 95999, 96000, 98304 };
        for (int hn : DELAYS) {
            const int size = SSB_DL;
            std::vector<int> data((size_t)(2 * size), 0);
            int wr = 0, cur = 0;
            const int D = ssb_delay(hn);
            for (int j = 0; j < 200000; j++) {
                int delay = hn; if (delay > size) delay = size;
                const int got = data[(size_t)(cur + size - delay)];
                const long src = (long)j - 1 - D;
                CHECK(got == (src < 0 ? 0 : (int)src + 1));          // w[k] is written as k + 1
                data[(size_t)wr] = j + 1; data[(size_t)(wr + size)] = j + 1; cur = wr;
                if (wr < size - 1) wr++; else wr = 0;
                checked++;
            }
        }
    }
    std::printf("ok %ld\n", checked);
    return 0;
}
