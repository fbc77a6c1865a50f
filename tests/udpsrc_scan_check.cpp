// Host check of sdrangel_amd/csrc/udpsrc_scan.hpp (built with plain g++ by tests/test_udpsrc_scan.py): the squelch of
// UDPSrc (calculateSquelch, udpsrc.h:238-278) as maps on one chain of positions, composed, against the literal automaton with
// its flag and two counters.
//   udpsrc_scan_check exhaustive            G, R in 0..6, every start state, every boolean string up to length 12: the maps
//                                           folded from the left, from the right and as a balanced tree
//   udpsrc_scan_check random <seed> <rounds>   long strings at G, R up to 5000 in the kernel's grouping (4 per lane, a
//                                           Hillis-Steele scan over 64 lanes, 4 waves per trip, the carried state), cut into feeds
//   udpsrc_scan_check agc <seed> <rounds>   MagAGC's four counters as UDPSrc sets them up -- gate, step-down delay and step length
//                                           three independent numbers, where SSB ties them to one -- as ssb_scan.hpp's three scans
//                                           (maps composed over random chunks in random association, applied to the carried
//                                           state) against the counters written with the reference's ifs
// prints "ok <checked>" or the first mismatch, exit status 0 / 1
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "udpsrc_scan.hpp"

using namespace sdrx;

static uint64_t g_s;
static uint64_t rnd() { uint64_t z = (g_s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static int rnd_int(int lo, int hi) { return lo + (int)(rnd() % (uint64_t)(hi - lo + 1)); }

// the literal automaton
struct Lit {
    bool open; int oc, cc, G, R;
    void step(bool above)
    {
        if (above) {
            if (G == 0) open = true;
            else if (oc < G) oc++;
            else { cc = R; open = true; }
        } else {
            if (G == 0) open = false;
            else if (cc > 0) cc--;
            else { oc = 0; open = false; }
        }
    }
};

static Lit lit_from(int p, int G, int R)
{
    Lit l; l.G = G; l.R = R;
    l.open = udp_sq_open(p, G); l.oc = udp_sq_open_count(p, G); l.cc = udp_sq_close_count(p, G);
    if (G == 0) { l.oc = 0; l.cc = 0; }                     // the stateless case: the counters stay where initSquelch(false) left them
    return l;
}
static bool same(const Lit& l, int p, int G)
{
    if (l.open != udp_sq_open(p, G)) return false;
    if (G == 0) return true;
    return l.oc == udp_sq_open_count(p, G) && l.cc == udp_sq_close_count(p, G);
}

static UdpSq tree(const std::vector<UdpSq>& m, int lo, int hi, int top)
{
    if (hi - lo == 1) return m[(size_t)lo];
    const int mid = (lo + hi) / 2;
    return udp_sq_compose(tree(m, lo, mid, top), tree(m, mid, hi, top), top);
}

static int exhaustive()
{
    long checked = 0;
    for (int G = 0; G <= 6; G++) for (int R = 0; R <= 6; R++) {
        const int Re = udp_sq_release(G, R), top = udp_sq_top(G, Re);
        for (int len = 0; len <= 12; len++) for (unsigned bitsv = 0; bitsv < (1u << len); bitsv++) {
            std::vector<UdpSq> m;
            for (int i = 0; i < len; i++) m.push_back(udp_sq_map((bitsv >> i) & 1, G, top));
            UdpSq left = udp_sq_identity(top), right = udp_sq_identity(top);
            for (int i = 0; i < len; i++) left = udp_sq_compose(left, m[(size_t)i], top);
            for (int i = len - 1; i >= 0; i--) right = udp_sq_compose(m[(size_t)i], right, top);
            const UdpSq bal = len ? tree(m, 0, len, top) : udp_sq_identity(top);
            for (int p0 = 0; p0 <= top; p0++) {
                Lit l = lit_from(p0, G, Re);
                int p = p0;
                for (int i = 0; i < len; i++) { l.step((bitsv >> i) & 1); p = udp_sq_step(p, (bitsv >> i) & 1, G, top); }
                if (!same(l, p, G) || udp_sq_apply(left, p0) != p || udp_sq_apply(right, p0) != p || udp_sq_apply(bal, p0) != p) {
                    printf("G %d R %d len %d string %x start %d: literal %d/%d/%d chain %d left %d right %d tree %d\n", G, R, len, bitsv, p0,
                           (int)l.open, l.oc, l.cc, p, udp_sq_apply(left, p0), udp_sq_apply(right, p0), udp_sq_apply(bal, p0));
                    return 1;
                }
                checked++;
            }
        }
    }
    printf("ok %ld\n", checked);
    return 0;
}

// one feed in the kernel's grouping; returns the positions after every sample
static void feed_cut(const std::vector<char>& above, int from, int n, int G, int top, int& carry, std::vector<int>& pos)
{
    for (int base = 0; base < n; base += 1024) {
        UdpSq lane_map[256], incl[256];
        for (int t = 0; t < 256; t++) {
            UdpSq m = udp_sq_identity(top);
            for (int k = 0; k < 4; k++) {
                const int i = base + t * 4 + k;
                if (i < n) m = udp_sq_compose(m, udp_sq_map(above[(size_t)(from + i)] != 0, G, top), top);
            }
            lane_map[t] = m;
        }
        for (int w = 0; w < 4; w++) {                       // Hillis-Steele over the wave's 64 lanes
            UdpSq cur[64];
            for (int l = 0; l < 64; l++) cur[l] = lane_map[w * 64 + l];
            for (int o = 1; o < 64; o *= 2) {
                UdpSq nxt[64];
                for (int l = 0; l < 64; l++) nxt[l] = l >= o ? udp_sq_compose(cur[l - o], cur[l], top) : cur[l];
                memcpy(cur, nxt, sizeof cur);
            }
            for (int l = 0; l < 64; l++) incl[w * 64 + l] = cur[l];
        }
        for (int t = 0; t < 256; t++) {
            const int w = t >> 6, l = t & 63;
            UdpSq pre = udp_sq_identity(top);
            for (int q = 0; q < w; q++) pre = udp_sq_compose(pre, incl[q * 64 + 63], top);
            const UdpSq ex = l == 0 ? udp_sq_identity(top) : incl[t - 1];
            int st = udp_sq_apply(udp_sq_compose(pre, ex, top), carry);
            for (int k = 0; k < 4; k++) {
                const int i = base + t * 4 + k;
                if (i < n) { st = udp_sq_step(st, above[(size_t)(from + i)] != 0, G, top); pos.push_back(st); }
            }
        }
        UdpSq all = incl[63];
        for (int q = 1; q < 4; q++) all = udp_sq_compose(all, incl[q * 64 + 63], top);
        carry = udp_sq_apply(all, carry);
    }
}

static int random_long(int rounds)
{
    long checked = 0;
    const int gates[] = { 0, 1, 2, 3, 80, 400, 1023, 1024, 4800, 5000 };
    for (int r = 0; r < rounds; r++) {
        const int G = gates[r % 10], R = r % 3 == 0 ? G : rnd_int(0, 5000);
        const int Re = udp_sq_release(G, R), top = udp_sq_top(G, Re);
        const int n = rnd_int(1, 6 * (G + Re + 400));
        std::vector<char> above((size_t)n);
        for (int i = 0; i < n;) {                           // runs on both sides of the gate and the release, and chatter
            const int kind = rnd_int(0, 3);
            int len = kind == 3 ? rnd_int(1, 40) : rnd_int(1, 2 * (G + Re) + 50);
            const bool v = rnd() & 1;
            for (; len > 0 && i < n; len--, i++) above[(size_t)i] = kind == 3 ? (char)(rnd() & 1) : (char)v;
        }
        const int p0 = r % 2 ? top : 0;                     // initSquelch(true) / initSquelch(false)
        Lit l = lit_from(p0, G, Re);
        int carry = p0;
        std::vector<int> pos;
        for (int at = 0; at < n;) {
            const int kind = rnd_int(0, 5);
            int m = kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? rnd_int(1, 40) : kind == 3 ? rnd_int(1, 3000) : rnd_int(1, n);
            if (m > n - at) m = n - at;
            feed_cut(above, at, m, G, top, carry, pos);
            at += m;
        }
        if ((int)pos.size() != n) { printf("round %d: %zu positions for %d samples\n", r, pos.size(), n); return 1; }
        for (int i = 0; i < n; i++) {
            l.step(above[(size_t)i] != 0);
            if (!same(l, pos[(size_t)i], G)) { printf("round %d G %d R %d sample %d: literal %d/%d/%d position %d\n", r, G, R, i, (int)l.open, l.oc, l.cc, pos[(size_t)i]); return 1; }
        }
        if (n > 0 && carry != pos[(size_t)n - 1]) { printf("round %d: carried state differs\n", r); return 1; }
        checked += n;
    }
    printf("ok %ld\n", checked);
    return 0;
}

template <class M, class C> static M fold(const std::vector<M>& m, int lo, int hi, C compose)
{
    if (hi - lo == 1) return m[(size_t)lo];
    const int mid = rnd_int(lo + 1, hi - 1);                // a random association
    return compose(fold(m, lo, mid, compose), fold(m, mid, hi, compose));
}

static int agc_counters(int rounds)
{
    long checked = 0;
    const int gates[] = { 0, 1, 5, 400 }, delays[] = { 1, 2, 80, 400 }, steps[] = { 1, 2, 50, 400 };
    for (int r = 0; r < rounds; r++) {
        const int gate = gates[rnd_int(0, 3)], sdd = delays[rnd_int(0, 3)], L = steps[rnd_int(0, 3)];
        const int n = rnd_int(1, 6 * (gate + sdd + L) + 200);
        std::vector<char> above((size_t)n);
        for (int i = 0; i < n;) {
            const int kind = rnd_int(0, 2);
            int len = kind == 2 ? rnd_int(1, 30) : rnd_int(1, 2 * (gate + sdd + L) + 20);
            const bool v = rnd() & 1;
            for (; len > 0 && i < n; len--, i++) above[(size_t)i] = kind == 2 ? (char)(rnd() & 1) : (char)v;
        }
        // the literal counters (agc.cpp:127-176), from the state resize() leaves
        int lg = 0, lc = 0, lu = 0, ld = L;
        SsbCounters st; st.g = 0; st.count = 0; st.ud.U = 0; st.ud.D = L;
        for (int at = 0; at < n;) {
            int m = rnd_int(1, 1500); if (m > n - at) m = n - at;
            std::vector<WfmClamp> gm, cm; std::vector<SsbPair> pm;
            int g = st.g, cnt = st.count; SsbUD ud = st.ud;
            for (int i = at; i < at + m; i++) {
                const bool ab = above[(size_t)i] != 0;
                // literal
                if (ab) { if (lg < gate) lg++; else lc = 0; } else { if (lc < sdd) lc++; lg = 0; }
                const bool lup = lc < sdd;
                if (lup) { ld = lu; if (lu < L) lu++; } else { lu = ld; if (ld > 0) ld--; }
                // the cut, stepped per sample from the chunk's start state
                const bool rst = ssb_reset(ab, g, gate);
                gm.push_back(ssb_gate_step(ab, gate)); g = wfm_apply(gm.back(), g);
                cm.push_back(ssb_count_step(rst, ab, sdd)); cnt = wfm_apply(cm.back(), cnt);
                const bool up = ssb_up(cnt, sdd);
                pm.push_back(ssb_pair_step(up, L)); ud = ssb_pair_apply(pm.back(), ud);
                if (g != lg || cnt != lc || up != lup || ud.U != lu || ud.D != ld) {
                    printf("round %d gate %d delay %d step %d sample %d: %d/%d %d/%d %d/%d %d/%d\n", r, gate, sdd, L, i, g, lg, cnt, lc, ud.U, lu, ud.D, ld);
                    return 1;
                }
            }
            // the chunk's composed maps carry the state to the next chunk
            st.g = wfm_apply(fold(gm, 0, m, [](WfmClamp a, WfmClamp b) { return wfm_compose(a, b); }), st.g);
            st.count = wfm_apply(fold(cm, 0, m, [](WfmClamp a, WfmClamp b) { return wfm_compose(a, b); }), st.count);
            st.ud = ssb_pair_apply(fold(pm, 0, m, [](SsbPair a, SsbPair b) { return ssb_pair_compose(a, b); }), st.ud);
            if (st.g != lg || st.count != lc || st.ud.U != lu || st.ud.D != ld) { printf("round %d: carried state differs after %d\n", r, at + m); return 1; }
            at += m;
            checked += m;
        }
    }
    printf("ok %ld\n", checked);
    return 0;
}

// udp_atan2f against the host's atan2f: products of two int16-sized factors as the discriminator forms them, fixed-point pairs
// and arbitrary bit patterns (zeros, subnormals, infinities, NaN).  Prints the count, how many differ and the largest distance in ulp.
static int arg_check(long rounds)
{
    long differ = 0, worst = 0;
    for (long i = 0; i < rounds; i++) {
        const uint64_t r = rnd();
        float y, x;
        if (i % 3 == 0) { const uint32_t a = (uint32_t)r, b = (uint32_t)(r >> 32); memcpy(&y, &a, 4); memcpy(&x, &b, 4); }
        else if (i % 3 == 1) { y = (float)(int32_t)(r & 0xffffffffu) * (1.0f / 65536.0f); x = (float)(int32_t)(r >> 32) * (1.0f / 65536.0f); }
        else {
            y = (float)((int)(r & 0xffff) - 32768) * (float)((int)((r >> 16) & 0xffff) - 32768);
            x = (float)((int)((r >> 32) & 0xffff) - 32768) * (float)((int)(r >> 48) - 32768) + y * 0.001f;
        }
        const float want = atan2f(y, x), got = udp_atan2f(y, x);
        if (want != want && got != got) continue;
        int32_t a, b; memcpy(&a, &want, 4); memcpy(&b, &got, 4);
        if (a == b) continue;
        differ++;
        if (a < 0) a = (int32_t)0x80000000u - a;
        if (b < 0) b = (int32_t)0x80000000u - b;
        const long d = labs((long)a - (long)b);
        if (want != want || got != got || d > worst) worst = (want != want || got != got) ? 1L << 40 : d;
    }
    printf("ok %ld %ld %ld\n", rounds, differ, worst);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 3 && !strcmp(argv[1], "arg")) { g_s = strtoull(argv[2], nullptr, 10); return arg_check(atol(argv[3])); }
    if (argc > 1 && !strcmp(argv[1], "exhaustive")) return exhaustive();
    if (argc > 3 && !strcmp(argv[1], "random")) { g_s = strtoull(argv[2], nullptr, 10); return random_long(atoi(argv[3])); }
    if (argc > 3 && !strcmp(argv[1], "agc")) { g_s = strtoull(argv[2], nullptr, 10); return agc_counters(atoi(argv[3])); }
    fprintf(stderr, "usage: udpsrc_scan_check exhaustive | random <seed> <rounds> | agc <seed> <rounds> | arg <seed> <rounds>\n");
    return 2;
}
