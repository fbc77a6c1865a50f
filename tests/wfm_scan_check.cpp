// Host check of sdrangel_amd/csrc/wfm_scan.hpp (built with plain g++ by tests/test_wfm_scan.py): the composed clamp operator
// and the last-open index scan against the serial loop of WFMDemod::feed, on random flag sequences cut into random tiles
// (the way the kernels cut a feed into threads, waves and blocks), including long runs that saturate at 0 and at the cap and
// non-integer rfBW / 10.
//   wfm_scan_check <seed> <rounds>     prints "ok <checked samples>" or the first mismatch, exit status 0 / 1
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "wfm_scan.hpp"

using namespace sdrx;

static uint64_t g_s;
static uint64_t rnd() { uint64_t z = (g_s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static int rnd_int(int lo, int hi) { return lo + (int)(rnd() % (uint64_t)(hi - lo + 1)); }

int main(int argc, char** argv)
{
    g_s = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int rounds = argc > 2 ? atoi(argv[2]) : 200;
    long checked = 0;
    const float bws[] = { 12500.0f, 12345.0f, 80000.0f, 80005.0f, 250000.0f, 15.0f, 7.0f, 100.0f, 199.0f, 1.0f };
    for (int r = 0; r < rounds; r++) {
        const float rf = bws[r % 10];
        const float cap_f = rf / 10, open_f = rf / 20;
        const int cap = wfm_counter_cap(cap_f);
        // the cap is where `state < cap_f` first fails
        if (cap < 0 || (float)cap < cap_f || (cap > 0 && !((float)(cap - 1) < cap_f))) { printf("cap %d wrong for %g\n", cap, (double)cap_f); return 1; }
        const int n = rnd_int(1, 6000) * (r % 7 == 0 ? 20 : 1);
        std::vector<uint8_t> flag((size_t)n);
        // runs of equal flags with lengths from 1 to beyond the cap, so that the counter saturates at both ends
        for (int i = 0; i < n;) {
            const int kind = rnd_int(0, 3);
            int len = kind == 0 ? 1 : kind == 1 ? rnd_int(1, 40) : kind == 2 ? rnd_int(1, cap + 2) : rnd_int(cap, 3 * cap + 10);
            const uint8_t f = (uint8_t)(rnd() & 1);
            for (; len > 0 && i < n; len--, i++) flag[(size_t)i] = kind == 0 ? (uint8_t)(rnd() & 1) : f;
        }
        const int s0 = rnd_int(0, cap);
        const bool mute = r % 11 == 5;
        // serial reference: the loop as the demodulator writes it
        std::vector<int> st((size_t)n), prev((size_t)n);
        {
            int s = s0, last = -1;
            for (int i = 0; i < n; i++) {
                if (flag[(size_t)i]) { if ((float)s < cap_f) s++; } else { if (s > 0) s--; }
                st[(size_t)i] = s;
                const bool open = (float)s > open_f && !mute;
                prev[(size_t)i] = last;
                if (open) last = i;
            }
        }
        // tiled scans: tiles of random sizes; per tile the composed map, an exclusive scan over the tiles, then each tile from
        // its start state -- with a second level of tiling inside (pairs, as a thread holds two samples)
        std::vector<int> cut{ 0 };
        while (cut.back() < n) cut.push_back(std::min(n, cut.back() + rnd_int(1, r % 3 == 0 ? 512 : 64)));
        const size_t nt = cut.size() - 1;
        std::vector<WfmClamp> tile(nt);
        for (size_t t = 0; t < nt; t++) {
            WfmClamp m = wfm_identity(cap);
            int i = cut[t];
            for (; i + 1 < cut[t + 1]; i += 2) m = wfm_compose(m, wfm_compose(wfm_step(flag[(size_t)i] != 0, cap), wfm_step(flag[(size_t)i + 1] != 0, cap)));
            if (i < cut[t + 1]) m = wfm_compose(m, wfm_step(flag[(size_t)i] != 0, cap));
            tile[t] = m;
        }
        std::vector<int> start(nt);
        {
            WfmClamp acc = wfm_identity(cap);
            for (size_t t = 0; t < nt; t++) { start[t] = wfm_apply(acc, s0); acc = wfm_compose(acc, tile[t]); }
            if (wfm_apply(acc, s0) != st[(size_t)n - 1]) { printf("round %d: end state %d != %d\n", r, wfm_apply(acc, s0), st[(size_t)n - 1]); return 1; }
        }
        std::vector<int> tile_last(nt, -1);
        std::vector<int> got_prev((size_t)n, -2);
        for (size_t t = 0; t < nt; t++) {
            WfmClamp acc = wfm_identity(cap);
            int last = -1;
            for (int i = cut[t]; i < cut[t + 1]; i++) {
                acc = wfm_compose(acc, wfm_step(flag[(size_t)i] != 0, cap));
                const int s = wfm_apply(acc, start[t]);
                if (s != st[(size_t)i]) { printf("round %d: state[%d] %d != %d (cap %d)\n", r, i, s, st[(size_t)i], cap); return 1; }
                const bool open = (float)s > open_f && !mute;
                got_prev[(size_t)i] = last;                   // in-tile exclusive max-scan; -1: from an earlier tile
                last = wfm_last_open(last, open ? i : -1);
                checked++;
            }
            tile_last[t] = last;
        }
        {
            int carry = -1;                                   // exclusive max-scan over the tiles
            for (size_t t = 0; t < nt; t++) {
                for (int i = cut[t]; i < cut[t + 1]; i++) {
                    const int p = wfm_last_open(carry, got_prev[(size_t)i]);
                    if (p != prev[(size_t)i]) { printf("round %d: prev[%d] %d != %d\n", r, i, p, prev[(size_t)i]); return 1; }
                }
                carry = wfm_last_open(carry, tile_last[t]);
            }
        }
    }
    printf("ok %ld\n", checked);
    return 0;
}
