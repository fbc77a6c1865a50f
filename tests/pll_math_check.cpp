// pll_sinf / pll_cosf (sdrangel_amd/csrc/pll_math.hpp) against the host's sinf, cosf and sincosf.
//   pll_math_check <set> <seed> <n>      set: small (|x| < 7), mid (|x| < 3e6), exp (2^6 .. 2^125, both signs), special
// prints "ok <count> <differ> <worst distance in ulp>"; count is the number of comparisons' inputs (each input is compared with
// all three host routines).  NaN equals NaN.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "pll_math.hpp"

static uint64_t g_s;
static uint64_t rnd() { g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17; return g_s; }
static double unit() { return (double)(rnd() >> 11) / 9007199254740992.0; }

static long ordered(float v) { int32_t i; std::memcpy(&i, &v, 4); return i < 0 ? (long)INT32_MIN - i : i; }
static long dist(float a, float b)
{
    if (std::isnan(a) && std::isnan(b)) return 0;
    if (std::isnan(a) || std::isnan(b)) return 1L << 40;
    uint32_t x, y; std::memcpy(&x, &a, 4); std::memcpy(&y, &b, 4);
    if (x == y) return 0;
    const long d = ordered(a) - ordered(b);
    return d < 0 ? -d : (d == 0 ? 1 : d);                   // +0 against -0 counts as a difference
}

int main(int argc, char** argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: pll_math_check small|mid|exp|special seed n\n"); return 2; }
    const char* set = argv[1];
    g_s = 0x9E3779B97F4A7C15ull ^ (uint64_t)std::atoll(argv[2]) * 0x2545F4914F6CDD1Dull;
    long n = std::atol(argv[3]);
    std::vector<float> xs;
    if (!std::strcmp(set, "special")) {
        const uint32_t bits[] = { 0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x007fffffu, 0x807fffffu, 0x00800000u, 0x80800000u,
                                  0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7f800001u, 0x7f7fffffu, 0xff7fffffu,
                                  0x39800000u, 0x397fffffu, 0x3f490fdau, 0x3f490fdbu, 0x3f490fd9u, 0x42f00000u, 0x42efffffu, 0x42f00001u };
        for (uint32_t b : bits) { float v; std::memcpy(&v, &b, 4); xs.push_back(v); }
        for (int e = 0; e < 255; e++)                        // every exponent, three mantissas, both signs
            for (uint32_t m : { 0u, 0x400000u, 0x7fffffu })
                for (uint32_t sg : { 0u, 0x80000000u }) { const uint32_t b = sg | ((uint32_t)e << 23) | m; float v; std::memcpy(&v, &b, 4); xs.push_back(v); }
        n = (long)xs.size();
    }
    long differ = 0, worst = 0;
    for (long i = 0; i < n; i++) {
        float x;
        if (!xs.empty()) x = xs[(size_t)i];
        else if (!std::strcmp(set, "small")) x = (float)((unit() * 2.0 - 1.0) * 7.0);
        else if (!std::strcmp(set, "mid")) x = (float)((unit() * 2.0 - 1.0) * 3.0e6);
        else if (!std::strcmp(set, "exp")) {
            const uint32_t r = (uint32_t)rnd();
            const uint32_t b = (r & 0x807fffffu) | ((127u + 6u + (uint32_t)(rnd() % 120)) << 23);        // 2^6 .. 2^125
            std::memcpy(&x, &b, 4);
        } else return 2;
        const float s = sdrx::pll_sinf(x), c = sdrx::pll_cosf(x);
        float s2, c2;
        sincosf(x, &s2, &c2);
        const long d[4] = { dist(s, sinf(x)), dist(c, cosf(x)), dist(s, s2), dist(c, c2) };
        long m = 0;
        for (long v : d) if (v > m) m = v;
        if (m) differ++;
        if (m > worst) worst = m;
    }
    std::printf("ok %ld %ld %ld\n", n, differ, worst);
    return 0;
}
