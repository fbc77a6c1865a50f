// Host check of sdrangel_amd/csrc/demod_carve.hpp: one layout description of mixed element sizes, run in counting mode
// (null base, no memory behind it) and in placing mode at two bases.  The placed arrays must be 256-aligned relative to the
// base, in description order, non-overlapping, and end exactly where counting mode said.  Prints "ok <arrays checked>".
#include "demod_carve.hpp"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace sdrx;

struct Placed { char* p; size_t bytes; };

// the layout under test: element sizes 2, 4 and 8; counts 0, 1, 63 and 4112 (a work arena's 4096 + 16) among others
static size_t describe(Carver& k, std::vector<Placed>* out)
{
    const size_t counts[] = { 4112, 0, 1, 63, 4112 / 256 + 1, 256, 64, 128 };
    for (size_t n : counts) {
        int16_t* a = k.take<int16_t>(n);
        float* b = k.take<float>(n);
        double* c = k.take<double>(n);
        if (out) {
            out->push_back({ reinterpret_cast<char*>(a), n * 2 });
            out->push_back({ reinterpret_cast<char*>(b), n * 4 });
            out->push_back({ reinterpret_cast<char*>(c), n * 8 });
        } else if (a || b || c) { std::printf("counting mode handed out a pointer\n"); std::exit(1); }
    }
    return k.off;
}

#define CHECK(cond) do { if (!(cond)) { std::printf("failed: %s (array %zu, base + %zu)\n", #cond, i, shift); return 1; } } while (0)

int main()
{
    Carver count{nullptr};
    const size_t total = describe(count, nullptr);          // touches no memory: there is none
    size_t checked = 0;
    std::vector<char> arena(total + 4096 + 256, 0);
    char* aligned = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(arena.data()) + 255) & ~(uintptr_t)255);
    for (size_t shift : { (size_t)0, (size_t)4096 }) {
        char* base = aligned + shift;
        Carver place{base};
        std::vector<Placed> got;
        const size_t placed = describe(place, &got);
        size_t i = got.size();
        CHECK(placed == total);
        char* end = base;                                   // where the arrays so far end, rounded up as the carver rounds
        for (i = 0; i < got.size(); i++) {
            CHECK((size_t)(got[i].p - base) % 256 == 0);
            CHECK(got[i].p >= end);                         // in order, and clear of every earlier array
            CHECK(got[i].p == end);                         // and no gap beyond the rounding
            for (size_t j = 0; j < got[i].bytes; j++) got[i].p[j] = (char)(i + 1);      // inside the arena, or the vector's bounds are broken
            end = got[i].p + Carver::al(got[i].bytes);
            checked++;
        }
        CHECK(end == base + total);
        for (i = 0; i < got.size(); i++)
            for (size_t j = 0; j < got[i].bytes; j++) CHECK(got[i].p[j] == (char)(i + 1));  // nobody wrote over anybody
    }
    // the history flavour: both sets get the same offsets
    {
        size_t i = 0, shift = 0;
        HistCarver h{{aligned}, {aligned + 4096}};
        const float* from; float* to;
        const double* dfrom; double* dto;
        h.pair(from, to, 63);
        h.pair(dfrom, dto, 1);
        CHECK(reinterpret_cast<const char*>(from) == aligned && reinterpret_cast<char*>(to) == aligned + 4096);
        CHECK(reinterpret_cast<const char*>(dfrom) == aligned + 256 && reinterpret_cast<char*>(dto) == aligned + 4096 + 256);
        CHECK(h.cur.off == 512 && h.next.off == 512);
        checked += 2;
    }
    std::printf("ok %zu\n", checked);
    return 0;
}
