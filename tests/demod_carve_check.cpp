// Host check of sdrangel_amd/csrc/demod_carve.hpp: one layout description of mixed element sizes, run in counting mode
// (null base, no memory behind it) and in placing mode at two bases.  The placed arrays must be 256-aligned relative to the
// base, in description order, non-overlapping, and end exactly where counting mode said.  Then a layout with kept ranges
// (take_kept) at two capacities: the same list either way, each range the front of its array, and a move between the two
// arenas that carries the ranges and nothing else.  Prints "ok <arrays checked>".
#include "demod_carve.hpp"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// a work arena in the shape of the back-end's: two arrays whose front carries state across feeds, between plain ones
struct Work { float* mixed; double* res; int16_t* out; float* tail; };
constexpr size_t KEEP_RES = 1024, KEEP_TAIL = 512;
static void describe_kept(Carver& k, size_t cap, Work& u)
{
    u.mixed = k.take<float>(256 + cap);
    u.res = k.take_kept<double>(cap + 1024 + KEEP_RES, KEEP_RES);
    u.out = k.take<int16_t>(cap + 8);
    u.tail = k.take_kept<float>((cap / KEEP_TAIL + 3) * KEEP_TAIL, KEEP_TAIL);
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
    // kept ranges: counting and placing record the same list, every range is the front of its array, and moving the ranges
    // from an arena laid out at one capacity into a zeroed one laid out at another carries them and nothing else
    {
        size_t i = 0, shift = 0;
        const size_t caps[2] = { 4096, 8192 };
        Carver placed[2] = { {nullptr}, {nullptr} };
        std::vector<char> mem[2];
        for (int a = 0; a < 2; a++) {
            Carver cnt{nullptr};
            Work none{};
            describe_kept(cnt, caps[a], none);
            CHECK(cnt.n_kept == 2 && !none.mixed && !none.res && !none.out && !none.tail);
            mem[a].assign(cnt.off + 256, 0);
            char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(mem[a].data()) + 255) & ~(uintptr_t)255);
            Carver& k = placed[a];
            k = Carver{base};
            Work u{};
            describe_kept(k, caps[a], u);
            CHECK(k.off == cnt.off && k.n_kept == cnt.n_kept);
            const char* arrays[2] = { reinterpret_cast<char*>(u.res), reinterpret_cast<char*>(u.tail) };
            const size_t bytes[2] = { (caps[a] + 1024 + KEEP_RES) * sizeof(double), (caps[a] / KEEP_TAIL + 3) * KEEP_TAIL * sizeof(float) };
            const size_t keep[2] = { KEEP_RES * sizeof(double), KEEP_TAIL * sizeof(float) };
            for (i = 0; i < 2; i++) {
                CHECK(k.kept[i].off == cnt.kept[i].off && k.kept[i].bytes == cnt.kept[i].bytes);
                CHECK(base + k.kept[i].off == arrays[i]);          // the front of its array
                CHECK(k.kept[i].bytes == keep[i] && k.kept[i].bytes <= bytes[i]);
                CHECK(k.kept[i].off + k.kept[i].bytes <= k.off);
                checked++;
            }
        }
        // the old arena holds no zero byte anywhere; the new one starts zeroed, as a grown arena does
        char* from = placed[0].base; char* to = placed[1].base;
        for (size_t j = 0; j < placed[0].off; j++) from[j] = (char)(1 + j % 251);
        for (i = 0; i < 2; i++) {
            CHECK(placed[0].kept[i].bytes == placed[1].kept[i].bytes);
            std::memcpy(to + placed[1].kept[i].off, from + placed[0].kept[i].off, placed[1].kept[i].bytes);
        }
        size_t j = 0;
        for (i = 0; i < 2; i++) {
            const Carver::Kept& o = placed[0].kept[i]; const Carver::Kept& n = placed[1].kept[i];
            for (; j < n.off; j++) CHECK(to[j] == 0);               // nothing else arrived
            for (; j < n.off + n.bytes; j++) CHECK(to[j] == from[o.off + (j - n.off)]);
            checked++;
        }
        for (; j < placed[1].off; j++) CHECK(to[j] == 0);
    }
    std::printf("ok %zu\n", checked);
    return 0;
}
