// One rule for cutting an arena into arrays, run twice per layout (demod_bank.hpp): with a null base it only counts, which
// sizes the allocation; with a base it hands out the pointers.  Either way array k starts al(count * sizeof(T)) bytes behind
// array k-1, so the two runs cannot disagree.  Plain C++: tests/demod_carve_check.cpp compiles it without HIP.
#pragma once
#include <cstddef>

namespace sdrx {

struct Carver {
    char* base;                           // nullptr: count only
    size_t off = 0;                       // bytes handed out so far: the arena's size once the layout has run
    static constexpr size_t al(size_t v) { return (v + 255) & ~(size_t)255; }
    template <class T> T* take(size_t count)
    {
        T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += al(count * sizeof(T));
        return r;
    }
};

// a carried array lives in two sets of the same layout: read from the current one, written to the next
struct HistCarver {
    Carver cur, next;
    template <class T> void pair(const T*& from, T*& to, size_t count) { from = cur.take<T>(count); to = next.take<T>(count); }
};

} // namespace sdrx
