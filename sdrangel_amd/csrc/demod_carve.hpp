// One rule for cutting an arena into arrays, run twice per layout (demod_bank.hpp, sdrx_backend.hip, sdrx_wfm.hip): with a
// null base it only counts, which sizes the allocation; with a base it hands out the pointers.  Either way array k starts
// al(count * sizeof(T)) bytes behind array k-1, so the two runs cannot disagree.  An array whose front carries state from
// feed to feed is taken with take_kept: both runs list {offset, kept bytes}, which is what a growing arena has to move
// (demod_grow_arena) and a reset has to clear (demod_clear_kept).  Plain C++: tests/demod_carve_check.cpp compiles it
// without HIP.
#pragma once
#include <cassert>
#include <cstddef>

namespace sdrx {

struct Carver {
    struct Kept { size_t off, bytes; };
    static constexpr int MAX_KEPT = 4;
    char* base;                           // nullptr: count only
    size_t off = 0;                       // bytes handed out so far: the arena's size once the layout has run
    Kept kept[MAX_KEPT] = {};             // the carried fronts, in description order
    int n_kept = 0;
    static constexpr size_t al(size_t v) { return (v + 255) & ~(size_t)255; }
    template <class T> T* take(size_t count)
    {
        T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += al(count * sizeof(T));
        return r;
    }
    template <class T> T* take_kept(size_t count, size_t kept_count)
    {
        assert(n_kept < MAX_KEPT && kept_count <= count);
        kept[n_kept++] = { off, kept_count * sizeof(T) };
        return take<T>(count);
    }
};

// a carried array lives in two sets of the same layout: read from the current one, written to the next
struct HistCarver {
    Carver cur, next;
    template <class T> void pair(const T*& from, T*& to, size_t count) { from = cur.take<T>(count); to = next.take<T>(count); }
};

} // namespace sdrx
