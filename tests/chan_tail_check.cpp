// Checks the array-history side of the lowering (MX_TAIL_BIT, sdrangel_amd/csrc/chan_lower.cpp) on host, for tests/test_chan_tails.py.
// stdin, one bank per line:  engine lds_kb max_levels in_rate n_ch  then n_ch x (channel id, rate, centre)   (as tests/chan_lower_check.cpp)
// stdout, one JSON object per bank: {"error": planner error, "lower": lowering error, "bad": [first problems found],
// "mx_passes" / "passes", "arrays": arrays below the roots of lean passes, "tails": tail jobs, "counts": tail jobs with 4, 6, 8, 10, 12
// arrays, "classes": tail jobs per epilogue class, "roots": lean subtrees with root arms E+O, E+A, E+O+A}.
//
// tree_mx_kernel.hpp keeps no history walk: the wave that runs a tail job copies slot -> head and tail -> slot for the job's
// arrays, from the job's own words.  What is checked, for every pass the lean kernel runs, restating the kernel's arithmetic
// (head = first child's base + 256 - PO, arrays PO apart, slots from 4 * (store_base + 16 * first) on, 64 bytes apart):
//   * every array a level produces belongs to exactly one tail job, and the tail bit sits on nothing else: the last job of an entry
//     with arms, whose own stores (the lanes with n16 >= 12) are the last 16 dwords of each of its arrays;
//   * the head the job restores is the first 16 dwords of the array's window, the slot it uses is the array's own
//     (TkArray::store = store_base + 16 * array index), and both lie inside the pass's LDS;
//   * no job of the level reads a head or a slot, none but the tail job writes an array's tail, and no job writes a head;
//   * the root arms' slots are the first ones, in arm order.
#include "chan_plan.hpp"
#include "chan_lower.hpp"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace sdrx;

namespace {

std::vector<std::string> bad;
void fail(const std::string& s) { if (bad.size() < 8) bad.push_back(s); }

// Lane spans of the kernel's job accesses (tests/chan_lower_check.cpp), the window's cut to the bytes that count: a block's load
// covers 64 entries, of which the first 15 + 24 carry a tap (hb_mfma.hpp, order 48); the rest meet zero taps.  The last block
// of an array needs exactly the array's end, and its load runs 48 don't-care bytes on, into whatever lies behind.
constexpr int WIN_SPAN = 32 * 15 + 2 * (15 + 24 + 1), CEN_SPAN = 32 * 15 + 8 * 3 + 12, OUT_SPAN = 16 * 15 + 4 * 3 + 4;

struct Range { long lo, hi; int job; };
bool meet(const Range& a, const Range& b) { return a.lo < b.hi && b.lo < a.hi; }

struct Stats { int arrays = 0, tails = 0, counts[5] = { 0, 0, 0, 0, 0 }, classes[MX_CLASSES] = { 0, 0, 0 }, roots[4] = { 0, 0, 0, 0 }; };

void check_level(const TkSubtree& st, const TkArray* arr, const TkLJob* jobs, int l, Stats& s)
{
    const TkLevel& lv = st.lv[l];
    const int PI = mx_pitch(l), PO = mx_pitch(l + 1);
    const std::string where = "level " + std::to_string(l);
    std::vector<int> owner((size_t)lv.arr_cnt, 0);
    std::vector<Range> reads, writes, heads, tails, slots;
    for (int q = 0; q < lv.n_mjobs; q++) {
        const TkLJob& r = jobs[q];
        const int f[2] = { mx_flags(r.meta, 0), mx_flags(r.meta, 1) };
        const int n = mx_arm_arrays(f[0]) + mx_arm_arrays(f[1]);
        for (int b : { r.b, r.b + PI }) reads.push_back(Range{ b, (long)b + WIN_SPAN, q });
        for (int c : { r.c, r.c + PI }) reads.push_back(Range{ c, (long)c + CEN_SPAN, q });
        for (int k = 0; k < 2; k++)
            for (int a = 0; a < mx_arm_arrays(f[k]); a++) writes.push_back(Range{ r.o[k] + a * PO, (long)r.o[k] + a * PO + OUT_SPAN, q });
        const bool last = r.out0 == lv.nout - 256;
        if (mx_tail(r.meta) != (last && n > 0)) { fail(where + ": tail bit on the wrong job"); continue; }
        if (!mx_tail(r.meta)) {
            if ((uint32_t)r.meta >> 17) fail(where + ": history words on a job that is no tail job");
            continue;
        }
        s.tails++;
        s.classes[mx_class(r.meta)]++;
        if (mx_tail_count(r.meta) != n || n < 4 || n > 12 || n % 2) { fail(where + ": array count of a tail job"); continue; }
        s.counts[n / 2 - 2]++;
        // what the kernel forms
        const int head = (f[0] ? r.o[0] : r.o[1]) + 256 - PO, first = mx_tail_first(r.meta);
        const int slot = 4 * (st.store_base + 16 * first);
        if (first < lv.arr_base || first + n > lv.arr_base + lv.arr_cnt) { fail(where + ": tail job names arrays of another level"); continue; }
        for (int a = 0; a < n; a++) {
            const TkArray& t = arr[first + a];
            if (4 * t.off != head + a * PO || 4 * t.len != PO) fail(where + ": restored head is not the array's window start");
            if (4 * t.store != slot + 64 * a || t.store != st.store_base + 16 * (first + a)) fail(where + ": derived slot is not the array's");
            if (slot + 64 * a < 0 || slot + 64 * (a + 1) > 4 * st.lds_dwords) fail(where + ": slot outside the pass's LDS");
            owner[(size_t)(first + a - lv.arr_base)]++;
            heads.push_back(Range{ head + a * PO, (long)head + a * PO + 64, q });
            tails.push_back(Range{ head + (a + 1) * PO - 64, (long)head + (a + 1) * PO, q });
            slots.push_back(Range{ slot + 64 * a, (long)slot + 64 * (a + 1), q });
        }
        // the job's own stores end every one of its arrays: child k's array a at o[k] + a PO, the last 16 dwords of 64
        int at = 0;
        for (int k = 0; k < 2; k++)
            for (int a = 0; a < mx_arm_arrays(f[k]); a++, at++)
                if (r.o[k] + a * PO + 192 != head + (at + 1) * PO - 64) fail(where + ": a tail the job does not store");
    }
    for (int c : owner) if (c != 1) { fail(where + ": an array without exactly one tail job"); break; }
    s.arrays += lv.arr_cnt;
    for (const Range& h : heads) {
        for (const Range& x : reads) if (meet(h, x)) { fail(where + ": a job reads a head of the level's own arrays"); break; }
        for (const Range& x : writes) if (meet(h, x)) { fail(where + ": a job stores into a head"); break; }
    }
    for (const Range& t : tails)
        for (const Range& x : writes) if (x.job != t.job && meet(t, x)) { fail(where + ": another job stores into an array's tail"); break; }
    for (const Range& t : slots) {
        for (const Range& x : reads) if (meet(t, x)) { fail(where + ": a job reads a slot"); break; }
        for (const Range& x : writes) if (meet(t, x)) { fail(where + ": a job stores into a slot"); break; }
        for (const Range& x : slots) if (&x != &t && meet(t, x)) { fail(where + ": two arrays share a slot"); break; }
    }
}

} // namespace

int main()
{
    char eng[16];
    int lds_kb, max_levels, in_rate, n;
    while (scanf("%15s %d %d %d %d", eng, &lds_kb, &max_levels, &in_rate, &n) == 5) {
        bad.clear();
        PlanOptions opt;
        opt.mfma = strcmp(eng, "valu") != 0;
        opt.lds_kb = lds_kb;
        if (max_levels) opt.max_levels = max_levels;
        std::vector<std::vector<uint8_t>> modes((size_t)n, std::vector<uint8_t>(MAX_STAGES));
        std::vector<PlanChain> chains;
        for (int i = 0; i < n; i++) {
            int id, rate, fc, out_rate, ofs;
            if (scanf("%d %d %d", &id, &rate, &fc) != 3) return 2;
            const int ns = plan_chain(in_rate, rate, fc, modes[(size_t)i].data(), MAX_STAGES, &out_rate, &ofs);
            if (ns > 0) chains.push_back(PlanChain{ id, ns, modes[(size_t)i].data() });
        }
        BankPlan p;
        const std::string err = plan_bank(chains, opt, p);
        LoweredBank lw;
        const std::string lerr = err.empty() ? lower_bank(p, lw) : std::string();
        Stats s;
        int mx_passes = 0;
        if (err.empty() && lerr.empty()) {
            for (size_t pi = 0; pi < p.passes.size(); pi++) {
                if (!lw.pass_mx[pi]) continue;
                mx_passes++;
                for (int si : p.passes[pi]) {
                    const size_t sub = (size_t)p.streams[(size_t)si].subtree;
                    const TkSubtree& st = p.subtrees[sub];
                    const TkArray* arr = p.arrays.data() + st.array_base;
                    const TkLRoot& root = lw.roots[sub];
                    if (root.kinds >= 1 && root.kinds <= 3) s.roots[root.kinds]++;
                    // the root histories: head = base + k P, slot = 4 * store_base + 64 k, k < mx_root_arrays(kinds)
                    for (int k = 0; k < mx_root_arrays(root.kinds); k++) {
                        if (k >= st.root_arr_cnt || 4 * arr[k].off != root.base + k * mx_pitch(0) || 4 * arr[k].len != mx_pitch(0)) fail("root: restored head is not the arm's window start");
                        else if (arr[k].store != st.store_base + 16 * k) fail("root: derived slot is not the arm's");
                    }
                    if (mx_root_arrays(root.kinds) != st.root_arr_cnt) fail("root: arm count");
                    for (int l = 0; l < st.n_levels; l++) check_level(st, arr, lw.jobs.data() + st.lv[l].mjob_base, l, s);
                }
            }
        }
        printf("{\"error\": \"%s\", \"lower\": \"%s\", \"mx_passes\": %d, \"passes\": %zu, \"arrays\": %d, \"tails\": %d, \"counts\": [%d, %d, %d, %d, %d], "
               "\"classes\": [%d, %d, %d], \"roots\": [%d, %d, %d], \"bad\": [", err.c_str(), lerr.c_str(), mx_passes, p.passes.size(), s.arrays, s.tails,
               s.counts[0], s.counts[1], s.counts[2], s.counts[3], s.counts[4], s.classes[0], s.classes[1], s.classes[2], s.roots[1], s.roots[2], s.roots[3]);
        for (size_t k = 0; k < bad.size(); k++) printf("%s\"%s\"", k ? ", " : "", bad[k].c_str());
        printf("]}\n");
    }
    return 0;
}
