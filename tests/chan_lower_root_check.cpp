// Checks the lowered root records (TkLRoot, sdrangel_amd/csrc/chan_lower.cpp) on host, for tests/test_chan_lower_root.py.
// stdin, one bank per line:  engine lds_kb max_levels in_rate n_ch  then n_ch x (channel id, rate, centre)   (as tests/chan_lower_check.cpp)
// stdout, one JSON object per bank: {"error": planner error, "lower": lowering error, "bad": [first problems found],
// "kinds": [lean subtrees with root arms E, E+O, E+A, E+O+A], "first": the kinds of the raw stream's subtree (-1: not lean),
// "passes" / "mx_passes": all passes / those on the lean kernel, "refused": how many of the tampered plans the lowering refused,
// "tampered": how many were tried}.
//
// What is checked:
//   * roots is parallel to the subtrees; a subtree of a lean pass has a record, any other has kinds = -1;
//   * the record restated as tree_mx_kernel.hpp uses it: E_I at base, E_Q one pitch on, the plain odd arms at 2 and 3 pitches, the
//     alternating ones behind them; that is where TkSubtree has the arms, the arms it lacks are the ones the record leaves out,
//     the arrays counted by mx_root_arrays() are the subtree's root arrays, and the root history copy's window is the same;
//   * a plan whose root arms sit elsewhere (one table entry moved, for every entry the kernel no longer reads) is refused:
//     its pass keeps the general kernel.
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

void check_root(const TkSubtree& st, const TkLRoot& r, size_t s)
{
    const std::string where = "subtree " + std::to_string(s);
    const int P = mx_pitch(0);
    if (r.kinds < 1 || r.kinds > (MX_ROOT_O | MX_ROOT_A)) { fail(where + ": kinds out of range"); return; }
    // byte addresses the kernel's root fill writes, in its order
    int at = r.base;
    const int eI = at, eQ = at + P;
    at += 2 * P;
    int oI = -1, oQ = -1, aI = -1, aQ = -1;
    if (r.kinds & MX_ROOT_O) { oI = at; oQ = at + P; at += 2 * P; }
    if (r.kinds & MX_ROOT_A) { aI = at; aQ = at + P; at += 2 * P; }
    auto same = [](int table_dw, int byte) { return table_dw < 0 ? byte < 0 : byte == 4 * table_dw; };
    if (!same(st.rootE_I, eI) || !same(st.rootE_Q, eQ)) fail(where + ": even arms elsewhere");
    if (!same(st.rootO_I, oI) || !same(st.rootO_Q, oQ)) fail(where + ": plain odd arms elsewhere");
    if (!same(st.rootA_I, aI) || !same(st.rootA_Q, aQ)) fail(where + ": alternating odd arms elsewhere");
    if (mx_root_arrays(r.kinds) != st.root_arr_cnt) fail(where + ": root array count");
    if (r.base != 4 * st.root_off || 4 * st.root_len != P) fail(where + ": root history window");
    if (at - r.base != st.root_arr_cnt * 4 * st.root_len) fail(where + ": root arms not back to back");
    if (at > st.lds_dwords * 4) fail(where + ": root arms outside the pass's LDS");
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
        int kinds[4] = { 0, 0, 0, 0 }, tampered = 0, refused = 0, first = -1, mx_passes = 0;
        if (err.empty() && lerr.empty()) {
            if (lw.roots.size() != p.subtrees.size()) fail("roots not parallel to the subtrees");
            for (uint8_t m : lw.pass_mx) mx_passes += m;
            if (!p.streams.empty() && p.streams[0].subtree >= 0 && (size_t)p.streams[0].subtree < lw.roots.size())
                first = lw.roots[(size_t)p.streams[0].subtree].kinds;
            std::vector<int> pass_of(p.subtrees.size(), -1);
            for (size_t pi = 0; pi < p.passes.size(); pi++)
                for (int si : p.passes[pi]) if (p.streams[(size_t)si].subtree >= 0) pass_of[(size_t)p.streams[(size_t)si].subtree] = (int)pi;
            for (size_t s = 0; s < p.subtrees.size() && s < lw.roots.size(); s++) {
                const bool lean = opt.mfma && subtree_all_mx(p.subtrees[s]);
                if (!lean) { if (lw.roots[s].kinds != -1) fail("a record for a subtree the lean kernel does not run"); continue; }
                check_root(p.subtrees[s], lw.roots[s], s);
                if (lw.roots[s].kinds >= 0 && lw.roots[s].kinds < 4) kinds[lw.roots[s].kinds]++;
                if (pass_of[s] < 0 || !lw.pass_mx[(size_t)pass_of[s]]) continue;
                // move one table entry of the first lean subtrees: the lowering has to notice each
                if (tampered >= 12) continue;
                int TkSubtree::* const field[] = { &TkSubtree::rootE_I, &TkSubtree::rootE_Q, &TkSubtree::rootO_I, &TkSubtree::rootO_Q,
                                                   &TkSubtree::rootA_I, &TkSubtree::rootA_Q, &TkSubtree::root_off, &TkSubtree::root_len,
                                                   &TkSubtree::root_arr_cnt };
                for (auto f : field) {
                    BankPlan q = p;
                    int& v = q.subtrees[s].*f;
                    v = v < 0 ? q.subtrees[s].rootE_I + 6 * q.subtrees[s].root_len : v + 1;
                    LoweredBank lq;
                    const std::string e = lower_bank(q, lq);
                    tampered++;
                    if (!e.empty() && lq.pass_mx[(size_t)pass_of[s]] == 0 && lq.roots[s].kinds == -1) refused++;
                    else fail("subtree " + std::to_string(s) + ": a moved root entry was lowered");
                }
            }
        }
        printf("{\"error\": \"%s\", \"lower\": \"%s\", \"kinds\": [%d, %d, %d, %d], \"first\": %d, \"passes\": %zu, \"mx_passes\": %d, "
               "\"tampered\": %d, \"refused\": %d, \"bad\": [", err.c_str(), lerr.c_str(),
               kinds[0], kinds[1], kinds[2], kinds[3], first, p.passes.size(), mx_passes, tampered, refused);
        for (size_t k = 0; k < bad.size(); k++) printf("%s\"%s\"", k ? ", " : "", bad[k].c_str());
        printf("]}\n");
    }
    return 0;
}
