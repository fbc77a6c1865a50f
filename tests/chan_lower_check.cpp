// Checks the lowering of the bank plan for the lean kernel (sdrangel_amd/csrc/chan_lower.cpp) on host, for tests/test_chan_lower.py.
// stdin, one bank per line:  engine lds_kb max_levels in_rate n_ch  then n_ch x (channel id, rate, centre)   (as tests/chan_plan_check.cpp)
// stdout, one JSON object per bank: {"error": planner error, "lower": lowering error, "bad": [first problems found], "jobs": n,
// "mx_passes": passes on the lean kernel, "passes": all passes, "classes": jobs per class}.
//
// What is checked, for every pass the lean kernel runs:
//   * every lowered job reads and writes the same arrays at the same byte offsets as the TkMJob it came from, with the
//     addresses tree_mx_kernel.hpp forms from it (base + pitch multiples), and keeps its sinks and first output;
//   * a level's lowered jobs are a permutation of its TkMJobs, sorted by class, and each class is what the job needs;
//   * within a level, no two bytes written by the level's jobs overlap, and nothing written overlaps what the level reads;
//   * every byte read or written lies inside the pass's LDS (TkSubtree::lds_dwords), and that fits the kernel's 160 KB.
#include "chan_plan.hpp"
#include "chan_lower.hpp"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace sdrx;

namespace {

struct Range { long lo, hi; int job; bool write; };

std::vector<std::string> bad;
void fail(const std::string& s) { if (bad.size() < 8) bad.push_back(s); }

// the lane offsets tree_mx_kernel.hpp adds: window reads 16 B at 32 n + 16 g (+ 64), centre reads 12 B at 32 n + 8 g,
// stores 4 B at 16 n + 4 g (n < 16, g < 4).  These spans and the base + pitch formulas below (check_job) restate the
// kernel's address arithmetic: keep them in step with tree_mx_kernel.hpp.  This checker proves the lowering consistent with the
// planner's tables and with that restatement; the epilogue's classes and signs are covered by the GPU suite, which runs the lean
// kernel for every default pass.
constexpr int WIN_SPAN = 32 * 15 + 16 * 3 + 64 + 16, CEN_SPAN = 32 * 15 + 8 * 3 + 12, OUT_SPAN = 16 * 15 + 4 * 3 + 4;

void check_job(const TkMJob& j, const TkLJob& r, int PI, int PO, int lvl, std::vector<Range>& rg, int q)
{
    char where[96];
    snprintf(where, sizeof where, "level %d job %d", lvl, q);
    const int cls = mx_class(r.meta);
    const bool lu = (r.meta & MX_LU_BIT) != 0;
    // reads: the odd arms, the centre taps (which even arm feeds I depends on the parent's mode)
    if (lu != (j.mode != 0)) fail(std::string(where) + ": parent mode differs");
    if (cls == MX_FAST && !lu) fail(std::string(where) + ": branch-free class for a centre stage");
    if (r.b != j.bI || r.b + PI != j.bQ) fail(std::string(where) + ": odd-arm windows differ");
    const int cI = lu ? r.c + PI : r.c, cQ = lu ? r.c : r.c + PI;
    if (cI != j.cI || cQ != j.cQ) fail(std::string(where) + ": centre taps differ");
    if (r.out0 != j.out0) fail(std::string(where) + ": first output differs");
    for (int b : { r.b, r.b + PI }) rg.push_back(Range{ b, (long)b + WIN_SPAN, q, false });
    for (int c : { cI, cQ }) rg.push_back(Range{ c, (long)c + CEN_SPAN, q, false });
    bool sink = false;
    for (int k = 0; k < 2; k++) {
        const TkMOut& m = j.o[k];
        const int f = mx_flags(r.meta, k);
        if (f != m.flags) fail(std::string(where) + ": arm flags differ");
        if (r.sink[k] != m.sink) fail(std::string(where) + ": sink list differs");
        sink |= m.sink >= 0;
        if (!f) continue;
        // the stores of tree_mx_kernel.hpp: E at 0 / PO, the odd arm at 2 PO / 3 PO (plain if f & 2, else alternating),
        // the alternating copy of a child with both kinds at 4 PO / 5 PO
        std::vector<std::pair<int, int>> want;      // (address the TkMJob names, address the lowered job writes)
        want.emplace_back(m.E_I, r.o[k]); want.emplace_back(m.E_Q, r.o[k] + PO);
        if (j.fast) { want.emplace_back(m.O_I, r.o[k] + 2 * PO); want.emplace_back(m.O_Q, r.o[k] + 3 * PO); }
        else if (f & 2) {
            want.emplace_back(m.O_I, r.o[k] + 2 * PO); want.emplace_back(m.O_Q, r.o[k] + 3 * PO);
            if (f & 4) { want.emplace_back(m.A_I, r.o[k] + 4 * PO); want.emplace_back(m.A_Q, r.o[k] + 5 * PO); }
        } else { want.emplace_back(m.A_I, r.o[k] + 2 * PO); want.emplace_back(m.A_Q, r.o[k] + 3 * PO); }
        for (const auto& w : want) {
            if (w.first != w.second) fail(std::string(where) + ": an arm store differs");
            rg.push_back(Range{ w.second, (long)w.second + OUT_SPAN, q, true });
        }
    }
    // the class: what the epilogue must do, no more
    const int want_cls = j.fast ? MX_FAST : sink ? MX_SINK : MX_ARMS;
    if (cls != want_cls) fail(std::string(where) + ": wrong class");
    if (!j.mode && (j.o[1].flags || j.o[1].sink >= 0)) fail(std::string(where) + ": centre stage with a second child");
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
        int classes[MX_CLASSES] = { 0 }, mx_passes = 0, njobs = 0;
        if (err.empty() && lerr.empty()) {
            if (lw.jobs.size() != p.mjobs.size() || lw.pass_mx.size() != p.passes.size()) fail("table sizes");
            for (size_t pi = 0; pi < p.passes.size(); pi++) {
                bool all = opt.mfma;
                for (int si : p.passes[pi]) all = all && subtree_all_mx(p.subtrees[(size_t)p.streams[(size_t)si].subtree]);
                if (lw.pass_mx[pi] != (all ? 1 : 0)) fail("pass " + std::to_string(pi) + ": kernel choice");
                if (!lw.pass_mx[pi]) continue;
                mx_passes++;
                for (int si : p.passes[pi]) {
                    const TkSubtree& st = p.subtrees[(size_t)p.streams[(size_t)si].subtree];
                    if (st.lds_dwords * 4 > 160 * 1024) fail("LDS over the kernel's 160 KB");
                    for (int l = 0; l < st.n_levels; l++) {
                        const TkLevel& lv = st.lv[l];
                        std::vector<Range> rg;
                        std::vector<int> seen;
                        int prev_cls = -1;
                        for (int q = 0; q < lv.n_mjobs; q++) {
                            const int i = lv.mjob_base + q, s = lw.src[(size_t)i];
                            if (s < lv.mjob_base || s >= lv.mjob_base + lv.n_mjobs) fail("job moved out of its level");
                            seen.push_back(s);
                            const TkLJob& r = lw.jobs[(size_t)i];
                            if (mx_class(r.meta) < prev_cls) fail("level not sorted by class");
                            prev_cls = mx_class(r.meta);
                            classes[std::min(MX_CLASSES - 1, std::max(0, mx_class(r.meta)))]++;
                            njobs++;
                            check_job(p.mjobs[(size_t)s], r, mx_pitch(l), mx_pitch(l + 1), l, rg, q);
                        }
                        std::sort(seen.begin(), seen.end());
                        for (size_t k = 0; k < seen.size(); k++) if (seen[k] != lv.mjob_base + (int)k) { fail("not a permutation"); break; }
                        for (const Range& a : rg) if (a.lo < 0 || a.hi > (long)st.lds_dwords * 4) fail("access outside the pass's LDS");
                        // a store may meet nothing else of the level: no other store, no read (of any job, its own included)
                        for (size_t x = 0; x < rg.size(); x++) {
                            if (!rg[x].write) continue;
                            for (size_t y = 0; y < rg.size(); y++)
                                if (x != y && rg[x].lo < rg[y].hi && rg[y].lo < rg[x].hi) { fail("level " + std::to_string(l) + ": overlapping LDS ranges"); break; }
                        }
                    }
                }
            }
        }
        printf("{\"error\": \"%s\", \"lower\": \"%s\", \"jobs\": %d, \"mx_passes\": %d, \"passes\": %zu, \"classes\": [", err.c_str(), lerr.c_str(),
               njobs, mx_passes, p.passes.size());
        for (int c = 0; c < MX_CLASSES; c++) printf("%s%d", c ? ", " : "", classes[c]);
        printf("], \"bad\": [");
        for (size_t k = 0; k < bad.size(); k++) printf("%s\"%s\"", k ? ", " : "", bad[k].c_str());
        printf("]}\n");
    }
    return 0;
}
