// Lists the branches of tree_kernel.hpp a bank plan makes the kernel take, for tests/test_bank_paths.py.  Host only: the planner
// (sdrangel_amd/csrc/chan_plan.cpp) and its table layouts, no HIP.
// stdin, one case per line, as tests/chan_plan_check.cpp:  engine lds_kb max_levels in_rate n_ch  then n_ch x (channel id, rate, centre).
// stdout, one JSON object per case: {"error": "<planner error, empty when planned>", "depth": <stages of the longest chain>,
// "paths": [sorted path names]}.
//
// Path names and the branch of tree_kernel.hpp each one stands for ({arms} = none | EO | EA | EOA: even arms with the plain and / or the
// alternating-sign odd arms a stage writes for its children; {sink} = none | end | stream | list: the stage's sink list, followed through
// `next`, is empty, one channel end, one node stream, or two or more entries):
//   mfma.fast.k<kinds>       matrix-core level, TkMJob::fast: the stores-only epilogue with `kinds` (0..3) picking the alternating copies
//   mfma.centre.{arms}.{sink}  matrix-core level, centre job (mode 0): emit() for o[0]
//   mfma.lower.{arms}.{sink}   matrix-core level, generic lower/upper job: emit() for the lower child o[0]
//   mfma.upper.{arms}.{sink}   ... for the upper child o[1]
//   mfma.lower.absent / mfma.upper.absent   that child skipped (flags 0, no sink)
//   mfma.tail                a wave's run of the level's jobs has an odd length: the `tt < t1` single job after the pairs
//   dot2.R8 / R4 / R2        dot2 level, job<R> (r_log2 = 3 / 2 / 1)
//   dot2.a.{arms}.{sink}     dot2 level, emit() of TkNode.a (a centre stage, a lone lower/upper one, or the lower of a fused pair)
//   dot2.b.{arms}.{sink}     dot2 level, emit() of TkNode.b, the fused upper sibling
//   dot2.b.absent            dot2 level, an entry without a fused sibling (nt[5].w == 0)
//   root.EO / EA / EOA       the root fill writes the plain (rO_I >= 0) and / or the alternating (rA_I >= 0) odd arms
//   root.bias / root.nobias  root_xm set (level 1 on the matrix cores) or not
//   warm.1 / warm.2 / warm.3+  warm-up chunks in front of a segment (stream history of warm + 1 chunks)
//   passes.1 / passes.2-5 / passes.6+   launches per feed of the group
// Tables the kernel would mishandle get names outside any vocabulary: mfma.fast.drops-outputs (a job marked fast whose children
// have sinks or other arms than the stores-only epilogue writes), mfma.centre.drops-second-child (a second child on a centre job),
// and arms "E" / "odd-without-even" (arm sets no planned stage has).
#include "chan_plan.hpp"
#include <cstdio>
#include <cstring>
#include <set>
#include <string>

using namespace sdrx;

static const char* arms_name(bool e, bool o, bool a)
{
    if (!e) return (o || a) ? "odd-without-even" : "none";
    return o ? (a ? "EOA" : "EO") : (a ? "EA" : "E");
}

static const char* sink_name(const BankPlan& p, int head)
{
    int n = 0, kind = -1;
    for (int s = head; s >= 0; s = p.sinks[(size_t)s].next) { n++; kind = p.sinks[(size_t)s].kind; }
    if (n == 0) return "none";
    if (n > 1) return "list";
    return kind == 0 ? "end" : "stream";
}

static std::string mfma_child(const BankPlan& p, const TkMOut& o)
{
    if (o.flags == 0 && o.sink < 0) return "absent";
    return std::string(arms_name(o.flags & 1, o.flags & 2, o.flags & 4)) + "." + sink_name(p, o.sink);
}

static std::string dot2_out(const BankPlan& p, const TkOut& o)
{
    return std::string(arms_name(o.outE_I >= 0, o.outO_I >= 0, o.outA_I >= 0)) + "." + sink_name(p, o.sink);
}

static void list_paths(const BankPlan& p, std::set<std::string>& out)
{
    const size_t np = p.passes.size();
    out.insert(np == 1 ? "passes.1" : np <= 5 ? "passes.2-5" : "passes.6+");
    for (const TkSubtree& st : p.subtrees) {
        out.insert(std::string("root.") + arms_name(st.rootE_I >= 0, st.rootO_I >= 0, st.rootA_I >= 0));
        out.insert(st.root_xm ? "root.bias" : "root.nobias");
        out.insert(st.warm == 1 ? "warm.1" : st.warm == 2 ? "warm.2" : "warm.3+");
        for (int l = 0; l < st.n_levels; l++) {
            const TkLevel& lv = st.lv[l];
            if (p.mfma && lv.mfma) {
                for (int q = 0; q < lv.n_mjobs; q++) {
                    const TkMJob& j = p.mjobs[(size_t)(lv.mjob_base + q)];
                    if (j.fast) {
                        out.insert("mfma.fast.k" + std::to_string(j.kinds));
                        // the stores-only epilogue writes even arms + one odd kind per child of a lower/upper pair and nothing else
                        for (int c = 0; c < 2; c++)
                            if (!j.mode || j.o[c].sink >= 0 || (j.o[c].flags != 3 && j.o[c].flags != 5) || ((j.kinds >> c) & 1) != (j.o[c].flags == 5))
                                out.insert("mfma.fast.drops-outputs");
                    } else if (j.mode == 0) {
                        out.insert("mfma.centre." + mfma_child(p, j.o[0]));
                        if (j.o[1].flags || j.o[1].sink >= 0) out.insert("mfma.centre.drops-second-child");     // mode 0 reads o[0] only
                    } else {
                        out.insert("mfma.lower." + mfma_child(p, j.o[0]));
                        out.insert("mfma.upper." + mfma_child(p, j.o[1]));
                    }
                }
                // the kernel's split of the level's jobs over its waves: contiguous runs of `per`, taken two at a time
                constexpr int WAVES = TK_THREADS / 64;
                const int per = (lv.n_mjobs + WAVES - 1) / WAVES;
                for (int w = 0; w < WAVES; w++) {
                    const int t0 = w * per, t1 = t0 + per < lv.n_mjobs ? t0 + per : lv.n_mjobs;
                    if (t1 > t0 && ((t1 - t0) & 1)) out.insert("mfma.tail");
                }
                continue;
            }
            out.insert("dot2.R" + std::to_string(1 << lv.r_log2));
            for (int e = 0; e < lv.n_nodes; e++) {
                const TkNode& nd = p.nodes[(size_t)(st.node_base + lv.node_base + e)];
                out.insert("dot2.a." + dot2_out(p, nd.a));
                out.insert(nd.b.present ? "dot2.b." + dot2_out(p, nd.b) : std::string("dot2.b.absent"));
            }
        }
    }
}

int main()
{
    char eng[16];
    int lds_kb, max_levels, in_rate, n;
    while (scanf("%15s %d %d %d %d", eng, &lds_kb, &max_levels, &in_rate, &n) == 5) {
        PlanOptions opt;
        opt.mfma = strcmp(eng, "valu") != 0;
        opt.lds_kb = lds_kb;
        if (max_levels) opt.max_levels = max_levels;
        std::vector<std::vector<uint8_t>> modes((size_t)n, std::vector<uint8_t>(MAX_STAGES));
        std::vector<PlanChain> chains;
        int depth = 0;
        for (int i = 0; i < n; i++) {
            int id, rate, fc, out_rate, ofs;
            if (scanf("%d %d %d", &id, &rate, &fc) != 3) return 2;
            const int ns = plan_chain(in_rate, rate, fc, modes[(size_t)i].data(), MAX_STAGES, &out_rate, &ofs);
            if (ns > 0) chains.push_back(PlanChain{ id, ns, modes[(size_t)i].data() });     // no stage: pass-through, no group
            if (ns > depth) depth = ns;
        }
        BankPlan p;
        std::set<std::string> paths;
        const std::string err = chains.empty() ? std::string() : plan_bank(chains, opt, p);
        if (err.empty() && !chains.empty()) list_paths(p, paths);
        printf("{\"error\": \"%s\", \"depth\": %d, \"paths\": [", err.c_str(), depth);
        bool first = true;
        for (const std::string& s : paths) { printf("%s\"%s\"", first ? "" : ", ", s.c_str()); first = false; }
        printf("]}\n");
    }
    return 0;
}
