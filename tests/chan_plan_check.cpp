// Runs the bank planner (sdrangel_amd/csrc/chan_plan.cpp) on host, for tests/test_chan_planner.py.
// stdin, one case per line:  engine lds_kb max_levels in_rate n_ch  then n_ch x (channel id, rate, centre)
//   (lds_kb / max_levels 0: the default).  stdout, one JSON object per case: the error (empty when planned), the stream,
// pass and sink lists, and the subtree, node, array and matrix-core job tables as hex of their raw bytes.
#include "chan_plan.hpp"
#include <cstdio>
#include <cstring>

using namespace sdrx;

static void hex(const char* name, const void* p, size_t n)
{
    printf(", \"%s\": \"", name);
    const unsigned char* c = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; i++) printf("%02x", c[i]);
    printf("\"");
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
        for (int i = 0; i < n; i++) {
            int id, rate, fc, out_rate, ofs;
            if (scanf("%d %d %d", &id, &rate, &fc) != 3) return 2;
            const int ns = plan_chain(in_rate, rate, fc, modes[(size_t)i].data(), MAX_STAGES, &out_rate, &ofs);
            if (ns > 0) chains.push_back(PlanChain{ id, ns, modes[(size_t)i].data() });     // no stage: pass-through, no group
        }
        BankPlan p;
        const std::string err = plan_bank(chains, opt, p);
        printf("{\"error\": \"%s\", \"streams\": [", err.c_str());
        for (size_t i = 0; i < p.streams.size(); i++) {
            const PlanStream& s = p.streams[i];
            printf("%s[%d, %d, %d, %d, %ld, %d]", i ? ", " : "", s.trie_node, s.depth, s.pass, s.subtree, s.hist_len, s.sink);
        }
        printf("], \"passes\": [");
        for (size_t q = 0; q < p.passes.size(); q++) {
            printf("%s[", q ? ", " : "");
            for (size_t k = 0; k < p.passes[q].size(); k++) printf("%s%d", k ? ", " : "", p.passes[q][k]);
            printf("]");
        }
        printf("], \"sinks\": [");
        for (size_t k = 0; k < p.sinks.size(); k++) {
            const PlanSink& s = p.sinks[k];
            printf("%s[%d, %d, %d, %d, %d]", k ? ", " : "", s.kind, s.ch, s.stream, s.depth, s.next);
        }
        printf("]");
        hex("subtrees", p.subtrees.data(), p.subtrees.size() * sizeof(TkSubtree));
        hex("nodes", p.nodes.data(), p.nodes.size() * sizeof(TkNode));
        hex("arrays", p.arrays.data(), p.arrays.size() * sizeof(TkArray));
        hex("mjobs", p.mjobs.data(), p.mjobs.size() * sizeof(TkMJob));
        printf("}\n");
    }
    return 0;
}
