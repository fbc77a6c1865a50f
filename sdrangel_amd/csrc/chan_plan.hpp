// The channelizer bank's planner, host only (no HIP): the float bisection that gives every channel its stage string, and
// the plan of a group of channels -- trie, passes, and the descriptor tables tree_kernel.hpp reads (tree_layout.hpp).
// sdrx_chan.hip allocates the buffers a plan names, uploads its tables and launches.
#pragma once
#include "tree_layout.hpp"
#include <string>
#include <vector>

namespace sdrx {

constexpr int MAX_STAGES = 30;

// DownChannelizer::applyConfiguration / createFilterChain (downchannelizer.cpp:157-189, 250-287), restated: the stage modes
// (SDRX_MODE_*) of the chain, at most `cap`; returns their number
int plan_chain(int32_t in_rate, int32_t req_rate, int32_t req_fc, uint8_t* modes, int cap, int32_t* out_rate, int32_t* ofs_out);

struct PlanOptions {
    bool mfma = true;                        // SDRX_CHAN_ENGINE: matrix-core levels unless "valu"
    int lds_kb = 0;                          // SDRX_CHAN_LDS_KB: LDS budget of a pass (16..150); 0: by the channel count
    int max_levels = TK_DEFAULT_LEVELS;      // SDRX_CHAN_MAX_LEVELS: levels per pass (1..TK_MAX_LEVELS)
    int dbg = 0;                             // SDRX_CHAN_DBG: TkSubtree::dbg
    bool debug = false;                      // SDRX_CHAN_DEBUG: print one line per pass stream to stderr
};
PlanOptions plan_options_from_env();         // read at every plan: bank create, reset, reconfigure, add_channel

struct PlanChain { int ch; int n; const uint8_t* modes; };    // a channel of the group: bank index, its n stage modes

struct PlanStream {
    int trie_node = 0, depth = 0, pass = 0;
    int subtree = -1;                        // the subtree the stream feeds (-1: none)
    long hist_len = TK_HIST;                 // samples kept between feeds: (warm-up chunks of its subtree + 1) chunks
    int sink = -1;                           // sink (in the producing pass) that writes a node stream
};
struct PlanSink { int kind; int ch; int stream; int depth; int next; };   // kind 0 channel `ch`, 1 node stream `stream`

struct BankPlan {
    bool mfma = true;                        // engine the tables were made for
    std::vector<PlanStream> streams;         // [0] = the raw stream
    std::vector<std::vector<int>> passes;    // stream indices per pass, contiguous in creation order
    std::vector<TkSubtree> subtrees;
    std::vector<TkNode> nodes;
    std::vector<TkArray> arrays;
    std::vector<TkMJob> mjobs;               // matrix-core jobs of every MFMA level
    std::vector<PlanSink> sinks;
};

// The plan of one group (channels with at least one stage).  Empty string, or what does not fit.
std::string plan_bank(const std::vector<PlanChain>& chains, const PlanOptions& opt, BankPlan& plan);

} // namespace sdrx
