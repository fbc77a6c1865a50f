// The bank's matrix-core jobs lowered for the lean kernel (tree_mx_kernel.hpp).  Host-safe: no HIP headers.
//
// A pass whose every level is a matrix-core level (the default plans: at most 4 levels, every entry >= 256 outputs per chunk)
// runs tree_mx_kernel instead of tree_kernel<true>.  That kernel reads one TkLJob per job, 8 dwords = one scalar load, where
// tree_kernel reads a 32-dword TkMJob of absolute LDS addresses.  The lowering uses what the planner's layout already
// guarantees (chan_plan.cpp: alloc_arms, take_array): one level's arrays all have the length arm_len(rel), and a stage's arms are
// allocated back to back, E_I E_Q [O_I O_Q] [A_I A_Q].  So every array a job touches sits at a fixed multiple of the level's
// pitch from ONE base: the odd arm Q at +PI from I, the even arm E[1] at +PI from E[0], and a child's arms at 0, PO, 2 PO, 3 PO
// (and 4 PO, 5 PO for the alternating copy of a child with both kinds).  The kernel adds the lane's share to a base once and
// reaches the rest with the ds_read / ds_write immediate offset.  plan_bank()'s tables are not changed.
#pragma once
#include "tree_layout.hpp"
#include "hb_consts.hpp"
#include <string>
#include <vector>

namespace sdrx {

struct BankPlan;

constexpr int MX_MAX_LEVELS = 4;             // TK_CHUNK >> rel >= 256: the deepest matrix-core level is rel = 4

// byte pitch of the arrays produced at `rel` levels below a pass's root (chan_plan.cpp: arm_len)
constexpr int mx_pitch(int rel) { return 4 * (HIST / 2 + (TK_CHUNK >> (rel + 2))); }

// Epilogue classes.  Within a level the jobs are sorted by class, so that the waves' job pairs are of one class; the kernel runs a
// body specialised for the class at compile time.  Centre stages and lower/upper pairs share the two general classes: the parent's
// mode only swaps the even arms that feed I and Q and flips centre-tap signs (meta bit MX_LU_BIT).
enum : int {
    MX_FAST = 0,        // lower/upper pair, both children present, each with even arms + ONE odd kind, no sink: eight stores, no branch
    MX_ARMS = 1,        // any other job without a sink: arm stores only
    MX_SINK = 2,        // a job with a sink list on either child (channel ends, node streams)
    MX_CLASSES = 3
};
constexpr int MX_LU_BIT = 1 << 16;
// Array histories.  Every entry of a lean pass has >= 256 outputs per chunk, so the last 16 dwords of each arm array of a child
// are written by ONE job, the entry's last of the chunk (the lanes with n16 >= 12), and that job's wave copies the histories of
// the job's arrays: slot -> head, tail -> slot.  A job's children lie back to back (lower, then upper: alloc order), and so do
// their slots: the job carries the first array's index in the subtree (slot = store_base + 16 * index) and the number of arrays.
constexpr int MX_TAIL_BIT = 1 << 17;         // the job writes the tails of its children's arrays (and has at least one array)
constexpr int MX_SLOT_SHIFT = 18, MX_SLOT_MASK = 1023;      // tail jobs: index of the first array of the first child with arms
constexpr int MX_CNT_SHIFT = 28;             // tail jobs: arrays of both children together, 4 .. 12 (the top bits of the word)
constexpr int mx_arm_arrays(int flags) { return flags == 7 ? 6 : flags ? 4 : 0; }

struct TkLJob {
    int b;              // byte address of window entry 0 of the job's first block, odd arm feeding I; Q at +PI
    int c;              // byte address of the centre-tap dword of even arm E[0] of the parent; E[1] at +PI
                        //   (centre: I <- E[0], Q <- E[1]; lower/upper: I <- E[1], Q <- E[0])
    int o[2];           // children's arms: byte address of E_I at the job's first block (0: no arms)
                        //   centre: child 0 only; lower/upper: 0 = lower, 1 = upper
    int sink[2];        // heads of the children's sink lists (-1: none)
    int out0;           // first output of the job inside the chunk
    int meta;           // class | flags of child 0 << 4 | flags of child 1 << 8 (TkMOut::flags: 1 even, 2 plain odd, 4 alternating odd)
                        //   | MX_LU_BIT for a lower/upper parent | MX_TAIL_BIT, first array << MX_SLOT_SHIFT, arrays << MX_CNT_SHIFT for a tail job
};
static_assert(sizeof(TkLJob) == 32, "one s_load_dwordx8 per job");

// A subtree's root arms.  alloc_arms() lays them out like a child's: E_I E_Q [O_I O_Q] [A_I A_Q], back to back, each
// mx_pitch(0) bytes.  So the root fill stores at one per-lane address plus immediates, and the kernel pins two numbers in scalar
// registers where the six arm offsets, their count and the window of TkSubtree took nine.
enum : int { MX_ROOT_O = 1, MX_ROOT_A = 2 };
struct TkLRoot {
    int base;           // byte address of the window of E_I, the first root array (TkSubtree::root_off)
    int kinds;          // MX_ROOT_O: plain odd arms at 2, 3 pitches; MX_ROOT_A: alternating odd arms after them (at 2, 3 without O);
                        // at least one of the two: a root is an inner node
};
constexpr int mx_root_arrays(int kinds) { return 2 + 2 * (kinds & 1) + (kinds & 2); }

inline int mx_class(int meta) { return meta & 15; }
inline int mx_flags(int meta, int k) { return (meta >> (4 + 4 * k)) & 15; }
inline bool mx_tail(int meta) { return (meta & MX_TAIL_BIT) != 0; }
inline int mx_tail_first(int meta) { return (int)(((uint32_t)meta >> MX_SLOT_SHIFT) & MX_SLOT_MASK); }
inline int mx_tail_count(int meta) { return (int)((uint32_t)meta >> MX_CNT_SHIFT); }

struct LoweredBank {
    std::vector<TkLJob> jobs;        // parallel to BankPlan::mjobs: a level's jobs keep their index range (TkLevel::mjob_base, n_mjobs),
                                     // sorted by class inside it
    std::vector<int> src;            // jobs[i] was lowered from mjobs[src[i]]
    std::vector<TkLRoot> roots;      // parallel to BankPlan::subtrees (kinds -1: a subtree the lowering did not take)
    std::vector<uint8_t> pass_mx;    // per pass: 1 = every subtree of the pass runs on tree_mx_kernel
};

// true when every level of the subtree is a matrix-core level (and so the lean kernel can run it)
bool subtree_all_mx(const TkSubtree& st);

// Lower a plan's matrix-core jobs.  Never fails the plan: a pass with a subtree the lowering does not recognise keeps
// tree_kernel<true> (pass_mx 0).  Returns the first such reason, empty when every all-MFMA subtree was lowered.
std::string lower_bank(const BankPlan& plan, LoweredBank& out);

} // namespace sdrx
