// Descriptor tables of the bank's tree kernel (tree_kernel.hpp), as the host planner (chan_plan.cpp) writes them and the
// kernel reads them.  Host-safe: no HIP headers, so host-only code and tests can include it.
#pragma once
#include <stdint.h>

namespace sdrx {

constexpr int TK_CHUNK = 4096;
constexpr int TK_THREADS = 256;
constexpr int TK_MAX_LEVELS = 10;
constexpr int TK_DEFAULT_LEVELS = 4;         // what the planner uses unless told otherwise: measured best for 32, 128 and 256 channels
                                             // (profiles/r02_tree_plan_sweep.txt); up to 6 levels need one warm-up chunk
constexpr int TK_HIST = 2 * TK_CHUNK;        // samples of stream history kept between feeds: (warm + 1) chunks, this for warm = 1

// One table entry = one half-band stage, or a FUSED lower/upper sibling pair: the lower- and the upper-half
// child of a node rotate the odd arm identically (j^(n+1) = (-j)^(n+1) for odd n) and only differ in the sign
// of the centre tap, so 24 of their 25 taps are one shared sum.  The pair costs 12.5 + 2 dot2 per output and
// component instead of 2 x 13.5, and reads the parent's window once.
struct TkOut {                  // 12 dwords: where one stage's outputs go + its centre taps
    int outE_I, outE_Q;         // own output arms (-1: none): even
    int outO_I, outO_Q;         //   odd, plain (for a centre child)
    int outA_I, outA_Q;         //   odd, alternating wrap-negated (for lower/upper children)
    int sink;                   // head of this stage's sink list (index into the sink table), -1: none
    int present;                // 0: this half of the entry is unused
    uint32_t cIe, cIo, cQe, cQo;// packed centre taps for even / odd output index
};
constexpr int TK_NODE_DW = 32;
struct TkNode {                 // 32 dwords
    int oddI, oddQ;             // LDS dword offsets: odd arm it reads (parent's plain or alt copy)
    int cenI, cenQ;             // even-arm arrays feeding the I / Q accumulators (swapped for L/U)
    TkOut a;                    // the stage itself (the LOWER child when fused)
    TkOut b;                    // the UPPER sibling when fused (present = 1)
    int mode_a;                 // SDRX_MODE_* of `a` (the MFMA path derives the centre-tap signs from it)
    int pad[3];
};
static_assert(sizeof(TkOut) == 48 && sizeof(TkNode) == TK_NODE_DW * 4, "node table layout");

struct TkLevel {
    int node_base, n_nodes, jobs_log2, nout;     // nout = outputs per node per chunk; jobs per node = nout >> r_log2
    int arr_base, arr_cnt;                       // arrays PRODUCED by this level's stages (relative to the subtree's array list)
    int r_log2;                                  // outputs per job: 8, 4 or 2
    int in_len;                                  // dwords of every array this level READS (its parents' arms)
    int mfma;                                    // 1: the level runs on the matrix cores (hb_mfma.hpp): nout >= 256, whole jobs per entry
    int mjob_base, n_mjobs;                      // its jobs in the group's TkMJob table (a job = 16 blocks of 16 outputs of one entry, I and Q = two MFMA tiles)
    uint32_t xm;                                 // XORed into the odd-arm dwords this level PRODUCES: HBM_BIAS2 if the next level is an MFMA level
    // The arrays of one level are allocated back to back with one length (chan_plan.cpp), and so are their history slots (16 dwords each,
    // in array order): the history walk computes its addresses from these five numbers instead of reading a per-array table from LDS
    // (a dependent LDS round trip in front of every copy).  Everything a level needs sits in this one 64-byte record = one scalar load.
    int prev_off, prev_arr_cnt;                  // the arrays this level READS (its parents' arms; level 1: the root arms): first window, count;
                                                 // their length is in_len, their slots end where this level's begin
    int arr_off, arr_len;                        // the arrays this level PRODUCES: first window (LDS dword offset), length of each
};
static_assert(sizeof(TkLevel) == 64, "one s_load_dwordx16 per level");

// One matrix-core job, everything resolved by the planner to LDS BYTE addresses of the job's first element (the lane adds its
// share): wave-uniform, fetched with three wide scalar loads.  o[0] / o[1]: a centre stage uses o[0]; a lower/upper pair has the
// lower child in o[0] and the upper one in o[1] (either may be absent: flags = 0, sink = -1).  Absent arm arrays of a present
// child point at a scratch slot, so the epilogue has no branch per array.
struct TkMOut { int E_I, E_Q, O_I, O_Q, A_I, A_Q; int sink; int flags; };     // flags: 1 = even arms, 2 = plain odd arms, 4 = alternating odd arms
struct TkMJob {
    int bI, bQ;                 // window entry 0 of block 16 tb of the odd arm feeding I / Q
    int cI, cQ;                 // dword holding even-arm entry 16 (16 tb) + 20 (centre taps of the job's first block)
    int mode;                   // 0: centre stage, else lower/upper pair
    int out0;                   // first output of the job inside the chunk: 256 tb
    int fast, kinds;            // fast = 1: a lower/upper pair whose two children are inner nodes with even arms + ONE odd-arm kind (its address in
                                // O_I / O_Q) and no sink: stores-only epilogue; kinds bit 0 / 1: child 0 / 1 wants the alternating-sign copy
    TkMOut o[2];
    int pad2[8];
};
static_assert(sizeof(TkMJob) == 128, "job table layout");

struct TkSubtree {
    int n_levels;
    int warm;                   // warm-up chunks in front of a segment
    int n_nodes;                // all levels
    int node_base;              // first node (global index) -- levels index relative to the table
    int n_arrays, array_base;   // all arrays: [root arrays][level-1 arrays][level-2 arrays]...
    int root_arr_cnt;           // the first root_arr_cnt arrays are the root arms
    int lds_dwords;             // two arm regions + history store + node table copy (+ 256 B scratch for the MFMA jobs' absent arms)
    int sink_base, n_sinks;     // this subtree's sinks are one contiguous run of the group's sink table
    int sink_tab;               // LDS dword offset of the copy of that run (TK_SINK_DW dwords each)
    int node_tab;               // LDS dword offset of the node table copy
    int store_base;             // LDS dword offset of the history slots: 16 dwords per array, in array order (root arms first)
    int root_off, root_len;     // the root arms: first window, length of each
    int rootE_I, rootE_Q, rootO_I, rootO_Q, rootA_I, rootA_Q;   // root arms (-1: none)
    uint32_t root_xm;           // XORed into the root odd arms (HBM_BIAS2 if level 1 is an MFMA level)
    int dbg;                    // timing experiments only (SDRX_CHAN_DBG, results are WRONG when set): 1 skip MFMA jobs, 2 skip the
                                // history walks, 4 skip the root fill (a bit 16, skip the MFMA epilogues, gave DESIGN 4.3a its split and was
                                // removed: its branch sat between the MFMAs and the epilogues of every pair)
    TkLevel lv[TK_MAX_LEVELS];
};

// One polyphase array.  Its window [off, off+len) = 16 dwords of history + the chunk's payload lives in one of
// two LDS regions that alternate by tree level (level l's arrays are dead once level l+1 has consumed them, so
// level l+2 reuses the space: 61 KB -> 40 KB for the cfg-3 raw pass, 2 -> 4 workgroups per CU); the 16-dword
// history survives in a persistent slot `store`: saved when the consumer level is done, restored in front of
// the window before the producer writes the next chunk.
struct TkArray { int off, len, store, bias; };     // bias = 1: an odd arm an MFMA level reads: its zero history is HBM_BIAS2

struct TkStream {               // per feed, per input stream of a pass
    const uint32_t* hist;       // hist_len samples: absolute positions [t_old - hist_len, t_old)
    const uint32_t* in;         // new samples: absolute positions [t_old, t_new)
    long t_old, t_new;
    long c_first, c_last;       // absolute chunk range to (re)compute
    int cps;                    // chunks per segment
    int subtree;
    long hist_len;              // (warm + 1) * TK_CHUNK
};

constexpr int TK_SINK_DW = 8;
struct TkSink {                 // where a node's outputs go in global memory
    uint32_t* ptr0;             // element for absolute output index 0 (= buffer - base: never dereferenced outside [lo, hi))
    long lo, hi;                // store only absolute output indices in [lo, hi)
    int shift;                  // 0: raw node stream; n > 0: channel end, value / 2^n (toward zero)
    int next;                   // next sink of the same node, -1: end of list
};

static_assert(sizeof(TkSink) == TK_SINK_DW * 4, "sink table layout");

} // namespace sdrx
