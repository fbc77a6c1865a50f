// libsdrx.so: the channelizer bank's planner (chan_plan.hpp).  Host code only, no HIP headers; sdrx_chan.hip compiles it in.
#include "chan_plan.hpp"
#include "hb_consts.hpp"
#include "../../include/sdrx.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace sdrx {

/* ------------------------------------------------------------------ the float bisection
 * All interval arithmetic is float32 (`Real`); the reference writes `x / 2.0` in two places, which is evaluated in
 * double and rounded to float when passed on -- kept.                                                               */
static bool contains(float ss, float se, float cs, float ce)
{
    if (se <= ss || ce <= cs) return false;               // signalContainsChannel (:240-248)
    return ss <= cs && se >= ce;
}

int plan_chain(int32_t in_rate, int32_t req_rate, int32_t req_fc, uint8_t* modes, int cap, int32_t* out_rate, int32_t* ofs_out)
{
    if (in_rate == 0) { *out_rate = 0; *ofs_out = 0; return 0; }   // "m_inputSampleRate=0 aborting"
    float s = (float)(in_rate / -2), e = (float)(in_rate / 2);
    const float cs = (float)(req_fc - req_rate / 2), ce = (float)(req_fc + req_rate / 2);
    int n = 0;
    while (n < cap) {
        const float bw = e - s, rot = bw / 4;
        const float mid_lo = (float)((double)s + (double)bw / 2.0);       // sigStart + sigBw / 2.0
        const float mid_hi = e - bw / 2.0f;                               // sigEnd - sigBw / 2.0f
        if (contains(s, mid_lo, cs, ce)) { modes[n++] = SDRX_MODE_LOWER; e = mid_lo; continue; }
        if (contains(mid_hi, e, cs, ce)) { modes[n++] = SDRX_MODE_UPPER; s = mid_hi; continue; }
        const float cs2 = s + rot, ce2 = e - rot;
        if (contains(cs2, ce2, cs, ce)) { modes[n++] = SDRX_MODE_CENTER; s = cs2; e = ce2; continue; }
        break;
    }
    const float ofs = (float)(((double)(ce - cs) / 2.0 + (double)cs) - ((double)(e - s) / 2.0 + (double)s));
    *ofs_out = (int32_t)ofs;                               // Real -> int m_currentCenterFrequency
    *out_rate = in_rate / (1 << n);
    return n;
}

PlanOptions plan_options_from_env()
{
    PlanOptions o;
    // half-band engine: the matrix cores (i8 MFMA, hb_mfma.hpp) unless "valu" asks for the dot2 kernel of rounds 1-2 (both
    // are gfx950 code, both bit-exact; tests run the matrix under each)
    const char* e = getenv("SDRX_CHAN_ENGINE");
    o.mfma = !(e && strcmp(e, "valu") == 0);
    e = getenv("SDRX_CHAN_LDS_KB");
    if (e && atoi(e) >= 16 && atoi(e) <= 150) o.lds_kb = atoi(e);
    // deeper passes (experiment, DESIGN 4.3: fewer node-stream bytes for more LDS) need ceil(46 * (2^levels - 1) / 4096)
    // warm-up chunks and as many more chunks of stream history
    e = getenv("SDRX_CHAN_MAX_LEVELS");
    if (e && atoi(e) >= 1 && atoi(e) <= TK_MAX_LEVELS) o.max_levels = atoi(e);
    e = getenv("SDRX_CHAN_DBG");
    o.dbg = e ? atoi(e) : 0;
    o.debug = getenv("SDRX_CHAN_DEBUG") != nullptr;
    return o;
}

/* ------------------------------------------------------------------ the plan of one group */
namespace {

constexpr int LDS_BUDGET_DW_DEFAULT = 40 * 1024 / 4;       // four workgroups per CU (the kernel has no static LDS)
constexpr int LDS_HARD_DW = 150 * 1024 / 4;                // arm regions of a pass
constexpr int LDS_MAX_DW = 159 * 1024 / 4;                 // everything: < the 160 KB of dynamic LDS the kernel may ask for

// Wide banks (cfg 4: 256 channels) have a dense tree top whose levels need ~25 KB each; with 40 KB the greedy cut ends up
// with 1-2 levels per pass and six passes.  64 KB (two workgroups per CU) measured 1.29 vs 1.42 ms per 64 Mi-sample feed
// for 256 channels, but 0.82 vs 0.71 ms for 128 and 0.62 vs 0.45 ms for 32 -- so only wide banks get it.
int lds_budget_dw(const PlanOptions& opt, size_t n_channels)
{
    if (opt.lds_kb) return opt.lds_kb * 1024 / 4;
    return n_channels >= 192 ? 64 * 1024 / 4 : LDS_BUDGET_DW_DEFAULT;
}

// a level runs on the matrix cores when an entry fills whole tiles (16 blocks of 16 outputs per component and chunk)
bool level_is_mfma(bool engine, int rel) { return engine && (TK_CHUNK >> rel) >= 256; }

int arm_len(int rel_depth) { return HIST / 2 + (TK_CHUNK >> (rel_depth + 2)); }   // dwords

struct HNode {
    int depth = 0;
    int child[3] = { -1, -1, -1 };   // by SDRX_MODE_*
    std::vector<int> ends;           // bank channel ids whose chain ends here
    bool has_centre() const { return child[SDRX_MODE_CENTER] >= 0; }
    bool has_lu() const { return child[SDRX_MODE_LOWER] >= 0 || child[SDRX_MODE_UPPER] >= 0; }
    bool inner() const { return has_centre() || has_lu(); }
};

std::vector<HNode> build_trie(const std::vector<PlanChain>& chains)
{
    std::vector<HNode> trie(1);
    for (const PlanChain& c : chains) {
        int id = 0;
        for (int s = 0; s < c.n; s++) {
            const int m = c.modes[s];
            if (trie[id].child[m] < 0) {
                trie[id].child[m] = (int)trie.size();
                trie.emplace_back();
                trie.back().depth = s + 1;
            }
            id = trie[id].child[m];
        }
        trie[id].ends.push_back(c.ch);
    }
    return trie;
}

int height(const std::vector<HNode>& trie, int id)
{
    int h = 0;
    for (int m = 0; m < 3; m++) if (trie[id].child[m] >= 0) h = std::max(h, 1 + height(trie, trie[id].child[m]));
    return h;
}

// LDS dwords a subtree of `levels` levels below trie node `root` needs: two arm regions (even / odd producer
// level, each as large as its biggest level), 16 dwords of persistent history per array, the node table
// (a lower/upper sibling pair shares one entry)
int subtree_lds(const std::vector<HNode>& trie, int root, int levels)
{
    int region[2] = { 0, 0 }, n_arrays = 0, n_entries = 0, n_sinks = 0;
    std::vector<int> cur{ root };
    for (int rel = 0; rel < levels; rel++) {
        std::vector<int> nxt;
        int level_dw = 0;
        for (int id : cur) {
            const bool c = trie[id].has_centre(), lu = trie[id].has_lu();
            if (!c && !lu) continue;
            const int na = 2 + (c ? 2 : 0) + (lu ? 2 : 0);
            level_dw += arm_len(rel) * na; n_arrays += na;
            n_entries += (c ? 1 : 0) + (lu ? 1 : 0);
            for (int m = 0; m < 3; m++) if (trie[id].child[m] >= 0) {
                const int kid = trie[id].child[m];
                nxt.push_back(kid);
                // sinks of the stage: every channel that ends there, plus a node stream where the tree goes on below the pass
                n_sinks += (int)trie[kid].ends.size();
                if (rel + 1 == levels && trie[kid].inner()) n_sinks++;
            }
        }
        region[rel & 1] = std::max(region[rel & 1], level_dw);
        cur.swap(nxt);
        if (cur.empty()) break;
    }
    // + one table dword per array (+ 1 for the 8-byte alignment of what follows) + the sink descriptors
    return region[0] + region[1] + n_arrays * 16 + n_entries * TK_NODE_DW + n_arrays + 1 + n_sinks * TK_SINK_DW;
}

// levels of the pass below `root`: as many as fit the budget, at least one
int choose_levels(const std::vector<HNode>& trie, int root, int budget_dw, int max_levels)
{
    const int h = height(trie, root);
    int levels = 1;
    while (levels < std::min(h, max_levels) && subtree_lds(trie, root, levels + 1) <= budget_dw) levels++;
    return levels;
}

// A stage's output arms, as indices into the subtree's array list (-1: none): even, plain odd (for a centre child),
// alternating-sign odd (for lower/upper children).  place_lds turns them into LDS offsets.
struct Arms { int E[2] = { -1, -1 }, O[2] = { -1, -1 }, A[2] = { -1, -1 }; };

// Windows are allocated per producer level inside region (level & 1), region-relative until place_lds.
struct Regions { int used[2] = { 0, 0 }, size[2] = { 0, 0 }, level = 0; };

int take_array(std::vector<TkArray>& arrays, int array_base, Regions& rg, int rel, int bias)
{
    const int len = arm_len(rel), r = rel & 1;
    arrays.push_back(TkArray{ rg.used[r], len, r, bias });   // store: region id for now
    rg.used[r] += len; rg.size[r] = std::max(rg.size[r], rg.used[r]);
    return (int)arrays.size() - 1 - array_base;
}

// the arms node `nd` writes at `rel` levels below the subtree root: none on the pass's last level (`inner` false) or for a leaf
Arms alloc_arms(const HNode& nd, int rel, bool inner, bool mfma, int array_base, Regions& rg, std::vector<TkArray>& arrays)
{
    Arms a;
    if (!inner || !nd.inner()) return a;
    if (rel != rg.level) { rg.level = rel; rg.used[rel & 1] = 0; }
    // an odd arm read by an MFMA level holds x ^ 0x0080 (hb_mfma.hpp): the consumers of an array sit one level down
    const int bias = level_is_mfma(mfma, rel + 1) ? 1 : 0;
    for (int q = 0; q < 2; q++) a.E[q] = take_array(arrays, array_base, rg, rel, 0);
    if (nd.has_centre()) for (int q = 0; q < 2; q++) a.O[q] = take_array(arrays, array_base, rg, rel, bias);
    if (nd.has_lu()) for (int q = 0; q < 2; q++) a.A[q] = take_array(arrays, array_base, rg, rel, bias);
    return a;
}

// One stage's output side: arms, centre taps, sinks -- every channel that ends there, and a node stream of the next pass
// where the tree goes on below this one (`pass_end`).
void fill_out(TkOut& o, int m, int kid, const Arms& own, bool pass_end, int pass, const std::vector<HNode>& trie, BankPlan& plan)
{
    o.present = 1;
    o.outE_I = own.E[0]; o.outE_Q = own.E[1];
    o.outO_I = own.O[0]; o.outO_Q = own.O[1];
    o.outA_I = own.A[0]; o.outA_Q = own.A[1];
    if (m == SDRX_MODE_CENTER) { o.cIe = pk16(0, 2048); o.cIo = pk16(2048, 0); o.cQe = pk16(0, 2048); o.cQo = pk16(2048, 0); }
    else {
        const int sg = m == SDRX_MODE_LOWER ? 1 : -1;
        // lower: k odd -> (-im, re), k even -> (im, -re); upper: the negation
        o.cIo = pk16(-2048 * sg, 0); o.cQo = pk16(2048 * sg, 0);
        o.cIe = pk16(0, 2048 * sg);  o.cQe = pk16(0, -2048 * sg);
    }
    const int depth = trie[kid].depth;
    o.sink = -1;
    for (int c : trie[kid].ends) {
        plan.sinks.push_back(PlanSink{ 0, c, -1, depth, o.sink });
        o.sink = (int)plan.sinks.size() - 1;
    }
    if (pass_end && trie[kid].inner()) {
        PlanStream ms; ms.trie_node = kid; ms.depth = depth; ms.pass = pass + 1;
        plan.sinks.push_back(PlanSink{ 1, -1, (int)plan.streams.size(), depth, o.sink });
        o.sink = ms.sink = (int)plan.sinks.size() - 1;
        plan.streams.push_back(ms);
    }
}

// The table entries of one parent's children (arms `own`, reading the parent's arms `pa`): a centre stage, and the lower and
// upper siblings fused into one entry -- they read the same alternating-sign odd arm and differ only in the centre tap
// (a = first present, b = the other).  Returns the number of entries.
int add_entries(const HNode& parent, const Arms& pa, const Arms own[3], bool pass_end, int pass, const std::vector<HNode>& trie,
                BankPlan& plan)
{
    const int* kid = parent.child;
    int n = 0;
    if (kid[SDRX_MODE_CENTER] >= 0) {
        TkNode nd; memset(&nd, 0xff, sizeof nd);
        nd.oddI = pa.O[0]; nd.oddQ = pa.O[1]; nd.cenI = pa.E[0]; nd.cenQ = pa.E[1];
        fill_out(nd.a, SDRX_MODE_CENTER, kid[SDRX_MODE_CENTER], own[SDRX_MODE_CENTER], pass_end, pass, trie, plan);
        nd.b.present = 0; nd.mode_a = SDRX_MODE_CENTER;
        plan.nodes.push_back(nd); n++;
    }
    if (parent.has_lu()) {
        TkNode nd; memset(&nd, 0xff, sizeof nd);
        nd.oddI = pa.A[0]; nd.oddQ = pa.A[1]; nd.cenI = pa.E[1]; nd.cenQ = pa.E[0];   // I <- eQ, Q <- eI
        nd.b.present = 0;
        nd.mode_a = kid[SDRX_MODE_LOWER] >= 0 ? SDRX_MODE_LOWER : SDRX_MODE_UPPER;
        fill_out(nd.a, nd.mode_a, kid[nd.mode_a], own[nd.mode_a], pass_end, pass, trie, plan);
        if (nd.mode_a == SDRX_MODE_LOWER && kid[SDRX_MODE_UPPER] >= 0)
            fill_out(nd.b, SDRX_MODE_UPPER, kid[SDRX_MODE_UPPER], own[SDRX_MODE_UPPER], pass_end, pass, trie, plan);
        plan.nodes.push_back(nd); n++;
    }
    return n;
}

// Absolute layout: [region 0][region 1][history store: 16 dwords per array][node table]; every array index in the
// subtree's record and entries becomes the array's LDS dword offset.
void place_lds(TkSubtree& st, const Regions& rg, const Arms& root, std::vector<TkArray>& arrays, std::vector<TkNode>& nodes)
{
    const int reg_base[2] = { 0, rg.size[0] };
    st.store_base = rg.size[0] + rg.size[1];
    st.node_tab = st.store_base + 16 * st.n_arrays;
    TkArray* arr = arrays.data() + st.array_base;
    for (int i = 0; i < st.n_arrays; i++) { arr[i].off += reg_base[arr[i].store]; arr[i].store = st.store_base + 16 * i; }
    auto fix = [arr](int v) { return v >= 0 ? arr[v].off : v; };
    st.rootE_I = fix(root.E[0]); st.rootE_Q = fix(root.E[1]);
    st.rootO_I = fix(root.O[0]); st.rootO_Q = fix(root.O[1]);
    st.rootA_I = fix(root.A[0]); st.rootA_Q = fix(root.A[1]);
    for (int i = 0; i < st.n_nodes; i++) {
        TkNode& nd = nodes[(size_t)(st.node_base + i)];
        for (int* v : { &nd.oddI, &nd.oddQ, &nd.cenI, &nd.cenQ }) *v = fix(*v);
        for (TkOut* o : { &nd.a, &nd.b }) {
            if (!o->present) continue;
            for (int* v : { &o->outE_I, &o->outE_Q, &o->outO_I, &o->outO_Q, &o->outA_I, &o->outA_Q }) *v = fix(*v);
        }
    }
}

// one child of a matrix-core job: LDS byte addresses of its arm windows at block tb; absent arms of a present child, and every
// arm of an absent one, go to the scratch slot `trash`
TkMOut job_out(const TkOut* o, int tb, int trash)
{
    if (!o) return TkMOut{ trash * 4, trash * 4, trash * 4, trash * 4, trash * 4, trash * 4, -1, 0 };
    auto at = [=](int off) { return (off >= 0 ? off + HIST / 2 + 64 * tb : trash) * 4; };
    return TkMOut{ at(o->outE_I), at(o->outE_Q), at(o->outO_I), at(o->outO_Q), at(o->outA_I), at(o->outA_Q), o->sink,
                   (o->outE_I >= 0 ? 1 : 0) | (o->outO_I >= 0 ? 2 : 0) | (o->outA_I >= 0 ? 4 : 0) };
}

// Matrix-core jobs of the subtree's MFMA levels: 256 tb outputs into the chunk of one entry each.  64 dwords of scratch
// behind the tables take the stores to arm arrays a child does not have.
void build_mjobs(TkSubtree& st, const std::vector<TkNode>& nodes, std::vector<TkMJob>& mjobs)
{
    const int trash = (st.lds_dwords + 3) & ~3;
    bool any = false;
    // the common inner job -- a lower/upper pair whose two children are inner nodes with ONE kind of odd arm and no sink --
    // gets a branch-free epilogue (tree_kernel.hpp): the odd target moves into O_I / O_Q whatever its kind, `kinds` says which
    // children want the alternating-sign copy
    // (the same treatment for single-child pairs and centre stages measured SLOWER, 3.22 vs 3.13 ms: three more inlined store groups
    // in both the paired and the single job body)
    // (nor did sending single-child pairs down this path with the absent child's stores going to the scratch slot: 3.15 vs 3.13)
    auto one_odd = [](const TkMOut& m) { return m.sink < 0 && (m.flags == (1 | 2) || m.flags == (1 | 4)); };
    for (int l = 0; l < st.n_levels; l++) {
        TkLevel& lv = st.lv[l];
        if (!lv.mfma) continue;
        any = true;
        lv.mjob_base = (int)mjobs.size();
        for (int e = 0; e < lv.n_nodes; e++) {
            const TkNode& nd = nodes[(size_t)(st.node_base + lv.node_base + e)];
            for (int tb = 0; tb < lv.nout / 256; tb++) {
                TkMJob j; memset(&j, 0, sizeof j);
                j.bI = (nd.oddI + 4 + 128 * tb) * 4; j.bQ = (nd.oddQ + 4 + 128 * tb) * 4;
                j.cI = (nd.cenI + 10 + 128 * tb) * 4; j.cQ = (nd.cenQ + 10 + 128 * tb) * 4;
                j.mode = nd.mode_a == SDRX_MODE_CENTER ? 0 : 1;
                j.out0 = 256 * tb;
                if (nd.mode_a == SDRX_MODE_UPPER) { j.o[0] = job_out(nullptr, tb, trash); j.o[1] = job_out(&nd.a, tb, trash); }
                else { j.o[0] = job_out(&nd.a, tb, trash); j.o[1] = job_out(nd.b.present ? &nd.b : nullptr, tb, trash); }
                if (j.mode && one_odd(j.o[0]) && one_odd(j.o[1])) {
                    j.fast = 1; j.kinds = ((j.o[0].flags & 4) ? 1 : 0) | ((j.o[1].flags & 4) ? 2 : 0);
                    for (TkMOut* m : { &j.o[0], &j.o[1] }) if (m->flags & 4) { m->O_I = m->A_I; m->O_Q = m->A_Q; }
                }
                mjobs.push_back(j);
            }
        }
        lv.n_mjobs = (int)mjobs.size() - lv.mjob_base;
    }
    if (any) st.lds_dwords = trash + 64;
}

// The history walk's address arithmetic (tree_kernel.hpp): a level's arrays are contiguous, of one length, slots in array
// order.  Fills in the level records' walk fields and checks that the layout is that.
std::string level_walk(TkSubtree& st, const std::vector<TkArray>& arrays)
{
    const TkArray* arr = arrays.data() + st.array_base;
    for (int l = 0; l < st.n_levels; l++) {
        TkLevel& lv = st.lv[l];
        lv.in_len = arm_len(l);
        const int pb = l == 0 ? 0 : st.lv[l - 1].arr_base, pc = l == 0 ? st.root_arr_cnt : st.lv[l - 1].arr_cnt;
        lv.prev_arr_cnt = pc;
        lv.prev_off = pc ? arr[pb].off : 0;
        lv.arr_off = lv.arr_cnt ? arr[lv.arr_base].off : 0;
        lv.arr_len = lv.arr_cnt ? arr[lv.arr_base].len : 0;
        if (pb + pc != lv.arr_base) return "internal: level arrays not in order";
        for (int k = 0; k < lv.arr_cnt; k++) {
            const TkArray& a = arr[lv.arr_base + k];
            if (a.off != lv.arr_off + k * lv.arr_len || a.len != lv.arr_len || a.store != st.store_base + 16 * (lv.arr_base + k))
                return "internal: level arrays not contiguous";
        }
        for (int k = 0; k < pc; k++) {
            const TkArray& a = arr[pb + k];
            if (a.off != lv.prev_off + k * lv.in_len || a.len != lv.in_len) return "internal: parent arrays not contiguous";
        }
    }
    st.root_off = st.root_arr_cnt ? arr[0].off : 0;
    st.root_len = st.root_arr_cnt ? arr[0].len : 0;
    return {};
}

// The subtree of `levels` levels below stream si's trie node: its record, entries, arrays, sinks, matrix-core jobs, and the
// node streams it writes for the next pass.
std::string plan_subtree(const std::vector<HNode>& trie, int si, int levels, const PlanOptions& opt, BankPlan& plan)
{
    const int root = plan.streams[(size_t)si].trie_node, pass = plan.streams[(size_t)si].pass;
    TkSubtree st; memset(&st, 0, sizeof st);
    st.n_levels = levels;
    st.warm = std::max(1, (int)((46L * ((1L << levels) - 1) + TK_CHUNK - 1) / TK_CHUNK));
    plan.streams[(size_t)si].hist_len = (long)(st.warm + 1) * TK_CHUNK;
    st.sink_base = (int)plan.sinks.size();
    st.node_base = (int)plan.nodes.size();
    st.array_base = (int)plan.arrays.size();
    st.root_xm = level_is_mfma(opt.mfma, 1) ? HBM_BIAS2 : 0u;
    st.dbg = opt.dbg;

    Regions rg;
    std::vector<int> cur{ root };
    std::vector<Arms> cur_arms{ alloc_arms(trie[root], 0, true, opt.mfma, st.array_base, rg, plan.arrays) };
    const Arms root_arms = cur_arms[0];
    st.root_arr_cnt = (int)plan.arrays.size() - st.array_base;
    for (int rel = 1; rel <= levels; rel++) {
        TkLevel& lv = st.lv[rel - 1];
        lv.node_base = st.n_nodes;
        lv.nout = TK_CHUNK >> rel;
        lv.mfma = level_is_mfma(opt.mfma, rel) ? 1 : 0;
        lv.xm = rel < levels && level_is_mfma(opt.mfma, rel + 1) ? HBM_BIAS2 : 0u;
        lv.arr_base = (int)plan.arrays.size() - st.array_base;
        std::vector<int> nxt; std::vector<Arms> nxt_arms;
        for (size_t pi = 0; pi < cur.size(); pi++) {
            const HNode& parent = trie[(size_t)cur[pi]];
            Arms own[3];
            for (int m = 0; m < 3; m++) {
                if (parent.child[m] < 0) continue;
                own[m] = alloc_arms(trie[(size_t)parent.child[m]], rel, rel < levels, opt.mfma, st.array_base, rg, plan.arrays);
                nxt.push_back(parent.child[m]); nxt_arms.push_back(own[m]);
            }
            lv.n_nodes += add_entries(parent, cur_arms[pi], own, rel == levels, pass, trie, plan);
        }
        st.n_nodes += lv.n_nodes;
        lv.arr_cnt = (int)plan.arrays.size() - st.array_base - lv.arr_base;
        // outputs per job: 8 while that gives every lane of the workgroup a job, else 4, else 2 (a level costs one job time)
        lv.r_log2 = 3;
        while (lv.r_log2 > 1 && (long)lv.n_nodes * (lv.nout >> lv.r_log2) < TK_THREADS) lv.r_log2--;
        while (((1 << lv.r_log2) << lv.jobs_log2) < lv.nout) lv.jobs_log2++;
        cur.swap(nxt); cur_arms.swap(nxt_arms);
    }
    st.n_arrays = (int)plan.arrays.size() - st.array_base;
    st.n_sinks = (int)plan.sinks.size() - st.sink_base;

    place_lds(st, rg, root_arms, plan.arrays, plan.nodes);
    for (int i = 0; i < st.n_arrays; i++) {
        // the matrix-core levels read their windows as aligned 16-byte vectors
        const TkArray& a = plan.arrays[(size_t)(st.array_base + i)];
        if (a.bias && (a.off & 3)) return "internal: MFMA window not 16-byte aligned";
    }
    st.sink_tab = (st.node_tab + st.n_nodes * TK_NODE_DW + 1) & ~1;      // 8-byte aligned: read as uint2
    st.lds_dwords = st.sink_tab + st.n_sinks * TK_SINK_DW;
    build_mjobs(st, plan.nodes, plan.mjobs);
    if (st.lds_dwords > LDS_MAX_DW) return "channel tree does not fit LDS";     // tables and the job scratch on top of the arm regions
    std::string err = level_walk(st, plan.arrays);
    if (!err.empty()) return err;

    plan.streams[(size_t)si].subtree = (int)plan.subtrees.size();
    plan.subtrees.push_back(st);
    if ((int)plan.passes.size() <= pass) plan.passes.resize((size_t)pass + 1);
    plan.passes[(size_t)pass].push_back(si);
    if (opt.debug) {
        int nj = 0, nf = 0;
        for (int l = 0; l < levels; l++)
            for (int q = 0; q < st.lv[l].n_mjobs; q++) { nj++; nf += plan.mjobs[(size_t)(st.lv[l].mjob_base + q)].fast; }
        fprintf(stderr, "sdrx plan: pass %d stream %d (trie node %d, depth %d): %d levels, %d entries, %d arrays, %d LDS dwords (regions %d + %d), %d matrix-core jobs per chunk (%d branch-free)\n",
                pass, si, root, plan.streams[(size_t)si].depth, levels, st.n_nodes, st.n_arrays, st.lds_dwords, rg.size[0], rg.size[1], nj, nf);
    }
    return {};
}

} // namespace

// Build the trie, cut it into passes, lay out LDS, fill the tables.  Every stream that has a subtree below it is planned in
// creation order; a subtree's node streams join the list as the next pass.
std::string plan_bank(const std::vector<PlanChain>& chains, const PlanOptions& opt, BankPlan& plan)
{
    plan = BankPlan{};
    plan.mfma = opt.mfma;
    const std::vector<HNode> trie = build_trie(chains);
    const int budget = lds_budget_dw(opt, chains.size());
    plan.streams.emplace_back();                            // the raw stream: trie root, depth 0, pass 0
    for (size_t si = 0; si < plan.streams.size(); si++) {
        const int root = plan.streams[si].trie_node;
        if (height(trie, root) == 0) continue;
        const int levels = choose_levels(trie, root, budget, opt.max_levels);
        if (subtree_lds(trie, root, levels) > LDS_HARD_DW) return "channel tree does not fit LDS";
        std::string err = plan_subtree(trie, (int)si, levels, opt, plan);
        if (!err.empty()) return err;
    }
    return {};
}

} // namespace sdrx
