// libsdrx.so: lowering of the bank plan's matrix-core jobs for tree_mx_kernel (chan_lower.hpp).  Host code only, no HIP
// headers; sdrx_chan.hip compiles it in next to the planner.
#include "chan_lower.hpp"
#include "chan_plan.hpp"
#include <algorithm>

namespace sdrx {

bool subtree_all_mx(const TkSubtree& st)
{
    if (st.n_levels < 1 || st.n_levels > MX_MAX_LEVELS) return false;
    for (int l = 0; l < st.n_levels; l++) if (!st.lv[l].mfma) return false;
    return true;
}

namespace {

// one job; `PI` / `PO` = byte pitch of the arrays the level reads / writes
std::string lower_job(const TkMJob& j, int PI, int PO, TkLJob& r)
{
    r.b = j.bI; r.c = j.mode ? j.cQ : j.cI; r.out0 = j.out0;
    if (j.bQ != j.bI + PI) return "lower: odd arms not one pitch apart";
    if ((j.mode ? j.cI - j.cQ : j.cQ - j.cI) != PI) return "lower: even arms not one pitch apart";
    bool sink = false;
    int meta = 0;
    for (int k = 0; k < 2; k++) {
        const TkMOut& m = j.o[k];
        const int f = m.flags;
        r.sink[k] = m.sink;
        sink |= m.sink >= 0;
        if (f != 0 && f != (1 | 2) && f != (1 | 4) && f != (1 | 2 | 4)) return "lower: unexpected arm set";
        r.o[k] = f ? m.E_I : 0;
        if (f) {
            // the odd arm at 2 PO whatever its kind (a fast job's O_I already holds the alternating copy's address); a child with
            // both kinds has the alternating copy at 4 PO
            if (m.E_Q != m.E_I + PO) return "lower: even arms of a child not one pitch apart";
            const int odd_I = (f & 2) || j.fast ? m.O_I : m.A_I, odd_Q = (f & 2) || j.fast ? m.O_Q : m.A_Q;
            if (odd_I != m.E_I + 2 * PO || odd_Q != m.E_I + 3 * PO) return "lower: odd arm of a child not at 2 pitches";
            if (f == 7 && (m.A_I != m.E_I + 4 * PO || m.A_Q != m.E_I + 5 * PO)) return "lower: alternating arm of a child not at 4 pitches";
        }
        meta |= f << (4 + 4 * k);
    }
    if (!j.mode && (j.o[1].flags || j.o[1].sink >= 0)) return "lower: centre stage with a second child";
    if (j.fast && sink) return "lower: branch-free job with a sink";
    const int cls = j.fast ? MX_FAST : sink ? MX_SINK : MX_ARMS;
    if (j.mode) meta |= MX_LU_BIT;
    r.meta = meta | cls;
    return {};
}

// the root arms: which kinds there are, and that they sit where the kernel's root fill and root history copy will look for them
std::string lower_root(const TkSubtree& st, const TkArray* arr, TkLRoot& r)
{
    const int P = mx_pitch(0) / 4;                          // the tables count dwords
    r.base = 4 * st.rootE_I;
    r.kinds = (st.rootO_I >= 0 ? MX_ROOT_O : 0) | (st.rootA_I >= 0 ? MX_ROOT_A : 0);
    // the kernel takes every array length from mx_pitch(), a constant of the level, not from the tables
    if (st.root_len != P) return "lower: root arrays of another length";
    if (!r.kinds) return "lower: root without odd arms";       // a root is an inner node: alloc_arms gives it O, A or both
    if (st.rootE_I < 0 || st.rootE_I != st.root_off || st.rootE_Q != st.rootE_I + P) return "lower: root even arms not at the window's start";
    if ((st.rootO_I >= 0) != (st.rootO_Q >= 0) || (st.rootA_I >= 0) != (st.rootA_Q >= 0)) return "lower: half a root odd arm";
    int at = st.rootE_I + 2 * P;
    if (r.kinds & MX_ROOT_O) { if (st.rootO_I != at || st.rootO_Q != at + P) return "lower: root odd arms not at 2 pitches"; at += 2 * P; }
    if (r.kinds & MX_ROOT_A) { if (st.rootA_I != at || st.rootA_Q != at + P) return "lower: root alternating arms not behind the others"; }
    if (st.root_arr_cnt != mx_root_arrays(r.kinds)) return "lower: unexpected root array count";
    // the root histories: the first slots, in arm order
    for (int k = 0; k < st.root_arr_cnt; k++)
        if (arr[k].off != st.rootE_I + k * P || arr[k].len != P || arr[k].store != st.store_base + 16 * k) return "lower: root history slots not in arm order";
    return {};
}

// The history copies of a level's tail jobs (chan_lower.hpp: MX_TAIL_BIT).  `jobs`: the level's lowered jobs.  Marks the last job
// of every entry that has arrays and checks what the kernel relies on: the job's arrays are one run of the level's arrays, PO
// bytes apart, their slots 16 dwords apart in the same order, and every array of the level belongs to exactly one tail job.
std::string mark_tails(const TkSubtree& st, const TkLevel& lv, const TkArray* arr, int PO, std::vector<TkLJob>& jobs)
{
    if (lv.nout < 256 || lv.nout % 256) return "lower: a level with part of a job per entry";
    if (lv.arr_cnt && (lv.arr_len * 4 != PO || lv.arr_len < 16 + 64)) return "lower: level arrays of another length";
    std::vector<int> owner((size_t)lv.arr_cnt, 0);
    // what the level reads and what it produces are two runs of arrays that do not meet: no job reads a head of this phase's arrays
    const int rd0 = 4 * lv.prev_off, rd1 = rd0 + 4 * lv.prev_arr_cnt * lv.in_len, wr0 = 4 * lv.arr_off, wr1 = wr0 + lv.arr_cnt * PO;
    if (lv.arr_cnt && rd0 < wr1 && wr0 < rd1) return "lower: a level that reads the arrays it produces";
    for (TkLJob& r : jobs) {
        const int f0 = mx_flags(r.meta, 0), f1 = mx_flags(r.meta, 1), n0 = mx_arm_arrays(f0), n = n0 + mx_arm_arrays(f1);
        if (r.out0 < 0 || r.out0 > lv.nout - 256 || r.out0 % 256) return "lower: a job off the entry's job grid";
        if (r.b < rd0 || r.b >= rd1 || r.c < rd0 || r.c >= rd1) return "lower: a job that reads outside the level's input arrays";
        // a job's 64 dwords per array sit at out0 bytes behind the 16-dword head of an array of the level: only the entry's last job
        // reaches the array's tail, and no job stores into a head
        for (int k = 0; k < 2; k++) {
            const int at = r.o[k] - 4 * (HIST / 2) - r.out0 - wr0;
            if (mx_flags(r.meta, k) && (at < 0 || at % PO || at + mx_arm_arrays(mx_flags(r.meta, k)) * PO > wr1 - wr0)) return "lower: child arms off the level's array grid";
        }
        if (r.out0 != lv.nout - 256 || !n) continue;
        // the window of the first array: the job's first block is entry HIST / 2 + out0 / 4 of it, and the job ends the window
        const int head = (f0 ? r.o[0] : r.o[1]) + 256 - PO;
        if (head != (f0 ? r.o[0] : r.o[1]) - 4 * (HIST / 2) - r.out0) return "lower: a tail job that does not end its arrays";
        if (f0 && f1 && r.o[1] != r.o[0] + n0 * PO) return "lower: children of a pair not back to back";
        if (head < 4 * lv.arr_off || (head - 4 * lv.arr_off) % PO) return "lower: child arms off the level's array grid";
        const int k0 = (head - 4 * lv.arr_off) / PO, a0 = lv.arr_base + k0;
        if (k0 + n > lv.arr_cnt || a0 > MX_SLOT_MASK) return "lower: child arms outside the level's arrays";
        for (int k = k0; k < k0 + n; k++) {
            const TkArray& a = arr[lv.arr_base + k];
            if (a.off * 4 != head + (k - k0) * PO || a.len * 4 != PO || a.store != st.store_base + 16 * (lv.arr_base + k)) return "lower: history slots not in array order";
            owner[(size_t)k]++;
        }
        r.meta |= MX_TAIL_BIT | (a0 << MX_SLOT_SHIFT) | (int)((uint32_t)n << MX_CNT_SHIFT);
    }
    for (int c : owner) if (c != 1) return "lower: an array without exactly one tail job";
    return {};
}

// one subtree's levels into out.jobs / out.src (their index range, sorted by class inside each level)
std::string lower_subtree(const BankPlan& plan, const TkSubtree& st, LoweredBank& out)
{
    std::string err;
    const TkArray* arr = plan.arrays.data() + st.array_base;
    for (int l = 0; l < st.n_levels; l++) {
        const TkLevel& lv = st.lv[l];
        const int PI = mx_pitch(l), PO = mx_pitch(l + 1);
        if (lv.in_len * 4 != PI || (lv.arr_cnt && lv.arr_len * 4 != PO)) return "lower: level arrays of another length";
        std::vector<std::pair<int, int>> order;             // (class, job)
        std::vector<TkLJob> lowered((size_t)lv.n_mjobs);
        for (int q = 0; q < lv.n_mjobs; q++) {
            const int i = lv.mjob_base + q;
            err = lower_job(plan.mjobs[(size_t)i], PI, PO, lowered[(size_t)q]);
            if (!err.empty()) return err;
            order.emplace_back(mx_class(lowered[(size_t)q].meta), q);
        }
        err = mark_tails(st, lv, arr, PO, lowered);
        if (!err.empty()) return err;
        std::stable_sort(order.begin(), order.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.first < b.first; });
        for (int q = 0; q < lv.n_mjobs; q++) {
            out.jobs[(size_t)(lv.mjob_base + q)] = lowered[(size_t)order[(size_t)q].second];
            out.src[(size_t)(lv.mjob_base + q)] = lv.mjob_base + order[(size_t)q].second;
        }
    }
    return {};
}

} // namespace

std::string lower_bank(const BankPlan& plan, LoweredBank& out)
{
    out = LoweredBank{};
    out.jobs.resize(plan.mjobs.size());
    out.src.resize(plan.mjobs.size());
    for (size_t i = 0; i < plan.mjobs.size(); i++) out.src[i] = (int)i;
    // a subtree the lean kernel cannot take (a level off the matrix cores, or a layout the lowering does not recognise) keeps
    // tree_kernel<true> for its pass: the first such layout is reported, the bank is planned all the same
    std::string first_err;
    std::vector<uint8_t> sub_mx(plan.subtrees.size(), 0);
    out.roots.assign(plan.subtrees.size(), TkLRoot{ 0, -1 });
    for (size_t s = 0; s < plan.subtrees.size(); s++) {
        const TkSubtree& st = plan.subtrees[s];
        if (!plan.mfma || !subtree_all_mx(st)) continue;
        TkLRoot root;
        std::string err = lower_root(st, plan.arrays.data() + st.array_base, root);
        if (err.empty()) err = lower_subtree(plan, st, out);
        if (err.empty()) out.roots[s] = root;
        if (err.empty()) sub_mx[s] = 1;
        else if (first_err.empty()) first_err = err;
    }
    out.pass_mx.assign(plan.passes.size(), 0);
    for (size_t p = 0; p < plan.passes.size(); p++) {
        bool all = !plan.passes[p].empty();
        for (int si : plan.passes[p]) {
            const int s = plan.streams[(size_t)si].subtree;
            all = all && s >= 0 && sub_mx[(size_t)s];
        }
        out.pass_mx[p] = plan.mfma && all ? 1 : 0;
    }
    return first_err;
}

} // namespace sdrx
