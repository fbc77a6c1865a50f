// libsdrx.so: sdrx_chan_* -- a bank of DownChannelizers fed from one device stream
// (reference: sdrbase/dsp/downchannelizer.{h,cpp}).  Device state + launches; planner in chan_plan.cpp, kernels in tree_kernel.hpp
// and (passes whose every level is a matrix-core level, jobs lowered by chan_lower.cpp) tree_mx_kernel.hpp.
#include "sdrx_common.hpp"
#include "chan_plan.hpp"
#include "tree_kernel.hpp"
#include "tree_mx_kernel.hpp"
#include <vector>
#include <cstring>
#include <new>
#include <algorithm>
// The planner is host-only code of its own (tests compile it with g++ alone); it is built as part of this translation unit
// so that the bank's host code, planner included, stands on sdrx_common + sdrx_chan (the host-slice sanitizer build)
#include "chan_plan.cpp"
#include "chan_lower.cpp"

using namespace sdrx;

namespace {

struct Channel {
    int32_t out_rate = 0, ofs = 0;
    int n = 0;
    uint8_t modes[32] = { 0 };
    int group = -1;               // -1: pass-through (0 stages) or dead
    bool passthrough = false;
    bool dead = false;            // removed: the index stays reserved, nothing is produced any more
    DevBuf out;                   // device queue of packed Samples
    int64_t avail = 0;            // complex samples queued
    int64_t last_off = 0, last_n = 0;
};

struct StreamBuf {                // device side of a plan stream
    uint32_t* hist[2] = { nullptr, nullptr };   // plan hist_len samples each: the current one and the next
    int cur = 0;
    DevBuf mid;                   // new samples of a node stream (unused for the raw stream)
};

struct Group {
    int index = -1;               // position in sdrx_chan_bank::groups
    int64_t T = 0;                // samples fed since this group's epoch
    std::vector<int> chans;
    BankPlan plan;
    LoweredBank low;              // the plan's matrix-core jobs for tree_mx_kernel, and which passes run it
    std::vector<StreamBuf> bufs;  // one per plan stream
    void* d_static = nullptr;     // subtrees | nodes | arrays | mjobs | lowered jobs | lowered roots
    TkSubtree* d_subtrees = nullptr; TkNode* d_nodes = nullptr; TkArray* d_arrays = nullptr; TkMJob* d_mjobs = nullptr;
    TkLJob* d_ljobs = nullptr;
    TkLRoot* d_lroots = nullptr;
};

} // namespace

struct sdrx_chan_bank {
    HandleCore core;
    int cus = 256;
    int32_t in_rate = 0;
    std::vector<Channel> ch;
    std::vector<Group*> groups;
    DevBuf stage_in;              // host-pointer feeds are staged here
    DevBuf scratch;               // queue compaction
    // per-feed dynamic tables: pinned host ring + device copies
    static constexpr int RING = 4;
    void* h_dyn[RING] = { nullptr, nullptr, nullptr, nullptr };
    void* d_dyn[RING] = { nullptr, nullptr, nullptr, nullptr };
    size_t dyn_cap[RING] = { 0, 0, 0, 0 };
    hipEvent_t dyn_ev[RING] = { nullptr, nullptr, nullptr, nullptr };
    int dyn_next = 0;
};

static void free_group(Group* g)
{
    if (!g) return;
    for (auto& s : g->bufs) { for (uint32_t* h : s.hist) if (h) (void)hipFree(h); s.mid.release(); }
    if (g->d_static) (void)hipFree(g->d_static);
    delete g;
}

// device side of a plan: zeroed histories for every stream and the static tables in one allocation
static int upload_group(sdrx_chan_bank* b, Group* g)
{
    const BankPlan& p = g->plan;
    g->bufs.resize(p.streams.size());
    for (size_t si = 0; si < p.streams.size(); si++) {
        const size_t bytes = (size_t)p.streams[si].hist_len * 4;
        for (uint32_t*& h : g->bufs[si].hist) {
            SDRX_HIP(hipMalloc(reinterpret_cast<void**>(&h), bytes));
            SDRX_HIP(hipMemsetAsync(h, 0, bytes, b->core.stream));
        }
    }
    const size_t b0 = p.subtrees.size() * sizeof(TkSubtree), b1 = p.nodes.size() * sizeof(TkNode), b2 = p.arrays.size() * sizeof(TkArray);
    const size_t b3 = p.mjobs.size() * sizeof(TkMJob), b4 = g->low.jobs.size() * sizeof(TkLJob);
    const size_t b5 = g->low.roots.size() * sizeof(TkLRoot);
    if (b0 + b1 + b2 == 0) return SDRX_OK;
    SDRX_HIP(hipMalloc(&g->d_static, b0 + b1 + b2 + b3 + b4 + b5 + 64));
    char* d = static_cast<char*>(g->d_static);
    g->d_subtrees = reinterpret_cast<TkSubtree*>(d);
    g->d_nodes = reinterpret_cast<TkNode*>(d + b0);
    g->d_arrays = reinterpret_cast<TkArray*>(d + b0 + b1);
    g->d_mjobs = reinterpret_cast<TkMJob*>(d + b0 + b1 + b2);
    g->d_ljobs = reinterpret_cast<TkLJob*>(d + b0 + b1 + b2 + b3);
    g->d_lroots = reinterpret_cast<TkLRoot*>(d + b0 + b1 + b2 + b3 + b4);
    if (b0) SDRX_HIP(hipMemcpy(g->d_subtrees, p.subtrees.data(), b0, hipMemcpyHostToDevice));
    if (b1) SDRX_HIP(hipMemcpy(g->d_nodes, p.nodes.data(), b1, hipMemcpyHostToDevice));
    if (b2) SDRX_HIP(hipMemcpy(g->d_arrays, p.arrays.data(), b2, hipMemcpyHostToDevice));
    if (b3) SDRX_HIP(hipMemcpy(g->d_mjobs, p.mjobs.data(), b3, hipMemcpyHostToDevice));
    if (b4) SDRX_HIP(hipMemcpy(g->d_ljobs, g->low.jobs.data(), b4, hipMemcpyHostToDevice));
    if (b5) SDRX_HIP(hipMemcpy(g->d_lroots, g->low.roots.data(), b5, hipMemcpyHostToDevice));
    return SDRX_OK;
}

static int configure_channel(sdrx_chan_bank* b, int c, int32_t req_rate, int32_t req_fc)
{
    Channel& ch = b->ch[c];
    ch.n = plan_chain(b->in_rate, req_rate, req_fc, ch.modes, MAX_STAGES, &ch.out_rate, &ch.ofs);
    ch.passthrough = ch.n == 0;
    return SDRX_OK;
}

static int new_group(sdrx_chan_bank* b, const std::vector<int>& chans)
{
    if (chans.empty()) return SDRX_OK;
    std::vector<PlanChain> chains;
    for (int c : chans) chains.push_back(PlanChain{ c, b->ch[(size_t)c].n, b->ch[(size_t)c].modes });
    BankPlan plan;
    const std::string err = plan_bank(chains, plan_options_from_env(), plan);
    if (!err.empty()) { set_error(err); return SDRX_EINVAL; }
    // (a pass the lowering does not recognise stays on tree_kernel<true>: not an error)
    LoweredBank low;
    (void)lower_bank(plan, low);
    Group* g = new (std::nothrow) Group;
    if (!g) return SDRX_ENOMEM;
    g->chans = chans;
    g->index = (int)b->groups.size();
    g->plan = std::move(plan);
    g->low = std::move(low);
    int rc = upload_group(b, g);
    if (rc) { free_group(g); return rc; }
    for (int c : chans) b->ch[c].group = g->index;
    b->groups.push_back(g);
    return SDRX_OK;
}

// A group none of whose channels is live any more (every one reconfigured away or removed) is dropped: its kernels,
// table uploads and device buffers would otherwise run / stay until reset.  Pending work on the stream may still read
// the group's buffers, hence the synchronisation.  Groups behind it move down one slot.
static int retire_dead_groups(sdrx_chan_bank* b)
{
    for (size_t gi = 0; gi < b->groups.size();) {
        Group* g = b->groups[gi];
        bool live = false;
        for (int c : g->chans) if (b->ch[(size_t)c].group == g->index) { live = true; break; }
        if (live) { gi++; continue; }
        SDRX_HIP(hipStreamSynchronize(b->core.stream));
        free_group(g);
        b->groups.erase(b->groups.begin() + (long)gi);
        for (size_t k = gi; k < b->groups.size(); k++) {
            const int old = b->groups[k]->index;
            b->groups[k]->index = (int)k;
            for (int c : b->groups[k]->chans) if (b->ch[(size_t)c].group == old) b->ch[(size_t)c].group = (int)k;
        }
    }
    return SDRX_OK;
}

// keep `used` bytes when growing a channel queue
static int grow_keep(sdrx_chan_bank* b, DevBuf& buf, size_t used, size_t need)
{
    if (need <= buf.cap) return SDRX_OK;
    size_t want = buf.cap ? buf.cap : (1 << 16);
    while (want < need) want *= 2;
    void* np = nullptr;
    SDRX_HIP(hipMalloc(&np, want));
    if (used) SDRX_HIP(hipMemcpyAsync(np, buf.p, used, hipMemcpyDeviceToDevice, b->core.stream));
    SDRX_HIP(hipStreamSynchronize(b->core.stream));
    if (buf.p) (void)hipFree(buf.p);
    buf.p = np; buf.cap = want;
    return SDRX_OK;
}

static int dyn_slot(sdrx_chan_bank* b, size_t bytes, int* slot)
{
    const int s = b->dyn_next; b->dyn_next = (b->dyn_next + 1) % sdrx_chan_bank::RING;
    if (b->dyn_ev[s]) SDRX_HIP(hipEventSynchronize(b->dyn_ev[s]));
    else SDRX_HIP(hipEventCreateWithFlags(&b->dyn_ev[s], hipEventDisableTiming));
    if (bytes > b->dyn_cap[s]) {
        size_t want = b->dyn_cap[s] ? b->dyn_cap[s] : 4096; while (want < bytes) want *= 2;
        if (b->h_dyn[s]) (void)hipHostFree(b->h_dyn[s]);
        if (b->d_dyn[s]) (void)hipFree(b->d_dyn[s]);
        b->h_dyn[s] = b->d_dyn[s] = nullptr; b->dyn_cap[s] = 0;
        SDRX_HIP(hipHostMalloc(&b->h_dyn[s], want, hipHostMallocDefault));
        SDRX_HIP(hipMalloc(&b->d_dyn[s], want));
        b->dyn_cap[s] = want;
    }
    *slot = s;
    return SDRX_OK;
}

static int feed_group(sdrx_chan_bank* b, Group* g, const uint32_t* d_in, int64_t n)
{
    const int64_t T0 = g->T, T1 = g->T + n;
    // --- make room in the channel queues and the node-stream buffers
    for (int c : g->chans) {
        Channel& ch = b->ch[c];
        if (ch.group != g->index) continue;                // reconfigured away from this group
        const int64_t add = (T1 >> ch.n) - (T0 >> ch.n);
        int rc = grow_keep(b, ch.out, (size_t)ch.avail * 4, (size_t)(ch.avail + add) * 4 + 64); if (rc) return rc;
    }
    const BankPlan& plan = g->plan;
    for (size_t si = 1; si < plan.streams.size(); si++) {
        const int64_t add = (T1 >> plan.streams[si].depth) - (T0 >> plan.streams[si].depth);
        int rc = g->bufs[si].mid.reserve((size_t)add * 4 + 64); if (rc) return rc;
    }
    // --- dynamic tables: [TkStream x n_streams][TkSink x n_sinks][TkHistJob x n_streams]
    const size_t ns = plan.streams.size(), nk = plan.sinks.size();
    const size_t o_sinks = ns * sizeof(TkStream), o_hist = o_sinks + nk * sizeof(TkSink), total = o_hist + ns * sizeof(TkHistJob);
    int slot; int rc = dyn_slot(b, total, &slot); if (rc) return rc;
    char* hp = static_cast<char*>(b->h_dyn[slot]); char* dp = static_cast<char*>(b->d_dyn[slot]);
    TkStream* hs = reinterpret_cast<TkStream*>(hp);
    TkSink* hk = reinterpret_cast<TkSink*>(hp + o_sinks);
    TkHistJob* hh = reinterpret_cast<TkHistJob*>(hp + o_hist);

    std::vector<long> segs(ns, 0);
    for (size_t si = 0; si < ns; si++) {
        const PlanStream& s = plan.streams[si];
        const StreamBuf& sb = g->bufs[si];
        TkStream& t = hs[si];
        t.hist = sb.hist[sb.cur];
        t.in = si == 0 ? d_in : static_cast<const uint32_t*>(sb.mid.p);
        t.t_old = T0 >> s.depth; t.t_new = T1 >> s.depth;
        t.subtree = s.subtree;
        t.c_first = t.t_old / TK_CHUNK;
        t.c_last = t.t_new > t.t_old ? (t.t_new - 1) / TK_CHUNK : t.c_first - 1;
        t.cps = 1;
        t.hist_len = s.hist_len;
        hh[si] = TkHistJob{ sb.hist[sb.cur], t.in, sb.hist[sb.cur ^ 1], t.t_new - t.t_old, s.hist_len };
    }
    for (size_t k = 0; k < nk; k++) {
        const PlanSink& si = plan.sinks[k];
        TkSink& t = hk[k];
        t.shift = 0; t.next = si.next;
        if (si.kind == 0) {
            Channel& ch = b->ch[si.ch];
            t.lo = T0 >> si.depth; t.hi = T1 >> si.depth;
            // element 0 of the queue's free space <-> absolute index lo; the address of index 0 is only ever used with an offset back into the buffer
            t.ptr0 = reinterpret_cast<uint32_t*>(reinterpret_cast<uintptr_t>(ch.out.p) - (uintptr_t)(4 * (t.lo - ch.avail)));
            t.shift = si.depth;
            if (ch.group != g->index) t.hi = t.lo;         // reconfigured away: still evaluated, not stored
        } else {
            const int depth = plan.streams[(size_t)si.stream].depth;
            t.lo = T0 >> depth; t.hi = T1 >> depth;
            t.ptr0 = reinterpret_cast<uint32_t*>(reinterpret_cast<uintptr_t>(g->bufs[(size_t)si.stream].mid.p) - (uintptr_t)(4 * t.lo));
        }
    }
    // chunks per segment, per pass: ~4 workgroups per CU overall, warm-up overhead <= 1/cps
    for (const std::vector<int>& ps : plan.passes) {
        long total_chunks = 0;
        for (int si : ps) total_chunks += std::max(0L, hs[si].c_last - hs[si].c_first + 1);
        // one round of workgroups (4 per CU) where the feed allows it: rounding DOWN here leaves a few segments for a second,
        // nearly empty round (61.44 M samples: 1072 workgroups for 1024 slots)
        long cps = (total_chunks + (long)b->cus * 4 - 1) / ((long)b->cus * 4);
        cps = std::max(1L, std::min(cps, 256L));
        for (int si : ps) {
            hs[si].cps = (int)cps;
            segs[si] = (std::max(0L, hs[si].c_last - hs[si].c_first + 1) + cps - 1) / cps;
        }
    }
    SDRX_HIP(hipMemcpyAsync(dp, hp, total, hipMemcpyHostToDevice, b->core.stream));
    SDRX_HIP(hipEventRecord(b->dyn_ev[slot], b->core.stream));

    const TkStream* d_streams = reinterpret_cast<const TkStream*>(dp);
    const TkSink* d_sinks = reinterpret_cast<const TkSink*>(dp + o_sinks);
    const TkHistJob* d_hist = reinterpret_cast<const TkHistJob*>(dp + o_hist);
    rc = b->core.timer.begin(b->core.stream); if (rc) return rc;
    for (size_t p = 0; p < plan.passes.size(); p++) {
        // the streams of one pass are contiguous in creation order; launch them as grid.y
        const std::vector<int>& ps = plan.passes[p];
        if (ps.empty()) continue;
        long max_segs = 0;
        for (int si : ps) max_segs = std::max(max_segs, segs[si]);
        if (max_segs == 0) continue;
        const int s0 = ps.front(), cnt = (int)ps.size();
        size_t lds_bytes = 0;                              // per pass: a deep pass must not cost the shallow ones their occupancy
        for (int si : ps) lds_bytes = std::max(lds_bytes, (size_t)plan.subtrees[(size_t)plan.streams[(size_t)si].subtree].lds_dwords * 4);
        // an all-matrix-core pass (every default pass) runs the lean kernel; deeper passes (SDRX_CHAN_MAX_LEVELS / _LDS_KB)
        // have dot2 levels and keep tree_kernel<true>.  Both are the matrix-core engine: last_launch() names it tree_kernel<mfma>.
        if (g->low.pass_mx[p])
            hipLaunchKernelGGL(tree_mx_kernel, dim3((unsigned)max_segs, (unsigned)cnt), dim3(TK_THREADS), lds_bytes, b->core.stream,
                               g->d_subtrees, g->d_arrays, d_streams + s0, d_sinks, g->d_ljobs, g->d_lroots);
        else if (plan.mfma)
            hipLaunchKernelGGL(tree_kernel<true>, dim3((unsigned)max_segs, (unsigned)cnt), dim3(TK_THREADS), lds_bytes, b->core.stream,
                               g->d_subtrees, g->d_nodes, g->d_arrays, d_streams + s0, d_sinks, g->d_mjobs);
        else
            hipLaunchKernelGGL(tree_kernel<false>, dim3((unsigned)max_segs, (unsigned)cnt), dim3(TK_THREADS), lds_bytes, b->core.stream,
                               g->d_subtrees, g->d_nodes, g->d_arrays, d_streams + s0, d_sinks, g->d_mjobs);
        SDRX_HIP(hipGetLastError());
        if (p == 0) b->core.note_launch(plan.mfma ? "tree_kernel<mfma>" : "tree_kernel<valu>", (int)(max_segs * cnt), TK_THREADS, (int)lds_bytes);
    }
    rc = b->core.timer.end(b->core.stream); if (rc) return rc;
    long max_hist = TK_HIST;
    for (const PlanStream& s : plan.streams) max_hist = std::max(max_hist, s.hist_len);
    hipLaunchKernelGGL(tree_hist_kernel, dim3((unsigned)(max_hist / 256), (unsigned)ns), dim3(256), 0, b->core.stream, d_hist);
    SDRX_HIP(hipGetLastError());
    for (StreamBuf& sb : g->bufs) sb.cur ^= 1;
    for (int c : g->chans) {
        Channel& ch = b->ch[c];
        if (ch.group != g->index) continue;
        const int64_t add = (T1 >> ch.n) - (T0 >> ch.n);
        ch.last_off = ch.avail; ch.last_n = add; ch.avail += add;
    }
    g->T = T1;
    return SDRX_OK;
}

static int feed_passthrough(sdrx_chan_bank* b, const uint32_t* d_in, int64_t n)
{
    // no stage at all: DownChannelizer::feed hands the input straight to the sink (downchannelizer.cpp:57-60)
    for (auto& ch : b->ch) {
        if (!ch.passthrough) continue;
        int rc = grow_keep(b, ch.out, (size_t)ch.avail * 4, (size_t)(ch.avail + n) * 4 + 64); if (rc) return rc;
        SDRX_HIP(hipMemcpyAsync(static_cast<uint32_t*>(ch.out.p) + ch.avail, d_in, (size_t)n * 4, hipMemcpyDeviceToDevice, b->core.stream));
        ch.last_off = ch.avail; ch.last_n = n; ch.avail += n;
    }
    return SDRX_OK;
}

extern "C" {

int sdrx_chan_plan(int32_t in_rate, int32_t req_rate, int32_t req_fc, uint8_t* modes, int32_t* out_rate, int32_t* residual_ofs)
{
    if (!modes || !out_rate || !residual_ofs) { set_error("sdrx_chan_plan: null argument"); return SDRX_EINVAL; }
    return plan_chain(in_rate, req_rate, req_fc, modes, MAX_STAGES, out_rate, residual_ofs);
}

int sdrx_chan_bank_create(sdrx_chan_bank_t** out, int device, int32_t in_rate, int32_t n_ch,
                          const int32_t* req_rate, const int32_t* req_fc)
{
    if (!out) { set_error("sdrx_chan_bank_create: null out"); return SDRX_EINVAL; }
    *out = nullptr;
    if (n_ch <= 0 || !req_rate || !req_fc || in_rate <= 0) { set_error("sdrx_chan_bank_create: bad argument"); return SDRX_EINVAL; }
    sdrx_chan_bank* b = new (std::nothrow) sdrx_chan_bank;
    if (!b) return SDRX_ENOMEM;
    int rc = b->core.open(device);
    if (rc) { delete b; return rc; }
    b->in_rate = in_rate; b->cus = device_cu_count(device);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&tree_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&tree_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&tree_mx_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) { sdrx_chan_bank_destroy(b); return hip_fail(e, "hipFuncSetAttribute", __FILE__, __LINE__); }
    b->ch.resize((size_t)n_ch);
    std::vector<int> all;
    for (int c = 0; c < n_ch; c++) {
        configure_channel(b, c, req_rate[c], req_fc[c]);
        if (!b->ch[c].passthrough) all.push_back(c);
    }
    rc = new_group(b, all);
    if (rc) { sdrx_chan_bank_destroy(b); return rc; }
    SDRX_HIP(hipStreamSynchronize(b->core.stream));
    *out = b;
    return SDRX_OK;
}

int sdrx_chan_bank_destroy(sdrx_chan_bank_t* b)
{
    if (!b) return SDRX_OK;
    (void)hipSetDevice(b->core.device);
    if (b->core.stream) (void)hipStreamSynchronize(b->core.stream);
    for (Group* g : b->groups) free_group(g);
    for (auto& c : b->ch) c.out.release();
    b->stage_in.release(); b->scratch.release();
    for (int i = 0; i < sdrx_chan_bank::RING; i++) {
        if (b->h_dyn[i]) (void)hipHostFree(b->h_dyn[i]);
        if (b->d_dyn[i]) (void)hipFree(b->d_dyn[i]);
        if (b->dyn_ev[i]) (void)hipEventDestroy(b->dyn_ev[i]);
    }
    b->core.close();
    delete b;
    return SDRX_OK;
}

int sdrx_chan_bank_info(const sdrx_chan_bank_t* b, int32_t c, int32_t* n_stages, uint8_t* modes, int32_t* out_rate, int32_t* residual_ofs)
{
    if (!b || c < 0 || c >= (int32_t)b->ch.size()) { set_error("sdrx_chan_bank_info: bad channel"); return SDRX_EINVAL; }
    const Channel& ch = b->ch[(size_t)c];
    if (n_stages) *n_stages = ch.n;
    if (modes) memcpy(modes, ch.modes, (size_t)ch.n);
    if (out_rate) *out_rate = ch.out_rate;
    if (residual_ofs) *residual_ofs = ch.ofs;
    return SDRX_OK;
}

int sdrx_chan_bank_reconfigure(sdrx_chan_bank_t* b, int32_t c, int32_t req_rate, int32_t req_fc)
{
    if (!b || c < 0 || c >= (int32_t)b->ch.size()) { set_error("sdrx_chan_bank_reconfigure: bad channel"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    Channel& ch = b->ch[(size_t)c];
    // the old chain keeps being evaluated inside its group (its prefixes are shared) but stops
    // storing; the new chain starts from zero history in a group of its own
    // (freeFilterChain + createFilterChain, downchannelizer.cpp:167-171)
    ch.group = -1; ch.dead = false;                        // (a removed channel comes back with the new configuration)
    configure_channel(b, c, req_rate, req_fc);
    // a group whose last live channel this was (typically the single-channel group of an earlier reconfigure) goes away;
    // dead chains inside a group that still serves others keep being evaluated (shared prefixes) until the next reset
    int rc = retire_dead_groups(b); if (rc) return rc;
    if (ch.passthrough) return SDRX_OK;
    return new_group(b, std::vector<int>{ (int)c });
}

int sdrx_chan_bank_add_channel(sdrx_chan_bank_t* b, int32_t req_rate, int32_t req_fc, int32_t* channel)
{
    if (!b) { set_error("sdrx_chan_bank_add_channel: null bank"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    // a new DownChannelizer next to the existing ones: they keep their histories and queued output
    b->ch.emplace_back();
    const int c = (int)b->ch.size() - 1;
    configure_channel(b, c, req_rate, req_fc);
    if (channel) *channel = c;
    if (b->ch[(size_t)c].passthrough) return SDRX_OK;
    const int rc = new_group(b, std::vector<int>{ c });
    if (rc) { b->ch.pop_back(); if (channel) *channel = -1; }
    return rc;
}

int sdrx_chan_bank_remove_channel(sdrx_chan_bank_t* b, int32_t c)
{
    if (!b || c < 0 || c >= (int32_t)b->ch.size()) { set_error("sdrx_chan_bank_remove_channel: bad channel"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    // the index stays reserved (other channels keep theirs); the chain stops producing and its queue is dropped
    Channel& ch = b->ch[(size_t)c];
    ch.group = -1; ch.passthrough = false; ch.dead = true; ch.n = 0; ch.out_rate = 0; ch.ofs = 0;
    ch.avail = 0; ch.last_off = 0; ch.last_n = 0;
    return retire_dead_groups(b);
}

/* checkpoint of the filter state: per group its sample count and every stream's history (the raw stream and the node
 * streams; the reference's ring buffers are a pure function of them).  Layout: [magic, n_groups] then per group
 * [T, n_streams] and per stream [hist_len, hist_len x 4 bytes].  Queued, unread output is NOT part of it.  A state only
 * fits a bank with the same channels configured in the same order (the same plan): set_state checks the shape. */
static const int64_t CHAN_STATE_MAGIC = 0x7364727863686b31LL;      // "sdrxchk1"

int64_t sdrx_chan_bank_state_bytes(const sdrx_chan_bank_t* b)
{
    if (!b) return SDRX_EINVAL;
    int64_t n = 16;
    for (const Group* g : b->groups) { n += 16; for (const PlanStream& s : g->plan.streams) n += 8 + (int64_t)s.hist_len * 4; }
    return n;
}

int sdrx_chan_bank_get_state(sdrx_chan_bank_t* b, void* host_buf)
{
    if (!b || !host_buf) { set_error("sdrx_chan_bank_get_state: null argument"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    char* p = static_cast<char*>(host_buf);
    auto put = [&](int64_t v) { std::memcpy(p, &v, 8); p += 8; };
    put(CHAN_STATE_MAGIC); put((int64_t)b->groups.size());
    for (Group* g : b->groups) {
        put(g->T); put((int64_t)g->plan.streams.size());
        for (size_t si = 0; si < g->bufs.size(); si++) {
            const long len = g->plan.streams[si].hist_len;
            put(len);
            SDRX_HIP(hipMemcpyAsync(p, g->bufs[si].hist[g->bufs[si].cur], (size_t)len * 4, hipMemcpyDeviceToHost, b->core.stream));
            p += (size_t)len * 4;
        }
    }
    SDRX_HIP(hipStreamSynchronize(b->core.stream));
    return SDRX_OK;
}

int sdrx_chan_bank_set_state(sdrx_chan_bank_t* b, const void* host_buf)
{
    if (!b || !host_buf) { set_error("sdrx_chan_bank_set_state: null argument"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    const char* p = static_cast<const char*>(host_buf);
    auto get = [&]() { int64_t v; std::memcpy(&v, p, 8); p += 8; return v; };
    // first pass: the shape must be this bank's
    const char* q = p;
    bool ok = get() == CHAN_STATE_MAGIC && get() == (int64_t)b->groups.size();
    for (size_t gi = 0; ok && gi < b->groups.size(); gi++) {
        const Group* g = b->groups[gi];
        (void)get();
        const std::vector<PlanStream>& ss = g->plan.streams;
        ok = get() == (int64_t)ss.size();
        for (size_t si = 0; ok && si < ss.size(); si++) { ok = get() == ss[si].hist_len; p += (size_t)ss[si].hist_len * 4; }
    }
    if (!ok) { set_error("sdrx_chan_bank_set_state: the state was taken from a bank with another configuration"); return SDRX_EINVAL; }
    p = q; (void)get(); (void)get();
    SDRX_HIP(hipStreamSynchronize(b->core.stream));
    for (Group* g : b->groups) {
        g->T = get(); (void)get();
        for (size_t si = 0; si < g->bufs.size(); si++) {
            (void)get();
            const size_t bytes = (size_t)g->plan.streams[si].hist_len * 4;
            SDRX_HIP(hipMemcpyAsync(g->bufs[si].hist[g->bufs[si].cur], p, bytes, hipMemcpyHostToDevice, b->core.stream));
            p += bytes;
        }
    }
    SDRX_HIP(hipStreamSynchronize(b->core.stream));
    for (auto& ch : b->ch) { ch.avail = 0; ch.last_off = 0; ch.last_n = 0; }     // the queues belong to the old timeline
    return SDRX_OK;
}

int32_t sdrx_chan_bank_group_count(const sdrx_chan_bank_t* b) { return b ? (int32_t)b->groups.size() : SDRX_EINVAL; }

int sdrx_chan_bank_reset(sdrx_chan_bank_t* b)
{
    if (!b) return SDRX_EINVAL;
    SDRX_HIP(hipSetDevice(b->core.device));
    SDRX_HIP(hipStreamSynchronize(b->core.stream));
    for (Group* g : b->groups) free_group(g);
    b->groups.clear();
    std::vector<int> all;
    for (size_t c = 0; c < b->ch.size(); c++) {
        b->ch[c].avail = 0; b->ch[c].last_n = 0; b->ch[c].group = -1;
        if (!b->ch[c].passthrough && !b->ch[c].dead) all.push_back((int)c);
    }
    return new_group(b, all);
}

int sdrx_chan_bank_feed_dev(sdrx_chan_bank_t* b, const int16_t* d_iq, int64_t n_cplx)
{
    if (!b || n_cplx < 0 || (n_cplx > 0 && !d_iq)) { set_error("sdrx_chan_bank_feed_dev: bad argument"); return SDRX_EINVAL; }
    if (reinterpret_cast<uintptr_t>(d_iq) & 3u) { set_error("sdrx_chan_bank_feed_dev: d_iq must be 4-byte aligned"); return SDRX_EINVAL; }
    if (n_cplx == 0) return SDRX_OK;
    SDRX_HIP(hipSetDevice(b->core.device));
    const uint32_t* in = reinterpret_cast<const uint32_t*>(d_iq);
    int rc = feed_passthrough(b, in, n_cplx); if (rc) return rc;
    for (Group* g : b->groups) { rc = feed_group(b, g, in, n_cplx); if (rc) return rc; }
    return SDRX_OK;
}

int sdrx_chan_bank_feed(sdrx_chan_bank_t* b, const int16_t* iq, int64_t n_cplx)
{
    if (!b || n_cplx < 0 || (n_cplx > 0 && !iq)) { set_error("sdrx_chan_bank_feed: bad argument"); return SDRX_EINVAL; }
    if (n_cplx == 0) return SDRX_OK;
    SDRX_HIP(hipSetDevice(b->core.device));
    SDRX_HIP(hipStreamSynchronize(b->core.stream));            // staging buffer may still be read by the previous feed
    int rc = b->stage_in.reserve((size_t)n_cplx * 4); if (rc) return rc;
    SDRX_HIP(hipMemcpyAsync(b->stage_in.p, iq, (size_t)n_cplx * 4, hipMemcpyHostToDevice, b->core.stream));
    return sdrx_chan_bank_feed_dev(b, static_cast<const int16_t*>(b->stage_in.p), n_cplx);
}

int64_t sdrx_chan_bank_available(sdrx_chan_bank_t* b, int32_t c)
{
    if (!b || c < 0 || c >= (int32_t)b->ch.size()) return SDRX_EINVAL;
    return b->ch[(size_t)c].avail;
}

int64_t sdrx_chan_bank_read(sdrx_chan_bank_t* b, int32_t c, int16_t* out_iq, int64_t cap)
{
    if (!b || c < 0 || c >= (int32_t)b->ch.size() || cap < 0 || (cap > 0 && !out_iq)) { set_error("sdrx_chan_bank_read: bad argument"); return SDRX_EINVAL; }
    if (hipSetDevice(b->core.device) != hipSuccess) return SDRX_EHIP;
    Channel& ch = b->ch[(size_t)c];
    const int64_t n = std::min(cap, ch.avail);
    if (n == 0) return 0;
    hipError_t e = hipMemcpyAsync(out_iq, ch.out.p, (size_t)n * 4, hipMemcpyDeviceToHost, b->core.stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(read)", __FILE__, __LINE__);
    const int64_t rest = ch.avail - n;
    if (rest > 0) {                                        // partial read: compact the queue
        int rc = b->scratch.reserve((size_t)rest * 4); if (rc) return rc;
        e = hipMemcpyAsync(b->scratch.p, static_cast<uint32_t*>(ch.out.p) + n, (size_t)rest * 4, hipMemcpyDeviceToDevice, b->core.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(ch.out.p, b->scratch.p, (size_t)rest * 4, hipMemcpyDeviceToDevice, b->core.stream);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(compact)", __FILE__, __LINE__);
    }
    e = hipStreamSynchronize(b->core.stream);
    if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize", __FILE__, __LINE__);
    ch.avail = rest; ch.last_off = 0; ch.last_n = 0;
    return n;
}

int64_t sdrx_chan_bank_skip(sdrx_chan_bank_t* b, int32_t c, int64_t n)
{
    if (!b || c < 0 || c >= (int32_t)b->ch.size()) { set_error("sdrx_chan_bank_skip: bad argument"); return SDRX_EINVAL; }
    Channel& ch = b->ch[(size_t)c];
    if (n < 0 || n >= ch.avail) { const int64_t k = ch.avail; ch.avail = 0; ch.last_off = 0; ch.last_n = 0; return k; }
    if (n == 0) return 0;
    if (hipSetDevice(b->core.device) != hipSuccess) return SDRX_EHIP;
    const int64_t rest = ch.avail - n;
    int rc = b->scratch.reserve((size_t)rest * 4); if (rc) return rc;
    hipError_t e = hipMemcpyAsync(b->scratch.p, static_cast<uint32_t*>(ch.out.p) + n, (size_t)rest * 4, hipMemcpyDeviceToDevice, b->core.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(ch.out.p, b->scratch.p, (size_t)rest * 4, hipMemcpyDeviceToDevice, b->core.stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(skip)", __FILE__, __LINE__);
    ch.avail = rest; ch.last_off = 0; ch.last_n = 0;
    return n;
}

int sdrx_chan_bank_last_dev(sdrx_chan_bank_t* b, int32_t c, const int16_t** d_out_iq, int64_t* n_cplx)
{
    if (!b || c < 0 || c >= (int32_t)b->ch.size() || !d_out_iq || !n_cplx) { set_error("sdrx_chan_bank_last_dev: bad argument"); return SDRX_EINVAL; }
    Channel& ch = b->ch[(size_t)c];
    *d_out_iq = reinterpret_cast<const int16_t*>(static_cast<uint32_t*>(ch.out.p) + ch.last_off);
    *n_cplx = ch.last_n;
    return SDRX_OK;
}

int sdrx_chan_bank_sync(sdrx_chan_bank_t* b) { return b ? b->core.sync() : SDRX_EINVAL; }

int sdrx_chan_bank_get_stream(sdrx_chan_bank_t* b, void** hip_stream)
{
    if (!b || !hip_stream) { set_error("sdrx_chan_bank_get_stream: null argument"); return SDRX_EINVAL; }
    return b->core.get_stream(hip_stream);
}

int sdrx_chan_bank_set_stream(sdrx_chan_bank_t* b, void* hip_stream) { return b ? b->core.set_stream(hip_stream) : SDRX_EINVAL; }

int sdrx_chan_bank_set_timing(sdrx_chan_bank_t* b, int enabled) { return b ? b->core.set_timing(enabled) : SDRX_EINVAL; }

int sdrx_chan_bank_get_timing(sdrx_chan_bank_t* b, double* total_ms, int64_t* feeds, int reset) { return b ? b->core.get_timing(total_ms, feeds, reset) : SDRX_EINVAL; }

int sdrx_chan_bank_last_launch(const sdrx_chan_bank_t* b, char* kernel_name, int name_cap, int* grid, int* block, int* lds_bytes) { return b ? b->core.last_launch(kernel_name, name_cap, grid, block, lds_bytes) : SDRX_EINVAL; }

} // extern "C"
