// libsdrx.so: sdrx_bfm_* -- N broadcast-FM stereo demodulators (BFMDemod::feed, plugins/channelrx/demodbfm/bfmdemod.cpp:116-281,
// m_rdsActive clear) on one device: int16 I/Q at the channelizer's output rate in, qint16 l, r audio and the sink stream out.
// Kernels: bfm_kernels.hpp.  Host side: the design products as the constructor, applyChannelSettings(force) and
// applySettings(force) leave them (bfmdemod.cpp:50-103, 396-515), launches, buffer bookkeeping: sdrx_wfm.hip's design.
#include "sdrx_common.hpp"
#include "bfm_kernels.hpp"
#include "backend_design.hpp"
#include "demod_common.hpp"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace sdrx;

namespace {

struct BfmHost {
    DevBuf arena;                 // work()'s layout for cap_in samples
    DevBuf stage_in;              // host-pointer feeds
    uint32_t* pend[2] = { nullptr, nullptr };
    int cur = 0;
    int64_t cap_in = 0;
    int pending = 0;              // host mirror of WfmChan::pending (a function of the feed lengths only)
    DevBuf rds_arena;             // rds_work()'s layout for rds_cap samples; channels with RDS on only
    int64_t rds_cap = 0;
};

// One channel's work arena for feeds of up to cap_in samples.  tail's slot 0 (ovlbuf) and the fronts of dem and st (the two
// resamplers' windows) carry state from feed to feed.
void work(Carver& k, int64_t cap_in, BfmBufs& u)
{
    const size_t n_blk = (size_t)(cap_in + WFM_H) / WFM_H + 1;       // pending (< 512) + new
    const size_t n_s = n_blk * WFM_H;
    u.w.head = k.take<float2>(n_s);
    u.w.tail = k.take_kept<float2>(n_s + WFM_H, WFM_H);
    u.w.flag = k.take<uint8_t>(n_s);
    u.w.blk_sum = k.take<double>(n_blk);
    u.w.blk_map = k.take<WfmClamp>(n_blk);
    u.w.blk_peak = k.take<float>(n_blk);
    u.w.blk_state = k.take<int>(n_blk);
    u.w.blk_last = k.take<int>(n_blk + 64 / sizeof(int));
    u.w.dem = k.take_kept<float>(WFM_HIST + n_s + WFM_HIST, WFM_HIST);
    u.st = k.take_kept<float2>(WFM_HIST + n_s + WFM_HIST, WFM_HIST);
    // every audio sample consumes at least one demodulated sample (step >= 1)
    u.w.sched = k.take<uint2>(n_s + 8);
    u.rf = k.take<float2>(n_s);
    u.opn = k.take<uint8_t>(n_s);
    u.blk_prev = k.take<int>(n_blk);
    u.psc = k.take<float2>(n_s);
    u.mix = k.take<float2>(n_s + 8);
    u.sink = k.take<uint32_t>(n_s);
    u.pairs = k.take<short2>(n_s + 8);
}

// RDS's arena of one channel.  Provable per-feed bounds: one RDS sample per filtered sample at most (Interpolator::decimate
// emits once per input or not at all); biphase runs at most once per eighth RDS sample, so bits <= n_rds / 8 + 2; a group
// needs 26 bits at least, so groups <= bits / 26 + 1.
void rds_work(Carver& k, int64_t cap_in, BfmRdsBufs& u)
{
    const size_t n_blk = (size_t)(cap_in + WFM_H) / WFM_H + 1;
    const size_t n_s = n_blk * WFM_H, n_bits = n_s / 8 + 2, n_groups = n_bits / 26 + 1;
    u.ph = k.take<float>(n_s);
    u.rin = k.take_kept<float>(WFM_HIST + n_s + WFM_HIST, WFM_HIST);
    u.sched = k.take<uint2>(n_s + 8);
    u.xv = k.take_kept<float>(RDS_XV_FRONT + n_s + RDS_XV_FRONT, RDS_XV_FRONT);
    u.bb = k.take<float>(n_s);
    u.bits = k.take<uint8_t>(n_bits);
    u.groups = k.take<uint16_t>(4 * n_groups);
}

} // namespace

struct sdrx_bfm {
    HandleCore core;
    int n_ch = 0;
    std::vector<sdrx_bfm_cfg> cfg;
    std::vector<BfmHost> ch;
    std::vector<BfmChan> h_chan;  // configuration and the state of a fresh handle
    BfmChan* d_chan = nullptr;
    BfmBufs* d_bufs = nullptr;
    BfmBufs* h_bufs = nullptr;    // pinned: the per-feed table goes to the device in one async copy
    hipEvent_t bufs_ev = nullptr;
    hipEvent_t prod_ev = nullptr, cons_ev = nullptr;       // device-side ordering against a producer stream (sdrx_bfm_feed_bank)
    float* d_nco = nullptr; float* d_taps = nullptr; float2* d_filters = nullptr; float* d_utbl = nullptr;
    InterpTables taps;
    std::vector<float> filters_all;
    bool any_dyadic = false, any_stereo = false;
    // RDS (sdrx_bfmrds_create): nothing of it exists in a handle without a channel that has it on
    bool any_rds = false, any_rds_stereo = false;
    std::vector<BfmRdsChan> h_rds;          // configuration and the state of a fresh handle
    BfmRdsChan* d_rds = nullptr;
    BfmRdsBufs* d_rbufs = nullptr;
    BfmRdsBufs* h_rbufs = nullptr;          // pinned, as h_bufs
    float* d_rds_taps = nullptr;
    InterpTables rds_taps;
};

static int bad(const char* field, const char* need)
{
    set_error(std::string("sdrx_bfm_create: bad channel configuration: ") + field + " (" + need + ")");
    return SDRX_EINVAL;
}

static int validate(int32_t n_ch, const sdrx_bfm_cfg* cfg)
{
    if (n_ch <= 0 || !cfg) { set_error("sdrx_bfm_create: bad argument"); return SDRX_EINVAL; }
    for (int c = 0; c < n_ch; c++) {
        const sdrx_bfm_cfg& k = cfg[c];
        if (k.in_rate <= 0) return bad("in_rate", "need in_rate > 0");
        if (k.audio_rate <= 0 || k.audio_rate > k.in_rate) return bad("audio_rate", "need 0 < audio_rate <= in_rate");
        if (!(k.rf_bandwidth > 0.0f) || !(k.rf_bandwidth <= 1.0e7f)) return bad("rf_bandwidth", "need 0 < rf_bandwidth <= 1e7");
        if (!(k.af_bandwidth > 0.0f) || !std::isfinite(k.af_bandwidth)) return bad("af_bandwidth", "need a finite af_bandwidth > 0");
        if (!std::isfinite(k.volume)) return bad("volume", "must be finite");
        if (!std::isfinite(k.squelch_db)) return bad("squelch_db", "must be finite");
        if (k.audio_stereo != 0 && k.audio_stereo != 1) return bad("audio_stereo", "0 or 1");
        if (k.lsb_stereo != 0 && k.lsb_stereo != 1) return bad("lsb_stereo", "0 or 1");
        if (k.show_pilot != 0 && k.show_pilot != 1) return bad("show_pilot", "0 or 1");
        // Interpolator::create(16, ...) with 4.5 taps per phase: the window both resamplers carry
        int nt = (int)(4.5 * 16); if (nt % 2) nt++;
        if (nt > WFM_HIST) return bad("af_bandwidth", "the resampler's taps per phase do not fit the carried window");
    }
    return SDRX_OK;
}

static int upload_fresh_state(sdrx_bfm* b)
{
    SDRX_HIP(hipMemcpyAsync(b->d_chan, b->h_chan.data(), (size_t)b->n_ch * sizeof(BfmChan), hipMemcpyHostToDevice, b->core.stream));
    for (auto& h : b->ch) {
        for (int i = 0; i < 2; i++) SDRX_HIP(hipMemsetAsync(h.pend[i], 0, WFM_H * 4, b->core.stream));
        int rc = demod_clear_kept<BfmBufs>(h.arena, h.cap_in, b->core.stream, work); if (rc) return rc;
        h.pending = 0; h.cur = 0;
        if (h.rds_arena.p) { rc = demod_clear_kept<BfmRdsBufs>(h.rds_arena, h.rds_cap, b->core.stream, rds_work); if (rc) return rc; }
    }
    if (b->any_rds) SDRX_HIP(hipMemcpyAsync(b->d_rds, b->h_rds.data(), (size_t)b->n_ch * sizeof(BfmRdsChan), hipMemcpyHostToDevice, b->core.stream));
    SDRX_HIP(hipStreamSynchronize(b->core.stream));
    return SDRX_OK;
}

extern "C" {

int sdrx_bfm_destroy(sdrx_bfm_t* b)
{
    if (!b) return SDRX_OK;
    (void)hipSetDevice(b->core.device);
    if (b->core.stream) (void)hipStreamSynchronize(b->core.stream);
    for (auto& h : b->ch) {
        h.arena.release(); h.stage_in.release(); h.rds_arena.release();
        for (int i = 0; i < 2; i++) if (h.pend[i]) (void)hipFree(h.pend[i]);
    }
    if (b->d_chan) (void)hipFree(b->d_chan);
    if (b->d_bufs) (void)hipFree(b->d_bufs);
    if (b->h_bufs) (void)hipHostFree(b->h_bufs);
    if (b->bufs_ev) (void)hipEventDestroy(b->bufs_ev);
    if (b->prod_ev) (void)hipEventDestroy(b->prod_ev);
    if (b->cons_ev) (void)hipEventDestroy(b->cons_ev);
    if (b->d_nco) (void)hipFree(b->d_nco);
    if (b->d_taps) (void)hipFree(b->d_taps);
    if (b->d_filters) (void)hipFree(b->d_filters);
    if (b->d_utbl) (void)hipFree(b->d_utbl);
    if (b->d_rds) (void)hipFree(b->d_rds);
    if (b->d_rbufs) (void)hipFree(b->d_rbufs);
    if (b->h_rbufs) (void)hipHostFree(b->h_rbufs);
    if (b->d_rds_taps) (void)hipFree(b->d_rds_taps);
    b->core.close();
    delete b;
    return SDRX_OK;
}

static int create_common(sdrx_bfm_t** out, int device, int32_t n_ch, const sdrx_bfm_cfg* cfg, const sdrx_bfmrds_cfg* rds)
{
    if (!out) { set_error("sdrx_bfm_create: null out"); return SDRX_EINVAL; }
    *out = nullptr;
    int rc = validate(n_ch, cfg); if (rc) return rc;
    for (int c = 0; rds && c < n_ch; c++)
        if (rds[c].rds_active != 0 && rds[c].rds_active != 1) return bad("rds_active", "0 or 1");
    sdrx_bfm* b = new (std::nothrow) sdrx_bfm;
    if (!b) return SDRX_ENOMEM;
    rc = b->core.open(device);
    if (rc) { delete b; return rc; }
    b->n_ch = n_ch;
    b->cfg.assign(cfg, cfg + n_ch);
    b->ch.resize((size_t)n_ch); b->h_chan.resize((size_t)n_ch);

    // NCO table (nco.cpp:30-39) and g_fft cosine table (gfft.h:141-150)
    rc = design_upload(&b->d_nco, design_nco_table(WFM_NCO_N));
    if (!rc) rc = design_upload(&b->d_utbl, design_gfft_table(WFM_FFT));
    if (rc) { sdrx_bfm_destroy(b); return rc; }
    SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&b->d_filters), (size_t)n_ch * WFM_FFT * 8), sdrx_bfm_destroy(b));
    b->filters_all.assign((size_t)n_ch * WFM_FFT * 2, 0.0f);
    for (int c = 0; c < n_ch; c++) {
        const sdrx_bfm_cfg& k = cfg[c];
        BfmHost& h = b->ch[(size_t)c];
        // m_interpolator.create(16, inputSampleRate, afBandwidth) and m_interpolatorStereo's twin: one table
        b->taps.add((double)k.in_rate, (double)k.af_bandwidth, 4.5);
        // Real lowCut = -(rfBandwidth / 2.0) / inputSampleRate, hiCut = +...; m_rfFilter->create_filter(lowCut, hiCut)
        const float f1 = (float)(-((double)k.rf_bandwidth / 2.0) / (double)k.in_rate);
        const float f2 = (float)(((double)k.rf_bandwidth / 2.0) / (double)k.in_rate);
        rc = design_fft_filter<WFM_FFT>(b->d_filters + (size_t)c * WFM_FFT, b->d_utbl, b->core.stream, &b->filters_all[(size_t)c * WFM_FFT * 2],
                                        [&](float* f, int h2) { fftfilt_fill_band(f1, f2, f, h2); });
        if (rc) { sdrx_bfm_destroy(b); return rc; }
        BfmChan& x = b->h_chan[(size_t)c];
        std::memset(&x, 0, sizeof x);
        WfmChan& s = x.w;
        s.nco_inc = (int)(((float)k.nco_freq * WFM_NCO_N) / (float)k.in_rate);          // NCO::setFreq (float math, truncation)
        s.step = (float)k.in_rate / (float)k.audio_rate;
        s.ntaps = b->taps.ntaps[(size_t)c]; s.taps_off = b->taps.off[(size_t)c];
        s.filt_off = c * WFM_FFT;
        const float excursion = 750000;                                                    // Real m_fmExcursion(default_excursion)
        s.fm_scaling = (float)k.in_rate / excursion;                                       // setFMScaling(inputSampleRate / m_fmExcursion)
        s.squelch_level = (float)std::pow(10.0, (double)k.squelch_db / 10.0);
        s.cap_f = k.rf_bandwidth / 10; s.open_f = k.rf_bandwidth / 20;
        s.cap = wfm_counter_cap(s.cap_f);
        s.volume = k.volume; s.mute = 0;
        design_dyadic_step(s.step, "SDRX_BFM_SERIAL_SCHEDULE", &s.dy_q, &s.dy_S);
        if (s.dy_q >= 0) b->any_dyadic = true;
        s.distance = s.step;                                                               // both ...DistanceRemain start at in / audio
        x.stereo = k.audio_stereo; x.lsb = k.lsb_stereo; x.show_pilot = k.show_pilot;
        if (x.stereo) b->any_stereo = true;
        bfm_pll_design(19000.0 / k.in_rate, 50.0 / k.in_rate, 0.01, &x.pk, &x.ps);
        bfm_rc_design((double)(50.0f * (float)k.audio_rate) * 1.0e-6, &x.rc_b0, &x.rc_a1);   // default_deemphasis * rate * 1.0e-6
        x.last_open = -1;
        if (s.ntaps > WFM_HIST) { set_error("sdrx_bfm_create: resampler window does not fit"); sdrx_bfm_destroy(b); return SDRX_EINVAL; }
        for (int i = 0; i < 2; i++) SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&h.pend[i]), WFM_H * 4), sdrx_bfm_destroy(b));
    }
    rc = design_upload(&b->d_taps, b->taps.all);
    if (rc) { sdrx_bfm_destroy(b); return rc; }
    SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&b->d_chan), (size_t)n_ch * sizeof(BfmChan)), sdrx_bfm_destroy(b));
    SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&b->d_bufs), (size_t)n_ch * sizeof(BfmBufs)), sdrx_bfm_destroy(b));
    SDRX_HIP_ELSE(hipHostMalloc(reinterpret_cast<void**>(&b->h_bufs), (size_t)n_ch * sizeof(BfmBufs), hipHostMallocDefault), sdrx_bfm_destroy(b));
    SDRX_HIP_ELSE(hipEventCreateWithFlags(&b->bufs_ev, hipEventDisableTiming), sdrx_bfm_destroy(b));
    SDRX_HIP_ELSE(hipEventRecord(b->bufs_ev, b->core.stream), sdrx_bfm_destroy(b));
    SDRX_HIP_ELSE(hipEventCreateWithFlags(&b->prod_ev, hipEventDisableTiming), sdrx_bfm_destroy(b));
    SDRX_HIP_ELSE(hipEventCreateWithFlags(&b->cons_ev, hipEventDisableTiming), sdrx_bfm_destroy(b));
    for (int c = 0; rds && c < n_ch; c++) if (rds[c].rds_active) b->any_rds = true;
    if (b->any_rds) {
        b->h_rds.resize((size_t)n_ch);
        for (int c = 0; c < n_ch; c++) {
            BfmRdsChan& r = b->h_rds[(size_t)c];
            std::memset(&r, 0, sizeof r);
            // m_interpolatorRDS.create(4, in_rate, 600.0): one table per rate (channels without RDS share in the bookkeeping only)
            b->rds_taps.add((double)cfg[c].in_rate, 600.0, 4.5, RDS_PHASES);
            r.active = rds[c].rds_active;
            r.ntaps = b->rds_taps.ntaps[(size_t)c]; r.taps_off = b->rds_taps.off[(size_t)c];
            r.step = (float)((double)(float)cfg[c].in_rate / 250000.0);          // (Real) in_rate / 250000.0
            r.distance = r.step;
            rds_demod_fresh(&r.d); rds_decoder_fresh(&r.k);
            if (r.ntaps > WFM_HIST) { set_error("sdrx_bfmrds_create: resampler window does not fit"); sdrx_bfm_destroy(b); return SDRX_EINVAL; }
            if (r.active && cfg[c].audio_stereo) b->any_rds_stereo = true;
        }
        rc = design_upload(&b->d_rds_taps, b->rds_taps.all);
        if (rc) { sdrx_bfm_destroy(b); return rc; }
        SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&b->d_rds), (size_t)n_ch * sizeof(BfmRdsChan)), sdrx_bfm_destroy(b));
        SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&b->d_rbufs), (size_t)n_ch * sizeof(BfmRdsBufs)), sdrx_bfm_destroy(b));
        SDRX_HIP_ELSE(hipHostMalloc(reinterpret_cast<void**>(&b->h_rbufs), (size_t)n_ch * sizeof(BfmRdsBufs), hipHostMallocDefault), sdrx_bfm_destroy(b));
    }
    rc = upload_fresh_state(b);
    if (rc) { sdrx_bfm_destroy(b); return rc; }
    *out = b;
    return SDRX_OK;
}

int sdrx_bfm_create(sdrx_bfm_t** out, int device, int32_t n_ch, const sdrx_bfm_cfg* cfg)
{
    return create_common(out, device, n_ch, cfg, nullptr);
}

int sdrx_bfmrds_create(sdrx_bfm_t** out, int device, int32_t n_ch, const sdrx_bfm_cfg* cfg, const sdrx_bfmrds_cfg* rds)
{
    return create_common(out, device, n_ch, cfg, rds);
}

int sdrx_bfm_reset(sdrx_bfm_t* b)
{
    if (!b) { set_error("sdrx_bfm_reset: null handle"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    SDRX_HIP(hipStreamSynchronize(b->core.stream));
    return upload_fresh_state(b);
}

// producer != nullptr: the input samples are being written on that stream; ordered as sdrx_wfm.hip's feed_common
static int feed_common(sdrx_bfm* b, const int16_t* const* d_iq, const int64_t* n_per_ch, hipStream_t producer = nullptr)
{
    int64_t max_blocks = 0, max_out = 0;
    int rc = demod_check_lengths(b->n_ch, n_per_ch, "sdrx_bfm_feed"); if (rc) return rc;
    rc = demod_check_dev_pointers(b->n_ch, d_iq, n_per_ch, "sdrx_bfm_feed"); if (rc) return rc;
    for (int c = 0; c < b->n_ch; c++) {
        BfmHost& h = b->ch[(size_t)c];
        rc = demod_grow_arena<BfmBufs>(h.arena, h.cap_in, std::max<int64_t>(n_per_ch[c], 1), b->core.stream, work); if (rc) return rc;
        const int64_t nb = (h.pending + n_per_ch[c]) / WFM_H;
        max_blocks = std::max(max_blocks, nb);
        // every audio sample after the first of a feed consumes >= floor(step) demodulated samples
        const int64_t per_out = std::max<int64_t>(1, (int64_t)std::floor(b->h_chan[(size_t)c].w.step));
        max_out = std::max(max_out, std::min<int64_t>(nb * WFM_H, nb * WFM_H / per_out + 4));
        if (b->any_rds && b->h_rds[(size_t)c].active) {
            rc = demod_grow_arena<BfmRdsBufs>(h.rds_arena, h.rds_cap, std::max<int64_t>(n_per_ch[c], 1), b->core.stream, rds_work); if (rc) return rc;
        }
    }
    SDRX_HIP(hipEventSynchronize(b->bufs_ev));            // previous feed's copy has read the table
    for (int c = 0; b->any_rds && c < b->n_ch; c++)
        b->h_rbufs[c] = demod_place<BfmRdsBufs>(b->ch[(size_t)c].rds_arena.p, b->ch[(size_t)c].rds_cap, rds_work);
    for (int c = 0; c < b->n_ch; c++) {
        BfmHost& h = b->ch[(size_t)c];
        BfmBufs& u = b->h_bufs[c];
        u = BfmBufs{};
        u.w.in = reinterpret_cast<const uint32_t*>(d_iq[c]);
        u.w.pend = h.pend[h.cur]; u.w.pend_next = h.pend[h.cur ^ 1];
        Carver k{static_cast<char*>(h.arena.p)};
        work(k, h.cap_in, u);
        u.w.n_in = n_per_ch[c];
    }
    rc = b->core.timer.begin(b->core.stream); if (rc) return rc;
    if (b->any_rds) SDRX_HIP(hipMemcpyAsync(b->d_rbufs, b->h_rbufs, (size_t)b->n_ch * sizeof(BfmRdsBufs), hipMemcpyHostToDevice, b->core.stream));
    rc = demod_upload_bufs(b->d_bufs, b->h_bufs, b->n_ch, b->bufs_ev, b->core.stream); if (rc) return rc;
    const unsigned nc = (unsigned)b->n_ch, gc = (nc + 63) / 64, nblk = (unsigned)max_blocks;
    const unsigned gw = (nc + BFM_WALK_WAVES - 1) / BFM_WALK_WAVES, go = (unsigned)((max_out + 255) / 256);
    hipStream_t st = b->core.stream;
    hipLaunchKernelGGL(bfm_prep_kernel, dim3(gc), dim3(64), 0, st, b->d_chan, b->d_bufs, b->n_ch);
    SDRX_HIP(hipGetLastError());
    if (nblk && b->any_dyadic) {
        hipLaunchKernelGGL(bfm_sched_fill_kernel, dim3(go, nc), dim3(256), 0, st, b->d_chan, b->d_bufs);
        SDRX_HIP(hipGetLastError());
    }
    // lanes whose channel the closed form took exit at once (prep's off-grid guard can hand a channel back)
    hipLaunchKernelGGL(bfm_sched_walk_kernel, dim3(gc), dim3(64), 0, st, b->d_chan, b->d_bufs, b->n_ch);
    SDRX_HIP(hipGetLastError());
    if (b->any_rds) {
        hipLaunchKernelGGL(bfm_rds_sched_kernel, dim3(gc), dim3(64), 0, st, b->d_chan, b->d_rds, b->d_rbufs, b->n_ch);
        SDRX_HIP(hipGetLastError());
    }
    rc = demod_stream_after(st, producer, b->prod_ev); if (rc) return rc;
    if (nblk) {
        hipLaunchKernelGGL(bfm_fft_kernel, dim3(nblk, nc), dim3(WFM_FFT / 8), 0, st, b->d_chan, b->d_bufs, b->d_filters, b->d_utbl, b->d_nco);
        SDRX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(bfm_pend_kernel, dim3(nc), dim3(WFM_H), 0, st, b->d_chan, b->d_bufs);
    SDRX_HIP(hipGetLastError());
    rc = demod_stream_after(producer, st, b->cons_ev); if (rc) return rc;
    if (nblk) {
        hipLaunchKernelGGL(bfm_level_kernel, dim3(nblk, nc), dim3(256), 0, st, b->d_chan, b->d_bufs);
        SDRX_HIP(hipGetLastError());
        hipLaunchKernelGGL(bfm_blockscan_kernel, dim3(nc), dim3(64), 0, st, b->d_chan, b->d_bufs);
        SDRX_HIP(hipGetLastError());
        hipLaunchKernelGGL(bfm_open_kernel, dim3(nblk, nc), dim3(256), 0, st, b->d_chan, b->d_bufs);
        SDRX_HIP(hipGetLastError());
        hipLaunchKernelGGL(bfm_lastopen_kernel, dim3(nc), dim3(64), 0, st, b->d_chan, b->d_bufs);
        SDRX_HIP(hipGetLastError());
        hipLaunchKernelGGL(bfm_discri_kernel, dim3(nblk, nc), dim3(256), 0, st, b->d_chan, b->d_bufs);
        SDRX_HIP(hipGetLastError());
        if (b->any_stereo) {
            if (b->any_rds_stereo) hipLaunchKernelGGL(bfm_walk_rds_kernel, dim3(gw), dim3(64 * BFM_WALK_WAVES), 0, st, b->d_chan, b->d_bufs, b->n_ch, b->d_rds, b->d_rbufs);
            else hipLaunchKernelGGL(bfm_walk_kernel, dim3(gw), dim3(64 * BFM_WALK_WAVES), 0, st, b->d_chan, b->d_bufs, b->n_ch);
            SDRX_HIP(hipGetLastError());
            b->core.note_launch(b->any_rds_stereo ? "bfm_walk_rds_kernel" : "bfm_walk_kernel", (int)gw, 64 * BFM_WALK_WAVES, 0);
            hipLaunchKernelGGL(bfm_post_kernel, dim3(2 * nblk, nc), dim3(256), 0, st, b->d_chan, b->d_bufs);
            SDRX_HIP(hipGetLastError());
        } else {
            b->core.note_launch("bfm_fft_kernel", (int)(nblk * nc), WFM_FFT / 8, (int)(2 * WFM_FFT * sizeof(float2) + (WFM_FFT / 4 + 1) * sizeof(float)));
        }
        hipLaunchKernelGGL(bfm_fir_kernel, dim3(go, nc), dim3(256), 0, st, b->d_chan, b->d_bufs, b->d_taps);
        SDRX_HIP(hipGetLastError());
        hipLaunchKernelGGL(bfm_deemph_kernel, dim3(gw), dim3(64 * BFM_WALK_WAVES), 0, st, b->d_chan, b->d_bufs, b->n_ch);
        SDRX_HIP(hipGetLastError());
    }
    if (b->any_rds) {
        // behind the pilot walk (the mixer's phases) and in front of the carry kernel (n_dem, the windows)
        if (nblk) {
            hipLaunchKernelGGL(bfm_rds_mix_kernel, dim3(2 * nblk, nc), dim3(256), 0, st, b->d_chan, b->d_rds, b->d_bufs, b->d_rbufs);
            SDRX_HIP(hipGetLastError());
            hipLaunchKernelGGL(bfm_rds_fir_kernel, dim3(2 * nblk, nc), dim3(256), 0, st, b->d_rds, b->d_rbufs, b->d_rds_taps);
            SDRX_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(bfm_rds_walk_kernel, dim3(gw), dim3(64 * BFM_WALK_WAVES), 0, st, b->d_rds, b->d_rbufs, b->n_ch);
        SDRX_HIP(hipGetLastError());
        hipLaunchKernelGGL(bfm_rds_carry_kernel, dim3(nc), dim3(WFM_HIST), 0, st, b->d_chan, b->d_rds, b->d_rbufs);
        SDRX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(bfm_carry_kernel, dim3(nc), dim3(WFM_H), 0, st, b->d_chan, b->d_bufs);
    SDRX_HIP(hipGetLastError());
    rc = b->core.timer.end(st); if (rc) return rc;
    for (int c = 0; c < b->n_ch; c++) {
        BfmHost& h = b->ch[(size_t)c];
        h.cur ^= 1;
        h.pending = (int)((h.pending + n_per_ch[c]) % WFM_H);
    }
    return SDRX_OK;
}

int sdrx_bfm_feed_dev(sdrx_bfm_t* b, const int16_t* const* d_iq, const int64_t* n_per_ch)
{
    if (!b || !d_iq || !n_per_ch) { set_error("sdrx_bfm_feed_dev: null argument"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    return feed_common(b, d_iq, n_per_ch);
}

int sdrx_bfm_feed_bank(sdrx_bfm_t* b, sdrx_chan_bank_t* bank)
{
    if (!b || !bank) { set_error("sdrx_bfm_feed_bank: null argument"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    void* ps = nullptr;
    int rc = sdrx_chan_bank_get_stream(bank, &ps); if (rc) return rc;
    std::vector<const int16_t*> d;
    std::vector<int64_t> n;
    rc = demod_gather_bank(bank, b->n_ch, "sdrx_bfm_feed_bank", d, n); if (rc) return rc;
    return feed_common(b, d.data(), n.data(), static_cast<hipStream_t>(ps));
}

int sdrx_bfm_feed(sdrx_bfm_t* b, const int16_t* const* iq, const int64_t* n_per_ch)
{
    if (!b || !iq || !n_per_ch) { set_error("sdrx_bfm_feed: null argument"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    std::vector<const int16_t*> d;
    int rc = demod_stage_inputs(b->ch, b->core.stream, iq, n_per_ch, "sdrx_bfm_feed", d); if (rc) return rc;
    rc = feed_common(b, d.data(), n_per_ch); if (rc) return rc;
    SDRX_HIP(hipStreamSynchronize(b->core.stream));            // the caller's buffers are free again on return
    return SDRX_OK;
}

static BfmBufs place(sdrx_bfm* b, int32_t c) { return demod_place<BfmBufs>(b->ch[(size_t)c].arena.p, b->ch[(size_t)c].cap_in, work); }

int64_t sdrx_bfm_read(sdrx_bfm_t* b, int32_t c, int16_t* audio_lr, int64_t cap)
{
    if (!b || c < 0 || c >= b->n_ch || cap < 0 || (cap > 0 && !audio_lr)) { set_error("sdrx_bfm_read: bad argument"); return SDRX_EINVAL; }
    BfmChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    const int64_t n = std::min<int64_t>(s.w.n_out, cap);
    if (n == 0) return 0;
    SDRX_HIP(hipMemcpy(audio_lr, place(b, c).pairs, (size_t)n * 4, hipMemcpyDeviceToHost));
    return n;
}

int sdrx_bfm_last_dev(sdrx_bfm_t* b, int32_t c, const int16_t** d_audio_lr, int64_t* n)
{
    if (!b || c < 0 || c >= b->n_ch || !d_audio_lr || !n) { set_error("sdrx_bfm_last_dev: bad argument"); return SDRX_EINVAL; }
    BfmChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    *d_audio_lr = reinterpret_cast<const int16_t*>(place(b, c).pairs);
    *n = s.w.n_out;
    return SDRX_OK;
}

int64_t sdrx_bfm_read_sink(sdrx_bfm_t* b, int32_t c, int16_t* samples_iq, int64_t cap_samples)
{
    if (!b || c < 0 || c >= b->n_ch || cap_samples < 0 || (cap_samples > 0 && !samples_iq)) { set_error("sdrx_bfm_read_sink: bad argument"); return SDRX_EINVAL; }
    BfmChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    const int64_t n = std::min<int64_t>(s.n_sink, cap_samples);
    if (n == 0) return 0;
    SDRX_HIP(hipMemcpy(samples_iq, place(b, c).sink, (size_t)n * 4, hipMemcpyDeviceToHost));
    return n;
}

int sdrx_bfm_sink_last_dev(sdrx_bfm_t* b, int32_t c, const int16_t** d_samples_iq, int64_t* n_samples)
{
    if (!b || c < 0 || c >= b->n_ch || !d_samples_iq || !n_samples) { set_error("sdrx_bfm_sink_last_dev: bad argument"); return SDRX_EINVAL; }
    BfmChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    *d_samples_iq = reinterpret_cast<const int16_t*>(place(b, c).sink);
    *n_samples = s.n_sink;
    return SDRX_OK;
}

int sdrx_bfm_pilot(sdrx_bfm_t* b, int32_t c, int32_t* locked, float* level, uint32_t* freq_bits, uint32_t* phase_bits)
{
    if (!b || c < 0 || c >= b->n_ch) { set_error("sdrx_bfm_pilot: bad argument"); return SDRX_EINVAL; }
    BfmChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    if (locked) *locked = bfm_pll_locked(s.pk, s.ps) ? 1 : 0;
    if (level) *level = 2 * s.ps.level;                       // get_pilot_level()
    if (freq_bits) std::memcpy(freq_bits, &s.ps.freq, 4);
    if (phase_bits) std::memcpy(phase_bits, &s.ps.phase, 4);
    return SDRX_OK;
}

int sdrx_bfm_squelch_open(sdrx_bfm_t* b, int32_t c)
{
    if (!b || c < 0 || c >= b->n_ch) { set_error("sdrx_bfm_squelch_open: bad argument"); return SDRX_EINVAL; }
    BfmChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    return s.w.sq_open;
}

int sdrx_bfm_levels(sdrx_bfm_t* b, int32_t c, double* sum, double* peak, int64_t* count, int reset)
{
    if (!b || c < 0 || c >= b->n_ch) { set_error("sdrx_bfm_levels: bad argument"); return SDRX_EINVAL; }
    BfmChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    if (sum) *sum = s.w.magsq_sum;
    if (peak) *peak = s.w.magsq_peak;
    if (count) *count = s.w.magsq_count;
    if (!reset) return SDRX_OK;                           // getMagSqLevels: sum, peak and count back to 0
    const size_t at = offsetof(BfmChan, w);
    return demod_zero_levels(b->core, b->d_chan + c, at + offsetof(WfmChan, magsq_sum), at + offsetof(WfmChan, magsq_peak), at + offsetof(WfmChan, magsq_count));
}

int sdrx_bfm_get_design(sdrx_bfm_t* b, int32_t c, int32_t* ntaps_per_phase, float* taps, int32_t taps_cap,
                        float* filter_iq, int32_t* nco_inc, float* squelch_level, float* pll7, int32_t* lock_delay, float* rc2)
{
    if (!b || c < 0 || c >= b->n_ch) { set_error("sdrx_bfm_get_design: bad channel"); return SDRX_EINVAL; }
    const int nt = b->taps.ntaps[(size_t)c];
    const BfmChan& s = b->h_chan[(size_t)c];
    if (ntaps_per_phase) *ntaps_per_phase = nt;
    if (taps && taps_cap > 0) std::memcpy(taps, &b->taps.all[(size_t)b->taps.off[(size_t)c]], (size_t)std::min(taps_cap, nt * 16) * 4);
    if (filter_iq) std::memcpy(filter_iq, &b->filters_all[(size_t)c * WFM_FFT * 2], WFM_FFT * 8);
    if (nco_inc) *nco_inc = s.w.nco_inc;
    if (squelch_level) *squelch_level = s.w.squelch_level;
    if (pll7) { const float v[7] = { s.pk.minfreq, s.pk.maxfreq, s.pk.b0, s.pk.a1, s.pk.a2, s.pk.lf_b0, s.pk.lf_b1 }; std::memcpy(pll7, v, sizeof v); }
    if (lock_delay) *lock_delay = s.pk.lock_delay;
    if (rc2) { rc2[0] = s.rc_b0; rc2[1] = s.rc_a1; }
    return SDRX_OK;
}

// ---- RDS
static int rds_fetch(sdrx_bfm* b, int32_t c, const char* who, BfmRdsChan* r)
{
    if (!b || c < 0 || c >= b->n_ch) { set_error(std::string(who) + ": bad argument"); return SDRX_EINVAL; }
    if (!b->any_rds || !b->h_rds[(size_t)c].active) { set_error(std::string(who) + ": the channel was created without RDS"); return SDRX_EINVAL; }
    return demod_fetch_state(b->core, b->d_rds, c, r);
}

static BfmRdsBufs rds_place(sdrx_bfm* b, int32_t c) { return demod_place<BfmRdsBufs>(b->ch[(size_t)c].rds_arena.p, b->ch[(size_t)c].rds_cap, rds_work); }

int64_t sdrx_bfmrds_read_bits(sdrx_bfm_t* b, int32_t c, uint8_t* bits, int64_t cap)
{
    BfmRdsChan r;
    if (cap < 0 || (cap > 0 && !bits)) { set_error("sdrx_bfmrds_read_bits: bad argument"); return SDRX_EINVAL; }
    int rc = rds_fetch(b, c, "sdrx_bfmrds_read_bits", &r); if (rc) return rc;
    const int64_t n = std::min<int64_t>(r.n_bits, cap);
    if (n == 0) return 0;
    SDRX_HIP(hipMemcpy(bits, rds_place(b, c).bits, (size_t)n, hipMemcpyDeviceToHost));
    return n;
}

int sdrx_bfmrds_bits_last_dev(sdrx_bfm_t* b, int32_t c, const uint8_t** d_bits, int64_t* n)
{
    BfmRdsChan r;
    if (!d_bits || !n) { set_error("sdrx_bfmrds_bits_last_dev: bad argument"); return SDRX_EINVAL; }
    int rc = rds_fetch(b, c, "sdrx_bfmrds_bits_last_dev", &r); if (rc) return rc;
    *d_bits = rds_place(b, c).bits; *n = r.n_bits;
    return SDRX_OK;
}

int64_t sdrx_bfmrds_read_groups(sdrx_bfm_t* b, int32_t c, uint16_t* blocks4, int64_t cap_groups)
{
    BfmRdsChan r;
    if (cap_groups < 0 || (cap_groups > 0 && !blocks4)) { set_error("sdrx_bfmrds_read_groups: bad argument"); return SDRX_EINVAL; }
    int rc = rds_fetch(b, c, "sdrx_bfmrds_read_groups", &r); if (rc) return rc;
    const int64_t n = std::min<int64_t>(r.n_groups, cap_groups);
    if (n == 0) return 0;
    SDRX_HIP(hipMemcpy(blocks4, rds_place(b, c).groups, (size_t)n * 8, hipMemcpyDeviceToHost));
    return n;
}

int sdrx_bfmrds_groups_last_dev(sdrx_bfm_t* b, int32_t c, const uint16_t** d_blocks4, int64_t* n_groups)
{
    BfmRdsChan r;
    if (!d_blocks4 || !n_groups) { set_error("sdrx_bfmrds_groups_last_dev: bad argument"); return SDRX_EINVAL; }
    int rc = rds_fetch(b, c, "sdrx_bfmrds_groups_last_dev", &r); if (rc) return rc;
    *d_blocks4 = rds_place(b, c).groups; *n_groups = r.n_groups;
    return SDRX_OK;
}

int64_t sdrx_bfmrds_read_bb(sdrx_bfm_t* b, int32_t c, float* subcarr_bb, int64_t cap)
{
    BfmRdsChan r;
    if (cap < 0 || (cap > 0 && !subcarr_bb)) { set_error("sdrx_bfmrds_read_bb: bad argument"); return SDRX_EINVAL; }
    int rc = rds_fetch(b, c, "sdrx_bfmrds_read_bb", &r); if (rc) return rc;
    const int64_t n = std::min<int64_t>(r.n_rds, cap);
    if (n == 0) return 0;
    SDRX_HIP(hipMemcpy(subcarr_bb, rds_place(b, c).bb, (size_t)n * 4, hipMemcpyDeviceToHost));
    return n;
}

int sdrx_bfmrds_report(sdrx_bfm_t* b, int32_t c, float* acc, float* qua, float* fclk, float* decoder_qua, int32_t* synced)
{
    BfmRdsChan r;
    int rc = rds_fetch(b, c, "sdrx_bfmrds_report", &r); if (rc) return rc;
    if (acc) *acc = r.d.rep_acc;
    if (qua) *qua = r.d.rep_qua;
    if (fclk) *fclk = r.d.rep_fclk;
    if (decoder_qua) *decoder_qua = r.k.qua;
    if (synced) *synced = r.k.sync;
    return SDRX_OK;
}

int sdrx_bfmrds_state(sdrx_bfm_t* b, int32_t c, sdrx_bfmrds_state_t* o)
{
    BfmRdsChan r;
    if (!o) { set_error("sdrx_bfmrds_state: bad argument"); return SDRX_EINVAL; }
    int rc = rds_fetch(b, c, "sdrx_bfmrds_state", &r); if (rc) return rc;
    auto fb = [](float v) { uint32_t i; std::memcpy(&i, &v, 4); return i; };
    auto db = [](double v) { uint64_t i; std::memcpy(&i, &v, 8); return i; };
    std::memset(o, 0, sizeof *o);
    o->subcarr_phi = db(r.d.subcarr_phi); o->clock_offset = db(r.d.clock_offset); o->clock_phi = db(r.d.clock_phi);
    o->prev_clock_phi = db(r.d.prev_clock_phi); o->d_cphi = db(r.d.d_cphi);
    for (int i = 0; i < 3; i++) { o->xv[i] = fb(r.d.xv[i]); o->yv[i] = fb(r.d.yv[i]); }
    o->prev_bb = fb(r.d.prev_bb); o->acc = fb(r.d.acc); o->prev_acc = fb(r.d.prev_acc);
    o->lo_clock = fb(r.d.lo_clock); o->prev_lo_clock = fb(r.d.prev_lo_clock);
    o->numsamples = r.d.numsamples; o->counter = r.d.counter; o->reading_frame = r.d.reading_frame;
    o->tot_errs[0] = r.d.tot_errs0; o->tot_errs[1] = r.d.tot_errs1; o->dbit = r.d.dbit;
    o->distance_remain = fb(r.distance); o->mix_phase = fb(r.mix_phase);
    o->n_rds = r.n_rds;
    o->reg = r.k.reg; o->lastseen_offset_counter = r.k.lastseenOffsetCounter; o->bit_counter = r.k.bitCounter;
    o->block_bit_counter = r.k.blockBitCounter; o->wrong_blocks_counter = r.k.wrongBlocksCounter; o->blocks_counter = r.k.blocksCounter;
    o->group_good_blocks_counter = r.k.groupGoodBlocksCounter;
    o->group[0] = r.k.group0; o->group[1] = r.k.group1; o->group[2] = r.k.group2; o->group[3] = r.k.group3;
    o->sync = r.k.sync; o->presync = r.k.presync; o->lastseen_offset = r.k.lastseenOffset; o->block_number = r.k.blockNumber;
    o->group_assembly_started = r.k.groupAssemblyStarted; o->good_block = r.k.goodBlock; o->decoder_qua = fb(r.k.qua);
    return SDRX_OK;
}

int64_t sdrx_bfmrds_unsure(sdrx_bfm_t* b, int32_t c, int reset)
{
    BfmRdsChan r;
    int rc = rds_fetch(b, c, "sdrx_bfmrds_unsure", &r); if (rc) return rc;
    if (reset) {
        SDRX_HIP(hipMemsetAsync(reinterpret_cast<char*>(b->d_rds + c) + offsetof(BfmRdsChan, unsure), 0, sizeof(unsigned long long), b->core.stream));
        SDRX_HIP(hipStreamSynchronize(b->core.stream));
    }
    return (int64_t)r.unsure;
}

int sdrx_bfm_sync(sdrx_bfm_t* b) { return b ? b->core.sync() : SDRX_EINVAL; }

int sdrx_bfm_set_stream(sdrx_bfm_t* b, void* hip_stream) { return b ? b->core.set_stream(hip_stream) : SDRX_EINVAL; }

int sdrx_bfm_get_stream(sdrx_bfm_t* b, void** hip_stream) { return b ? b->core.get_stream(hip_stream) : SDRX_EINVAL; }

int sdrx_bfm_set_timing(sdrx_bfm_t* b, int enabled) { return b ? b->core.set_timing(enabled) : SDRX_EINVAL; }

int sdrx_bfm_get_timing(sdrx_bfm_t* b, double* total_ms, int64_t* feeds, int reset) { return b ? b->core.get_timing(total_ms, feeds, reset) : SDRX_EINVAL; }

int sdrx_bfm_last_launch(const sdrx_bfm_t* b, char* kernel_name, int name_cap, int* grid, int* block, int* lds_bytes) { return b ? b->core.last_launch(kernel_name, name_cap, grid, block, lds_bytes) : SDRX_EINVAL; }

} // extern "C"
