// libsdrx.so: sdrx_wfm_* -- N wideband-FM demodulators (WFMDemod::feed, plugins/channelrx/demodwfm/wfmdemod.cpp:90-183) on
// one device: int16 I/Q at the channelizer's output rate in, mono qint16 audio out.  Kernels: wfm_kernels.hpp.
// Host side: the design products exactly as applyChannelSettings / applySettings derive them (wfmdemod.cpp:277-345),
// launches, buffer bookkeeping.
#include "sdrx_common.hpp"
#include "wfm_kernels.hpp"
#include "backend_design.hpp"
#include "demod_common.hpp"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

using namespace sdrx;

namespace {

struct WfmHost {
    DevBuf arena;                 // work()'s layout for cap_in samples
    DevBuf stage_in;              // host-pointer feeds
    uint32_t* pend[2] = { nullptr, nullptr };
    int cur = 0;
    int64_t cap_in = 0;
    int pending = 0;              // host mirror of WfmChan::pending (a function of the feed lengths only)
};

// One channel's work arena for feeds of up to cap_in samples.  tail's slot 0 (ovlbuf) and the front of dem (the resampler's
// window) carry state from feed to feed.
void work(Carver& k, int64_t cap_in, WfmBufs& u)
{
    const size_t n_blk = (size_t)(cap_in + WFM_H) / WFM_H + 1;       // pending (< 512) + new
    const size_t n_s = n_blk * WFM_H;
    u.head = k.take<float2>(n_s);
    u.tail = k.take_kept<float2>(n_s + WFM_H, WFM_H);
    u.arg = k.take<float>(n_s);
    u.flag = k.take<uint8_t>(n_s);
    u.blk_sum = k.take<double>(n_blk);
    u.blk_map = k.take<WfmClamp>(n_blk);
    u.blk_peak = k.take<float>(n_blk);
    u.blk_state = k.take<int>(n_blk);
    u.blk_first = k.take<int>(n_blk);
    u.blk_last = k.take<int>(n_blk + 64 / sizeof(int));
    u.dem = k.take_kept<float>(WFM_HIST + n_s + WFM_HIST, WFM_HIST);
    // every audio sample consumes at least one demodulated sample (step >= 1)
    u.sched = k.take<uint2>(n_s + 8);
    u.audio = k.take<int16_t>(n_s + 8);
}

} // namespace

struct sdrx_wfm {
    HandleCore core;
    int n_ch = 0;
    std::vector<sdrx_wfm_cfg> cfg;
    std::vector<WfmHost> ch;
    std::vector<WfmChan> h_chan;  // configuration and the state of a fresh handle
    WfmChan* d_chan = nullptr;
    WfmBufs* d_bufs = nullptr;
    WfmBufs* h_bufs = nullptr;    // pinned: the per-feed table goes to the device in one async copy
    hipEvent_t bufs_ev = nullptr;
    hipEvent_t prod_ev = nullptr, cons_ev = nullptr;       // device-side ordering against a producer stream (sdrx_wfm_feed_bank)
    float* d_nco = nullptr; float* d_taps = nullptr; float2* d_filters = nullptr; float* d_utbl = nullptr;
    InterpTables taps;
    std::vector<float> filters_all;
    bool any_dyadic = false, any_serial = false;
};

static int validate(int32_t n_ch, const sdrx_wfm_cfg* cfg)
{
    if (n_ch <= 0 || !cfg) { set_error("sdrx_wfm_create: bad argument"); return SDRX_EINVAL; }
    for (int c = 0; c < n_ch; c++) {
        const sdrx_wfm_cfg& k = cfg[c];
        if (k.in_rate <= 0 || k.audio_rate <= 0 || k.audio_rate > k.in_rate) {
            set_error("sdrx_wfm_create: bad channel configuration (need 0 < audio_rate <= in_rate)"); return SDRX_EINVAL;
        }
        if (!(k.rf_bandwidth > 0.0f) || !(k.rf_bandwidth <= 1.0e7f) || !(k.af_bandwidth > 0.0f) || !std::isfinite(k.af_bandwidth)) {
            set_error("sdrx_wfm_create: bad channel configuration (need 0 < rf_bandwidth <= 1e7 and af_bandwidth > 0)"); return SDRX_EINVAL;
        }
        if (!std::isfinite(k.volume) || !std::isfinite(k.squelch_db)) {
            set_error("sdrx_wfm_create: bad channel configuration (volume and squelch_db must be finite)"); return SDRX_EINVAL;
        }
    }
    return SDRX_OK;
}

static int upload_fresh_state(sdrx_wfm* b)
{
    SDRX_HIP(hipMemcpyAsync(b->d_chan, b->h_chan.data(), (size_t)b->n_ch * sizeof(WfmChan), hipMemcpyHostToDevice, b->core.stream));
    for (auto& h : b->ch) {
        for (int i = 0; i < 2; i++) SDRX_HIP(hipMemsetAsync(h.pend[i], 0, WFM_H * 4, b->core.stream));
        int rc = demod_clear_kept<WfmBufs>(h.arena, h.cap_in, b->core.stream, work); if (rc) return rc;
        h.pending = 0;
    }
    SDRX_HIP(hipStreamSynchronize(b->core.stream));
    return SDRX_OK;
}

extern "C" {

int sdrx_wfm_destroy(sdrx_wfm_t* b)
{
    if (!b) return SDRX_OK;
    (void)hipSetDevice(b->core.device);
    if (b->core.stream) (void)hipStreamSynchronize(b->core.stream);
    for (auto& h : b->ch) {
        h.arena.release(); h.stage_in.release();
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
    b->core.close();
    delete b;
    return SDRX_OK;
}

int sdrx_wfm_create(sdrx_wfm_t** out, int device, int32_t n_ch, const sdrx_wfm_cfg* cfg)
{
    if (!out) { set_error("sdrx_wfm_create: null out"); return SDRX_EINVAL; }
    *out = nullptr;
    int rc = validate(n_ch, cfg); if (rc) return rc;
    sdrx_wfm* b = new (std::nothrow) sdrx_wfm;
    if (!b) return SDRX_ENOMEM;
    rc = b->core.open(device);
    if (rc) { delete b; return rc; }
    b->n_ch = n_ch;
    b->cfg.assign(cfg, cfg + n_ch);
    b->ch.resize((size_t)n_ch); b->h_chan.resize((size_t)n_ch);

    // NCO table (nco.cpp:30-39) and g_fft cosine table (gfft.h:141-150)
    rc = design_upload(&b->d_nco, design_nco_table(WFM_NCO_N));
    if (!rc) rc = design_upload(&b->d_utbl, design_gfft_table(WFM_FFT));
    if (rc) { sdrx_wfm_destroy(b); return rc; }
    SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&b->d_filters), (size_t)n_ch * WFM_FFT * 8), sdrx_wfm_destroy(b));
    b->filters_all.assign((size_t)n_ch * WFM_FFT * 2, 0.0f);
    for (int c = 0; c < n_ch; c++) {
        const sdrx_wfm_cfg& k = cfg[c];
        WfmHost& h = b->ch[(size_t)c];
        // m_interpolator.create(16, inputSampleRate, afBandwidth)
        b->taps.add((double)k.in_rate, (double)k.af_bandwidth, 4.5);
        // Real lowCut = -(rfBandwidth / 2.0) / inputSampleRate, hiCut = +...; m_rfFilter->create_filter(lowCut, hiCut)
        const float f1 = (float)(-((double)k.rf_bandwidth / 2.0) / (double)k.in_rate);
        const float f2 = (float)(((double)k.rf_bandwidth / 2.0) / (double)k.in_rate);
        rc = design_fft_filter<WFM_FFT>(b->d_filters + (size_t)c * WFM_FFT, b->d_utbl, b->core.stream, &b->filters_all[(size_t)c * WFM_FFT * 2],
                                        [&](float* f, int h2) { fftfilt_fill_band(f1, f2, f, h2); });
        if (rc) { sdrx_wfm_destroy(b); return rc; }
        WfmChan& s = b->h_chan[(size_t)c];
        std::memset(&s, 0, sizeof s);
        s.nco_inc = (int)(((float)k.nco_freq * WFM_NCO_N) / (float)k.in_rate);          // NCO::setFreq (float math, truncation)
        s.step = (float)k.in_rate / (float)k.audio_rate;
        s.ntaps = b->taps.ntaps[(size_t)c]; s.taps_off = b->taps.off[(size_t)c];
        s.filt_off = c * WFM_FFT;
        const float excursion = k.rf_bandwidth / (float)k.in_rate;                        // m_fmExcursion
        s.fm_scaling = 1.0f / excursion;
        s.squelch_level = (float)std::pow(10.0, (double)k.squelch_db / 10.0);
        s.cap_f = k.rf_bandwidth / 10; s.open_f = k.rf_bandwidth / 20;
        s.cap = wfm_counter_cap(s.cap_f);
        s.volume = k.volume; s.mute = k.audio_mute ? 1 : 0;
        design_dyadic_step(s.step, "SDRX_WFM_SERIAL_SCHEDULE", &s.dy_q, &s.dy_S);
        (s.dy_q >= 0 ? b->any_dyadic : b->any_serial) = true;
        s.distance = s.step;                                                               // m_interpolatorDistanceRemain starts at in / audio
        if (s.ntaps > WFM_HIST) { set_error("sdrx_wfm_create: resampler window does not fit"); sdrx_wfm_destroy(b); return SDRX_EINVAL; }
        for (int i = 0; i < 2; i++) SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&h.pend[i]), WFM_H * 4), sdrx_wfm_destroy(b));
    }
    rc = design_upload(&b->d_taps, b->taps.all);
    if (rc) { sdrx_wfm_destroy(b); return rc; }
    SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&b->d_chan), (size_t)n_ch * sizeof(WfmChan)), sdrx_wfm_destroy(b));
    SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&b->d_bufs), (size_t)n_ch * sizeof(WfmBufs)), sdrx_wfm_destroy(b));
    SDRX_HIP_ELSE(hipHostMalloc(reinterpret_cast<void**>(&b->h_bufs), (size_t)n_ch * sizeof(WfmBufs), hipHostMallocDefault), sdrx_wfm_destroy(b));
    SDRX_HIP_ELSE(hipEventCreateWithFlags(&b->bufs_ev, hipEventDisableTiming), sdrx_wfm_destroy(b));
    SDRX_HIP_ELSE(hipEventRecord(b->bufs_ev, b->core.stream), sdrx_wfm_destroy(b));
    SDRX_HIP_ELSE(hipEventCreateWithFlags(&b->prod_ev, hipEventDisableTiming), sdrx_wfm_destroy(b));
    SDRX_HIP_ELSE(hipEventCreateWithFlags(&b->cons_ev, hipEventDisableTiming), sdrx_wfm_destroy(b));
    rc = upload_fresh_state(b);
    if (rc) { sdrx_wfm_destroy(b); return rc; }
    *out = b;
    return SDRX_OK;
}

int sdrx_wfm_reset(sdrx_wfm_t* b)
{
    if (!b) { set_error("sdrx_wfm_reset: null handle"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    SDRX_HIP(hipStreamSynchronize(b->core.stream));
    return upload_fresh_state(b);
}

// producer != nullptr: the input samples are being written on that stream.  The schedule kernels (they need the counts
// only) are launched first and overlap the producer; the readers of `in` (wfm_fft: NCO mix on load, wfm_pend: the raw
// remainder) wait for the producer on the device, and the producer's stream waits until they are done before it may run
// anything queued after this call.
static int feed_common(sdrx_wfm* b, const int16_t* const* d_iq, const int64_t* n_per_ch, hipStream_t producer = nullptr)
{
    int64_t max_blocks = 0, max_out = 0;
    int rc = demod_check_lengths(b->n_ch, n_per_ch, "sdrx_wfm_feed"); if (rc) return rc;
    rc = demod_check_dev_pointers(b->n_ch, d_iq, n_per_ch, "sdrx_wfm_feed"); if (rc) return rc;
    for (int c = 0; c < b->n_ch; c++) {
        WfmHost& h = b->ch[(size_t)c];
        rc = demod_grow_arena<WfmBufs>(h.arena, h.cap_in, std::max<int64_t>(n_per_ch[c], 1), b->core.stream, work); if (rc) return rc;
        const int64_t nb = (h.pending + n_per_ch[c]) / WFM_H;
        max_blocks = std::max(max_blocks, nb);
        // every audio sample after the first of a feed consumes >= floor(step) demodulated samples
        const int64_t per_out = std::max<int64_t>(1, (int64_t)std::floor(b->h_chan[(size_t)c].step));
        max_out = std::max(max_out, std::min<int64_t>(nb * WFM_H, nb * WFM_H / per_out + 4));
    }
    SDRX_HIP(hipEventSynchronize(b->bufs_ev));            // previous feed's copy has read the table
    for (int c = 0; c < b->n_ch; c++) {
        WfmHost& h = b->ch[(size_t)c];
        WfmBufs& u = b->h_bufs[c];
        u.in = reinterpret_cast<const uint32_t*>(d_iq[c]);
        u.pend = h.pend[h.cur]; u.pend_next = h.pend[h.cur ^ 1];
        Carver k{static_cast<char*>(h.arena.p)};
        work(k, h.cap_in, u);
        u.n_in = n_per_ch[c];
    }
    rc = b->core.timer.begin(b->core.stream); if (rc) return rc;
    rc = demod_upload_bufs(b->d_bufs, b->h_bufs, b->n_ch, b->bufs_ev, b->core.stream); if (rc) return rc;
    const unsigned nc = (unsigned)b->n_ch, gc = (nc + 63) / 64, nblk = (unsigned)max_blocks;
    hipLaunchKernelGGL(wfm_prep_kernel, dim3(gc), dim3(64), 0, b->core.stream, b->d_chan, b->d_bufs, b->n_ch);
    SDRX_HIP(hipGetLastError());
    if (nblk && b->any_dyadic) {
        hipLaunchKernelGGL(wfm_sched_fill_kernel, dim3((unsigned)((max_out + 255) / 256), nc), dim3(256), 0, b->core.stream, b->d_chan, b->d_bufs);
        SDRX_HIP(hipGetLastError());
    }
    // lanes whose channel the closed form took exit at once (prep's off-grid guard can hand a channel back)
    hipLaunchKernelGGL(wfm_sched_walk_kernel, dim3(gc), dim3(64), 0, b->core.stream, b->d_chan, b->d_bufs, b->n_ch);
    SDRX_HIP(hipGetLastError());
    rc = demod_stream_after(b->core.stream, producer, b->prod_ev); if (rc) return rc;
    if (nblk) {
        hipLaunchKernelGGL(wfm_fft_kernel, dim3(nblk, nc), dim3(WFM_FFT / 8), 0, b->core.stream, b->d_chan, b->d_bufs, b->d_filters, b->d_utbl, b->d_nco);
        SDRX_HIP(hipGetLastError());
        b->core.note_launch("wfm_fft_kernel", (int)(nblk * nc), WFM_FFT / 8, (int)(2 * WFM_FFT * sizeof(float2) + (WFM_FFT / 4 + 1) * sizeof(float)));
    }
    hipLaunchKernelGGL(wfm_pend_kernel, dim3(nc), dim3(WFM_H), 0, b->core.stream, b->d_chan, b->d_bufs);
    SDRX_HIP(hipGetLastError());
    rc = demod_stream_after(producer, b->core.stream, b->cons_ev); if (rc) return rc;
    if (nblk) {
        hipLaunchKernelGGL(wfm_level_kernel, dim3(nblk, nc), dim3(256), 0, b->core.stream, b->d_chan, b->d_bufs);
        SDRX_HIP(hipGetLastError());
        hipLaunchKernelGGL(wfm_blockscan_kernel, dim3(nc), dim3(64), 0, b->core.stream, b->d_chan, b->d_bufs);
        SDRX_HIP(hipGetLastError());
        hipLaunchKernelGGL(wfm_demod_kernel, dim3(nblk, nc), dim3(256), 0, b->core.stream, b->d_chan, b->d_bufs);
        SDRX_HIP(hipGetLastError());
        hipLaunchKernelGGL(wfm_fixup_kernel, dim3(nc), dim3(64), 0, b->core.stream, b->d_chan, b->d_bufs);
        SDRX_HIP(hipGetLastError());
        hipLaunchKernelGGL(wfm_fir_kernel, dim3((unsigned)((max_out + 255) / 256), nc), dim3(256), 0, b->core.stream, b->d_chan, b->d_bufs, b->d_taps);
        SDRX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(wfm_carry_kernel, dim3(nc), dim3(WFM_H), 0, b->core.stream, b->d_chan, b->d_bufs);
    SDRX_HIP(hipGetLastError());
    rc = b->core.timer.end(b->core.stream); if (rc) return rc;
    for (int c = 0; c < b->n_ch; c++) {
        WfmHost& h = b->ch[(size_t)c];
        h.cur ^= 1;
        h.pending = (int)((h.pending + n_per_ch[c]) % WFM_H);
    }
    return SDRX_OK;
}

int sdrx_wfm_feed_dev(sdrx_wfm_t* b, const int16_t* const* d_iq, const int64_t* n_per_ch)
{
    if (!b || !d_iq || !n_per_ch) { set_error("sdrx_wfm_feed_dev: null argument"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    return feed_common(b, d_iq, n_per_ch);
}

int sdrx_wfm_feed_bank(sdrx_wfm_t* b, sdrx_chan_bank_t* bank)
{
    if (!b || !bank) { set_error("sdrx_wfm_feed_bank: null argument"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    void* ps = nullptr;
    int rc = sdrx_chan_bank_get_stream(bank, &ps); if (rc) return rc;
    std::vector<const int16_t*> d;
    std::vector<int64_t> n;
    rc = demod_gather_bank(bank, b->n_ch, "sdrx_wfm_feed_bank", d, n); if (rc) return rc;
    return feed_common(b, d.data(), n.data(), static_cast<hipStream_t>(ps));
}

int sdrx_wfm_feed(sdrx_wfm_t* b, const int16_t* const* iq, const int64_t* n_per_ch)
{
    if (!b || !iq || !n_per_ch) { set_error("sdrx_wfm_feed: null argument"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    std::vector<const int16_t*> d;
    int rc = demod_stage_inputs(b->ch, b->core.stream, iq, n_per_ch, "sdrx_wfm_feed", d); if (rc) return rc;
    rc = feed_common(b, d.data(), n_per_ch); if (rc) return rc;
    SDRX_HIP(hipStreamSynchronize(b->core.stream));            // the caller's buffers are free again on return
    return SDRX_OK;
}

int64_t sdrx_wfm_read(sdrx_wfm_t* b, int32_t c, int16_t* audio, int64_t cap)
{
    if (!b || c < 0 || c >= b->n_ch || cap < 0 || (cap > 0 && !audio)) { set_error("sdrx_wfm_read: bad argument"); return SDRX_EINVAL; }
    WfmChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    const int64_t n = std::min<int64_t>(s.n_out, cap);
    if (n == 0) return 0;
    SDRX_HIP(hipMemcpy(audio, demod_place<WfmBufs>(b->ch[(size_t)c].arena.p, b->ch[(size_t)c].cap_in, work).audio, (size_t)n * 2, hipMemcpyDeviceToHost));
    return n;
}

int sdrx_wfm_last_dev(sdrx_wfm_t* b, int32_t c, const int16_t** d_audio, int64_t* n)
{
    if (!b || c < 0 || c >= b->n_ch || !d_audio || !n) { set_error("sdrx_wfm_last_dev: bad argument"); return SDRX_EINVAL; }
    WfmChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    *d_audio = demod_place<WfmBufs>(b->ch[(size_t)c].arena.p, b->ch[(size_t)c].cap_in, work).audio;
    *n = s.n_out;
    return SDRX_OK;
}

int sdrx_wfm_squelch_open(sdrx_wfm_t* b, int32_t c)
{
    if (!b || c < 0 || c >= b->n_ch) { set_error("sdrx_wfm_squelch_open: bad argument"); return SDRX_EINVAL; }
    WfmChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    return s.sq_open;
}

int sdrx_wfm_levels(sdrx_wfm_t* b, int32_t c, double* sum, double* peak, int64_t* count, int reset)
{
    if (!b || c < 0 || c >= b->n_ch) { set_error("sdrx_wfm_levels: bad argument"); return SDRX_EINVAL; }
    WfmChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    if (sum) *sum = s.magsq_sum;
    if (peak) *peak = s.magsq_peak;
    if (count) *count = s.magsq_count;
    if (!reset) return SDRX_OK;                           // getMagSqLevels: sum, peak and count back to 0
    return demod_zero_levels(b->core, b->d_chan + c, offsetof(WfmChan, magsq_sum), offsetof(WfmChan, magsq_peak), offsetof(WfmChan, magsq_count));
}

int sdrx_wfm_get_design(sdrx_wfm_t* b, int32_t c, int32_t* ntaps_per_phase, float* taps, int32_t taps_cap,
                        float* filter_iq, int32_t* nco_inc, float* squelch_level)
{
    if (!b || c < 0 || c >= b->n_ch) { set_error("sdrx_wfm_get_design: bad channel"); return SDRX_EINVAL; }
    const int nt = b->taps.ntaps[(size_t)c];
    if (ntaps_per_phase) *ntaps_per_phase = nt;
    if (taps && taps_cap > 0) std::memcpy(taps, &b->taps.all[(size_t)b->taps.off[(size_t)c]], (size_t)std::min(taps_cap, nt * 16) * 4);
    if (filter_iq) std::memcpy(filter_iq, &b->filters_all[(size_t)c * WFM_FFT * 2], WFM_FFT * 8);
    if (nco_inc) *nco_inc = b->h_chan[(size_t)c].nco_inc;
    if (squelch_level) *squelch_level = b->h_chan[(size_t)c].squelch_level;
    return SDRX_OK;
}

int sdrx_wfm_sync(sdrx_wfm_t* b) { return b ? b->core.sync() : SDRX_EINVAL; }

int sdrx_wfm_set_stream(sdrx_wfm_t* b, void* hip_stream) { return b ? b->core.set_stream(hip_stream) : SDRX_EINVAL; }

int sdrx_wfm_get_stream(sdrx_wfm_t* b, void** hip_stream) { return b ? b->core.get_stream(hip_stream) : SDRX_EINVAL; }

int sdrx_wfm_set_timing(sdrx_wfm_t* b, int enabled) { return b ? b->core.set_timing(enabled) : SDRX_EINVAL; }

int sdrx_wfm_get_timing(sdrx_wfm_t* b, double* total_ms, int64_t* feeds, int reset) { return b ? b->core.get_timing(total_ms, feeds, reset) : SDRX_EINVAL; }

int sdrx_wfm_last_launch(const sdrx_wfm_t* b, char* kernel_name, int name_cap, int* grid, int* block, int* lds_bytes) { return b ? b->core.last_launch(kernel_name, name_cap, grid, block, lds_bytes) : SDRX_EINVAL; }

} // extern "C"
