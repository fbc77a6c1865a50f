// libsdrx.so: sdrx_backend_* -- per-channel NCO -> Interpolator -> fftfilt -> discriminator bank, the
// common front of the channelrx demods' feed() (nfmdemod.cpp:150-163, ssbdemod.cpp:158-172).
// Host side: filter / tap / table design exactly as the reference does it at configure time
// (Interpolator::create interpolator.cpp:21-129, fftfilt::create_filter fftfilt.cpp:108-146,
// NCO::initTable nco.cpp:30-39, g_fft::fftCosInit gfft.h:141-150), launches, state bookkeeping.
#include "sdrx_common.hpp"
#include "backend_kernels.hpp"
#include "backend_design.hpp"
#include "backend_view.hpp"
#include "demod_common.hpp"
#include <cstddef>
#include <vector>
#include <cmath>
#include <cstring>
#include <new>
#include <algorithm>

using namespace sdrx;

namespace {

// One channel's work arena for feeds of up to cap_in samples.  The fronts of res (the resampled samples waiting for a full
// fftfilt block) and of tail (slot 0: ovlbuf) carry state from feed to feed.
void work(Carver& k, int64_t cap_in, size_t half, BeBufs& u)
{
    // pending (<512) + at most one resampler output per input (distance step >= 1 by construction of decimate())
    const size_t n_res_max = (size_t)cap_in + 1024;
    const size_t n_blk_max = n_res_max / half + 2;
    u.mixed = k.take<float2>((size_t)(BE_HIST + cap_in));
    u.ph = k.take<uint16_t>((size_t)cap_in);
    u.res = k.take_kept<float2>(n_res_max + BE_FFT, BE_FFT);
    u.head = k.take<float2>(n_blk_max * half);
    u.tail = k.take_kept<float2>((n_blk_max + 1) * half, half);
    u.cplx_out = k.take<float2>(n_res_max);
    u.real_out = k.take<float>(n_res_max);
}

struct ChanHost {
    sdrx_backend_cfg cfg;
    DevBuf arena;                 // work()'s layout for cap_in samples
    uint32_t* hist[2] = { nullptr, nullptr };   // BE_HIST packed Samples, then BE_HIST NCOF table indices
    int cur = 0;
    int64_t cap_in = 0;
    DevBuf stage_in;              // host-pointer feeds
    auto lay() const { return [this](Carver& k, int64_t cap, BeBufs& u) { work(k, cap, cfg.filt_mode >= 4 ? BE_FFT : BE_FFT / 2, u); }; }
    BeBufs placed() const { return demod_place<BeBufs>(arena.p, cap_in, lay()); }      // null pointers before the first feed
};

} // namespace

struct sdrx_backend {
    HandleCore core;
    int n_ch = 0;
    std::vector<ChanHost> ch;
    std::vector<BeChan> h_chan;   // host mirror of the config part (state lives on the device)
    BeChan* d_chan = nullptr;
    BeBufs* d_bufs = nullptr;
    DevBuf sched;                 // bank-wide, channel-interleaved: entry o of channel c at [o * n_ch + c]
    int64_t sched_cap = 0;        // entries per channel
    BeBufs* h_bufs = nullptr;     // pinned: the per-feed table goes to the device in one async copy
    hipEvent_t bufs_ev = nullptr; // recorded behind that copy; waited on before the table is rewritten
    hipEvent_t prod_ev = nullptr, cons_ev = nullptr;       // device-side ordering against a producer stream (sdrx_backend_feed_bank)
    float* d_nco = nullptr; float* d_taps = nullptr; float2* d_filters = nullptr;
    float* d_utbl = nullptr; float* d_utbl2 = nullptr;     // g_fft cosine tables for N = 1024 / 2048
    bool any1024 = false, any2048 = false;
    bool any_dyadic = false;      // some resampling ratio has a closed-form schedule
    bool any_ncof = false;        // some channel's oscillator is NCOF (backend_set_front)
    bool all_bypass = false;      // no channel has an Interpolator: no schedule, no FIR
    InterpTables taps; std::vector<float> filters_all;     // kept for inspection (tests)
    std::vector<int> perm, col_of;    // schedule column q holds channel perm[q]; col_of[c] is its inverse
    int* d_perm = nullptr;
    bool state_valid = false;     // d_chan state initialised
};

// the distance step and, where step * 2^q is an integer, the closed-form schedule's constants
static void set_step(BeChan& s, float step)
{
    s.step = step;
    design_dyadic_step(s.step, "SDRX_BE_SERIAL_SCHEDULE", &s.dy_q, &s.dy_S);
}

extern "C" {

int sdrx_backend_destroy(sdrx_backend_t* b)
{
    if (!b) return SDRX_OK;
    (void)hipSetDevice(b->core.device);
    if (b->core.stream) (void)hipStreamSynchronize(b->core.stream);
    for (auto& h : b->ch) {
        h.arena.release(); h.stage_in.release();
        for (int i = 0; i < 2; i++) if (h.hist[i]) (void)hipFree(h.hist[i]);
    }
    b->sched.release();
    if (b->d_chan) (void)hipFree(b->d_chan);
    if (b->d_bufs) (void)hipFree(b->d_bufs);
    if (b->h_bufs) (void)hipHostFree(b->h_bufs);
    if (b->bufs_ev) (void)hipEventDestroy(b->bufs_ev);
    if (b->prod_ev) (void)hipEventDestroy(b->prod_ev);
    if (b->cons_ev) (void)hipEventDestroy(b->cons_ev);
    if (b->d_nco) (void)hipFree(b->d_nco);
    if (b->d_taps) (void)hipFree(b->d_taps);
    if (b->d_perm) (void)hipFree(b->d_perm);
    if (b->d_filters) (void)hipFree(b->d_filters);
    if (b->d_utbl) (void)hipFree(b->d_utbl);
    if (b->d_utbl2) (void)hipFree(b->d_utbl2);
    b->core.close();
    delete b;
    return SDRX_OK;
}

// sdrx_backend_create with, where `cutoff` is not null, cutoff[c] in place of (double) cfg[c].interp_cutoff (backend_create_cutoff)
static int backend_create_impl(sdrx_backend_t** out, int device, int32_t n_ch, const sdrx_backend_cfg* cfg, const double* cutoff)
{
    if (!out) { set_error("sdrx_backend_create: null out"); return SDRX_EINVAL; }
    *out = nullptr;
    if (n_ch <= 0 || !cfg) { set_error("sdrx_backend_create: bad argument"); return SDRX_EINVAL; }
    for (int c = 0; c < n_ch; c++) {
        const sdrx_backend_cfg& k = cfg[c];
        if (k.in_rate <= 0 || k.out_rate <= 0 || k.out_rate > k.in_rate || k.filt_mode < 0 || k.filt_mode > 7 ||
            k.discri < 0 || k.discri > 2 || k.taps_per_phase <= 0 || k.taps_per_phase * 16 > BE_HIST) {
            set_error("sdrx_backend_create: bad channel configuration (need out_rate <= in_rate, taps_per_phase*16 <= 256)");
            return SDRX_EINVAL;
        }
        // Interpolator::create takes (int)(taps_per_phase * 16) taps per phase: none at all leaves an empty tap vector
        if ((int)((double)k.taps_per_phase * 16) < 1) {
            set_error("sdrx_backend_create: taps_per_phase too small (need (int)(taps_per_phase * 16) >= 1)");
            return SDRX_EINVAL;
        }
    }
    sdrx_backend* b = new (std::nothrow) sdrx_backend;
    if (!b) return SDRX_ENOMEM;
    int rc = b->core.open(device);
    if (rc) { delete b; return rc; }
    b->n_ch = n_ch;
    b->ch.resize((size_t)n_ch); b->h_chan.resize((size_t)n_ch);

    // NCO table (nco.cpp:30-39) and g_fft cosine tables (gfft.h:141-150)
    rc = design_upload(&b->d_nco, design_nco_table(BE_NCO_N));
    if (!rc) rc = design_upload(&b->d_utbl, design_gfft_table(BE_FFT));
    if (!rc) rc = design_upload(&b->d_utbl2, design_gfft_table(BE_FFT_MAX));
    if (rc) { sdrx_backend_destroy(b); return rc; }

    // per channel design
    SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&b->d_filters), (size_t)n_ch * 2 * BE_FFT_MAX * 8), sdrx_backend_destroy(b));   // [filter | filterOpp] per channel
    b->filters_all.assign((size_t)n_ch * 2 * BE_FFT_MAX * 2, 0.0f);
    for (int c = 0; c < n_ch; c++) {
        const sdrx_backend_cfg& k = cfg[c];
        ChanHost& h = b->ch[(size_t)c];
        h.cfg = k;
        b->taps.add((double)k.in_rate, cutoff ? cutoff[c] : (double)k.interp_cutoff, (double)k.taps_per_phase);
        const int flen = k.filt_mode >= 4 ? BE_FFT_MAX : BE_FFT;          // runDSB / runAsym: "double the FFT size used for SSB"
        // fftfilt::create_filter / create_dsb_filter / create_asym_filter.  which: 0 = filter, 1 = filterOpp (runAsym only:
        // low pass at f1 = the opposite band's width)
        auto design = [&](int which) -> int {
            float2* dst = b->d_filters + (size_t)c * 2 * BE_FFT_MAX + (size_t)which * BE_FFT_MAX;
            float* copy = &b->filters_all[((size_t)c * 2 + (size_t)which) * BE_FFT_MAX * 2];
            if (k.filt_mode == 7) {                         // create_rrc_filter(fb = f1, a = f2): no transform, the bins themselves
                std::vector<float> f((size_t)BE_FFT_MAX * 2);
                fftfilt_rrc(k.f1, k.f2, f.data(), BE_FFT_MAX);
                SDRX_HIP(hipMemcpy(dst, f.data(), f.size() * 4, hipMemcpyHostToDevice));
                std::copy(f.begin(), f.end(), copy);
                return SDRX_OK;
            }
            if (k.filt_mode < 4)
                return design_fft_filter<BE_FFT>(dst, b->d_utbl, b->core.stream, copy, [&](float* f, int h2) { fftfilt_fill_band(k.f1, k.f2, f, h2); });
            // fftfilt(f2, len) / create_asym_filter(fopp = f1, fin = f2)
            return design_fft_filter<BE_FFT_MAX>(dst, b->d_utbl2, b->core.stream, copy, [&](float* f, int h2) { fftfilt_fill_lowpass(which ? k.f1 : k.f2, f, h2); });
        };
        if (k.filt_mode) {
            int drc = design(0);
            if (!drc && k.filt_mode >= 5) drc = design(1);
            if (drc) { sdrx_backend_destroy(b); return drc; }
            (flen == BE_FFT ? b->any1024 : b->any2048) = true;
        }
        BeChan& s = b->h_chan[(size_t)c];
        std::memset(&s, 0, sizeof s);
        s.nco_inc = (int)(((float)k.nco_freq * BE_NCO_N) / (float)k.in_rate);          // NCO::setFreq (float math, truncation)
        set_step(s, (float)k.in_rate / (float)k.out_rate);
        s.ntaps = b->taps.ntaps[(size_t)c]; s.phase_steps = 16;
        s.taps_off = b->taps.off[(size_t)c]; s.filt_mode = k.filt_mode; s.filt_off = c * 2 * BE_FFT_MAX;
        s.discri = k.discri; s.fm_scaling = k.fm_scaling;
        if (s.dy_q >= 0) b->any_dyadic = true;
        s.half = flen / 2;
        for (int i = 0; i < 2; i++) {
            SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&h.hist[i]), BE_HIST * 6), sdrx_backend_destroy(b));
            SDRX_HIP_ELSE(hipMemsetAsync(h.hist[i], 0, BE_HIST * 6, b->core.stream), sdrx_backend_destroy(b));   // on the handle's own (non-blocking) stream: ordered before its kernels
        }
    }
    // schedule columns: channels sorted by tap table, so that a FIR tile of 16 columns normally sees one design
    b->perm.resize((size_t)n_ch); b->col_of.resize((size_t)n_ch);
    for (int c = 0; c < n_ch; c++) b->perm[(size_t)c] = c;
    std::stable_sort(b->perm.begin(), b->perm.end(), [&](int x, int y) { return b->taps.off[(size_t)x] < b->taps.off[(size_t)y]; });
    for (int q = 0; q < n_ch; q++) b->col_of[(size_t)b->perm[(size_t)q]] = q;
    SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&b->d_perm), (size_t)n_ch * sizeof(int)), sdrx_backend_destroy(b));
    SDRX_HIP_ELSE(hipMemcpy(b->d_perm, b->perm.data(), (size_t)n_ch * sizeof(int), hipMemcpyHostToDevice), sdrx_backend_destroy(b));
    rc = design_upload(&b->d_taps, b->taps.all);
    if (rc) { sdrx_backend_destroy(b); return rc; }
    SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&b->d_chan), (size_t)n_ch * sizeof(BeChan)), sdrx_backend_destroy(b));
    SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&b->d_bufs), (size_t)n_ch * sizeof(BeBufs)), sdrx_backend_destroy(b));
    SDRX_HIP_ELSE(hipHostMalloc(reinterpret_cast<void**>(&b->h_bufs), (size_t)n_ch * sizeof(BeBufs), hipHostMallocDefault), sdrx_backend_destroy(b));
    SDRX_HIP_ELSE(hipEventCreateWithFlags(&b->bufs_ev, hipEventDisableTiming), sdrx_backend_destroy(b));
    SDRX_HIP_ELSE(hipEventRecord(b->bufs_ev, b->core.stream), sdrx_backend_destroy(b));
    SDRX_HIP_ELSE(hipEventCreateWithFlags(&b->prod_ev, hipEventDisableTiming), sdrx_backend_destroy(b));
    SDRX_HIP_ELSE(hipEventCreateWithFlags(&b->cons_ev, hipEventDisableTiming), sdrx_backend_destroy(b));
    SDRX_HIP_ELSE(hipMemcpy(b->d_chan, b->h_chan.data(), (size_t)n_ch * sizeof(BeChan), hipMemcpyHostToDevice), sdrx_backend_destroy(b));
    *out = b;
    return SDRX_OK;
}

int sdrx_backend_create(sdrx_backend_t** out, int device, int32_t n_ch, const sdrx_backend_cfg* cfg)
{
    return backend_create_impl(out, device, n_ch, cfg, nullptr);
}

// producer != nullptr: the input samples are being written on that stream.  The schedule kernel (needs the counts only) is
// launched first and overlaps the producer; the readers of `in` (be_mix: NCO mix + raw history) wait for the producer on the
// device, and the producer's stream waits until they are done before it may run anything queued after this call.
static int feed_common(sdrx_backend* b, const int16_t* const* d_iq, const int64_t* n_per_ch, hipStream_t producer = nullptr)
{
    int64_t n_max = 0, n_res_bound = 0;
    for (int c = 0; c < b->n_ch; c++) {
        if (n_per_ch[c] < 0 || n_per_ch[c] > 0x0fffffff) { set_error("sdrx_backend_feed: bad length"); return SDRX_EINVAL; }
        ChanHost& h = b->ch[(size_t)c];
        int rc = demod_grow_arena<BeBufs>(h.arena, h.cap_in, std::max<int64_t>(n_per_ch[c], 1), b->core.stream, h.lay()); if (rc) return rc;
        n_max = std::max(n_max, n_per_ch[c]);
        // every resampler output after the first two of a stream consumes >= floor(step) inputs (distance >= step before the `-= 1` walk)
        const int64_t per_out = std::max<int64_t>(1, (int64_t)std::floor(b->h_chan[(size_t)c].step));
        if (!b->h_chan[(size_t)c].bypass) n_res_bound = std::max(n_res_bound, n_per_ch[c] / per_out + 4);
    }
    if (n_max + 1024 > b->sched_cap) {
        int64_t cap = b->sched_cap ? b->sched_cap : 8192;
        while (cap < n_max + 1024) cap *= 2;
        SDRX_HIP(hipStreamSynchronize(b->core.stream));
        int rc = b->sched.reserve((size_t)cap * (size_t)b->n_ch * sizeof(uint2)); if (rc) return rc;
        b->sched_cap = cap;
    }
    // per-feed table (pointers + n_in), pinned, one async copy
    SDRX_HIP(hipEventSynchronize(b->bufs_ev));            // previous feed's copy has read the table
    for (int c = 0; c < b->n_ch; c++) {
        ChanHost& h = b->ch[(size_t)c];
        BeBufs& u = b->h_bufs[c];
        u.in = reinterpret_cast<const uint32_t*>(d_iq[c]);
        u.hist = h.hist[h.cur]; u.hist_next = h.hist[h.cur ^ 1];
        u.ph_hist = reinterpret_cast<const uint16_t*>(u.hist + BE_HIST); u.ph_hist_next = reinterpret_cast<uint16_t*>(u.hist_next + BE_HIST);
        u.sched = static_cast<uint2*>(b->sched.p) + b->col_of[(size_t)c]; u.sched_stride = b->n_ch;
        Carver k{static_cast<char*>(h.arena.p)};
        h.lay()(k, h.cap_in, u);
        u.n_in = n_per_ch[c];
    }
    int rc = demod_upload_bufs(b->d_bufs, b->h_bufs, b->n_ch, b->bufs_ev, b->core.stream); if (rc) return rc;
    const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(256, (n_max + BE_HIST + 255) / 256));
    // closed-form schedule for dyadic ratios (prep decides per channel and feed), the serial walk for the rest
    hipLaunchKernelGGL(be_sched_dyadic_prep_kernel, dim3((unsigned)((b->n_ch + 63) / 64)), dim3(64), 0, b->core.stream, b->d_chan, b->d_bufs, b->d_perm, b->n_ch);
    SDRX_HIP(hipGetLastError());
    if (b->any_dyadic && !b->all_bypass) {
        hipLaunchKernelGGL(be_sched_dyadic_fill_kernel, dim3((unsigned)((n_res_bound + 255) / 256), (unsigned)((b->n_ch + 63) / 64)), dim3(256), 0,
                           b->core.stream, b->d_chan, b->d_bufs, b->d_perm, b->n_ch);
        SDRX_HIP(hipGetLastError());
    }
    // always launched: lanes whose channel the closed form took exit at once (prep's off-grid guard can hand a channel back)
    if (!b->all_bypass) {
        hipLaunchKernelGGL(be_schedule_kernel, dim3((unsigned)((b->n_ch + 63) / 64)), dim3(64), 0, b->core.stream, b->d_chan, b->d_bufs, b->d_perm, b->n_ch);
        SDRX_HIP(hipGetLastError());
    }
    if (b->any_ncof) {                                      // needs the counts only, like the schedule
        hipLaunchKernelGGL(be_ncof_kernel, dim3((unsigned)((b->n_ch + 63) / 64)), dim3(64), 0, b->core.stream, b->d_chan, b->d_bufs, b->n_ch);
        SDRX_HIP(hipGetLastError());
    }
    rc = demod_stream_after(b->core.stream, producer, b->prod_ev); if (rc) return rc;
    // be_mix stages the 16 KB NCO table per workgroup: at least 8192 samples each
    const unsigned gx_mix = (unsigned)std::max<int64_t>(1, std::min<int64_t>(256, (n_max + BE_HIST + 8191) / 8192));
    hipLaunchKernelGGL(be_mix_kernel, dim3(gx_mix, (unsigned)b->n_ch), dim3(256), 0, b->core.stream, b->d_chan, b->d_bufs, b->d_nco);
    SDRX_HIP(hipGetLastError());
    rc = demod_stream_after(producer, b->core.stream, b->cons_ev); if (rc) return rc;
    if (!b->all_bypass) {
        hipLaunchKernelGGL(be_fir_kernel, dim3((unsigned)((n_res_bound + BE_FIR_TO - 1) / BE_FIR_TO), (unsigned)((b->n_ch + BE_FIR_TC - 1) / BE_FIR_TC)), dim3(256), 0,
                           b->core.stream, b->d_chan, b->d_bufs, b->d_taps, b->d_perm, b->n_ch);
        SDRX_HIP(hipGetLastError());
    }
    if (b->any1024) {
        const unsigned max_blocks = (unsigned)((n_max + BE_FFT) / (BE_FFT / 2) + 1);
        hipLaunchKernelGGL(be_fft_kernel<BE_FFT>, dim3(max_blocks, (unsigned)b->n_ch), dim3(BE_FFT / 8), 0, b->core.stream, b->d_chan, b->d_bufs, b->d_filters, b->d_utbl);
        SDRX_HIP(hipGetLastError());
    }
    if (b->any2048) {
        const unsigned max_blocks = (unsigned)((n_max + BE_FFT_MAX) / (BE_FFT_MAX / 2) + 1);
        hipLaunchKernelGGL(be_fft_kernel<BE_FFT_MAX>, dim3(max_blocks, (unsigned)b->n_ch), dim3(BE_FFT_MAX / 8), 0, b->core.stream, b->d_chan, b->d_bufs, b->d_filters, b->d_utbl2);
        SDRX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(be_finish_kernel, dim3(gx, (unsigned)b->n_ch), dim3(256), 0, b->core.stream, b->d_chan, b->d_bufs);
    SDRX_HIP(hipGetLastError());
    hipLaunchKernelGGL(be_carry_kernel, dim3((unsigned)b->n_ch), dim3(256), 0, b->core.stream, b->d_chan, b->d_bufs);
    SDRX_HIP(hipGetLastError());
    for (auto& h : b->ch) h.cur ^= 1;
    return SDRX_OK;
}

int sdrx_backend_feed_dev(sdrx_backend_t* b, const int16_t* const* d_iq, const int64_t* n_per_ch)
{
    if (!b || !d_iq || !n_per_ch) { set_error("sdrx_backend_feed_dev: null argument"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    return feed_common(b, d_iq, n_per_ch);
}

int sdrx_backend_feed_bank(sdrx_backend_t* b, sdrx_chan_bank_t* bank)
{
    if (!b || !bank) { set_error("sdrx_backend_feed_bank: null argument"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    void* ps = nullptr;
    int rc = sdrx_chan_bank_get_stream(bank, &ps); if (rc) return rc;
    std::vector<const int16_t*> d;
    std::vector<int64_t> n;
    rc = demod_gather_bank(bank, b->n_ch, "sdrx_backend_feed_bank", d, n, "the back-end"); if (rc) return rc;
    return feed_common(b, d.data(), n.data(), static_cast<hipStream_t>(ps));
}

int sdrx_backend_feed(sdrx_backend_t* b, const int16_t* const* iq, const int64_t* n_per_ch)
{
    if (!b || !iq || !n_per_ch) { set_error("sdrx_backend_feed: null argument"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    SDRX_HIP(hipStreamSynchronize(b->core.stream));
    std::vector<const int16_t*> d((size_t)b->n_ch);
    for (int c = 0; c < b->n_ch; c++) {
        ChanHost& h = b->ch[(size_t)c];
        int rc = h.stage_in.reserve((size_t)std::max<int64_t>(n_per_ch[c], 1) * 4); if (rc) return rc;
        if (n_per_ch[c] > 0) SDRX_HIP(hipMemcpyAsync(h.stage_in.p, iq[c], (size_t)n_per_ch[c] * 4, hipMemcpyHostToDevice, b->core.stream));
        d[(size_t)c] = static_cast<const int16_t*>(h.stage_in.p);
    }
    return feed_common(b, d.data(), n_per_ch);
}

int64_t sdrx_backend_read(sdrx_backend_t* b, int32_t c, float* out, int64_t cap_floats)
{
    if (!b || c < 0 || c >= b->n_ch || cap_floats < 0 || (cap_floats > 0 && !out)) { set_error("sdrx_backend_read: bad argument"); return SDRX_EINVAL; }
    const float* src; int64_t n_floats;
    int rc = sdrx_backend_last_dev(b, c, &src, &n_floats); if (rc) return rc;
    if (n_floats > cap_floats) n_floats = cap_floats;
    if (n_floats == 0) return 0;
    SDRX_HIP(hipMemcpy(out, src, (size_t)n_floats * 4, hipMemcpyDeviceToHost));
    return n_floats;
}

int sdrx_backend_last_dev(sdrx_backend_t* b, int32_t c, const float** d_out, int64_t* n_floats)
{
    if (!b || c < 0 || c >= b->n_ch || !d_out || !n_floats) { set_error("sdrx_backend_last_dev: bad argument"); return SDRX_EINVAL; }
    BeChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    const bool real = s.discri != 0;
    const BeBufs u = b->ch[(size_t)c].placed();
    *d_out = real ? u.real_out : reinterpret_cast<const float*>(u.cplx_out);
    *n_floats = (int64_t)s.n_out * (real ? 1 : 2);
    return SDRX_OK;
}

int sdrx_backend_get_design(sdrx_backend_t* b, int32_t c, int32_t* ntaps_per_phase, float* taps, int32_t taps_cap,
                            float* filter_iq, int32_t* nco_inc)
{
    if (!b || c < 0 || c >= b->n_ch) { set_error("sdrx_backend_get_design: bad channel"); return SDRX_EINVAL; }
    const int nt = b->taps.ntaps[(size_t)c];
    if (ntaps_per_phase) *ntaps_per_phase = nt;
    if (taps) std::memcpy(taps, &b->taps.all[(size_t)b->taps.off[(size_t)c]], (size_t)std::min(taps_cap, nt * 16) * 4);
    if (filter_iq) std::memcpy(filter_iq, &b->filters_all[(size_t)c * 2 * BE_FFT_MAX * 2], BE_FFT_MAX * 8);
    if (nco_inc) *nco_inc = b->h_chan[(size_t)c].nco_inc;
    return SDRX_OK;
}

int sdrx_backend_sync(sdrx_backend_t* b) { return b ? b->core.sync() : SDRX_EINVAL; }

} // extern "C"

namespace sdrx {

int backend_view(sdrx_backend_t* b, int32_t c, BackendView* v)
{
    if (!b || c < 0 || c >= b->n_ch || !v) { set_error("backend_view: bad argument"); return SDRX_EINVAL; }
    const ChanHost& h = b->ch[(size_t)c];
    const BeBufs u = h.placed();
    v->out = h.cfg.discri ? static_cast<const void*>(u.real_out) : static_cast<const void*>(u.cplx_out);
    v->n_out = reinterpret_cast<const int*>(reinterpret_cast<const char*>(b->d_chan + c) + offsetof(BeChan, n_out));
    return SDRX_OK;
}

int backend_create_cutoff(sdrx_backend_t** out, int device, int32_t n_ch, const sdrx_backend_cfg* cfg, const double* cutoff)
{
    if (n_ch > 0 && !cutoff) { set_error("backend_create_cutoff: bad argument"); return SDRX_EINVAL; }
    return backend_create_impl(out, device, n_ch, cfg, cutoff);
}

int backend_set_stream(sdrx_backend_t* b, hipStream_t hip_stream)
{
    return b ? b->core.set_stream(hip_stream) : SDRX_EINVAL;
}

int backend_set_front(sdrx_backend_t* b, int32_t c, int bypass, int ncof)
{
    if (!b || c < 0 || c >= b->n_ch) { set_error("backend_set_front: bad argument"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    SDRX_HIP(hipStreamSynchronize(b->core.stream));
    BeChan& s = b->h_chan[(size_t)c];                       // the config part and a fresh state
    const sdrx_backend_cfg& k = b->ch[(size_t)c].cfg;
    s.bypass = bypass ? 1 : 0;
    s.ncof = ncof ? 1 : 0;
    s.ncof_inc = ((float)k.nco_freq * BE_NCO_N) / (float)k.in_rate;     // NCOF::setFreq(Real freq, Real sampleRate)
    b->any_ncof = false; b->all_bypass = true;
    for (const BeChan& q : b->h_chan) { b->any_ncof = b->any_ncof || q.ncof; b->all_bypass = b->all_bypass && q.bypass; }
    SDRX_HIP(hipMemcpy(b->d_chan + c, &s, sizeof s, hipMemcpyHostToDevice));
    return SDRX_OK;
}

int backend_set_nomix(sdrx_backend_t* b, int32_t c)
{
    if (!b || c < 0 || c >= b->n_ch) { set_error("backend_set_nomix: bad argument"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    SDRX_HIP(hipStreamSynchronize(b->core.stream));
    BeChan& s = b->h_chan[(size_t)c];                       // the config part and a fresh state
    s.nomix = 1;
    SDRX_HIP(hipMemcpy(b->d_chan + c, &s, sizeof s, hipMemcpyHostToDevice));
    return SDRX_OK;
}

int backend_start_at(sdrx_backend_t* b, int32_t c, float step, float distance)
{
    if (!b || c < 0 || c >= b->n_ch || !(step >= 1.0f) || !(distance >= 0.0f)) { set_error("backend_start_at: bad argument"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    SDRX_HIP(hipStreamSynchronize(b->core.stream));
    BeChan& s = b->h_chan[(size_t)c];                       // the config part and a fresh state
    set_step(s, step);
    b->any_dyadic = false;                                  // recomputed: the channel may have left the closed form
    for (const BeChan& k : b->h_chan) b->any_dyadic = b->any_dyadic || k.dy_q >= 0;
    // h_chan keeps distance 0 (it mirrors the configuration; nothing uploads it again after create): the start lives on the
    // device only, and a caller that wants a fresh stream makes a fresh back-end and calls this again (sdrx_udpsrc_reset)
    BeChan fresh = s;
    fresh.distance = distance;
    SDRX_HIP(hipMemcpy(b->d_chan + c, &fresh, sizeof fresh, hipMemcpyHostToDevice));
    return SDRX_OK;
}

} // namespace sdrx
