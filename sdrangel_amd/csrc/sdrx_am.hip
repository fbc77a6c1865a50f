// libsdrx.so: sdrx_am_* -- N AM demodulators (AMDemod::feed / processOneSample, plugins/channelrx/demodam/amdemod.cpp:101-276,
// in envelope mode or, per channel of sdrx_am_create_ex, with m_pll: synchronous AM) on one device: int16 I/Q at the
// channelizer's output rate in, mono qint16 audio out.  The front (NCO, Interpolator) is a channel back-end the handle owns and
// launches on its own stream; the tail's kernels are in am_kernels.hpp, those of synchronous AM in am_sync_kernels.hpp.  Host
// side: the design products as the constructor / applyChannelSettings / applyAudioSampleRate / applySettings derive them
// (amdemod.cpp:55-90, 360-475), the two layouts and the launches; the rest is demod_bank.hpp's.
#include "sdrx_common.hpp"
#include "am_kernels.hpp"
#include "am_sync_kernels.hpp"
#include "backend_design.hpp"
#include "demod_bank.hpp"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace sdrx;

// what one channel is made from: sdrx_am_create fills `sync` with zeros
struct AmCfgEx { sdrx_am_cfg base; sdrx_am_sync_cfg sync; };

// m_audioSampleRate and m_rfBandwidth when AMDemod was constructed: what SSBFilter is designed from, once
static int am_ssb_design_rate(const sdrx_am_sync_cfg& y) { return y.ssb_design_rate ? y.ssb_design_rate : 48000; }
static float am_ssb_design_bw(const sdrx_am_sync_cfg& y) { return y.ssb_design_bw != 0.0f ? y.ssb_design_bw : 5000.0f; }

struct AmFamily : DemodDefaults {
    using Handle = sdrx_am;
    using Cfg = AmCfgEx;
    using Chan = AmChan;
    using Bufs = AmBufs;
    static constexpr const char* name = "sdrx_am";
    static constexpr const float2* AmBufs::* input = &AmBufs::ci;
    static constexpr int bp_taps = AM_BP_H + 1 + AMS_PF_H + 1;      // Bandpass taps, m_pllFilt taps

    static int validate(int32_t n_ch, const AmCfgEx* cfg)
    {
        if (n_ch <= 0 || !cfg) { set_error("sdrx_am_create: bad argument"); return SDRX_EINVAL; }
        for (int c = 0; c < n_ch; c++) {
            const sdrx_am_cfg& k = cfg[c].base;
            const sdrx_am_sync_cfg& y = cfg[c].sync;
            if (y.sync_op < 0 || y.sync_op > 2) { set_error("sdrx_am_create_ex: bad sync configuration (need 0 <= sync_op <= 2: DSB, USB, LSB)"); return SDRX_EINVAL; }
            if (y.ssb_design_rate < 0) { set_error("sdrx_am_create_ex: bad sync configuration (need ssb_design_rate >= 0; 0 is 48000)"); return SDRX_EINVAL; }
            if (!std::isfinite(y.ssb_design_bw) || y.ssb_design_bw < 0.0f) {
                set_error("sdrx_am_create_ex: bad sync configuration (ssb_design_bw must be finite and >= 0; 0 is 5000)"); return SDRX_EINVAL;
            }
            if (k.in_rate <= 0 || k.audio_rate < 1000 || k.audio_rate > k.in_rate) {
                set_error("sdrx_am_create: bad channel configuration (need 1000 <= audio_rate <= in_rate; the interpolating branch is left out)");
                return SDRX_EINVAL;
            }
            if (!(k.rf_bandwidth > 0.0f) || !(k.rf_bandwidth <= 1.0e7f)) {
                set_error("sdrx_am_create: bad channel configuration (need 0 < rf_bandwidth <= 1e7)"); return SDRX_EINVAL;
            }
            if (!std::isfinite(k.volume) || !std::isfinite(k.squelch_db)) {
                set_error("sdrx_am_create: bad channel configuration (volume and squelch_db must be finite)"); return SDRX_EINVAL;
            }
        }
        return SDRX_OK;
    }

    static void design(int c, const AmCfgEx& kx, sdrx_backend_cfg& f, AmChan& s, float* bp)
    {
        const sdrx_am_cfg& k = kx.base;
        f.in_rate = k.in_rate; f.nco_freq = k.nco_freq; f.out_rate = k.audio_rate;
        f.interp_cutoff = k.rf_bandwidth / 2.2f;            // m_interpolator.create(16, inputSampleRate, rfBandwidth / 2.2f)
        f.taps_per_phase = 4.5f;
        s.rate = k.audio_rate; s.D = k.audio_rate / 20; s.H = k.audio_rate / 10;
        s.level = (float)std::pow(10.0, (double)k.squelch_db / 10.0);      // CalcDb::powerFromdB
        s.volume = k.volume;
        s.att = 0.05f * (float)(uint32_t)k.audio_rate;
        s.gain = (float)(uint32_t)(k.audio_rate / 24);
        s.mute = k.audio_mute ? 1 : 0; s.bandpass = k.bandpass_enable ? 1 : 0;
        s.bp_off = c * bp_taps;
        s.agc_sum = (double)s.H * am_agc_initial();         // m_sum = (Type) m_history.size() * initial
        // m_bandpass.create(301, audioSampleRate, 300.0, rfBandwidth / 2.0f)
        demod_bandpass_design((double)k.audio_rate, 300.0, (double)(k.rf_bandwidth / 2.0f), bp);
        if (!kx.sync.pll) return;
        s.sync = AMS_DSB + kx.sync.sync_op;
        s.s_B = ams_block(s.sync); s.s_hn = ams_agc_len(k.audio_rate);
        s.pf_off = s.bp_off + AM_BP_H + 1;
        s.filt_off = c * AMS_DSB_FLEN;
        ams_lowpass_design((double)k.audio_rate, 200.0, bp + AM_BP_H + 1);  // m_pllFilt.create(101, sampleRate, 200.0)
        s.pk = ams_pll_design(k.audio_rate);
    }

    // one history set: [16 magsq | D roots | H fed values | 300 demods]
    static void hist(HistCarver& k, const AmChan& s, AmBufs& u)
    {
        k.pair(u.mhist, u.mhist_next, AM_MA);
        k.pair(u.rhist, u.rhist_next, (size_t)s.D);
        k.pair(u.vhist, u.vhist_next, (size_t)s.H);
        k.pair(u.dhist, u.dhist_next, AM_BP_HIST);
        if (!s.sync) return;
        // [100 open (re, im) | the open block | ovlbuf | rate / 4 magsq | the last block of zsum], all zeros in a fresh one: rings
        // and ovlbuf cleared by their classes, m_syncAMAGC's history by fill(0), m_syncAMBuff pinned to 0 (sdrx.h)
        k.pair(u.xhist, u.xhist_next, AMS_PF_HIST);
        k.pair(u.pend, u.pend_next, (size_t)s.s_B);
        k.pair(u.ovl, u.ovl_next, (size_t)s.s_B);
        k.pair(u.phist, u.phist_next, (size_t)s.s_hn);
        k.pair(u.zhist, u.zhist_next, (size_t)s.s_B);
    }

    // MovingAverage<double>(rate / 10, 0.003): every entry (double) 0.003f; everything else starts at 0 (the delay line too:
    // DoubleBufferFIFO does not clear its array, see sdrx.h)
    static void fresh(const AmChan& s, AmBufs& u) { for (int i = 0; i < s.H; i++) u.vhist_next[i] = am_agc_initial(); }

    static void work(Carver& k, size_t n, const AmChan& s, AmBufs& u)
    {
        const size_t nblk = n / 256 + 1;
        u.msq = k.take<float>(n); u.root = k.take<float>(n);
        u.cnt = k.take<int>(n); u.aidx = k.take<int>(n); u.fcnt = k.take<int>(n);
        u.dterm = k.take<double>(n); u.tot = k.take<double>(n);
        u.vnew = k.take<double>(n); u.uterm = k.take<double>(n); u.agc = k.take<double>(n);
        u.dem = k.take<float>(n);
        u.audio = k.take<int16_t>(n);
        u.blk_sum = k.take<double>(nblk); u.blk_peak = k.take<float>(nblk);
        if (!s.sync) return;
        // the filter hands out what it held back as well: fewer than one block more than the open samples of the feed
        const size_t no = n + AMS_BLOCK_MAX;
        u.xc = k.take<float2>(n); u.pf = k.take<float2>(n); u.osc = k.take<float2>(n);
        u.head = k.take<float2>(no); u.tail = k.take<float2>(no);
        u.pw = k.take<float>(no); u.sterm = k.take<double>(no); u.stot = k.take<double>(no);
    }

    static int64_t outputs_bound(const AmCfgEx& k, int64_t n_in) { return demod_outputs_bound(k.base.in_rate / k.base.audio_rate, n_in); }

    static int launch_sync(DemodBank<AmFamily>& b, unsigned nc, unsigned gx);

    static int launch(DemodBank<AmFamily>& b, unsigned nc, unsigned gx)
    {
        const unsigned gp = (nc + AM_PS_CH - 1) / AM_PS_CH;
        hipLaunchKernelGGL(am_level_kernel, dim3(gx, nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
        SDRX_HIP(hipGetLastError());
        hipLaunchKernelGGL(am_psum_kernel, dim3(gp), dim3(64), 0, b.core.stream, b.d_chan, b.d_bufs, b.n_ch, 0);
        SDRX_HIP(hipGetLastError());
        hipLaunchKernelGGL(am_gate_kernel, dim3(nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
        SDRX_HIP(hipGetLastError());
        hipLaunchKernelGGL(am_psum_kernel, dim3(gp), dim3(64), 0, b.core.stream, b.d_chan, b.d_bufs, b.n_ch, 1);
        SDRX_HIP(hipGetLastError());
        hipLaunchKernelGGL(am_demod_kernel, dim3(gx, nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
        SDRX_HIP(hipGetLastError());
        const bool any_sync = std::any_of(b.cfg.begin(), b.cfg.end(), [](const AmCfgEx& k) { return k.sync.pll != 0; });
        if (any_sync) { int rc = launch_sync(b, nc, gx); if (rc) return rc; }
        hipLaunchKernelGGL(am_out_kernel, dim3(gx, nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs, b.d_bp);
        SDRX_HIP(hipGetLastError());
        b.core.note_launch("am_out_kernel", (int)(gx * nc), 256, (int)((AM_BP_H + 1) * sizeof(float)));
        hipLaunchKernelGGL(am_carry_kernel, dim3(nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
        SDRX_HIP(hipGetLastError());
        if (any_sync) {
            hipLaunchKernelGGL(am_sync_carry_kernel, dim3(nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
            SDRX_HIP(hipGetLastError());
        }
        return SDRX_OK;
    }

    static double magsq(const AmChan& s) { return s.magsq; }
};

// the handle: the bank, and what only a handle with a sync channel has -- every such channel's frequency-domain filter
// (AMS_DSB_FLEN bins apiece) and the two g_fft cosine tables
struct sdrx_am : DemodBank<AmFamily> {
    float2* d_filt = nullptr;
    float* d_u2048 = nullptr;
    float* d_u1024 = nullptr;
    std::vector<float> filt_all;
    bool any_dsb = false, any_ssb = false;
};
using Bank = DemodBank<AmFamily>;

// the sync chain of a feed, between am_demod_kernel and am_out_kernel; gx blocks of 256 cover the feed's samples
int AmFamily::launch_sync(DemodBank<AmFamily>& bank, unsigned nc, unsigned gx)
{
    sdrx_am& b = static_cast<sdrx_am&>(bank);
    hipLaunchKernelGGL(am_sync_pack_kernel, dim3(gx, nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
    SDRX_HIP(hipGetLastError());
    hipLaunchKernelGGL(am_sync_prefilt_kernel, dim3(gx, nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs, b.d_bp);
    SDRX_HIP(hipGetLastError());
    hipLaunchKernelGGL(am_sync_walk_kernel, dim3((nc + AM_WALK_WAVES - 1) / AM_WALK_WAVES), dim3(64 * AM_WALK_WAVES), 0, b.core.stream,
                       b.d_chan, b.d_bufs, b.n_ch);
    SDRX_HIP(hipGetLastError());
    // a feed of at most 256 gx open samples completes at most 256 gx / B + 1 blocks
    if (b.any_dsb) {
        hipLaunchKernelGGL(am_sync_fft_kernel<AMS_DSB_FLEN>, dim3(gx * 256 / (AMS_DSB_FLEN / 2) + 1, nc), dim3(AMS_DSB_FLEN / 8), 0, b.core.stream,
                           b.d_chan, b.d_bufs, b.d_filt, b.d_u2048);
        SDRX_HIP(hipGetLastError());
    }
    if (b.any_ssb) {
        hipLaunchKernelGGL(am_sync_fft_kernel<AMS_SSB_FLEN>, dim3(gx * 256 / (AMS_SSB_FLEN / 2) + 1, nc), dim3(AMS_SSB_FLEN / 8), 0, b.core.stream,
                           b.d_chan, b.d_bufs, b.d_filt, b.d_u1024);
        SDRX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(am_sync_power_kernel, dim3(gx + AMS_BLOCK_MAX / 256, nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
    SDRX_HIP(hipGetLastError());
    hipLaunchKernelGGL(am_sync_psum_kernel, dim3((nc + PS_CH - 1) / PS_CH), dim3(64), 0, b.core.stream, b.d_chan, b.d_bufs, b.n_ch);
    SDRX_HIP(hipGetLastError());
    hipLaunchKernelGGL(am_sync_select_kernel, dim3(gx, nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
    SDRX_HIP(hipGetLastError());
    return SDRX_OK;
}

// DSBFilter and SSBFilter of the sync channels (amdemod.cpp:72-73, 376, 439): DSBFilter follows the channel's rf_bandwidth and
// audio_rate, SSBFilter keeps the constructor's design
static int am_design_filters(sdrx_am* b)
{
    bool any = false;
    for (const AmChan& s : b->h_chan) { any |= s.sync != AMS_OFF; b->any_dsb |= s.sync == AMS_DSB; b->any_ssb |= s.sync == AMS_USB || s.sync == AMS_LSB; }
    if (!any) return SDRX_OK;
    SDRX_HIP(hipSetDevice(b->core.device));
    b->filt_all.assign((size_t)b->n_ch * AMS_DSB_FLEN * 2, 0.0f);
    SDRX_HIP(hipMalloc(reinterpret_cast<void**>(&b->d_filt), b->filt_all.size() * 4));
    SDRX_HIP(hipMemset(b->d_filt, 0, b->filt_all.size() * 4));
    int rc = design_upload(&b->d_u2048, design_gfft_table(AMS_DSB_FLEN)); if (rc) return rc;
    rc = design_upload(&b->d_u1024, design_gfft_table(AMS_SSB_FLEN)); if (rc) return rc;
    for (int c = 0; c < b->n_ch; c++) {
        const AmChan& s = b->h_chan[(size_t)c];
        if (!s.sync) continue;
        const AmCfgEx& k = b->cfg[(size_t)c];
        float2* dst = b->d_filt + s.filt_off;
        float* copy = &b->filt_all[(size_t)s.filt_off * 2];
        if (s.sync == AMS_DSB) {
            const float f2 = (2.0f * k.base.rf_bandwidth) / (float)k.base.audio_rate;      // create_dsb_filter
            rc = design_fft_filter<AMS_DSB_FLEN>(dst, b->d_u2048, b->core.stream, copy, [&](float* f, int h2) { fftfilt_fill_lowpass(f2, f, h2); });
        } else {
            const float f2 = am_ssb_design_bw(k.sync) / (float)(uint32_t)am_ssb_design_rate(k.sync);   // fftfilt(0.0f, rfBW / rate, 1024)
            rc = design_fft_filter<AMS_SSB_FLEN>(dst, b->d_u1024, b->core.stream, copy, [&](float* f, int h2) { fftfilt_fill_band(0.0f, f2, f, h2); });
        }
        if (rc) return rc;
    }
    return SDRX_OK;
}

static int am_destroy(sdrx_am* b)
{
    if (!b) return SDRX_OK;
    (void)hipSetDevice(b->core.device);
    if (b->core.stream) (void)hipStreamSynchronize(b->core.stream);
    if (b->d_filt) (void)hipFree(b->d_filt);
    if (b->d_u2048) (void)hipFree(b->d_u2048);
    if (b->d_u1024) (void)hipFree(b->d_u1024);
    return Bank::destroy(b);
}

extern "C" {

int sdrx_am_create_ex(sdrx_am_t** out, int device, int32_t n_ch, const sdrx_am_cfg* cfg, const sdrx_am_sync_cfg* sync)
{
    if (out) *out = nullptr;
    std::vector<AmCfgEx> both;
    if (n_ch > 0 && cfg) {
        both.resize((size_t)n_ch);                              // value-initialised: sync all zero
        for (int c = 0; c < n_ch; c++) { both[(size_t)c].base = cfg[c]; if (sync) both[(size_t)c].sync = sync[c]; }
    }
    int rc = Bank::create(out, device, n_ch, both.empty() ? nullptr : both.data()); if (rc) return rc;
    rc = am_design_filters(*out);
    if (rc) { am_destroy(*out); *out = nullptr; }
    return rc;
}
int sdrx_am_create(sdrx_am_t** out, int device, int32_t n_ch, const sdrx_am_cfg* cfg) { return sdrx_am_create_ex(out, device, n_ch, cfg, nullptr); }
int sdrx_am_destroy(sdrx_am_t* b) { return am_destroy(b); }
int sdrx_am_reset(sdrx_am_t* b) { return Bank::reset(b); }
int sdrx_am_feed_dev(sdrx_am_t* b, const int16_t* const* d_iq, const int64_t* n_per_ch) { return Bank::feed_dev(b, d_iq, n_per_ch); }
int sdrx_am_feed_bank(sdrx_am_t* b, sdrx_chan_bank_t* bank) { return Bank::feed_bank(b, bank); }
int sdrx_am_feed(sdrx_am_t* b, const int16_t* const* iq, const int64_t* n_per_ch) { return Bank::feed(b, iq, n_per_ch); }
int64_t sdrx_am_read(sdrx_am_t* b, int32_t c, int16_t* audio, int64_t cap) { return Bank::read(b, "read", c, audio, cap, &AmBufs::audio, &AmChan::n, 2); }
int sdrx_am_last_dev(sdrx_am_t* b, int32_t c, const int16_t** d_audio, int64_t* n) { return Bank::last_dev(b, "last_dev", c, d_audio, n, &AmBufs::audio, &AmChan::n); }
int sdrx_am_squelch_open(sdrx_am_t* b, int32_t c) { return Bank::flag(b, "squelch_open", c, &AmChan::sq_open); }
int sdrx_am_levels(sdrx_am_t* b, int32_t c, double* magsq, double* sum, double* peak, int64_t* count, int reset) { return Bank::levels(b, c, magsq, sum, peak, count, reset); }

int sdrx_am_get_design(sdrx_am_t* b, int32_t c, int32_t* ntaps_per_phase, float* taps, int32_t taps_cap,
                       float* bandpass_taps, int32_t* nco_inc, float* squelch_level)
{
    if (!Bank::in_range(b, c)) return Bank::fail("get_design", ": bad channel");
    int rc = sdrx_backend_get_design(b->front, c, ntaps_per_phase, taps_cap > 0 ? taps : nullptr, taps_cap, nullptr, nco_inc); if (rc) return rc;
    if (bandpass_taps) std::memcpy(bandpass_taps, &b->bp_all[(size_t)b->h_chan[(size_t)c].bp_off], (AM_BP_H + 1) * 4);
    if (squelch_level) *squelch_level = b->h_chan[(size_t)c].level;
    return SDRX_OK;
}

int sdrx_am_pll(sdrx_am_t* b, int32_t c, int32_t* locked, float* freq)
{
    AmChan s;
    int rc = Bank::fetch(b, "pll", c, &s); if (rc) return rc;
    if (locked) *locked = s.sync != AMS_OFF && pll_locked(s.pk, s.ps) ? 1 : 0;       // getPllLocked: m_settings.m_pll && m_pll.locked()
    if (freq) *freq = s.ps.freq;
    return SDRX_OK;
}

int sdrx_am_get_sync_design(sdrx_am_t* b, int32_t c, float* pll_filt_taps, float* filter_iq, int32_t* filter_len, float* pll_coef5)
{
    if (!Bank::in_range(b, c)) return Bank::fail("get_sync_design", ": bad channel");
    const AmChan& s = b->h_chan[(size_t)c];
    if (!s.sync) return Bank::fail("get_sync_design", ": an envelope channel has no sync design");
    if (pll_filt_taps) std::memcpy(pll_filt_taps, &b->bp_all[(size_t)s.pf_off], (AMS_PF_H + 1) * 4);
    if (filter_iq) std::memcpy(filter_iq, &b->filt_all[(size_t)s.filt_off * 2], (size_t)ams_flen(s.sync) * 8);
    if (filter_len) *filter_len = ams_flen(s.sync);
    if (pll_coef5) { const float k[5] = { s.pk.a1, s.pk.a2, s.pk.b0, s.pk.b1, s.pk.b2 }; std::memcpy(pll_coef5, k, sizeof k); }
    return SDRX_OK;
}

int sdrx_am_sync(sdrx_am_t* b) { return b ? b->core.sync() : SDRX_EINVAL; }
int sdrx_am_set_stream(sdrx_am_t* b, void* hip_stream) { return Bank::set_stream(b, hip_stream); }
int sdrx_am_get_stream(sdrx_am_t* b, void** hip_stream) { return b ? b->core.get_stream(hip_stream) : SDRX_EINVAL; }
int sdrx_am_set_timing(sdrx_am_t* b, int enabled) { return b ? b->core.set_timing(enabled) : SDRX_EINVAL; }
int sdrx_am_get_timing(sdrx_am_t* b, double* total_ms, int64_t* feeds, int reset) { return b ? b->core.get_timing(total_ms, feeds, reset) : SDRX_EINVAL; }
int sdrx_am_last_launch(const sdrx_am_t* b, char* kernel_name, int name_cap, int* grid, int* block, int* lds_bytes) { return b ? b->core.last_launch(kernel_name, name_cap, grid, block, lds_bytes) : SDRX_EINVAL; }

} // extern "C"
