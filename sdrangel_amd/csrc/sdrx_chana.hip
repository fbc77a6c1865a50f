// libsdrx.so: sdrx_chana_* and sdrx_chanapll_* -- N ChannelAnalyzers (ChannelAnalyzer::feed, plugins/channelrx/chanalyzer/
// chanalyzer.cpp:92-182; with m_pll, m_fll and InputPLL through sdrx_chanapll_create) on one device: int16 I/Q at the channelizer's output rate in, the Samples the analyzer hands to its scope / spectrum sink
// out.  The front (NCOF, the optional Interpolator, fftfilt runSSB / runDSB / runFilt) is a channel back-end the handle owns and
// launches on its own stream; the tail's kernels are in chana_kernels.hpp and chana_pll_kernels.hpp.  Host side: the design products as the constructor,
// applySettings(settings, true), applyChannelSettings and start() leave them (:35-65, 247-392), the two layouts and the
// launches; the rest is demod_bank.hpp's.
#include "sdrx_common.hpp"
#include "chana_kernels.hpp"
#include "chana_pll_kernels.hpp"
#include "backend_design.hpp"
#include "demod_bank.hpp"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace sdrx;

namespace {
constexpr int CHANA_BLOCK_MAX = 1024;               // runDSB and runFilt hand out 1024 samples at a time, runSSB 512

// sdrx_chanapll_create's extras for the create underneath it: the PLL is let through, and the PSK order of every channel
thread_local bool tl_pll_ok = false;
thread_local const int32_t* tl_psk_order = nullptr;

struct ChanaDerived { int rate; float band, low; bool usb; float rrc_fb; };

// setFilters(rate, bandwidth, lowCutoff) (chanalyzer.cpp:281-306) and, where the Interpolator is in use, the last
// create_rrc_filter of applySettings (:353-359), which takes the settings' own bandwidth
ChanaDerived derive(const sdrx_chana_cfg& k)
{
    ChanaDerived d;
    d.rate = k.down_sample ? k.down_sample_rate : k.in_rate;
    d.band = (float)k.bandwidth; d.low = (float)k.low_cutoff; d.usb = true;
    if (d.band < 0) { d.band = -d.band; d.low = -d.low; d.usb = false; }
    if (d.band < 100.0f) { d.band = 100.0f; d.low = 0; }
    d.rrc_fb = k.down_sample ? (float)k.bandwidth / (float)(uint32_t)k.down_sample_rate : d.band / (float)d.rate;
    return d;
}

} // namespace

struct ChanaFamily : DemodDefaults {
    using Handle = sdrx_chana;
    using Cfg = sdrx_chana_cfg;
    using Chan = ChanaChan;
    using Bufs = ChanaBufs;
    static constexpr const char* name = "sdrx_chana";
    static constexpr const float2* ChanaBufs::* input = &ChanaBufs::s;
    // at most one filter input per input sample plus what the filter held back: fewer than one block
    static constexpr int work_extra = CHANA_BLOCK_MAX;

    static int validate(int32_t n_ch, const sdrx_chana_cfg* cfg)
    {
        const std::string who = tl_pll_ok ? "sdrx_chanapll_create" : "sdrx_chana_create";
        if (n_ch <= 0 || !cfg) { set_error(who + ": bad argument"); return SDRX_EINVAL; }
        for (int c = 0; c < n_ch; c++) {
            const sdrx_chana_cfg& k = cfg[c];
            if (k.in_rate <= 0) { set_error(who + ": bad channel configuration (need in_rate > 0)"); return SDRX_EINVAL; }
            // NCOF's wrap loops take |nco_freq| / in_rate trips per sample and never end once 4096 is below the phase's ulp
            if ((int64_t)k.nco_freq > k.in_rate || (int64_t)k.nco_freq < -(int64_t)k.in_rate) {
                set_error(who + ": bad channel configuration (need |nco_freq| <= in_rate)"); return SDRX_EINVAL;
            }
            if (!tl_pll_ok && (k.pll || k.fll || k.input_type == 1)) {
                set_error("sdrx_chana_create: the PLL, the FLL and the PLL input (input_type 1) are left out: their loop is serial and calls libm (DESIGN.md 10)");
                return SDRX_EINVAL;
            }
            if (tl_pll_ok && tl_psk_order && (tl_psk_order[c] < 1 || tl_psk_order[c] > 31)) {
                set_error(who + ": bad channel configuration (need 1 <= psk_order <= 31)"); return SDRX_EINVAL;
            }
            if (k.input_type < 0 || k.input_type > 2 || (!tl_pll_ok && k.input_type == 1)) {
                set_error(who + ": bad channel configuration (input_type is 0, signal, or 2, autocorrelation" + (tl_pll_ok ? ", or 1, the PLL)" : ")")); return SDRX_EINVAL;
            }
            if (k.span_log2 < 0 || k.span_log2 > 8) { set_error(who + ": bad channel configuration (need 0 <= span_log2 <= 8)"); return SDRX_EINVAL; }
            if (k.rrc_rolloff < 0 || k.rrc_rolloff > 100) { set_error(who + ": bad channel configuration (need 0 <= rrc_rolloff <= 100, in hundredths)"); return SDRX_EINVAL; }
            if (k.down_sample && (k.down_sample_rate < 1 || k.down_sample_rate > k.in_rate)) {
                set_error(who + ": bad channel configuration (down_sample needs 1 <= down_sample_rate <= in_rate; the interpolating branch is left out)");
                return SDRX_EINVAL;
            }
        }
        return SDRX_OK;
    }

    static void design(int c, const sdrx_chana_cfg& k, sdrx_backend_cfg& f, ChanaChan& s, float*)
    {
        const ChanaDerived d = derive(k);
        f.in_rate = k.in_rate; f.nco_freq = k.nco_freq; f.out_rate = d.rate;
        f.interp_cutoff = k.in_rate / 2.2f;                 // m_interpolator.create(16, inputSampleRate, inputSampleRate / 2.2f)
        f.taps_per_phase = 4.5f;
        if (k.ssb) {                                        // create_filter(lowCutoff / sampleRate, bandwidth / sampleRate), length 1024
            f.filt_mode = d.usb ? 2 : 3;
            f.f1 = d.low / (float)d.rate; f.f2 = d.band / (float)d.rate;
        } else if (k.rrc) {                                 // create_rrc_filter(fb, m_rrcRolloff / 100.0), length 2048
            f.filt_mode = 7;
            f.f1 = d.rrc_fb; f.f2 = (float)((uint32_t)k.rrc_rolloff / 100.0);
        } else {                                            // create_dsb_filter(bandwidth / sampleRate), length 2048
            f.filt_mode = 4;
            f.f2 = d.band / (float)d.rate;
        }
        s.decim = 1 << k.span_log2;
        s.swap_iq = (k.ssb && !d.usb) ? 1 : 0;
        s.corr = k.input_type == 2 ? 1 : 0;
        s.osc_out = k.input_type == 1 ? 1 : 0;
        // both loops as the configuration sequence leaves them; the state of a fresh one is all zeros (reset() of either class)
        s.pk = pll_design(k.in_rate, k.down_sample != 0, (unsigned)k.down_sample_rate, k.span_log2, k.pll != 0, k.fll != 0,
                          (unsigned)(tl_psk_order ? tl_psk_order[c] : 1));
    }

    // the front of a ChannelAnalyzer: NCOF, and no Interpolator unless m_downSample
    static int front_made(sdrx_backend_t* front, int n_ch, const sdrx_chana_cfg* cfg)
    {
        for (int c = 0; c < n_ch; c++) { int rc = backend_set_front(front, c, cfg[c].down_sample ? 0 : 1, 1); if (rc) return rc; }
        return SDRX_OK;
    }

    // one history set: fftcorr's [open block | last product].  A fresh one is all zeros: dataP is value-initialised
    static void hist(HistCarver& k, const ChanaChan& s, ChanaBufs& u)
    {
        const size_t n = s.corr ? (size_t)CHANA_CORR_H : 1;
        k.pair(u.part, u.part_next, n);
        k.pair(u.p, u.p_next, n);
    }

    static void work(Carver& k, size_t n, const ChanaChan& s, ChanaBufs& u)
    {
        u.out = k.take<int16_t>(2 * n);
        u.g = k.take<float2>(s.corr ? n : 1);
        u.pblk = k.take<float2>(s.corr ? (n / CHANA_CORR_H + 1) * CHANA_CORR_H : 1);
        u.avg = k.take<float2>(s.pk.mode != PLL_OFF || s.osc_out ? n : 1);
        u.osc = k.take<float2>(s.pk.mode != PLL_OFF ? n : 1);
    }

    // the filter's inputs (one per input without the Interpolator), and the filter adds what it held back
    static int64_t outputs_bound(const sdrx_chana_cfg& k, int64_t n_in)
    {
        return (k.down_sample ? demod_outputs_bound(k.in_rate / k.down_sample_rate, n_in) : n_in) + CHANA_BLOCK_MAX;
    }

    static int launch(DemodBank<ChanaFamily>& b, unsigned nc, unsigned gx);

    static double magsq(const ChanaChan& s) { return s.magsq; }
};

struct sdrx_chana : DemodBank<ChanaFamily> {
    float* d_utbl = nullptr;      // g_fft cosine table for N = 8192, made when a channel wants the autocorrelation
    bool walk = false, post = false;    // a channel runs a loop; a channel's Samples come from chana_post_kernel
};
using Bank = DemodBank<ChanaFamily>;

int ChanaFamily::launch(Bank& b, unsigned nc, unsigned gx)
{
    sdrx_chana& h = static_cast<sdrx_chana&>(b);
    hipLaunchKernelGGL(chana_group_kernel, dim3(gx, nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
    SDRX_HIP(hipGetLastError());
    b.core.note_launch("chana_group_kernel", (int)(gx * nc), 256, 0);
    if (h.walk) {
        const unsigned gw = (nc + CHANA_WALK_WAVES - 1) / CHANA_WALK_WAVES;
        hipLaunchKernelGGL(chana_walk_kernel, dim3(gw), dim3(64 * CHANA_WALK_WAVES), 0, b.core.stream, b.d_chan, b.d_bufs, (int)nc);
        SDRX_HIP(hipGetLastError());
        b.core.note_launch("chana_walk_kernel", (int)gw, 64 * CHANA_WALK_WAVES, 0);
    }
    if (h.post) {
        hipLaunchKernelGGL(chana_post_kernel, dim3(gx, nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
        SDRX_HIP(hipGetLastError());
    }
    if (h.d_utbl) {
        // a feed whose groups number at most gx * 256 completes at most this many blocks on top of an open one
        const unsigned nblk = (unsigned)((CHANA_CORR_H - 1 + (size_t)gx * 256) / CHANA_CORR_H);
        hipLaunchKernelGGL(chana_corr_kernel, dim3(nblk, nc), dim3(CHANA_CORR_N / 8), 0, b.core.stream, b.d_chan, b.d_bufs, h.d_utbl);
        SDRX_HIP(hipGetLastError());
        b.core.note_launch("chana_corr_kernel", (int)(nblk * nc), CHANA_CORR_N / 8, CHANA_CORR_LDS);
        hipLaunchKernelGGL(chana_emit_kernel, dim3(gx, nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
        SDRX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(chana_carry_kernel, dim3(nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
    SDRX_HIP(hipGetLastError());
    return SDRX_OK;
}

extern "C" {

int sdrx_chana_destroy(sdrx_chana_t* b)
{
    if (b && b->d_utbl) { (void)hipSetDevice(b->core.device); (void)hipStreamSynchronize(b->core.stream); (void)hipFree(b->d_utbl); b->d_utbl = nullptr; }
    return Bank::destroy(b);
}

int sdrx_chana_create(sdrx_chana_t** out, int device, int32_t n_ch, const sdrx_chana_cfg* cfg)
{
    int rc = Bank::create(out, device, n_ch, cfg); if (rc) return rc;
    bool any = false;
    for (int c = 0; c < n_ch; c++) any = any || cfg[c].input_type == 2;
    if (any) {
        rc = design_upload(&(*out)->d_utbl, design_gfft_table(CHANA_CORR_N));
        if (rc) { sdrx_chana_destroy(*out); *out = nullptr; return rc; }
    }
    return SDRX_OK;
}

int sdrx_chanapll_create(sdrx_chana_t** out, int device, int32_t n_ch, const sdrx_chana_cfg* cfg, const int32_t* psk_order)
{
    tl_pll_ok = true; tl_psk_order = psk_order;
    const int rc = sdrx_chana_create(out, device, n_ch, cfg);
    tl_pll_ok = false; tl_psk_order = nullptr;
    if (rc) return rc;
    for (const ChanaChan& s : (*out)->h_chan) {
        (*out)->walk = (*out)->walk || s.pk.mode != PLL_OFF;
        (*out)->post = (*out)->post || s.pk.mode != PLL_OFF || s.osc_out;
    }
    return SDRX_OK;
}

int sdrx_chanapll_state(sdrx_chana_t* b, int32_t c, int32_t* locked, float* freq, float* delta_phi, float* phi_hat)
{
    ChanaChan s;
    int rc = Bank::fetch(b, "state", c, &s); if (rc) return rc;
    if (locked) *locked = s.pk.mode != PLL_OFF && pll_locked(s.pk, s.ps) ? 1 : 0;         // m_settings.m_pll && m_pll.locked()
    if (freq) *freq = s.ps.freq;
    if (delta_phi) *delta_phi = s.ps.dphi;
    if (phi_hat) *phi_hat = s.ps.phi_hat;
    return SDRX_OK;
}

int sdrx_chana_reset(sdrx_chana_t* b) { return Bank::reset(b); }
int sdrx_chana_feed_dev(sdrx_chana_t* b, const int16_t* const* d_iq, const int64_t* n_per_ch) { return Bank::feed_dev(b, d_iq, n_per_ch); }
int sdrx_chana_feed_bank(sdrx_chana_t* b, sdrx_chan_bank_t* bank) { return Bank::feed_bank(b, bank); }
int sdrx_chana_feed(sdrx_chana_t* b, const int16_t* const* iq, const int64_t* n_per_ch) { return Bank::feed(b, iq, n_per_ch); }
int64_t sdrx_chana_read(sdrx_chana_t* b, int32_t c, int16_t* samples_iq, int64_t cap) { return Bank::read(b, "read", c, samples_iq, cap, &ChanaBufs::out, &ChanaChan::n_out, 4); }
int sdrx_chana_last_dev(sdrx_chana_t* b, int32_t c, const int16_t** d_samples_iq, int64_t* n) { return Bank::last_dev(b, "last_dev", c, d_samples_iq, n, &ChanaBufs::out, &ChanaChan::n_out); }

int sdrx_chana_positive_only(sdrx_chana_t* b, int32_t c)
{
    if (!Bank::in_range(b, c)) return Bank::fail("positive_only", ": bad argument");
    return b->cfg[(size_t)c].ssb ? 1 : 0;
}

int sdrx_chana_magsq(sdrx_chana_t* b, int32_t c, double* magsq)
{
    if (!magsq) return Bank::fail("magsq", ": bad argument");
    ChanaChan s;
    int rc = Bank::fetch(b, "magsq", c, &s); if (rc) return rc;
    *magsq = s.magsq;
    return SDRX_OK;
}

int sdrx_chana_get_design(sdrx_chana_t* b, int32_t c, int32_t* ntaps_per_phase, float* taps, int32_t taps_cap, float* filter_iq, float* nco_inc)
{
    if (!Bank::in_range(b, c)) return Bank::fail("get_design", ": bad channel");
    int rc = sdrx_backend_get_design(b->front, c, ntaps_per_phase, taps_cap > 0 ? taps : nullptr, taps_cap, filter_iq, nullptr); if (rc) return rc;
    const sdrx_chana_cfg& k = b->cfg[(size_t)c];
    if (nco_inc) *nco_inc = ((float)k.nco_freq * 4096) / (float)k.in_rate;         // NCOF::setFreq
    return SDRX_OK;
}

int sdrx_chana_seek(sdrx_chana_t* b, int32_t c, uint64_t filtered_samples)
{
    if (!Bank::in_range(b, c)) return Bank::fail("seek", ": bad argument");
    SDRX_HIP(hipSetDevice(b->core.device));
    SDRX_HIP(hipStreamSynchronize(b->core.stream));
    ChanaChan s = b->h_chan[(size_t)c];                     // the configuration and a fresh state
    s.usc = (unsigned)filtered_samples;
    // the groups closed so far: the first sample closes one, then every decim-th
    const uint64_t calls = (filtered_samples + (uint64_t)s.decim - 1) / (uint64_t)s.decim;
    s.fill = s.corr ? (int)(calls % CHANA_CORR_H) : 0;
    SDRX_HIP(hipMemcpy(b->d_chan + c, &s, sizeof s, hipMemcpyHostToDevice));
    return SDRX_OK;
}

int sdrx_chana_sync(sdrx_chana_t* b) { return b ? b->core.sync() : SDRX_EINVAL; }
int sdrx_chana_set_stream(sdrx_chana_t* b, void* hip_stream) { return Bank::set_stream(b, hip_stream); }
int sdrx_chana_get_stream(sdrx_chana_t* b, void** hip_stream) { return b ? b->core.get_stream(hip_stream) : SDRX_EINVAL; }
int sdrx_chana_set_timing(sdrx_chana_t* b, int enabled) { return b ? b->core.set_timing(enabled) : SDRX_EINVAL; }
int sdrx_chana_get_timing(sdrx_chana_t* b, double* total_ms, int64_t* feeds, int reset) { return b ? b->core.get_timing(total_ms, feeds, reset) : SDRX_EINVAL; }
int sdrx_chana_last_launch(const sdrx_chana_t* b, char* kernel_name, int name_cap, int* grid, int* block, int* lds_bytes) { return b ? b->core.last_launch(kernel_name, name_cap, grid, block, lds_bytes) : SDRX_EINVAL; }

} // extern "C"
