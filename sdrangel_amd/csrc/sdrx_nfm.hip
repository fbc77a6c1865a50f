// libsdrx.so: sdrx_nfm_* -- N narrowband-FM demodulators (NFMDemod::feed, plugins/channelrx/demodnfm/nfmdemod.cpp:140-332, with
// power or AF squelch) on one device: int16 I/Q at the channelizer's output rate in, mono qint16 audio out.  The
// front (NCO, Interpolator) is a channel back-end the handle owns and launches on its own stream; the tail's kernels are in
// nfm_kernels.hpp, those of CTCSS and the AF squelch (sdrx_nfm_create_ex) in nfm_tone_kernels.hpp.  Host side: the design products as
// the constructor / applySettings(settings, true) derive them (nfmdemod.cpp:80-91, 495-538), the two layouts and the launches;
// the rest is demod_bank.hpp's.
#include "sdrx_common.hpp"
#include "nfm_kernels.hpp"
#include "nfm_tone_kernels.hpp"
#include "demod_bank.hpp"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace sdrx;

constexpr int NFM_MAX_GATE = 1000;                  // 10 s: 2 * gate stays far inside an int at any audio rate

// what one channel is made from: sdrx_nfm_create fills `tone` with zeros
struct NfmCfgEx { sdrx_nfm_cfg base; sdrx_nfm_tone_cfg tone; };

struct NfmFamily : DemodDefaults {
    using Handle = sdrx_nfm;
    using Cfg = NfmCfgEx;
    using Chan = NfmChan;
    using Bufs = NfmBufs;
    static constexpr const char* name = "sdrx_nfm";
    static constexpr const float2* NfmBufs::* input = &NfmBufs::ci;
    static constexpr int bp_taps = NFM_TAB;                // Bandpass taps, Lowpass taps, Goertzel coefficients

    static int validate(int32_t n_ch, const NfmCfgEx* cfg)
    {
        if (n_ch <= 0 || !cfg) { set_error("sdrx_nfm_create: bad argument"); return SDRX_EINVAL; }
        for (int c = 0; c < n_ch; c++) {
            const sdrx_nfm_cfg& k = cfg[c].base;
            const sdrx_nfm_tone_cfg& t = cfg[c].tone;
            if (t.delta_squelch < 0 || t.delta_squelch > 1 || t.ctcss_on < 0 || t.ctcss_on > 1 || t.ctcss_index < 0 || t.ctcss_index > CT_TONES ||
                t.reserved != 0) {
                set_error("sdrx_nfm_create_ex: bad tone configuration (need delta_squelch 0|1, ctcss_on 0|1, 0 <= ctcss_index <= 32, reserved 0)");
                return SDRX_EINVAL;
            }

            if (k.in_rate <= 0 || k.audio_rate < 1000 || k.audio_rate > k.in_rate) {
                set_error("sdrx_nfm_create: bad channel configuration (need 1000 <= audio_rate <= in_rate; the interpolating branch is left out)");
                return SDRX_EINVAL;
            }
            if (!(k.rf_bandwidth > 0.0f) || !(k.rf_bandwidth <= 1.0e7f)) {
                set_error("sdrx_nfm_create: bad channel configuration (need 0 < rf_bandwidth <= 1e7)"); return SDRX_EINVAL;
            }
            if (!(k.af_bandwidth > 300.0f) || !(k.af_bandwidth <= 1.0e7f)) {
                set_error("sdrx_nfm_create: bad channel configuration (need 300 < af_bandwidth <= 1e7: the Bandpass starts at 300 Hz)"); return SDRX_EINVAL;
            }
            if (k.fm_deviation <= 0) { set_error("sdrx_nfm_create: bad channel configuration (need fm_deviation > 0)"); return SDRX_EINVAL; }
            if (k.squelch_gate < 0 || k.squelch_gate > NFM_MAX_GATE) {
                set_error("sdrx_nfm_create: bad channel configuration (need 0 <= squelch_gate <= 1000, in 10s of ms)"); return SDRX_EINVAL;
            }
            if (!std::isfinite(k.volume) || !std::isfinite(k.squelch)) {
                set_error("sdrx_nfm_create: bad channel configuration (volume and squelch must be finite)"); return SDRX_EINVAL;
            }
        }
        return SDRX_OK;
    }

    static void design(int c, const NfmCfgEx& kx, sdrx_backend_cfg& f, NfmChan& s, float* bp)
    {
        const sdrx_nfm_cfg& k = kx.base;
        f.in_rate = k.in_rate; f.nco_freq = k.nco_freq; f.out_rate = k.audio_rate;
        f.interp_cutoff = k.rf_bandwidth / 2.2f;            // m_interpolator.create(16, inputSampleRate, rfBandwidth / 2.2f)
        f.taps_per_phase = 4.5f;
        s.gate = (k.audio_rate / 100) * k.squelch_gate;     // gate is given in 10s of ms
        s.D = nfm_delay(s.gate);
        s.level = (float)std::pow(10.0, (double)k.squelch / 100.0);         // centi-Bels
        s.volume = k.volume;
        s.fm_scaling = (8.0f * (float)(uint32_t)k.audio_rate) / (float)k.fm_deviation;
        s.comp = (float)(uint32_t)k.audio_rate / 48000.0f; s.comp *= std::sqrt(s.comp);     // nfmdemod.cpp:82-83, sqrt of a Real
        s.mute = k.audio_mute ? 1 : 0;
        s.bp_off = c * bp_taps;
        // m_bandpass.create(301, audioSampleRate, 300.0, afBandwidth)
        demod_bandpass_design((double)k.audio_rate, 300.0, (double)k.af_bandwidth, bp);
        // m_lowpass.create(301, audioSampleRate, 250.0); m_ctcssDetector.setCoefficients(audioSampleRate / 16, audioSampleRate / 8.0f)
        ct_lowpass_design((double)k.audio_rate, 250.0, bp + NFM_TAB_LP);
        for (int j = 0; j < CT_TONES; j++) bp[NFM_TAB_COEF + j] = ct_coef(ct_tone_set()[j], ct_rate(k.audio_rate));
        s.ct_on = kx.tone.ctcss_on; s.ct_sel = kx.tone.ctcss_index;
        // m_afSquelch.setCoefficients(audioSampleRate / 2000, 600, audioSampleRate, 200, 0, {1000.0, 6000.0}); with m_deltaSquelch
        // applySettings sets m_squelchLevel = (-squelch) / 1000.0 and the detector's threshold to it
        s.af_on = kx.tone.delta_squelch;
        s.af_n = af_block_n(k.audio_rate); s.af_z = (int)((uint32_t)k.audio_rate / 10u);
        for (int j = 0; j < 2; j++) s.af_coef[j] = af_coef(af_tone(j, k.audio_rate), k.audio_rate);
        if (s.af_on) { s.level = af_level(k.squelch); s.af_thr = (double)s.level; }
        s.ct_n = ct_block_n(k.audio_rate);
    }

    // one history set: [32 magsq | D delay-line writes | 300 Bandpass inputs | with CTCSS: 300 Lowpass inputs].  A fresh one is all zeros: moving average empty
    // (the power before the stream counts as 0), delay line and Bandpass ring 0 (the delay line too: DoubleBufferFIFO does not
    // clear its array, see sdrx.h)
    static void hist(HistCarver& k, const NfmChan& s, NfmBufs& u)
    {
        k.pair(u.mhist, u.mhist_next, NFM_MA);
        k.pair(u.whist, u.whist_next, (size_t)s.D);
        k.pair(u.xhist, u.xhist_next, AM_BP_HIST);
        if (s.ct_on) k.pair(u.lhist, u.lhist_next, CT_LP_HIST);
        if (s.af_on) { k.pair(u.dl, u.dl_next, 2 * (size_t)NFM_DL); k.pair(u.afh, u.afh_next, 2 * (size_t)AF_MA); }
    }

    static void work(Carver& k, size_t n, const NfmChan& s, NfmBufs& u)
    {
        const size_t nblk = n / 256 + 1;
        u.msq = k.take<float>(n); u.wraw = k.take<float>(n); u.w = k.take<float>(n);
        u.x = k.take<float>(n); u.aidx = k.take<int>(n);
        u.dterm = k.take<double>(n); u.tot = k.take<double>(n);
        u.audio = k.take<int16_t>(n);
        u.blk_sum = k.take<double>(nblk); u.blk_peak = k.take<float>(nblk);
        u.blk_a = k.take<int>(nblk);
        if (!s.ct_on) return;
        // one sample in eight goes to the detector; a detector block is at least 1000 / 16 of those
        const size_t ndet = n / 8 + 16;
        u.aidx_a = k.take<int>(n); u.xl = k.take<float>(n); u.xa = k.take<float>(n); u.ctl = k.take<float>(n);
        u.ev = k.take<int>(n); u.ev_at = k.take<int>(n); u.ev_idx = k.take<int>(n);
        u.cs = k.take<float>(ndet); u.cpos = k.take<int>(ndet); u.cblk = k.take<int>(nblk + 4);
    }

    static int64_t outputs_bound(const NfmCfgEx& k, int64_t n_in) { return demod_outputs_bound(k.base.in_rate / k.base.audio_rate, n_in); }

    static int launch(DemodBank<NfmFamily>& b, unsigned nc, unsigned gx)
    {
        const unsigned gp = (nc + PS_CH - 1) / PS_CH;
        hipLaunchKernelGGL(nfm_level_kernel, dim3(gx, nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
        SDRX_HIP(hipGetLastError());
        hipLaunchKernelGGL(nfm_psum_kernel, dim3(gp), dim3(64), 0, b.core.stream, b.d_chan, b.d_bufs, b.n_ch);
        SDRX_HIP(hipGetLastError());
        hipLaunchKernelGGL(nfm_gate_kernel, dim3(nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
        SDRX_HIP(hipGetLastError());
        if (std::any_of(b.cfg.begin(), b.cfg.end(), [](const NfmCfgEx& k) { return k.tone.delta_squelch != 0; })) {
            hipLaunchKernelGGL(nfm_af_walk_kernel, dim3((nc + 63) / 64), dim3(64), 0, b.core.stream, b.d_chan, b.d_bufs, b.n_ch);
            SDRX_HIP(hipGetLastError());
        }
        if (std::any_of(b.cfg.begin(), b.cfg.end(), [](const NfmCfgEx& k) { return k.tone.ctcss_on != 0; })) {
            hipLaunchKernelGGL(nfm_ct_pack_kernel, dim3(gx, nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
            SDRX_HIP(hipGetLastError());
            hipLaunchKernelGGL(nfm_ct_lowpass_kernel, dim3(gx, nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs, b.d_bp);
            SDRX_HIP(hipGetLastError());
            hipLaunchKernelGGL(nfm_ct_detect_kernel, dim3(nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs, b.d_bp);
            SDRX_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(nfm_out_kernel, dim3(gx, nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs, b.d_bp);
        SDRX_HIP(hipGetLastError());
        b.core.note_launch("nfm_out_kernel", (int)(gx * nc), 256, (int)((AM_BP_H + 1 + NFM_OUT_WIN) * sizeof(float)));
        hipLaunchKernelGGL(nfm_carry_kernel, dim3(nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
        SDRX_HIP(hipGetLastError());
        return SDRX_OK;
    }

    static double magsq(const NfmChan& s) { return s.total / (double)NFM_MA; }      // m_movingAverage.asDouble()
};

struct sdrx_nfm : DemodBank<NfmFamily> {};
using Bank = DemodBank<NfmFamily>;

extern "C" {

int sdrx_nfm_create_ex(sdrx_nfm_t** out, int device, int32_t n_ch, const sdrx_nfm_cfg* cfg, const sdrx_nfm_tone_cfg* tone)
{
    if (out) *out = nullptr;
    std::vector<NfmCfgEx> both;
    if (n_ch > 0 && cfg) {
        both.resize((size_t)n_ch);                              // value-initialised: tone all zero
        for (int c = 0; c < n_ch; c++) { both[(size_t)c].base = cfg[c]; if (tone) both[(size_t)c].tone = tone[c]; }
    }
    return Bank::create(out, device, n_ch, both.empty() ? nullptr : both.data());
}
int sdrx_nfm_create(sdrx_nfm_t** out, int device, int32_t n_ch, const sdrx_nfm_cfg* cfg) { return sdrx_nfm_create_ex(out, device, n_ch, cfg, nullptr); }
int sdrx_nfm_destroy(sdrx_nfm_t* b) { return Bank::destroy(b); }
int sdrx_nfm_reset(sdrx_nfm_t* b) { return Bank::reset(b); }
int sdrx_nfm_feed_dev(sdrx_nfm_t* b, const int16_t* const* d_iq, const int64_t* n_per_ch) { return Bank::feed_dev(b, d_iq, n_per_ch); }
int sdrx_nfm_feed_bank(sdrx_nfm_t* b, sdrx_chan_bank_t* bank) { return Bank::feed_bank(b, bank); }
int sdrx_nfm_feed(sdrx_nfm_t* b, const int16_t* const* iq, const int64_t* n_per_ch) { return Bank::feed(b, iq, n_per_ch); }
int64_t sdrx_nfm_read(sdrx_nfm_t* b, int32_t c, int16_t* audio, int64_t cap) { return Bank::read(b, "read", c, audio, cap, &NfmBufs::audio, &NfmChan::n, 2); }
int sdrx_nfm_last_dev(sdrx_nfm_t* b, int32_t c, const int16_t** d_audio, int64_t* n) { return Bank::last_dev(b, "last_dev", c, d_audio, n, &NfmBufs::audio, &NfmChan::n); }
int sdrx_nfm_squelch_open(sdrx_nfm_t* b, int32_t c) { return Bank::flag(b, "squelch_open", c, &NfmChan::sq_open); }
int sdrx_nfm_levels(sdrx_nfm_t* b, int32_t c, double* magsq, double* sum, double* peak, int64_t* count, int reset) { return Bank::levels(b, c, magsq, sum, peak, count, reset); }

int sdrx_nfm_get_design(sdrx_nfm_t* b, int32_t c, int32_t* ntaps_per_phase, float* taps, int32_t taps_cap,
                        float* bandpass_taps, int32_t* nco_inc, float* squelch_level, int32_t* squelch_gate)
{
    if (!Bank::in_range(b, c)) return Bank::fail("get_design", ": bad channel");
    int rc = sdrx_backend_get_design(b->front, c, ntaps_per_phase, taps_cap > 0 ? taps : nullptr, taps_cap, nullptr, nco_inc); if (rc) return rc;
    if (bandpass_taps) std::memcpy(bandpass_taps, &b->bp_all[(size_t)b->h_chan[(size_t)c].bp_off], (AM_BP_H + 1) * 4);
    if (squelch_level) *squelch_level = b->h_chan[(size_t)c].level;
    if (squelch_gate) *squelch_gate = b->h_chan[(size_t)c].gate;
    return SDRX_OK;
}

int sdrx_nfm_ctcss(sdrx_nfm_t* b, int32_t c, int32_t* index, float* tone_hz, int64_t* n_changes)
{
    NfmChan s;
    int rc = Bank::fetch(b, "ctcss", c, &s); if (rc) return rc;
    if (index) *index = s.ct_index;
    if (tone_hz) *tone_hz = s.ct_index > 0 ? ct_tone_set()[s.ct_index - 1] : 0.0f;
    if (n_changes) *n_changes = s.ct_changes;
    return SDRX_OK;
}

int64_t sdrx_nfm_ctcss_events(sdrx_nfm_t* b, int32_t c, int64_t* at, int32_t* index, int64_t cap)
{
    if (cap < 0 || (cap > 0 && (!at || !index))) return Bank::fail("ctcss_events", ": bad argument");
    NfmChan s;
    int rc = Bank::fetch(b, "ctcss_events", c, &s); if (rc) return rc;
    const int64_t n = std::min<int64_t>(s.n_ev, cap);
    if (n > 0) {
        std::vector<int> pos((size_t)n);
        SDRX_HIP(hipMemcpy(pos.data(), b->h_bufs[c].ev_at, (size_t)n * 4, hipMemcpyDeviceToHost));
        SDRX_HIP(hipMemcpy(index, b->h_bufs[c].ev_idx, (size_t)n * 4, hipMemcpyDeviceToHost));
        std::copy(pos.begin(), pos.end(), at);
    }
    return s.n_ev;
}

int sdrx_nfm_ctcss_powers(sdrx_nfm_t* b, int32_t c, float* power32, int32_t* detected, int32_t* max_index, int64_t* n_blocks)
{
    NfmChan s;
    int rc = Bank::fetch(b, "ctcss_powers", c, &s); if (rc) return rc;
    if (power32) std::memcpy(power32, s.ct_power, sizeof s.ct_power);
    if (detected) *detected = s.ct_detected;
    if (max_index) *max_index = s.ct_max_index;
    if (n_blocks) *n_blocks = s.ct_blocks;
    return SDRX_OK;
}

// a channel without m_deltaSquelch never calls its AFSquelch: the state stays the one setCoefficients left, all zero
int sdrx_nfm_af_squelch(sdrx_nfm_t* b, int32_t c, int32_t* open, double* sums2, int32_t* count)
{
    NfmChan s;
    int rc = Bank::fetch(b, "af_squelch", c, &s); if (rc) return rc;
    if (open) *open = s.af.af_open;
    if (sums2) { sums2[0] = s.af.sum[0]; sums2[1] = s.af.sum[1]; }
    if (count) *count = s.af.count;
    return SDRX_OK;
}

int sdrx_nfm_get_tone_design(sdrx_nfm_t* b, int32_t c, int32_t* ctcss_n, int32_t* ctcss_rate, float* coef32, float* lowpass_taps,
                             int32_t* af_n, double* af_tones2, double* af_coef2, double* af_threshold)
{
    if (!Bank::in_range(b, c)) return Bank::fail("get_tone_design", ": bad channel");
    const int rate = b->cfg[(size_t)c].base.audio_rate;
    if (af_n) *af_n = af_block_n(rate);
    for (int j = 0; j < 2; j++) {
        if (af_tones2) af_tones2[j] = af_tone(j, rate);
        if (af_coef2) af_coef2[j] = af_coef(af_tone(j, rate), rate);
    }
    if (af_threshold) *af_threshold = b->h_chan[(size_t)c].af_thr;
    const float* row = &b->bp_all[(size_t)b->h_chan[(size_t)c].bp_off];
    if (ctcss_n) *ctcss_n = b->h_chan[(size_t)c].ct_n;
    if (ctcss_rate) *ctcss_rate = ct_rate(b->cfg[(size_t)c].base.audio_rate);
    if (coef32) std::memcpy(coef32, row + NFM_TAB_COEF, CT_TONES * 4);
    if (lowpass_taps) std::memcpy(lowpass_taps, row + NFM_TAB_LP, (CT_LP_H + 1) * 4);
    return SDRX_OK;
}

int sdrx_nfm_sync(sdrx_nfm_t* b) { return b ? b->core.sync() : SDRX_EINVAL; }
int sdrx_nfm_set_stream(sdrx_nfm_t* b, void* hip_stream) { return Bank::set_stream(b, hip_stream); }
int sdrx_nfm_get_stream(sdrx_nfm_t* b, void** hip_stream) { return b ? b->core.get_stream(hip_stream) : SDRX_EINVAL; }
int sdrx_nfm_set_timing(sdrx_nfm_t* b, int enabled) { return b ? b->core.set_timing(enabled) : SDRX_EINVAL; }
int sdrx_nfm_get_timing(sdrx_nfm_t* b, double* total_ms, int64_t* feeds, int reset) { return b ? b->core.get_timing(total_ms, feeds, reset) : SDRX_EINVAL; }
int sdrx_nfm_last_launch(const sdrx_nfm_t* b, char* kernel_name, int name_cap, int* grid, int* block, int* lds_bytes) { return b ? b->core.last_launch(kernel_name, name_cap, grid, block, lds_bytes) : SDRX_EINVAL; }

} // extern "C"
