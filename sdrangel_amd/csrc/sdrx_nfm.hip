// libsdrx.so: sdrx_nfm_* -- N narrowband-FM demodulators (NFMDemod::feed, plugins/channelrx/demodnfm/nfmdemod.cpp:140-332, with
// m_deltaSquelch and m_ctcssOn off) on one device: int16 I/Q at the channelizer's output rate in, mono qint16 audio out.  The
// front (NCO, Interpolator) is a channel back-end the handle owns and launches on its own stream; the tail's kernels are in
// nfm_kernels.hpp.  Host side: the design products as the constructor / applySettings(settings, true) derive them
// (nfmdemod.cpp:80-91, 495-538), the two layouts and the launches; the rest is demod_bank.hpp's.
#include "sdrx_common.hpp"
#include "nfm_kernels.hpp"
#include "demod_bank.hpp"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace sdrx;

constexpr int NFM_MAX_GATE = 1000;                  // 10 s: 2 * gate stays far inside an int at any audio rate

struct NfmFamily : DemodDefaults {
    using Handle = sdrx_nfm;
    using Cfg = sdrx_nfm_cfg;
    using Chan = NfmChan;
    using Bufs = NfmBufs;
    static constexpr const char* name = "sdrx_nfm";
    static constexpr const float2* NfmBufs::* input = &NfmBufs::ci;
    static constexpr int bp_taps = AM_BP_H + 1;

    static int validate(int32_t n_ch, const sdrx_nfm_cfg* cfg)
    {
        if (n_ch <= 0 || !cfg) { set_error("sdrx_nfm_create: bad argument"); return SDRX_EINVAL; }
        for (int c = 0; c < n_ch; c++) {
            const sdrx_nfm_cfg& k = cfg[c];
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

    static void design(int c, const sdrx_nfm_cfg& k, sdrx_backend_cfg& f, NfmChan& s, float* bp)
    {
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
    }

    // one history set: [32 magsq | D delay-line writes | 300 Bandpass inputs].  A fresh one is all zeros: moving average empty
    // (the power before the stream counts as 0), delay line and Bandpass ring 0 (the delay line too: DoubleBufferFIFO does not
    // clear its array, see sdrx.h)
    static void hist(HistCarver& k, const NfmChan& s, NfmBufs& u)
    {
        k.pair(u.mhist, u.mhist_next, NFM_MA);
        k.pair(u.whist, u.whist_next, (size_t)s.D);
        k.pair(u.xhist, u.xhist_next, AM_BP_HIST);
    }

    static void work(Carver& k, size_t n, NfmBufs& u)
    {
        const size_t nblk = n / 256 + 1;
        u.msq = k.take<float>(n); u.wraw = k.take<float>(n); u.w = k.take<float>(n);
        u.x = k.take<float>(n); u.aidx = k.take<int>(n);
        u.dterm = k.take<double>(n); u.tot = k.take<double>(n);
        u.audio = k.take<int16_t>(n);
        u.blk_sum = k.take<double>(nblk); u.blk_peak = k.take<float>(nblk);
        u.blk_a = k.take<int>(nblk);
    }

    static int64_t outputs_bound(const sdrx_nfm_cfg& k, int64_t n_in) { return demod_outputs_bound(k.in_rate / k.audio_rate, n_in); }

    static int launch(DemodBank<NfmFamily>& b, unsigned nc, unsigned gx)
    {
        const unsigned gp = (nc + PS_CH - 1) / PS_CH;
        hipLaunchKernelGGL(nfm_level_kernel, dim3(gx, nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
        SDRX_HIP(hipGetLastError());
        hipLaunchKernelGGL(nfm_psum_kernel, dim3(gp), dim3(64), 0, b.core.stream, b.d_chan, b.d_bufs, b.n_ch);
        SDRX_HIP(hipGetLastError());
        hipLaunchKernelGGL(nfm_gate_kernel, dim3(nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
        SDRX_HIP(hipGetLastError());
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

int sdrx_nfm_create(sdrx_nfm_t** out, int device, int32_t n_ch, const sdrx_nfm_cfg* cfg) { return Bank::create(out, device, n_ch, cfg); }
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

int sdrx_nfm_sync(sdrx_nfm_t* b) { return b ? b->core.sync() : SDRX_EINVAL; }
int sdrx_nfm_set_stream(sdrx_nfm_t* b, void* hip_stream) { return Bank::set_stream(b, hip_stream); }
int sdrx_nfm_get_stream(sdrx_nfm_t* b, void** hip_stream) { return b ? b->core.get_stream(hip_stream) : SDRX_EINVAL; }
int sdrx_nfm_set_timing(sdrx_nfm_t* b, int enabled) { return b ? b->core.set_timing(enabled) : SDRX_EINVAL; }
int sdrx_nfm_get_timing(sdrx_nfm_t* b, double* total_ms, int64_t* feeds, int reset) { return b ? b->core.get_timing(total_ms, feeds, reset) : SDRX_EINVAL; }
int sdrx_nfm_last_launch(const sdrx_nfm_t* b, char* kernel_name, int name_cap, int* grid, int* block, int* lds_bytes) { return b ? b->core.last_launch(kernel_name, name_cap, grid, block, lds_bytes) : SDRX_EINVAL; }

} // extern "C"
