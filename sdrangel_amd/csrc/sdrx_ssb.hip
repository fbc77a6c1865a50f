// libsdrx.so: sdrx_ssb_* -- N SSB / DSB demodulators (SSBDemod::feed, plugins/channelrx/demodssb/ssbdemod.cpp:147-285) on one
// device: int16 I/Q at the channelizer's output rate in, qint16 l,r audio and the decimated sideband stream of the spectrum
// sink out.  The front (NCO, Interpolator, fftfilt runSSB / runDSB) is a channel back-end the handle owns and launches on its
// own stream; the tail's kernels are in ssb_kernels.hpp.  Host side: the design products as the constructor,
// applyAudioSampleRate and applySettings(settings, true) derive them (ssbdemod.cpp:46-101, 401-422, 457-533), the two
// layouts and the launches; the rest is demod_bank.hpp's.
#include "sdrx_common.hpp"
#include "ssb_kernels.hpp"
#include "demod_bank.hpp"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace sdrx;

namespace {
constexpr int SSB_BLOCK_MAX = 1024;                 // runDSB hands out 1024 samples at a time, runSSB 512

struct SsbDerived { float band, low; bool usb; int hn, gate; };

// band and cutoff as applySettings derives them (ssbdemod.cpp:457-489); hn and gate as :502-505
SsbDerived derive(const sdrx_ssb_cfg& k)
{
    SsbDerived d;
    d.band = k.rf_bandwidth; d.low = k.low_cutoff; d.usb = true;
    if (d.band < 0) { d.band = -d.band; d.low = -d.low; d.usb = false; }
    if (d.band < 100.0f) { d.band = 100.0f; d.low = 0; }
    d.hn = (k.audio_rate / 1000) * (1 << k.agc_time_log2);
    d.gate = (k.audio_rate / 1000) * k.agc_threshold_gate;
    return d;
}

} // namespace

struct SsbFamily : DemodDefaults {
    using Handle = sdrx_ssb;
    using Cfg = sdrx_ssb_cfg;
    using Chan = SsbChan;
    using Bufs = SsbBufs;
    static constexpr const char* name = "sdrx_ssb";
    static constexpr const float2* SsbBufs::* input = &SsbBufs::s;
    // at most one resampler output per input (step >= 1) plus what the filter held back: fewer than one block
    static constexpr int work_extra = SSB_BLOCK_MAX;

    static int validate(int32_t n_ch, const sdrx_ssb_cfg* cfg)
    {
        if (n_ch <= 0 || !cfg) { set_error("sdrx_ssb_create: bad argument"); return SDRX_EINVAL; }
        for (int c = 0; c < n_ch; c++) {
            const sdrx_ssb_cfg& k = cfg[c];
            // 192000 keeps audio_rate / 1000 below 375, so hn == 12000 (where resize() is skipped and the constructor's MagAGC,
            // history filled with R and step length 2400, would be the object) cannot be asked for
            if (k.in_rate <= 0 || k.audio_rate < 1000 || k.audio_rate > 192000 || k.audio_rate > k.in_rate) {
                set_error("sdrx_ssb_create: bad channel configuration (need 1000 <= audio_rate <= 192000 and audio_rate <= in_rate; the interpolating branch is left out)");
                return SDRX_EINVAL;
            }
            if (!std::isfinite(k.rf_bandwidth) || !(std::fabs(k.rf_bandwidth) <= 1.0e7f) || !std::isfinite(k.low_cutoff) || !(std::fabs(k.low_cutoff) <= 1.0e7f)) {
                set_error("sdrx_ssb_create: bad channel configuration (need |rf_bandwidth| <= 1e7 and |low_cutoff| <= 1e7)"); return SDRX_EINVAL;
            }
            if (!std::isfinite(k.volume)) { set_error("sdrx_ssb_create: bad channel configuration (volume must be finite)"); return SDRX_EINVAL; }
            if (k.span_log2 < 1 || k.span_log2 > 8) {
                set_error("sdrx_ssb_create: bad channel configuration (need 1 <= span_log2 <= 8: decim_mask is an unsigned char)"); return SDRX_EINVAL;
            }
            if (k.agc_time_log2 < 0 || k.agc_time_log2 > 17) { set_error("sdrx_ssb_create: bad channel configuration (need 0 <= agc_time_log2 <= 17)"); return SDRX_EINVAL; }
            const int64_t hn = (int64_t)(k.audio_rate / 1000) << k.agc_time_log2;
            if (hn < 2 || hn > SSB_MAX_HN) {
                set_error("sdrx_ssb_create: bad channel configuration (need 2 <= (audio_rate / 1000) << agc_time_log2 <= 131072)"); return SDRX_EINVAL;
            }
            if (k.agc_threshold_gate < 0 || k.agc_threshold_gate > 10000) {
                set_error("sdrx_ssb_create: bad channel configuration (need 0 <= agc_threshold_gate <= 10000, in ms)"); return SDRX_EINVAL;
            }
            if (k.agc_power_threshold < -300 || k.agc_power_threshold > 300) {
                set_error("sdrx_ssb_create: bad channel configuration (need -300 <= agc_power_threshold <= 300, in dB)"); return SDRX_EINVAL;
            }
        }
        return SDRX_OK;
    }

    static void design(int, const sdrx_ssb_cfg& k, sdrx_backend_cfg& f, SsbChan& s, float*)
    {
        const SsbDerived d = derive(k);
        f.in_rate = k.in_rate; f.nco_freq = k.nco_freq; f.out_rate = k.audio_rate;
        f.interp_cutoff = d.band * 1.5f;                    // m_interpolator.create(16, m_inputSampleRate, m_Bandwidth * 1.5f, 2.0f)
        f.taps_per_phase = 2.0f;
        f.filt_mode = k.dsb ? 4 : (d.usb ? 2 : 3);
        f.f1 = d.low / (float)(uint32_t)k.audio_rate;      // create_filter(m_LowCutoff / (float) rate, m_Bandwidth / (float) rate)
        f.f2 = k.dsb ? (2.0f * d.band) / (float)(uint32_t)k.audio_rate : d.band / (float)(uint32_t)k.audio_rate;
        s.hn = d.hn; s.D = ssb_delay(d.hn); s.gate = d.gate;
        s.decim = 1 << (k.span_log2 - 1);
        s.agc = k.agc ? 1 : 0;
        s.thr_enable = k.agc_power_threshold != 100 ? 1 : 0;    // != -m_minPowerThresholdDB, which is -100 in the 16-bit build
        s.clamping = k.agc_clamping ? 1 : 0;
        s.mute = k.audio_mute ? 1 : 0; s.binaural = k.audio_binaural ? 1 : 0; s.flip = k.audio_flip ? 1 : 0;
        s.swap_iq = (!k.dsb && !d.usb) ? 1 : 0;
        s.volume = (float)((double)k.volume / 4.0);
        s.threshold = std::pow(10.0, (double)k.agc_power_threshold / 10.0) * (32768.0 * 32768.0);
        s.step_delta = 1.0 / (double)(d.hn / 2);
        s.U = 0; s.Dn = d.hn / 2;                           // resize(): m_stepUpCounter = 0, m_stepDownCounter = m_stepLength
        s.u0 = 1.0;
    }

    // one history set: [hn powers | D + 1 delay-line writes].  A fresh one is all zeros: moving-average history 0 (resize()
    // then fill(0)); delay line 0 (DoubleBufferFIFO does not clear its array, see sdrx.h)
    static void hist(HistCarver& k, const SsbChan& s, SsbBufs& u)
    {
        k.pair(u.phist, u.phist_next, (size_t)s.hn);
        k.pair(u.whist, u.whist_next, (size_t)(s.D + 1));
    }

    static void work(Carver& k, size_t n, const SsbChan&, SsbBufs& u)
    {
        const size_t nblk = n / 256 + 1;
        u.pw = k.take<float>(n); u.sv = k.take<float>(n);
        u.dterm = k.take<double>(n); u.tot = k.take<double>(n);
        u.w = k.take<float2>(n);
        u.audio = k.take<int16_t>(2 * n); u.spec = k.take<int16_t>(2 * n);
        u.blk_sum = k.take<double>(nblk); u.blk_peak = k.take<double>(nblk);
    }

    // the resampler's outputs, and the filter adds what it held back
    static int64_t outputs_bound(const sdrx_ssb_cfg& k, int64_t n_in) { return demod_outputs_bound(k.in_rate / k.audio_rate, n_in) + SSB_BLOCK_MAX; }

    static int launch(DemodBank<SsbFamily>& b, unsigned nc, unsigned gx)
    {
        const unsigned gp = (nc + PS_CH - 1) / PS_CH;
        hipLaunchKernelGGL(ssb_level_kernel, dim3(gx, nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
        SDRX_HIP(hipGetLastError());
        hipLaunchKernelGGL(ssb_psum_kernel, dim3(gp), dim3(64), 0, b.core.stream, b.d_chan, b.d_bufs, b.n_ch);
        SDRX_HIP(hipGetLastError());
        hipLaunchKernelGGL(ssb_gate_kernel, dim3(nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
        SDRX_HIP(hipGetLastError());
        hipLaunchKernelGGL(ssb_out_kernel, dim3(gx, nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
        SDRX_HIP(hipGetLastError());
        b.core.note_launch("ssb_out_kernel", (int)(gx * nc), 256, 0);
        hipLaunchKernelGGL(ssb_carry_kernel, dim3(nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
        SDRX_HIP(hipGetLastError());
        return SDRX_OK;
    }

    static double magsq(const SsbChan& s) { return s.magsq; }
};

struct sdrx_ssb : DemodBank<SsbFamily> {};
using Bank = DemodBank<SsbFamily>;

extern "C" {

int sdrx_ssb_create(sdrx_ssb_t** out, int device, int32_t n_ch, const sdrx_ssb_cfg* cfg) { return Bank::create(out, device, n_ch, cfg); }
int sdrx_ssb_destroy(sdrx_ssb_t* b) { return Bank::destroy(b); }
int sdrx_ssb_reset(sdrx_ssb_t* b) { return Bank::reset(b); }
int sdrx_ssb_feed_dev(sdrx_ssb_t* b, const int16_t* const* d_iq, const int64_t* n_per_ch) { return Bank::feed_dev(b, d_iq, n_per_ch); }
int sdrx_ssb_feed_bank(sdrx_ssb_t* b, sdrx_chan_bank_t* bank) { return Bank::feed_bank(b, bank); }
int sdrx_ssb_feed(sdrx_ssb_t* b, const int16_t* const* iq, const int64_t* n_per_ch) { return Bank::feed(b, iq, n_per_ch); }
int64_t sdrx_ssb_read(sdrx_ssb_t* b, int32_t c, int16_t* audio_lr, int64_t cap) { return Bank::read(b, "read", c, audio_lr, cap, &SsbBufs::audio, &SsbChan::n, 4); }
int sdrx_ssb_last_dev(sdrx_ssb_t* b, int32_t c, const int16_t** d_audio_lr, int64_t* n) { return Bank::last_dev(b, "last_dev", c, d_audio_lr, n, &SsbBufs::audio, &SsbChan::n); }
int64_t sdrx_ssb_read_spectrum(sdrx_ssb_t* b, int32_t c, int16_t* samples_iq, int64_t cap) { return Bank::read(b, "read_spectrum", c, samples_iq, cap, &SsbBufs::spec, &SsbChan::n_spec, 4); }
int sdrx_ssb_spectrum_last_dev(sdrx_ssb_t* b, int32_t c, const int16_t** d_samples_iq, int64_t* n) { return Bank::last_dev(b, "spectrum_last_dev", c, d_samples_iq, n, &SsbBufs::spec, &SsbChan::n_spec); }
int sdrx_ssb_audio_active(sdrx_ssb_t* b, int32_t c) { return Bank::flag(b, "audio_active", c, &SsbChan::audio_active); }
int sdrx_ssb_levels(sdrx_ssb_t* b, int32_t c, double* magsq, double* sum, double* peak, int64_t* count, int reset) { return Bank::levels(b, c, magsq, sum, peak, count, reset); }

int sdrx_ssb_get_design(sdrx_ssb_t* b, int32_t c, int32_t* ntaps_per_phase, float* taps, int32_t taps_cap, float* filter_iq,
                        int32_t* nco_inc, int32_t* agc_nb_samples, int32_t* agc_gate, double* agc_threshold, float* volume)
{
    if (!Bank::in_range(b, c)) return Bank::fail("get_design", ": bad channel");
    int rc = sdrx_backend_get_design(b->front, c, ntaps_per_phase, taps_cap > 0 ? taps : nullptr, taps_cap, filter_iq, nco_inc); if (rc) return rc;
    const SsbChan& s = b->h_chan[(size_t)c];
    if (agc_nb_samples) *agc_nb_samples = s.hn;
    if (agc_gate) *agc_gate = s.gate;
    if (agc_threshold) *agc_threshold = s.threshold;
    if (volume) *volume = s.volume;
    return SDRX_OK;
}

int sdrx_ssb_sync(sdrx_ssb_t* b) { return b ? b->core.sync() : SDRX_EINVAL; }
int sdrx_ssb_set_stream(sdrx_ssb_t* b, void* hip_stream) { return Bank::set_stream(b, hip_stream); }
int sdrx_ssb_get_stream(sdrx_ssb_t* b, void** hip_stream) { return b ? b->core.get_stream(hip_stream) : SDRX_EINVAL; }
int sdrx_ssb_set_timing(sdrx_ssb_t* b, int enabled) { return b ? b->core.set_timing(enabled) : SDRX_EINVAL; }
int sdrx_ssb_get_timing(sdrx_ssb_t* b, double* total_ms, int64_t* feeds, int reset) { return b ? b->core.get_timing(total_ms, feeds, reset) : SDRX_EINVAL; }
int sdrx_ssb_last_launch(const sdrx_ssb_t* b, char* kernel_name, int name_cap, int* grid, int* block, int* lds_bytes) { return b ? b->core.last_launch(kernel_name, name_cap, grid, block, lds_bytes) : SDRX_EINVAL; }

} // extern "C"
