// libsdrx.so: sdrx_am_* -- N AM demodulators (AMDemod::feed / processOneSample in envelope mode,
// plugins/channelrx/demodam/amdemod.cpp:101-276) on one device: int16 I/Q at the channelizer's output rate in, mono qint16
// audio out.  The front (NCO, Interpolator) is a channel back-end the handle owns and launches on its own stream; the tail's
// kernels are in am_kernels.hpp.  Host side: the design products as applyChannelSettings / applyAudioSampleRate /
// applySettings derive them (amdemod.cpp:360-475), the two layouts and the launches; the rest is demod_bank.hpp's.
#include "sdrx_common.hpp"
#include "am_kernels.hpp"
#include "demod_bank.hpp"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace sdrx;

struct AmFamily : DemodDefaults {
    using Handle = sdrx_am;
    using Cfg = sdrx_am_cfg;
    using Chan = AmChan;
    using Bufs = AmBufs;
    static constexpr const char* name = "sdrx_am";
    static constexpr const float2* AmBufs::* input = &AmBufs::ci;
    static constexpr int bp_taps = AM_BP_H + 1;

    static int validate(int32_t n_ch, const sdrx_am_cfg* cfg)
    {
        if (n_ch <= 0 || !cfg) { set_error("sdrx_am_create: bad argument"); return SDRX_EINVAL; }
        for (int c = 0; c < n_ch; c++) {
            const sdrx_am_cfg& k = cfg[c];
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

    static void design(int c, const sdrx_am_cfg& k, sdrx_backend_cfg& f, AmChan& s, float* bp)
    {
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
    }

    // one history set: [16 magsq | D roots | H fed values | 300 demods]
    static void hist(HistCarver& k, const AmChan& s, AmBufs& u)
    {
        k.pair(u.mhist, u.mhist_next, AM_MA);
        k.pair(u.rhist, u.rhist_next, (size_t)s.D);
        k.pair(u.vhist, u.vhist_next, (size_t)s.H);
        k.pair(u.dhist, u.dhist_next, AM_BP_HIST);
    }

    // MovingAverage<double>(rate / 10, 0.003): every entry (double) 0.003f; everything else starts at 0 (the delay line too:
    // DoubleBufferFIFO does not clear its array, see sdrx.h)
    static void fresh(const AmChan& s, AmBufs& u) { for (int i = 0; i < s.H; i++) u.vhist_next[i] = am_agc_initial(); }

    static void work(Carver& k, size_t n, const AmChan&, AmBufs& u)
    {
        const size_t nblk = n / 256 + 1;
        u.msq = k.take<float>(n); u.root = k.take<float>(n);
        u.cnt = k.take<int>(n); u.aidx = k.take<int>(n); u.fcnt = k.take<int>(n);
        u.dterm = k.take<double>(n); u.tot = k.take<double>(n);
        u.vnew = k.take<double>(n); u.uterm = k.take<double>(n); u.agc = k.take<double>(n);
        u.dem = k.take<float>(n);
        u.audio = k.take<int16_t>(n);
        u.blk_sum = k.take<double>(nblk); u.blk_peak = k.take<float>(nblk);
    }

    static int64_t outputs_bound(const sdrx_am_cfg& k, int64_t n_in) { return demod_outputs_bound(k.in_rate / k.audio_rate, n_in); }

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
        hipLaunchKernelGGL(am_out_kernel, dim3(gx, nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs, b.d_bp);
        SDRX_HIP(hipGetLastError());
        b.core.note_launch("am_out_kernel", (int)(gx * nc), 256, (int)((AM_BP_H + 1) * sizeof(float)));
        hipLaunchKernelGGL(am_carry_kernel, dim3(nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
        SDRX_HIP(hipGetLastError());
        return SDRX_OK;
    }

    static double magsq(const AmChan& s) { return s.magsq; }
};

struct sdrx_am : DemodBank<AmFamily> {};
using Bank = DemodBank<AmFamily>;

extern "C" {

int sdrx_am_create(sdrx_am_t** out, int device, int32_t n_ch, const sdrx_am_cfg* cfg) { return Bank::create(out, device, n_ch, cfg); }
int sdrx_am_destroy(sdrx_am_t* b) { return Bank::destroy(b); }
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

int sdrx_am_sync(sdrx_am_t* b) { return b ? b->core.sync() : SDRX_EINVAL; }
int sdrx_am_set_stream(sdrx_am_t* b, void* hip_stream) { return Bank::set_stream(b, hip_stream); }
int sdrx_am_get_stream(sdrx_am_t* b, void** hip_stream) { return b ? b->core.get_stream(hip_stream) : SDRX_EINVAL; }
int sdrx_am_set_timing(sdrx_am_t* b, int enabled) { return b ? b->core.set_timing(enabled) : SDRX_EINVAL; }
int sdrx_am_get_timing(sdrx_am_t* b, double* total_ms, int64_t* feeds, int reset) { return b ? b->core.get_timing(total_ms, feeds, reset) : SDRX_EINVAL; }
int sdrx_am_last_launch(const sdrx_am_t* b, char* kernel_name, int name_cap, int* grid, int* block, int* lds_bytes) { return b ? b->core.last_launch(kernel_name, name_cap, grid, block, lds_bytes) : SDRX_EINVAL; }

} // extern "C"
