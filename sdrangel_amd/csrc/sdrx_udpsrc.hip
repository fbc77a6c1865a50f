// libsdrx.so: sdrx_udpsrc_* -- N UDPSrc channels (UDPSrc::feed, plugins/channelrx/udpsrc/udpsrc.cpp:136-321) on one device:
// int16 I/Q at the channelizer's output rate in, the samples UDPSrc hands to its UDPSink (the datagram payload) out.  The
// front (NCO, Interpolator) is a channel back-end the handle owns and launches on its own stream, started one distance step
// in as UDPSrc starts it; the tail's kernels are in udpsrc_kernels.hpp.  Host side: the design products as the constructor,
// applySettings(settings, true) and applyChannelSettings(.., true) derive them (udpsrc.cpp:463-621), the two layouts and
// the launches; the rest is demod_bank.hpp's.  The SSB formats 4 .. 7 (sdrx_udpsrc_create_ex) add the one fftfilt design every
// UDPSrc shares and the kernels of udpsrc_ssb_kernels.hpp.
#include "sdrx_common.hpp"
#include "udpsrc_kernels.hpp"
#include "udpsrc_ssb_kernels.hpp"
#include "demod_bank.hpp"
#include "backend_design.hpp"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace sdrx;

namespace {

constexpr int UDP_MAX_GATE = 1000;                  // 10 s

int elem_size(int fmt) { return fmt == UDP_IQ24 ? 8 : (fmt == UDP_IQ16 || fmt == UDP_NFM || fmt == UDP_LSB || fmt == UDP_USB ? 4 : 2); }

// sdrx_udpsrc_create_ex's flags for the validate() of the create call in progress on this thread
thread_local uint32_t create_flags = 0;

// m_sampleDistanceRemain = m_inputSampleRate / m_outputSampleRate, a float quotient, is both the distance step and where it starts
float distance_step(const sdrx_udpsrc_cfg& k) { return (float)k.in_rate / k.output_sample_rate; }

} // namespace

struct UdpFamily : DemodDefaults {
    using Handle = sdrx_udpsrc;
    using Cfg = sdrx_udpsrc_cfg;
    using Chan = UdpChan;
    using Bufs = UdpBufs;
    static constexpr const char* name = "sdrx_udpsrc";
    static constexpr const float2* UdpBufs::* input = &UdpBufs::ci;
    static constexpr int bp_taps = AM_BP_H + 1;

    static int validate(int32_t n_ch, const sdrx_udpsrc_cfg* cfg)
    {
        if (n_ch <= 0 || !cfg) { set_error("sdrx_udpsrc_create: bad argument"); return SDRX_EINVAL; }
        for (int c = 0; c < n_ch; c++) {
            const sdrx_udpsrc_cfg& k = cfg[c];
            const int f = k.sample_format;
            if (udp_fmt_ssb(f) && !(create_flags & SDRX_UDPSRC_SSB_FORMATS)) {
                set_error("sdrx_udpsrc_create: the SSB formats (4 .. 7) are left out: they need the 512-point g_fft network and an AGC factor in front of the filter");
                return SDRX_EINVAL;
            }
            if (f < 0 || f > UDP_AM_BPF_MONO) { set_error("sdrx_udpsrc_create: bad channel configuration (unknown sample_format)"); return SDRX_EINVAL; }
            if (k.in_rate <= 0 || !(k.output_sample_rate >= 1000.0f) || !(k.output_sample_rate <= (float)k.in_rate) || !(k.output_sample_rate <= 1.0e7f)) {
                set_error("sdrx_udpsrc_create: bad channel configuration (need 1000 <= output_sample_rate <= min(in_rate, 1e7); the interpolating branch is left out)");
                return SDRX_EINVAL;
            }
            if (!(k.rf_bandwidth > 0.0f) || !(k.rf_bandwidth <= 1.0e7f)) {
                set_error("sdrx_udpsrc_create: bad channel configuration (need 0 < rf_bandwidth <= 1e7)"); return SDRX_EINVAL;
            }
            if (f == UDP_AM_BPF_MONO && !(k.rf_bandwidth > 600.0f)) {
                set_error("sdrx_udpsrc_create: bad channel configuration (need rf_bandwidth > 600 for format 10: the Bandpass starts at 300 Hz)"); return SDRX_EINVAL;
            }
            if (k.fm_deviation <= 0) { set_error("sdrx_udpsrc_create: bad channel configuration (need fm_deviation > 0)"); return SDRX_EINVAL; }
            if (k.squelch_gate < 0 || k.squelch_gate > UDP_MAX_GATE) {
                set_error("sdrx_udpsrc_create: bad channel configuration (need 0 <= squelch_gate <= 1000, in 1/100 s)"); return SDRX_EINVAL;
            }
            if (k.squelch_db < -300 || k.squelch_db > 300) { set_error("sdrx_udpsrc_create: bad channel configuration (need -300 <= squelch_db <= 300)"); return SDRX_EINVAL; }
            if (!std::isfinite(k.gain)) { set_error("sdrx_udpsrc_create: bad channel configuration (gain must be finite)"); return SDRX_EINVAL; }
            // rate >= 1000 keeps every window at 5 entries or more (int(rate * 0.005)): no window can come out below 1
        }
        return SDRX_OK;
    }

    static void design(int c, const sdrx_udpsrc_cfg& k, sdrx_backend_cfg& f, UdpChan& s, float* bp)
    {
        const float rate = k.output_sample_rate;
        f.in_rate = k.in_rate; f.nco_freq = k.nco_freq; f.out_rate = (int32_t)rate;       // the step itself goes in through backend_start_at
        f.interp_cutoff = k.rf_bandwidth / 2.0f;            // m_interpolator.create(16, inputSampleRate, rfBandwidth / 2.0): the halving is exact
        f.taps_per_phase = 4.5f;
        s.fmt = k.sample_format;
        s.ssb = udp_fmt_ssb(s.fmt) ? 1 : 0;
        const int release = (int)((rate * (float)k.squelch_gate) / 100.0f);       // (m_outputSampleRate * m_squelchGate) / 100, float arithmetic
        s.gate = s.ssb ? (int)((double)rate * 0.05) : release;                    // the SSB formats: m_outputSampleRate * 0.05, a double product
        s.top = udp_sq_top(s.gate, udp_sq_release(s.gate, release));
        s.sq_enabled = k.squelch_enabled ? 1 : 0;
        s.w_in = (int)((double)rate * 0.01);
        s.w_am = (int)((double)rate * 0.005);
        s.xk = s.fmt == UDP_AM_NODC_MONO ? s.w_am : (s.fmt == UDP_AM_BPF_MONO ? AM_BP_HIST : 1);
        s.bp_off = c * bp_taps;
        s.level = std::pow(10.0, (double)k.squelch_db / 10.0);        // CalcDb::powerFromdB
        s.gain = k.gain;
        s.fm_scaling = rate / (2.0f * (float)k.fm_deviation);
        // m_agc.resize(rate / 5, rate / 20, m_agcTarget), setStepDownDelay((rate * (gate == 0 ? 1 : gate)) / 100), setGate(rate * 0.05),
        // setThreshold(m_squelch * (1 << 23)): float quotients and products truncated to int
        s.agc = (k.agc && s.fmt >= UDP_LSB) ? 1 : 0;          // udpsrc.cpp:155-163 excludes formats 0 .. 3 only
        s.a_hn = (int)(rate / 5); s.a_L = (int)(rate / 20);
        s.a_sdd = (int)((rate * (float)(k.squelch_gate == 0 ? 1 : k.squelch_gate)) / 100.0f);
        s.a_gate = (int)((double)rate * 0.05);
        s.a_thr = s.level * (double)(1 << 23);
        s.a_g = 0; s.a_count = 0; s.a_U = 0; s.a_D = s.a_L; s.agc_sum = 0.0;
        s.pos = 0;                                                    // initSquelch(false)
        s.in_sum = (double)s.w_in * udp_ma_initial();
        s.am_sum = (double)s.w_am * udp_ma_initial();
        // m_bandpass.create(301, outputSampleRate, 300.0, rfBandwidth / 2.0f)
        demod_bandpass_design((double)rate, 300.0, (double)(k.rf_bandwidth / 2.0f), bp);
    }

    static int front_made(sdrx_backend_t* front, int n_ch, const sdrx_udpsrc_cfg* cfg)
    {
        for (int c = 0; c < n_ch; c++) {
            int rc = backend_start_at(front, c, distance_step(cfg[c]), distance_step(cfg[c])); if (rc) return rc;
        }
        return SDRX_OK;
    }

    // one history set: [w_in input powers | xk compacted-stream elements | a_hn raw powers (AGC on)]
    static void hist(HistCarver& k, const UdpChan& s, UdpBufs& u)
    {
        k.pair(u.mhist, u.mhist_next, (size_t)s.w_in);
        k.pair(u.xhist, u.xhist_next, (size_t)s.xk);
        u.ghist = nullptr; u.ghist_next = nullptr;          // no AGC, no history: a use would fault plainly
        if (s.agc) k.pair(u.ghist, u.ghist_next, (size_t)s.a_hn);
        u.pend = nullptr; u.pend_next = nullptr; u.ovl = nullptr; u.ovl_next = nullptr;
        if (s.ssb) { k.pair(u.pend, u.pend_next, (size_t)UDP_SSB_H); k.pair(u.ovl, u.ovl_next, (size_t)UDP_SSB_H); }
    }

    // both averages are filled with 1e-10 (resize(n, 1e-10)); the Bandpass ring and the AGC history are 0
    static void fresh(const UdpChan& s, UdpBufs& u)
    {
        for (int i = 0; i < s.w_in; i++) u.mhist_next[i] = udp_ma_initial();
        if (s.fmt == UDP_AM_NODC_MONO) for (int i = 0; i < s.xk; i++) u.xhist_next[i] = udp_ma_initial();
    }

    static void work(Carver& k, size_t n, const UdpChan& s, UdpBufs& u)
    {
        const size_t nblk = n / 256 + 1;
        u.dterm = k.take<double>(n); u.tot = k.take<double>(n);
        // format 4 interleaves n raw elements with up to n / 256 + 1 blocks of 256: udp_ssb_payload_bound(n) elements of 4 bytes
        u.x = k.take<double>(n); u.out = k.take<char>(s.ssb ? (size_t)udp_ssb_payload_bound((long)n) * 4 : n * 8);
        u.gterm = k.take<double>(n); u.gtot = k.take<double>(n);
        u.aidx = k.take<int>(n); u.spec = k.take<int16_t>(2 * n);
        u.blk_a = k.take<int>(nblk);
        u.head = nullptr; u.tail = nullptr;
        if (s.ssb) { u.head = k.take<float2>(nblk * UDP_SSB_H); u.tail = k.take<float2>(nblk * UDP_SSB_H); }
    }

    static int64_t outputs_bound(const sdrx_udpsrc_cfg& k, int64_t n_in) { return demod_outputs_bound((int64_t)std::floor(distance_step(k)), n_in); }

    static int launch(DemodBank<UdpFamily>& b, unsigned nc, unsigned gx);
};

// the handle adds what only the SSB formats need: fftfilt(0.0, (12500 / 2.0) / 48000, 512), built once in UDPSrc's constructor from
// the default settings and never rebuilt by applySettings, so one design serves every channel
struct sdrx_udpsrc : DemodBank<UdpFamily> {
    bool any_ssb = false;
    float2* d_filt = nullptr;
    float* d_utbl = nullptr;
    std::vector<float> filt;                                // the 512 complex bins
};
using Bank = DemodBank<UdpFamily>;

int UdpFamily::launch(DemodBank<UdpFamily>& b, unsigned nc, unsigned gx)
    {
        const unsigned gp = (nc + PS_CH - 1) / PS_CH;
        hipLaunchKernelGGL(udp_level_kernel, dim3(gx, nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
        SDRX_HIP(hipGetLastError());
        hipLaunchKernelGGL(udp_psum_kernel, dim3(gp), dim3(64), 0, b.core.stream, b.d_chan, b.d_bufs, b.n_ch);
        SDRX_HIP(hipGetLastError());
        bool any_nodc = false, any_agc = false;
        for (const UdpChan& s : b.h_chan) { any_nodc = any_nodc || s.fmt == UDP_AM_NODC_MONO; any_agc = any_agc || s.agc; }
        if (any_agc) {
            hipLaunchKernelGGL(udp_agcpsum_kernel, dim3(gp), dim3(64), 0, b.core.stream, b.d_chan, b.d_bufs, b.n_ch);
            SDRX_HIP(hipGetLastError());
            hipLaunchKernelGGL(udp_agc_kernel, dim3(nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
            SDRX_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(udp_gate_kernel, dim3(nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
        SDRX_HIP(hipGetLastError());
        if (any_nodc) {
            hipLaunchKernelGGL(udp_amterm_kernel, dim3(gx, nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
            SDRX_HIP(hipGetLastError());
            hipLaunchKernelGGL(udp_ampsum_kernel, dim3(gp), dim3(64), 0, b.core.stream, b.d_chan, b.d_bufs, b.n_ch);
            SDRX_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(udp_out_kernel, dim3(gx, nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs, b.d_bp);
        SDRX_HIP(hipGetLastError());
        b.core.note_launch("udp_out_kernel", (int)(gx * nc), 256, (int)((AM_BP_H + 1) * sizeof(float) + UDP_OUT_WIN * sizeof(double)));
        const sdrx_udpsrc& h = static_cast<const sdrx_udpsrc&>(b);
        if (h.any_ssb) {
            // a feed's blocks: at most ceil(n / 256) <= gx, whatever was pending
            hipLaunchKernelGGL(udp_ssb_fft_kernel, dim3((gx + UDP_SSB_WAVES - 1) / UDP_SSB_WAVES, nc), dim3(64 * UDP_SSB_WAVES), 0, b.core.stream,
                               b.d_chan, b.d_bufs, h.d_filt, h.d_utbl);
            SDRX_HIP(hipGetLastError());
            hipLaunchKernelGGL(udp_ssb_out_kernel, dim3(gx, nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
            SDRX_HIP(hipGetLastError());
            hipLaunchKernelGGL(udp_ssb_carry_kernel, dim3(nc), dim3(UDP_SSB_H), 0, b.core.stream, b.d_chan, b.d_bufs);
            SDRX_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(udp_carry_kernel, dim3(nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
        SDRX_HIP(hipGetLastError());
        return SDRX_OK;
    }

// the shared design, behind a successful Bank::create
static int make_ssb_design(sdrx_udpsrc* b)
{
    for (const UdpChan& s : b->h_chan) b->any_ssb = b->any_ssb || s.ssb;
    if (!b->any_ssb) return SDRX_OK;
    SDRX_HIP(hipSetDevice(b->core.device));
    int rc = design_upload(&b->d_utbl, design_gfft_table(UDP_SSB_FLEN)); if (rc) return rc;
    SDRX_HIP(hipMalloc(reinterpret_cast<void**>(&b->d_filt), (size_t)UDP_SSB_FLEN * sizeof(float2)));
    b->filt.assign((size_t)UDP_SSB_FLEN * 2, 0.0f);
    // (m_rfBandwidth / 2.0) / m_outputSampleRate at the defaults 12500 and 48000: a double quotient narrowed to the float parameter
    const float f2 = (float)((12500.0 / 2.0) / 48000.0);
    return design_fft_filter<UDP_SSB_FLEN>(b->d_filt, b->d_utbl, b->core.stream, b->filt.data(),
                                           [&](float* f, int h2) { fftfilt_fill_band(0.0f, f2, f, h2); });
}

static int destroy_udpsrc(sdrx_udpsrc* b)
{
    if (b) {
        (void)hipSetDevice(b->core.device);
        if (b->core.stream) (void)hipStreamSynchronize(b->core.stream);
        if (b->d_filt) (void)hipFree(b->d_filt);
        if (b->d_utbl) (void)hipFree(b->d_utbl);
    }
    return Bank::destroy(b);
}

// the size of a payload sample for read(), which refuses a bad b or c itself
static size_t payload_bytes(const sdrx_udpsrc* b, int32_t c) { return Bank::in_range(b, c) ? (size_t)elem_size(b->h_chan[(size_t)c].fmt) : 0; }

extern "C" {

int sdrx_udpsrc_create_ex(sdrx_udpsrc_t** out, int device, int32_t n_ch, const sdrx_udpsrc_cfg* cfg, uint32_t flags)
{
    if (out) *out = nullptr;
    if (flags & ~SDRX_UDPSRC_SSB_FORMATS) { set_error("sdrx_udpsrc_create_ex: unknown flag bits"); return SDRX_EINVAL; }
    create_flags = flags;
    int rc = Bank::create(out, device, n_ch, cfg);
    create_flags = 0;
    if (rc) return rc;
    rc = make_ssb_design(*out);
    if (rc) { destroy_udpsrc(*out); *out = nullptr; }
    return rc;
}
int sdrx_udpsrc_create(sdrx_udpsrc_t** out, int device, int32_t n_ch, const sdrx_udpsrc_cfg* cfg) { return sdrx_udpsrc_create_ex(out, device, n_ch, cfg, 0); }
int sdrx_udpsrc_destroy(sdrx_udpsrc_t* b) { return destroy_udpsrc(b); }
int sdrx_udpsrc_reset(sdrx_udpsrc_t* b) { return Bank::reset(b); }
int sdrx_udpsrc_feed_dev(sdrx_udpsrc_t* b, const int16_t* const* d_iq, const int64_t* n_per_ch) { return Bank::feed_dev(b, d_iq, n_per_ch); }
int sdrx_udpsrc_feed_bank(sdrx_udpsrc_t* b, sdrx_chan_bank_t* bank) { return Bank::feed_bank(b, bank); }
int sdrx_udpsrc_feed(sdrx_udpsrc_t* b, const int16_t* const* iq, const int64_t* n_per_ch) { return Bank::feed(b, iq, n_per_ch); }
int64_t sdrx_udpsrc_read(sdrx_udpsrc_t* b, int32_t c, void* payload, int64_t cap_samples) { return Bank::read(b, "read", c, payload, cap_samples, &UdpBufs::out, &UdpChan::n_pay, payload_bytes(b, c)); }
int sdrx_udpsrc_last_dev(sdrx_udpsrc_t* b, int32_t c, const void** d_payload, int64_t* n_samples) { return Bank::last_dev(b, "last_dev", c, d_payload, n_samples, &UdpBufs::out, &UdpChan::n_pay); }
int64_t sdrx_udpsrc_read_spectrum(sdrx_udpsrc_t* b, int32_t c, int16_t* samples_iq, int64_t cap_samples) { return Bank::read(b, "read_spectrum", c, samples_iq, cap_samples, &UdpBufs::spec, &UdpChan::n, 4); }
int sdrx_udpsrc_spectrum_last_dev(sdrx_udpsrc_t* b, int32_t c, const int16_t** d_samples_iq, int64_t* n_samples) { return Bank::last_dev(b, "spectrum_last_dev", c, d_samples_iq, n_samples, &UdpBufs::spec, &UdpChan::n); }

int32_t sdrx_udpsrc_sample_bytes(sdrx_udpsrc_t* b, int32_t c)
{
    if (!Bank::in_range(b, c)) return Bank::fail("sample_bytes", ": bad argument");
    return elem_size(b->h_chan[(size_t)c].fmt);
}

int sdrx_udpsrc_squelch_open(sdrx_udpsrc_t* b, int32_t c)
{
    UdpChan s;
    int rc = Bank::fetch(b, "squelch_open", c, &s); if (rc) return rc;
    return udp_sq_open(s.pos, s.gate) ? 1 : 0;
}

int sdrx_udpsrc_squelch_counts(sdrx_udpsrc_t* b, int32_t c, int32_t* open_count, int32_t* close_count)
{
    UdpChan s;
    int rc = Bank::fetch(b, "squelch_counts", c, &s); if (rc) return rc;
    // m_squelchGate == 0: the counters never move
    if (open_count) *open_count = s.gate ? udp_sq_open_count(s.pos, s.gate) : 0;
    if (close_count) *close_count = s.gate ? udp_sq_close_count(s.pos, s.gate) : 0;
    return SDRX_OK;
}

int sdrx_udpsrc_in_magsq(sdrx_udpsrc_t* b, int32_t c, double* in_magsq)
{
    if (!in_magsq) return Bank::fail("in_magsq", ": bad argument");
    UdpChan s;
    int rc = Bank::fetch(b, "in_magsq", c, &s); if (rc) return rc;
    // m_inMagsq = m_inMovingAverage.average(); 0 (the constructor's value) until the first output sample
    *in_magsq = s.total > 0 ? s.in_sum / (double)s.w_in : 0.0;
    return SDRX_OK;
}

int64_t sdrx_udpsrc_total(sdrx_udpsrc_t* b, int32_t c)
{
    UdpChan s;
    int rc = Bank::fetch(b, "total", c, &s); if (rc) return rc;
    return (int64_t)(s.ssb ? s.total_pay : s.total);
}

int sdrx_udpsrc_ssb_state(sdrx_udpsrc_t* b, int32_t c, int32_t* pending, int64_t* blocks, float* filter_iq)
{
    UdpChan s;
    int rc = Bank::fetch(b, "ssb_state", c, &s); if (rc) return rc;
    if (!s.ssb) return Bank::fail("ssb_state", ": the channel has none of the SSB formats 4 .. 7");
    if (pending) *pending = s.s_pend;
    if (blocks) *blocks = (int64_t)s.s_blocks;
    if (filter_iq) std::copy(b->filt.begin(), b->filt.end(), filter_iq);
    return SDRX_OK;
}

int sdrx_udpsrc_get_design(sdrx_udpsrc_t* b, int32_t c, int32_t* ntaps_per_phase, double* taps, int32_t taps_cap, double* bandpass_taps,
                           int32_t* nco_inc, int32_t* windows, int32_t* squelch_gate, int32_t* squelch_release, double* squelch_level,
                           float* fm_scaling, float* distance_step, int32_t* agc_ints, double* agc_threshold)
{
    if (!Bank::in_range(b, c)) return Bank::fail("get_design", ": bad channel");
    int nt = 0;
    int rc = sdrx_backend_get_design(b->front, c, &nt, nullptr, 0, nullptr, nco_inc); if (rc) return rc;
    if (ntaps_per_phase) *ntaps_per_phase = nt;
    if (taps && taps_cap > 0) {
        std::vector<float> t((size_t)nt * 16);
        rc = sdrx_backend_get_design(b->front, c, nullptr, t.data(), nt * 16, nullptr, nullptr); if (rc) return rc;
        for (int i = 0; i < std::min(taps_cap, nt * 16); i++) taps[i] = (double)t[(size_t)i];
    }
    const UdpChan& s = b->h_chan[(size_t)c];
    if (bandpass_taps) for (int i = 0; i <= AM_BP_H; i++) bandpass_taps[i] = (double)b->bp_all[(size_t)s.bp_off + (size_t)i];
    if (windows) { windows[0] = s.w_in; windows[1] = s.w_am; windows[2] = s.w_in; }   // m_inMovingAverage, m_amMovingAverage, m_outMovingAverage
    if (squelch_gate) *squelch_gate = s.gate;
    if (squelch_release) *squelch_release = (int)((b->cfg[(size_t)c].output_sample_rate * (float)b->cfg[(size_t)c].squelch_gate) / 100.0f);     // m_squelchRelease
    if (squelch_level) *squelch_level = s.level;
    if (fm_scaling) *fm_scaling = s.fm_scaling;
    if (distance_step) *distance_step = ::distance_step(b->cfg[(size_t)c]);
    if (agc_ints) { agc_ints[0] = s.a_hn; agc_ints[1] = s.a_L; agc_ints[2] = s.a_sdd; agc_ints[3] = s.a_gate; }
    if (agc_threshold) *agc_threshold = s.a_thr;
    return SDRX_OK;
}

int sdrx_udpsrc_sync(sdrx_udpsrc_t* b) { return b ? b->core.sync() : SDRX_EINVAL; }
int sdrx_udpsrc_set_stream(sdrx_udpsrc_t* b, void* hip_stream) { return Bank::set_stream(b, hip_stream); }
int sdrx_udpsrc_get_stream(sdrx_udpsrc_t* b, void** hip_stream) { return b ? b->core.get_stream(hip_stream) : SDRX_EINVAL; }
int sdrx_udpsrc_set_timing(sdrx_udpsrc_t* b, int enabled) { return b ? b->core.set_timing(enabled) : SDRX_EINVAL; }
int sdrx_udpsrc_get_timing(sdrx_udpsrc_t* b, double* total_ms, int64_t* feeds, int reset) { return b ? b->core.get_timing(total_ms, feeds, reset) : SDRX_EINVAL; }
int sdrx_udpsrc_last_launch(const sdrx_udpsrc_t* b, char* kernel_name, int name_cap, int* grid, int* block, int* lds_bytes) { return b ? b->core.last_launch(kernel_name, name_cap, grid, block, lds_bytes) : SDRX_EINVAL; }

} // extern "C"
