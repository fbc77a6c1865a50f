// libsdrx.so: sdrx_udpsrc_* -- N UDPSrc channels (UDPSrc::feed, plugins/channelrx/udpsrc/udpsrc.cpp:136-321) on one device:
// int16 I/Q at the channelizer's output rate in, the samples UDPSrc hands to its UDPSink (the datagram payload) out.  The
// front (NCO, Interpolator) is a channel back-end the handle owns and launches on its own stream, started one distance step
// in as UDPSrc starts it; the tail's kernels are in udpsrc_kernels.hpp.  Host side: the design products as the constructor,
// applySettings(settings, true) and applyChannelSettings(.., true) derive them (udpsrc.cpp:463-621), launches, buffer
// bookkeeping.
#include "sdrx_common.hpp"
#include "udpsrc_kernels.hpp"
#include "backend_view.hpp"
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

struct UdpHost {
    DevBuf work, stage_in;
    char* hist = nullptr;             // two sets of [w_in input powers | xk compacted-stream elements | a_hn raw powers (AGC on)]
    size_t hist_set = 0;              // bytes of one set
    int cur = 0;
    int64_t cap_in = 0;
    float step = 0.0f;                // in_rate / output_sample_rate: the distance step and the starting distance
};

constexpr int UDP_MAX_GATE = 1000;                  // 10 s
constexpr size_t al(size_t v) { return (v + 255) & ~(size_t)255; }

int elem_size(int fmt) { return fmt == UDP_IQ24 ? 8 : (fmt == UDP_IQ16 || fmt == UDP_NFM ? 4 : 2); }

} // namespace

struct sdrx_udpsrc {
    HandleCore core;
    int n_ch = 0;
    std::vector<sdrx_udpsrc_cfg> cfg;
    std::vector<sdrx_backend_cfg> be_cfg;
    sdrx_backend_t* front = nullptr;
    std::vector<UdpHost> ch;
    std::vector<UdpChan> h_chan;   // configuration and the state of a fresh handle
    std::vector<int> release;      // m_squelchRelease as the reference derives it
    UdpChan* d_chan = nullptr;
    UdpBufs* d_bufs = nullptr;
    UdpBufs* h_bufs = nullptr;     // pinned: the per-feed table goes to the device in one async copy
    hipEvent_t bufs_ev = nullptr;
    float* d_bp = nullptr;
    std::vector<float> bp_all;
};

static int validate(int32_t n_ch, const sdrx_udpsrc_cfg* cfg)
{
    if (n_ch <= 0 || !cfg) { set_error("sdrx_udpsrc_create: bad argument"); return SDRX_EINVAL; }
    for (int c = 0; c < n_ch; c++) {
        const sdrx_udpsrc_cfg& k = cfg[c];
        const int f = k.sample_format;
        if (f >= UDP_LSB && f <= UDP_USB_MONO) {
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

static int ensure_capacity(sdrx_udpsrc* b, int c, int64_t n_in)
{
    UdpHost& h = b->ch[(size_t)c];
    if (n_in <= h.cap_in) return SDRX_OK;
    int64_t cap = h.cap_in ? h.cap_in : 4096;
    while (cap < n_in) cap *= 2;
    // every output sample consumes at least one input (step >= 1): at most `cap` samples per feed; nothing here carries state
    const size_t n = (size_t)cap + 16, nblk = n / 256 + 1;
    const size_t bytes = 6 * al(n * 8) + 2 * al(n * 4) + al(nblk * 4);
    SDRX_HIP(hipStreamSynchronize(b->core.stream));
    int rc = h.work.reserve(bytes); if (rc) return rc;
    h.cap_in = cap;
    return SDRX_OK;
}

static int make_front(sdrx_udpsrc* b)
{
    int rc = sdrx_backend_create(&b->front, b->core.device, b->n_ch, b->be_cfg.data()); if (rc) return rc;
    // m_sampleDistanceRemain = m_inputSampleRate / m_outputSampleRate, a float quotient, is both the step and where it starts
    for (int c = 0; c < b->n_ch; c++) {
        rc = backend_start_at(b->front, c, b->ch[(size_t)c].step, b->ch[(size_t)c].step); if (rc) return rc;
    }
    return backend_set_stream(b->front, b->core.stream);
}

static int upload_fresh_state(sdrx_udpsrc* b)
{
    SDRX_HIP(hipMemcpyAsync(b->d_chan, b->h_chan.data(), (size_t)b->n_ch * sizeof(UdpChan), hipMemcpyHostToDevice, b->core.stream));
    for (int c = 0; c < b->n_ch; c++) {
        UdpHost& h = b->ch[(size_t)c];
        const UdpChan& s = b->h_chan[(size_t)c];
        // both averages are filled with 1e-10 (resize(n, 1e-10)); the Bandpass ring and the AGC history are 0
        std::vector<double> set(h.hist_set / 8, 0.0);
        for (int i = 0; i < s.w_in; i++) set[(size_t)i] = udp_ma_initial();
        if (s.fmt == UDP_AM_NODC_MONO) for (int i = 0; i < s.xk; i++) set[al((size_t)s.w_in * 8) / 8 + (size_t)i] = udp_ma_initial();
        for (int k = 0; k < 2; k++) SDRX_HIP(hipMemcpy(h.hist + (size_t)k * h.hist_set, set.data(), h.hist_set, hipMemcpyHostToDevice));
        h.cur = 0;
    }
    SDRX_HIP(hipStreamSynchronize(b->core.stream));
    return SDRX_OK;
}

extern "C" {

int sdrx_udpsrc_destroy(sdrx_udpsrc_t* b)
{
    if (!b) return SDRX_OK;
    (void)hipSetDevice(b->core.device);
    if (b->core.stream) (void)hipStreamSynchronize(b->core.stream);
    if (b->front) (void)sdrx_backend_destroy(b->front);
    for (auto& h : b->ch) {
        h.work.release(); h.stage_in.release();
        if (h.hist) (void)hipFree(h.hist);
    }
    if (b->d_chan) (void)hipFree(b->d_chan);
    if (b->d_bufs) (void)hipFree(b->d_bufs);
    if (b->h_bufs) (void)hipHostFree(b->h_bufs);
    if (b->bufs_ev) (void)hipEventDestroy(b->bufs_ev);
    if (b->d_bp) (void)hipFree(b->d_bp);
    b->core.close();
    delete b;
    return SDRX_OK;
}

int sdrx_udpsrc_create(sdrx_udpsrc_t** out, int device, int32_t n_ch, const sdrx_udpsrc_cfg* cfg)
{
    if (!out) { set_error("sdrx_udpsrc_create: null out"); return SDRX_EINVAL; }
    *out = nullptr;
    int rc = validate(n_ch, cfg); if (rc) return rc;
    sdrx_udpsrc* b = new (std::nothrow) sdrx_udpsrc;
    if (!b) return SDRX_ENOMEM;
    rc = b->core.open(device);
    if (rc) { delete b; return rc; }
    b->n_ch = n_ch;
    b->cfg.assign(cfg, cfg + n_ch);
    b->ch.resize((size_t)n_ch); b->h_chan.resize((size_t)n_ch); b->be_cfg.resize((size_t)n_ch); b->release.resize((size_t)n_ch);
    b->bp_all.assign((size_t)n_ch * (AM_BP_H + 1), 0.0f);

    for (int c = 0; c < n_ch; c++) {
        const sdrx_udpsrc_cfg& k = cfg[c];
        const float rate = k.output_sample_rate;
        sdrx_backend_cfg& f = b->be_cfg[(size_t)c];
        std::memset(&f, 0, sizeof f);
        f.in_rate = k.in_rate; f.nco_freq = k.nco_freq; f.out_rate = (int32_t)rate;       // the step itself goes in through backend_start_at
        f.interp_cutoff = k.rf_bandwidth / 2.0f;            // m_interpolator.create(16, inputSampleRate, rfBandwidth / 2.0): the halving is exact
        f.taps_per_phase = 4.5f;
        UdpHost& h = b->ch[(size_t)c];
        h.step = (float)k.in_rate / rate;
        UdpChan& s = b->h_chan[(size_t)c];
        std::memset(&s, 0, sizeof s);
        s.fmt = k.sample_format;
        s.gate = (int)((rate * (float)k.squelch_gate) / 100.0f);      // (m_outputSampleRate * m_squelchGate) / 100, float arithmetic
        b->release[(size_t)c] = s.gate;                               // m_squelchRelease: the same expression
        s.top = udp_sq_top(s.gate, udp_sq_release(s.gate, s.gate));
        s.sq_enabled = k.squelch_enabled ? 1 : 0;
        s.w_in = (int)((double)rate * 0.01);
        s.w_am = (int)((double)rate * 0.005);
        s.xk = s.fmt == UDP_AM_NODC_MONO ? s.w_am : (s.fmt == UDP_AM_BPF_MONO ? AM_BP_HIST : 1);
        s.bp_off = c * (AM_BP_H + 1);
        s.level = std::pow(10.0, (double)k.squelch_db / 10.0);        // CalcDb::powerFromdB
        s.gain = k.gain;
        s.fm_scaling = rate / (2.0f * (float)k.fm_deviation);
        // m_agc.resize(rate / 5, rate / 20, m_agcTarget), setStepDownDelay((rate * (gate == 0 ? 1 : gate)) / 100), setGate(rate * 0.05),
        // setThreshold(m_squelch * (1 << 23)): float quotients and products truncated to int
        s.agc = (k.agc && s.fmt >= UDP_AM_MONO) ? 1 : 0;
        s.a_hn = (int)(rate / 5); s.a_L = (int)(rate / 20);
        s.a_sdd = (int)((rate * (float)(k.squelch_gate == 0 ? 1 : k.squelch_gate)) / 100.0f);
        s.a_gate = (int)((double)rate * 0.05);
        s.a_thr = s.level * (double)(1 << 23);
        s.a_g = 0; s.a_count = 0; s.a_U = 0; s.a_D = s.a_L; s.agc_sum = 0.0;
        s.pos = 0;                                                    // initSquelch(false)
        s.in_sum = (double)s.w_in * udp_ma_initial();
        s.am_sum = (double)s.w_am * udp_ma_initial();
        // m_bandpass.create(301, outputSampleRate, 300.0, rfBandwidth / 2.0f)
        demod_bandpass_design((double)rate, 300.0, (double)(k.rf_bandwidth / 2.0f), &b->bp_all[(size_t)s.bp_off]);
        h.hist_set = al((size_t)s.w_in * 8) + al((size_t)s.xk * 8) + (s.agc ? al((size_t)s.a_hn * 8) : 0);
        SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&h.hist), 2 * h.hist_set), sdrx_udpsrc_destroy(b));
    }
    SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&b->d_bp), b->bp_all.size() * 4), sdrx_udpsrc_destroy(b));
    SDRX_HIP_ELSE(hipMemcpy(b->d_bp, b->bp_all.data(), b->bp_all.size() * 4, hipMemcpyHostToDevice), sdrx_udpsrc_destroy(b));
    SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&b->d_chan), (size_t)n_ch * sizeof(UdpChan)), sdrx_udpsrc_destroy(b));
    SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&b->d_bufs), (size_t)n_ch * sizeof(UdpBufs)), sdrx_udpsrc_destroy(b));
    SDRX_HIP_ELSE(hipHostMalloc(reinterpret_cast<void**>(&b->h_bufs), (size_t)n_ch * sizeof(UdpBufs), hipHostMallocDefault), sdrx_udpsrc_destroy(b));
    SDRX_HIP_ELSE(hipEventCreateWithFlags(&b->bufs_ev, hipEventDisableTiming), sdrx_udpsrc_destroy(b));
    SDRX_HIP_ELSE(hipEventRecord(b->bufs_ev, b->core.stream), sdrx_udpsrc_destroy(b));
    rc = make_front(b);
    if (!rc) rc = upload_fresh_state(b);
    if (rc) { sdrx_udpsrc_destroy(b); return rc; }
    *out = b;
    return SDRX_OK;
}

int sdrx_udpsrc_reset(sdrx_udpsrc_t* b)
{
    if (!b) { set_error("sdrx_udpsrc_reset: null handle"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    SDRX_HIP(hipStreamSynchronize(b->core.stream));
    // the front has no reset of its own: a fresh one with the same design
    if (b->front) { (void)sdrx_backend_destroy(b->front); b->front = nullptr; }
    int rc = make_front(b); if (rc) return rc;
    return upload_fresh_state(b);
}

// the tail behind a front feed that has just been queued on the handle's stream
static int tail_common(sdrx_udpsrc* b, const int64_t* n_per_ch)
{
    int64_t bound = 0;
    for (int c = 0; c < b->n_ch; c++) {
        int rc = ensure_capacity(b, c, std::max<int64_t>(n_per_ch[c], 1)); if (rc) return rc;
        // every output sample after the first two of a stream consumes >= floor(step) inputs
        const int64_t per_out = std::max<int64_t>(1, (int64_t)std::floor(b->ch[(size_t)c].step));
        bound = std::max(bound, std::min<int64_t>(n_per_ch[c], n_per_ch[c] / per_out + 4));
    }
    SDRX_HIP(hipEventSynchronize(b->bufs_ev));            // previous feed's copy has read the table
    for (int c = 0; c < b->n_ch; c++) {
        UdpHost& h = b->ch[(size_t)c];
        const UdpChan& s = b->h_chan[(size_t)c];
        UdpBufs& u = b->h_bufs[c];
        BackendView v;
        int rc = backend_view(b->front, c, &v); if (rc) return rc;
        u.ci = static_cast<const float2*>(v.out); u.n_ptr = v.n_out;
        char* set[2] = { h.hist + (size_t)h.cur * h.hist_set, h.hist + (size_t)(h.cur ^ 1) * h.hist_set };
        size_t o = 0;
        u.mhist = reinterpret_cast<const double*>(set[0] + o); u.mhist_next = reinterpret_cast<double*>(set[1] + o); o += al((size_t)s.w_in * 8);
        u.xhist = reinterpret_cast<const double*>(set[0] + o); u.xhist_next = reinterpret_cast<double*>(set[1] + o); o += al((size_t)s.xk * 8);
        u.ghist = nullptr; u.ghist_next = nullptr;          // no AGC, no history: a use would fault plainly
        if (s.agc) { u.ghist = reinterpret_cast<const double*>(set[0] + o); u.ghist_next = reinterpret_cast<double*>(set[1] + o); }
        const size_t n = (size_t)h.cap_in + 16, nblk = n / 256 + 1;
        char* p = static_cast<char*>(h.work.p);
        auto take = [&](size_t bytes) { char* r = p; p += al(bytes); return r; };
        u.dterm = reinterpret_cast<double*>(take(n * 8)); u.tot = reinterpret_cast<double*>(take(n * 8));
        u.x = reinterpret_cast<double*>(take(n * 8)); u.out = take(n * 8);
        u.gterm = reinterpret_cast<double*>(take(n * 8)); u.gtot = reinterpret_cast<double*>(take(n * 8));
        u.aidx = reinterpret_cast<int*>(take(n * 4)); u.spec = reinterpret_cast<int16_t*>(take(n * 4));
        u.blk_a = reinterpret_cast<int*>(take(nblk * 4));
    }
    int rc = demod_upload_bufs(b->d_bufs, b->h_bufs, b->n_ch, b->bufs_ev, b->core.stream); if (rc) return rc;
    const unsigned nc = (unsigned)b->n_ch, gp = (nc + PS_CH - 1) / PS_CH, gx = (unsigned)std::max<int64_t>(1, (bound + 255) / 256);
    hipLaunchKernelGGL(udp_level_kernel, dim3(gx, nc), dim3(256), 0, b->core.stream, b->d_chan, b->d_bufs);
    SDRX_HIP(hipGetLastError());
    hipLaunchKernelGGL(udp_psum_kernel, dim3(gp), dim3(64), 0, b->core.stream, b->d_chan, b->d_bufs, b->n_ch);
    SDRX_HIP(hipGetLastError());
    bool any_nodc = false, any_agc = false;
    for (const UdpChan& s : b->h_chan) { any_nodc = any_nodc || s.fmt == UDP_AM_NODC_MONO; any_agc = any_agc || s.agc; }
    if (any_agc) {
        hipLaunchKernelGGL(udp_agcpsum_kernel, dim3(gp), dim3(64), 0, b->core.stream, b->d_chan, b->d_bufs, b->n_ch);
        SDRX_HIP(hipGetLastError());
        hipLaunchKernelGGL(udp_agc_kernel, dim3(nc), dim3(256), 0, b->core.stream, b->d_chan, b->d_bufs);
        SDRX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(udp_gate_kernel, dim3(nc), dim3(256), 0, b->core.stream, b->d_chan, b->d_bufs);
    SDRX_HIP(hipGetLastError());
    if (any_nodc) {
        hipLaunchKernelGGL(udp_amterm_kernel, dim3(gx, nc), dim3(256), 0, b->core.stream, b->d_chan, b->d_bufs);
        SDRX_HIP(hipGetLastError());
        hipLaunchKernelGGL(udp_ampsum_kernel, dim3(gp), dim3(64), 0, b->core.stream, b->d_chan, b->d_bufs, b->n_ch);
        SDRX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(udp_out_kernel, dim3(gx, nc), dim3(256), 0, b->core.stream, b->d_chan, b->d_bufs, b->d_bp);
    SDRX_HIP(hipGetLastError());
    b->core.note_launch("udp_out_kernel", (int)(gx * nc), 256, (int)((AM_BP_H + 1) * sizeof(float) + UDP_OUT_WIN * sizeof(double)));
    hipLaunchKernelGGL(udp_carry_kernel, dim3(nc), dim3(256), 0, b->core.stream, b->d_chan, b->d_bufs);
    SDRX_HIP(hipGetLastError());
    for (auto& h : b->ch) h.cur ^= 1;
    return SDRX_OK;
}

int sdrx_udpsrc_feed_dev(sdrx_udpsrc_t* b, const int16_t* const* d_iq, const int64_t* n_per_ch)
{
    if (!b || !d_iq || !n_per_ch) { set_error("sdrx_udpsrc_feed_dev: null argument"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    int rc = demod_check_lengths(b->n_ch, n_per_ch, "sdrx_udpsrc_feed_dev"); if (rc) return rc;
    rc = demod_check_dev_pointers(b->n_ch, d_iq, n_per_ch, "sdrx_udpsrc_feed_dev"); if (rc) return rc;
    rc = b->core.timer.begin(b->core.stream); if (rc) return rc;
    rc = sdrx_backend_feed_dev(b->front, d_iq, n_per_ch); if (rc) return rc;
    rc = tail_common(b, n_per_ch); if (rc) return rc;
    return b->core.timer.end(b->core.stream);
}

int sdrx_udpsrc_feed_bank(sdrx_udpsrc_t* b, sdrx_chan_bank_t* bank)
{
    if (!b || !bank) { set_error("sdrx_udpsrc_feed_bank: null argument"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    std::vector<const int16_t*> d;                          // the front takes them from the bank itself
    std::vector<int64_t> n;
    int rc = demod_gather_bank(bank, b->n_ch, "sdrx_udpsrc_feed_bank", d, n); if (rc) return rc;
    rc = demod_check_lengths(b->n_ch, n.data(), "sdrx_udpsrc_feed_bank"); if (rc) return rc;
    rc = b->core.timer.begin(b->core.stream); if (rc) return rc;
    // the front orders its readers against the bank's stream (sdrx_backend_feed_bank); the tail reads the front's output only
    rc = sdrx_backend_feed_bank(b->front, bank); if (rc) return rc;
    rc = tail_common(b, n.data()); if (rc) return rc;
    return b->core.timer.end(b->core.stream);
}

int sdrx_udpsrc_feed(sdrx_udpsrc_t* b, const int16_t* const* iq, const int64_t* n_per_ch)
{
    if (!b || !iq || !n_per_ch) { set_error("sdrx_udpsrc_feed: null argument"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    std::vector<const int16_t*> d;
    int rc = demod_stage_inputs(b->ch, b->core.stream, iq, n_per_ch, "sdrx_udpsrc_feed", d); if (rc) return rc;
    rc = sdrx_udpsrc_feed_dev(b, d.data(), n_per_ch); if (rc) return rc;
    SDRX_HIP(hipStreamSynchronize(b->core.stream));            // the caller's buffers are free again on return
    return SDRX_OK;
}

int32_t sdrx_udpsrc_sample_bytes(sdrx_udpsrc_t* b, int32_t c)
{
    if (!b || c < 0 || c >= b->n_ch) { set_error("sdrx_udpsrc_sample_bytes: bad argument"); return SDRX_EINVAL; }
    return elem_size(b->h_chan[(size_t)c].fmt);
}

int64_t sdrx_udpsrc_read(sdrx_udpsrc_t* b, int32_t c, void* payload, int64_t cap_samples)
{
    if (!b || c < 0 || c >= b->n_ch || cap_samples < 0 || (cap_samples > 0 && !payload)) { set_error("sdrx_udpsrc_read: bad argument"); return SDRX_EINVAL; }
    UdpChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    const int64_t n = std::min<int64_t>(s.n, cap_samples);
    if (n == 0) return 0;
    SDRX_HIP(hipMemcpy(payload, b->h_bufs[c].out, (size_t)n * (size_t)elem_size(s.fmt), hipMemcpyDeviceToHost));
    return n;
}

int sdrx_udpsrc_last_dev(sdrx_udpsrc_t* b, int32_t c, const void** d_payload, int64_t* n_samples)
{
    if (!b || c < 0 || c >= b->n_ch || !d_payload || !n_samples) { set_error("sdrx_udpsrc_last_dev: bad argument"); return SDRX_EINVAL; }
    UdpChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    *d_payload = s.n > 0 ? b->h_bufs[c].out : b->ch[(size_t)c].work.p;
    *n_samples = s.n;
    return SDRX_OK;
}

int64_t sdrx_udpsrc_read_spectrum(sdrx_udpsrc_t* b, int32_t c, int16_t* samples_iq, int64_t cap_samples)
{
    if (!b || c < 0 || c >= b->n_ch || cap_samples < 0 || (cap_samples > 0 && !samples_iq)) { set_error("sdrx_udpsrc_read_spectrum: bad argument"); return SDRX_EINVAL; }
    UdpChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    const int64_t n = std::min<int64_t>(s.n, cap_samples);
    if (n == 0) return 0;
    SDRX_HIP(hipMemcpy(samples_iq, b->h_bufs[c].spec, (size_t)n * 4, hipMemcpyDeviceToHost));
    return n;
}

int sdrx_udpsrc_spectrum_last_dev(sdrx_udpsrc_t* b, int32_t c, const int16_t** d_samples_iq, int64_t* n_samples)
{
    if (!b || c < 0 || c >= b->n_ch || !d_samples_iq || !n_samples) { set_error("sdrx_udpsrc_spectrum_last_dev: bad argument"); return SDRX_EINVAL; }
    UdpChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    *d_samples_iq = s.n > 0 ? b->h_bufs[c].spec : static_cast<const int16_t*>(b->ch[(size_t)c].work.p);
    *n_samples = s.n;
    return SDRX_OK;
}

int sdrx_udpsrc_squelch_open(sdrx_udpsrc_t* b, int32_t c)
{
    if (!b || c < 0 || c >= b->n_ch) { set_error("sdrx_udpsrc_squelch_open: bad argument"); return SDRX_EINVAL; }
    UdpChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    return udp_sq_open(s.pos, s.gate) ? 1 : 0;
}

int sdrx_udpsrc_squelch_counts(sdrx_udpsrc_t* b, int32_t c, int32_t* open_count, int32_t* close_count)
{
    if (!b || c < 0 || c >= b->n_ch) { set_error("sdrx_udpsrc_squelch_counts: bad argument"); return SDRX_EINVAL; }
    UdpChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    // m_squelchGate == 0: the counters never move
    if (open_count) *open_count = s.gate ? udp_sq_open_count(s.pos, s.gate) : 0;
    if (close_count) *close_count = s.gate ? udp_sq_close_count(s.pos, s.gate) : 0;
    return SDRX_OK;
}

int sdrx_udpsrc_in_magsq(sdrx_udpsrc_t* b, int32_t c, double* in_magsq)
{
    if (!b || c < 0 || c >= b->n_ch || !in_magsq) { set_error("sdrx_udpsrc_in_magsq: bad argument"); return SDRX_EINVAL; }
    UdpChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    // m_inMagsq = m_inMovingAverage.average(); 0 (the constructor's value) until the first output sample
    *in_magsq = s.total > 0 ? s.in_sum / (double)s.w_in : 0.0;
    return SDRX_OK;
}

int64_t sdrx_udpsrc_total(sdrx_udpsrc_t* b, int32_t c)
{
    if (!b || c < 0 || c >= b->n_ch) { set_error("sdrx_udpsrc_total: bad argument"); return SDRX_EINVAL; }
    UdpChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    return (int64_t)s.total;
}

int sdrx_udpsrc_get_design(sdrx_udpsrc_t* b, int32_t c, int32_t* ntaps_per_phase, double* taps, int32_t taps_cap, double* bandpass_taps,
                           int32_t* nco_inc, int32_t* windows, int32_t* squelch_gate, int32_t* squelch_release, double* squelch_level,
                           float* fm_scaling, float* distance_step, int32_t* agc_ints, double* agc_threshold)
{
    if (!b || c < 0 || c >= b->n_ch) { set_error("sdrx_udpsrc_get_design: bad channel"); return SDRX_EINVAL; }
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
    if (squelch_release) *squelch_release = b->release[(size_t)c];
    if (squelch_level) *squelch_level = s.level;
    if (fm_scaling) *fm_scaling = s.fm_scaling;
    if (distance_step) *distance_step = b->ch[(size_t)c].step;
    if (agc_ints) { agc_ints[0] = s.a_hn; agc_ints[1] = s.a_L; agc_ints[2] = s.a_sdd; agc_ints[3] = s.a_gate; }
    if (agc_threshold) *agc_threshold = s.a_thr;
    return SDRX_OK;
}

int sdrx_udpsrc_sync(sdrx_udpsrc_t* b) { return b ? b->core.sync() : SDRX_EINVAL; }

int sdrx_udpsrc_set_stream(sdrx_udpsrc_t* b, void* hip_stream)
{
    if (!b) return SDRX_EINVAL;
    int rc = b->core.set_stream(hip_stream); if (rc) return rc;
    return backend_set_stream(b->front, b->core.stream);      // the front launches on the same stream
}

int sdrx_udpsrc_get_stream(sdrx_udpsrc_t* b, void** hip_stream) { return b ? b->core.get_stream(hip_stream) : SDRX_EINVAL; }

int sdrx_udpsrc_set_timing(sdrx_udpsrc_t* b, int enabled) { return b ? b->core.set_timing(enabled) : SDRX_EINVAL; }

int sdrx_udpsrc_get_timing(sdrx_udpsrc_t* b, double* total_ms, int64_t* feeds, int reset) { return b ? b->core.get_timing(total_ms, feeds, reset) : SDRX_EINVAL; }

int sdrx_udpsrc_last_launch(const sdrx_udpsrc_t* b, char* kernel_name, int name_cap, int* grid, int* block, int* lds_bytes) { return b ? b->core.last_launch(kernel_name, name_cap, grid, block, lds_bytes) : SDRX_EINVAL; }

} // extern "C"
