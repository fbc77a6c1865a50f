// libsdrx.so: sdrx_nfm_* -- N narrowband-FM demodulators (NFMDemod::feed, plugins/channelrx/demodnfm/nfmdemod.cpp:140-332, with
// m_deltaSquelch and m_ctcssOn off) on one device: int16 I/Q at the channelizer's output rate in, mono qint16 audio out.  The
// front (NCO, Interpolator) is a channel back-end the handle owns and launches on its own stream; the tail's kernels are in
// nfm_kernels.hpp.  Host side: the design products as the constructor / applySettings(settings, true) derive them
// (nfmdemod.cpp:80-91, 495-538), launches, buffer bookkeeping.
#include "sdrx_common.hpp"
#include "nfm_kernels.hpp"
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

struct NfmHost {
    DevBuf work, stage_in;
    char* hist = nullptr;             // two sets of [32 magsq | D delay-line writes | 300 Bandpass inputs]
    size_t hist_set = 0;              // bytes of one set
    int cur = 0;
    int64_t cap_in = 0;
};

constexpr int NFM_MAX_GATE = 1000;                  // 10 s: 2 * gate stays far inside an int at any audio rate
constexpr size_t al(size_t v) { return (v + 255) & ~(size_t)255; }

} // namespace

struct sdrx_nfm {
    HandleCore core;
    int n_ch = 0;
    std::vector<sdrx_nfm_cfg> cfg;
    std::vector<sdrx_backend_cfg> be_cfg;
    sdrx_backend_t* front = nullptr;
    std::vector<NfmHost> ch;
    std::vector<NfmChan> h_chan;   // configuration and the state of a fresh handle
    NfmChan* d_chan = nullptr;
    NfmBufs* d_bufs = nullptr;
    NfmBufs* h_bufs = nullptr;     // pinned: the per-feed table goes to the device in one async copy
    hipEvent_t bufs_ev = nullptr;
    float* d_bp = nullptr;
    std::vector<float> bp_all;
};

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

static int ensure_capacity(sdrx_nfm* b, int c, int64_t n_in)
{
    NfmHost& h = b->ch[(size_t)c];
    if (n_in <= h.cap_in) return SDRX_OK;
    int64_t cap = h.cap_in ? h.cap_in : 4096;
    while (cap < n_in) cap *= 2;
    // every audio sample consumes at least one input (step >= 1): at most `cap` samples per feed; nothing here carries state
    const size_t n = (size_t)cap + 16, nblk = n / 256 + 1;
    const size_t bytes = 5 * al(n * 4) + 2 * al(n * 8) + al(n * 2) + al(nblk * 8) + 2 * al(nblk * 4);
    SDRX_HIP(hipStreamSynchronize(b->core.stream));
    int rc = h.work.reserve(bytes); if (rc) return rc;
    h.cap_in = cap;
    return SDRX_OK;
}

static int upload_fresh_state(sdrx_nfm* b)
{
    SDRX_HIP(hipMemcpyAsync(b->d_chan, b->h_chan.data(), (size_t)b->n_ch * sizeof(NfmChan), hipMemcpyHostToDevice, b->core.stream));
    for (int c = 0; c < b->n_ch; c++) {
        NfmHost& h = b->ch[(size_t)c];
        // moving average empty (the power before the stream counts as 0), delay line and Bandpass ring 0 (the delay line too:
        // DoubleBufferFIFO does not clear its array, see sdrx.h)
        SDRX_HIP(hipMemsetAsync(h.hist, 0, 2 * h.hist_set, b->core.stream));
        h.cur = 0;
    }
    SDRX_HIP(hipStreamSynchronize(b->core.stream));
    return SDRX_OK;
}

static int make_front(sdrx_nfm* b)
{
    int rc = sdrx_backend_create(&b->front, b->core.device, b->n_ch, b->be_cfg.data()); if (rc) return rc;
    return backend_set_stream(b->front, b->core.stream);
}

extern "C" {

int sdrx_nfm_destroy(sdrx_nfm_t* b)
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

int sdrx_nfm_create(sdrx_nfm_t** out, int device, int32_t n_ch, const sdrx_nfm_cfg* cfg)
{
    if (!out) { set_error("sdrx_nfm_create: null out"); return SDRX_EINVAL; }
    *out = nullptr;
    int rc = validate(n_ch, cfg); if (rc) return rc;
    sdrx_nfm* b = new (std::nothrow) sdrx_nfm;
    if (!b) return SDRX_ENOMEM;
    rc = b->core.open(device);
    if (rc) { delete b; return rc; }
    b->n_ch = n_ch;
    b->cfg.assign(cfg, cfg + n_ch);
    b->ch.resize((size_t)n_ch); b->h_chan.resize((size_t)n_ch); b->be_cfg.resize((size_t)n_ch);
    b->bp_all.assign((size_t)n_ch * (AM_BP_H + 1), 0.0f);

    for (int c = 0; c < n_ch; c++) {
        const sdrx_nfm_cfg& k = cfg[c];
        sdrx_backend_cfg& f = b->be_cfg[(size_t)c];
        std::memset(&f, 0, sizeof f);
        f.in_rate = k.in_rate; f.nco_freq = k.nco_freq; f.out_rate = k.audio_rate;
        f.interp_cutoff = k.rf_bandwidth / 2.2f;            // m_interpolator.create(16, inputSampleRate, rfBandwidth / 2.2f)
        f.taps_per_phase = 4.5f;
        NfmChan& s = b->h_chan[(size_t)c];
        std::memset(&s, 0, sizeof s);
        s.gate = (k.audio_rate / 100) * k.squelch_gate;     // gate is given in 10s of ms
        s.D = nfm_delay(s.gate);
        s.level = (float)std::pow(10.0, (double)k.squelch / 100.0);         // centi-Bels
        s.volume = k.volume;
        s.fm_scaling = (8.0f * (float)(uint32_t)k.audio_rate) / (float)k.fm_deviation;
        s.comp = (float)(uint32_t)k.audio_rate / 48000.0f; s.comp *= std::sqrt(s.comp);     // nfmdemod.cpp:82-83, sqrt of a Real
        s.mute = k.audio_mute ? 1 : 0;
        s.bp_off = c * (AM_BP_H + 1);
        // m_bandpass.create(301, audioSampleRate, 300.0, afBandwidth)
        demod_bandpass_design((double)k.audio_rate, 300.0, (double)k.af_bandwidth, &b->bp_all[(size_t)s.bp_off]);
        NfmHost& h = b->ch[(size_t)c];
        h.hist_set = al(NFM_MA * 4) + al((size_t)s.D * 4) + al(AM_BP_HIST * 4);
        SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&h.hist), 2 * h.hist_set), sdrx_nfm_destroy(b));
    }
    SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&b->d_bp), b->bp_all.size() * 4), sdrx_nfm_destroy(b));
    SDRX_HIP_ELSE(hipMemcpy(b->d_bp, b->bp_all.data(), b->bp_all.size() * 4, hipMemcpyHostToDevice), sdrx_nfm_destroy(b));
    SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&b->d_chan), (size_t)n_ch * sizeof(NfmChan)), sdrx_nfm_destroy(b));
    SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&b->d_bufs), (size_t)n_ch * sizeof(NfmBufs)), sdrx_nfm_destroy(b));
    SDRX_HIP_ELSE(hipHostMalloc(reinterpret_cast<void**>(&b->h_bufs), (size_t)n_ch * sizeof(NfmBufs), hipHostMallocDefault), sdrx_nfm_destroy(b));
    SDRX_HIP_ELSE(hipEventCreateWithFlags(&b->bufs_ev, hipEventDisableTiming), sdrx_nfm_destroy(b));
    SDRX_HIP_ELSE(hipEventRecord(b->bufs_ev, b->core.stream), sdrx_nfm_destroy(b));
    rc = make_front(b);
    if (!rc) rc = upload_fresh_state(b);
    if (rc) { sdrx_nfm_destroy(b); return rc; }
    *out = b;
    return SDRX_OK;
}

int sdrx_nfm_reset(sdrx_nfm_t* b)
{
    if (!b) { set_error("sdrx_nfm_reset: null handle"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    SDRX_HIP(hipStreamSynchronize(b->core.stream));
    // the front has no reset of its own: a fresh one with the same design
    if (b->front) { (void)sdrx_backend_destroy(b->front); b->front = nullptr; }
    int rc = make_front(b); if (rc) return rc;
    return upload_fresh_state(b);
}

// the tail behind a front feed that has just been queued on the handle's stream
static int tail_common(sdrx_nfm* b, const int64_t* n_per_ch)
{
    int64_t bound = 0;
    for (int c = 0; c < b->n_ch; c++) {
        int rc = ensure_capacity(b, c, std::max<int64_t>(n_per_ch[c], 1)); if (rc) return rc;
        // every audio sample after the first two of a stream consumes >= floor(step) inputs
        const int64_t per_out = std::max<int64_t>(1, b->cfg[(size_t)c].in_rate / b->cfg[(size_t)c].audio_rate);
        bound = std::max(bound, std::min<int64_t>(n_per_ch[c], n_per_ch[c] / per_out + 4));
    }
    SDRX_HIP(hipEventSynchronize(b->bufs_ev));            // previous feed's copy has read the table
    for (int c = 0; c < b->n_ch; c++) {
        NfmHost& h = b->ch[(size_t)c];
        const NfmChan& s = b->h_chan[(size_t)c];
        NfmBufs& u = b->h_bufs[c];
        BackendView v;
        int rc = backend_view(b->front, c, &v); if (rc) return rc;
        u.ci = static_cast<const float2*>(v.out); u.n_ptr = v.n_out;
        char* set[2] = { h.hist + (size_t)h.cur * h.hist_set, h.hist + (size_t)(h.cur ^ 1) * h.hist_set };
        size_t o = 0;
        u.mhist = reinterpret_cast<const float*>(set[0] + o); u.mhist_next = reinterpret_cast<float*>(set[1] + o); o += al(NFM_MA * 4);
        u.whist = reinterpret_cast<const float*>(set[0] + o); u.whist_next = reinterpret_cast<float*>(set[1] + o); o += al((size_t)s.D * 4);
        u.xhist = reinterpret_cast<const float*>(set[0] + o); u.xhist_next = reinterpret_cast<float*>(set[1] + o);
        const size_t n = (size_t)h.cap_in + 16, nblk = n / 256 + 1;
        char* p = static_cast<char*>(h.work.p);
        auto take = [&](size_t bytes) { char* r = p; p += al(bytes); return r; };
        u.msq = reinterpret_cast<float*>(take(n * 4)); u.wraw = reinterpret_cast<float*>(take(n * 4)); u.w = reinterpret_cast<float*>(take(n * 4));
        u.x = reinterpret_cast<float*>(take(n * 4)); u.aidx = reinterpret_cast<int*>(take(n * 4));
        u.dterm = reinterpret_cast<double*>(take(n * 8)); u.tot = reinterpret_cast<double*>(take(n * 8));
        u.audio = reinterpret_cast<int16_t*>(take(n * 2));
        u.blk_sum = reinterpret_cast<double*>(take(nblk * 8)); u.blk_peak = reinterpret_cast<float*>(take(nblk * 4));
        u.blk_a = reinterpret_cast<int*>(take(nblk * 4));
    }
    int rc = demod_upload_bufs(b->d_bufs, b->h_bufs, b->n_ch, b->bufs_ev, b->core.stream); if (rc) return rc;
    const unsigned nc = (unsigned)b->n_ch, gp = (nc + PS_CH - 1) / PS_CH, gx = (unsigned)std::max<int64_t>(1, (bound + 255) / 256);
    hipLaunchKernelGGL(nfm_level_kernel, dim3(gx, nc), dim3(256), 0, b->core.stream, b->d_chan, b->d_bufs);
    SDRX_HIP(hipGetLastError());
    hipLaunchKernelGGL(nfm_psum_kernel, dim3(gp), dim3(64), 0, b->core.stream, b->d_chan, b->d_bufs, b->n_ch);
    SDRX_HIP(hipGetLastError());
    hipLaunchKernelGGL(nfm_gate_kernel, dim3(nc), dim3(256), 0, b->core.stream, b->d_chan, b->d_bufs);
    SDRX_HIP(hipGetLastError());
    hipLaunchKernelGGL(nfm_out_kernel, dim3(gx, nc), dim3(256), 0, b->core.stream, b->d_chan, b->d_bufs, b->d_bp);
    SDRX_HIP(hipGetLastError());
    b->core.note_launch("nfm_out_kernel", (int)(gx * nc), 256, (int)((AM_BP_H + 1 + NFM_OUT_WIN) * sizeof(float)));
    hipLaunchKernelGGL(nfm_carry_kernel, dim3(nc), dim3(256), 0, b->core.stream, b->d_chan, b->d_bufs);
    SDRX_HIP(hipGetLastError());
    for (auto& h : b->ch) h.cur ^= 1;
    return SDRX_OK;
}

int sdrx_nfm_feed_dev(sdrx_nfm_t* b, const int16_t* const* d_iq, const int64_t* n_per_ch)
{
    if (!b || !d_iq || !n_per_ch) { set_error("sdrx_nfm_feed_dev: null argument"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    int rc = demod_check_lengths(b->n_ch, n_per_ch, "sdrx_nfm_feed_dev"); if (rc) return rc;
    rc = demod_check_dev_pointers(b->n_ch, d_iq, n_per_ch, "sdrx_nfm_feed_dev"); if (rc) return rc;
    rc = b->core.timer.begin(b->core.stream); if (rc) return rc;
    rc = sdrx_backend_feed_dev(b->front, d_iq, n_per_ch); if (rc) return rc;
    rc = tail_common(b, n_per_ch); if (rc) return rc;
    return b->core.timer.end(b->core.stream);
}

int sdrx_nfm_feed_bank(sdrx_nfm_t* b, sdrx_chan_bank_t* bank)
{
    if (!b || !bank) { set_error("sdrx_nfm_feed_bank: null argument"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    std::vector<const int16_t*> d;                          // the front takes them from the bank itself
    std::vector<int64_t> n;
    int rc = demod_gather_bank(bank, b->n_ch, "sdrx_nfm_feed_bank", d, n); if (rc) return rc;
    rc = demod_check_lengths(b->n_ch, n.data(), "sdrx_nfm_feed_bank"); if (rc) return rc;
    rc = b->core.timer.begin(b->core.stream); if (rc) return rc;
    // the front orders its readers against the bank's stream (sdrx_backend_feed_bank); the tail reads the front's output only
    rc = sdrx_backend_feed_bank(b->front, bank); if (rc) return rc;
    rc = tail_common(b, n.data()); if (rc) return rc;
    return b->core.timer.end(b->core.stream);
}

int sdrx_nfm_feed(sdrx_nfm_t* b, const int16_t* const* iq, const int64_t* n_per_ch)
{
    if (!b || !iq || !n_per_ch) { set_error("sdrx_nfm_feed: null argument"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    std::vector<const int16_t*> d;
    int rc = demod_stage_inputs(b->ch, b->core.stream, iq, n_per_ch, "sdrx_nfm_feed", d); if (rc) return rc;
    rc = sdrx_nfm_feed_dev(b, d.data(), n_per_ch); if (rc) return rc;
    SDRX_HIP(hipStreamSynchronize(b->core.stream));            // the caller's buffers are free again on return
    return SDRX_OK;
}

int64_t sdrx_nfm_read(sdrx_nfm_t* b, int32_t c, int16_t* audio, int64_t cap)
{
    if (!b || c < 0 || c >= b->n_ch || cap < 0 || (cap > 0 && !audio)) { set_error("sdrx_nfm_read: bad argument"); return SDRX_EINVAL; }
    NfmChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    const int64_t n = std::min<int64_t>(s.n, cap);
    if (n == 0) return 0;
    SDRX_HIP(hipMemcpy(audio, b->h_bufs[c].audio, (size_t)n * 2, hipMemcpyDeviceToHost));
    return n;
}

int sdrx_nfm_last_dev(sdrx_nfm_t* b, int32_t c, const int16_t** d_audio, int64_t* n)
{
    if (!b || c < 0 || c >= b->n_ch || !d_audio || !n) { set_error("sdrx_nfm_last_dev: bad argument"); return SDRX_EINVAL; }
    NfmChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    *d_audio = s.n > 0 ? b->h_bufs[c].audio : static_cast<const int16_t*>(b->ch[(size_t)c].work.p);
    *n = s.n;
    return SDRX_OK;
}

int sdrx_nfm_squelch_open(sdrx_nfm_t* b, int32_t c)
{
    if (!b || c < 0 || c >= b->n_ch) { set_error("sdrx_nfm_squelch_open: bad argument"); return SDRX_EINVAL; }
    NfmChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    return s.sq_open;
}

int sdrx_nfm_levels(sdrx_nfm_t* b, int32_t c, double* magsq, double* sum, double* peak, int64_t* count, int reset)
{
    if (!b || c < 0 || c >= b->n_ch) { set_error("sdrx_nfm_levels: bad argument"); return SDRX_EINVAL; }
    NfmChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    if (magsq) *magsq = s.total / (double)NFM_MA;        // m_movingAverage.asDouble()
    if (sum) *sum = s.magsq_sum;
    if (peak) *peak = s.magsq_peak;
    if (count) *count = s.magsq_count;
    if (!reset) return SDRX_OK;                           // getMagSqLevels: sum, peak and count back to 0; the moving average stays
    return demod_zero_levels(b->core, b->d_chan + c, offsetof(NfmChan, magsq_sum), offsetof(NfmChan, magsq_peak), offsetof(NfmChan, magsq_count));
}

int sdrx_nfm_get_design(sdrx_nfm_t* b, int32_t c, int32_t* ntaps_per_phase, float* taps, int32_t taps_cap,
                        float* bandpass_taps, int32_t* nco_inc, float* squelch_level, int32_t* squelch_gate)
{
    if (!b || c < 0 || c >= b->n_ch) { set_error("sdrx_nfm_get_design: bad channel"); return SDRX_EINVAL; }
    int rc = sdrx_backend_get_design(b->front, c, ntaps_per_phase, taps_cap > 0 ? taps : nullptr, taps_cap, nullptr, nco_inc); if (rc) return rc;
    if (bandpass_taps) std::memcpy(bandpass_taps, &b->bp_all[(size_t)b->h_chan[(size_t)c].bp_off], (AM_BP_H + 1) * 4);
    if (squelch_level) *squelch_level = b->h_chan[(size_t)c].level;
    if (squelch_gate) *squelch_gate = b->h_chan[(size_t)c].gate;
    return SDRX_OK;
}

int sdrx_nfm_sync(sdrx_nfm_t* b) { return b ? b->core.sync() : SDRX_EINVAL; }

int sdrx_nfm_set_stream(sdrx_nfm_t* b, void* hip_stream)
{
    if (!b) return SDRX_EINVAL;
    int rc = b->core.set_stream(hip_stream); if (rc) return rc;
    return backend_set_stream(b->front, b->core.stream);      // the front launches on the same stream
}

int sdrx_nfm_get_stream(sdrx_nfm_t* b, void** hip_stream) { return b ? b->core.get_stream(hip_stream) : SDRX_EINVAL; }

int sdrx_nfm_set_timing(sdrx_nfm_t* b, int enabled) { return b ? b->core.set_timing(enabled) : SDRX_EINVAL; }

int sdrx_nfm_get_timing(sdrx_nfm_t* b, double* total_ms, int64_t* feeds, int reset) { return b ? b->core.get_timing(total_ms, feeds, reset) : SDRX_EINVAL; }

int sdrx_nfm_last_launch(const sdrx_nfm_t* b, char* kernel_name, int name_cap, int* grid, int* block, int* lds_bytes) { return b ? b->core.last_launch(kernel_name, name_cap, grid, block, lds_bytes) : SDRX_EINVAL; }

} // extern "C"
