// libsdrx.so: sdrx_ssb_* -- N SSB / DSB demodulators (SSBDemod::feed, plugins/channelrx/demodssb/ssbdemod.cpp:147-285) on one
// device: int16 I/Q at the channelizer's output rate in, qint16 l,r audio and the decimated sideband stream of the spectrum
// sink out.  The front (NCO, Interpolator, fftfilt runSSB / runDSB) is a channel back-end the handle owns and launches on its
// own stream; the tail's kernels are in ssb_kernels.hpp.  Host side: the design products as the constructor,
// applyAudioSampleRate and applySettings(settings, true) derive them (ssbdemod.cpp:46-101, 401-422, 457-533), launches,
// buffer bookkeeping.
#include "sdrx_common.hpp"
#include "ssb_kernels.hpp"
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

struct SsbHost {
    DevBuf work, stage_in;
    char* hist = nullptr;             // two sets of [hn powers | D + 1 delay-line writes]
    size_t hist_set = 0;              // bytes of one set
    int cur = 0;
    int64_t cap_in = 0;
};

constexpr int SSB_BLOCK_MAX = 1024;                 // runDSB hands out 1024 samples at a time, runSSB 512
constexpr size_t al(size_t v) { return (v + 255) & ~(size_t)255; }

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

struct sdrx_ssb {
    HandleCore core;
    int n_ch = 0;
    std::vector<sdrx_ssb_cfg> cfg;
    std::vector<sdrx_backend_cfg> be_cfg;
    sdrx_backend_t* front = nullptr;
    std::vector<SsbHost> ch;
    std::vector<SsbChan> h_chan;   // configuration and the state of a fresh handle
    SsbChan* d_chan = nullptr;
    SsbBufs* d_bufs = nullptr;
    SsbBufs* h_bufs = nullptr;     // pinned: the per-feed table goes to the device in one async copy
    hipEvent_t bufs_ev = nullptr;
};

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

static int ensure_capacity(sdrx_ssb* b, int c, int64_t n_in)
{
    SsbHost& h = b->ch[(size_t)c];
    if (n_in <= h.cap_in) return SDRX_OK;
    int64_t cap = h.cap_in ? h.cap_in : 4096;
    while (cap < n_in) cap *= 2;
    // at most one resampler output per input (step >= 1) plus what the filter held back: fewer than one block.  Nothing
    // here carries state
    const size_t n = (size_t)cap + SSB_BLOCK_MAX + 16, nblk = n / 256 + 1;
    const size_t bytes = 2 * al(n * 4) + 2 * al(n * 8) + al(n * 8) + 2 * al(n * 4) + 2 * al(nblk * 8);
    SDRX_HIP(hipStreamSynchronize(b->core.stream));
    int rc = h.work.reserve(bytes); if (rc) return rc;
    h.cap_in = cap;
    return SDRX_OK;
}

static int upload_fresh_state(sdrx_ssb* b)
{
    SDRX_HIP(hipMemcpyAsync(b->d_chan, b->h_chan.data(), (size_t)b->n_ch * sizeof(SsbChan), hipMemcpyHostToDevice, b->core.stream));
    for (int c = 0; c < b->n_ch; c++) {
        SsbHost& h = b->ch[(size_t)c];
        // moving-average history 0 (resize() then fill(0)); delay line 0 (DoubleBufferFIFO does not clear its array, see sdrx.h)
        SDRX_HIP(hipMemsetAsync(h.hist, 0, 2 * h.hist_set, b->core.stream));
        h.cur = 0;
    }
    SDRX_HIP(hipStreamSynchronize(b->core.stream));
    return SDRX_OK;
}

static int make_front(sdrx_ssb* b)
{
    int rc = sdrx_backend_create(&b->front, b->core.device, b->n_ch, b->be_cfg.data()); if (rc) return rc;
    return backend_set_stream(b->front, b->core.stream);
}

extern "C" {

int sdrx_ssb_destroy(sdrx_ssb_t* b)
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
    b->core.close();
    delete b;
    return SDRX_OK;
}

int sdrx_ssb_create(sdrx_ssb_t** out, int device, int32_t n_ch, const sdrx_ssb_cfg* cfg)
{
    if (!out) { set_error("sdrx_ssb_create: null out"); return SDRX_EINVAL; }
    *out = nullptr;
    int rc = validate(n_ch, cfg); if (rc) return rc;
    sdrx_ssb* b = new (std::nothrow) sdrx_ssb;
    if (!b) return SDRX_ENOMEM;
    rc = b->core.open(device);
    if (rc) { delete b; return rc; }
    b->n_ch = n_ch;
    b->cfg.assign(cfg, cfg + n_ch);
    b->ch.resize((size_t)n_ch); b->h_chan.resize((size_t)n_ch); b->be_cfg.resize((size_t)n_ch);

    for (int c = 0; c < n_ch; c++) {
        const sdrx_ssb_cfg& k = cfg[c];
        const SsbDerived d = derive(k);
        sdrx_backend_cfg& f = b->be_cfg[(size_t)c];
        std::memset(&f, 0, sizeof f);
        f.in_rate = k.in_rate; f.nco_freq = k.nco_freq; f.out_rate = k.audio_rate;
        f.interp_cutoff = d.band * 1.5f;                    // m_interpolator.create(16, m_inputSampleRate, m_Bandwidth * 1.5f, 2.0f)
        f.taps_per_phase = 2.0f;
        f.filt_mode = k.dsb ? 4 : (d.usb ? 2 : 3);
        f.f1 = d.low / (float)(uint32_t)k.audio_rate;      // create_filter(m_LowCutoff / (float) rate, m_Bandwidth / (float) rate)
        f.f2 = k.dsb ? (2.0f * d.band) / (float)(uint32_t)k.audio_rate : d.band / (float)(uint32_t)k.audio_rate;
        SsbChan& s = b->h_chan[(size_t)c];
        std::memset(&s, 0, sizeof s);
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
        SsbHost& h = b->ch[(size_t)c];
        h.hist_set = al((size_t)s.hn * 4) + al((size_t)(s.D + 1) * 8);
        SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&h.hist), 2 * h.hist_set), sdrx_ssb_destroy(b));
    }
    SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&b->d_chan), (size_t)n_ch * sizeof(SsbChan)), sdrx_ssb_destroy(b));
    SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&b->d_bufs), (size_t)n_ch * sizeof(SsbBufs)), sdrx_ssb_destroy(b));
    SDRX_HIP_ELSE(hipHostMalloc(reinterpret_cast<void**>(&b->h_bufs), (size_t)n_ch * sizeof(SsbBufs), hipHostMallocDefault), sdrx_ssb_destroy(b));
    SDRX_HIP_ELSE(hipEventCreateWithFlags(&b->bufs_ev, hipEventDisableTiming), sdrx_ssb_destroy(b));
    SDRX_HIP_ELSE(hipEventRecord(b->bufs_ev, b->core.stream), sdrx_ssb_destroy(b));
    rc = make_front(b);
    if (!rc) rc = upload_fresh_state(b);
    if (rc) { sdrx_ssb_destroy(b); return rc; }
    *out = b;
    return SDRX_OK;
}

int sdrx_ssb_reset(sdrx_ssb_t* b)
{
    if (!b) { set_error("sdrx_ssb_reset: null handle"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    SDRX_HIP(hipStreamSynchronize(b->core.stream));
    // the front has no reset of its own: a fresh one with the same design
    if (b->front) { (void)sdrx_backend_destroy(b->front); b->front = nullptr; }
    int rc = make_front(b); if (rc) return rc;
    return upload_fresh_state(b);
}

// the tail behind a front feed that has just been queued on the handle's stream
static int tail_common(sdrx_ssb* b, const int64_t* n_per_ch)
{
    int64_t bound = 0;
    for (int c = 0; c < b->n_ch; c++) {
        int rc = ensure_capacity(b, c, std::max<int64_t>(n_per_ch[c], 1)); if (rc) return rc;
        // every resampler output after the first two of a stream consumes >= floor(step) inputs; the filter adds what it held back
        const int64_t per_out = std::max<int64_t>(1, b->cfg[(size_t)c].in_rate / b->cfg[(size_t)c].audio_rate);
        bound = std::max(bound, std::min<int64_t>(n_per_ch[c], n_per_ch[c] / per_out + 4) + SSB_BLOCK_MAX);
    }
    SDRX_HIP(hipEventSynchronize(b->bufs_ev));            // previous feed's copy has read the table
    for (int c = 0; c < b->n_ch; c++) {
        SsbHost& h = b->ch[(size_t)c];
        const SsbChan& s = b->h_chan[(size_t)c];
        SsbBufs& u = b->h_bufs[c];
        BackendView v;
        int rc = backend_view(b->front, c, &v); if (rc) return rc;
        u.s = static_cast<const float2*>(v.out); u.n_ptr = v.n_out;
        char* set[2] = { h.hist + (size_t)h.cur * h.hist_set, h.hist + (size_t)(h.cur ^ 1) * h.hist_set };
        const size_t o = al((size_t)s.hn * 4);
        u.phist = reinterpret_cast<const float*>(set[0]); u.phist_next = reinterpret_cast<float*>(set[1]);
        u.whist = reinterpret_cast<const float2*>(set[0] + o); u.whist_next = reinterpret_cast<float2*>(set[1] + o);
        const size_t n = (size_t)h.cap_in + SSB_BLOCK_MAX + 16, nblk = n / 256 + 1;
        char* p = static_cast<char*>(h.work.p);
        auto take = [&](size_t bytes) { char* r = p; p += al(bytes); return r; };
        u.pw = reinterpret_cast<float*>(take(n * 4)); u.sv = reinterpret_cast<float*>(take(n * 4));
        u.dterm = reinterpret_cast<double*>(take(n * 8)); u.tot = reinterpret_cast<double*>(take(n * 8));
        u.w = reinterpret_cast<float2*>(take(n * 8));
        u.audio = reinterpret_cast<int16_t*>(take(n * 4)); u.spec = reinterpret_cast<int16_t*>(take(n * 4));
        u.blk_sum = reinterpret_cast<double*>(take(nblk * 8)); u.blk_peak = reinterpret_cast<double*>(take(nblk * 8));
    }
    int rc = demod_upload_bufs(b->d_bufs, b->h_bufs, b->n_ch, b->bufs_ev, b->core.stream); if (rc) return rc;
    const unsigned nc = (unsigned)b->n_ch, gp = (nc + PS_CH - 1) / PS_CH, gx = (unsigned)std::max<int64_t>(1, (bound + 255) / 256);
    hipLaunchKernelGGL(ssb_level_kernel, dim3(gx, nc), dim3(256), 0, b->core.stream, b->d_chan, b->d_bufs);
    SDRX_HIP(hipGetLastError());
    hipLaunchKernelGGL(ssb_psum_kernel, dim3(gp), dim3(64), 0, b->core.stream, b->d_chan, b->d_bufs, b->n_ch);
    SDRX_HIP(hipGetLastError());
    hipLaunchKernelGGL(ssb_gate_kernel, dim3(nc), dim3(256), 0, b->core.stream, b->d_chan, b->d_bufs);
    SDRX_HIP(hipGetLastError());
    hipLaunchKernelGGL(ssb_out_kernel, dim3(gx, nc), dim3(256), 0, b->core.stream, b->d_chan, b->d_bufs);
    SDRX_HIP(hipGetLastError());
    b->core.note_launch("ssb_out_kernel", (int)(gx * nc), 256, 0);
    hipLaunchKernelGGL(ssb_carry_kernel, dim3(nc), dim3(256), 0, b->core.stream, b->d_chan, b->d_bufs);
    SDRX_HIP(hipGetLastError());
    for (auto& h : b->ch) h.cur ^= 1;
    return SDRX_OK;
}

int sdrx_ssb_feed_dev(sdrx_ssb_t* b, const int16_t* const* d_iq, const int64_t* n_per_ch)
{
    if (!b || !d_iq || !n_per_ch) { set_error("sdrx_ssb_feed_dev: null argument"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    int rc = demod_check_lengths(b->n_ch, n_per_ch, "sdrx_ssb_feed_dev"); if (rc) return rc;
    rc = demod_check_dev_pointers(b->n_ch, d_iq, n_per_ch, "sdrx_ssb_feed_dev"); if (rc) return rc;
    rc = b->core.timer.begin(b->core.stream); if (rc) return rc;
    rc = sdrx_backend_feed_dev(b->front, d_iq, n_per_ch); if (rc) return rc;
    rc = tail_common(b, n_per_ch); if (rc) return rc;
    return b->core.timer.end(b->core.stream);
}

int sdrx_ssb_feed_bank(sdrx_ssb_t* b, sdrx_chan_bank_t* bank)
{
    if (!b || !bank) { set_error("sdrx_ssb_feed_bank: null argument"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    std::vector<const int16_t*> d;                          // the front takes them from the bank itself
    std::vector<int64_t> n;
    int rc = demod_gather_bank(bank, b->n_ch, "sdrx_ssb_feed_bank", d, n); if (rc) return rc;
    rc = demod_check_lengths(b->n_ch, n.data(), "sdrx_ssb_feed_bank"); if (rc) return rc;
    rc = b->core.timer.begin(b->core.stream); if (rc) return rc;
    // the front orders its readers against the bank's stream (sdrx_backend_feed_bank); the tail reads the front's output only
    rc = sdrx_backend_feed_bank(b->front, bank); if (rc) return rc;
    rc = tail_common(b, n.data()); if (rc) return rc;
    return b->core.timer.end(b->core.stream);
}

int sdrx_ssb_feed(sdrx_ssb_t* b, const int16_t* const* iq, const int64_t* n_per_ch)
{
    if (!b || !iq || !n_per_ch) { set_error("sdrx_ssb_feed: null argument"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(b->core.device));
    std::vector<const int16_t*> d;
    int rc = demod_stage_inputs(b->ch, b->core.stream, iq, n_per_ch, "sdrx_ssb_feed", d); if (rc) return rc;
    rc = sdrx_ssb_feed_dev(b, d.data(), n_per_ch); if (rc) return rc;
    SDRX_HIP(hipStreamSynchronize(b->core.stream));            // the caller's buffers are free again on return
    return SDRX_OK;
}

int64_t sdrx_ssb_read(sdrx_ssb_t* b, int32_t c, int16_t* audio_lr, int64_t cap)
{
    if (!b || c < 0 || c >= b->n_ch || cap < 0 || (cap > 0 && !audio_lr)) { set_error("sdrx_ssb_read: bad argument"); return SDRX_EINVAL; }
    SsbChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    const int64_t n = std::min<int64_t>(s.n, cap);
    if (n == 0) return 0;
    SDRX_HIP(hipMemcpy(audio_lr, b->h_bufs[c].audio, (size_t)n * 4, hipMemcpyDeviceToHost));
    return n;
}

int sdrx_ssb_last_dev(sdrx_ssb_t* b, int32_t c, const int16_t** d_audio_lr, int64_t* n)
{
    if (!b || c < 0 || c >= b->n_ch || !d_audio_lr || !n) { set_error("sdrx_ssb_last_dev: bad argument"); return SDRX_EINVAL; }
    SsbChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    *d_audio_lr = s.n > 0 ? b->h_bufs[c].audio : static_cast<const int16_t*>(b->ch[(size_t)c].work.p);
    *n = s.n;
    return SDRX_OK;
}

int64_t sdrx_ssb_read_spectrum(sdrx_ssb_t* b, int32_t c, int16_t* samples_iq, int64_t cap)
{
    if (!b || c < 0 || c >= b->n_ch || cap < 0 || (cap > 0 && !samples_iq)) { set_error("sdrx_ssb_read_spectrum: bad argument"); return SDRX_EINVAL; }
    SsbChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    const int64_t n = std::min<int64_t>(s.n_spec, cap);
    if (n == 0) return 0;
    SDRX_HIP(hipMemcpy(samples_iq, b->h_bufs[c].spec, (size_t)n * 4, hipMemcpyDeviceToHost));
    return n;
}

int sdrx_ssb_spectrum_last_dev(sdrx_ssb_t* b, int32_t c, const int16_t** d_samples_iq, int64_t* n)
{
    if (!b || c < 0 || c >= b->n_ch || !d_samples_iq || !n) { set_error("sdrx_ssb_spectrum_last_dev: bad argument"); return SDRX_EINVAL; }
    SsbChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    *d_samples_iq = s.n_spec > 0 ? b->h_bufs[c].spec : static_cast<const int16_t*>(b->ch[(size_t)c].work.p);
    *n = s.n_spec;
    return SDRX_OK;
}

int sdrx_ssb_audio_active(sdrx_ssb_t* b, int32_t c)
{
    if (!b || c < 0 || c >= b->n_ch) { set_error("sdrx_ssb_audio_active: bad argument"); return SDRX_EINVAL; }
    SsbChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    return s.audio_active;
}

int sdrx_ssb_levels(sdrx_ssb_t* b, int32_t c, double* magsq, double* sum, double* peak, int64_t* count, int reset)
{
    if (!b || c < 0 || c >= b->n_ch) { set_error("sdrx_ssb_levels: bad argument"); return SDRX_EINVAL; }
    SsbChan s;
    int rc = demod_fetch_state(b->core, b->d_chan, c, &s); if (rc) return rc;
    if (magsq) *magsq = s.magsq;
    if (sum) *sum = s.magsq_sum;
    if (peak) *peak = s.magsq_peak;
    if (count) *count = s.magsq_count;
    if (!reset) return SDRX_OK;                           // getMagSqLevels: sum, peak and count back to 0
    return demod_zero_levels(b->core, b->d_chan + c, offsetof(SsbChan, magsq_sum), offsetof(SsbChan, magsq_peak), offsetof(SsbChan, magsq_count));
}

int sdrx_ssb_get_design(sdrx_ssb_t* b, int32_t c, int32_t* ntaps_per_phase, float* taps, int32_t taps_cap, float* filter_iq,
                        int32_t* nco_inc, int32_t* agc_nb_samples, int32_t* agc_gate, double* agc_threshold, float* volume)
{
    if (!b || c < 0 || c >= b->n_ch) { set_error("sdrx_ssb_get_design: bad channel"); return SDRX_EINVAL; }
    int rc = sdrx_backend_get_design(b->front, c, ntaps_per_phase, taps_cap > 0 ? taps : nullptr, taps_cap, filter_iq, nco_inc); if (rc) return rc;
    const SsbChan& s = b->h_chan[(size_t)c];
    if (agc_nb_samples) *agc_nb_samples = s.hn;
    if (agc_gate) *agc_gate = s.gate;
    if (agc_threshold) *agc_threshold = s.threshold;
    if (volume) *volume = s.volume;
    return SDRX_OK;
}

int sdrx_ssb_sync(sdrx_ssb_t* b) { return b ? b->core.sync() : SDRX_EINVAL; }

int sdrx_ssb_set_stream(sdrx_ssb_t* b, void* hip_stream)
{
    if (!b) return SDRX_EINVAL;
    int rc = b->core.set_stream(hip_stream); if (rc) return rc;
    return backend_set_stream(b->front, b->core.stream);      // the front launches on the same stream
}

int sdrx_ssb_get_stream(sdrx_ssb_t* b, void** hip_stream) { return b ? b->core.get_stream(hip_stream) : SDRX_EINVAL; }

int sdrx_ssb_set_timing(sdrx_ssb_t* b, int enabled) { return b ? b->core.set_timing(enabled) : SDRX_EINVAL; }

int sdrx_ssb_get_timing(sdrx_ssb_t* b, double* total_ms, int64_t* feeds, int reset) { return b ? b->core.get_timing(total_ms, feeds, reset) : SDRX_EINVAL; }

int sdrx_ssb_last_launch(const sdrx_ssb_t* b, char* kernel_name, int name_cap, int* grid, int* block, int* lds_bytes) { return b ? b->core.last_launch(kernel_name, name_cap, grid, block, lds_bytes) : SDRX_EINVAL; }

} // extern "C"
