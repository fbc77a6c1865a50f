// libsdrx.so: sdrx_spectrum_* -- SpectrumVis (sdrgui/dsp/spectrumvis.{h,cpp}, v4.0.6, kissfft engine) on the device: the
// spectrum / waterfall sink of a device set.  Every frame the reference would hand to GLSpectrum::newSpectrum is queued on
// the device until read.  Kernels: spectrum_kernel.hpp.  Host side: the 4096-entry buffer's fill, the averaging index,
// the window and twiddle tables (built here with the reference's formulas and precision) and the frame queue.
#include "sdrx_common.hpp"
#include "spectrum_kernel.hpp"
#include <cmath>
#include <complex>
#include <cstring>
#include <new>
#include <vector>

using namespace sdrx;
using namespace sdrx_spec;

namespace {

// FFTWindow (sdrbase/dsp/fftwindow.{h,cpp}): Real arguments, double arithmetic, stored as float
constexpr double PI_D = 3.14159265358979323846;

float window_value(int fn, float n, float i)
{
    switch (fn) {
    case 0: return (float)((2.0 / (n - 1.0)) * ((n - 1.0) / 2.0 - std::fabs(i - (n - 1.0) / 2.0)) * 2.0);              // Bartlett
    case 1: return (float)((0.35875 - 0.48829 * std::cos((2.0 * PI_D * i) / n) + 0.14128 * std::cos((4.0 * PI_D * i) / n)
                            - 0.01168 * std::cos((6.0 * PI_D * i) / n)) * 2.79);                                       // BlackmanHarris
    case 2: return (float)(1.0 - 1.93 * std::cos((2.0 * PI_D * i) / n) + 1.29 * std::cos((4.0 * PI_D * i) / n)
                           - 0.388 * std::cos((6.0 * PI_D * i) / n) + 0.03222 * std::cos((8.0 * PI_D * i) / n));      // Flattop
    case 3: return (float)((0.54 - 0.46 * std::cos((2.0 * PI_D * i) / n)) * 1.855);                                  // Hamming
    case 4: return (float)((0.5 - 0.5 * std::cos((2.0 * PI_D * i) / n)) * 2.0);                                      // Hanning
    default: return 1.0f;                                                                                             // Rectangle
    }
}

// 2 * ov < N, N a power of two in [64, 4096] after handleConfigure's clamps (spectrumvis.cpp:272-300)
int validate(const sdrx_spectrum_cfg* c, const char* who, int* n_out, int* ov_out)
{
    if (!c) { set_error(std::string(who) + ": null cfg"); return SDRX_EINVAL; }
    int n = c->fft_size < 64 ? 64 : c->fft_size > BUF ? BUF : c->fft_size;
    const int pct = c->overlap_percent < 0 ? 0 : c->overlap_percent > 100 ? 100 : c->overlap_percent;
    if (n & (n - 1)) { set_error(std::string(who) + ": fft_size must be a power of two (kissfft radix 4/2 only)"); return SDRX_EINVAL; }
    const int ov = n * pct / 100;
    if (2 * ov >= n) {
        set_error(std::string(who) + ": overlap must stay below 50 % (2*overlap >= fft_size: the reference loops forever at 50 % and writes past its buffer above)");
        return SDRX_EINVAL;
    }
    if (c->window < SDRX_SPECTRUM_BARTLETT || c->window > SDRX_SPECTRUM_RECTANGLE) { set_error(std::string(who) + ": bad window"); return SDRX_EINVAL; }
    if (c->avg_mode < SDRX_SPECTRUM_AVG_NONE || c->avg_mode > SDRX_SPECTRUM_AVG_FIXED) { set_error(std::string(who) + ": bad avg_mode"); return SDRX_EINVAL; }
    if (!std::isfinite(c->scalef) || c->scalef == 0.0f) { set_error(std::string(who) + ": scalef must be finite and non-zero"); return SDRX_EINVAL; }
    *n_out = n; *ov_out = ov;
    return SDRX_OK;
}

} // namespace

struct sdrx_spectrum {
    HandleCore core;
    // configuration (handleConfigure)
    sdrx_spectrum_cfg cfg{};
    int n = 0, log2n = 0, ov = 0, r = 0, nst = 0, last_radix = 4, mode = 0;   // mode: 0 none, 1 moving, 2 fixed (depth > 1)
    unsigned depth = 0;
    float mult = 0, ofs = 0, powdiv = 1;
    std::vector<float> win;
    // running state
    int fill = 0;                  // m_fftBufferFill
    unsigned avg_idx = 0;          // m_avgIndex of the active average
    bool stale_zero = true;        // B outside [ov, R) is all zero (nothing fed since the last reset)
    bool dirty = false;            // a sample has been written to B since the last reset
    float2* d_buf[2] = { nullptr, nullptr };
    int cur = 0;
    float* d_win = nullptr;
    float2* d_tw = nullptr;
    double* d_avg_data = nullptr;  // moving: depth x N, fixed: unused
    double* d_avg_sum = nullptr;   // N
    size_t avg_data_cap = 0;
    DevBuf d_in, d_raw;
    // frame queue: q_count frames of N floats from frame q_head on
    float* d_q = nullptr;
    size_t q_floats = 0;
    long q_head = 0, q_count = 0;
};

static int apply_config(sdrx_spectrum* h, const sdrx_spectrum_cfg* c, int n, int ov)
{
    h->cfg = *c;
    h->n = n; h->ov = ov; h->r = n - ov;
    h->log2n = 0; while ((1 << h->log2n) < n) h->log2n++;
    h->nst = (h->log2n + 1) / 2; h->last_radix = (h->log2n & 1) ? 2 : 4;
    h->depth = c->avg_nb;
    h->mode = (c->avg_mode == SDRX_SPECTRUM_AVG_NONE || c->avg_nb <= 1) ? 0 : c->avg_mode;
    h->mult = 10.0f / log2f(10.0f);                      // SpectrumVis::m_mult
    h->ofs = 20.0f * log10f(1.0f / (float)n);            // m_ofs
    h->powdiv = (float)(n * n);                          // m_powFFTDiv
    h->fill = ov;
    h->avg_idx = 0;
    if (h->dirty) h->stale_zero = false;                 // old samples may now sit in the stale ranges
    h->win.resize((size_t)n);
    for (int i = 0; i < n; i++) h->win[(size_t)i] = window_value(c->window, (float)n, (float)i);
    // kissfft_utils::traits::fill_twiddles: phinc = -2 * acos(-1.f) / nfft, exp(complex<float>(0, i * phinc)), all float
    std::vector<float2> tw((size_t)n);
    const float phinc = -2 * std::acos((float)-1) / n;
    for (int i = 0; i < n; i++) {
        const std::complex<float> t = std::exp(std::complex<float>(0, i * phinc));
        tw[(size_t)i] = make_float2(t.real(), t.imag());
    }
    SDRX_HIP(hipMemcpyAsync(h->d_win, h->win.data(), sizeof(float) * (size_t)n, hipMemcpyHostToDevice, h->core.stream));
    SDRX_HIP(hipMemcpyAsync(h->d_tw, tw.data(), sizeof(float2) * (size_t)n, hipMemcpyHostToDevice, h->core.stream));
    // MovingAverage2D::resize / FixedAverage2D::resize: zeroed state, index 0
    const size_t want = h->mode == 1 ? (size_t)n * h->depth : 0;
    if (want > h->avg_data_cap) {
        SDRX_HIP(hipStreamSynchronize(h->core.stream));
        if (h->d_avg_data) { (void)hipFree(h->d_avg_data); h->d_avg_data = nullptr; h->avg_data_cap = 0; }
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->d_avg_data), want * sizeof(double));
        if (e != hipSuccess) { h->d_avg_data = nullptr; set_error("sdrx_spectrum: averaging state does not fit (fft_size x avg_nb doubles)"); return SDRX_ENOMEM; }
        h->avg_data_cap = want;
    }
    if (want) SDRX_HIP(hipMemsetAsync(h->d_avg_data, 0, want * sizeof(double), h->core.stream));
    SDRX_HIP(hipMemsetAsync(h->d_avg_sum, 0, sizeof(double) * BUF, h->core.stream));
    SDRX_HIP(hipStreamSynchronize(h->core.stream));           // the host tables above are released on return
    return SDRX_OK;
}

// room for `more` frames behind the queued ones (the queue holds frames of the current N only: configure refuses to change N
// while frames are queued)
static int queue_reserve(sdrx_spectrum* h, long more)
{
    if (h->q_count == 0) h->q_head = 0;
    if ((size_t)(h->q_head + h->q_count + more) * (size_t)h->n <= h->q_floats) return SDRX_OK;
    size_t cap = h->q_floats ? h->q_floats : (size_t)64 * BUF;
    while (cap < (size_t)(h->q_count + more) * (size_t)h->n) cap *= 2;
    float* nq = nullptr;
    SDRX_HIP(hipMalloc(reinterpret_cast<void**>(&nq), sizeof(float) * cap));
    hipError_t e = hipSuccess;
    if (h->q_count) e = hipMemcpyAsync(nq, h->d_q + h->q_head * h->n, sizeof(float) * (size_t)h->q_count * (size_t)h->n, hipMemcpyDeviceToDevice, h->core.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->core.stream);
    if (e != hipSuccess) { (void)hipFree(nq); return hip_fail(e, "sdrx_spectrum queue grow", __FILE__, __LINE__); }
    if (h->d_q) (void)hipFree(h->d_q);
    h->d_q = nq; h->q_floats = cap; h->q_head = 0;
    return SDRX_OK;
}

static int feed_device(sdrx_spectrum* h, const uint32_t* d_in, long n_in, int positive_only)
{
    if (n_in <= 0) return SDRX_OK;
    const int n = h->n, ov = h->ov, r = h->r, s = r - ov;
    const long need0 = r - h->fill;
    long frames = 0, consumed = 0;
    if (n_in >= need0) { frames = 1 + (n_in - need0) / s; consumed = need0 + (frames - 1) * s; }
    const int fill_f = frames ? ov : h->fill;
    const int rem = (int)(n_in - consumed);
    if (frames > 0x7fffffffL) { set_error("sdrx_spectrum_feed: too many frames in one feed"); return SDRX_EINVAL; }

    // frames the feed emits (FixedAverage2D::nextAverage returns true every depth-th frame)
    long emitted = frames;
    if (h->mode == 2) emitted = ((long)h->avg_idx + frames) / h->depth;

    Geom g{};
    g.n = n; g.log2n = h->log2n; g.ov = ov; g.r = r; g.s = s; g.fill0 = h->fill;
    g.nst = h->nst; g.last_radix = h->last_radix;
    g.fpb = n >= MIN_LDS_CPLX ? 1 : MIN_LDS_CPLX / n;
    g.frames = (int)frames; g.stale_zero = h->stale_zero ? 1 : 0; g.scalef = h->cfg.scalef;
    Post o{ h->cfg.linear ? 1 : 0, positive_only ? 1 : 0, h->mult, h->ofs, h->powdiv };

    int rc = h->core.timer.begin(h->core.stream); if (rc) return rc;
    if (frames > 0) {
        rc = queue_reserve(h, emitted); if (rc) return rc;
        float* qtail = h->d_q + (h->q_head + h->q_count) * n;
        float* dst = qtail;
        if (h->mode) {
            rc = h->d_raw.reserve(sizeof(float) * (size_t)frames * (size_t)n); if (rc) return rc;
            dst = static_cast<float*>(h->d_raw.p);
        }
        const unsigned grid = (unsigned)((frames + g.fpb - 1) / g.fpb);
        const int lds = (int)sizeof(float2) * g.fpb * n;
        hipLaunchKernelGGL(spectrum_fft_kernel, dim3(grid), dim3(NT), lds, h->core.stream,
                           d_in, h->d_buf[h->cur], h->d_win, h->d_tw, dst, g, o, h->mode ? 1 : 0);
        SDRX_HIP(hipGetLastError());
        h->core.note_launch("spectrum_fft_kernel", (int)grid, NT, lds);
        if (h->mode) {
            Avg a{ h->mode, h->depth, h->avg_idx, (int)frames };
            hipLaunchKernelGGL(spectrum_avg_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, h->core.stream,
                               static_cast<const float*>(h->d_raw.p), h->d_avg_data, h->d_avg_sum, qtail, n, a, o);
            SDRX_HIP(hipGetLastError());
            h->avg_idx = (unsigned)(((unsigned long)h->avg_idx + (unsigned long)frames) % h->depth);   // nextAverage() per frame
        }
    }
    hipLaunchKernelGGL(spectrum_buf_kernel, dim3(BUF / NT), dim3(NT), 0, h->core.stream,
                       d_in, h->d_buf[h->cur], h->d_buf[h->cur ^ 1], g, consumed, fill_f, rem);
    SDRX_HIP(hipGetLastError());
    rc = h->core.timer.end(h->core.stream); if (rc) return rc;
    h->cur ^= 1;
    h->fill = fill_f + rem;
    h->q_count += emitted;
    h->dirty = true;
    return SDRX_OK;
}

extern "C" {

int sdrx_spectrum_create(sdrx_spectrum_t** out, int device, const sdrx_spectrum_cfg* cfg)
{
    if (!out) { set_error("sdrx_spectrum_create: null out"); return SDRX_EINVAL; }
    *out = nullptr;
    int n = 0, ov = 0;
    int rc = validate(cfg, "sdrx_spectrum_create", &n, &ov); if (rc) return rc;
    sdrx_spectrum* h = new (std::nothrow) sdrx_spectrum;
    if (!h) return SDRX_ENOMEM;
    rc = h->core.open(device);
    if (rc) { delete h; return rc; }
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->d_buf[0]), sizeof(float2) * BUF);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->d_buf[1]), sizeof(float2) * BUF);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->d_win), sizeof(float) * BUF);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->d_tw), sizeof(float2) * BUF);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->d_avg_sum), sizeof(double) * BUF);
    if (e != hipSuccess) { sdrx_spectrum_destroy(h); return hip_fail(e, "sdrx_spectrum_create", __FILE__, __LINE__); }
    rc = apply_config(h, cfg, n, ov);
    if (!rc) rc = sdrx_spectrum_reset(h);
    if (rc) { sdrx_spectrum_destroy(h); return rc; }
    *out = h;
    return SDRX_OK;
}

int sdrx_spectrum_destroy(sdrx_spectrum_t* h)
{
    if (!h) return SDRX_OK;
    (void)hipSetDevice(h->core.device);
    if (h->core.stream) (void)hipStreamSynchronize(h->core.stream);
    for (int i = 0; i < 2; i++) if (h->d_buf[i]) (void)hipFree(h->d_buf[i]);
    if (h->d_win) (void)hipFree(h->d_win);
    if (h->d_tw) (void)hipFree(h->d_tw);
    if (h->d_avg_data) (void)hipFree(h->d_avg_data);
    if (h->d_avg_sum) (void)hipFree(h->d_avg_sum);
    if (h->d_q) (void)hipFree(h->d_q);
    h->d_in.release(); h->d_raw.release();
    h->core.close();
    delete h;
    return SDRX_OK;
}

int sdrx_spectrum_reset(sdrx_spectrum_t* h)
{
    if (!h) return SDRX_EINVAL;
    SDRX_HIP(hipSetDevice(h->core.device));
    for (int i = 0; i < 2; i++) SDRX_HIP(hipMemsetAsync(h->d_buf[i], 0, sizeof(float2) * BUF, h->core.stream));
    h->dirty = false; h->stale_zero = true;
    h->q_head = h->q_count = 0;
    const sdrx_spectrum_cfg c = h->cfg;
    return apply_config(h, &c, h->n, h->ov);
}

int sdrx_spectrum_configure(sdrx_spectrum_t* h, const sdrx_spectrum_cfg* cfg)
{
    if (!h) { set_error("sdrx_spectrum_configure: null handle"); return SDRX_EINVAL; }
    int n = 0, ov = 0;
    int rc = validate(cfg, "sdrx_spectrum_configure", &n, &ov); if (rc) return rc;
    if (n != h->n && h->q_count) { set_error("sdrx_spectrum_configure: read or skip the queued frames before changing fft_size"); return SDRX_ESTATE; }
    SDRX_HIP(hipSetDevice(h->core.device));
    return apply_config(h, cfg, n, ov);
}

int sdrx_spectrum_feed_dev(sdrx_spectrum_t* h, const int16_t* d_iq, int64_t n_cplx, int positive_only)
{
    if (!h || n_cplx < 0 || (n_cplx > 0 && !d_iq)) { set_error("sdrx_spectrum_feed_dev: bad argument"); return SDRX_EINVAL; }
    if (reinterpret_cast<uintptr_t>(d_iq) & 3u) { set_error("sdrx_spectrum_feed_dev: 4-byte alignment"); return SDRX_EINVAL; }
    SDRX_HIP(hipSetDevice(h->core.device));
    return feed_device(h, reinterpret_cast<const uint32_t*>(d_iq), (long)n_cplx, positive_only);
}

int sdrx_spectrum_feed(sdrx_spectrum_t* h, const int16_t* iq, int64_t n_cplx, int positive_only)
{
    if (!h || n_cplx < 0 || (n_cplx > 0 && !iq)) { set_error("sdrx_spectrum_feed: bad argument"); return SDRX_EINVAL; }
    if (n_cplx == 0) return SDRX_OK;
    SDRX_HIP(hipSetDevice(h->core.device));
    int rc = h->d_in.reserve((size_t)n_cplx * 4); if (rc) return rc;
    SDRX_HIP(hipMemcpyAsync(h->d_in.p, iq, (size_t)n_cplx * 4, hipMemcpyHostToDevice, h->core.stream));
    rc = feed_device(h, static_cast<const uint32_t*>(h->d_in.p), (long)n_cplx, positive_only); if (rc) return rc;
    SDRX_HIP(hipStreamSynchronize(h->core.stream));
    return SDRX_OK;
}

int64_t sdrx_spectrum_available(sdrx_spectrum_t* h)
{
    if (!h) return SDRX_EINVAL;
    return h->q_count;
}

int64_t sdrx_spectrum_read(sdrx_spectrum_t* h, float* out, int64_t max_frames)
{
    if (!h || max_frames < 0 || (max_frames > 0 && !out)) { set_error("sdrx_spectrum_read: bad argument"); return SDRX_EINVAL; }
    const long k = max_frames < h->q_count ? (long)max_frames : h->q_count;
    if (k == 0) return 0;
    SDRX_HIP(hipSetDevice(h->core.device));
    SDRX_HIP(hipMemcpyAsync(out, h->d_q + h->q_head * h->n, sizeof(float) * (size_t)k * (size_t)h->n, hipMemcpyDeviceToHost, h->core.stream));
    SDRX_HIP(hipStreamSynchronize(h->core.stream));
    h->q_head += k; h->q_count -= k;
    if (!h->q_count) h->q_head = 0;
    return k;
}

int64_t sdrx_spectrum_skip(sdrx_spectrum_t* h, int64_t n)
{
    if (!h) return SDRX_EINVAL;
    const long k = (n < 0 || n > h->q_count) ? h->q_count : (long)n;
    h->q_head += k; h->q_count -= k;
    if (!h->q_count) h->q_head = 0;
    return k;
}

int sdrx_spectrum_window(const sdrx_spectrum_t* h, float* out, int32_t cap)
{
    if (!h || cap < 0 || (cap > 0 && !out)) { set_error("sdrx_spectrum_window: bad argument"); return SDRX_EINVAL; }
    const int k = cap < h->n ? cap : h->n;
    if (k) std::memcpy(out, h->win.data(), sizeof(float) * (size_t)k);
    return h->n;
}

int sdrx_spectrum_sync(sdrx_spectrum_t* h) { return h ? h->core.sync() : SDRX_EINVAL; }

int sdrx_spectrum_set_stream(sdrx_spectrum_t* h, void* hip_stream) { return h ? h->core.set_stream(hip_stream) : SDRX_EINVAL; }

int sdrx_spectrum_get_stream(sdrx_spectrum_t* h, void** hip_stream) { return h ? h->core.get_stream(hip_stream) : SDRX_EINVAL; }

int sdrx_spectrum_set_timing(sdrx_spectrum_t* h, int enabled) { return h ? h->core.set_timing(enabled) : SDRX_EINVAL; }

int sdrx_spectrum_get_timing(sdrx_spectrum_t* h, double* total_ms, int64_t* feeds, int reset) { return h ? h->core.get_timing(total_ms, feeds, reset) : SDRX_EINVAL; }

int sdrx_spectrum_last_launch(const sdrx_spectrum_t* h, char* kernel_name, int name_cap, int* grid, int* block, int* lds_bytes) { return h ? h->core.last_launch(kernel_name, name_cap, grid, block, lds_bytes) : SDRX_EINVAL; }

} // extern "C"
