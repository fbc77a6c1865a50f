// libsdrx.so: sdrx_atv_* -- N ATV demodulators (ATVDemod::feed, plugins/channelrx/demodatv/atvdemod.cpp:167-444) on one device:
// int16 I/Q at the channelizer's output rate in; the frames the screen was asked to render, the screen as it stands, the scope
// stream and the state out.  The front is a channel back-end in bypass that the handle owns and launches on its own stream: the
// NCO mix (none at offset 0, as the reference skips it).  The tail's kernels are in atv_kernels.hpp -- the "decimator" as a FIR,
// the FFT filter, the discriminators, the walk -- the per-sample step and the design integers in atv_scan.hpp.  Host side:
// validate, the designs of m_interpolator's phase-0 row and of create_asym_filter, the two layouts, the screens and the filters'
// carried blocks, and the launches; the rest is demod_bank.hpp's.
#include "sdrx_common.hpp"
#include "atv_kernels.hpp"
#include "demod_bank.hpp"
#include "backend_design.hpp"
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

using namespace sdrx;

namespace {

int design_of(const sdrx_atv_cfg& k, AtvDesign& d)
{
    return atv_design(k.in_rate, k.modulation, k.standard, k.n_lines, k.line_duration, k.top_duration, k.frames_per_s, k.level_synchro_top,
                      k.level_black, k.fm_deviation, k.hsync, k.vsync, k.invert_video, k.scope, d);
}

} // namespace

struct AtvFamily : DemodDefaults {
    using Handle = sdrx_atv;
    using Cfg = sdrx_atv_cfg;
    using Chan = AtvChan;
    using Bufs = AtvBufs;
    static constexpr const char* name = "sdrx_atv";
    static constexpr const float2* AtvBufs::* input = &AtvBufs::x;

    static int validate(int32_t n_ch, const sdrx_atv_cfg* cfg)
    {
        if (n_ch <= 0 || !cfg) { set_error("sdrx_atv_create: bad argument"); return SDRX_EINVAL; }
        for (int c = 0; c < n_ch; c++) {
            AtvDesign d;
            const int e = design_of(cfg[c], d);
            const char* text = e ? atv_design_error(e) : nullptr;
            if (!text && cfg[c].frames_cap < 1) text = "frames_cap < 1";
            if (!text && (size_t)d.rows * (size_t)d.cols * (size_t)cfg[c].frames_cap > ((size_t)1 << 30)) text = "frames_cap snapshots of the screen exceed 1 GiB";
            if (!text && (cfg[c].fft_filtering || cfg[c].decimator_enable) && !(cfg[c].rf_bw > 0.0f && cfg[c].rf_bw < 1.0e9f))
                text = "bad rf_bw (the decimator and the FFT filter are designed from it)";
            if (!text && cfg[c].fft_filtering && !(cfg[c].rf_opp_bw >= 0.0f && cfg[c].rf_opp_bw < 1.0e9f)) text = "bad rf_opp_bw";
            if (text) { set_error("sdrx_atv_create: channel " + std::to_string(c) + ": " + text); return SDRX_EINVAL; }
        }
        return SDRX_OK;
    }

    static void design(int, const sdrx_atv_cfg& k, sdrx_backend_cfg& f, AtvChan& s, float*)
    {
        f.in_rate = k.in_rate; f.nco_freq = k.nco_freq; f.out_rate = k.in_rate;     // bypass: one output per input
        f.interp_cutoff = k.in_rate / 2.2f; f.taps_per_phase = 4.5f;                // a design the bypass never runs
        (void)design_of(k, s.d);
        s.decim = k.decimator_enable != 0; s.filt = k.fft_filtering != 0;
        s.fm_scaling = 1.0f / k.fm_deviation;               // setFMScaling(1.0f / m_fmDeviation)
        s.frames_cap = k.frames_cap;
        s.img_bytes = (s.d.rows * s.d.cols + 3) & ~3;
        atv_fresh(s.s);
        // img is the handle's to fill in; the FM buffers start as zeros (the constructor's memset)
    }

    static int front_made(sdrx_backend_t* front, int n_ch, const sdrx_atv_cfg* cfg)
    {
        for (int c = 0; c < n_ch; c++) {
            int rc = backend_set_front(front, c, 1, 0); if (rc) return rc;
            if (cfg[c].nco_freq == 0) { rc = backend_set_nomix(front, c); if (rc) return rc; }      // if (m_intFrequencyOffset != 0) c *= nextIQ()
        }
        return SDRX_OK;
    }

    static void hist(HistCarver& k, const AtvChan&, AtvBufs& u)
    {
        k.pair(u.nh, u.nh_next, (size_t)ATV_HIST);
        k.pair(u.xh, u.xh_next, (size_t)ATV_TAPS_MAX);
    }

    static void work(Carver& k, size_t n, const AtvChan& s, AtvBufs& u)
    {
        u.ci = k.take<float2>(s.decim ? n : 1);
        u.head = k.take<float2>(s.filt ? n + 2 * ATV_BLK : 1);
        u.tail = k.take<float2>(s.filt ? n + 2 * ATV_BLK : 1);
        u.raw = k.take<float>(n);
        u.grey = k.take<unsigned char>(n);
        u.scope = k.take<int16_t>(n);
        u.events = k.take<int>(n);                          // a sample renders at most once
        u.snaps = k.take<unsigned char>((size_t)s.frames_cap * (size_t)s.img_bytes);
    }

    static int64_t outputs_bound(const sdrx_atv_cfg&, int64_t n_in) { return n_in; }

    static int launch(DemodBank<AtvFamily>& b, unsigned nc, unsigned gx);
};

// the handle: the bank, every channel's screen and what the decimator and the FFT filter need, one allocation each
struct sdrx_atv : DemodBank<AtvFamily> {
    unsigned char* d_img = nullptr;
    size_t img_total = 0;
    char* d_aux = nullptr;                  // per channel: taps | filter, filterOpp | pend, ovl, fbuf
    float* d_utbl = nullptr;
    bool any_decim = false, any_filt = false;
    std::vector<std::vector<float>> taps;   // the phase-0 row per channel (empty without the decimator)
    std::vector<std::vector<float>> filt;   // filter | filterOpp as (re, im) pairs per channel (empty without the filter)
};
using Bank = DemodBank<AtvFamily>;
constexpr size_t AUX_TAPS = Carver::al(ATV_TAPS_MAX * 4), AUX_FILT = 2 * ATV_FFT * 8, AUX_BLK = ATV_BLK * 8;
constexpr size_t AUX_CH = AUX_TAPS + AUX_FILT + 3 * AUX_BLK;

int AtvFamily::launch(DemodBank<AtvFamily>& bank, unsigned nc, unsigned gx)
    {
        sdrx_atv& b = static_cast<sdrx_atv&>(bank);
        if (b.any_decim) {
            hipLaunchKernelGGL(atv_fir_kernel, dim3(gx, nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
            SDRX_HIP(hipGetLastError());
        }
        if (b.any_filt) {
            hipLaunchKernelGGL(atv_filt_kernel, dim3(gx / (ATV_BLK / 256) + 2, nc), dim3(ATV_FFT / 8), 0, b.core.stream, b.d_chan, b.d_bufs);
            SDRX_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(atv_video_kernel, dim3(gx, nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
        SDRX_HIP(hipGetLastError());
        const unsigned gw = (nc + ATV_WALK_WAVES - 1) / ATV_WALK_WAVES;
        hipLaunchKernelGGL(atv_walk_kernel, dim3(gw), dim3(64 * ATV_WALK_WAVES), 0, b.core.stream, b.d_chan, b.d_bufs, b.n_ch);
        SDRX_HIP(hipGetLastError());
        b.core.note_launch("atv_walk_kernel", (int)gw, 64 * ATV_WALK_WAVES, 0);
        hipLaunchKernelGGL(atv_carry_kernel, dim3(nc), dim3(256), 0, b.core.stream, b.d_chan, b.d_bufs);
        SDRX_HIP(hipGetLastError());
        return SDRX_OK;
    }

static int atv_destroy(sdrx_atv* b)
{
    if (!b) return SDRX_OK;
    (void)hipSetDevice(b->core.device);
    if (b->core.stream) (void)hipStreamSynchronize(b->core.stream);
    if (b->d_img) (void)hipFree(b->d_img);
    if (b->d_aux) (void)hipFree(b->d_aux);
    if (b->d_utbl) (void)hipFree(b->d_utbl);
    return Bank::destroy(b);
}

// the screens start as zeros; the channels' image pointers go up with the fresh state
static int atv_make_screens(sdrx_atv* b)
{
    SDRX_HIP(hipSetDevice(b->core.device));
    size_t total = 0;
    for (const AtvChan& s : b->h_chan) total += Carver::al((size_t)s.img_bytes);
    SDRX_HIP(hipMalloc(reinterpret_cast<void**>(&b->d_img), total));
    b->img_total = total;
    size_t off = 0;
    for (AtvChan& s : b->h_chan) { s.img = b->d_img + off; off += Carver::al((size_t)s.img_bytes); }
    SDRX_HIP(hipMemset(b->d_img, 0, total));
    // m_interpolator.create(24, tvRate, rf_bw / 2.2f, 3.0): its phase-0 row; fftfilt(.., 2048) + create_asym_filter(rf_opp_bw /
    // tvRate, rf_bw / tvRate), the quotients floats; the filter's carried blocks start as zeros
    const int n_ch = b->n_ch;
    b->taps.assign((size_t)n_ch, {}); b->filt.assign((size_t)n_ch, {});
    SDRX_HIP(hipMalloc(reinterpret_cast<void**>(&b->d_aux), (size_t)n_ch * AUX_CH));
    SDRX_HIP(hipMemset(b->d_aux, 0, (size_t)n_ch * AUX_CH));
    int rc = design_upload(&b->d_utbl, design_gfft_table(ATV_FFT)); if (rc) return rc;
    for (int c = 0; c < n_ch; c++) {
        AtvChan& s = b->h_chan[(size_t)c];
        const sdrx_atv_cfg& k = b->cfg[(size_t)c];
        char* base = b->d_aux + (size_t)c * AUX_CH;
        s.taps = reinterpret_cast<const float*>(base);
        s.filters = reinterpret_cast<const float2*>(base + AUX_TAPS);
        s.utbl = b->d_utbl;
        s.pend = reinterpret_cast<float2*>(base + AUX_TAPS + AUX_FILT);
        s.ovl = s.pend + ATV_BLK; s.fbuf = s.ovl + ATV_BLK;
        if (s.decim) {
            std::vector<float> poly; int nt = 0;
            design_interp(24, (double)s.d.tv_rate, (double)(k.rf_bw / 2.2f), 3.0, poly, &nt);
            if (nt > ATV_TAPS_MAX) return Bank::fail("create", ": the decimator has more taps per phase than the FIR carries");
            s.ntaps = nt;
            b->taps[(size_t)c].assign(poly.begin(), poly.begin() + nt);
            SDRX_HIP(hipMemcpy(base, poly.data(), (size_t)nt * 4, hipMemcpyHostToDevice));
            b->any_decim = true;
        }
        if (s.filt) {
            b->filt[(size_t)c].assign((size_t)2 * ATV_FFT * 2, 0.0f);
            const float fin = k.rf_bw / (float)s.d.tv_rate, fopp = k.rf_opp_bw / (float)s.d.tv_rate;
            for (int which = 0; which < 2; which++) {
                float2* dst = const_cast<float2*>(s.filters) + (size_t)which * ATV_FFT;
                rc = design_fft_filter<ATV_FFT>(dst, b->d_utbl, b->core.stream, &b->filt[(size_t)c][(size_t)which * ATV_FFT * 2],
                                                [&](float* f, int h2) { fftfilt_fill_lowpass(which ? fopp : fin, f, h2); });
                if (rc) return rc;
            }
            b->any_filt = true;
        }
    }
    return Bank::upload_fresh_state(b);
}

// the filters' carried blocks back to zeros (the taps and the spectra stay)
static int atv_clear_blocks(sdrx_atv* b)
{
    for (int c = 0; c < b->n_ch; c++)
        SDRX_HIP(hipMemset(b->d_aux + (size_t)c * AUX_CH + AUX_TAPS + AUX_FILT, 0, 3 * AUX_BLK));
    return SDRX_OK;
}

// a stored frame or the screen: rows * cols bytes from `src`
static int64_t atv_copy_image(sdrx_atv* b, const char* fn, int32_t c, const unsigned char* src, uint8_t* buf, int64_t cap)
{
    const AtvChan& s = b->h_chan[(size_t)c];
    const int64_t bytes = (int64_t)s.d.rows * s.d.cols;
    if (!buf || cap < bytes) return Bank::fail(fn, ": the buffer is too small for rows * cols bytes");
    SDRX_HIP(hipMemcpy(buf, src, (size_t)bytes, hipMemcpyDeviceToHost));
    return bytes;
}

extern "C" {

int sdrx_atv_create(sdrx_atv_t** out, int device, int32_t n_ch, const sdrx_atv_cfg* cfg)
{
    int rc = Bank::create(out, device, n_ch, cfg); if (rc) return rc;
    rc = atv_make_screens(*out);
    if (rc) { atv_destroy(*out); *out = nullptr; }
    return rc;
}
int sdrx_atv_destroy(sdrx_atv_t* b) { return atv_destroy(b); }
int sdrx_atv_reset(sdrx_atv_t* b)
{
    int rc = Bank::reset(b); if (rc) return rc;
    SDRX_HIP(hipMemset(b->d_img, 0, b->img_total));
    return atv_clear_blocks(b);
}
int sdrx_atv_feed_dev(sdrx_atv_t* b, const int16_t* const* d_iq, const int64_t* n_per_ch) { return Bank::feed_dev(b, d_iq, n_per_ch); }
int sdrx_atv_feed_bank(sdrx_atv_t* b, sdrx_chan_bank_t* bank) { return Bank::feed_bank(b, bank); }
int sdrx_atv_feed(sdrx_atv_t* b, const int16_t* const* iq, const int64_t* n_per_ch) { return Bank::feed(b, iq, n_per_ch); }

int64_t sdrx_atv_frames(sdrx_atv_t* b, int32_t c, int64_t* n_events)
{
    AtvChan s;
    int rc = Bank::fetch(b, "frames", c, &s); if (rc) return rc;
    if (n_events) *n_events = s.n_events;
    return std::min<int64_t>(s.n_events, s.frames_cap);
}
int64_t sdrx_atv_read_events(sdrx_atv_t* b, int32_t c, int32_t* index, int64_t cap)
{
    return Bank::read(b, "read_events", c, reinterpret_cast<int*>(index), cap, &AtvBufs::events, &AtvChan::n_events, 4);
}
int64_t sdrx_atv_read_frame(sdrx_atv_t* b, int32_t c, int64_t k, uint8_t* buf, int64_t cap)
{
    AtvChan s;
    int rc = Bank::fetch(b, "read_frame", c, &s); if (rc) return rc;
    if (k < 0 || k >= std::min<int64_t>(s.n_events, s.frames_cap)) return Bank::fail("read_frame", ": no such stored frame in the last feed");
    return atv_copy_image(b, "read_frame", c, b->h_bufs[c].snaps + (size_t)k * (size_t)s.img_bytes, buf, cap);
}
int64_t sdrx_atv_read_screen(sdrx_atv_t* b, int32_t c, uint8_t* buf, int64_t cap)
{
    AtvChan s;
    int rc = Bank::fetch(b, "read_screen", c, &s); if (rc) return rc;       // waits for the stream
    return atv_copy_image(b, "read_screen", c, s.img, buf, cap);
}
int sdrx_atv_frames_last_dev(sdrx_atv_t* b, int32_t c, const uint8_t** d_frames, int64_t* n_stored, int64_t* pitch)
{
    if (!d_frames || !n_stored || !pitch) return Bank::fail("frames_last_dev", ": bad argument");
    AtvChan s;
    int rc = Bank::fetch(b, "frames_last_dev", c, &s); if (rc) return rc;
    *n_stored = std::min<int64_t>(s.n_events, s.frames_cap);
    *pitch = s.img_bytes;
    *d_frames = b->ch[(size_t)c].cap_in ? b->h_bufs[c].snaps : nullptr;      // the snapshot arena (none before the first feed), never the live screen
    return SDRX_OK;
}
int sdrx_atv_screen_last_dev(sdrx_atv_t* b, int32_t c, const uint8_t** d_screen, int32_t* rows, int32_t* cols)
{
    if (!d_screen || !Bank::in_range(b, c)) return Bank::fail("screen_last_dev", ": bad argument");
    const AtvChan& s = b->h_chan[(size_t)c];
    *d_screen = s.img;
    if (rows) *rows = s.d.rows;
    if (cols) *cols = s.d.cols;
    return SDRX_OK;
}

int64_t sdrx_atv_read(sdrx_atv_t* b, int32_t c, int16_t* scope_re, int64_t cap)
{
    return Bank::read(b, "read", c, scope_re, cap, &AtvBufs::scope, &AtvChan::n_scope, 2);
}
int sdrx_atv_last_dev(sdrx_atv_t* b, int32_t c, const int16_t** d_scope_re, int64_t* n)
{
    return Bank::last_dev(b, "last_dev", c, d_scope_re, n, &AtvBufs::scope, &AtvChan::n_scope);
}

int sdrx_atv_state(sdrx_atv_t* b, int32_t c, sdrx_atv_state_t* out)
{
    if (!out) return Bank::fail("state", ": bad argument");
    AtvChan q;
    int rc = Bank::fetch(b, "state", c, &q); if (rc) return rc;
    const AtvState& s = q.s;
    auto bits = [](float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; };
    out->image_index = s.image_index; out->synchro_points = s.synchro_points; out->synchro_detected = s.synchro_detected;
    out->vertical_synchro_detected = s.vsynchro_detected; out->col_index = s.col_index; out->sample_index = s.sample_index;
    out->row_index = s.row_index; out->line_index = s.line_index; out->avg_col_index = s.avg_col_index; out->screen_row = s.screen_row;
    out->amp_line_average = bits(s.amp_line_average); out->eff_min = bits(s.eff_min); out->eff_max = bits(s.eff_max);
    out->amp_min = bits(s.amp_min); out->amp_max = bits(s.amp_max); out->amp_delta = bits(s.amp_delta);
    for (int k = 0; k < ATV_HIST; k++) { out->buffer_i[k] = bits(q.hist[k].x); out->buffer_q[k] = bits(q.hist[k].y); }
    return SDRX_OK;
}

int sdrx_atv_get_design(sdrx_atv_t* b, int32_t c, sdrx_atv_design_t* out)
{
    if (!out || !Bank::in_range(b, c)) return Bank::fail("get_design", ": bad argument");
    const AtvDesign& d = b->h_chan[(size_t)c].d;
    out->samples_per_line = d.spl; out->samples_per_top = d.spt; out->samples_per_line_signals = d.sp_signals; out->samples_per_hsync = d.sp_hsync;
    out->sync_lines = d.sync_lines; out->black_lines = d.black_lines; out->eq_lines = d.eq_lines; out->interleaved = d.interleaved;
    out->tv_rate = d.tv_rate; out->cols = d.cols; out->rows = d.rows;
    return sdrx_backend_get_design(b->front, c, nullptr, nullptr, 0, nullptr, &out->nco_inc);
}

int sdrx_atv_get_filters(sdrx_atv_t* b, int32_t c, int32_t* ntaps, float* taps, int32_t taps_cap, float* filter_iq, float* filter_opp_iq)
{
    if (!Bank::in_range(b, c)) return Bank::fail("get_filters", ": bad argument");
    const std::vector<float>& t = b->taps[(size_t)c];
    const std::vector<float>& f = b->filt[(size_t)c];
    if (ntaps) *ntaps = (int32_t)t.size();
    if (taps && taps_cap > 0) std::memcpy(taps, t.data(), std::min<size_t>(t.size(), (size_t)taps_cap) * 4);
    if (!f.empty()) {
        if (filter_iq) std::memcpy(filter_iq, f.data(), (size_t)ATV_FFT * 8);
        if (filter_opp_iq) std::memcpy(filter_opp_iq, f.data() + (size_t)ATV_FFT * 2, (size_t)ATV_FFT * 8);
    }
    return f.empty() ? 0 : ATV_FFT;
}

int sdrx_atv_sync(sdrx_atv_t* b) { return b ? b->core.sync() : SDRX_EINVAL; }
int sdrx_atv_set_stream(sdrx_atv_t* b, void* hip_stream) { return Bank::set_stream(b, hip_stream); }
int sdrx_atv_get_stream(sdrx_atv_t* b, void** hip_stream) { return b ? b->core.get_stream(hip_stream) : SDRX_EINVAL; }
int sdrx_atv_set_timing(sdrx_atv_t* b, int enabled) { return b ? b->core.set_timing(enabled) : SDRX_EINVAL; }
int sdrx_atv_get_timing(sdrx_atv_t* b, double* total_ms, int64_t* feeds, int reset) { return b ? b->core.get_timing(total_ms, feeds, reset) : SDRX_EINVAL; }
int sdrx_atv_last_launch(const sdrx_atv_t* b, char* kernel_name, int name_cap, int* grid, int* block, int* lds_bytes) { return b ? b->core.last_launch(kernel_name, name_cap, grid, block, lds_bytes) : SDRX_EINVAL; }

} // extern "C"
