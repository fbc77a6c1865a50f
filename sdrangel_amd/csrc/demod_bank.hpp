// The host skeleton of a demodulator bank whose front is a channel back-end (sdrx_am.hip, sdrx_nfm.hip, sdrx_ssb.hip,
// sdrx_udpsrc.hip, sdrx_lora.hip, sdrx_atv.hip): the handle's members, create / destroy / reset, capacity growth, the per-feed pointer table, the three
// feed entry points and the getters that only fetch one channel's state.  A family F supplies what is its own:
//   Handle, Cfg, Chan, Bufs      the opaque C type (struct sdrx_x : DemodBank<F> {}), its configuration, the device-resident
//                                channel state and the per-channel pointer table of its kernel header
//   name                         "sdrx_x": the prefix of every error text
//   input                        the member of Bufs that takes the front's output (n_ptr takes its count)
//   validate(n_ch, cfg)          before the first HIP call
//   design(c, k, f, s, bp)       channel c: the front's configuration f and the fresh state s, both zeroed beforehand, and the
//                                bp_taps Bandpass taps at bp (nullptr where bp_taps is 0)
//   hist(k, s, u)                the layout of one history set: a k.pair() per carried array
//   fresh(s, u)                  fills a zeroed host image of one history set through u's *_next pointers
//   work(k, n, s, u)             the layout of channel s's per-feed work arena for n = capacity + work_extra + 16 elements
//   outputs_bound(k, n_in)       most outputs channel k's feed of n_in inputs can have: sizes the grids
//   launch(b, nc, gx)            the kernel sequence with its note_launch; gx blocks of 256 cover the bound
//   front_made(front, n, cfg)    runs on a fresh front before it is fed
//   cutoff(k, f)                 the Interpolator's cutoff as the double the reference passes to create()
// DemodDefaults has work_extra, bp_taps, fresh, front_made and cutoff for a family without them.  Both layouts run twice through
// demod_carve.hpp, counting and placing, so an arena's size and its pointers come from one description.  DESIGN.md 4.11.
#pragma once
#include "sdrx_common.hpp"
#include "backend_view.hpp"
#include "demod_common.hpp"
#include "demod_carve.hpp"
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

namespace sdrx {

struct DemodDefaults {
    static constexpr int work_extra = 0;
    static constexpr int bp_taps = 0;
    template <class Chan, class Bufs> static void fresh(const Chan&, Bufs&) {}      // all zeros
    template <class Cfg> static int front_made(sdrx_backend_t*, int, const Cfg*) { return SDRX_OK; }
    // what Interpolator::create gets as its cutoff: the float of the front's configuration, widened
    template <class Cfg> static double cutoff(const Cfg&, const sdrx_backend_cfg& f) { return (double)f.interp_cutoff; }
};

// every output after the first two of a stream consumes >= floor(step) inputs
inline int64_t demod_outputs_bound(int64_t floor_step, int64_t n_in) { return std::min<int64_t>(n_in, n_in / std::max<int64_t>(1, floor_step) + 4); }

template <class F>
struct DemodBank {
    using H = typename F::Handle;
    using Cfg = typename F::Cfg;
    using Chan = typename F::Chan;
    using Bufs = typename F::Bufs;

    struct Host {
        DevBuf work, stage_in;
        char* hist = nullptr;             // two sets of F::hist's layout
        size_t hist_set = 0;              // bytes of one set
        int cur = 0;
        int64_t cap_in = 0;
    };

    HandleCore core;
    int n_ch = 0;
    std::vector<Cfg> cfg;
    std::vector<sdrx_backend_cfg> be_cfg;
    sdrx_backend_t* front = nullptr;
    std::vector<Host> ch;
    std::vector<Chan> h_chan;     // configuration and the state of a fresh handle
    Chan* d_chan = nullptr;
    Bufs* d_bufs = nullptr;
    Bufs* h_bufs = nullptr;       // pinned: the per-feed table goes to the device in one async copy
    hipEvent_t bufs_ev = nullptr;
    float* d_bp = nullptr;        // bp_taps Bandpass taps per channel
    std::vector<float> bp_all;

    static std::string who(const char* fn) { return std::string(F::name) + "_" + fn; }
    static int fail(const char* fn, const char* text) { set_error(who(fn) + text); return SDRX_EINVAL; }
    static bool in_range(const H* b, int32_t c) { return b && c >= 0 && c < b->n_ch; }

    // the two layouts: null bases count, real ones fill u; the size comes back either way
    static size_t lay_hist(const Chan& s, Bufs& u, char* cur, char* next)
    {
        HistCarver k{{cur}, {next}};
        F::hist(k, s, u);
        return k.cur.off;
    }
    static size_t lay_work(int64_t cap_in, const Chan& s, Bufs& u, char* base)
    {
        Carver k{base};
        F::work(k, (size_t)cap_in + F::work_extra + 16, s, u);
        return k.off;
    }

    static int ensure_capacity(H* b, int c, int64_t n_in)
    {
        Host& h = b->ch[(size_t)c];
        if (n_in <= h.cap_in) return SDRX_OK;
        int64_t cap = h.cap_in ? h.cap_in : 4096;
        while (cap < n_in) cap *= 2;
        // every output consumes at least one input (step >= 1): at most `cap` per feed, plus work_extra; nothing here carries state
        Bufs u{};
        const size_t bytes = lay_work(cap, b->h_chan[(size_t)c], u, nullptr);
        SDRX_HIP(hipStreamSynchronize(b->core.stream));
        int rc = h.work.reserve(bytes); if (rc) return rc;
        h.cap_in = cap;
        return SDRX_OK;
    }

    // both sets get the fresh image: the carry kernel rewrites a set in full before it is read as the current one
    static int upload_fresh_state(H* b)
    {
        SDRX_HIP(hipMemcpyAsync(b->d_chan, b->h_chan.data(), (size_t)b->n_ch * sizeof(Chan), hipMemcpyHostToDevice, b->core.stream));
        size_t total = 0;
        for (const Host& h : b->ch) total += h.hist_set;
        std::vector<char> img(total, 0);                    // every channel's image, alive until the copies are done
        char* p = img.data();
        for (int c = 0; c < b->n_ch; c++) {
            Host& h = b->ch[(size_t)c];
            Bufs u{};
            lay_hist(b->h_chan[(size_t)c], u, p, p);
            F::fresh(b->h_chan[(size_t)c], u);
            for (int k = 0; k < 2; k++)
                SDRX_HIP(hipMemcpyAsync(h.hist + (size_t)k * h.hist_set, p, h.hist_set, hipMemcpyHostToDevice, b->core.stream));
            h.cur = 0;
            p += h.hist_set;
        }
        SDRX_HIP(hipStreamSynchronize(b->core.stream));
        return SDRX_OK;
    }

    static int make_front(H* b)
    {
        std::vector<double> cut((size_t)b->n_ch);
        for (int c = 0; c < b->n_ch; c++) cut[(size_t)c] = F::cutoff(b->cfg[(size_t)c], b->be_cfg[(size_t)c]);
        int rc = backend_create_cutoff(&b->front, b->core.device, b->n_ch, b->be_cfg.data(), cut.data()); if (rc) return rc;
        rc = F::front_made(b->front, b->n_ch, b->cfg.data()); if (rc) return rc;
        return backend_set_stream(b->front, b->core.stream);
    }

    static int destroy(H* b)
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

    static int create(H** out, int device, int32_t n_ch, const Cfg* cfg)
    {
        if (!out) return fail("create", ": null out");
        *out = nullptr;
        int rc = F::validate(n_ch, cfg); if (rc) return rc;
        H* b = new (std::nothrow) H;
        if (!b) return SDRX_ENOMEM;
        rc = b->core.open(device);
        if (rc) { delete b; return rc; }
        b->n_ch = n_ch;
        b->cfg.assign(cfg, cfg + n_ch);
        b->ch.resize((size_t)n_ch); b->h_chan.resize((size_t)n_ch); b->be_cfg.resize((size_t)n_ch);
        b->bp_all.assign((size_t)n_ch * F::bp_taps, 0.0f);

        for (int c = 0; c < n_ch; c++) {
            sdrx_backend_cfg& f = b->be_cfg[(size_t)c];
            std::memset(&f, 0, sizeof f);
            Chan& s = b->h_chan[(size_t)c];
            std::memset(&s, 0, sizeof s);
            F::design(c, cfg[c], f, s, F::bp_taps ? &b->bp_all[(size_t)c * F::bp_taps] : nullptr);
            Host& h = b->ch[(size_t)c];
            Bufs u{};
            h.hist_set = lay_hist(s, u, nullptr, nullptr);
            SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&h.hist), 2 * h.hist_set), destroy(b));
        }
        if (F::bp_taps) {
            SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&b->d_bp), b->bp_all.size() * 4), destroy(b));
            SDRX_HIP_ELSE(hipMemcpy(b->d_bp, b->bp_all.data(), b->bp_all.size() * 4, hipMemcpyHostToDevice), destroy(b));
        }
        SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&b->d_chan), (size_t)n_ch * sizeof(Chan)), destroy(b));
        SDRX_HIP_ELSE(hipMalloc(reinterpret_cast<void**>(&b->d_bufs), (size_t)n_ch * sizeof(Bufs)), destroy(b));
        SDRX_HIP_ELSE(hipHostMalloc(reinterpret_cast<void**>(&b->h_bufs), (size_t)n_ch * sizeof(Bufs), hipHostMallocDefault), destroy(b));
        SDRX_HIP_ELSE(hipEventCreateWithFlags(&b->bufs_ev, hipEventDisableTiming), destroy(b));
        SDRX_HIP_ELSE(hipEventRecord(b->bufs_ev, b->core.stream), destroy(b));
        rc = make_front(b);
        if (!rc) rc = upload_fresh_state(b);
        if (rc) { destroy(b); return rc; }
        *out = b;
        return SDRX_OK;
    }

    static int reset(H* b)
    {
        if (!b) return fail("reset", ": null handle");
        SDRX_HIP(hipSetDevice(b->core.device));
        SDRX_HIP(hipStreamSynchronize(b->core.stream));
        // the front has no reset of its own: a fresh one with the same design
        if (b->front) { (void)sdrx_backend_destroy(b->front); b->front = nullptr; }
        int rc = make_front(b); if (rc) return rc;
        return upload_fresh_state(b);
    }

    // the tail behind a front feed that has just been queued on the handle's stream
    static int tail(H* b, const int64_t* n_per_ch)
    {
        int64_t bound = 0;
        for (int c = 0; c < b->n_ch; c++) {
            int rc = ensure_capacity(b, c, std::max<int64_t>(n_per_ch[c], 1)); if (rc) return rc;
            bound = std::max(bound, F::outputs_bound(b->cfg[(size_t)c], n_per_ch[c]));
        }
        SDRX_HIP(hipEventSynchronize(b->bufs_ev));            // previous feed's copy has read the table
        for (int c = 0; c < b->n_ch; c++) {
            Host& h = b->ch[(size_t)c];
            Bufs& u = b->h_bufs[c];
            BackendView v;
            int rc = backend_view(b->front, c, &v); if (rc) return rc;
            u.*F::input = static_cast<const float2*>(v.out); u.n_ptr = v.n_out;
            lay_hist(b->h_chan[(size_t)c], u, h.hist + (size_t)h.cur * h.hist_set, h.hist + (size_t)(h.cur ^ 1) * h.hist_set);
            lay_work(h.cap_in, b->h_chan[(size_t)c], u, static_cast<char*>(h.work.p));
        }
        int rc = demod_upload_bufs(b->d_bufs, b->h_bufs, b->n_ch, b->bufs_ev, b->core.stream); if (rc) return rc;
        rc = F::launch(*b, (unsigned)b->n_ch, (unsigned)std::max<int64_t>(1, (bound + 255) / 256)); if (rc) return rc;
        for (auto& h : b->ch) h.cur ^= 1;
        return SDRX_OK;
    }

    static int feed_dev(H* b, const int16_t* const* d_iq, const int64_t* n_per_ch)
    {
        static const std::string me = who("feed_dev");
        if (!b || !d_iq || !n_per_ch) return fail("feed_dev", ": null argument");
        SDRX_HIP(hipSetDevice(b->core.device));
        int rc = demod_check_lengths(b->n_ch, n_per_ch, me.c_str()); if (rc) return rc;
        rc = demod_check_dev_pointers(b->n_ch, d_iq, n_per_ch, me.c_str()); if (rc) return rc;
        rc = b->core.timer.begin(b->core.stream); if (rc) return rc;
        rc = sdrx_backend_feed_dev(b->front, d_iq, n_per_ch); if (rc) return rc;
        rc = tail(b, n_per_ch); if (rc) return rc;
        return b->core.timer.end(b->core.stream);
    }

    static int feed_bank(H* b, sdrx_chan_bank_t* bank)
    {
        static const std::string me = who("feed_bank");
        if (!b || !bank) return fail("feed_bank", ": null argument");
        SDRX_HIP(hipSetDevice(b->core.device));
        std::vector<const int16_t*> d;                          // the front takes them from the bank itself
        std::vector<int64_t> n;
        int rc = demod_gather_bank(bank, b->n_ch, me.c_str(), d, n); if (rc) return rc;
        rc = demod_check_lengths(b->n_ch, n.data(), me.c_str()); if (rc) return rc;
        rc = b->core.timer.begin(b->core.stream); if (rc) return rc;
        // the front orders its readers against the bank's stream (sdrx_backend_feed_bank); the tail reads the front's output only
        rc = sdrx_backend_feed_bank(b->front, bank); if (rc) return rc;
        rc = tail(b, n.data()); if (rc) return rc;
        return b->core.timer.end(b->core.stream);
    }

    static int feed(H* b, const int16_t* const* iq, const int64_t* n_per_ch)
    {
        static const std::string me = who("feed");
        if (!b || !iq || !n_per_ch) return fail("feed", ": null argument");
        SDRX_HIP(hipSetDevice(b->core.device));
        std::vector<const int16_t*> d;
        int rc = demod_stage_inputs(b->ch, b->core.stream, iq, n_per_ch, me.c_str(), d); if (rc) return rc;
        rc = feed_dev(b, d.data(), n_per_ch); if (rc) return rc;
        SDRX_HIP(hipStreamSynchronize(b->core.stream));            // the caller's buffers are free again on return
        return SDRX_OK;
    }

    // channel c's state as the device has it once the stream is idle; `fn` names the entry point in the error text
    static int fetch(H* b, const char* fn, int32_t c, Chan* s)
    {
        if (!in_range(b, c)) return fail(fn, ": bad argument");
        return demod_fetch_state(b->core, b->d_chan, c, s);
    }

    // an output stream of the last feed: `out` in the pointer table, `count` samples of `bytes` each
    template <class T>
    static int64_t read(H* b, const char* fn, int32_t c, T* dst, int64_t cap, T* Bufs::* out, int Chan::* count, size_t bytes)
    {
        if (cap < 0 || (cap > 0 && !dst)) return fail(fn, ": bad argument");
        Chan s;
        int rc = fetch(b, fn, c, &s); if (rc) return rc;
        const int64_t n = std::min<int64_t>(s.*count, cap);
        if (n == 0) return 0;
        SDRX_HIP(hipMemcpy(dst, b->h_bufs[c].*out, (size_t)n * bytes, hipMemcpyDeviceToHost));
        return n;
    }

    template <class T>
    static int last_dev(H* b, const char* fn, int32_t c, const T** d, int64_t* n, T* Bufs::* out, int Chan::* count)
    {
        if (!d || !n) return fail(fn, ": bad argument");
        Chan s;
        int rc = fetch(b, fn, c, &s); if (rc) return rc;
        *d = s.*count > 0 ? b->h_bufs[c].*out : static_cast<const T*>(b->ch[(size_t)c].work.p);
        *n = s.*count;
        return SDRX_OK;
    }

    static int flag(H* b, const char* fn, int32_t c, int Chan::* m)
    {
        Chan s;
        int rc = fetch(b, fn, c, &s); if (rc) return rc;
        return s.*m;
    }

    // getMagSqLevels: F::magsq(s) is the family's m_magsq; a reset takes the sum, the peak and the count back to 0, m_magsq stays
    static int levels(H* b, int32_t c, double* magsq, double* sum, double* peak, int64_t* count, int reset)
    {
        Chan s;
        int rc = fetch(b, "levels", c, &s); if (rc) return rc;
        if (magsq) *magsq = F::magsq(s);
        if (sum) *sum = s.magsq_sum;
        if (peak) *peak = s.magsq_peak;
        if (count) *count = s.magsq_count;
        if (!reset) return SDRX_OK;
        return demod_zero_levels(b->core, b->d_chan + c, offsetof(Chan, magsq_sum), offsetof(Chan, magsq_peak), offsetof(Chan, magsq_count));
    }

    static int set_stream(H* b, void* hip_stream)
    {
        if (!b) return SDRX_EINVAL;
        int rc = b->core.set_stream(hip_stream); if (rc) return rc;
        return backend_set_stream(b->front, b->core.stream);      // the front launches on the same stream
    }
};

} // namespace sdrx
