// host code the demodulator banks and the channel back-end share (sdrx_wfm.hip and sdrx_backend.hip directly; sdrx_am.hip,
// sdrx_nfm.hip, sdrx_ssb.hip and sdrx_udpsrc.hip through demod_bank.hpp): input staging and checks, the hand-over from a
// channelizer bank and the ordering against its stream, one channel's device state, the per-feed pointer table, growth
// and reset of a work arena with carried fronts, the Bandpass design.  `who` is the entry point named in the error text.
#pragma once
#include "sdrx_common.hpp"
#include "demod_carve.hpp"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace sdrx {

inline int demod_check_lengths(int n_ch, const int64_t* n_per_ch, const char* who)
{
    for (int c = 0; c < n_ch; c++)
        if (n_per_ch[c] < 0 || n_per_ch[c] > 0x0fffffff) { set_error(std::string(who) + ": bad length"); return SDRX_EINVAL; }
    return SDRX_OK;
}

inline int demod_check_dev_pointers(int n_ch, const int16_t* const* d_iq, const int64_t* n_per_ch, const char* who)
{
    for (int c = 0; c < n_ch; c++)
        if (n_per_ch[c] > 0 && (!d_iq[c] || (reinterpret_cast<uintptr_t>(d_iq[c]) & 3u))) {
            set_error(std::string(who) + ": null or misaligned channel pointer"); return SDRX_EINVAL;
        }
    return SDRX_OK;
}

// host-pointer feed: once the stream is idle, channel c's samples go to ch[c].stage_in on it; d[c] is that device copy
template <class Host>
int demod_stage_inputs(std::vector<Host>& ch, hipStream_t stream, const int16_t* const* iq, const int64_t* n_per_ch, const char* who,
                       std::vector<const int16_t*>& d)
{
    SDRX_HIP(hipStreamSynchronize(stream));
    d.resize(ch.size());
    for (size_t c = 0; c < ch.size(); c++) {
        if (n_per_ch[c] < 0 || n_per_ch[c] > 0x0fffffff || (n_per_ch[c] > 0 && !iq[c])) { set_error(std::string(who) + ": bad length or null channel pointer"); return SDRX_EINVAL; }
        DevBuf& st = ch[c].stage_in;
        int rc = st.reserve((size_t)std::max<int64_t>(n_per_ch[c], 1) * 4); if (rc) return rc;
        if (n_per_ch[c] > 0) SDRX_HIP(hipMemcpyAsync(st.p, iq[c], (size_t)n_per_ch[c] * 4, hipMemcpyHostToDevice, stream));
        d[c] = static_cast<const int16_t*>(st.p);
    }
    return SDRX_OK;
}

// what the bank's last feed produced for its channels 0 .. n_ch-1; `me` is what the error text calls the caller
inline int demod_gather_bank(sdrx_chan_bank_t* bank, int n_ch, const char* who, std::vector<const int16_t*>& d, std::vector<int64_t>& n,
                             const char* me = "the demodulator bank")
{
    d.resize((size_t)n_ch); n.resize((size_t)n_ch);
    for (int c = 0; c < n_ch; c++) {
        int rc = sdrx_chan_bank_last_dev(bank, c, &d[(size_t)c], &n[(size_t)c]);
        if (rc) { set_error(std::string(who) + ": the bank has fewer channels than " + me); return rc; }
    }
    return SDRX_OK;
}

template <class Chan>
int demod_fetch_state(const HandleCore& core, const Chan* d_chan, int32_t c, Chan* s)
{
    SDRX_HIP(hipSetDevice(core.device));
    SDRX_HIP(hipMemcpyAsync(s, d_chan + c, sizeof *s, hipMemcpyDeviceToHost, core.stream));
    SDRX_HIP(hipStreamSynchronize(core.stream));
    return SDRX_OK;
}

// getMagSqLevels' reset: the sum and the peak (doubles) and the count (long long) of one channel's state back to 0
template <class Chan>
int demod_zero_levels(const HandleCore& core, Chan* chan, size_t sum_off, size_t peak_off, size_t count_off)
{
    char* base = reinterpret_cast<char*>(chan);
    SDRX_HIP(hipMemsetAsync(base + sum_off, 0, sizeof(double), core.stream));
    SDRX_HIP(hipMemsetAsync(base + peak_off, 0, sizeof(double), core.stream));
    SDRX_HIP(hipMemsetAsync(base + count_off, 0, sizeof(long long), core.stream));
    SDRX_HIP(hipStreamSynchronize(core.stream));
    return SDRX_OK;
}

// the pinned per-feed table goes to the device in one async copy; `ev` behind it is what the next feed waits for
// (hipEventSynchronize) before it rewrites the table
template <class Bufs>
int demod_upload_bufs(Bufs* d_bufs, const Bufs* h_bufs, int n_ch, hipEvent_t ev, hipStream_t stream)
{
    SDRX_HIP(hipMemcpyAsync(d_bufs, h_bufs, (size_t)n_ch * sizeof(Bufs), hipMemcpyHostToDevice, stream));
    SDRX_HIP(hipEventRecord(ev, stream));
    return SDRX_OK;
}

// A work arena whose layout marks carried fronts (Carver::take_kept): `lay(k, cap, bufs)` describes it for feeds of up to
// `cap` samples.  demod_place: the pointers it hands out at `base`, all null for a null base.
template <class Bufs, class Lay>
Bufs demod_place(void* base, int64_t cap, Lay lay)
{
    Bufs u{};
    Carver k{static_cast<char*>(base)};
    lay(k, cap, u);
    return u;
}

// Growth starts at 4096 samples and doubles until n_in fits.  The new arena is zeroed, takes each kept range from where the
// old layout had it, and replaces the old arena after a single wait for the stream.
template <class Bufs, class Lay>
int demod_grow_arena(DevBuf& arena, int64_t& cap_in, int64_t n_in, hipStream_t stream, Lay lay)
{
    if (n_in <= cap_in) return SDRX_OK;
    int64_t cap = cap_in ? cap_in : 4096;
    while (cap < n_in) cap *= 2;
    Carver was{nullptr}, now{nullptr};
    Bufs u{};
    lay(was, cap_in, u); lay(now, cap, u);
    char* np = nullptr;
    SDRX_HIP(hipMalloc(reinterpret_cast<void**>(&np), now.off));
    hipError_t e = hipMemsetAsync(np, 0, now.off, stream);
    for (int i = 0; arena.p && i < now.n_kept && e == hipSuccess; i++)
        e = hipMemcpyAsync(np + now.kept[i].off, static_cast<const char*>(arena.p) + was.kept[i].off, now.kept[i].bytes, hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) { (void)hipFree(np); return hip_fail(e, "grow arena", __FILE__, __LINE__); }
    arena.release();
    arena.p = np; arena.cap = now.off; cap_in = cap;
    return SDRX_OK;
}

// a fresh stream: the kept ranges of an arena laid out for cap_in samples back to zero, on the stream
template <class Bufs, class Lay>
int demod_clear_kept(const DevBuf& arena, int64_t cap_in, hipStream_t stream, Lay lay)
{
    Carver k{nullptr};
    Bufs u{};
    lay(k, cap_in, u);
    for (int i = 0; arena.p && i < k.n_kept; i++) SDRX_HIP(hipMemsetAsync(static_cast<char*>(arena.p) + k.kept[i].off, 0, k.kept[i].bytes, stream));
    return SDRX_OK;
}

// Device-side ordering of a feed against the stream that is still writing its input: `later` runs nothing queued from here on
// until `earlier` has done what it holds now.  Once with (feed's stream, producer) in front of the kernels that read the
// input, once with (producer, feed's stream) behind them; a no-op without a second stream.
inline int demod_stream_after(hipStream_t later, hipStream_t earlier, hipEvent_t ev)
{
    if (!later || !earlier || later == earlier) return SDRX_OK;
    SDRX_HIP(hipEventRecord(ev, earlier));
    SDRX_HIP(hipStreamWaitEvent(later, ev, 0));
    return SDRX_OK;
}

// Bandpass<Real>::create(301, sampleRate, lowCutoff, highCutoff) (bandpass.h:15-75): the folded taps [0 .. 150]
inline void demod_bandpass_design(double rate, double f1, double f2, float* t)
{
    const double PI = 3.14159265358979323846;
    const int ntaps = 301, nt = 151;
    const double mid = ((double)ntaps - 1.0) / 2.0;
    const double Wcl = 2.0 * PI * f1 / rate, Wch = 2.0 * PI * f2 / rate;
    std::vector<float> lp((size_t)nt), hp((size_t)nt);
    for (int i = 0; i < nt; i++) {
        if (i == (ntaps - 1) / 2) { lp[(size_t)i] = (float)(Wch / PI); hp[(size_t)i] = (float)(-(Wcl / PI)); }
        else {
            lp[(size_t)i] = (float)(std::sin(((double)i - mid) * Wch) / (((double)i - mid) * PI));
            hp[(size_t)i] = (float)(-std::sin(((double)i - mid) * Wcl) / (((double)i - mid) * PI));
        }
    }
    hp[(size_t)((ntaps - 1) / 2)] += 1;
    for (int i = 0; i < nt; i++) {
        const double w = 0.54 + 0.46 * std::cos((2.0 * PI * ((double)i - mid)) / (double)ntaps);
        lp[(size_t)i] = (float)(lp[(size_t)i] * w); hp[(size_t)i] = (float)(hp[(size_t)i] * w);
        t[i] = -(lp[(size_t)i] + hp[(size_t)i]);
    }
    t[(ntaps - 1) / 2] += 1;
    float sum = 0; int i;
    for (i = 0; i < nt - 1; i++) sum += t[i] * 2;
    sum += t[i];
    for (i = 0; i < nt; i++) t[i] /= sum;
}

} // namespace sdrx
