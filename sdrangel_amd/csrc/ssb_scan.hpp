// The recurrences of SSBDemod::feed's per-sample loop (plugins/channelrx/demodssb/ssbdemod.cpp:181-250) and of
// MagAGC::feedAndGetValue (sdrbase/dsp/agc.cpp:98-182, m_squared = false) cut into terms that can be computed in
// parallel.  Stream indexing (am_stream_at / am_hist_next) is am_scan.hpp's.  Compiles for the host too
// (tests/ssb_scan_check.cpp), no HIP header needed.
//
// 1. Spectrum stream: m_sum += s[j] in float; a group closes on the sample whose pre-increment m_undersampleCount is a
//    multiple of decim = 1 << (span_log2 - 1), so groups are independent once the counter is known (ssb_first_close): group q
//    of a feed closes at i0 + q * decim and sums the decim samples up to there in their order, from 0.  Only the open group's
//    partial sum and the counter carry.
// 2. MovingAverage<double>: m_sum += magsq[j] - magsq[j - hn], the history 0 before the stream: a rounded prefix sum of terms
//    known in advance (psum_rows).  magsq is the double of a float sum of squares, so the history is kept in float.
// 3. m_u0 is pointwise from magsq[j] and the sum after sample j (ssb_u0).
// 4. The four counters, three scans in a row, each over maps that are closed under composition:
//      above[j] = magsq[j] > threshold
//      a. m_gateCounter  g -> above ? min(g + 1, gate) : 0                     WfmClamp {1, 0, gate} / the constant {0, 0, 0}
//         reset[j] = above[j] && g[j - 1] >= gate   (`if (m_gateCounter < m_gate) m_gateCounter++; else m_count = 0;`)
//      b. m_count        c -> reset ? 0 : (above ? c : min(c + 1, hn))         WfmClamp {0, 0, 0} / {0, 0, hn} / {1, 0, hn}
//         up[j] = c[j] < hn                          (m_stepDownDelay = hn)
//      c. the step counters are a pair (U, D) = (m_stepUpCounter, m_stepDownCounter), both in [0, L], L = hn / 2:
//           up step    (U, D) -> (min(U + 1, L), U)
//           down step  (U, D) -> (D, max(D - 1, 0))
//         Either reads ONE component x of its input and gives (cu(x), cd(x)) with two clamp maps: SsbPair {sel, u, d}.
//         g after f reads component g.sel of f's output, which is f's clamp map for that component applied to f's x:
//           (g o f) = {f.sel, compose(f[g.sel], g.u), compose(f[g.sel], g.d)}
//         and clamp maps are closed under composition, so SsbPair is; the identity reads both components and carries a flag
//         (sel = -1).
//    The factor feedAndGetValue returns and getStepValue() are pointwise from the pair before and after the step
//    (ssb_agc_value, ssb_step_value).
// 5. DoubleBufferFIFO<cmplx>(96000): readBack(hn) runs BEFORE this sample's write, m_currentIndex names the previous write:
//    x[j] = w[j - 1 - hn] for hn < 96000.  readBack clamps its delay to the line's size, and at delay == size the slot it
//    names is m_currentIndex itself: for hn >= 96000 x[j] = w[j - 1] (ssb_delay), as NFM's line does at its size.
#pragma once
#include "am_scan.hpp"
#if defined(__HIPCC__)
#include "demod_wg.hpp"                   // wg_scan, for magagc_trip at the end
#endif

namespace sdrx {

constexpr int SSB_DL = 2 * 48000;                          // m_squelchDelayLine(2*48000)
constexpr int SSB_MAX_HN = 131072;
constexpr double SSB_CLAMP_MAX = 32768.0 / 100.0;           // m_agc.setClampMax(SDR_RX_SCALED/100.0)

AM_HD int ssb_delay(int hn) { return hn >= SSB_DL ? 0 : hn; }          // x[j] = w[j - 1 - ssb_delay(hn)]
AM_HD double ssb_agc_target() { return (double)(float)3276.8; }         // resize(n, n / 2, Real agcTarget)

// index in this feed of the first sample that closes a group, the counter being usc before the feed
AM_HD int ssb_first_close(unsigned usc, int decim) { return (int)((0u - usc) & (unsigned)(decim - 1)); }
AM_HD int ssb_closes(int n, int i0, int decim) { return n > i0 ? (n - 1 - i0) / decim + 1 : 0; }

AM_HD float ssb_smootherstep(float x)                       // util/stepfunctions.h:23-36
{
    if (x == 1.0f) return 1.0f; else if (x == 0.0f) return 0.0f;
    const double x3 = x * x * x, x4 = x * x3, x5 = x * x4;
    return (float)(6.0 * x5 - 15.0 * x4 + 10.0 * x3);
}

AM_HD double ssb_u0(double magsq, double sum, int hn, bool clamping)
{
    if (clamping) {
        const double rm = __builtin_sqrt(magsq);
        if (rm > SSB_CLAMP_MAX) return SSB_CLAMP_MAX / rm;
    }
    return ssb_agc_target() / __builtin_sqrt(sum / (double)hn);
}

AM_HD WfmClamp ssb_const(int v) { WfmClamp m; m.a = 0; m.lo = v; m.hi = v; return m; }
AM_HD WfmClamp ssb_gate_step(bool above, int gate)
{
    if (!above) return ssb_const(0);
    WfmClamp m; m.a = 1; m.lo = 0; m.hi = gate; return m;
}
AM_HD bool ssb_reset(bool above, int g_before, int gate) { return above && g_before >= gate; }
AM_HD WfmClamp ssb_count_step(bool reset, bool above, int hn)
{
    if (reset) return ssb_const(0);
    WfmClamp m; m.a = above ? 0 : 1; m.lo = 0; m.hi = hn; return m;
}
AM_HD bool ssb_up(int count, int hn) { return count < hn; }

struct SsbPair { int sel; WfmClamp u, d; };                // sel: 0 reads U, 1 reads D, -1 identity
struct SsbUD { int U, D; };

AM_HD SsbPair ssb_pair_identity(int L) { SsbPair m; m.sel = -1; m.u = wfm_identity(L); m.d = wfm_identity(L); return m; }
AM_HD SsbPair ssb_pair_step(bool up, int L)
{
    SsbPair m;
    m.u = wfm_identity(L); m.d = wfm_identity(L);
    if (up) { m.sel = 0; m.u.a = 1; } else { m.sel = 1; m.d.a = -1; }
    return m;
}
// first f, then g
AM_HD SsbPair ssb_pair_compose(SsbPair f, SsbPair g)
{
    if (f.sel < 0) return g;
    if (g.sel < 0) return f;
    const WfmClamp base = g.sel == 0 ? f.u : f.d;
    SsbPair r;
    r.sel = f.sel; r.u = wfm_compose(base, g.u); r.d = wfm_compose(base, g.d);
    return r;
}
AM_HD SsbUD ssb_pair_apply(SsbPair m, SsbUD s)
{
    if (m.sel < 0) return s;
    const int x = m.sel == 0 ? s.U : s.D;
    SsbUD r; r.U = wfm_apply(m.u, x); r.D = wfm_apply(m.d, x);
    return r;
}

// what feedAndGetValue returns with the threshold enabled: `was` the pair before this sample's step, `now` after it
AM_HD double ssb_agc_value(bool up, SsbUD was, SsbUD now, int L, double step_delta, double u0)
{
    if (up) return was.U < L ? u0 * ssb_smootherstep((float)(now.U * step_delta)) : u0;
    return was.D > 0 ? u0 * ssb_smootherstep((float)(now.D * step_delta)) : 0.0;
}
// getStepValue()
AM_HD float ssb_step_value(bool up, SsbUD now, double step_delta) { return ssb_smootherstep((float)((up ? now.U : now.D) * step_delta)); }

// the state the four counters carry, and one sample of them in the reference's statement order (the serial form the scan
// is checked against)
struct SsbCounters { int g, count; SsbUD ud; };
AM_HD bool ssb_counters_step(SsbCounters& s, bool above, int gate, int hn, SsbUD* was)
{
    const bool reset = ssb_reset(above, s.g, gate);
    s.g = wfm_apply(ssb_gate_step(above, gate), s.g);
    s.count = wfm_apply(ssb_count_step(reset, above, hn), s.count);
    const bool up = ssb_up(s.count, hn);
    *was = s.ud;
    s.ud = ssb_pair_apply(ssb_pair_step(up, hn / 2), s.ud);
    return up;
}

#if defined(__HIPCC__)
__device__ __forceinline__ SsbPair ssb_pair_shfl_up(SsbPair m, int o)
{
    SsbPair r; r.sel = __shfl_up(m.sel, o, 64); r.u = wfm_shfl_up(m.u, o); r.d = wfm_shfl_up(m.d, o);
    return r;
}
struct SsbPairOps {                                         // for wg_scan (demod_wg.hpp)
    using Map = SsbPair;
    int L;
    __device__ __forceinline__ SsbPair identity() const { return ssb_pair_identity(L); }
    __device__ __forceinline__ SsbPair compose(SsbPair f, SsbPair g) const { return ssb_pair_compose(f, g); }
    __device__ __forceinline__ SsbPair shfl_up(SsbPair m, int o) const { return ssb_pair_shfl_up(m, o); }
};

// ---- one 1024-sample trip of the three counter scans (4a-c) over a workgroup of 256 lanes, four consecutive samples per lane:
// ssb_gate_kernel's and udp_agc_kernel's.  Three wg_scans in a row on three slot arrays, no barrier of its own (demod_wg.hpp).
struct MagAgcSlots { WfmClamp g[4], c[4]; SsbPair p[4]; };  // __shared__, one per kernel

// Samples i0 .. i0 + 3 of this lane (those below n), the workgroup's lanes in stream order.  cap: where m_count stops (the step-down
// delay); magsq_at(i): m_magsq of sample i; sink(i, up, was, now, magsq): the pair before and after sample i's step.  st goes
// from the counters before the trip's first sample to those after its last, in every lane.
template <class Load, class Sink>
__device__ __forceinline__ void magagc_trip(SsbCounters& st, MagAgcSlots& slots, int i0, int n, int lane, int w, int gate, int cap, int L,
                                            double thr, Load magsq_at, Sink sink)
{
    const WfmClampOps gop{gate}, cop{cap};
    const SsbPairOps pop{L};
    bool above[4], rst[4], up[4];
    double magsq[4];
    WfmClamp gm = gop.identity();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        above[k] = false; magsq[k] = 0.0;
        if (i0 + k < n) {
            magsq[k] = magsq_at(i0 + k);
            above[k] = magsq[k] > thr;
            gm = wfm_compose(gm, ssb_gate_step(above[k], gate));
        }
    }
    // a. gate counter
    int g = wfm_apply(wg_scan(gop, gm, lane, w, slots.g), st.g);
    st.g = wfm_apply(wg_total(gop, slots.g), st.g);
    WfmClamp cm = cop.identity();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        rst[k] = false;
        if (i0 + k < n) {
            rst[k] = ssb_reset(above[k], g, gate);
            g = wfm_apply(ssb_gate_step(above[k], gate), g);
            cm = wfm_compose(cm, ssb_count_step(rst[k], above[k], cap));
        }
    }
    // b. m_count
    int cnt = wfm_apply(wg_scan(cop, cm, lane, w, slots.c), st.count);
    st.count = wfm_apply(wg_total(cop, slots.c), st.count);
    SsbPair pm = pop.identity();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        up[k] = false;
        if (i0 + k < n) {
            cnt = wfm_apply(ssb_count_step(rst[k], above[k], cap), cnt);
            up[k] = ssb_up(cnt, cap);
            pm = ssb_pair_compose(pm, ssb_pair_step(up[k], L));
        }
    }
    // c. the step pair
    SsbUD ud = ssb_pair_apply(wg_scan(pop, pm, lane, w, slots.p), st.ud);
    st.ud = ssb_pair_apply(wg_total(pop, slots.p), st.ud);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (i0 + k < n) {
            const SsbUD was = ud;
            ud = ssb_pair_apply(ssb_pair_step(up[k], L), ud);
            sink(i0 + k, up[k], was, ud, magsq[k]);
        }
    }
}
#endif

} // namespace sdrx
