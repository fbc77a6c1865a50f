// The two recurrences of WFMDemod::feed's per-sample loop (plugins/channelrx/demodwfm/wfmdemod.cpp:121-140) as
// associative scan operators.  Compiles for the host too (tests/wfm_scan_check.cpp), no HIP header needed; the shuffle and the
// ops struct at the end are there for hipcc only (the scans that use them: demod_wg.hpp).
//
// 1. Squelch counter.  `if (magsq >= level) { if (state < rfBW / 10) state++; } else { if (state > 0) state--; }` with an
//    int state compared against a float.  With H = the smallest integer that is not below the float bound (wfm_counter_cap),
//    the state never leaves [0, H] and a step is  s -> min(s + 1, H)  or  s -> max(s - 1, 0).  Both are members of
//        f(s) = clamp(s + a, lo, hi),   lo <= hi
//    and that family is closed under composition:
//        g(f(s)) = clamp(s + (a_f + a_g), clamp(lo_f + a_g, lo_g, hi_g), clamp(hi_f + a_g, lo_g, hi_g))
//    so the state after every sample is an inclusive prefix scan of the step maps applied to the carried state.
// 2. m_prevArg.  The discriminator runs on open samples only, so the previous argument of sample i is the argument of the
//    last open sample before i: an exclusive max-scan of (open ? index : -1); -1 = the value carried in.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WFM_HD __host__ __device__ __forceinline__
#else
#define WFM_HD inline
#endif

namespace sdrx {

struct WfmClamp { int a, lo, hi; };                        // s -> clamp(s + a, lo, hi)

WFM_HD int wfm_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
WFM_HD WfmClamp wfm_step(bool up, int cap) { WfmClamp m; m.a = up ? 1 : -1; m.lo = 0; m.hi = cap; return m; }
WFM_HD WfmClamp wfm_identity(int cap) { WfmClamp m; m.a = 0; m.lo = 0; m.hi = cap; return m; }
WFM_HD int wfm_apply(WfmClamp m, int s) { return wfm_clampi(s + m.a, m.lo, m.hi); }
// first f, then g
WFM_HD WfmClamp wfm_compose(WfmClamp f, WfmClamp g)
{
    WfmClamp r;
    r.a = f.a + g.a;
    r.lo = wfm_clampi(f.lo + g.a, g.lo, g.hi);
    r.hi = wfm_clampi(f.hi + g.a, g.lo, g.hi);
    return r;
}
// the counter's saturation value: the smallest H >= 0 with !((float)H < bound), i.e. where `state < bound` first fails
WFM_HD int wfm_counter_cap(float bound)
{
    if (!(bound > 0.0f)) return 0;
    int h = (int)bound;                                     // truncation: h <= bound
    while ((float)h < bound) h++;
    while (h > 0 && !((float)(h - 1) < bound)) h--;
    return h;
}
// last-open scan: combine = max
WFM_HD int wfm_last_open(int left, int right) { return left > right ? left : right; }

#if defined(__HIPCC__)
__device__ __forceinline__ WfmClamp wfm_shfl_up(WfmClamp m, int o)
{
    WfmClamp r; r.a = __shfl_up(m.a, o, 64); r.lo = __shfl_up(m.lo, o, 64); r.hi = __shfl_up(m.hi, o, 64);
    return r;
}
struct WfmClampOps {                                        // what wg_wave_scan / wg_scan (demod_wg.hpp) ask of a map type
    using Map = WfmClamp;
    int cap;
    __device__ __forceinline__ WfmClamp identity() const { return wfm_identity(cap); }
    __device__ __forceinline__ WfmClamp compose(WfmClamp f, WfmClamp g) const { return wfm_compose(f, g); }
    __device__ __forceinline__ WfmClamp shfl_up(WfmClamp m, int o) const { return wfm_shfl_up(m, o); }
};
#endif

} // namespace sdrx
