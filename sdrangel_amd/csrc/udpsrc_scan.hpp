// The recurrences of UDPSrc::feed's per-sample loop (plugins/channelrx/udpsrc/udpsrc.cpp:136-321, udpsrc.h:238-294) cut into
// terms that can be computed in parallel.  Stream indexing (am_stream_at / am_hist_next) is am_scan.hpp's.  Compiles for the
// host too (tests/udpsrc_scan_check.cpp), no HIP header needed.
//
// 1. m_inMovingAverage / m_amMovingAverage (MovingAverage<double>): m_sum += value - oldest, the history before the stream
//    being 1e-10 and the sum starting at size * 1e-10: a rounded prefix sum of terms known in advance (psum_rows).
// 2. calculateSquelch.  From either initSquelch state the triple (m_squelchOpen, m_squelchOpenCount, m_squelchCloseCount) only
//    takes two kinds of value: closed with openCount in 0..G and closeCount 0, or open with openCount G and closeCount in 0..R.
//    That is one chain of G + R + 2 positions p (udp_sq_pos): p = openCount when closed, p = G + 1 + closeCount when open, and
//        above:  p -> p < G ? p + 1 : TOP          TOP = G + 1 + R
//        below:  p -> p > G + 1 ? p - 1 : 0
//    Both are monotone.  A run of k aboves is  p <= G - k ? p + k : TOP,  a run of k belows  p >= G + 1 + k ? p - k : 0,  and
//    as soon as both kinds have occurred the image has at most two points, so the map is a monotone step  p < t ? c1 : c2.
//    All of them are members of
//        f(p) = p < lo ? c_lo : (p > hi ? c_hi : p + a)                                         (UdpSq)
//    and udp_sq_compose gives the member for "first f, then g" of any two maps that strings of steps produce
//    (tests/udpsrc_scan_check.cpp checks it exhaustively against the literal automaton).  m_squelchGate == 0 is the stateless
//    case -- the flag follows `above`, the counters never move -- which the chain gives with G = R = 0 (udp_sq_release).
// 3. The discriminator (formats 2, 3), m_amMovingAverage (9) and the Bandpass (10) advance on open samples only: they run on
//    the compacted sequence of open samples, the previous open sample being element a - 1 of it (a = 0: the carried one).
#pragma once
#include "ssb_scan.hpp"

namespace sdrx {

// UDPSrcSettings::SampleFormat
enum { UDP_IQ16 = 0, UDP_IQ24 = 1, UDP_NFM = 2, UDP_NFM_MONO = 3, UDP_LSB = 4, UDP_USB = 5, UDP_LSB_MONO = 6, UDP_USB_MONO = 7,
       UDP_AM_MONO = 8, UDP_AM_NODC_MONO = 9, UDP_AM_BPF_MONO = 10 };

AM_HD double udp_ma_initial() { return 1e-10; }             // MovingAverage<double>::resize(n, 1e-10)
AM_HD double udp_ma_term(double cur, double oldest) { return cur - oldest; }
// inMagSq / (SDR_RX_SCALED * SDR_RX_SCALED), inMagSq the double of a float sum of squares
AM_HD double udp_in_power(float raw) { return (double)raw / (32768.0 * 32768.0); }
AM_HD bool udp_above(double sum, int window, bool enabled, double level) { return !enabled || sum / (double)window > level; }

// ---- MagAGC as UDPSrc sets it up (agc.cpp:98-182, udpsrc.cpp:101-102, 531-534, 579): constructed (9600, 16384.0f, 1e-6), clampMax
// 2^30 with clamping on, m_squared false, the threshold enabled; resize(rate / 5, rate / 20, 16384) leaves the history 0, the sum
// 0, m_stepUpCounter 0 and m_stepDownCounter = the step length.  The gate counter, m_count and the step pair are ssb_scan.hpp's
// scans as they are, with the step-down delay where SSB has hn and the step length given instead of hn / 2; the history sum is
// a rounded prefix sum of magsq[j] - magsq[j - hn] (psum_rows).  Only m_u0 has other constants here.
AM_HD double udp_agc_target() { return (double)16384.0f; }
AM_HD double udp_agc_clamp_max() { return 32768.0 * 32768.0; }
AM_HD double udp_agc_u0(double magsq, double sum, int hn)
{
    const double rm = __builtin_sqrt(magsq);
    if (rm > udp_agc_clamp_max()) return udp_agc_clamp_max() / rm;
    return udp_agc_target() / __builtin_sqrt(sum / (double)hn);
}

// ---- the squelch chain
AM_HD int udp_sq_release(int G, int R) { return G == 0 ? 0 : R; }
AM_HD int udp_sq_top(int G, int R) { return G + 1 + R; }
AM_HD int udp_sq_pos(bool open, int open_count, int close_count, int G) { return open ? G + 1 + close_count : open_count; }
AM_HD bool udp_sq_open(int p, int G) { return p > G; }
AM_HD int udp_sq_open_count(int p, int G) { return p > G ? G : p; }
AM_HD int udp_sq_close_count(int p, int G) { return p > G ? p - G - 1 : 0; }
AM_HD int udp_sq_step(int p, bool above, int G, int top) { return above ? (p < G ? p + 1 : top) : (p > G + 1 ? p - 1 : 0); }

struct UdpSq { int lo, hi, c_lo, c_hi, a; };               // p < lo ? c_lo : (p > hi ? c_hi : p + a)

AM_HD int udp_sq_apply(UdpSq m, int p) { return p < m.lo ? m.c_lo : (p > m.hi ? m.c_hi : p + m.a); }
AM_HD UdpSq udp_sq_identity(int top) { UdpSq m; m.lo = 0; m.hi = top; m.c_lo = 0; m.c_hi = top; m.a = 0; return m; }
AM_HD UdpSq udp_sq_map(bool above, int G, int top)
{
    UdpSq m;
    if (above) { m.lo = 0; m.hi = G - 1; m.c_lo = 0; m.c_hi = top; m.a = 1; }
    else { m.lo = G + 2; m.hi = top; m.c_lo = 0; m.c_hi = top; m.a = -1; }
    return m;
}
// first f, then g.  Where both shift on a common stretch the result is a shift with one constant on either side (a pure run);
// otherwise it is a step with at most two values, whose threshold is one of the four breakpoints.
AM_HD UdpSq udp_sq_compose(UdpSq f, UdpSq g, int top)
{
    UdpSq r;
    const int sl = f.lo > g.lo - f.a ? f.lo : g.lo - f.a, sh = f.hi < g.hi - f.a ? f.hi : g.hi - f.a;
    if (sl <= sh && sl <= top && sh >= 0) {
        r.lo = sl < 0 ? 0 : sl; r.hi = sh > top ? top : sh; r.a = f.a + g.a;
        r.c_lo = r.lo > 0 ? udp_sq_apply(g, udp_sq_apply(f, r.lo - 1)) : 0;
        r.c_hi = r.hi < top ? udp_sq_apply(g, udp_sq_apply(f, r.hi + 1)) : top;
        return r;
    }
    r.a = 0;
    r.c_lo = udp_sq_apply(g, udp_sq_apply(f, 0));
    r.c_hi = udp_sq_apply(g, udp_sq_apply(f, top));
    int t = top + 1;                                        // the smallest p that gives c_hi
    const int cand[4] = { f.lo, f.hi + 1, g.lo - f.a, g.hi - f.a + 1 };
    for (int i = 0; i < 4; i++) {
        const int p = cand[i] < 0 ? 0 : (cand[i] > top ? top : cand[i]);
        if (p < t && udp_sq_apply(g, udp_sq_apply(f, p)) == r.c_hi) t = p;
    }
    if (r.c_lo == r.c_hi) t = 0;
    r.lo = t; r.hi = t - 1;
    return r;
}

// ---- Bandpass<double>::filter (bandpass.h:77-122) on the compacted sequence: Real taps, double samples and accumulator;
// X(k) = the value k open samples back, the walk as am_bandpass
template <class F> AM_HD double udp_bandpass(const float* taps, F X)
{
    double acc = 0.0;
    acc += (X(0) + X(1)) * taps[0];
    for (int i = 1; i < AM_BP_H; i++) acc += (X(AM_BP_TAPS - i) + X(1 + i)) * taps[i];
    acc += X(AM_BP_H + 1) * taps[AM_BP_H];
    return acc;
}

// ---- payload conversions (x86-64, strict IEEE): an implicit float -> qint16 is cvttss2si and the low 16 bits, a double ->
// int16_t cvttsd2si and the low 16 bits; out of the int32 range (and NaN) either instruction gives 0x80000000, i.e. 0
AM_HD int udp_q16f(float v)
{
    const int i = (v >= -2147483648.0f && v < 2147483648.0f) ? (int)v : (int)0x80000000u;
    return (int)(short)i;
}
AM_HD int udp_q16d(double v)
{
    const int i = (v > -2147483649.0 && v < 2147483648.0) ? (int)v : (int)0x80000000u;
    return (int)(short)i;
}

// ---- std::arg(Complex) = atan2f for formats 2 and 3.  The payload is (int16)(arg / pi * fm_scaling * gain * 32768): at
// fm_scaling * gain = 720 one ulp of the angle near pi is two units of the int16, so "within a few ulp of the host's libm" is
// not enough there.  This is the evaluation of the fdlibm float routines (e_atan2f.c, s_atanf.c: argument reduction to four
// intervals, an odd polynomial of degree 23 in two interleaved halves, hi + lo constants), which glibc's atan2f was up to 2.40,
// operation for operation in float; with -ffp-contract=off and IEEE division it returns that libm's bits on the host and on the
// device (tests/udpsrc_scan_check.cpp compares it with the host's atan2f).  NaN and infinite arguments follow the same routine.
AM_HD int udp_f2i(float v) { int i; __builtin_memcpy(&i, &v, 4); return i; }
AM_HD float udp_atanf(float x)
{
    const float hi[4] = { 4.6364760399e-01f, 7.8539812565e-01f, 9.8279368877e-01f, 1.5707962513e+00f };     // atan(0.5), atan(1), atan(1.5), atan(inf)
    const float lo[4] = { 5.0121582440e-09f, 3.7748947079e-08f, 3.4473217170e-08f, 7.5497894159e-08f };
    const float t0 = 3.3333334327e-01f, t1 = -2.0000000298e-01f, t2 = 1.4285714924e-01f, t3 = -1.1111110449e-01f, t4 = 9.0908870101e-02f,
                t5 = -7.6918758452e-02f, t6 = 6.6610731184e-02f, t7 = -5.8335702866e-02f, t8 = 4.9768779427e-02f, t9 = -3.6531571299e-02f,
                t10 = 1.6285819933e-02f;
    const int hx = udp_f2i(x), ix = hx & 0x7fffffff;
    int id = -1;
    if (ix >= 0x4c000000) {                                 // |x| >= 2^25
        if (ix > 0x7f800000) return x + x;
        return hx > 0 ? hi[3] + lo[3] : -hi[3] - lo[3];
    }
    if (ix < 0x3ee00000) {                                  // |x| < 0.4375
        if (ix < 0x31000000) return x;                      // |x| < 2^-29
    } else {
        x = __builtin_fabsf(x);
        if (ix < 0x3f980000) {                              // |x| < 1.1875
            if (ix < 0x3f300000) { id = 0; x = (2.0f * x - 1.0f) / (2.0f + x); }
            else { id = 1; x = (x - 1.0f) / (x + 1.0f); }
        } else {
            if (ix < 0x401c0000) { id = 2; x = (x - 1.5f) / (1.0f + 1.5f * x); }     // |x| < 2.4375
            else { id = 3; x = -1.0f / x; }
        }
    }
    const float z = x * x, w = z * z;
    const float s1 = z * (t0 + w * (t2 + w * (t4 + w * (t6 + w * (t8 + w * t10)))));
    const float s2 = w * (t1 + w * (t3 + w * (t5 + w * (t7 + w * t9))));
    if (id < 0) return x - x * (s1 + s2);
    const float r = hi[id] - ((x * (s1 + s2) - lo[id]) - x);
    return hx < 0 ? -r : r;
}
AM_HD float udp_atan2f(float y, float x)
{
    const float tiny = 1.0e-30f, pi_o_4 = 7.8539818525e-01f, pi_o_2 = 1.5707963705e+00f, pi = 3.1415927410e+00f, pi_lo = -8.7422776573e-08f;
    const int hx = udp_f2i(x), ix = hx & 0x7fffffff, hy = udp_f2i(y), iy = hy & 0x7fffffff;
    if (ix > 0x7f800000 || iy > 0x7f800000) return x + y;   // NaN
    if (hx == 0x3f800000) return udp_atanf(y);              // x = 1
    const int m = ((hy >> 31) & 1) | ((hx >> 30) & 2);      // 2 * sign(x) + sign(y)
    if (iy == 0) return m < 2 ? y : (m == 2 ? pi + tiny : -pi - tiny);
    if (ix == 0) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
    if (ix == 0x7f800000) {
        if (iy == 0x7f800000) return m == 0 ? pi_o_4 + tiny : (m == 1 ? -pi_o_4 - tiny : (m == 2 ? 3.0f * pi_o_4 + tiny : -3.0f * pi_o_4 - tiny));
        return m == 0 ? 0.0f : (m == 1 ? -0.0f : (m == 2 ? pi + tiny : -pi - tiny));
    }
    if (iy == 0x7f800000) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
    const int k = (iy - ix) >> 23;
    float z;
    if (k > 60) z = pi_o_2 + 0.5f * pi_lo;                  // |y / x| > 2^60
    else if (hx < 0 && k < -60) z = 0.0f;                   // |y| / x < -2^60
    else z = udp_atanf(__builtin_fabsf(y / x));
    return m == 0 ? z : (m == 1 ? -z : (m == 2 ? pi - (z - pi_lo) : (z - pi_lo) - pi));
}

#if defined(__HIPCC__)
__device__ __forceinline__ UdpSq udp_sq_shfl_up(UdpSq m, int o)
{
    UdpSq r;
    r.lo = __shfl_up(m.lo, o, 64); r.hi = __shfl_up(m.hi, o, 64); r.c_lo = __shfl_up(m.c_lo, o, 64); r.c_hi = __shfl_up(m.c_hi, o, 64);
    r.a = __shfl_up(m.a, o, 64);
    return r;
}
struct UdpSqOps {                                           // for wg_scan (demod_wg.hpp)
    using Map = UdpSq;
    int top;
    __device__ __forceinline__ UdpSq identity() const { return udp_sq_identity(top); }
    __device__ __forceinline__ UdpSq compose(UdpSq f, UdpSq g) const { return udp_sq_compose(f, g, top); }
    __device__ __forceinline__ UdpSq shfl_up(UdpSq m, int o) const { return udp_sq_shfl_up(m, o); }
};
#endif

} // namespace sdrx
