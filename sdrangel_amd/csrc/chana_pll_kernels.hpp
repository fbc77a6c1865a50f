// ChannelAnalyzer bank, the PLL and the FLL: what ChannelAnalyzer::processOneSample does between m_magsq and feedOneSample when
// m_pll is set (plugins/channelrx/chanalyzer/chanalyzer.cpp:160-178), and feedOneSample's InputPLL (chanalyzer.h:254-262).
//     m_pll & !m_fll:  m_pll.feed(re, im);  mix = m_sum * std::conj(m_pll.getComplex())
//     m_pll &  m_fll:  m_fll.feed(re, im);  mix = m_sum * std::conj(m_fll.getComplex())
//     feedOneSample(m_pll ? mix : m_sum, m_fll ? m_fll.getComplex() : m_pll.getComplex())
// chana_group_kernel leaves m_sum of every closed group in `avg`.  feed() of either loop is one dependent chain per channel
// (pll_math.hpp has a step): chana_walk_kernel walks it and leaves the oscillator of every step in `osc`.  Everything behind is
// parallel again: chana_post_kernel makes the Sample, or fftcorr's input for the kernels of chana_kernels.hpp.
#pragma once
#include "chana_kernels.hpp"
#include "wave_walk.hpp"

namespace sdrx {

constexpr int CHANA_WALK_WAVES = 4;                     // channels per workgroup of the walk, one wave each

// ---- the serial walk, one wave per channel.  The chain never waits for memory: the wave loads 64 groups ahead, one per lane,
// while it steps through the 64 it holds; every lane takes step j's input from lane j's register and runs the same step (the
// loop's branches are then the wave's), lane j keeps the oscillator of step j, and the 64 go out in one store.  The state stays
// in registers from the first step of a feed to its last.
__global__ __launch_bounds__(64 * CHANA_WALK_WAVES)
void chana_walk_kernel(ChanaChan* __restrict__ ch, const ChanaBufs* __restrict__ bufs, int n_ch)
{
    // the wave's index is the same in all its lanes; said so, the step's values and branches are scalar to the compiler
    const int c = __builtin_amdgcn_readfirstlane(blockIdx.x * CHANA_WALK_WAVES + (int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (c >= n_ch) return;
    ChanaChan& s = ch[c];
    const PllCfg k = s.pk;
    if (k.mode == PLL_OFF) return;
    const ChanaBufs b = bufs[c];
    const int n = s.n_out;
    PllState st = s.ps;
    float2 next = lane < n ? walk_global_load(b.avg + lane) : make_float2(0.0f, 0.0f);
    for (int base = 0; base < n; base += 64) {
        const float2 cur = next;
        if (base + 64 + lane < n) next = walk_global_load(b.avg + base + 64 + lane);
        const float re = cur.x / 32768.0f, im = cur.y / 32768.0f;             // SDR_RX_SCALEF
        const int cnt = min(64, n - base);
        float2 mine = make_float2(0.0f, 0.0f);
        for (int j = 0; j < cnt; j++) {
            const float r = walk_lane_value(re, j), i = walk_lane_value(im, j);
            float yr, yi;
            if (k.mode == PLL_FREQ) pll_freq_step(k, st, r, i, &yr, &yi, (PllProbe*)nullptr);
            else pll_phase_step(k, st, r, i, &yr, &yi, (PllProbe*)nullptr);
            if (lane == j) mine = make_float2(yr, yi);
        }
        if (base + lane < n) walk_global_store(b.osc + base + lane, mine);
    }
    if (lane == 0) s.ps = st;
}

// ---- per closed group of a channel with m_pll or InputPLL: the Sample, or fftcorr's input
__global__ __launch_bounds__(256)
void chana_post_kernel(const ChanaChan* __restrict__ ch, const ChanaBufs* __restrict__ bufs)
{
    const int c = blockIdx.y;
    const ChanaChan& s = ch[c];
    if (!chana_has_post(s)) return;
    const long o = (long)blockIdx.x * 256 + threadIdx.x;
    if (o >= s.n_out) return;
    const ChanaBufs& b = bufs[c];
    const bool fed = s.pk.mode != PLL_OFF;
    const float2 sum = b.avg[o];
    const float2 y = fed ? b.osc[o] : make_float2(1.0f, 0.0f);                // an unfed loop's m_y
    const float2 sig = fed ? c_mul(sum, make_float2(y.x, -y.y)) : sum;         // m_sum * std::conj(y)
    float2 v = sig;
    if (s.osc_out) v = make_float2(y.x * 32768.0f, y.y * 32768.0f);
    else if (s.corr) {
        const float k = 32768.0f / 768.0f;
        b.g[o] = make_float2(sig.x / k, sig.y / k);
        return;
    }
    const int o_re = sdrx_to_q16(s.swap_iq ? v.y : v.x), o_im = sdrx_to_q16(s.swap_iq ? v.x : v.y);
    reinterpret_cast<short2*>(b.out)[o] = make_short2((short)o_re, (short)o_im);
}

} // namespace sdrx
