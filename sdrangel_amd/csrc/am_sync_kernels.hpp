// AM demodulator bank, synchronous AM: what AMDemod::processOneSample does with an open, unmuted sample when m_pll is set
// (plugins/channelrx/demodam/amdemod.cpp:191-238), for the channels of a handle made with sdrx_am_create_ex.
//     s = m_pllFilt.filter(complex(re, im));  m_pll.feed(s.real(), s.imag())
//     cs = (re * m_pll.getImag() - im * m_pll.getReal(), re * m_pll.getReal() + im * m_pll.getImag())
//     n = DSBFilter->runDSB(cs, &sb, false)  or  SSBFilter->runSSB(cs, &sb, usb, false)
//     i < n: m_syncAMBuff[i] = z.real() + z.imag(), z = sb[i] * (float) m_syncAMAGC.feedAndGetValue(sb[i]); index = 0
//     demod = m_syncAMBuff[index++] * 4.0f
// These kernels run between am_gate_kernel (the compaction indices aidx, n_act) and am_out_kernel (Bandpass, attack and
// conversion over the compacted `dem`), behind am_demod_kernel, whose envelope value of a sync channel am_sync_select_kernel
// replaces.  am_sync_scan.hpp has the cut of the chain and the index arithmetic; DESIGN.md 4.10 the kernel table.  The only
// loop that is serial along time is the walk's: everything else is one lane per sample or one workgroup per block.
// Float rules as in am_kernels.hpp: reference operand order, -ffp-contract=off.
#pragma once
#include "am_kernels.hpp"
#include "gfft_kernel.hpp"
#include "wave_walk.hpp"

namespace sdrx {

constexpr int AM_WALK_WAVES = 4;                            // channels per workgroup of the walk, one wave each

// the filter's input for compacted index q of this feed (q < 0: carried, already turned)
__device__ __forceinline__ float2 ams_input(const AmBufs& b, int pend, int q)
{
    return q < 0 ? b.pend[pend + q] : ams_rotate(b.xc[q], b.osc[q]);
}
// filter output o of this feed: output[i] = ovlbuf[i] + data[i]
__device__ __forceinline__ float2 ams_sideband(const AmBufs& b, int B, int o)
{
    const float2 v = o < B ? b.ovl[o] : b.tail[o - B], h = b.head[o];
    float2 r; r.x = v.x + h.x; r.y = v.y + h.y;
    return r;
}
// zsum of filter output o of this feed (o < 0: carried)
__device__ __forceinline__ float ams_zsum_at(const AmChan& s, const AmBufs& b, int o)
{
    if (o < 0) return b.zhist[s.s_B + o];
    return ams_zsum(ams_sideband(b, s.s_B, o), ams_u0(b.stot[o], s.s_hn));
}

// ---- S1. per sample: an open one's (re, im) into the compacted sequence; the number of blocks this feed completes
__global__ __launch_bounds__(256)
void am_sync_pack_kernel(AmChan* __restrict__ ch, const AmBufs* __restrict__ bufs)
{
    const int c = blockIdx.y;
    AmChan& s = ch[c];
    if (!s.sync) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) s.s_nb = ams_blocks(s.s_pend, s.n_act, s.s_B);
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= s.n) return;
    const AmBufs& b = bufs[c];
    const int a = b.aidx[i];
    if (a < 0) return;
    const float2 v = b.ci[i];
    b.xc[a] = make_float2(v.x / 32768.0f, v.y / 32768.0f);  // SDR_RX_SCALEF
}

// ---- S2. per open sample: m_pllFilt over the compacted sequence (one lane per open sample, taps from LDS)
__global__ __launch_bounds__(256)
void am_sync_prefilt_kernel(const AmChan* __restrict__ ch, const AmBufs* __restrict__ bufs, const float* __restrict__ tap_table)
{
    __shared__ float taps[AMS_PF_H + 1];
    const int c = blockIdx.y;
    const AmChan& s = ch[c];
    if (!s.sync || (long)blockIdx.x * 256 >= s.n_act) return;
    if (threadIdx.x <= AMS_PF_H) taps[threadIdx.x] = tap_table[s.pf_off + threadIdx.x];
    __syncthreads();
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= s.n_act) return;
    const AmBufs& b = bufs[c];
    const float2* __restrict__ hist = b.xhist;
    const float2* __restrict__ cur = b.xc;
    b.pf[a] = ams_prefilter<float2>(taps, [&](int k) { return am_stream_at(hist, AMS_PF_HIST, cur, (long)a - k); });
}

// ---- S3. the serial walk, one wave per sync channel, as chana_walk_kernel: the wave loads 64 filtered samples ahead, one per
// lane, while it steps through the 64 it holds; every lane takes step j's input from lane j's register and runs the same step
// (pll_phase_step, pll_math.hpp: the loop's branches are then the wave's), lane j keeps (m_yRe, m_yIm) of step j, and the 64 go
// out in one store.  The state stays in registers from the first step of a feed to its last.
__global__ __launch_bounds__(64 * AM_WALK_WAVES)
void am_sync_walk_kernel(AmChan* __restrict__ ch, const AmBufs* __restrict__ bufs, int n_ch)
{
    const int c = __builtin_amdgcn_readfirstlane(blockIdx.x * AM_WALK_WAVES + (int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (c >= n_ch) return;
    AmChan& s = ch[c];
    if (!s.sync) return;
    const PllCfg k = s.pk;
    const AmBufs b = bufs[c];
    const int n = s.n_act;
    if (n <= 0) return;
    PllState st = s.ps;
    float2 next = lane < n ? walk_global_load(b.pf + lane) : make_float2(0.0f, 0.0f);
    for (int base = 0; base < n; base += 64) {
        const float2 cur = next;
        if (base + 64 + lane < n) next = walk_global_load(b.pf + base + 64 + lane);
        const int cnt = min(64, n - base);
        float2 mine = make_float2(0.0f, 0.0f);
        for (int j = 0; j < cnt; j++) {
            const float r = walk_lane_value(cur.x, j), i = walk_lane_value(cur.y, j);
            float yr, yi;
            pll_phase_step(k, st, r, i, &yr, &yi, (PllProbe*)nullptr);
            if (lane == j) mine = make_float2(yr, yi);
        }
        if (base + lane < n) walk_global_store(b.osc + base + lane, mine);
    }
    if (lane == 0) s.ps = st;
}

// ---- S4. one workgroup per (channel, completed block): the B turned samples zero-padded to N = 2 B, forward g_fft, the bin
// rule of runDSB / runSSB with getDC = false, inverse g_fft; the two halves go to head / tail as in be_fft_kernel.
//     runDSB: data[i] *= filter[i] for every bin, then data[0] = 0
//     runSSB: data[0] = 0; usb: data[i] *= filter[i], data[B + i] = 0 for 0 < i < B; lsb the other way round; bin B stays
template <int N>
__global__ __launch_bounds__(N / 8)
void am_sync_fft_kernel(const AmChan* __restrict__ ch, const AmBufs* __restrict__ bufs, const float2* __restrict__ filters,
                        const float* __restrict__ utbl)
{
    constexpr int NT = N / 8, H = N / 2;
    __shared__ float2 xa[N], ya[N];
    __shared__ float us[N / 4 + 1];
    const int c = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    const AmChan& s = ch[c];
    if (!s.sync || s.s_B != H || blk >= s.s_nb) return;
    const AmBufs& b = bufs[c];
    const int pend = s.s_pend, sync = s.sync;
    for (int i = tid; i <= N / 4; i += NT) us[i] = utbl[i];
    for (int j = tid; j < H; j += NT) {
        xa[j] = ams_input(b, pend, ams_block_source(pend, H, blk, j));
        xa[H + j] = make_float2(0.0f, 0.0f);
    }
    __syncthreads();
    gfft<N, false>(ya, xa, us, tid);
    const float2* __restrict__ filt = filters + s.filt_off;
    const float2 zero = make_float2(0.0f, 0.0f);
    for (int i = tid; i < H; i += NT) {
        float2 lo = ya[i], hi = ya[H + i];
        if (sync == AMS_DSB) { lo = i == 0 ? zero : c_mul(lo, filt[i]); hi = c_mul(hi, filt[H + i]); }
        else if (i == 0) lo = zero;
        else if (sync == AMS_USB) { lo = c_mul(lo, filt[i]); hi = zero; }
        else { lo = zero; hi = c_mul(hi, filt[H + i]); }
        xa[i] = lo; xa[H + i] = hi;
    }
    __syncthreads();
    gfft<N, true>(ya, xa, us, tid);
    for (int i = tid; i < H; i += NT) {
        b.head[(size_t)blk * H + i] = ya[i];
        b.tail[(size_t)blk * H + i] = ya[H + i];
    }
}

// ---- S5. per filter output: magsq and the moving-average term
__global__ __launch_bounds__(256)
void am_sync_power_kernel(const AmChan* __restrict__ ch, const AmBufs* __restrict__ bufs)
{
    const int c = blockIdx.y;
    const AmChan& s = ch[c];
    if (!s.sync) return;
    const int B = s.s_B, hn = s.s_hn, no = s.s_nb * B;
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= no) return;
    const AmBufs& b = bufs[c];
    const float p = ams_magsq(ams_sideband(b, B, o));
    const float old = o >= hn ? ams_magsq(ams_sideband(b, B, o - hn)) : b.phist[o];
    b.pw[o] = p;
    b.sterm[o] = ams_agc_term(p, old);
}

// ---- S6. the moving-average sum after every filter output: one wave per 16 channels (psum_rows); envelope channels have no terms
__global__ __launch_bounds__(64)
void am_sync_psum_kernel(AmChan* __restrict__ ch, const AmBufs* __restrict__ bufs, int n_ch)
{
    // psum_rows loads a row's first term whatever its count: an envelope channel, which has no sterm, names its dterm / tot
    psum_channels(n_ch, [&](int c) {
        const bool on = ch[c].sync != AMS_OFF;
        return PsumRow{on ? bufs[c].sterm : bufs[c].dterm, on ? bufs[c].stot : bufs[c].tot, on ? ch[c].s_nb * ch[c].s_B : 0, ch[c].s_total, &ch[c].s_total_next};
    });
}

// ---- S7. per open sample: what m_syncAMBuff[m_syncAMBuffIndex++] holds for it, times 4, into the compacted demod sequence
__global__ __launch_bounds__(256)
void am_sync_select_kernel(const AmChan* __restrict__ ch, const AmBufs* __restrict__ bufs)
{
    const int c = blockIdx.y;
    const AmChan& s = ch[c];
    if (!s.sync) return;
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= s.n_act) return;
    const AmBufs& b = bufs[c];
    b.dem[a] = ams_zsum_at(s, b, ams_select_index(s.s_pend, a, s.s_B)) * 4.0f;
}

// ---- S8. carry: the histories of the next feed (double-buffered: this feed's are still being read), the open block, the sum
// and the counts.  m_pll's state was left by the walk.
__global__ __launch_bounds__(256)
void am_sync_carry_kernel(AmChan* __restrict__ ch, const AmBufs* __restrict__ bufs)
{
    const int c = blockIdx.x, tid = threadIdx.x;
    AmChan& s = ch[c];
    if (!s.sync) return;
    const AmBufs b = bufs[c];
    const int na = s.n_act, pend = s.s_pend, B = s.s_B, hn = s.s_hn, nb = s.s_nb, no = nb * B;
    const int left = ams_left(pend, na, B);
    for (int i = tid; i < AMS_PF_HIST; i += 256) b.xhist_next[i] = am_hist_next(b.xhist, AMS_PF_HIST, (const float2*)b.xc, na, i);
    for (int i = tid; i < B; i += 256) {
        b.pend_next[i] = i < left ? ams_input(b, pend, ams_block_source(pend, B, nb, i)) : make_float2(0.0f, 0.0f);
        b.ovl_next[i] = nb > 0 ? b.tail[(size_t)(nb - 1) * B + i] : b.ovl[i];
        b.zhist_next[i] = ams_zsum_at(s, b, no - B + i);
    }
    for (int i = tid; i < hn; i += 256) b.phist_next[i] = am_hist_next(b.phist, hn, (const float*)b.pw, no, i);
    __syncthreads();                                        // every lane has read s_pend
    if (tid == 0) { s.s_pend = left; s.s_open += na; s.s_total = s.s_total_next; }
}

} // namespace sdrx
