// Wideband-FM demodulator bank kernels: WFMDemod::feed (plugins/channelrx/demodwfm/wfmdemod.cpp:90-183)
//     c = Complex(re, im) * m_nco.nextIQ();                                NCO            sdrbase/dsp/nco.cpp:30-64
//     rf_out = m_rfFilter->runFilt(c, &rf);                                 fftfilt 1024   fftfilt.cpp:261-282 (g_fft)
//     for each rf[i]: magsq, level sums, squelch counter, gated phaseDiscriminatorDelta   phasediscri.h:61-78
//                     m_interpolator.decimate(&dist, Complex(demod, 0), &ci)              interpolator.h:23-36,182-195
//                     (qint16)(ci.real() * 3276.8f * volume)
// Audio is bit-identical to the strict-IEEE scalar reference build: every float expression keeps the reference's operand
// order and the file is compiled with -ffp-contract=off.  DESIGN.md 4.9 has the kernel cut and what bounds each kernel.
//
// Steps 1, 2, 4 and 8 and the FIR's accumulation are fm_front.hpp's device functions, which sdrx_bfm_* runs too.
#pragma once
#include "fm_front.hpp"

namespace sdrx {

// ---- 1. the resampler schedule, 2. the filter blocks and the pending samples: fm_front.hpp
__global__ void wfm_prep_kernel(WfmChan* __restrict__ ch, const WfmBufs* __restrict__ bufs, int n_ch)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n_ch) wfm_prep_body(ch[c], bufs[c]);
}

__global__ void __launch_bounds__(256) wfm_sched_fill_kernel(const WfmChan* __restrict__ ch, const WfmBufs* __restrict__ bufs)
{
    wfm_sched_fill_body(ch[blockIdx.y], bufs[blockIdx.y]);
}

__global__ void wfm_sched_walk_kernel(WfmChan* __restrict__ ch, const WfmBufs* __restrict__ bufs, int n_ch)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n_ch) wfm_sched_walk_body(ch[c], bufs[c]);
}

__global__ __launch_bounds__(WFM_FFT / 8)
void wfm_fft_kernel(const WfmChan* __restrict__ ch, const WfmBufs* __restrict__ bufs, const float2* __restrict__ filters,
                    const float* __restrict__ utbl, const float* __restrict__ nco_tbl)
{
    wfm_fft_body<false>(ch[blockIdx.y], bufs[blockIdx.y], filters, utbl, nco_tbl);
}

__global__ __launch_bounds__(WFM_H)
void wfm_pend_kernel(const WfmChan* __restrict__ ch, const WfmBufs* __restrict__ bufs)
{
    wfm_pend_body(ch[blockIdx.x], bufs[blockIdx.x]);
}

// ---- 3. overlap-add, level statistics, squelch flag and the argument of every filtered sample; per block the composed
// counter map, the magsq sum and peak.  256 threads, two consecutive samples each.
__global__ __launch_bounds__(256)
void wfm_level_kernel(const WfmChan* __restrict__ ch, const WfmBufs* __restrict__ bufs)
{
    __shared__ WfmClamp maps[256];
    __shared__ double sums[256];
    __shared__ float peaks[256];
    const int c = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    const WfmChan& s = ch[c];
    if (blk >= s.n_blocks) return;
    const WfmBufs b = bufs[c];
    const long j0 = (long)blk * WFM_H + 2 * tid;
    const float4 o = *reinterpret_cast<const float4*>(b.tail + j0), h = *reinterpret_cast<const float4*>(b.head + j0);
    float2 r0, r1;                                          // output[i] = ovlbuf[i] + data[i] (tail slots are shifted by one block)
    r0.x = o.x + h.x; r0.y = o.y + h.y; r1.x = o.z + h.z; r1.y = o.w + h.w;
    const float level = s.squelch_level;
    const double scale = 32768.0 * 32768.0;                 // SDR_RX_SCALED * SDR_RX_SCALED
    const double msq0 = (double)(r0.x * r0.x + r0.y * r0.y), msq1 = (double)(r1.x * r1.x + r1.y * r1.y);
    const float mag0 = (float)(msq0 / scale), mag1 = (float)(msq1 / scale);
    const bool f0 = mag0 >= level, f1 = mag1 >= level;
    *reinterpret_cast<float2*>(b.arg + j0) = make_float2(atan2_approx2(r0.y, r0.x), atan2_approx2(r1.y, r1.x));
    *reinterpret_cast<uchar2*>(b.flag + j0) = make_uchar2(f0 ? 1 : 0, f1 ? 1 : 0);
    wfm_block_reduce(b, blk, tid, s.cap, f0, f1, mag0, mag1, maps, sums, peaks);
}

// ---- 4. one wave per channel: scan of the block maps (fm_front.hpp)
__global__ __launch_bounds__(64)
void wfm_blockscan_kernel(WfmChan* __restrict__ ch, const WfmBufs* __restrict__ bufs)
{
    wfm_blockscan_body(ch[blockIdx.x], bufs[blockIdx.x]);
}

// ---- 5. per (block, channel): the counter after every sample (scan of the step maps from the block's start state),
// open flags, last-open scan, gated discriminator.  The block's first open sample takes its prevArg from an earlier block
// or from the carried state: left to wfm_fixup_kernel.
__global__ __launch_bounds__(256)
void wfm_demod_kernel(const WfmChan* __restrict__ ch, const WfmBufs* __restrict__ bufs)
{
    __shared__ float args[WFM_H];
    __shared__ WfmClamp wmap[4];
    __shared__ int wmax[4];
    __shared__ int first;
    const int c = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const WfmChan& s = ch[c];
    if (blk >= s.n_blocks) return;
    const WfmBufs b = bufs[c];
    const long j0 = (long)blk * WFM_H + 2 * tid;
    const float2 a2 = *reinterpret_cast<const float2*>(b.arg + j0);
    const uchar2 f2 = *reinterpret_cast<const uchar2*>(b.flag + j0);
    args[2 * tid] = a2.x; args[2 * tid + 1] = a2.y;
    if (tid == 0) first = -1;
    bool open0, open1;
    wfm_open_pair(s, b.blk_state[blk], f2, lane, w, wmap, &open0, &open1);
    const int mine = open1 ? 2 * tid + 1 : (open0 ? 2 * tid : -1);
    const int mincl = wfm_wave_max_scan(mine, lane);
    if (lane == 63) wmax[w] = mincl;
    __syncthreads();
    int prev0 = __shfl_up(mincl, 1, 64);
    if (lane == 0) prev0 = -1;
    for (int q = 0; q < w; q++) prev0 = wfm_last_open(prev0, wmax[q]);
    const int prev1 = open0 ? 2 * tid : prev0;
    const float fm = s.fm_scaling;
    float d0 = 0.0f, d1 = 0.0f;
    if (open0) { if (prev0 >= 0) d0 = wfm_discri(a2.x, args[prev0], fm); else first = 2 * tid; }
    if (open1) { if (prev1 >= 0) d1 = wfm_discri(a2.y, args[prev1], fm); else first = 2 * tid + 1; }
    *reinterpret_cast<float2*>(b.dem + WFM_HIST + j0) = make_float2(d0, d1);
    __syncthreads();
    if (tid == 255) b.blk_last[blk] = wfm_last_open(prev0, mine);
    if (tid == 0) b.blk_first[blk] = first;
}

// ---- 6. one wave per channel: prevArg across blocks -> the first open sample of every block; m_prevArg of the next feed
__global__ __launch_bounds__(64)
void wfm_fixup_kernel(WfmChan* __restrict__ ch, const WfmBufs* __restrict__ bufs)
{
    const int c = blockIdx.x, lane = threadIdx.x;
    WfmChan& s = ch[c];
    const WfmBufs b = bufs[c];
    const int nb = s.n_blocks;
    const float fm = s.fm_scaling;
    float carry = s.prev_arg;
    for (int b0 = 0; b0 < nb; b0 += 64) {
        const int blk = b0 + lane;
        const bool in = blk < nb;
        const int last = in ? b.blk_last[blk] : -1;
        const int incl = wfm_wave_max_scan(last >= 0 ? blk : -1, lane);     // nearest block up to here with an open sample
        int ex = __shfl_up(incl, 1, 64);
        if (lane == 0) ex = -1;
        const int fi = in ? b.blk_first[blk] : -1;
        if (fi >= 0) {
            const float prev = ex >= 0 ? b.arg[(long)ex * WFM_H + b.blk_last[ex]] : carry;
            const long j = (long)blk * WFM_H + fi;
            b.dem[WFM_HIST + j] = wfm_discri(b.arg[j], prev, fm);
        }
        const int tot = __shfl(incl, 63, 64);
        if (tot >= 0) carry = b.arg[(long)tot * WFM_H + b.blk_last[tot]];
    }
    if (lane == 0) s.prev_arg = carry;
}

// ---- 7. the polyphase FIR (fm_front.hpp), then the qint16 conversion
__global__ __launch_bounds__(256)
void wfm_fir_kernel(const WfmChan* __restrict__ ch, const WfmBufs* __restrict__ bufs, const float* __restrict__ taps)
{
    const int c = blockIdx.y;
    const WfmChan& s = ch[c];
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= s.n_out) return;
    const WfmBufs b = bufs[c];
    const float acc = wfm_fir_acc(wfm_fir_taps(s, b.sched[o], taps), s.ntaps, b.dem + WFM_HIST + (int)b.sched[o].x);
    b.audio[o] = (int16_t)sdrx_to_q16(acc * 3276.8f * s.volume);
}

// ---- 8. carry (fm_front.hpp)
__global__ __launch_bounds__(WFM_H)
void wfm_carry_kernel(WfmChan* __restrict__ ch, const WfmBufs* __restrict__ bufs)
{
    wfm_carry_body(ch[blockIdx.x], bufs[blockIdx.x]);
}

} // namespace sdrx
