// NFM demodulator bank kernels: the tail of NFMDemod::feed (plugins/channelrx/demodnfm/nfmdemod.cpp:157-300) with
// m_deltaSquelch and m_ctcssOn off.  The front (NCO, Interpolator::decimate) is the channel back-end's
// (backend_kernels.hpp); these kernels start from its complex resampler output `ci` at the audio rate.
//     demod = phaseDiscriminatorDelta(ci);  magsq = |ci|^2 / 2^30;  m_movingAverage(magsq);  level sums
//     below = (Real) m_movingAverage < level;  m_squelchDelayLine.write(below ? 0 : demod * comp);  counter, cap 2 * gate
//     open (count > gate) and not muted: (qint16)(m_bandpass.filter(readBack(gate)) * volume);  else 0
// Audio is bit-identical to the strict-IEEE scalar reference build: every float expression keeps the reference's operand
// order and the file is compiled with -ffp-contract=off.  nfm_scan.hpp has the cut of the recurrences; DESIGN.md 4.12 the
// kernel table.  The only loop that is serial along time is psum_rows' (demod_psum.hpp): a load, one double add, a store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nfm_tone_scan.hpp"
#include "demod_psum.hpp"
#include "demod_wg.hpp"
#include "dsp_device.hpp"
#include "gfft_kernel.hpp"              // atan2_approx2

namespace sdrx {

struct NfmChan {                        // device resident: config + carried state of one channel
    // --- config
    int gate;                           // m_squelchGate = (rate / 100) * squelch_gate: opening count; the counter's cap is 2 * gate
    int D;                              // nfm_delay(gate): how far back readBack(gate) reaches in the written stream
    float level;                        // m_squelchLevel = (Real) pow(10.0, squelch / 100.0)
    float volume;
    float fm_scaling;                   // (8.0f * rate) / fm_deviation
    float comp;                         // m_discriCompensation
    int mute;
    int bp_off;                         // float offset into the Bandpass tap table (151 per channel)
    // --- state
    int count, sq_open;                 // m_squelchCount, m_squelchOpen
    float prev_arg;                     // PhaseDiscriminators::m_prevArg
    double total;                       // MovingAverageUtil::m_total
    double magsq_sum, magsq_peak;
    long long magsq_count;
    // --- per feed
    int n, n_act;                       // audio samples; open and unmuted ones
    double total_next;                  // written by nfm_psum_kernel, committed by nfm_carry_kernel
    // --- CTCSS (nfm_tone_kernels.hpp).  Every channel carries this state, 440 B, and its row of the tap table has the Lowpass
    // taps and the 32 coefficients whether CTCSS is on or not (ct_n is filled too): measured as no difference in a plain
    // handle's feed.  Without ct_on no kernel reads or writes any of it
    int ct_on, ct_sel, ct_n;            // m_ctcssOn, m_ctcssIndexSelected, CTCSSDetector::N
    int ct_fill, ct_index;              // samplesProcessed, m_ctcssIndex
    int ct_detected, ct_max_index;      // toneDetected, maxPowerIndex of the last completed block
    int sc;                             // m_sampleCount & 7
    int n_act_a, n_ev;                  // per feed: open and unmuted samples (n_act becomes those that pass the tone test); index changes
    long long ct_changes, ct_blocks;    // index changes and completed blocks since create / reset
    float ct_u0[32], ct_u1[32], ct_power[32];
    // --- AF squelch (nfm_af_walk_kernel, nfm_tone_kernels.hpp); af_on 0: none of it is read or written
    int af_on, af_n, af_z;              // m_deltaSquelch, AFSquelch::m_N, audio_rate / 10 (zeroBack's reach)
    int af_sq_count;                    // m_squelchCount of NFMDemod in delta mode (count above is then a copy of it)
    double af_coef[2], af_thr;          // AFSquelch::m_coef, m_threshold
    AfState af;
    AfDelay afq;
};

struct NfmBufs {                        // per channel device pointers (per feed capacity ensured by the host)
    const float2* ci;                   // the front's output of this feed
    const int* n_ptr;                   // its count (device side)
    const float* mhist; float* mhist_next;       // last 32 magsq
    const float* whist; float* whist_next;       // last D delay-line writes
    const float* xhist; float* xhist_next;       // last 300 Bandpass inputs
    float* msq; float* wraw; float* w;  // per sample: magsq, demod * comp, what the delay line was given
    double* dterm; double* tot;         // moving-average terms and totals
    int* aidx;                          // index in the open sequence (-1: closed or muted)
    int* blk_a;                         // per 256 samples: open samples of this feed before them
    float* x;                           // per open sample: the delayed sample the Bandpass is given
    int16_t* audio;
    double* blk_sum; float* blk_peak;   // per 256 samples
    // --- CTCSS channels only
    const float* lhist; float* lhist_next;       // last 300 Lowpass inputs
    int* aidx_a;                        // aidx as nfm_gate_kernel left it (open and unmuted)
    float* xl; float* xa;               // per open sample: demod * comp (the Lowpass input), and x as nfm_gate_kernel left it
    float* ctl;                         // per sample: the Lowpass output where the detector takes one
    float* cs; int* cpos;               // per detector sample: its input, its audio sample position
    int* ev;                            // per sample: the index event (-1: none)
    int* cblk;                          // per detector block ended in this feed: its maxPowerIndex (-1: no power above 0)
    int* ev_at; int* ev_idx;            // per index change: audio sample position, new index
    // --- AF squelch channels only: the reference's containers.  The walk alone touches them, in place, in the lower of the
    // two history sets (af_set0)
    const float* dl; float* dl_next;             // DoubleBufferFIFO's 2 * 24000 entries
    const double* afh; double* afh_next;         // the two MovingAverage<double> histories, 128 entries each
};

constexpr int NFM_OUT_WIN = 256 + AM_BP_HIST;              // Bandpass inputs one block of nfm_out_kernel can touch

// ---- 1. per sample: discriminator, magsq, the moving-average term; per 256 samples the level partials
__global__ __launch_bounds__(256)
void nfm_level_kernel(NfmChan* __restrict__ ch, const NfmBufs* __restrict__ bufs)
{
    __shared__ double sums[256];
    __shared__ float peaks[256];
    const int c = blockIdx.y, tid = threadIdx.x;
    const NfmBufs b = bufs[c];
    const int n = *b.n_ptr;
    if (blockIdx.x == 0 && tid == 0) ch[c].n = n;
    const long i = (long)blockIdx.x * 256 + tid;
    if ((long)blockIdx.x * 256 >= n) return;
    const NfmChan& s = ch[c];
    float m = 0.0f;
    if (i < n) {
        const float2 v = b.ci[i];
        m = nfm_magsq(v.x * v.x + v.y * v.y);
        float old = b.mhist[min(i, (long)NFM_MA - 1)], prev = s.prev_arg;
        if (i >= NFM_MA) { const float2 o = b.ci[i - NFM_MA]; old = nfm_magsq(o.x * o.x + o.y * o.y); }
        if (i > 0) { const float2 p = b.ci[i - 1]; prev = atan2_approx2(p.y, p.x); }
        b.msq[i] = m;
        b.wraw[i] = nfm_demod(atan2_approx2(v.y, v.x), prev, s.fm_scaling) * s.comp;
        b.dterm[i] = am_ma_term(m, old);
    }
    wg_level_reduce(sums, peaks, tid, (double)m, m);
    if (tid == 0) { b.blk_sum[blockIdx.x] = sums[0]; b.blk_peak[blockIdx.x] = peaks[0]; }
}

// ---- 2. the moving-average total after every sample: one wave per 16 channels (psum_rows)
__global__ __launch_bounds__(64)
void nfm_psum_kernel(NfmChan* __restrict__ ch, const NfmBufs* __restrict__ bufs, int n_ch)
{
    psum_channels(n_ch, [&](int c) { return PsumRow{bufs[c].dterm, bufs[c].tot, ch[c].n, ch[c].total, &ch[c].total_next}; });
}

// what the delay line holds for stream index j of this feed (j < 0: the carried history)
__device__ __forceinline__ float nfm_w_at(const NfmBufs& b, int D, float level, long j)
{
    if (j < 0) return b.whist[D + j];
    return nfm_up(b.tot[j], level) ? b.wraw[j] : 0.0f;
}

// ---- 3. one workgroup per channel, 1024 samples per trip: the squelch counter as a scan of clamp maps, the delay-line
// stream, the open flags and their prefix count (the compaction index), the compacted Bandpass inputs; level accumulators
__global__ __launch_bounds__(256)
void nfm_gate_kernel(NfmChan* __restrict__ ch, const NfmBufs* __restrict__ bufs)
{
    __shared__ WfmClamp wmap[4];
    __shared__ int wact[4];
    __shared__ double sums[256];
    __shared__ float peaks[256];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    NfmChan& s = ch[c];
    const NfmBufs b = bufs[c];
    const int n = s.n, gate = s.gate, cap = 2 * s.gate, D = s.D;
    const float level = s.level;
    const bool mute = s.mute != 0;
    const WfmClampOps sq{cap};
    int carry = s.count, nact = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i0 = base + tid * 4;
        bool up[4];
        WfmClamp m = sq.identity();
#pragma unroll
        for (int k = 0; k < 4; k++) {
            up[k] = false;
            if (i0 + k < n) {
                up[k] = nfm_up(b.tot[i0 + k], level);
                m = wfm_compose(m, wfm_step(up[k], cap));
                b.w[i0 + k] = up[k] ? b.wraw[i0 + k] : 0.0f;
            }
        }
        int st = wfm_apply(wg_scan(sq, m, lane, w, wmap), carry);
        bool act[4];
        int a_loc = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            act[k] = false;
            if (i0 + k < n) {
                st = wfm_apply(wfm_step(up[k], cap), st);
                act[k] = nfm_open(st, gate) && !mute;
                a_loc += act[k];
            }
        }
        int a_ex = nact + wg_scan_incl(WgCount{}, a_loc, lane, w, wact) - a_loc;
        if (lane == 0 && i0 < n) b.blk_a[i0 >> 8] = a_ex;   // i0 is a multiple of 256 here
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (i0 + k < n) {
                b.aidx[i0 + k] = act[k] ? a_ex : -1;
                if (act[k]) b.x[a_ex++] = nfm_w_at(b, D, level, (long)(i0 + k) - D);
            }
        }
        carry = wfm_apply(wg_total(sq, wmap), carry);
        nact += wg_total(WgCount{}, wact);
        __syncthreads();                                    // wmap / wact are rewritten by the next trip
    }
    // level accumulators: the 256-sample partials of nfm_level_kernel, in a fixed order
    wg_level_gather(sums, peaks, tid, (n + 255) / 256, b.blk_sum, b.blk_peak);
    if (tid == 0) {
        s.n_act = nact;
        if (n > 0) {
            s.count = carry;
            s.sq_open = nfm_open(carry, gate) ? 1 : 0;
            s.magsq_sum += sums[0];
            if ((double)peaks[0] > s.magsq_peak) s.magsq_peak = (double)peaks[0];
            s.magsq_count += n;
        }
    }
}

// ---- 4. per sample: the Bandpass over the compacted sequence, volume, conversion; closed or muted samples are 0.
// The open samples of a block are consecutive in the compacted sequence: their 256 + 300 inputs and the taps are staged
// in LDS once, lane p then reads [p - k], neighbours in neighbouring banks.
__global__ __launch_bounds__(256)
void nfm_out_kernel(const NfmChan* __restrict__ ch, const NfmBufs* __restrict__ bufs, const float* __restrict__ bp_taps)
{
    __shared__ float taps[AM_BP_H + 1];
    __shared__ float win[NFM_OUT_WIN];
    const int c = blockIdx.y, tid = threadIdx.x;
    const NfmChan& s = ch[c];
    if ((long)blockIdx.x * 256 >= s.n) return;
    const NfmBufs& b = bufs[c];
    const long i = (long)blockIdx.x * 256 + tid;
    const int a = i < s.n ? b.aidx[i] : -1;
    if (__syncthreads_count(a >= 0) == 0) {                 // nothing open in this block
        if (i < s.n) b.audio[i] = 0;
        return;
    }
    const int a0 = b.blk_a[blockIdx.x], n_act = s.n_act;
    for (int k = tid; k <= AM_BP_H; k += 256) taps[k] = bp_taps[s.bp_off + k];
    for (int j = tid; j < NFM_OUT_WIN; j += 256) {
        const long idx = (long)a0 - AM_BP_HIST + j;
        win[j] = idx < n_act ? am_stream_at(b.xhist, AM_BP_HIST, (const float*)b.x, idx) : 0.0f;
    }
    __syncthreads();
    if (i >= s.n) return;
    int q = 0;
    if (a >= 0) {
        const int p = a - a0 + AM_BP_HIST;
        const float y = am_bandpass(taps, [&](int k) { return win[p - k]; });
        q = sdrx_to_q16(y * s.volume);
    }
    b.audio[i] = (int16_t)q;
}

// ---- 5. carry: the histories of the next feed (double-buffered: this feed's are still being read), m_prevArg, the total
__global__ __launch_bounds__(256)
void nfm_carry_kernel(NfmChan* __restrict__ ch, const NfmBufs* __restrict__ bufs)
{
    const int c = blockIdx.x, tid = threadIdx.x;
    NfmChan& s = ch[c];
    const NfmBufs b = bufs[c];
    const int n = s.n;
    if (tid < NFM_MA) b.mhist_next[tid] = am_hist_next(b.mhist, NFM_MA, (const float*)b.msq, n, tid);
    for (int i = tid; i < s.D; i += 256) b.whist_next[i] = am_hist_next(b.whist, s.D, (const float*)b.w, n, i);
    for (int i = tid; i < AM_BP_HIST; i += 256) b.xhist_next[i] = am_hist_next(b.xhist, AM_BP_HIST, (const float*)b.x, s.n_act, i);
    if (tid == 0) {
        s.total = s.total_next;
        if (n > 0) { const float2 v = b.ci[n - 1]; s.prev_arg = atan2_approx2(v.y, v.x); }
    }
}

} // namespace sdrx
